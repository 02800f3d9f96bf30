"""The facet rule without a device: the two statements of the labelling against each other on the case matrix, closed forms,
invariants, the plane against numpy's least squares, every argument rejection of the Python layer and of the C entries (they
come before any HIP call), and planted errors that `differing` reports."""
import numpy as np
import pytest

import dsm_facet_oracle as fo
import dsm_facet_scene as fs

ND = fs.ND
MATRIX = fs.matrix()


def _partition(labels):
    """A label map up to numbering: the first cell of every cell's facet."""
    flat = labels.ravel()
    first = np.full(int(flat.max()) + 1, -1, np.int64)
    idx = np.arange(flat.size)[::-1]
    first[flat[::-1]] = idx
    out = first[flat]
    out[flat == 0] = -1
    return out.reshape(labels.shape)


# ---- the two statements ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MATRIX, ids=[c[0] for c in MATRIX])
def test_the_two_statements_agree(case):
    name, z, T, Ax, Ay = case
    for conn in (4, 8):
        for grow in (False, True):
            a, na = fo.facets(z, T, Ax, Ay, conn, grow, statement="loop")
            b, nb = fo.facets(z, T, Ax, Ay, conn, grow, statement="graph")
            assert na == nb and fo.differing(a, b) is None, (name, conn, grow, na, nb, fo.differing(a, b))
            assert a.dtype == np.int32 and set(np.unique(a[a > 0]).tolist()) <= set(range(1, na + 1))
            if not grow:
                assert len(np.unique(a[a > 0])) == na
                firsts = [int(np.flatnonzero(a.ravel() == k)[0]) for k in range(1, na + 1)]
                assert firsts == sorted(firsts)                  # raster order of the first planar cells


def test_the_roof_scene_meets_its_answer():
    for seed in (None, 1):
        z, faces = fs.roof_scene(seed)
        for tol, slope_tol in ((0.25, 0.1), (0.5, 0.2)):
            labels, n = fo.facets(z, *fo.terms(fs.RES, fs.RES, tol, slope_tol))
            fs.check_roof_answer(labels, n, faces)


# ---- closed forms ----------------------------------------------------------------------------------------------------------------
def test_a_quantised_plane_is_one_facet_with_its_exact_plane():
    gh, gw, a, b, q0 = 19, 23, 3, -2, 1000
    z = fs.quantised_plane(gh, gw, a, b, q0)
    labels, n = fo.facets(z, 0, 0, 0)
    assert n == 1 and (labels == 1).all()
    inner, n = fo.facets(z, 0, 0, 0, grow=False)
    assert n == 1 and (inner[1:-1, 1:-1] == 1).all() and inner.sum() == (gh - 2) * (gw - 2)
    Gx, Gy, planar = fo.normals(z, 0)
    assert (Gx[1:-1, 1:-1] == 8 * a).all() and (Gy[1:-1, 1:-1] == 8 * b).all() and Gx[0].sum() == 0 and planar.sum() == (gh - 2) * (gw - 2)
    p = fo.planes(labels, 1, z)
    cb, rb = (gw - 1) // 2, (gh - 1) // 2
    assert p["sums"][0].tolist()[:3] == [gh * gw, gh * gw * (gw - 1) // 2, gw * gh * (gh - 1) // 2]
    assert p["centre"][0].tolist()[:2] == [cb, rb]
    assert p["plane"][0, 0] == a and p["plane"][0, 1] == b and p["plane"][0, 2] == q0 + a * cb + b * rb
    assert p["sse"][0] == 0 and p["max_abs"][0] == 0


def test_a_gable_is_two_facets():
    """8 x 12 cells, the ridge between rows 3 and 4.  Rows 1, 2 and 5, 6 are planar (without the first and last column); rows 3
    and 4 see both faces in their windows and are not, so no link crosses the ridge.  Growth gives every face its rim back: a
    rim cell lies on its own face's plane exactly and at least T + 1 off the other's."""
    h, w, s = 8, 12, 2.0
    r = np.arange(h, dtype=np.float64)[:, None] * np.ones((1, w))
    z = (50.0 + s * np.minimum(r + 0.5, h - r - 0.5)).astype(np.float32)
    T, Ax, Ay = fo.terms(5.0, 5.0)
    labels, n = fo.facets(z, T, Ax, Ay)
    assert n == 2 and (labels[:4] == 1).all() and (labels[4:] == 2).all()
    core, n = fo.facets(z, T, Ax, Ay, grow=False)
    want = np.zeros((h, w), np.int32)
    want[1:3, 1:-1], want[5:7, 1:-1] = 1, 2
    assert n == 2 and fo.differing(core, want) is None
    p = fo.planes(labels, 2, z)
    assert p["plane"][:, 0].tolist() == [0.0, 0.0] and p["plane"][:, 1].tolist() == [512.0, -512.0] and p["sse"].tolist() == [0, 0]


def test_the_smallest_grids():
    z = fs.quantised_plane(3, 3)
    labels, n = fo.facets(z, 0, 0, 0)
    assert n == 1 and (labels == 1).all()
    core, n = fo.facets(z, 0, 0, 0, grow=False)
    assert n == 1 and core.sum() == 1 and core[1, 1] == 1
    for shape in ((1, 1), (1, 9), (9, 1), (2, 2), (2, 7)):
        labels, n = fo.facets(fs.quantised_plane(*shape), 5, 5, 5)
        assert n == 0 and not labels.any(), shape


def _pair(q, gx, planar=(True, True)):
    """Two cells side by side with given heights and Gx, Gy = 0: the link alone."""
    return (np.array([q], np.int64), np.array([gx], np.int64), np.zeros((1, 2), np.int64), np.array([planar], bool))


@pytest.mark.parametrize("label", [fo.label_loop, fo.label_graph])
def test_the_link_at_its_thresholds(label):
    T, A = 7, 16
    assert label(*_pair([100, 100 + T], [0, 0]), T, A, A, 4)[1] == 1              # a step of exactly T links
    assert label(*_pair([100, 100 + T + 1], [0, 0]), T, A, A, 4)[1] == 2          # T + 1 does not
    assert label(*_pair([100 - T, 100], [0, 0]), T, A, A, 4)[1] == 1
    assert label(*_pair([100, 101], [0, A]), T, A, A, 4)[1] == 1                  # a gradient difference of exactly Ax; the step fits
    assert label(*_pair([100, 101], [0, A + 1]), T, A, A, 4)[1] == 2              # Ax + 1
    assert label(*_pair([100, 101], [A, 0]), T, A, A, 4)[1] == 1                  # symmetric
    q, gx, gy, pl = _pair([100, 100], [0, 0])
    assert label(q.T.copy(), gx.T.copy(), np.array([[0], [A]], np.int64), pl.T.copy(), T, 0, A, 4)[1] == 1       # Ay along rows
    assert label(q.T.copy(), gx.T.copy(), np.array([[0], [A + 1]], np.int64), pl.T.copy(), T, 0, A, 4)[1] == 2
    assert label(*_pair([100, 100], [0, 0], (True, False)), T, A, A, 4)[1] == 1   # a cell that is not planar links nothing


def test_collinear_cells_have_no_plane():
    gh = gw = 60
    z = fs.roof_scene(seed=1)[0][:gh, :gw]
    labels = np.zeros((gh, gw), np.int32)
    labels[1, 3:30] = 1                                      # a row
    labels[7:33, 58] = 2                                     # a column
    d = np.arange(20)
    labels[3 + d, 3 + d] = 3                                 # a diagonal
    labels[55 - d[:13], 3 + d[:13]] = 4                      # an anti-diagonal of odd length
    labels[55 - d[:12], 25 + d[:12]] = 5                     # and of even length: dr = 1 - dc
    labels[0, 0] = 6                                         # one cell
    labels[58, 40] = labels[59, 41] = 7                      # two cells
    labels[30:33, 40:42] = 8                                 # six cells in general position
    p = fo.planes(labels, 9, z)
    assert np.isnan(p["plane"][[0, 1, 2, 3, 4, 5, 6, 8]]).all() and np.isfinite(p["plane"][7]).all()
    assert p["sums"][:, 0].tolist() == [27, 26, 20, 13, 12, 1, 2, 6, 0] and p["sse"][[0, 8]].tolist() == [0, 0]


def test_a_void_in_a_face():
    z = fs.quantised_plane(12, 14)
    z[6, 7] = np.nan
    labels, n = fo.facets(z, 0, 0, 0)
    assert n == 1 and labels[6, 7] == 0 and (labels == 1).sum() == 12 * 14 - 1
    core, _ = fo.facets(z, 0, 0, 0, grow=False)
    assert not core[5:8, 6:9].any() and (core[1:-1, 1:-1] == 1).sum() == 10 * 12 - 9


# ---- invariants ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MATRIX, ids=[c[0] for c in MATRIX])
def test_transposition_swaps_the_axes(case):
    name, z, T, Ax, Ay = case
    for conn in (4, 8):
        a, na = fo.facets(z, T, Ax, Ay, conn, grow=False)
        b, nb = fo.facets(np.ascontiguousarray(z.T), T, Ay, Ax, conn, grow=False)
        assert na == nb and np.array_equal(_partition(a) >= 0, _partition(b).T >= 0)
        pa, pb = _partition(a), _partition(np.ascontiguousarray(b.T))
        pairs = np.unique(np.stack([pa.ravel(), pb.ravel()]), axis=1)        # a bijection between the two sets of facets
        assert pairs.shape[1] == len(np.unique(pa)) == len(np.unique(pb)), name


@pytest.mark.parametrize("case", MATRIX, ids=[c[0] for c in MATRIX])
def test_a_larger_tolerance_never_splits_a_facet(case):
    name, z, T, Ax, Ay = case
    fine, nf = fo.facets(z, T, Ax, Ay, grow=False)
    coarse, _ = fo.facets(z, 2 * T + 3, Ax, Ay, grow=False)
    for k in range(1, nf + 1):
        on = np.unique(coarse[fine == k])
        assert len(on) == 1 and on[0] > 0, (name, k)


@pytest.mark.parametrize("case", MATRIX, ids=[c[0] for c in MATRIX])
def test_a_mask_equals_voiding_the_cells_outside(case):
    name, z, T, Ax, Ay = case
    mask = fs.random_mask(*z.shape, seed=11)
    voided = np.where(mask != 0, z, ND)
    for grow in (False, True):
        a, na = fo.facets(z, T, Ax, Ay, grow=grow, mask=mask)
        b, nb = fo.facets(voided, T, Ax, Ay, grow=grow)
        assert na == nb and fo.differing(a, b) is None and not a[mask == 0].any(), name


def test_the_plane_against_least_squares():
    """The plane from the integer moments against numpy's least squares on the centred coordinates.  The moments are exact and
    below 2^53 here, so the centred second moments carry a few roundings each (relative 4 eps of their terms, which cancel by at
    most the factor N Sxx / (N Sxx - Sx^2) <= 2 about an integer centre); Cramer's rule on the 2 x 2 system C then loses at most
    cond(C): |da|, |db| <= 64 eps cond(C) |(a, b)|.  lstsq works on the n x 3 matrix, whose condition is sqrt(cond) of its normal
    matrix, and is allowed the same.  h0 follows from a, b and the means."""
    z, _ = fs.roof_scene(seed=1)
    labels, n = fo.facets(z, *fo.terms(fs.RES, fs.RES))
    p = fo.planes(labels, n, z)
    q, ok = fo.quantise(z)
    eps = np.finfo(np.float64).eps
    for k in range(n):
        assert np.abs(p["moments"][k]).max() < 2 ** 53
        r, c = np.nonzero((labels == k + 1) & ok)
        cb, rb, qb = p["centre"][k]
        A = np.stack([c - cb, r - rb, np.ones(len(r))], axis=1).astype(np.float64)
        sol = np.linalg.lstsq(A, (q[r, c] - qb).astype(np.float64), rcond=None)[0]
        a, b, h0 = p["plane"][k]
        N = float(len(r))
        Sx, Sy, _, Sxx, Sxy, Syy, _, _ = (float(v) for v in p["moments"][k])
        Cm = np.array([[Sxx - Sx * Sx / N, Sxy - Sx * Sy / N], [Sxy - Sx * Sy / N, Syy - Sy * Sy / N]])
        bound = 64.0 * eps * np.linalg.cond(Cm) * max(np.hypot(a, b), 1.0)
        assert abs(a - sol[0]) <= bound and abs(b - sol[1]) <= bound, (k, a - sol[0], b - sol[1], bound)
        assert abs(h0 - (qb + sol[2])) <= 64.0 * eps * (abs(h0) + 1.0) + bound * (abs(Sx / N) + abs(Sy / N) + 1.0), k
        assert p["max_abs"][k] <= 64 * 3 or k == int(labels[0, 0]) - 1           # a roof face lies within its noise; the terrain is curved


# ---- planted errors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", fo.VARIANTS)
def test_differing_reports_a_planted_error(variant):
    """<  for <= in the link; the step test with one cell's gradient only; growth taking the last k; growth in two rounds; rint
    half away from zero in q; rows growing northwards in Gy."""
    assert len(fo.VARIANTS) >= 6
    found = []
    for name, z, T, Ax, Ay in MATRIX:
        want, _ = fo.facets(z, T, Ax, Ay)
        got, _ = fo.facets(z, T, Ax, Ay, variant=variant)
        d = fo.differing(got, want)
        if d is not None:
            assert "the first at" in d
            found.append(name)
    # The link alone, on arrays no DSM gives: between two PLANAR cells the step test is the difference of their two planarity
    # residuals towards each other, so it holds whenever both are planar and its asymmetric form hides behind planarity too.
    pair = _pair([100, 101], [0, 16])
    want, _ = fo.label_loop(*pair, 0, 16, 16, 4)
    got, _ = fo.label_loop(*pair, 0, 16, 16, 4, variant=variant)
    assert want.tolist() == [[1, 1]]
    if fo.differing(got, want) is not None:
        found.append("pair")
    assert ("pair" in found) == (variant in ("lt", "asym"))
    assert found, variant
    assert fo.differing(want, want.copy()) is None
    assert "shape" in fo.differing(want[1:], want) and fo.differing(np.array([np.nan, 0.0]), np.array([np.nan, -0.0])) is not None


# ---- argument rejections -------------------------------------------------------------------------------------------------------------
def test_python_argument_rejections():
    from satmvs_amd import dsm
    grid = dsm.DSMGrid(0.0, 0.0, 5.0, 2.5, 8, 6)
    z = np.zeros((6, 8), np.float32)
    lab = np.zeros((6, 8), np.int32)
    assert dsm.facet_terms(grid) == (64, 1024, 512) and dsm.facet_terms(grid, 0.0, 0.0) == (0, 0, 0)
    assert dsm.facet_terms(grid, 0.25, 0.1) == fo.terms(5.0, 2.5)
    for kw in ({"tol": -1.0}, {"tol": float("nan")}, {"slope_tol": -0.1}, {"slope_tol": float("inf")}, {"tol": 2.0 ** 19}, {"slope_tol": 1e5}):
        with pytest.raises(ValueError):
            dsm.facet_terms(grid, **kw)
    with pytest.raises(ValueError):
        dsm.facet_terms(dsm.DSMGrid(0.0, 0.0, 0.0, 5.0, 8, 6))
    for bad in (z.astype(np.float64), z[0], np.zeros((0, 4), np.float32)):
        with pytest.raises(ValueError):
            dsm.facets(bad, grid)
        with pytest.raises(ValueError):
            dsm.local_planes(bad)
        with pytest.raises(ValueError):
            dsm.facet_planes(lab, 1, bad)
    with pytest.raises(ValueError, match="differs from the grid"):
        dsm.facets(z[:5], grid)
    for conn in (6, True, 8.0, "8"):
        with pytest.raises(ValueError, match="connectivity"):
            dsm.facets(z, grid, connectivity=conn)
    for mask in (np.zeros((6, 8), np.float32), np.zeros((6, 7), np.uint8), np.zeros(8, bool)):
        with pytest.raises(ValueError, match="mask"):
            dsm.facets(z, grid, mask=mask)
        with pytest.raises(ValueError, match="mask"):
            dsm.local_planes(z, mask=mask)
    with pytest.raises(ValueError, match="tol"):
        dsm.local_planes(z, tol=-0.5)
    for n in (-1, 2 ** 31, 1.0, True):
        with pytest.raises(ValueError, match="n must be"):
            dsm.facet_planes(lab, n, z)
    with pytest.raises(ValueError, match="int32"):
        dsm.facet_planes(lab.astype(np.int64), 1, z)
    with pytest.raises(ValueError, match="differs from the labels"):
        dsm.facet_planes(lab, 1, z[:5])
    with pytest.raises(ValueError, match="2\\^24"):
        dsm.facet_planes(np.zeros((4096, 4096), np.int32), 1, np.zeros((4096, 4096), np.float32))
    with pytest.raises(ValueError, match="32768"):
        dsm.facet_planes(np.zeros((1, 32769), np.int32), 1, np.zeros((1, 32769), np.float32))
    with pytest.raises(ValueError, match="differs from the grid"):
        dsm.facet_planes(lab, 1, z, grid=dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, 9, 6))
    for kw in ({"facet_min_area_m2": -1.0}, {"max_rms": -1.0}, {"max_rms": float("nan")}, {"tol": -1.0}):
        with pytest.raises(ValueError):
            dsm.extract_roofs(z, z, grid, **kw)


@pytest.fixture(scope="module")
def lib():
    from satmvs_amd import _lib, build
    build.build()
    return _lib.load()


def test_c_argument_rejections(lib):
    """Every rejection of the three entries and of the size query comes before any HIP call, so it shows without a device."""
    fs.check_c_rejections(lib)
