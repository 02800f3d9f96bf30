"""The numpy statements of the sun rules (tests/dsm_sun_oracle.py) against each other, against brute force and against closed
forms; the transposition identity the column-major kernels rest on; what the GPU tests assume of their case matrix; sun_terms;
every Python argument rejection that needs no GPU; and planted errors that the GPU file's comparison must report."""
import math

import numpy as np
import pytest

import dsm_sun_oracle as so
import dsm_sun_scene as sc
from dsm_testkit import scene as _scene
from satmvs_amd import dsm
from satmvs_amd.dsm import DSMGrid

ND = sc.ND


def _differs(got, want):
    """Whether the GPU file's comparison (dsm_sun_scene.compare) reports a difference."""
    try:
        sc.compare(got, want, "planted")
    except AssertionError:
        return True
    return False


# ---- the rule, three times -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u", sc.DIRECTIONS)
def test_the_statements_agree(u):
    for shape, seed in (((1, 1), 1), ((1, 9), 2), ((11, 1), 3), ((2, 2), 4), ((13, 17), 5), ((35, 9), 6), ((8, 37), 7)):
        z = sc.special(shape, seed)
        for ab, tol in ((sc.terms(*u), 0.1), ((0.0, 0.0), 0.0)):
            loop = so.shadow_loop(z, ND, *u, *ab, tol)
            sc.compare(so.shadow_scan(z, ND, *u, *ab, tol), loop, (u, shape, "scan"))
            sc.compare(so.shadow_brute(z, ND, *u, *ab, tol), loop, (u, shape, "brute"))


def test_random_directions_and_grids():
    rng = np.random.default_rng(10)
    for i in range(60):
        shape = (int(rng.integers(1, 40)), int(rng.integers(1, 40)))
        az, el = rng.uniform(0.0, 360.0), rng.uniform(5.0, 80.0)
        t = dsm.sun_terms(DSMGrid(0.0, 0.0, rng.uniform(1.0, 9.0), rng.uniform(1.0, 9.0), shape[1], shape[0]), az, el)
        z = sc.special(shape, 20 + i, extremes=False)
        sc.compare(so.shadow_scan(z, ND, *t, 0.1), so.shadow_loop(z, ND, *t, 0.1), (shape, az, el))


@pytest.mark.parametrize("u", [u for u in sc.DIRECTIONS if abs(u[0]) != abs(u[1])])
def test_the_transposition_identity(u):
    """The rule on the transposed grid with (ucol, urow) and (a, b) swapped gives the transposed result, bit for bit -- stated
    with the loop, which does not transpose anything itself.  (A tie is row-major on both grids, so the two sides would walk
    different lines; the kernels never transpose a tie.)"""
    z = sc.special((19, 27), 30)
    a, b = sc.terms(*u)
    shade, depth = so.shadow_loop(z, ND, u[0], u[1], a, b, 0.1)
    shade_t, depth_t = so.shadow_loop(np.ascontiguousarray(z.T), ND, u[1], u[0], b, a, 0.1)
    sc.compare((np.ascontiguousarray(shade_t.T), np.ascontiguousarray(depth_t.T)), (shade, depth), u)


def test_lines_by_hand():
    row_major, s, asc = so.lines(5, 9, 0.5, -1.0)             # m = -0.5: floor(-0.5 r + 0.5)
    assert row_major and asc and s.tolist() == [0, 0, -1, -1, -2]
    row_major, s, asc = so.lines(5, 4, 1.0, 0.5)              # column-major, m = 0.5, the sun in the east: descending c
    assert not row_major and not asc and s.tolist() == [0, 1, 1, 2]
    assert so.lines(3, 3, 1.0, -1.0)[0] and so.lines(3, 3, -1.0, 1.0)[0]                    # ties are row-major
    assert so.lines(50, 3, 1e-18, -1.0)[1].tolist() == [0] * 50
    z = np.array([[5.0, 0.0, 0.0, 0.0]], np.float32)          # the sun in the west at 45 degrees over 1 m cells: a = -1
    shade, depth = so.shadow_scan(z, ND, -1.0, 0.0, -1.0, 0.0, 0.1)
    assert shade.tolist() == [[1, 2, 2, 2]] and depth[0, 1:].tolist() == [4.0, 3.0, 2.0] and depth[0, 0] == -np.inf
    shade, _ = so.shadow_scan(z, ND, -1.0, 0.0, -2.0, 0.0, 0.1)                             # steeper: g = z + 2 c
    assert shade.tolist() == [[1, 2, 2, 1]]


def test_zeros_and_voids():
    z = np.array([[-0.0, 0.0, -0.0, np.nan, 0.0]], np.float32)
    for fn in (so.shadow_loop, so.shadow_scan, so.shadow_brute):
        shade, depth = fn(z, ND, -1.0, 0.0, 0.0, 0.0, 0.0)   # g = z - 0.0: -0.0, +0.0, -0.0, -, +0.0; the maximum keeps +0.0
        assert shade.tolist() == [[1, 1, 1, 0, 1]]
        assert depth[0, 0] == -np.inf and depth[0, 3] == ND
        assert [bool(np.signbit(v)) for v in depth[0, [1, 2, 4]]] == [True, False, False]   # -0 - +0, +0 - -0, +0 - +0


# ---- closed forms ----------------------------------------------------------------------------------------------------------------
BOX = dict(r0=37, r1=42, c0=36, c1=43, height=30.0, res=5.0)                 # 30 m high, 30 m x 40 m, on an 80 x 80 grid of 5 m


@pytest.mark.parametrize("elevation", [20.0, 30.0, 45.0])
def test_box_on_a_plane(elevation):
    """No cell farther than 1.5 cells outside the swept footprint is shadowed, none farther than 1.5 cells inside is lit: a line
    stays within one cell of the ray across it (both s(i) - m i lie in (-1/2, 1/2]) and the swept polygon is that of the cell
    centres, half a cell inside the cells' outline."""
    grid = DSMGrid(0.0, 0.0, BOX["res"], BOX["res"], 80, 80)
    z = so.box_on_plane(80, 80, BOX["r0"], BOX["r1"], BOX["c0"], BOX["c1"], BOX["height"])
    for azimuth in np.arange(14) * (360.0 / 14.0) + 3.0:
        shade, _ = so.shadow_scan(z, ND, *dsm.sun_terms(grid, azimuth, elevation), 0.1)
        out, lit, n_inside = so.box_violations(shade, azimuth=azimuth, elevation=elevation, **BOX)
        assert (out, lit) == (0, 0) and n_inside > 0, (azimuth, elevation, out, lit, n_inside)


def test_polygon_distance():
    square = so._hull([(0.0, 0.0), (4.0, 0.0), (4.0, 4.0), (0.0, 4.0), (2.0, 2.0)])
    assert len(square) == 4
    x, y = np.array([2.0, 5.0, 7.0, 0.0]), np.array([2.0, 2.0, 8.0, 1.0])
    assert np.allclose(so.signed_distance(square, x, y), [-2.0, 1.0, 5.0, 0.0])


def test_terrain_casts_no_shadow_above_its_steepest_slope():
    c, r = np.meshgrid(np.arange(120), np.arange(100))
    E, N = 500000.0 + 5.0 * c, 4000000.0 - 5.0 * r
    grid = DSMGrid(500000.0, 4000000.0, 5.0, 5.0, 120, 100)
    z = _scene(E, N, blocks=False, holes=False)
    assert math.hypot(20.0 / 53.0, 20.0 / 71.0) < math.tan(math.radians(30.0))           # a bound of the scene's steepest slope
    for azimuth in (0.0, 77.0, 180.0, 250.0):
        assert not (so.shadow_scan(z, ND, *dsm.sun_terms(grid, azimuth, 30.0), 0.1)[0] == 2).any()
    assert (so.shadow_scan(_scene(E, N, holes=False), ND, *dsm.sun_terms(grid, 135.0, 30.0), 0.1)[0] == 2).any()


# ---- gradient and hillshade --------------------------------------------------------------------------------------------------------
def test_gradient_statement():
    r, c = np.mgrid[0:9, 0:11].astype(np.float64)
    z = (3.0 + 0.5 * c * 5.0 - 0.25 * (-r * 4.0)).astype(np.float32)          # rises 0.5 m/m eastwards, falls 0.25 m/m northwards
    de, dn = so.gradient(z, ND, 5.0, 4.0)
    assert np.all(de[1:-1, 1:-1] == np.float32(0.5)) and np.all(dn[1:-1, 1:-1] == np.float32(-0.25))
    assert np.all(de[1:-1, 0] == np.float32(0.25)) and np.all(dn[0, 1:-1] == np.float32(-0.125))       # a border: half the difference
    z[4, 5] = np.nan
    de, dn = so.gradient(z, ND, 5.0, 4.0)
    assert de[4, 5] == ND and dn[4, 5] == ND and de[4, 4] == np.float32((2.0 * (z[4, 4] - z[4, 3]) + 2.0 * 5.0) / 40.0)
    one = so.gradient(np.array([[7.0]], np.float32), ND, 5.0, 5.0)
    assert one[0][0, 0] == 0.0 and one[1][0, 0] == 0.0
    flat = so.cos_incidence(np.zeros(3), np.zeros(3), 315.0, 45.0)
    assert np.allclose(flat, math.sin(math.radians(45.0)))
    facing = so.cos_incidence(np.array([-1.0]), np.array([0.0]), 90.0, 45.0)      # falls eastwards at 45 degrees, the sun in the east
    assert np.allclose(facing, 1.0) and so.cos_incidence(np.array([1.0]), np.array([0.0]), 90.0, 44.0)[0] == 0.0


# ---- what the GPU tests assume of their matrix ---------------------------------------------------------------------------------
def test_the_matrix_straddles_the_constants():
    B, T, K = sc.BAND, sc.TILE, sc.BLOCK
    assert {s[0] for s in sc.BANDS_ROWS} == {B - 1, B, B + 1, 2 * B + 1} == {s[1] for s in sc.BANDS_COLS}
    assert [s[1] + B + 1 for s in sc.SLOTS] == [K - 1, K, K + 1]
    assert [sc.line_count(*s, 0.0, -1.0) for s in sc.LINES_FLAT] == [K - 1, K, K + 1]
    assert [sc.line_count(*s, 1.0, -1.0) for s in sc.LINES_DIAG] == [K - 1, K, K + 1]
    assert {s[0] for s in sc.TILES} == {T - 1, T, T + 1} == {s[1] for s in sc.TILES}
    majors = {(abs(u[1]) >= abs(u[0]), (u[1] if abs(u[1]) >= abs(u[0]) else u[0]) < 0) for u in sc.MAJORS}
    assert len(majors) == 4                                   # both majors, both scan orders
    ms = {(u[0] / u[1] if abs(u[1]) >= abs(u[0]) else u[1] / u[0]) for u in sc.DIRECTIONS}
    assert {0.0, 1.0, -1.0, 0.5, -0.5, 1.0 / 3.0, -1.0 / 3.0, 1e-18, -1e-18} <= ms
    for shape in sc.LARGE:
        assert min(shape) > sc.BLOCK and max(shape) > 8 * sc.BLOCK and max(shape) > 64 * B and shape[0] * shape[1] <= 2300 * 300
    names = [c[0] for g in sc.GROUPS for c in sc.matrix(g)]
    assert len(names) == len(set(names)) > 200
    for g in sc.GROUPS:
        for name, z, nodata, u, ab, tol in sc.matrix(g):
            assert z.dtype == np.float32 and z.ndim == 2 and tol >= 0.0, name
    kinds = sc.special((67, 130), 100)
    assert np.isnan(kinds).any() and np.isinf(kinds).any() and (kinds == ND).any() and (np.abs(kinds) == sc.FLT_MAX).any()
    assert np.signbit(kinds[kinds == 0]).any() and not np.signbit(kinds[kinds == 0]).all()


def test_the_tol_pairs_sit_at_the_tie_and_one_ulp_above():
    z, nodata, u, ab, tol = sc.tol_pairs()
    g = so.keys(z, *ab)
    assert np.array_equal(g, z.astype(np.float64))            # a = b = 0: g = z exactly
    assert g[0, 0] - g[1, 0] == tol and g[0, 1] - g[1, 1] == np.nextafter(tol, 2.0)
    shade, depth = so.shadow_loop(z, nodata, *u, *ab, tol)
    assert shade.tolist() == [[1, 1], [1, 2]] and depth[1].tolist() == [1.0, 1.0]


# ---- the Python layer without a GPU ----------------------------------------------------------------------------------------------
def test_sun_terms_for_the_cardinal_azimuths():
    grid = DSMGrid(0.0, 0.0, 5.0, 2.0, 8, 8)
    k = math.tan(math.radians(45.0))
    for azimuth, towards in ((0.0, (0, -1)), (90.0, (1, 0)), (180.0, (0, 1)), (270.0, (-1, 0)), (-90.0, (-1, 0)), (450.0, (1, 0))):
        ucol, urow, a, b = dsm.sun_terms(grid, azimuth, 45.0)
        assert np.allclose([ucol * 5.0, urow * 2.0], towards, atol=1e-15), azimuth
        assert np.allclose([a, b], [k * 5.0 * towards[0], k * 2.0 * towards[1]], atol=1e-14), azimuth
        row_major = so.lines(8, 8, ucol, urow)[0]
        assert row_major == (towards[0] == 0), azimuth        # 1e-16 of the other component does not change the major
    ucol, urow, a, b = dsm.sun_terms(grid, 33.0, 20.0)
    sA, cA, k = math.sin(math.radians(33.0)), math.cos(math.radians(33.0)), math.tan(math.radians(20.0))
    assert (ucol, urow, a, b) == (sA / 5.0, -cA / 2.0, k * 5.0 * sA, -k * 2.0 * cA)


def test_python_rejections():
    g = DSMGrid(0.0, 0.0, 5.0, 5.0, 6, 4)
    z = np.zeros((4, 6), np.float32)
    for bad in (0.0, 90.0, -5.0, 120.0, float("nan")):
        with pytest.raises(ValueError, match="elevation"):
            dsm.cast_shadows(z, g, 10.0, bad)
        with pytest.raises(ValueError, match="elevation"):
            dsm.hillshade(z, g, elevation=bad)
        with pytest.raises(ValueError, match="elevation"):
            dsm.sun_exposure(z, g, [(10.0, 30.0), (20.0, bad)])
        with pytest.raises(ValueError, match="elevation"):
            dsm.sun_terms(g, 0.0, bad)
    for bad in (float("inf"), float("nan")):
        with pytest.raises(ValueError, match="azimuth"):
            dsm.cast_shadows(z, g, bad, 30.0)
        with pytest.raises(ValueError, match="azimuth"):
            dsm.hillshade(z, g, azimuth=bad)
    for bad in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="tol"):
            dsm.cast_shadows(z, g, 10.0, 30.0, tol=bad)
        with pytest.raises(ValueError, match="tol"):
            dsm.hillshade(z, g, shadows=True, tol=bad)
        with pytest.raises(ValueError, match="tol"):
            dsm.sun_exposure(z, g, [(10.0, 30.0)], tol=bad)
    wrong = np.zeros((3, 3), np.float32)
    for fn in (lambda: dsm.cast_shadows(wrong, g, 10.0, 30.0), lambda: dsm.gradient(wrong, g), lambda: dsm.slope(wrong, g),
               lambda: dsm.aspect(wrong, g), lambda: dsm.hillshade(wrong, g), lambda: dsm.sun_exposure(wrong, g, [(10.0, 30.0)])):
        with pytest.raises(ValueError, match="shape"):
            fn()
    flat = DSMGrid(0.0, 0.0, 0.0, 5.0, 6, 4)
    for fn in (lambda: dsm.cast_shadows(z, flat, 10.0, 30.0), lambda: dsm.gradient(z, flat), lambda: dsm.hillshade(z, flat),
               lambda: dsm.sun_terms(flat, 10.0, 30.0), lambda: dsm.sun_exposure(z, flat, [(10.0, 30.0)])):
        with pytest.raises(ValueError, match="resolution"):
            fn()
    with pytest.raises(ValueError, match="at least one sun"):
        dsm.sun_exposure(z, g, [])
    with pytest.raises(ValueError, match="pairs"):
        dsm.sun_exposure(z, g, [10.0, 30.0])
    with pytest.raises(ValueError, match="one weight per sun"):
        dsm.sun_exposure(z, g, [(10.0, 30.0)], weights=[1.0, 2.0])
    with pytest.raises(ValueError, match="weight"):
        dsm.sun_exposure(z, g, [(10.0, 30.0)], weights=[float("nan")])


# ---- planted errors: the comparison of the GPU file has to report each ---------------------------------------------------------
@pytest.mark.parametrize("plant", ["inclusive", "rint", "no carry", "order", "invalid occlude"])
def test_planted_errors_are_reported(plant):
    z = sc.relief((2 * sc.BAND + 9, 40), 40)
    z[0, :] = ND                                              # the row nearest the sun is void: what occludes if voids do
    u = (0.5, -1.0)                                           # halves in s: rint and floor(x + 0.5) part at every other row
    a, b = sc.terms(*u)
    good = so.shadow_loop(z, ND, *u, a, b, 0.1)
    assert not _differs(so.shadow_scan(z, ND, *u, a, b, 0.1), good)
    bad = so.shadow_loop(z, ND, *u, a, b, 0.1, plant=plant, band=sc.BAND)
    assert _differs(bad, good), plant
    if plant in ("no carry", "order", "rint"):
        assert not np.array_equal(bad[0], good[0]), plant    # the shade map alone shows these
