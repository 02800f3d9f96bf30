"""Ground extraction, the parts that run without a GPU: the numpy oracle (tests/dsm_morph_oracle.py) against its per-cell
formulation bit for bit and against scipy.ndimage as an independent statement, the properties the rules promise, the
schedule, the known-answer scene with its 99 % condition, and the argument checks of smvs_dsm_morph / smvs_dsm_ground
(rejected before any HIP call) and of the Python functions (before any device work)."""
import ctypes as C

import numpy as np
import pytest

import dsm_morph_oracle as mo
from dsm_testkit import lib  # noqa: F401  (fixtures)

ND = np.float32(-999.0)


# ---- the oracle against itself and against scipy -------------------------------------------------------------------------------
def test_keys_order_like_floats_with_minus_zero_below_plus_zero():
    v = np.array([-np.inf, -3.5, -1e-40, -0.0, 0.0, 1e-40, 2.0, np.inf], np.float32)
    k = mo.f2key(v)
    assert (np.diff(k.astype(np.int64)) > 0).all() and mo.same_bits(mo.key2f(k), v)
    assert (k != 0).all() and (k != 0xffffffff).all()                      # 0 is free for "none", and so is its complement


@pytest.mark.parametrize("shape,seed", [((1, 1), 0), ((1, 17), 1), ((13, 2), 2), ((19, 23), 3), ((24, 31), 4)])
def test_oracle_equals_the_per_cell_formulation(shape, seed):
    z = mo.scene(*shape, seed=seed, voids=0.25)
    for nodata in (-999.0, float("nan")):
        for radius in (1, 2, 5) + ((40,) if z.size <= 450 and nodata == -999.0 else ()):      # 40: wider than the grid
            for op in mo.OPS:
                a, b = mo.morph(z, radius, op, nodata), mo.morph_brute(z, radius, op, nodata)
                assert mo.same_bits(a, b), (op, radius, nodata)
    for radii, thresholds in (([1], [0.5]), ([1, 2, 4], [1.5, 4.5, 6.0]), ([2, 3, 7], [0.0, 2.0, 2.0])):
        a, ca = mo.ground(z, radii, thresholds)
        b, cb = mo.ground_brute(z, radii, thresholds)
        assert mo.same_bits(a, b) and np.array_equal(ca, cb), radii


def test_special_grids():
    void = np.full((9, 11), np.nan, np.float32)
    void[2] = ND
    for op in mo.OPS:
        assert mo.same_bits(mo.morph(void, 3, op), void)
    dtm, cls = mo.ground(void, [1, 2], [1.0, 2.0])
    assert mo.same_bits(dtm, void) and (cls == 0).all()
    one = void.copy()
    one[4, 5] = 7.25
    for op in mo.OPS:
        assert mo.same_bits(mo.morph(one, 2, op), one)                     # the only value of its window, whatever the op
    zeros = np.zeros((5, 6), np.float32)
    zeros[2, 3] = -0.0
    assert np.signbit(mo.morph(zeros, 1, "erode")[1:4, 2:5]).all() and not np.signbit(mo.morph(zeros, 1, "erode")[0, 0])
    assert not np.signbit(mo.morph(zeros, 1, "dilate")).any()


@pytest.mark.parametrize("radius", [1, 3, 8])
def test_erosion_and_dilation_against_scipy(radius):
    ndi = pytest.importorskip("scipy.ndimage")
    z = mo.scene(57, 64, seed=7, voids=0.3)
    ok = mo.valid(z, ND)
    lo = ndi.minimum_filter(np.where(ok, z, np.float32(np.inf)), size=2 * radius + 1, mode="constant", cval=np.inf)
    hi = ndi.maximum_filter(np.where(ok, z, np.float32(-np.inf)), size=2 * radius + 1, mode="constant", cval=-np.inf)
    assert np.array_equal(mo.morph(z, radius, "erode")[ok], lo[ok])        # values: scipy does not say which zero it returns
    assert np.array_equal(mo.morph(z, radius, "dilate")[ok], hi[ok])
    # the fields at INVALID cells too (what an opening's second step reads): transparent cells, none where the window is empty
    k = mo.erode_keys(mo.keys_of(z, ND), radius)
    assert np.array_equal(k != 0, np.isfinite(lo)) and np.array_equal(mo.key2f(k)[k != 0], lo[k != 0])
    opened = ndi.maximum_filter(np.where(np.isfinite(lo), lo, np.float32(-np.inf)), size=2 * radius + 1, mode="constant", cval=-np.inf)
    assert np.array_equal(mo.morph(z, radius, "open")[ok], opened[ok])


def test_opening_never_raises_and_closing_never_lowers():
    z = mo.scene(80, 90, seed=8, voids=0.2)
    ok = mo.valid(z, ND)
    for radius in (1, 2, 6, 33, 100):
        o, c = mo.morph(z, radius, "open"), mo.morph(z, radius, "close")
        assert (mo.f2key(o)[ok] <= mo.f2key(z)[ok]).all() and (mo.f2key(c)[ok] >= mo.f2key(z)[ok]).all()
        assert np.array_equal(o.view(np.uint32)[~ok], z.view(np.uint32)[~ok])          # a NaN stays that NaN
        assert mo.same_bits(mo.morph(o, radius, "open"), o)                # idempotent


def test_crop_property_of_the_oracle():
    z = mo.scene(90, 100, seed=9, voids=0.2)
    radii, thresholds = [1, 2, 4], [1.5, 4.5, 6.0]
    m = 2 * sum(radii)
    r0, r1, c0, c1 = 30, 50, 35, 60
    whole, cw = mo.ground(z, radii, thresholds)
    crop, cc = mo.ground(z[r0 - m:r1 + m, c0 - m:c1 + m], radii, thresholds)
    assert mo.same_bits(crop[m:-m, m:-m], whole[r0:r1, c0:c1]) and np.array_equal(cc[m:-m, m:-m], cw[r0:r1, c0:c1])


# ---- the schedule and the known-answer scene -----------------------------------------------------------------------------------
def test_schedule():
    from satmvs_amd import dsm
    assert mo.schedule(5.0, 16)[0] == [1, 2, 4, 8, 16] and mo.schedule(5.0, 20)[0] == [1, 2, 4, 8, 16, 20]
    assert mo.schedule(5.0, 1) == ([1], [1.5]) and mo.schedule(5.0, 2)[0] == [1, 2] and mo.schedule(5.0, 3)[0] == [1, 2, 3]
    assert mo.schedule(5.0, 16)[1] == [1.5, min(6.0, 0.3 * 2.0 * 5.0 + 1.5), 6.0, 6.0, 6.0]
    assert mo.schedule(0.5, 4, slope=0.2, dh0=0.25, dh_max=9.0)[1] == [0.25, 0.2 * 2.0 * 0.5 + 0.25, 0.2 * 4.0 * 0.5 + 0.25]
    for args in ((5.0, 16), (5.0, 20), (2.5, 1), (0.5, 256, 0.11, 0.3, 77.0), (5.0, 255, 0.0, 0.0, 0.0), (3.0, 100)):
        assert dsm.ground_schedule(*args) == mo.schedule(*args), args
    for bad in ((0.0, 16), (-5.0, 16), (np.nan, 16), (5.0, 0), (5.0, 257), (5.0, 2.5), (5.0, 16, -0.1), (5.0, 16, 0.3, np.inf),
                (5.0, 16, 0.3, 1.5, np.nan)):
        with pytest.raises(ValueError):
            dsm.ground_schedule(*bad)


def test_known_answer_scene():
    """The condition of the feature: with the defaults (5 m cells, max_radius 16) at least 99 % of the valid box cells are
    removed and at least 99 % of the valid other cells stay ground."""
    z, box = mo.known_answer_scene()
    ok = mo.valid(z, ND)
    radii, thresholds = mo.schedule(5.0)
    assert radii == [1, 2, 4, 8, 16]
    dtm, cls = mo.ground(z, radii, thresholds)
    removed_boxes = (cls[ok & box] >= 2).mean()
    kept_ground = (cls[ok & ~box] == 1).mean()
    print("known-answer scene: %.4f of the box cells removed, %.4f of the other cells kept" % (removed_boxes, kept_ground))
    assert (ok & box).sum() > 10000 and removed_boxes >= 0.99 and kept_ground >= 0.99
    assert np.array_equal(cls == 0, ~ok) and np.array_equal(dtm.view(np.uint32)[cls <= 1], z.view(np.uint32)[cls <= 1])
    assert (dtm[cls >= 2] == ND).all() and cls.max() <= 1 + len(radii)


def test_ndsm():
    import torch
    from satmvs_amd import dsm
    rng = np.random.default_rng(3)
    a = rng.normal(100.0, 5.0, (20, 30)).astype(np.float32)
    b = (a - rng.normal(2.0, 3.0, a.shape)).astype(np.float32)
    a[2, 3], b[4, 5], a[6, 7], b[6, 8] = np.nan, ND, ND, np.inf
    b[9, 9] = a[9, 9]
    for clamp in (True, False):
        want = mo.ndsm(a, b, clamp=clamp)
        got = dsm.ndsm(a, b, clamp=clamp)
        assert isinstance(got, np.ndarray) and mo.same_bits(got, want)
        assert mo.same_bits(dsm.ndsm(torch.from_numpy(a), torch.from_numpy(b), clamp=clamp).numpy(), want)
    out = dsm.ndsm(a, b)
    assert out[2, 3] == ND and out[4, 5] == ND and out[6, 7] == ND and out[6, 8] == ND and out[9, 9] == 0.0
    assert (out[out != ND] >= 0).all() and (dsm.ndsm(a, b, clamp=False) < 0).any()
    with pytest.raises(ValueError, match="float32"):
        dsm.ndsm(a.astype(np.float64), b)
    with pytest.raises(ValueError, match="one shape"):
        dsm.ndsm(a, b[:, :5])


# ---- argument checks -----------------------------------------------------------------------------------------------------------
def test_morph_entries_reject_bad_arguments_without_a_gpu(lib):
    from satmvs_amd import _lib
    a, b, m, w = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20), C.c_void_p(4 << 20)
    need = lib.smvs_dsm_morph_workspace_bytes(8, 8, 16)
    assert need >= 3 * 8 * 8 * 4
    assert lib.smvs_dsm_morph_workspace_bytes(0, 8, 16) == 0 and lib.smvs_dsm_morph_workspace_bytes(65536, 32768, 16) == 0
    assert lib.smvs_dsm_morph_workspace_bytes(8, 8, 0) == 0 and lib.smvs_dsm_morph_workspace_bytes(8, 8, 257) == 0

    def morph(dsm=a, gw=8, gh=8, radius=2, op=2, out=b, ws=w, nbytes=need):
        _lib.call("smvs_dsm_morph", dsm, gw, gh, -999.0, radius, op, out, ws, nbytes, None)

    def ground(dsm=a, gw=8, gh=8, radii=(1, 2, 4), thresholds=(1.5, 4.5, 6.0), n=None, dtm=b, cls=m, ws=w, nbytes=need):
        r, t = np.asarray(radii, np.int32), np.asarray(thresholds, np.float64)
        _lib.call("smvs_dsm_ground", dsm, gw, gh, -999.0, r.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p),
                  len(r) if n is None else n, dtm, cls, ws, nbytes, None)

    for kw in ({"dsm": None}, {"out": None}, {"ws": None}):
        with pytest.raises(_lib.SatMVSNativeError, match="null pointer"):
            morph(**kw)
    for kw in ({"dsm": None}, {"dtm": None}, {"cls": None}, {"ws": None}):
        with pytest.raises(_lib.SatMVSNativeError, match="null pointer"):
            ground(**kw)
    for f in (morph, ground):
        with pytest.raises(_lib.SatMVSNativeError, match="non-positive grid"):
            f(gh=0)
        with pytest.raises(_lib.SatMVSNativeError, match="grid too large"):
            f(gw=65536, gh=32768)
        with pytest.raises(_lib.SatMVSNativeError, match="workspace too small"):
            f(nbytes=need - 1)
        with pytest.raises(_lib.SatMVSNativeError, match="workspace aliases"):
            f(ws=C.c_void_p((2 << 20) - need + 4))
    for r in (0, 257, -1):
        with pytest.raises(_lib.SatMVSNativeError, match="radius must be"):
            morph(radius=r)
    for op in (-1, 4):
        with pytest.raises(_lib.SatMVSNativeError, match="op must be"):
            morph(op=op)
    with pytest.raises(_lib.SatMVSNativeError, match="out aliases dsm"):
        morph(out=C.c_void_p((1 << 20) + 8 * 8 * 4 - 4))
    for n in (0, 17, -1):
        with pytest.raises(_lib.SatMVSNativeError, match="n_levels must be"):
            ground(n=n)
    for radii in ((0, 2, 4), (1, 2, 257)):
        with pytest.raises(_lib.SatMVSNativeError, match=r"radii\[\d\] must be"):
            ground(radii=radii)
    for radii in ((1, 1, 4), (2, 1, 4), (1, 4, 3)):
        with pytest.raises(_lib.SatMVSNativeError, match="strictly increasing"):
            ground(radii=radii)
    for t in (-0.5, np.nan, np.inf):
        with pytest.raises(_lib.SatMVSNativeError, match=r"thresholds\[1\] must be"):
            ground(thresholds=(1.5, t, 6.0))
    with pytest.raises(_lib.SatMVSNativeError, match="dtm aliases dsm"):
        ground(dtm=a)
    with pytest.raises(_lib.SatMVSNativeError, match="cls aliases"):
        ground(cls=C.c_void_p((2 << 20) + 16))
    with pytest.raises(_lib.SatMVSNativeError, match="cls aliases"):
        ground(cls=C.c_void_p((1 << 20) - 1))


def test_python_entries_validate_before_the_gpu():
    import torch
    from satmvs_amd import dsm
    z = np.zeros((4, 6), np.float32)
    grid = dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, 6, 4)
    cases = [
        (lambda: dsm.morph(np.zeros((2, 4, 6), np.float32), 1, "open"), r"\(gh, gw\)"),
        (lambda: dsm.morph(z.astype(np.float64), 1, "open"), "float32"),
        (lambda: dsm.morph(torch.zeros(4, 6, dtype=torch.float16), 1, "open"), "float32"),
        (lambda: dsm.morph(z, 0, "open"), "radius"),
        (lambda: dsm.morph(z, 257, "open"), "radius"),
        (lambda: dsm.morph(z, 1.5, "open"), "radius"),
        (lambda: dsm.morph(z, True, "open"), "radius"),
        (lambda: dsm.morph(z, 1, "median"), "op must be"),
        (lambda: dsm.ground_filter(np.zeros(6, np.float32), 5.0), r"\(gh, gw\)"),
        (lambda: dsm.ground_filter(z.astype(np.int32), 5.0), "float32"),
        (lambda: dsm.ground_filter(z), "cell size"),
        (lambda: dsm.ground_filter(z, 0.0), "cell must be"),
        (lambda: dsm.ground_filter(z, 5.0, max_radius=300), "max_radius"),
        (lambda: dsm.ground_filter(z, 5.0, slope=-1.0), "slope"),
        (lambda: dsm.ground_filter(z, 5.0, dh0=float("nan")), "dh0"),
        (lambda: dsm.ground_filter(z, schedule=([], [])), "1 .. 16 radii"),
        (lambda: dsm.ground_filter(z, schedule=(list(range(1, 18)), [1.0] * 17)), "1 .. 16 radii"),
        (lambda: dsm.ground_filter(z, schedule=([1, 2], [1.0])), "as many thresholds"),
        (lambda: dsm.ground_filter(z, schedule=([2, 2], [1.0, 1.0])), "strictly increasing"),
        (lambda: dsm.ground_filter(z, schedule=([1, 2], [1.0, -1.0])), "thresholds must be"),
        (lambda: dsm.extract_dtm(np.zeros((5, 6), np.float32), grid), "differs from the grid"),
        (lambda: dsm.extract_dtm(z, grid, max_steps=0), "max_steps"),
        (lambda: dsm.extract_dtm(z, grid, min_hits=9), "min_hits"),
        (lambda: dsm.extract_dtm(z, grid, max_radius=0), "max_radius"),
    ]
    for f, pattern in cases:
        with pytest.raises(ValueError, match=pattern):
            f()
