"""The numpy statements of the distance transform and the mosaic (tests/dsm_mosaic_oracle.py) against each other, against
scipy and against closed forms; the identities the mosaic's rules promise; the alignment rule and mosaic_grid on hand-made
grids; every Python argument rejection that needs no GPU; and planted errors that the GPU file's comparison must report."""
import numpy as np
import pytest

import dsm_mosaic_oracle as xo
from dsm_testkit import same as _same
from satmvs_amd import dsm
from satmvs_amd.dsm import DSMGrid

ND = np.float32(-999.0)


def _mask(shape, density, seed):
    return np.random.default_rng(seed).random(shape) < density


def _differs(got, want):
    """Whether the GPU file's comparison (dsm_testkit.same) reports a difference."""
    try:
        _same(got, want, "planted")
    except AssertionError:
        return True
    return False


# ---- the transform --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", [0, 1])
@pytest.mark.parametrize("cap", [1, 5, 64])
def test_the_two_statements_agree(border, cap):
    for shape, density, seed in (((1, 1), 0.5, 1), ((1, 37), 0.9, 2), ((41, 3), 0.9, 3), ((48, 45), 0.5, 4), ((40, 48), 0.95, 5),
                                 ((48, 48), 0.999, 6), ((30, 30), 1.1, 7), ((30, 30), -1.0, 8)):
        m = _mask(shape, density, seed)
        _same(xo.dist_two_pass(m, border, cap), xo.dist_brute(m, border, cap), (shape, density, border, cap))


@pytest.mark.parametrize("border", [0, 1])
@pytest.mark.parametrize("density", [0.5, 0.95, 0.999])
def test_the_statements_agree_with_scipy(border, density):
    ndi = pytest.importorskip("scipy.ndimage")
    m = _mask((90, 130), density, int(density * 1000))
    if border:
        edt = ndi.distance_transform_edt(np.pad(m, 1))[1:-1, 1:-1]
    else:
        edt = ndi.distance_transform_edt(m) if not m.all() else np.full(m.shape, np.inf)
    exact = np.rint(np.minimum(edt, 1e4) ** 2).astype(np.int64)
    for cap in (1, 5, 64):
        want = np.minimum(exact, cap * cap).astype(np.int32)
        _same(xo.dist_two_pass(m, border, cap), want, (density, border, cap))


def test_closed_forms():
    gh, gw = 33, 47
    r, c = np.mgrid[0:gh, 0:gw]
    for br, bc in ((0, 0), (gh - 1, gw - 1), (16, 20)):
        m = np.ones((gh, gw), bool)
        m[br, bc] = False
        for cap in (1, 5, 64):
            want = np.minimum((r - br) ** 2 + (c - bc) ** 2, cap * cap).astype(np.int32)
            _same(xo.dist_two_pass(m, 0, cap), want, (br, bc, cap))
            edge = np.minimum(np.minimum(r + 1, gh - r), np.minimum(c + 1, gw - c)) ** 2
            _same(xo.dist_two_pass(m, 1, cap), np.minimum(want, edge).astype(np.int32), (br, bc, cap, "border"))
    full = np.ones((gh, gw), bool)
    assert (xo.dist_two_pass(full, 0, 7) == 49).all() and (xo.dist_brute(full, 0, 7) == 49).all()        # the empty set
    assert (xo.dist_two_pass(~full, 0, 7) == 0).all()
    m = np.ones((9, 9), np.uint8)
    m[0, 0] = 0
    d = xo.dist_two_pass(m, 0, 5)
    assert d[3, 4] == 25 and d[4, 3] == 25 and d[4, 4] == 25 and xo.dist_two_pass(m, 0, 6)[4, 4] == 32   # 3-4-5: exactly the cap; capped


def test_buffer_mask_statement():
    m = np.zeros((20, 20), bool)
    m[10, 10] = True
    r, c = np.mgrid[0:20, 0:20]
    d2 = (r - 10) ** 2 + (c - 10) ** 2
    for radius in (1, 1.5, 2.9, 16):
        assert np.array_equal(xo.buffer_mask(m, radius), d2 <= radius * radius), radius


# ---- the mosaic's identities ----------------------------------------------------------------------------------------------------
def _layer(shape, seed):
    rng = np.random.default_rng(seed)
    z = rng.normal(100.0, 30.0, shape).astype(np.float32)
    z[rng.random(shape) < 0.1] = np.nan
    z[rng.random(shape) < 0.1] = ND
    z[rng.random(shape) < 0.02] = np.inf
    z[rng.random(shape) < 0.05] = -0.0
    return z


def test_one_layer_comes_back_in_every_mode():
    z = _layer((40, 50), 11)
    d2 = xo.dist_two_pass(xo.valid(z, ND), 1, 8)
    want = np.where(xo.valid(z, ND), z, ND)
    for mode in xo.MODES:
        out, count, source, spread = xo.mosaic([(z, d2, 0, 0)], ND, mode, 8, 50, 40)
        _same(out, want, mode)
        assert np.array_equal(count, xo.valid(z, ND).astype(np.uint8))
        assert np.array_equal(source, np.where(xo.valid(z, ND), 0, 255).astype(np.uint8))
        _same(spread, np.where(xo.valid(z, ND), np.float32(0.0), ND), mode)
    assert np.signbit(want[xo.valid(z, ND)]).any()                             # -0.0 went through


def test_equal_layers_give_the_layer():
    """K equal layers: w z summed over K layers and divided by the sum of w is z to far less than half a float32 ulp."""
    rng = np.random.default_rng(12)
    z = (rng.normal(0.0, 1.0, (400, 500)) * 10.0 ** rng.integers(-3, 4, (400, 500))).astype(np.float32)      # 2e5 values
    d2 = rng.integers(0, 300, z.shape).astype(np.int32)
    for K in range(1, 6):
        for mode in ("mean", "feather"):
            out = xo.mosaic([(z, d2, 0, 0)] * K, ND, mode, 16, 500, 400)[0]
            _same(out, z, (K, mode))


def test_offsets_and_overhang():
    a = np.arange(12, dtype=np.float32).reshape(3, 4) + 1
    b = np.full((2, 2), 50.0, np.float32)
    out, count, source, spread = xo.mosaic([(a, None, -1, 1), (b, None, 1, 2), (b, None, 9, 9)], ND, "last", 1, 4, 4)
    want = np.array([[ND] * 4, [2, 3, 4, ND], [6, 50, 50, ND], [10, 50, 50, ND]], np.float32)
    _same(out, want, "last")
    assert count.tolist() == [[0] * 4, [1, 1, 1, 0], [1, 2, 2, 0], [1, 2, 2, 0]]
    assert source[2, 1] == 1 and source[1, 1] == 0 and source[0, 0] == 255
    assert spread[2, 1] == 50 - 7 and spread[1, 0] == 0 and spread[0, 0] == ND
    first = xo.mosaic([(a, None, -1, 1), (b, None, 1, 2)], ND, "first", 1, 4, 4)[0]
    flipped = xo.mosaic([(b, None, 1, 2), (a, None, -1, 1)], ND, "last", 1, 4, 4)[0]
    _same(first, flipped, "first = last of the reversed list")


# ---- grids ----------------------------------------------------------------------------------------------------------------------
def test_layer_offsets_and_alignment():
    d = DSMGrid(500000.0, 4000000.0, 5.0, 5.0, 100, 80)
    g = DSMGrid(500000.0 + 35.0, 4000000.0 - 60.0, 5.0, 5.0, 10, 10)
    assert dsm._layer_offset(g, d) == (7, 12, True) and xo.offset(g, d) == (7, 12)
    assert dsm._layer_offset(DSMGrid(500000.0 - 15.0, 4000000.0 + 5.0, 5.0, 5.0, 10, 10), d) == (-3, -1, True)
    assert dsm._layer_offset(DSMGrid(500000.0 + 35.0 + 4e-6, 4000000.0, 5.0, 5.0, 10, 10), d)[2]            # 8e-7 cell
    assert not dsm._layer_offset(DSMGrid(500000.0 + 35.0 + 6e-6, 4000000.0, 5.0, 5.0, 10, 10), d)[2]        # 1.2e-6 cell
    assert not dsm._layer_offset(DSMGrid(500000.0, 4000000.0 - 2.5, 5.0, 5.0, 10, 10), d)[2]
    assert not dsm._layer_offset(DSMGrid(500000.0, 4000000.0, 2.5, 5.0, 10, 10), d)[2]


def test_mosaic_grid():
    a = DSMGrid(1000.0, 2000.0, 5.0, 5.0, 10, 8)
    assert dsm.mosaic_grid([a]) == a
    b = DSMGrid(1000.0 - 15.0, 2000.0 + 10.0, 5.0, 5.0, 4, 30)
    assert dsm.mosaic_grid([a, b]) == DSMGrid(985.0, 2010.0, 5.0, 5.0, 13, 30)
    c = DSMGrid(1000.0 + 47.5, 2000.0 - 2.5, 5.0, 5.0, 2, 2)                   # half a cell off: centres at 9.5, 10.5 columns
    assert dsm.mosaic_grid([a, c]) == DSMGrid(1000.0, 2000.0, 5.0, 5.0, 12, 8)
    e = DSMGrid(1000.0, 2000.0, 10.0, 10.0, 10, 2)                             # coarser: centres up to 90 m east
    assert dsm.mosaic_grid([a, e]) == DSMGrid(1000.0, 2000.0, 5.0, 5.0, 19, 8)
    with pytest.raises(ValueError):
        dsm.mosaic_grid([])
    with pytest.raises(ValueError, match="64"):
        dsm.mosaic_grid([a] * 65)
    with pytest.raises(ValueError):
        dsm.mosaic_grid([a, DSMGrid(float("nan"), 0.0, 5.0, 5.0, 2, 2)])


# ---- rejections that need no GPU ------------------------------------------------------------------------------------------------
def test_python_rejections():
    g = DSMGrid(0.0, 0.0, 5.0, 5.0, 6, 4)
    z = np.zeros((4, 6), np.float32)
    m = np.ones((4, 6), bool)
    for bad in (0, 1025, 2.5, True, -1):
        with pytest.raises(ValueError, match="max_dist"):
            dsm.distance(m, max_dist=bad)
    with pytest.raises(ValueError):
        dsm.distance(np.ones((4, 6), np.float32))
    with pytest.raises(ValueError):
        dsm.distance(np.ones((2, 4, 6), bool))
    for bad in (0, -1.0, 1024, 2000.0, float("nan")):
        with pytest.raises(ValueError, match="radius"):
            dsm.buffer_mask(m, bad)
    with pytest.raises(ValueError):
        dsm.buffer_mask(np.ones(5, bool), 2)
    with pytest.raises(ValueError, match="mode"):
        dsm.mosaic([z], [g], mode="median")
    with pytest.raises(ValueError, match="align"):
        dsm.mosaic([z], [g], align="cubic")
    for bad in (0, 1025, 1.5):
        with pytest.raises(ValueError, match="feather"):
            dsm.mosaic([z], [g], feather=bad)
    with pytest.raises(ValueError, match="64"):
        dsm.mosaic([z] * 65, [g] * 65)
    with pytest.raises(ValueError):
        dsm.mosaic([], [])
    with pytest.raises(ValueError, match="one grid per DSM"):
        dsm.mosaic([z, z], [g])
    with pytest.raises(ValueError, match="shape"):
        dsm.mosaic([np.zeros((3, 3), np.float32)], [g])
    with pytest.raises(ValueError):
        dsm.mosaic([z], [g], to_grid=DSMGrid(0.0, 0.0, -5.0, 5.0, 6, 4))
    half = DSMGrid(2.5, 0.0, 5.0, 5.0, 6, 4)
    with pytest.raises(ValueError, match="align.*regrid"):
        dsm.mosaic([z, z], [g, half])
    with pytest.raises(ValueError, match="align.*regrid"):
        dsm.mosaic([z, z], [g, DSMGrid(0.0, 0.0, 2.5, 2.5, 6, 4)])
    with pytest.raises(ValueError, match="2\\^30"):
        dsm.mosaic([z], [g], to_grid=DSMGrid(-5.0 * 2 ** 30, 0.0, 5.0, 5.0, 6, 4))


# ---- planted errors: the comparison of the GPU file has to report each ---------------------------------------------------------
def test_planted_errors_are_reported():
    m = np.ones((9, 40), bool)
    m[4, 3] = False
    good = xo.dist_two_pass(m, 0, 16)
    assert not _differs(good, xo.dist_brute(m, 0, 16))
    assert _differs(xo.dist_two_pass(m, 0, 16, plant="short halo"), good)      # the cell 15 columns east loses its 225
    assert _differs(xo.dist_two_pass(m, 0, 16, plant="cap first"), good)
    z = np.array([[-0.0, 3.0, 7.0]], np.float32)
    d2 = np.array([[4, 4, 4]], np.int32)
    for mode in ("mean", "feather"):
        good = xo.mosaic([(z, d2, 0, 0)], ND, mode, 4, 3, 1)[0]
        assert not _differs(good, z)
        assert _differs(xo.mosaic([(z, d2, 0, 0)], ND, mode, 4, 3, 1, plant="from zero")[0], good)        # 0.0 + -0.0 = +0.0
    tie = [(np.array([[0.0, 5.0]], np.float32), d2[:, :2], 0, 0), (np.array([[-0.0, 5.0]], np.float32), d2[:, :2], 0, 0),
           (np.array([[0.0, 5.0]], np.float32), d2[:, :2], 0, 0)]
    for mode in ("min", "max", "feather"):
        good = xo.mosaic(tie, ND, mode, 4, 2, 1)
        late = xo.mosaic(tie, ND, mode, 4, 2, 1, plant="late ties")
        assert _differs(late[2], good[2]), mode                               # the source map names the later layer
    assert xo.mosaic(tie, ND, "min", 4, 2, 1)[2].tolist() == [[1, 0]] and xo.mosaic(tie, ND, "max", 4, 2, 1)[2].tolist() == [[0, 0]]
