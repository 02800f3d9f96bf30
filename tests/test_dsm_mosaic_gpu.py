"""The distance transform and the mosaic on the MI355X (smvs_dsm_dist, smvs_dsm_mosaic, dsm.distance / buffer_mask / mosaic)
against the numpy oracle (tests/dsm_mosaic_oracle.py): every comparison is equal integers or equal bits, no cell excused.
Shapes around the kernels' piece sizes, caps from 1 to 1024, closed forms, guard words, garbage in the workspace, side
streams, the host checks of both C entries, and the chains tiles -> mosaic and coregister -> mosaic."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import dsm_mosaic_oracle as xo
from dsm_testkit import dev, lib, same as _same, scene as _scene  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ND = np.float32(-999.0)
SIZES = [(1, 1), (1, 70), (67, 3), (128, 160), (257, 301)]                 # those of test_dsm_post_gpu
CAPS = [1, 2, 5, 16, 64, 256]
ERR_ARG = 1                                                                # SMVS_ERR_ARG


def _mask(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def _both(mask, caps, what):
    """dsm.distance(squared=True) at every cap and both borders, device-resident (one upload), against the oracle."""
    from satmvs_amd import dsm
    md = torch.from_numpy(mask).cuda()
    for cap in caps:
        for border in (0, 1):
            got = dsm.distance(md, max_dist=cap, border=bool(border), squared=True).cpu().numpy()
            _same(got, xo.dist_two_pass(mask, border, cap), (what, mask.shape, cap, border))


# ---- distance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SIZES)
def test_distance_against_the_oracle(dev, shape):
    _both(_mask(shape, 0.95, 60), CAPS, "0.95")
    _both(_mask(shape, 0.5, 61), [1, 5, 64], "0.5")


@pytest.mark.parametrize("shape", [(300, 2300), (1100, 40)])
def test_distance_beyond_one_piece(dev, shape):
    """(300, 2300): wider than a row piece of 2048 cells; (1100, 40): taller than four column bands of 256 rows."""
    _both(_mask(shape, 0.999, 62), CAPS, "0.999")
    _both(_mask(shape, 0.95, 63), [5, 64], "0.95")


@pytest.mark.parametrize("shape,cap", [((3, 2047), 64), ((3, 2048), 64), ((3, 2049), 64),       # DIST_ROW_SEG = 2048
                                       ((31, 70), 16), ((32, 70), 16), ((33, 70), 16),          # DIST_MIN_BAND = 32
                                       ((99, 70), 100), ((100, 70), 100), ((101, 70), 100),     # a band of `cap` rows between the two
                                       ((255, 70), 256), ((256, 70), 256), ((257, 70), 256)])   # DIST_MAX_BAND = 256
def test_distance_at_the_piece_sizes(dev, shape, cap):
    _both(_mask(shape, 0.998, 64), [cap], "piece")
    one = np.ones(shape, np.uint8)
    one[shape[0] - 1, shape[1] - 1] = 0                                    # the last cell: every carry and halo has to arrive
    _both(one, [cap, 1024], "piece, one cell")


@pytest.mark.parametrize("shape", [(40, 2300), (1100, 40)])
def test_distance_at_the_largest_cap(dev, shape):
    _both(_mask(shape, 0.9995, 65), [1024], "1024")
    _both(np.ones(shape, np.uint8), [1024], "1024, no background")


def test_distance_uniform_masks(dev):
    from satmvs_amd import dsm
    for shape in ((1, 1), (70, 300)):
        for cap in (1, 7, 300):
            for border in (False, True):
                r, c = np.mgrid[0:shape[0], 0:shape[1]]
                edge = np.minimum(np.minimum(r + 1, shape[0] - r), np.minimum(c + 1, shape[1] - c)) ** 2
                want = np.minimum(edge, cap * cap) if border else np.full(shape, cap * cap)
                _same(dsm.distance(np.ones(shape, bool), cap, border, squared=True), want.astype(np.int32), ("foreground", shape, cap, border))
                assert not dsm.distance(np.zeros(shape, bool), cap, border, squared=True).any()


def test_distance_closed_forms(dev):
    """One background cell: the corners, the middle, and just across a row piece (column 2048) and a band (row 64 at cap 64)."""
    from satmvs_amd import dsm
    gh, gw, cap = 130, 2100, 64
    r, c = np.mgrid[0:gh, 0:gw]
    edge = np.minimum(np.minimum(r + 1, gh - r), np.minimum(c + 1, gw - c)) ** 2
    for br, bc in ((0, 0), (0, gw - 1), (gh - 1, 0), (gh - 1, gw - 1), (65, 1000), (64, 2048), (63, 2047)):
        m = np.ones((gh, gw), np.uint8)
        m[br, bc] = 0
        md = torch.from_numpy(m).cuda()
        want = np.minimum((r - br) ** 2 + (c - bc) ** 2, cap * cap)
        _same(dsm.distance(md, cap, False, squared=True).cpu().numpy(), want.astype(np.int32), (br, bc))
        _same(dsm.distance(md, cap, True, squared=True).cpu().numpy(), np.minimum(want, edge).astype(np.int32), (br, bc, "border"))
    m = np.ones((9, 9), np.uint8)
    m[0, 0] = 0
    d = dsm.distance(m, 5, squared=True)
    assert d[3, 4] == 25 and d[4, 3] == 25 and d[4, 4] == 25 and d[2, 4] == 20          # 3-4-5: the cap exactly; (4, 4) capped
    assert dsm.distance(m, 6, squared=True)[4, 4] == 32


def test_distance_mask_bytes_and_dtypes(dev):
    from satmvs_amd import dsm
    base = _mask((67, 130), 0.9, 66)
    want = xo.dist_two_pass(base, 0, 16)
    for byte in (2, 255):                                                  # the C entry itself: any non-zero byte is foreground
        _same(_dist_c(torch.from_numpy(base * np.uint8(byte)).cuda(), 0, 16), want, byte)
    for m in (base.astype(bool), base.astype(np.int32) * 7, torch.from_numpy(base.astype(bool)).cuda()):
        got = dsm.distance(m, 16, squared=True)
        _same(got.cpu().numpy() if isinstance(got, torch.Tensor) else got, want, "dtype")
    d = dsm.distance(base, squared=False)                                  # the default cap: ceil(hypot(67, 130)) = 147
    full = xo.dist_two_pass(base, 0, 147)
    assert d.dtype == np.float32 and np.array_equal(d, np.sqrt(full.astype(np.float64)).astype(np.float32))


@pytest.mark.parametrize("density", [0.001, 0.05, 0.5, 0.95])
def test_distance_densities(dev, density):
    _both(_mask((257, 301), density, int(density * 1000)), [5, 64], density)


def _dist_c(md, border, cap, ws=None, guard=0, stream=None):
    """The C entry on a device mask: d2 inside a buffer with `guard` words at both ends, on `stream`."""
    from satmvs_amd import _lib
    gh, gw = md.shape
    lib = _lib.load()
    nbytes = lib.smvs_dsm_dist_workspace_bytes(gw, gh, cap)
    assert nbytes >= 2 * gw * gh
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=md.device)
    assert ws.numel() >= nbytes
    buf = torch.full((gw * gh + 2 * guard,), 0x5a5a5a5a, dtype=torch.int32, device=md.device)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        _lib.call("smvs_dsm_dist", _lib.ptr(md), gw, gh, border, cap, C.c_void_p(buf.data_ptr() + 4 * guard), _lib.ptr(ws), ws.numel(),
                  _lib.current_stream(md.device))
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert (b[:guard] == 0x5a5a5a5a).all() and (b[gw * gh + guard:] == 0x5a5a5a5a).all()
    return b[guard:gw * gh + guard].reshape(gh, gw)


def test_distance_entry_initialises_guards_and_repeats(dev, lib):
    """Guard words around d2, a workspace full of 0xff, a side stream, two calls, and a larger call before a smaller one on one
    workspace."""
    big, small = _mask((300, 2300), 0.99, 67), _mask((70, 130), 0.9, 68)
    bd, sd = torch.from_numpy(big).cuda(), torch.from_numpy(small).cuda()
    nbytes = lib.smvs_dsm_dist_workspace_bytes(2300, 300, 64)
    ws = torch.full((nbytes,), 0xff, dtype=torch.uint8, device=dev)
    for border in (0, 1):
        want = xo.dist_two_pass(big, border, 64)
        runs = [_dist_c(bd, border, 64, ws=ws, guard=64), _dist_c(bd, border, 64, guard=64),
                _dist_c(bd, border, 64, ws=torch.full((nbytes,), 0xff, dtype=torch.uint8, device=dev), stream=torch.cuda.Stream(dev))]
        assert all(np.array_equal(r, want) for r in runs)
        _same(_dist_c(sd, border, 16, ws=ws, guard=64), xo.dist_two_pass(small, border, 16), "the smaller call on the used workspace")


def test_distance_rejections(dev, lib):
    gw, gh = 40, 30
    m = torch.ones((gh, gw), dtype=torch.uint8, device=dev)
    d2 = torch.full((gh, gw), 77, dtype=torch.int32, device=dev)
    nbytes = lib.smvs_dsm_dist_workspace_bytes(gw, gh, 16)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    P = lambda t: t.data_ptr()
    ok = dict(mask=P(m), gw=gw, gh=gh, border=0, cap=16, d2=P(d2), ws=P(ws), n=nbytes)
    bad = [dict(mask=None), dict(d2=None), dict(ws=None), dict(gw=0), dict(gh=-1), dict(gw=65536, gh=32768), dict(border=2), dict(border=-1),
           dict(cap=0), dict(cap=1025), dict(d2=P(m)), dict(ws=P(m)), dict(ws=P(d2)), dict(d2=P(ws)), dict(n=nbytes - 1), dict(n=0)]
    for change in bad:
        a = dict(ok, **change)
        rc = lib.smvs_dsm_dist(a["mask"], a["gw"], a["gh"], a["border"], a["cap"], a["d2"], a["ws"], a["n"], None)
        assert rc == ERR_ARG and lib.smvs_last_error().decode(), change
    assert lib.smvs_dsm_dist_workspace_bytes(0, 5, 4) == 0 and lib.smvs_dsm_dist_workspace_bytes(5, 5, 0) == 0
    assert lib.smvs_dsm_dist_workspace_bytes(5, 5, 1025) == 0 and lib.smvs_dsm_dist_workspace_bytes(65536, 32768, 4) == 0
    torch.cuda.synchronize()
    assert (d2 == 77).all()                                                # nothing ran


# ---- mosaic: the C entry ---------------------------------------------------------------------------------------------------------
def _special(shape, seed):
    """Heights with every kind of void and both zeros."""
    rng = np.random.default_rng(seed)
    z = rng.normal(100.0, 30.0, shape).astype(np.float32)
    for share, v in ((0.08, np.nan), (0.08, ND), (0.02, np.inf), (0.02, -np.inf), (0.04, -0.0), (0.04, 0.0)):
        z[rng.random(shape) < share] = v
    return z


def _mosaic_c(layers, mode, feather, gw, gh, nodata=-999.0, outputs=(True, True, True), stream=None, guard=0):
    """The C entry on host layers (z, d2 or None, ox, oy) -> [out, count, source, spread], None for the outputs left null."""
    from satmvs_amd import _lib, dsm
    d = torch.device("cuda", 0)
    held, table = [], (dsm._Layer * max(len(layers), 1))()
    for k, (z, d2, ox, oy) in enumerate(layers):
        zt = torch.from_numpy(np.ascontiguousarray(z, np.float32)).to(d)
        dt = torch.from_numpy(np.ascontiguousarray(d2, np.int32)).to(d) if d2 is not None else None
        held.append((zt, dt))
        table[k] = dsm._Layer(zt.data_ptr(), dt.data_ptr() if dt is not None else None, z.shape[1], z.shape[0], ox, oy)
    n = gw * gh
    fills = [(torch.float32, 12345.0), (torch.uint8, 0x5a), (torch.uint8, 0x5a), (torch.float32, 12345.0)]
    bufs = [torch.full((n + 2 * guard,), fill, dtype=dt, device=d) if want else None
            for (dt, fill), want in zip(fills, (True,) + tuple(outputs))]
    ptrs = [C.c_void_p(b.data_ptr() + guard * b.element_size()) if b is not None else None for b in bufs]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        _lib.call("smvs_dsm_mosaic", table, len(layers), float(nodata), xo.MODES.index(mode), feather, gw, gh, *ptrs, _lib.current_stream(d))
    torch.cuda.synchronize()
    res = []
    for b, (dt, fill) in zip(bufs, fills):
        if b is None:
            res.append(None)
            continue
        h = b.cpu().numpy()
        assert (h[:guard] == h.dtype.type(fill)).all() and (h[n + guard:] == h.dtype.type(fill)).all()
        res.append(h[guard:n + guard].reshape(gh, gw))
    return res


def _mosaic_both(layers, mode, feather, gw, gh, what, nodata=-999.0, **kw):
    got = _mosaic_c(layers, mode, feather, gw, gh, nodata, **kw)
    want = xo.mosaic(layers, nodata, mode, feather, gw, gh)
    for g, w, name in zip(got, want, ("out", "count", "source", "spread")):
        if g is not None:
            _same(g, w, (what, mode, name))
    return got


def _with_d2(z, feather, ox, oy, nodata=ND):
    return (z, xo.dist_two_pass(xo.valid(z, nodata), 1, feather), ox, oy)


def test_mosaic_one_layer_is_the_layer(dev):
    z = _special((67, 130), 70)
    want = np.where(xo.valid(z, ND), z, ND)
    assert np.signbit(want[want == 0]).any()
    for mode in xo.MODES:
        out = _mosaic_both([_with_d2(z, 8, 0, 0)], mode, 8, 130, 67, "K = 1")[0]
        _same(out, want, mode)
    zn = np.where(np.isnan(z), np.float32(5.0), z)                         # a NaN nodata: -999 is a height
    for mode in xo.MODES:
        _mosaic_both([_with_d2(zn, 8, 0, 0, np.nan)], mode, 8, 130, 67, "NaN nodata", nodata=float("nan"))


@pytest.mark.parametrize("K", [2, 3, 64])
def test_mosaic_layers_against_the_oracle(dev, K):
    """Layers of several sizes at negative offsets, overhanging every side, one larger than the destination, one that misses
    it."""
    gw, gh = 150, 90
    rng = np.random.default_rng(71 + K)
    layers = [_with_d2(_special((120, 200), 72), 6, -20, -10), _with_d2(_special((50, 60), 73), 6, -30, 60)]
    while len(layers) < K - 1:
        h, w = int(rng.integers(1, 80)), int(rng.integers(1, 100))
        layers.append(_with_d2(_special((h, w), 100 + len(layers)), 6, int(rng.integers(-60, gw)), int(rng.integers(-50, gh))))
    if K > 2:
        layers.append(_with_d2(_special((10, 10), 74), 6, gw, -3))        # touches nothing
    for mode in xo.MODES:
        _mosaic_both(layers[:K], mode, 6, gw, gh, K)
        _mosaic_both(layers[:K], mode, 6, 1, 1, (K, "1 x 1"))


def test_mosaic_ties_and_order(dev):
    a = np.array([[0.0, 5.0, -0.0, 1.0]], np.float32)
    b = np.array([[-0.0, 5.0, 0.0, 2.0]], np.float32)
    layers = [_with_d2(a, 4, 0, 0), _with_d2(b, 4, 0, 0), _with_d2(a, 4, 0, 0)]
    lo = _mosaic_both(layers, "min", 4, 4, 1, "ties")
    hi = _mosaic_both(layers, "max", 4, 4, 1, "ties")
    assert lo[2].tolist() == [[1, 0, 0, 0]] and hi[2].tolist() == [[0, 0, 1, 1]]
    assert np.signbit(lo[0][0, 0]) and not np.signbit(hi[0][0, 0])
    z = [_special((40, 50), 75 + k) for k in range(3)]
    ls = [(z[0], None, 0, 0), (z[1], None, 7, -5), (z[2], None, -9, 11)]
    first = _mosaic_both(ls, "first", 1, 50, 40, "first")[0]
    last = _mosaic_both(ls[::-1], "last", 1, 50, 40, "last")[0]
    _same(first, last, "first = last of the reversed list")


def test_mosaic_optional_outputs_guards_and_streams(dev):
    layers = [_with_d2(_special((67, 130), 80), 5, 0, 0), _with_d2(_special((67, 130), 81), 5, 33, -20)]
    for mode in ("max", "feather"):
        full = _mosaic_both(layers, mode, 5, 130, 67, "all", guard=64)
        for outputs in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
            part = _mosaic_both(layers, mode, 5, 130, 67, outputs, outputs=outputs, guard=64)
            assert [p is None for p in part[1:]] == [not o for o in outputs]
            _same(part[0], full[0], outputs)
        side = _mosaic_both(layers, mode, 5, 130, 67, "side stream", stream=torch.cuda.Stream(dev))
        assert all(np.array_equal(s.view(np.uint8), f.view(np.uint8)) for s, f in zip(side, full))


def test_mosaic_weights_by_hand(dev):
    """d2 = 0, 1, feather^2 - 1, feather^2 and above against a layer of weight 1: w = sqrt(min(max(d2, 1), feather^2))."""
    F = 7
    d2 = np.array([[0, 1, F * F - 1, F * F, F * F + 1, 10 ** 6, -5]], np.int32)
    a = np.full((1, 7), 10.0, np.float32)
    b = np.full((1, 7), 20.0, np.float32)
    got = _mosaic_both([(a, d2, 0, 0), (b, np.ones((1, 7), np.int32), 0, 0)], "feather", F, 7, 1, "weights")
    w = np.sqrt(np.array([1, 1, F * F - 1, F * F, F * F, F * F, 1], np.float64))
    assert np.array_equal(got[0][0], ((w * 10.0 + 20.0) / (w + 1.0)).astype(np.float32))
    assert got[2].tolist() == [[0, 0, 0, 0, 0, 0, 0]] and np.array_equal(got[3][0], np.full(7, 10.0, np.float32))
    assert got[0][0, 3] == np.float32((7 * 10.0 + 20.0) / 8.0)


def test_mosaic_rejections(dev, lib):
    from satmvs_amd import dsm
    gw, gh = 20, 10
    z = torch.zeros((gh, gw), dtype=torch.float32, device=dev)
    d2 = torch.ones((gh, gw), dtype=torch.int32, device=dev)
    out = torch.full((gh, gw), 77.0, dtype=torch.float32, device=dev)
    cnt = torch.empty((gh, gw), dtype=torch.uint8, device=dev)
    src = torch.empty((gh, gw), dtype=torch.uint8, device=dev)
    spr = torch.empty((gh, gw), dtype=torch.float32, device=dev)
    P = lambda t: t.data_ptr()

    def run(n=1, mode=5, feather=4, gw_=gw, gh_=gh, o=P(out), c=P(cnt), s=P(src), p=P(spr), layer=None, table=True):
        t = (dsm._Layer * 65)()
        for k in range(65):
            t[k] = dsm._Layer(**dict(dict(z=P(z), d2=P(d2), gw=gw, gh=gh, ox=0, oy=0), **(layer or {})))
        return lib.smvs_dsm_mosaic(t if table else None, n, -999.0, mode, feather, gw_, gh_, o, c, s, p, None)

    assert run() == 0 and run(n=64) == 0 and run(mode=0, feather=0, layer=dict(d2=None)) == 0
    torch.cuda.synchronize()
    out.fill_(77.0)
    torch.cuda.synchronize()
    bad = [dict(table=False), dict(o=None), dict(n=0), dict(n=65), dict(mode=-1), dict(mode=6), dict(feather=0), dict(feather=1025),
           dict(gw_=0), dict(gh_=0), dict(gw_=65536, gh_=32768), dict(layer=dict(z=None)), dict(layer=dict(d2=None)),
           dict(layer=dict(gw=0)), dict(layer=dict(gh=-2)), dict(layer=dict(gw=65536, gh=32768)),
           dict(layer=dict(ox=2 ** 30)), dict(layer=dict(oy=-2 ** 30)), dict(c=P(out)), dict(s=P(cnt)), dict(p=P(out)), dict(p=P(src)),
           dict(o=P(z)), dict(c=P(z)), dict(s=P(d2)), dict(p=P(d2)), dict(o=P(d2))]
    for change in bad:
        assert run(**change) == ERR_ARG and lib.smvs_last_error().decode(), change
    torch.cuda.synchronize()
    assert (out == 77.0).all()                                             # nothing ran


# ---- end to end ------------------------------------------------------------------------------------------------------------------
GH, GW, RES = 200, 240, 5.0
E0, N0 = 500000.0, 4000000.0
CUTS = [(0, 112, 0, 132), (0, 112, 108, 240), (88, 200, 0, 132), (88, 200, 108, 240)]      # four quadrants, 24 cells of overlap


def _scene_on(grid, **kw):
    c, r = np.meshgrid(np.arange(grid.width), np.arange(grid.height))
    return _scene(grid.e0 + c * grid.xres, grid.n0 - r * grid.yres, **kw)


@pytest.fixture(scope="module")
def tiles():
    from satmvs_amd.dsm import DSMGrid
    whole = DSMGrid(E0, N0, RES, RES, GW, GH)
    z = _scene_on(whole, seed=90, voids=0.03)
    assert xo.valid(z, ND).mean() < 0.98 and not np.signbit(z[z == 0]).any()
    grids = [DSMGrid(E0 + c0 * RES, N0 - r0 * RES, RES, RES, c1 - c0, r1 - r0) for r0, r1, c0, c1 in CUTS]
    return z, whole, [z[r0:r1, c0:c1].copy() for r0, r1, c0, c1 in CUTS], grids


def test_tiles_of_a_scene_come_back(dev, tiles):
    from satmvs_amd import dsm
    z, whole, parts, grids = tiles
    assert dsm.mosaic_grid(grids) == whole
    want = np.where(xo.valid(z, ND), z, ND)
    for mode in xo.MODES:
        out, count = dsm.mosaic(parts, grids, mode=mode, feather=8, return_count=True)
        _same(out, want, mode)
        assert count.max() == 4 and np.array_equal(count == 0, ~xo.valid(z, ND))


def test_biased_tiles_feather_has_no_step(dev, tiles):
    from satmvs_amd import dsm
    z, whole, parts, grids = tiles
    F, bias = 8, (0.5, -0.5, -0.5, 0.5)
    gap = max(bias) - min(bias)
    ok = xo.valid(z, ND)
    moved = [np.where(xo.valid(p, ND), p + np.float32(b), p) for p, b in zip(parts, bias)]

    def largest_step(out):
        """The largest neighbour-to-neighbour change of out - scene: what the mosaic adds to the scene's own steps."""
        e = np.where(ok, out.astype(np.float64) - z.astype(np.float64), np.nan)
        with np.errstate(invalid="ignore"):
            return max(np.nanmax(np.abs(np.diff(e, axis=0))), np.nanmax(np.abs(np.diff(e, axis=1))))

    first = dsm.mosaic(moved, grids, mode="first")
    layers = [(m, xo.dist_two_pass(xo.valid(m, ND), 1, F), *xo.offset(g, whole)) for m, g in zip(moved, grids)]
    _same(first, xo.mosaic(layers, ND, "first", F, GW, GH)[0], "first")
    blend, source, spread = dsm.mosaic(moved, grids, mode="feather", feather=F, return_source=True, return_spread=True)
    want = xo.mosaic(layers, ND, "feather", F, GW, GH)
    _same(blend, want[0], "feather")
    _same(source, want[2], "source")
    _same(spread, want[3], "spread")
    # out - scene is the mean of the biases under the normalised weights t.  Between two neighbouring valid cells the sets of
    # layers share a member (the overlap is wider than two cells and the voids are the scene's, the same in every tile); a
    # shared layer weighs at least 1 of at most K F at both, so the two weight vectors overlap by 1 / (K F) and the mean
    # moves by at most gap (1 - 1 / (K F)); float32 rounding of heights near 200 m adds less than 1e-4.
    K = len(parts)
    bound = gap * (1.0 - 1.0 / (K * F)) + 1e-4
    print("largest step added to the scene: first %.4f, feather %.4f, bound %.4f, gap %.1f" % (largest_step(first), largest_step(blend), bound, gap))
    assert largest_step(first) >= gap - 1e-4
    assert largest_step(blend) <= bound < gap


def test_align_bilinear_is_regrid_then_mosaic(dev, tiles):
    from satmvs_amd import dsm
    from satmvs_amd.dsm import DSMGrid
    z, whole, parts, grids = tiles
    off = DSMGrid(E0 + 10.5 * RES, N0 - 30 * RES, RES, RES, 40, 50)       # half a cell east of the lattice: columns 10 .. 50
    zo = _scene_on(off, seed=91, voids=0.02)
    with pytest.raises(ValueError, match="align"):
        dsm.mosaic([parts[0], zo], [grids[0], off])
    sub = DSMGrid(E0 + 10 * RES, N0 - 30 * RES, RES, RES, 41, 50)
    for align in ("bilinear", "nearest"):
        on = dsm.regrid(zo, off, sub, mode=align)
        for mode in ("last", "feather"):
            got = dsm.mosaic([parts[0], zo], [grids[0], off], to_grid=grids[0], mode=mode, align=align)
            _same(got, dsm.mosaic([parts[0], on], [grids[0], sub], to_grid=grids[0], mode=mode), (align, mode))
    gone = DSMGrid(E0 - 500.25 * RES, N0, RES, RES, 40, 50)                # unaligned and off the destination: contributes nothing
    _same(dsm.mosaic([parts[0], zo], [grids[0], gone], to_grid=grids[0], mode="last", align="nearest"),
          np.where(xo.valid(parts[0], ND), parts[0], ND), "no overlap")


def test_coregister_then_mosaic(dev, tiles):
    from satmvs_amd import dsm
    from satmvs_amd.dsm import DSMGrid
    z, whole, parts, grids = tiles
    rng = np.random.default_rng(92)
    r0, r1, c0, c1 = 40, 160, 60, 200
    tile = z[r0:r1, c0:c1].copy()
    ok = xo.valid(tile, ND)
    tile = np.where(ok, tile + np.float32(1.5) + rng.normal(0.0, 0.1, tile.shape).astype(np.float32), np.float32(np.nan)).astype(np.float32)
    said = DSMGrid(E0 + (c0 + 2) * RES, N0 - (r0 - 1) * RES, RES, RES, c1 - c0, r1 - r0)      # the georeference is 2, -1 cells off
    reg = dsm.coregister(tile, said, z, whole)
    assert abs(reg["grid"].e0 - (E0 + c0 * RES)) < 0.1 * RES and abs(reg["grid"].n0 - (N0 - r0 * RES)) < 0.1 * RES
    assert abs(reg["dz"] - 1.5) < 0.05
    out, count = dsm.mosaic([z, tile - np.float32(reg["dz"])], [whole, reg["grid"]], to_grid=whole, align="bilinear", return_count=True)
    both = count == 2
    assert both.sum() > 0.5 * ok.sum()
    err = np.abs(out.astype(np.float64) - z.astype(np.float64))[both]
    print("coregister -> mosaic: mean |error| %.4f m over %d cells, registration std %.4f m" % (err.mean(), both.sum(), reg["std"]))
    assert err.mean() <= reg["std"]
    untouched = (count == 1)
    assert np.array_equal(out[untouched].view(np.uint32), z[untouched].view(np.uint32))


@pytest.mark.parametrize("radius", [1, 1.5, 2.9, 16])
def test_buffer_mask(dev, radius):
    from satmvs_amd import dsm
    m = _mask((150, 170), 0.002, 93).astype(bool)
    m[0, 0] = m[149, 169] = True
    for border in (False, True):
        got = dsm.buffer_mask(m, radius, border)
        assert got.dtype == np.bool_ and np.array_equal(got, xo.buffer_mask(m, radius, border)), (radius, border)
        assert got[m].all()
    on = dsm.buffer_mask(torch.from_numpy(m).cuda(), radius)
    assert isinstance(on, torch.Tensor) and on.dtype == torch.bool and np.array_equal(on.cpu().numpy(), xo.buffer_mask(m, radius))
