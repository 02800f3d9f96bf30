"""DSM production on the MI355X: Transverse Mercator against the reference's outputs, the bin pass against numpy, the reduce
against a per-cell np.lexsort oracle (every sort tier, one cell of more than 4 M points), determinism under reruns and map
order, a known answer, and the filter -> DSM chain; then the case matrix of tests/dsm_scene.py (the scan past one chunk, every
bucket size and tier threshold, listed cells beyond the grids of the workgroup tiers, special key values, cancellation) in all
four modes with no cell excused and the mean inside its derived interval (dsm_oracle.reference), equal bits under permutation,
the C entry on a guarded workspace, the bin pass at partial waves, every run length and pixels on cell edges, smvs_tm_project
alone, heights_to_dsm on other dtypes, layouts and streams, and a seeded random run.  tests/test_dsm_cpu.py asserts what
these tests assume of the matrix and that their comparisons report nine planted errors."""
import functools

import numpy as np
import pytest
import torch

import dsm_oracle as orc
import dsm_scene as sc
from dsm_testkit import dev, proj, tm7  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

MODES = ("median", "mean", "min", "max")


def _ulp_diff(a, b):
    ia = a.astype(np.float32).view(np.int32).astype(np.int64)
    ib = b.astype(np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def _check_against_oracle(got, want, mode):
    if mode == "mean":
        assert _ulp_diff(got, want).max() <= 1
    else:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (mode, int((got != want).sum()))


@pytest.mark.parametrize("name", ["whu", "example"])
def test_tm_project_matches_reference(golden, dev, name):
    from satmvs_amd.transverse_mercator import Ellipsoid, TransverseMercator
    g = golden("tm")
    tm7 = g[name + ".tm7"]
    proj = TransverseMercator(Ellipsoid(tm7[0], tm7[1]), *tm7[2:])
    en = proj.proj(g[name + ".latlon"])
    assert isinstance(en, np.ndarray) and en.shape == (2000, 2)
    assert np.abs(en - g[name + ".en"]).max() <= 1e-6
    ll = proj.proj(g[name + ".en"], reverse=True)
    assert np.abs(ll - g[name + ".latlon_back"]).max() <= 1e-11
    t = torch.from_numpy(g[name + ".en"]).to(dev).reshape(40, 50, 2)       # device tensors stay on the device, shape kept
    out = proj.EastNorth2latlon(t)
    assert out.is_cuda and out.shape == (40, 50, 2)
    assert np.abs(out.cpu().numpy().reshape(-1, 2) - g[name + ".latlon_back"]).max() <= 1e-11


def _scene(H, W, seed, lon0=-134.6, lat0=31.0, nan_share=0.02):
    from satmvs_amd import rpc_synth
    rng = np.random.default_rng(seed)
    rpc = rpc_synth.make_view_rpcs(1, H, W, seed=seed, gsd=2.1, lat0=lat0, lon0=lon0)[0]
    h = (150.0 + 60.0 * np.sin(np.arange(W) / 9.0)[None, :] + rng.normal(0.0, 3.0, (H, W))).astype(np.float32)
    h[rng.random((H, W)) < nan_share] = np.nan
    return h, rpc


def test_bin_pass_against_numpy(dev):
    from satmvs_amd import dsm, rpc_synth
    from satmvs_amd.transverse_mercator import whu_tlc_projection
    proj = whu_tlc_projection()
    tm7 = proj.tm7()
    H, W = 96, 160
    h, rpc = _scene(H, W, 5)
    mask = np.random.default_rng(6).random((H, W)) > 0.1
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    lat, lon = rpc_synth.photo2obj(rpc, x, y, h.astype(np.float64))
    E, N = orc.tm_forward(tm7, lat, lon)
    valid = mask & np.isfinite(h)
    # a grid over the middle of the extent: some points fall off it
    grid = dsm.grid_from_extent(np.percentile(E[valid], 10), np.percentile(E[valid], 90), np.percentile(N[valid], 10),
                                np.percentile(N[valid], 90), 5.0)
    (east, north), = dsm.project_to_map([h], [rpc], proj, [mask])
    east, north = east.cpu().numpy(), north.cpu().numpy()
    assert np.array_equal(np.isfinite(east), valid) and np.array_equal(np.isfinite(north), valid)
    assert np.abs(east - E)[valid].max() <= 1e-5 and np.abs(north - N)[valid].max() <= 1e-5
    cell = torch.empty(H * W, dtype=torch.int32, device=dev)
    count = torch.zeros(grid.width * grid.height, dtype=torch.int32, device=dev)
    hd = torch.from_numpy(h).to(dev)
    md = torch.from_numpy(mask.astype(np.uint8)).to(dev)
    dsm._bin(hd, torch.from_numpy(rpc).to(dev), md, tm7, grid.grid4(), grid.width, grid.height, cell, count)
    got = cell.cpu().numpy().reshape(H, W)
    # numpy binning of the GPU's own E / N: bit-equal cells
    assert np.array_equal(got, orc.cells(east, north, grid.grid4(), grid.width, grid.height))
    # numpy's own E / N: equal wherever the point is more than 1e-6 m from a cell edge
    want = orc.cells(np.where(valid, E, np.nan), np.where(valid, N, np.nan), grid.grid4(), grid.width, grid.height)
    with np.errstate(invalid="ignore"):
        fc = (E - grid.e0) / grid.xres + 0.5
        fr = (grid.n0 - N) / grid.yres + 0.5
        far = (np.minimum(fc - np.floor(fc), np.ceil(fc) - fc) * grid.xres > 1e-6) & \
              (np.minimum(fr - np.floor(fr), np.ceil(fr) - fr) * grid.yres > 1e-6)
    sel = far | ~valid
    assert np.array_equal(got[sel], want[sel])
    assert (got == -1).sum() > valid.size * 0.2 and (got >= 0).sum() > valid.size * 0.3      # both on and off the grid
    assert np.array_equal(count.cpu().numpy(), np.bincount(got[got >= 0], minlength=grid.width * grid.height))


def _oracle_dsm(heights, rpcs, proj, grid, masks, mode, nodata):
    from satmvs_amd import dsm
    en = dsm.project_to_map(heights, rpcs, proj, masks)
    cells = np.concatenate([orc.cells(e.cpu().numpy(), n.cpu().numpy(), grid.grid4(), grid.width, grid.height).reshape(-1)
                            for e, n in en])
    hs = np.concatenate([np.asarray(h, np.float32).reshape(-1) for h in heights])
    out, count = orc.reduce(cells, hs, grid.width * grid.height, mode, nodata)
    return out.reshape(grid.height, grid.width), count.reshape(grid.height, grid.width)


def test_heights_to_dsm_against_oracle(dev):
    """Two maps of different sizes, NaN heights, masked pixels, points off the grid, empty cells; ~6 points per cell."""
    from satmvs_amd import dsm
    from satmvs_amd.transverse_mercator import whu_tlc_projection
    proj = whu_tlc_projection()
    (h1, r1), (h2, r2) = _scene(120, 200, 11), _scene(90, 150, 12, nan_share=0.05)
    m1 = np.random.default_rng(13).random(h1.shape) > 0.15
    m2 = np.ones(h2.shape, bool)
    m2[:, :20] = False                                       # a masked band
    h1[50:70, 80:120] = np.nan                               # the same patch of ground missing in both maps: empty cells
    h2[35:55, 55:95] = np.nan
    full = dsm.grid_for([h1, h2], [r1, r2], proj, 5.0, masks=[m1, m2])
    # cut the grid: points off it on every side; 5 m cells at a 2.1 m GSD hold ~6 points of one map
    grid = dsm.DSMGrid(full.e0 + 50.0, full.n0 - 40.0, 5.0, 5.0, full.width - 25, full.height - 15)
    for mode in MODES:
        got, cnt = dsm.heights_to_dsm([h1, h2], [r1, r2], proj, grid, masks=[m1, m2], mode=mode, nodata=-999.0,
                                      return_count=True)
        want, wcnt = _oracle_dsm([h1, h2], [r1, r2], proj, grid, [m1, m2], mode, -999.0)
        assert got.dtype == np.float32 and got.shape == (grid.height, grid.width) and cnt.dtype == np.int32
        assert np.array_equal(cnt, wcnt)
        assert (cnt == 0).sum() > 0 and (got[cnt == 0] == -999.0).all()                      # empty cells
        assert 3.0 < cnt[cnt > 0].mean() < 14.0
        _check_against_oracle(got, want, mode)


def test_every_sort_tier(dev):
    """Cells of 1 .. 32 points (one lane), 33 .. 4096 (bitonic in LDS), more (radix), one of them above 4 M points."""
    from satmvs_amd import dsm
    rng = np.random.default_rng(21)
    sizes = {0: 0, 1: 1, 2: 2, 3: 7, 4: 32, 5: 33, 6: 100, 7: 1000, 8: 4096, 9: 4097, 10: 10000, 11: (1 << 22) + 123}
    gw, gh = 4, 4                                            # cells 12 .. 15 stay empty
    cell = np.concatenate([np.full(n, c, np.int32) for c, n in sizes.items()])
    h = rng.normal(0.0, 100.0, cell.size).astype(np.float32)
    h[::7] = np.round(h[::7])                                # many ties
    h[::11] = 0.0
    h[::13] = -0.0
    perm = rng.permutation(cell.size)
    cell, h = cell[perm], h[perm]
    grid = dsm.DSMGrid(0.0, 0.0, 1.0, 1.0, gw, gh)
    cd, hd = torch.from_numpy(cell).to(dev), torch.from_numpy(h).to(dev)
    count = torch.bincount(cd.long(), minlength=gw * gh).to(torch.int32)
    for mode in MODES:
        got = dsm.reduce_cells(cd, hd, count, grid, mode, nodata=-1.0).cpu().numpy().reshape(-1)
        want, _ = orc.reduce(cell, h, gw * gh, mode, -1.0)
        _check_against_oracle(got, want, mode)
        assert (got[12:] == -1.0).all() and got[0] == -1.0


def test_deterministic_under_reruns_and_map_order(dev):
    from satmvs_amd import dsm
    from satmvs_amd.transverse_mercator import whu_tlc_projection
    proj = whu_tlc_projection()
    maps = [_scene(256, 384, 31), _scene(200, 320, 32), _scene(256, 384, 33)]
    hs = [torch.from_numpy(h).to(dev) for h, _ in maps]
    rs = [torch.from_numpy(r).to(dev) for _, r in maps]
    grid = dsm.grid_for(hs, rs, proj, 5.0)
    for mode in MODES:
        a = dsm.heights_to_dsm(hs, rs, proj, grid, mode=mode)
        b = dsm.heights_to_dsm(hs, rs, proj, grid, mode=mode)
        c = dsm.heights_to_dsm(hs[::-1], rs[::-1], proj, grid, mode=mode)
        assert a.is_cuda
        a, b, c = (t.cpu().numpy().view(np.uint32) for t in (a, b, c))
        assert np.array_equal(a, b) and np.array_equal(a, c), mode


def test_constant_height_known_answer(dev):
    from satmvs_amd import dsm
    from satmvs_amd.transverse_mercator import whu_tlc_projection
    proj = whu_tlc_projection()
    _, rpc = _scene(128, 192, 41)
    h = np.full((128, 192), 123.25, np.float32)
    grid = dsm.grid_for([h], [rpc], proj, 5.0)
    for mode in MODES:
        got, cnt = dsm.heights_to_dsm([h], [rpc], proj, grid, mode=mode, nodata=-999.0, return_count=True)
        assert cnt.sum() == h.size
        assert (got[cnt > 0] == np.float32(123.25)).all(), mode
        assert (got[cnt == 0] == -999.0).all()


def test_filter_to_dsm_chain(golden, dev):
    from satmvs_amd import dsm, rpc_filter
    from satmvs_amd.transverse_mercator import Ellipsoid, TransverseMercator
    g = golden("filter")
    depths, rpcs = g["depths"], g["rpc"]
    mask, averaged = rpc_filter.filter_depth([d for d in depths], [r for r in rpcs], float(g["p_ratio"]),
                                             float(g["d_ratio"]), int(g["geo_consist_num"]), prob=g["prob"],
                                             confidence_ratio=float(g["confidence_ratio"]))
    assert mask.any()
    proj = TransverseMercator(Ellipsoid(), 0.0, float(np.round(rpcs[0][3])), 0.9996, 500000.0, 0.0)
    en = dsm.project_to_map([averaged.astype(np.float32)], [rpcs[0]], proj, [mask])[0]
    e = en[0][torch.isfinite(en[0])]
    res = float(e.max() - e.min()) / 12.0                     # a dozen cells across: several points per cell
    grid = dsm.grid_for([averaged], [rpcs[0]], proj, res, masks=[mask])
    for mode in MODES:
        got = dsm.heights_to_dsm([averaged], [rpcs[0]], proj, grid, masks=[mask], mode=mode)
        want, cnt = _oracle_dsm([averaged.astype(np.float32)], [rpcs[0]], proj, grid, [mask], mode, -999.0)
        assert cnt.sum() == mask.sum()
        _check_against_oracle(got, want, mode)


# ---- the case matrix -------------------------------------------------------------------------------------------------------------
NODATAS = (-999.0, -0.0, float("nan"))


@functools.lru_cache(maxsize=None)
def _ref(name):
    c = sc.case(name)
    return orc.reference(c.cell, c.height, c.gh * c.gw)


def _reduce(dev, c, mode, nodata, cell=None, height=None):
    from satmvs_amd import dsm
    cd = torch.from_numpy(np.array(c.cell if cell is None else cell)).to(dev)
    hd = torch.from_numpy(np.array(c.height if height is None else height)).to(dev)
    ok = (cd >= 0) & (cd < c.gh * c.gw)
    count = torch.bincount(cd[ok].long(), minlength=c.gh * c.gw).to(torch.int32)
    out = dsm.reduce_cells(cd, hd, count, dsm.DSMGrid(0.0, 0.0, 1.0, 1.0, c.gw, c.gh), mode, nodata=nodata)
    assert out.shape == (c.gh, c.gw) and out.dtype == torch.float32
    return out.cpu().numpy().reshape(-1)


def _report(name, figures):
    for tier, (ratio, ulps) in sorted(figures.items()):
        print("MEAN %s | %s | err/delta %.3g | ulps %d" % (name, tier, ratio, ulps))


@pytest.mark.parametrize("name", sc.CASES)
def test_reduce_matrix_against_the_oracle(dev, name):
    c, ref = sc.case(name), _ref(name)
    for nodata in NODATAS:
        for mode in MODES:
            _report(name, orc.check(_reduce(dev, c, mode, nodata), ref, mode, nodata))


@pytest.mark.parametrize("name", sc.PERMUTED_CASES)
def test_bits_unchanged_under_permutation(dev, name):
    c = sc.case(name)
    perm = np.random.default_rng(77).permutation(c.cell.size)
    for mode in MODES:
        a = _reduce(dev, c, mode, -999.0)
        b = _reduce(dev, c, mode, -999.0, c.cell[perm], c.height[perm])
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), mode


@pytest.mark.parametrize("seed", sc.RANDOM_SEEDS)
def test_random_run(dev, seed):
    worst = {}
    for c in sc.random_cases(seed):
        ref = orc.reference(c.cell, c.height, c.gh * c.gw)
        for mode in MODES:
            for tier, (ratio, ulps) in orc.check(_reduce(dev, c, mode, -999.0), ref, mode, -999.0).items():
                worst[tier] = (max(worst.get(tier, (0.0, 0))[0], ratio), max(worst.get(tier, (0.0, 0))[1], ulps))
    _report("random %d" % seed, worst)


# ---- the C entry called directly -------------------------------------------------------------------------------------------------
GUARD = 256                                                  # bytes (workspace) and floats (out) on either side
GUARD_BITS = 0x7fa5a5a5


def _direct(dev, c, mode, nodata=-999.0, big=None):
    """smvs_dsm_reduce on a workspace inside a larger tensor, guard bytes around it and guard words around `out`.  Without
    `big` the workspace is new and pre-filled with 0xff; with it, the call finds whatever the earlier call on `big` left.
    -> (result, the larger tensor); the guards are checked here."""
    from satmvs_amd import _lib, dsm
    n, ncells = c.cell.size, c.gh * c.gw
    nbytes = _lib.load().smvs_dsm_workspace_bytes(n, c.gw, c.gh)
    assert nbytes > 0
    if big is None:
        big = torch.full((nbytes + 2 * GUARD,), 0xff, dtype=torch.uint8, device=dev)
    assert big.numel() >= nbytes + 2 * GUARD
    ws = big[GUARD:GUARD + nbytes]
    big[:GUARD].fill_(0xa5)
    big[GUARD + nbytes:].fill_(0xa5)
    cd, hd = torch.from_numpy(np.array(c.cell)).to(dev), torch.from_numpy(np.array(c.height)).to(dev)
    count = torch.bincount(cd[(cd >= 0) & (cd < ncells)].long(), minlength=ncells).to(torch.int32)
    out_big = torch.full((ncells + 2 * GUARD,), GUARD_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    out = out_big[GUARD:GUARD + ncells]
    _lib.launch(dev, "smvs_dsm_reduce", cd, hd, n, count, c.gw, c.gh, dsm.MODES[mode], float(nodata), out, ws, nbytes)
    torch.cuda.current_stream(dev).synchronize()
    ob = out_big.view(torch.int32)
    assert bool((ob[:GUARD] == GUARD_BITS).all()) and bool((ob[GUARD + ncells:] == GUARD_BITS).all()), "guard words of out"
    assert bool((big[:GUARD] == 0xa5).all()) and bool((big[GUARD + nbytes:] == 0xa5).all()), "guard words of the workspace"
    return out.cpu().numpy(), big


@pytest.mark.parametrize("name", ["tiers mixed", "scan %d" % (sc.CHUNK_CELLS + 1), "sizes 0 to 70"])
def test_c_entry_on_a_guarded_workspace(dev, name):
    c, ref = sc.case(name), _ref(name)
    for mode in MODES:
        got, _ = _direct(dev, c, mode)
        orc.check(got, ref, mode, -999.0)


def test_c_entry_on_a_side_stream(dev):
    c, ref = sc.case("tiers mixed"), _ref("tiers mixed")
    side = torch.cuda.Stream(dev)
    for mode in MODES:
        want, _ = _direct(dev, c, mode)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            got, _ = _direct(dev, c, mode)
        torch.cuda.current_stream(dev).wait_stream(side)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), mode
        orc.check(got, ref, mode, -999.0)


def test_c_entry_twice_on_one_workspace(dev):
    """A larger n and grid first, then a smaller one on the same bytes: stale keys, twins and list counters must not show."""
    first, second = sc.case("tiers mixed"), sc.case("both zeros")
    assert first.cell.size > second.cell.size and first.gh * first.gw > second.gh * second.gw
    for mode in MODES:
        got, big = _direct(dev, first, mode)
        orc.check(got, _ref(first.name), mode, -999.0)
        got, _ = _direct(dev, second, mode, big=big)
        orc.check(got, _ref(second.name), mode, -999.0)
        got, _ = _direct(dev, first, mode, big=big)         # and the larger one again, after the smaller one
        orc.check(got, _ref(first.name), mode, -999.0)


def test_no_points(dev):
    """n = 0 today: reduce_cells on empty tensors is a clean error before any launch (an empty tensor has no address, and the C
    entry rejects null pointers); the C entry itself with n = 0 and real addresses gives a grid of nodata."""
    from satmvs_amd import _lib, dsm
    grid = dsm.DSMGrid(0.0, 0.0, 1.0, 1.0, 5, 3)
    count = torch.zeros(15, dtype=torch.int32, device=dev)
    with pytest.raises((ValueError, _lib.SatMVSNativeError), match="null pointer"):
        dsm.reduce_cells(torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.float32, device=dev), count, grid)
    one_c, one_h = torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, dtype=torch.float32, device=dev)
    nbytes = _lib.load().smvs_dsm_workspace_bytes(0, 5, 3)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xff, dtype=torch.uint8, device=dev)
    for mode in MODES:
        out = torch.zeros(15, dtype=torch.float32, device=dev)
        _lib.launch(dev, "smvs_dsm_reduce", one_c, one_h, 0, count, 5, 3, dsm.MODES[mode], -999.0, out, ws, nbytes)
        assert (out.cpu().numpy() == np.float32(-999.0)).all()


# ---- the bin pass ----------------------------------------------------------------------------------------------------------------
def _bin(dev, h, rpc, mask, grid4, gw, gh, en=True, count=None, tm7=None):
    """One bin call.  -> (cell (H, W) int64, count (gw gh) int64, east, north float64 or None), numpy."""
    from satmvs_amd import dsm
    from satmvs_amd.transverse_mercator import whu_tlc_projection
    H, W = h.shape
    cell = torch.full((H * W,), -7, dtype=torch.int32, device=dev)
    if count is None:
        count = torch.zeros(gw * gh, dtype=torch.int32, device=dev)
    east = torch.full((H, W), 7.0, dtype=torch.float64, device=dev) if en else None
    north = torch.full((H, W), 7.0, dtype=torch.float64, device=dev) if en else None
    md = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).to(dev)
    dsm._bin(torch.from_numpy(np.ascontiguousarray(h, np.float32)).to(dev), torch.from_numpy(rpc).to(dev), md,
             whu_tlc_projection().tm7() if tm7 is None else tm7, np.asarray(grid4, np.float64), gw, gh, cell, count, east, north)
    back = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return cell.cpu().numpy().reshape(H, W).astype(np.int64), count.cpu().numpy().astype(np.int64), back(east), back(north)


def _check_bin(got, cnt, east, north, valid, grid4, gw, gh):
    assert np.array_equal(np.isfinite(east), valid) and np.array_equal(np.isfinite(north), valid)
    assert np.isnan(east[~valid]).all() and np.isnan(north[~valid]).all()
    assert np.array_equal(got, orc.cells(east, north, grid4, gw, gh))
    assert got.min() >= -1 and got.max() < gw * gh
    assert np.array_equal(cnt, np.bincount(got[got >= 0], minlength=gw * gh))


def _middle_grid(east, north, res, lo=10, hi=90):
    from satmvs_amd import dsm
    ok = np.isfinite(east)
    return dsm.grid_from_extent(np.percentile(east[ok], lo), np.percentile(east[ok], hi), np.percentile(north[ok], lo),
                                np.percentile(north[ok], hi), res)


HUGE = (np.array([0.0, 0.0, 1.0e9, 1.0e9]), 1, 1)            # one cell that holds every point


@pytest.mark.parametrize("H,W", sc.BIN_SIZES)
def test_bin_pass_sizes(dev, H, W):
    h, rpc = _scene(H, W, 100 + H + W, nan_share=0.1 if H * W > 1 else 0.0)
    mask = np.random.default_rng(H * W).random((H, W)) > (0.2 if H * W > 1 else 0.0)
    valid = mask & np.isfinite(h)
    _, _, east, north = _bin(dev, h, rpc, mask, *HUGE)
    grid = _middle_grid(east, north, 5.0)
    for g4, gw, gh in ((grid.grid4(), grid.width, grid.height), HUGE):
        got, cnt, e2, n2 = _bin(dev, h, rpc, mask, g4, gw, gh)
        assert np.array_equal(e2, east, equal_nan=True) and np.array_equal(n2, north, equal_nan=True)
        _check_bin(got, cnt, e2, n2, valid, g4, gw, gh)
    assert cnt[0] == valid.sum()
    if H * W > 60:
        assert (got == -1).any()


@pytest.mark.parametrize("H,W", [(53, 41), (1, 257), (128, 64)])
@pytest.mark.parametrize("kind", sc.RUN_MASKS)
def test_bin_pass_run_lengths(dev, kind, H, W):
    """One huge cell: every valid stretch of a wave is one run (one atomic)."""
    h, rpc = _scene(H, W, 7, nan_share=0.0)
    mask = sc.run_mask(kind, H, W)
    got, cnt, east, north = _bin(dev, h, rpc, mask, *HUGE)
    _check_bin(got, cnt, east, north, mask, *HUGE)
    assert cnt.tolist() == [int(mask.sum())] and np.array_equal(got == 0, mask)
    grid = _middle_grid(east, north, 5.0, 0, 100)            # and on cells of a few points: runs of whatever the scene gives
    got, cnt, east, north = _bin(dev, h, rpc, mask, grid.grid4(), grid.width, grid.height)
    _check_bin(got, cnt, east, north, mask, grid.grid4(), grid.width, grid.height)
    assert cnt.sum() == mask.sum()


def test_bin_pass_masks_and_outputs(dev):
    H, W = 37, 41
    h, rpc = _scene(H, W, 8)
    valid = np.isfinite(h)
    _, _, east, north = _bin(dev, h, rpc, None, *HUGE)
    grid = _middle_grid(east, north, 5.0)
    g = (grid.grid4(), grid.width, grid.height)
    want, wcnt, east, north = _bin(dev, h, rpc, None, *g)
    _check_bin(want, wcnt, east, north, valid, *g)
    got, cnt, e2, n2 = _bin(dev, h, rpc, np.ones((H, W), np.uint8), *g)          # no mask = a mask of ones
    assert np.array_equal(got, want) and np.array_equal(cnt, wcnt) and np.array_equal(e2, east, equal_nan=True)
    bytes_ = np.random.default_rng(9).choice(np.array([0, 1, 2, 255], np.uint8), (H, W))          # 2 and 255 count as set
    got, cnt, e2, n2 = _bin(dev, h, rpc, bytes_, *g)
    _check_bin(got, cnt, e2, n2, valid & (bytes_ != 0), *g)
    assert np.array_equal(got, np.where(bytes_ != 0, want, -1))
    got, cnt, e2, n2 = _bin(dev, h, rpc, None, *g, en=False)                     # without east / north
    assert e2 is None and np.array_equal(got, want) and np.array_equal(cnt, wcnt)
    count = torch.zeros(g[1] * g[2], dtype=torch.int32, device=dev)             # two calls into one count add up
    h2, rpc2 = _scene(20, 33, 10)
    a, _, _, _ = _bin(dev, h, rpc, None, *g, count=count)
    b, cnt, _, _ = _bin(dev, h2, rpc2, None, *g, count=count)
    both = np.concatenate([a.reshape(-1), b.reshape(-1)])
    assert (b >= 0).any() and np.array_equal(cnt, np.bincount(both[both >= 0], minlength=g[1] * g[2]))
    far = np.array([grid.e0 + 1.0e6, grid.n0 - 1.0e6, 5.0, 5.0])                 # a grid a long way from the scene
    got, cnt, _, _ = _bin(dev, h, rpc, None, far, 40, 30)
    assert (got == -1).all() and not cnt.any()


def test_bin_pass_non_finite_and_huge_heights(dev):
    H, W = 37, 41
    h, rpc = _scene(H, W, 12, nan_share=0.0)
    _, _, east, north = _bin(dev, h, rpc, None, *HUGE)
    grid = _middle_grid(east, north, 5.0, 0, 100)
    g = (grid.grid4(), grid.width, grid.height)
    rng = np.random.default_rng(13)
    kind = rng.integers(0, 12, (H, W))
    for k, v in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, 1.0e30), (4, -1.0e30)):
        h[kind == k] = np.float32(v)
    got, cnt, east, north = _bin(dev, h, rpc, None, *g)
    bad = kind <= 2
    assert (got[bad] == -1).all() and np.isnan(east[bad]).all() and np.isnan(north[bad]).all()
    assert not np.isnan(east[kind >= 5]).any() and (got[kind >= 5] >= 0).all()
    assert np.array_equal(got, orc.cells(east, north, *g)) and got.min() >= -1 and got.max() < g[1] * g[2]
    assert np.array_equal(cnt, np.bincount(got[got >= 0], minlength=g[1] * g[2]))
    got, cnt, _, _ = _bin(dev, h, rpc, None, *HUGE)          # +-1e30 m: whatever E / N come out, the rule applied to them
    _, _, east, north = _bin(dev, h, rpc, None, *HUGE)
    assert np.array_equal(got, orc.cells(east, north, *HUGE)) and cnt[0] == (got == 0).sum()


def test_bin_pass_pixels_on_cell_edges(dev):
    H, W = 37, 41
    h, rpc = _scene(H, W, 14, nan_share=0.0)
    _, _, east, north = _bin(dev, h, rpc, None, *HUGE)
    p, q = (18, 20), (5, 33)
    grids = sc.edge_grids(east[p], north[p], east[q], north[q])
    by_name = {g.name: g for g in grids}
    assert sc.rule_arguments(east[p], north[p], by_name["p on both lower edges"].grid4) == (0.0, 0.0)
    assert sc.rule_arguments(east[q], north[q], by_name["q on the upper column edge"].grid4)[0] == float(sc.EDGE_GW)
    assert sc.rule_arguments(east[q], north[q], by_name["q on the upper row edge"].grid4)[1] == float(sc.EDGE_GH)
    for g in grids:
        got, cnt, e2, n2 = _bin(dev, h, rpc, None, g.grid4, sc.EDGE_GW, sc.EDGE_GH)
        assert np.array_equal(e2, east) and np.array_equal(n2, north)
        _check_bin(got, cnt, e2, n2, np.ones((H, W), bool), g.grid4, sc.EDGE_GW, sc.EDGE_GH)
        at = got[p] if g.pixel == "p" else got[q]
        assert (at >= 0) == g.on, g.name
        if g.name == "p on both lower edges":
            assert at == 0
        if g.name == "q, e0 one ulp up":
            assert at % sc.EDGE_GW == sc.EDGE_GW - 1
        if g.name == "q, n0 one ulp down":
            assert at // sc.EDGE_GW == sc.EDGE_GH - 1


@pytest.mark.parametrize("res", [5.0, 0.3])
def test_bin_pass_ieee_quotients_on_1e5_points(dev, res):
    H, W = 320, 330
    h, rpc = _scene(H, W, 15)
    _, _, east, north = _bin(dev, h, rpc, None, *HUGE)
    grid = _middle_grid(east, north, res, 2, 98)
    got, cnt, e2, n2 = _bin(dev, h, rpc, None, grid.grid4(), grid.width, grid.height)
    assert H * W > 100000 and (got >= 0).sum() > 90000
    _check_bin(got, cnt, e2, n2, np.isfinite(h), grid.grid4(), grid.width, grid.height)


# ---- smvs_tm_project alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097])
def test_tm_project_alone(dev, proj, tm7, n):
    rng = np.random.default_rng(n)
    ll = np.stack([rng.uniform(29.0, 33.0, n), rng.uniform(-137.0, -133.0, n)], axis=1)
    E, N = orc.tm_forward(tm7, ll[:, 0], ll[:, 1])
    en = proj.proj(ll)
    assert en.shape == (n, 2) and np.abs(en - np.stack([E, N], 1)).max() <= 1e-6
    lat, lon = orc.tm_inverse(tm7, E, N)
    back = proj.proj(np.stack([E, N], 1), reverse=True)
    assert np.abs(back - np.stack([lat, lon], 1)).max() <= 1e-11
    # a non-contiguous input, and a non-contiguous device tensor: equal bits
    wide = np.zeros((n, 2, 3))
    wide[:, :, 1] = ll
    assert np.array_equal(proj.proj(wide[:, :, 1]), en)
    t = torch.from_numpy(wide).to(dev)[:, :, 1]
    out = proj.proj(t)
    assert out.is_cuda and not t.is_contiguous() and np.array_equal(out.cpu().numpy(), en)
    # NaN and +-Inf inputs: non-finite outputs at exactly those points
    for direction, pts in ((False, ll), (True, np.stack([E, N], 1))):
        bad = pts.copy()
        where = rng.random(n) < 0.3
        where[0] = True
        vals = rng.choice([np.nan, np.inf, -np.inf], n)
        col = rng.integers(0, 2, n)
        bad[where, col[where]] = vals[where]
        out = proj.proj(bad, reverse=direction)
        assert np.array_equal(~np.isfinite(out).any(axis=1), where) and np.array_equal(~np.isfinite(out).all(axis=1), where)
        assert np.array_equal(out[~where], (back if direction else en)[~where])


# ---- heights_to_dsm end to end ---------------------------------------------------------------------------------------------------
def _check_dsm(got, cnt, heights, rpcs, proj, grid, masks, mode, nodata=-999.0):
    """got / cnt of heights_to_dsm against the reference on numpy binning of the GPU's own E / N."""
    from satmvs_amd import dsm
    en = dsm.project_to_map(heights, rpcs, proj, masks)
    cells = np.concatenate([orc.cells(e.cpu().numpy(), n.cpu().numpy(), grid.grid4(), grid.width, grid.height).reshape(-1) for e, n in en])
    hs = np.concatenate([np.asarray(h).astype(np.float32).reshape(-1) for h in heights])
    ref = orc.reference(cells, hs, grid.width * grid.height)
    assert got.shape == (grid.height, grid.width) and got.dtype == np.float32
    assert np.array_equal(np.asarray(cnt).reshape(-1), ref.count) and ref.count.max() > 1 and (ref.count == 0).any()
    orc.check(got, ref, mode, nodata)


@pytest.fixture(scope="module")
def three_maps():
    maps = [_scene(60, 90, s) for s in (51, 52, 53)]
    return np.stack([h for h, _ in maps]), [r for _, r in maps]


def _cut_grid(hs, rs, proj):
    from satmvs_amd import dsm
    full = dsm.grid_for(list(hs), rs, proj, 5.0)
    return dsm.DSMGrid(full.e0 + 20.0, full.n0 - 20.0, 5.0, 5.0, full.width - 2, full.height + 3)


def test_heights_to_dsm_stacked_maps(dev, proj, three_maps):
    from satmvs_amd import dsm
    hs, rs = three_maps
    grid = _cut_grid(hs, rs, proj)
    for mode in MODES:
        got, cnt = dsm.heights_to_dsm(hs, rs, proj, grid, mode=mode, return_count=True)           # one (3, H, W) array
        _check_dsm(got, cnt, list(hs), rs, proj, grid, None, mode)


@pytest.mark.parametrize("dtype", [np.float64, np.float16])
def test_heights_to_dsm_converts_other_dtypes(dev, proj, three_maps, dtype):
    from satmvs_amd import dsm
    hs, rs = three_maps
    hs = (hs.astype(np.float64) + 1.0e-7).astype(dtype)       # float64 heights that are no float32
    grid = _cut_grid(hs.astype(np.float32), rs, proj)
    for mode in MODES:
        got, cnt = dsm.heights_to_dsm(list(hs), rs, proj, grid, mode=mode, return_count=True)
        _check_dsm(got, cnt, list(hs.astype(np.float32)), rs, proj, grid, None, mode)


def test_heights_to_dsm_non_contiguous_tensors_and_a_side_stream(dev, proj, three_maps):
    from satmvs_amd import dsm
    hs, rs = three_maps
    grid = _cut_grid(hs, rs, proj)
    wide = torch.from_numpy(np.repeat(hs, 2, axis=2)).to(dev)
    views = [wide[i, :, ::2] for i in range(3)]
    masks = [torch.from_numpy(np.random.default_rng(i).random(hs[i].shape) > 0.2).to(dev).t().contiguous().t() for i in range(3)]
    assert not any(v.is_contiguous() for v in views) and not any(m.is_contiguous() for m in masks)
    side = torch.cuda.Stream(dev)
    for mode in MODES:
        got, cnt = dsm.heights_to_dsm(views, rs, proj, grid, masks=masks, mode=mode, return_count=True)
        assert got.is_cuda and cnt.is_cuda
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            again = dsm.heights_to_dsm(views, rs, proj, grid, masks=masks, mode=mode)
        torch.cuda.current_stream(dev).wait_stream(side)
        got, cnt, again = got.cpu().numpy(), cnt.cpu().numpy(), again.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), mode
        _check_dsm(got, cnt, list(hs), rs, proj, grid, [m.cpu().numpy() for m in masks], mode)
