"""DSM production on the MI355X: Transverse Mercator against the reference's outputs, the bin pass against numpy, the reduce
against a per-cell np.lexsort oracle (every sort tier, one cell of more than 4 M points), determinism under reruns and map
order, a known answer, and the filter -> DSM chain."""
import numpy as np
import pytest
import torch

import dsm_oracle as orc
from dsm_testkit import dev  # noqa: F401  (fixtures)

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
