"""Rendering a DSM into a view on the MI355X (dsm.render_heights / smvs_rpc_dsm_render): the numpy oracle on terrain and on a
block with holes, known answers (plane, occlusion), the crossing property, holes at nadir, the DSM -> heights -> DSM round
trip, determinism and tiles, and one 2048 x 2048 view."""
import numpy as np
import pytest
import torch

import dsm_render_oracle as ro
from dsm_testkit import dev, proj, scene, views_fixture  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

H, W = 128, 160
TOL = 1e-3
views = views_fixture(H, W, seed=11)


def _terrain(grid, base=130.0, amp=20.0):
    return scene(*ro.cell_centres(grid), blocks=False, holes=False, base=base, amp=amp)


def _agree(got, o, tol=TOL):
    """Validity masks equal and |got - oracle| <= tol, except at pixels whose deciding oracle |f| is below 1e-6 m (a sample
    whose sign device and numpy arithmetic may round differently); at most 1e-4 of the pixels may be excepted."""
    want = o["height"]
    vg, vw = np.isfinite(got), np.isfinite(want)
    with np.errstate(invalid="ignore"):
        bad = (vg != vw) | (vg & vw & ~(np.abs(got.astype(np.float64) - want) <= tol))
    excepted = bad & (np.abs(o["f_decide"]) < 1e-6)
    assert not (bad & ~excepted).any(), (int(bad.sum()), int(excepted.sum()))
    assert excepted.sum() <= 1e-4 * got.size
    return vw


def _f(z, grid, nodata, proj, rpc, x, y, h):
    e, n = ro.G(rpc, proj.tm7(), x, y, h)
    ok, S = ro.surface(z, grid.grid4(), nodata, e, n)
    return ok, S - h


def test_against_the_oracle(dev, proj, views):
    from satmvs_amd import dsm
    rpc = views[0.4]
    tm7 = proj.tm7()
    grid = ro.grid_over([(rpc, (H, W))], tm7, 100.0, 160.0, 5.0, margin=-10.0)      # some rays leave the grid
    # (a) smooth terrain
    za = _terrain(grid)
    got = dsm.render_heights(za, grid, rpc, proj, (H, W))
    o = ro.render_view(za, grid, -999.0, tm7, rpc, H, W)
    assert got.dtype == np.float32 and got.shape == (H, W)
    valid = _agree(got, o)
    assert 0.5 < valid.mean() < 1.0
    # (b) flat ground, a block, NaN and nodata holes next to it
    zb = np.full((grid.height, grid.width), 100.0, np.float32)
    r0, c0 = grid.height // 2 - 3, grid.width // 2 - 3
    zb[r0:r0 + 6, c0:c0 + 6] = 150.0
    zb[r0:r0 + 3, c0 + 6:c0 + 8] = np.nan
    zb[r0 + 6:r0 + 8, c0:c0 + 4] = -999.0
    zb[2, 2] = 160.0                                                             # the bracket's top, in a corner
    got = dsm.render_heights(zb, grid, rpc, proj, (H, W))
    o = ro.render_view(zb, grid, -999.0, tm7, rpc, H, W)
    valid = _agree(got, o)
    assert (~valid).sum() > 200 and valid.mean() > 0.5
    assert (np.abs(got[valid] - 150.0) <= TOL).sum() > 20 and (np.abs(got[valid] - 100.0) <= TOL).sum() > 1000


@pytest.mark.parametrize("shift", [0.0, 0.4, -0.4])
def test_planar_dsm_known_answer(dev, proj, views, shift):
    from satmvs_amd import dsm
    rpc = views[shift]
    tm7 = proj.tm7()
    grid = ro.grid_over([(rpc, (H, W))], tm7, 60.0, 240.0, 5.0, margin=20.0)
    E, N = ro.cell_centres(grid)
    Ec, Nc = E.mean(), N.mean()

    def plane(e, n):
        return 150.0 + 0.15 * (e - Ec) - 0.11 * (n - Nc)

    got = dsm.render_heights(plane(E, N).astype(np.float32), grid, rpc, proj, (H, W)).astype(np.float64)
    assert np.isfinite(got).all()
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    e, n = ro.G(rpc, tm7, x, y, got)
    assert np.abs(plane(e, n) - got).max() <= 1e-3


def test_occlusion_known_answer(dev, proj, views):
    from satmvs_amd import dsm
    rpc = views[0.4]
    tm7 = proj.tm7()
    res = 5.0
    grid = ro.grid_over([(rpc, (H, W))], tm7, 100.0, 160.0, res, margin=20.0)
    z = np.full((grid.height, grid.width), 100.0, np.float32)
    r0, c0 = grid.height // 2 - 3, grid.width // 2 - 3
    z[r0:r0 + 6, c0:c0 + 6] = 160.0
    got = dsm.render_heights(z, grid, rpc, proj, (H, W))
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)

    def uv(h):
        e, n = ro.G(rpc, tm7, x, y, np.full(x.shape, h))
        return (e - grid.e0) / res, (grid.n0 - n) / res, e

    u100, v100, e100 = uv(100.0)
    u160, v160, e160 = uv(160.0)
    eps = 1e-6
    # rays that meet the flat top at 160: its interior is u in [c0, c0 + 5], v in [r0, r0 + 5] (cell centres)
    top = (u160 >= c0 + eps) & (u160 <= c0 + 5 - eps) & (v160 >= r0 + eps) & (v160 <= r0 + 5 - eps)
    assert top.sum() > 20
    assert (np.abs(got[top] - 160.0) <= 1e-3).all()
    # the shadow band: the view moves west with height (u160 < u100), so the band lies east of the block's bilinear footprint
    # (u < c0 + 6).  Rays whose ground point at 100 lies more than one cell and less than 60 * shift - 2 res past it, and whose
    # path stays within the flat top's rows, must see the top or the ramp.
    assert (u160 < u100).all()
    shift = np.abs(e160 - e100) / 60.0
    d = (u100 - (c0 + 6)) * res
    lateral = (np.minimum(v100, v160) >= r0 + eps) & (np.maximum(v100, v160) <= r0 + 5 - eps)
    shadow = lateral & (d > res) & (d < 60.0 * shift - 2 * res)
    assert shadow.sum() > 5
    assert (got[shadow] > 101.0).all()
    # ground clear of the block: the ray's path from 100 to 160 stays more than a cell from the footprint
    def clear(u, v):
        return (u < c0 - 2) | (u > c0 + 7) | (v < r0 - 2) | (v > r0 + 7)
    same_side = ((u100 < c0 - 2) & (u160 < c0 - 2)) | ((u100 > c0 + 7) & (u160 > c0 + 7)) | \
                ((v100 < r0 - 2) & (v160 < r0 - 2)) | ((v100 > r0 + 7) & (v160 > r0 + 7))
    ground = same_side & clear(u100, v100) & clear(u160, v160)
    assert ground.sum() > 1000
    assert (np.abs(got[ground] - 100.0) <= 1e-3).all()


def test_hit_is_the_visible_crossing(dev, proj, views):
    from satmvs_amd import dsm
    rpc = views[-0.4]
    tm7 = proj.tm7()
    grid = ro.grid_over([(rpc, (H, W))], tm7, 100.0, 160.0, 5.0, margin=20.0)
    z = _terrain(grid)
    h_lo, h_hi = ro.h_range(z, -999.0)
    got = dsm.render_heights(z, grid, rpc, proj, (H, W)).astype(np.float64)
    v = np.isfinite(got)
    assert v.mean() > 0.99
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    x, y, h = x[v], y[v], got[v]
    ok_up, f_up = _f(z, grid, -999.0, proj, rpc, x, y, h + TOL)
    ok_dn, f_dn = _f(z, grid, -999.0, proj, rpc, x, y, h - TOL)
    assert ok_up.all() and ok_dn.all()
    assert (f_up < 0.0).all() and (f_dn >= 0.0).all()
    for t in np.linspace(0.0, 1.0, 65)[1:]:                                   # 64 heights in (h + tol, h_hi]
        hp = (h + TOL) + t * (h_hi - (h + TOL))
        ok, f = _f(z, grid, -999.0, proj, rpc, x, y, hp)
        sel = hp > h + TOL
        assert (ok[sel] & (f[sel] < 0.0)).all()


def test_holes_near_nadir(dev, proj, views):
    from satmvs_amd import dsm
    rpc = views[0.0]
    tm7 = proj.tm7()
    grid = ro.grid_over([(rpc, (H, W))], tm7, 100.0, 160.0, 5.0, margin=20.0)
    z = _terrain(grid)
    zh = z.copy()
    r0, c0 = grid.height // 2 - 2, grid.width // 2 - 2
    zh[r0:r0 + 4, c0:c0 + 4] = -999.0
    assert ro.h_range(zh, -999.0) == ro.h_range(z, -999.0)               # the same bracket, hence the same samples
    free = dsm.render_heights(z, grid, rpc, proj, (H, W))
    holed = dsm.render_heights(zh, grid, rpc, proj, (H, W))
    o = ro.render_view(z, grid, -999.0, tm7, rpc, H, W, keep_samples=True)
    assert (o["K"] == 1).all()                                               # less than half a cell of travel

    def touches(E, N):
        """Whether the 2x2 bilinear support of each point includes a patch cell (NaN points: False)."""
        with np.errstate(invalid="ignore"):
            cu = np.floor((E - grid.e0) / grid.xres)
            cv = np.floor((grid.n0 - N) / grid.yres)
            return (cu >= c0 - 1) & (cu <= c0 + 3) & (cv >= r0 - 1) & (cv <= r0 + 3)

    clear = ~touches(o["E"], o["N"]).any(axis=0)
    assert clear.sum() > 1000
    assert np.array_equal(holed[clear].view(np.uint32), free[clear].view(np.uint32))
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    e, n = ro.G(rpc, tm7, x, y, free.astype(np.float64))
    hit = touches(e, n)
    assert hit.sum() > 20
    assert np.isnan(holed[hit]).all()


def test_round_trip_through_heights_to_dsm(dev, proj):
    from satmvs_amd import dsm
    S = 512
    rpcs = [ro.view_rpc(S, S, s, seed=21) for s in (0.0, 0.4, -0.4)]
    tm7 = proj.tm7()
    grid = ro.grid_over([(r, (S, S)) for r in rpcs], tm7, 100.0, 160.0, 5.0, margin=10.0)
    E, N = ro.cell_centres(grid)
    z = (130.0 + 10.0 * np.sin(E / 80.0) + 8.0 * np.cos(N / 70.0)).astype(np.float32)    # |grad| <= 0.166 <= slope_max
    slope_max = 0.2
    heights = [dsm.render_heights(z, grid, r, proj, (S, S)) for r in rpcs]
    for h in heights:
        assert np.isfinite(h).mean() > 0.95
    fused, cnt = dsm.heights_to_dsm(heights, rpcs, proj, grid, mode="median", nodata=-999.0, return_count=True)
    ok = fused != -999.0
    nb = np.ones_like(ok)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            sh = np.zeros_like(ok)
            sh[max(dr, 0):ok.shape[0] + min(dr, 0), max(dc, 0):ok.shape[1] + min(dc, 0)] = \
                ok[max(-dr, 0):ok.shape[0] + min(-dr, 0), max(-dc, 0):ok.shape[1] + min(-dc, 0)]
            nb &= sh
    sel = (cnt >= 3) & nb
    assert sel.sum() > 5000
    err = np.abs(fused[sel].astype(np.float64) - z[sel])
    assert err.max() <= slope_max * (np.sqrt(2.0) / 2.0) * grid.xres + 0.01, float(err.max())


def test_deterministic_and_tiles(dev, proj, views):
    from satmvs_amd import dsm
    rpc = views[0.4]
    grid = ro.grid_over([(rpc, (H, W))], proj.tm7(), 100.0, 160.0, 5.0, margin=-10.0)
    z = _terrain(grid)
    zd, rd = torch.from_numpy(z).to(dev), torch.from_numpy(rpc).to(dev)
    a = dsm.render_heights(zd, grid, rd, proj, (H, W))
    b = dsm.render_heights(zd, grid, rd, proj, (H, W))
    assert a.is_cuda and a.dtype == torch.float32 and a.shape == (H, W)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert bool(torch.isnan(a).any()) and bool(torch.isfinite(a).any())     # the grid is cut: both kinds of pixel
    for y0, x0, th, tw in ((0, 0, 64, 80), (0, 80, 64, 80), (64, 0, 64, 80), (64, 80, 64, 80)):
        t = dsm.render_heights(zd, grid, rd, proj, (th, tw), origin=(x0, y0))
        assert torch.equal(t.view(torch.int32), a[y0:y0 + th, x0:x0 + tw].contiguous().view(torch.int32))
    n = dsm.render_heights(z, grid, rpc, proj, (H, W))
    assert isinstance(n, np.ndarray) and np.array_equal(n.view(np.uint32), a.cpu().numpy().view(np.uint32))
    with pytest.raises(ValueError, match="no valid cell"):
        dsm.render_heights(np.full_like(z, -999.0), grid, rpc, proj, (H, W))


def test_large_view(dev, proj):
    from satmvs_amd import dsm
    S = 2048
    rpc = ro.view_rpc(S, S, 0.4, seed=31)
    tm7 = proj.tm7()
    g = ro.grid_over([(rpc, (S, S))], tm7, 100.0, 200.0, 7.5)
    assert g.width <= 600 and g.height <= 600
    grid = type(g)(g.e0 - 7.5 * ((600 - g.width) // 2), g.n0 + 7.5 * ((600 - g.height) // 2), 7.5, 7.5, 600, 600)
    E, N = ro.cell_centres(grid)
    z = (140.0 + 30.0 * np.sin(E / 150.0) * np.cos(N / 190.0)).astype(np.float32)
    z[(np.floor(E / 60.0) % 5 == 0) & (np.floor(N / 60.0) % 4 == 0)] += 25.0                # blocks
    got = dsm.render_heights(z, grid, rpc, proj, (S, S))
    assert got.shape == (S, S) and np.isfinite(got).mean() > 0.9
    ys, xs = np.mgrid[16:S:32, 16:S:32].astype(np.float64)                               # 64 x 64 = 4096 pixels
    o = ro.render(z, grid.grid4(), -999.0, tm7, rpc, xs, ys)
    _agree(got[16::32, 16::32], o)
