"""Orthophotos on the MI355X (dsm.visibility / dsm.orthorectify / smvs_rpc_ortho): the numpy oracle per view with occlusion on
and off, image coordinates on a flat DSM, occlusion behind a block, the mosaic rule in every order, holes, tiles, determinism,
channel counts and one 2048 x 2048 view."""
import numpy as np
import pytest
import torch

import dsm_render_oracle as ro
import ortho_oracle as oo
from dsm_testkit import dev, proj, scene, views_fixture  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

H, W = 128, 160
views = views_fixture(H, W, seed=11)


def _image(shape, C, seed):
    return np.random.default_rng(seed).uniform(0.0, 255.0, tuple(shape) + (C,)).astype(np.float32)


def _scene(grid):
    return scene(*ro.cell_centres(grid))


def _agree_states(got, o, shape):
    """State maps equal except at borderline cells (oracle |f - occ_tol| < 1e-6 m, u or v within 1e-9 px of a border); at most
    1e-4 of the cells may be excepted."""
    bad = got != o["state"]
    excepted = bad & oo.borderline(o, shape)
    assert not (bad & ~excepted).any(), (int(bad.sum()), int(excepted.sum()))
    assert excepted.sum() <= 1e-4 * got.size
    return ~bad


def _agree_values(got, o, where):
    """|got - oracle| <= 1e-5 of the taps' range plus one float32 ulp, channel by channel, at `where`."""
    want = o["value"][where].astype(np.float64)
    g = got[where].astype(np.float64)
    lim = 1e-5 * o["tap_range"][where] + np.spacing(np.abs(o["value"][where])).astype(np.float64)
    assert np.isfinite(g).all() and (np.abs(g - want) <= lim).all(), float(np.abs(g - want).max())


@pytest.mark.parametrize("occlusion", [True, False])
@pytest.mark.parametrize("shift", [0.0, 0.4, -0.4])
def test_against_the_oracle(dev, proj, views, shift, occlusion):
    from satmvs_amd import dsm
    rpc = views[shift]
    tm7 = proj.tm7()
    grid = ro.grid_over([(rpc, (H, W))], tm7, 100.0, 160.0, 5.0, margin=20.0)
    z = _scene(grid)
    img = _image((H, W), 3, seed=5)
    vis = dsm.visibility(z, grid, rpc, proj, (H, W), occlusion=occlusion)
    assert vis.dtype == np.uint8 and vis.shape == (grid.height, grid.width)
    o = oo.ortho(z, grid, -999.0, tm7, rpc, img, occlusion=occlusion)
    same = _agree_states(vis, o, (H, W))
    counts = np.bincount(vis.reshape(-1), minlength=4)
    assert counts[0] == 3 * 2 + 2 * 4 and counts[1] > 100 and counts[3] > 1000
    assert (counts[2] > 5) == (occlusion and shift != 0.0)
    ortho, src = dsm.orthorectify(img, rpc, z, grid, proj, occlusion=occlusion, return_source=True)
    assert ortho.dtype == np.float32 and ortho.shape == (grid.height, grid.width, 3)
    assert src.dtype == np.int32 and np.array_equal(src == 0, vis == oo.VISIBLE) and (src[vis != oo.VISIBLE] == -1).all()
    assert np.isnan(ortho[src < 0]).all()
    _agree_values(ortho, o, same & (vis == oo.VISIBLE))


def test_flat_dsm_returns_image_coordinates(dev, proj, views):
    from satmvs_amd import dsm, rpc_synth
    import dsm_oracle
    rpc = views[0.4]
    tm7 = proj.tm7()
    grid = ro.grid_over([(rpc, (H, W))], tm7, 130.0, 130.0, 5.0, margin=20.0)
    z = np.full((grid.height, grid.width), 130.0, np.float32)
    i, j = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.stack([j, i], axis=-1)                                          # I0 = x (column), I1 = y (row)
    ortho, src = dsm.orthorectify(img, rpc, z, grid, proj, return_source=True)
    seen = src == 0
    assert seen.sum() > 500 and (~seen).sum() > 100
    E, N = ro.cell_centres(grid)
    lat, lon = dsm_oracle.tm_inverse(tm7, E[seen], N[seen])
    x, y = rpc_synth.obj2photo(rpc, lat, lon, np.full(lat.shape, 130.0))
    assert np.abs(ortho[seen][:, 0] - x).max() <= 1e-4
    assert np.abs(ortho[seen][:, 1] - y).max() <= 1e-4


def _block_geometry(grid, tm7, rpc, z_ground, height, rows, cols, H_, W_):
    """Per ground cell: the ray's travel (du, dv) [cells] from z_ground to z_ground + height, and (u, v) in the view."""
    from satmvs_amd import rpc_synth
    import dsm_oracle
    E, N = ro.cell_centres(grid)
    lat, lon = dsm_oracle.tm_inverse(tm7, E, N)
    x, y = rpc_synth.obj2photo(rpc, lat, lon, np.full(E.shape, z_ground))
    e1, n1 = ro.G(rpc, tm7, x, y, np.full(E.shape, z_ground + height))
    return (e1 - E) / grid.xres, (N - n1) / grid.yres, x, y


def _swept(rows, cols, du, dv, r_lo, r_hi, c_lo, c_hi, t0, t1, n=256):
    """Cells from which the ray, between travel fractions t0 and t1, enters the box [r_lo, r_hi] x [c_lo, c_hi] (cell units)."""
    hit = np.zeros(rows.shape, bool)
    for t in np.linspace(t0, t1, n):
        cc, rr = cols + t * du, rows + t * dv
        hit |= (cc >= c_lo) & (cc <= c_hi) & (rr >= r_lo) & (rr <= r_hi)
    return hit


def test_occlusion_known_answer(dev, proj, views):
    from satmvs_amd import dsm
    tm7 = proj.tm7()
    res, nb, top = 2.0, 10, 40.0
    for shift in (0.0, 0.4):
        rpc = views[shift]
        grid = ro.grid_over([(rpc, (H, W))], tm7, 100.0, 140.0, res, margin=10.0)
        z = np.full((grid.height, grid.width), 100.0, np.float32)
        r0, c0 = grid.height // 2 - nb // 2, grid.width // 2 - nb // 2
        z[r0:r0 + nb, c0:c0 + nb] = 100.0 + top
        st = dsm.visibility(z, grid, rpc, proj, (H, W))
        rows, cols = np.mgrid[0:grid.height, 0:grid.width].astype(np.float64)
        du, dv, x, y = _block_geometry(grid, tm7, rpc, 100.0, top, rows, cols, H, W)
        ground = z == 100.0
        inside = (x >= 1) & (x <= W - 2) & (y >= 1) & (y <= H - 2)
        assert (st[r0:r0 + nb, c0:c0 + nb] == oo.VISIBLE).all()                   # the roof
        if shift == 0.0:
            assert not (st == oo.OCCLUDED).any()
            assert (st[ground & inside] == oo.VISIBLE).all()
            continue
        L = np.hypot(du, dv)
        assert (np.abs(L * res - top * shift) <= 0.1 * top * shift).all()        # the strip's length: height x shift
        # the hidden strip: the ray enters the roof shrunk by 2 cells at travel fractions [2 / L, 1 - 2 / L] (the strip's ends
        # excluded), where it lies more than 10 m under the roof; every march sample is within half a cell of any point of the ray
        m = 2.0 / L.min()
        strip = ground & inside & _swept(rows, cols, du, dv, r0 + 2, r0 + nb - 3, c0 + 2, c0 + nb - 3, m, 1.0 - m)
        assert strip.sum() >= 20
        assert (st[strip] == oo.OCCLUDED).all()
        assert cols[strip].min() > c0 + nb - 1                                   # the sensor's side is west: the strip is east
        # clear ground: more than 2 cells from the block's bilinear footprint and from its strip
        near = _swept(rows, cols, du, dv, r0 - 3, r0 + nb + 2, c0 - 3, c0 + nb + 2, 0.0, 1.0)
        clear = ground & inside & ~near
        assert clear.sum() > 1000
        assert (st[clear] == oo.VISIBLE).all()


def test_mosaic_rule(dev, proj):
    from satmvs_amd import dsm
    tm7 = proj.tm7()
    shifts = (0.4, -0.25)                                                        # opposite views, view 1 nearer nadir
    rpcs = [ro.view_rpc(H, W, s, seed=13) for s in shifts]
    res = 2.0
    grid = ro.grid_over([(r, (H, W)) for r in rpcs], tm7, 100.0, 140.0, res, margin=10.0)
    z = np.full((grid.height, grid.width), 100.0, np.float32)
    r0, c0 = grid.height // 2 - 5, grid.width // 2 - 8
    z[r0:r0 + 10, c0:c0 + 6] = 140.0                                             # two blocks and a 6 m street between them
    z[r0:r0 + 10, c0 + 9:c0 + 15] = 140.0
    imgs = [_image((H, W), 3, seed=20 + v) for v in range(2)]
    vis = [dsm.visibility(z, grid, r, proj, (H, W)) for r in rpcs]
    singles = [dsm.orthorectify(imgs[v], rpcs[v], z, grid, proj, return_source=True) for v in range(2)]
    assert dsm.nadir_order(rpcs, grid, proj, 140.0) == [1, 0]
    hidden = (vis[0] == oo.OCCLUDED) & (vis[1] == oo.OCCLUDED)
    assert hidden.sum() >= 5                                                     # the street
    results = {}
    for order, seq in (("given", [0, 1]), ([1, 0], [1, 0]), ("nadir", [1, 0])):
        o, src = dsm.orthorectify(imgs, rpcs, z, grid, proj, order=order, return_source=True)
        want = np.full(src.shape, -1, np.int32)
        for v in reversed(seq):
            want[vis[v] == oo.VISIBLE] = v
        assert np.array_equal(src, want)
        for v in range(2):
            sel = src == v
            assert sel.sum() > 100
            assert np.array_equal(o[sel].view(np.uint32), singles[v][0][sel].view(np.uint32))
        assert np.isnan(o[src < 0]).all() and (src[hidden] == -1).all()
        results[str(order)] = (o, src)
    assert np.array_equal(results["nadir"][1], results["[1, 0]"][1])
    assert (results["given"][1] != results["nadir"][1]).sum() > 50                # the order matters where both views see
    o1, s1 = dsm.orthorectify([imgs[0]], [rpcs[0]], z, grid, proj, return_source=True)
    assert np.array_equal(o1.view(np.uint32), singles[0][0].view(np.uint32)) and np.array_equal(s1, singles[0][1])


def test_holes_keep_fill(dev, proj, views):
    from satmvs_amd import dsm
    rpc = views[0.4]
    grid = ro.grid_over([(rpc, (H, W))], proj.tm7(), 100.0, 160.0, 5.0, margin=20.0)
    z = _scene(grid)
    holes = ~np.isfinite(z) | (z == -999.0)
    assert holes.sum() == 14
    st = dsm.visibility(z, grid, rpc, proj, (H, W))
    assert np.array_equal(st == oo.NO_HEIGHT, holes)
    o, src = dsm.orthorectify(_image((H, W), 2, seed=3), rpc, z, grid, proj, fill=-7.0, return_source=True)
    assert (o[holes] == -7.0).all() and (src[holes] == -1).all()
    assert (o[src < 0] == -7.0).all()
    # nodata = NaN: -999 cells are heights then (and far below the view: they project outside it)
    st_nan = dsm.visibility(z, grid, rpc, proj, (H, W), nodata=float("nan"))
    assert np.array_equal(st_nan == oo.NO_HEIGHT, ~np.isfinite(z))
    with pytest.raises(ValueError, match="no valid cell"):
        dsm.visibility(np.full_like(z, -999.0), grid, rpc, proj, (H, W))
    with pytest.raises(ValueError, match="no valid cell"):
        dsm.orthorectify(_image((H, W), 1, seed=3), rpc, np.full_like(z, np.nan), grid, proj)


def test_tiles(dev, proj, views):
    from satmvs_amd import dsm
    rpc = views[-0.4]
    tm7 = proj.tm7()
    grid = ro.grid_over([(rpc, (H, W))], tm7, 100.0, 160.0, 5.0, margin=20.0)
    z = _scene(grid)
    img = _image((H, W), 3, seed=8)
    whole, wsrc = dsm.orthorectify(img, rpc, z, grid, proj, return_source=True)
    wst = dsm.visibility(z, grid, rpc, proj, (H, W))
    o = oo.ortho(z, grid, -999.0, tm7, rpc, shape=(H, W))
    x0, y0, th, tw = 40, 30, 64, 80
    tile, tsrc = dsm.orthorectify(img[y0:y0 + th, x0:x0 + tw], rpc, z, grid, proj, origins=(x0, y0), return_source=True)
    tst = dsm.visibility(z, grid, rpc, proj, (th, tw), origin=(x0, y0))
    u, v = o["u"] - x0, o["v"] - y0
    eps = 1e-6
    with np.errstate(invalid="ignore"):
        within = (u >= eps) & (u <= tw - 1 - eps) & (v >= eps) & (v <= th - 1 - eps)
        beyond = (u < -eps) | (u > tw - 1 + eps) | (v < -eps) | (v > th - 1 + eps)
    has = wst != oo.NO_HEIGHT
    assert (within & has).sum() > 200 and (beyond & has).sum() > 200
    assert np.array_equal(tst[within], wst[within])
    assert (tst[beyond & has] == oo.OUTSIDE).all()
    seen = within & (tst == oo.VISIBLE)
    assert np.array_equal(tsrc == 0, tst == oo.VISIBLE) and np.array_equal(wsrc[seen], tsrc[seen])
    assert np.array_equal(tile[seen].view(np.uint32), whole[seen].view(np.uint32))


def test_deterministic_on_device_tensors(dev, proj, views):
    from satmvs_amd import dsm
    rpcs = [views[s] for s in (0.4, 0.0, -0.4)]
    grid = ro.grid_over([(r, (H, W)) for r in rpcs], proj.tm7(), 100.0, 160.0, 5.0, margin=10.0)
    z = torch.from_numpy(_scene(grid)).to(dev)
    imgs = [torch.from_numpy(_image((H, W), 4, seed=30 + v)).to(dev) for v in range(3)]
    rd = [torch.from_numpy(r).to(dev) for r in rpcs]
    a, sa = dsm.orthorectify(imgs, rd, z, grid, proj, return_source=True)
    b, sb = dsm.orthorectify(imgs, rd, z, grid, proj, return_source=True)
    assert a.is_cuda and a.dtype == torch.float32 and a.shape == (grid.height, grid.width, 4) and sa.dtype == torch.int32
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(sa, sb)
    assert set(torch.unique(sa).tolist()) == {-1, 0, 1, 2}
    v1 = dsm.visibility(z, grid, rd[0], proj, (H, W))
    v2 = dsm.visibility(z, grid, rd[0], proj, (H, W))
    assert v1.is_cuda and torch.equal(v1, v2)


@pytest.mark.parametrize("C", [1, 3, 4, 16])
def test_channel_counts(dev, proj, views, C):
    from satmvs_amd import dsm
    rpc = views[0.4]
    tm7 = proj.tm7()
    grid = ro.grid_over([(rpc, (H, W))], tm7, 100.0, 160.0, 5.0, margin=20.0)
    z = _scene(grid)
    img = _image((H, W), C, seed=40 + C)
    if C == 1:
        img = img[:, :, 0]                                                       # (H, W) is one channel
    ortho, src = dsm.orthorectify(img, rpc, z, grid, proj, return_source=True)
    assert ortho.shape == (grid.height, grid.width, C)
    vis = dsm.visibility(z, grid, rpc, proj, (H, W))
    assert np.array_equal(src == 0, vis == oo.VISIBLE)
    o = oo.ortho(z, grid, -999.0, tm7, rpc, img)
    same = _agree_states(vis, o, (H, W))
    _agree_values(ortho, o, same & (vis == oo.VISIBLE))


def test_large_view(dev, proj):
    from satmvs_amd import dsm
    S, res = 2048, 4.5
    rpc = ro.view_rpc(S, S, 0.4, seed=31)
    tm7 = proj.tm7()
    g = ro.grid_over([(rpc, (S, S))], tm7, 100.0, 200.0, res)
    assert g.width <= 1000 and g.height <= 1000
    grid = type(g)(g.e0 - res * ((1000 - g.width) // 2), g.n0 + res * ((1000 - g.height) // 2), res, res, 1000, 1000)
    E, N = ro.cell_centres(grid)
    z = (140.0 + 30.0 * np.sin(E / 150.0) * np.cos(N / 190.0)).astype(np.float32)
    z[(np.floor(E / 60.0) % 5 == 0) & (np.floor(N / 60.0) % 4 == 0)] += 25.0                # blocks
    img = _image((S, S), 3, seed=9)
    st = dsm.visibility(z, grid, rpc, proj, (S, S))
    ortho, src = dsm.orthorectify(img, rpc, z, grid, proj, return_source=True)
    counts = np.bincount(st.reshape(-1), minlength=4)
    assert counts[2] > 1000 and counts[3] > 500000 and counts[1] > 1000
    assert np.array_equal(src == 0, st == oo.VISIBLE)
    rows, cols = np.mgrid[8:1000:16, 8:1000:16]                                   # 63 x 63 cells
    o = oo.ortho(z, grid, -999.0, tm7, rpc, img, rows=rows, cols=cols)
    same = _agree_states(st[8::16, 8::16], o, (S, S))
    _agree_values(ortho[8::16, 8::16], o, same & (st[8::16, 8::16] == oo.VISIBLE))
