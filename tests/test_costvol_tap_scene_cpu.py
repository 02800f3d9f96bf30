"""The scenes of tests/costvol_tap_scene.py have the properties they are named for (CPU: the oracle's float64 source coordinates)."""
import numpy as np

import costvol_tap_scene as cts

BW, R = 44, 5          # staged box of the per-wave instances (costvol_kernels.h: DM_BW, DM_R)


def _patches(H, W):
    for y0 in range(0, H, 2):
        for x0 in range(0, W, 32):
            yield slice(y0, min(y0 + 2, H)), slice(x0, min(x0 + 32, W))


def _inside(ix, iy, H, W):
    return (ix >= -1) & (ix <= W - 1) & (iy >= -1) & (iy <= H - 1)


def test_saturation_scene(oracle):
    for nan_voxel in (False, True):
        sc = cts.saturation(nan_voxel)
        ix, iy = cts.cells(oracle, sc)
        H, W = sc["H"], sc["W"]
        if nan_voxel:
            b, d, y, x = sc["nan_at"]
            assert np.isnan(ix[:, d, y, x]).all() and np.isnan(ix).sum() == ix.shape[0]
        else:
            assert np.isfinite(ix).all() and np.isfinite(iy).all()
        far16, far32 = sc["far_planes"]
        assert (np.abs(ix[:, far16]) > 40000).all() and (np.abs(ix[:, far16]) < 2.0 ** 31).all()         # beyond int16, inside int32
        assert (np.abs(ix[:, far32]) > 2.0 ** 31).all() and (ix[0, far32] > 0).all() and (ix[1, far32] < 0).all()      # saturates, both signs
        near = [d for d in range(ix.shape[1]) if d not in sc["far_planes"]]
        ok = _inside(ix[:, near], iy[:, near], H, W)
        assert ok.mean() > 0.9                                                                           # ... next to valid taps


def test_image_edge_scenes(oracle):
    for W in (96, 70, 40):
        sc = cts.image_edges(W)
        ix, iy = cts.cells(oracle, sc)
        H = sc["H"]
        assert np.isfinite(ix).all() and np.isfinite(iy).all()
        sides = dict(left=ix < -1, right=ix > W - 1, top=iy < -1, bottom=iy > H - 1)
        ok = _inside(ix, iy, H, W)
        for name, out in sides.items():
            # one wave patch and plane group (4 planes) that holds taps beyond this side AND taps inside the image
            mixed = any((out[:, g:g + 4, ys, xs].any() and ok[:, g:g + 4, ys, xs].any()) for ys, xs in _patches(H, W) for g in (0, 4))
            assert mixed, (W, name)
        assert (ix == -1).any() and (ix == W - 1).any() and (iy == -1).any() and (iy == H - 1).any()     # the border cells themselves


def test_box_overflow_scene(oracle):
    sc = cts.box_overflow()
    ix, iy = cts.cells(oracle, sc)
    H, W = sc["H"], sc["W"]
    assert np.isfinite(ix).all() and np.isfinite(iy).all()
    ok = _inside(ix, iy, H, W)
    wide = single = 0
    for ys, xs in _patches(H, W):
        m = ok[0, :, ys, xs]
        if m.any():
            c = ix[0, :, ys, xs][m]
            wide += (c.max() - c.min() + 2) > BW + 3          # wider than the box whatever the alignment of its origin
        for d in range(ix.shape[1]):
            m1 = ok[0, d, ys, xs]
            if m1.any():
                c, r = ix[0, d, ys, xs][m1], iy[0, d, ys, xs][m1]
                single += (c.max() - c.min() + 2 + 3 > BW) or (r.max() - r.min() + 2 > R)
    assert wide >= 12 and single == 0, (wide, single)


def test_tail_group_scenes(oracle):
    for V, C, D in ((3, 32, 12), (3, 32, 5), (5, 32, 8)):
        sc = cts.tail_group(V, C, D)
        ix, iy = cts.cells(oracle, sc)
        assert np.isfinite(ix).all() and _inside(ix, iy, sc["H"], sc["W"]).mean() > 0.8


def test_clamp_extent_scene(oracle):
    sc = cts.clamp_extents()
    ix, iy = cts.cells(oracle, sc)
    W = sc["W"]
    assert np.isfinite(ix).all() and np.isfinite(iy).all()
    have = set(np.unique(ix).astype(np.int64).tolist())
    assert {-2, -1, 0, W - 2, W - 1, W}.issubset(have), sorted(have)
    assert max(have) > 32767
    # no coordinate within 1e-6 px of a cell boundary: the cells are the same in any float64 evaluation order
    _, _, samp, _ = oracle.rpc_warp_coords(sc["rpc"][:, 1], sc["rpc"][:, 0], sc["depth"], sc["H"], W)
    px = samp[0] * W / (W - 1.0) - 0.5
    near = px[np.abs(px) < 1000]
    assert np.abs(near - np.round(near)).min() > 1e-6
