"""DSM clean-up on the MI355X (dsm.despike / dsm.fill_voids, smvs_dsm_despike / smvs_dsm_fill) against the numpy oracle
(tests/dsm_post_oracle.py), every comparison bit for bit: all radii, methods, reaches and hit thresholds on scenes with
speckles and voids and on degenerate grids, the crop property across the kernels' tiles and bands, determinism, the chain
heights_to_dsm -> despike -> fill_voids -> visibility / orthorectify, and one 2048 x 2048 grid per operation."""
import numpy as np
import pytest
import torch

import dsm_post_oracle as po
import dsm_render_oracle as ro
from dsm_testkit import dev, same as _same  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ND = np.float32(-999.0)
SIZES = [(1, 1), (1, 70), (67, 3), (128, 160), (257, 301)]


def _despike_both(z, **kw):
    from satmvs_amd import dsm
    got, removed = dsm.despike(z, return_removed=True, **kw)
    want, wremoved = po.despike(z, **kw)
    _same(got, want, ("despike", z.shape, kw))
    _same(removed, wremoved, ("removed", z.shape, kw))
    return got, removed


def _fill_both(z, **kw):
    from satmvs_amd import dsm
    got, hits = dsm.fill_voids(z, return_hits=True, **kw)
    want, whits = po.fill(z, **kw)
    _same(hits, whits, ("hits", z.shape, kw))
    _same(got, want, ("fill", z.shape, kw))
    return got, hits


# ---- despike -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("shape", SIZES)
def test_despike_against_the_oracle(dev, shape, radius):
    z = po.scene(*shape, seed=10 + radius)
    window = (2 * radius + 1) ** 2
    n_removed = []
    for thresh, min_valid in ((10.0, 3), (10.0, 1), (25.0, window), (0.0, 1), (0.0, 3)):
        out, removed = _despike_both(z, radius=radius, thresh=thresh, min_valid=min_valid)
        n_removed.append(int(removed.sum()))
        assert np.array_equal(removed == 1, po.valid(z, ND) & ~po.valid(out, ND))
    if shape == (257, 301):
        assert n_removed[0] > 500 and n_removed[1] <= n_removed[0] < n_removed[3]        # spikes go; thresh = 0 takes far more
    # nodata = NaN: -999 cells are heights then, far from everything; removed cells are written as NaN
    out, removed = _despike_both(z, nodata=float("nan"), radius=radius, thresh=10.0, min_valid=3)
    assert np.isnan(out[removed == 1]).all()


def test_despike_known_answers(dev):
    from satmvs_amd import dsm
    rows, cols = np.mgrid[0:40, 0:90]
    z = (100.0 + 0.5 * cols - 0.25 * rows).astype(np.float32)
    z[8, 9] += 50.0
    z[15, 70] -= 50.0
    z[39, 89] += 50.0                                                      # a corner: window of 9 cells at radius 2
    for radius in (1, 2, 3):
        out, removed = dsm.despike(z, radius=radius, return_removed=True)
        assert removed.sum() == 3 and removed[8, 9] and removed[15, 70] and removed[39, 89]
        assert (out[removed == 1] == ND).all() and np.array_equal(out[removed == 0], z[removed == 0])
    lone = np.full((40, 90), np.nan, np.float32)
    lone[20, 64] = 100.0                                                   # on a tile boundary of 64 columns
    lone[30, 10:12] = 100.0
    lone[5:7, 5:7] = 100.0
    out, removed = dsm.despike(lone, radius=2, min_valid=3, return_removed=True)
    assert removed.sum() == 3 and removed[20, 64] and removed[30, 10:12].all() and np.isnan(out[0, 0])


# ---- fill ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", po.METHODS)
@pytest.mark.parametrize("shape", SIZES)
def test_fill_against_the_oracle(dev, shape, method):
    z = po.scene(*shape, seed=20, voids=0.35)
    gh, gw = shape
    r, c = gh // 3, gw // 3
    z[r:r + gh // 4, c:c + gw // 3] = np.nan                              # one void deeper than the short reaches
    for max_steps in (1, 7, 64, max(gh, gw) + 5):
        for min_hits in (1, 3, 8):
            out, hits = _fill_both(z, max_steps=max_steps, min_hits=min_hits, method=method)
            assert np.array_equal(po.valid(out, ND), po.valid(z, ND) | ((hits >= min_hits) & (hits != 255)))
    _fill_both(z, nodata=float("nan"), max_steps=7, min_hits=3, method=method)          # -999 cells are heights then


@pytest.mark.parametrize("method", po.METHODS)
def test_fill_special_grids(dev, method):
    from satmvs_amd import dsm
    gh, gw = 70, 300
    full = po.scene(gh, gw, seed=3, voids=0.0)
    full[~po.valid(full, ND)] = 50.0
    out, hits = _fill_both(full, max_steps=9, method=method)
    assert po.same_bits(out, full) and (hits == 255).all()
    for void in (np.full((gh, gw), ND, np.float32), np.full((gh, gw), np.nan, np.float32)):
        out, hits = _fill_both(void, max_steps=400, min_hits=1, method=method)
        assert po.same_bits(out, void) and (hits == 0).all()
    for r, c in ((0, 0), (0, gw - 1), (gh - 1, 0), (gh - 1, gw - 1)):     # one valid cell in a corner
        one = np.full((gh, gw), ND, np.float32)
        one[r, c] = 77.5
        out, hits = _fill_both(one, max_steps=4096, min_hits=1, method=method)
        seen = (hits == 1)
        assert seen.sum() == (gh - 1) + (gw - 1) + (min(gh, gw) - 1) and (out[seen] == 77.5).all()
        out, hits = _fill_both(one, max_steps=100, min_hits=1, method=method)
        assert (hits == 1).sum() == min(100, gh - 1) + 100 + min(100, gh - 1)
    border = po.scene(gh, gw, seed=4, voids=0.05)                          # voids touching every border, NaN and nodata mixed
    border[:3] = np.nan
    border[-2:] = ND
    border[:, :5] = ND
    border[:, -70:] = np.nan
    border[10:20, 100:230] = np.nan
    for max_steps in (2, 40, 256):
        _fill_both(border, max_steps=max_steps, min_hits=2, method=method)
    # the known answers: a hole in an exact plane, a slot in a constant
    rows, cols = np.mgrid[0:gh, 0:gw]
    plane = (100.0 + 0.5 * cols - 0.25 * rows).astype(np.float32)
    hole = plane.copy()
    hole[33, 191] = ND
    hole[50:53, 63:66] = np.nan
    out = dsm.fill_voids(hole, max_steps=4, method=method)
    if method == "idw":
        assert out[33, 191] == plane[33, 191] and out[51, 64] == plane[51, 64]
    const = np.full((gh, gw), 123.25, np.float32)
    slot = const.copy()
    slot[30:34] = ND
    assert po.same_bits(dsm.fill_voids(slot, max_steps=8, method=method), const)


# ---- the crop property ---------------------------------------------------------------------------------------------------------
def test_crop_property(dev):
    """The operation on a window grown by its reach, cut back, equals the window of the operation on the whole grid.  The fill
    marches in bands of max(32, max_steps) rows and combines in waves of 64 columns; despike works on tiles of 64 x 16 cells:
    the windows straddle those boundaries, and the grown crops start at rows and columns that shift them."""
    from satmvs_amd import dsm
    z = po.scene(300, 340, seed=6, voids=0.3)
    z[120:200, 40:330] = np.nan                                            # deeper than the reach, across wave boundaries
    for max_steps, (r0, r1, c0, c1) in ((16, (40, 100, 100, 280)), (5, (27, 70, 59, 135)), (40, (41, 250, 45, 290)),
                                        (70, (75, 220, 72, 260))):
        for method in po.METHODS:
            whole, hw = dsm.fill_voids(z, max_steps=max_steps, method=method, return_hits=True)
            m = max_steps
            crop, hc = dsm.fill_voids(z[r0 - m:r1 + m, c0 - m:c1 + m], max_steps=max_steps, method=method, return_hits=True)
            _same(crop[m:-m, m:-m], whole[r0:r1, c0:c1], ("fill crop", max_steps, method))
            _same(hc[m:-m, m:-m], hw[r0:r1, c0:c1], ("hits crop", max_steps, method))
    for radius in (1, 2, 3):
        for r0, r1, c0, c1 in ((10, 40, 50, 140), (15, 17, 63, 65), (31, 130, 120, 200)):
            whole, rw = dsm.despike(z, radius=radius, return_removed=True)
            R = radius
            crop, rc = dsm.despike(z[r0 - R:r1 + R, c0 - R:c1 + R], radius=radius, return_removed=True)
            _same(crop[R:-R, R:-R], whole[r0:r1, c0:c1], ("despike crop", radius))
            _same(rc[R:-R, R:-R], rw[r0:r1, c0:c1], ("removed crop", radius))


# ---- determinism, streams, inputs left alone -------------------------------------------------------------------------------
def test_deterministic_on_device_tensors(dev):
    from satmvs_amd import dsm
    z = po.scene(257, 301, seed=7, voids=0.3)
    zd = torch.from_numpy(z).to(dev)
    keep = zd.clone()
    a, ra = dsm.despike(zd, radius=3, return_removed=True)
    b, rb = dsm.despike(zd, radius=3, return_removed=True)
    f, hf = dsm.fill_voids(zd, max_steps=20, return_hits=True)
    g, hg = dsm.fill_voids(zd, max_steps=20, return_hits=True)
    assert a.is_cuda and a.dtype == torch.float32 and ra.dtype == torch.uint8 and hf.dtype == torch.uint8 and f.shape == zd.shape
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ra, rb)
    assert torch.equal(f.view(torch.int32), g.view(torch.int32)) and torch.equal(hf, hg)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        c, rc = dsm.despike(zd, radius=3, return_removed=True)
        h, hh = dsm.fill_voids(zd, max_steps=20, return_hits=True)
    side.synchronize()
    assert torch.equal(a.view(torch.int32), c.view(torch.int32)) and torch.equal(ra, rc)
    assert torch.equal(f.view(torch.int32), h.view(torch.int32)) and torch.equal(hf, hh)
    assert torch.equal(zd.view(torch.int32), keep.view(torch.int32))                      # the input is not modified
    _same(a.cpu().numpy(), po.despike(z, radius=3)[0], "despike on tensors")
    _same(f.cpu().numpy(), po.fill(z, max_steps=20)[0], "fill on tensors")
    # a non-contiguous view and a numpy input give the same bits; numpy in, numpy out, and the array is left alone
    wide = torch.from_numpy(np.concatenate([z, z], axis=1)).to(dev)
    assert torch.equal(dsm.fill_voids(wide[:, :301], max_steps=20).view(torch.int32), f.view(torch.int32))
    zc = z.copy()
    out = dsm.fill_voids(zc, max_steps=20)
    assert isinstance(out, np.ndarray) and po.same_bits(out, f.cpu().numpy()) and po.same_bits(zc, z)


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_production_chain(dev):
    """Three views of a known surface -> height maps with holes and a few wrong heights -> heights_to_dsm -> despike ->
    fill_voids -> visibility / orthorectify: state 0 is exactly the cells the clean-up left void, and completeness rises."""
    from satmvs_amd import dsm
    from satmvs_amd.transverse_mercator import whu_tlc_projection
    proj = whu_tlc_projection()
    tm7 = proj.tm7()
    H, W, res = 128, 160, 2.5
    rpcs = [ro.view_rpc(H, W, s, seed=11) for s in (0.0, 0.4, -0.4)]
    grid = ro.grid_over([(r, (H, W)) for r in rpcs], tm7, 100.0, 200.0, res, margin=15.0)
    E, N = ro.cell_centres(grid)
    truth = (140.0 + 15.0 * np.sin(E / 53.0) * np.cos(N / 71.0)).astype(np.float32)
    r0, c0 = grid.height // 2 - 8, grid.width // 2 - 8
    truth[r0:r0 + 16, c0:c0 + 16] += 35.0                                  # a block: occlusion shadows in the tilted views
    rng = np.random.default_rng(12)
    hs = []
    for rpc in rpcs:
        h = dsm.render_heights(truth, grid, rpc, proj, (H, W))
        h[rng.random((H, W)) < 0.35] = np.nan                              # what a consistency filter rejects
        wrong = rng.random((H, W)) < 0.01
        h[wrong] += rng.choice([-60.0, 60.0], (H, W))[wrong].astype(np.float32)
        hs.append(h)
    fused = dsm.heights_to_dsm(hs, rpcs, proj, grid, mode="mean")
    min_hits, max_steps = 3, 8
    clean, removed = dsm.despike(fused, radius=2, thresh=10.0, min_valid=3, return_removed=True)
    filled, hits = dsm.fill_voids(clean, max_steps=max_steps, min_hits=min_hits, return_hits=True)
    want_clean, want_removed = po.despike(fused, radius=2, thresh=10.0, min_valid=3)
    want_filled, want_hits = po.fill(want_clean, max_steps=max_steps, min_hits=min_hits)
    _same(clean, want_clean, "chain despike")
    _same(filled, want_filled, "chain fill")
    _same(hits, want_hits, "chain hits")
    void_before, void_after = ~po.valid(fused, ND), ~po.valid(filled, ND)
    print("chain: %d cells, void %d -> %d, removed %d" % (fused.size, void_before.sum(), void_after.sum(), removed.sum()))
    assert removed.sum() > 20
    assert np.array_equal(void_after, want_hits < min_hits)                # 255 (valid) and hits >= min_hits are not void
    assert 0 < void_after.sum() < void_before.sum()
    state = dsm.visibility(filled, grid, rpcs[0], proj, (H, W))
    assert np.array_equal(state == 0, void_after)
    assert (dsm.visibility(fused, grid, rpcs[0], proj, (H, W)) == 0).sum() == void_before.sum()
    img = rng.uniform(0.0, 255.0, (H, W, 3)).astype(np.float32)
    ortho, src = dsm.orthorectify(img, rpcs[0], filled, grid, proj, return_source=True)
    assert np.isnan(ortho[void_after]).all() and (src[void_after] == -1).all()
    before = dsm.dsm_metrics(fused, truth, -999.0)
    after = dsm.dsm_metrics(filled, truth, -999.0)
    want_valid = (want_hits == 255) | (want_hits >= min_hits)              # truth is valid everywhere
    assert after["completeness"] == want_valid.sum() / truth.size
    assert after["completeness"] > before["completeness"]
    print("chain: completeness %.4f -> %.4f, mae %.3f -> %.3f" % (before["completeness"], after["completeness"], before["mae"],
                                                                    after["mae"]))


# ---- one large grid per operation ------------------------------------------------------------------------------------------
def _large():
    z = po.scene(2048, 2048, seed=8, voids=0.1)
    rows, cols = np.mgrid[0:2048, 0:2048]
    z[(rows + 2 * cols < 1500) | (rows > 1700 + cols // 8)] = ND            # exterior wedges, as in a fused DSM's bounding box
    z[600:900, 700:1100] = np.nan                                          # water
    return z


def test_large_despike(dev):
    z = _large()
    out, removed = _despike_both(z, radius=2, thresh=10.0, min_valid=3)
    assert removed.sum() > 10000


def test_large_fill(dev):
    z = _large()
    out, hits = _fill_both(z, max_steps=32, min_hits=3)
    assert (hits == 0).sum() > 100000 and ((hits >= 3) & (hits != 255)).sum() > 100000
