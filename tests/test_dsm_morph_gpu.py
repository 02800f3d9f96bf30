"""Ground extraction on the MI355X (dsm.morph / ground_filter / extract_dtm / ndsm, smvs_dsm_morph / smvs_dsm_ground) against
the numpy oracle (tests/dsm_morph_oracle.py), every comparison bit for bit: all operations and radii from 1 to 256 on grids
smaller than the window and wider than a row piece, degenerate grids, several schedules, the crop property across the
kernels' pieces, determinism, the host checks of the C entries, the chain heights_to_dsm -> despike -> extract_dtm -> ndsm,
and one 2048 x 2048 grid."""
import ctypes as C

import numpy as np
import pytest
import torch

import dsm_morph_oracle as mo
import dsm_post_oracle as po
import dsm_render_oracle as ro
from dsm_testkit import dev, same as _same  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ND = np.float32(-999.0)
SIZES = [(1, 1), (1, 70), (67, 3), (128, 160), (257, 301)]                 # those of test_dsm_post_gpu
RADII = [1, 2, 3, 7, 16, 64, 256]


def _morph_all(z, radii=RADII, nodata=-999.0):
    """Every op at every radius, device-resident (one upload), against the oracle."""
    from satmvs_amd import dsm
    zd = torch.from_numpy(z).cuda()
    for radius in radii:
        for op in mo.OPS:
            got = dsm.morph(zd, radius, op, nodata=nodata).cpu().numpy()
            _same(got, mo.morph(z, radius, op, nodata), (op, radius, z.shape, nodata))


# ---- morph ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SIZES + [(40, 50), (300, 2300), (1100, 40)])
def test_morph_against_the_oracle(dev, shape):
    """(40, 50): both sides below most radii; (300, 2300): wider than a row piece of 2048 cells; (1100, 40): taller than a
    column piece of 1024 rows."""
    z = mo.scene(*shape, seed=30)
    _morph_all(z)
    _morph_all(z, radii=[2, 64], nodata=float("nan"))                       # -999 cells are heights then, the lowest of all


def test_morph_special_grids(dev):
    from satmvs_amd import dsm
    gh, gw = 70, 300
    for void in (np.full((gh, gw), ND, np.float32), np.full((gh, gw), np.nan, np.float32)):
        _morph_all(void, radii=[1, 16, 256])
        assert mo.same_bits(dsm.morph(void, 16, "open"), void)
    for r, c in ((0, 0), (gh - 1, gw - 1), (33, 255)):
        one = np.full((gh, gw), ND, np.float32)
        one[5, 5:9] = np.nan
        one[r, c] = 77.5
        _morph_all(one, radii=[1, 16, 256])
        assert mo.same_bits(dsm.morph(one, 256, "erode"), one)
    full = mo.scene(gh, gw, seed=31, voids=0.0)
    full[~mo.valid(full, ND)] = 50.0
    _morph_all(full, radii=[1, 7, 64])
    zeros = np.zeros((gh, gw), np.float32)
    zeros[20, 130] = -0.0
    lo, hi = dsm.morph(zeros, 2, "erode"), dsm.morph(zeros, 2, "dilate")
    assert np.signbit(lo).sum() == 25 and np.signbit(lo[18:23, 128:133]).all() and not np.signbit(hi).any()
    z = mo.scene(gh, gw, seed=32)
    ok = mo.valid(z, ND)
    for radius in (1, 5, 40):
        o = dsm.morph(z, radius, "open")
        assert (mo.f2key(o)[ok] <= mo.f2key(z)[ok]).all()                  # an opening never raises a cell


# ---- ground filter -------------------------------------------------------------------------------------------------------------
SCHEDULES = [([1], [0.5]), ([1, 2, 4, 8, 16], None), ([1, 2, 4, 8, 16, 20], None), ([3, 5, 40], [0.0, 2.0, 3.5]),
             ([1, 2, 4, 8, 16, 32, 64, 128, 256], None), (list(range(1, 17)), [0.25 * k for k in range(16)])]


def _ground_both(z, radii, thresholds, nodata=-999.0):
    from satmvs_amd import dsm
    dtm, cls = dsm.ground_filter(z, nodata=nodata, schedule=(radii, thresholds), return_class=True)
    want, wcls = mo.ground(z, radii, thresholds, nodata)
    _same(cls, wcls, ("cls", z.shape, radii))
    _same(dtm, want, ("dtm", z.shape, radii))
    ok = mo.valid(z, nodata)
    assert np.array_equal(cls == 0, ~ok) and np.array_equal(dtm.view(np.uint32)[cls <= 1], z.view(np.uint32)[cls <= 1])
    assert np.array_equal(dtm.view(np.uint32)[cls >= 2], np.full(int((cls >= 2).sum()), np.float32(nodata)).view(np.uint32))
    return dtm, cls


@pytest.mark.parametrize("shape", SIZES + [(300, 340)])
def test_ground_filter_against_the_oracle(dev, shape):
    from satmvs_amd import dsm
    z = mo.scene(*shape, seed=40)
    for radii, thresholds in SCHEDULES:
        if thresholds is None:
            thresholds = mo.schedule(5.0, radii[-1])[1]
            assert mo.schedule(5.0, radii[-1])[0] == radii
        _ground_both(z, radii, thresholds)
    _ground_both(z, [1, 2, 4], [1.5, 4.5, 6.0], nodata=float("nan"))
    dtm, cls = dsm.ground_filter(z, 5.0, max_radius=20, return_class=True)                 # by parameters = by its schedule
    want, wcls = mo.ground(z, *mo.schedule(5.0, 20))
    _same(dtm, want, "by parameters")
    _same(cls, wcls, "by parameters")


def test_known_answer_scene_on_the_device(dev):
    z, box = mo.known_answer_scene()
    dtm, cls = _ground_both(z, *mo.schedule(5.0))
    ok = mo.valid(z, ND)
    print("known-answer scene on the device: %.4f of the box cells removed, %.4f of the others kept"
          % ((cls[ok & box] >= 2).mean(), (cls[ok & ~box] == 1).mean()))


# ---- the crop property ---------------------------------------------------------------------------------------------------------
def test_crop_property(dev):
    """A crop that keeps 2 sum(r_k) cells around a region gives that region's bits (windows are clipped at the border, so
    only the interior compares).  Row pieces are 2048 cells and whole rows here; column pieces are 256 - 2 r rows up to
    radius 64: the crops start at rows that shift the seams."""
    from satmvs_amd import dsm
    z = mo.scene(700, 420, seed=50, voids=0.15)
    for radii, thresholds in (([1, 2, 4, 8], [1.5, 4.5, 6.0, 6.0]), ([3, 30], [1.0, 5.0]), ([60], [2.0])):
        m = 2 * sum(radii)
        whole, cw = dsm.ground_filter(z, schedule=(radii, thresholds), return_class=True)
        for r0, r1, c0, c1 in ((m + 7, 700 - m - 11, m + 5, 420 - m - 3), (m + 130, m + 200, m + 1, m + 90)):
            crop, cc = dsm.ground_filter(z[r0 - m:r1 + m, c0 - m:c1 + m], schedule=(radii, thresholds), return_class=True)
            _same(crop[m:-m, m:-m], whole[r0:r1, c0:c1], ("dtm crop", radii))
            _same(cc[m:-m, m:-m], cw[r0:r1, c0:c1], ("cls crop", radii))
    for radius in (5, 64, 100):
        m = 2 * radius
        whole = dsm.morph(z, radius, "open")
        crop = dsm.morph(z[29:700, 3:420], radius, "open")
        _same(crop[m:-m, m:-m], whole[29 + m:700 - m, 3 + m:420 - m], ("open crop", radius))


# ---- determinism, streams, inputs left alone, host checks ----------------------------------------------------------------------
def test_deterministic_on_device_tensors(dev):
    from satmvs_amd import dsm
    z = mo.scene(257, 301, seed=60, voids=0.2)
    zd = torch.from_numpy(z).to(dev)
    keep = zd.clone()
    sched = mo.schedule(5.0, 20)
    a, ca = dsm.ground_filter(zd, schedule=sched, return_class=True)
    b, cb = dsm.ground_filter(zd, schedule=sched, return_class=True)
    o1, o2 = dsm.morph(zd, 70, "close"), dsm.morph(zd, 70, "close")
    assert a.is_cuda and a.dtype == torch.float32 and ca.dtype == torch.uint8 and a.shape == zd.shape == ca.shape
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ca, cb)
    assert torch.equal(o1.view(torch.int32), o2.view(torch.int32))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        c, cc = dsm.ground_filter(zd, schedule=sched, return_class=True)
        o3 = dsm.morph(zd, 70, "close")
    side.synchronize()
    assert torch.equal(a.view(torch.int32), c.view(torch.int32)) and torch.equal(ca, cc) and torch.equal(o1.view(torch.int32), o3.view(torch.int32))
    assert torch.equal(zd.view(torch.int32), keep.view(torch.int32))                      # the input is not modified
    _same(a.cpu().numpy(), mo.ground(z, *sched)[0], "ground on tensors")
    _same(o1.cpu().numpy(), mo.morph(z, 70, "close"), "close on tensors")
    wide = torch.from_numpy(np.concatenate([z, z], axis=1)).to(dev)                      # a non-contiguous view
    assert torch.equal(dsm.morph(wide[:, :301], 70, "close").view(torch.int32), o1.view(torch.int32))
    zc = z.copy()
    out = dsm.ground_filter(zc, schedule=sched)
    assert isinstance(out, np.ndarray) and mo.same_bits(out, a.cpu().numpy()) and mo.same_bits(zc, z)
    nd = dsm.ndsm(zd, a)
    assert nd.is_cuda and mo.same_bits(nd.cpu().numpy(), mo.ndsm(z, a.cpu().numpy()))


def test_c_entries_reject_bad_arguments(dev):
    from satmvs_amd import _lib
    lib = _lib.load()
    gh, gw = 32, 48
    z = torch.zeros((gh, gw), dtype=torch.float32, device=dev)
    out = torch.full_like(z, 5.0)
    cls = torch.full((gh, gw), 9, dtype=torch.uint8, device=dev)
    need = lib.smvs_dsm_morph_workspace_bytes(gw, gh, 8)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    radii, thresholds = np.array([1, 2, 4], np.int32), np.array([1.0, 2.0, 3.0], np.float64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    stream = _lib.current_stream(dev)

    def morph(src=z, radius=2, op=2, dst=out, w=ws, nbytes=need):
        _lib.call("smvs_dsm_morph", _lib.ptr(src), gw, gh, -999.0, radius, op, _lib.ptr(dst), _lib.ptr(w), nbytes, stream)

    def ground(src=z, r=radii, t=thresholds, dst=out, c=cls, w=ws, nbytes=need):
        _lib.call("smvs_dsm_ground", _lib.ptr(src), gw, gh, -999.0, vp(r), vp(t), len(r), _lib.ptr(dst), _lib.ptr(c), _lib.ptr(w), nbytes, stream)

    bad = [(lambda: morph(dst=z), "out aliases"), (lambda: morph(nbytes=need - 1), "workspace too small"),
           (lambda: morph(radius=0), "radius must be"), (lambda: morph(radius=257), "radius must be"), (lambda: morph(op=4), "op must be"),
           (lambda: morph(w=out), "workspace aliases"),
           (lambda: ground(dst=z), "dtm aliases"), (lambda: ground(nbytes=need - 1), "workspace too small"),
           (lambda: ground(r=np.array([1, 1, 4], np.int32)), "strictly increasing"),
           (lambda: ground(r=np.array([1, 2, 300], np.int32)), r"radii\[2\]"),
           (lambda: ground(t=np.array([1.0, np.nan, 3.0])), r"thresholds\[1\]"),
           (lambda: ground(c=out.view(torch.uint8)), "cls aliases"), (lambda: ground(w=cls), "workspace")]
    for f, pattern in bad:
        with pytest.raises(_lib.SatMVSNativeError, match=r"code 1\b.*" + pattern):      # SMVS_ERR_ARG
            f()
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((cls == 9).all())              # nothing was launched
    morph()
    ground()
    torch.cuda.synchronize()
    assert bool((out == 0.0).all()) and bool((cls == 1).all())


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_production_chain(dev):
    """Three views of a gentle surface with one 16 x 16-cell block 35 m high -> height maps with holes and a few wrong
    heights -> heights_to_dsm -> despike -> extract_dtm -> ndsm, equal to the oracle chain; the block is removed and stands
    about 35 m above the DTM."""
    from satmvs_amd import dsm
    from satmvs_amd.transverse_mercator import whu_tlc_projection
    proj = whu_tlc_projection()
    tm7 = proj.tm7()
    H, W, res = 128, 160, 2.5
    rpcs = [ro.view_rpc(H, W, s, seed=11) for s in (0.0, 0.4, -0.4)]
    grid = ro.grid_over([(r, (H, W)) for r in rpcs], tm7, 100.0, 200.0, res, margin=15.0)
    E, N = ro.cell_centres(grid)
    truth = (140.0 + 3.0 * np.sin(E / 53.0) * np.cos(N / 71.0)).astype(np.float32)        # slopes below 0.06
    r0, c0 = grid.height // 2 - 8, grid.width // 2 - 8
    truth[r0:r0 + 16, c0:c0 + 16] += 35.0
    rng = np.random.default_rng(12)
    hs = []
    for rpc in rpcs:
        h = dsm.render_heights(truth, grid, rpc, proj, (H, W))
        h[rng.random((H, W)) < 0.35] = np.nan
        wrong = rng.random((H, W)) < 0.01
        h[wrong] += rng.choice([-60.0, 60.0], (H, W))[wrong].astype(np.float32)
        hs.append(h)
    fused = dsm.heights_to_dsm(hs, rpcs, proj, grid, mode="mean")
    clean = dsm.despike(fused, radius=2, thresh=10.0, min_valid=3)
    dtm, cls = dsm.extract_dtm(clean, grid, return_class=True)
    above = dsm.ndsm(clean, dtm)
    # the oracle chain
    want_clean, _ = po.despike(fused, radius=2, thresh=10.0, min_valid=3)
    radii, thresholds = mo.schedule(res)
    want_holes, want_cls = mo.ground(want_clean, radii, thresholds)
    want_dtm, _ = po.fill(want_holes, max_steps=256, min_hits=3, method="idw")
    want_above = mo.ndsm(want_clean, want_dtm)
    _same(clean, want_clean, "chain despike")
    _same(cls, want_cls, "chain classes")
    _same(dtm, want_dtm, "chain dtm")
    _same(above, want_above, "chain ndsm")
    _same(dsm.ground_filter(clean, res), want_holes, "chain filter")
    ground_cells = want_cls == 1
    assert np.array_equal(want_dtm.view(np.uint32)[ground_cells], want_clean.view(np.uint32)[ground_cells])
    assert (want_above[mo.valid(want_above, ND)] >= 0).all()
    inner = (slice(r0 + 2, r0 + 14), slice(c0 + 2, c0 + 14))
    ok = mo.valid(want_clean[inner], ND)
    print("chain: %d cells, %d removed, block interior: %d valid, nDSM %.2f .. %.2f m"
          % (fused.size, (want_cls >= 2).sum(), ok.sum(), want_above[inner][ok].min(), want_above[inner][ok].max()))
    assert ok.sum() > 50 and (want_cls[inner][ok] >= 2).all()
    assert (want_above[inner][ok] >= 25.0).all() and (want_above[inner][ok] <= 45.0).all()


# ---- one large grid ------------------------------------------------------------------------------------------------------------
def test_large_ground_filter(dev):
    z = po.scene(2048, 2048, seed=8, voids=0.1)
    rows, cols = np.mgrid[0:2048, 0:2048]
    z[(rows + 2 * cols < 1500) | (rows > 1700 + cols // 8)] = ND            # exterior wedges, as in a fused DSM's bounding box
    z[600:900, 700:1100] = np.nan
    dtm, cls = _ground_both(z, *mo.schedule(5.0, 64))
    assert (cls >= 2).sum() > 10000 and (cls == 1).sum() > 10000           # both classes are exercised (the scene's relief is steep)
