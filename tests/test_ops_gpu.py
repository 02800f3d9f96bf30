"""The stand-alone operators of csrc/warp.hip and csrc/regress.hip beyond their one golden fixture each (tests/test_hip_parity.py):
the warps against the oracle bit for bit with every differing voxel tied to its float32 coordinate, against an independent numpy
float64 sampler inside a derived bound, at the edges of the sampler and of the Python surface; both warp backwards against a
float64 scatter inside the float32 summation bound; the regressions against the oracle and against float64 with every window
confidence that differs explained; the flat projectors and the homography composition.  Scenes, references, bounds and checks:
tests/ops_scene.py; what they assume: tests/test_ops_cpu.py.  Nothing here depends on the order in which blocks run."""
import ctypes as C

import numpy as np
import pytest
import torch

import ops_scene as osn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the GPU suite needs an MI355X")
    return torch.device("cuda", 0)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _warp(dev, geo, fea, src, ref, depth):
    from satmvs_amd.modules import warping
    f = fea if isinstance(fea, torch.Tensor) else _t(fea, dev)
    d = depth if isinstance(depth, torch.Tensor) else _t(depth, dev)
    if geo == "rpc":
        return warping.rpc_warping(f, _t(src, dev), _t(ref, dev), d, None)
    return warping.homo_warping(f, _t(src, dev), _t(ref, dev), d)


def _oracle_warp(orc, geo, fea, src, ref, depth):
    return orc.rpc_warping(fea, src, ref, depth) if geo == "rpc" else orc.homo_warping(fea, src, ref, depth)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


_KINDS = pytest.mark.parametrize("per_pixel", [False, True], ids=["planes", "perpixel"])
_GEO = pytest.mark.parametrize("geo", osn.GEOS)


# ---- 1. forward against the oracle, every difference explained ------------------------------------------------------------------
@_KINDS
@pytest.mark.parametrize("case", osn.WARP_CASES, ids=osn.case_id)
@_GEO
def test_warp_forward_every_difference_explained(dev, oracle, geo, case, per_pixel):
    from satmvs_amd.modules import warping
    B, C, D, H, W = case
    fea, src, ref, depth = osn.scene(geo, B, C, D, H, W, seed=31, per_pixel=per_pixel)
    out = _warp(dev, geo, fea, src, ref, depth)
    got = out.cpu().numpy()
    want = _oracle_warp(oracle, geo, fea, src, ref, depth)
    msgs, n = osn.explain_warp(oracle, geo, got, want, fea, src, ref, depth)
    print("%s %s: %d explained voxels of %d" % (geo, osn.case_id(case), n, B * D * H * W))
    assert not msgs, "\n".join(msgs)
    if H == 1 or W == 1:
        # the reference divides the pixel coordinate by (W-1)/2 = 0: the coordinate is +-inf or NaN, its fraction inf - inf = NaN,
        # all four taps are dropped (read 0) and 0 * NaN = NaN -- what ATen's sampler and the oracle give: NaN everywhere
        assert np.isnan(want).all() and np.isnan(got).all()
    else:
        assert np.isfinite(got).all()
    if geo == "rpc":                                                               # the QC-dictionary entry: the same bits
        qs, qr = ({k: _t(v, dev) for k, v in osn.qc_dict(r).items()} for r in (src, ref))
        eni = warping.rpc_warping_enisum(_t(fea, dev), qs, qr, _t(depth, dev))
        assert np.array_equal(np.isnan(eni.cpu().numpy()), np.isnan(got)) and bool(((eni == out) | (eni.isnan() & out.isnan())).all())


@_GEO
def test_warp_forward_full_tile(dev, oracle, geo):
    """768 x 384, 64 planes, per-pixel heights: the whole volume."""
    B, C, D, H, W = osn.BIG_CASE
    fea, src, ref, depth = osn.scene(geo, B, C, D, H, W, seed=32, per_pixel=True)
    got = _warp(dev, geo, fea, src, ref, depth).cpu().numpy()
    want = _oracle_warp(oracle, geo, fea, src, ref, depth)
    msgs, n = osn.explain_warp(oracle, geo, got, want, fea, src, ref, depth)
    print("%s %s: %d explained voxels of %d" % (geo, osn.case_id(osn.BIG_CASE), n, B * D * H * W))
    assert not msgs, "\n".join(msgs)


# ---- 2. forward against the independent float64 sampler ----------------------------------------------------------------------------
@_KINDS
@pytest.mark.parametrize("case", [c for c in osn.WARP_CASES if c[3] > 1 and c[4] > 1], ids=osn.case_id)
@_GEO
def test_warp_forward_inside_the_float64_bound(dev, geo, case, per_pixel):
    B, C, D, H, W = case
    fea, src, ref, depth = osn.scene(geo, B, C, D, H, W, seed=33, per_pixel=per_pixel, smooth=True)
    got = _warp(dev, geo, fea, src, ref, depth).cpu().numpy()
    px, py = osn.numpy_coords(geo, src, ref, depth, H, W)
    val, mag = osn.sampler_f64(fea, px, py, H, W)
    bound = osn.sampler_bound(px, py, mag, H, W)
    err = np.abs(got.astype(np.float64) - val)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("%s %s: worst error / bound %.3g" % (geo, osn.case_id(case), worst))
    assert (err <= bound).all(), worst


# ---- 3. edges of the sampler and of the surface --------------------------------------------------------------------------------------
def _shift_pair(B, tx, ty, z0=0.0):
    """Pinhole pair whose composition moves pixel (x, y) to (x + tx, y + ty) at depth 1: X = (x + tx) d', Z = d + z0."""
    src = np.tile(np.eye(4), (B, 1, 1))
    src[:, 0, 2], src[:, 1, 2], src[:, 2, 3] = tx, ty, z0
    return src, np.tile(np.eye(4), (B, 1, 1))


@pytest.mark.parametrize("shift", [(-0.6, 0.0), (0.7, 0.0), (0.0, -0.4), (0.0, 0.2), (-0.6, 0.2), (0.3, 0.3)], ids=str)
def test_partial_taps_at_the_border(dev, oracle, shift):
    """Coordinates in (-1, 0) and (W-1, W) (rows: (-1, 0) and (H-1, H)): one column / row of taps is zero padding.  Bits of the
    oracle, and the float64 statement of the rule inside its bound."""
    B, C, D, H, W = 1, 3, 2, 9, 70
    fea = osn.smooth_features(B, C, H, W, seed=50)
    src, ref = _shift_pair(B, *shift)
    depth = np.ones((B, D), np.float32)
    got = _warp(dev, "pinhole", fea, src, ref, depth).cpu().numpy()
    msgs, n = osn.explain_warp(oracle, "pinhole", got, oracle.homo_warping(fea, src, ref, depth), fea, src, ref, depth)
    assert not msgs and n == 0, msgs
    px, py = osn.numpy_coords("pinhole", src, ref, depth, H, W)
    xs, ys = px * W / (W - 1) - 0.5, py * H / (H - 1) - 0.5                           # where the reference's two formulas put the sample
    partial = ((xs > -1) & (xs < 0)) | ((xs > W - 1) & (xs < W)) | ((ys > -1) & (ys < 0)) | ((ys > H - 1) & (ys < H))
    assert partial.sum() >= min(H, W) // 2, "the case has no partial taps"
    val, mag = osn.sampler_f64(fea, px, py, H, W)
    assert (np.abs(got - val) <= osn.sampler_bound(px, py, mag, H, W)).all()
    assert (np.abs(val[:, :, partial[0]]) > 1e-3).any()


@pytest.mark.parametrize("shift", [(500.0, 0.0), (-500.0, 0.0), (0.0, 90.0), (1e30, 0.0)], ids=str)
def test_no_overlap_is_exactly_zero(dev, shift):
    B, C, D, H, W = 2, 5, 3, 9, 70
    fea = np.random.default_rng(51).standard_normal((B, C, H, W)).astype(np.float32)
    src, ref = _shift_pair(B, *shift)
    got = _warp(dev, "pinhole", fea, src, ref, np.ones((B, D), np.float32)).cpu().numpy()
    assert not got.view(np.uint32).any()                                           # +0.0 everywhere


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf, 3e38], ids=str)
@pytest.mark.parametrize("whole", [False, True], ids=["patch", "whole"])
@_GEO
def test_non_finite_depths(dev, oracle, geo, whole, value):
    B, C, D, H, W = 2, 3, 9, 12, 70
    fea, src, ref, depth = osn.scene(geo, B, C, D, H, W, seed=52, per_pixel=True)
    if whole:
        depth[:] = value
    else:
        depth[1, 2:5, 3:8, 10:40] = value
    got = _warp(dev, geo, fea, src, ref, depth).cpu().numpy()
    want = _oracle_warp(oracle, geo, fea, src, ref, depth)
    msgs, n = osn.explain_warp(oracle, geo, got, want, fea, src, ref, depth)
    assert not msgs, "\n".join(msgs)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    if not whole:
        assert np.isfinite(got[0]).all() and np.isfinite(got[1, :, 0]).all()           # nothing leaks out of the patch


def test_pinhole_points_behind_the_camera(dev, oracle):
    """Z = d - 500: planes with Z < 0 (the division mirrors the point, as the reference's does) and the plane with Z = 0
    (x / 0 = +-inf, 0 / 0 = NaN: taps dropped, NaN weights)."""
    B, C, D, H, W = 1, 3, 5, 9, 70
    fea = np.random.default_rng(53).standard_normal((B, C, H, W)).astype(np.float32)
    src, ref = _shift_pair(B, 0.25, 0.25, z0=-500.0)
    depth = np.array([[300.0, 499.0, 500.0, 501.0, 900.0]], np.float32)
    got = _warp(dev, "pinhole", fea, src, ref, depth).cpu().numpy()
    want = oracle.homo_warping(fea, src, ref, depth)
    msgs, n = osn.explain_warp(oracle, "pinhole", got, want, fea, src, ref, depth)
    assert not msgs, "\n".join(msgs)
    assert np.isnan(want[:, :, 2]).all() and np.isnan(got[:, :, 2]).all()            # Z = 0
    assert np.isfinite(got[:, :, [0, 1, 3, 4]]).all() and np.abs(got[:, :, 4]).max() > 0


def test_non_finite_features(dev, oracle):
    """A tap in range with weight exactly 0 makes NaN out of a NaN feature (0 * NaN, as torch); a feature that no tap of a voxel
    reaches -- another batch item's, or one outside the voxel's 2 x 2 cell -- does not."""
    B, C, D, H, W = 2, 2, 1, 4, 4
    fea = np.random.default_rng(54).standard_normal((B, C, H, W)).astype(np.float32)
    fea[1] = np.nan                                                                 # batch item 1 is all NaN: must stay there
    fea[0, 0, :, 2] = np.nan                                                        # column 2 of channel 0
    fea[0, 1, 3, 3] = np.inf
    # u = x + 1.125: for x = 0, g + 1 = 1.125 / 1.5 = 0.75 and the sample lands on 0.75 * 2 - 0.5 = 1.0 exactly: west tap column 1
    # with weight 1, east tap column 2 with weight 0 and in range
    src, ref = _shift_pair(B, 1.125, 0.0)
    got = _warp(dev, "pinhole", fea, src, ref, np.ones((B, D), np.float32)).cpu().numpy()
    want = oracle.homo_warping(fea, src, ref, np.ones((B, D), np.float32))
    msgs, n = osn.explain_warp(oracle, "pinhole", got, want, fea, src, ref, np.ones((B, D), np.float32))
    assert not msgs and n == 0, msgs
    assert np.isnan(got[0, 0, 0, :, 0]).all()                                       # weight 0, in range: NaN
    assert np.isfinite(got[0, 1, 0, :3, 0]).all()                                   # channel 1 has no NaN, and inf at (3,3) is out of reach
    assert np.isnan(got[1][..., :3]).all() and not got[1][..., 3].view(np.uint32).any()   # x = 3 samples at 5.0: all taps dropped, finite weights
    clean = fea.copy()
    clean[0, 0, :, 2] = 0.0
    clean[0, 1, 3, 3] = 0.0
    ok = _warp(dev, "pinhole", clean, src, ref, np.ones((B, D), np.float32)).cpu().numpy()
    assert np.isfinite(ok[0]).all()                                                 # item 1's NaNs are never read for item 0


@pytest.mark.parametrize("offset", [1, 2, 3])
@_GEO
def test_unaligned_storage(dev, geo, offset):
    """Feature and depth tensors that start 4, 8 and 12 bytes into a larger storage: the bits of the aligned call."""
    B, C, D, H, W = 2, 3, 9, 7, 67
    fea, src, ref, depth = osn.scene(geo, B, C, D, H, W, seed=55, per_pixel=True)
    want = _warp(dev, geo, fea, src, ref, depth)
    big_f = torch.full((fea.size + 8,), float("nan"), device=dev)
    big_d = torch.full((depth.size + 8,), float("nan"), device=dev)
    f = big_f[offset:offset + fea.size].view(fea.shape)
    d = big_d[offset:offset + depth.size].view(depth.shape)
    f.copy_(_t(fea, dev)); d.copy_(_t(depth, dev))
    assert f.data_ptr() % 16 == 4 * offset and f.is_contiguous()
    got = _warp(dev, geo, f, src, ref, d)
    assert torch.equal(got, want)
    f2 = f.clone().requires_grad_(True)
    f3 = big_f[offset:offset + fea.size].view(fea.shape).detach().requires_grad_(True)
    g = torch.randn_like(want)
    _warp(dev, geo, f2, src, ref, d.clone()).backward(g)
    _warp(dev, geo, f3, src, ref, d).backward(g)
    assert (f2.grad - f3.grad).abs().max() <= 1e-4 * max(1.0, float(f2.grad.abs().max()))


@_GEO
def test_non_contiguous_inputs(dev, geo):
    """Channel-sliced and transposed views: the result of the contiguous copy, or SatMVSNativeError -- never other memory."""
    from satmvs_amd import _lib
    B, C, D, H, W = 2, 6, 5, 8, 66
    fea, src, ref, depth = osn.scene(geo, B, C, D, H, W, seed=56, per_pixel=True)
    f, d = _t(fea, dev), _t(depth, dev)
    views = [(f[:, ::2], d), (f[:, 1:4], d), (f.transpose(2, 3).contiguous().transpose(2, 3), d),
             (f, d.transpose(2, 3).contiguous().transpose(2, 3)), (f, d[:, :, :1, :1].expand(B, D, H, W)),
             (f, _t(depth[:, :, 0, 0], dev).t().contiguous().t())]
    for fv, dv in views:
        assert not (fv.is_contiguous() and dv.is_contiguous())
        want = _warp(dev, geo, fv.contiguous(), src, ref, dv.contiguous())
        try:
            got = _warp(dev, geo, fv, src, ref, dv)
        except _lib.SatMVSNativeError:
            continue
        assert torch.equal(got, want)


def test_c_entries_reject_bad_arguments(dev):
    """Host-side argument checks of every entry of warp.hip / regress.hip: error code 1, smvs_last_error set, nothing launched.
    The buffers are small and real; the huge sizes are dimensions only, and the check returns before any launch."""
    from satmvs_amd import _lib
    from satmvs_amd.modules.depth_range import GeneratedHeights
    B, Cc, D, H, W = 1, 2, 3, 4, 8
    z = lambda *s, dt=torch.float32: torch.full(s, 5.0, dtype=dt, device=dev)
    fea, depth, out5, gsrc = z(B, Cc, H, W), z(B, D), z(B, Cc, D, H, W), z(B, Cc, H, W)
    rpc, proj, pout = z(B, 170, dt=torch.float64), z(B, 16, dt=torch.float64), z(B, 16, dt=torch.float64)
    reg, od, oc = z(B, D, H, W), z(B, H, W), z(B, H, W)
    st = [z(B, H, W, dt=torch.float64) for _ in range(3)]
    pts = [z(16, dt=torch.float64) for _ in range(5)]
    gen = GeneratedHeights(z(B, H, W), D, 2.5, (H, W), (H, W))
    gs = gen.c_struct()
    hyp = z(B, D, H, W)
    p, s, NUL = _lib.ptr, _lib.current_stream(dev), None

    def rpc_warp(name, a=fea, o=out5, sr=rpc, rr=rpc, dp=depth, dims=(B, Cc, D, H, W)):
        _lib.call(name, p(a) if a is not None else NUL, p(sr) if sr is not None else NUL, p(rr) if rr is not None else NUL,
                  p(dp) if dp is not None else NUL, 0, p(o) if o is not None else NUL, *dims, s)

    def homo_warp(name, a=fea, o=out5, pr=proj, dp=depth, dims=(B, Cc, D, H, W)):
        _lib.call(name, p(a) if a is not None else NUL, p(pr) if pr is not None else NUL, p(dp) if dp is not None else NUL, 0,
                  p(o) if o is not None else NUL, *dims, s)

    def softmax(r=reg, dp=depth, a=od, b=oc, dims=(B, D, H, W)):
        _lib.call("smvs_softmax_regress_fwd", p(r) if r is not None else NUL, p(dp) if dp is not None else NUL, 0,
                  p(a) if a is not None else NUL, p(b) if b is not None else NUL, *dims, s)

    def window(r=reg, dp=depth, a=od, b=oc, dims=(B, D, H, W)):
        _lib.call("smvs_window_regress_fwd", p(r) if r is not None else NUL, p(dp) if dp is not None else NUL, 0,
                  p(a) if a is not None else NUL, p(b) if b is not None else NUL, NUL, 0.0, *dims, s)

    def step(r=od, dp=depth, acc=st, dims=(B, D, H, W), d=0):
        _lib.call("smvs_stream_regress_step", p(r) if r is not None else NUL, p(dp) if dp is not None else NUL, 0,
                  *[p(a) if a is not None else NUL for a in acc], *dims, d, s)

    def final(acc=st, a=od, b=oc):
        _lib.call("smvs_stream_regress_final", *[p(x) if x is not None else NUL for x in acc], p(a) if a is not None else NUL,
                  p(b) if b is not None else NUL, B * H * W, s)

    def project(r=rpc, arrs=pts, n=16, direction=0):
        _lib.call("smvs_rpc_project", p(r) if r is not None else NUL, *[p(a) if a is not None else NUL for a in arrs], n, direction, s)

    def compose(a=proj, b=proj, o=pout, n=B):
        _lib.call("smvs_homo_compose", p(a) if a is not None else NUL, p(b) if b is not None else NUL, p(o) if o is not None else NUL, n, s)

    def hypotheses(g=gs, o=hyp, dims=(B, H, W)):
        _lib.call("smvs_height_hypotheses", C.addressof(g) if g is not None else NUL, p(o) if o is not None else NUL, *dims, s)

    null, dim = "null pointer", "non-positive dimension"
    huge_map = (1, 1 << 15, 1, 1 << 7, 1 << 7)             # C H W 4 = 2^31 bytes
    huge_grid = (1, 1, 1 << 14, 1 << 14, 1 << 14)          # 256 x 4096 tiles x 2048 plane chunks = 2^31 blocks; C H W 4 = 2^30
    bad = []
    for name, f in (("smvs_rpc_warp_fwd", rpc_warp), ("smvs_rpc_warp_bwd", rpc_warp), ("smvs_homo_warp_fwd", homo_warp),
                    ("smvs_homo_warp_bwd", homo_warp)):
        bad += [(lambda f=f, n=name: f(n, a=None), null), (lambda f=f, n=name: f(n, o=None), null), (lambda f=f, n=name: f(n, dp=None), null)]
        bad += [(lambda f=f, n=name, k=k: f(n, dims=tuple(0 if i == k else v for i, v in enumerate((B, Cc, D, H, W)))), dim) for k in range(5)]
        bad += [(lambda f=f, n=name: f(n, dims=(B, Cc, -1, H, W)), dim), (lambda f=f, n=name: f(n, dims=huge_map), "larger than 2 GiB"),
                (lambda f=f, n=name: f(n, dims=huge_grid), "grid too large")]
    bad += [(lambda n=n: rpc_warp(n, sr=None), null) for n in ("smvs_rpc_warp_fwd", "smvs_rpc_warp_bwd")]
    bad += [(lambda n=n: rpc_warp(n, rr=None), null) for n in ("smvs_rpc_warp_fwd", "smvs_rpc_warp_bwd")]
    bad += [(lambda n=n: homo_warp(n, pr=None), null) for n in ("smvs_homo_warp_fwd", "smvs_homo_warp_bwd")]
    bad += [(lambda: compose(a=None), null), (lambda: compose(b=None), null), (lambda: compose(o=None), null),
            (lambda: compose(n=0), "non-positive matrix count"), (lambda: compose(n=-3), "non-positive matrix count")]
    for f in (softmax, window):
        bad += [(lambda f=f: f(r=None), null), (lambda f=f: f(dp=None), null), (lambda f=f: f(a=None), null), (lambda f=f: f(b=None), null)]
        bad += [(lambda f=f, k=k: f(dims=tuple(0 if i == k else v for i, v in enumerate((B, D, H, W)))), dim) for k in range(4)]
    bad += [(lambda: step(r=None), null), (lambda: step(dp=None), null), (lambda: step(acc=[st[0], None, st[2]]), null),
            (lambda: step(d=-1), "plane index -1 of 3"), (lambda: step(d=D), "plane index 3 of 3"), (lambda: step(d=D + 7), "plane index"),
            (lambda: step(dims=(0, D, H, W)), "bad dimension"), (lambda: step(dims=(B, D, H, 0)), "bad dimension"),
            (lambda: final(acc=[None, st[1], st[2]]), null), (lambda: final(a=None), null), (lambda: final(b=None), null)]
    bad += [(lambda: project(r=None), null), (lambda: project(arrs=pts[:2] + [None] + pts[3:]), null), (lambda: project(arrs=pts[:4] + [None]), null),
            (lambda: project(direction=2), "dir must be"), (lambda: project(direction=-1), "dir must be")]
    bad += [(lambda: hypotheses(g=None), null), (lambda: hypotheses(o=None), null), (lambda: hypotheses(dims=(0, H, W)), dim),
            (lambda: hypotheses(dims=(B, H, 0)), dim), (lambda: hypotheses(dims=(B, H, W + 1)), "integer multiple")]
    for f, pattern in bad:
        with pytest.raises(_lib.SatMVSNativeError, match=r"code 1\b.*" + pattern):     # SMVS_ERR_ARG
            f()
        assert pattern.split()[0] in _lib.load().smvs_last_error().decode()
    torch.cuda.synchronize()
    for tns in [fea, depth, out5, gsrc, reg, od, oc, hyp, pout] + st + pts:
        assert bool((tns == 5.0).all())                                              # nothing was launched
    rpc_warp("smvs_rpc_warp_bwd", a=out5, o=gsrc); compose(); softmax(); hypotheses()  # and the good calls run
    torch.cuda.synchronize()
    assert not bool((hyp == 5.0).all())


# ---- 4. backward ------------------------------------------------------------------------------------------------------------------
def _backward_case(dev, orc, geo, case, per_pixel, seed, twice=False):
    B, C, D, H, W = case
    fea, src, ref, depth = osn.scene(geo, B, C, D, H, W, seed=seed, per_pixel=per_pixel)
    f = _t(fea, dev).requires_grad_(True)
    out = _warp(dev, geo, f, src, ref, depth)
    # voxels whose forward differs from the oracle's sit on a coordinate the two float64 chains round apart: their taps are not the
    # oracle's, so they are taken out of both sides (their gradient is zero for the kernel and for the reference)
    want = _oracle_warp(orc, geo, fea, src, ref, depth)
    got = out.detach().cpu().numpy()
    vox = ((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))).any(1)
    assert vox.sum() <= max(1, osn.MAX_EXPLAINED * vox.size)
    gout = np.random.default_rng(seed + 1).standard_normal(got.shape).astype(np.float32)
    gout[np.broadcast_to(vox[:, None], gout.shape)] = 0.0
    off, wts = osn.taps_from_grid(*osn.oracle_grid(orc, geo, src, ref, depth, H, W), H, W)
    out.backward(_t(gout, dev), retain_graph=twice)
    msgs, worst, nmax = osn.check_backward(f.grad.cpu().numpy(), gout, off, wts, H, W, "first call")
    if twice:
        first = f.grad.clone()
        f.grad = None
        out.backward(_t(gout, dev))
        m2, _, _ = osn.check_backward(f.grad.cpu().numpy(), gout, off, wts, H, W, "second call")
        msgs += m2
        assert float((f.grad - first).abs().max()) <= 1e-3 * max(1.0, float(first.abs().max()))   # not 2 x the first
    print("%s %s: worst error / bound %.3g, most contributions to a cell %d" % (geo, osn.case_id(case), worst, nmax))
    return msgs


@_KINDS
@pytest.mark.parametrize("case", osn.WARP_CASES, ids=osn.case_id)
@_GEO
def test_warp_backward_inside_the_summation_bound(dev, oracle, geo, case, per_pixel):
    msgs = _backward_case(dev, oracle, geo, case, per_pixel, seed=60)
    assert not msgs, "\n".join(msgs)


@_GEO
def test_warp_backward_full_tile(dev, oracle, geo):
    msgs = _backward_case(dev, oracle, geo, osn.BIG_CASE, True, seed=61)
    assert not msgs, "\n".join(msgs)


@_GEO
def test_warp_backward_twice_through_autograd(dev, oracle, geo):
    """Two backward calls in a row: each inside the bound, the second not on top of the first (grad_src starts from zero)."""
    msgs = _backward_case(dev, oracle, geo, (2, 3, 9, 33, 65), True, seed=62, twice=True)
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("hw", [(33, 65), (96, 192)], ids=str)
def test_warp_backward_hot_cell(dev, oracle, hw):
    """A degenerate homography sends every voxel to one source position: all D H W contributions of a channel land on the same four
    addresses, 19 305 resp. 165 888 atomics per address.  The bound is the same (n + 1) 2^-24 sum |g w| with n the actual count: a
    worst-case bound on n roundings in any order, so it holds however the atomics are serialised -- 1.2e-3 resp. 1e-2 of sum |g w|
    here.  (At the full tile n 2^-24 exceeds 1 and the bound would say nothing; that size is not run.)"""
    H, W = hw
    B, C, D = 1, 2, 9
    fea = np.random.default_rng(63).standard_normal((B, C, H, W)).astype(np.float32)
    src = np.zeros((B, 4, 4))
    src[:, 0, 3], src[:, 1, 3], src[:, 2, 3], src[:, 3, 3] = 20.3, 10.6, 1.0, 1.0        # X = 20.3, Y = 10.6, Z = 1 for every pixel and depth
    ref = np.tile(np.eye(4), (B, 1, 1))
    depth = np.linspace(1.0, 2.0, D, dtype=np.float32)[None]
    f = _t(fea, dev).requires_grad_(True)
    out = _warp(dev, "pinhole", f, src, ref, depth)
    assert _bits_equal(out.detach().cpu().numpy(), oracle.homo_warping(fea, src, ref, depth))
    gout = np.random.default_rng(64).standard_normal((B, C, D, H, W)).astype(np.float32)
    out.backward(_t(gout, dev))
    off, wts = osn.taps_from_grid(*osn.oracle_grid(oracle, "pinhole", src, ref, depth, H, W), H, W)
    msgs, worst, nmax = osn.check_backward(f.grad.cpu().numpy(), gout, off, wts, H, W, "hot cell")
    print("hot cell %s: worst error / bound %.3g, %d contributions per address" % (hw, worst, nmax))
    assert nmax == D * H * W and int((f.grad != 0).sum()) == 4 * C
    assert not msgs, "\n".join(msgs)


# ---- 5. regressions ---------------------------------------------------------------------------------------------------------------
_REG_IDS = lambda c: "D%d-%s-%s" % (c[0], "x".join(map(str, c[1])), c[2])


def _regress_checks(dev, orc, reg, heights, D, lamb=1.5):
    """softmax and window regression of one scene against the oracle (the tolerances of test_window_regression_golden) and against
    float64 (the oracle's own largest distance plus that tolerance; for the height never less than the project's 1e-3 m)."""
    from satmvs_amd.modules import module as M
    r, h = _t(reg, dev), _t(heights, dev)
    with torch.no_grad():
        d1, c1 = (x.cpu().numpy() for x in M.softmax_depth_regression(r, h))
        d2, c2, v2 = (x.cpu().numpy() for x in M.window_depth_regression(r, h, lamb=lamb))
        d3, c3 = (x.cpu().numpy() for x in M.window_depth_regression(r, h))
    assert _bits_equal(d2, d3) and _bits_equal(c2, c3) and _bits_equal(d1, d2)
    od, oc = orc.softmax_regress(reg, heights)
    wd, wc, wv = orc.window_regress(reg, heights, lamb=lamb)
    f64 = osn.regress_f64(reg, heights, lamb=lamb)
    np.testing.assert_allclose(d1, od, rtol=0, atol=osn.TOL_DEPTH)
    np.testing.assert_allclose(c1, oc, rtol=osn.TOL_CONF_R, atol=osn.TOL_CONF_A)
    np.testing.assert_allclose(d2, wd, rtol=0, atol=osn.TOL_DEPTH)
    np.testing.assert_allclose(v2, wv, rtol=osn.TOL_VAR_R, atol=osn.TOL_VAR_A)
    own = np.abs(od - f64["depth"]).max()
    allow = max(osn.TOL_PROJECT, own + osn.TOL_DEPTH)
    print("D=%d: oracle %.3g m from float64, allowance %.3g m%s" % (D, own, allow, " (the project's 1e-3)" if allow == osn.TOL_PROJECT else ""))
    assert np.abs(d1 - f64["depth"]).max() <= allow
    assert (np.abs(v2 - f64["var"]) <= np.abs(wv - f64["var"]).max() + osn.TOL_VAR_R * np.abs(f64["var"]) + osn.TOL_VAR_A).all()
    assert (np.abs(c1 - f64["conf_max"]) <= np.abs(oc - f64["conf_max"]).max() + osn.TOL_CONF_R * f64["conf_max"] + osn.TOL_CONF_A).all()
    msgs, excused = osn.check_window_conf(c2, f64, D)
    print("D=%d: %.3g of the pixels excused" % (D, excused))
    assert not msgs, "\n".join(msgs)
    return allow


@pytest.mark.parametrize("case", osn.reg_cases(), ids=_REG_IDS)
def test_regressions_against_oracle_and_float64(dev, oracle, case):
    """Every case of this matrix has an allowance of the project's 1e-3 m against float64 (the oracle's own distance plus 1e-4 m
    stays below it; printed per case)."""
    D, bhw, kind = case
    reg, heights = osn.reg_scene(D, bhw, kind, seed=40 + D)
    _regress_checks(dev, oracle, reg, heights, D)


@pytest.mark.parametrize("case", [(48, osn.REG_BIG, "tensor"), (64, osn.REG_BIG, "planes")], ids=_REG_IDS)
def test_regressions_full_tile(dev, oracle, case):
    D, bhw, kind = case
    reg, heights = osn.reg_scene(D, bhw, kind, seed=40 + D)
    _regress_checks(dev, oracle, reg, heights, D)


@pytest.mark.parametrize("sampler", ["interval1", "interval2", "ucs"])
@pytest.mark.parametrize("case", [c for c in osn.reg_cases() if c[0] >= 2 and c[2] == "tensor"] + [(48, osn.REG_BIG, "tensor")], ids=_REG_IDS)
def test_generated_heights_give_the_bits_of_the_tensor(dev, oracle, case, sampler):
    """Every regression entry fed a GeneratedHeights object (interval sampler at scale 1 and 2, UCS sampler) returns the bits of the
    call fed the materialised tensor; the materialised tensor is the oracle's."""
    from satmvs_amd.modules import module as M
    from satmvs_amd.modules.depth_range import GeneratedHeights
    D, (B, H, W), _ = case
    rng = np.random.default_rng(70 + D)
    reg = _t((rng.standard_normal((B, D, H, W)) * 3).astype(np.float32), dev)
    hp, wp = max(1, (H + 1) // 2), max(1, (W + 1) // 2)
    prev = (200.0 + rng.normal(0, 6.0, (B, hp, wp))).astype(np.float32)
    if sampler == "ucs":
        var = rng.uniform(0.5, 12.0, (B, hp, wp)).astype(np.float32)
        lo, hi = np.full(B, 190.0, np.float32), np.full(B, 215.0, np.float32)
        gen = GeneratedHeights.ucs(_t(prev, dev), _t(var, dev), _t(lo, dev), _t(hi, dev), D, (H, W))
        want = oracle.ucs_hypotheses(prev, var, lo, hi, D, (H, W))
    else:
        up = 1 if sampler == "interval1" else 2
        gen = GeneratedHeights(_t(prev, dev), D, 2.5, (H * up, W * up), (H, W))
        want = oracle.height_hypotheses(prev, D, 2.5, (H * up, W * up), (H, W))
    dv = gen.materialize()
    assert _bits_equal(dv.cpu().numpy(), want)
    with torch.no_grad():
        for a, b in zip(M.softmax_depth_regression(reg, gen) + M.window_depth_regression(reg, gen, lamb=1.5) + M.window_depth_regression(reg, gen),
                        M.softmax_depth_regression(reg, dv) + M.window_depth_regression(reg, dv, lamb=1.5) + M.window_depth_regression(reg, dv)):
            assert torch.equal(a, b)


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 48])
def test_one_hot_and_uniform_logits(dev, D):
    """One-hot logits (gap 120 > 104: every other exp underflows to 0 in float32) at planes 0, 1, D-2, D-1: the height is that
    plane's, bit for bit, the softmax confidence exactly 1, the window confidence the float64 sum of the planes inside
    [idx-1, idx+2] -- 1, with the window hanging over plane 0 or D-1 and, for D < 4, larger than the volume.  All-equal logits:
    p = 1/D, the height the mean, the window min(D, 4) / D (idx = trunc((D-1)/2) keeps four planes inside for D >= 4)."""
    from satmvs_amd.modules import module as M
    planes = sorted({0, min(1, D - 1), max(D - 2, 0), D - 1})
    H, W = 3, 5
    heights = np.random.default_rng(80).uniform(0, 400, (1, D, H, W)).astype(np.float32)
    for k in planes:
        reg = np.full((1, D, H, W), -60.0, np.float32)
        reg[:, k] = 60.0
        with torch.no_grad():
            d1, c1 = M.softmax_depth_regression(_t(reg, dev), _t(heights, dev))
            d2, c2, v2 = M.window_depth_regression(_t(reg, dev), _t(heights, dev), lamb=1.5)
        assert _bits_equal(d1.cpu().numpy(), heights[:, k]) and _bits_equal(d2.cpu().numpy(), heights[:, k])
        assert bool((c1 == 1.0).all()) and bool((c2 == 1.0).all()) and bool((v2 == 0.0).all())
    reg = np.full((1, D, H, W), 0.37, np.float32)
    with torch.no_grad():
        d1, c1 = M.softmax_depth_regression(_t(reg, dev), _t(heights, dev))
        d2, c2 = M.window_depth_regression(_t(reg, dev), _t(heights, dev))
    np.testing.assert_allclose(c1.cpu().numpy(), 1.0 / D, rtol=2 * osn.U32)
    np.testing.assert_allclose(c2.cpu().numpy(), min(D, 4) / D, rtol=8 * osn.U32)
    np.testing.assert_allclose(d1.cpu().numpy(), heights.astype(np.float64).mean(1), rtol=0, atol=(D + 2) * osn.U32 * 400.0)


def _torch_regress(reg, heights, lamb):
    """The reference's operator sequence on the CPU: torch.softmax and its reductions (oracle/torch_composite.py holds the same)."""
    r, h = torch.from_numpy(reg), torch.from_numpy(heights)
    p = torch.softmax(r, 1)
    D = r.shape[1]
    hv = h.view(*h.shape, 1, 1) if h.dim() == 2 else h
    depth = torch.sum(p * hv, 1)
    sum4 = 4 * torch.nn.functional.avg_pool3d(torch.nn.functional.pad(p.unsqueeze(1), pad=(0, 0, 0, 0, 1, 2)), (4, 1, 1), stride=1, padding=0).squeeze(1)
    idx = torch.sum(p * torch.arange(D, dtype=torch.float32).view(1, D, 1, 1), 1).long()
    conf = torch.gather(sum4, 1, idx.clamp(min=0, max=D - 1).unsqueeze(1)).squeeze(1)
    return depth.numpy(), p.max(1)[0].numpy(), conf.numpy()


@pytest.mark.parametrize("name", ["pm80", "pm3e38", "some_ninf", "all_ninf", "pinf", "nan_first", "nan_middle", "nan_last"])
def test_extreme_logits(dev, name):
    """+-80, +-3e38, -inf in some planes, -inf in all, +inf, NaN in the first / a middle / the last plane: the NaN mask and the finite
    values of torch's softmax and the reference's two reductions on the CPU."""
    from satmvs_amd.modules import module as M
    B, D, H, W = 1, 9, 4, 16
    rng = np.random.default_rng(81)
    reg = (rng.standard_normal((B, D, H, W)) * 3).astype(np.float32)
    heights = np.linspace(0, 400, D, dtype=np.float32)[None]
    col = slice(0, W // 2)                                                           # half of the pixels keep ordinary logits
    if name == "pm80":
        reg[:, ::2, :, col], reg[:, 1::2, :, col] = 80.0, -80.0
    elif name == "pm3e38":
        reg[:, 2, :, col], reg[:, 5, :, col] = 3e38, -3e38
    elif name == "some_ninf":
        reg[:, [0, 3, 8], :, col] = -np.inf
    elif name == "all_ninf":
        reg[:, :, :, col] = -np.inf
    elif name == "pinf":
        reg[:, 4, :, col] = np.inf
    else:
        reg[:, {"nan_first": 0, "nan_middle": 4, "nan_last": D - 1}[name], :, col] = np.nan
    td, tc, tw = _torch_regress(reg, heights, 1.5)
    with torch.no_grad():
        d1, c1 = (x.cpu().numpy() for x in M.softmax_depth_regression(_t(reg, dev), _t(heights, dev)))
        d2, c2 = (x.cpu().numpy() for x in M.window_depth_regression(_t(reg, dev), _t(heights, dev)))
    for got, want, atol in ((d1, td, 1e-4), (d2, td, 1e-4), (c1, tc, 1e-6)):
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        np.testing.assert_allclose(got[~np.isnan(want)], want[~np.isnan(want)], rtol=1e-5, atol=atol)
    # window confidence: where the softmax is NaN the index is undefined behaviour in the reference (.long() of NaN); the kernel must
    # give NaN there (every probability is NaN) and torch's value elsewhere
    ok = ~np.isnan(td)
    assert np.isnan(c2[~ok]).all(), name
    np.testing.assert_allclose(c2[ok], tw[ok], rtol=1e-5, atol=1e-6)
    assert ok[..., W // 2:].all()                                                    # the ordinary half stays ordinary


@pytest.mark.parametrize("kind", ["planes", "tensor"])
@pytest.mark.parametrize("D,bhw", [(1, (1, 1, 1)), (5, (1, 1, 255)), (17, (1, 16, 16)), (64, (1, 1, 257)), (48, (3, 33, 70))], ids=str)
def test_streaming_regression(dev, oracle, D, bhw, kind):
    """The three float64 accumulators against a numpy float64 accumulation (1e-13, 1e-12, 1e-13 relative, as test_regression_golden),
    the result against the oracle; a second volume through a fresh accumulator starts from zero; d >= D is rejected."""
    from satmvs_amd import _lib
    from satmvs_amd.modules import module as M
    B, H, W = bhw
    reg, heights = osn.reg_scene(D, bhw, kind, seed=90 + D)
    h = _t(heights, dev)
    results = []
    for volume in range(2):
        acc = M.StreamingRegression(B, H, W, dev)
        assert not bool(acc.state.any())
        for d in range(D):
            acc.step(_t(reg[:, d], dev), h, d)
        st = acc.state.cpu().numpy()
        es, di, mx = osn.stream_f64(reg, heights)
        np.testing.assert_allclose(st[0], es, rtol=1e-13)
        np.testing.assert_allclose(st[1], di, rtol=1e-12)
        np.testing.assert_allclose(st[2], mx, rtol=1e-13)
        results.append(tuple(x.cpu().numpy() for x in acc.result()))
    assert all(_bits_equal(a, b) for a, b in zip(*results))
    oacc = oracle.StreamRegress(B, H, W)
    for d in range(D):
        oacc.step(reg[:, d], heights, d)
    od, oc = oacc.final()
    np.testing.assert_allclose(results[0][0], od, rtol=0, atol=1e-4)
    np.testing.assert_allclose(results[0][1], oc, rtol=1e-6)
    before = acc.state.clone()
    for d in (D, D + 1, -1):
        with pytest.raises(_lib.SatMVSNativeError, match="plane index"):
            acc.step(_t(reg[:, 0], dev), h, d)
    assert torch.equal(acc.state, before)


def test_streaming_regression_where_exp_overflows(dev, oracle):
    """Logits near and above 709.78 (exp overflows float64; float32 logits reach 3.4e38): the oracle's states and results,
    non-finite ones included."""
    from satmvs_amd.modules import module as M
    B, D, H, W = 1, 6, 4, 8
    rng = np.random.default_rng(91)
    reg = rng.uniform(700.0, 712.0, (B, D, H, W)).astype(np.float32)
    reg[:, 2, 0, :4] = [709.7, 709.8, 1000.0, 3e38]
    reg[:, 3, 1, :2] = [-3e38, -800.0]
    heights = np.linspace(0, 400, D, dtype=np.float32)[None]
    acc, oacc = M.StreamingRegression(B, H, W, dev), oracle.StreamRegress(B, H, W)
    for d in range(D):
        acc.step(_t(reg[:, d], dev), _t(heights, dev), d)
        oacc.step(reg[:, d], heights, d)
    st = acc.state.cpu().numpy()
    for got, want, rtol in ((st[0], oacc.exp_sum[:, 0], 1e-13), (st[1], oacc.depth_img[:, 0], 1e-12), (st[2], oacc.max_prob[:, 0], 1e-13)):
        assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(np.isnan(got), np.isnan(want))
        fin = np.isfinite(want)
        np.testing.assert_allclose(got[fin], want[fin], rtol=rtol)
    assert np.isinf(st[0]).any() and np.isfinite(st[0]).any()
    (gd, gc), (od, oc) = (tuple(x.cpu().numpy() for x in acc.result())), oacc.final()
    for got, want in ((gd, od), (gc, oc)):
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
        fin = np.isfinite(want)
        np.testing.assert_allclose(got[fin], want[fin], rtol=1e-6, atol=1e-4)


def test_sharded_fold_of_non_finite_partials(dev):
    """smvs_regress_fold (the reduce step of the depth-sharded streaming regression) folds the ranks' [exp_sum | depth_img | max_prob]
    in rank order: sums for the first two rows, and for the third the same 0/1 blend as the streaming step -- so inf met on two ranks, or
    a NaN partial, gives NaN, exactly what one device accumulating the same planes in sequence holds."""
    from satmvs_amd import _lib
    world, n = 3, 300
    rng = np.random.default_rng(92)
    recv = rng.uniform(0.0, 5.0, (world, 3, n))
    recv[0, 2, :4], recv[1, 2, :4], recv[2, 2, :4] = [np.inf, np.inf, 1.0, np.nan], [np.inf, 2.0, np.inf, 3.0], [1.0, np.inf, 7.0, 9.0]
    recv[1, 0, 10], recv[2, 1, 11], recv[0, 0, 12], recv[1, 0, 12] = np.inf, np.nan, np.inf, -np.inf
    want = recv[0].copy()
    with np.errstate(invalid="ignore"):
        for r in range(1, world):
            want[:2] = want[:2] + recv[r, :2]
            flag = (want[2] < recv[r, 2]).astype(np.float64)
            want[2] = flag * recv[r, 2] + (1.0 - flag) * want[2]
    assert np.isnan(want[2, 0]) and np.isnan(want[2, 1]) and np.isnan(want[2, 3]) and want[2, 2] == np.inf       # the cases above
    out = torch.full((3, n), -1.0, dtype=torch.float64, device=dev)
    rt = _t(recv.reshape(world, 3 * n), dev)
    _lib.call("smvs_regress_fold", _lib.ptr(rt), _lib.ptr(out), world, 3 * n, 0, n, _lib.current_stream(dev))
    got = out.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])
    # the same planes through one accumulator: the same max_prob state
    B, H, W = 1, 1, 4
    from satmvs_amd.modules import module as M
    acc = M.StreamingRegression(B, H, W, dev)
    with np.errstate(divide="ignore", invalid="ignore"):
        logits = np.log(recv[:, 2, :4]).astype(np.float32)                           # exp(log(inf)) = inf, exp(log(NaN)) = NaN
    finite = np.isfinite(recv[:, 2, :4])
    for r in range(world):
        acc.step(_t(logits[r].reshape(B, H, W), dev), _t(np.ones((B, world), np.float32), dev), r)
    one = acc.state[2].cpu().numpy().ravel()
    assert np.array_equal(np.isnan(one), np.isnan(got[2, :4])) and np.array_equal(np.isinf(one), np.isinf(got[2, :4])), (one, got[2, :4], finite)


# ---- 6. flat projectors and the composition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", osn.PROJECT_N + (osn.PROJECT_BIG,))
def test_rpc_project_sizes_and_round_trip(dev, oracle, n):
    from satmvs_amd import rpc_synth
    from satmvs_amd.modules import warping
    H, W = 384, 768
    rpc = rpc_synth.make_view_rpcs(2, H, W, seed=95)[1]
    samp, line, hei = osn.project_points(n, H, W, seed=96)
    r = _t(rpc[None], dev)
    lat, lon = warping.RPC_Photo2Obj(_t(samp, dev)[None], _t(line, dev)[None], _t(hei, dev)[None], r, None)
    s2, l2 = warping.RPC_Obj2Photo(lat, lon, _t(hei, dev)[None], r, None)
    olat, olon = oracle.rpc_project(rpc, samp, line, hei, 0)
    np.testing.assert_allclose(lat[0].cpu().numpy(), olat, rtol=0, atol=1e-12)
    np.testing.assert_allclose(lon[0].cpu().numpy(), olon, rtol=0, atol=1e-12)
    os_, ol = oracle.rpc_project(rpc, olat, olon, hei, 1)
    np.testing.assert_allclose(s2[0].cpu().numpy(), os_, rtol=0, atol=1e-8)
    np.testing.assert_allclose(l2[0].cpu().numpy(), ol, rtol=0, atol=1e-8)
    # photo -> object -> photo: the inverse coefficients are a fit; its error on this RPC, as rpc_synth.roundtrip_error measures it on the
    # CPU, is the bound -- no factor, no constant
    fit = float(np.max(rpc_synth.roundtrip_error(rpc, W, H)))
    back = np.hypot(s2[0].cpu().numpy() - samp, l2[0].cpu().numpy() - line).max()
    print("n=%d: round trip %.3g px, fit error %.3g px" % (n, back, fit))
    assert back <= fit


def test_rpc_round_trip_on_the_lattice_of_the_fit_error(dev):
    """The GPU round trip at the very points rpc_synth.roundtrip_error evaluates (16 x 16 x 5 over the image and the height range): each
    coordinate within the project's 1e-8 px of the numpy round trip, so the error per point is the fit's own."""
    from satmvs_amd import rpc_synth
    from satmvs_amd.modules import warping
    H, W = 384, 768
    for v in range(2):
        rpc = rpc_synth.make_view_rpcs(2, H, W, seed=95)[v]
        h = np.linspace(rpc[rpc_synth.HEIGHT_OFF] - rpc[rpc_synth.HEIGHT_SCALE], rpc[rpc_synth.HEIGHT_OFF] + rpc[rpc_synth.HEIGHT_SCALE], 5)
        x, y, h = (a.reshape(-1) for a in np.meshgrid(np.linspace(0, W, 16), np.linspace(0, H, 16), h))
        xs, ys = rpc_synth.obj2photo(rpc, *rpc_synth.photo2obj(rpc, x, y, h), h)
        want = np.hypot(xs - x, ys - y)
        assert np.array_equal(want, rpc_synth.roundtrip_error(rpc, W, H))           # the same lattice, the same numbers
        r = _t(rpc[None], dev)
        lat, lon = warping.RPC_Photo2Obj(_t(x, dev)[None], _t(y, dev)[None], _t(h, dev)[None], r, None)
        s2, l2 = (t[0].cpu().numpy() for t in warping.RPC_Obj2Photo(lat, lon, _t(h, dev)[None], r, None))
        np.testing.assert_allclose(s2, xs, rtol=0, atol=1e-8)
        np.testing.assert_allclose(l2, ys, rtol=0, atol=1e-8)
        assert (np.hypot(s2 - x, l2 - y) <= want + 2e-8).all()                       # 1e-8 per coordinate


def test_rpc_project_nan_inputs_stay_where_they_are(dev):
    from satmvs_amd import rpc_synth
    from satmvs_amd.modules import warping
    H, W, n = 384, 768, 1000
    rpc = rpc_synth.make_view_rpcs(2, H, W, seed=95)[0]
    samp, line, hei = osn.project_points(n, H, W, seed=97)
    bad = np.zeros(n, bool)
    samp[[0, 255]], line[[256, 511]], hei[[512, 999]] = np.nan, np.nan, np.nan
    bad[[0, 255, 256, 511, 512, 999]] = True
    r = _t(rpc[None], dev)
    lat, lon = (x[0].cpu().numpy() for x in warping.RPC_Photo2Obj(_t(samp, dev)[None], _t(line, dev)[None], _t(hei, dev)[None], r, None))
    assert np.isnan(lat[bad]).all() and np.isnan(lon[bad]).all() and np.isfinite(lat[~bad]).all() and np.isfinite(lon[~bad]).all()
    h2 = np.where(np.isnan(hei), 100.0, hei)
    lat, lon = np.where(bad, 30.0, lat), np.where(bad, 114.0, lon)
    lat[[3, 700]] = np.nan
    s, l = (x[0].cpu().numpy() for x in warping.RPC_Obj2Photo(_t(lat, dev)[None], _t(lon, dev)[None], _t(h2, dev)[None], r, None))
    nanpos = np.zeros(n, bool)
    nanpos[[3, 700]] = True
    assert np.isnan(s[nanpos]).all() and np.isnan(l[nanpos]).all() and np.isfinite(s[~nanpos]).all() and np.isfinite(l[~nanpos]).all()


@pytest.mark.parametrize("n", osn.COMPOSE_N)
def test_homo_compose_counts_pivots_and_bound(dev, golden, n):
    from satmvs_amd.modules import warping
    src, ref = osn.compose_scene(n, seed=98)
    piv = osn.pivot_matrices()
    for i, m in enumerate(piv):                                                     # pivot cases spread over the batch (and over both 64-lane blocks)
        ref[(i * 13) % n] = m
    ints = np.arange(1.0, 17.0).reshape(4, 4)
    src[(3 * 13) % n] = ints
    if n > 52:
        src[(4 * 13) % n] = ints
    got = warping._compose_homography(_t(src, dev), _t(ref, dev)).cpu().numpy()
    assert np.isfinite(got).all()
    worst = 0.0
    for i in range(n):
        want = src[i] @ np.linalg.inv(ref[i])
        bound = osn.compose_bound(src[i], ref[i])
        worst = max(worst, np.abs(got[i] - want).max() / bound)
        assert np.abs(got[i] - want).max() <= bound, (i, n)
        if np.linalg.cond(ref[i]) < 1e7:                                            # fixture-like conditioning: the fixture's own tolerance
            np.testing.assert_allclose(got[i], want, rtol=1e-11, atol=1e-9)
    print("n=%d: worst error / bound %.3g" % (n, worst))
    i = (3 * 13) % n
    if np.array_equal(ref[i], piv[3]):
        assert np.array_equal(got[i], ints @ piv[3].T)                               # a permutation: exact
    if n > 52:
        assert np.array_equal(got[(4 * 13) % n], ints @ piv[4].T)
    g = golden("homo_warp")
    comp = warping._compose_homography(_t(g["proj"][:, 1], dev), _t(g["proj"][:, 0], dev))
    np.testing.assert_allclose(comp.cpu().numpy(), g["composed"], rtol=1e-11, atol=1e-9)


def test_homo_compose_singular_reference_returns(dev):
    from satmvs_amd.modules import warping
    src, ref = osn.compose_scene(5, seed=99)
    ref[1] = 0.0
    ref[3, 2] = ref[3, 1]                                                           # two equal rows
    got = warping._compose_homography(_t(src, dev), _t(ref, dev)).cpu().numpy()
    torch.cuda.synchronize()
    assert not np.isfinite(got[1]).all() and not np.isfinite(got[3]).all()
    for i in (0, 2, 4):
        assert np.abs(got[i] - src[i] @ np.linalg.inv(ref[i])).max() <= osn.compose_bound(src[i], ref[i])


# ---- the launcher's stream rule --------------------------------------------------------------------------
def test_launch_runs_on_the_current_stream(dev, monkeypatch):
    """A native call goes to the stream that is current where it is made (_lib.launch).  Under `with torch.cuda.stream(side)` the
    blend of the ConvGRU cell is handed `side`'s handle and not the handle of the stream that produced the operands -- read off the
    call itself, on both of launch's paths (device already current / selected by the guard) -- and, with the copy back on `side`
    too and only `side` synchronised, the result is bit for bit u * h + (1 - u) * y."""
    from satmvs_amd import _lib
    from satmvs_amd.modules.train_fns import _GruBlendFn
    g = torch.Generator().manual_seed(11)
    producer = torch.cuda.current_stream(dev)
    u, h, y = (torch.rand(3, 1024, generator=g).to(dev) * s for s in (1.0, 3.0, -2.0))      # produced on `producer`
    want = (u * h + (1 - u) * y).cpu()
    side = torch.cuda.Stream(dev)
    assert side.cuda_stream != producer.cuda_stream
    seen = []
    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: (seen.append((name, args[-1].value or 0)), real_call(name, *args))[1])
    side.wait_stream(producer)
    with torch.cuda.stream(side):
        out = _GruBlendFn.apply(u, h, y)
        got = torch.empty(out.shape, dtype=out.dtype).pin_memory()
        got.copy_(out, non_blocking=True)
        monkeypatch.setattr(torch.cuda, "current_device", lambda: -1)      # "another device is current": launch enters its guard
        out2 = _GruBlendFn.apply(u, h, y)
        monkeypatch.undo()
        got2 = out2.cpu()
    side.synchronize()
    assert seen == [("smvs_gru_blend_fwd", side.cuda_stream)] * 2
    assert got.shape == (3, 1024) and torch.equal(got, want) and torch.equal(got2, want)
    torch.cuda.synchronize(dev)
