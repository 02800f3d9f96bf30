"""The staged cost-volume build's tap bookkeeping (costvol_kernels.h: packed 16-bit cells, extents, LDS bases) at the smallest
shapes at which it can go wrong -- scenes of tests/costvol_tap_scene.py, whose properties tests/test_costvol_tap_scene_cpu.py
checks on the CPU.  Through the C ABI, both entries (smvs_rpc_costvol_fwd; smvs_rpc_plane_coef + smvs_rpc_costvol_fwd_pc), both
arithmetic modes, against oracle.costvol_variance:

  * exact arithmetic: every voxel bit for bit, NaN for NaN;
  * fused arithmetic: |got - want| <= 1e-5 max(1, |want|), NaN for NaN.
"""
import numpy as np
import pytest
import torch

import costvol_tap_scene as cts

pytestmark = pytest.mark.gpu

_WANT = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _build(dev, sc, use_pc, d_begin=0, d_end=None):
    """smvs_rpc_costvol_fwd (use_pc False) or smvs_rpc_plane_coef + smvs_rpc_costvol_fwd_pc; the output starts out as 7."""
    from satmvs_amd import _lib
    f = [_t(x, dev) for x in sc["feats"]]
    r, d = _t(sc["rpc"], dev), _t(sc["depth"], dev)
    B, C, H, W = f[0].shape
    D = d.shape[1]
    is4d = 1 if d.dim() == 4 else 0
    d_end = D if d_end is None else d_end
    out = torch.full((B, C, d_end - d_begin, H, W), 7.0, dtype=torch.float32, device=dev)
    st = _lib.current_stream(dev)
    srcs = _lib.ptr_array(f[1:])
    if use_pc:
        pc = torch.zeros(_lib.load().smvs_rpc_plane_coef_bytes(B, len(f) - 1, D) // 8, dtype=torch.float64, device=dev)
        _lib.call("smvs_rpc_plane_coef", _lib.ptr(r), _lib.ptr(d), is4d, _lib.ptr(pc), B, len(f) - 1, D, H, W, 0, D, st)
        _lib.call("smvs_rpc_costvol_fwd_pc", _lib.ptr(f[0]), srcs, len(f) - 1, _lib.ptr(r), _lib.ptr(d), is4d, _lib.ptr(pc), _lib.ptr(out),
                  B, C, D, H, W, d_begin, d_end, d_end - d_begin, 0, st)
    else:
        _lib.call("smvs_rpc_costvol_fwd", _lib.ptr(f[0]), srcs, len(f) - 1, _lib.ptr(r), _lib.ptr(d), is4d, _lib.ptr(out),
                  B, C, D, H, W, d_begin, d_end, d_end - d_begin, 0, st)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _want(oracle, key, sc):
    """The oracle's volume of a scene, computed once; finite except at a planted NaN height (no case passes vacuously)."""
    if key not in _WANT:
        w = oracle.costvol_variance(sc["feats"], sc["rpc"], sc["depth"], "rpc")
        nan = np.zeros(w.shape, bool)
        if sc["nan_at"] is not None:
            b, d, y, x = sc["nan_at"]
            nan[b, :, d, y, x] = True
        assert np.array_equal(np.isnan(w), nan) and np.isfinite(w[~nan]).all()
        w.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


def _check(got, want, arith, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    g, w = got[~nan], want[~nan]
    nbad = int((g != w).sum())
    rel = float((np.abs(g.astype(np.float64) - w) / (1e-5 * np.maximum(1.0, np.abs(w)))).max())
    print("%s, %s: %d of %d voxels differ from the oracle, largest |diff| / (1e-5 max(1,|v|)) = %.3g" % (what, arith, nbad, g.size, rel))
    if arith == "exact":
        assert nbad == 0, (what, nbad)
    else:
        assert rel <= 1.0, (what, rel)


def _both_entries(dev, oracle, arith, key, sc):
    want = _want(oracle, key, sc)
    got = {}
    for use_pc in (False, True):
        got[use_pc] = _build(dev, sc, use_pc)
        _check(got[use_pc], want, arith, "%s, %s" % (key, "plane_coef + fwd_pc" if use_pc else "fwd"))
    return want, got


@pytest.mark.parametrize("nan_voxel", [False, True])
def test_saturated_taps_share_a_wave_with_valid_ones(dev, oracle, arith, nan_voxel):
    """Planes 1e9 m and 3e12 m off (cells beyond int16 / saturated int32, both signs) between valid planes: the box is the valid
    taps' box (else they would read zeros or the wave would fall back: either shows against the oracle), the far taps read
    zeros: a far plane's variance is that of (ref, 0, 0).  With one NaN height: NaN in that voxel's channels only."""
    sc = cts.saturation(nan_voxel)
    want, got = _both_entries(dev, oracle, arith, "saturation%d" % nan_voxel, sc)
    ref = sc["feats"][0][0].astype(np.float64)
    zero_taps = ref * ref / 3.0 - (ref / 3.0) ** 2
    for d in sc["far_planes"]:           # (the oracle's own far planes; got was compared with them above)
        assert (np.abs(want[0, :, d] - zero_taps) <= 1e-5 * np.maximum(1.0, zero_taps)).all()


@pytest.mark.parametrize("W", [96, 70, 40])
def test_taps_leave_the_image_on_every_side(dev, oracle, arith, W):
    """Left/top (source 1) and right/bottom (source 2) inside one wave; W = 70: W % 4 != 0; W = 40: lanes beyond the image."""
    _both_entries(dev, oracle, arith, "edges%d" % W, cts.image_edges(W))


def test_box_overflow_takes_the_fallback(dev, oracle, arith):
    """8 planes of a wave span more than the staged box: the direct-gather fall-back.  Bit-equal to the same planes built one
    at a time (one plane per wave: fits), in both modes and on both entries."""
    sc = cts.box_overflow()
    _, got = _both_entries(dev, oracle, arith, "overflow", sc)
    D = sc["depth"].shape[1]
    for use_pc in (False, True):
        for d in range(D):
            one = _build(dev, sc, use_pc, d, d + 1)
            assert np.array_equal(one[:, :, 0], got[use_pc][:, :, d]), (use_pc, d)


@pytest.mark.parametrize("V,C,D", [(3, 32, 12), (3, 32, 5), (5, 32, 8)])
def test_tail_groups_and_shared_form(dev, oracle, arith, V, C, D):
    """D = 12 (window of 12): no group of 8, three groups of 4; D = 5: a group of one plane in the 4-plane instance (its three
    tail planes take no part in the box and store nothing); 5 views, D = 8: the shared 2 x 2 form.  Windows: same bits."""
    sc = cts.tail_group(V, C, D)
    _, got = _both_entries(dev, oracle, arith, "tail%d_%d" % (V, D), sc)
    for use_pc in (False, True):
        for lo, hi in ((0, D), (1, D), (D - 3, D - 1)):
            part = _build(dev, sc, use_pc, lo, hi)
            assert np.array_equal(part, got[use_pc][:, :, lo:hi]), (use_pc, lo, hi)


def test_cells_next_to_the_border_and_beyond_int16(dev, oracle, arith):
    """Cells -2, -1, 0, W-2, W-1, W and 1.25e6 in one wave: the in-image test is (ix0 + 1) <= W, unsigned, as before."""
    _both_entries(dev, oracle, arith, "clamp", cts.clamp_extents())
