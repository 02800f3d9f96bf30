"""The folded (plane-coefficient) source cubics in nested Horner form (csrc/smvs_device.h, o2p_pc_xn), through the C ABI
(smvs_rpc_plane_coef + smvs_rpc_costvol_fwd_pc), against the CPU oracle under a rule that does not depend on the code under
test (tests/plane_coef_scene.py): outside the float32 rounding-boundary voxels -- found in numpy.longdouble, at most 5 % of a
scene -- the exact arithmetic equals the oracle bit for bit, the fused arithmetic lies within 1e-5 max(1, |v|), and the NaN
patterns are equal.  One scene per instance or path that evaluates the nested form: 8 / 4 / 2 planes per wave (passes of 4, 4
and 2 planes), a cut-short plane group, the workgroup-shared form at four sources, batched records, the oversized-box fallback
(one plane at a time) and the check-and-redo path of a wave whose heights are not its planes'."""
import numpy as np
import pytest
import torch

import plane_coef_scene as pcs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _build(dev, feats, rpc, depth, planes=None, use_pc=True):
    """The volume through the C ABI: coefficients folded for `planes` (default: the heights themselves), then the build on `depth`."""
    from satmvs_amd import _lib
    f = [_t(x, dev) for x in feats]
    r, d = _t(rpc, dev), _t(depth, dev)
    B, C, H, W = f[0].shape
    D = d.shape[1]
    is4d = 1 if d.dim() == 4 else 0
    out = torch.full((B, C, D, H, W), 7.0, dtype=torch.float32, device=dev)
    st = _lib.current_stream(dev)
    srcs = _lib.ptr_array(f[1:])
    if not use_pc:
        _lib.call("smvs_rpc_costvol_fwd", _lib.ptr(f[0]), srcs, len(f) - 1, _lib.ptr(r), _lib.ptr(d), is4d, _lib.ptr(out),
                  B, C, D, H, W, 0, D, D, 0, st)
    else:
        pc = torch.zeros(_lib.load().smvs_rpc_plane_coef_bytes(B, len(f) - 1, D) // 8, dtype=torch.float64, device=dev)
        pl = d if planes is None else _t(planes, dev)
        _lib.call("smvs_rpc_plane_coef", _lib.ptr(r), _lib.ptr(pl), 1 if pl.dim() == 4 else 0, _lib.ptr(pc), B, len(f) - 1, D, H, W, 0, D, st)
        _lib.call("smvs_rpc_costvol_fwd_pc", _lib.ptr(f[0]), srcs, len(f) - 1, _lib.ptr(r), _lib.ptr(d), is4d, _lib.ptr(pc), _lib.ptr(out),
                  B, C, D, H, W, 0, D, D, 0, st)
    torch.cuda.synchronize()
    return out.cpu().numpy()


_REFERENCE = {}


def _reference(oracle, name):
    """(features, rpc, heights, the oracle's volume, the interior (pixel, plane)s): computed once per scene, never written to"""
    if name not in _REFERENCE:
        feats, rpc, depth = pcs.load(name)
        H, W = feats[0].shape[2:]
        bnd = pcs.boundary(rpc, depth, H, W)
        assert bnd.mean() <= pcs.MAX_BOUNDARY, bnd.mean()                   # a condition on the inputs (see the CPU test)
        want = oracle.costvol_variance(feats, rpc, depth, "rpc")
        for a in (want, bnd):
            a.setflags(write=False)
        _REFERENCE[name] = (feats, rpc, depth, want, ~bnd)
    return _REFERENCE[name]


def _accept(got, want, interior, arith):
    C = got.shape[1]
    m = np.broadcast_to(interior[:, None], got.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    g, w = got[m], want[m]
    ok = ~np.isnan(w)
    g, w = g[ok], w[ok]
    nbad = int((g != w).sum())
    err = float(np.abs(g.astype(np.float64) - w).max())
    rel = float((np.abs(g.astype(np.float64) - w) / (1e-5 * np.maximum(1.0, np.abs(w)))).max())
    print("%s: %d of %d interior voxels differ from the oracle, max |diff| %.3g = %.3g of the fused bound; %d boundary voxels set aside"
          % (arith, nbad, g.size, err, rel, C * int((~interior).sum())))
    if arith == "exact":
        assert nbad == 0, (nbad, err)
    else:
        assert rel <= 1.0, rel


@pytest.mark.parametrize("name", list(pcs.SCENES) + ["overflow"])
def test_folded_build_equals_the_oracle_off_the_rounding_boundaries(dev, oracle, arith, name):
    feats, rpc, planes, want, interior = _reference(oracle, name)
    _accept(_build(dev, feats, rpc, planes), want, interior, arith)


def test_folded_build_takes_plane_heights_as_a_volume_too(dev, oracle, arith):
    """(B,D,H,W) heights that equal their planes': the same waves, the same records, the same bits as (B,D) heights"""
    feats, rpc, planes, want, interior = _reference(oracle, "dp4_d6")
    H, W = feats[0].shape[2:]
    got = _build(dev, feats, rpc, pcs.four(planes, H, W))
    _accept(got, want, interior, arith)
    assert np.array_equal(got, _build(dev, feats, rpc, planes))


def test_one_jittered_pixel_sends_its_wave_down_the_trivariate_chain(dev, oracle, arith):
    """Coefficients folded for the planes, heights with one pixel 1.5 m off: the wave that holds it redoes its planes on the
    trivariate chain with its own heights -- the bits of the build without coefficients there, the oracle's everywhere
    off the rounding boundaries."""
    feats, rpc, depth, want, interior = _reference(oracle, "jittered")
    planes = pcs.scene("dp8_d8")[2]
    got = _build(dev, feats, rpc, depth, planes=planes)
    _accept(got, want, interior, arith)
    tri = _build(dev, feats, rpc, depth, use_pc=False)
    d, y, x = pcs.JITTER_AT
    y0, x0 = y // pcs.WAVE_Y * pcs.WAVE_Y, x // pcs.WAVE_X * pcs.WAVE_X
    assert np.array_equal(got[:, :, :, y0:y0 + pcs.WAVE_Y, x0:x0 + pcs.WAVE_X], tri[:, :, :, y0:y0 + pcs.WAVE_Y, x0:x0 + pcs.WAVE_X])
    # ... and the jitter is seen: the voxel is not the plane's
    clean = _reference(oracle, "dp8_d8")[3]
    assert not np.array_equal(got[0, :, d, y, x], clean[0, :, d, y, x])
