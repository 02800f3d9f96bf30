"""The scenes of tests/plane_coef_scene.py have the properties the GPU tests rely on (no GPU needed): few rounding-boundary
voxels, a long-double reference that the oracle's float64 chain follows far inside the boundary margin, a box overflow where
one is meant."""
import numpy as np
import pytest

import plane_coef_scene as pcs


@pytest.mark.parametrize("name", pcs.ALL)
def test_boundary_voxels_are_few_and_the_reference_is_tight(oracle, name):
    feats, rpc, depth = pcs.load(name)
    H, W = feats[0].shape[2:]
    frac = float(pcs.boundary(rpc, depth, H, W).mean())
    print("%s: %.2f %% boundary voxels" % (name, 100 * frac))
    assert frac <= pcs.MAX_BOUNDARY, frac
    # the oracle's float64 chain against the long-double one: what the margin has to cover
    samp, line = pcs.reference_coords(rpc, depth, H, W)
    worst = 0.0
    for s in range(1, rpc.shape[1]):
        _, _, os_, ol = oracle.rpc_warp_coords(rpc[:, s], rpc[:, 0], depth, H, W)
        worst = max(worst, float(np.abs(os_ - samp[:, s - 1]).max()), float(np.abs(ol - line[:, s - 1]).max()))
    print("%s: float64 chain within %.3g px of the long-double one" % (name, worst))
    assert worst <= pcs.BOUNDARY_PX / 10, worst


def test_long_double_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < 1e-18


def test_overflow_scene_overflows():
    feats, rpc, planes = pcs.overflow()
    H, W = feats[0].shape[2:]
    samp, line = pcs.reference_coords(rpc, planes, H, W)
    bw, bh = pcs.wave_boxes(samp, line, H, W, 8)
    assert (bw > pcs.BOX_W).any() or (bh > pcs.BOX_H).any(), (bw.max(), bh.max())
