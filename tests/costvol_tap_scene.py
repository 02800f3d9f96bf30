"""Scenes for the tap bookkeeping of the staged cost-volume build (tests/test_costvol_tap_bookkeeping.py): small inputs whose
source taps saturate the float -> int conversion, leave the image on every side inside one wave, overflow the staging box,
end in a cut-short plane group, or sit on the cells next to the image border.

Host code (numpy + the CPU oracle's coordinates); tests/test_costvol_tap_scene_cpu.py checks that every scene really has the
property it is named for, so that no GPU case passes vacuously.

A tap's north-west cell is floor(px), px = samp * W / (W - 1) - 0.5 (the reference normalises by (W - 1) / 2 and
grid_sample un-normalises with align_corners=False); cells() evaluates that in float64 from the oracle's source coordinates.
"""
import numpy as np

from satmvs_amd import rpc_synth


def _feats(V, C, H, W, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((1, C, H, W)).astype(np.float32) for _ in range(V)]


def _four(planes, H, W):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(planes, np.float32)[:, :, None, None], planes.shape + (H, W))).copy()


def affine_rpcs(V, H, W, seed):
    """Views without the seeded higher-order terms: the source coordinate is x + tilt_v * (h - 200) / 200 * W / 2 to ~1e-10 px,
    for any height -- a height of 1e9 m is 8.75e6 columns away at W = 70, not wherever a cubic's tail happens to point."""
    return rpc_synth.make_view_rpcs(V, H, W, seed=seed, num_noise=0.0, den_noise=0.0)[None]


def saturation(nan_voxel=False):
    """3 views, D=8, 40 x 70, C=8 (4 planes per wave).  Plane 3 stands 1e9 m off: its taps are ~ +-8.75e6 columns and ~ +-1e6 rows
    away (beyond int16, inside int32).  Plane 6 stands 3e12 m off: ~ +-2.6e10 columns, the conversion to int32 saturates at both
    ends.  Both share their waves with the valid taps of the other planes.  nan_voxel: one height of a valid plane is NaN."""
    V, C, D, H, W = 3, 8, 8, 40, 70
    rpc = affine_rpcs(V, H, W, seed=31)
    planes = np.array([[3.7, 47.3, 101.9, 1.0e9, 149.1, 231.7, 3.0e12, 277.3]], np.float32)
    depth = planes
    nan_at = None
    if nan_voxel:
        depth = _four(planes, H, W)
        nan_at = (0, 4, 17, 33)
        depth[nan_at] = np.nan
    return dict(feats=_feats(V, C, H, W, 32), rpc=rpc, depth=depth, nan_at=nan_at, far_planes=(3, 6), H=H, W=W)


def image_edges(W):
    """3 views, D=8, 24 x W, C=8.  Source 1 is shifted by (-9.3, -1.6) pixels, source 2 by (+9.3, +1.6): taps leave the image on
    the left and at the top (source 1), on the right and at the bottom (source 2), each inside one 32 x 2 wave patch that also
    holds taps inside.  W = 96: three whole tiles; 70: ragged, W % 4 != 0; 40: lanes beyond the image in the second tile."""
    V, C, D, H = 3, 8, 8, 24
    rpc = rpc_synth.make_view_rpcs(V, H, W, seed=33)[None]
    rpc[0, 1, rpc_synth.SAMP_OFF] -= 9.3
    rpc[0, 1, rpc_synth.LINE_OFF] -= 1.6
    rpc[0, 2, rpc_synth.SAMP_OFF] += 9.3
    rpc[0, 2, rpc_synth.LINE_OFF] += 1.6
    planes = np.linspace(11.0, 389.0, D, dtype=np.float32)[None]
    return dict(feats=_feats(V, C, H, W, 34), rpc=rpc, depth=planes, nan_at=None, H=H, W=W)


def box_overflow():
    """2 views, D=8, 24 x 96, C=32 (8 planes per wave).  Heights 0 .. 4 000 m: the source column moves by 0.012 px per metre
    (tilt 0.05, W / 2 = 48, height scale 200), 48 columns over the sweep and 7 between neighbouring planes -- the 8 planes of a
    wave's 32 columns span far more than the 44 staged columns, so every wave with taps inside the image takes the direct-gather fall-back.
    Plane by plane (one plane per launch) a wave's taps span 32 columns + slope and fit."""
    V, C, D, H, W = 2, 32, 8, 24, 96
    rpc = rpc_synth.make_view_rpcs(V, H, W, seed=35)[None]
    planes = np.linspace(0.0, 4000.0, D, dtype=np.float32)[None]
    return dict(feats=_feats(V, C, H, W, 36), rpc=rpc, depth=planes, nan_at=None, H=H, W=W)


def tail_group(V, C, D):
    """18 x 45 tiles (ragged in x and y).  D = 12, C = 32, 3 views: the sweep does not divide into eights, three full groups of
    4 planes; D = 5: 4 planes per wave, the second group holds 1 plane; 5 views, D = 8: the shared 2 x 2 form."""
    H, W = 18, 45
    rpc = rpc_synth.make_view_rpcs(V, H, W, seed=37 + V)[None]
    planes = np.linspace(7.0, 393.0, D, dtype=np.float32)[None]
    return dict(feats=_feats(V, C, H, W, 38 + D), rpc=rpc, depth=planes, nan_at=None, H=H, W=W)


def clamp_extents():
    """2 views, D=8, 6 x 10, C=32 (8 planes per wave; one wave holds the whole image).  Affine views: the source column is
    x + 0.00125 (h - 200).  The heights put column 0's cell on -1 and -2, column 9's on W - 1 and W, and one plane 1e9 m off
    (1.25e6 columns: beyond int16) -- the cells on which the in-image test (ix0 + 1) <= W, unsigned, flips."""
    V, C, D, H, W = 2, 32, 8, 6, 10
    rpc = affine_rpcs(V, H, W, seed=39)
    planes = np.array([[-1100.0, -430.0, 90.0, 230.0, 710.0, 1050.0, 1.0e9, 1900.0]], np.float32)
    return dict(feats=_feats(V, C, H, W, 40), rpc=rpc, depth=planes, nan_at=None, H=H, W=W)


def cells(orc, scene):
    """float64 north-west cells (ix0, iy0) per source: arrays (S, D, H, W); NaN where the coordinate is NaN."""
    rpc, depth, H, W = scene["rpc"], scene["depth"], scene["H"], scene["W"]
    ix, iy = [], []
    for s in range(1, rpc.shape[1]):
        _, _, samp, line = orc.rpc_warp_coords(rpc[:, s], rpc[:, 0], depth, H, W)
        ix.append(np.floor(samp[0] * W / (W - 1.0) - 0.5))
        iy.append(np.floor(line[0] * H / (H - 1.0) - 0.5))
    return np.stack(ix), np.stack(iy)
