"""Scenes and the acceptance rule for the folded (plane-coefficient) source cubics of the cost-volume build
(tests/test_plane_coef_horner.py): the smallest shapes at which each instance that evaluates o2p_pc_xn (csrc/smvs_device.h) can
go wrong, and a rule that does not depend on the code under test.

Host code (numpy + the CPU oracle); tests/test_plane_coef_scene_cpu.py checks the conditions on the inputs.

The rule.  The build rounds a source view's float64 pixel coordinates (samp, line) to float32 and does float32 arithmetic
from there on, bit for bit the oracle's.  A voxel can therefore differ from the oracle only where one of its float64 coordinates
lies so close to the midpoint of two neighbouring float32 values that float64 rounding decides which way it falls.
reference_coords() evaluates the reference chain (RPC_Photo2Obj of the ref pixel, RPC_Obj2Photo into every source) in
numpy.longdouble; boundary() marks a (pixel, plane) whose coordinates come within BOUNDARY_PX of such a midpoint.  The
reference's own float64 evaluation scatters by up to 2.7e-10 px around the long-double value on these synthetic RPCs (the CPU
test measures it against the oracle's coordinates), the nested evaluation of the folded cubics adds ~1e-13 px: 1e-8 px covers both
37 times over.  Everywhere else: exact arithmetic equals the oracle bit for bit, fused arithmetic lies within
1e-5 max(1, |v|), and the NaN patterns are equal.  So that the rule has teeth, boundary voxels are at most MAX_BOUNDARY of every
scene -- a condition on the inputs (small coordinates have small ulps: a coordinate below 1 px is within 1e-8 px of a midpoint
one time in three, one at 64 px one time in 380), met by the choice of seeds and tile sizes.
"""
import numpy as np

from satmvs_amd import rpc_synth as R

BOUNDARY_PX = 1e-8
MAX_BOUNDARY = 0.05
WAVE_X, WAVE_Y = 32, 2          # ref pixels of one wave (csrc/costvol_kernels.h, WV_TX x WV_TY)
BOX_W, BOX_H = 44, 5            # staged box of a per-wave instance (DM_BW x DM_R)


def _inputs(B, V, C, D, H, W, seed, lo=0.0, hi=400.0):
    rng = np.random.default_rng(seed)
    feats = [rng.standard_normal((B, C, H, W)).astype(np.float32) for _ in range(V)]
    rpc = np.stack([R.make_view_rpcs(V, H, W, seed=seed + 7 * b) for b in range(B)])
    planes = np.stack([np.linspace(lo, hi, D) + 3.0 * b for b in range(B)]).astype(np.float32)
    return feats, rpc, planes


def four(planes, H, W):
    return np.ascontiguousarray(np.broadcast_to(planes[:, :, None, None], planes.shape + (H, W))).copy()


# name -> (B, V, C, D, H, W, seed): what the case reaches (csrc/costvol_kernels.h, launch_ct)
SCENES = {
    "dp8_d8": (1, 3, 32, 8, 170, 182, 5),           # 8 planes per wave (the headline instance), two passes of 4
    "dp8_d16": (1, 3, 32, 16, 170, 182, 6),         # ... two plane groups
    "dp4_d4": (1, 3, 8, 4, 170, 182, 7),            # 4 planes per wave: one pass of 4 since the nested form
    "dp4_d12": (1, 3, 8, 12, 170, 182, 8),          # ... three groups
    "dp4_d6": (1, 3, 8, 6, 170, 182, 9),            # ... the second group cut short: its pass reads two records behind the sweep
    "shared_2x2": (1, 5, 32, 8, 340, 366, 10),      # 4 sources: workgroup of 2 x 2 waves, 4 planes each
    "dp2": (1, 2, 16, 2, 90, 100, 11),           # 2 planes per wave, one source
    "batched": (2, 3, 8, 4, 170, 182, 12),          # two items with RPCs and planes of their own: records at [b][source][cubic][d]
}


def scene(name):
    B, V, C, D, H, W, seed = SCENES[name]
    feats, rpc, planes = _inputs(B, V, C, D, H, W, seed)
    return feats, rpc, planes


def overflow():
    """3 views, C=32, D=8: planes 230 m apart.  The 8 planes of a wave spread its taps over more columns than the staged
    box holds, so the wave gathers directly and rebuilds its taps plane by plane: o2p_pc_xn<1>."""
    return _inputs(1, 3, 32, 8, 170, 182, 13, lo=-600.0, hi=1000.0)


JITTER_AT = (3, 5, 17)          # plane, row, column


def jittered():
    """dp8_d8 as (B,D,H,W) heights with ONE pixel of one plane 1.5 m off its plane: its wave (rows 4-5, columns 0-31, all 8
    planes) fails the check of its heights against the folded planes' and redoes its planes on the trivariate chain."""
    feats, rpc, planes = scene("dp8_d8")
    depth = four(planes, 170, 182)
    depth[(0,) + JITTER_AT] += np.float32(1.5)
    return feats, rpc, planes, depth


def load(name):
    """(features, rpc, heights) of a scene by name; heights (B,D), or (B,D,H,W) for "jittered"""
    if name == "overflow":
        return overflow()
    if name == "jittered":
        feats, rpc, _, depth = jittered()
        return feats, rpc, depth
    return scene(name)


ALL = list(SCENES) + ["overflow", "jittered"]


def _cubics(P, L, H, coeffs):
    """sum_i c_i m_i(P, L, H) for each 20-vector of `coeffs`, monomials in the reference's order
    1,L,P,H,LP,LH,PH,LL,PP,HH,PLH,LLL,LPP,LHH,LLP,PPP,PHH,LLH,PPH,HHH (one monomial at a time: no (..., 20) long-double stack)"""
    LL, PP, HH = L * L, P * P, H * H
    mono = (None, L, P, H, L * P, L * H, P * H, LL, PP, HH, P * L * H, L * LL, L * PP, L * HH, LL * P, P * PP, P * HH, LL * H, PP * H, H * HH)
    out = [np.full(P.shape, c[0], np.longdouble) for c in coeffs]
    for i in range(1, 20):
        for o, c in zip(out, coeffs):
            o += c[i] * mono[i]
    return out


def reference_coords(rpc, depth, H, W):
    """(samp, line) of every source view, (B, V-1, D, H, W) each, in numpy.longdouble: the reference chain
    (rpc_synth.photo2obj / obj2photo, the sum of 20 products in the reference's monomial order) on the float32 heights."""
    ld = np.longdouble
    rpc = np.asarray(rpc, np.float64).astype(ld)
    B, V = rpc.shape[:2]
    h = np.asarray(depth, np.float32)
    h = (h[:, :, None, None] if h.ndim == 2 else h).astype(ld)
    D = h.shape[1]
    h = np.broadcast_to(h, (B, D, H, W))
    x = np.broadcast_to(np.arange(W, dtype=ld)[None, None, None, :], (B, D, H, W))
    y = np.broadcast_to(np.arange(H, dtype=ld)[None, None, :, None], (B, D, H, W))
    samp, line = np.empty((B, V - 1, D, H, W), ld), np.empty((B, V - 1, D, H, W), ld)
    for b in range(B):
        r = rpc[b, 0]
        an, ad, on, od = _cubics((x[b] - r[R.SAMP_OFF]) / r[R.SAMP_SCALE], (y[b] - r[R.LINE_OFF]) / r[R.LINE_SCALE], (h[b] - r[R.HEIGHT_OFF]) / r[R.HEIGHT_SCALE],
                                 (r[R.LATNUM], r[R.LATDEN], r[R.LONNUM], r[R.LONDEN]))
        lat = an / ad * r[R.LAT_SCALE] + r[R.LAT_OFF]
        lon = on / od * r[R.LONG_SCALE] + r[R.LONG_OFF]
        for s in range(1, V):
            r = rpc[b, s]
            sn, sd, ln, ldn = _cubics((lat - r[R.LAT_OFF]) / r[R.LAT_SCALE], (lon - r[R.LONG_OFF]) / r[R.LONG_SCALE], (h[b] - r[R.HEIGHT_OFF]) / r[R.HEIGHT_SCALE],
                                      (r[R.SNUM], r[R.SDEN], r[R.LNUM], r[R.LDEN]))
            samp[b, s - 1] = sn / sd * r[R.SAMP_SCALE] + r[R.SAMP_OFF]
            line[b, s - 1] = ln / ldn * r[R.LINE_SCALE] + r[R.LINE_OFF]
    return samp, line


def _near_midpoint(c):
    """c (longdouble) within BOUNDARY_PX of the midpoint of two neighbouring float32 values"""
    f = c.astype(np.float32)                                        # either neighbour will do: both of its midpoints are looked at
    up = (f.astype(np.longdouble) + np.nextafter(f, np.float32(np.inf)).astype(np.longdouble)) / 2
    dn = (f.astype(np.longdouble) + np.nextafter(f, np.float32(-np.inf)).astype(np.longdouble)) / 2
    return np.minimum(np.abs(c - up), np.abs(c - dn)) <= BOUNDARY_PX


def boundary(rpc, depth, H, W):
    """(B, D, H, W) bool: some source coordinate of the (pixel, plane) is a float32 rounding boundary case"""
    samp, line = reference_coords(rpc, depth, H, W)
    return (_near_midpoint(samp) | _near_midpoint(line)).any(axis=1)


def wave_boxes(samp, line, H, W, dp):
    """Per (source, plane group, wave) the columns and rows that the staged box of a per-wave instance must hold: the extent of the
    tap cells that touch the image (+ 2: the east / south neighbours), as csrc/costvol_kernels.h part B takes it before aligning the
    origin.  Returns (widths, heights), flat."""
    B, S, D = samp.shape[:3]
    px = np.asarray(samp, np.float64) * W / (W - 1) - 0.5
    py = np.asarray(line, np.float64) * H / (H - 1) - 0.5
    ix, iy = np.floor(px), np.floor(py)
    ok = (ix >= -1) & (ix <= W - 1) & (iy >= -1) & (iy <= H - 1)
    bw, bh = [], []
    for b in range(B):
        for s in range(S):
            for d0 in range(0, D, dp):
                for y0 in range(0, H, WAVE_Y):
                    for x0 in range(0, W, WAVE_X):
                        sl = (b, s, slice(d0, d0 + dp), slice(y0, y0 + WAVE_Y), slice(x0, x0 + WAVE_X))
                        m = ok[sl]
                        if m.any():
                            bw.append(ix[sl][m].max() - ix[sl][m].min() + 2)
                            bh.append(iy[sl][m].max() - iy[sl][m].min() + 2)
    return np.array(bw), np.array(bh)
