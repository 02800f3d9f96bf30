"""Scenes, a float64 reference with a per-cell derived bound, and a census of the paths smvs_costvol_bwd (csrc/costvol_bwd.hip)
takes, for tests/test_costvol_bwd_scene_cpu.py (which asserts, without a GPU, what the GPU tests assume about these scenes),
tests/test_costvol_bwd_gpu.py and tests/fuzz/fuzz_costvol_bwd.py.

Host code: numpy + the CPU oracle (`orc`, oracle/oracle.py, handed in by the caller).  Taps are the oracle's float32 source
coordinates (ops_scene.oracle_grid -> ops_scene.taps_from_grid, once per source view); everything after the taps is float64.

    warped_s = sum_q a_q w_q   (a dropped corner reads 0)        m = (r + sum_s warped_s) / V
    kappa_s  = g (2/V) (warped_s - m)                             grad_src_s = scatter of kappa_s w_q
    grad_ref = sum_d g (2/V) (r - m)

The bound.  u = 2^-24, gamma(n) = n u / (1 - n u), A_s = sum_q |a_q w_q|, M = |r| + sum_s A_s.  Counted from the kernel:
  * the four weights are the products tap_from_grid forms, in both scatter schemes: the same float32 numbers as the reference's;
  * warped_s: a0 w0, then three fma (register scheme) or two products, two fma and one addition (boxed): every term passes at
    most 4 roundings, |error| <= 4 u A_s;
  * sum = r + warped_1 + ...: V - 1 additions of partial sums below M, plus the taps' errors: |error| <= (V + 3) u M;
  * m = sum / V: div_by_views is correctly rounded, the interior of the boxed path multiplies by RN(1/V) (two roundings):
    |error of m| <= ((V + 3) u M + 2 u M) / V = (V + 5) u M / V;
  * warped_s - m: |error| <= (4 + (V + 5) / V) u M before the subtraction rounds;  r - m: (V + 5) u M / V (r is exact);
  * then the subtraction, RN(2/V), g * RN(2/V) and the product with the difference: 4 relative roundings of the coefficient
    (3 for the reference gradient, whose last product is inside an fma that is counted with the sum below).
(A count that does not divide the sum's error by V arrives at (V + 8) M; 4 + (V + 5) / V <= 7.5 is what the operations give.)  With E_s = |g| (2/V) [(4 + (V + 5) / V) M + 4 |warped_s - m|] and E_r = |g| (2/V) [((V + 5) / V) M + 3 |r - m|]:
  * grad_src cell with n contributions: one rounding per product kappa w and at most n - 1 additions in any order (float32
    atomics, run registers, or a float64 box rounded once per flush, which replaces the additions it holds by one rounding):
        gamma(n + 1) sum |kappa w| + (1 + gamma(n + 1)) u sum E_s w
  * grad_ref cell: D fma (each rounds a partial sum) and one atomic per plane chunk:
        gamma(D + chunks) sum_d |g (2/V)(r - m)| + (1 + gamma(D + chunks)) u sum_d E_r
  * a buffer that is not zero when the call starts takes part in every atomic that reaches the cell, at most one per
    contribution (grad_src) resp. one per chunk (grad_ref): + gamma(n) |initial| resp. gamma(chunks) |initial|, and the n - 1
    additions become n (already inside n + 1 above: the product's rounding touches one term only).
No coordinate term: the backward runs the forward's coordinate chain, which equals the oracle's bit for bit.
"""
import functools

import numpy as np

import costvol_tap_scene as cts
import ops_scene as S
from satmvs_amd import rpc_synth

U = S.U32
BOX_W, BOX_H, BOX_MAX_SRC = 64, 8, 4
OLD_RTOL = 1e-4                      # the criterion the backward was held by so far: max |got - other| <= 1e-4 max |other|
GUARD = 64                           # guard words on either side of every gradient buffer


def src_class(n_src):
    return "1-2" if n_src <= 2 else "3-4" if n_src <= 4 else "5-7"


def patch(n_src):
    """(width, height) of a wave's pixels."""
    return (32, 2) if n_src <= BOX_MAX_SRC else (64, 1)


def chunk(n_src):
    """planes per lane (launch_bwd_n)."""
    return 8 if n_src <= 4 else 2


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def _rpc_views(B, V, H, W, seed, tilts=None, affine=False):
    gh, gw = max(H, 16), max(W, 16)                        # the cameras of a tile of at least 16 x 16 (ops_scene.scene)
    kw = dict(num_noise=0.0, den_noise=0.0) if affine else {}
    return np.stack([rpc_synth.make_view_rpcs(V, gh, gw, seed=seed + 7 * b, tilts=tilts, **kw) for b in range(B)])


def _pinhole_views(B, V, H, W, rng):
    gh, gw = max(H, 16), max(W, 16)
    gp = np.zeros((B, V, 4, 4))
    for b in range(B):
        for v in range(V):
            f = 1.1 * gw
            K = np.array([[f, 0, gw / 2.0, 0], [0, f, gh / 2.0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1]])
            E = np.eye(4)
            a = rng.normal(0, 0.02) * (v > 0)
            E[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
            E[:3, 3] = [25.0 * v * (-1) ** v, 3.0 * v, 0.5 * v]
            gp[b, v] = K @ E
    return gp


def _const_view(px, py):
    """Pinhole source whose x and y rows ignore the pixel (with an identity reference): every voxel lands on (px, py)."""
    P = np.zeros((4, 4))
    P[0, 3], P[1, 3], P[2, 3], P[3, 3] = px, py, 1.0, 1.0
    return P


def _sweep_view(shift, t, yshift=0.0, ty=0.0):
    """Pinhole source (identity reference) with px = x + shift + t / depth, py = y + yshift + ty / depth."""
    return np.array([[1.0, 0, shift, t], [0, 1.0, yshift, ty], [0, 0, 1.0, 0], [0, 0, 0, 1.0]])


def _planes(lo, hi, D, B):
    if D == 1:
        return np.full((B, 1), 0.5 * (lo + hi), np.float32)
    return np.linspace(lo, hi, D, dtype=np.float32)[None].repeat(B, 0)


def _spec(V, geo, B, C, D, H, W, px, needs=(), **kw):
    return dict(V=V, geo=geo, B=B, C=C, D=D, H=H, W=W, px=px, needs=tuple(needs), **kw)


# name -> spec.  `needs`: census properties the case is there for (test_costvol_bwd_scene_cpu asserts each).  W % 64 takes
# 1, 31, 32, 33, 63, 0; H both parities; D 1, 7, 8, 9, 17 up to 4 sources and 1, 2, 3 beyond; C 1, 2, 3, 5.
CASES = {
    # every view count in both geometries, small parallax (boxed wherever boxes exist)
    "v2_rpc":      _spec(2, "rpc", 1, 2, 8, 6, 64, False, ["boxed", "rows_lt8", "overhang_e"]),
    "v2_pin":      _spec(2, "pinhole", 2, 1, 9, 7, 65, True, ["boxed", "cut_chunks", "inactive_lanes", "w_partial"]),
    "v3_rpc":      _spec(3, "rpc", 2, 3, 17, 9, 95, True, ["boxed", "cut_chunks", "inactive_lanes"]),
    "v3_pin":      _spec(3, "pinhole", 1, 5, 7, 8, 33, False, ["boxed", "cut_chunks", "overhang_e"]),
    "v4_rpc":      _spec(4, "rpc", 1, 1, 1, 5, 31, True, ["boxed", "cut_chunks", "overhang_s"]),
    "v4_pin":      _spec(4, "pinhole", 2, 2, 8, 4, 96, False, ["boxed"]),
    "v5_rpc":      _spec(5, "rpc", 1, 3, 9, 7, 127, False, ["boxed", "cut_chunks"]),
    "v5_pin":      _spec(5, "pinhole", 1, 2, 17, 6, 63, True, ["boxed", "cut_chunks"]),
    "v6_rpc":      _spec(6, "rpc", 2, 2, 3, 5, 65, True, ["register", "cut_chunks", "takes", "runs2", "inactive_lanes"]),
    "v6_pin":      _spec(6, "pinhole", 1, 1, 1, 4, 95, False, ["register", "cut_chunks"]),
    "v7_rpc":      _spec(7, "rpc", 1, 5, 2, 3, 33, False, ["register", "takes"]),
    "v7_pin":      _spec(7, "pinhole", 1, 3, 3, 6, 64, True, ["register", "cut_chunks"]),
    "v8_rpc":      _spec(8, "rpc", 1, 2, 3, 4, 127, True, ["register", "runs2", "runs_lastgive"]),
    "v8_pin":      _spec(8, "pinhole", 2, 1, 2, 5, 96, False, ["register"]),
    # degenerate sizes: the reference normalises by (W - 1) / 2 resp. (H - 1) / 2 = 0
    "h1_v3":       _spec(3, "rpc", 1, 2, 3, 1, 40, False, ["nonfinite"]),
    "w1_v3":       _spec(3, "rpc", 1, 2, 3, 9, 1, True, ["nonfinite"]),
    "h1_v6":       _spec(6, "pinhole", 1, 2, 3, 1, 70, False, ["nonfinite"]),
    "w1_v6":       _spec(6, "rpc", 1, 1, 2, 5, 1, False, ["nonfinite"]),
    "2x2_v3":      _spec(3, "rpc", 1, 3, 8, 2, 2, True, ["inactive_lanes"]),
    "2x2_v6":      _spec(6, "rpc", 1, 3, 3, 2, 2, True, ["inactive_lanes"]),
    # parallax: huge (no box fits: register scheme everywhere), mixed (a height ramp across the image: both kinds of wave in one launch)
    "huge_v3":     _spec(3, "rpc", 1, 2, 17, 12, 128, True, ["register", "few_boxed", "cut_chunks"], span=(0.0, 30000.0), affine=True),
    "huge_v5":     _spec(5, "rpc", 1, 2, 17, 16, 128, True, ["register", "few_boxed", "cut_chunks"], span=(0.0, 30000.0), affine=True),
    # (there a corner wave that keeps one plane of full taps inside the image still fits its boxes; pinhole views that sweep 24 rows
    # up the image over the planes leave no such wave)
    "sweep_v3":    _spec(3, "sweep2", 1, 2, 8, 16, 40, False, ["register", "no_boxed", "takes"]),
    "sweep_v5":    _spec(5, "sweep2", 1, 1, 8, 16, 33, False, ["register", "no_boxed", "takes"]),
    "mixed_v3":    _spec(3, "rpc", 1, 2, 8, 12, 130, True, ["boxed", "register"], ramp=40.0),
    "mixed_v4":    _spec(4, "rpc", 1, 2, 9, 10, 128, True, ["boxed", "register"], ramp=40.0),
    # one quiet view beside one that sweeps across the image: register waves with runs, hand-overs and border taps
    "runs_v3":     _spec(3, "sweep", 1, 2, 8, 6, 70, False, ["register", "takes", "runs2", "runs_lastgive", "w_partial", "w_dropped"]),
    "runs_v5":     _spec(5, "sweep", 1, 2, 9, 6, 70, False, ["register", "takes", "runs2", "runs_lastgive", "w_partial", "w_dropped", "cut_chunks"]),
    # views that leave the image on each of the four sides inside one wave
    "edges_v3":    _spec(3, "edges", 1, 2, 8, 24, 70, False, ["boxed", "w_partial", "w_dropped"]),
    "edges_v5":    _spec(5, "edges", 1, 2, 8, 12, 40, False, ["boxed", "w_partial", "w_dropped"]),
    "edges_v6":    _spec(6, "edges", 1, 2, 3, 12, 70, False, ["register", "w_partial", "w_dropped", "w_view_none"]),
    # far planes (all taps dropped) and one NaN height: tests/costvol_tap_scene.py's affine RPCs
    "far_v3":      _spec(3, "far", 1, 2, 8, 40, 70, False, ["w_dropped"]),
    "far_nan_v3":  _spec(3, "far", 1, 2, 8, 40, 70, True, ["w_dropped", "nonfinite"], nan_height=True),
    # collapse: every voxel of a view lands in one cell
    "collapse_v3": _spec(3, "collapse", 1, 2, 8, 12, 40, False, ["boxed", "rows_lt8", "hot"]),
    "collapse_v6": _spec(6, "collapse", 1, 1, 3, 6, 70, False, ["register", "runs2", "hot"]),
    "collapse_runs_v3": _spec(3, "collapse_sweep", 1, 2, 8, 6, 70, False, ["register", "runs8", "hot"]),
    # grad_var and feature variants of one boxed scene
    "g_zero":      _spec(3, "rpc", 1, 2, 8, 6, 70, False, ["boxed"], gmode="zero"),
    "g_zero_box":  _spec(3, "rpc", 1, 2, 8, 6, 70, False, ["boxed"], gmode="zero_box"),
    "g_nan_inf":   _spec(3, "rpc", 1, 2, 8, 6, 70, False, ["boxed", "nonfinite"], gmode="nan_inf"),
    "g_nan_inf_v6": _spec(6, "rpc", 1, 2, 3, 6, 70, False, ["register", "nonfinite"], gmode="nan_inf"),
    "f_nan":       _spec(3, "rpc", 1, 2, 8, 6, 70, False, ["boxed", "nonfinite"], fea_nan=True),
    "f_nan_v6":    _spec(6, "rpc", 1, 2, 3, 6, 70, False, ["register", "nonfinite"], fea_nan=True),
}
MODEL_SCENES = ("v3_rpc", "runs_v5", "v8_rpc")           # the three cases held against float64 torch autograd


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> dict(feats [V x (B,C,H,W) f32], geo 'rpc' | 'pinhole', gp (B,V,170) | (B,V,4,4) f64, depth (B,D) | (B,D,H,W) f32,
    gvar (B,C,D,H,W) f32, plus the spec).  Cached: the arrays are shared and must not be written to."""
    sp = CASES[name]
    V, B, C, D, H, W = (sp[k] for k in "VBCDHW")
    seed = 1000 + sorted(CASES).index(name)
    rng = np.random.default_rng(seed)
    feats = [rng.standard_normal((B, C, H, W)).astype(np.float32) for _ in range(V)]
    kind, geo = sp["geo"], "rpc"
    lo, hi = sp.get("span", (0.0, 400.0))
    if kind == "rpc":
        gp = _rpc_views(B, V, H, W, seed, affine=sp.get("affine", False))       # (affine: no cubic tail far outside the height range)
    elif kind == "pinhole":
        geo, gp, (lo, hi) = "pinhole", _pinhole_views(B, V, H, W, rng), sp.get("span", (400.0, 700.0))
    elif kind == "edges":                                   # costvol_tap_scene.image_edges: odd sources shifted up-left, even ones down-right
        gp = _rpc_views(B, V, H, W, seed)
        for v in range(1, V):
            sgn = -1.0 if v % 2 else 1.0
            gp[:, v, rpc_synth.SAMP_OFF] += sgn * 9.3
            gp[:, v, rpc_synth.LINE_OFF] += sgn * 1.6
        lo, hi = 11.0, 389.0
    elif kind == "far":
        gp = _rpc_views(B, V, H, W, seed, affine=True)
    elif kind in ("sweep", "sweep2", "collapse", "collapse_sweep"):
        geo = "pinhole"
        gp = np.zeros((B, V, 4, 4))
        gp[:, 0] = np.eye(4)
        lo, hi = 400.0, 700.0
        for v in range(1, V):
            if kind == "collapse":
                gp[:, v] = _const_view(3.37 + 5.21 * v, 1.61 + 0.53 * v)
            elif kind == "sweep2":
                gp[:, v] = _sweep_view(0.3 * v, 0.0, -44.0 - 0.2 * v, 22400.0)     # +12 .. -12 rows over the planes: no 8-row box fits
            elif v == V - 1:                                # the last view sweeps ~110 columns over the planes: no box fits
                gp[:, v] = _sweep_view(-195.0, 1.0e5)
            elif kind == "collapse_sweep":
                gp[:, v] = _const_view(7.37 + 5.21 * v, 2.61)
            else:                                           # quiet views: 0.3 .. 0.6 columns over the whole sweep
                gp[:, v] = _sweep_view(0.4 * v, 300.0 * v)
    planes = _planes(lo, hi, D, B)
    if kind == "far":
        planes = np.array([[3.7, 47.3, 101.9, 1.0e9, 149.1, 231.7, 3.0e12, 277.3]], np.float32)
    depth = planes
    if sp["px"]:
        depth = planes.astype(np.float64)[:, :, None, None] + rng.normal(0, 2.0, (B, D, H, W))
        if "ramp" in sp:                                    # the plane spacing grows from 1 to `ramp` times across the image
            k = np.arange(D).reshape(1, D, 1, 1) * (hi - lo) / max(D - 1, 1)
            depth = depth + k * (sp["ramp"] - 1.0) * (np.arange(W).reshape(1, 1, 1, W) / max(W - 1, 1)) ** 4
        depth = depth.astype(np.float32)
        if kind == "far":
            depth = cts._four(planes, H, W)
    if sp.get("nan_height"):
        depth[0, 4, 17, 33] = np.nan
    gvar = rng.standard_normal((B, C, D, H, W)).astype(np.float32)
    mode = sp.get("gmode", "random")
    if mode == "zero":
        gvar[:] = 0.0
    elif mode == "zero_box":                                # the pixels of one whole wave (32 x 2), all planes and channels
        gvar[:, :, :, 2:4, 32:64] = 0.0
    elif mode == "nan_inf":
        gvar[0, 0, D // 2, 3, 17] = np.nan
        gvar[0, C - 1, D - 1, 1, 50] = np.inf
    if sp.get("fea_nan"):
        feats[1][0, 0, 3, 21] = np.nan
        feats[0][0, C - 1, 2, 44] = np.nan
    out = dict(sp, name=name, feats=feats, geo=geo, gp=gp, depth=depth, gvar=gvar, n_src=V - 1)
    for a in feats + [gp, depth, gvar]:
        a.setflags(write=False)
    return out


# ---- taps and the float64 reference ------------------------------------------------------------------------------------------
def taps_of(orc, geo, gp, depth, H, W, nudge=None):
    """[(off, wts)] per source view, each (4,B,D,H,W) (ops_scene.taps_from_grid on the oracle's float32 grid).  nudge = (s, k):
    the x coordinate of source s moved by k float32 ulps (the planted error of the CPU test)."""
    out = []
    for v in range(1, gp.shape[1]):
        gx, gy = S.oracle_grid(orc, geo, np.ascontiguousarray(gp[:, v]), np.ascontiguousarray(gp[:, 0]), depth, H, W)
        if nudge is not None and nudge[0] == v - 1:
            for _ in range(abs(nudge[1])):
                gx = np.nextafter(gx, np.float32(np.inf if nudge[1] > 0 else -np.inf))
        out.append(S.taps_from_grid(gx, gy, H, W))
    return out


def reference(orc, feats, geo, gp, depth, gvar, taps=None):
    """-> dict(taps, src=[per view dict(ref, mag, extra, cnt)], ref=dict(ref, mag, extra)): float64 gradients, sum |kappa w|,
    sum E w and the contribution counts, per cell (see the module docstring)."""
    B, C, H, W = feats[0].shape
    V, D = len(feats), gvar.shape[2]
    taps = taps_of(orc, geo, gp, depth, H, W) if taps is None else taps
    g = np.asarray(gvar, np.float64)
    r = np.asarray(feats[0], np.float64)[:, :, None]
    with np.errstate(invalid="ignore", over="ignore"):
        warped = [S.sample_from_taps(feats[s + 1], *taps[s]) for s in range(V - 1)]
        A = [S.sample_from_taps(np.abs(feats[s + 1]), taps[s][0], np.abs(taps[s][1])) for s in range(V - 1)]
        m = (r + sum(warped)) / V
        M = np.abs(r) + sum(A)
        c = 2.0 / V
        src = []
        for s in range(V - 1):
            diff = warped[s] - m
            ref, mag, cnt = S.scatter_f64(g * c * diff, *taps[s], H, W)
            E = np.abs(g) * c * ((4.0 + (V + 5.0) / V) * M + 4.0 * np.abs(diff))
            _, extra, _ = S.scatter_f64(E, *taps[s], H, W)
            src.append(dict(ref=ref, mag=mag, extra=extra, cnt=cnt))
        t = g * c * (r - m)
        Er = np.abs(g) * c * (((V + 5.0) / V) * M + 3.0 * np.abs(r - m))
        refd = dict(ref=t.sum(2), mag=np.abs(t).sum(2), extra=Er.sum(2))
    return dict(taps=taps, src=src, ref=refd, V=V, D=D)


@functools.lru_cache(maxsize=None)
def _scene_reference(name):
    from oracle import oracle as orc
    sc = scene(name)
    return reference(orc, sc["feats"], sc["geo"], sc["gp"], sc["depth"], sc["gvar"])


def scene_reference(name):
    """The reference of a case of CASES, computed once per process and shared (read-only)."""
    return _scene_reference(name)


def bound_src(ref, s, init=None):
    d = ref["src"][s]
    n = d["cnt"][:, None].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        b = gamma(n + 1) * d["mag"] + (1.0 + gamma(n + 1)) * U * d["extra"]
        if init is not None:
            b = b + gamma(n) * np.abs(np.asarray(init, np.float64))
    return b


def bound_ref(ref, init=None):
    d = ref["ref"]
    nch = -(-ref["D"] // chunk(ref["V"] - 1))
    with np.errstate(invalid="ignore", over="ignore"):
        b = gamma(ref["D"] + nch) * d["mag"] + (1.0 + gamma(ref["D"] + nch)) * U * d["extra"]
        if init is not None:
            b = b + gamma(nch) * np.abs(np.asarray(init, np.float64))
    return b


def check(got, want, bound, cnt=None, init=None, what=""):
    """got (B,C,H,W) float32 from the kernel -> (messages, largest err / bound over the finite reached cells).  want / bound
    float64 per cell, cnt (B,H,W) contributions (None: every cell is reached), init what the buffer held before the call
    (None: zeros; `want` does not include it).  Per cell, no cell excused:
      * nothing contributes: the cell holds its initial bits;
      * the float64 reference is not finite: the kernel's value is not finite either, and in no other cell;
      * otherwise |got - (initial + want)| <= bound."""
    got = np.ascontiguousarray(got, np.float32)
    init = np.zeros(got.shape, np.float32) if init is None else np.ascontiguousarray(init, np.float32)
    want = np.asarray(want, np.float64)
    reached = np.ones(got.shape, bool) if cnt is None else np.broadcast_to((cnt > 0)[:, None], got.shape)
    msgs = []

    def first(mask, text):
        i = tuple(int(k) for k in np.argwhere(mask)[0])
        msgs.append("%s: %d cells %s; first (b,c,y,x) = %s: got %r, float64 %r, initial %r, bound %.3g%s"
                    % (what, int(mask.sum()), text, i, got[i], want[i], init[i], bound[i],
                       "" if cnt is None else " (n = %d)" % cnt[i[0], i[2], i[3]]))
    keep = ~reached & (got.view(np.uint32) != init.view(np.uint32))
    if keep.any():
        first(keep, "without a contribution lost their initial bits")
    nf_want, nf_got = reached & ~np.isfinite(want), ~np.isfinite(got)
    if (nf_got != nf_want).any():
        first(nf_got != nf_want, "non-finite on one side only")
    fin = reached & ~nf_want & ~nf_got
    if (fin & ~np.isfinite(bound)).any():
        first(fin & ~np.isfinite(bound), "with a finite reference and no finite bound (scene error)")
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(got.astype(np.float64) - (init.astype(np.float64) + want))
        bad = fin & ~(err <= bound)
    if bad.any():
        first(bad, "outside the bound")
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(fin & (bound > 0), err / np.maximum(bound, 1e-300), 0.0)
    return msgs, ratio


def old_criterion(got, other):
    """What held the backward before: max |got - other| <= 1e-4 max |other|.  -> (passes, ratio to the allowance)."""
    scale = float(np.abs(other).max())
    err = float(np.abs(np.asarray(got, np.float64) - other).max())
    return err <= OLD_RTOL * scale, err / (OLD_RTOL * scale)


def closed_form_collapse(sc, s, taps):
    """Collapse scenes: all voxels of view s share one tap, so its (up to) four cells hold w_q * sum over the voxels of
    g (2/V) (v_s - m) with v_s the per-channel sample -- no scatter needed.  -> {(y, x): (C,) float64 sums} for batch item 0."""
    off, wts = taps[s]
    V, (B, C, H, W) = sc["V"], sc["feats"][0].shape
    assert (off == off[:, :1, :1, :1, :1]).all()
    vals = []
    for v in range(V - 1):
        vals.append(S.sample_from_taps(sc["feats"][v + 1], *taps[v])[0])          # (C,D,H,W)
    m = (np.asarray(sc["feats"][0][0], np.float64)[:, None] + sum(vals)) / V
    tot = (np.asarray(sc["gvar"][0], np.float64) * (2.0 / V) * (vals[s] - m)).sum((1, 2, 3))
    out = {}
    for q in range(4):
        o = int(off[q, 0, 0, 0, 0])
        if o >= 0:
            out[(o // W, o % W)] = tot * float(wts[q, 0, 0, 0, 0])
    return out


# ---- census -----------------------------------------------------------------------------------------------------------------
COUNTERS = ("boxed", "register", "w_partial", "w_dropped", "w_view_none", "rows_lt8", "overhang_e", "overhang_s", "takes",
            "runs2", "runs_lastgive", "cut_chunks", "inactive_lanes")
BOXED_ONLY = ("boxed", "rows_lt8", "overhang_e", "overhang_s")      # no boxes beyond BOX_MAX_SRC source views


def census(n_src, taps, D, H, W):
    """What the kernel decides per wave and plane chunk, from the oracle's taps.  -> dict of COUNTERS (+ runs8, hot = the largest
    contribution count of a cell, and `boxed_vox` / `partial_vox` / `lost_east` (S,B,D,H,W) masks: the voxel is worked on by a
    boxed wave / is a border tap / keeps an east pair inside a run whose last plane gives its own away).
      patch 32 x 2 and 8 planes up to 4 sources, 64 x 1 and 2 planes beyond; a wave is boxed when in EVERY view the extent of the
      north-west cells of its full taps + 2 fits 64 x 8 (a view without a full tap needs no box); `take`: a full tap whose west
      lane (same patch row) has a full tap one cell to the west in the same row; a run: consecutive full taps of a lane within the
      chunk in the same cell (border and dropped taps in between do not end it)."""
    pw, ph = patch(n_src)
    dch = chunk(n_src)
    B = taps[0][0].shape[1]
    Sn = len(taps)
    Wp, Hp, dct = -(-W // 64) * 64, -(-H // 2) * 2, -(-D // dch)
    Dp, nwy, nwx = dct * dch, Hp // ph, Wp // pw
    full, part = np.zeros((Sn, B, Dp, Hp, Wp), bool), np.zeros((Sn, B, Dp, Hp, Wp), bool)
    x0, y0 = np.zeros((Sn, B, Dp, Hp, Wp), np.int64), np.zeros((Sn, B, Dp, Hp, Wp), np.int64)
    for s, (off, _) in enumerate(taps):
        v = off >= 0
        f = v.all(0)
        full[s, :, :D, :H, :W], part[s, :, :D, :H, :W] = f, v.any(0) & ~f
        x0[s, :, :D, :H, :W], y0[s, :, :D, :H, :W] = np.where(f, off[0] % W, 0), np.where(f, off[0] // W, 0)
    active = np.zeros((Dp, Hp, Wp), bool)
    active[:D, :H, :W] = True

    def waves(a):                                           # (..., Dp, Hp, Wp) -> (..., dct, nwy, nwx, dch, ph, pw)
        lead = a.shape[:-3]
        a = a.reshape(lead + (dct, dch, nwy, ph, nwx, pw))
        n = len(lead)
        return a.transpose(tuple(range(n)) + tuple(n + i for i in (0, 2, 4, 1, 3, 5)))

    def pixels(a):                                          # the inverse of waves(), cropped to (..., D, H, W)
        lead = a.shape[:-6]
        n = len(lead)
        a = a.transpose(tuple(range(n)) + tuple(n + i for i in (0, 3, 1, 4, 2, 5)))
        return a.reshape(lead + (Dp, Hp, Wp))[..., :D, :H, :W]
    fw, pwv, xw, yw, aw = waves(full), waves(part), waves(x0), waves(y0), waves(np.broadcast_to(active, full.shape))
    big = 1 << 30
    red = (-3, -2, -1)
    ax, bx = np.where(fw, xw, big).min(red), np.where(fw, xw, -big).max(red)
    ay, by = np.where(fw, yw, big).min(red), np.where(fw, yw, -big).max(red)
    none = bx < ax                                          # (S,B,dct,nwy,nwx)
    fits = (none | ((bx - ax + 2 <= BOX_W) & (by - ay + 2 <= BOX_H))).all(0)
    boxed_w = fits & (n_src <= BOX_MAX_SRC)                  # (B,dct,nwy,nwx)
    any_full, any_live = fw.any(red).any(0), (fw | pwv).any(red).any(0)
    any_active = aw.any(red)[0]
    dropped = aw & ~fw & ~pwv
    out = dict(boxed=int((boxed_w & any_full).sum()), register=int((~boxed_w & any_live).sum()),
               w_partial=int(pwv.any(red).any(0).sum()), w_dropped=int((dropped.any(red).any(0) & any_live).sum()),
               w_view_none=int((none & any_active[None] & any_live[None]).any(0).sum()))
    rows = np.minimum(by - ay + 2, BOX_H)
    bview = boxed_w[None] & ~none
    out["rows_lt8"] = int((bview & (rows < BOX_H)).sum())
    out["overhang_e"] = int((bview & (ax + BOX_W > W)).sum())
    out["overhang_s"] = int((bview & (ay + BOX_H > H)).sum())
    # hand-overs
    west_f = np.zeros_like(fw)
    west_f[..., 1:] = fw[..., :-1]
    west_x, west_y = np.roll(xw, 1, -1), np.roll(yw, 1, -1)
    take = fw & west_f & (west_y == yw) & (west_x + 1 == xw)
    give = np.zeros_like(take)
    give[..., :-1] = take[..., 1:]
    regw = (~boxed_w)[None, ..., None, None, None]
    out["takes"] = int((take & regw).sum())
    # runs, plane by plane
    shp = fw.shape[:-3] + fw.shape[-2:]
    rkey, rlen, rid = np.full(shp, -1, np.int64), np.zeros(shp, np.int64), np.zeros(shp, np.int64)
    kept, lastge, kbl = np.zeros(shp, bool), np.zeros(shp, bool), np.zeros(shp, bool)
    flagged = np.zeros(shp + (dch + 2,), bool)
    runid = np.zeros(fw.shape, np.int64)
    reg_lane = np.broadcast_to((~boxed_w)[None, ..., None, None], shp)
    counts = dict(runs2=0, runs8=0, runs_lastgive=0)

    def close(mask):
        done = mask & (rlen >= 2) & reg_lane
        counts["runs2"] += int(done.sum())
        counts["runs8"] += int((done & (rlen >= 8)).sum())
        lg = done & lastge & kbl
        counts["runs_lastgive"] += int(lg.sum())
        idx = np.nonzero(lg)
        flagged[idx + (rid[idx],)] = True
    for k in range(dch):
        f, ge = fw[..., k, :, :], give[..., k, :, :]
        key = yw[..., k, :, :] * W + xw[..., k, :, :]
        new = f & (key != rkey)
        close(new & (rkey >= 0))
        rkey[new], rlen[new], kept[new] = key[new], 0, False
        rid[new] += 1
        runid[..., k, :, :] = rid
        rlen[f] += 1
        kbl[f] = kept[f]
        lastge[f] = ge[f]
        kept[f] |= ~ge[f]
    close(rkey >= 0)
    out.update(counts)
    lost = np.zeros(fw.shape, bool)
    for k in range(dch):
        lost[..., k, :, :] = fw[..., k, :, :] & ~give[..., k, :, :] & np.take_along_axis(flagged, runid[..., k, :, :][..., None], -1)[..., 0]
    out["cut_chunks"] = int(any_active[:, -1].sum()) if D % dch else 0
    out["inactive_lanes"] = B * (Hp * Wp - H * W)
    out["hot"] = max(_hottest(off, H * W) for off, _ in taps)
    out["boxed_vox"] = pixels(np.broadcast_to(boxed_w[None, ..., None, None, None], fw.shape))
    out["partial_vox"] = part[:, :, :D, :H, :W]
    out["lost_east"] = pixels(lost)
    return out


def _hottest(off, HW):
    best = 0
    for b in range(off.shape[1]):
        o = off[:, b].ravel()
        o = o[o >= 0]
        if o.size:
            best = max(best, int(np.bincount(o, minlength=HW).max()))
    return best


def has(cen, prop):
    """Does a census have the property a case names?"""
    if prop == "no_boxed":
        return cen["boxed"] == 0
    if prop == "few_boxed":
        return 8 * cen["boxed"] <= cen["register"]
    if prop == "hot":                                       # a cell that thousands of voxels add to
        return cen["hot"] >= 1000
    if prop == "nonfinite":                                 # asserted on the reference, not on the census
        return True
    return cen[prop] > 0


def cell_schemes(cen, taps, s, H, W):
    """Per cell (B,H,W) of view s: 2 where a border tap contributes, else 1 where a register wave does, else 0 (boxed only)."""
    off = taps[s][0]
    B = off.shape[1]
    out = np.zeros((B, H * W), np.int64)
    for b in range(B):
        for q in range(4):
            o = off[q, b].ravel()
            ok = o >= 0
            for level, mask in ((1, ~cen["boxed_vox"][s, b].ravel()), (2, cen["partial_vox"][s, b].ravel())):
                hit = np.bincount(o[ok & mask], minlength=H * W) > 0
                out[b] = np.where(hit, np.maximum(out[b], level), out[b])
    return out.reshape(B, H, W)


# ---- a float32 model of the kernel's arithmetic (CPU tests: does the bound hold for float32, does check() see planted errors) --
def model32(feats, gvar, taps, init=None, drop_below=None, skip_border=False, skip_last_ref_plane=False, lost_east=None,
            scatter_taps=None):
    """The kernel's products and float32 sums in plane order: warped = a0 w0, then fused multiply-adds; sum and the correctly
    rounded division; g RN(2/V) (warped - m) w_q; per plane and corner the contributions of one cell are summed (as a box does)
    and added to the float32 cell.  -> ([grad_src per view], grad_ref), float32.
    Planted errors: drop_below (contributions with a smaller weight are not scattered), skip_border (border taps are not
    scattered), skip_last_ref_plane (plane D - 1 is left out of grad_ref), lost_east (S,B,D,H,W): the east corners of these
    voxels are not scattered; scatter_taps: the taps the scatter uses (default: `taps`)."""
    f32, f64 = np.float32, np.float64
    B, C, H, W = feats[0].shape
    V, D, HW = len(feats), gvar.shape[2], H * W
    fV = f32(V)
    two_over_v = f32(2.0) / fV
    scatter_taps = taps if scatter_taps is None else scatter_taps
    gsrc = [np.zeros((B, C, HW), f32) if init is None else np.array(init[s + 1], f32).reshape(B, C, HW) for s in range(V - 1)]
    gref = np.zeros((B, C, H, W), f32) if init is None else np.array(init[0], f32)
    cidx = (np.arange(C) * HW)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            r = feats[0][b][:, None]                                        # (C,1,H,W)
            wv = []
            total = np.broadcast_to(r, (C, D, H, W)).astype(f32)
            for s in range(V - 1):
                off, wts = taps[s]
                f = feats[s + 1][b].reshape(C, HW)
                t = None
                for q in range(4):
                    o = off[q, b]
                    a = np.where(o >= 0, f[:, np.maximum(o, 0)], f32(0))     # (C,D,H,W)
                    t = a * wts[q, b] if t is None else (a.astype(f64) * wts[q, b] + t).astype(f32)
                wv.append(t)
                total = total + t
            m = total / fV
            g = np.asarray(gvar[b], f32) * two_over_v
            for d in range(D):
                if not (skip_last_ref_plane and d == D - 1):
                    gref[b] = (g[:, d].astype(f64) * (r[:, 0] - m[:, d]) + gref[b]).astype(f32)
            for s in range(V - 1):
                off, wts = scatter_taps[s]
                gw = g * (wv[s] - m)
                border = (off[:, b] >= 0).any(0) & ~(off[:, b] >= 0).all(0)
                for d in range(D):
                    for q in range(4):
                        o = off[q, b, d].ravel()
                        ok = o >= 0
                        if drop_below is not None:
                            ok = ok & ~(wts[q, b, d].ravel() < drop_below)
                        if skip_border:
                            ok = ok & ~border[d].ravel()
                        if lost_east is not None and q in (1, 3):
                            ok = ok & ~lost_east[s, b, d].ravel()
                        if not ok.any():
                            continue
                        c = (gw[:, d] * wts[q, b, d]).reshape(C, HW)[:, ok]
                        idx = (o[ok][None] + cidx).ravel()
                        add = np.bincount(idx, weights=c.ravel().astype(f64), minlength=C * HW).astype(f32).reshape(C, HW)
                        hit = np.bincount(o[ok], minlength=HW) > 0
                        gsrc[s][b][:, hit] = gsrc[s][b][:, hit] + add[:, hit]
    return [x.reshape(B, C, H, W) for x in gsrc], gref
