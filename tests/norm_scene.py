"""Cases, scenes, float64 references, per-element error bounds, float32 models and a checker for the normalisation and GRU element-wise
entries: smvs_groupnorm1_fwd / _bwd / _pair_fwd / _pair_bwd / _fwd_blend / _pair_fwd_mul and the five smvs_gru_* of csrc/groupnorm.hip,
smvs_batchnorm_train_fwd / _bwd of csrc/batchnorm.hip.  numpy only.  Shared by tests/test_norm_cpu.py (which asserts, without a GPU, what
the GPU tests assume about the cases, the references and the bounds) and tests/test_norm_gpu.py.

The branch rules of the kernels are local to a workgroup, so the census below mirrors them in a few lines (the constants are named once,
here) instead of asking the library: which chunks and row segments take the float4 path, which folds stride a second time.

Bounds.  u = 2^-24.  Every bound is a sum of the kernel's own roundings, each at the magnitude where it happens, times SLACK = 1 + 2^-10
for the products of two roundings, plus TINY = 4 * 2^-126 for a result in the subnormal range.  Nothing is compared by a max-norm.

GroupNorm forward (gn_ref_fwd).  The statistics are float64 sums: a thread adds 16 values, the wave and block folds 9, the second fold
at most 2 + 9 -- D = 40 float64 additions deep with the divisions -- so
    |mean - m|  <= u |m| + D 2^-53 mean|x|                       (one float32 rounding of the float64 mean)
    |var_k - var| <= 3 D 2^-53 q/n,  q/n = mean x^2               (q/n - m^2 cancels: (q/n) / (var + eps) is the condition number)
    |rstd - r|  <= r (2u + 0.5 * 3 D 2^-53 (q/n) / (var + eps))
(tighter than a bound with the number of elements in it: the depth of the sum counts, not its length).  The apply pass forms
g = fl(gamma rstd), o = fl(beta - fl(mean g)), pre = fl(x g + o) (one fused multiply-add): four roundings,
    |pre_k - pre| <= u (|(x - mean) g| + 2 |mean g| + |beta| + |pre|) + |gamma| (rstd E_mean + |x - mean| E_rstd)
the 2 |mean g| being the price of the uncentred form.  Activations: E_y = L E_pre + allowance, L the largest derivative on
[|pre| - E_pre, |pre|] (at most 1/4 / 1), allowance 8u y (sigmoid: exp <= 3 ulp, the add, the divide, OpenCL's single-precision limits
which the device library is specified to) and 10u |y| (tanh <= 5 ulp): the one number here that is not counted from the code.

GroupNorm backward (gn_ref_bwd): a function of what the kernel is handed -- dy, x, gamma and the forward KERNEL's y and mean_rstd --
in float64.  dz = dy act'(y): E_dz = 0 / 3u |dz| / u |dy| y^2 + 2u |dz|;  xhat = fl(fl(x - mean) rstd): 2u |xhat|;  a row sum on the
float4 path adds four float32 values (two roundings each) before the float64 sum, products rounded first:
    E_S1 = sum (E_dz + 2u |dz|),   E_S2 = sum |xhat| (E_dz + 5u |dz|)
    E_a = sum_c |gamma_c| E_S1 / N + u |a|,  E_q likewise;   dgamma, dbeta: the E_S summed + u |result|
    E_dx = rstd (|g| E_dz + 2u |dz g| + u |a| + E_a + 3u |xhat q| + |xhat| E_q) + 2u |dx|

BatchNorm (bn_ref_fwd / bn_ref_bwd), pivot p = x[0, c, 0], d = x - p, a thread's float32 sums have at most 64 terms:
    |saved[2c] + p - m| <= 65u mean|d| + u |m - p|;   E_var = 67u mean d^2 + 2 |m - p| 65u mean|d|;   E_rstd = r (2u + E_var / 2 (var + eps))
    E_pre = |scale| (u |d| + u |x - m| + E_ms) + |gamma| |x - m| E_rstd + u |scale (x - m)| + u |pre|,  ReLU: the same bound
    backward: E_xc = u |d| + u |xc|, E_xh = rstd E_xc + u |xhat|;  E_T1 = 64u sum |dz|,  E_T2 = sum |dz| E_xh + 64u sum |dz xhat|
    E_dx = |scale| (u (|dz| + |t1|) + E_t1 + E_xh |t2| + |xhat| E_t2 + u |xhat t2| + u |dz - t1 - xhat t2|) + 2u |dx|
The running statistics add the momentum blend's four roundings.

The GRU entries and the fused epilogues are built without contraction: a numpy float32 expression gives their bits; bwd_acc's single
fused multiply-add is held to u |ref|.
"""
import functools
import math
from collections import namedtuple

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
TINY = 4 * 2.0 ** -126
SLACK = 1 + 2.0 ** -10
D64 = 40                                   # depth, in float64 additions, of a GroupNorm statistic (see above)
GN_ELEMS, GN_THREADS = 4096, 256           # csrc/groupnorm.hip
BN_BLOCK, BN_CHUNK, BN_STEP = 256, 16384, 4096      # csrc/batchnorm.hip: BN_STEP = BN_BLOCK * 4 * BN_UNROLL elements per unrolled step
GE_THREADS = 256
ACT_ALLOW = {1: 8.0, 2: 10.0}              # evaluation allowance of sigmoid / tanh in u |y|
BN_WORKSPACE_ZERO = 2                      # SMVS_BN_WORKSPACE_ZERO


def cdiv(a, b):
    return -(-a // b)


# ---- cases ------------------------------------------------------------------------------------------------------------------------
# B: the entry's B (the pair form has 2B internal samples of C channels);  xbs / dxbs: batch strides in floats (None: contiguous);
# sliced: x is the second half of a (B, 2C, HW) tensor and dx the second half of another;  off: base offset in floats of every operand
# from a 16-byte boundary;  acts: the activations the case runs with
GnCase = namedtuple("GnCase", "name B C HW xbs dxbs sliced off acts pair")


def _gn(B, C, HW, xbs=None, dxbs=None, sliced=False, off=0, acts=(0,), pair=False, tag=""):
    name = "%s%dx%dx%d%s" % ("pair-" if pair else "", B, C, HW, tag)
    return GnCase(name, B, C, HW, xbs, dxbs, sliced, off, tuple(acts), pair)


GN_CASES = [
    _gn(1, 1, 1),
    _gn(1, 2, 3, acts=(0, 1, 2)),
    _gn(2, 4, 1024, acts=(0, 1, 2)),
    _gn(1, 4, 1025),
    _gn(1, 3, 1366),
    _gn(1, 2, 4100),
    _gn(1, 2, 4098, acts=(0, 1, 2)),
    _gn(3, 8, 100, sliced=True, acts=(0, 1, 2), tag="-sliced"),
    _gn(2, 4, 64, xbs=4 * 64 + 1, dxbs=4 * 64 + 3, tag="-strides"),
    _gn(1, 300, 5),
    _gn(2, 130, 4100),
    _gn(1, 4, 262400),
    _gn(1, 4, 1024, off=1, tag="-off1"),
    _gn(1, 4, 1024, off=2, tag="-off2"),
    _gn(1, 4, 1024, off=3, tag="-off3"),
]
PAIR_CASES = [
    _gn(1, 1, 2, pair=True, acts=(0, 1)),
    _gn(2, 4, 1024, pair=True, acts=(0, 1)),
    _gn(2, 3, 1366, pair=True, acts=(0, 1)),
    _gn(1, 8, 4100, pair=True, acts=(0, 1)),
    _gn(3, 5, 7, pair=True, acts=(0, 1, 2)),
]
GN_BY_NAME = {c.name: c for c in GN_CASES + PAIR_CASES}
assert len(GN_BY_NAME) == len(GN_CASES) + len(PAIR_CASES)

BnCase = namedtuple("BnCase", "name B C N off")
BN_CASES = [BnCase("%dx%dx%d%s" % (B, C, N, "-off%d" % off if off else ""), B, C, N, off) for B, C, N, off in
            [(2, 1, 1, 0), (1, 2, 3, 0), (1, 3, 4, 0), (3, 5, 4100, 0), (1, 2, 16384, 0), (3, 2, 16388, 0), (2, 3, 16385, 0),
             (1, 4, 4096, 1), (1, 4, 4096, 2), (1, 4, 4096, 3)]]
BN_BY_NAME = {c.name: c for c in BN_CASES}

BLEND_N = (1, 3, 4, 5, 1023, 1024, 1027, 2051)
MULCAT = ((1, 0, 1, 1), (2, 3, 2, 5), (1, 1, 1, 255), (1, 1, 1, 256), (2, 1, 1, 257))          # (B, Cx, Ch, HW)

GN_KINDS = ("exact0", "exact96", "real", "offset", "const", "saturating")
BN_KINDS = ("exact0", "exact96", "real", "offset", "const", "saturating", "zero-gamma", "pivot-outlier")


def internal_B(c):
    return 2 * c.B if c.pair else c.B


GnLayout = namedtuple("GnLayout", "x xbs y dy dx dxbs")      # float offsets from a 16-byte boundary; y and dy are (B, C, HW) contiguous


def gn_layout(c):
    n = c.C * c.HW
    if c.sliced:
        return GnLayout(c.off + n, 2 * n, c.off, c.off, c.off + n, 2 * n)
    return GnLayout(c.off, c.xbs or n, c.off, c.off, c.off, c.dxbs or n)


def gn_segments(c):
    return [(i0, min(c.HW, i0 + GN_ELEMS)) for i0 in range(0, c.HW, GN_ELEMS)]


def gn_row_vec4(c, b, ch, seg, operands, extra=0):
    """the float4 rule of the apply / rows / dx kernels for row (b, ch), segment (i0, i1): every named operand's row pointer on a
    16-byte boundary (extra: the offsets of the epilogue operands, or-ed in the same way) and a segment length that is a multiple of 4"""
    L = gn_layout(c)
    i0, i1 = seg
    ptrs = {"x": L.x + b * L.xbs + ch * c.HW, "y": L.y + (b * c.C + ch) * c.HW, "dy": L.dy + (b * c.C + ch) * c.HW,
            "dx": L.dx + b * L.dxbs + ch * c.HW}
    return all(ptrs[o] % 4 == 0 for o in operands) and extra % 4 == 0 and (i1 - i0) % 4 == 0 and i0 % 4 == 0


def gn_stats_chunks(c, b):
    """[(i0, i1, float4?)] of sample b in the statistics pass: chunks of the flat C*HW sample"""
    L = gn_layout(c)
    n = c.C * c.HW
    al = (L.x + b * L.xbs) % 4 == 0
    return [(i0, min(n, i0 + GN_ELEMS), al and (min(n, i0 + GN_ELEMS) - i0) % 4 == 0) for i0 in range(0, n, GN_ELEMS)]


def gn_classes(c):
    """The classes case c reaches, computed from its shape with the kernels' rules."""
    t = set()
    Bi, C, HW = internal_B(c), c.C, c.HW
    n, nseg = C * HW, cdiv(HW, GN_ELEMS)
    t.add("pair" if c.pair else "single")
    for b in range(Bi):
        ch = gn_stats_chunks(c, b)
        kinds = {v for _, _, v in ch}
        t.update("stats-float4" if v else "stats-scalar" for v in kinds)
        if len(kinds) == 2:
            t.add("stats-float4-and-scalar-in-one-sample")
        if any(i0 // HW != (i1 - 1) // HW for i0, i1, _ in ch):
            t.add("stats-chunk-crosses-a-channel")
        if ch[-1][1] - ch[-1][0] < GN_ELEMS:
            t.add("stats-short-last-chunk")
        if len(ch) > GN_THREADS:
            t.add("stats-fold-strides-twice")
    for which, ops in (("apply", ("x", "y")), ("dx", ("x", "dy", "y", "dx"))):
        per_sample = []
        for b in range(Bi):
            rows = [[gn_row_vec4(c, b, k, s, ops) for s in gn_segments(c)] for k in range(C)]
            flat = {v for r in rows for v in r}
            per_sample.append(flat)
            t.update(which + ("-float4" if v else "-scalar") for v in flat)
            if any(len(r) > 1 and r[0] and not r[1] for r in rows):
                t.add(which + "-row-float4-then-scalar")
            if any(rows[k] != rows[k + 1] for k in range(C - 1)):
                t.add(which + "-rows-differ")
        if len(set().union(*per_sample)) == 2:
            t.add(which + "-both-paths-in-one-call")
        if Bi > 1 and any(per_sample[i] != per_sample[0] for i in range(1, Bi)):
            t.add(which + "-samples-differ")
    t.add("nseg=%d" % nseg)
    if nseg > 1:
        t.add("dx-fold-divides-by-nseg")
    if C * nseg > GN_THREADS:
        t.add("dx-fold-strides-twice")
    if C > GN_THREADS:
        t.add("dgamma-loop-strides-twice")
    L = gn_layout(c)
    if L.xbs % 4 and Bi > 1:
        t.add("x-batch-stride-not-a-multiple-of-4")
    if C > 1 and len({(L.x + k * HW) % 4 == 0 for k in range(C)}) == 2:
        t.add("row-pointers-aligned-and-not")
    if L.dxbs > n:
        t.add("dx-batch-stride-beyond-a-sample")
    if c.sliced:
        t.add("sliced")
    if c.off:
        t.add("base-offset-%d" % c.off)
    if n == 1:
        t.add("one-element")
    if Bi > 1:
        t.add("B>1")
    if c.pair:
        t.add("pair-B=%d" % c.B)
        t.add("pair-odd-count" if n % 2 else "pair-even-count")
    for a in c.acts:
        t.add("act=%d" % a)
    return t


GN_REQUIRED = {"single", "pair", "stats-float4", "stats-scalar", "stats-float4-and-scalar-in-one-sample", "stats-chunk-crosses-a-channel",
               "stats-short-last-chunk", "stats-fold-strides-twice", "apply-float4", "apply-scalar", "apply-row-float4-then-scalar",
               "apply-rows-differ", "apply-both-paths-in-one-call", "apply-samples-differ", "dx-float4", "dx-scalar",
               "dx-row-float4-then-scalar", "dx-both-paths-in-one-call", "dx-samples-differ", "nseg=1", "nseg=2", "nseg=65",
               "dx-fold-divides-by-nseg", "dx-fold-strides-twice", "dgamma-loop-strides-twice", "x-batch-stride-not-a-multiple-of-4",
               "dx-batch-stride-beyond-a-sample", "sliced", "row-pointers-aligned-and-not", "base-offset-1", "base-offset-2", "base-offset-3", "one-element", "B>1",
               "pair-B=1", "pair-B=2", "pair-B=3", "pair-odd-count", "pair-even-count", "act=0", "act=1", "act=2"}
# what each case was chosen for (asserted in tests/test_norm_cpu.py)
GN_INTENDED = {
    "1x1x1": {"one-element", "stats-scalar", "apply-scalar"},
    "1x2x3": {"stats-scalar", "apply-scalar", "act=1", "act=2"},
    "2x4x1024": {"stats-float4", "apply-float4", "dx-float4", "B>1", "act=1", "act=2"},
    "1x4x1025": {"stats-float4", "stats-short-last-chunk", "stats-chunk-crosses-a-channel", "apply-scalar"},
    "1x3x1366": {"stats-short-last-chunk", "stats-float4-and-scalar-in-one-sample", "row-pointers-aligned-and-not"},
    "1x2x4100": {"nseg=2", "stats-chunk-crosses-a-channel", "apply-float4", "dx-fold-divides-by-nseg"},
    "1x2x4098": {"apply-row-float4-then-scalar", "dx-row-float4-then-scalar", "apply-both-paths-in-one-call", "act=1", "act=2"},
    "3x8x100-sliced": {"sliced", "dx-batch-stride-beyond-a-sample", "act=1", "act=2"},
    "2x4x64-strides": {"x-batch-stride-not-a-multiple-of-4", "dx-batch-stride-beyond-a-sample", "apply-samples-differ", "dx-samples-differ"},
    "1x300x5": {"dgamma-loop-strides-twice", "dx-fold-strides-twice"},
    "2x130x4100": {"dx-fold-strides-twice", "dx-fold-divides-by-nseg", "nseg=2"},
    "1x4x262400": {"stats-fold-strides-twice", "nseg=65"},
    "1x4x1024-off1": {"base-offset-1", "stats-scalar", "apply-scalar", "dx-scalar"},
    "1x4x1024-off2": {"base-offset-2", "apply-scalar"},
    "1x4x1024-off3": {"base-offset-3", "apply-scalar"},
    "pair-1x1x2": {"pair-B=1", "pair-even-count"},
    "pair-2x4x1024": {"pair-B=2", "apply-float4"},
    "pair-2x3x1366": {"pair-B=2", "row-pointers-aligned-and-not", "x-batch-stride-not-a-multiple-of-4"},
    "pair-1x8x4100": {"pair-B=1", "nseg=2", "dx-fold-divides-by-nseg"},
    "pair-3x5x7": {"pair-B=3", "pair-odd-count", "act=2"},
}


def bn_vec4(c):
    return c.N % 4 == 0 and c.off == 0


def bn_classes(c):
    t = set()
    nchunk = cdiv(c.N, BN_CHUNK)
    t.add("nchunk=%d" % nchunk)
    if nchunk > 1 and c.B > 1:
        t.add("block-index-splits-into-b-and-chunk")
    t.add("float4" if bn_vec4(c) else "scalar")
    if c.off:
        t.add("scalar-by-base-offset-%d" % c.off)
    if c.N % 4:
        t.add("scalar-by-length")
    last = c.N - (nchunk - 1) * BN_CHUNK
    if bn_vec4(c) and last % BN_STEP:
        t.add("float4-partial-last-step")
    if bn_vec4(c) and any(l > BN_STEP and l % BN_STEP == 0 for l in (min(BN_CHUNK, c.N), last)):
        t.add("float4-whole-steps")
    if c.B * c.N == 2:
        t.add("two-elements")
    if c.N < 4:
        t.add("N<4")
    if c.B > 1:
        t.add("B>1")
    if last < BN_CHUNK and nchunk > 1:
        t.add("short-last-chunk")
    if (c.B * c.N) % 2:
        t.add("odd-count")
    return t


BN_REQUIRED = {"nchunk=1", "nchunk=2", "block-index-splits-into-b-and-chunk", "float4", "scalar", "scalar-by-base-offset-1",
               "scalar-by-base-offset-2", "scalar-by-base-offset-3", "scalar-by-length", "float4-partial-last-step", "float4-whole-steps",
               "two-elements", "N<4", "B>1", "short-last-chunk", "odd-count"}
BN_INTENDED = {
    "2x1x1": {"two-elements", "scalar"}, "1x2x3": {"N<4", "odd-count", "scalar-by-length"}, "1x3x4": {"float4", "float4-partial-last-step"},
    "3x5x4100": {"float4-partial-last-step", "B>1", "nchunk=1"}, "1x2x16384": {"float4-whole-steps", "nchunk=1"},
    "3x2x16388": {"nchunk=2", "block-index-splits-into-b-and-chunk", "float4", "short-last-chunk"},
    "2x3x16385": {"nchunk=2", "scalar-by-length", "block-index-splits-into-b-and-chunk"},
    "1x4x4096-off1": {"scalar-by-base-offset-1"}, "1x4x4096-off2": {"scalar-by-base-offset-2"}, "1x4x4096-off3": {"scalar-by-base-offset-3"},
}


def blend_classes(n):
    n4 = n // 4
    t = {"blocks=%d" % max(1, cdiv(n4, GE_THREADS))}
    t.add("tail-only" if n4 == 0 else "tail=%d" % (n % 4))
    if n4 and n4 % GE_THREADS == 0:
        t.add("full-last-block")
    if cdiv(n4, GE_THREADS) > 1 and n % 4:
        t.add("tail-beside-a-second-block")
    return t


BLEND_REQUIRED = {"tail-only", "tail=0", "tail=1", "tail=3", "blocks=1", "blocks=2", "full-last-block", "tail-beside-a-second-block"}


def mulcat_classes(m):
    B, Cx, Ch, HW = m
    nx, nh = Cx * HW, Ch * HW
    t = {"blocks=%d" % cdiv(nx + nh, GE_THREADS)}
    if Cx == 0:
        t.add("Cx=0")
    if nx % GE_THREADS:
        t.add("split-inside-a-block")
    if nx and nx % GE_THREADS == 0:
        t.add("split-on-a-block-edge")
    if (nx + nh) % GE_THREADS == 0:
        t.add("full-last-block")
    if B > 1:
        t.add("B>1")
    return t


MULCAT_REQUIRED = {"Cx=0", "split-inside-a-block", "split-on-a-block-edge", "full-last-block", "blocks=1", "blocks=2", "blocks=3", "B>1"}


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def _rng(name, kind):
    return np.random.RandomState((sum(ord(ch) * (i + 1) for i, ch in enumerate(name + "/" + kind)) * 7919 + 13) % (2 ** 31))


def _balanced(shape_lead, count, m, rng):
    """(lead..., count) of m + 1 and m - 1 in equal numbers along the last axis, shuffled"""
    base = np.where(np.arange(count) % 2 == 0, 1.0, -1.0)
    out = np.empty(tuple(shape_lead) + (count,), F32)
    for idx in np.ndindex(*shape_lead):
        out[idx] = m + rng.permutation(base)
    return out


GnScene = namedtuple("GnScene", "x gamma beta gamma2 beta2 eps dy u h hm")
# x, dy, u, h: (Bi, C, HW) float32 (Bi internal samples);  hm: (B, C, HW), the mul epilogue's state;  gamma2 / beta2: None (single form)


def gn_scene_applies(c, kind):
    return not (kind.startswith("exact") and (c.C * c.HW) % 2)


@functools.lru_cache(maxsize=None)
def gn_scene(c, kind):
    """Shared: do not modify."""
    assert gn_scene_applies(c, kind)
    rng = _rng(c.name, kind)
    Bi, C, HW = internal_B(c), c.C, c.HW
    shape = (Bi, C, HW)
    eps = 1e-5
    if kind.startswith("exact"):
        m = float(kind[5:])
        x = _balanced((Bi,), C * HW, m, rng).reshape(shape)
        gamma = (2.0 ** rng.randint(-1, 3, C)) * rng.choice([-1.0, 1.0], C)
        beta = rng.randint(-3, 4, C).astype(F64)
        gamma2, beta2 = -4.0 * gamma, beta + 5.0
        dy = rng.randint(-3, 4, shape).astype(F32)
        eps = 3.0
    else:
        scales = np.logspace(-1, 1, C)[rng.permutation(C)][None, :, None]
        x = rng.randn(*shape) * scales + 0.7 * scales
        gamma = rng.randn(C) * 0.5 + 1.0
        beta = rng.randn(C) * 0.3
        gamma2, beta2 = -(np.abs(gamma) + 3.0), beta + 5.0
        dy = rng.randn(*shape)
        if kind == "offset":
            x = 1000.0 + rng.randn(*shape)
        elif kind == "const":
            x[0] = 1.5
        elif kind == "saturating":
            gamma = rng.choice([-1.0, 1.0], C) * 100.0 / 3.0
            gamma2 = -2.0 * gamma
        else:
            assert kind == "real"
    u = 1.0 / (1.0 + np.exp(-2.0 * rng.randn(*shape)))
    h = rng.randn(*shape)
    hm = rng.randn(c.B, C, HW)
    f = lambda a: np.ascontiguousarray(a, dtype=F32)
    return GnScene(f(x), f(gamma), f(beta), f(gamma2) if c.pair else None, f(beta2) if c.pair else None, float(F32(eps)), f(dy), f(u), f(h), f(hm))


def per_sample(sc, first, second, swap=False):
    """(Bi, C): the parameter set of every internal sample -- odd samples of the pair form take the second"""
    Bi = sc.x.shape[0]
    if second is None:
        return np.broadcast_to(first, (Bi,) + first.shape)
    odd = (np.arange(Bi) % 2 == 1) != swap
    return np.where(odd[:, None], second[None], first[None])


BnScene = namedtuple("BnScene", "x gamma beta eps momentum rm rv dy")


def bn_scene_applies(c, kind):
    if kind.startswith("exact"):
        return (c.B * c.N) % 2 == 0
    return True


@functools.lru_cache(maxsize=None)
def bn_scene(c, kind):
    assert bn_scene_applies(c, kind)
    rng = _rng("bn" + c.name, kind)
    B, C, N = c.B, c.C, c.N
    shape = (B, C, N)
    eps, mom = 1e-5, 0.1
    rm, rv = rng.randn(C), 0.5 + rng.rand(C)
    if kind.startswith("exact"):
        m = float(kind[5:])
        x = _balanced((C,), B * N, m, rng).reshape(C, B, N).transpose(1, 0, 2)
        gamma = (2.0 ** rng.randint(-1, 3, C)) * rng.choice([-1.0, 1.0], C)
        beta = rng.randint(-3, 4, C).astype(F64)
        dy = rng.randint(-3, 4, shape).astype(F32)
        eps, mom = 3.0, 0.25
        rm, rv = 4.0 * rng.randint(-3, 4, C), 4.0 * rng.randint(1, 4, C)
    else:
        scales = np.logspace(-1, 1, C)[rng.permutation(C)][None, :, None]
        x = rng.randn(*shape) * scales + 0.7 * scales
        gamma = rng.randn(C) * 0.5 + 1.0
        beta = rng.randn(C) * 0.3
        dy = rng.randn(*shape)
        if kind == "offset":
            x = 1000.0 * scales + rng.randn(*shape) * scales
        elif kind == "const":
            x[:, 0] = 1.5
        elif kind == "saturating":
            gamma = rng.choice([-1.0, 1.0], C) * 100.0 / 3.0
        elif kind == "zero-gamma":                           # the ReLU mask decided by > 0 on an exact zero, and by beta alone
            gamma[0], beta[0] = 0.0, 0.0
            if C > 1:
                gamma[1], beta[1] = 0.0, 0.5
        elif kind == "pivot-outlier":                        # the pivot 8 standard deviations from the channel mean
            x[0, C - 1, 0] = 0.7 * scales[0, C - 1, 0] + 8.0 * scales[0, C - 1, 0]
        else:
            assert kind == "real"
    f = lambda a: np.ascontiguousarray(a, dtype=F32)
    return BnScene(f(x), f(gamma), f(beta), float(F32(eps)), float(F32(mom)), f(rm), f(rv), f(dy))


@functools.lru_cache(maxsize=None)
def blend_scene(n):
    rng = _rng("blend%d" % n, "real")
    u = 1.0 / (1.0 + np.exp(-2.0 * rng.randn(n)))
    return tuple(np.ascontiguousarray(a, dtype=F32) for a in (rng.randn(n), u, rng.randn(n), rng.randn(n)))       # dy, u, h, y


@functools.lru_cache(maxsize=None)
def mulcat_scene(m):
    B, Cx, Ch, HW = m
    rng = _rng("mulcat%d-%d-%d-%d" % m, "real")
    f = lambda *s: np.ascontiguousarray(rng.randn(*s), dtype=F32)
    return f(B, Cx, HW), f(B, Ch, HW), f(B, Ch, HW), f(B, Cx + Ch, HW), f(B, Ch, HW)                               # x, r, h, dcat, dh_acc


# ---- checker ----------------------------------------------------------------------------------------------------------------------
Report = namedtuple("Report", "ok ratio message")


def assert_complete(ref, bound, shape, what=""):
    """the reference decides every element: it has the output's shape, it and its bound are finite, the bound is not negative"""
    ref, bound = np.asarray(ref), np.asarray(bound)
    assert ref.shape == tuple(shape) == bound.shape, (what, ref.shape, bound.shape, shape)
    assert np.isfinite(ref).all() and np.isfinite(bound).all() and (bound >= 0).all(), what


def check(got, ref, bound, what):
    """got against ref within bound, element by element, no element left out: a non-finite value where the reference is finite (and
    the reverse) counts as an infinite error, any difference under a zero bound too.  -> Report(ok, worst err / bound, message)"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    bound = np.broadcast_to(np.asarray(bound, F64), ref.shape)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        fin = np.isfinite(ref)
        err = np.abs(got - ref)
        err = np.where(fin, np.where(np.isfinite(got), err, np.inf), np.where(np.isnan(got) == np.isnan(ref), 0.0, np.inf))
        err = np.where(~fin & (got == ref), 0.0, err)
        ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 0.0))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    if ratio.size == 0:
        return Report(True, 0.0, "")
    i = int(np.argmax(ratio))
    worst = float(ratio.flat[i])
    if worst <= 1.0:
        return Report(True, worst, "")
    bad = np.flatnonzero(ratio.reshape(-1) > 1.0)
    k = int(bad[0])
    at = [int(v) for v in np.unravel_index(k, ref.shape)] if ref.ndim else []
    return Report(False, worst, "%s%s: got %r, reference %r, error %.3e, bound %.3e (%d of %d outside; worst ratio %.3g at flat index %d)" % (
        what, at, float(got.flat[k]), float(ref.flat[k]), float(err.flat[k]), float(bound.flat[k]), len(bad), ratio.size, worst, i))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def rounds_to(got, ref64):
    """got (float32) is the float32 rounding of the float64 reference, bit for bit"""
    return same_bits(got, np.asarray(ref64, F64).astype(F32))


# ---- activations ------------------------------------------------------------------------------------------------------------------
def act64(pre, act):
    with np.errstate(over="ignore"):
        if act == 1:
            return 1.0 / (1.0 + np.exp(-pre))
        if act == 2:
            return np.tanh(pre)
    return pre


def dact64(y, act):
    if act == 1:
        return y * (1.0 - y)
    if act == 2:
        return 1.0 - y * y
    return np.ones_like(y)


def act_bound(pre, Epre, act):
    """(y, propagated part of the bound, evaluation allowance)"""
    y = act64(pre, act)
    if act == 0:
        return y, Epre, np.zeros_like(y)
    v = np.maximum(np.abs(pre) - Epre, 0.0)                                  # both derivatives fall with |pre|
    e = np.exp(-v) if act == 1 else np.exp(-2.0 * v)                         # (from the exponential: y (1 - y) of a y next to 1 cancels)
    L = (1.0 if act == 1 else 4.0) * e / ((1.0 + e) * (1.0 + e))
    return y, L * Epre, ACT_ALLOW[act] * U * np.abs(y) + TINY


# ---- GroupNorm: float64 reference ---------------------------------------------------------------------------------------------------
def gn_ref_fwd(sc, act, swap=False):
    """-> dict: mean, rstd (Bi), y (Bi, C, HW) float64 with their bounds E_mean, E_rstd, E_y = E_prop + E_eval"""
    x = sc.x.astype(F64)
    Bi, C, HW = x.shape
    G = per_sample(sc, sc.gamma, sc.gamma2, swap).astype(F64)[:, :, None]
    Bt = per_sample(sc, sc.beta, sc.beta2, swap).astype(F64)[:, :, None]
    mean = x.mean(axis=(1, 2))
    xc = x - mean[:, None, None]
    var = (xc * xc).mean(axis=(1, 2))
    rstd = 1.0 / np.sqrt(var + sc.eps)
    q = (x * x).mean(axis=(1, 2))
    Em = U * np.abs(mean) + D64 * 2.0 ** -53 * np.abs(x).mean(axis=(1, 2)) + TINY
    Er = rstd * (2 * U + 0.5 * 3 * D64 * 2.0 ** -53 * q / (var + sc.eps)) * SLACK + TINY
    m3, r3 = mean[:, None, None], rstd[:, None, None]
    g = G * r3
    pre = xc * g + Bt
    Epre = SLACK * (U * (np.abs(xc * g) + 2 * np.abs(m3 * g) + np.abs(Bt) + np.abs(pre))
                    + np.abs(G) * (r3 * Em[:, None, None] + np.abs(xc) * Er[:, None, None])) + TINY
    y, Eprop, Eeval = act_bound(pre, Epre, act)
    return dict(mean=mean, rstd=rstd, y=y, pre=pre, E_mean=Em, E_rstd=Er, E_y=Eprop + Eeval, E_prop=Eprop, E_eval=Eeval)


def _edz(dy, y, dz, act):
    if act == 1:
        return 3 * U * np.abs(dz)
    if act == 2:
        return U * np.abs(dy) * y * y + 2 * U * np.abs(dz)
    return np.zeros_like(dz)


def gn_ref_bwd(sc, act, y_k, mr_k):
    """The backward of what the kernel is handed: dy, x, gamma, the forward kernel's y (ignored for act 0) and mean_rstd (Bi, 2).
    -> dict: dx (Bi, C, HW), dgamma, dbeta (C) [, dgamma2, dbeta2] and E_* for each"""
    x, dy = sc.x.astype(F64), sc.dy.astype(F64)
    Bi, C, HW = x.shape
    N = C * HW
    G = per_sample(sc, sc.gamma, sc.gamma2).astype(F64)
    mean, rstd = mr_k[:, 0].astype(F64)[:, None, None], mr_k[:, 1].astype(F64)[:, None, None]
    y = np.asarray(y_k, F64) if act else np.zeros_like(x)
    dz = dy * dact64(y, act)
    Edz = _edz(dy, y, dz, act)
    xhat = (x - mean) * rstd
    S1, S2 = dz.sum(axis=2), (dz * xhat).sum(axis=2)                     # (Bi, C)
    ES1 = (Edz + 2 * U * np.abs(dz)).sum(axis=2) + 2.0 ** -50 * np.abs(dz).sum(axis=2)
    ES2 = (np.abs(xhat) * (Edz + 5 * U * np.abs(dz))).sum(axis=2) + 2.0 ** -50 * np.abs(dz * xhat).sum(axis=2)
    a, q = (G * S1).sum(axis=1) / N, (G * S2).sum(axis=1) / N            # (Bi)
    Ea = (np.abs(G) * ES1).sum(axis=1) / N + U * np.abs(a)
    Eq = (np.abs(G) * ES2).sum(axis=1) / N + U * np.abs(q)
    a3, q3, g3 = a[:, None, None], q[:, None, None], G[:, :, None]
    dx = rstd * (dz * g3 - a3 - xhat * q3)
    Edx = SLACK * (rstd * (np.abs(g3) * Edz + 2 * U * np.abs(dz * g3) + U * np.abs(a3) + Ea[:, None, None] + 3 * U * np.abs(xhat * q3)
                           + np.abs(xhat) * Eq[:, None, None]) + 2 * U * np.abs(dx)) + TINY
    out = dict(dx=dx, E_dx=Edx)
    sets = [("", np.arange(Bi) % 2 == 0), ("2", np.arange(Bi) % 2 == 1)] if sc.gamma2 is not None else [("", np.ones(Bi, bool))]
    for tag, sel in sets:
        for name, S, ES in (("dgamma", S2, ES2), ("dbeta", S1, ES1)):
            v = S[sel].sum(axis=0)
            out[name + tag] = v
            out["E_" + name + tag] = SLACK * (ES[sel].sum(axis=0) + U * np.abs(v)) + TINY
    return out


# ---- GroupNorm: a float32 model of the kernels' order of operations ---------------------------------------------------------------
def fma32(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def act32(v, act):
    """float32 in, float32 out, the kernel's expressions with a correctly rounded exp / tanh"""
    v = np.asarray(v, F32)
    with np.errstate(over="ignore"):
        if act == 1:
            e = np.exp(-v.astype(F64)).astype(F32)
            return (F32(1) / (F32(1) + e)).astype(F32)
        if act == 2:
            return np.tanh(v.astype(F64)).astype(F32)
    return v


def dact32(dy, y, act):
    if act == 1:
        return dy * (y * (F32(1) - y))
    if act == 2:
        return dy * (F32(1) - y * y)
    return dy


GN_PLANTS = ("chunk-last-element-dropped", "pair-parity-swapped", "fold-gamma-index-j-mod-C", "dx-at-stride-of-one-sample")


def gn_plant_applies(c, plant):
    if plant == "pair-parity-swapped":
        return c.pair
    if plant == "fold-gamma-index-j-mod-C":
        return cdiv(c.HW, GN_ELEMS) > 1 and c.C > 1
    if plant == "dx-at-stride-of-one-sample":
        return internal_B(c) > 1 and gn_layout(c).dxbs > c.C * c.HW
    return True


def gn_model_fwd(c, sc, act, plant=None):
    """-> (y (Bi, C, HW) float32, mean_rstd (Bi, 2) float32)"""
    x = sc.x
    Bi, C, HW = x.shape
    n = C * HW
    mr = np.zeros((Bi, 2), F32)
    for b in range(Bi):
        flat = x[b].reshape(-1).astype(F64)
        s = q = 0.0
        for i0, i1, _ in gn_stats_chunks(c, b):
            if plant == "chunk-last-element-dropped":
                i1 -= 1
            s += flat[i0:i1].sum()
            q += (flat[i0:i1] * flat[i0:i1]).sum()
        m = s / n
        var = max(q / n - m * m, 0.0)
        mr[b] = F32(m), F32(1.0 / math.sqrt(var + float(sc.eps)))
    swap = plant == "pair-parity-swapped"
    G, Bt = per_sample(sc, sc.gamma, sc.gamma2, swap), per_sample(sc, sc.beta, sc.beta2, swap)
    g = (G * mr[:, 1:2]).astype(F32)                                      # (Bi, C)
    o = (Bt - (mr[:, 0:1] * g).astype(F32)).astype(F32)
    y = act32(fma32(x, g[:, :, None], o[:, :, None]), act)
    return y, mr


def gn_model_bwd(c, sc, act, y, mr, plant=None, y_null=False):
    """The backward kernels on the forward's (y, mean_rstd).  -> dict dx (Bi, C, HW), dgamma, dbeta[, dgamma2, dbeta2], float32.
    dx passes through a flat buffer at the case's batch stride, NaN between the samples, as the entry writes it."""
    x, dy = sc.x, sc.dy
    Bi, C, HW = x.shape
    N = C * HW
    mean, rstd = mr[:, 0][:, None, None], mr[:, 1][:, None, None]
    dz = dact32(dy, y, act).astype(F32)
    xh = ((x - mean) * rstd).astype(F32)
    segs = gn_segments(c)
    nseg = len(segs)
    rows = np.zeros((Bi, C, nseg, 2))
    ops = ("x", "dy") if y_null else ("x", "dy", "y")
    for b in range(Bi):
        for k in range(C):
            for s, (i0, i1) in enumerate(segs):
                z, h = dz[b, k, i0:i1], xh[b, k, i0:i1]
                if gn_row_vec4(c, b, k, (i0, i1), ops):
                    zq, pq = z.reshape(-1, 4), (z * h).reshape(-1, 4)
                    rows[b, k, s, 0] = ((zq[:, 0] + zq[:, 1]) + (zq[:, 2] + zq[:, 3])).astype(F64).sum()
                    rows[b, k, s, 1] = ((pq[:, 0] + pq[:, 1]) + (pq[:, 2] + pq[:, 3])).astype(F64).sum()
                else:
                    rows[b, k, s, 0] = z.astype(F64).sum()
                    rows[b, k, s, 1] = (z.astype(F64) * h.astype(F64)).sum()
    G = per_sample(sc, sc.gamma, sc.gamma2)
    j = np.arange(C * nseg)
    gi = j % C if plant == "fold-gamma-index-j-mod-C" else j // nseg
    fl = rows.reshape(Bi, C * nseg, 2)
    a = ((G[:, gi].astype(F64) * fl[:, :, 0]).sum(axis=1) / N).astype(F32)[:, None, None]
    q = ((G[:, gi].astype(F64) * fl[:, :, 1]).sum(axis=1) / N).astype(F32)[:, None, None]
    dx = (rstd * ((dz * G[:, :, None] - a) - xh * q)).astype(F32)
    L = gn_layout(c)
    stride = N if plant == "dx-at-stride-of-one-sample" else L.dxbs
    buf = np.full(((Bi - 1) * L.dxbs + N,), np.nan, F32)
    for b in range(Bi):
        buf[b * stride:b * stride + N] = dx[b].reshape(-1)
    out = dict(dx=np.stack([buf[b * L.dxbs:b * L.dxbs + N] for b in range(Bi)]).reshape(Bi, C, HW))
    sets = [("", np.arange(Bi) % 2 == 0), ("2", np.arange(Bi) % 2 == 1)] if sc.gamma2 is not None else [("", np.ones(Bi, bool))]
    for tag, sel in sets:
        out["dbeta" + tag] = rows[sel][..., 0].sum(axis=(0, 2)).astype(F32)
        out["dgamma" + tag] = rows[sel][..., 1].sum(axis=(0, 2)).astype(F32)
    return out


# ---- BatchNorm --------------------------------------------------------------------------------------------------------------------
def bn_ref_fwd(sc, relu):
    """-> dict: mean, rstd, mean - pivot (C), y (B, C, N), new running statistics, and E_* for each (E_saved0: of saved[2c] + pivot)"""
    x = sc.x.astype(F64)
    B, C, N = x.shape
    cnt = B * N
    p = x[0, :, 0]
    mean = x.mean(axis=(0, 2))
    xc = x - mean[None, :, None]
    var = (xc * xc).mean(axis=(0, 2))
    rstd = 1.0 / np.sqrt(var + sc.eps)
    d = x - p[None, :, None]
    ad, dd = np.abs(d).mean(axis=(0, 2)), (d * d).mean(axis=(0, 2))
    ms = mean - p
    Esum = 65 * U * ad                                                   # of the float64 mean of d, before its float32 rounding
    Ems = SLACK * (Esum + U * np.abs(ms)) + TINY
    Evar = SLACK * (67 * U * dd + 2 * np.abs(ms) * Esum + Esum * Esum)
    Er = SLACK * rstd * (2 * U + 0.5 * Evar / (var + sc.eps)) + TINY
    gam, bet = sc.gamma.astype(F64)[None, :, None], sc.beta.astype(F64)[None, :, None]
    scale = gam * rstd[None, :, None]
    pre = xc * scale + bet
    Epre = SLACK * (np.abs(scale) * (U * np.abs(d) + U * np.abs(xc) + Ems[None, :, None]) + np.abs(gam * xc) * Er[None, :, None]
                    + U * np.abs(scale * xc) + U * np.abs(pre)) + TINY
    y = np.maximum(pre, 0.0) if relu else pre
    mom = float(sc.momentum)
    Emean = Esum + U * np.abs(mean)
    unb = var * cnt / (cnt - 1.0) if cnt > 1 else var
    Eunb = Evar * (cnt / (cnt - 1.0) if cnt > 1 else 1.0) + U * np.abs(unb)
    rm0, rv0 = sc.rm.astype(F64), sc.rv.astype(F64)
    rm, rv = (1 - mom) * rm0 + mom * mean, (1 - mom) * rv0 + mom * unb
    Erm = SLACK * (mom * Emean + U * (2 * np.abs((1 - mom) * rm0) + np.abs(mom * mean) + np.abs(rm))) + TINY
    Erv = SLACK * (mom * Eunb + U * (2 * np.abs((1 - mom) * rv0) + np.abs(mom * unb) + np.abs(rv))) + TINY
    return dict(mean=mean, rstd=rstd, y=y, pre=pre, rm=rm, rv=rv, E_saved0=Ems, E_rstd=Er, E_y=Epre, E_rm=Erm, E_rv=Erv)


def bn_ref_bwd(sc, relu, y_k, saved_k):
    """The backward of what the kernel is handed: dy, x, gamma, beta and the forward kernel's saved pair; the ReLU mask is the forward
    kernel's y > 0.  -> dict dx, dgamma, dbeta, E_*"""
    x, dy = sc.x.astype(F64), sc.dy.astype(F64)
    B, C, N = x.shape
    cnt = B * N
    p = x[0, :, 0][None, :, None]
    ms, rstd = saved_k[:, 0].astype(F64)[None, :, None], saved_k[:, 1].astype(F64)[None, :, None]
    gam = sc.gamma.astype(F64)[None, :, None]
    d = x - p
    xc = d - ms
    xhat = xc * rstd
    dz = np.where(np.asarray(y_k) > 0, dy, 0.0) if relu else dy
    scale = gam * rstd
    T1, T2 = dz.sum(axis=(0, 2)), (dz * xhat).sum(axis=(0, 2))
    Exc = U * np.abs(d) + U * np.abs(xc)
    Exh = rstd * Exc + U * np.abs(xhat)
    ET1 = 64 * U * np.abs(dz).sum(axis=(0, 2))
    ET2 = (np.abs(dz) * Exh).sum(axis=(0, 2)) + 64 * U * np.abs(dz * xhat).sum(axis=(0, 2))
    t1, t2 = (T1 / cnt)[None, :, None], (T2 / cnt)[None, :, None]
    Et1, Et2 = (ET1 / cnt)[None, :, None] + U * np.abs(t1), (ET2 / cnt)[None, :, None] + U * np.abs(t2)
    inner = dz - t1 - xhat * t2
    dx = scale * inner
    Edx = SLACK * (np.abs(scale) * (U * (np.abs(dz) + np.abs(t1)) + Et1 + Exh * np.abs(t2) + np.abs(xhat) * Et2 + U * np.abs(xhat * t2)
                                    + U * np.abs(inner)) + 2 * U * np.abs(dx)) + TINY
    return dict(dx=dx, dgamma=T2, dbeta=T1, E_dx=Edx, E_dgamma=SLACK * (ET2 + U * np.abs(T2)) + TINY, E_dbeta=SLACK * (ET1 + U * np.abs(T1)) + TINY)


BN_PLANTS = ("pivot-from-channel-0", "mask-greater-or-equal")


def bn_plant_applies(c, plant, kind=None):
    if plant == "pivot-from-channel-0":
        return c.C > 1
    return True


def _bn_threads(c, a):
    """(B, C, N) -> (B, C, nchunk, 64, 256): element [.., r, t] is the r-th a thread t of the chunk's block meets (0 where it meets
    none: an exact no-op in both sums).  float4: thread t takes 4 t .. 4 t + 3 of every 1024; scalar: t of every 256."""
    B, C, N = a.shape
    nchunk = cdiv(N, BN_CHUNK)
    pad = np.zeros((B, C, nchunk * BN_CHUNK), a.dtype)
    pad[:, :, :N] = a
    if bn_vec4(c):
        return pad.reshape(B, C, nchunk, 16, BN_BLOCK, 4).transpose(0, 1, 2, 3, 5, 4).reshape(B, C, nchunk, 64, BN_BLOCK)
    return pad.reshape(B, C, nchunk, 64, BN_BLOCK)


def bn_model_fwd(c, sc, relu, plant=None):
    """-> dict y (B, C, N), saved (C, 2), rm, rv (C), float32"""
    x = sc.x
    B, C, N = x.shape
    cnt = float(B * N)
    p = x[0, :, 0].copy()
    ps = np.full_like(p, p[0]) if plant == "pivot-from-channel-0" else p              # (the statistics kernel's pivot alone)
    dv = _bn_threads(c, (x - ps[None, :, None]).astype(F32))
    s1 = np.zeros(dv.shape[:3] + (BN_BLOCK,), F32)
    s2 = np.zeros_like(s1)
    for r in range(64):
        s1 = s1 + dv[:, :, :, r]
        s2 = fma32(dv[:, :, :, r], dv[:, :, :, r], s2)
    S1, S2 = s1.astype(F64).sum(axis=(0, 2, 3)), s2.astype(F64).sum(axis=(0, 2, 3))
    ms = S1 / cnt
    m = p.astype(F64) + ms
    var = np.maximum(S2 / cnt - ms * ms, 0.0)
    mean, mshift, rstd = m.astype(F32), ms.astype(F32), (1.0 / np.sqrt(var + float(sc.eps))).astype(F32)
    scale = (sc.gamma * rstd).astype(F32)
    xc = ((x - p[None, :, None]).astype(F32) - mshift[None, :, None]).astype(F32)
    y = fma32(xc, scale[None, :, None], sc.beta[None, :, None])
    if relu:
        y = np.maximum(y, F32(0))
    mom = F32(sc.momentum)
    unb = (var * cnt / (cnt - 1.0) if cnt > 1 else var).astype(F32)
    rm = ((F32(1) - mom) * sc.rm + mom * mean).astype(F32)
    rv = ((F32(1) - mom) * sc.rv + mom * unb).astype(F32)
    return dict(y=y, saved=np.stack([mshift, rstd], axis=1), rm=rm, rv=rv)


def bn_model_bwd(c, sc, relu, saved, plant=None):
    x, dy = sc.x, sc.dy
    B, C, N = x.shape
    cnt = float(B * N)
    p = x[0, :, 0][None, :, None]
    mean, rstd = saved[:, 0][None, :, None], saved[:, 1][None, :, None]
    scale = (sc.gamma[None, :, None] * rstd).astype(F32)
    xc = ((x - p).astype(F32) - mean).astype(F32)
    pre = fma32(xc, scale, sc.beta[None, :, None])
    keep = (pre >= 0 if plant == "mask-greater-or-equal" else pre > 0) if relu else np.ones(x.shape, bool)
    g = np.where(keep, dy, F32(0)).astype(F32)
    xh = (xc * rstd).astype(F32)
    gt, ht = _bn_threads(c, g), _bn_threads(c, xh)
    s1 = np.zeros(gt.shape[:3] + (BN_BLOCK,), F32)
    s2 = np.zeros_like(s1)
    for r in range(64):
        s1 = s1 + gt[:, :, :, r]
        s2 = fma32(gt[:, :, :, r], ht[:, :, :, r], s2)
    T1, T2 = s1.astype(F64).sum(axis=(0, 2, 3)), s2.astype(F64).sum(axis=(0, 2, 3))
    t1, t2 = (T1 / cnt).astype(F32)[None, :, None], (T2 / cnt).astype(F32)[None, :, None]
    dx = (scale * ((g - t1) - xh * t2)).astype(F32)
    return dict(dx=dx, dgamma=T2.astype(F32), dbeta=T1.astype(F32))


# ---- GRU element-wise entries: float32 expressions that give the kernels' bits ----------------------------------------------------
def blend_fwd32(u, h, y, plant=None):
    out = (u * h + (F32(1) - u) * y).astype(F32)
    if plant == "blend-tail-dropped":
        out[4 * (len(out) // 4):] = np.nan                               # (never written: the caller's sentinel stays)
    return out


def blend_bwd32(dy, u, h, y):
    return (dy * (h - y)).astype(F32), (dy * u).astype(F32), (dy * (F32(1) - u)).astype(F32)          # du, dh, dcand


def mulcat_fwd32(x, r, h):
    return np.concatenate([x, (r * h).astype(F32)], axis=1)


def mulcat_bwd32(dcat, r, h, Cx):
    g = dcat[:, Cx:]
    return (g * h).astype(F32), (g * r).astype(F32)                     # dr, dh


def mulcat_bwd_acc64(dcat, r, h, dh_acc, Cx):
    """-> dr (float32 bits), the new second half of dcat in float64 and its bound u |ref|"""
    g = dcat[:, Cx:]
    ref = g.astype(F64) * r.astype(F64) + dh_acc.astype(F64)
    return (g * h).astype(F32), ref, U * np.abs(ref) + TINY


# ---- judges: one call's outputs against reference and bound, shared by the CPU and the GPU tests ---------------------------------
class Verdict:
    """ok, the failures' messages, and the worst err / bound per output (act-allowance: the share of the activation's evaluation
    allowance used after the propagated part of the bound is taken off)"""

    def __init__(self):
        self.ratios, self.messages = {}, []

    @property
    def ok(self):
        return not self.messages

    def held(self, name, got, ref, bound, what):
        r = check(got, ref, bound, what + " " + name)
        self.ratios[name] = max(self.ratios.get(name, 0.0), r.ratio)
        if not r.ok:
            self.messages.append(r.message)

    def equal(self, name, got, ref64, what):
        if not rounds_to(got, ref64):
            self.messages.append("%s %s: not the float32 rounding of the float64 reference (%d elements differ)" % (
                what, name, int((np.asarray(got, F32) != np.asarray(ref64, F64).astype(F32)).sum())))


def gn_judge_fwd(c, kind, act, y, mr, ref=None):
    sc = gn_scene(c, kind)
    ref = ref or gn_ref_fwd(sc, act)
    what = "%s %s act %d" % (c.name, kind, act)
    for k in ("y", "mean", "rstd"):
        assert_complete(ref[k], ref["E_" + k], sc.x.shape if k == "y" else sc.x.shape[:1], what + " " + k)
    v = Verdict()
    v.held("mean", mr[:, 0], ref["mean"], ref["E_mean"], what)
    v.held("rstd", mr[:, 1], ref["rstd"], ref["E_rstd"], what)
    v.held("y", y, ref["y"], ref["E_y"], what)
    if act:
        excess = np.maximum(np.abs(np.asarray(y, F64) - ref["y"]) - ref["E_prop"], 0.0)
        excess = np.where(np.isfinite(excess), excess, np.inf)
        v.ratios["act-allowance"] = float((excess / ref["E_eval"]).max())
    elif kind.startswith("exact"):
        v.equal("mean", mr[:, 0], ref["mean"], what)
        v.equal("rstd", mr[:, 1], ref["rstd"], what)
        v.equal("y", y, ref["y"], what)
    return v


def gn_judge_bwd(c, kind, act, y_k, mr_k, got):
    """got: dict dx, dgamma, dbeta[, dgamma2, dbeta2] of the backward fed with the forward's (y_k, mr_k)"""
    sc = gn_scene(c, kind)
    ref = gn_ref_bwd(sc, act, y_k, mr_k)
    what = "%s %s act %d" % (c.name, kind, act)
    v = Verdict()
    names = ["dx", "dgamma", "dbeta"] + (["dgamma2", "dbeta2"] if c.pair else [])
    for k in names:
        assert_complete(ref[k], ref["E_" + k], sc.x.shape if k == "dx" else (c.C,), what + " " + k)
        v.held(k, got[k], ref[k], ref["E_" + k], what)
        if kind.startswith("exact") and act == 0 and k != "dx":
            v.equal(k, got[k], ref[k], what)
    return v


def bn_judge_fwd(c, kind, relu, got, running=True, ref=None):
    """got: dict y, saved[, rm, rv]"""
    sc = bn_scene(c, kind)
    ref = ref or bn_ref_fwd(sc, relu)
    what = "bn %s %s relu %d" % (c.name, kind, relu)
    v = Verdict()
    p = sc.x[0, :, 0].astype(F64)
    outs = [("y", got["y"], ref["y"], ref["E_y"]), ("mean", got["saved"][:, 0].astype(F64) + p, ref["mean"], ref["E_saved0"]),
            ("rstd", got["saved"][:, 1], ref["rstd"], ref["E_rstd"])]
    if running:
        outs += [("running_mean", got["rm"], ref["rm"], ref["E_rm"]), ("running_var", got["rv"], ref["rv"], ref["E_rv"])]
    for k, g, r, e in outs:
        assert_complete(r, e, sc.x.shape if k == "y" else (c.C,), what + " " + k)
        v.held(k, g, r, e, what)
        if kind.startswith("exact") and k != "running_var":
            v.equal(k, g, r, what)
    return v


def bn_judge_bwd(c, kind, relu, y_k, saved_k, got):
    sc = bn_scene(c, kind)
    ref = bn_ref_bwd(sc, relu, y_k, saved_k)
    what = "bn %s %s relu %d" % (c.name, kind, relu)
    v = Verdict()
    for k in ("dx", "dgamma", "dbeta"):
        assert_complete(ref[k], ref["E_" + k], sc.x.shape if k == "dx" else (c.C,), what + " " + k)
        v.held(k, got[k], ref[k], ref["E_" + k], what)
        if kind.startswith("exact") and k != "dx":
            v.equal(k, got[k], ref[k], what)
    return v
