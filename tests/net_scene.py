"""Cases, parameters, packing references, float64 layers and per-element bounds for the three native inference networks --
smvs_featnet_fwd (csrc/featnet.hip), smvs_costreg_fwd (csrc/costreg.hip) and smvs_red_step_fwd (csrc/red.hip) -- judged LAYER BY LAYER:
each entry keeps every intermediate tensor in a caller-owned workspace whose layout is a plain sequence of take() calls, mirrored here.
After one call the GPU test reads every tensor back, and each layer is evaluated in float64 on the float32 input the GPU itself
produced, so no propagated error enters a bound and no element is excused.  Shared by tests/test_net_cpu.py (which proves, without a
GPU, that the judge accepts a correct float32 evaluation and rejects planted kernel faults) and tests/test_net_gpu.py.  Nothing here
imports the kernels.  The sections: featnet (below), costreg, RED's packing and sizes, RED's plane step stage by stage.

The bound of one layer, per element (u = 2^-24):
    acc   = the kernel's chain of n fused multiply-adds from 0.0f  (fn_conv_kernel: n = Cin K K; fn_convT_kernel: at most 4 taps
            of every input channel reach one output, n = 4 Cin): |acc - y| <= gamma_n A, A = the same layer on |x|, |w|
    r     = fmaf(acc, scale, shift): one rounding of the exact acc * scale + shift
    r     = max(r, 0): 1-Lipschitz, exact
    r     = up + r (fpn lateral): one more rounding
so  |got - ref| <= (n + 2) u M  [+ u (|up| + M) with a lateral]  with M = |scale| A + |shift|, as long as 2 n u + n^2 u <= 1 (n <= 800
here).  The constant c = 2 of conv_scene.bound_from is therefore 1 (first-order slack of gamma_n) + 1 (the fma of the epilogue); these
kernels neither split channels over waves nor split K.  (n + 2) 2^-126 (1 + |scale|) covers products that underflow.
scale and shift are the float32 numbers the GPU packed (checked bit for bit against fn_pack_reference on their own)."""
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import norm_scene as _N

U32 = 2.0 ** -24
TINY = 2.0 ** -126
BN_EPS = 1e-5                                  # the eps the pack kernels fold (csrc/featnet.hip: fn_pack_bn_kernel)

# ---- featnet ----------------------------------------------------------------------------------------------------------------------
FnLayer = namedtuple("FnLayer", "name cin cout k stride transposed bn relu bias")
FnStep = namedtuple("FnStep", "inA inB CB out lin lout up")          # tensor names; lin / lout: 0 full, 1 half, 2 quarter
FnCase = namedtuple("FnCase", "N H W c arch")

_FN_SHAPES = [(1, 4, 4, 8), (3, 8, 260, 8), (1, 20, 64, 5), (1, 12, 68, 4), (1, 36, 72, 12), (2, 12, 132, 16)]
FN_CASES = [FnCase(*s, arch) for s in _FN_SHAPES for arch in (0, 1)]
FN_COT = 8


def fn_id(case):
    return "%s-n%d-%dx%d-c%d" % ("unet" if case.arch == 0 else "fpn", case.N, case.H, case.W, case.c)


def fn_layers(c, arch):
    """The layers in execution order (fn_layers of csrc/featnet.hip)."""
    L = [FnLayer("conv0.0", 3, c, 3, 1, 0, 1, 1, 0), FnLayer("conv0.1", c, c, 3, 1, 0, 1, 1, 0),
         FnLayer("conv1.0", c, 2 * c, 5, 2, 0, 1, 1, 0), FnLayer("conv1.1", 2 * c, 2 * c, 3, 1, 0, 1, 1, 0), FnLayer("conv1.2", 2 * c, 2 * c, 3, 1, 0, 1, 1, 0),
         FnLayer("conv2.0", 2 * c, 4 * c, 5, 2, 0, 1, 1, 0), FnLayer("conv2.1", 4 * c, 4 * c, 3, 1, 0, 1, 1, 0), FnLayer("conv2.2", 4 * c, 4 * c, 3, 1, 0, 1, 1, 0)]
    if arch == 0:
        return L + [FnLayer("out1", 4 * c, 4 * c, 1, 1, 0, 0, 0, 0),
                    FnLayer("deconv1.deconv", 4 * c, 2 * c, 3, 2, 1, 1, 1, 0), FnLayer("deconv1.conv", 4 * c, 2 * c, 3, 1, 0, 1, 1, 0),
                    FnLayer("out2", 2 * c, 2 * c, 1, 1, 0, 0, 0, 0),
                    FnLayer("deconv2.deconv", 2 * c, c, 3, 2, 1, 1, 1, 0), FnLayer("deconv2.conv", 2 * c, c, 3, 1, 0, 1, 1, 0),
                    FnLayer("out3", c, c, 1, 1, 0, 0, 0, 0)]
    return L + [FnLayer("out1", 4 * c, 4 * c, 1, 1, 0, 0, 0, 0),
                FnLayer("inner1", 2 * c, 4 * c, 1, 1, 0, 0, 0, 1), FnLayer("out2", 4 * c, 2 * c, 3, 1, 0, 0, 0, 0),
                FnLayer("inner2", c, 4 * c, 1, 1, 0, 0, 0, 1), FnLayer("out3", 4 * c, c, 3, 1, 0, 0, 0, 0)]


def fn_steps(c, arch):
    """Which tensors each layer reads and writes (the Step tables of smvs_featnet_fwd)."""
    S = [FnStep("imgs", None, 0, "t0", 0, 0, None), FnStep("t0", None, 0, "c0", 0, 0, None),
         FnStep("c0", None, 0, "t1a", 0, 1, None), FnStep("t1a", None, 0, "t1b", 1, 1, None), FnStep("t1b", None, 0, "c1", 1, 1, None),
         FnStep("c1", None, 0, "t2a", 1, 2, None), FnStep("t2a", None, 0, "t2b", 2, 2, None), FnStep("t2b", None, 0, "c2", 2, 2, None)]
    if arch == 0:
        return S + [FnStep("c2", None, 0, "stage1", 2, 2, None),
                    FnStep("c2", None, 0, "up1", 2, 1, None), FnStep("up1", "c1", 2 * c, "f1", 1, 1, None),
                    FnStep("f1", None, 0, "stage2", 1, 1, None),
                    FnStep("f1", None, 0, "up2", 1, 0, None), FnStep("up2", "c0", c, "f2", 0, 0, None),
                    FnStep("f2", None, 0, "stage3", 0, 0, None)]
    return S + [FnStep("c2", None, 0, "stage1", 2, 2, None),
                FnStep("c1", None, 0, "f1", 1, 1, "c2"), FnStep("f1", None, 0, "stage2", 1, 1, None),
                FnStep("c0", None, 0, "f2", 0, 0, "f1"), FnStep("f2", None, 0, "stage3", 0, 0, None)]


def fn_accepts(N, H, W, c, arch):
    """smvs_featnet_workspace_bytes != 0, and the pack entry's limit of 64 folded channels per layer."""
    if N < 1 or c < 1 or H < 4 or W < 4 or H % 4 or W % 4 or arch not in (0, 1):
        return False
    if 4 * c * H * W * 4 >= 2 ** 31 or N * ((4 * c + FN_COT - 1) // FN_COT) > 65535:
        return False
    return 4 * c <= 64


def _round4(n):
    return (n + 3) & ~3


def fn_workspace(N, H, W, c, arch):
    """name -> (offset in floats, shape), and the total in floats (fn_workspace of csrc/featnet.hip)."""
    o = 0
    lay = {}

    def take(name, ch, lvl):
        nonlocal o
        shape = (N, ch, H >> lvl, W >> lvl)
        lay[name] = (o, shape)
        o += _round4(int(np.prod(shape)))
    take("t0", c, 0); take("c0", c, 0)
    take("t1a", 2 * c, 1); take("t1b", 2 * c, 1); take("c1", 2 * c, 1)
    take("t2a", 4 * c, 2); take("t2b", 4 * c, 2); take("c2", 4 * c, 2)
    if arch == 0:
        take("up1", 2 * c, 1); take("f1", 2 * c, 1); take("up2", c, 0); take("f2", c, 0)
    else:
        take("f1", 4 * c, 1); take("f2", 4 * c, 0)
    return lay, o


def fn_out_shapes(case):
    N, H, W, c = case[:4]
    return {"stage1": (N, 4 * c, H // 4, W // 4), "stage2": (N, 2 * c, H // 2, W // 2), "stage3": (N, c, H, W)}


def fn_packed_layout(c, arch):
    """per layer (w, scale, shift) offsets in floats, and the total (fn_layout)."""
    o = 0
    lay = []
    for l in fn_layers(c, arch):
        ncog = (l.cout + FN_COT - 1) // FN_COT
        wo = o; o += ncog * l.cin * l.k * l.k * FN_COT
        so = o; o += ncog * FN_COT
        to = o; o += ncog * FN_COT
        lay.append((wo, so, to))
    return lay, o


def fn_param_names(c, arch):
    """The pointer order of smvs_featnet_pack_weights as include/satmvs.h states it: 63 names (unet) or 47 (fpn)."""
    bn5 = (".conv.weight", ".bn.weight", ".bn.bias", ".bn.running_mean", ".bn.running_var")
    names = [b + s for b in ("conv0.0", "conv0.1", "conv1.0", "conv1.1", "conv1.2", "conv2.0", "conv2.1", "conv2.2") for s in bn5]
    if arch == 0:
        names += [b + s for b in ("deconv1.deconv", "deconv1.conv", "deconv2.deconv", "deconv2.conv") for s in bn5]
        return names + ["out1.weight", "out2.weight", "out3.weight"]
    return names + ["out1.weight", "inner1.weight", "inner1.bias", "out2.weight", "inner2.weight", "inner2.bias", "out3.weight"]


def _layer_keys(l):
    """state-dict names of a layer's (weight, then the four BatchNorm tensors or the bias)."""
    if l.bn:
        return [l.name + s for s in (".conv.weight", ".bn.weight", ".bn.bias", ".bn.running_mean", ".bn.running_var")]
    return [l.name + ".weight"] + ([l.name + ".bias"] if l.bias else [])


@functools.lru_cache(maxsize=None)
def fn_params(c, arch, seed=0):
    """name -> float32 CPU tensor, every tensor the pack entry takes randomised.  BatchNorm gamma of both signs with one exact zero per
    layer, one small running variance per layer (1e-4: eps is a tenth of it; its gamma is small so that the channel does not take
    over the next layer), beta and running mean away from zero.  Weights scaled so that activations neither die nor grow."""
    g = torch.Generator().manual_seed(1000 * c + 10 * arch + seed)
    P = {}
    for i, l in enumerate(fn_layers(c, arch)):
        wshape = (l.cin, l.cout, l.k, l.k) if l.transposed else (l.cout, l.cin, l.k, l.k)
        fan = l.cin * (4 if l.transposed else l.k * l.k)
        keys = _layer_keys(l)
        P[keys[0]] = torch.randn(wshape, generator=g) * (2.0 / fan) ** 0.5
        if l.bn:
            sign = 1.0 - 2.0 * ((torch.arange(l.cout) + i) % 2)               # alternating: both signs at any cout >= 3
            gamma = (0.5 + torch.rand(l.cout, generator=g)) * sign
            var = 0.5 + 1.5 * torch.rand(l.cout, generator=g)
            small, zero = (3 * i + 1) % l.cout, (5 * i + 2) % l.cout
            if zero == small:
                zero = (zero + 1) % l.cout
            var[small] = 1e-4
            gamma[small] = 0.02 * sign[small]
            gamma[zero] = 0.0
            P[keys[1]] = gamma
            P[keys[2]] = 0.5 * torch.randn(l.cout, generator=g)
            P[keys[3]] = 0.3 * torch.randn(l.cout, generator=g)
            P[keys[4]] = var
        elif l.bias:
            P[keys[1]] = torch.randn(l.cout, generator=g)
    assert list(P) and sorted(P) == sorted(fn_param_names(c, arch))
    return P


@functools.lru_cache(maxsize=None)
def fn_images(case):
    g = torch.Generator().manual_seed(7 + case.N * 31 + case.H * 17 + case.W * 3 + case.c * 5 + case.arch)
    return torch.randn((case.N, 3, case.H, case.W), generator=g)


def fold_bn(gamma, beta, mean, var, eps=BN_EPS):
    """(scale, shift) float32: the float32 rounding of the float64 expressions of fn_pack_bn_kernel."""
    sd = gamma.double() / torch.sqrt(var.double() + eps)
    return sd.float(), (beta.double() - mean.double() * sd).float()


def fn_pack_reference(P, c, arch):
    """The packed buffer as smvs_featnet_pack_weights must write it: weights permuted to [cout group][cin][tap][8] (zero beyond cout),
    then scale and shift padded to 8 with the identity (1, 0); modes "fold the BatchNorm", "plain bias" (scale 1) and "identity"."""
    lay, total = fn_packed_layout(c, arch)
    out = torch.zeros(total, dtype=torch.float32)
    for l, (wo, so, to) in zip(fn_layers(c, arch), lay):
        keys = _layer_keys(l)
        w = P[keys[0]]
        if l.transposed:
            w = w.permute(1, 0, 2, 3)
        ncog = (l.cout + FN_COT - 1) // FN_COT
        wp = torch.zeros((ncog * FN_COT, l.cin, l.k * l.k), dtype=torch.float32)
        wp[:l.cout] = w.reshape(l.cout, l.cin, l.k * l.k)
        out[wo:wo + wp.numel()] = wp.view(ncog, FN_COT, l.cin, l.k * l.k).permute(0, 2, 3, 1).reshape(-1)
        s = torch.ones(ncog * FN_COT)
        t = torch.zeros(ncog * FN_COT)
        if l.bn:
            s[:l.cout], t[:l.cout] = fold_bn(*[P[k] for k in keys[1:]])
        elif l.bias:
            t[:l.cout] = P[keys[1]]
        out[so:so + s.numel()] = s
        out[to:to + t.numel()] = t
    return out


def fn_scale_shift(packed, c, arch):
    """per layer (scale, shift), float32 of length cout, out of a packed buffer"""
    lay, _ = fn_packed_layout(c, arch)
    return [(packed[so:so + l.cout].clone(), packed[to:to + l.cout].clone()) for l, (wo, so, to) in zip(fn_layers(c, arch), lay)]


def _conv(l, x, w):
    if l.transposed:
        return F.conv_transpose2d(x, w, stride=2, padding=1, output_padding=1)
    return F.conv2d(x, w, stride=l.stride, padding=l.k // 2)


def _up2(t):
    return t.repeat_interleave(2, 2).repeat_interleave(2, 3)


def fn_layer64(l, xa, xb, w, scale, shift, up):
    """-> (ref, bound) float64 of one layer on the float32 tensors given."""
    x = (xa if xb is None else torch.cat([xa, xb], 1)).double()
    wd = w.double()
    s, t = scale.double().view(1, -1, 1, 1), shift.double().view(1, -1, 1, 1)
    r = _conv(l, x, wd) * s + t
    if l.relu:
        r = F.relu(r)
    n = l.cin * (4 if l.transposed else l.k * l.k)
    M = _conv(l, x.abs(), wd.abs()) * s.abs() + t.abs()
    bound = (n + 2) * U32 * M + (n + 2) * TINY * (1.0 + s.abs())
    if up is not None:
        u = _up2(up.double())
        r = r + u
        bound = bound + U32 * (u.abs() + M)
    return r, bound


def worst_ratio(got, ref, bound):
    """largest err / bound and where; a non-finite `got` where ref is finite counts as infinite"""
    err = (got.double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    r = err / bound
    i = int(torch.argmax(r))
    return float(r.flatten()[i]), tuple(int(v) for v in np.unravel_index(i, tuple(r.shape)))


def fn_judge(case, P, packed, T):
    """T: name -> float32 CPU tensor of every tensor of one forward ("imgs", the workspace tensors, "stage1".."stage3").
    -> list over layers of (layer name, kernel kind, ratio, where): every layer in float64 on the inputs found in T."""
    L, S = fn_layers(case.c, case.arch), fn_steps(case.c, case.arch)
    ss = fn_scale_shift(packed, case.c, case.arch)
    res = []
    for l, st, (s, t) in zip(L, S, ss):
        ref, bound = fn_layer64(l, T[st.inA], T[st.inB] if st.inB else None, P[_layer_keys(l)[0]], s, t, T[st.up] if st.up else None)
        got = T[st.out]
        assert got.shape == ref.shape, (l.name, got.shape, ref.shape)
        ratio, where = worst_ratio(got, ref, bound)
        res.append((l.name, fn_kind(l), ratio, where))
    return res


def fn_kind(l):
    return "convT" if l.transposed else "conv%dx%d s%d" % (l.k, l.k, l.stride)


def fn_tensors(case, imgs, ws, outs):
    """The dict fn_judge takes, from the workspace read back as a flat float32 tensor and the three outputs."""
    lay, total = fn_workspace(*case)
    assert ws.numel() == total
    T = {"imgs": imgs}
    for name, (o, shape) in lay.items():
        T[name] = ws[o:o + int(np.prod(shape))].view(shape)
    T.update(outs)
    return T


def fma32(a, s, t):
    """fmaf(a, s, t) on float32 tensors: the product of two float32 is exact in float64 and the sum is rounded once there (2^-53),
    then to float32"""
    return (a.double() * s.double() + t.double()).float()


FN_FAULTS = ("tile-column-zero", "shift-mod-8", "concat-swapped", "lateral-row-stride")


def fn_model32(case, P, packed, imgs, fault=None, at=None):
    """A float32 CPU evaluation of the network, layer by layer with torch's float32 operators in place of the kernels: the tensors of
    fn_tensors.  fault (one of FN_FAULTS) plants a kernel error into layer index `at`."""
    L, S = fn_layers(case.c, case.arch), fn_steps(case.c, case.arch)
    ss = fn_scale_shift(packed, case.c, case.arch)
    T = {"imgs": imgs}
    for i, (l, st, (s, t)) in enumerate(zip(L, S, ss)):
        bad = fault if i == at else None
        xa, xb = T[st.inA], T[st.inB] if st.inB else None
        if bad == "concat-swapped":
            assert xb is not None and xa.shape == xb.shape
            xa, xb = xb, xa
        x = xa if xb is None else torch.cat([xa, xb], 1)
        acc = _conv(l, x, P[_layer_keys(l)[0]])
        if bad == "shift-mod-8":
            assert l.cout > 8
            t = t[torch.arange(l.cout) % 8]
        r = fma32(acc, s.view(1, -1, 1, 1), t.view(1, -1, 1, 1))
        if l.relu:
            r = F.relu(r)
        if st.up:
            u = T[st.up]
            if bad == "lateral-row-stride":            # the coarse row taken at (oy >> 1) * Wo instead of (oy >> 1) * (Wo >> 1)
                Ho, Wo = r.shape[2:]
                oy, ox = torch.meshgrid(torch.arange(Ho), torch.arange(Wo), indexing="ij")
                idx = ((oy >> 1) * Wo + (ox >> 1)).clamp(max=(Ho // 2) * (Wo // 2) - 1)
                uu = u.reshape(u.shape[0], u.shape[1], -1)[:, :, idx.reshape(-1)].view(r.shape)
            else:
                uu = _up2(u)
            r = uu + r
        if bad == "tile-column-zero":
            assert r.shape[3] >= 64
            r = r.clone()
            r[..., 63] = 0.0
        T[st.out] = r
    return T


def fn_classes(case):
    """Remainder classes of the launches of a case against the 64 x 4 workgroup (of the input plane for the transposed layers), the
    8-channel output groups, and the channel-pair loop, as tags."""
    tags = set()
    for l, st in zip(fn_layers(case.c, case.arch), fn_steps(case.c, case.arch)):
        lvl = st.lin if l.transposed else st.lout
        h, w = case.H >> lvl, case.W >> lvl
        k = fn_kind(l)
        tags.add((k, "W<64" if w < 64 else "W=64" if w == 64 else "W=65" if w == 65 else "W>65"))
        tags.add((k, "H<4" if h < 4 else "H=4" if h == 4 else "H=5" if h == 5 else "H>5"))
        tags.add((k, "Cout%%8=%d" % (l.cout % 8)))
        tags.add((k, "Cin odd" if l.cin % 2 else "Cin even"))
        if st.inB:
            tags.add((k, "CA odd" if (l.cin - st.CB) % 2 else "CA even"))
    return tags


# ---- costreg ----------------------------------------------------------------------------------------------------------------------
# smvs_costreg_fwd (csrc/costreg.hip): 11 layers of 3 x 3 x 3 taps.  The same bound with n = 27 Cin (transposed: at most 8 taps of every
# input channel reach one output, n = 8 Cin) and the skip added after the ReLU as the lateral above.  Two of the kernels do not run one
# chain: the MFMA layers (conv3..conv6) split the input channels over 4 or 8 waves and the coarse transposed layers over 4, each wave
# a chain of n / KS products from 0, the partial sums then added one by one -- a product passes through n / KS + KS - 1 <= n roundings,
# so the constant stays (the matrix instruction adds its two products per step in order, csrc/mfma_conv.h).  The 62-column row kernel
# multiplies channel pairs with packed fused multiply-adds: one chain per output as before.
# cr_pack_bn_kernel folds the BatchNorm in FLOAT32 (the library is built without contraction): scale = gamma / sqrtf(var + 1e-5f),
# shift = beta - mean * scale, every operation rounded.
CrLayer = namedtuple("CrLayer", "name cin cout stride transposed bn relu")
CrStep = namedtuple("CrStep", "inp out skip lin lout")
CrCase = namedtuple("CrCase", "B C D H W")
CR_CASES = [CrCase(1, 8, 8, 8, 8), CrCase(2, 8, 8, 16, 72), CrCase(1, 32, 16, 8, 136), CrCase(1, 5, 8, 24, 8)]
CR_COT = 8


def cr_id(case):
    return "b%d-c%d-%dx%dx%d" % case


def cr_layers(C):
    t = [("conv0", C, 8, 1, 0), ("conv1", 8, 16, 2, 0), ("conv2", 16, 16, 1, 0), ("conv3", 16, 32, 2, 0), ("conv4", 32, 32, 1, 0),
         ("conv5", 32, 64, 2, 0), ("conv6", 64, 64, 1, 0), ("conv7", 64, 32, 2, 1), ("conv9", 32, 16, 2, 1), ("conv11", 16, 8, 2, 1)]
    return [CrLayer(*l, 1, 1) for l in t] + [CrLayer("prob", 8, 1, 1, 0, 0, 0)]


def cr_steps():
    return [CrStep("vol", "c0", None, 0, 0), CrStep("c0", "t1", None, 0, 1), CrStep("t1", "c2", None, 1, 1), CrStep("c2", "t3", None, 1, 2),
            CrStep("t3", "c4", None, 2, 2), CrStep("c4", "t5", None, 2, 3), CrStep("t5", "t6", None, 3, 3), CrStep("t6", "x7", "c4", 3, 2),
            CrStep("x7", "x9", "c2", 2, 1), CrStep("x9", "x11", "c0", 1, 0), CrStep("x11", "out", None, 0, 0)]


def mfma_conv_ok(CA, CB, Cout):
    cin = CA + CB
    return Cout in (32, 64, 128) and cin % 8 == 0 and CA % 2 == 0 and cin >= 8


def cr_use_mfma(l):
    return not l.transposed and mfma_conv_ok(l.cin, 0, l.cout)


def cr_accepts(B, C, D, H, W):
    if B < 1 or C < 1 or D < 8 or H < 8 or W < 8 or D % 8 or H % 8 or W % 8:
        return False
    return D * H // 4 + 1 <= 65535


def cr_workspace(B, D, H, W):
    """name -> (offset in floats, shape), total (cr_workspace of csrc/costreg.hip)"""
    o = 0
    lay = {}
    for name, ch, lvl in (("c0", 8, 0), ("t1", 16, 1), ("c2", 16, 1), ("t3", 32, 2), ("c4", 32, 2), ("t5", 64, 3), ("t6", 64, 3), ("x7", 32, 2),
                          ("x9", 16, 1), ("x11", 8, 0)):
        shape = (B, ch, D >> lvl, H >> lvl, W >> lvl)
        lay[name] = (o, shape)
        o += _round4(int(np.prod(shape)))
    return lay, o


def cr_packed_layout(C):
    """per layer (w, scale, shift, wm or None), total (cr_layout)"""
    o = 0
    lay = []
    for l in cr_layers(C):
        ncog = (l.cout + CR_COT - 1) // CR_COT
        wo = o; o += ncog * l.cin * 27 * CR_COT
        so = o; o += ncog * CR_COT
        to = o; o += ncog * CR_COT
        wm = None
        if cr_use_mfma(l):
            wm = o; o += (l.cin // 2) * 27 * ((l.cout + 31) // 32) * 64
        lay.append((wo, so, to, wm))
    return lay, o


def cr_param_names():
    """The 51 pointers of smvs_costreg_pack_weights as include/satmvs.h states them"""
    bn5 = (".conv.weight", ".bn.weight", ".bn.bias", ".bn.running_mean", ".bn.running_var")
    return [l + s for l in ("conv0", "conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "conv9", "conv11") for s in bn5] + ["prob.weight"]


def _cr_keys(l):
    return [l.name + s for s in (".conv.weight", ".bn.weight", ".bn.bias", ".bn.running_mean", ".bn.running_var")] if l.bn else [l.name + ".weight"]


@functools.lru_cache(maxsize=None)
def cr_params(C, seed=0):
    """name -> float32 CPU tensor; BatchNorm tensors as in fn_params"""
    g = torch.Generator().manual_seed(77 + 13 * C + seed)
    P = {}
    for i, l in enumerate(cr_layers(C)):
        keys = _cr_keys(l)
        wshape = ((l.cin, l.cout) if l.transposed else (l.cout, l.cin)) + (3, 3, 3)
        P[keys[0]] = torch.randn(wshape, generator=g) * (2.0 / (l.cin * (8 if l.transposed else 27))) ** 0.5
        if l.bn:
            sign = 1.0 - 2.0 * ((torch.arange(l.cout) + i) % 2)
            gamma = (0.5 + torch.rand(l.cout, generator=g)) * sign
            var = 0.5 + 1.5 * torch.rand(l.cout, generator=g)
            small, zero = (3 * i + 1) % l.cout, (5 * i + 2) % l.cout
            if zero == small:
                zero = (zero + 1) % l.cout
            var[small] = 1e-4
            gamma[small] = 0.02 * sign[small]
            gamma[zero] = 0.0
            P[keys[1]] = gamma
            P[keys[2]] = 0.5 * torch.randn(l.cout, generator=g)
            P[keys[3]] = 0.3 * torch.randn(l.cout, generator=g)
            P[keys[4]] = var
    assert sorted(P) == sorted(cr_param_names())
    return P


@functools.lru_cache(maxsize=None)
def cr_volume(case):
    g = torch.Generator().manual_seed(5 + case.B + 3 * case.C + 7 * case.D + 11 * case.H + 13 * case.W)
    return torch.randn((case.B, case.C, case.D, case.H, case.W), generator=g)


def fold_bn32(gamma, beta, mean, var):
    """cr_pack_bn_kernel: float32 throughout, every operation correctly rounded once (numpy: torch's vectorised float32 sqrt on the
    CPU is not correctly rounded in every element)"""
    g, b, m, v = [t.numpy().astype(np.float32) for t in (gamma, beta, mean, var)]
    s = g / np.sqrt(v + np.float32(1e-5))
    assert s.dtype == np.float32
    return torch.from_numpy(s), torch.from_numpy(b - m * s)


def cr_pack_reference(P, C):
    lay, total = cr_packed_layout(C)
    out = torch.zeros(total, dtype=torch.float32)
    for l, (wo, so, to, wm) in zip(cr_layers(C), lay):
        keys = _cr_keys(l)
        w = P[keys[0]]
        wc = (w.transpose(0, 1) if l.transposed else w).reshape(l.cout, l.cin, 27)          # [co][ci][tap]
        ncog = (l.cout + CR_COT - 1) // CR_COT
        wp = torch.zeros((ncog * CR_COT, l.cin, 27), dtype=torch.float32)
        wp[:l.cout] = wc
        out[wo:wo + wp.numel()] = wp.view(ncog, CR_COT, l.cin, 27).permute(0, 2, 3, 1).reshape(-1)
        s, t = torch.ones(ncog * CR_COT), torch.zeros(ncog * CR_COT)
        if l.bn:
            s[:l.cout], t[:l.cout] = fold_bn32(*[P[k] for k in keys[1:]])
        out[so:so + s.numel()] = s
        out[to:to + t.numel()] = t
        if wm is not None:
            # [channel pair][step p][cout tile][k-slot h][32]: kk = 2p + h in the (ci0 taps..., ci1 taps...) list of the pair
            nt = (l.cout + 31) // 32
            i = torch.arange((l.cin // 2) * 27 * nt * 64)
            j, h, t_, p, cip = i & 31, (i >> 5) & 1, (i >> 6) % nt, (i // (64 * nt)) % 27, i // (64 * nt * 27)
            kk = 2 * p + h
            ci, tap, co = 2 * cip + (kk >= 27).long(), torch.where(kk >= 27, kk - 27, kk), t_ * 32 + j
            out[wm:wm + i.numel()] = wc[co, ci, tap]
    return out


def cr_scale_shift(packed, C):
    lay, _ = cr_packed_layout(C)
    return [(packed[so:so + l.cout].clone(), packed[to:to + l.cout].clone()) for l, (wo, so, to, wm) in zip(cr_layers(C), lay)]


def _conv3(l, x, w):
    if l.transposed:
        return F.conv_transpose3d(x, w, stride=2, padding=1, output_padding=1)
    return F.conv3d(x, w, stride=l.stride, padding=1)


def cr_kind(l):
    if cr_use_mfma(l):
        return "mfma s%d" % l.stride
    return "convT3d" if l.transposed else "conv3d s%d" % l.stride


def cr_layer64(l, x, w, scale, shift, skip):
    xd, wd = x.double(), w.double()
    s, t = scale.double().view(1, -1, 1, 1, 1), shift.double().view(1, -1, 1, 1, 1)
    r = _conv3(l, xd, wd) * s + t
    if l.relu:
        r = F.relu(r)
    n = l.cin * (8 if l.transposed else 27)
    M = _conv3(l, xd.abs(), wd.abs()) * s.abs() + t.abs()
    bound = (n + 2) * U32 * M + (n + 2) * TINY * (1.0 + s.abs())
    if skip is not None:
        r = r + skip.double()
        bound = bound + U32 * (skip.double().abs() + M)
    return r, bound


def cr_judge(case, P, packed, T):
    """-> list over layers of (layer name, kernel kind, ratio, where)"""
    res = []
    for l, st, (s, t) in zip(cr_layers(case.C), cr_steps(), cr_scale_shift(packed, case.C)):
        ref, bound = cr_layer64(l, T[st.inp], P[_cr_keys(l)[0]], s, t, T[st.skip] if st.skip else None)
        assert T[st.out].shape == ref.shape, (l.name, T[st.out].shape, ref.shape)
        ratio, where = worst_ratio(T[st.out], ref, bound)
        res.append((l.name, cr_kind(l), ratio, where))
    return res


def cr_tensors(case, vol, ws, out):
    lay, total = cr_workspace(case.B, case.D, case.H, case.W)
    assert ws.numel() == total
    T = {"vol": vol, "out": out}
    for name, (o, shape) in lay.items():
        T[name] = ws[o:o + int(np.prod(shape))].view(shape)
    return T


CR_FAULTS = ("tile-column-zero", "shift-mod-8", "skip-from-input")


def cr_model32(case, P, packed, vol, fault=None, at=None):
    """A float32 CPU evaluation layer by layer; fault plants an error into layer index `at`: the last column of the first 62-column
    tile zero, the shift of channel j taken from j mod 8, the skip read from the layer's own input level (x7 for conv9's c2: the
    tensor of the same shape written just before)."""
    T = {"vol": vol}
    for i, (l, st, (s, t)) in enumerate(zip(cr_layers(case.C), cr_steps(), cr_scale_shift(packed, case.C))):
        bad = fault if i == at else None
        acc = _conv3(l, T[st.inp], P[_cr_keys(l)[0]])
        if bad == "shift-mod-8":
            assert l.cout > 8
            t = t[torch.arange(l.cout) % 8]
        r = fma32(acc, s.view(1, -1, 1, 1, 1), t.view(1, -1, 1, 1, 1))
        if l.relu:
            r = F.relu(r)
        if st.skip:
            sk = T[st.skip]
            if bad == "skip-from-input":
                other = {"c4": "t3", "c2": "t1", "c0": "x11"}[st.skip]
                sk = T[other] if other in T else torch.zeros_like(sk)
            r = sk + r
        if bad == "tile-column-zero":
            assert r.shape[-1] >= 62
            r = r.clone()
            r[..., 61] = 0.0
        T[st.out] = r
    return T


# ---- RED: packed parameters and workspace size ----------------------------------------------------------------------------------------
# smvs_red_pack_weights / smvs_red_workspace_bytes (csrc/red.hip: red_layout, red_workspace, red_chunk).
RedCase = namedtuple("RedCase", "B C H W")
RED_CASES = [RedCase(1, 8, 8, 8), RedCase(2, 8, 8, 72), RedCase(3, 32, 24, 136), RedCase(1, 5, 16, 64), RedCase(1, 8, 2048, 8)]
RED_HID = (8, 16, 32, 64)
RED_NSLOT = 64


def red_id(case):
    return "b%d-c%d-%dx%d" % case


def red_accepts(B, C, H, W):
    if B < 1 or C < 1 or H < 8 or W < 8 or H % 8 or W % 8:
        return False
    return (C + 8) * H * W * 4 < 2 ** 31


def red_chunk(B, C, H, W):
    ch = 8 if B * H * W <= 131072 else 4
    while ch > 1 and C * ch * H * W * 4 >= 2 ** 30:
        ch >>= 1
    return ch


def red_workspace_floats(B, C, H, W):
    CH = red_chunk(B, C, H, W)
    NSL = 2 * CH
    hw = [(H >> g) * (W >> g) for g in range(4)]
    o = 0
    for i, ech in enumerate((16, 32, 64)):
        o += _round4(B * ech * hw[i + 1] * NSL)
    for g in range(4):
        o += _round4(B * 2 * RED_HID[g] * hw[g]) + 2 * _round4(B * RED_HID[g] * hw[g]) + _round4(B * RED_HID[g] * hw[g] * NSL)
    for g in range(3):
        o += _round4(CH * B * RED_HID[g] * hw[g])
    return o + 2 * _round4(B * 4 * 3 * RED_NSLOT * 2 * 2)


def red_param_names():
    """The 48 pointers of smvs_red_pack_weights as include/satmvs.h states them"""
    names = [g + n for g in ("conv_gru1.", "conv_gru2.", "conv_gru3.", "conv_gru4.")
             for n in ("gate_conv.weight", "gate_conv.bias", "reset_gate_norm.weight", "reset_gate_norm.bias", "update_gate_norm.weight",
                       "update_gate_norm.bias", "output_conv.weight", "output_conv.bias", "output_norm.weight", "output_norm.bias")]
    return names + ["conv1.conv.weight", "conv2.conv.weight", "conv3.conv.weight", "upconv1.conv.weight", "upconv2.conv.weight",
                    "upconv3.conv.weight", "upconv2d.weight", "upconv2d.bias"]


@functools.lru_cache(maxsize=None)
def red_params(C, seed=0):
    """name -> float32 CPU tensor: every tensor random, the three norms of a cell distinct in weight and bias (their shapes are equal:
    with the defaults 1 / 0 a swap among them would change nothing)."""
    g = torch.Generator().manual_seed(4242 + 17 * C + seed)
    xin = (C, 16, 32, 64)
    P = {}
    for i, hc in enumerate(RED_HID):
        p = "conv_gru%d." % (i + 1)
        cin = xin[i] + hc
        P[p + "gate_conv.weight"] = torch.randn((2 * hc, cin, 3, 3), generator=g) / (9 * cin) ** 0.5
        P[p + "gate_conv.bias"] = 0.3 * torch.randn(2 * hc, generator=g)
        P[p + "output_conv.weight"] = torch.randn((hc, cin, 3, 3), generator=g) / (9 * cin) ** 0.5
        P[p + "output_conv.bias"] = 0.3 * torch.randn(hc, generator=g)
        for n in ("reset_gate_norm", "update_gate_norm", "output_norm"):
            P[p + n + ".weight"] = 1.0 + 0.5 * torch.randn(hc, generator=g)
            P[p + n + ".bias"] = 0.5 * torch.randn(hc, generator=g)
    for i, (ci, co) in enumerate(((C, 16), (16, 32), (32, 64))):
        P["conv%d.conv.weight" % (i + 1)] = torch.randn((co, ci, 3, 3), generator=g) * (2.0 / (9 * ci)) ** 0.5
    for i, (ci, co) in enumerate(((16, 8), (32, 16), (64, 32))):
        P["upconv%d.conv.weight" % (i + 1)] = torch.randn((ci, co, 3, 3), generator=g) * (2.0 / (2.25 * ci)) ** 0.5
    P["upconv2d.weight"] = torch.randn((8, 1, 3, 3), generator=g) / 72 ** 0.5
    P["upconv2d.bias"] = 0.3 * torch.randn(1, generator=g)
    assert sorted(P) == sorted(red_param_names())
    return P


def _pack9(w_co_ci_t, cout, cin):
    """[cout group][cin][tap][8], zero beyond cout; w as [co][ci][tap]"""
    ncog = (cout + 7) // 8
    wp = torch.zeros((ncog * 8, cin, 9), dtype=torch.float32)
    wp[:cout] = w_co_ci_t
    return wp.view(ncog, 8, cin, 9).permute(0, 2, 3, 1).reshape(-1)


def _pack9_mfma(w_co_ci_t, cout, cin):
    """mfma_pack_kernel, 9 taps: [channel pair][cout tile][k-slot h = channel of the pair][32][12], taps 9..11 zero"""
    nt = (cout + 31) // 32
    out = torch.zeros((cin // 2, nt, 2, 32, 12), dtype=torch.float32)
    out[..., :9] = w_co_ci_t.view(nt, 32, cin // 2, 2, 9).permute(2, 0, 3, 1, 4)
    return out.reshape(-1)


def red_pack_reference(P, C):
    """-> (packed float32, written bool): the buffer smvs_red_pack_weights must write and which floats of it the entry writes at all
    (the output convolution's bias owns 8 floats and has one)."""
    xin = (C, 16, 32, 64)
    parts, written = [], []

    def put(t, reserve=None):
        parts.append(t.reshape(-1).float())
        written.append(torch.ones(t.numel(), dtype=torch.bool))
        if reserve:
            parts.append(torch.zeros(reserve - t.numel()))
            written.append(torch.zeros(reserve - t.numel(), dtype=torch.bool))
    enc = ((C, 16), (16, 32), (32, 64))
    for i, (ci, co) in enumerate(enc):
        put(_pack9(P["conv%d.conv.weight" % (i + 1)].reshape(co, ci, 9), co, ci))
    for i, hc in enumerate(RED_HID):
        p = "conv_gru%d." % (i + 1)
        cin = xin[i] + hc
        put(_pack9(P[p + "gate_conv.weight"].reshape(2 * hc, cin, 9), 2 * hc, cin))
        put(P[p + "gate_conv.bias"])
        for n in ("reset_gate_norm", "update_gate_norm"):
            put(P[p + n + ".weight"]); put(P[p + n + ".bias"])
        put(_pack9(P[p + "output_conv.weight"].reshape(hc, cin, 9), hc, cin))
        put(P[p + "output_conv.bias"])
        put(P[p + "output_norm.weight"]); put(P[p + "output_norm.bias"])
    for i, (ci, co) in enumerate(((16, 8), (32, 16), (64, 32))):                    # ConvTranspose2d weight (cin, cout, 3, 3), taps kept
        put(_pack9(P["upconv%d.conv.weight" % (i + 1)].reshape(ci, co, 9).transpose(0, 1), co, ci))
    put(_pack9(P["upconv2d.weight"].reshape(8, 1, 9).transpose(0, 1).flip(2), 1, 8))  # stride 1: the correlation with flipped taps
    put(P["upconv2d.bias"], reserve=8)
    for i, (ci, co) in enumerate(enc):
        if mfma_conv_ok(ci, 0, co):
            put(_pack9_mfma(P["conv%d.conv.weight" % (i + 1)].reshape(co, ci, 9), co, ci))
    for i, hc in enumerate(RED_HID):
        p = "conv_gru%d." % (i + 1)
        cin = xin[i] + hc
        if mfma_conv_ok(xin[i], hc, 2 * hc):
            put(_pack9_mfma(P[p + "gate_conv.weight"].reshape(2 * hc, cin, 9), 2 * hc, cin))
        if mfma_conv_ok(xin[i], hc, hc):
            put(_pack9_mfma(P[p + "output_conv.weight"].reshape(hc, cin, 9), hc, cin))
    return torch.cat(parts), torch.cat(written)


# ---- RED: one plane step, stage by stage --------------------------------------------------------------------------------------------
# smvs_red_step_fwd keeps every stage of the plane in the workspace (ring buffers at slot 0), the GroupNorm partial sums included.  So
# the stages are judged one by one on what the GPU itself left there:
#   convolutions      encoder (stride 2, ReLU), gate and candidate convolutions (bias; job kinds 0 / 1 / 6 direct, 2 / 3 / 4 MFMA): a chain of
#                     n = 9 Cin products per output, split over 4 waves (kind 1) or over 2 / 4 waves of K (kinds 2 / 3) with the partial
#                     sums added afterwards -- never more than n roundings per product -- then the bias: (n + 2) u (A + |bias|), as
#                     conv_scene.bound_from.  Decoder: n = 4 Cin, ReLU, then the skip added: + u (|skip| + A).  Output: n = 72, bias.
#   statistics        per (sample, norm) S1 = sum r and S2 = sum r^2 over the 64 slots, against the float64 sums of the raw values found
#                     in the workspace.  Each value passes through the lane's float32 chain (8 values: kinds 0 and 1; 32: kind 6; 16: the
#                     MFMA epilogue; r^2 enters by fmaf) and 6 butterfly steps before float64 takes over: depth d = chain + 6,
#                     |dS1| <= (d + 1) u sum |r|, |dS2| <= (d + 1) u sum r^2.  The float64 part is counted too: a partial sum enters its
#                     slot by one atomic among at most n / 8 (every wave or workgroup that adds one holds 8 values or more), 3 additions
#                     join a workgroup's waves before it, and the 64 slots are added here: red_f64_depth(n) = n / 8 + 3 + 64
#                     additions of 2^-53 each, on the same magnitudes.  In terms of the variance this is the (d + 1) u (1 + mu^2 / var)
#                     of a float32 sum of squares: at |mean| / std = 30 the statistics are allowed ~900 times the relative error of
#                     centred ones, which is what the kernels' arithmetic can give -- see the README.
#   gate apply        z = fmaf((r - mean) * rstd, w, b), rh = sigmoid(z) * h, with mean and rstd recomputed in float64 from the GPU's own
#                     slots exactly as gn_coeffs does (eps = float32(1e-5), both rounded to float32; one ulp of each is allowed for
#                     the different order of the float64 slot sum): |dz| <= 3 u (|d s w| + |b|) + u (|mean s w| + |d s w|), d = r - mean;
#                     sigmoid by its derivative at the nearer end plus norm_scene.ACT_ALLOW; the product one rounding.
#   combine           u = sigmoid(z_u), y = tanh(z_o) likewise; h' = u h + (1 - u) y as four rounded operations (the library is built
#                     without contraction): E = eu |h| + u32 |u h| + (eu + u32) |y| + |1 - u| ey + u32 |(1 - u) y| + u32 |h'|, with a
#                     factor 1 + 2^-10 for the second-order terms.  The state and its snapshot for the decoder carry the same bits.
RED_SLACK = 1.0 + 2.0 ** -10


def red_job_kinds(case):
    """(stage, level) -> job kind of the 8 level-batched convolutions (conv_job of csrc/red.hip)"""
    B, C, H, W = case
    xin = (C, 16, 32, 64)
    kinds = {}
    for g, hc in enumerate(RED_HID):
        Ho, Wo = H >> g, W >> g
        for stage, cout in (("gate", 2 * hc), ("cand", hc)):
            if mfma_conv_ok(xin[g], hc, cout):
                units1 = -(-Wo // 32) * Ho * (cout // 32)
                kinds[(stage, g)] = 4 if units1 >= 1024 else 3 if units1 >= 512 else 2
                continue
            ncog, gx = -(-cout // 8), -(-Wo // 64)
            split = gx * -(-Ho // 4) * B * ncog < 512
            kinds[(stage, g)] = 1 if split else 6 if gx * -(-Ho // 4) * ncog >= 1024 else 0
    return kinds


RED_STAT_CHAIN = {0: 8, 1: 8, 6: 32, 2: 16, 3: 16, 4: 16}


def red_workspace(B, C, H, W):
    """name -> (offset in floats, shape) of every tensor of a single step (slot 0 of the rings), the offset of the first statistics
    buffer, and the total in floats"""
    CH = red_chunk(B, C, H, W)
    NSL = 2 * CH
    dims = [(H >> g, W >> g) for g in range(4)]
    o = 0
    lay = {}

    def take(name, shape, times=1):
        nonlocal o
        if name:
            lay[name] = (o, shape)
        o += _round4(int(np.prod(shape)) * times)
    for i, ech in enumerate((16, 32, 64)):
        take("e%d" % (i + 1), (B, ech) + dims[i + 1], NSL)
    for g, hc in enumerate(RED_HID):
        take("gates%d" % g, (B, 2 * hc) + dims[g])
        take("rh%d" % g, (B, hc) + dims[g])
        take("cand%d" % g, (B, hc) + dims[g])
        take("hsnap%d" % g, (B, hc) + dims[g], NSL)
    for g in range(3):
        take("sum%d" % g, (B, RED_HID[g]) + dims[g], CH)
    stats = o
    take(None, (B * 4 * 3 * RED_NSLOT * 2 * 2,))
    take(None, (B * 4 * 3 * RED_NSLOT * 2 * 2,))
    return lay, stats, o


def red_state_shapes(case):
    B, C, H, W = case
    return [(B, hc, H >> g, W >> g) for g, hc in enumerate(RED_HID)]


@functools.lru_cache(maxsize=None)
def red_inputs(case, seed=0):
    """-> (cost, [h0..h3]) float32: a variance plane and states as a running pred loop holds them (blends of tanh values)"""
    g = torch.Generator().manual_seed(99 + 7 * case.B + 3 * case.C + case.H + 5 * case.W + seed)
    cost = torch.randn((case.B, case.C, case.H, case.W), generator=g).abs()
    return cost, [torch.tanh(torch.randn(s, generator=g)) for s in red_state_shapes(case)]


def _conv2(x, w, stride=1):
    return F.conv2d(x, w, stride=stride, padding=1)


def _convT2(x, w):
    return F.conv_transpose2d(x, w, stride=2, padding=1, output_padding=1)


def red_f64_depth(n):
    """float64 additions a value of a norm group of n elements passes through at most: the atomics into its slot, the join of a
    workgroup's 4 waves, the sum of the 64 slots"""
    return -(-n // 8) + 3 + RED_NSLOT


def red_group_sums(raw, hc_groups):
    """raw (B, G * hc, h, w) float32 -> float64 (B, G, 4): S1, S2, sum |r|, sum r^2 per norm group"""
    B = raw.shape[0]
    r = raw.double().reshape(B, hc_groups, -1)
    return torch.stack([r.sum(2), (r * r).sum(2), r.abs().sum(2), (r * r).sum(2)], 2)


def red_coeffs(S1, S2, n):
    """gn_coeffs of csrc/red.hip on float64 sums: mean and rstd rounded to float32, as float64 numbers"""
    mu = S1 / n
    var = (S2 / n - mu * mu).clamp(min=0.0)
    eps = float(np.float32(1e-5))
    return mu.float().double(), (1.0 / torch.sqrt(var + eps)).float().double()


def _act(pre, Epre, act):
    """norm_scene.act_bound in torch: (y, bound) of sigmoid (1) / tanh (2) at pre +- Epre"""
    y = torch.sigmoid(pre) if act == 1 else torch.tanh(pre)
    v = (pre.abs() - Epre).clamp(min=0.0)
    e = torch.exp(-v) if act == 1 else torch.exp(-2.0 * v)
    L = (1.0 if act == 1 else 4.0) * e / ((1.0 + e) * (1.0 + e))
    return y, L * Epre + _N.ACT_ALLOW[act] * U32 * y.abs() + 4 * TINY


def _norm_pre(raw, mean, rstd, w, b):
    """z = fmaf((r - mean) * rstd, w, b) in float64 and its bound; mean, rstd (B,), w, b (hc,)"""
    m, s = mean.view(-1, 1, 1, 1), rstd.view(-1, 1, 1, 1)
    wv, bv = w.double().view(1, -1, 1, 1), b.double().view(1, -1, 1, 1)
    d = raw.double() - m
    dsw = (d * s * wv).abs()
    z = d * s * wv + bv
    return z, RED_SLACK * (3 * U32 * (dsw + bv.abs()) + U32 * ((m * s * wv).abs() + dsw)) + 4 * TINY


def red_stats_view(stats, B):
    """the first statistics buffer (float64, flat) -> per level (gates (B, 2, 64, 2), output (B, 64, 2))"""
    out = []
    per = B * 3 * RED_NSLOT * 2
    for g in range(4):
        blk = stats[g * per:(g + 1) * per]
        out.append((blk[:B * 2 * RED_NSLOT * 2].view(B, 2, RED_NSLOT, 2), blk[B * 2 * RED_NSLOT * 2:].view(B, RED_NSLOT, 2)))
    return out


def red_judge(case, P, T):
    """T: "cost", "h0".."h3" (states before), "state0".."state3" (after), "out", "stats" (float64, flat) and the workspace tensors of
    red_workspace.  -> list of (stage name, kind label, ratio, where)."""
    B, C, H, W = case
    xin = (C, 16, 32, 64)
    kinds = red_job_kinds(case)
    res = []

    def conv_check(name, label, got, ref, A, n, bias=None, extra=None):
        m = A if bias is None else A + bias.double().abs().view(1, -1, 1, 1)
        bound = (n + 2) * U32 * m + n * TINY
        if extra is not None:
            bound = bound + extra
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        ratio, where = worst_ratio(got, ref, bound)
        res.append((name, label, ratio, where))

    # encoder
    x = -T["cost"].double()
    for i in range(3):
        w = P["conv%d.conv.weight" % (i + 1)].double()
        got = T["e%d" % (i + 1)]
        conv_check("conv%d" % (i + 1), "encoder", got, F.relu(_conv2(x, w, 2)), _conv2(x.abs(), w.abs(), 2), 9 * w.shape[1])
        x = got.double()
    sv = red_stats_view(T["stats"], B)
    for g, hc in enumerate(RED_HID):
        p = "conv_gru%d." % (g + 1)
        xg = -T["cost"].double() if g == 0 else T["e%d" % g].double()
        h = T["h%d" % g].double()
        n_hw = hc * (H >> g) * (W >> g)
        # gate convolution and its two statistics
        w, b = P[p + "gate_conv.weight"].double(), P[p + "gate_conv.bias"]
        cat = torch.cat([xg, h], 1)
        gates = T["gates%d" % g]
        k = kinds[("gate", g)]
        conv_check("gate%d" % g, "job kind %d" % k, gates, _conv2(cat, w) + b.double().view(1, -1, 1, 1), _conv2(cat.abs(), w.abs()), 9 * w.shape[1], b)
        sums = red_group_sums(gates, 2)
        got = sv[g][0].sum(2)                                              # (B, 2, 2)
        d = RED_STAT_CHAIN[k] + 6
        for j, nm in ((0, "S1"), (1, "S2")):
            bound = ((d + 1) * U32 + red_f64_depth(n_hw) * 2.0 ** -53) * sums[:, :, 2 + j] + TINY
            ratio, where = worst_ratio(got[:, :, j], sums[:, :, j], bound)
            res.append(("gate%d %s" % (g, nm), "stats kind %d" % k, ratio, where))
        mr, sr = red_coeffs(got[:, 0, 0], got[:, 0, 1], n_hw)
        mu, su = red_coeffs(got[:, 1, 0], got[:, 1, 1], n_hw)
        # gate apply
        z, Ez = _norm_pre(gates[:, :hc], mr, sr, P[p + "reset_gate_norm.weight"], P[p + "reset_gate_norm.bias"])
        r, Er = _act(z, Ez, 1)
        ref = r * h
        bound = RED_SLACK * (Er * h.abs() + U32 * ref.abs()) + TINY
        ratio, where = worst_ratio(T["rh%d" % g], ref, bound)
        res.append(("apply%d" % g, "gate apply", ratio, where))
        # candidate convolution and its statistics
        w, b = P[p + "output_conv.weight"].double(), P[p + "output_conv.bias"]
        cat = torch.cat([xg, T["rh%d" % g].double()], 1)
        cand = T["cand%d" % g]
        k = kinds[("cand", g)]
        conv_check("cand%d" % g, "job kind %d" % k, cand, _conv2(cat, w) + b.double().view(1, -1, 1, 1), _conv2(cat.abs(), w.abs()), 9 * w.shape[1], b)
        sums = red_group_sums(cand, 1)
        goto = sv[g][1].sum(1)                                             # (B, 2)
        d = RED_STAT_CHAIN[k] + 6
        for j, nm in ((0, "S1"), (1, "S2")):
            bound = ((d + 1) * U32 + red_f64_depth(n_hw) * 2.0 ** -53) * sums[:, 0, 2 + j] + TINY
            ratio, where = worst_ratio(goto[:, j], sums[:, 0, j], bound)
            res.append(("cand%d %s" % (g, nm), "stats kind %d" % k, ratio, where))
        mo, so = red_coeffs(goto[:, 0], goto[:, 1], n_hw)
        # combine
        zu, Ezu = _norm_pre(gates[:, hc:], mu, su, P[p + "update_gate_norm.weight"], P[p + "update_gate_norm.bias"])
        zo, Ezo = _norm_pre(cand, mo, so, P[p + "output_norm.weight"], P[p + "output_norm.bias"])
        u, Eu = _act(zu, Ezu, 1)
        y, Ey = _act(zo, Ezo, 2)
        ref = u * h + (1.0 - u) * y
        bound = RED_SLACK * (Eu * h.abs() + U32 * (u * h).abs() + (Eu + U32) * y.abs() + (1.0 - u).abs() * Ey + U32 * ((1.0 - u) * y).abs() + U32 * ref.abs()) + TINY
        ratio, where = worst_ratio(T["state%d" % g], ref, bound)
        res.append(("combine%d" % g, "combine", ratio, where))
        same = torch.equal(T["state%d" % g].view(torch.int32), T["hsnap%d" % g].view(torch.int32))
        res.append(("hsnap%d" % g, "snapshot", 0.0 if same else float("inf"), ()))
    # decoder
    src = T["hsnap3"]
    for g in (3, 2, 1):
        w = P["upconv%d.conv.weight" % g].double()
        skip = T["hsnap%d" % (g - 1)].double()
        A = _convT2(src.double().abs(), w.abs())
        conv_check("upconv%d" % g, "decoder", T["sum%d" % (g - 1)], F.relu(_convT2(src.double(), w)) + skip, A, 4 * w.shape[0], extra=U32 * (skip.abs() + A))
        src = T["sum%d" % (g - 1)]
    w, b = P["upconv2d.weight"].double(), P["upconv2d.bias"]
    s0 = T["sum0"].double()
    ref = F.conv_transpose2d(s0, w, stride=1, padding=1) + b.double().view(1, -1, 1, 1)
    conv_check("upconv2d", "output", T["out"], ref, F.conv_transpose2d(s0.abs(), w.abs(), stride=1, padding=1), 72, b)
    return res


def red_tensors(case, cost, h_old, ws, states, out):
    """The dict red_judge takes from the workspace read back flat (float32), the states after the call and reg_out"""
    lay, stats, total = red_workspace(*case)
    assert ws.numel() == total
    T = {"cost": cost, "out": out}
    for g in range(4):
        T["h%d" % g], T["state%d" % g] = h_old[g], states[g]
    for name, (o, shape) in lay.items():
        T[name] = ws[o:o + int(np.prod(shape))].view(shape)
    T["stats"] = ws[stats:stats + case.B * 4 * 3 * RED_NSLOT * 2 * 2].clone().view(torch.float64)
    return T


def _sums32(raw, groups):
    """S1 and S2 per (sample, norm group) summed in float32 (torch's blocked pairwise sum), as float64 (B, G, 2)"""
    r = raw.reshape(raw.shape[0], groups, -1)
    return torch.stack([r.sum(2), (r * r).sum(2)], 2).double()


RED_FAULTS = ("stats-swapped", "affine-swapped", "stats-of-sample-0", "hsnap-stale", "skip-from-old-state", "update-inverted")


def red_model32(case, P, cost, h_old, fault=None, at=0):
    """A float32 CPU evaluation of the step, stage by stage, leaving what the kernels leave (the statistics as float64 sums of its own
    raw values in slot 0).  fault plants an error at level `at`."""
    B, C, H, W = case
    T = {"cost": cost}
    x = -cost
    for i in range(3):
        x = F.relu(_conv2(x, P["conv%d.conv.weight" % (i + 1)], 2))
        T["e%d" % (i + 1)] = x
    stats = torch.zeros(4 * B * 3 * RED_NSLOT * 2, dtype=torch.float64)
    sv = red_stats_view(stats, B)
    for g, hc in enumerate(RED_HID):
        bad = fault if g == at else None
        p = "conv_gru%d." % (g + 1)
        xg = -cost if g == 0 else T["e%d" % g]
        h = h_old[g]
        T["h%d" % g] = h
        n_hw = hc * (H >> g) * (W >> g)
        gates = _conv2(torch.cat([xg, h], 1), P[p + "gate_conv.weight"]) + P[p + "gate_conv.bias"].view(1, -1, 1, 1)
        T["gates%d" % g] = gates
        sums = _sums32(gates, 2)
        sv[g][0][:, :, 0, :] = sums[:, :, :2]
        cr = red_coeffs(sums[:, 0, 0], sums[:, 0, 1], n_hw)
        cu = red_coeffs(sums[:, 1, 0], sums[:, 1, 1], n_hw)
        if bad == "stats-swapped":
            cr, cu = cu, cr
        if bad == "stats-of-sample-0":
            assert B > 1
            cr = tuple(t[:1].expand(B).clone() for t in cr)
        names = ["reset_gate_norm", "update_gate_norm"]
        if bad == "affine-swapped":
            names.reverse()

        def norm(raw, coef, nm):
            d = raw - coef[0].float().view(-1, 1, 1, 1)
            return fma32(d * coef[1].float().view(-1, 1, 1, 1), P[p + nm + ".weight"].view(1, -1, 1, 1), P[p + nm + ".bias"].view(1, -1, 1, 1))
        rh = torch.sigmoid(norm(gates[:, :hc], cr, names[0])) * h
        T["rh%d" % g] = rh
        cand = _conv2(torch.cat([xg, rh], 1), P[p + "output_conv.weight"]) + P[p + "output_conv.bias"].view(1, -1, 1, 1)
        T["cand%d" % g] = cand
        so = _sums32(cand, 1)
        sv[g][1][:, 0, :] = so[:, 0, :2]
        co = red_coeffs(so[:, 0, 0], so[:, 0, 1], n_hw)
        u = torch.sigmoid(norm(gates[:, hc:], cu, names[1]))
        y = torch.tanh(norm(cand, co, "output_norm"))
        if bad == "update-inverted":
            u = 1.0 - u
        new = u * h + (1.0 - u) * y
        T["state%d" % g] = new
        T["hsnap%d" % g] = h.clone() if bad == "hsnap-stale" else new
    src = T["hsnap3"]
    for g in (3, 2, 1):
        skip = T["h%d" % (g - 1)] if (fault == "skip-from-old-state" and at == g - 1) else T["hsnap%d" % (g - 1)]
        src = F.relu(_convT2(src, P["upconv%d.conv.weight" % g])) + skip
        T["sum%d" % (g - 1)] = src
    T["out"] = F.conv_transpose2d(src, P["upconv2d.weight"], stride=1, padding=1) + P["upconv2d.bias"].view(1, -1, 1, 1)
    T["stats"] = stats
    return T


RED_HOT = 30.0                                 # |mean| / std of the raw gate and candidate outputs of a "hot" scene
RED_HOT_CASES = [RedCase(1, 8, 2048, 8), RedCase(3, 32, 24, 136)]


@functools.lru_cache(maxsize=None)
def red_params_hot(case):
    """red_params with one bias per convolution of every level moved so that the raw reset, update and candidate outputs of this case's
    inputs have mean / std = 30 over the batch (a constant added to a group moves its mean and nothing else: GroupNorm removes it
    again, so the reset gate, and with it the candidate's spread, stay as they were)."""
    P = dict(red_params(case.C))
    cost, h = red_inputs(case)
    T = red_model32(case, P, cost, h)
    for g, hc in enumerate(RED_HID):
        p = "conv_gru%d." % (g + 1)
        gb = P[p + "gate_conv.bias"].clone()
        for j in range(2):
            half = T["gates%d" % g][:, j * hc:(j + 1) * hc].double()
            gb[j * hc:(j + 1) * hc] += float(RED_HOT * half.std() - half.mean())
        P[p + "gate_conv.bias"] = gb
        c = T["cand%d" % g].double()
        P[p + "output_conv.bias"] = P[p + "output_conv.bias"] + float(RED_HOT * c.std() - c.mean())
    return P


def red_raw64(case, P, cost, h_old):
    """The raw reset / update (gates) and candidate outputs of one step in float64 throughout: "gates0".."gates3", "cand0".."cand3" """
    x = -cost.double()
    e = []
    for i in range(3):
        x = F.relu(_conv2(x, P["conv%d.conv.weight" % (i + 1)].double(), 2))
        e.append(x)
    eps = float(np.float32(1e-5))
    R = {}
    for g, hc in enumerate(RED_HID):
        p = "conv_gru%d." % (g + 1)
        xg = -cost.double() if g == 0 else e[g - 1]
        h = h_old[g].double()
        gates = _conv2(torch.cat([xg, h], 1), P[p + "gate_conv.weight"].double()) + P[p + "gate_conv.bias"].double().view(1, -1, 1, 1)
        r = F.group_norm(gates[:, :hc], 1, P[p + "reset_gate_norm.weight"].double(), P[p + "reset_gate_norm.bias"].double(), eps)
        rh = torch.sigmoid(r) * h
        R["gates%d" % g] = gates
        R["cand%d" % g] = _conv2(torch.cat([xg, rh], 1), P[p + "output_conv.weight"].double()) + P[p + "output_conv.bias"].double().view(1, -1, 1, 1)
    return R
