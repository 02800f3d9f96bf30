"""Cases, parameters, the float64 reference and the judge for the hand-written autograd layer of the RED regulariser's training path
(satmvs_amd/modules/train_fns.py; ConvGRUCell2 and RED_Regularization of satmvs_amd/modules/module.py): what composes the HIP kernels
into a gradient -- the one-node cell, the deferred weight gradients, the layer node, the cell forms and the loop forms.  Shared by
tests/test_red_train_cpu.py (which proves without a GPU that the judge accepts a correct float32 evaluation and rejects swapped norm
parameters and detached states) and tests/test_red_train_gpu.py.  Importable without a GPU; nothing here launches a kernel.

The criterion.  Per tensor t of a run (the output, the gradient of every input, the gradient of every parameter)
    e(t) = max|t - t64| / max|t64|        and the same with root mean squares,
t64 from reference(): a float64 deep copy of the module on the CPU, fed the float32 bits of the inputs, loss = sum(out * weight).
The float32 composite of torch's own operators (the GPU's, SW.train_composite_mask = 511) gives e_base(t) the same way.  A native path
passes when, for both measures and every tensor,
    e_native(t) <= 4 max(e_base(t), median over the run's tensors of e_base).
4 is the project's rule for a native float32 path against the float32 composite it replaces (profiles/net_bound_ratios.txt).  The
median is a floor: the composite's error in a one-element tensor (upconv2d.bias) can be near zero by accident.  No absolute tolerance
appears anywhere.

Every GroupNorm of every case carries random gamma and beta, the three norms of a cell visibly different ones: with the defaults
(1, 0) a swap of two norms' parameters, or the wrong gamma in a kernel's apply pass, changes no bit (test_red_train_cpu.py states
that blind spot as a test)."""
import copy
import functools
import math
from collections import namedtuple

import torch

LIMIT = 4.0

# kind "cell": ConvGRUCell2(C, ch) run for `D` chained steps on x (D, B, C, H, W) and h (B, ch, H, W); kind "red": RED_Regularization(C) on a
# volume (B, C, D, H, W)
Case = namedtuple("Case", "id kind B C ch D H W")

CASES = [
    Case("cell-1", "cell", 1, 8, 8, 2, 8, 12),          # one-node cell; the dh of step 2 flows into step 1
    Case("cell-odd", "cell", 2, 32, 8, 1, 7, 9),        # piecewise cell (batch 2); HW not a multiple of 4
    Case("cell-64", "cell", 1, 64, 64, 1, 8, 8),        # MFMA forward and adjoint in the one-node cell
    Case("red-d1", "red", 1, 8, 0, 1, 16, 24),          # no plane views, no sink: weight gradients launched per call
    Case("red-d2", "red", 1, 16, 0, 2, 16, 24),         # smallest sink; level 4 is 2 x 3
    Case("red-wide", "red", 1, 16, 0, 3, 24, 72),       # W > 64: two weight-gradient column strips, ragged convolution tile
    Case("red-b2", "red", 2, 8, 0, 3, 16, 24),          # piecewise cells inside the sink; two samples per entry of the list launch
    Case("red-32", "red", 1, 32, 0, 4, 16, 16),         # stage-1 channel count
]
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]
# With one plane the state is zero throughout: r multiplies h = 0, so nothing reaches the reset gate's norm.  These gradients are zero by
# structure, in float64 and in any correct float32 path alike; they are held to exactly zero, and every other tensor has to be non-zero.
ZERO_BY_STRUCTURE = {"red-d1": tuple("conv_gru%d.reset_gate_norm.%s" % (g, t) for g in (1, 2, 3, 4) for t in ("weight", "bias"))}

SWITCH_FORMS = [("train_streams", False), ("train_loop_pipeline", False), ("train_defer_wgrad", False), ("train_plane_views", False),
                ("train_composite_mask", 1), ("train_composite_mask", 2), ("train_composite_mask", 4), ("train_composite_mask", 8),
                ("train_composite_mask", 16), ("train_composite_mask", 32)]
SAME_OUTPUT_BITS = ("train_streams", "train_loop_pipeline", "train_defer_wgrad", "train_plane_views")     # forms that only move or regroup launches
FROZEN = ("conv_gru2.gate_conv.weight", "conv1.conv.weight", "conv_gru1.output_norm.weight", "conv_gru1.output_norm.bias",
          "conv_gru2.output_norm.weight", "conv_gru2.output_norm.bias", "conv_gru3.output_norm.weight", "conv_gru3.output_norm.bias",
          "conv_gru4.output_norm.weight", "conv_gru4.output_norm.bias")


def form_id(form):
    return "%s=%s" % (form[0].replace("train_", ""), form[1])


def randomise(net, seed):
    """Every *_norm.weight from U(0.5, 1.5), every *_norm.bias from N(0, 0.3), every convolution bias from N(0, 0.1): one seeded CPU
    generator, so that a GPU copy and a CPU copy of `net` carry the same bits.  Returns net."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if "_norm." in name:
                v = 0.5 + torch.rand(p.shape, generator=g) if name.endswith(".weight") else 0.3 * torch.randn(p.shape, generator=g)
            elif name.endswith(".bias"):
                v = 0.1 * torch.randn(p.shape, generator=g)
            else:
                continue
            p.copy_(v.to(device=p.device, dtype=p.dtype))
    return net


def _seed(case):
    return 1000 + 97 * IDS.index(case.id)


def module(case, randomised=True, eps=None):
    """The case's module on the CPU in float32 (a fresh one per call); eps: one value for all norms, or (reset, update, output)."""
    from satmvs_amd.modules.module import ConvGRUCell2, RED_Regularization
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(_seed(case))
        net = ConvGRUCell2(case.C, case.ch, 3) if case.kind == "cell" else RED_Regularization(case.C)
    if randomised:
        randomise(net, _seed(case) + 1)
    if eps is not None:
        three = eps if isinstance(eps, tuple) else (eps, eps, eps)
        for name, m in net.named_modules():
            for tail, e in zip(("reset_gate_norm", "update_gate_norm", "output_norm"), three):
                if name.endswith(tail):
                    m.eps = e
    return net


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> (inputs, weight): float32 CPU tensors; inputs = (volume,) or (x, h).  The weight on the output is random (a loss that reaches
    every element of every plane with its own factor)."""
    g = torch.Generator().manual_seed(_seed(case) + 2)
    if case.kind == "cell":
        ins = (torch.randn((case.D, case.B, case.C, case.H, case.W), generator=g), torch.randn((case.B, case.ch, case.H, case.W), generator=g))
        weight = torch.randn((case.B, case.ch, case.H, case.W), generator=g)
    else:
        ins = (torch.randn((case.B, case.C, case.D, case.H, case.W), generator=g).abs(),)          # a variance volume is non-negative
        weight = torch.randn((case.B, case.D, case.H, case.W), generator=g)
    return ins, weight


def input_names(net):
    return ("dx", "dh") if type(net).__name__ == "ConvGRUCell2" else ("dvol",)


def forward(net, leaves, detach_states=False):
    """The module on its inputs: the cell for x.shape[0] chained steps from h, or the regulariser on the volume.  detach_states: the
    regulariser's plain plane loop with the states cut between planes (a planted fault of the CPU tests)."""
    if type(net).__name__ == "ConvGRUCell2":
        x, h = leaves
        for k in range(x.shape[0]):
            h = net(x[k], h)[0]
        return h
    vol, = leaves
    if not detach_states:
        return net(vol)
    b, _, d_num, hh, ww = vol.shape
    s = net.initial_states(b, hh, ww, vol.device, vol.dtype)
    outs = []
    for d in range(d_num):
        reg, *s = net.step(vol[:, :, d], *s)
        s = [t.detach() for t in s]
        outs.append(reg)
    return torch.stack(outs, dim=1).squeeze(2)


def collect(net, out, leaves):
    """name -> tensor (detached, on the CPU, its own dtype; None for a parameter without gradient): "out", the input gradients, then
    every parameter's gradient by name"""
    T = {"out": out.detach().cpu()}
    for name, leaf in zip(input_names(net), leaves):
        T[name] = leaf.grad.detach().cpu().clone()
    for name, p in net.named_parameters():
        T[name] = None if p.grad is None else p.grad.detach().cpu().clone()
    return T


def run(net, ins, weight, backwards=1, **kw):
    """One forward and `backwards` backward passes of sum(out * weight) through the same graph, from cleared gradients; ins and weight
    are moved to the module's device and dtype.  -> collect()"""
    p0 = next(net.parameters())
    leaves = [t.detach().to(device=p0.device, dtype=p0.dtype).clone().requires_grad_(True) for t in ins]
    w = weight.to(device=p0.device, dtype=p0.dtype)
    net.zero_grad(set_to_none=True)
    out = forward(net, leaves, **kw)
    loss = (out * w).sum()
    for k in range(backwards):
        loss.backward(retain_graph=k + 1 < backwards)
    return collect(net, out, leaves)


class no_native_launch:
    """Asserts that no native call is made inside the block: the float64 CPU module has to take torch's composite everywhere."""

    def __enter__(self):
        from satmvs_amd import _lib
        self.lib, self.saved, self.names = _lib, _lib.launch, []
        _lib.launch = lambda dev, name, *a: self.names.append(name) or self.saved(dev, name, *a)
        return self

    def __exit__(self, *exc):
        self.lib.launch = self.saved
        assert not self.names, "the float64 reference made native calls: %s" % sorted(set(self.names))
        return False


def reference(net, vol, weight):
    """The float64 run: a deep copy of `net` (its requires_grad flags and norm eps included) in float64 on the CPU, on the float32 bits
    of `vol` (a tensor or a tuple of tensors, from any device) cast up.  -> (out, input gradient(s), {name: grad}), float64."""
    ins = vol if isinstance(vol, (tuple, list)) else (vol,)
    net64 = copy.deepcopy(net).to("cpu").double()
    for (_, p), (_, q) in zip(net.named_parameters(), net64.named_parameters()):
        q.requires_grad_(p.requires_grad)
    with no_native_launch():
        T = run(net64, [t.detach().cpu() for t in ins], weight.detach().cpu())
    assert all(t is None or t.dtype is torch.float64 for t in T.values())
    dins = tuple(T[n] for n in input_names(net))
    grads = {n: T[n] for n, _ in net.named_parameters()}
    return T["out"], (dins[0] if len(dins) == 1 else dins), grads


def as_set(net, out, dins, grads):
    """The triple of reference() as the name -> tensor set that run() returns and judge() takes"""
    T = {"out": out}
    T.update(zip(input_names(net), dins if isinstance(dins, tuple) else (dins,)))
    T.update(grads)
    return T


@functools.lru_cache(maxsize=None)
def want(case):
    """The float64 set of a case, computed once and shared (callers leave it unchanged)"""
    net = module(case)
    ins, weight = inputs(case)
    T = as_set(net, *reference(net, ins, weight))
    for name, t in T.items():
        zero = name in ZERO_BY_STRUCTURE.get(case.id, ())
        assert t is not None and (float(t.abs().max()) > 0.0) != zero, "%s: %s is %szero in float64" % (case.id, name, "" if not zero else "not ")
    return T


def errors(got, want64):
    """name -> (e_max, e_rms) of got against want64; a tensor that must be None (frozen parameter) is asserted None and left out; a
    non-finite element counts as an infinite error; a tensor that is zero in float64 (ZERO_BY_STRUCTURE) has error 0 when every
    element of got is zero and an infinite one otherwise"""
    E = {}
    assert set(got) == set(want64), sorted(set(got) ^ set(want64))
    for name, w in want64.items():
        g = got[name]
        if w is None:
            assert g is None, "%s has a gradient where the reference has none" % name
            continue
        assert g is not None, "%s has no gradient" % name
        assert tuple(g.shape) == tuple(w.shape), (name, tuple(g.shape), tuple(w.shape))
        d = (g.detach().cpu().double() - w).abs()
        d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
        wmax, wrms = float(w.abs().max()), math.sqrt(float((w * w).mean()))
        if wmax == 0.0:
            E[name] = (0.0, 0.0) if float(d.max()) == 0.0 else (float("inf"), float("inf"))
            continue
        E[name] = (float(d.max()) / wmax, math.sqrt(float((d * d).mean())) / wrms)
    return E


def _median(v):
    v = sorted(v)
    n = len(v)
    return v[n // 2] if n % 2 else 0.5 * (v[n // 2 - 1] + v[n // 2])


def judge(got, want64, base):
    """-> (ratios, (worst ratio, its tensor)): per tensor the larger, over the two measures, of e_got / max(e_base, median of e_base).
    The run passes when the worst ratio is <= LIMIT."""
    eg, eb = errors(got, want64), errors(base, want64)
    ratios = {}
    for k in (0, 1):
        med = _median([e[k] for e in eb.values()])
        assert med > 0.0 and math.isfinite(med), "the composite's median error is %r: nothing to measure against" % med
        for name in eg:
            r = eg[name][k] / max(eb[name][k], med)
            ratios[name] = max(ratios.get(name, 0.0), r)
    worst = max(ratios, key=ratios.get)
    return ratios, (ratios[worst], worst)


def failing(ratios):
    return sorted(n for n, r in ratios.items() if not r <= LIMIT)


def scaled(T, factor, but=("out",)):
    """T with every gradient multiplied by factor (a power of two: exact)"""
    return {n: (t if t is None or n in but else t * factor) for n, t in T.items()}
