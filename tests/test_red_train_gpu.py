"""The hand-written autograd layer of the RED regulariser's training path (satmvs_amd/modules/train_fns.py, ConvGRUCell2 and
RED_Regularization of satmvs_amd/modules/module.py) on the MI355X against float64 autograd, form by form (tests/red_train_scene.py):
every case, every switch setting, frozen parameters, a second backward, accumulation over two forwards, norm eps away from the
default, a side stream -- and planted faults in single native calls, which the judge has to reject.  The measure is the float32
composite of torch's own operators on the same GPU: a native form may be at most four times as far from float64 as that."""
import contextlib
import ctypes
import gc
import os
import weakref

import pytest
import torch

import red_train_scene as S

pytestmark = pytest.mark.gpu

RATIOS = {}             # ("case" | "form" | "fault" | ..., id) -> text of one line of profiles/red_train_ratios.txt
_NETS, _BASE, _GOT = {}, {}, {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("these tests need the MI355X")
    from satmvs_amd import build
    build.build()
    torch.backends.cudnn.benchmark = False
    return torch.device("cuda:0")


@contextlib.contextmanager
def switch(name, value):
    from satmvs_amd.modules.switches import SW
    saved = getattr(SW, name)
    setattr(SW, name, value)
    try:
        yield
    finally:
        setattr(SW, name, saved)


def gpu_net(case, dev):
    if case.id not in _NETS:
        _NETS[case.id] = S.module(case).to(dev)
    return _NETS[case.id]


def run(net, case, **kw):
    ins, weight = S.inputs(case)
    T = S.run(net, ins, weight, **kw)
    torch.cuda.synchronize()
    return T


def composite(net, case, **kw):
    """the float32 composite of torch's operators on the GPU: the measure, none of it code under test"""
    with switch("train_composite_mask", 511):
        return run(net, case, **kw)


def base(case, dev):
    if case.id not in _BASE:
        _BASE[case.id] = composite(gpu_net(case, dev), case)
    return _BASE[case.id]


def native(case, dev):
    """the default switches' result of a case, computed once"""
    if case.id not in _GOT:
        _GOT[case.id] = run(gpu_net(case, dev), case)
    return _GOT[case.id]


def judged(key, got, want, basis):
    """judge, print every figure, record the worst, then assert"""
    ratios, (worst, name) = S.judge(got, want, basis)
    print("ratios %s: worst %.3f %s | %s" % (key, worst, name, " ".join("%s=%.2f" % (n, r) for n, r in sorted(ratios.items(), key=lambda kv: -kv[1])[:6])))
    RATIOS[key] = "worst %8.3f  %s" % (worst, name)
    assert worst <= S.LIMIT, (key, name, worst, S.failing(ratios))
    return ratios


class Spy:
    """satmvs_amd._lib.launch with every call's name kept and, optionally, the arguments of some calls rewritten"""

    def __init__(self, monkeypatch, rewrite=None):
        from satmvs_amd.modules import train_fns
        self.names, self.hits, self.args = [], 0, {}
        inner = train_fns._lib.launch

        def wrapper(dev, name, *a):
            self.names.append(name)
            self.args.setdefault(name, a)
            if rewrite is not None:
                b = rewrite(name, list(a))
                if b is not None:
                    self.hits += 1
                    a = b
            return inner(dev, name, *a)
        monkeypatch.setattr(train_fns._lib, "launch", wrapper)


# ---- 1. every case ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.CASES, ids=S.IDS)
def test_every_case_against_float64(dev, case, monkeypatch):
    """Default switches: output, input gradients and every parameter gradient inside the criterion -- and the form the case is there
    for is the one that ran."""
    spy = Spy(monkeypatch)
    got = _GOT[case.id] = run(gpu_net(case, dev), case)
    assert ("smvs_groupnorm1_pair_fwd_mul" in spy.names) == (case.B == 1)          # the one-node cell
    assert ("smvs_groupnorm1_pair_fwd" in spy.names) == (case.B > 1)               # the piecewise cell
    if case.kind == "red":
        assert "smvs_conv3x3_wgrad_list" in spy.names and "smvs_conv3x3_wgrad_strided" not in spy.names
    judged(("case", case.id), got, S.want(case), base(case, dev))


def test_sink_sums_all_planes_in_one_launch_per_layer(dev, monkeypatch):
    """red-d2: 8 cell layers + 7 plain layers, each one smvs_conv3x3_wgrad_list launch over both planes; red-d1 (no plane views):
    one launch per layer call with one entry."""
    for cid, n_want in (("red-d2", 2), ("red-d1", 1)):
        counts = []

        def look(name, a):
            if name == "smvs_conv3x3_wgrad_list":
                counts.append(a[3])
            return None
        Spy(monkeypatch, look)
        run(gpu_net(S.BY_ID[cid], dev), S.BY_ID[cid])
        monkeypatch.undo()
        assert counts == [n_want] * 15, (cid, counts)


# ---- 2. every form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", S.SWITCH_FORMS, ids=[S.form_id(f) for f in S.SWITCH_FORMS])
@pytest.mark.parametrize("cid", ["red-d2", "red-b2"])
def test_every_form_against_float64(dev, cid, form):
    """One switch away from the default at a time.  The forms that only move launches to other streams or regroup the weight-gradient
    sums leave the output's bits alone."""
    case = S.BY_ID[cid]
    with switch(*form):
        got = run(gpu_net(case, dev), case)
    judged(("form", "%s %s" % (cid, S.form_id(form))), got, S.want(case), base(case, dev))
    if form[0] in S.SAME_OUTPUT_BITS:
        assert torch.equal(got["out"], native(case, dev)["out"])


# ---- 3. frozen parameters -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frozen", [S.FROZEN, S.FROZEN + ("conv_gru2.gate_conv.bias", "conv_gru3.output_conv.weight", "conv_gru3.output_conv.bias")],
                         ids=["weights-and-norms", "whole-layers-too"])
def test_frozen_parameters(dev, frozen, monkeypatch):
    """Frozen parameters end without a gradient, every other gradient is right, and when the backward is over the sink holds no entry
    and keeps no recorded tensor alive -- a cell layer whose weight AND bias are frozen records nothing, since nobody would collect it."""
    from satmvs_amd.modules import module as M
    case = S.BY_ID["red-d2"]
    net = S.module(case)
    for n, p in net.named_parameters():
        p.requires_grad_(n not in frozen)
    ins, weight = S.inputs(case)
    want = S.as_set(net, *S.reference(net, ins, weight))
    assert {n for n, t in want.items() if t is None} == set(frozen)
    net = net.to(dev)
    basis = composite(net, case)
    sinks = []

    class Recording(M._WgradSink):
        def __init__(self):
            super().__init__()
            self.windows = []
            sinks.append(self)

        def add(self, weight, bias, win, win2, grid, stride):
            self.windows.append(weakref.ref(win))
            super().add(weight, bias, win, win2, grid, stride)

    monkeypatch.setattr(M, "_WgradSink", Recording)
    got = run(net, case)
    assert {n for n, t in got.items() if t is None} == set(frozen)
    judged(("frozen", "red-d2 %d frozen" % len(frozen)), got, want, basis)
    assert len(sinks) == 1 and len(sinks[0].windows) > 0
    assert len(sinks[0].layers) == 0, "entries nobody collected: %d" % len(sinks[0].layers)
    gc.collect()
    assert all(w() is None for w in sinks[0].windows)


# ---- 4. second backward, accumulation -------------------------------------------------------------------------------------------------
def test_second_backward_through_the_same_graph_doubles_every_gradient(dev):
    case = S.BY_ID["red-d2"]
    got = run(gpu_net(case, dev), case, backwards=2)
    judged(("twice", "red-d2 backward twice"), got, S.scaled(S.want(case), 2.0), S.scaled(base(case, dev), 2.0))
    assert torch.equal(got["out"], native(case, dev)["out"])


def test_two_forwards_accumulate_into_the_same_gradients(dev):
    case = S.BY_ID["red-d2"]
    net = gpu_net(case, dev)
    ins, weight = S.inputs(case)
    leaves = [t.to(dev).clone().requires_grad_(True) for t in ins]
    net.zero_grad(set_to_none=True)
    for _ in range(2):
        out = S.forward(net, leaves)
        (out * weight.to(dev)).sum().backward()
    torch.cuda.synchronize()
    got = S.collect(net, out, leaves)
    judged(("twice", "red-d2 two forwards"), got, S.scaled(S.want(case), 2.0), S.scaled(base(case, dev), 2.0))


# ---- 5. norm eps ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["cell-1", "cell-odd"])
@pytest.mark.parametrize("eps", [1e-3, (1e-3, 1e-4, 1e-5)], ids=["eps-equal", "eps-differ"])
def test_norm_eps_away_from_the_default(dev, cid, eps, monkeypatch):
    """Three norms with eps = 1e-3 stay on the one-node path (batch 1), which receives that eps; norms that differ take the cell piece by
    piece, every norm with its own eps."""
    case = S.BY_ID[cid]
    net = S.module(case, eps=eps)
    ins, weight = S.inputs(case)
    want = S.as_set(net, *S.reference(net, ins, weight))
    assert float((want["out"] - S.want(case)["out"]).abs().max()) > 1e-5          # eps is visible in float64
    net = net.to(dev)
    basis = composite(net, case)
    spy = Spy(monkeypatch)
    got = run(net, case)
    equal = not isinstance(eps, tuple)
    judged(("eps", "%s %s" % (cid, "1e-3" if equal else "1e-3/1e-4/1e-5")), got, want, basis)
    assert ("smvs_groupnorm1_pair_fwd_mul" in spy.names) == (equal and case.B == 1)
    assert ("smvs_groupnorm1_pair_fwd" in spy.names) == (equal and case.B > 1)
    for name in ("smvs_groupnorm1_pair_fwd_mul", "smvs_groupnorm1_pair_fwd"):
        if name in spy.names:
            assert spy.args[name][5] == 1e-3
    if not equal:
        assert spy.names.count("smvs_groupnorm1_fwd") == 3 * case.D


# ---- 6. side stream -------------------------------------------------------------------------------------------------------------------
def test_on_a_side_stream(dev):
    case = S.BY_ID["red-d2"]
    net = S.module(case).to(dev)                   # a fresh module: its kernel-layout copies are made on the side stream too
    torch.cuda.synchronize()
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        got = run(net, case)
    judged(("stream", "red-d2 side stream"), got, S.want(case), base(case, dev))
    assert torch.equal(got["out"], native(case, dev)["out"])


# ---- 7. planted faults ----------------------------------------------------------------------------------------------------------------
# One native call's arguments rewritten; every pointer stays valid and of the original size.  reaches: the tensors the fault must fail.
def _fault_a(name, a):                  # the gate norms' backward: reset and update gamma swapped
    if name == "smvs_groupnorm1_pair_bwd":
        a[3], a[4] = a[4], a[3]
        return a


def _fault_b(name, a):                  # the gate norms' forward (+ r*h): (gamma, beta) of the two gates swapped
    if name == "smvs_groupnorm1_pair_fwd_mul":
        a[1], a[2], a[3], a[4] = a[3], a[4], a[1], a[2]
        return a


def _fault_c(name, a):                  # the gate convolution's input gradient no longer starts from the candidate path's [dx | dh]
    if name == "smvs_conv3x3_fwd" and a[7] is not None:
        a[7] = None
        return a


def _fault_d(name, a):                  # the blend's state gradient never reaches dh
    if name == "smvs_gru_mul_cat_bwd_acc":
        a[3] = torch.zeros_like(a[3])
        return a


def _fault_e(name, a):                  # the last plane dropped from every deferred weight-gradient sum
    if name == "smvs_conv3x3_wgrad_list" and a[3] > 1:
        n = a[3] - 1
        for k in (0, 1, 2):
            if a[k] is not None:
                a[k] = (ctypes.c_void_p * n)(*a[k][:n])
        a[3] = n
        return a


def _fault_f(name, a):                  # the output norm (+ blend) with a hundred times the eps
    if name == "smvs_groupnorm1_fwd_blend":
        a[4] = a[4] * 100.0
        return a


def _is_conv_weight(n):
    return n.endswith("conv.weight") or n == "upconv2d.weight"


FAULTS = {"a": (_fault_a, lambda n: n.endswith("gate_conv.weight") or n == "dvol"),
          "b": (_fault_b, lambda n: n == "out"),
          "c": (_fault_c, lambda n: n == "dvol" or n.endswith("gate_conv.weight")),
          "d": (_fault_d, lambda n: n == "dvol" or n.endswith("gate_conv.weight")),
          "e": (_fault_e, _is_conv_weight),
          "f": (_fault_f, lambda n: n == "out")}


@pytest.mark.parametrize("which", sorted(FAULTS))
def test_planted_fault_fails_the_judge(dev, which, monkeypatch):
    case = S.BY_ID["red-d2"]
    rewrite, reaches = FAULTS[which]
    healthy, (healthy_worst, _) = S.judge(native(case, dev), S.want(case), base(case, dev))
    spy = Spy(monkeypatch, rewrite)
    got = run(S.module(case).to(dev), case)
    monkeypatch.undo()
    assert spy.hits > 0, "the fault was never planted"
    ratios, (worst, name) = S.judge(got, S.want(case), base(case, dev))
    bad = S.failing(ratios)
    smallest = min(ratios[n] for n in bad) if bad else float("nan")
    print("fault %s: %d of %d tensors fail, smallest failing ratio %.1f, largest %.3g (%s); healthy worst %.3f" % (
        which, len(bad), len(ratios), smallest, worst, name, healthy_worst))
    RATIOS[("fault", which)] = "%2d of %d tensors fail  smallest failing ratio %10.1f  largest %10.3g  %s   (healthy worst %.3f)" % (
        len(bad), len(ratios), smallest, worst, name, healthy_worst)
    assert bad and any(reaches(n) for n in bad), (which, bad)
    if which == "e":                    # every layer with a deferred sum lost a plane
        assert all(n in bad for n in ratios if _is_conv_weight(n)), sorted(n for n in ratios if _is_conv_weight(n) and n not in bad)


# ---- records ----------------------------------------------------------------------------------------------------------------------------
def test_write_ratios():
    """With SMVS_WRITE_RATIOS=<path> the figures of this run go there (profiles/red_train_ratios.txt is such a file); asserts nothing."""
    path = os.environ.get("SMVS_WRITE_RATIOS")
    lines = ["%-7s %-34s %s" % (kind, ident, text) for (kind, ident), text in RATIOS.items()]
    for line in lines:
        print("red-train", line)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
