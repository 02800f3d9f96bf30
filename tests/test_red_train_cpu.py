"""tests/red_train_scene.py without a GPU: the cases can see an error in every tensor, the judge accepts a correct float32 evaluation of
the training graph (torch's composite on the CPU) and rejects the faults the hand-written autograd layer could have -- norm parameters
swapped between the gates, states cut between the planes."""
import copy
import time

import pytest
import torch

import red_train_scene as S


@pytest.fixture(scope="module")
def SW():
    from satmvs_amd.modules.switches import SW
    return SW


def _float32(case, net=None, **kw):
    net = S.module(case) if net is None else net
    ins, weight = S.inputs(case)
    return S.run(net, ins, weight, **kw)


def _base(case, SW):
    """the float32 composite in its other association: every parameter used directly by every plane, autograd adding plane by plane"""
    saved = SW.train_plane_views
    SW.train_plane_views = False
    try:
        return _float32(case)
    finally:
        SW.train_plane_views = saved


def _swap_gate_gammas(net):
    with torch.no_grad():
        for name, m in net.named_modules():
            if hasattr(m, "reset_gate_norm"):
                r, u = m.reset_gate_norm.weight, m.update_gate_norm.weight
                t = r.clone()
                r.copy_(u)
                u.copy_(t)
    return net


def test_scene_imports_without_a_gpu_and_its_references_are_quick():
    """Importing the scene initialises no GPU, and the float64 references of all cases together take a few seconds at the most."""
    assert not torch.cuda.is_initialized()
    t0 = time.perf_counter()
    for case in S.CASES:
        S.want(case)
    assert time.perf_counter() - t0 < 20.0
    assert not torch.cuda.is_initialized()


@pytest.mark.parametrize("case", S.CASES, ids=S.IDS)
def test_every_float64_gradient_is_nonzero(case):
    """want() asserts max|t64| > 0 for the output, every input gradient and every parameter gradient; every parameter is there."""
    T = S.want(case)
    net = S.module(case)
    assert set(T) == {"out", *S.input_names(net)} | {n for n, _ in net.named_parameters()}
    zero = S.ZERO_BY_STRUCTURE.get(case.id, ())
    assert all(t.dtype is torch.float64 and (float(t.abs().max()) > 0.0) != (n in zero) for n, t in T.items())
    assert set(S.ZERO_BY_STRUCTURE) == {"red-d1"}
    if case.kind == "red":
        assert len(T) == 2 + 48


def test_randomise_gives_the_norms_of_a_cell_different_values():
    net = S.module(S.BY_ID["red-d2"])
    for cell in (net.conv_gru1, net.conv_gru2, net.conv_gru3, net.conv_gru4):
        norms = [(m.weight.detach(), m.bias.detach()) for m in (cell.reset_gate_norm, cell.update_gate_norm, cell.output_norm)]
        for a in range(3):
            for b in range(a + 1, 3):
                assert float((norms[a][0] - norms[b][0]).abs().min()) > 0.0
                assert float((norms[a][1] - norms[b][1]).abs().min()) > 0.0
            assert 0.5 <= float(norms[a][0].min()) and float(norms[a][0].max()) <= 1.5
        assert float(cell.gate_conv.bias.abs().max()) > 0.0
    again = S.module(S.BY_ID["red-d2"])
    assert all(torch.equal(p, q) for p, q in zip(net.parameters(), again.parameters()))


@pytest.mark.parametrize("case", S.CASES, ids=S.IDS)
def test_float32_composite_passes(case, SW):
    """The float32 CPU composite with per-plane parameter views against the same composite without them (another association of the
    same sums; the same bits where the case has no plane loop): inside the criterion, and every composite error positive."""
    got, base = _float32(case), _base(case, SW)
    zero = S.ZERO_BY_STRUCTURE.get(case.id, ())
    assert all((e[0] > 0.0 and e[1] > 0.0) != (n in zero) for n, e in S.errors(base, S.want(case)).items())
    ratios, (worst, name) = S.judge(got, S.want(case), base)
    assert worst <= S.LIMIT, (name, worst)


@pytest.mark.parametrize("cid", ["red-d2", "red-b2", "cell-1"])
def test_swapped_gate_gammas_fail(cid, SW):
    """Reset and update gamma swapped in every cell of a float32 copy: the judge rejects the output and the input gradient."""
    case = S.BY_ID[cid]
    got = _float32(case, _swap_gate_gammas(S.module(case)))
    ratios, (worst, name) = S.judge(got, S.want(case), _base(case, SW))
    bad = S.failing(ratios)
    assert "out" in bad and S.input_names(S.module(case))[0] in bad, bad
    assert worst > 1000.0


def test_swapped_gate_gammas_change_no_bit_at_the_default_initialisation():
    """The blind spot of a test with default norms (gamma 1, beta 0): the same swap leaves every output and gradient bit in place."""
    case = S.BY_ID["red-d2"]
    plain = S.module(case, randomised=False)
    a = _float32(case, plain)
    b = _float32(case, _swap_gate_gammas(copy.deepcopy(plain)))
    assert all(torch.equal(a[n], b[n]) for n in a)


def test_detached_states_fail(SW):
    """The states cut between the planes: the forward is untouched, the recurrent gradients are not."""
    case = S.BY_ID["red-d2"]
    got = _float32(case, detach_states=True)
    ratios, _ = S.judge(got, S.want(case), _base(case, SW))
    bad = S.failing(ratios)
    assert "out" not in bad
    assert "dvol" in bad and any(n.endswith("gate_conv.weight") for n in bad), bad


@pytest.mark.parametrize("cid", ["cell-1", "cell-odd"])
def test_one_eps_for_both_gate_norms_fails(cid):
    """Norms with eps 1e-3 / 1e-4 / 1e-5, evaluated with the reset norm's eps in the update norm too (what one call for both gate
    norms does): the judge rejects it."""
    case = S.BY_ID[cid]
    net = S.module(case, eps=(1e-3, 1e-4, 1e-5))
    ins, weight = S.inputs(case)
    want = S.as_set(net, *S.reference(net, ins, weight))
    basis = S.run(net, ins, weight)
    ratios, (worst, name) = S.judge(S.run(S.module(case, eps=(1e-3, 1e-3, 1e-5)), ins, weight), want, basis)
    print("one eps for both gate norms, %s: worst %.1f %s, %d of %d tensors fail" % (cid, worst, name, len(S.failing(ratios)), len(ratios)))
    assert "out" in S.failing(ratios) and "update_gate_norm.weight" in S.failing(ratios)


def test_frozen_parameters_have_no_gradient_in_the_reference():
    case = S.BY_ID["red-d2"]
    net = S.module(case)
    for n, p in net.named_parameters():
        p.requires_grad_(n not in S.FROZEN)
    ins, weight = S.inputs(case)
    T = S.as_set(net, *S.reference(net, ins, weight))
    assert {n for n, t in T.items() if t is None} == set(S.FROZEN)
    got = S.run(net, ins, weight)
    ratios, (worst, name) = S.judge(got, T, got)
    assert worst <= 1.0 and set(ratios) == set(T) - set(S.FROZEN)


def test_judge_refuses_a_gradient_where_none_is_due_and_a_non_finite_one():
    case = S.BY_ID["cell-1"]
    want = S.want(case)
    got = _float32(case)
    none_due = dict(want, dh=None)
    with pytest.raises(AssertionError):
        S.judge(got, none_due, got)
    bad = dict(got)
    bad["dx"] = got["dx"].clone()
    bad["dx"].view(-1)[3] = float("nan")
    ratios, (worst, name) = S.judge(bad, want, got)
    assert name == "dx" and worst == float("inf")
