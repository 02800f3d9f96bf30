"""smvs_costvol_bwd cell by cell against the float64 reference and the derived bound of tests/costvol_bwd_scene.py: the case matrix
through the C entry (guard words round all V gradient buffers) and through warping.variance_cost_volume(...).backward, buffers
that are not zero when the call starts, a side stream, a larger call before a smaller one and two calls against each other.
tests/test_costvol_bwd_scene_cpu.py asserts, without a GPU, that every case runs the kernel paths it is named for."""
import numpy as np
import pytest
import torch

import costvol_bwd_scene as Q

pytestmark = pytest.mark.gpu
NAMES = list(Q.CASES)
SENTINEL = 1234.5
REPORT = {}                                                 # (scheme, source-count class) -> largest err / bound seen
SCHEMES = ("boxed", "register", "border")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def orc(oracle):
    return oracle


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                 # (a copy: the scenes are shared and read-only)


def run_entry(dev, name, init=None):
    """One call of the C entry on the current stream.  The V gradient buffers lie in one allocation, GUARD words before, between and
    behind them (so they are 4-byte aligned, no more); init: V arrays the buffers hold when the call starts (default zeros).
    -> (grad_src list, grad_ref) as numpy; asserts that the guard words kept their bits."""
    from satmvs_amd import _lib
    from satmvs_amd.modules import warping
    sc = Q.scene(name)
    V, (B, C, H, W) = sc["V"], sc["feats"][0].shape
    fs = [_t(f, dev) for f in sc["feats"]]
    kind, geo = warping.prepare_geometry(fs, _t(sc["gp"], dev), sc["geo"])
    depth, is4d, D = warping._depth_arg(_t(sc["depth"], dev), B, H, W)
    n, G = B * C * H * W, Q.GUARD
    host = np.full(V * n + (V + 1) * G, SENTINEL, np.float32)
    for v in range(V):
        host[G + v * (n + G):G + v * (n + G) + n] = 0.0 if init is None else np.asarray(init[v], np.float32).ravel()
    flat = _t(host, dev)
    bufs = [flat[G + v * (n + G):G + v * (n + G) + n] for v in range(V)]
    _lib.launch(dev, "smvs_costvol_bwd", kind, _t(sc["gvar"], dev), fs[0], _lib.ptr_array(fs[1:]), V - 1, geo, depth, is4d, bufs[0],
                _lib.ptr_array(bufs[1:]), B, C, D, H, W)
    torch.cuda.current_stream(dev).synchronize()
    out = flat.cpu().numpy()
    guard = np.ones(out.size, bool)
    for v in range(V):
        guard[G + v * (n + G):G + v * (n + G) + n] = False
    assert (out[guard].view(np.uint32) == np.float32(SENTINEL).view(np.uint32)).all(), "%s: guard words written" % name
    res = [out[G + v * (n + G):G + v * (n + G) + n].reshape(B, C, H, W) for v in range(V)]
    return res[1:], res[0]


def run_autograd(dev, name):
    from satmvs_amd.modules import warping
    sc = Q.scene(name)
    fs = [_t(f, dev).requires_grad_(True) for f in sc["feats"]]
    var = warping.variance_cost_volume(fs, _t(sc["gp"], dev), _t(sc["depth"], dev), sc["geo"])
    var.backward(_t(sc["gvar"], dev))
    res = [f.grad.cpu().numpy() for f in fs]
    return res[1:], res[0]


def check_case(name, grads, gref, init=None, record=True):
    """Every view's gradient and the reference view's through Q.check; -> messages."""
    sc, ref = Q.scene(name), Q.scene_reference(name)
    cls = Q.src_class(sc["n_src"])
    cen = Q.census(sc["n_src"], ref["taps"], sc["D"], sc["H"], sc["W"]) if record else None
    msgs = []
    for s in range(sc["n_src"]):
        i = None if init is None else init[s + 1]
        m, ratio = Q.check(grads[s], ref["src"][s]["ref"], Q.bound_src(ref, s, i), ref["src"][s]["cnt"], i, "%s view %d" % (name, s + 1))
        msgs += m
        if record:
            scheme = Q.cell_schemes(cen, ref["taps"], s, sc["H"], sc["W"])[:, None]
            for level, key in enumerate(SCHEMES):
                r = float(np.where(scheme == level, ratio, 0.0).max())
                REPORT[(key, cls)] = max(REPORT.get((key, cls), 0.0), r)
    i = None if init is None else init[0]
    m, ratio = Q.check(gref, ref["ref"]["ref"], Q.bound_ref(ref, i), None, i, "%s reference view" % name)
    if record:
        REPORT[("grad_ref", cls)] = max(REPORT.get(("grad_ref", cls), 0.0), float(ratio.max()))
    return msgs + m


def extra_checks(name, grads, gref):
    sc, ref = Q.scene(name), Q.scene_reference(name)
    if sc.get("gmode") == "zero":                           # every output keeps its initial bits
        assert all((g.view(np.uint32) == 0).all() for g in grads + [gref])
    if sc.get("gmode") == "zero_box":                       # cells only the zeroed wave reaches: +-0, nothing else
        for s in range(sc["n_src"]):
            only = (ref["src"][s]["cnt"] > 0)[:, None] & (ref["src"][s]["mag"] == 0)
            assert only.any() and (grads[s][only] == 0).all()
    if sc["geo"] == "pinhole" and name.startswith("collapse"):
        n_const = sc["n_src"] - (1 if name == "collapse_runs_v3" else 0)
        for s in range(n_const):                            # the four cells against the closed-form sum, inside the same bound
            bound = Q.bound_src(ref, s)
            for (y, x), tot in Q.closed_form_collapse(sc, s, ref["taps"]).items():
                err = np.abs(grads[s][0, :, y, x].astype(np.float64) - tot)
                assert (err <= bound[0, :, y, x] * (1 + 1e-9)).all(), (name, s, y, x, err, bound[0, :, y, x])
            assert ref["src"][s]["cnt"].max() * Q.U < 1.0


@pytest.mark.parametrize("name", NAMES)
def test_c_entry(dev, orc, name):
    grads, gref = run_entry(dev, name)
    msgs = check_case(name, grads, gref)
    assert not msgs, "\n".join(msgs)
    extra_checks(name, grads, gref)


@pytest.mark.parametrize("name", NAMES)
def test_autograd_backward(dev, orc, name):
    grads, gref = run_autograd(dev, name)
    msgs = check_case(name, grads, gref, record=False)
    assert not msgs, "\n".join(msgs)
    extra_checks(name, grads, gref)


@pytest.mark.parametrize("name", ["v3_rpc", "runs_v5", "v8_rpc", "collapse_v3", "g_zero"])
def test_buffers_that_are_not_zero_accumulate(dev, orc, name):
    """The C entry accumulates: the result is the initial value plus the gradient.  Every atomic that reaches a cell rounds a sum
    that includes the initial value, at most one per contribution (grad_src) or per plane chunk (grad_ref): the bound grows by
    gamma(n) |initial| resp. gamma(chunks) |initial| (costvol_bwd_scene.bound_src / bound_ref); a cell nothing reaches keeps its bits."""
    sc = Q.scene(name)
    rng = np.random.default_rng(11)
    init = [(3.0 * rng.standard_normal(sc["feats"][0].shape)).astype(np.float32) for _ in range(sc["V"])]
    grads, gref = run_entry(dev, name, init)
    msgs = check_case(name, grads, gref, init, record=False)
    assert not msgs, "\n".join(msgs)
    if name == "g_zero":
        assert all((g.view(np.uint32) == i.view(np.uint32)).all() for g, i in zip([gref] + grads, init))


def test_side_stream(dev, orc):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        grads, gref = run_entry(dev, "mixed_v3")
    side.synchronize()
    msgs = check_case("mixed_v3", grads, gref, record=False)
    assert not msgs, "\n".join(msgs)


def test_larger_call_before_smaller_and_two_calls(dev, orc):
    """Nothing of a larger launch (boxes in LDS, taps) reaches a smaller one that follows; two calls on the same inputs are both
    inside the bound and therefore within twice the bound of each other (the atomics' order is free)."""
    for name in ("v3_rpc", "2x2_v3", "huge_v5", "v4_rpc"):
        grads, gref = run_entry(dev, name)
        msgs = check_case(name, grads, gref, record=False)
        assert not msgs, "\n".join(msgs)
    ref = Q.scene_reference("v4_rpc")
    again, gref2 = run_entry(dev, "v4_rpc")
    for s, (a, b) in enumerate(zip(grads, again)):
        assert (np.abs(a.astype(np.float64) - b) <= 2 * Q.bound_src(ref, s)).all()
    assert (np.abs(gref.astype(np.float64) - gref2) <= 2 * Q.bound_ref(ref)).all()


def test_report_largest_error_over_bound(dev, orc):
    """Prints what the cases above measured (run the file with -s): largest err / bound per scatter scheme and source-count class."""
    if not REPORT:                                          # selected on its own
        for name in ("v3_rpc", "runs_v5", "v8_rpc"):
            assert not check_case(name, *run_entry(dev, name))
    for key in SCHEMES + ("grad_ref",):
        print("costvol_bwd err/bound  %-9s" % key, "  ".join("%s sources: %.3f" % (cls, REPORT.get((key, cls), 0.0)) for cls in ("1-2", "3-4", "5-7")))
    assert max(REPORT.values()) <= 1.0
