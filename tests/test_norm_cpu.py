"""What tests/test_norm_gpu.py assumes about tests/norm_scene.py, asserted without a GPU: the cases reach the classes they were chosen
for and every class is reached; the float64 references are torch's float64 group_norm / batch_norm and their autograd; a float32 model
of each kernel's order of operations lies inside every bound on every scene and gives the exact scenes' bits; the planted errors --
the wrong results a kernel of this design could return -- are each outside a bound, or unequal on an exact scene, on every case of
their class; and no reference leaves an element undecided (the judges assert shape, finiteness and a non-negative bound of all of them)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_scene as S

GN_ALL = S.GN_CASES + S.PAIR_CASES
GN_IDS = [c.name for c in GN_ALL]
BN_IDS = [c.name for c in S.BN_CASES]


def test_every_case_reaches_its_classes_and_every_class_is_reached():
    for cases, classes, intended, required in ((GN_ALL, S.gn_classes, S.GN_INTENDED, S.GN_REQUIRED),
                                               (S.BN_CASES, S.bn_classes, S.BN_INTENDED, S.BN_REQUIRED)):
        assert sorted(intended) == sorted(c.name for c in cases)
        reached = {c.name: classes(c) for c in cases}
        for c in cases:
            assert intended[c.name] <= reached[c.name], (c.name, sorted(intended[c.name] - reached[c.name]))
        for cls in sorted(required):
            assert any(cls in r for r in reached.values()), "no case reaches " + cls
    for cls in sorted(S.BLEND_REQUIRED):
        assert any(cls in S.blend_classes(n) for n in S.BLEND_N), "no blend size reaches " + cls
    for cls in sorted(S.MULCAT_REQUIRED):
        assert any(cls in S.mulcat_classes(m) for m in S.MULCAT), "no mul_cat shape reaches " + cls
    # the statements of the case list, from the rules: 4098 = float4 then scalar on row 0 and scalar on row 1; 64 + 1: sample 1 scalar
    c = S.GN_BY_NAME["1x2x4098"]
    segs = S.gn_segments(c)
    assert [[S.gn_row_vec4(c, 0, k, s, ("x", "y")) for s in segs] for k in range(2)] == [[True, False], [False, False]]
    c = S.GN_BY_NAME["2x4x64-strides"]
    assert [S.gn_row_vec4(c, b, 1, (0, 64), ("x", "y")) for b in range(2)] == [True, False]
    assert [S.gn_row_vec4(c, b, 1, (0, 64), ("x", "dy", "y", "dx")) for b in range(2)] == [True, False]
    c = S.GN_BY_NAME["1x3x1366"]
    assert [(i1 - i0, v) for i0, i1, v in S.gn_stats_chunks(c, 0)] == [(4096, True), (2, False)]
    c = S.GN_BY_NAME["1x4x262400"]
    assert len(S.gn_stats_chunks(c, 0)) == 257
    c = S.GN_BY_NAME["2x130x4100"]
    assert c.C * len(S.gn_segments(c)) == 260
    for c in S.PAIR_CASES:                                     # the two parameter sets differ clearly: a swapped parity is far outside
        for kind in S.GN_KINDS:
            if S.gn_scene_applies(c, kind):
                sc = S.gn_scene(c, kind)
                assert (np.abs(sc.gamma2 - sc.gamma) >= 2.0).all() and (np.abs(sc.beta2 - sc.beta) >= 5.0).all()


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b) / (1.0 + np.abs(b))
    assert err.max() <= 1e-10, (what, float(err.max()))


SMALL = [c for c in GN_ALL if c.C * c.HW <= 20000]


@pytest.mark.parametrize("c", SMALL, ids=[c.name for c in SMALL])
def test_groupnorm_references_are_torch_float64(c):
    for kind in S.GN_KINDS:
        if not S.gn_scene_applies(c, kind):
            continue
        sc = S.gn_scene(c, kind)
        Bi, C, HW = sc.x.shape
        G, Bt = S.per_sample(sc, sc.gamma, sc.gamma2), S.per_sample(sc, sc.beta, sc.beta2)
        for act in c.acts:
            ref = S.gn_ref_fwd(sc, act)
            mr = np.stack([ref["mean"], ref["rstd"]], axis=1)
            back = S.gn_ref_bwd(sc, act, ref["y"], mr)
            for b in range(Bi):
                x = _t(sc.x[b:b + 1]).requires_grad_(True)
                g, bt = _t(G[b]).requires_grad_(True), _t(Bt[b]).requires_grad_(True)
                y = torch.native_group_norm(x, g, bt, 1, C, HW, 1, sc.eps)[0]      # (F.group_norm refuses a sample of one value)
                y = torch.sigmoid(y) if act == 1 else torch.tanh(y) if act == 2 else y
                _close(ref["y"][b], y.detach().numpy()[0], (c.name, kind, act, "y"))
                dx, dg, db = torch.autograd.grad(y, (x, g, bt), _t(sc.dy[b:b + 1]))
                _close(back["dx"][b], dx.numpy()[0], (c.name, kind, act, "dx"))
                if Bi == 1:
                    _close(back["dgamma"], dg.numpy(), (c.name, kind, act, "dgamma"))
                    _close(back["dbeta"], db.numpy(), (c.name, kind, act, "dbeta"))


@pytest.mark.parametrize("c", S.BN_CASES, ids=BN_IDS)
def test_batchnorm_references_are_torch_float64(c):
    for kind in S.BN_KINDS:
        if not S.bn_scene_applies(c, kind):
            continue
        sc = S.bn_scene(c, kind)
        for relu in (0, 1):
            ref = S.bn_ref_fwd(sc, relu)
            p = sc.x[0, :, 0].astype(np.float64)
            back = S.bn_ref_bwd(sc, relu, ref["y"], np.stack([ref["mean"] - p, ref["rstd"]], axis=1))
            x = _t(sc.x).requires_grad_(True)
            g, bt = _t(sc.gamma).requires_grad_(True), _t(sc.beta).requires_grad_(True)
            rm, rv = _t(sc.rm).clone(), _t(sc.rv).clone()
            y = F.batch_norm(x, rm, rv, g, bt, True, sc.momentum, sc.eps)
            y = torch.relu(y) if relu else y
            _close(ref["y"], y.detach().numpy(), (c.name, kind, relu, "y"))
            _close(ref["rm"], rm.numpy(), (c.name, kind, "running_mean"))
            _close(ref["rv"], rv.numpy(), (c.name, kind, "running_var"))
            dx, dg, db = torch.autograd.grad(y, (x, g, bt), _t(sc.dy))
            _close(back["dx"], dx.numpy(), (c.name, kind, relu, "dx"))
            _close(back["dgamma"], dg.numpy(), (c.name, kind, relu, "dgamma"))
            _close(back["dbeta"], db.numpy(), (c.name, kind, relu, "dbeta"))


def _gn_model_verdicts(c, kind, act, plant=None):
    sc = S.gn_scene(c, kind)
    y, mr = S.gn_model_fwd(c, sc, act, plant)
    vf = S.gn_judge_fwd(c, kind, act, y, mr)
    vb = S.gn_judge_bwd(c, kind, act, y, mr, S.gn_model_bwd(c, sc, act, y, mr, plant))
    return vf, vb


@pytest.mark.parametrize("c", GN_ALL, ids=GN_IDS)
def test_groupnorm_model_lies_inside_every_bound(c):
    """... and equals the reference on the exact scenes (the judges assert both)."""
    worst = {}
    for kind in S.GN_KINDS:
        if not S.gn_scene_applies(c, kind):
            continue
        for act in c.acts:
            for v in _gn_model_verdicts(c, kind, act):
                assert v.ok, v.messages[0]
                for k, r in v.ratios.items():
                    worst[k] = max(worst.get(k, 0.0), r)
    print("norm-model-ratio gn %-18s %s" % (c.name, " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("c", S.BN_CASES, ids=BN_IDS)
def test_batchnorm_model_lies_inside_every_bound(c):
    worst = {}
    for kind in S.BN_KINDS:
        if not S.bn_scene_applies(c, kind):
            continue
        sc = S.bn_scene(c, kind)
        for relu in (0, 1):
            f = S.bn_model_fwd(c, sc, relu)
            vs = [S.bn_judge_fwd(c, kind, relu, f), S.bn_judge_bwd(c, kind, relu, f["y"], f["saved"], S.bn_model_bwd(c, sc, relu, f["saved"]))]
            for v in vs:
                assert v.ok, v.messages[0]
                for k, r in v.ratios.items():
                    worst[k] = max(worst.get(k, 0.0), r)
    print("norm-model-ratio bn %-18s %s" % (c.name, " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("plant", S.GN_PLANTS)
def test_groupnorm_planted_errors_are_caught(plant):
    """On every case of the plant's class, on the real scene and on the first exact scene that applies: a verdict fails."""
    hit = 0
    for c in GN_ALL:
        if not S.gn_plant_applies(c, plant):
            continue
        kinds = ["real"] + [k for k in ("exact96",) if S.gn_scene_applies(c, k)]
        for kind in kinds:
            vf, vb = _gn_model_verdicts(c, kind, 0, plant)
            assert not (vf.ok and vb.ok), (plant, c.name, kind, "passes")
            hit += 1
    assert hit >= 2, plant


@pytest.mark.parametrize("plant", S.BN_PLANTS)
def test_batchnorm_planted_errors_are_caught(plant):
    hit = 0
    for c in S.BN_CASES:
        if not S.bn_plant_applies(c, plant):
            continue
        kind = "zero-gamma" if plant == "mask-greater-or-equal" else "real"
        sc = S.bn_scene(c, kind)
        f = S.bn_model_fwd(c, sc, 1, plant)
        vf = S.bn_judge_fwd(c, kind, 1, f)
        vb = S.bn_judge_bwd(c, kind, 1, f["y"], f["saved"], S.bn_model_bwd(c, sc, 1, f["saved"], plant))
        assert not (vf.ok and vb.ok), (plant, c.name, "passes")
        hit += 1
    assert hit >= 5, plant


def test_gru_models_and_the_dropped_tail():
    """The float32 expressions are within u of float64 (they are what the GPU tests demand bit for bit); a blend without its tail is
    unequal wherever n is not a multiple of 4."""
    for n in S.BLEND_N:
        dy, u, h, y = S.blend_scene(n)
        out = S.blend_fwd32(u, h, y)
        d = lambda a: a.astype(np.float64)
        ref = d(u) * d(h) + (1 - d(u)) * d(y)
        assert S.check(out, ref, 3 * S.U * (np.abs(d(u) * d(h)) + np.abs((1 - d(u)) * d(y))) + S.TINY, "blend").ok
        du, dh, dc = S.blend_bwd32(dy, u, h, y)
        assert S.check(du, d(dy) * (d(h) - d(y)), 2 * S.U * np.abs(d(dy) * (d(h) - d(y))) + S.TINY, "du").ok
        assert S.check(dh, d(dy) * d(u), S.U * np.abs(d(dy) * d(u)) + S.TINY, "dh").ok
        assert S.check(dc, d(dy) * (1 - d(u)), 2 * S.U * np.abs(d(dy) * (1 - d(u))) + S.TINY, "dcand").ok
        assert S.same_bits(S.blend_fwd32(u, h, y, "blend-tail-dropped"), out) == (n % 4 == 0)
    for m in S.MULCAT:
        x, r, h, dcat, dh_acc = S.mulcat_scene(m)
        out = S.mulcat_fwd32(x, r, h)
        assert out.shape == dcat.shape and S.same_bits(out[:, :m[1]], x)
        dr, ref, bound = S.mulcat_bwd_acc64(dcat, r, h, dh_acc, m[1])
        assert S.same_bits(dr, S.mulcat_bwd32(dcat, r, h, m[1])[0])
        assert S.check(S.fma32(dcat[:, m[1]:], r, dh_acc), ref, bound, "bwd_acc").ok


def test_the_checker_leaves_nothing_out():
    ref, bound = np.array([1.0, 2.0, np.nan, 0.0]), np.array([0.1, 0.0, 0.1, 0.0])
    assert S.check(np.array([1.05, 2.0, np.nan, 0.0]), ref, bound, "t").ok
    for got in ([1.2, 2.0, np.nan, 0.0], [1.0, 2.0000001, np.nan, 0.0], [1.0, 2.0, 0.0, 0.0], [np.nan, 2.0, np.nan, 0.0],
                [1.0, 2.0, np.nan, np.inf], [1.0, 2.0, np.nan, 1e-300]):
        assert not S.check(np.array(got), ref, bound, "t").ok, got
    with pytest.raises(AssertionError):
        S.assert_complete(ref, bound, (4,))
    with pytest.raises(AssertionError):
        S.assert_complete(ref[:2], bound[:2], (3,))
