"""What tests/test_wgrad_gpu.py assumes about tests/wgrad_scene.py, checked without a GPU: the cases reach every class of the split
(asked from the library's plan queries, the functions the launchers call), the workspace query agrees with the plan, the float64
reference is the definition and what autograd gives, the integer scenes stay exact in float32, a float32 model that sums the way the
plan says passes the real scenes' bound, and planted kernel errors do not pass check()."""
import ctypes as C

import numpy as np
import pytest
import torch

import wgrad_scene as S

IDS = [c.name for c in S.CASES]


@pytest.fixture(scope="module")
def lib():
    from satmvs_amd import build, _lib
    build.build()
    return _lib.load()


def plan_queries(lib):
    def plan2(*a):
        p = (C.c_int * 6)()
        return lib.smvs_conv3x3_wgrad_plan(*a, p), list(p)

    def plan3(*a):
        p = (C.c_int * 6)()
        return lib.smvs_conv3d_wgrad_plan(*a, p), list(p)
    return plan2, plan3


@pytest.fixture(scope="module")
def queries(lib):
    return plan_queries(lib)


def test_cases_are_well_formed():
    for c in S.CASES:
        assert c.stride in (1, 2) and c.role in ("conv", "transposed") and c.dw0 in ("zero", "nonzero"), c.name
        if c.entry == "3d":
            assert len(c.dims) == 3 and c.form in ("atomic", "two_stage") and not c.CB and not c.db, c.name
        else:
            assert len(c.dims) == 2 and c.form is None, c.name
            assert c.entry in ("wgrad", "strided", "cat", "list"), c.name
            assert c.stride == 1 or c.entry in ("strided", "list"), c.name
            assert not c.CB or (c.entry in ("cat", "list") and c.CA % 2 == 0 and c.CA >= 2), c.name


@pytest.mark.parametrize("c", S.CASES, ids=IDS)
def test_every_case_is_accepted_by_its_plan_query(queries, c):
    for p in S.plans(c, *queries):
        assert min(p) >= 1, (c.name, p)
    if c.entry == "3d":                         # ... in either form: the GPU tests run every 3-D case in both
        for form in ("atomic", "two_stage"):
            assert min(S.plans(c, *queries, form=form)[0]) >= 1


def test_the_cases_reach_every_class_of_the_split(queries):
    """The census of the issue, read from the plan queries: tests/wgrad_scene.py holds no copy of the split rule."""
    got2, got3 = S.covered(S.CASES_2D, *queries), S.covered(S.CASES_3D, *queries)
    assert not S.REQUIRED_2D - got2, "2-D classes without a case: %s" % sorted(S.REQUIRED_2D - got2)
    assert not S.REQUIRED_3D - got3, "3-D classes without a case: %s" % sorted(S.REQUIRED_3D - got3)


def test_targets_worked_out_from_the_code(queries):
    """The splits the case table names in its comments, as the launchers take them."""
    plan2, plan3 = queries
    assert plan2(1, 2, 9, 17, 65, 1) == (0, [1, 1, 9, 2, 2, 8])                 # H = 17: rows 9 + 8
    assert plan2(1, 3, 1, 33, 127, 1)[1][2:4] == [9, 4]                          # H = 33: rows 9, 9, 9, 6
    assert plan2(9, 128, 64, 4, 8, 1)[1][:2] == [2, 5]                           # B = 9: samples 2, 2, 2, 2, 1
    assert plan2(64, 2, 3, 2, 3, 2)[1][:2] == [1, 64]
    assert plan3(1, 64, 64, 8, 4, 8, 1, 0)[1][:2] == [2, 4]                      # atomic: planes 2, 2, 2, 2
    assert plan3(1, 64, 64, 8, 4, 8, 1, 1)[1][:2] == [4, 2]                      # two-stage: planes 4, 4
    straddle = S.BY_NAME["list-n3-straddle"]
    (bchunk, nbc, *_), = S.plans(straddle, *queries)
    assert (bchunk, nbc, straddle.Bper) == (2, 5, 3)                             # chunk {2, 3} holds samples of tensors 0 and 1
    assert len(S.launches(S.BY_NAME["list-n65"])) == 2


@pytest.mark.parametrize("c", S.CASES_3D, ids=[c.name for c in S.CASES_3D])
def test_workspace_query_equals_the_plans_count(lib, queries, c):
    plan, = S.plans(c, *queries, form="two_stage")
    D, H, W = c.dims
    want = S.workspace_floats(c, plan)
    assert lib.smvs_conv3d_wgrad_workspace_floats(c.B, S.cwin(c), c.Cgrid, D, H, W) == want
    assert plan[5] == ((S.cwin(c) + 1) // 2) * ((c.Cgrid + 7) // 8) * 3 * S.waves_per_group(c, plan)


def test_workspace_query_equals_the_plans_count_over_a_sweep(lib, queries):
    plan3 = queries[1]
    for B, Cw, Cg, D, H, W in [(1, 8, 8, 48, 96, 192), (2, 16, 8, 24, 48, 96), (1, 64, 32, 6, 12, 24), (3, 1, 1, 7, 33, 129), (1, 32, 1, 32, 64, 64)]:
        rc, p = plan3(B, Cw, Cg, D, H, W, 1, 1)
        assert rc == 0 and plan3(B, Cw, Cg, D, H, W, 2, 1) == (0, p)            # the split does not depend on the stride
        assert lib.smvs_conv3d_wgrad_workspace_floats(B, Cw, Cg, D, H, W) == ((Cw + 1) // 2) * ((Cg + 7) // 8) * 3 * (B * p[1] * p[4] * p[3]) * 144


@pytest.mark.parametrize("c", S.CASES, ids=IDS)
def test_reference_is_what_autograd_gives(c):
    """wgrad() against the float64 autograd of conv / conv_transpose of the case's role, and against explicit loops where tiny."""
    sc = S.scene(c, "real")
    win, grid = torch.cat(sc.wins).double(), torch.cat(sc.grids).double()
    ref = S.wgrad(win, grid, c.stride)
    auto = S.autograd_wgrad(c, win, grid)
    scale = S.wgrad(win.abs(), grid.abs(), c.stride)
    assert bool(((ref - auto).abs() <= 1e-13 * scale + 1e-300).all()), c.name
    if win.numel() * c.Cgrid <= 40000:
        loop = torch.from_numpy(S.loop_wgrad(win.numpy(), grid.numpy(), c.stride))
        assert bool(((ref - loop).abs() <= 1e-13 * scale + 1e-300).all()), c.name
    full = S.reference(c, "real")
    assert torch.equal(full.dw, sc.dw0.double() + ref)
    if c.db:
        assert bool(((full.db - sc.db0.double() - torch.cat(sc.grids).double().transpose(0, 1).flatten(1).sum(1)).abs() <= 1e-9).all())
    else:
        assert full.db is None


@pytest.mark.parametrize("c", S.CASES, ids=IDS)
def test_integer_scenes_are_exact_in_float32(queries, c):
    """Values in {-3..3} without 0, |init| + sum |terms| < 2^24 (reference_of asserts it), the reference is an integer that float32
    holds, and the float32 model -- any order -- returns exactly it."""
    sc = S.scene(c, "int")
    for t in sc.wins + sc.grids:
        assert set(t.unique().tolist()) <= set(float(v) for v in S.VALUES)
    ref = S.reference(c, "int")
    assert torch.equal(ref.dw, ref.dw.round()) and torch.equal(ref.dw.float().double(), ref.dw)
    assert float(ref.dw.abs().max()) < S.INT_LIMIT
    dw, db = S.model_f32(c, sc, S.plans(c, *queries), seed=1)
    ok, ratio, msg = S.check_case(c, "int", dw, db)
    assert ok and ratio == 0.0, msg
    assert torch.equal(dw, ref.dw.float())


@pytest.mark.parametrize("c", S.CASES, ids=IDS)
def test_float32_model_meets_the_real_scene_bound(queries, c):
    """Sequential per-lane chains, a pairwise lane reduction and the waves' sums in a shuffled order (two-stage: the fold's order),
    all following the plan: inside the bound at every weight.  3-D cases in both forms.  Prints the worst ratio."""
    sc = S.scene(c, "real")
    for form in (("atomic", "two_stage") if c.entry == "3d" else (None,)):
        dw, db = S.model_f32(c, sc, S.plans(c, *queries, form=form), seed=2, form=form)
        ok, ratio, msg = S.check_case(c, "real", dw, db)
        print("wgrad-model-ratio %-24s %-9s %.4f" % (c.name, form or "-", ratio))
        assert ok, msg
        assert 0.0 < ratio <= 1.0


PLANTED = [(c, p) for c in S.CASES for p in S.PLANTS]


def test_every_planted_error_has_cases(queries):
    for plant in S.PLANTS:
        n = sum(S.applicable(c, plant, S.plans(c, *queries)) for c in S.CASES)
        assert n >= 2, (plant, n)


@pytest.mark.parametrize("c", S.CASES, ids=IDS)
def test_planted_errors_are_caught(queries, c):
    """Every planted error, in the integer and in the real scene of every case it applies to: check() fails and names a weight."""
    pl = S.plans(c, *queries)
    for plant in S.PLANTS:
        if not S.applicable(c, plant, pl):
            continue
        for kind in ("int", "real"):
            ref = S.reference(c, kind)
            r = S.check(S.planted(c, kind, plant, pl), ref.dw, ref.dw_bound, c.name)
            assert not r.ok and r.ratio > 1.0 and r.first is not None, (c.name, plant, kind)
            assert c.name in r.message and str(list(r.first)) in r.message
            # ... and the correct result, rounded once, passes
            assert S.check(ref.dw.float(), ref.dw, ref.dw_bound).ok


def test_check_counts_non_finite_values():
    ref = torch.tensor([1.0, float("nan"), 2.0], dtype=torch.float64)
    bound = torch.full((3,), 1e-6, dtype=torch.float64)
    assert S.check(torch.tensor([1.0, float("nan"), 2.0]), ref, bound).ok
    assert not S.check(torch.tensor([float("nan"), float("nan"), 2.0]), ref, bound).ok
    assert not S.check(torch.tensor([1.0, 5.0, 2.0]), ref, bound).ok
    assert not S.check(torch.tensor([1.0, float("nan"), float("inf")]), ref, bound).ok
    r = S.check(torch.tensor([1.0, float("nan"), 2.5]), ref, bound, "w")
    assert r.first == (2,) and "w[2]" in r.message
