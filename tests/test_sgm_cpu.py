"""The two numpy statements of each SGM rule (tests/sgm_oracle.py) against each other on the case matrix; the invariants of the
aggregation and of the parabola; a hand-computed example; every argument rejection of satmvs_amd.sgm and of the three C entries
that needs no GPU; planted errors that the GPU file's comparison must report; and the end-to-end scene on the oracle, with the
warps of oracle/torch_composite."""
import ctypes as C

import numpy as np
import pytest

import sgm_oracle as so
import sgm_scene as sc
from dsm_testkit import lib  # noqa: F401  (fixture)

ERR_ARG = 1


# ---- the rules, twice --------------------------------------------------------------------------------------------------------------
def test_census_statements_agree():
    names = []
    for name, ref, warped, radius, cov_min in sc.census_matrix():
        names.append(name)
        sc.compare(so.census_cost(ref, warped, radius, cov_min), so.census_cost_loop(ref, warped, radius, cov_min), name)
    assert len(names) == len(set(names)) > 25


def test_aggregate_statements_agree():
    names = []
    for name, cost, kw in sc.aggregate_matrix():
        names.append(name)
        sc.compare(so.aggregate(cost, **kw), so.aggregate(cost, walk=True, **kw), name)
    assert len(names) == len(set(names)) > 50


def test_select_statements_agree():
    for name, total, depth, kw in sc.select_matrix():
        got, want = so.select(total, depth, **kw), so.select_loop(total, depth, **kw)
        for g, w, what in zip(got, want, ("index", "height", "min_sum", "support")):
            assert (g is None) == (w is None)
            if g is not None:
                sc.compare(g, w, "%s: %s" % (name, what))


def test_the_matrix_is_what_the_gpu_tests_assume():
    grids = {c[1].shape[1:] for c in sc.census_matrix()}
    assert {(1, 1), (1, 70), (67, 1), (2, 2), (7, 7)} <= grids
    assert {sc.TILE_H - 1, sc.TILE_H, sc.TILE_H + 1} <= {g[0] for g in grids} and {sc.TILE_W - 1, sc.TILE_W, sc.TILE_W + 1} <= {g[1] for g in grids}
    assert {len(c[2]) for c in sc.census_matrix()} >= {1, 2, 3, 7} and {c[3] for c in sc.census_matrix()} == {1, 2, 3}
    assert {c[2][0].shape[2] for c in sc.census_matrix()} >= {1, 7, 8, 9}
    voids = [float((so.census_cost(*c[1:]) == sc.VOID).mean()) for c in sc.census_matrix()]
    assert max(voids) == 1.0 and min(voids) == 0.0 and 0.05 < np.median(voids) < 0.9
    agg = sc.aggregate_matrix()
    assert {c[1].shape[3] for c in agg} >= set(sc.AGG_D) and {c[1].shape[1:3] for c in agg} >= set(sc.AGG_GRIDS)
    assert {c[1].shape[0] for c in agg} == {1, 2} and {c[2]["paths"] for c in agg} == {4, 8}
    assert any(c[2]["paths"] * (c[2].get("cost_max", 768) + c[2]["P2"]) > 65535 - c[2]["paths"] for c in agg)      # one more P2 would wrap
    index = np.concatenate([so.select(*c[1:3], **c[3])[0].ravel() for c in sc.select_matrix()])
    assert (index == -1).any() and (index == 0).any() and (index >= 0).mean() > 0.3
    edge = [c for c in sc.select_matrix() if c[0] == "uniqueness threshold"][0]
    assert so.select(*edge[1:3], **edge[3])[0][0, 0].tolist() == [2, -1, 2, -1]


# ---- invariants --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def volume():
    rng = np.random.default_rng(1)
    return sc.valley_cost(rng, 2, 13, 17, 21)


def test_every_path_lies_between_the_cost_and_the_cost_plus_p2(volume):
    cp = so.clamped(volume, 768, 96)
    for L in so.aggregate(volume, 16, 96, 8, parts=True):
        assert (L >= cp).all() and (L <= cp + 96).all()
    g = sc.guide_image(np.random.default_rng(2), 2, 13, 17)
    for L in so.aggregate(volume, 10, 120, 8, guide=g, alpha=5, p2_min=20, parts=True):
        assert (L >= cp).all() and (L <= cp + 120).all()


def test_without_penalties_the_sum_is_the_cost(volume):
    for paths in (4, 8):
        sc.compare(so.aggregate(volume, 0, 0, paths), (paths * so.clamped(volume, 768, 96)).astype(np.uint16), paths)


def test_a_constant_volume_stays_constant():
    for paths in (4, 8):
        for D in (1, 2, 40):
            assert (so.aggregate(np.full((1, 6, 7, D), 55, np.uint16), 16, 96, paths) == paths * 55).all()


def test_flips_and_the_transpose(volume):
    want = so.aggregate(volume, 16, 96, 8)
    sc.compare(so.aggregate(volume[:, :, ::-1], 16, 96, 8), want[:, :, ::-1], "flipped along W")
    sc.compare(so.aggregate(volume[:, ::-1], 16, 96, 8), want[:, ::-1], "flipped along H")
    sc.compare(so.aggregate(volume.transpose(0, 2, 1, 3), 16, 96, 8), want.transpose(0, 2, 1, 3), "transposed")
    four = so.aggregate(volume, 16, 96, 4)
    sc.compare(so.aggregate(volume[:, :, ::-1], 16, 96, 4), four[:, :, ::-1], "4 paths flipped along W")
    sc.compare(so.aggregate(volume, 16, 96, 8, guide=np.full(volume.shape[:3], 9, np.uint8), alpha=7, p2_min=20), want, "a guide of equal bytes")


def test_three_steps_by_hand():
    """A 1 x 3 volume of 3 planes, P1 = 1, P2 = 4.  Rightwards: L(p0) = C = (5, 1, 7), m = 1; L(p1) = (2 + min(5, 2, 5) - 1,
    6 + min(1, 6, 8, 5) - 1, 0 + min(7, 2, 5) - 1) = (3, 6, 1), m = 1; L(p2) = (3 + 3 - 1, 3 + min(6, 4, 2, 5) - 1, 3 + 1 - 1) =
    (5, 4, 3).  Leftwards from p2 = (3, 3, 3): L(p1) = (2, 6, 0), L(p0) = (5 + 2, 1 + 1, 7 + 0).  Up and down the single row
    L = C."""
    cost = np.array([[[[5, 1, 7], [2, 6, 0], [3, 3, 3]]]], np.uint16)
    right, left, down, up = so.aggregate(cost, 1, 4, 4, parts=True)
    assert right[0, 0].tolist() == [[5, 1, 7], [3, 6, 1], [5, 4, 3]]
    assert left[0, 0].tolist() == [[7, 2, 7], [2, 6, 0], [3, 3, 3]]
    assert np.array_equal(down, cost) and np.array_equal(up, cost)
    assert so.aggregate(cost, 1, 4, 4)[0, 0].tolist() == [[22, 5, 28], [9, 24, 1], [14, 13, 12]]


def test_raising_uniqueness_never_accepts_and_t_is_at_most_a_half():
    rng = np.random.default_rng(3)
    total = rng.integers(0, 3000, (1, 20, 30, 16)).astype(np.uint16)
    depth = np.linspace(0, 30, 16, dtype=np.float32)[None]
    kept = np.ones((1, 20, 30), bool)
    shares = []
    for u in (0, 1, 5, 20, 50, 99):
        index = so.select(total, depth, u)[0]
        assert not ((index >= 0) & ~kept).any()
        kept = index >= 0
        shares.append(kept.mean())
    assert shares[0] == 1.0 and shares[-1] < 0.2
    for _, s, _, _ in sc.select_matrix():
        assert (np.abs(so.parabola_t(s)) <= 0.5).all()
    assert np.abs(so.parabola_t(total)).max() > 0.4


# ---- rejections --------------------------------------------------------------------------------------------------------------------
def test_python_rejections():
    """Every check of satmvs_amd.sgm comes before the first device call, so it raises without a GPU."""
    from satmvs_amd import sgm
    img = np.zeros((1, 8, 9), np.float32)
    rpc = np.zeros((1, 170))
    dv = np.linspace(0, 10, 4, dtype=np.float32)[None]
    ok = dict(ref=img, srcs=[img], ref_geo=rpc, src_geos=[rpc], depth_values=dv)
    for change in (dict(radius=0), dict(radius=4), dict(radius=2.0), dict(cov_min=float("nan")), dict(plane_chunk=0), dict(geo_model="affine"),
                   dict(srcs=[]), dict(srcs=[img] * 8, src_geos=[rpc] * 8), dict(src_geos=[rpc, rpc]), dict(srcs=[np.zeros((1, 8, 8), np.float32)]),
                   dict(ref=np.zeros((8, 9), np.float32)), dict(ref_geo=np.zeros((1, 4, 4))), dict(src_geos=[np.zeros((2, 170))]),
                   dict(geo_model="pinhole")):
        with pytest.raises(ValueError):
            sgm.census_cost(**dict(ok, **change))
    cost = np.zeros((1, 4, 5, 6), np.uint16)
    for change in (dict(paths=6), dict(paths=16), dict(p1=-1), dict(p1=97), dict(p2=-1), dict(p2_min=15), dict(p2_min=97), dict(alpha=-1), dict(alpha=65536),
                   dict(cost_max=-1), dict(void_cost=769), dict(void_cost=-1), dict(p2=65535 // 8 - 768 + 1), dict(paths=4, p2=65535 // 4 - 768 + 1),
                   dict(cost=cost.astype(np.int32)), dict(cost=cost[0]), dict(cost=np.zeros((1, 2, 2, 257), np.uint16)), dict(cost=np.zeros((1, 0, 2, 3), np.uint16)),
                   dict(guide=np.zeros((1, 4, 5), np.float32)), dict(guide=np.zeros((1, 5, 4), np.uint8)), dict(p1=1.5)):
        with pytest.raises(ValueError):
            sgm.aggregate(**dict(dict(cost=cost), **change))
    for change in (dict(uniqueness=-1), dict(uniqueness=100), dict(uniqueness=0.5), dict(min_support=-1), dict(sum=cost.astype(np.float32)),
                   dict(sum=np.zeros((4, 5, 6), np.uint16))):
        with pytest.raises(ValueError):
            sgm.select(**dict(dict(sum=cost, depth_values=np.zeros((1, 6), np.float32)), **change))
    for change in (dict(images=[img]), dict(images=[img] * 9), dict(proj_matrices=np.zeros((1, 3, 170))), dict(geo_model="pinhole"), dict(radius=5),
                   dict(p2=8000), dict(uniqueness=100), dict(void_cost=800)):
        with pytest.raises(ValueError):
            sgm.sgm_heights(**dict(dict(images=[img, img], proj_matrices=np.zeros((1, 2, 170)), depth_values=dv), **change))


def test_c_rejections_need_no_device(lib):
    """SMVS_ERR_ARG with a message before any HIP call: the pointers are never followed."""
    P = 1 << 20                                               # pointers far apart; none is read
    host = (C.c_void_p * 7)(*[P * (8 + k) for k in range(7)])
    ok = dict(ref=P, warped=host, n_src=2, radius=2, cov_min=0.999, cost=2 * P, B=1, H=8, W=9, d_begin=0, Dc=4, D=8, ws=3 * P, nbytes=1024)

    def census(**change):
        a = dict(ok, **change)
        return lib.smvs_sgm_census_cost(a["ref"], a["warped"], a["n_src"], a["radius"], a["cov_min"], a["cost"], a["B"], a["H"], a["W"], a["d_begin"],
                                        a["Dc"], a["D"], a["ws"], a["nbytes"], None)

    assert lib.smvs_sgm_census_workspace_bytes(1, 8, 9) == 768 and lib.smvs_sgm_census_workspace_bytes(0, 8, 9) == 0
    assert lib.smvs_sgm_census_workspace_bytes(1 << 15, 1 << 15, 2) == 0
    null_in = (C.c_void_p * 7)(8 * P, None, 0, 0, 0, 0, 0)
    for change in (dict(ref=None), dict(warped=None), dict(cost=None), dict(ws=None), dict(n_src=0), dict(n_src=8), dict(radius=0), dict(radius=4),
                   dict(cov_min=float("nan")), dict(B=0), dict(H=0), dict(W=-1), dict(D=0), dict(D=257), dict(d_begin=-1), dict(Dc=0), dict(d_begin=5),
                   dict(Dc=9), dict(B=1 << 10, H=1 << 10, W=1 << 10), dict(nbytes=767), dict(warped=null_in), dict(cost=P), dict(ws=P + 4), dict(cost=3 * P - 2),
                   dict(ref=8 * P + 16), dict(warped=(C.c_void_p * 7)(8 * P, 8 * P + 4 * 2 * 4 * 72 - 1, 0, 0, 0, 0, 0))):
        assert census(**change) == ERR_ARG and lib.smvs_last_error().decode(), change

    agg_ok = dict(cost=P, guide=None, sum=2 * P, B=1, H=8, W=9, D=8, P1=16, P2=96, p2_min=16, alpha=0, cost_max=768, void_cost=96, paths=8)

    def aggregate(**change):
        a = dict(agg_ok, **change)
        return lib.smvs_sgm_aggregate(a["cost"], a["guide"], a["sum"], a["B"], a["H"], a["W"], a["D"], a["P1"], a["P2"], a["p2_min"], a["alpha"],
                                      a["cost_max"], a["void_cost"], a["paths"], None)

    for change in (dict(cost=None), dict(sum=None), dict(B=0), dict(D=0), dict(D=257), dict(B=4, H=1 << 12, W=1 << 12, D=32), dict(paths=0), dict(paths=5), dict(paths=16),
                   dict(P1=-1), dict(P1=17), dict(p2_min=97), dict(P2=15, p2_min=15), dict(alpha=-1), dict(alpha=65536), dict(void_cost=-1), dict(void_cost=769),
                   dict(P2=65535 // 8 - 768 + 1), dict(paths=4, P2=65535 // 4 - 768 + 1), dict(cost_max=65535, void_cost=0, P1=0, p2_min=0, P2=0),
                   dict(sum=P), dict(sum=P + 2 * 576 - 1), dict(guide=P + 10), dict(guide=2 * P - 71)):
        assert aggregate(**change) == ERR_ARG and lib.smvs_last_error().decode(), change

    sel_ok = dict(sum=P, cost=2 * P, depth=3 * P, is4d=0, u=10, ms=1, index=4 * P, height=5 * P, min_sum=6 * P, support=7 * P, B=1, H=8, W=9, D=8)

    def select(**change):
        a = dict(sel_ok, **change)
        return lib.smvs_sgm_select(a["sum"], a["cost"], a["depth"], a["is4d"], a["u"], a["ms"], a["index"], a["height"], a["min_sum"], a["support"],
                                   a["B"], a["H"], a["W"], a["D"], None)

    for change in (dict(sum=None), dict(depth=None), dict(index=None), dict(height=None), dict(B=0), dict(D=0), dict(D=257), dict(is4d=2), dict(is4d=-1),
                   dict(u=-1), dict(u=100), dict(ms=-1), dict(cost=None), dict(index=P), dict(height=4 * P + 4), dict(min_sum=5 * P + 2), dict(support=6 * P),
                   dict(index=3 * P + 28), dict(is4d=1, index=3 * P + 4 * 576 - 4), dict(height=2 * P + 100)):
        assert select(**change) == ERR_ARG and lib.smvs_last_error().decode(), change


# ---- planted errors ----------------------------------------------------------------------------------------------------------------
def _reported(got, want, what):
    with pytest.raises(AssertionError):
        sc.compare(got, want, what)


def test_planted_errors_are_reported():
    """Each wrong rule differs from the right one somewhere on the matrix, and sc.compare says so."""
    census = [c for c in sc.census_matrix() if c[0] in ("radius 2", "equal intensities")]
    for plant in ("le", "uncovered_ignored"):
        assert census
        for name, ref, warped, radius, cov_min in census[:1]:
            _reported(so.census_cost(ref, warped, radius, cov_min, plant=plant), so.census_cost(ref, warped, radius, cov_min), plant)
    name, cost, kw = [c for c in sc.aggregate_matrix() if c[0] == "valleys"][0]
    want = so.aggregate(cost, **kw)
    for plant in ("p1_on_d", "no_minus_m", "start_zero"):
        _reported(so.aggregate(cost, plant=plant, **kw), want, plant)
    name, total, depth, kw = [c for c in sc.select_matrix() if c[0] == "few, planes, u 15 with cost"][0]
    want = so.select(total, depth, **kw)
    _reported(so.select(total, depth, plant="last_tie", **kw)[0], want[0], "last_tie")
    name, total, depth, kw = [c for c in sc.select_matrix() if c[0] == "uniqueness threshold"][0]
    _reported(so.select(total, depth, plant="unique_near", **kw)[0], so.select(total, depth, **kw)[0], "unique_near")
    name, total, depth, kw = [c for c in sc.select_matrix() if c[0] == "wide, planes"][0]
    _reported(so.select(total, depth, plant="t_den", **kw)[1], so.select(total, depth, **kw)[1], "t_den")
    _reported(np.array([np.nan], np.float32), np.array([-np.nan], np.float32), "NaNs of different bits")
    _reported(np.zeros(3, np.uint16), np.zeros(3, np.int16), "dtype")


# ---- the scene ---------------------------------------------------------------------------------------------------------------------
def test_scene_on_the_oracle():
    """The chain in numpy over torch's CPU warps (oracle/torch_composite.rpc_warping) meets the scene's conditions: median error
    within one plane spacing, 90 % within two, and better than the winner of the raw cost on both."""
    import torch
    from oracle import torch_composite as tc
    images, rpc, truth = sc.scene()
    assert abs(sc.DH - 1.915) < 0.001 and truth[0].max() - truth[0].min() > 40.0
    warped = []
    for v in (1, 2):
        fea = torch.from_numpy(np.stack([images[v], np.ones_like(images[v])])[None])
        warped.append(tc.rpc_warping(fea, torch.from_numpy(rpc[v:v + 1]), torch.from_numpy(rpc[0:1]), torch.from_numpy(sc.planes())).numpy())
    sgm, raw, cost, total = sc.oracle_heights(images[0][None], warped, sc.planes())
    assert 0.02 < (cost == sc.VOID).mean() < 0.2 and (sgm[0][0, sc.BORDER:-sc.BORDER, sc.BORDER:-sc.BORDER] >= 0).all() and (sgm[0] == -1).any()
    sc.check_quality(sgm[1][0], raw[1][0], truth[0])
