"""What tests/test_ops_gpu.py assumes about its scenes, references and checks (tests/ops_scene.py), asserted without a GPU:
the shape matrix covers the kernel's decomposition, two independent float64 evaluations of the geometry give the same
float32 coordinates, the oracle alone meets the derived float64 sampler bound, the numpy taps behind the backward reference
are the oracle's, the regression scenes' at-risk shares are small, and the checks themselves reject what they should."""
import numpy as np
import pytest

import ops_scene as osn

_ALL = osn.WARP_CASES + [osn.BIG_CASE]


# ---- the matrix ---------------------------------------------------------------------------------------------------------
def test_matrix_covers_the_decomposition():
    B, C, D, H, W = (set(c[i] for c in _ALL) for i in range(5))
    assert W >= {1, 2, 63, 64, 65, 129, 768} and H >= {1, 3, 4, 5, 33, 384} and D >= {1, 7, 8, 9, 17, 64}
    assert B >= {1, 2, 3} and C >= {1, 3, 8, 32, 33}
    assert {osn.block_count(b, d, h, w) % 8 for b, _, d, h, w in osn.WARP_CASES} == set(range(8))      # every remainder of xcd_remap
    assert osn.block_count(*[osn.BIG_CASE[i] for i in (0, 2, 3, 4)]) == 12 * 96 * 8
    # plane chunks: fewer than 8 planes, exactly one chunk, chunk + 1, several chunks + 1, whole chunks only
    assert {d if d < 8 else d % 8 for d in D} >= {1, 7, 0}
    assert any(d > 8 and d % 8 == 1 for d in D) and any(d >= 16 and d % 8 == 0 for d in D)
    # column tiles of 64: one partial, one full, full + 1, two full + 1, last column of a tile missing
    assert {w % 64 for w in W} >= {0, 1, 2, 63} and any(w > 64 and w % 64 == 1 for w in W)
    # row tiles of 4: every tail
    assert {h % 4 for h in H} >= {0, 1, 3} and any(h > 4 and h % 4 == 1 for h in H)


def test_regression_matrix_covers_the_sizes():
    cases = osn.reg_cases()
    assert {c[0] for c in cases} == set(osn.REG_D)
    assert {int(np.prod(c[1])) for c in cases} == {1, 255, 256, 257, 3 * 33 * 70}
    assert int(np.prod(osn.REG_BIG)) == 768 * 384
    for D in osn.REG_D:
        assert {c[2] for c in cases if c[0] == D} == {"planes", "tensor"}


# ---- coordinates: two float64 evaluations, one float32 answer -----------------------------------------------------------
@pytest.mark.parametrize("per_pixel", [False, True], ids=["planes", "perpixel"])
@pytest.mark.parametrize("case", osn.WARP_CASES, ids=osn.case_id)
@pytest.mark.parametrize("geo", osn.GEOS)
def test_float64_evaluations_round_alike(oracle, geo, case, per_pixel):
    B, C, D, H, W = case
    _, src, ref, depth = osn.scene(geo, B, 1, D, H, W, seed=31, per_pixel=per_pixel)
    share, dist = osn.coord_disagreement(oracle, geo, src, ref, depth, H, W)
    print("%s %s: share %.3g, float64 distance %.3g px" % (geo, osn.case_id(case), share, dist))
    assert share <= osn.MAX_EXPLAINED or share * B * D * H * W <= 1
    assert dist <= 1e-8                                                            # the project's pixel tolerance


@pytest.mark.parametrize("geo", osn.GEOS)
def test_float64_evaluations_round_alike_full_tile(oracle, geo):
    B, C, D, H, W = osn.BIG_CASE
    _, src, ref, depth = osn.scene(geo, B, 1, D, H, W, seed=32, per_pixel=True)
    share, dist = osn.coord_disagreement(oracle, geo, src, ref, depth, H, W)
    print("%s %s: share %.3g, float64 distance %.3g px" % (geo, osn.case_id(osn.BIG_CASE), share, dist))
    assert share <= osn.MAX_EXPLAINED and dist <= 1e-8


# ---- the oracle against the independent float64 sampler -------------------------------------------------------------------
_SMOOTH = [c for c in osn.WARP_CASES if c[3] > 1 and c[4] > 1]


def smooth_check(orc, geo, case, per_pixel, warped=None):
    B, C, D, H, W = case
    fea, src, ref, depth = osn.scene(geo, B, C, D, H, W, seed=33, per_pixel=per_pixel, smooth=True)
    px, py = osn.numpy_coords(geo, src, ref, depth, H, W)
    val, mag = osn.sampler_f64(fea, px, py, H, W)
    bound = osn.sampler_bound(px, py, mag, H, W)
    if warped is None:
        warped = orc.rpc_warping(fea, src, ref, depth) if geo == "rpc" else orc.homo_warping(fea, src, ref, depth)
    err = np.abs(warped.astype(np.float64) - val)
    return err, bound, val


@pytest.mark.parametrize("per_pixel", [False, True], ids=["planes", "perpixel"])
@pytest.mark.parametrize("case", _SMOOTH, ids=osn.case_id)
@pytest.mark.parametrize("geo", osn.GEOS)
def test_oracle_meets_the_float64_sampler_bound(oracle, geo, case, per_pixel):
    err, bound, val = smooth_check(oracle, geo, case, per_pixel)
    assert np.isfinite(val).all() and (np.abs(val) > 0.01).mean() > 0.2, "the scene samples mostly nothing"
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("%s %s: worst error / bound %.3g, largest error %.3g" % (geo, osn.case_id(case), worst, err.max()))
    assert (err <= bound).all(), worst
    assert bound.max() <= 1e-3                                                      # the bound says something


def test_the_sampler_bound_catches_a_wrong_tap(oracle):
    """A sampler that is one column off is outside the bound almost everywhere."""
    case = (1, 3, 9, 33, 65)
    B, C, D, H, W = case
    fea, src, ref, depth = osn.scene("rpc", B, C, D, H, W, seed=33, per_pixel=True, smooth=True)
    shifted = oracle.rpc_warping(np.roll(fea, 1, axis=3), src, ref, depth)
    err, bound, _ = smooth_check(oracle, "rpc", case, True, warped=shifted)
    assert (err > bound).mean() > 0.5


# ---- the numpy taps behind the backward reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in osn.WARP_CASES if c[1] <= 8], ids=osn.case_id)
@pytest.mark.parametrize("geo", osn.GEOS)
def test_numpy_taps_are_the_oracles(oracle, geo, case):
    """sample_from_taps (float64, from the float32 weights) is within 4 roundings of the oracle's float32 sampler at every
    voxel, dropped taps included; and the float64 scatter is the exact adjoint of that sampler."""
    B, C, D, H, W = case
    fea, src, ref, depth = osn.scene(geo, B, C, D, H, W, seed=34, per_pixel=True)
    gx, gy = osn.oracle_grid(oracle, geo, src, ref, depth, H, W)
    off, wts = osn.taps_from_grid(gx, gy, H, W)
    want = oracle.rpc_warping(fea, src, ref, depth) if geo == "rpc" else oracle.homo_warping(fea, src, ref, depth)
    mine = osn.sample_from_taps(fea, off, wts)
    mag = osn.sample_from_taps(np.abs(fea), off, wts)
    assert np.array_equal(np.isnan(mine), np.isnan(want))
    assert (np.abs(mine - want) <= 4 * osn.U32 * mag)[~np.isnan(want)].all()
    if H == 1 or W == 1:
        # (W-1)/2 = 0: the coordinate is +-inf or NaN, its fraction inf - inf = NaN; every tap is dropped (reads 0) and 0 * NaN = NaN
        assert (off < 0).all() and np.isnan(want).all()
        mine = np.zeros_like(mine)
    rng = np.random.default_rng(3)
    g = rng.standard_normal(want.shape).astype(np.float32)
    ref64, mag64, cnt = osn.scatter_f64(g, off, wts, H, W)
    lhs, rhs = float((mine * g).sum()), float((ref64 * fea.astype(np.float64)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, float((np.abs(mine) * np.abs(g)).sum()))
    assert cnt.sum() == (off >= 0).sum() // 1 and (mag64 >= np.abs(ref64) - 1e-12).all()


def test_backward_check_rejects_swapped_taps_and_stale_sums(oracle):
    B, C, D, H, W = 1, 3, 9, 33, 65
    fea, src, ref, depth = osn.scene("rpc", B, C, D, H, W, seed=35, per_pixel=True)
    gx, gy = osn.oracle_grid(oracle, "rpc", src, ref, depth, H, W)
    off, wts = osn.taps_from_grid(gx, gy, H, W)
    g = np.random.default_rng(4).standard_normal((B, C, D, H, W)).astype(np.float32)
    good, _, _ = osn.scatter_f64(g, off, wts, H, W)
    assert not osn.check_backward(good.astype(np.float32), g, off, wts, H, W)[0]
    swapped, _, _ = osn.scatter_f64(g, off[[0, 2, 1, 3]], wts, H, W)                # south-west and north-east offsets exchanged
    assert osn.check_backward(swapped.astype(np.float32), g, off, wts, H, W)[0]
    assert osn.check_backward((2 * good).astype(np.float32), g, off, wts, H, W)[0]  # a second backward on top of the first


# ---- the explained-difference rule itself ---------------------------------------------------------------------------------
def test_explain_rule_accepts_an_ulp_and_nothing_else(oracle):
    B, C, D, H, W = 1, 3, 2, 9, 20
    fea, src, ref, depth = osn.scene("rpc", B, C, D, H, W, seed=36, per_pixel=True)
    want = oracle.rpc_warping(fea, src, ref, depth)
    assert osn.explain_warp(oracle, "rpc", want, want, fea, src, ref, depth) == ([], 0)
    samp, line = osn.oracle_coords(oracle, "rpc", src, ref, depth, H, W)
    px, py = samp.astype(np.float32), line.astype(np.float32)
    v = (0, 1, 4, 7)
    px[v] = np.nextafter(px[v], np.float32(np.inf))
    gx, gy = osn.grid_from_pixel32(px, py, H, W)
    moved = oracle.grid_sample(fea, np.stack([gx, gy], -1).reshape(B, D * H, W, 2)).reshape(B, C, D, H, W)
    assert (moved != want).any()
    msgs, n = osn.explain_warp(oracle, "rpc", moved, want, fea, src, ref, depth)
    assert not msgs and n == 1
    wrong = want.copy()
    wrong[0, :, 1, 4, 7] = want[0, :, 1, 4, 8]                                       # the neighbouring pixel's value: not an ulp
    msgs, _ = osn.explain_warp(oracle, "rpc", wrong, want, fea, src, ref, depth)
    assert msgs
    nan = want.copy()
    nan[0, 0, 0, 0, 0] = np.nan
    assert osn.explain_warp(oracle, "rpc", nan, want, fea, src, ref, depth)[0]
    many = want.copy()
    many[0, 0, 0, :2, :] += 1                                                       # more than the cap
    assert osn.explain_warp(oracle, "rpc", many, want, fea, src, ref, depth)[0]


# ---- regressions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", osn.reg_cases() + [(48, osn.REG_BIG, "tensor"), (64, osn.REG_BIG, "planes")],
                         ids=lambda c: "D%d-%s-%s" % (c[0], "x".join(map(str, c[1])), c[2]))
def test_regression_scenes_at_risk_share_and_oracle_distance(oracle, case):
    D, bhw, kind = case
    reg, heights = osn.reg_scene(D, bhw, kind, seed=40 + D)
    f64 = osn.regress_f64(reg, heights, lamb=1.5)
    share = float(osn.at_risk(f64, D).mean())
    n = int(np.prod(bhw))
    print("D=%d n=%d: at-risk share %.3g (band %.3g)" % (D, n, share, osn.index_band(D)))
    assert share <= osn.MAX_AT_RISK or share * n <= 1
    od, oc, ov = oracle.window_regress(reg, heights, lamb=1.5)
    msgs, excused = osn.check_window_conf(oc, f64, D)                                  # the oracle passes the rule the kernel is held to
    assert not msgs, msgs
    sd, sc = oracle.softmax_regress(reg, heights)
    assert np.array_equal(sd, od)
    assert np.abs(sc - f64["conf_max"]).max() <= 1e-5 * 1 + 1e-6
    print("oracle: depth %.3g m, spread %.3g from float64; %.3g excused" % (np.abs(od - f64["depth"]).max(), np.abs(ov - f64["var"]).max(), excused))
    assert np.abs(od - f64["depth"]).max() <= D * osn.U32 * 400.0 * 2                  # D products and additions of values up to 400


def test_window_check_rejects_a_narrow_window(oracle):
    """A window that stops at idx + 1 is off by p[idx+2] at most pixels: not excused."""
    D, bhw = 48, (1, 16, 16)
    reg, heights = osn.reg_scene(D, bhw, "planes", seed=41)
    f64 = osn.regress_f64(reg, heights)
    idx = np.clip(np.trunc(f64["fidx"]).astype(np.int64), 0, D - 1)
    last = np.where(idx + 2 < D, np.take_along_axis(f64["p"], np.clip(idx + 2, 0, D - 1)[:, None], 1)[:, 0], 0.0)
    assert osn.check_window_conf((f64["conf_win"] - last).astype(np.float32), f64, D)[0]


def test_stream_reference_is_the_oracles(oracle):
    D, (B, H, W) = 17, (2, 5, 9)
    reg, heights = osn.reg_scene(D, (B, H, W), "tensor", seed=42)
    acc = oracle.StreamRegress(B, H, W)
    for d in range(D):
        acc.step(reg[:, d], heights, d)
    es, di, mx = osn.stream_f64(reg, heights)
    np.testing.assert_allclose(acc.exp_sum[:, 0], es, rtol=1e-13)
    np.testing.assert_allclose(acc.depth_img[:, 0], di, rtol=1e-12)
    np.testing.assert_allclose(acc.max_prob[:, 0], mx, rtol=1e-13)


# ---- composition -----------------------------------------------------------------------------------------------------------------
def test_pivot_matrices_need_their_swaps_and_the_oracle_is_inside_the_bound(oracle):
    mats = osn.pivot_matrices()
    for col, m in enumerate(mats[:3]):
        a = m.copy()
        for k in range(col):                                                       # eliminate the columns before, no swap needed there
            assert a[k, k] != 0 and abs(a[k, k]) >= np.abs(a[k + 1:, k]).max()
            for r in range(k + 1, 4):
                a[r] = a[r] - a[r, k] / a[k, k] * a[k]
        assert a[col, col] == 0 and np.abs(a[col + 1:, col]).max() > 0, (col, a)
        assert abs(np.linalg.det(m)) > 1
    src = np.arange(1.0, 17.0).reshape(4, 4)
    for m in mats:
        got = oracle.homo_compose(src[None], m[None])[0]
        want = src @ np.linalg.inv(m)
        assert np.abs(got - want).max() <= osn.compose_bound(src, m)
    for p in mats[3:]:
        assert np.array_equal(oracle.homo_compose(src[None], p[None])[0], src @ p.T)  # a permutation: exact
    s, r = osn.compose_scene(65, seed=5)
    got = oracle.homo_compose(s, r)
    for i in range(65):
        assert np.abs(got[i] - s[i] @ np.linalg.inv(r[i])).max() <= osn.compose_bound(s[i], r[i])
