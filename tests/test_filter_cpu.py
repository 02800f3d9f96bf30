"""The scenes and checks of tests/filter_scene.py on the CPU: what tests/test_filter_gpu.py and tests/fuzz/fuzz_filter.py take
for granted about their scenes is asserted here from the oracle alone -- the maps are consistent, both mask values occur, the
blunder patch is rejected, the at-risk share is under the project's caps (1e-3 RPC, 2e-3 pinhole), no pixel sits close to a
threshold of the mask rule -- and the checks themselves pass on the oracle and fail on a wrong implementation.

The pinhole at-risk set is narrower than "one float32 ulp moves the fixed-point coordinate": that set holds
2 * 32 * ulp(c) of the pixels per coordinate for ANY implementation (1.3e-2 at 2048 x 2304, 3.5e-3 at 384 x 768; printed by
test_pinhole_ulp_share_is_a_property_of_the_size), which passes the 2e-3 cap from about 250 pixels on.  The set used,
Pinhole.at_risk, bounds the float64 forward error of the coordinate instead; it lies inside the one-ulp set, so "differing
pixels are a subset of it" asks more."""
import numpy as np
import pytest

import filter_scene as fs


def _kinds_pairs():
    return [(k, r, s) for k in ("rpc", "pinhole") for r, s in fs.PAIRS + (fs.BIG,)]


@pytest.mark.parametrize("kind,ref,src", _kinds_pairs(), ids=lambda v: str(v).replace(" ", ""))
def test_scene_caps_and_empty_exception_sets(oracle, kind, ref, src):
    g, dr, ds, p, d = fs.pair(kind, oracle, ref, src)
    big = (ref, src) == fs.BIG
    msgs, share, diff = fs.end_to_end(g, fs.OracleModule(oracle, kind), dr, ds, p, d)
    print("%s %s <- %s: at-risk share %.3g" % (kind, ref, src, share))
    assert not msgs and not diff.any() and share <= g.cap
    assert not fs.near_threshold(g, dr, ds, p, d).any()
    if not big:
        assert not fs.stages(g, fs.OracleModule(oracle, kind), dr, ds, p, d)
    mask = g.oracle_check(dr, ds, p, d)[0]
    if min(ref) >= 64:
        pr, pc = fs.patch(*src)
        assert mask.any() and not mask.all() and mask.mean() > 0.3
        cx, cy = g.coords(dr)                                               # the blunder patch of the source is rejected
        inner = (cx > pc.start + 2) & (cx < pc.stop - 3) & (cy > pr.start + 2) & (cy < pr.stop - 3)
        assert inner.sum() >= 5 and not mask[inner].any()


@pytest.mark.parametrize("size", fs.SIZES + ((40, 61), (300, 333)))
def test_scene_builder_is_consistent(size):
    H, W = size
    depths, rpcs, prob, h64 = fs.rpc_scene((size, size), seed=1)
    for v in range(2):
        assert fs.rpc_residual(rpcs[v], h64[v]).max() < 1e-6
        assert depths[v].dtype == np.float32 and depths[v].shape == size
    assert prob.shape == size and prob.dtype == np.float32
    pd, K, E = fs.pinhole_scene((size, size), seed=1, blunder=0)
    for v in range(2):                                                      # the pixel's ray at its depth ends on the surface
        vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        d = pd[v].astype(np.float64)
        Xw = np.linalg.inv(fs._proj(K[v], E[v])) @ np.vstack(((d * uu).ravel(), (d * vv).ravel(), d.ravel(), np.ones(H * W)))
        assert np.abs(Xw[2] - fs.pin_surface(Xw[0], Xw[1])).max() < 1e-3      # float32 depths of about 400: half an ulp is 1.5e-5


@pytest.mark.parametrize("V", sorted(fs.FILTER_VIEWS))
def test_filter_depth_scenes(oracle, V):
    sizes = fs.FILTER_VIEWS[V]
    depths, rpcs, prob, _ = fs.rpc_scene(sizes, seed=2)
    for v in range(1, V):
        g = fs.Rpc(oracle, rpcs[0], rpcs[v])
        cx, cy = g.coords(depths[0])
        assert g.at_risk(depths[0], cx, cy).mean() <= fs.RPC_CAP
        assert not fs.near_threshold(g, depths[0], depths[v], *fs.RPC_PARAMS).any()
    seen = set()
    for n in range(1, V):
        f, a = oracle.filter_depth(depths, rpcs, 1.0, 2.5, n, prob=prob, confidence_ratio=0.3)
        assert f.shape == sizes[0] and a.dtype == np.float64
        assert not f[:sizes[0][0] // 8, :sizes[0][1] // 8].any()              # the low-confidence corner
        seen |= set(np.unique(f).tolist())
    assert seen == {False, True}


@pytest.mark.parametrize("hw", fs.SHIFT_SIZES, ids=str)
@pytest.mark.parametrize("shift", fs.SHIFTS, ids=str)
def test_known_answers_against_the_oracle_remap(oracle, hw, shift):
    dr, ref, src_map, src, xs, ys, val = fs.shift_case(hw[0], hw[1], *shift)
    got = oracle.remap_linear_const(src_map, xs, ys, border=0.0)
    assert np.array_equal(got.view(np.uint32), val.view(np.uint32))
    dep, xb, yb, oxs, oys = oracle.pinhole_reproject_with_depth(dr, *ref, src_map, *src)
    assert np.array_equal(oxs, xs) and np.array_equal(oys, ys) and np.array_equal(dep.view(np.uint32), val.view(np.uint32))
    t, w = fs.taps(src_map, xs, ys, 0.0)
    assert np.array_equal((t[0] * w[0] + t[1] * w[1] + t[2] * w[2] + t[3] * w[3]).view(np.uint32), val.view(np.uint32))


def test_known_answers_cover_what_they_claim():
    ties = neg = half = out = 0
    for tx, ty in fs.SHIFTS:
        ties += (tx * 64) % 2 == 1 and (ty * 64) % 2 == 1
        neg += -1 < tx < 0 or -1 < ty < 0
        half += tx % 1 == 0.5 or ty % 1 == 0.5
        out += abs(tx) > 400 or abs(ty) > 400
    assert ties >= 5 and neg >= 2 and half >= 1 and out >= 3
    # round half to even, both ways: 32 (x + 1/64) = 32 x + 1/2 -> 32 x; 32 (x + 3/64) = 32 x + 3/2 -> 32 x + 2
    assert fs.fixed(np.float32(5 + 1 / 64)) == 160 and fs.fixed(np.float32(5 + 3 / 64)) == 162 and fs.fixed(np.float32(-1 / 64)) == 0
    assert fs.fixed(np.float32(-3 / 64)) == -2 and fs.fixed(np.float32(-2)) >> 5 == -2 and (fs.fixed(np.float32(-33 / 64)) >> 5, fs.fixed(np.float32(-33 / 64)) & 31) == (-1, 16)


def test_oracle_remap_takes_the_border_at_non_finite_coordinates(oracle):
    img = np.arange(1, 13, dtype=np.float32).reshape(3, 4)
    c = np.array([[np.nan, np.inf, -np.inf, 1e12, -1e12, 3e9, 1.0]], np.float32)
    for border in (-999.0, 0.0):
        for x, y in ((c, np.full_like(c, 1.25)), (np.full_like(c, 1.25), c), (c, c)):
            with np.errstate(invalid="ignore", over="ignore"):
                got = oracle.remap_linear_const(img, x, y, border=border)
            assert (got[0, :6] == np.float32(border)).all() and got[0, 6] != np.float32(border)


def test_pinhole_ulp_share_is_a_property_of_the_size(oracle):
    """The one-ulp set grows with the coordinates whatever the implementation; the set the tests use stays empty."""
    for ref in ((64, 96), (384, 768)):
        g, dr, ds, p, d = fs.pair("pinhole", oracle, ref, ref)
        cx, cy = g.coords(dr)
        ulp, strict = g.at_risk_ulp(cx, cy), g.at_risk(dr, cx, cy)
        print("pinhole %s: one-ulp share %.3g, forward-error share %.3g" % (ref, ulp.mean(), strict.mean()))
        assert not (strict & ~ulp).any()
    assert ulp.mean() > fs.PIN_CAP                                           # 384 x 768: no scene of this size passes the cap


class _Wrong:
    """The oracle with one defect, under the product module's names."""
    def __init__(self, orc, kind, defect):
        self.orc, self.kind, self.defect, self.base = orc, kind, defect, fs.OracleModule(orc, kind)

    def reproject_with_depth(self, *a):
        dep, xb, yb, xs, ys = self.base.reproject_with_depth(*a)
        if self.defect == "nan->pixel00":
            src = np.asarray(a[2] if self.kind == "rpc" else a[3], np.float32)
            dep = np.where(np.isnan(xs), src[0, 0], dep).astype(np.float32)
        elif self.defect == "sample":
            dep = dep.copy()
            dep[dep.shape[0] // 2, dep.shape[1] // 2] *= np.float32(1 + 2.0 ** -20)
        elif self.defect == "coords":
            xs = xs + (3e-8 if self.kind == "rpc" else 4 * np.spacing(xs))
        return dep, xb, yb, xs, ys

    def check_geometric_consistency(self, *a):
        m, dm, xs, ys = self.base.check_geometric_consistency(*a)
        if self.defect == "mask":
            m = m.copy()
            m[0, 0] = ~m[0, 0]
        elif self.defect == "coords":
            xs = xs + (3e-8 if self.kind == "rpc" else 4 * np.spacing(xs))
        return m, dm, xs, ys


@pytest.mark.parametrize("kind", ["rpc", "pinhole"])
def test_checks_fail_on_a_wrong_implementation(oracle, kind):
    g, dr, ds, p, d = fs.pair(kind, oracle, (64, 96), (40, 61))
    for defect in ("sample", "coords", "mask"):
        assert fs.stages(g, _Wrong(oracle, kind, defect), dr, ds, p, d), defect
        assert fs.end_to_end(g, _Wrong(oracle, kind, defect), dr, ds, p, d)[0], defect
    bad = fs.spoil(dr, np.nan, "patch")
    assert not fs.stages(g, fs.OracleModule(oracle, kind), bad, ds, p, d)
    assert fs.stages(g, _Wrong(oracle, kind, "nan->pixel00"), bad, ds, p, d)
    assert fs.end_to_end(g, _Wrong(oracle, kind, "nan->pixel00"), bad, ds, p, d, cap=False)[0]


@pytest.mark.parametrize("kind", ["rpc", "pinhole"])
def test_checks_pass_on_the_oracle_with_spoilt_maps(oracle, kind):
    g, dr, ds, p, d = fs.pair(kind, oracle, (64, 96), (40, 61))
    om = fs.OracleModule(oracle, kind)
    for what in fs.SPOILS:
        for where in ("patch", "all"):
            for a, b in ((fs.spoil(dr, what, where), ds), (dr, fs.spoil(ds, what, where))):
                assert not fs.stages(g, om, a, b, p, d), (what, where)
                assert not fs.end_to_end(g, om, a, b, p, d, cap=False)[0], (what, where)
                m, dm, _, _ = g.oracle_check(a, b, p, d)
                assert not np.isnan(dm).any()
    g, dr, ds, p, d = fs.pair(kind, oracle, (64, 96), (64, 96), away=True)
    dep = g.oracle_reproject(dr, ds)[0]
    assert (dep == np.float32(g.border)).all() and not g.oracle_check(dr, ds, p, d)[0].any()
