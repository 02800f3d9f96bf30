"""The zonal order statistics without a device: the two numpy statements of the rule (tests/dsm_quantile_oracle.py) against each
other, the integer ranks of satmvs_amd.dsm.quantile_ranks against Fraction arithmetic and against numpy's own quantiles, the
invariants of the rule, every Python argument rejection, and six planted mistakes that the comparison has to report."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import dsm_quantile_oracle as qo
from dsm_testkit import f2key, same_bits, valid
from satmvs_amd import dsm
from satmvs_amd.dsm import compare_dsms_robust, dsm_metrics_robust, label_nmad, label_quantiles, quantile_ranks  # noqa: F401  (the names under test)

QS = (0, Fraction(1, 4), Fraction(1, 3), Fraction(1, 2), 0.6827, 0.9, 0.95, 1)
NUMPY_QS = (0.0, 0.25, 0.5, 0.6827, 0.9, 0.95, 1.0)
RANK_SETS = ((1, 0), (2, 1), (7, 2), (8, 3))                 # (n_ranks, the kind the columns start at)


# ---- the two statements ----------------------------------------------------------------------------------------------------------
def test_the_two_statements_agree():
    seen = 0
    for c in qo.matrix():
        m = qo.n_valid(c["labels"], c["values"], c["n"], c["nodata"], c["centre"])
        for R, turn in RANK_SETS:
            if c["labels"].size > 10000 and R not in (2, 8):                   # the descent costs 32 R passes with np.add.at
                continue
            r = qo.rank_matrix(m, R, turn)
            a = qo.select_sorted(c["labels"], c["values"], c["n"], r, c["nodata"], c["centre"])
            b = qo.select_descent(c["labels"], c["values"], c["n"], r, c["nodata"], c["centre"])
            d = qo.differing(*b, *a)
            assert d is None, (c["name"], R, d)
            assert np.array_equal(a[1], m)
            seen += 1
    assert seen > 100


# ---- ranks -----------------------------------------------------------------------------------------------------------------------
def test_quantile_ranks_against_fractions():
    m = np.arange(0, 301, dtype=np.int32)
    want = qo.ranks(m, QS)
    for kind, got in (("numpy", quantile_ranks(m, QS)), ("torch", quantile_ranks(torch.from_numpy(m), QS))):
        got = [np.asarray(g) for g in got]
        assert [g.dtype for g in got] == [np.int32, np.int32, np.int64, np.int64], kind
        for g, w, name in zip(got, want, ("lo", "hi", "rem", "den")):
            assert np.array_equal(g, w), (kind, name, np.argwhere(g != w)[:3].tolist())
    lo, hi, rem, den = want
    assert (lo[0] == -1).all() and (hi[0] == -1).all() and (rem[0] == 0).all()
    assert den.tolist() == [1, 4, 3, 2, 10000, 10, 20, 1]


def test_quantile_ranks_do_not_overflow():
    big = 2 ** 31 - 1
    qs = (Fraction(65535, 65536), (1, 65536), Fraction(32767, 65536), 1)
    want = [qo.ranks_of(big, q) for q in qs]
    assert want[0][0] == (big - 1) * 65535 // 65536 and want[0][0] > 2 ** 30
    for m in (np.array([big, 0, 1], np.int32), torch.tensor([big, 0, 1], dtype=torch.int32), np.array([big, 0, 1], np.int64)):
        lo, hi, rem, den = [np.asarray(t) for t in quantile_ranks(m, qs)]
        assert [(int(lo[0, i]), int(hi[0, i]), int(rem[0, i]), int(den[i])) for i in range(len(qs))] == want
        assert lo[1].tolist() == [-1] * len(qs) and lo[2].tolist() == [0] * len(qs) and hi[2].tolist() == [0] * len(qs)


def _samples(count, seed, heights):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        m = int(rng.integers(1, 60))
        x = rng.uniform(127.5, 132.5, m) if heights else rng.normal(0.0, 50.0, m)
        yield x.astype(np.float32)


def _order_statistics(x, qs):
    """lo, hi, the ranks and the linear value of one sample through the package's ranks and the oracle's selection."""
    m = np.array([len(x)], np.int32)
    lo_rank, hi_rank, rem, den = quantile_ranks(m, qs)
    zone = np.ones((1, len(x)), np.int32)
    lo, _ = qo.select_sorted(zone, x[None], 1, lo_rank)
    hi, _ = qo.select_sorted(zone, x[None], 1, hi_rank)
    return lo[0], hi[0], qo.value(lo, hi, lo_rank, rem, den, "linear")[0]


def test_lo_and_hi_are_numpys_lower_and_higher():
    for x in _samples(2000, 1, heights=False):
        lo, hi, _ = _order_statistics(x, NUMPY_QS)
        assert same_bits(lo, np.quantile(x, NUMPY_QS, method="lower")), (len(x), lo)
        assert same_bits(hi, np.quantile(x, NUMPY_QS, method="higher")), (len(x), hi)


def test_linear_is_numpys_linear_within_its_roundings():
    """Within 8 float64 ulps of M = max(|lo|, |hi|).  With a, b the two order statistics as float64, t = rem / den and u = 2^-53:
    the rule computes a + (b - a) t.  b - a is exact here (float32 values less than 29 binades apart); t and the product are
    rounded once each, |b - a| 2 u together, and the sum once, ulp(M) / 2.  numpy takes t as the fraction of the position
    (m - 1) q computed in float64 and evaluates a + (b - a) t, or b - (b - a) (1 - t) from t = 1/2 on: the product |b - a| u,
    1 - t another |b - a| u / 2, the sum ulp(M) / 2, and t itself off by dt: 0 where (m - 1) q is exact in float64 (q of 0,
    1/4, 1/2 and 1), else at most 58 u for q as a float plus 2^-48 for the product (below 64), under 2^-46.5.  The two differ by
    at most ulp(M) + |b - a| (3.5 u + dt).
    First family, every q: heights of 130 +- 2.5 m, so |b - a| <= 5 and ulp(M) >= 2^-46: 1 + 5 (3.5 x 2^-7 + 2^-0.5) < 4.7 ulps.
    Second family, the exact q only, values of any sign: |b - a| <= 2 M and M u <= ulp(M), so 1 + 2 x 3.5 = 8 ulps."""
    exact_qs = (0.0, 0.25, 0.5, 1.0)
    for heights, qs in ((True, NUMPY_QS), (False, exact_qs)):
        worst = 0.0
        for x in _samples(2000, 2 + heights, heights):
            lo, hi, got = _order_statistics(x, qs)
            want = np.quantile(x.astype(np.float64), qs)
            M = np.maximum(np.abs(lo), np.abs(hi)).astype(np.float64)
            ulps = np.abs(got - want) / np.spacing(M)
            worst = max(worst, float(ulps.max()))
            assert (ulps <= 8.0).all(), (heights, len(x), ulps.tolist())
        print("linear against numpy, heights %s: at most %.3g ulps" % (heights, worst))


def test_every_method_in_torch_is_the_oracles():
    rng = np.random.default_rng(4)
    m = rng.integers(0, 40, 200).astype(np.int32)
    lo_rank, hi_rank, rem, den = qo.ranks(m, QS)
    lo = rng.normal(100.0, 30.0, lo_rank.shape).astype(np.float32)
    hi = (lo + np.abs(rng.normal(0.0, 5.0, lo.shape))).astype(np.float32)
    for method in qo.METHODS:
        want = qo.value(lo, hi, lo_rank, rem, den, method)
        got = dsm._quantile_value(torch.from_numpy(lo), torch.from_numpy(hi), torch.from_numpy(lo_rank), torch.from_numpy(rem), torch.from_numpy(den), method)
        assert np.array_equal(got.numpy().view(np.uint64), want.view(np.uint64)), method
    # nearest: below, above, and on a tie the even rank
    one = lambda r, d, k: float(qo.value(np.float32([1.0]), np.float32([2.0]), np.array([k]), np.array([r]), np.array([d]), "nearest")[0])
    assert one(1, 4, 0) == 1.0 and one(3, 4, 0) == 2.0 and one(1, 2, 0) == 1.0 and one(1, 2, 1) == 2.0
    assert dsm.QUANTILE_METHODS == qo.METHODS


# ---- invariants ------------------------------------------------------------------------------------------------------------------
def test_invariants_of_the_rule():
    for c in qo.matrix(large=False):
        lab, v, n, nd = c["labels"], c["values"], c["n"], c["nodata"]
        if c["centre"] is not None or n == 0 or n > 500:
            continue
        qs = (0, Fraction(1, 10), 0.25, 0.5, 0.6827, 0.9, 1)
        res = qo.quantiles(lab, n, v, qs, "linear", None, nd)
        ok = valid(v, nd)
        perm = np.random.default_rng(1).permutation(lab.size)
        again = qo.quantiles(lab.reshape(-1)[perm].reshape(lab.shape), n, v.reshape(-1)[perm].reshape(v.shape), qs, "linear", None, nd)
        for key in res:
            assert np.array_equal(np.asarray(res[key]).view(np.uint8), np.asarray(again[key]).view(np.uint8)), (c["name"], key, "a permutation of the cells")
        for k in range(n):
            mine = v[(lab == k + 1) & ok]
            assert res["n_valid"][k] == mine.size
            if mine.size == 0:
                assert same_bits(res["lo"][k], np.full(len(qs), nd, np.float32)) and np.isnan(res["value"][k]).all()
                continue
            keys = f2key(mine)
            # q = 0 and q = 1: label_stats' vmin and vmax, the cells of the lowest and the highest key
            assert same_bits(res["lo"][k, :1], mine[np.argmin(keys)][None]) and same_bits(res["hi"][k, -1:], mine[np.argmax(keys)][None]), c["name"]
            mine_bits = set(mine.view(np.uint32).tolist())
            assert set(res["lo"][k].view(np.uint32).tolist()) <= mine_bits and set(res["hi"][k].view(np.uint32).tolist()) <= mine_bits, c["name"]
            for name in ("lo", "hi"):
                kk = f2key(res[name][k]).astype(np.int64)
                assert (np.diff(kk) >= 0).all(), (c["name"], name, "monotone in q")
            assert (f2key(res["lo"][k]) <= f2key(res["hi"][k])).all()


def test_mad_of_a_constant_zone_is_plus_zero():
    lab = qo.random_labels(20, 30, 3, seed=1)
    for const in (130.25, -7.5, 0.0, -0.0):
        s = qo.nmad(lab, 3, np.full(lab.shape, const, np.float32))
        assert (s["n_valid"] > 0).all()
        assert np.array_equal(s["mad"].view(np.uint64), np.zeros(3, np.uint64)) and np.array_equal(s["nmad"].view(np.uint64), np.zeros(3, np.uint64))
        assert np.array_equal(s["median"], np.full(3, const))


def test_robust_figures_of_a_planted_error_field():
    """The oracle's own end-to-end statement on a case whose answer is known by counting."""
    errors = np.array([-3.0, -1.0, -0.5, 0.0, 0.0, 0.25, 0.5, 1.0, 2.0, 40.0], np.float32)
    gt = np.full((20, 30), 100.0, np.float32)
    field = np.resize(errors, gt.shape).astype(np.float32)          # 600 cells: every value 60 times
    r = qo.metrics_robust(gt + field, gt)
    assert r["n"] == 600 and r["median"] == 0.125                   # ranks 299 and 300: 0.0 and 0.25
    # |d| sorted: 0 x 120, 0.25 x 60, 0.5 x 120, 1 x 120, 2 x 60, 3 x 60, 40 x 60; 599 x 0.9 = 539.1: a tenth of the way from 3 to 40
    assert r["le68"] == 1.0 and r["le90"] == 3.0 + 37.0 * (1.0 / 10.0) and r["le95"] == 40.0
    # |d - 0.125| sorted: 0.125 x 180, 0.375 x 60, 0.625 x 60, 0.875 x 60, ...: ranks 299 and 300 are 0.625 and 0.875
    assert r["nmad"] == 1.4826 * 0.75
    assert set(r) == {"n", "median", "nmad", "le68", "le90", "le95"}


# ---- argument rejections (before any device work) -----------------------------------------------------------------------------------
def test_python_argument_rejections():
    lab = np.ones((4, 5), np.int32)
    v = np.ones((4, 5), np.float32)
    bad_q = [(-0.1,), (1.5,), (Fraction(3, 2),), ((1, 65537),), (Fraction(1, 2 ** 16 + 1),), (float("nan"),), (), ((1, 0),), ("half",), ((1, 2, 3),), (True,)]
    for q in bad_q:
        with pytest.raises(ValueError):
            quantile_ranks(np.array([3], np.int32), q)
        with pytest.raises(ValueError):
            label_quantiles(lab, 1, v, q)
        with pytest.raises(ValueError):
            dsm_metrics_robust(v, v, levels=q)
    for m in (np.array([3.0]), np.array([[3]], np.int32), torch.tensor([1.5]), np.array([-1], np.int32), np.array([2 ** 31], np.int64)):
        with pytest.raises(ValueError):
            quantile_ranks(m, (0.5,))
    rejected = [dict(labels=lab.astype(np.int64)), dict(labels=lab[0]), dict(values=v.astype(np.float64)), dict(values=v[:, :4]), dict(values=v[0]),
                dict(n=-1), dict(n=1.0), dict(n=True), dict(method="cubic"), dict(method=None),
                dict(centre=np.zeros(2, np.float32)), dict(centre=np.zeros((1, 1), np.float32)), dict(centre=np.zeros(1, np.float64)),
                dict(centre=torch.zeros(3)), dict(n=2 ** 27 + 1, q=(0.1, 0.2, 0.3, 0.4))]
    for kw in rejected:
        args = dict(labels=lab, n=1, values=v)
        args.update(kw)
        with pytest.raises(ValueError):
            label_quantiles(**args)
    with pytest.raises(ValueError):
        label_nmad(lab.astype(np.int16), 1, v)
    with pytest.raises(ValueError):
        label_nmad(lab, 1, v.astype(np.float16))


# ---- planted mistakes --------------------------------------------------------------------------------------------------------------
def _planted_case():
    """Three zones: negatives and positives with both zeros; heights with nodata cells; a few distinct values with duplicates."""
    lab = np.repeat(np.array([[1], [2], [3]], np.int32), 12, axis=1)
    v = np.array([[-5.0, -2.0, -0.0, 0.0, 0.0, -0.0, 1.0, 3.0, -7.5, 4.0, -1.0, 2.0],
                  [130.0, 131.0, -999.0, 132.0, 129.5, -999.0, 128.0, 133.0, 127.0, -999.0, 134.0, 135.0],
                  [5.0, 5.0, 7.0, 7.0, 7.0, 9.0, 9.0, 5.0, 9.0, 9.0, 7.0, 5.0]], np.float32)
    return lab, v, 3


@pytest.mark.parametrize("plant,first", [("ceil_lo", 1), ("hi_always_next", 1), ("zeros_tied", 1), ("raw_bit_order", 1), ("nodata_counted", 2), ("descent_lt", 1)])
def test_planted_mistakes_are_reported(plant, first):
    lab, v, n = _planted_case()
    qs = (0, Fraction(1, 4), Fraction(1, 3), Fraction(1, 2), 0.9, 1)
    select = qo.select_descent if plant == "descent_lt" else qo.select_sorted
    want = qo.quantiles(lab, n, v, qs, select=select)
    sound = qo.quantiles(lab, n, v, qs, select=qo.select_descent)
    for key in ("lo", "hi"):
        assert qo.differing(sound[key], sound["n_valid"], want[key], want["n_valid"]) is None
    wrong = qo.quantiles(lab, n, v, qs, plant=plant, select=select)
    reports = [qo.differing(wrong[key], wrong["n_valid"], want[key], want["n_valid"]) for key in ("lo", "hi")]
    hit = [r for r in reports if r is not None]
    assert hit, plant
    assert min(r["label"] for r in hit) == first, (plant, hit)
    assert all(r["got"] != r["want"] or r["got_bits"] != r["want_bits"] or r["got_nvalid"] != r["want_nvalid"] for r in hit)
    assert plant in qo.PLANTS and len(qo.PLANTS) == 6
