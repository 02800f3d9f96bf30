"""The rule of the zonal order statistics (include/satmvs.h, "Zonal order statistics") in numpy, stated twice:

  select_sorted   per label, the keys of the cells that count, sorted, and an index at the rank
  select_descent  the descent over the 32 key bits on counts, all labels at once with np.add.at

and around them the ranks of a quantile in Python Fractions, the deviation mode, every `method`, NMAD in its two steps and the
robust accuracy figures.  numpy only: nothing here imports torch or the package.  `plant` puts one named mistake into a statement,
for the tests that show the comparison notices it."""
import math
from fractions import Fraction

import numpy as np

from dsm_testkit import f2key, key2f, valid

MAX_DEN = 1 << 16
METHODS = ("linear", "lower", "higher", "midpoint", "nearest")
PLANTS = ("ceil_lo", "hi_always_next", "zeros_tied", "raw_bit_order", "nodata_counted", "descent_lt")


# ---- which cells count, and their keys -------------------------------------------------------------------------------------------
def cells(labels, values, n, nodata=-999.0, centre=None, plant=None):
    """-> (k (int64: label - 1), key (uint32)) of the cells that count, in raster order.  With centre (n) float32 the keys are those
    of d = float32(|float64(v) - float64(centre[k])|), and a label whose centre is not finite has no cell."""
    lab = np.asarray(labels, np.int32).reshape(-1).astype(np.int64)
    v = np.ascontiguousarray(values, np.float32).reshape(-1)
    ok = (lab >= 1) & (lab <= n)
    ok &= np.isfinite(v) if plant == "nodata_counted" else valid(v, nodata)
    k = lab[ok] - 1
    v = v[ok]
    if centre is not None:
        c = np.asarray(centre, np.float32)
        assert c.shape == (n,)
        fin = np.isfinite(c[k])
        k, v = k[fin], v[fin]
        with np.errstate(over="ignore"):
            v = np.abs(v.astype(np.float64) - c[k].astype(np.float64)).astype(np.float32)
    if plant == "raw_bit_order":
        key = np.ascontiguousarray(v).view(np.uint32) ^ np.uint32(0x80000000)      # right for positives, backwards for negatives
    elif plant == "zeros_tied":
        key = f2key(np.where(v == 0.0, np.float32(0.0), v))
    else:
        key = f2key(v)
    return k, key.astype(np.uint32)


def n_valid(labels, values, n, nodata=-999.0, centre=None):
    k, _ = cells(labels, values, n, nodata, centre)
    return np.bincount(k, minlength=n).astype(np.int32)


# ---- statement (a): sort and index ----------------------------------------------------------------------------------------------
def select_sorted(labels, values, n, ranks, nodata=-999.0, centre=None, plant=None):
    """ranks (n, R) int -> (out (n, R) float32, nvalid (n) int32)."""
    ranks = np.asarray(ranks, np.int64)
    assert ranks.ndim == 2 and len(ranks) == n
    k, key = cells(labels, values, n, nodata, centre, plant)
    order = np.lexsort((key, k))
    k, key = k[order], key[order]
    m = np.bincount(k, minlength=n)
    start = np.cumsum(m) - m
    out = np.full(ranks.shape, np.float32(nodata), np.float32)
    inside = (ranks >= 0) & (ranks < m[:, None])
    at = (start[:, None] + ranks)[inside]
    out[inside] = key2f(key[at])
    return out, m.astype(np.int32)


# ---- statement (b): the descent on counts ---------------------------------------------------------------------------------------
def select_descent(labels, values, n, ranks, nodata=-999.0, centre=None, plant=None):
    ranks = np.asarray(ranks, np.int64)
    assert ranks.ndim == 2 and len(ranks) == n
    R = ranks.shape[1]
    k, key = cells(labels, values, n, nodata, centre, plant)
    m = np.bincount(k, minlength=n)
    prefix = np.zeros((n, R), np.uint32)
    rem = ranks.copy()
    for bit in range(31, -1, -1):
        for j in range(R):
            zero_side = ((key ^ prefix[k, j]) >> np.uint32(bit)) == 0            # continues the prefix with a 0 at this bit
            cnt = np.zeros(n, np.int64)
            np.add.at(cnt, k[zero_side], 1)
            right = rem[:, j] > cnt if plant == "descent_lt" else rem[:, j] >= cnt
            prefix[right, j] |= np.uint32(1 << bit)
            rem[right, j] -= cnt[right]
    inside = (ranks >= 0) & (ranks < m[:, None])
    out = np.where(inside, key2f(prefix.reshape(-1)).reshape(n, R), np.float32(nodata)).astype(np.float32)
    return out, m.astype(np.int32)


# ---- the comparison -------------------------------------------------------------------------------------------------------------
def differing(got_out, got_nvalid, want_out, want_nvalid):
    """None if both are equal (out by its bits), else a dict that names the first differing label."""
    got_out, want_out = np.ascontiguousarray(got_out, np.float32), np.ascontiguousarray(want_out, np.float32)
    if got_out.shape != want_out.shape or np.shape(got_nvalid) != np.shape(want_nvalid):
        return {"shapes": (got_out.shape, want_out.shape, np.shape(got_nvalid), np.shape(want_nvalid))}
    bad = (got_out.view(np.uint32) != want_out.view(np.uint32)).any(axis=1)               # out is (n, R)
    bad |= np.asarray(got_nvalid) != np.asarray(want_nvalid)
    if not bad.any():
        return None
    k = int(np.argmax(bad))
    return {"label": k + 1, "labels_differing": int(bad.sum()), "got": got_out[k].tolist(), "want": want_out[k].tolist(),
            "got_bits": [hex(b) for b in got_out[k].view(np.uint32).reshape(-1)], "want_bits": [hex(b) for b in want_out[k].view(np.uint32).reshape(-1)],
            "got_nvalid": int(np.asarray(got_nvalid)[k]), "want_nvalid": int(np.asarray(want_nvalid)[k])}


# ---- ranks of a quantile, in Fractions ------------------------------------------------------------------------------------------
def as_fraction(q):
    if isinstance(q, Fraction):
        f = q
    elif isinstance(q, (tuple, list)):
        f = Fraction(int(q[0]), int(q[1]))
    else:
        f = Fraction(q).limit_denominator(MAX_DEN)
    assert 0 <= f <= 1 and f.denominator <= MAX_DEN, q
    return f


def ranks_of(m, q, plant=None):
    """One label with m cells that count, one level -> (lo, hi, rem, den) as Python integers."""
    f = as_fraction(q)
    if m == 0:
        return -1, -1, 0, f.denominator
    h = (m - 1) * f                                           # a Fraction: the position among the sorted cells
    lo = h.numerator // h.denominator                         # its floor
    part = h - lo
    rem = part * f.denominator
    assert rem.denominator == 1
    hi = lo + (1 if part > 0 else 0)
    if plant == "ceil_lo":
        lo = hi
    if plant == "hi_always_next":
        hi = lo + 1
    return lo, hi, int(rem), f.denominator


def ranks(m, q, plant=None):
    """m (n) ints, q a sequence of levels -> lo, hi int32 (n, Q), rem int64 (n, Q), den int64 (Q)."""
    rows = [[ranks_of(int(mk), qi, plant) for qi in q] for mk in np.asarray(m).reshape(-1)]
    a = np.array(rows, dtype=np.int64).reshape(len(rows), len(q), 4)
    den = np.array([as_fraction(qi).denominator for qi in q], np.int64)
    return a[:, :, 0].astype(np.int32), a[:, :, 1].astype(np.int32), a[:, :, 2], den


def value(lo, hi, lo_rank, rem, den, method):
    """The quantile in float64 from its two order statistics, in the rule's operation order."""
    a, b = np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if method == "linear":
            return a + (b - a) * (np.asarray(rem, np.float64) / np.asarray(den, np.float64))
        if method == "lower":
            return a
        if method == "higher":
            return b
        if method == "midpoint":
            return (a + b) * 0.5
        if method == "nearest":
            upper = (2 * rem > den) | ((2 * rem == den) & (np.asarray(lo_rank) % 2 == 1))
            return np.where(upper, b, a)
    raise ValueError(method)


def quantiles(labels, n, values, q=(0.5,), method="linear", centre=None, nodata=-999.0, plant=None, select=select_sorted):
    """What satmvs_amd.dsm.label_quantiles returns."""
    m = select(labels, values, n, np.zeros((n, 1), np.int64), nodata, centre, plant)[1]
    lo_rank, hi_rank, rem, den = ranks(m, q, plant)
    lo, _ = select(labels, values, n, lo_rank, nodata, centre, plant)
    hi, _ = select(labels, values, n, hi_rank, nodata, centre, plant)
    val = value(lo, hi, lo_rank, rem, den, method)
    val = np.where((m > 0)[:, None], val, np.nan)
    return {"n_valid": m.astype(np.int32), "lo": lo, "hi": hi, "value": val}


def nmad(labels, n, values, nodata=-999.0):
    """The two steps of label_nmad: the linear median, then the linear median of the deviations from float32(median)."""
    first = quantiles(labels, n, values, (Fraction(1, 2),), "linear", None, nodata)
    median = first["value"][:, 0]
    second = quantiles(labels, n, values, (Fraction(1, 2),), "linear", median.astype(np.float32), nodata)
    mad = second["value"][:, 0]
    return {"median": median, "mad": mad, "nmad": mad * 1.4826, "n_valid": first["n_valid"]}


def metrics_robust(est, gt, nodata=-999.0, levels=(0.6827, 0.9, 0.95)):
    """What satmvs_amd.dsm.dsm_metrics_robust returns: one zone over the cells valid in both, d in float32."""
    e, g = np.asarray(est, np.float32), np.asarray(gt, np.float32)
    both = valid(e, nodata) & valid(g, nodata)
    d = (e.astype(np.float64) - g.astype(np.float64)).astype(np.float32)
    zone = both.astype(np.int32)
    s = nmad(zone, 1, d, nodata=np.nan)
    le = quantiles(zone, 1, d, levels, "linear", np.zeros(1, np.float32), np.nan)
    out = {"n": int(s["n_valid"][0]), "median": float(s["median"][0]), "nmad": float(s["nmad"][0])}
    for q, v in zip(levels, le["value"][0]):
        out["le%d" % math.floor(100 * as_fraction(q) + Fraction(1, 2))] = float(v)
    return out


# ---- inputs the tests share -----------------------------------------------------------------------------------------------------
def random_labels(gh, gw, n, seed, background=0.3):
    """A zone map with labels 0 .. n scattered in patches (not connected), some cells at 0, n + 1 and -1."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(1, n + 1, ((gh + 3) // 4, (gw + 5) // 6))
    lab = np.kron(coarse, np.ones((4, 6), np.int64))[:gh, :gw]
    lab = np.where(rng.random((gh, gw)) < background, 0, lab)
    odd = rng.random((gh, gw))
    lab = np.where(odd < 0.02, n + 1, np.where(odd < 0.04, -1, lab))
    return lab.astype(np.int32)


def special_values(gh, gw, seed):
    """float32 values with everything the order has to get right: both zeros, denormals, neighbours in the lowest and the highest
    bit, negatives, NaN, both infinities and nodata, many duplicates."""
    rng = np.random.default_rng(seed)
    pool = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.0, np.nextafter(np.float32(1.0), np.float32(2.0)), -1.0,
                     np.nextafter(np.float32(-1.0), np.float32(-2.0)), 2.5, -2.5, 3.4e38, -3.4e38, 130.25, 130.25, -999.0,
                     np.nan, np.inf, -np.inf, 7.0, 7.0, 7.0, -7.0], dtype=np.float32)
    return pool[rng.integers(0, len(pool), (gh, gw))]


def kit_scene(gh, gw, seed, voids=0.0, salt=0.0):
    """The test kit's scene on a 5 m grid of gh x gw cells."""
    from dsm_testkit import scene
    r, c = np.meshgrid(np.arange(gh, dtype=np.float64), np.arange(gw, dtype=np.float64), indexing="ij")
    return scene(5.0 * c, -5.0 * r, seed=seed, voids=voids, salt=salt)


def rank_matrix(m, R, turn=0):
    """(n, R) int32 ranks for labels with m (n) cells that count: the first, the last, one before the first (-1), one past the
    last (m), the middle twice (duplicates in a row), a third and two thirds of the way; the columns start at kind `turn`."""
    m = np.asarray(m, np.int64)
    kinds = [np.zeros_like(m), m - 1, -np.ones_like(m), m, m // 2, m // 2, m // 3, (2 * m) // 3]
    return np.stack([kinds[(turn + j) % len(kinds)] for j in range(R)], axis=1).astype(np.int32)


def hand_map():
    """6 x 9: label 1 in two pieces, label 2 once, label 3 without a cell, label 4 with voids only, and 0, n + 1 = 5 and -1."""
    lab = np.array([[1, 1, 0, 0, 2, 2, 2, 5, -1],
                    [1, 1, 0, 0, 2, 2, 2, 5, -1],
                    [0, 0, 0, 0, 0, 0, 0, 0, 0],
                    [4, 4, 4, 0, 0, 1, 1, 1, 0],
                    [4, 4, 4, 0, 0, 1, 1, 1, 0],
                    [0, 0, 0, 0, 2, 0, 0, 0, 0]], np.int32)
    rng = np.random.default_rng(3)
    v = rng.normal(10.0, 3.0, lab.shape).astype(np.float32)
    v[lab == 4] = np.where(rng.random(int((lab == 4).sum())) < 0.5, np.float32(np.nan), np.float32(-999.0))
    return lab, v, 4


def matrix(large=True):
    """The cases both test files walk: dicts of name, labels, values, n, nodata, centre (None or (n) float32)."""
    out = []

    def add(name, labels, values, n, nodata=-999.0, centre=None):
        out.append({"name": name, "labels": np.ascontiguousarray(labels, np.int32), "values": np.ascontiguousarray(values, np.float32),
                    "n": int(n), "nodata": nodata, "centre": None if centre is None else np.ascontiguousarray(centre, np.float32)})

    shapes = [(1, 1), (1, 70), (67, 1), (2, 2), (5, 63), (5, 64), (5, 65), (33, 129)] + ([(257, 301)] if large else [])
    for i, (gh, gw) in enumerate(shapes):
        n = max(1, min(6, gh * gw // 2))
        add("special %dx%d" % (gh, gw), random_labels(gh, gw, n, seed=i), special_values(gh, gw, seed=10 + i), n)
        add("scene %dx%d" % (gh, gw), random_labels(gh, gw, n, seed=20 + i, background=0.1), kit_scene(gh, gw, 30 + i, voids=0.05, salt=0.02), n)
    gh, gw = (257, 301) if large else (40, 70)
    for voids in (0.0, 0.05, 0.3):
        add("kit voids %g" % voids, random_labels(gh, gw, 40, seed=int(100 * voids)), kit_scene(gh, gw, 7, voids=voids, salt=0.02), 40)
    lab, v, n = hand_map()
    add("hand-made map", lab, v, n)
    add("another nodata", lab, np.where(lab == 2, np.float32(-1.0), v), n, nodata=-1.0)
    gh, gw = 37, 65
    whole = np.ones((gh, gw), np.int32)
    own = np.arange(1, gh * gw + 1, dtype=np.int32).reshape(gh, gw)
    spec = special_values(gh, gw, seed=5)
    add("one label over the grid", whole, spec, 1)
    add("one label over the grid, scene", whole, kit_scene(gh, gw, 9, voids=0.05, salt=0.05), 1)
    add("every cell its own label", own, spec, gh * gw)
    add("n = 0", whole, spec, 0)
    add("all values equal", random_labels(gh, gw, 5, seed=1), np.full((gh, gw), 130.25, np.float32), 5)
    rng = np.random.default_rng(11)
    add("two distinct values", random_labels(gh, gw, 5, seed=2), np.where(rng.random((gh, gw)) < 0.4, np.float32(2.0), np.float32(-3.0)), 5)
    add("negatives and positives", random_labels(gh, gw, 5, seed=3), rng.normal(0.0, 5.0, (gh, gw)).astype(np.float32), 5)
    add("both zeros in one zone", whole, np.where(rng.random((gh, gw)) < 0.5, np.float32(0.0), np.float32(-0.0)), 1)
    den = (rng.integers(-40, 41, (gh, gw)).astype(np.float64) * 1.401298464324817e-45).astype(np.float32)
    add("denormals", random_labels(gh, gw, 3, seed=4), den, 3)
    low = (np.uint32(0x42f00000) + rng.integers(0, 2, (gh, gw)).astype(np.uint32)).view(np.float32)
    high = (np.uint32(0x42f00000) ^ (rng.integers(0, 2, (gh, gw)).astype(np.uint32) << np.uint32(31))).view(np.float32)
    add("lowest bit only", random_labels(gh, gw, 3, seed=5), low, 3)
    add("highest bit only", random_labels(gh, gw, 3, seed=6), high, 3)
    # deviation mode
    lab5 = random_labels(gh, gw, 5, seed=8, background=0.1)
    vals = np.round(rng.normal(20.0, 4.0, (gh, gw)) * 4.0).astype(np.float32) / np.float32(4.0)       # quarters: ties with a centre
    med = quantiles(lab5, 5, vals, (Fraction(1, 2),))["value"][:, 0].astype(np.float32)
    add("deviation from the median", lab5, vals, 5, centre=med)
    add("deviation, a centre among the cells", lab5, vals, 5, centre=np.array([20.0, 19.75, 20.25, 16.0, 24.0], np.float32))
    add("deviation, centres not finite", lab5, vals, 5, centre=np.array([np.nan, np.inf, -np.inf, 20.0, np.nan], np.float32))
    add("deviation, centres of both zeros", lab5, spec, 5, centre=np.array([0.0, -0.0, 0.0, -0.0, 0.0], np.float32))
    add("deviation, special values", lab5, spec, 5, centre=np.array([1.0, -2.5, 3.4e38, 1e-40, 7.0], np.float32))
    return out
