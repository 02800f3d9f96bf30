"""Test-local numpy oracle of DSM production: the Transverse Mercator series in the operation order of the reference's numpy
code (pinned against tests/golden/tm.npz), the bin rule, a per-cell reduce by np.lexsort, the same reduce vectorised with the
derived interval of the mean and the comparison that goes with it, and the kernel's steps restated with switches that plant
errors in them."""
import math
from collections import namedtuple

import numpy as np

from dsm_testkit import f2key as keys  # noqa: F401  (re-exported)

PI = 3.14159265358979323846


def _consts(tm7):
    a, inv_f, lat0, lon0, k0, fe, fn = [float(v) for v in tm7]
    f = 1.0 / inv_f
    e = np.sqrt(2 * f - f * f)
    e2 = e * e
    e4, e6 = e2 * e2, e2 * e2 * e2
    sec_e = np.sqrt((e * e) / (1 - e * e))
    m = (1 - e2 / 4 - 3 * e4 / 64 - 5 * e6 / 256, 3 * e2 / 8 + 3 * e4 / 32 + 45 * e6 / 1024, 15 * e4 / 256 + 45 * e6 / 1024,
         35 * e6 / 3072)
    phi0, lam0 = lat0 / 180 * PI, lon0 / 180 * PI
    m0 = a * (m[0] * phi0 - m[1] * np.sin(2 * phi0) + m[2] * np.sin(4 * phi0) - m[3] * np.sin(6 * phi0))
    return dict(a=a, e=e, e2=e2, sec_e=sec_e, m=m, m0=m0, lam0=lam0, k0=k0, fe=fe, fn=fn)


def tm_forward(tm7, lat, lon):
    c = _consts(tm7)
    phi, lam = np.asarray(lat, np.float64) / 180 * PI, np.asarray(lon, np.float64) / 180 * PI
    e2, se, a, m = c["e2"], c["sec_e"], c["a"], c["m"]
    cp, sp, tp = np.cos(phi), np.sin(phi), np.tan(phi)
    T = tp * tp
    C = e2 * cp * cp / (1 - e2)
    A = (lam - c["lam0"]) * cp
    nu = a / np.sqrt(1 - e2 * sp * sp)
    M = a * (m[0] * phi - m[1] * np.sin(2 * phi) + m[2] * np.sin(4 * phi) - m[3] * np.sin(6 * phi))
    A2, A3 = A * A, A * A * A
    E = c["fe"] + c["k0"] * nu * (A + (1 - T + C) * A3 / 6 + (5 - 18 * T + T * T + 72 * C - 58 * se * se) * A2 * A3 / 120)
    N = c["fn"] + c["k0"] * (M - c["m0"] + nu * tp * (A2 / 2 + (5 - T + 9 * C + 4 * C * C) * A2 * A2 / 24 +
                                                       (61 - 58 * T + T * T + 600 * C - 330 * se * se) * A3 * A3 / 720))
    return E, N


def tm_inverse(tm7, E, N):
    c = _consts(tm7)
    e, e2, a, m, k0 = c["e"], c["e2"], c["a"], c["m"], c["k0"]
    E, N = np.asarray(E, np.float64), np.asarray(N, np.float64)
    r = np.sqrt(1 - e * e)
    e1 = (1 - r) / (1 + r)
    e1s = e1 * e1
    mu = (c["m0"] + (N - c["fn"]) / k0) / (a * m[0])
    phi1 = (mu + (3 * e1 / 2 - 27 * e1s * e1 / 32) * np.sin(2 * mu) + (21 * e1s / 16 - 55 * e1s * e1s / 32) * np.sin(4 * mu)
            + (151 * e1s * e1 / 96) * np.sin(6 * mu) + (1097 * e1s * e1s / 512) * np.sin(8 * mu))
    q = np.sqrt(1 - e2 * np.sin(phi1) * np.sin(phi1))
    nu1 = a / q
    rho1 = a * (1 - e2) / (q * q * q)
    T1 = np.tan(phi1) * np.tan(phi1)
    C1 = c["sec_e"] * np.cos(phi1)
    C1 = C1 * C1
    D = (E - c["fe"]) / (nu1 * k0)
    D2, D3 = D * D, D * D * D
    s2 = c["sec_e"] * c["sec_e"]
    phi = phi1 - (nu1 * np.tan(phi1) / rho1) * (D2 / 2 - (5 + 3 * T1 + 10 * C1 - 4 * C1 * C1 - 9 * s2) * D2 * D2 / 24 +
                                               (61 + 90 * T1 + 298 * C1 + 45 * T1 * T1 - 252 * s2 - 3 * C1 * C1) * D3 * D3 / 720)
    lam = c["lam0"] + (D - (1 + 2 * T1 + C1) * D3 / 6 +
                       (5 - 2 * C1 + 28 * T1 - 3 * C1 * C1 + 8 * s2 + 24 * T1 * T1) * D2 * D3 / 120) / np.cos(phi1)
    return phi * 180 / PI, lam * 180 / PI


def cells(east, north, grid4, gw, gh, fault=None):
    """The bin rule on given E / N: row * gw + col, or -1 off the grid / non-finite.  `fault` plants an error (CELL_FAULTS)."""
    e0, n0, xr, yr = [float(v) for v in grid4]
    with np.errstate(invalid="ignore", over="ignore"):
        if fault == "rint":
            col, row = np.rint((east - e0) / xr), np.rint((n0 - north) / yr)
        else:
            col = np.floor((east - e0) / xr + 0.5)
            row = np.floor((n0 - north) / yr + 0.5)
        ok = (col >= 0) & ((col <= gw) if fault == "col <= gw" else (col < gw)) & (row >= 0) & (row < gh)
    out = np.full(np.shape(east), -1, np.int64)
    out[ok] = (row[ok].astype(np.int64) * gw + col[ok].astype(np.int64))
    return out


def reduce(cell, height, ncells, mode, nodata):
    """Per-cell median / mean / min / max of the heights sorted on their uint32 keys; empty cells -> nodata.  float32."""
    cell = np.asarray(cell).reshape(-1)
    height = np.asarray(height, np.float32).reshape(-1)
    ok = (cell >= 0) & (cell < ncells)
    c, h = cell[ok], height[ok]
    order = np.lexsort((keys(h), c))
    c, h = c[order], h[order]
    out = np.full(ncells, np.float32(nodata), np.float32)
    count = np.bincount(c, minlength=ncells)
    starts = np.concatenate([[0], np.cumsum(count)])
    for cc in np.nonzero(count)[0]:
        v = h[starts[cc]:starts[cc + 1]]
        n = v.size
        with np.errstate(invalid="ignore", over="ignore"):   # buckets with NaN or infinities
            if mode == "min":
                out[cc] = v[0]
            elif mode == "max":
                out[cc] = v[-1]
            elif mode == "mean":
                out[cc] = np.float32(v.astype(np.float64).sum() / n)
            elif n % 2:
                out[cc] = v[n // 2]
            else:
                out[cc] = np.float32(0.5 * (np.float64(v[n // 2 - 1]) + np.float64(v[n // 2])))
    return out, count


# ---- the reduce, vectorised, with the derived bound of the mean ------------------------------------------------------------------
# reduce() above stays the plain statement (a loop over the cells); reference() gives the same medians, minima and maxima by
# index arithmetic on one np.lexsort, so that grids of 2e6 cells take seconds, and for the mean not a value but an interval:
# mean_exact = fsum(bucket) / m in float64, delta = (m + 1) 2^-53 sum|h| / m.  A float64 sum of m terms in ANY order is
# within (m - 1) 2^-53 sum|h| of the exact sum (to first order; the second-order terms are below 2^-53 of that for
# m < 2^31), the division rounds once more, and fsum / m itself is within 2^-53 of the exact mean: m + 1 in all.  The kernel
# rounds its float64 mean once to float32, and rounding is monotone, so its result lies in [f32(mean_exact - delta),
# f32(mean_exact + delta)].  A bucket of one value has delta = 0.  A bucket with a non-finite value has no interval but a
# kind: NaN (a NaN in it, or both infinities) or the signed infinity.
Ref = namedtuple("Ref", "count median min max mean_exact delta kind")
FINITE, IS_NAN, PLUS_INF, MINUS_INF = 0, 1, 2, 3
TIERS = (("tier 0", 1, 32), ("tier 1", 33, 4096), ("tier 2", 4097, 2 ** 31))
U53 = 2.0 ** -53


def reference(cell, height, ncells):
    cell = np.asarray(cell).reshape(-1).astype(np.int64)
    height = np.asarray(height, np.float32).reshape(-1)
    ok = (cell >= 0) & (cell < ncells)
    c, h = cell[ok], height[ok]
    order = np.lexsort((keys(h), c))
    c, h = c[order], h[order]
    count = np.bincount(c, minlength=ncells)
    full = np.nonzero(count)[0]
    m = count[full]
    lo = (np.cumsum(count) - count)[full]
    out = {k: np.zeros(ncells, np.float32) for k in ("median", "min", "max")}
    mean_exact, delta, kind = np.full(ncells, np.nan), np.zeros(ncells), np.full(ncells, -1, np.int8)
    if full.size:
        out["min"][full], out["max"][full] = h[lo], h[lo + m - 1]
        a, b = h[lo + (m - 1) // 2], h[lo + m // 2]
        with np.errstate(invalid="ignore", over="ignore"):
            even = (0.5 * (a.astype(np.float64) + b.astype(np.float64))).astype(np.float32)
        out["median"][full] = np.where(m % 2 == 1, b.view(np.uint32), even.view(np.uint32)).view(np.float32)
        n_nan = np.add.reduceat(np.isnan(h).astype(np.int64), lo)
        n_pos = np.add.reduceat((h == np.inf).astype(np.int64), lo)
        n_neg = np.add.reduceat((h == -np.inf).astype(np.int64), lo)
        k = np.where((n_nan > 0) | ((n_pos > 0) & (n_neg > 0)), IS_NAN, np.where(n_pos > 0, PLUS_INF, np.where(n_neg > 0, MINUS_INF, FINITE)))
        kind[full] = k
        with np.errstate(invalid="ignore"):
            h64 = h.astype(np.float64)
        for i in np.nonzero(k == FINITE)[0]:
            v = h64[lo[i]:lo[i] + m[i]].tolist()
            mean_exact[full[i]] = math.fsum(v) / m[i]
            if m[i] > 1:
                delta[full[i]] = (m[i] + 1) * U53 * math.fsum([abs(x) for x in v]) / m[i]
    return Ref(count, out["median"], out["min"], out["max"], mean_exact, delta, kind)


def check(got, ref, mode, nodata):
    """Assert a (ncells) float32 result of `mode` against a Ref, no cell excused.  -> for the mean, {tier: (a, b)} over the
    tier's finite buckets of more than one value; else {}.  a = the largest (|got - mean_exact| - half a float32 ulp of got) /
    delta, at least 0: the final rounding to float32 moves a float64 mean by up to half an ulp, which is far more than delta
    unless the bucket cancels, so this is the share of delta that the float64 mean before the rounding must have used at
    least.  b = the largest distance of got from f32(mean_exact) in float32 ulps, over the buckets whose interval is at most one
    ulp wide (0 = correctly rounded)."""
    got = np.ascontiguousarray(got, np.float32).reshape(-1)
    bits = got.view(np.uint32)
    assert got.size == ref.count.size
    empty = ref.count == 0
    nd = np.array([nodata], np.float32).view(np.uint32)[0]
    assert (bits[empty] == nd).all(), (mode, "empty cells without nodata's bits", int((bits[empty] != nd).sum()))
    if mode != "mean":
        bad = ~empty & (bits != getattr(ref, mode).view(np.uint32))
        assert not bad.any(), (mode, int(bad.sum()), np.nonzero(bad)[0][:5].tolist(), ref.count[bad][:5].tolist())
        return {}
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = (ref.mean_exact - ref.delta).astype(np.float32), (ref.mean_exact + ref.delta).astype(np.float32)
        fin = ref.kind == FINITE
        bad = fin & ~((got >= lo) & (got <= hi))
        assert not bad.any(), ("mean outside its interval", int(bad.sum()), np.nonzero(bad)[0][:5].tolist(), ref.count[bad][:5].tolist(),
                               got[bad][:5].tolist(), ref.mean_exact[bad][:5].tolist(), ref.delta[bad][:5].tolist())
        bad = ((ref.kind == IS_NAN) & ~np.isnan(got)) | ((ref.kind == PLUS_INF) & (got != np.inf)) | ((ref.kind == MINUS_INF) & (got != -np.inf))
        assert not bad.any(), ("mean of a non-finite bucket", int(bad.sum()), np.nonzero(bad)[0][:5].tolist(), got[bad][:5].tolist())
        half_ulp = 0.5 * np.spacing(np.abs(got)).astype(np.float64)
        ratio = np.maximum(np.abs(got.astype(np.float64) - ref.mean_exact) - half_ulp, 0.0) / np.where(ref.delta > 0, ref.delta, np.inf)
        nearest = ref.mean_exact.astype(np.float32)
        ulps = np.abs(_ordered(got) - _ordered(nearest))
        narrow = _ordered(hi) - _ordered(lo) <= 1
    out = {}
    for name, a, b in TIERS:
        sel = fin & (ref.count > 1) & np.isfinite(got) & (ref.count >= a) & (ref.count <= b)
        if sel.any():
            out[name] = (float(ratio[sel].max()), int(ulps[sel & narrow].max()) if (sel & narrow).any() else 0)
    return out


def _ordered(f):
    """float32 -> int64 in the order of the values (both zeros at 0): differences are distances in ulps."""
    i = np.ascontiguousarray(f, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


# ---- planted errors: the kernel's steps restated in numpy, each with a switch that breaks it --------------------------------------
REDUCE_FAULTS = ("upper median", "carry dropped", "one tile off", "nan lowest", "zeros merged", "pad key 0", "radix skips byte 3")
CELL_FAULTS = ("rint", "col <= gw")
SCAN_TILE, SCAN_CHUNK = 4096, 256


def model_reduce(cell, height, ncells, mode, nodata, fault=None):
    """The reduce as the kernels do it -- tile sums, their scan in chunks, the cells' offsets, the scatter into one key array,
    the clamp of bucket(), a sort per bucket padded as its tier pads it -- with `fault` (one of REDUCE_FAULTS) planted."""
    from dsm_testkit import key2f
    cell = np.asarray(cell).reshape(-1).astype(np.int64)
    height = np.asarray(height, np.float32).reshape(-1)
    n = cell.size
    ok = (cell >= 0) & (cell < ncells)
    c, h = cell[ok], height[ok]
    if fault == "zeros merged":
        h = np.where(h == 0, np.float32(0.0), h)
    k = keys(h)
    count = np.bincount(c, minlength=ncells)
    ntiles = -(-ncells // SCAN_TILE)
    padded = np.zeros(ntiles * SCAN_TILE, np.int64)
    padded[:ncells] = count
    tiles = padded.reshape(ntiles, SCAN_TILE)
    total = tiles.sum(axis=1)
    base = np.cumsum(total) - total
    if fault == "carry dropped":
        for b0 in range(SCAN_CHUNK, ntiles, SCAN_CHUNK):
            base[b0:b0 + SCAN_CHUNK] -= base[b0]
    if fault == "one tile off":
        base = np.concatenate([[0], base[:-1]])
    offs = np.concatenate([(base[:, None] + np.cumsum(tiles, axis=1) - tiles).reshape(-1)[:ncells], [total.sum()]])
    order = np.argsort(c, kind="stable")
    cs, ks = c[order], k[order]
    slot = offs[cs] + np.arange(cs.size) - (np.cumsum(count) - count)[cs]
    keep = (slot >= offs[cs]) & (slot < offs[cs + 1]) & (slot < n)
    key_arr = np.zeros(max(n, 1), np.uint32)
    key_arr[slot[keep]] = ks[keep]
    lo, hi = np.minimum(offs[:-1], n), np.minimum(offs[1:], n)
    m_all = np.minimum(count, np.where(hi > lo, hi - lo, 0))
    out = np.full(ncells, np.float32(nodata), np.float32)
    for cc in np.nonzero(m_all)[0]:
        m = int(m_all[cc])
        v = key_arr[lo[cc]:lo[cc] + m]
        with np.errstate(invalid="ignore", over="ignore"):
            if fault == "nan lowest":
                v = v[np.argsort(np.where(np.isnan(key2f(v)), np.uint32(0), v), kind="stable")]
            elif fault == "radix skips byte 3" and m > 4096:
                v = v[np.argsort(v & np.uint32(0xffffff), kind="stable")]
            else:
                v = np.sort(v)
            if fault == "pad key 0" and m <= 4096:
                P = 32 if m <= 32 else 1 << (m - 1).bit_length()
                v = np.concatenate([np.zeros(P - m, np.uint32), v])[:m]
            f = key2f(v)
            if mode == "min":
                out[cc] = f[0]
            elif mode == "max":
                out[cc] = f[m - 1]
            elif mode == "mean":
                out[cc] = np.float32(f.astype(np.float64).sum() / m)
            elif m % 2 or fault == "upper median":
                out[cc] = f[m // 2]
            else:
                out[cc] = np.float32(0.5 * (np.float64(f[m // 2 - 1]) + np.float64(f[m // 2])))
    return out
