"""numpy statements of the rules of smvs_dsm_stack_select and smvs_dsm_stack_fuse (include/satmvs.h, "Stack fusion"), for
test_dsm_stack_cpu.py and test_dsm_stack_gpu.py.  Each rule is stated twice, independently:

  select_cells / fuse_cells    a Python loop over the destination cells: the layers that reach the cell, sorted() by their keys,
                               Python floats (IEEE float64) for the arithmetic and struct for every rounding to float32
  select_sorted / fuse_sorted  arrays: the layers placed by slices into a (K, gh, gw) stack of keys with a sentinel above every
                               key where a layer is void or absent, np.sort along the layer axis, np.take_along_axis

A layer is (z, ox, oy): z (h, w) float32, its cell (r, c) on destination cell (r + oy, c + ox).  The array statements take a
`flaw`: one deliberate departure from the rule each (FLAWS), for the tests that show the case matrix tells them apart."""
import struct

import numpy as np

from dsm_testkit import f2key, key2f, valid

SENTINEL = np.uint64(1) << np.uint64(32)                                   # above every uint32 key
FLAWS = ("midpoint", "strict", "sum_from_zero", "ties_by_layer", "hi_no_remainder", "valid_on_d")


# ---- scalars: float32 roundings and keys without numpy ---------------------------------------------------------------------------
def _f32(x):
    """(float)x of a Python float, to nearest even, as a Python float."""
    try:
        return struct.unpack("<f", struct.pack("<f", x))[0]
    except OverflowError:                                                  # struct refuses what rounds to an infinity
        return float("inf") if x > 0 else float("-inf")


def _key(x):
    u = struct.unpack("<I", struct.pack("<f", x))[0]
    return (~u & 0xffffffff) if u & 0x80000000 else (u | 0x80000000)


def _unkey(k):
    u = (k & 0x7fffffff) if k & 0x80000000 else (~k & 0xffffffff)
    return struct.unpack("<f", struct.pack("<I", u))[0]


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _middle(keys, m):
    """The linear median a + (b - a) (rem / 2) of m sorted keys, float64."""
    mid, rem = (m - 1) // 2, (m - 1) % 2
    a, b = _unkey(keys[mid]), _unkey(keys[mid + rem])
    return a + (b - a) * (rem / 2)


def _cell_layers(layers, nodata, r, c):
    """[(k, z as a Python float)] of the layers valid on destination cell (r, c), ascending k."""
    nd = float(np.float32(nodata))
    out = []
    for k, (z, ox, oy) in enumerate(layers):
        rr, cc = r - oy, c - ox
        if 0 <= rr < z.shape[0] and 0 <= cc < z.shape[1]:
            v = float(z[rr, cc])
            if v == v and abs(v) != float("inf") and v != nd:
                out.append((k, v))
    return out


# ---- the loop statements -----------------------------------------------------------------------------------------------------------
def select_cells(layers, nodata, levels, centre, gw, gh):
    """-> count uint8 (gh, gw), lo, hi float32 (Q, gh, gw)."""
    Q = len(levels)
    nd_bits = _bits(float(np.float32(nodata)))
    count = np.zeros((gh, gw), np.uint8)
    lo = np.full((Q, gh, gw), nd_bits, np.uint32)
    hi = lo.copy()
    for r in range(gh):
        for c in range(gw):
            V = _cell_layers(layers, nodata, r, c)
            if centre is not None:
                ctr = float(centre[r, c])
                if ctr != ctr or abs(ctr) == float("inf"):
                    V = []
                vals = [_f32(abs(z - ctr)) for _, z in V]
            else:
                vals = [z for _, z in V]
            keys = sorted(_key(v) for v in vals)
            m = len(keys)
            count[r, c] = m
            if m == 0:
                continue
            for j, (num, den) in enumerate(levels):
                h = (m - 1) * num
                lo_rank = h // den
                hi_rank = lo_rank + (1 if h % den > 0 else 0)
                lo[j, r, c] = _bits(_unkey(keys[lo_rank]))
                hi[j, r, c] = _bits(_unkey(keys[hi_rank]))
    return count, lo.view(np.float32), hi.view(np.float32)


def fuse_cells(layers, nodata, kmad, floor, min_count, gw, gh):
    """-> out, median, mad float32; count, n_in uint8; members, inliers int64, all (gh, gw)."""
    nd_bits = _bits(float(np.float32(nodata)))
    out = np.full((gh, gw), nd_bits, np.uint32)
    median, mad = out.copy(), out.copy()
    count, n_in = np.zeros((gh, gw), np.uint8), np.zeros((gh, gw), np.uint8)
    members, inliers = np.zeros((gh, gw), np.uint64), np.zeros((gh, gw), np.uint64)
    for r in range(gh):
        for c in range(gw):
            V = _cell_layers(layers, nodata, r, c)
            m = len(V)
            count[r, c] = m
            if m < max(min_count, 1):
                continue
            med = _f32(_middle(sorted(_key(z) for _, z in V), m))
            d = [_f32(abs(z - med)) for _, z in V]
            spread = _f32(_middle(sorted(_key(v) for v in d), m))
            product = kmad * spread
            thr = floor if product != product else max(product, floor)      # fmax: a NaN product loses
            S, n, mem, inl = 0.0, 0, 0, 0
            for (k, z), dk in zip(V, d):
                mem |= 1 << k
                if dk <= thr:
                    S = z if n == 0 else S + z
                    n += 1
                    inl |= 1 << k
            median[r, c], mad[r, c] = _bits(med), _bits(spread)
            out[r, c] = _bits(_f32(S / n)) if n else _bits(med)
            n_in[r, c], members[r, c], inliers[r, c] = n, mem, inl
    return (out.view(np.float32), median.view(np.float32), mad.view(np.float32), count, n_in, members.view(np.int64),
            inliers.view(np.int64))


# ---- the array statements ----------------------------------------------------------------------------------------------------------
def stack(layers, nodata, gw, gh):
    """The layers placed on the destination -> (Z float32 (K, gh, gw), NaN where a layer does not reach; ok bool (K, gh, gw))."""
    Z = np.full((len(layers), gh, gw), np.nan, np.float32)
    for k, (z, ox, oy) in enumerate(layers):
        h, w = z.shape
        r0, r1, c0, c1 = max(oy, 0), min(oy + h, gh), max(ox, 0), min(ox + w, gw)
        if r0 < r1 and c0 < c1:
            Z[k, r0:r1, c0:c1] = z[r0 - oy:r1 - oy, c0 - ox:c1 - ox]
    return Z, valid(Z, nodata)


def deviations(Z, centre):
    """(float)fabs((double)z - (double)centre), centre (gh, gw) or (K, gh, gw)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.abs(Z.astype(np.float64) - np.asarray(centre, np.float32).astype(np.float64)).astype(np.float32)


def _sorted_keys(values, ok, by_value=False):
    """(K, gh, gw) uint64 keys ascending along the layers, the sentinel where not ok.  by_value: the flaw -- ordered as floats
    compare, -0.0 equal to +0.0 and the earlier layer first."""
    keys = np.where(ok, f2key(values).astype(np.uint64), SENTINEL)
    if by_value:
        order = np.argsort(np.where(ok, values, np.inf).astype(np.float64), axis=0, kind="stable")
        return np.take_along_axis(keys, order, axis=0)
    return np.sort(keys, axis=0)


def _at(keys, rank):
    """The float32 value of the key at `rank` (gh, gw) of every cell; rank clipped into the stack (the caller masks m = 0)."""
    k = np.take_along_axis(keys, np.clip(rank, 0, keys.shape[0] - 1)[None].astype(np.int64), axis=0)[0]
    return key2f((k & np.uint64(0xffffffff)).astype(np.uint32))


def _linear_half(keys, m, flaw=None):
    """The linear median over the first m keys of every cell, float64 (gh, gw); garbage where m = 0."""
    mid, rem = (m - 1) // 2, (m - 1) % 2
    a, b = _at(keys, mid).astype(np.float64), _at(keys, mid + rem).astype(np.float64)
    with np.errstate(invalid="ignore"):
        if flaw == "midpoint":
            return (a + b) * 0.5
        return a + (b - a) * (rem / 2.0)


def select_sorted(layers, nodata, levels, centre, gw, gh, flaw=None):
    Z, ok = stack(layers, nodata, gw, gh)
    values = Z
    if centre is not None:
        values = deviations(Z, centre)
        ok = ok & np.isfinite(np.asarray(centre, np.float32))[None]
        if flaw == "valid_on_d":
            ok = ok & np.isfinite(values)
    keys = _sorted_keys(values, ok, by_value=flaw == "ties_by_layer")
    m = ok.sum(axis=0).astype(np.int64)
    nd = np.float32(nodata)
    lo = np.empty((len(levels), gh, gw), np.float32)
    hi = np.empty_like(lo)
    for j, (num, den) in enumerate(levels):
        h = np.maximum(m - 1, 0) * num
        lo_rank = h // den
        hi_rank = lo_rank + (h % den > 0)
        if flaw == "hi_no_remainder":
            hi_rank = np.minimum(lo_rank + 1, np.maximum(m - 1, 0))
        lo[j] = np.where(m > 0, _at(keys, lo_rank), nd)
        hi[j] = np.where(m > 0, _at(keys, hi_rank), nd)
    return m.astype(np.uint8), lo, hi


def fuse_sorted(layers, nodata, kmad, floor, min_count, gw, gh, flaw=None):
    Z, ok = stack(layers, nodata, gw, gh)
    K = len(layers)
    m = ok.sum(axis=0).astype(np.int64)
    keep = m >= max(min_count, 1)
    med32 = _linear_half(_sorted_keys(Z, ok, by_value=flaw == "ties_by_layer"), m, flaw).astype(np.float32)
    d = deviations(Z, med32)
    with np.errstate(over="ignore", invalid="ignore"):
        mad32 = _linear_half(_sorted_keys(d, ok), m, flaw).astype(np.float32)
        thr = np.fmax(kmad * mad32.astype(np.float64), floor)
        inl = ok & ((d.astype(np.float64) < thr) if flaw == "strict" else (d.astype(np.float64) <= thr)) & keep[None]
    S = np.zeros((gh, gw), np.float64)
    started = np.full((gh, gw), flaw == "sum_from_zero")
    for k in range(K):
        with np.errstate(invalid="ignore"):
            S = np.where(inl[k], np.where(started, S + Z[k].astype(np.float64), Z[k].astype(np.float64)), S)
        started = started | inl[k]
    n_in = inl.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = (S / n_in).astype(np.float32)
    nd = np.float32(nodata)
    out = np.where(keep, np.where(n_in > 0, mean, med32), nd)
    bit = (np.uint64(1) << np.arange(K, dtype=np.uint64))[:, None, None]
    members = np.where(keep, (ok * bit).sum(axis=0, dtype=np.uint64), np.uint64(0))
    inliers = (inl * bit).sum(axis=0, dtype=np.uint64)
    return (out, np.where(keep, med32, nd), np.where(keep, mad32, nd), m.astype(np.uint8), n_in.astype(np.uint8),
            members.view(np.int64), inliers.view(np.int64))


SELECT_NAMES = ("count", "lo", "hi")
FUSE_NAMES = ("out", "median", "mad", "count", "n_in", "members", "inliers")


def differs(got, want):
    """Whether two result tuples differ anywhere, floats by their bits (what the GPU file's comparison reports)."""
    for g, w in zip(got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        if g.shape != w.shape or not np.array_equal(g, w):
            return True
    return False
