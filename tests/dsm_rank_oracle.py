"""The rule of the focal order statistics (include/satmvs.h, "Focal order statistics") in numpy and Python, stated twice:

  select_loop / count_loop      a loop over every cell: the window's valid values gathered, their keys sorted by Python's sorted,
                                the ranks taken from Python integers
  select_sorted / count_sorted  vectorised: the grid padded with cells that are not valid, sliding_window_view, the footprint as a
                                mask, np.sort, a gather at the ranks

A window is a 2-D boolean footprint of odd sizes about its middle cell.  Around the two statements: the footprints of the tests,
the Python layer's functions (quantiles, the midpoint median, NMAD, the robust despike, the elevation percentile), the matrix
of cases and the comparison by bits.  numpy only: nothing here imports torch or the package."""
from fractions import Fraction

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import dsm_quantile_oracle as qo
from dsm_testkit import f2key, key2f, valid

TILE = 32                                                    # SMVS_DSM_RANK_TILE of include/satmvs.h
VOID = 1 << 32                                               # above every key
LEVELS = ((0, 1), (1, 1), (1, 2), (1, 4), (9, 10), (1, 65536), (65535, 65536))
FLT_MAX = np.float32(3.4028234663852886e38)


# ---- footprints -----------------------------------------------------------------------------------------------------------------
def footprint(kind, radius=0, inner=None):
    """box, disc (dx^2 + dy^2 <= radius^2), annulus (the disc without the disc of `inner`), row and column (2 radius + 1 cells),
    lopsided (a 3 x radius block east of the centre: every dx > 0)."""
    r = int(radius)
    d = np.arange(-r, r + 1)
    d2 = d[None, :] ** 2 + d[:, None] ** 2
    if kind == "box":
        return np.ones((2 * r + 1, 2 * r + 1), bool)
    if kind == "disc":
        return d2 <= r * r
    if kind == "annulus":
        return (d2 <= r * r) & (d2 > inner * inner)
    if kind == "row":
        return np.ones((1, 2 * r + 1), bool)
    if kind == "column":
        return np.ones((2 * r + 1, 1), bool)
    if kind == "lopsided":
        foot = np.zeros((3, 2 * r + 1), bool)
        foot[:, r + 1:] = True
        foot[0, r + 1] = False
        return foot
    raise ValueError(kind)


def runs_of(foot):
    """The footprint as the entry's records {dy, dx0, dx1}, sorted by (dy, dx0), (k, 3) int32."""
    ky, kx = foot.shape[0] // 2, foot.shape[1] // 2
    out = []
    for r in range(foot.shape[0]):
        c = 0
        while c < foot.shape[1]:
            if foot[r, c]:
                c1 = c
                while c1 + 1 < foot.shape[1] and foot[r, c1 + 1]:
                    c1 += 1
                out.append((r - ky, c - kx, c1 - kx))
                c = c1 + 1
            else:
                c += 1
    return np.array(out, np.int32).reshape(-1, 3)


def rank_pair(n, num, den):
    """(lo_rank, hi_rank, rem) of a window with n valid cells, Python integers; n >= 1."""
    h = (n - 1) * num
    lo = h // den
    return lo, lo + (1 if h % den > 0 else 0), h % den


def _deviation(v, c):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.abs(np.asarray(v, np.float32).astype(np.float64) - np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


# ---- statement (a): a loop over every cell --------------------------------------------------------------------------------------
def _window_values(z, ok, foot, r, c):
    """The valid values of the window of cell (r, c): its cells (r + dy, c + dx) that lie on the grid and hold a height."""
    at = np.argwhere(foot) - np.array([foot.shape[0] // 2, foot.shape[1] // 2]) + np.array([r, c])
    at = at[(at[:, 0] >= 0) & (at[:, 0] < z.shape[0]) & (at[:, 1] >= 0) & (at[:, 1] < z.shape[1])]
    at = at[ok[at[:, 0], at[:, 1]]]
    return z[at[:, 0], at[:, 1]]


def select_loop(dsm, foot, levels, nodata=-999.0, centre=None):
    """-> (n int32 (gh, gw), lo, hi float32 (Q, gh, gw))."""
    z = np.ascontiguousarray(dsm, np.float32)
    ok = valid(z, nodata)
    gh, gw = z.shape
    n = np.zeros((gh, gw), np.int32)
    lo = np.full((len(levels), gh, gw), np.float32(nodata), np.float32)
    hi = lo.copy()
    for r in range(gh):
        for c in range(gw):
            v = _window_values(z, ok, foot, r, c)
            if centre is not None:
                v = _deviation(v, centre[r, c]) if np.isfinite(centre[r, c]) else v[:0]
            keys = sorted(int(k) for k in f2key(v))
            n[r, c] = len(keys)
            if not keys:
                continue
            for j, (num, den) in enumerate(levels):
                a, b, _ = rank_pair(len(keys), int(num), int(den))
                lo[j, r, c] = key2f(np.array([keys[a]], np.uint32))[0]
                hi[j, r, c] = key2f(np.array([keys[b]], np.uint32))[0]
    return n, lo, hi


def count_loop(dsm, foot, t, nodata=-999.0):
    """-> (n, below, equal) int32 (gh, gw)."""
    z = np.ascontiguousarray(dsm, np.float32)
    t = np.ascontiguousarray(t, np.float32)
    ok = valid(z, nodata)
    n, below, equal = (np.zeros(z.shape, np.int32) for _ in range(3))
    for r in range(z.shape[0]):
        for c in range(z.shape[1]):
            keys = [int(k) for k in f2key(_window_values(z, ok, foot, r, c))]
            n[r, c] = len(keys)
            if np.isnan(t[r, c]):
                below[r, c] = equal[r, c] = -1
                continue
            tk = int(f2key(t[r:r + 1, c:c + 1])[0, 0])
            below[r, c] = sum(1 for k in keys if k < tk)
            equal[r, c] = sum(1 for k in keys if k == tk)
    return n, below, equal


# ---- statement (b): vectorised -----------------------------------------------------------------------------------------------------
def _window_keys(dsm, foot, nodata, centre, r0, r1):
    """int64 keys (r1 - r0, gw, K) of the windows of rows r0 .. r1 - 1, VOID for what does not count."""
    z = np.ascontiguousarray(dsm, np.float32)
    ky, kx = foot.shape[0] // 2, foot.shape[1] // 2
    padded = np.full((r1 - r0 + 2 * ky, z.shape[1] + 2 * kx), np.float32(np.nan), np.float32)
    a, b = max(r0 - ky, 0), min(r1 + ky, z.shape[0])
    padded[a - (r0 - ky):b - (r0 - ky), kx:kx + z.shape[1]] = z[a:b]
    w = sliding_window_view(padded, foot.shape)[:, :, foot]
    ok = valid(w, nodata)
    if centre is not None:
        c = np.asarray(centre, np.float32)[r0:r1, :, None]
        ok &= np.isfinite(c)
        w = _deviation(w, c)
    return np.where(ok, f2key(w).astype(np.int64), VOID)


def select_sorted(dsm, foot, levels, nodata=-999.0, centre=None, band=16):
    z = np.ascontiguousarray(dsm, np.float32)
    gh, gw = z.shape
    n = np.zeros((gh, gw), np.int32)
    lo = np.full((len(levels), gh, gw), np.float32(nodata), np.float32)
    hi = lo.copy()
    for r0 in range(0, gh, band):
        r1 = min(r0 + band, gh)
        keys = np.sort(_window_keys(z, foot, nodata, centre, r0, r1), axis=-1)
        m = (keys != VOID).sum(axis=-1)
        n[r0:r1] = m
        some = m > 0
        for j, (num, den) in enumerate(levels):
            h = np.maximum(m.astype(np.int64) - 1, 0) * int(num)
            a = h // int(den)
            b = a + (h % int(den) > 0)
            for out, rank in ((lo, a), (hi, b)):
                k = np.take_along_axis(keys, rank[:, :, None], axis=-1)[:, :, 0]
                out[j, r0:r1] = np.where(some, key2f(np.where(some, k, 0).astype(np.uint32)), np.float32(nodata))
    return n, lo, hi


def count_sorted(dsm, foot, t, nodata=-999.0, band=16):
    z = np.ascontiguousarray(dsm, np.float32)
    t = np.ascontiguousarray(t, np.float32)
    n, below, equal = (np.zeros(z.shape, np.int32) for _ in range(3))
    for r0 in range(0, z.shape[0], band):
        r1 = min(r0 + band, z.shape[0])
        keys = _window_keys(z, foot, nodata, None, r0, r1)
        tk = f2key(t[r0:r1]).astype(np.int64)[:, :, None]
        nan = np.isnan(t[r0:r1])
        n[r0:r1] = (keys != VOID).sum(axis=-1)
        below[r0:r1] = np.where(nan, -1, (keys < tk).sum(axis=-1))
        equal[r0:r1] = np.where(nan, -1, (keys == tk).sum(axis=-1))
    return n, below, equal


# ---- the comparison -------------------------------------------------------------------------------------------------------------
def differing(got, want):
    """got, want: tuples of grids (None = not asked for, skipped); float32 by their bits.  None if equal, else the first cell."""
    for i, (g, w) in enumerate(zip(got, want)):
        if g is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        if g.shape != w.shape or g.dtype != w.dtype:
            return {"output": i, "shapes": (g.shape, w.shape), "dtypes": (g.dtype, w.dtype)}
        gb, wb = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else (g, w)
        bad = gb != wb
        if bad.any():
            at = tuple(int(v) for v in np.argwhere(bad)[0])
            return {"output": i, "cells_differing": int(bad.sum()), "at": at, "got": g[at].item(), "want": w[at].item(),
                    "got_bits": hex(int(gb[at])), "want_bits": hex(int(wb[at]))}
    return None


# ---- the Python layer -----------------------------------------------------------------------------------------------------------
def quantiles(dsm, foot, q=(0.5,), method="linear", centre=None, min_valid=1, nodata=-999.0, select=select_sorted):
    """What satmvs_amd.dsm.focal_quantiles returns."""
    fr = [qo.as_fraction(v) for v in q]
    levels = [(f.numerator, f.denominator) for f in fr]
    n, lo, hi = select(dsm, foot, levels, nodata, centre)
    m = n.astype(np.int64)
    val = np.empty(lo.shape, np.float64)
    for j, (num, den) in enumerate(levels):
        h = np.maximum(m - 1, 0) * num
        val[j] = qo.value(lo[j], hi[j], h // den, h % den, den, method)
    val = np.where((n >= max(min_valid, 1))[None], val, np.nan)
    return {"n_valid": n, "lo": lo, "hi": hi, "value": val}


def median(dsm, foot, min_valid=1, nodata=-999.0, fill=False):
    """What focal_median returns: despike's median, (float) of the midpoint of the two middle ranks."""
    z = np.ascontiguousarray(dsm, np.float32)
    got = quantiles(z, foot, (Fraction(1, 2),), "midpoint", None, min_valid, nodata)
    with np.errstate(invalid="ignore"):
        out = np.where(np.isnan(got["value"][0]), np.float32(nodata), got["value"][0].astype(np.float32))
    return out if fill else np.where(valid(z, nodata), out, z)


def nmad(dsm, foot, min_valid=1, nodata=-999.0):
    first = quantiles(dsm, foot, (Fraction(1, 2),), "linear", None, min_valid, nodata)
    med = first["value"][0]
    second = quantiles(dsm, foot, (Fraction(1, 2),), "linear", med.astype(np.float32), min_valid, nodata)
    mad = second["value"][0]
    return {"median": med, "mad": mad, "nmad": mad * 1.4826, "n_valid": first["n_valid"]}


def despike_robust(dsm, foot, k=3.0, floor=0.5, min_valid=3, nodata=-999.0):
    z = np.ascontiguousarray(dsm, np.float32)
    s = nmad(z, foot, min_valid, nodata)
    with np.errstate(invalid="ignore"):
        far = np.abs(z.astype(np.float64) - s["median"]) > np.maximum(k * s["nmad"], floor)
    removed = valid(z, nodata) & ((s["n_valid"] < min_valid) | far)
    return np.where(removed, np.float32(nodata), z), removed.astype(np.uint8)


def elevation_percentile(dsm, foot, min_valid=2, nodata=-999.0, count=count_sorted):
    z = np.ascontiguousarray(dsm, np.float32)
    n, below, equal = count(z, foot, z, nodata)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = (below.astype(np.float64) + 0.5 * (equal.astype(np.float64) - 1.0)) / (n.astype(np.float64) - 1.0)
    return np.where(valid(z, nodata) & (n >= max(min_valid, 2)), share, np.nan)


# ---- inputs the tests share -----------------------------------------------------------------------------------------------------
GRIDS = ((1, 1), (1, 70), (67, 1), (2, 2), (5, 63), (5, 64), (5, 65),
         (TILE - 1, 2 * TILE + 1), (TILE, TILE), (TILE + 1, TILE - 1), (2 * TILE + 1, TILE + 1))
LEVEL_SETS = (LEVELS[:4], LEVELS[4:] + ((1, 2),), ((1, 2),))


def windows(max_radius=8):
    out = [("box %d" % r, footprint("box", r)) for r in (0, 1, 3, 8) if r <= max_radius]
    out += [("disc %d" % r, footprint("disc", r)) for r in (0, 1, 3, 8) if r <= max_radius]
    if max_radius >= 8:
        out += [("annulus 4..8", footprint("annulus", 8, 4)), ("one row", footprint("row", 8)), ("one column", footprint("column", 8)),
                ("lopsided", footprint("lopsided", 5))]
    return out


def scene(gh, gw, seed, voids=0.1):
    """The kit's scene with about 10 % voids (NaN and nodata mixed) and a few cells at +Inf and -Inf, which are not valid either."""
    z = qo.kit_scene(gh, gw, seed, voids=voids, salt=0.02)
    rng = np.random.default_rng(seed + 1000)
    odd = rng.random((gh, gw))
    z[odd < 0.01] = np.inf
    z[odd > 0.99] = -np.inf
    return z


def matrix(large=True):
    """The cases both test files walk: dicts of name, dsm, foot, levels, nodata, centre (None or (gh, gw) float32).  large: with
    70 x 90 at radius 32 and 257 x 301 at radii <= 4, where statement (a) takes too long."""
    out = []

    def add(name, dsm, foot, levels, nodata=-999.0, centre=None):
        out.append({"name": name, "dsm": np.ascontiguousarray(dsm, np.float32), "foot": foot, "levels": tuple(levels), "nodata": nodata,
                    "centre": None if centre is None else np.ascontiguousarray(centre, np.float32)})

    turn = 0
    for i, (gh, gw) in enumerate(GRIDS):
        z = scene(gh, gw, 40 + i)
        for wname, foot in windows():
            add("scene %dx%d %s" % (gh, gw, wname), z, foot, LEVEL_SETS[turn % 3])
            turn += 1
    z = scene(70, 90, 7)
    for wname, foot in windows() + ([("box 32", footprint("box", 32)), ("disc 32", footprint("disc", 32))] if large else []):
        add("scene 70x90 %s" % wname, z, foot, LEVEL_SETS[turn % 3])
        turn += 1
    if large:
        z = scene(257, 301, 8)
        for wname, foot in windows(3) + [("box 4", footprint("box", 4)), ("disc 4", footprint("disc", 4))]:
            add("scene 257x301 %s" % wname, z, foot, LEVEL_SETS[turn % 3])
            turn += 1
    # values
    gh, gw = 33, 37
    rng = np.random.default_rng(5)
    spec = qo.special_values(gh, gw, seed=5)                 # both zeros, denormals, +-FLT_MAX, NaN, +-Inf, nodata, duplicates
    zeros = np.where(rng.random((gh, gw)) < 0.5, np.float32(0.0), np.float32(-0.0))
    den = (rng.integers(-40, 41, (gh, gw)).astype(np.float64) * 1.401298464324817e-45).astype(np.float32)
    other = np.where(rng.random((gh, gw)) < 0.2, np.float32(-1.0), scene(gh, gw, 9))
    for wname, foot in (("box 1", footprint("box", 1)), ("disc 3", footprint("disc", 3)), ("lopsided", footprint("lopsided", 5))):
        add("all invalid " + wname, np.where(rng.random((gh, gw)) < 0.5, np.float32(np.nan), np.float32(-999.0)), foot, LEVEL_SETS[0])
        add("one repeated value " + wname, np.full((gh, gw), 130.25, np.float32), foot, LEVEL_SETS[1])
        add("both zeros " + wname, zeros, foot, LEVEL_SETS[0])
        add("special values " + wname, spec, foot, LEVEL_SETS[turn % 3])
        add("denormals " + wname, den, foot, LEVEL_SETS[1])
        add("another nodata " + wname, other, foot, LEVEL_SETS[0], nodata=-1.0)
        turn += 1
    # deviation mode
    z = scene(gh, gw, 11)
    quarters = np.round(rng.normal(20.0, 4.0, (gh, gw)) * 4.0).astype(np.float32) / np.float32(4.0)      # ties with a centre
    for wname, foot in (("box 1", footprint("box", 1)), ("disc 3", footprint("disc", 3)), ("box 8", footprint("box", 8))):
        for vname, v in (("scene", z), ("quarters", quarters)):
            med = quantiles(v, foot, (Fraction(1, 2),))["value"][0].astype(np.float32)      # NaN where the window is empty
            med[3, 4], med[20, 30] = np.nan, np.inf
            add("deviation from the median, %s %s" % (vname, wname), v, foot, LEVEL_SETS[turn % 3], centre=med)
            turn += 1
        big = spec.copy()
        big[10, 10], big[10, 11] = FLT_MAX, -FLT_MAX
        c = np.where(rng.random((gh, gw)) < 0.5, FLT_MAX, -FLT_MAX).astype(np.float32)
        c[10, 10] = -FLT_MAX                                  # FLT_MAX - (-FLT_MAX) rounds to +Inf
        add("deviation that rounds to +Inf " + wname, big, foot, LEVEL_SETS[0], centre=c)
    return out
