"""Test-local numpy oracle of the DSM clean-up (include/satmvs.h smvs_dsm_despike / smvs_dsm_fill, DESIGN.md section 9,
"Cleaning a DSM"), float64 where the rules say so, and a second, independent statement of the same rules as a Python loop per
cell (despike_brute / fill_brute) that the CPU tests hold against the vectorised one bit for bit.

despike(): the window as (2 radius + 1)^2 shifted copies of the padded grid, sorted along the stack with invalid cells as +inf.
fill():    the directional search as shifted-array passes: step k looks, for every void cell still without a hit in direction
           d, at the cell k steps along d; the lists of unresolved cells shrink as hits are found, so the cost is the sum of
           the reaches, not max_steps per cell."""
import numpy as np

import dsm_testkit as kit
from dsm_testkit import same_bits, valid  # noqa: F401  (re-exported)

# (dcol, drow), rows running south: E, NE, N, NW, W, SW, S, SE
DIRS = ((1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1))
METHODS = ("idw", "nearest", "min")


def median_of_sorted(v, n):
    """The median rule of smvs_dsm_reduce on rows of ascending float32 values v[..., :n] (n >= 1 per row) -> float32."""
    i = np.arange(v.shape[0])
    hi = v[i, n // 2]
    lo = v[i, np.maximum(n // 2 - 1, 0)]
    even = (0.5 * (lo.astype(np.float64) + hi.astype(np.float64))).astype(np.float32)
    return np.where(n % 2 == 1, hi, even)


def despike(dsm, nodata=-999.0, radius=2, thresh=10.0, min_valid=3, band=256):
    """-> (cleaned float32, removed uint8).  Row bands keep the window stack small."""
    z = np.asarray(dsm, np.float32)
    gh, gw = z.shape
    ok = valid(z, nodata)
    R = int(radius)
    pad = np.full((gh + 2 * R, gw + 2 * R), np.inf, np.float32)
    pad[R:R + gh, R:R + gw] = np.where(ok, z, np.float32(np.inf))
    removed = np.zeros((gh, gw), bool)
    for r0 in range(0, gh, band):
        r1 = min(gh, r0 + band)
        rows, cols = np.nonzero(ok[r0:r1])
        if rows.size == 0:
            continue
        win = np.stack([pad[r0 + dr:r1 + dr, dc:dc + gw][rows, cols] for dr in range(2 * R + 1) for dc in range(2 * R + 1)], axis=1)
        win.sort(axis=1)                                                     # +inf (invalid, off the grid) goes last
        n = np.isfinite(win).sum(axis=1)
        m = median_of_sorted(win, n)
        far = np.abs(z[r0:r1][rows, cols].astype(np.float64) - m.astype(np.float64)) > float(thresh)
        removed[r0 + rows, cols] = (n < int(min_valid)) | far
    out = z.copy()
    out[removed] = np.float32(nodata)
    return out, removed.astype(np.uint8)


def hits_of(dsm, nodata, max_steps):
    """(k (8, gh, gw) int64, 0 = no hit; zhit (8, gh, gw) float32) of every invalid cell, by shifted passes."""
    z = np.asarray(dsm, np.float32)
    gh, gw = z.shape
    ok = valid(z, nodata)
    k_out = np.zeros((8, gh, gw), np.int64)
    z_out = np.zeros((8, gh, gw), np.float32)
    vr, vc = np.nonzero(~ok)
    for d, (dc, dr) in enumerate(DIRS):
        r, c = vr, vc
        for k in range(1, int(max_steps) + 1):
            if r.size == 0:
                break
            hr, hc = r + k * dr, c + k * dc
            on = (hr >= 0) & (hr < gh) & (hc >= 0) & (hc < gw)
            r, c, hr, hc = r[on], c[on], hr[on], hc[on]                      # a line that left the grid finds nothing more
            hit = ok[hr, hc]
            k_out[d, r[hit], c[hit]] = k
            z_out[d, r[hit], c[hit]] = z[hr[hit], hc[hit]]
            r, c = r[~hit], c[~hit]
    return k_out, z_out


def fill(dsm, nodata=-999.0, max_steps=32, min_hits=3, method="idw"):
    """-> (filled float32, hits uint8: 255 where the input cell was valid)."""
    assert method in METHODS
    z = np.asarray(dsm, np.float32)
    ok = valid(z, nodata)
    k, zh = hits_of(z, nodata, max_steps)
    has = k > 0
    nh = has.sum(axis=0)
    mult = np.array([1.0, 2.0] * 4).reshape(8, 1, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        d2 = k.astype(np.float64) * k.astype(np.float64) * mult              # an exact integer
        if method == "idw":
            num = np.zeros(z.shape, np.float64)
            den = np.zeros(z.shape, np.float64)
            for d in range(8):                                               # the fixed order of the sums
                w = 1.0 / d2[d]
                num = np.where(has[d], num + w * zh[d].astype(np.float64), num)
                den = np.where(has[d], den + w, den)
            value = (num / den).astype(np.float32)
        else:
            value = np.zeros(z.shape, np.float32)
            best = np.full(z.shape, np.inf)
            for d in range(8):                                               # strict comparisons: ties keep the earlier direction
                score = d2[d] if method == "nearest" else zh[d].astype(np.float64)
                take = has[d] & (score < best)
                value = np.where(take, zh[d], value)
                best = np.where(take, score, best)
    filled = ~ok & (nh >= int(min_hits))
    out = z.copy()
    out[filled] = value[filled]
    return out, np.where(ok, 255, nh).astype(np.uint8)


# ---- the same rules, one cell at a time ------------------------------------------------------------------------------------
def despike_brute(dsm, nodata=-999.0, radius=2, thresh=10.0, min_valid=3):
    z = np.asarray(dsm, np.float32)
    gh, gw = z.shape
    ok = valid(z, nodata)
    out = z.copy()
    removed = np.zeros((gh, gw), np.uint8)
    for r in range(gh):
        for c in range(gw):
            if not ok[r, c]:
                continue
            v = sorted(float(z[rr, cc]) for rr in range(max(0, r - radius), min(gh, r + radius + 1))
                       for cc in range(max(0, c - radius), min(gw, c + radius + 1)) if ok[rr, cc])
            n = len(v)
            if n >= min_valid:
                m = v[n // 2] if n % 2 else float(np.float32(0.5 * (v[n // 2 - 1] + v[n // 2])))    # Python floats are float64
                if not abs(float(z[r, c]) - m) > thresh:
                    continue
            out[r, c] = np.float32(nodata)
            removed[r, c] = 1
    return out, removed


def fill_brute(dsm, nodata=-999.0, max_steps=32, min_hits=3, method="idw"):
    z = np.asarray(dsm, np.float32)
    gh, gw = z.shape
    ok = valid(z, nodata)
    out = z.copy()
    hits = np.full((gh, gw), 255, np.uint8)
    for r in range(gh):
        for c in range(gw):
            if ok[r, c]:
                continue
            found = []                                                       # (d2, height) in direction order
            for i, (dc, dr) in enumerate(DIRS):
                for k in range(1, max_steps + 1):
                    rr, cc = r + k * dr, c + k * dc
                    if not (0 <= rr < gh and 0 <= cc < gw):
                        break
                    if ok[rr, cc]:
                        found.append((k * k * (2 if i % 2 else 1), z[rr, cc]))
                        break
            hits[r, c] = len(found)
            if len(found) < min_hits:
                continue
            if method == "idw":
                num = den = 0.0
                for d2, zd in found:
                    w = 1.0 / float(d2)
                    num += w * float(zd)
                    den += w
                out[r, c] = np.float32(num / den)
            elif method == "nearest":
                out[r, c] = min(found, key=lambda t: t[0])[1]                # min() keeps the first of equal keys
            else:
                out[r, c] = min(found, key=lambda t: float(t[1]))[1]
    return out, hits


# ---- what the tests compare and build scenes from ----------------------------------------------------------------------------
def scene(gh, gw, seed=0, voids=0.1, salt=0.02):
    """dsm_testkit.scene on a (gh, gw) grid of 5 m cells, with seeded salt noise and random voids."""
    rows, cols = np.mgrid[0:gh, 0:gw].astype(np.float64)
    return kit.scene(5.0 * cols, -5.0 * rows, seed=seed, voids=voids, salt=salt)
