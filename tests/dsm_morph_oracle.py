"""Test-local numpy oracle of the ground extraction (include/satmvs.h smvs_dsm_morph / smvs_dsm_ground, DESIGN.md section 9,
"Ground extraction"), stated twice: vectorised over fields of order-preserving keys, and as a plain Python loop per cell over
the clipped window (the *_brute functions) that the CPU tests hold against the vectorised one bit for bit.  Plus the schedule
of the ground filter, the nDSM, and the generators of the test scenes.  Nothing here imports satmvs_amd.

A field is a uint32 array of keys: key(z) orders like z, with -0.0 below +0.0, and 0 stands for "invalid / none".  The lowest
of a window is the highest of the complements, so there is one window operation, the maximum, with 0 as its identity."""
import numpy as np

from dsm_testkit import f2key, key2f, same_bits, valid  # noqa: F401  (re-exported)

OPS = ("erode", "dilate", "open", "close")


def keys_of(z, nodata):
    """The field of a grid: keys at valid cells, 0 elsewhere."""
    return np.where(valid(z, nodata), f2key(z), np.uint32(0)).astype(np.uint32)


def flip(k):
    """Complements of the keys of a field; "none" stays none.  (No valid float has key 0xffffffff, so no complement is 0.)"""
    return np.where(k != 0, ~k, np.uint32(0)).astype(np.uint32)


def window_max(k, r):
    """Highest key of the (2 r + 1)^2 window clipped at the border: rows, then columns.  Along a line of the zero-padded
    field, m[i] = max of [i, i + span) by doubling up to the largest span = 2^j <= 2 r + 1, and the window of cell i is the
    union of the runs at i and at i + 2 r + 1 - span (so the cost grows with log r, and a 2048^2 grid stays testable)."""
    w = 2 * r + 1
    for axis in (1, 0):
        m = np.moveaxis(k, axis, 1)
        n = m.shape[1]
        m = np.pad(m, [(0, 0), (r, r)])
        span = 1
        while 2 * span <= w:
            m = np.maximum(m, np.pad(m[:, span:], [(0, 0), (0, span)]))
            span *= 2
        k = np.moveaxis(np.maximum(m[:, :n], m[:, w - span:w - span + n]), 1, axis)
    return np.ascontiguousarray(k)


def dilate_keys(k, r):
    return window_max(k, r)


def erode_keys(k, r):
    return flip(window_max(flip(k), r))


def open_keys(k, r):
    return dilate_keys(erode_keys(k, r), r)


def close_keys(k, r):
    return erode_keys(dilate_keys(k, r), r)


KEY_OPS = {"erode": erode_keys, "dilate": dilate_keys, "open": open_keys, "close": close_keys}


def morph(dsm, radius, op, nodata=-999.0):
    """-> float32: the result at valid cells, the input's bits elsewhere."""
    z = np.ascontiguousarray(dsm, np.float32)
    k = KEY_OPS[op](keys_of(z, nodata), int(radius))
    ok = valid(z, nodata)
    out = z.copy()
    out[ok] = key2f(k)[ok]
    return out


def schedule(cell, max_radius=16, slope=0.3, dh0=1.5, dh_max=6.0):
    radii = []
    r = 1
    while r < max_radius:
        radii.append(r)
        r *= 2
    radii.append(int(max_radius))
    w = [2 * r + 1 for r in radii]
    thresholds = [float(dh0)] + [min(float(dh_max), float(slope) * float(w[k] - w[k - 1]) * float(cell) + float(dh0))
                                 for k in range(1, len(w))]
    return radii, thresholds


def ground(dsm, radii, thresholds, nodata=-999.0, opening=open_keys):
    """-> (dtm float32, cls uint8)."""
    z = np.ascontiguousarray(dsm, np.float32)
    ok = valid(z, nodata)
    S = keys_of(z, nodata)
    cls = ok.astype(np.uint8)
    for k, (r, t) in enumerate(zip(radii, thresholds)):
        O = opening(S, int(r))
        drop = np.zeros(z.shape, np.float64)
        drop[ok] = key2f(S)[ok].astype(np.float64) - key2f(O)[ok].astype(np.float64)
        cls[ok & (cls == 1) & (drop > float(t))] = 2 + k
        S = np.where(ok, O, np.uint32(0)).astype(np.uint32)
    dtm = z.copy()
    dtm[cls >= 2] = np.float32(nodata)
    return dtm, cls


def ndsm(dsm, dtm, nodata=-999.0, clamp=True):
    a, b = np.asarray(dsm, np.float32), np.asarray(dtm, np.float32)
    both = valid(a, nodata) & valid(b, nodata)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (a - b).astype(np.float32)
    if clamp:
        d = np.where(d > 0, d, np.float32(0.0)).astype(np.float32)
    return np.where(both, d, np.float32(nodata)).astype(np.float32)


# ---- the same rules, one cell at a time ------------------------------------------------------------------------------------
def _extreme_brute(val, has, r, lowest):
    """val float32, has bool (where the field is defined) -> (val', has'): the lowest / highest defined value of every
    cell's clipped window, by the order of the keys."""
    gh, gw = val.shape
    out, out_has = np.zeros((gh, gw), np.float32), np.zeros((gh, gw), bool)
    keys, has = f2key(val).tolist(), np.asarray(has).tolist()              # Python ints and bools: the loop below is plain Python
    for i in range(gh):
        for j in range(gw):
            best = None
            for ii in range(max(0, i - r), min(gh, i + r + 1)):
                for jj in range(max(0, j - r), min(gw, j + r + 1)):
                    if has[ii][jj]:
                        kk = keys[ii][jj]
                        if best is None or (kk < best[0] if lowest else kk > best[0]):
                            best = (kk, val[ii, jj])
            if best is not None:
                out[i, j], out_has[i, j] = best[1], True
    return out, out_has


def morph_brute(dsm, radius, op, nodata=-999.0):
    z = np.ascontiguousarray(dsm, np.float32)
    ok = valid(z, nodata)
    first_lowest = op in ("erode", "open")
    v, h = _extreme_brute(z, ok, radius, first_lowest)
    if op in ("open", "close"):
        v, h = _extreme_brute(v, h, radius, not first_lowest)
    out = z.copy()
    out[ok] = v[ok]
    return out


def ground_brute(dsm, radii, thresholds, nodata=-999.0):
    z = np.ascontiguousarray(dsm, np.float32)
    ok = valid(z, nodata)
    S = z.copy()
    cls = ok.astype(np.uint8)
    for k, (r, t) in enumerate(zip(radii, thresholds)):
        v, h = _extreme_brute(S, ok, r, True)
        O, _ = _extreme_brute(v, h, r, False)
        for i, j in zip(*np.nonzero(ok)):
            if cls[i, j] == 1 and float(S[i, j]) - float(O[i, j]) > t:
                cls[i, j] = 2 + k
        S = np.where(ok, O, S)
    dtm = z.copy()
    dtm[cls >= 2] = np.float32(nodata)
    return dtm, cls


# ---- what the tests compare and build scenes from ----------------------------------------------------------------------------
def scene(gh, gw, seed=0, voids=0.1):
    """Terrain with blocks, both zeros, +-inf and NaN cells, a nodata hole and random voids (NaN and nodata mixed)."""
    rng = np.random.default_rng(seed)
    rows, cols = np.mgrid[0:gh, 0:gw].astype(np.float64)
    z = (20.0 * np.sin(cols / 11.0) * np.cos(rows / 14.0) + rng.normal(0.0, 0.5, (gh, gw))).astype(np.float32)
    for _ in range(max(1, gh * gw // 400)):
        r0, c0 = int(rng.integers(0, gh)), int(rng.integers(0, gw))
        z[r0:r0 + int(rng.integers(1, 9)), c0:c0 + int(rng.integers(1, 9))] += np.float32(rng.uniform(5.0, 60.0))
    flat = rng.random((gh, gw))
    z[flat < 0.02] = np.float32(0.0)
    z[(flat >= 0.02) & (flat < 0.04)] = np.float32(-0.0)
    z[(flat >= 0.04) & (flat < 0.045)] = np.float32(np.inf)
    z[(flat >= 0.045) & (flat < 0.05)] = np.float32(-np.inf)
    z[gh // 3:gh // 3 + 5, gw // 4:gw // 4 + 7] = np.float32(-999.0)
    gone = rng.random((gh, gw)) < voids
    z[gone] = np.where(rng.random((gh, gw)) < 0.5, np.float32(np.nan), np.float32(-999.0))[gone]
    return z


def known_answer_scene(gh=600, gw=700, seed=1, nodata=-999.0):
    """5 m cells; ground 200 + 0.4 col - 0.25 row + 30 sin(col / 90) cos(row / 70) m; 150 boxes with sides of 2 .. 24 cells
    set to the highest ground under them + 8 .. 80 m; noise sigma 0.3 m; 3 % nodata; one 60 x 80 block NaN.
    -> (dsm float32, is_box bool)."""
    rng = np.random.default_rng(seed)
    rows, cols = np.mgrid[0:gh, 0:gw].astype(np.float64)
    ground_z = 200.0 + 0.4 * cols - 0.25 * rows + 30.0 * np.sin(cols / 90.0) * np.cos(rows / 70.0)
    z = ground_z.copy()
    box = np.zeros((gh, gw), bool)
    for _ in range(150):
        h, w = int(rng.integers(2, 25)), int(rng.integers(2, 25))
        r0, c0 = int(rng.integers(0, gh - h + 1)), int(rng.integers(0, gw - w + 1))
        z[r0:r0 + h, c0:c0 + w] = ground_z[r0:r0 + h, c0:c0 + w].max() + rng.uniform(8.0, 80.0)
        box[r0:r0 + h, c0:c0 + w] = True
    z = (z + rng.normal(0.0, 0.3, (gh, gw))).astype(np.float32)
    z[rng.random((gh, gw)) < 0.03] = np.float32(nodata)
    z[200:260, 300:380] = np.float32(np.nan)
    return z, box
