"""The rule of the focal statistics (include/satmvs.h, "Focal statistics") in numpy and Python integers, stated twice:

  query_direct   a loop over every cell of every window with Python ints (small grids)
  query_tables   the prefix tables by cumsum over Python ints (object arrays) with an explicit wrap modulo 2^64, or over
                 uint64 arrays whose sums wrap the same way, then four corner differences per rectangle

and around them the header, the buffer's layout, the float rules restated from Python integers, the windows by brute force, the
float64 statements of the Python layer's grids and the cases.  numpy only: nothing here imports torch or the package.  `plant`
puts one named mistake into a statement, for the tests that show the comparison notices it."""
import math

import numpy as np

from dsm_testkit import scene, valid

SEG = 1024                   # FOCAL_SEG of csrc/dsm_focal.hip: table entries of one step of the row pass
BAND = 16                    # FOCAL_BAND: rows of one band of the column pass
HEADER_BYTES = 256
MAX_RECTS, MAX_OFFSET, MAX_AREA = 1024, 4096, 1 << 24
MOD = 1 << 64
PLANTS = ("c_up", "unclipped", "sample_var", "half_away", "high_word")
OUTPUTS = ("n", "s1", "s2", "mean", "var")


# ---- cells, header, layout ---------------------------------------------------------------------------------------------------------
def quantise(z, nodata=-999.0, plant=None):
    """-> (ok bool, q int64) per cell: valid iff finite, != (float)nodata and |z| <= 32768; q = rint(256 z), halves to even."""
    z = np.asarray(z, np.float32)
    with np.errstate(invalid="ignore"):
        ok = valid(z, nodata) & (np.abs(z) <= np.float32(32768.0))
    x = np.where(ok, z, np.float32(0)).astype(np.float64) * 256.0
    q = np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5)) if plant == "half_away" else np.rint(x)
    return ok, q.astype(np.int64)


def header(z, nodata=-999.0, plant=None):
    ok, q = quantise(z, nodata, plant)
    if not ok.any():
        return {"qmin": 0, "qmax": 0, "n_valid": 0, "c": 0, "D": 0}
    lo, hi = int(q[ok].min()), int(q[ok].max())
    c = -((-(lo + hi)) >> 1) if plant == "c_up" else (lo + hi) >> 1
    return {"qmin": lo, "qmax": hi, "n_valid": int(ok.sum()), "c": c, "D": max(c - lo, hi - c)}


def header_words(h):
    return np.array([h["qmin"], h["qmax"], h["n_valid"], h["c"], h["D"], 0, 0, 0], dtype=np.int64)


def _align(b):
    return (b + 255) & ~255


def layout(gw, gh):
    """Byte offsets of the tables in the buffer, the start of the working space behind them, and the buffer's size."""
    e, t = (gw + 1) * (gh + 1), ((gh + BAND - 1) // BAND) * gw
    n = HEADER_BYTES
    s1 = n + _align(e * 4)
    s2 = s1 + _align(e * 8)
    work = s2 + _align(e * 8)
    return {"n": n, "s1": s1, "s2": s2, "work": work, "bytes": work + _align(t * 4) + 2 * _align(t * 8) + MAX_RECTS * 8}


def split(buffer, gw, gh):
    """A table buffer (uint8 numpy) as (header words int64 (8), N int32, S1 int64, S2 uint64, each (gh + 1, gw + 1))."""
    l, e = layout(gw, gh), (gw + 1) * (gh + 1)
    b = np.ascontiguousarray(buffer, np.uint8)
    take = lambda at, dtype: b[at:at + e * np.dtype(dtype).itemsize].view(dtype).reshape(gh + 1, gw + 1)
    return b[:64].view(np.int64), take(l["n"], np.int32), take(l["s1"], np.int64), take(l["s2"], np.uint64)


# ---- the tables ------------------------------------------------------------------------------------------------------------------
def tables(z, nodata=-999.0, plant=None, exact=False):
    """-> (h, N int32, S1 int64, S2 uint64), (gh + 1, gw + 1) each, row 0 and column 0 zero.  exact: cumsum over Python ints, S2
    reduced modulo 2^64 at the end; otherwise over int64 / uint64 arrays, which wrap modulo 2^64 as they go: the same words."""
    h = header(z, nodata, plant)
    ok, q = quantise(z, nodata, plant)
    gh, gw = ok.shape
    d = np.where(ok, q - h["c"], 0)
    N = np.zeros((gh + 1, gw + 1), np.int32)
    S1 = np.zeros((gh + 1, gw + 1), np.int64)
    S2 = np.zeros((gh + 1, gw + 1), np.uint64)
    N[1:, 1:] = ok.astype(np.int64).cumsum(0).cumsum(1)
    S1[1:, 1:] = d.cumsum(0).cumsum(1)
    if exact:
        full = (d.astype(object) * d.astype(object)).cumsum(0).cumsum(1)
        S2[1:, 1:] = np.array([[int(v) % MOD for v in row] for row in full], dtype=np.uint64).reshape(gh, gw)
    else:
        S2[1:, 1:] = (d * d).astype(np.uint64).cumsum(0, dtype=np.uint64).cumsum(1, dtype=np.uint64)
    return h, N, S1, S2


# ---- the float rules, from Python integers ---------------------------------------------------------------------------------------
def mean_of(n, s1, c, min_valid=1):
    if n < max(min_valid, 1):
        return math.nan
    return (float(c) + float(s1) / float(n)) * 2.0 ** -8


def var_of(n, s1, s2, min_valid=1, plant=None):
    """s2 as the low 64 bits; V = n s2 - s1 s1 modulo 2^128, as the entry forms it."""
    if n < max(min_valid, 1):
        return math.nan
    V = (n * s2 - s1 * s1) % (1 << 128)
    Vd = float(V >> 64) * 2.0 ** 64 + float(V & (MOD - 1))
    if plant == "high_word":
        Vd = float(V >> 64) * 2.0 ** 64
    if plant == "sample_var":
        return Vd / (float(n) * float(n - 1)) * 2.0 ** -16 if n > 1 else math.nan
    return Vd / (float(n) * float(n)) * 2.0 ** -16


def _moments(n, s1, s2, c, min_valid, plant):
    flat = [(int(a), int(b), int(v)) for a, b, v in zip(n.reshape(-1), s1.reshape(-1), s2.reshape(-1))]
    mean = np.array([mean_of(a, b, c, min_valid) for a, b, _ in flat], dtype=np.float64).reshape(n.shape)
    var = np.array([var_of(a, b, v, min_valid, plant) for a, b, v in flat], dtype=np.float64).reshape(n.shape)
    return mean, var


def _centres(gw, gh, q):
    ow, oh = q.get("ow"), q.get("oh")
    c0, r0, sx, sy = q.get("c0", 0), q.get("r0", 0), q.get("sx", 1), q.get("sy", 1)
    if ow is None:
        ow, oh = (gw - 1 - c0) // sx + 1, (gh - 1 - r0) // sy + 1
    return r0 + sy * np.arange(oh), c0 + sx * np.arange(ow)


# ---- statement (a): every cell of every window -----------------------------------------------------------------------------------
def query_direct(z, rects, nodata=-999.0, min_valid=1, plant=None, **q):
    """-> dict n int32, s1 int64, s2 uint64 (low 64 bits), mean, var float64, (oh, ow) each, and the header h."""
    h = header(z, nodata, plant)
    ok, qq = quantise(z, nodata, plant)
    gh, gw = ok.shape
    rows, cols = _centres(gw, gh, q)
    n = np.zeros((len(rows), len(cols)), np.int32)
    s1 = np.zeros(n.shape, np.int64)
    s2 = np.zeros(n.shape, np.uint64)
    for R, r in enumerate(rows):
        for C, c in enumerate(cols):
            a, b, v = 0, 0, 0
            for dx0, dx1, dy0, dy1, sign in np.asarray(rects).tolist():
                for y in range(r + dy0, r + dy1 + 1):
                    for x in range(c + dx0, c + dx1 + 1):
                        if plant == "unclipped":
                            y, x = min(max(y, 0), gh - 1), min(max(x, 0), gw - 1)     # the edge cells stand in for the outside
                        elif not (0 <= y < gh and 0 <= x < gw):
                            continue
                        if ok[y, x]:
                            d = int(qq[y, x]) - h["c"]
                            a, b, v = a + sign, b + sign * d, v + sign * d * d
            n[R, C], s1[R, C], s2[R, C] = a, b, v % MOD
    mean, var = _moments(n, s1, s2, h["c"], min_valid, plant)
    return {"n": n, "s1": s1, "s2": s2, "mean": mean, "var": var, "h": h}


# ---- statement (b): corner differences of the prefix tables ----------------------------------------------------------------------
def query_tables(z, rects, nodata=-999.0, min_valid=1, plant=None, exact=False, **q):
    h, N, S1, S2 = tables(z, nodata, plant, exact)
    gh, gw = N.shape[0] - 1, N.shape[1] - 1
    rows, cols = _centres(gw, gh, q)
    n = np.zeros((len(rows), len(cols)), np.int64)
    s1 = np.zeros(n.shape, np.uint64)
    s2 = np.zeros(n.shape, np.uint64)
    U1 = S1.view(np.uint64)
    for dx0, dx1, dy0, dy1, sign in np.asarray(rects).tolist():
        x0, y0 = np.clip(cols + dx0, 0, gw), np.clip(rows + dy0, 0, gh)
        x1, y1 = np.maximum(np.clip(cols + dx1 + 1, 0, gw), x0), np.maximum(np.clip(rows + dy1 + 1, 0, gh), y0)
        box = lambda T: T[np.ix_(y1, x1)] - T[np.ix_(y0, x1)] - T[np.ix_(y1, x0)] + T[np.ix_(y0, x0)]
        dn, d1, d2 = box(N.astype(np.int64)), box(U1), box(S2)        # uint64 differences wrap modulo 2^64
        if sign > 0:
            n, s1, s2 = n + dn, s1 + d1, s2 + d2
        else:
            n, s1, s2 = n - dn, s1 - d1, s2 - d2
    n, s1 = n.astype(np.int32), s1.view(np.int64)
    mean, var = _moments(n, s1, s2, h["c"], min_valid, plant)
    return {"n": n, "s1": s1, "s2": s2, "mean": mean, "var": var, "h": h}


def differing(got, want, outputs=OUTPUTS):
    """None if every output agrees (integers by value, floats by their bits), else a line that names the first output and cell that
    differ."""
    for name in outputs:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        if g.shape != w.shape:
            return "%s: shape %s, want %s" % (name, g.shape, w.shape)
        if name in ("mean", "var"):
            gb, wb = np.ascontiguousarray(g, np.float64).view(np.uint64), np.ascontiguousarray(w, np.float64).view(np.uint64)
        else:
            gb, wb = g.astype(np.int64) if name == "n" else g.view(np.uint64), w.astype(np.int64) if name == "n" else w.view(np.uint64)
        bad = np.argwhere(gb != wb)
        if len(bad):
            at = tuple(int(v) for v in bad[0])
            return "%s differs at %d cells, first at %s: got %r, want %r" % (name, len(bad), at, g[at], w[at])
    return None


# ---- windows by brute force ------------------------------------------------------------------------------------------------------
def window_mask(shape, radius, inner=None, xres=1.0, yres=1.0, reach=None):
    """-> (member bool (2 k + 1, 2 k + 1), k): cell (dx, dy) at [dy + k, dx + k]."""
    k = reach if reach is not None else int(max(radius / xres, radius / yres)) + 2
    dx = np.arange(-k, k + 1, dtype=np.float64)[None, :] * np.float64(xres)
    dy = np.arange(-k, k + 1, dtype=np.float64)[:, None] * np.float64(yres)
    r = np.float64(radius)
    if shape == "box":
        return (np.abs(dx) <= r) & (np.abs(dy) <= r), k
    d2 = dx * dx + dy * dy
    m = d2 <= r * r
    if shape == "annulus":
        m &= d2 > np.float64(inner) * np.float64(inner)
    return m, k


def rasterise(rects, k):
    """The signed count of the records over (dx, dy) in [-k, k]^2: 1 on a window's members and 0 elsewhere if it is sound."""
    out = np.zeros((2 * k + 1, 2 * k + 1), np.int64)
    for dx0, dx1, dy0, dy1, sign in np.asarray(rects).tolist():
        assert -k <= dx0 and dx1 <= k and -k <= dy0 and dy1 <= k
        out[dy0 + k:dy1 + k + 1, dx0 + k:dx1 + k + 1] += sign
    return out


def box(rx, ry=None):
    ry = rx if ry is None else ry
    return np.array([[-rx, rx, -ry, ry, 1]], dtype=np.int32)


def disc(radius, sign=1):
    """A disc in cells as records, row by row merged, from the brute-force mask."""
    m, k = window_mask("disc", radius)
    hx = m.sum(axis=1)
    out, start = [], None
    for i in range(2 * k + 2):
        w = hx[i] if i <= 2 * k else -1
        if start is not None and w != hx[start]:
            out.append(((1 - hx[start]) // 2, (hx[start] - 1) // 2, start - k, i - 1 - k, sign))
            start = None
        if start is None and w > 0:
            start = i
    return np.array(out, dtype=np.int32)


def annulus(radius, inner):
    return np.concatenate([disc(radius), disc(inner, -1)])


def many_records(k):
    """k one-cell records on a diagonal that steps two columns a row, signs +1: a window no two records of which merge."""
    return np.array([[2 * i - k, 2 * i - k, i - k // 2, i - k // 2, 1] for i in range(k)], dtype=np.int32)


# ---- the Python layer's grids in float64 ----------------------------------------------------------------------------------------
def grid_of(value, keep, nodata=-999.0):
    keep = keep & ~np.isnan(value)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(keep, value.astype(np.float32), np.float32(nodata)).astype(np.float32)


def tpi_terms(z, n, mean, var, nodata=-999.0, min_valid=1):
    """(t = (double)z - mean, std, keep) from a query's own n, mean and var."""
    ok, _ = quantise(z, nodata)
    with np.errstate(invalid="ignore"):
        return np.asarray(z, np.float32).astype(np.float64) - mean, np.sqrt(var), ok & (n >= min_valid)


def slope_codes(d, s, slope_deg=5.0, nodata=-999.0):
    """The class map from dev (float32, nodata where none) and slope (float32, NaN where none)."""
    cls = np.full(d.shape, 3, np.uint8)
    with np.errstate(invalid="ignore"):
        cls[s > slope_deg] = 4
        cls[d <= -0.5] = 2
        cls[d <= -1.0] = 1
        cls[d >= 0.5] = 5
        cls[d >= 1.0] = 6
    cls[(d == np.float32(nodata)) | np.isnan(s)] = 0
    return cls


def block_mean(z, f, nodata=-999.0, min_valid=1):
    """aggregate() from the integers of each block: (mean float32 with nodata, count int32)."""
    got = query_tables(z, np.array([[0, f - 1, 0, f - 1, 1]]), nodata, min_valid, sx=f, sy=f)
    return grid_of(got["mean"], got["n"] >= min_valid, nodata), got["n"]


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def kit_scene(gh, gw, seed, voids=0.0, salt=0.0):
    E, N = np.meshgrid(5.0 * np.arange(gw), 5.0 * np.arange(gh)[::-1])
    return scene(E, N, seed=seed, voids=voids, salt=salt)


def edge_values(gh, gw, seed):
    """Heights on quantisation halves, both zeros, NaN, +-Inf, nodata, +-32768 and one ulp beyond, scattered over a gentle ramp."""
    rng = np.random.default_rng(seed)
    z = (rng.integers(-2000, 2000, (gh, gw)) / 512.0).astype(np.float32)          # every other one a half of the quantum
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, -999.0, 32768.0, -32768.0, np.nextafter(np.float32(32768.0), np.float32(np.inf)),
                        np.nextafter(np.float32(-32768.0), np.float32(-np.inf)), 0.001953125, -0.001953125, 0.005859375], dtype=np.float32)
    at = rng.choice(gh * gw, size=min(gh * gw, 3 * len(special)), replace=False)
    z.reshape(-1)[at] = np.resize(special, len(at))
    return z


def checkerboard(gh, gw, height=32768.0):
    r, c = np.indices((gh, gw))
    return np.where((r + c) % 2 == 0, np.float32(height), np.float32(-height)).astype(np.float32)


def matrix(large=True):
    """[(name, z, nodata, rects, query)]: small cases for both statements; with `large`, those only statement (b) can afford."""
    cases = []
    for gh, gw in ((1, 1), (1, 70), (67, 1), (2, 2), (67, 3)):
        z = edge_values(gh, gw, seed=gh * 100 + gw)
        cases.append(("edge %dx%d box1" % (gh, gw), z, -999.0, box(1), {}))
        cases.append(("edge %dx%d disc2.5 min_valid 9" % (gh, gw), z, -999.0, disc(2.5), {"min_valid": 9}))
    z = kit_scene(19, 23, seed=3, voids=0.3, salt=0.05)
    cases.append(("scene 19x23 asymmetric", z, -999.0, np.array([[-3, 1, 0, 4, 1], [2, 2, -5, -5, 1]], np.int32), {}))
    cases.append(("scene 19x23 annulus", z, -999.0, annulus(4, 2), {"min_valid": 0}))
    cases.append(("scene 19x23 stride", z, -999.0, np.array([[0, 3, 0, 2, 1]], np.int32), {"sx": 4, "sy": 3}))
    cases.append(("scene 19x23 origin", z, -999.0, box(2), {"c0": 22, "r0": 18, "ow": 1, "oh": 1}))
    cases.append(("scene 19x23 larger than the grid", z, -999.0, box(40), {"sx": 5, "sy": 5}))
    cases.append(("all invalid", np.full((5, 7), np.nan, np.float32), -999.0, box(1), {}))
    one = np.full((5, 7), -999.0, np.float32)
    one[3, 2] = 12.5
    cases.append(("one valid cell", one, -999.0, box(1), {}))
    cases.append(("checkerboard 12x12", checkerboard(12, 12), -999.0, box(3), {}))
    if large:
        z = kit_scene(257, 301, seed=5, voids=0.05, salt=0.01)
        cases.append(("scene 257x301 disc 100", z, -999.0, disc(100), {}))
        cases.append(("scene 257x301 box 31 nan nodata", z, np.nan, box(31), {"min_valid": 9}))
    return cases
