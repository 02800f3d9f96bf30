"""The numpy statements of the sun rules (include/satmvs.h, "Sun"): cast shadows stated three times (a loop per line, a shear
with np.maximum.accumulate, and an O(n^2) search over pairs of cells), Horn's gradient, the float64 hillshade, and the closed
form of a box's shadow on a plane.  numpy only.  `plant` puts a known mistake into a statement (tests/test_dsm_sun_cpu.py)."""
import math

import numpy as np

from dsm_testkit import valid  # noqa: F401  (re-exported)

MINKEY = np.int64(-0x7ff0000000000001)                                       # the key of -inf
_LOW63 = np.int64(0x7fffffffffffffff)


def d2key(g):
    """The order-preserving int64 image of float64 values: signed order = the doubles' order, -0.0 below +0.0."""
    u = np.ascontiguousarray(g, np.float64).view(np.int64)
    return u ^ ((u >> np.int64(63)) & _LOW63)


def key2d(k):
    k = np.ascontiguousarray(k, np.int64)
    return (k ^ ((k >> np.int64(63)) & _LOW63)).view(np.float64)


def keys(z, a, b):
    """g(r, c) = (double)z - (a c + b r), every operation rounded by itself."""
    gh, gw = z.shape
    r, c = np.mgrid[0:gh, 0:gw].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return z.astype(np.float64) - (np.float64(a) * c + np.float64(b) * r)


def lines(gh, gw, ucol, urow, plant=None):
    """(row_major, s, ascending): s over the scan axis (rows if row_major, else columns)."""
    row_major = abs(urow) >= abs(ucol)
    along, across, n = (urow, ucol, gh) if row_major else (ucol, urow, gw)
    m = np.float64(across) / np.float64(along)
    x = m * np.arange(n, dtype=np.float64)
    s = (np.rint(x) if plant == "rint" else np.floor(x + 0.5)).astype(np.int64)
    ascending = along < 0
    if plant == "order":
        ascending = not ascending
    return row_major, s, ascending


def _finish(z, nodata, ok, g, G, tol):
    with np.errstate(invalid="ignore", over="ignore"):
        d = G - g
        shade = np.where(ok, np.where(d > tol, 2, 1), 0).astype(np.uint8)
        depth = np.where(ok, d.astype(np.float32), np.float32(nodata)).astype(np.float32)
    return shade, depth


def shadow_loop(z, nodata, ucol, urow, a, b, tol, plant=None, band=32):
    """The rule cell by cell: every line walked in sunward order with a running maximum."""
    z = np.asarray(z, np.float32)
    gh, gw = z.shape
    row_major, s, ascending = lines(gh, gw, ucol, urow, plant)
    ok, g = valid(z, nodata), keys(z, a, b)
    k = d2key(g)
    G = np.full((gh, gw), MINKEY, np.int64)
    run = {}
    n = gh if row_major else gw
    for step, i in enumerate(range(n) if ascending else range(n - 1, -1, -1)):
        if plant == "no carry" and step % band == 0:
            run = {}
        for j in range(gw if row_major else gh):
            r, c = (i, j) if row_major else (j, i)
            L = j - int(s[i])
            if not ok[r, c] and plant != "invalid occlude":
                continue
            if plant == "inclusive":
                run[L] = max(run.get(L, MINKEY), k[r, c])
            G[r, c] = run.get(L, MINKEY)
            run[L] = max(run.get(L, MINKEY), k[r, c])
    return _finish(z, nodata, ok, g, key2d(G), tol)


def _scan_rows(k, s, ascending):
    """The exclusive running maximum of the keys k (H, W; MINKEY where a cell does not count) along the lines c - s(r)."""
    H, W = k.shape
    smax, smin = max(int(s.max()), 0), min(int(s.min()), 0)
    nl = W + smax - smin
    col = np.arange(W)[None, :] - s[:, None] + smax           # the slot of cell (r, c) in the sheared array
    row = np.arange(H)[:, None] + np.zeros((1, W), np.int64)
    sheared = np.full((H, nl), MINKEY, np.int64)
    sheared[row, col] = k
    if not ascending:
        sheared = sheared[::-1]
    acc = np.maximum.accumulate(sheared, axis=0)
    acc = np.concatenate([np.full((1, nl), MINKEY, np.int64), acc[:-1]], axis=0)      # exclusive: shifted by one
    if not ascending:
        acc = acc[::-1]
    return acc[row, col]


def shadow_scan(z, nodata, ucol, urow, a, b, tol):
    """The rule as a shear and np.maximum.accumulate; the column-major directions on the transposed grid with (ucol, urow)
    and (a, b) swapped."""
    z = np.asarray(z, np.float32)
    if abs(urow) < abs(ucol):
        shade, depth = shadow_scan(np.ascontiguousarray(z.T), nodata, urow, ucol, b, a, tol)
        return np.ascontiguousarray(shade.T), np.ascontiguousarray(depth.T)
    gh, gw = z.shape
    _, s, ascending = lines(gh, gw, ucol, urow)
    ok, g = valid(z, nodata), keys(z, a, b)
    G = _scan_rows(np.where(ok, d2key(g), MINKEY), s, ascending)
    return _finish(z, nodata, ok, g, key2d(G), tol)


def shadow_brute(z, nodata, ucol, urow, a, b, tol):
    """O(n^2), for tiny grids: every valid cell against every valid cell of its line that lies sunward."""
    z = np.asarray(z, np.float32)
    gh, gw = z.shape
    row_major, s, ascending = lines(gh, gw, ucol, urow)
    r, c = np.mgrid[0:gh, 0:gw]
    pos = (r if row_major else c).ravel()                    # along the scan
    line = ((c - s[r]) if row_major else (r - s[c])).ravel()
    ok, g = valid(z, nodata).ravel(), keys(z, a, b).ravel()
    k = d2key(g)
    before = (pos[None, :] < pos[:, None]) if ascending else (pos[None, :] > pos[:, None])
    counts = before & (line[None, :] == line[:, None]) & ok[None, :]
    G = np.where(counts, k[None, :], MINKEY).max(axis=1)
    shade, depth = _finish(z.ravel(), nodata, ok, g, key2d(G), tol)
    return shade.reshape(gh, gw), depth.reshape(gh, gw)


# ---- gradient and hillshade -------------------------------------------------------------------------------------------------
def gradient(z, nodata, xres, yres):
    z = np.asarray(z, np.float32)
    gh, gw = z.shape
    ok = valid(z, nodata)
    zd = z.astype(np.float64)
    pad_z = np.pad(zd, 1, constant_values=0.0)
    pad_ok = np.pad(ok, 1, constant_values=False)

    def n(dr, dc):
        """The neighbour (dr, dc), the centre where it is off the grid or invalid."""
        sl = (slice(1 + dr, 1 + dr + gh), slice(1 + dc, 1 + dc + gw))
        return np.where(pad_ok[sl], pad_z[sl], zd)

    with np.errstate(invalid="ignore", over="ignore"):
        de = (((n(-1, 1) + 2.0 * n(0, 1)) + n(1, 1)) - ((n(-1, -1) + 2.0 * n(0, -1)) + n(1, -1))) / (8.0 * np.float64(xres))
        dn = (((n(-1, -1) + 2.0 * n(-1, 0)) + n(-1, 1)) - ((n(1, -1) + 2.0 * n(1, 0)) + n(1, 1))) / (8.0 * np.float64(yres))
        nd = np.float32(nodata)
        return np.where(ok, de.astype(np.float32), nd).astype(np.float32), np.where(ok, dn.astype(np.float32), nd).astype(np.float32)


def cos_incidence(dzde, dzdn, azimuth, elevation):
    """max(0, (sinE - cosE (dzde sA + dzdn cA)) / sqrt(1 + dzde^2 + dzdn^2)) in float64."""
    de, dn = np.asarray(dzde, np.float64), np.asarray(dzdn, np.float64)
    sA, cA = math.sin(math.radians(azimuth)), math.cos(math.radians(azimuth))
    sE, cE = math.sin(math.radians(elevation)), math.cos(math.radians(elevation))
    return np.maximum((sE - cE * (de * sA + dn * cA)) / np.sqrt(1.0 + de * de + dn * dn), 0.0)


# ---- the closed form: a box on a plane ---------------------------------------------------------------------------------------
def _hull(points):
    """Convex hull (monotone chain), counter-clockwise, of a list of (x, y)."""
    pts = sorted(set(points))

    def half(seq):
        h = []
        for p in seq:
            while len(h) >= 2 and (h[-1][0] - h[-2][0]) * (p[1] - h[-2][1]) - (h[-1][1] - h[-2][1]) * (p[0] - h[-2][0]) <= 0:
                h.pop()
            h.append(p)
        return h

    lower, upper = half(pts), half(pts[::-1])
    return lower[:-1] + upper[:-1]


def signed_distance(poly, x, y):
    """Distance [same units] of the points (x, y) to the boundary of the convex polygon `poly`: negative inside."""
    p = np.asarray(poly, np.float64)
    q = np.roll(p, -1, axis=0)
    best = np.full(x.shape, np.inf)
    inside = np.ones(x.shape, bool)
    for (x0, y0), (x1, y1) in zip(p, q):
        ex, ey = x1 - x0, y1 - y0
        t = np.clip(((x - x0) * ex + (y - y0) * ey) / (ex * ex + ey * ey), 0.0, 1.0)
        best = np.minimum(best, np.hypot(x - (x0 + t * ex), y - (y0 + t * ey)))
        inside &= ex * (y - y0) - ey * (x - x0) >= 0.0
    return np.where(inside, -best, best)


def box_shadow_polygon(r0, r1, c0, c1, height, res, azimuth, elevation):
    """The footprint of the box of cells [r0, r1] x [c0, c1] (centres) swept away from the sun by height / tan(elevation),
    in cell units (x = column, y = row): a convex polygon."""
    reach = height / math.tan(math.radians(elevation)) / res
    dx, dy = -math.sin(math.radians(azimuth)) * reach, math.cos(math.radians(azimuth)) * reach      # away from the sun; rows run south
    corners = [(c0, r0), (c1, r0), (c1, r1), (c0, r1)]
    return _hull([(float(x), float(y)) for x, y in corners] + [(x + dx, y + dy) for x, y in corners])


def box_on_plane(gh, gw, r0, r1, c0, c1, height, base=100.0):
    z = np.full((gh, gw), base, np.float32)
    z[r0:r1 + 1, c0:c1 + 1] += np.float32(height)
    return z


def box_violations(shade, r0, r1, c0, c1, height, res, azimuth, elevation, margin=1.5):
    """(shadowed cells farther than `margin` outside the swept footprint, lit cells farther than `margin` inside it, the size
    of the inside set); the box's own cells belong to neither set."""
    gh, gw = shade.shape
    y, x = np.mgrid[0:gh, 0:gw].astype(np.float64)
    sd = signed_distance(box_shadow_polygon(r0, r1, c0, c1, height, res, azimuth, elevation), x, y)
    ground = np.ones((gh, gw), bool)
    ground[r0:r1 + 1, c0:c1 + 1] = False
    outside, inside = ground & (sd > margin), ground & (sd < -margin)
    return int((outside & (shade == 2)).sum()), int((inside & (shade != 2)).sum()), int(inside.sum())
