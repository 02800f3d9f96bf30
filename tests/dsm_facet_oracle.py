"""The numpy statement of the facet rule (include/satmvs.h, "Facets"): heights in units of 2^-8 m, the 3 x 3 integer gradient and
the planar flag, the labelling stated twice (a loop over cell pairs with a dictionary union-find; arrays and
scipy.sparse.csgraph.connected_components where scipy is installed), the growth as a loop over k, the moments with Python
integers, the plane in the header's operation order with Python floats, and `differing`, which names the first differing cell.
`variant` plants one error in the rule (VARIANTS); the tests show that `differing` reports each of them."""
import numpy as np

ND = np.float32(-999.0)
D8_DC = (1, 1, 0, -1, -1, -1, 0, 1)                          # E, SE, S, SW, W, NW, N, NE: columns east, rows south
D8_DR = (0, 1, 1, 1, 0, -1, -1, -1)
VARIANTS = ("lt", "asym", "last_k", "two_rounds", "half_away", "north")
MAX_TERM = 2 ** 26

try:
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    HAVE_SCIPY = True
except ImportError:                                          # the loop statement stands alone
    HAVE_SCIPY = False


def terms(xres, yres, tol=0.25, slope_tol=0.1):
    """(T, Ax, Ay) = floor(256 tol), floor(2048 slope_tol xres), floor(2048 slope_tol yres), in float64."""
    import math
    return int(math.floor(256.0 * tol)), int(math.floor(2048.0 * slope_tol * xres)), int(math.floor(2048.0 * slope_tol * yres))


def quantise(z, nodata=ND, mask=None, variant=None):
    """(q int64, valid bool): q = rn(256 z), halves to even, of the cells that are finite, != nodata, |z| <= 32768 and inside the mask."""
    z = np.asarray(z, np.float32)
    ok = np.isfinite(z) & (z != np.float32(nodata))
    ok &= np.abs(np.where(ok, z, 0)) <= np.float32(32768.0)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    x = np.where(ok, z, 0).astype(np.float64) * 256.0
    q = np.sign(x) * np.floor(np.abs(x) + 0.5) if variant == "half_away" else np.rint(x)
    return q.astype(np.int64), ok


def shifted(a, dr, dc, fill=0):
    """b[r, c] = a[r + dr, c + dc], `fill` beyond the grid."""
    gh, gw = a.shape
    b = np.full_like(a, fill)
    r0, r1, c0, c1 = max(0, -dr), min(gh, gh - dr), max(0, -dc), min(gw, gw - dc)
    if r0 < r1 and c0 < c1:
        b[r0:r1, c0:c1] = a[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
    return b


def local_planes(q, ok, T, variant=None):
    """(Gx, Gy int64, planar bool): zeros and False where a cell of the 3 x 3 window is off the grid or invalid."""
    whole = np.ones_like(ok)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            whole &= shifted(ok, dr, dc, False)
    n = {(dr, dc): shifted(q, dr, dc) for dr in (-1, 0, 1) for dc in (-1, 0, 1)}
    Gx = (n[-1, 1] + 2 * n[0, 1] + n[1, 1]) - (n[-1, -1] + 2 * n[0, -1] + n[1, -1])
    Gy = (n[1, -1] + 2 * n[1, 0] + n[1, 1]) - (n[-1, -1] + 2 * n[-1, 0] + n[-1, 1])
    if variant == "north":
        Gy = -Gy
    planar = whole.copy()
    for (dr, dc), qk in n.items():
        if (dr, dc) != (0, 0):
            planar &= np.abs(8 * (qk - q) - (Gx * dc + Gy * dr)) <= 8 * T
    return np.where(whole, Gx, 0), np.where(whole, Gy, 0), planar


def pair_offsets(connectivity):
    """Half of the neighbourhood, (dr, dc): every unordered pair of neighbours once."""
    return [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])


def link_scalar(qp, gxp, gyp, qn, gxn, gyn, dx, dy, T, Ax, Ay, variant=None):
    step = 16 * (qn - qp) - ((gxp + gxn) * dx + (gyp + gyn) * dy)
    if variant == "asym":
        step = 16 * (qn - qp) - 2 * (gxp * dx + gyp * dy)
    if variant == "lt":
        return abs(gxp - gxn) < Ax and abs(gyp - gyn) < Ay and abs(step) < 16 * T
    return abs(gxp - gxn) <= Ax and abs(gyp - gyn) <= Ay and abs(step) <= 16 * T


def numbered(root_of, planar):
    """labels int32 from a root (any representative id) per planar cell: 1 .. n in raster order of every class's first cell."""
    labels = np.zeros(planar.shape, np.int32)
    cells = np.flatnonzero(planar.ravel())
    if len(cells) == 0:
        return labels, 0
    ids = np.asarray(root_of)
    _, first, inverse = np.unique(ids, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                 # classes by their first cell
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    labels.ravel()[cells] = (rank[inverse.ravel()] + 1).astype(np.int32)
    return labels, int(len(order))


def label_loop(q, Gx, Gy, planar, T, Ax, Ay, connectivity, variant=None):
    """Statement one: every pair of neighbouring planar cells, a dictionary union-find."""
    gh, gw = planar.shape
    parent = {}

    def find(a):
        while parent.get(a, a) != a:
            a = parent[a]
        return a
    ql, gxl, gyl, pl = q.tolist(), Gx.tolist(), Gy.tolist(), planar.tolist()
    for r in range(gh):
        for c in range(gw):
            if not pl[r][c]:
                continue
            for dr, dc in pair_offsets(connectivity):
                rr, cc = r + dr, c + dc
                if not (0 <= rr < gh and 0 <= cc < gw and pl[rr][cc]):
                    continue
                if link_scalar(ql[r][c], gxl[r][c], gyl[r][c], ql[rr][cc], gxl[rr][cc], gyl[rr][cc], dc, dr, T, Ax, Ay, variant):
                    a, b = find(r * gw + c), find(rr * gw + cc)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
    cells = np.flatnonzero(planar.ravel())
    return numbered([find(int(i)) for i in cells], planar)


def link_arrays(q, Gx, Gy, planar, T, Ax, Ay, dr, dc, variant=None):
    """Whether cell p = (r, c) and n = (r + dr, c + dc) are linked, as an array over p."""
    qn, gxn, gyn = shifted(q, dr, dc), shifted(Gx, dr, dc), shifted(Gy, dr, dc)
    both = planar & shifted(planar, dr, dc, False)
    step = 16 * (qn - q) - ((Gx + gxn) * dc + (Gy + gyn) * dr)
    if variant == "asym":
        step = 16 * (qn - q) - 2 * (Gx * dc + Gy * dr)
    if variant == "lt":
        return both & (np.abs(Gx - gxn) < Ax) & (np.abs(Gy - gyn) < Ay) & (np.abs(step) < 16 * T)
    return both & (np.abs(Gx - gxn) <= Ax) & (np.abs(Gy - gyn) <= Ay) & (np.abs(step) <= 16 * T)


def label_graph(q, Gx, Gy, planar, T, Ax, Ay, connectivity, variant=None):
    """Statement two: the links as a sparse graph, its connected components (scipy's, or a propagation in numpy without it)."""
    gh, gw = planar.shape
    src, dst = [], []
    for dr, dc in pair_offsets(connectivity):
        p = np.flatnonzero(link_arrays(q, Gx, Gy, planar, T, Ax, Ay, dr, dc, variant).ravel())
        src.append(p)
        dst.append(p + dr * gw + dc)
    src, dst = np.concatenate(src), np.concatenate(dst)
    if not HAVE_SCIPY:                                       # without scipy: the lowest cell index spread along the links to a fixed point
        low = np.arange(gh * gw)
        while True:
            nxt = low.copy()
            np.minimum.at(nxt, src, low[dst])
            np.minimum.at(nxt, dst, low[src])
            nxt = np.minimum(nxt, nxt[nxt])                   # and a jump: the lowest index its lowest index knows
            if np.array_equal(nxt, low):
                return numbered(low[np.flatnonzero(planar.ravel())], planar)
            low = nxt
    graph = coo_matrix((np.ones(len(src), np.int8), (src, dst)), shape=(gh * gw, gh * gw))
    _, comp = connected_components(graph, directed=False)
    return numbered(comp[np.flatnonzero(planar.ravel())], planar)


def grown(labels, q, ok, Gx, Gy, planar, T, variant=None):
    """One round of growth, a loop over k = 0 .. 7: the first planar neighbour whose plane passes within T."""
    out = labels.copy()
    todo = ok & ~planar
    done = np.zeros_like(todo)
    for k in range(8):
        dr, dc = D8_DR[k], D8_DC[k]
        qp, gxp, gyp = shifted(q, dr, dc), shifted(Gx, dr, dc), shifted(Gy, dr, dc)
        fits = todo & shifted(planar, dr, dc, False) & (np.abs(8 * (q - qp) - (gxp * -dc + gyp * -dr)) <= 8 * T)
        if variant != "last_k":
            fits &= ~done
        out[fits] = shifted(labels, dr, dc)[fits]
        done |= fits
    if variant == "two_rounds":                              # a second round from the grown cells, by height alone
        for k in range(8):
            dr, dc = D8_DR[k], D8_DC[k]
            more = todo & ~done & (out == 0) & shifted(done, dr, dc, False) & (np.abs(q - shifted(q, dr, dc)) <= T)
            out[more] = shifted(out, dr, dc)[more]
    return out


def facets(z, T, Ax, Ay, connectivity=8, grow=True, mask=None, nodata=ND, statement=None, variant=None):
    """-> (labels (gh, gw) int32, n): the whole rule.  statement "loop" or "graph" (the default)."""
    q, ok = quantise(z, nodata, mask, variant)
    Gx, Gy, planar = local_planes(q, ok, T, variant)
    if statement is None:
        statement = "graph"
    labels, n = (label_graph if statement == "graph" else label_loop)(q, Gx, Gy, planar, T, Ax, Ay, connectivity, variant)
    if grow:
        labels = grown(labels, q, ok, Gx, Gy, planar, T, variant)
    return labels, n


def normals(z, T, mask=None, nodata=ND):
    """What smvs_dsm_facet_normals writes: Gx, Gy int32, planar uint8."""
    q, ok = quantise(z, nodata, mask)
    Gx, Gy, planar = local_planes(q, ok, T)
    return Gx.astype(np.int32), Gy.astype(np.int32), planar.astype(np.uint8)


def floor_div(a, b):
    return a // b                                            # Python integers: floor


def fit(N, m, qb):
    """a, b, h0 from n, the eight centred sums and the centre's height, Python floats in the header's order."""
    if N == 0:
        return (float("nan"),) * 3
    Nf = float(N)
    Sx, Sy, Sz, Sxx, Sxy, Syy, Sxz, Syz = (float(v) for v in m)
    cxx, cxy, cyy = Sxx - (Sx * Sx) / Nf, Sxy - (Sx * Sy) / Nf, Syy - (Sy * Sy) / Nf
    cxz, cyz = Sxz - (Sx * Sz) / Nf, Syz - (Sy * Sz) / Nf
    det = cxx * cyy - cxy * cxy
    if not det > 0.0:
        return (float("nan"),) * 3
    a = (cxz * cyy - cyz * cxy) / det
    b = (cyz * cxx - cxz * cxy) / det
    return a, b, float(qb) + ((Sz / Nf - a * (Sx / Nf)) - b * (Sy / Nf))


def planes(labels, n, z, nodata=ND):
    """What smvs_dsm_facet_planes writes: sums (n, 4), centre (n, 3), moments (n, 8), plane (n, 3), sse (n), max_abs (n)."""
    q, ok = quantise(z, nodata)
    lab = np.asarray(labels).astype(np.int64)
    counted = ok & (lab >= 1) & (lab <= n)
    cells = np.flatnonzero(counted.ravel())
    cells = cells[np.argsort(lab.ravel()[cells], kind="stable")]
    cuts = np.searchsorted(lab.ravel()[cells], np.arange(1, n + 2))
    gw = lab.shape[1]
    out = {"sums": np.zeros((n, 4), np.int64), "centre": np.zeros((n, 3), np.int32), "moments": np.zeros((n, 8), np.int64),
           "plane": np.full((n, 3), np.nan), "sse": np.zeros(n, np.int64), "max_abs": np.zeros(n, np.int32)}
    for k in range(n):
        mine = cells[cuts[k]:cuts[k + 1]]
        cs, rs, qs = (mine % gw).tolist(), (mine // gw).tolist(), q.ravel()[mine].tolist()
        N = len(cs)
        out["sums"][k] = [N, sum(cs), sum(rs), sum(qs)]
        if N == 0:
            continue
        cb, rb, qb = floor_div(sum(cs), N), floor_div(sum(rs), N), floor_div(sum(qs), N)
        out["centre"][k] = [cb, rb, qb]
        dc, dr, dq = [c - cb for c in cs], [r - rb for r in rs], [v - qb for v in qs]
        m = [sum(dc), sum(dr), sum(dq), sum(x * x for x in dc), sum(x * y for x, y in zip(dc, dr)), sum(y * y for y in dr),
             sum(x * v for x, v in zip(dc, dq)), sum(y * v for y, v in zip(dr, dq))]
        assert all(abs(v) < 2 ** 63 for v in m)
        out["moments"][k] = m
        a, b, h0 = fit(N, m, qb)
        out["plane"][k] = [a, b, h0]
        if h0 == h0:
            at = (h0 + a * np.asarray(dc, np.float64)) + b * np.asarray(dr, np.float64)
            e = np.clip(np.asarray(qs, np.int64) - np.rint(np.clip(at, -2.0 ** 40, 2.0 ** 40)).astype(np.int64), -65536, 65536).tolist()
            out["sse"][k] = sum(v * v for v in e)
            out["max_abs"][k] = max(abs(v) for v in e)
    return out


def differing(got, want):
    """None if two arrays agree in shape, dtype and every element (floats by their bits); else a sentence that names the first
    differing cell."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return "shape / dtype %s %s against %s %s" % (got.shape, got.dtype, want.shape, want.dtype)
    g, w = got, want
    if got.dtype.kind == "f":
        bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        g, w = np.ascontiguousarray(got).view(bits), np.ascontiguousarray(want).view(bits)
    bad = np.argwhere(g != w)
    if len(bad) == 0:
        return None
    at = tuple(int(i) for i in bad[0])
    return "%d of %d differ, the first at %s: got %r, want %r" % (len(bad), got.size, at, got[at].item(), want[at].item())


def same_planes(got, want, what):
    for key, w in want.items():
        d = differing(np.asarray(got[key]).reshape(w.shape), w)
        assert d is None, (what, key, d)
