"""The rule of the DSM meshes (include/satmvs.h, "Meshes") stated twice in numpy and Python integers.

  recursion   triangle objects after the rule's text: the hierarchy by bisection, every triangle's error by brute force over
              the lattice vertices of its closed area, saturation triangle by triangle, emission by the top-down descent
  arrays      level by level in closed form: the closed squares of side h as blocks, the triangles as masks over a block,
              saturation by slices, emission by the LOCAL rule (apex active, split vertex not), heights by a vectorised walk

Errors count in units of 2^-8 m / S (S the tile): every barycentric weight of a hierarchy triangle has a denominator that
divides S.  Root corners hold 0.  +infinity is INF = 2^63 - 1.  Both statements return the device's arrays: the int64 error map,
and a mesh as a dict of vertices int32 (V, 2) col, row; z float32 (V); triangles int32 (T, 3); tri_level uint8 (T)."""
import numpy as np

from dsm_testkit import scene as kit_scene

INF = int(np.iinfo(np.int64).max)
VARIANTS = ("midpoint", "ge", "nosat", "open", "voids", "side")      # the planted errors of the array statement
XRES, YRES = 2.5, 2.0


# ---- what both statements share: quanta, the cover, the order ------------------------------------------------------------------
def quantum(z, nodata=-999.0):
    """q = rn(256 z) (ties to even) as int64 and the validity: finite, != (float32)nodata, |z| <= 32768."""
    z = np.asarray(z, np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(z) & (z != np.float32(nodata)) & (np.abs(z) <= np.float32(32768.0))
    q = np.rint(np.where(ok, z, np.float32(0)).astype(np.float64) * 256.0).astype(np.int64)
    return q, ok


def log2_tile(S):
    k = int(S).bit_length() - 1
    assert 2 <= S <= 1024 and 1 << k == S, S
    return k


def cover(gh, gw, S):
    """The extent in cells of the root squares that cover the lattice from (0, 0); at least one square each way."""
    return max(1, -(-(gh - 1) // S)) * S, max(1, -(-(gw - 1) // S)) * S


def padded(z, nodata, S):
    """Quanta and validity over the cover's vertices; beyond the grid nothing is valid."""
    gh, gw = z.shape
    ch, cw = cover(gh, gw, S)
    q, ok = quantum(z, nodata)
    Q, V = np.zeros((ch + 1, cw + 1), np.int64), np.zeros((ch + 1, cw + 1), bool)
    Q[:gh, :gw], V[:gh, :gw] = q, ok
    return Q, V


def threshold(tol, S):
    """tol [m] -> (tol_units, threshold in the errors' units)."""
    units = int(np.floor(256.0 * float(tol)))
    return units, units * S


def assemble(rows, z):
    """rows: int array (T, 7) of ar, ac, br, bc, cr, cc, level in any order -> the mesh in the rule's order."""
    z = np.asarray(z, np.float32)
    gh, gw = z.shape
    rows = np.asarray(rows, np.int64).reshape(-1, 7)
    a, b, c, level = rows[:, 0:2], rows[:, 2:4], rows[:, 4:6], rows[:, 6]
    other = a + b - c                                        # the apex of the triangle across the hypotenuse
    side = ((c[:, 0] > other[:, 0]) | ((c[:, 0] == other[:, 0]) & (c[:, 1] > other[:, 1]))).astype(np.int64)
    key = a + b
    order = np.lexsort((side, key[:, 1], key[:, 0]))
    a, b, c, level, side, key = a[order], b[order], c[order], level[order], side[order], key[order]
    # counter-clockwise seen from above, east right and north up: x = col, y = -row
    cross = (b[:, 1] - a[:, 1]) * (a[:, 0] - c[:, 0]) - (a[:, 0] - b[:, 0]) * (c[:, 1] - a[:, 1])
    assert (cross != 0).all()
    swap = cross < 0
    a2, b2 = np.where(swap[:, None], b, a), np.where(swap[:, None], a, b)
    flat = np.concatenate([a2[:, 0] * gw + a2[:, 1], b2[:, 0] * gw + b2[:, 1], c[:, 0] * gw + c[:, 1]])
    used = np.unique(flat)
    tri = np.searchsorted(used, flat).reshape(3, -1).T
    return {"vertices": np.stack([used % gw, used // gw], axis=1).astype(np.int32), "z": z.reshape(-1)[used].copy(),
            "triangles": np.ascontiguousarray(tri, np.int32), "tri_level": level.astype(np.uint8),
            "key": np.stack([key[:, 0], key[:, 1], side], axis=1)}


def corners(mesh):
    """(T, 3, 2) row, col of every triangle's corners."""
    v = mesh["vertices"].astype(np.int64)
    return v[mesh["triangles"].astype(np.int64)][:, :, ::-1]


def differing(got, want, keys=("triangles", "tri_level", "vertices", "z")):
    """[] if the meshes agree in every bit, else what differs, the first differing triangle named by its corners."""
    out = []
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.dtype != w.dtype or g.shape != w.shape:
            out.append("%s: %s %s against %s %s" % (k, g.dtype, g.shape, w.dtype, w.shape))
        elif k == "z" and not np.array_equal(g.view(np.uint32), w.view(np.uint32)):
            out.append("z: %d heights differ in their bits" % int((g.view(np.uint32) != w.view(np.uint32)).sum()))
        elif k != "z" and not np.array_equal(g, w):
            out.append("%s: %d entries differ" % (k, int((g != w).sum())))
    if out:
        cg, cw_ = corners(got), corners(want)
        n = min(len(cg), len(cw_))
        bad = np.nonzero((cg[:n] != cw_[:n]).any(axis=(1, 2)))[0]
        at = int(bad[0]) if len(bad) else n
        name = lambda c, i: "none" if i >= len(c) else "(%s)" % ", ".join("(%d, %d)" % tuple(p) for p in c[i].tolist())      # noqa: E731
        out.insert(0, "first differing triangle %d: got %s, want %s (row, col of a, b, c)" % (at, name(cg, at), name(cw_, at)))
    return out


# ---- the recursion -------------------------------------------------------------------------------------------------------------
class Tri:
    __slots__ = ("a", "b", "c", "level")

    def __init__(self, a, b, c, level):
        self.a, self.b, self.c, self.level = a, b, c, level

    def mid(self):
        return ((self.a[0] + self.b[0]) // 2, (self.a[1] + self.b[1]) // 2)

    def children(self):
        m = self.mid()
        return Tri(self.c, self.a, m, self.level + 1), Tri(self.b, self.c, m, self.level + 1)

    def points(self):
        """The lattice vertices of the closed triangle, by the signs of three cross products."""
        (ar, ac), (br, bc), (cr, cc) = self.a, self.b, self.c
        out = []
        for r in range(min(ar, br, cr), max(ar, br, cr) + 1):
            for c in range(min(ac, bc, cc), max(ac, bc, cc) + 1):
                d = [(x1 - x0) * (c - y0) - (y1 - y0) * (r - x0) for (x0, y0), (x1, y1) in ((self.a, self.b), (self.b, self.c), (self.c, self.a))]
                if all(v >= 0 for v in d) or all(v <= 0 for v in d):
                    out.append((r, c))
        return out

    def plane(self, p, Q):
        """(numerator, denominator) of the plane's height at p in units of 2^-8 m, Python integers."""
        xr, xc, yr, yc = self.a[0] - self.c[0], self.a[1] - self.c[1], self.b[0] - self.c[0], self.b[1] - self.c[1]
        D = xr * xr + xc * xc
        s, t = (p[0] - self.c[0]) * xr + (p[1] - self.c[1]) * xc, (p[0] - self.c[0]) * yr + (p[1] - self.c[1]) * yc
        qa, qb, qc = int(Q[self.a]), int(Q[self.b]), int(Q[self.c])
        return qc * D + (qa - qc) * s + (qb - qc) * t, D


def root_triangles(gh, gw, S):
    ch, cw = cover(gh, gw, S)
    for r0 in range(0, ch, S):
        for c0 in range(0, cw, S):
            yield Tri((r0, c0), (r0 + S, c0 + S), (r0 + S, c0), 0)
            yield Tri((r0 + S, c0 + S), (r0, c0), (r0, c0 + S), 0)


def hierarchy(gh, gw, S):
    """Every triangle of every level, level by level."""
    k = log2_tile(S)
    levels = [list(root_triangles(gh, gw, S))]
    for _ in range(2 * k):
        levels.append([ch for T in levels[-1] for ch in T.children()])
    return levels


def exact_error(T, Q, V, S):
    """E(T) in units of 2^-8 m / S, a Python integer; INF with a void or off-grid vertex in the closed triangle."""
    worst = 0
    for p in T.points():
        if not V[p]:
            return INF
        num, D = T.plane(p, Q)
        dev = abs(int(Q[p]) * D - num) * S
        assert dev % D == 0                                  # the weights' denominators divide S
        worst = max(worst, dev // D)
    return worst


def errors_recursive(z, S, nodata=-999.0):
    z = np.asarray(z, np.float32)
    gh, gw = z.shape
    k = log2_tile(S)
    Q, V = padded(z, nodata, S)
    levels = hierarchy(gh, gw, S)
    e = {}
    for level in range(2 * k):
        for T in levels[level]:
            m = T.mid()
            e[m] = max(e.get(m, 0), exact_error(T, Q, V, S))
    on = lambda p: p[0] < gh and p[1] < gw                   # noqa: E731
    for level in range(2 * k - 1, 0, -1):                    # the root triangles' apexes are corners: always active, they hold 0
        for T in levels[level]:
            m = T.mid()
            e[T.c] = max(e[T.c], e[m] if on(m) else INF)
    out = np.zeros((gh, gw), np.int64)
    for (r, c), v in e.items():
        if r < gh and c < gw:
            out[r, c] = v
    return out


def _active_fn(errors, S, thr):
    gh, gw = errors.shape
    return lambda p: (p[0] % S == 0 and p[1] % S == 0) or p[0] >= gh or p[1] >= gw or int(errors[p]) > thr


def emitted_recursive(errors, z, S, tol, nodata=-999.0):
    """The emitted triangles of the top-down descent from the root triangles."""
    z = np.asarray(z, np.float32)
    gh, gw = z.shape
    k = log2_tile(S)
    _, V = padded(z, nodata, S)
    active = _active_fn(errors, S, threshold(tol, S)[1])
    out, stack = [], list(root_triangles(gh, gw, S))
    while stack:
        T = stack.pop()
        if T.level == 2 * k:
            if V[T.a] and V[T.b] and V[T.c]:
                out.append(T)
        elif active(T.mid()):
            stack.extend(T.children())
        else:
            out.append(T)
    return out


def mesh_recursive(errors, z, S, tol, nodata=-999.0):
    tris = emitted_recursive(errors, z, S, tol, nodata)
    return assemble([[*T.a, *T.b, *T.c, T.level] for T in tris], z)


def heights_recursive(errors, z, S, tol, nodata=-999.0):
    """Every emitted triangle's plane at every lattice vertex of its closed area; the values of a shared vertex are asserted
    equal.  -> heights float32 (nodata where uncovered), dev int64 (S q - S plane; INF where uncovered)."""
    z = np.asarray(z, np.float32)
    gh, gw = z.shape
    Q, _ = padded(z, nodata, S)
    plane = {}
    for T in emitted_recursive(errors, z, S, tol, nodata):
        for p in T.points():
            num, D = T.plane(p, Q)
            assert (num * S) % D == 0
            v = num * S // D
            assert plane.setdefault(p, v) == v, (p, plane[p], v)
    h, dev = np.full((gh, gw), np.float32(nodata), np.float32), np.full((gh, gw), INF, np.int64)
    for (r, c), v in plane.items():
        h[r, c] = np.float32(np.float64(v) / np.float64(S * 256))
        dev[r, c] = int(Q[r, c]) * S - v
    return h, dev


# ---- the arrays ----------------------------------------------------------------------------------------------------------------
def _blocks(A, h):
    """(ch + 1, cw + 1) -> (nR, nC, h + 1, h + 1): the closed squares of side h."""
    nR, nC = (A.shape[0] - 1) // h, (A.shape[1] - 1) // h
    ir = np.arange(nR)[:, None] * h + np.arange(h + 1)[None, :]
    ic = np.arange(nC)[:, None] * h + np.arange(h + 1)[None, :]
    return A[ir[:, None, :, None], ic[None, :, None, :]]


def _block_max(dev, member, VB, scale, variant, centre):
    """max over the member vertices of each block of dev * scale; INF with a void among them."""
    if variant == "midpoint":
        member = member & centre
    worst = np.where(member, dev, 0).max(axis=(2, 3)) * scale
    if variant != "voids":
        worst = np.where((member & ~VB).any(axis=(2, 3)), INF, worst)
    return worst


def errors_arrays(z, S, nodata=-999.0, variant=None):
    z = np.asarray(z, np.float32)
    gh, gw = z.shape
    k = log2_tile(S)
    Q, V = padded(z, nodata, S)
    ch, cw = Q.shape[0] - 1, Q.shape[1] - 1
    e = np.zeros((ch + 1, cw + 1), np.int64)
    strict = variant == "open"
    for j in range(k):
        h = S >> j
        half, scale = h // 2, S // h
        B, VB = _blocks(Q, h), _blocks(V, h)
        nR, nC = B.shape[:2]
        u, v = np.mgrid[0:h + 1, 0:h + 1]
        u, v = u[None, None], v[None, None]
        TL, TR, BL, BR, CN = (B[:, :, i, jj][:, :, None, None] for i, jj in ((0, 0), (0, h), (h, 0), (h, h), (half, half)))
        everyone = np.ones((1, 1, h + 1, h + 1), bool)
        # level 2 j: the two halves of a square share its centre; on the diagonal their planes agree
        main = ((np.arange(nR)[:, None] ^ np.arange(nC)[None, :]) & 1) == 0 if j else np.ones((nR, nC), bool)
        main = main[:, :, None, None]
        lower = h * BL + (TL - BL) * (h - u) + (BR - BL) * v
        upper = h * TR + (TL - TR) * (h - v) + (BR - TR) * u
        first = h * TL + (TR - TL) * v + (BL - TL) * u
        last = h * BR + (BL - BR) * (h - v) + (TR - BR) * (h - u)
        plane = np.where(main, np.where(u >= v, lower, upper), np.where(u + v <= h, first, last))
        member = everyone
        if strict:                                           # planted: the open triangles, without their rims
            member = (u > 0) & (u < h) & (v > 0) & (v < h) & np.where(main, u != v, u + v != h)
        centre = (u == half) & (v == half)
        e[half::h, half::h] = _block_max(np.abs(h * B - plane), np.broadcast_to(member, B.shape), VB, scale, variant, centre)
        # level 2 j + 1: four triangles with their apex at the centre; a side's middle takes the two that meet in that side
        lt = (lambda a, b: a < b) if strict else (lambda a, b: a <= b)
        sides = {}
        for name, qa, qb, x, y, member, mid in (
                ("top", TL, TR, v - half, u, lt(u, v) & lt(u, h - v), (u == 0) & (v == half)),
                ("bottom", BL, BR, v - half, h - u, lt(h - u, v) & lt(h - u, h - v), (u == h) & (v == half)),
                ("left", TL, BL, u - half, v, lt(v, u) & lt(v, h - u), (v == 0) & (u == half)),
                ("right", TR, BR, u - half, h - v, lt(h - v, u) & lt(h - v, h - u), (v == h) & (u == half))):
            if strict:
                member = member & (y > 0)
            plane = (qa + qb) * half + (qb - qa) * x + (2 * CN - qa - qb) * y
            sides[name] = _block_max(np.abs(h * B - plane), np.broadcast_to(member, B.shape), VB, scale, variant, mid)
        H = np.zeros((nR + 1, nC), np.int64)
        H[:nR] = sides["top"]
        H[1:] = np.maximum(H[1:], sides["bottom"])
        W = np.zeros((nR, nC + 1), np.int64)
        W[:, :nC] = sides["left"]
        W[:, 1:] = np.maximum(W[:, 1:], sides["right"])
        e[0::h, half::h], e[half::h, 0::h] = H, W
    if variant != "nosat":
        for lv in range(2 * k - 2, -1, -1):
            h = S >> (lv // 2)
            half, q = h // 2, h // 4
            if lv % 2 == 0:
                own = e[half::h, half::h]
                for other in (e[0:ch:h, half::h], e[h::h, half::h], e[half::h, 0:cw:h], e[half::h, h::h]):
                    own = np.maximum(own, other)
                e[half::h, half::h] = own
            else:
                H = e[0::h, half::h].copy()                  # (nR + 1, nC): the triangles under rows 0 .. nR - 1, over rows 1 .. nR
                for dc in (half - q, half + q):
                    H[:-1] = np.maximum(H[:-1], e[q::h, dc::h])
                    H[1:] = np.maximum(H[1:], e[h - q::h, dc::h])
                W = e[half::h, 0::h].copy()
                for dr in (half - q, half + q):
                    W[:, :-1] = np.maximum(W[:, :-1], e[dr::h, q::h])
                    W[:, 1:] = np.maximum(W[:, 1:], e[dr::h, h - q::h])
                e[0::h, half::h], e[half::h, 0::h] = H, W
    return e[:gh, :gw].copy()


def _active_map(errors, S, thr, variant=None):
    """Over the cover's vertices: root corners and everything off the grid are active."""
    gh, gw = errors.shape
    ch, cw = cover(gh, gw, S)
    act = np.ones((ch + 1, cw + 1), bool)
    act[:gh, :gw] = errors >= thr if variant == "ge" else errors > thr
    act[0::S, 0::S] = True
    return act


def emitted_arrays(errors, z, S, tol, nodata=-999.0, variant=None):
    """The LOCAL rule, level by level -> rows of ar, ac, br, bc, cr, cc, level."""
    z = np.asarray(z, np.float32)
    gh, gw = z.shape
    k = log2_tile(S)
    _, V = padded(z, nodata, S)
    ch, cw = V.shape[0] - 1, V.shape[1] - 1
    act = _active_map(errors, S, threshold(tol, S)[1], variant)
    rows = []

    def take(keep, ar, ac, br, bc, cr, cc, level):
        ar, ac, br, bc, cr, cc, keep = np.broadcast_arrays(ar, ac, br, bc, cr, cc, keep)
        rows.append(np.stack([x[keep] for x in (ar, ac, br, bc, cr, cc)] + [np.full(int(keep.sum()), level)], axis=1))

    for j in range(k):
        h = S >> j
        half = h // 2
        nR, nC = ch // h, cw // h
        R, C = np.mgrid[0:nR, 0:nC]
        r, c = R * h + half, C * h + half                    # the centres: level 2 j
        main = ((R ^ C) & 1) == 0 if j else np.ones((nR, nC), bool)
        quiet = ~act[r, c]
        take(quiet & main & act[r - half, c + half], r - half, c - half, r + half, c + half, r - half, c + half, 2 * j)
        take(quiet & main & act[r + half, c - half], r - half, c - half, r + half, c + half, r + half, c - half, 2 * j)
        take(quiet & ~main & act[r - half, c - half], r - half, c + half, r + half, c - half, r - half, c - half, 2 * j)
        take(quiet & ~main & act[r + half, c + half], r - half, c + half, r + half, c - half, r + half, c + half, 2 * j)
        R, C = np.mgrid[0:nR + 1, 0:nC]                      # the middles of the sides along a row: level 2 j + 1
        r, c = R * h, C * h + half
        quiet = ~act[r, c]
        take(quiet & (r > 0) & act[np.maximum(r - half, 0), c], r, c - half, r, c + half, r - half, c, 2 * j + 1)
        take(quiet & (r < ch) & act[np.minimum(r + half, ch), c], r, c - half, r, c + half, r + half, c, 2 * j + 1)
        R, C = np.mgrid[0:nR, 0:nC + 1]
        r, c = R * h + half, C * h
        quiet = ~act[r, c]
        take(quiet & (c > 0) & act[r, np.maximum(c - half, 0)], r - half, c, r + half, c, r, c - half, 2 * j + 1)
        take(quiet & (c < cw) & act[r, np.minimum(c + half, cw)], r - half, c, r + half, c, r, c + half, 2 * j + 1)
    r, c = np.mgrid[0:ch, 0:cw]                              # the cells: level 2 k
    main = ((r ^ c) & 1) == 0
    whole = lambda a, b, cc_: V[a] & V[b] & V[cc_]           # noqa: E731
    TL, TR, BL, BR = (r, c), (r, c + 1), (r + 1, c), (r + 1, c + 1)
    take(main & act[TR] & whole(TL, BR, TR), *TL, *BR, *TR, 2 * k)
    take(main & act[BL] & whole(TL, BR, BL), *TL, *BR, *BL, 2 * k)
    take(~main & act[TL] & whole(TR, BL, TL), *TR, *BL, *TL, 2 * k)
    take(~main & act[BR] & whole(TR, BL, BR), *TR, *BL, *BR, 2 * k)
    return np.concatenate(rows, axis=0)


def mesh_arrays(errors, z, S, tol, nodata=-999.0, variant=None):
    rows = emitted_arrays(errors, z, S, tol, nodata, variant)
    if variant == "side":                                    # planted: the two triangles of a hypotenuse the other way round
        m = assemble(rows, z)
        key = m["key"].copy()
        key[:, 2] = 1 - key[:, 2]
        order = np.lexsort((key[:, 2], key[:, 1], key[:, 0]))
        m["triangles"], m["tri_level"], m["key"] = m["triangles"][order], m["tri_level"][order], key[order]
        return m
    return assemble(rows, z)


def mesh(z, S, tol, nodata=-999.0, errors=None, variant=None):
    """The array statement end to end (a planted variant changes the errors and the emission alike)."""
    if errors is None:
        errors = errors_arrays(z, S, nodata, variant)
    return mesh_arrays(errors, z, S, tol, nodata, variant)


def heights_arrays(errors, z, S, tol, nodata=-999.0):
    """The walk of every vertex at once: down from the root triangle by the active flags, at most 2 k steps."""
    z = np.asarray(z, np.float32)
    gh, gw = z.shape
    k = log2_tile(S)
    Q, V = padded(z, nodata, S)
    ch, cw = V.shape[0] - 1, V.shape[1] - 1
    act = _active_map(errors, S, threshold(tol, S)[1])
    r, c = np.mgrid[0:gh, 0:gw]
    r0, c0 = np.minimum(r // S * S, ch - S), np.minimum(c // S * S, cw - S)
    low = (r - r0) >= (c - c0)
    ar, ac = np.where(low, r0, r0 + S), np.where(low, c0, c0 + S)
    br, bc = np.where(low, r0 + S, r0), np.where(low, c0 + S, c0)
    cr, cc = np.where(low, r0 + S, r0), np.where(low, c0, c0 + S)
    going = np.ones((gh, gw), bool)
    for _ in range(2 * k):
        mr, mc = (ar + br) // 2, (ac + bc) // 2
        going = going & act[mr, mc]
        lr, lc = mr - cr, mc - cc
        dp, da = lr * (c - cc) - lc * (r - cr), lr * (ac - cc) - lc * (ar - cr)
        first = (dp == 0) | ((dp > 0) == (da > 0))           # the child (c, a, m); else (b, c, m)
        na_r, na_c = np.where(first, cr, br), np.where(first, cc, bc)
        nb_r, nb_c = np.where(first, ar, cr), np.where(first, ac, cc)
        ar, ac, br, bc = (np.where(going, n, o) for n, o in ((na_r, ar), (na_c, ac), (nb_r, br), (nb_c, bc)))
        cr, cc = np.where(going, mr, cr), np.where(going, mc, cc)
    whole = V[ar, ac] & V[br, bc] & V[cr, cc]
    xr, xc, yr, yc = ar - cr, ac - cc, br - cr, bc - cc
    D = xr * xr + xc * xc
    s, t = (r - cr) * xr + (c - cc) * xc, (r - cr) * yr + (c - cc) * yc
    pd = Q[cr, cc] * D + (Q[ar, ac] - Q[cr, cc]) * s + (Q[br, bc] - Q[cr, cc]) * t
    assert ((pd * S) % D == 0).all()
    plane = pd * S // D
    m = mesh_arrays(errors, z, S, tol, nodata)
    used = np.zeros((gh, gw), bool)
    used[m["vertices"][:, 1], m["vertices"][:, 0]] = True
    own = Q[:gh, :gw] * S
    plane = np.where(whole, plane, own)
    covered = V[:gh, :gw] & (whole | (going & used))         # still going after 2 k steps: a finest triangle with a void corner
    h = np.where(covered, (plane.astype(np.float64) / np.float64(S * 256)).astype(np.float32), np.float32(nodata)).astype(np.float32)
    return h, np.where(covered, own - plane, INF).astype(np.int64)


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def grid_en(gh, gw):
    rows, cols = np.mgrid[0:gh, 0:gw]
    return 400000.0 + XRES * cols, 3500000.0 - YRES * rows


def scene(gh, gw, seed, voids=0.0, salt=0.02):
    E, N = grid_en(gh, gw)
    return kit_scene(E, N, seed=seed, voids=voids, salt=salt)


def quantised_plane(gh, gw, a=3, b=-5, q0=1000):
    """Heights whose quanta are q0 + a row + b col: exactly planar after quantisation."""
    r, c = np.mgrid[0:gh, 0:gw]
    return ((q0 + a * r + b * c) / 256.0).astype(np.float32)


def noise(gh, gw, seed, lo=0, hi=20000):
    """Quanta drawn at random: no three of them in a line worth a tolerance of 0."""
    return (np.random.default_rng(seed).integers(lo, hi, (gh, gw)) / 256.0).astype(np.float32)


def full_resolution_count(z, nodata=-999.0):
    """The finest half-cells with three valid corners (the diagonals run through the centres of the 2 x 2 squares)."""
    _, ok = quantum(z, nodata)
    gh, gw = ok.shape
    if gh < 2 or gw < 2:
        return 0
    r, c = np.mgrid[0:gh - 1, 0:gw - 1]
    main = ((r ^ c) & 1) == 0
    TL, TR, BL, BR = ok[:-1, :-1], ok[:-1, 1:], ok[1:, :-1], ok[1:, 1:]
    return int(np.where(main, (TL & BR & TR).astype(int) + (TL & BR & BL), (TR & BL & TL).astype(int) + (TR & BL & BR)).sum())


SMALL_GRIDS = [(1, 1), (1, 70), (67, 1), (2, 2), (67, 3)]
ROOT_SIDES = [(S, n) for S in (4, 16, 64) for n in (S, S + 1, S + 2)]
TILES = (2, 4, 64, 256, 1024)
TOLS = (0.0, 1.0 / 256.0, 0.5, 2.0, 1e9)
SCENES = [(gh, gw, voids) for gh, gw in ((128, 160), (257, 301)) for voids in (0.0, 0.05, 0.3)]
