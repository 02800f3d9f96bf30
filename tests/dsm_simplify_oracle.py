"""Test-local oracle of the simplified outlines (include/satmvs.h, "Simplified outlines" and smvs_dsm_burn_polygons; DESIGN.md
section 9).  The Douglas-Peucker rule on closed rings is stated twice: recursively with an explicit stack and
fractions.Fraction distances to the segment compared with tol16 / 16 (simplify), and round by round with the integer keys
(simplify_rounds), which also counts the rounds.  Plus the even-odd fill for edges of any direction with Fraction crossings
(fill), the comparison that names the first ring that differs, the closed-form scenes, and the planted errors a comparison
must report.  Nothing here imports satmvs_amd.

A ring of m vertices v_0 .. v_(m-1) is the open chain v_0 .. v_m with v_m = v_0."""
from fractions import Fraction

import numpy as np

KEYS = ("label", "first_ring", "offset", "vertices", "area2", "kept", "simplified")
PLANTED = ("line", "ge", "first_index", "anchor_high", "no_fallback")
PLANTED_FILL = ("rint",)


# ---- pieces ---------------------------------------------------------------------------------------------------------------------
def ring_lists(rings):
    """[[(x, y) ...] per ring], python ints."""
    V = np.asarray(rings["vertices"]).reshape(-1, 2).tolist()
    off = np.asarray(rings["offset"]).tolist()
    return [[tuple(p) for p in V[off[r]:off[r + 1]]] for r in range(len(off) - 1)]


def shoelace2(ring):
    """Twice the area of a ring [(x, y)], integers, north up as dsm.outlines has it: the sum of x1 y0 - x0 y1."""
    return sum(x1 * y0 - x0 * y1 for (x0, y0), (x1, y1) in zip(ring, ring[1:] + ring[:1]))


def dist2(p, a, b, plant=None):
    """The squared distance of p to the segment (a, b) as a Fraction (to the line with plant == "line")."""
    dx, dy, ux, uy = b[0] - a[0], b[1] - a[1], p[0] - a[0], p[1] - a[1]
    L = dx * dx + dy * dy
    if L == 0:
        return Fraction(ux * ux + uy * uy)
    t = Fraction(ux * dx + uy * dy, L)
    if plant != "line":
        t = min(max(t, Fraction(0)), Fraction(1))
    cx, cy = ux - t * dx, uy - t * dy
    return cx * cx + cy * cy


def anchor(ring, plant=None):
    """The index of the vertex farthest from vertex 0, ties to the lowest; 0 if all vertices are equal."""
    d = [(x - ring[0][0]) ** 2 + (y - ring[0][1]) ** 2 for x, y in ring]
    top = max(d)
    if top == 0:
        return 0
    hits = [j for j, v in enumerate(d) if v == top]
    return hits[-1] if plant == "anchor_high" else hits[0]


def _fallback(ring, kept, plant=None):
    """(kept, simplified): all vertices back if fewer than 3 are kept, the area is 0 or its sign has turned."""
    before, after = shoelace2(ring), shoelace2([ring[i] for i in kept])
    ok = len(kept) >= 3 and after != 0 and before != 0 and (after > 0) == (before > 0)
    if ok or plant == "no_fallback":
        return kept, 1 if ok else 0
    return list(range(len(ring))), 0


# ---- statement one: the recursion, Fractions ------------------------------------------------------------------------------------
def simplify_ring(ring, tol16, plant=None):
    """-> the sorted indices kept of one ring, before the fall-back."""
    m = len(ring)
    far = anchor(ring, plant) if m >= 3 else 0
    if far == 0:
        return list(range(m))
    chain = ring + ring[:1]
    tol2 = Fraction(tol16 * tol16, 256)
    kept = {0, far}
    stack = [(0, far), (far, m)]
    while stack:
        a, b = stack.pop()
        if b - a < 2:
            continue
        best = None
        for i in range(a + 1, b):
            d = dist2(chain[i], chain[a], chain[b], plant)
            order = (-d, abs(2 * i - a - b), i) if plant != "first_index" else (-d, i)
            if best is None or order < best[0]:
                best = (order, i, d)
        _, i, d = best
        if d > tol2 or (plant == "ge" and d >= tol2):
            kept.add(i)
            stack.append((a, i))
            stack.append((i, b))
    return sorted(kept)


# ---- statement two: rounds, integer keys ------------------------------------------------------------------------------------------
def int_keys(chain, a, b):
    """The integer keys of the vertices strictly between a and b (a list), and L."""
    (xa, ya), (xb, yb) = chain[a], chain[b]
    dx, dy = xb - xa, yb - ya
    L = dx * dx + dy * dy
    if b - a > 48:                                           # long segments in numpy: every key is below 2^62
        P = np.array(chain[a + 1:b], np.int64)
        ux, uy = P[:, 0] - xa, P[:, 1] - ya
        uu, t = ux * ux + uy * uy, ux * dx + uy * dy
        if L == 0:
            return uu.tolist(), L
        wx, wy = P[:, 0] - xb, P[:, 1] - yb
        cross = dx * uy - dy * ux
        return np.where(t <= 0, uu * L, np.where(t >= L, (wx * wx + wy * wy) * L, cross * cross)).tolist(), L
    out = []
    for x, y in chain[a + 1:b]:
        ux, uy = x - xa, y - ya
        t = ux * dx + uy * dy
        if L == 0:
            out.append(ux * ux + uy * uy)
        elif t <= 0:
            out.append((ux * ux + uy * uy) * L)
        elif t >= L:
            out.append(((x - xb) ** 2 + (y - yb) ** 2) * L)
        else:
            out.append((dx * uy - dy * ux) ** 2)
    return out, L


def simplify_ring_rounds(ring, tol16, sizes=None):
    """-> (the sorted indices kept of one ring before the fall-back, the number of rounds in which a segment of it split).
    sizes: a list that gets the number of interior vertices of every segment treated."""
    m = len(ring)
    far = anchor(ring) if m >= 3 else 0
    if far == 0:
        return list(range(m)), 0
    chain = ring + ring[:1]
    kept = [0, far]
    live = [(0, far), (far, m)]
    rounds = 0
    while live:
        nxt = []
        for a, b in live:
            if b - a < 2:
                continue
            keys, L = int_keys(chain, a, b)
            if sizes is not None:
                sizes.append(b - a - 1)
            top = max(keys)
            bound = (tol16 * tol16 * L if L else tol16 * tol16) >> 8
            if top <= bound:
                continue
            i = min((abs(2 * (a + 1 + j) - a - b), a + 1 + j) for j, k in enumerate(keys) if k == top)[1]
            kept.append(i)
            nxt += [(a, i), (i, b)]
        if nxt:
            rounds += 1
        live = nxt
    return sorted(kept), rounds


# ---- the table ------------------------------------------------------------------------------------------------------------------
def _table(rings, lists, per_ring, rounds):
    """per_ring: [(kept indices, simplified)] -> the dict of dsm.simplify_outlines without a grid."""
    off = np.asarray(rings["offset"]).tolist()
    verts, kept_all, sizes, area2, simplified = [], [], [], [], []
    for r, (ring, (kept, simp)) in enumerate(zip(lists, per_ring)):
        chosen = [ring[i] for i in kept]
        verts += chosen
        kept_all += [off[r] + i for i in kept]
        sizes.append(len(kept))
        area2.append(shoelace2(chosen) if chosen else 0)
        simplified.append(simp)
    return {"label": np.asarray(rings["label"], np.int32).copy(), "first_ring": np.asarray(rings["first_ring"], np.int32).copy(),
            "offset": np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), "vertices": np.array(verts, np.int32).reshape(-1, 2),
            "area2": np.array(area2, np.int64).reshape(-1), "kept": np.array(kept_all, np.int32).reshape(-1),
            "simplified": np.array(simplified, np.uint8).reshape(-1), "rounds": rounds}


def simplify(rings, tol16, plant=None):
    """Statement one over a ring table.  `rounds` is not part of it (None)."""
    lists = ring_lists(rings)
    return _table(rings, lists, [_fallback(ring, simplify_ring(ring, tol16, plant), plant) for ring in lists], None)


def simplify_rounds(rings, tol16):
    """Statement two over a ring table; rounds = the rounds up to and with the first in which no segment of any ring split
    (one more than the deepest ring's splitting rounds), 0 without vertices."""
    lists = ring_lists(rings)
    done = [simplify_ring_rounds(ring, tol16) for ring in lists]
    rounds = 1 + max([k for _, k in done] + [0]) if sum(len(ring) for ring in lists) else 0
    return _table(rings, lists, [_fallback(ring, kept) for ring, (kept, _) in zip(lists, done)], rounds)


def with_grid(out, grid):
    """The entries dsm.simplify_outlines adds with a grid; perimeter_m added edge after edge in vertex order."""
    out = dict(out)
    v = out["vertices"].astype(np.float64)
    xres, yres = float(grid.xres), float(grid.yres)
    out["vertices_en"] = np.stack([float(grid.e0) + (v[:, 0] - 0.5) * xres, float(grid.n0) - (v[:, 1] - 0.5) * yres], 1).reshape(-1, 2)
    per = []
    for r in range(len(out["label"])):
        p = v[out["offset"][r]:out["offset"][r + 1]]
        d = np.roll(p, -1, axis=0) - p
        total = 0.0
        for length in np.sqrt((d[:, 0] * xres) ** 2 + (d[:, 1] * yres) ** 2).tolist():
            total += length
        per.append(total)
    out["perimeter_m"] = np.array(per, np.float64).reshape(-1)
    n = len(out["first_ring"]) - 1
    out["n_holes"] = np.bincount(out["label"][out["area2"] < 0].astype(np.int64) - 1, minlength=n).astype(np.int32)[:n]
    return out


def difference(got, want, skip=()):
    """None if the two tables are equal in every entry of `want` (dtype, shape, values; perimeter_m and rounds are the
    caller's); else a sentence that names the first ring that differs and in what."""
    keys = [k for k in want if k not in ("rounds", "perimeter_m") + tuple(skip)]
    for key in keys:
        if key not in got:
            return "entry %r is missing" % key
        g, w = np.asarray(got[key]), np.asarray(want[key])
        if g.dtype != w.dtype:
            return "entry %r has dtype %s, not %s" % (key, g.dtype, w.dtype)
    if "edges" in got:
        return "an entry 'edges'"
    nr = len(want["label"])
    if len(got["offset"]) == nr + 1 and len(got["area2"]) == nr and len(got["simplified"]) == nr:
        for r in range(nr):
            g0, g1, w0, w1 = got["offset"][r], got["offset"][r + 1], want["offset"][r], want["offset"][r + 1]
            gv, wv = got["vertices"][g0:g1], want["vertices"][w0:w1]
            if got["simplified"][r] != want["simplified"][r]:
                return "ring %d: simplified %d, not %d" % (r, got["simplified"][r], want["simplified"][r])
            if not np.array_equal(gv, wv):
                return "ring %d: %d vertices %s ..., not %d %s ..." % (r, len(gv), gv[:6].tolist(), len(wv), wv[:6].tolist())
            if got["area2"][r] != want["area2"][r]:
                return "ring %d: area2 %d, not %d" % (r, got["area2"][r], want["area2"][r])
            if not np.array_equal(got["kept"][g0:g1], want["kept"][w0:w1]):
                return "ring %d: kept %s ..., not %s ..." % (r, got["kept"][g0:g1][:6].tolist(), want["kept"][w0:w1][:6].tolist())
    for key in keys:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        if g.shape != w.shape or not np.array_equal(g, w, equal_nan=g.dtype.kind == "f"):
            return "entry %r differs" % key
    return None


def same(got, want, what="", skip=()):
    message = difference(got, want, skip)
    assert message is None, (what, message)


def hausdorff_holds(rings, out, tol16):
    """Every vertex of every input ring within tol16 / 16 of the segment between its kept neighbours, exactly."""
    lists = ring_lists(rings)
    tol2 = Fraction(tol16 * tol16, 256)
    off = np.asarray(rings["offset"]).tolist()
    for r, ring in enumerate(lists):
        kept = (np.asarray(out["kept"][out["offset"][r]:out["offset"][r + 1]]) - off[r]).tolist()
        chain = ring + ring[:1]
        for a, b in zip(kept, kept[1:] + [len(ring)]):
            if any(dist2(chain[i], chain[a], chain[b]) > tol2 for i in range(a + 1, b)):
                return False
    return True


# ---- the fill -------------------------------------------------------------------------------------------------------------------
def fill(vertices, offset, ring_label, shape, plant=None):
    """The even-odd fill of smvs_dsm_burn_polygons: per edge and row the crossing of the row's centre line as a Fraction, the
    first column whose centre lies strictly right of it toggled, then the running XOR of every row."""
    gh, gw = shape
    T = np.zeros((gh, gw), np.int32)
    V = np.asarray(vertices).reshape(-1, 2).tolist()
    off = np.asarray(offset).tolist()
    for r in range(len(ring_label)):
        ring = V[off[r]:off[r + 1]]
        for (x0, y0), (x1, y1) in zip(ring, ring[1:] + ring[:1]):
            if y0 == y1:
                continue
            for row in range(max(min(y0, y1), 0), min(max(y0, y1), gh)):
                xc = x0 + Fraction((x1 - x0) * (2 * row + 1 - 2 * y0), 2 * (y1 - y0))
                c = int(round(float(xc))) if plant == "rint" else (xc + Fraction(1, 2)).__floor__()
                if c < gw:
                    T[row, max(c, 0)] ^= np.int32(ring_label[r])
    return np.bitwise_xor.accumulate(T, axis=1).astype(np.int32)


# ---- closed forms ---------------------------------------------------------------------------------------------------------------
def table(n, *rings):
    """rings: (label, [(x, y) ...]) in table order -> a ring table as dsm.outlines gives it (label, first_ring, offset, vertices)."""
    label = np.array([k for k, _ in rings], np.int32).reshape(-1)
    return {"label": label, "first_ring": np.searchsorted(label, np.arange(1, n + 2), side="left").astype(np.int32),
            "offset": np.concatenate([[0], np.cumsum([len(v) for _, v in rings])]).astype(np.int32),
            "vertices": np.array([p for _, v in rings for p in v], np.int32).reshape(-1, 2)}


def rectangle(w, h, x=0, y=0):
    return [(x, y), (x, y + h), (x + w, y + h), (x + w, y)]


def rectangle_threshold16(w, h):
    """The smallest tol16 at which the w x h rectangle falls back: the far anchor is the opposite corner, the two other
    corners stand w h / sqrt(w^2 + h^2) from the diagonal, and they are dropped iff that is <= tol16 / 16."""
    t = 0
    while Fraction(t * t, 256) < Fraction(w * w * h * h, w * w + h * h):
        t += 1
    return t


def staircase(g):
    """The ring of the digitised triangle x + y < g (g >= 1) as dsm.outlines gives it: (0, 0), down the left side to (0, g), the
    staircase (k, g - k + 1), (k, g - k) for k = 1 .. g up to (g, 0), and back along the top side: 2 g + 2 vertices."""
    return [(0, 0), (0, g)] + [p for k in range(1, g + 1) for p in ((k, g - k + 1), (k, g - k))]


def triangle_mask(g):
    r, c = np.mgrid[0:g, 0:g]
    return (r + c < g).astype(np.int32)


def notch(w, h, at):
    """A w x h rectangle with a one-cell notch in its top side at column `at` (1 <= at < w - 1), as a ring from (0, 0)."""
    return [(0, 0), (0, h), (w, h), (w, 0), (at + 1, 0), (at + 1, 1), (at, 1), (at, 0)]


TOUCHING = [(0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (2, 1), (1, 1), (1, 0)]    # two cells that meet at a corner, connectivity 8
