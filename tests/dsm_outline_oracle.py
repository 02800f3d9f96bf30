"""Test-local numpy oracle of the outlines (include/satmvs.h smvs_dsm_outline_count / _write / smvs_dsm_burn, DESIGN.md section
9, "Outlines"), stated twice: as the walk over (cell, side) edges with the right-first successor (trace), and by corners alone
(trace_corners): the boundary edges of every label as a multiset of corner pairs, linked through a dictionary from tail corner
to the edges that leave it, with the right turn taken where two leave.  Plus the even-odd fill, the GeoJSON reader-back, the
comparison that names the first differing ring, and the closed-form scenes.  Nothing here imports satmvs_amd.

Corner (x, y) is the upper-left corner of cell (row y, col x).  Sides: 0 south, 1 east, 2 north, 3 west; an edge has its own
cell on the left, north up: south side heading east, east side north, north side west, west side south."""
import json

import numpy as np

HEAD = ((1, 0), (0, -1), (-1, 0), (0, 1))                    # (dx, dy) of the heading of side s; across side s lies HEAD[(s + 3) % 4]
TAIL = ((0, 1), (1, 1), (1, 0), (0, 0))                      # the tail corner of side s of cell (0, 0), (x, y)
KEYS = ("label", "area2", "edges", "offset", "first_ring", "vertices")
PLANTED = ("left_first", "reversed", "start_edge", "collinear", "edge_order")


def clean(labels, n):
    """The label map with every value outside 1 .. n zeroed."""
    L = np.asarray(labels)
    return np.where((L >= 1) & (L <= n), L, 0).astype(np.int32)


def _table(rings, n):
    """rings: a list of (label, vertices [(x, y)], area2, ew, ns, order key) -> the dict of dsm.outlines, sorted by the keys."""
    rings = sorted(rings, key=lambda r: r[5])
    out = {"label": np.array([r[0] for r in rings], np.int32).reshape(-1),
           "area2": np.array([r[2] for r in rings], np.int64).reshape(-1),
           "edges": np.array([[r[3], r[4]] for r in rings], np.int32).reshape(-1, 2),
           "offset": np.concatenate([[0], np.cumsum([len(r[1]) for r in rings])]).astype(np.int32),
           "vertices": np.array([v for r in rings for v in r[1]], np.int32).reshape(-1, 2)}
    out["first_ring"] = np.searchsorted(out["label"], np.arange(1, n + 2), side="left").astype(np.int32)
    return out


def trace(labels, n, plant=None):
    """Statement one: the walk.  plant: None, or one of PLANTED, a wrong rule a comparison must report."""
    L = clean(labels, n)
    gh, gw = L.shape
    P = np.zeros((gh + 2, gw + 2), np.int32)
    P[1:-1, 1:-1] = L
    inner = P[1:-1, 1:-1]

    def shifted(dx, dy):
        return P[1 + dy:1 + dy + gh, 1 + dx:1 + dx + gw]

    is_edge = np.zeros((gh, gw, 4), bool)
    succ = np.full((gh, gw, 4), -1, np.int64)
    rr, cc = np.mgrid[0:gh, 0:gw]
    for s in range(4):
        hx, hy = HEAD[s]
        ox, oy = HEAD[(s + 3) % 4]
        is_edge[:, :, s] = (inner != 0) & (shifted(ox, oy) != inner)
        b = shifted(hx, hy) == inner                         # the cell ahead, B; off the grid it is 0 and inner is not
        c = shifted(hx + ox, hy + oy) == inner               # the cell diagonally ahead, C
        right = 4 * ((rr + hy + oy) * gw + cc + hx + ox) + (s + 3) % 4
        straight = 4 * ((rr + hy) * gw + cc + hx) + s
        left = 4 * (rr * gw + cc) + (s + 1) % 4
        if plant == "left_first":
            succ[:, :, s] = np.where(b, np.where(c, right, straight), left)
        else:
            succ[:, :, s] = np.where(c, right, np.where(b, straight, left))
    flat_edge, flat_succ = is_edge.reshape(-1), succ.reshape(-1).tolist()
    ids = np.nonzero(flat_edge)[0]
    assert flat_edge[succ.reshape(-1)[ids]].all()            # the successor of a boundary edge is a boundary edge
    assert len(np.unique(succ.reshape(-1)[ids])) == len(ids)                 # and the successor is a permutation of them
    seen = [False] * flat_edge.size
    rings = []
    for e0 in ids.tolist():
        if seen[e0]:
            continue
        cyc, e = [], e0
        while not seen[e]:
            seen[e] = True
            cyc.append(e)
            e = flat_succ[e]
        assert e == e0 and len(cyc) <= len(ids)
        cell, side = np.array(cyc) // 4, np.array(cyc) % 4
        tx = cell % gw + np.array(TAIL)[side, 0]
        ty = cell // gw + np.array(TAIL)[side, 1]
        corner = ty * (gw + 1) + tx
        at = int(np.argmin(corner))
        assert (corner == corner[at]).sum() == 1             # the smallest corner is passed once
        if plant == "start_edge":
            at = 0                                           # e0 is the smallest edge of the ring: ids are in rising order
        cell, side, tx, ty = (np.roll(a, -at) for a in (cell, side, tx, ty))
        hx, hy = tx + np.array(HEAD)[side, 0], ty + np.array(HEAD)[side, 1]
        keep = side != np.roll(side, 1) if plant != "collinear" else np.ones(len(side), bool)
        verts = list(zip(tx[keep].tolist(), ty[keep].tolist()))
        if plant == "reversed":
            verts = verts[:1] + verts[1:][::-1]
        k = int(L.reshape(-1)[cell[0]])
        key = (k, int(ty[0]), int(tx[0])) if plant != "edge_order" else (0, e0, 0)
        rings.append((k, verts, int((hx * ty - tx * hy).sum()), int((side % 2 == 0).sum()), int((side % 2 == 1).sum()), key))
    out = _table(rings, n)
    if plant == "edge_order":
        out["first_ring"] = np.zeros(n + 1, np.int32)
    return out


def trace_corners(labels, n):
    """Statement two: corners only.  Per label, the directed unit edges (tail, head) of its cells' sides that face another
    value; a dictionary from tail to the headings that leave it; a walk that takes, where two leave, the right turn."""
    L = clean(labels, n)
    gh, gw = L.shape
    rings = []
    P = np.zeros((gh + 2, gw + 2), np.int32)
    P[1:-1, 1:-1] = L
    leaving = {}                                             # (label, tail x, tail y) -> set of headings
    for s in range(4):
        ox, oy = HEAD[(s + 3) % 4]
        rows, cols = np.nonzero((L != 0) & (P[1 + oy:1 + oy + gh, 1 + ox:1 + ox + gw] != L))
        for r, c, k in zip(rows.tolist(), cols.tolist(), L[rows, cols].tolist()):
            leaving.setdefault((k, c + TAIL[s][0], r + TAIL[s][1]), set()).add(HEAD[s])
    todo = {(k, x, y, h) for (k, x, y), hs in leaving.items() for h in hs}
    total = len(todo)
    for k, x, y, h in sorted(todo, key=lambda e: (e[0], e[2], e[1], e[3] != (0, 1))):
        # in this order the first edge met of a ring leaves the ring's smallest corner: heading south (exterior) before east (hole)
        if (k, x, y, h) not in todo:
            continue
        path, steps = [], 0
        cx, cy, ch = x, y, h
        while (k, cx, cy, ch) in todo:
            todo.discard((k, cx, cy, ch))
            path.append((cx, cy, ch))
            cx, cy = cx + ch[0], cy + ch[1]
            out = leaving[(k, cx, cy)]
            assert len(out) in (1, 2)
            turn_right = (-ch[1], ch[0])                     # E -> S -> W -> N -> E with y down
            ch = turn_right if len(out) == 2 else next(iter(out))
            assert ch in out
            steps += 1
            assert steps <= total
        assert (cx, cy, ch) == (x, y, h)
        assert min((py, px) for px, py, _ in path) == (y, x)
        verts = [(px, py) for i, (px, py, ph) in enumerate(path) if path[i - 1][2] != ph]
        closed = verts + verts[:1]
        area2 = sum(x1 * y0 - x0 * y1 for (x0, y0), (x1, y1) in zip(closed[:-1], closed[1:]))
        ew = sum(abs(x1 - x0) for (x0, _), (x1, _) in zip(closed[:-1], closed[1:]))
        ns = sum(abs(y1 - y0) for (_, y0), (_, y1) in zip(closed[:-1], closed[1:]))
        rings.append((k, verts, area2, ew, ns, (k, y, x)))
    return _table(rings, n)


def with_grid(rings, grid, n):
    """The entries dsm.outlines adds with a grid."""
    out = dict(rings)
    v = rings["vertices"].astype(np.float64)
    xres, yres = float(grid.xres), float(grid.yres)
    out["vertices_en"] = np.stack([float(grid.e0) + (v[:, 0] - 0.5) * xres, float(grid.n0) - (v[:, 1] - 0.5) * yres], 1)
    out["perimeter_m"] = rings["edges"][:, 0].astype(np.float64) * xres + rings["edges"][:, 1].astype(np.float64) * yres
    per = np.zeros((n, 2), np.int64)
    np.add.at(per, rings["label"].astype(np.int64) - 1, rings["edges"].astype(np.int64))
    out["label_perimeter_m"] = per[:, 0].astype(np.float64) * xres + per[:, 1].astype(np.float64) * yres
    out["n_holes"] = np.bincount(rings["label"][rings["area2"] < 0].astype(np.int64) - 1, minlength=n).astype(np.int32)[:n]
    return out


def difference(got, want):
    """None if the two ring tables are equal in every entry, dtype and shape; else a sentence that names the first ring that
    differs and in what."""
    for key in want:
        if key not in got:
            return "entry %r is missing" % key
        g, w = np.asarray(got[key]), np.asarray(want[key])
        if g.dtype != w.dtype:
            return "entry %r has dtype %s, not %s" % (key, g.dtype, w.dtype)
    if sorted(got) != sorted(want):
        return "entries %s, not %s" % (sorted(got), sorted(want))
    nr = len(want["label"])
    for r in range(min(nr, len(got["label"]))):
        for key in ("label", "area2", "edges"):
            if not np.array_equal(got[key][r], want[key][r]):
                return "ring %d: %s %s, not %s" % (r, key, got[key][r].tolist(), want[key][r].tolist())
        gv = got["vertices"][got["offset"][r]:got["offset"][r + 1]]
        wv = want["vertices"][want["offset"][r]:want["offset"][r + 1]]
        if not np.array_equal(gv, wv):
            return "ring %d (label %d): vertices %s ..., not %s ..." % (r, want["label"][r], gv[:6].tolist(), wv[:6].tolist())
    if len(got["label"]) != nr:
        return "%d rings, not %d" % (len(got["label"]), nr)
    for key in want:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        if g.shape != w.shape or not np.array_equal(g, w, equal_nan=g.dtype.kind == "f"):
            return "entry %r differs" % key
    return None


def same_rings(got, want, what=""):
    message = difference(got, want)
    assert message is None, (what, message)


def fill(vertices, offset, ring_label, shape):
    """The even-odd fill of smvs_dsm_burn: toggles along the vertical edges, then the running XOR of every row."""
    gh, gw = shape
    T = np.zeros((gh, gw), np.int32)
    V = np.asarray(vertices).reshape(-1, 2).tolist()
    for r in range(len(ring_label)):
        ring = V[offset[r]:offset[r + 1]]
        for (x0, y0), (x1, y1) in zip(ring, ring[1:] + ring[:1]):
            if x0 != x1 and y0 != y1:
                raise ValueError("diagonal edge")
            if x0 == x1 and x0 < gw:
                ya, yb = max(min(y0, y1), 0), min(max(y0, y1), gh)
                if ya < yb:
                    T[ya:yb, max(x0, 0)] ^= np.int32(ring_label[r])
    return np.bitwise_xor.accumulate(T, axis=1).astype(np.int32)


def shoelace2(ring):
    """Twice the signed area of a closed or open list of (x, y), counter-clockwise positive in a y-up frame."""
    a = np.asarray(ring, np.float64)
    b = np.roll(a, -1, axis=0)
    return float((a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]).sum())


def read_geojson(path):
    """-> [(properties, [ring (m, 2) float64, closed])] of a FeatureCollection of Polygons."""
    with open(path) as f:
        doc = json.load(f)
    assert doc["type"] == "FeatureCollection"
    out = []
    for feature in doc["features"]:
        assert feature["type"] == "Feature" and feature["geometry"]["type"] == "Polygon"
        rings = [np.array(ring, np.float64).reshape(-1, 2) for ring in feature["geometry"]["coordinates"]]
        assert all(len(ring) >= 5 and (ring[0] == ring[-1]).all() for ring in rings)
        out.append((feature["properties"], rings))
    return out


# ---- closed forms ---------------------------------------------------------------------------------------------------------------
def _rings(n, *rings):
    """rings: (label, [(x, y) ...]) in table order -> the dict, with area2 and edges from the vertices."""
    rows = []
    for k, verts in rings:
        closed = verts + verts[:1]
        pairs = list(zip(closed[:-1], closed[1:]))
        rows.append((k, verts, sum(x1 * y0 - x0 * y1 for (x0, y0), (x1, y1) in pairs), sum(abs(x1 - x0) for (x0, _), (x1, _) in pairs),
                     sum(abs(y1 - y0) for (_, y0), (_, y1) in pairs), (k, verts[0][1], verts[0][0])))
    return _table(rows, n)


def serpentine(g, r, c):
    """Every other column, joined in turn at the last row and at row 0: one 4-connected snake of g / 2 columns (g even), whose
    one ring has 4 (g / 2) vertices, starts at (0, 0) and ends at (1, 0).  r, c: row and column indices, numpy or torch."""
    return (c % 2 == 0) | ((c % 4 == 1) & (r == g - 1) & (c < g - 1)) | ((c % 4 == 3) & (r == 0) & (c < g - 1))


def closed_forms():
    """[(name, labels, n, rings)]: the scenes of the issue with their rings written out by hand."""
    out = []
    out.append(("single cell", np.array([[1]], np.int32), 1, _rings(1, (1, [(0, 0), (0, 1), (1, 1), (1, 0)]))))
    out.append(("full grid", np.ones((3, 5), np.int32), 1, _rings(1, (1, [(0, 0), (0, 3), (5, 3), (5, 0)]))))
    frame = np.ones((3, 3), np.int32)
    frame[1, 1] = 0
    out.append(("frame", frame, 1, _rings(1, (1, [(0, 0), (0, 3), (3, 3), (3, 0)]), (1, [(1, 1), (2, 1), (2, 2), (1, 2)]))))
    two4 = np.array([[1, 0], [0, 2]], np.int32)              # connectivity 4 gives two labels: two squares that share a corner
    out.append(("two cells at a corner, connectivity 4", two4, 2,
                _rings(2, (1, [(0, 0), (0, 1), (1, 1), (1, 0)]), (2, [(1, 1), (1, 2), (2, 2), (2, 1)]))))
    two8 = np.array([[1, 0], [0, 1]], np.int32)              # connectivity 8 gives one: right first joins them in one ring
    out.append(("two cells at a corner, connectivity 8", two8, 1,
                _rings(1, (1, [(0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (2, 1), (1, 1), (1, 0)]))))
    pinched = np.ones((4, 4), np.int32)                      # a frame whose hole is two cells that meet at a corner: two holes
    pinched[1, 1] = pinched[2, 2] = 0
    out.append(("frame pinched at a corner", pinched, 1,
                _rings(1, (1, [(0, 0), (0, 4), (4, 4), (4, 0)]), (1, [(1, 1), (2, 1), (2, 2), (1, 2)]), (1, [(2, 2), (3, 2), (3, 3), (2, 3)]))))
    island = np.ones((5, 5), np.int32)                       # cell (2, 2) stands in the hole and meets cell (1, 1) of the frame at
    island[1, 2:4] = island[2, 1] = island[2, 3] = island[3, 1:4] = 0       # corner (2, 2) only: the hole's ring passes it twice
    out.append(("island in a hole joined by a corner", island, 1,
                _rings(1, (1, [(0, 0), (0, 5), (5, 5), (5, 0)]),
                       (1, [(2, 1), (4, 1), (4, 4), (1, 4), (1, 2), (2, 2), (2, 3), (3, 3), (3, 2), (2, 2)]))))
    return out
