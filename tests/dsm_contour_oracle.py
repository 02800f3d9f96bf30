"""The contour rule of include/satmvs.h ("Contours") in numpy, twice: walk() follows the rule's text with dictionaries, one level
and one crossing at a time; trace() states it on arrays for all levels at once (the crossings of every lattice edge as a range
of the sorted level table, a successor array, then a walk over it) and is fast enough for 257 x 301.  Both give the dict of
dsm.contours; same_lines() compares two such dicts entry by entry, the float64 vertices by their bits."""
import json

import numpy as np

MAX_Z = np.float32(32768.0)
KEYS = ("level_index", "level", "closed", "offset", "first_line", "vertices", "edge")
PLANTED = ("above_ge", "saddle", "right", "ring_start", "t_other_end", "three_corners")


# ---- heights and levels --------------------------------------------------------------------------------------------------------
def quantise(dsm, nodata=-999.0):
    """(ok, q): a node is valid iff finite, != (float)nodata and |z| <= 32768; q = rint((double)z 256), halves to even."""
    z = np.asarray(dsm, np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(z) & (z != np.float32(nodata)) & (np.abs(z) <= MAX_Z)
    return ok, np.rint(np.where(ok, z, np.float32(0.0)).astype(np.float64) * 256.0).astype(np.int64)


def level_keys(levels_m):
    """Levels in metres -> the odd integers K = 2 floor(256 level) + 1 in units of 2^-9 m."""
    return (2 * np.floor(256.0 * np.asarray(levels_m, np.float64)).astype(np.int64) + 1).astype(np.int64)


def levels_for(dsm, interval, base=0.0, nodata=-999.0):
    """dsm.contour_levels: base + k interval strictly inside the valid heights' range, float64."""
    ok, _ = quantise(dsm, nodata)
    if not ok.any():
        return np.zeros(0, np.float64)
    z = np.asarray(dsm, np.float32)[ok].astype(np.float64)
    k = np.arange(np.floor((z.min() - base) / interval), np.ceil((z.max() - base) / interval) + 1.0)
    levels = base + k * interval
    return levels[(levels > z.min()) & (levels < z.max())]


def _eid(p, q, gw):
    """The lattice edge between two adjacent nodes."""
    (r0, c0), (r1, c1) = min(p, q), max(p, q)
    assert (r1 - r0, c1 - c0) in ((0, 1), (1, 0))
    return 2 * (r0 * gw + c0) + (1 if r1 != r0 else 0)


def _vertex(q, K, e, gw, plant=None):
    """The vertex of crossing (K, e): one division of two exact integers, one addition."""
    r, c, o = (e >> 1) // gw, (e >> 1) % gw, e & 1
    qa, qb = int(q[r, c]), int(q[(r, c + 1) if o == 0 else (r + 1, c)])
    t = np.float64(K - 2 * qa) / np.float64(2 * qb - 2 * qa)
    if plant == "t_other_end":
        t = np.float64(1.0) - np.float64(K - 2 * qb) / np.float64(2 * qa - 2 * qb)
    return (np.float64(c) + t, np.float64(r)) if o == 0 else (np.float64(c), np.float64(r) + t)


def _table(lines, K, n_levels):
    """[(level index, closed, [eid], [(x, y)])] ordered by (level index, first eid) -> the dict."""
    lines = sorted(lines, key=lambda t: (t[0], t[2][0]))
    index = np.array([t[0] for t in lines], np.int32).reshape(-1)
    offset = np.zeros(len(lines) + 1, np.int32)
    offset[1:] = np.cumsum([len(t[2]) for t in lines])
    xy = [p for t in lines for p in t[3]]
    return {"level_index": index, "level": np.asarray(K, np.float64)[index] / 512.0,
            "closed": np.array([t[1] for t in lines], bool).reshape(-1), "offset": offset,
            "first_line": np.searchsorted(index, np.arange(n_levels + 1), side="left").astype(np.int32),
            "vertices": np.array(xy, np.float64).reshape(-1, 2), "edge": np.array([e for t in lines for e in t[2]], np.int32).reshape(-1)}


# ---- the rule, one crossing at a time ------------------------------------------------------------------------------------------
def walk(dsm, K, nodata=-999.0, plant=None):
    """The rule's text.  K: odd integers, strictly rising.  plant: one of PLANTED, a wrong reading of the rule."""
    ok, q = quantise(dsm, nodata)
    gh, gw = q.shape
    lines = []
    for li, k in enumerate(int(v) for v in K):
        kk = k - 1 if plant == "above_ge" else k             # an even level: a node on it counts as above

        def valid(p):
            return 0 <= p[0] < gh and 0 <= p[1] < gw and bool(ok[p])

        def above(p):
            if plant == "right":
                return 2 * int(q[p]) < kk
            return 2 * int(q[p]) >= kk if plant == "above_ge" else 2 * int(q[p]) > kk

        crossed = {}
        for r in range(gh):
            for c in range(gw):
                for o, b in ((0, (r, c + 1)), (1, (r + 1, c))):
                    if valid((r, c)) and valid(b) and above((r, c)) != above(b):
                        crossed[2 * (r * gw + c) + o] = ((r, c), b)
        succ = {}
        for e, (a, b) in crossed.items():
            (r, c), o = a, e & 1
            if o == 0:                                       # west above: north into (r - 1, c); east above: south into (r, c)
                H, L, S = (a, b, (r - 1, c)) if above(a) else (b, a, (r, c))
            else:                                            # north above: east into (r, c); south above: west into (r, c - 1)
                H, L, S = (a, b, (r, c)) if above(a) else (b, a, (r, c - 1))
            corners = [(S[0], S[1]), (S[0], S[1] + 1), (S[0] + 1, S[1] + 1), (S[0] + 1, S[1])]
            n_valid = sum(valid(p) for p in corners)
            if n_valid < (3 if plant == "three_corners" else 4):
                continue
            near = lambda p, other: next(x for x in corners if x != other and abs(x[0] - p[0]) + abs(x[1] - p[1]) == 1)   # noqa: E731
            H2, L2 = near(H, L), near(L, H)
            up = lambda p: valid(p) and above(p)             # noqa: E731  (an invalid corner only under the planted error)
            if not up(H2) and not up(L2):
                out = (H, H2)
            elif up(H2) and not up(L2):
                out = (H2, L2)
            elif up(H2) and up(L2):
                out = (L, L2)
            else:
                total = sum(int(q[p]) for p in corners if valid(p))
                mean_above = total < 2 * kk if plant == "right" else total > 2 * kk
                if plant == "saddle":
                    mean_above = not mean_above
                out = (L, L2) if mean_above else (H, H2)
            e2 = _eid(out[0], out[1], gw)
            if e2 in crossed:                                # always, but for the planted three-corner squares
                succ[e] = e2
        pred = {e2: e for e, e2 in succ.items()}
        assert len(pred) == len(succ)                        # the successor is injective
        seen = set()
        for e in sorted(crossed):
            if e in pred or e not in succ:
                continue
            chain = [e]
            while chain[-1] in succ:
                chain.append(succ[chain[-1]])
            seen.update(chain)
            lines.append((li, False, chain, [_vertex(q, kk, x, gw, plant) for x in chain]))
        for e in sorted(crossed):
            if e in seen or e not in succ or e not in pred:
                continue
            ring = [e]
            while succ[ring[-1]] != e:
                ring.append(succ[ring[-1]])
            seen.update(ring)
            if plant == "ring_start":
                ring = ring[1:] + ring[:1]
            lines.append((li, True, ring, [_vertex(q, kk, x, gw, plant) for x in ring]))
    return _table(lines, K, len(K))


# ---- the rule on arrays --------------------------------------------------------------------------------------------------------
def crossings(dsm, K, nodata=-999.0):
    """Per lattice edge (2 gh gw slots, eid order): the first level that crosses it and how many do.  -> lo, cnt, ok, q."""
    ok, q = quantise(dsm, nodata)
    K = np.asarray(K, np.int64)
    gh, gw = q.shape
    lo, cnt = np.zeros((gh, gw, 2), np.int64), np.zeros((gh, gw, 2), np.int64)
    for o, (a, b) in enumerate(((np.s_[:, :-1], np.s_[:, 1:]), (np.s_[:-1, :], np.s_[1:, :]))):
        both = ok[a] & ok[b]
        first = np.searchsorted(K, 2 * np.minimum(q[a], q[b]), side="right")
        last = np.searchsorted(K, 2 * np.maximum(q[a], q[b]), side="right")
        lo[a + (o,)] = first
        cnt[a + (o,)] = np.where(both, last - first, 0)
    return lo.reshape(-1), cnt.reshape(-1), ok, q


def trace(dsm, K, nodata=-999.0):
    """The same lines from arrays: every crossing (eid, level) numbered in that order, its successor's number, then a walk."""
    K = np.asarray(K, np.int64)
    lo, cnt, ok, q = crossings(dsm, K, nodata)
    gh, gw = q.shape
    base = np.concatenate([[0], np.cumsum(cnt)])
    n = int(base[-1])
    e = np.repeat(np.arange(2 * gh * gw), cnt)
    lev = lo[e] + np.arange(n) - base[e]
    k = K[lev] if n else np.zeros(0, np.int64)
    r, c, o = (e >> 1) // gw, (e >> 1) % gw, e & 1
    br, bc = r + o, c + 1 - o
    qa, qb = q[r, c], q[br, bc]
    a_up = 2 * qa > k
    hr, hc, lr, lc = np.where(a_up, r, br), np.where(a_up, c, bc), np.where(a_up, br, r), np.where(a_up, bc, c)
    dr = np.where(o == 0, np.where(a_up, -1, 1), 0)
    dc = np.where(o == 1, np.where(a_up, 1, -1), 0)
    h2r, h2c, l2r, l2c = hr + dr, hc + dc, lr + dr, lc + dc
    inside = (h2r >= 0) & (h2r < gh) & (h2c >= 0) & (h2c < gw)
    cr = lambda x, m: np.clip(x, 0, m - 1)                   # noqa: E731
    live = inside & ok[cr(h2r, gh), cr(h2c, gw)] & ok[cr(l2r, gh), cr(l2c, gw)]
    qh, ql, qh2, ql2 = q[hr, hc], q[lr, lc], q[cr(h2r, gh), cr(h2c, gw)], q[cr(l2r, gh), cr(l2c, gw)]
    h2_up, l2_up = 2 * qh2 > k, 2 * ql2 > k
    way = np.where(h2_up, np.where(l2_up, 2, 1), np.where(l2_up & (qh + ql + qh2 + ql2 > 2 * k), 2, 0))      # 0 left, 1 straight, 2 right
    pr, pc = np.choose(way, [hr, h2r, lr]), np.choose(way, [hc, h2c, lc])
    sr, sc = np.where(way == 0, h2r, l2r), np.where(way == 0, h2c, l2c)
    e2 = np.where(live, 2 * (np.minimum(pr, sr) * gw + np.minimum(pc, sc)) + (pr != sr), 0)
    succ = np.where(live, base[e2] + lev - lo[e2], -1)
    assert (succ < n).all() and (lev[succ[live]] == lev[live]).all() and (e[succ[live]] == e2[live]).all()
    has_pred = np.zeros(n, bool)
    has_pred[succ[live]] = True
    assert has_pred.sum() == live.sum()                      # injective
    t = (k - 2 * qa).astype(np.float64) / np.where(qa == qb, 1, 2 * qb - 2 * qa).astype(np.float64)
    x = np.where(o == 0, c.astype(np.float64) + t, c.astype(np.float64))
    y = np.where(o == 0, r.astype(np.float64), r.astype(np.float64) + t)
    nxt, seen, lines = succ.tolist(), np.zeros(n, bool), []
    for j in np.flatnonzero(~has_pred & live).tolist():
        chain = [j]
        while nxt[chain[-1]] >= 0:
            chain.append(nxt[chain[-1]])
        seen[chain] = True
        lines.append((False, chain))
    for j in np.flatnonzero(has_pred & live).tolist():       # id order: the first crossing of a ring met is its smallest eid
        if seen[j]:
            continue
        ring = [j]
        while nxt[ring[-1]] != j:
            ring.append(nxt[ring[-1]])
        seen[ring] = True
        lines.append((True, ring))
    lines.sort(key=lambda t: (lev[t[1][0]], e[t[1][0]]))
    order = np.array([j for _, ids in lines for j in ids], np.int64).reshape(-1)
    index = np.array([lev[ids[0]] for _, ids in lines], np.int32).reshape(-1)
    offset = np.zeros(len(lines) + 1, np.int32)
    offset[1:] = np.cumsum([len(ids) for _, ids in lines])
    return {"level_index": index, "level": K.astype(np.float64)[index] / 512.0, "closed": np.array([cl for cl, _ in lines], bool).reshape(-1),
            "offset": offset, "first_line": np.searchsorted(index, np.arange(len(K) + 1), side="left").astype(np.int32),
            "vertices": np.stack([x[order], y[order]], axis=1).reshape(-1, 2), "edge": e[order].astype(np.int32)}


def n_cross(dsm, K, nodata=-999.0):
    return int(crossings(dsm, K, nodata)[1].sum())


# ---- the grid's entries, GeoJSON -------------------------------------------------------------------------------------------------
def with_grid(lines, grid):
    """vertices_en and length_m as dsm.contours adds them: a line's segment lengths added one after the other in vertex order,
    a ring's closing segment last."""
    out = dict(lines)
    v, off = lines["vertices"], lines["offset"]
    en = np.stack([float(grid.e0) + v[:, 0] * float(grid.xres), float(grid.n0) - v[:, 1] * float(grid.yres)], axis=1).reshape(-1, 2)
    length = np.zeros(len(off) - 1, np.float64)
    for i in range(len(length)):
        p = en[off[i]:off[i + 1]]
        if lines["closed"][i]:
            p = np.concatenate([p, p[:1]])
        d = p[1:] - p[:-1]
        total = np.float64(0.0)
        for s in np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2):
            total = total + s
        length[i] = total
    out["vertices_en"], out["length_m"] = en, length
    return out


def read_geojson(path):
    """[(properties, coordinates as a float64 (m, 2) array)] of a FeatureCollection of LineStrings."""
    with open(path) as f:
        doc = json.load(f)
    assert doc["type"] == "FeatureCollection"
    out = []
    for feature in doc["features"]:
        assert feature["type"] == "Feature" and feature["geometry"]["type"] == "LineString"
        out.append((feature["properties"], np.array(feature["geometry"]["coordinates"], np.float64).reshape(-1, 2)))
    return out


# ---- the comparison ---------------------------------------------------------------------------------------------------------------
def difference(got, want):
    """None if every entry of `want` is in `got` with the same dtype, shape and values (float64 by their bits), else what differs."""
    for key in want:
        if key not in got:
            return "entry %r is missing" % key
        g, w = np.asarray(got[key]), np.asarray(want[key])
        if g.dtype != w.dtype:
            return "entry %r: dtype %s, expected %s" % (key, g.dtype, w.dtype)
        if g.shape != w.shape:
            return "entry %r: shape %s, expected %s" % (key, g.shape, w.shape)
        if g.dtype == np.float64:
            g, w = np.ascontiguousarray(g).view(np.int64), np.ascontiguousarray(w).view(np.int64)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[0].tolist()
            return "entry %r differs at %s: %r, expected %r (%d places)" % (key, at, g[tuple(at)].item(), w[tuple(at)].item(), int((g != w).sum()))
    return None


def same_lines(got, want, what):
    message = difference(got, want)
    assert message is None, (what, message)


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def random_scene(gh, gw, seed, voids=0.05, amp=3.0):
    """Smooth hills plus noise of a few metres, a share `voids` of the cells NaN or nodata."""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:gh, 0:gw]
    z = (20.0 + 8.0 * np.sin(c / 5.0) * np.cos(r / 7.0) + amp * rng.standard_normal((gh, gw))).astype(np.float32)
    gone = rng.random((gh, gw)) < voids
    z[gone] = np.where(rng.random((gh, gw)) < 0.5, np.float32(np.nan), np.float32(-999.0))[gone]
    return z


def cone(gh, gw, top=50.0, slope=3.0):
    r, c = np.mgrid[0:gh, 0:gw]
    return (top - slope * np.hypot(r - (gh - 1) / 2.0 - 0.13, c - (gw - 1) / 2.0 + 0.21)).astype(np.float32)


def serpentine(gh, gw, low=0.0, high=10.0, step=2):
    """A ridge that runs east along row 1, turns at the end, runs back along row 1 + step, and so on (joined alternately at the
    east and the west end): one level between low and high gives one closed line round all of it, of about 4 gh gw / step
    vertices."""
    z = np.full((gh, gw), low, np.float32)
    rows = np.arange(1, gh - 1, step)
    for i, r in enumerate(rows):
        z[r, 1:gw - 1] = high
        if i + 1 < len(rows):
            col = gw - 2 if i % 2 == 0 else 1
            z[r:r + step + 1, col] = high
    return z


def shoelace2(p):
    """Twice the signed area of a closed line with y running SOUTH, as seen north up: > 0 counter-clockwise."""
    x, y = p[:, 0], -p[:, 1]
    return float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))
