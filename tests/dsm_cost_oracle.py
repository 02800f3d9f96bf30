"""The cost-distance rule of include/satmvs.h ("Cost distance") in Python, every part stated twice: the keys as a heapq Dijkstra
on Python ints and as synchronous numpy sweeps of the key equation, the back-links as a loop after the text and as arrays.  The
two statements are held against each other in test_dsm_cost_cpu.py and the device against them in test_dsm_cost_gpu.py.  The
switches of the loop statements (neighbours, own_friction, low_ties, barriers_passable, slope_sign, rint_bin, floor_one, and a
diagonal length handed to lengths()) plant the errors the GPU file's comparison has to report; their defaults are the rule.
numpy only."""
import heapq
import math

import numpy as np

import dsm_hydro_oracle as ho

DC, DR = ho.DC, ho.DR                                         # k = 0 .. 7: E, SE, S, SW, W, NW, N, NE; columns east, rows south
BARRIER = np.uint64(0xffffffffffffffff)
INF = np.uint64(0xfffffffffffffffe)
NO_MAX = 2 ** 64 - 1
BIG = np.int64(2 ** 62)                                       # above every D: the sweeps' +infinity
XRES, YRES = 5.0, 2.5


# ---- quantisation ----------------------------------------------------------------------------------------------------------------
def lengths(xres, yres, diagonal=None):
    """L[k] = rint(256 length of step k), Python ints.  Planted error: diagonal = another length for the diagonal steps [m]."""
    h = math.hypot(xres, yres) if diagonal is None else diagonal
    return [int(np.rint(256.0 * d)) for d in (xres, h, yres, h, xres, h, yres, h)]


def quantise_friction(f, nodata=-999.0):
    f = np.asarray(f)
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(f) | (f == np.asarray(nodata, f.dtype)) | (f <= 0)
    q = np.where(bad, 0.0, np.rint(256.0 * np.where(bad, 0, f).astype(np.float64)))
    if q.max(initial=0.0) > 65535:
        raise ValueError("friction above 65535 / 256")
    return q.astype(np.uint16)


def slope_table(fn):
    table = np.zeros(256, np.int32)
    for b in range(256):
        v = float(fn((b - 127.5) / 32.0))
        if math.isfinite(v) and v > 0.0:
            if v > 65535 / 256.0:
                raise ValueError("vertical factor above 65535 / 256")
            table[b] = int(np.rint(256.0 * v))
    return table


def tobler(t):
    v = math.exp(3.5 * (abs(t + 0.05) - 0.05)) * math.sqrt(1.0 + t * t)
    return v if v <= 65535 / 256.0 else float("nan")


def passable(gh, gw, friction=None, z=None, nodata=-999.0):
    ok = np.ones((gh, gw), bool) if friction is None else np.asarray(friction) != 0
    return ok if z is None else ok & ho.valid(z, nodata)


# ---- the step, on Python ints --------------------------------------------------------------------------------------------------
def bin_of(delta, length, rint_bin=False):
    """clamp(floor(32 delta / length), -128, 127) + 128.  Planted error: rint_bin rounds to nearest instead."""
    b = int(np.rint(32 * delta / length)) if rint_bin else (32 * delta) // length
    return min(max(b, -128), 127) + 128


def step_cost(fc, fn, qc, qn, length, table=None, reverse=False, own_friction=False, slope_sign=1, rint_bin=False, floor_one=True):
    """w of the step c -> n, or None where the table forbids it.  Planted errors: own_friction takes 2 f_c for f_c + f_n,
    slope_sign=-1 turns the slope, rint_bin as bin_of, floor_one=False leaves max(1, .) off."""
    T = 256
    if table is not None:
        delta = (qc - qn) if reverse else (qn - qc)
        T = int(table[bin_of(slope_sign * delta, length, rint_bin)])
        if T == 0:
            return None
    w = ((2 * fc if own_friction else fc + fn) * length * T) >> 10
    return max(1, w) if floor_one else w


def _inputs(src, friction, z, nodata, barriers_passable=False):
    src = np.asarray(src)
    gh, gw = src.shape
    ok = passable(gh, gw, friction, z, nodata)
    walk = np.ones_like(ok) if barriers_passable else ok
    f = (np.full((gh, gw), 256) if friction is None else np.asarray(friction)).astype(np.int64).tolist()
    q = (np.zeros((gh, gw), np.int64) if z is None else ho.quanta(z, nodata)).tolist()
    return gh, gw, ok, walk, f, q


def pack(D, ok):
    """int64 D with BIG for unreached -> the device's uint64 words."""
    return np.where(~ok, BARRIER, np.where(D >= BIG, INF, D.astype(np.uint64)))


# ---- keys: Dijkstra on Python ints -------------------------------------------------------------------------------------------------
def keys_heap(src, L, friction=None, z=None, table=None, reverse=False, nodata=-999.0, neighbours=8, barriers_passable=False, **step):
    """-> (gh, gw) uint64 keys.  Planted errors: neighbours=4 steps through E, S, W, N only; barriers_passable walks over
    barriers (friction 0, height 0) although they keep their all-ones key unless reached; the rest as step_cost."""
    gh, gw, ok, walk, f, q = _inputs(src, friction, z, nodata, barriers_passable)
    tab = None if table is None else [int(t) for t in table]
    L = [int(v) for v in L]
    ks = range(8) if neighbours == 8 else (0, 2, 4, 6)
    D = {}
    heap = [(0, int(r), int(c)) for r, c in np.argwhere((np.asarray(src) != 0) & ok)]
    for _, r, c in heap:
        D[(r, c)] = 0
    heapq.heapify(heap)
    done = set()
    while heap:
        d, r, c = heapq.heappop(heap)
        if (r, c) in done:
            continue
        done.add((r, c))
        for k in ks:                                         # the cell that has (r, c) as its neighbour k
            rr, cc = r - DR[k], c - DC[k]
            if rr < 0 or rr >= gh or cc < 0 or cc >= gw or not walk[rr, cc] or (rr, cc) in done:
                continue
            w = step_cost(f[rr][cc], f[r][c], q[rr][cc], q[r][c], L[k], tab, reverse, **step)
            if w is not None and d + w < D.get((rr, cc), 1 << 63):
                D[(rr, cc)] = d + w
                heapq.heappush(heap, (d + w, rr, cc))
    out = np.where(ok, INF, BARRIER)
    for (r, c), d in D.items():
        out[r, c] = d
    return out


# ---- keys: synchronous sweeps of the key equation --------------------------------------------------------------------------------
def step_costs(gh, gw, L, friction=None, z=None, table=None, reverse=False, nodata=-999.0):
    """W (8, gh, gw) int64: the cost of the step from each cell towards its neighbour k, -1 where there is none."""
    ok = passable(gh, gw, friction, z, nodata)
    f = np.full((gh, gw), 256, np.int64) if friction is None else np.asarray(friction).astype(np.int64)
    q = np.zeros((gh, gw), np.int64) if z is None else ho.quanta(z, nodata)
    pad = lambda a: np.pad(a, 1)                             # noqa: E731  (zeros / False beyond the grid)
    pf, pq, pok = pad(f), pad(q), pad(ok)
    W = np.empty((8, gh, gw), np.int64)
    for k in range(8):
        sl = (slice(1 + DR[k], 1 + DR[k] + gh), slice(1 + DC[k], 1 + DC[k] + gw))
        T = np.full((gh, gw), 256, np.int64)
        if table is not None:
            delta = (q - pq[sl]) if reverse else (pq[sl] - q)
            T = np.asarray(table, np.int64)[np.clip(np.floor_divide(32 * delta, int(L[k])), -128, 127) + 128]
        w = np.maximum(1, ((f + pf[sl]) * int(L[k]) * T) >> 10)
        W[k] = np.where(ok & pok[sl] & (T != 0), w, -1)
    return W


def _candidates(D, W):
    """(8, gh, gw) int64: neighbour + w for every allowed step towards a reached neighbour, BIG elsewhere."""
    gh, gw = D.shape
    pD = np.pad(D, 1, constant_values=BIG)
    out = np.empty((8, gh, gw), np.int64)
    for k in range(8):
        Dn = pD[1 + DR[k]:1 + DR[k] + gh, 1 + DC[k]:1 + DC[k] + gw]
        out[k] = np.where((W[k] >= 0) & (Dn < BIG), Dn + np.maximum(W[k], 0), BIG)
    return out


def keys_sweeps(src, L, friction=None, z=None, table=None, reverse=False, nodata=-999.0, return_sweeps=False):
    """D <- min(D, min over k of D(neighbour k) + W[k]) on the whole grid at once, until nothing moves -> uint64 keys."""
    src = np.asarray(src)
    gh, gw = src.shape
    ok = passable(gh, gw, friction, z, nodata)
    W = step_costs(gh, gw, L, friction, z, table, reverse, nodata)
    D = np.where((src != 0) & ok, np.int64(0), BIG)
    sweeps = 0
    while True:
        new = np.minimum(D, _candidates(D, W).min(axis=0))
        sweeps += 1
        if np.array_equal(new, D):
            break
        D = new
    return (pack(D, ok), sweeps) if return_sweeps else pack(D, ok)


# ---- back-links ------------------------------------------------------------------------------------------------------------------
def backlinks_loop(keys, L, friction=None, z=None, table=None, reverse=False, nodata=-999.0, max_cost=NO_MAX, low_ties=True, neighbours=8,
                   barriers_passable=False, **step):
    """After the text: 0 at a source, 255 at barriers and unreached cells, else k + 1 of the cheapest step.  Planted error:
    low_ties=False gives ties to the highest k."""
    gh, gw, ok, walk, f, q = _inputs(np.zeros(keys.shape), friction, z, nodata, barriers_passable)
    tab = None if table is None else [int(t) for t in table]
    D = [[int(v) for v in row] for row in keys]
    inf = int(INF)
    code = np.full((gh, gw), 255, np.uint8)
    ks = range(8) if neighbours == 8 else (0, 2, 4, 6)
    for r in range(gh):
        for c in range(gw):
            own = D[r][c]
            if own >= inf or own > max_cost:
                continue
            if own == 0:
                code[r, c] = 0
                continue
            best = None
            for k in ks:
                rr, cc = r + DR[k], c + DC[k]
                if rr < 0 or rr >= gh or cc < 0 or cc >= gw or D[rr][cc] >= inf:
                    continue
                w = step_cost(f[r][c], f[rr][cc], q[r][c], q[rr][cc], int(L[k]), tab, reverse, **step)
                if w is None:
                    continue
                if best is None or D[rr][cc] + w < best or (not low_ties and D[rr][cc] + w == best):
                    best, code[r, c] = D[rr][cc] + w, k + 1
    return code


def backlinks_arrays(keys, L, friction=None, z=None, table=None, reverse=False, nodata=-999.0, max_cost=NO_MAX):
    gh, gw = keys.shape
    W = step_costs(gh, gw, L, friction, z, table, reverse, nodata)
    reached = (keys < INF) & (keys <= np.uint64(max_cost))
    D = np.where(keys < INF, keys, 0).astype(np.int64) + np.where(keys < INF, 0, BIG)
    cand = _candidates(D, W)
    code = np.where(cand.min(axis=0) < BIG, cand.argmin(axis=0) + 1, 255)            # argmin: the first, so the lowest k
    return np.where(~reached, 255, np.where(D == 0, 0, code)).astype(np.uint8)


# ---- reading, the whole chain, the comparison ------------------------------------------------------------------------------------
def read(keys, max_cost=NO_MAX):
    """-> raw int64, cost float64 (the conversion rounds to nearest even, the division by 2^15 is exact)."""
    reached = (keys < INF) & (keys <= np.uint64(max_cost))
    raw = np.where(reached, keys, 0).astype(np.int64) - (~reached).astype(np.int64)
    cost = np.where(keys == BARRIER, np.nan, np.where(reached, np.where(reached, keys, 0).astype(np.float64) / 32768.0, np.inf))
    return raw, cost


def chain(src, L, friction=None, z=None, table=None, reverse=False, nodata=-999.0, max_cost=NO_MAX, arrays=False, **planted):
    """Everything the device computes: {"keys", "raw", "cost", "backlink"}, by the loop statements (arrays=True: the sweeps and
    the array back-links, the same values).  `planted` takes the switches of keys_heap, step_cost and backlinks_loop."""
    if arrays:
        assert not planted
        keys = keys_sweeps(src, L, friction, z, table, reverse, nodata)
        link = backlinks_arrays(keys, L, friction, z, table, reverse, nodata, max_cost)
    else:
        kk = {k: v for k, v in planted.items() if k != "low_ties"}
        keys = keys_heap(src, L, friction, z, table, reverse, nodata, **kk)
        link = backlinks_loop(keys, L, friction, z, table, reverse, nodata, max_cost, **planted)
    raw, cost = read(keys, max_cost)
    return {"keys": keys, "raw": raw, "cost": cost, "backlink": link}


def differing(got, want):
    """One line per output that differs, with the first differing cell named: bits for floats, values otherwise, no cell
    excused.  The GPU tests assert that this is empty."""
    bad = []
    for name in want:
        a, b = np.asarray(got[name]), np.asarray(want[name])
        if a.dtype != b.dtype or a.shape != b.shape:
            bad.append("%s: got %s %s, want %s %s" % (name, a.dtype, a.shape, b.dtype, b.shape))
            continue
        ia, ib = (a.view(np.uint64), b.view(np.uint64)) if a.dtype == np.float64 else (a, b)
        if not np.array_equal(ia, ib):
            at = tuple(int(v) for v in np.argwhere(ia != ib)[0])
            bad.append("%s at cell %s: got %r, want %r (%d cells differ)" % (name, at, a[at].item(), b[at].item(), int((ia != ib).sum())))
    return bad


def walk(backlink, r, c, limit=None):
    """The cells from (r, c) along the back-links to a source, both included, and the codes taken."""
    cells, codes = [(r, c)], []
    limit = backlink.size if limit is None else limit
    while backlink[r, c] != 0:
        k = int(backlink[r, c]) - 1
        assert 0 <= k < 8 and len(codes) <= limit, (r, c, k)
        r, c = r + DR[k], c + DC[k]
        cells.append((r, c))
        codes.append(k)
    return cells, codes


def octile(gh, gw, r0, c0, L, f=256):
    """The closed form on uniform friction f without a table: m diagonal steps and the rest straight, if the diagonal is no
    shorter than a side and no longer than both."""
    wx, wd, wy = (max(1, (2 * f * int(L[k]) * 256) >> 10) for k in (0, 1, 2))
    assert max(wx, wy) <= wd <= wx + wy
    dr, dc = np.abs(np.arange(gh) - r0)[:, None], np.abs(np.arange(gw) - c0)[None, :]
    m = np.minimum(dr, dc)
    return (m * wd + (dc - m) * wx + (dr - m) * wy).astype(np.int64)


# ---- scenes the CPU and GPU tests share --------------------------------------------------------------------------------------------
FRICTION_3 = (1, 256, 65535)
FRICTION_12 = (1, 2, 3, 64, 128, 255, 256, 257, 512, 1000, 4096, 65535)
TABLE = slope_table(tobler)                                   # forbids what is steeper than about 56 degrees: cliffs abound


def friction_of(gh, gw, seed, kind, barriers=None):
    """kind None: no grid; 3 / 12: drawn from FRICTION_3 / FRICTION_12.  `barriers`: a mask of cells set to 0."""
    if kind is None and barriers is None:
        return None
    rng = np.random.default_rng(seed + 2000)
    f = np.full((gh, gw), 256, np.uint16) if kind is None else rng.choice(np.array(FRICTION_3 if kind == 3 else FRICTION_12, np.uint16), (gh, gw))
    if barriers is not None:
        f[barriers] = 0
    return np.ascontiguousarray(f)


def sources_of(ok, seed, kind):
    """kind "one": the passable cell nearest the centre; "several": five passable cells and one barrier cell if there is one;
    "all": every cell."""
    gh, gw = ok.shape
    src = np.zeros((gh, gw), np.uint8)
    if kind == "all":
        src[:] = 1
        return src
    cells = np.argwhere(ok)
    if kind == "one":
        r, c = cells[np.argmin((cells[:, 0] - gh // 2) ** 2 + (cells[:, 1] - gw // 2) ** 2)]
        src[r, c] = 1
        return src
    rng = np.random.default_rng(seed + 3000)
    for r, c in cells[rng.choice(len(cells), min(5, len(cells)), replace=False)]:
        src[r, c] = 7
    if (~ok).any():
        r, c = np.argwhere(~ok)[0]
        src[r, c] = 1
    return src


def case(gh, gw, seed, voids, kind, levels, with_table, reverse, sources="several"):
    """One scene as the keyword arguments of chain(): dsm_testkit's scene (through the hydrology oracle's hills) with a share of
    voids as barriers, by the DSM with a table and by friction 0 without one."""
    z = ho.hills(gh, gw, seed, voids, levels)
    gone = ~ho.valid(z)
    if with_table:
        friction = friction_of(gh, gw, seed, kind)
        args = dict(friction=friction, z=z, table=TABLE, reverse=reverse)
    else:
        friction = friction_of(gh, gw, seed, kind, gone if gone.any() else None)
        args = dict(friction=friction, z=None, table=None, reverse=False)
    args["src"] = sources_of(passable(gh, gw, args["friction"], args["z"]), seed, sources)
    return args


# (gh, gw, seed, share of voids, friction kind, levels, table, reverse, sources); 5 m x 2.5 m cells throughout
SCENE_CASES = [(40, 50, 1, 0.0, 3, None, False, False, "one"), (40, 50, 2, 0.05, 12, None, False, False, "several"),
               (40, 50, 3, 0.3, 3, None, False, False, "several"), (37, 45, 4, 0.0, 12, 12, True, False, "several"),
               (37, 45, 5, 0.05, 3, 12, True, True, "one"), (37, 45, 6, 0.3, 12, 12, True, False, "several"),
               (37, 45, 7, 0.05, None, None, True, True, "several"), (37, 45, 8, 0.05, 12, None, False, False, "all")]
GRID_SHAPES = [(1, 1), (1, 70), (67, 1), (2, 2), (67, 3), (31, 32), (32, 33), (33, 31)]
VARIANTS = ((False, False), (True, False), (True, True))      # without the table; with it; with it and reverse
GRID_CASES = [(gh, gw, 20 + i, 0.05, 12, 12, t, r, "several") for i, (gh, gw) in enumerate(GRID_SHAPES) for t, r in VARIANTS]
LARGE_CASES = [(257, 301, 40 + i, 0.05, 12, None, t, r, "several") for i, (t, r) in enumerate(VARIANTS)]


def case_id(case):
    return "%dx%d-s%d-v%g-f%s-l%s-%s%s-%s" % (case[:6] + ("table" if case[6] else "flat", "-rev" if case[7] else "", case[8]))


TINY_XRES, TINY_YRES = 2.0 ** -8, 2.0 ** -7                   # L = 1, 2, 2: with friction 1 .. 3 the floor of one unit a step holds


def tiny_case(gh=21, gw=35, seed=9):
    """Cells of 2^-8 m x 2^-7 m with friction from 1, 2, 3 and a few barriers: x >> 10 is 0 .. 3, so max(1, .) decides.
    -> (the keyword arguments of chain(), L)."""
    rng = np.random.default_rng(seed)
    f = rng.integers(1, 4, (gh, gw)).astype(np.uint16)
    f[rng.random((gh, gw)) < 0.05] = 0
    return dict(friction=f, z=None, table=None, reverse=False, src=sources_of(f != 0, seed, "several")), lengths(TINY_XRES, TINY_YRES)


def serpentine(gh, gw):
    """Walls (friction 0) and a corridor of friction 256 along every second row, turning at alternate ends; the source is its
    first cell: the longest path a grid of this size has.  -> (friction, sources, the corridor's cells in order)."""
    _, path = ho.serpentine(gh, gw)
    f = np.zeros((gh, gw), np.uint16)
    for r, c in path:
        f[r, c] = 256
    src = np.zeros((gh, gw), np.uint8)
    src[path[0]] = 1
    return f, src, path


# the planted errors: the switches that turn the loop statements into each, as chain() takes them
PLANTED = {"4-neighbour steps": dict(neighbours=4), "own friction instead of the sum": dict(own_friction=True),
           "ties to the highest k": dict(low_ties=False), "diagonal length equal to the straight one": "diagonal",
           "barriers passable": dict(barriers_passable=True), "the slope's sign turned": dict(slope_sign=-1),
           "rint for the floor in the bin": dict(rint_bin=True), "the max(1, .) left off": dict(floor_one=False)}
