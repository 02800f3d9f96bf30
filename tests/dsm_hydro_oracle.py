"""The hydrology rule of include/satmvs.h ("Hydrology") in Python, every part stated twice: a loop after the text on Python ints,
and arrays.  The two statements are held against each other in test_dsm_hydro_cpu.py and the device against one of them in
test_dsm_hydro_gpu.py.  The switches of the loop statements (neighbours, reset_d, void_outlets, steepest, low_ties, diagonal,
own) plant the errors the GPU file's comparison has to report; their defaults are the rule.  numpy only."""
import heapq

import numpy as np

DC = (1, 1, 0, -1, -1, -1, 0, 1)                              # k = 0 .. 7: E, SE, S, SW, W, NW, N, NE; columns east, rows south
DR = (0, 1, 1, 1, 0, -1, -1, -1)
MAX_Z = 32768.0
INVALID_KEY = np.uint64(0xffffffffffffffff)
ROOT, VOID = -1, -2                                           # receivers: a cell index, ROOT, or VOID for a cell without a code


# ---- cells, heights ------------------------------------------------------------------------------------------------------------
def valid(z, nodata=-999.0):
    z = np.asarray(z, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(z) & (z != np.float32(nodata)) & (np.abs(z) <= np.float32(MAX_Z))


def quanta(z, nodata=-999.0):
    """q = llrint((double)z * 256), halves to even, int64; 0 where invalid."""
    v = valid(z, nodata)
    return np.where(v, np.rint(np.where(v, z, 0).astype(np.float64) * 256.0), 0).astype(np.int64)


def outlets(v):
    """Valid cells with a neighbour off the grid or invalid."""
    gh, gw = v.shape
    p = np.zeros((gh + 2, gw + 2), bool)
    p[1:-1, 1:-1] = v
    ring = np.ones_like(v)
    for k in range(8):
        ring &= p[1 + DR[k]:1 + DR[k] + gh, 1 + DC[k]:1 + DC[k] + gw]
    return v & ~ring


def pack(w, d, v):
    """(w, d) -> the device's uint64 words; invalid cells all ones."""
    key = ((w.astype(np.int64) + 2 ** 31).astype(np.uint64) << np.uint64(32)) | d.astype(np.int64).astype(np.uint64)
    return np.where(v, key, INVALID_KEY)


def unpack(keys):
    keys = np.ascontiguousarray(keys).view(np.uint64)
    v = keys != INVALID_KEY
    w = np.where(v, (keys >> np.uint64(32)).astype(np.int64) - 2 ** 31, 0)
    d = np.where(v, (keys & np.uint64(0xffffffff)).astype(np.int64), -1)
    return w, d, v


# ---- keys: a heap flood on Python ints ---------------------------------------------------------------------------------------------
def keys_heap(z, nodata=-999.0, neighbours=8, reset_d=True, void_outlets=True):
    """Dijkstra from the outlets over pairs (w, d): -> w, d int64 (0 and -1 where invalid), valid mask.
    Planted errors: neighbours=4 floods through E, S, W, N only; reset_d=False carries d over a rise; void_outlets=False takes
    voids as walls, so that only the grid's edge lets water out."""
    v = valid(z, nodata)
    q = quanta(z, nodata)
    gh, gw = v.shape
    ks = range(8) if neighbours == 8 else (0, 2, 4, 6)
    out = outlets(v if void_outlets else np.ones_like(v)) & v
    w = np.zeros((gh, gw), np.int64)
    d = np.full((gh, gw), -1, np.int64)
    best, heap = {}, []
    for r, c in zip(*np.nonzero(out)):
        best[(r, c)] = (int(q[r, c]), 0)
        heap.append((int(q[r, c]), 0, int(r), int(c)))
    heapq.heapify(heap)
    done = np.zeros((gh, gw), bool)
    while heap:
        kw, kd, r, c = heapq.heappop(heap)
        if done[r, c]:
            continue
        done[r, c] = True
        w[r, c], d[r, c] = kw, kd
        for k in ks:
            rr, cc = r + DR[k], c + DC[k]
            if not (0 <= rr < gh and 0 <= cc < gw) or not v[rr, cc] or done[rr, cc] or out[rr, cc]:
                continue
            qn = int(q[rr, cc])
            if reset_d:
                cand = max((qn, 0), (kw, kd + 1))
            else:
                cand = (max(qn, kw), kd + 1)
            if cand < best.get((rr, cc), (2 ** 62, 0)):
                best[(rr, cc)] = cand
                heapq.heappush(heap, (cand[0], cand[1], rr, cc))
    return w, d, v


# ---- keys: synchronous numpy sweeps to the fixed point ---------------------------------------------------------------------------
def keys_sweeps(z, nodata=-999.0, return_sweeps=False):
    """K <- min(K, max((q, 0), min over the neighbours of K + 1)) on all cells at once, from +infinity, until nothing moves.
    A key is the int64 w 2^32 + d here."""
    v = valid(z, nodata)
    q = quanta(z, nodata)
    gh, gw = v.shape
    out = outlets(v)
    inf = np.int64(2 ** 62)
    floor = q << 32
    key = np.where(out, floor, inf)
    open_ = v & ~out
    sweeps = 0
    while True:
        p = np.full((gh + 2, gw + 2), inf, np.int64)
        p[1:-1, 1:-1] = key
        low = np.full((gh, gw), inf, np.int64)
        for k in range(8):
            low = np.minimum(low, p[1 + DR[k]:1 + DR[k] + gh, 1 + DC[k]:1 + DC[k] + gw])
        new = np.where(open_, np.minimum(key, np.maximum(floor, low + 1)), key)
        sweeps += 1
        if np.array_equal(new, key):
            break
        key = new
    assert not (v & (key >= inf)).any()
    w, d = np.where(v, key >> 32, 0), np.where(v, key & 0xffffffff, -1)
    return (w, d, v, sweeps) if return_sweeps else (w, d, v)


def filled_of(z, w, d, v, nodata=-999.0):
    """filled, depth float32 and flat_dist int32 of the keys."""
    z = np.asarray(z, np.float32)
    q = quanta(z, nodata)
    nd = np.float32(nodata)
    filled = np.where(v, np.where(w == q, z, (w / 256.0).astype(np.float32)), nd).astype(np.float32)
    depth = np.where(v, ((w - q) / 256.0).astype(np.float32), nd).astype(np.float32)
    return filled, depth, np.where(v, d, -1).astype(np.int32)


# ---- directions --------------------------------------------------------------------------------------------------------------------
def distances(xres, yres, diagonal=None):
    h = float(np.hypot(xres, yres)) if diagonal is None else float(diagonal)
    return [float(xres), h, float(yres), h, float(xres), h, float(yres), h]


def directions_loop(w, d, v, dist, steepest=True, low_ties=True):
    """The text, cell by cell.  Planted errors: steepest=False takes the lowest neighbour whatever its distance; low_ties=False
    lets the highest k win a tie."""
    gh, gw = v.shape
    code = np.full((gh, gw), 255, np.uint8)
    for r in range(gh):
        for c in range(gw):
            if not v[r, c]:
                continue
            near = []
            for k in range(8):
                rr, cc = r + DR[k], c + DC[k]
                near.append((k, int(w[rr, cc]), int(d[rr, cc])) if 0 <= rr < gh and 0 <= cc < gw and v[rr, cc] else None)
            if None in near:
                code[r, c] = 0
                continue
            wc = int(w[r, c])
            lower = [(float(wc - wn) / dist[k] if steepest else float(wc - wn), k) for k, wn, _ in near if wn < wc]
            if lower:
                top = max(s for s, _ in lower)
                ks = [k for s, k in lower if s == top]
            else:
                level = [(dn, k) for k, wn, dn in near if wn == wc]
                if not level:
                    code[r, c] = 0
                    continue
                top = min(dn for dn, _ in level)
                ks = [k for dn, k in level if dn == top]
            code[r, c] = (min(ks) if low_ties else max(ks)) + 1
    return code


def directions_arrays(w, d, v, dist):
    gh, gw = v.shape
    big = np.int64(2 ** 62)
    pw = np.zeros((gh + 2, gw + 2), np.int64); pd = np.zeros_like(pw); pv = np.zeros((gh + 2, gw + 2), bool)
    pw[1:-1, 1:-1], pd[1:-1, 1:-1], pv[1:-1, 1:-1] = w, d, v
    sl = [(slice(1 + DR[k], 1 + DR[k] + gh), slice(1 + DC[k], 1 + DC[k] + gw)) for k in range(8)]
    wn = np.stack([pw[s] for s in sl]); dn = np.stack([pd[s] for s in sl]); vn = np.stack([pv[s] for s in sl])
    drop = (w[None] - wn).astype(np.float64) / np.asarray(dist, np.float64)[:, None, None]
    slope = np.where(wn < w[None], drop, -1.0)
    steep = np.argmax(slope, axis=0)                          # the first of equal maxima: the lowest k
    flat = np.argmin(np.where(wn == w[None], dn, big), axis=0)
    some_level = (wn == w[None]).any(axis=0)
    code = np.where(slope.max(axis=0) > 0.0, steep + 1, np.where(some_level, flat + 1, 0))
    code = np.where(vn.all(axis=0), code, 0)
    return np.where(v, code, 255).astype(np.uint8)


# ---- receivers, roots and cycles of any code grid ----------------------------------------------------------------------------------
def receivers(code, pour=None):
    """flat int64: the cell a code sends its cell to, ROOT, or VOID (codes 9 .. 255).  Pour cells with a code are roots."""
    code = np.asarray(code, np.uint8)
    gh, gw = code.shape
    recv = np.full(gh * gw, VOID, np.int64)
    for r in range(gh):
        for c in range(gw):
            k = int(code[r, c])
            if k > 8:
                continue
            i = r * gw + c
            recv[i] = ROOT
            if k == 0 or (pour is not None and pour[r, c]):
                continue
            rr, cc = r + DR[k - 1], c + DC[k - 1]
            if 0 <= rr < gh and 0 <= cc < gw and code[rr, cc] <= 8:
                recv[i] = rr * gw + cc
    return recv


def receivers_arrays(code, pour=None):
    code = np.asarray(code, np.uint8)
    gh, gw = code.shape
    r, c = np.mgrid[:gh, :gw]
    k = np.minimum(code, 8).astype(np.int64) - 1
    rr, cc = r + np.asarray(DR)[k], c + np.asarray(DC)[k]
    on = (rr >= 0) & (rr < gh) & (cc >= 0) & (cc < gw)
    target = np.where(on, rr * gw + cc, 0)
    on &= code.reshape(-1)[target] <= 8
    root = (code == 0) | ~on
    if pour is not None:
        root |= np.asarray(pour) != 0
    return np.where(code > 8, VOID, np.where(root, ROOT, target)).reshape(-1).astype(np.int64)


def roots_walk(recv):
    """The root of every cell by walking: a cell index, -1 for a cell on a cycle or draining into one, -2 for VOID."""
    n = recv.size
    root = np.full(n, -3, np.int64)
    for i in range(n):
        if root[i] != -3:
            continue
        if recv[i] == VOID:
            root[i] = -2
            continue
        path, at = [], i
        on_path = set()
        while True:
            if root[at] != -3:
                end = root[at]
                break
            if at in on_path:
                end = -1
                break
            path.append(at)
            on_path.add(at)
            if recv[at] == ROOT:
                end = at
                break
            at = recv[at]
        for p in path:
            root[p] = end
    return root


def roots_doubling(recv):
    """The same by squaring the pointers ceil(log2 n) + 1 times."""
    n = recv.size
    up = np.where(recv >= 0, recv, np.arange(n))
    for _ in range(int(np.ceil(np.log2(max(n, 1)))) + 1):
        up = up[up]
    return np.where(recv == VOID, -2, np.where(recv[up] == ROOT, up, -1))


# ---- accumulation ------------------------------------------------------------------------------------------------------------------
def _weights(weight, n):
    return [1] * n if weight is None else [int(x) for x in np.asarray(weight).reshape(-1)]


def _wrap(x):
    return (int(x) + 2 ** 63) % 2 ** 64 - 2 ** 63


def accumulate_by_keys(code, w, d, weight=None, own=True, arrays=False):
    """Cells visited in falling key order, each handing its sum to its receiver (the directions of a flood never cycle).
    Planted error: own=False leaves the cell itself out."""
    gh, gw = code.shape
    recv = receivers_arrays(code) if arrays else receivers(code)
    wt = _weights(weight, gh * gw)
    acc = [(wt[i] if own and recv[i] != VOID else 0) for i in range(gh * gw)]
    order = np.lexsort((-d.reshape(-1), -w.reshape(-1)))
    for i in order:
        if recv[i] >= 0:
            acc[recv[i]] += acc[i] + (0 if own else wt[i])
    return np.array([_wrap(a) for a in acc], np.int64).reshape(gh, gw)


def accumulate_subtrees(code, weight=None):
    """acc(c) = weight(c) + the sum over the cells that drain into c of acc, from the roots down, on any code grid (a stack
    stands for the recursion, which a long river would overflow); -1 for cells without a root.  -> acc, whether any was cyclic."""
    gh, gw = code.shape
    n = gh * gw
    recv = receivers(code)
    root = roots_walk(recv)
    wt = _weights(weight, n)
    children = [[] for _ in range(n)]
    for i in range(n):
        if recv[i] >= 0 and root[i] >= 0:
            children[recv[i]].append(i)
    acc = [0] * n
    for top in range(n):
        if recv[top] != ROOT:
            continue
        stack = [(top, 0)]
        while stack:
            node, at = stack.pop()
            if at == 0:
                acc[node] = wt[node]
            if at < len(children[node]):
                stack.append((node, at + 1))
                stack.append((children[node][at], 0))
            elif recv[node] >= 0:
                acc[recv[node]] += acc[node]
    cyclic = root == -1
    out = np.array([_wrap(a) for a in acc], np.int64)
    return np.where(cyclic, -1, out).reshape(gh, gw), bool(cyclic.any())


def accumulate_peel(code, weight=None):
    """The same by peeling leaves (in-degrees), on any code grid."""
    gh, gw = code.shape
    n = gh * gw
    recv = receivers_arrays(code)
    root = roots_doubling(recv)
    wt = _weights(weight, n)
    tree = root >= 0
    indeg = np.zeros(n, np.int64)
    np.add.at(indeg, recv[tree & (recv >= 0)], 1)
    acc = [wt[i] if tree[i] else 0 for i in range(n)]
    ready = [i for i in range(n) if tree[i] and indeg[i] == 0]
    while ready:
        i = ready.pop()
        p = recv[i]
        if p >= 0:
            acc[p] += acc[i]
            indeg[p] -= 1
            if indeg[p] == 0:
                ready.append(p)
    out = np.array([_wrap(a) for a in acc], np.int64)
    return np.where(root == -1, -1, out).reshape(gh, gw), bool((root == -1).any())


# ---- basins ------------------------------------------------------------------------------------------------------------------------
def basins_walk(code, pour=None):
    """-> labels int32, n, whether any cell was cyclic: a walk to the root, the roots numbered in row-major order."""
    gh, gw = code.shape
    recv = receivers(code, pour)
    root = roots_walk(recv)
    numbered = recv == ROOT
    if pour is not None:
        numbered &= np.asarray(pour).reshape(-1) != 0
    number = np.cumsum(numbered) * numbered
    lab = np.where(root >= 0, number[np.maximum(root, 0)], 0)
    return lab.reshape(gh, gw).astype(np.int32), int(numbered.sum()), bool((root == -1).any())


def basins_arrays(code, pour=None):
    gh, gw = code.shape
    recv = receivers_arrays(code, pour)
    root = roots_doubling(recv)
    numbered = recv == ROOT
    if pour is not None:
        numbered &= np.asarray(pour).reshape(-1) != 0
    number = np.cumsum(numbered) * numbered
    lab = np.where(root >= 0, number[np.maximum(root, 0)], 0)
    return lab.reshape(gh, gw).astype(np.int32), int(numbered.sum()), bool((root == -1).any())


# ---- the whole chain, and the comparison the GPU tests make ------------------------------------------------------------------------
def chain(z, xres=5.0, yres=5.0, nodata=-999.0, weight=None, arrays=False, **planted):
    """Everything the device computes from a DSM, by the loop statements: a dict of arrays.  `planted` takes the switches of
    keys_heap, directions_loop, accumulate_by_keys and `diagonal` (the diagonal step length).  arrays=True takes the array
    statements of the directions, receivers and basins instead (the same values, test_dsm_hydro_cpu.py; quicker on large grids)."""
    kk = {k: planted[k] for k in ("neighbours", "reset_d", "void_outlets") if k in planted}
    dk = {k: planted[k] for k in ("steepest", "low_ties") if k in planted}
    z = np.asarray(z, np.float32)
    w, d, v = keys_heap(z, nodata, **kk)
    filled, depth, flat = filled_of(z, w, d, v, nodata)
    dist = distances(xres, yres, planted.get("diagonal"))
    code = directions_arrays(w, d, v, dist) if arrays else directions_loop(w, d, v, dist, **dk)
    acc = accumulate_by_keys(code, w, d, weight, own=planted.get("own", True), arrays=arrays)
    lab, n, _ = (basins_arrays if arrays else basins_walk)(code)
    return {"keys": pack(w, d, v), "filled": filled, "depth": depth, "flat_dist": flat, "dir": code, "acc": acc, "basin": lab,
            "n": np.int64(n)}


def differing(got, want):
    """The names of the outputs that differ: bits for floats (np.array_equal on their uint32 images), values otherwise, no cell
    excused.  The GPU tests assert that this is empty."""
    bad = []
    for name in want:
        a, b = np.asarray(got[name]), np.asarray(want[name])
        if a.dtype == np.float32 and b.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(a, b):
            bad.append(name)
    return bad


# ---- scenes the CPU and GPU tests share --------------------------------------------------------------------------------------------
def hills(gh, gw, seed, voids=0.0, levels=None):
    """dsm_testkit.scene with salt noise (pits and spikes) and a share of voids (NaN and nodata mixed).  With `levels` the
    heights are drawn from that many values, a tenth of the cells at random, so that flats and ties abound."""
    import dsm_testkit as tk
    rng = np.random.default_rng(seed + 1000)                  # not the scene's own stream, whose first draw places the salt
    c, r = np.meshgrid(np.arange(gw) * 5.0, -np.arange(gh) * 5.0)
    z = tk.scene(c, r, blocks=True, holes=False, seed=seed, salt=0.03)
    if levels:
        step = np.clip(np.round((z - 110.0) / 40.0 * (levels - 1)), 0, levels - 1)
        anew = rng.random((gh, gw)) < 0.1
        step[anew] = rng.integers(0, levels, (gh, gw))[anew]
        z = (100.0 + 0.75 * step).astype(np.float32)
    gone = rng.random((gh, gw)) < voids
    z[gone] = np.where(rng.random((gh, gw)) < 0.5, np.float32(np.nan), np.float32(-999.0))[gone]
    return z


def crater(n):
    """A raised rim round a flat floor: one basin as large as the grid, filled in one flat, d up to about half the side."""
    z = np.full((n, n), 100.0, np.float32)
    z[1:-1, 1:-1] = 90.0
    z[0, :] = z[-1, :] = z[:, 0] = z[:, -1] = 95.0
    z[2:-2, 2:-2] = 80.0
    return z


def serpentine(gh, gw):
    """Walls at 200 m and a channel that runs along every second row, turning at alternate ends and falling by 2^-8 m a cell
    towards its mouth in the top left corner: the flow path passes every channel cell, the deepest tree a grid of this size has."""
    z = np.full((gh, gw), 200.0, np.float32)
    path = []
    rows = list(range(1, gh - 1, 2))
    for j, r in enumerate(rows):
        cols = list(range(1, gw - 1))
        if j % 2:
            cols.reverse()
        path += [(r, c) for c in cols]
        if j + 1 < len(rows):
            path.append((r + 1, cols[-1]))
    path.insert(0, (1, 0))                                    # the mouth, on the grid's edge
    for step, (r, c) in enumerate(path):
        z[r, c] = np.float32(10.0 + step / 256.0)
    return z, path


def comb(gh, gw):
    """Parallel channels running south into one collector along the bottom, which runs east to its mouth."""
    z = np.full((gh, gw), 150.0, np.float32)
    for c in range(1, gw - 1, 2):
        z[1:gh - 2, c] = (60.0 + np.arange(gh - 3, 0, -1) / 256.0 + (gw - c) / 64.0).astype(np.float32)
    z[gh - 2, 1:] = (20.0 + np.arange(gw - 1, 0, -1) / 256.0).astype(np.float32)
    return z


# (gh, gw, seed, share of voids, levels) of the random hills both test files run; xres, yres = 5 m, 2.5 m throughout, where the
# steepest neighbour differs from the square-cell one
RANDOM_CASES = [(40, 50, 1, 0.0, None), (40, 50, 2, 0.05, None), (40, 50, 3, 0.3, None),
                (37, 45, 4, 0.0, 12), (37, 45, 5, 0.05, 12), (37, 45, 6, 0.3, 12)]
XRES, YRES = 5.0, 2.5
