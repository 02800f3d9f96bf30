"""The stream-network rule of include/satmvs.h ("Stream network") in Python, every part stated twice: a loop after the text on
Python ints, and arrays.  The two statements are held against each other in test_dsm_stream_cpu.py and the device against one
of them in test_dsm_stream_gpu.py.  The switches (any_two, shreve, four, gaps, heads_two, junction, by_mouth, diagonal_ew)
plant the errors the GPU file's comparison has to report; their defaults are the rule.  Receivers and cycles come from
dsm_hydro_oracle.  numpy only."""
import functools

import numpy as np

import dsm_hydro_oracle as ho

KEYS = ("order_map", "link", "head", "order", "next_link", "offset", "vertices", "steps")


# ---- the induced forest --------------------------------------------------------------------------------------------------------
def induced(code, mask, four=False, gaps=True):
    """-> in_s (flat bool), down (flat int64, -1 where a cell of S has no receiver in S and outside S), whether the grid holds a
    cyclic cell.  Planted errors: four=True lets only E, S, W, N steps flow into a cell; gaps=False takes every tree cell for
    a stream cell (the mask's gaps ignored: full-forest receivers)."""
    code = np.asarray(code, np.uint8)
    recv = ho.receivers_arrays(code)
    root = ho.roots_doubling(recv)
    in_s = root >= 0
    if gaps:
        in_s = in_s & (np.asarray(mask).reshape(-1) != 0)
    down = np.where(in_s & (recv >= 0) & in_s[np.maximum(recv, 0)], recv, -1)
    if four:
        down = np.where(code.reshape(-1) % 2 == 1, down, -1)
    return in_s, down, bool((root == -1).any())


def inflow(in_s, down):
    return np.bincount(down[down >= 0], minlength=in_s.size)


def step_kind(code):
    """0 E-W, 1 N-S, 2 diagonal for the codes 1 .. 8."""
    code = np.asarray(code, np.int64)
    return np.where(code % 2 == 0, 2, ((code - 1) // 2) % 2)


# ---- order -----------------------------------------------------------------------------------------------------------------------
def order_peel(in_s, down, any_two=False, shreve=False):
    """(a) The text, cells taken in the order of a peel by in-degree.  Planted errors: any_two=True gives m + 1 for any two
    inflows; shreve=True adds the inflowing orders up."""
    n = in_s.size
    indeg = inflow(in_s, down)
    left = indeg.copy()
    order = np.zeros(n, np.int64)
    best, count, total = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    ready = [int(i) for i in np.nonzero(in_s & (indeg == 0))[0]]
    while ready:
        i = ready.pop()
        if indeg[i] == 0:
            order[i] = 1
        elif shreve:
            order[i] = total[i]
        elif any_two:
            order[i] = best[i] + 1 if indeg[i] >= 2 else best[i]
        else:
            order[i] = best[i] + 1 if count[i] >= 2 else best[i]
        d = int(down[i])
        if d >= 0:
            total[d] += order[i]
            if order[i] > best[d]:
                best[d], count[d] = order[i], 1
            elif order[i] == best[d]:
                count[d] += 1
            left[d] -= 1
            if left[d] == 0:
                ready.append(d)
    return order


def depth(down):
    """Steps to the mouth along down, by doubling."""
    n = down.size
    ptr = np.where(down >= 0, down, np.arange(n))
    d = (down >= 0).astype(np.int64)
    for _ in range(int(np.ceil(np.log2(max(n, 2))))):
        d = d + d[ptr]
        ptr = ptr[ptr]
    return d


def subtree_sums(down, value, dep):
    """The sum of value over every cell and everything that flows into it: levels from the deepest up."""
    total = value.astype(np.int64).copy()
    cells = np.nonzero(down >= 0)[0]
    cells = cells[np.argsort(-dep[cells], kind="stable")]
    if cells.size:
        d = dep[cells]
        cuts = np.nonzero(np.diff(d))[0] + 1
        for level in np.split(cells, cuts):
            np.add.at(total, down[level], total[level])
    return total


def order_sets(in_s, down):
    """(b) A_1 = S; A_{k+1} = the cells with a cell of J_k in their subtree (themselves included), J_k = the cells with two
    inflowing cells in A_k; order = the greatest k with the cell in A_k."""
    order = in_s.astype(np.int64)
    dep = depth(down)
    k = 1
    while True:
        a_k = order >= k
        feeders = np.bincount(down[a_k & (down >= 0)], minlength=in_s.size)
        j_k = a_k & (feeders >= 2)
        if not j_k.any():
            return order
        order[subtree_sums_up(down, j_k, dep) > 0] = k + 1
        k += 1


def subtree_sums_up(down, marks, dep):
    """For every cell the number of marked cells in its subtree (upstream of it, itself included)."""
    return subtree_sums(down, marks.astype(np.int64), dep)


# ---- links -----------------------------------------------------------------------------------------------------------------------
def links_walk(code, in_s, down, order, heads_two=False, junction=True, by_mouth=False, diagonal_ew=False):
    """(a) A walk from every head after the text.  Planted errors: heads_two=True starts links at junctions only; junction=False
    leaves the closing vertex off; by_mouth=True numbers the links by their last cell; diagonal_ew=True counts diagonal
    steps as E-W."""
    code = np.asarray(code, np.uint8)
    gh, gw = code.shape
    flat = code.reshape(-1)
    indeg = inflow(in_s, down)
    heads = [int(i) for i in np.nonzero(in_s & ((indeg >= 2) if heads_two else (indeg != 1)))[0]]
    walked = []
    for h in heads:
        cells = [h]
        while down[cells[-1]] >= 0 and indeg[down[cells[-1]]] == 1:
            cells.append(int(down[cells[-1]]))
        walked.append(cells)
    if by_mouth:
        walked.sort(key=lambda cells: cells[-1])
    number = {cells[0]: k for k, cells in enumerate(walked)}
    link = np.zeros(gh * gw, np.int32)
    head, link_order, next_link, offset, vertices, steps = [], [], [], [0], [], []
    for k, cells in enumerate(walked):
        link[cells] = k + 1
        head.append(cells[0])
        link_order.append(int(order[cells[0]]))
        end = int(down[cells[-1]])
        next_link.append(number.get(end, -1) if end >= 0 else -1)
        points = cells + ([end] if end >= 0 and junction else [])
        vertices += [(p % gw, p // gw) for p in points]
        offset.append(len(vertices))
        count = [0, 0, 0]
        for c in cells:
            if down[c] >= 0:
                kind = int(step_kind(flat[c]))
                count[0 if diagonal_ew and kind == 2 else kind] += 1
        steps.append(count)
    return {"link": link.reshape(gh, gw), "head": np.array(head, np.int32), "order": np.array(link_order, np.int32),
            "next_link": np.array(next_link, np.int32), "offset": np.array(offset, np.int32),
            "vertices": np.array(vertices, np.int32).reshape(-1, 2), "steps": np.array(steps, np.int32).reshape(-1, 3)}


def links_arrays(code, in_s, down, order):
    """(b) Arrays: head flags, a cumulative numbering, the head of every cell by doubling "the one cell flowing into me",
    positions from depth differences."""
    code = np.asarray(code, np.uint8)
    gh, gw = code.shape
    n = gh * gw
    cell = np.arange(n)
    indeg = inflow(in_s, down)
    is_head = in_s & (indeg != 1)
    number = np.cumsum(is_head) - 1                           # at a head: its link
    nl = int(is_head.sum())
    feeder = np.full(n, -1, np.int64)
    feeder[down[down >= 0]] = cell[down >= 0]                 # the one inflowing cell where in = 1 (any of them elsewhere: unused)
    ptr = np.where(in_s & ~is_head, feeder, cell)
    for _ in range(int(np.ceil(np.log2(max(n, 2)))) + 1):
        ptr = ptr[ptr]
    dep = depth(down)
    at = dep[ptr] - dep                                       # position in the link
    of = np.where(in_s, number[ptr], -1)
    s = np.nonzero(in_s)[0]
    ends = s[(down[s] < 0) | (indeg[np.maximum(down[s], 0)] >= 2)]
    closing = down[ends] >= 0
    length = np.zeros(nl, np.int64)
    length[of[ends]] = at[ends] + 1 + closing
    offset = np.concatenate([[0], np.cumsum(length)])
    vertices = np.zeros((int(offset[-1]), 2), np.int32)
    vertices[offset[of[s]] + at[s]] = np.stack([s % gw, s // gw], axis=1)
    e = ends[closing]
    vertices[offset[of[e]] + at[e] + 1] = np.stack([down[e] % gw, down[e] // gw], axis=1)
    next_link = np.full(nl, -1, np.int32)
    next_link[of[e]] = number[down[e]]
    steps = np.zeros((nl, 3), np.int32)
    flows = s[down[s] >= 0]
    np.add.at(steps, (of[flows], step_kind(code.reshape(-1)[flows])), 1)
    head = np.nonzero(is_head)[0].astype(np.int32)
    return {"link": (of + 1).astype(np.int32).reshape(gh, gw), "head": head, "order": order[head].astype(np.int32), "next_link": next_link,
            "offset": offset.astype(np.int32), "vertices": vertices, "steps": steps}


def network(code, mask, arrays=True, **planted):
    """Everything stream_links() gives without a grid, plus counts (stream cells, links, vertices, highest order) and cyclic.
    arrays=True takes the (b) statements (quick on large grids) and no planted error; arrays=False the loops."""
    code = np.asarray(code, np.uint8)
    ik = {k: planted[k] for k in ("four", "gaps") if k in planted}
    ok = {k: planted[k] for k in ("any_two", "shreve") if k in planted}
    lk = {k: planted[k] for k in ("heads_two", "junction", "by_mouth", "diagonal_ew") if k in planted}
    assert not (arrays and planted)
    in_s, down, cyclic = induced(code, mask, **ik)
    if arrays:
        order = order_sets(in_s, down)
        out = links_arrays(code, in_s, down, order)
    else:
        order = order_peel(in_s, down, **ok)
        out = links_walk(code, in_s, down, order, **lk)
    out["order_map"] = order.astype(np.uint8).reshape(code.shape)
    out["counts"] = np.array([in_s.sum(), len(out["head"]), len(out["vertices"]), order.max() if order.size else 0], np.int64)
    out["cyclic"] = cyclic
    return out


def length_m(steps, xres, yres):
    """(n_ew xres + n_ns yres) + n_diag hypot(xres, yres) in float64, in exactly that order."""
    s = np.asarray(steps).astype(np.float64)
    return (s[..., 0] * float(xres) + s[..., 1] * float(yres)) + s[..., 2] * float(np.hypot(float(xres), float(yres)))


# ---- flow length -----------------------------------------------------------------------------------------------------------------
def flow_length_walk(code, diagonal_ew=False):
    """(a) A walk to the root from every cell (memoised along the path) -> int32 (gh, gw, 3), whether any cell was cyclic."""
    code = np.asarray(code, np.uint8)
    gh, gw = code.shape
    recv = ho.receivers(code)
    root = ho.roots_walk(recv)
    flat = code.reshape(-1)
    out = np.full((gh * gw, 3), -1, np.int64)
    for i in range(gh * gw):
        if root[i] < 0 or out[i, 0] >= 0:
            continue
        path, at = [], i
        while out[at, 0] < 0 and recv[at] >= 0:
            path.append(at)
            at = int(recv[at])
        if out[at, 0] < 0:
            out[at] = 0                                       # the root
        for p in reversed(path):
            kind = int(step_kind(flat[p]))
            out[p] = out[recv[p]]
            out[p, 0 if diagonal_ew and kind == 2 else kind] += 1
    return out.astype(np.int32).reshape(gh, gw, 3), bool((root == -1).any())


def flow_length_doubling(code):
    """(b) Pointer doubling with the three counts as sums."""
    code = np.asarray(code, np.uint8)
    gh, gw = code.shape
    n = gh * gw
    recv = ho.receivers_arrays(code)
    root = ho.roots_doubling(recv)
    moves = recv >= 0
    ptr = np.where(moves, recv, np.arange(n))
    sums = np.zeros((n, 3), np.int64)
    sums[np.nonzero(moves)[0], step_kind(code.reshape(-1)[moves])] = 1
    for _ in range(int(np.ceil(np.log2(max(n, 2))))):
        sums = sums + sums[ptr]
        ptr = ptr[ptr]
    sums[root < 0] = -1
    return sums.astype(np.int32).reshape(gh, gw, 3), bool((root == -1).any())


# ---- the comparison the GPU tests make -----------------------------------------------------------------------------------------
def differing(got, want):
    """One line per output of `want` that differs from `got`'s, naming the first entry that does: dtype, shape, then values
    (floats by their bits), no entry excused.  The GPU tests assert that this is empty."""
    bad = []
    for name in want:
        if name not in got:
            bad.append("%s: missing" % name)
            continue
        a, b = np.asarray(got[name]), np.asarray(want[name])
        if a.dtype != b.dtype or a.shape != b.shape:
            bad.append("%s: %s %s, want %s %s" % (name, a.dtype, a.shape, b.dtype, b.shape))
            continue
        if a.dtype.kind == "f":
            a, b = a.view("u%d" % a.dtype.itemsize), b.view("u%d" % b.dtype.itemsize)
        if not np.array_equal(a, b):
            at = tuple(int(x) for x in np.argwhere(a != b)[0]) if a.ndim else ()
            bad.append("%s%s: %s, want %s" % (name, list(at), a[at], b[at]))
    return bad


# ---- scenes the CPU and GPU tests share ----------------------------------------------------------------------------------------
def code_of(z, xres=ho.XRES, yres=ho.YRES):
    """The directions and accumulation of a DSM by the hydrology oracle's array statements."""
    z = np.asarray(z, np.float32)
    w, d, v = ho.keys_heap(z)
    code = ho.directions_arrays(w, d, v, ho.distances(xres, yres))
    acc, _ = ho.accumulate_peel(code)
    return code, acc


RANDOM_SCENES = list(ho.RANDOM_CASES) + [(257, 301, 7, 0.05, None)]
SIZES = [(1, 1), (1, 70), (67, 1), (2, 2), (67, 3), (31, 31), (32, 32), (33, 33), (31, 33), (33, 31), (11, 93), (25, 41)]     # the last two and 32 x 32: 1023, 1025, 1024 cells


@functools.lru_cache(maxsize=None)
def hill_codes(gh, gw, seed, voids, levels):
    """(code, acc) of ho.hills at 5 m x 2.5 m, computed once for all tests of a process; treat them as read-only."""
    return code_of(ho.hills(gh, gw, seed, voids, levels))


def masks_of(code, acc, seed=0):
    """The masks every random scene runs: three thresholds, a random half (gaps cut the network), all ones, all zeros."""
    rng = np.random.default_rng(seed)
    return [("acc >= 1", acc >= 1), ("acc >= 4", acc >= 4), ("acc >= 50", acc >= 50), ("a random half", rng.random(code.shape) < 0.5),
            ("all ones", np.ones(code.shape, bool)), ("all zeros", np.zeros(code.shape, bool))]


def first_tree_cells(code, count):
    """A mask of the first `count` tree cells in row-major order."""
    tree = ho.roots_doubling(ho.receivers_arrays(code)) >= 0
    return (tree & (np.cumsum(tree) <= count)).reshape(code.shape)


def cyclic_grid():
    """The hydrology tests' edited grid: a 2-cycle, a ring of 60 cells round a block, trees draining into the ring, codes 9 and
    254, targets off the grid and on a void; the rest drains to the cell below or off the bottom edge."""
    gh, gw = 40, 47
    code = np.full((gh, gw), 3, np.uint8)
    code[5, 5], code[5, 6] = 1, 5
    code[10, 10:30], code[10:20, 30], code[20, 11:31], code[11:21, 10] = 1, 3, 5, 7
    code[2:10, 15] = 3
    code[15, 11:30] = 1
    code[30, 3], code[30, 4], code[31, 3] = 9, 254, 255
    code[0, 0], code[0, gw - 1], code[gh - 1, 0] = 7, 8, 4
    code[29, 4] = 3
    return code


def serpentine_codes(gh, gw):
    """ho.serpentine's channel as hand-made codes: every channel cell points at the one before it on the path, the mouth has
    code 0 and the walls none.  (The D8 directions of the heights cut the corners of the turns.)  -> code, the path from the mouth."""
    _, path = ho.serpentine(gh, gw)
    code = np.full((gh, gw), 255, np.uint8)
    code[path[0]] = 0
    for (r0, c0), (r1, c1) in zip(path[:-1], path[1:]):
        code[r1, c1] = 1 + [k for k in range(8) if (ho.DR[k], ho.DC[k]) == (r0 - r1, c0 - c1)][0]
    return code, path


def htree(levels):
    """A complete binary tree of `levels` levels of junctions laid out as an H-tree of direction codes: the root in the middle
    flows off to nowhere (code 0); every junction has two arms of 2^j cells that end in the next junctions, alternately
    horizontal and vertical; the leaves are sources.  -> code (uint8, 255 off the tree), the root's cell (row, col)."""
    half = [2 ** ((levels - j + 1) // 2) for j in range(1, levels + 1)]       # arm lengths, root's first
    size = 2 * sum(half) + 1
    code = np.full((size, size), 255, np.uint8)
    mid = size // 2
    code[mid, mid] = 0

    def grow(r, c, j):
        if j == levels:
            return
        arm = half[j]
        for sign in (-1, 1):
            horizontal = j % 2 == 0
            for step in range(1, arm + 1):
                rr, cc = (r, c + sign * step) if horizontal else (r + sign * step, c)
                code[rr, cc] = (5 if sign > 0 else 1) if horizontal else (7 if sign > 0 else 3)          # back towards (r, c)
            grow(rr, cc, j + 1)

    grow(mid, mid, 0)
    return code, (mid, mid)


def junction_codes():
    """Hand-made grids of the closed forms: name -> (code, the cell to look at, its order)."""
    out = {}
    # three order-2 tributaries (each the join of two sources) meet in one cell: 3, not 4
    code = np.full((9, 9), 255, np.uint8)
    code[4, 4] = 3
    code[5:8, 4] = 3
    code[8, 4] = 0
    code[4, 1:4] = 1                                          # from the west: a stem of three cells ...
    code[3, 1], code[5, 1] = 2, 8                             # ... whose second cell takes two more sources: order 2
    code[1:4, 4] = 3                                          # from the north
    code[1, 3], code[1, 5] = 1, 5
    code[4, 5:8] = 5                                          # from the east
    code[3, 7], code[5, 7] = 4, 6
    out["three of order 2"] = (code, (4, 4), 3)
    # order 2 meets order 1: stays 2
    code = np.full((7, 7), 255, np.uint8)
    code[3, 1:6] = 1
    code[3, 6] = 0
    code[2, 1], code[4, 1] = 2, 8                             # two more sources into (3, 2), SE and NE: order 2 from there on
    code[2, 4] = 3                                            # a lone source into (3, 4)
    out["order 2 with order 1"] = (code, (3, 4), 2)
    # a mouth with eight inflowing stream cells, all sources: the mouth has order 2 and is a one-vertex link
    code = np.full((5, 5), 255, np.uint8)
    code[2, 2] = 0
    for k in range(8):
        code[2 - ho.DR[k], 2 - ho.DC[k]] = k + 1
    out["a mouth with eight inflows"] = (code, (2, 2), 2)
    return out
