"""The seeded flood of include/satmvs.h ("Seeded flood") in Python, the keys stated twice: a heapq Dijkstra from the seeds on
Python int pairs, and synchronous numpy sweeps from +infinity to the fixed point on the device's uint64 words.  Then the
back-link, the surface, the walk along the links, and numpy statements of dsm.peaks, dsm.watershed and dsm.split_objects on top
of them.  The two statements of the keys are held against each other in test_dsm_watershed_cpu.py and the device against them in
test_dsm_watershed_gpu.py.  The switches (saturate, void_outlets, seed_wins, neighbours, reset_d, low_ties, clamp, offset_first)
plant the errors the GPU file's comparison has to report; their defaults are the rule.  numpy only."""
import heapq

import numpy as np

import dsm_hydro_oracle as ho
import dsm_label_oracle as lo

DC, DR = ho.DC, ho.DR
INVALID_KEY = np.uint64(0xffffffffffffffff)
INF_KEY = np.uint64(0xfffffffe00000000)
OUT = ("keys", "surface", "steps", "backlink")
# the wrong implementations the comparison has to tell from the rule: chain(**PLANTED[name])
PLANTED = {"non-saturating infinity": dict(saturate=False), "voids as outlets": dict(void_outlets=True), "the seed loses ties": dict(seed_wins=False),
           "4 neighbours": dict(neighbours=4), "d carried over a rise": dict(reset_d=False), "ties to the highest k": dict(low_ties=False),
           "the marker not clamped": dict(clamp=False), "the offset before the polarity": dict(offset_first=True)}


# ---- cells, seeds --------------------------------------------------------------------------------------------------------------
def setup(z, marker, domain=None, polarity=1, offset=0, nodata=-999.0, clamp=True, offset_first=False, void_outlets=False):
    """-> v (valid cells), g = polarity q, seed (mask), s (the seeds' levels; 0 elsewhere), all (gh, gw), int64 heights.
    Planted errors: clamp=False leaves a marker below the surface where it is; offset_first=True adds the offset before the
    polarity is applied; void_outlets=True makes every valid cell beside a wall a seed at its own height, as the flood has it."""
    assert polarity in (1, -1)
    z = np.asarray(z, np.float32)
    v = ho.valid(z, nodata)
    if domain is not None:
        v &= np.asarray(domain) != 0
    g = polarity * ho.quanta(z, nodata)
    qm = ho.quanta(marker, nodata)
    seed = v & ho.valid(marker, nodata)
    s = polarity * (qm + offset) if offset_first else polarity * qm + offset
    if clamp:
        s = np.maximum(s, g)
    if void_outlets:
        out = ho.outlets(v)
        s = np.where(out & seed, np.minimum(s, g), np.where(out, g, s))
        seed = seed | out
    return v, np.where(v, g, 0), seed, np.where(seed, s, 0)


def pack(w, d):
    return ((np.asarray(w, np.int64) + 2 ** 31).astype(np.uint64) << np.uint64(32)) | np.asarray(d, np.int64).astype(np.uint64)


def unpack(keys):
    """-> w, d int64 (0, -1 where the key is all ones or +infinity), reached."""
    keys = np.ascontiguousarray(keys).view(np.uint64)
    reached = keys < INF_KEY
    w = np.where(reached, (keys >> np.uint64(32)).astype(np.int64) - 2 ** 31, 0)
    d = np.where(reached, (keys & np.uint64(0xffffffff)).astype(np.int64), -1)
    return w, d, reached


# ---- keys: Dijkstra from the seeds on Python ints ------------------------------------------------------------------------------
def keys_heap(v, g, seed, s, neighbours=8, reset_d=True):
    """-> the uint64 keys: all ones where invalid, +infinity where no seed reaches.
    Planted errors: neighbours=4 floods through E, S, W, N only; reset_d=False carries d over a rise."""
    gh, gw = v.shape
    ks = range(8) if neighbours == 8 else (0, 2, 4, 6)
    vl, gl = v.tolist(), g.tolist()
    keys = np.where(v, INF_KEY, INVALID_KEY)
    best, heap = {}, []
    for r, c in zip(*(a.tolist() for a in np.nonzero(seed))):
        level = max(int(s[r, c]), gl[r][c])                   # K = max((g, 0), .): an unclamped marker is still floored
        best[(r, c)] = (level, 0)
        heap.append((level, 0, r, c))
    heapq.heapify(heap)
    done = set()
    while heap:
        kw, kd, r, c = heapq.heappop(heap)
        if (r, c) in done:
            continue
        done.add((r, c))
        keys[r, c] = (kw + 2 ** 31) << 32 | kd
        for k in ks:
            rr, cc = r + DR[k], c + DC[k]
            if not (0 <= rr < gh and 0 <= cc < gw) or not vl[rr][cc] or (rr, cc) in done:
                continue
            gn = gl[rr][cc]
            cand = max((gn, 0), (kw, kd + 1)) if reset_d else (max(gn, kw), kd + 1)
            if cand < best.get((rr, cc), (2 ** 62, 0)):
                best[(rr, cc)] = cand
                heapq.heappush(heap, (cand[0], cand[1], rr, cc))
    return keys


# ---- keys: synchronous sweeps on the device's words --------------------------------------------------------------------------------
def neighbour_keys(keys):
    """(8, gh, gw): the key of every cell's neighbour k, all ones beyond the grid."""
    gh, gw = keys.shape
    p = np.full((gh + 2, gw + 2), INVALID_KEY, np.uint64)
    p[1:-1, 1:-1] = keys
    return np.stack([p[1 + DR[k]:1 + DR[k] + gh, 1 + DC[k]:1 + DC[k] + gw] for k in range(8)])


def keys_sweeps(v, g, seed, s, saturate=True, return_sweeps=False):
    """K <- min(K, max((g, 0), min over the neighbours of K + 1)) on all valid cells at once, from (S, +infinity), until nothing
    moves; walls hold all ones and +infinity + 1 = +infinity.  Planted error: saturate=False adds the 1 whatever the minimum is,
    in the words' own arithmetic, so that all ones wrap to 0 on a cell between walls."""
    floor = pack(g, 0)
    key = np.where(v, np.where(seed, pack(np.maximum(s, g), 0), INF_KEY), INVALID_KEY)
    sweeps = 0
    while True:
        low = neighbour_keys(key).min(axis=0)
        with np.errstate(over="ignore"):
            step = low + np.uint64(1)
        cand = np.maximum(floor, step)
        if saturate:
            cand = np.where(low >= INF_KEY, INF_KEY, cand)
        new = np.where(v, np.minimum(key, cand), key)
        sweeps += 1
        if np.array_equal(new, key):
            break
        key = new
    return (key, sweeps) if return_sweeps else key


# ---- back-link, surface --------------------------------------------------------------------------------------------------------
def backlinks(keys, v, g, seed, s, low_ties=True, seed_wins=True):
    """uint8: 255 invalid or unreached, 0 a seed with K == S, else k + 1 of the neighbour with the least key, ties to the lowest k
    (0 if no neighbour is lower: not a fixed point's keys).  Planted errors: low_ties=False takes the highest k; seed_wins=False
    links a seed whose neighbours offer it the very key it has."""
    reached = v & (keys < INF_KEY)
    nk = neighbour_keys(keys)
    low, code = keys.copy(), np.zeros(keys.shape, np.int64)
    for k in range(8):
        better = (nk[k] < low) | (np.bool_(not low_ties) & (nk[k] == low) & (code > 0))
        low, code = np.where(better, nk[k], low), np.where(better, k + 1, code)
    root = seed & reached & (keys == pack(s, 0))
    if not seed_wins:
        offered = np.maximum(pack(g, 0), np.minimum(low, INF_KEY - np.uint64(1)) + np.uint64(1))
        root &= ~((code > 0) & (offered == keys))
    return np.where(~reached, 255, np.where(root, 0, code)).astype(np.uint8)


def surface_of(z, keys, v, g, polarity, nodata=-999.0):
    """surface float32 (own bits where w == g, else polarity w / 256) and steps int32 of the keys."""
    z = np.asarray(z, np.float32)
    w, d, reached = unpack(keys)
    reached &= v
    surface = np.where(reached, np.where(w == g, z, (polarity * w / 256.0).astype(np.float32)), np.float32(nodata)).astype(np.float32)
    return surface, np.where(reached, d, -1).astype(np.int32)


def chain(z, marker, domain=None, polarity=1, offset=0, nodata=-999.0, heap=False, **planted):
    """Every output of the rule for one set of inputs -> dict keys, surface, steps, backlink, n_seeds, n_unreached."""
    pick = lambda *names: {k: planted[k] for k in names if k in planted}     # noqa: E731
    v, g, seed, s = setup(z, marker, domain, polarity, offset, nodata, **pick("clamp", "offset_first", "void_outlets"))
    if heap or "neighbours" in planted or "reset_d" in planted:
        keys = keys_heap(v, g, seed, s, **pick("neighbours", "reset_d"))
    else:
        keys = keys_sweeps(v, g, seed, s, **pick("saturate"))
    surface, steps = surface_of(z, keys, v, g, polarity, nodata)
    return {"keys": keys, "surface": surface, "steps": steps, "backlink": backlinks(keys, v, g, seed, s, **pick("low_ties", "seed_wins")),
            "n_seeds": int(seed.sum()), "n_unreached": int((v & (keys >= INF_KEY)).sum())}


def differing(got, want):
    """The outputs of `want` that differ in `got`, each with its first differing cell: [] if all are equal, float32 by bits."""
    out = []
    for name, w in want.items():
        g = np.asarray(got[name])
        w = np.asarray(w)
        if g.dtype == np.int64 and w.dtype == np.uint64:
            g = g.view(np.uint64)
        if g.shape != w.shape or g.dtype != w.dtype:
            out.append((name, "shape or dtype", g.shape, g.dtype, w.shape, w.dtype))
            continue
        a, b = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else (g, w)
        if not np.array_equal(a, b):
            at = np.argwhere(np.atleast_1d(a != b))
            out.append((name, int(len(at)), tuple(int(i) for i in at[0])))
    return out


# ---- the forest ----------------------------------------------------------------------------------------------------------------
def roots_of(link):
    """The root cell (flat index) every cell's links end at, -1 where the code is 255, by walking."""
    gh, gw = link.shape
    code = link.reshape(-1).astype(np.int64)
    cell = np.arange(gh * gw)
    step = np.array([0] + [DR[k] * gw + DC[k] for k in range(8)])
    at = np.where(code <= 8, cell, -1)
    for _ in range(gh * gw + 1):
        on = at >= 0
        nxt = np.where(on, at + step[np.where(on, code[np.maximum(at, 0)], 0)], -1)
        if np.array_equal(nxt, at):
            return at.reshape(gh, gw)
        at = nxt
    raise AssertionError("the links hold a cycle")


# ---- the Python layer ----------------------------------------------------------------------------------------------------------
def h_quanta(h):
    return int(np.floor(float(h) * 256.0))


def peaks(z, h, mask=None, min_height=None, connectivity=8, nodata=-999.0, **planted):
    """dsm.peaks in numpy -> (labels, n, table with first, area, height, dome)."""
    z = np.asarray(z, np.float32)
    H = h_quanta(h)
    got = chain(z, z, mask, -1, H, nodata, **planted)
    w, _, reached = unpack(got["keys"])
    q = ho.quanta(z, nodata)
    dome_q = np.where(reached, q + w, 0)
    top = reached & (dome_q == H)
    if min_height is not None:
        top &= z > np.float32(min_height)
    labels, n = lo.label(top, connectivity)
    st = lo.stats(labels, n, z, nodata)
    flat = labels.reshape(-1)
    first = np.array([int(np.argmax(flat == k + 1)) for k in range(n)], np.int64)
    gw = z.shape[1]
    table = {"first": np.stack([first // gw, first % gw], 1).astype(np.int32).reshape(n, 2), "area": st["area"], "height": st["max"]}
    dome = np.where(reached, (dome_q / 256.0).astype(np.float32), np.float32(nodata)).astype(np.float32)
    return labels, n, table, dome


def watershed(z, markers, mask=None, peaks_up=True, nodata=-999.0, **planted):
    """dsm.watershed in numpy -> (labels int32, level float32): every cell takes the marker label at the end of its links."""
    z = np.asarray(z, np.float32)
    markers = np.asarray(markers, np.int32)
    polarity = -1 if peaks_up else 1
    got = chain(z, np.where(markers > 0, z, np.float32(np.nan)), mask, polarity, 0, nodata, **planted)
    root = roots_of(got["backlink"])
    labels = np.where(root >= 0, markers.reshape(-1)[np.maximum(root, 0)], 0).astype(np.int32)
    return labels, got["surface"]


def split_objects(above, grid, h=2.0, min_height=2.5, min_area_m2=50.0, connectivity=8, nodata=-999.0):
    """dsm.split_objects in numpy -> (labels, n, table)."""
    z = np.asarray(above, np.float32)
    objects, _ = lo.objects(z, grid, min_height, min_area_m2, connectivity, nodata)
    inside = objects > 0
    tops, n, _, _ = peaks(z, h, inside, None, connectivity, nodata)
    seg, _ = watershed(z, tops, inside, True, nodata)
    flat = seg.reshape(-1)
    first = np.array([int(np.argmax(flat == k + 1)) for k in range(n)], np.int64)
    order = np.argsort(first, kind="stable")
    new_id = np.zeros(n + 1, np.int32)
    new_id[order + 1] = np.arange(1, n + 1)
    labels = new_id[seg]
    table = lo.stats(labels, n, z, nodata, grid)
    table["object"] = objects.reshape(-1)[first[order]].astype(np.int32)
    return labels, n, table
