"""numpy statements of the rules of smvs_dsm_dist and smvs_dsm_mosaic (include/satmvs.h, "Mosaic"), for test_dsm_mosaic_cpu.py
and test_dsm_mosaic_gpu.py.  The transform is stated twice, by brute force over the background cells and as the separable
two-pass rule; the mosaic once, in float64 operations in the layers' order.  The `plant` arguments build the wrong variants
that the CPU tests show the comparisons catch."""
import numpy as np

from dsm_testkit import f2key, key2f, same_bits, valid  # noqa: F401  (re-exported for the test files)

MODES = ("first", "last", "min", "max", "mean", "feather")
FAR = 1 << 40


# ---- distance ------------------------------------------------------------------------------------------------------------------
def dist_brute(mask, border, cap):
    """d2 by its definition: every cell against every background cell; with a border, against the ring of cells just off the
    grid as well (the nearest off-grid cell of any cell lies on that ring).  For small grids."""
    mask = np.asarray(mask) != 0
    gh, gw = mask.shape
    br, bc = np.nonzero(~mask)
    if border:
        rr = np.concatenate([np.full(gw + 2, -1), np.full(gw + 2, gh), np.arange(gh), np.arange(gh)])
        cc = np.concatenate([np.arange(-1, gw + 1), np.arange(-1, gw + 1), np.full(gh, -1), np.full(gh, gw)])
        br, bc = np.concatenate([br, rr]), np.concatenate([bc, cc])
    out = np.full((gh, gw), cap * cap, np.int64)
    if br.size:
        r, c = np.mgrid[0:gh, 0:gw]
        d = (r[..., None] - br) ** 2 + (c[..., None] - bc) ** 2
        out = np.minimum(out, d.min(axis=2))
    return out.astype(np.int32)


def rows_to_background(mask, border, cap):
    """g(r, c): the distance in rows to the nearest background cell of column c, above or below, capped."""
    mask = np.asarray(mask) != 0
    gh, gw = mask.shape
    rows = np.arange(gh, dtype=np.int64)[:, None]
    none = -1 if border else -FAR                            # the row of the background "cell" above the grid
    last = np.maximum.accumulate(np.where(~mask, rows, none), axis=0)
    last = np.maximum(last, none)
    none = gh if border else FAR
    nxt = np.minimum.accumulate(np.where(~mask, rows, none)[::-1], axis=0)[::-1]
    return np.minimum(np.minimum(rows - last, nxt - rows), cap)


def dist_two_pass(mask, border, cap, plant=None):
    """d2 as the separable rule: g by columns, then min over k of k^2 + g(r, c + k)^2 by rows, off-grid columns 0 with a
    border and cap^2 without.  plant = "short halo": the columns cap - 1 away are not looked at; plant = "cap first": the cap
    is applied to the distance's square as if it were the distance."""
    g = rows_to_background(mask, border, cap)
    gh, gw = g.shape
    reach = cap - 2 if plant == "short halo" else cap
    g2 = np.full((gh, gw + 2 * cap), 0 if border else cap * cap, np.int64)
    g2[:, cap:cap + gw] = g * g
    out = np.full((gh, gw), cap * cap, np.int64)
    for k in range(reach + 1):                               # vectorised over the cells, k = -cap .. cap as the pairs -k, +k
        if k * k >= out.max():                               # no cell can gain from this k or a later one
            break
        np.minimum(out, k * k + g2[:, cap - k:cap - k + gw], out=out)
        np.minimum(out, k * k + g2[:, cap + k:cap + k + gw], out=out)
    if plant == "cap first":
        out = np.minimum(out, cap)
    return out.astype(np.int32)


def buffer_mask(mask, radius, border=False):
    """True within `radius` cells (Euclidean, inclusive) of a set cell: d2 <= floor(radius^2) on the complement's transform."""
    cap = int(np.floor(radius)) + 1
    return dist_two_pass(~(np.asarray(mask) != 0), border, cap) <= int(np.floor(radius * radius))


# ---- mosaic --------------------------------------------------------------------------------------------------------------------
def mosaic(layers, nodata, mode, feather, gw, gh, plant=None):
    """layers: a list of (z float32 (lh, lw), d2 int32 (lh, lw) or None, ox, oy).  -> (out float32, count uint8, source uint8,
    spread float32), each (gh, gw).  Every float64 operation is one numpy operation: rounded by itself, in the layers' order.
    plant = "from zero": the sums start from 0.0; plant = "late ties": min / max / the largest weight keep the later layer."""
    nd = np.float32(nodata)
    m = np.zeros((gh, gw), np.int64)
    src = np.full((gh, gw), 255, np.int64)
    pick = np.full((gh, gw), nd, np.float32)
    pick_key = np.zeros((gh, gw), np.uint32)
    lo, hi = np.zeros((gh, gw), np.uint32), np.zeros((gh, gw), np.uint32)
    S, W, wbest = np.zeros((gh, gw)), np.zeros((gh, gw)), np.zeros((gh, gw))
    late = plant == "late ties"
    for k, (z, d2, ox, oy) in enumerate(layers):
        z = np.asarray(z, np.float32)
        lh, lw = z.shape
        r0, r1, c0, c1 = max(0, oy), min(gh, oy + lh), max(0, ox), min(gw, ox + lw)
        if r1 <= r0 or c1 <= c0:
            continue
        here = np.zeros((gh, gw), bool)
        zc = np.zeros((gh, gw), np.float32)
        dc = np.ones((gh, gw), np.int64)
        part = z[r0 - oy:r1 - oy, c0 - ox:c1 - ox]
        here[r0:r1, c0:c1] = valid(part, nd)
        zc[r0:r1, c0:c1] = np.where(valid(part, nd), part, np.float32(0.0))
        if d2 is not None:
            dc[r0:r1, c0:c1] = np.asarray(d2)[r0 - oy:r1 - oy, c0 - ox:c1 - ox]
        first = here & (m == 0)
        if plant == "from zero":
            first = np.zeros_like(first)
        key = f2key(zc)
        lo = np.where(here & (m == 0), key, np.where(here, np.minimum(lo, key), lo))
        hi = np.where(here & (m == 0), key, np.where(here, np.maximum(hi, key), hi))
        z64 = zc.astype(np.float64)
        if mode == "feather":
            w = np.sqrt(np.clip(dc, 1, feather * feather).astype(np.float64))
            wz = w * z64
            S = np.where(first, wz, np.where(here, S + wz, S))
            W = np.where(first, w, np.where(here, W + w, W))
            better = here & ((m == 0) | ((w >= wbest) if late else (w > wbest)))
            wbest = np.where(better, w, wbest)
            src = np.where(better, k, src)
        elif mode == "mean":
            S = np.where(first, z64, np.where(here, S + z64, S))
            src = np.where(here & (m == 0), k, src)
        else:
            if mode == "first":
                take = here & (m == 0)
            elif mode == "last":
                take = here
            elif mode == "min":
                take = here & ((m == 0) | ((key <= pick_key) if late else (key < pick_key)))
            else:
                take = here & ((m == 0) | ((key >= pick_key) if late else (key > pick_key)))
            pick = np.where(take, zc, pick)
            pick_key = np.where(take, key, pick_key)
            src = np.where(take, k, src)
        m = m + here
    some = m > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == "feather":
            res = (S / W).astype(np.float32)
        elif mode == "mean":
            res = (S / m.astype(np.float64)).astype(np.float32)
        else:
            res = pick
        spread = (key2f(hi).astype(np.float64) - key2f(lo).astype(np.float64)).astype(np.float32)
    out = np.where(some, res, nd).astype(np.float32)
    return out, m.astype(np.uint8), src.astype(np.uint8), np.where(some, spread, nd).astype(np.float32)


def offset(grid, to_grid):
    """(ox, oy) of a layer on the destination from the world-file numbers, float64 (to the nearest cell)."""
    u = (float(grid.e0) - float(to_grid.e0)) / float(to_grid.xres)
    v = (float(to_grid.n0) - float(grid.n0)) / float(to_grid.yres)
    return int(np.floor(u + 0.5)), int(np.floor(v + 0.5))
