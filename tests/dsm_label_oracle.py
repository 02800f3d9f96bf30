"""Test-local numpy oracle of the object labelling (include/satmvs.h smvs_dsm_label / smvs_dsm_label_stats, DESIGN.md section 9,
"Objects"), stated twice: vectorised over row runs with a union-find over the runs, and as a flood fill per cell (label_brute)
that the CPU tests hold against it.  Plus the statistics, the sieve, and the structured masks with their closed-form answers.
Nothing here imports satmvs_amd.

A component's number is the rank, from 1, of its first cell in raster order among the first cells of all components: the
numbering of scipy.ndimage.label."""
import numpy as np

from dsm_testkit import f2key, key2f, scene as kit_scene, valid  # noqa: F401  (re-exported)

INT_MAX = 2 ** 31 - 1
Q_CLAMP = float(2 ** 21)


# ---- labelling -----------------------------------------------------------------------------------------------------------------
def label(mask, connectivity=8):
    """-> (labels int32 (gh, gw), n).  Runs of foreground cells along the rows, numbered in raster order; runs of neighbouring
    rows that touch (over a diagonal too with connectivity 8) are united, the higher root under the lower, until nothing
    changes; a component's root is then its first run."""
    fg = np.asarray(mask) != 0
    gh, gw = fg.shape
    start = fg.copy()
    start[:, 1:] &= ~fg[:, :-1]
    rid = np.where(fg, np.cumsum(start.ravel()).reshape(gh, gw) - 1, -1)    # the run of every cell
    nruns = int(start.sum())
    pairs = []
    if gh > 1:
        both = [(rid[1:], rid[:-1])]                                         # a cell and the one above it
        if connectivity == 8 and gw > 1:
            both += [(rid[1:, 1:], rid[:-1, :-1]), (rid[1:, :-1], rid[:-1, 1:])]
        for lo, up in both:
            ok = (lo >= 0) & (up >= 0)
            pairs.append(np.stack([lo[ok], up[ok]], 1))
    pairs = np.unique(np.concatenate(pairs), axis=0) if pairs else np.zeros((0, 2), np.int64)
    root = np.arange(nruns)
    while len(pairs):
        ra, rb = root[pairs[:, 0]], root[pairs[:, 1]]
        differ = ra != rb
        if not differ.any():
            break
        pairs, ra, rb = pairs[differ], ra[differ], rb[differ]
        np.minimum.at(root, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:                                                          # every run to its root
            up = root[root]
            if np.array_equal(up, root):
                break
            root = up
    firsts, number = np.unique(root, return_inverse=True)
    labels = np.where(fg, (number.reshape(-1) + 1)[np.maximum(rid, 0)] if nruns else 0, 0).astype(np.int32)
    return labels, int(len(firsts))


def label_brute(mask, connectivity=8):
    """The same by a flood fill from every unlabelled foreground cell in raster order."""
    fg = (np.asarray(mask) != 0).tolist()
    gh, gw = len(fg), len(fg[0])
    steps = [(0, 1), (-1, 0), (0, -1), (1, 0)] + ([(-1, 1), (-1, -1), (1, -1), (1, 1)] if connectivity == 8 else [])
    lab = [[0] * gw for _ in range(gh)]
    n = 0
    for i in range(gh):
        for j in range(gw):
            if fg[i][j] and not lab[i][j]:
                n += 1
                lab[i][j] = n
                stack = [(i, j)]
                while stack:
                    r, c = stack.pop()
                    for dr, dc in steps:
                        rr, cc = r + dr, c + dc
                        if 0 <= rr < gh and 0 <= cc < gw and fg[rr][cc] and not lab[rr][cc]:
                            lab[rr][cc] = n
                            stack.append((rr, cc))
    return np.array(lab, np.int32).reshape(gh, gw), n


# ---- statistics ----------------------------------------------------------------------------------------------------------------
def q(v):
    """The fixed-point image of float32 values: units of 2^-10 m, clamped to +-2^21 m, halves to even.  -> int64."""
    return np.rint(np.clip(np.asarray(v, np.float32).astype(np.float64), -Q_CLAMP, Q_CLAMP) * 1024.0).astype(np.int64)


def stats(labels, n, values=None, nodata=-999.0, grid=None):
    """The dict of dsm.label_stats: labels int32 (gh, gw), entry k for label k + 1; cells outside 1 .. n count for nothing."""
    labels = np.asarray(labels)
    sel = (labels >= 1) & (labels <= n)
    rows, cols = np.nonzero(sel)
    k = labels[sel].astype(np.int64) - 1
    area = np.bincount(k, minlength=n).astype(np.int32)
    bbox = np.empty((n, 4), np.int32)
    bbox[:, :2], bbox[:, 2:] = INT_MAX, -1
    np.minimum.at(bbox[:, 0], k, rows)
    np.minimum.at(bbox[:, 1], k, cols)
    np.maximum.at(bbox[:, 2], k, rows)
    np.maximum.at(bbox[:, 3], k, cols)
    rc = np.zeros((n, 2), np.int64)
    np.add.at(rc[:, 0], k, rows)
    np.add.at(rc[:, 1], k, cols)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = {"area": area, "bbox": bbox, "rc_sum": rc, "centroid": rc.astype(np.float64) / area.astype(np.float64)[:, None]}
        if grid is not None:
            out["area_m2"] = area.astype(np.float64) * float(grid.xres) * float(grid.yres)
            out["centroid_en"] = np.stack([float(grid.e0) + out["centroid"][:, 1] * float(grid.xres),
                                           float(grid.n0) - out["centroid"][:, 0] * float(grid.yres)], 1)
        if values is not None:
            z = np.ascontiguousarray(values, np.float32)
            ok = valid(z, nodata)[sel]
            kv, zv = k[ok], z[sel][ok]
            nvalid = np.bincount(kv, minlength=n).astype(np.int32)
            kmin, kmax = np.full(n, 0xffffffff, np.uint32), np.zeros(n, np.uint32)
            np.minimum.at(kmin, kv, f2key(zv))
            np.maximum.at(kmax, kv, f2key(zv))
            qsum = np.zeros(n, np.int64)
            np.add.at(qsum, kv, q(zv))
            some = nvalid > 0
            out["n_valid"] = nvalid
            out["min"] = np.where(some, key2f(kmin), np.float32(nodata)).astype(np.float32)
            out["max"] = np.where(some, key2f(kmax), np.float32(nodata)).astype(np.float32)
            out["qsum"] = qsum
            out["mean"] = np.where(some, qsum.astype(np.float64) / 1024.0 / np.maximum(nvalid, 1).astype(np.float64), np.nan)
            if grid is not None:
                out["volume"] = qsum.astype(np.float64) / 1024.0 * float(grid.xres) * float(grid.yres)
    return out


def same_stats(got, want, what=""):
    """Every entry equal: integers by value, float32 by bits, float64 by value with NaN at the same places."""
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for key, w in want.items():
        g = np.asarray(got[key])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, key, g.shape, g.dtype, w.shape, w.dtype)
        if g.dtype == np.float32:
            equal = np.array_equal(g.view(np.uint32), w.view(np.uint32))
        else:
            equal = np.array_equal(g, w, equal_nan=g.dtype == np.float64)
        assert equal, (what, key, np.argwhere(np.atleast_1d(g != w))[:5].tolist())


def sieve(labels, area, min_area=1, max_area=None):
    """-> (labels', n', kept int64): components outside min_area .. max_area become 0, the rest keep their order."""
    area = np.asarray(area)
    keep = area >= min_area
    if max_area is not None:
        keep &= area <= max_area
    lut = np.concatenate([[0], np.cumsum(keep) * keep]).astype(np.int32)
    return lut[np.asarray(labels)], int(keep.sum()), np.nonzero(keep)[0].astype(np.int64)


def objects(above, grid, min_height=2.5, min_area_m2=50.0, connectivity=8, nodata=-999.0):
    """dsm.extract_objects in numpy."""
    z = np.ascontiguousarray(above, np.float32)
    with np.errstate(invalid="ignore"):
        fg = valid(z, nodata) & (z > np.float32(min_height))
    labels, n = label(fg, connectivity)
    st = stats(labels, n, z, nodata, grid)
    labels, _, kept = sieve(labels, st["area"], int(np.ceil(min_area_m2 / (float(grid.xres) * float(grid.yres)))))
    return labels, {k: v[kept] for k, v in st.items()}


# ---- masks and value grids -----------------------------------------------------------------------------------------------------
def random_mask(gh, gw, density, seed):
    return (np.random.default_rng(seed).random((gh, gw)) < density).astype(np.uint8)


def spiral(gh, gw):
    """A one-cell-wide path from the upper-left corner inwards, one cell of background between its arms: one component
    under both connectivities whose path is half the grid."""
    m = np.zeros((gh, gw), np.uint8)
    r = c = 0
    dr, dc = 0, 1
    m[0, 0] = 1
    turns = 0
    while turns < 2:
        nr, nc, ar, ac = r + dr, c + dc, r + 2 * dr, c + 2 * dc
        free = 0 <= nr < gh and 0 <= nc < gw and not m[nr, nc] and not (0 <= ar < gh and 0 <= ac < gw and m[ar, ac])
        if free:
            r, c, turns = nr, nc, 0
            m[r, c] = 1
        else:
            dr, dc, turns = dc, -dr, turns + 1
    return m


STRUCTURED = ("empty", "full", "corners", "checkerboard", "rows", "columns", "spiral", "comb", "two_combs", "diagonal", "antidiagonal")


def structured(name, gh, gw):
    """The structured masks of the GPU tests, uint8 (gh, gw)."""
    r, c = np.mgrid[0:gh, 0:gw]
    m = np.zeros((gh, gw), np.uint8)
    if name == "full":
        m[:] = 1
    elif name == "corners":
        m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = 1
    elif name == "checkerboard":
        m[(r + c) % 2 == 0] = 1
    elif name == "rows":
        m[::2] = 1
    elif name == "columns":
        m[:, ::2] = 1
    elif name == "spiral":
        m = spiral(gh, gw)
    elif name == "comb":                                                     # teeth that meet only in the last row
        m[:, ::2] = 1
        m[-1] = 1
    elif name == "two_combs":                                                # one hangs from row 0, one stands on the last row
        m[0] = 1
        m[:gh - 2, ::4] = 1
        m[-1] = 1
        m[2:, 2::4] = 1
    elif name == "diagonal":                                                 # from the upper-left corner, one step down and right
        m[c == r] = 1
    elif name == "antidiagonal":                                             # from the upper-right corner, one step down and left
        m[c == gw - 1 - r] = 1
    elif name != "empty":
        raise ValueError(name)
    return m


def closed_form(name, gh, gw, connectivity):
    """(labels, n) of structured(name, gh, gw) by formula (gh, gw >= 5)."""
    m = structured(name, gh, gw)
    r, c = np.mgrid[0:gh, 0:gw]
    one = (m.astype(np.int32), 1)
    each = (np.where(m != 0, np.cumsum(m.ravel() != 0).reshape(gh, gw), 0).astype(np.int32), int((m != 0).sum()))
    if name == "empty":
        return m.astype(np.int32), 0
    if name in ("full", "spiral", "comb"):
        return one
    if name == "corners":
        return each
    if name == "checkerboard":
        return one if connectivity == 8 else each
    if name == "rows":
        return (m * (r // 2 + 1)).astype(np.int32), (gh + 1) // 2
    if name == "columns":
        return (m * (c // 2 + 1)).astype(np.int32), (gw + 1) // 2
    if name == "two_combs":
        lab = m.astype(np.int32)
        lab[2:, 2::4] = 2 * m[2:, 2::4]
        lab[-1] = 2
        return lab, 2
    if name in ("diagonal", "antidiagonal"):                                 # one cell per row
        return one if connectivity == 8 else ((m * (r + 1)).astype(np.int32), min(gh, gw))
    raise ValueError(name)


def squares(gh, gw, side=3, pitch=4):
    """side x side squares on a pitch: (mask, labels, n), label = the square's raster index + 1 under both connectivities."""
    r, c = np.mgrid[0:gh, 0:gw]
    inside = (r % pitch < side) & (c % pitch < side)
    per_row = (gw + pitch - 1) // pitch
    labels = np.where(inside, (r // pitch) * per_row + c // pitch + 1, 0).astype(np.int32)
    return inside.astype(np.uint8), labels, per_row * ((gh + pitch - 1) // pitch)


def value_grid(gh, gw, seed=0, voids=0.1):
    """Heights for the statistics: dsm_testkit.scene about zero (negative heights, NaN and nodata voids and holes), -0.0 beside
    +0.0, one 3e6 (clamped by q) and, from 40 cells on, one -3e6."""
    r, c = np.mgrid[0:gh, 0:gw].astype(np.float64)
    z = kit_scene(5.0 * c, -5.0 * r, seed=seed, voids=voids, salt=0.02, base=3.0, amp=20.0)
    flat = z.reshape(-1)
    n = flat.size
    flat[n // 2] = np.float32(-0.0)
    if n > 1:
        flat[n // 2 - 1] = np.float32(0.0)
    if n > 4:
        flat[n // 3] = np.float32(3e6)
    if n >= 40:
        flat[n // 5] = np.float32(-3e6)
    return z
