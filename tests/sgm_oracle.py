"""The rules of the census plane sweep and semi-global matching (include/satmvs.h, smvs_sgm_*) in numpy, each stated twice:

    census     census_cost (a loop over the window's offsets on padded arrays)      census_cost_loop (pixel by pixel)
    aggregate  aggregate (arrays: all lines of a direction step together)           aggregate_walk (pixel by pixel along each path)
    select     select (arrays)                                                      select_loop (pixel by pixel)

The GPU tests compare with the first of each pair; tests/test_sgm_cpu.py holds the pairs against each other.  Every function
takes keyword switches that plant one error each (`plant=`), for the tests that show that the comparison reports them.
Volumes are plane-minor, (B, H, W, D) uint16; a warped volume is (B, 2, Dc, H, W) float32 = [image, coverage]."""
import numpy as np

VOID = 0xFFFF
NAN32 = np.uint32(0x7FC00000).view(np.float32)
DIRS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))


def offsets(radius):
    """The window in row-major order of (dy, dx), the centre left out."""
    return [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if (dy, dx) != (0, 0)]


# ---- census ----------------------------------------------------------------------------------------------------------------------
def _shifted(a, dy, dx, r, fill):
    """a (..., H, W) read at (y + dy, x + dx), `fill` off the grid."""
    H, W = a.shape[-2:]
    pad = np.full(a.shape[:-2] + (H + 2 * r, W + 2 * r), fill, a.dtype)
    pad[..., r:r + H, r:r + W] = a
    return pad[..., r + dy:r + dy + H, r + dx:r + dx + W]


def census_bits(img, radius, plant=None):
    """img (..., H, W) float32 -> (bits, mask), both (nbits, ..., H, W) bool: bits[k] = I(p + o_k) < I(p); mask[k] = p + o_k on the grid."""
    img = np.asarray(img, np.float32)
    on = np.ones(img.shape, bool)
    bits, mask = [], []
    with np.errstate(invalid="ignore"):
        for dy, dx in offsets(radius):
            q = _shifted(img, dy, dx, radius, np.float32(0))
            bits.append(q <= img if plant == "le" else q < img)
            mask.append(_shifted(on, dy, dx, radius, False))
    return np.stack(bits), np.stack(mask)


def census_cost(ref, warped, radius, cov_min, plant=None):
    """ref (B, H, W), warped: a list of (B, 2, Dc, H, W) -> cost (B, H, W, Dc) uint16."""
    ref = np.asarray(ref, np.float32)
    rbits, mask = census_bits(ref, radius, plant)                                # (nb, B, H, W)
    B, H, W = ref.shape
    Dc = warped[0].shape[2]
    ham = np.zeros((B, Dc, H, W), np.int64)
    n = np.zeros((B, Dc, H, W), np.int64)
    for w in warped:
        w = np.asarray(w, np.float32)
        sbits, _ = census_bits(w[:, 0], radius, plant)                           # (nb, B, Dc, H, W)
        with np.errstate(invalid="ignore"):
            ok = w[:, 1] >= np.float32(cov_min)
        valid = ok.copy()
        if plant != "uncovered_ignored":
            for dy, dx in offsets(radius):
                valid &= _shifted(ok, dy, dx, radius, True)
        h = ((sbits ^ rbits[:, :, None]) & mask[:, :, None]).sum(axis=0)
        ham += np.where(valid, h, 0)
        n += valid
    cost = np.where(n > 0, (16 * ham) // np.maximum(n, 1), VOID)
    return np.ascontiguousarray(cost.transpose(0, 2, 3, 1)).astype(np.uint16)


def census_cost_loop(ref, warped, radius, cov_min):
    """The same rule voxel by voxel, in Python numbers."""
    ref = np.asarray(ref, np.float32)
    B, H, W = ref.shape
    Dc = warped[0].shape[2]
    offs = offsets(radius)
    cm = np.float32(cov_min)
    out = np.empty((B, H, W, Dc), np.uint16)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                inside = [(dy, dx) for dy, dx in offs if 0 <= y + dy < H and 0 <= x + dx < W]
                cref = [bool(ref[b, y + dy, x + dx] < ref[b, y, x]) for dy, dx in inside]
                for d in range(Dc):
                    total = n = 0
                    for w in warped:
                        img, cov = w[b, 0, d], w[b, 1, d]
                        if not (cov[y, x] >= cm and all(cov[y + dy, x + dx] >= cm for dy, dx in inside)):
                            continue
                        total += sum(bool(img[y + dy, x + dx] < img[y, x]) != c for (dy, dx), c in zip(inside, cref))
                        n += 1
                    out[b, y, x, d] = (16 * total) // n if n else VOID
    return out


# ---- aggregation -------------------------------------------------------------------------------------------------------------------
def clamped(cost, cost_max, void_cost):
    c = np.asarray(cost, np.uint16).astype(np.int64)
    return np.where(c == VOID, void_cost, np.minimum(c, cost_max))


def _p2(guide, p, q, P2, alpha, p2_min):
    return P2 if guide is None else max(p2_min, P2 - alpha * abs(int(guide[p]) - int(guide[q])))


def path_walk(cp, ry, rx, P1, P2, guide=None, alpha=0, p2_min=0):
    """L_r of one direction, pixel by pixel in an order in which q = p - r comes before p; cp (B, H, W, D) int64."""
    B, H, W, D = cp.shape
    L = np.zeros_like(cp)
    ys = range(H) if ry >= 0 else range(H - 1, -1, -1)
    xs = range(W) if rx >= 0 else range(W - 1, -1, -1)
    for b in range(B):
        for y in ys:
            for x in xs:
                qy, qx = y - ry, x - rx
                if not (0 <= qy < H and 0 <= qx < W):
                    L[b, y, x] = cp[b, y, x]
                    continue
                q = L[b, qy, qx]
                m = int(q.min())
                p2 = _p2(guide, (b, y, x), (b, qy, qx), P2, alpha, p2_min)
                best = np.minimum(q, m + p2)                                     # the planes of one pixel at once
                best[1:] = np.minimum(best[1:], q[:-1] + P1)                     # d - 1 exists
                best[:-1] = np.minimum(best[:-1], q[1:] + P1)                    # d + 1 exists
                L[b, y, x] = cp[b, y, x] + best - m
    return L


def path_lines(cp, ry, rx, P1, P2, guide=None, alpha=0, p2_min=0, plant=None):
    """L_r of one direction with all its lines stepping together: row by row (ry != 0) or column by column."""
    if ry == 0:                                                                  # columns as rows of the transposed volume
        g = None if guide is None else guide.transpose(0, 2, 1)
        return path_lines(cp.transpose(0, 2, 1, 3), rx, 0, P1, P2, g, alpha, p2_min, plant).transpose(0, 2, 1, 3)
    B, H, W, D = cp.shape
    big = np.int64(1) << 40
    L = np.zeros_like(cp)
    rows = range(H) if ry > 0 else range(H - 1, -1, -1)
    x = np.arange(W)
    on = (x - rx >= 0) & (x - rx < W)                                            # whether q is on the grid, per column
    src = np.clip(x - rx, 0, W - 1)
    for k, y in enumerate(rows):
        if k == 0:
            L[:, y] = 0 if plant == "start_zero" else cp[:, y]
            continue
        q = L[:, y - ry][:, src]                                                 # (B, W, D)
        m = q.min(axis=-1, keepdims=True)
        if guide is None:
            p2 = np.int64(P2)
        else:
            dg = np.abs(guide[:, y].astype(np.int64) - guide[:, y - ry][:, src].astype(np.int64))
            p2 = np.maximum(p2_min, P2 - alpha * dg)[..., None]
        down = np.concatenate([np.full((B, W, 1), big), q[..., :-1]], axis=-1) + P1
        up = np.concatenate([q[..., 1:], np.full((B, W, 1), big)], axis=-1) + P1
        same = q + P1 if plant == "p1_on_d" else q
        best = np.minimum(np.minimum(same, np.minimum(down, up)), m + p2)
        step = cp[:, y] + best - (0 if plant == "no_minus_m" else m)
        L[:, y] = np.where(on[None, :, None], step, 0 if plant == "start_zero" else cp[:, y])
    return L


def aggregate(cost, P1, P2, paths=8, guide=None, alpha=0, p2_min=None, cost_max=768, void_cost=96, plant=None, walk=False, parts=False):
    """sum (B, H, W, D) uint16 of the L_r of `paths` directions; parts=True: the list of L_r (int64) instead."""
    p2_min = P1 if p2_min is None else p2_min
    assert 0 <= P1 <= p2_min <= P2 and 0 <= void_cost <= cost_max and paths in (4, 8)
    cp = clamped(cost, cost_max, void_cost)
    g = None if guide is None else np.asarray(guide, np.uint8)
    if walk:
        Ls = [path_walk(cp, ry, rx, P1, P2, g, alpha, p2_min) for ry, rx in DIRS[:paths]]
    else:
        Ls = [path_lines(cp, ry, rx, P1, P2, g, alpha, p2_min, plant) for ry, rx in DIRS[:paths]]
    if parts:
        return Ls
    total = sum(Ls)
    if plant is None:
        assert total.max() <= 65535 and paths * (cost_max + P2) <= 65535
    return (total & 0xFFFF).astype(np.uint16)


# ---- select ------------------------------------------------------------------------------------------------------------------------
def _depth4(depth, shape):
    B, H, W, D = shape
    depth = np.asarray(depth, np.float32)
    return np.broadcast_to(depth[:, :, None, None], (B, D, H, W)) if depth.ndim == 2 else depth


def select(total, depth, uniqueness=0, cost=None, min_support=1, plant=None):
    """-> (index int32, height float32, min_sum uint16, support uint16 or None), each (B, H, W)."""
    s = np.asarray(total, np.uint16).astype(np.int64)
    B, H, W, D = s.shape
    z = _depth4(depth, s.shape).transpose(0, 2, 3, 1).astype(np.float64)         # (B, H, W, D)
    d0 = D - 1 - s[..., ::-1].argmin(-1) if plant == "last_tie" else s.argmin(-1)
    best = np.take_along_axis(s, d0[..., None], -1)[..., 0]
    d = np.arange(D)
    far = np.abs(d - d0[..., None]) > (0 if plant == "unique_near" else 1)
    keep = ~(far & (s * (100 - uniqueness) < best[..., None] * 100)).any(-1)
    support = None
    if cost is not None:
        support = (np.asarray(cost, np.uint16) != VOID).sum(-1)
        keep &= support >= min_support
    take = lambda a, k: np.take_along_axis(a, np.clip(k, 0, D - 1)[..., None], -1)[..., 0]      # noqa: E731
    a, c = take(s, d0 - 1), take(s, d0 + 1)
    den = np.where((d0 > 0) & (d0 < D - 1), a + c - 2 * best, 0)
    with np.errstate(all="ignore"):
        t = (a - c).astype(np.float64) / ((1 if plant == "t_den" else 2) * np.where(den == 0, 1, den)).astype(np.float64)
        h0 = take(z, d0)
        span = np.where(t >= 0, take(z, d0 + 1) - h0, h0 - take(z, d0 - 1))
        h = np.where(den != 0, h0 + t * span, h0).astype(np.float32)
    h = np.where(keep & ~np.isnan(h), h, NAN32).astype(np.float32)
    return (np.where(keep, d0, -1).astype(np.int32), h, best.astype(np.uint16), None if support is None else support.astype(np.uint16))


def select_loop(total, depth, uniqueness=0, cost=None, min_support=1):
    s = np.asarray(total, np.uint16)
    B, H, W, D = s.shape
    z = _depth4(depth, s.shape)
    index, height = np.empty((B, H, W), np.int32), np.empty((B, H, W), np.float32)
    min_sum = np.empty((B, H, W), np.uint16)
    support = None if cost is None else np.empty((B, H, W), np.uint16)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                v = [int(e) for e in s[b, y, x]]
                d0 = v.index(min(v))
                keep = not any(abs(d - d0) > 1 and v[d] * (100 - uniqueness) < v[d0] * 100 for d in range(D))
                if cost is not None:
                    support[b, y, x] = n = sum(int(e) != VOID for e in cost[b, y, x])
                    keep = keep and n >= min_support
                min_sum[b, y, x] = v[d0]
                h = np.float64(z[b, d0, y, x])
                if 0 < d0 < D - 1 and v[d0 - 1] + v[d0 + 1] - 2 * v[d0] != 0:
                    t = np.float64(v[d0 - 1] - v[d0 + 1]) / np.float64(2 * (v[d0 - 1] + v[d0 + 1] - 2 * v[d0]))
                    with np.errstate(all="ignore"):
                        span = np.float64(z[b, d0 + 1, y, x]) - h if t >= 0 else h - np.float64(z[b, d0 - 1, y, x])
                        h = h + t * span
                with np.errstate(all="ignore"):
                    h = np.float32(h)
                index[b, y, x] = d0 if keep else -1
                height[b, y, x] = h if keep and not np.isnan(h) else NAN32
    return index, height, min_sum, support


def parabola_t(total):
    """t of every pixel (0 where the rule sets it), for the |t| <= 1/2 invariant."""
    s = np.asarray(total, np.uint16).astype(np.int64)
    D = s.shape[-1]
    d0 = s.argmin(-1)
    take = lambda k: np.take_along_axis(s, np.clip(k, 0, D - 1)[..., None], -1)[..., 0]      # noqa: E731
    a, b, c = take(d0 - 1), take(d0), take(d0 + 1)
    den = np.where((d0 > 0) & (d0 < D - 1), a + c - 2 * b, 0)
    return np.where(den != 0, (a - c) / (2.0 * np.where(den == 0, 1, den)), 0.0)
