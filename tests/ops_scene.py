"""Scenes, float64 references and "explain every difference" checks for the stand-alone operators of csrc/warp.hip
(rpc / homography warp forward and backward, homography composition) and csrc/regress.hip (softmax, window and
streaming regression, flat RPC projectors).  Shared by tests/test_ops_cpu.py (which asserts what the GPU tests assume
about these scenes and references, without a GPU), tests/test_ops_gpu.py and tests/fuzz/fuzz_ops.py.

Nothing here imports the GPU package's kernels; `orc` is the ctypes oracle (oracle/oracle.py) handed in by the caller."""
import numpy as np

U32 = 2.0 ** -24            # unit roundoff of float32
TILE_X, TILE_Y, DCH = 64, 4, 8          # decomposition of warp_kernel (csrc/warp.hip): 64 x 4 pixel tiles, plane chunks of 8
MAX_EXPLAINED = 1e-4        # the project's cap on voxels that differ from the oracle -- here a cap on EXPLAINED voxels only


# ---- the warp matrix --------------------------------------------------------------------------------------------------
# (B, C, D, H, W).  Block count of a launch = ceil(W/64) * ceil(H/4) * ceil(D/min(D,8)) * B; xcd_remap's remainder branch
# runs whenever that is not a multiple of 8.  What each case is there for:
WARP_CASES = [
    (1, 1, 1, 1, 1),        # W = 1 and H = 1 ((W-1)/2 = 0), D = 1, C = 1;                        1 block   (remainder 1)
    (1, 3, 7, 3, 2),        # W = 2, H = 3 (row tail 3 of 4), D = 7 (one short chunk), C odd;     1 block   (remainder 1)
    (2, 8, 8, 4, 63),       # W = 63 (column tail 63 of 64), H = 4 (full tile), D = 8 (one full chunk), B = 2;  2 blocks (2)
    (1, 32, 1, 3, 129),     # W = 129 (two full tiles + 1 column), D = 1, C = 32;                 3 blocks  (remainder 3)
    (3, 33, 9, 5, 64),      # W = 64 (exactly one tile), H = 5 (full tile + 1 row), D = 9 (chunk + 1 plane), B = 3, C = 33;  12 blocks (4)
    (1, 3, 7, 17, 63),      # H = 17: five row tiles;                                             5 blocks  (remainder 5)
    (1, 3, 17, 33, 65),     # W = 65 (tile + 1 column), H = 33 (8 tiles + 1 row), D = 17 (two chunks + 1 plane);  54 blocks (6)
    (3, 1, 8, 17, 2),       # B = 3 with five row tiles;                                          15 blocks (remainder 7)
    (1, 8, 64, 4, 64),      # D = 64 (eight full chunks);                                         8 blocks  (remainder 0)
    (1, 1, 9, 1, 768),      # H = 1 at W = 768 (twelve column tiles);                             24 blocks (remainder 0)
    (2, 3, 1, 384, 1),      # W = 1 at H = 384 (96 row tiles), B = 2;                             192 blocks (remainder 0)
]
BIG_CASE = (1, 3, 64, 384, 768)     # the 768 x 384 tile, 64 planes, per-pixel heights: 12 * 96 * 8 = 9216 blocks; C = 3 keeps the
#                                     oracle at a few seconds (57 M output values)
GEOS = ("rpc", "pinhole")


def block_count(B, D, H, W):
    dch = D if D < DCH else DCH
    return -(-W // TILE_X) * -(-H // TILE_Y) * -(-D // dch) * B


def case_id(c):
    return "B%dC%dD%dH%dW%d" % tuple(c)


def scene(geo, B, C, D, H, W, seed, per_pixel, smooth=False):
    """-> src_fea (B,C,H,W) f32, src geometry, ref geometry ((B,170) or (B,4,4) f64), heights (B,D) or (B,D,H,W) f32.
    The geometry is the project's synthetic one (rpc_synth.make_view_rpcs / a pinhole pair with a small rotation and a
    baseline), heights 0 - 400 m resp. depths 400 - 700; `smooth` features are low-frequency sinusoids of amplitude 1
    (see sampler_bound)."""
    from satmvs_amd import rpc_synth
    rng = np.random.default_rng(seed)
    if smooth:
        fea = smooth_features(B, C, H, W, seed)
    else:
        fea = rng.standard_normal((B, C, H, W)).astype(np.float32)
    # the cameras are those of a tile of at least 16 x 16: a 1-pixel-wide image is a strip of such a tile
    gh, gw = max(H, 16), max(W, 16)
    if geo == "rpc":
        gp = np.stack([rpc_synth.make_view_rpcs(2, gh, gw, seed=seed + 7 * b) for b in range(B)])
        lo, hi = 0.0, 400.0
    else:
        gp = np.zeros((B, 2, 4, 4))
        for b in range(B):
            for v in range(2):
                f = 1.1 * gw
                K = np.array([[f, 0, gw / 2.0, 0], [0, f, gh / 2.0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1]])
                E = np.eye(4)
                a = rng.normal(0, 0.02) * (v > 0)
                E[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
                E[:3, 3] = [25.0 * v * (-1) ** v, 3.0 * v, 0.5 * v]
                gp[b, v] = K @ E
        lo, hi = 400.0, 700.0
    planes = np.linspace(lo, hi, D, dtype=np.float32)[None].repeat(B, 0) if D > 1 else np.full((B, 1), 0.5 * (lo + hi), np.float32)
    if per_pixel:
        depth = (planes.astype(np.float64)[:, :, None, None] + rng.normal(0, 2.0, (B, D, H, W))).astype(np.float32)
    else:
        depth = planes
    return fea, np.ascontiguousarray(gp[:, 1]), np.ascontiguousarray(gp[:, 0]), depth


def smooth_features(B, C, H, W, seed):
    """f[b,c,y,x] = sin(a x + p) * cos(q y + r), |a|, |q| <= 0.5 rad / px, float32-rounded.  Adjacent samples differ by at
    most 0.5, the border samples by at most 1 from the zero padding: the zero-padded bilinear interpolant is continuous
    with a Lipschitz constant of 1 per axis."""
    rng = np.random.default_rng(seed + 1000)
    a, q = rng.uniform(0.05, 0.5, (B, C, 1, 1)), rng.uniform(0.05, 0.5, (B, C, 1, 1))
    p, r = rng.uniform(0, 6.28, (B, C, 1, 1)), rng.uniform(0, 6.28, (B, C, 1, 1))
    y, x = np.arange(H).reshape(1, 1, H, 1), np.arange(W).reshape(1, 1, 1, W)
    return (np.sin(a * x + p) * np.cos(q * y + r)).astype(np.float32)


LIPSCHITZ = 1.0


def qc_dict(rpc):
    """(B,170) -> the reference's QC dictionary layout (numpy arrays), the argument of rpc_warping_enisum."""
    from satmvs_amd import rpc_synth
    keys = ["line_off", "samp_off", "lat_off", "lon_off", "height_off", "line_scale", "samp_scale", "lat_scale",
            "lon_scale", "height_scale"]
    d = {k: np.ascontiguousarray(rpc[:, i]) for i, k in enumerate(keys)}
    for j, nm in enumerate(["line_num", "line_den", "samp_num", "samp_den", "lat_num", "lat_den", "lon_num", "lon_den"]):
        d[nm + "_tensor"] = np.stack([rpc_synth.coeffs_to_qc_tensor(x[10 + 20 * j:30 + 20 * j]) for x in rpc])
    return d


# ---- coordinates ------------------------------------------------------------------------------------------------------
def _heights64(depth, H, W):
    depth = np.asarray(depth, np.float32).astype(np.float64)
    return depth if depth.ndim == 4 else np.broadcast_to(depth[:, :, None, None], depth.shape + (H, W))


def numpy_coords(geo, src, ref, depth, H, W):
    """float64 source-image pixel coordinates (px, py), each (B,D,H,W), by numpy alone: rpc_synth.photo2obj -> obj2photo
    resp. src @ inv(ref) applied to (x, y, 1) * depth.  Independent of oracle.c and of the kernels."""
    from satmvs_amd import rpc_synth
    h = _heights64(depth, H, W)
    B, D = h.shape[:2]
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    px, py = np.empty((B, D, H, W)), np.empty((B, D, H, W))
    for b in range(B):
        if geo == "rpc":
            for d in range(D):                                                   # plane by plane: 20 monomials per point
                lat, lon = rpc_synth.photo2obj(ref[b], xx, yy, h[b, d])
                px[b, d], py[b, d] = rpc_synth.obj2photo(src[b], lat, lon, h[b, d])
        else:
            P = src[b] @ np.linalg.inv(ref[b])
            with np.errstate(divide="ignore", invalid="ignore"):
                rx, ry, rz = (P[i, 0] * xx + P[i, 1] * yy + P[i, 2] for i in range(3))
                X, Y, Z = rx * h[b] + P[0, 3], ry * h[b] + P[1, 3], rz * h[b] + P[2, 3]
                px[b], py[b] = X / Z, Y / Z
    return px, py


def oracle_coords(orc, geo, src, ref, depth, H, W):
    """What the oracle feeds its sampler.  rpc: float64 pixel coordinates (samp, line) -- the reference casts them to
    float32 and normalises in float32; pinhole: the float32 normalised grid (gx, gy) -- the reference normalises in float64."""
    if geo == "rpc":
        _, _, samp, line = orc.rpc_warp_coords(src, ref, depth, H, W)
        return samp, line
    return orc.homo_warp_coords(src, ref, depth, H, W)


def grid_from_pixel32(px32, py32, H, W):
    """The reference's float32 normalisation of float32 pixel coordinates: p / float32((W-1)/2) - 1 (division by zero at W = 1)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        gx = (px32 / np.float32((W - 1) / 2.0) - np.float32(1)).astype(np.float32)
        gy = (py32 / np.float32((H - 1) / 2.0) - np.float32(1)).astype(np.float32)
    return gx, gy


def oracle_grid(orc, geo, src, ref, depth, H, W):
    """float32 normalised grid (gx, gy) of either geometry, as the oracle's sampler sees it."""
    a, b = oracle_coords(orc, geo, src, ref, depth, H, W)
    if geo == "rpc":
        return grid_from_pixel32(a.astype(np.float32), b.astype(np.float32), H, W)
    return a, b


def numpy_grid32(geo, px, py, H, W):
    """The float32 numbers the reference's sequence makes of float64 pixel coordinates: the value whose disagreement
    between two float64 evaluations is the only legitimate source of a differing voxel."""
    if geo == "rpc":
        return px.astype(np.float32), py.astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (px / ((W - 1) / 2.0) - 1.0).astype(np.float32), (py / ((H - 1) / 2.0) - 1.0).astype(np.float32)


def coord_disagreement(orc, geo, src, ref, depth, H, W):
    """Share of voxels at which the oracle's float64 chain and the numpy chain round to different float32 coordinates
    (NaN = NaN), and the largest float64 distance between the two in pixels."""
    a, b = oracle_coords(orc, geo, src, ref, depth, H, W)
    px, py = numpy_coords(geo, src, ref, depth, H, W)
    nx, ny = numpy_grid32(geo, px, py, H, W)
    if geo == "rpc":
        ox, oy = a.astype(np.float32), b.astype(np.float32)
        dist = max(np.nanmax(np.abs(a - px), initial=0.0), np.nanmax(np.abs(b - py), initial=0.0))
    else:
        ox, oy = a, b
        _, _, u, v = orc.homo_warp_coords(src, ref, depth, H, W, pixels=True)
        dist = max(np.nanmax(np.abs(u - px), initial=0.0), np.nanmax(np.abs(v - py), initial=0.0))
    same = lambda u, v: (u.view(np.uint32) == v.view(np.uint32)) | (np.isnan(u) & np.isnan(v)) | (u == v)
    differ = ~(same(ox, nx) & same(oy, ny))
    return float(differ.mean()), float(dist)


# ---- section 1: every differing voxel explained -----------------------------------------------------------------------
def _same_bits(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def explain_warp(orc, geo, got, want, fea, src, ref, depth):
    """got / want (B,C,D,H,W) float32: the kernel's and the oracle's warp.  -> (messages, number of explained voxels).
    NaN masks must be equal and every other value equal as uint32, except at voxels (b,d,y,x) where ALL channels of `got`
    equal, bit for bit, the oracle's sampler at one of the eight neighbours of the oracle's own float32 coordinate
    (+-1 ulp in sample, in line, or in both) -- the only thing two float64 evaluations of the geometry can turn into.
    At most max(1, 1e-4 * voxels) voxels may be explained that way."""
    msgs = []
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return ["shape %s != %s" % (got.shape, want.shape)], 0
    B, C, D, H, W = got.shape
    bad = ~_same_bits(got, want)
    vox = bad.any(1)                                                              # (B,D,H,W)
    nvox = int(vox.sum())
    if nvox == 0:
        return msgs, 0
    cap = max(1, int(MAX_EXPLAINED * vox.size))
    if nvox > cap:
        first = tuple(np.argwhere(vox)[0])
        return ["%d of %d voxels differ (cap %d); first (b,d,y,x) = %s: tile (%d,%d) chunk %d" %
                (nvox, vox.size, cap, first, first[3] // TILE_X, first[2] // TILE_Y, first[1] // DCH)], 0
    a, b_ = oracle_coords(orc, geo, src, ref, depth, H, W)
    cx, cy = (a.astype(np.float32), b_.astype(np.float32))
    for (b, d, y, x) in np.argwhere(vox):
        x0, y0 = cx[b, d, y, x], cy[b, d, y, x]
        cand_x = [np.nextafter(x0, np.float32(-np.inf)), x0, np.nextafter(x0, np.float32(np.inf))]
        cand_y = [np.nextafter(y0, np.float32(-np.inf)), y0, np.nextafter(y0, np.float32(np.inf))]
        nb = np.array([(u, v) for u in cand_x for v in cand_y if not (u == x0 and v == y0)], np.float32)
        if geo == "rpc":
            gx, gy = grid_from_pixel32(nb[:, 0], nb[:, 1], H, W)
        else:
            gx, gy = nb[:, 0], nb[:, 1]
        grid = np.stack([gx, gy], -1).reshape(1, 1, -1, 2)
        alt = orc.grid_sample(fea[b:b + 1], grid)[0, :, 0, :]                      # (C, 8)
        g = got[b, :, d, y, x]
        if not _same_bits(alt, g[:, None]).all(0).any():
            msgs.append("voxel (b,d,y,x) = (%d,%d,%d,%d) [tile (%d,%d), chunk %d]: got %r, oracle %r, no +-1 ulp neighbour of (%r, %r) gives it"
                        % (b, d, y, x, x // TILE_X, y // TILE_Y, d // DCH, g[:4], want[b, :4, d, y, x], x0, y0))
            if len(msgs) >= 5:
                break
    return msgs, nvox


# ---- section 2: an independent float64 sampler and its derived bound ---------------------------------------------------
def sampler_f64(fea, px, py, H, W):
    """numpy float64 restatement of the reference's rule: pixel -> g = p / ((W-1)/2) - 1 -> x = (g+1) W/2 - 0.5 -> bilinear
    with zero padding.  fea (B,C,H,W), px / py (B,D,H,W) float64 -> value (B,C,D,H,W), sum |w f| (same shape), both float64.
    A non-finite coordinate drops all four taps."""
    f = np.asarray(fea, np.float64)
    B, C = f.shape[:2]
    with np.errstate(divide="ignore", invalid="ignore"):
        x = (px / ((W - 1) / 2.0) - 1.0 + 1.0) * (W / 2.0) - 0.5
        y = (py / ((H - 1) / 2.0) - 1.0 + 1.0) * (H / 2.0) - 0.5
    fin = np.isfinite(x) & np.isfinite(y) & (np.abs(x) < 2.0 ** 30) & (np.abs(y) < 2.0 ** 30)
    x, y = np.where(fin, x, -10.0), np.where(fin, y, -10.0)
    x0, y0 = np.floor(x), np.floor(y)
    wx, wy = x - x0, y - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    val = np.zeros((B, C) + px.shape[1:])
    mag = np.zeros_like(val)
    bi = np.arange(B).reshape(B, 1, 1, 1)
    for dy, dx, w in ((0, 0, (1 - wy) * (1 - wx)), (0, 1, (1 - wy) * wx), (1, 0, wy * (1 - wx)), (1, 1, wy * wx)):
        xi, yi = x0 + dx, y0 + dy
        ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        w = np.where(ok, w, 0.0)
        xi, yi = np.clip(xi, 0, W - 1), np.clip(yi, 0, H - 1)
        for c in range(C):
            t = f[:, c][bi, yi, xi]
            val[:, c] += w * t
            mag[:, c] += w * np.abs(t)
    return val, mag


def sampler_bound(px, py, mag, H, W):
    """|float32 chain - sampler_f64| is at most this, per voxel (B,C,D,H,W).  Derivation, u = 2^-24, per axis (x shown):
        p^ = fl32(p)                      error u |p|
        q^ = p^ / fl32((W-1)/2)           error 2u |q| in total, q = 2 p / (W-1)    (the divisor is exact)
        g^ = q^ - 1,  t^ = g^ + 1         error 2u |q| + u |g| + u |q|  <=  u (4 |q| + 1)
        x^ = fma(t^, W/2, -0.5)           error (W/2) u (4 |q| + 1) + u |x|  <=  u ((5/2) |q| W + W/2 + 1/2)
    i.e. e_x = u (5 |p| W / (W-1) + (W+1)/2): for a coordinate inside the image at most 5.5 + 1/W ulps (of 2^-24) of W.  The
    pinhole chain normalises in float64 and rounds once (u |g| instead of the first three lines): it is inside the same
    bound.  To that the float64 geometry adds the project's own 1e-8 px (two float64 evaluations differ by ~1e-9 px).
    The interpolant is Lipschitz with constant LIPSCHITZ per axis (smooth_features), so the value moves by at most
    LIPSCHITZ (e_x + e_y); the float32 weights (1 - w, two products: 3 roundings) and the four-term fma chain (4 roundings)
    add at most 8 u sum |w f|.  Second-order terms: 1 %."""
    ex = U32 * (5.0 * np.abs(px) * W / max(W - 1, 1) + (W + 1) / 2.0) + 1e-8
    ey = U32 * (5.0 * np.abs(py) * H / max(H - 1, 1) + (H + 1) / 2.0) + 1e-8
    e = np.where(np.isfinite(px) & np.isfinite(py), ex + ey, 0.0)[:, None]
    return 1.01 * (LIPSCHITZ * e + 8.0 * U32 * mag)


# ---- section 4: float64 scatter (the backward) from the oracle's float32 taps --------------------------------------------
def taps_from_grid(gx, gy, H, W):
    """numpy restatement of tap_from_grid (csrc/smvs_device.h) / make_tap_norm (oracle.c): -> flat offsets (4, ...) int64
    with -1 for a dropped tap, float32 weights (4, ...) in the order nw, ne, sw, se.  The one fma of the sequence is
    evaluated in float64 and rounded once: (g+1) has 24 bits and W/2 at most 12, the product is exact and so is the sum
    unless the product is below 2^-18, where the result is -0.5 either way."""
    gx, gy = np.asarray(gx, np.float32), np.asarray(gy, np.float32)
    one = np.float32(1)
    with np.errstate(invalid="ignore", over="ignore"):
        x = ((gx + one).astype(np.float64) * (W * 0.5) - 0.5).astype(np.float32)
        y = ((gy + one).astype(np.float64) * (H * 0.5) - 0.5).astype(np.float32)
        xw, yn = np.floor(x), np.floor(y)
        w = (x - xw).astype(np.float32); e = (one - w).astype(np.float32)
        n = (y - yn).astype(np.float32); s = (one - n).astype(np.float32)
        wts = np.stack([s * e, s * w, n * e, n * w]).astype(np.float32)
        xin0, xin1 = (xw >= 0) & (xw <= W - 1), (xw >= -1) & (xw <= W - 2)
        yin0, yin1 = (yn >= 0) & (yn <= H - 1), (yn >= -1) & (yn <= H - 2)
    x0 = np.where(xin0 | xin1, xw, 0).astype(np.int64)
    y0 = np.where(yin0 | yin1, yn, 0).astype(np.int64)
    base = y0 * W + x0
    off = np.stack([np.where(xin0 & yin0, base, -1), np.where(xin1 & yin0, base + 1, -1),
                    np.where(xin0 & yin1, base + W, -1), np.where(xin1 & yin1, base + W + 1, -1)])
    return off, wts


def sample_from_taps(fea, off, wts):
    """float64 sample of fea (B,C,H,W) at taps of shape (4,B,D,H,W): exact products of the float32 weights, float64 sums.
    A dropped tap reads 0 and is still multiplied by its weight, as in ATen: a NaN weight (non-finite coordinate) gives NaN."""
    B, C, H, W = fea.shape
    f = np.asarray(fea, np.float64).reshape(B, C, H * W)
    out = np.zeros((B, C) + off.shape[2:])
    for b in range(B):
        for k in range(4):
            o = off[k, b]
            with np.errstate(invalid="ignore"):
                out[b] += np.where(o >= 0, f[b][:, np.maximum(o, 0)], 0.0) * wts[k, b].astype(np.float64)
    return out


def scatter_f64(grad_out, off, wts, H, W):
    """grad_src (B,C,H,W) of the warp in float64: every voxel adds grad_out * weight to its (up to) four taps.  Also
    sum |g w| per cell (B,C,H,W) and the number of contributions per cell (B,H,W): the float32 summation bound is
    (n + 1) u sum |g w| -- n - 1 additions in any order plus one rounding per product."""
    g = np.asarray(grad_out, np.float64)
    B, C = g.shape[:2]
    HW = H * W
    ref, mag, cnt = np.zeros((B, C, HW)), np.zeros((B, C, HW)), np.zeros((B, HW), np.int64)
    for b in range(B):
        for k in range(4):
            o = off[k, b].ravel()
            ok = o >= 0
            idx = o[ok]
            w = wts[k, b].ravel()[ok].astype(np.float64)
            cnt[b] += np.bincount(idx, minlength=HW)
            for c in range(C):
                t = g[b, c].ravel()[ok] * w
                ref[b, c] += np.bincount(idx, weights=t, minlength=HW)
                mag[b, c] += np.bincount(idx, weights=np.abs(t), minlength=HW)
    return ref.reshape(B, C, H, W), mag.reshape(B, C, H, W), cnt.reshape(B, H, W)


def check_backward(got, grad_out, off, wts, H, W, what=""):
    """got (B,C,H,W) float32 from the kernel -> messages.  Every cell within (n + 1) 2^-24 sum |g w| of the float64
    scatter; a cell nothing contributes to exactly 0.0 (bit pattern of +0)."""
    ref, mag, cnt = scatter_f64(grad_out, off, wts, H, W)
    got = np.asarray(got)
    msgs = []
    bound = (cnt[:, None] + 1) * U32 * mag
    err = np.abs(got.astype(np.float64) - ref)
    bad = ~(err <= bound)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        msgs.append("%s: %d cells outside the float32 summation bound; first %s: got %r, float64 %r, bound %.3g (n = %d)"
                    % (what, int(bad.sum()), i, got[i], ref[i], bound[i], cnt[i[0], i[2], i[3]]))
    empty = np.broadcast_to((cnt == 0)[:, None], got.shape)
    if (got[empty].view(np.uint32) != 0).any():
        msgs.append("%s: %d cells without a contribution are not +0.0" % (what, int((got[empty].view(np.uint32) != 0).sum())))
    worst = float((err / np.maximum(bound, 1e-300))[cnt[:, None].repeat(got.shape[1], 1) > 0].max(initial=0.0))
    return msgs, worst, int(cnt.max(initial=0))


# ---- section 5: regressions ---------------------------------------------------------------------------------------------
REG_D = (1, 2, 3, 4, 5, 8, 48, 64, 192, 384)
REG_N = ((1, 1, 1), (1, 1, 255), (1, 16, 16), (1, 1, 257), (3, 33, 70))            # (B, H, W): B H W = 1, 255, 256, 257, 6930
REG_BIG = (1, 384, 768)
TOL_DEPTH, TOL_VAR_R, TOL_VAR_A, TOL_CONF_R, TOL_CONF_A = 1e-4, 1e-5, 1e-4, 1e-5, 1e-6    # GPU against the oracle (test_window_regression_golden)
TOL_PROJECT = 1e-3                                                                 # the project's height tolerance, metres
WINDOW_CONF_TOL = 1e-5
MAX_AT_RISK = 1e-3


def reg_cases():
    """(D, (B,H,W), height kind): every D and every pixel count appears; kinds alternate so that each of them meets small,
    large, odd and even D."""
    kinds = ("planes", "tensor")
    out = []
    for i, D in enumerate(REG_D):
        out.append((D, REG_N[i % len(REG_N)], kinds[i % 2]))
        out.append((D, REG_N[(i + 2) % len(REG_N)], kinds[(i + 1) % 2]))
    return out


def reg_scene(D, bhw, kind, seed, sigma=3.0):
    """logits (B,D,H,W) ~ N(0, sigma^2) float32, heights in the project's 0 - 400 m range as (B,D) planes or a jittered
    (B,D,H,W) tensor.  The derived band index_band(D) covers 2 D (D-1) 2^-24 of the unit interval: 2.7e-4 at D = 48 but
    4.4e-3 at D = 192 and 1.8e-2 at D = 384, so random logits cannot stay under the 1e-3 cap on excused pixels there.  For
    D > 64 the pixels inside the band are drawn again until none is left: those cases allow no excused pixel at all, and
    the truncation rule is exercised where at-risk pixels occur by themselves (D <= 64)."""
    B, H, W = bhw
    rng = np.random.default_rng(seed)
    reg = (rng.standard_normal((B, D, H, W)) * sigma).astype(np.float32)
    planes = np.linspace(0.0, 400.0, D, dtype=np.float32)[None].repeat(B, 0) if D > 1 else np.full((B, 1), 200.0, np.float32)
    if D > 64:
        for _ in range(50):
            risk = at_risk(dict(fidx=_fidx64(reg)), D)
            if not risk.any():
                break
            b, y, x = np.nonzero(risk)
            reg[b, :, y, x] = (rng.standard_normal((len(b), D)) * sigma).astype(np.float32)
    if kind == "planes":
        return reg, planes
    return reg, np.clip(planes.astype(np.float64)[:, :, None, None] + rng.normal(0, 2.0, (B, D, H, W)), 0.0, 400.0).astype(np.float32)


def _fidx64(reg):
    r = np.asarray(reg, np.float32).astype(np.float64)
    e = np.exp(r - r.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True) * np.arange(r.shape[1]).reshape(1, -1, 1, 1)).sum(1)


def regress_f64(reg, heights, lamb=None):
    """softmax, expectation, max probability, window-4 confidence and UCS spread in numpy float64 from the float32 logits.
    -> dict(depth, conf_max, fidx, conf_win, conf_lo, conf_hi, var): conf_lo / conf_hi are the window sums for the index
    below / above trunc(sum p d) (what a float32 sum p d on the other side of an integer selects)."""
    r = np.asarray(reg, np.float32).astype(np.float64)
    B, D, H, W = r.shape
    h = np.asarray(heights, np.float32).astype(np.float64)
    h = h[:, :, None, None] if h.ndim == 2 else h
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(r - r.max(1, keepdims=True))
        p = e / e.sum(1, keepdims=True)
        depth = (p * h).sum(1)
        fidx = (p * np.arange(D).reshape(1, D, 1, 1)).sum(1)
    pp = np.concatenate([np.zeros((B, 2, H, W)), np.nan_to_num(p), np.zeros((B, 3, H, W))], 1)      # plane d at d + 2

    def window(idx):
        idx = np.clip(idx, 0, D - 1)[:, None]
        return sum(np.take_along_axis(pp, idx + 2 + k, 1) for k in (-1, 0, 1, 2))[:, 0]
    idx = np.nan_to_num(np.trunc(fidx)).astype(np.int64)
    out = dict(depth=depth, conf_max=p.max(1), fidx=fidx, conf_win=window(idx), conf_lo=window(idx - 1), conf_hi=window(idx + 1), p=p)
    if lamb is not None:
        out["var"] = lamb * np.sqrt((p * (h - depth[:, None]) ** 2).sum(1))
    return out


def index_band(D):
    """float32 accumulation bound of sum_d p_d d: D additions and D products, each relative 2^-24, of a sum below D - 1."""
    return D * U32 * max(D - 1, 1)


def at_risk(f64, D):
    """Pixels whose float64 sum p d lies within index_band of an integer 1 .. D-1: the only ones where truncation may pick
    another index (the sum is never negative, and an index above D-1 is clamped)."""
    f = f64["fidx"]
    k = np.rint(f)
    with np.errstate(invalid="ignore"):
        return (np.abs(f - k) <= index_band(D)) & (k >= 1) & (k <= D - 1)


def check_window_conf(conf, f64, D):
    """conf (B,H,W) float32 from the kernel -> (messages, share of excused pixels).  A pixel off the float64 confidence by
    more than 1e-5 must be at risk AND match the float64 confidence of a neighbouring index within 1e-5; such pixels are
    at most 1e-3 of the case (and at least one pixel is allowed)."""
    c = np.asarray(conf, np.float64)
    off = ~(np.abs(c - f64["conf_win"]) <= WINDOW_CONF_TOL)
    nb = (np.abs(c - f64["conf_lo"]) <= WINDOW_CONF_TOL) | (np.abs(c - f64["conf_hi"]) <= WINDOW_CONF_TOL)
    excused = off & at_risk(f64, D) & nb
    msgs = []
    unexplained = off & ~excused
    if unexplained.any():
        i = tuple(np.argwhere(unexplained)[0])
        msgs.append("%d pixels off the float64 window confidence without cause; first %s: got %r, float64 %r (sum p d = %r)"
                    % (int(unexplained.sum()), i, c[i], f64["conf_win"][i], f64["fidx"][i]))
    if excused.sum() > max(1, MAX_AT_RISK * c.size):
        msgs.append("%d of %d pixels excused" % (int(excused.sum()), c.size))
    return msgs, float(excused.mean())


def stream_f64(reg, heights):
    """The three float64 accumulators of the streaming regression after all planes, by numpy: sum exp, sum h exp, max exp."""
    r = np.asarray(reg, np.float32).astype(np.float64)
    h = np.asarray(heights, np.float32).astype(np.float64)
    h = h[:, :, None, None] if h.ndim == 2 else h
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(r)
        es, di, mx = np.zeros(r.shape[:1] + r.shape[2:]), np.zeros(r.shape[:1] + r.shape[2:]), np.zeros(r.shape[:1] + r.shape[2:])
        for d in range(r.shape[1]):                                                # plane order, like the accumulators
            es = es + e[:, d]
            di = h[:, d] * e[:, d] + di
            mx = np.where(mx < e[:, d], e[:, d], mx)
    return es, di, mx


# ---- section 6: projectors and the homography composition ---------------------------------------------------------------
PROJECT_N = (1, 255, 256, 257)
PROJECT_BIG = 5120 * 5120
COMPOSE_N = (1, 63, 64, 65, 1000)


def project_points(n, H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, W, n), rng.uniform(0, H, n), rng.uniform(0.0, 400.0, n)


def compose_scene(n, seed):
    """n pairs of projection-like matrices K [R|t] with bottom row 0 0 0 1, as the networks receive them."""
    rng = np.random.default_rng(seed)
    out = np.zeros((2, n, 4, 4))
    for v in range(2):
        for i in range(n):
            f = rng.uniform(500, 3000)
            K = np.array([[f, 0, rng.uniform(100, 1000)], [0, f, rng.uniform(100, 1000)], [0, 0, 1.0]])
            a, b, c = rng.normal(0, 0.1, 3)
            Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
            Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
            Rx = np.array([[1, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]])
            E = np.eye(4)
            E[:3, :3] = Rz @ Ry @ Rx
            E[:3, 3] = rng.normal(0, 50, 3)
            out[v, i] = np.eye(4)
            out[v, i, :3] = K @ E[:3]
    return out[0], out[1]


def pivot_matrices():
    """Reference matrices whose elimination needs a row swap at column 0, 1 and 2 (a zero on the diagonal when that column
    is reached), and two permutation matrices -- for those the inverse, and src @ inverse for an integer src, is exact."""
    z0 = np.array([[0.0, 2, 1, 3], [4, 1, 0, 2], [1, 3, 5, 1], [2, 0, 1, 6]])
    z1 = np.array([[4.0, 2, 1, 3], [2, 1, 3, 2], [1, 3, 5, 1], [2, 0, 1, 6]])       # after column 0: row 1 = (0, 0, 2.5, 0.5)
    z2 = np.array([[4.0, 0, 1, 3], [0, 2, 1, 2], [4, 2, 2, 1], [2, 0, 1, 6]])       # after columns 0, 1: row 2 = (0, 0, 0, -4)
    p1 = np.eye(4)[[1, 2, 3, 0]]
    p2 = np.eye(4)[[3, 0, 2, 1]]
    return [z0, z1, z2, p1, p2]


def compose_bound(src, ref):
    """|GPU - src @ inv(ref)| entrywise: 16 * 2^-52 * cond(ref) * ||src|| * ||inv(ref)|| (2-norms)."""
    inv = np.linalg.inv(ref)
    return 16 * 2.0 ** -52 * np.linalg.cond(ref) * np.linalg.norm(src, 2) * np.linalg.norm(inv, 2)
