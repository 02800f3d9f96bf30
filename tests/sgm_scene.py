"""The case matrix of the SGM tests (tests/test_sgm_cpu.py, tests/test_sgm_gpu.py), the comparison they share, and the
end-to-end scene: three RPC views of a smooth surface with a plateau, textured on the ground.  numpy only at import."""
import numpy as np

import sgm_oracle as so

VOID = so.VOID
TILE_H, TILE_W = 8, 32                                       # SG_TILE_H, SG_TILE_W of satmvs_amd/csrc/sgm.hip
GRIDS = ((1, 1), (1, 70), (67, 1), (2, 2), (7, 7), (TILE_H - 1, TILE_W + 1), (TILE_H, TILE_W), (TILE_H + 1, TILE_W - 1), (2 * TILE_H + 1, 2 * TILE_W + 1))
AGG_D = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 256)
AGG_GRIDS = ((1, 1), (1, 70), (67, 1), (2, 2), (3, 67), (33, 47), (64, 96))


def compare(got, want, what):
    """Equal shapes, dtypes and bits; no element excused."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
    bad = g != w
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())


# ---- census ------------------------------------------------------------------------------------------------------------------------
def warped_volume(rng, B, Dc, H, W, levels=6, holes=0.15, cov_min=0.999):
    """(B, 2, Dc, H, W): an image of few levels (many equal intensities) and a coverage with patches below cov_min, values exactly
    cov_min and one ulp below it."""
    cm = np.float32(cov_min)
    img = rng.integers(0, levels, (B, Dc, H, W)).astype(np.float32)
    cov = np.ones((B, Dc, H, W), np.float32)
    kind = rng.random((B, Dc, H, W))
    cov[kind < holes] = rng.random(int((kind < holes).sum())).astype(np.float32) * np.float32(0.99)
    cov[(kind >= holes) & (kind < holes + 0.05)] = cm
    cov[(kind >= holes + 0.05) & (kind < holes + 0.08)] = np.nextafter(cm, np.float32(0))
    return np.stack([img, cov], axis=1)


def census_case(seed, B, H, W, Dc, S, specials=False, levels=6, holes=0.15, cov_min=0.999):
    """-> (ref (B, H, W), [S warped volumes], cov_min)."""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, levels, (B, H, W)).astype(np.float32)
    warped = [warped_volume(rng, B, Dc, H, W, levels, holes, cov_min) for _ in range(S)]
    if specials:                                             # NaN and both infinities in every image, a NaN coverage
        for a in [ref] + [w[:, 0] for w in warped]:
            flat = a.reshape(-1)
            pick = rng.choice(flat.size, max(3, flat.size // 10), replace=False)
            flat[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), pick.size)
        warped[0][:, 1].reshape(-1)[:: 7] = np.nan
    return ref, warped, cov_min


def census_matrix():
    """(name, ref, warped, radius, cov_min): every grid at radius 2 and two sources, every radius, S = 1, 2, 3, 7, Dc = 1, 7, 8, 9,
    special values, a source with no covered voxel, and nothing covered at all."""
    out = []
    for k, (H, W) in enumerate(GRIDS):
        out.append(("grid %dx%d" % (H, W),) + census_case(100 + k, 1, H, W, 3, 2)[:2] + (2, 0.999))
    for r in (1, 2, 3):
        out.append(("radius %d" % r,) + census_case(120 + r, 2, 11, 37, 5, 3)[:2] + (r, 0.999))
    for S in (1, 2, 3, 7):
        out.append(("S %d" % S,) + census_case(130 + S, 1, 9, 35, 2, S)[:2] + (3, 0.999))
    for Dc in (1, 7, 8, 9, 16, 17):
        out.append(("Dc %d" % Dc,) + census_case(140 + Dc, 1, 10, 34, Dc, 2)[:2] + (1, 0.999))
    for r in (1, 3):
        out.append(("specials r%d" % r,) + census_case(150 + r, 1, 12, 40, 4, 2, specials=True)[:2] + (r, 0.999))
    out.append(("cov_min 0.5",) + census_case(160, 1, 9, 33, 3, 2, cov_min=0.5)[:2] + (2, 0.5))
    ref, warped, _ = census_case(161, 1, 9, 33, 3, 2, holes=0.0)
    warped[1][:, 1] = 0.5                                    # the second source covers nothing: the first alone decides
    out.append(("one source void", ref, warped, 2, 0.999))
    ref, warped, _ = census_case(162, 1, 9, 33, 3, 2)
    for w in warped:
        w[:, 1] = 0.0
    out.append(("all void", ref, warped, 2, 0.999))
    out.append(("equal intensities",) + census_case(163, 1, 9, 33, 3, 2, levels=1, holes=0.0)[:2] + (2, 0.999))
    return out


# ---- aggregation -------------------------------------------------------------------------------------------------------------------
def random_cost(rng, B, H, W, D, top=900, voids=0.05):
    c = rng.integers(0, top, (B, H, W, D)).astype(np.uint16)
    c[rng.random((B, H, W, D)) < voids] = VOID
    return c


def valley_cost(rng, B, H, W, D, voids=0.03):
    """One valley per pixel about a smooth surface of plane indices, with noise: what a matching cost looks like."""
    y, x = np.mgrid[0:H, 0:W]
    centre = (D - 1) * (0.5 + 0.35 * np.sin(x / 9.0 + 0.3) * np.cos(y / 7.0))
    centre = centre + np.where((x > W // 2) & (y > H // 3), 0.2 * D, 0.0)
    d = np.arange(D)
    c = np.minimum(np.abs(d[None, None, None, :] - centre[None, :, :, None]) * 60.0, 600.0) + rng.integers(0, 120, (B, H, W, D))
    c = c.astype(np.uint16)
    c[rng.random((B, H, W, D)) < voids] = VOID
    return c


def guide_image(rng, B, H, W):
    g = rng.integers(0, 256, (B, H, W)).astype(np.uint8)
    g[:, :, W // 2:] //= 4                                   # an edge down the middle
    return g


def aggregate_matrix():
    """(name, cost, kwargs of so.aggregate): every D on a small grid at both path counts, every grid, B = 2, the penalty edge cases,
    guides, and the three kinds of volume."""
    rng = np.random.default_rng(200)
    out = []
    for D in AGG_D:
        for paths in (4, 8):
            out.append(("D %d paths %d" % (D, paths), random_cost(rng, 1, 5, 9, D), dict(P1=16, P2=96, paths=paths)))
    for H, W in AGG_GRIDS:
        D = 5 if H * W > 1000 else 33
        out.append(("grid %dx%d" % (H, W), random_cost(rng, 1, H, W, D), dict(P1=16, P2=96, paths=8)))
        out.append(("grid %dx%d paths 4" % (H, W), random_cost(rng, 1, H, W, D), dict(P1=7, P2=50, paths=4)))
    out.append(("B 2", random_cost(rng, 2, 9, 13, 40), dict(P1=16, P2=96, paths=8)))
    out.append(("B 2 D 70", valley_cost(rng, 2, 12, 17, 70), dict(P1=16, P2=96, paths=8)))
    out.append(("P1 0", random_cost(rng, 1, 9, 13, 20), dict(P1=0, P2=96, paths=8)))
    out.append(("P1 = P2", random_cost(rng, 1, 9, 13, 20), dict(P1=96, P2=96, paths=8)))
    out.append(("P1 = P2 = 0", random_cost(rng, 1, 9, 13, 20), dict(P1=0, P2=0, paths=8)))
    for paths in (4, 8):                                     # the largest P2 with paths (cost_max + P2) <= 65535 (65535 is odd: equality cannot be met)
        cost_max = 768
        P2 = 65535 // paths - cost_max
        out.append(("P2 at the bound, paths %d" % paths, random_cost(rng, 1, 7, 11, 12, top=2000), dict(P1=P2 // 3, P2=P2, paths=paths, cost_max=cost_max)))
    out.append(("cost_max 65535 / 4", random_cost(rng, 1, 6, 8, 9, top=65535), dict(P1=0, P2=0, paths=4, cost_max=65535 // 4, void_cost=65535 // 4)))
    out.append(("costs above cost_max", random_cost(rng, 1, 9, 13, 20, top=5000, voids=0.2), dict(P1=16, P2=96, paths=8, cost_max=300, void_cost=300)))
    out.append(("void_cost 0", random_cost(rng, 1, 9, 13, 20, voids=0.3), dict(P1=16, P2=96, paths=8, void_cost=0)))
    for alpha in (0, 1, 7):
        out.append(("guide alpha %d" % alpha, valley_cost(rng, 2, 11, 15, 34), dict(P1=10, P2=120, paths=8, guide=guide_image(rng, 2, 11, 15), alpha=alpha, p2_min=20)))
    out.append(("guide paths 4", random_cost(rng, 1, 11, 15, 66), dict(P1=10, P2=120, paths=4, guide=guide_image(rng, 1, 11, 15), alpha=3, p2_min=10)))
    out.append(("valleys", valley_cost(rng, 1, 33, 47, 48), dict(P1=16, P2=96, paths=8)))
    out.append(("constant", np.full((1, 9, 13, 20), 123, np.uint16), dict(P1=16, P2=96, paths=8)))
    return out


# ---- select ------------------------------------------------------------------------------------------------------------------------
def select_matrix():
    """(name, sum, depth, kwargs of so.select)."""
    rng = np.random.default_rng(300)
    out = []
    B, H, W, D = 2, 7, 9, 12
    planes = np.stack([np.linspace(170.0, 260.0, D), np.linspace(90.0, 10.0, D) ** 1.1]).astype(np.float32)      # rising, and falling unevenly
    per_pixel = (planes[:, :, None, None] + rng.normal(0, 1.0, (B, D, H, W))).astype(np.float32)
    few = rng.integers(0, 6, (B, H, W, D)).astype(np.uint16)                     # many ties, den = 0, winners at both ends
    wide = rng.integers(0, 6000, (B, H, W, D)).astype(np.uint16)
    cost = random_cost(rng, B, H, W, D, voids=0.5)
    cost[0, 0, 0] = VOID
    cost[0, 0, 1, 1:] = VOID
    for name, s in (("few", few), ("wide", wide)):
        for dname, depth in (("planes", planes), ("per pixel", per_pixel)):
            out.append(("%s, %s" % (name, dname), s, depth, dict()))
            out.append(("%s, %s, u 99" % (name, dname), s, depth, dict(uniqueness=99)))
            out.append(("%s, %s, u 15 with cost" % (name, dname), s, depth, dict(uniqueness=15, cost=cost, min_support=6)))
    out.append(("min_support 0", wide, planes, dict(cost=cost, min_support=0)))
    out.append(("min_support 1", wide, planes, dict(cost=cost, min_support=1)))
    out.append(("min_support D", wide, planes, dict(cost=cost, min_support=D)))
    # sums exactly on the uniqueness threshold and one off it: u = 20, the winner 800: a far plane at 1000 passes (1000 * 80 = 800 * 100), 999 rejects
    edge = np.full((1, 1, 4, 6), 5000, np.uint16)
    edge[0, 0, :, 2] = 800
    edge[0, 0, 0, 5] = 1000
    edge[0, 0, 1, 5] = 999
    edge[0, 0, 2, 3] = 801                                   # a neighbour of the winner: never tested
    edge[0, 0, 3, 0] = 999
    out.append(("uniqueness threshold", edge, np.linspace(0, 50, 6, dtype=np.float32)[None], dict(uniqueness=20)))
    nan_depth = planes.copy()
    nan_depth[0, 3] = np.nan
    nan_depth[1, 5] = np.inf
    out.append(("NaN and Inf heights", few, nan_depth, dict()))
    out.append(("D 1", rng.integers(0, 9, (1, 3, 4, 1)).astype(np.uint16), np.array([[7.5]], np.float32), dict(uniqueness=50)))
    out.append(("D 2", rng.integers(0, 9, (1, 3, 4, 2)).astype(np.uint16), np.array([[7.5, 9.0]], np.float32), dict(uniqueness=50)))
    out.append(("D 256", rng.integers(0, 65535, (1, 5, 6, 256)).astype(np.uint16), np.linspace(0, 500, 256, dtype=np.float32)[None], dict(uniqueness=5)))
    out.append(("large sums", rng.integers(60000, 65536, (1, 5, 6, 9)).astype(np.uint16), np.linspace(0, 8, 9, dtype=np.float32)[None], dict(uniqueness=3)))
    return out


# ---- the end-to-end scene ------------------------------------------------------------------------------------------------------------
H, W, D = 64, 96, 48
H_LO, H_HI = 170.0, 260.0
DH = (H_HI - H_LO) / (D - 1)
BORDER = 8
_CACHE = {}


def planes():
    return np.linspace(H_LO, H_HI, D, dtype=np.float32)[None]


def _gauss_fields(rng, shape, sigmas):
    fy, fx = np.fft.fftfreq(shape[0])[:, None], np.fft.rfftfreq(shape[1])[None, :]
    out = np.zeros(shape)
    for k, sg in enumerate(sigmas):
        spec = np.fft.rfft2(rng.standard_normal(shape)) * np.exp(-2.0 * (np.pi * sg) ** 2 * (fy * fy + fx * fx))
        t = np.fft.irfft2(spec, s=shape)
        out += t / t.std() / np.sqrt(k + 1.0)
    return out / out.std()


def scene(seed=7):
    """-> (images: 3 x (H, W) float32, rpc (3, 170) float64, truth: 3 x (H, W) float32 heights seen by each view).
    A surface of 200 +- 12 m with a +30 m plateau behind steep sigmoid edges; a ground texture of three octaves of Gaussian-filtered
    noise at 1.5, 5 and 16 ground cells (two cells per pixel); every view samples the texture where its pixel's ray meets the surface
    (fixed-point iteration on the inverse RPC).  The views tilt by 0 and +-0.4: 0.096 px of parallax per metre, 0.18 px per plane."""
    if seed in _CACHE:
        return _CACHE[seed]
    from satmvs_amd import rpc_synth
    rpc = rpc_synth.make_view_rpcs(3, H, W, seed=seed, tilts=(0.0, 0.4, -0.4), gsd=1.0)
    rng = np.random.default_rng(seed + 1)
    lat0, lon0, ls, os_ = rpc[0, 2], rpc[0, 3], rpc[0, 7], rpc[0, 8]
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))  # noqa: E731

    def surface(lat, lon):
        u, v = (lat - lat0) / ls, (lon - lon0) / os_
        plateau = sig((0.3 - np.abs(u - 0.05)) / 0.04) * sig((0.35 - np.abs(v + 0.1)) / 0.04)
        return 200.0 + 12.0 * np.sin(2.1 * u + 0.4) * np.cos(1.7 * v - 0.3) + 30.0 * plateau

    gh, gw = int(2 * H * 1.2) + 8, int(2 * W * 1.2) + 8
    tex = _gauss_fields(rng, (gh, gw), (1.5, 5.0, 16.0))
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    images, truth = [], []
    for v in range(3):
        h = np.full(H * W, 200.0)
        for _ in range(40):
            lat, lon = rpc_synth.photo2obj(rpc[v], xx.ravel(), yy.ravel(), h)
            h = surface(lat, lon)
        lat, lon = rpc_synth.photo2obj(rpc[v], xx.ravel(), yy.ravel(), h)
        u, w_ = (lat - lat0) / ls, (lon - lon0) / os_
        fy = np.clip((1.0 - (u + 1.0) * 0.5) * (gh - 1), 0, gh - 1.001)
        fx = np.clip((w_ + 1.0) * 0.5 * (gw - 1), 0, gw - 1.001)
        y0, x0 = np.floor(fy).astype(np.int64), np.floor(fx).astype(np.int64)
        wy, wx = fy - y0, fx - x0
        img = tex[y0, x0] * (1 - wy) * (1 - wx) + tex[y0, x0 + 1] * (1 - wy) * wx + tex[y0 + 1, x0] * wy * (1 - wx) + tex[y0 + 1, x0 + 1] * wy * wx
        images.append((128.0 + 40.0 * img).reshape(H, W).astype(np.float32))
        truth.append(h.reshape(H, W).astype(np.float32))
    _CACHE[seed] = images, rpc, truth
    return _CACHE[seed]


def quality(height, truth):
    """(median |error| [m], share within 2 DH) over the pixels BORDER in from the edge; a rejected pixel counts as wrong."""
    e = np.abs(height.astype(np.float64) - truth)[BORDER:-BORDER, BORDER:-BORDER]
    e = np.where(np.isnan(e), np.inf, e)
    return float(np.median(e)), float((e <= 2 * DH).mean())


def check_quality(sgm_height, raw_height, truth):
    """The conditions of the scene: the median within DH, 90 % within 2 DH, and SGM strictly better than the raw winner on both."""
    med, share = quality(sgm_height, truth)
    raw_med, raw_share = quality(raw_height, truth)
    print("SGM: median %.3f m (%.2f DH), within 2 DH %.3f; raw winner: median %.3f m, within 2 DH %.3f" % (med, med / DH, share, raw_med, raw_share))
    assert med <= DH and share >= 0.90, (med, share)
    assert med < raw_med and share > raw_share, (med, raw_med, share, raw_share)
    return med, share, raw_med, raw_share


def oracle_heights(ref, warped, depth, radius=2, P1=16, P2=96):
    """The oracle's chain on given warped volumes -> (sgm (index, height, min_sum, support), raw winner likewise, cost, sum)."""
    cost = so.census_cost(ref, warped, radius, 0.999)
    total = so.aggregate(cost, P1, P2, 8, void_cost=4 * len(so.offsets(radius)))
    raw = np.where(cost == VOID, 4 * len(so.offsets(radius)), np.minimum(cost, 768)).astype(np.uint16)
    return so.select(total, depth, 0, cost, 1), so.select(raw, depth, 0, cost, 1), cost, total
