"""The case matrix of the stack fusion tests (test_dsm_stack_cpu.py, test_dsm_stack_gpu.py): the smallest stacks at which
smvs_dsm_stack_select / smvs_dsm_stack_fuse can still go wrong.  numpy only, seeded, nothing read from disk.

  destinations  1 x 1, 1 x 70, 67 x 1, and 255 / 256 / 257 / 513 cells: the remainders of a workgroup of 256 lanes
  layers        1, 2, 3, 4, 5, 63, 64; the number valid varies from cell to cell, down to cells no layer covers
  placing       negative offsets, overhangs on every side, a layer larger than the destination, a layer that misses it
  values        voids as NaN, +-Inf and nodata; heights on a coarse lattice, so layers agree exactly; both zeros; +-3e38, whose
                deviations round to +Inf
  levels        0, 1, 1/2, 1/3, 65535/65536 and three more, 1 .. 8 of them a call"""
import numpy as np

ND = np.float32(-999.0)
BIG = np.float32(3e38)

# (name, gh, gw, n_layers)
SHAPES = [("1x1 K1", 1, 1, 1), ("1x1 K64", 1, 1, 64), ("1x70 K2", 1, 70, 2), ("67x1 K3", 67, 1, 3), ("255 K4", 15, 17, 4),
          ("256 K5", 16, 16, 5), ("257 K63", 1, 257, 63), ("513 K64", 27, 19, 64), ("513 K7", 19, 27, 7)]
LEVELS = [(0, 1), (1, 1), (1, 2), (1, 3), (65535, 65536), (1, 4), (3, 4), (2, 3)]
# (k nmad-factor product, floor, min_count) of smvs_dsm_stack_fuse
FUSE_PARAMS = [(3.0 * 1.4826, 0.5, 1), (0.0, 0.0, 0), (1.0, 0.0, 3), (0.0, 1e30, 64), (2.0, 0.25, 2)]


def heights(shape, seed, voids=0.16):
    """Heights with every kind of void, both zeros, exact agreement between layers and the two huge values."""
    rng = np.random.default_rng(seed)
    z = (np.round(rng.normal(100.0, 3.0, shape) * 2.0) / 2.0).astype(np.float32)        # a lattice of 0.5 m: ties across layers
    fine = rng.random(shape) < 0.4
    z[fine] = rng.normal(100.0, 30.0, shape).astype(np.float32)[fine]
    for share, v in ((voids * 0.4, np.nan), (voids * 0.4, ND), (voids * 0.1, np.inf), (voids * 0.1, -np.inf),
                     (0.06, -0.0), (0.06, 0.0), (0.03, BIG), (0.03, -BIG)):
        z[rng.random(shape) < share] = v
    return z


def layers_of(gh, gw, K, seed):
    """K layers (z, ox, oy) about a (gh, gw) destination."""
    rng = np.random.default_rng(seed)
    layers = [(heights((gh + 7, gw + 9), seed * 100), -4, -3)]                          # larger than the destination
    while len(layers) < K:
        k = len(layers)
        kind = k % 4 if K <= 8 else (k % 16 if k % 16 < 4 else 4)
        if kind == 1:                                                                     # overhangs the lower right
            h, w, ox, oy = max(gh // 2, 1) + 3, max(gw // 2, 1) + 3, gw - max(gw // 2, 1), gh - max(gh // 2, 1)
        elif kind == 2:                                                                   # overhangs the upper left
            h, w, ox, oy = max(gh // 2, 1) + 2, max(gw // 2, 1) + 2, -2, -2
        elif kind == 3:                                                                   # misses the destination
            h, w, ox, oy = 3, 4, gw, -1
        elif kind == 0:                                                                   # somewhere inside
            h, w = int(rng.integers(1, gh + 1)), int(rng.integers(1, gw + 1))
            ox, oy = int(rng.integers(0, gw - w + 1)), int(rng.integers(0, gh - h + 1))
        else:                                                                             # covers it: the deep cells of 63 and 64
            h, w, ox, oy = gh + 2, gw + 1, -1, -2
        layers.append((heights((h, w), seed * 100 + k, voids=0.08 if kind == 4 else 0.16), ox, oy))
    layers = layers[:K]
    if gw * gh > 200:                                                                     # three cells no layer covers, one the last
        for n, (r, c) in enumerate(((0, 0), (gh // 2, gw // 2), (gh - 1, gw - 1))):
            for k, (z, ox, oy) in enumerate(layers):
                if 0 <= r - oy < z.shape[0] and 0 <= c - ox < z.shape[1]:
                    z[r - oy, c - ox] = (np.nan, ND, np.inf)[(n + k) % 3]
    return layers


def centre_of(gh, gw, seed):
    """A centre grid for the deviation mode: near the heights, with cells that are not finite and the huge values."""
    rng = np.random.default_rng(seed)
    c = rng.normal(100.0, 5.0, (gh, gw)).astype(np.float32)
    for share, v in ((0.05, np.nan), (0.03, np.inf), (0.03, -np.inf), (0.08, -BIG), (0.05, BIG), (0.05, 0.0), (0.03, ND)):
        c[rng.random((gh, gw)) < share] = v
    return c


def full_layers(gh, gw, K, seed):
    """K layers that all cover the destination, few voids: columns of all K keys, layer k lower than layer k - 1 in the left half
    (every insertion travels the whole column), higher in the right half, level (all equal) in the last column."""
    rng = np.random.default_rng(seed)
    layers = []
    for k in range(K):
        step = np.where(np.arange(gw) < gw // 2, -0.25 * k, 0.25 * k).astype(np.float32)
        z = np.float32(100.0) + step[None] + (np.round(rng.normal(0.0, 0.2, (gh, gw)) * 8.0) / 8.0).astype(np.float32)
        z[rng.random(z.shape) < 0.01] = ND
        z[:, gw // 2 - 1], z[:, gw // 2], z[:, gw - 1] = 100.0 - 0.25 * k, 100.0 + 0.25 * k, 77.0       # three columns without a void
        z = np.pad(z.astype(np.float32), ((k % 3, 1), (2, k % 2)), constant_values=np.nan)
        layers.append((z, -2, -(k % 3)))
    return layers


def cases():
    """[(name, layers, gw, gh, centre)] over SHAPES, and one stack of 64 layers that all cover the destination."""
    out = [(name, layers_of(gh, gw, K, 11 + i), gw, gh, centre_of(gh, gw, 500 + i)) for i, (name, gh, gw, K) in enumerate(SHAPES)]
    return out + [("260 K64 full", full_layers(2, 130, 64, 40), 130, 2, centre_of(2, 130, 540))]


TOWN = dict(gh=96, gw=120, res=5.0, e0=500000.0, n0=4000000.0, layers=7, raised=3, lift=40.0, block=(8, 30, 10, 50), noise=0.5, k=3.0, floor=1.0)


def town():
    """The synthetic town of the other DSM tests (dsm_testkit.scene) seen seven times: every layer is the truth plus uniform noise
    held within +-0.5 m exactly (clipped in float32: truth +- 0.5 is exact at these heights), the truth's own voids in every layer,
    and layer 3 raised by 40 m over a block of valid cells -- a cloud, a crane, a mismatch.  The fusion's floor is 1 m, twice the
    noise bound: two layers within 0.5 m of the truth lie within 1 m of each other, so of the median, and with floor = 1 none of
    them can be an outlier however small the MAD of a cell turns out (with the default 0.5 m some are).
    -> (truth, [layer], block slices)."""
    from dsm_testkit import scene
    t = TOWN
    c, r = np.meshgrid(np.arange(t["gw"]), np.arange(t["gh"]))
    truth = scene(t["e0"] + c * t["res"], t["n0"] - r * t["res"])
    rng = np.random.default_rng(77)
    half = np.float32(t["noise"])
    layers = []
    for k in range(t["layers"]):
        z = (truth + rng.uniform(-t["noise"], t["noise"], truth.shape).astype(np.float32)).astype(np.float32)
        z = np.clip(z, truth - half, truth + half)
        layers.append(np.where(np.isfinite(truth) & (truth != ND), z, truth).astype(np.float32))
    r0, r1, c0, c1 = t["block"]
    block = (slice(r0, r1), slice(c0, c1))
    layers[t["raised"]][block] += np.float32(t["lift"])
    return truth, layers, block


def zeros_case():
    """Both zeros against each other and alone: where a sort by value, a sum from 0.0 or a midpoint shows.  1 x 8, 3 layers:
    cell 0: -0 alone; 1: +0 before -0; 2: -0, -0, -0; 3: +0, -0, +0; 4: -0 and +0 (even m); 5: none; 6: 1, -0, -1; 7: -0, -0."""
    n, p, v = np.float32(-0.0), np.float32(0.0), np.float32(np.nan)
    rows = [[n, p, n, p, n, v, 1.0, n],
            [v, n, n, n, p, v, n, n],
            [v, v, n, p, v, ND, -1.0, v]]
    return [(np.array([row], np.float32), 0, 0) for row in rows], 8, 1


def edge_case():
    """The threshold's edges, 1 x 6, 4 layers; with floor = 2 and kmad = 0:
    cell 0: 10, 12, 14: d = 2, 0, 2, two layers exactly at thr; cell 1: 10, 12, 14 + 2^-19 (one float32 ulp): d of the last is above
    thr; cell 2: m = 2, 10 and 20: median 15, both d = 5 > 2: n_in = 0 and out = the median; cell 3: m = 1; cell 4: m = 4, two pairs;
    cell 5: -3e38, 3e38, 3e38: the first layer's deviation rounds to +Inf."""
    v = np.float32(np.nan)
    up = np.nextafter(np.float32(14.0), np.float32(np.inf))
    rows = [[10.0, 10.0, 10.0, 7.5, 1.0, -BIG],
            [12.0, 12.0, 20.0, v, 1.0, BIG],
            [14.0, up, v, v, 4.0, BIG],
            [v, v, v, v, 4.0, v]]
    return [(np.array([row], np.float32), 0, 0) for row in rows], 6, 1
