"""Cases of the DSM production tests (tests/test_dsm_cpu.py, tests/test_dsm_gpu.py): the matrix of reduce cases, the masks of the
bin pass and the grids that put a pixel on a cell edge.  Numpy only: nothing here imports torch or the kernels.

The reduce (csrc/dsm.hip) scans the counts in tiles of SCAN_TILE = 4096 cells whose sums one block scans in chunks of
SCAN_CHUNK = 256 tiles, scatters the heights into per-cell buckets and sorts every bucket: up to TIER0_MAX = 32 keys by one
lane in registers, up to TIER1_MAX = 4096 by one of TIER1_BLOCKS = 2048 workgroups in LDS, more by one of TIER2_BLOCKS = 256
workgroups with a 4-pass radix sort over tiles of 1024 keys.  A case is (name, gh, gw, cell int32[n], height float32[n]);
case(name) builds it from a fixed seed, once, read-only."""
import functools
from collections import namedtuple

import numpy as np

import dsm_testkit as tk

SCAN_TILE, SCAN_CHUNK = 4096, 256
TIER0_MAX, TIER1_MAX = 32, 4096
TIER1_BLOCKS, TIER2_BLOCKS = 2048, 256
CHUNK_CELLS = SCAN_CHUNK * SCAN_TILE                         # 2^20: the first cell whose offset needs the carry
INT32_MAX = 2 ** 31 - 1
FLT_MAX = np.float32(3.4028234663852886e38)

Case = namedtuple("Case", "name gh gw cell height")

# ---- scan: ncells -> (gh, gw) ----------------------------------------------------------------------------------------------------
SCAN_SHAPES = {
    1: (1, 1), 2: (2, 1), 255: (1, 255), 256: (16, 16), 257: (257, 1), 4095: (63, 65), 4096: (64, 64), 4097: (17, 241),
    8191: (1, 8191), 8193: (3, 2731), CHUNK_CELLS - 1: (1023, 1025), CHUNK_CELLS: (1024, 1024), CHUNK_CELLS + 1: (61681, 17),
    257 * SCAN_TILE + 1: (3, 350891), 513 * SCAN_TILE + 5: (2101253, 1),
}
# cells whose buckets hold values that occur nowhere else (where they exist): the ends of the grid, of a tile and of a chunk
SENTINELS = (0, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, CHUNK_CELLS - 1, CHUNK_CELLS, CHUNK_CELLS + 1)
SCAN_FILLED = 6000                                            # cells with points per scan case, 0 .. 40 points each


def sentinel_cells(ncells):
    return sorted(set(c for c in SENTINELS + (ncells - 1,) if 0 <= c < ncells))


def sentinel_values(k, m):
    """The bucket of the k-th sentinel: m values around 1e6 + 1000 k, exact in float32 and far from every other bucket."""
    return (1.0e6 + 1000.0 * k + np.arange(m)).astype(np.float32)


def _scan_buckets(ncells, rng):
    cells = rng.choice(ncells, size=min(ncells, SCAN_FILLED), replace=False)
    buckets = {int(c): _finite(int(m), rng) for c, m in zip(cells, rng.integers(0, 41, cells.size))}
    for k, c in enumerate(sentinel_cells(ncells)):
        buckets[c] = sentinel_values(k, 3 + k)
    return buckets


# ---- bucket sizes ----------------------------------------------------------------------------------------------------------------
POWER_SIZES = [p + d for p in (64, 128, 256, 512, 1024, 2048, 4096) for d in (-1, 0, 1)]
RADIX_SIZES = [5119, 5120, 5121, 65535, 65536, 65537]
BIG_BUCKET = 1 << 20
# the sizes at which every kind of key value runs: an even and an odd one per tier
VALUE_SIZES = (24, 31, 1000, 777, 5000, 4999)


def _finite(m, rng):
    """Heights as a DSM has them, with ties and both zeros."""
    h = rng.normal(0.0, 100.0, m).astype(np.float32)
    h[::7] = np.round(h[::7])
    h[3::11] = 0.0
    h[5::13] = -0.0
    return h


def _from_bits(u):
    return np.ascontiguousarray(u, np.uint32).view(np.float32)


def _mixed(m, rng, shares):
    """m values drawn from (share, generator) pairs; the rest finite."""
    out = _finite(m, rng)
    kind = rng.random(m)
    lo = 0.0
    for share, gen in shares:
        sel = (kind >= lo) & (kind < lo + share)
        out[sel] = gen(int(sel.sum()))
        lo += share
    return out


def _nan(rng, sign, k):
    """k NaNs of one sign with random payloads, quiet and signalling."""
    return _from_bits(np.uint32(0x7f800000 | (sign << 31)) | rng.integers(1, 1 << 23, k, dtype=np.uint32))


QUIET_NAN = 0x7fc01234


def _byte_only(byte):
    """Keys that differ in one byte only (the other three from 0xc2a55a3c, heights near 83 m); byte 3 stays off 0x00 and 0xff,
    whose heights would be NaN."""
    def gen(m, rng):
        lo, hi = (1, 255) if byte == 3 else (0, 256)
        keys = (np.uint32(0xc2a55a3c) & ~np.uint32(0xff << (8 * byte))) | (rng.integers(lo, hi, m, dtype=np.uint32) << np.uint32(8 * byte))
        return tk.key2f(keys)
    return gen


VALUE_KINDS = {
    "all equal": lambda m, rng: np.full(m, 3.25, np.float32),
    "ascending": lambda m, rng: (np.arange(m) * 0.5 - 100.0).astype(np.float32),
    "descending": lambda m, rng: (np.arange(m)[::-1] * 0.5 - 100.0).astype(np.float32),
    "two values": lambda m, rng: rng.choice(np.array([1.5, -2.25], np.float32), m),
    "both zeros": lambda m, rng: rng.choice(np.array([0.0, -0.0], np.float32), m),
    "denormals": lambda m, rng: _from_bits(rng.integers(1, 1 << 23, m, dtype=np.uint32) | (rng.integers(0, 2, m, dtype=np.uint32) << np.uint32(31))),
    "flt_max": lambda m, rng: _mixed(m, rng, [(0.2, lambda k: np.full(k, FLT_MAX)), (0.2, lambda k: np.full(k, -FLT_MAX))]),
    "both infinities": lambda m, rng: _mixed(m, rng, [(0.1, lambda k: np.full(k, np.inf, np.float32)), (0.1, lambda k: np.full(k, -np.inf, np.float32)),
                                                      (0.1, lambda k: np.full(k, FLT_MAX)), (0.1, lambda k: np.full(k, -FLT_MAX))]),
    "mostly +inf": lambda m, rng: _mixed(m, rng, [(0.7, lambda k: np.full(k, np.inf, np.float32))]),
    "mostly -inf": lambda m, rng: _mixed(m, rng, [(0.7, lambda k: np.full(k, -np.inf, np.float32))]),
    "nan at both ends": lambda m, rng: _mixed(m, rng, [(0.15, lambda k: _nan(rng, 1, k)), (0.15, lambda k: _nan(rng, 0, k))]),
    "mostly one nan": lambda m, rng: _mixed(m, rng, [(0.7, lambda k: _from_bits(np.full(k, QUIET_NAN, np.uint32))), (0.1, lambda k: _nan(rng, 1, k))]),
    "byte 0 only": _byte_only(0), "byte 1 only": _byte_only(1), "byte 2 only": _byte_only(2), "byte 3 only": _byte_only(3),
}
ORDERED = ("ascending", "descending")                         # cases whose points stay in the order they were made in


def _cancel_large(m, rng):
    """+-1e6-scale pairs, each value + 1: the exact mean is 1."""
    x = (rng.integers(1 << 23, 1 << 25, m // 2) / 16.0).astype(np.float32)       # multiples of 2^-4 in 5e5 .. 2e6: x + 1 is exact
    v = np.concatenate([x + np.float32(1.0), np.float32(1.0) - x, np.ones(m % 2, np.float32)])
    return v.astype(np.float32)


CANCEL_KINDS = {
    "cancel 1e6": _cancel_large,
    "near 1e4": lambda m, rng: (1.0e4 + rng.uniform(-1.0e-2, 1.0e-2, m)).astype(np.float32),
}


# ---- the matrix ------------------------------------------------------------------------------------------------------------------
def _assemble(name, gh, gw, buckets, rng, shuffle=True, extra=None):
    cells = sorted(buckets)
    cell = np.concatenate([np.full(len(buckets[c]), c, np.int32) for c in cells] + [np.zeros(0, np.int32)])
    height = np.concatenate([np.asarray(buckets[c], np.float32) for c in cells] + [np.zeros(0, np.float32)])
    if extra is not None:
        cell, height = np.concatenate([cell, extra[0]]), np.concatenate([height, extra[1]])
    if shuffle:
        perm = rng.permutation(cell.size)
        cell, height = cell[perm], height[perm]
    cell, height = np.ascontiguousarray(cell, np.int32), np.ascontiguousarray(height, np.float32)
    cell.setflags(write=False)
    height.setflags(write=False)
    return Case(name, gh, gw, cell, height)


def _sized(name, gh, gw, sizes, rng):
    return _assemble(name, gh, gw, {c: _finite(m, rng) for c, m in enumerate(sizes)}, rng)


def _build(name):
    rng = np.random.default_rng([len(name)] + [ord(ch) for ch in name])
    if name.startswith("scan "):
        ncells = int(name[5:])
        gh, gw = SCAN_SHAPES[ncells]
        return _assemble(name, gh, gw, _scan_buckets(ncells, rng), rng)
    if name == "sizes 0 to 70":
        return _sized(name, 1, 71, range(71), rng)
    if name == "sizes 2^k":
        return _sized(name, 3, 7, POWER_SIZES, rng)
    if name == "sizes radix":
        return _sized(name, 2, 3, RADIX_SIZES, rng)
    if name == "size 2^20":
        return _sized(name, 1, 3, [BIG_BUCKET, 0, 5], rng)
    if name == "tier 1 twice":                              # 4097 listed cells on 2048 workgroups: two or three cells each
        return _sized(name, 17, 241, rng.integers(33, 65, 4097), rng)
    if name == "tier 2 twice":                              # 257 listed cells on 256 workgroups: one takes two
        return _sized(name, 257, 1, rng.integers(4097, 4201, 257), rng)
    if name == "tiers mixed":
        sizes = [0 if c % 4 == 0 else int(rng.integers(1, 33)) if c % 4 == 1 else int(rng.integers(33, 601)) if c % 4 == 2 else
                 int(rng.integers(4097, 5001)) if c % 40 == 3 else int(rng.integers(1, 33)) for c in range(600)]
        return _sized(name, 20, 30, sizes, rng)
    if name in VALUE_KINDS or name in CANCEL_KINDS:
        gen = VALUE_KINDS.get(name) or CANCEL_KINDS[name]
        buckets = {c: gen(m, rng) for c, m in enumerate(VALUE_SIZES)}          # cells 6 and 7 stay empty
        return _assemble(name, 2, 4, buckets, rng, shuffle=name not in ORDERED)
    if name == "ignored entries":
        gh, gw = 5, 7
        buckets = {c: _finite(int(m), rng) for c, m in enumerate(rng.integers(0, 200, gh * gw))}
        bad = np.repeat(np.array([-1, -5, gh * gw, INT32_MAX], np.int32), 200)
        return _assemble(name, gh, gw, buckets, rng, extra=(bad, rng.normal(0.0, 100.0, bad.size).astype(np.float32)))
    raise KeyError(name)


SCAN_CASES = ["scan %d" % n for n in SCAN_SHAPES]
SIZE_CASES = ["sizes 0 to 70", "sizes 2^k", "sizes radix", "size 2^20"]
LIST_CASES = ["tier 1 twice", "tier 2 twice", "tiers mixed"]
VALUE_CASES = list(VALUE_KINDS)
CANCEL_CASES = list(CANCEL_KINDS)
CASES = SCAN_CASES + SIZE_CASES + LIST_CASES + VALUE_CASES + CANCEL_CASES + ["ignored entries"]
PERMUTED_CASES = ["sizes 0 to 70", "tier 1 twice", "tier 2 twice", "tiers mixed"]      # one per tier, and all three together


@functools.lru_cache(maxsize=None)
def case(name):
    return _build(name)


# ---- the seeded random run -------------------------------------------------------------------------------------------------------
RANDOM_SEEDS = range(4)
RANDOM_PER_SEED = 50


def random_cases(seed):
    """RANDOM_PER_SEED small cases: gh, gw from 1 to 70, n from 1 to 20 000, the cells' popularity skewed by a random power so
    that all tiers occur; finite heights with ties, both zeros and denormals, and in a fifth of the cases +Inf and one NaN."""
    rng = np.random.default_rng(1000 + seed)
    for k in range(RANDOM_PER_SEED):
        hi = 9 if k % 4 == 3 else 71                          # every fourth grid has few cells, so that radix buckets occur
        gh, gw = int(rng.integers(1, hi)), int(rng.integers(1, hi))
        n = int(np.exp(rng.uniform(0.0, np.log(20000.0)))) if k % 2 else int(rng.integers(1, 20001))
        cell = np.minimum((gh * gw * rng.random(n) ** rng.integers(1, 9)).astype(np.int64), gh * gw - 1).astype(np.int32)
        h = _finite(n, rng)
        h[rng.random(n) < 0.01] = _from_bits(np.uint32(rng.integers(1, 1 << 23)))
        if k % 5 == 0:
            h[rng.random(n) < 0.05] = np.inf
            h[rng.random(n) < 0.05] = _from_bits(np.uint32(QUIET_NAN))
        if k % 7 == 0:
            cell[rng.random(n) < 0.1] = rng.choice(np.array([-1, -5, gh * gw, INT32_MAX], np.int32))
        yield Case("random %d.%d" % (seed, k), gh, gw, cell, h)


# ---- the bin pass ----------------------------------------------------------------------------------------------------------------
BIN_SIZES = [(1, 1), (1, 63), (1, 64), (1, 65), (1, 255), (1, 257), (300, 1), (1, 300), (37, 41)]
RUN_MASKS = ("runs of 64", "runs of 1", "runs of 1 to 64")


def run_mask(kind, H, W):
    """A mask over H x W pixels in raster order (the order of the lanes): everything, a checkerboard of single pixels, or valid
    stretches of every length from 1 to 64, each followed by one invalid pixel."""
    n = H * W
    if kind == "runs of 64":
        m = np.ones(n, bool)
    elif kind == "runs of 1":
        m = np.arange(n) % 2 == 0
    else:
        m = np.ones(n, bool)
        at = 0
        while at < n:
            for length in range(1, 65):
                at += length
                if at < n:
                    m[at] = False
                at += 1
    return m.reshape(H, W)


EdgeGrid = namedtuple("EdgeGrid", "name grid4 pixel on")     # `pixel` ("p" or "q") must land on the grid iff `on`
EDGE_RES, EDGE_GW, EDGE_GH = 4.0, 7, 5                        # odd sizes: np.rint and floor(x + 0.5) differ at gw - 1/2


def edge_grids(Ep, Np, Eq, Nq, gw=EDGE_GW, gh=EDGE_GH, res=EDGE_RES):
    """Grids of resolution `res` that put pixel p (map coordinates Ep, Np) on the lower edge of column 0 and of row 0, and
    pixel q on the upper edge of column gw - 1 or of row gh - 1 (the other coordinate of q mid-grid), and the same grids with the
    origin one float64 ulp to either side.  The rule's argument is exactly 0.0 on a lower edge (on the grid) and exactly gw or
    gh on an upper edge (off it)."""
    half = res / 2.0
    e0p, n0p = Ep + half, Np - half
    e0q, n0q = Eq - (res * gw - half), Nq + (res * gh - half)
    e0m, n0m = Eq - res * (gw // 2), Nq + res * (gh // 2)
    up, down = (lambda v: float(np.nextafter(v, np.inf))), (lambda v: float(np.nextafter(v, -np.inf)))
    g = lambda e0, n0: np.array([e0, n0, res, res], np.float64)          # noqa: E731
    return [
        EdgeGrid("p on both lower edges", g(e0p, n0p), "p", True),
        EdgeGrid("p, e0 one ulp up", g(up(e0p), n0p), "p", False),
        EdgeGrid("p, e0 one ulp down", g(down(e0p), n0p), "p", True),
        EdgeGrid("p, n0 one ulp down", g(e0p, down(n0p)), "p", False),
        EdgeGrid("p, n0 one ulp up", g(e0p, up(n0p)), "p", True),
        EdgeGrid("q on the upper column edge", g(e0q, n0m), "q", False),
        EdgeGrid("q, e0 one ulp up", g(up(e0q), n0m), "q", True),
        EdgeGrid("q, e0 one ulp down", g(down(e0q), n0m), "q", False),
        EdgeGrid("q on the upper row edge", g(e0m, n0q), "q", False),
        EdgeGrid("q, n0 one ulp down", g(e0m, down(n0q)), "q", True),
        EdgeGrid("q, n0 one ulp up", g(e0m, up(n0q)), "q", False),
    ]


def rule_arguments(E, N, grid4):
    """The arguments of the floor in the kernel's rule, float64."""
    e0, n0, xr, yr = [float(v) for v in grid4]
    return (np.float64(E) - e0) / xr + 0.5, (n0 - np.float64(N)) / yr + 0.5
