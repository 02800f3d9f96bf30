"""Cases of the registration tests (tests/test_dsm_coreg_cpu.py, tests/test_dsm_coreg_gpu.py): the shape matrix of
smvs_dsm_shift_stats, the grids with special values, and the displaced scenes of the end-to-end tests.  Nothing here imports
the kernels.

The kernel (csrc/dsm_coreg.hip) walks tiles of T = 64 x 16 (width x height) cells of b with at most 1024 persistent
workgroups of 256 lanes (512 at radius >= 18), holds 1, 2, 3, 5, 9, 13 or 17 shifts per lane (the first that covers
(2R + 1)^2 / 256), and below 129 shifts splits the lanes into 256 / 2^k parts.  A case is
(name, b (h, w), a (h, w), (ox, oy), radius); every case runs with dz0 = DZ0 and trim = TRIM on grids from special_grid()."""
import functools
from collections import namedtuple

import numpy as np

import dsm_testkit as tk

TW, TH = 64, 16
DZ0, TRIM = 0.375, 6.0
Case = namedtuple("Case", "name b a offset radius")

SHAPE_CASES = [
    # b's width and height with remainder 0, 1 and T - 1 modulo T
    Case("tile exact", (TH, TW), (TH, TW), (0, 0), 2),
    Case("two by two tiles exact", (2 * TH, 2 * TW), (2 * TH, 2 * TW), (0, 0), 1),
    Case("remainder 1", (TH + 1, TW + 1), (TH + 1, TW + 1), (0, 0), 2),
    Case("remainder 1, two tiles", (2 * TH + 1, 2 * TW + 1), (2 * TH + 3, 2 * TW + 2), (1, 1), 3),
    Case("remainder T - 1", (TH - 1, TW - 1), (TH - 1, TW - 1), (0, 0), 2),
    Case("remainder T - 1, two tiles", (2 * TH - 1, 2 * TW - 1), (2 * TH - 1, 2 * TW - 1), (0, 0), 4),
    Case("1 x 1", (1, 1), (1, 1), (0, 0), 1),
    Case("1 x 1 in a larger a", (1, 1), (5, 7), (3, 2), 2),
    Case("1 x W", (1, 70), (1, 70), (0, 0), 3),
    Case("H x 1", (37, 1), (37, 1), (0, 0), 3),
    # fewer tiles than workgroups; every workgroup visits at least two tiles (25 x 95 = 2375 tiles > 2 x 1024)
    Case("8 x 8", (8, 8), (8, 8), (0, 0), 8),
    Case("300 x 700", (300, 700), (310, 690), (-4, 6), 8),
    Case("every workgroup twice", (1505, 1537), (1500, 1540), (2, -3), 1),
    # the radii: (2R + 1)^2 below, at and not a multiple of the block; every count of shifts per lane and of parts
    Case("radius 0", (33, 70), (33, 70), (0, 0), 0),
    Case("radius 1", (33, 70), (33, 70), (0, 0), 1),
    Case("radius 5", (33, 70), (40, 66), (-2, 3), 5),
    Case("radius 6", (20, 66), (20, 66), (0, 0), 6),
    Case("radius 7", (33, 70), (33, 70), (0, 0), 7),
    Case("radius 8", (33, 70), (30, 75), (1, -1), 8),
    Case("radius 12", (20, 66), (20, 66), (0, 0), 12),
    Case("radius 16", (20, 66), (25, 60), (2, 2), 16),
    Case("radius 20", (18, 65), (18, 65), (0, 0), 20),
    Case("radius 25", (18, 65), (18, 65), (0, 0), 25),
    Case("radius 32", (18, 65), (40, 100), (10, 5), 32),
    # a smaller than, equal to, larger than b; offsets of both signs; shifts with partial and with no overlap
    Case("a smaller", (40, 90), (12, 30), (-20, -10), 6),
    Case("a larger", (12, 30), (40, 90), (20, 10), 6),
    Case("negative offsets, partial overlap", (33, 70), (33, 70), (-65, -28), 7),
    Case("positive offsets, partial overlap", (33, 70), (33, 70), (65, 28), 7),
    Case("mixed offsets", (33, 70), (50, 50), (-10, 30), 8),
    Case("ox beyond a", (33, 70), (33, 70), (200, 0), 4),
    Case("ox beyond b on the other side", (33, 70), (20, 30), (-150, 3), 4),
    Case("oy beyond", (33, 70), (33, 70), (0, -2000), 8),
    Case("far beyond", (33, 70), (33, 70), (2 ** 30 - 1, -(2 ** 30 - 1)), 32),
]


@functools.lru_cache(maxsize=None)
def special_grid(gh, gw, seed, nodata=-999.0):
    """Heights around 100 m, on multiples of 2^-10 m mostly (so halves occur), with NaN, +-Inf, nodata, -0.0 and a few far
    values sprinkled in.  Shared among the tests: nobody writes to it."""
    rng = np.random.default_rng(seed)
    z = (np.rint(rng.normal(100.0, 2.5, (gh, gw)) * 1024.0) / 1024.0).astype(np.float32)
    kind = rng.random((gh, gw))
    for lo, v in ((0.00, np.nan), (0.02, np.inf), (0.03, -np.inf), (0.04, nodata), (0.07, -0.0), (0.08, 1.0e30), (0.085, 100.1)):
        z[(kind >= lo) & (kind < lo + 0.01)] = np.float32(v)
    z.setflags(write=False)
    return z


def case_grids(case, nodata=-999.0):
    return special_grid(*case.a, seed=11 + case.radius, nodata=nodata), special_grid(*case.b, seed=12 + case.radius, nodata=nodata)


class Grid:                                                  # what the oracle reads of a DSMGrid
    def __init__(self, gh, gw, e0=500000.0, n0=3400000.0, xres=5.0, yres=5.0):
        self.e0, self.n0, self.xres, self.yres, self.width, self.height = e0, n0, xres, yres, gw, gh


# ---- the displaced scenes of the end-to-end tests --------------------------------------------------------------------------------
# (gh, gw, seed, radius, sx, sy, dz): b = the scene, a = the same scene displaced by (sx, sy) cells, raised by dz, with noise
DISPLACED = [(64, 80, 1, 4, 3, -2, 4.25), (97, 131, 2, 8, -7, 5, -3.5), (40, 50, 3, 3, 0, 0, 0.0), (33, 65, 4, 2, 2, 2, 1.0)]
RES = 5.0


@functools.lru_cache(maxsize=None)
def textured(gh, gw, seed, res=RES, e0=1000.0, n0=5000.0):
    """dsm_testkit.scene with 5 % voids and 1 % salt over a (gh, gw) grid, plus sigma = 1.5 m texture so that the minimum of the
    spread is sharp.  -> (float32 scene, Grid)."""
    r, c = np.mgrid[0:gh, 0:gw]
    z = tk.scene(e0 + c * res, n0 - r * res, seed=seed, voids=0.05, salt=0.01)
    z = (z + np.random.default_rng(seed + 100).normal(0.0, 1.5, z.shape).astype(np.float32)).astype(np.float32)
    z.setflags(write=False)
    return z, Grid(gh, gw, e0, n0, res, res)


@functools.lru_cache(maxsize=None)
def displaced(gh, gw, seed, radius, sx, sy, dz, sigma=0.3):
    """-> (a, grid_a, b, grid_b): b a (gh, gw) window of a larger textured scene, a a window two cells larger whose cell
    (r + 1 + sy, c + 1 + sx) holds b's cell (r, c), + dz + noise, while the georeferences claim that a's cell (r + 1, c + 1)
    does: coregister must find shift_cells = (sx, sy), dz, and de = -sx res, dn = sy res."""
    pad = radius + 2
    big, gbig = textured(gh + 2 * pad, gw + 2 * pad, seed)
    b = big[pad:pad + gh, pad:pad + gw].copy()
    a = (big + np.float32(dz)).astype(np.float32)[pad - sy - 1:pad - sy + gh + 1, pad - sx - 1:pad - sx + gw + 1].copy()
    a = (a + np.random.default_rng(seed + 7).normal(0.0, sigma, a.shape).astype(np.float32)).astype(np.float32)
    grid_b = Grid(gh, gw, gbig.e0 + pad * RES, gbig.n0 - pad * RES, RES, RES)
    grid_a = Grid(gh + 2, gw + 2, grid_b.e0 - RES, grid_b.n0 + RES, RES, RES)
    for g in (a, b):
        g.setflags(write=False)
    return a, grid_a, b, grid_b
