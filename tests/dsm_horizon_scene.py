"""The case matrix of the horizon tests (tests/test_dsm_horizon_gpu.py runs it on the device, tests/test_dsm_horizon_cpu.py
checks what it assumes), the constants of csrc/dsm_horizon.hip the sizes straddle, and the comparison both files use.
numpy only."""
import math
from collections import namedtuple

import numpy as np

from dsm_testkit import same

ND = np.float32(-999.0)
TILE = 64               # HZ_TILE: the transposes of the column-major directions
LANES = 64              # HZ_LANES: lines of one workgroup of the walk
PF = 4                  # HZ_PF: rows of q a lane loads ahead
MAX_DIRS = 64           # HZ_MAX_DIRS: directions of one call, which walk side by side in one launch
MAX_Z = np.float32(32768.0)

Grid = namedtuple("Grid", "xres yres width height")     # what terms() needs of a dsm.DSMGrid

AZIMUTHS = [0.0, 33.0, 45.0, 90.0, 123.0, 135.0, 180.0, 213.0, 270.0, 303.0, 315.0, 359.5]
RESOLUTIONS = [(5.0, 5.0), (0.3, 0.5)]

# ---- sizes (gh, gw) --------------------------------------------------------------------------------------------------------------
SMALL = [(1, 1), (1, 65), (65, 1), (2, 2)]
LINES = [(32, 32), (32, 33), (33, 33), (60, 68), (64, 65), (65, 65)]       # gw + gh - 1 = 63, 64, 65, 127, 128, 129 on a diagonal
TILES = [(TILE - 1, TILE + 1), (TILE, TILE), (TILE + 1, TILE - 1)]
AHEAD = [(PF - 1, PF + 1), (PF, PF), (PF + 1, PF - 1), (2 * PF, 2 * PF + 1), (2 * PF + 1, 2 * PF - 1)]
LARGE = [(257, 255), (300, 2300), (1100, 40)]
SIZES = SMALL + LINES + TILES + AHEAD


def terms(grid, azimuth):
    """dsm.horizon_terms with the same operations: (ucol, urow, a, b)."""
    sA, cA = math.sin(math.radians(azimuth)), math.cos(math.radians(azimuth))
    return sA / grid.xres, -cA / grid.yres, 256.0 * grid.xres * sA, -256.0 * grid.yres * cA


def directions(shape, azimuths=AZIMUTHS, res=(5.0, 5.0)):
    g = Grid(res[0], res[1], shape[1], shape[0])
    return [terms(g, az) for az in azimuths]


def towards(ucol, urow, cell=5.0):
    """(ucol, urow, a, b) of a direction given in cells over square cells: for shears the azimuths do not hit exactly."""
    n = math.hypot(ucol, urow)
    return ucol, urow, 256.0 * cell * ucol / n, 256.0 * cell * urow / n


# ---- cell values -----------------------------------------------------------------------------------------------------------------
def special(shape, seed, voids=0.15):
    """Heights on the 2^-8 m lattice and off it, with every kind of void (a share `voids` in all), both zeros, heights on
    quantisation halves, and |z| = 32768 next to one float32 ulp above it (invalid)."""
    rng = np.random.default_rng(seed)
    z = rng.normal(100.0, 30.0, shape).astype(np.float32)
    half = rng.random(shape) < 0.2
    z[half] = (np.rint(z[half] * 256.0) + 0.5).astype(np.float32) / np.float32(256.0)      # k + 1/2 units: ties to even
    kinds = [(voids * 0.4, np.nan), (voids * 0.4, ND), (voids * 0.05, np.inf), (voids * 0.05, -np.inf),
             (voids * 0.05, np.nextafter(MAX_Z, np.float32(np.inf))), (voids * 0.05, -np.nextafter(MAX_Z, np.float32(np.inf))),
             (0.03, -0.0), (0.03, 0.0), (0.005, MAX_Z), (0.005, -MAX_Z)]
    for share, v in kinds:
        z[rng.random(shape) < share] = v
    return z


def bowl(shape):
    """z grows with the squared distance from the centre: along a straight line the upper hull of the cells walked so far
    is its two ends, so every new cell pops the one before it and the stack stays at two elements or fewer."""
    r, c = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    return (0.05 * ((r - shape[0] / 2.0) ** 2 + (c - shape[1] / 2.0) ** 2)).astype(np.float32)


def dome(shape):
    """The bowl upside down: along a straight line every cell stays on the upper hull, so the stack grows to the line's
    length."""
    return (np.float32(2000.0) - bowl(shape)).astype(np.float32)


def sawtooth(shape, period=7):
    r, c = np.mgrid[0:shape[0], 0:shape[1]]
    return (100.0 + 3.0 * ((r + 2 * c) % period) + 0.01 * r).astype(np.float32)


def plane(shape, per_col=0.5):
    """z = per_col * c: along azimuth 90 or 270 every point of a line is collinear."""
    return (per_col * np.arange(shape[1], dtype=np.float64)[None, :] + np.zeros((shape[0], 1))).astype(np.float32)


def wall(shape, col, height):
    z = np.zeros(shape, np.float32)
    z[:, col] = height
    return z


def float_pop_trap():
    """Three valid cells on one row of 5 m cells, seen towards the east (azimuth 90; P = 1280 c), everything else nodata, q in
    units of 2^-8 m: i at column 1 (q = 0), t 28 cells east of it (q = 1399521), u 47 cells east of it (q = 2349196).  The
    slope from i to u is the greater by 6 parts in 10^8, so t is popped and T(i) is the slope to u; float32 quotients taken
    as a product with the reciprocal order the two the other way round, keep t, and read the slope to t, whose float32
    differs.  -> (z (1, 50), the direction)."""
    z = np.full((1, 50), ND, np.float32)
    for col, q in ((1, 0), (29, 1399521), (48, 2349196)):
        z[0, col] = np.float32(q) / np.float32(256.0)
    return z, terms(Grid(5.0, 5.0, z.shape[1], 1), 90.0)


GROUPS = ("sizes", "large", "stacks", "values")


def matrix(group):
    """[(name, z, nodata, [direction, ...])] of one group; every case is one call of the entry."""
    cases = []
    if group == "sizes":
        for i, shape in enumerate(SIZES):
            res = RESOLUTIONS[i % 2]
            cases.append(("size %r, 12 azimuths at %r" % (shape, res), special(shape, 100 + i), ND, directions(shape, res=res)))
        cases.append(("size (33, 47), shears of 1/2 and 1/3", special((33, 47), 150), ND,
                      [towards(0.5, -1.0), towards(-0.5, 1.0), towards(1.0, 0.5), towards(-1.0, -0.5), towards(1.0, -3.0), towards(-3.0, 1.0)]))
    elif group == "large":
        cases.append(("size (257, 255), 12 azimuths at 5 m", special((257, 255), 200), ND, directions((257, 255))))
        cases.append(("size (257, 255), 12 azimuths at 0.3 x 0.5 m", special((257, 255), 201, voids=0.5), ND, directions((257, 255), res=RESOLUTIONS[1])))
        cases.append(("size (300, 2300)", special((300, 2300), 202, voids=0.02), ND, directions((300, 2300), [0.0, 123.0, 315.0])))
        cases.append(("size (1100, 40)", special((1100, 40), 203, voids=0.02), ND, directions((1100, 40), [33.0, 90.0, 213.0])))
    elif group == "stacks":
        four = [0.0, 123.0, 225.0, 270.0]
        for name, fn in (("bowl", bowl), ("dome", dome), ("sawtooth", sawtooth)):
            cases.append(("%s (70, 90)" % name, fn((70, 90)), ND, directions((70, 90), four)))
            cases.append(("%s (1, 300)" % name, fn((1, 300)), ND, directions((1, 300), [90.0, 270.0])))
            cases.append(("%s (300, 1)" % name, fn((300, 1)), ND, directions((300, 1), [0.0, 180.0], RESOLUTIONS[1])))
        for share in (0.0, 0.15, 0.5):
            cases.append(("random heights, voids %g" % share, special((70, 90), 300, voids=share), ND, directions((70, 90), four)))
        cases.append(("all invalid", np.full((40, 50), np.nan, np.float32), ND, directions((40, 50), four)))
        one = np.full((40, 50), ND, np.float32)
        one[17, 23] = 5.0
        cases.append(("one valid cell", one, ND, directions((40, 50), four)))
    elif group == "values":
        z = special((40, 50), 400)
        cases.append(("NaN nodata", np.where(np.isnan(z), np.float32(7.0), z), np.float32(np.nan), directions((40, 50))))
        edge = np.zeros((6, 8), np.float32)
        edge[0] = [MAX_Z, -MAX_Z, np.nextafter(MAX_Z, np.float32(np.inf)), -np.nextafter(MAX_Z, np.float32(np.inf)), 0.0, -0.0, np.inf, -np.inf]
        edge[1] = [(k + 0.5) / 256.0 for k in range(-4, 4)]                                     # halves: -3.5 .. 3.5 units
        edge[2] = [np.nan, ND, 1.0, -1.0, 0.001953125, -0.001953125, 100.0, -100.0]
        edge[3:] = np.float32(0.5 / 256.0)
        cases.append(("edge values", edge, ND, directions((6, 8))))
        cases.append(("edge values, transposed", np.ascontiguousarray(edge.T), ND, directions((8, 6), res=RESOLUTIONS[1])))
        cases.append(("the float pop trap",) + (float_pop_trap()[0], ND, [float_pop_trap()[1]]))
        cases.append(("a collinear plane", plane((5, 60)), ND, directions((5, 60), [90.0, 270.0, 45.0])))
    else:
        raise ValueError(group)
    return cases


def compare(got, want, what):
    """The comparison of the GPU tests: tangents by equal bits, NaN and -inf included; no cell is excused."""
    assert got.dtype == np.float32 and got.ndim == 3, what
    same(got, want, what)
