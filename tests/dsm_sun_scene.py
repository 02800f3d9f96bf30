"""The case matrix of the shadow tests (tests/test_dsm_sun_gpu.py runs it on the device, tests/test_dsm_sun_cpu.py checks what
it assumes), the constants of csrc/dsm_sun.hip the sizes straddle, and the comparison both files use.  numpy only."""
import math

import numpy as np

from dsm_testkit import same

ND = np.float32(-999.0)
FLT_MAX = np.finfo(np.float32).max
BAND = 32               # SUN_BAND: rows of a line that one lane scans
BLOCK = 256             # SUN_THREADS: slots of a band (W + BAND + 1 of them), and lines of the carry, per workgroup
TILE = 64               # SUN_TILE: the transposes of the column-major directions

# ---- directions (ucol, urow), towards the sun in cells ---------------------------------------------------------------------------
OCTANTS = [(0.0, -1.0), (0.0, 1.0), (1.0, 0.0), (-1.0, 0.0), (1.0, -1.0), (1.0, 1.0), (-1.0, -1.0), (-1.0, 1.0)]
HALVES = [(0.5, -1.0), (-0.5, -1.0), (0.5, 1.0), (1.0, 0.5), (-1.0, 0.5), (-1.0, -0.5)]                   # m = +-1/2: halves in s
THIRDS = [(1.0, -3.0), (-1.0, 3.0), (3.0, 1.0), (-3.0, -1.0)]
TINY = [(1e-18, -1.0), (-1e-18, 1.0), (1.0, 1e-18), (-1.0, -1e-18)]
IRRATIONAL = [(math.sqrt(2.0), -math.pi), (-math.e, math.sqrt(7.0)), (math.pi, math.sqrt(3.0)), (-math.sqrt(5.0), -math.e / 3.0)]
DIRECTIONS = OCTANTS + HALVES + THIRDS + TINY + IRRATIONAL
MAJORS = [(0.3, -1.0), (-0.7, 1.0), (1.0, 0.4), (-1.0, -0.6)]            # one per major axis and scan order

# ---- sizes (gh, gw) --------------------------------------------------------------------------------------------------------------
SMALL = [(1, 1), (1, 37), (41, 1), (2, 2)]
BANDS_ROWS = [(BAND - 1, 70), (BAND, 70), (BAND + 1, 70), (2 * BAND + 1, 70)]          # the scan axis of the row-major directions
BANDS_COLS = [(70, BAND - 1), (70, BAND), (70, BAND + 1), (70, 2 * BAND + 1)]          # ... of the column-major ones
SLOTS = [(40, BLOCK - BAND - 2), (40, BLOCK - BAND - 1), (40, BLOCK - BAND)]           # W + BAND + 1 = 255, 256, 257
LINES_FLAT = [(5, BLOCK - 1), (5, BLOCK), (5, BLOCK + 1)]                              # m = 0: gw lines
LINES_DIAG = [(40, BLOCK - 40), (40, BLOCK - 39), (40, BLOCK - 38)]                    # |m| = 1: gw + 39 lines
TILES = [(TILE - 1, TILE + 1), (TILE, TILE), (TILE + 1, TILE - 1)]
LARGE = [(300, 2300), (2300, 300)]
SIZES = SMALL + BANDS_ROWS + BANDS_COLS + SLOTS + LINES_FLAT + LINES_DIAG + TILES


def line_count(gh, gw, ucol, urow):
    """gw + the shear's span on the working grid (the transposed one for a column-major direction)."""
    rows = abs(urow) >= abs(ucol)
    H, W, m = (gh, gw, ucol / urow) if rows else (gw, gh, urow / ucol)
    return W + abs(int(math.floor(m * float(H - 1) + 0.5)))


def terms(ucol, urow, k=0.5, cell=5.0):
    """(a, b) of a sun in the direction (ucol, urow) at tan(elevation) = k over square cells."""
    n = math.hypot(ucol, urow)
    return k * cell * ucol / n, k * cell * urow / n


# ---- cell values -----------------------------------------------------------------------------------------------------------------
def special(shape, seed, extremes=True):
    """Heights with every kind of void, both zeros and, with `extremes`, +-FLT_MAX."""
    rng = np.random.default_rng(seed)
    z = rng.normal(100.0, 30.0, shape).astype(np.float32)
    kinds = [(0.06, np.nan), (0.06, ND), (0.02, np.inf), (0.02, -np.inf), (0.04, -0.0), (0.04, 0.0)]
    if extremes:
        kinds += [(0.01, FLT_MAX), (0.01, -FLT_MAX)]
    for share, v in kinds:
        z[rng.random(shape) < share] = v
    return z


def relief(shape, seed):
    """A surface whose shadows are long and many: smooth hills plus sparse towers, a few voids."""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    z = (100.0 + 15.0 * np.sin(c / 23.0) * np.cos(r / 31.0)).astype(np.float32)
    z[rng.random(shape) < 0.004] += np.float32(300.0)
    z[rng.random(shape) < 0.01] = np.nan
    z[rng.random(shape) < 0.01] = ND
    return z


GROUPS = ("directions", "sizes", "large", "values")


def matrix(group):
    """[(name, z, nodata, (ucol, urow), (a, b), tol)] of one group: every direction on two grids of special values; every
    size in the four majors, on a diagonal and along both axes; the large grids; the value cases."""
    cases = []
    if group == "directions":
        for i, u in enumerate(DIRECTIONS):
            cases.append(("direction %r on 67 x 130" % (u,), special((67, 130), 100 + i), ND, u, terms(*u), 0.1))
            cases.append(("direction %r on 131 x 66, no slope" % (u,), special((131, 66), 200 + i, extremes=False), ND, u, (0.0, 0.0), 0.0))
    elif group == "sizes":
        for i, shape in enumerate(SIZES):
            for u in MAJORS + [(1.0, -1.0), (0.0, -1.0), (-1.0, 0.0)]:
                cases.append(("size %r towards %r" % (shape, u), special(shape, 300 + i), ND, u, terms(*u), 0.1))
    elif group == "large":
        for i, shape in enumerate(LARGE):
            for u in MAJORS + [(-1.0, 1.0)]:
                cases.append(("size %r towards %r" % (shape, u), relief(shape, 400 + i), ND, u, terms(*u, k=0.3), 0.1))
    elif group == "values":
        z = special((40, 50), 500)
        for u in MAJORS:
            cases.append(("NaN nodata towards %r" % (u,), np.where(np.isnan(z), np.float32(7.0), z), np.float32(np.nan), u, terms(*u), 0.1))
            cases.append(("all invalid towards %r" % (u,), np.full((40, 50), np.nan, np.float32), ND, u, terms(*u), 0.1))
            one = np.full((40, 50), ND, np.float32)
            one[17, 23] = 5.0
            cases.append(("one valid cell towards %r" % (u,), one, ND, u, terms(*u), 0.1))
            cases.append(("xres != yres towards %r" % (u,), special((40, 50), 501), ND, (u[0] / 5.0, u[1] / 3.0),
                          (0.5 * 5.0 * u[0], 0.5 * 3.0 * u[1]), 0.1))
        cases.append(("the tol pairs",) + tol_pairs())
    else:
        raise ValueError(group)
    return cases


def tol_pairs():
    """With a = b = 0 (g = z exactly) and the sun in the north: column 0 holds a pair with G - g == tol, column 1 a pair one
    float64 ulp above it.  -> (z, nodata, direction, (a, b), tol)"""
    z = np.array([[2.0, 1.0], [1.0, -2.0 ** -52]], np.float32)
    return z, ND, (0.0, -1.0), (0.0, 0.0), 1.0


def compare(got, want, what):
    """The comparison of the GPU tests: shade by equal values, depth (if any) by equal bits; no cell is excused."""
    assert got[0].dtype == np.uint8 and np.array_equal(got[0], want[0]), (what, "shade", int((got[0] != want[0]).sum()),
                                                                        np.argwhere(got[0] != want[0])[:5].tolist())
    if got[1] is not None:
        same(got[1], want[1], (what, "depth"))
