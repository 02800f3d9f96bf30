"""The case matrix of the viewshed tests (tests/test_dsm_viewshed_gpu.py runs it on the device, tests/test_dsm_viewshed_cpu.py
holds the two statements of the rule against each other on it), the constants of csrc/dsm_viewshed.hip the sizes straddle, and
the comparison both files use.  numpy only."""
from collections import namedtuple

import numpy as np

import dsm_viewshed_oracle as vo
from dsm_horizon_scene import MAX_Z, ND, special  # noqa: F401  (the cell values of the horizon tests: halves, zeros, voids, +-32768)
from dsm_testkit import scene as terrain

TILE_H, TILE_W, WAVES = 8, 8, 4     # VS_TILE_H, VS_TILE_W, VS_WAVES: a wave is 8 x 8 targets, a workgroup 8 rows by 32 columns
MAX_OBS = 64                        # VS_MAX_OBS: observers of one call

Grid = namedtuple("Grid", "xres yres width height")     # what terms() needs of a dsm.DSMGrid

# ---- sizes (gh, gw) --------------------------------------------------------------------------------------------------------------
SMALL = [(1, 1), (1, 70), (67, 1), (2, 2), (67, 3)]
SIDES = [(7, 9), (8, 8), (9, 7), (63, 65), (64, 64), (65, 63)]          # the remainders of both lane mappings (8 x 8 and 1 x 64)
SIZES = SMALL + SIDES
RESOLUTIONS = [(5.0, 5.0), (5.0, 2.5), (30.0, 30.0)]


def terms(shape, res=(5.0, 5.0), **kw):
    return vo.terms(Grid(res[0], res[1], shape[1], shape[0]), **kw)


def observer(row, col, eye_m=1.6, mode=0, tgt_m=0.0):
    """The HOST record (col, row, eye, mode, tgt) with the heights in metres."""
    return (int(col), int(row), vo.units(eye_m), int(mode), vo.units(tgt_m))


def corners_and_centre(shape, **kw):
    gh, gw = shape
    return [observer(r, c, **kw) for r, c in ((0, 0), (0, gw - 1), (gh - 1, 0), (gh - 1, gw - 1), (gh // 2, 0), (gh // 2, gw // 2))]


def town(shape, seed, voids=0.0, res=(5.0, 5.0), salt=0.01):
    """dsm_testkit.scene over `shape`: terrain, two blocks about the centre, holes, salt noise and random voids."""
    c, r = np.meshgrid(np.arange(shape[1]), np.arange(shape[0]))
    return terrain(500000.0 + res[0] * c, 4000000.0 - res[1] * r, seed=seed, voids=voids, salt=salt)


def town_observers(shape):
    """The four corners, an edge and the centre; on the roof of the first block, and in the street between the blocks; one
    absolute eye above the NaN hole beside the first block."""
    gh, gw = shape
    r0, c0 = gh // 2 - 3, gw // 2 - 3
    return corners_and_centre(shape) + [observer(r0 + 4, c0 + 2), observer(r0 - 4, c0 + 4), observer(r0 + 1, c0 + 6, eye_m=190.0, mode=1)]


def wall(shape, col, height):
    z = np.zeros(shape, np.float32)
    z[:, col] = height
    return z


def tilted(shape, per_col=0.5):
    """z = per_col * c: seen from column 0 at eye 0 every sample of a row lies exactly on the line of sight."""
    return (per_col * np.arange(shape[1], dtype=np.float64)[None, :] + np.zeros((shape[0], 1))).astype(np.float32)


def edge_values():
    edge = np.zeros((6, 8), np.float32)
    edge[0] = [MAX_Z, -MAX_Z, np.nextafter(MAX_Z, np.float32(np.inf)), -np.nextafter(MAX_Z, np.float32(np.inf)), 0.0, -0.0, np.inf, -np.inf]
    edge[1] = [(k + 0.5) / 256.0 for k in range(-4, 4)]                                     # halves: -3.5 .. 3.5 units
    edge[2] = [np.nan, ND, 1.0, -1.0, 0.001953125, -0.001953125, 100.0, -100.0]
    edge[3:] = np.float32(0.5 / 256.0)
    return edge


def wall_closed_form(xp, ct, rt, co, ro, a, Hq, hq, tgt):
    """The similar-triangle statement for an eye hq units above cell (ro, co) of the plane q = 0, a wall of Hq < hq units in
    column a > co across all rows, and targets tgt units above the cells (rt, ct), without curvature.  A target behind the wall
    (ct > a) is hidden iff (Hq - hq) n > (tgt - hq) i, i the last step at which its line is in the wall's column: a - co for a
    line that steps along columns, and for one that steps along rows the last i with floor((2 i dx + n) / (2 n)) <= a - co,
    which is ceil(n (2 (a - co) + 1) / (2 dx)) - 1; the samples on the plane never hide anything.  xp is numpy or torch, the
    cells are int64 arrays of it -> (hidden, need in units where hidden)."""
    dx, dy, da = ct - co, rt - ro, a - co
    rows = abs(dy) >= abs(dx)
    n = xp.where(rows, abs(dy), abs(dx))
    behind = dx > da
    i = xp.where(rows, -((-(n * (2 * da + 1))) // (2 * xp.where(behind, dx, dx * 0 + 1))) - 1, dx * 0 + da)
    hidden = behind & ((Hq - hq) * n > (tgt - hq) * i)
    return hidden, -((-((Hq - hq) * n)) // xp.where(behind, i, i * 0 + 1)) + hq


GROUPS = ("sizes", "town", "large town", "values", "parameters")


def matrix(group):
    """[(name, z, nodata, terms, [observer, ...])] of one group; every case is one call of the entry."""
    cases = []
    if group == "sizes":
        for i, shape in enumerate(SIZES):
            res = RESOLUTIONS[i % 2]
            obs = corners_and_centre(shape) + [observer(shape[0] // 2, shape[1] // 2, eye_m=150.0, mode=1, tgt_m=10.0)]
            cases.append(("size %r at %r" % (shape, res), special(shape, 100 + i), ND, terms(shape, res, curvature=i % 3 != 0), obs))
    elif group in ("town", "large town"):
        for shape, seed in [((128, 160), 200)] if group == "town" else [((257, 301), 210)]:
            for k, voids in enumerate((0.0, 0.05, 0.3)):
                obs = town_observers(shape)
                obs = obs if shape[0] < 200 else [obs[0], obs[3], obs[5], obs[6], obs[7]][k:k + 3]      # the long lines cost the oracle most
                cases.append(("town %r, voids %g" % (shape, voids), town(shape, seed + k, voids), ND, terms(shape, curvature=k != 1), obs))
    elif group == "values":
        z = special((40, 50), 400)
        cases.append(("NaN nodata", np.where(np.isnan(z), np.float32(7.0), z), np.float32(np.nan), terms((40, 50)), corners_and_centre((40, 50))))
        e = edge_values()
        everywhere = [observer(r, c, eye_m=0.0) for r in range(6) for c in range(8)]
        cases.append(("edge values", e, ND, terms((6, 8), (5.0, 2.5)), everywhere + [observer(2, 0, eye_m=-32768.0, mode=1), observer(0, 2, eye_m=32768.0, mode=1)]))
        cases.append(("edge values, transposed", np.ascontiguousarray(e.T), ND, terms((8, 6), curvature=False),
                      [observer(c, r, eye_m=0.0, tgt_m=32768.0) for r in range(6) for c in range(8)]))
        cases.append(("voids 50 %", special((30, 40), 410, voids=0.75), ND, terms((30, 40), (5.0, 2.5)), corners_and_centre((30, 40), eye_m=20.0, mode=1)))
        cases.append(("all invalid", np.full((20, 30), np.nan, np.float32), ND, terms((20, 30)), [observer(3, 4, mode=1), observer(0, 0, eye_m=5.0, mode=1)]))
        one = np.full((20, 30), ND, np.float32)
        one[7, 13] = 5.0
        cases.append(("one valid cell", one, ND, terms((20, 30)), [observer(7, 13), observer(0, 0, eye_m=0.0, mode=1)]))
        cases.append(("a tilted plane: grazing everywhere", tilted((5, 60)), ND, terms((5, 60), curvature=False), [observer(r, 0, eye_m=0.0) for r in range(5)]))
        cases.append(("a level plane", np.zeros((9, 33), np.float32), ND, terms((9, 33), curvature=False), corners_and_centre((9, 33), eye_m=0.0)))
    elif group == "parameters":
        shape = (70, 90)
        z = town(shape, 300, 0.05)
        for name, t, kw in (("tgt 10 m", terms(shape), dict(tgt_m=10.0)), ("max_distance 150 m", terms(shape, max_distance=150.0), {}),
                            ("max_distance 150 m on 5 x 2.5 m cells", terms(shape, (5.0, 2.5), max_distance=150.0), dict(tgt_m=2.0)),
                            ("curvature on at 30 m cells", terms(shape, (30.0, 30.0)), {}), ("no refraction at 30 m cells", terms(shape, (30.0, 30.0), refraction=0.0), {}),
                            ("an eye below the surface", terms(shape), dict(eye_m=100.0, mode=1))):
            cases.append((name, z, ND, t, corners_and_centre(shape, **kw)))
        cases.append(("a 1 x 400 row of 30 m cells", np.zeros((1, 400), np.float32), ND, terms((1, 400), (30.0, 30.0)), [observer(0, 0), observer(0, 399), observer(0, 200)]))
    else:
        raise ValueError(group)
    return cases


def compare(got, want, what):
    """The comparison of the GPU tests: codes by value, `above` by its bits; no cell is excused, and the first differing cell
    is named."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
    if not np.array_equal(g, w):
        first = tuple(int(v) for v in np.argwhere(g != w)[0])
        raise AssertionError("%s: %d cells differ, the first at %s: got %r, want %r" % (what, int((g != w).sum()), first, got[first], want[first]))
