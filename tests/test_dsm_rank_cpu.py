"""The focal order statistics without a device: the two statements of the rule (tests/dsm_rank_oracle.py) against each other,
satmvs_amd.dsm._window_runs against focal_window's membership cell by cell, the order of the runs, every Python-side rejection,
and the elevation percentile on a hand-made window."""
from fractions import Fraction

import numpy as np
import pytest

import dsm_rank_oracle as ro
from satmvs_amd import dsm
from satmvs_amd.dsm import DSMGrid, FocalWindow, _window_runs, focal_window


# ---- the two statements ----------------------------------------------------------------------------------------------------------
def test_the_two_statements_agree():
    cases = ro.matrix(large=False)
    for c in cases:
        a = ro.select_loop(c["dsm"], c["foot"], c["levels"], c["nodata"], c["centre"])
        b = ro.select_sorted(c["dsm"], c["foot"], c["levels"], c["nodata"], c["centre"])
        assert ro.differing(b, a) is None, (c["name"], ro.differing(b, a))
    names = [c["name"] for c in cases]
    for gh, gw in ro.GRIDS + ((70, 90),):
        for w in ("box 0", "box 8", "disc 8", "annulus 4..8", "one row", "one column", "lopsided"):
            assert "scene %dx%d %s" % (gh, gw, w) in names
    assert {len(c["levels"]) for c in cases} == {1, 4} and {lv for c in cases for lv in c["levels"]} == set(ro.LEVELS)


def test_the_two_counts_agree():
    for c in ro.matrix(large=False)[5::7]:
        if c["centre"] is not None:
            continue
        z = c["dsm"]
        t = z.copy()
        at = np.arange(0, t.size, 5)
        t.reshape(-1)[at] = np.array([np.nan, np.inf, -np.inf, c["nodata"], 0.0], np.float32)[np.arange(len(at)) % 5]
        for thr in (z, t):
            a, b = ro.count_loop(z, c["foot"], thr, c["nodata"]), ro.count_sorted(z, c["foot"], thr, c["nodata"])
            assert ro.differing(b, a) is None, (c["name"], ro.differing(b, a))


def test_the_matrix_holds_what_it_should():
    z = np.array([[0.0, -0.0, 0.0], [-0.0, 0.0, -0.0], [0.0, -0.0, 0.0]], np.float32)
    n, lo, hi = ro.select_loop(z, ro.footprint("box", 1), ((0, 1), (1, 1)))
    assert n[1, 1] == 9 and lo.view(np.uint32)[0, 1, 1] == 0x80000000 and lo.view(np.uint32)[1, 1, 1] == 0      # rank 0 is -0.0
    c = [c for c in ro.matrix(large=False) if c["name"].startswith("deviation that rounds to +Inf box 1")][0]
    n, lo, hi = ro.select_sorted(c["dsm"], c["foot"], ((1, 1),), c["nodata"], c["centre"])
    assert np.isposinf(lo[0, 10, 10]) and n[10, 10] > 0
    c = [c for c in ro.matrix(large=False) if c["name"].startswith("deviation from the median, scene box 1")][0]
    n = ro.select_sorted(c["dsm"], c["foot"], ((1, 2),), c["nodata"], c["centre"])[0]
    assert n[3, 4] == 0 and n[20, 30] == 0 and n.max() == 9


def test_ranks_are_quantile_ranks():
    m = np.arange(0, 200, dtype=np.int32)
    lo, hi, rem, den = dsm.quantile_ranks(m, [Fraction(*lv) for lv in ro.LEVELS])
    for j, (num, d) in enumerate(ro.LEVELS):
        for n in range(1, 200):
            assert ro.rank_pair(n, num, d) == (lo[n, j], hi[n, j], rem[n, j])


# ---- the windows -----------------------------------------------------------------------------------------------------------------
def _member(shape, dx, dy, radius, inner, xres, yres):
    if shape == "box":
        return abs(dx * xres) <= radius and abs(dy * yres) <= radius
    d2 = (dx * xres) * (dx * xres) + (dy * yres) * (dy * yres)
    return d2 <= radius * radius and (shape != "annulus" or d2 > inner * inner)


def _cells_of(runs):
    return {(int(dy), dx) for dy, dx0, dx1 in runs for dx in range(int(dx0), int(dx1) + 1)}


@pytest.mark.parametrize("shape,radius,inner", [("box", 0, None), ("box", 3, None), ("box", 32, None), ("disc", 0.5, None), ("disc", 4.5, None),
                                                ("disc", 32, None), ("annulus", 8, 4), ("annulus", 32, 31.5), ("annulus", 20.25, 0)])
def test_window_runs_hold_focal_windows_cells(shape, radius, inner):
    for grid, (xres, yres) in ((None, (1.0, 1.0)), (DSMGrid(0.0, 0.0, 2.0, 5.0, 10, 10), (2.0, 5.0))):
        scale = 1.0 if grid is None else 2.0                 # metres on the anisotropic grid: 32 cells east are 64 m
        w = focal_window(shape, radius * scale, None if inner is None else inner * scale, grid)
        runs = _window_runs(w)
        want = {(dy, dx) for dy in range(-40, 41) for dx in range(-40, 41)
                if _member(shape, dx, dy, np.float64(radius * scale), None if inner is None else np.float64(inner * scale), xres, yres)}
        assert _cells_of(runs) == want and len(want) == w.cells
        _runs_in_order(runs)


def _runs_in_order(runs):
    assert runs.dtype == np.int32 and runs.ndim == 2 and runs.shape[1] == 3 and 1 <= len(runs) <= dsm.MAX_RANK_RUNS
    assert (runs[:, 1] <= runs[:, 2]).all() and np.abs(runs).max() <= dsm.MAX_RANK_OFFSET
    for a, b in zip(runs[:-1], runs[1:]):
        assert b[0] > a[0] or (b[0] == a[0] and b[1] > a[2] + 1), (a, b)         # sorted by (dy, dx0); never touching in a row


def test_window_runs_of_footprints():
    for name, foot in ro.windows() + [("box 32", ro.footprint("box", 32))]:
        runs = _window_runs(foot)
        assert np.array_equal(runs, ro.runs_of(foot)), name
        _runs_in_order(runs)
    comb = np.zeros((5, 9), bool)
    comb[:, ::2] = True
    comb[2, 3] = True                                        # bridges two teeth: one run of three, four runs in that row
    runs = _window_runs(comb)
    assert len(runs) == 4 * 5 + 4 and np.array_equal(runs, ro.runs_of(comb))
    _runs_in_order(runs)
    import torch
    assert np.array_equal(_window_runs(torch.from_numpy(comb)), runs)


def test_window_runs_reject():
    twice = FocalWindow(np.array([[-1, 1, -1, 1, 1], [0, 2, 0, 2, 1]], np.int32), 17, 18)
    minus = FocalWindow(np.array([[-1, 1, -1, 1, 1], [1, 2, 0, 0, -1]], np.int32), 7, 9)
    for bad, text in ((twice, "0 or 1 times"), (minus, "0 or 1 times"), (focal_window("box", 33), "at most 32 cells"),
                      (focal_window("disc", 33), "at most 32 cells"), (np.ones((4, 3), bool), "odd sizes"), (np.ones(3, bool), "odd sizes"),
                      (np.ones((67, 1), bool), "at most 32 cells"), (np.zeros((3, 3), bool), "row runs")):
        with pytest.raises(ValueError, match=text):
            _window_runs(bad)
    wide = np.zeros((67, 67), bool)
    wide[1:-1, 1:-1] = True                                  # a border of cells that do not belong may lie beyond the reach
    assert np.array_equal(_window_runs(wide), _window_runs(np.ones((65, 65), bool)))
    teeth = np.zeros((65, 7), bool)
    teeth[:, ::2] = True                                     # 4 runs a row over 65 rows
    with pytest.raises(ValueError, match="1 .. 130 row runs"):
        _window_runs(teeth)


# ---- every Python-side rejection ---------------------------------------------------------------------------------------------------
def test_python_rejections_need_no_device():
    z = np.zeros((6, 7), np.float32)
    box = focal_window("box", 1)
    calls = [
        (lambda: dsm.focal_quantiles(z.astype(np.float64), box), "float32"),
        (lambda: dsm.focal_quantiles(z[0], box), r"\(gh, gw\)"),
        (lambda: dsm.focal_quantiles(z, focal_window("box", 40)), "at most 32 cells"),
        (lambda: dsm.focal_quantiles(z, box, q=()), "non-empty"),
        (lambda: dsm.focal_quantiles(z, box, q=(1.5,)), r"in \[0, 1\]"),
        (lambda: dsm.focal_quantiles(z, box, method="cubic"), "method must be one of"),
        (lambda: dsm.focal_quantiles(z, box, centre=np.zeros((6, 6), np.float32)), "centre is float32"),
        (lambda: dsm.focal_quantiles(z, box, centre=z.astype(np.float64)), "centre is float32"),
        (lambda: dsm.focal_quantiles(z, box, min_valid=-1), "min_valid"),
        (lambda: dsm.focal_quantiles(z, box, min_valid=1.5), "min_valid"),
        (lambda: dsm.focal_median(z.astype(np.float64), box), "float32"),
        (lambda: dsm.focal_median(z, np.ones((2, 2), bool)), "odd sizes"),
        (lambda: dsm.focal_median(z, box, min_valid=-2), "min_valid"),
        (lambda: dsm.focal_nmad(z, focal_window("disc", 33)), "at most 32 cells"),
        (lambda: dsm.focal_nmad(z, box, min_valid=True), "min_valid"),
        (lambda: dsm.despike_robust(z, box, k=-1.0), "k and floor"),
        (lambda: dsm.despike_robust(z, box, floor=float("nan")), "floor"),
        (lambda: dsm.despike_robust(z, box, min_valid=0), "min_valid"),
        (lambda: dsm.despike_robust(z.astype(np.int32), box), "float32"),
        (lambda: dsm.focal_counts(z, box, threshold=np.zeros((7, 6), np.float32)), "threshold is float32"),
        (lambda: dsm.focal_counts(z, box, threshold="high"), "threshold is float32"),
        (lambda: dsm.focal_counts(z, np.zeros((3, 3), bool)), "row runs"),
        (lambda: dsm.elevation_percentile(z, box, min_valid=-1), "min_valid"),
        (lambda: dsm.elevation_percentile(z.astype(np.float16), box), "float32"),
    ]
    for call, text in calls:
        with pytest.raises(ValueError, match=text):
            call()


# ---- the elevation percentile by hand ---------------------------------------------------------------------------------------------
def test_elevation_percentile_on_a_hand_made_window():
    nan = np.float32(np.nan)
    z = np.array([[1.0, 2.0, 2.0],
                  [5.0, 2.0, nan],
                  [-999.0, 9.0, 0.0]], np.float32)
    for count in (ro.count_loop, ro.count_sorted):
        n, below, equal = count(z, ro.footprint("box", 1), z)
        assert (n[1, 1], below[1, 1], equal[1, 1]) == (7, 2, 3)                  # 0, 1 below; three 2s; 5 and 9 above
        p = ro.elevation_percentile(z, ro.footprint("box", 1), count=count)
        assert p[1, 1] == (2 + 0.5 * 2) / 6                   # the three 2s hold ranks 2, 3, 4 of 0 .. 6: their middle is 3
        assert p[2, 2] == 0.0 and p[2, 1] == 1.0              # the lowest and the highest of their windows
        assert np.isnan(p[1, 2]) and np.isnan(p[2, 0])        # no height, no percentile
        assert p[0, 0] == 0.0 and p[0, 1] == (1 + 0.5 * 2) / 4                   # 1 | 2 2 2 | 5
        assert np.isnan(ro.elevation_percentile(z, ro.footprint("box", 1), min_valid=8, count=count)).all()
    lone = np.full((3, 3), nan, np.float32)
    lone[1, 1] = 4.0
    assert np.isnan(ro.elevation_percentile(lone, ro.footprint("box", 1))).all()                  # n = 1: no neighbour to rank against
