"""Registration, the parts that run without a GPU: the two numpy statements of the shift statistics and of the regrid
(tests/dsm_coreg_oracle.py) against each other, the selection rule of coregister (exact integers against a float64 argmin, the
tie order, the sub-cell vertex), the argument checks of smvs_dsm_shift_stats / smvs_dsm_regrid (rejected before any HIP call)
and of the Python functions (before any device work), and the case matrix of tests/dsm_coreg_scene.py."""
import ctypes as C
import math

import numpy as np
import pytest

import dsm_coreg_oracle as co
import dsm_coreg_scene as cs
from dsm_testkit import lib, same  # noqa: F401  (fixtures)


# ---- the oracle against itself -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,a,offset,radius", [((1, 1), (1, 1), (0, 0), 1), ((5, 9), (7, 6), (-1, 2), 2), ((9, 12), (9, 12), (0, 0), 3),
                                               ((6, 7), (4, 20), (8, -3), 4), ((4, 4), (4, 4), (30, 0), 2)])
def test_shift_stats_statements_agree(b, a, offset, radius):
    za, zb = cs.special_grid(*a, seed=1), cs.special_grid(*b, seed=2)
    for dz0, trim in ((0.0, 256.0), (cs.DZ0, cs.TRIM), (-1.0, 0.5)):
        fast = co.shift_stats(za, zb, *offset, radius, dz0, trim)
        slow = co.shift_stats_loop(za, zb, *offset, radius, dz0, trim)
        assert fast.dtype == np.int64 and fast.shape == (2 * radius + 1, 2 * radius + 1, 3)
        assert np.array_equal(fast, slow), (dz0, trim)
    assert co.shift_stats(za, zb, *offset, radius, 0.0, 256.0)[..., 0].max() > 0 or offset[0] == 30


def test_shift_stats_rules_on_known_values():
    b = np.zeros((1, 6), np.float32)
    a = np.array([[0.5, 1.5, -0.5, -1.5, 2.5, -0.0]], np.float32) / np.float32(256.0)
    st = co.shift_stats(a, b, radius=0)
    assert st.tolist() == [[[6, 0 + 2 + 0 - 2 + 2 + 0, 0 + 4 + 0 + 4 + 4 + 0]]]          # halves to even
    a = np.array([[2.5, -2.5, 5.0, np.nan, np.inf, -999.0]], np.float32)
    assert co.shift_stats(a, b, radius=0, trim=2.5)[0, 0].tolist() == [2, 0, 2 * 640 * 640]         # |d| == trim counts
    assert co.shift_stats(a, b, radius=0, trim=np.nextafter(2.5, 0.0))[0, 0, 0] == 0
    below = float(np.nextafter(2.5, 0.0))
    assert (5.0 - below) == float(np.nextafter(2.5, 3.0))                                  # one float64 ulp above the trim
    assert co.shift_stats(a, b, radius=0, dz0=below, trim=2.5)[0, 0].tolist() == [1, 0, 0]      # 2.5 - dz0 alone; 5 - dz0 is out
    assert co.shift_stats(a, b, radius=0, dz0=2.5, trim=2.5)[0, 0].tolist() == [2, 640 - 0, 640 * 640]      # 5 - 2.5 and 2.5 - 2.5
    assert co.shift_stats(a, b, radius=0)[0, 0, 0] == 3 and co.shift_stats(a, b, radius=0, nodata=5.0)[0, 0, 0] == 2     # another nodata
    st = co.shift_stats(np.full((4, 4), 256.0, np.float32), np.zeros((4, 4), np.float32), radius=1)
    assert st[1, 1].tolist() == [16, 16 * 2 ** 16, 16 * 2 ** 32] and st[0, 0, 0] == 9


@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
def test_regrid_statements_agree(mode):
    src = cs.special_grid(9, 13, seed=5)
    gs = cs.Grid(9, 13, 1000.0, 2000.0, 5.0, 2.5)
    for gd in (gs, cs.Grid(4, 5, 1010.0, 1995.0, 5.0, 2.5), cs.Grid(12, 16, 990.0, 2005.0, 5.0, 2.5), cs.Grid(9, 13, 1002.5, 1998.75, 5.0, 2.5),
               cs.Grid(18, 26, 998.75, 2000.625, 2.5, 1.25), cs.Grid(5, 7, 1002.5, 1998.75, 10.0, 5.0), cs.Grid(6, 6, 1001.0, 1999.0, 3.0, 3.0)):
        for dz in (0.0, -1.25):
            same(co.regrid(src, gs, gd, mode, dz), co.regrid_loop(src, gs, gd, mode, dz), (mode, dz, gd.e0))
    own = co.regrid(src, gs, gs, mode)
    ok = np.isfinite(src) & (src != np.float32(-999.0))
    assert np.array_equal(own.view(np.uint32)[ok], src.view(np.uint32)[ok]) and (own[~ok] == np.float32(-999.0)).all()
    assert np.signbit(own[ok & (src == 0.0)]).all()                                        # -0.0 keeps its sign with dz = 0


# ---- the selection rule --------------------------------------------------------------------------------------------------------
def _stats(entries, R=1, fill=(0, 0, 0)):
    st = np.zeros((2 * R + 1, 2 * R + 1, 3), np.int64)
    st[:] = fill
    for (sx, sy), v in entries.items():
        st[sy + R, sx + R] = v
    return st


def test_exact_integers_decide_where_floats_tie():
    """Two shifts whose variances differ by 1 / n^2 at a mean of 2^27 q: n S2 - S1^2 differs by n in integers, while
    S2 / n - (S1 / n)^2 rounds both to the same float64 (the terms are near 2^54, where floats step by 4)."""
    from satmvs_amd import dsm
    n, m = 3, 2 ** 27
    s1 = n * m + 1                                           # a mean just off m
    k0 = (-(s1 * s1)) % n                                    # S2 = (S1^2 + k) / n must be an integer
    st = _stats({(0, 0): (n, s1, (s1 * s1 + k0 + 2 * n) // n), (1, 0): (n, s1, (s1 * s1 + k0 + n) // n)})
    num = {s: n * int(st[1, s + 1, 2]) - s1 * s1 for s in (0, 1)}
    assert num[1] < num[0] and num[0] - num[1] == n
    fx, fy, var = co.best_shift_float(st, 0.5)
    assert var[1, 1] == var[1, 2]                            # the float64 variances tie ...
    assert (fx, fy) == (0, 0)                                # ... and the float argmin keeps the first
    pick = dsm.best_shift(st, 0.5)
    assert pick["shift"] == (1, 0) and co.best_shift(st, 0.5)[:2] == (1, 0)               # the integers do not
    assert pick["n"] == n and pick["sum_q"] == s1


def test_tie_order():
    from satmvs_amd import dsm
    v = (10, 5, 100)
    every = {(sx, sy): v for sx in (-1, 0, 1) for sy in (-1, 0, 1)}
    assert dsm.best_shift(_stats(every))["shift"] == (0, 0)                               # the smallest sx^2 + sy^2
    del every[0, 0]
    assert dsm.best_shift(_stats(every))["shift"] == (0, -1)                              # then the lower sy
    del every[0, -1]
    assert dsm.best_shift(_stats(every))["shift"] == (-1, 0)                              # then the lower sx (sy = 0 for both)
    del every[-1, 0], every[1, 0]
    assert dsm.best_shift(_stats(every))["shift"] == (0, 1)
    del every[0, 1]
    assert dsm.best_shift(_stats(every))["shift"] == (-1, -1)
    for st in (_stats(every), _stats({(0, 0): v, (1, 1): (10, 5, 99)}), _stats({(1, 0): v, (-1, 0): v})):
        pick, want = dsm.best_shift(st), co.best_shift(st)
        assert (pick["shift"] + pick["subcell"] + (pick["n"], pick["sum_q"])) == want


def test_eligibility_and_subcell():
    from satmvs_amd import dsm
    # variance n S2 - S1^2 over n^2 with S1 = 0: S2 / n
    st = _stats({(-1, 0): (100, 0, 900), (0, 0): (100, 0, 100), (1, 0): (100, 0, 500), (0, -1): (100, 0, 300), (0, 1): (49, 0, 0)})
    pick = dsm.best_shift(st, 0.5)
    assert pick["shift"] == (0, 0)                           # (0, 1) has the least spread but under half the pairs
    assert pick["subcell"][0] == 0.5 * (9.0 - 5.0) / (9.0 - 2.0 + 5.0) and pick["subcell"][1] == 0.0    # a neighbour not eligible
    assert dsm.best_shift(st, 0.49)["shift"] == (0, 1)
    assert dsm.best_shift(st, 0.0)["shift"] == (0, 1)
    flat = _stats({(-1, 0): (10, 0, 10), (0, 0): (10, 0, 10), (1, 0): (10, 0, 10)})
    assert dsm.best_shift(flat)["subcell"] == (0.0, 0.0)     # the denominator is 0
    steep = _stats({(-1, 0): (10, 0, 11), (0, 0): (10, 0, 10), (1, 0): (10, 0, 1000)})
    assert dsm.best_shift(steep)["shift"] == (0, 0) and -0.5 <= dsm.best_shift(steep)["subcell"][0] < 0.0
    edge = _stats({(1, 1): (10, 0, 10), (0, 1): (10, 0, 20)})
    assert dsm.best_shift(edge)["shift"] == (1, 1) and dsm.best_shift(edge)["subcell"] == (0.0, 0.0)     # no neighbour beyond the radius
    assert dsm.best_shift(_stats({})) is None and dsm.best_shift(_stats({(0, 0): (1, 3, 9)})) is None   # fewer than two pairs
    assert co.best_shift(_stats({})) is None
    with pytest.raises(ValueError, match="min_overlap"):
        dsm.best_shift(st, 1.5)
    with pytest.raises(ValueError, match="stats is"):
        dsm.best_shift(np.zeros((3, 2, 3), np.int64))


def test_case_matrix_covers_the_kernel_paths():
    """What the GPU tests assume about tests/dsm_coreg_scene.py: remainders, workgroup counts, shifts per lane, parts, overlaps."""
    by_name = {c.name: c for c in cs.SHAPE_CASES}
    assert len(by_name) == len(cs.SHAPE_CASES)
    rem = {(c.b[1] % cs.TW, c.b[0] % cs.TH) for c in cs.SHAPE_CASES}
    assert {(0, 0), (1, 1), (cs.TW - 1, cs.TH - 1)} <= rem
    tiles = lambda c: -(-c.b[1] // cs.TW) * -(-c.b[0] // cs.TH)
    assert tiles(by_name["every workgroup twice"]) >= 2 * 1024 and tiles(by_name["8 x 8"]) == 1 and tiles(by_name["300 x 700"]) > 200
    per_lane = {next(ns for ns in (1, 2, 3, 5, 9, 13, 17) if ns * 256 >= (2 * c.radius + 1) ** 2) for c in cs.SHAPE_CASES}
    assert per_lane == {1, 2, 3, 5, 9, 13, 17}
    parts = {256 // (1 << max(0, math.ceil(math.log2((2 * c.radius + 1) ** 2)))) for c in cs.SHAPE_CASES if c.radius <= 7}
    assert parts == {256, 16, 8, 4, 2, 1}
    assert {0, 1, 7, 8, 32} <= {c.radius for c in cs.SHAPE_CASES}
    for name, none in (("ox beyond a", True), ("far beyond", True), ("oy beyond", True), ("negative offsets, partial overlap", False)):
        c = by_name[name]
        a, b = cs.case_grids(c)
        n = co.shift_stats(a, b, *c.offset, min(c.radius, 8), cs.DZ0, cs.TRIM)[..., 0] if abs(c.offset[0]) < 10 ** 6 else np.zeros(1)
        assert (n.max() == 0) == none and (none or n.min() == 0), name        # partial: some shifts have pairs and some none
    a, b = cs.case_grids(by_name["radius 8"])
    for v in (np.nan, np.inf, -np.inf, -999.0):
        assert (a == v).any() or (np.isnan(v) and np.isnan(a).any())
    assert (np.signbit(a) & (a == 0)).any() and (np.signbit(b) & (b == 0)).any()


# ---- argument checks -----------------------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_a_gpu(lib):
    from satmvs_amd import _lib
    MB = 1 << 20
    pa, pb, ps, pw = C.c_void_p(1 * MB), C.c_void_p(2 * MB), C.c_void_p(3 * MB), C.c_void_p(64 * MB)
    query = lib.smvs_dsm_shift_workspace_bytes
    need = query(8, 8, 8, 8, 8)
    assert need >= 17 * 17 * 3 * 8
    assert query(300, 300, 1505, 1537, 1) >= 1024 * 9 * 24 and query(8, 8, 8, 8, 0) >= 24 and query(8, 8, 8, 8, 32) >= 65 * 65 * 24
    for bad in ((0, 8, 8, 8, 8), (8, -1, 8, 8, 8), (8, 8, 0, 8, 8), (8, 8, 8, 0, 8), (65536, 32768, 8, 8, 8), (8, 8, 65536, 32768, 8),
                (8, 8, 8, 8, -1), (8, 8, 8, 8, 33)):
        assert query(*bad) == 0, bad

    def shift(a=pa, gwa=8, gha=8, b=pb, gwb=8, ghb=8, ox=0, oy=0, radius=8, dz0=0.0, trim=10.0, stats=ps, ws=pw, nbytes=need):
        _lib.call("smvs_dsm_shift_stats", a, gwa, gha, b, gwb, ghb, -999.0, ox, oy, radius, dz0, trim, stats, ws, nbytes, None)

    for kw in ({"a": None}, {"b": None}, {"stats": None}, {"ws": None}):
        with pytest.raises(_lib.SatMVSNativeError, match="null pointer"):
            shift(**kw)
    for kw in ({"gwa": 0}, {"gha": -2}, {"gwb": 0}, {"ghb": 0}):
        with pytest.raises(_lib.SatMVSNativeError, match="non-positive grid"):
            shift(**kw)
    for kw in ({"gwa": 65536, "gha": 32768}, {"gwb": 65536, "ghb": 32768}):
        with pytest.raises(_lib.SatMVSNativeError, match="grid too large"):
            shift(**kw)
    for r in (-1, 33, 2 ** 20):
        with pytest.raises(_lib.SatMVSNativeError, match="radius must be"):
            shift(radius=r)
    for kw in ({"ox": 2 ** 30}, {"ox": -(2 ** 30)}, {"oy": 2 ** 30}, {"oy": -(2 ** 31)}):
        with pytest.raises(_lib.SatMVSNativeError, match="offset out of range"):
            shift(**kw)
    for v in (math.nan, math.inf, -math.inf):
        with pytest.raises(_lib.SatMVSNativeError, match="dz0 must be finite"):
            shift(dz0=v)
    for v in (0.0, -1.0, math.nan, math.inf, float(np.nextafter(256.0, 300.0))):
        with pytest.raises(_lib.SatMVSNativeError, match="trim must be"):
            shift(trim=v)
    with pytest.raises(_lib.SatMVSNativeError, match="workspace too small"):
        shift(nbytes=need - 1)
    nstats = 17 * 17 * 24
    for bad in (MB + 255, MB - nstats + 1, 2 * MB, 2 * MB + 8 * 8 * 4 - 1):
        with pytest.raises(_lib.SatMVSNativeError, match="stats aliases"):
            shift(stats=C.c_void_p(bad))
    for bad in (MB - need + 1, MB + 8, 2 * MB + 255, 3 * MB - need + 1, 3 * MB + nstats - 1):
        with pytest.raises(_lib.SatMVSNativeError, match="workspace aliases"):
            shift(ws=C.c_void_p(bad))

    g = np.array([0.0, 0.0, 5.0, 5.0])

    def regrid(src=pa, gws=8, ghs=8, gs=g, gd=g, gwd=8, ghd=8, mode=1, dz=0.0, out=pb):
        p = [None if x is None else x.ctypes.data_as(C.c_void_p) for x in (gs, gd)]
        _lib.call("smvs_dsm_regrid", src, gws, ghs, p[0], -999.0, p[1], gwd, ghd, mode, dz, out, None)

    for kw in ({"src": None}, {"gs": None}, {"gd": None}, {"out": None}):
        with pytest.raises(_lib.SatMVSNativeError, match="null pointer"):
            regrid(**kw)
    for kw in ({"gws": 0}, {"ghs": 0}, {"gwd": -1}, {"ghd": 0}):
        with pytest.raises(_lib.SatMVSNativeError, match="non-positive grid"):
            regrid(**kw)
    for kw in ({"gws": 65536, "ghs": 32768}, {"gwd": 65536, "ghd": 32768}):
        with pytest.raises(_lib.SatMVSNativeError, match="grid too large"):
            regrid(**kw)
    for which in ("gs", "gd"):
        for k in (0, 1):
            for v in (math.nan, math.inf):
                bad = g.copy()
                bad[k] = v
                with pytest.raises(_lib.SatMVSNativeError, match="origin must be finite"):
                    regrid(**{which: bad})
        for k in (2, 3):
            for v in (0.0, -5.0, math.nan, math.inf):
                bad = g.copy()
                bad[k] = v
                with pytest.raises(_lib.SatMVSNativeError, match="resolutions must be"):
                    regrid(**{which: bad})
    for m in (-1, 2, 7):
        with pytest.raises(_lib.SatMVSNativeError, match="mode must be"):
            regrid(mode=m)
    for v in (math.nan, -math.inf):
        with pytest.raises(_lib.SatMVSNativeError, match="dz must be finite"):
            regrid(dz=v)
    for bad in (MB, MB + 255, MB - 255):
        with pytest.raises(_lib.SatMVSNativeError, match="out aliases src"):
            regrid(out=C.c_void_p(bad))


def test_python_entries_validate_before_the_gpu():
    import torch
    from satmvs_amd import dsm
    z = np.zeros((4, 6), np.float32)
    grid = dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, 6, 4)
    wide = dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, 7, 4)
    coarse = dsm.DSMGrid(0.0, 0.0, 10.0, 5.0, 6, 4)
    tall = dsm.DSMGrid(0.0, 0.0, 5.0, 2.5, 6, 4)
    cases = [
        (lambda: dsm.regrid(z, wide, grid), "differs from the grid"),
        (lambda: dsm.regrid(z, grid, grid, mode="cubic"), "mode must be"),
        (lambda: dsm.regrid(z, grid, grid, dz=float("nan")), "dz must be finite"),
        (lambda: dsm.regrid(z, grid, dsm.DSMGrid(0.0, 0.0, 0.0, 5.0, 6, 4)), "to_grid needs"),
        (lambda: dsm.regrid(z, dsm.DSMGrid(float("inf"), 0.0, 5.0, 5.0, 6, 4), grid), "grid needs"),
        (lambda: dsm.regrid(z, grid, dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, 0, 4)), "positive sizes"),
        (lambda: dsm.shift_stats(z.astype(np.float64), z), "float32"),               # the strict policy: never converted
        (lambda: dsm.shift_stats(z, torch.zeros(4, 6, dtype=torch.float16)), "float32"),
        (lambda: dsm.shift_stats(z[0], z), r"\(gh, gw\)"),
        (lambda: dsm.shift_stats(z, z, offset=(0.5, 0)), "pair of integers"),
        (lambda: dsm.shift_stats(z, z, offset=(0, 2 ** 30)), "offset must be"),
        (lambda: dsm.shift_stats(z, z, radius=-1), "radius"),
        (lambda: dsm.shift_stats(z, z, radius=33), "radius"),
        (lambda: dsm.shift_stats(z, z, radius=2.0), "radius"),
        (lambda: dsm.shift_stats(z, z, dz0=float("inf")), "dz0 must be finite"),
        (lambda: dsm.shift_stats(z, z, trim=0.0), "trim must be"),
        (lambda: dsm.shift_stats(z, z, trim=256.5), "trim must be"),
        (lambda: dsm.shift_stats(z, z, trim=float("nan")), "trim must be"),
        (lambda: dsm.coregister(z, grid, z, coarse), "regrid"),                      # unequal resolution names the way out
        (lambda: dsm.coregister(z, grid, z, tall), "regrid"),
        (lambda: dsm.coregister(z, wide, z, grid), "differs from the grid"),
        (lambda: dsm.coregister(z.astype(np.float64), grid, z, grid), "float32"),
        (lambda: dsm.coregister(z, grid, z, grid, radius=40), "radius"),
        (lambda: dsm.coregister(z, grid, z, grid, trim=-1.0), "trim must be"),
        (lambda: dsm.coregister(z, grid, z, grid, min_overlap=1.5), "min_overlap"),
        (lambda: dsm.coregister(z, grid, z, grid, min_overlap=float("nan")), "min_overlap"),
        (lambda: dsm.coregister(z, grid, z, grid, rounds=0), "rounds"),
        (lambda: dsm.coregister(z, grid, z, dsm.DSMGrid(1e13, 0.0, 5.0, 5.0, 6, 4)), "no overlap"),
        (lambda: dsm.compare_dsms(z, grid, z, wide), "differs from the grid"),
        (lambda: dsm.changes(z, grid, z, wide), "differs from the grid"),
    ]
    for f, pattern in cases:
        with pytest.raises(ValueError, match=pattern):
            f()
