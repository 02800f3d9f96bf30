"""Registration on the device against the numpy oracle (tests/dsm_coreg_oracle.py): the shift statistics over the case matrix
of tests/dsm_coreg_scene.py and the edge values, compared with np.array_equal; the regrid compared bit for bit; coregister,
compare_dsms and changes end to end on displaced synthetic scenes.  No tolerances except where the issue of a test is a
measured quantity (dz within 0.05 m of the truth, the sub-cell step within 0.25 cells)."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import dsm_coreg_oracle as co
import dsm_coreg_scene as cs
from dsm_testkit import dev, lib, same  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
ND = np.float32(-999.0)


def _grid(g):
    from satmvs_amd import dsm
    return dsm.DSMGrid(g.e0, g.n0, g.xres, g.yres, g.width, g.height)


# ---- shift statistics ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cs.SHAPE_CASES, ids=[c.name for c in cs.SHAPE_CASES])
def test_shift_stats_shape_matrix(dev, case):
    from satmvs_amd import dsm
    a, b = cs.case_grids(case)
    got = dsm.shift_stats(a, b, case.offset, case.radius, cs.DZ0, cs.TRIM)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64
    want = co.shift_stats(a, b, *case.offset, case.radius, cs.DZ0, cs.TRIM)
    assert np.array_equal(got, want), (case.name, int((got != want).any(-1).sum()), np.argwhere((got != want).any(-1))[:5].tolist())
    if "beyond" in case.name:
        assert not got.any()
    if "partial overlap" in case.name:
        assert (got[..., 0] == 0).any() and (got[..., 0] > 0).any() and not got[got[..., 0] == 0].any()


def test_edge_values(dev):
    from satmvs_amd import dsm
    b = np.zeros((1, 6), np.float32)
    halves = np.array([[0.5, 1.5, -0.5, -1.5, 2.5, -0.0]], np.float32) / np.float32(256.0)
    assert dsm.shift_stats(halves, b, radius=0).tolist() == [[[6, 2, 12]]]                 # halves go to even
    a = np.array([[2.5, -2.5, 5.0, np.nan, np.inf, -999.0]], np.float32)
    below = float(np.nextafter(2.5, 0.0))
    for kw in ({"trim": 2.5}, {"trim": below}, {"dz0": below, "trim": 2.5}, {"dz0": 2.5, "trim": 2.5}, {"nodata": 5.0}, {"dz0": -3.0, "trim": 0.5}):
        got, want = dsm.shift_stats(a, b, radius=0, **kw), co.shift_stats(a, b, radius=0, **kw)
        assert np.array_equal(got, want), (kw, got.tolist(), want.tolist())
    assert dsm.shift_stats(a, b, radius=0, trim=2.5)[0, 0, 0] == 2                         # |d| == trim is counted
    assert dsm.shift_stats(a, b, radius=0, trim=below)[0, 0, 0] == 0
    assert dsm.shift_stats(a, b, radius=0, dz0=below, trim=2.5)[0, 0, 0] == 1              # 5 - dz0 is one ulp above the trim
    for nodata in (0.0, 100.1, float("nan")):                # 100.1 occurs in the special grids; a NaN nodata leaves finiteness alone
        za, zb = cs.special_grid(33, 70, 3), cs.special_grid(33, 70, 4)
        got = dsm.shift_stats(za, zb, (1, -1), 3, cs.DZ0, cs.TRIM, nodata=nodata)
        assert np.array_equal(got, co.shift_stats(za, zb, 1, -1, 3, cs.DZ0, cs.TRIM, nodata=nodata)), nodata


def test_sums_beyond_32_bits(dev):
    """1024 x 1024 cells of |d| = trim = 256: sum q = 2^36 and sum q^2 = 2^52 at the centre shift."""
    from satmvs_amd import dsm
    a = torch.full((1024, 1024), 256.0, dtype=torch.float32, device=dev)
    b = torch.zeros((1024, 1024), dtype=torch.float32, device=dev)
    got = dsm.shift_stats(a, b, radius=1, trim=256.0).cpu().numpy()
    n = np.array([[(1024 - abs(sx)) * (1024 - abs(sy)) for sx in (-1, 0, 1)] for sy in (-1, 0, 1)], np.int64)
    assert np.array_equal(got[..., 0], n) and np.array_equal(got[..., 1], n * 2 ** 16) and np.array_equal(got[..., 2], n * 2 ** 32)
    assert got[1, 1].tolist() == [2 ** 20, 2 ** 36, 2 ** 52]
    neg = dsm.shift_stats(b, a, radius=1, trim=256.0).cpu().numpy()
    assert np.array_equal(neg[..., 1], -n * 2 ** 16) and np.array_equal(neg[..., 2], n * 2 ** 32)


def test_entry_initialises_guards_and_repeats(dev, lib):
    """The C entry with garbage in stats, guard words around stats and the workspace, twice, and on a side stream."""
    from satmvs_amd import _lib
    case = next(c for c in cs.SHAPE_CASES if c.name == "300 x 700")
    a, b = cs.case_grids(case)
    za, zb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    (gha, gwa), (ghb, gwb), R = a.shape, b.shape, case.radius
    want = co.shift_stats(a, b, *case.offset, R, cs.DZ0, cs.TRIM)
    nbytes = lib.smvs_dsm_shift_workspace_bytes(gwa, gha, gwb, ghb, R)
    nstats, guard = (2 * R + 1) ** 2 * 3, 64
    runs = []
    for stream in (None, None, torch.cuda.Stream(dev)):
        stats = torch.full((nstats + 2 * guard,), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device=dev)
        ws = torch.full((nbytes + 512,), 0xa5, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            _lib.call("smvs_dsm_shift_stats", _lib.ptr(za), gwa, gha, _lib.ptr(zb), gwb, ghb, -999.0, case.offset[0], case.offset[1], R,
                      cs.DZ0, cs.TRIM, C.c_void_p(stats.data_ptr() + 8 * guard), C.c_void_p(ws.data_ptr() + 256), nbytes, _lib.current_stream(dev))
        torch.cuda.synchronize()
        s, w = stats.cpu().numpy(), ws.cpu().numpy()
        assert (s[:guard] == 0x5a5a5a5a5a5a5a5a).all() and (s[-guard:] == 0x5a5a5a5a5a5a5a5a).all()
        assert (w[:256] == 0xa5).all() and (w[-256:] == 0xa5).all()
        runs.append(s[guard:-guard].reshape(want.shape))
    assert all(np.array_equal(r, want) for r in runs)


def test_python_inputs(dev):
    from satmvs_amd import dsm
    a, b = cs.special_grid(40, 90, 7), cs.special_grid(33, 70, 8)
    want = co.shift_stats(a, b, 2, 1, 4, cs.DZ0, cs.TRIM)
    ta, tb = torch.from_numpy(np.ascontiguousarray(a.T)).to(dev).T, torch.from_numpy(b).to(dev)          # a not contiguous
    assert not ta.is_contiguous()
    got = dsm.shift_stats(ta, tb, (2, 1), 4, cs.DZ0, cs.TRIM)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int64 and got.shape == (9, 9, 3) and np.array_equal(got.cpu().numpy(), want)
    wide = np.zeros((40, 180), np.float32)
    wide[:, ::2] = a
    assert np.array_equal(dsm.shift_stats(wide[:, ::2], b, (2, 1), 4, cs.DZ0, cs.TRIM), want)           # numpy, strided
    assert np.array_equal(dsm.shift_stats(a, tb, (2, 1), 4, cs.DZ0, cs.TRIM), want)                     # mixed: numpy decides


# ---- regrid --------------------------------------------------------------------------------------------------------------------
GS = cs.Grid(37, 70, 1000.0, 2000.0, 5.0, 2.5)
TARGETS = {"own": GS, "crop": cs.Grid(12, 20, 1015.0, 1990.0, 5.0, 2.5), "overhang": cs.Grid(45, 80, 980.0, 2007.5, 5.0, 2.5),
           "half cell": cs.Grid(37, 70, 1002.5, 1998.75, 5.0, 2.5), "finer": cs.Grid(74, 140, 998.75, 2000.625, 2.5, 1.25),
           "coarser": cs.Grid(19, 35, 1002.5, 1998.75, 10.0, 5.0), "skew": cs.Grid(300, 280, 999.0, 2001.0, 1.3, 0.7)}


@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
@pytest.mark.parametrize("target", sorted(TARGETS))
def test_regrid(dev, target, mode):
    from satmvs_amd import dsm
    src, gd = cs.special_grid(GS.height, GS.width, 21), TARGETS[target]
    for dz in (0.0, 1.625):
        got = dsm.regrid(src, _grid(GS), _grid(gd), mode, dz)
        same(got, co.regrid(src, GS, gd, mode, dz), (target, mode, dz))
    if target in ("own", "crop"):                            # a crop of the bits at valid cells, nodata at the others
        own = dsm.regrid(src, _grid(GS), _grid(gd), mode)
        r0, c0 = (0, 0) if target == "own" else (4, 3)
        part = src[r0:r0 + own.shape[0], c0:c0 + own.shape[1]]
        ok = np.isfinite(part) & (part != ND)
        assert np.array_equal(own.view(np.uint32)[ok], part.view(np.uint32)[ok]) and (own[~ok] == ND).all() and ok.any() and (~ok).any()


def test_regrid_taps_and_small_sources(dev):
    from satmvs_amd import dsm
    src = np.array([[1.0, np.nan], [3.0, 5.0]], np.float32)
    g = dsm.DSMGrid(0.0, 0.0, 1.0, 1.0, 2, 2)
    at = lambda e, n: dsm.regrid(src, g, dsm.DSMGrid(e, n, 1.0, 1.0, 1, 1))[0, 0]
    assert at(0.0, 0.0) == 1.0 and at(0.0, -1.0) == 3.0      # the NaN lies under a zero weight: not read
    assert at(0.0, -0.5) == 2.0 and at(0.5, -1.0) == 4.0
    assert at(0.5, 0.0) == ND and at(0.25, -0.5) == ND       # under a non-zero weight: nodata
    assert at(1.0, 0.0) == ND and at(1.0, -1.0) == 5.0 and at(1.5, -1.0) == ND and at(-0.5, 0.0) == ND
    one = np.array([[7.5]], np.float32)
    g1 = dsm.DSMGrid(10.0, 20.0, 2.0, 2.0, 1, 1)
    for mode in ("nearest", "bilinear"):
        got = dsm.regrid(one, g1, dsm.DSMGrid(8.0, 22.0, 1.0, 1.0, 5, 5), mode, dz=0.5)
        same(got, co.regrid(one, cs.Grid(1, 1, 10.0, 20.0, 2.0, 2.0), cs.Grid(5, 5, 8.0, 22.0, 1.0, 1.0), mode, 0.5), mode)
        assert got[2, 2] == 8.0 and (got == 8.0).sum() == (4 if mode == "nearest" else 1)
    t = dsm.regrid(torch.from_numpy(src).to(dev).double(), g, g, "nearest")                # the converting policy
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t[1, 1] == 5.0


# ---- end to end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", cs.DISPLACED, ids=["%dx%d" % s[:2] for s in cs.DISPLACED])
def test_coregister_recovers_the_displacement(dev, scene):
    from satmvs_amd import dsm
    gh, gw, seed, radius, sx, sy, dz = scene
    a, ga, b, gb = cs.displaced(*scene)
    got = dsm.coregister(a, _grid(ga), b, _grid(gb), radius=radius)
    print("coregister %s: shift %s subcell %s dz %.4f (truth %s, %.2f) n %d std %.3f m" % (scene[:2], got["shift_cells"], got["subcell"], got["dz"], (sx, sy), dz, got["n"], got["std"]))
    assert got["shift_cells"] == (sx, sy) and got["offset"] == (1, 1)
    assert abs(got["dz"] - dz) < 0.05
    for k in (0, 1):                                         # every round agrees with the rule on the oracle's statistics
        trim, dz0 = (256.0, 0.0) if k == 0 else (10.0, dz1)
        want = co.shift_stats(a, b, 1, 1, radius, dz0, trim)
        pick = co.best_shift(want)
        dz1 = dz0 + pick[5] / (256.0 * pick[4])
    assert np.array_equal(got["stats"], want) and got["shift_cells"] + got["subcell"] == pick[:4] and got["dz"] == dz1 and got["n"] == pick[4]
    assert got["de"] == (0.0 - sx - got["subcell"][0]) * cs.RES and got["dn"] == (sy + got["subcell"][1] - 0.0) * cs.RES
    assert got["grid"].e0 == ga.e0 + got["de"] and got["grid"].n0 == ga.n0 + got["dn"] and got["grid"].width == ga.width
    assert 0.2 < got["std"] < 0.6                            # a - b is the sigma = 0.3 m noise, quantised to 2^-8 m
    one = dsm.coregister(a, _grid(ga), b, _grid(gb), radius=radius, rounds=1)
    assert one["shift_cells"] == (sx, sy)                    # recovered in both rounds


def test_half_cell_displacement(dev):
    """b = the scene, a = the scene resampled half a cell east with regrid; the georeference of a claims no displacement."""
    from satmvs_amd import dsm
    b, gb = cs.textured(80, 100, 9)
    smooth = dsm.fill_voids(np.ascontiguousarray(b), max_steps=8, min_hits=1)
    g = _grid(gb)
    half = dsm.DSMGrid(g.e0 + 0.5 * cs.RES, g.n0, g.xres, g.yres, g.width, g.height)
    a = dsm.regrid(smooth, g, half)                          # a's cell c holds the scene at c + 1/2
    got = dsm.coregister(a, g, np.ascontiguousarray(b), g, radius=3)
    total = got["shift_cells"][0] + got["subcell"][0]        # b's cell c meets a's index c + total: the truth is -1/2
    print("half-cell displacement: shift %s subcell %s, sx + dx = %.4f (truth -0.5), dz %.4f, std %.3f" % (got["shift_cells"], got["subcell"], total, got["dz"], got["std"]))
    assert got["shift_cells"] in ((0, 0), (-1, 0)) and 0.25 <= abs(got["subcell"][0]) <= 0.5 and abs(total + 0.5) <= 0.25


def test_compare_dsms_and_changes(dev):
    from satmvs_amd import dsm
    scene = cs.DISPLACED[0]
    a, ga, b, gb = cs.displaced(*scene)
    ga, gb = _grid(ga), _grid(gb)
    res = dsm.compare_dsms(a, ga, b, gb, radius=scene[3])
    print("compare_dsms: before rmse %.3f, after rmse %.3f, shift %s" % (res["before"]["rmse"], res["after"]["rmse"], res["shift"]["shift_cells"]))
    assert res["shift"]["shift_cells"] == scene[4:6] and res["after"]["rmse"] < res["before"]["rmse"]
    by_hand = dsm.regrid(a, res["shift"]["grid"], gb, dz=-res["shift"]["dz"])
    assert res["after"] == dsm.dsm_metrics(by_hand, b, -999.0)
    assert res["before"] == dsm.dsm_metrics(dsm.regrid(a, ga, gb), b, -999.0)
    plain = dsm.compare_dsms(a, ga, b, gb, register=False)
    assert plain["shift"] is None and plain["after"] == plain["before"] == res["before"]
    fine = dsm.DSMGrid(ga.e0, ga.n0, 2.5, 2.5, 2 * ga.width - 1, 2 * ga.height - 1)      # est at another resolution
    res2 = dsm.compare_dsms(dsm.regrid(a, ga, fine), fine, b, gb, radius=scene[3])
    assert res2["shift"]["shift_cells"] == scene[4:6] and res2["after"]["rmse"] < res2["before"]["rmse"]
    # changes: a block of 6 x 5 cells, 12 m high, added to the displaced epoch
    new = a.copy()
    r0, c0 = 20 + 1 + scene[5], 30 + 1 + scene[4]
    new[r0:r0 + 6, c0:c0 + 5] = np.where(np.isfinite(new[r0:r0 + 6, c0:c0 + 5]) & (new[r0:r0 + 6, c0:c0 + 5] != ND), new[r0:r0 + 6, c0:c0 + 5] + np.float32(12.0), new[r0:r0 + 6, c0:c0 + 5])
    diff, labels, stats = dsm.changes(new, ga, b, gb, min_dh=6.0, min_area_m2=250.0, radius=scene[3])
    assert isinstance(diff, np.ndarray) and diff.shape == b.shape and labels.dtype == np.int32
    assert stats["sign"].tolist() == [1] and labels.max() == 1               # one rise, nothing else above the sieve
    rr, cc = np.nonzero(labels)
    # the registered epoch is resampled bilinearly at the sub-cell shift, which spreads an edge by at most one cell
    assert rr.min() >= 19 and rr.max() <= 26 and cc.min() >= 29 and cc.max() <= 35 and stats["area"][0] >= 20


def test_no_overlap_and_unequal_resolution(dev):
    from satmvs_amd import dsm
    a, ga, b, gb = cs.displaced(*cs.DISPLACED[3])
    ga, gb = _grid(ga), _grid(gb)
    far = dsm.DSMGrid(gb.e0 + 10000.0, gb.n0, gb.xres, gb.yres, gb.width, gb.height)
    with pytest.raises(ValueError, match="no overlap"):
        dsm.coregister(a, ga, b, far)
    empty = np.full_like(b, ND)
    with pytest.raises(ValueError, match="no overlap"):
        dsm.coregister(a, ga, empty, gb)
    with pytest.raises(ValueError, match="regrid"):
        dsm.coregister(a, ga, b, dsm.DSMGrid(gb.e0, gb.n0, 2.5, gb.yres, gb.width, gb.height))
