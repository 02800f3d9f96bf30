"""The outline oracle (tests/dsm_outline_oracle.py) without a device: its two statements against each other, the invariants the
rule promises against independent counts (cell counts, holes as 4-connected components of the complement, scipy.ndimage where
it is installed), the closed-form scenes, the even-odd fill, the GeoJSON round trip, the five planted errors the GPU file's
comparison must report, and every argument rejection of dsm.outlines, dsm.burn_rings and dsm.write_geojson on host arrays and
of the three C entries on made-up pointers."""
import ctypes as C
import json

import numpy as np
import pytest

import dsm_label_oracle as lo
import dsm_outline_oracle as oo
from dsm_testkit import lib  # noqa: F401  (fixture)

SHAPES = [(1, 1), (1, 9), (7, 1), (3, 4), (17, 23), (64, 65)]
DENSITIES = (0.3, 0.45, 0.593, 0.8, 0.95)


class Grid:                                                  # what the oracle reads of a DSMGrid
    def __init__(self, gh, gw, e0=500000.0, n0=3400000.0, xres=5.0, yres=2.5):
        self.e0, self.n0, self.xres, self.yres, self.width, self.height = e0, n0, xres, yres, gw, gh


def _cases():
    for shape in SHAPES:
        for density in DENSITIES:
            for conn in (4, 8):
                labels, n = lo.label(lo.random_mask(*shape, density, seed=int(100 * density) + shape[0]), conn)
                yield shape, density, conn, labels, n


def _ring(rings, r):
    return rings["vertices"][rings["offset"][r]:rings["offset"][r + 1]]


# ---- the two statements, and what the rule promises ----------------------------------------------------------------------------
def test_the_two_statements_agree():
    for shape, density, conn, labels, n in _cases():
        oo.same_rings(oo.trace_corners(labels, n), oo.trace(labels, n), (shape, density, conn))
    mixed = np.random.default_rng(5).integers(-1, 6, (23, 31)).astype(np.int32)        # any label map: labels in several pieces
    for n in (0, 1, 3, 4, 9):
        oo.same_rings(oo.trace_corners(mixed, n), oo.trace(mixed, n), ("mixed", n))


def test_invariants():
    for shape, density, conn, labels, n in _cases():
        what = (shape, density, conn)
        rings = oo.trace(labels, n)
        first, area2 = rings["first_ring"], rings["area2"]
        assert rings["label"].tolist() == sorted(rings["label"].tolist()) and first[-1] == len(area2), what
        cells = np.bincount(labels.reshape(-1), minlength=n + 1)[1:]
        for k in range(n):
            mine = slice(first[k], first[k + 1])
            assert first[k + 1] > first[k] and area2[first[k]] > 0 and (area2[mine][1:] < 0).all(), (what, k)      # one exterior ring
            assert area2[mine].sum() == 2 * cells[k], (what, k)
            if shape[0] * shape[1] <= 17 * 23:               # holes = 4-connected components of the padded complement, minus one
                outside = np.pad(labels != k + 1, 1, constant_values=True)
                assert first[k + 1] - first[k] - 1 == lo.label(outside, 4)[1] - 1, (what, k)
        assert np.array_equal(oo.fill(rings["vertices"], rings["offset"], rings["label"], labels.shape), labels), what
        for r in range(len(area2)):
            v = _ring(rings, r)
            assert len(v) >= 4 and len(v) % 2 == 0 and (v[0] == v[np.lexsort((v[:, 0], v[:, 1]))[0]]).all(), (what, r)
            step = np.roll(v, -1, axis=0) - v
            assert ((step != 0).sum(axis=1) == 1).all(), (what, r)                       # along the lattice
            turn = step[:, 0] * np.roll(step, -1, axis=0)[:, 1] - step[:, 1] * np.roll(step, -1, axis=0)[:, 0]
            assert (turn != 0).all(), (what, r)                                          # no collinear point, no reversal
            assert (step[0] > 0).tolist() == ([False, True] if area2[r] > 0 else [True, False]), (what, r)    # leaves south / east
            assert (v.tolist().count(v[0].tolist()) == 1), (what, r)                     # the start corner is passed once
            assert np.abs(step).sum(axis=0).tolist() == rings["edges"][r].tolist(), (what, r)
            if conn == 4:
                assert len(np.unique(v, axis=0)) == len(v), (what, r)                    # simple


def test_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    eight = np.ones((3, 3), int)
    for shape, density, conn, labels, n in _cases():
        want_labels, want_n = ndi.label(labels != 0, structure=eight if conn == 8 else None)
        assert want_n == n and np.array_equal(want_labels, labels)
        rings = oo.trace(labels, n)
        area = ndi.sum(labels != 0, labels, np.arange(1, n + 1)) if n else np.zeros(0)
        assert np.array_equal(np.add.reduceat(rings["area2"], rings["first_ring"][:-1]) if n else np.zeros(0), 2 * np.asarray(area, np.int64))
        for k in range(n):
            holes = ndi.label(np.pad(labels != k + 1, 1, constant_values=True))[1] - 1
            assert rings["first_ring"][k + 1] - rings["first_ring"][k] - 1 == holes


@pytest.mark.parametrize("case", oo.closed_forms(), ids=lambda c: c[0])
def test_closed_forms(case):
    name, labels, n, want = case
    oo.same_rings(oo.trace(labels, n), want, name)
    oo.same_rings(oo.trace_corners(labels, n), want, name)
    assert np.array_equal(oo.fill(want["vertices"], want["offset"], want["label"], labels.shape), labels)
    assert want["area2"].sum() == 2 * (labels != 0).sum()
    if name == "island in a hole joined by a corner":        # the self-touching hole: corner (2, 2) twice
        assert _ring(want, 1).tolist().count([2, 2]) == 2 and want["area2"].tolist() == [50, -14]
    if name == "two cells at a corner, connectivity 8":
        assert _ring(want, 0).tolist().count([1, 1]) == 2


def test_serpentine_closed_form():
    """The formula the GPU file's 2300 x 2300 case uses, where the walk is cheap."""
    for g in (4, 12, 18):
        r, c = np.mgrid[0:g, 0:g]
        labels = oo.serpentine(g, r, c).astype(np.int32)
        assert lo.label(labels, 4)[1] == 1
        want = oo.trace(labels, 1)
        assert len(want["label"]) == 1 and len(want["vertices"]) == 4 * (g // 2) and want["area2"][0] == 2 * labels.sum()
        assert want["vertices"][0].tolist() == [0, 0] and want["vertices"][-1].tolist() == [1, 0]


def test_with_grid_entries():
    labels = np.array([[1, 1, 1, 0], [1, 0, 1, 2], [1, 1, 1, 2]], np.int32)
    got = oo.with_grid(oo.trace(labels, 3), Grid(3, 4, 100.0, 50.0, 2.0, 0.5), 3)
    assert got["perimeter_m"].tolist() == [6 * 2.0 + 6 * 0.5, 2 * 2.0 + 2 * 0.5, 2 * 2.0 + 4 * 0.5]
    assert got["label_perimeter_m"].tolist() == [8 * 2.0 + 8 * 0.5, 2 * 2.0 + 4 * 0.5, 0.0] and got["n_holes"].tolist() == [1, 0, 0]
    assert got["vertices_en"][0].tolist() == [99.0, 50.25] and got["vertices_en"].dtype == np.float64     # corner (0, 0): half a cell up and left


# ---- the comparison reports the planted errors ---------------------------------------------------------------------------------
@pytest.mark.parametrize("plant", oo.PLANTED)
def test_planted_errors_are_reported(plant):
    labels, n = lo.label(lo.random_mask(64, 65, 0.593, seed=3), 8)
    want = oo.trace(labels, n)
    assert oo.difference(want, oo.trace(labels, n)) is None
    message = oo.difference(oo.trace(labels, n, plant=plant), want)
    assert message is not None and message.startswith("ring "), (plant, message)
    with pytest.raises(AssertionError):
        oo.same_rings(oo.trace(labels, n, plant=plant), want, plant)


def test_difference_reports_table_damage():
    labels, n = lo.label(lo.random_mask(20, 21, 0.5, seed=2), 4)
    want = oo.trace(labels, n)
    for key in oo.KEYS:
        bad = {k: v.copy() for k, v in want.items()}
        bad[key].reshape(-1)[-1] += 1
        assert oo.difference(bad, want) is not None, key
        bad[key] = want[key].astype(np.float64)
        assert "dtype" in oo.difference(bad, want)
    assert "missing" in oo.difference({k: v for k, v in want.items() if k != "offset"}, want)
    short = {k: (v[:-1] if k in ("label", "area2", "edges", "offset") else v) for k, v in want.items()}
    assert oo.difference(short, want) is not None


# ---- the fill ------------------------------------------------------------------------------------------------------------------
def test_fill_cases():
    i32 = lambda a: np.array(a, np.int32)                    # noqa: E731
    sq = i32([(1, 1), (1, 3), (4, 3), (4, 1)])
    want = np.zeros((4, 5), np.int32)
    want[1:3, 1:4] = 7
    assert np.array_equal(oo.fill(sq, i32([0, 4]), i32([7]), (4, 5)), want)
    assert np.array_equal(oo.fill(sq[::-1], i32([0, 4]), i32([7]), (4, 5)), want)
    assert not oo.fill(np.concatenate([sq, sq]), i32([0, 4, 8]), i32([7, 7]), (4, 5)).any()          # twice: nothing
    off_grid = oo.fill(sq - 2, i32([0, 4]), i32([7]), (4, 5))                                         # x < 0 clamps to column 0
    assert off_grid[0, :2].tolist() == [7, 7] and off_grid.sum() == 14
    assert not oo.fill(sq + 10, i32([0, 4]), i32([7]), (4, 5)).any()
    with pytest.raises(ValueError):
        oo.fill(i32([(0, 0), (0, 2), (2, 1)]), i32([0, 3]), i32([1]), (4, 4))


# ---- GeoJSON -------------------------------------------------------------------------------------------------------------------
def test_geojson_round_trip(tmp_path):
    from satmvs_amd import dsm
    labels = np.array([[1, 1, 1, 0, 0], [1, 0, 1, 0, 3], [1, 1, 1, 0, 3], [0, 0, 0, 0, 0]], np.int32)      # label 2 has no cell
    n = 3
    grid = dsm.DSMGrid(500000.0, 3400000.0, 5.0, 2.5, 5, 4)
    rings = oo.with_grid(oo.trace(labels, n), grid, n)
    stats = lo.stats(labels, n, values=np.where(labels > 0, np.float32(4.0), np.float32(np.nan)).astype(np.float32), grid=Grid(4, 5))
    path = str(tmp_path / "rings.geojson")
    assert dsm.write_geojson(path, rings, grid, stats) == 2
    features = oo.read_geojson(path)
    assert [f[0]["label"] for f in features] == [1, 3] and [len(f[1]) for f in features] == [2, 1]
    for prop, polygon in features:
        k = prop["label"] - 1
        assert oo.shoelace2(polygon[0]) > 0 and all(oo.shoelace2(h) < 0 for h in polygon[1:])          # RFC 7946 winding, east / north
        assert sum(oo.shoelace2(ring) for ring in polygon) / 2.0 == stats["area_m2"][k] == prop["area_m2"]
        assert prop["area"] == stats["area"][k] and prop["bbox"] == stats["bbox"][k].tolist() and prop["centroid"] == stats["centroid"][k].tolist()
        assert prop["mean"] == 4.0 and isinstance(prop["area"], int) and isinstance(prop["volume"], float)
        for r, ring in zip(range(rings["first_ring"][k], rings["first_ring"][k + 1]), polygon):
            assert np.array_equal(ring[:-1], rings["vertices_en"][rings["offset"][r]:rings["offset"][r + 1]])
    assert features[0][1][0][0].tolist() == [500000.0 - 2.5, 3400000.0 + 1.25]
    assert dsm.write_geojson(path, {k: rings[k] for k in oo.KEYS}, grid) == 2 and [sorted(f[0]) for f in oo.read_geojson(path)] == [["label"]] * 2
    nan_stats = {"mean": np.array([np.nan, 1.0, np.inf])}
    dsm.write_geojson(path, rings, grid, nan_stats)
    with open(path) as f:
        text = f.read()
    assert "NaN" not in text and "Infinity" not in text and json.loads(text)["features"][0]["properties"]["mean"] is None
    empty = oo.trace(np.zeros((4, 5), np.int32), 2)
    assert dsm.write_geojson(path, empty, grid) == 0 and oo.read_geojson(path) == []
    with pytest.raises(ValueError, match="one entry per label"):
        dsm.write_geojson(path, rings, grid, {"area": np.zeros(2)})
    with pytest.raises(ValueError, match="one entry per label"):
        dsm.write_geojson(path, rings, grid, {"cube": np.zeros((3, 2, 2))})
    with pytest.raises(ValueError, match="dict of outlines"):
        dsm.write_geojson(path, dict(rings, offset=rings["offset"][:-1]), grid)
    with pytest.raises(ValueError, match="resolutions"):
        dsm.write_geojson(path, rings, dsm.DSMGrid(0.0, 0.0, 0.0, 1.0, 5, 4))


# ---- argument rejections, Python ------------------------------------------------------------------------------------------------
def test_outlines_rejects_bad_arguments_without_a_gpu():
    from satmvs_amd import dsm
    good = np.zeros((4, 5), np.int32)
    for labels, match in ((np.zeros((4, 5), np.int64), "int32"), (np.zeros((4, 5), np.float32), "int32"), (np.zeros(5, np.int32), "gh, gw"),
                          (np.zeros((2, 4, 5), np.int32), "gh, gw"), (np.zeros((0, 5), np.int32), "positive sizes"),
                          (np.broadcast_to(np.int32(0), (2 ** 15, 2 ** 14)), "2\\^29")):
        with pytest.raises(ValueError, match=match):
            dsm.outlines(labels, 1)
    for n in (-1, 1.0, True, None, 2 ** 31, "3"):
        with pytest.raises(ValueError, match="n must be"):
            dsm.outlines(good, n)
    with pytest.raises(ValueError, match="differs from the grid"):
        dsm.outlines(good, 1, dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, 4, 5))


def test_burn_rings_rejects_bad_arguments_without_a_gpu():
    import torch
    from satmvs_amd import dsm
    v, off, lab = np.zeros((4, 2), np.int32), np.array([0, 4], np.int32), np.ones(1, np.int32)
    bad = [((v.astype(np.int64), off, lab, (4, 4)), "vertices is int32"), ((v.reshape(-1), off, lab, (4, 4)), "vertices has 2 axes"),
           ((np.zeros((4, 3), np.int32), off, lab, (4, 4)), "x, y"), ((v, off.astype(np.int64), lab, (4, 4)), "offset is int32"),
           ((v, off, lab.astype(np.float32), (4, 4)), "ring_label is int32"), ((v, off[None], lab, (4, 4)), "offset has 1 axes"),
           ((v, np.array([0, 2, 4], np.int32), lab, (4, 4)), "n_rings \\+ 1"), ((v, off, np.ones((1, 1), np.int32), (4, 4)), "ring_label has 1 axes"),
           ((v, torch.from_numpy(off), lab, (4, 4)), "both be numpy"), ((torch.from_numpy(v), off, lab, (4, 4)), "both be numpy"),
           ((v, off, lab, (4,)), "pair of integers"), ((v, off, lab, (4.0, 4)), "pair of integers"), ((v, off, lab, (0, 4)), "positive sizes"),
           ((v, off, lab, (2 ** 16, 2 ** 15)), "2\\^31"), ((v, np.array([1, 4], np.int32), lab, (4, 4)), "rise from 0"),
           ((v, np.array([0, 3], np.int32), lab, (4, 4)), "rise from 0"),
           ((v, np.array([0, 3, 2, 4], np.int32), np.ones(3, np.int32), (4, 4)), "rise from 0")]
    for args, match in bad:
        with pytest.raises(ValueError, match=match):
            dsm.burn_rings(*args)


# ---- argument rejections, C ------------------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_a_gpu(lib):
    from satmvs_amd import _lib
    MB = 1 << 20
    at = lambda i: C.c_void_p(i * MB)                        # noqa: E731  (made-up pointers a megabyte apart: nothing is dereferenced)
    gw, gh, n = 9, 7, 3
    need0, need = lib.smvs_dsm_outline_workspace_bytes(gw, gh, 0), lib.smvs_dsm_outline_workspace_bytes(gw, gh, 32)
    assert need > need0 >= 5 * (gw + 1) * (gh + 1) and need - need0 >= 61 * 32 and need < MB
    assert lib.smvs_dsm_outline_workspace_bytes(0, 5, 0) == 0 and lib.smvs_dsm_outline_workspace_bytes(5, -1, 0) == 0
    assert lib.smvs_dsm_outline_workspace_bytes(5, 5, -1) == 0 and lib.smvs_dsm_outline_workspace_bytes(5, 5, 101) == 0
    assert lib.smvs_dsm_outline_workspace_bytes(2 ** 15, 2 ** 14, 0) == 0 and lib.smvs_dsm_outline_workspace_bytes(2 ** 15 - 1, 2 ** 14, 0) > 0

    def count(labels=at(1), gw=gw, gh=gh, n=n, max_edges=32, counts=at(2), ws=at(3), nbytes=need):
        _lib.call("smvs_dsm_outline_count", labels, gw, gh, n, max_edges, counts, ws, nbytes, None)

    def write(labels=at(1), gw=gw, gh=gh, n=n, ne=32, nr=2, nv=8, label=at(4), area2=at(5), edges=at(6), offset=at(7), first=at(8),
              vertices=at(9), ws=at(3), nbytes=need):
        _lib.call("smvs_dsm_outline_write", labels, gw, gh, n, ne, nr, nv, label, area2, edges, offset, first, vertices, ws, nbytes, None)

    def burn(vertices=at(1), offset=at(2), label=at(3), nr=2, nv=8, gw=gw, gh=gh, out=at(4), flag=at(5)):
        _lib.call("smvs_dsm_burn", vertices, offset, label, nr, nv, gw, gh, out, flag, None)

    bad = [(count, dict(labels=None), "null pointer"), (count, dict(counts=None), "null pointer"), (count, dict(ws=None), "null pointer"),
           (count, dict(gw=0), "non-positive grid"), (count, dict(gh=-2), "non-positive grid"), (count, dict(gw=2 ** 15, gh=2 ** 14), "below 2\\^29"),
           (count, dict(n=-1), "n must be"), (count, dict(max_edges=-1), "max_edges"), (count, dict(max_edges=4 * gw * gh + 1), "max_edges"),
           (count, dict(nbytes=need - 1), "workspace too small"), (count, dict(counts=at(1)), "counts aliases labels"),
           (count, dict(ws=at(1)), "workspace aliases labels"), (count, dict(ws=at(2)), "workspace aliases counts"),
           (write, dict(labels=None), "null pointer"), (write, dict(offset=None), "null pointer"), (write, dict(first=None), "null pointer"),
           (write, dict(ws=None), "null pointer"), (write, dict(label=None), "null pointer"), (write, dict(area2=None), "null pointer"),
           (write, dict(edges=None), "null pointer"), (write, dict(vertices=None), "null pointer"), (write, dict(gw=-1), "non-positive grid"),
           (write, dict(gw=2 ** 15, gh=2 ** 14), "below 2\\^29"), (write, dict(n=-1), "n must be"), (write, dict(n=0), "without labels"),
           (write, dict(ne=-1), "max_edges"), (write, dict(ne=4 * gw * gh + 1), "max_edges"), (write, dict(nr=0), "n_rings"),
           (write, dict(nr=33), "n_rings"), (write, dict(nr=-1), "n_rings"), (write, dict(nv=0), "n_rings"), (write, dict(nv=33), "n_rings"),
           (write, dict(ne=0), "n_rings"), (write, dict(nbytes=need - 1), "workspace too small"), (write, dict(label=at(1)), "ring_label aliases labels"),
           (write, dict(offset=at(4)), "offset aliases ring_label"), (write, dict(vertices=at(3)), "vertices aliases workspace"),
           (write, dict(first=at(5)), "first_ring aliases area2"), (write, dict(edges=at(1)), "edges aliases labels"),
           (write, dict(area2=at(3)), "area2 aliases workspace"),
           (burn, dict(out=None), "null pointer"), (burn, dict(flag=None), "null pointer"), (burn, dict(vertices=None), "null pointer"),
           (burn, dict(offset=None), "null pointer"), (burn, dict(label=None), "null pointer"), (burn, dict(nr=-1), "must be >= 0"),
           (burn, dict(nv=-1), "must be >= 0"), (burn, dict(gw=0), "non-positive grid"), (burn, dict(gw=2 ** 16, gh=2 ** 15), "grid too large"),
           (burn, dict(flag=at(4)), "flag aliases out"), (burn, dict(out=at(1)), "out aliases vertices"), (burn, dict(out=at(2)), "out aliases offset"),
           (burn, dict(out=at(3)), "out aliases ring_label"), (burn, dict(flag=at(1)), "flag aliases vertices")]
    for fn, kw, match in bad:
        with pytest.raises(_lib.SatMVSNativeError, match=match):
            fn(**kw)
