"""The simplification oracle (tests/dsm_simplify_oracle.py) without a device: its two statements against each other on the
outlines of random masks (scipy.ndimage.label where it is installed, the label oracle otherwise, both connectivities), the
closed forms, the Hausdorff property in exact fractions, the identity at tolerance 0, the fill against the lattice fill of the
outline oracle, the planted errors the GPU file's comparisons must report, and every argument rejection of
dsm.simplify_outlines and dsm.burn_polygons on host arrays and of the C entries on made-up pointers."""
import ctypes as C
import math

import numpy as np
import pytest

import dsm_label_oracle as lo
import dsm_outline_oracle as oo
import dsm_simplify_oracle as so
from dsm_testkit import lib  # noqa: F401  (fixture)

TOL16 = (0, 1, 11, 12, 16, 40, 65535)
SHAPES = [(1, 1), (1, 9), (7, 1), (17, 23), (48, 51)]


def _label(mask, conn):
    try:
        import scipy.ndimage as ndi
    except ImportError:
        return lo.label(mask, conn)
    labels, n = ndi.label(mask, structure=np.ones((3, 3), int) if conn == 8 else None)
    return labels.astype(np.int32), int(n)


def _cases():
    for shape in SHAPES:
        for density in (0.3, 0.593, 0.95):
            for conn in (4, 8):
                labels, n = _label(lo.random_mask(*shape, density, seed=int(100 * density) + shape[1]), conn)
                yield (shape, density, conn), oo.trace(labels, n)


CASES = list(_cases())


def _one(ring, label=1):
    return so.table(label, (label, ring))


# ---- the two statements ----------------------------------------------------------------------------------------------------------
def test_the_two_statements_agree():
    for what, rings in CASES:
        for tol16 in TOL16:
            a, b = so.simplify(rings, tol16), so.simplify_rounds(rings, tol16)
            so.same(a, b, (what, tol16))
            assert b["rounds"] >= 1 or not len(rings["vertices"])
            assert np.array_equal(a["label"], rings["label"]) and np.array_equal(a["first_ring"], rings["first_ring"])
            assert np.array_equal(a["vertices"], rings["vertices"][a["kept"]]) and (np.diff(a["kept"]) > 0).all()
            assert (a["kept"][a["offset"][:-1]] == rings["offset"][:-1]).all()           # every ring still starts at its first vertex
            assert (np.sign(a["area2"]) == np.sign(rings["area2"])).all()
            same = np.diff(a["offset"]) == np.diff(rings["offset"])
            assert (a["area2"][same] == rings["area2"][same]).all()


def test_hausdorff_property():
    """Every vertex of the ring as given lies within tol16 / 16 of the segment between its kept neighbours: exact."""
    for what, rings in CASES:
        for tol16 in TOL16:
            assert so.hausdorff_holds(rings, so.simplify_rounds(rings, tol16), tol16), (what, tol16)
    # not a matter of course: (3, 0) is 0.27 from the line through (5, 4) and (7, 11) and 4.5 from the segment between them
    ring = _one([(5, 4), (3, 0), (7, 11), (11, 4), (9, 8), (3, 7), (2, 10)])
    loose = so.simplify(ring, 16, plant="line")
    assert loose["kept"].tolist() == [0, 2, 3, 4, 5, 6] and not so.hausdorff_holds(ring, loose, 16)
    assert so.simplify(ring, 16)["kept"].tolist() == list(range(7)) and so.hausdorff_holds(ring, so.simplify(ring, 16), 16)


def test_identity_at_tolerance_zero():
    for what, rings in CASES:
        got = so.simplify_rounds(rings, 0)
        for key in ("offset", "vertices", "area2"):
            assert np.array_equal(got[key], rings[key]), (what, key)
        assert np.array_equal(got["kept"], np.arange(len(rings["vertices"]))) and got["simplified"].all(), what


# ---- closed forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(3, 4), (1, 1), (40, 9), (5, 12), (300, 1)])
def test_rectangle(w, h):
    rings = _one(so.rectangle(w, h, 2, 3))
    t = so.rectangle_threshold16(w, h)
    assert (t - 1) / 16.0 < w * h / math.hypot(w, h) <= t / 16.0 + 1e-12
    for statement in (so.simplify, so.simplify_rounds):
        below, at = statement(rings, t - 1), statement(rings, t)
        assert np.array_equal(below["vertices"], rings["vertices"]) and below["simplified"].tolist() == [1]
        assert np.array_equal(at["vertices"], rings["vertices"]) and at["simplified"].tolist() == [0]      # falls back: unchanged too
        assert below["area2"].tolist() == at["area2"].tolist() == [2 * w * h]
    if (w, h) == (3, 4):
        assert t == 39                                       # 12 / 5 = 2.4 cells = 38.4 sixteenths


@pytest.mark.parametrize("g", [1, 2, 3, 9, 33, 130])
def test_digitised_triangle(g):
    rings = oo.trace(so.triangle_mask(g), 1)
    assert so.ring_lists(rings)[0] == so.staircase(g)
    for statement in (so.simplify, so.simplify_rounds):
        got = statement(rings, 16)
        if g == 1:
            assert got["simplified"].tolist() == [0] and len(got["vertices"]) == 4
        else:
            assert got["vertices"].tolist() == [[0, 0], [1, g], [g, 0]] and got["simplified"].tolist() == [1], g
            assert got["area2"].tolist() == [g * g]


def test_notch():
    rings = _one(so.notch(9, 5, 4))
    for statement in (so.simplify, so.simplify_rounds):
        gone, kept = statement(rings, 16), statement(rings, 15)
        assert gone["vertices"].tolist() == [[0, 0], [0, 5], [9, 5], [9, 0]] and gone["area2"].tolist() == [90]
        # at 15 / 16 the notch stays, as the dent (5, 0), (5, 1): (5, 1) is 1 from (9, 0) - (0, 0), (5, 0) 4 / sqrt 17 = 0.97 from
        # (9, 0) - (5, 1), and (4, 1), (4, 0) are 1 / sqrt 26 and 4 / sqrt 26 from (5, 1) - (0, 0)
        assert kept["vertices"].tolist() == [[0, 0], [0, 5], [9, 5], [9, 0], [5, 0], [5, 1]] and kept["area2"].tolist() == [85]
        assert gone["simplified"].tolist() == kept["simplified"].tolist() == [1]


def test_ring_that_touches_itself():
    """Connectivity 8 joins two cells at a corner in one ring that passes the corner twice; the anchor is the far corner (2, 2),
    and when (1, 1) has been kept on both sides the segments (1, 1) .. (1, 1) have L = 0."""
    rings = oo.trace(np.array([[1, 0], [0, 1]], np.int32), 1)
    assert so.ring_lists(rings)[0] == so.TOUCHING
    for statement in (so.simplify, so.simplify_rounds):
        assert np.array_equal(statement(rings, 7)["vertices"], rings["vertices"])        # (1, 1) is 1 / sqrt 5 = 7.16 sixteenths from (0, 1) - (2, 2)
        got = statement(rings, 11)                           # (0, 1) and (2, 1) are 1 / sqrt 2 = 11.3 sixteenths from the diagonal
        assert got["vertices"].tolist() == [[0, 0], [0, 1], [2, 2], [2, 1]] and got["area2"].tolist() == [4] and got["simplified"].tolist() == [1]
        got = statement(rings, 12)
        assert got["simplified"].tolist() == [0] and np.array_equal(got["vertices"], rings["vertices"])    # (0, 0) (2, 2): no area
    spike = _one([(0, 0), (0, 6), (3, 6), (3, 9), (3, 6), (6, 6), (6, 0)])               # out and back along one edge
    sizes = []
    so.simplify_ring_rounds(so.ring_lists(spike)[0], 16, sizes)
    assert sizes == [2, 3, 1, 2, 1]                          # the third: (3, 9) between (3, 6) and (3, 6), L = 0, key 9 > 1
    for tol16, want in ((16, spike["vertices"].tolist()), (47, [[0, 0], [3, 9], [6, 0]]), (48, [[0, 0], [3, 9], [6, 0]]), (100, spike["vertices"].tolist())):
        a, b = so.simplify(spike, tol16), so.simplify_rounds(spike, tol16)
        so.same(a, b, ("spike", tol16))
        assert a["vertices"].tolist() == want and a["simplified"].tolist() == [int(tol16 < 100)]


def test_short_and_degenerate_rings():
    rings = so.table(6, (1, []), (2, [(3, 3)]), (3, [(1, 1), (4, 5)]), (4, [(0, 0), (0, 3), (3, 0)]), (5, [(2, 2)] * 5),
                     (6, so.rectangle(3, 3)), (6, so.rectangle(3, 3)))
    for tol16 in (0, 16, 65535):
        a, b = so.simplify(rings, tol16), so.simplify_rounds(rings, tol16)
        so.same(a, b, tol16)
        assert np.array_equal(a["vertices"], rings["vertices"]) and a["offset"].tolist() == rings["offset"].tolist()
        assert a["simplified"].tolist() == [0, 0, 0] + ([1, 0, 1, 1] if tol16 < 34 else [0, 0, 0, 0]), tol16
        assert a["area2"].tolist() == [0, 0, 0, 9, 0, 18, 18]
    empty = so.table(2)
    got = so.simplify_rounds(empty, 16)
    assert got["rounds"] == 0 and got["offset"].tolist() == [0] and got["vertices"].shape == (0, 2) and got["kept"].shape == (0,)


# ---- the fill -------------------------------------------------------------------------------------------------------------------
def test_fill_on_lattice_rings_is_the_lattice_fill():
    for what, rings in CASES:
        shape = what[0]
        want = oo.fill(rings["vertices"], rings["offset"], rings["label"], shape)
        assert np.array_equal(so.fill(rings["vertices"], rings["offset"], rings["label"], shape), want), what
    sq = np.array([(1, 1), (1, 3), (4, 3), (4, 1)], np.int32)
    one, off = np.array([7], np.int32), np.array([0, 4], np.int32)
    for shift in (0, -2, 10):
        assert np.array_equal(so.fill(sq + shift, off, one, (4, 5)), oo.fill(sq + shift, off, one, (4, 5)))


def test_fill_cases():
    i32 = lambda a: np.array(a, np.int32)                    # noqa: E731
    tri = i32([(0, 0), (0, 4), (4, 0)])                      # x + y < 4: the centres on the diagonal, c + r = 3, are not strictly right of it: in
    got = so.fill(tri, i32([0, 3]), i32([5]), (4, 4))
    r, c = np.mgrid[0:4, 0:4]
    assert np.array_equal(got, np.where(r + c < 4, 5, 0))
    # Two triangles that share an edge through cell centres.  With integer ends an edge of slope 2 : 1 cannot pass a centre
    # (2 c + 1 - 2 x0 = r + 1/2 - y0 has no solution); slopes 1 : 1 and 3 : 1 do: (0, 0) - (2, 6) passes the centres of
    # cells (1, 0) and (4, 1), (0, 0) - (4, 4) those of the diagonal.
    for (ex, ey), on_edge in (((2, 6), [(1, 0), (4, 1)]), ((4, 4), [(k, k) for k in range(4)])):
        left, right = [(0, 0), (0, ey), (ex, ey)], [(0, 0), (ex, ey), (ex, 0)]
        both = so.fill(i32(left + right), i32([0, 3, 6]), i32([1, 2]), (ey, ex))
        assert (both > 0).all() and (both < 3).all()         # every cell in exactly one of them: in both would give 3, in neither 0
        assert all(both[r, c] == 1 for r, c in on_edge)      # on the edge: not strictly right of it, so with the polygon on its left
        assert (both == 1).sum() == (ex * ey + len(on_edge)) // 2
    off_grid = so.fill(i32([(-5, -3), (2, 9), (9, -4)]), i32([0, 3]), i32([3]), (5, 6))
    assert off_grid[0, 0] == 3 and off_grid.any() and (off_grid[:, -1] == 3).any()
    assert not so.fill(i32(left + left), i32([0, 3, 6]), i32([1, 1]), (8, 4)).any()      # a ring given twice cancels
    assert not np.array_equal(so.fill(tri, i32([0, 3]), i32([5]), (4, 4), plant="rint"), got)          # halves to even: not the rule


# ---- planted errors -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plant", so.PLANTED)
def test_planted_errors_are_reported(plant):
    labels, n = lo.label(lo.random_mask(64, 65, 0.593, seed=3), 8)
    rings = oo.trace(labels, n)
    want = so.simplify_rounds(rings, 16)
    assert so.difference(so.simplify(rings, 16), want) is None
    message = so.difference(so.simplify(rings, 16, plant=plant), want)
    assert message is not None and message.startswith("ring "), (plant, message)
    with pytest.raises(AssertionError):
        so.same(so.simplify(rings, 16, plant=plant), want, plant)


def test_difference_reports_table_damage():
    rings = CASES[-1][1]
    want = so.simplify_rounds(rings, 12)
    for key in so.KEYS:
        bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in want.items()}
        bad[key].reshape(-1)[-1] += 1
        assert so.difference(bad, want) is not None, key
        bad[key] = want[key].astype(np.float64)
        assert "dtype" in so.difference(bad, want)
    assert "missing" in so.difference({k: v for k, v in want.items() if k != "kept"}, want)
    assert "edges" in so.difference(dict(want, edges=np.zeros((1, 2), np.int32)), want)


def test_with_grid_entries():
    class Grid:
        e0, n0, xres, yres = 100.0, 50.0, 3.0, 4.0
    got = so.with_grid(so.simplify_rounds(so.table(2, (1, [(0, 0), (0, 2), (1, 0)]), (1, [(5, 5), (6, 5), (6, 6)]), (2, so.rectangle(2, 1))), 0), Grid)
    assert got["perimeter_m"].tolist() == [8.0 + math.sqrt(9.0 + 64.0) + 3.0, 5.0 + 4.0 + 3.0, 12.0 + 8.0]
    assert got["n_holes"].tolist() == [1, 0] and got["vertices_en"][0].tolist() == [98.5, 52.0]


# ---- argument rejections, Python ------------------------------------------------------------------------------------------------
def test_simplify_outlines_rejects_bad_arguments_without_a_gpu():
    import torch
    from satmvs_amd import dsm
    good = so.table(1, (1, so.rectangle(3, 4)))
    for tol in (-1, float("nan"), float("inf"), "1", None, True, 4096):
        with pytest.raises(ValueError, match="tol "):
            dsm.simplify_outlines(good, tol)
    bad = [(dict(good, vertices=good["vertices"].astype(np.int64)), "vertices is int32"), (dict(good, vertices=good["vertices"].reshape(-1)), "vertices has 2 axes"),
           (dict(good, vertices=np.zeros((4, 3), np.int32)), "x, y"), (dict(good, offset=good["offset"].astype(np.int64)), "offset is int32"),
           (dict(good, offset=np.array([0, 2, 4], np.int32)), "n_rings \\+ 1"), (dict(good, label=good["label"].astype(np.float32)), "ring_label is int32"),
           (dict(good, first_ring=good["first_ring"].astype(np.int64)), "first_ring is int32"), (dict(good, offset=torch.from_numpy(good["offset"])), "both be numpy"),
           (dict(good, offset=np.array([1, 4], np.int32)), "rise from 0"), (dict(good, offset=np.array([0, 3], np.int32)), "rise from 0"),
           (dict(good, vertices=good["vertices"] - 1), "0 .. 32767"), (dict(good, vertices=good["vertices"] + 32765), "0 .. 32767"),
           ({k: v for k, v in good.items() if k != "first_ring"}, "'first_ring' is missing"), ({k: v for k, v in good.items() if k != "label"}, "'label' is missing")]
    for rings, match in bad:
        with pytest.raises(ValueError, match=match):
            dsm.simplify_outlines(rings, 1.0)
    with pytest.raises(ValueError, match="resolutions"):
        dsm.simplify_outlines(good, 1.0, dsm.DSMGrid(0.0, 0.0, 0.0, 1.0, 5, 4))


def test_burn_polygons_rejects_bad_arguments_without_a_gpu():
    import torch
    from satmvs_amd import dsm
    v, off, lab = np.zeros((4, 2), np.int32), np.array([0, 4], np.int32), np.ones(1, np.int32)
    bad = [((v.astype(np.int64), off, lab, (4, 4)), "vertices is int32"), ((v.reshape(-1), off, lab, (4, 4)), "vertices has 2 axes"),
           ((np.zeros((4, 3), np.int32), off, lab, (4, 4)), "x, y"), ((v, off.astype(np.int64), lab, (4, 4)), "offset is int32"),
           ((v, off, lab.astype(np.float32), (4, 4)), "ring_label is int32"), ((v, np.array([0, 2, 4], np.int32), lab, (4, 4)), "n_rings \\+ 1"),
           ((v, torch.from_numpy(off), lab, (4, 4)), "both be numpy"), ((v, off, lab, (4,)), "pair of integers"), ((v, off, lab, (0, 4)), "positive sizes"),
           ((v, off, lab, (2 ** 16, 2 ** 15)), "2\\^31"), ((v, np.array([1, 4], np.int32), lab, (4, 4)), "rise from 0"),
           ((v, np.array([0, 3, 2, 4], np.int32), np.ones(3, np.int32), (4, 4)), "rise from 0")]
    for args, match in bad:
        with pytest.raises(ValueError, match=match):
            dsm.burn_polygons(*args)


# ---- argument rejections, C ------------------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_a_gpu(lib):
    from satmvs_amd import _lib
    MB = 1 << 20
    at = lambda i: C.c_void_p(i * MB)                        # noqa: E731  (made-up pointers a megabyte apart: nothing is dereferenced)
    nr, nv = 5, 40
    need = lib.smvs_dsm_simplify_workspace_bytes(nr, nv)
    assert 56 * nv + 29 * nr <= need < MB and lib.smvs_dsm_simplify_workspace_bytes(0, 0) > 0
    assert lib.smvs_dsm_simplify_workspace_bytes(-1, 4) == 0 and lib.smvs_dsm_simplify_workspace_bytes(4, -1) == 0
    assert lib.smvs_dsm_simplify_workspace_bytes(0, 4) == 0 and lib.smvs_dsm_simplify_workspace_bytes(4, 0) > 0

    def begin(v=at(1), off=at(2), nr=nr, nv=nv, flag=at(3), ws=at(4), nbytes=need):
        _lib.call("smvs_dsm_simplify_begin", v, off, nr, nv, flag, ws, nbytes, None)

    def rounds(v=at(1), off=at(2), nr=nr, nv=nv, tol16=16, rounds=8, status=at(3), ws=at(4), nbytes=need):
        _lib.call("smvs_dsm_simplify_rounds", v, off, nr, nv, tol16, rounds, status, ws, nbytes, None)

    def count(v=at(1), off=at(2), nr=nr, nv=nv, n_out=at(3), ws=at(4), nbytes=need):
        _lib.call("smvs_dsm_simplify_count", v, off, nr, nv, n_out, ws, nbytes, None)

    def write(v=at(1), off=at(2), nr=nr, nv=nv, n_out=20, ooff=at(5), overt=at(6), area2=at(7), kept=at(8), simp=at(9), ws=at(4), nbytes=need):
        _lib.call("smvs_dsm_simplify_write", v, off, nr, nv, n_out, ooff, overt, area2, kept, simp, ws, nbytes, None)

    def burn(vertices=at(1), offset=at(2), label=at(3), nr=2, nv=8, gw=9, gh=7, out=at(4), flag=at(5)):
        _lib.call("smvs_dsm_burn_polygons", vertices, offset, label, nr, nv, gw, gh, out, flag, None)

    bad = []
    for fn, word in ((begin, "flag"), (rounds, "status"), (count, "n_out")):
        bad += [(fn, dict(v=None), "null pointer"), (fn, dict(off=None), "null pointer"), (fn, dict(ws=None), "null pointer"), (fn, {word: None}, "null pointer"),
                (fn, dict(nr=-1), "n_rings and n_vertices"), (fn, dict(nv=-1), "n_rings and n_vertices"), (fn, dict(nr=0), "without rings"),
                (fn, dict(nbytes=need - 1), "workspace too small"), (fn, dict(ws=at(1)), "workspace aliases vertices"), (fn, dict(ws=at(2)), "workspace aliases offset"),
                (fn, {word: at(1)}, "%s aliases vertices" % word), (fn, {word: at(2)}, "%s aliases offset" % word), (fn, {word: at(4)}, "%s aliases workspace" % word),
                (fn, dict(off=at(1)), "offset aliases vertices")]
    bad += [(rounds, dict(tol16=-1), "tol16"), (rounds, dict(tol16=65536), "tol16"), (rounds, dict(rounds=-1), "rounds must be"), (rounds, dict(rounds=4097), "rounds must be"),
            (write, dict(v=None), "null pointer"), (write, dict(off=None), "null pointer"), (write, dict(ws=None), "null pointer"), (write, dict(ooff=None), "null pointer"),
            (write, dict(overt=None), "null pointer"), (write, dict(area2=None), "null pointer"), (write, dict(kept=None), "null pointer"),
            (write, dict(simp=None), "null pointer"), (write, dict(n_out=-1), "n_out"), (write, dict(n_out=nv + 1), "n_out"), (write, dict(nr=-1), "n_rings and n_vertices"),
            (write, dict(nbytes=need - 1), "workspace too small"), (write, dict(ooff=at(1)), "out_offset aliases vertices"),
            (write, dict(overt=at(2)), "out_vertices aliases offset"), (write, dict(area2=at(4)), "area2 aliases workspace"), (write, dict(kept=at(5)), "kept aliases out_offset"),
            (write, dict(simp=at(6)), "simplified aliases out_vertices"), (write, dict(simp=at(8)), "simplified aliases kept"),
            (burn, dict(out=None), "null pointer"), (burn, dict(flag=None), "null pointer"), (burn, dict(vertices=None), "null pointer"),
            (burn, dict(offset=None), "null pointer"), (burn, dict(label=None), "null pointer"), (burn, dict(nr=-1), "must be >= 0"),
            (burn, dict(nv=-1), "must be >= 0"), (burn, dict(gw=0), "non-positive grid"), (burn, dict(gw=2 ** 16, gh=2 ** 15), "grid too large"),
            (burn, dict(flag=at(4)), "flag aliases out"), (burn, dict(out=at(1)), "out aliases vertices"), (burn, dict(out=at(2)), "out aliases offset"),
            (burn, dict(out=at(3)), "out aliases ring_label"), (burn, dict(flag=at(1)), "flag aliases vertices")]
    for fn, kw, match in bad:
        with pytest.raises(_lib.SatMVSNativeError, match=match):
            fn(**kw)
