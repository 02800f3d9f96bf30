"""The contour oracle (tests/dsm_contour_oracle.py) without a device: its two statements against each other, against contourpy
where it is installed, the invariants the rule promises against independent counts, closed forms, contour_levels, the GeoJSON
round trip, the six planted errors the GPU file's comparison must report, and every argument rejection of dsm.contours,
dsm.contour_levels and dsm.write_contours on host arrays and of the three C entries on made-up pointers."""
import ctypes as C
import json

import numpy as np
import pytest

import dsm_contour_oracle as co
from dsm_testkit import lib  # noqa: F401  (fixture)

SHAPES = [(2, 2), (3, 9), (7, 2), (17, 23), (40, 50)]
LEVELS_M = [12.3, 18.0, 20.5, 26.1]


class Grid:                                                  # what the oracle reads of a DSMGrid
    def __init__(self, gh, gw, e0=500000.0, n0=3400000.0, xres=5.0, yres=2.5):
        self.e0, self.n0, self.xres, self.yres, self.width, self.height = e0, n0, xres, yres, gw, gh


def _cases():
    for i, shape in enumerate(SHAPES):
        for voids in (0.0, 0.05, 0.3):
            yield shape, voids, co.random_scene(*shape, seed=10 * i + int(10 * voids), voids=voids)


def _line(lines, i, key="vertices"):
    return lines[key][lines["offset"][i]:lines["offset"][i + 1]]


def _squares_of(e, gh, gw):
    """The squares on the two sides of lattice edge e that are on the lattice."""
    r, c, o = (e >> 1) // gw, (e >> 1) % gw, e & 1
    both = [(r - 1, c), (r, c)] if o == 0 else [(r, c - 1), (r, c)]
    return [s for s in both if 0 <= s[0] < gh - 1 and 0 <= s[1] < gw - 1]


def _live(ok, s):
    return bool(ok[s[0]:s[0] + 2, s[1]:s[1] + 2].all())


# ---- the two statements ----------------------------------------------------------------------------------------------------------
def test_the_two_statements_agree():
    K = co.level_keys(LEVELS_M)
    for shape, voids, z in _cases():
        co.same_lines(co.trace(z, K), co.walk(z, K), (shape, voids))
    z = co.random_scene(9, 11, seed=77)
    z[0, :4] = [np.inf, -np.inf, 32768.0, np.nextafter(np.float32(32768.0), np.float32(np.inf))]
    z[1, :4] = [-32768.0, 0.0, -0.0, np.float32(20.0) + np.float32(1.0 / 512.0)]         # a height on a quantisation half
    for K in (co.level_keys([-40000.0 / 2, 0.0, 19.99, 20.0, 30000.0]), np.array([-1, 1], np.int64), np.array([2 ** 25 - 1], np.int64)):
        co.same_lines(co.trace(z, K), co.walk(z, K), K.tolist())
    assert len(co.walk(z, np.array([2 ** 25 - 1], np.int64))["closed"]) == 0              # above every height


def test_against_contourpy():
    """Equal numbers of lines, closed lines and vertices per level, and every vertex within 1e-12 cells of one of contourpy's
    and the reverse, on scenes in which no saddle's corners sum to exactly 2 K (there contourpy's float mean may round)."""
    contourpy = pytest.importorskip("contourpy")
    K = co.level_keys(LEVELS_M)
    for shape, voids, z in _cases():
        ok, q = co.quantise(z)
        live = ok[:-1, :-1] & ok[:-1, 1:] & ok[1:, :-1] & ok[1:, 1:]
        total = q[:-1, :-1] + q[:-1, 1:] + q[1:, :-1] + q[1:, 1:]
        up = 2 * q[None] > K[:, None, None]
        saddle = (up[:, :-1, :-1] == up[:, 1:, 1:]) & (up[:, :-1, 1:] == up[:, 1:, :-1]) & (up[:, :-1, :-1] != up[:, :-1, 1:])
        assert (live[None] & saddle).any() or shape[0] * shape[1] < 100, (shape, voids)
        assert not (live[None] & saddle & (total[None] == 2 * K[:, None, None])).any(), (shape, voids)
        gen = contourpy.contour_generator(z=np.ma.masked_array(q / 256.0, mask=~ok), name="serial", corner_mask=False, line_type="Separate")
        got = co.trace(z, K)
        for li, k in enumerate(K):
            theirs = gen.lines(k / 512.0)
            ring = [len(p) > 1 and bool((p[0] == p[-1]).all()) for p in theirs]
            mine = range(got["first_line"][li], got["first_line"][li + 1])
            assert len(theirs) == len(mine) and sum(ring) == int(got["closed"][mine.start:mine.stop].sum()), (shape, voids, li)
            want = np.concatenate([p[:-1] if cl else p for p, cl in zip(theirs, ring)] + [np.zeros((0, 2))])
            have = got["vertices"][got["offset"][mine.start]:got["offset"][mine.stop]]
            assert len(want) == len(have), (shape, voids, li)
            if len(have):
                d = np.abs(have[:, None, :] - want[None, :, :]).max(axis=2)
                assert d.min(axis=1).max() <= 1e-12 and d.min(axis=0).max() <= 1e-12, (shape, voids, li)


# ---- what the rule promises --------------------------------------------------------------------------------------------------------
def test_invariants():
    K = co.level_keys(LEVELS_M)
    for shape, voids, z in _cases():
        what = (shape, voids)
        gh, gw = shape
        ok, q = co.quantise(z)
        lines = co.walk(z, K)
        # every crossing with a live square on either side appears exactly once, and nothing else does
        want = set()
        for li, k in enumerate(K.tolist()):
            for e in range(2 * gh * gw):
                r, c, o = (e >> 1) // gw, (e >> 1) % gw, e & 1
                b = (r, c + 1) if o == 0 else (r + 1, c)
                if b[0] < gh and b[1] < gw and ok[r, c] and ok[b] and (2 * q[r, c] > k) != (2 * q[b] > k) and any(_live(ok, s) for s in _squares_of(e, gh, gw)):
                    want.add((li, e))
        have = list(zip(np.repeat(lines["level_index"], np.diff(lines["offset"])).tolist(), lines["edge"].tolist()))
        assert len(have) == len(set(have)) and set(have) == want, what
        assert co.n_cross(z, K) >= len(have)
        first = [int(_line(lines, i, "edge")[0]) for i in range(len(lines["closed"]))]
        order = list(zip(lines["level_index"].tolist(), first))
        assert order == sorted(order) and len(set(order)) == len(order), what
        assert lines["first_line"][0] == 0 and lines["first_line"][-1] == len(first) and (np.diff(lines["first_line"]) >= 0).all(), what
        for i in range(len(first)):
            e, v, closed = _line(lines, i, "edge").tolist(), _line(lines, i), bool(lines["closed"][i])
            assert len(e) >= (4 if closed else 2), (what, i)
            if closed:
                assert e[0] == min(e), (what, i)
            pairs = list(zip(e, e[1:] + e[:1])) if closed else list(zip(e[:-1], e[1:]))
            for e1, e2 in pairs:                             # consecutive vertices share a live square and differ
                assert e1 != e2 and any(_live(ok, s) for s in _squares_of(e1, gh, gw) if s in _squares_of(e2, gh, gw)), (what, i)
            assert (np.abs(np.diff(v, axis=0)).max(axis=1) > 0).all(), (what, i)
            assert lines["level"][i] == K[lines["level_index"][i]] / 512.0


def test_height_at_the_vertices():
    """The bilinear surface of the quantised heights at a vertex against the level.  The bound: with f = x - c (exact: c is a
    multiple of ulp(x)), |f - t| <= 2^-53 t (the division) + 2^(6 - 53) (the addition: x < 64 on these grids); za + f (zb - za)
    in float64 with |zb - za| <= 2^16 and |z| <= 2^15 is off by at most 2^16 (2^-53 + 2^-47) + 2^16 2^-53 + 2^15 2^-53 < 2^-30.
    The assertion is the 2^-29 m of the rule's statement."""
    K = co.level_keys([-100.0] + LEVELS_M + [5000.0])
    for shape, voids, z in _cases():
        z = z.copy()
        z[0, 0], z[-1, -1] = 32768.0, -32768.0               # the largest differences the rule admits
        ok, q = co.quantise(z)
        lines = co.trace(z, K)
        gw = shape[1]
        e = lines["edge"].astype(np.int64)
        r, c, o = (e >> 1) // gw, (e >> 1) % gw, e & 1
        za, zb = q[r, c] / 256.0, q[r + o, c + 1 - o] / 256.0
        f = np.where(o == 0, lines["vertices"][:, 0] - c, lines["vertices"][:, 1] - r)
        assert ((f > 0) & (f < 1)).all() and (np.where(o == 0, lines["vertices"][:, 1] - r, lines["vertices"][:, 0] - c) == 0).all()
        level = np.repeat(lines["level"], np.diff(lines["offset"]))
        assert len(f) == 0 or np.abs(za + f * (zb - za) - level).max() <= 2.0 ** -29, (shape, voids)


# ---- closed forms ----------------------------------------------------------------------------------------------------------------
def test_plane():
    gh, gw = 6, 9
    z = np.tile(np.arange(gw, dtype=np.float32), (gh, 1))    # the height is the column: high ground to the east
    K = co.level_keys(np.arange(gw - 1) + 0.5)
    for lines in (co.walk(z, K), co.trace(z, K)):
        assert len(lines["closed"]) == gw - 1 and not lines["closed"].any() and lines["offset"].tolist() == list(range(0, gh * gw, gh))
        for i in range(gw - 1):                              # east on the left: the line runs south, from row 0 to the last row
            assert _line(lines, i).tolist() == [[i + 0.5 + 1.0 / 512.0, float(r)] for r in range(gh)]
            assert _line(lines, i, "edge").tolist() == [2 * (r * gw + i) for r in range(gh)]
    lines = co.trace(z.T.copy(), K)                          # high ground to the south: the lines run west
    assert _line(lines, 2).tolist() == [[float(c), 2.5 + 1.0 / 512.0] for c in range(gh)][::-1]
    lines = co.trace(-z, co.level_keys([-2.5]))              # high ground to the west: north
    assert _line(lines, 0)[:, 1].tolist() == [float(r) for r in range(gh)][::-1]


def test_cone_rings_run_counter_clockwise():
    z = co.cone(31, 33)
    K = co.level_keys([10.0, 20.0, 30.0, 40.0, 60.0])
    lines = co.trace(z, K)
    co.same_lines(lines, co.walk(z, K), "cone")
    closed = lines["closed"]
    assert closed[lines["level_index"] >= 1].all() and (lines["level_index"] < 4).all() and np.diff(lines["first_line"]).tolist()[1:] == [1, 1, 1, 0]
    for i in np.flatnonzero(closed):
        assert co.shoelace2(_line(lines, i)) > 0
    pit = co.trace(-z, co.level_keys([-30.0]))
    assert pit["closed"].tolist() == [True] and co.shoelace2(_line(pit, 0)) < 0


def test_single_saddle_square():
    """Highs at (0, 0) and (1, 1), q = 257, lows 0: the corners sum to 514.  K = 255: the mean is above (514 > 510), the lines
    pass between the highs' far sides and cut off the lows; K = 257, the tie, and K = 259: not above, they cut off the highs."""
    z = np.array([[257, 0], [0, 257]], np.float32) / np.float32(256.0)
    K = np.array([255, 257, 259], np.int64)
    for lines in (co.walk(z, K), co.trace(z, K)):
        assert lines["first_line"].tolist() == [0, 2, 4, 6] and not lines["closed"].any()
        sets = [sorted(_line(lines, i, "edge").tolist()) for i in range(6)]
        assert sorted(sets[0:2]) == [[0, 3], [1, 4]] and sorted(sets[2:4]) == [[0, 1], [3, 4]] == sorted(sets[4:6])
        assert _line(lines, 2, "edge").tolist() == [1, 0]    # round the high at (0, 0) with it on the left: from the left edge to the top edge


def test_one_cell_wide_grids_have_crossings_but_no_line():
    K = co.level_keys([0.5, 1.5, 2.5])
    for z in (np.arange(7, dtype=np.float32)[None, :], np.arange(5, dtype=np.float32)[:, None], np.zeros((1, 1), np.float32)):
        for lines in (co.walk(z, K), co.trace(z, K)):
            assert len(lines["closed"]) == 0 and lines["vertices"].shape == (0, 2) and lines["offset"].tolist() == [0] and lines["first_line"].tolist() == [0] * 4
        assert co.n_cross(z, K) == (3 if z.size > 1 else 0)


def test_serpentine_is_one_long_ring():
    lines = co.trace(co.serpentine(33, 21), co.level_keys([5.0]))
    assert lines["closed"].tolist() == [True] and len(lines["vertices"]) > 0.9 * 33 * 21


# ---- the comparison reports the planted errors -----------------------------------------------------------------------------------
@pytest.mark.parametrize("plant", co.PLANTED)
def test_planted_errors_are_reported(plant):
    z = co.random_scene(40, 50, seed=4)
    K = co.level_keys(LEVELS_M)
    want = co.walk(z, K)
    assert co.difference(co.trace(z, K), want) is None
    assert co.difference(co.walk(z, K, plant=plant), want) is not None, plant
    with pytest.raises(AssertionError):
        co.same_lines(co.walk(z, K, plant=plant), want, plant)


def test_difference_reports_table_damage():
    want = co.trace(co.random_scene(12, 13, seed=2), co.level_keys(LEVELS_M))
    for key in co.KEYS:
        bad = {k: v.copy() for k, v in want.items()}
        flat = bad[key].reshape(-1)
        flat[-1] = ~flat[-1] if flat.dtype == bool else np.nextafter(flat[-1], np.inf) if flat.dtype == np.float64 else flat[-1] + 1
        assert co.difference(bad, want) is not None, key
        bad[key] = want[key].astype(np.float32)
        assert "dtype" in co.difference(bad, want)
    assert "missing" in co.difference({k: v for k, v in want.items() if k != "offset"}, want)


# ---- the Python layer without a device -------------------------------------------------------------------------------------------
def test_contour_levels():
    from satmvs_amd import dsm
    z = np.array([[10.0, 12.5], [np.nan, 20.0], [-999.0, 40000.0]], np.float32)
    assert dsm.contour_levels(z, 2.5).tolist() == [12.5, 15.0, 17.5]                     # strictly inside 10 .. 20
    assert dsm.contour_levels(z, 5.0, base=1.0).tolist() == [11.0, 16.0]
    assert dsm.contour_levels(z, 100.0).tolist() == [] and dsm.contour_levels(np.full((2, 2), np.nan, np.float32), 1.0).tolist() == []
    assert dsm.contour_levels(z, 2.5, nodata=10.0).tolist() == [-997.5 + 2.5 * k for k in range(407)]
    big = co.random_scene(17, 23, seed=3)
    for interval, base in ((1.0, 0.0), (0.7, 0.3), (2.5, -1.0)):
        got = dsm.contour_levels(big, interval, base)
        assert got.dtype == np.float64 and np.array_equal(got, co.levels_for(big, interval, base))
    for bad in (0, -1.0, np.nan, np.inf, "1", None, True):
        with pytest.raises(ValueError, match="interval"):
            dsm.contour_levels(z, bad)
    with pytest.raises(ValueError, match="base"):
        dsm.contour_levels(z, 1.0, base=np.nan)
    with pytest.raises(ValueError, match="2\\^20"):
        dsm.contour_levels(z, 1e-6)


def test_geojson_round_trip(tmp_path):
    from satmvs_amd import dsm
    gh, gw = 17, 23
    grid = dsm.DSMGrid(500000.0, 3400000.0, 5.0, 2.5, gw, gh)
    K = co.level_keys(LEVELS_M)
    lines = co.with_grid(co.trace(co.random_scene(gh, gw, seed=3), K), grid)
    assert lines["closed"].any() and not lines["closed"].all()
    path = str(tmp_path / "contours.geojson")
    assert dsm.write_contours(path, lines, grid) == len(lines["closed"])
    features = co.read_geojson(path)
    for i, (prop, xy) in enumerate(features):
        want = _line(lines, i, "vertices_en")
        assert sorted(prop) == ["closed", "length_m", "level_m"] and prop["closed"] == bool(lines["closed"][i]) and prop["level_m"] == lines["level"][i]
        assert np.array_equal(xy[:len(want)], want) and len(xy) == len(want) + int(prop["closed"]) and (not prop["closed"] or (xy[0] == xy[-1]).all())
        steps = np.sqrt((np.diff(xy, axis=0) ** 2).sum(axis=1))
        assert prop["length_m"] == lines["length_m"][i] and abs(prop["length_m"] - steps.sum()) <= (len(xy) + 2) * 2.0 ** -52 * steps.sum()
    bare = {k: lines[k] for k in co.KEYS}                    # without length_m: computed on the host, the same bits
    assert dsm.write_contours(path, bare, grid) == len(features)
    assert [p["length_m"] for p, _ in co.read_geojson(path)] == lines["length_m"].tolist()
    assert features[0][1][0].tolist() == [500000.0 + 5.0 * lines["vertices"][0, 0], 3400000.0 - 2.5 * lines["vertices"][0, 1]]
    empty = co.trace(np.zeros((3, 3), np.float32), K)
    assert dsm.write_contours(path, empty, grid) == 0 and co.read_geojson(path) == []
    with open(path) as f:
        assert json.load(f) == {"type": "FeatureCollection", "features": []}
    with pytest.raises(ValueError, match="missing"):
        dsm.write_contours(path, {k: v for k, v in lines.items() if k != "level"}, grid)
    with pytest.raises(ValueError, match="dict of contours"):
        dsm.write_contours(path, dict(lines, offset=lines["offset"][:-1]), grid)
    with pytest.raises(ValueError, match="resolutions"):
        dsm.write_contours(path, lines, dsm.DSMGrid(0.0, 0.0, 0.0, 1.0, gw, gh))


def test_contours_rejects_bad_arguments_without_a_gpu():
    from satmvs_amd import dsm
    good = np.zeros((4, 5), np.float32)
    for z, match in ((np.zeros(5, np.float32), "gh, gw"), (np.zeros((2, 4, 5), np.float32), "gh, gw"), (np.zeros((0, 5), np.float32), "positive sizes"),
                     (np.broadcast_to(np.float32(0), (2 ** 15, 2 ** 14)), "2\\^29")):
        with pytest.raises(ValueError, match=match):
            dsm.contours(z, levels=[1.0])
    with pytest.raises(ValueError, match="exactly one"):
        dsm.contours(good)
    with pytest.raises(ValueError, match="exactly one"):
        dsm.contours(good, levels=[1.0], interval=1.0)
    for levels, match in (([1.0, np.nan], "finite"), ([np.inf], "finite"), ([32768.5], "32768"), ([-40000.0], "32768"), ([[1.0, 2.0]], "list of heights"),
                          ([1.0, 1.001], "same step"), ([2.0, 1.0, 2.0], "same step")):
        with pytest.raises(ValueError, match=match):
            dsm.contours(good, levels=levels)
    with pytest.raises(ValueError, match="interval"):
        dsm.contours(good, interval=0.0)
    with pytest.raises(ValueError, match="differs from the grid"):
        dsm.contours(good, levels=[1.0], grid=dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, 4, 5))
    with pytest.raises(ValueError, match="resolutions"):
        dsm.contours(good, levels=[1.0], grid=dsm.DSMGrid(0.0, 0.0, -5.0, 5.0, 5, 4))
    assert dsm._level_keys([0.0, -0.001, 1.0 / 256.0, 32768.0, -32768.0]).tolist() == [-2 ** 24 + 1, -1, 1, 3, 2 ** 24 + 1]


# ---- argument rejections, C ------------------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_a_gpu(lib):
    from satmvs_amd import _lib
    MB = 1 << 20
    at = lambda i: C.c_void_p(i * MB)                        # noqa: E731  (made-up pointers a megabyte apart: nothing is dereferenced)
    gw, gh = 9, 7
    lv = np.array([-3, 1, 5], np.int32)                      # the levels are a host array: read before any HIP call
    host = lambda a: a.ctypes.data_as(C.c_void_p)            # noqa: E731
    size = lib.smvs_dsm_contour_workspace_bytes
    need0, need = size(gw, gh, 3, 0), size(gw, gh, 3, 64)
    assert need > need0 >= 8 * gw * gh + 4 * 4096 and 35 * 64 <= need - need0 < 47 * 64 + 20 * 256 and need < MB
    assert size(0, 5, 1, 0) == 0 and size(5, -1, 1, 0) == 0 and size(5, 5, 0, 0) == 0 and size(5, 5, 4097, 0) == 0 and size(5, 5, 1, -1) == 0
    assert size(2 ** 15, 2 ** 14, 1, 0) == 0 and size(2 ** 15 - 1, 2 ** 14, 1, 0) > 0 and size(5, 5, 4096, 2 ** 31 - 1) > 47 * (2 ** 31 - 1)

    def count(dsm=at(1), gw=gw, gh=gh, levels=lv, n=3, max_cross=64, counts=at(2), ws=at(3), nbytes=need):
        _lib.call("smvs_dsm_contour_count", dsm, gw, gh, -999.0, None if levels is None else host(levels), n, max_cross, counts, ws, nbytes, None)

    def write(dsm=at(1), gw=gw, gh=gh, levels=lv, n=3, nc=64, nl=2, nv=8, level=at(4), closed=at(5), offset=at(6), first=at(7),
              vertices=at(8), edge=at(9), ws=at(3), nbytes=need):
        _lib.call("smvs_dsm_contour_write", dsm, gw, gh, -999.0, None if levels is None else host(levels), n, nc, nl, nv, level, closed, offset,
                  first, vertices, edge, ws, nbytes, None)

    i32 = lambda a: np.array(a, np.int32)                    # noqa: E731
    both = [(dict(dsm=None), "null pointer"), (dict(levels=None), "null pointer"), (dict(ws=None), "null pointer"), (dict(gw=0), "non-positive grid"),
            (dict(gh=-2), "non-positive grid"), (dict(gw=2 ** 15, gh=2 ** 14), "below 2\\^29"), (dict(n=0), "n_levels"), (dict(n=4097), "n_levels"),
            (dict(levels=i32([1, 2, 5])), "odd"), (dict(levels=i32([1, 1, 5])), "rise"), (dict(levels=i32([5, 3, 7])), "rise"),
            (dict(levels=i32([1, 3, 2 ** 25 + 1])), "2\\^25"), (dict(levels=i32([-2 ** 25 - 1, 3, 5])), "2\\^25"), (dict(nbytes=need - 1), "workspace too small"),
            (dict(ws=at(1)), "workspace aliases dsm")]
    bad = [(count, kw, match) for kw, match in both] + [(write, kw, match) for kw, match in both] + [
        (count, dict(counts=None), "null pointer"), (count, dict(max_cross=-1), "max_cross"), (count, dict(counts=at(1)), "counts aliases dsm"),
        (count, dict(ws=at(2)), "workspace aliases counts"),
        (write, dict(offset=None), "null pointer"), (write, dict(first=None), "null pointer"), (write, dict(level=None), "null pointer"),
        (write, dict(closed=None), "null pointer"), (write, dict(vertices=None), "null pointer"), (write, dict(nc=-1), "max_cross"),
        (write, dict(nl=-1), "n_lines"), (write, dict(nv=-1), "n_lines"), (write, dict(nl=0), "n_lines"), (write, dict(nv=0), "n_lines"),
        (write, dict(nv=65), "n_lines"), (write, dict(nl=5), "n_lines"), (write, dict(level=at(1)), "line_level aliases dsm"),
        (write, dict(closed=at(4)), "line_closed aliases line_level"), (write, dict(offset=at(3)), "offset aliases workspace"),
        (write, dict(first=at(6)), "first_line aliases offset"), (write, dict(vertices=at(7)), "vertices aliases first_line"),
        (write, dict(edge=at(8)), "vertex_edge aliases vertices"), (write, dict(edge=at(1)), "vertex_edge aliases dsm")]
    for fn, kw, match in bad:
        with pytest.raises(_lib.SatMVSNativeError, match=match):
            fn(**kw)
