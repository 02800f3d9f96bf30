"""The stream network without a GPU: the two Python statements of every part of the rule (dsm_stream_oracle.py) against each
other on the scenes the GPU file runs, invariants, closed forms, the GeoJSON writer on host arrays, the argument rejections of
the Python functions and of the C entries, and the planted errors that the GPU file's comparison has to report."""
import ctypes as C
import json

import numpy as np
import pytest

import dsm_hydro_oracle as ho
import dsm_stream_oracle as so
from dsm_testkit import lib  # noqa: F401  (fixture)


def _both(code, mask, what):
    """The network by both statements, equal in every entry -> the loops' one."""
    a, b = so.network(code, mask, arrays=False), so.network(code, mask, arrays=True)
    assert so.differing(a, b) == [] and so.differing(b, a) == [], what
    return a


def _invariants(code, net, what):
    gh, gw = code.shape
    order_map, link = net["order_map"].reshape(-1), net["link"].reshape(-1)
    head, order, nxt, offset, v, steps = (net[k] for k in ("head", "order", "next_link", "offset", "vertices", "steps"))
    nl = len(head)
    in_s = order_map > 0
    assert np.array_equal(in_s, link > 0) and nl == net["counts"][1] and in_s.sum() == net["counts"][0], what
    assert np.array_equal(np.sort(np.unique(link[in_s])), np.arange(1, nl + 1)), what                   # every cell of S in exactly one link
    assert np.array_equal(np.sort(head), head) and np.array_equal(link[head], np.arange(1, nl + 1)), what
    cells = v[:, 1].astype(np.int64) * gw + v[:, 0]
    own = 0
    for k in range(nl):
        c = cells[offset[k]:offset[k + 1] - (1 if nxt[k] >= 0 else 0)]
        own += len(c)
        assert (link[c] == k + 1).all() and (order_map[c] == order[k]).all() and c[0] == head[k], what   # constant along a link
        if nxt[k] >= 0:
            assert order[nxt[k]] >= order[k] and cells[offset[k + 1] - 1] == head[nxt[k]], what            # never falls downstream
        d = np.abs(np.diff(v[offset[k]:offset[k + 1]], axis=0))
        assert (d.max(axis=1) == 1).all() if len(d) else True, what
        assert list(steps[k]) == [int(((d[:, 0] == 1) & (d[:, 1] == 0)).sum()), int(((d[:, 0] == 0) & (d[:, 1] == 1)).sum()), int((d.sum(axis=1) == 2).sum())], what
    assert own == in_s.sum() and len(v) - own == (nxt >= 0).sum(), what
    seen = np.zeros(nl, bool)                                 # the link tree has no cycle: every walk along next_link ends
    for k in range(nl):
        at, walk = k, 0
        while at >= 0 and not seen[at]:
            at, walk = nxt[at], walk + 1
            assert walk <= nl, what
        seen[k] = True
    sources = int((order == 1).sum()) if nl else 0
    assert net["counts"][3] <= (int(np.log2(sources)) + 1 if sources else 0), what


# ---- the statement pairs, invariants ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", so.RANDOM_SCENES)
def test_the_two_statements_agree_on_random_scenes(case):
    code, acc = so.hill_codes(*case)
    top = 0
    for name, mask in so.masks_of(code, acc):
        net = _both(code, mask, (case, name))
        _invariants(code, net, (case, name))
        top = max(top, int(net["counts"][3]))
    a, ca = so.flow_length_walk(code)
    b, cb = so.flow_length_doubling(code)
    assert np.array_equal(a, b) and not ca and not cb
    assert top >= (3 if case[3] < 0.3 else 2)
    if case[0] == 257:                                        # what the issue counted on this scene
        assert so.network(code, acc >= 1)["counts"][0] == 73537


@pytest.mark.parametrize("shape", so.SIZES)
def test_the_two_statements_agree_on_small_grids(shape):
    gh, gw = shape
    code, acc = so.hill_codes(gh, gw, gh + gw, 0.02 if gh * gw > 500 else 0.0, 12)
    for name, mask in (("all ones", np.ones(shape, bool)), ("acc >= 2", acc >= 2)):
        _invariants(code, _both(code, mask, (shape, name)), (shape, name))
    assert np.array_equal(so.flow_length_walk(code)[0], so.flow_length_doubling(code)[0])


def test_flow_length_falls_by_one_step_kind_along_every_step():
    code, _ = so.hill_codes(*so.RANDOM_SCENES[3])
    steps, _ = so.flow_length_doubling(code)
    recv = ho.receivers_arrays(code)
    flat = steps.reshape(-1, 3).astype(np.int64)
    moves = np.nonzero(recv >= 0)[0]
    fall = flat[moves] - flat[recv[moves]]
    assert (fall.sum(axis=1) == 1).all() and (fall.min(axis=1) == 0).all()
    assert np.array_equal(np.argmax(fall, axis=1), so.step_kind(code.reshape(-1)[moves]))
    assert (flat[recv == ho.ROOT] == 0).all() and (flat[recv == ho.VOID] == -1).all()


def test_cycles_and_arbitrary_code_grids():
    code = so.cyclic_grid()
    net = _both(code, np.ones(code.shape, bool), "cyclic grid")
    plain, cyc = ho.accumulate_subtrees(code)
    assert net["cyclic"] and cyc and np.array_equal(net["order_map"] == 0, (plain <= 0))             # cyclic and void cells are outside S
    a, ca = so.flow_length_walk(code)
    b, cb = so.flow_length_doubling(code)
    assert np.array_equal(a, b) and ca and cb and np.array_equal(a[..., 0] == -1, plain <= 0)
    rng = np.random.default_rng(5)
    codes = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 9, 254, 255], np.uint8)
    for _ in range(30):
        shape = tuple(rng.integers(1, 25, 2))
        code = rng.choice(codes, shape)
        mask = rng.random(shape) < 0.8
        _invariants(code, _both(code, mask, "random codes"), "random codes")
        assert np.array_equal(so.flow_length_walk(code)[0], so.flow_length_doubling(code)[0])


# ---- closed forms ------------------------------------------------------------------------------------------------------------------
def test_htree_is_a_complete_binary_tree():
    code, root = so.htree(7)
    assert (code <= 8).sum() == 465
    net = _both(code, code <= 8, "H-tree")
    order, nxt = net["order"], net["next_link"]
    assert net["order_map"][root] == 8 and list(net["counts"]) == [465, 255, 465 + 254, 8]
    assert [int((order == k).sum()) for k in range(1, 9)] == [128, 64, 32, 16, 8, 4, 2, 1]
    inner = nxt >= 0
    assert inner.sum() == 254 and (order[nxt[inner]] == order[inner] + 1).all()
    assert (np.bincount(nxt[inner], minlength=255)[order > 1] == 2).all()
    _invariants(code, net, "H-tree")


def test_comb_collector_stays_order_two():
    z = ho.comb(257, 301)
    code, _ = so.code_of(z)
    net = _both(code, z < 150.0, "comb")
    teeth = len(range(1, 300, 2))
    assert net["counts"][1] == 2 * teeth - 1 and net["counts"][3] == 2 and (net["order"] == 1).sum() == teeth
    assert (net["order_map"][255, 3:] == 2).all() and (net["order_map"][255, 1:3] == 1).all()


def test_serpentine_is_one_link():
    code, path = so.serpentine_codes(257, 301)
    net = _both(code, code <= 8, "serpentine")
    assert list(net["counts"]) == [len(path), 1, len(path), 1] and net["next_link"][0] == -1
    assert np.array_equal(net["vertices"], np.array([(c, r) for r, c in reversed(path)], np.int32))
    turns = len(range(1, 256, 2)) - 1
    assert list(net["steps"][0]) == [len(path) - 1 - 2 * turns, 2 * turns, 0]
    steps, _ = so.flow_length_walk(code)
    assert list(steps[path[-1]]) == list(net["steps"][0]) and list(steps[path[1]]) == [1, 0, 0]


def test_junction_closed_forms():
    for name, (code, cell, order) in so.junction_codes().items():
        net = _both(code, code <= 8, name)
        assert net["order_map"][cell] == order, name
        _invariants(code, net, name)
    code, cell, _ = so.junction_codes()["a mouth with eight inflows"]
    net = so.network(code, code <= 8)
    k = net["link"][cell] - 1                                 # a junction that is itself a mouth: a link of one vertex
    assert net["offset"][k + 1] - net["offset"][k] == 1 and net["next_link"][k] == -1 and (np.delete(net["next_link"], k) == k).all()
    assert list(net["head"][:3]) == [6, 7, 8]                 # heads adjacent in row-major order keep that order
    lone = np.zeros((3, 4), np.uint8)
    both = _both(lone, np.array([[0, 0, 0, 0], [0, 1, 0, 1], [0, 0, 0, 0]]), "two unconnected cells")
    assert list(both["counts"]) == [2, 2, 2, 1] and list(both["offset"]) == [0, 1, 2]


# ---- the writer ------------------------------------------------------------------------------------------------------------------
def test_geojson_round_trip_on_host_arrays(tmp_path):
    from satmvs_amd import dsm
    code, acc = so.hill_codes(*so.RANDOM_SCENES[0])
    net = so.network(code, acc >= 4)
    grid = dsm.DSMGrid(500000.0, 3400000.0, 5.0, 2.5, 50, 40)
    path = str(tmp_path / "streams.geojson")
    lines = int((np.diff(net["offset"]) >= 2).sum())
    assert dsm.write_streams(path, net, grid) == lines
    with open(path) as f:
        doc = json.load(f)
    assert doc["type"] == "FeatureCollection" and len(doc["features"]) == lines
    first = {}
    for f in doc["features"]:
        first[f["properties"]["link"]] = f["geometry"]["coordinates"][0]
    total = 0
    for f in doc["features"]:
        p, xy = f["properties"], np.array(f["geometry"]["coordinates"])
        k = p["link"]
        assert f["geometry"]["type"] == "LineString" and p["order"] == net["order"][k] and p["next_link"] == net["next_link"][k]
        assert np.array_equal(xy, np.stack([500000.0 + 5.0 * net["vertices"][net["offset"][k]:net["offset"][k + 1], 0],
                                            3400000.0 - 2.5 * net["vertices"][net["offset"][k]:net["offset"][k + 1], 1]], axis=1))
        assert p["length_m"] == float(so.length_m(net["steps"][k], 5.0, 2.5)) and p["n_cells"] == len(xy) - (p["next_link"] >= 0)
        if p["next_link"] >= 0 and p["next_link"] in first:
            assert list(xy[-1]) == first[p["next_link"]]
        total += p["n_cells"]
    skipped = np.diff(net["offset"]) < 2
    assert total + skipped.sum() == net["counts"][0]
    for key in ("order", "offset", "steps"):
        with pytest.raises(ValueError, match=key):
            dsm.write_streams(path, {k: v for k, v in net.items() if k != key}, grid)
    with pytest.raises(ValueError, match="stream_links"):
        dsm.write_streams(path, dict(net, offset=net["offset"][:-1]), grid)
    empty = so.network(code, np.zeros(code.shape, bool))
    assert dsm.write_streams(path, empty, grid) == 0

    class Scaled:                                             # a projection's interface: (n, 2) east, north -> lat, lon
        def EastNorth2latlon(self, en):
            return np.asarray(en)[:, ::-1] / 65536.0

    assert dsm.write_streams(path, net, grid, Scaled()) == lines
    with open(path) as f:
        lon, lat = json.load(f)["features"][0]["geometry"]["coordinates"][0]
    k = doc["features"][0]["properties"]["link"]
    col, row = net["vertices"][net["offset"][k]]
    assert lon == (500000.0 + 5.0 * col) / 65536.0 and lat == (3400000.0 - 2.5 * row) / 65536.0


# ---- argument rejections, Python -----------------------------------------------------------------------------------------------
def test_functions_reject_bad_arguments_without_a_gpu():
    from satmvs_amd import dsm
    codes, mask = np.zeros((4, 5), np.uint8), np.ones((4, 5), bool)
    grid = dsm.DSMGrid(0.0, 0.0, 5.0, 2.5, 5, 4)
    wrong_grid = dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, 4, 5)
    bad_codes = ((codes.astype(np.int32), "uint8"), (codes[0], "gh, gw"), (np.zeros((0, 5), np.uint8), "positive sizes"),
                 (np.broadcast_to(np.uint8(0), (2 ** 15, 2 ** 15)), "2\\^30"))
    for d, match in bad_codes:
        for fn in (lambda d: dsm.stream_order(d, mask), lambda d: dsm.stream_links(d, mask), dsm.flow_length):
            with pytest.raises(ValueError, match=match):
                fn(d)
    for fn in (dsm.stream_order, dsm.stream_links):
        for m, match in ((mask.astype(np.float32), "bool or an integer"), (mask[0], "gh, gw"), (np.ones((5, 4), bool), "differs from the directions")):
            with pytest.raises(ValueError, match=match):
                fn(codes, m)
        with pytest.raises(ValueError, match="cycles"):
            fn(codes, mask, cycles="ignore")
    with pytest.raises(ValueError, match="cycles"):
        dsm.flow_length(codes, cycles=None)
    with pytest.raises(ValueError, match="differs from the grid"):
        dsm.stream_links(codes, mask, grid=wrong_grid)
    with pytest.raises(ValueError, match="differs from the grid"):
        dsm.flow_length(codes, grid=wrong_grid)
    with pytest.raises(ValueError, match="resolutions"):
        dsm.flow_length(codes, grid=dsm.DSMGrid(0.0, 0.0, 5.0, 0.0, 5, 4))
    good = np.zeros((4, 5), np.float32)
    with pytest.raises(ValueError, match="float32"):
        dsm.extract_streams(good.astype(np.float64), grid)
    with pytest.raises(ValueError, match="differs from the grid"):
        dsm.extract_streams(good, wrong_grid)
    for value in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="min_area_m2"):
            dsm.extract_streams(good, grid, min_area_m2=value)
    with pytest.raises(ValueError, match="resolutions"):
        dsm.write_streams("unused", so.network(codes, mask), dsm.DSMGrid(0.0, 0.0, 0.0, 5.0, 5, 4))


# ---- argument rejections, C ----------------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_a_gpu(lib):
    from satmvs_amd import _lib
    MB = 1 << 20
    at = lambda i: C.c_void_p(i * MB)                        # noqa: E731  (made-up pointers a megabyte apart: nothing is dereferenced)
    gw, gh = 9, 7
    n = gw * gh
    size = lib.smvs_dsm_stream_workspace_bytes
    ws = size(gw, gh)
    assert 54 * n <= ws < 54 * n + 10 * 256 + 512 and ws < MB
    assert size(0, 5) == 0 and size(5, -1) == 0 and size(2 ** 15, 2 ** 15) == 0 and size(2 ** 15 - 1, 2 ** 15) > 54 * (2 ** 30 - 2 ** 15)

    def order(code=at(1), mask=at(2), gw=gw, gh=gh, out=at(3), link=at(4), counts=at(5), flag=at(6), ws=at(7), nbytes=ws):
        _lib.call("smvs_dsm_stream_order", code, mask, gw, gh, out, link, counts, flag, ws, nbytes, None)

    def write(code=at(1), mask=at(2), gw=gw, gh=gh, nl=5, nv=9, head=at(3), link_order=at(4), nxt=at(5), offset=at(6), vertices=at(8), steps=at(9), ws=at(7), nbytes=ws):
        _lib.call("smvs_dsm_stream_write", code, mask, gw, gh, nl, nv, head, link_order, nxt, offset, vertices, steps, ws, nbytes, None)

    def length(code=at(1), gw=gw, gh=gh, steps=at(3), flag=at(6), ws=at(7), nbytes=ws):
        _lib.call("smvs_dsm_flow_length", code, gw, gh, steps, flag, ws, nbytes, None)

    grids = [(dict(gw=0), "non-positive grid"), (dict(gh=-2), "non-positive grid"), (dict(gw=2 ** 15, gh=2 ** 15), "below 2\\^30")]
    bad = [(fn, kw, match) for fn in (order, write, length) for kw, match in grids]
    for fn in (order, write, length):
        bad += [(fn, dict(code=None), "null pointer"), (fn, dict(ws=None), "null pointer"), (fn, dict(nbytes=ws - 1), "workspace too small"),
                (fn, dict(ws=at(1)), "workspace aliases dir")]
    bad += [(order, {k: None}, "null pointer") for k in ("mask", "out", "counts", "flag")]
    bad += [(order, dict(mask=at(1)), "mask aliases dir"), (order, dict(out=at(2)), "order aliases mask"), (order, dict(link=at(3)), "link_map aliases order"),
            (order, dict(counts=at(4)), "counts aliases link_map"), (order, dict(flag=at(5)), "flag aliases counts"), (order, dict(ws=at(6)), "workspace aliases flag"),
            (order, dict(ws=at(4)), "workspace aliases link_map")]
    bad += [(write, {k: None}, "null pointer") for k in ("mask", "head", "link_order", "nxt", "offset", "vertices", "steps")]
    bad += [(write, dict(nl=-1), "negative count"), (write, dict(nv=-1), "negative count"), (write, dict(nl=n + 1), "more links"), (write, dict(nv=2 * n + 1), "more links"),
            (write, dict(mask=at(1)), "mask aliases dir"), (write, dict(head=at(2)), "head aliases mask"), (write, dict(link_order=at(3)), "link_order aliases head"),
            (write, dict(nxt=at(4)), "next_link aliases link_order"), (write, dict(offset=at(5)), "offset aliases next_link"),
            (write, dict(vertices=at(6)), "vertices aliases offset"), (write, dict(steps=at(8)), "steps aliases vertices"), (write, dict(ws=at(9)), "workspace aliases steps"),
            (write, dict(ws=at(6)), "workspace aliases offset")]
    bad += [(length, dict(steps=None), "null pointer"), (length, dict(flag=None), "null pointer"), (length, dict(steps=at(1)), "steps aliases dir"),
            (length, dict(flag=at(3)), "flag aliases steps"), (length, dict(ws=at(6)), "workspace aliases flag")]
    for fn, kw, match in bad:
        with pytest.raises(_lib.SatMVSNativeError, match=match):
            fn(**kw)
    # what may be null is null without complaint up to the first HIP call, which these made-up pointers must not reach: the
    # check that comes last (the workspace size) still fires
    with pytest.raises(_lib.SatMVSNativeError, match="workspace too small"):
        order(link=None, nbytes=16)
    # the offsets' one entry past n_links counts: offset and a buffer right behind its n_links entries overlap
    with pytest.raises(_lib.SatMVSNativeError, match="steps aliases offset"):
        write(steps=C.c_void_p(6 * MB + 5 * 4))


# ---- planted errors --------------------------------------------------------------------------------------------------------------
PLANTS = {"m + 1 for any two inflows": (dict(any_two=True), {"order_map", "order"}), "Shreve sums": (dict(shreve=True), {"order_map", "order"}),
          "4-neighbour inflows": (dict(four=True), {"order_map", "link", "head", "next_link", "offset", "vertices", "steps"}),
          "the mask's gaps ignored": (dict(gaps=False), {"order_map", "link", "head", "offset", "vertices"}),
          "heads only where in >= 2": (dict(heads_two=True), {"link", "head", "offset", "vertices"}),
          "the junction vertex left off": (dict(junction=False), {"offset", "vertices"}),
          "links numbered by mouth": (dict(by_mouth=True), {"link", "head", "next_link"}),
          "diagonal steps counted as E-W": (dict(diagonal_ew=True), {"steps"})}


@pytest.mark.parametrize("plant", sorted(PLANTS))
def test_planted_errors_are_reported(plant):
    """The comparison of the GPU file (dsm_stream_oracle.differing over the outputs of network()) reports each planted error on
    the random hills that file runs, and names an entry."""
    switches, expect = PLANTS[plant]
    seen = set()
    for case in so.RANDOM_SCENES[3:5]:
        code, acc = so.hill_codes(*case)
        for name, mask in so.masks_of(code, acc)[:4]:
            good = so.network(code, mask)
            lines = so.differing(so.network(code, mask, arrays=False, **switches), {k: good[k] for k in so.KEYS})
            assert all("[" in line or "want" in line for line in lines)
            seen |= {line.split("[")[0].split(":")[0] for line in lines}
    assert expect <= seen, (plant, seen)
    if plant == "diagonal steps counted as E-W":
        code, _ = so.hill_codes(*so.RANDOM_SCENES[3])
        assert not np.array_equal(so.flow_length_walk(code, diagonal_ew=True)[0], so.flow_length_doubling(code)[0])
