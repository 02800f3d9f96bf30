"""Hydrology without a GPU: the two Python statements of every part of the rule (dsm_hydro_oracle.py) against each other,
the filled surface against a brute-force minimax path, invariants, closed forms, the ESRI table, the argument rejections of
the Python functions and of the C entries, and the planted errors that the GPU file's comparison has to report."""
import ctypes as C

import numpy as np
import pytest

import dsm_hydro_oracle as ho
from dsm_testkit import lib  # noqa: F401  (fixture)


def _scenes():
    for gh, gw, seed, voids, levels in ho.RANDOM_CASES:
        yield ho.hills(gh, gw, seed, voids, levels)
    yield ho.crater(21)
    yield ho.comb(12, 15)
    yield ho.serpentine(11, 14)[0]


# ---- the statement pairs -----------------------------------------------------------------------------------------------------------
def test_the_two_statements_agree():
    rng = np.random.default_rng(0)
    raised = flat = 0
    for z in _scenes():
        w, d, v = ho.keys_heap(z)
        w2, d2, v2 = ho.keys_sweeps(z)
        assert np.array_equal(w, w2) and np.array_equal(d, d2) and np.array_equal(v, v2)
        raised += int((w > ho.quanta(z))[v].sum())
        flat += int((d > 1).sum())
        dist = ho.distances(ho.XRES, ho.YRES)
        code = ho.directions_loop(w, d, v, dist)
        assert np.array_equal(code, ho.directions_arrays(w, d, v, dist))
        assert np.array_equal(ho.receivers(code), ho.receivers_arrays(code))
        weight = rng.integers(-7, 9, z.shape).astype(np.int32)
        for wt in (None, weight):
            by_keys = ho.accumulate_by_keys(code, w, d, wt)
            sub, cyc = ho.accumulate_subtrees(code, wt)
            peel, cyc2 = ho.accumulate_peel(code, wt)
            assert np.array_equal(by_keys, sub) and np.array_equal(sub, peel) and not cyc and not cyc2
        a, b = ho.basins_walk(code), ho.basins_arrays(code)
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:] == (int((code == 0).sum()), False)
        assert np.array_equal(ho.unpack(ho.pack(w, d, v))[0], w) and np.array_equal(ho.unpack(ho.pack(w, d, v))[1], d)
    assert raised > 300 and flat > 100                       # the scenes do have depressions and flats


def test_receivers_and_cycles_on_arbitrary_code_grids():
    rng = np.random.default_rng(1)
    codes = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 9, 254, 255], np.uint8)
    cyclic = 0
    for _ in range(40):
        gh, gw = rng.integers(1, 13, 2)
        code = rng.choice(codes, (gh, gw))
        pour = rng.random((gh, gw)) < 0.1
        wt = rng.integers(-9, 9, (gh, gw)).astype(np.int32)
        for p in (None, pour):
            recv = ho.receivers(code, p)
            assert np.array_equal(recv, ho.receivers_arrays(code, p))
            assert np.array_equal(ho.roots_walk(recv), ho.roots_doubling(recv))
            a, b = ho.basins_walk(code, p), ho.basins_arrays(code, p)
            assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
        sub, c1 = ho.accumulate_subtrees(code, wt)
        peel, c2 = ho.accumulate_peel(code, wt)
        assert np.array_equal(sub, peel) and c1 == c2
        cyclic += c1
    assert cyclic > 5
    # a 2-cycle with a tributary, codes 9 and 254 as voids, a target off the grid and a target on a void as roots
    code = np.array([[1, 5, 255, 3],
                     [7, 0, 9, 254],
                     [1, 1, 7, 8]], np.uint8)
    recv = ho.receivers(code).reshape(3, 4)
    assert recv.tolist() == [[1, 0, ho.VOID, ho.ROOT], [0, ho.ROOT, ho.VOID, ho.VOID], [9, 10, ho.ROOT, ho.ROOT]]
    acc, cyc = ho.accumulate_subtrees(code)
    assert cyc and acc.tolist() == [[-1, -1, 0, 1], [-1, 1, 0, 0], [1, 2, 3, 1]]
    lab, n, cyc = ho.basins_walk(code)
    assert cyc and n == 4 and lab.tolist() == [[0, 0, 0, 1], [0, 2, 0, 0], [3, 3, 3, 4]]


# ---- brute force -------------------------------------------------------------------------------------------------------------------
def test_filled_surface_is_the_minimax_path_to_an_outlet():
    """w(c) = the least, over the 8-connected paths from c to an outlet, of the highest q on the path (Floyd-Warshall on the
    bottleneck semiring)."""
    for seed, (gh, gw), voids, levels in ((0, (12, 12), 0.0, 5), (1, (9, 12), 0.06, 5), (2, (12, 7), 0.0, None), (3, (10, 11), 0.1, 12)):
        z = ho.hills(gh, gw, seed + 40, voids, levels)
        if levels is None:
            z = z - np.float32(7.0) * np.random.default_rng(seed).integers(0, 2, z.shape).astype(np.float32)
        v, q = ho.valid(z), ho.quanta(z)
        n = gh * gw
        big = 2 ** 40
        B = np.full((n, n), big, np.int64)
        for r in range(gh):
            for c in range(gw):
                if not v[r, c]:
                    continue
                B[r * gw + c, r * gw + c] = q[r, c]
                for k in range(8):
                    rr, cc = r + ho.DR[k], c + ho.DC[k]
                    if 0 <= rr < gh and 0 <= cc < gw and v[rr, cc]:
                        B[r * gw + c, rr * gw + cc] = max(q[r, c], q[rr, cc])
        for k in range(n):
            B = np.minimum(B, np.maximum(B[:, k, None], B[None, k, :]))
        out = ho.outlets(v).reshape(-1)
        want = B[:, out].min(axis=1).reshape(gh, gw)
        w, _, _ = ho.keys_heap(z)
        assert np.array_equal(w[v], want[v])


# ---- invariants --------------------------------------------------------------------------------------------------------------------
def test_invariants():
    for z in _scenes():
        gh, gw = z.shape
        w, d, v = ho.keys_heap(z)
        q, out = ho.quanta(z), ho.outlets(v)
        assert (w >= q)[v].all() and np.array_equal(w[out], q[out]) and (d[out] == 0).all() and (d[~v] == -1).all()
        code = ho.directions_loop(w, d, v, ho.distances(ho.XRES, ho.YRES))
        assert np.array_equal(code == 255, ~v) and np.array_equal(code == 0, out)
        pointed = np.zeros((gh, gw), bool)
        for r, c in zip(*np.nonzero(v & ~out)):
            near = [(w[r + ho.DR[k], c + ho.DC[k]], d[r + ho.DR[k], c + ho.DC[k]]) for k in range(8)]
            assert min(near) < (w[r, c], d[r, c])            # every non-outlet has a neighbour with a smaller key
            k = int(code[r, c]) - 1
            assert near[k] < (w[r, c], d[r, c])              # (w, d) falls along every flow step
            if near[k][0] == w[r, c]:
                assert near[k][1] == d[r, c] - 1
            pointed[r + ho.DR[k], c + ho.DC[k]] = True
        acc = ho.accumulate_by_keys(code, w, d)
        assert acc[code == 0].sum() == v.sum()               # everything leaves through a root
        assert np.array_equal(acc == 1, v & ~pointed) and (acc[~v] == 0).all()
        filled, depth, flat = ho.filled_of(z, w, d, v)
        same = v & (w == q)
        assert np.array_equal(filled[same].view(np.uint32), z[same].view(np.uint32)) and (depth[v] >= 0).all()
        assert np.array_equal(filled[~v], np.full((~v).sum(), -999.0, np.float32)) and np.array_equal(flat, d)


# ---- closed forms ------------------------------------------------------------------------------------------------------------------
def test_bowl_with_a_notch_fills_to_the_notch():
    n = 15
    r, c = np.mgrid[:n, :n]
    ring = np.maximum(np.abs(r - n // 2), np.abs(c - n // 2))
    z = (40.0 + ring).astype(np.float32)                     # a bowl ...
    z[ring == n // 2 - 1] = 100.0                            # ... inside a rim one cell in from the edge ...
    z[ring == n // 2] = 0.0                                  # ... which is low ground
    z[n // 2, n - 2] = 53.25                                 # the notch
    w, d, v = ho.keys_heap(z)
    inside = ring < n // 2 - 1
    assert np.array_equal(w[inside], np.maximum(ho.quanta(z)[inside], int(53.25 * 256)))
    filled, depth, _ = ho.filled_of(z, w, d, v)
    assert (w[inside] == int(53.25 * 256)).all()
    assert filled[n // 2, n // 2] == np.float32(53.25) and depth[n // 2, n // 2] == np.float32(13.25) and depth[~inside].max() == 0.0
    assert d[n // 2, n - 2] == 0 and d[n // 2, n - 3] == 1 and d[n // 2, n // 2] == n // 2 - 1


def test_a_tilted_plane_gives_one_code_per_direction():
    gh, gw = 9, 11
    r, c = np.mgrid[:gh, :gw]
    for k in range(8):
        z = (100.0 - 0.5 * (ho.DC[k] * c + ho.DR[k] * r)).astype(np.float32)
        w, d, v = ho.keys_heap(z)
        code = ho.directions_loop(w, d, v, ho.distances(5.0, 5.0))
        assert (code[1:-1, 1:-1] == k + 1).all() and (code[0] == 0).all() and (code[:, -1] == 0).all()
        assert np.array_equal(w, ho.quanta(z)) and (d == 0).all()


def test_a_level_grid_counts_the_steps_to_its_edge():
    gh, gw = 9, 14
    r, c = np.mgrid[:gh, :gw]
    w, d, v = ho.keys_heap(np.full((gh, gw), 7.5, np.float32))
    assert np.array_equal(d, np.minimum(np.minimum(r, gh - 1 - r), np.minimum(c, gw - 1 - c))) and (w == 1920).all()
    z = np.full((gh, gw), 7.5, np.float32)
    z[4, 6] = np.nan                                          # a void is a way out as well
    w, d, v = ho.keys_heap(z)
    want = np.minimum(np.minimum(np.minimum(r, gh - 1 - r), np.minimum(c, gw - 1 - c)), np.maximum(np.abs(r - 4), np.abs(c - 6)) - 1)
    assert np.array_equal(d[v], want[v]) and not v[4, 6]


def test_the_thalweg_of_a_v_valley():
    gh, gw, c0 = 10, 13, 6
    r, c = np.mgrid[:gh, :gw]
    z = (10.0 * np.abs(c - c0) + (gh - 1 - r)).astype(np.float32)
    out = ho.chain(z, 5.0, 5.0)
    code, acc = out["dir"], out["acc"]
    assert (code[1:-1, 1:c0] == 1).all() and (code[1:-1, c0 + 1:-1] == 5).all() and (code[1:-1, c0] == 3).all()
    assert acc[1:-1, c0].tolist() == [(gw - 2) * k for k in range(1, gh - 1)]
    assert acc[gh - 1, c0] == (gw - 2) * (gh - 2) + 1 and out["n"] == 2 * gh + 2 * gw - 4
    assert (out["basin"][1:-1, 1:-1] == out["basin"][gh - 1, c0]).all()


def test_one_cell_wide_grids_are_all_outlets():
    for shape in ((1, 9), (9, 1), (1, 1)):
        z = np.random.default_rng(3).uniform(0, 50, shape).astype(np.float32)
        out = ho.chain(z)
        assert (out["dir"] == 0).all() and (out["acc"] == 1).all() and (out["flat_dist"] == 0).all()
        assert np.array_equal(out["filled"].view(np.uint32), z.view(np.uint32)) and out["n"] == z.size
        assert np.array_equal(out["basin"].reshape(-1), np.arange(1, z.size + 1))


def test_quantisation_and_validity_edges():
    z = np.array([[0.001953125, 0.005859375, -0.0, 0.0, np.nan, np.inf, -np.inf, -999.0, 32768.0, -32768.0,
                   np.nextafter(np.float32(32768.0), np.float32(np.inf)), np.nextafter(np.float32(-32768.0), np.float32(-np.inf))]], np.float32)
    assert ho.valid(z).tolist() == [[True, True, True, True, False, False, False, False, True, True, False, False]]
    assert ho.quanta(z)[0, :4].tolist() == [0, 2, 0, 0] and ho.quanta(z)[0, 8:10].tolist() == [2 ** 23, -2 ** 23]


def test_serpentine_is_one_long_river():
    """The flow follows the channel through every second row; at a turn it cuts the corner cell diagonally (two quanta over a
    diagonal beat one over a side), so the river is shorter than the channel by at most the two corner cells of every turn."""
    gh, gw = 11, 14
    z, path = ho.serpentine(gh, gw)
    out = ho.chain(z, 5.0, 5.0)
    recv = ho.receivers(out["dir"])
    at, steps = path[-1][0] * gw + path[-1][1], 0
    while recv[at] >= 0:
        at, steps = recv[at], steps + 1
    turns = len(range(1, gh - 1, 2)) - 1
    assert (at // gw, at % gw) == path[0] and len(path) - 1 - 2 * turns <= steps <= len(path) - 1
    assert (out["depth"] == 0).all() and out["acc"][path[0]] >= len(path)


# ---- the ESRI table, streams -------------------------------------------------------------------------------------------------------
def test_flow_codes():
    from satmvs_amd import dsm
    assert dsm.flow_codes("index").tolist() == list(range(9)) + [255] * 247
    esri = dsm.flow_codes("esri")
    assert esri.dtype == np.uint8 and esri[:9].tolist() == [0, 1, 2, 4, 8, 16, 32, 64, 128] and (esri[9:] == 255).all()
    with pytest.raises(ValueError, match="encoding"):
        dsm.flow_codes("taudem")
    g = dsm.DSMGrid(0.0, 0.0, 5.0, 2.5, 4, 3)
    assert dsm.flow_distances(g).tolist() == ho.distances(5.0, 2.5) and dsm.flow_distances(g)[1] == np.hypot(5.0, 2.5)
    acc = np.array([[1, 5], [7, -1]], np.int64)
    assert dsm.streams(acc, 5).tolist() == [[False, True], [True, False]]
    with pytest.raises(ValueError, match="finite"):
        dsm.streams(acc, np.nan)
    with pytest.raises(ValueError, match="gh, gw"):
        dsm.streams(acc[0], 1)


# ---- argument rejections, Python ---------------------------------------------------------------------------------------------------
def test_functions_reject_bad_arguments_without_a_gpu():
    from satmvs_amd import dsm
    good = np.zeros((4, 5), np.float32)
    grid = dsm.DSMGrid(0.0, 0.0, 5.0, 2.5, 5, 4)
    huge = np.broadcast_to(np.float32(0), (2 ** 15, 2 ** 15))
    for z, match in ((np.zeros(5, np.float32), "gh, gw"), (np.zeros((0, 5), np.float32), "positive sizes"), (good.astype(np.float64), "float32"),
                     (huge, "2\\^30")):
        with pytest.raises(ValueError, match=match):
            dsm.fill_depressions(z)
        with pytest.raises(ValueError, match=match):
            dsm.depressions(z, grid)
    for batch in (0, 4097, 2.5):
        with pytest.raises(ValueError, match="batch"):
            dsm.fill_depressions(good, batch=batch)
    with pytest.raises(ValueError, match="differs from the grid"):
        dsm.flow_direction(good, dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, 4, 5))
    with pytest.raises(ValueError, match="resolutions"):
        dsm.flow_direction(good, dsm.DSMGrid(0.0, 0.0, 5.0, 0.0, 5, 4))
    with pytest.raises(ValueError, match="encoding"):
        dsm.flow_direction(good, grid, encoding="d-inf")
    codes = np.zeros((4, 5), np.uint8)
    for fn in (dsm.flow_accumulation, dsm.basins):
        for d, match in ((codes.astype(np.int32), "uint8"), (codes[0], "gh, gw"), (np.zeros((0, 5), np.uint8), "positive sizes"),
                         (np.broadcast_to(np.uint8(0), (2 ** 15, 2 ** 15)), "2\\^30")):
            with pytest.raises(ValueError, match=match):
                fn(d)
    with pytest.raises(ValueError, match="cycles"):
        dsm.flow_accumulation(codes, cycles="ignore")
    for w in (np.zeros((4, 5), np.int64), np.zeros((5, 4), np.int32), np.zeros((4, 5), np.float32)):
        with pytest.raises(ValueError, match="weights"):
            dsm.flow_accumulation(codes, weights=w)
    with pytest.raises(ValueError, match="differs from the grid"):
        dsm.flow_accumulation(codes, grid=dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, 4, 5))
    for pour, match in ((np.zeros((4, 5), np.float32), "bool or an integer"), (np.zeros((3, 3), np.uint8), "mask or an"), (np.zeros(4, np.int64), "mask or an"),
                        (np.array([[1.0, 2.0]]), "integers"), (np.array([[4, 0]]), "lie on"), (np.array([[0, 5]]), "lie on"), (np.array([[-1, 0]]), "lie on")):
        with pytest.raises(ValueError, match=match):
            dsm.basins(codes, pour)
    for kw, match in ((dict(min_depth=0.0), "min_depth"), (dict(min_depth=np.nan), "min_depth"), (dict(min_area_m2=-1.0), "min_area_m2")):
        with pytest.raises(ValueError, match=match):
            dsm.depressions(good, grid, **kw)


# ---- argument rejections, C --------------------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_a_gpu(lib):
    from satmvs_amd import _lib
    MB = 1 << 20
    at = lambda i: C.c_void_p(i * MB)                        # noqa: E731  (made-up pointers a megabyte apart: nothing is dereferenced)
    host = lambda a: a.ctypes.data_as(C.c_void_p)            # noqa: E731
    gw, gh = 9, 7
    n = gw * gh
    flood_ws, flow_ws = lib.smvs_dsm_flood_workspace_bytes(gw, gh), lib.smvs_dsm_flow_workspace_bytes(gw, gh)
    assert flood_ws == 4096 * 4 and 56 * n <= flow_ws < 56 * n + 8 * 256 and flow_ws < MB
    for size in (lib.smvs_dsm_flood_workspace_bytes, lib.smvs_dsm_flow_workspace_bytes):
        assert size(0, 5) == 0 and size(5, -1) == 0 and size(2 ** 15, 2 ** 15) == 0 and size(2 ** 15 - 1, 2 ** 15) > 0
    dist = np.array(ho.distances(5.0, 2.5))

    def begin(dsm=at(1), gw=gw, gh=gh, keys=at(2), ws=at(3), nbytes=flood_ws):
        _lib.call("smvs_dsm_flood_begin", dsm, gw, gh, -999.0, keys, ws, nbytes, None)

    def rounds(dsm=at(1), gw=gw, gh=gh, keys=at(2), k=8, status=at(4), ws=at(3), nbytes=flood_ws):
        _lib.call("smvs_dsm_flood_rounds", dsm, gw, gh, -999.0, keys, k, status, ws, nbytes, None)

    def read(dsm=at(1), gw=gw, gh=gh, keys=at(2), filled=at(5), depth=at(6), flat=at(7)):
        _lib.call("smvs_dsm_flood_read", dsm, gw, gh, -999.0, keys, filled, depth, flat, None)

    def flow_dir(keys=at(2), gw=gw, gh=gh, dist=dist, out=at(8)):
        _lib.call("smvs_dsm_flow_dir", keys, gw, gh, None if dist is None else host(dist), out, None)

    def accumulate(code=at(8), weight=at(9), gw=gw, gh=gh, acc=at(10), flag=at(11), ws=at(12), nbytes=flow_ws):
        _lib.call("smvs_dsm_flow_accumulate", code, weight, gw, gh, acc, flag, ws, nbytes, None)

    def basins(code=at(8), pour=at(9), gw=gw, gh=gh, basin=at(10), n_out=at(13), flag=at(11), ws=at(12), nbytes=flow_ws):
        _lib.call("smvs_dsm_flow_basins", code, pour, gw, gh, basin, n_out, flag, ws, nbytes, None)

    grids = [(dict(gw=0), "non-positive grid"), (dict(gh=-2), "non-positive grid"), (dict(gw=2 ** 15, gh=2 ** 15), "below 2\\^30")]
    bad = [(fn, kw, match) for fn in (begin, rounds, read, flow_dir, accumulate, basins) for kw, match in grids]
    for fn in (begin, rounds):
        bad += [(fn, dict(dsm=None), "null pointer"), (fn, dict(keys=None), "null pointer"), (fn, dict(ws=None), "null pointer"),
                (fn, dict(nbytes=flood_ws - 1), "workspace too small"), (fn, dict(keys=at(1)), "keys aliases dsm"), (fn, dict(ws=at(2)), "workspace aliases keys"),
                (fn, dict(ws=at(1)), "workspace aliases dsm")]
    bad += [(rounds, dict(status=None), "null pointer"), (rounds, dict(k=0), "rounds must be"), (rounds, dict(k=4097), "rounds must be"),
            (rounds, dict(status=at(2)), "status aliases keys"), (rounds, dict(ws=at(4)), "workspace aliases status"),
            (read, dict(dsm=None), "null pointer"), (read, dict(keys=None), "null pointer"), (read, dict(filled=at(1)), "filled aliases dsm"),
            (read, dict(depth=at(5)), "depth aliases filled"), (read, dict(flat=at(2)), "flat_dist aliases keys"), (read, dict(flat=at(6)), "flat_dist aliases depth"),
            (flow_dir, dict(keys=None), "null pointer"), (flow_dir, dict(dist=None), "null pointer"), (flow_dir, dict(out=None), "null pointer"),
            (flow_dir, dict(out=at(2)), "dir aliases keys")]
    for k in range(8):
        for value in (0.0, -5.0, np.nan, np.inf):
            wrong = dist.copy()
            wrong[k] = value
            bad.append((flow_dir, dict(dist=wrong), "dist\\[%d\\]" % k))
    for fn, out in ((accumulate, "acc"), (basins, "basin")):
        bad += [(fn, dict(code=None), "null pointer"), (fn, {out: None}, "null pointer"), (fn, dict(flag=None), "null pointer"), (fn, dict(ws=None), "null pointer"),
                (fn, dict(nbytes=flow_ws - 1), "workspace too small"), (fn, {out: at(8)}, out + " aliases dir"), (fn, dict(flag=at(10)), "flag aliases " + out),
                (fn, dict(ws=at(8)), "workspace aliases dir"), (fn, dict(ws=at(11)), "workspace aliases flag")]
    bad += [(accumulate, dict(weight=at(8)), "weight aliases dir"), (accumulate, dict(acc=at(9)), "acc aliases weight"),
            (basins, dict(pour=at(8)), "pour aliases dir"), (basins, dict(n_out=None), "null pointer"), (basins, dict(n_out=at(10)), "n_out aliases basin"),
            (basins, dict(flag=at(13)), "flag aliases n_out")]
    for fn, kw, match in bad:
        with pytest.raises(_lib.SatMVSNativeError, match=match):
            fn(**kw)
    # what may be null is null without complaint up to the first HIP call, which these made-up pointers must not reach: the
    # checks that come last (the workspace size) still fire
    with pytest.raises(_lib.SatMVSNativeError, match="workspace too small"):
        accumulate(weight=None, nbytes=16)
    with pytest.raises(_lib.SatMVSNativeError, match="workspace too small"):
        basins(pour=None, nbytes=16)


# ---- planted errors ----------------------------------------------------------------------------------------------------------------
PLANTS = {"4-neighbour flood": dict(neighbours=4), "d not reset on a rise": dict(reset_d=False), "smallest w, not steepest slope": dict(steepest=False),
          "ties to the highest k": dict(low_ties=False), "diagonal distance 1": dict(diagonal=1.0), "voids as walls": dict(void_outlets=False),
          "accumulation without the cell itself": dict(own=False)}


@pytest.mark.parametrize("plant", sorted(PLANTS))
def test_planted_errors_are_reported(plant):
    """The comparison of the GPU file (dsm_hydro_oracle.differing over the outputs of chain()) reports each planted error on
    the random hills that file runs."""
    seen = set()
    for gh, gw, seed, voids, levels in ho.RANDOM_CASES[3:5]:
        z = ho.hills(gh, gw, seed, voids, levels)
        good = ho.chain(z, ho.XRES, ho.YRES)
        assert ho.differing(ho.chain(z, ho.XRES, ho.YRES), good) == []
        seen |= set(ho.differing(ho.chain(z, ho.XRES, ho.YRES, **PLANTS[plant]), good))
    expect = {"4-neighbour flood": {"keys", "filled", "depth", "dir", "acc"}, "d not reset on a rise": {"keys", "flat_dist"}, "voids as walls": {"keys", "filled", "dir"},
              "accumulation without the cell itself": {"acc"}}.get(plant, {"dir", "acc"})
    assert expect <= seen, (plant, seen)
