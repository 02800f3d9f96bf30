"""Cost distance without a device: the two Python statements of the rule (tests/dsm_cost_oracle.py) against each other on every
scene, the invariants and closed forms of the rule, the host helpers of satmvs_amd.dsm, every argument rejection of the Python
layer and of the C entries, and the eight planted errors as the GPU file's comparison reports them."""
import ctypes as C

import numpy as np
import pytest

import dsm_cost_oracle as co
import dsm_hydro_oracle as ho
from dsm_testkit import lib                                  # noqa: F401

L = co.lengths(co.XRES, co.YRES)


def _grid(gh, gw, xres=co.XRES, yres=co.YRES):
    from satmvs_amd import dsm
    return dsm.DSMGrid(500000.0, 4000000.0, xres, yres, gw, gh)


@pytest.fixture(scope="module", autouse=True)
def rule():
    """The statements speak of the package's rule: its step lengths and its walking table are the oracle's, integer for integer."""
    from satmvs_amd import dsm
    assert dsm.cost_terms(_grid(7, 9)).tolist() == L and dsm.cost_terms(_grid(7, 9)).dtype == np.int32
    assert np.array_equal(dsm.tobler_table(), co.TABLE) and dsm.tobler_table().dtype == np.int32


_chains = {}


def _chain(case, arrays=False):
    """chain() of a scene case, computed once and shared (read-only)."""
    key = (case, arrays)
    if key not in _chains:
        _chains[key] = (co.case(*case), None)
        _chains[key] = (_chains[key][0], co.chain(L=L, arrays=arrays, **_chains[key][0]))
    return _chains[key]


# ---- the statements against each other ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", co.SCENE_CASES + co.GRID_CASES, ids=co.case_id)
def test_the_two_statements_agree(case):
    args, loop = _chain(case)
    arrays = co.chain(L=L, arrays=True, **args)
    assert co.differing(loop, arrays) == []
    assert loop["keys"].dtype == np.uint64 and loop["raw"].dtype == np.int64 and loop["cost"].dtype == np.float64 and loop["backlink"].dtype == np.uint8


def test_the_scenes_hold_what_they_are_for():
    """Barriers, unreachable cells, forbidden steps and ties all occur, so that no branch of the rule goes unvisited."""
    seen = dict(barrier=0, unreached=0, tie=0, forbidden=0)
    for case in co.SCENE_CASES:
        args, want = _chain(case)
        gh, gw = want["keys"].shape
        seen["barrier"] += int((want["keys"] == co.BARRIER).sum())
        seen["unreached"] += int((want["keys"] == co.INF).sum())
        hi = co.backlinks_loop(want["keys"], L, args["friction"], args["z"], args["table"], args["reverse"], low_ties=False)
        seen["tie"] += int((hi != want["backlink"]).sum())
        W = co.step_costs(gh, gw, L, args["friction"], args["z"], args["table"], args["reverse"])
        ok = co.passable(gh, gw, args["friction"], args["z"])
        seen["forbidden"] += int(((W[0] < 0) & ok & np.roll(ok, -1, axis=1))[:, :-1].sum()) if args["table"] is not None else 0
    assert all(v > 0 for v in seen.values()), seen
    args, tiny = co.tiny_case()
    assert tiny == [1, 2, 2, 2, 1, 2, 2, 2]
    W = co.step_costs(*args["src"].shape, tiny, args["friction"])
    x = (args["friction"][:, :-1].astype(int) + args["friction"][:, 1:]) * 256 >> 10
    assert (W[0][:, :-1][x == 0] == np.where((args["friction"][:, :-1] != 0) & (args["friction"][:, 1:] != 0), 1, -1)[x == 0]).all() and (x == 0).sum() > 20
    assert co.differing(co.chain(L=tiny, **args), co.chain(L=tiny, arrays=True, **args)) == []


# ---- invariants --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", co.SCENE_CASES, ids=co.case_id)
def test_invariants_of_the_surface(case):
    args, want = _chain(case)
    keys, link = want["keys"], want["backlink"]
    gh, gw = keys.shape
    ok = co.passable(gh, gw, args["friction"], args["z"])
    assert np.array_equal(keys == 0, (args["src"] != 0) & ok)                       # D = 0 exactly at the passable sources
    assert np.array_equal(link == 0, keys == 0) and np.array_equal(link == 255, keys >= co.INF)
    W = co.step_costs(gh, gw, L, args["friction"], args["z"], args["table"], args["reverse"])
    for r, c in np.argwhere((link >= 1) & (link <= 8)):
        k = int(link[r, c]) - 1
        rr, cc = r + co.DR[k], c + co.DC[k]
        assert W[k, r, c] >= 1 and int(keys[r, c]) - int(keys[rr, cc]) == int(W[k, r, c])      # D falls by exactly w along a back-link
    reached = np.argwhere(keys < co.INF)
    for r, c in reached[:: max(1, len(reached) // 60)]:                             # every finite cell reaches a source
        cells, codes = co.walk(link, int(r), int(c))
        assert keys[cells[-1]] == 0 and sum(int(W[k][cell]) for k, cell in zip(codes, cells)) == int(keys[r, c])


def test_raising_one_friction_value_never_lowers_any_cost():
    args, want = _chain(co.SCENE_CASES[1])
    rng = np.random.default_rng(5)
    for _ in range(4):
        f = args["friction"].copy()
        r, c = rng.integers(0, f.shape[0]), rng.integers(0, f.shape[1])
        f[r, c] = min(65535, int(f[r, c]) * 3 + 1) if f[r, c] else 0
        keys = co.keys_sweeps(args["src"], L, f)
        assert (keys >= want["keys"]).all()


def test_symmetry_without_a_table_and_under_reverse():
    """Without a table w(c -> n) = w(n -> c), so D from A at B is D from B at A.  With one, the plain run from A prices at B
    the trip B -> A with every step's slope read in the direction of travel; the run from B with reverse prices at A the trip
    away from B, which is the same trip B -> A: the two numbers are equal, and reverse is not a no-op."""
    gh, gw = 23, 29
    z = ho.hills(gh, gw, 11, 0.05, 12)
    f = co.friction_of(gh, gw, 11, 12)
    ok = co.passable(gh, gw, f, z)
    cells = np.argwhere(ok)
    (ra, ca), (rb, cb) = cells[7], cells[-9]
    a, b = np.zeros((gh, gw), np.uint8), np.zeros((gh, gw), np.uint8)
    a[ra, ca], b[rb, cb] = 1, 1
    fb = f.copy()
    fb[~ok] = 0                                               # the same barriers without the DSM
    assert co.keys_heap(a, L, fb)[rb, cb] == co.keys_heap(b, L, fb)[ra, ca] < co.INF
    plain = co.keys_heap(a, L, f, z, co.TABLE)                # D(c): from c towards A
    back = co.keys_heap(b, L, f, z, co.TABLE, reverse=True)   # D(c): from B towards c
    assert plain[rb, cb] == back[ra, ca]
    assert any(co.keys_heap(a, L, f, z, co.TABLE)[r, c] != co.keys_heap(a, L, f, z, co.TABLE, reverse=True)[r, c] for r, c in cells[::17])


# ---- closed forms --------------------------------------------------------------------------------------------------------------------
def test_octile_distance_on_a_uniform_grid():
    gh, gw = 19, 27
    src = np.zeros((gh, gw), np.uint8)
    src[4, 20] = 1
    for f in (None, np.full((gh, gw), 256, np.uint16), np.full((gh, gw), 1000, np.uint16)):
        want = co.octile(gh, gw, 4, 20, L, 256 if f is None else 1000 if f[0, 0] == 1000 else 256)
        got = co.chain(src, L, f)
        assert np.array_equal(got["raw"], want) and np.array_equal(got["cost"], want / 32768.0)
    assert want[4, 21] == (2000 * 1280 * 256) >> 10 and L == [1280, 1431, 640, 1431, 1280, 1431, 640, 1431]


def test_a_wall_with_one_gap():
    gh, gw = 9, 11
    f = np.full((gh, gw), 256, np.uint16)
    f[:, 5] = 0
    f[7, 5] = 256
    src = np.zeros((gh, gw), np.uint8)
    src[1, 2] = 1
    got = co.chain(src, L, f)
    wx, wd, wy = 128 * L[0], 128 * L[1], 128 * L[2]
    through = co.octile(gh, gw, 1, 2, L)[7, 5]
    assert got["raw"][7, 5] == through == 3 * wd + 3 * wy
    assert got["raw"][1, 8] == through + co.octile(gh, gw, 7, 5, L)[1, 8]            # every trip to the far side passes the gap
    cells, _ = co.walk(got["backlink"], 1, 8)
    assert (7, 5) in cells and (got["backlink"][:, 5] == 255).sum() == gh - 1 and np.isnan(got["cost"][0, 5])
    f[7, 5] = 0
    shut = co.chain(src, L, f)
    assert (shut["raw"][:, 6:] == -1).all() and np.isposinf(shut["cost"][:, 6:]).all() and (shut["backlink"][:, 6:] == 255).all()


def test_one_row_and_one_column():
    for shape, k in (((1, 9), 0), ((9, 1), 2)):
        src = np.zeros(shape, np.uint8)
        src.flat[2] = 1
        got = co.chain(src, L)
        assert got["raw"].reshape(-1).tolist() == [128 * L[k] * abs(i - 2) for i in range(9)]
        assert got["backlink"].reshape(-1).tolist() == [k + 1] * 2 + [0] + [k + 5] * 6


def test_a_table_that_allows_level_steps_only():
    table = np.zeros(256, np.int32)
    table[128] = 256                                          # 0 <= tan < 1 / 32
    z = np.full((6, 8), 50.0, np.float32)
    z[:, 4:] = 50.0 + 1.0 / 256                               # one quantum up: still bin 128 going up, bin 127 going down
    z[3:, :] = 70.0
    src = np.zeros((6, 8), np.uint8)
    src[0, 0] = 1
    up = co.chain(src, L, None, z, table, reverse=True)       # from the source: onto the raised half, never back, never to 70 m
    assert (up["raw"][:3] >= 0).all() and (up["raw"][3:] == -1).all()
    down = co.chain(src, L, None, z, table)                   # towards the source: the raised half would have to step down
    assert (down["raw"][:3, :4] >= 0).all() and (down["raw"][:3, 4:] == -1).all()
    assert np.array_equal(up["raw"][:3, :4], co.octile(6, 8, 0, 0, L)[:3, :4])


def test_a_cliff_table():
    table = co.slope_table(lambda t: 1.0 if abs(t) < 1.0 else 0.0)
    z = np.zeros((5, 9), np.float32)
    z[:, 5:] = 30.0                                           # a 30 m cliff over 5 m: no way up or down
    src = np.zeros((5, 9), np.uint8)
    src[2, 0] = 1
    got = co.chain(src, L, None, z, table)
    assert (got["raw"][:, :5] >= 0).all() and (got["raw"][:, 5:] == -1).all()
    ramp = z.copy()
    ramp[0, 1:5] = [6.0, 12.0, 18.0, 24.0]                    # 6 m per 5 m east: tan 1.2 along the row and more towards row 1
    assert (co.chain(src, L, None, ramp, table)["raw"][:, 5:] == -1).all()
    ramp[0, 1:5] = [4.0, 8.0, 12.0, 16.0]                     # tan 0.8 along the row, and 16 -> 30 is a cliff still
    assert (co.chain(src, L, None, ramp, table)["raw"][:, 5:] == -1).all()
    ramp[0, 5:8] = [20.0, 24.0, 28.0]                         # the ramp goes on to the top
    assert (co.chain(src, L, None, ramp, table)["raw"][:, 5:] >= 0).all()


def test_the_floor_of_one_unit_a_step():
    """Friction 1 on cells of 2^-8 m: (1 + 1) 1 256 >> 10 = 0, so every step costs the floor, 1, and D is the Chebyshev distance."""
    tiny = co.lengths(2.0 ** -8, 2.0 ** -8)
    assert tiny == [1] * 8
    f = np.ones((7, 9), np.uint16)
    src = np.zeros((7, 9), np.uint8)
    src[3, 4] = 1
    got = co.chain(src, tiny, f)
    assert np.array_equal(got["raw"], np.maximum(np.abs(np.arange(7) - 3)[:, None], np.abs(np.arange(9) - 4)[None, :]))
    assert np.array_equal(got["cost"], got["raw"] / 32768.0)
    # ties to the lowest k: SW (3) before W (4) and NW (5); SE (1) before S (2) and SW (3); in the corner's line SW alone is nearer
    assert got["backlink"][3, 8] == 4 and got["backlink"][0, 4] == 2 and got["backlink"][0, 7] == 4


def test_max_cost_cuts_at_a_cell_and_keeps_the_forest_closed():
    args, want = _chain(co.SCENE_CASES[1])
    keys = want["keys"]
    r, c = np.argwhere((keys > 0) & (keys < co.INF))[123]
    d = int(keys[r, c])
    at = co.chain(L=L, max_cost=d, **args)
    below = co.chain(L=L, max_cost=d - 1, **args)
    assert at["raw"][r, c] == d and at["backlink"][r, c] == want["backlink"][r, c]
    assert below["raw"][r, c] == -1 and below["backlink"][r, c] == 255 and np.isposinf(below["cost"][r, c])
    for out in (at, below):
        for rr, cc in np.argwhere((out["backlink"] >= 1) & (out["backlink"] <= 8)):
            k = int(out["backlink"][rr, cc]) - 1
            assert out["backlink"][rr + co.DR[k], cc + co.DC[k]] <= 8


# ---- the host helpers ----------------------------------------------------------------------------------------------------------------
def test_tables_and_quantisation_helpers():
    from satmvs_amd import dsm
    t = dsm.tobler_table().astype(np.int64)
    low = 126                                                 # the bin of tan in [-2/32, -1/32), where walking is quickest
    assert t.argmax() != low and t[t > 0].min() == t[low] and t[128] == int(np.rint(256 * co.tobler(0.5 / 32)))
    live = np.flatnonzero(t)
    assert live.min() > 0 and live.max() < 255 and np.array_equal(live, np.arange(live.min(), live.max() + 1))     # forbidden beyond both ends only
    assert (np.diff(t[low:live.max() + 1]) > 0).all() and (np.diff(t[live.min():low + 1]) < 0).all()     # monotone away from the quickest slope
    lin = dsm.slope_table(lambda s: 1.0 + abs(s))
    assert np.array_equal(lin, co.slope_table(lambda s: 1.0 + abs(s))) and (np.diff(lin[128:]) > 0).all() and (np.diff(lin[:128]) < 0).all()
    assert lin[128] == int(np.rint(256 * (1 + 0.5 / 32))) and lin[0] == int(np.rint(256 * (1 + 127.5 / 32)))
    odd = dsm.slope_table(lambda s: float("nan") if s > 3 else -1.0 if s < -3 else float("inf") if s > 2 else 1e-9 if s < -2 else 1.0)
    assert set(odd[:64 - 32].tolist()) == {0} and odd[128] == 256 and odd[255] == 0 and odd[128 + 80] == 0 and odd[128 - 80] == 0
    with pytest.raises(ValueError, match="above 65535 / 256"):
        dsm.slope_table(lambda s: 256.0)
    assert dsm.slope_table(lambda s: 65535 / 256.0).tolist() == [65535] * 256
    f = np.array([[0.0, 1.0, 0.5, -2.0], [np.nan, np.inf, -999.0, 255.99], [1 / 512, 0.0019, 1.001953125, 1.005859375]])
    want = np.array([[0, 256, 128, 0], [0, 0, 0, 65533], [0, 0, 256, 258]], np.uint16)      # halves to even: 0.5 -> 0, 256.5 -> 256, 257.5 -> 258
    for dtype in (np.float64, np.float32):
        got = dsm.quantise_friction(f.astype(dtype))
        assert got.dtype == np.uint16 and np.array_equal(got, co.quantise_friction(f.astype(dtype)))
    assert np.array_equal(dsm.quantise_friction(f), want)
    import torch
    assert np.array_equal(dsm.quantise_friction(torch.from_numpy(f)).numpy(), want)
    with pytest.raises(ValueError, match="does not fit"):
        dsm.quantise_friction(np.array([[256.0]]))
    with pytest.raises(ValueError, match="float dtype"):
        dsm.quantise_friction(np.ones((2, 2), np.int32))
    assert dsm.cost_terms(_grid(3, 3, 2.0 ** -8, 90.0)).tolist() == [1, 23040, 23040, 23040, 1, 23040, 23040, 23040]
    for xres, yres in ((2.0 ** -10, 1.0), (100.0, 100.0), (1.0, 128.0)):
        with pytest.raises(ValueError, match="step lengths"):
            dsm.cost_terms(_grid(3, 3, xres, yres))
    assert dsm._max_cost_units(None) == dsm._max_cost_units(float("inf")) == 2 ** 64 - 1 and dsm._max_cost_units(1.5) == 49152
    assert dsm._max_cost_units(12345 / 32768.0) == 12345 and dsm._max_cost_units(0) == 0


def test_python_rejections_need_no_device():
    from satmvs_amd import dsm
    gh, gw = 6, 7
    grid = _grid(gh, gw)
    src = np.zeros((gh, gw), np.uint8)
    src[2, 3] = 1
    f = np.full((gh, gw), 256, np.uint16)
    z = np.zeros((gh, gw), np.float32)
    bad = [dict(friction=f.astype(np.float32)), dict(friction=f[:-1]), dict(friction=f.astype(np.int32)), dict(dsm=z), dict(vertical=co.TABLE),
           dict(dsm=z.astype(np.float64), vertical=co.TABLE), dict(dsm=z[:, :-1], vertical=co.TABLE), dict(dsm=z, vertical=co.TABLE[:-1]),
           dict(dsm=z, vertical=co.TABLE.astype(np.float64)), dict(dsm=z, vertical=co.TABLE - 1), dict(dsm=z, vertical=co.TABLE + 65535),
           dict(max_cost=-1.0), dict(max_cost=float("nan")), dict(batch=0), dict(batch=4097)]
    for kw in bad:
        with pytest.raises(ValueError):
            dsm.cost_distance(src, grid, **kw)
    for sources in (src[:-1], src.astype(np.float32), [(0, gw)], [(-1, 0)], [(0.5, 1.0)], np.zeros((3, 3), np.uint8)):
        with pytest.raises(ValueError):
            dsm.cost_distance(sources, grid)
    with pytest.raises(ValueError, match="2\\^24 cells"):
        dsm.cost_distance([(0, 0)], _grid(1, 2 ** 24 + 1))
    with pytest.raises(ValueError, match="step lengths"):
        dsm.cost_distance(src, _grid(gh, gw, 200.0, 200.0))
    link = np.zeros((gh, gw), np.uint8)
    for kw in (dict(targets=src[:-1]), dict(targets=[(gh, 0)]), dict(targets=src, raw=np.zeros((gh, gw), np.int32)), dict(targets=src, grid=_grid(gh, gw + 1))):
        with pytest.raises(ValueError):
            dsm.least_cost_paths(link, **kw)
    with pytest.raises(ValueError):
        dsm.least_cost_paths(link.astype(np.int32), src)
    with pytest.raises(ValueError):
        dsm.cost_allocation(link.astype(np.int32))


def test_native_rejections_need_no_device(lib):              # noqa: F811
    """SMVS_ERR_ARG before any HIP call: made-up pointers a megabyte apart, nothing is dereferenced but the HOST arrays."""
    from satmvs_amd import _lib
    MB = 1 << 20
    at = lambda i: C.c_void_p(i * MB)                        # noqa: E731
    gw, gh = 9, 7
    n = gw * gh
    size = lib.smvs_dsm_cost_workspace_bytes
    ws_bytes = size(gw, gh)
    assert ws_bytes == 4096 * 4 + 1024 + 256 and size(4096, 4096) == 4096 * 4 + 1024 + 4 * 65536
    assert size(0, 5) == 0 and size(5, -1) == 0 and size(4096, 4097) == 0 and size(2 ** 24 + 1, 1) == 0 and size(2 ** 24, 1) > 0 and size(2 ** 16, 2 ** 16) == 0
    Lh = np.array(co.lengths(5.0, 2.5), np.int32)
    table = co.TABLE.copy()
    host = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)          # noqa: E731

    def begin(friction=at(1), sources=at(2), dsm=at(3), gw=gw, gh=gh, keys=at(4), count=at(5), ws=at(6), nbytes=ws_bytes):
        _lib.call("smvs_dsm_cost_begin", friction, sources, dsm, gw, gh, -999.0, keys, count, ws, nbytes, None)

    def rounds(friction=at(1), dsm=at(3), gw=gw, gh=gh, L=Lh, table=table, reverse=0, keys=at(4), k=8, status=at(5), ws=at(6), nbytes=ws_bytes):
        _lib.call("smvs_dsm_cost_rounds", friction, dsm, gw, gh, -999.0, host(L), host(table), reverse, keys, k, status, ws, nbytes, None)

    def read(friction=at(1), dsm=at(3), gw=gw, gh=gh, L=Lh, table=table, reverse=0, keys=at(4), raw=at(7), cost=at(8), link=at(9), ws=at(6), nbytes=ws_bytes):
        _lib.call("smvs_dsm_cost_read", friction, dsm, gw, gh, -999.0, host(L), host(table), reverse, keys, 2 ** 64 - 1, raw, cost, link, ws, nbytes, None)

    def rejected(call, match, **kw):
        with pytest.raises(_lib.SatMVSNativeError, match=match):
            call(**kw)

    for name in ("sources", "keys", "count", "ws"):
        rejected(begin, "null pointer", **{name: None})
    for name in ("keys", "status", "ws", "L"):
        rejected(rounds, "null pointer", **{name: None})
    for name in ("keys", "ws", "L"):
        rejected(read, "null pointer", **{name: None})
    for call in (begin, rounds, read):
        rejected(call, "non-positive grid", gw=0)
        rejected(call, "non-positive grid", gh=-3)
        rejected(call, "at most 2\\^24", gw=2 ** 24 + 1, gh=1)
        rejected(call, "at most 2\\^24", gw=4097, gh=4096)
        rejected(call, "workspace too small", nbytes=ws_bytes - 1)
        rejected(call, "aliases", keys=at(1))                # the keys on the friction
        rejected(call, "workspace aliases", ws=C.c_void_p(4 * MB + n * 8 - 1))
    rejected(begin, "aliases", count=C.c_void_p(2 * MB + n - 1))
    rejected(begin, "aliases", dsm=C.c_void_p(1 * MB + 2 * n - 1))
    rejected(rounds, "aliases", status=C.c_void_p(4 * MB + 8))
    rejected(read, "aliases", raw=at(8))
    rejected(read, "aliases", link=C.c_void_p(8 * MB + n * 8 - 1))
    for k in (0, -1, 4097):
        rejected(rounds, "rounds must be in 1 .. 4096", k=k)
    for call in (rounds, read):
        rejected(call, "go together", dsm=None)
        rejected(call, "go together", table=None)
        rejected(call, "reverse must be 0 or 1", reverse=2)
        for k, v in ((0, 0), (3, 32768), (7, -5)):
            bad = Lh.copy()
            bad[k] = v
            rejected(call, "L\\[%d\\] must be in 1 .. 32767" % k, L=bad)
        for b, v in ((0, -1), (255, 65536)):
            bad = table.copy()
            bad[b] = v
            rejected(call, "table\\[%d\\] must be in 0 .. 65535" % b, table=bad)
    # what is allowed to be null is
    for call, kw in ((begin, dict(friction=None, dsm=None)), (rounds, dict(friction=None, dsm=None, table=None)), (read, dict(raw=None, cost=None, link=None))):
        rejected(call, "workspace too small", nbytes=0, **kw)


# ---- the planted errors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(co.PLANTED))
def test_the_comparison_reports_a_planted_error(name):
    """differing(), the comparison of the GPU file, with a wrong implementation standing in for the device: it names the output
    and the first cell that differs, on at least one of the scenes both files run."""
    found = []
    scenes = [_chain(case) + (L, co.XRES, co.YRES) for case in co.SCENE_CASES]
    args, tiny = co.tiny_case()
    scenes.insert(0, (args, co.chain(L=tiny, **args), tiny, co.TINY_XRES, co.TINY_YRES))
    for args, want, lengths, xres, yres in scenes:
        if co.PLANTED[name] == "diagonal":
            wrong = co.chain(L=co.lengths(xres, yres, diagonal=xres), **args)
        else:
            wrong = co.chain(L=lengths, **args, **co.PLANTED[name])
        found += co.differing(wrong, want)
        if found:
            break
    assert found and all(" at cell (" in line and "got" in line and "want" in line for line in found), (name, found)
    assert co.differing(want, want) == []
