"""Cost distance on the device against the Python statements of the rule (tests/dsm_cost_oracle.py): every compared array by
np.array_equal, the float64 cost by its bits, no cell excused.  The grids round the tile size, the scenes with their barriers,
ties, cliffs and unreachable cells, the sources, the serpentine corridor, the limits, the calling conditions of the C entries
(batching, guard words, workspaces full of anything, a side stream, null outputs, rejections that write nothing) and the chain
extract_dtm -> friction -> cost_distance -> cost_allocation -> least_cost_paths -> write_streams."""
import ctypes
import json
import time

import numpy as np
import pytest
import torch

import dsm_cost_oracle as co
from dsm_testkit import dev, lib, scene as kit_scene         # noqa: F401

pytestmark = pytest.mark.gpu

L = co.lengths(co.XRES, co.YRES)
OUT = ("raw", "cost", "backlink")


def _grid(gh, gw, xres=co.XRES, yres=co.YRES):
    from satmvs_amd import dsm
    return dsm.DSMGrid(400000.0, 3500000.0, xres, yres, gw, gh)


def _device(args, xres=co.XRES, yres=co.YRES, **kw):
    """cost_distance() of a scene's arguments under the oracle's names; numpy in, numpy out."""
    from satmvs_amd import dsm
    gh, gw = args["src"].shape
    cost, link, raw, rounds = dsm.cost_distance(args["src"], _grid(gh, gw, xres, yres), args["friction"], args["z"], args["table"], args["reverse"],
                                                return_raw=True, return_rounds=True, **kw)
    assert all(isinstance(t, np.ndarray) for t in (cost, link, raw)) and 1 <= rounds <= gh * gw + 2 + 4096
    return {"raw": raw, "cost": cost, "backlink": link, "rounds": rounds}


def _want(chain):
    return {k: chain[k] for k in OUT}


_shared = {}


def _reference(case):
    """The arguments and the loop statements' outputs of a scene case, computed once and left alone."""
    if case not in _shared:
        args = co.case(*case)
        _shared[case] = (args, co.chain(L=L, **args))
    return _shared[case]


# ---- grids and scenes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", co.GRID_CASES + co.LARGE_CASES + co.SCENE_CASES, ids=co.case_id)
def test_grids_and_scenes_against_the_statements(dev, case):  # noqa: F811
    args, want = _reference(case)
    assert co.differing(_device(args), _want(want)) == []


def test_the_floor_of_one_unit_on_tiny_cells(dev):           # noqa: F811
    args, tiny = co.tiny_case()
    assert co.differing(_device(args, co.TINY_XRES, co.TINY_YRES), _want(co.chain(L=tiny, **args))) == []


# ---- sources ---------------------------------------------------------------------------------------------------------------------
def test_sources_none_on_a_barrier_and_walled_in(dev):       # noqa: F811
    from satmvs_amd import dsm
    gh, gw = 35, 41
    f = np.full((gh, gw), 256, np.uint16)
    f[10:13, 10:13] = 0
    f[11, 11] = 300                                           # a passable cell walled in by barriers
    f[30, 5] = 0
    grid = _grid(gh, gw)
    src = np.zeros((gh, gw), np.uint8)
    src[30, 5] = 1                                            # on a barrier: no source
    with pytest.raises(ValueError, match="no passable source"):
        dsm.cost_distance(src, grid, f)
    with pytest.raises(ValueError, match="no passable source"):
        dsm.cost_distance(np.zeros((gh, gw), bool), grid, f)
    with pytest.raises(ValueError, match="no passable source"):
        dsm.cost_distance(np.zeros((0, 2), np.int64), grid)
    src[11, 11] = 1                                           # walled in: it reaches nothing and nothing reaches it
    alone = _device(dict(src=src, friction=f, z=None, table=None, reverse=False))
    assert co.differing(alone, _want(co.chain(src, L, f))) == []
    assert (alone["raw"] >= 0).sum() == 1 and alone["backlink"][11, 11] == 0 and alone["backlink"][30, 5] == 255
    src[3, 37] = 1
    both = _device(dict(src=src, friction=f, z=None, table=None, reverse=False))
    assert co.differing(both, _want(co.chain(src, L, f))) == []
    listed = dsm.cost_distance([(30, 5), (11, 11), (3, 37)], grid, f, return_raw=True)       # the same sources as a list
    assert np.array_equal(listed[2], both["raw"]) and np.array_equal(listed[1], both["backlink"])
    labels, n = dsm.cost_allocation(both["backlink"])
    assert n == 2 and labels[11, 11] == 2 and labels[3, 37] == 1 and (labels[both["raw"] < 0] == 0).all() and ((labels == 1) == ((both["raw"] >= 0) & (labels != 2))).all()


# ---- the serpentine ----------------------------------------------------------------------------------------------------------------
def test_serpentine_corridor(dev):                           # noqa: F811
    """One corridor through every second row of 257 x 301: the longest path, the most rounds.  Rounds and time are printed (they
    go into profiles/dsm_cost_bench.json through tools/bench_dsm_cost.py), not asserted beyond the bound on the rounds."""
    gh, gw = 257, 301
    f, src, path = co.serpentine(gh, gw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = _device(dict(src=src, friction=f, z=None, table=None, reverse=False))
    seconds = time.perf_counter() - t0
    print("serpentine %d x %d: %d cells in the corridor, %d rounds, %.3f s" % (gh, gw, len(path), got["rounds"], seconds))
    want = co.chain(src, L, f)
    assert co.differing(got, _want(want)) == []
    along = [int(got["raw"][cell]) for cell in path]         # the trip cuts the corners of the turns, and costs more cell after cell
    assert along[0] == 0 and all(a < b for a, b in zip(along, along[1:])) and along[-1] < 128 * L[0] * len(path)
    assert len(co.walk(got["backlink"], *path[-1])[0]) > len(path) - 2 * gh
    assert got["rounds"] <= gh * gw + 2 + 4096


# ---- limits ----------------------------------------------------------------------------------------------------------------------
def test_a_grid_above_2_22_cells_against_the_octile_form(dev):   # noqa: F811
    """2300 x 2300 uniform cells, above 2^22 and below the 2^24 limit, against the closed form evaluated on the device."""
    from satmvs_amd import dsm
    n, r0, c0 = 2300, 700, 1900
    src = torch.zeros((n, n), dtype=torch.uint8, device=dev)
    src[r0, c0] = 1
    cost, link, raw = dsm.cost_distance(src, _grid(n, n), return_raw=True)
    assert cost.is_cuda and link.is_cuda and raw.is_cuda
    wx, wd, wy = 128 * L[0], 128 * L[1], 128 * L[2]
    dr = (torch.arange(n, device=dev) - r0).abs()[:, None]
    dc = (torch.arange(n, device=dev) - c0).abs()[None, :]
    m = torch.minimum(dr, dc)
    want = m * wd + (dc - m) * wx + (dr - m) * wy
    assert torch.equal(raw, want) and torch.equal(cost, want.double() / 32768.0)
    assert int((link == 0).sum()) == 1 and int(link[r0, c0]) == 0 and int((link > 8).sum()) == 0
    assert int(link[r0, c0 + 5]) == 5 and int(link[r0 + 5, c0]) == 7 and int(link[r0 + 9, c0 + 9]) == 6 and int(link[r0 - 9, c0 - 9]) == 2


def test_one_cell_above_the_limit_is_rejected_without_a_launch(dev, lib):     # noqa: F811
    from satmvs_amd import _lib, dsm
    with pytest.raises(ValueError, match="2\\^24 cells"):
        dsm.cost_distance([(0, 0)], _grid(1, 2 ** 24 + 1))
    word = torch.full((64,), 77, dtype=torch.int64, device=dev)
    p = _lib.ptr
    with pytest.raises(_lib.SatMVSNativeError, match="at most 2\\^24"):
        _lib.call("smvs_dsm_cost_begin", None, p(word), None, 2 ** 24 + 1, 1, -999.0, p(word[8:]), p(word[16:]), p(word[24:]), 1 << 30, _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert bool((word == 77).all()) and lib.smvs_dsm_cost_workspace_bytes(2 ** 24 + 1, 1) == 0


def test_heights_at_the_edges_of_the_quantum(dev):           # noqa: F811
    """Heights on quantisation halves (ties to even), both zeros, NaN, +-Inf, nodata, +-32768 and one ulp beyond, under a table
    with a different entry in every bin, so that a quantum or a bin off changes a cost."""
    gh, gw = 33, 40
    rng = np.random.default_rng(77)
    z = ((rng.integers(0, 200, (gh, gw)) + 0.5 * rng.integers(0, 2, (gh, gw))) / 256.0).astype(np.float32)
    z[rng.random((gh, gw)) < 0.3] *= -1
    z[2, 3], z[2, 4], z[5, 5], z[5, 9], z[9, 9], z[20, 20] = 0.0, -0.0, np.nan, np.inf, -np.inf, -999.0
    z[12, 30], z[12, 31] = 32768.0, np.nextafter(np.float32(32768.0), np.float32(np.inf))
    z[25, 7], z[25, 8] = -32768.0, np.nextafter(np.float32(-32768.0), np.float32(-np.inf))
    z[12, 29], z[25, 6] = 32767.5, -32767.5                   # neighbours near enough for the 32768 m cells to be reached
    table = co.slope_table(lambda t: 1.0 + abs(t) / 4.0 + (0.01 if t < 0 else 0.0))
    table[[0, 255]] = [700, 900]                              # the end bins, where the 32768 m cells' steps land
    assert len(set(table.tolist())) == 256
    f = co.friction_of(gh, gw, 77, 12)
    src = co.sources_of(co.passable(gh, gw, f, z), 77, "several")
    for reverse in (False, True):
        args = dict(src=src, friction=f, z=z, table=table, reverse=reverse)
        want = co.chain(L=L, **args)
        assert want["raw"][12, 30] >= 0 and want["raw"][25, 7] >= 0 and want["raw"][12, 31] == -1 and want["raw"][25, 8] == -1 and np.isnan(want["cost"][5, 5])
        assert co.differing(_device(args), _want(want)) == []


def test_friction_0_1_and_65535_as_neighbours(dev):          # noqa: F811
    gh, gw = 34, 37
    rng = np.random.default_rng(3)
    f = rng.choice(np.array([0, 1, 65535], np.uint16), (gh, gw), p=[0.2, 0.4, 0.4])
    src = co.sources_of(f != 0, 3, "several")
    z = np.where(rng.random((gh, gw)) < 0.5, np.float32(0.0), np.float32(300.0))      # 300 m steps: the end bins with 65535 in them
    table = np.full(256, 65535, np.int32)
    for args in (dict(src=src, friction=f, z=None, table=None, reverse=False), dict(src=src, friction=f, z=z, table=table, reverse=False)):
        want = co.chain(L=L, **args)
        assert co.differing(_device(args), _want(want)) == []
    assert want["raw"].max() > 2 ** 31                        # into a cell of friction 65535: (65536 640 65535) >> 10 at the least


def test_max_cost_at_a_cell_and_one_below(dev):              # noqa: F811
    args, want = _reference(co.SCENE_CASES[1])
    r, c = np.argwhere(want["raw"] > 0)[123]
    d = int(want["raw"][r, c])
    for limit in (d, d - 1):
        got = _device(args, max_cost=limit / 32768.0)
        ref = co.chain(L=L, max_cost=limit, **args)
        assert co.differing(got, _want(ref)) == []
        assert (got["raw"][r, c] == d) == (limit == d) and (got["backlink"][r, c] == 255) == (limit != d)


# ---- calling conditions ------------------------------------------------------------------------------------------------------------
def _native(args, dev, batch=8, fill=0x5a, stream=None, outputs=OUT, G=64):     # noqa: F811
    """The three entries called directly, every output and the workspace between guard words, the workspace full of `fill`.
    -> the outputs (and keys, n_sources, rounds) as numpy."""
    from satmvs_amd import _lib
    lib = _lib.load()                                        # noqa: F811
    p = _lib.ptr
    stream = stream or _lib.current_stream(dev)
    src = args["src"]
    gh, gw = src.shape
    n = gh * gw
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    sd, fd, zd = up(src), up(args["friction"]), up(args["z"])
    q = lambda t: ctypes.c_void_p(0) if t is None else p(t)  # noqa: E731
    host = lambda a: ctypes.c_void_p(0) if a is None else a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    Lh = np.array(L, np.int32)
    table = None if args["table"] is None else np.ascontiguousarray(args["table"], np.int32)
    spec = {"keys": (torch.int64, n), "count": (torch.int32, 1), "status": (torch.int32, 1), "raw": (torch.int64, n), "cost": (torch.float64, n),
            "backlink": (torch.uint8, n)}
    bufs = {k: torch.full((m + 2 * G,), 77, dtype=dt, device=dev) for k, (dt, m) in spec.items()}
    at = {k: (p(bufs[k][G:]) if k not in OUT or k in outputs else ctypes.c_void_p(0)) for k in spec}
    nbytes = lib.smvs_dsm_cost_workspace_bytes(gw, gh)
    ws = torch.full((nbytes + 512,), fill, dtype=torch.uint8, device=dev)
    rev = int(args["reverse"])
    _lib.call("smvs_dsm_cost_begin", q(fd), p(sd), q(zd), gw, gh, -999.0, at["keys"], at["count"], p(ws[256:]), nbytes, stream)
    rounds = 0
    while True:
        _lib.call("smvs_dsm_cost_rounds", q(fd), q(zd), gw, gh, -999.0, host(Lh), host(table), rev, at["keys"], batch, at["status"], p(ws[256:]), nbytes, stream)
        rounds += batch
        torch.cuda.synchronize()
        if int(bufs["status"][G].item()) == 0:
            break
        assert rounds <= n + 2
    _lib.call("smvs_dsm_cost_read", q(fd), q(zd), gw, gh, -999.0, host(Lh), host(table), rev, at["keys"], 2 ** 64 - 1, at["raw"], at["cost"], at["backlink"],
              p(ws[256:]), nbytes, stream)
    torch.cuda.synchronize()
    for k, (dt, m) in spec.items():
        assert bool((bufs[k][:G] == 77).all()) and bool((bufs[k][G + m:] == 77).all()), k
        if k in OUT and k not in outputs:
            assert bool((bufs[k] == 77).all()), k             # a null output: nothing written anywhere near
    assert bool((ws[:256] == fill).all()) and bool((ws[256 + nbytes:] == fill).all())
    out = {k: bufs[k][G:G + m].cpu().numpy().reshape(gh, gw) for k, (dt, m) in spec.items() if m == n and (k not in OUT or k in outputs)}
    out["keys"] = out["keys"].view(np.uint64)
    out["n_sources"], out["rounds"] = int(bufs["count"][G].item()), rounds
    return out


@pytest.mark.parametrize("index", [1, 5], ids=["flat", "table-rev"])
def test_batches_workspaces_guards_and_a_side_stream(dev, index):     # noqa: F811
    """Batches of 1, 3 and 8 rounds, workspaces full of 0xff, 0x00 and 0x5a, and a side stream: equal keys and outputs, equal to
    the statements, nothing written outside the outputs; then the same bits again."""
    from satmvs_amd import _lib
    args, want = _reference(co.SCENE_CASES[index])
    runs = [_native(args, dev, batch, fill) for batch, fill in ((1, 0xff), (3, 0x00), (8, 0x5a), (8, 0x5a))]
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        runs.append(_native(args, dev, 8, 0xff, _lib.current_stream(dev)))
    ok = co.passable(*args["src"].shape, args["friction"], args["z"])
    for got in runs:
        assert co.differing(got, {k: want[k] for k in ("keys",) + OUT}) == []
        assert got["n_sources"] == int(((args["src"] != 0) & ok).sum())


def test_every_output_null_and_non_null(dev):                # noqa: F811
    args, want = _reference(co.SCENE_CASES[3])
    for outputs in ((), ("raw",), ("cost",), ("backlink",), ("raw", "backlink"), OUT):
        got = _native(args, dev, outputs=outputs)
        assert co.differing(got, {k: want[k] for k in ("keys",) + tuple(outputs)}) == []


def test_a_larger_call_before_a_smaller_one_and_the_same_bits_twice(dev):     # noqa: F811
    big, want_big = _reference(co.LARGE_CASES[1])
    small, want_small = _reference(co.GRID_CASES[13])
    first = _device(big)
    then = _device(small)
    again = _device(big)
    assert co.differing(first, _want(want_big)) == [] and co.differing(then, _want(want_small)) == []
    assert co.differing(again, {k: first[k] for k in OUT}) == []


def test_device_tensors_in_and_out(dev, monkeypatch):        # noqa: F811
    """Tensors in, tensors out, and no grid goes to the host on the way (a Tensor.cpu() call fails the test)."""
    from satmvs_amd import dsm
    args, want = _reference(co.SCENE_CASES[5])
    gh, gw = args["src"].shape
    sd, fd, zd = (torch.from_numpy(args[k]).to(dev) for k in ("src", "friction", "z"))

    def no_host_copy(self, *a, **k):
        raise AssertionError("a grid went to the host")
    monkeypatch.setattr(torch.Tensor, "cpu", no_host_copy)
    cost, link, raw = dsm.cost_distance(sd, _grid(gh, gw), fd, zd, args["table"], args["reverse"], return_raw=True)
    labels, n = dsm.cost_allocation(link)
    monkeypatch.undo()
    assert cost.is_cuda and link.is_cuda and raw.is_cuda and labels.is_cuda
    got = {"raw": raw.cpu().numpy(), "cost": cost.cpu().numpy(), "backlink": link.cpu().numpy()}
    assert co.differing(got, _want(want)) == []
    assert n == int((want["raw"] == 0).sum())
    assert dsm.quantise_friction(torch.tensor([[0.5, -1.0, 255.0]], device=dev)).cpu().tolist() == [[128, 0, 65280]]


def test_native_rejections_write_nothing(dev, lib):          # noqa: F811
    from satmvs_amd import _lib
    gw, gh = 9, 7
    n = gw * gh
    stream = _lib.current_stream(dev)
    p, null = _lib.ptr, ctypes.c_void_p(0)
    names = ("friction", "sources", "dsm", "keys", "count", "status", "raw", "cost", "link", "ws")
    nbytes = lib.smvs_dsm_cost_workspace_bytes(gw, gh)
    buf = {k: torch.full((max(n, nbytes // 8 + 1),), 77, dtype=torch.int64, device=dev) for k in names}
    Lh, table = np.array(L, np.int32), co.TABLE.copy()
    host = lambda a: null if a is None else a.ctypes.data_as(ctypes.c_void_p)       # noqa: E731

    def begin(friction=p(buf["friction"]), sources=p(buf["sources"]), dsm=p(buf["dsm"]), gw=gw, gh=gh, keys=p(buf["keys"]), count=p(buf["count"]),
              ws=p(buf["ws"]), nbytes=nbytes):
        _lib.call("smvs_dsm_cost_begin", friction, sources, dsm, gw, gh, -999.0, keys, count, ws, nbytes, stream)

    def rounds(friction=p(buf["friction"]), dsm=p(buf["dsm"]), gw=gw, gh=gh, L=Lh, table=table, reverse=0, keys=p(buf["keys"]), k=8, status=p(buf["status"]),
               ws=p(buf["ws"]), nbytes=nbytes):
        _lib.call("smvs_dsm_cost_rounds", friction, dsm, gw, gh, -999.0, host(L), host(table), reverse, keys, k, status, ws, nbytes, stream)

    def read(friction=p(buf["friction"]), dsm=p(buf["dsm"]), gw=gw, gh=gh, L=Lh, table=table, reverse=0, keys=p(buf["keys"]), raw=p(buf["raw"]),
             cost=p(buf["cost"]), link=p(buf["link"]), ws=p(buf["ws"]), nbytes=nbytes):
        _lib.call("smvs_dsm_cost_read", friction, dsm, gw, gh, -999.0, host(L), host(table), reverse, keys, 2 ** 64 - 1, raw, cost, link, ws, nbytes, stream)

    def rejected(call, match, **kw):
        with pytest.raises(_lib.SatMVSNativeError, match=match):
            call(**kw)

    inside = lambda k, off: ctypes.c_void_p(buf[k].data_ptr() + off)               # noqa: E731
    for name in ("sources", "keys", "count", "ws"):
        rejected(begin, "null pointer", **{name: null})
    for name in ("keys", "status", "ws", "L"):
        rejected(rounds, "null pointer", **{name: None if name == "L" else null})
    for name in ("keys", "ws", "L"):
        rejected(read, "null pointer", **{name: None if name == "L" else null})
    for call in (begin, rounds, read):
        rejected(call, "non-positive grid", gw=0)
        rejected(call, "at most 2\\^24", gw=4097, gh=4096)
        rejected(call, "workspace too small", nbytes=nbytes - 1)
        rejected(call, "aliases", keys=inside("friction", 2 * n - 1))
        rejected(call, "workspace aliases", ws=inside("keys", 8 * n - 1))
    rejected(begin, "aliases", count=inside("sources", n - 1))
    rejected(rounds, "aliases", status=inside("keys", 8))
    rejected(read, "aliases", raw=p(buf["cost"]))
    rejected(read, "aliases", link=inside("cost", 8 * n - 1))
    for k in (0, 4097):
        rejected(rounds, "rounds must be in", k=k)
    for call in (rounds, read):
        rejected(call, "go together", dsm=null)
        rejected(call, "go together", table=None)
        rejected(call, "reverse must be", reverse=-1)
        bad = Lh.copy()
        bad[5] = 32768
        rejected(call, "L\\[5\\]", L=bad)
        bad = table.copy()
        bad[77] = 65536
        rejected(call, "table\\[77\\]", table=bad)
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in buf.values())


def test_cost_distance_gives_up_on_a_status_that_never_clears(dev, monkeypatch):     # noqa: F811
    from satmvs_amd import _lib, dsm
    real = dsm._call

    def stuck(dev_, name, *args):                            # a device that keeps reporting changed tiles
        real(dev_, name, *args)
        if name == "smvs_dsm_cost_rounds":
            args[10].fill_(1)

    monkeypatch.setattr(dsm, "_call", stuck)
    with pytest.raises(_lib.SatMVSNativeError, match="smvs_dsm_cost_rounds: tiles still change"):
        dsm.cost_distance([(1, 1)], _grid(3, 4))
    calls = []
    with pytest.raises(_lib.SatMVSNativeError, match="stub: tiles still change after 24 rounds"):
        dsm._relax(lambda k: calls.append(k) or 1, 20, "stub")
    assert calls == [8, 16]


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_dtm_to_least_cost_paths_geojson(dev, tmp_path):     # noqa: F811
    """extract_dtm -> friction from slope with the object footprints as barriers -> cost_distance from three sources ->
    cost_allocation -> least_cost_paths for 50 targets -> write_streams read back."""
    from satmvs_amd import dsm
    gh, gw = 96, 120
    grid = _grid(gh, gw)
    E, N = grid.e0 + co.XRES * np.mgrid[0:gh, 0:gw][1], grid.n0 - co.YRES * np.mgrid[0:gh, 0:gw][0]
    zd = torch.from_numpy(kit_scene(E, N, holes=False)).to(dev)
    dtm = dsm.extract_dtm(zd, grid)
    labels, _ = dsm.extract_objects(dsm.ndsm(zd, dtm), grid)
    f = dsm.quantise_friction(1.0 + dsm.slope(dtm, grid).cpu().numpy().astype(np.float64) / 10.0)      # NaN (no slope) becomes a barrier
    f[labels.cpu().numpy() > 0] = 0
    assert f.dtype == np.uint16 and (f == 0).sum() > 20 and len(np.unique(f)) > 20
    open_cells = np.argwhere(f != 0)
    sources = [tuple(int(v) for v in open_cells[i]) for i in (50, len(open_cells) // 2, len(open_cells) - 70)]
    cost, link, raw = dsm.cost_distance(sources, grid, f, return_raw=True)
    src = np.zeros((gh, gw), np.uint8)
    for r, c in sources:
        src[r, c] = 1
    assert co.differing({"raw": raw, "cost": cost, "backlink": link}, _want(co.chain(src, L, f))) == []
    singles = [dsm.cost_distance([s], grid, f, return_raw=True)[2] for s in sources]
    least = np.minimum.reduce([np.where(s < 0, 2 ** 62, s) for s in singles])
    assert np.array_equal(raw, np.where(least == 2 ** 62, -1, least))              # the cell-wise minimum of the single-source runs
    served, n = dsm.cost_allocation(link)
    order = sorted(range(3), key=lambda i: sources[i])       # the sources are numbered in row-major order
    assert n == 3
    assert np.array_equal(served > 0, raw >= 0)
    for r, c in np.argwhere(raw >= 0)[::37]:
        assert singles[order[served[r, c] - 1]][r, c] == raw[r, c]          # the allocated source attains the minimum
    rng = np.random.default_rng(8)
    targets = [tuple(int(v) for v in open_cells[i]) for i in rng.choice(len(open_cells), 48, replace=False)]
    barrier = tuple(int(v) for v in np.argwhere(f == 0)[3])
    targets += [barrier, sources[0]]                          # one that is reported, not followed, and one that is its own path
    paths = dsm.least_cost_paths(link, targets, grid, raw)
    unfollowed = {i for i, (r, c) in enumerate(targets) if link[r, c] == 255}
    assert 48 in unfollowed and len(unfollowed) < 10
    assert paths["target_link"][48] == -1 and np.isnan(paths["target_length_m"][48]) and np.isposinf(paths["target_cost"][48]) and (paths["target_steps"][48] == -1).all()
    assert np.array_equal(paths["target_cell"], np.array(targets, np.int32))
    W = co.step_costs(gh, gw, L, f)
    hyp = float(np.hypot(co.XRES, co.YRES))
    for i, (r, c) in enumerate(targets):
        if i in unfollowed:
            continue
        cells, codes = co.walk(link, r, c)
        ew, ns, dg = (sum(1 for k in codes if k in ks) for ks in ((0, 4), (2, 6), (1, 3, 5, 7)))
        assert paths["target_steps"][i].tolist() == [ew, ns, dg]
        assert paths["target_length_m"][i] == (ew * co.XRES + ns * co.YRES) + dg * hyp            # the formula on the step counts, bit for bit
        assert paths["target_cost"][i] == raw[r, c] / 32768.0
    path = str(tmp_path / "paths.geojson")
    written = dsm.write_streams(path, paths, grid)
    with open(path) as fh:
        features = json.load(fh)["features"]
    by_link = {ft["properties"]["link"]: ft for ft in features}
    assert written == len(features) > 0
    nxt, offset, vertices = paths["next_link"], paths["offset"], paths["vertices"]
    source_cells = set(sources)
    for i, (r, c) in enumerate(targets):
        if i in unfollowed:
            continue
        k = int(paths["target_link"][i])
        assert k >= 0
        # from the target's own vertex along its link and the links after it: the written vertices are the walk of the back-links
        line = [tuple(v) for v in vertices[offset[k]:offset[k + 1]].tolist()]
        at = line.index((c, r))
        walked, total = line[at:], 0
        while nxt[k] >= 0:
            k = int(nxt[k])
            line = [tuple(v) for v in vertices[offset[k]:offset[k + 1]].tolist()]
            assert line[0] == walked[-1]
            walked += line[1:]
        assert (walked[-1][1], walked[-1][0]) in source_cells                  # following next_link reaches a source
        assert [(cc, rr) for rr, cc in co.walk(link, r, c)[0]] == walked
        if offset[k + 1] - offset[k] >= 2:
            en = by_link[k]["geometry"]["coordinates"]
            assert en[-1] == [grid.e0 + walked[-1][0] * co.XRES, grid.n0 - walked[-1][1] * co.YRES]
        for (c0, r0), (c1, r1) in zip(walked, walked[1:]):
            k8 = [k8 for k8 in range(8) if (co.DR[k8], co.DC[k8]) == (r1 - r0, c1 - c0)][0]
            total += int(W[k8, r0, c0])
        assert total == raw[r, c]                             # the integer step costs along the written vertices
