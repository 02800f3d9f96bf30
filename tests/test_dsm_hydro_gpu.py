"""Hydrology on the device against the Python statement of the rule (tests/dsm_hydro_oracle.py): keys, filled, depth, flat_dist,
directions, accumulation, basins and their count are compared by np.array_equal (floats by their bits), no cell excused.

Sizes.  The flood works on tiles of 32 x 32 cells (T - 1, T, T + 1 on both sides: 31, 32, 33); the other kernels run 256 lanes a
workgroup over the cells and over the tour's 2 gw gh elements, and the basins scan the cells in blocks of 2048 on three levels.
SIZES holds the issue's grids and three of 1023, 1024 and 1025 cells (11 x 93, 32 x 32, 25 x 41), whose tours straddle a scan
block.  The 2300 x 2300 plane has more than 2048^2 cells and tour elements: the scan's second level holds more than one block.
The serpentine at 257 x 301 is the deepest tree and takes the most flood rounds."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

import dsm_hydro_oracle as ho
from dsm_testkit import dev, scene as kit_scene  # noqa: F401  (dev: fixture)

pytestmark = pytest.mark.gpu
SIZES = [(1, 1), (1, 70), (67, 1), (2, 2), (67, 3), (31, 31), (32, 32), (33, 33), (31, 33), (33, 31), (11, 93), (25, 41), (257, 301)]
G = 64                                                       # guard words on both sides of an output
XRES, YRES = ho.XRES, ho.YRES                                # 5 m x 2.5 m: the steepest neighbour differs from the square cell's


def _grid(dsm, gh, gw):
    return dsm.DSMGrid(500000.0, 3400000.0, XRES, YRES, gw, gh)


def _device_chain(z, weight=None):
    """The outputs of the Python layer for a DSM, under the oracle's names; numpy in, numpy out."""
    from satmvs_amd import dsm
    z = np.ascontiguousarray(z, np.float32)
    gh, gw = z.shape
    grid = _grid(dsm, gh, gw)
    filled, depth, flat, rounds = dsm.fill_depressions(z, return_depth=True, return_rounds=True)
    keys, _ = dsm._flood(torch.from_numpy(z).cuda(), -999.0)
    code = dsm.flow_direction(z, grid)
    acc = dsm.flow_accumulation(code, weight)
    basin, n = dsm.basins(code)
    out = {"keys": keys.cpu().numpy().view(np.uint64), "filled": filled, "depth": depth, "flat_dist": flat, "dir": code, "acc": acc,
           "basin": basin, "n": np.int64(n)}
    assert all(isinstance(t, (np.ndarray, np.int64)) for t in out.values()) and rounds >= 1
    assert np.array_equal(dsm.fill_depressions(z).view(np.uint32), filled.view(np.uint32))
    return out


def _check(z, what, weight=None):
    want = ho.chain(z, XRES, YRES, weight=weight, arrays=True)
    got = _device_chain(z, weight)
    assert ho.differing(got, want) == [], what
    return got


# ---- random hills, sizes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ho.RANDOM_CASES)
def test_random_hills(dev, case):
    gh, gw, seed, voids, levels = case
    got = _check(ho.hills(gh, gw, seed, voids, levels), case)
    if voids < 0.3:
        assert (got["depth"] > 0).sum() > 10 and got["acc"].max() > 20 and (not levels or got["flat_dist"].max() >= 2)


@pytest.mark.parametrize("shape", SIZES)
def test_sizes(dev, shape):
    gh, gw = shape
    got = _check(ho.hills(gh, gw, gh + gw, 0.02 if gh * gw > 500 else 0.0, 12), shape)
    if min(shape) <= 2:
        assert (got["dir"] == 0).all() and got["n"] == gh * gw


def test_large_plane_closed_form(dev):
    """2300 x 2300 on the device only: z = col / 4 falls to the west, so every inner cell drains west (code 5) into the outlet at
    the left end of its row; acc = the cells east of it in the row, itself included; the roots are the edge cells."""
    from satmvs_amd import dsm
    g = 2300
    col = torch.arange(g, device=dev)
    z = (col.float() * 0.25).repeat(g, 1).contiguous()
    filled, depth, flat = dsm.fill_depressions(z, return_depth=True)
    assert filled.is_cuda and torch.equal(filled.view(torch.int32), z.view(torch.int32)) and not depth.any() and not flat.any()
    code = dsm.flow_direction(z, dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, g, g))
    inner = torch.zeros((g, g), dtype=torch.bool, device=dev)
    inner[1:-1, 1:-1] = True
    assert torch.equal(code, torch.where(inner, 5, 0).to(torch.uint8))
    acc = dsm.flow_accumulation(code)
    want = torch.where(inner, (g - 1 - col).repeat(g, 1), 1)
    want[1:-1, 0] = g - 1
    assert acc.dtype == torch.int64 and torch.equal(acc, want)
    basin, n = dsm.basins(code)
    row = torch.arange(g, device=dev)[:, None]
    number = torch.where(row == 0, col + 1, torch.where(row == g - 1, g + 2 * (g - 2) + col + 1, g + 2 * (row - 1) + 1 + (col == g - 1).long())).to(torch.int32)
    assert n == 4 * g - 4 and torch.equal(basin, torch.where(inner, number[:, :1].expand(g, g), number))


# ---- shapes ------------------------------------------------------------------------------------------------------------------------
def test_crater_is_one_flat(dev):
    n = 129
    got = _check(ho.crater(n), "crater")
    assert got["flat_dist"].max() == n // 2 and (got["filled"] == 95.0).all() and (got["depth"][2:-2, 2:-2] == 15.0).all()


def test_serpentine(dev):
    z, path = ho.serpentine(257, 301)
    got = _check(z, "serpentine")
    assert got["acc"][path[0]] > len(path) - 300 and not got["depth"].any()


def test_comb(dev):
    got = _check(ho.comb(65, 97), "comb")
    assert got["acc"].max() > 48 * 60


def test_degenerate_grids(dev):
    empty = np.full((37, 41), np.nan, np.float32)
    empty[::2] = -999.0
    got = _check(empty, "all invalid")
    assert got["n"] == 0 and (got["dir"] == 255).all() and not got["acc"].any() and (got["filled"] == -999.0).all()
    one = empty.copy()
    one[17, 33] = 12.5
    got = _check(one, "one valid cell")
    assert got["n"] == 1 and got["basin"][17, 33] == 1 and got["acc"].sum() == 1 and got["dir"][17, 33] == 0
    pit = np.full((35, 35), 50.0, np.float32)
    pit[10:25, 10:25] = 20.0
    assert _check(pit, "a pit")["depth"].max() == 30.0
    pit[17, 17] = np.nan
    got = _check(pit, "a void in the middle of a pit drains it")
    assert got["depth"][np.isfinite(pit)].max() == 0.0 and got["flat_dist"].max() == 6


def test_height_edges(dev):
    """Heights on quantisation halves, both zeros, NaN, +-Inf, nodata, +-32768 and one ulp beyond."""
    f = np.float32
    special = [f(1.0) / 512, f(3.0) / 512, f(5.0) / 512, -f(1.0) / 512, -f(3.0) / 512, f(0.0), -f(0.0), f(np.nan), f(np.inf), -f(np.inf), f(-999.0),
               f(32768.0), f(-32768.0), np.nextafter(f(32768.0), f(np.inf)), np.nextafter(f(-32768.0), f(-np.inf)), f(1e-30), f(-1e-30)]
    rng = np.random.default_rng(8)
    z = rng.choice(np.array(special, np.float32), (40, 45))
    z[5:30, 5:30] = rng.choice(np.array(special[:7], np.float32), (25, 25))       # a block without voids: flats of zeros of both signs
    got = _check(z, "edges")
    v = ho.valid(z)
    assert np.array_equal(got["dir"] == 255, ~v) and v[z == f(32768.0)].all() and not v[np.abs(z) > f(32768.0)].any()
    untouched = v & (got["depth"] == 0)
    assert np.array_equal(got["filled"][untouched].view(np.uint32), z[untouched].view(np.uint32)) and (np.signbit(z[untouched]) & (z[untouched] == 0)).any()


def test_nodata_and_esri(dev):
    from satmvs_amd import dsm
    z = ho.hills(40, 50, 9, 0.05, 12)
    z[z == -999.0] = 12345.0
    z[3, 3] = -999.0                                          # a height like any other now
    want = ho.chain(z, XRES, YRES, nodata=12345.0, arrays=True)
    filled, depth, flat = dsm.fill_depressions(z, nodata=12345.0, return_depth=True)
    grid = _grid(dsm, 40, 50)
    code = dsm.flow_direction(z, grid, nodata=12345.0)
    assert ho.differing({"filled": filled, "depth": depth, "flat_dist": flat, "dir": code}, {k: want[k] for k in ("filled", "depth", "flat_dist", "dir")}) == []
    assert want["dir"][3, 3] != 255
    esri = dsm.flow_direction(torch.from_numpy(z).to(dev), grid, nodata=12345.0, encoding="esri")
    assert esri.is_cuda and np.array_equal(esri.cpu().numpy(), dsm.flow_codes("esri")[code])
    square = dsm.flow_direction(z, dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, 50, 40), nodata=12345.0)
    assert np.array_equal(square, ho.chain(z, 5.0, 5.0, nodata=12345.0, arrays=True)["dir"]) and (square != code).any()


# ---- arbitrary code grids ------------------------------------------------------------------------------------------------------------
def _cyclic_grid():
    """A 2-cycle, a long cycle round a block, a tree draining into that cycle, codes 9 and 254, targets off the grid; the rest
    drains to the cell below or off the bottom edge."""
    gh, gw = 40, 47
    code = np.full((gh, gw), 3, np.uint8)                     # south, the last row off the grid: roots
    code[5, 5], code[5, 6] = 1, 5                             # a 2-cycle
    code[10, 10:30], code[10:20, 30], code[20, 11:31], code[11:21, 10] = 1, 3, 5, 7          # a ring of 60 cells, clockwise
    code[2:10, 15] = 3                                        # a tributary of the ring (it is south-bound anyway)
    code[15, 11:30] = 1                                       # inside the ring, eastwards into its east side
    code[30, 3], code[30, 4], code[31, 3] = 9, 254, 255
    code[0, 0], code[0, gw - 1], code[gh - 1, 0] = 7, 8, 4    # targets off the grid
    code[29, 4] = 3                                           # a target without a code: a root
    return code


def test_cycles_voids_and_roots(dev):
    from satmvs_amd import dsm
    code = _cyclic_grid()
    weight = np.random.default_rng(2).integers(-50, 50, code.shape).astype(np.int32)
    for wt in (None, weight):
        want, cyc = ho.accumulate_subtrees(code, wt)
        assert cyc and (want == -1).sum() >= 2 + 60
        with pytest.raises(ValueError, match="cycle"):
            dsm.flow_accumulation(code, wt)
        got = dsm.flow_accumulation(code, wt, cycles="mark")
        assert got.dtype == np.int64 and np.array_equal(got, want)
    lab, n, cyc = ho.basins_walk(code)
    got, gn = dsm.basins(code)
    plain, _ = ho.accumulate_subtrees(code)                   # without weights -1 is no sum: the cells without a root
    assert cyc and gn == n and got.dtype == np.int32 and np.array_equal(got, lab) and (lab[plain == -1] == 0).all()
    grid = _grid(dsm, *code.shape)
    area = dsm.flow_accumulation(code, grid=grid, cycles="mark")
    assert area.dtype == np.float64 and np.array_equal(area, np.where(plain == -1, -1.0, plain * (XRES * YRES)))
    rng = np.random.default_rng(5)
    for _ in range(6):                                        # anything at all
        shape = tuple(rng.integers(1, 60, 2))
        code = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 9, 254, 255], np.uint8), shape)
        want, cyc = ho.accumulate_peel(code)
        assert np.array_equal(dsm.flow_accumulation(code, cycles="mark"), want)
        lab, n, _ = ho.basins_arrays(code)
        got, gn = dsm.basins(code)
        assert gn == n and np.array_equal(got, lab)


def test_weights_pass_two_to_the_32(dev):
    from satmvs_amd import dsm
    gh, gw = 3, 4000
    code = np.full((gh, gw), 5, np.uint8)                     # west; the first column off the grid
    code[0], code[2] = 3, 7                                   # the outer rows into the middle one
    weight = np.full((gh, gw), 2 ** 31 - 1, np.int32)
    weight[0, ::3] = -2 ** 31
    weight[2, ::5] = -7
    want, cyc = ho.accumulate_peel(code, weight)
    got = dsm.flow_accumulation(code, weight)
    assert not cyc and np.array_equal(got, want) and got[1, 0] == weight.astype(np.int64).sum() > 2 ** 32


def test_pour_points(dev):
    from satmvs_amd import dsm
    z = ho.hills(60, 70, 11, 0.03, None)
    want = ho.chain(z, XRES, YRES, arrays=True)
    code, acc = want["dir"], want["acc"]
    recv = ho.receivers(code)
    far = (recv >= 0) & (recv[np.maximum(recv, 0)] >= 0)      # two steps at least from its root
    r, c = np.unravel_index(np.argmax(np.where(far.reshape(acc.shape), acc, 0)), acc.shape)           # the largest such river
    down = recv[r * 70 + c]
    root = int(ho.roots_walk(recv)[r * 70 + c])
    void = tuple(np.argwhere(code == 255)[0])
    points = [(r, c), divmod(int(down), 70), divmod(root, 70), void, (r, c)]             # two on one river, one on a root, one on a void, one twice
    mask = np.zeros(code.shape, bool)
    for p in points:
        mask[p] = True
    lab, n, _ = ho.basins_walk(code, mask)
    assert n == 3 and len(np.unique(lab)) == 4
    for pour in (mask, mask.astype(np.int16) * 7, np.array(points, np.int64), torch.tensor(points, dtype=torch.int32), torch.from_numpy(mask).to(dev)):
        got, gn = dsm.basins(code, pour)
        assert gn == n and np.array_equal(got, lab)
    got, gn = dsm.basins(code, np.zeros((0, 2), np.int64))
    assert gn == 0 and not got.any()


# ---- robustness ----------------------------------------------------------------------------------------------------------------------
def _native(dev, z, fill, batch, weight=None, pour=None):
    """Every entry called directly: guard words round every output and the workspaces, the workspaces full of `fill` -> the
    outputs under the oracle's names, and the rounds run."""
    from satmvs_amd import _lib
    lib = _lib.load()
    p, stream = _lib.ptr, _lib.current_stream(dev)
    gh, gw = z.shape
    n = gh * gw
    zd = torch.from_numpy(z).to(dev)
    spec = {"keys": (torch.int64, n), "status": (torch.int32, 1), "filled": (torch.float32, n), "depth": (torch.float32, n), "flat_dist": (torch.int32, n),
            "dir": (torch.uint8, n), "acc": (torch.int64, n), "flag": (torch.int32, 1), "basin": (torch.int32, n), "n": (torch.int32, 1), "flag2": (torch.int32, 1)}
    bufs = {k: torch.full((m + 2 * G,), 77, dtype=dt, device=dev) for k, (dt, m) in spec.items()}
    at = {k: p(bufs[k][G:]) for k in spec}
    flood_bytes, flow_bytes = lib.smvs_dsm_flood_workspace_bytes(gw, gh), lib.smvs_dsm_flow_workspace_bytes(gw, gh)
    ws1 = torch.full((flood_bytes + 512,), fill, dtype=torch.uint8, device=dev)
    ws2 = torch.full((flow_bytes + 512,), fill, dtype=torch.uint8, device=dev)
    dist = np.array(ho.distances(XRES, YRES))
    wd = None if weight is None else torch.from_numpy(weight).to(dev)
    pd = None if pour is None else torch.from_numpy(pour.astype(np.uint8)).to(dev)
    null = ctypes.c_void_p(0)
    _lib.call("smvs_dsm_flood_begin", p(zd), gw, gh, -999.0, at["keys"], p(ws1[256:]), flood_bytes, stream)
    rounds = 0
    while True:
        _lib.call("smvs_dsm_flood_rounds", p(zd), gw, gh, -999.0, at["keys"], batch, at["status"], p(ws1[256:]), flood_bytes, stream)
        rounds += batch
        if int(bufs["status"][G].item()) == 0:
            break
        assert rounds <= n + 2
    _lib.call("smvs_dsm_flood_read", p(zd), gw, gh, -999.0, at["keys"], at["filled"], at["depth"], at["flat_dist"], stream)
    _lib.call("smvs_dsm_flow_dir", at["keys"], gw, gh, dist.ctypes.data_as(ctypes.c_void_p), at["dir"], stream)
    _lib.call("smvs_dsm_flow_accumulate", at["dir"], null if wd is None else p(wd), gw, gh, at["acc"], at["flag"], p(ws2[256:]), flow_bytes, stream)
    _lib.call("smvs_dsm_flow_basins", at["dir"], null if pd is None else p(pd), gw, gh, at["basin"], at["n"], at["flag2"], p(ws2[256:]), flow_bytes, stream)
    torch.cuda.synchronize()
    for k, (dt, m) in spec.items():
        assert bool((bufs[k][:G] == 77).all()) and bool((bufs[k][G + m:] == 77).all()), k
    for ws, nbytes in ((ws1, flood_bytes), (ws2, flow_bytes)):
        assert bool((ws[:256] == fill).all()) and bool((ws[256 + nbytes:] == fill).all())
    out = {k: bufs[k][G:G + m].cpu().numpy() for k, (dt, m) in spec.items()}
    assert out["flag"][0] == 0 and out["flag2"][0] == 0 and out["status"][0] == 0
    shaped = {k: out[k].reshape(gh, gw) for k in ("filled", "depth", "flat_dist", "dir", "acc", "basin")}
    shaped.update(keys=out["keys"].view(np.uint64).reshape(gh, gw), n=np.int64(out["n"][0]))
    return shaped, rounds


def test_entries_keep_to_their_outputs(dev):
    z = ho.hills(97, 131, 4, 0.04, 12)
    weight = np.random.default_rng(1).integers(-99, 99, z.shape).astype(np.int32)
    want = ho.chain(z, XRES, YRES, weight=weight, arrays=True)
    rounds = {}
    for fill, batch in ((0xff, 1), (0x00, 3), (0x5a, 8)):
        got, rounds[batch] = _native(dev, z, fill, batch, weight)
        assert ho.differing(got, want) == [], "workspace full of 0x%02x, batches of %d" % (fill, batch)
    assert rounds[1] >= 2 and rounds[3] >= rounds[1] and rounds[3] % 3 == 0 and rounds[8] % 8 == 0
    pour = np.zeros(z.shape, bool)
    pour[40:60:3, 50:90:7] = True
    got, _ = _native(dev, z, 0x5a, 8, None, pour)
    lab, n, _ = ho.basins_walk(want["dir"], pour)
    assert got["n"] == n and np.array_equal(got["basin"], lab) and np.array_equal(got["acc"], ho.chain(z, XRES, YRES, arrays=True)["acc"])


def test_deterministic_streams_and_device_tensors(dev):
    from satmvs_amd import dsm
    big, small = ho.hills(300, 340, 1, 0.02, 12), ho.hills(40, 50, 2, 0.0, None)
    grid = _grid(dsm, 300, 340)
    bd, sd = torch.from_numpy(big).to(dev), torch.from_numpy(small).to(dev)
    keep = bd.clone()

    def run(z, g):
        filled, depth, flat = dsm.fill_depressions(z, return_depth=True)
        code = dsm.flow_direction(z, g)
        acc = dsm.flow_accumulation(code)
        basin, n = dsm.basins(code)
        return {"filled": filled, "depth": depth, "flat_dist": flat, "dir": code, "acc": acc, "basin": basin, "n": n}

    a = run(bd, grid)                                        # a larger call before a smaller one
    s = run(sd, _grid(dsm, 40, 50))
    b = run(bd, grid)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        c = run(bd, grid)
    side.synchronize()
    assert torch.equal(bd.view(torch.int32), keep.view(torch.int32))
    for k in a:
        if k == "n":
            assert a[k] == b[k] == c[k]
            continue
        assert a[k].is_cuda and b[k].is_cuda and c[k].is_cuda, k
        for other in (b, c):
            x, y = a[k], other[k]
            if x.dtype == torch.float32:
                x, y = x.view(torch.int32), y.view(torch.int32)
            assert x.dtype == y.dtype and torch.equal(x, y), k
    host = lambda o: {k: (t.cpu().numpy() if k != "n" else np.int64(t)) for k, t in o.items()}                # noqa: E731
    for got, z in ((a, big), (s, small)):
        want = ho.chain(z, XRES, YRES, arrays=True)
        assert ho.differing(host(got), {k: want[k] for k in got}) == []
    assert dsm.streams(a["acc"], 50).is_cuda and np.array_equal(dsm.streams(a["acc"], 50).cpu().numpy(), ho.chain(big, XRES, YRES, arrays=True)["acc"] >= 50)


def test_flood_gives_up_on_a_status_that_never_clears(dev, monkeypatch):
    from satmvs_amd import _lib, dsm
    real = dsm._call

    def stuck(dev_, name, *args):                            # a device that keeps reporting changed tiles
        real(dev_, name, *args)
        if name == "smvs_dsm_flood_rounds":
            args[6].fill_(1)

    monkeypatch.setattr(dsm, "_call", stuck)
    with pytest.raises(_lib.SatMVSNativeError, match="still change"):
        dsm.fill_depressions(np.zeros((3, 4), np.float32))


def test_native_argument_rejections(dev):
    from satmvs_amd import _lib
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    gw, gh = 9, 7
    n = gw * gh
    z = torch.zeros((gh, gw), dtype=torch.float32, device=dev)
    z[3, 4] = -5.0
    flood_bytes, flow_bytes = lib.smvs_dsm_flood_workspace_bytes(gw, gh), lib.smvs_dsm_flow_workspace_bytes(gw, gh)
    ws1 = torch.empty(flood_bytes, dtype=torch.uint8, device=dev)
    ws2 = torch.empty(flow_bytes, dtype=torch.uint8, device=dev)
    out = {k: torch.zeros(n, dtype=torch.int64, device=dev) for k in ("keys", "status", "filled", "depth", "flat", "dir", "weight", "acc", "flag", "basin", "n")}
    p, null, host = _lib.ptr, ctypes.c_void_p(0), lambda a: a.ctypes.data_as(ctypes.c_void_p)
    dist = np.array(ho.distances(XRES, YRES))

    def begin(dsm=p(z), gw=gw, gh=gh, keys=p(out["keys"]), ws=p(ws1), nbytes=flood_bytes):
        _lib.call("smvs_dsm_flood_begin", dsm, gw, gh, -999.0, keys, ws, nbytes, stream)

    def rounds(dsm=p(z), gw=gw, gh=gh, keys=p(out["keys"]), k=8, status=p(out["status"]), ws=p(ws1), nbytes=flood_bytes):
        _lib.call("smvs_dsm_flood_rounds", dsm, gw, gh, -999.0, keys, k, status, ws, nbytes, stream)

    def read(dsm=p(z), gw=gw, gh=gh, keys=p(out["keys"]), filled=p(out["filled"]), depth=p(out["depth"]), flat=p(out["flat"])):
        _lib.call("smvs_dsm_flood_read", dsm, gw, gh, -999.0, keys, filled, depth, flat, stream)

    def flow_dir(keys=p(out["keys"]), gw=gw, gh=gh, dist=dist, code=p(out["dir"])):
        _lib.call("smvs_dsm_flow_dir", keys, gw, gh, null if dist is None else host(dist), code, stream)

    def accumulate(code=p(out["dir"]), weight=p(out["weight"]), gw=gw, gh=gh, acc=p(out["acc"]), flag=p(out["flag"]), ws=p(ws2), nbytes=flow_bytes):
        _lib.call("smvs_dsm_flow_accumulate", code, weight, gw, gh, acc, flag, ws, nbytes, stream)

    def basins(code=p(out["dir"]), pour=null, gw=gw, gh=gh, basin=p(out["basin"]), n_out=p(out["n"]), flag=p(out["flag"]), ws=p(ws2), nbytes=flow_bytes):
        _lib.call("smvs_dsm_flow_basins", code, pour, gw, gh, basin, n_out, flag, ws, nbytes, stream)

    bad = [(fn, kw) for fn in (begin, rounds, read, flow_dir, accumulate, basins) for kw in (dict(gw=0), dict(gh=-1), dict(gw=2 ** 15, gh=2 ** 15))]
    for fn in (begin, rounds):
        bad += [(fn, dict(dsm=null)), (fn, dict(keys=null)), (fn, dict(ws=null)), (fn, dict(nbytes=flood_bytes - 1)), (fn, dict(keys=p(z))), (fn, dict(ws=p(out["keys"])))]
    bad += [(rounds, dict(status=null)), (rounds, dict(k=0)), (rounds, dict(k=4097)), (rounds, dict(status=p(out["keys"]))), (rounds, dict(status=p(ws1))),
            (read, dict(dsm=null)), (read, dict(keys=null)), (read, dict(filled=p(z))), (read, dict(depth=p(out["filled"]))), (read, dict(flat=p(out["keys"]))),
            (flow_dir, dict(keys=null)), (flow_dir, dict(dist=None)), (flow_dir, dict(code=null)), (flow_dir, dict(code=p(out["keys"])))]
    for value in (0.0, -1.0, np.nan, np.inf):
        wrong = dist.copy()
        wrong[5] = value
        bad.append((flow_dir, dict(dist=wrong)))
    for fn, name in ((accumulate, "acc"), (basins, "basin")):
        bad += [(fn, dict(code=null)), (fn, {name: null}), (fn, dict(flag=null)), (fn, dict(ws=null)), (fn, dict(nbytes=flow_bytes - 1)), (fn, {name: p(out["dir"])}),
                (fn, dict(flag=p(out[name]))), (fn, dict(ws=p(out["dir"])))]
    bad += [(accumulate, dict(weight=p(out["dir"]))), (basins, dict(pour=p(out["dir"]))), (basins, dict(n_out=null)), (basins, dict(n_out=p(out["basin"])))]
    for fn, kw in bad:
        with pytest.raises(_lib.SatMVSNativeError, match="code 1"):
            fn(**kw)
    torch.cuda.synchronize()
    begin()                                                  # and the same arguments unchanged are accepted
    rounds()
    read(depth=null, flat=null)
    flow_dir()
    out["weight"].view(torch.int32)[:n] = 2
    accumulate()
    basins()
    torch.cuda.synchronize()
    assert out["status"].view(torch.int32)[0].item() == 0 and out["filled"].view(torch.float32)[3 * gw + 4].item() == 0.0
    roots = out["dir"].view(torch.uint8)[:n] == 0
    assert out["acc"][:n][roots].sum().item() == 2 * n and out["n"].view(torch.int32)[0].item() == int(roots.sum()) == 2 * gw + 2 * gh - 4


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_dtm_to_geojson(dev, tmp_path):
    """extract_dtm -> fill_depressions -> flow_direction -> flow_accumulation -> basins -> depressions -> outlines -> write_geojson
    read back: the basins' areas sum to the valid cells and every depression's volume is the sum of depth over its cells."""
    from satmvs_amd import dsm
    gh, gw = 96, 120
    grid = dsm.DSMGrid(400000.0, 3500000.0, 5.0, 2.5, gw, gh)
    E, N = grid.e0 + 5.0 * np.mgrid[0:gh, 0:gw][1], grid.n0 - 2.5 * np.mgrid[0:gh, 0:gw][0]
    raw = kit_scene(E, N, holes=False, amp=2.0)               # gentle terrain and two blocks for the ground filter to remove
    raw[30:50, 40:70] -= np.float32(12.0)                     # a quarry deeper than the terrain varies across it: ground, and closed
    raw[70:74, 20:25] -= np.float32(3.0)                      # a pond of 20 cells
    raw[80, 100] -= np.float32(2.0)                           # a pit of one cell, which the sieve drops
    dtm = dsm.extract_dtm(torch.from_numpy(raw).to(dev), grid)
    z = dtm.cpu().numpy()
    want = ho.chain(z, 5.0, 2.5, arrays=True)
    filled, depth, flat = dsm.fill_depressions(dtm, return_depth=True)
    code = dsm.flow_direction(dtm, grid)
    acc = dsm.flow_accumulation(code, grid=grid)
    basin, n = dsm.basins(code)
    got = {"filled": filled, "depth": depth, "flat_dist": flat, "dir": code, "basin": basin}
    assert all(t.is_cuda for t in got.values()) and acc.is_cuda and n == want["n"]
    assert ho.differing({k: t.cpu().numpy() for k, t in got.items()}, {k: want[k] for k in got}) == []
    assert np.array_equal(acc.cpu().numpy(), want["acc"] * 12.5)
    stats = dsm.label_stats(basin, n, grid=grid)
    valid = ho.valid(z)
    assert int(stats["area"].sum()) == int(valid.sum()) and float(stats["area_m2"].sum()) == valid.sum() * 12.5
    labels, table, depth2 = dsm.depressions(dtm, grid, min_depth=0.5, min_area_m2=50.0)
    assert torch.equal(depth2.view(torch.int32), depth.view(torch.int32))
    m = len(table["area"])
    lab, dep = labels.cpu().numpy(), want["depth"].astype(np.float64)
    assert m == 2 and lab.max() == m and ((dep >= 0.5) | (lab == 0)).all() and dep[80, 100] >= 0.5 and lab[80, 100] == 0
    for k in range(m):
        cells = lab == k + 1
        assert int(table["area"][k]) == cells.sum() >= 4 and float(table["volume"][k]) == dep[cells].sum() * 12.5
        assert float(table["max"][k]) == dep[cells].max()
    rings = dsm.outlines(labels, m, grid)
    path = str(tmp_path / "depressions.geojson")
    assert dsm.write_geojson(path, rings, grid, table) == m
    with open(path) as f:
        doc = json.load(f)
    assert doc["type"] == "FeatureCollection" and len(doc["features"]) == m
    for k, feature in enumerate(doc["features"]):
        assert feature["geometry"]["type"] == "Polygon" and feature["properties"]["label"] == k + 1
        assert feature["properties"]["volume"] == float(table["volume"][k]) and feature["properties"]["area"] == int(table["area"][k])
