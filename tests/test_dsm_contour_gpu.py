"""Contours on the device against the numpy oracle (tests/dsm_contour_oracle.py): every entry of the line table and the vertex
list is compared for equality, the float64 coordinates by their bits, no line or vertex excused; length_m, a sum of square roots
taken by torch on the device, is held to the bound derived at _same_on_grid and to equal bits from run to run.

Sizes.  The kernels run 256 lanes a workgroup over the lattice edges (2 gw gh slots), the crossings and the lines, and scan them
in blocks of 2048 on three levels.  SIZES holds the issue's grids and three whose edge counts are 2046, 2048 and 2050
(11 x 93, 32 x 32, 25 x 41).  The 2300 x 2300 plane has more than 2048^2 edge slots, so the second level of the scan holds more
than one block; the serpentine at 257 x 301 is one ring of more than 2^16 vertices: 17 rounds of the doubling."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

import dsm_contour_oracle as co
from dsm_testkit import dev, scene as kit_scene  # noqa: F401  (dev: fixture)

pytestmark = pytest.mark.gpu
SIZES = [(1, 1), (1, 70), (67, 1), (2, 2), (67, 3), (128, 160), (257, 301), (11, 93), (32, 32), (25, 41)]
LEVELS_M = [9.7, 12.3, 15.0, 18.0, 20.5, 23.25, 26.1, 31.0]
G = 64                                                       # guard words on both sides of an output


def _grid(dsm, gh, gw):
    return dsm.DSMGrid(500000.0, 3400000.0, 5.0, 2.5, gw, gh)


def _same_on_grid(got, want, what):
    """same_lines for everything but length_m, which is held to a bound: the device's float64 square root is within one ulp
    (2^-52 relative) where numpy's is correctly rounded (2^-53), and both add a line's m segments one after the other, each
    partial sum within 2^-53 of itself, so the two totals differ by at most (2^-52 + 2^-53 + 2 m 2^-53) <= (m + 2) 2^-52 of the
    total."""
    co.same_lines({k: v for k, v in got.items() if k != "length_m"}, {k: v for k, v in want.items() if k != "length_m"}, what)
    m = np.diff(want["offset"]).astype(np.float64)
    assert got["length_m"].dtype == np.float64 and got["length_m"].shape == want["length_m"].shape, what
    assert (np.abs(got["length_m"] - want["length_m"]) <= (m + 2.0) * 2.0 ** -52 * want["length_m"]).all(), what


def _check(z, levels_m, what, want=None):
    """dsm.contours of a DSM against the oracle's trace (or `want`), with and without a grid."""
    from satmvs_amd import dsm
    z = np.ascontiguousarray(z, np.float32)
    gh, gw = z.shape
    grid = _grid(dsm, gh, gw)
    if want is None:
        want = co.trace(z, co.level_keys(np.sort(levels_m)))
    got = dsm.contours(z, levels=levels_m, grid=grid)
    assert all(isinstance(t, np.ndarray) for t in got.values())
    _same_on_grid(got, co.with_grid(want, grid), what)
    assert sorted(got) == sorted(co.KEYS + ("vertices_en", "length_m"))
    bare = dsm.contours(z, levels=levels_m)
    co.same_lines(bare, want, (what, "without a grid"))
    assert sorted(bare) == sorted(co.KEYS)
    return got


@functools.lru_cache(maxsize=None)
def _scene(gh, gw, voids):
    E, N = 5.0 * np.mgrid[0:gh, 0:gw][1], -2.5 * np.mgrid[0:gh, 0:gw][0]
    z = kit_scene(E, N, seed=gh + gw, voids=voids, base=20.0, amp=8.0)
    z += (3.0 * np.random.default_rng(gw).standard_normal((gh, gw))).astype(np.float32)          # noise of a few metres
    return z


# ---- sizes, voids ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SIZES)
def test_sizes(dev, shape):
    got = _check(co.random_scene(*shape, seed=shape[0] + shape[1]), LEVELS_M, shape)
    if min(shape) >= 25:
        assert got["closed"].any() and not got["closed"].all()
    if min(shape) == 1:
        assert len(got["closed"]) == 0


@pytest.mark.parametrize("voids", [0.0, 0.05, 0.3])
def test_test_kit_scene(dev, voids):
    got = _check(_scene(128, 160, voids), LEVELS_M + [40.0, 55.0], voids)
    assert len(got["closed"]) > 100


# ---- levels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4096, 4097])
def test_level_counts(dev, n):
    """n levels in one call (4097: two native passes behind dsm.contours), the lowest below and the highest above every height."""
    z = co.random_scene(16, 19, seed=5, voids=0.03)
    lo, hi = float(np.nanmin(np.where(z == -999.0, np.nan, z))), float(np.nanmax(z))
    levels = np.linspace(lo - 1.0, hi + 1.0, n) if n > 1 else np.array([0.5 * (lo + hi)])
    got = _check(z, levels, n)
    if n > 1:
        assert got["first_line"][1] == 0 and got["first_line"][-2] == got["first_line"][-1] == len(got["closed"])
    assert len(got["first_line"]) == n + 1 and (len(got["closed"]) > 0) == (n != 2)


def test_cliff_whose_edges_carry_4096_crossings(dev):
    z = np.zeros((6, 8), np.float32)
    z[:, 4:] = 100.0
    levels = (np.arange(4096) + 1.0) * (100.0 / 4097.0)
    assert co.n_cross(z, co.level_keys(levels)) == 6 * 4096
    got = _check(z, levels, "cliff")
    assert len(got["closed"]) == 4096 and not got["closed"].any() and (np.diff(got["offset"]) == 6).all()
    assert (got["edge"].reshape(4096, 6) == 2 * (np.arange(6) * 8 + 3)).all()


# ---- long and large ------------------------------------------------------------------------------------------------------------------
def test_serpentine_ring(dev):
    got = _check(co.serpentine(257, 301), [5.0], "serpentine")
    assert got["closed"].tolist() == [True] and len(got["vertices"]) > 2 ** 16


def test_large_plane_closed_form(dev):
    """2300 x 2300 on the device only: z = col / 4, 64 levels between columns: every line runs south down its column gap, 2300
    vertices at x = col + 65 / 128 (K = 128 col + 65 against 2 q = 128 col and 128 col + 128)."""
    from satmvs_amd import dsm
    g, n = 2300, 64
    cols = torch.arange(n, device=dev) * 35 + 7
    z = (torch.arange(g, device=dev, dtype=torch.float32) * 0.25).repeat(g, 1).contiguous()
    got = dsm.contours(z, levels=(cols.double().cpu().numpy() + 0.5) * 0.25)
    assert all(t.is_cuda for t in got.values())
    rows = torch.arange(g, device=dev)
    assert torch.equal(got["offset"], (torch.arange(n + 1, device=dev) * g).to(torch.int32)) and not bool(got["closed"].any())
    assert torch.equal(got["level_index"], torch.arange(n, device=dev, dtype=torch.int32)) and torch.equal(got["first_line"], torch.arange(n + 1, device=dev, dtype=torch.int32))
    want = torch.stack([(cols.double() + 65.0 / 128.0)[:, None].expand(n, g), rows.double()[None, :].expand(n, g)], dim=2).reshape(-1, 2)
    assert torch.equal(got["vertices"].view(torch.int64), want.contiguous().view(torch.int64))
    assert torch.equal(got["edge"], (2 * (rows[None, :] * g + cols[:, None])).reshape(-1).to(torch.int32))
    assert torch.equal(got["level"], (128 * cols + 65).double() / 512.0)


# ---- extreme heights -----------------------------------------------------------------------------------------------------------------
def test_extreme_heights(dev):
    z = co.random_scene(9, 11, seed=77)
    top = np.float32(32768.0)
    z[0, :4] = [np.inf, -np.inf, top, np.nextafter(top, np.float32(np.inf))]
    z[1, :5] = [-top, 0.0, -0.0, np.float32(20.0) + np.float32(1.0 / 512.0), np.float32(20.0) + np.float32(3.0 / 512.0)]   # quantisation halves
    z[2, :3] = [np.nan, -999.0, np.nextafter(-top, np.float32(-np.inf))]
    z[5:8, 5:8] = 20.0
    z[6, 6] = -top                                           # a pit as deep as the rule admits: a ring at the lowest level
    got = _check(z, [-32768.0, -20000.0, -0.001, 0.0, 19.99, 20.0, 20.004, 30000.0, 32767.99], "extreme")
    assert got["level"].min() == (-2 ** 24 + 1) / 512.0 and len(got["closed"]) > 8
    assert len(_check(z, [32768.0], "above every height")["closed"]) == 0
    other = np.where(z == -999.0, np.float32(7.0), z)
    other[3, 3] = 12.5
    from satmvs_amd import dsm
    co.same_lines(dsm.contours(other, levels=LEVELS_M, nodata=12.5), co.trace(other, co.level_keys(LEVELS_M), nodata=12.5), "another nodata")


# ---- the C entries: guard words, workspaces full of anything --------------------------------------------------------------------------
def _native(dev, z, K, fill=0xff, spare=0):
    """smvs_dsm_contour_count twice and smvs_dsm_contour_write (twice: it may be repeated) on raw pointers with guarded, seeded
    outputs and a guarded workspace -> the dict, numpy, and n_cross."""
    from satmvs_amd import _lib
    lib = _lib.load()
    gh, gw = z.shape
    zd = torch.from_numpy(np.ascontiguousarray(z, np.float32)).to(dev)
    K = np.ascontiguousarray(K, np.int32)
    kp, n = K.ctypes.data_as(ctypes.c_void_p), len(K)
    stream = _lib.current_stream(dev)
    counts = torch.full((3 + 2 * G,), 77, dtype=torch.int32, device=dev)

    def workspace(max_cross):
        nbytes = lib.smvs_dsm_contour_workspace_bytes(gw, gh, n, max_cross)
        ws = torch.full((nbytes + 512,), fill, dtype=torch.uint8, device=dev)
        ws[:256], ws[256 + nbytes:] = 0xa7, 0xa7
        return ws, nbytes

    ws, nbytes = workspace(0)
    _lib.call("smvs_dsm_contour_count", _lib.ptr(zd), gw, gh, -999.0, kp, n, 0, _lib.ptr(counts[G:]), _lib.ptr(ws[256:]), nbytes, stream)
    nc = int(counts[G].item())
    assert counts[G + 1:G + 3].tolist() == [0, 0] and bool((ws[:256] == 0xa7).all()) and bool((ws[256 + nbytes:] == 0xa7).all())
    ws, nbytes = workspace(nc)
    _lib.call("smvs_dsm_contour_count", _lib.ptr(zd), gw, gh, -999.0, kp, n, nc, _lib.ptr(counts[G:]), _lib.ptr(ws[256:]), nbytes, stream)
    assert bool((counts[:G] == 77).all()) and bool((counts[G + 3:] == 77).all())
    nc2, nl, nv = counts[G:G + 3].tolist()
    assert nc2 == nc
    spec = {"level_index": (torch.int32, nl), "closed": (torch.uint8, nl), "offset": (torch.int32, nl + 1), "first_line": (torch.int32, n + 1),
            "vertices": (torch.float64, 2 * nv), "edge": (torch.int32, nv)}
    out = None
    for again in range(2):
        bufs = {k: torch.full((m + 2 * G,), 77, dtype=dt, device=dev) for k, (dt, m) in spec.items()}
        _lib.call("smvs_dsm_contour_write", _lib.ptr(zd), gw, gh, -999.0, kp, n, nc, nl, nv, *[_lib.ptr(bufs[k][G:]) for k in spec],
                  _lib.ptr(ws[256:]), nbytes, stream)
        torch.cuda.synchronize()
        for k, (dt, m) in spec.items():
            assert bool((bufs[k][:G] == 77).all()) and bool((bufs[k][G + m:] == 77).all()), k
        assert bool((ws[:256] == 0xa7).all()) and bool((ws[256 + nbytes:] == 0xa7).all())
        now = {k: bufs[k][G:G + m].cpu().numpy() for k, (dt, m) in spec.items()}
        assert out is None or all(np.array_equal(now[k], out[k]) for k in now)
        out = now
    out["vertices"], out["closed"] = out["vertices"].reshape(nv, 2), out["closed"].astype(bool)
    out["level"] = K.astype(np.float64)[out["level_index"]] / 512.0
    return out, nc


def test_entries_keep_to_their_outputs(dev):
    z = co.random_scene(97, 131, seed=4, voids=0.08)
    K = co.level_keys(LEVELS_M)
    want = co.trace(z, K)
    for fill in (0xff, 0x00, 0x5a):
        got, nc = _native(dev, z, K, fill)
        co.same_lines(got, want, "workspace full of 0x%02x" % fill)
        assert nc == co.n_cross(z, K) > len(want["vertices"])                            # the dropped crossings are counted
    one, nc = _native(dev, np.array([[0.0, 1.0], [np.nan, np.nan]], np.float32), co.level_keys([0.5]))
    assert nc == 1 and len(one["closed"]) == 0                                           # a lone crossing: no doubling round, no line


def test_more_crossings_than_room(dev, monkeypatch):
    from satmvs_amd import _lib, dsm
    lib = _lib.load()
    z = co.random_scene(20, 21, seed=6)
    K = np.ascontiguousarray(co.level_keys(LEVELS_M), np.int32)
    nc = co.n_cross(z, K)
    zd = torch.from_numpy(z).to(dev)
    counts = torch.zeros(3, dtype=torch.int32, device=dev)
    nbytes = lib.smvs_dsm_contour_workspace_bytes(21, 20, len(K), nc - 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.call("smvs_dsm_contour_count", _lib.ptr(zd), 21, 20, -999.0, K.ctypes.data_as(ctypes.c_void_p), len(K), nc - 1, _lib.ptr(counts), _lib.ptr(ws),
              nbytes, _lib.current_stream(dev))
    assert counts.tolist() == [-1, -1, -1]
    real = dsm._call

    def short(dev_, name, *args):                            # the second count call finds one crossing more than it has room for
        if name == "smvs_dsm_contour_count" and args[6] > 0:
            args = args[:6] + (args[6] - 1,) + args[7:]
        real(dev_, name, *args)

    monkeypatch.setattr(dsm, "_call", short)
    with pytest.raises(_lib.SatMVSNativeError, match="gave up"):
        dsm.contours(z, levels=LEVELS_M)


# ---- determinism, streams, device tensors ---------------------------------------------------------------------------------------
def test_deterministic_streams_and_device_tensors(dev):
    from satmvs_amd import dsm
    big, small = co.random_scene(300, 340, seed=1, voids=0.02), co.random_scene(40, 50, seed=2)
    K = co.level_keys(LEVELS_M)
    grid = _grid(dsm, 300, 340)
    bd, sd = torch.from_numpy(big).to(dev), torch.from_numpy(small).to(dev)
    keep = bd.clone()
    a = dsm.contours(bd, levels=LEVELS_M, grid=grid)         # a larger call before a smaller one
    s = dsm.contours(sd, levels=LEVELS_M)
    b = dsm.contours(bd, levels=LEVELS_M, grid=grid)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        c = dsm.contours(bd, levels=torch.tensor(LEVELS_M[::-1], dtype=torch.float64), grid=grid)             # any order, a tensor
    side.synchronize()
    assert torch.equal(bd.view(torch.int32), keep.view(torch.int32))
    for k in a:
        assert a[k].is_cuda and b[k].is_cuda and c[k].is_cuda, k
        for other in (b, c):
            x, y = a[k], other[k]
            if x.dtype == torch.float64:
                x, y = x.view(torch.int64), y.view(torch.int64)
            assert x.dtype == y.dtype and torch.equal(x, y), k
    _same_on_grid({k: t.cpu().numpy() for k, t in a.items()}, co.with_grid(co.trace(big, K), grid), "device tensors")
    co.same_lines({k: t.cpu().numpy() for k, t in s.items()}, co.trace(small, K), "the smaller call")
    assert dsm.contour_levels(bd, 2.5).tolist() == dsm.contour_levels(big, 2.5).tolist() == co.levels_for(big, 2.5).tolist()
    co.same_lines(dsm.contours(big.astype(np.float64), interval=2.5, base=0.5), co.trace(big, co.level_keys(co.levels_for(big, 2.5, 0.5))), "interval")


def test_native_argument_rejections(dev):
    from satmvs_amd import _lib
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    gw, gh = 9, 7
    z = torch.zeros((gh, gw), dtype=torch.float32, device=dev)
    z[:, 4:] = 10.0
    lv = np.array([-3, 1, 5], np.int32)
    nbytes = lib.smvs_dsm_contour_workspace_bytes(gw, gh, 3, 64)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.zeros(3, dtype=torch.int32, device=dev)
    out = {k: torch.zeros(256, dtype=torch.int64, device=dev) for k in ("level", "closed", "offset", "first", "vertices", "edge")}
    p, null, host = _lib.ptr, ctypes.c_void_p(0), lambda a: a.ctypes.data_as(ctypes.c_void_p)
    i32 = lambda a: np.array(a, np.int32)                    # noqa: E731

    def count(dsm=p(z), gw=gw, gh=gh, levels=lv, n=3, max_cross=64, counts=p(counts), ws=p(ws), nbytes=nbytes):
        _lib.call("smvs_dsm_contour_count", dsm, gw, gh, -999.0, null if levels is None else host(levels), n, max_cross, counts, ws, nbytes, stream)

    def write(dsm=p(z), gw=gw, gh=gh, levels=lv, n=3, nc=64, nl=2, nv=8, level=p(out["level"]), closed=p(out["closed"]), offset=p(out["offset"]),
              first=p(out["first"]), vertices=p(out["vertices"]), edge=p(out["edge"]), ws=p(ws), nbytes=nbytes):
        _lib.call("smvs_dsm_contour_write", dsm, gw, gh, -999.0, null if levels is None else host(levels), n, nc, nl, nv, level, closed, offset, first,
                  vertices, edge, ws, nbytes, stream)

    both = [dict(dsm=null), dict(levels=None), dict(ws=null), dict(gw=0), dict(gh=-1), dict(gw=2 ** 15, gh=2 ** 14), dict(n=0), dict(n=4097),
            dict(levels=i32([1, 2, 5])), dict(levels=i32([1, 1, 5])), dict(levels=i32([5, 3, 7])), dict(levels=i32([1, 3, 2 ** 25 + 1])),
            dict(nbytes=nbytes - 1), dict(ws=p(z))]
    bad = [(count, kw) for kw in both] + [(write, kw) for kw in both] + [
        (count, dict(counts=null)), (count, dict(max_cross=-1)), (count, dict(counts=p(z))), (count, dict(counts=p(ws))),
        (write, dict(offset=null)), (write, dict(first=null)), (write, dict(level=null)), (write, dict(closed=null)), (write, dict(vertices=null)),
        (write, dict(nc=-1)), (write, dict(nl=-1)), (write, dict(nv=-1)), (write, dict(nl=0)), (write, dict(nv=0)), (write, dict(nv=65)), (write, dict(nl=5)),
        (write, dict(level=p(z))), (write, dict(closed=p(out["level"]))), (write, dict(offset=p(ws))), (write, dict(first=p(out["offset"]))),
        (write, dict(vertices=p(out["first"]))), (write, dict(edge=p(out["vertices"])))]
    for fn, kw in bad:
        with pytest.raises(_lib.SatMVSNativeError, match="code 1"):
            fn(**kw)
    torch.cuda.synchronize()
    count()                                                  # and the same arguments unchanged are accepted
    write(nc=0, nl=0, nv=0, level=null, closed=null, vertices=null, edge=null)
    torch.cuda.synchronize()
    assert counts.tolist() == [14, 2, 14] and out["offset"][0].item() == 0


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_dtm_to_geojson(dev, tmp_path):
    """extract_dtm -> contours(interval) -> write_contours -> read back with json: a feature per line, closed features closed,
    and length_m against the float64 sum over the written coordinates."""
    from satmvs_amd import dsm
    gh, gw = 96, 120
    grid = dsm.DSMGrid(400000.0, 3500000.0, 5.0, 2.5, gw, gh)
    E, N = grid.e0 + 5.0 * np.mgrid[0:gh, 0:gw][1], grid.n0 - 2.5 * np.mgrid[0:gh, 0:gw][0]
    zd = torch.from_numpy(kit_scene(E, N, holes=False)).to(dev)
    dtm = dsm.extract_dtm(zd, grid)
    lines = dsm.contours(dtm, interval=2.5, grid=grid)
    assert all(t.is_cuda for t in lines.values())
    n_lines = int(lines["closed"].numel())
    assert n_lines > 5 and int(lines["offset"][-1]) == lines["vertices"].shape[0]
    want = co.with_grid(co.trace(dtm.cpu().numpy(), co.level_keys(co.levels_for(dtm.cpu().numpy(), 2.5))), grid)
    _same_on_grid({k: t.cpu().numpy() for k, t in lines.items()}, want, "the DTM's contours")
    path = str(tmp_path / "contours.geojson")
    assert dsm.write_contours(path, lines, grid) == n_lines
    with open(path) as f:
        doc = json.load(f)
    assert doc["type"] == "FeatureCollection" and len(doc["features"]) == n_lines
    for i, feature in enumerate(doc["features"]):
        xy = np.array(feature["geometry"]["coordinates"], np.float64)
        prop = feature["properties"]
        assert feature["geometry"]["type"] == "LineString" and prop["closed"] == bool(lines["closed"][i]) and prop["level_m"] == float(lines["level"][i])
        if prop["closed"]:
            assert (xy[0] == xy[-1]).all()
        m = len(xy)
        total = np.sqrt((np.diff(xy, axis=0) ** 2).sum(axis=1)).sum()
        assert abs(prop["length_m"] - total) <= (m + 2) * 2.0 ** -52 * total and prop["length_m"] == float(lines["length_m"][i])
        assert m == int(lines["offset"][i + 1] - lines["offset"][i]) + int(prop["closed"])
