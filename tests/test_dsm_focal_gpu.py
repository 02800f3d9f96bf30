"""Focal statistics on the device against the numpy oracle (tests/dsm_focal_oracle.py).  smvs_dsm_focal_build and
smvs_dsm_focal_query are called at their C interface with guard words round the table buffer and every output, the buffer seeded;
the header and the tables are compared entry by entry, wrapped words included, n, s1 and s2 with np.array_equal, mean and var by
their bits, no cell excused.  Then the Python layer end to end."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dsm_focal_oracle as fo
from dsm_testkit import dev, lib, same  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
ND = -999.0
G = 64                                                       # guard bytes / words on both sides of a buffer
DTYPES = {"n": torch.int32, "s1": torch.int64, "s2": torch.int64, "mean": torch.float64, "var": torch.float64}


def _intact(buf, n, fill=77):
    return bool((buf[:G] == fill).all()) and bool((buf[G + n:] == fill).all())


def _build(z, dev, nodata=ND, fill=0x5a, stream=None, compare=True):
    """smvs_dsm_focal_build at its C entry on a seeded, guarded buffer; the header and the three tables against the oracle.
    -> (the guarded buffer, gw, gh)."""
    from satmvs_amd import _lib
    z_d = z if isinstance(z, torch.Tensor) else torch.from_numpy(np.array(z, np.float32)).to(dev)
    gh, gw = z_d.shape
    nbytes = _lib.load().smvs_dsm_focal_table_bytes(gw, gh)
    assert nbytes == fo.layout(gw, gh)["bytes"]
    ws = torch.full((nbytes + 2 * G,), fill, dtype=torch.uint8, device=dev)
    ws[:G] = 77
    ws[G + nbytes:] = 77
    torch.cuda.synchronize()
    _lib.call("smvs_dsm_focal_build", _lib.ptr(z_d), gw, gh, nodata, _lib.ptr(ws[G:]), nbytes, stream if stream is not None else _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert _intact(ws, nbytes), "a guard word changed"
    if compare:
        h, N, S1, S2 = fo.tables(z_d.cpu().numpy(), nodata)
        hdr, gN, g1, g2 = fo.split(ws[G:G + fo.layout(gw, gh)["work"]].cpu().numpy(), gw, gh)
        assert hdr.tolist() == fo.header_words(h).tolist(), (hdr.tolist(), h)
        for name, got, want in (("N", gN, N), ("S1", g1, S1), ("S2", g2, S2)):
            assert np.array_equal(got, want), (name, np.argwhere(got != want)[:3].tolist())
    return ws, gw, gh


def _query(ws, gw, gh, rects, min_valid=1, outputs=fo.OUTPUTS, stream=None, **q):
    """smvs_dsm_focal_query at its C entry on guarded outputs -> dict of numpy arrays and "status"."""
    from satmvs_amd import _lib
    dev = ws.device
    rows, cols = fo._centres(gw, gh, q)
    oh, ow = len(rows), len(cols)
    rects = np.ascontiguousarray(rects, np.int32)
    bufs = {k: torch.full((oh * ow + 2 * G,), 77, dtype=DTYPES[k], device=dev) for k in fo.OUTPUTS}
    status = torch.full((1 + 2 * G,), 77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    _lib.call("smvs_dsm_focal_query", _lib.ptr(ws[G:]), gw, gh, rects.ctypes.data, len(rects), ow, oh, q.get("c0", 0), q.get("r0", 0),
              q.get("sx", 1), q.get("sy", 1), min_valid, *[_lib.ptr(bufs[k][G:]) if k in outputs else None for k in fo.OUTPUTS],
              _lib.ptr(status[G:]), stream if stream is not None else _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert _intact(status, 1) and _intact(ws, ws.numel() - 2 * G), "a guard word changed"
    out = {"status": int(status[G])}
    for k in fo.OUTPUTS:
        assert _intact(bufs[k], oh * ow), "a guard word of %s changed" % k
        if k in outputs:
            a = bufs[k][G:G + oh * ow].cpu().numpy().reshape(oh, ow)
            out[k] = a.view(np.uint64) if k == "s2" else a
        else:
            assert bool((bufs[k] == 77).all()), "%s was written though null" % k
    return out


def _check(dev, z, rects, nodata=ND, min_valid=1, outputs=fo.OUTPUTS, built=None, **q):
    ws, gw, gh = built or _build(z, dev, nodata)
    got = _query(ws, gw, gh, rects, min_valid, outputs, **q)
    want = fo.query_tables(z, rects, nodata, min_valid, **q)
    d = fo.differing(got, want, outputs)
    assert d is None and got["status"] == 0, (d, got["status"])
    return got


@functools.lru_cache(maxsize=None)
def _matrix():
    return fo.matrix()                                       # shared: nobody writes to it


@functools.lru_cache(maxsize=None)
def _scene(gh=67, gw=83, voids=0.05):
    z = fo.kit_scene(gh, gw, seed=7, voids=voids, salt=0.02)
    z.setflags(write=False)
    return z


# ---- grids, values, voids --------------------------------------------------------------------------------------------------------
def test_the_matrix(dev):
    names = [c[0] for c in _matrix()]
    for shape in ("1x1", "1x70", "67x1", "2x2", "67x3"):
        assert "edge %s box1" % shape in names
    assert "scene 257x301 disc 100" in names and "all invalid" in names and "one valid cell" in names
    for name, z, nodata, rects, q in _matrix():
        _check(dev, z, rects, nodata, **q)


@pytest.mark.parametrize("gh,gw", [(fo.BAND - 1, fo.SEG - 1), (fo.BAND, fo.SEG), (fo.BAND + 1, fo.SEG + 1), (2 * fo.BAND - 1, 2 * fo.SEG - 1),
                                   (2 * fo.BAND, 2 * fo.SEG), (2 * fo.BAND + 1, 2 * fo.SEG + 1), (1, 3 * fo.SEG + 5), (5 * fo.BAND + 3, 1)])
def test_round_the_segment_and_the_band(dev, gh, gw):
    """Widths one below, at and one above the row pass's segment (and two of them), heights likewise round the column pass's band.
    The row pass carries a segment's total in registers: there is no second level to outgrow."""
    z = fo.kit_scene(gh, gw, seed=gh + gw, voids=0.1, salt=0.02)
    _check(dev, z, fo.box(2, 1), sx=max(gw // 40, 1), sy=max(gh // 20, 1))


def test_a_tilted_plane_against_its_closed_form_on_the_device(dev):
    """2300 x 2300: q = 128 col + 64 row; the tables' closed forms in int64 on the device, every entry; the mean of a symmetric window
    away from the edges is the cell itself and the variance of a box of width w = 61 is ((128^2 + 64^2) (w^2 - 1) / 12) 2^-16, exactly."""
    n = 2300
    i = torch.arange(n, device=dev, dtype=torch.int64)
    q = 128 * i[None, :] + 64 * i[:, None]
    z = (q.double() / 256.0).float()
    ws, gw, gh = _build(z, dev, compare=False)
    l = fo.layout(n, n)
    e = (n + 1) * (n + 1)
    body = ws[G:]
    hdr = body[:64].view(torch.int64).tolist()
    K = (192 * (n - 1)) >> 1
    assert hdr == [0, 192 * (n - 1), n * n, K, 192 * (n - 1) - K, 0, 0, 0]
    x = torch.arange(n + 1, device=dev, dtype=torch.int64)
    p1, p2 = x * (x - 1) // 2, (x - 1) * x * (2 * x - 1) // 6
    X, Y, P1x, P1y, P2x, P2y = x[None, :], x[:, None], p1[None, :], p1[:, None], p2[None, :], p2[:, None]
    N = X * Y
    S1 = 128 * Y * P1x + 64 * X * P1y - K * N
    S2 = 128 * 128 * Y * P2x + 64 * 64 * X * P2y + K * K * N + 2 * 128 * 64 * P1x * P1y - 2 * 128 * K * Y * P1x - 2 * 64 * K * X * P1y
    assert torch.equal(body[l["n"]:l["n"] + 4 * e].view(torch.int32).view(n + 1, n + 1), N.int())
    assert torch.equal(body[l["s1"]:l["s1"] + 8 * e].view(torch.int64).view(n + 1, n + 1), S1)
    assert torch.equal(body[l["s2"]:l["s2"] + 8 * e].view(torch.int64).view(n + 1, n + 1), S2)
    from satmvs_amd import _lib
    mean = torch.empty((n, n), dtype=torch.float64, device=dev)
    var = torch.empty_like(mean)
    status = torch.ones(1, dtype=torch.int32, device=dev)
    rects = fo.box(30)
    _lib.call("smvs_dsm_focal_query", _lib.ptr(body), n, n, rects.ctypes.data, 1, n, n, 0, 0, 1, 1, 1, None, None, None, _lib.ptr(mean), _lib.ptr(var),
              _lib.ptr(status), _lib.current_stream(dev))
    inner = (slice(30, -30), slice(30, -30))
    assert int(status) == 0 and torch.equal(mean[inner], z.double()[inner])
    assert bool((var[inner] == (128 * 128 + 64 * 64) * ((61 * 61 - 1) // 12) / 65536.0).all())       # 3720 / 12 = 310: exact


@pytest.mark.parametrize("voids", [0.0, 0.05, 0.3])
def test_the_scene_with_voids_and_salt(dev, voids):
    z = fo.kit_scene(120, 141, seed=9, voids=voids, salt=0.03)
    _check(dev, z, fo.disc(4.5))


def test_edge_values(dev):
    """Halves of the quantum, both zeros, NaN, +-Inf, nodata, +-32768 and one ulp beyond."""
    z = fo.edge_values(40, 50, seed=1)
    ok, q = fo.quantise(z)
    assert ok.sum() < z.size and q[ok].max() == 1 << 23 and q[ok].min() == -(1 << 23) and (np.abs(z) > 32768).any()
    assert (np.abs(np.abs(z[ok].astype(np.float64) * 256) % 1 - 0.5) == 0).sum() > 100           # on halves
    got = _check(dev, z, fo.box(1))
    assert got["s1"].any()
    _check(dev, z, fo.disc(6), min_valid=0)


def test_wrapped_tables_stay_exact(dev):
    """A 600 x 600 checkerboard of +-32768 m: S2 wraps past 2^64 (360 000 x 2^46), a 361 x 361 box (130 321 < 2^17 cells) is exact
    with status 0, a 363 x 363 box (131 769 cells) sets status and is refused by the Python layer before any query."""
    from satmvs_amd import dsm
    z = fo.checkerboard(600, 600)
    built = _build(z, dev)
    _, _, _, S2 = fo.tables(z)
    assert int(S2[600, 600]) == (360000 << 46) % fo.MOD and 360000 << 46 > fo.MOD
    got = _check(dev, z, fo.box(180), built=built, c0=3, r0=1, sx=7, sy=11)
    assert int(got["n"].max()) == 130321 and int(got["s2"].max()) == 130321 << 46
    assert _query(*built, fo.box(181), c0=300, r0=300, ow=1, oh=1)["status"] == 1
    assert _query(*built, fo.box(180), c0=300, r0=300, ow=1, oh=1)["status"] == 0
    tables = dsm.focal_tables(z)
    assert (tables.qmin, tables.qmax, tables.n_valid, tables.centre, tables.max_abs) == (-(1 << 23), 1 << 23, 360000, 0, 1 << 23)
    assert np.array_equal(dsm.focal_sums(tables, fo.box(180), origin=(300, 300), shape=(1, 1))["s2"], [[130321 << 46]])
    with pytest.raises(ValueError, match="may wrap"):
        dsm.focal_sums(tables, fo.box(181))


# ---- windows ---------------------------------------------------------------------------------------------------------------------
WINDOWS = {"box 0": fo.box(0), "box 1": fo.box(1), "box 31": fo.box(31), "box 2047": fo.box(2047), "box 4096 x 0": fo.box(4096, 0),
           "box 0 x 4096": fo.box(0, 4096), "wide": fo.box(40, 0), "tall": fo.box(0, 70),
           "asymmetric": np.array([[-5, 1, 2, 3, 1], [0, 9, -7, -7, 1], [-60, -50, -60, 60, 1]], np.int32),
           "disc 1": fo.disc(1), "disc 2.5": fo.disc(2.5), "disc 100": fo.disc(100), "annulus": fo.annulus(9, 4.5), "1024 records": fo.many_records(1024)}


@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_window_shapes(dev, name):
    _check(dev, _scene(), WINDOWS[name])


def test_a_box_of_radius_4096_is_too_large(dev):
    """8193^2 cells are more than the 2^24 a window's positive records may hold: the offsets allow the radius, the area does not.  The
    widest square box is that of radius 2047 (4095^2 cells), and +-4096 is reached by the flat boxes above."""
    from satmvs_amd import _lib
    assert 4095 ** 2 <= fo.MAX_AREA < 4097 ** 2
    ws, gw, gh = _build(_scene(), dev)
    with pytest.raises(_lib.SatMVSNativeError, match="window too large"):
        _query(ws, gw, gh, fo.box(4096))


def test_1025_records_are_rejected(dev):
    from satmvs_amd import _lib, dsm
    ws, gw, gh = _build(_scene(), dev)
    with pytest.raises(_lib.SatMVSNativeError, match="n_rects must be"):
        _query(ws, gw, gh, fo.many_records(1025))
    with pytest.raises(ValueError, match="1 .. 1024 records"):
        dsm.focal_sums(dsm.focal_tables(_scene()), fo.many_records(1025))


def test_discs_of_the_python_layer_on_the_large_grid(dev):
    from satmvs_amd import dsm
    z = fo.kit_scene(257, 301, seed=5, voids=0.05, salt=0.01)
    built = _build(z, dev)
    for w in (dsm.focal_window("disc", 100), dsm.focal_window("annulus", 60.0, 25.0, dsm.DSMGrid(0.0, 0.0, 5.0, 2.5, 301, 257))):
        _check(dev, z, w.rects, built=built, sx=2, sy=3, c0=1)


# ---- strides, origins, min_valid -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [{"sx": 4, "sy": 4}, {"sx": 5, "sy": 3}, {"sx": 83, "sy": 67}, {"c0": 82, "r0": 66, "ow": 1, "oh": 1},
                               {"c0": 2, "r0": 1, "sx": 8, "sy": 13, "ow": 11, "oh": 6}, {"c0": 80, "sx": 1, "ow": 3, "oh": 67}])
def test_strides_and_origins(dev, q):
    """Block aggregation with a last partial block (83 = 20 x 4 + 3, 67 = 16 x 4 + 3), an output centre on the last cell."""
    f = q.get("sx", 1)
    _check(dev, _scene(), np.array([[0, f - 1, 0, q.get("sy", 1) - 1, 1]], np.int32), **q)
    _check(dev, _scene(), fo.disc(3), **q)


@pytest.mark.parametrize("min_valid", [0, 1, 9])
def test_min_valid(dev, min_valid):
    z = _scene(voids=0.3)
    got = _check(dev, z, fo.box(1), min_valid=min_valid)
    assert np.array_equal(np.isnan(got["mean"]), got["n"] < max(min_valid, 1)) and np.isnan(got["mean"]).any() and (got["n"] == 0).any()


# ---- call variations -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outputs", [(), ("n",), ("s1",), ("s2",), ("mean",), ("var",), ("n", "var"), fo.OUTPUTS])
def test_every_output_null_and_not(dev, outputs):
    _check(dev, _scene(), fo.disc(2.5), outputs=outputs)


@pytest.mark.parametrize("fill", [0xff, 0x00, 0x5a])
def test_the_buffer_is_initialised_by_the_build(dev, fill):
    z = _scene()
    built = _build(z, dev, fill=fill)
    _check(dev, z, fo.box(2), built=built)


def test_side_stream_order_of_calls_and_equal_bits(dev):
    from satmvs_amd import _lib
    big, small = fo.kit_scene(130, 257, seed=2, voids=0.1), _scene()
    side = torch.cuda.Stream(dev)
    handle = C.c_void_p(side.cuda_stream)
    built = _build(big, dev, stream=handle)
    first = _query(*built, fo.disc(5), stream=handle)
    assert fo.differing(first, fo.query_tables(big, fo.disc(5))) is None
    again_small = _build(small, dev, stream=handle)           # a larger call before a smaller one
    got = _query(*again_small, fo.disc(5), stream=handle)
    assert fo.differing(got, fo.query_tables(small, fo.disc(5))) is None
    rebuilt = _build(big, dev)
    assert torch.equal(rebuilt[0][G:G + fo.layout(257, 130)["work"]], built[0][G:G + fo.layout(257, 130)["work"]])
    second = _query(*rebuilt, fo.disc(5))
    assert fo.differing(second, first) is None and _query(*built, fo.box(1))["status"] == 0


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def _grid(z, res=5.0):
    from satmvs_amd import dsm
    return dsm.DSMGrid(1000.0, 2000.0, res, res, z.shape[1], z.shape[0])


def _cast_within(got, want, keep, nodata=ND, eps=2.0 ** -50):
    """got (float32) is the cast of a float64 value within eps relative of `want` where keep, nodata elsewhere."""
    assert got.dtype == np.float32 and np.all(got[~keep] == np.float32(nodata))
    w = want[keep]
    lo, hi = (w - np.abs(w) * eps).astype(np.float32), (w + np.abs(w) * eps).astype(np.float32)
    assert np.all((lo <= got[keep]) & (got[keep] <= hi)), int(((lo > got[keep]) | (got[keep] > hi)).sum())


def test_sums_and_stats_with_numpy_and_device_tensors(dev):
    from satmvs_amd import dsm
    z = _scene()
    w = dsm.focal_window("disc", 3)
    want = fo.query_tables(z, w.rects)
    for src in (z, torch.from_numpy(z.copy()).to(dev)):
        tables = dsm.focal_tables(src)
        h = want["h"]
        assert (tables.qmin, tables.qmax, tables.n_valid, tables.centre, tables.max_abs) == (h["qmin"], h["qmax"], h["n_valid"], h["c"], h["D"])
        sums, stats = dsm.focal_sums(tables, w), dsm.focal_stats(tables, w)
        direct = dsm.focal_stats(src, w)
        for out in (sums, stats, direct):
            for k, v in out.items():
                if k != "centre":
                    assert isinstance(v, torch.Tensor) == isinstance(src, torch.Tensor) and (not isinstance(v, torch.Tensor) or v.device == src.device), k
        host = lambda d: {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
        sums, stats, direct = host(sums), host(stats), host(direct)
        sums["s2"] = sums["s2"].view(np.uint64)
        assert sums["centre"] == h["c"] and fo.differing(sums, want, ("n", "s1", "s2")) is None
        assert fo.differing(stats, want, ("n", "mean", "var")) is None and fo.differing(direct, want, ("n", "mean", "var")) is None
        ok = ~np.isnan(want["var"])
        assert np.array_equal(np.isnan(stats["std"]), ~ok)
        assert np.all(np.abs(stats["std"][ok] - np.sqrt(stats["var"][ok])) <= 2.0 ** -50 * np.sqrt(stats["var"][ok]))
    strided = dsm.focal_sums(dsm.focal_tables(z), fo.box(1), stride=(3, 4), origin=(1, 2))
    assert fo.differing({**strided, "s2": strided["s2"].view(np.uint64)}, fo.query_tables(z, fo.box(1), sx=4, sy=3, c0=2, r0=1), ("n", "s1", "s2")) is None


@pytest.mark.parametrize("inner,min_valid", [(None, 1), (10.0, 5)])
def test_tpi_dev_roughness_and_focal_mean(dev, inner, min_valid):
    """Against the float64 statement on the device's own mean and var, within 2^-50 relative before the cast to float32 (sqrt, the
    difference and the quotient run in torch)."""
    from satmvs_amd import dsm
    z = _scene(voids=0.3)
    grid = _grid(z)
    w = dsm.focal_window("disc" if inner is None else "annulus", 25.0, inner, grid)
    stats = dsm.focal_stats(z, w, min_valid)
    assert fo.differing(stats, fo.query_tables(z, w.rects, min_valid=min_valid), ("n", "mean", "var")) is None
    t, std, keep = fo.tpi_terms(z, stats["n"], stats["mean"], stats["var"], ND, min_valid)
    enough = stats["n"] >= max(min_valid, 1)
    assert keep.any() and (~keep).any()
    _cast_within(dsm.tpi(z, grid, 25.0, inner, min_valid), t, keep)
    with np.errstate(invalid="ignore", divide="ignore"):
        _cast_within(dsm.dev(z, grid, 25.0, inner, min_valid), t / std, keep & (std > 0))
    _cast_within(dsm.roughness(z, w, min_valid), std, enough)
    _cast_within(dsm.focal_mean(z, w, min_valid), stats["mean"], enough, eps=0.0)
    z_d = torch.from_numpy(z.copy()).to(dev)
    got = dsm.tpi(z_d, grid, 25.0, inner, min_valid, tables=dsm.focal_tables(z_d))
    assert isinstance(got, torch.Tensor) and got.device == z_d.device
    same(got.cpu().numpy(), dsm.tpi(z, grid, 25.0, inner, min_valid), "tpi from device tensors")


def test_focal_fraction_of_object_footprints(dev):
    from satmvs_amd import dsm
    z = fo.kit_scene(90, 110, seed=4)
    objects = (np.nan_to_num(z, nan=0.0) > 140.0)
    assert 0 < objects.sum() < objects.size
    w = dsm.focal_window("disc", 4)
    want = fo.query_tables(objects.astype(np.float32), w.rects)
    count = (want["s1"] + want["n"].astype(np.int64) * want["h"]["c"]) >> 8
    inside = fo.query_tables(np.ones(objects.shape, np.float32), w.rects)["n"]
    assert np.array_equal(want["n"], inside)
    for mask in (objects, objects.astype(np.uint8) * 7, torch.from_numpy(objects).to(dev)):
        got = dsm.focal_fraction(mask, w)
        got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
        assert got.dtype == np.float64 and np.array_equal(got, count.astype(np.float64) / inside.astype(np.float64))
    assert got.min() == 0.0 and got.max() == 1.0


@pytest.mark.parametrize("factor", [2, 3, 8])
def test_aggregate(dev, factor):
    from satmvs_amd import dsm
    z = _scene(voids=0.3)
    grid = _grid(z, 2.5)
    for min_valid in (1, factor * factor):
        got, coarse, count = dsm.aggregate(z, grid, factor, min_valid)
        want, n = fo.block_mean(z, factor, ND, min_valid)
        same(got, want, "aggregate %d" % factor)
        assert np.array_equal(count, n)
    assert (got == ND).any()                                 # whole blocks asked for, 30 % voids
    assert got.shape == (-(-67 // factor), -(-83 // factor)) and (coarse.width, coarse.height) == got.shape[::-1]
    assert (coarse.xres, coarse.yres) == (2.5 * factor, 2.5 * factor)
    assert coarse.e0 == grid.e0 + (factor - 1) / 2 * 2.5 and coarse.n0 == grid.n0 - (factor - 1) / 2 * 2.5


def test_slope_position(dev):
    from satmvs_amd import dsm
    z = fo.kit_scene(90, 110, seed=6, voids=0.05, salt=0.01)
    grid = _grid(z)
    got = dsm.slope_position(z, grid, 40.0, slope_deg=5.0)
    want = fo.slope_codes(dsm.dev(z, grid, 40.0), dsm.slope(z, grid), 5.0)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert {0, 1, 6} <= set(np.unique(got).tolist()) <= set(range(7))           # voids, and the salt noise as valleys and ridges
    assert len(dsm.SLOPE_POSITIONS) == 7


def test_dtm_to_tpi_to_label_stats(dev):
    from satmvs_amd import dsm
    z = fo.kit_scene(90, 110, seed=8, voids=0.02)
    grid = _grid(z)
    dtm = dsm.extract_dtm(z, grid)
    t = dsm.tpi(dtm, grid, 30.0)
    ok = np.isfinite(dtm) & (dtm != ND)
    assert ok.any() and np.array_equal(t != ND, ok) and np.isfinite(t).all()
    labels, n = dsm.label(ok)
    stats = dsm.label_stats(labels, n, values=t, grid=grid)
    assert n >= 1 and int(np.asarray(stats["n_valid"]).sum()) == int(ok.sum())
