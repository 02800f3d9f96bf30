"""The focal statistics without a device: the two statements of the rule (tests/dsm_focal_oracle.py) against each other, closed
forms, the windows of satmvs_amd.dsm.focal_window against a brute-force membership test, scipy's uniform filter, block means, the
host-side overflow check, every Python and C argument rejection (host checks: no device), and five planted mistakes that the
comparison has to report."""
import ctypes as C

import numpy as np
import pytest
import torch

import dsm_focal_oracle as fo
from dsm_testkit import lib  # noqa: F401  (fixture)
from satmvs_amd import dsm
from satmvs_amd.dsm import DSMGrid, FocalTables, FocalWindow, focal_window


# ---- the two statements ----------------------------------------------------------------------------------------------------------
def test_the_two_statements_agree():
    seen = 0
    for name, z, nodata, rects, q in fo.matrix(large=False):
        a = fo.query_direct(z, rects, nodata, **q)
        for exact in (False, True):
            b = fo.query_tables(z, rects, nodata, exact=exact, **q)
            assert fo.differing(b, a) is None, (name, exact, fo.differing(b, a))
            assert a["h"] == b["h"], name
        seen += 1
    assert seen >= 18


def test_wrapped_tables_agree_with_python_integers():
    """S2 of a +-32768 m checkerboard wraps past 2^64 within 600 x 600 cells; object cumsum reduced modulo 2^64 gives the same words."""
    z = fo.checkerboard(600, 600)
    h, N, S1, S2 = fo.tables(z)
    assert h == {"qmin": -(1 << 23), "qmax": 1 << 23, "n_valid": 360000, "c": 0, "D": 1 << 23}
    assert 360000 * (1 << 46) > fo.MOD and int(S2[600, 600]) == (360000 << 46) % fo.MOD
    small = fo.tables(z[:40, :40], exact=True)
    assert all(np.array_equal(a, b) for a, b in zip(small[1:], fo.tables(z[:40, :40])[1:]))
    got = fo.query_tables(z, fo.box(180), c0=300, r0=300, ow=1, oh=1)        # 361 x 361 = 130 321 cells, below 2^17
    assert int(got["n"][0, 0]) == 130321 and int(got["s2"][0, 0]) == 130321 << 46 and int(got["s1"][0, 0]) == 1 << 23
    assert got["mean"][0, 0] == 32768.0 / 130321 and abs(got["var"][0, 0] - 32768.0 ** 2) < 1e-4 * 32768.0 ** 2


# ---- closed forms ----------------------------------------------------------------------------------------------------------------
def test_plane_under_a_symmetric_window():
    r, c = np.indices((40, 50))
    z = (0.5 * c - 0.25 * r + 100.0).astype(np.float32)
    for rects in (fo.box(3), fo.disc(4.5), fo.annulus(6, 2)):
        got = fo.query_tables(z, rects)
        inner = (slice(7, -7), slice(7, -7))
        assert np.array_equal(got["mean"][inner], z.astype(np.float64)[inner])
        t, _, keep = fo.tpi_terms(z, got["n"], got["mean"], got["var"])
        assert keep.all() and not t[inner].any()


@pytest.mark.parametrize("w", (5, 7))
def test_variance_of_a_ramp_under_a_box(w):
    step = 0.75
    z = (step * np.indices((30, 41))[1]).astype(np.float32)
    got = fo.query_tables(z, fo.box(w // 2))
    inner = got["var"][w:-w, w:-w]
    assert np.all(inner == (w * w - 1) / 12 * step * step)


def test_a_single_valid_cell_and_a_single_row():
    one = np.full((9, 11), np.nan, np.float32)
    one[4, 6] = -17.25
    got = fo.query_tables(one, fo.box(2))
    near = np.zeros(one.shape, bool)
    near[2:7, 4:9] = True
    assert np.array_equal(got["n"], near.astype(np.int32)) and np.all(got["mean"][near] == -17.25) and np.all(got["var"][near] == 0.0)
    assert np.isnan(got["mean"][~near]).all() and np.isnan(got["var"][~near]).all()
    row = (np.arange(70) % 7 * 0.5).astype(np.float32)[None, :]
    got = fo.query_tables(row, fo.box(3))
    q = np.rint(row[0].astype(np.float64) * 256).astype(np.int64)
    h = fo.header(row)
    assert np.array_equal(got["s1"][0], np.convolve(q - h["c"], np.ones(7, np.int64), "same"))
    assert np.array_equal(got["n"][0], np.convolve(np.ones(70, np.int64), np.ones(7, np.int64), "same"))


# ---- windows ---------------------------------------------------------------------------------------------------------------------
def _sound(window, shape, radius, inner=None, xres=1.0, yres=1.0):
    assert isinstance(window, FocalWindow) and window.rects.dtype == np.int32 and window.rects.flags.c_contiguous
    k = int(np.abs(window.rects[:, :4]).max()) + 2
    member, _ = fo.window_mask(shape, radius, inner, xres, yres, reach=k)
    edge = np.ones_like(member)
    edge[1:-1, 1:-1] = False
    assert not member[edge].any()                            # the brute-force square is wide enough
    assert np.array_equal(fo.rasterise(window.rects, k), member.astype(np.int64))
    assert window.cells == int(member.sum())
    assert window.positive == int(sum((r[1] - r[0] + 1) * (r[3] - r[2] + 1) for r in window.rects.tolist() if r[4] > 0))


def test_disc_cell_counts_against_brute_force():
    for radius in list(range(65)) + [0.5, 1.5, 2.5, 7.07, 63.999]:
        w = focal_window("disc", radius)
        _sound(w, "disc", radius)
        rows = w.rects[:, 3] - w.rects[:, 2] + 1
        assert int(rows.sum()) == 2 * int(radius) + 1         # every row once
        assert len(w.rects) == 1 or (np.diff(w.rects[:, 1]) != 0).all()           # rows of equal extent are merged
    assert focal_window("disc", 0).rects.tolist() == [[0, 0, 0, 0, 1]]
    assert focal_window("disc", 1).cells == 5 and focal_window("disc", 2.5).cells == 21 and focal_window("disc", 100).cells == 31417


def test_ellipses_boxes_and_annuli():
    grid = DSMGrid(0.0, 0.0, 5.0, 2.5, 10, 10)
    for radius in (0.0, 2.5, 5.0, 12.5, 33.0, 250.0):
        _sound(focal_window("disc", radius, grid=grid), "disc", radius, None, 5.0, 2.5)
        _sound(focal_window("box", radius, grid=grid), "box", radius, None, 5.0, 2.5)
    w = focal_window("box", 12.5, grid=grid)
    assert w.rects.tolist() == [[-2, 2, -5, 5, 1]] and w.cells == 55
    for radius, inner in ((4, 2), (10, 0), (30.5, 30.0), (3, 2.9)):
        a = focal_window("annulus", radius, inner)
        _sound(a, "annulus", radius, inner)
        outer, hole = focal_window("disc", radius), focal_window("disc", inner)
        assert a.cells == outer.cells - hole.cells and a.positive == outer.cells
        assert np.array_equal(a.rects, np.concatenate([outer.rects, hole.rects * np.array([1, 1, 1, 1, -1], np.int32)]))
    _sound(focal_window("annulus", 50.0, 20.0, grid=grid), "annulus", 50.0, 20.0, 5.0, 2.5)


def test_the_record_limit():
    assert dsm._window_checked(fo.many_records(1024)).cells == 1024
    with pytest.raises(ValueError, match="1 .. 1024 records"):
        dsm._window_checked(fo.many_records(1025))
    assert len(focal_window("disc", 870).rects) == 1021                            # the widest discs one call serves
    for args in (("disc", 880), ("disc", 1024), ("annulus", 800, 100)):
        with pytest.raises(ValueError, match="1 .. 1024 records"):
            focal_window(*args)


# ---- against other libraries' means ----------------------------------------------------------------------------------------------
def test_uniform_filter_of_a_void_free_copy():
    ndimage = pytest.importorskip("scipy.ndimage")
    z = np.round(fo.kit_scene(60, 75, seed=11, salt=0.02) * 256) / 256           # void-free where voids = 0 ... but for the two holes
    z = np.where(np.isfinite(z) & (z != -999.0), z, 130.0).astype(np.float32)
    for r in (1, 4, 9):
        got = fo.query_tables(z, fo.box(r))
        k = 2 * r + 1
        want = ndimage.uniform_filter(z.astype(np.float64), k, mode="constant") / ndimage.uniform_filter(np.ones(z.shape), k, mode="constant")
        assert np.abs(got["mean"] - want).max() < 1e-9


def test_aggregate_against_reshape_and_mean():
    z = (np.round(fo.kit_scene(24, 36, seed=2) * 256) / 256).astype(np.float32)
    ok, _ = fo.quantise(z)
    for f in (2, 3, 4, 12):
        mean, count = fo.block_mean(z, f)
        v = np.where(ok, z.astype(np.float64), 0.0).reshape(24 // f, f, 36 // f, f)
        cnt = ok.reshape(24 // f, f, 36 // f, f).sum(axis=(1, 3))
        assert np.array_equal(count, cnt)
        with np.errstate(invalid="ignore"):
            want = v.sum(axis=(1, 3)) / cnt
        assert np.allclose(mean[cnt > 0], want[cnt > 0], rtol=2.0 ** -22, atol=0) and np.all(mean[cnt == 0] == -999.0)
    mean, count = fo.block_mean(z[:23, :35], 4)               # a last partial block is kept and clipped
    assert mean.shape == (6, 9) and count[5, 8] == int(ok[20:23, 32:35].sum()) and count[0, 8] == int(ok[0:4, 32:35].sum())


# ---- the host-side overflow check ------------------------------------------------------------------------------------------------
def _fake_tables(gw=50, gh=40, max_abs=1 << 23):
    return FocalTables(torch.zeros(1, dtype=torch.uint8), gw, gh, [-max_abs, max_abs, gw * gh, 0, max_abs, 0, 0, 0], True)


def test_overflow_check_on_both_sides_of_the_bound():
    t = _fake_tables()
    t.check(FocalWindow(fo.box(180), 130321, 130321))                              # 130 321 2^46 < 2^63
    t.check(FocalWindow(fo.box(1), (1 << 17) - 1, (1 << 17) - 1))
    for positive in (1 << 17, 131769):
        with pytest.raises(ValueError, match="may wrap"):
            t.check(FocalWindow(fo.box(1), positive, positive))
    with pytest.raises(ValueError, match="may wrap"):
        dsm.focal_sums(t, fo.box(181))                                             # 363 x 363 = 131 769 cells: before any device work
    _fake_tables(max_abs=1 << 19).check(FocalWindow(fo.box(1), 1 << 24, 1 << 24))           # the largest window: 2^62
    _fake_tables(max_abs=1 << 20).check(FocalWindow(fo.box(1), (1 << 23) - 1, (1 << 23) - 1))
    with pytest.raises(ValueError, match="may wrap"):
        _fake_tables(max_abs=1 << 20).check(FocalWindow(fo.box(1), 1 << 23, 1 << 23))     # 2^63 itself


# ---- argument rejections ---------------------------------------------------------------------------------------------------------
def test_python_argument_rejections():
    grid = DSMGrid(0.0, 0.0, 5.0, 5.0, 50, 40)
    for args, match in ((("ring", 3), "shape must be"), (("disc", -1), "radius must be >= 0"), (("disc", float("nan")), "finite"),
                        (("disc", 3, 1), "inner goes with"), (("annulus", 3), "inner goes with"), (("annulus", 3, 3), "inner must be"),
                        (("annulus", 3, -1), "inner must be"), (("box", 5000), "at most 4096 cells"), (("box", 2100), "2\\^24 cells"),
                        (("disc", 1e9), "at most 4096 cells")):
        with pytest.raises(ValueError, match=match):
            focal_window(*args)
    with pytest.raises(ValueError, match="positive finite resolutions"):
        focal_window("disc", 10.0, grid=DSMGrid(0.0, 0.0, 0.0, 5.0, 5, 5))
    for bad, match in ((np.zeros((3, 4), np.int32), "\\(k, 5\\) integers"), (np.array([[0, 1, 0, 1, 2]]), "sign"), (np.array([[1, 0, 0, 0, 1]]), "dx0 <= dx1"),
                       (np.array([[0, 0, 0, 5000, 1]]), "at most 4096"), (np.zeros((0, 5), np.int32), "records"),
                       (np.zeros((1, 5), np.float32), "integers")):
        with pytest.raises(ValueError, match=match):
            dsm._window_checked(bad)
    for bad, match in ((np.zeros((4, 5), np.float64), "float32"), (np.zeros((2, 3, 4), np.float32), "gh, gw"), (torch.zeros(4, 5, dtype=torch.float64), "float32")):
        with pytest.raises(ValueError, match=match):
            dsm.focal_tables(bad)
        with pytest.raises(ValueError, match=match):
            dsm.focal_stats(bad, fo.box(1))
        with pytest.raises(ValueError, match=match):
            dsm.tpi(bad, grid, 10.0)
    t = _fake_tables(max_abs=100)
    for kw, match in (({"stride": (0, 1)}, "stride must be"), ({"stride": (1, 2, 3)}, "pair"), ({"origin": (40, 0)}, "origin"), ({"origin": (0, -1)}, "origin"),
                      ({"shape": (41, 50)}, "inside the grid"), ({"shape": (0, 5)}, "inside the grid"), ({"stride": (2, 2), "shape": (21, 25)}, "inside the grid")):
        with pytest.raises(ValueError, match=match):
            dsm.focal_sums(t, fo.box(1), **kw)
    with pytest.raises(ValueError, match="min_valid"):
        dsm.focal_stats(t, fo.box(1), min_valid=-1)
    with pytest.raises(ValueError, match="focal_tables"):
        dsm.focal_sums(np.zeros((4, 5), np.float32), fo.box(1))
    z = np.zeros((40, 50), np.float32)
    with pytest.raises(ValueError, match="differs from the grid"):
        dsm.tpi(z, DSMGrid(0.0, 0.0, 5.0, 5.0, 51, 40), 10.0)
    with pytest.raises(ValueError, match="factor"):
        dsm.aggregate(z, grid, 0)
    with pytest.raises(ValueError, match="mask"):
        dsm.focal_fraction(np.zeros((4, 5), np.float32), fo.box(1))


def test_c_argument_rejections(lib):
    """Host checks of both entries: a message and SMVS_ERR_ARG before any HIP call, on made-up pointers."""
    from satmvs_amd import _lib
    assert lib.smvs_dsm_focal_table_bytes(0, 5) == 0 and lib.smvs_dsm_focal_table_bytes(5, -1) == 0
    assert lib.smvs_dsm_focal_table_bytes(46340, 46340) == 0 and lib.smvs_dsm_focal_table_bytes(46339, 46340) > 0
    assert lib.smvs_dsm_focal_table_bytes(2 ** 31 - 1, 1) == 0
    for gw, gh in ((1, 1), (70, 1), (3, 67), (301, 257), (2158, 2199)):
        assert lib.smvs_dsm_focal_table_bytes(gw, gh) == fo.layout(gw, gh)["bytes"]
    nbytes = lib.smvs_dsm_focal_table_bytes(50, 40)
    p = lambda v: C.c_void_p(v)
    build = lambda *a: _lib.call("smvs_dsm_focal_build", *a, None)
    for args, match in (((None, 50, 40, -999.0, p(1 << 30), nbytes), "null pointer"), ((p(1 << 20), 50, 40, -999.0, None, nbytes), "null pointer"),
                        ((p(1 << 20), 0, 40, -999.0, p(1 << 30), nbytes), "non-positive"), ((p(1 << 20), 50, -3, -999.0, p(1 << 30), nbytes), "non-positive"),
                        ((p(1 << 20), 46340, 46340, -999.0, p(1 << 40), 1 << 40), "grid too large"),
                        ((p(1 << 20), 50, 40, -999.0, p(1 << 30), nbytes - 1), "table buffer too small"),
                        ((p(1 << 20), 50, 40, -999.0, p((1 << 20) + 7996), nbytes), "aliases dsm"),
                        ((p((1 << 20) + nbytes - 4), 50, 40, -999.0, p(1 << 20), nbytes), "aliases dsm")):
        with pytest.raises(_lib.SatMVSNativeError, match=match):
            build(*args)
    one = fo.box(1)
    T, OUT = 1 << 30, 1 << 40                                # the tables and outputs far apart, 1 MiB between the outputs

    def query(rects=one, n_rects=None, tables=p(T), gw=50, gh=40, ow=50, oh=40, c0=0, r0=0, sx=1, sy=1, min_valid=1, outs=None, status=p(OUT + (6 << 20))):
        rects = None if rects is None else np.ascontiguousarray(rects, np.int32)
        outs = [p(OUT + (k << 20)) for k in range(5)] if outs is None else outs
        k = (0 if rects is None else len(rects)) if n_rects is None else n_rects
        _lib.call("smvs_dsm_focal_query", tables, gw, gh, None if rects is None else rects.ctypes.data_as(C.c_void_p), k, ow, oh, c0, r0, sx, sy,
                  min_valid, *outs, status, None)

    for kw, match in (({"tables": None}, "null pointer"), ({"rects": None, "n_rects": 1}, "null pointer"), ({"status": None}, "null pointer"),
                      ({"gw": 0}, "non-positive"), ({"n_rects": 0}, "n_rects must be"), ({"rects": fo.many_records(1025)}, "n_rects must be"),
                      ({"rects": [[-4097, 0, 0, 0, 1]]}, "offset"), ({"rects": [[0, 0, 0, 4097, 1]]}, "offset"), ({"rects": [[1, 0, 0, 0, 1]]}, "empty bounds"),
                      ({"rects": [[0, 0, 2, 1, 1]]}, "empty bounds"), ({"rects": [[0, 0, 0, 0, 0]]}, "sign"), ({"rects": [[0, 0, 0, 0, 2]]}, "sign"),
                      ({"rects": [[-2048, 2047, -2048, 2047, 1], [0, 0, 0, 0, 1]]}, "window too large"), ({"sx": 0}, "must be >= 1"), ({"sy": -1}, "must be >= 1"),
                      ({"ow": 0}, "must be >= 1"), ({"oh": 0}, "must be >= 1"), ({"c0": -1}, "outside the grid"), ({"r0": 1}, "outside the grid"),
                      ({"ow": 51}, "outside the grid"), ({"sx": 2}, "outside the grid"), ({"sy": 2, "oh": 21}, "outside the grid"),
                      ({"min_valid": -1}, "min_valid"), ({"outs": [p(T + 64)] + [None] * 4}, "n aliases tables"),
                      ({"outs": [p(OUT), p(OUT + 7999), None, None, None]}, "s1 aliases n"), ({"outs": [None, None, None, p(OUT), p(OUT + 8)]}, "var aliases mean"),
                      ({"outs": [None] * 5, "status": p(T + nbytes - 1)}, "status aliases tables"), ({"outs": [None, None, p(OUT), None, None], "status": p(OUT + 15999)}, "status aliases s2")):
        with pytest.raises(_lib.SatMVSNativeError, match=match):
            query(**kw)
    with pytest.raises(_lib.SatMVSNativeError, match="window too large"):
        query(rects=[[-2048, 2047, -2048, 2047, 1], [0, 0, 0, 0, -1], [5, 5, 5, 5, 1]])      # W+ = 2^24 + 1; the negative record does not count


# ---- planted mistakes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plant", fo.PLANTS)
def test_planted_mistakes_are_reported(plant):
    z = (np.random.default_rng(4).integers(-2000, 2000, (9, 11)) / 512.0).astype(np.float32)   # every other one on a half
    z[0, 0], z[0, 1], z[4, 4] = -5.0, 5.00390625, np.nan
    want = fo.query_tables(z, fo.box(2))
    assert (want["h"]["qmin"], want["h"]["qmax"]) == (-1280, 1281)                 # an odd sum: rounding the centre up moves it
    state = fo.query_direct if plant == "unclipped" else fo.query_tables
    got = state(z, fo.box(2), plant=plant)
    d = fo.differing(got, want)
    assert d is not None, plant
    expect = {"c_up": "s1", "unclipped": "n", "sample_var": "var", "half_away": "s1", "high_word": "var"}[plant]
    assert d.startswith(expect + " differs"), (plant, d)
    assert fo.differing(state(z, fo.box(2)), want) is None
