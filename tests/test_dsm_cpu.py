"""DSM production, the parts that run without a GPU: the numpy Transverse Mercator mirror against the reference's outputs
(tests/golden/tm.npz), the world file and float32 TIFF round trips, grid snapping, and argument checks of the C entries; and
what tests/test_dsm_gpu.py assumes of its case matrix (tests/dsm_scene.py), of its oracle and of its comparisons: the oracle's
statements against each other, the matrix against the kernel's tiles and thresholds, nine planted errors that the comparisons
must report, and the mean's interval against three ways of summing."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import dsm_oracle as orc
import dsm_scene as sc
import dsm_testkit as tk
from dsm_testkit import lib  # noqa: F401  (fixtures)


@pytest.mark.parametrize("name", ["whu", "example"])
def test_tm_mirror_matches_reference(golden, name):
    g = golden("tm")
    tm7, ll, en, back = g[name + ".tm7"], g[name + ".latlon"], g[name + ".en"], g[name + ".latlon_back"]
    E, N = orc.tm_forward(tm7, ll[:, 0], ll[:, 1])
    assert np.abs(E - en[:, 0]).max() <= 1e-9 and np.abs(N - en[:, 1]).max() <= 1e-9
    lat, lon = orc.tm_inverse(tm7, en[:, 0], en[:, 1])
    assert np.abs(lat - back[:, 0]).max() <= 1e-12 and np.abs(lon - back[:, 1]).max() <= 1e-12
    # the truncated series round trip: within 1e-6 deg (a few cm) out to 6 deg from the central meridian
    assert np.abs(back - ll).max() < 1e-6


def test_whu_tlc_projection_parameters():
    from satmvs_amd.transverse_mercator import whu_tlc_projection
    assert whu_tlc_projection().tm7().tolist() == [6378137.0, 298.257223563, 0.0, -135.0, 0.9996, 500000.0, 0.0]


def test_tfw_round_trip_and_format(tmp_path):
    from satmvs_amd.data_io import read_tfw
    from satmvs_amd.dsm import DSMGrid, write_dsm
    grid = DSMGrid(e0=512345.0, n0=3312345.0, xres=5.0, yres=5.0, width=3, height=2)
    path = str(tmp_path / "dsm.tif")
    write_dsm(path, np.zeros((2, 3), np.float32), grid)
    text = open(str(tmp_path / "dsm.tfw")).read()
    assert text == "5.0\n0\n0\n-5.0\n512345.0\n3312345.0"          # the reference's gdal_create_dsm_file layout
    assert read_tfw(str(tmp_path / "dsm.tfw")).tolist() == [5.0, 0.0, 0.0, -5.0, 512345.0, 3312345.0]
    (tmp_path / "bad.tfw").write_text("1\n2\n3\n")
    with pytest.raises(ValueError, match="6 parameters"):
        read_tfw(str(tmp_path / "bad.tfw"))


def test_float32_tiff_round_trip(tmp_path):
    from satmvs_amd.dsm import DSMGrid, read_dsm, write_dsm
    rng = np.random.default_rng(3)
    a = rng.normal(100.0, 50.0, (37, 53)).astype(np.float32)
    a[3, 4], a[5, 6] = -999.0, np.float32(1e-30)
    grid = DSMGrid(1000.0, 2000.0, 2.5, 2.5, 53, 37)
    path = str(tmp_path / "x.tif")
    write_dsm(path, a, grid)
    b, g2 = read_dsm(path)
    assert b.dtype == np.float32 and b.shape == a.shape
    assert np.array_equal(b.view(np.uint32), a.view(np.uint32))
    assert g2 == grid
    with pytest.raises(ValueError, match="differs"):
        write_dsm(path, a[:, :5], grid)


def test_grid_snapping():
    from satmvs_amd.dsm import grid_from_extent
    g = grid_from_extent(501233.7, 503011.2, 3300402.1, 3302999.9, 5.0)
    assert g.e0 % 5.0 == 0.0 and g.n0 % 5.0 == 0.0 and g.xres == g.yres == 5.0
    assert (g.e0, g.n0) == (501235.0, 3303000.0)
    for e, n in [(501233.7, 3302999.9), (503011.2, 3300402.1)]:
        col, row = g.cell_of(e, n)
        assert 0 <= col < g.width and 0 <= row < g.height
    assert g.cell_of(501233.7, 3302999.9) == (0.0, 0.0)
    assert g.cell_of(503011.2, 3300402.1) == (g.width - 1, g.height - 1)
    # extremes exactly on a half cell: still inside by the kernel's rule
    g = grid_from_extent(12.5, 22.5, -7.5, 2.5, 5.0)
    assert g.cell_of(12.5, 2.5) == (0.0, 0.0) and g.cell_of(22.5, -7.5) == (g.width - 1, g.height - 1)
    # a single point
    g = grid_from_extent(7.0, 7.0, 9.0, 9.0, 2.0)
    assert (g.width, g.height, g.e0, g.n0) == (1, 1, 8.0, 8.0)
    with pytest.raises(ValueError):
        grid_from_extent(0.0, 1.0, 0.0, 1.0, 0.0)


def test_metrics_known_answers():
    from satmvs_amd.dsm import dsm_metrics
    gt = np.array([[10.0, 20.0, -999.0], [30.0, 40.0, 50.0]], np.float32)
    est = np.array([[11.0, 20.0, 5.0], [-999.0, 48.0, np.nan]], np.float32)
    m = dsm_metrics(est, gt, -999.0)
    assert m["n"] == 3
    assert m["completeness"] == pytest.approx(3 / 5)
    assert m["mae"] == pytest.approx(3.0) and m["rmse"] == pytest.approx(np.sqrt(65 / 3))
    assert m["<2.5"] == pytest.approx(2 / 3) and m["<7.5"] == pytest.approx(2 / 3)


def test_dsm_entries_reject_bad_arguments_without_a_gpu(lib):
    from satmvs_amd import _lib
    d = C.c_void_p(16)
    tm7 = np.array([6378137.0, 298.257223563, 0.0, -135.0, 0.9996, 500000.0, 0.0])
    grid4 = np.array([0.0, 0.0, 5.0, 5.0])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731
    with pytest.raises(_lib.SatMVSNativeError, match="null pointer"):
        _lib.call("smvs_tm_project", None, d, d, d, d, 4, 0, None)
    with pytest.raises(_lib.SatMVSNativeError, match="dir must be"):
        _lib.call("smvs_tm_project", vp(tm7), d, d, d, d, 4, 2, None)
    bad = tm7.copy()
    bad[4] = 0.0
    with pytest.raises(_lib.SatMVSNativeError, match="projection parameters"):
        _lib.call("smvs_tm_project", vp(bad), d, d, d, d, 4, 0, None)
    with pytest.raises(_lib.SatMVSNativeError, match="null pointer"):
        _lib.call("smvs_rpc_dsm_bin", d, None, None, 4, 4, vp(tm7), vp(grid4), 8, 8, d, d, None, None, None)
    with pytest.raises(_lib.SatMVSNativeError, match="go together"):
        _lib.call("smvs_rpc_dsm_bin", d, None, d, 4, 4, vp(tm7), vp(grid4), 8, 8, d, d, d, None, None)
    with pytest.raises(_lib.SatMVSNativeError, match="non-positive dimension"):
        _lib.call("smvs_rpc_dsm_bin", d, None, d, 0, 4, vp(tm7), vp(grid4), 8, 8, d, d, None, None, None)
    with pytest.raises(_lib.SatMVSNativeError, match="non-positive grid"):
        _lib.call("smvs_rpc_dsm_bin", d, None, d, 4, 4, vp(tm7), vp(grid4), 0, 8, d, d, None, None, None)
    with pytest.raises(_lib.SatMVSNativeError, match="grid too large"):
        _lib.call("smvs_rpc_dsm_bin", d, None, d, 4, 4, vp(tm7), vp(grid4), 65536, 32768, d, d, None, None, None)
    for g in ([0.0, 0.0, 0.0, 5.0], [0.0, 0.0, 5.0, -1.0], [np.nan, 0.0, 5.0, 5.0], [0.0, 0.0, np.inf, 5.0]):
        with pytest.raises(_lib.SatMVSNativeError, match="bad grid"):
            _lib.call("smvs_rpc_dsm_bin", d, None, d, 4, 4, vp(tm7), vp(np.array(g)), 8, 8, d, d, None, None, None)
    with pytest.raises(_lib.SatMVSNativeError, match="projection parameters"):
        _lib.call("smvs_rpc_dsm_bin", d, None, d, 4, 4, vp(bad), vp(grid4), 8, 8, d, d, None, None, None)
    ws = lib.smvs_dsm_workspace_bytes(100, 8, 8)
    assert ws > 0
    assert lib.smvs_dsm_workspace_bytes(1 << 31, 8, 8) == 0
    assert lib.smvs_dsm_workspace_bytes(100, 0, 8) == 0
    assert lib.smvs_dsm_workspace_bytes(100, 65536, 32768) == 0
    with pytest.raises(_lib.SatMVSNativeError, match="null pointer"):
        _lib.call("smvs_dsm_reduce", None, d, 100, d, 8, 8, 0, -999.0, d, d, ws, None)
    with pytest.raises(_lib.SatMVSNativeError, match="mode must be"):
        _lib.call("smvs_dsm_reduce", d, d, 100, d, 8, 8, 4, -999.0, d, d, ws, None)
    with pytest.raises(_lib.SatMVSNativeError, match="mode must be"):
        _lib.call("smvs_dsm_reduce", d, d, 100, d, 8, 8, -1, -999.0, d, d, ws, None)
    with pytest.raises(_lib.SatMVSNativeError, match="too many points"):
        _lib.call("smvs_dsm_reduce", d, d, 1 << 31, d, 8, 8, 0, -999.0, d, d, ws, None)
    with pytest.raises(_lib.SatMVSNativeError, match="non-positive grid"):
        _lib.call("smvs_dsm_reduce", d, d, 100, d, 8, -2, 0, -999.0, d, d, ws, None)
    with pytest.raises(_lib.SatMVSNativeError, match="workspace too small"):
        _lib.call("smvs_dsm_reduce", d, d, 100, d, 8, 8, 0, -999.0, d, d, ws - 1, None)


def test_python_surface_validates_before_the_gpu():
    from satmvs_amd import dsm
    from satmvs_amd.transverse_mercator import whu_tlc_projection
    grid = dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, 4, 4)
    with pytest.raises(ValueError, match="mode must be"):
        dsm.heights_to_dsm([np.zeros((4, 4), np.float32)], [np.zeros(170)], whu_tlc_projection(), grid, mode="mode")


# ---- what tests/test_dsm_gpu.py assumes ------------------------------------------------------------------------------------------
MODES = ("median", "mean", "min", "max")
SMALL_CASES = [n for n in sc.CASES if n not in ("size 2^20", "tier 2 twice")]


@functools.lru_cache(maxsize=None)
def _ref(name):
    c = sc.case(name)
    return orc.reference(c.cell, c.height, c.gh * c.gw)


def _buckets(c):
    """{cell: its values sorted on their keys} of a case, the ignored entries left out."""
    ok = (c.cell >= 0) & (c.cell < c.gh * c.gw)
    cell, h = c.cell[ok], c.height[ok]
    order = np.lexsort((tk.f2key(h), cell))
    cell, h = cell[order], h[order]
    cut = np.nonzero(np.diff(cell))[0] + 1
    return {int(v[0]): w for v, w in zip(np.split(cell, cut), np.split(h, cut)) if v.size}


def _naive(c, mode, nodata):
    """The third statement: Python's sorted on the keys, a textbook median, math.fsum for the mean."""
    out = np.full(c.gh * c.gw, np.float32(nodata), np.float32)
    pts = {}
    for cc, k, h in zip(c.cell.tolist(), tk.f2key(c.height).tolist(), c.height):
        if 0 <= cc < c.gh * c.gw:
            pts.setdefault(cc, []).append((k, h))
    for cc, kv in pts.items():
        v = [h for _, h in sorted(kv, key=lambda t: t[0])]
        m = len(v)
        if mode == "min":
            out[cc] = v[0]
        elif mode == "max":
            out[cc] = v[-1]
        elif mode == "mean":
            with np.errstate(invalid="ignore"):
                out[cc] = np.float32(math.fsum(float(x) for x in v) / m) if all(math.isfinite(x) for x in v) else np.float32(np.sum(np.float64(v)) / m)
        elif m % 2:
            out[cc] = v[m // 2]
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                out[cc] = np.float32(0.5 * (np.float64(v[m // 2 - 1]) + np.float64(v[m // 2])))
    return out


@pytest.mark.parametrize("name", ["scan 257", "scan 4097", "sizes 0 to 70", "both zeros", "nan at both ends", "mostly one nan", "both infinities",
                                  "denormals", "byte 3 only", "cancel 1e6", "ignored entries"])
def test_the_three_statements_of_the_reduce_agree(name):
    c = sc.case(name)
    ncells = c.gh * c.gw
    ref = _ref(name)
    for mode in MODES:
        loop, count = orc.reduce(c.cell, c.height, ncells, mode, -999.0)
        naive = _naive(c, mode, -999.0)
        assert np.array_equal(count, ref.count)
        orc.check(loop, ref, mode, -999.0)
        orc.check(naive, ref, mode, -999.0)
        orc.check(orc.model_reduce(c.cell, c.height, ncells, mode, -999.0), ref, mode, -999.0)
        if mode != "mean":
            assert tk.same_bits(loop, naive), mode


def test_matrix_bucket_sizes():
    sizes = {name: _ref(name).count for name in sc.SIZE_CASES + sc.LIST_CASES}
    assert sizes["sizes 0 to 70"].tolist() == list(range(71))
    assert sorted(sizes["sizes 2^k"].tolist()) == sorted(p + d for p in (64, 128, 256, 512, 1024, 2048, 4096) for d in (-1, 0, 1))
    assert {sc.TIER1_MAX - 1, sc.TIER1_MAX, sc.TIER1_MAX + 1} <= set(sizes["sizes 2^k"].tolist())
    assert sizes["sizes radix"].tolist() == [5119, 5120, 5121, 65535, 65536, 65537]
    radix = np.concatenate([sizes["sizes radix"], sizes["size 2^20"], sizes["tier 2 twice"]])
    assert {0, 1023} <= set((radix % 1024).tolist()) and {0, 63} <= set((radix % 64).tolist())
    assert sizes["size 2^20"].max() >= 1 << 20
    t1, t2 = sizes["tier 1 twice"], sizes["tier 2 twice"]
    assert ((t1 > sc.TIER0_MAX) & (t1 <= sc.TIER1_MAX)).sum() > 2 * sc.TIER1_BLOCKS and set(t1.tolist()) == set(range(33, 65))
    assert (t2 > sc.TIER1_MAX).sum() > sc.TIER2_BLOCKS and t2.min() >= 4097 and t2.max() <= 4200
    mixed = sizes["tiers mixed"]
    assert (mixed == 0).sum() > 100 and ((mixed > 0) & (mixed <= 32)).sum() > 100 and ((mixed > 32) & (mixed <= 4096)).sum() > 100 and (mixed > 4096).sum() > 10
    tier = np.where(mixed == 0, 0, np.where(mixed <= 32, 1, np.where(mixed <= 4096, 2, 3)))
    assert (np.diff(tier) != 0).mean() > 0.9                                       # interleaved
    for name in sc.VALUE_CASES + sc.CANCEL_CASES:
        assert _ref(name).count.tolist() == list(sc.VALUE_SIZES) + [0, 0], name
    assert [m <= 32 for m in sc.VALUE_SIZES] == [True, True, False, False, False, False]
    assert [m > 4096 for m in sc.VALUE_SIZES] == [False, False, False, False, True, True]


def test_matrix_scan_cases():
    wanted = [1, 2, 255, 256, 257, 4095, 4096, 4097, 8191, 8193, 256 * 4096 - 1, 256 * 4096, 256 * 4096 + 1, 257 * 4096 + 1, 513 * 4096 + 5]
    assert list(sc.SCAN_SHAPES) == wanted and sc.SCAN_CASES == ["scan %d" % n for n in wanted]
    shapes = [sc.SCAN_SHAPES[n] for n in wanted]
    assert all(gh * gw == n for (gh, gw), n in zip(shapes, wanted))
    assert any(gw == 1 and gh > 1 for gh, gw in shapes) and any(gh == 1 and gw > 1 for gh, gw in shapes)
    assert any(gh > 1 and gw > 1 and gh != gw for gh, gw in shapes)
    tiles = lambda n: -(-n // sc.SCAN_TILE)                 # noqa: E731
    assert any(tiles(n) > sc.SCAN_CHUNK and n % sc.SCAN_TILE for n in wanted) and sc.CHUNK_CELLS in wanted
    assert max(tiles(n) for n in wanted) > 2 * sc.SCAN_CHUNK                       # a third chunk: the carry is carried on
    for n in wanted:
        c = sc.case("scan %d" % n)
        count = _ref(c.name).count
        assert (c.gh, c.gw) == sc.SCAN_SHAPES[n] and c.cell.size <= 2.5e5 and count.max() <= 40
        if n > sc.SCAN_FILLED:
            assert set(np.unique(count).tolist()) >= set(range(0, 41, 5))
        buckets = _buckets(c)
        sent = sc.sentinel_cells(n)
        assert 0 in sent and n - 1 in sent and all(s in sent for s in sc.SENTINELS if s < n)
        others = np.concatenate([v for cc, v in buckets.items() if cc not in sent] + [np.zeros(0, np.float32)])
        for k, s in enumerate(sent):                         # values that occur in no other cell
            v = buckets[s]
            assert v.size == 3 + k and np.unique(v).size == v.size and not np.isin(v, others).any()
            assert all(not np.isin(v, buckets[t]).any() for t in sent if t != s)
        if n > sc.CHUNK_CELLS:                               # the carry is not zero where it first acts
            assert count[:sc.CHUNK_CELLS].sum() > 1000 and count[sc.CHUNK_CELLS:].sum() > 0


def test_matrix_key_values():
    key = lambda name: tk.f2key(sc.case(name).height)        # noqa: E731
    for byte in range(4):
        k = key("byte %d only" % byte)
        varying = np.bitwise_or.reduce(k ^ k[0])
        assert varying & ~np.uint32(0xff << (8 * byte)) == 0 and bin(int(varying)).count("1") == 8, byte
        for v in _buckets(sc.case("byte %d only" % byte)).values():
            assert np.unique(v).size > min(v.size, 200) // 2 and np.isfinite(v).all()
    bits = lambda name: sc.case(name).height.view(np.uint32)  # noqa: E731
    assert set(bits("both zeros").tolist()) == {0, 0x80000000}
    d = sc.case("denormals").height
    assert ((d != 0) & (np.abs(d) < np.finfo(np.float32).tiny)).all() and (d < 0).any() and (d > 0).any()
    for name in ("nan at both ends", "mostly one nan"):
        for v in _buckets(sc.case(name)).values():
            nan = np.isnan(v)
            assert np.signbit(v[nan]).any() and np.unique(v[nan].view(np.uint32)).size > 1, name
    both = sc.case("nan at both ends").height
    nb = both.view(np.uint32)[np.isnan(both)]
    assert ((nb >> 31) == 0).any() and ((nb >> 31) == 1).any() and ((nb & 0x400000) == 0).any() and ((nb & 0x400000) != 0).any()
    inf = sc.case("both infinities").height
    assert all((inf == v).any() for v in (np.inf, -np.inf, sc.FLT_MAX, -sc.FLT_MAX))
    assert np.isfinite(sc.case("flt_max").height).all() and (np.abs(sc.case("flt_max").height) == sc.FLT_MAX).any()
    for name, sign in (("mostly +inf", np.inf), ("mostly -inf", -np.inf)):
        r = _ref(name)
        assert (r.median[:6] == sign).all() and (r.kind[:6] == (orc.PLUS_INF if sign > 0 else orc.MINUS_INF)).all()
    assert np.isnan(_ref("mostly one nan").median[:6]).all() and np.isfinite(_ref("nan at both ends").median[:6]).all()
    for name in sc.ORDERED:
        c = sc.case(name)
        step = np.diff(c.height[c.cell == 4])
        assert (step > 0).all() if name == "ascending" else (step < 0).all()
    ig = sc.case("ignored entries")
    for v in (-1, -5, ig.gh * ig.gw, sc.INT32_MAX):
        assert (ig.cell == v).sum() == 200
    assert _ref("ignored entries").count.sum() == ig.cell.size - 800


def test_even_medians_leave_no_nan_to_the_hardware():
    """IEEE 754 leaves open which NaN a sum of two different NaNs, or of opposite infinities, gives: x86 and the GPU differ.  The
    comparisons demand equal bits of every median, so no even bucket of the matrix or of the random run may have such a middle
    pair, nor a signalling NaN in it (the conversion to float64 would quiet it)."""
    cases = [sc.case(n) for n in sc.CASES if not n.startswith("scan ")] + [c for s in sc.RANDOM_SEEDS for c in sc.random_cases(s)]
    for c in cases:
        for v in _buckets(c).values():
            if v.size % 2 == 0:
                a, b = v[v.size // 2 - 1], v[v.size // 2]
                ua, ub = (int(x.view(np.uint32)) for x in (a, b))
                assert not (np.isnan(a) and np.isnan(b) and ua != ub), c.name
                assert not (np.isinf(a) and np.isinf(b) and a != b), c.name
                assert not any(np.isnan(x) and not u & 0x400000 for x, u in ((a, ua), (b, ub))), c.name


def test_random_run_reaches_every_tier():
    n_cases, tiers, shapes = 0, np.zeros(4, np.int64), set()
    for seed in sc.RANDOM_SEEDS:
        for c in sc.random_cases(seed):
            n_cases += 1
            assert 1 <= c.gh <= 70 and 1 <= c.gw <= 70 and 1 <= c.cell.size <= 20000
            count = np.bincount(c.cell[(c.cell >= 0) & (c.cell < c.gh * c.gw)], minlength=c.gh * c.gw)
            tiers += [(count == 0).sum(), ((count > 0) & (count <= 32)).sum(), ((count > 32) & (count <= 4096)).sum(), (count > 4096).sum()]
            shapes.add((c.gh == 1, c.gw == 1))
    assert n_cases == 200 and (tiers > [1000, 1000, 1000, 20]).all(), tiers


# ---- planted errors ------------------------------------------------------------------------------------------------------------
# fault -> the cases that must report it (every one of them must; the same cases pass without the fault)
PLANTED = {
    "upper median": ["sizes 0 to 70", "tiers mixed"],
    "carry dropped": ["scan %d" % n for n in (256 * 4096 + 1, 257 * 4096 + 1, 513 * 4096 + 5)],
    "one tile off": ["scan 4097", "scan 8193", "scan %d" % (256 * 4096)],
    "nan lowest": ["nan at both ends", "mostly one nan"],
    "zeros merged": ["both zeros"],
    "pad key 0": ["sizes 0 to 70", "sizes 2^k", "ascending"],
    "radix skips byte 3": ["byte 3 only", "sizes radix", "tiers mixed"],
}


def _reported(c, ref, fault, modes=MODES):
    """The modes in which the comparison of the GPU tests rejects the model with `fault` planted."""
    out = []
    for mode in modes:
        got = orc.model_reduce(c.cell, c.height, c.gh * c.gw, mode, -999.0, fault)
        try:
            orc.check(got, ref, mode, -999.0)
        except AssertionError:
            out.append(mode)
    return out


def test_the_planted_errors_are_the_issue_s_nine():
    assert sorted(PLANTED) == sorted(orc.REDUCE_FAULTS) and len(orc.REDUCE_FAULTS) + len(orc.CELL_FAULTS) == 9


@pytest.mark.parametrize("fault", orc.REDUCE_FAULTS)
def test_planted_reduce_error_is_reported(fault):
    for name in PLANTED[fault]:
        c, ref = sc.case(name), _ref(name)
        assert _reported(c, ref, None, ("median", "min")) == [], name          # the model itself passes
        modes = _reported(c, ref, fault)
        assert modes, (fault, name)
        if fault == "upper median":
            assert modes == ["median"]
        if fault == "zeros merged":
            assert "min" in modes


EP, NP, EQ, NQ = 538123.4567891234, 3431987.6543219876, 538777.1234567891, 3431222.9876543211


def test_edge_grids_put_the_pixels_on_the_edges():
    grids = {g.name: g for g in sc.edge_grids(EP, NP, EQ, NQ)}
    assert len(grids) == 11 and sc.EDGE_GW % 2 == 1 and sc.EDGE_GH % 2 == 1
    assert sc.rule_arguments(EP, NP, grids["p on both lower edges"].grid4) == (0.0, 0.0)
    assert sc.rule_arguments(EQ, NQ, grids["q on the upper column edge"].grid4) == (float(sc.EDGE_GW), sc.EDGE_GH // 2 + 0.5)
    assert sc.rule_arguments(EQ, NQ, grids["q on the upper row edge"].grid4) == (sc.EDGE_GW // 2 + 0.5, float(sc.EDGE_GH))
    for g in grids.values():
        E, N = (EP, NP) if g.pixel == "p" else (EQ, NQ)
        ac, ar = sc.rule_arguments(E, N, g.grid4)
        if "ulp" in g.name:                                  # one ulp of the origin moves the argument off the integer
            assert (ac != np.floor(ac)) != (ar != np.floor(ar)) or g.pixel == "q", g.name
            assert ac != np.floor(ac) or ar != np.floor(ar), g.name
        cell = int(orc.cells(np.float64(E), np.float64(N), g.grid4, sc.EDGE_GW, sc.EDGE_GH))
        assert (cell >= 0) == g.on, g.name
    assert sum(g.on for g in grids.values()) == 5


@pytest.mark.parametrize("fault", orc.CELL_FAULTS)
def test_planted_cell_rule_error_is_reported(fault):
    """The comparison of the bin tests is np.array_equal with orc.cells: the planted rule must give another cell on an edge grid."""
    differs = []
    for g in sc.edge_grids(EP, NP, EQ, NQ):
        E, N = np.array([EP, EQ]), np.array([NP, NQ])
        if not np.array_equal(orc.cells(E, N, g.grid4, sc.EDGE_GW, sc.EDGE_GH, fault), orc.cells(E, N, g.grid4, sc.EDGE_GW, sc.EDGE_GH)):
            differs.append(g.name)
    assert "q on the upper column edge" in differs, differs
    # away from the edges the planted rules agree with the kernel's: random points do not tell them apart
    rng = np.random.default_rng(5)
    E, N = EP + rng.uniform(-20.0, 60.0, 1000), NP + rng.uniform(-60.0, 20.0, 1000)
    g = sc.edge_grids(EP, NP, EQ, NQ)[0]
    assert np.array_equal(orc.cells(E, N, g.grid4, 200, 200, fault), orc.cells(E, N, g.grid4, 200, 200))


def test_run_masks_hold_the_run_lengths_they_promise():
    def lengths(m):
        d = np.diff(np.concatenate([[0], m.reshape(-1).astype(np.int64), [0]]))
        return set((np.nonzero(d == -1)[0] - np.nonzero(d == 1)[0]).tolist())
    assert lengths(sc.run_mask("runs of 1", 53, 41)) == {1} and sc.run_mask("runs of 1", 53, 41).sum() == (53 * 41 + 1) // 2
    assert sc.run_mask("runs of 64", 128, 64).all()
    for H, W in ((53, 41), (128, 64)):
        assert lengths(sc.run_mask("runs of 1 to 64", H, W)) >= set(range(1, 65))
    assert (53 * 41) % 64 != 0 and 257 % 64 == 1              # a partial last wave
    assert sc.BIN_SIZES == [(1, 1), (1, 63), (1, 64), (1, 65), (1, 255), (1, 257), (300, 1), (1, 300), (37, 41)]


# ---- the mean's interval ---------------------------------------------------------------------------------------------------------
def _means(c, how):
    out = np.full(c.gh * c.gw, np.float32(-999.0), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for cc, v in _buckets(c).items():
            if how == "sequential":
                out[cc] = np.float32(np.cumsum(v.astype(np.float64))[-1] / v.size)
            elif how == "pairwise":
                out[cc] = np.float32(np.sum(v.astype(np.float64)) / v.size)
            elif how == "reversed":
                out[cc] = np.float32(np.cumsum(v[::-1].astype(np.float64))[-1] / v.size)
            else:
                out[cc] = np.cumsum(v, dtype=np.float32)[-1] / np.float32(v.size)
    return out


@pytest.mark.parametrize("name", sc.CASES)
def test_float64_sums_lie_in_the_mean_s_interval(name):
    c, ref = sc.case(name), _ref(name)
    for how in ("sequential", "pairwise", "reversed"):
        orc.check(_means(c, how), ref, "mean", -999.0)


@pytest.mark.parametrize("name", sc.CANCEL_CASES)
def test_a_float32_sum_leaves_the_mean_s_interval(name):
    c, ref = sc.case(name), _ref(name)
    with pytest.raises(AssertionError, match="outside its interval"):
        orc.check(_means(c, "float32"), ref, "mean", -999.0)
    got = _means(c, "float32")
    lo, hi = (ref.mean_exact - ref.delta).astype(np.float32), (ref.mean_exact + ref.delta).astype(np.float32)
    outside = ~((got >= lo) & (got <= hi))[:6]
    assert outside.all() if name == "cancel 1e6" else outside.any(), outside       # under cancellation in every tier, not in one alone


def test_the_interval_is_no_looser_than_one_ulp_without_cancellation():
    """Where all values of a bucket have one sign, delta is below half a float32 ulp of the mean (for m + 1 < 2^28), so the
    interval holds at most the two float32 neighbours of mean_exact: at least as tight as 1 ulp of a float64 sum."""
    for name in ("sizes 2^k", "near 1e4"):
        c, ref = sc.case(name), _ref(name)
        one_sign = np.array([cc for cc, v in _buckets(c).items() if v.size > 1 and ((v > 0).all() or (v < 0).all())], np.int64)
        if name == "near 1e4":
            assert one_sign.size == 6
        lo, hi = (ref.mean_exact - ref.delta).astype(np.float32), (ref.mean_exact + ref.delta).astype(np.float32)
        for cc in one_sign:
            assert np.nextafter(lo[cc], np.float32(np.inf)) >= hi[cc]
