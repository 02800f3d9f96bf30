"""DSM production, the parts that run without a GPU: the numpy Transverse Mercator mirror against the reference's outputs
(tests/golden/tm.npz), the world file and float32 TIFF round trips, grid snapping, and argument checks of the C entries."""
import ctypes as C
import os

import numpy as np
import pytest

import dsm_oracle as orc
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
