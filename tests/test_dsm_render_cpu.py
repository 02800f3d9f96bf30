"""Rendering a DSM into a view, the parts that run without a GPU: known answers of the numpy oracle (tests/dsm_render_oracle.py),
argument checks of smvs_rpc_dsm_render (rejected before any HIP call) and of dsm.render_heights (before any device work)."""
import ctypes as C

import numpy as np
import pytest

import dsm_render_oracle as ro
from dsm_testkit import lib, tilted_fixture, tm7  # noqa: F401  (fixtures)

H, W = 24, 32
tilted = tilted_fixture(H, W, seed=3)


def test_constant_dsm_renders_the_constant(tm7, tilted):
    grid = ro.grid_over([(tilted, (H, W))], tm7, 120.0, 130.0, 5.0, margin=15.0)
    z = np.full((grid.height, grid.width), 123.25, np.float32)
    o = ro.render_view(z, grid, -999.0, tm7, tilted, H, W)
    assert (o["height"] == np.float32(123.25)).all()
    assert (o["K"] == 1).all() and (o["evals"] == 1).all()                   # h_lo == h_hi: the first sample is the hit


def test_planar_dsm_renders_the_plane(tm7, tilted):
    grid = ro.grid_over([(tilted, (H, W))], tm7, 80.0, 220.0, 5.0, margin=15.0)
    E, N = ro.cell_centres(grid)
    Ec, Nc = E.mean(), N.mean()

    def plane(e, n):
        return 150.0 + 0.12 * (e - Ec) - 0.09 * (n - Nc)

    z = plane(E, N).astype(np.float32)
    o = ro.render_view(z, grid, -999.0, tm7, tilted, H, W)
    h = o["height"].astype(np.float64)
    assert np.isfinite(h).all()                                              # the grid covers every ray
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    Eh, Nh = ro.G(tilted, tm7, x, y, h)
    assert np.abs(plane(Eh, Nh) - h).max() <= 1e-3
    assert (o["K"] > 1).all()                                                # the march took several steps


def test_rays_off_the_grid_are_invalid(tm7, tilted):
    full = ro.grid_over([(tilted, (H, W))], tm7, 100.0, 160.0, 5.0, margin=15.0)
    from satmvs_amd.dsm import DSMGrid
    grid = DSMGrid(full.e0, full.n0, 5.0, 5.0, full.width // 2, full.height)     # the western half only
    E, N = ro.cell_centres(grid)
    z = (130.0 + 20.0 * np.sin(E / 40.0)).astype(np.float32)
    h_lo, h_hi = ro.h_range(z, -999.0)
    o = ro.render_view(z, grid, -999.0, tm7, tilted, H, W)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    off_everywhere = np.ones((H, W), bool)
    for hh in np.linspace(h_lo, h_hi, 65):                                    # denser than any march of this scene
        e, n = ro.G(tilted, tm7, x, y, np.full(x.shape, hh))
        ok, _ = ro.surface(z, grid.grid4(), -999.0, e, n)
        off_everywhere &= ~ok
    assert off_everywhere.sum() > 20 and (~off_everywhere).sum() > 20
    assert np.isnan(o["height"][off_everywhere]).all()
    # a grid far away from the view: nothing to see
    far = DSMGrid(grid.e0 + 1e5, grid.n0, 5.0, 5.0, grid.width, grid.height)
    assert np.isnan(ro.render_view(z, far, -999.0, tm7, tilted, H, W)["height"]).all()


def test_ray_entering_the_grid_just_before_the_hit_is_invalid(tm7, tilted):
    """Flat ground at 100 (one cell at 160 sets the bracket).  The hit is the last sample h_K = h_lo; where the sample before
    it is off the grid the ray may have passed under unknown terrain, so the pixel is invalid; where both are on, it reads 100."""
    full = ro.grid_over([(tilted, (H, W))], tm7, 100.0, 160.0, 5.0, margin=15.0)
    from satmvs_amd.dsm import DSMGrid
    # cut the grid on the side the rays come from: the view shifts west with height, so drop columns in the west
    cut = 12
    grid = DSMGrid(full.e0 + cut * 5.0, full.n0, 5.0, 5.0, full.width - cut, full.height)
    z = np.full((grid.height, grid.width), 100.0, np.float32)
    z[-1, -1] = 160.0
    o = ro.render_view(z, grid, -999.0, tm7, tilted, H, W)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    e_hi, n_hi = ro.G(tilted, tm7, x, y, np.full(x.shape, 160.0))
    e_lo, n_lo = ro.G(tilted, tm7, x, y, np.full(x.shape, 100.0))
    K = ro.march_steps(e_hi, n_hi, e_lo, n_lo, 5.0, 5.0)
    h_before = 160.0 - (K - 1) * (60.0 / K)
    e_b, n_b = ro.G(tilted, tm7, x, y, h_before)
    ok_before, _ = ro.surface(z, grid.grid4(), -999.0, e_b, n_b)
    ok_last, _ = ro.surface(z, grid.grid4(), -999.0, e_lo, n_lo)
    entering = ok_last & ~ok_before
    seen = ok_last & ok_before
    assert entering.sum() >= 5 and seen.sum() >= 5
    assert np.isnan(o["height"][entering]).all()
    assert (np.abs(o["height"][seen] - 100.0) <= 1e-3).all()
    assert (o["K"] == K).all()


def test_render_entry_rejects_bad_arguments_without_a_gpu(lib, tm7):
    from satmvs_amd import _lib
    d = C.c_void_p(16)
    grid4 = np.array([0.0, 0.0, 5.0, 5.0])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731

    def call(dsm=d, gw=8, gh=8, g4=grid4, t7=tm7, rpc=d, Hh=4, Ww=4, x0=0, y0=0, h_lo=100.0, h_hi=160.0, tol=1e-3, out=d):
        _lib.call("smvs_rpc_dsm_render", dsm, gw, gh, vp(g4) if g4 is not None else None, -999.0,
                  vp(t7) if t7 is not None else None, rpc, Hh, Ww, x0, y0, h_lo, h_hi, tol, out, None)

    for kw in ({"dsm": None}, {"g4": None}, {"t7": None}, {"rpc": None}, {"out": None}):
        with pytest.raises(_lib.SatMVSNativeError, match="null pointer"):
            call(**kw)
    with pytest.raises(_lib.SatMVSNativeError, match="non-positive dimension"):
        call(Hh=0)
    with pytest.raises(_lib.SatMVSNativeError, match="view too large"):
        call(Hh=65536, Ww=32768)
    with pytest.raises(_lib.SatMVSNativeError, match="non-positive grid"):
        call(gw=0)
    with pytest.raises(_lib.SatMVSNativeError, match="grid too large"):
        call(gw=65536, gh=32768)
    for g in ([0.0, 0.0, 0.0, 5.0], [0.0, 0.0, 5.0, -1.0], [np.nan, 0.0, 5.0, 5.0], [0.0, 0.0, np.inf, 5.0]):
        with pytest.raises(_lib.SatMVSNativeError, match="bad grid"):
            call(g4=np.array(g))
    bad = tm7.copy()
    bad[4] = 0.0
    with pytest.raises(_lib.SatMVSNativeError, match="projection parameters"):
        call(t7=bad)
    for x0, y0 in ((-1, 0), (0, -5)):
        with pytest.raises(_lib.SatMVSNativeError, match="negative origin"):
            call(x0=x0, y0=y0)
    with pytest.raises(_lib.SatMVSNativeError, match="does not fit"):
        call(x0=2 ** 31 - 3)
    for lo, hi in ((160.0, 100.0), (np.nan, 100.0), (100.0, np.inf)):
        with pytest.raises(_lib.SatMVSNativeError, match="height bracket"):
            call(h_lo=lo, h_hi=hi)
    for tol in (0.0, -1e-3, np.nan, np.inf):
        with pytest.raises(_lib.SatMVSNativeError, match="tol must be"):
            call(tol=tol)


def test_render_heights_validates_before_the_gpu(tm7):
    from satmvs_amd import dsm
    from satmvs_amd.transverse_mercator import whu_tlc_projection
    proj = whu_tlc_projection()
    grid = dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, 6, 4)
    z = np.zeros((4, 6), np.float32)
    rpc = np.zeros(170)
    cases = [
        (dict(rpc=np.zeros(169)), "170 values"),
        (dict(shape=(0, 8)), "shape must be"),
        (dict(shape=(8,)), "shape must be"),
        (dict(shape=(8.0, 8)), "shape must be"),
        (dict(shape=(65536, 32768)), "shape must be"),
        (dict(origin=(-1, 0)), "origin must be"),
        (dict(origin=(0, 2 ** 31 - 4)), "origin must be"),
        (dict(dsm=np.zeros((6, 4), np.float32)), "differs from the grid"),
        (dict(tol=0.0), "tol must be"),
        (dict(tol=float("nan")), "tol must be"),
    ]
    for kw, msg in cases:
        args = dict(dsm=z, grid=grid, rpc=rpc, projection=proj, shape=(8, 8))
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            dsm.render_heights(**args)
