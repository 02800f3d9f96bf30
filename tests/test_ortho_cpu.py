"""The orthophoto, the parts that run without a GPU: known answers of the numpy oracle (tests/ortho_oracle.py), argument checks
of smvs_rpc_ortho (rejected before any HIP call) and of dsm.visibility / dsm.orthorectify (before any device work), and the
TIFF + world file that write_ortho writes."""
import ctypes as C
import os

import numpy as np
import pytest

import dsm_render_oracle as ro
import ortho_oracle as oo
from dsm_testkit import lib, tilted_fixture, tm7  # noqa: F401  (fixtures)

H, W = 24, 32
tilted = tilted_fixture(H, W, seed=3)


def test_constant_dsm_is_visible_inside_the_footprint(tm7, tilted):
    grid = ro.grid_over([(tilted, (H, W))], tm7, 120.0, 130.0, 5.0, margin=15.0)
    z = np.full((grid.height, grid.width), 123.25, np.float32)
    o = oo.ortho(z, grid, -999.0, tm7, tilted, shape=(H, W))
    st = o["state"]
    assert set(np.unique(st)) == {oo.OUTSIDE, oo.VISIBLE}
    inside = (o["u"] >= 0) & (o["u"] <= W - 1) & (o["v"] >= 0) & (o["v"] <= H - 1)
    assert np.array_equal(st == oo.VISIBLE, inside)
    assert inside.sum() > 20 and (~inside).sum() > 20
    assert (o["K"] == 0).all()                                                # z == h_hi: no samples
    # a lower cell elsewhere does not hide ground far from it
    z2 = z.copy()
    z2[0, 0] = 100.0
    assert np.array_equal(oo.ortho(z2, grid, -999.0, tm7, tilted, shape=(H, W))["state"][1:, 1:], st[1:, 1:])


def test_image_bilinear_of_an_affine_image_is_exact():
    Hh, Ww = 7, 9
    i, j = np.mgrid[0:Hh, 0:Ww].astype(np.float64)
    img = np.stack([3.0 + 2.0 * j - 1.0 * i, 0.5 * i + 0.25 * j], axis=-1).astype(np.float32)   # exact in float32
    rng = np.random.default_rng(0)
    u = np.concatenate([rng.uniform(0, Ww - 1, 200), [0.0, Ww - 1, Ww - 1, 0.0, 3.0]])
    v = np.concatenate([rng.uniform(0, Hh - 1, 200), [0.0, Hh - 1, 0.0, Hh - 1, 2.0]])
    val, rng_ = oo.bilinear(img, u, v)
    want = np.stack([3.0 + 2.0 * u - 1.0 * v, 0.5 * v + 0.25 * u], axis=-1)
    assert np.array_equal(val, want.astype(np.float32))
    assert (rng_ > 0).all()
    # one column / one row: both taps are that column / row
    one = np.arange(5, dtype=np.float32).reshape(5, 1, 1)
    val, _ = oo.bilinear(one, np.zeros(3), np.array([0.0, 1.5, 4.0]))
    assert np.array_equal(val[:, 0], np.array([0.0, 1.5, 4.0], np.float32))


def test_block_hides_the_ground_behind_it(tm7, tilted):
    """Flat ground with one block: some ground cells are occluded, and every occluded cell is ground; without occlusion all
    ground in the footprint is visible."""
    grid = ro.grid_over([(tilted, (H, W))], tm7, 100.0, 140.0, 2.0, margin=10.0)
    z = np.full((grid.height, grid.width), 100.0, np.float32)
    r0, c0 = grid.height // 2 - 3, grid.width // 2 - 3
    z[r0:r0 + 6, c0:c0 + 6] = 140.0
    o = oo.ortho(z, grid, -999.0, tm7, tilted, shape=(H, W))
    occ = o["state"] == oo.OCCLUDED
    assert occ.sum() >= 6 and (z[occ] == 100.0).all()
    assert (o["state"][r0:r0 + 6, c0:c0 + 6] == oo.VISIBLE).all()                  # the roof
    off = oo.ortho(z, grid, -999.0, tm7, tilted, shape=(H, W), occlusion=False)
    assert not (off["state"] == oo.OCCLUDED).any()
    assert np.array_equal(off["state"] == oo.VISIBLE, (o["state"] == oo.VISIBLE) | occ)


def test_ortho_entry_rejects_bad_arguments_without_a_gpu(lib, tm7):
    from satmvs_amd import _lib
    d = C.c_void_p(16)
    grid4 = np.array([0.0, 0.0, 5.0, 5.0])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731

    def call(dsm=d, gw=8, gh=8, g4=grid4, t7=tm7, rpc=d, image=d, Hh=4, Ww=4, Cc=3, x0=0, y0=0, h_hi=160.0, occlusion=1,
             occ_tol=0.5, view=0, ortho=d, source=d, state=d):
        _lib.call("smvs_rpc_ortho", dsm, gw, gh, vp(g4) if g4 is not None else None, -999.0,
                  vp(t7) if t7 is not None else None, rpc, image, Hh, Ww, Cc, x0, y0, h_hi, occlusion, occ_tol, view,
                  ortho, source, state, None)

    for kw in ({"dsm": None}, {"g4": None}, {"t7": None}, {"rpc": None}, {"image": None}, {"ortho": None},
               {"source": None}, {"ortho": None, "image": None, "source": None, "state": None}):
        with pytest.raises(_lib.SatMVSNativeError, match="null pointer"):
            call(**kw)
    with pytest.raises(_lib.SatMVSNativeError, match="ortho needs source"):
        call(source=None, state=d)
    for cc in (0, 17, -1):
        with pytest.raises(_lib.SatMVSNativeError, match="channel count"):
            call(Cc=cc)
    with pytest.raises(_lib.SatMVSNativeError, match="non-positive dimension"):
        call(Ww=0)
    with pytest.raises(_lib.SatMVSNativeError, match="view too large"):
        call(Hh=65536, Ww=32768)
    with pytest.raises(_lib.SatMVSNativeError, match="non-positive grid"):
        call(gh=0)
    with pytest.raises(_lib.SatMVSNativeError, match="grid too large"):
        call(gw=65536, gh=32768)
    for g in ([0.0, 0.0, 0.0, 5.0], [0.0, 0.0, 5.0, -1.0], [np.nan, 0.0, 5.0, 5.0], [0.0, 0.0, np.inf, 5.0]):
        with pytest.raises(_lib.SatMVSNativeError, match="bad grid"):
            call(g4=np.array(g))
    bad = tm7.copy()
    bad[0] = -1.0
    with pytest.raises(_lib.SatMVSNativeError, match="projection parameters"):
        call(t7=bad)
    with pytest.raises(_lib.SatMVSNativeError, match="negative origin"):
        call(x0=-1)
    with pytest.raises(_lib.SatMVSNativeError, match="does not fit"):
        call(y0=2 ** 31 - 3)
    for h in (np.nan, np.inf, -np.inf):
        with pytest.raises(_lib.SatMVSNativeError, match="h_hi must be finite"):
            call(h_hi=h)
    for t in (np.nan, -0.1, np.inf):
        with pytest.raises(_lib.SatMVSNativeError, match="occ_tol"):
            call(occ_tol=t)
    with pytest.raises(_lib.SatMVSNativeError, match="view must be non-negative"):
        call(view=-1)


def test_python_entries_validate_before_the_gpu():
    from satmvs_amd import dsm
    from satmvs_amd.transverse_mercator import whu_tlc_projection
    proj = whu_tlc_projection()
    grid = dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, 6, 4)
    z = np.zeros((4, 6), np.float32)
    rpc = np.zeros(170)
    img = np.zeros((8, 8, 3), np.float32)
    vis_cases = [
        (dict(rpc=np.zeros(169)), "170 values"),
        (dict(shape=(0, 8)), "shape must be"),
        (dict(shape=(65536, 32768)), "shape must be"),
        (dict(origin=(-1, 0)), "origin must be"),
        (dict(dsm=np.zeros((6, 4), np.float32)), "differs from the grid"),
        (dict(occ_tol=float("nan")), "occ_tol"),
        (dict(occ_tol=-1.0), "occ_tol"),
        (dict(occ_tol=float("inf")), "occ_tol"),
    ]
    for kw, msg in vis_cases:
        args = dict(dsm=z, grid=grid, rpc=rpc, projection=proj, shape=(8, 8))
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            dsm.visibility(**args)
    ortho_cases = [
        (dict(rpcs=np.zeros(169)), "170 values"),
        (dict(rpcs=[rpc, rpc]), "one RPC per image"),
        (dict(images=[img, img], rpcs=[rpc]), "one RPC per image"),
        (dict(images=[img, np.zeros((8, 8, 4), np.float32)], rpcs=[rpc, rpc]), "same number of channels"),
        (dict(images=np.zeros((8, 8, 17), np.float32)), "1 .. 16 channels"),
        (dict(images=np.zeros((8, 8, 0), np.float32)), "1 .. 16 channels"),
        (dict(images=np.zeros((2, 8, 8, 3), np.float32)), r"\(H, W\) or \(H, W, C\)"),
        (dict(images=np.zeros((8, 8), np.complex64)), "real dtype"),
        (dict(images=[]), "no image"),
        (dict(origins=(-1, 0)), "origin must be"),
        (dict(origins=[(0, 0), (0, 0)]), "one origin per image"),
        (dict(dsm=np.zeros((6, 4), np.float32)), "differs from the grid"),
        (dict(occ_tol=-0.5), "occ_tol"),
        (dict(order="best"), "order must be"),
        (dict(order=[1]), "order must be"),
        (dict(order=[0, 0]), "order must be"),
        (dict(order=[0.0]), "order must be"),
    ]
    for kw, msg in ortho_cases:
        args = dict(images=img, rpcs=rpc, dsm=z, grid=grid, projection=proj)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            dsm.orthorectify(**args)


def test_write_ortho_round_trips(tmp_path):
    from PIL import Image
    from satmvs_amd import dsm
    from satmvs_amd.data_io import read_tfw
    grid = dsm.DSMGrid(512345.0, 3432100.0, 5.0, 2.5, 7, 5)
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    gray = rng.integers(0, 256, (5, 7), dtype=np.uint8)
    flt = rng.standard_normal((5, 7, 1)).astype(np.float32)
    for name, a, mode in (("rgb.tif", rgb, "RGB"), ("gray.tif", gray, "L"), ("gray1.tif", gray[:, :, None], "L"),
                          ("f.tif", flt, "F")):
        p = str(tmp_path / name)
        assert dsm.write_ortho(p, a, grid) == p
        im = Image.open(p)
        assert im.mode == mode
        back = np.array(im)
        assert np.array_equal(back.reshape(a.shape), a) and back.dtype == a.dtype
        t = read_tfw(os.path.splitext(p)[0] + ".tfw")
        g = dsm.DSMGrid(float(t[4]), float(t[5]), float(t[0]), float(-t[3]), back.shape[1], back.shape[0])
        assert g == grid and t[1] == 0.0 and t[2] == 0.0
    for bad in (np.zeros((5, 7, 3), np.float32), np.zeros((5, 7, 4), np.uint8), np.zeros((5, 7), np.int16),
                np.zeros((5, 7, 2), np.uint8), np.zeros((7, 5), np.uint8), np.zeros((5, 7), np.float64)):
        with pytest.raises(ValueError):
            dsm.write_ortho(str(tmp_path / "bad.tif"), bad, grid)
