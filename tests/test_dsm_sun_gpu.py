"""Cast shadows, the gradient and what the Python layer builds on them on the MI355X (smvs_dsm_shadow, smvs_dsm_gradient,
dsm.cast_shadows / gradient / slope / aspect / hillshade / sun_exposure) against the numpy oracle (tests/dsm_sun_oracle.py):
shade by equal values, depth and the gradient by equal bits, no cell excused.  The case matrix of tests/dsm_sun_scene.py
(sizes around the band, the block and the transposes' tile; every octant boundary, halves and thirds in the shear, a shear
of 1e-18, irrational directions; voids of every kind, both zeros, +-FLT_MAX, a tie at tol), closed forms, guard words, garbage
in the workspace, side streams, repeated calls, and the host checks of both C entries."""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest
import torch

import dsm_sun_oracle as so
import dsm_sun_scene as sc
from dsm_testkit import dev, lib, same as _same, scene as _scene  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ND = sc.ND
ERR_ARG = 1                                                                # SMVS_ERR_ARG
GUARD = 64


def _shadow_c(z, nodata, u, ab, tol, depth=True, ws=None, guard=GUARD, stream=None):
    """The C entry on a host grid: shade and depth inside buffers with `guard` elements at both ends, the workspace full of
    0xff unless one is given, on `stream` -> (shade, depth or None)."""
    from satmvs_amd import _lib
    d = torch.device("cuda", 0)
    gh, gw = z.shape
    n = gw * gh
    zd = z if isinstance(z, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(z, np.float32)).to(d)
    nbytes = _lib.load().smvs_dsm_shadow_workspace_bytes(gw, gh)
    assert nbytes > 0
    if ws is None:
        ws = torch.full((nbytes,), 0xff, dtype=torch.uint8, device=d)
    assert ws.numel() >= nbytes
    sb = torch.full((n + 2 * guard,), 0x5a, dtype=torch.uint8, device=d)
    db = torch.full((n + 2 * guard,), 12345.0, dtype=torch.float32, device=d) if depth else None
    torch.cuda.synchronize()
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        _lib.call("smvs_dsm_shadow", _lib.ptr(zd), gw, gh, float(nodata), float(u[0]), float(u[1]), float(ab[0]), float(ab[1]), float(tol),
                  C.c_void_p(sb.data_ptr() + guard), C.c_void_p(db.data_ptr() + 4 * guard) if depth else None,
                  _lib.ptr(ws), ws.numel(), _lib.current_stream(d))
    torch.cuda.synchronize()
    out = []
    for b, fill in ((sb, 0x5a), (db, 12345.0)):
        if b is None:
            out.append(None)
            continue
        h = b.cpu().numpy()
        assert (h[:guard] == h.dtype.type(fill)).all() and (h[n + guard:] == h.dtype.type(fill)).all()
        out.append(h[guard:n + guard].reshape(gh, gw))
    return tuple(out)


# ---- the matrix ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", sc.GROUPS)
def test_shadow_against_the_oracle(dev, group):
    for name, z, nodata, u, ab, tol in sc.matrix(group):
        sc.compare(_shadow_c(z, nodata, u, ab, tol), so.shadow_scan(z, nodata, *u, *ab, tol), name)


def test_shadow_tol_pairs(dev):
    z, nodata, u, ab, tol = sc.tol_pairs()
    shade, depth = _shadow_c(z, nodata, u, ab, tol)
    assert shade.tolist() == [[1, 1], [1, 2]] and depth[1].tolist() == [1.0, 1.0] and np.all(depth[0] == -np.inf)


# ---- closed forms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u", sc.MAJORS + [(1.0, -1.0), (0.0, 1.0), (1.0, 0.0)])
def test_a_pillar_shadows_its_own_line(dev, u):
    """One pillar on a plane: shadowed are exactly the cells of the pillar's line that lie behind it and whose g is more than
    tol below the pillar's."""
    gh, gw, pr, pc, tol = 90, 110, 44, 57, 0.1
    a, b = sc.terms(*u, k=0.4)
    z = np.zeros((gh, gw), np.float32)
    z[pr, pc] = 37.0
    row_major, s, ascending = so.lines(gh, gw, *u)
    r, c = np.mgrid[0:gh, 0:gw]
    line, pos = (c - s[r], r) if row_major else (r - s[c], c)
    behind = (pos > pos[pr, pc]) if ascending else (pos < pos[pr, pc])
    g = so.keys(z, a, b)
    want = (line == line[pr, pc]) & behind & (g[pr, pc] - g > tol)
    assert 10 < want.sum() < 40                               # 37 m / (0.4 x 5 m) = 18.5 cells along the ray
    shade, depth = _shadow_c(z, ND, u, (a, b), tol)
    assert np.array_equal(shade == 2, want) and (shade != 0).all()
    sc.compare((shade, depth), so.shadow_scan(z, ND, *u, a, b, tol), u)


@pytest.mark.parametrize("elevation", [20.0, 45.0])
def test_box_on_a_plane(dev, elevation):
    """No cell farther than 1.5 cells outside the swept footprint is shadowed, none farther than 1.5 cells inside is lit (the
    margin: a line stays within one cell of the ray across it, and the polygon is that of the cell centres); the inside set is
    not empty.  The reference rule holds this with no violation on the CPU (tests/test_dsm_sun_cpu.py)."""
    from satmvs_amd import dsm
    box = dict(r0=37, r1=42, c0=36, c1=43, height=30.0, res=5.0)
    grid = dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, 80, 80)
    z = so.box_on_plane(80, 80, box["r0"], box["r1"], box["c0"], box["c1"], box["height"])
    zd = torch.from_numpy(z).to(dev)
    for azimuth in (0.0, 33.0, 90.0, 200.0, 315.0):
        shade = dsm.cast_shadows(zd, grid, azimuth, elevation).cpu().numpy()
        out, lit, n_inside = so.box_violations(shade, azimuth=azimuth, elevation=elevation, **box)
        assert (out, lit) == (0, 0) and n_inside > 0, (azimuth, elevation, out, lit, n_inside)


def test_terrain_and_blocks(dev):
    """The test terrain casts no shadow under a sun above its steepest slope; with the blocks, every shadow lies behind a block:
    farther from the sun than the blocks' sunward end and within the longest possible shadow of a block cell."""
    from satmvs_amd import dsm
    c, r = np.meshgrid(np.arange(120), np.arange(100))
    grid = dsm.DSMGrid(500000.0, 4000000.0, 5.0, 5.0, 120, 100)
    E, N = grid.e0 + 5.0 * c, grid.n0 - 5.0 * r
    bare, built = _scene(E, N, blocks=False, holes=False), _scene(E, N, holes=False)
    blocks = built != bare
    reach = float(built.max() - bare.min()) / math.tan(math.radians(30.0)) / 5.0 + 1.5      # cells: the highest top over the lowest ground
    br, bc = np.nonzero(blocks)
    for azimuth in (0.0, 77.0, 135.0, 250.0):
        assert not (dsm.cast_shadows(bare, grid, azimuth, 30.0) == 2).any(), azimuth
        shade = dsm.cast_shadows(built, grid, azimuth, 30.0)
        sc.compare((shade, None), so.shadow_scan(built, ND, *dsm.sun_terms(grid, azimuth, 30.0), 0.1), azimuth)
        sr, scol = np.nonzero(shade == 2)
        assert len(sr) > 20
        sA, cA = math.sin(math.radians(azimuth)), math.cos(math.radians(azimuth))
        towards = lambda rr, cc: cc * sA - rr * cA            # distance towards the sun [cells]
        assert towards(sr, scol).max() < towards(br, bc).max()
        nearest = np.sqrt(((sr[:, None] - br[None, :]) ** 2 + (scol[:, None] - bc[None, :]) ** 2).min(axis=1))
        assert nearest.max() <= reach, (azimuth, nearest.max(), reach)


# ---- call hygiene ----------------------------------------------------------------------------------------------------------------
def test_shadow_entry_repeats_streams_and_workspaces(dev, lib):
    """Depth null and non-null, a side stream, equal bits over two calls, and a larger call before a smaller one on one
    workspace (guard words and a workspace full of 0xff are in every call of this file)."""
    big, small = sc.relief((300, 700), 50), sc.special((70, 130), 51)
    bd = torch.from_numpy(big).to(dev)
    nbytes = lib.smvs_dsm_shadow_workspace_bytes(700, 300)
    assert nbytes >= lib.smvs_dsm_shadow_workspace_bytes(130, 70) > 0
    ws = torch.full((nbytes,), 0xff, dtype=torch.uint8, device=dev)
    for u in sc.MAJORS:
        ab = sc.terms(*u, k=0.3)
        want = so.shadow_scan(big, ND, *u, *ab, 0.1)
        first = _shadow_c(bd, ND, u, ab, 0.1, ws=ws)
        again = _shadow_c(bd, ND, u, ab, 0.1, ws=ws)
        side = _shadow_c(bd, ND, u, ab, 0.1, stream=torch.cuda.Stream(dev))
        bare = _shadow_c(bd, ND, u, ab, 0.1, depth=False)
        for got in (first, again, side):
            sc.compare(got, want, u)
        assert bare[1] is None and np.array_equal(bare[0], want[0])
        assert np.array_equal(first[1].view(np.uint32), again[1].view(np.uint32))
        sc.compare(_shadow_c(small, ND, u, sc.terms(*u), 0.1, ws=ws), so.shadow_scan(small, ND, *u, *sc.terms(*u), 0.1), "the smaller call on the used workspace")


def test_shadow_rejections(dev, lib):
    gw, gh = 40, 30
    z = torch.zeros((gh, gw), dtype=torch.float32, device=dev)
    shade = torch.full((gh, gw), 77, dtype=torch.uint8, device=dev)
    depth = torch.full((gh, gw), 77.0, dtype=torch.float32, device=dev)
    nbytes = lib.smvs_dsm_shadow_workspace_bytes(gw, gh)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    P = lambda t: t.data_ptr()
    inf, nan = float("inf"), float("nan")
    ok = dict(z=P(z), gw=gw, gh=gh, ucol=0.3, urow=-1.0, a=1.0, b=-2.0, tol=0.1, shade=P(shade), depth=P(depth), ws=P(ws), n=nbytes)

    def run(**change):
        a = dict(ok, **change)
        return lib.smvs_dsm_shadow(a["z"], a["gw"], a["gh"], -999.0, a["ucol"], a["urow"], a["a"], a["b"], a["tol"], a["shade"], a["depth"],
                                   a["ws"], a["n"], None)

    bad = [dict(z=None), dict(shade=None), dict(ws=None), dict(gw=0), dict(gh=-1), dict(gw=65536, gh=32768),
           dict(ucol=nan), dict(ucol=inf), dict(urow=nan), dict(urow=-inf), dict(ucol=0.0, urow=0.0), dict(ucol=-0.0, urow=0.0),
           dict(a=nan), dict(a=inf), dict(b=nan), dict(b=-inf), dict(a=1e300), dict(b=-1e300),
           dict(tol=-1e-9), dict(tol=nan), dict(tol=inf),
           dict(shade=P(z)), dict(depth=P(z)), dict(depth=P(shade)), dict(shade=P(depth)), dict(ws=P(z)), dict(ws=P(shade)), dict(ws=P(depth)),
           dict(shade=P(ws)), dict(depth=P(ws) + 256), dict(n=nbytes - 1), dict(n=0)]
    for change in bad:
        assert run(**change) == ERR_ARG and lib.smvs_last_error().decode(), change
    for size in ((0, 5), (5, 0), (-1, 5), (65536, 32768)):
        assert lib.smvs_dsm_shadow_workspace_bytes(*size) == 0, size
    torch.cuda.synchronize()
    assert (shade == 77).all() and (depth == 77.0).all()      # nothing ran
    assert run() == 0 and run(depth=None) == 0 and run(ucol=0.0) == 0 and run(urow=0.0) == 0 and run(tol=0.0) == 0
    torch.cuda.synchronize()


# ---- gradient --------------------------------------------------------------------------------------------------------------------
def _gradient_c(z, nodata, xres, yres, guard=GUARD):
    from satmvs_amd import _lib
    d = torch.device("cuda", 0)
    gh, gw = z.shape
    n = gw * gh
    zd = torch.from_numpy(np.ascontiguousarray(z, np.float32)).to(d)
    bufs = [torch.full((n + 2 * guard,), 12345.0, dtype=torch.float32, device=d) for _ in range(2)]
    torch.cuda.synchronize()
    _lib.call("smvs_dsm_gradient", _lib.ptr(zd), gw, gh, float(nodata), float(xres), float(yres),
              *[C.c_void_p(b.data_ptr() + 4 * guard) for b in bufs], _lib.current_stream(d))
    torch.cuda.synchronize()
    out = []
    for b in bufs:
        h = b.cpu().numpy()
        assert (h[:guard] == np.float32(12345.0)).all() and (h[n + guard:] == np.float32(12345.0)).all()
        out.append(h[guard:n + guard].reshape(gh, gw))
    return out


@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (67, 1), (2, 2), (3, 3), (67, 130), (257, 301)])
def test_gradient_against_the_oracle(dev, shape):
    for seed, (xres, yres), nodata in ((60, (5.0, 5.0), ND), (61, (0.3, 7.0), ND), (62, (5.0, 5.0), np.float32(np.nan))):
        z = sc.special(shape, seed)
        if np.isnan(nodata):
            z = np.where(np.isnan(z), np.float32(3.0), z)
        got, want = _gradient_c(z, nodata, xres, yres), so.gradient(z, nodata, xres, yres)
        _same(got[0], want[0], (shape, seed, "dzde"))
        _same(got[1], want[1], (shape, seed, "dzdn"))
    z = sc.relief(shape, 63)                                  # moderate heights: every valid cell gets a finite slope
    got, want = _gradient_c(z, ND, 5.0, 5.0), so.gradient(z, ND, 5.0, 5.0)
    _same(got[0], want[0], (shape, "relief dzde"))
    _same(got[1], want[1], (shape, "relief dzdn"))
    assert np.isfinite(got[0][so.valid(z, ND)]).all()


def test_gradient_rejections(dev, lib):
    gw, gh = 40, 30
    z = torch.zeros((gh, gw), dtype=torch.float32, device=dev)
    de = torch.full((gh, gw), 77.0, dtype=torch.float32, device=dev)
    dn = torch.full((gh, gw), 77.0, dtype=torch.float32, device=dev)
    P = lambda t: t.data_ptr()
    ok = dict(z=P(z), gw=gw, gh=gh, xres=5.0, yres=5.0, de=P(de), dn=P(dn))
    bad = [dict(z=None), dict(de=None), dict(dn=None), dict(gw=0), dict(gh=-3), dict(gw=65536, gh=32768), dict(xres=0.0), dict(yres=0.0),
           dict(xres=-5.0), dict(yres=float("nan")), dict(xres=float("inf")), dict(de=P(z)), dict(dn=P(z)), dict(dn=P(de)), dict(dn=P(de) + 4)]
    for change in bad:
        a = dict(ok, **change)
        rc = lib.smvs_dsm_gradient(a["z"], a["gw"], a["gh"], -999.0, a["xres"], a["yres"], a["de"], a["dn"], None)
        assert rc == ERR_ARG and lib.smvs_last_error().decode(), change
    torch.cuda.synchronize()
    assert (de == 77.0).all() and (dn == 77.0).all()          # nothing ran


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
GH, GW = 100, 120


@pytest.fixture(scope="module")
def built():
    from satmvs_amd.dsm import DSMGrid
    grid = DSMGrid(500000.0, 4000000.0, 5.0, 4.0, GW, GH)
    c, r = np.meshgrid(np.arange(GW), np.arange(GH))
    return _scene(grid.e0 + grid.xres * c, grid.n0 - grid.yres * r, seed=70, voids=0.02), grid


def test_cast_shadows_numpy_and_tensor(dev, built):
    from satmvs_amd import dsm
    z, grid = built
    for azimuth, elevation in ((135.0, 25.0), (280.0, 50.0)):
        want = so.shadow_scan(z, ND, *dsm.sun_terms(grid, azimuth, elevation), 0.1)
        got = dsm.cast_shadows(z, grid, azimuth, elevation, return_depth=True)
        assert isinstance(got[0], np.ndarray) and (got[0] == 2).any()
        sc.compare(got, want, (azimuth, elevation))
        on = dsm.cast_shadows(torch.from_numpy(z).to(dev), grid, azimuth, elevation, return_depth=True)
        assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in on)
        sc.compare(tuple(t.cpu().numpy() for t in on), want, (azimuth, elevation, "tensor"))
        alone = dsm.cast_shadows(z.astype(np.float64), grid, azimuth, elevation, tol=0.5)
        assert isinstance(alone, np.ndarray) and np.array_equal(alone, so.shadow_scan(z, ND, *dsm.sun_terms(grid, azimuth, elevation), 0.5)[0])


def test_hillshade(dev, built):
    """Within 2^-22 absolute of the float64 numpy evaluation on the GPU's own gradient: one float32 rounding of a value in
    [0, 1] (2^-25) plus last-bit differences of float64 sqrt and quotient."""
    from satmvs_amd import dsm
    z, grid = built
    ok = so.valid(z, ND)
    dzde, dzdn = dsm.gradient(z, grid)
    want_g = so.gradient(z, ND, grid.xres, grid.yres)
    _same(dzde, want_g[0], "dzde")
    _same(dzdn, want_g[1], "dzdn")
    for azimuth, elevation in ((315.0, 45.0), (100.0, 15.0)):
        want = so.cos_incidence(dzde, dzdn, azimuth, elevation)
        h = dsm.hillshade(z, grid, azimuth, elevation)
        assert h.dtype == np.float32 and np.array_equal(np.isnan(h), ~ok)
        err = np.abs(h[ok].astype(np.float64) - want[ok]).max()
        print("hillshade at (%g, %g): largest error %.3g, bound %.3g" % (azimuth, elevation, err, 2.0 ** -22))
        assert err <= 2.0 ** -22 and h[ok].min() >= 0.0 and h[ok].max() <= 1.0
        shade = dsm.cast_shadows(z, grid, azimuth, elevation)
        hs = dsm.hillshade(z, grid, azimuth, elevation, shadows=True)
        assert (shade == 2).any() and np.array_equal(hs[ok] == 0.0, (shade[ok] == 2) | (h[ok] == 0.0))
        assert np.array_equal(hs[shade == 1], h[shade == 1]) and np.array_equal(np.isnan(hs), ~ok)
    default = dsm.hillshade(torch.from_numpy(z).to(dev), grid)
    assert isinstance(default, torch.Tensor) and np.array_equal(default.cpu().numpy(), dsm.hillshade(z, grid, 315.0, 45.0), equal_nan=True)


def test_sun_exposure_is_the_sum_by_hand(dev, built):
    from satmvs_amd import dsm
    z, grid = built
    ok = so.valid(z, ND)
    suns, weights = [(110.0, 20.0), (180.0, 55.0), (250.0, 20.0)], [1.0, 2.5, 0.5]
    dzde, dzdn = dsm.gradient(z, grid)
    for incidence in (True, False):
        total = np.zeros(z.shape, np.float64)
        for (az, el), w in zip(suns, weights):
            lit = dsm.cast_shadows(z, grid, az, el) != 2
            total += np.where(lit, w * (so.cos_incidence(dzde, dzdn, az, el) if incidence else 1.0), 0.0)
        got = dsm.sun_exposure(z, grid, suns, weights, incidence=incidence)
        assert got.dtype == np.float32 and np.array_equal(np.isnan(got), ~ok)
        # float32 rounding of a sum below 4 (2^-23) plus, per sun, the last bits of sqrt and quotient
        assert np.abs(got[ok].astype(np.float64) - total[ok]).max() <= 2.0 ** -21
        if not incidence:
            assert np.array_equal(got[ok], total[ok].astype(np.float32))
    ones = dsm.sun_exposure(z, grid, suns, incidence=False)
    assert ones[ok].max() == 3.0 and ones[ok].min() < 3.0


def test_slope_and_aspect_on_a_tilted_plane(dev):
    from satmvs_amd import dsm
    grid = dsm.DSMGrid(0.0, 0.0, 5.0, 4.0, 40, 30)
    c, r = np.meshgrid(np.arange(40), np.arange(30))
    z = (50.0 + 0.5 * (5.0 * c) + 0.25 * (4.0 * r)).astype(np.float32)     # rises 0.5 m/m eastwards and 0.25 m/m southwards
    z[10, 10] = ND
    inner = np.zeros(z.shape, bool)
    inner[1:-1, 1:-1] = True
    inner[9:12, 9:12] = False
    dzde, dzdn = dsm.gradient(z, grid)
    assert np.all(dzde[inner] == np.float32(0.5)) and np.all(dzdn[inner] == np.float32(-0.25)) and dzde[10, 10] == ND
    s, sr, a = dsm.slope(z, grid), dsm.slope(z, grid, degrees=False), dsm.aspect(z, grid)
    assert np.allclose(s[inner], math.degrees(math.atan(math.hypot(0.5, 0.25))), rtol=1e-6)
    assert np.allclose(sr[inner], math.atan(math.hypot(0.5, 0.25)), rtol=1e-6)
    assert np.allclose(a[inner], math.degrees(math.atan2(-0.5, 0.25)) % 360.0, rtol=1e-6)      # downslope: west-north-west
    assert np.isnan(s[10, 10]) and np.isnan(a[10, 10]) and not np.isnan(s[inner]).any()
    flat = np.full((5, 6), 9.0, np.float32)
    g6 = dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, 6, 5)
    assert np.isnan(dsm.aspect(flat, g6)).all() and (dsm.slope(flat, g6) == 0.0).all()
    north = np.repeat(np.arange(5, dtype=np.float32)[:, None], 6, axis=1)     # rises southwards: faces north, aspect 0
    an = dsm.aspect(torch.from_numpy(north).to(dev), g6)
    assert isinstance(an, torch.Tensor) and (an.cpu().numpy()[:, 1:-1] == 0.0).all()           # (the corners see a side slope)
