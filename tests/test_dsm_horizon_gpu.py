"""Horizon maps and what the Python layer builds on them on the MI355X (smvs_dsm_horizon, dsm.horizon / sky_view_factor /
horizon_lit / sun_exposure_from_horizon) against the numpy oracle (tests/dsm_horizon_oracle.py): tangents by equal bits, NaN
and -inf included, no cell excused.  The case matrix of tests/dsm_horizon_scene.py (sizes around the wave of lines, the
transposes' tile and the rows loaded ahead; twelve azimuths at two resolutions, mixed orientations in every call; bowl, dome,
sawtooth, voids, edge values), batches of 1 to 65 directions, closed forms, guard words, garbage in the workspace, side
streams, repeated calls, the host checks, and the agreement with cast_shadows."""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest
import torch

import dsm_horizon_oracle as ho
import dsm_horizon_scene as sc
import dsm_sun_oracle as so
from dsm_testkit import dev, lib, scene as _scene  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ND = sc.ND
ERR_ARG = 1                                                                # SMVS_ERR_ARG
GUARD = 64


def _horizon_c(z, nodata, dirs, ws=None, guard=GUARD, stream=None):
    """The C entry on a host grid: tan_h inside a buffer with `guard` elements at both ends, the workspace full of 0xff unless
    one is given, on `stream` -> (K, gh, gw) float32."""
    from satmvs_amd import _lib
    d = torch.device("cuda", 0)
    gh, gw = z.shape
    K = len(dirs)
    n = K * gw * gh
    zd = z if isinstance(z, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(z, np.float32)).to(d)
    nbytes = _lib.load().smvs_dsm_horizon_workspace_bytes(gw, gh, K)
    assert nbytes > 0
    if ws is None:
        ws = torch.full((nbytes,), 0xff, dtype=torch.uint8, device=d)
    assert ws.numel() >= nbytes
    out = torch.full((n + 2 * guard,), 12345.0, dtype=torch.float32, device=d)
    host_dirs = np.ascontiguousarray(np.array(dirs, np.float64).reshape(K, 4))
    torch.cuda.synchronize()
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        _lib.call("smvs_dsm_horizon", _lib.ptr(zd), gw, gh, float(nodata), host_dirs.ctypes.data_as(C.c_void_p), K,
                  C.c_void_p(out.data_ptr() + 4 * guard), _lib.ptr(ws), ws.numel(), _lib.current_stream(d))
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[:guard] == np.float32(12345.0)).all() and (h[n + guard:] == np.float32(12345.0)).all()
    return h[guard:n + guard].reshape(K, gh, gw)


# ---- the matrix ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", sc.GROUPS)
def test_horizon_against_the_oracle(dev, group):
    for name, z, nodata, dirs in sc.matrix(group):
        sc.compare(_horizon_c(z, nodata, dirs), ho.horizon(z, nodata, dirs), name)


@pytest.fixture(scope="module")
def sixty_four():
    """One grid, 64 evenly spaced azimuths, the oracle's maps: shared by the batching tests and left unchanged."""
    from satmvs_amd import dsm
    shape = (45, 52)
    z = sc.special(shape, 500)
    azimuths = dsm.horizon_azimuths(64)
    return z, azimuths, sc.directions(shape, azimuths, sc.RESOLUTIONS[1]), ho.horizon(z, ND, sc.directions(shape, azimuths, sc.RESOLUTIONS[1]))


@pytest.mark.parametrize("K", [1, 2, 3, 16, 17, 64])
def test_batches_have_equal_bits(dev, sixty_four, K):
    """K directions in one call (with a stride through the 64, so that every batch mixes both orientations) against the
    oracle, and against the same directions one call each."""
    z, _, dirs, want = sixty_four
    pick = {1: [7], 2: [0, 16], 3: [0, 21, 42], 16: list(range(0, 64, 4))}.get(K, list(range(K)))
    got = _horizon_c(z, ND, [dirs[k] for k in pick])
    sc.compare(got, want[pick], K)
    if K > 1:
        orient = {abs(dirs[k][1]) >= abs(dirs[k][0]) for k in pick}
        assert orient == {True, False}
    for j in (0, K - 1):
        sc.compare(_horizon_c(z, ND, [dirs[pick[j]]]), got[j:j + 1], (K, j, "alone"))


def test_sixty_five_azimuths_through_python(dev, sixty_four):
    from satmvs_amd import dsm
    z, azimuths, _, want = sixty_four
    grid = dsm.DSMGrid(0.0, 0.0, sc.RESOLUTIONS[1][0], sc.RESOLUTIONS[1][1], z.shape[1], z.shape[0])
    az65 = azimuths + [123.0]
    got = dsm.horizon(z, grid, az65)
    assert isinstance(got, np.ndarray) and got.shape == (65,) + z.shape
    sc.compare(got[:64], want, "the first 64 of 65")
    sc.compare(got[64:], dsm.horizon(z, grid, [123.0]), "the 65th alone")
    sc.compare(got[64:], ho.horizon(z, ND, [ho.terms(grid, 123.0)]), "the 65th against the oracle")
    on = dsm.horizon(torch.from_numpy(z).to(dev), grid, az65[60:])
    assert isinstance(on, torch.Tensor) and on.is_cuda
    sc.compare(on.cpu().numpy(), got[60:], "a device tensor")
    sc.compare(dsm.horizon(z.astype(np.float64), grid, [33.0]), ho.horizon(z, ND, [ho.terms(grid, 33.0)]), "float64 in")


# ---- closed forms ----------------------------------------------------------------------------------------------------------------
def test_a_wall_and_a_plane(dev):
    z = sc.wall((3, 60), 40, 12.5)
    east, west = sc.directions((3, 60), [90.0, 270.0])
    t = _horizon_c(z, ND, [east, west])
    for n in (1, 2, 7, 40):
        assert np.all(t[0][:, 40 - n] == np.float32(256.0 * 12.5 / (1280.0 * n)))          # T = 256 h / dP
    assert np.all(t[0][:, 41:59] == 0.0) and np.all(t[0][:, 59] == -np.inf) and np.all(t[1][:, 41] == np.float32(2.5))
    p = _horizon_c(sc.plane((4, 50)), ND, sc.directions((4, 50), [90.0, 270.0]))
    assert np.all(p[0][:, :49] == np.float32(0.1)) and np.all(p[0][:, 49] == -np.inf)
    assert np.all(p[1][:, 1:] == np.float32(-0.1)) and np.all(p[1][:, 0] == -np.inf)


# ---- call hygiene ----------------------------------------------------------------------------------------------------------------
def test_horizon_entry_repeats_streams_and_workspaces(dev, lib):
    """A side stream, equal bits over two calls, and a larger call before a smaller one on one workspace (guard words and a
    workspace full of 0xff are in every call of this file)."""
    big, small = sc.special((150, 310), 50, voids=0.05), sc.special((70, 33), 51)
    dirs_big, dirs_small = sc.directions((150, 310), [33.0, 123.0, 213.0, 315.0]), sc.directions((70, 33), [0.0, 90.0])
    nbytes = lib.smvs_dsm_horizon_workspace_bytes(310, 150, 4)
    assert nbytes >= lib.smvs_dsm_horizon_workspace_bytes(33, 70, 2) > 0
    ws = torch.full((nbytes,), 0xff, dtype=torch.uint8, device=dev)
    bd = torch.from_numpy(big).to(dev)
    want = ho.horizon(big, ND, dirs_big)
    first = _horizon_c(bd, ND, dirs_big, ws=ws)
    again = _horizon_c(bd, ND, dirs_big, ws=ws)
    side = _horizon_c(bd, ND, dirs_big, stream=torch.cuda.Stream(dev))
    for got in (first, again, side):
        sc.compare(got, want, "repeats")
    assert np.array_equal(first.view(np.uint32), again.view(np.uint32))
    sc.compare(_horizon_c(small, ND, dirs_small, ws=ws), ho.horizon(small, ND, dirs_small), "the smaller call on the used workspace")


def test_the_size_query(lib):
    for size in ((0, 5, 1), (5, 0, 1), (-1, 5, 1), (65536, 32768, 1), (5, 5, 0), (5, 5, 65), (5, 5, -1)):
        assert lib.smvs_dsm_horizon_workspace_bytes(*size) == 0, size
    one, sixteen, many = (lib.smvs_dsm_horizon_workspace_bytes(100, 80, k) for k in (1, 16, 64))
    assert 0 < one < sixteen < many                           # q and its transpose, then per direction a grid of links and a transposed map
    assert one >= 4 * 100 * 80 * 4 and many - sixteen >= 48 * 2 * 100 * 80 * 4


def test_horizon_rejections(dev, lib):
    gw, gh = 40, 30
    z = torch.zeros((gh, gw), dtype=torch.float32, device=dev)
    out = torch.full((2, gh, gw), 77.0, dtype=torch.float32, device=dev)
    nbytes = lib.smvs_dsm_horizon_workspace_bytes(gw, gh, 2)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    P = lambda t: t.data_ptr()
    inf, nan = float("inf"), float("nan")
    good = [0.2, -0.05, 1280.0, -320.0, -0.1, 0.2, -640.0, 1280.0]
    ok = dict(z=P(z), gw=gw, gh=gh, dirs=good, n=2, out=P(out), ws=P(ws), nbytes=nbytes)

    def run(**change):
        a = dict(ok, **change)
        host = None if a["dirs"] is None else (C.c_double * len(a["dirs"]))(*a["dirs"])
        return lib.smvs_dsm_horizon(a["z"], a["gw"], a["gh"], -999.0, host, a["n"], a["out"], a["ws"], a["nbytes"], None)

    def second(ucol, urow, a, b):
        return dict(dirs=good[:4] + [ucol, urow, a, b])

    bad = [dict(z=None), dict(dirs=None), dict(out=None), dict(ws=None), dict(gw=0), dict(gh=-1), dict(gw=65536, gh=32768),
           dict(n=0), dict(n=-1), dict(n=65, dirs=good[:4] * 65),
           second(nan, 0.2, -640.0, 1280.0), second(-0.1, inf, -640.0, 1280.0), second(-0.1, 0.2, nan, 1280.0), second(-0.1, 0.2, -640.0, -inf),
           second(0.0, 0.0, 0.0, 1280.0), second(-0.0, 0.0, -640.0, 1280.0),
           second(-0.1, 0.2, 640.0, 1280.0), second(-0.1, 0.2, -640.0, -1280.0),            # a against ucol, b against urow
           second(-0.1, 0.2, -640.0, 3.9), second(0.2, -0.1, 3.9, -640.0),                  # the term along the scan below 4
           second(-0.1, 0.2, -640.0, 2.0 ** 37 / gh), second(0.2, 0.1, 2.0 ** 37 / gw, 640.0),   # |a| gw + |b| gh reaches 2^37
           dict(out=P(z)), dict(ws=P(z)), dict(ws=P(out)), dict(out=P(ws)), dict(out=P(ws) + 256), dict(out=P(z) + 4),
           dict(nbytes=nbytes - 1), dict(nbytes=0)]
    for change in bad:
        assert run(**change) == ERR_ARG and lib.smvs_last_error().decode(), change
    torch.cuda.synchronize()
    assert (out == 77.0).all()                                # nothing ran
    assert run() == 0 and run(n=1) == 0 and run(**second(-0.1, 0.0, -640.0, 0.0)) == 0 and run(**second(0.0, 0.2, 0.0, 4.0)) == 0
    torch.cuda.synchronize()


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
GH, GW = 100, 120
LISTED = [22.5 * k for k in range(16)]


@pytest.fixture(scope="module")
def built():
    """The test terrain with its blocks and voids, and the device's own 16 horizon maps of it (left unchanged)."""
    from satmvs_amd import dsm
    from satmvs_amd.dsm import DSMGrid
    grid = DSMGrid(500000.0, 4000000.0, 5.0, 4.0, GW, GH)
    c, r = np.meshgrid(np.arange(GW), np.arange(GH))
    z = _scene(grid.e0 + grid.xres * c, grid.n0 - grid.yres * r, seed=70, voids=0.02)
    t = dsm.horizon(z, grid, LISTED)
    sc.compare(t, ho.horizon(z, ND, [ho.terms(grid, a) for a in LISTED]), "the 16 maps of the terrain")
    return z, grid, t


def test_sky_view_factor(dev, built):
    """Held to 2^-50 relative: sums of 16 terms in (0, 1], each one float64 product, sum and quotient."""
    from satmvs_amd import dsm
    z, grid, t = built
    ok = ho.valid(z, ND)
    want = ho.sky_view_factor(t)
    for got in (dsm.sky_view_factor(t), dsm.sky_view_factor(torch.from_numpy(t).to(dev)).cpu().numpy()):
        assert got.dtype == np.float64 and np.array_equal(np.isnan(got), ~ok)
        err = np.abs(got[ok] - want[ok]) / want[ok]
        print("sky_view_factor: largest relative error %.3g, bound %.3g" % (err.max(), 2.0 ** -50))
        assert err.max() <= 2.0 ** -50
        assert 0.0 < got[ok].min() < 0.9 and got[ok].max() <= 1.0


def test_horizon_lit(dev, built):
    from satmvs_amd import dsm
    z, grid, t = built
    td = torch.from_numpy(t).to(dev)
    for az, el in ((90.0, 20.0), (135.0, 10.0), (100.0, 15.0), (350.0, 25.0), (-11.0, 30.0), (11.25, 40.0)):
        for interp in ("linear", "nearest"):
            want = ho.horizon_lit(t, LISTED, az, el, interp)
            got = dsm.horizon_lit(td, LISTED, az, el, interp)
            assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8
            assert np.array_equal(got.cpu().numpy(), want), (az, el, interp)
    assert (ho.horizon_lit(t, LISTED, 100.0, 15.0) == 2).any()


def test_sun_exposure_from_horizon(dev, built):
    from satmvs_amd import dsm
    z, grid, t = built
    ok = ho.valid(z, ND)
    suns, weights = [(110.0, 20.0), (180.0, 55.0), (250.0, 20.0)], [1.0, 2.5, 0.5]
    dzde, dzdn = dsm.gradient(z, grid)
    for incidence in (True, False):
        for interp in ("linear", "nearest"):
            want = ho.exposure(t, LISTED, suns, weights, dzde, dzdn, incidence, interp)
            got = dsm.sun_exposure_from_horizon(z, grid, t, LISTED, suns, weights, incidence=incidence, interp=interp)
            assert got.dtype == np.float32 and np.array_equal(np.isnan(got), ~ok)
            # the tolerance of sun_exposure's test: float32 rounding of a sum below 4 (2^-23) plus, per sun, the last bits of sqrt and quotient
            assert np.abs(got[ok].astype(np.float64) - want[ok]).max() <= 2.0 ** -21
            if not incidence:
                assert np.array_equal(got[ok], want[ok].astype(np.float32))
    ones = dsm.sun_exposure_from_horizon(torch.from_numpy(z).to(dev), grid, torch.from_numpy(t).to(dev), LISTED, suns, incidence=False)
    assert isinstance(ones, torch.Tensor) and float(ones[torch.from_numpy(ok).to(dev)].max()) == 3.0


# ---- agreement with cast_shadows -------------------------------------------------------------------------------------------------
def test_horizon_lit_agrees_with_cast_shadows(dev):
    """With the same azimuth and tol = 0, horizon_lit equals the shade of cast_shadows at every valid cell whose T differs from
    k = tan E by more than a bound, and at most 1 % of the valid cells are excused.

    The scene's heights are multiples of 2^-8 m, so q is exact: q_j - q_i = 256 (z_j - z_i).  cast_shadows hides cell i iff
    z_j - z_i > k d_ij for some valid cell j of its line towards the sun, d_ij the distance along the azimuth (the float64
    roundings of its keys are 10^-13 m); horizon_lit hides it iff (q_j - q_i) / (P_j - P_i) > k for some such j, and
    P_j - P_i = 256 d_ij + e with |e| <= 1: each P is rounded once, by at most half a unit.  So the slope the horizon takes to
    j is the shadow's times 256 d_ij / (P_j - P_i), off by at most its own size over the smallest step of P along a line, which
    is at least dP_min = (the term along the scan) - 1.  If the two maps differ at i, some j has its two slopes on different
    sides of k, the horizon's one no larger in size than T, so |T - k| <= |T| / dP_min; the float32 rounding of T adds 2^-24 |T|.
    Cells with |T - k| <= |T| (1 / dP_min + 2^-23) are excused, all others must agree."""
    from satmvs_amd import dsm
    rng = np.random.default_rng(80)
    gh, gw = 120, 140
    grid = dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, gw, gh)
    z = so.box_on_plane(gh, gw, 45, 74, 50, 89, 30.0)                       # a 30 m box, 30 x 40 cells
    z = (z + rng.integers(-3, 4, z.shape).astype(np.float32) / np.float32(256.0)).astype(np.float32)
    z[rng.random(z.shape) < 0.05] = ND
    ok = ho.valid(z, ND)
    azimuths = [20.0, 75.0, 135.0, 200.0, 260.0, 330.0]
    t = dsm.horizon(z, grid, azimuths)
    excused = total = 0
    for k, az in enumerate(azimuths):
        ucol, urow, a, b = dsm.horizon_terms(grid, az)
        dp_min = (abs(b) if abs(urow) >= abs(ucol) else abs(a)) - 1.0       # one step along the scan, both roundings against it
        for el in (15.0, 35.0, 60.0):
            tan_e = math.tan(math.radians(el))
            shade = dsm.cast_shadows(z, grid, az, el, tol=0.0)
            lit = dsm.horizon_lit(t, azimuths, az, el)
            T = t[k].astype(np.float64)
            with np.errstate(invalid="ignore"):
                near = ok & np.isfinite(T) & (np.abs(T - tan_e) <= np.abs(T) * (1.0 / dp_min + 2.0 ** -23))
            assert np.array_equal(lit == 0, shade == 0)
            assert np.array_equal(lit[ok & ~near], shade[ok & ~near]), (az, el, int((lit[ok & ~near] != shade[ok & ~near]).sum()))
            excused += int(near.sum())
            total += int(ok.sum())
            assert (shade == 2).any() and (shade == 1).any()
    print("excused %d of %d cells (%.4f %%)" % (excused, total, 100.0 * excused / total))
    assert excused <= 0.01 * total
