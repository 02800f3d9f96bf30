"""The DSM meshes on the device against the numpy statements of the rule (tests/dsm_mesh_oracle.py): the error map, every array
of the mesh and the heights by np.array_equal, z and the heights by their bits, no triangle excused.  The grids round the root
squares, the scenes with their voids, every tile and tolerance, the edges of the height quantum, an error on the threshold and
one unit above it, levels of detail from one error map, closed forms beyond the oracle's reach, the calling conditions of the
C entries (guard words, workspaces full of anything, a capacity one too small, a side stream, rejections that write nothing)
and the chain extract_dtm -> mesh -> write_ply with an orthophoto's colours."""
import ctypes

import numpy as np
import pytest
import torch

import dsm_mesh_oracle as mo
from dsm_testkit import dev, lib, same_bits                  # noqa: F401

pytestmark = pytest.mark.gpu

OUT = ("triangles", "tri_level", "vertices", "z")


def _grid(gh, gw):
    from satmvs_amd import dsm
    return dsm.DSMGrid(400000.0, 3500000.0, mo.XRES, mo.YRES, gw, gh)


def _check(z, S, tols, heights=(), nodata=-999.0):
    """errors, mesh at every tol and heights at some, device against the array statement; -> the oracle's error map."""
    from satmvs_amd import dsm
    want_e = mo.errors_arrays(z, S, nodata)
    got_e = dsm.mesh_errors(z, tile=S, nodata=nodata)
    assert got_e.dtype == np.int64 and np.array_equal(got_e, want_e), ("errors", np.argwhere(got_e != want_e)[:5].tolist())
    for tol in tols:
        want = mo.mesh_arrays(want_e, z, S, tol, nodata)
        got = dsm.mesh(z, tol=tol, tile=S, nodata=nodata)
        assert mo.differing(got, want) == [], (S, tol)
        assert got["n_triangles"] == len(want["triangles"]) and got["n_vertices"] == len(want["vertices"])
        assert got["tile"] == S and got["tol_units"] == mo.threshold(tol, S)[0]
    for tol in heights:
        wh, wd = mo.heights_arrays(want_e, z, S, tol, nodata)
        gh_, gd = dsm.mesh_heights(z, tol, tile=S, nodata=nodata, return_dev=True)
        assert same_bits(gh_, wh) and np.array_equal(gd, wd), (S, tol)
    return want_e


# ---- grids -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mo.SMALL_GRIDS, ids=lambda s: "%dx%d" % s)
def test_small_grids(dev, shape):                            # noqa: F811
    z = mo.noise(*shape, seed=11)
    for S in (2, 4, 64):
        _check(z, S, (0.0, 0.5, 1e9), heights=(0.0, 0.5))
    from satmvs_amd import dsm
    if min(shape) == 1:
        assert dsm.mesh(z, tol=0.0, tile=2)["n_triangles"] == 0


@pytest.mark.parametrize("S,n", mo.ROOT_SIDES, ids=lambda v: str(v))
def test_root_squares_exact_and_spilling(dev, S, n):         # noqa: F811
    """n = S, S + 1, S + 2 vertices a side: short of one root square, one exactly, one spilling into the next."""
    z = mo.scene(n, n, seed=S + n, voids=0.02, salt=0.05)
    _check(z, S, (0.0, 0.5, 2.0, 1e9), heights=(0.5,))
    z = mo.scene(n, n + 3, seed=S, voids=0.0, salt=0.0)
    _check(z, S, (1.0 / 256.0, 2.0), heights=(2.0,))


_scenes = {}


def _scene(case):
    if case not in _scenes:
        gh, gw, voids = case
        _scenes[case] = mo.scene(gh, gw, seed=gh + int(100 * voids), voids=voids, salt=0.02)
    return _scenes[case]


@pytest.mark.parametrize("S", mo.TILES)
@pytest.mark.parametrize("case", mo.SCENES, ids=lambda c: "%dx%d-%d%%" % (c[0], c[1], round(100 * c[2])))
def test_scenes_tiles_and_tolerances(dev, case, S):          # noqa: F811
    _check(_scene(case), S, mo.TOLS, heights=(0.5,))


def test_all_cells_invalid_and_one_valid_cell(dev):          # noqa: F811
    from satmvs_amd import dsm
    z = np.full((37, 41), np.nan, np.float32)
    z[::2] = -999.0
    for S in (4, 16):
        _check(z, S, (0.0, 1e9), heights=(0.0,))
    assert dsm.mesh(z, tile=4)["n_triangles"] == 0 and (dsm.mesh_heights(z, 0.5, tile=4) == np.float32(-999.0)).all()
    z[20, 20] = 5.0
    for S in (4, 16):
        _check(z, S, (0.0, 1e9), heights=(0.0,))
    assert dsm.mesh(z, tile=4)["n_vertices"] == 0


def test_heights_at_the_edges_of_the_quantum(dev):           # noqa: F811
    """Heights on quantisation halves (ties to even), both zeros, NaN, +-Inf, +-32768 and one ulp beyond, another nodata."""
    gh, gw = 33, 40
    rng = np.random.default_rng(77)
    z = ((rng.integers(0, 40, (gh, gw)) + 0.5 * rng.integers(0, 2, (gh, gw))) / 256.0).astype(np.float32)
    z[rng.random((gh, gw)) < 0.3] *= -1
    z[2, 3], z[2, 4], z[5, 5], z[5, 9], z[9, 9], z[20, 20] = 0.0, -0.0, np.nan, np.inf, -np.inf, -999.0
    z[12, 30], z[12, 31] = 32768.0, np.nextafter(np.float32(32768.0), np.float32(np.inf))
    z[25, 7], z[25, 8] = -32768.0, np.nextafter(np.float32(-32768.0), np.float32(-np.inf))
    z[30, 30] = 7.25
    for nodata in (-999.0, 7.25):
        q, ok = mo.quantum(z, nodata)
        assert ok[12, 30] and ok[25, 7] and not ok[12, 31] and not ok[25, 8] and ok[20, 20] == (nodata == 7.25) and ok[30, 30] == (nodata == -999.0)
        for S in (8, 32):
            _check(z, S, (0.0, 1.0 / 256.0, 1.0, 300.0), heights=(0.0, 1.0), nodata=nodata)


def test_an_error_on_the_threshold_and_one_unit_above(dev):  # noqa: F811
    """5 x 5 at tile 4.  The centre raised by 2 quanta: both root triangles err by exactly 8 units = floor(256 tol) S at tol =
    2 / 256: not active, 2 triangles.  The corner (0, 0) raised by 3 quanta: the plane at (1, 1) is 9 / 4 quanta, 9 units, one
    above: active."""
    from satmvs_amd import dsm
    on = np.zeros((5, 5), np.float32)
    on[2, 2] = 2 / 256.0
    above = np.zeros((5, 5), np.float32)
    above[0, 0] = 3 / 256.0
    e_on, e_above = (_check(z, 4, (0.0, 1 / 256.0, 2 / 256.0, 3 / 256.0), heights=(2 / 256.0,)) for z in (on, above))
    assert e_on[2, 2] == 8 and e_above[2, 2] == 9
    assert dsm.mesh(on, tol=2 / 256.0, tile=4)["n_triangles"] == 2 and dsm.mesh(above, tol=2 / 256.0, tile=4)["n_triangles"] > 2
    assert dsm.mesh(above, tol=3 / 256.0, tile=4)["n_triangles"] == 2


def test_levels_of_detail_from_one_error_map(dev):           # noqa: F811
    from satmvs_amd import dsm
    z = _scene(mo.SCENES[4])
    zd = torch.from_numpy(z).to(dev)
    e = dsm.mesh_errors(zd, tile=64)
    before = e.clone()
    last = None
    for tol in (0.25, 0.5, 1.0, 2.0):
        reused, fresh = dsm.mesh(zd, tol=tol, tile=64, errors=e), dsm.mesh(zd, tol=tol, tile=64)
        assert all(torch.equal(reused[k], fresh[k]) for k in OUT)
        assert torch.equal(dsm.mesh_heights(zd, tol, tile=64, errors=e), dsm.mesh_heights(zd, tol, tile=64))
        assert last is None or reused["n_triangles"] <= last
        last = reused["n_triangles"]
    assert torch.equal(e, before)


# ---- closed forms beyond the oracle's reach ----------------------------------------------------------------------------------------
def _plane_on_device(n, dev):                                # noqa: F811
    r = torch.arange(n, device=dev, dtype=torch.float64)
    return ((1000.0 + 3.0 * r[:, None] - 5.0 * r[None, :]) / 256.0).float()


@pytest.mark.parametrize("n,S,count", [(2049, 1024, 8), (2305, 256, 162)])
def test_a_quantised_plane_gives_its_root_triangles(dev, n, S, count):      # noqa: F811
    from satmvs_amd import dsm
    z = _plane_on_device(n, dev)
    m = dsm.mesh(z, tol=0.0, tile=S)
    assert m["n_triangles"] == count and m["n_vertices"] == ((n - 1) // S + 1) ** 2
    assert bool((m["tri_level"] == 0).all()) and bool((m["vertices"] % S == 0).all())
    e = dsm.mesh_errors(z, tile=S)
    assert int(e.max()) == 0
    h, d = dsm.mesh_heights(z, 0.0, tile=S, return_dev=True)
    assert torch.equal(h, z) and int(d.abs().max()) == 0


def test_noise_at_tol_0_is_the_full_resolution(dev):         # noqa: F811
    """1500 x 1500: 2 * 1499^2 triangles, all of level 2 k; the scan over 4.5 M slots has two blocks at its second level."""
    from satmvs_amd import dsm
    n, S = 1500, 64
    g = torch.Generator(device="cpu").manual_seed(5)
    z = (torch.randint(0, 1 << 20, (n, n), generator=g).double() / 256.0).float().to(dev)
    m = dsm.mesh(z, tol=0.0, tile=S)
    t, v = m["triangles"].long(), m["vertices"].long()
    assert m["n_triangles"] == 2 * (n - 1) ** 2 == t.shape[0] and m["n_vertices"] == n * n
    assert bool((m["tri_level"] == 12).all()) and int(t.min()) == 0 and int(t.max()) == n * n - 1
    at = torch.arange(n * n, device=dev)
    assert torch.equal(v[:, 0], at % n) and torch.equal(v[:, 1], at // n) and torch.equal(m["z"], z.reshape(-1))
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    cross = (b[:, 0] - a[:, 0]) * (a[:, 1] - c[:, 1]) - (a[:, 1] - b[:, 1]) * (c[:, 0] - a[:, 0])     # x = col, y = -row
    assert bool((cross == 1).all())                           # half a cell each, counter-clockwise
    key = ((a[:, 1] + b[:, 1]) * (2 * n) + a[:, 0] + b[:, 0]) * 2
    assert bool((key[1:] >= key[:-1]).all()) and bool((key[2:] > key[:-2]).all())


# ---- heights -----------------------------------------------------------------------------------------------------------------------
def test_mesh_heights_against_the_dsm(dev):                  # noqa: F811
    """|height - z| <= floor(256 tol) / 256 + 2^-9 + spacing(height) / 2.  A covered vertex's plane lies within floor(256 tol) quanta
    of q / 256 (the guarantee); q = rn(256 z), so q / 256 lies within half a quantum, 2^-9 m, of z; and the height is the plane's
    value rounded once to the nearest float32, at most half the spacing of the float32 it lands on (rounding to a power of two
    from below errs by half the spacing of the binade beneath it, which is less).  The three terms and the difference of the two
    float32 values are exact in float64, so the comparison adds nothing of its own."""
    from satmvs_amd import dsm
    z = _scene(mo.SCENES[4])
    q, ok = mo.quantum(z)
    e = dsm.mesh_errors(z, tile=64)
    for tol in (0.0, 0.5, 2.0):
        units, thr = mo.threshold(tol, 64)
        h, d = dsm.mesh_heights(z, tol, tile=64, errors=e, return_dev=True)
        m = dsm.mesh(z, tol=tol, tile=64, errors=e)
        covered = d != mo.INF
        assert not covered[~ok].any() and (h[~covered] == np.float32(-999.0)).all()
        assert (np.abs(d[covered]) <= thr).all()
        assert (d[m["vertices"][:, 1], m["vertices"][:, 0]] == 0).all()
        assert same_bits(h[m["vertices"][:, 1], m["vertices"][:, 0]], (q[m["vertices"][:, 1], m["vertices"][:, 0]] / 256.0).astype(np.float32))
        assert (np.abs(h[covered].astype(np.float64) - z[covered].astype(np.float64)) <= units / 256.0 + 2.0 ** -9 + 0.5 * np.spacing(np.abs(h[covered])).astype(np.float64)).all()
        assert covered.sum() > 0.6 * ok.sum()


# ---- calling conditions ------------------------------------------------------------------------------------------------------------
def _native(z, S, tol, dev, fill=0x5a, stream=None, G=64, want_dev=True, nodata=-999.0):     # noqa: F811
    """The four entries called directly, every output and the workspace between guard words, the workspace full of `fill`."""
    from satmvs_amd import _lib
    lib = _lib.load()                                        # noqa: F811
    p = _lib.ptr
    stream = stream or _lib.current_stream(dev)
    gh, gw = z.shape
    n = gh * gw
    thr = mo.threshold(tol, S)[1]
    zd = torch.from_numpy(z).to(dev)
    guarded = lambda dt, m: torch.full((m + 2 * G,), 77, dtype=dt, device=dev)      # noqa: E731
    nbytes = lib.smvs_dsm_mesh_workspace_bytes(gw, gh, S)
    assert nbytes > 0
    ws = torch.full((nbytes + 512,), fill, dtype=torch.uint8, device=dev)
    e, counts, status = guarded(torch.int64, n), guarded(torch.int32, 2), guarded(torch.int32, 1)
    h, d = guarded(torch.float32, n), guarded(torch.int64, n)
    _lib.call("smvs_dsm_mesh_errors", p(zd), gw, gh, nodata, S, p(e[G:]), stream)
    _lib.call("smvs_dsm_mesh_heights", p(e[G:]), p(zd), gw, gh, nodata, S, thr, p(h[G:]), p(d[G:]) if want_dev else ctypes.c_void_p(0), p(ws[256:]), nbytes, stream)
    _lib.call("smvs_dsm_mesh_count", p(e[G:]), p(zd), gw, gh, nodata, S, thr, p(counts[G:]), p(ws[256:]), nbytes, stream)
    torch.cuda.synchronize()
    nt, nv = counts[G:G + 2].tolist()
    tri, lev, ver, zz = guarded(torch.int32, 3 * nt), guarded(torch.uint8, nt), guarded(torch.int32, 2 * nv), guarded(torch.float32, nv)
    for _ in range(2):                                       # the write may be repeated
        _lib.call("smvs_dsm_mesh_write", p(zd), gw, gh, S, nt, nv, p(tri[G:]), p(lev[G:]), p(ver[G:]), p(zz[G:]), p(status[G:]), p(ws[256:]), nbytes, stream)
    torch.cuda.synchronize()
    for t, m in ((e, n), (counts, 2), (status, 1), (h, n), (d, n), (tri, 3 * nt), (lev, nt), (ver, 2 * nv), (zz, nv)):
        assert bool((t[:G] == 77).all()) and bool((t[G + m:] == 77).all())
    if not want_dev:
        assert bool((d == 77).all())
    assert bool((ws[:256] == fill).all()) and bool((ws[256 + nbytes:] == fill).all()) and int(status[G]) == nt
    cut = lambda t, m, *shape: t[G:G + m].cpu().numpy().reshape(*shape)             # noqa: E731
    return {"errors": cut(e, n, gh, gw), "heights": cut(h, n, gh, gw), "dev": cut(d, n, gh, gw), "triangles": cut(tri, 3 * nt, nt, 3),
            "tri_level": cut(lev, nt, nt), "vertices": cut(ver, 2 * nv, nv, 2), "z": cut(zz, nv, nv)}


def test_guards_workspaces_a_side_stream_and_the_same_bits_twice(dev):        # noqa: F811
    from satmvs_amd import _lib
    z, S, tol = _scene(mo.SCENES[1]), 16, 0.5
    want_e = mo.errors_arrays(z, S)
    want = mo.mesh_arrays(want_e, z, S, tol)
    wh, wd = mo.heights_arrays(want_e, z, S, tol)
    runs = [_native(z, S, tol, dev, fill) for fill in (0xff, 0x00, 0x5a, 0x5a)]
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        runs.append(_native(z, S, tol, dev, 0xff, _lib.current_stream(dev)))
    runs.append(_native(z, S, tol, dev, want_dev=False))
    for i, got in enumerate(runs):
        assert np.array_equal(got["errors"], want_e) and mo.differing(got, want) == [] and same_bits(got["heights"], wh)
        assert i == len(runs) - 1 or np.array_equal(got["dev"], wd)


def test_a_capacity_one_too_small(dev):                      # noqa: F811
    from satmvs_amd import _lib, dsm
    z = torch.from_numpy(_scene(mo.SCENES[0])).to(dev)
    gh, gw = z.shape
    e = dsm.mesh_errors(z, tile=16)
    nbytes = _lib.load().smvs_dsm_mesh_workspace_bytes(gw, gh, 16)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    dsm._call(dev, "smvs_dsm_mesh_count", e, z, gw, gh, -999.0, 16, mo.threshold(0.5, 16)[1], counts, ws, nbytes)
    nt, nv = counts.tolist()
    assert nt > 100 and nv > 100
    for a, b in ((nt - 1, nv), (nt, nv - 1), (nt + 1, nv)):
        with pytest.raises(_lib.SatMVSNativeError, match="not the counts of its workspace"):
            dsm._mesh_status_checked(dsm._mesh_write(z, 16, a, b, ws, nbytes)[1], a, b)
    out, status = dsm._mesh_write(z, 16, nt, nv, ws, nbytes)  # the workspace is as count left it
    dsm._mesh_status_checked(status, nt, nv)
    want = dsm.mesh(z, tol=0.5, tile=16)
    assert all(torch.equal(out[k], want[k]) for k in OUT)


def test_a_larger_call_before_a_smaller_one(dev):            # noqa: F811
    big, small = _scene(mo.SCENES[3]), mo.noise(9, 11, seed=2)
    _check(big, 64, (0.5,), heights=(0.5,))
    _check(small, 4, (0.0, 0.5), heights=(0.5,))
    _check(big, 64, (0.5,), heights=(0.5,))


def test_device_tensors_in_and_out(dev, monkeypatch):        # noqa: F811
    """Tensors in, tensors out, and no grid goes to the host on the way (a Tensor.cpu() call fails the test)."""
    from satmvs_amd import dsm
    z = _scene(mo.SCENES[1])
    zd = torch.from_numpy(z).to(dev)

    def no_host_copy(self, *a, **k):
        raise AssertionError("a grid went to the host")
    monkeypatch.setattr(torch.Tensor, "cpu", no_host_copy)
    e = dsm.mesh_errors(zd, tile=32)
    m = dsm.mesh(zd, _grid(*z.shape), tol=0.5, tile=32, errors=e)
    h = dsm.mesh_heights(zd, 0.5, tile=32, errors=e)
    monkeypatch.undo()
    assert e.is_cuda and h.is_cuda and all(m[k].is_cuda for k in OUT + ("xyz",))
    want_e = mo.errors_arrays(z, 32)
    want = mo.mesh_arrays(want_e, z, 32, 0.5)
    assert np.array_equal(e.cpu().numpy(), want_e) and mo.differing({k: m[k].cpu().numpy() for k in OUT}, want) == []
    E, N = mo.grid_en(*z.shape)
    v = want["vertices"]
    assert np.array_equal(m["xyz"].cpu().numpy(), np.stack([E[v[:, 1], v[:, 0]], N[v[:, 1], v[:, 0]], want["z"].astype(np.float64)], axis=1))


def test_native_rejections_write_nothing(dev, lib):          # noqa: F811
    from satmvs_amd import _lib
    gw, gh, S = 9, 7, 4
    n = gw * gh
    stream = _lib.current_stream(dev)
    p, null = _lib.ptr, ctypes.c_void_p(0)
    nbytes = lib.smvs_dsm_mesh_workspace_bytes(gw, gh, S)
    names = ("dsm", "errors", "counts", "tri", "lev", "ver", "z", "status", "h", "d", "ws")
    buf = {k: torch.full((max(2 * n, nbytes // 8 + 1),), 77, dtype=torch.int64, device=dev) for k in names}
    b = lambda k: p(buf[k])                                  # noqa: E731

    def errors(dsm=b("dsm"), gw=gw, gh=gh, tile=S, errors=b("errors")):
        _lib.call("smvs_dsm_mesh_errors", dsm, gw, gh, -999.0, tile, errors, stream)

    def count(errors=b("errors"), dsm=b("dsm"), gw=gw, gh=gh, tile=S, thr=0, counts=b("counts"), ws=b("ws"), nbytes=nbytes):
        _lib.call("smvs_dsm_mesh_count", errors, dsm, gw, gh, -999.0, tile, thr, counts, ws, nbytes, stream)

    def write(dsm=b("dsm"), gw=gw, gh=gh, tile=S, nt=5, nv=5, tri=b("tri"), lev=b("lev"), ver=b("ver"), z=b("z"), status=b("status"), ws=b("ws"),
              nbytes=nbytes):
        _lib.call("smvs_dsm_mesh_write", dsm, gw, gh, tile, nt, nv, tri, lev, ver, z, status, ws, nbytes, stream)

    def heights(errors=b("errors"), dsm=b("dsm"), gw=gw, gh=gh, tile=S, thr=0, h=b("h"), d=b("d"), ws=b("ws"), nbytes=nbytes):
        _lib.call("smvs_dsm_mesh_heights", errors, dsm, gw, gh, -999.0, tile, thr, h, d, ws, nbytes, stream)

    def rejected(call, match, **kw):
        with pytest.raises(_lib.SatMVSNativeError, match=match):
            call(**kw)

    inside = lambda k, off: ctypes.c_void_p(buf[k].data_ptr() + off)               # noqa: E731
    for call, args in ((errors, ("dsm", "errors")), (count, ("errors", "dsm", "counts", "ws")),
                       (write, ("dsm", "tri", "lev", "ver", "z", "status", "ws")), (heights, ("errors", "dsm", "h", "ws"))):
        for name in args:
            rejected(call, "null pointer", **{name: null})
        rejected(call, "non-positive grid", gw=0)
        rejected(call, "non-positive grid", gh=-3)
        rejected(call, "below 2\\^29", gw=1 << 15, gh=1 << 14)
        for tile in (0, 1, 3, 48, 2048, -4):
            rejected(call, "power of two", tile=tile)
        if call is not errors:
            rejected(call, "workspace too small", nbytes=nbytes - 1)
            rejected(call, "workspace aliases", ws=inside("dsm", 4 * n - 1))
    rejected(errors, "errors aliases dsm", errors=inside("dsm", 4 * n - 1))
    rejected(count, "dsm aliases errors", dsm=inside("errors", 8 * n - 1))
    rejected(count, "counts aliases", counts=inside("errors", 8))
    rejected(count, "threshold", thr=-1)
    rejected(heights, "threshold", thr=-1)
    rejected(heights, "heights aliases", h=inside("dsm", 0))
    rejected(heights, "dev aliases", d=inside("h", 4 * n - 1))
    rejected(write, "negative counts", nt=-1)
    rejected(write, "negative counts", nv=-1)
    rejected(write, "than the grid holds", nt=2 * n + 1)
    rejected(write, "than the grid holds", nv=n + 1)
    rejected(write, "tri_level aliases", lev=inside("tri", 59))
    rejected(write, "status aliases", status=inside("z", 16))
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in buf.values())
    assert lib.smvs_dsm_mesh_workspace_bytes(0, 5, 4) == 0 and lib.smvs_dsm_mesh_workspace_bytes(5, 5, 3) == 0
    assert lib.smvs_dsm_mesh_workspace_bytes(1 << 15, 1 << 14, 4) == 0


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_dtm_to_a_coloured_ply(dev, tmp_path):               # noqa: F811
    """extract_dtm -> mesh(tol = 0.5) -> write_ply with the colours of an orthophoto on the same grid, read back.  On this
    smooth 62 x 76 scene the full resolution is 2 * 61 * 75 = 9 150 triangles.  Two recorded facts, neither a target: for the DTM
    that extract_dtm makes on an MI355X the array statement and the device both give 1 154 triangles at tile 64, 12.6 % (the
    figure this test prints); for the scene built without its blocks, a surface the CPU can make without the device and smoother
    than that DTM (extract_dtm leaves steps where the blocks stood), the array statement gives 869, 9.5 %.  The test asserts
    that the device's mesh is the oracle's for the device's DTM and strictly below the full resolution."""
    import dsm_render_oracle as ro
    from dsm_testkit import scene as kit_scene
    from satmvs_amd import dsm
    from satmvs_amd.transverse_mercator import whu_tlc_projection
    proj = whu_tlc_projection()
    H, W = 128, 160
    rpc = ro.view_rpc(H, W, 0.0, seed=11)
    grid = ro.grid_over([(rpc, (H, W))], proj.tm7(), 100.0, 160.0, 5.0, margin=20.0)
    zd = torch.from_numpy(kit_scene(*ro.cell_centres(grid), holes=False)).to(dev)
    dtm = dsm.extract_dtm(zd, grid)
    image = np.random.default_rng(1).uniform(0.0, 255.0, (H, W, 3)).astype(np.float32)
    ortho = dsm.orthorectify(image, rpc, dtm, grid, proj)
    colours = torch.nan_to_num(ortho).clamp(0, 255).to(torch.uint8).cpu().numpy()
    assert len(np.unique(colours)) > 50
    m = dsm.mesh(dtm, grid, tol=0.5, tile=64)
    host = dtm.cpu().numpy()
    want = mo.mesh(host, 64, 0.5)
    assert mo.differing({k: m[k].cpu().numpy() for k in OUT}, want) == []
    full = mo.full_resolution_count(host)
    print("dtm mesh: %d triangles of %d at full resolution (%.1f %%)" % (m["n_triangles"], full, 100.0 * m["n_triangles"] / max(full, 1)))
    assert 0 < m["n_triangles"] < full
    path = str(tmp_path / "dtm.ply")
    assert dsm.write_ply(path, m, grid, colors=colours) == m["n_triangles"]
    with open(path, "rb") as fh:
        blob = fh.read()
    head, body = blob.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    nv, nt = (int([ln for ln in lines if ln.startswith("element " + k)][0].split()[2]) for k in ("vertex", "face"))
    assert (nv, nt) == (m["n_vertices"], m["n_triangles"]) and "format binary_little_endian 1.0" in lines
    rec = np.frombuffer(body, dtype=[("p", "<f8", (3,)), ("rgb", "u1", (3,))], count=nv)
    faces = np.frombuffer(body, dtype=[("n", "u1"), ("v", "<i4", (3,))], count=nt, offset=nv * 27)
    assert len(body) == nv * 27 + nt * 13 and (faces["n"] == 3).all()
    v = m["vertices"].cpu().numpy()
    assert np.array_equal(faces["v"], m["triangles"].cpu().numpy()) and faces["v"].min() >= 0 and faces["v"].max() < nv
    assert np.array_equal(rec["p"], m["xyz"].cpu().numpy())
    assert np.array_equal(rec["p"][:, 0], grid.e0 + v[:, 0] * grid.xres) and np.array_equal(rec["p"][:, 1], grid.n0 - v[:, 1] * grid.yres)
    assert np.array_equal(rec["rgb"], colours[v[:, 1], v[:, 0]])
