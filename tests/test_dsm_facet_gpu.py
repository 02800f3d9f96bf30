"""Facets on the device against the numpy oracle (tests/dsm_facet_oracle.py): Gx, Gy, planar, labels, n, every moment and the
float64 plane by its bits are compared for equality, no cell or facet excused.  Every native labelling call here runs with guard
words round its outputs and its workspace, the workspace seeded."""
import functools
import json

import numpy as np
import pytest
import torch

import dsm_facet_oracle as fo
import dsm_facet_scene as fs
from dsm_testkit import dev, lib  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
ND = fs.ND
G = 64                                                       # guard words on both sides of a buffer
COMBOS = [(conn, grow, masked) for conn in (4, 8) for grow in (0, 1) for masked in (False, True)]


def _guarded(n, dtype, dev, fill=77):
    return torch.full((n + 2 * G,), fill, dtype=dtype, device=dev)


def _intact(buf, n, fill=77):
    return bool((buf[:G] == fill).all()) and bool((buf[G + n:] == fill).all())


def _native_label(zd, md, T, Ax, Ay, conn, grow, fill=0x5a, stream=None):
    """smvs_dsm_facet_label at its C entry -> (labels (gh, gw) int32 numpy, n)."""
    from satmvs_amd import _lib
    dev = zd.device
    gh, gw = zd.shape
    nbytes = _lib.load().smvs_dsm_facet_workspace_bytes(gw, gh)
    ws = torch.full((nbytes + 2 * G,), fill, dtype=torch.uint8, device=dev)
    ws[:G] = 77
    ws[G + nbytes:] = 77
    out, n_out = _guarded(gh * gw, torch.int32, dev), _guarded(1, torch.int32, dev)
    _lib.call("smvs_dsm_facet_label", _lib.ptr(zd), _lib.ptr(md) if md is not None else None, gw, gh, -999.0, T, Ax, Ay, conn, grow,
              _lib.ptr(out[G:]), _lib.ptr(n_out[G:]), _lib.ptr(ws[G:]), nbytes, stream if stream is not None else _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert _intact(out, gh * gw) and _intact(n_out, 1) and _intact(ws, nbytes), "a guard word changed"
    return out[G:G + gh * gw].cpu().numpy().reshape(gh, gw), int(n_out[G])


def _native_normals(zd, md, T):
    from satmvs_amd import _lib
    dev = zd.device
    gh, gw = zd.shape
    Gx, Gy, pl = _guarded(gh * gw, torch.int32, dev), _guarded(gh * gw, torch.int32, dev), _guarded(gh * gw, torch.uint8, dev)
    _lib.call("smvs_dsm_facet_normals", _lib.ptr(zd), _lib.ptr(md) if md is not None else None, gw, gh, -999.0, T,
              _lib.ptr(Gx[G:]), _lib.ptr(Gy[G:]), _lib.ptr(pl[G:]), _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert all(_intact(b, gh * gw) for b in (Gx, Gy, pl))
    return tuple(b[G:G + gh * gw].cpu().numpy().reshape(gh, gw) for b in (Gx, Gy, pl))


def _native_planes(lab_d, zd, n):
    """smvs_dsm_facet_planes at its C entry, outputs seeded and guarded -> the oracle's dict."""
    from satmvs_amd import _lib
    dev = zd.device
    gh, gw = zd.shape
    spec = {"sums": (torch.int64, 4 * n), "centre": (torch.int32, 3 * n), "moments": (torch.int64, 8 * n), "plane": (torch.float64, 3 * n),
            "sse": (torch.int64, n), "max_abs": (torch.int32, n)}
    bufs = {k: _guarded(m, dt, dev) for k, (dt, m) in spec.items()}
    _lib.call("smvs_dsm_facet_planes", _lib.ptr(lab_d), _lib.ptr(zd), gw, gh, -999.0, n, *[_lib.ptr(bufs[k][G:]) for k in spec], _lib.current_stream(dev))
    torch.cuda.synchronize()
    for k, (dt, m) in spec.items():
        assert _intact(bufs[k], m), k
    shape = {"sums": (n, 4), "centre": (n, 3), "moments": (n, 8), "plane": (n, 3), "sse": (n,), "max_abs": (n,)}
    return {k: bufs[k][G:G + m].cpu().numpy().reshape(shape[k]) for k, (dt, m) in spec.items()}


def _check(dev, z, T, Ax, Ay, what, combos=COMBOS, planes=True, mask_seed=5):
    """Normals, labels under every combination of connectivity, growth and mask, and the planes of the last labelling against
    the oracle.  -> (labels, n) of the last combination."""
    zd = torch.from_numpy(z).to(dev)
    mask = fs.random_mask(*z.shape, seed=mask_seed)
    md = torch.from_numpy(mask).to(dev)
    for m_np, m_d in ((None, None), (mask, md)):
        for got, want, name in zip(_native_normals(zd, m_d, T), fo.normals(z, T, m_np), ("Gx", "Gy", "planar")):
            d = fo.differing(got, want)
            assert d is None, (what, name, m_np is not None, d)
    for conn, grow, masked in combos:
        want, nw = fo.facets(z, T, Ax, Ay, conn, bool(grow), mask if masked else None)
        got, n = _native_label(zd, md if masked else None, T, Ax, Ay, conn, grow)
        d = fo.differing(got, want)
        assert n == nw and d is None, (what, conn, grow, masked, n, nw, d)
    if planes and z.size < 2 ** 24:
        fo.same_planes(_native_planes(torch.from_numpy(got).to(dev), zd, n), fo.planes(want, nw, z), what)
    return got, n


# ---- sizes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (67, 1), (2, 2), (3, 3), (67, 3)])
def test_small_grids(dev, shape):
    for z in (fs.quantised_plane(*shape), fs.kit(*shape, seed=sum(shape), voids=0.05)):
        labels, n = _check(dev, z, 64, 1024, 1024, shape)
        if min(shape) < 3:
            assert n == 0 and not labels.any()


@pytest.mark.parametrize("shape", [(15, 63), (16, 64), (17, 65), (16, 65), (17, 64), (33, 129)])
def test_either_side_of_the_tile(dev, shape):
    """The labelling tile is 16 rows of 64 columns."""
    labels, n = _check(dev, fs.quantised_plane(*shape), 0, 0, 0, shape, combos=[(8, 1, False), (4, 0, False)])
    assert n == 1
    _check(dev, fs.kit(*shape, seed=7, voids=0.05, salt=0.02), 64, 1024, 1024, shape)


@functools.lru_cache(maxsize=None)
def _kit(voids, salt):
    return fs.kit(257, 301, seed=int(100 * voids) + 1, voids=voids, salt=salt)         # shared: nobody writes to it


@pytest.mark.parametrize("voids,salt", [(0.0, 0.0), (0.05, 0.01), (0.3, 0.05)])
def test_the_kit_scene(dev, voids, salt):
    for T, Ax, Ay in ((64, 1024, 1024), (8, 64, 32)):
        labels, n = _check(dev, _kit(voids, salt), T, Ax, Ay, (voids, salt, T))
    assert n > 1


def test_the_large_plane_on_the_device(dev):
    """2300 x 2300, q = q0 + 3 c - 2 r exactly: more than 2048^2 cells, so the scan's second level holds more than one block; one
    facet of every cell; the moments near their bound (gw gh < 2^24), all exactly representable, so the plane is exact."""
    from satmvs_amd import dsm
    g, a, b, q0 = 2300, 3, -2, 1000
    r, c = torch.meshgrid(torch.arange(g, device=dev), torch.arange(g, device=dev), indexing="ij")
    z = ((q0 + a * c + b * r).double() / 256.0).float()
    grid = dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, g, g)
    labels, n = dsm.facets(z, grid, tol=0.0, slope_tol=0.0)
    assert n == 1 and labels.is_cuda and labels.dtype == torch.int32 and bool((labels == 1).all())
    core, n = dsm.facets(z, grid, tol=0.0, slope_tol=0.0, connectivity=4, grow=False)
    assert n == 1 and bool((core[1:-1, 1:-1] == 1).all()) and int(core.sum()) == (g - 2) ** 2
    Gx, Gy, planar = dsm.local_planes(z, grid, tol=0.0)
    assert bool((Gx[1:-1, 1:-1] == 8 * a).all()) and bool((Gy[1:-1, 1:-1] == 8 * b).all()) and int(planar.sum()) == (g - 2) ** 2
    t = dsm.facet_planes(labels, 1, z, grid)
    N, cb = g * g, (g - 1) // 2
    assert t["n_cells"].tolist() == [N] and t["sums"].tolist() == [[N * (g - 1) // 2, N * (g - 1) // 2, N * q0 + (a + b) * N * (g - 1) // 2]]
    qb = q0 + (a + b) * cb                                   # the mean lies a half above it
    assert t["centre"].tolist() == [[cb, cb]] and t["centre_q"].tolist() == [qb]
    sxx = g * sum((x - cb) ** 2 for x in range(g))
    moments = [N // 2, N // 2, N // 2, sxx, N // 4, sxx, a * sxx + b * (N // 4), a * (N // 4) + b * sxx]
    assert t["moments"].tolist() == [moments] and max(moments) > 2 ** 42
    want = fo.fit(N, moments, qb)                            # the products of the fit pass 2^53: the header's order decides the last bit
    assert t["plane"].tolist() == [list(want)] and max(abs(want[0] - a), abs(want[1] - b), abs(want[2] - qb)) < 1e-9
    assert t["sse"].tolist() == [0] and t["max_abs"].tolist() == [0] and t["rms_m"].tolist() == [0.0]
    assert t["dzde"].tolist() == [want[0] / 1280.0] and t["dzdn"].tolist() == [-want[1] / 1280.0] and t["area_m2"].tolist() == [25.0 * N]


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [None, 1])
def test_the_roof_scene(dev, seed):
    from satmvs_amd import dsm
    z, faces = fs.roof_scene(seed)
    grid = dsm.DSMGrid(500000.0, 3400000.0, fs.RES, fs.RES, z.shape[1], z.shape[0])
    for tol, slope_tol in ((0.25, 0.1), (0.5, 0.2)):
        T, Ax, Ay = dsm.facet_terms(grid, tol, slope_tol)
        want, nw = fo.facets(z, T, Ax, Ay)
        labels, n = dsm.facets(z, grid, tol, slope_tol)
        assert isinstance(labels, np.ndarray) and labels.dtype == np.int32 and isinstance(n, int)
        assert n == nw and fo.differing(labels, want) is None
        fs.check_roof_answer(labels, n, faces)
    _check(dev, z, T, Ax, Ay, ("roofs", seed))
    t = dsm.facet_planes(labels, n, z, grid)
    w = fo.planes(want, nw, z)
    for key, ref in (("n_cells", w["sums"][:, 0]), ("sums", w["sums"][:, 1:]), ("centre", w["centre"][:, [1, 0]]), ("centre_q", w["centre"][:, 2]),
                     ("moments", w["moments"]), ("plane", w["plane"]), ("sse", w["sse"]), ("max_abs", w["max_abs"])):
        assert fo.differing(t[key], ref) is None, (key, fo.differing(t[key], ref))
    shed = int(labels[faces["shed"]][0]) - 1
    flat = int(labels[faces["flat"]][0]) - 1
    north = int(labels[faces["gable_a_north"]][0]) - 1
    assert abs(t["dzde"][shed] - 0.3) < 0.01 and abs(t["aspect_deg"][shed] - 270.0) < 2.0 and abs(t["slope_deg"][shed] - 16.7) < 0.5
    assert t["slope_deg"][flat] < 0.5 and t["area_m2"][flat] == 140 * 25.0 and abs(t["mean_m"][flat] - (fs.ROOF_BASE + 3.0)) < 0.05
    assert abs(t["aspect_deg"][north] - 0.0) < 2.0 or abs(t["aspect_deg"][north] - 360.0) < 2.0         # it falls towards the north
    assert abs(t["surface_m2"][north] / t["area_m2"][north] - np.sqrt(1.16)) < 0.01 and (t["rms_m"][[shed, flat, north]] < 0.1).all()


def test_ties_at_the_thresholds(dev):
    """Heights drawn from 12 values T / 2 apart: residuals sit on 8 T and gradient differences on Ax, Ay again and again."""
    for T, Ax, Ay in ((8, 16, 24), (4, 32, 32), (0, 0, 0)):
        _check(dev, fs.twelve_values(130, 150, seed=T + 3, T=max(T, 2)), T, Ax, Ay, ("twelve", T))
    flat = np.full((70, 90), 12.5, np.float32)
    labels, n = _check(dev, flat, 0, 0, 0, "T = 0, Ax = Ay = 0")
    z = fs.quantised_plane(70, 90)
    z[::7, ::5] += np.float32(1.0 / 256.0)                   # one unit off the plane
    for T in (0, 1):
        _check(dev, z, T, 0, 0, ("one unit off", T))


def test_the_serpentine(dev):
    z = fs.serpentine(257, 301)
    labels, n = _check(dev, z, 0, 0, 0, "serpentine")
    full, n = _native_label(torch.from_numpy(z).to(dev), None, 0, 0, 0, 4, 1)
    assert n == 1 and np.array_equal(full > 0, z != ND)      # one facet through every band, and growth gives back every rim


def test_the_checkerboard_has_no_link(dev):
    for T in (0, 5):
        labels, n = _check(dev, fs.checkerboard(130, 150, T), T, 2 ** 26, 2 ** 26, ("checkerboard", T))
        assert n == 0 and not labels.any()


def test_special_values(dev):
    for T in (0, 1, 2):
        _check(dev, fs.special_values(131, 149, seed=6), T, 4, 4, ("special", T))
    z = fs.special_values(131, 149, seed=8)
    zd = torch.from_numpy(z).to(dev)
    for nodata in (float("nan"), 0.0):                       # through the Python layer: another nodata
        from satmvs_amd import dsm
        grid = dsm.DSMGrid(0.0, 0.0, 1.0, 1.0, 149, 131)
        T, Ax, Ay = dsm.facet_terms(grid, 2.0 / 256.0, 4.0 / 2048.0)
        got, n = dsm.facets(zd, grid, 2.0 / 256.0, 4.0 / 2048.0, nodata=nodata)
        want, nw = fo.facets(z, T, Ax, Ay, nodata=nodata)
        assert (T, Ax, Ay) == (2, 4, 4) and n == nw and fo.differing(got.cpu().numpy(), want) is None


# ---- the entries keep to themselves --------------------------------------------------------------------------------------------------
def test_any_workspace_will_do_and_runs_repeat(dev):
    z = _kit(0.05, 0.01)
    zd = torch.from_numpy(z).to(dev)
    want, nw = fo.facets(z, 64, 1024, 1024)
    for fill in (0xff, 0x00, 0x5a):
        got, n = _native_label(zd, None, 64, 1024, 1024, 8, 1, fill=fill)
        assert n == nw and fo.differing(got, want) is None, fill
    small = torch.from_numpy(np.ascontiguousarray(z[:50, :70])).to(dev)      # a smaller call after a larger one
    got, n = _native_label(small, None, 64, 1024, 1024, 8, 1)
    want_s, nw_s = fo.facets(z[:50, :70], 64, 1024, 1024)
    assert n == nw_s and fo.differing(got, want_s) is None
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    from satmvs_amd import dsm
    grid = dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, 301, 257)
    keep = zd.clone()
    with torch.cuda.stream(side):
        a, na = dsm.facets(zd, grid)
        ta = dsm.facet_planes(a, na, zd, grid)
    side.synchronize()
    b, nb = dsm.facets(zd, grid)
    tb = dsm.facet_planes(b, nb, zd, grid)
    assert a.is_cuda and na == nb == nw and torch.equal(a, b) and torch.equal(zd.view(torch.int32), keep.view(torch.int32)) and fo.differing(a.cpu().numpy(), want) is None
    for k in ta:
        assert ta[k].is_cuda and fo.differing(ta[k].cpu().numpy(), tb[k].cpu().numpy()) is None, k
    fo.same_planes(_native_planes(a, zd, na), fo.planes(want, nw, z), "kit planes")


def test_planes_of_arbitrary_labels(dev):
    """Labels that no labelling gives: outside 1 .. n, on invalid cells, collinear sets (NaN planes), a label without a cell."""
    gh, gw = 130, 150
    z = _kit(0.0, 0.0)[:gh, :gw].copy()
    labels = np.random.default_rng(3).integers(-2, 9, (gh, gw)).astype(np.int32)
    labels[labels == 5] = 0
    labels[3, 10:90], labels[20:120, 7] = 10, 11
    d = np.arange(60)
    labels[30 + d, 40 + d], labels[100 - d, 80 + d] = 12, 13
    labels[0, 0], labels[-1, -1] = -2 ** 31, 2 ** 31 - 1
    zd, ld = torch.from_numpy(z).to(dev), torch.from_numpy(labels).to(dev)
    for n in (14, 9, 3):
        want = fo.planes(labels, n, z)
        fo.same_planes(_native_planes(ld, zd, n), want, n)
    assert np.isnan(want["plane"]).sum() == 0 and np.isnan(fo.planes(labels, 14, z)["plane"][:, 0]).nonzero()[0].tolist() == [4, 8, 9, 10, 11, 12, 13]
    from satmvs_amd import dsm
    empty = dsm.facet_planes(labels, 0, z, dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, gw, gh))
    assert empty["plane"].shape == (0, 3) and empty["n_cells"].shape == (0,) and empty["slope_deg"].shape == (0,)


def test_rejections_write_nothing(dev, lib):
    fs.check_c_rejections(lib)
    from satmvs_amd import _lib
    gh, gw = 40, 70
    zd = torch.from_numpy(fs.kit(gh, gw, seed=1)).to(dev)
    nbytes = lib.smvs_dsm_facet_workspace_bytes(gw, gh)
    out, n_out, ws = _guarded(gh * gw, torch.int32, dev), _guarded(1, torch.int32, dev), _guarded(nbytes, torch.uint8, dev)
    for T, Ax, conn, grow, nb in ((-1, 5, 8, 1, nbytes), (5, -1, 8, 1, nbytes), (5, 5, 6, 1, nbytes), (5, 5, 8, 2, nbytes), (5, 5, 8, 1, nbytes - 1)):
        with pytest.raises(_lib.SatMVSNativeError):
            _lib.call("smvs_dsm_facet_label", _lib.ptr(zd), None, gw, gh, -999.0, T, Ax, 5, conn, grow, _lib.ptr(out[G:]), _lib.ptr(n_out[G:]),
                      _lib.ptr(ws[G:]), nb, _lib.current_stream(dev))
    with pytest.raises(_lib.SatMVSNativeError, match="aliases"):
        _lib.call("smvs_dsm_facet_label", _lib.ptr(zd), None, gw, gh, -999.0, 5, 5, 5, 8, 1, _lib.ptr(out[G:]), _lib.ptr(out[G + 5:]),
                  _lib.ptr(ws[G:]), nbytes, _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert bool((out == 77).all()) and bool((n_out == 77).all()) and bool((ws == 77).all())


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_roofs_end_to_end(dev, tmp_path):
    """extract_dtm -> ndsm -> extract_roofs -> outlines -> write_geojson, read back with json; label_stats(values=sun_exposure)
    per facet.  On device tensors throughout, then numpy in, numpy out."""
    from satmvs_amd import dsm
    z, faces = fs.roof_scene(seed=1)
    gh, gw = z.shape
    grid = dsm.DSMGrid(500000.0, 3400000.0, fs.RES, fs.RES, gw, gh)
    zd = torch.from_numpy(z).to(dev)
    above = dsm.ndsm(zd, dsm.extract_dtm(zd, grid))
    labels, table = dsm.extract_roofs(zd, above, grid)
    assert labels.is_cuda and labels.dtype == torch.int32 and all(t.is_cuda for t in table.values())
    n = len(table["n_cells"])
    got = labels.cpu().numpy()
    assert n >= 10 and got.max() == n and (table["object"] > 0).all() and (table["area_m2"] >= 25.0).all()
    for name in ("flat", "shed", "gable_a_north", "gable_a_south", "gable_b_north", "gable_b_south"):
        ks = np.unique(got[faces[name]])
        assert len(ks) == 1 and ks[0] > 0 and np.array_equal(got == ks[0], faces[name]), name          # each face cell for cell
    objects, _ = dsm.extract_objects(above, grid)
    first = [int(np.flatnonzero(got.ravel() == k + 1)[0]) for k in range(n)]
    assert np.array_equal(table["object"].cpu().numpy(), objects.cpu().numpy().ravel()[first])
    strict, strict_table = dsm.extract_roofs(zd, above, grid, max_rms=0.01, facet_min_area_m2=500.0)
    assert len(strict_table["n_cells"]) < n and (strict_table["rms_m"] <= 0.01).all() and (strict_table["area_m2"] >= 500.0).all()
    rings = dsm.outlines(labels, n, grid)
    table["nothing"] = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    path = tmp_path / "roofs.geojson"
    assert dsm.write_geojson(str(path), rings, grid, table) == n
    doc = json.loads(path.read_text())
    assert len(doc["features"]) == n
    for f in doc["features"]:
        k = f["properties"]["label"] - 1
        assert f["properties"]["nothing"] is None and f["properties"]["n_cells"] == int(table["n_cells"][k])
        assert f["properties"]["plane"] == table["plane"][k].tolist() and f["properties"]["object"] == int(table["object"][k])
        assert f["geometry"]["type"] == "Polygon" and len(f["geometry"]["coordinates"][0]) >= 5
    suns = [(135.0, 30.0), (180.0, 45.0), (225.0, 30.0)]
    per_facet = dsm.label_stats(labels, n, values=dsm.sun_exposure(zd, grid, suns), grid=grid)
    south, north = int(got[faces["gable_a_south"]][0]) - 1, int(got[faces["gable_a_north"]][0]) - 1
    assert per_facet["mean"].shape == (n,) and float(per_facet["mean"][south]) > float(per_facet["mean"][north])
    labels_np, table_np = dsm.extract_roofs(z, above.cpu().numpy(), grid)
    assert isinstance(labels_np, np.ndarray) and np.array_equal(labels_np, got)
    for k, t in table_np.items():
        assert isinstance(t, np.ndarray) and fo.differing(t, table[k].cpu().numpy()) is None, k
