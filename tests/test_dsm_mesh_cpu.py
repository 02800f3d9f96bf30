"""The rule of the DSM meshes without a device: the oracle's two statements against each other, the invariants the rule promises
each against an independent count, closed forms, the PLY and OBJ writers read back, every argument rejection that needs no
device, and planted errors that the GPU file's comparison must report."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import dsm_mesh_oracle as mo
from dsm_testkit import lib                                  # noqa: F401


def _surface(kind, gh, gw, seed, voids):
    if kind == "plane":
        z = mo.quantised_plane(gh, gw)
    elif kind == "noise":
        z = mo.noise(gh, gw, seed, hi=600)
    else:
        z = mo.scene(gh, gw, seed, voids=0.0, salt=0.04)
    rng = np.random.default_rng(seed + 1)
    gone = rng.random((gh, gw)) < voids
    z[gone] = np.where(rng.random((gh, gw)) < 0.5, np.float32(np.nan), np.float32(-999.0))[gone]
    return z


MATRIX = [(gh, gw, S, kind, voids) for (gh, gw), S in (((9, 9), 4), ((12, 12), 4), ((20, 27), 4), ((17, 17), 8), ((13, 22), 8), ((33, 33), 16),
                                                       ((16, 18), 16), ((7, 5), 2), ((1, 6), 4), ((5, 1), 2))
          for kind, voids in (("plane", 0.0), ("hill", 0.0), ("hill", 0.05), ("noise", 0.1))]
TOLS = (0.0, 1 / 256.0, 0.25, 1.0, 1e9)
_ref = {}


def _reference(case):
    """z, the error map and the recursion's meshes of a case, computed once and left alone."""
    if case not in _ref:
        gh, gw, S, kind, voids = case
        z = _surface(kind, gh, gw, gh * gw + S, voids)
        e = mo.errors_recursive(z, S)
        _ref[case] = (z, e, {tol: mo.mesh_recursive(e, z, S, tol) for tol in TOLS})
    return _ref[case]


def _id(case):
    return "%dx%d-S%d-%s-%d%%" % (case[0], case[1], case[2], case[3], round(100 * case[4]))


def _area2(m):
    c = mo.corners(m)
    a, b, cc = c[:, 0], c[:, 1], c[:, 2]
    return np.abs((b[:, 1] - a[:, 1]) * (cc[:, 0] - a[:, 0]) - (b[:, 0] - a[:, 0]) * (cc[:, 1] - a[:, 1]))


# ---- the two statements ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MATRIX, ids=_id)
def test_the_two_statements_agree(case):
    z, e, meshes = _reference(case)
    S = case[2]
    assert np.array_equal(mo.errors_arrays(z, S), e)
    for tol in TOLS:
        assert mo.differing(mo.mesh_arrays(e, z, S, tol), meshes[tol]) == []
        h1, d1 = mo.heights_recursive(e, z, S, tol)          # asserts that all triangles agree at a shared vertex
        h2, d2 = mo.heights_arrays(e, z, S, tol)
        assert np.array_equal(h1.view(np.uint32), h2.view(np.uint32)) and np.array_equal(d1, d2)


@pytest.mark.parametrize("case", MATRIX, ids=_id)
def test_the_local_rule_is_the_top_down_descent(case):
    z, e, _ = _reference(case)
    S = case[2]
    for tol in TOLS:
        # a triangle as (the two ends of its hypotenuse in either order, apex, level)
        local = [(frozenset({tuple(row[0:2]), tuple(row[2:4])}), tuple(row[4:6]), row[6]) for row in mo.emitted_arrays(e, z, S, tol).tolist()]
        descent = [(frozenset({T.a, T.b}), T.c, T.level) for T in mo.emitted_recursive(e, z, S, tol)]
        assert len(set(local)) == len(local) and len(set(descent)) == len(descent) and set(local) == set(descent)


# ---- invariants --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MATRIX, ids=_id)
def test_invariants_of_the_mesh(case):
    z, e, meshes = _reference(case)
    gh, gw, S = case[:3]
    Q, V = mo.padded(z, -999.0, S)
    last = None
    for tol in TOLS:
        m = meshes[tol]
        c = mo.corners(m)
        # no vertex of the mesh strictly inside an edge of the mesh: an edge is straight or diagonal, so its inner lattice
        # points are the steps between its ends
        used = {tuple(p) for p in m["vertices"][:, ::-1].tolist()}
        for tri in c.tolist():
            for (r0, c0), (r1, c1) in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
                n = max(abs(r1 - r0), abs(c1 - c0))
                assert abs(r1 - r0) in (0, n) and abs(c1 - c0) in (0, n)
                for k in range(1, n):
                    assert (r0 + (r1 - r0) * k // n, c0 + (c1 - c0) * k // n) not in used
        # the twice-areas sum to the finest half-cells with three valid corners
        assert int(_area2(m).sum()) == mo.full_resolution_count(z)
        # every triangle's brute-force error is within the threshold, in exact integers
        units, thr = mo.threshold(tol, S)
        for tri, level in zip(c.tolist(), m["tri_level"].tolist()):
            assert mo.exact_error(mo.Tri(tuple(tri[0]), tuple(tri[1]), tuple(tri[2]), level), Q, V, S) <= thr
        # counter-clockwise in map coordinates (x = col, y = -row)
        a, b, cc = c[:, 0], c[:, 1], c[:, 2]
        assert ((b[:, 1] - a[:, 1]) * (a[:, 0] - cc[:, 0]) - (a[:, 0] - b[:, 0]) * (cc[:, 1] - a[:, 1]) > 0).all()
        # hypotenuse a - b, right angle at c
        assert (((a - cc) * (b - cc)).sum(axis=1) == 0).all() and (((a - cc) ** 2).sum(axis=1) == ((b - cc) ** 2).sum(axis=1)).all()
        # the order key is unique and rising
        key = [tuple(k) for k in m["key"].tolist()]
        assert key == sorted(set(key))
        assert np.array_equal(m["key"][:, :2], a + b)
        # vertices in row-major order, heights by their bits
        flat = m["vertices"][:, 1].astype(np.int64) * gw + m["vertices"][:, 0]
        assert (np.diff(flat) > 0).all() and np.array_equal(m["z"].view(np.uint32), z.reshape(-1)[flat].view(np.uint32))
        # raising tol never adds a triangle: the meshes over one error map are nested
        assert last is None or len(m["triangles"]) <= last
        last = len(m["triangles"])


def test_the_error_bound_in_fractions():
    """Every lattice vertex in an emitted triangle within floor(256 tol) quanta of the plane, with Fraction barycentric weights
    from the corners' coordinates: no shared code with the oracle's integer plane."""
    case = (20, 27, 4, "hill", 0.05)
    z, e, meshes = _reference(case)
    q, ok = mo.quantum(z)
    for tol in (0.25, 1.0):
        units = int(np.floor(256 * tol))
        seen = 0
        for (a, b, c), level in zip(mo.corners(meshes[tol]).tolist(), meshes[tol]["tri_level"].tolist()):
            det = (b[0] - c[0]) * (a[1] - c[1]) - (a[0] - c[0]) * (b[1] - c[1])
            for r in range(min(a[0], b[0], c[0]), max(a[0], b[0], c[0]) + 1):
                for cc in range(min(a[1], b[1], c[1]), max(a[1], b[1], c[1]) + 1):
                    wa = Fraction((b[0] - c[0]) * (cc - c[1]) - (r - c[0]) * (b[1] - c[1]), det)
                    wb = Fraction((r - c[0]) * (a[1] - c[1]) - (a[0] - c[0]) * (cc - c[1]), det)
                    wc = 1 - wa - wb
                    if min(wa, wb, wc) < 0:
                        continue
                    assert ok[r, cc]
                    plane = wa * int(q[a[0], a[1]]) + wb * int(q[b[0], b[1]]) + wc * int(q[c[0], c[1]])
                    assert abs(int(q[r, cc]) - plane) <= units
                    seen += 1
        assert seen >= int(ok.sum()) - 40


# ---- closed forms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (2, 4, 16))
def test_a_quantised_plane_gives_its_root_triangles(S):
    for squares in (1, 2):
        n = squares * S + 1
        m = mo.mesh(mo.quantised_plane(n, n), S, 0.0)
        assert len(m["triangles"]) == 2 * squares ** 2 and (m["tri_level"] == 0).all() and len(m["vertices"]) == (squares + 1) ** 2
        assert int(mo.errors_arrays(mo.quantised_plane(n, n), S).max()) == 0


def test_one_raised_cell_in_a_plane():
    """9 x 9 at tile 8, the vertex (3, 5) raised by 40 quanta.  At tol 0 every triangle that holds (3, 5) inside or on its rim
    errs, so the mesh refines down to (3, 5) as a vertex and nowhere deeper than conformity asks; the vertex is in the mesh, its
    height exact.  At a tolerance of 40 quanta nothing errs by more: the two root triangles."""
    z = mo.quantised_plane(9, 9)
    z[3, 5] += np.float32(40 / 256.0)
    e = mo.errors_arrays(z, 8)
    assert np.array_equal(e, mo.errors_recursive(z, 8))
    m = mo.mesh_arrays(e, z, 8, 0.0)
    assert mo.differing(m, mo.mesh_recursive(e, z, 8, 0.0)) == []
    assert [5, 3] in m["vertices"].tolist() and 2 < len(m["triangles"]) < mo.full_resolution_count(z)
    h, d = mo.heights_arrays(e, z, 8, 0.0)
    assert (d == 0).all() and np.array_equal(h.view(np.uint32), z.view(np.uint32))
    assert len(mo.mesh_arrays(e, z, 8, 40 / 256.0)["triangles"]) == 2 and len(mo.mesh_arrays(e, z, 8, 39 / 256.0)["triangles"]) > 2
    assert e.max() == 40 * 8                                 # the deviation at the vertex itself, weight 1, in units of 1 / S


def test_one_void_in_a_plane():
    """The finest diagonals run from the centre of every 2 x 2 square, an (odd, odd) vertex, to its corners, (even, even)
    vertices.  A void at a vertex with row + col even is therefore the end of the diagonals of all four cells round it: the
    hole is exactly their 8 half-cells.  With row + col odd all four diagonals pass the vertex by and only the 4 half-cells with
    their right angle there are lost.  Nothing else goes: at any tolerance the rim of the hole is refined down to single cells."""
    for at, lost in (((3, 5), 8), ((2, 6), 8), ((4, 3), 4), ((5, 2), 4)):
        z = mo.quantised_plane(9, 9)
        z[at] = np.nan
        m = mo.mesh(z, 8, 1e9)
        assert int(_area2(m).sum()) == 2 * 8 * 8 - lost == mo.full_resolution_count(z)
        assert list(at)[::-1] not in m["vertices"].tolist()
        assert mo.differing(m, mo.mesh_recursive(mo.errors_recursive(z, 8), z, 8, 1e9)) == []
        # the hole's rim is made of single half-cells: its corners, the 8 or the 4 nearest neighbours, are mesh vertices
        near = {(at[1] + dc, at[0] + dr) for dr in (-1, 0, 1) for dc in (-1, 0, 1) if 0 < abs(dr) + abs(dc) <= (2 if lost == 8 else 1)}
        assert near <= {tuple(v) for v in m["vertices"].tolist()}


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1)])
def test_grids_without_a_cell_give_an_empty_mesh(shape):
    z = mo.noise(*shape, seed=1)
    for S in (2, 8):
        m = mo.mesh(z, S, 0.0)
        assert m["triangles"].shape == (0, 3) and m["vertices"].shape == (0, 2) and m["z"].shape == (0,) and m["tri_level"].shape == (0,)
        assert mo.differing(m, mo.mesh_recursive(mo.errors_recursive(z, S), z, S, 0.0)) == []
        assert (mo.heights_arrays(mo.errors_arrays(z, S), z, S, 0.0)[0] == np.float32(-999.0)).all()


def test_tol_0_on_noise_gives_the_full_resolution():
    z = mo.noise(12, 12, seed=4)
    m = mo.mesh(z, 4, 0.0)
    assert len(m["triangles"]) == 2 * 11 * 11 == 242 and (m["tri_level"] == 4).all() and len(m["vertices"]) == 144
    z = mo.noise(33, 33, seed=4)
    assert len(mo.mesh(z, 16, 1e9)["triangles"]) == 8


# ---- writers -----------------------------------------------------------------------------------------------------------------------
def _mesh_and_grid():
    from satmvs_amd import dsm
    z = mo.scene(20, 27, seed=3, voids=0.03)
    m = mo.mesh(z, 8, 0.5)
    m.update(tile=8, tol_units=128)
    return z, m, dsm.DSMGrid(400000.0, 3500000.0, mo.XRES, mo.YRES, 27, 20)


def test_write_ply_read_back(tmp_path):
    from satmvs_amd import dsm
    z, m, grid = _mesh_and_grid()
    colours = np.random.default_rng(1).integers(0, 256, (20, 27, 3)).astype(np.uint8)
    for with_colours in (False, True):
        path = str(tmp_path / "m.ply")
        assert dsm.write_ply(path, m, grid, colors=colours if with_colours else None) == len(m["triangles"])
        with open(path, "rb") as fh:
            head, body = fh.read().split(b"end_header\n", 1)
        lines = head.decode("ascii").splitlines()
        assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
        nv, nt = (int([ln for ln in lines if ln.startswith("element " + k)][0].split()[2]) for k in ("vertex", "face"))
        props = [ln.split()[1:] for ln in lines if ln.startswith("property")]
        assert props[:3] == [["double", "x"], ["double", "y"], ["double", "z"]] and props[-1] == ["list", "uchar", "int", "vertex_indices"]
        assert (len(props) == 7) == with_colours and (nv, nt) == (len(m["vertices"]), len(m["triangles"]))
        fields = [("p", "<f8", (3,))] + ([("rgb", "u1", (3,))] if with_colours else [])
        rec = np.frombuffer(body, dtype=fields, count=nv)
        faces = np.frombuffer(body, dtype=[("n", "u1"), ("v", "<i4", (3,))], count=nt, offset=rec.nbytes)
        assert len(body) == rec.nbytes + nt * 13 and (faces["n"] == 3).all()
        assert np.array_equal(faces["v"], m["triangles"]) and faces["v"].min() >= 0 and faces["v"].max() < nv
        col, row = m["vertices"][:, 0], m["vertices"][:, 1]
        assert np.array_equal(rec["p"][:, 0], 400000.0 + col * mo.XRES) and np.array_equal(rec["p"][:, 1], 3500000.0 - row * mo.YRES)
        assert np.array_equal(rec["p"][:, 2], z[row, col].astype(np.float64))
        if with_colours:
            assert np.array_equal(rec["rgb"], colours[row, col])


def test_write_obj_read_back(tmp_path):
    from satmvs_amd import dsm
    z, m, grid = _mesh_and_grid()
    for tex in (False, True):
        path = str(tmp_path / "m.obj")
        assert dsm.write_obj(path, m, grid, texcoords=tex) == len(m["triangles"])
        with open(path) as fh:
            rows = [ln.split() for ln in fh if not ln.startswith("#")]
        v = np.array([[float(x) for x in r[1:]] for r in rows if r[0] == "v"])
        vt = np.array([[float(x) for x in r[1:]] for r in rows if r[0] == "vt"]).reshape(-1, 2)
        f = [r[1:] for r in rows if r[0] == "f"]
        col, row = m["vertices"][:, 0], m["vertices"][:, 1]
        assert np.array_equal(v, np.stack([400000.0 + col * mo.XRES, 3500000.0 - row * mo.YRES, z[row, col].astype(np.float64)], axis=1))
        assert len(vt) == (len(v) if tex else 0) and len(f) == len(m["triangles"])
        if tex:
            assert np.array_equal(vt, np.stack([col / 26, 1.0 - row / 19], axis=1))
            assert all(part.split("/")[0] == part.split("/")[1] for face in f for part in face)
        index = np.array([[int(part.split("/")[0]) for part in face] for face in f])
        assert np.array_equal(index - 1, m["triangles"]) and index.min() >= 1 and index.max() <= len(v)


def test_writers_reject_what_is_no_mesh(tmp_path):
    from satmvs_amd import dsm
    z, m, grid = _mesh_and_grid()
    path = str(tmp_path / "x.ply")
    with pytest.raises(ValueError, match="entry 'z' is missing"):
        dsm.write_ply(path, {k: v for k, v in m.items() if k != "z"}, grid)
    with pytest.raises(ValueError, match="index outside"):
        dsm.write_obj(path, dict(m, triangles=m["triangles"] + 1000), grid)
    with pytest.raises(ValueError, match="outside the grid"):
        dsm.write_ply(path, m, dsm.DSMGrid(0.0, 0.0, 1.0, 1.0, 5, 5))
    with pytest.raises(ValueError, match="colors is a uint8"):
        dsm.write_ply(path, m, grid, colors=np.zeros((20, 27, 3), np.float32))
    with pytest.raises(ValueError, match="colors is a uint8"):
        dsm.write_ply(path, m, grid, colors=np.zeros((27, 20, 3), np.uint8))


# ---- rejections --------------------------------------------------------------------------------------------------------------------
def test_python_rejections_need_no_device():
    from satmvs_amd import dsm
    z = mo.noise(9, 9, seed=1)
    e = np.zeros((9, 9), np.int64)
    for call in (lambda **kw: dsm.mesh(z, **kw), lambda **kw: dsm.mesh_heights(z, kw.pop("tol", 0.5), **kw), lambda **kw: dsm.mesh_errors(z, **kw)):
        for tile in (0, 1, 3, 48, 2048, -4, 4.0, True, "8"):
            with pytest.raises(ValueError, match="tile must be"):
                call(tile=tile)
    for call in (lambda **kw: dsm.mesh(z, **kw), lambda **kw: dsm.mesh_heights(z, kw.pop("tol"), **kw)):
        for tol in (-1e-9, float("nan"), float("inf"), None, "1", True):
            with pytest.raises(ValueError, match="tol is a finite number"):
                call(tol=tol)
        with pytest.raises(ValueError, match="errors is int64"):
            call(tol=0.5, errors=e.astype(np.int32))
        with pytest.raises(ValueError, match="errors shape"):
            call(tol=0.5, errors=e[:8])
        with pytest.raises(ValueError, match="both be numpy arrays or both be tensors"):
            import torch
            call(tol=0.5, errors=torch.zeros((9, 9), dtype=torch.int64))
    for bad in (z.astype(np.float64), z[0], np.zeros((0, 4), np.float32)):
        with pytest.raises(ValueError, match="a DSM"):
            dsm.mesh(bad)
        with pytest.raises(ValueError, match="a DSM"):
            dsm.mesh_errors(bad)
    with pytest.raises(ValueError, match="fewer than 2\\^29 cells"):
        dsm.mesh_errors(np.broadcast_to(np.float32(0), (1 << 15, 1 << 14)))
    with pytest.raises(ValueError, match="differs from the grid"):
        dsm.mesh(z, dsm.DSMGrid(0.0, 0.0, 1.0, 1.0, 9, 8))


def test_native_rejections_need_no_device(lib):              # noqa: F811
    """Every SMVS_ERR_ARG of the four entries comes before any HIP call: made-up pointers, no device."""
    from satmvs_amd import _lib
    MB = 1 << 20
    at = lambda i: C.c_void_p(i * MB)                        # noqa: E731
    gw, gh, S = 9, 7, 4
    n = gw * gh
    nbytes = lib.smvs_dsm_mesh_workspace_bytes(gw, gh, S)
    assert 0 < nbytes < MB and nbytes >= 14 * n
    null = C.c_void_p(0)

    def errors(dsm=at(1), gw=gw, gh=gh, tile=S, errors=at(2)):
        _lib.call("smvs_dsm_mesh_errors", dsm, gw, gh, -999.0, tile, errors, None)

    def count(errors=at(2), dsm=at(1), gw=gw, gh=gh, tile=S, thr=0, counts=at(3), ws=at(11), nbytes=nbytes):
        _lib.call("smvs_dsm_mesh_count", errors, dsm, gw, gh, -999.0, tile, thr, counts, ws, nbytes, None)

    def write(dsm=at(1), gw=gw, gh=gh, tile=S, nt=5, nv=5, tri=at(4), lev=at(5), ver=at(6), z=at(7), status=at(8), ws=at(11), nbytes=nbytes):
        _lib.call("smvs_dsm_mesh_write", dsm, gw, gh, tile, nt, nv, tri, lev, ver, z, status, ws, nbytes, None)

    def heights(errors=at(2), dsm=at(1), gw=gw, gh=gh, tile=S, thr=0, h=at(9), d=at(10), ws=at(11), nbytes=nbytes):
        _lib.call("smvs_dsm_mesh_heights", errors, dsm, gw, gh, -999.0, tile, thr, h, d, ws, nbytes, None)

    def rejected(call, match, **kw):
        with pytest.raises(_lib.SatMVSNativeError, match=match):
            call(**kw)

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
            rejected(call, "workspace aliases dsm", ws=C.c_void_p(MB + 4 * n - 1))
    rejected(errors, "errors aliases dsm", errors=C.c_void_p(MB + 4 * n - 1))
    rejected(count, "dsm aliases errors", dsm=C.c_void_p(2 * MB + 8 * n - 1))
    rejected(count, "counts aliases errors", counts=C.c_void_p(2 * MB + 8))
    rejected(count, "threshold", thr=-1)
    rejected(heights, "threshold", thr=-1)
    rejected(heights, "heights aliases dsm", h=at(1))
    rejected(heights, "dev aliases heights", d=C.c_void_p(9 * MB + 4 * n - 1))
    rejected(write, "negative counts", nt=-1)
    rejected(write, "negative counts", nv=-1)
    rejected(write, "than the grid holds", nt=2 * n + 1)
    rejected(write, "than the grid holds", nv=n + 1)
    rejected(write, "tri_level aliases triangles", lev=C.c_void_p(4 * MB + 59))
    rejected(write, "status aliases z", status=C.c_void_p(7 * MB + 16))
    assert lib.smvs_dsm_mesh_workspace_bytes(0, 5, 4) == 0 and lib.smvs_dsm_mesh_workspace_bytes(5, 5, 3) == 0
    assert lib.smvs_dsm_mesh_workspace_bytes(1 << 15, 1 << 14, 4) == 0 and lib.smvs_dsm_mesh_workspace_bytes(5, 5, 2048) == 0


# ---- planted errors ----------------------------------------------------------------------------------------------------------------
def _planted_case(variant):
    """A grid and a tolerance on which the planted error shows."""
    if variant == "ge":                                      # an error exactly on the threshold: the centre raised by 2 quanta
        z = np.zeros((5, 5), np.float32)
        z[2, 2] = 2 / 256.0
        return z, 4, 2 / 256.0
    if variant == "voids":
        z = mo.quantised_plane(17, 17)
        z[5, 9] = np.nan
        return z, 8, 1.0
    if variant == "side":
        return mo.noise(9, 9, seed=2), 4, 0.0
    if variant == "midpoint":                                # a cliff of 250 quanta beside column 0: every hypotenuse that crosses it has
        z = np.full((17, 17), 250 / 256.0, np.float32)       # one end below and its midpoint above, 125 from the mean of its ends, under
        z[:, 0] = 0.0                                        # the 128 of the tolerance; the root's plane at (1, 1) is 234 below the ground
        return z, 16, 0.5
    return mo.scene(33, 33, seed=9, voids=0.0, salt=0.05), 16, 0.5


@pytest.mark.parametrize("variant", mo.VARIANTS)
def test_planted_errors_are_reported(variant):
    """The comparison of the GPU file, mo.differing, reports each planted error and names the first differing triangle."""
    z, S, tol = _planted_case(variant)
    want = mo.mesh(z, S, tol)
    assert mo.differing(mo.mesh(z, S, tol), want) == []
    report = mo.differing(mo.mesh(z, S, tol, variant=variant), want)
    assert report and report[0].startswith("first differing triangle ") and "got" in report[0] and "want" in report[0]
    if variant != "side":
        assert not np.array_equal(mo.errors_arrays(z, S, variant=variant), mo.errors_arrays(z, S)) or variant == "ge"
