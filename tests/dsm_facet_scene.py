"""The cases of the facet tests (CPU and GPU share them) and the roof scene with its known answer.  numpy only."""
import ctypes as C

import numpy as np

from dsm_testkit import scene as kit_scene

ND = np.float32(-999.0)
RES = 5.0
ROOF_SHAPE = (96, 128)
# name -> (top row, left column, rows, columns)
ROOFS = {"gable_a": (10, 12, 8, 12), "gable_b": (14, 40, 6, 10), "flat": (40, 16, 10, 14), "shed": (44, 60, 10, 10), "pyramid": (70, 90, 12, 12)}
ROOF_BASE = 165.0                                            # eaves: above the terrain's 150 m everywhere


def roof_scene(seed=None):
    """(z (96, 128) float32, faces): terrain 130 + 20 sin(E / 253) cos(N / 171) over cells of 5 m, two gables (8 x 12 cells at
    2.0 m per row, 6 x 10 at 2.5 m per row, the ridge between the middle rows), a flat roof of 10 x 14 cells, a shed roof of 10
    x 10 at 1.5 m per column, a pyramid of 12 x 12 at 2.0 m per cell; with a seed, Gaussian noise of sigma = 0.05 m everywhere.
    faces: name -> bool mask of the six gable, flat and shed faces, and "pyramid" of the whole pyramid."""
    gh, gw = ROOF_SHAPE
    r, c = np.mgrid[0:gh, 0:gw].astype(np.float64)
    z = 130.0 + 20.0 * np.sin(RES * c / 253.0) * np.cos(-RES * r / 171.0)
    faces = {}

    def box(name):
        r0, c0, h, w = ROOFS[name]
        rr, cc = np.mgrid[0:h, 0:w].astype(np.float64)
        return (slice(r0, r0 + h), slice(c0, c0 + w)), rr, cc, h, w

    for name, per_row in (("gable_a", 2.0), ("gable_b", 2.5)):
        where, rr, cc, h, w = box(name)
        z[where] = ROOF_BASE + per_row * np.minimum(rr + 0.5, h - rr - 0.5)
        for side, rows in (("north", slice(0, h // 2)), ("south", slice(h // 2, h))):
            m = np.zeros((gh, gw), bool)
            m[where][rows] = True
            faces[name + "_" + side] = m
    where, rr, cc, h, w = box("flat")
    z[where] = ROOF_BASE + 3.0
    faces["flat"] = np.zeros((gh, gw), bool)
    faces["flat"][where] = True
    where, rr, cc, h, w = box("shed")
    z[where] = ROOF_BASE + 1.5 * (cc + 0.5)
    faces["shed"] = np.zeros((gh, gw), bool)
    faces["shed"][where] = True
    where, rr, cc, h, w = box("pyramid")
    z[where] = ROOF_BASE + 2.0 * np.minimum(np.minimum(rr + 0.5, h - rr - 0.5), np.minimum(cc + 0.5, w - cc - 0.5))
    faces["pyramid"] = np.zeros((gh, gw), bool)
    faces["pyramid"][where] = True
    if seed is not None:
        z = z + np.random.default_rng(seed).normal(0.0, 0.05, z.shape)
    return z.astype(np.float32), faces


def check_roof_answer(labels, n, faces):
    """The end-to-end condition: 11 facets; each of the six gable, flat and shed faces cell for cell under one label that is
    nowhere else; four facets on the pyramid of 34, 31, 31 and 28 cells; the terrain one facet.  The pyramid's hip lines: 124
    of its 144 cells are labelled, so only 20 stay 0 -- the corners and the apex -- and 12 of those are hip cells; a hip cell
    beside a planar cell lies exactly on that face's plane and growth hands it over."""
    assert n == 11, n
    used = set()
    for name, m in faces.items():
        if name == "pyramid":
            continue
        ks = np.unique(labels[m])
        assert len(ks) == 1 and ks[0] > 0, (name, ks.tolist())
        assert np.array_equal(labels == ks[0], m), name
        used.add(int(ks[0]))
    on = labels[faces["pyramid"]]
    ks, counts = np.unique(on[on > 0], return_counts=True)
    assert sorted(counts.tolist(), reverse=True) == [34, 31, 31, 28], counts.tolist()
    for k in ks:
        assert not (labels[~faces["pyramid"]] == k).any()
    used.update(int(k) for k in ks)
    r0, c0, h, w = ROOFS["pyramid"]
    d = np.arange(h)
    hips = np.zeros(labels.shape, bool)
    hips[r0 + d, c0 + d] = hips[r0 + d, c0 + w - 1 - d] = True
    zero = faces["pyramid"] & (labels == 0)                  # 144 - 124 cells: the 2 x 2 corners and the 2 x 2 apex, where no face has a
    assert int(zero.sum()) == 20 and hips[zero].sum() == 12  # planar cell beside them; every other hip cell lies on both planes and is grown
    roofs = np.zeros(labels.shape, bool)
    for m in faces.values():
        roofs |= m
    terrain = np.unique(labels[~roofs & (labels > 0)])
    assert len(terrain) == 1 and int(terrain[0]) not in used and len(used) == 10


def cell_centres(gh, gw, res=RES):
    r, c = np.mgrid[0:gh, 0:gw].astype(np.float64)
    return res * c, -res * r


def kit(gh, gw, seed, voids=0.0, salt=0.0):
    """The test kit's scene over cells of 5 m."""
    E, N = cell_centres(gh, gw)
    return kit_scene(E, N, seed=seed, voids=voids, salt=salt)


def quantised_plane(gh, gw, a=3, b=-2, q0=1000):
    """q = q0 + a c + b r exactly (integers of 2^-8 m): one facet of every cell."""
    r, c = np.mgrid[0:gh, 0:gw]
    return ((q0 + a * c + b * r) / 256.0).astype(np.float32)


def twelve_values(gh, gw, seed, T):
    """Heights drawn from 12 values T / 2 units apart: ties at T abound."""
    rng = np.random.default_rng(seed)
    return ((rng.integers(0, 12, (gh, gw)) * max(T // 2, 1) + 256 * 100) / 256.0).astype(np.float32)


def serpentine(gh, gw):
    """Bands of three valid rows (so that their middle rows are planar) between void rows, all at one height, joined by a
    bridge of three cells at alternating ends: one facet that runs east along the first band, west along the next, ... through
    every fourth row -- a planar cell needs its whole window, so bands cannot be closer.  The deepest tree."""
    z = np.full((gh, gw), ND, np.float32)
    for i, r0 in enumerate(range(0, gh - 2, 4)):
        z[r0:r0 + 3, :] = 100.0
        if r0 + 6 < gh:
            z[r0 + 3, (slice(gw - 3, gw) if i % 2 == 0 else slice(0, 3))] = 100.0
    return z


def checkerboard(gh, gw, T):
    """Steps of +-(T + 1) units between every two 4-neighbours."""
    r, c = np.mgrid[0:gh, 0:gw]
    return ((256 * 50 + ((r + c) % 2) * (T + 1)) / 256.0).astype(np.float32)


def special_values(gh, gw, seed):
    """A gentle plane with cells on quantisation halves, both zeros, NaN, +-Inf, nodata, +-32768 and one ulp beyond."""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:gh, 0:gw]
    z = ((3 * c + 2 * r) / 256.0).astype(np.float32) - np.float32(0.5)
    halves = rng.random((gh, gw)) < 0.3
    z[halves] += np.float32(0.5 / 256.0)                     # q on a half: to even
    picks = [np.float32(0.0), np.float32(-0.0), np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), ND, np.float32(32768.0),
             np.float32(-32768.0), np.nextafter(np.float32(32768.0), np.float32(np.inf)), np.nextafter(np.float32(-32768.0), np.float32(-np.inf)),
             np.float32(0.5 / 256.0), np.float32(-1.5 / 256.0)]
    where = rng.random((gh, gw)) < 0.02
    z[where] = rng.choice(np.array(picks, np.float32), int(where.sum()))
    return z


def random_mask(gh, gw, seed, share=0.7):
    """Blobs: about `share` of the cells inside."""
    rng = np.random.default_rng(seed)
    coarse = rng.random(((gh + 7) // 8, (gw + 7) // 8)) < share
    return np.kron(coarse, np.ones((8, 8), bool))[:gh, :gw].astype(np.uint8)


# The matrix of the CPU tests: (name, z, T, Ax, Ay).  Small, so that the loop statement stays quick.
def matrix():
    cases = []
    z, _ = roof_scene(seed=1)
    cases.append(("roofs", z[:60, :80], 64, 1024, 1024))
    cases.append(("kit", kit(40, 50, seed=3, voids=0.05, salt=0.01), 64, 1024, 1024))
    cases.append(("twelve", twelve_values(33, 47, 5, 8), 8, 16, 24))
    cases.append(("special", special_values(35, 41, 6), 1, 4, 4))
    cases.append(("serpentine", serpentine(30, 37), 0, 0, 0))
    cases.append(("checkerboard", checkerboard(20, 21, 5), 5, 100, 100))
    cases.append(("plane", quantised_plane(19, 23), 0, 0, 0))
    return cases


# ---- the C entries' argument checks (the CPU and the GPU tests both run them) ------------------------------------------------------
def _p(k):
    return C.c_void_p((k + 1) << 24)                         # buffers 16 MB apart: nothing overlaps by accident


def check_c_rejections(lib):
    """Every rejection of the three entries and of the size query; they come before any HIP call, so they show without a device."""
    import pytest
    from satmvs_amd import _lib
    E = _lib.SatMVSNativeError
    gw, gh = 70, 40
    nbytes = lib.smvs_dsm_facet_workspace_bytes(gw, gh)
    assert nbytes >= 17 * gw * gh and lib.smvs_dsm_facet_workspace_bytes(0, 4) == 0 and lib.smvs_dsm_facet_workspace_bytes(4, -1) == 0
    assert lib.smvs_dsm_facet_workspace_bytes(65536, 32768) == 0 and lib.smvs_dsm_facet_workspace_bytes(65536, 32767) > 0

    def normals(dsm=_p(0), mask=_p(1), gw=gw, gh=gh, T=5, Gx=_p(2), Gy=_p(3), planar=_p(4)):
        _lib.call("smvs_dsm_facet_normals", dsm, mask, gw, gh, -999.0, T, Gx, Gy, planar, None)

    def label(dsm=_p(0), mask=_p(1), gw=gw, gh=gh, T=5, Ax=6, Ay=7, conn=8, grow=1, labels=_p(2), n_out=_p(3), ws=_p(4), nb=nbytes):
        _lib.call("smvs_dsm_facet_label", dsm, mask, gw, gh, -999.0, T, Ax, Ay, conn, grow, labels, n_out, ws, nb, None)

    def planes(labels=_p(0), dsm=_p(1), gw=gw, gh=gh, n=3, sums=_p(2), centre=_p(3), moments=_p(4), plane=_p(5), sse=_p(6), max_abs=_p(7)):
        _lib.call("smvs_dsm_facet_planes", labels, dsm, gw, gh, -999.0, n, sums, centre, moments, plane, sse, max_abs, None)

    for name in ("dsm", "Gx", "Gy", "planar"):
        with pytest.raises(E, match="null pointer"):
            normals(**{name: None})
    for name in ("dsm", "labels", "n_out", "ws"):
        with pytest.raises(E, match="null pointer"):
            label(**{name: None})
    for name in ("labels", "dsm", "sums", "centre", "moments", "plane", "sse", "max_abs"):
        with pytest.raises(E, match="null pointer"):
            planes(**{name: None})
    for call in (normals, label, planes):
        for kw in ({"gw": 0}, {"gh": 0}, {"gw": -3}):
            with pytest.raises(E, match="non-positive"):
                call(**kw)
    for call in (normals, label):
        with pytest.raises(E, match="too large"):
            call(gw=65536, gh=32768)
        for T in (-1, 2 ** 26 + 1):
            with pytest.raises(E, match="T must be"):
                call(T=T)
    for kw in ({"Ax": -1}, {"Ay": -1}, {"Ax": 2 ** 26 + 1}, {"Ay": 2 ** 26 + 1}):
        with pytest.raises(E, match="Ax and Ay"):
            label(**kw)
    for conn in (0, 6, 9):
        with pytest.raises(E, match="connectivity"):
            label(conn=conn)
    for grow in (-1, 2):
        with pytest.raises(E, match="grow must be"):
            label(grow=grow)
    with pytest.raises(E, match="workspace too small"):
        label(nb=nbytes - 1)
    for kw in ({"gw": 32769, "gh": 1}, {"gw": 1, "gh": 32769}, {"gw": 4096, "gh": 4096}):
        with pytest.raises(E, match="grid too large"):
            planes(**kw)
    with pytest.raises(E, match="n must be"):
        planes(n=-1)
    # aliasing: an output on an input, two outputs, the workspace
    with pytest.raises(E, match="aliases"):
        normals(Gx=_p(0))
    with pytest.raises(E, match="aliases"):
        normals(Gy=_p(2))
    with pytest.raises(E, match="aliases"):
        normals(planar=_p(1))
    with pytest.raises(E, match="aliases"):
        label(labels=_p(0))
    with pytest.raises(E, match="aliases"):
        label(n_out=C.c_void_p(_p(2).value + 4 * gw * gh - 4))
    with pytest.raises(E, match="aliases"):
        label(ws=C.c_void_p(_p(2).value - nbytes + 1))
    with pytest.raises(E, match="aliases"):
        label(ws=_p(1))
    for name in ("sums", "centre", "moments", "plane", "sse", "max_abs"):
        with pytest.raises(E, match="aliases"):
            planes(**{name: _p(1)})
    with pytest.raises(E, match="aliases"):
        planes(max_abs=C.c_void_p(_p(6).value + 8 * 3 - 1))
    assert lib.smvs_last_error().decode() != ""
    planes(n=0)                                              # SMVS_OK without a launch
