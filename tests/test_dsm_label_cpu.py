"""Object labelling, the parts that run without a GPU: the numpy oracle (tests/dsm_label_oracle.py) against its flood fill
and against scipy.ndimage as an independent statement, the closed-form scenes, the fixed-point image of a height, the sieve,
and the argument checks of smvs_dsm_label / smvs_dsm_label_stats (rejected before any HIP call) and of the Python functions
(before any device work)."""
import ctypes as C

import numpy as np
import pytest

import dsm_label_oracle as lo
from dsm_testkit import lib  # noqa: F401  (fixtures)

ND = np.float32(-999.0)
DENSITIES = (0.3, 0.45, 0.593, 0.8)


# ---- the oracle against itself and against scipy -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,seed", [((1, 1), 0), ((1, 17), 1), ((13, 2), 2), ((19, 23), 3), ((24, 31), 4)])
def test_oracle_equals_the_flood_fill(shape, seed):
    for density in DENSITIES + (0.0, 1.0):
        m = lo.random_mask(*shape, density, seed)
        for conn in (4, 8):
            a, na = lo.label(m, conn)
            b, nb = lo.label_brute(m, conn)
            assert na == nb and np.array_equal(a, b) and a.dtype == np.int32, (density, conn)


@pytest.mark.parametrize("density", DENSITIES)
def test_oracle_equals_scipy(density):
    ndi = pytest.importorskip("scipy.ndimage")
    m = lo.random_mask(300, 340, density, seed=int(density * 1000))
    z = lo.value_grid(300, 340, seed=5, voids=0.0)
    z[~np.isfinite(z) | (z == ND)] = np.float32(1.0)         # scipy knows no invalid cells: compare on a grid without them
    for conn, structure in ((4, None), (8, np.ones((3, 3), int))):
        want, nw = ndi.label(m, structure=structure)
        got, n = lo.label(m, conn)
        assert n == nw and np.array_equal(got, want)         # as they come: no renumbering
        st = lo.stats(got, n, z)
        idx = np.arange(1, n + 1)
        assert np.array_equal(st["area"], ndi.sum(m, want, idx).astype(np.int32))
        assert np.array_equal(st["min"], ndi.minimum(z, want, idx).astype(np.float32))
        assert np.array_equal(st["max"], ndi.maximum(z, want, idx).astype(np.float32))
        boxes = np.array([[s[0].start, s[1].start, s[0].stop - 1, s[1].stop - 1] for s in ndi.find_objects(want)], np.int32).reshape(n, 4)
        assert np.array_equal(st["bbox"], boxes)
        assert np.array_equal(st["qsum"], np.rint(ndi.sum(lo.q(z).astype(np.float64), want, idx)).astype(np.int64))
        com = np.array(ndi.center_of_mass(m, want, idx)).reshape(n, 2)
        assert np.allclose(st["centroid"], com, rtol=0, atol=1e-9) and (st["n_valid"] == st["area"]).all()


@pytest.mark.parametrize("shape", [(5, 5), (9, 14), (16, 11), (24, 31), (33, 70)])
def test_closed_form_scenes_equal_the_oracle(shape):
    gh, gw = shape
    for name in lo.STRUCTURED:
        m = lo.structured(name, gh, gw)
        for conn in (4, 8):
            got, n = lo.label(m, conn)
            brute, nb = lo.label_brute(m, conn)
            assert n == nb and np.array_equal(got, brute), (name, conn)
            cf = lo.closed_form(name, gh, gw, conn)
            assert cf[1] == n and np.array_equal(cf[0], got), (name, conn)
    assert lo.structured("spiral", gh, gw).sum() >= gh * gw // 2 - gh - gw        # its path is half the grid
    m, labels, n = lo.squares(gh, gw)
    for conn in (4, 8):
        got, ng = lo.label(m, conn)
        assert ng == n and np.array_equal(got, labels)


def test_q_edge_values():
    v = np.array([2.0 ** 21, 3e6, np.inf, -2.0 ** 21, -3e6, -np.inf, 0.0, -0.0, 1.0, -1.0], np.float32)
    assert lo.q(v).tolist() == [2 ** 31, 2 ** 31, 2 ** 31, -2 ** 31, -2 ** 31, -2 ** 31, 0, 0, 1024, -1024]
    halves = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 3.5], np.float64) / 1024.0            # exact in float32: halves go to even
    assert lo.q(halves.astype(np.float32)).tolist() == [0, 2, 2, 0, -2, 4]
    assert lo.q(np.float32(np.nextafter(np.float32(2.0 ** 21), np.float32(0.0)))) == 2 ** 31 - 128      # the last float32 below the clamp
    assert (2 ** 31 - 1) * 2 ** 31 < 2 ** 62                 # the most cells the entries accept, each at the clamp
    labels = np.ones((3, 4), np.int32)
    st = lo.stats(labels, 1, np.full((3, 4), 3e6, np.float32))
    assert st["qsum"].tolist() == [12 * 2 ** 31] and st["mean"].tolist() == [2.0 ** 21] and st["max"].tolist() == [np.float32(3e6)]
    z = np.zeros((1, 4), np.float32)
    z[0, 1] = -0.0
    st = lo.stats(np.ones((1, 4), np.int32), 1, z)
    assert np.signbit(st["min"][0]) and not np.signbit(st["max"][0])


def test_stats_rules():
    labels = np.array([[1, 1, 0, 3], [0, -5, 4, 3], [2, 2, 2, 3]], np.int32)
    z = np.array([[1.0, np.nan, 5.0, -999.0], [2.0, 2.0, 2.0, np.nan], [-1.5, 0.25, -999.0, np.inf]], np.float32)
    st = lo.stats(labels, 3, z)
    assert st["area"].tolist() == [2, 3, 3] and st["n_valid"].tolist() == [1, 2, 0]
    assert st["bbox"].tolist() == [[0, 0, 0, 1], [2, 0, 2, 2], [0, 3, 2, 3]]
    assert st["rc_sum"].tolist() == [[0, 1], [6, 3], [3, 9]] and st["centroid"].tolist() == [[0.0, 0.5], [2.0, 1.0], [1.0, 3.0]]
    assert st["min"].tolist() == [1.0, -1.5, -999.0] and st["max"].tolist() == [1.0, 0.25, -999.0]
    assert st["qsum"].tolist() == [1024, -1280, 0] and st["mean"][:2].tolist() == [1.0, -0.625] and np.isnan(st["mean"][2])
    none = lo.stats(labels, 5)
    assert none["area"].tolist() == [2, 3, 3, 1, 0] and none["bbox"][4].tolist() == [lo.INT_MAX, lo.INT_MAX, -1, -1]
    assert sorted(none) == ["area", "bbox", "centroid", "rc_sum"] and lo.stats(labels, 0)["area"].shape == (0,)


def test_sieve_labels_keeps_raster_order():
    import torch
    from satmvs_amd import dsm
    m = lo.random_mask(40, 50, 0.45, seed=3)
    labels, n = lo.label(m, 4)
    area = lo.stats(labels, n)["area"]
    for lo_a, hi_a in ((1, None), (3, None), (2, 6), (0, 1), (10 ** 6, None)):
        want, nw, kw = lo.sieve(labels, area, lo_a, hi_a)
        relabelled, n2 = lo.label(want != 0, 4)              # the survivors, labelled afresh: the same numbering
        assert n2 == nw and np.array_equal(relabelled, want)
        got, ng, kg = dsm.sieve_labels(labels, area, lo_a, hi_a)
        assert isinstance(got, np.ndarray) and got.dtype == np.int32 and ng == nw
        assert np.array_equal(got, want) and np.array_equal(kg, kw) and kg.dtype == np.int64
        assert ((area[kw] >= lo_a) & (area[kw] <= (hi_a or 10 ** 9))).all()
        t, nt, kt = dsm.sieve_labels(torch.from_numpy(labels), torch.from_numpy(area), lo_a, hi_a)
        assert isinstance(t, torch.Tensor) and nt == nw and np.array_equal(t.numpy(), want) and np.array_equal(kt.numpy(), kw)


# ---- argument checks -----------------------------------------------------------------------------------------------------------
def test_label_entries_reject_bad_arguments_without_a_gpu(lib):
    from satmvs_amd import _lib
    MB = 1 << 20
    m, l, n_out, w = C.c_void_p(1 * MB), C.c_void_p(2 * MB), C.c_void_p(3 * MB), C.c_void_p(4 * MB)
    need = lib.smvs_dsm_label_workspace_bytes(8, 8)
    assert need >= 8 * 8 * 4 + 8
    assert lib.smvs_dsm_label_workspace_bytes(0, 8) == 0 and lib.smvs_dsm_label_workspace_bytes(8, -1) == 0
    assert lib.smvs_dsm_label_workspace_bytes(65536, 32768) == 0 and lib.smvs_dsm_label_workspace_bytes(65535, 32768) > 2 ** 32

    def label(mask=m, gw=8, gh=8, conn=8, labels=l, n=n_out, ws=w, nbytes=need):
        _lib.call("smvs_dsm_label", mask, gw, gh, conn, labels, n, ws, nbytes, None)

    for kw in ({"mask": None}, {"labels": None}, {"n": None}, {"ws": None}):
        with pytest.raises(_lib.SatMVSNativeError, match="null pointer"):
            label(**kw)
    for kw in ({"gh": 0}, {"gw": 0}, {"gw": -3}):
        with pytest.raises(_lib.SatMVSNativeError, match="non-positive grid"):
            label(**kw)
    with pytest.raises(_lib.SatMVSNativeError, match="grid too large"):
        label(gw=65536, gh=32768)
    for conn in (0, 6, -8, 9):
        with pytest.raises(_lib.SatMVSNativeError, match="connectivity must be"):
            label(conn=conn)
    with pytest.raises(_lib.SatMVSNativeError, match="workspace too small"):
        label(nbytes=need - 1)
    with pytest.raises(_lib.SatMVSNativeError, match="labels aliases mask"):
        label(labels=C.c_void_p(MB + 60))
    for bad in (MB + 63, 2 * MB, 2 * MB + 8 * 8 * 4 - 1):
        with pytest.raises(_lib.SatMVSNativeError, match="n_out aliases"):
            label(n=C.c_void_p(bad))
    for bad in (MB - need + 1, 2 * MB + 252, 3 * MB - need + 1, 3 * MB + 3):
        with pytest.raises(_lib.SatMVSNativeError, match="workspace aliases"):
            label(ws=C.c_void_p(bad))

    n = 10
    names = ("area", "bbox", "rc_sum", "nvalid", "vmin", "vmax", "qsum")
    sizes = dict(zip(names, (4 * n, 16 * n, 16 * n, 4 * n, 4 * n, 4 * n, 8 * n)))
    at = {name: (10 + i) * MB for i, name in enumerate(names)}

    def stats(labels=l, values=m, gw=8, gh=8, n=n, **kw):
        p = {name: C.c_void_p(at[name]) for name in names}
        if values is None:
            p.update(nvalid=None, vmin=None, vmax=None, qsum=None)
        p.update(kw)
        _lib.call("smvs_dsm_label_stats", labels, values, gw, gh, -999.0, n, *[p[name] for name in names], None)

    for kw in ({"labels": None}, {"area": None}, {"bbox": None}, {"rc_sum": None}):
        with pytest.raises(_lib.SatMVSNativeError, match="null pointer"):
            stats(**kw)
    for name in names[3:]:
        with pytest.raises(_lib.SatMVSNativeError, match="values without"):
            stats(**{name: None})
        with pytest.raises(_lib.SatMVSNativeError, match="without values"):
            stats(values=None, **{name: C.c_void_p(at[name])})
    with pytest.raises(_lib.SatMVSNativeError, match="non-positive grid"):
        stats(gh=0)
    with pytest.raises(_lib.SatMVSNativeError, match="grid too large"):
        stats(gw=65536, gh=32768)
    for bad in (-1, -2 ** 31):
        with pytest.raises(_lib.SatMVSNativeError, match="n must be"):
            stats(n=bad)
    stats(n=0)                                               # nothing to do: SMVS_OK without a launch, here without a GPU
    stats(n=0, values=None)
    for i, name in enumerate(names):                         # every output against labels, values and every other output
        for other, base, size in [("labels", 2 * MB, 8 * 8 * 4), ("values", MB, 8 * 8 * 4)] + [(o, at[o], sizes[o]) for o in names[:i]]:
            for bad in (base + size - 1, base - sizes[name] + 1):
                with pytest.raises(_lib.SatMVSNativeError, match="%s aliases %s" % (name, other)):
                    stats(**{name: C.c_void_p(bad)})
    for name in names[:3]:                                   # without values: the three outputs among themselves and against labels
        with pytest.raises(_lib.SatMVSNativeError, match="%s aliases labels" % name):
            stats(values=None, **{name: C.c_void_p(2 * MB + 4)})
    with pytest.raises(_lib.SatMVSNativeError, match="rc_sum aliases area"):
        stats(values=None, rc_sum=C.c_void_p(at["area"] + 4 * n - 1))


def test_python_entries_validate_before_the_gpu():
    import torch
    from satmvs_amd import dsm
    m = np.zeros((4, 6), np.uint8)
    lab = np.zeros((4, 6), np.int32)
    z = np.zeros((4, 6), np.float32)
    area = np.zeros(3, np.int32)
    grid = dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, 6, 4)
    other = dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, 7, 4)
    cases = [
        (lambda: dsm.label(m.astype(np.float32)), "bool or an integer"),
        (lambda: dsm.label(torch.zeros(4, 6, dtype=torch.float16)), "bool or an integer"),
        (lambda: dsm.label(np.zeros((2, 4, 6), np.uint8)), r"\(gh, gw\)"),
        (lambda: dsm.label(np.zeros(6, bool)), r"\(gh, gw\)"),
        (lambda: dsm.label(np.zeros((0, 6), np.uint8)), "positive sizes"),
        (lambda: dsm.label(m, 6), "connectivity"),
        (lambda: dsm.label(m, 8.0), "connectivity"),
        (lambda: dsm.label(m, True), "connectivity"),
        (lambda: dsm.label_stats(lab.astype(np.int64), 1), "int32"),
        (lambda: dsm.label_stats(m, 1), "int32"),
        (lambda: dsm.label_stats(lab[0], 1), r"\(gh, gw\)"),
        (lambda: dsm.label_stats(lab, -1), "n must be"),
        (lambda: dsm.label_stats(lab, 1.0), "n must be"),
        (lambda: dsm.label_stats(lab, 2 ** 31), "n must be"),
        (lambda: dsm.label_stats(lab, 1, values=z.astype(np.float64)), "float32"),
        (lambda: dsm.label_stats(lab, 1, values=z[:, :5]), "differs from the labels"),
        (lambda: dsm.label_stats(lab, 1, values=z[0]), r"\(gh, gw\)"),
        (lambda: dsm.label_stats(lab, 1, grid=other), "differs from the grid"),
        (lambda: dsm.sieve_labels(lab.astype(np.int16), area), "int32"),
        (lambda: dsm.sieve_labels(lab, area, min_area=-1), "min_area"),
        (lambda: dsm.sieve_labels(lab, area, min_area=1.5), "min_area"),
        (lambda: dsm.sieve_labels(lab, area, min_area=3, max_area=2), "max_area"),
        (lambda: dsm.sieve_labels(lab, area.astype(np.float32)), "1-D integer"),
        (lambda: dsm.sieve_labels(lab, area.reshape(1, 3)), "1-D integer"),
        (lambda: dsm.extract_objects(z.astype(np.float64), grid), "float32"),
        (lambda: dsm.extract_objects(z, other), "differs from the grid"),
        (lambda: dsm.extract_objects(z, grid, min_height=float("nan")), "min_height"),
        (lambda: dsm.extract_objects(z, grid, min_area_m2=-1.0), "min_area_m2"),
        (lambda: dsm.extract_objects(z, grid, min_area_m2=float("inf")), "min_area_m2"),
        (lambda: dsm.extract_objects(z, grid, connectivity=5), "connectivity"),
    ]
    for f, pattern in cases:
        with pytest.raises(ValueError, match=pattern):
            f()
