"""Outlines on the device against the numpy oracle (tests/dsm_outline_oracle.py): every entry of the ring table and the vertex
list is compared for equality, no ring excused, and every ring table is burnt back into the label map it came from.

Sizes.  The kernels run 256 lanes a workgroup over corners ((gw + 1) (gh + 1) of them), edges, rings and vertices, and scan
them in blocks of 2048 on three levels.  SIZES holds the issue's grids and three whose corner counts are 2047, 2048 and 2049
(22 x 88, 31 x 63, 2 x 682); 257 x 301 has 77916 corners (38 blocks and a tail), and its random masks between 2048 and 2048^2
edges.  The 2300 x 2300 case has more than 2048^2 corners and edges, so the third level of every scan holds more than one
block's worth, and its serpentine is one ring of more than 2^20 edges: 23 rounds of the doubling."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dsm_label_oracle as lo
import dsm_morph_oracle as mo
import dsm_outline_oracle as oo
from dsm_testkit import dev, scene as kit_scene  # noqa: F401  (dev: fixture)

pytestmark = pytest.mark.gpu
DENSITIES = (0.3, 0.45, 0.593, 0.8, 0.95)
SIZES = [(1, 1), (1, 70), (67, 3), (128, 160), (257, 301), (22, 88), (31, 63), (2, 682)]
GH, GW = 257, 301
G = 64                                                       # guard words on both sides of an output


def _grid(dsm, gh, gw):
    return dsm.DSMGrid(500000.0, 3400000.0, 5.0, 2.5, gw, gh)


def _check(labels, n, what, want=None):
    """dsm.outlines of a label map against the oracle's walk (or `want`), and dsm.burn_rings of the result against the map."""
    from satmvs_amd import dsm
    labels = np.ascontiguousarray(labels, np.int32)
    gh, gw = labels.shape
    grid = _grid(dsm, gh, gw)
    if want is None:
        want = oo.trace(labels, n)
    got = dsm.outlines(labels, n, grid)
    assert all(isinstance(t, np.ndarray) for t in got.values())
    oo.same_rings(got, oo.with_grid(want, grid, n), what)
    bare = dsm.outlines(labels, n)
    oo.same_rings(bare, want, (what, "without a grid"))
    back = dsm.burn_rings(got["vertices"], got["offset"], got["label"], labels.shape)
    assert isinstance(back, np.ndarray) and back.dtype == np.int32 and np.array_equal(back, oo.clean(labels, n)), (what, "burn")
    return got


@functools.lru_cache(maxsize=None)
def _structured(name, conn):
    labels, n = lo.closed_form(name, GH, GW, conn)
    return labels, n, oo.trace(labels, n)                    # shared: nobody writes to it


# ---- random and structured masks -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", SIZES)
def test_random_masks(dev, shape, conn, density):
    from satmvs_amd import dsm
    labels, n = dsm.label(lo.random_mask(*shape, density, seed=int(1000 * density) + shape[1]), conn)
    got = _check(labels, n, (shape, conn, density))
    assert got["first_ring"][-1] == len(got["label"]) and (np.diff(got["first_ring"]) >= 1).all()      # every label has a ring
    assert (got["area2"][got["first_ring"][:-1]] > 0).all()


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", lo.STRUCTURED)
def test_structured_masks(dev, name, conn):
    labels, n, want = _structured(name, conn)
    got = _check(labels, n, (name, conn), want)
    if name in ("spiral", "comb"):                           # one ring of about gh gw edges: the depth of the doubling
        assert len(got["label"]) == 1 and got["edges"].sum() > GH * GW - 2 * (GH + GW)
    if name == "checkerboard":
        assert got["edges"].sum() == 4 * ((GH * GW + 1) // 2)


def test_hand_made_label_maps(dev):
    from satmvs_amd import dsm
    labels = np.array([[1, 1, 2, 2, 0, 7],
                       [1, 3, 3, 2, -1, 7],
                       [1, 3, 6, 2, 2, 0],
                       [1, 1, 1, 5, 5, 5],
                       [-1, 6, 1, 5, 0, 5],
                       [0, 6, 1, 5, 5, 5]], np.int32)          # n = 5: 6 = n + 1, 7 and -1 count as background; label 4 has no cell
    got = _check(labels, 5, "hand made")
    assert got["first_ring"].tolist() == [0, 1, 2, 3, 3, 5] and got["label"].tolist() == [1, 2, 3, 5, 5]
    assert got["area2"].tolist() == [18, 10, 6, 18, -2] and got["n_holes"].tolist() == [0, 0, 0, 0, 1]
    _check(labels, 7, "hand made, n = 7")                    # 6 now has two components: two exterior rings under one label
    _check(labels, 2, "hand made, n = 2")
    _check(labels, 1000, "hand made, n far above the map's labels")
    for n in (0, 3):
        empty = dsm.outlines(np.zeros((5, 9), np.int32), n, _grid(dsm, 5, 9))
        assert sorted(empty) == sorted(oo.KEYS + ("vertices_en", "perimeter_m", "label_perimeter_m", "n_holes"))
        assert empty["label"].shape == (0,) and empty["area2"].shape == (0,) and empty["edges"].shape == (0, 2)
        assert empty["offset"].tolist() == [0] and empty["first_ring"].tolist() == [0] * (n + 1) and empty["vertices"].shape == (0, 2)
        assert empty["vertices_en"].shape == (0, 2) and empty["label_perimeter_m"].tolist() == [0.0] * n and empty["n_holes"].tolist() == [0] * n
        assert not dsm.burn_rings(empty["vertices"], empty["offset"], empty["label"], (5, 9)).any()
    none = dsm.outlines(labels, 0)
    assert none["offset"].tolist() == [0] and none["first_ring"].tolist() == [0]
    view = np.concatenate([labels * 0 + 9, labels, labels * 0 + 9], 1)[:, 6:12]                 # a view, not contiguous
    oo.same_rings(dsm.outlines(view, 5), oo.trace(labels, 5), "view")


# ---- large grids by closed forms -------------------------------------------------------------------------------------------------
def test_wide_grid(dev):
    """3 x 2300: more columns than a scan block holds."""
    labels = np.zeros((3, 2300), np.int32)
    labels[0, :] = 1
    labels[1, ::2] = 1
    labels[2, 5:2290] = 2
    got = _check(labels, 2, "3 x 2300")
    assert got["label"].tolist() == [1, 2] and got["area2"].tolist() == [2 * (2300 + 1150), 2 * 2285]


def test_large_grid_closed_forms(dev):
    """2300 x 2300 on the device only: a full grid, stripes, and the serpentine, one ring of more than 2^20 edges.  Ring and
    vertex counts, area2 against label_stats' area, first and last vertices, and the way back through burn_rings."""
    from satmvs_amd import dsm
    g = 2300
    r, c = torch.meshgrid(torch.arange(g, device=dev), torch.arange(g, device=dev), indexing="ij")

    def run(labels, n, rings, vertices):
        labels = labels.to(torch.int32).contiguous()
        got = dsm.outlines(labels, n)
        assert all(t.is_cuda for t in got.values())
        assert got["label"].numel() == rings and got["vertices"].shape == (vertices, 2) and int(got["offset"][-1]) == vertices
        area = dsm.label_stats(labels, n)["area"]
        assert torch.equal(got["area2"], 2 * area.long()) and torch.equal(got["label"], torch.arange(1, n + 1, device=dev, dtype=torch.int32))
        assert torch.equal(got["first_ring"], torch.arange(n + 1, device=dev, dtype=torch.int32))
        back = dsm.burn_rings(got["vertices"], got["offset"], got["label"], (g, g))
        assert back.is_cuda and torch.equal(back, labels)
        return got

    got = run(torch.ones((g, g), device=dev), 1, 1, 4)
    assert got["vertices"].tolist() == [[0, 0], [0, g], [g, g], [g, 0]] and got["edges"].tolist() == [[2 * g, 2 * g]]
    got = run(torch.where(r % 2 == 0, r // 2 + 1, 0), g // 2, g // 2, 4 * (g // 2))
    i = torch.arange(g // 2, device=dev, dtype=torch.int32)
    zero, wide = torch.zeros_like(i), torch.full_like(i, g)
    want = torch.stack([zero, 2 * i, zero, 2 * i + 1, wide, 2 * i + 1, wide, 2 * i], 1).reshape(-1, 2)
    assert torch.equal(got["vertices"], want) and torch.equal(got["offset"], 4 * torch.arange(g // 2 + 1, device=dev, dtype=torch.int32))
    got = run(oo.serpentine(g, r, c), 1, 1, 4 * (g // 2))
    assert int(got["edges"].sum()) > 2 ** 20 and got["vertices"][0].tolist() == [0, 0] and got["vertices"][-1].tolist() == [1, 0]


# ---- the C entries: guard words, a workspace full of 0xff, garbage in the outputs ----------------------------------------------
def _native(dev, labels, n, fill=0xff):
    """smvs_dsm_outline_count twice and smvs_dsm_outline_write on raw pointers with guarded, seeded outputs -> the dict, numpy."""
    from satmvs_amd import _lib
    lib = _lib.load()
    gh, gw = labels.shape
    lab = torch.from_numpy(np.ascontiguousarray(labels)).to(dev)
    stream = _lib.current_stream(dev)
    counts = torch.full((3 + 2 * G,), 77, dtype=torch.int32, device=dev)
    nbytes = lib.smvs_dsm_outline_workspace_bytes(gw, gh, 0)
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)
    _lib.call("smvs_dsm_outline_count", _lib.ptr(lab), gw, gh, n, 0, _lib.ptr(counts[G:]), _lib.ptr(ws), nbytes, stream)
    ne = int(counts[G].item())
    assert counts[G + 1:G + 3].tolist() == [0, 0]
    nbytes = lib.smvs_dsm_outline_workspace_bytes(gw, gh, ne)
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)
    _lib.call("smvs_dsm_outline_count", _lib.ptr(lab), gw, gh, n, ne, _lib.ptr(counts[G:]), _lib.ptr(ws), nbytes, stream)
    assert bool((counts[:G] == 77).all()) and bool((counts[G + 3:] == 77).all())
    ne2, nr, nv = counts[G:G + 3].tolist()
    assert ne2 == ne
    spec = {"label": (torch.int32, nr), "area2": (torch.int64, nr), "edges": (torch.int32, 2 * nr), "offset": (torch.int32, nr + 1),
            "first_ring": (torch.int32, n + 1), "vertices": (torch.int32, 2 * nv)}
    bufs = {k: torch.full((m + 2 * G,), 77, dtype=dt, device=dev) for k, (dt, m) in spec.items()}
    _lib.call("smvs_dsm_outline_write", _lib.ptr(lab), gw, gh, n, ne, nr, nv, *[_lib.ptr(bufs[k][G:]) for k in spec], _lib.ptr(ws), nbytes, stream)
    torch.cuda.synchronize()
    for k, (dt, m) in spec.items():
        assert bool((bufs[k][:G] == 77).all()) and bool((bufs[k][G + m:] == 77).all()), k
    out = {k: bufs[k][G:G + m].cpu().numpy() for k, (dt, m) in spec.items()}
    out["edges"], out["vertices"] = out["edges"].reshape(nr, 2), out["vertices"].reshape(nv, 2)
    return out


def test_entries_keep_to_their_outputs(dev):
    labels, n = lo.label(lo.random_mask(97, 131, 0.55, seed=4), 8)
    labels[labels == 0] = np.where(np.arange((labels == 0).sum()) % 2 == 0, n + 1, -5)
    want = oo.trace(labels, n)
    for fill in (0xff, 0x00, 0x5a):
        oo.same_rings(_native(dev, labels, n, fill), want, "workspace full of 0x%02x" % fill)


def test_burn_entry_keeps_to_its_output(dev):
    from satmvs_amd import _lib
    labels, n = lo.label(lo.random_mask(53, 77, 0.5, seed=8), 4)
    rings = oo.trace(labels, n)
    v, off, lab = (torch.from_numpy(rings[k]).to(dev) for k in ("vertices", "offset", "label"))
    out = torch.full((53 * 77 + 2 * G,), 77, dtype=torch.int32, device=dev)
    flag = torch.full((1 + 2 * G,), 77, dtype=torch.int32, device=dev)
    _lib.call("smvs_dsm_burn", _lib.ptr(v), _lib.ptr(off), _lib.ptr(lab), len(rings["label"]), len(rings["vertices"]), 77, 53,
              _lib.ptr(out[G:]), _lib.ptr(flag[G:]), _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert bool((out[:G] == 77).all()) and bool((out[-G:] == 77).all()) and bool((flag[:G] == 77).all()) and bool((flag[G + 1:] == 77).all())
    assert int(flag[G]) == 0 and np.array_equal(out[G:-G].cpu().numpy().reshape(53, 77), labels)


# ---- determinism, streams, device tensors ---------------------------------------------------------------------------------------
def test_deterministic_streams_and_device_tensors(dev):
    from satmvs_amd import dsm
    big, nb = lo.label(lo.random_mask(300, 340, 0.593, seed=1), 8)
    small, ns = lo.label(lo.random_mask(40, 50, 0.45, seed=2), 4)
    want_big, want_small = oo.trace(big, nb), oo.trace(small, ns)
    grid = _grid(dsm, 300, 340)
    bd, sd = torch.from_numpy(big).to(dev), torch.from_numpy(small).to(dev)
    keep = bd.clone()
    a = dsm.outlines(bd, nb, grid)                           # a larger call before a smaller one
    s = dsm.outlines(sd, ns)
    b = dsm.outlines(bd, nb, grid)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        c = dsm.outlines(bd, nb, grid)
        back = dsm.burn_rings(c["vertices"], c["offset"], c["label"], big.shape)
    side.synchronize()
    assert torch.equal(bd, keep) and torch.equal(back, bd) and back.is_cuda
    for k in a:
        assert a[k].is_cuda and b[k].is_cuda and c[k].is_cuda, k
        for other in (b, c):
            x, y = a[k], other[k]
            if x.dtype == torch.float64:
                x, y = x.view(torch.int64), y.view(torch.int64)
            assert x.dtype == y.dtype and torch.equal(x, y), k
    oo.same_rings({k: t.cpu().numpy() for k, t in a.items()}, oo.with_grid(want_big, grid, nb), "device tensors")
    oo.same_rings({k: t.cpu().numpy() for k, t in s.items()}, want_small, "the smaller call")


# ---- burn_rings -----------------------------------------------------------------------------------------------------------------
def test_burn_rings_cases(dev):
    from satmvs_amd import dsm
    i32 = lambda a: np.array(a, np.int32)                    # noqa: E731
    square = lambda x0, y0, x1, y1: [(x0, y0), (x0, y1), (x1, y1), (x1, y0)]    # noqa: E731
    rings = [(3, square(-4, -2, 3, 2)), (5, square(6, 3, 20, 9)), (9, square(30, 0, 40, 4)), (9, square(-9, -9, -2, -1)),
             (2, square(1, 4, 5, 6)), (2, square(2, 5, 4, 6)[::-1]), (6, square(0, 0, 2, 8)), (6, square(0, 0, 2, 8))]
    v = i32([p for _, ring in rings for p in ring]).reshape(-1, 2)
    off = i32(np.concatenate([[0], np.cumsum([len(ring) for _, ring in rings])]))
    lab = i32([k for k, _ in rings])
    want = oo.fill(v, off, lab, (7, 10))
    assert want[0, 0] == 3 and want[1, 2] == 3 and want[2, 0] == 0 and want[3, 6] == 5 and want[6, 9] == 5       # partly off the grid
    assert not (want == 9).any() and not (want == 6).any() and want[4, 1] == 2 and want[5, 2] == 0 and want[5, 1] == 2
    got = dsm.burn_rings(v, off, lab, (7, 10))
    assert np.array_equal(got, want)
    got_d = dsm.burn_rings(*(torch.from_numpy(t).to(dev) for t in (v, off, lab)), (7, 10))
    assert got_d.is_cuda and np.array_equal(got_d.cpu().numpy(), want)
    assert np.array_equal(dsm.burn_rings(v[::-1].copy(), off, lab[::-1].copy(), (7, 10)), want)       # the winding does not matter
    assert not dsm.burn_rings(i32([]).reshape(0, 2), i32([0]), i32([]), (4, 4)).any()
    assert dsm.burn_rings(i32(square(0, 0, 2, 2)), i32([0, 0, 0, 4, 4]), i32([1, 2, 8, 3]), (1, 1)).tolist() == [[8]]   # empty rings between
    with pytest.raises(ValueError, match="both coordinates"):
        dsm.burn_rings(i32([(0, 0), (0, 3), (2, 2)]), i32([0, 3]), i32([1]), (4, 4))
    with pytest.raises(ValueError, match="offset"):
        dsm.burn_rings(*(torch.from_numpy(t).to(dev) for t in (i32(square(0, 0, 2, 2)), i32([0, 3, 2, 4]), i32([1, 2, 3]))), (4, 4))
    wide = dsm.burn_rings(i32(square(1, 0, 2299, 2)), i32([0, 4]), i32([4]), (2, 2300))               # a row longer than a wave's step
    assert (wide[:, 1:2299] == 4).all() and not wide[:, 0].any() and not wide[:, 2299].any()


def test_native_argument_rejections(dev):
    from satmvs_amd import _lib
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    gw, gh, n = 9, 7, 3
    lab = torch.ones((gh, gw), dtype=torch.int32, device=dev)
    nbytes = lib.smvs_dsm_outline_workspace_bytes(gw, gh, 32)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.zeros(3, dtype=torch.int32, device=dev)
    out = {k: torch.zeros(64, dtype=torch.int64 if k == "area2" else torch.int32, device=dev) for k in ("label", "area2", "edges", "offset", "first", "vertices")}
    p, null = _lib.ptr, ctypes.c_void_p(0)
    assert lib.smvs_dsm_outline_workspace_bytes(0, 5, 0) == 0 and lib.smvs_dsm_outline_workspace_bytes(5, 5, -1) == 0
    assert lib.smvs_dsm_outline_workspace_bytes(2 ** 15, 2 ** 14, 0) == 0 and lib.smvs_dsm_outline_workspace_bytes(5, 5, 101) == 0
    assert lib.smvs_dsm_outline_workspace_bytes(5, 5, 100) > lib.smvs_dsm_outline_workspace_bytes(5, 5, 0) > 0

    def count(labels=p(lab), gw=gw, gh=gh, n=n, max_edges=32, counts=p(counts), ws=p(ws), nbytes=nbytes):
        _lib.call("smvs_dsm_outline_count", labels, gw, gh, n, max_edges, counts, ws, nbytes, stream)

    def write(labels=p(lab), gw=gw, gh=gh, n=n, ne=32, nr=1, nv=4, label=p(out["label"]), area2=p(out["area2"]), edges=p(out["edges"]),
              offset=p(out["offset"]), first=p(out["first"]), vertices=p(out["vertices"]), ws=p(ws), nbytes=nbytes):
        _lib.call("smvs_dsm_outline_write", labels, gw, gh, n, ne, nr, nv, label, area2, edges, offset, first, vertices, ws, nbytes, stream)

    v = torch.zeros((4, 2), dtype=torch.int32, device=dev)
    off = torch.tensor([0, 4], dtype=torch.int32, device=dev)
    one = torch.ones(1, dtype=torch.int32, device=dev)
    grid_out = torch.zeros((gh, gw), dtype=torch.int32, device=dev)

    def burn(vertices=p(v), offset=p(off), label=p(one), nr=1, nv=4, gw=gw, gh=gh, out=p(grid_out), flag=p(counts)):
        _lib.call("smvs_dsm_burn", vertices, offset, label, nr, nv, gw, gh, out, flag, stream)

    bad = [(count, dict(labels=null)), (count, dict(counts=null)), (count, dict(ws=null)), (count, dict(gw=0)), (count, dict(gh=-1)),
           (count, dict(gw=2 ** 15, gh=2 ** 14)), (count, dict(n=-1)), (count, dict(max_edges=-1)), (count, dict(max_edges=4 * gw * gh + 1)),
           (count, dict(nbytes=nbytes - 1)), (count, dict(counts=p(lab))), (count, dict(ws=p(lab))), (count, dict(counts=p(ws))),
           (write, dict(labels=null)), (write, dict(label=null)), (write, dict(area2=null)), (write, dict(edges=null)), (write, dict(offset=null)),
           (write, dict(first=null)), (write, dict(vertices=null)), (write, dict(ws=null)), (write, dict(gw=0)), (write, dict(gw=2 ** 15, gh=2 ** 14)),
           (write, dict(n=-1)), (write, dict(n=0)), (write, dict(ne=-1)), (write, dict(nr=0)), (write, dict(nr=33)), (write, dict(nv=0)),
           (write, dict(nv=33)), (write, dict(ne=0)), (write, dict(nbytes=nbytes - 1)), (write, dict(label=p(lab))), (write, dict(offset=p(out["label"]))),
           (write, dict(vertices=p(ws))), (write, dict(first=p(out["area2"]))), (write, dict(edges=p(out["vertices"]))),
           (burn, dict(out=null)), (burn, dict(flag=null)), (burn, dict(vertices=null)), (burn, dict(offset=null)), (burn, dict(label=null)),
           (burn, dict(nr=-1)), (burn, dict(nv=-1)), (burn, dict(gw=0)), (burn, dict(gw=2 ** 16, gh=2 ** 15)), (burn, dict(out=p(v))),
           (burn, dict(flag=p(grid_out))), (burn, dict(out=p(off))), (burn, dict(out=p(one)))]
    for fn, kw in bad:
        with pytest.raises(_lib.SatMVSNativeError, match="code 1"):
            fn(**kw)
    torch.cuda.synchronize()
    count()                                                  # and the same arguments unchanged are accepted
    write(ne=0, nr=0, nv=0, label=null, area2=null, edges=null, vertices=null)
    burn(nr=0, nv=0, vertices=null, offset=null, label=null)
    torch.cuda.synchronize()
    assert counts[0].item() == 0 and not grid_out.any()


def test_more_edges_than_room(dev):
    """A label map that changes between the two count calls: the second finds more edges than max_edges and says so."""
    from satmvs_amd import _lib
    lib = _lib.load()
    lab = torch.ones((8, 8), dtype=torch.int32, device=dev)
    lab[::2, ::2] = 0
    counts = torch.zeros(3, dtype=torch.int32, device=dev)
    nbytes = lib.smvs_dsm_outline_workspace_bytes(8, 8, 16)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.call("smvs_dsm_outline_count", _lib.ptr(lab), 8, 8, 1, 16, _lib.ptr(counts), _lib.ptr(ws), nbytes, _lib.current_stream(dev))
    assert counts.tolist() == [-1, -1, -1]


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_objects_to_geojson(dev, tmp_path):
    """extract_objects on the known-answer scene -> outlines -> write_geojson -> read back: every feature's shoelace area is
    its object's area_m2 exactly, and the two blocks' perimeters are their closed forms."""
    from satmvs_amd import dsm
    z, box = mo.known_answer_scene()
    gh, gw = z.shape
    grid = dsm.DSMGrid(400000.0, 3500000.0, 5.0, 5.0, gw, gh)
    zd = torch.from_numpy(z).to(dev)
    above = dsm.ndsm(zd, dsm.extract_dtm(zd, grid))
    labels, stats = dsm.extract_objects(above, grid)
    n = int(stats["area"].numel())
    rings = dsm.outlines(labels, n, grid)
    assert all(t.is_cuda for t in rings.values())
    path = str(tmp_path / "objects.geojson")
    assert dsm.write_geojson(path, rings, grid, stats) == n
    features = oo.read_geojson(path)
    area_m2, area = stats["area_m2"].cpu().numpy(), stats["area"].cpu().numpy()
    assert [f[0]["label"] for f in features] == list(range(1, n + 1))
    for k, (prop, polygon) in enumerate(features):
        assert oo.shoelace2(polygon[0]) > 0 and all(oo.shoelace2(hole) < 0 for hole in polygon[1:])
        assert sum(oo.shoelace2(ring) for ring in polygon) / 2.0 == area_m2[k] == prop["area_m2"] and prop["area"] == area[k]
        assert prop["bbox"] == stats["bbox"][k].tolist() and len(prop["centroid"]) == 2
    want = oo.with_grid(oo.trace(labels.cpu().numpy(), n), grid, n)
    oo.same_rings({k: t.cpu().numpy() for k, t in rings.items()}, want, "known-answer scene")
    # the two blocks of the test kit's scene (6 x 6 and 4 x 4 cells of 5 m x 2.5 m) above its terrain
    gh, gw = 40, 50
    grid = dsm.DSMGrid(400000.0, 3500000.0, 5.0, 2.5, gw, gh)
    E, N = grid.e0 + 5.0 * np.mgrid[0:gh, 0:gw][1], grid.n0 - 2.5 * np.mgrid[0:gh, 0:gw][0]
    above = kit_scene(E, N, blocks=True, holes=False) - kit_scene(E, N, blocks=False, holes=False)
    labels, stats = dsm.extract_objects(above, grid, min_height=10.0)
    rings = dsm.outlines(labels, 2, grid)
    assert stats["area"].tolist() == [16, 36] and rings["area2"].tolist() == [32, 72] and rings["n_holes"].tolist() == [0, 0]
    assert rings["perimeter_m"].tolist() == [8 * 5.0 + 8 * 2.5, 12 * 5.0 + 12 * 2.5] == rings["label_perimeter_m"].tolist()
    assert dsm.write_geojson(path, rings, grid, stats) == 2
    for (prop, polygon), m2 in zip(oo.read_geojson(path), (200.0, 450.0)):
        assert len(polygon) == 1 and oo.shoelace2(polygon[0]) / 2.0 == m2 == prop["area_m2"]
        steps = np.abs(np.diff(polygon[0], axis=0))
        assert steps.sum() == {200.0: 60.0, 450.0: 90.0}[m2] and (steps.min(axis=1) == 0).all()
