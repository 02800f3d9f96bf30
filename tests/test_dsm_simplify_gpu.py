"""Simplified outlines and the polygon burn on the device against the oracle (tests/dsm_simplify_oracle.py): every entry of the
result is compared with np.array_equal, no ring or vertex excused; `rounds` against the round-by-round statement.

Sizes.  The kernels run 256 lanes a workgroup over the vertices, lanes of a wave that share a segment combine before the atomic,
and the scans work in blocks of 2048.  The random masks give from no ring to tens of thousands; the digitised triangles give
single segments of 63 .. 65 and 255 .. 257 interior vertices, where every vertex ties (wave and workgroup boundaries); the disc
and the rotated rectangle give the depth of the rounds; the checkerboard tens of thousands of 4-vertex rings that all fall back."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dsm_label_oracle as lo
import dsm_morph_oracle as mo
import dsm_outline_oracle as oo
import dsm_simplify_oracle as so
from dsm_testkit import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
TOL16 = (0, 1, 11, 12, 16, 40, 65535)
SIZES = [(1, 1), (1, 70), (67, 3), (128, 160), (257, 301)]
G = 64                                                       # guard words on both sides of an output


def _grid(dsm, gh, gw):
    return dsm.DSMGrid(500000.0, 3400000.0, 5.0, 2.5, gw, gh)


def _numpy(d):
    return {k: (t.cpu().numpy() if isinstance(t, torch.Tensor) else t) for k, t in d.items()}


def _check(rings, tol16, what, grid=None):
    """dsm.simplify_outlines against the round-by-round statement, rounds included."""
    from satmvs_amd import dsm
    want = so.simplify_rounds(rings, tol16)
    got = dsm.simplify_outlines(rings, tol16 / 16.0, grid)
    so.same(_numpy(got), want, (what, tol16))
    assert got["rounds"] == want["rounds"], (what, tol16, got["rounds"], want["rounds"])
    assert sorted(got) == sorted(so.KEYS + ("rounds",) + (("vertices_en", "perimeter_m", "n_holes") if grid is not None else ()))
    if grid is not None:
        full = so.with_grid(want, grid)
        g = _numpy(got)
        assert np.array_equal(g["vertices_en"], full["vertices_en"]) and np.array_equal(g["n_holes"], full["n_holes"]) and g["n_holes"].dtype == np.int32
        m = np.diff(want["offset"]).astype(np.float64)
        assert g["perimeter_m"].dtype == np.float64 and (np.abs(g["perimeter_m"] - full["perimeter_m"]) <= (m + 2) * 2.0 ** -52 * full["perimeter_m"]).all()
    return got, want


@functools.lru_cache(maxsize=None)
def _mask_rings(shape, conn, density):
    """label -> outlines on the device, once per mask: (labels, n, the rings as numpy).  Shared: nobody writes to it."""
    from satmvs_amd import dsm
    labels, n = dsm.label(lo.random_mask(*shape, density, seed=int(1000 * density) + shape[1]), conn)
    return labels, n, dsm.outlines(labels, n)


# ---- random masks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol16", TOL16)
@pytest.mark.parametrize("density", (0.3, 0.593, 0.95))
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", SIZES)
def test_random_masks(dev, shape, conn, density, tol16):
    from satmvs_amd import dsm
    labels, n, rings = _mask_rings(shape, conn, density)
    grid = _grid(dsm, *shape) if tol16 in (0, 16) else None
    got, want = _check(rings, tol16, (shape, conn, density), grid)
    if tol16 == 0:                                           # the identity, and burn_polygons == burn_rings on lattice rings
        for key in ("offset", "vertices", "area2"):
            assert np.array_equal(got[key], rings[key]), key
        assert got["simplified"].all() and np.array_equal(got["kept"], np.arange(len(rings["vertices"])))
        back = dsm.burn_polygons(rings["vertices"], rings["offset"], rings["label"], shape)
        assert back.dtype == np.int32 and np.array_equal(back, dsm.burn_rings(rings["vertices"], rings["offset"], rings["label"], shape))
        assert np.array_equal(back, labels)
    if tol16 in (12, 40) and shape[0] * shape[1] <= 128 * 160:                           # the simplified rings burnt back against the oracle's fill
        back = dsm.burn_polygons(got["vertices"], got["offset"], got["label"], shape)
        assert np.array_equal(back, so.fill(want["vertices"], want["offset"], want["label"], shape))


# ---- single long segments where every vertex ties -----------------------------------------------------------------------------------
def _staircase_with_segment(count):
    """A digitised triangle x + y < g, as it is or without its corner (0, g) or (g, 0), in which tolerance 1 treats a segment of
    exactly `count` interior vertices: the staircase, whose vertices all lie 0 or 1 / sqrt 2 from the chord."""
    for g in range(max(2, count // 2 - 2), count // 2 + 6):
        for drop in (None, 1, -1):
            ring = so.staircase(g)
            if drop is not None:
                ring = ring[:drop] + ring[drop + 1:] if drop > 0 else ring[:-1]
            sizes = []
            so.simplify_ring_rounds(ring, 16, sizes)
            if count in sizes:
                return ring
    raise AssertionError("no staircase with a segment of %d interior vertices" % count)


@pytest.mark.parametrize("count", [63, 64, 65, 255, 256, 257])
def test_segment_lengths(dev, count):
    ring = _staircase_with_segment(count)
    rings = so.table(2, (1, so.rectangle(3, 3)), (2, ring), (2, ring[:1] + ring[1:][::-1]))           # the ring, and the ring the other way round
    for tol16 in (11, 12, 16, 17):                           # 1 / sqrt 2 = 11.3 sixteenths
        got, want = _check(rings, tol16, ("staircase", count))
    assert len(got["vertices"]) < 20


# ---- depth: a disc and a rotated rectangle built on the device ----------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["disc", "rectangle"])
def test_depth(dev, scene):
    from satmvs_amd import dsm
    g = 1410
    r, c = torch.meshgrid(torch.arange(g, device=dev), torch.arange(g, device=dev), indexing="ij")
    if scene == "disc":
        mask = (r - 704) ** 2 + (c - 704) ** 2 < 700 ** 2
    else:                                                    # 1100 x 500 cells about the centre, turned by 27 degrees: integer arithmetic
        u, v = 891 * (c - 705) + 454 * (r - 705), -454 * (c - 705) + 891 * (r - 705)     # 1000 (cos, sin) of 27 degrees
        mask = (u.abs() < 550000) & (v.abs() < 250000)
    labels, n = dsm.label(mask, 4)
    assert n == 1
    rings = dsm.outlines(labels, n)
    assert all(t.is_cuda for t in rings.values()) and rings["label"].numel() == 1 and rings["vertices"].shape[0] > 2000
    host = _numpy(rings)
    for tol16 in (8, 16, 24, 32):
        want = so.simplify_rounds(host, tol16)
        got = dsm.simplify_outlines(rings, tol16 / 16.0)
        assert all(t.is_cuda for k, t in got.items() if k != "rounds")
        so.same(_numpy(got), want, (scene, tol16))
        assert got["rounds"] == want["rounds"] and 1 <= got["rounds"] <= rings["vertices"].shape[0]      # at most a round per vertex
        assert so.hausdorff_holds(host, want, tol16)
    if scene == "rectangle":
        assert len(want["vertices"]) <= 8                    # at 2 cells the staircases are gone: the four corners, cut or not


def test_many_tiny_rings(dev):
    """The 257 x 301 checkerboard under connectivity 4: tens of thousands of 4-vertex rings, all falling back at 1 cell."""
    from satmvs_amd import dsm
    labels, n = lo.closed_form("checkerboard", 257, 301, 4)
    rings = dsm.outlines(labels, n)
    assert len(rings["label"]) == n > 30000 and len(rings["vertices"]) == 4 * n
    for tol16 in (11, 16):
        got = dsm.simplify_outlines(rings, tol16 / 16.0)
        assert got["rounds"] == (2 if tol16 == 11 else 1) and np.array_equal(got["vertices"], rings["vertices"]) and np.array_equal(got["offset"], rings["offset"])
        assert np.array_equal(got["area2"], rings["area2"]) and np.array_equal(got["kept"], np.arange(4 * n))
        assert got["simplified"].tolist() == [int(tol16 == 11)] * n                      # 1 / sqrt 2 = 11.3 sixteenths
    small = oo.trace(labels[:40, :50], int(labels[:40, :50].max()))                      # and a corner of it against the oracle
    _check(small, 16, "checkerboard corner")


# ---- hand-made rings ----------------------------------------------------------------------------------------------------------------
def test_short_degenerate_and_repeated_rings(dev):
    rings = so.table(7, (1, []), (2, [(3, 3)]), (3, [(1, 1), (4, 5)]), (4, [(0, 0), (0, 3), (3, 0)]), (5, [(2, 2)] * 5),
                     (6, so.rectangle(3, 3)), (6, so.rectangle(3, 3)), (7, []), (7, so.notch(9, 5, 4)), (7, so.TOUCHING), (7, []))
    for tol16 in (0, 7, 11, 12, 15, 16, 33, 34, 65535):
        got, want = _check(rings, tol16, "short rings")
    assert np.array_equal(got["vertices"], rings["vertices"]) and not got["simplified"].any()          # at 65535 everything falls back
    for n_empty in (1, 3):                                   # rings without a vertex only, and no ring at all
        empty = so.table(1, *[(1, [])] * n_empty)
        got, want = _check(empty, 16, "empty rings")
        assert got["rounds"] == 0 and got["offset"].tolist() == [0] * (n_empty + 1) and got["vertices"].shape == (0, 2) and got["area2"].tolist() == [0] * n_empty
    none, _ = _check(so.table(3), 16, "no ring")
    assert none["offset"].tolist() == [0] and none["kept"].shape == (0,) and none["simplified"].shape == (0,) and none["first_ring"].tolist() == [0] * 4


def test_general_rings(dev):
    """Rings whose edges are not along the lattice: random polygons, a spike (a segment whose ends are one point), coordinates at
    the limit 32767, where the keys reach 2^61."""
    rng = np.random.default_rng(11)
    polys = [(1 + k % 5, [tuple(int(v) for v in p) for p in rng.integers(0, 60, (int(rng.integers(3, 40)), 2))]) for k in range(300)]
    polys.sort(key=lambda t: t[0])
    spike = [(0, 0), (0, 6), (3, 6), (3, 9), (3, 6), (6, 6), (6, 0)]
    big = [(0, 0), (0, 32767), (16000, 32767), (16001, 16384), (32767, 32767), (32767, 0), (16383, 1), (16384, 16383)]
    wide = [tuple(int(v) for v in p) for p in rng.integers(0, 32768, (500, 2))]
    rings = so.table(8, *polys, (6, spike), (7, big), (8, wide))
    for tol16 in (0, 16, 47, 48, 100, 400, 65535):
        _check(rings, tol16, "general rings")
    far = so.table(1, (1, [(0, 0), (0, 32767), (32767, 32767), (32767, 0)] + [(32767 - k, 1 + k % 2) for k in range(1, 3000)]))
    for tol16 in (15, 16, 23, 65535):
        _check(far, tol16, "a long ring at the coordinate limit")


# ---- the C entries: guard words, workspaces full of anything -------------------------------------------------------------------------
def _native(dev, rings, tol16, fill, batch=3):
    """The four entries on raw pointers with guarded, seeded outputs and a workspace full of `fill` -> the dict, numpy."""
    from satmvs_amd import _lib
    lib = _lib.load()
    v, off = (torch.from_numpy(np.ascontiguousarray(rings[k])).to(dev) for k in ("vertices", "offset"))
    nr, nv = len(rings["label"]), len(rings["vertices"])
    stream, p = _lib.current_stream(dev), _lib.ptr
    nbytes = lib.smvs_dsm_simplify_workspace_bytes(nr, nv)
    ws = torch.full((nbytes + 2 * G,), fill, dtype=torch.uint8, device=dev)
    word = torch.full((2 + 2 * G,), 77, dtype=torch.int32, device=dev)
    _lib.call("smvs_dsm_simplify_begin", p(v), p(off), nr, nv, p(word[G:]), p(ws[G:]), nbytes, stream)
    assert word[G:G + 2].tolist() == [0, 77]
    rounds = 0
    for _ in range(200):
        _lib.call("smvs_dsm_simplify_rounds", p(v), p(off), nr, nv, tol16, batch, p(word[G:]), p(ws[G:]), nbytes, stream)
        splits, rounds = word[G:G + 2].tolist()
        assert splits >= 0
        if splits == 0:
            break
    _lib.call("smvs_dsm_simplify_count", p(v), p(off), nr, nv, p(word[G:]), p(ws[G:]), nbytes, stream)
    n_out = int(word[G].item())
    assert bool((word[:G] == 77).all()) and bool((word[G + 2:] == 77).all()) and 0 <= n_out <= nv
    spec = {"offset": (torch.int32, nr + 1), "vertices": (torch.int32, 2 * n_out), "area2": (torch.int64, nr), "kept": (torch.int32, n_out),
            "simplified": (torch.uint8, nr)}
    bufs = {k: torch.full((m + 2 * G,), 77, dtype=dt, device=dev) for k, (dt, m) in spec.items()}
    _lib.call("smvs_dsm_simplify_write", p(v), p(off), nr, nv, n_out, *[p(bufs[k][G:]) for k in spec], p(ws[G:]), nbytes, stream)
    torch.cuda.synchronize()
    for k, (dt, m) in spec.items():
        assert bool((bufs[k][:G] == 77).all()) and bool((bufs[k][G + m:] == 77).all()), k
    assert bool((ws[:G] == fill).all()) and bool((ws[G + nbytes:] == fill).all())
    out = {k: bufs[k][G:G + m].cpu().numpy() for k, (dt, m) in spec.items()}
    out["vertices"] = out["vertices"].reshape(n_out, 2)
    out["label"], out["first_ring"], out["rounds"] = rings["label"], rings["first_ring"], rounds
    return out


def test_entries_keep_to_their_outputs(dev):
    labels, n = lo.label(lo.random_mask(97, 131, 0.55, seed=4), 8)
    rings = oo.trace(labels, n)
    want = so.simplify_rounds(rings, 16)
    for fill, batch in ((0xff, 3), (0x00, 1), (0x5a, 8)):
        got = _native(dev, rings, 16, fill, batch)
        so.same(got, want, "workspace full of 0x%02x" % fill)
        assert got["rounds"] == want["rounds"]


def test_burn_polygons_entry_keeps_to_its_output(dev):
    from satmvs_amd import _lib
    rng = np.random.default_rng(3)
    rings = so.table(3, *[(1 + k, [tuple(int(v) for v in p) for p in rng.integers(-9, 90, (9, 2))]) for k in range(3)])
    v, off, lab = (torch.from_numpy(rings[k]).to(dev) for k in ("vertices", "offset", "label"))
    out = torch.full((53 * 77 + 2 * G,), 77, dtype=torch.int32, device=dev)
    flag = torch.full((1 + 2 * G,), 77, dtype=torch.int32, device=dev)
    _lib.call("smvs_dsm_burn_polygons", _lib.ptr(v), _lib.ptr(off), _lib.ptr(lab), 3, 27, 77, 53, _lib.ptr(out[G:]), _lib.ptr(flag[G:]), _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert bool((out[:G] == 77).all()) and bool((out[-G:] == 77).all()) and bool((flag[:G] == 77).all()) and bool((flag[G + 1:] == 77).all())
    assert int(flag[G]) == 0 and np.array_equal(out[G:-G].cpu().numpy().reshape(53, 77), so.fill(rings["vertices"], rings["offset"], rings["label"], (53, 77)))


# ---- determinism, streams, device tensors -------------------------------------------------------------------------------------------
def test_deterministic_streams_and_device_tensors(dev):
    from satmvs_amd import dsm
    big = oo.trace(*lo.label(lo.random_mask(300, 340, 0.593, seed=1), 8))
    small = oo.trace(*lo.label(lo.random_mask(40, 50, 0.45, seed=2), 4))
    want_big, want_small = so.simplify_rounds(big, 16), so.simplify_rounds(small, 16)
    grid = _grid(dsm, 300, 340)
    bd = {k: torch.from_numpy(t).to(dev) for k, t in big.items()}
    sd = {k: torch.from_numpy(t).to(dev) for k, t in small.items()}
    keep = {k: t.clone() for k, t in bd.items()}
    a = dsm.simplify_outlines(bd, 1.0, grid)                 # a larger call before a smaller one
    s = dsm.simplify_outlines(sd, 1.0)
    b = dsm.simplify_outlines(bd, 1.0, grid)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        c = dsm.simplify_outlines(bd, 1.0, grid)
        back = dsm.burn_polygons(c["vertices"], c["offset"], c["label"], (300, 340))
    side.synchronize()
    assert all(torch.equal(bd[k], keep[k]) for k in bd) and back.is_cuda
    assert np.array_equal(back.cpu().numpy(), so.fill(want_big["vertices"], want_big["offset"], want_big["label"], (300, 340)))
    for k in a:
        if k == "rounds":
            assert a[k] == b[k] == c[k] == want_big["rounds"]
            continue
        assert a[k].is_cuda and b[k].is_cuda and c[k].is_cuda, k
        for other in (b, c):
            x, y = a[k], other[k]
            if x.dtype == torch.float64:
                x, y = x.view(torch.int64), y.view(torch.int64)
            assert x.dtype == y.dtype and torch.equal(x, y), k
    so.same(_numpy(a), want_big, "device tensors")
    so.same(_numpy(s), want_small, "the smaller call")


# ---- rejections ---------------------------------------------------------------------------------------------------------------------
def test_flag_bits(dev):
    from satmvs_amd import dsm
    good = so.table(2, (1, so.rectangle(3, 4)), (2, so.rectangle(5, 5, 10, 10)))
    on_dev = lambda d: {k: torch.from_numpy(t).to(dev) for k, t in d.items()}             # noqa: E731  (the host checks do not see tensors)
    for bad_value in (-1, 32768, 2 ** 31 - 1):
        v = good["vertices"].copy()
        v[5, 1] = bad_value
        with pytest.raises(ValueError, match="0 .. 32767"):
            dsm.simplify_outlines(on_dev(dict(good, vertices=v)), 1.0)
    for offset in ([1, 4, 8], [0, 5, 4], [0, 4, 7], [0, 4, 9], [0, -1, 8]):
        with pytest.raises(ValueError, match="rise from 0"):
            dsm.simplify_outlines(on_dev(dict(good, offset=np.array(offset, np.int32))), 1.0)
        with pytest.raises(ValueError, match="rise from 0"):
            dsm.burn_polygons(*(torch.from_numpy(t).to(dev) for t in (good["vertices"], np.array(offset, np.int32), good["label"])), (20, 20))
    for bad_value in (2 ** 20, -2 ** 20, 2 ** 31 - 1):
        v = good["vertices"].copy()
        v[2, 0] = bad_value
        with pytest.raises(ValueError, match="2\\^20"):
            dsm.burn_polygons(v, good["offset"], good["label"], (20, 20))
    v = good["vertices"].copy()
    v[2, 0] = 2 ** 20 - 1                                    # the largest coordinate: taken
    assert np.array_equal(dsm.burn_polygons(v, good["offset"], good["label"], (20, 20)), so.fill(v, good["offset"], good["label"], (20, 20)))
    assert dsm.simplify_outlines(on_dev(good), 1.0)["rounds"] == 2                       # and the same tables unchanged are accepted


def test_native_argument_rejections(dev):
    from satmvs_amd import _lib
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    good = so.table(2, (1, so.rectangle(3, 4)), (2, so.rectangle(5, 5, 10, 10)))
    v, off = torch.from_numpy(good["vertices"]).to(dev), torch.from_numpy(good["offset"]).to(dev)
    nr, nv = 2, 8
    nbytes = lib.smvs_dsm_simplify_workspace_bytes(nr, nv)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    word = torch.zeros(2, dtype=torch.int32, device=dev)
    out = {k: torch.zeros(64, dtype=torch.int64 if k == "area2" else torch.uint8 if k == "simp" else torch.int32, device=dev) for k in ("ooff", "overt", "area2", "kept", "simp")}
    p, null = _lib.ptr, ctypes.c_void_p(0)

    def begin(v=p(v), off=p(off), nr=nr, nv=nv, flag=p(word), ws=p(ws), nbytes=nbytes):
        _lib.call("smvs_dsm_simplify_begin", v, off, nr, nv, flag, ws, nbytes, stream)

    def rounds(v=p(v), off=p(off), nr=nr, nv=nv, tol16=16, rounds=2, status=p(word), ws=p(ws), nbytes=nbytes):
        _lib.call("smvs_dsm_simplify_rounds", v, off, nr, nv, tol16, rounds, status, ws, nbytes, stream)

    def count(v=p(v), off=p(off), nr=nr, nv=nv, n_out=p(word), ws=p(ws), nbytes=nbytes):
        _lib.call("smvs_dsm_simplify_count", v, off, nr, nv, n_out, ws, nbytes, stream)

    def write(v=p(v), off=p(off), nr=nr, nv=nv, n_out=8, ooff=p(out["ooff"]), overt=p(out["overt"]), area2=p(out["area2"]), kept=p(out["kept"]),
              simp=p(out["simp"]), ws=p(ws), nbytes=nbytes):
        _lib.call("smvs_dsm_simplify_write", v, off, nr, nv, n_out, ooff, overt, area2, kept, simp, ws, nbytes, stream)

    bad = []
    for fn, word_name in ((begin, "flag"), (rounds, "status"), (count, "n_out")):
        bad += [(fn, dict(v=null)), (fn, dict(off=null)), (fn, dict(ws=null)), (fn, {word_name: null}), (fn, dict(nr=-1)), (fn, dict(nv=-1)), (fn, dict(nr=0)),
                (fn, dict(nbytes=nbytes - 1)), (fn, dict(ws=p(v))), (fn, {word_name: p(off)}), (fn, {word_name: p(ws)})]
    bad += [(rounds, dict(tol16=-1)), (rounds, dict(tol16=65536)), (rounds, dict(rounds=-1)), (rounds, dict(rounds=4097)),
            (write, dict(v=null)), (write, dict(off=null)), (write, dict(ws=null)), (write, dict(ooff=null)), (write, dict(overt=null)), (write, dict(area2=null)),
            (write, dict(kept=null)), (write, dict(simp=null)), (write, dict(n_out=-1)), (write, dict(n_out=9)), (write, dict(nbytes=nbytes - 1)),
            (write, dict(ooff=p(v))), (write, dict(overt=p(off))), (write, dict(area2=p(ws))), (write, dict(kept=p(out["ooff"]))), (write, dict(simp=p(out["kept"])))]
    for fn, kw in bad:
        with pytest.raises(_lib.SatMVSNativeError, match="code 1"):
            fn(**kw)
    torch.cuda.synchronize()
    begin()                                                  # and the same arguments unchanged are accepted
    rounds()
    assert word.tolist() == [0, 2]                           # the corners split in the first round, nothing in the second
    count()
    assert word[0].item() == 8
    write()
    write(nr=0, nv=0, n_out=0, v=null, off=null, overt=null, area2=null, kept=null, simp=null)
    torch.cuda.synchronize()
    assert out["ooff"][:3].tolist() == [0, 4, 8] and out["simp"][:2].tolist() == [1, 1] and out["area2"][:2].tolist() == [24, 50]


# ---- burn_polygons ------------------------------------------------------------------------------------------------------------------
def test_burn_polygons_cases(dev):
    from satmvs_amd import dsm
    i32 = lambda a: np.array(a, np.int32)                    # noqa: E731
    rng = np.random.default_rng(5)
    triangles = [(1 + k % 7, [tuple(int(v) for v in p) for p in rng.integers(-40, 140, (3, 2))]) for k in range(60)]
    triangles.sort(key=lambda t: t[0])
    rings = so.table(7, *triangles, (7, [(-1000000, -1000000), (50, 1000000), (1000000, 3)]))
    want = so.fill(rings["vertices"], rings["offset"], rings["label"], (90, 101))
    got = dsm.burn_polygons(rings["vertices"], rings["offset"], rings["label"], (90, 101))
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and np.array_equal(got, want) and len(np.unique(want)) > 4
    got_d = dsm.burn_polygons(*(torch.from_numpy(rings[k]).to(dev) for k in ("vertices", "offset", "label")), (90, 101))
    assert got_d.is_cuda and np.array_equal(got_d.cpu().numpy(), want)
    # An edge through cell centres: with integer ends a slope of 2 : 1 cannot pass one (tests/test_dsm_simplify_cpu.py), slopes
    # 1 : 1 and 3 : 1 do.  The two triangles on either side of it: every cell in exactly one, the centres on the edge on its left.
    for (ex, ey), on_edge in (((2, 6), [(1, 0), (4, 1)]), ((4, 4), [(k, k) for k in range(4)]), ((70, 210), [(3 * k + 1, k) for k in range(70)])):
        left, right = [(0, 0), (0, ey), (ex, ey)], [(0, 0), (ex, ey), (ex, 0)]
        both = dsm.burn_polygons(i32(left + right), i32([0, 3, 6]), i32([1, 2]), (ey, ex))
        assert (both > 0).all() and (both < 3).all() and all(both[r, c] == 1 for r, c in on_edge)
        assert np.array_equal(both, so.fill(i32(left + right), i32([0, 3, 6]), i32([1, 2]), (ey, ex)))
        flipped = dsm.burn_polygons(i32(left[::-1] + right[::-1]), i32([0, 3, 6]), i32([1, 2]), (ey, ex))                 # the winding does not matter
        assert np.array_equal(flipped, both)
    assert not dsm.burn_polygons(i32([]).reshape(0, 2), i32([0]), i32([]), (4, 4)).any()
    assert not dsm.burn_polygons(i32(left + left), i32([0, 3, 6]), i32([5, 5]), (9, 9)).any()        # a ring given twice cancels
    tall = dsm.burn_polygons(i32([(1, -5), (3, 2305), (2000, 2305), (1998, -5)]), i32([0, 4]), i32([4]), (2300, 2300))   # long edges, long rows
    assert (tall[:, 3:1998] == 4).all() and not tall[:, 0].any() and not tall[:, 2000:].any()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_objects_simplified_and_burnt_back(dev, tmp_path):
    """extract_objects -> outlines -> simplify_outlines(tol) -> burn_polygons against the label map, and write_geojson of the
    simplified dict read back.

    The bound.  A cell in which the burnt map differs from the labels has its centre between an object's outline and the
    simplified ring, and every point there is within tol of the outline (the Hausdorff property, both ways: the chain between
    two kept vertices projects onto their segment continuously from end to end).  The nearest outline point lies on a side of a
    boundary cell of that object, at most half a cell diagonal, 0.71, from that cell's centre.  So the centre is within
    tol + 0.71 <= tol + 1 of a boundary cell's centre, which is what dsm.distance measures."""
    from satmvs_amd import dsm
    z, box = mo.known_answer_scene()
    gh, gw = z.shape
    grid = dsm.DSMGrid(400000.0, 3500000.0, 5.0, 2.5, gw, gh)
    zd = torch.from_numpy(z).to(dev)
    above = dsm.ndsm(zd, dsm.extract_dtm(zd, grid))
    labels, stats = dsm.extract_objects(above, grid, min_area_m2=25.0)
    n = int(stats["area"].numel())
    assert n >= 1
    rings = dsm.outlines(labels, n, grid)
    host = _numpy(rings)
    pad = torch.nn.functional.pad(labels, (1, 1, 1, 1))
    for tol in (0.0, 0.5, 1.0, 2.0):
        simple = dsm.simplify_outlines(rings, tol, grid)
        want = so.with_grid(so.simplify_rounds(host, int(16 * tol)), grid)
        got = _numpy(simple)
        so.same(got, want, ("objects", tol))
        burnt = dsm.burn_polygons(simple["vertices"], simple["offset"], simple["label"], (gh, gw))
        if tol == 0.0:
            assert torch.equal(burnt, labels)
        for k in range(1, n + 1):
            mine = pad == k
            inner = mine[1:-1, 1:-1]
            edge = inner & ~(mine[:-2, 1:-1] & mine[2:, 1:-1] & mine[1:-1, :-2] & mine[1:-1, 2:])      # the object's boundary cells
            far = dsm.distance(~edge, max_dist=64)
            differs = (burnt == k) != inner
            assert bool((far[differs] <= tol + 1).all()), (tol, k, float(far[differs].max()))
        path = str(tmp_path / "simple.geojson")
        assert dsm.write_geojson(path, simple, grid) == n
        features = oo.read_geojson(path) if tol == 0.0 else _read_geojson(path)
        assert [f[0]["label"] for f in features] == list(range(1, n + 1))
        for k, (prop, polygon) in enumerate(features):
            mine = slice(got["first_ring"][k], got["first_ring"][k + 1])
            assert len(polygon) == mine.stop - mine.start
            assert sum(oo.shoelace2(ring) for ring in polygon) / 2.0 == got["area2"][mine].sum() / 2.0 * grid.xres * grid.yres
        m = np.diff(got["offset"]).astype(np.float64)
        assert (np.abs(got["perimeter_m"] - want["perimeter_m"]) <= (m + 2) * 2.0 ** -52 * want["perimeter_m"]).all()
        assert np.array_equal(got["vertices_en"], want["vertices_en"]) and np.array_equal(got["n_holes"], want["n_holes"])


def _read_geojson(path):
    """oo.read_geojson without its floor of four vertices a ring: a simplified ring may be a triangle."""
    import json
    with open(path) as f:
        doc = json.load(f)
    return [(ft["properties"], [np.array(ring, np.float64).reshape(-1, 2) for ring in ft["geometry"]["coordinates"]]) for ft in doc["features"]]
