"""Viewsheds and lines of sight on the MI355X (smvs_dsm_viewshed, smvs_dsm_los, dsm.viewshed / visibility_count / line_of_sight /
intervisibility) against the numpy oracle (tests/dsm_viewshed_oracle.py): codes by value, `above` by its bits, no cell excused.
The case matrix of tests/dsm_viewshed_scene.py (sizes around both lane mappings' tiles, a town with voids and salt noise seen
from its corners, an edge, the centre, a roof and a street, edge values, target heights, ranges, curvature), batches of 1 to 65
observers, a 2300 x 2300 closed form, guard words, garbage in the workspace, side streams, repeated calls, every host check,
the list of lines, and the objects of a DSM seen from the highest of them."""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest
import torch

import dsm_viewshed_oracle as vo
import dsm_viewshed_scene as sc
from dsm_testkit import dev, lib, scene as _scene  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ND = sc.ND
ERR_ARG = 1                                                                # SMVS_ERR_ARG
GUARD = 64


def _guarded(n, dtype, fill, d):
    """A buffer of n elements with GUARD more at both ends, all `fill` -> (the whole tensor, the pointer to element GUARD)."""
    t = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=d)
    return t, C.c_void_p(t.data_ptr() + GUARD * t.element_size())


def _inner(t, n, fill, what):
    """The n elements between the guards, on the host, after checking that the guards still hold `fill`."""
    h = t.cpu().numpy()
    assert (h[:GUARD] == fill).all() and (h[n + GUARD:] == fill).all(), "%s: written outside its buffer" % what
    return h[GUARD:n + GUARD]


def _viewshed_c(z, nodata, t, observers, above=True, fill=0xff, stream=None):
    """The C entry on a host grid (or a device tensor): every output and the workspace inside guard words, the workspace full of
    `fill`, on `stream` -> (seen (m, gh, gw) uint8, above (m, gh, gw) float32 or None, status (m) int32)."""
    from satmvs_amd import _lib
    d = torch.device("cuda", 0)
    gh, gw = z.shape
    m = len(observers)
    n = m * gw * gh
    zd = z if isinstance(z, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(z, np.float32)).to(d)
    nbytes = _lib.load().smvs_dsm_viewshed_workspace_bytes(gw, gh, m)
    assert nbytes > 0 and nbytes % 256 == 0
    ws, ws_p = _guarded(nbytes, torch.uint8, fill, d)
    seen, seen_p = _guarded(n, torch.uint8, 77, d)
    ab, ab_p = _guarded(n, torch.float32, 12345.0, d) if above else (None, None)
    status, status_p = _guarded(m, torch.int32, -7, d)
    host = np.ascontiguousarray(np.array(observers, np.int32).reshape(m, 5))
    torch.cuda.synchronize()
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        _lib.call("smvs_dsm_viewshed", _lib.ptr(zd), gw, gh, float(nodata), t[0], t[1], t[2], t[3], host.ctypes.data_as(C.c_void_p), m,
                  seen_p, ab_p, status_p, ws_p, nbytes, _lib.current_stream(d))
    torch.cuda.synchronize()
    _inner(ws, nbytes, fill, "workspace")                                  # only its guards are looked at
    return (_inner(seen, n, 77, "seen").reshape(m, gh, gw), _inner(ab, n, np.float32(12345.0), "above").reshape(m, gh, gw) if above else None,
            _inner(status, m, -7, "status"))


def _los_c(z, nodata, t, pairs, above=True, stream=None):
    """smvs_dsm_los on a host grid and an (n, 7) host list, the outputs inside guard words -> (seen (n), above (n) or None)."""
    from satmvs_amd import _lib
    d = torch.device("cuda", 0)
    gh, gw = z.shape
    p = torch.from_numpy(np.ascontiguousarray(pairs, np.int32).reshape(-1, 7)).to(d)
    n = p.shape[0]
    zd = z if isinstance(z, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(z, np.float32)).to(d)
    seen, seen_p = _guarded(n, torch.uint8, 77, d)
    ab, ab_p = _guarded(n, torch.float32, 12345.0, d) if above else (None, None)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        _lib.call("smvs_dsm_los", _lib.ptr(zd), gw, gh, float(nodata), t[0], t[1], t[2], t[3], _lib.ptr(p), n, seen_p, ab_p, _lib.current_stream(d))
    torch.cuda.synchronize()
    return _inner(seen, n, 77, "seen"), _inner(ab, n, np.float32(12345.0), "above") if above else None


def _compare(got, want, what):
    sc.compare(got[0], want[0], "%s: seen" % (what,))
    sc.compare(got[1], want[1], "%s: above" % (what,))
    sc.compare(np.ascontiguousarray(got[2]), want[2], "%s: status" % (what,))


# ---- the matrix ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", sc.GROUPS)
def test_viewshed_against_the_oracle(dev, group):
    """Every case with `above` and without it: equal codes both ways, and equal to the oracle's."""
    for name, z, nodata, t, observers in sc.matrix(group):
        want = vo.viewshed(z, nodata, t, observers)
        _compare(_viewshed_c(z, nodata, t, observers), want, name)
        bare = _viewshed_c(z, nodata, t, observers, above=False)
        sc.compare(bare[0], want[0], "%s: seen without above" % name)
        sc.compare(np.ascontiguousarray(bare[2]), want[2], "%s: status without above" % name)


@pytest.fixture(scope="module")
def sixty_five():
    """One grid, 65 observers on cells with a height (every fifth an absolute eye), the oracle's maps: shared by the batching
    tests and left unchanged."""
    shape = (45, 52)
    z = sc.special(shape, 500)
    rng = np.random.default_rng(501)
    r, c = np.nonzero(vo.valid(z, ND))
    pick = rng.choice(r.size, 65, replace=False)
    heights = rng.integers(0, 4000, 65) / 256.0
    records = [sc.observer(r[k], c[k], eye_m=150.0 + heights[i] if i % 5 == 0 else heights[i], mode=1 if i % 5 == 0 else 0, tgt_m=float(i % 3))
               for i, k in enumerate(pick)]
    t = sc.terms(shape, (5.0, 2.5))
    return z, t, np.stack([r[pick], c[pick]], axis=1), heights, records, vo.viewshed(z, ND, t, records)


@pytest.mark.parametrize("K", [1, 2, 3, 63, 64])
def test_batches_have_equal_bits(dev, sixty_five, K):
    """K observers in one call against the oracle, and every one of them against a call of its own."""
    z, t, _, _, records, want = sixty_five
    pick = {1: [7], 2: [0, 16], 3: [0, 21, 42]}.get(K, list(range(K)))
    got = _viewshed_c(z, ND, t, [records[k] for k in pick])
    _compare(got, tuple(w[pick] for w in want), K)
    for j in range(K):
        alone = _viewshed_c(z, ND, t, [records[pick[j]]])
        _compare(alone, tuple(g[j:j + 1] for g in got), (K, j, "alone"))


def test_sixty_five_observers_through_python(dev, sixty_five):
    from satmvs_amd import dsm
    z, t, cells, heights, _, _ = sixty_five
    grid = dsm.DSMGrid(0.0, 0.0, 5.0, 2.5, z.shape[1], z.shape[0])
    records = [sc.observer(r, c, eye_m=h, tgt_m=1.0) for (r, c), h in zip(cells, heights)]
    want = vo.viewshed(z, ND, t, records)
    seen, above = dsm.viewshed(z, grid, cells, observer_height=heights, target_height=1.0, return_above=True)
    assert isinstance(seen, np.ndarray) and seen.shape == (65,) + z.shape and above.shape == seen.shape
    sc.compare(seen, want[0], "65 observers: seen")
    sc.compare(above, want[1], "65 observers: above")
    sc.compare(dsm.viewshed(z, grid, cells[64:], observer_height=heights[64], target_height=1.0), want[0][64:], "the 65th alone")
    on = dsm.viewshed(torch.from_numpy(z).to(dev), grid, torch.from_numpy(cells[60:]).to(dev), observer_height=heights[60:], target_height=1.0)
    assert isinstance(on, torch.Tensor) and on.is_cuda and on.dtype == torch.uint8
    sc.compare(on.cpu().numpy(), want[0][60:], "device tensors in and out")
    sc.compare(dsm.viewshed(z.astype(np.float64), grid, cells[:2].tolist(), observer_height=float(heights[0]), target_height=1.0)[:1], want[0][:1], "float64 in, lists")
    count = dsm.visibility_count(seen)
    assert count.dtype == np.int32 and np.array_equal(count, vo.visibility_count(want[0]))
    assert np.array_equal(dsm.visibility_count(torch.from_numpy(seen).to(dev)).cpu().numpy(), count)
    absolute = dsm.viewshed(z, grid, cells[:3], observer_height=300.0, absolute=True, curvature=False, max_distance=90.0, return_above=True)
    want_abs = vo.viewshed(z, ND, sc.terms(z.shape, (5.0, 2.5), curvature=False, max_distance=90.0), [sc.observer(r, c, eye_m=300.0, mode=1) for r, c in cells[:3]])
    sc.compare(absolute[0], want_abs[0], "absolute eyes: seen")
    sc.compare(absolute[1], want_abs[1], "absolute eyes: above")


def test_an_observer_on_a_void(dev):
    from satmvs_amd import dsm
    shape = (30, 40)
    z = sc.town(shape, 600)
    grid = dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, shape[1], shape[0])
    void = (shape[0] // 2 - 2, shape[1] // 2 + 3)                          # in the NaN hole beside the first block
    assert np.isnan(z[void])
    with pytest.raises(ValueError, match=r"observer 1 stands on cell \(row %d, col %d\)" % void):
        dsm.viewshed(z, grid, [(0, 0), void])
    seen, above = dsm.viewshed(z, grid, [(0, 0), void], invalid_observer="mark", return_above=True)
    assert (seen[1] == 0).all() and (above[1] == ND).all() and (seen[0] == 1).any()
    got = _viewshed_c(z, ND, sc.terms(shape), [sc.observer(0, 0), sc.observer(*void), sc.observer(*void, eye_m=180.0, mode=1)])
    assert got[2].tolist() == [1, 0, 1] and (got[0][1] == 0).all() and (got[0][2] == 1).any()
    _compare(got, vo.viewshed(z, ND, sc.terms(shape), [sc.observer(0, 0), sc.observer(*void), sc.observer(*void, eye_m=180.0, mode=1)]), "void observers")
    over = dsm.viewshed(z, grid, [void], observer_height=180.0, absolute=True)          # an absolute eye may hang over a void
    sc.compare(over, got[0][2:], "absolute over a void")


# ---- a large closed form ---------------------------------------------------------------------------------------------------------
def test_a_wall_on_a_large_plane(dev):
    """A 2300 x 2300 plane with a 6 m wall in column 100, seen from 10 m above the corner, against the similar triangles
    (dsm_viewshed_scene.wall_closed_form) evaluated by torch on the device: n reaches 2299."""
    from satmvs_amd import _lib
    side, a = 2300, 100
    z = torch.zeros((side, side), dtype=torch.float32, device=dev)
    z[:, a] = 6.0
    seen = torch.full((side * side,), 77, dtype=torch.uint8, device=dev)
    above = torch.empty(side * side, dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    nbytes = _lib.load().smvs_dsm_viewshed_workspace_bytes(side, side, 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    host = np.array([sc.observer(0, 0, eye_m=10.0, tgt_m=0.5)], np.int32)
    _lib.call("smvs_dsm_viewshed", _lib.ptr(z), side, side, -999.0, 5.0, 5.0, 0.0, math.inf, host.ctypes.data_as(C.c_void_p), 1,
              _lib.ptr(seen), _lib.ptr(above), _lib.ptr(status), _lib.ptr(ws), nbytes, _lib.current_stream(dev))
    rt, ct = torch.meshgrid(torch.arange(side, device=dev), torch.arange(side, device=dev), indexing="ij")
    hidden, need = sc.wall_closed_form(torch, ct, rt, 0, 0, a, vo.units(6.0), vo.units(10.0), vo.units(0.5))
    want_seen = torch.where(hidden, 2, 1).to(torch.uint8)
    want_above = torch.where(hidden, (need.double() / 256.0).float(), torch.zeros_like(above).reshape(side, side))
    assert int(status[0]) == 1 and 10 ** 5 < int(hidden.sum()) < side * side // 2
    wrong = (seen.reshape(side, side) != want_seen) | (above.reshape(side, side).view(torch.int32) != want_above.view(torch.int32))
    assert not bool(wrong.any()), (int(wrong.sum()), torch.nonzero(wrong)[:3].tolist())


# ---- call hygiene ----------------------------------------------------------------------------------------------------------------
def test_entry_repeats_streams_and_workspaces(dev, lib):
    """A workspace full of 0xff, 0x00 and 0x5a, a side stream, equal bits over two calls, a larger call before a smaller one
    (guard words round every output and the workspace are in every call of this file)."""
    big, small = sc.town((150, 210), 50, voids=0.05), sc.special((70, 33), 51)
    obs_big, obs_small = sc.town_observers((150, 210))[3:8], sc.corners_and_centre((70, 33))[:2]
    t_big, t_small = sc.terms((150, 210)), sc.terms((70, 33), (5.0, 2.5))
    assert lib.smvs_dsm_viewshed_workspace_bytes(210, 150, 5) >= lib.smvs_dsm_viewshed_workspace_bytes(33, 70, 2) > 0
    bd = torch.from_numpy(big).to(dev)
    want = vo.viewshed(big, ND, t_big, obs_big)
    runs = [_viewshed_c(bd, ND, t_big, obs_big, fill=fill) for fill in (0xff, 0x00, 0x5a, 0xff)]
    runs.append(_viewshed_c(bd, ND, t_big, obs_big, stream=torch.cuda.Stream(dev)))
    for got in runs:
        _compare(got, want, "repeats")
    assert np.array_equal(runs[0][1].view(np.uint32), runs[3][1].view(np.uint32)) and np.array_equal(runs[0][0], runs[3][0])
    _compare(_viewshed_c(small, ND, t_small, obs_small), vo.viewshed(small, ND, t_small, obs_small), "the smaller call after the larger")


def test_rejections(dev, lib):
    gw, gh = 40, 30
    z = torch.zeros((gh, gw), dtype=torch.float32, device=dev)
    seen = torch.full((2, gh, gw), 77, dtype=torch.uint8, device=dev)
    above = torch.full((2, gh, gw), 77.0, dtype=torch.float32, device=dev)
    status = torch.full((2,), 77, dtype=torch.int32, device=dev)
    pairs = torch.zeros((50, 7), dtype=torch.int32, device=dev)
    nbytes = lib.smvs_dsm_viewshed_workspace_bytes(gw, gh, 2)
    ws = torch.full((nbytes,), 77, dtype=torch.uint8, device=dev)
    P = lambda t: t.data_ptr()                                # noqa: E731
    inf, nan = float("inf"), float("nan")
    good = [3, 4, 410, 0, 0, 39, 29, -5, 1, 2560]
    ok = dict(z=P(z), gw=gw, gh=gh, xres=5.0, yres=5.0, c256=1.7e-5, r2max=inf, obs=good, n=2, seen=P(seen), above=P(above), status=P(status), ws=P(ws),
              nbytes=nbytes, pairs=P(pairs), n_pairs=50)

    def shed(**change):
        a = dict(ok, **change)
        host = None if a["obs"] is None else (C.c_int * len(a["obs"]))(*a["obs"])
        return lib.smvs_dsm_viewshed(a["z"], a["gw"], a["gh"], -999.0, a["xres"], a["yres"], a["c256"], a["r2max"], host, a["n"], a["seen"], a["above"],
                                     a["status"], a["ws"], a["nbytes"], None)

    def los(**change):
        a = dict(ok, **change)
        return lib.smvs_dsm_los(a["z"], a["gw"], a["gh"], -999.0, a["xres"], a["yres"], a["c256"], a["r2max"], a["pairs"], a["n_pairs"], a["seen"], a["above"], None)

    def second(*o):
        return dict(obs=good[:5] + list(o))

    scalars = [dict(z=None), dict(seen=None), dict(gw=0), dict(gh=-1), dict(gw=65536, gh=32768), dict(gw=65537, gh=1), dict(gw=1, gh=65537),
               dict(xres=0.0), dict(yres=-5.0), dict(xres=nan), dict(yres=inf), dict(c256=-1e-9), dict(c256=nan), dict(c256=inf),
               dict(c256=1.001 * 2.0 ** 30 / (200.0 ** 2 + 150.0 ** 2)), dict(c256=0.0, xres=1e200), dict(r2max=0.0), dict(r2max=-1.0), dict(r2max=nan), dict(r2max=-inf),
               dict(seen=P(z)), dict(above=P(z)), dict(above=P(seen)), dict(seen=P(z) + 4 * gw * gh - 1)]
    bad_shed = scalars + [dict(obs=None), dict(status=None), dict(ws=None), dict(n=0), dict(n=-1), dict(n=65, obs=good[:5] * 65),
                          second(40, 0, 0, 0, 0), second(-1, 0, 0, 0, 0), second(0, 30, 0, 0, 0), second(0, -1, 0, 0, 0), second(0, 0, 0, 2, 0), second(0, 0, 0, -1, 0),
                          second(0, 0, -1, 0, 0), second(0, 0, 2 ** 23 + 1, 0, 0), second(0, 0, 2 ** 23 + 1, 1, 0), second(0, 0, -2 ** 23 - 1, 1, 0),
                          second(0, 0, 0, 0, -1), second(0, 0, 0, 1, 2 ** 23 + 1), dict(nbytes=nbytes - 1), dict(nbytes=0),
                          dict(status=P(seen)), dict(ws=P(z)), dict(ws=P(above)), dict(status=P(ws) + 256), dict(seen=P(ws) + nbytes - 1), dict(status=P(above) + 4)]
    bad_los = scalars + [dict(pairs=None), dict(n_pairs=0), dict(n_pairs=-3), dict(pairs=P(z)), dict(seen=P(pairs)), dict(above=P(pairs) + 28 * 50 - 1),
                         dict(above=P(seen) + 49)]
    for fn, bad in ((shed, bad_shed), (los, bad_los)):
        for change in bad:
            assert fn(**change) == ERR_ARG and lib.smvs_last_error().decode(), (fn.__name__, change)
    torch.cuda.synchronize()
    for t in (seen, above, status, ws):
        assert (t == 77).all()                                # nothing ran
    assert shed() == 0 and shed(n=1) == 0 and shed(above=None) == 0 and shed(r2max=1e-300, c256=0.0) == 0 and shed(**second(39, 29, 2 ** 23, 0, 2 ** 23)) == 0
    assert los() == 0 and los(above=None) == 0 and los(n_pairs=1) == 0
    torch.cuda.synchronize()


# ---- the list of lines -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large_town():
    shape = (257, 301)
    return sc.town(shape, 700, voids=0.05), shape


def test_los_on_random_pairs(dev, large_town):
    """4096 random pairs of the 257 x 301 town with heights, modes and target heights of their own, some with a field out of
    range (code 0: the kernel tests before it reads), with curvature and a range, with `above` and without."""
    z, (gh, gw) = large_town
    rng = np.random.default_rng(701)
    n = 4096
    pairs = np.stack([rng.integers(0, gw, n), rng.integers(0, gh, n), rng.integers(0, 3000, n), rng.integers(0, 2, n),
                      rng.integers(0, gw, n), rng.integers(0, gh, n), rng.integers(0, 1500, n)], axis=1)
    absolute = pairs[:, 3] == 1
    pairs[absolute, 2] += vo.units(150.0)
    pairs[:20, :] = pairs[20:40, :]
    for k, (field, value) in enumerate(((0, -1), (0, gw), (1, -1), (1, gh), (4, -1), (4, gw), (5, -5), (5, gh), (3, 2), (3, -1), (2, 2 ** 23 + 1),
                                        (2, -2 ** 31), (6, -1), (6, 2 ** 23 + 1), (0, 2 ** 31 - 1), (5, 2 ** 31 - 1))):
        pairs[k, field] = value
    pairs[16, 2:4] = (-1, 0)                                  # a negative eye above the observer's own cell
    pairs[17, 2:4] = (-2 ** 23 - 1, 1)
    pairs[40:60, 4:6] = pairs[40:60, 0:2]                     # n = 0
    for t in (sc.terms((gh, gw)), sc.terms((gh, gw), (30.0, 30.0), max_distance=4000.0), sc.terms((gh, gw), (5.0, 2.5), curvature=False)):
        want = vo.los(z, ND, t, pairs)
        got = _los_c(z, ND, t, pairs)
        sc.compare(got[0], want[0], "los: seen")
        sc.compare(got[1], want[1], "los: above")
        sc.compare(_los_c(z, ND, t, pairs, above=False, stream=torch.cuda.Stream(dev))[0], want[0], "los without above, on a side stream")
    assert (want[0][:18] == 0).all() and {0, 1, 2} <= set(want[0].tolist())
    assert 3 in vo.los(z, ND, sc.terms((gh, gw), (30.0, 30.0), max_distance=4000.0), pairs)[0]


def test_need_is_the_least_height_that_is_seen(dev, large_town):
    """1000 hidden cells of a viewshed, as lines of sight: with tgt = need all are seen, with need - 1 unit all hidden."""
    z, (gh, gw) = large_town
    t = sc.terms((gh, gw))
    cells = np.argwhere(vo.valid(z, ND))
    o = sc.observer(*cells[cells.shape[0] // 7])
    seen, above, _ = _viewshed_c(z, ND, t, [o])
    rt, ct = np.nonzero(seen[0] == 2)
    pick = np.random.default_rng(702).choice(rt.size, 1000, replace=False)
    rt, ct = rt[pick], ct[pick]
    need = np.rint(above[0][rt, ct].astype(np.float64) * 256.0).astype(np.int64)
    assert (need >= 1).all() and np.array_equal((need / 256.0).astype(np.float32), above[0][rt, ct])
    for lift, code in ((0, 1), (-1, 2)):
        pairs = np.stack([np.full(1000, o[0]), np.full(1000, o[1]), np.full(1000, o[2]), np.zeros(1000, np.int64), ct, rt, need + lift], axis=1)
        got = _los_c(z, ND, t, pairs)
        assert (got[0] == code).all(), (lift, np.argwhere(got[0] != code)[:3].tolist())
        assert (got[1].view(np.uint32) == 0).all() if code == 1 else np.array_equal(got[1], above[0][rt, ct])       # need does not depend on tgt


def test_line_of_sight_and_intervisibility(dev, large_town):
    from satmvs_amd import dsm
    z, (gh, gw) = large_town
    grid = dsm.DSMGrid(500000.0, 4000000.0, 5.0, 5.0, gw, gh)
    rng = np.random.default_rng(703)
    points = np.stack([rng.integers(0, gh, 40), rng.integers(0, gw, 40)], axis=1)
    points[0] = (gh // 2 - 2, gw // 2 + 3)                                 # in the NaN hole
    assert np.isnan(z[tuple(points[0])])
    maps = dsm.viewshed(z, grid, points, observer_height=2.0, target_height=2.0, invalid_observer="mark")
    inter = dsm.intervisibility(z, grid, points, height=2.0)
    assert inter.dtype == np.uint8 and inter.shape == (40, 40)
    sc.compare(inter, np.ascontiguousarray(maps[:, points[:, 0], points[:, 1]]), "intervisibility against the viewsheds read at the points")
    valid = vo.valid(z, ND)[points[:, 0], points[:, 1]]
    assert np.array_equal(np.diag(inter), valid.astype(np.uint8)) and not valid[0] and (inter[0] == 0).all() and (inter[:, 0] == 0).all()
    a, b = points[:20], points[20:]
    heights = rng.integers(0, 2000, 20) / 256.0
    code, above = dsm.line_of_sight(z, grid, a, b, observer_height=heights, target_height=0.5, max_distance=900.0, return_above=True)
    t = sc.terms((gh, gw), max_distance=900.0)
    want = vo.los(z, ND, t, np.stack([a[:, 1], a[:, 0], np.rint(256.0 * heights).astype(np.int64), np.zeros(20, np.int64), b[:, 1], b[:, 0], np.full(20, 128)], axis=1))
    sc.compare(code, want[0], "line_of_sight: codes")
    sc.compare(above, want[1], "line_of_sight: above")
    on = dsm.line_of_sight(torch.from_numpy(z).to(dev), grid, torch.from_numpy(a).to(dev), b.tolist(), observer_height=160.0, absolute=True)
    assert isinstance(on, torch.Tensor) and on.is_cuda
    want_abs = vo.los(z, ND, sc.terms((gh, gw)), np.stack([a[:, 1], a[:, 0], np.full(20, vo.units(160.0)), np.ones(20, np.int64), b[:, 1], b[:, 0], np.zeros(20, np.int64)], axis=1))
    sc.compare(on.cpu().numpy(), want_abs[0], "line_of_sight: absolute, device tensors")


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_objects_seen_from_the_highest_of_them(dev):
    """extract_dtm -> extract_objects -> an observer on the highest object's centroid cell and two more -> viewshed ->
    visibility_count -> label_stats(values=count): no object is seen by more than the three observers, and the observer's own
    object is seen at least by itself."""
    from satmvs_amd import dsm
    gh, gw = 96, 128
    grid = dsm.DSMGrid(500000.0, 4000000.0, 5.0, 5.0, gw, gh)
    c, r = np.meshgrid(np.arange(gw), np.arange(gh))
    z = _scene(grid.e0 + grid.xres * c, grid.n0 - grid.yres * r)
    dtm = dsm.extract_dtm(z, grid)
    labels, stats = dsm.extract_objects(dsm.ndsm(z, dtm), grid)
    n = len(stats["area"])
    assert n >= 2
    top = int(np.argmax(stats["max"]))
    row, col = (int(v) for v in np.rint(stats["centroid"][top]))
    assert labels[row, col] == top + 1
    seen = dsm.viewshed(z, grid, [(row, col), (0, 0), (gh - 1, gw - 1)])
    assert seen[0, row, col] == 1
    count = dsm.visibility_count(seen)
    assert np.array_equal(count, vo.visibility_count(vo.viewshed(z, ND, sc.terms((gh, gw)), [sc.observer(row, col), sc.observer(0, 0), sc.observer(gh - 1, gw - 1)])[0]))
    per = dsm.label_stats(labels, n, values=count.astype(np.float32))
    assert (per["n_valid"] == stats["area"]).all() and (per["max"] <= 3.0).all() and (per["min"] >= 0.0).all() and per["max"][top] >= 1.0
