"""The two numpy statements of the viewshed rule (tests/dsm_viewshed_oracle.py) against each other on the case matrix and
against closed forms; the invariants of the rule; the accumulator form of the minor coordinate; viewshed_terms; every argument
rejection of the Python layer and of the C entries that needs no GPU; and planted errors that the GPU file's comparison must
report."""
import ctypes as C
import math

import numpy as np
import pytest

import dsm_viewshed_oracle as vo
import dsm_viewshed_scene as sc
from dsm_testkit import lib  # noqa: F401  (fixture)
from satmvs_amd.dsm import DSMGrid, intervisibility, line_of_sight, viewshed, viewshed_terms, visibility_count

ND = sc.ND
FLAT = (5.0, 5.0, 0.0, math.inf)


# ---- the rule, twice -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", sc.GROUPS)
def test_the_statements_agree(group):
    """The loop over pairs (Python ints, Fraction) against the arrays on every scene of the matrix: every target of grids of up
    to 700 cells, and 40 random targets of the larger ones, for the first and the last observer of the case."""
    rng = np.random.default_rng(7)
    for name, z, nodata, t, observers in sc.matrix(group):
        ok, q = vo.heights(z, nodata)
        gh, gw = z.shape
        for o in (observers[0], observers[-1]):
            code, need = vo.needs(z, nodata, t, o)
            if gh * gw <= 700:
                targets = [(r, c) for r in range(gh) for c in range(gw)]
            else:
                targets = list(zip(rng.integers(0, gh, 40).tolist(), rng.integers(0, gw, 40).tolist()))
            for r, c in targets:
                k, nd = vo.line(ok, q, t, o[0], o[1], o[2], o[3], c, r, o[4])
                assert k == code[r, c] and (k != 2 or nd == need[r, c]), (name, o, r, c, k, nd, code[r, c], need[r, c])


def test_the_matrix_is_what_the_gpu_tests_assume():
    assert {(1, 1), (1, 70), (67, 1), (2, 2), (67, 3)} <= set(sc.SIZES)
    assert {7, 8, 9, 63, 64, 65} <= {s[0] for s in sc.SIZES} and {7, 8, 9, 63, 64, 65} <= {s[1] for s in sc.SIZES}
    assert sc.TILE_H * sc.TILE_W == 64
    names, codes, res, curved = [], set(), set(), set()
    for g in sc.GROUPS:
        for name, z, nodata, t, observers in sc.matrix(g):
            names.append(name)
            assert z.dtype == np.float32 and z.ndim == 2 and 1 <= len(observers) <= sc.MAX_OBS, name
            res.add(t[:2])
            curved.add(t[2] > 0.0)
            if z.size <= 7000:
                codes |= set(np.unique(vo.viewshed(z, nodata, t, observers[:2])[0]).tolist())
    assert len(names) == len(set(names)) > 25 and codes == {0, 1, 2, 3}
    assert {(5.0, 5.0), (5.0, 2.5), (30.0, 30.0)} <= res and curved == {True, False}
    for voids in (0.05, 0.3):
        z = sc.town((128, 160), 201, voids)
        assert abs((~vo.valid(z, ND)).mean() - voids) < 0.03
    assert 0.48 < (~vo.valid(sc.special((30, 40), 410, voids=0.75), ND)).mean() < 0.6      # the kinds of void overlap: half the cells


# ---- closed forms ----------------------------------------------------------------------------------------------------------------
def test_a_level_plane_is_seen_everywhere():
    """Eye 0 on a level plane: every sample lies exactly on the line, and grazing counts as seen."""
    z = np.full((9, 33), 12.5, np.float32)
    for o in sc.corners_and_centre((9, 33), eye_m=0.0):
        seen, above, status = vo.viewshed(z, ND, FLAT, [o])
        assert (seen == 1).all() and (above.view(np.uint32) == 0).all() and status.tolist() == [1]
    seen, _, _ = vo.viewshed(sc.tilted((5, 60)), ND, FLAT, [sc.observer(2, 0, eye_m=0.0)])
    assert (seen[0, 2] == 1).all()                            # along the row the tilted plane grazes too


def test_a_wall_hides_what_the_similar_triangles_name():
    gh, gw, a = 41, 120, 30
    Hq, hq = vo.units(6.0), vo.units(10.0)
    z = sc.wall((gh, gw), a, 6.0)
    rt, ct = np.mgrid[0:gh, 0:gw]
    for ro, tgt_m in ((20, 0.0), (0, 0.0), (40, 1.5)):
        seen, above, _ = vo.viewshed(z, ND, FLAT, [sc.observer(ro, 0, eye_m=10.0, tgt_m=tgt_m)])
        hidden, need = sc.wall_closed_form(np, ct, rt, 0, ro, a, Hq, hq, vo.units(tgt_m))
        assert np.array_equal(seen[0] == 2, hidden) and (seen[0][~hidden] == 1).all() and hidden.sum() > 300
        assert np.array_equal(above[0][hidden], (need[hidden] / 256.0).astype(np.float32))
    along = vo.viewshed(z, ND, FLAT, [sc.observer(20, 0, eye_m=10.0)])[0][0, 20]           # along the observer's row: n < h a / (h - H) = 75
    assert along[31:75].tolist() == [2] * 44 and along[75:].tolist() == [1] * 45 and along[:31].tolist() == [1] * 31


def test_the_horizon_of_a_curved_row():
    """A 1 x 400 row of 30 m cells at eye 1.6 m: everything nearer than 0.9 sqrt(1.6 / k) is seen and everything beyond 1.1
    sqrt(1.6 / k) is hidden, k = 0.87 / (2 R): the horizon is about 4.84 km, 161 cells."""
    grid = sc.Grid(30.0, 30.0, 400, 1)
    t = vo.terms(grid)
    horizon = math.sqrt(1.6 / (0.87 / (2.0 * 6371008.8)))
    assert abs(horizon - 4840.0) < 10.0 and t[2] == 256.0 * 0.87 / (2.0 * 6371008.8)
    seen = vo.viewshed(np.zeros((1, 400), np.float32), ND, t, [sc.observer(0, 0)])[0][0, 0]
    d = 30.0 * np.arange(400)
    assert (seen[d < 0.9 * horizon] == 1).all() and (seen[d > 1.1 * horizon] == 2).all()
    assert (vo.viewshed(np.zeros((1, 400), np.float32), ND, vo.terms(grid, curvature=False), [sc.observer(0, 0)])[0] == 1).all()


def test_thin_grids_and_neighbours():
    for shape in ((1, 40), (40, 1)):
        z = sc.special(shape, 11, voids=0.2)
        for o in (sc.observer(0, 0, eye_m=200.0, mode=1), sc.observer(shape[0] - 1, shape[1] - 1, eye_m=50.0, mode=1)):
            got, want = vo.viewshed(z, ND, sc.terms(shape), [o]), vo.viewshed_loop(z, ND, sc.terms(shape), o)
            assert np.array_equal(got[0][0], want[0]) and np.array_equal(got[1][0].view(np.uint32), want[1].view(np.uint32))
    z = sc.special((9, 9), 12, voids=0.0)
    z[4, 4] = -30000.0                                        # an eye far below everything around it
    ok = vo.valid(z, ND)
    seen = vo.viewshed(z, ND, sc.terms((9, 9)), [sc.observer(4, 4, eye_m=0.0)])[0][0]
    assert (seen[3:6, 3:6][ok[3:6, 3:6]] == 1).all()          # n = 0 and n = 1: nothing stands between


# ---- invariants ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_town():
    shape = (40, 50)
    return sc.town(shape, 31, 0.05), shape


def test_raising_the_target_never_hides(small_town):
    z, shape = small_town
    t = sc.terms(shape)
    for o in sc.corners_and_centre(shape)[::2]:
        before = vo.viewshed(z, ND, t, [o])[0][0]
        for tgt in (0.5, 10.0, 200.0):
            after = vo.viewshed(z, ND, t, [o[:4] + (vo.units(tgt),)])[0][0]
            assert not ((before == 1) & (after != 1)).any() and np.array_equal(before == 0, after == 0)
            before = after


def test_need_is_the_least_height_that_is_seen(small_town):
    z, shape = small_town
    t = sc.terms(shape)
    ok, q = vo.heights(z, ND)
    o = sc.observer(3, 4)
    code, need = vo.needs(z, ND, t, o)
    rt, ct = np.nonzero(code == 2)
    assert rt.size > 200 and (need[rt, ct] >= 1).all()
    at = vo.lines(ok, q, t, o[0], o[1], o[2], o[3], ct, rt, need[rt, ct])[0]
    under = vo.lines(ok, q, t, o[0], o[1], o[2], o[3], ct, rt, need[rt, ct] - 1)[0]
    assert (at == 1).all() and (under == 2).all()


def test_max_distance_only_marks(small_town):
    z, shape = small_town
    o = sc.observer(20, 25)
    free = vo.viewshed(z, ND, sc.terms(shape), [o])
    near = vo.viewshed(z, ND, sc.terms(shape, max_distance=60.0), [o])
    out = near[0] == 3
    assert out.any() and (near[0] != 3).sum() > 300
    assert np.array_equal(near[0][~out], free[0][~out]) and np.array_equal(near[1][~out].view(np.uint32), free[1][~out].view(np.uint32))
    r, c = np.mgrid[0:shape[0], 0:shape[1]]
    assert np.array_equal(out[0], vo.valid(z, ND) & ((5.0 * (c - 25)) ** 2 + (5.0 * (r - 20)) ** 2 > 3600.0))


def test_straight_lines_are_reciprocal(small_town):
    """Without curvature and with equal heights at both ends, lines along rows, columns and exact diagonals see the same
    cells both ways; other lines sample other cells and are not asserted."""
    z, shape = small_town
    ok, q = vo.heights(z, ND)
    t = sc.terms(shape, curvature=False)
    rng = np.random.default_rng(5)
    ro, co = rng.integers(0, shape[0], 400), rng.integers(0, shape[1], 400)
    for dr, dc in ((0, 1), (1, 0), (1, 1), (1, -1)):
        k = rng.integers(-30, 31, 400)
        rt, ct = ro + k * dr, co + k * dc
        on = (rt >= 0) & (rt < shape[0]) & (ct >= 0) & (ct < shape[1])
        h = vo.units(1.6)
        there = vo.lines(ok, q, t, co[on], ro[on], h, 0, ct[on], rt[on], h)[0]
        back = vo.lines(ok, q, t, ct[on], rt[on], h, 0, co[on], ro[on], h)[0]
        assert np.array_equal(there, back) and {1, 2} <= set(there.tolist())


# ---- formulas --------------------------------------------------------------------------------------------------------------------
def test_the_accumulator_equals_the_floor_formula():
    """The kernel's form of the minor coordinate -- acc starts at n, takes 2 dm per step, and gives or takes 2 n when it leaves
    [0, 2 n) -- against floor((2 i dm + n) / (2 n)) for every n up to 300, every |dm| <= n and every step."""
    for n in range(1, 301):
        dm = np.arange(-n, n + 1)
        acc, m = np.full(dm.shape, n), np.zeros(dm.shape, np.int64)
        for i in range(1, n):
            acc = acc + 2 * dm
            up, down = acc >= 2 * n, acc < 0
            acc, m = acc - 2 * n * up + 2 * n * down, m + up - down
            assert np.array_equal(m, vo.minor(i, dm, n)) and (acc >= 0).all() and (acc < 2 * n).all(), (n, i)
    assert [vo.minor(1, 1, 2), vo.minor(1, -1, 2), vo.minor(1, 3, 6), vo.minor(1, -3, 6)] == [1, 0, 1, 0]      # halves go towards +inf


def test_viewshed_terms():
    g = DSMGrid(0.0, 0.0, 5.0, 2.5, 300, 200)
    assert viewshed_terms(g) == vo.terms(g) == (5.0, 2.5, 256.0 * 0.87 / (2.0 * 6371008.8), math.inf)
    assert viewshed_terms(g, curvature=False, max_distance=1000.0) == vo.terms(g, curvature=False, max_distance=1000.0) == (5.0, 2.5, 0.0, 1e6)
    assert viewshed_terms(g, refraction=0.0, earth_radius=6.4e6)[2] == 256.0 / 1.28e7
    assert viewshed_terms(g, refraction=1.0)[2] == 0.0
    assert vo.units(1.6) == 410 and vo.units(0.5 / 256.0) == 0 and vo.units(1.5 / 256.0) == 2


# ---- argument rejections, Python ---------------------------------------------------------------------------------------------------
def test_python_rejections():
    g = DSMGrid(0.0, 0.0, 5.0, 5.0, 6, 4)
    z = np.zeros((4, 6), np.float32)
    one = [(1, 2)]
    for kw, match in ((dict(refraction=float("nan")), "refraction"), (dict(refraction=1.5), "refraction"), (dict(earth_radius=0.0), "earth_radius"),
                      (dict(earth_radius=float("inf")), "earth_radius"), (dict(max_distance=0.0), "max_distance"), (dict(max_distance=-3.0), "max_distance"),
                      (dict(max_distance=float("nan")), "max_distance"), (dict(max_distance=1e-200), "max_distance")):
        with pytest.raises(ValueError, match=match):
            viewshed_terms(g, **kw)
        if "earth_radius" not in kw:
            with pytest.raises(ValueError, match=match):
                viewshed(z, g, one, **kw)
            with pytest.raises(ValueError, match=match):
                line_of_sight(z, g, one, one, **kw)
    with pytest.raises(ValueError, match="resolution"):
        viewshed_terms(DSMGrid(0.0, 0.0, 0.0, 5.0, 6, 4))
    with pytest.raises(ValueError, match="at most 65536"):
        viewshed_terms(DSMGrid(0.0, 0.0, 5.0, 5.0, 65537, 4))
    with pytest.raises(ValueError, match="too long"):
        viewshed_terms(DSMGrid(0.0, 0.0, 1e6, 1e6, 600, 400))
    assert viewshed_terms(DSMGrid(0.0, 0.0, 1e6, 1e6, 600, 400), curvature=False)[2] == 0.0
    for fn in (lambda **kw: viewshed(z, g, **kw), lambda observers=one, **kw: line_of_sight(z, g, observers, one, **kw)):
        for bad, match in (([], "m >= 1"), ([1, 2], "m >= 1"), ([(1, 2, 3)], "m >= 1"), ([(1.0, 2.0)], "integers"), ([(4, 0)], "lie on"),
                           ([(0, 6)], "lie on"), ([(-1, 0)], "lie on")):
            with pytest.raises(ValueError, match=match):
                fn(observers=bad)
        for kw, match in ((dict(observer_height=-0.1), "observer_height"), (dict(observer_height=float("nan")), "observer_height"),
                          (dict(observer_height=40000.0), "observer_height"), (dict(observer_height=-40000.0, absolute=True), "observer_height"),
                          (dict(observer_height=[1.0, 2.0]), "observer_height"), (dict(target_height=-1.0), "target_height"),
                          (dict(target_height=40000.0), "target_height"), (dict(target_height=float("inf")), "target_height")):
            with pytest.raises(ValueError, match=match):
                fn(observers=one, **kw)
    with pytest.raises(ValueError, match="invalid_observer"):
        viewshed(z, g, one, invalid_observer="skip")
    with pytest.raises(ValueError, match="shape"):
        viewshed(np.zeros((3, 3), np.float32), g, one)
    with pytest.raises(ValueError, match="shape"):
        line_of_sight(np.zeros((3, 3), np.float32), g, one, one)
    with pytest.raises(ValueError, match="one cell per line"):
        line_of_sight(z, g, one, [(0, 0), (1, 1)])
    with pytest.raises(ValueError, match="lie on"):
        line_of_sight(z, g, one, [(0, 6)])
    for kw, match in ((dict(points=[(4, 0)]), "lie on"), (dict(points=[]), "m >= 1"), (dict(points=one, height=-1.0), "height"),
                      (dict(points=one, height=[1.0, 2.0]), "height"), (dict(points=one, max_distance=0.0), "max_distance")):
        with pytest.raises(ValueError, match=match):
            intervisibility(z, g, **kw)
    with pytest.raises(ValueError, match="shape"):
        intervisibility(np.zeros((3, 3), np.float32), g, one)
    for bad in (np.zeros((4, 6), np.uint8), np.zeros((2, 4, 6), np.float32), np.zeros((0, 4, 6), np.uint8)):
        with pytest.raises(ValueError, match="seen is"):
            visibility_count(bad)


# ---- argument rejections, C --------------------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_a_gpu(lib):
    from satmvs_amd import _lib
    MB = 1 << 20
    at = lambda i: C.c_void_p(i * MB)                        # noqa: E731  (made-up pointers a megabyte apart: nothing is dereferenced)
    gw, gh = 90, 70
    nbytes = lib.smvs_dsm_viewshed_workspace_bytes(gw, gh, 2)
    assert 4 * gw * gh <= nbytes < 4 * gw * gh + 256 and nbytes == lib.smvs_dsm_viewshed_workspace_bytes(gw, gh, 64)
    for size in ((0, 5, 1), (5, 0, 1), (-1, 5, 1), (65537, 4, 1), (4, 65537, 1), (65536, 32768, 1), (5, 5, 0), (5, 5, 65), (5, 5, -1)):
        assert lib.smvs_dsm_viewshed_workspace_bytes(*size) == 0, size
    assert lib.smvs_dsm_viewshed_workspace_bytes(65536, 32767, 64) > 0
    good = [3, 4, 410, 0, 0, 89, 69, -5, 1, 2560]
    inf, nan = float("inf"), float("nan")

    def shed(dsm=at(1), gw=gw, gh=gh, xres=5.0, yres=5.0, c256=1.7e-5, r2max=inf, obs=good, n=2, seen=at(2), above=at(3), status=at(4), ws=at(5), nbytes=nbytes):
        host = None if obs is None else (C.c_int * len(obs))(*obs)
        _lib.call("smvs_dsm_viewshed", dsm, gw, gh, -999.0, xres, yres, c256, r2max, host, n, seen, above, status, ws, nbytes, None)

    def los(dsm=at(1), gw=gw, gh=gh, xres=5.0, yres=5.0, c256=1.7e-5, r2max=inf, pairs=at(2), n=1000, seen=at(3), above=at(4)):
        _lib.call("smvs_dsm_los", dsm, gw, gh, -999.0, xres, yres, c256, r2max, pairs, n, seen, above, None)

    def second(*o):
        return dict(obs=good[:5] + list(o))

    scalars = [(dict(gw=0), "non-positive grid"), (dict(gh=-2), "non-positive grid"), (dict(gw=65536, gh=32768), "below 2\\^31"),
               (dict(gw=65537, gh=1), "at most 65536"), (dict(gw=1, gh=65537), "at most 65536"),
               (dict(xres=0.0), "xres and yres"), (dict(yres=-5.0), "xres and yres"), (dict(xres=nan), "xres and yres"), (dict(yres=inf), "xres and yres"),
               (dict(c256=-1e-9), "c256 must be"), (dict(c256=nan), "c256 must be"), (dict(c256=inf), "c256 must be"),
               (dict(c256=1.001 * 2.0 ** 30 / (450.0 ** 2 + 350.0 ** 2)), "below 2\\^30"), (dict(c256=0.0, xres=1e200), "below 2\\^30"),
               (dict(r2max=0.0), "r2max"), (dict(r2max=-1.0), "r2max"), (dict(r2max=nan), "r2max"), (dict(r2max=-inf), "r2max")]
    bad = [(fn, kw, match) for fn in (shed, los) for kw, match in scalars]
    bad += [(shed, dict(dsm=None), "null pointer"), (shed, dict(obs=None), "null pointer"), (shed, dict(seen=None), "null pointer"),
            (shed, dict(status=None), "null pointer"), (shed, dict(ws=None), "null pointer"),
            (shed, dict(n=0), "n_obs must be"), (shed, dict(n=-1), "n_obs must be"), (shed, dict(n=65, obs=good[:5] * 65), "n_obs must be"),
            (shed, second(90, 0, 0, 0, 0), "off the"), (shed, second(-1, 0, 0, 0, 0), "off the"), (shed, second(0, 70, 0, 0, 0), "off the"),
            (shed, second(0, -1, 0, 0, 0), "off the"), (shed, second(0, 0, 0, 2, 0), "mode must be"), (shed, second(0, 0, 0, -1, 0), "mode must be"),
            (shed, second(0, 0, -1, 0, 0), "eye must be"), (shed, second(0, 0, 2 ** 23 + 1, 0, 0), "eye must be"), (shed, second(0, 0, 2 ** 23 + 1, 1, 0), "eye must be"),
            (shed, second(0, 0, -2 ** 23 - 1, 1, 0), "eye must be"), (shed, second(0, 0, 0, 0, -1), "tgt must be"), (shed, second(0, 0, 0, 1, 2 ** 23 + 1), "tgt must be"),
            (shed, dict(nbytes=nbytes - 1), "workspace too small"), (shed, dict(nbytes=0), "workspace too small"),
            (shed, dict(seen=at(1)), "must not overlap"), (shed, dict(above=at(1)), "must not overlap"), (shed, dict(status=at(2)), "must not overlap"),
            (shed, dict(ws=at(3)), "must not overlap"), (shed, dict(ws=at(1)), "must not overlap"), (shed, dict(above=at(2)), "must not overlap"),
            (shed, dict(status=C.c_void_p(5 * MB + nbytes - 1)), "must not overlap"), (shed, dict(seen=C.c_void_p(MB + 4 * gw * gh - 1)), "must not overlap"),
            (los, dict(dsm=None), "null pointer"), (los, dict(pairs=None), "null pointer"), (los, dict(seen=None), "null pointer"),
            (los, dict(n=0), "n_pairs must be"), (los, dict(n=-5), "n_pairs must be"),
            (los, dict(pairs=at(1)), "must not overlap"), (los, dict(seen=at(1)), "must not overlap"), (los, dict(above=at(2)), "must not overlap"),
            (los, dict(above=at(3)), "must not overlap"), (los, dict(seen=C.c_void_p(2 * MB + 27999)), "must not overlap")]
    for fn, kw, match in bad:
        with pytest.raises(_lib.SatMVSNativeError, match=match):
            fn(**kw)


# ---- planted errors: the comparison of the GPU file has to report each ---------------------------------------------------------
def _planted_scene(plant):
    if plant in ("strict", "float quotients"):                # grazing at every sample
        return sc.tilted((5, 60)), sc.terms((5, 60), curvature=False), [sc.observer(r, 0, eye_m=0.0) for r in range(5)]
    if plant == "ends occlude":                               # an absolute eye below its own cell
        return sc.town((40, 50), 32), sc.terms((40, 50)), [sc.observer(20, 25, eye_m=100.0, mode=1), sc.observer(3, 4)]
    if plant in ("no target drop", "drop added"):
        return sc.town((40, 50), 33), sc.terms((40, 50), (30.0, 30.0)), sc.corners_and_centre((40, 50))
    return sc.town((41, 40), 34, voids=0.15), sc.terms((41, 40)), sc.corners_and_centre((41, 40))


@pytest.mark.parametrize("plant", vo.PLANTS)
def test_planted_errors_are_reported(plant):
    z, t, observers = _planted_scene(plant)
    good = vo.viewshed(z, ND, t, observers)
    wrong = vo.viewshed(z, ND, t, observers, plant)
    for k in (0, 1):
        sc.compare(vo.viewshed(z, ND, t, observers)[k], good[k], "the statement against itself")
    with pytest.raises(AssertionError, match=r"cells differ, the first at \(\d+, \d+, \d+\)"):
        sc.compare(wrong[0], good[0], plant)
    if plant not in ("strict", "ends occlude", "float quotients"):       # a cell hidden at a tie needs 0 units more: the bits of a seen one
        with pytest.raises(AssertionError, match=r"cells differ, the first at \(\d+, \d+, \d+\)"):
            sc.compare(wrong[1], good[1], plant)
