"""The seeded flood without a device: the two Python statements of the rule (tests/dsm_watershed_oracle.py) against each other on
the whole case matrix, closed forms, the identities of geodesic reconstruction, the tie to the hydrology's flood, every Python
and C argument rejection, and the planted errors the GPU file's comparison has to name."""
import ctypes as C

import numpy as np
import pytest

import dsm_hydro_oracle as ho
import dsm_label_oracle as lo
import dsm_watershed_oracle as wo
import dsm_watershed_scene as sc
from dsm_testkit import lib, same_bits                       # noqa: F401

NODATA = sc.NODATA


def _grid(gh, gw, xres=5.0, yres=5.0):
    from satmvs_amd import dsm
    return dsm.DSMGrid(400000.0, 3500000.0, xres, yres, gw, gh)


_shared = {}


def _chain(case):
    if case not in _shared:
        args = sc.case(case)
        _shared[case] = (args, wo.chain(**args))
    return _shared[case]


# ---- the two statements ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.ALL_CASES, ids=sc.case_id)
def test_the_two_statements_agree(case):
    args, sweeps = _chain(case)
    assert wo.differing(wo.chain(heap=True, **args), sweeps) == []


def test_the_scenes_hold_what_they_are_for():
    _, domain = _chain(("domain",))
    assert domain["n_unreached"] == 40 * 35 and (domain["backlink"][:, 35:] == 255).all() and (domain["keys"][:, 35:] == wo.INF_KEY).all()
    assert (domain["keys"][:, 33:35] == wo.INVALID_KEY).all() and (domain["surface"][:, 33:] == NODATA).all()
    _, spiral = _chain(("spiral",))
    assert spiral["steps"].max() > 4000 and spiral["n_unreached"] == 0 and (spiral["backlink"] == 0).sum() == 1
    args, none = _chain(("town", 0.05, 1, 0, "none"))
    assert none["n_seeds"] == 0 and none["n_unreached"] == int(ho.valid(args["z"]).sum()) > 70000 and (none["backlink"] == 255).all()
    args, quantum = _chain(("quantum", 1))
    assert quantum["keys"][12, 31] == wo.INVALID_KEY and quantum["keys"][25, 8] == wo.INVALID_KEY and quantum["keys"][12, 30] < wo.INF_KEY
    args, marker = _chain(("marker", -1, 700))
    q, qm = ho.quanta(args["z"]), ho.quanta(args["marker"])
    seeds = ho.valid(args["z"]) & ho.valid(args["marker"])
    assert all((seeds & cmp).sum() > 20 for cmp in (qm > q, qm < q, qm == q)) and (np.isnan(args["marker"]).sum() > 20)
    big = [wo.unpack(_chain(c)[1]["keys"])[0] for c in sc.TOWN_CASES[3:]]
    assert big[0].max() > 2 ** 24 - 2 ** 17 and (big[1] == ho.quanta(sc.case(sc.TOWN_CASES[4])["z"])).all()


# ---- closed forms ----------------------------------------------------------------------------------------------------------------
def test_two_cones_peaks_on_either_side_of_both_prominences():
    s, z = sc.CONES, sc.two_cones()
    a, b = (s["row"], s["col_a"]), (s["row"], s["col_b"])
    eps = 1.0 / 256.0
    for h, want_a, want_b in ((0.5, True, True), (6.0 - eps, True, True), (6.0, True, True), (6.0 + eps, True, False), (19.0, True, False),
                              (20.0, True, False), (20.0 + eps, False, False), (29.0, False, False)):
        labels, n, table, dome = wo.peaks(z, h)
        assert (labels[a] > 0) == want_a and (labels[b] > 0) == want_b and n == 1 + want_a + want_b, h
        wall = labels[0, s["wall_col"]]
        assert wall > 0 and (labels[:, s["wall_col"]:] == wall).all() and table["area"][wall - 1] == s["gh"] * (s["gw"] - s["wall_col"])
        # the reconstruction at a top: the best over the seeds of min(the seed's marker, the lowest pass on the way)
        H = wo.h_quanta(h) / 256.0
        under_a, under_b = max(20.0 - H, min(30.0 - H, 0.0)), max(14.0 - H, min(20.0 - H, 8.0), min(30.0 - H, 0.0))
        assert dome[a] == np.float32(20.0 - under_a) and dome[b] == np.float32(14.0 - under_b) and dome[0, 0] == 0 and dome[0, -1] == np.float32(H)
        assert table["height"].tolist() == [30.0] + [20.0] * want_a + [14.0] * want_b and table["first"][0].tolist() == [0, s["wall_col"]]


def test_two_cones_part_on_the_saddles_bisector():
    s, z = sc.CONES, sc.two_cones()
    tops, n, _, _ = wo.peaks(z, 2.0)
    assert n == 3
    seg, level = wo.watershed(z, tops)
    la, lb = tops[s["row"], s["col_a"]], tops[s["row"], s["col_b"]]
    rows = slice(s["row"] - 3, s["row"] + 4)
    assert (seg[rows, 2:s["saddle_col"]] == la).all() and (seg[rows, s["saddle_col"] + 1:s["col_b"] + 10] == lb).all()
    assert np.isin(seg[rows, s["saddle_col"]], (la, lb)).all() and (seg > 0).all()
    assert (seg[rows, s["saddle_col"]] == lb).all()          # the rule itself: level neighbours tie, the lowest k is E
    assert same_bits(level[tops > 0], z[tops > 0]) and (level >= z).all()
    assert level[0, 0] == 0.0 and level[s["row"], s["saddle_col"]] == s["saddle"]
    # with the pits as markers and peaks_up=False the same surface negated gives the same segments
    seg_down, _ = wo.watershed(-z, tops, peaks_up=False)
    assert np.array_equal(seg_down, seg)


def test_a_plateau_gets_one_marker_and_a_sub_peak_one_quantum_lower_is_kept():
    z = np.zeros((9, 30), np.float32)
    z[2:7, 3:12] = 10.0                                       # a plateau top
    z[4, 20], z[4, 24] = 10.0, np.float32(10.0 - 1.0 / 256.0)   # a top, and a sub-peak one quantum under it across a saddle at 0 m
    z[4, 21:24] = (6.0, 2.0, 6.0)
    labels, n, table, dome = wo.peaks(z, 2.0)
    assert n == 3 and table["area"].tolist() == [45, 1, 1] and table["first"].tolist() == [[2, 3], [4, 20], [4, 24]]
    assert same_bits(table["height"], np.array([10.0, 10.0, 10.0 - 1.0 / 256.0], np.float32))
    assert dome[4, 22] == 0.0 and dome[4, 24] == 2.0 and dome[4, 21] == 0.0 and dome[4, 23] == 0.0
    assert wo.peaks(z, 8.0 - 1.0 / 256.0)[1] == 3 and wo.peaks(z, 8.0)[1] == 2   # it stands 8 m less one quantum over its saddle at 2 m
    assert wo.peaks(z, 65536.0)[1] == 2                       # two tops of one height: neither has higher ground, both stay at any h
    assert wo.peaks(z, 2.0, min_height=10.0 - 0.5 / 256.0)[1] == 2


# ---- identities ------------------------------------------------------------------------------------------------------------------
IDENTITY_CASES = [c for c in sc.SMALL_CASES if c[0] in ("grid", "marker", "quantum")] + sc.TOWN_CASES[:2]


@pytest.mark.parametrize("case", IDENTITY_CASES, ids=sc.case_id)
def test_identities_of_the_reconstruction(case):
    args, got = _chain(case)
    z, pol = args["z"], args["polarity"]
    v, g, seed, s = wo.setup(**args)
    w, d, reached = wo.unpack(got["keys"])
    # between the surface and the clamped marker, in the flood's own orientation
    assert (w[reached] >= g[reached]).all() and (w[seed] <= s[seed]).all() and (s[seed] >= g[seed]).all()
    out = got["surface"]
    ok = reached & v
    assert same_bits(out[ok & (w == g)], z[ok & (w == g)]) and (out[~ok] == NODATA).all()
    with np.errstate(invalid="ignore"):
        assert (pol * out[ok].astype(np.float64) >= pol * z[ok].astype(np.float64)).all()
    # idempotent: the result as the marker of the same surface changes nothing
    if np.abs(w[ok]).max() <= 2 ** 23:                        # (an offset of 2^24 lifts the result out of a marker's range)
        again = wo.chain(z, out, args["domain"], pol, 0)
        assert np.array_equal(wo.unpack(again["keys"])[0][ok], w[ok]) and same_bits(again["surface"][ok], out[ok])
    # erosion is the negated dilation of the negated grids
    flip = lambda a: np.where(ho.valid(a), -a, a).astype(np.float32)      # noqa: E731
    other = wo.chain(flip(z), flip(args["marker"]), args["domain"], -pol, args["offset"])
    assert np.array_equal(other["keys"], got["keys"]) and np.array_equal(other["backlink"], got["backlink"])
    assert np.array_equal(np.where(ok, -other["surface"], NODATA), out)     # by value: a computed 0 m is +0.0 either way
    # the links strictly lower the key, every root is a seed at its own level, every reached cell ends at a root
    link = got["backlink"]
    nk = wo.neighbour_keys(got["keys"])
    linked = (link >= 1) & (link <= 8)
    k = np.where(linked, link.astype(np.int64) - 1, 0)
    assert (np.take_along_axis(nk, k[None], 0)[0][linked] < got["keys"][linked]).all()
    assert (seed[link == 0]).all() and (got["keys"][link == 0] == wo.pack(s, 0)[link == 0]).all() and ((link == 255) == ~ok).all()
    root = wo.roots_of(link)
    assert (root[ok] >= 0).all() and (link.reshape(-1)[root[ok]] == 0).all()


@pytest.mark.parametrize("polarity", [1, -1])
def test_h_maxima_with_the_largest_h_is_flat_per_component(polarity):
    z = sc.case(("town", 0.3, 1, 0, "random"))["z"]
    got = wo.chain(z, z, None, polarity, sc.BIG)
    w, _, reached = wo.unpack(got["keys"])
    v = ho.valid(z)
    comp, n = lo.label(v, 8)
    assert n > 3 and reached[v].all()
    g = polarity * ho.quanta(z)
    for k in range(1, n + 1):
        cells = comp == k
        assert (w[cells] == g[cells].min() + sc.BIG).all()


@pytest.mark.parametrize("case", ho.RANDOM_CASES[::3] + [(33, 65, 9, 0.0, 6)], ids=str)
def test_seeded_at_the_outlets_it_is_the_hydrology_flood(case):
    """Seeds = the hydrology's outlets at their own height, voids as walls: on a grid without interior voids the keys are the
    flood's, word for word, and the surface is fill_depressions' filled surface."""
    gh, gw, seed, voids, levels = case
    z = ho.hills(gh, gw, seed, 0.0, levels)
    v = ho.valid(z)
    assert v.all()
    marker = np.where(ho.outlets(v), z, NODATA).astype(np.float32)
    got = wo.chain(z, marker, None, 1, 0)
    w, d, _ = ho.keys_heap(z)
    assert np.array_equal(got["keys"], ho.pack(w, d, v))
    assert same_bits(got["surface"], ho.filled_of(z, w, d, v)[0]) and np.array_equal(got["steps"], d.astype(np.int32))


def test_the_terrace_scene_is_what_the_end_to_end_test_needs():
    """The oracle alone: two objects, six segments in raster order, borders within one cell of the saddles."""
    above = sc.terrace()
    grid = _grid(*above.shape)
    objects, stats = lo.objects(above, grid)
    assert len(stats["area"]) == 2
    labels, n, table = wo.split_objects(above, grid)
    want, loose = sc.terrace_expected()
    assert n == 6 and np.array_equal((labels > 0), objects > 0)
    assert np.array_equal(labels[~loose], want[~loose])
    assert all(labels[r, c] in (want[r, c], want[r, c - 1]) for r, c in np.argwhere(loose))
    assert table["object"].tolist() == [1, 1, 1, 1, 2, 2] and table["area"].sum() == (objects > 0).sum()
    assert same_bits(table["max"], np.array([9, 9, 9, 9, 8, 7.5], np.float32))
    # one quantum more than the lower dome stands over the pass (2.25 m), and the trees stay one segment; the four ridges are
    # of one height, so none has higher ground and all stay at any h
    assert wo.split_objects(above, grid, h=2.25)[1] == 6 and wo.split_objects(above, grid, h=2.25 + 1.0 / 256.0)[1] == 5
    assert wo.split_objects(above, grid, h=100.0)[1] == 5


# ---- rejections ------------------------------------------------------------------------------------------------------------------
def test_python_rejections_need_no_device():
    from satmvs_amd import dsm
    gh, gw = 6, 7
    z = np.zeros((gh, gw), np.float32)
    lab = np.zeros((gh, gw), np.int32)
    grid = _grid(gh, gw)
    for kw in (dict(marker=z[:-1]), dict(marker=z.astype(np.float64)), dict(surface=z.astype(np.float64)), dict(surface=z[0]), dict(method="opening"),
               dict(mask=np.ones((gh, gw), np.float32)), dict(mask=np.ones((gh, gw + 1), bool)), dict(batch=0), dict(batch=4097), dict(batch=1.5)):
        with pytest.raises(ValueError):
            dsm.reconstruct(**{**dict(marker=z, surface=z), **kw})
    for fn in (dsm.h_maxima, dsm.h_minima, lambda *a, **k: dsm.peaks(*a, **k)):
        for h in (0.0, 1.0 / 512.0, -1.0, 65536.0 + 1.0 / 256.0, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                fn(z, h)
        with pytest.raises(ValueError):
            fn(z.astype(np.float64), 1.0)
        with pytest.raises(ValueError):
            fn(z, 1.0, mask=np.ones((gh + 1, gw), bool))
    assert dsm._h_quanta(1.0 / 256.0) == 1 and dsm._h_quanta(65536.0) == 2 ** 24 and dsm._h_quanta(2.0) == 512 and dsm._h_quanta(0.3) == 76
    for kw in (dict(connectivity=6), dict(min_height=float("nan")), dict(grid=_grid(gh, gw + 1))):
        with pytest.raises(ValueError):
            dsm.peaks(z, 1.0, **kw)
    for kw in (dict(markers=lab[:-1]), dict(markers=lab.astype(np.int64)), dict(markers=lab.astype(np.float32)), dict(surface=z.astype(np.float64)),
               dict(mask=np.ones((gh, gw), np.float64))):
        with pytest.raises(ValueError):
            dsm.watershed(**{**dict(surface=z, markers=lab), **kw})
    for kw in (dict(h=0.0), dict(grid=_grid(gh + 1, gw)), dict(connectivity=5), dict(min_area_m2=-1.0), dict(min_height=float("inf")), dict(above=z.astype(np.float64))):
        with pytest.raises(ValueError):
            dsm.split_objects(**{**dict(above=z, grid=grid), **kw})
    for kw in (dict(radius=0), dict(radius=257), dict(dsm=z.astype(np.float64))):
        with pytest.raises(ValueError):
            dsm.open_by_reconstruction(**{**dict(dsm=z, radius=2), **kw})


def test_native_rejections_need_no_device(lib):              # noqa: F811
    """SMVS_ERR_ARG before any HIP call: made-up pointers a megabyte apart, nothing is dereferenced."""
    from satmvs_amd import _lib
    MB = 1 << 20
    at = lambda i: C.c_void_p(i * MB)                        # noqa: E731
    gw, gh = 9, 7
    n = gw * gh
    size = lib.smvs_dsm_seed_workspace_bytes
    ws_bytes = size(gw, gh)
    assert ws_bytes == 4096 * 4 + 256 and size(4096, 4096) == 4096 * 4 + 4 * 65536
    assert size(0, 5) == 0 and size(5, -1) == 0 and size(2 ** 15, 2 ** 15) == 0 and size(2 ** 30 - 1, 1) > 0 and size(2 ** 30, 1) == 0

    def begin(dsm=at(1), marker=at(2), domain=at(3), gw=gw, gh=gh, polarity=1, offset=0, keys=at(4), count=at(5), ws=at(6), nbytes=ws_bytes):
        _lib.call("smvs_dsm_seed_begin", dsm, marker, domain, gw, gh, -999.0, polarity, offset, keys, count, ws, nbytes, None)

    def rounds(dsm=at(1), gw=gw, gh=gh, polarity=1, keys=at(4), k=8, status=at(5), ws=at(6), nbytes=ws_bytes):
        _lib.call("smvs_dsm_seed_rounds", dsm, gw, gh, -999.0, polarity, keys, k, status, ws, nbytes, None)

    def read(dsm=at(1), marker=at(2), domain=at(3), gw=gw, gh=gh, polarity=1, offset=0, keys=at(4), surface=at(7), steps=at(8), link=at(9), count=at(5),
             ws=at(6), nbytes=ws_bytes):
        _lib.call("smvs_dsm_seed_read", dsm, marker, domain, gw, gh, -999.0, polarity, offset, keys, surface, steps, link, count, ws, nbytes, None)

    def rejected(call, match, **kw):
        with pytest.raises(_lib.SatMVSNativeError, match=match):
            call(**kw)

    for name in ("dsm", "marker", "keys", "count", "ws"):
        rejected(begin, "null pointer", **{name: None})
    for name in ("dsm", "keys", "status", "ws"):
        rejected(rounds, "null pointer", **{name: None})
    for name in ("dsm", "marker", "keys", "ws"):
        rejected(read, "null pointer", **{name: None})
    for call in (begin, rounds, read):
        for polarity in (0, 2, -2):
            rejected(call, "polarity must be \\+1 or -1", polarity=polarity)
        rejected(call, "non-positive grid", gw=0)
        rejected(call, "non-positive grid", gh=-3)
        rejected(call, "below 2\\^30", gw=2 ** 15, gh=2 ** 15)
        rejected(call, "below 2\\^30", gw=2 ** 30, gh=1)
        rejected(call, "workspace too small", nbytes=ws_bytes - 1)
        rejected(call, "workspace aliases keys", ws=C.c_void_p(4 * MB + n * 8 - 1))
    for call in (begin, rounds):
        rejected(call, "keys aliases dsm", keys=at(1))
    for call in (begin, read):
        for offset in (2 ** 25 + 1, -2 ** 25 - 1, 2 ** 31 - 1, -2 ** 31):
            rejected(call, "offset must be within", offset=offset)
    rejected(begin, "keys aliases marker", keys=C.c_void_p(2 * MB + n * 4 - 1))
    rejected(begin, "keys aliases domain", keys=C.c_void_p(3 * MB + n - 1))
    rejected(read, "surface aliases marker", surface=C.c_void_p(2 * MB + n * 4 - 1))
    rejected(read, "backlink aliases domain", link=C.c_void_p(3 * MB + n - 1))
    rejected(begin, "n_seeds aliases keys", count=C.c_void_p(4 * MB + n * 8 - 1))
    rejected(rounds, "status aliases keys", status=C.c_void_p(4 * MB + 8))
    rejected(read, "surface aliases dsm", surface=at(1))
    rejected(read, "level_steps aliases surface", steps=C.c_void_p(7 * MB + n * 4 - 1))
    rejected(read, "backlink aliases keys", link=C.c_void_p(4 * MB + n * 8 - 1))
    rejected(read, "n_unreached aliases backlink", count=C.c_void_p(9 * MB + n - 1))
    for k in (0, -1, 4097):
        rejected(rounds, "rounds must be in 1 .. 4096", k=k)
    # what is allowed: null domain and outputs, the extreme offsets, and inputs that share their bytes (the DSM as its own marker)
    for call, kw in ((begin, dict(domain=None, marker=at(1), offset=2 ** 25)), (begin, dict(offset=-2 ** 25, polarity=-1)), (rounds, dict(polarity=-1)),
                     (read, dict(domain=None, surface=None, steps=None, link=None, count=None, marker=at(1)))):
        rejected(call, "workspace too small", nbytes=0, **kw)


# ---- the planted errors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(wo.PLANTED))
def test_the_comparison_reports_a_planted_error(name):
    """differing(), the comparison of the GPU file, with a wrong implementation standing in for the device: it names the output
    and the first cell that differs, on at least one of the cases both files run."""
    found = []
    for case in sc.SMALL_CASES:
        args, want = _chain(case)
        found = wo.differing(wo.chain(**args, **wo.PLANTED[name]), {k: want[k] for k in wo.OUT})
        if found:
            break
    assert found and all(line[0] in wo.OUT and isinstance(line[1], int) and line[1] > 0 and len(line[2]) == 2 for line in found), (name, found)
    assert wo.differing(want, want) == []
