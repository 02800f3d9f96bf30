"""The stack fusion's rules without a GPU: the two numpy statements of tests/dsm_stack_oracle.py against each other over the
whole case matrix (tests/dsm_stack_scene.py), closed forms, the linear median against dsm._quantile_value, every rejection of the
Python layer and of the two C entries (before any HIP call: the pointers are never followed), and planted errors that the GPU
file's comparison has to report."""
import ctypes as C

import numpy as np
import pytest
import torch

import dsm_stack_oracle as so
import dsm_stack_scene as sc
from dsm_testkit import lib, same as _same, same_bits, valid  # noqa: F401  (fixture)
from satmvs_amd import dsm
from satmvs_amd.dsm import DSMGrid

ND = sc.ND
ERR_ARG = 1                                                                # SMVS_ERR_ARG


def _equal(got, want, names, what):
    for g, w, name in zip(got, want, names):
        _same(np.ascontiguousarray(g), np.ascontiguousarray(w), (what, name))


@pytest.fixture(scope="module")
def matrix():
    return sc.cases()


# ---- the two statements ----------------------------------------------------------------------------------------------------------
def test_the_select_statements_agree(matrix):
    deepest = 0
    for i, (name, layers, gw, gh, centre) in enumerate(matrix):
        n = 1 + i % 8                                                      # 1 .. 8 levels a call, every level in some call
        levels = (sc.LEVELS[i % 8:] + sc.LEVELS[:i % 8])[:n]
        for lv, c in ((levels, None), (sc.LEVELS, None), (levels, centre), (sc.LEVELS[:5], centre)):
            a = so.select_cells(layers, ND, lv, c, gw, gh)
            b = so.select_sorted(layers, ND, lv, c, gw, gh)
            _equal(a, b, so.SELECT_NAMES, (name, len(lv), c is not None))
        count = so.select_sorted(layers, ND, [(1, 2)], None, gw, gh)[0]
        deepest = max(deepest, int(count.max()))
        if gw * gh > 200 and "full" not in name:
            assert count.min() == 0 and len(np.unique(count)) >= 3, name      # m varies, down to cells no layer covers
    assert deepest == 64                                                   # a column of all 64 layers


def test_the_fuse_statements_agree(matrix):
    for name, layers, gw, gh, _ in matrix:
        for kmad, floor, min_count in sc.FUSE_PARAMS:
            a = so.fuse_cells(layers, ND, kmad, floor, min_count, gw, gh)
            b = so.fuse_sorted(layers, ND, kmad, floor, min_count, gw, gh)
            _equal(a, b, so.FUSE_NAMES, (name, kmad, floor, min_count))
    for layers, gw, gh in (sc.zeros_case(), sc.edge_case()):
        for kmad, floor, min_count in sc.FUSE_PARAMS + [(0.0, 2.0, 1), (0.0, float(np.nextafter(2.0, 0.0)), 1)]:
            _equal(so.fuse_cells(layers, ND, kmad, floor, min_count, gw, gh), so.fuse_sorted(layers, ND, kmad, floor, min_count, gw, gh),
                   so.FUSE_NAMES, (gw, kmad, floor, min_count))
        _equal(so.select_cells(layers, ND, sc.LEVELS, None, gw, gh), so.select_sorted(layers, ND, sc.LEVELS, None, gw, gh), so.SELECT_NAMES, gw)


def test_the_matrix_holds_what_it_promises(matrix):
    """Every kind of void, both zeros, exact ties, deviations that round to +Inf, and m on both sides of every min_count."""
    seen = dict(nan=False, inf=False, nodata=False, neg0=False, pos0=False, tie=False, inf_dev=False, empty=False, odd=False, even=False)
    for name, layers, gw, gh, centre in matrix:
        for z, _, _ in layers:
            seen["nan"] |= bool(np.isnan(z).any())
            seen["inf"] |= bool(np.isinf(z).any())
            seen["nodata"] |= bool((z == ND).any())
            seen["neg0"] |= bool(((z == 0) & np.signbit(z)).any())
            seen["pos0"] |= bool(((z == 0) & ~np.signbit(z)).any())
        Z, ok = so.stack(layers, ND, gw, gh)
        if len(layers) > 1:
            keys = np.where(ok, Z, np.nan)
            seen["tie"] |= bool((np.sort(keys, axis=0)[1:] == np.sort(keys, axis=0)[:-1]).any())
        seen["inf_dev"] |= bool((np.isinf(so.deviations(Z, centre)) & ok & np.isfinite(centre)[None]).any())
        m = ok.sum(axis=0)
        seen["empty"] |= bool((m == 0).any())
        seen["odd"] |= bool(((m % 2 == 1) & (m > 1)).any())
        seen["even"] |= bool(((m % 2 == 0) & (m > 0)).any())
    assert all(seen.values()), seen
    layers, gw, gh = sc.edge_case()
    Z, ok = so.stack(layers, ND, gw, gh)
    med = so.fuse_sorted(layers, ND, 0.0, 0.0, 1, gw, gh)[1]
    assert np.isinf(so.deviations(Z, med)[0, 0, 5]) and ok[0, 0, 5]           # -3e38 against a median of 3e38


# ---- closed forms ----------------------------------------------------------------------------------------------------------------
def test_constant_stacks():
    for K in (1, 2, 5, 64):
        z = np.full((3, 4), 12.25, np.float32)
        layers = [(z, 0, 0)] * K
        count, lo, hi = so.select_sorted(layers, ND, sc.LEVELS, None, 4, 3)
        assert (count == K).all() and (lo == 12.25).all() and (hi == 12.25).all()
        out, median, mad, count, n_in, members, inliers = so.fuse_sorted(layers, ND, 0.0, 0.0, 1, 4, 3)
        assert (out == 12.25).all() and (median == 12.25).all() and (mad == 0).all() and (n_in == K).all()
        full = np.uint64((1 << K) - 1).astype(np.int64) if K < 64 else np.int64(-1)
        assert (members == full).all() and (inliers == full).all()


def test_one_layer_comes_back_bit_for_bit():
    z = sc.heights((9, 31), 5)
    want = np.where(valid(z, ND), z, ND)
    assert np.signbit(want[want == 0]).any() and (want == sc.BIG).any()
    for kmad, floor, min_count in sc.FUSE_PARAMS[:3]:
        got = so.fuse_sorted([(z, 0, 0)], ND, kmad, floor, min(min_count, 1), 31, 9)
        assert same_bits(got[0], want), (kmad, floor)
        assert np.array_equal(got[4], valid(z, ND).astype(np.uint8))
    count, lo, hi = so.select_sorted([(z, 0, 0)], ND, sc.LEVELS, None, 31, 9)
    assert all(same_bits(lo[j], want) and same_bits(hi[j], want) for j in range(len(sc.LEVELS)))


def test_a_permutation_of_the_layers_leaves_select_unchanged(matrix):
    for name, layers, gw, gh, centre in matrix[2:7]:
        order = np.random.default_rng(3).permutation(len(layers))
        mixed = [layers[k] for k in order]
        for c in (None, centre):
            _equal(so.select_sorted(mixed, ND, sc.LEVELS, c, gw, gh), so.select_sorted(layers, ND, sc.LEVELS, c, gw, gh), so.SELECT_NAMES, name)
        a = so.fuse_sorted(layers, ND, 2.0, 0.25, 1, gw, gh)
        b = so.fuse_sorted(mixed, ND, 2.0, 0.25, 1, gw, gh)
        _equal(a[1:5], b[1:5], so.FUSE_NAMES[1:5], name)                      # median, mad and the counts; the sum has an order


def test_an_odd_stack_has_an_inlier_at_distance_zero(matrix):
    for name, layers, gw, gh, _ in matrix:
        out, median, mad, count, n_in, members, inliers = so.fuse_sorted(layers, ND, 0.0, 0.0, 1, gw, gh)
        odd = count % 2 == 1
        assert (n_in[odd] >= 1).all(), name
        Z, ok = so.stack(layers, ND, gw, gh)
        at_median = (ok & (Z == median[None])).sum(axis=0)
        assert np.array_equal(n_in[odd], at_median[odd].astype(np.uint8)), name      # thr = 0: exactly the layers on the median
        assert (n_in[(count > 0) & ~odd] == at_median[(count > 0) & ~odd]).all(), name
        assert ((n_in == 0) & (count > 0)).any() or gw * gh < 200, name               # even m, a != b: out is the median
        assert same_bits(out[(n_in == 0) & (count > 0)], median[(n_in == 0) & (count > 0)])


def test_the_linear_median_is_quantile_value():
    """a + (b - a) (rem / 2) of the oracle against dsm._quantile_value(..., "linear") at q = 1/2, on hard pairs."""
    rng = np.random.default_rng(9)
    a = np.concatenate([rng.normal(0, 1e3, 4000), [-0.0, 0.0, -0.0, 3e38, -3e38, 1e-40, 1.0]]).astype(np.float32)
    b = np.concatenate([rng.normal(0, 1e3, 4000), [-0.0, -0.0, 0.0, 3e38, 3e38, 3e-40, np.nextafter(np.float32(1), np.float32(2))]]).astype(np.float32)
    a, b = np.minimum(a, b), np.maximum(a, b)
    for m in (1, 2, 3, 4, 63, 64):
        lo_rank, hi_rank, rem, den = dsm.quantile_ranks(np.array([m], np.int32), [(1, 2)])
        assert lo_rank[0, 0] == (m - 1) // 2 and hi_rank[0, 0] == (m - 1) // 2 + (m - 1) % 2 and rem[0, 0] == (m - 1) % 2 and den[0] == 2
        hi = b if (m - 1) % 2 else a
        want = dsm._quantile_value(torch.from_numpy(a), torch.from_numpy(hi), torch.full((len(a),), int(lo_rank[0, 0])),
                                   torch.full((len(a),), int(rem[0, 0])), torch.tensor(2), "linear").numpy()
        for i in range(len(a)):
            keys = [so._key(float(a[i]))] * ((m - 1) // 2 + 1) + [so._key(float(hi[i]))] * (m - (m - 1) // 2 - 1)
            got = so._middle(keys, m)
            assert np.float64(got).tobytes() == want[i].tobytes(), (m, a[i], hi[i])
    assert np.signbit(np.float32(-0.0)) and not np.signbit(so._middle([so._key(-0.0)], 1))      # -0 + (+0) 0: the rule gives +0


# ---- rejections that need no GPU ------------------------------------------------------------------------------------------------
def test_python_rejections():
    g = DSMGrid(0.0, 0.0, 5.0, 5.0, 6, 4)
    z = np.zeros((4, 6), np.float32)
    for f in (dsm.stack_quantiles, dsm.stack_median, dsm.stack_nmad, dsm.fuse_stack):
        with pytest.raises(ValueError, match="64"):
            f([z] * 65, [g] * 65)
        with pytest.raises(ValueError):
            f([], [])
        with pytest.raises(ValueError, match="one grid per DSM"):
            f([z, z], [g])
        with pytest.raises(ValueError, match="shape"):
            f([np.zeros((3, 3), np.float32)], [g])
        with pytest.raises(ValueError, match="align"):
            f([z], [g], align="cubic")
        with pytest.raises(ValueError, match="align.*regrid"):
            f([z, z], [g, DSMGrid(2.5, 0.0, 5.0, 5.0, 6, 4)])
        with pytest.raises(ValueError, match="2\\^30"):
            f([z], [g], to_grid=DSMGrid(-5.0 * 2 ** 30, 0.0, 5.0, 5.0, 6, 4))
        for bad in (-1, 65, 1.5, True):
            with pytest.raises(ValueError, match="min_layers"):
                f([z], [g], min_layers=bad)
    for bad in ((), (1.5,), (-0.1,), (float("nan"),), ((1, 0),), "half"):
        with pytest.raises(ValueError):
            dsm.stack_quantiles([z], [g], q=bad)
    with pytest.raises(ValueError, match="method"):
        dsm.stack_quantiles([z], [g], method="cubic")
    for bad in (np.zeros((4, 6), np.float64), np.zeros((4, 5), np.float32), np.zeros(24, np.float32)):
        with pytest.raises(ValueError, match="centre"):
            dsm.stack_quantiles([z], [g], centre=bad)
    for bad in (dict(k=-1.0), dict(k=float("nan")), dict(k=float("inf")), dict(floor=-0.5), dict(floor=float("inf"))):
        with pytest.raises(ValueError):
            dsm.fuse_stack([z], [g], **bad)
    info = dict(members=np.array([[5, -1]], np.int64), inliers=np.array([[1, 2 ** 63 - 1]], np.int64))
    assert dsm.stack_outliers(info, 2).tolist() == [[1, 0]] and dsm.stack_outliers(info, 0).tolist() == [[0, 0]]
    assert dsm.stack_outliers(info, 63).tolist() == [[0, 1]]
    as_t = {k: torch.from_numpy(v) for k, v in info.items()}
    assert dsm.stack_outliers(as_t, 63).tolist() == [[0, 1]] and dsm.stack_outliers(as_t, 2).dtype == torch.uint8
    for bad in (-1, 64, 1.0):
        with pytest.raises(ValueError):
            dsm.stack_outliers(info, bad)


def test_c_rejections_need_no_device(lib):
    """SMVS_ERR_ARG with a message before any HIP call: the pointers are never followed."""
    P = 1 << 24                                                            # buffers far apart; none is read
    gw, gh = 20, 10
    half = (C.c_int * 2)(1, 2)

    def table(**layer):
        t = (dsm._Layer * 65)()
        for k in range(65):
            t[k] = dsm._Layer(**dict(dict(z=P, d2=None, gw=gw, gh=gh, ox=0, oy=0), **layer))
        return t

    sel_ok = dict(t=table(), n=1, lv=half, nl=1, centre=None, gw=gw, gh=gh, count=2 * P, lo=3 * P, hi=4 * P)

    def select(**change):
        a = dict(sel_ok, **change)
        return lib.smvs_dsm_stack_select(a["t"], a["n"], -999.0, a["lv"], a["nl"], a["centre"], a["gw"], a["gh"], a["count"], a["lo"], a["hi"], None)

    def levels(*pairs):
        flat = [v for p in pairs for v in p]
        return dict(lv=(C.c_int * len(flat))(*flat), nl=len(pairs))

    shared = [dict(t=None), dict(n=0), dict(n=65), dict(gw=0), dict(gh=0), dict(gw=65536, gh=32768), dict(t=table(z=None)), dict(t=table(gw=0)),
              dict(t=table(gh=-2)), dict(t=table(gw=65536, gh=32768)), dict(t=table(ox=2 ** 30)), dict(t=table(oy=-2 ** 30)),
              dict(t=table(ox=-2 ** 30)), dict(t=table(oy=2 ** 30))]
    for change in shared + [dict(lv=None), dict(lo=None), dict(nl=0), dict(nl=9), levels((-1, 2)), levels((3, 2)), levels((1, 0)), levels((1, 65537)),
                            levels((1, 2), (0, 0)), dict(count=3 * P), dict(hi=3 * P + 4), dict(hi=2 * P + 199), dict(lo=P), dict(count=P + 799),
                            dict(hi=P), dict(centre=3 * P), dict(centre=2 * P + 100), dict(centre=4 * P + 796),
                            dict(levels((0, 1), (1, 1)), hi=3 * P + 800 * 2 - 4)]:
        assert select(**change) == ERR_ARG and lib.smvs_last_error().decode(), change

    fuse_ok = dict(t=table(), n=1, kmad=4.0, floor=0.5, mc=1, gw=gw, gh=gh, out=2 * P, median=3 * P, mad=4 * P, count=5 * P, n_in=6 * P,
                   members=7 * P, inliers=8 * P)

    def fuse(**change):
        a = dict(fuse_ok, **change)
        return lib.smvs_dsm_stack_fuse(a["t"], a["n"], -999.0, a["kmad"], a["floor"], a["mc"], a["gw"], a["gh"], a["out"], a["median"], a["mad"],
                                       a["count"], a["n_in"], a["members"], a["inliers"], None)

    for change in shared + [dict(out=None), dict(kmad=-1.0), dict(kmad=float("nan")), dict(kmad=float("inf")), dict(floor=-1e-9),
                            dict(floor=float("nan")), dict(floor=float("inf")), dict(mc=-1), dict(mc=65), dict(median=2 * P), dict(mad=3 * P + 796),
                            dict(count=2 * P + 799), dict(n_in=5 * P + 199), dict(members=6 * P + 199), dict(inliers=7 * P + 1599),
                            dict(inliers=2 * P), dict(out=P), dict(median=P + 796), dict(mad=P), dict(count=P), dict(n_in=P + 799),
                            dict(members=P - 1592), dict(inliers=P + 4)]:
        assert fuse(**change) == ERR_ARG and lib.smvs_last_error().decode(), change


# ---- the town: the premises of the GPU file's end-to-end test, by the oracle ------------------------------------------------------
def test_the_town_satisfies_its_premises():
    truth, layers, block = sc.town()
    t = sc.TOWN
    ok = valid(truth, ND)
    assert ok[block].all() and 0.9 < ok.mean() < 1.0                                      # a block of valid cells; the truth has voids
    for k, z in enumerate(layers):
        e = np.abs(z.astype(np.float64) - truth.astype(np.float64))
        inside = np.zeros_like(ok)
        inside[block] = k == t["raised"]
        assert np.array_equal(valid(z, ND), ok) and (e[ok & ~inside] <= 0.5).all(), k    # the bound is hard
        if k == t["raised"]:
            assert (e[block] >= t["lift"] - 0.5).all()
    out, median, mad, count, n_in, members, inliers = so.fuse_sorted([(z, 0, 0) for z in layers], ND, t["k"] * dsm.NMAD_FACTOR, t["floor"], 1, t["gw"], t["gh"])
    assert (count[ok] == 7).all() and (count[~ok] == 0).all()
    assert (mad[ok] <= 1.0).all() and max(t["k"] * dsm.NMAD_FACTOR * 1.0, t["floor"]) < t["lift"] - 1.0      # thr stays far below the lift
    half = so.fuse_sorted([(z, 0, 0) for z in layers], ND, t["k"] * dsm.NMAD_FACTOR, 0.5, 1, t["gw"], t["gh"])
    outside = np.ones(ok.shape, bool)
    outside[block] = False
    assert ((half[5] & ~half[6])[outside] != 0).any()      # why the floor is not 0.5: where a cell's MAD is small, an honest layer is out
    outliers = (members & ~inliers)
    for k in range(7):
        want = np.zeros(ok.shape, np.int64)
        if k == t["raised"]:
            want[block] = 1
        assert np.array_equal(outliers >> k & 1, want), k
    assert (np.abs(out[ok].astype(np.float64) - truth[ok].astype(np.float64)) <= 0.5).all()
    mean = np.mean(np.stack(layers).astype(np.float64), axis=0)
    assert (np.abs(mean[block] - truth[block]) > 5.0).all()                               # 40 / 7 less the noise


# ---- planted errors: the comparison of the GPU file has to report each ---------------------------------------------------------
def test_planted_errors_are_reported(matrix):
    """Each flaw of the oracle changes some output somewhere in the cases the GPU file runs; the rule itself changes none."""
    sel_cases = [(layers, gw, gh, centre) for _, layers, gw, gh, centre in matrix] + [(*sc.zeros_case(), None), (*sc.edge_case(), None)]
    params = sc.FUSE_PARAMS + [(0.0, 2.0, 1)]

    def select_shows(flaw):
        shown = False
        for layers, gw, gh, centre in sel_cases:
            for c in (None, centre):
                good = so.select_sorted(layers, ND, sc.LEVELS, c, gw, gh)
                assert not so.differs(so.select_cells(layers, ND, sc.LEVELS, c, gw, gh), good)
                shown |= so.differs(so.select_sorted(layers, ND, sc.LEVELS, c, gw, gh, flaw=flaw), good)
        return shown

    def fuse_shows(flaw, cases):
        shown = False
        for layers, gw, gh, _ in cases:
            for kmad, floor, min_count in params:
                good = so.fuse_sorted(layers, ND, kmad, floor, min_count, gw, gh)
                shown |= so.differs(so.fuse_sorted(layers, ND, kmad, floor, min_count, gw, gh, flaw=flaw), good)
        return shown

    small = sel_cases[-2:]
    assert fuse_shows("midpoint", small) and fuse_shows("midpoint", sel_cases[:-2])      # a median of -0.0: (a + b) 0.5 keeps the sign
    assert fuse_shows("strict", small) and fuse_shows("strict", sel_cases[:-2])          # d = thr, at the least d = 0 = thr
    assert fuse_shows("sum_from_zero", small) and fuse_shows("sum_from_zero", sel_cases[:-2])      # 0.0 + -0.0 = +0.0
    assert select_shows("ties_by_layer")           # +0.0 before -0.0 in the list (the linear median of zeros is +0.0 either way)
    assert select_shows("hi_no_remainder")                                               # q = 1/2 over an odd m
    assert select_shows("valid_on_d")                                                    # a deviation of +Inf still counts
    for flaw in so.FLAWS:
        assert flaw in ("midpoint", "strict", "sum_from_zero", "ties_by_layer", "hi_no_remainder", "valid_on_d")
