"""The stack fusion on the MI355X (smvs_dsm_stack_select, smvs_dsm_stack_fuse, dsm.stack_quantiles / stack_median / stack_nmad /
fuse_stack / stack_outliers) against the numpy oracle (tests/dsm_stack_oracle.py) over the case matrix of
tests/dsm_stack_scene.py: every comparison is equal bits or equal integers, no cell excused.  Both C entries over the matrix, the
extremes against smvs_dsm_mosaic in the same process, the deviation mode, the fusion's edges by hand, guard words round every
output, outputs full of garbage, a side stream, a larger call before a smaller one, equal bits twice, every rejection with
nothing written, the Python layer, and the fused town."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import dsm_stack_oracle as so
import dsm_stack_scene as sc
from dsm_testkit import dev, lib, same as _same, same_bits, valid  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ND = sc.ND
ERR_ARG = 1                                                                # SMVS_ERR_ARG
GUARD = 64
CASES = sc.cases()
SELECT_FILLS = [(torch.uint8, 0x5a), (torch.float32, 12345.0), (torch.float32, 12345.0)]
FUSE_FILLS = [(torch.float32, 12345.0), (torch.float32, 12345.0), (torch.float32, 12345.0), (torch.uint8, 0x5a), (torch.uint8, 0x5a),
              (torch.int64, 0x5a5a5a5a5a5a5a5a), (torch.int64, 0x5a5a5a5a5a5a5a5a)]


def _table(layers):
    """Host layers (z, ox, oy) on the device -> (the smvs_dsm_layer table, the tensors to keep alive)."""
    from satmvs_amd import dsm
    d = torch.device("cuda", 0)
    held = [torch.from_numpy(np.ascontiguousarray(z, np.float32)).to(d) for z, _, _ in layers]
    table = (dsm._Layer * len(layers))()
    for k, ((z, ox, oy), zt) in enumerate(zip(layers, held)):
        table[k] = dsm._Layer(zt.data_ptr(), None, z.shape[1], z.shape[0], ox, oy)
    return table, held


def _run(entry, fills, sizes, want, call, stream=None):
    """One call of a C entry: every output wanted is a buffer full of garbage between two guards; `call` gets the pointers (None
    for an output left null).  -> the outputs as numpy, None for those left null; the guards are checked."""
    from satmvs_amd import _lib
    d = torch.device("cuda", 0)
    bufs = [torch.full((n + 2 * GUARD,), fill, dtype=dt, device=d) if w else None for (dt, fill), n, w in zip(fills, sizes, want)]
    ptrs = [C.c_void_p(b.data_ptr() + GUARD * b.element_size()) if b is not None else None for b in bufs]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        _lib.call(entry, *call(ptrs), _lib.current_stream(d))
    torch.cuda.synchronize()
    res = []
    for b, (dt, fill), n in zip(bufs, fills, sizes):
        if b is None:
            res.append(None)
            continue
        h = b.cpu().numpy()
        assert (h[:GUARD] == h.dtype.type(fill)).all() and (h[n + GUARD:] == h.dtype.type(fill)).all(), entry
        res.append(h[GUARD:n + GUARD])
    return res


def _select_c(layers, levels, centre, gw, gh, outputs=(True, True), nodata=-999.0, stream=None):
    """smvs_dsm_stack_select -> [count, lo, hi], None for count or hi left null."""
    table, held = _table(layers)
    Q, n = len(levels), gw * gh
    lv = np.array(levels, np.int32)
    ct = torch.from_numpy(np.ascontiguousarray(centre, np.float32)).cuda() if centre is not None else None
    got = _run("smvs_dsm_stack_select", SELECT_FILLS, (n, Q * n, Q * n), (outputs[0], True, outputs[1]),
               lambda p: (table, len(layers), float(nodata), lv.ctypes.data, Q, C.c_void_p(ct.data_ptr()) if ct is not None else None, gw, gh, *p),
               stream)
    del held
    return [got[0].reshape(gh, gw) if got[0] is not None else None, got[1].reshape(Q, gh, gw), got[2].reshape(Q, gh, gw) if got[2] is not None else None]


def _fuse_c(layers, kmad, floor, min_count, gw, gh, outputs=(True,) * 6, nodata=-999.0, stream=None):
    """smvs_dsm_stack_fuse -> [out, median, mad, count, n_in, members, inliers], None for those left null."""
    table, held = _table(layers)
    n = gw * gh
    got = _run("smvs_dsm_stack_fuse", FUSE_FILLS, (n,) * 7, (True,) + tuple(outputs),
               lambda p: (table, len(layers), float(nodata), float(kmad), float(floor), min_count, gw, gh, *p), stream)
    del held
    return [g.reshape(gh, gw) if g is not None else None for g in got]


def _equal(got, want, names, what):
    for g, w, name in zip(got, want, names):
        if g is not None:
            _same(np.ascontiguousarray(g), np.ascontiguousarray(w), (what, name))


# ---- both entries against the oracle over the matrix -----------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_select_against_the_oracle(dev, i):
    name, layers, gw, gh, centre = CASES[i]
    n = 1 + i % 8                                                          # 1 .. 8 levels a call over the cases
    levels = (sc.LEVELS[i % 8:] + sc.LEVELS[:i % 8])[:n]
    for lv, c in ((levels, None), (sc.LEVELS, None), (levels, centre), (sc.LEVELS[:5], centre)):
        _equal(_select_c(layers, lv, c, gw, gh), so.select_sorted(layers, ND, lv, c, gw, gh), so.SELECT_NAMES, (name, len(lv), c is not None))
    for lv in ([q] for q in sc.LEVELS[:5]):                                # every level alone
        _equal(_select_c(layers, lv, None, gw, gh), so.select_sorted(layers, ND, lv, None, gw, gh), so.SELECT_NAMES, (name, lv))


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_fuse_against_the_oracle(dev, i):
    name, layers, gw, gh, _ = CASES[i]
    for kmad, floor, min_count in sc.FUSE_PARAMS:
        _equal(_fuse_c(layers, kmad, floor, min_count, gw, gh), so.fuse_sorted(layers, ND, kmad, floor, min_count, gw, gh), so.FUSE_NAMES,
               (name, kmad, floor, min_count))


def test_the_loop_statement_too(dev):
    """The per-cell statement of the oracle on two cases, so that the device is held to both."""
    for name, layers, gw, gh, centre in (CASES[4], CASES[8]):
        _equal(_select_c(layers, sc.LEVELS, centre, gw, gh), so.select_cells(layers, ND, sc.LEVELS, centre, gw, gh), so.SELECT_NAMES, name)
        _equal(_fuse_c(layers, 2.0, 0.25, 2, gw, gh), so.fuse_cells(layers, ND, 2.0, 0.25, 2, gw, gh), so.FUSE_NAMES, name)


def test_a_nan_nodata_leaves_finiteness_alone(dev):
    name, layers, gw, gh, _ = CASES[4]
    got = _select_c(layers, [(1, 2)], None, gw, gh, nodata=float("nan"))
    want = so.select_sorted(layers, np.nan, [(1, 2)], None, gw, gh)
    assert np.array_equal(got[0], want[0]) and (got[0] > so.select_sorted(layers, ND, [(1, 2)], None, gw, gh)[0]).any()      # -999 is a height
    some = want[0] > 0
    assert same_bits(got[1][0][some], want[1][0][some]) and np.isnan(got[1][0][~some]).all()


# ---- the extremes are the mosaic's -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [2, 5, 7, 9])
def test_select_extremes_against_the_mosaic(dev, i):
    """q = 0 and q = 1 are smvs_dsm_mosaic's min and max, count its count: two kernels, one process, the same table."""
    from satmvs_amd import _lib
    name, layers, gw, gh, _ = CASES[i]
    count, lo, _ = _select_c(layers, [(0, 1), (1, 1)], None, gw, gh, outputs=(True, False))
    table, held = _table(layers)
    for mode, mine in ((2, lo[0]), (3, lo[1])):
        out = torch.empty((gh, gw), dtype=torch.float32, device=dev)
        cnt = torch.empty((gh, gw), dtype=torch.uint8, device=dev)
        _lib.call("smvs_dsm_mosaic", table, len(layers), -999.0, mode, 1, gw, gh, _lib.ptr(out), _lib.ptr(cnt), None, None, _lib.current_stream(dev))
        torch.cuda.synchronize()
        _same(out.cpu().numpy(), mine, (name, mode))
        _same(cnt.cpu().numpy(), count, (name, "count"))


# ---- the deviation mode ----------------------------------------------------------------------------------------------------------
def test_deviation_mode_and_centres_that_are_not_finite(dev):
    name, layers, gw, gh, centre = CASES[7]
    count, lo, hi = _select_c(layers, sc.LEVELS, centre, gw, gh)
    plain = _select_c(layers, [(1, 2)], None, gw, gh)[0]
    shut = ~np.isfinite(centre)
    assert shut.any() and (count[shut] == 0).all() and (plain[shut] > 0).any()
    assert same_bits(lo[:, shut], np.full_like(lo[:, shut], ND)) and same_bits(hi[:, shut], np.full_like(hi[:, shut], ND))
    assert np.array_equal(count[~shut], plain[~shut])                      # validity is decided on z, whatever d is
    assert np.isinf(lo[1][~shut]).any() and not np.isnan(lo[:, count > 0]).any()       # a d that rounds to +Inf is selected as such
    assert (lo[:, count > 0] >= 0).all() and not np.signbit(lo[:, count > 0]).any()
    # a layer as the centre: its own deviation is 0, the lowest
    z0 = so.stack(layers, ND, gw, gh)[0][0]
    c0 = np.where(valid(z0, ND), z0, np.float32(np.nan))
    got = _select_c(layers, [(0, 1)], c0, gw, gh)
    _equal(got, so.select_sorted(layers, ND, [(0, 1)], c0, gw, gh), so.SELECT_NAMES, "own layer")
    assert (got[1][0][got[0] > 0] == 0).all()


# ---- the fusion's edges ----------------------------------------------------------------------------------------------------------
def _fuse_both(layers, kmad, floor, min_count, gw, gh, what, **kw):
    got = _fuse_c(layers, kmad, floor, min_count, gw, gh, **kw)
    _equal(got, so.fuse_sorted(layers, ND, kmad, floor, min_count, gw, gh), so.FUSE_NAMES, what)
    _equal(got, so.fuse_cells(layers, ND, kmad, floor, min_count, gw, gh), so.FUSE_NAMES, (what, "cells"))
    return got


def test_fuse_edges_by_hand(dev):
    layers, gw, gh = sc.edge_case()
    below = float(np.nextafter(2.0, 0.0))                                  # thr one float64 ulp below d = 2
    out, median, mad, count, n_in, members, inliers = _fuse_both(layers, 0.0, 2.0, 1, gw, gh, "d = thr")
    assert count[0].tolist() == [3, 3, 2, 1, 4, 3]
    assert n_in[0, 0] == 3 and inliers[0, 0] == 0b111 and out[0, 0] == 12.0               # d = 2, 0, 2 against thr = 2: inclusive
    assert n_in[0, 1] == 2 and inliers[0, 1] == 0b011 and out[0, 1] == 11.0               # 14 + one float32 ulp is out
    assert n_in[0, 2] == 0 and inliers[0, 2] == 0 and members[0, 2] == 0b011              # m = 2, 10 and 20: d = 5, 5
    assert out[0, 2] == 15.0 and median[0, 2] == 15.0 and mad[0, 2] == 5.0                # nothing passes: out is the median
    assert out[0, 3] == 7.5 and median[0, 3] == 7.5 and mad[0, 3] == 0.0 and n_in[0, 3] == 1      # m = 1
    assert median[0, 4] == 2.5 and mad[0, 4] == 1.5 and n_in[0, 4] == 4 and out[0, 4] == 2.5
    assert median[0, 5] == sc.BIG and mad[0, 5] == 0.0 and inliers[0, 5] == 0b110 and out[0, 5] == sc.BIG      # d_0 = +Inf against thr
    got = _fuse_both(layers, 0.0, below, 1, gw, gh, "d one ulp above thr")
    assert got[4][0, 0] == 1 and got[6][0, 0] == 0b010 and got[0][0, 0] == 12.0
    got = _fuse_both(layers, 0.0, 0.0, 1, gw, gh, "kmad = 0, floor = 0")
    assert got[4][0].tolist() == [1, 1, 0, 1, 0, 2] and got[0][0, 4] == 2.5 and got[0][0, 2] == 15.0      # even m, a != b: n_in = 0
    got = _fuse_both(layers, 1e6, 0.0, 1, gw, gh, "a wide k: the mean of all")
    assert got[4][0].tolist() == [3, 3, 2, 1, 4, 2] and got[0][0, 2] == 15.0                # mad = 0 at cell 5: +Inf stays out
    for min_count, kept in ((0, [1, 1, 1, 1, 1, 1]), (1, [1, 1, 1, 1, 1, 1]), (2, [1, 1, 1, 0, 1, 1]), (3, [1, 1, 0, 0, 1, 1]), (4, [0, 0, 0, 0, 1, 0]),
                            (5, [0] * 6), (64, [0] * 6)):
        got = _fuse_both(layers, 3.0, 0.5, min_count, gw, gh, ("min_count", min_count))
        assert (got[5][0] != 0).tolist() == [bool(v) for v in kept] and got[3][0].tolist() == [3, 3, 2, 1, 4, 3]
        gone = np.array(kept) == 0
        assert same_bits(got[0][0, gone], np.full(gone.sum(), ND)) and same_bits(got[1][0, gone], np.full(gone.sum(), ND))
        assert same_bits(got[2][0, gone], np.full(gone.sum(), ND)) and (got[4][0, gone] == 0).all() and (got[6][0, gone] == 0).all()


def test_fuse_zeros_and_single_layers(dev):
    layers, gw, gh = sc.zeros_case()
    for kmad, floor in ((0.0, 0.0), (3.0, 0.5)):
        out, median, mad, count, n_in, members, inliers = _fuse_both(layers, kmad, floor, 1, gw, gh, ("zeros", kmad))
        assert np.signbit(out[0, 0]) and not np.signbit(median[0, 0])                       # one layer: its bits; the linear median of -0 is +0
        assert np.signbit(out[0, 2]) and np.signbit(out[0, 7]) and not np.signbit(out[0, 1]) and not np.signbit(out[0, 3])
        assert count[0].tolist() == [1, 2, 3, 3, 2, 0, 3, 2] and same_bits(out[0, 5:6], np.array([ND]))
    _equal(_select_c(layers, sc.LEVELS, None, gw, gh), so.select_sorted(layers, ND, sc.LEVELS, None, gw, gh), so.SELECT_NAMES, "zeros")
    lo = _select_c(layers, [(0, 1), (1, 1)], None, gw, gh)[1]
    assert np.signbit(lo[0, 0, 1]) and not np.signbit(lo[1, 0, 1]) and np.signbit(lo[0, 0, 3]) and not np.signbit(lo[1, 0, 3])      # -0.0 below +0.0
    z = sc.heights((9, 31), 5)                                                              # one layer alone comes back bit for bit
    want = np.where(valid(z, ND), z, ND)
    for min_count in (0, 1):
        got = _fuse_both([(z, 0, 0)], 3.0, 0.5, min_count, 31, 9, "one layer")
        assert same_bits(got[0], want)
    got = _select_c([(z, 0, 0)], sc.LEVELS, None, 31, 9)
    assert all(same_bits(got[1][j], want) and same_bits(got[2][j], want) for j in range(8))


def test_optional_outputs_streams_and_repeats(dev):
    name, layers, gw, gh, centre = CASES[8]
    full = _fuse_c(layers, 2.0, 0.25, 2, gw, gh)
    for j in range(6):                                                     # every optional output alone, and none
        want = tuple(k == j for k in range(6))
        part = _fuse_c(layers, 2.0, 0.25, 2, gw, gh, outputs=want)
        assert [p is None for p in part[1:]] == [not w for w in want]
        _equal(part, full, so.FUSE_NAMES, ("only", so.FUSE_NAMES[j + 1]))
    _equal(_fuse_c(layers, 2.0, 0.25, 2, gw, gh, outputs=(False,) * 6), full, so.FUSE_NAMES, "out alone")
    sel = _select_c(layers, sc.LEVELS, centre, gw, gh)
    for outputs in ((False, False), (True, False), (False, True)):
        part = _select_c(layers, sc.LEVELS, centre, gw, gh, outputs=outputs)
        assert (part[0] is None, part[2] is None) == (not outputs[0], not outputs[1])
        _equal(part, sel, so.SELECT_NAMES, outputs)
    side = torch.cuda.Stream(dev)
    _equal(_fuse_c(layers, 2.0, 0.25, 2, gw, gh, stream=side), full, so.FUSE_NAMES, "side stream")
    _equal(_select_c(layers, sc.LEVELS, centre, gw, gh, stream=side), sel, so.SELECT_NAMES, "side stream")
    # a larger call first (64 layers, 64 KiB of LDS), then the smaller one again, twice: nothing is left behind
    big = CASES[7]
    _fuse_c(big[1], 2.0, 0.25, 2, big[2], big[3])
    _select_c(big[1], sc.LEVELS, big[4], big[2], big[3])
    for _ in range(2):
        _equal(_fuse_c(layers, 2.0, 0.25, 2, gw, gh), full, so.FUSE_NAMES, "after a larger call")
        _equal(_select_c(layers, sc.LEVELS, centre, gw, gh), sel, so.SELECT_NAMES, "after a larger call")


# ---- rejections ------------------------------------------------------------------------------------------------------------------
def test_rejections_write_nothing(dev, lib):
    from satmvs_amd import dsm
    gw, gh = 20, 10
    z = torch.zeros((gh, gw), dtype=torch.float32, device=dev)
    ctr = torch.zeros((gh, gw), dtype=torch.float32, device=dev)
    f32 = lambda n=1: torch.full((n, gh, gw), 77.0, dtype=torch.float32, device=dev)
    u8 = lambda: torch.full((gh, gw), 77, dtype=torch.uint8, device=dev)
    i64 = lambda: torch.full((gh, gw), 77, dtype=torch.int64, device=dev)
    P = lambda t: t.data_ptr()
    half = (C.c_int * 2)(1, 2)

    def table(**layer):
        t = (dsm._Layer * 65)()
        for k in range(65):
            t[k] = dsm._Layer(**dict(dict(z=P(z), d2=None, gw=gw, gh=gh, ox=0, oy=0), **layer))
        return t

    def levels(*pairs):
        flat = [v for p in pairs for v in p]
        return dict(lv=(C.c_int * len(flat))(*flat), nl=len(pairs))

    cnt, lo, hi = u8(), f32(8), f32(8)
    sel_ok = dict(t=table(), n=1, lv=half, nl=1, centre=P(ctr), gw=gw, gh=gh, count=P(cnt), lo=P(lo), hi=P(hi))

    def select(**change):
        a = dict(sel_ok, **change)
        return lib.smvs_dsm_stack_select(a["t"], a["n"], -999.0, a["lv"], a["nl"], a["centre"], a["gw"], a["gh"], a["count"], a["lo"], a["hi"], None)

    out, med, mad, n_in, mem, inl = f32(), f32(), f32(), u8(), i64(), i64()
    fuse_ok = dict(t=table(), n=1, kmad=4.0, floor=0.5, mc=1, gw=gw, gh=gh, out=P(out), median=P(med), mad=P(mad), count=P(cnt), n_in=P(n_in),
                   members=P(mem), inliers=P(inl))

    def fuse(**change):
        a = dict(fuse_ok, **change)
        return lib.smvs_dsm_stack_fuse(a["t"], a["n"], -999.0, a["kmad"], a["floor"], a["mc"], a["gw"], a["gh"], a["out"], a["median"], a["mad"],
                                       a["count"], a["n_in"], a["members"], a["inliers"], None)

    assert select() == 0 and select(n=64, **levels(*sc.LEVELS)) == 0 and select(centre=None, count=None, hi=None) == 0 and select(centre=P(z)) == 0
    assert fuse() == 0 and fuse(n=64, mc=64, kmad=0.0, floor=0.0) == 0 and fuse(median=None, mad=None, count=None, n_in=None, members=None, inliers=None) == 0
    torch.cuda.synchronize()
    outputs = (cnt, lo, hi, out, med, mad, n_in, mem, inl)
    for t in outputs:
        t.fill_(77)
    torch.cuda.synchronize()
    shared = [dict(t=None), dict(n=0), dict(n=65), dict(gw=0), dict(gh=0), dict(gw=65536, gh=32768), dict(t=table(z=None)), dict(t=table(gw=0)),
              dict(t=table(gh=-2)), dict(t=table(gw=65536, gh=32768)), dict(t=table(ox=2 ** 30)), dict(t=table(oy=-2 ** 30))]
    for change in shared + [dict(lv=None), dict(lo=None), dict(nl=0), dict(nl=9), levels((-1, 2)), levels((3, 2)), levels((1, 0)), levels((1, 65537)),
                            levels((1, 2), (0, 0)), dict(count=P(lo)), dict(hi=P(lo) + 4), dict(hi=P(cnt)), dict(lo=P(z)), dict(count=P(z) + 799),
                            dict(hi=P(z)), dict(centre=P(lo)), dict(centre=P(cnt)), dict(centre=P(hi) + 796)]:
        assert select(**change) == ERR_ARG and lib.smvs_last_error().decode(), change
    for change in shared + [dict(out=None), dict(kmad=-1.0), dict(kmad=float("nan")), dict(kmad=float("inf")), dict(floor=-1e-9),
                            dict(floor=float("nan")), dict(floor=float("inf")), dict(mc=-1), dict(mc=65), dict(median=P(out)), dict(mad=P(med) + 796),
                            dict(count=P(out) + 799), dict(n_in=P(cnt) + 199), dict(members=P(n_in) + 192), dict(inliers=P(mem) + 1592),
                            dict(inliers=P(out)), dict(out=P(z)), dict(median=P(z) + 796), dict(mad=P(z)), dict(count=P(z)), dict(n_in=P(z) + 799),
                            dict(members=P(z)), dict(inliers=P(z) + 8)]:
        assert fuse(**change) == ERR_ARG and lib.smvs_last_error().decode(), change
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in outputs)                     # nothing ran


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def _grids_of(layers, gw, gh):
    """DSMGrids that place host layers (z, ox, oy) on a (gh, gw) destination at 5 m."""
    from satmvs_amd.dsm import DSMGrid
    E0, N0, R = 500000.0, 4000000.0, 5.0
    to = DSMGrid(E0, N0, R, R, gw, gh)
    return to, [DSMGrid(E0 + ox * R, N0 - oy * R, R, R, z.shape[1], z.shape[0]) for z, ox, oy in layers]


@pytest.mark.parametrize("i", [4, 6, 8])
def test_python_layer_against_the_entries(dev, i):
    from satmvs_amd import dsm
    name, layers, gw, gh, centre = CASES[i]
    to, grids = _grids_of(layers, gw, gh)
    zs = [z for z, _, _ in layers]
    for k, floor, min_layers in ((3.0, 0.5, 1), (0.0, 0.0, 0), (1.0, 0.25, 3)):
        want = so.fuse_sorted(layers, ND, k * dsm.NMAD_FACTOR, floor, min_layers, gw, gh)
        out, info = dsm.fuse_stack(zs, grids, to_grid=to, k=k, floor=floor, min_layers=min_layers, return_info=True)
        assert isinstance(out, np.ndarray) and all(isinstance(v, np.ndarray) for v in info.values())
        _equal([out] + [info[n] for n in ("median", "mad", "count", "n_inliers", "members", "inliers")], want, so.FUSE_NAMES, (name, k))
        _same(dsm.fuse_stack(zs, grids, to_grid=to, k=k, floor=floor, min_layers=min_layers), out, "without info")
        _same(dsm.stack_median(zs, grids, to_grid=to, min_layers=min_layers), info["median"], (name, "stack_median"))
        nm = dsm.stack_nmad(zs, grids, to_grid=to, min_layers=min_layers)
        keep = info["count"] >= max(min_layers, 1)
        assert np.array_equal(np.isnan(nm["median"]), ~keep) and np.array_equal(np.isnan(nm["mad"]), ~keep) and nm["median"].dtype == np.float64
        assert same_bits(nm["median"].astype(np.float32)[keep], info["median"][keep]) and same_bits(nm["mad"].astype(np.float32)[keep], info["mad"][keep])
        assert np.array_equal(nm["nmad"][keep], nm["mad"][keep] * dsm.NMAD_FACTOR) and np.array_equal(nm["n_valid"], info["count"])
        for j in range(len(layers)):
            _same(dsm.stack_outliers(info, j), ((info["members"] & ~info["inliers"]) >> j & 1).astype(np.uint8), (name, "outliers", j))
    # device tensors in, device tensors out
    zt = [torch.from_numpy(z).to(dev) for z in zs]
    out_t, info_t = dsm.fuse_stack(zt, grids, to_grid=to, return_info=True)
    assert out_t.is_cuda and all(v.is_cuda for v in info_t.values())
    out, info = dsm.fuse_stack(zs, grids, to_grid=to, return_info=True)
    _same(out_t.cpu().numpy(), out, "tensors")
    _same(dsm.stack_outliers(info_t, 1).cpu().numpy(), dsm.stack_outliers(info, 1), "outliers of tensors")
    # the quantiles: 8 levels and 11 (two chunks), with and without a centre
    from fractions import Fraction
    q11 = [Fraction(n, d) for n, d in sc.LEVELS] + [0.1, 0.9, (5, 7)]
    lv11 = sc.LEVELS + [(1, 10), (9, 10), (5, 7)]
    for q, lv, c in ((q11[:8], sc.LEVELS, None), (q11, lv11, None), (q11, lv11, centre)):
        got = dsm.stack_quantiles(zs, grids, to_grid=to, q=q, centre=c, min_layers=2)
        count, lo, hi = so.select_sorted(layers, ND, lv, c, gw, gh)
        _equal([got["n_valid"], got["lo"], got["hi"]], (count, lo, hi), so.SELECT_NAMES, (name, len(lv), c is not None))
        m = count.astype(np.int64)
        assert got["value"].dtype == np.float64 and got["value"].shape == lo.shape
        for j, (num, den) in enumerate(lv):
            rem = (np.maximum(m - 1, 0) * num) % den
            with np.errstate(invalid="ignore"):
                want = lo[j].astype(np.float64) + (hi[j].astype(np.float64) - lo[j].astype(np.float64)) * (rem.astype(np.float64) / float(den))
            keep = (m >= 2) & ~np.isnan(want)
            assert np.array_equal(got["value"][j][keep], want[keep]) and np.isnan(got["value"][j][m < 2]).all(), (name, j)
    mid = dsm.stack_quantiles(zs, grids, to_grid=to, q=0.5, method="midpoint")
    assert np.array_equal(mid["value"][0][mid["n_valid"] > 0], ((mid["lo"][0].astype(np.float64) + mid["hi"][0].astype(np.float64)) * 0.5)[mid["n_valid"] > 0])


def test_to_grid_none_align_and_too_many_layers(dev):
    from satmvs_amd import dsm
    from satmvs_amd.dsm import DSMGrid
    name, layers, gw, gh, _ = CASES[8]
    to, grids = _grids_of(layers, gw, gh)
    zs = [z for z, _, _ in layers]
    whole = dsm.mosaic_grid(grids)
    big = dsm.fuse_stack(zs, grids)                                        # to_grid=None: the grid that covers every layer
    assert big.shape == (whole.height, whole.width)
    ox, oy = round((to.e0 - whole.e0) / 5.0), round((whole.n0 - to.n0) / 5.0)
    _same(np.ascontiguousarray(big[oy:oy + gh, ox:ox + gw]), dsm.fuse_stack(zs, grids, to_grid=to), "a crop of the covering grid")
    off = DSMGrid(to.e0 + 3.5 * 5.0, to.n0 - 2 * 5.0, 5.0, 5.0, 12, 9)     # half a cell east of the lattice: columns 3 .. 15
    zo = sc.heights((9, 12), 91, voids=0.05)
    zo[~np.isfinite(zo) | (np.abs(zo) > 1e30)] = ND                        # regrid's blend wants numbers
    with pytest.raises(ValueError, match="align"):
        dsm.fuse_stack(zs + [zo], grids + [off], to_grid=to)
    sub = DSMGrid(to.e0 + 3 * 5.0, to.n0 - 2 * 5.0, 5.0, 5.0, 13, 9)
    for align in ("bilinear", "nearest"):
        on = dsm.regrid(zo, off, sub, mode=align)
        a, ia = dsm.fuse_stack(zs + [zo], grids + [off], to_grid=to, align=align, return_info=True)
        b, ib = dsm.fuse_stack(zs + [on], grids + [sub], to_grid=to, return_info=True)
        _same(a, b, align)
        assert all(np.array_equal(ia[k].view(np.uint8), ib[k].view(np.uint8)) for k in ia)
        _same(dsm.stack_median(zs + [zo], grids + [off], to_grid=to, align=align), dsm.stack_median(zs + [on], grids + [sub], to_grid=to), align)
        qa = dsm.stack_quantiles(zs + [zo], grids + [off], to_grid=to, align=align, q=(0.25, 0.5))
        qb = dsm.stack_quantiles(zs + [on], grids + [sub], to_grid=to, q=(0.25, 0.5))
        assert all(np.array_equal(qa[k].view(np.uint8), qb[k].view(np.uint8)) for k in qa)
    one = np.zeros((4, 6), np.float32)
    g = DSMGrid(0.0, 0.0, 5.0, 5.0, 6, 4)
    for f in (dsm.stack_quantiles, dsm.stack_median, dsm.stack_nmad, dsm.fuse_stack):
        with pytest.raises(ValueError, match="64"):
            f([one] * 65, [g] * 65)
    assert (dsm.fuse_stack([one] * 64, [g] * 64) == 0).all()


# ---- end to end: the town seen seven times -----------------------------------------------------------------------------------------
def test_the_fused_town(dev):
    """Seven layers of the town within +-0.5 m of the truth, layer 3 raised by 40 m over a block.  All inliers lie within 0.5 m
    of the truth and thr <= 3 * 1.4826 * 1.0 < 40 (test_dsm_stack_cpu.py checks these premises with the oracle), so the fusion
    names the block in layer 3 and nothing else, and stays within 0.5 m everywhere; the mean is off by 40 / 7 in the block.
    k = 3 and floor = 1 m, twice the noise bound (dsm_stack_scene.town says why)."""
    from satmvs_amd import dsm
    from satmvs_amd.dsm import DSMGrid
    truth, layers, block = sc.town()
    t = sc.TOWN
    g = DSMGrid(t["e0"], t["n0"], t["res"], t["res"], t["gw"], t["gh"])
    ok = valid(truth, ND)
    fused, info = dsm.fuse_stack(layers, [g] * 7, k=t["k"], floor=t["floor"], return_info=True)
    _equal([fused] + [info[n] for n in ("median", "mad", "count", "n_inliers", "members", "inliers")],
           so.fuse_sorted([(z, 0, 0) for z in layers], ND, t["k"] * dsm.NMAD_FACTOR, t["floor"], 1, t["gw"], t["gh"]), so.FUSE_NAMES, "town")
    for k in range(7):
        want = np.zeros(truth.shape, np.uint8)
        if k == t["raised"]:
            want[block] = 1
        _same(dsm.stack_outliers(info, k), want, ("outliers", k))
    assert same_bits(fused[~ok], np.full((~ok).sum(), ND))
    err = np.abs(fused[ok].astype(np.float64) - truth[ok].astype(np.float64))
    mean = dsm.mosaic(layers, [g] * 7, mode="mean")
    off = np.abs(mean[block].astype(np.float64) - truth[block].astype(np.float64))
    print("fused town: largest error %.4f m; the mean's smallest error in the block %.4f m" % (err.max(), off.min()))
    assert (err <= 0.5).all()
    assert (off > 5.0).all()
