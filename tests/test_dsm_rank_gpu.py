"""Focal order statistics on the device against the numpy oracle (tests/dsm_rank_oracle.py).  smvs_dsm_focal_select and
smvs_dsm_focal_count are called at their C interface with guard words round every output and the outputs seeded; float32 grids
are compared by their bits and counts with equality, no cell excused.  Statement (a), the loop, is the reference where it takes
well under a second, statement (b) elsewhere (tests/test_dsm_rank_cpu.py holds the two against each other).  Then the
certificate of every selected value on the device, despike's own median, streams, every limit, and the Python layer."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import dsm_rank_oracle as ro
from dsm_testkit import dev, lib, same_bits, valid  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
ND = -999.0
G = 64                                                       # guard words on both sides of a buffer
SEED = 77                                                    # what every output and guard word holds before a call
LOOP_BUDGET = 60000                                          # cells x window cells up to which statement (a) is the reference
PARTS = 8


def _guarded(n, dtype, dev):
    return torch.full((n + 2 * G,), SEED, dtype=dtype, device=dev)


def _intact(buf, n):
    return bool((buf[:G] == SEED).all()) and bool((buf[G + n:] == SEED).all())


def _select(z_d, foot, levels, nodata=ND, centre=None, want_hi=True, want_n=True, stream=None):
    """smvs_dsm_focal_select at its C entry -> (n, lo, hi) numpy, None for an output passed as null."""
    from satmvs_amd import _lib
    dev = z_d.device
    gh, gw = z_d.shape
    runs = ro.runs_of(foot)
    lv = np.ascontiguousarray(levels, np.int32).reshape(-1, 2)
    Q, cells = len(lv), gh * gw
    n, lo, hi = _guarded(cells, torch.int32, dev), _guarded(Q * cells, torch.float32, dev), _guarded(Q * cells, torch.float32, dev)
    c_d = None if centre is None else torch.from_numpy(np.ascontiguousarray(centre, np.float32)).to(dev)
    torch.cuda.synchronize()
    _lib.call("smvs_dsm_focal_select", _lib.ptr(z_d), gw, gh, nodata, runs.ctypes.data, len(runs), lv.ctypes.data, Q,
              _lib.ptr(c_d) if c_d is not None else None, _lib.ptr(n[G:]) if want_n else None, _lib.ptr(lo[G:]),
              _lib.ptr(hi[G:]) if want_hi else None, stream if stream is not None else _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert _intact(n, cells) and _intact(lo, Q * cells) and _intact(hi, Q * cells), "a guard word changed"
    assert want_n or bool((n == SEED).all())
    assert want_hi or bool((hi == SEED).all())
    return (n[G:G + cells].cpu().numpy().reshape(gh, gw) if want_n else None, lo[G:G + Q * cells].cpu().numpy().reshape(Q, gh, gw),
            hi[G:G + Q * cells].cpu().numpy().reshape(Q, gh, gw) if want_hi else None)


def _count(z_d, foot, t_d, nodata=ND, want_n=True, stream=None):
    """smvs_dsm_focal_count at its C entry -> (n, below, equal) numpy."""
    from satmvs_amd import _lib
    dev = z_d.device
    gh, gw = z_d.shape
    runs = ro.runs_of(foot)
    cells = gh * gw
    n, below, equal = (_guarded(cells, torch.int32, dev) for _ in range(3))
    torch.cuda.synchronize()
    _lib.call("smvs_dsm_focal_count", _lib.ptr(z_d), gw, gh, nodata, runs.ctypes.data, len(runs), _lib.ptr(t_d),
              _lib.ptr(n[G:]) if want_n else None, _lib.ptr(below[G:]), _lib.ptr(equal[G:]), stream if stream is not None else _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert _intact(n, cells) and _intact(below, cells) and _intact(equal, cells), "a guard word changed"
    assert want_n or bool((n == SEED).all())
    return tuple(b[G:G + cells].cpu().numpy().reshape(gh, gw) if b is not n or want_n else None for b in (n, below, equal))


@functools.lru_cache(maxsize=None)
def _matrix():
    return ro.matrix()                                       # shared: nobody writes to it


def _cheap(c):
    return c["dsm"].size * int(c["foot"].sum()) <= LOOP_BUDGET


@functools.lru_cache(maxsize=None)
def _want(i):
    c = _matrix()[i]
    return (ro.select_loop if _cheap(c) else ro.select_sorted)(c["dsm"], c["foot"], c["levels"], c["nodata"], c["centre"])


def _case(name):
    return [c for c in _matrix() if c["name"] == name][0]


# ---- the matrix: grids, windows, values, levels, the deviation mode ----------------------------------------------------------------
@pytest.mark.parametrize("part", range(PARTS))
def test_the_matrix(dev, part):
    for i in range(part, len(_matrix()), PARTS):
        c = _matrix()[i]
        got = _select(torch.from_numpy(c["dsm"]).to(dev), c["foot"], c["levels"], c["nodata"], c["centre"])
        d = ro.differing(got, _want(i))
        assert d is None, (c["name"], c["levels"], d)


def test_the_matrix_holds_what_it_should(dev):
    names = [c["name"] for c in _matrix()]
    T = ro.TILE
    from satmvs_amd import dsm
    assert T == dsm.RANK_TILE
    for gh, gw in ((1, 1), (1, 70), (67, 1), (2, 2), (5, 63), (5, 64), (5, 65), (T - 1, 2 * T + 1), (T, T), (T + 1, T - 1), (2 * T + 1, T + 1), (70, 90)):
        for w in ("box 0", "box 1", "box 3", "box 8", "disc 0", "disc 1", "disc 3", "disc 8", "annulus 4..8", "one row", "one column", "lopsided"):
            assert "scene %dx%d %s" % (gh, gw, w) in names
    for w in ("box 32", "disc 32"):
        assert "scene 70x90 " + w in names and not any(n.endswith(w) and not n.startswith("scene 70x90") for n in names)
    assert all(c["foot"].shape[0] <= 9 and c["foot"].shape[1] <= 9 for c in _matrix() if "257x301" in c["name"])
    assert any(_cheap(c) for c in _matrix()) and any(not _cheap(c) for c in _matrix())
    assert ro.footprint("lopsided", 5)[:, :6].sum() == 0     # every dx > 0
    z = _case("scene 70x90 box 8")["dsm"]
    assert 0.08 < 1.0 - valid(z, ND).mean() < 0.16 and np.isnan(z).any() and np.isposinf(z).any() and np.isneginf(z).any() and (z == ND).any()
    assert any(name.startswith("both zeros") for name in names)
    r, col = np.indices((9, 40))
    zeros = np.where((r + col) % 2 == 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32)  # both zeros in every window
    n, lo, _ = _select(torch.from_numpy(zeros).to(dev), ro.footprint("box", 1), ((0, 1), (1, 1)))
    assert n.min() == 4 and (lo[0].view(np.uint32) == 0x80000000).all() and (lo[1].view(np.uint32) == 0).all()    # rank 0 comes back as -0.0
    c = _case("deviation that rounds to +Inf box 1")
    n, lo, _ = _select(torch.from_numpy(c["dsm"]).to(dev), c["foot"], ((1, 1),), centre=c["centre"])
    assert np.isposinf(lo[0, 10, 10]) and n[10, 10] > 0


@pytest.mark.parametrize("name", ["scene 5x65 disc 3", "scene 65x33 annulus 4..8", "scene 70x90 box 8", "special values disc 3",
                                  "deviation from the median, quarters disc 3"])
def test_null_outputs_and_one_level(dev, name):
    """hi null, n_out null, both; each level on its own gives the bits it gives among four."""
    c = _case(name)
    z_d = torch.from_numpy(c["dsm"]).to(dev)
    levels = ro.LEVELS[2:6]
    want = ro.select_sorted(c["dsm"], c["foot"], levels, c["nodata"], c["centre"])
    for want_hi, want_n in ((True, True), (False, True), (True, False), (False, False)):
        got = _select(z_d, c["foot"], levels, c["nodata"], c["centre"], want_hi=want_hi, want_n=want_n)
        assert ro.differing(got, want) is None, (want_hi, want_n, ro.differing(got, want))
    for j, lv in enumerate(levels):
        got = _select(z_d, c["foot"], (lv,), c["nodata"], c["centre"])
        assert ro.differing(got, (want[0], want[1][j:j + 1], want[2][j:j + 1])) is None, lv


# ---- smvs_dsm_focal_count ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(4))
def test_counts_with_the_cells_own_heights(dev, part):
    cases = [c for c in _matrix() if c["centre"] is None and "32" not in c["name"]][part::12]
    assert len(cases) >= 8
    for c in cases:
        z_d = torch.from_numpy(c["dsm"]).to(dev)
        want = (ro.count_loop if _cheap(c) else ro.count_sorted)(c["dsm"], c["foot"], c["dsm"], c["nodata"])
        d = ro.differing(_count(z_d, c["foot"], z_d, c["nodata"]), want)
        assert d is None, (c["name"], d)


@pytest.mark.parametrize("name", ["scene 65x33 disc 8", "scene 70x90 lopsided", "special values box 1", "both zeros disc 3", "another nodata disc 3"])
def test_counts_with_any_threshold(dev, name):
    c = _case(name)
    z = c["dsm"]
    t = np.roll(z, -3, axis=1).copy()                        # the height three cells east, a cell of every window: `equal` counts
    at = np.arange(0, t.size, 7)
    t.reshape(-1)[at] = np.array([np.nan, np.inf, -np.inf, c["nodata"], 0.0, -0.0], np.float32)[np.arange(len(at)) % 6]
    z_d = torch.from_numpy(z).to(dev)
    want = ro.count_sorted(z, c["foot"], t, c["nodata"])
    assert (want[1][np.isnan(t)] == -1).all() and (want[2][~np.isnan(t)] > 0).any()
    for want_n in (True, False):
        d = ro.differing(_count(z_d, c["foot"], torch.from_numpy(t).to(dev), c["nodata"], want_n=want_n), want)
        assert d is None, (want_n, d)


def test_every_selected_value_carries_its_certificate(dev):
    """257 x 301 at radius 8, on the device alone: below <= rank < below + equal for every lo and hi of seven levels."""
    z = ro.scene(257, 301, 8)
    z_d = torch.from_numpy(z).to(dev)
    for foot in (ro.footprint("box", 8), ro.footprint("disc", 8)):
        for levels in (ro.LEVELS[:4], ro.LEVELS[3:]):
            n, lo, hi = _select(z_d, foot, levels)
            m = n.astype(np.int64)
            assert m.max() > 0.9 * foot.sum() and m.min() < 0.3 * foot.sum()          # windows nearly full, and clipped corners
            for j, (num, den) in enumerate(levels):
                h = (m - 1) * num
                for value, rank in ((lo[j], h // den), (hi[j], h // den + (h % den > 0))):
                    n2, below, equal = _count(z_d, foot, torch.from_numpy(value).to(dev))
                    assert np.array_equal(n2, n)
                    held = ((below <= rank) & (rank < below + equal)) | (m == 0)
                    assert held.all(), (levels[j], int((~held).sum()))


# ---- existing native code: despike's median ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius,thresh,min_valid", [(1, 4.0, 3), (2, 10.0, 3), (3, 2.5, 20)])
def test_despike_removes_what_the_focal_median_says(dev, radius, thresh, min_valid):
    from satmvs_amd import dsm
    z = ro.qo.kit_scene(70, 90, 21, voids=0.1, salt=0.05)
    _, removed = dsm.despike(z, ND, radius, thresh, min_valid, return_removed=True)
    box = dsm.focal_window("box", radius)
    med = dsm.focal_median(z, box)
    n = dsm.focal_counts(z, box)[0]
    with np.errstate(invalid="ignore"):
        want = valid(z, ND) & ((n < min_valid) | (np.abs(z.astype(np.float64) - med.astype(np.float64)) > thresh))
    assert removed.dtype == np.uint8 and np.array_equal(removed.astype(bool), want) and 0 < want.sum() < valid(z, ND).sum()


# ---- run conditions ------------------------------------------------------------------------------------------------------------------
def test_streams_and_repeats(dev):
    from satmvs_amd import _lib
    c = _case("scene 70x90 disc 8")
    other = _case("scene 70x90 annulus 4..8")
    z_d = torch.from_numpy(c["dsm"]).to(dev)
    levels = ro.LEVELS[:4]
    first = _select(z_d, c["foot"], levels)
    assert ro.differing(first, ro.select_sorted(c["dsm"], c["foot"], levels)) is None
    assert ro.differing(_select(z_d, c["foot"], levels), first) is None                          # two calls, equal bits
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    assert ro.differing(_select(z_d, c["foot"], levels, stream=_lib.C.c_void_p(s1.cuda_stream)), first) is None
    assert ro.differing(_count(z_d, c["foot"], z_d, stream=_lib.C.c_void_p(s1.cuda_stream)), ro.count_sorted(c["dsm"], c["foot"], c["dsm"])) is None
    # two windows at once on two streams: the run lists travel in each launch's own arguments
    gh, gw = z_d.shape
    cells, Q = gh * gw, len(levels)
    lv = np.ascontiguousarray(levels, np.int32)
    outs = []
    for _ in range(6):
        n, lo, hi = _guarded(cells, torch.int32, dev), _guarded(Q * cells, torch.float32, dev), _guarded(Q * cells, torch.float32, dev)
        outs.append((n, lo, hi))
    torch.cuda.synchronize()
    for (foot, s), (n, lo, hi) in zip(((c["foot"], s1), (other["foot"], s2)) * 3, outs):
        runs = ro.runs_of(foot)
        _lib.call("smvs_dsm_focal_select", _lib.ptr(z_d), gw, gh, ND, runs.ctypes.data, len(runs), lv.ctypes.data, Q, None,
                  _lib.ptr(n[G:]), _lib.ptr(lo[G:]), _lib.ptr(hi[G:]), _lib.C.c_void_p(s.cuda_stream))
    torch.cuda.synchronize()
    second = ro.select_sorted(other["dsm"], other["foot"], levels)
    assert ro.differing(second, first) is not None
    for k, (n, lo, hi) in enumerate(outs):
        assert _intact(n, cells) and _intact(lo, Q * cells) and _intact(hi, Q * cells)
        got = (n[G:G + cells].cpu().numpy().reshape(gh, gw), lo[G:G + Q * cells].cpu().numpy().reshape(Q, gh, gw),
               hi[G:G + Q * cells].cpu().numpy().reshape(Q, gh, gw))
        assert ro.differing(got, first if k % 2 == 0 else second) is None, k


# ---- every limit: SMVS_ERR_ARG, nothing written --------------------------------------------------------------------------------------
def _rejected(lib, name, args, message):
    rc = getattr(lib, name)(*args)
    assert rc == 1, (message, rc)                            # SMVS_ERR_ARG
    assert message in lib.smvs_last_error().decode(), (message, lib.smvs_last_error().decode())


def test_argument_rejections_write_nothing(dev, lib):
    from satmvs_amd import _lib
    gh, gw, Q = 6, 9, 2
    cells = gh * gw
    z = torch.ones((gh, gw), dtype=torch.float32, device=dev)
    t = torch.ones((gh, gw), dtype=torch.float32, device=dev)
    centre = torch.zeros((gh, gw), dtype=torch.float32, device=dev)
    bufs = {k: _guarded(Q * cells, dt, dev) for k, dt in (("n", torch.int32), ("lo", torch.float32), ("hi", torch.float32),
                                                          ("below", torch.int32), ("equal", torch.int32))}
    p = lambda x: _lib.ptr(x).value
    runs = lambda *r: np.array(r, np.int32).reshape(-1, 3)
    keep = []                                                # host arrays stay alive until the calls have returned

    def host(a):
        keep.append(np.ascontiguousarray(a, np.int32))
        return keep[-1].ctypes.data

    box = runs((-1, -1, 1), (0, -1, 1), (1, -1, 1))
    good_runs = dict(runs=host(box), n_runs=3)
    window_faults = [
        (dict(runs=None), "null pointer"), (dict(n_runs=0), "n_runs must be in 1 .. 130"), (dict(n_runs=-3), "n_runs must be in 1 .. 130"),
        (dict(runs=host(np.tile(box[1], (131, 1))), n_runs=131), "n_runs must be in 1 .. 130"),
        (dict(runs=host(runs((33, 0, 0))), n_runs=1), "outside -32 .. 32"), (dict(runs=host(runs((-33, 0, 0))), n_runs=1), "outside -32 .. 32"),
        (dict(runs=host(runs((0, -33, 0))), n_runs=1), "outside -32 .. 32"), (dict(runs=host(runs((0, 0, 33))), n_runs=1), "outside -32 .. 32"),
        (dict(runs=host(runs((0, 1, 0))), n_runs=1), "empty bounds"),
        (dict(runs=host(runs((1, 0, 0), (0, 0, 0))), n_runs=2), "sorted by (dy, dx0)"),
        (dict(runs=host(runs((0, 2, 3), (0, 0, 0))), n_runs=2), "sorted by (dy, dx0)"),
        (dict(runs=host(runs((0, 0, 2), (0, 2, 3))), n_runs=2), "neither overlap nor touch"),
        (dict(runs=host(runs((0, 0, 2), (0, 3, 4))), n_runs=2), "neither overlap nor touch"),
        (dict(runs=host(runs((0, 0, 2), (0, 0, 2))), n_runs=2), "neither overlap nor touch"),
        (dict(gw=0), "grid size"), (dict(gh=-1), "grid size"), (dict(gw=65536, gh=32768), "too large"),
    ]
    stream = _lib.current_stream(dev)
    # select
    good = dict(dsm=p(z), gw=gw, gh=gh, nodata=ND, **good_runs, levels=host([[1, 2], [1, 4]]), n_levels=Q, centre=p(centre),
                n_out=p(bufs["n"][G:]), lo=p(bufs["lo"][G:]), hi=p(bufs["hi"][G:]))
    order = ["dsm", "gw", "gh", "nodata", "runs", "n_runs", "levels", "n_levels", "centre", "n_out", "lo", "hi"]
    faults = window_faults + [
        (dict(dsm=None), "null pointer"), (dict(levels=None), "null pointer"), (dict(lo=None), "null pointer"),
        (dict(n_levels=0), "n_levels must be in 1 .. 4"), (dict(n_levels=5), "n_levels must be in 1 .. 4"),
        (dict(levels=host([[1, 2], [-1, 4]])), "level 1"), (dict(levels=host([[3, 2], [1, 4]])), "level 0"),
        (dict(levels=host([[1, 2], [0, 0]])), "level 1"), (dict(levels=host([[1, 2], [1, 65537]])), "level 1"),
        (dict(lo=p(z)), "lo aliases dsm"), (dict(lo=p(centre)), "lo aliases centre"), (dict(hi=p(z)), "hi aliases dsm"),
        (dict(hi=p(bufs["lo"][G:])), "hi aliases lo"), (dict(n_out=p(z)), "n_out aliases dsm"), (dict(n_out=p(bufs["lo"][G:])), "lo aliases n_out"),
        (dict(centre=p(bufs["hi"][G:])), "hi aliases centre"), (dict(hi=p(bufs["lo"][G + cells:])), "hi aliases lo"),
    ]
    for change, message in faults:
        args = dict(good)
        args.update(change)
        _rejected(lib, "smvs_dsm_focal_select", [args[k] for k in order] + [stream], message)
    # count
    good = dict(dsm=p(z), gw=gw, gh=gh, nodata=ND, **good_runs, t=p(t), n_out=p(bufs["n"][G:]), below=p(bufs["below"][G:]), equal=p(bufs["equal"][G:]))
    order = ["dsm", "gw", "gh", "nodata", "runs", "n_runs", "t", "n_out", "below", "equal"]
    faults = window_faults + [
        (dict(dsm=None), "null pointer"), (dict(t=None), "null pointer"), (dict(below=None), "null pointer"), (dict(equal=None), "null pointer"),
        (dict(below=p(z)), "below aliases dsm"), (dict(equal=p(t)), "equal aliases t"), (dict(equal=p(bufs["below"][G:])), "equal aliases below"),
        (dict(n_out=p(t)), "n_out aliases t"), (dict(below=p(bufs["n"][G:])), "below aliases n_out"),
    ]
    for change, message in faults:
        args = dict(good)
        args.update(change)
        _rejected(lib, "smvs_dsm_focal_count", [args[k] for k in order] + [stream], message)
    torch.cuda.synchronize()
    assert all(bool((b == SEED).all()) for b in bufs.values()), "a rejected call wrote"
    # what the limits allow: 130 runs, offsets of +-32, den = 2^16, t = dsm
    full = ro.footprint("annulus", 32, 16)
    assert len(ro.runs_of(full)) == 2 * 33 + 32 and np.abs(ro.runs_of(full)).max() == 32
    teeth = np.zeros((65, 65), bool)
    teeth[:, 0] = teeth[:, -1] = True
    assert len(ro.runs_of(teeth)) == 130
    zs = ro.scene(40, 45, 3)
    got = _select(torch.from_numpy(zs).to(dev), teeth, ((1, 65536), (65536, 65536)))
    assert ro.differing(got, ro.select_sorted(zs, teeth, ((1, 65536), (1, 1)))) is None


# ---- the Python layer end to end -----------------------------------------------------------------------------------------------------
def _same_dict(got, want, what):
    assert set(got) == set(want), what
    for k, w in want.items():
        g = got[k]
        assert isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype)
        view = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
        assert np.array_equal(g.view(view), w.view(view)), (what, k, int((g.view(view) != w.view(view)).sum()))


@pytest.mark.parametrize("method", ro.qo.METHODS)
def test_focal_quantiles(dev, method):
    """Nine levels, so three calls of four; a FocalWindow and a footprint; with and without a centre; min_valid."""
    from satmvs_amd import dsm
    z = ro.scene(45, 70, 13, voids=0.3)
    qs = (0, 0.1, 0.25, Fraction(1, 3), 0.5, (2, 3), 0.9, 0.95, 1)
    for window, foot in ((dsm.focal_window("disc", 3), ro.footprint("disc", 3)), (ro.footprint("lopsided", 5), ro.footprint("lopsided", 5))):
        for min_valid in (1, 12):
            want = ro.quantiles(z, foot, qs, method, None, min_valid)
            _same_dict(dsm.focal_quantiles(z, window, qs, method, min_valid=min_valid), want, (method, min_valid))
        centre = ro.quantiles(z, foot, (0.5,))["value"][0].astype(np.float32)
        _same_dict(dsm.focal_quantiles(z, window, qs[2:6], method, centre=centre), ro.quantiles(z, foot, qs[2:6], method, centre), (method, "centre"))
    assert np.isnan(want["value"]).any() and not np.isnan(want["value"]).all()


def test_focal_median_nmad_and_percentile(dev):
    from satmvs_amd import dsm
    z = ro.scene(45, 70, 14, voids=0.3)
    for window, foot in ((dsm.focal_window("box", 2), ro.footprint("box", 2)), (dsm.focal_window("annulus", 6, 2), ro.footprint("annulus", 6, 2))):
        for fill in (False, True):
            for min_valid in (1, 15):
                got = dsm.focal_median(z, window, min_valid=min_valid, fill=fill)
                assert isinstance(got, np.ndarray) and same_bits(got, ro.median(z, foot, min_valid, fill=fill)), (fill, min_valid)
        kept = dsm.focal_median(z, window)
        assert same_bits(kept[~valid(z, ND)], z[~valid(z, ND)]) and not same_bits(dsm.focal_median(z, window, fill=True), kept)
        _same_dict(dsm.focal_nmad(z, window, min_valid=3), ro.nmad(z, foot, 3), "nmad")
        for min_valid in (2, 9):
            got = dsm.elevation_percentile(z, window, min_valid=min_valid)
            want = ro.elevation_percentile(z, foot, min_valid)
            assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64)), min_valid
        for threshold in (None, 130.0, np.roll(z, 1, axis=0)):
            t = z if threshold is None else np.full_like(z, threshold) if isinstance(threshold, float) else threshold
            got = dsm.focal_counts(z, window, threshold)
            assert all(isinstance(g, np.ndarray) and g.dtype == np.int32 for g in got) and ro.differing(got, ro.count_sorted(z, foot, t)) is None
    other = np.where(z == np.float32(ND), np.float32(-5.0), z)
    assert same_bits(dsm.focal_median(other, ro.footprint("disc", 2), nodata=-5.0), ro.median(other, ro.footprint("disc", 2), nodata=-5.0))


def test_despike_robust_takes_the_spike_and_keeps_the_roof_edge(dev):
    """A flat roof 12 m over gently sloping ground, a 9 m spike on the ground three cells from the roof's edge, 15 x 15 windows:
    despike() cannot reach that far (7 x 7 at most); here the spike goes and both sides of the edge stay."""
    from satmvs_amd import dsm
    r, c = np.indices((60, 80))
    z = (100.0 + 0.02 * c + 0.01 * r).astype(np.float32)
    z += (np.random.default_rng(3).normal(0.0, 0.05, z.shape)).astype(np.float32)
    roof = (r >= 15) & (r < 45) & (c >= 20) & (c < 50)
    z[roof] += np.float32(12.0)
    z[30, 53] += np.float32(9.0)                             # on the ground, 3 cells east of the roof's edge
    z[5, 5] = np.float32(ND)
    window = dsm.focal_window("box", 7)
    out, removed = dsm.despike_robust(z, window, k=3.0, floor=0.5, min_valid=3, return_removed=True)
    want_out, want_removed = ro.despike_robust(z, ro.footprint("box", 7), 3.0, 0.5, 3)
    assert isinstance(out, np.ndarray) and same_bits(out, want_out) and removed.dtype == np.uint8 and np.array_equal(removed, want_removed)
    assert removed[30, 53] == 1 and out[30, 53] == np.float32(ND)
    edge = np.zeros_like(roof)
    edge[23:37, 17:23] = edge[23:37, 47:53] = True           # three cells on either side of the roof's east and west edges, between
    assert removed[edge].sum() == 0 and same_bits(out[edge], z[edge])            # the corners, which no median filter keeps
    assert removed.sum() < 0.05 * z.size and out.view(np.uint32)[5, 5] == z.view(np.uint32)[5, 5]
    assert same_bits(dsm.despike_robust(z, window), out)


def test_numpy_in_numpy_out_tensors_in_tensors_out(dev):
    from satmvs_amd import dsm
    z = ro.scene(20, 33, 15)
    z_d = torch.from_numpy(z).to(dev)
    box = dsm.focal_window("box", 1)
    calls = (lambda a: dsm.focal_quantiles(a, box), lambda a: dsm.focal_median(a, box), lambda a: dsm.focal_nmad(a, box),
             lambda a: dsm.despike_robust(a, box, return_removed=True), lambda a: dsm.focal_counts(a, box), lambda a: dsm.elevation_percentile(a, box),
             lambda a: dsm.focal_counts(a, box, a))
    for call in calls:
        host, device = call(z), call(z_d)
        host = list(host.values()) if isinstance(host, dict) else list(host) if isinstance(host, tuple) else [host]
        device = list(device.values()) if isinstance(device, dict) else list(device) if isinstance(device, tuple) else [device]
        assert len(host) == len(device)
        for h, d in zip(host, device):
            assert isinstance(h, np.ndarray) and isinstance(d, torch.Tensor) and d.device == z_d.device
            assert h.dtype == d.cpu().numpy().dtype and np.array_equal(h, d.cpu().numpy(), equal_nan=True)
