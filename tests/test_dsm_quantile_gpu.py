"""Zonal order statistics on the device against the numpy oracle (tests/dsm_quantile_oracle.py).  smvs_dsm_label_select is called
at its C interface with guard words round `out`, `nvalid` and the workspace, the workspace seeded; `out` is compared by its bits
and `nvalid` with np.array_equal, no label excused.  Then the Python layer end to end."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import dsm_quantile_oracle as qo
from dsm_testkit import dev, lib, same_bits  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
ND = -999.0
G = 64                                                       # guard words on both sides of a buffer
RANK_SETS = ((1, 0), (2, 1), (7, 2), (8, 3))                 # (n_ranks, the kind the columns start at)


def _guarded(n, dtype, dev, fill=77):
    return torch.full((n + 2 * G,), fill, dtype=dtype, device=dev)


def _intact(buf, n, fill=77):
    return bool((buf[:G] == fill).all()) and bool((buf[G + n:] == fill).all())


def _native(lab_d, val_d, n, ranks, nodata=ND, centre=None, fill=0x5a, stream=None, nvalid=True):
    """smvs_dsm_label_select at its C entry -> (out (n, R) float32 numpy, nvalid (n) int32 numpy or None)."""
    from satmvs_amd import _lib
    dev = lab_d.device
    gh, gw = lab_d.shape
    ranks = np.ascontiguousarray(ranks, np.int32)
    R = ranks.shape[1]
    assert ranks.shape == (n, R)
    nbytes = _lib.load().smvs_dsm_label_select_workspace_bytes(n, R)
    assert nbytes > 0
    ws = torch.full((nbytes + 2 * G,), fill, dtype=torch.uint8, device=dev)
    ws[:G] = 77
    ws[G + nbytes:] = 77
    out, nv = _guarded(n * R, torch.float32, dev), _guarded(n, torch.int32, dev)
    r_d = torch.zeros(max(n * R, 1), dtype=torch.int32, device=dev)            # never a null pointer, n = 0 included
    r_d[:n * R] = torch.from_numpy(ranks.reshape(-1)).to(dev)
    c_d = None if centre is None else torch.from_numpy(np.ascontiguousarray(centre, np.float32)).to(dev)
    torch.cuda.synchronize()
    _lib.call("smvs_dsm_label_select", _lib.ptr(lab_d), _lib.ptr(val_d), gw, gh, nodata, n, _lib.ptr(c_d) if c_d is not None else None,
              _lib.ptr(r_d), R, _lib.ptr(out[G:]), _lib.ptr(nv[G:]) if nvalid else None, _lib.ptr(ws[G:]), nbytes,
              stream if stream is not None else _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert _intact(out, n * R) and _intact(nv, n) and _intact(ws, nbytes), "a guard word changed"
    if not nvalid:
        assert bool((nv == 77).all())
    return out[G:G + n * R].cpu().numpy().reshape(n, R), nv[G:G + n].cpu().numpy() if nvalid else None


def _check(dev, c, R, turn, **kw):
    """One case of the matrix at one rank set against statement (a)."""
    lab_d, val_d = torch.from_numpy(c["labels"]).to(dev), torch.from_numpy(c["values"]).to(dev)
    m = qo.n_valid(c["labels"], c["values"], c["n"], c["nodata"], c["centre"])
    r = qo.rank_matrix(m, R, turn)
    want = qo.select_sorted(c["labels"], c["values"], c["n"], r, c["nodata"], c["centre"])
    got = _native(lab_d, val_d, c["n"], r, c["nodata"], c["centre"], **kw)
    d = qo.differing(*got, *want)
    assert d is None, (c["name"], R, turn, d)
    return got


@functools.lru_cache(maxsize=None)
def _matrix():
    return qo.matrix()                                       # shared: nobody writes to it


# ---- the matrix: grids, labels, values, ranks, the deviation mode ------------------------------------------------------------------
@pytest.mark.parametrize("R,turn", RANK_SETS)
def test_the_matrix(dev, R, turn):
    for c in _matrix():
        _check(dev, c, R, turn)


def test_the_matrix_holds_what_it_should():
    names = [c["name"] for c in _matrix()]
    for shape in ("1x1", "1x70", "67x1", "2x2", "5x63", "5x64", "5x65", "257x301"):
        assert "special " + shape in names and "scene " + shape in names
    rank0 = None
    for c in _matrix():
        if c["name"] == "both zeros in one zone":
            rank0 = qo.select_sorted(c["labels"], c["values"], 1, np.zeros((1, 1), np.int32))[0]
    assert rank0.view(np.uint32).tolist() == [[0x80000000]]                     # rank 0 comes back as -0.0


@pytest.mark.parametrize("density", [0.2, 0.5, 0.8])
def test_labels_of_random_masks(dev, density):
    """Zones from dsm.label at both connectivities, values the kit's scene with salt noise and 0, 5 and 30 % voids."""
    from satmvs_amd import dsm
    gh, gw = 257, 301
    rng = np.random.default_rng(int(10 * density))
    coarse = rng.random(((gh + 2) // 3, (gw + 2) // 3)) < density
    mask = np.kron(coarse, np.ones((3, 3), bool))[:gh, :gw] & (rng.random((gh, gw)) < 0.95)
    for conn, voids in ((4, 0.0), (8, 0.05), (8, 0.3)):
        labels, n = dsm.label(mask, conn)
        assert n > 1
        c = {"name": "label %g %d %g" % (density, conn, voids), "labels": labels, "values": qo.kit_scene(gh, gw, 3, voids=voids, salt=0.02),
             "n": n, "nodata": ND, "centre": None}
        _check(dev, c, 8, 0)
        _check(dev, c, 2, 4)


# ---- grouping of ranks into calls ---------------------------------------------------------------------------------------------------
def test_any_grouping_of_ranks_gives_the_same_bits(dev):
    c = [c for c in _matrix() if c["name"] == "kit voids 0.05"][0]
    lab_d, val_d = torch.from_numpy(c["labels"]).to(dev), torch.from_numpy(c["values"]).to(dev)
    m = qo.n_valid(c["labels"], c["values"], c["n"])
    r = qo.rank_matrix(m, 8, 0)
    whole, nv = _native(lab_d, val_d, c["n"], r)
    for groups in ([[0], [1, 2, 3, 4, 5, 6, 7]], [[0, 1, 2, 3], [4, 5, 6, 7]], [[7, 6, 5], [4, 3], [2], [1, 0]], [[3, 3, 3, 0, 0, 7, 7, 7]]):
        for g in groups:
            part, nv_part = _native(lab_d, val_d, c["n"], r[:, g], nvalid=len(g) != 2)
            assert same_bits(part, whole[:, g]), groups
            assert nv_part is None or np.array_equal(nv_part, nv)


@pytest.mark.parametrize("qs,slots", [((0, 0.1, 0.25, 0.5, 0.9), 9), ((0.05, 0.1, 0.25, Fraction(1, 3), 0.5, 0.6827, 0.9, 0.95, 1), 17)])
def test_label_quantiles_in_chunks_of_eight(dev, qs, slots):
    """More slots than one call takes: 9 and 17 (q = 0 and q = 1 take one slot, the others two)."""
    from satmvs_amd import dsm
    assert len(qs) + sum(1 for q in qs if q not in (0, 1)) == slots
    c = [c for c in _matrix() if c["name"] == "kit voids 0.3"][0]
    for method in qo.METHODS:
        want = qo.quantiles(c["labels"], c["n"], c["values"], qs, method)
        got = dsm.label_quantiles(c["labels"], c["n"], c["values"], qs, method)
        _same_quantiles(got, want, (slots, method))


def _same_quantiles(got, want, what):
    assert set(got) == set(want) == {"n_valid", "lo", "hi", "value"}
    got = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in got.items()}
    assert got["n_valid"].dtype == np.int32 and got["lo"].dtype == got["hi"].dtype == np.float32 and got["value"].dtype == np.float64, what
    assert np.array_equal(got["n_valid"], want["n_valid"]), what
    for key in ("lo", "hi"):
        d = qo.differing(got[key], got["n_valid"], want[key], want["n_valid"])
        assert d is None, (what, key, d)
    assert got["value"].shape == want["value"].shape and np.array_equal(got["value"].view(np.uint64), want["value"].view(np.uint64)), what


# ---- closed form on the device ------------------------------------------------------------------------------------------------------
def test_closed_form_at_2300(dev):
    """2300 x 2300: value (r, c) = (7919 c) mod 2300, label r // 100 + 1.  7919 is prime to 2300, so every row, and every label a
    hundred times over, holds each of 0 .. 2299: rank t is t // 100.  More cells than 2^22, 1292 workgroups, zones of whole rows."""
    from satmvs_amd import _lib
    g, n, R = 2300, 23, 8
    r, c = torch.meshgrid(torch.arange(g, device=dev), torch.arange(g, device=dev), indexing="ij")
    values = ((7919 * c) % g).float().contiguous()
    labels = (r // 100 + 1).to(torch.int32).contiguous()
    m = 100 * g
    k = torch.arange(n, device=dev)
    ranks = torch.stack([torch.zeros_like(k), k * 0 + 99, k * 0 + 100, k * 0 + m - 1, k * 0 + m, k * 0 - 1, (k * 9973 + 17) % m, (k * 104729) % m], dim=1).to(torch.int32).contiguous()
    nbytes = _lib.load().smvs_dsm_label_select_workspace_bytes(n, R)
    ws = torch.full((nbytes + 2 * G,), 0xa5, dtype=torch.uint8, device=dev)
    out, nv = _guarded(n * R, torch.float32, dev), _guarded(n, torch.int32, dev)
    _lib.call("smvs_dsm_label_select", _lib.ptr(labels), _lib.ptr(values), g, g, ND, n, None, _lib.ptr(ranks), R,
              _lib.ptr(out[G:]), _lib.ptr(nv[G:]), _lib.ptr(ws[G:]), nbytes, _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert _intact(out, n * R) and _intact(nv, n) and bool((ws[:G] == 0xa5).all()) and bool((ws[G + nbytes:] == 0xa5).all())
    inside = (ranks >= 0) & (ranks < m)
    want = torch.where(inside, (ranks // 100).float(), torch.full_like(ranks, ND, dtype=torch.float32))
    assert torch.equal(out[G:G + n * R].reshape(n, R).view(torch.int32), want.view(torch.int32))
    assert bool((nv[G:G + n] == m).all())


# ---- robustness of the entry --------------------------------------------------------------------------------------------------------
def test_workspace_contents_streams_and_order_of_calls(dev):
    big = [c for c in _matrix() if c["name"] == "kit voids 0.05"][0]
    small = [c for c in _matrix() if c["name"] == "hand-made map"][0]
    first = _check(dev, big, 8, 0, fill=0xff)
    for fill in (0x00, 0x5a):
        again = _check(dev, big, 8, 0, fill=fill)
        assert same_bits(again[0], first[0]) and np.array_equal(again[1], first[1])                 # equal bits, run after run
    _check(dev, small, 8, 0)                                 # a smaller call after a larger one
    _check(dev, small, 1, 1)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        on_side = _check(dev, big, 8, 0, stream=C.c_void_p(side.cuda_stream))
    assert same_bits(on_side[0], first[0])


def test_unaligned_grids_take_the_scalar_loads(dev):
    """labels and values that start 4 bytes past a 16-byte boundary: the other instance of the counting kernel."""
    for name in ("kit voids 0.05", "special 5x65", "one label over the grid"):
        c = [c for c in _matrix() if c["name"] == name][0]
        gh, gw = c["labels"].shape
        lab = torch.zeros(gh * gw + 1, dtype=torch.int32, device=dev)
        val = torch.zeros(gh * gw + 1, dtype=torch.float32, device=dev)
        lab[1:] = torch.from_numpy(c["labels"].reshape(-1)).to(dev)
        val[1:] = torch.from_numpy(c["values"].reshape(-1)).to(dev)
        lab_d, val_d = lab[1:].view(gh, gw), val[1:].view(gh, gw)
        assert lab_d.data_ptr() % 16 == 4 and val_d.data_ptr() % 16 == 4
        m = qo.n_valid(c["labels"], c["values"], c["n"])
        r = qo.rank_matrix(m, 7, 1)
        d = qo.differing(*_native(lab_d, val_d, c["n"], r), *qo.select_sorted(c["labels"], c["values"], c["n"], r))
        assert d is None, (name, d)


def test_without_nvalid(dev):
    c = [c for c in _matrix() if c["name"] == "hand-made map"][0]
    lab_d, val_d = torch.from_numpy(c["labels"]).to(dev), torch.from_numpy(c["values"]).to(dev)
    r = qo.rank_matrix(qo.n_valid(c["labels"], c["values"], c["n"]), 3, 0)
    out, nv = _native(lab_d, val_d, c["n"], r, nvalid=False)
    assert nv is None and same_bits(out, qo.select_sorted(c["labels"], c["values"], c["n"], r)[0])


def test_argument_rejections_write_nothing(dev, lib):
    from satmvs_amd import _lib
    gh, gw, n, R = 6, 9, 4, 2
    q = lib.smvs_dsm_label_select_workspace_bytes
    assert q(-1, 1) == 0 and q(1, 0) == 0 and q(1, 9) == 0 and q(2 ** 28, 1) == 0 and q(2 ** 25, 8) == 0 and q(2 ** 31 - 1, 8) == 0
    assert q(0, 1) > 0 and q(2 ** 25 - 1, 8) > 0 and q(n, R) >= 3 * 4 * n * R + 4 * n
    nbytes = q(n, R)
    lab, val = torch.ones((gh, gw), dtype=torch.int32, device=dev), torch.ones((gh, gw), dtype=torch.float32, device=dev)
    ranks = torch.zeros((n, R), dtype=torch.int32, device=dev)
    centre = torch.zeros(n, dtype=torch.float32, device=dev)
    out, nv, ws = _guarded(n * R, torch.float32, dev), _guarded(n, torch.int32, dev), _guarded(nbytes, torch.uint8, dev)
    p = _lib.ptr
    good = dict(labels=p(lab), values=p(val), gw=gw, gh=gh, nodata=ND, n=n, centre=p(centre), ranks=p(ranks), n_ranks=R, out=p(out[G:]),
                nvalid=p(nv[G:]), workspace=p(ws[G:]), workspace_bytes=nbytes)
    order = list(good)
    bad = [(dict(labels=None), "null pointer"), (dict(values=None), "null pointer"), (dict(ranks=None), "null pointer"), (dict(out=None), "null pointer"),
           (dict(workspace=None), "null pointer"), (dict(gw=0), "grid size"), (dict(gh=-1), "grid size"), (dict(gw=65536, gh=32768), "too large"),
           (dict(n=-1), "n must be"), (dict(n_ranks=0), "n_ranks"), (dict(n_ranks=9), "n_ranks"), (dict(n=2 ** 27, n_ranks=2), "2\\^28"),
           (dict(workspace_bytes=nbytes - 1), "workspace too small"), (dict(workspace_bytes=0), "workspace too small"),
           (dict(out=p(lab)), "out aliases labels"), (dict(out=p(val)), "out aliases values"), (dict(out=p(centre)), "out aliases centre"),
           (dict(out=p(ranks)), "out aliases ranks"), (dict(nvalid=p(out[G:])), "nvalid aliases out"), (dict(nvalid=p(lab)), "nvalid aliases labels"),
           (dict(workspace=p(out[G:])), "workspace aliases out"),
           # the workspace is longer than ranks or values: it may reach into whatever the allocator put behind them first
           (dict(workspace=p(ranks)), "workspace aliases (labels|values|centre|ranks)"), (dict(workspace=p(val)), "workspace aliases (labels|values)")]
    for change, message in bad:
        args = dict(good)
        args.update(change)
        with pytest.raises(_lib.SatMVSNativeError, match=message):
            _lib.call("smvs_dsm_label_select", *[args[k] for k in order], _lib.current_stream(dev))
    # n = 0: SMVS_OK and no launch
    args = dict(good, n=0)
    _lib.call("smvs_dsm_label_select", *[args[k] for k in order], _lib.current_stream(dev))
    torch.cuda.synchronize()
    for buf in (out, nv, ws):
        assert bool((buf == 77).all())
    assert bool((lab == 1).all()) and bool((val == 1).all()) and not bool(ranks.any()) and not bool(centre.any())


# ---- the Python layer end to end ------------------------------------------------------------------------------------------------------
def test_device_tensors_in_and_out(dev):
    from satmvs_amd import dsm
    c = [c for c in _matrix() if c["name"] == "deviation from the median"][0]
    lab_d, val_d, cen_d = (torch.from_numpy(c[k]).to(dev) for k in ("labels", "values", "centre"))
    for centre_d, centre in ((None, None), (cen_d, c["centre"])):
        got = dsm.label_quantiles(lab_d, c["n"], val_d, (0.25, 0.5), "midpoint", centre_d)
        assert all(t.is_cuda for t in got.values())
        _same_quantiles(got, qo.quantiles(c["labels"], c["n"], c["values"], (0.25, 0.5), "midpoint", centre), "device tensors")
    s = dsm.label_nmad(lab_d, c["n"], val_d)
    assert all(t.is_cuda for t in s.values())
    empty = dsm.label_quantiles(lab_d, 0, val_d, (0.5, 1))
    assert empty["lo"].shape == (0, 2) and empty["value"].shape == (0, 2) and empty["n_valid"].shape == (0,)


def test_nmad_against_the_two_step_statement(dev):
    from satmvs_amd import dsm
    for name in ("kit voids 0.05", "hand-made map", "special 33x129", "one label over the grid, scene", "all values equal"):
        c = [c for c in _matrix() if c["name"] == name][0]
        got = dsm.label_nmad(c["labels"], c["n"], c["values"])
        want = qo.nmad(c["labels"], c["n"], c["values"])
        assert set(got) == set(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (name, k, got[k], want[k])
    assert (want["mad"] == 0.0).all() and not np.signbit(want["mad"]).any()      # a constant zone: +0.0


def test_objects_of_an_ndsm(dev):
    """extract_dtm -> ndsm -> extract_objects -> label_quantiles(q = (0.5, 0.9)) against the oracle on the device's own nDSM.  The
    scene stands on a level ground of 130 m, so the cells of its 6 x 6 block are 40 m above it: the block's median in closed
    form."""
    from dsm_testkit import scene
    from satmvs_amd import dsm
    gh, gw = 96, 128
    r, c = np.meshgrid(np.arange(gh, dtype=np.float64), np.arange(gw, dtype=np.float64), indexing="ij")
    z = scene(5.0 * c, -5.0 * r, holes=False, amp=0.0)
    grid = dsm.DSMGrid(400000.0, 3500000.0, 5.0, 5.0, gw, gh)
    zd = torch.from_numpy(z).to(dev)
    above = dsm.ndsm(zd, dsm.extract_dtm(zd, grid))
    labels, stats = dsm.extract_objects(above, grid)
    n = int(stats["area"].numel())
    got = dsm.label_quantiles(labels, n, above, (0.5, 0.9))
    lab, a = labels.cpu().numpy(), above.cpu().numpy()
    _same_quantiles(got, qo.quantiles(lab, n, a, (0.5, 0.9)), "objects")
    block = int(lab[gh // 2, gw // 2])
    assert block > 0 and int((lab == block).sum()) == 36
    print("the block's nDSM cells:", np.unique(a[lab == block]).tolist())
    assert got["value"][block - 1].tolist() == [40.0, 40.0] and int(got["n_valid"][block - 1]) == 36


def test_exposure_of_facets(dev):
    """facets -> label_quantiles of sun_exposure: the median exposure per roof face."""
    from satmvs_amd import dsm
    gh, gw = 96, 128
    z = qo.kit_scene(gh, gw, 5, voids=0.02, salt=0.01)
    grid = dsm.DSMGrid(400000.0, 3500000.0, 5.0, 5.0, gw, gh)
    zd = torch.from_numpy(z).to(dev)
    labels, n = dsm.facets(zd, grid, tol=2.0)
    assert n > 1
    exposure = dsm.sun_exposure(zd, grid, [(135.0, 30.0), (180.0, 45.0), (225.0, 30.0)])
    assert exposure.dtype == torch.float32
    got = dsm.label_quantiles(labels, n, exposure, (0.5,), "nearest")
    _same_quantiles(got, qo.quantiles(labels.cpu().numpy(), n, exposure.cpu().numpy(), (0.5,), "nearest"), "facets")


ERRORS = np.array([-3.0, -1.0, -0.5, 0.0, 0.0, 0.25, 0.5, 1.0, 2.0, 40.0], np.float32)


def test_robust_metrics_of_a_planted_error_field(dev):
    """A DSM displaced by errors drawn from a fixed list, every value equally often: median, NMAD and LE90 by counting (the
    counting is in tests/test_dsm_quantile_cpu.py, which holds the oracle to it)."""
    from satmvs_amd import dsm
    gt = np.full((20, 30), 100.0, np.float32)
    est = gt + np.resize(ERRORS, gt.shape).astype(np.float32)
    for e, g in ((est, gt), (torch.from_numpy(est).to(dev), torch.from_numpy(gt).to(dev))):
        r = dsm.dsm_metrics_robust(e, g)
        assert r == qo.metrics_robust(est, gt)
        assert r["n"] == 600 and r["median"] == 0.125 and r["nmad"] == 1.4826 * 0.75 and r["le90"] == 3.0 + 37.0 * (1.0 / 10.0)
    est[3, 4] = np.nan
    gt[5, 6] = ND
    gt[7, 8] = 1099.0                                        # d = -999: a difference like any other, not nodata
    r = dsm.dsm_metrics_robust(est, gt)
    assert r == qo.metrics_robust(est, gt) and r["n"] == 598
    none = dsm.dsm_metrics_robust(np.full((3, 3), ND, np.float32), gt[:3, :3])
    assert none["n"] == 0 and all(np.isnan(none[k]) for k in ("median", "nmad", "le68", "le90", "le95"))


def test_nmad_holds_where_rmse_does_not(dev):
    """1 % salt of 30 - 80 m over an error of N(0, 0.5 m).  Replacing k of the n differences moves every order statistic by at
    most k ranks, so the salted median lies between the clean order statistics at the levels 1/2 -+ (k + 1) / n, and the salted
    MAD between those of the clean deviations, widened by how far the median can have moved: a band round the planted spread
    that the oracle computes from the clean differences.  NMAD stays inside it; dsm_metrics' RMSE leaves it."""
    from dsm_testkit import valid
    from satmvs_amd import dsm
    gh, gw = 120, 150
    rng = np.random.default_rng(8)
    gt = qo.kit_scene(gh, gw, None)
    noise = rng.normal(0.0, 0.5, (gh, gw)).astype(np.float32)
    salt = np.where(rng.random((gh, gw)) < 0.01, rng.uniform(30.0, 80.0, (gh, gw)) * rng.choice([-1.0, 1.0], (gh, gw)), 0.0).astype(np.float32)
    clean, salted = (gt + noise).astype(np.float32), (gt + noise + salt).astype(np.float32)
    zone = valid(gt, ND).astype(np.int32)
    assert same_bits(clean[salt == 0], salted[salt == 0])    # the other differences are the clean ones, bit for bit
    d_clean = (clean.astype(np.float64) - gt.astype(np.float64)).astype(np.float32)
    n, k = int(zone.sum()), int(((salt != 0) & (zone == 1)).sum())
    assert 0 < k < n // 50
    half, s = Fraction(1, 2), Fraction(k + 1, n)
    centre = qo.quantiles(zone, 1, d_clean, (half - s, half, half + s), nodata=np.nan)
    median = centre["value"][0, 1]
    moved = max(float(centre["hi"][0, 2]) - median, median - float(centre["lo"][0, 0]))
    spread = qo.quantiles(zone, 1, d_clean, (half - s, half + s), centre=np.array([median], np.float32), nodata=np.nan)
    slack = 1e-5                                             # the float32 roundings of the centre and of the deviations
    band = (1.4826 * (float(spread["lo"][0, 0]) - moved - slack), 1.4826 * (float(spread["hi"][0, 1]) + moved + slack))
    want = qo.metrics_robust(salted, gt)
    got = dsm.dsm_metrics_robust(torch.from_numpy(salted).to(dev), torch.from_numpy(gt).to(dev))
    assert got == want and got["n"] == n
    plain = dsm.dsm_metrics(torch.from_numpy(salted).to(dev), torch.from_numpy(gt).to(dev), ND)
    d = (salted.astype(np.float64) - gt.astype(np.float64))[zone == 1]
    assert abs(plain["rmse"] - float(np.sqrt((d * d).mean()))) <= 1e-9
    print("nmad %.4f in the band %.4f .. %.4f; rmse %.4f" % (got["nmad"], band[0], band[1], plain["rmse"]))
    assert 0.4 < band[0] < band[1] < 0.6                     # the band is round the planted 0.5 m
    assert band[0] <= got["nmad"] <= band[1]
    assert plain["rmse"] > band[1]
    g5 = dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, gw, gh)
    both = dsm.compare_dsms_robust(salted, g5, gt, g5, register=False)
    assert both["shift"] is None and both["before"] == want and both["after"] == want
