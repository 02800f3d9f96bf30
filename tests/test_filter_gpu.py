"""The geometric-consistency kernels (csrc/filter.hip: smvs_rpc_geo_consistency, smvs_pinhole_geo_consistency) beyond the one
64 x 96 fixture of tests/test_filter.py: stage-by-stage parity with no excepted pixels, end to end against the oracle with
the differing pixels tied to their cause, a shape matrix from 1 x 1 to 2048 x 2304 with sources of other sizes, bit-exact
remap answers, non-finite and degenerate maps, filter_depth over view counts / dtypes / streams, and the chain into the DSM.
Scenes, bounds and checks: tests/filter_scene.py; what they assume about the scenes: tests/test_filter_cpu.py."""
import numpy as np
import pytest
import torch

import filter_scene as fs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the GPU suite needs an MI355X")
    return torch.device("cuda", 0)


def _mod(kind):
    from satmvs_amd import pinhole_filter, rpc_filter
    return rpc_filter if kind == "rpc" else pinhole_filter


_IDS = lambda v: str(v).replace(" ", "")


@pytest.mark.parametrize("ref,src", fs.PAIRS, ids=_IDS)
@pytest.mark.parametrize("kind", ["rpc", "pinhole"])
def test_stage_by_stage_and_end_to_end(dev, oracle, kind, ref, src):
    g, dr, ds, p, d = fs.pair(kind, oracle, ref, src)
    msgs = fs.stages(g, _mod(kind), dr, ds, p, d)
    e2e, share, diff = fs.end_to_end(g, _mod(kind), dr, ds, p, d)
    print("%s %s <- %s: at-risk share %.3g, %d differing pixels" % (kind, ref, src, share, int(diff.sum())))
    assert not msgs + e2e, "\n".join(msgs + e2e)


@pytest.mark.parametrize("kind", ["rpc", "pinhole"])
def test_full_size_pair_against_oracle(dev, oracle, kind):
    g, dr, ds, p, d = fs.pair(kind, oracle, *fs.BIG)
    e2e, share, diff = fs.end_to_end(g, _mod(kind), dr, ds, p, d)
    print("%s %s: at-risk share %.3g, %d differing pixels" % (kind, fs.BIG[0], share, int(diff.sum())))
    assert not e2e, "\n".join(e2e)


@pytest.mark.parametrize("hw", fs.SHIFT_SIZES, ids=_IDS)
@pytest.mark.parametrize("shift", fs.SHIFTS, ids=_IDS)
def test_remap_known_answers(dev, hw, shift):
    from satmvs_amd import pinhole_filter
    dr, ref, src_map, src, xs, ys, val = fs.shift_case(hw[0], hw[1], *shift)
    dep, xb, yb, gx, gy = pinhole_filter.reproject_with_depth(dr, *ref, src_map, *src)
    assert np.array_equal(gx.view(np.uint32), xs.view(np.uint32)) and np.array_equal(gy.view(np.uint32), ys.view(np.uint32))
    bad = dep.view(np.uint32) != val.view(np.uint32)
    assert not bad.any(), "%d pixels, first %s: %r, expected %r" % (bad.sum(), tuple(np.argwhere(bad)[0]), dep[bad][0], val[bad][0])
    # the sample goes back to where it came from: x_back = x exactly where something was sampled; the rule is strict, so a
    # threshold equal to the distance (0) or to the relative difference itself rejects
    hit = val > 0
    H, W = dr.shape
    xr, yr = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    assert np.array_equal(xb[hit], xr[hit]) and np.array_equal(yb[hit], yr[hit])
    m, dm, _, _ = pinhole_filter.check_geometric_consistency(dr, *ref, src_map, *src, 0.0, 1e9)
    assert not m.any() and not dm.any()
    rel = np.abs(val - dr) / dr
    if hit.any():
        t = float(rel[hit].flat[0])                                                 # a float32 value: the rule compares in float32
        m, dm, _, _ = pinhole_filter.check_geometric_consistency(dr, *ref, src_map, *src, 1.0, t)
        assert np.array_equal(m[hit], (rel < np.float32(t))[hit]) and not m[hit & (rel == np.float32(t))].any()
        assert np.array_equal(dm[hit], np.where(m, val, np.float32(0))[hit])


def test_rpc_rule_is_strict_at_its_thresholds(dev, oracle):
    """A threshold equal to a pixel's own height difference / reprojection distance rejects that pixel (<, not <=)."""
    from satmvs_amd import rpc_filter
    g, dr, ds, p, d = fs.pair("rpc", oracle, (64, 96), (90, 131))
    dep, xb, yb, _, _ = rpc_filter.reproject_with_depth(dr, g.rpc_ref, ds, g.rpc_src)
    _, _, dist, dd = g.rule(dr, dep, xb, yb, p, d)
    inside = np.argwhere((dd > 0) & (dd < 1) & (dist > 0) & (dist < 1))
    assert len(inside) > 1000
    for i in (tuple(inside[0]), tuple(inside[len(inside) // 2]), tuple(inside[-1])):
        t = float(dd[i])
        m, _, _, _ = rpc_filter.check_geometric_consistency(dr, g.rpc_ref, ds, g.rpc_src, 1.0, t)
        want = (dist < 1.0) & (dd.astype(np.float64) < t)
        assert not m[i] and np.array_equal(m, want)
        m, _, _, _ = rpc_filter.check_geometric_consistency(dr, g.rpc_ref, ds, g.rpc_src, 1.0, float(np.nextafter(np.float32(t), np.float32(9))))
        assert m[i]
        t = float(dist[i])
        m, _, _, _ = rpc_filter.check_geometric_consistency(dr, g.rpc_ref, ds, g.rpc_src, t, 2.5)
        assert not m[i] and np.array_equal(m, (dist < t) & (dd < 2.5))
        assert rpc_filter.check_geometric_consistency(dr, g.rpc_ref, ds, g.rpc_src, float(np.nextafter(t, 9.0)), 2.5)[0][i]


@pytest.mark.parametrize("where", ["patch", "all"])
@pytest.mark.parametrize("what", fs.SPOILS, ids=str)
@pytest.mark.parametrize("kind", ["rpc", "pinhole"])
def test_non_finite_and_degenerate_maps(dev, oracle, kind, what, where):
    """Expected values come from the oracle, the raw sample at a non-finite coordinate (the border value) included."""
    g, dr, ds, p, d = fs.pair(kind, oracle, (64, 96), (40, 61))
    for side, a, b in (("reference", fs.spoil(dr, what, where), ds), ("source", dr, fs.spoil(ds, what, where))):
        msgs = fs.stages(g, _mod(kind), a, b, p, d, tag=" %s %s in the %s" % (where, what, side))
        msgs += fs.end_to_end(g, _mod(kind), a, b, p, d, tag=" %s %s in the %s" % (where, what, side), cap=False)[0]
        assert not msgs, "\n".join(msgs)
        dep, xb, yb, xs, ys = g.run_reproject(_mod(kind), a, b)
        m, dm, _, _ = g.run_check(_mod(kind), a, b, p, d)
        bad_coord = ~np.isfinite(xs) | ~np.isfinite(ys)
        assert (dep[bad_coord] == np.float32(g.border)).all()                       # not source pixel (0, 0)
        assert not np.isnan(dm).any() and not m[np.isnan(dep) | np.isnan(a)].any()


@pytest.mark.parametrize("kind", ["rpc", "pinhole"])
def test_source_that_does_not_overlap(dev, oracle, kind):
    g, dr, ds, p, d = fs.pair(kind, oracle, (64, 96), (70, 101), away=True)
    msgs = fs.stages(g, _mod(kind), dr, ds, p, d) + fs.end_to_end(g, _mod(kind), dr, ds, p, d)[0]
    assert not msgs, "\n".join(msgs)
    dep = g.run_reproject(_mod(kind), dr, ds)[0]
    m, dm, _, _ = g.run_check(_mod(kind), dr, ds, p, d)
    assert (dep == np.float32(g.border)).all() and not m.any() and not dm.any()


def _filter_diff(oracle, depths, rpcs, p, d):
    """Pixels of the reference where some pair's masked sample or mask differs between kernel and oracle, and the pixels where
    that is allowed (at risk)."""
    from satmvs_amd import rpc_filter
    diff, risk = np.zeros(depths[0].shape, bool), np.zeros(depths[0].shape, bool)
    for v in range(1, len(depths)):
        g = fs.Rpc(oracle, rpcs[0], rpcs[v])
        msgs, _, df = fs.end_to_end(g, rpc_filter, depths[0], depths[v], p, d, tag=" view %d" % v)
        assert not msgs, "\n".join(msgs)
        cx, cy = g.coords(depths[0])
        diff |= df
        risk |= g.at_risk(depths[0], cx, cy)
    return diff, risk


@pytest.mark.parametrize("V", sorted(fs.FILTER_VIEWS))
def test_filter_depth_view_counts_and_parameters(dev, oracle, V):
    from satmvs_amd import rpc_filter
    depths, rpcs, prob, _ = fs.rpc_scene(fs.FILTER_VIEWS[V], seed=2)
    keep = [x.copy() for x in depths], rpcs.copy(), prob.copy()
    diff, risk = _filter_diff(oracle, depths, rpcs, 1.0, 2.5)
    assert not (diff & ~risk).any()
    vals = np.unique(prob)
    ratios = (None, 0.3, float(vals[0]), float(np.nextafter(vals[0], np.float32(-1))), float(vals[len(vals) // 2]), float(vals[-1]), 2.0, -1.0)
    for n in range(1, V):
        for c in ratios:
            kw = {} if c is None else dict(prob=prob, confidence_ratio=c)
            f, a = rpc_filter.filter_depth(depths, rpcs, 1.0, 2.5, n, **kw)
            wf, wa = oracle.filter_depth(depths, rpcs, 1.0, 2.5, n, **kw)
            assert isinstance(f, np.ndarray) and isinstance(a, np.ndarray) and f.dtype == wf.dtype == np.bool_ and a.dtype == wa.dtype == np.float64
            assert np.array_equal(f[~diff], wf[~diff]) and np.array_equal(a[~diff].view(np.uint64), wa[~diff].view(np.uint64)), (n, c)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(depths, keep[0]))
    assert np.array_equal(rpcs, keep[1]) and np.array_equal(prob, keep[2])


def test_filter_depth_inputs_streams_and_determinism(dev, oracle):
    from satmvs_amd import rpc_filter
    sizes = fs.FILTER_VIEWS[3]
    depths, rpcs, prob, _ = fs.rpc_scene(sizes, seed=2)
    depths = [x.astype(np.float16).astype(np.float32) for x in depths]              # values every input dtype below can hold
    prob = prob.astype(np.float16).astype(np.float32)
    args = (1.0, 2.5, 2)
    f0, a0 = rpc_filter.filter_depth(depths, rpcs, *args, prob=prob, confidence_ratio=0.3)
    assert isinstance(f0, np.ndarray) and f0.any() and not f0.all()
    wf, wa = oracle.filter_depth(depths, rpcs, *args, prob=prob, confidence_ratio=0.3)
    diff, risk = _filter_diff(oracle, depths, rpcs, 1.0, 2.5)
    assert not (diff & ~risk).any() and np.array_equal(f0[~diff], wf[~diff]) and np.array_equal(a0[~diff], wa[~diff])

    def same(f, a):
        return np.array_equal(f, f0) and np.array_equal(a.view(np.uint64), a0.view(np.uint64))
    td = [torch.from_numpy(x).to(dev) for x in depths]
    tr, tp = torch.from_numpy(rpcs).to(dev), torch.from_numpy(prob).to(dev)
    keep = [x.clone() for x in td]
    assert same(*rpc_filter.filter_depth(td, tr, *args, prob=tp, confidence_ratio=0.3))                      # device tensors
    assert same(*rpc_filter.filter_depth(td, tr, *args, prob=tp, confidence_ratio=0.3))                      # twice
    assert same(*rpc_filter.filter_depth([x.double() for x in td], tr, *args, prob=tp.double(), confidence_ratio=0.3))
    assert same(*rpc_filter.filter_depth([x.half() for x in td], tr, *args, prob=tp.half(), confidence_ratio=0.3))
    assert same(*rpc_filter.filter_depth([x.astype(np.float64) for x in depths], [r for r in rpcs], *args, prob=prob.astype(np.float16), confidence_ratio=0.3))
    wide = [torch.cat([x, x + 1], dim=1)[:, :x.shape[1]] for x in td]                                           # non-contiguous views
    step = [torch.stack([x, x], dim=2)[:, :, 0] for x in td]
    assert not wide[0].is_contiguous() and not step[0].is_contiguous()
    assert same(*rpc_filter.filter_depth(wide, tr, *args, prob=torch.cat([tp, tp], dim=1)[:, :tp.shape[1]], confidence_ratio=0.3))
    assert same(*rpc_filter.filter_depth(step, tr, *args, prob=tp, confidence_ratio=0.3))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fs_, as_ = rpc_filter.filter_depth(td, tr, *args, prob=tp, confidence_ratio=0.3)
    side.synchronize()
    assert same(fs_, as_)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(td, keep))            # inputs left alone
    # the per-pair entries: device tensors in, the same bits as numpy in
    for mod, g in ((_mod("rpc"), fs.Rpc(oracle, rpcs[0], rpcs[2])),):
        a = g.run_reproject(mod, depths[0], depths[2])
        b = g.run_reproject(mod, td[0], td[2])
        c = g.run_reproject(mod, wide[0], step[2])
        assert all(np.array_equal(x, y, equal_nan=True) and np.array_equal(x, z, equal_nan=True) for x, y, z in zip(a, b, c))
    pd, K, E = fs.pinhole_scene(((64, 96), (40, 61)), seed=1)
    from satmvs_amd import pinhole_filter
    a = pinhole_filter.reproject_with_depth(pd[0], K[0], E[0], pd[1], K[1], E[1])
    t0, t1 = torch.from_numpy(pd[0]).to(dev), torch.from_numpy(pd[1]).to(dev)
    b = pinhole_filter.reproject_with_depth(torch.cat([t0, t0], dim=1)[:, :96], torch.from_numpy(K[0]), torch.from_numpy(E[0]), t1.double(), K[1], E[1])
    with torch.cuda.stream(side):
        c = pinhole_filter.reproject_with_depth(t0, K[0], E[0], t1, K[1], E[1])
    side.synchronize()
    assert all(np.array_equal(x, y, equal_nan=True) and np.array_equal(x, z, equal_nan=True) for x, y, z in zip(a, b, c))


def test_filter_to_dsm_chain_five_views(dev, oracle):
    """filter_depth on five views of their own sizes -> heights_to_dsm, against the oracle's filter -> the DSM oracle, in every
    cell that no differing pixel falls into."""
    import dsm_oracle
    from satmvs_amd import dsm, rpc_filter
    from satmvs_amd.transverse_mercator import Ellipsoid, TransverseMercator
    depths, rpcs, prob, _ = fs.rpc_scene(fs.FILTER_VIEWS[5], seed=2)
    f, a = rpc_filter.filter_depth(depths, rpcs, 1.0, 2.5, 3, prob=prob, confidence_ratio=0.3)
    wf, wa = oracle.filter_depth(depths, rpcs, 1.0, 2.5, 3, prob=prob, confidence_ratio=0.3)
    diff, risk = _filter_diff(oracle, depths, rpcs, 1.0, 2.5)
    assert not (diff & ~risk).any() and f.any() and not f.all()
    proj = TransverseMercator(Ellipsoid(), 0.0, float(np.round(rpcs[0][3])), 0.9996, 500000.0, 0.0)
    a32, wa32 = a.astype(np.float32), wa.astype(np.float32)
    (east, north), = dsm.project_to_map([wa32], [rpcs[0]], proj, [np.ones_like(wf)])
    east, north = east.cpu().numpy(), north.cpu().numpy()
    res = float(east.max() - east.min()) / 14.0
    grid = dsm.grid_from_extent(east.min(), east.max(), north.min(), north.max(), res)
    for mode in ("median", "mean", "min", "max"):
        got, cnt = dsm.heights_to_dsm([a32], [rpcs[0]], proj, grid, masks=[f], mode=mode, return_count=True)
        cells = dsm_oracle.cells(np.where(wf, east, np.nan), np.where(wf, north, np.nan), grid.grid4(), grid.width, grid.height)
        want, wcnt = dsm_oracle.reduce(cells, wa32, grid.width * grid.height, mode, -999.0)
        want, wcnt = want.reshape(grid.height, grid.width), wcnt.reshape(grid.height, grid.width)
        touched = np.zeros(grid.width * grid.height, bool)
        all_cells = dsm_oracle.cells(east, north, grid.grid4(), grid.width, grid.height)
        touched[all_cells[diff & (all_cells >= 0)]] = True
        sel = ~touched.reshape(grid.height, grid.width)
        assert sel.mean() > 0.9 and np.array_equal(cnt[sel], wcnt[sel]) and cnt.sum() > 0.3 * f.size
        if mode == "mean":
            assert (np.abs(got[sel].astype(np.float64) - want[sel]) <= np.spacing(np.abs(want[sel]))).all()        # one ulp, as tests/test_dsm_gpu.py
        else:
            assert np.array_equal(got[sel].view(np.uint32), want[sel].view(np.uint32)), mode
