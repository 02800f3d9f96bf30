"""The census plane sweep and SGM on the MI355X (smvs_sgm_census_cost, smvs_sgm_aggregate, smvs_sgm_select, satmvs_amd.sgm) against
the numpy oracle (tests/sgm_oracle.py): every output by np.array_equal, heights by their bits, no voxel or pixel excused.  The case
matrix of tests/sgm_scene.py, chunks that tile the planes unevenly, guard words round every output and the workspace, side
streams, repeated calls, a larger call before a smaller one, device tensors, every host check, and the end-to-end scene: equal
bits with the oracle on the GPU's own warped volumes, the quality conditions, a pinhole sweep, and the chain into a DSM."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import sgm_oracle as so
import sgm_scene as sc
from dsm_testkit import dev, lib  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ERR_ARG = 1
GUARD = 64
FILL16 = 0x7777


def _guarded(n, dtype, fill, d):
    """A buffer of n elements with GUARD more at both ends, all `fill` -> (the whole tensor, the pointer to element GUARD)."""
    t = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=d)
    return t, C.c_void_p(t.data_ptr() + GUARD * t.element_size())


def _inner(t, n, fill, what):
    """The n elements between the guards, on the host, after checking that the guards still hold `fill`."""
    h = t.cpu().numpy()
    assert (h[:GUARD] == fill).all() and (h[n + GUARD:] == fill).all(), "%s: written outside its buffer" % what
    return h[GUARD:n + GUARD]


def _on(stream):
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


def _u16(h):
    return h.view(np.uint16)


def _census_c(ref, warped, radius, cov_min, D=None, d_begin=0, cost=None, stream=None, ws_fill=0xff):
    """The C entry on host arrays: cost (all D planes, FILL16 where the call writes nothing) and the workspace inside guard words.
    `cost`: the (tensor, pointer) of an earlier chunk, to go on with."""
    from satmvs_amd import _lib
    d = torch.device("cuda", 0)
    B, H, W = ref.shape
    Dc = warped[0].shape[2]
    D = Dc if D is None else D
    n = B * H * W * D
    rd = torch.from_numpy(np.ascontiguousarray(ref, np.float32)).to(d)
    wd = [torch.from_numpy(np.ascontiguousarray(w, np.float32)).to(d) for w in warped]
    nbytes = _lib.load().smvs_sgm_census_workspace_bytes(B, H, W)
    assert nbytes >= 8 * B * H * W and nbytes % 256 == 0
    ws, ws_p = _guarded(nbytes, torch.uint8, ws_fill, d)
    cost = _guarded(n, torch.int16, FILL16, d) if cost is None else cost
    torch.cuda.synchronize()
    with _on(stream):
        _lib.call("smvs_sgm_census_cost", _lib.ptr(rd), _lib.ptr_array(wd), len(wd), radius, float(cov_min), cost[1], B, H, W, d_begin, Dc, D,
                  ws_p, nbytes, _lib.current_stream(d))
    torch.cuda.synchronize()
    _inner(ws, nbytes, ws_fill, "workspace")
    return _u16(_inner(cost[0], n, FILL16, "cost")).reshape(B, H, W, D), cost


def _aggregate_c(cost, P1, P2, paths=8, guide=None, alpha=0, p2_min=None, cost_max=768, void_cost=96, stream=None):
    from satmvs_amd import _lib
    d = torch.device("cuda", 0)
    B, H, W, D = cost.shape
    cd = torch.from_numpy(np.ascontiguousarray(cost).view(np.int16)).to(d)
    gd = None if guide is None else torch.from_numpy(np.ascontiguousarray(guide)).to(d)
    out, out_p = _guarded(cost.size, torch.int16, FILL16, d)
    torch.cuda.synchronize()
    with _on(stream):
        _lib.call("smvs_sgm_aggregate", _lib.ptr(cd), None if gd is None else _lib.ptr(gd), out_p, B, H, W, D, P1, P2, P1 if p2_min is None else p2_min,
                  alpha, cost_max, void_cost, paths, _lib.current_stream(d))
    torch.cuda.synchronize()
    return _u16(_inner(out, cost.size, FILL16, "sum")).reshape(cost.shape)


def _select_c(total, depth, uniqueness=0, cost=None, min_support=1, want_min_sum=True, want_support=True, stream=None):
    """-> (index, height, min_sum or None, support or None); support only with cost."""
    from satmvs_amd import _lib
    d = torch.device("cuda", 0)
    B, H, W, D = total.shape
    n = B * H * W
    sd = torch.from_numpy(np.ascontiguousarray(total).view(np.int16)).to(d)
    cd = None if cost is None else torch.from_numpy(np.ascontiguousarray(cost).view(np.int16)).to(d)
    zd = torch.from_numpy(np.ascontiguousarray(depth, np.float32)).to(d)
    index, index_p = _guarded(n, torch.int32, -7, d)
    height, height_p = _guarded(n, torch.float32, 12345.0, d)
    ms, ms_p = _guarded(n, torch.int16, FILL16, d) if want_min_sum else (None, None)
    sp, sp_p = _guarded(n, torch.int16, FILL16, d) if want_support and cost is not None else (None, None)
    torch.cuda.synchronize()
    with _on(stream):
        _lib.call("smvs_sgm_select", _lib.ptr(sd), None if cd is None else _lib.ptr(cd), _lib.ptr(zd), 1 if depth.ndim == 4 else 0, uniqueness, min_support,
                  index_p, height_p, ms_p, sp_p, B, H, W, D, _lib.current_stream(d))
    torch.cuda.synchronize()
    shape = (B, H, W)
    return (_inner(index, n, -7, "index").reshape(shape), _inner(height, n, np.float32(12345.0), "height").reshape(shape),
            None if ms is None else _u16(_inner(ms, n, FILL16, "min_sum")).reshape(shape), None if sp is None else _u16(_inner(sp, n, FILL16, "support")).reshape(shape))


def _compare_select(got, want, what, fields=("index", "height", "min_sum", "support")):
    for g, w, f in zip(got, want, fields):
        assert (g is None) == (w is None), (what, f)
        if g is not None:
            sc.compare(g, w, "%s: %s" % (what, f))


# ---- census ------------------------------------------------------------------------------------------------------------------------
def test_census_against_the_oracle(dev):
    for name, ref, warped, radius, cov_min in sc.census_matrix():
        sc.compare(_census_c(ref, warped, radius, cov_min)[0], so.census_cost(ref, warped, radius, cov_min), name)


@pytest.mark.parametrize("chunks", [(7, 8, 5), (9, 11), (1, 16, 3), (20,), (8, 8, 4), (8, 9, 7), (16, 8), (3, 21)])
def test_chunks_tile_the_planes(dev, chunks):
    """D = 20 (and 24, where whole groups of 8 planes go out as 16-byte stores) in uneven chunks: every call writes its planes and
    leaves the others alone (FILL16 until their turn), in any order."""
    D = sum(chunks)
    ref, warped, cov_min = sc.census_case(400, 2, 11, 37, D, 2)
    want = so.census_cost(ref, warped, 2, cov_min)
    assert not (want == FILL16).any()
    begins = np.concatenate([[0], np.cumsum(chunks)[:-1]])
    done = np.zeros(D, bool)
    cost = None
    for k in np.argsort(-begins, kind="stable"):                                 # the last chunk first
        d0, dc = int(begins[k]), int(chunks[k])
        got, cost = _census_c(ref, [np.ascontiguousarray(w[:, :, d0:d0 + dc]) for w in warped], 2, cov_min, D=D, d_begin=d0, cost=cost)
        done[d0:d0 + dc] = True
        sc.compare(got[..., done], want[..., done], "planes written so far")
        assert (got[..., ~done] == FILL16).all(), "a plane outside the chunk was written"


# ---- aggregate ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(4))
def test_aggregate_against_the_oracle(dev, part):
    for name, cost, kw in sc.aggregate_matrix()[part::4]:
        sc.compare(_aggregate_c(cost, **kw), so.aggregate(cost, **kw), name)


def test_a_guide_of_equal_bytes_is_no_guide(dev):
    rng = np.random.default_rng(410)
    cost = sc.valley_cost(rng, 1, 12, 19, 65)
    want = so.aggregate(cost, 16, 96, 8)
    sc.compare(_aggregate_c(cost, 16, 96, 8, guide=np.full((1, 12, 19), 200, np.uint8), alpha=7, p2_min=16), want, "equal bytes")
    sc.compare(_aggregate_c(cost, 16, 96, 8), want, "no guide")


# ---- select ------------------------------------------------------------------------------------------------------------------------
def test_select_against_the_oracle(dev):
    for name, total, depth, kw in sc.select_matrix():
        want = so.select(total, depth, **kw)
        _compare_select(_select_c(total, depth, **kw), want, name)
        bare = _select_c(total, depth, want_min_sum=False, want_support=False, **kw)
        assert bare[2] is None and bare[3] is None
        _compare_select(bare[:2], want[:2], name + ", no optional output")
        if kw.get("cost") is not None:
            one = _select_c(total, depth, want_min_sum=False, **kw)
            sc.compare(one[3], want[3], name + ": support alone")
            _compare_select(one[:2], want[:2], name + ", support alone")


# ---- call hygiene ------------------------------------------------------------------------------------------------------------------
def test_streams_repeats_and_a_smaller_call_after_a_larger(dev):
    side = torch.cuda.Stream(dev)
    ref, warped, cov_min = sc.census_case(420, 2, 40, 70, 12, 3)
    small = sc.census_case(421, 1, 5, 9, 3, 1)
    want = so.census_cost(ref, warped, 3, cov_min)
    runs = [_census_c(ref, warped, 3, cov_min, ws_fill=f)[0] for f in (0xff, 0x00, 0x5a)] + [_census_c(ref, warped, 3, cov_min, stream=side)[0]]
    for got in runs:
        sc.compare(got, want, "census repeats")
    sc.compare(_census_c(small[0], small[1], 1, small[2])[0], so.census_cost(small[0], small[1], 1, small[2]), "the smaller census call")
    rng = np.random.default_rng(422)
    big, little = sc.valley_cost(rng, 2, 40, 70, 70), sc.random_cost(rng, 1, 5, 9, 7)
    guide = sc.guide_image(rng, 2, 40, 70)
    kw = dict(P1=10, P2=120, paths=8, guide=guide, alpha=3, p2_min=20)
    want = so.aggregate(big, **kw)
    for got in (_aggregate_c(big, **kw), _aggregate_c(big, **kw), _aggregate_c(big, stream=side, **kw)):
        sc.compare(got, want, "aggregate repeats")
    sc.compare(_aggregate_c(little, 16, 96, 4), so.aggregate(little, 16, 96, 4), "the smaller aggregate call")
    depth = np.linspace(100, 300, 70, dtype=np.float32)[None].repeat(2, 0)
    wsel = so.select(want, depth, 10, big, 60)
    for got in (_select_c(want, depth, 10, big, 60), _select_c(want, depth, 10, big, 60, stream=side)):
        _compare_select(got, wsel, "select repeats")
    tiny = so.aggregate(little, 16, 96, 4)
    _compare_select(_select_c(tiny, np.arange(7, dtype=np.float32)[None]), so.select(tiny, np.arange(7, dtype=np.float32)[None]), "the smaller select call")


def test_python_layer_on_device_tensors_and_host_arrays(dev):
    from satmvs_amd import sgm
    rng = np.random.default_rng(430)
    cost = sc.valley_cost(rng, 2, 17, 23, 40)
    guide = sc.guide_image(rng, 2, 17, 23)
    depth = np.linspace(50, 90, 40, dtype=np.float32)[None].repeat(2, 0)
    want = so.aggregate(cost, 16, 96, 8, guide=guide, alpha=2, p2_min=30)
    got = sgm.aggregate(cost, guide=guide, alpha=2, p2_min=30)
    assert isinstance(got, np.ndarray)
    sc.compare(got, want, "aggregate, host arrays")
    on = sgm.aggregate(torch.from_numpy(cost.view(np.int16)).to(dev), guide=torch.from_numpy(guide).to(dev), alpha=2, p2_min=30)
    assert isinstance(on, torch.Tensor) and on.is_cuda and on.dtype == torch.int16
    sc.compare(on.cpu().numpy().view(np.uint16), want, "aggregate, device tensors")
    sc.compare(sgm.aggregate(cost, paths=4, void_cost=10), so.aggregate(cost, 16, 96, 4, void_cost=10), "aggregate, 4 paths")
    wsel = so.select(want, depth, 5, cost, 39)
    _compare_select(sgm.select(want, depth, 5, cost, 39), wsel, "select, host arrays")
    dsel = sgm.select(on, torch.from_numpy(depth).to(dev), 5, torch.from_numpy(cost.view(np.int16)).to(dev), 39)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in dsel)
    _compare_select((dsel[0].cpu().numpy(), dsel[1].cpu().numpy(), dsel[2].cpu().numpy().view(np.uint16), dsel[3].cpu().numpy().view(np.uint16)), wsel, "select, device tensors")
    bare = sgm.select(want, depth)
    assert bare[3] is None
    _compare_select(bare[:3], so.select(want, depth)[:3], "select without cost")


def test_rejections_write_nothing(dev, lib):
    B, H, W, D, Dc = 1, 8, 9, 8, 4
    f = lambda *s: torch.full(s, 77.0, dtype=torch.float32, device=dev)      # noqa: E731
    h = lambda *s: torch.full(s, 77, dtype=torch.int16, device=dev)          # noqa: E731
    ref, w0, w1 = f(B, H, W), f(B, 2, Dc, H, W), f(B, 2, Dc, H, W)
    cost, total = h(B, H, W, D), h(B, H, W, D)
    nbytes = lib.smvs_sgm_census_workspace_bytes(B, H, W)
    ws = torch.full((nbytes,), 77, dtype=torch.uint8, device=dev)
    index = torch.full((B, H, W), 77, dtype=torch.int32, device=dev)
    height, depth = f(B, H, W), f(B, D)
    ms, sp = h(B, H, W), h(B, H, W)
    guide = torch.full((B, H, W), 77, dtype=torch.uint8, device=dev)
    P = lambda t: t.data_ptr()                                # noqa: E731
    ptrs = lambda *t: (C.c_void_p * 7)(*[P(x) for x in t])    # noqa: E731

    def census(**c):
        a = dict(dict(ref=P(ref), warped=ptrs(w0, w1), n_src=2, radius=2, cov_min=0.999, cost=P(cost), d_begin=0, Dc=Dc, D=D, ws=P(ws), nbytes=nbytes), **c)
        return lib.smvs_sgm_census_cost(a["ref"], a["warped"], a["n_src"], a["radius"], a["cov_min"], a["cost"], B, H, W, a["d_begin"], a["Dc"], a["D"], a["ws"], a["nbytes"], None)

    def aggregate(**c):
        a = dict(dict(cost=P(cost), guide=P(guide), sum=P(total), P1=16, P2=96, p2_min=16, alpha=1, cost_max=768, void_cost=96, paths=8), **c)
        return lib.smvs_sgm_aggregate(a["cost"], a["guide"], a["sum"], B, H, W, D, a["P1"], a["P2"], a["p2_min"], a["alpha"], a["cost_max"], a["void_cost"], a["paths"], None)

    def select(**c):
        a = dict(dict(sum=P(total), cost=P(cost), depth=P(depth), is4d=0, u=10, ms=1, index=P(index), height=P(height), min_sum=P(ms), support=P(sp)), **c)
        return lib.smvs_sgm_select(a["sum"], a["cost"], a["depth"], a["is4d"], a["u"], a["ms"], a["index"], a["height"], a["min_sum"], a["support"], B, H, W, D, None)

    bad = [(census, c) for c in (dict(ref=None), dict(cost=None), dict(ws=None), dict(n_src=0), dict(n_src=8), dict(radius=0), dict(radius=4), dict(cov_min=float("nan")),
                                 dict(d_begin=-1), dict(d_begin=5), dict(Dc=0), dict(D=257), dict(nbytes=nbytes - 1), dict(warped=ptrs(w0, w0)), dict(warped=ptrs(w0, ref)),
                                 dict(cost=P(ref)), dict(ws=P(cost)), dict(cost=P(w1) + 64))]
    bad += [(aggregate, c) for c in (dict(cost=None), dict(sum=None), dict(paths=5), dict(P1=-1), dict(P1=17), dict(p2_min=97), dict(alpha=-1), dict(void_cost=769),
                                     dict(P2=65535 // 8 - 768 + 1), dict(paths=4, P2=65535 // 4 - 768 + 1), dict(sum=P(cost)), dict(sum=P(cost) + 2), dict(guide=P(total) + 8))]
    bad += [(select, c) for c in (dict(sum=None), dict(depth=None), dict(index=None), dict(height=None), dict(is4d=2), dict(u=-1), dict(u=100), dict(ms=-1), dict(cost=None),
                                  dict(index=P(total)), dict(height=P(index)), dict(min_sum=P(sp)), dict(support=P(depth)))]
    for fn, change in bad:
        assert fn(**change) == ERR_ARG and lib.smvs_last_error().decode(), (fn.__name__, change)
    torch.cuda.synchronize()
    for t in (cost, total, ws, index, height, ms, sp):
        assert (t == 77).all()                                # nothing ran
    assert census() == 0 and census(Dc=1, d_begin=7, n_src=1) == 0
    assert aggregate() == 0 and aggregate(guide=None) == 0 and aggregate(P2=65535 // 8 - 768) == 0 and aggregate(paths=4, P2=65535 // 4 - 768) == 0
    assert select() == 0 and select(min_sum=None, support=None) == 0 and select(cost=None, support=None) == 0
    torch.cuda.synchronize()


# ---- the scene ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    return sc.scene()


def _gpu_warps(dev, images, rpc, ref_v, depth):
    """The GPU's own warped [image, ones] volumes of the other views into view ref_v, on the host."""
    from satmvs_amd.modules import warping
    out = []
    for v in range(len(images)):
        if v != ref_v:
            fea = torch.from_numpy(np.stack([images[v], np.ones_like(images[v])])[None]).to(dev)
            out.append(warping.rpc_warping(fea, torch.from_numpy(rpc[v:v + 1]).to(dev), torch.from_numpy(rpc[ref_v:ref_v + 1]).to(dev), torch.from_numpy(depth).to(dev)).cpu().numpy())
    return out


def test_scene_equals_the_oracle_and_meets_the_conditions(dev, scene):
    from satmvs_amd import sgm
    images, rpc, truth = scene
    depth = sc.planes()
    got = sgm.sgm_heights([im[None] for im in images], rpc[None], depth)
    want, raw, cost, total = sc.oracle_heights(images[0][None], _gpu_warps(dev, images, rpc, 0, depth), depth)
    _compare_select((got["index"], got["height"], got["min_sum"], got["support"]), want, "sgm_heights")
    sc.check_quality(got["height"][0], raw[1][0], truth[0])
    on = sgm.sgm_heights([torch.from_numpy(im[None]).to(dev) for im in images], torch.from_numpy(rpc[None]).to(dev), torch.from_numpy(depth).to(dev), plane_chunk=7)
    assert on["height"].is_cuda
    sc.compare(on["height"].cpu().numpy(), want[1], "device tensors, chunks of 7")
    per_pixel = np.ascontiguousarray(np.broadcast_to(depth[:, :, None, None], (1, sc.D, sc.H, sc.W)))
    sc.compare(sgm.sgm_heights([im[None] for im in images], rpc[None], per_pixel, plane_chunk=48)["height"], want[1], "per-pixel planes, one chunk")


def test_a_pinhole_sweep(dev):
    """An identity reference and two sources that see a fronto-parallel plane at depth 50 shifted by +-600 / depth pixels (12 px
    there, 0.24 px per plane of 1 unit: the parallax per plane of the RPC scene): the oracle on the GPU's homography warps bit for
    bit, and the scene's own condition, 90 % within two planes of the truth, away from the columns the sources do not see."""
    from satmvs_amd import sgm
    from satmvs_amd.modules import warping
    H, W, D, z0 = 40, 72, 21, 50.0
    rng = np.random.default_rng(440)
    tex = sc._gauss_fields(rng, (H, 4 * W), (1.5, 5.0, 16.0))

    def view(shift):                                                            # I(x) = tex(x + shift), linear between the columns
        x = np.arange(W) + W + shift
        x0 = np.floor(x).astype(int)
        return ((1 - (x - x0)) * tex[:, x0] + (x - x0) * tex[:, x0 + 1]).astype(np.float32)

    eye = np.eye(4)
    mats = [eye] + [np.array([[1.0, 0, 0, t], [0, 1.0, 0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]]) for t in (600.0, -600.0)]
    images = [view(0.0), view(-600.0 / z0), view(600.0 / z0)]                   # a source sees pixel x of the reference at x + t / depth
    depth = np.linspace(40.0, 60.0, D, dtype=np.float32)[None]
    pm = np.stack(mats)[None]
    got = sgm.sgm_heights([im[None] for im in images], pm, depth, geo_model="pinhole")
    warped = []
    for v in (1, 2):
        fea = torch.from_numpy(np.stack([images[v], np.ones_like(images[v])])[None]).to(dev)
        warped.append(warping.homo_warping(fea, torch.from_numpy(pm[:, v]).to(dev), torch.from_numpy(pm[:, 0]).to(dev), torch.from_numpy(depth).to(dev)).cpu().numpy())
    want = sc.oracle_heights(images[0][None], warped, depth)[0]
    _compare_select((got["index"], got["height"], got["min_sum"], got["support"]), want, "pinhole")
    inner = got["index"][0, 4:-4, 16:-16]
    assert (np.abs(inner - D // 2) <= 2).mean() >= 0.9, float((np.abs(inner - D // 2) <= 2).mean())


def test_the_chain_into_a_dsm(dev, scene):
    """sgm_heights with each view as the reference -> rpc_filter.filter_depth -> dsm.heights_to_dsm: the cells of the DSM lie within
    three plane spacings of the DSM of the true heights at the median."""
    from satmvs_amd import dsm, rpc_filter, sgm
    from satmvs_amd.transverse_mercator import Ellipsoid, TransverseMercator
    proj = TransverseMercator(Ellipsoid(6378137.0, 298.257223563), 0.0, 114.0, 0.9996, 500000.0, 0.0)      # the scene lies on the meridian 114 E
    images, rpc, truth = scene
    depth = sc.planes()
    heights = []
    for v in range(3):
        order = [v] + [k for k in range(3) if k != v]
        heights.append(sgm.sgm_heights([images[k][None] for k in order], rpc[order][None], depth)["height"][0])
    maps, masks = [], []
    for v in range(3):
        order = [v] + [k for k in range(3) if k != v]
        mask, averaged = rpc_filter.filter_depth([heights[k] for k in order], [rpc[k] for k in order], 1.0, 2 * sc.DH, 1)      # a pixel, and two plane spacings in metres, in one other view
        maps.append(averaged.astype(np.float32))
        masks.append(mask & np.isfinite(averaged))
    assert min(m[sc.BORDER:-sc.BORDER, sc.BORDER:-sc.BORDER].mean() for m in masks) > 0.5
    grid = dsm.grid_for(truth, list(rpc), proj, 2.0)
    est = dsm.heights_to_dsm(maps, list(rpc), proj, grid, masks=masks)
    ref = dsm.heights_to_dsm(truth, list(rpc), proj, grid)
    both = (est != -999.0) & (ref != -999.0)
    assert both.sum() > 0.4 * (ref != -999.0).sum()
    err = np.abs(est[both].astype(np.float64) - ref[both])
    print("DSM: %d cells, median |error| %.3f m (%.2f DH)" % (both.sum(), np.median(err), np.median(err) / sc.DH))
    assert np.median(err) <= 3 * sc.DH
