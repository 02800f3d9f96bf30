"""The seeded flood on the device against the Python statements of the rule (tests/dsm_watershed_oracle.py): every compared array
by np.array_equal, the surface by its bits, no cell excused.  The case matrix of tests/dsm_watershed_scene.py through the three C
entries (guard words round every output and the workspace, workspaces full of anything), the batching of the rounds, null
outputs, a side stream, rejections that write nothing, the Python layer on numpy and on device tensors, the tie to
fill_depressions, and peaks -> watershed -> split_objects -> outlines end to end."""
import ctypes

import numpy as np
import pytest
import torch

import dsm_hydro_oracle as ho
import dsm_label_oracle as lo
import dsm_watershed_oracle as wo
import dsm_watershed_scene as sc
from dsm_testkit import dev, lib, same_bits                  # noqa: F401

pytestmark = pytest.mark.gpu

OUT = ("surface", "steps", "backlink")
_shared = {}


def _grid(gh, gw, xres=5.0, yres=5.0):
    from satmvs_amd import dsm
    return dsm.DSMGrid(400000.0, 3500000.0, xres, yres, gw, gh)


def _reference(case):
    """The arguments and the statement's outputs of a case, computed once and left alone."""
    if case not in _shared:
        args = sc.case(case)
        _shared[case] = (args, wo.chain(**args))
    return _shared[case]


def _native(args, dev, batch=8, fill=0x5a, stream=None, outputs=OUT + ("unreached",), G=64, max_rounds=None):     # noqa: F811
    """The three entries called directly, every output and the workspace between guard words, the workspace full of `fill`.
    -> the outputs (and keys, n_seeds, n_unreached, rounds) as numpy."""
    from satmvs_amd import _lib
    lib = _lib.load()                                        # noqa: F811
    p = _lib.ptr
    stream = stream or _lib.current_stream(dev)
    z = args["z"]
    gh, gw = z.shape
    n = gh * gw
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    zd, md, dd = up(z), up(args["marker"]), up(args["domain"])
    q = lambda t: ctypes.c_void_p(0) if t is None else p(t)  # noqa: E731
    pol, off = int(args["polarity"]), int(args["offset"])
    spec = {"keys": (torch.int64, n), "count": (torch.int32, 1), "status": (torch.int32, 1), "surface": (torch.float32, n), "steps": (torch.int32, n),
            "backlink": (torch.uint8, n), "unreached": (torch.int32, 1)}
    bufs = {k: torch.full((m + 2 * G,), 77, dtype=dt, device=dev) for k, (dt, m) in spec.items()}
    optional = OUT + ("unreached",)
    at = {k: (p(bufs[k][G:]) if k not in optional or k in outputs else ctypes.c_void_p(0)) for k in spec}
    nbytes = lib.smvs_dsm_seed_workspace_bytes(gw, gh)
    ws = torch.full((nbytes + 512,), fill, dtype=torch.uint8, device=dev)
    _lib.call("smvs_dsm_seed_begin", p(zd), p(md), q(dd), gw, gh, -999.0, pol, off, at["keys"], at["count"], p(ws[256:]), nbytes, stream)
    rounds = 0
    while True:
        _lib.call("smvs_dsm_seed_rounds", p(zd), gw, gh, -999.0, pol, at["keys"], batch, at["status"], p(ws[256:]), nbytes, stream)
        rounds += batch
        torch.cuda.synchronize()
        if int(bufs["status"][G].item()) == 0 or (max_rounds and rounds >= max_rounds):
            break
        assert rounds <= n + 2 + batch
    _lib.call("smvs_dsm_seed_read", p(zd), p(md), q(dd), gw, gh, -999.0, pol, off, at["keys"], at["surface"], at["steps"], at["backlink"], at["unreached"],
              p(ws[256:]), nbytes, stream)
    torch.cuda.synchronize()
    for k, (dt, m) in spec.items():
        assert bool((bufs[k][:G] == 77).all()) and bool((bufs[k][G + m:] == 77).all()), k
        if k in optional and k not in outputs:
            assert bool((bufs[k] == 77).all()), k             # a null output: nothing written anywhere near
    assert bool((ws[:256] == fill).all()) and bool((ws[256 + nbytes:] == fill).all())
    out = {k: bufs[k][G:G + m].cpu().numpy().reshape(gh, gw) for k, (dt, m) in spec.items() if m == n and (k not in OUT or k in outputs)}
    out["keys"] = out["keys"].view(np.uint64)
    out["n_seeds"], out["rounds"], out["status"] = int(bufs["count"][G].item()), rounds, int(bufs["status"][G].item())
    if "unreached" in outputs:
        out["n_unreached"] = int(bufs["unreached"][G].item())
    return out


def _want(chain, names=("keys",) + OUT):
    return {k: chain[k] for k in names}


# ---- the matrix ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.ALL_CASES, ids=sc.case_id)
def test_the_matrix_against_the_statement(dev, case):        # noqa: F811
    args, want = _reference(case)
    got = _native(args, dev)
    assert wo.differing(got, _want(want)) == []
    assert got["n_seeds"] == want["n_seeds"] and got["n_unreached"] == want["n_unreached"]


def test_a_seedless_half_stays_at_infinity_after_64_rounds(dev):     # noqa: F811
    """The domain cuts the component in two and only the left half holds seeds: after 64 rounds, long past the fixed point, the
    right half is at exactly 0xfffffffe00000000; without any seed the whole grid is, and n_unreached is the valid count."""
    args, want = _reference(("domain",))
    for batch in (1, 64):
        got = _native(args, dev, batch=batch, max_rounds=64) if batch == 64 else _native(args, dev, batch=1)
        assert wo.differing(got, _want(want)) == [] and got["status"] == 0
        assert (got["keys"][:, 35:] == wo.INF_KEY).all() and got["n_unreached"] == 40 * 35 and (got["backlink"][:, 35:] == 255).all()
    args, want = _reference(("constant", "none"))
    got = _native(args, dev, batch=64)
    assert got["rounds"] == 64 and (got["keys"] == wo.INF_KEY).all() and got["n_unreached"] == args["z"].size and got["n_seeds"] == 0
    assert (got["surface"] == sc.NODATA).all() and (got["steps"] == -1).all() and (got["backlink"] == 255).all()


def test_the_spiral_corridor(dev):                           # noqa: F811
    args, want = _reference(("spiral",))
    got = _native(args, dev, batch=64)
    print("spiral 97 x 97: d up to %d, %d rounds" % (got["steps"].max(), got["rounds"]))
    assert wo.differing(got, _want(want)) == [] and got["steps"].max() > 4000


# ---- calling conditions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("marker", -1, 700), ("grid", 63, 33, 8), ("town", 0.3, -1, -1, "random")], ids=sc.case_id)
def test_batches_workspaces_guards_and_a_side_stream(dev, case):     # noqa: F811
    """Batches of 1, 8 and 4096 rounds, workspaces full of 0xff, 0x00 and 0x5a, and a side stream: equal keys and outputs, equal
    to the statement, nothing written outside the outputs."""
    from satmvs_amd import _lib
    args, want = _reference(case)
    runs = [_native(args, dev, batch, fill) for batch, fill in ((1, 0xff), (8, 0x00), (4096, 0x5a), (8, 0xff))]
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        runs.append(_native(args, dev, 8, 0xff, _lib.current_stream(dev)))
    for got in runs:
        assert wo.differing(got, _want(want)) == []
        assert got["n_seeds"] == want["n_seeds"] and got["n_unreached"] == want["n_unreached"]


def test_every_output_null_and_non_null(dev):                # noqa: F811
    args, want = _reference(("marker", 1, -1))
    for outputs in ((), ("surface",), ("steps",), ("backlink",), ("unreached",), ("surface", "backlink"), OUT + ("unreached",)):
        got = _native(args, dev, outputs=outputs)
        assert wo.differing(got, _want(want, ("keys",) + tuple(k for k in outputs if k in OUT))) == []
        assert ("unreached" not in outputs) or got["n_unreached"] == want["n_unreached"]


def test_native_rejections_write_nothing(dev, lib):          # noqa: F811
    from satmvs_amd import _lib
    gw, gh = 9, 7
    n = gw * gh
    stream = _lib.current_stream(dev)
    p, null = _lib.ptr, ctypes.c_void_p(0)
    names = ("dsm", "marker", "domain", "keys", "count", "status", "surface", "steps", "link", "unreached", "ws")
    nbytes = lib.smvs_dsm_seed_workspace_bytes(gw, gh)
    buf = {k: torch.full((max(n, nbytes // 8 + 1),), 77, dtype=torch.int64, device=dev) for k in names}

    def begin(dsm=p(buf["dsm"]), marker=p(buf["marker"]), domain=p(buf["domain"]), gw=gw, gh=gh, polarity=1, offset=0, keys=p(buf["keys"]),
              count=p(buf["count"]), ws=p(buf["ws"]), nbytes=nbytes):
        _lib.call("smvs_dsm_seed_begin", dsm, marker, domain, gw, gh, -999.0, polarity, offset, keys, count, ws, nbytes, stream)

    def rounds(dsm=p(buf["dsm"]), gw=gw, gh=gh, polarity=1, keys=p(buf["keys"]), k=8, status=p(buf["status"]), ws=p(buf["ws"]), nbytes=nbytes):
        _lib.call("smvs_dsm_seed_rounds", dsm, gw, gh, -999.0, polarity, keys, k, status, ws, nbytes, stream)

    def read(dsm=p(buf["dsm"]), marker=p(buf["marker"]), domain=p(buf["domain"]), gw=gw, gh=gh, polarity=1, offset=0, keys=p(buf["keys"]),
             surface=p(buf["surface"]), steps=p(buf["steps"]), link=p(buf["link"]), count=p(buf["unreached"]), ws=p(buf["ws"]), nbytes=nbytes):
        _lib.call("smvs_dsm_seed_read", dsm, marker, domain, gw, gh, -999.0, polarity, offset, keys, surface, steps, link, count, ws, nbytes, stream)

    def rejected(call, match, **kw):
        with pytest.raises(_lib.SatMVSNativeError, match=match):
            call(**kw)

    inside = lambda k, off: ctypes.c_void_p(buf[k].data_ptr() + off)               # noqa: E731
    for name in ("dsm", "marker", "keys", "count", "ws"):
        rejected(begin, "null pointer", **{name: null})
    for name in ("dsm", "keys", "status", "ws"):
        rejected(rounds, "null pointer", **{name: null})
    for name in ("dsm", "marker", "keys", "ws"):
        rejected(read, "null pointer", **{name: null})
    for call in (begin, rounds, read):
        rejected(call, "polarity must be", polarity=0)
        rejected(call, "non-positive grid", gw=0)
        rejected(call, "below 2\\^30", gw=2 ** 15, gh=2 ** 15)
        rejected(call, "workspace too small", nbytes=nbytes - 1)
        rejected(call, "workspace aliases keys", ws=inside("keys", 8 * n - 1))
    for call in (begin, read):
        rejected(call, "offset must be within", offset=2 ** 25 + 1)
        rejected(call, "offset must be within", offset=-2 ** 25 - 1)
    rejected(begin, "keys aliases dsm", keys=inside("dsm", 4 * n - 1))
    rejected(begin, "n_seeds aliases marker", count=inside("marker", 4))
    rejected(rounds, "keys aliases dsm", keys=p(buf["dsm"]))
    rejected(rounds, "status aliases keys", status=inside("keys", 8))
    rejected(read, "surface aliases keys", surface=p(buf["keys"]))
    rejected(read, "backlink aliases level_steps", link=inside("steps", 4 * n - 1))
    rejected(read, "n_unreached aliases domain", count=inside("domain", n - 1))
    for k in (0, 4097):
        rejected(rounds, "rounds must be in", k=k)
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in buf.values())


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("marker", -1, 0), ("marker", 1, 0), ("quantum", -1), ("town", 0.0, -1, 0, "random")], ids=sc.case_id)
def test_reconstruct_on_numpy(dev, case):                    # noqa: F811
    from satmvs_amd import dsm
    args, want = _reference(case)
    method = "dilation" if args["polarity"] < 0 else "erosion"
    surface, steps, link, rounds = dsm.reconstruct(args["marker"], args["z"], method, return_steps=True, return_link=True, return_rounds=True)
    assert all(isinstance(a, np.ndarray) for a in (surface, steps, link)) and 1 <= rounds <= args["z"].size + 2 + 4096
    assert wo.differing({"surface": surface, "steps": steps, "backlink": link}, _want(want, OUT)) == []
    alone = dsm.reconstruct(args["marker"], args["z"], method, batch=3)
    assert isinstance(alone, np.ndarray) and same_bits(alone, want["surface"])


def test_a_larger_call_before_a_smaller_one_and_the_same_bits_twice(dev):     # noqa: F811
    from satmvs_amd import dsm
    big, want_big = _reference(("town", 0.3, -1, -1, "random"))
    small, want_small = _reference(("grid", 31, 65, 5))
    z, H = big["z"], 2.0
    hm = wo.chain(z, z, None, -1, wo.h_quanta(H))
    first = dsm.h_maxima(z, H)
    then = dsm.reconstruct(small["marker"], small["z"], "erosion", return_link=True)
    again = dsm.h_maxima(z, H)
    assert same_bits(first, hm["surface"]) and same_bits(again, first)
    ref = wo.chain(small["z"], small["marker"], None, 1, 0)
    assert same_bits(then[0], ref["surface"]) and np.array_equal(then[1], ref["backlink"])
    low = dsm.h_minima(z, H)
    assert same_bits(low, wo.chain(z, z, None, 1, wo.h_quanta(H))["surface"])
    with np.errstate(invalid="ignore"):
        v = ho.valid(z)
        assert (first[v] <= z[v]).all() and (low[v] >= z[v]).all() and (z[v] - first[v]).max() == H == (low[v] - z[v]).max()


def test_the_mask_is_the_domain_and_h_at_its_limits(dev):    # noqa: F811
    from satmvs_amd import dsm
    args, want = _reference(("domain",))
    got = dsm.reconstruct(args["marker"], args["z"], "dilation", mask=args["domain"] != 0, return_link=True)
    assert same_bits(got[0], want["surface"]) and np.array_equal(got[1], want["backlink"])
    z = sc.case(("grid", 33, 63, 7))["z"]
    for h in (1.0 / 256.0, 65536.0):
        assert same_bits(dsm.h_maxima(z, h), wo.chain(z, z, None, -1, wo.h_quanta(h))["surface"])


def test_device_tensors_in_and_out(dev, monkeypatch):        # noqa: F811
    """Tensors in, tensors out, and no grid goes to the host on the way (a Tensor.cpu() call fails the test)."""
    from satmvs_amd import dsm
    above = sc.terrace()
    grid = _grid(*above.shape)
    zd = torch.from_numpy(above).to(dev)

    def no_host_copy(self, *a, **k):
        raise AssertionError("a grid went to the host")
    monkeypatch.setattr(torch.Tensor, "cpu", no_host_copy)
    hm = dsm.h_maxima(zd, 2.0)
    tops, n, table, dome = dsm.peaks(zd, 2.0, grid)
    seg, level = dsm.watershed(zd, tops, return_level=True)
    labels, m, stats = dsm.split_objects(zd, grid)
    opened = dsm.open_by_reconstruction(zd, 2)
    monkeypatch.undo()
    assert all(t.is_cuda for t in (hm, tops, dome, seg, level, labels, opened, table["first"], stats["object"]))
    want_tops, want_n, want_table, want_dome = wo.peaks(above, 2.0)
    assert n == want_n and np.array_equal(tops.cpu().numpy(), want_tops) and same_bits(dome.cpu().numpy(), want_dome)
    want_seg, want_level = wo.watershed(above, want_tops)
    assert np.array_equal(seg.cpu().numpy(), want_seg) and same_bits(level.cpu().numpy(), want_level)
    assert m == 6 and np.array_equal(labels.cpu().numpy(), wo.split_objects(above, grid)[0])


def test_seeded_at_the_outlets_it_is_fill_depressions(dev):  # noqa: F811
    """The new kernel against the old one: seeds = the hydrology's outlets at their own height, on a grid without interior
    voids -> fill_depressions' filled surface and flat_dist, bit for bit."""
    from satmvs_amd import dsm
    z = ho.hills(130, 97, 4, 0.0, 12)
    v = ho.valid(z)
    assert v.all()
    marker = np.where(ho.outlets(v), z, sc.NODATA).astype(np.float32)
    surface, steps = dsm.reconstruct(marker, z, "erosion", return_steps=True)
    filled, depth, flat = dsm.fill_depressions(z, return_depth=True)
    assert same_bits(surface, filled) and np.array_equal(steps, flat) and (depth > 0).sum() > 100


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_peaks_and_watershed_on_the_two_cones(dev):          # noqa: F811
    from satmvs_amd import dsm
    s, z = sc.CONES, sc.two_cones()
    grid = _grid(*z.shape)
    for h in (6.0, 6.0 + 1.0 / 256.0, 20.0, 20.0 + 1.0 / 256.0):
        tops, n, table, dome = dsm.peaks(z, h, grid)
        want_tops, want_n, want_table, want_dome = wo.peaks(z, h)
        assert n == want_n and np.array_equal(tops, want_tops) and same_bits(dome, want_dome) and tops.dtype == np.int32
        assert sorted(table) == ["area", "east", "first", "height", "north"]
        for k in ("first", "area", "height"):
            assert table[k].dtype == want_table[k].dtype and np.array_equal(table[k], want_table[k]), k
        assert np.array_equal(table["east"], grid.e0 + table["first"][:, 1] * 5.0) and np.array_equal(table["north"], grid.n0 - table["first"][:, 0] * 5.0)
    tops, n, _, _ = dsm.peaks(z, 2.0)
    seg, level = dsm.watershed(z, tops, return_level=True)
    want_seg, want_level = wo.watershed(z, tops)
    assert n == 3 and np.array_equal(seg, want_seg) and same_bits(level, want_level) and seg.dtype == np.int32
    la, lb = tops[s["row"], s["col_a"]], tops[s["row"], s["col_b"]]
    assert (seg[s["row"], 2:s["saddle_col"]] == la).all() and (seg[s["row"], s["saddle_col"] + 1:s["col_b"] + 10] == lb).all()
    down = dsm.watershed(-z, tops, peaks_up=False)
    assert np.array_equal(down, seg)
    masked = dsm.watershed(z, tops, mask=z > 0)
    assert np.array_equal(masked, wo.watershed(z, tops, z > 0)[0]) and (masked[z == 0] == 0).all()
    high = dsm.peaks(z, 2.0, min_height=15.0)
    assert high[1] == 2 and np.array_equal(high[0], wo.peaks(z, 2.0, min_height=15.0)[0])


def test_split_objects_on_the_terrace(dev):                  # noqa: F811
    """Four gabled houses that share walls and two touching tree domes: two objects, six segments whose borders lie within one
    cell of the saddles; the result goes through outlines(), burn_rings() and label_quantiles() as it is."""
    from satmvs_amd import dsm
    above = sc.terrace()
    grid = _grid(*above.shape)
    objects, _ = dsm.extract_objects(above, grid)
    assert objects.max() == 2
    labels, n, table = dsm.split_objects(above, grid)
    want_labels, want_n, want_table = wo.split_objects(above, grid)
    assert n == want_n == 6 and np.array_equal(labels, want_labels) and labels.dtype == np.int32
    lo.same_stats(table, want_table, "split_objects")
    expected, loose = sc.terrace_expected()
    assert np.array_equal(labels[~loose], expected[~loose])
    assert all(labels[r, c] in (expected[r, c], expected[r, c - 1]) for r, c in np.argwhere(loose))
    assert table["object"].tolist() == [1, 1, 1, 1, 2, 2]
    rings = dsm.outlines(labels, n, grid)
    assert np.array_equal(dsm.burn_rings(rings["vertices"], rings["offset"], rings["label"], labels.shape), labels)
    per = dsm.label_quantiles(labels, n, above, q=(0.5, 1.0))
    assert per["value"].shape == (6, 2) and per["value"][:, 1].tolist() == [9.0, 9.0, 9.0, 9.0, 8.0, 7.5]
    assert dsm.split_objects(above, grid, h=2.25 + 1.0 / 256.0)[1] == 5
    opened = dsm.open_by_reconstruction(above, 2)
    assert same_bits(opened, wo.chain(above, dsm.morph(above, 2, "open"), None, -1, 0)["surface"])
    with np.errstate(invalid="ignore"):
        assert (opened <= above).all() and (opened[sc.TERRACE["row0"] + 2, :] == above[sc.TERRACE["row0"] + 2, :]).sum() > 30
