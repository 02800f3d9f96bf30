"""The stream network on the device against the Python statement of the rule (tests/dsm_stream_oracle.py): the order map, the
link map, every per-link table, the vertices and the flow-length counts are compared by np.array_equal (float64 metres by their
bits), no cell, link or vertex excused.

Sizes.  Every kernel runs 256 lanes a workgroup over the cells or the tour's 2 gw gh elements; the scans (mouths, marks at
tour positions, heads, offsets) work in blocks of 2048 on three levels.  SIZES holds the issue's grids and three of 1023, 1024
and 1025 cells (11 x 93, 32 x 32, 25 x 41) whose tours of a full mask straddle a scan block; masks of 2047, 2048 and 2049
stream cells do the same to the marks' scan whatever the grid.  The 2300 x 2300 plane has more than 2048^2 tour elements: the
scans' second level holds more than one block.  The serpentine at 257 x 301 is the deepest chain a grid of this size has."""
import ctypes
import json
import time

import numpy as np
import pytest
import torch

import dsm_hydro_oracle as ho
import dsm_stream_oracle as so
from dsm_testkit import dev, scene as kit_scene  # noqa: F401  (dev: fixture)

pytestmark = pytest.mark.gpu
G = 64                                                       # guard words on both sides of an output
XRES, YRES = ho.XRES, ho.YRES


def _grid(dsm, gh, gw, xres=XRES, yres=YRES):
    return dsm.DSMGrid(500000.0, 3400000.0, xres, yres, gw, gh)


def _check(code, mask, what, cycles="raise"):
    """stream_links() and stream_order() of numpy inputs against the oracle's array statement -> the device's dict."""
    from satmvs_amd import dsm
    want = so.network(code, mask)
    got = dsm.stream_links(code, mask, cycles=cycles)
    assert all(isinstance(t, np.ndarray) for t in got.values()) and sorted(got) == sorted(so.KEYS), what
    assert so.differing(got, {k: want[k] for k in so.KEYS}) == [], what
    assert np.array_equal(dsm.stream_order(code, mask, cycles=cycles), want["order_map"]), what
    return got


def _check_length(code, what, cycles="raise"):
    from satmvs_amd import dsm
    want, _ = so.flow_length_doubling(code)
    got = dsm.flow_length(code, cycles=cycles)
    assert so.differing({"steps": got}, {"steps": want}) == [], what
    for xres, yres in ((5.0, 2.5), (0.3, 0.5)):                # float64 metres by bits against the same numpy expression
        metres = dsm.flow_length(code, grid=_grid(dsm, *code.shape, xres, yres), cycles=cycles)
        expect = np.where(want[..., 0] < 0, -1.0, so.length_m(want, xres, yres))
        expect = np.where(code > 8, np.nan, expect)
        assert so.differing({"metres": metres}, {"metres": expect}) == [], (what, xres, yres)
    return got


# ---- random scenes, sizes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", so.RANDOM_SCENES)
def test_random_scenes(dev, case):
    code, acc = so.hill_codes(*case)
    top = 0
    for name, mask in so.masks_of(code, acc):
        got = _check(code, mask, (case, name))
        top = max(top, int(got["order_map"].max()))
        if name == "all zeros":
            assert len(got["head"]) == 0 and list(got["offset"]) == [0] and got["vertices"].shape == (0, 2) and not got["link"].any()
    assert top >= (3 if case[3] < 0.3 else 2)
    _check_length(code, case)


@pytest.mark.parametrize("shape", so.SIZES)
def test_sizes(dev, shape):
    gh, gw = shape
    code, acc = so.hill_codes(gh, gw, gh + gw, 0.02 if gh * gw > 500 else 0.0, 12)
    got = _check(code, np.ones(shape, bool), (shape, "all ones"))
    _check(code, acc >= 2, (shape, "acc >= 2"))
    _check_length(code, shape)
    if min(shape) <= 2:                                       # every cell an outlet: every cell a link of one vertex
        assert len(got["head"]) == gh * gw and (got["next_link"] == -1).all() and not got["steps"].any()


@pytest.mark.parametrize("cells", [2047, 2048, 2049])
def test_stream_cell_counts_round_a_scan_block(dev, cells):
    code, _ = so.hill_codes(60, 70, 11, 0.03, None)
    mask = so.first_tree_cells(code, cells)
    got = _check(code, mask, cells)
    assert (got["order_map"] > 0).sum() == cells


# ---- closed forms ----------------------------------------------------------------------------------------------------------------
def test_htree(dev):
    code, root = so.htree(7)
    got = _check(code, code <= 8, "H-tree")
    order, nxt = got["order"], got["next_link"]
    inner = nxt >= 0
    assert got["order_map"][root] == 8 and len(order) == 255 and inner.sum() == 254 and (order[nxt[inner]] == order[inner] + 1).all()
    assert [int((order == k).sum()) for k in range(1, 9)] == [128, 64, 32, 16, 8, 4, 2, 1]
    _check_length(code, "H-tree")


def test_comb(dev):
    z = ho.comb(257, 301)
    code, _ = so.code_of(z)
    got = _check(code, z < 150.0, "comb")
    assert len(got["head"]) == 2 * 150 - 1 and got["order"].max() == 2 and (got["order"] == 1).sum() == 150 and (got["order_map"][255, 3:] == 2).all()
    _check_length(code, "comb")


def _seconds(fn, repeats=3):
    best = None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best or 1e9, time.perf_counter() - t)
    return best


def test_serpentine_is_one_link_and_no_slower(dev):
    """The deepest chain of a 257 x 301 grid: one link through every channel cell in river order.  Both grids have the same
    number of cells, so the same launches: the chain may cost what its one link's 38 000 integer adds into three words cost,
    not a launch more -- well inside twice the random scene plus 20 ms."""
    from satmvs_amd import dsm
    code, path = so.serpentine_codes(257, 301)
    got = _check(code, code <= 8, "serpentine")
    assert len(got["head"]) == 1 and got["order"][0] == 1 and np.array_equal(got["vertices"], np.array([(c, r) for r, c in reversed(path)], np.int32))
    steps = _check_length(code, "serpentine")
    assert list(steps[path[-1]]) == list(got["steps"][0]) == [len(path) - 1 - 2 * 127, 2 * 127, 0] and list(steps[path[0]]) == [0, 0, 0]
    hills, acc = so.hill_codes(*so.RANDOM_SCENES[-1])
    cd, md = torch.from_numpy(code).to(dev), torch.from_numpy(code <= 8).to(dev)
    hd, hm = torch.from_numpy(hills).to(dev), torch.from_numpy(acc >= 1).to(dev)
    chain, random = _seconds(lambda: dsm.stream_links(cd, md)), _seconds(lambda: dsm.stream_links(hd, hm))
    print("stream_links 257 x 301: serpentine %.2f ms, random hills %.2f ms" % (chain * 1e3, random * 1e3))
    assert chain <= 2 * random + 0.02


def test_junction_closed_forms(dev):
    for name, (code, cell, order) in so.junction_codes().items():
        got = _check(code, code <= 8, name)
        assert got["order_map"][cell] == order, name
    code, cell, _ = so.junction_codes()["a mouth with eight inflows"]
    got = _check(code, code <= 8, "mouth")
    k = got["link"][cell] - 1                                 # a junction that is itself a mouth: a link of one vertex
    assert got["offset"][k + 1] - got["offset"][k] == 1 and got["next_link"][k] == -1 and list(got["head"][:3]) == [6, 7, 8]
    lone = _check(np.zeros((3, 4), np.uint8), np.array([[0, 0, 0, 0], [0, 1, 0, 1], [0, 0, 0, 0]]), "two unconnected cells")
    assert list(lone["offset"]) == [0, 1, 2] and list(lone["head"]) == [5, 7]


def test_large_plane_closed_form(dev):
    """2300 x 2300 on the device only: every cell drains west, the first column off the grid.  Every row is one link of order 1
    from its east end to its west end, no junction anywhere; the flow length of a cell is its column."""
    from satmvs_amd import dsm
    g = 2300
    code = torch.full((g, g), 5, dtype=torch.uint8, device=dev)
    links = dsm.stream_links(code, torch.ones((g, g), dtype=torch.bool, device=dev))
    assert all(t.is_cuda for t in links.values())
    row, col = torch.arange(g, device=dev, dtype=torch.int32), torch.arange(g, device=dev, dtype=torch.int32)
    assert torch.equal(links["order_map"], torch.ones_like(code)) and torch.equal(links["link"], (row + 1)[:, None].expand(g, g))
    assert torch.equal(links["head"], row * g + (g - 1)) and torch.equal(links["order"], torch.ones_like(row)) and torch.equal(links["next_link"], -torch.ones_like(row))
    assert torch.equal(links["offset"], torch.arange(g + 1, device=dev, dtype=torch.int32) * g)
    want = torch.stack([col.flip(0)[None, :].expand(g, g), row[:, None].expand(g, g)], dim=2).reshape(-1, 2)
    assert links["vertices"].dtype == torch.int32 and torch.equal(links["vertices"], want)
    assert torch.equal(links["steps"], torch.tensor([g - 1, 0, 0], dtype=torch.int32, device=dev).expand(g, 3))
    steps = dsm.flow_length(code)
    assert steps.dtype == torch.int32 and torch.equal(steps[..., 0], col[None, :].expand(g, g)) and not steps[..., 1:].any()


# ---- edited directions -----------------------------------------------------------------------------------------------------------
def test_cycles_voids_and_roots(dev):
    from satmvs_amd import dsm
    code = so.cyclic_grid()
    plain, cyc = ho.accumulate_subtrees(code)
    rng = np.random.default_rng(3)
    for mask in (np.ones(code.shape, bool), rng.random(code.shape) < 0.7, plain > 2):
        with pytest.raises(ValueError, match="cycle"):
            dsm.stream_links(code, mask)
        with pytest.raises(ValueError, match="cycle"):
            dsm.stream_order(code, mask)
        got = _check(code, mask, "cyclic grid", cycles="mark")
        assert cyc and not got["order_map"][plain == -1].any() and not got["link"][plain == -1].any()
    with pytest.raises(ValueError, match="cycle"):
        dsm.flow_length(code)
    steps = _check_length(code, "cyclic grid", cycles="mark")
    assert np.array_equal(steps[..., 0] == -1, plain <= 0) and (plain == -1).sum() >= 62
    codes = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 9, 254, 255], np.uint8)
    rng = np.random.default_rng(5)
    for _ in range(6):                                        # anything at all
        shape = tuple(rng.integers(1, 60, 2))
        code = rng.choice(codes, shape)
        _check(code, rng.random(shape) < 0.8, "random codes", cycles="mark")
        _check_length(code, "random codes", cycles="mark")


# ---- robustness ------------------------------------------------------------------------------------------------------------------
def _native(dev, code, mask, fill, short=(0, 0)):
    """The entries called directly: guard words round every output and the workspace, the workspace full of `fill` -> the
    outputs under the oracle's names, the counts and the flags.  short = (links, vertices) to take off the counts given to write."""
    from satmvs_amd import _lib
    lib = _lib.load()
    p, stream = _lib.ptr, _lib.current_stream(dev)
    gh, gw = code.shape
    n = gh * gw
    cd, md = torch.from_numpy(code).to(dev), torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).to(dev)
    nbytes = lib.smvs_dsm_stream_workspace_bytes(gw, gh)
    ws = torch.full((nbytes + 512,), fill, dtype=torch.uint8, device=dev)

    def guarded(spec):
        bufs = {k: torch.full((m + 2 * G,), 77, dtype=dt, device=dev) for k, (dt, m) in spec.items()}
        return bufs, {k: p(bufs[k][G:]) for k in spec}

    def intact(spec, bufs):
        for k, (dt, m) in spec.items():
            assert bool((bufs[k][:G] == 77).all()) and bool((bufs[k][G + m:] == 77).all()), k
        assert bool((ws[:256] == fill).all()) and bool((ws[256 + nbytes:] == fill).all())

    spec1 = {"order_map": (torch.uint8, n), "link": (torch.int32, n), "counts": (torch.int32, 4), "flag": (torch.int32, 1), "length": (torch.int32, 3 * n),
             "flag2": (torch.int32, 1)}
    b1, at = guarded(spec1)
    _lib.call("smvs_dsm_stream_order", p(cd), p(md), gw, gh, at["order_map"], at["link"], at["counts"], at["flag"], p(ws[256:]), nbytes, stream)
    _lib.call("smvs_dsm_flow_length", p(cd), gw, gh, at["length"], at["flag2"], p(ws[256:]), nbytes, stream)
    torch.cuda.synchronize()
    intact(spec1, b1)
    counts = [int(x) for x in b1["counts"][G:G + 4].tolist()]
    nl, nv = counts[1] - short[0], counts[2] - short[1]
    spec2 = {"head": (torch.int32, nl), "order": (torch.int32, nl), "next_link": (torch.int32, nl), "offset": (torch.int32, nl + 1), "vertices": (torch.int32, 2 * nv),
             "steps": (torch.int32, 3 * nl)}
    b2, at2 = guarded(spec2)
    ws[256:256 + nbytes] = fill                               # write reads nothing of the order call
    _lib.call("smvs_dsm_stream_write", p(cd), p(md), gw, gh, nl, nv, at2["head"], at2["order"], at2["next_link"], at2["offset"], at2["vertices"], at2["steps"],
              p(ws[256:]), nbytes, stream)
    torch.cuda.synchronize()
    intact(spec2, b2)
    out = {k: b1[k][G:G + m].cpu().numpy() for k, (dt, m) in spec1.items()}
    out.update({k: b2[k][G:G + m].cpu().numpy() for k, (dt, m) in spec2.items()})
    out.update(order_map=out["order_map"].reshape(gh, gw), link=out["link"].reshape(gh, gw), vertices=out["vertices"].reshape(-1, 2), steps=out["steps"].reshape(-1, 3),
               length=out["length"].reshape(gh, gw, 3), counts=np.array(counts, np.int64))
    return out


def test_entries_keep_to_their_outputs(dev):
    code, acc = so.hill_codes(97, 131, 4, 0.04, 12)
    mask = (acc >= 3).astype(np.uint8)
    mask[::3] *= 2                                            # any non-zero byte marks a stream cell
    mask[1::3] *= 255
    want = so.network(code, mask)
    length, _ = so.flow_length_doubling(code)
    for fill in (0xff, 0x00, 0x5a):
        got = _native(dev, code, mask, fill)
        assert so.differing(got, dict({k: want[k] for k in so.KEYS}, counts=want["counts"], length=length)) == [], "workspace full of 0x%02x" % fill
        assert got["flag"][0] == 0 and got["flag2"][0] == 0
    cyc = _native(dev, so.cyclic_grid(), np.ones((40, 47), np.uint8), 0x5a)
    assert cyc["flag"][0] == 1 and cyc["flag2"][0] == 1 and so.differing(cyc, {k: so.network(so.cyclic_grid(), np.ones((40, 47)))[k] for k in so.KEYS}) == []
    for short in ((1, 0), (0, 1)):                            # counts one too small: -1 behind the offsets and nothing else, guards intact
        got = _native(dev, code, mask, 0x5a, short)
        assert got["offset"][-1] == -1 and (got["offset"][:-1] == 77).all() and (got["vertices"] == 77).all() and (got["head"] == 77).all()


def test_counts_that_do_not_fit_are_raised(dev, monkeypatch):
    from satmvs_amd import _lib, dsm
    code, acc = so.hill_codes(*so.RANDOM_SCENES[0])
    real = dsm._stream_order
    for cut in ((1, 0), (0, 1)):
        def fewer(*args, **kw):
            order, link, (cells, nl, nv, top) = real(*args, **kw)
            return order, link, [cells, nl - cut[0], nv - cut[1], top]
        monkeypatch.setattr(dsm, "_stream_order", fewer)
        with pytest.raises(_lib.SatMVSNativeError, match="counts differ"):
            dsm.stream_links(code, acc >= 4)
    monkeypatch.setattr(dsm, "_stream_order", real)
    _check(code, acc >= 4, "and the same call unharmed")


def test_deterministic_streams_and_device_tensors(dev):
    from satmvs_amd import dsm
    big, big_acc = so.hill_codes(300, 340, 1, 0.02, 12)
    small, small_acc = so.hill_codes(*so.RANDOM_SCENES[1])
    grid = _grid(dsm, 300, 340)
    bd, bm = torch.from_numpy(big).to(dev), torch.from_numpy(big_acc >= 2).to(dev)
    sd, sm = torch.from_numpy(small).to(dev), torch.from_numpy((small_acc >= 2).astype(np.int16) * 7).to(dev)
    keep_d, keep_m = bd.clone(), bm.clone()

    def run(d, m, g):
        out = dsm.stream_links(d, m, grid=g)
        out["length"] = dsm.flow_length(d)
        out["only_order"] = dsm.stream_order(d, m)
        return out

    a = run(bd, bm, grid)                                    # a larger call before a smaller one
    s = run(sd, sm, _grid(dsm, 40, 50))
    b = run(bd, bm, grid)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        c = run(bd, bm, grid)
    side.synchronize()
    assert torch.equal(bd, keep_d) and torch.equal(bm, keep_m)
    for k in a:
        assert a[k].is_cuda and b[k].is_cuda and c[k].is_cuda, k
        for other in (b, c):
            x, y = a[k], other[k]
            if x.dtype == torch.float64:
                x, y = x.view(torch.int64), y.view(torch.int64)
            assert x.dtype == y.dtype and torch.equal(x, y), k
    for got, code, mask, res in ((a, big, big_acc >= 2, (300, 340)), (s, small, small_acc >= 2, (40, 50))):
        want = so.network(code, mask)
        host = {k: t.cpu().numpy() for k, t in got.items()}
        expect = {k: want[k] for k in so.KEYS}
        expect["length_m"] = so.length_m(want["steps"], XRES, YRES)
        expect["vertices_en"] = np.stack([500000.0 + want["vertices"][:, 0].astype(np.float64) * XRES, 3400000.0 - want["vertices"][:, 1].astype(np.float64) * YRES], axis=1)
        expect["length"], expect["only_order"] = so.flow_length_doubling(code)[0], want["order_map"]
        assert so.differing(host, expect) == [] and sorted(host) == sorted(expect)


def test_native_argument_rejections(dev):
    from satmvs_amd import _lib
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    gw, gh = 9, 7
    n = gw * gh
    nbytes = lib.smvs_dsm_stream_workspace_bytes(gw, gh)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = {k: torch.zeros(4 * n, dtype=torch.int32, device=dev) for k in ("code", "mask", "order", "link", "counts", "flag", "head", "link_order", "next", "offset", "vertices", "steps", "length")}
    out["mask"].view(torch.uint8)[:n] = 1
    p, null = _lib.ptr, ctypes.c_void_p(0)

    def order(code=p(out["code"]), mask=p(out["mask"]), gw=gw, gh=gh, order=p(out["order"]), link=p(out["link"]), counts=p(out["counts"]), flag=p(out["flag"]),
              ws=p(ws), nbytes=nbytes):
        _lib.call("smvs_dsm_stream_order", code, mask, gw, gh, order, link, counts, flag, ws, nbytes, stream)

    def write(code=p(out["code"]), mask=p(out["mask"]), gw=gw, gh=gh, nl=n, nv=n, head=p(out["head"]), link_order=p(out["link_order"]), nxt=p(out["next"]),
              offset=p(out["offset"]), vertices=p(out["vertices"]), steps=p(out["steps"]), ws=p(ws), nbytes=nbytes):
        _lib.call("smvs_dsm_stream_write", code, mask, gw, gh, nl, nv, head, link_order, nxt, offset, vertices, steps, ws, nbytes, stream)

    def length(code=p(out["code"]), gw=gw, gh=gh, steps=p(out["length"]), flag=p(out["flag"]), ws=p(ws), nbytes=nbytes):
        _lib.call("smvs_dsm_flow_length", code, gw, gh, steps, flag, ws, nbytes, stream)

    bad = [(fn, kw) for fn in (order, write, length) for kw in (dict(gw=0), dict(gh=-1), dict(gw=2 ** 15, gh=2 ** 15), dict(code=null), dict(ws=null),
                                                                dict(nbytes=nbytes - 1), dict(ws=p(out["code"])))]
    bad += [(order, {k: null}) for k in ("mask", "order", "counts", "flag")] + [(write, {k: null}) for k in ("mask", "head", "link_order", "nxt", "offset", "vertices", "steps")]
    bad += [(order, dict(mask=p(out["code"]))), (order, dict(order=p(out["mask"]))), (order, dict(link=p(out["order"]))), (order, dict(counts=p(out["link"]))),
            (order, dict(flag=p(out["counts"]))), (write, dict(nl=-1)), (write, dict(nv=-1)), (write, dict(nl=n + 1)), (write, dict(nv=2 * n + 1)),
            (write, dict(head=p(out["mask"]))), (write, dict(offset=p(out["next"]))), (write, dict(steps=p(out["vertices"]))), (write, dict(vertices=p(out["head"]))),
            (length, dict(steps=null)), (length, dict(flag=null)), (length, dict(steps=p(out["code"]))), (length, dict(flag=p(out["length"])))]
    for fn, kw in bad:
        with pytest.raises(_lib.SatMVSNativeError, match="code 1"):
            fn(**kw)
    torch.cuda.synchronize()
    order()                                                  # and the same arguments unchanged are accepted: 63 roots, 63 links of one vertex
    order(link=null)
    write()
    length()
    torch.cuda.synchronize()
    assert out["counts"][:4].tolist() == [n, n, n, 1] and out["flag"][0].item() == 0 and out["offset"][:n + 1].tolist() == list(range(n + 1))
    assert out["head"][:n].tolist() == list(range(n)) and not out["length"][:3 * n].any() and (out["next"][:n] == -1).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_dtm_to_streams_geojson(dev, tmp_path):
    """extract_dtm -> extract_streams -> write_streams read back: a feature per link of two vertices or more, lines that connect,
    lengths exact in their integers, and the links as labels for label_stats."""
    from satmvs_amd import dsm
    gh, gw = 96, 120
    grid = dsm.DSMGrid(400000.0, 3500000.0, 5.0, 2.5, gw, gh)
    E, N = grid.e0 + 5.0 * np.mgrid[0:gh, 0:gw][1], grid.n0 - 2.5 * np.mgrid[0:gh, 0:gw][0]
    raw = kit_scene(E, N, holes=False, amp=2.0)
    raw[30:50, 40:70] -= np.float32(12.0)
    dtm = dsm.extract_dtm(torch.from_numpy(raw).to(dev), grid)
    links = dsm.extract_streams(dtm, grid, min_area_m2=250.0)                  # 20 cells
    assert all(t.is_cuda for t in links.values())
    code, acc = so.code_of(dtm.cpu().numpy(), 5.0, 2.5)
    mask = acc * 12.5 >= 250.0
    want = so.network(code, mask)
    host = {k: t.cpu().numpy() for k, t in links.items()}
    assert so.differing(host, {k: want[k] for k in so.KEYS}) == [] and len(want["head"]) > 10 and want["counts"][3] >= 2
    path = str(tmp_path / "streams.geojson")
    lines = int((np.diff(want["offset"]) >= 2).sum())
    assert dsm.write_streams(path, links, grid) == lines
    with open(path) as f:
        doc = json.load(f)
    assert doc["type"] == "FeatureCollection" and len(doc["features"]) == lines
    first = host["vertices_en"][want["offset"][:-1]]          # of every link, the one-vertex links without a line included
    cells = 0
    for f in doc["features"]:
        p, xy = f["properties"], np.array(f["geometry"]["coordinates"])
        k = p["link"]
        step = np.abs(np.diff(xy, axis=0)) / np.array([5.0, 2.5])
        assert f["geometry"]["type"] == "LineString" and (step.max(axis=1) == 1.0).all() and set(np.unique(step)) <= {0.0, 1.0}
        assert p["order"] == want["order"][k] and p["next_link"] == want["next_link"][k]
        assert list(xy[0]) == list(first[k])
        if p["next_link"] >= 0:
            assert list(xy[-1]) == list(first[p["next_link"]])
        assert p["length_m"] == float(so.length_m(want["steps"][k], 5.0, 2.5)) == float(host["length_m"][k])
        cells += p["n_cells"]
    assert cells + int((np.diff(want["offset"]) < 2).sum()) == mask.sum() == want["counts"][0]
    # the filled surface as the rule has it, w / 256 (exact in float32): fill_depressions() gives an unraised cell its own bits
    # back, up to 2^-9 m off its w, which is what falls along a flow step
    keys, _ = dsm._flood(dtm.contiguous(), -999.0)
    w = ((keys >> 32) & 0xffffffff) - 2 ** 31
    filled = torch.where(keys == -1, torch.full_like(dtm, -999.0), (w.double() / 256.0).float())
    stats = dsm.label_stats(links["link"], len(want["head"]), values=filled)
    top = filled.reshape(-1)[links["head"].long()]
    assert bool((stats["max"] >= stats["min"]).all()) and torch.equal(stats["max"], top) and torch.equal(stats["area"].long().sum(), torch.tensor(int(mask.sum()), device=dev))
