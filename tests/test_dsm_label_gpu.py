"""Object labelling on the device against the numpy oracle (tests/dsm_label_oracle.py): labels, n and every statistic are
compared for equality, no cell excused.  Random masks on both sides of both percolation thresholds, structured masks with
closed-form answers, one grid wider than 2048 cells and larger than 2048^2 (every level of the scan), the statistics' edge
cases with guard words, determinism, extract_objects on the known-answer scene, the chain on device tensors, void labelling."""
import functools

import numpy as np
import pytest
import torch

import dsm_label_oracle as lo
import dsm_morph_oracle as mo
import dsm_render_oracle as ro
from dsm_testkit import dev, valid  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
ND = np.float32(-999.0)
DENSITIES = (0.3, 0.45, 0.593, 0.8)
SIZES = [(1, 1), (1, 70), (67, 3), (128, 160), (257, 301), (300, 340)]
GH, GW = 257, 301


class Grid:                                                  # what the oracle reads of a DSMGrid
    def __init__(self, gh, gw, e0=500000.0, n0=3400000.0, xres=5.0, yres=2.5):
        self.e0, self.n0, self.xres, self.yres, self.width, self.height = e0, n0, xres, yres, gw, gh


@functools.lru_cache(maxsize=None)
def _values(gh, gw):
    return lo.value_grid(gh, gw, seed=gh + gw)               # shared among the tests: nobody writes to it


def _check(mask, conn, what, expect=None):
    """dsm.label and dsm.label_stats of a mask against the oracle (and a closed form, if given); -> (labels, n)."""
    from satmvs_amd import dsm
    gh, gw = mask.shape
    want, nw = lo.label(mask, conn)
    if expect is not None:
        assert expect[1] == nw and np.array_equal(expect[0], want), (what, "closed form against the oracle")
    got, n = dsm.label(mask, conn)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.shape == mask.shape and isinstance(n, int)
    assert n == nw, (what, n, nw)
    assert np.array_equal(got, want), (what, int((got != want).sum()), np.argwhere(got != want)[:5].tolist())
    z, grid = _values(gh, gw), Grid(gh, gw)
    dgrid = dsm.DSMGrid(grid.e0, grid.n0, grid.xres, grid.yres, gw, gh)
    lo.same_stats(dsm.label_stats(got, n, values=z, grid=dgrid), lo.stats(want, nw, z, ND, grid), what)
    return got, n


# ---- random and structured masks -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", SIZES)
def test_random_masks(dev, shape, conn):
    for density in DENSITIES:
        _check(lo.random_mask(*shape, density, seed=int(1000 * density) + shape[1]), conn, (shape, density, conn))


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", lo.STRUCTURED)
def test_structured_masks(dev, name, conn):
    mask = lo.structured(name, GH, GW)
    labels, n = _check(mask, conn, (name, conn), lo.closed_form(name, GH, GW, conn))
    if name == "spiral":
        assert n == 1 and mask.sum() > GH * GW // 2 - GH - GW                 # one component whose path is half the grid
    if name == "comb":
        assert n == 1 and labels[0, 0] == 1 and labels[0, GW - 1] == 1        # the teeth meet in the last row only
    if name in ("diagonal", "antidiagonal"):
        assert n == (1 if conn == 8 else GH)


def test_large_grid_closed_forms(dev):
    """2300 x 2300: wider than 2048 and more than 2048^2 cells, so all three levels of the scan hold more than one block's
    worth.  Closed-form scenes and statistics only; the comparisons run on the device."""
    from satmvs_amd import dsm
    g = 2300
    r, c = torch.meshgrid(torch.arange(g, device=dev), torch.arange(g, device=dev), indexing="ij")
    z = torch.full((g, g), 2.5, dtype=torch.float32, device=dev)

    def run(mask, conn, want_labels, want_n):
        labels, n = dsm.label(mask, conn)
        assert n == want_n and labels.dtype == torch.int32 and torch.equal(labels, want_labels.to(torch.int32))
        st = dsm.label_stats(labels, n, values=z)
        assert torch.equal(st["n_valid"], st["area"]) and torch.equal(st["qsum"], 2560 * st["area"].long())
        assert bool((st["min"] == 2.5).all()) and bool((st["max"] == 2.5).all()) and bool((st["mean"] == 2.5).all())
        return st

    full = torch.ones((g, g), dtype=torch.uint8, device=dev)
    for conn in (4, 8):
        st = run(full, conn, full, 1)
        assert st["area"].tolist() == [g * g] and st["bbox"].tolist() == [[0, 0, g - 1, g - 1]]
        assert st["rc_sum"].tolist() == [[g * g * (g - 1) // 2] * 2] and st["centroid"].tolist() == [[(g - 1) / 2.0] * 2]
    inside = (r % 4 < 3) & (c % 4 < 3)
    per_row = g // 4
    want = torch.where(inside, (r // 4) * per_row + c // 4 + 1, 0)
    br, bc = torch.meshgrid(torch.arange(per_row, device=dev), torch.arange(per_row, device=dev), indexing="ij")
    br, bc = 4 * br.reshape(-1), 4 * bc.reshape(-1)
    for conn in (4, 8):
        st = run(inside, conn, want, per_row * per_row)
        assert bool((st["area"] == 9).all()) and torch.equal(st["bbox"], torch.stack([br, bc, br + 2, bc + 2], 1).to(torch.int32))
        assert torch.equal(st["rc_sum"], torch.stack([9 * (br + 1), 9 * (bc + 1)], 1))
    board = (r + c) % 2 == 0
    rank = torch.cumsum(board.reshape(-1), 0).reshape(g, g)
    st = run(board, 4, torch.where(board, rank, 0), g * g // 2)
    assert g * g // 2 == 2645000 and bool((st["area"] == 1).all())
    cells = torch.nonzero(board)
    assert torch.equal(st["rc_sum"], cells) and torch.equal(st["bbox"], torch.cat([cells, cells], 1).to(torch.int32))


# ---- statistics: further cases -------------------------------------------------------------------------------------------------
def test_stats_edge_cases(dev):
    from satmvs_amd import dsm
    mask = lo.random_mask(130, 150, 0.45, seed=9)
    labels, n = lo.label(mask, 8)
    z = _values(130, 150).copy()
    for k in (1, 5, n):                                      # components with no valid value
        z[labels == k] = np.where(np.arange((labels == k).sum()) % 2 == 0, np.float32(np.nan), ND)
    want = lo.stats(labels, n, z)
    assert (want["n_valid"] == 0).sum() >= 3 and (want["min"][want["n_valid"] == 0] == ND).all()
    lo.same_stats(dsm.label_stats(labels, n, values=z), want, "no valid value")
    lo.same_stats(dsm.label_stats(labels, n), lo.stats(labels, n), "values=None")
    lo.same_stats(dsm.label_stats(labels, n, values=z, nodata=float("nan")), lo.stats(labels, n, z, np.nan), "nodata=nan")
    seeded = labels.copy()                                   # labels outside 1 .. n count for nothing and write nowhere
    seeded[mask == 0] = np.where(np.arange((mask == 0).sum()) % 3 == 0, -5, np.where(np.arange((mask == 0).sum()) % 3 == 1, n + 1, 0))
    seeded[0, 0], seeded[-1, -1] = -2 ** 31, 2 ** 31 - 1
    lo.same_stats(dsm.label_stats(seeded, n, values=z), lo.stats(seeded, n, z), "seeded")
    lo.same_stats(dsm.label_stats(labels, n - 7, values=z), lo.stats(labels, n - 7, z), "fewer labels than the map holds")
    lo.same_stats(dsm.label_stats(labels, n + 3, values=z), lo.stats(labels, n + 3, z), "more labels than the map holds")
    empty = dsm.label_stats(labels, 0, values=z, grid=dsm.DSMGrid(0.0, 0.0, 5.0, 5.0, 150, 130))
    lo.same_stats(empty, lo.stats(labels, 0, z, ND, Grid(130, 150, 0.0, 0.0, 5.0, 5.0)), "n = 0")
    assert empty["bbox"].shape == (0, 4) and empty["volume"].shape == (0,)
    # non-contiguous and offset inputs
    wide_l = torch.from_numpy(np.concatenate([labels, labels], 1)).to(dev)
    wide_z = torch.from_numpy(np.concatenate([z * 0, z], 1)).to(dev)
    got = dsm.label_stats(wide_l[:, :150], n, values=wide_z[:, 150:])
    assert all(t.is_cuda for t in got.values())
    lo.same_stats({k: t.cpu().numpy() for k, t in got.items()}, want, "views")
    wide_m = np.concatenate([mask * 0, mask, mask * 0], 1)
    for view in (wide_m[:, 150:300], torch.from_numpy(wide_m).to(dev)[:, 150:300], np.asfortranarray(mask), mask.astype(bool),
                 mask.astype(np.int64) * -7, mask.astype(np.uint16) * 256):
        got_l, got_n = dsm.label(view, 8)
        got_l = got_l.cpu().numpy() if isinstance(got_l, torch.Tensor) else got_l
        assert got_n == n and np.array_equal(got_l, labels)


def test_stats_entry_keeps_to_its_outputs(dev):
    """The C entry with guard words before and after every output, seeded outputs (the entry initialises them itself), and
    labels outside 1 .. n on the map."""
    from satmvs_amd import _lib
    gh, gw = 97, 131
    labels, n = lo.label(lo.random_mask(gh, gw, 0.5, seed=4), 4)
    labels[labels == 0] = np.where(np.arange((labels == 0).sum()) % 2 == 0, n + 1, -5)
    z = _values(gh, gw)
    want = lo.stats(labels, n, z)
    G = 64                                                   # guard words on both sides
    spec = {"area": (torch.int32, n), "bbox": (torch.int32, 4 * n), "rc_sum": (torch.int64, 2 * n), "nvalid": (torch.int32, n),
            "vmin": (torch.float32, n), "vmax": (torch.float32, n), "qsum": (torch.int64, n)}
    bufs = {k: torch.full((m + 2 * G,), 77, dtype=dt, device=dev) for k, (dt, m) in spec.items()}
    lab_d, z_d = torch.from_numpy(labels).to(dev), torch.from_numpy(z).to(dev)
    _lib.call("smvs_dsm_label_stats", _lib.ptr(lab_d), _lib.ptr(z_d), gw, gh, -999.0, n,
              *[_lib.ptr(bufs[k][G:]) for k in spec], _lib.current_stream(dev))
    torch.cuda.synchronize()
    for k, (dt, m) in spec.items():
        assert bool((bufs[k][:G] == 77).all()) and bool((bufs[k][G + m:] == 77).all()), k
    inner = {k: bufs[k][G:G + m].cpu().numpy() for k, (dt, m) in spec.items()}
    assert np.array_equal(inner["area"], want["area"]) and np.array_equal(inner["bbox"].reshape(n, 4), want["bbox"])
    assert np.array_equal(inner["rc_sum"].reshape(n, 2), want["rc_sum"]) and np.array_equal(inner["nvalid"], want["n_valid"])
    assert np.array_equal(inner["vmin"].view(np.uint32), want["min"].view(np.uint32))
    assert np.array_equal(inner["vmax"].view(np.uint32), want["max"].view(np.uint32)) and np.array_equal(inner["qsum"], want["qsum"])
    # the labelling entry: guard words around labels and n_out
    mask = torch.from_numpy(lo.random_mask(gh, gw, 0.5, seed=4)).to(dev)
    out = torch.full((gh * gw + 2 * G,), 77, dtype=torch.int32, device=dev)
    n_out = torch.full((1 + 2 * G,), 77, dtype=torch.int32, device=dev)
    nbytes = _lib.load().smvs_dsm_label_workspace_bytes(gw, gh)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.call("smvs_dsm_label", _lib.ptr(mask), gw, gh, 4, _lib.ptr(out[G:]), _lib.ptr(n_out[G:]), _lib.ptr(ws), nbytes, _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert bool((out[:G] == 77).all()) and bool((out[G + gh * gw:] == 77).all())
    assert n_out[G:G + 1].tolist() == [n] and bool((n_out[:G] == 77).all()) and bool((n_out[G + 1:] == 77).all())
    assert np.array_equal(out[G:G + gh * gw].cpu().numpy().reshape(gh, gw), lo.label(mask.cpu().numpy(), 4)[0])


# ---- determinism ---------------------------------------------------------------------------------------------------------------
def test_deterministic(dev):
    from satmvs_amd import dsm
    z = torch.from_numpy(_values(300, 340)).to(dev)
    for mask in (lo.random_mask(300, 340, 0.593, seed=1), np.ones((300, 340), np.uint8)):
        m = torch.from_numpy(mask).to(dev)
        keep = m.clone()
        for conn in (4, 8):
            a, na = dsm.label(m, conn)
            b, nb = dsm.label(m, conn)
            assert a.is_cuda and na == nb and torch.equal(a, b) and torch.equal(m, keep)
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                c, nc = dsm.label(m, conn)
                sc = dsm.label_stats(c, nc, values=z)
            side.synchronize()
            assert nc == na and torch.equal(a, c)
            sa, sb = dsm.label_stats(a, na, values=z), dsm.label_stats(b, nb, values=z, nodata=-999.0)
            for k in sa:
                for other in (sb, sc):
                    x, y = sa[k], other[k]
                    if x.dtype == torch.float32:
                        x, y = x.view(torch.int32), y.view(torch.int32)
                    elif x.dtype == torch.float64:
                        x, y = x.view(torch.int64), y.view(torch.int64)
                    assert torch.equal(x, y), k


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_extract_objects_on_the_known_answer_scene(dev):
    """extract_dtm and ndsm on the device, then extract_objects against the oracle pipeline on the device's own nDSM, and the
    structural facts.  The share of the scene's boxes that come back as exactly one object each is printed, not asserted:
    nobody has measured it."""
    from satmvs_amd import dsm
    z, box = mo.known_answer_scene()
    gh, gw = z.shape
    grid = dsm.DSMGrid(400000.0, 3500000.0, 5.0, 5.0, gw, gh)
    zd = torch.from_numpy(z).to(dev)
    above = dsm.ndsm(zd, dsm.extract_dtm(zd, grid))
    labels, stats = dsm.extract_objects(above, grid)
    assert labels.is_cuda and labels.dtype == torch.int32 and all(t.is_cuda for t in stats.values())
    a = above.cpu().numpy()
    want_labels, want_stats = lo.objects(a, grid)
    got = labels.cpu().numpy()
    assert np.array_equal(got, want_labels)
    lo.same_stats({k: t.cpu().numpy() for k, t in stats.items()}, want_stats, "extract_objects")
    got_np, stats_np = dsm.extract_objects(a, grid)          # numpy in, numpy out
    assert isinstance(got_np, np.ndarray) and np.array_equal(got_np, got)
    lo.same_stats(stats_np, want_stats, "extract_objects, numpy")
    high = valid(a, ND) & (a > np.float32(2.5))
    assert (high[got > 0]).all()                             # every labelled cell stands above min_height
    all_labels, n_all = lo.label(high, 8)
    big = np.concatenate([[False], lo.stats(all_labels, n_all)["area"] >= 2])[all_labels]       # 50 m^2 = 2 cells of 25 m^2
    assert np.array_equal(got > 0, big)                      # and every such cell in an object of the minimum area is labelled
    assert int(stats_np["area"].sum()) == int((got > 0).sum()) and len(stats_np["area"]) == got.max()
    assert (stats_np["min"] > 2.5).all() and (stats_np["volume"] > 0).all()
    box_labels, n_boxes = lo.label(box, 8)                   # the scene's boxes (touching boxes count as one)
    exact = 0
    for k in range(1, n_boxes + 1):
        inside = np.unique(got[(box_labels == k) & high])
        inside = inside[inside > 0]
        exact += len(inside) == 1 and not (got[box_labels != k] == inside[0]).any()
    print("known-answer scene: %d objects; %d of %d box groups recovered as exactly one object each (%.3f)"
          % (got.max(), exact, n_boxes, exact / n_boxes))


def test_production_chain_on_device_tensors(dev, monkeypatch):
    """heights_to_dsm -> despike -> extract_dtm -> ndsm -> extract_objects on device tensors: no grid goes to the host (a
    Tensor.cpu() call fails the test; reading n, one int, is .item())."""
    from satmvs_amd import dsm
    from satmvs_amd.transverse_mercator import whu_tlc_projection
    proj = whu_tlc_projection()
    H, W, res = 128, 160, 2.5
    rpcs = [ro.view_rpc(H, W, s, seed=11) for s in (0.0, 0.4, -0.4)]
    grid = ro.grid_over([(r, (H, W)) for r in rpcs], proj.tm7(), 100.0, 200.0, res, margin=15.0)
    E, N = ro.cell_centres(grid)
    truth = (140.0 + 3.0 * np.sin(E / 53.0) * np.cos(N / 71.0)).astype(np.float32)
    r0, c0 = grid.height // 2 - 8, grid.width // 2 - 8
    truth[r0:r0 + 16, c0:c0 + 16] += 35.0
    hs = [torch.from_numpy(dsm.render_heights(truth, grid, rpc, proj, (H, W))).to(dev) for rpc in rpcs]
    rpcs_d = [torch.from_numpy(np.asarray(r, np.float64)).to(dev) for r in rpcs]

    def no_host_copy(self, *a, **k):
        raise AssertionError("a tensor of shape %s went to the host" % (tuple(self.shape),))
    monkeypatch.setattr(torch.Tensor, "cpu", no_host_copy)
    monkeypatch.setattr(torch.Tensor, "numpy", no_host_copy)
    fused = dsm.heights_to_dsm(hs, rpcs_d, proj, grid, mode="mean")
    clean = dsm.despike(fused, radius=2, thresh=10.0, min_valid=3)
    above = dsm.ndsm(clean, dsm.extract_dtm(clean, grid))
    labels, stats = dsm.extract_objects(above, grid)
    monkeypatch.undo()
    assert labels.is_cuda and above.is_cuda and all(t.is_cuda for t in stats.values())
    want_labels, want_stats = lo.objects(above.cpu().numpy(), grid)
    assert np.array_equal(labels.cpu().numpy(), want_labels)
    lo.same_stats({k: t.cpu().numpy() for k, t in stats.items()}, want_stats, "chain")
    inner = labels[r0 + 3:r0 + 13, c0 + 3:c0 + 13]
    k = int(inner.max())
    assert k > 0 and bool(((inner == k) | (inner == 0)).all())              # the block is one object
    assert stats["area"][k - 1] >= 100 and 25.0 <= float(stats["mean"][k - 1]) <= 45.0


def test_void_labelling(dev):
    from satmvs_amd import dsm
    z = mo.scene(200, 230, seed=70, voids=0.1)
    ok = valid(z, ND)
    for conn in (4, 8):
        got, n = dsm.label(~ok, conn)
        want, nw = lo.label(~ok, conn)
        assert n == nw and n > 100 and np.array_equal(got, want)
    zd = torch.from_numpy(z).to(dev)
    okd = torch.isfinite(zd) & (zd != -999.0)
    got_d, n_d = dsm.label(~okd)
    assert n_d == nw and np.array_equal(got_d.cpu().numpy(), want)
