#!/usr/bin/env python
"""Cost-distance timing on one MI355X ("Cost distance").

Workload: the DTM (dsm.extract_dtm) of the grid of tools/bench_dsm_label.py (bench_dsm_morph's grid, 2199 x 2158 at the default
size).  Sources: one in the centre, one in a corner, 64 scattered (each moved to the nearest passable cell).  Friction: uniform
(none), 1 + slope / 10 degrees, the Tobler table on the DTM, and the slope friction with the footprints of dsm.extract_objects
as barriers.  Per case: the global rounds, smvs_dsm_cost_begin and the rounds to the fixed point with the Python layer's batches
(host clock around a synchronise: the loop reads the device's status once per batch), ms per round, smvs_dsm_cost_read on its
own (device events) and dsm.cost_distance() end to end.  Beside them in the same process, on the back-links of the last case:
dsm.fill_depressions, dsm.basins (the allocation), dsm.flow_length and dsm.least_cost_paths for 1000 targets; the serpentine
corridor of the tests (257 x 301); a torch composite of the synchronous sweep of the key equation (int64 tensors, one source in
the centre, slope friction), its keys asserted equal to the device's; and the oracle's heap on the host over a crop of
--host-side cells a side (Python ints: a statement of the rule, not a competitor), held against the device on that crop.

    python tools/bench_dsm_cost.py [--size 5120] [--reps 10] [--warmup 2] [--no-host] [--json profiles/dsm_cost_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_dsm_morph import NODATA, bench_grid  # noqa: E402
from bench_dsm_outline import host_clock  # noqa: E402
from dsm_bench_common import timed  # noqa: E402
from satmvs_amd import _lib, dsm  # noqa: E402

NO_MAX = 2 ** 64 - 1


def kernel_resources():
    """{kernel: {vgpr, lds, scratch}} of the cd_ kernels, from the code objects inside the built library (tools/kernel_regs.py)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), _lib.LIB_PATH], capture_output=True, text=True).stdout
    table = {}
    for line in out.splitlines()[1:]:
        f = line.split()
        if len(f) >= 8 and f[0].startswith("cd_"):
            table[" ".join(f[:-7])] = {"vgpr": int(f[-7]), "lds": int(f[-4]), "scratch": int(f[-3])}
    return table


def nearest_passable(ok, r, c):
    rr, cc = torch.nonzero(ok, as_tuple=True)
    i = int(torch.argmin((rr - r) ** 2 + (cc - c) ** 2).item())
    return int(rr[i].item()), int(cc[i].item())


def torch_sweeps(src, friction, L, check=64):
    """The synchronous sweep of the key equation as torch operators, table-free: D <- min(D, D(neighbour k) + w_k) over the whole
    grid, until a sweep changes nothing (looked at every `check` sweeps).  -> (D int64 with 2^61 for unreached, sweeps)."""
    big = 1 << 61                                            # twice it still fits an int64
    gh, gw = src.shape
    f = friction.to(torch.int64)                             # an int32 grid: torch has few operators for uint16
    ok = f != 0
    pf = torch.nn.functional.pad(f, (1, 1, 1, 1))
    dc, dr = (1, 1, 0, -1, -1, -1, 0, 1), (0, 1, 1, 1, 0, -1, -1, -1)
    W = []
    for k in range(8):
        fn = pf[1 + dr[k]:1 + dr[k] + gh, 1 + dc[k]:1 + dc[k] + gw]
        w = torch.clamp(((f + fn) * int(L[k]) * 256) >> 10, min=1)
        W.append(torch.where(ok & (fn != 0), w, torch.full_like(w, big)))
    D = torch.where((src != 0) & ok, torch.zeros_like(f), torch.full_like(f, big))
    sweeps = 0
    while True:
        before = D
        for _ in range(check):
            pD = torch.nn.functional.pad(D, (1, 1, 1, 1), value=big)
            new = D
            for k in range(8):
                new = torch.minimum(new, torch.clamp(pD[1 + dr[k]:1 + dr[k] + gh, 1 + dc[k]:1 + dc[k] + gw] + W[k], max=big))
            D = new
        sweeps += check
        if torch.equal(D, before):
            return D, sweeps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=5120)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--res", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--speckle", type=float, default=0.01)
    ap.add_argument("--drop", type=float, default=0.05)
    ap.add_argument("--host-side", type=int, default=768, help="side of the crop the heap oracle runs on")
    ap.add_argument("--no-host", action="store_true", help="leave the heap oracle out")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dsm_cost needs an MI355X")
    dev = torch.device("cuda:0")
    z, grid = bench_grid(a, dev)
    gh, gw = z.shape
    n = gh * gw
    dtm = dsm.extract_dtm(z, grid, NODATA).contiguous()
    labels, _ = dsm.extract_objects(dsm.ndsm(z, dtm, NODATA), grid, nodata=NODATA)
    # friction grids are made on the host (torch has few operators for uint16); `wide` keeps an int32 copy of each for the masks
    slope_host = dsm.quantise_friction(1.0 + dsm.slope(dtm, grid, NODATA).cpu().numpy().astype(np.float64) / 10.0, NODATA)
    buildings_host = np.where(labels.cpu().numpy() > 0, 0, slope_host).astype(np.uint16)
    by_slope, with_buildings = torch.from_numpy(slope_host).to(dev), torch.from_numpy(buildings_host).to(dev)
    wide = {id(t): torch.from_numpy(h.astype(np.int32)).to(dev) for t, h in ((by_slope, slope_host), (with_buildings, buildings_host))}
    table = dsm.tobler_table()
    L = dsm.cost_terms(grid)
    frictions = {"uniform": (None, None, None), "slope": (by_slope, None, None), "tobler": (None, dtm, table), "buildings": (with_buildings, None, None)}
    rng = np.random.default_rng(0)
    scattered = np.stack([rng.integers(0, gh, 64), rng.integers(0, gw, 64)], axis=1)
    spots = {"centre": [(gh // 2, gw // 2)], "corner": [(0, 0)], "scattered 64": [tuple(int(v) for v in rc) for rc in scattered]}
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    p = _lib.ptr
    q = lambda t: None if t is None else p(t)                # noqa: E731
    host = lambda t: None if t is None else t.ctypes.data_as(_lib.C.c_void_p)      # noqa: E731
    nbytes = lib.smvs_dsm_cost_workspace_bytes(gw, gh)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    keys = torch.empty((gh, gw), dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    raw = torch.empty((gh, gw), dtype=torch.int64, device=dev)
    cost = torch.empty((gh, gw), dtype=torch.float64, device=dev)
    link = torch.empty((gh, gw), dtype=torch.uint8, device=dev)
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "the DTM of bench_dsm_label's grid (%dx%d, %.1f m cells)" % (gw, gh, a.res), "cells": n, "tiles": ((gw + 31) // 32) * ((gh + 31) // 32),
           "kernel_resources": kernel_resources(), "cost_workspace_bytes": nbytes, "barrier_cells_with_buildings": int((buildings_host == 0).sum()),
           "cases": [], "kernel_traces": "not measured", "real_dtms": "not measured"}
    for fname, (f, zz, tab) in frictions.items():
        ok = (wide[id(f)] != 0) if f is not None else torch.ones((gh, gw), dtype=torch.bool, device=dev)
        if zz is not None:
            ok = ok & torch.isfinite(zz) & (zz != NODATA)
        for sname, cells in spots.items():
            cells = sorted(set(nearest_passable(ok, r, c) for r, c in cells))
            src = torch.zeros((gh, gw), dtype=torch.uint8, device=dev)
            for r, c in cells:
                src[r, c] = 1

            def relax():
                _lib.call("smvs_dsm_cost_begin", q(f), p(src), q(zz), gw, gh, NODATA, p(keys), p(count), p(ws), nbytes, stream)
                return dsm._cost_relax(dev, f, zz, gw, gh, NODATA, L, tab, 0, keys, ws, nbytes)

            relax_ms, rounds = host_clock(relax, 3)
            read_ms = timed(lambda: _lib.call("smvs_dsm_cost_read", q(f), q(zz), gw, gh, NODATA, host(L), host(tab), 0, p(keys), NO_MAX, p(raw), p(cost), p(link),
                                              p(ws), nbytes, stream), a.reps, a.warmup)
            api_ms, _ = host_clock(lambda: dsm.cost_distance(src, grid, f, zz, tab), 3)
            res["cases"].append({"friction": fname, "sources": sname, "n_sources": len(cells), "rounds": rounds, "begin_and_rounds_ms": relax_ms,
                                 "ms_per_round": relax_ms["median"] / rounds, "read_ms": read_ms, "cost_distance_api_ms": api_ms,
                                 "reached_cells": int((raw >= 0).sum().item()), "highest_cost": float(torch.where(raw >= 0, cost, torch.zeros_like(cost)).max().item())})
    # the forest tools on the last case's back-links (buildings as barriers, 64 sources), and the flood for scale
    res["fill_depressions_api_ms"], _ = host_clock(lambda: dsm.fill_depressions(dtm, NODATA), 3)
    res["basins_api_ms"], (_, n_served) = host_clock(lambda: dsm.basins(link), 3)
    res["flow_length_api_ms"], _ = host_clock(lambda: dsm.flow_length(link, grid), 3)
    reached = torch.nonzero(raw > 0)
    targets = reached[torch.from_numpy(rng.choice(len(reached), 1000, replace=False)).to(dev)]
    res["least_cost_paths_1000_api_ms"], paths = host_clock(lambda: dsm.least_cost_paths(link, targets, grid, raw), 3)
    res["allocation_sources"] = int(n_served)
    res["paths_links"], res["paths_vertices"] = int(paths["head"].numel()), int(paths["vertices"].shape[0])
    res["paths_network_length_km"] = float(paths["length_m"].sum().item()) / 1e3
    # the serpentine of the tests
    import dsm_cost_oracle as co
    sf, ssrc, spath = co.serpentine(257, 301)
    sgrid = dsm.DSMGrid(0.0, 0.0, 5.0, 2.5, 301, 257)
    s_ms, s_out = host_clock(lambda: dsm.cost_distance(ssrc, sgrid, sf, return_rounds=True), 3)
    res["serpentine_257x301"] = {"corridor_cells": len(spath), "rounds": s_out[2], "cost_distance_api_ms": s_ms}
    # the synchronous sweep as torch operators: one source in the centre, slope friction
    centre = nearest_passable(wide[id(by_slope)] != 0, gh // 2, gw // 2)
    src = torch.zeros((gh, gw), dtype=torch.uint8, device=dev)
    src[centre] = 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    D, sweeps = torch_sweeps(src, wide[id(by_slope)], L)
    torch.cuda.synchronize()
    sweep_ms = 1e3 * (time.perf_counter() - t0)
    native_ms, got = host_clock(lambda: dsm.cost_distance(src, grid, by_slope, return_raw=True, return_rounds=True), 3)
    equal = bool(torch.equal(torch.where(D >= (1 << 61), torch.full_like(D, -1), D), got[2]))
    assert equal, "the torch sweeps and the device disagree"
    res["torch_sweeps"] = {"ms": sweep_ms, "sweeps": sweeps, "native_api_ms": native_ms, "native_rounds": got[3], "equal_keys": equal}
    if a.no_host:
        res["heap_oracle_host"] = "not measured"
    else:
        side = min(a.host_side, gh, gw)
        crop = np.ascontiguousarray(buildings_host[:side, :side])
        csrc = np.zeros((side, side), np.uint8)
        csrc[nearest_passable(torch.from_numpy(crop != 0), side // 2, side // 2)] = 1
        t0 = time.perf_counter()
        want = co.keys_heap(csrc, L.tolist(), crop)
        host_ms = 1e3 * (time.perf_counter() - t0)
        cgrid = dsm.DSMGrid(grid.e0, grid.n0, grid.xres, grid.yres, side, side)
        crop_ms, got = host_clock(lambda: dsm.cost_distance(csrc, cgrid, crop, return_raw=True), 3)
        res["heap_oracle_host"] = {"ms": host_ms, "cells": side * side, "native_api_ms": crop_ms, "equal": bool(np.array_equal(co.read(want)[0], got[2]))}
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
