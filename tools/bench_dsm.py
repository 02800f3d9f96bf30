#!/usr/bin/env python
"""DSM production timing on one MI355X.

Workload: three 5120 x 5120 height maps with synthetic TLC-shaped RPCs (rpc_synth.make_view_rpcs, GSD 2.1 m, near the WHU-TLC
central meridian) fused into a 5 m WHU-TLC UTM grid, median mode.  Reports the bin pass (three calls), the reduce pass and the
total (count zero-fill + bins + reduce) over --reps timed repetitions after warm-up, device events: min / median / max in ms.
With --oracle, times the numpy route once on ONE map (inverse RPC + TM + cell + lexsort median, float64, chunked) for a speedup
figure.  Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script (--reps 3, no oracle).

    python tools/bench_dsm.py [--size 5120] [--reps 20] [--warmup 3] [--oracle] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dsm_bench_common import stats, synth_heights  # noqa: E402
from satmvs_amd import dsm, rpc_synth  # noqa: E402
from satmvs_amd.transverse_mercator import whu_tlc_projection  # noqa: E402


def numpy_oracle_one_map(h, rpc, tm7, grid, chunk=1 << 20):
    """The numpy route for one map: float64 inverse RPC + TM forward + cell rule, then a lexsort median per cell."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import dsm_oracle as orc
    H, W = h.shape
    hf = h.reshape(-1)
    cells = np.empty(hf.size, np.int64)
    for s in range(0, hf.size, chunk):
        i = np.arange(s, min(s + chunk, hf.size))
        x, y = (i % W).astype(np.float64), (i // W).astype(np.float64)
        lat, lon = rpc_synth.photo2obj(rpc, x, y, hf[i].astype(np.float64))
        E, N = orc.tm_forward(tm7, lat, lon)
        c = orc.cells(E, N, grid.grid4(), grid.width, grid.height)
        c[~np.isfinite(hf[i])] = -1
        cells[s:s + len(i)] = c
    ok = cells >= 0
    c, v = cells[ok], hf[ok]
    order = np.lexsort((orc.keys(v), c))
    c, v = c[order], v[order]
    cnt = np.bincount(c, minlength=grid.width * grid.height)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    nz = cnt > 0
    out = np.full(cnt.size, np.float32(-999.0), np.float32)
    lo = start[nz] + (cnt[nz] - 1) // 2
    hi = start[nz] + cnt[nz] // 2
    out[nz] = np.where(cnt[nz] % 2 == 1, v[hi], (0.5 * (v[lo].astype(np.float64) + v[hi].astype(np.float64))).astype(np.float32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=5120)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--res", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", default="median")
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dsm needs an MI355X")
    dev = torch.device("cuda:0")
    proj = whu_tlc_projection()
    t0 = time.perf_counter()
    rpcs_np = rpc_synth.make_view_rpcs(a.views, a.size, a.size, seed=0, gsd=2.1, lat0=31.0, lon0=-134.6)
    t_rpc = time.perf_counter() - t0
    rpcs = [torch.from_numpy(r).to(dev) for r in rpcs_np]
    hs = synth_heights(a.views, a.size, dev)
    grid = dsm.grid_for(hs, rpcs, proj, a.res)
    n = sum(h.numel() for h in hs)
    tm7, grid4 = proj.tm7(), grid.grid4()
    cell = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.zeros(grid.width * grid.height, dtype=torch.int32, device=dev)
    flat = torch.cat([h.reshape(-1) for h in hs])

    def run(ev=None):
        count.zero_()
        at = 0
        for h, r in zip(hs, rpcs):
            dsm._bin(h, r, None, tm7, grid4, grid.width, grid.height, cell[at:at + h.numel()], count)
            at += h.numel()
        if ev:
            ev.record()
        return dsm.reduce_cells(cell, flat, count, grid, a.mode)

    for _ in range(a.warmup):
        out = run()
    torch.cuda.synchronize()
    t_bin, t_red, t_tot = [], [], []
    for _ in range(a.reps):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        out = run(e1)
        e2.record()
        torch.cuda.synchronize()
        t_bin.append(e0.elapsed_time(e1))
        t_red.append(e1.elapsed_time(e2))
        t_tot.append(e0.elapsed_time(e2))
    res = {"workload": "%d x %dx%d height maps, GSD 2.1 m, %.1f m grid %dx%d, mode %s" % (a.views, a.size, a.size, a.res, grid.width,
                                                                                          grid.height, a.mode),
           "points": n, "cells": grid.width * grid.height, "on_grid_points": int(count.sum()),
           "occupied_cells": int((count > 0).sum()), "max_points_per_cell": int(count.max()),
           "bin_ms": stats(t_bin), "reduce_ms": stats(t_red), "total_ms": stats(t_tot),
           "rpc_fit_s_host": t_rpc, "dsm_checksum": float(out[out != -999.0].double().sum())}
    if a.oracle:
        h0, r0 = hs[0].cpu().numpy(), rpcs_np[0]
        t0 = time.perf_counter()
        want = numpy_oracle_one_map(h0, r0, tm7, grid)
        t_np = time.perf_counter() - t0
        # the same map on the GPU, bin + reduce, for the like-for-like figure and an agreement count
        c1 = torch.zeros_like(count)
        cell1 = torch.empty(hs[0].numel(), dtype=torch.int32, device=dev)
        ts = []
        for k in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c1.zero_()
            dsm._bin(hs[0], rpcs[0], None, tm7, grid4, grid.width, grid.height, cell1, c1)
            got = dsm.reduce_cells(cell1, hs[0].reshape(-1), c1, grid, "median")
            e1.record()
            torch.cuda.synchronize()
            if k >= a.warmup:
                ts.append(e0.elapsed_time(e1))
        got = got.cpu().numpy().reshape(-1)
        res["numpy_one_map_s"] = t_np
        res["gpu_one_map_ms"] = stats(ts)
        res["speedup_one_map"] = t_np * 1e3 / stats(ts)["median"]
        res["one_map_cells_differing_from_numpy"] = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
