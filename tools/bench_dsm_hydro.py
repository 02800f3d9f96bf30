#!/usr/bin/env python
"""Hydrology timing on one MI355X ("Hydrology").

Workload: the grid of tools/bench_dsm_label.py (bench_dsm_morph's grid, 2199 x 2158 at the default size): its DTM
(dsm.extract_dtm) and the DSM itself, which has more pits and voids.  Per surface: the global rounds of the flood to convergence
and its time under three batch policies (host clock around a synchronise: every batch ends in one read of the device's status);
the rounds alone in calls of up to 4096 without a read between them (device events); smvs_dsm_flood_read, smvs_dsm_flow_dir,
smvs_dsm_flow_accumulate and smvs_dsm_flow_basins on their own (device events, --reps calls after --warmup, workspace and outputs
allocated outside the timed span); the share of raised cells and the longest flat.  Beside them in the same process:
dsm.extract_dtm and dsm.label + dsm.label_stats on the nDSM mask, the steps the tool chain had before; the oracle's heap flood on
the host over a crop of --host-side cells a side (pure Python: a statement of the rule, not a competitor); and a torch composite of
the synchronous sweep (shifted minima of int64 keys, convergence read every 16 sweeps), stopped after --max-sweeps.
The tile of the flood is a compile-time constant (32 x 32): its sensitivity is not measured here.

    python tools/bench_dsm_hydro.py [--size 5120] [--reps 10] [--warmup 2] [--no-host] [--json profiles/dsm_hydro_bench.json]
"""
import argparse
import ctypes
import json
import os
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
from dsm_bench_common import scratch_sizes, timed  # noqa: E402
from satmvs_amd import _lib, dsm  # noqa: E402

MIN_HEIGHT = 2.5
DC = (1, 1, 0, -1, -1, -1, 0, 1)
DR = (0, 1, 1, 1, 0, -1, -1, -1)


def torch_sweeps(z, max_sweeps):
    """The synchronous relaxation as torch operators: -> (keys int64 w 2^32 + d with 2^62 where invalid, sweeps, converged)."""
    gh, gw = z.shape
    valid = torch.isfinite(z) & (z != NODATA) & (z.abs() <= 32768.0)
    q = torch.round(torch.where(valid, z, torch.zeros_like(z)).double() * 256.0).long()
    inf = 2 ** 62
    pad = torch.zeros((gh + 2, gw + 2), dtype=torch.bool, device=z.device)
    pad[1:-1, 1:-1] = valid
    ring = torch.ones_like(valid)
    for k in range(8):
        ring &= pad[1 + DR[k]:1 + DR[k] + gh, 1 + DC[k]:1 + DC[k] + gw]
    floor = q << 32
    open_ = valid & ring
    key = torch.where(valid & ~ring, floor, torch.full_like(floor, inf))
    big = torch.full((gh + 2, gw + 2), inf, dtype=torch.int64, device=z.device)
    sweeps = 0
    while sweeps < max_sweeps:
        before = key
        for _ in range(16):
            big[1:-1, 1:-1] = key
            low = big[1 + DR[0]:1 + DR[0] + gh, 1 + DC[0]:1 + DC[0] + gw]
            for k in range(1, 8):
                low = torch.minimum(low, big[1 + DR[k]:1 + DR[k] + gh, 1 + DC[k]:1 + DC[k] + gw])
            key = torch.where(open_, torch.minimum(key, torch.maximum(floor, low + 1)), key)
        sweeps += 16
        if torch.equal(before, key):
            return key, sweeps, True
    return key, sweeps, False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=5120)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--res", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--speckle", type=float, default=0.01)
    ap.add_argument("--drop", type=float, default=0.05)
    ap.add_argument("--host-side", type=int, default=768, help="side of the crop the Python heap flood runs on")
    ap.add_argument("--max-sweeps", type=int, default=4096)
    ap.add_argument("--no-host", action="store_true", help="leave the Python heap flood out")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dsm_hydro needs an MI355X")
    dev = torch.device("cuda:0")
    z, grid = bench_grid(a, dev)
    gh, gw = z.shape
    n = gh * gw
    dtm_ms, dtm = host_clock(lambda: dsm.extract_dtm(z, grid, NODATA), 3)
    above = dsm.ndsm(z, dtm, NODATA)
    mask = torch.isfinite(above) & (above != NODATA) & (above > MIN_HEIGHT)

    def label_and_stats():
        labels, m = dsm.label(mask, 8)
        return dsm.label_stats(labels, m, values=above, grid=grid, nodata=NODATA), m

    label_ms, (_, n_objects) = host_clock(label_and_stats, 3)
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    p = _lib.ptr
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "bench_dsm_label's grid (%dx%d, %.1f m cells): the DTM and the DSM" % (gw, gh, a.res),
           "cells": n, "scratch_bytes": scratch_sizes(r"hy_|fl_"), "extract_dtm_api_ms": dtm_ms,
           "label_and_stats_api_ms": label_ms, "n_objects": int(n_objects), "surfaces": [],
           "tile_shape_sensitivity": "not measured: the tile is a compile-time constant", "kernel_traces": "not measured", "real_dtms": "not measured"}
    flood_bytes, flow_bytes = lib.smvs_dsm_flood_workspace_bytes(gw, gh), lib.smvs_dsm_flow_workspace_bytes(gw, gh)
    ws1 = torch.empty(flood_bytes, dtype=torch.uint8, device=dev)
    ws2 = torch.empty(flow_bytes, dtype=torch.uint8, device=dev)
    dist = dsm.flow_distances(grid)
    dp = dist.ctypes.data_as(ctypes.c_void_p)
    for name, surface in (("dtm", dtm), ("dsm", z)):
        surface = surface.contiguous()
        row = {"surface": name, "flow_workspace_bytes": flow_bytes}
        for policy, batch in (("8_then_doubling", None), ("8", 8), ("64", 64)):
            ms, (keys, rounds) = host_clock(lambda: dsm._flood(surface, NODATA, batch), 3)
            row["flood_api_ms_batch_" + policy] = ms
            row["flood_rounds_run_batch_" + policy] = rounds
        status = torch.empty(1, dtype=torch.int32, device=dev)
        # the least number of rounds: single rounds until the status clears (untimed), then that many rounds without a read between
        _lib.call("smvs_dsm_flood_begin", p(surface), gw, gh, NODATA, p(keys), p(ws1), flood_bytes, stream)
        need = 0
        while True:
            _lib.call("smvs_dsm_flood_rounds", p(surface), gw, gh, NODATA, p(keys), 1, p(status), p(ws1), flood_bytes, stream)
            need += 1
            if int(status.item()) == 0 or need > n + 2:
                break
        row["flood_rounds_to_convergence"] = need

        def rounds_only():
            _lib.call("smvs_dsm_flood_begin", p(surface), gw, gh, NODATA, p(keys), p(ws1), flood_bytes, stream)
            left = need
            while left > 0:
                k = min(left, 4096)
                _lib.call("smvs_dsm_flood_rounds", p(surface), gw, gh, NODATA, p(keys), k, p(status), p(ws1), flood_bytes, stream)
                left -= k

        row["flood_begin_and_rounds_ms"] = timed(rounds_only, a.reps, a.warmup)
        row["flood_round_ms_mean"] = row["flood_begin_and_rounds_ms"]["median"] / need
        filled, depth = torch.empty_like(surface), torch.empty_like(surface)
        flat = torch.empty((gh, gw), dtype=torch.int32, device=dev)
        row["flood_read_ms"] = timed(lambda: _lib.call("smvs_dsm_flood_read", p(surface), gw, gh, NODATA, p(keys), p(filled), p(depth), p(flat), stream), a.reps, a.warmup)
        code = torch.empty((gh, gw), dtype=torch.uint8, device=dev)
        row["flow_dir_ms"] = timed(lambda: _lib.call("smvs_dsm_flow_dir", p(keys), gw, gh, dp, p(code), stream), a.reps, a.warmup)
        acc = torch.empty((gh, gw), dtype=torch.int64, device=dev)
        word = torch.empty(2, dtype=torch.int32, device=dev)
        row["flow_accumulate_ms"] = timed(lambda: _lib.call("smvs_dsm_flow_accumulate", p(code), None, gw, gh, p(acc), p(word[1:]), p(ws2), flow_bytes, stream), a.reps, a.warmup)
        basin = torch.empty((gh, gw), dtype=torch.int32, device=dev)
        row["flow_basins_ms"] = timed(lambda: _lib.call("smvs_dsm_flow_basins", p(code), None, gw, gh, p(basin), p(word[:1]), p(word[1:]), p(ws2), flow_bytes, stream), a.reps, a.warmup)
        valid = code != 255
        row.update({"valid_cells": int(valid.sum().item()), "outlets": int((code == 0).sum().item()), "raised_cells": int(((depth > 0) & valid).sum().item()),
                    "deepest_m": float(torch.where(valid, depth, torch.zeros_like(depth)).max().item()), "longest_flat_steps": int(flat.max().item()),
                    "largest_accumulation_cells": int(acc.max().item()), "basins": int(word[0].item()), "cyclic_flag": int(word[1].item()),
                    "roots_sum_to_valid_cells": int(acc[code == 0].sum().item()) == int(valid.sum().item()),
                    "tour_elements": 2 * n, "tour_doubling_rounds": (2 * n - 1).bit_length(), "root_doubling_rounds": (n - 1).bit_length() + 1})
        t0 = time.perf_counter()
        tk, sweeps, done = torch_sweeps(surface, a.max_sweeps)
        torch.cuda.synchronize()
        row["torch_sweeps"] = {"ms": 1e3 * (time.perf_counter() - t0), "sweeps": sweeps, "converged": done}
        if done:
            upper = (keys >> 32) & 0xffffffff                # the uint64 word read as int64: w + 2^31 sits in the upper half
            mine = torch.where(valid, ((upper - 2 ** 31) << 32) | (keys & 0xffffffff), torch.full_like(keys, 2 ** 62))
            row["torch_sweeps"]["equal_keys"] = bool(torch.equal(mine, tk))
        del tk
        if a.no_host:
            row["python_heap_flood_host"] = "not measured"
        else:
            import dsm_hydro_oracle as ho
            side = min(a.host_side, gh, gw)
            crop = surface[:side, :side].contiguous()
            t0 = time.perf_counter()
            w_host, d_host, v_host = ho.keys_heap(crop.cpu().numpy(), NODATA)
            host_ms = 1e3 * (time.perf_counter() - t0)
            crop_keys, _ = dsm._flood(crop, NODATA)
            row["python_heap_flood_host"] = {"ms": host_ms, "cells": side * side,
                                             "equal_keys": bool(np.array_equal(ho.pack(w_host, d_host, v_host), crop_keys.cpu().numpy().view(np.uint64)))}
        res["surfaces"].append(row)
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
