#!/usr/bin/env python
"""Outline timing on one MI355X ("Outlines").

Workload: the grid of tools/bench_dsm_label.py (bench_dsm_morph's grid, extract_dtm, ndsm).  Two label maps on it, both under
connectivity 8: the nDSM mask (valid and above 2.5 m) and the grid's void mask.  Device events time --reps calls after
--warmup, workspace and outputs allocated outside the timed span: smvs_dsm_label and smvs_dsm_label_stats as the yardstick,
then the three native steps of dsm.outlines (the edge count, the full count with its doubling, the write) and smvs_dsm_burn of
the result; dsm.outlines and dsm.burn_rings end to end on device tensors (host clock around a synchronise: allocation and the
two reads of the counts included).  The doubling is not timed by itself: (full count - edge count) / rounds bounds a round from
above.  What a user has without the native entries is the label map copied to the host and traced in Python: the numpy
oracle's walk (tests/dsm_outline_oracle.py), one run, host clock; with --oracle its rings are compared with the device's.

    python tools/bench_dsm_outline.py [--size 5120] [--reps 20] [--warmup 3] [--oracle] [--no-host] [--json profiles/dsm_outline_bench.json]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_dsm_morph import NODATA, bench_grid  # noqa: E402
from dsm_bench_common import scratch_sizes, stats, timed  # noqa: E402
from satmvs_amd import _lib, dsm  # noqa: E402

MIN_HEIGHT = 2.5


def host_clock(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return stats(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=5120)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--res", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--speckle", type=float, default=0.01)
    ap.add_argument("--drop", type=float, default=0.05)
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--no-host", action="store_true", help="leave the Python walk on the host out")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dsm_outline needs an MI355X")
    dev = torch.device("cuda:0")
    z, grid = bench_grid(a, dev)
    gh, gw = z.shape
    above = dsm.ndsm(z, dsm.extract_dtm(z, grid, NODATA), NODATA)
    ok = torch.isfinite(above) & (above != NODATA)
    values = torch.where(ok, above, torch.zeros_like(above)).contiguous()
    masks = [("ndsm", 8, ok & (above > MIN_HEIGHT)), ("voids", 8, ~(torch.isfinite(z) & (z != NODATA)))]
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    p = _lib.ptr
    label_bytes = lib.smvs_dsm_label_workspace_bytes(gw, gh)
    label_ws = torch.empty(label_bytes, dtype=torch.uint8, device=dev)
    labels = torch.empty((gh, gw), dtype=torch.int32, device=dev)
    n_dev = torch.empty(1, dtype=torch.int32, device=dev)
    counts = torch.empty(3, dtype=torch.int32, device=dev)
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "bench_dsm_label's grid (%dx%d, %.1f m cells): nDSM mask above %.1f m and void mask, connectivity 8" % (gw, gh, a.res, MIN_HEIGHT),
           "cells": gw * gh, "scratch_bytes": scratch_sizes(r"ol_"), "masks": [],
           "kernel_traces": "not measured", "counters": "not measured", "real_dsms": "not measured"}
    for name, conn, mask in masks:
        m8 = mask.to(torch.uint8).contiguous()
        label_ms = timed(lambda: _lib.call("smvs_dsm_label", p(m8), gw, gh, conn, p(labels), p(n_dev), p(label_ws), label_bytes, stream), a.reps, a.warmup)
        n = int(n_dev.item())
        out = [torch.empty(n * k, dtype=dt, device=dev) for dt, k in ((torch.int32, 1), (torch.int32, 4), (torch.int64, 2), (torch.int32, 1),
                                                                        (torch.float32, 1), (torch.float32, 1), (torch.int64, 1))]
        stats_ms = timed(lambda: _lib.call("smvs_dsm_label_stats", p(labels), p(values), gw, gh, NODATA, n, *[p(t) for t in out], stream), a.reps, a.warmup)
        del out
        bytes0 = lib.smvs_dsm_outline_workspace_bytes(gw, gh, 0)
        ws0 = torch.empty(bytes0, dtype=torch.uint8, device=dev)
        census_ms = timed(lambda: _lib.call("smvs_dsm_outline_count", p(labels), gw, gh, n, 0, p(counts), p(ws0), bytes0, stream), a.reps, a.warmup)
        ne = int(counts[0].item())
        nbytes = lib.smvs_dsm_outline_workspace_bytes(gw, gh, ne)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        count_ms = timed(lambda: _lib.call("smvs_dsm_outline_count", p(labels), gw, gh, n, ne, p(counts), p(ws), nbytes, stream), a.reps, a.warmup)
        ne, nr, nv = counts.tolist()
        ring = {"label": torch.empty(nr, dtype=torch.int32, device=dev), "area2": torch.empty(nr, dtype=torch.int64, device=dev),
                "edges": torch.empty((nr, 2), dtype=torch.int32, device=dev), "offset": torch.empty(nr + 1, dtype=torch.int32, device=dev),
                "first_ring": torch.empty(n + 1, dtype=torch.int32, device=dev), "vertices": torch.empty((nv, 2), dtype=torch.int32, device=dev)}
        write_ms = timed(lambda: _lib.call("smvs_dsm_outline_write", p(labels), gw, gh, n, ne, nr, nv, *[p(ring[k]) for k in ring], p(ws), nbytes, stream),
                         a.reps, a.warmup)
        burnt = torch.empty_like(labels)
        burn_ms = timed(lambda: _lib.call("smvs_dsm_burn", p(ring["vertices"]), p(ring["offset"]), p(ring["label"]), nr, nv, gw, gh, p(burnt), p(n_dev), stream),
                        a.reps, a.warmup)
        rounds = max(0, (ne - 1).bit_length())
        api_ms, got = host_clock(lambda: dsm.outlines(labels, n), 5)
        burn_api_ms, back = host_clock(lambda: dsm.burn_rings(got["vertices"], got["offset"], got["label"], (gh, gw)), 5)
        native = census_ms["median"] + count_ms["median"] + write_ms["median"]
        yardstick = label_ms["median"] + stats_ms["median"]
        row = {"mask": name, "connectivity": conn, "foreground": int(m8.sum()), "n": n, "n_edges": ne, "n_rings": nr, "n_vertices": nv,
               "workspace_bytes": nbytes, "label_ms": label_ms, "stats_ms": stats_ms, "edge_count_ms": census_ms, "count_ms": count_ms, "write_ms": write_ms,
               "burn_ms": burn_ms, "doubling_rounds": rounds, "doubling_round_ms_at_most": (count_ms["median"] - census_ms["median"]) / max(rounds, 1),
               "outlines_native_ms": native, "label_plus_stats_ms": yardstick, "outlines_over_label_plus_stats": native / yardstick,
               "outlines_api_ms": api_ms, "burn_rings_api_ms": burn_api_ms,
               "round_trip_equal": bool(torch.equal(back, labels)) and bool(torch.equal(burnt, labels)),
               "api_equals_native": all(bool(torch.equal(got[k], ring[k])) for k in ring)}
        if a.no_host:
            row["host_walk_ms"] = row["equal"] = "not measured"
        else:
            import dsm_outline_oracle as oo
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            want = oo.trace(labels.cpu().numpy(), n)
            row["host_walk_ms"] = 1e3 * (time.perf_counter() - t0)
            row["host_walk_over_outlines_api"] = row["host_walk_ms"] / api_ms["median"]
            row["equal"] = oo.difference({k: t.cpu().numpy() for k, t in got.items()}, want) is None if a.oracle else "not measured"
        res["masks"].append(row)
        del ws, ws0, ring, burnt, got, back
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
