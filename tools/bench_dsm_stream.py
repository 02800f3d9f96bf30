#!/usr/bin/env python
"""Stream-network timing on one MI355X ("Stream network").

Workload: the DTM (dsm.extract_dtm) of the grid of tools/bench_dsm_label.py (bench_dsm_morph's grid, 2199 x 2158 at the default
size), its D8 directions and accumulation, and the stream masks acc >= 1, >= 100 and >= 1000 cells.  Per threshold:
smvs_dsm_stream_order and smvs_dsm_stream_write on their own (device events, --reps calls after --warmup, workspace and outputs
allocated outside the timed span) and dsm.stream_links() end to end (host clock around a synchronise: it allocates, reads the
counts once and runs both passes); the stream cells, links, vertices, highest order and the order rounds that did work (the
highest order: the last of them finds no junction and the rounds after it leave at once).  smvs_dsm_flow_length on the same
directions.  Beside them in the same process: smvs_dsm_flow_accumulate, dsm.extract_dtm and dsm.label + dsm.label_stats on
the nDSM mask, for scale; and the oracle's array statement on the host over a crop of --host-side cells a side (numpy: a
statement of the rule, not a competitor), held against the device on that crop.

    python tools/bench_dsm_stream.py [--size 5120] [--reps 10] [--warmup 2] [--no-host] [--json profiles/dsm_stream_bench.json]
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

MIN_HEIGHT = 2.5
THRESHOLDS = (1, 100, 1000)


def kernel_resources():
    """{kernel: {vgpr, scratch}} of the st_ kernels and the d8_ ones of csrc/dsm_flow.h, from the code objects inside the built
    library (tools/kernel_regs.py; dsm_bench_common.scratch_sizes looks at the kernels named dsm_ only)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), _lib.LIB_PATH], capture_output=True, text=True).stdout
    table = {}
    for line in out.splitlines()[1:]:
        f = line.split()
        if len(f) >= 8 and f[0].startswith(("st_", "d8_")):
            table[f[0]] = {"vgpr": int(f[1]), "scratch": int(f[-3])}
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=5120)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--res", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--speckle", type=float, default=0.01)
    ap.add_argument("--drop", type=float, default=0.05)
    ap.add_argument("--host-side", type=int, default=512, help="side of the crop the numpy oracle runs on")
    ap.add_argument("--no-host", action="store_true", help="leave the numpy oracle out")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dsm_stream needs an MI355X")
    dev = torch.device("cuda:0")
    z, grid = bench_grid(a, dev)
    gh, gw = z.shape
    n = gh * gw
    dtm_ms, dtm = host_clock(lambda: dsm.extract_dtm(z, grid, NODATA), 3)
    above = dsm.ndsm(z, dtm, NODATA)
    objects = torch.isfinite(above) & (above != NODATA) & (above > MIN_HEIGHT)

    def label_and_stats():
        labels, m = dsm.label(objects, 8)
        return dsm.label_stats(labels, m, values=above, grid=grid, nodata=NODATA), m

    label_ms, (_, n_objects) = host_clock(label_and_stats, 3)
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    p = _lib.ptr
    code = dsm.flow_direction(dtm.contiguous(), grid, NODATA)
    flow_bytes, nbytes = lib.smvs_dsm_flow_workspace_bytes(gw, gh), lib.smvs_dsm_stream_workspace_bytes(gw, gh)
    ws = torch.empty(max(flow_bytes, nbytes), dtype=torch.uint8, device=dev)
    acc = torch.empty((gh, gw), dtype=torch.int64, device=dev)
    word = torch.empty(8, dtype=torch.int32, device=dev)
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "the DTM of bench_dsm_label's grid (%dx%d, %.1f m cells)" % (gw, gh, a.res),
           "cells": n, "kernel_resources": kernel_resources(), "stream_workspace_bytes": nbytes, "extract_dtm_api_ms": dtm_ms,
           "label_and_stats_api_ms": label_ms, "n_objects": int(n_objects), "thresholds": [],
           "root_doubling_rounds": (n - 1).bit_length() + 1, "tour_doubling_rounds": (2 * n - 1).bit_length(), "link_doubling_rounds": (n - 1).bit_length() + 1,
           "order_rounds_launched": min(30, n.bit_length() - 1), "kernel_traces": "not measured", "real_dtms": "not measured"}
    res["flow_accumulate_ms"] = timed(lambda: _lib.call("smvs_dsm_flow_accumulate", p(code), None, gw, gh, p(acc), p(word[4:]), p(ws), flow_bytes, stream), a.reps, a.warmup)
    steps = torch.empty((gh, gw, 3), dtype=torch.int32, device=dev)
    res["flow_length_ms"] = timed(lambda: _lib.call("smvs_dsm_flow_length", p(code), gw, gh, p(steps), p(word[4:]), p(ws), nbytes, stream), a.reps, a.warmup)
    res["longest_flow_path_steps"] = int(steps.sum(dim=2).max().item())
    order = torch.empty((gh, gw), dtype=torch.uint8, device=dev)
    link = torch.empty((gh, gw), dtype=torch.int32, device=dev)
    for t in THRESHOLDS:
        mask = (acc >= t).to(torch.uint8).contiguous()
        row = {"threshold_cells": t}
        row["stream_order_ms"] = timed(lambda: _lib.call("smvs_dsm_stream_order", p(code), p(mask), gw, gh, p(order), p(link), p(word), p(word[4:]), p(ws), nbytes, stream),
                                       a.reps, a.warmup)
        cells, nl, nv, top = (int(x) for x in word[:4].tolist())
        row.update({"stream_cells": cells, "links": nl, "vertices": nv, "highest_order": top, "order_rounds_with_work": top, "cyclic_flag": int(word[4].item())})
        tables = [torch.empty(max(m, 1), dtype=torch.int32, device=dev) for m in (nl, nl, nl, nl + 1, 2 * nv, 3 * nl)]
        if nl:
            row["stream_write_ms"] = timed(lambda: _lib.call("smvs_dsm_stream_write", p(code), p(mask), gw, gh, nl, nv, *[p(t_) for t_ in tables], p(ws), nbytes, stream),
                                           a.reps, a.warmup)
            row["write_accepted_the_counts"] = int(tables[3][nl].item()) == nv
        row["stream_links_api_ms"], links = host_clock(lambda: dsm.stream_links(code, mask, grid=grid), 3)
        row["longest_link_vertices"] = int((links["offset"][1:] - links["offset"][:-1]).max().item()) if nl else 0
        row["network_length_km"] = float(links["length_m"].sum().item()) / 1e3
        res["thresholds"].append(row)
    if a.no_host:
        res["numpy_oracle_host"] = "not measured"
    else:
        import dsm_stream_oracle as so
        side = min(a.host_side, gh, gw)
        crop = code[:side, :side].contiguous()
        crop_acc = dsm.flow_accumulation(crop)
        crop_mask = crop_acc >= 100
        t0 = time.perf_counter()
        want = so.network(crop.cpu().numpy(), crop_mask.cpu().numpy())
        host_ms = 1e3 * (time.perf_counter() - t0)
        got = {k: t_.cpu().numpy() for k, t_ in dsm.stream_links(crop, crop_mask).items()}
        res["numpy_oracle_host"] = {"ms": host_ms, "cells": side * side, "threshold_cells": 100, "links": int(len(want["head"])),
                                    "equal": so.differing(got, {k: want[k] for k in so.KEYS}) == []}
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
