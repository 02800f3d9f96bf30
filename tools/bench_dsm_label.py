#!/usr/bin/env python
"""Object-labelling timing on one MI355X ("Objects").

Workload: the grid of tools/bench_dsm_morph.py (bench_dsm_post's grid after despike radius 2), then dsm.extract_dtm and
dsm.ndsm.  Five masks on it: the nDSM mask (valid and above 2.5 m) under connectivity 4 and 8, the grid's void mask (8), a full
mask (8; one component: the worst case for the contention of the statistics) and a checkerboard (4; one component per
foreground cell: the worst case for the compaction).  Device events time --reps calls after --warmup, workspace and outputs
allocated outside the timed span: smvs_dsm_label, then smvs_dsm_label_stats with the nDSM as values on that label map; and
dsm.extract_objects end to end (host clock around a synchronise).  Each mask is held against what a user has without the
native entries, in the same run: the mask copied to the host, scipy.ndimage.label, ndimage.sum / minimum / maximum /
find_objects, and the labels copied back to the device (host clock, --host-reps runs, one for the checkerboard).  The
condition reported: native label + stats, device-resident, not slower than that path on any of the five masks; and the
full-mask statistics at most 3 x the nDSM-mask statistics.  With --oracle the labels and the statistics are also compared with
that path's for equality.

    python tools/bench_dsm_label.py [--size 5120] [--reps 20] [--warmup 3] [--oracle] [--json profiles/dsm_label_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_dsm_morph import NODATA, bench_grid  # noqa: E402
from dsm_bench_common import scratch_sizes, stats, timed  # noqa: E402
from satmvs_amd import _lib, dsm  # noqa: E402

MIN_HEIGHT = 2.5


def host_path(mask, values, conn, ndi, dev):
    """What a user has today: -> (seconds, labels, n, (area, lowest, highest, boxes))."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m, v = mask.cpu().numpy(), values.cpu().numpy()
    labels, n = ndi.label(m, structure=np.ones((3, 3), int) if conn == 8 else None)
    idx = np.arange(1, n + 1)
    area = ndi.sum(m, labels, idx)
    lowest, highest = ndi.minimum(v, labels, idx), ndi.maximum(v, labels, idx)
    boxes = ndi.find_objects(labels)
    back = torch.from_numpy(labels).to(dev)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del back
    return dt, labels, n, (area, lowest, highest, boxes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=5120)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--res", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--speckle", type=float, default=0.01)
    ap.add_argument("--drop", type=float, default=0.05)
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dsm_label needs an MI355X")
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    dev = torch.device("cuda:0")
    z, grid = bench_grid(a, dev)
    gh, gw = z.shape
    above = dsm.ndsm(z, dsm.extract_dtm(z, grid, NODATA), NODATA)
    ok = torch.isfinite(above) & (above != NODATA)
    values = torch.where(ok, above, torch.zeros_like(above)).contiguous()   # every cell valid: the host path knows no nodata
    r, c = torch.meshgrid(torch.arange(gh, device=dev), torch.arange(gw, device=dev), indexing="ij")
    masks = [("ndsm", 4, ok & (above > MIN_HEIGHT)), ("ndsm", 8, ok & (above > MIN_HEIGHT)),
             ("voids", 8, ~(torch.isfinite(z) & (z != NODATA))), ("full", 8, torch.ones_like(ok)), ("checkerboard", 4, (r + c) % 2 == 0)]
    del r, c
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    nbytes = lib.smvs_dsm_label_workspace_bytes(gw, gh)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    labels = torch.empty((gh, gw), dtype=torch.int32, device=dev)
    n_dev = torch.empty(1, dtype=torch.int32, device=dev)
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "bench_dsm_morph's grid (%dx%d, %.1f m cells) after despike, extract_dtm and ndsm; foreground above %.1f m" % (gw, gh, a.res, MIN_HEIGHT),
           "cells": gw * gh, "workspace_bytes": nbytes, "scratch_bytes": scratch_sizes(r"dsm_label"), "masks": [],
           "kernel_traces": "not measured", "counters": "not measured", "real_dsms": "not measured"}
    for name, conn, mask in masks:
        m8 = mask.to(torch.uint8).contiguous()
        label_ms = timed(lambda: _lib.call("smvs_dsm_label", _lib.ptr(m8), gw, gh, conn, _lib.ptr(labels), _lib.ptr(n_dev), _lib.ptr(ws), nbytes, stream),
                         a.reps, a.warmup)
        n = int(n_dev.item())
        out = [torch.empty(n * k, dtype=dt, device=dev) for dt, k in ((torch.int32, 1), (torch.int32, 4), (torch.int64, 2), (torch.int32, 1),
                                                                        (torch.float32, 1), (torch.float32, 1), (torch.int64, 1))]
        stats_ms = timed(lambda: _lib.call("smvs_dsm_label_stats", _lib.ptr(labels), _lib.ptr(values), gw, gh, NODATA, n,
                                           *[_lib.ptr(t) for t in out], stream), a.reps, a.warmup)
        row = {"mask": name, "connectivity": conn, "foreground": int(m8.sum()), "n": n, "label_ms": label_ms, "stats_ms": stats_ms,
               "native_ms": label_ms["median"] + stats_ms["median"]}
        if ndi is None:
            row["host_ms"] = row["equal"] = "not measured (no scipy)"
        else:
            runs = [host_path(m8, values, conn, ndi, dev) for _ in range(1 if name == "checkerboard" else a.host_reps)]
            row["host_ms"] = stats([1e3 * t[0] for t in runs])
            row["host_over_native"] = row["host_ms"]["median"] / row["native_ms"]
            row["condition_native_not_slower"] = bool(row["native_ms"] <= row["host_ms"]["median"])
            if a.oracle:
                _, want, nw, (area, lowest, highest, boxes) = runs[0]
                boxes = np.array([[s[0].start, s[1].start, s[0].stop - 1, s[1].stop - 1] for s in boxes], np.int32).reshape(nw, 4)
                row["equal"] = bool(nw == n and np.array_equal(labels.cpu().numpy(), want)
                                    and np.array_equal(out[0].cpu().numpy(), area.astype(np.int32))
                                    and np.array_equal(out[1].cpu().numpy().reshape(n, 4), boxes)
                                    and np.array_equal(out[4].cpu().numpy(), np.asarray(lowest, np.float32))
                                    and np.array_equal(out[5].cpu().numpy(), np.asarray(highest, np.float32)))
            else:
                row["equal"] = "not measured"
        res["masks"].append(row)
        del out
    by = {(row["mask"], row["connectivity"]): row for row in res["masks"]}
    res["full_stats_over_ndsm_stats"] = by[("full", 8)]["stats_ms"]["median"] / by[("ndsm", 8)]["stats_ms"]["median"]
    res["condition_full_stats_at_most_3x_ndsm_stats"] = bool(res["full_stats_over_ndsm_stats"] <= 3.0)
    if ndi is not None:
        res["condition_native_not_slower_on_every_mask"] = all(row["condition_native_not_slower"] for row in res["masks"])
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        obj_labels, obj_stats = dsm.extract_objects(above, grid, MIN_HEIGHT, nodata=NODATA)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    res["extract_objects_api_ms"] = stats(ts)
    res["extract_objects_kept"] = int(obj_stats["area"].numel())
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
