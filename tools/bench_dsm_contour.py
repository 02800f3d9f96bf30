#!/usr/bin/env python
"""Contour timing on one MI355X ("Contours").

Workload: the grid of tools/bench_dsm_label.py (bench_dsm_morph's grid, 2199 x 2158 at the default size), its DTM
(dsm.extract_dtm) and the DSM itself (voids and all), each at intervals of 10, 2 and 0.5 m.  Per case: the number of levels,
crossings, lines and vertices, the rounds of the doubling, and the three native steps of dsm.contours by device events (--reps
calls after --warmup, workspace and outputs allocated outside the timed span): the crossing count (max_cross = 0), the full
count with its link and doubling, the write; then dsm.contours end to end on device tensors (host clock around a synchronise:
allocation and the two reads of the counts included).  Beside them in the same process: dsm.outlines on the nDSM mask, the
vector step the tool chain had before, and, if contourpy imports, its serial generator for the same levels on the host with the
copy of the grid to the host (one run, host clock; the quantised heights, voids masked, corner_mask off).

    python tools/bench_dsm_contour.py [--size 5120] [--reps 10] [--warmup 2] [--no-host] [--json profiles/dsm_contour_bench.json]
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

INTERVALS = (10.0, 2.0, 0.5)
MIN_HEIGHT = 2.5


def contourpy_ms(z, levels):
    """The host route: the grid copied down, contourpy's serial generator, one level at a time.  None if it is not installed."""
    try:
        import contourpy
    except ImportError:
        return None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    zh = z.cpu().numpy()
    ok = np.isfinite(zh) & (zh != np.float32(NODATA)) & (np.abs(zh) <= 32768.0)
    q = np.rint(np.where(ok, zh, 0.0).astype(np.float64) * 256.0) / 256.0
    gen = contourpy.contour_generator(z=np.ma.masked_array(q, mask=~ok), name="serial", corner_mask=False, line_type="Separate")
    n = 0
    for level in levels:
        n += len(gen.lines(float(level)))
    return {"ms": 1e3 * (time.perf_counter() - t0), "n_lines": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=5120)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--res", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--speckle", type=float, default=0.01)
    ap.add_argument("--drop", type=float, default=0.05)
    ap.add_argument("--no-host", action="store_true", help="leave contourpy on the host out")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dsm_contour needs an MI355X")
    dev = torch.device("cuda:0")
    z, grid = bench_grid(a, dev)
    gh, gw = z.shape
    dtm = dsm.extract_dtm(z, grid, NODATA)
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    p = _lib.ptr
    counts = torch.empty(3, dtype=torch.int32, device=dev)
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "bench_dsm_label's grid (%dx%d, %.1f m cells): the DTM and the DSM at intervals of 10, 2 and 0.5 m" % (gw, gh, a.res),
           "cells": gw * gh, "scratch_bytes": scratch_sizes(r"ct_"), "cases": [],
           "kernel_traces": "not measured", "counters": "not measured", "real_dsms": "not measured", "more_than_4096_levels": "not measured"}
    above = dsm.ndsm(z, dtm, NODATA)
    labels, n = dsm.label(torch.isfinite(above) & (above != NODATA) & (above > MIN_HEIGHT), 8)
    outline_ms, rings = host_clock(lambda: dsm.outlines(labels, n), 5)
    res["outlines_ndsm_mask"] = {"n": int(n), "n_vertices": int(rings["vertices"].shape[0]), "outlines_api_ms": outline_ms}
    del rings, labels, above
    for name, surface in (("dtm", dtm), ("dsm", z)):
        for interval in INTERVALS:
            levels = dsm.contour_levels(surface, interval, 0.0, NODATA)
            keys = np.ascontiguousarray(dsm._level_keys(levels), np.int32)
            nl_in = len(keys)
            if not 1 <= nl_in <= dsm.MAX_CONTOUR_LEVELS:
                res["cases"].append({"surface": name, "interval_m": interval, "n_levels": nl_in, "native": "not measured: one native pass takes 1 .. 4096 levels"})
                continue
            kp = keys.ctypes.data_as(ctypes.c_void_p)
            bytes0 = lib.smvs_dsm_contour_workspace_bytes(gw, gh, nl_in, 0)
            ws0 = torch.empty(bytes0, dtype=torch.uint8, device=dev)
            census_ms = timed(lambda: _lib.call("smvs_dsm_contour_count", p(surface), gw, gh, NODATA, kp, nl_in, 0, p(counts), p(ws0), bytes0, stream), a.reps, a.warmup)
            nc = int(counts[0].item())
            nbytes = lib.smvs_dsm_contour_workspace_bytes(gw, gh, nl_in, nc)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            count_ms = timed(lambda: _lib.call("smvs_dsm_contour_count", p(surface), gw, gh, NODATA, kp, nl_in, nc, p(counts), p(ws), nbytes, stream), a.reps, a.warmup)
            nc, nl, nv = counts.tolist()
            out = [torch.empty(nl, dtype=torch.int32, device=dev), torch.empty(nl, dtype=torch.uint8, device=dev), torch.empty(nl + 1, dtype=torch.int32, device=dev),
                   torch.empty(nl_in + 1, dtype=torch.int32, device=dev), torch.empty((nv, 2), dtype=torch.float64, device=dev), torch.empty(nv, dtype=torch.int32, device=dev)]
            write_ms = timed(lambda: _lib.call("smvs_dsm_contour_write", p(surface), gw, gh, NODATA, kp, nl_in, nc, nl, nv, *[p(t) for t in out], p(ws), nbytes, stream),
                             a.reps, a.warmup)
            api_ms, got = host_clock(lambda: dsm.contours(surface, levels=levels, grid=grid, nodata=NODATA), 5)
            rounds = max(0, (nc - 1).bit_length())
            native = census_ms["median"] + count_ms["median"] + write_ms["median"]
            row = {"surface": name, "interval_m": interval, "n_levels": nl_in, "n_cross": nc, "n_lines": nl, "n_vertices": nv, "workspace_bytes": nbytes,
                   "doubling_rounds": rounds, "cross_count_ms": census_ms, "count_ms": count_ms, "write_ms": write_ms, "contours_native_ms": native,
                   "doubling_round_ms_at_most": (count_ms["median"] - census_ms["median"]) / max(rounds, 1), "contours_api_ms": api_ms,
                   "write_offset_ok": int(out[2][-1].item()) == nv,
                   "api_equals_native": bool(torch.equal(got["vertices"].view(torch.int64), out[4].view(torch.int64))) and bool(torch.equal(got["offset"], out[2])),
                   "longest_line_vertices": int((got["offset"][1:] - got["offset"][:-1]).max().item()) if nl else 0,
                   "closed_lines": int(got["closed"].sum().item())}
            if a.no_host:
                row["contourpy_host"] = "not measured"
            else:
                host = contourpy_ms(surface, keys.astype(np.float64) / 512.0)
                row["contourpy_host"] = host if host is not None else "not measured: contourpy is not installed"
                if host is not None:
                    row["contourpy_over_contours_api"] = host["ms"] / api_ms["median"]
                    row["contourpy_lines_equal"] = host["n_lines"] == nl
            res["cases"].append(row)
            del ws, ws0, out, got
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
