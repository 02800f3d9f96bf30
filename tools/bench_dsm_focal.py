#!/usr/bin/env python
"""Focal statistics timing on one MI355X ("Focal statistics").

Workload: the grid of tools/bench_dsm_label.py (bench_dsm_morph's grid, 2199 x 2158 at the default size, after despike radius 2).
Device events time --reps calls after --warmup, buffers allocated outside the timed span: smvs_dsm_focal_build; smvs_dsm_focal_query
with all five outputs for a box, a disc and an annulus (inner = radius / 2) at radii 4, 32, 256 and 1024 cells (a window the entry
does not serve -- more than 1024 records -- is listed with the reason); beside them in the same process a torch composite of the
same rule (two int64 cumsums per table, then slicing by clamped corner indices per record), whose n, s1 and s2 are asserted equal to
the native ones in every integer before it is timed, and dsm.morph "open" at the same radii (it serves radii up to 256).  dsm.tpi end
to end (tables, window, query, the float32 grid) and dsm.aggregate at factors 2 and 8 are under a host clock round a synchronise.

    python tools/bench_dsm_focal.py [--size 5120] [--reps 20] [--warmup 3] [--json profiles/dsm_focal_bench.json]
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
from bench_dsm_morph import NODATA, bench_grid  # noqa: E402
from dsm_bench_common import scratch_sizes, stats, timed  # noqa: E402
from satmvs_amd import _lib, dsm  # noqa: E402

RADII = (4, 32, 256, 1024)
COMPOSITE_MAX_RECORDS = 512                                  # the composite costs 12 gathers of the grid per record


def host_clock(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return stats(ts), out


def composite_tables(z, nodata):
    """The rule in torch: (centre, N, S1, S2) with a zero first row and column, int64 (S2 wraps as int64 sums do)."""
    ok = torch.isfinite(z) & (z != nodata) & (z.abs() <= 32768.0)
    q = torch.round(torch.where(ok, z, torch.zeros_like(z)).double() * 256.0).long()
    c = (int(q[ok].min()) + int(q[ok].max())) >> 1 if bool(ok.any()) else 0
    d = torch.where(ok, q - c, torch.zeros_like(q))
    pad = lambda t: torch.nn.functional.pad(t.cumsum(0).cumsum(1), (1, 0, 1, 0))
    return c, pad(ok.long()), pad(d), pad(d * d)


def composite_query(tabs, rects, gw, gh):
    rows, cols = torch.arange(gh, device=tabs[0].device), torch.arange(gw, device=tabs[0].device)
    out = [torch.zeros((gh, gw), dtype=torch.int64, device=tabs[0].device) for _ in tabs]
    for dx0, dx1, dy0, dy1, sign in rects.tolist():
        x0, y0 = (cols + dx0).clamp(0, gw), (rows + dy0).clamp(0, gh)
        x1, y1 = torch.maximum((cols + dx1 + 1).clamp(0, gw), x0), torch.maximum((rows + dy1 + 1).clamp(0, gh), y0)
        for o, T in zip(out, tabs):
            o += sign * (T[y1][:, x1] - T[y0][:, x1] - T[y1][:, x0] + T[y0][:, x0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=5120)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--res", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--speckle", type=float, default=0.01)
    ap.add_argument("--drop", type=float, default=0.05)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dsm_focal needs an MI355X")
    dev = torch.device("cuda:0")
    z, grid = bench_grid(a, dev)
    z = z.contiguous()
    gh, gw = z.shape
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    nbytes = lib.smvs_dsm_focal_table_bytes(gw, gh)
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "bench_dsm_morph's grid (%dx%d, %.1f m cells) after despike" % (gw, gh, a.res), "cells": gw * gh,
           "table_bytes": nbytes, "build_bytes_least": gw * gh * 24, "scratch_bytes": scratch_sizes(r"dsm_focal_"), "launches_per_build": 7,
           "windows": [], "fused_tile_build": "not built", "kernel_traces": "not measured", "counters": "not measured", "real_dsms": "not measured"}
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    res["build_ms"] = timed(lambda: _lib.call("smvs_dsm_focal_build", _lib.ptr(z), gw, gh, NODATA, _lib.ptr(buf), nbytes, stream), a.reps, a.warmup)
    t0 = composite_tables(z, NODATA)
    res["torch_composite_build_ms"] = timed(lambda: composite_tables(z, NODATA), max(3, a.reps // 4), 1)
    tables = dsm.focal_tables(z, NODATA)
    assert tables.centre == t0[0]
    outs = [torch.empty((gh, gw), dtype=dt, device=dev) for dt in (torch.int32, torch.int64, torch.int64, torch.float64, torch.float64)]
    status = torch.empty(1, dtype=torch.int32, device=dev)

    def query(rects):
        _lib.call("smvs_dsm_focal_query", _lib.ptr(buf), gw, gh, rects.ctypes.data, len(rects), gw, gh, 0, 0, 1, 1, 1, *[_lib.ptr(t) for t in outs],
                  _lib.ptr(status), stream)

    for radius in RADII:
        morph_ms = timed(lambda: dsm.morph(z, radius, "open", NODATA), a.reps, a.warmup) if radius <= dsm.MAX_MORPH_RADIUS else "not served: morph takes radii up to %d" % dsm.MAX_MORPH_RADIUS
        for shape in dsm.FOCAL_SHAPES:
            row = {"shape": shape, "radius": radius, "morph_open_ms": morph_ms}
            try:
                w = dsm.focal_window(shape, radius, radius / 2 if shape == "annulus" else None)
            except ValueError as e:
                row["query_ms"] = "not served: %s" % e
                res["windows"].append(row)
                continue
            row.update({"records": len(w.rects), "cells": w.cells})
            row["query_ms"] = timed(lambda: query(w.rects), a.reps, a.warmup)
            assert int(status) == 0
            if len(w.rects) <= COMPOSITE_MAX_RECORDS:
                want = composite_query(t0[1:], w.rects, gw, gh)
                assert all(torch.equal(g.long(), t) for g, t in zip(outs[:3], want)), (shape, radius)
                row["composite_equal"] = True
                row["torch_composite_query_ms"] = timed(lambda: composite_query(t0[1:], w.rects, gw, gh), 3, 1)
                row["composite_over_query"] = row["torch_composite_query_ms"]["median"] / row["query_ms"]["median"]
            else:
                row["torch_composite_query_ms"] = "not measured: %d records" % len(w.rects)
            res["windows"].append(row)
    res["tpi_api_ms"] = {str(r): host_clock(lambda: dsm.tpi(z, grid, r * a.res, nodata=NODATA), 5)[0] for r in (4, 32, 256)}
    res["aggregate_api_ms"] = {str(f): host_clock(lambda: dsm.aggregate(z, grid, f, nodata=NODATA), 5)[0] for f in (2, 8)}
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
