#!/usr/bin/env python
"""Registration timing on one MI355X ("Registration").

Workload: the grid of tools/bench_dsm_morph.py (bench_dsm_post's grid after despike radius 2) as the fixed DSM b, and as the
moving DSM a a copy displaced by (--sx, --sy) cells and --dz metres with sigma = 0.3 m noise and 2 % more voids.  Device events
time --reps calls after --warmup, workspace and outputs allocated outside the timed span: smvs_dsm_shift_stats at radius 4, 8,
16 and 32 (dz0 = 0, trim = 256), and smvs_dsm_regrid in both modes onto a grid half a cell off.  Each radius up to
--composite-radius is held against the same statistics from a torch-on-device composite written here (float64 grids with NaN
at invalid cells made once per call, then one pass per shift over slices of both, int64 sums), timed in the same run with
--composite-reps calls.  The conditions reported: native not slower than the composite at radius 8 and at radius 16, and the
native statistics equal to the composite's; and whether dsm.coregister returns the displacement.

    python tools/bench_dsm_coreg.py [--size 5120] [--reps 20] [--warmup 3] [--json profiles/dsm_coreg_bench.json]
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

RADII = (4, 8, 16, 32)


def displaced_copy(z, sx, sy, dz, dev, seed=0):
    """a with a[r + sy, c + sx] = z[r, c] + dz + noise; the cells that wrapped around and 2 % of the others are nodata."""
    g = torch.Generator(device=dev).manual_seed(seed)
    gh, gw = z.shape
    ok = torch.isfinite(z) & (z != NODATA)
    a = torch.where(ok, z + dz + 0.3 * torch.randn(z.shape, device=dev, generator=g), z)
    a = torch.roll(a, (sy, sx), (0, 1))
    r, c = torch.meshgrid(torch.arange(gh, device=dev), torch.arange(gw, device=dev), indexing="ij")
    wrapped = (r - sy < 0) | (r - sy >= gh) | (c - sx < 0) | (c - sx >= gw)
    a[wrapped | (torch.rand(z.shape, device=dev, generator=g) < 0.02)] = NODATA
    return a.contiguous()


def composite(a, b, radius, dz0, trim):
    """The statistics with torch operators: one pass per shift, int64 sums.  -> (2R + 1, 2R + 1, 3) int64."""
    gh, gw = b.shape
    nan = torch.full((), float("nan"), dtype=torch.float64, device=a.device)
    a64 = torch.where(torch.isfinite(a) & (a != NODATA), a.double(), nan)
    b64 = torch.where(torch.isfinite(b) & (b != NODATA), b.double(), nan)
    S = 2 * radius + 1
    out = torch.zeros((S, S, 3), dtype=torch.int64, device=a.device)
    for sy in range(-radius, radius + 1):
        r0, r1 = max(0, -sy), min(gh, a.shape[0] - sy)
        for sx in range(-radius, radius + 1):
            c0, c1 = max(0, -sx), min(gw, a.shape[1] - sx)
            d = (a64[r0 + sy:r1 + sy, c0 + sx:c1 + sx] - b64[r0:r1, c0:c1]) - dz0
            ok = d.abs() <= trim
            q = torch.where(ok, torch.round(d * 256.0), torch.zeros_like(d)).to(torch.int64)
            out[sy + radius, sx + radius, 0] = ok.sum()
            out[sy + radius, sx + radius, 1] = q.sum()
            out[sy + radius, sx + radius, 2] = (q * q).sum()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=5120)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--res", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--composite-reps", type=int, default=3)
    ap.add_argument("--composite-radius", type=int, default=16)
    ap.add_argument("--speckle", type=float, default=0.01)
    ap.add_argument("--drop", type=float, default=0.05)
    ap.add_argument("--sx", type=int, default=5)
    ap.add_argument("--sy", type=int, default=-3)
    ap.add_argument("--dz", type=float, default=2.75)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dsm_coreg needs an MI355X")
    dev = torch.device("cuda:0")
    zb, grid = bench_grid(a, dev)
    gh, gw = zb.shape
    za = displaced_copy(zb, a.sx, a.sy, a.dz, dev)
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "bench_dsm_morph's grid (%dx%d, %.1f m cells) against a copy displaced by (%d, %d) cells and %.2f m, sigma 0.3 m noise, 2 %% more voids"
                       % (gw, gh, a.res, a.sx, a.sy, a.dz),
           "cells": gw * gh, "scratch_bytes": scratch_sizes(r"dsm_shift|dsm_regrid"), "shift_stats": [], "regrid": [],
           "kernel_traces": "not measured", "counters": "not measured", "real_dsms": "not measured",
           "subcell_accuracy_beyond_the_synthetic_scene": "not measured"}
    for radius in RADII:
        nbytes = lib.smvs_dsm_shift_workspace_bytes(gw, gh, gw, gh, radius)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty((2 * radius + 1, 2 * radius + 1, 3), dtype=torch.int64, device=dev)
        ms = timed(lambda: _lib.call("smvs_dsm_shift_stats", _lib.ptr(za), gw, gh, _lib.ptr(zb), gw, gh, NODATA, 0, 0, radius, 0.0, 256.0,
                                     _lib.ptr(out), _lib.ptr(ws), nbytes, stream), a.reps, a.warmup)
        pairs = gw * gh * (2 * radius + 1) ** 2
        row = {"radius": radius, "shifts": (2 * radius + 1) ** 2, "workspace_bytes": nbytes, "native_ms": ms,
               "cell_pairs_per_s": pairs / (1e-3 * ms["median"])}
        if radius <= a.composite_radius:
            want = composite(za, zb, radius, 0.0, 256.0)     # also the warm-up
            ts = []
            for _ in range(a.composite_reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                composite(za, zb, radius, 0.0, 256.0)
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t0))
            row["composite_ms"] = stats(ts)
            row["composite_over_native"] = row["composite_ms"]["median"] / ms["median"]
            row["condition_native_not_slower"] = bool(ms["median"] <= row["composite_ms"]["median"])
            row["equal"] = bool(torch.equal(out, want))
        else:
            row["composite_ms"] = row["equal"] = "not measured"
        res["shift_stats"].append(row)
        del ws, out
    by = {row["radius"]: row for row in res["shift_stats"]}
    res["condition_native_not_slower_at_radius_8_and_16"] = bool(by[8].get("condition_native_not_slower") is True and by[16].get("condition_native_not_slower") is True)
    res["condition_native_equals_composite"] = all(row["equal"] is True for row in res["shift_stats"] if row["equal"] != "not measured")
    to = dsm.DSMGrid(grid.e0 + 0.5 * grid.xres, grid.n0 - 0.5 * grid.yres, grid.xres, grid.yres, gw, gh)
    out = torch.empty((gh, gw), dtype=torch.float32, device=dev)
    for mode, code in sorted(dsm.REGRID_MODES.items()):
        g4s, g4d = grid.grid4(), to.grid4()
        ms = timed(lambda: _lib.call("smvs_dsm_regrid", _lib.ptr(za), gw, gh, g4s.ctypes.data, NODATA, g4d.ctypes.data, gw, gh, code, 0.0,
                                     _lib.ptr(out), stream), a.reps, a.warmup)
        res["regrid"].append({"mode": mode, "ms": ms, "cells_per_s": gw * gh / (1e-3 * ms["median"])})
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reg = dsm.coregister(za, grid, zb, grid, radius=8)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    res["coregister_api_ms"] = stats(ts)
    res["displacement"] = {"truth": [a.sx, a.sy, a.dz], "shift_cells": list(reg["shift_cells"]), "subcell": list(reg["subcell"]), "dz": reg["dz"],
                           "std": reg["std"], "n": reg["n"]}
    res["displacement_recovered"] = bool(tuple(reg["shift_cells"]) == (a.sx, a.sy) and abs(reg["dz"] - a.dz) < 0.05)
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
