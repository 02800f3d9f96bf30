#!/usr/bin/env python
"""Cast shadows, gradient, hillshade and sun exposure timing on one MI355X ("Sun").

Workload: the grid of tools/bench_dsm_morph.py (bench_dsm_post's grid after despike radius 2).  Device events time --reps calls
after --warmup, workspace and outputs allocated outside the timed span.
smvs_dsm_shadow: azimuths 0, 33, 90, 123 at elevations 20 and 45 (0 and 33 scan along the rows, 90 and 123 along the columns,
through the transposes), with and without the depth output, against a torch-on-device composite of the same rule written here
and timed in the same run: a sheared scatter of the keys, torch.cummax, a shift by one, a gather back (the column-major
directions on the transposed grid, as the rule's symmetry allows).  Conditions, stated before the run, no margin: shade and
depth have equal bits with the composite's; the native call is not slower than the composite; the column-major directions cost
at most twice the row-major ones.  A condition that fails is reported as failed, with its numbers.
smvs_dsm_gradient alone, dsm.hillshade(shadows=True) and dsm.sun_exposure over 24 suns (host clock around a synchronise,
median of 3).

    python tools/bench_dsm_sun.py [--size 5120] [--reps 20] [--warmup 3] [--json profiles/dsm_sun_bench.json]
"""
import argparse
import json
import math
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

AZIMUTHS = (0.0, 33.0, 90.0, 123.0)
ELEVATIONS = (20.0, 45.0)
TOL = 0.1
LOW63 = 0x7fffffffffffffff
MINKEY = -0x7ff0000000000001                                 # the key of -inf


def host_timed(fn, reps=3):
    fn()                                                     # warm-up
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return stats(ts)


def _key(g):
    u = g.view(torch.int64)
    return u ^ ((u >> 63) & LOW63)


def composite(z, ucol, urow, a, b, tol):
    """The shadow rule with torch operators -> (shade uint8, depth float32)."""
    if abs(urow) < abs(ucol):
        shade, depth = composite(z.t().contiguous(), urow, ucol, b, a, tol)
        return shade.t().contiguous(), depth.t().contiguous()
    H, W = z.shape
    dev = z.device
    rows = torch.arange(H, device=dev, dtype=torch.float64)
    s = torch.floor((ucol / urow) * rows + 0.5).long()
    last = int(math.floor((ucol / urow) * float(H - 1) + 0.5))                # s is monotone from s(0) = 0: no read-back
    smax, smin = max(last, 0), min(last, 0)
    nl = W + smax - smin
    slot = torch.arange(W, device=dev)[None, :] - s[:, None] + smax
    ok = torch.isfinite(z) & (z != NODATA)
    g = z.double() - (a * torch.arange(W, device=dev, dtype=torch.float64)[None, :] + b * rows[:, None])
    sheared = torch.full((H, nl), MINKEY, dtype=torch.int64, device=dev)
    sheared.scatter_(1, slot, torch.where(ok, _key(g), torch.full_like(slot, MINKEY)))
    if urow > 0:                                             # sunward order is descending r
        sheared = sheared.flip(0)
    acc = torch.cummax(sheared, dim=0).values
    acc = torch.cat([torch.full((1, nl), MINKEY, dtype=torch.int64, device=dev), acc[:-1]], dim=0)       # exclusive
    if urow > 0:
        acc = acc.flip(0)
    d = _key(acc.gather(1, slot)).view(torch.float64) - g
    shade = torch.where(ok, torch.where(d > tol, 2, 1), 0).to(torch.uint8)
    return shade, torch.where(ok, d.float(), torch.full_like(z, NODATA))


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
        sys.exit("bench_dsm_sun needs an MI355X")
    dev = torch.device("cuda:0")
    z, grid = bench_grid(a, dev)
    gh, gw = z.shape
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    void = 1.0 - float((torch.isfinite(z) & (z != NODATA)).float().mean())
    nbytes = lib.smvs_dsm_shadow_workspace_bytes(gw, gh)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    shade = torch.empty((gh, gw), dtype=torch.uint8, device=dev)
    depth = torch.empty((gh, gw), dtype=torch.float32, device=dev)
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "bench_dsm_morph's grid (%dx%d, %.1f m cells) after despike radius 2, void share %.4f" % (gw, gh, a.res, void),
           "cells": gw * gh, "workspace_bytes": nbytes, "scratch_bytes": scratch_sizes(r"dsm_sun"), "shadow": [],
           "kernel_traces": "not measured", "counters": "not measured", "real_dsms": "not measured"}
    for elevation in ELEVATIONS:
        for azimuth in AZIMUTHS:
            t = dsm.sun_terms(grid, azimuth, elevation)

            def native(dp):
                _lib.call("smvs_dsm_shadow", _lib.ptr(z), gw, gh, NODATA, t[0], t[1], t[2], t[3], TOL, _lib.ptr(shade), dp, _lib.ptr(ws), nbytes, stream)

            ms_bare = timed(lambda: native(None), a.reps, a.warmup)
            ms = timed(lambda: native(_lib.ptr(depth)), a.reps, a.warmup)
            want = composite(z, *t, TOL)
            cms = timed(lambda: composite(z, *t, TOL), a.reps, a.warmup)
            res["shadow"].append({"azimuth": azimuth, "elevation": elevation, "major": "rows" if abs(t[1]) >= abs(t[0]) else "columns",
                                  "native_ms": ms, "native_shade_only_ms": ms_bare, "composite_ms": cms,
                                  "composite_over_native": cms["median"] / ms["median"],
                                  "condition_native_not_slower": bool(ms["median"] <= cms["median"]),
                                  "equal_bits": bool(torch.equal(shade, want[0]) and torch.equal(depth.view(torch.int32), want[1].view(torch.int32))),
                                  "shadowed_share": float((shade == 2).float().mean()), "cells_per_s": gw * gh / (1e-3 * ms["median"])})
            del want
    by = lambda major, key: [r[key]["median"] for r in res["shadow"] if r["major"] == major]
    res["columns_over_rows"] = max(by("columns", "native_ms")) / min(by("rows", "native_ms"))
    res["columns_over_rows_shade_only"] = max(by("columns", "native_shade_only_ms")) / min(by("rows", "native_shade_only_ms"))
    res["condition_shadow_equals_composite"] = all(r["equal_bits"] for r in res["shadow"])
    res["condition_shadow_not_slower_than_composite"] = all(r["condition_native_not_slower"] for r in res["shadow"])
    res["condition_columns_at_most_twice_rows"] = bool(res["columns_over_rows"] <= 2.0)
    dzde, dzdn = torch.empty_like(z), torch.empty_like(z)
    gms = timed(lambda: _lib.call("smvs_dsm_gradient", _lib.ptr(z), gw, gh, NODATA, float(grid.xres), float(grid.yres), _lib.ptr(dzde), _lib.ptr(dzdn), stream),
                a.reps, a.warmup)
    res["gradient"] = {"native_ms": gms, "cells_per_s": gw * gh / (1e-3 * gms["median"])}
    res["hillshade_with_shadows_api_ms"] = host_timed(lambda: dsm.hillshade(z, grid, 315.0, 45.0, shadows=True, nodata=NODATA))
    suns = [(90.0 + 7.5 * i, 10.0 + 50.0 * (1.0 - abs(i - 11.5) / 11.5)) for i in range(24)]      # east to west over a day
    res["sun_exposure_24_suns_api_ms"] = host_timed(lambda: dsm.sun_exposure(z, grid, suns, nodata=NODATA))
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
