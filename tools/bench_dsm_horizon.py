#!/usr/bin/env python
"""Horizon maps, and sun exposure through them, timed on one MI355X ("Horizon").

Workload: the grid of tools/bench_dsm_sun.py (bench_dsm_morph's grid after despike radius 2).  Device events time --reps calls
after --warmup, workspace and outputs allocated outside the timed span.
smvs_dsm_horizon at K = 1, 8, 16, 32 and 64 evenly spaced azimuths (min, median, max; per direction; per cell and direction), a
batch of 8 row-major directions and one of 8 column-major ones, and the workspace of each call.  From the same run:
smvs_dsm_shadow per sun, dsm.sun_exposure over the 24 suns of bench_dsm_sun, and dsm.sun_exposure_from_horizon over the same
suns including its 16-direction horizon (host clock around a synchronise, median of 3), with the mean and largest absolute
difference between the two exposures: the price of 16 directions and interpolation.  No time is a condition.

    python tools/bench_dsm_horizon.py [--size 5120] [--reps 20] [--warmup 3] [--json profiles/dsm_horizon_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_dsm_morph import NODATA, bench_grid  # noqa: E402
from bench_dsm_sun import host_timed  # noqa: E402
from dsm_bench_common import scratch_sizes, timed  # noqa: E402
from satmvs_amd import _lib, dsm  # noqa: E402

BATCHES = (1, 8, 16, 32, 64)
ROW_MAJOR = (0.0, 10.0, 20.0, 30.0, 170.0, 180.0, 190.0, 200.0)
COLUMN_MAJOR = (60.0, 75.0, 90.0, 105.0, 240.0, 255.0, 270.0, 285.0)


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
        sys.exit("bench_dsm_horizon needs an MI355X")
    dev = torch.device("cuda:0")
    z, grid = bench_grid(a, dev)
    gh, gw = z.shape
    cells = gw * gh
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    void = 1.0 - float((torch.isfinite(z) & (z != NODATA)).float().mean())
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "bench_dsm_morph's grid (%dx%d, %.1f m cells) after despike radius 2, void share %.4f" % (gw, gh, a.res, void),
           "cells": cells, "scratch_bytes": scratch_sizes(r"dsm_horizon"), "horizon": [],
           "kernel_traces": "not measured", "counters": "not measured", "real_dsms": "not measured",
           "strided_column_major_stores": "not built"}

    def horizon_row(name, azimuths):
        K = len(azimuths)
        dirs = np.ascontiguousarray(np.array([dsm.horizon_terms(grid, az) for az in azimuths], np.float64))
        nbytes = lib.smvs_dsm_horizon_workspace_bytes(gw, gh, K)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty((K, gh, gw), dtype=torch.float32, device=dev)
        ms = timed(lambda: _lib.call("smvs_dsm_horizon", _lib.ptr(z), gw, gh, NODATA, dirs.ctypes.data_as(_lib.C.c_void_p), K, _lib.ptr(out),
                                     _lib.ptr(ws), nbytes, stream), a.reps, a.warmup)
        columns = sum(1 for d in dirs if abs(d[1]) < abs(d[0]))
        res["horizon"].append({"batch": name, "directions": K, "column_major": columns, "workspace_bytes": nbytes, "ms": ms,
                               "ms_per_direction": ms["median"] / K, "ns_per_cell_and_direction": 1e6 * ms["median"] / (K * cells),
                               "open_share": float(torch.isinf(out).float().mean())})
        del ws, out

    for K in BATCHES:
        horizon_row("%d evenly spaced" % K, dsm.horizon_azimuths(K))
    horizon_row("8 row-major", ROW_MAJOR)
    horizon_row("8 column-major", COLUMN_MAJOR)

    suns = [(90.0 + 7.5 * i, 10.0 + 50.0 * (1.0 - abs(i - 11.5) / 11.5)) for i in range(24)]      # east to west over a day: bench_dsm_sun's
    nbytes = lib.smvs_dsm_shadow_workspace_bytes(gw, gh)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    shade = torch.empty((gh, gw), dtype=torch.uint8, device=dev)
    res["shadow_per_sun"] = []
    for az, el in (suns[0], suns[6], suns[12]):
        t = dsm.sun_terms(grid, az, el)
        ms = timed(lambda: _lib.call("smvs_dsm_shadow", _lib.ptr(z), gw, gh, NODATA, t[0], t[1], t[2], t[3], 0.1, _lib.ptr(shade), None,
                                     _lib.ptr(ws), nbytes, stream), a.reps, a.warmup)
        res["shadow_per_sun"].append({"azimuth": az, "elevation": el, "ms": ms})
    del ws, shade
    listed = dsm.horizon_azimuths(16)
    res["sun_exposure_24_suns_api_ms"] = host_timed(lambda: dsm.sun_exposure(z, grid, suns, nodata=NODATA))
    res["sun_exposure_from_horizon_24_suns_api_ms"] = host_timed(
        lambda: dsm.sun_exposure_from_horizon(z, grid, dsm.horizon(z, grid, listed, nodata=NODATA), listed, suns, nodata=NODATA))
    tan_h = dsm.horizon(z, grid, listed, nodata=NODATA)
    res["horizon_16_api_ms"] = host_timed(lambda: dsm.horizon(z, grid, listed, nodata=NODATA))
    res["exposure_from_16_maps_24_suns_api_ms"] = host_timed(lambda: dsm.sun_exposure_from_horizon(z, grid, tan_h, listed, suns, nodata=NODATA))
    per_sun = (res["sun_exposure_24_suns_api_ms"]["median"]) / 24.0
    per_sun_h = res["exposure_from_16_maps_24_suns_api_ms"]["median"] / 24.0
    res["suns_from_which_the_horizon_route_is_faster"] = (
        int(np.floor(res["horizon_16_api_ms"]["median"] / (per_sun - per_sun_h))) + 1 if per_sun > per_sun_h else None)
    direct = dsm.sun_exposure(z, grid, suns, nodata=NODATA).double()
    routed = dsm.sun_exposure_from_horizon(z, grid, tan_h, listed, suns, nodata=NODATA).double()
    both = ~torch.isnan(direct) & ~torch.isnan(routed)
    diff = (direct - routed).abs()[both]
    res["exposure_difference"] = {"mean_abs": float(diff.mean()), "max_abs": float(diff.max()), "mean_exposure": float(direct[both].mean()),
                                  "cells_that_differ": float((diff > 0).double().mean()), "tol_of_sun_exposure": 0.1}
    res["sky_view_factor_16_api_ms"] = host_timed(lambda: dsm.sky_view_factor(tan_h))
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
