#!/usr/bin/env python
"""Distance transform and mosaic timing on one MI355X ("Mosaic").

Workload: the grid of tools/bench_dsm_morph.py (bench_dsm_post's grid after despike radius 2).  Device events time --reps calls
after --warmup, workspace and outputs allocated outside the timed span.
smvs_dsm_dist: the grid's validity mask with border = 1 at max_dist 16, 64, 256 and 1024, each checked against
scipy.ndimage.distance_transform_edt of the padded mask, which is timed on the host with its copies (host clock, median of 3).
Condition: the native call is not slower.
smvs_dsm_mosaic: four quadrant tiles of the grid overlapping by --overlap cells, modes first and feather (feather 16 and 64, d2
made outside the timed span), against a torch-on-device composite of the same rule written here and timed in the same run:
the tiles sliced into NaN-padded float64 canvases, then the sums in the layers' order.  Conditions, stated before the run, no
margin: the native mosaic is not slower than the composite in either mode, and their outputs have equal bits.  Also the whole
dsm.mosaic call with its four transforms (host clock, median of 3).

    python tools/bench_dsm_mosaic.py [--size 5120] [--reps 20] [--warmup 3] [--json profiles/dsm_mosaic_bench.json]
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

CAPS = (16, 64, 256, 1024)


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


def composite(tiles, d2s, offsets, mode, feather, gw, gh):
    """The mosaic's rule with torch operators: NaN-padded float64 canvases, then the sums in the layers' order -> float32."""
    dev = tiles[0].device
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    S = torch.full((gh, gw), float("nan"), dtype=torch.float64, device=dev)
    W = torch.full((gh, gw), float("nan"), dtype=torch.float64, device=dev)
    for z, d2, (ox, oy) in zip(tiles, d2s, offsets):
        h, w = z.shape
        canvas = torch.full((gh, gw), float("nan"), dtype=torch.float64, device=dev)
        canvas[oy:oy + h, ox:ox + w] = torch.where(torch.isfinite(z) & (z != NODATA), z.double(), nan)
        here = ~torch.isnan(canvas)
        first = here & torch.isnan(S)
        if mode == "first":
            S = torch.where(first, canvas, S)
            continue
        wc = torch.ones((gh, gw), dtype=torch.float64, device=dev)
        wc[oy:oy + h, ox:ox + w] = d2.clamp(1, feather * feather).double().sqrt()
        wz = wc * canvas
        S = torch.where(first, wz, torch.where(here, S + wz, S))
        W = torch.where(first, wc, torch.where(here, W + wc, W))
    out = S if mode == "first" else S / W
    return torch.where(torch.isnan(out), torch.full_like(out, NODATA), out).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=5120)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--res", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--speckle", type=float, default=0.01)
    ap.add_argument("--drop", type=float, default=0.05)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dsm_mosaic needs an MI355X")
    dev = torch.device("cuda:0")
    z, grid = bench_grid(a, dev)
    gh, gw = z.shape
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    valid = (torch.isfinite(z) & (z != NODATA)).to(torch.uint8).contiguous()
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "bench_dsm_morph's grid (%dx%d, %.1f m cells) after despike radius 2, void share %.4f" % (gw, gh, a.res, 1.0 - float(valid.float().mean())),
           "cells": gw * gh, "scratch_bytes": scratch_sizes(r"dsm_dist|dsm_mosaic"), "dist": [], "mosaic": [],
           "kernel_traces": "not measured", "counters": "not measured", "real_dsms": "not measured"}
    # ---- the transform -------------------------------------------------------------------------------------------------------
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    edt2 = None
    if ndimage is not None:
        def on_host():
            m = np.pad(valid.cpu().numpy(), 1)
            return torch.from_numpy(ndimage.distance_transform_edt(m)[1:-1, 1:-1]).to(dev)
        res["scipy_edt_ms"] = host_timed(on_host)
        edt2 = torch.round(on_host() ** 2).to(torch.int64)
    else:
        res["scipy_edt_ms"] = "not measured (scipy is not installed)"
    d2 = torch.empty((gh, gw), dtype=torch.int32, device=dev)
    for cap in CAPS:
        nbytes = lib.smvs_dsm_dist_workspace_bytes(gw, gh, cap)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ms = timed(lambda: _lib.call("smvs_dsm_dist", _lib.ptr(valid), gw, gh, 1, cap, _lib.ptr(d2), _lib.ptr(ws), nbytes, stream), a.reps, a.warmup)
        row = {"max_dist": cap, "workspace_bytes": nbytes, "native_ms": ms, "cells_per_s": gw * gh / (1e-3 * ms["median"]),
               "largest_d2": int(d2.max())}
        if edt2 is not None:
            row["equals_scipy"] = bool(torch.equal(d2.to(torch.int64), edt2.clamp(max=cap * cap)))
            row["scipy_over_native"] = res["scipy_edt_ms"]["median"] / ms["median"]
            row["condition_native_not_slower"] = bool(ms["median"] <= res["scipy_edt_ms"]["median"])
        res["dist"].append(row)
        del ws
    # ---- the mosaic ----------------------------------------------------------------------------------------------------------
    hr, hc, o = gh // 2, gw // 2, a.overlap // 2
    cuts = [(0, hr + o, 0, hc + o), (0, hr + o, hc - o, gw), (hr - o, gh, 0, hc + o), (hr - o, gh, hc - o, gw)]
    tiles = [z[r0:r1, c0:c1].contiguous() for r0, r1, c0, c1 in cuts]
    offsets = [(c0, r0) for r0, r1, c0, c1 in cuts]
    grids = [dsm.DSMGrid(grid.e0 + c0 * grid.xres, grid.n0 - r0 * grid.yres, grid.xres, grid.yres, c1 - c0, r1 - r0) for r0, r1, c0, c1 in cuts]
    out = torch.empty((gh, gw), dtype=torch.float32, device=dev)
    for mode, feather in (("first", 1), ("feather", 16), ("feather", 64)):
        d2s = [dsm._dist((torch.isfinite(t) & (t != NODATA)).to(torch.uint8), feather, True) if mode == "feather" else None for t in tiles]
        table = (dsm._Layer * 4)(*[dsm._Layer(t.data_ptr(), d.data_ptr() if d is not None else None, t.shape[1], t.shape[0], ox, oy)
                                   for t, d, (ox, oy) in zip(tiles, d2s, offsets)])
        ms = timed(lambda: _lib.call("smvs_dsm_mosaic", table, 4, NODATA, dsm.MOSAIC_MODES[mode], feather, gw, gh, _lib.ptr(out), None, None, None, stream),
                   a.reps, a.warmup)
        want = composite(tiles, d2s, offsets, mode, feather, gw, gh)
        cms = host_timed(lambda: composite(tiles, d2s, offsets, mode, feather, gw, gh))
        api = host_timed(lambda: dsm.mosaic(tiles, grids, to_grid=grid, mode=mode, feather=feather, nodata=NODATA))
        res["mosaic"].append({"mode": mode, "feather": feather, "layers": 4, "overlap": a.overlap, "native_ms": ms, "composite_ms": cms,
                              "composite_over_native": cms["median"] / ms["median"],
                              "condition_native_not_slower": bool(ms["median"] <= cms["median"]),
                              "equal_bits": bool(torch.equal(out.view(torch.int32), want.view(torch.int32))),
                              "dsm_mosaic_api_ms": api, "cells_per_s": gw * gh / (1e-3 * ms["median"])})
    res["condition_dist_not_slower_than_scipy"] = all(r.get("condition_native_not_slower") is True for r in res["dist"]) if edt2 is not None else "not measured"
    res["condition_mosaic_not_slower_than_composite"] = all(r["condition_native_not_slower"] for r in res["mosaic"])
    res["condition_mosaic_equals_composite"] = all(r["equal_bits"] for r in res["mosaic"])
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
