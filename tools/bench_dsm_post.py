#!/usr/bin/env python
"""DSM clean-up timing on one MI355X ("Cleaning a DSM").

Workload: the DSM that tools/bench_dsm.py's workload produces (three 5120 x 5120 height maps fused into a 5 m grid, median
mode, with the voids fusion leaves: 1 % holes per map and the wedges of the grid's bounding box that no view covers), plus
seeded speckles: --speckle of the valid cells moved by +-30 .. 80 m, and --drop of them voided (NaN and nodata mixed) so that
there is something to fill inside the footprint too.  Device events time --reps calls of smvs_dsm_despike (radius 1, 2, 3) and
smvs_dsm_fill (max_steps 16 with the three methods, max_steps 256 with "idw"; workspace allocated outside the timed span)
after --warmup: min / median / max in ms.  Also reported: the void share before and after each operation, the cells removed,
the scratch (private segment) size of every kernel read from the built library, and, with --oracle, the time of the numpy
oracle (tests/dsm_post_oracle.py) on the same grid and whether the device result equals it bit for bit.

    python tools/bench_dsm_post.py [--size 5120] [--reps 20] [--warmup 3] [--oracle] [--json profiles/dsm_post_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dsm_bench_common import scratch_sizes, stats, synth_heights, timed  # noqa: E402
from satmvs_amd import _lib, dsm, rpc_synth  # noqa: E402
from satmvs_amd.transverse_mercator import whu_tlc_projection  # noqa: E402

NODATA = -999.0


def void_share(z):
    return float((~(torch.isfinite(z) & (z != NODATA))).double().mean())


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
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dsm_post needs an MI355X")
    dev = torch.device("cuda:0")
    proj = whu_tlc_projection()
    rpcs = [torch.from_numpy(r).to(dev) for r in rpc_synth.make_view_rpcs(a.views, a.size, a.size, seed=0, gsd=2.1, lat0=31.0, lon0=-134.6)]
    hs = synth_heights(a.views, a.size, dev)
    grid = dsm.grid_for(hs, rpcs, proj, a.res)
    z = dsm.heights_to_dsm(hs, rpcs, proj, grid, mode="median", nodata=NODATA)
    del hs
    gh, gw = z.shape
    void_fused = void_share(z)
    g = torch.Generator(device=dev).manual_seed(1)
    ok = torch.isfinite(z) & (z != NODATA)
    u = torch.rand((gh, gw), device=dev, generator=g)
    amp = (30.0 + 50.0 * torch.rand((gh, gw), device=dev, generator=g)) * torch.where(torch.rand((gh, gw), device=dev, generator=g) < 0.5, -1.0, 1.0)
    z = torch.where(ok & (u < a.speckle), z + amp, z)
    drop = ok & (u > 1.0 - a.drop)
    z = torch.where(drop & (amp > 0), torch.full_like(z, float("nan")), torch.where(drop, torch.full_like(z, NODATA), z)).contiguous()
    stream = _lib.current_stream(dev)
    out = torch.empty_like(z)
    flags = torch.empty((gh, gw), dtype=torch.uint8, device=dev)
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "%d x %dx%d height maps (GSD 2.1 m) fused into a %.1f m grid %dx%d (median); %.3g of the valid cells moved by "
                       "+-30..80 m, %.3g voided" % (a.views, a.size, a.size, a.res, gw, gh, a.speckle, a.drop),
           "cells": gw * gh, "void_share_fused": void_fused, "void_share_input": void_share(z), "scratch_bytes": scratch_sizes(r"^dsm_(despike|fill)"),
           "despike": [], "fill": []}

    def despike(radius):
        _lib.call("smvs_dsm_despike", _lib.ptr(z), gw, gh, NODATA, radius, 10.0, 3, _lib.ptr(out), _lib.ptr(flags), stream)

    for radius in (1, 2, 3):
        ms = timed(lambda: despike(radius), a.reps, a.warmup)
        res["despike"].append({"radius": radius, "thresh": 10.0, "min_valid": 3, "ms": ms, "removed": int(flags.sum()),
                               "void_share_after": void_share(out)})
    despike(2)
    clean = out.clone()                                                        # the fill's input: the radius 2 result
    res["fill_input"] = "despike radius 2, void share %.6f" % void_share(clean)

    def fill(max_steps, method, ws):
        _lib.call("smvs_dsm_fill", _lib.ptr(clean), gw, gh, NODATA, max_steps, 3, dsm.FILL_METHODS[method], _lib.ptr(out),
                  _lib.ptr(flags), _lib.ptr(ws), ws.numel(), stream)

    for max_steps, method in ((16, "idw"), (16, "nearest"), (16, "min"), (256, "idw")):
        ws = torch.empty(_lib.load().smvs_dsm_fill_workspace_bytes(gw, gh, max_steps), dtype=torch.uint8, device=dev)
        ms = timed(lambda: fill(max_steps, method, ws), a.reps, a.warmup)
        res["fill"].append({"max_steps": max_steps, "min_hits": 3, "method": method, "ms": ms, "workspace_bytes": ws.numel(),
                            "filled": int(((flags >= 3) & (flags != 255)).sum()), "void_share_after": void_share(out)})
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dsm.fill_voids(dsm.despike(z, radius=2), max_steps=16)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    res["despike_fill_api_ms"] = stats(ts)
    if a.oracle:
        import dsm_post_oracle as po
        zn, cn = z.cpu().numpy(), clean.cpu().numpy()
        orc = {}
        t0 = time.perf_counter()
        want, _ = po.despike(zn, NODATA, radius=2, thresh=10.0, min_valid=3)
        orc["despike_radius_2_s"] = time.perf_counter() - t0
        orc["despike_radius_2_equal_bits"] = bool(po.same_bits(want, cn))
        for max_steps in (16, 256):
            t0 = time.perf_counter()
            want, _ = po.fill(cn, NODATA, max_steps=max_steps, min_hits=3, method="idw")
            orc["fill_idw_%d_s" % max_steps] = time.perf_counter() - t0
            got = dsm.fill_voids(clean, NODATA, max_steps=max_steps, min_hits=3, method="idw").cpu().numpy()
            orc["fill_idw_%d_equal_bits" % max_steps] = bool(po.same_bits(want, got))
        res["numpy_oracle"] = orc
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
