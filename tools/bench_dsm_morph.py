#!/usr/bin/env python
"""Ground-extraction timing on one MI355X ("Ground extraction").

Workload: the grid of tools/bench_dsm_post.py (three 5120 x 5120 height maps fused into a 5 m grid, speckles and voids
seeded the same way) after despike radius 2.  Device events time --reps calls after --warmup, workspace allocated outside
the timed span: smvs_dsm_morph "open" at radius 1, 4, 16, 64, 256; smvs_dsm_ground with the default schedule at max_radius 16
and 64; dsm.extract_dtm end to end (host clock around a synchronise).  Each is held against what a user has without the
native entries, on the same device in the same run: separable torch.nn.functional.max_pool2d (kernel (1, w) then (w, 1),
stride 1, padding r, erosion by negation, invalid cells at -+inf, which is also the pool's padding value) with the
classification in torch operators; that composite's classes are also compared with the native ones.  Two conditions are
reported with their numbers: native ground_filter not slower than the composite at either max_radius, and open at radius 256
at most 2 x open at radius 4.  With --oracle the numpy oracle (tests/dsm_morph_oracle.py) is timed on the same grid and the
device result compared with it bit for bit.

    python tools/bench_dsm_morph.py [--size 5120] [--reps 20] [--warmup 3] [--oracle] [--json profiles/dsm_morph_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dsm_bench_common import scratch_sizes, stats, synth_heights, timed  # noqa: E402
from satmvs_amd import _lib, dsm, rpc_synth  # noqa: E402
from satmvs_amd.transverse_mercator import whu_tlc_projection  # noqa: E402

NODATA = -999.0
INF = float("inf")


def bench_grid(a, dev):
    """The despiked grid of bench_dsm_post's workload, a device tensor, and its DSMGrid."""
    proj = whu_tlc_projection()
    rpcs = [torch.from_numpy(r).to(dev) for r in rpc_synth.make_view_rpcs(a.views, a.size, a.size, seed=0, gsd=2.1, lat0=31.0, lon0=-134.6)]
    hs = synth_heights(a.views, a.size, dev)
    grid = dsm.grid_for(hs, rpcs, proj, a.res)
    z = dsm.heights_to_dsm(hs, rpcs, proj, grid, mode="median", nodata=NODATA)
    del hs
    gh, gw = z.shape
    g = torch.Generator(device=dev).manual_seed(1)
    ok = torch.isfinite(z) & (z != NODATA)
    u = torch.rand((gh, gw), device=dev, generator=g)
    amp = (30.0 + 50.0 * torch.rand((gh, gw), device=dev, generator=g)) * torch.where(torch.rand((gh, gw), device=dev, generator=g) < 0.5, -1.0, 1.0)
    z = torch.where(ok & (u < a.speckle), z + amp, z)
    drop = ok & (u > 1.0 - a.drop)
    z = torch.where(drop & (amp > 0), torch.full_like(z, float("nan")), torch.where(drop, torch.full_like(z, NODATA), z)).contiguous()
    return dsm.despike(z, radius=2), grid


# ---- the composite a user has without the native entries ------------------------------------------------------------------------
def pool_max(x, r):
    """Window maximum of a (gh, gw) tensor whose cells without a value hold -inf: rows, then columns."""
    x = F.max_pool2d(x[None, None], (1, 2 * r + 1), stride=1, padding=(0, r))
    return F.max_pool2d(x, (2 * r + 1, 1), stride=1, padding=(r, 0))[0, 0]


def pool_open(s, r):
    """s: +inf where there is no value (the erosion's identity) -> the opening, -inf where it has no value."""
    eroded = -pool_max(-s, r)                                              # +inf where the window is empty
    return pool_max(torch.where(eroded == INF, torch.full_like(eroded, -INF), eroded), r)


def pool_ground(z, radii, thresholds):
    ok = torch.isfinite(z) & (z != NODATA)
    s = torch.where(ok, z, torch.full_like(z, INF))
    cls = ok.to(torch.uint8)
    for k, (r, t) in enumerate(zip(radii, thresholds)):
        o = pool_open(s, r)
        far = ok & (cls == 1) & ((s.double() - o.double()) > t)
        cls = torch.where(far, torch.full_like(cls, 2 + k), cls)
        s = torch.where(ok, o, torch.full_like(o, INF))
    return torch.where(cls >= 2, torch.full_like(z, NODATA), z), cls


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
        sys.exit("bench_dsm_morph needs an MI355X")
    dev = torch.device("cuda:0")
    z, grid = bench_grid(a, dev)
    gh, gw = z.shape
    stream = _lib.current_stream(dev)
    out = torch.empty_like(z)
    cls = torch.empty((gh, gw), dtype=torch.uint8, device=dev)
    nbytes = _lib.load().smvs_dsm_morph_workspace_bytes(gw, gh, 256)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ok = torch.isfinite(z) & (z != NODATA)
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "bench_dsm_post's grid (%d x %dx%d maps, %.1f m cells, %dx%d) after despike radius 2, void share %.4f"
                       % (a.views, a.size, a.size, a.res, gw, gh, float((~ok).double().mean())),
           "cells": gw * gh, "workspace_bytes": nbytes, "scratch_bytes": scratch_sizes(r"dsm_morph"), "open": [], "ground": []}

    def native_open(r):
        _lib.call("smvs_dsm_morph", _lib.ptr(z), gw, gh, NODATA, r, 2, _lib.ptr(out), _lib.ptr(ws), nbytes, stream)

    s_inf = torch.where(ok, z, torch.full_like(z, INF))
    for r in (1, 4, 16, 64, 256):
        ms = timed(lambda: native_open(r), a.reps, a.warmup)
        row = {"radius": r, "native_ms": ms}
        if r <= 64:                                                        # the pool walks its window: 513 cells are not worth the GPU time
            row["torch_ms"] = timed(lambda: pool_open(s_inf, r), a.reps, a.warmup)
            want = pool_open(s_inf, r)
            row["equal_values_at_valid_cells"] = bool(torch.equal(out[ok], want[ok]))
        else:
            row["torch_ms"] = "not measured"
        res["open"].append(row)
    by_r = {row["radius"]: row["native_ms"]["median"] for row in res["open"]}
    res["open_256_over_open_4"] = by_r[256] / by_r[4]
    res["condition_open_256_at_most_2x_open_4"] = bool(by_r[256] <= 2.0 * by_r[4])

    for max_radius in (16, 64):
        radii, thresholds = dsm.ground_schedule(a.res, max_radius)
        r_arr, t_arr = np.asarray(radii, np.int32), np.asarray(thresholds, np.float64)

        def native_ground():
            _lib.call("smvs_dsm_ground", _lib.ptr(z), gw, gh, NODATA, r_arr.ctypes.data_as(dsm.ctypes.c_void_p),
                      t_arr.ctypes.data_as(dsm.ctypes.c_void_p), len(radii), _lib.ptr(out), _lib.ptr(cls), _lib.ptr(ws), nbytes, stream)

        ms = timed(native_ground, a.reps, a.warmup)
        tms = timed(lambda: pool_ground(z, radii, thresholds), a.reps, a.warmup)
        want_dtm, want_cls = pool_ground(z, radii, thresholds)
        res["ground"].append({"max_radius": max_radius, "levels": len(radii), "launches": 4 * len(radii), "native_ms": ms, "torch_ms": tms,
                              "equal_classes": bool(torch.equal(cls, want_cls)), "removed": int((cls >= 2).sum()),
                              "ground": int((cls == 1).sum()), "condition_native_not_slower": bool(ms["median"] <= tms["median"])})
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dsm.extract_dtm(z, grid, NODATA)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    res["extract_dtm_api_ms"] = stats(ts)
    if a.oracle:
        import dsm_morph_oracle as mo
        zn = z.cpu().numpy()
        orc = {}
        for max_radius in (16, 64):
            radii, thresholds = mo.schedule(a.res, max_radius)
            t0 = time.perf_counter()
            want, wcls = mo.ground(zn, radii, thresholds, NODATA)
            orc["ground_%d_s" % max_radius] = time.perf_counter() - t0
            got, gcls = dsm.ground_filter(z, a.res, NODATA, max_radius, return_class=True)
            orc["ground_%d_equal_bits" % max_radius] = bool(mo.same_bits(want, got.cpu().numpy()) and np.array_equal(wcls, gcls.cpu().numpy()))
        t0 = time.perf_counter()
        want = mo.morph(zn, 256, "open", NODATA)
        orc["open_256_s"] = time.perf_counter() - t0
        orc["open_256_equal_bits"] = bool(mo.same_bits(want, dsm.morph(z, 256, "open", NODATA).cpu().numpy()))
        res["numpy_oracle"] = orc
    else:
        res["numpy_oracle"] = "not measured"
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
