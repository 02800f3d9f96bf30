#!/usr/bin/env python
"""DSM rendering timing on one MI355X ("Rendering a DSM into a view").

Workload: three synthetic 5120 x 5120 views (rpc_synth.make_view_rpcs, GSD 2.1 m, tilts for 0 and +-0.4 m of ground shift per
metre of height) over a 5 m DSM covering their footprints: smooth terrain plus 20 - 60 m blocks.  Each view is rendered by
smvs_rpc_dsm_render; device events time --reps repetitions per view after --warmup: min / median / max ms per view.  Also
reported: the mean number of evaluations per pixel K + 1 + B (computed on the host from the same formulas, from the G(h_lo) /
G(h_hi) of every pixel and its hit), the share of valid pixels, and the numpy oracle's time on a 256 x 256 crop of view 1 with
its agreement count.

    python tools/bench_dsm_render.py [--size 5120] [--reps 20] [--warmup 3] [--json profiles/dsm_render_bench.json]
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
from dsm_bench_common import SHIFTS, scene_dsm, stats  # noqa: E402
from satmvs_amd import dsm, rpc_synth  # noqa: E402
from satmvs_amd.transverse_mercator import whu_tlc_projection  # noqa: E402

def evals_per_pixel(heights, rpc, tm7, grid, h_lo, h_hi, tol, stride):
    """Mean K + 1 + B over a strided sample of the pixels (the kernel's formulas; invalid pixels: K + 1)."""
    import dsm_render_oracle as ro
    S = heights.shape[0]
    ys, xs = np.mgrid[stride // 2:S:stride, stride // 2:S:stride].astype(np.float64)
    e_hi, n_hi = ro.G(rpc, tm7, xs, ys, np.full(xs.shape, h_hi))
    e_lo, n_lo = ro.G(rpc, tm7, xs, ys, np.full(xs.shape, h_lo))
    K = ro.march_steps(e_hi, n_hi, e_lo, n_lo, grid.xres, grid.yres)
    step = (h_hi - h_lo) / K
    h = heights[stride // 2::stride, stride // 2::stride].astype(np.float64)
    valid = np.isfinite(h)
    k = np.where(valid, np.minimum(np.ceil((h_hi - h) / step), K), K)      # the hit sample: first h_k at or below h
    B = np.where(valid & (k > 0), ro.bisect_steps(step, tol), 0)
    return float((k + 1 + B).mean()), float(K.mean()), float(B[valid & (k > 0)].mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=5120)
    ap.add_argument("--res", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-3)
    ap.add_argument("--crop", type=int, default=256)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dsm_render needs an MI355X")
    import dsm_render_oracle as ro
    dev = torch.device("cuda:0")
    proj = whu_tlc_projection()
    tm7 = proj.tm7()
    S = a.size
    rpcs = [ro.view_rpc(S, S, s, seed=0) for s in SHIFTS]
    grid = ro.grid_over([(r, (S, S)) for r in rpcs], tm7, 100.0, 250.0, a.res, margin=50.0)
    z = scene_dsm(grid)
    h_lo, h_hi = ro.h_range(z, -999.0)
    zd = torch.from_numpy(z).to(dev)
    rds = [torch.from_numpy(r).to(dev) for r in rpcs]
    res = {"workload": "3 views %dx%d (GSD 2.1 m, shift 0 / +0.4 / -0.4 m per m) over a %.1f m DSM %dx%d, heights %.1f .. %.1f m, tol %g m"
                       % (S, S, a.res, grid.width, grid.height, h_lo, h_hi, a.tol),
           "views": []}
    for shift, r, rd in zip(SHIFTS, rpcs, rds):
        for _ in range(a.warmup):
            out = dsm.render_heights(zd, grid, rd, proj, (S, S), tol=a.tol)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = dsm.render_heights(zd, grid, rd, proj, (S, S), tol=a.tol)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        h = out.cpu().numpy()
        ev, K, B = evals_per_pixel(h, r, tm7, grid, h_lo, h_hi, a.tol, stride=max(1, S // 256))
        res["views"].append({"shift_m_per_m": shift, "ms": stats(ts), "valid_share": float(np.isfinite(h).mean()),
                             "evals_per_pixel": ev, "mean_K": K, "mean_B": B})
    allms = sorted(t for v in res["views"] for t in [v["ms"]["median"]])
    res["ms_per_view_median"] = {"min": allms[0], "median": allms[len(allms) // 2], "max": allms[-1]}
    res["evals_per_pixel"] = float(np.mean([v["evals_per_pixel"] for v in res["views"]]))
    # the numpy oracle on a crop of view 1 (the tilted one), against the same crop of the device render
    c, x0, y0 = a.crop, S // 2, S // 2
    t0 = time.perf_counter()
    o = ro.render_view(z, grid, -999.0, tm7, rpcs[1], c, c, x0, y0, tol=a.tol)
    t_np = time.perf_counter() - t0
    got = dsm.render_heights(zd, grid, rds[1], proj, (c, c), origin=(x0, y0), tol=a.tol).cpu().numpy()
    want = o["height"]
    both = np.isfinite(got) & np.isfinite(want)
    res["numpy_crop"] = {"pixels": c * c, "s": t_np, "evals_per_pixel": float(o["evals"].mean()),
                         "validity_differs": int((np.isfinite(got) != np.isfinite(want)).sum()),
                         "max_abs_diff_m": float(np.abs(got[both].astype(np.float64) - want[both]).max()) if both.any() else None,
                         "projected_s_per_view": t_np * (S * S) / (c * c)}
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
