#!/usr/bin/env python
"""Orthophoto timing on one MI355X ("Orthorectifying views onto the DSM").

Workload: the scene of tools/bench_dsm_render.py, three synthetic 5120 x 5120 views (GSD 2.1 m, ground shift 0 and +-0.4 m per
metre of height) over a 5 m DSM of terrain plus 20 - 60 m blocks, with RGB float32 images.  Device events time --reps calls
of smvs_rpc_ortho after --warmup: one view with occlusion at nadir and tilted, one view without occlusion, and the three-view
mosaic in nadir order (source reset to -1 before each rep, outside the timed span).  Also reported: the visibility shares per
view, the mean number of march samples K per cell that needs a march (oracle formulas on a strided sample of the cells), and
the end-to-end time of dsm.orthorectify for the mosaic (allocation, h_hi, nadir order and the three calls).

    python tools/bench_ortho.py [--size 5120] [--reps 20] [--warmup 3] [--json profiles/ortho_bench.json]
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
from dsm_bench_common import SHIFTS, scene_dsm, stats, timed  # noqa: E402
from satmvs_amd import dsm  # noqa: E402
from satmvs_amd.transverse_mercator import whu_tlc_projection  # noqa: E402


def march_samples(z, grid, tm7, rpc, h_hi, S, stride):
    """Mean K over the strided cells that march (valid, inside the view, below h_hi), from the oracle's formulas."""
    import ortho_oracle as oo
    rows, cols = np.mgrid[stride // 2:grid.height:stride, stride // 2:grid.width:stride]
    o = oo.ortho(z, grid, -999.0, tm7, rpc, shape=(S, S), rows=rows, cols=cols, h_hi=h_hi, occ_tol=0.5)
    k = o["K"][o["K"] > 0]
    return float(k.mean()) if k.size else 0.0, float(k.max()) if k.size else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=5120)
    ap.add_argument("--res", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--occ-tol", type=float, default=0.5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ortho needs an MI355X")
    import dsm_render_oracle as ro
    dev = torch.device("cuda:0")
    proj = whu_tlc_projection()
    tm7 = proj.tm7()
    S = a.size
    rpcs = [ro.view_rpc(S, S, s, seed=0) for s in SHIFTS]
    grid = ro.grid_over([(r, (S, S)) for r in rpcs], tm7, 100.0, 250.0, a.res, margin=50.0)
    z = scene_dsm(grid)
    zd = torch.from_numpy(z).to(dev)
    _, h_hi = dsm._valid_range(zd, -999.0, lower=False)
    rds = [torch.from_numpy(r).to(dev) for r in rpcs]
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    imgs = [torch.rand((S, S, 3), generator=g, device=dev, dtype=torch.float32) * 255.0 for _ in rpcs]
    gh, gw = grid.height, grid.width
    ortho = torch.empty((gh, gw, 3), dtype=torch.float32, device=dev)
    source = torch.empty((gh, gw), dtype=torch.int32, device=dev)

    def reset():
        source.fill_(-1)

    def one(v, occlusion):
        return lambda: dsm._ortho_call(zd, grid, -999.0, tm7, rds[v], imgs[v], S, S, 3, 0, 0, h_hi, occlusion, a.occ_tol, v,
                                       ortho, source, None)

    order = dsm.nadir_order(rpcs, grid, proj, h_hi)

    def mosaic():
        for v in order:
            one(v, True)()

    res = {"workload": "3 views %dx%d RGB float32 (GSD 2.1 m, shift 0 / +0.4 / -0.4 m per m) over a %.1f m DSM %dx%d, h_hi %.1f m, "
                       "occ_tol %g m" % (S, S, a.res, gw, gh, h_hi, a.occ_tol),
           "nadir_order": order, "views": []}
    for v, shift in enumerate(SHIFTS):
        st = dsm.visibility(zd, grid, rds[v], proj, (S, S), occ_tol=a.occ_tol)
        share = (torch.bincount(st.reshape(-1).long(), minlength=4).double() / st.numel()).tolist()
        K, Kmax = march_samples(z, grid, tm7, rpcs[v], h_hi, S, stride=max(1, min(gh, gw) // 64))
        res["views"].append({"shift_m_per_m": shift, "ms_occlusion": timed(one(v, True), a.reps, a.warmup, reset=reset),
                             "state_share": dict(zip(dsm.ORTHO_STATES, share)), "mean_K": K, "max_K": Kmax})
    res["views"][0]["ms_no_occlusion"] = timed(one(0, False), a.reps, a.warmup, reset=reset)
    res["views"][1]["ms_no_occlusion"] = timed(one(1, False), a.reps, a.warmup, reset=reset)
    res["mosaic_3_views_ms"] = timed(mosaic, a.reps, a.warmup, reset=reset)
    src = source.cpu().numpy()
    res["mosaic_source_share"] = {str(k): float((src == k).mean()) for k in (-1, 0, 1, 2)}
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dsm.orthorectify(imgs, rds, zd, grid, proj)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    res["orthorectify_api_ms"] = stats(ts)
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
