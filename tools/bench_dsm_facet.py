#!/usr/bin/env python
"""Facet timing on one MI355X ("Facets").

Workload: the grid of tools/bench_dsm_label.py (bench_dsm_morph's grid, 2199 x 2158 at the default size, after despike radius 2),
its DTM and nDSM.  The grid carries about a metre of height noise, so it is segmented twice: at the defaults (tol 0.25 m,
slope_tol 0.1: few cells are planar) and at tol 2 m, slope_tol 0.4 (most are).  Device events time --reps calls after --warmup,
workspace and outputs allocated outside the timed span: smvs_dsm_facet_normals; smvs_dsm_facet_label with growth on and off, on the
whole DSM and under the nDSM mask; smvs_dsm_facet_planes on the grown labels.  Beside them in the same process: smvs_dsm_label on
the nDSM mask and smvs_dsm_label_stats on its labels (the ratio facet_label / label is reported), dsm.facets and
dsm.extract_roofs end to end (host clock around a synchronise), and the numpy oracle (tests/dsm_facet_oracle.py) on a --crop
square, which with --oracle is also compared with the device for equality.

    python tools/bench_dsm_facet.py [--size 5120] [--reps 20] [--warmup 3] [--crop 512] [--oracle] [--json profiles/dsm_facet_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_dsm_morph import NODATA, bench_grid  # noqa: E402
from dsm_bench_common import scratch_sizes, stats, timed  # noqa: E402
from satmvs_amd import _lib, dsm  # noqa: E402

MIN_HEIGHT = 2.5
SETTINGS = (("default", 0.25, 0.1), ("loose", 2.0, 0.4))


def host_clock(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return stats(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=5120)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--res", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--speckle", type=float, default=0.01)
    ap.add_argument("--drop", type=float, default=0.05)
    ap.add_argument("--crop", type=int, default=512)
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dsm_facet needs an MI355X")
    import dsm_facet_oracle as fo
    dev = torch.device("cuda:0")
    z, grid = bench_grid(a, dev)
    gh, gw = z.shape
    above = dsm.ndsm(z, dsm.extract_dtm(z, grid, NODATA), NODATA)
    high = (torch.isfinite(above) & (above != NODATA) & (above > MIN_HEIGHT)).to(torch.uint8).contiguous()
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    nbytes = lib.smvs_dsm_facet_workspace_bytes(gw, gh)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    labels = torch.empty((gh, gw), dtype=torch.int32, device=dev)
    n_dev = torch.empty(1, dtype=torch.int32, device=dev)
    Gx, Gy = torch.empty_like(labels), torch.empty_like(labels)
    planar = torch.empty((gh, gw), dtype=torch.uint8, device=dev)
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "bench_dsm_morph's grid (%dx%d, %.1f m cells) after despike; the nDSM mask is above %.1f m" % (gw, gh, a.res, MIN_HEIGHT),
           "cells": gw * gh, "mask_cells": int(high.sum()), "workspace_bytes": nbytes, "scratch_bytes": scratch_sizes(r"dsm_facet_"), "settings": [],
           "kernel_traces": "not measured", "counters": "not measured", "real_dsms": "not measured"}

    def facet_label(mask, T, Ax, Ay, grow):
        _lib.call("smvs_dsm_facet_label", _lib.ptr(z), _lib.ptr(mask) if mask is not None else None, gw, gh, NODATA, T, Ax, Ay, 8, grow,
                  _lib.ptr(labels), _lib.ptr(n_dev), _lib.ptr(ws), nbytes, stream)

    # the objects' labelling on the nDSM mask, in the same process
    lws_bytes = lib.smvs_dsm_label_workspace_bytes(gw, gh)
    lws = torch.empty(lws_bytes, dtype=torch.uint8, device=dev)
    label_ms = timed(lambda: _lib.call("smvs_dsm_label", _lib.ptr(high), gw, gh, 8, _lib.ptr(labels), _lib.ptr(n_dev), _lib.ptr(lws), lws_bytes, stream),
                     a.reps, a.warmup)
    n_obj = int(n_dev.item())
    out = [torch.empty(n_obj * k, dtype=dt, device=dev) for dt, k in ((torch.int32, 1), (torch.int32, 4), (torch.int64, 2), (torch.int32, 1),
                                                                          (torch.float32, 1), (torch.float32, 1), (torch.int64, 1))]
    stats_ms = timed(lambda: _lib.call("smvs_dsm_label_stats", _lib.ptr(labels), _lib.ptr(above), gw, gh, NODATA, n_obj, *[_lib.ptr(t) for t in out], stream),
                     a.reps, a.warmup)
    res["label_on_the_mask"] = {"n": n_obj, "label_ms": label_ms, "stats_ms": stats_ms}
    del out, lws
    for name, tol, slope_tol in SETTINGS:
        T, Ax, Ay = dsm.facet_terms(grid, tol, slope_tol)
        row = {"setting": name, "tol": tol, "slope_tol": slope_tol, "T": T, "Ax": Ax, "Ay": Ay}
        row["normals_ms"] = timed(lambda: _lib.call("smvs_dsm_facet_normals", _lib.ptr(z), None, gw, gh, NODATA, T, _lib.ptr(Gx), _lib.ptr(Gy),
                                                    _lib.ptr(planar), stream), a.reps, a.warmup)
        row["planar_cells"] = int(planar.sum())
        for key, mask, grow in (("label_ms", None, 0), ("label_grow_ms", None, 1), ("label_masked_ms", high, 0), ("label_masked_grow_ms", high, 1)):
            row[key] = timed(lambda: facet_label(mask, T, Ax, Ay, grow), a.reps, a.warmup)
            row[key.replace("_ms", "_n")] = int(n_dev.item())
            row[key.replace("_ms", "_labelled")] = int((labels > 0).sum())
        row["masked_facet_label_over_label"] = row["label_masked_ms"]["median"] / label_ms["median"]
        facet_label(None, T, Ax, Ay, 1)
        n = int(n_dev.item())
        if gw * gh < dsm.MAX_FACET_PLANE_CELLS:
            bufs = [torch.empty(n * k, dtype=dt, device=dev) for dt, k in ((torch.int64, 4), (torch.int32, 3), (torch.int64, 8), (torch.float64, 3),
                                                                             (torch.int64, 1), (torch.int32, 1))]
            row["planes_ms"] = timed(lambda: _lib.call("smvs_dsm_facet_planes", _lib.ptr(labels), _lib.ptr(z), gw, gh, NODATA, n,
                                                       *[_lib.ptr(t) for t in bufs], stream), a.reps, a.warmup)
            row["largest_facet_cells"] = int(bufs[0].reshape(n, 4)[:, 0].max()) if n else 0
            del bufs
        else:
            row["planes_ms"] = "not measured (2^24 cells or more)"
        row["facets_api_ms"], (_, row["facets_api_n"]) = host_clock(lambda: dsm.facets(z, grid, tol, slope_tol, nodata=NODATA), 5)
        if gw * gh < dsm.MAX_FACET_PLANE_CELLS:
            row["extract_roofs_api_ms"], (_, table) = host_clock(lambda: dsm.extract_roofs(z, above, grid, MIN_HEIGHT, tol=tol, slope_tol=slope_tol, nodata=NODATA), 5)
            row["extract_roofs_kept"] = int(table["n_cells"].numel())
        else:
            row["extract_roofs_api_ms"] = "not measured (2^24 cells or more)"
        k = min(a.crop, gh, gw)
        crop = z[:k, :k].contiguous()
        zc = crop.cpu().numpy()
        t0 = time.perf_counter()
        want, nw = fo.facets(zc, T, Ax, Ay, nodata=np.float32(NODATA))
        row["oracle_crop_ms"] = 1e3 * (time.perf_counter() - t0)
        row["oracle_crop_cells"] = k * k
        row["oracle_statement"] = "graph (scipy)" if fo.HAVE_SCIPY else "graph (numpy propagation)"
        if a.oracle:
            got, n_got = dsm.facets(crop, dsm.DSMGrid(grid.e0, grid.n0, grid.xres, grid.yres, k, k), tol, slope_tol, nodata=NODATA)
            row["equal"] = bool(n_got == nw and fo.differing(got.cpu().numpy(), want) is None)
        else:
            row["equal"] = "not measured"
        res["settings"].append(row)
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
