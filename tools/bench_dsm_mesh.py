#!/usr/bin/env python
"""Mesh timing on one MI355X ("Meshes").

Workload: the grid of tools/bench_dsm_label.py (bench_dsm_morph's grid, 2199 x 2158 at the default size), as the DSM itself and
as its DTM (dsm.extract_dtm), at tol 0.25, 0.5, 1 and 2 m and tile 64, 256 and 1024.  Per surface and tile: smvs_dsm_mesh_errors
(device events).  Per surface, tile and tolerance: smvs_dsm_mesh_count, smvs_dsm_mesh_write and smvs_dsm_mesh_heights on their own
(device events), dsm.mesh() end to end with the error map given and without (host clock around a synchronise: the call reads
the device's counts), and the triangle and vertex counts against the full resolution 2 (gh - 1) (gw - 1).  Beside them in the
same process, as yardsticks: dsm.outlines of the objects and dsm.contours of the DTM at 2.5 m.  And the oracle's array statement
on the host over a crop of --host-side cells a side (numpy: a statement of the rule, not a competitor), every output asserted
equal to the device's on that crop.

    python tools/bench_dsm_mesh.py [--size 5120] [--reps 10] [--warmup 2] [--no-host] [--json profiles/dsm_mesh_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_dsm_morph import NODATA, bench_grid  # noqa: E402
from bench_dsm_outline import host_clock  # noqa: E402
from dsm_bench_common import timed  # noqa: E402
from satmvs_amd import _lib, dsm  # noqa: E402

TOLS = (0.25, 0.5, 1.0, 2.0)
TILES = (64, 256, 1024)


def kernel_resources():
    """{kernel: {vgpr, lds, scratch}} of the mesh kernels, from the code objects inside the built library (tools/kernel_regs.py)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), _lib.LIB_PATH], capture_output=True, text=True).stdout
    table = {}
    for line in out.splitlines()[1:]:
        f = line.split()
        if len(f) >= 8 and f[0].startswith(("me_", "mc_", "mw_", "mh_")):
            table[" ".join(f[:-7])] = {"vgpr": int(f[-7]), "lds": int(f[-4]), "scratch": int(f[-3])}
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=5120)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--res", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--speckle", type=float, default=0.01)
    ap.add_argument("--drop", type=float, default=0.05)
    ap.add_argument("--host-side", type=int, default=768, help="side of the crop the array statement runs on")
    ap.add_argument("--no-host", action="store_true", help="leave the array statement out")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dsm_mesh needs an MI355X")
    dev = torch.device("cuda:0")
    z, grid = bench_grid(a, dev)
    z = z.contiguous()
    gh, gw = z.shape
    dtm = dsm.extract_dtm(z, grid, NODATA).contiguous()
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    p = _lib.ptr
    full = 2 * (gh - 1) * (gw - 1)
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "bench_dsm_label's grid (%dx%d, %.1f m cells) and its DTM" % (gw, gh, a.res), "cells": gh * gw,
           "full_resolution_triangles": full, "kernel_resources": kernel_resources(),
           "workspace_bytes": lib.smvs_dsm_mesh_workspace_bytes(gw, gh, 256), "errors": [], "cases": [],
           "kernel_traces": "not measured", "real_dsms": "not measured"}
    errors = torch.empty((gh, gw), dtype=torch.int64, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    heights = torch.empty((gh, gw), dtype=torch.float32, device=dev)
    nbytes = lib.smvs_dsm_mesh_workspace_bytes(gw, gh, 256)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    for sname, surface in (("dsm", z), ("dtm", dtm)):
        for tile in TILES:
            e_ms = timed(lambda: _lib.call("smvs_dsm_mesh_errors", p(surface), gw, gh, NODATA, tile, p(errors), stream), a.reps, a.warmup)
            torch.cuda.synchronize()
            res["errors"].append({"surface": sname, "tile": tile, "errors_ms": e_ms, "infinite_vertices": int((errors == dsm.MESH_INF).sum().item())})
            for tol in TOLS:
                thr = int(np.floor(256.0 * tol)) * tile
                count = lambda: _lib.call("smvs_dsm_mesh_count", p(errors), p(surface), gw, gh, NODATA, tile, thr, p(counts), p(ws), nbytes, stream)  # noqa: E731
                c_ms = timed(count, a.reps, a.warmup)
                torch.cuda.synchronize()
                nt, nv = counts.tolist()
                tri = torch.empty((nt, 3), dtype=torch.int32, device=dev)
                lev = torch.empty(nt, dtype=torch.uint8, device=dev)
                ver = torch.empty((nv, 2), dtype=torch.int32, device=dev)
                zz = torch.empty(nv, dtype=torch.float32, device=dev)
                w_ms = timed(lambda: _lib.call("smvs_dsm_mesh_write", p(surface), gw, gh, tile, nt, nv, p(tri), p(lev), p(ver), p(zz), p(status), p(ws), nbytes,
                                               stream), a.reps, a.warmup)
                h_ms = timed(lambda: _lib.call("smvs_dsm_mesh_heights", p(errors), p(surface), gw, gh, NODATA, tile, thr, p(heights), None, p(ws), nbytes,
                                               stream), a.reps, a.warmup)
                lod_ms, m = host_clock(lambda: dsm.mesh(surface, grid, tol=tol, tile=tile, nodata=NODATA, errors=errors), 3)
                api_ms, _ = host_clock(lambda: dsm.mesh(surface, grid, tol=tol, tile=tile, nodata=NODATA), 3)
                assert m["n_triangles"] == nt and int(status.item()) == nt
                res["cases"].append({"surface": sname, "tile": tile, "tol_m": tol, "count_ms": c_ms, "write_ms": w_ms, "heights_ms": h_ms,
                                     "mesh_api_with_errors_ms": lod_ms, "mesh_api_ms": api_ms, "triangles": nt, "vertices": nv,
                                     "triangles_of_full_resolution": nt / full, "covered_vertices": int((heights != NODATA).sum().item())})
    # yardsticks in the same process: the vector tools over the same grid
    labels, stats = dsm.extract_objects(dsm.ndsm(z, dtm, NODATA), grid, nodata=NODATA)
    n_labels = int(stats["area"].numel())
    res["outlines_api_ms"], rings = host_clock(lambda: dsm.outlines(labels, n_labels, grid), 3)
    res["outline_vertices"] = int(rings["vertices"].shape[0])
    res["contours_2p5m_api_ms"], lines = host_clock(lambda: dsm.contours(dtm, interval=2.5, grid=grid, nodata=NODATA), 3)
    res["contour_vertices"] = int(lines["vertices"].shape[0])
    if a.no_host:
        res["array_statement_host"] = "not measured"
    else:
        import dsm_mesh_oracle as mo
        side = min(a.host_side, gh, gw)
        crop = np.ascontiguousarray(z[:side, :side].cpu().numpy())
        t0 = time.perf_counter()
        want_e = mo.errors_arrays(crop, 256, NODATA)
        want = mo.mesh_arrays(want_e, crop, 256, 0.5, NODATA)
        want_h, want_d = mo.heights_arrays(want_e, crop, 256, 0.5, NODATA)
        host_ms = 1e3 * (time.perf_counter() - t0)

        def native():
            e = dsm.mesh_errors(crop, 256, NODATA)
            return e, dsm.mesh(crop, tol=0.5, tile=256, nodata=NODATA, errors=e), dsm.mesh_heights(crop, 0.5, 256, NODATA, errors=e, return_dev=True)
        crop_ms, (got_e, got, (got_h, got_d)) = host_clock(native, 3)
        equal = bool(np.array_equal(got_e, want_e) and mo.differing(got, want) == [] and np.array_equal(got_h.view(np.uint32), want_h.view(np.uint32))
                     and np.array_equal(got_d, want_d))
        assert equal, "the array statement and the device disagree"
        res["array_statement_host"] = {"ms": host_ms, "cells": side * side, "tile": 256, "tol_m": 0.5, "triangles": int(len(want["triangles"])),
                                       "native_api_ms": crop_ms, "equal": equal}
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
