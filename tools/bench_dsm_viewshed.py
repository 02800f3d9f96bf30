#!/usr/bin/env python
"""Viewsheds and lines of sight, timed on one MI355X ("Viewshed").

Workload: the grid of tools/bench_dsm_horizon.py (bench_dsm_morph's grid after despike radius 2).  Device events time --reps
calls after --warmup, workspace and outputs allocated outside the timed span.
smvs_dsm_viewshed (the quantise and the walk of one call) for an observer in the centre and one in a corner, for 1, 16 and 64
observers per call (eyes 1.6 m above a lattice of valid cells), with `above` and without it, without a range and with
max_distance 1 km, and with a range so small that every target is out of it: the quantise and a walk that reads and writes
but never steps.  With --variant-lib, the same calls on a second build of the library, e.g. the other lane mapping
(python -c "from satmvs_amd import build; build.build(extra_flags=['-DVS_TILE_H=1'], out='<path>')"), with its maps held equal
in bits to the first build's.  Beside them, from the same process: dsm.viewshed end to end (host clock around a synchronise,
median of 3), smvs_dsm_los on 10^6 random pairs, one direction of smvs_dsm_horizon, and a torch composite of the same rule (a
loop over i with one gather of the whole grid per step, one observer in the centre, timed once) whose maps are asserted equal in
bits.  No time is a condition.

    python tools/bench_dsm_viewshed.py [--size 5120] [--reps 20] [--warmup 3] [--variant-lib PATH] [--json profiles/dsm_viewshed_bench.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_dsm_morph import NODATA, bench_grid  # noqa: E402
from bench_dsm_sun import host_timed  # noqa: E402
from dsm_bench_common import timed  # noqa: E402
from satmvs_amd import _lib, dsm  # noqa: E402

EYE = 410                                                     # 1.6 m in units of 2^-8 m


def scratch_sizes():
    """{kernel: private segment bytes} of the viewshed's kernels in the built library (template arguments hold spaces, which
    dsm_bench_common.scratch_sizes splits at)."""
    import re
    import subprocess
    sizes = {}
    for name in ("dsm_viewshed", "dsm_los"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), _lib.LIB_PATH, name], capture_output=True, text=True).stdout
        for line in out.splitlines()[1:]:
            hit = re.match(r"(.*?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$", line)
            if hit:
                sizes[hit.group(1)] = int(hit.group(6))
    return sizes


def composite(z, terms, obs, nodata):
    """The viewshed rule of one observer (col, row, eye, mode, tgt) with torch operators: every target at once, a loop over
    the step i with one gather of the whole grid per step -> (seen uint8, above float32)."""
    xres, yres, c256, r2max = terms
    co, ro, eye, mode, tgt = obs
    gh, gw = z.shape
    dev = z.device
    ok = torch.isfinite(z) & (z != float(np.float32(nodata))) & (z.abs() <= 32768.0)
    q = torch.where(ok, torch.round(z.double() * 256.0).long(), torch.zeros((), dtype=torch.int64, device=dev))
    stands = mode == 1 or bool(ok[ro, co])
    E = eye if mode == 1 else int(q[ro, co]) + eye
    rt, ct = torch.meshgrid(torch.arange(gh, device=dev), torch.arange(gw, device=dev), indexing="ij")
    dx, dy = ct - co, rt - ro
    rows = dy.abs() >= dx.abs()
    n, dm = torch.where(rows, dy.abs(), dx.abs()), torch.where(rows, dx, dy)
    sg = torch.where(torch.where(rows, dy, dx) < 0, -1, 1)

    def dist2(dc, dr):
        x, y = dc.double() * xres, dr.double() * yres
        return x * x + y * y

    d2 = dist2(dx, dy)
    top = q - torch.round(c256 * d2).long() + tgt - E
    best_num, best_i = torch.zeros_like(n), torch.zeros_like(n)
    qf, okf, two_n = q.flatten(), ok.flatten(), (2 * n).clamp(min=1)
    for i in range(1, int(n.max())):
        m = torch.div(2 * i * dm + n, two_n, rounding_mode="floor")
        dc, dr = torch.where(rows, m, i * sg), torch.where(rows, i * sg, m)
        at = (ro + dr).clamp(0, gh - 1) * gw + (co + dc).clamp(0, gw - 1)
        num = qf[at] - torch.round(c256 * dist2(dc, dr)).long() - E
        better = okf[at] & (n > i) & ((best_i == 0) | (num * best_i > best_num * i))
        best_num, best_i = torch.where(better, num, best_num), torch.where(better, i, best_i)
    hidden = (best_i > 0) & (best_num * n > top * best_i)
    need = -torch.div(-(best_num * n), best_i.clamp(min=1), rounding_mode="floor") - (top - tgt)
    code = torch.where(hidden, 2, 1)
    code = torch.where(d2 <= r2max, code, 3)
    code = torch.where(ok & stands, code, 0).to(torch.uint8)
    above = torch.where(code == 2, (need.double() / 256.0).float(), torch.where(code == 1, 0.0, float(np.float32(nodata))).float())
    return code, above


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=5120)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--res", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--speckle", type=float, default=0.01)
    ap.add_argument("--drop", type=float, default=0.05)
    ap.add_argument("--variant-lib", default=None, help="a second build of the library to time on the same calls")
    ap.add_argument("--variant-name", default="a wave is 64 cells of a row (-DVS_TILE_H=1)")
    ap.add_argument("--skip-composite", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dsm_viewshed needs an MI355X")
    dev = torch.device("cuda:0")
    z, grid = bench_grid(a, dev)
    gh, gw = z.shape
    cells = gw * gh
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    ok = (torch.isfinite(z) & (z != NODATA) & (z.abs() <= 32768.0)).cpu().numpy()
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "bench_dsm_morph's grid (%dx%d, %.1f m cells) after despike radius 2, void share %.4f" % (gw, gh, a.res, 1.0 - ok.mean()),
           "cells": cells, "scratch_bytes": scratch_sizes(),
           "mapping": "a wave is an 8 x 8 block of cells (the library as built)", "viewshed": [],
           "kernel_traces": "not measured", "counters": "not measured", "real_dsms": "not measured"}
    libs = [("built", lib)]
    if a.variant_lib:
        other = C.CDLL(a.variant_lib)
        other.smvs_dsm_viewshed.argtypes = _lib._SIGNATURES["smvs_dsm_viewshed"]
        other.smvs_dsm_viewshed.restype = C.c_int
        libs.append(("variant", other))
        res["variant"] = a.variant_name

    def on_valid(r, c):
        """The valid cell nearest (r, c) along its row."""
        for d in range(gw):
            for cc in (c + d, c - d):
                if 0 <= cc < gw and ok[r, cc]:
                    return r, cc
        raise ValueError("row %d holds no height" % r)

    def lattice(k):
        """k x k observers spread over the grid, each on a valid cell."""
        return [on_valid((2 * i + 1) * gh // (2 * k), (2 * j + 1) * gw // (2 * k)) for i in range(k) for j in range(k)]

    curved = dsm.viewshed_terms(grid)
    near = dsm.viewshed_terms(grid, max_distance=1000.0)
    nowhere = (curved[0], curved[1], curved[2], 1e-300)
    nbytes = lib.smvs_dsm_viewshed_workspace_bytes(gw, gh, 64)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    status = torch.empty(64, dtype=torch.int32, device=dev)

    def viewshed_row(name, where, terms, with_above):
        m = len(where)
        obs = np.ascontiguousarray(np.array([(c, r, EYE, 0, 0) for r, c in where], np.int32))
        row = {"case": name, "observers": m, "above": with_above, "max_distance_m": None if math.isinf(terms[3]) else math.sqrt(terms[3])}
        first = None
        for which, handle in libs:
            seen = torch.empty((m, gh, gw), dtype=torch.uint8, device=dev)
            above = torch.empty((m, gh, gw), dtype=torch.float32, device=dev) if with_above else None

            def call():
                rc = handle.smvs_dsm_viewshed(_lib.ptr(z), gw, gh, NODATA, terms[0], terms[1], terms[2], terms[3], obs.ctypes.data_as(C.c_void_p), m,
                                              _lib.ptr(seen), None if above is None else _lib.ptr(above), _lib.ptr(status), _lib.ptr(ws), nbytes, stream)
                assert rc == 0, rc
            ms = timed(call, a.reps, a.warmup)
            row[which] = {"ms": ms, "ms_per_observer": ms["median"] / m, "ns_per_cell_and_observer": 1e6 * ms["median"] / (m * cells)}
            if first is None:
                first = (seen, above)
                row["seen_share"] = float((seen == 1).float().mean())
                row["hidden_share"] = float((seen == 2).float().mean())
            else:
                assert torch.equal(seen, first[0]) and (above is None or torch.equal(above.view(torch.int32), first[1].view(torch.int32))), name
                row["variant_bits_equal"] = True
            del seen, above
        res["viewshed"].append(row)

    centre, corner = [on_valid(gh // 2, gw // 2)], [on_valid(0, 0)]
    for with_above in (True, False):
        viewshed_row("centre", centre, curved, with_above)
        viewshed_row("corner", corner, curved, with_above)
        viewshed_row("centre, 1 km", centre, near, with_above)
        viewshed_row("16 observers", lattice(4), curved, with_above)
        viewshed_row("64 observers", lattice(8), curved, with_above)
    viewshed_row("64 observers, 1 km", lattice(8), near, True)
    viewshed_row("centre, nothing in range: the quantise and a walk that never steps", centre, nowhere, True)
    viewshed_row("centre, flat earth", centre, dsm.viewshed_terms(grid, curvature=False), True)

    res["viewshed_api_ms"] = {"1 observer, centre": host_timed(lambda: dsm.viewshed(z, grid, centre, nodata=NODATA, return_above=True)),
                              "16 observers": host_timed(lambda: dsm.viewshed(z, grid, lattice(4), nodata=NODATA, return_above=True))}

    n_pairs = 10 ** 6
    rng = np.random.default_rng(0)
    pairs = np.stack([rng.integers(0, gw, n_pairs), rng.integers(0, gh, n_pairs), np.full(n_pairs, EYE), np.zeros(n_pairs, np.int64),
                      rng.integers(0, gw, n_pairs), rng.integers(0, gh, n_pairs), np.zeros(n_pairs, np.int64)], axis=1).astype(np.int32)
    pd = torch.from_numpy(pairs).to(dev)
    code = torch.empty(n_pairs, dtype=torch.uint8, device=dev)
    need = torch.empty(n_pairs, dtype=torch.float32, device=dev)
    res["los_1e6_pairs"] = {}
    for name, out in (("with above", need), ("without above", None)):
        ms = timed(lambda: _lib.call("smvs_dsm_los", _lib.ptr(z), gw, gh, NODATA, curved[0], curved[1], curved[2], curved[3], _lib.ptr(pd), n_pairs,
                                     _lib.ptr(code), None if out is None else _lib.ptr(out), stream), a.reps, a.warmup)
        res["los_1e6_pairs"][name] = {"ms": ms, "ns_per_pair": 1e6 * ms["median"] / n_pairs, "seen_share": float((code == 1).float().mean())}

    dirs = np.ascontiguousarray(np.array([dsm.horizon_terms(grid, 0.0)], np.float64))
    hbytes = lib.smvs_dsm_horizon_workspace_bytes(gw, gh, 1)
    hws = torch.empty(hbytes, dtype=torch.uint8, device=dev)
    tan_h = torch.empty((1, gh, gw), dtype=torch.float32, device=dev)
    res["horizon_one_direction_ms"] = timed(lambda: _lib.call("smvs_dsm_horizon", _lib.ptr(z), gw, gh, NODATA, dirs.ctypes.data_as(C.c_void_p), 1, _lib.ptr(tan_h),
                                                              _lib.ptr(hws), hbytes, stream), a.reps, a.warmup)
    del hws, tan_h

    if a.skip_composite:
        res["torch_composite"] = "not measured"
    else:
        r, c = centre[0]
        seen, above = dsm.viewshed(z, grid, centre, nodata=NODATA, return_above=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want_seen, want_above = composite(z, curved, (c, r, EYE, 0, 0), NODATA)
        torch.cuda.synchronize()
        res["torch_composite"] = {"case": "centre, with above", "ms_once": 1e3 * (time.perf_counter() - t0),
                                  "bits_equal": bool(torch.equal(seen[0], want_seen) and torch.equal(above[0].view(torch.int32), want_above.view(torch.int32)))}
        assert res["torch_composite"]["bits_equal"]
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
