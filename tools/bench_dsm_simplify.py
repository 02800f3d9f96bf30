#!/usr/bin/env python
"""Timing of the simplified outlines on one MI355X ("Simplified outlines").

Workload: the grid of tools/bench_dsm_outline.py (bench_dsm_morph's grid, extract_dtm, ndsm), the nDSM mask (valid and above
2.5 m) labelled under connectivity 8 and outlined.  Host clock around a synchronise, --reps calls after --warmup, allocation
and the reads of the device's words included: dsm.outlines and dsm.burn_rings as the yardsticks in the same process, then
dsm.simplify_outlines at 0.5, 1 and 2 cells and dsm.burn_polygons of each result, all on device tensors.  Device events time
one batch of rounds of the native entry by itself (smvs_dsm_simplify_begin before every batch, outside the timed span), which
gives the time per round.  What a user has without the native entries is the rings copied to the host and the recursion in
Python: the oracle's first statement (tests/dsm_simplify_oracle.py), one run, host clock, on the --host-rings largest rings
(all of them with --host-rings 0); its kept vertices are compared with the device's.

    python tools/bench_dsm_simplify.py [--size 5120] [--reps 10] [--warmup 2] [--host-rings 200] [--json profiles/dsm_simplify_bench.json]
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
from bench_dsm_outline import MIN_HEIGHT, host_clock  # noqa: E402
from dsm_bench_common import scratch_sizes, timed  # noqa: E402
from satmvs_amd import _lib, dsm  # noqa: E402

TOLERANCES = (0.5, 1.0, 2.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=5120)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--res", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--speckle", type=float, default=0.01)
    ap.add_argument("--drop", type=float, default=0.05)
    ap.add_argument("--host-rings", type=int, default=200)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dsm_simplify needs an MI355X")
    dev = torch.device("cuda:0")
    z, grid = bench_grid(a, dev)
    gh, gw = z.shape
    above = dsm.ndsm(z, dsm.extract_dtm(z, grid, NODATA), NODATA)
    mask = torch.isfinite(above) & (above != NODATA) & (above > MIN_HEIGHT)
    labels, n = dsm.label(mask, 8)
    n = int(n)
    for _ in range(a.warmup):
        rings = dsm.outlines(labels, n)
    outlines_ms, rings = host_clock(lambda: dsm.outlines(labels, n), a.reps)
    burn_rings_ms, back = host_clock(lambda: dsm.burn_rings(rings["vertices"], rings["offset"], rings["label"], (gh, gw)), a.reps)
    nr, nv = int(rings["label"].numel()), int(rings["vertices"].shape[0])
    sizes = (rings["offset"][1:] - rings["offset"][:-1])
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "bench_dsm_outline's grid (%dx%d, %.1f m cells): nDSM mask above %.1f m, connectivity 8, outlined" % (gw, gh, a.res, MIN_HEIGHT),
           "cells": gw * gh, "n": n, "n_rings": nr, "n_vertices_in": nv, "longest_ring": int(sizes.max().item()) if nr else 0,
           "scratch_bytes": scratch_sizes(r"sp_"), "outlines_api_ms": outlines_ms, "burn_rings_api_ms": burn_rings_ms,
           "burn_rings_round_trip_equal": bool(torch.equal(back, torch.where((labels >= 1) & (labels <= n), labels, torch.zeros_like(labels)))),
           "tolerances": [], "kernel_traces": "not measured", "counters": "not measured", "real_dsms": "not measured"}
    lib = _lib.load()
    stream, p = _lib.current_stream(dev), _lib.ptr
    nbytes = lib.smvs_dsm_simplify_workspace_bytes(nr, nv)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    word = torch.empty(2, dtype=torch.int32, device=dev)
    res["workspace_bytes"] = nbytes
    import dsm_simplify_oracle as so
    host = {k: t.cpu().numpy() for k, t in rings.items()}
    order = np.argsort(-np.diff(host["offset"]), kind="stable")
    chosen = np.sort(order[:a.host_rings] if a.host_rings else order)
    lists = so.ring_lists(host)
    for tol in TOLERANCES:
        tol16 = int(16 * tol)
        for _ in range(a.warmup):
            dsm.simplify_outlines(rings, tol)
        api_ms, got = host_clock(lambda: dsm.simplify_outlines(rings, tol), a.reps)
        burn_ms, burnt = host_clock(lambda: dsm.burn_polygons(got["vertices"], got["offset"], got["label"], (gh, gw)), a.reps)
        rounds = got["rounds"]

        def batch():
            _lib.call("smvs_dsm_simplify_rounds", p(rings["vertices"]), p(rings["offset"]), nr, nv, tol16, rounds, p(word), p(ws), nbytes, stream)

        def begin():
            _lib.call("smvs_dsm_simplify_begin", p(rings["vertices"]), p(rings["offset"]), nr, nv, p(word), p(ws), nbytes, stream)

        rounds_ms = timed(batch, a.reps, a.warmup, reset=begin)["median"]
        t0 = time.perf_counter()
        kept_host = [so._fallback(lists[r], so.simplify_ring(lists[r], tol16))[0] for r in chosen.tolist()]
        host_ms = 1e3 * (time.perf_counter() - t0)
        kept_dev, off_out = got["kept"].cpu().numpy(), got["offset"].cpu().numpy()
        equal = all((kept_dev[off_out[r]:off_out[r + 1]] - host["offset"][r]).tolist() == k for r, k in zip(chosen.tolist(), kept_host))
        res["tolerances"].append({"tol_cells": tol, "tol16": tol16, "n_vertices_out": int(got["vertices"].shape[0]), "rounds": rounds,
                                  "rings_simplified": int(got["simplified"].sum().item()), "simplify_api_ms": api_ms, "burn_polygons_api_ms": burn_ms,
                                  "rounds_native_ms": rounds_ms, "ms_per_round": rounds_ms / max(rounds, 1),
                                  "simplify_over_outlines": api_ms["median"] / outlines_ms["median"],
                                  "burn_polygons_over_burn_rings": burn_ms["median"] / burn_rings_ms["median"],
                                  "cells_changed_by_burn": int((burnt != back).sum().item()),
                                  "host_recursion_rings": int(len(chosen)), "host_recursion_vertices": int(sum(len(lists[r]) for r in chosen.tolist())),
                                  "host_recursion_ms": host_ms, "host_equals_device": bool(equal)})
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
