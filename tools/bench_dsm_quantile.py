#!/usr/bin/env python
"""Zonal order statistics timing on one MI355X ("Zonal order statistics").

Workload: the grid of tools/bench_dsm_label.py (bench_dsm_morph's grid, 2199 x 2158 at the default size, after despike radius 2),
its DTM and nDSM.  Four zone maps over it: the nDSM objects of dsm.extract_objects, the facets at tol 2 m, one zone over the whole
grid (as dsm_metrics_robust runs it), and every cell its own label on a --crop square.  For each, with the ranks of q = (0.5, 0.9)
(four slots: lo and hi of both), device events time --reps calls after --warmup, workspace and outputs allocated outside the timed
span: smvs_dsm_label_select; beside it in the same process smvs_dsm_label_stats on the same labels and values, and a torch
composite of the same rule (torch.sort of a composite int64 key (label, f2key), a gather at the ranks), whose output is asserted
equal to the native one in bits before it is timed.  dsm.label_quantiles end to end is under a host clock round a synchronise.  On
the objects the native entry is also timed alone at n_ranks 1, 2 and 8.

    python tools/bench_dsm_quantile.py [--size 5120] [--reps 20] [--warmup 3] [--crop 512] [--json profiles/dsm_quantile_bench.json]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_dsm_morph import NODATA, bench_grid  # noqa: E402
from dsm_bench_common import scratch_sizes, stats, timed  # noqa: E402
from satmvs_amd import _lib, dsm  # noqa: E402

MIN_HEIGHT = 2.5
QS = (0.5, 0.9)


def host_clock(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return stats(ts), out


def composite(labels, values, n, ranks, nodata):
    """The rule in torch: the cells that count sorted by (label, key), and a gather at the ranks -> (out (n, R) float32, m int32)."""
    lab = labels.reshape(-1).long()
    v = values.reshape(-1)
    ok = (lab >= 1) & (lab <= n) & torch.isfinite(v) & (v != nodata)
    u = v.view(torch.int32).long() & 0xffffffff
    key = torch.where((u & 0x80000000) != 0, ~u & 0xffffffff, u | 0x80000000)
    k = (lab - 1)[ok]
    s, _ = torch.sort((k << 32) | key[ok])
    m = torch.bincount(k, minlength=n)
    start = torch.cumsum(m, 0) - m
    inside = (ranks >= 0) & (ranks < m[:, None])
    at = (start[:, None] + ranks.long()).clamp(0, max(int(s.numel()) - 1, 0))
    got = (s[at] if s.numel() else torch.zeros_like(at)) & 0xffffffff
    bits = torch.where((got & 0x80000000) != 0, got & 0x7fffffff, ~got & 0xffffffff)
    f = (bits - ((bits >> 31) << 32)).to(torch.int32).view(torch.float32)
    return torch.where(inside, f, torch.full_like(f, nodata)), m.to(torch.int32)


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
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dsm_quantile needs an MI355X")
    dev = torch.device("cuda:0")
    z, grid = bench_grid(a, dev)
    gh, gw = z.shape
    above = dsm.ndsm(z, dsm.extract_dtm(z, grid, NODATA), NODATA)
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "bench_dsm_morph's grid (%dx%d, %.1f m cells) after despike, its nDSM above %.1f m; q = %s" % (gw, gh, a.res, MIN_HEIGHT, list(QS)),
           "cells": gw * gh, "scratch_bytes": scratch_sizes(r"dsm_zonal_"), "launches_per_call": 66, "zones": [],
           "wider_digits": "not built", "kernel_traces": "not measured", "counters": "not measured", "real_dsms": "not measured"}

    def select(labels, values, n, ranks, out, nv, ws, nbytes):
        _lib.call("smvs_dsm_label_select", _lib.ptr(labels), _lib.ptr(values), labels.shape[1], labels.shape[0], NODATA, n, None,
                  _lib.ptr(ranks), ranks.shape[1], _lib.ptr(out), _lib.ptr(nv), _lib.ptr(ws), nbytes, stream)

    def one_zone_map(name, labels, n, values):
        labels, values = labels.contiguous(), values.contiguous()
        h, w = labels.shape
        row = {"zones": name, "n": n, "cells": h * w, "labelled_cells": int(((labels >= 1) & (labels <= n)).sum())}
        st = [torch.empty(n * k, dtype=dt, device=dev) for dt, k in ((torch.int32, 1), (torch.int32, 4), (torch.int64, 2), (torch.int32, 1),
                                                                       (torch.float32, 1), (torch.float32, 1), (torch.int64, 1))]
        row["label_stats_ms"] = timed(lambda: _lib.call("smvs_dsm_label_stats", _lib.ptr(labels), _lib.ptr(values), w, h, NODATA, n, *[_lib.ptr(t) for t in st], stream),
                                      a.reps, a.warmup)
        m = st[3]
        row["valid_cells"] = int(m.sum())
        row["largest_zone_cells"] = int(m.max())
        lo, hi, _, _ = dsm.quantile_ranks(m, QS)
        ranks = torch.cat([lo, hi], dim=1).contiguous()
        R = ranks.shape[1]
        nbytes = lib.smvs_dsm_label_select_workspace_bytes(n, R)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out, nv = torch.empty((n, R), dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        row["workspace_bytes"] = nbytes
        row["select_ms"] = timed(lambda: select(labels, values, n, ranks, out, nv, ws, nbytes), a.reps, a.warmup)
        want, want_m = composite(labels, values, n, ranks, NODATA)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)) and torch.equal(nv, want_m), name
        row["composite_equal"] = True
        row["torch_composite_ms"] = timed(lambda: composite(labels, values, n, ranks, NODATA), max(3, a.reps // 4), 1)
        row["select_over_label_stats"] = row["select_ms"]["median"] / row["label_stats_ms"]["median"]
        row["composite_over_select"] = row["torch_composite_ms"]["median"] / row["select_ms"]["median"]
        row["label_quantiles_api_ms"], _ = host_clock(lambda: dsm.label_quantiles(labels, n, values, QS, nodata=NODATA), 5)
        res["zones"].append(row)
        return m

    objects, table = dsm.extract_objects(above, grid, MIN_HEIGHT, nodata=NODATA)
    n_obj = int(table["area"].numel())
    m_obj = one_zone_map("nDSM objects", objects, n_obj, above)
    facets, n_facets = dsm.facets(z, grid, tol=2.0, slope_tol=0.4, nodata=NODATA)
    one_zone_map("facets at tol 2 m", facets, n_facets, z)
    one_zone_map("one zone over the grid", torch.ones((gh, gw), dtype=torch.int32, device=dev), 1, above)
    k = min(a.crop, gh, gw)
    own = torch.arange(1, k * k + 1, dtype=torch.int32, device=dev).reshape(k, k)
    one_zone_map("every cell its own label (%d x %d crop)" % (k, k), own, k * k, z[:k, :k])
    # the entry alone on the objects, by the number of ranks
    m64 = m_obj.long()
    kinds = [m64 // 2, (9 * m64) // 10, torch.zeros_like(m64), m64 - 1, m64 // 4, m64 // 3, (2 * m64) // 3, (3 * m64) // 4]
    res["by_n_ranks"] = []
    for R in (1, 2, 8):
        ranks = torch.stack(kinds[:R], dim=1).to(torch.int32).contiguous()
        nbytes = lib.smvs_dsm_label_select_workspace_bytes(n_obj, R)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out, nv = torch.empty((n_obj, R), dtype=torch.float32, device=dev), torch.empty(n_obj, dtype=torch.int32, device=dev)
        ms = timed(lambda: select(objects, above, n_obj, ranks, out, nv, ws, nbytes), a.reps, a.warmup)
        want, _ = composite(objects, above, n_obj, ranks, NODATA)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), R
        res["by_n_ranks"].append({"n_ranks": R, "n": n_obj, "select_ms": ms})
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
