#!/usr/bin/env python
"""Stack fusion timing on one MI355X ("Stack fusion").

Workload: the grid of tools/bench_dsm_morph.py (bench_dsm_post's grid after despike radius 2).  Cases: the four quadrant tiles of
tools/bench_dsm_mosaic.py overlapping by --overlap cells, and full-overlap stacks of 3, 7, 16 and 64 layers, each layer the grid
plus its own normal noise (sigma 0.5 m), 1 % blunders of +-30 .. 80 m and 2 % voids of its own.  Device events time --reps calls
after --warmup, outputs allocated outside the timed span.  For each case, in one process and on the same layers:
  smvs_dsm_stack_select  the median alone (one level, count, lo and hi) and four levels (1/10, 1/4, 1/2, 9/10)
  smvs_dsm_stack_fuse    with all seven outputs, k = 3, floor = 0.5
  smvs_dsm_mosaic        mode mean: it reads the same bytes once and adds them up -- the memory floor of any per-cell statistic
  a torch composite      of the same rules: the layers stacked as order-preserving int32 keys with a sentinel above every key,
                         torch.sort along the layer axis, gathers at the ranks, float64 arithmetic in the rule's order; its
                         outputs must have the bits of the native ones (asserted), and its time includes the stacking, which a
                         user of torch would have to do as well (host clock around a synchronised call, median of 3)
Nothing is fixed in advance: the times and the ratios native / mosaic-mean and composite / native are what the run reports.

    python tools/bench_dsm_stack.py [--size 5120] [--reps 20] [--warmup 3] [--json profiles/dsm_stack_bench.json]
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

LEVELS4 = [(1, 10), (1, 4), (1, 2), (9, 10)]
SENTINEL = 0x7fffffff                                        # the signed key of a NaN: above the key of every finite float
K_FACTOR, FLOOR = 3.0, 0.5


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


def keys_of(x):
    """float32 -> int32 whose signed order is the order of the floats, -0.0 below +0.0; its own inverse."""
    b = x.view(torch.int32)
    return b ^ ((b >> 31) & 0x7fffffff)


def canvas(layers, offsets, gw, gh):
    """(K, gh, gw) float32, NaN where a layer does not reach, and the validity of every entry."""
    Z = torch.full((len(layers), gh, gw), float("nan"), dtype=torch.float32, device=layers[0].device)
    for k, (z, (ox, oy)) in enumerate(zip(layers, offsets)):
        Z[k, oy:oy + z.shape[0], ox:ox + z.shape[1]] = z
    return Z, torch.isfinite(Z) & (Z != NODATA)


def at_rank(keys, rank):
    return keys_of(torch.gather(keys, 0, rank.clamp(0, keys.shape[0] - 1)[None])[0]).view(torch.float32)


def composite_select(layers, offsets, gw, gh, levels):
    Z, ok = canvas(layers, offsets, gw, gh)
    sentinel = torch.full((), SENTINEL, dtype=torch.int32, device=Z.device)
    keys = torch.sort(torch.where(ok, keys_of(Z), sentinel), dim=0).values
    m = ok.sum(dim=0)
    nd = torch.full((gh, gw), NODATA, dtype=torch.float32, device=Z.device)
    lo, hi = [], []
    for num, den in levels:
        h = (m - 1).clamp(min=0) * num
        lo_rank = torch.div(h, den, rounding_mode="floor")
        hi_rank = lo_rank + (h - lo_rank * den > 0)
        lo.append(torch.where(m > 0, at_rank(keys, lo_rank), nd))
        hi.append(torch.where(m > 0, at_rank(keys, hi_rank), nd))
    return m.to(torch.uint8), torch.stack(lo), torch.stack(hi)


def linear_half(keys, m):
    mid = torch.div((m - 1).clamp(min=0), 2, rounding_mode="floor")
    rem = (m - 1).clamp(min=0) - 2 * mid
    a, b = at_rank(keys, mid).double(), at_rank(keys, mid + rem).double()
    return a + (b - a) * (rem.double() / 2.0)


def composite_fuse(layers, offsets, gw, gh, kmad, floor):
    Z, ok = canvas(layers, offsets, gw, gh)
    sentinel = torch.full((), SENTINEL, dtype=torch.int32, device=Z.device)
    m = ok.sum(dim=0)
    some = m > 0
    med = linear_half(torch.sort(torch.where(ok, keys_of(Z), sentinel), dim=0).values, m).float()
    d = (Z.double() - med.double()[None]).abs().float()
    mad = linear_half(torch.sort(torch.where(ok, keys_of(d), sentinel), dim=0).values, m).float()
    thr = torch.fmax(kmad * mad.double(), torch.full((), floor, dtype=torch.float64, device=Z.device))
    inl = ok & (d.double() <= thr[None])
    S = torch.zeros((gh, gw), dtype=torch.float64, device=Z.device)
    started = torch.zeros((gh, gw), dtype=torch.bool, device=Z.device)
    for k in range(Z.shape[0]):                              # the sum in the layers' order, started from its first term
        zk = Z[k].double()
        S = torch.where(inl[k], torch.where(started, S + zk, zk), S)
        started = started | inl[k]
    n_in = inl.sum(dim=0)
    nd = torch.full((gh, gw), NODATA, dtype=torch.float32, device=Z.device)
    out = torch.where(some, torch.where(n_in > 0, (S / n_in).float(), med), nd)
    return out, torch.where(some, med, nd), torch.where(some, mad, nd), m.to(torch.uint8), n_in.to(torch.uint8)


def same_bits(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def run_case(name, layers, offsets, gw, gh, dev, a):
    stream = _lib.current_stream(dev)
    K = len(layers)
    table = (dsm._Layer * K)(*[dsm._Layer(t.data_ptr(), None, t.shape[1], t.shape[0], ox, oy) for t, (ox, oy) in zip(layers, offsets)])
    f32 = lambda *s: torch.empty(s + (gh, gw), dtype=torch.float32, device=dev)
    u8 = lambda: torch.empty((gh, gw), dtype=torch.uint8, device=dev)
    i64 = lambda: torch.empty((gh, gw), dtype=torch.int64, device=dev)
    P = _lib.ptr
    half = np.array([(1, 2)], np.int32)
    four = np.array(LEVELS4, np.int32)
    count, lo1, hi1, lo4, hi4 = u8(), f32(1), f32(1), f32(4), f32(4)
    out, med, mad, n_in, mem, inl, mean = f32(), f32(), f32(), u8(), i64(), i64(), f32()
    kmad = K_FACTOR * dsm.NMAD_FACTOR
    t_median = timed(lambda: _lib.call("smvs_dsm_stack_select", table, K, NODATA, half.ctypes.data, 1, None, gw, gh, P(count), P(lo1), P(hi1), stream),
                     a.reps, a.warmup)
    t_four = timed(lambda: _lib.call("smvs_dsm_stack_select", table, K, NODATA, four.ctypes.data, 4, None, gw, gh, P(count), P(lo4), P(hi4), stream),
                   a.reps, a.warmup)
    t_fuse = timed(lambda: _lib.call("smvs_dsm_stack_fuse", table, K, NODATA, kmad, FLOOR, 1, gw, gh, P(out), P(med), P(mad), P(count), P(n_in),
                                     P(mem), P(inl), stream), a.reps, a.warmup)
    t_mean = timed(lambda: _lib.call("smvs_dsm_mosaic", table, K, NODATA, dsm.MOSAIC_MODES["mean"], 1, gw, gh, P(mean), None, None, None, stream),
                   a.reps, a.warmup)
    c_count, c_lo, c_hi = composite_select(layers, offsets, gw, gh, [(1, 2)])
    equal_select = same_bits(c_lo, lo1) and same_bits(c_hi, hi1) and bool(torch.equal(c_count, count))
    c4 = composite_select(layers, offsets, gw, gh, LEVELS4)
    equal_four = same_bits(c4[1], lo4) and same_bits(c4[2], hi4)
    del c4
    c = composite_fuse(layers, offsets, gw, gh, kmad, FLOOR)
    equal_fuse = same_bits(c[0], out) and same_bits(c[1], med) and same_bits(c[2], mad) and bool(torch.equal(c[3], count)) and bool(torch.equal(c[4], n_in))
    del c, c_count, c_lo, c_hi
    assert equal_select and equal_four and equal_fuse, (name, equal_select, equal_four, equal_fuse)
    ct_median = host_timed(lambda: composite_select(layers, offsets, gw, gh, [(1, 2)]))
    ct_four = host_timed(lambda: composite_select(layers, offsets, gw, gh, LEVELS4))
    ct_fuse = host_timed(lambda: composite_fuse(layers, offsets, gw, gh, kmad, FLOOR))
    read_bytes = sum(int(t.numel()) * 4 for t in layers)
    r = lambda x, y: x["median"] / y["median"]
    return {"case": name, "layers": K, "cells": gw * gh, "layer_bytes": read_bytes, "mean_valid_layers": float(count.float().mean()),
            "outlier_share": float(((mem & ~inl) != 0).float().mean()),
            "select_median_ms": t_median, "select_four_levels_ms": t_four, "fuse_ms": t_fuse, "mosaic_mean_ms": t_mean,
            "composite_select_median_ms": ct_median, "composite_select_four_levels_ms": ct_four, "composite_fuse_ms": ct_fuse,
            "select_median_over_mosaic_mean": r(t_median, t_mean), "select_four_levels_over_mosaic_mean": r(t_four, t_mean),
            "fuse_over_mosaic_mean": r(t_fuse, t_mean),
            "composite_over_select_median": r(ct_median, t_median), "composite_over_select_four_levels": r(ct_four, t_four),
            "composite_over_fuse": r(ct_fuse, t_fuse),
            "select_median_layer_GBps": read_bytes / (1e6 * t_median["median"]), "mosaic_mean_layer_GBps": read_bytes / (1e6 * t_mean["median"]),
            "equal_bits_select": equal_select, "equal_bits_four_levels": equal_four, "equal_bits_fuse": equal_fuse}


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
    ap.add_argument("--stacks", default="3,7,16,64")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dsm_stack needs an MI355X")
    dev = torch.device("cuda:0")
    z, grid = bench_grid(a, dev)
    gh, gw = z.shape
    ok = torch.isfinite(z) & (z != NODATA)
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "bench_dsm_morph's grid (%dx%d, %.1f m cells) after despike radius 2, void share %.4f" % (gw, gh, a.res, 1.0 - float(ok.float().mean())),
           "cells": gw * gh, "fuse": {"k": K_FACTOR, "floor": FLOOR, "min_count": 1}, "levels_of_four": LEVELS4,
           "scratch_bytes": scratch_sizes(r"dsm_stack|dsm_mosaic"), "cases": [],
           "kernel_traces": "not measured", "counters": "not measured", "real_dsms": "not measured"}
    hr, hc, o = gh // 2, gw // 2, a.overlap // 2
    cuts = [(0, hr + o, 0, hc + o), (0, hr + o, hc - o, gw), (hr - o, gh, 0, hc + o), (hr - o, gh, hc - o, gw)]
    tiles = [z[r0:r1, c0:c1].contiguous() for r0, r1, c0, c1 in cuts]
    res["cases"].append(run_case("four tiles, overlap %d" % a.overlap, tiles, [(c0, r0) for r0, r1, c0, c1 in cuts], gw, gh, dev, a))
    del tiles
    g = torch.Generator(device=dev).manual_seed(7)
    for K in [int(v) for v in a.stacks.split(",")]:
        layers = []
        for _ in range(K):
            t = z + 0.5 * torch.randn((gh, gw), device=dev, generator=g)
            u = torch.rand((gh, gw), device=dev, generator=g)
            amp = (30.0 + 50.0 * torch.rand((gh, gw), device=dev, generator=g)) * torch.where(torch.rand((gh, gw), device=dev, generator=g) < 0.5, -1.0, 1.0)
            t = torch.where(u < 0.01, t + amp, t)
            t = torch.where(ok & (u < 0.98), t, torch.full_like(t, NODATA))
            layers.append(t.contiguous())
        res["cases"].append(run_case("full overlap, %d layers" % K, layers, [(0, 0)] * K, gw, gh, dev, a))
        del layers
        torch.cuda.empty_cache()
    res["equal_bits_everywhere"] = all(c["equal_bits_select"] and c["equal_bits_four_levels"] and c["equal_bits_fuse"] for c in res["cases"])
    res["native_loses_to_composite"] = [c["case"] for c in res["cases"]
                                        if min(c["composite_over_select_median"], c["composite_over_select_four_levels"], c["composite_over_fuse"]) < 1.0]
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
