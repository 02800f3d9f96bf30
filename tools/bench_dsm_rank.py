#!/usr/bin/env python
"""Focal order statistics timing on one MI355X ("Focal order statistics").

Workload: the grid of tools/bench_dsm_label.py (bench_dsm_morph's grid, 2199 x 2158 at the default size, after despike radius 2).
Device events time --reps calls after --warmup (a quarter of them at radii of 16 and more), buffers allocated outside the timed
span: smvs_dsm_focal_select for the median (one level, n_out, lo and hi) over a box and a disc at radii 1, 3, 8, 16 and 32; the
same in deviation mode (centre = the median grid) and smvs_dsm_focal_count (t = the DSM) at radius 8.  Every formulation of the
descent is timed on the same calls: the library as built, and with --variant-lib NAME=PATH (repeatable) further builds of it, e.g.
    python -c "from satmvs_amd import build; build.build(extra_flags=['-DSMVS_RANK_BITS=1'], out='<path>')"
each with its outputs held equal in bits to the first build's.  Beside them, from the same process: smvs_dsm_despike, the only
moving-window median the library had, at radii 1 to 3 (square windows, its own rule on top of the median), and a torch composite
of the same rule at every radius (the int64 keys padded with a key above all, rows staged in chunks, unfold windows masked by the
footprint, torch.sort, a gather at the two ranks) whose n, lo and hi are asserted equal to the native ones in every bit; it is
timed --composite-reps times up to radius 8 and once beyond.  dsm.focal_median, dsm.despike_robust and dsm.elevation_percentile
end to end are under a host clock round a synchronise.  No time is a condition.

    python tools/bench_dsm_rank.py [--size 5120] [--reps 20] [--warmup 3] [--variant-lib NAME=PATH] [--json profiles/dsm_rank_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_dsm_focal import host_clock  # noqa: E402
from bench_dsm_morph import NODATA, bench_grid  # noqa: E402
from dsm_bench_common import scratch_sizes, timed  # noqa: E402
from satmvs_amd import _lib, dsm  # noqa: E402

RADII = (1, 3, 8, 16, 32)
VOID = 1 << 32                                               # above every key
COMPOSITE_BYTES = 1 << 30                                    # keys of one chunk of rows


def keys_of(z, nodata):
    """int64: the order-preserving image of the bits of a valid cell, VOID elsewhere."""
    u = z.view(torch.int32).long() & 0xffffffff
    key = torch.where(u >= 0x80000000, u ^ 0xffffffff, u | 0x80000000)
    return torch.where(torch.isfinite(z) & (z != nodata), key, torch.full_like(key, VOID))


def composite_median(z, foot, nodata):
    """The rule in torch for the level 1 / 2 -> (n int32, lo key, hi key int64), VOID where n = 0."""
    gh, gw = z.shape
    fh, fw = foot.shape
    padded = torch.nn.functional.pad(keys_of(z, nodata), (fw // 2, fw // 2, fh // 2, fh // 2), value=VOID)
    rows = max(1, COMPOSITE_BYTES // (8 * gw * int(foot.sum())))
    n, lo, hi = [], [], []
    beat = time.monotonic()
    for r0 in range(0, gh, rows):
        if time.monotonic() - beat > 60.0:                   # a radius-32 call takes minutes: say that it is alive
            beat = time.monotonic()
            print("bench_dsm_rank: composite at row %d of %d" % (r0, gh), file=sys.stderr, flush=True)
        r1 = min(r0 + rows, gh)
        k = padded[r0:r1 + fh - 1].unfold(0, fh, 1).unfold(1, fw, 1)[:, :, foot].sort(dim=-1).values
        m = (k != VOID).sum(dim=-1)
        h = (m - 1).clamp(min=0)
        n.append(m.int())
        lo.append(k.gather(-1, (h // 2)[:, :, None])[:, :, 0])
        hi.append(k.gather(-1, (h // 2 + h % 2)[:, :, None])[:, :, 0])
        del k
    return torch.cat(n), torch.cat(lo), torch.cat(hi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=5120)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--res", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--composite-reps", type=int, default=3)
    ap.add_argument("--speckle", type=float, default=0.01)
    ap.add_argument("--drop", type=float, default=0.05)
    ap.add_argument("--built-name", default="2 bits a round (the library as built)")
    ap.add_argument("--variant-lib", action="append", default=[], metavar="NAME=PATH", help="a further build of the library to time on the same calls")
    ap.add_argument("--skip-composite", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dsm_rank needs an MI355X")
    dev = torch.device("cuda:0")
    z, _ = bench_grid(a, dev)
    z = z.contiguous()
    gh, gw = z.shape
    stream = _lib.current_stream(dev)
    libs = [(a.built_name, _lib.load())]
    for spec in a.variant_lib:
        name, path = spec.split("=", 1)
        other = C.CDLL(path)
        for entry in ("smvs_dsm_focal_select", "smvs_dsm_focal_count"):
            getattr(other, entry).argtypes = _lib._SIGNATURES[entry]
            getattr(other, entry).restype = C.c_int
        libs.append((name, other))
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "bench_dsm_morph's grid (%dx%d, %.1f m cells) after despike" % (gw, gh, a.res), "cells": gw * gh,
           "valid_share": float((torch.isfinite(z) & (z != NODATA)).float().mean()), "tile": dsm.RANK_TILE,
           "formulations": [name for name, _ in libs], "scratch_bytes": scratch_sizes(r"dsm_rank_"), "launches_per_call": 1, "median": [],
           "tile_rank_compression": "not built", "kernel_traces": "not measured", "counters": "not measured", "real_dsms": "not measured",
           "levels_beyond_one": "not measured", "windows_other_than_box_and_disc": "not measured"}
    n, lo, hi = (torch.empty((gh, gw), dtype=dt, device=dev) for dt in (torch.int32, torch.float32, torch.float32))
    first = [torch.empty_like(t) for t in (n, lo, hi)]
    half = np.array([[1, 2]], dtype=np.int32)

    def select(lib, runs, centre=None):
        rc = lib.smvs_dsm_focal_select(_lib.ptr(z), gw, gh, NODATA, runs.ctypes.data, len(runs), half.ctypes.data, 1,
                                       _lib.ptr(centre) if centre is not None else None, _lib.ptr(n), _lib.ptr(lo), _lib.ptr(hi), stream)
        assert rc == 0, _lib.load().smvs_last_error()

    def every_formulation(call, reps):
        """{name: stats} of call(lib), the outputs of every later build asserted equal in bits to the first one's."""
        out = {}
        for k, (name, lib) in enumerate(libs):
            out[name] = timed(lambda: call(lib), reps, a.warmup)
            for got, keep in zip((n, lo, hi), first):
                if k == 0:
                    keep.copy_(got)
                else:
                    assert torch.equal(got.view(torch.int32), keep.view(torch.int32)), name
        return out

    out = torch.empty_like(z)
    for radius in RADII:
        reps = a.reps if radius < 16 else max(3, a.reps // 4)
        despike_ms = (timed(lambda: _lib.call("smvs_dsm_despike", _lib.ptr(z), gw, gh, NODATA, radius, 10.0, 3, _lib.ptr(out), None, stream), a.reps, a.warmup)
                      if radius <= 3 else "not served: despike takes radii up to 3")
        for shape in ("box", "disc"):
            w = dsm.focal_window(shape, radius)
            runs = dsm._window_runs(w)
            row = {"shape": shape, "radius": radius, "cells": w.cells, "runs": len(runs), "despike_ms": despike_ms}
            row["select_ms"] = every_formulation(lambda lib: select(lib, runs), reps)
            if not a.skip_composite:
                foot = torch.zeros((2 * radius + 1, 2 * radius + 1), dtype=torch.bool, device=dev)
                for dy, dx0, dx1 in runs.tolist():
                    foot[dy + radius, dx0 + radius:dx1 + radius + 1] = True
                kept = []                                    # the last timed call's outputs are the ones compared
                row["torch_composite_ms"] = timed(lambda: kept.append(composite_median(z, foot, NODATA)) or kept.__delitem__(slice(0, -1)),
                                                  a.composite_reps if radius <= 8 else 1, 0)
                cn, clo, chi = kept.pop()
                some = cn > 0
                assert torch.equal(cn, first[0]), (shape, radius)
                for got, want in ((first[1], clo), (first[2], chi)):
                    assert torch.equal(torch.where(some, keys_of(got, float("nan")), torch.full_like(want, VOID)), want), (shape, radius)
                    assert bool((got[~some] == NODATA).all())
                del cn, clo, chi
                row["composite_equal"] = True
                row["composite_over_select"] = row["torch_composite_ms"]["median"] / row["select_ms"][libs[0][0]]["median"]
            res["median"].append(row)
            print("bench_dsm_rank: %s radius %d done" % (shape, radius), file=sys.stderr, flush=True)
    # radius 8: the deviation mode and the counts
    res["radius_8"] = []
    below, equal = torch.empty_like(n), torch.empty_like(n)
    for shape in ("box", "disc"):
        runs = dsm._window_runs(dsm.focal_window(shape, 8))
        select(libs[0][1], runs)
        centre = (0.5 * (lo.double() + hi.double())).float()
        row = {"shape": shape, "deviation_select_ms": every_formulation(lambda lib: select(lib, runs, centre), a.reps)}
        row["count_ms"] = timed(lambda: _lib.call("smvs_dsm_focal_count", _lib.ptr(z), gw, gh, NODATA, runs.ctypes.data, len(runs), _lib.ptr(z),
                                                  _lib.ptr(n), _lib.ptr(below), _lib.ptr(equal), stream), a.reps, a.warmup)
        res["radius_8"].append(row)
    res["api_ms"] = {"focal_median disc 8": host_clock(lambda: dsm.focal_median(z, dsm.focal_window("disc", 8), nodata=NODATA), 5)[0],
                     "despike_robust box 7": host_clock(lambda: dsm.despike_robust(z, dsm.focal_window("box", 7), nodata=NODATA), 5)[0],
                     "elevation_percentile disc 8": host_clock(lambda: dsm.elevation_percentile(z, dsm.focal_window("disc", 8), nodata=NODATA), 5)[0]}
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
