#!/usr/bin/env python
"""Seeded-flood timing on one MI355X ("Seeded flood").

Workload: the grid of tools/bench_dsm_label.py (bench_dsm_morph's grid, 2199 x 2158 at the default size) and its nDSM
(dsm.extract_dtm, dsm.ndsm).  h_maxima of the nDSM at h = 0.5, 2 and 8 m: the global rounds to convergence (single rounds until
the status clears, untimed), then begin and that many rounds without a read between them (device events, --reps calls after
--warmup), and the API call under the default batch policy (host clock round a synchronise).  dsm.peaks, dsm.watershed from those
peaks and dsm.split_objects on the nDSM as API calls.  Beside them in the same process: smvs_dsm_flood_rounds on the DTM, the
same measurement; a torch composite of the same rule (3 x 3 max_pool2d + minimum on the quanta, swept to the fixed point, the
convergence read every 16 sweeps, stopped after --max-sweeps) with the surface asserted equal; and scipy.ndimage.grey_dilation
iterated on the host over a crop of --host-side cells a side, asserted equal too.  Nothing is gated.

    python tools/bench_dsm_watershed.py [--size 5120] [--reps 10] [--warmup 2] [--no-host] [--json profiles/dsm_watershed_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_dsm_morph import NODATA, bench_grid  # noqa: E402
from bench_dsm_outline import host_clock  # noqa: E402
from dsm_bench_common import timed  # noqa: E402
from satmvs_amd import _lib, dsm  # noqa: E402

HS = (0.5, 2.0, 8.0)


def quanta(z):
    """(q float32 with -inf where invalid, valid): |q| <= 2^23, exact in float32."""
    valid = torch.isfinite(z) & (z != NODATA) & (z.abs() <= 32768.0)
    q = torch.round(torch.where(valid, z, torch.zeros_like(z)).double() * 256.0).float()
    return torch.where(valid, q, torch.full_like(q, float("-inf"))), valid


def torch_h_maxima(q, H, max_sweeps):
    """Reconstruction by dilation of q - H under q as torch operators -> (quanta, sweeps, converged)."""
    rec = (q - H)[None, None]
    surface = q[None, None]
    sweeps = 0
    while sweeps < max_sweeps:
        before = rec
        for _ in range(16):
            rec = torch.minimum(F.max_pool2d(rec, 3, 1, 1), surface)
        sweeps += 16
        if torch.equal(before, rec):
            return rec[0, 0], sweeps, True
    return rec[0, 0], sweeps, False


def host_h_maxima(q, H):
    """The same with scipy.ndimage.grey_dilation on the host -> (quanta, sweeps)."""
    from scipy import ndimage
    rec, sweeps = q - H, 0
    while True:
        new = np.minimum(ndimage.grey_dilation(rec, size=(3, 3), mode="constant", cval=-np.inf), q)
        sweeps += 1
        if np.array_equal(new, rec):
            return rec, sweeps
        rec = new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=5120)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--res", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--speckle", type=float, default=0.01)
    ap.add_argument("--drop", type=float, default=0.05)
    ap.add_argument("--host-side", type=int, default=512, help="side of the crop scipy's grey_dilation is iterated on")
    ap.add_argument("--max-sweeps", type=int, default=4096)
    ap.add_argument("--no-host", action="store_true", help="leave the scipy iteration out")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dsm_watershed needs an MI355X")
    dev = torch.device("cuda:0")
    z, grid = bench_grid(a, dev)
    gh, gw = z.shape
    n = gh * gw
    dtm = dsm.extract_dtm(z, grid, NODATA).contiguous()
    above = dsm.ndsm(z, dtm, NODATA).contiguous()
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    p = _lib.ptr
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "bench_dsm_label's grid (%dx%d, %.1f m cells): its nDSM, and the DTM for the flood beside it" % (gw, gh, a.res),
           "cells": n, "h_maxima": [], "kernel_traces": "not measured", "real_ndsms": "not measured"}
    nbytes = lib.smvs_dsm_seed_workspace_bytes(gw, gh)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    keys = torch.empty((gh, gw), dtype=torch.int64, device=dev)
    word = torch.empty(2, dtype=torch.int32, device=dev)
    q, valid = quanta(above)
    for h in HS:
        H = dsm._h_quanta(h)
        row = {"h_m": h}

        def begin():
            _lib.call("smvs_dsm_seed_begin", p(above), p(above), None, gw, gh, NODATA, -1, H, p(keys), p(word[:1]), p(ws), nbytes, stream)

        def rounds(k):
            _lib.call("smvs_dsm_seed_rounds", p(above), gw, gh, NODATA, -1, p(keys), k, p(word[1:]), p(ws), nbytes, stream)

        begin()
        need = 0
        while True:
            rounds(1)
            need += 1
            if int(word[1].item()) == 0 or need > n + 2:
                break
        row["rounds_to_convergence"] = need

        def rounds_only():
            begin()
            left = need
            while left > 0:
                k = min(left, 4096)
                rounds(k)
                left -= k

        row["begin_and_rounds_ms"] = timed(rounds_only, a.reps, a.warmup)
        row["round_ms_mean"] = row["begin_and_rounds_ms"]["median"] / need
        surface = torch.empty_like(above)
        steps = torch.empty((gh, gw), dtype=torch.int32, device=dev)
        link = torch.empty((gh, gw), dtype=torch.uint8, device=dev)
        row["read_ms"] = timed(lambda: _lib.call("smvs_dsm_seed_read", p(above), p(above), None, gw, gh, NODATA, -1, H, p(keys), p(surface), p(steps), p(link),
                                                 p(word[:1]), p(ws), nbytes, stream), a.reps, a.warmup)
        row["api_ms"], (hm, run) = host_clock(lambda: dsm.h_maxima(above, h, nodata=NODATA, return_rounds=True), 3)
        row["api_rounds_run"] = run
        assert torch.equal(hm, surface)
        row["longest_flat_steps"] = int(steps.max().item())
        t0 = time.perf_counter()
        rec, sweeps, done = torch_h_maxima(q, float(H), a.max_sweeps)
        torch.cuda.synchronize()
        row["torch_composite"] = {"ms": 1e3 * (time.perf_counter() - t0), "sweeps": sweeps, "converged": done}
        if done:
            mine = torch.where(valid, torch.round(surface.double() * 256.0).float(), torch.full_like(q, float("-inf")))
            assert torch.equal(mine, rec), "the composite and the device differ at h = %g" % h
            row["torch_composite"]["equal_surface"] = True
        if a.no_host:
            row["scipy_grey_dilation_host"] = "not measured"
        else:
            side = min(a.host_side, gh, gw)
            crop = above[:side, :side].contiguous()
            qc = quanta(crop)[0].cpu().numpy()
            t0 = time.perf_counter()
            rec_host, sweeps_host = host_h_maxima(qc, np.float32(H))
            host_ms = 1e3 * (time.perf_counter() - t0)
            mine = dsm.h_maxima(crop, h, nodata=NODATA)
            mine = torch.where(quanta(crop)[1], torch.round(mine.double() * 256.0).float(), torch.full_like(mine, float("-inf"))).cpu().numpy()
            assert np.array_equal(mine, rec_host), "scipy and the device differ at h = %g" % h
            row["scipy_grey_dilation_host"] = {"ms": host_ms, "cells": side * side, "sweeps": sweeps_host, "equal_surface": True}
        res["h_maxima"].append(row)
    peaks_ms, (tops, n_tops, _, _) = host_clock(lambda: dsm.peaks(above, 2.0, grid, nodata=NODATA), 3)
    shed_ms, seg = host_clock(lambda: dsm.watershed(above, tops, nodata=NODATA), 3)
    split_ms, (labels, n_seg, table) = host_clock(lambda: dsm.split_objects(above, grid, nodata=NODATA), 3)
    objects, _ = dsm.extract_objects(above, grid, nodata=NODATA)
    res.update({"peaks_api_ms_h2": peaks_ms, "n_peaks_h2": int(n_tops), "watershed_api_ms": shed_ms, "watershed_cells_labelled": int((seg > 0).sum().item()),
                "split_objects_api_ms": split_ms, "n_segments": int(n_seg), "n_objects": int(objects.max().item())})
    # the flood beside it, in the same process
    fbytes = lib.smvs_dsm_flood_workspace_bytes(gw, gh)
    fws = torch.empty(fbytes, dtype=torch.uint8, device=dev)

    def flood_begin():
        _lib.call("smvs_dsm_flood_begin", p(dtm), gw, gh, NODATA, p(keys), p(fws), fbytes, stream)

    flood_begin()
    need = 0
    while True:
        _lib.call("smvs_dsm_flood_rounds", p(dtm), gw, gh, NODATA, p(keys), 1, p(word[1:]), p(fws), fbytes, stream)
        need += 1
        if int(word[1].item()) == 0 or need > n + 2:
            break

    def flood_rounds_only():
        flood_begin()
        left = need
        while left > 0:
            k = min(left, 4096)
            _lib.call("smvs_dsm_flood_rounds", p(dtm), gw, gh, NODATA, p(keys), k, p(word[1:]), p(fws), fbytes, stream)
            left -= k

    ms = timed(flood_rounds_only, a.reps, a.warmup)
    res["flood_on_the_dtm"] = {"rounds_to_convergence": need, "begin_and_rounds_ms": ms, "round_ms_mean": ms["median"] / need}
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
