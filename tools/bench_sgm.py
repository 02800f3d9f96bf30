#!/usr/bin/env python
"""The census plane sweep and SGM, timed on one MI355X ("Census plane sweep and SGM").

Workload: the headline shape, 3 views of 768 x 384 and 64 planes, synthetic RPCs (rpc_synth, tilts 0 and +-0.4) and a generated
ground texture seen by every view over a smooth surface; nothing is read from disk.  Device events time --reps calls after
--warmup, workspaces and outputs allocated outside the timed span.
smvs_sgm_census_cost on one chunk of 16 planes (its warped volumes made before) and the whole sweep through sgm.census_cost
(warps included), smvs_sgm_aggregate at 4 and at 8 paths (with the time per step of a line derived from them: 2 W + 2 H steps
of launches that run one after the other at 4 paths, 4 min(H, W) more at 8), smvs_sgm_select, and sgm.sgm_heights end to end
(host clock around a synchronise, median of 3).  Beside them, from the same process: the variance cost volume of 8-channel
features on the same planes, one Infer_CascadeREDNet forward (random weights, 48 / 32 / 8 planes), and a torch composite of
the aggregation rule (a loop over the steps with tensor operators on all lines of a direction, timed once) whose sum is
asserted equal in bits.  The one condition: the native aggregation is faster than the composite.

    python tools/bench_sgm.py [--height 384] [--width 768] [--planes 64] [--reps 20] [--warmup 3] [--json profiles/sgm_bench.json]
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
from bench_dsm_sun import host_timed  # noqa: E402
from dsm_bench_common import timed  # noqa: E402
from satmvs_amd import _lib, rpc_synth, sgm  # noqa: E402
from satmvs_amd.modules import warping  # noqa: E402

CLOCK_GHZ = 2.4                                               # the nominal shader clock, for cycles per step
DIRS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))


def views(H, W, seed=0):
    """(images 3 x (H, W) float32, rpc (3, 170)): a ground texture of Gaussian-filtered noise seen over 200 + 12 sin cos metres."""
    rpc = rpc_synth.make_view_rpcs(3, H, W, seed=seed, tilts=(0.0, 0.4, -0.4), gsd=1.0)
    rng = np.random.default_rng(seed + 1)
    gh, gw = 2 * H + 8, 2 * W + 8
    fy, fx = np.fft.fftfreq(gh)[:, None], np.fft.rfftfreq(gw)[None, :]
    tex = np.zeros((gh, gw))
    for sg in (1.5, 5.0, 16.0):
        t = np.fft.irfft2(np.fft.rfft2(rng.standard_normal((gh, gw))) * np.exp(-2.0 * (np.pi * sg) ** 2 * (fy * fy + fx * fx)), s=(gh, gw))
        tex += t / t.std()
    lat0, lon0, ls, os_ = rpc[0, 2], rpc[0, 3], rpc[0, 7], rpc[0, 8]
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    images = []
    for v in range(3):
        h = np.full(H * W, 200.0)
        for _ in range(6):
            lat, lon = rpc_synth.photo2obj(rpc[v], xx.ravel(), yy.ravel(), h)
            h = 200.0 + 12.0 * np.sin(2.1 * (lat - lat0) / ls + 0.4) * np.cos(1.7 * (lon - lon0) / os_ - 0.3)
        fy_ = np.clip((1.0 - ((lat - lat0) / ls + 1.0) * 0.5) * (gh - 1), 0, gh - 1.001)
        fx_ = np.clip(((lon - lon0) / os_ + 1.0) * 0.5 * (gw - 1), 0, gw - 1.001)
        y0, x0 = np.floor(fy_).astype(np.int64), np.floor(fx_).astype(np.int64)
        wy, wx = fy_ - y0, fx_ - x0
        img = tex[y0, x0] * (1 - wy) * (1 - wx) + tex[y0, x0 + 1] * (1 - wy) * wx + tex[y0 + 1, x0] * wy * (1 - wx) + tex[y0 + 1, x0 + 1] * wy * wx
        images.append((128.0 + 40.0 * img).reshape(H, W).astype(np.float32))
    return images, rpc


def composite(cost, P1, P2, paths, cost_max, void_cost):
    """The aggregation rule with torch operators: per direction a loop over the rows (or columns) with all lines stepping at once.
    cost (B, H, W, D) int16 holding uint16 bits -> sum, the same."""
    c = cost.to(torch.int32) & 0xFFFF
    cp = torch.where(c == 0xFFFF, void_cost, c.clamp(max=cost_max))
    B, H, W, D = cp.shape
    big = 1 << 30
    total = torch.zeros_like(cp)
    pad = torch.full((B, 1, 1), big, dtype=torch.int32, device=cp.device)
    for ry, rx in DIRS[:paths]:
        v = cp if ry != 0 else cp.transpose(1, 2)             # rows step; a horizontal direction steps the rows of the transpose
        sy, sx = (ry, rx) if ry != 0 else (rx, 0)
        n, w = v.shape[1], v.shape[2]
        x = torch.arange(w, device=cp.device)
        on = ((x - sx >= 0) & (x - sx < w))[None, :, None]
        src = (x - sx).clamp(0, w - 1)
        L = torch.empty_like(v)
        rows = range(n) if sy > 0 else range(n - 1, -1, -1)
        prev = None
        for y in rows:
            if prev is None:
                cur = v[:, y]
            else:
                q = prev[:, src]
                m = q.min(dim=-1, keepdim=True).values
                down = torch.cat([pad.expand(B, w, 1), q[..., :-1]], dim=-1) + P1
                up = torch.cat([q[..., 1:], pad.expand(B, w, 1)], dim=-1) + P1
                best = torch.minimum(torch.minimum(q, torch.minimum(down, up)), m + P2)
                cur = torch.where(on, v[:, y] + best - m, v[:, y])
            L[:, y] = cur
            prev = cur
        total += L if ry != 0 else L.transpose(1, 2)
    return total.to(torch.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-composite", action="store_true")
    ap.add_argument("--skip-cascade", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sgm needs an MI355X")
    dev = torch.device("cuda:0")
    H, W, D = a.height, a.width, a.planes
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    images, rpc = views(H, W)
    imgs = [torch.from_numpy(im[None]).to(dev) for im in images]
    pm = torch.from_numpy(rpc[None]).to(dev)
    depth = torch.linspace(170.0, 260.0, D, device=dev)[None].contiguous()
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
           "workload": "3 views %d x %d, %d planes 170 .. 260 m, radius 2, P1 16, P2 96, synthetic RPCs and a generated texture" % (W, H, D),
           "voxels": H * W * D, "clock_ghz_assumed": CLOCK_GHZ, "kernel_traces": "not measured", "counters": "not measured", "real_images": "not measured"}

    # census: one chunk of 16 planes on volumes warped before, and the whole sweep with its warps
    dc = min(16, D)
    feats = [torch.stack([im, torch.ones_like(im)], dim=1) for im in imgs[1:]]
    vols = [warping.rpc_warping(f, pm[:, v + 1], pm[:, 0], depth[:, :dc].contiguous()).contiguous() for v, f in enumerate(feats)]
    cost = torch.empty((1, H, W, D), dtype=torch.int16, device=dev)
    nbytes = lib.smvs_sgm_census_workspace_bytes(1, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ptrs = _lib.ptr_array(vols)
    ms = timed(lambda: _lib.call("smvs_sgm_census_cost", _lib.ptr(imgs[0]), ptrs, 2, 2, 0.999, _lib.ptr(cost), 1, H, W, 0, dc, D, _lib.ptr(ws), nbytes, stream), a.reps, a.warmup)
    res["census_chunk"] = {"planes": dc, "sources": 2, "ms": ms, "ms_for_all_planes": ms["median"] * D / dc,
                           "GB_per_s_of_warped_volume_read": 2 * 2 * dc * H * W * 4 / ms["median"] / 1e6}
    res["warp_chunk_ms"] = timed(lambda: warping.rpc_warping(feats[0], pm[:, 1], pm[:, 0], depth[:, :dc].contiguous()), a.reps, a.warmup)
    del vols
    res["census_sweep_ms"] = timed(lambda: sgm.census_cost(imgs[0], imgs[1:], pm[:, 0], [pm[:, 1], pm[:, 2]], depth), max(3, a.reps // 4), 1)
    cost = sgm.census_cost(imgs[0], imgs[1:], pm[:, 0], [pm[:, 1], pm[:, 2]], depth)
    res["void_share"] = float((cost == -1).float().mean())

    # aggregation
    total = torch.empty_like(cost)
    res["aggregate"] = {}
    for paths in (4, 8):
        ms = timed(lambda: _lib.call("smvs_sgm_aggregate", _lib.ptr(cost), None, _lib.ptr(total), 1, H, W, D, 16, 96, 16, 0, 768, 96, paths, stream), a.reps, a.warmup)
        res["aggregate"]["paths %d" % paths] = {"ms": ms}
    t4, t8 = res["aggregate"]["paths 4"]["ms"]["median"], res["aggregate"]["paths 8"]["ms"]["median"]
    axis_steps, diag_steps = 2 * W + 2 * H, 4 * min(H, W)
    res["aggregate"]["derived"] = {
        "axis_steps": axis_steps, "diagonal_steps": diag_steps,
        "ns_per_step_axis": 1e6 * t4 / axis_steps, "cycles_per_step_axis": 1e6 * t4 / axis_steps * CLOCK_GHZ,
        "ns_per_step_diagonal": 1e6 * (t8 - t4) / diag_steps, "cycles_per_step_diagonal": 1e6 * (t8 - t4) / diag_steps * CLOCK_GHZ,
        "GB_per_s_at_8_paths": (8 * 2 + 7 * 2 + 8 * 2) * H * W * D / t8 / 1e6,
        "note": "a launch is one direction and its waves (one per line) all run at once, so a launch lasts steps x the time of a step"}

    # select
    index = torch.empty((1, H, W), dtype=torch.int32, device=dev)
    height = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    min_sum, support = torch.empty((1, H, W), dtype=torch.int16, device=dev), torch.empty((1, H, W), dtype=torch.int16, device=dev)
    res["select_ms"] = timed(lambda: _lib.call("smvs_sgm_select", _lib.ptr(total), _lib.ptr(cost), _lib.ptr(depth), 0, 0, 1, _lib.ptr(index), _lib.ptr(height),
                                               _lib.ptr(min_sum), _lib.ptr(support), 1, H, W, D, stream), a.reps, a.warmup)
    res["sgm_heights_ms"] = host_timed(lambda: sgm.sgm_heights(imgs, pm, depth))

    # beside them: the variance volume and the learned cascade
    feas = [torch.randn(1, 8, H, W, device=dev) for _ in range(3)]
    with torch.no_grad():
        res["variance_cost_volume_8ch_ms"] = timed(lambda: warping.variance_cost_volume(feas, pm, depth, "rpc"), max(3, a.reps // 4), 1)
    del feas
    if a.skip_cascade:
        res["infer_cascade_red_ms"] = "not measured"
    else:
        from satmvs_amd.networks.casred import Infer_CascadeREDNet
        torch.manual_seed(0)
        net = Infer_CascadeREDNet("rpc", ndepths=[48, 32, 8]).to(dev).eval()
        x = torch.randn(1, 3, 3, H, W, device=dev)
        r0 = rpc_synth.make_view_rpcs(3, H, W, seed=0)[None]
        pms = {"stage1": torch.from_numpy(rpc_synth.rescale_rpc(r0, 4)).to(dev), "stage2": torch.from_numpy(rpc_synth.rescale_rpc(r0, 2)).to(dev),
               "stage3": torch.from_numpy(r0).to(dev)}
        dv = torch.tensor([[0.0, 400.0]], device=dev)
        with torch.no_grad():
            res["infer_cascade_red_ms"] = host_timed(lambda: net(x, pms, dv), reps=5)
        del net, x

    if a.skip_composite:
        res["torch_composite"] = "not measured"
    else:
        _lib.call("smvs_sgm_aggregate", _lib.ptr(cost), None, _lib.ptr(total), 1, H, W, D, 16, 96, 16, 0, 768, 96, 8, stream)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = composite(cost, 16, 96, 8, 768, 96)
        torch.cuda.synchronize()
        res["torch_composite"] = {"case": "8 paths", "ms_once": 1e3 * (time.perf_counter() - t0), "bits_equal": bool(torch.equal(want, total))}
        res["torch_composite"]["native_is_faster"] = bool(t8 < res["torch_composite"]["ms_once"])
        assert res["torch_composite"]["bits_equal"] and res["torch_composite"]["native_is_faster"], res["torch_composite"]
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
