#!/usr/bin/env python
"""Random shapes through the smaller operators of the path against the CPU oracle: rpc_warping / homo_warping (bits; a differing voxel
must be explained by its float32 coordinate, tests/ops_scene.py::explain_warp) and their backwards (float64 scatter, float32 summation
bound), softmax and window regressions, streaming regression, in-kernel height hypotheses (bits).   python tests/fuzz/fuzz_ops.py [n] [seed]"""
import os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as orc
from satmvs_amd.modules import module as M
from satmvs_amd.modules import warping
from satmvs_amd.modules.depth_range import GeneratedHeights
import ops_scene as osn

orc.build()
dev = torch.device("cuda:0")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 60
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
bad = 0
for it in range(n):
    C = int(rng.integers(1, 41)); D = int(rng.integers(1, 81)); H = int(rng.integers(1, 90)); W = int(rng.integers(1, 150)); B = int(rng.integers(1, 4))
    while C > 1 and B * C * D * H * W > 1.5e6:                   # the float64 references run on the CPU: thin the channels of the large draws
        C = max(1, C // 2)
    jitter = bool(rng.random() < 0.6)
    # ---- warps: forward (bits, every difference explained) and backward (float64 scatter of the oracle's taps)
    for geo in ("rpc", "pinhole"):
        seed = int(rng.integers(0, 10000))
        fea, src, ref, depth = osn.scene(geo, B, C, D, H, W, seed=seed, per_pixel=jitter)
        f = t(fea).requires_grad_(True)
        if geo == "rpc":
            out = warping.rpc_warping(f, t(src), t(ref), t(depth), None)
            want = orc.rpc_warping(fea, src, ref, depth)
        else:
            out = warping.homo_warping(f, t(src), t(ref), t(depth))
            want = orc.homo_warping(fea, src, ref, depth)
        got = out.detach().cpu().numpy()
        msgs, nb = osn.explain_warp(orc, geo, got, want, fea, src, ref, depth)
        if msgs:
            bad += 1; print("MISMATCH warp %s it=%d B=%d C=%d D=%d H=%d W=%d jitter=%s seed=%d: %s" % (geo, it, B, C, D, H, W, jitter, seed, msgs[0]))
            continue
        vox = ((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))).any(1)
        gout = np.random.default_rng(seed).standard_normal(got.shape).astype(np.float32)
        gout[np.broadcast_to(vox[:, None], gout.shape)] = 0.0    # a voxel whose forward differs has other taps than the oracle's: out of both sides
        out.backward(t(gout))
        off, wts = osn.taps_from_grid(*osn.oracle_grid(orc, geo, src, ref, depth, H, W), H, W)
        msgs, worst, nmax = osn.check_backward(f.grad.cpu().numpy(), gout, off, wts, H, W, "backward")
        if msgs:
            bad += 1; print("MISMATCH warp backward %s it=%d B=%d C=%d D=%d H=%d W=%d jitter=%s seed=%d: %s" % (geo, it, B, C, D, H, W, jitter, seed, msgs[0]))
    # ---- regressions
    reg = (rng.standard_normal((B, D, H, W)) * 3).astype(np.float32)
    dvals = depth if depth.ndim == 4 else depth
    with torch.no_grad():
        d1, c1 = M.softmax_depth_regression(t(reg), t(dvals))
        d2, c2, v2 = M.window_depth_regression(t(reg), t(dvals), lamb=1.5)
    od, oc = orc.softmax_regress(reg, dvals)
    wd, wc, wv = orc.window_regress(reg, dvals, lamb=1.5)
    e = [np.abs(d1.cpu().numpy() - od).max(), np.abs(c1.cpu().numpy() - oc).max(), np.abs(d2.cpu().numpy() - wd).max(), np.abs(v2.cpu().numpy() - wv).max()]
    if e[0] > 1e-3 or e[1] > 1e-5 or e[2] > 1e-3 or e[3] > 2e-3 or (np.abs(c2.cpu().numpy() - wc) > 1e-5).mean() > 0.01:
        bad += 1; print("MISMATCH regress it=%d B=%d D=%d H=%d W=%d: %s" % (it, B, D, H, W, e))
    acc = M.StreamingRegression(B, H, W, dev)
    oacc = orc.StreamRegress(B, H, W)
    for d in range(D):
        acc.step(t(reg[:, d]), t(dvals), d)
        oacc.step(reg[:, d], dvals, d)
    sd, sc = acc.result()
    osd, osc = oacc.final()
    if np.abs(sd.cpu().numpy() - osd).max() > 1e-4 or np.abs(sc.cpu().numpy() - osc).max() > 1e-6:
        bad += 1; print("MISMATCH streaming it=%d" % it, np.abs(sd.cpu().numpy() - osd).max())
    # ---- in-kernel hypotheses (bit comparison)
    sh, sw = int(rng.integers(2, 40)), int(rng.integers(2, 60))
    scale = int(rng.choice([1, 2]))
    prev = (200.0 + 50.0 * rng.standard_normal((B, sh, sw))).astype(np.float32)
    nd = int(rng.integers(2, 12)); interval = float(rng.choice([1.25, 2.5, 5.0, 10.0]))
    img_hw, stage_hw = (sh * 2 * scale, sw * 2 * scale), (sh * 2, sw * 2)
    gen = GeneratedHeights(t(prev), nd, interval, img_hw, stage_hw)
    got = gen.materialize().cpu().numpy()
    want = orc.height_hypotheses(prev, nd, interval, img_hw, stage_hw)
    if not np.array_equal(got, want):
        bad += 1; print("MISMATCH hypotheses it=%d prev %s nd=%d interval=%g img=%s stage=%s: %d differ" % (it, prev.shape, nd, interval, img_hw, stage_hw, int((got != want).sum())))
print("%d rounds, %d mismatching checks" % (n, bad))
