#!/usr/bin/env python
"""Random pairs through the geometric-consistency kernels (RPC and pinhole) against the CPU oracle: reference and source sizes drawn
independently (1 ... 400 per side, the reference at most 4 x the source along an axis), random view geometry and thresholds, a share
of NaN, border-valued and blunder pixels in both maps.  Every stage against the oracle applied to the kernel's own output of the stage before, and end to end with the differing
pixels a subset of the at-risk pixels (tests/filter_scene.py).   python tests/fuzz/fuzz_filter.py [n] [seed]"""
import os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as orc
from satmvs_amd import pinhole_filter, rpc_filter
import filter_scene as fs

orc.build()
assert torch.cuda.is_available()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
bad = pixels = 0
for it in range(n):
    side = lambda: int(rng.integers(1, 401)) if rng.random() < 0.8 else int(rng.integers(1, 9))
    while True:
        ref, src = (side(), side()), (side(), side())
        # both views have one ground resolution, so a reference more than 4 x the source along an axis projects its rim to more than
        # 4 x the source RPC's normalised range: the rational cubics near their poles there, where two float64 evaluations of the
        # SAME coordinate part by up to 2.5e-4 px (393 x 228 onto 7 x 101) -- not an input the 1e-8 px bound speaks about
        if ref[0] <= 4 * src[0] and ref[1] <= 4 * src[1]:
            break
    seed = int(rng.integers(0, 1000))
    shares = rng.random(3) * np.array([0.05, 0.05, 0.1]) * (rng.random(3) < 0.7)              # NaN, border value, blunders
    for kind, mod in (("rpc", rpc_filter), ("pinhole", pinhole_filter)):
        g, dr, ds, _, _ = fs.pair(kind, orc, ref, src, seed)
        dr, ds = dr.copy(), ds.copy()
        for a in (dr, ds):
            r = rng.random(a.shape)
            a[r < shares[2]] += np.float32(rng.choice([-9.0, 3.0, 40.0]))
            a[(r > 0.5) & (r < 0.5 + shares[1])] = g.border
            a[r > 1.0 - shares[0]] = np.nan
        p, d = float(rng.choice([0.25, 1.0, 3.0])), float(rng.choice([0.5, 2.5, 10.0]) if kind == "rpc" else rng.choice([0.002, 0.01, 0.1]))
        msgs = fs.stages(g, mod, dr, ds, p, d) + fs.end_to_end(g, mod, dr, ds, p, d, cap=False)[0]
        pixels += dr.size
        for m in msgs:
            bad += 1; print("MISMATCH it=%d ref=%s src=%s seed=%d p=%g d=%g shares=%s: %s" % (it, ref, src, seed, p, d, np.round(shares, 3).tolist(), m))
print("%d rounds, %d mismatching checks (%d reference pixels)" % (n, bad, pixels))
