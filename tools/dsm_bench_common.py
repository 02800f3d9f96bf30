"""What the DSM bench tools (bench_dsm, bench_dsm_render, bench_dsm_post, bench_dsm_morph, bench_ortho) share: timing with
HIP events, the {min, median, max, reps} summary, the scratch sizes of the kernels in the built library, and the two scene
builders (height maps for production, a DSM with blocks for rendering and the orthophoto)."""
import os
import re
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFTS = (0.0, 0.4, -0.4)


def stats(ts):
    ts = sorted(ts)
    return {"min": ts[0], "median": ts[len(ts) // 2], "max": ts[-1], "reps": len(ts)}


def timed(fn, reps, warmup, reset=None):
    """stats() of `reps` event-timed calls of fn after `warmup` untimed ones; `reset`, if given, runs untimed before each call."""
    for _ in range(warmup):
        if reset:
            reset()
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        if reset:
            reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return stats(ts)


def scratch_sizes(pattern):
    """{kernel: private segment bytes} of the kernels whose name matches `pattern`, from the code objects inside the built library."""
    from satmvs_amd import _lib
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), _lib.LIB_PATH, "dsm_"],
                         capture_output=True, text=True).stdout
    sizes = {}
    for line in out.splitlines()[1:]:
        f = line.split()
        if len(f) >= 8 and re.search(pattern, f[0]):
            sizes[f[0]] = int(f[-3])
    return sizes


def synth_heights(n_views, size, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    y = torch.arange(size, device=dev, dtype=torch.float32)[:, None]
    x = torch.arange(size, device=dev, dtype=torch.float32)[None, :]
    base = 150.0 + 60.0 * torch.sin(x / 97.0) * torch.cos(y / 131.0)
    out = []
    for _ in range(n_views):
        h = base + 2.0 * torch.randn((size, size), device=dev, generator=g)
        h[torch.rand((size, size), device=dev, generator=g) < 0.01] = float("nan")    # holes, as after filtering
        out.append(h.contiguous())
    return out


def scene_dsm(grid, seed=0):
    """Terrain (+-30 m over kilometres) plus rectangular blocks 20 - 60 m high, float32 (gh, gw)."""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:grid.height, 0:grid.width].astype(np.float64)
    E, N = grid.e0 + c * grid.xres, grid.n0 - r * grid.yres
    z = 150.0 + 30.0 * np.sin(E / 900.0) * np.cos(N / 1300.0) + 5.0 * np.sin(E / 170.0 + N / 230.0)
    nb = grid.width * grid.height // 400                    # about one block per 400 cells
    rr, cc = rng.integers(0, grid.height - 12, nb), rng.integers(0, grid.width - 12, nb)
    hh, ww = rng.integers(3, 12, nb), rng.integers(3, 12, nb)
    up = rng.uniform(20.0, 60.0, nb)
    for i in range(nb):
        z[rr[i]:rr[i] + hh[i], cc[i]:cc[i] + ww[i]] += up[i]
    return z.astype(np.float32)
