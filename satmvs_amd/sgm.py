"""Heights from images alone: a census plane sweep and semi-global matching on the MI355X (smvs_sgm_* of include/satmvs.h,
satmvs_amd/csrc/sgm.hip).  No weights, no training.

    census_cost(ref, srcs, ref_geo, src_geos, depth_values, ...)  -> cost (B, H, W, D) uint16, 0xFFFF = no source covers the voxel
    aggregate(cost, p1, p2, paths, ...)                            -> sum  (B, H, W, D) uint16
    select(sum, depth_values, ...)                                 -> index, height, min_sum, support
    sgm_heights(images, proj_matrices, depth_values, ...)          -> {"height", "index", "min_sum", "support"}

The sweep warps the 2-channel feature [grey image, ones] of every source with the existing rpc_warping / homo_warping (channel 1
comes back as the coverage of the bilinear taps), `plane_chunk` planes at a time, so the float volumes never exist whole.  All
volumes are plane-minor: the D planes of a pixel are contiguous.  Device tensors give device tensors (a uint16 volume or map as
int16 with the same bits); host arrays are moved to the current device and the results come back as numpy, uint16 where the C
entry writes uint16.  Every argument is checked here, with ValueError, before the native call.

The defaults (radius 2, P1 16, P2 96, cost_max 768, void_cost 4 nbits, cov_min 0.999) were chosen on a synthetic 64 x 96 scene
(tests/sgm_scene.py); they are not tuned on real imagery.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .dsm import _back, _to_device
from .modules import warping

VOID = 0xFFFF
MAX_PLANES = 256
MAX_SOURCES = 7
NBITS = {1: 8, 2: 24, 3: 48}


def _int_in(v, name, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError("%s must be an integer in %d .. %d, got %r" % (name, lo, hi, v))
    return int(v)


def _volume(v, name):
    """A (B, H, W, D) plane-minor volume, checked before any device work -> what _put() takes."""
    if isinstance(v, torch.Tensor):
        if v.dtype not in (torch.int16, torch.uint16):
            raise ValueError("%s must hold uint16 (torch.uint16, or int16 with the same bits), got %s" % (name, v.dtype))
    else:
        v = np.asarray(v)
        if v.dtype != np.uint16:
            raise ValueError("%s must be uint16, got %s" % (name, v.dtype))
        v = v.view(np.int16)
    if v.ndim != 4:
        raise ValueError("%s must be (B, H, W, D), got shape %s" % (name, tuple(v.shape)))
    B, H, W, D = (int(s) for s in v.shape)
    if min(B, H, W) < 1 or not 1 <= D <= MAX_PLANES or B * H * W * D >= 2 ** 31:
        raise ValueError("%s needs B, H, W >= 1, 1 <= D <= %d and fewer than 2^31 cells, got %s" % (name, MAX_PLANES, (B, H, W, D)))
    return v


def _put(v, dev=None):
    """A checked volume -> (device int16 tensor holding the uint16 bits, whether the caller gave numpy)."""
    t, as_numpy = _to_device(v, None, dev)
    return (t.view(torch.int16) if t.dtype == torch.uint16 else t), as_numpy


def _u16(t, as_numpy):
    """The way back of a uint16 result: numpy uint16 for a caller who gave numpy, else the device tensor, int16 with those bits
    (torch has few operators for uint16)."""
    if t is None:
        return None
    return t.cpu().numpy().view(np.uint16) if as_numpy else t


def _image(a, name, shape=None):
    if not isinstance(a, torch.Tensor):
        a = np.asarray(a, dtype=np.float32)
    if a.ndim == 4 and a.shape[1] == 1:
        a = a[:, 0]
    if a.ndim != 3 or (shape is not None and tuple(a.shape) != tuple(shape)):
        raise ValueError("%s must be a grey image (B, H, W)%s, got shape %s" % (name, "" if shape is None else " = %s" % (tuple(shape),), tuple(a.shape)))
    return a


def _depths(depth_values, B, H, W):
    """The planes, checked before any device work -> (float32 array or tensor, depth_is_4d)."""
    d = depth_values if isinstance(depth_values, torch.Tensor) else np.asarray(depth_values, dtype=np.float32)
    if d.ndim == 2 and d.shape[0] == B:
        is4d = 0
    elif d.ndim == 4 and (d.shape[0], d.shape[2], d.shape[3]) == (B, H, W):
        is4d = 1
    else:
        raise ValueError("depth_values must be (B, D) or (B, D, H, W) with B, H, W = %s, got %s" % ((B, H, W), tuple(d.shape)))
    if not 1 <= d.shape[1] <= MAX_PLANES:
        raise ValueError("1 <= D <= %d planes, got %d" % (MAX_PLANES, d.shape[1]))
    if B * H * W * d.shape[1] >= 2 ** 31:
        raise ValueError("B H W D must be below 2^31, got %s planes of %s" % (d.shape[1], (B, H, W)))
    return d, is4d


def census_cost(ref, srcs, ref_geo, src_geos, depth_values, geo_model="rpc", radius=2, cov_min=0.999, plane_chunk=16):
    """The census matching cost of `ref` (B, H, W) against the sources `srcs` (a list of 1 .. 7 images of the same shape) over the
    planes `depth_values` ((B, D) or (B, D, H, W)) -> (B, H, W, D) uint16, 0xFFFF where no source covers the voxel's window.
    ref_geo / src_geos: (B, 170) RPCs, or (B, 4, 4) projection matrices with geo_model="pinhole"."""
    if geo_model not in ("rpc", "pinhole"):
        raise ValueError("geo_model must be 'rpc' or 'pinhole', got %r" % (geo_model,))
    radius = _int_in(radius, "radius", 1, 3)
    plane_chunk = _int_in(plane_chunk, "plane_chunk", 1, MAX_PLANES)
    cov_min = float(cov_min)
    if cov_min != cov_min:
        raise ValueError("cov_min must not be NaN")
    ref = _image(ref, "ref")
    if not isinstance(srcs, (list, tuple)) or not 1 <= len(srcs) <= MAX_SOURCES:
        raise ValueError("srcs must be a list of 1 .. %d images" % MAX_SOURCES)
    if not isinstance(src_geos, (list, tuple)) or len(src_geos) != len(srcs):
        raise ValueError("src_geos must be a list with one geometry per source")
    srcs = [_image(s, "srcs[%d]" % k, ref.shape) for k, s in enumerate(srcs)]
    B, H, W = (int(s) for s in ref.shape)
    if min(B, H, W) < 1 or B * H * W >= 2 ** 31:
        raise ValueError("ref needs positive sizes and fewer than 2^31 pixels, got %s" % ((B, H, W),))
    geo_shape = (B, 170) if geo_model == "rpc" else (B, 4, 4)
    for k, g in enumerate([ref_geo] + list(src_geos)):
        if tuple(np.shape(g)) != geo_shape:
            raise ValueError("%s must be %s for geo_model %r, got %s" % ("ref_geo" if k == 0 else "src_geos[%d]" % (k - 1), geo_shape, geo_model, tuple(np.shape(g))))
    depth, is4d = _depths(depth_values, B, H, W)
    r, as_numpy = _to_device(ref, torch.float32)
    dev = r.device
    depth = _to_device(depth, torch.float32, dev)[0]
    D = int(depth.shape[1])
    feats = [torch.stack([_to_device(s, torch.float32, dev)[0], torch.ones((B, H, W), dtype=torch.float32, device=dev)], dim=1) for s in srcs]
    rg = _to_device(ref_geo, torch.float64, dev)[0]
    sgs = [_to_device(g, torch.float64, dev)[0] for g in src_geos]
    warp = warping.rpc_warping if geo_model == "rpc" else warping.homo_warping
    cost = torch.empty((B, H, W, D), dtype=torch.int16, device=dev)
    nbytes = _lib.load().smvs_sgm_census_workspace_bytes(B, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.no_grad():
        for d0 in range(0, D, plane_chunk):
            dc = min(plane_chunk, D - d0)
            dv = depth[:, d0:d0 + dc].contiguous()
            vols = [warp(f, g, rg, dv).contiguous() for f, g in zip(feats, sgs)]
            _lib.launch(dev, "smvs_sgm_census_cost", r, _lib.ptr_array(vols), len(vols), radius, cov_min, cost, B, H, W, d0, dc, D, ws, nbytes)
    return _u16(cost, as_numpy)


def _penalties(p1, p2, paths, alpha, p2_min, cost_max, void_cost):
    paths = _int_in(paths, "paths", 4, 8)
    if paths not in (4, 8):
        raise ValueError("paths must be 4 or 8, got %d" % paths)
    p2 = _int_in(p2, "p2", 0, 65535)
    p1 = _int_in(p1, "p1", 0, p2)
    p2_min = p1 if p2_min is None else _int_in(p2_min, "p2_min", p1, p2)
    alpha = _int_in(alpha, "alpha", 0, 65535)
    cost_max = _int_in(cost_max, "cost_max", 0, 65535)
    void_cost = min(4 * NBITS[2], cost_max) if void_cost is None else _int_in(void_cost, "void_cost", 0, cost_max)
    if paths * (cost_max + p2) > 65535:
        raise ValueError("paths (cost_max + p2) must be at most 65535 for the sums to fit uint16, got %d (%d + %d)" % (paths, cost_max, p2))
    return p1, p2, paths, alpha, p2_min, cost_max, void_cost


def aggregate(cost, p1=16, p2=96, paths=8, guide=None, alpha=0, p2_min=None, cost_max=768, void_cost=None):
    """Semi-global aggregation of a (B, H, W, D) uint16 cost volume over 4 or 8 paths -> sum, the same shape and dtype.
    guide: (B, H, W) uint8; across an edge of it P2 falls to max(p2_min, p2 - alpha |dG|) (p2_min defaults to p1).  void_cost is
    what a void voxel (0xFFFF) costs; the default is 4 bits per bit of the radius-2 census, 96, clamped to cost_max."""
    p1, p2, paths, alpha, p2_min, cost_max, void_cost = _penalties(p1, p2, paths, alpha, p2_min, cost_max, void_cost)
    cost = _volume(cost, "cost")
    B, H, W, D = cost.shape
    if guide is not None:
        if not isinstance(guide, torch.Tensor):
            guide = np.asarray(guide)
        if guide.dtype not in (np.uint8, torch.uint8) or tuple(guide.shape) != (B, H, W):
            raise ValueError("guide must be uint8 of shape %s, got %s %s" % ((B, H, W), guide.dtype, tuple(guide.shape)))
    c, as_numpy = _put(cost)
    g = None if guide is None else _to_device(guide, None, c.device)[0]
    out = torch.empty_like(c)
    _lib.launch(c.device, "smvs_sgm_aggregate", c, g, out, B, H, W, D, p1, p2, p2_min, alpha, cost_max, void_cost, paths)
    return _u16(out, as_numpy)


def select(sum, depth_values, uniqueness=0, cost=None, min_support=1):
    """Winner-take-all over a (B, H, W, D) uint16 volume with a uniqueness test (0 .. 99 per cent; 0 = none) and a parabola through
    the winner and its neighbours -> (index int32, height float32, min_sum uint16, support uint16 or None), each (B, H, W).
    With `cost`, support counts a pixel's non-void planes and pixels below min_support are rejected (index -1, height NaN)."""
    uniqueness = _int_in(uniqueness, "uniqueness", 0, 99)
    min_support = _int_in(min_support, "min_support", 0, MAX_PLANES)
    sum = _volume(sum, "sum")
    B, H, W, D = sum.shape
    if cost is not None:
        cost = _volume(cost, "cost")
        if tuple(cost.shape) != tuple(sum.shape):
            raise ValueError("cost must have sum's shape %s, got %s" % (tuple(sum.shape), tuple(cost.shape)))
    depth, is4d = _depths(depth_values, B, H, W)
    if depth.shape[1] != D:
        raise ValueError("depth_values has %d planes, sum has %d" % (depth.shape[1], D))
    s, as_numpy = _put(sum)
    dev = s.device
    c = None if cost is None else _put(cost, dev)[0]
    depth = _to_device(depth, torch.float32, dev)[0]
    index = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    height = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    min_sum = torch.empty((B, H, W), dtype=torch.int16, device=dev)
    support = torch.empty((B, H, W), dtype=torch.int16, device=dev) if c is not None else None
    _lib.launch(dev, "smvs_sgm_select", s, c, depth, is4d, uniqueness, min_support, index, height, min_sum, support, B, H, W, D)
    return _back(as_numpy, index, height) + (_u16(min_sum, as_numpy), _u16(support, as_numpy))


def sgm_heights(images, proj_matrices, depth_values, geo_model="rpc", radius=2, cov_min=0.999, plane_chunk=16, p1=16, p2=96, paths=8,
                guide=None, alpha=0, p2_min=None, cost_max=768, void_cost=None, uniqueness=0, min_support=1):
    """Heights of view 0 from images alone.  images: a list of V grey images (B, H, W), view 0 the reference; proj_matrices:
    (B, V, 170) RPCs or, with geo_model="pinhole", (B, V, 4, 4); depth_values: (B, D) or (B, D, H, W) float32.
    -> {"height": float32 (NaN where rejected), "index": int32 (-1 where rejected), "min_sum": uint16, "support": uint16}.
    void_cost defaults to 4 per census bit of `radius`.  The defaults were chosen on a synthetic scene, not tuned on real data."""
    if not isinstance(images, (list, tuple)) or not 2 <= len(images) <= MAX_SOURCES + 1:
        raise ValueError("images must be a list of 2 .. %d views" % (MAX_SOURCES + 1))
    V = len(images)
    pm = proj_matrices if isinstance(proj_matrices, torch.Tensor) else np.asarray(proj_matrices, dtype=np.float64)
    want = (V, 170) if geo_model == "rpc" else (V, 4, 4)
    if pm.ndim != len(want) + 1 or tuple(pm.shape[1:]) != want:
        raise ValueError("proj_matrices must be (B,) + %s for geo_model %r, got %s" % (want, geo_model, tuple(pm.shape)))
    radius = _int_in(radius, "radius", 1, 3)
    if void_cost is None:
        void_cost = min(4 * NBITS[radius], _int_in(cost_max, "cost_max", 0, 65535))
    pen = _penalties(p1, p2, paths, alpha, p2_min, cost_max, void_cost)             # before any device work
    _int_in(uniqueness, "uniqueness", 0, 99)
    cost = census_cost(images[0], list(images[1:]), pm[:, 0], [pm[:, v] for v in range(1, V)], depth_values, geo_model, radius, cov_min, plane_chunk)
    total = aggregate(cost, pen[0], pen[1], pen[2], guide, pen[3], pen[4], pen[5], pen[6])
    index, height, min_sum, support = select(total, depth_values, uniqueness, cost, min_support)
    return {"height": height, "index": index, "min_sum": min_sum, "support": support}
