"""Test-local numpy oracle of the orthophoto (include/satmvs.h smvs_rpc_ortho), float64, step for step:
the cell's height, TM inverse and direct RPC into the view, the bounds test, the occlusion march through the render's surface
(dsm_render_oracle.surface / G) and the image bilinear.  Vectorised over cells.

The state does not depend on where a lane stops marching, so the oracle evaluates every sample h_1 .. h_K of a cell.  ortho()
also returns what the tests reason with: per cell the deciding f - occ_tol (of the defined sample with the smallest
|f - occ_tol|: a sign that device and numpy arithmetic may round differently), u and v (a bounds test that may flip), K and
the range of the four taps per channel."""
import numpy as np

import dsm_oracle
import dsm_render_oracle as ro
from satmvs_amd import rpc_synth

NO_HEIGHT, OUTSIDE, OCCLUDED, VISIBLE = 0, 1, 2, 3


def h_top(dsm, nodata):
    return ro.h_range(dsm, nodata)[1]


def bilinear(image, u, v):
    """Values (n, C) float32 and tap ranges (n, C) float64 of an (H, W, C) float32 image at in-bounds (u, v) (n,)."""
    img = np.asarray(image, np.float32)
    H, W, _ = img.shape
    if W > 1:
        c0 = np.minimum(np.floor(u), W - 2).astype(np.int64)
        c1, du = c0 + 1, u - c0
    else:
        c0 = c1 = np.zeros(u.shape, np.int64)
        du = np.zeros(u.shape)
    if H > 1:
        r0 = np.minimum(np.floor(v), H - 2).astype(np.int64)
        r1, dv = r0 + 1, v - r0
    else:
        r0 = r1 = np.zeros(v.shape, np.int64)
        dv = np.zeros(v.shape)
    p00, p01 = img[r0, c0].astype(np.float64), img[r0, c1].astype(np.float64)
    p10, p11 = img[r1, c0].astype(np.float64), img[r1, c1].astype(np.float64)
    du, dv = du[:, None], dv[:, None]
    a = p00 + du * (p01 - p00)
    b = p10 + du * (p11 - p10)
    taps = np.stack([p00, p01, p10, p11])
    return (a + dv * (b - a)).astype(np.float32), taps.max(axis=0) - taps.min(axis=0)


def ortho(dsm, grid, nodata, tm7, rpc, image=None, shape=None, x0=0, y0=0, h_hi=None, occlusion=True, occ_tol=0.5,
          rows=None, cols=None):
    """The orthophoto of one view at cells (rows, cols) (any equal shapes; default every cell).  image (H, W) or (H, W, C), or
    None with shape = (H, W) for the states alone.  -> dict with "state" uint8, "value" (..., C) float32 (NaN unless state 3),
    "tap_range" (..., C), "f_decide" (f - occ_tol, NaN where no sample was defined), "u", "v" (NaN where state 0), "K"."""
    z = np.asarray(dsm, np.float32)
    if rows is None:
        rows, cols = np.mgrid[0:grid.height, 0:grid.width]
    out_shape = np.shape(rows)
    r = np.asarray(rows, np.int64).reshape(-1)
    c = np.asarray(cols, np.int64).reshape(-1)
    if image is not None:
        image = np.asarray(image, np.float32)
        if image.ndim == 2:
            image = image[:, :, None]
        shape = image.shape[:2]
    H, W = shape
    C = image.shape[2] if image is not None else 1
    if h_hi is None:
        h_hi = h_top(z, nodata)
    n = r.size
    zc = z[r, c]
    state = np.zeros(n, np.uint8)
    value = np.full((n, C), np.nan, np.float32)
    trange = np.full((n, C), np.nan)
    fdec = np.full(n, np.nan)
    u, v = np.full(n, np.nan), np.full(n, np.nan)
    K = np.zeros(n, np.int64)
    # 1. height
    has = np.isfinite(zc) & (zc != np.float32(nodata))
    i = np.flatnonzero(has)
    # 2. projection
    E = grid.e0 + c[i].astype(np.float64) * grid.xres
    N = grid.n0 - r[i].astype(np.float64) * grid.yres
    lat, lon = dsm_oracle.tm_inverse(tm7, E, N)
    h = zc[i].astype(np.float64)
    x, y = rpc_synth.obj2photo(rpc, lat, lon, h)
    u[i], v[i] = x - x0, y - y0
    with np.errstate(invalid="ignore"):
        inside = (u[i] >= 0.0) & (u[i] <= W - 1) & (v[i] >= 0.0) & (v[i] <= H - 1)
    state[i] = np.where(inside, VISIBLE, OUTSIDE)
    # 3. occlusion: every sample h_1 .. h_K of every candidate
    if occlusion:
        m = inside & (h < h_hi)
        j, x, y, h = i[m], x[m], y[m], h[m]
        Ez, Nz = ro.G(rpc, tm7, x, y, h)
        Eh, Nh = ro.G(rpc, tm7, x, y, np.full(h.shape, h_hi))
        Kj = ro.march_steps(Eh, Nh, Ez, Nz, grid.xres, grid.yres)
        K[j] = Kj
        step = (h_hi - h) / Kj.astype(np.float64)
        occ = np.zeros(j.size, bool)
        best = np.full(j.size, np.nan)
        for k in range(1, int(Kj.max(initial=0)) + 1):
            a = np.flatnonzero(k <= Kj)
            hk = np.where(k == Kj[a], h_hi, h[a] + float(k) * step[a])
            e, nn = ro.G(rpc, tm7, x[a], y[a], hk)
            ok, S = ro.surface(z, grid.grid4(), nodata, e, nn)
            d = S - hk - occ_tol
            occ[a] |= ok & (d > 0.0)
            closer = ok & ~(np.abs(best[a]) <= np.abs(np.where(ok, d, np.inf)))
            best[a[closer]] = d[closer]
        state[j[occ]] = OCCLUDED
        fdec[j] = best
    # 4. visible: the image bilinear
    vis = np.flatnonzero(state == VISIBLE)
    if image is not None and vis.size:
        value[vis], trange[vis] = bilinear(image, u[vis], v[vis])
    return {"state": state.reshape(out_shape), "value": value.reshape(out_shape + (C,)),
            "tap_range": trange.reshape(out_shape + (C,)), "f_decide": fdec.reshape(out_shape), "u": u.reshape(out_shape),
            "v": v.reshape(out_shape), "K": K.reshape(out_shape)}


def borderline(o, shape, f_eps=1e-6, uv_eps=1e-9):
    """Cells whose state device and numpy arithmetic may decide differently: |f - occ_tol| < f_eps, or u / v within uv_eps px of
    an image border."""
    H, W = shape
    u, v = o["u"], o["v"]
    with np.errstate(invalid="ignore"):
        near = (np.abs(u) < uv_eps) | (np.abs(u - (W - 1)) < uv_eps) | (np.abs(v) < uv_eps) | (np.abs(v - (H - 1)) < uv_eps)
        return (np.abs(o["f_decide"]) < f_eps) | near
