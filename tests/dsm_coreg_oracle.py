"""Numpy statements of the registration rules (include/satmvs.h, "Registration"): the shift statistics and the regrid twice
each, once vectorised and once as a loop over cells with Python-integer sums and Python float64 arithmetic, and the selection
rule of coregister over exact fractions.  Nothing here imports satmvs_amd or torch."""
import math
from fractions import Fraction

import numpy as np

from dsm_testkit import valid


# ---- shift statistics ----------------------------------------------------------------------------------------------------------
def shift_stats(a, b, ox=0, oy=0, radius=8, dz0=0.0, trim=256.0, nodata=-999.0):
    """One vectorised pass per shift -> (2R + 1, 2R + 1, 3) int64."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    (gha, gwa), (ghb, gwb) = a.shape, b.shape
    S = 2 * radius + 1
    out = np.zeros((S, S, 3), np.int64)
    vb = valid(b, nodata)
    b64 = b.astype(np.float64)
    for sy in range(-radius, radius + 1):
        r0, r1 = max(0, -(oy + sy)), min(ghb, gha - (oy + sy))            # rows of b whose partner is on a
        if r1 <= r0:
            continue
        for sx in range(-radius, radius + 1):
            c0, c1 = max(0, -(ox + sx)), min(gwb, gwa - (ox + sx))
            if c1 <= c0:
                continue
            pa = a[r0 + oy + sy:r1 + oy + sy, c0 + ox + sx:c1 + ox + sx]
            ok = valid(pa, nodata) & vb[r0:r1, c0:c1]
            with np.errstate(invalid="ignore", over="ignore"):
                d = (pa.astype(np.float64) - b64[r0:r1, c0:c1]) - np.float64(dz0)
                ok &= np.abs(d) <= np.float64(trim)
            q = np.rint(d[ok] * 256.0).astype(np.int64)
            out[sy + radius, sx + radius] = (q.size, q.sum(), (q * q).sum())
    return out


def shift_stats_loop(a, b, ox=0, oy=0, radius=8, dz0=0.0, trim=256.0, nodata=-999.0):
    """The same rules cell by cell: Python floats (IEEE float64) and Python integers."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    (gha, gwa), (ghb, gwb) = a.shape, b.shape
    nd = float(np.float32(nodata))
    S = 2 * radius + 1
    out = [[[0, 0, 0] for _ in range(S)] for _ in range(S)]
    for r in range(ghb):
        for c in range(gwb):
            zb = float(b[r, c])
            if not math.isfinite(zb) or zb == nd:
                continue
            for sy in range(-radius, radius + 1):
                ra = r + oy + sy
                if not 0 <= ra < gha:
                    continue
                for sx in range(-radius, radius + 1):
                    ca = c + ox + sx
                    if not 0 <= ca < gwa:
                        continue
                    za = float(a[ra, ca])
                    if not math.isfinite(za) or za == nd:
                        continue
                    d = (za - zb) - float(dz0)
                    if not abs(d) <= float(trim):
                        continue
                    q = round(d * 256.0)                     # Python's round: halves to even, exact on a float
                    cell = out[sy + radius][sx + radius]
                    cell[0] += 1
                    cell[1] += q
                    cell[2] += q * q
    return np.array(out, dtype=np.int64).reshape(S, S, 3)


# ---- regrid --------------------------------------------------------------------------------------------------------------------
def regrid(src, gs, gd, mode="bilinear", dz=0.0, nodata=-999.0):
    """Vectorised.  gs, gd: objects with e0, n0, xres, yres, width, height.  -> (gd.height, gd.width) float32."""
    src = np.asarray(src, np.float32)
    ghs, gws = src.shape
    nd = np.float32(nodata)
    r, c = np.mgrid[0:gd.height, 0:gd.width].astype(np.float64)
    E = np.float64(gd.e0) + c * np.float64(gd.xres)
    N = np.float64(gd.n0) - r * np.float64(gd.yres)
    u = (E - np.float64(gs.e0)) / np.float64(gs.xres)
    v = (np.float64(gs.n0) - N) / np.float64(gs.yres)
    if mode == "nearest":
        i, j = np.floor(u + 0.5), np.floor(v + 0.5)
        wx = [np.ones_like(u), np.zeros_like(u)]
        wy = [np.ones_like(u), np.zeros_like(u)]
    else:
        i, j = np.floor(u), np.floor(v)
        wx = [None, u - i]
        wx[0] = 1.0 - wx[1]
        wy = [None, v - j]
        wy[0] = 1.0 - wy[1]
    ok = np.ones(u.shape, bool)
    z = [[None, None], [None, None]]
    for dj in (0, 1):
        for di in (0, 1):
            read = (wx[di] != 0.0) & (wy[dj] != 0.0)
            row, col = j + dj, i + di
            on = (row >= 0) & (row < ghs) & (col >= 0) & (col < gws)
            t = np.zeros(u.shape, np.float32)
            at = read & on
            t[at] = src[row[at].astype(np.int64), col[at].astype(np.int64)]
            ok &= ~read | (on & valid(t, nodata))
            z[dj][di] = np.where(at, t, np.float32(0.0)).astype(np.float32)
    z64 = [[z[dj][di].astype(np.float64) for di in (0, 1)] for dj in (0, 1)]
    with np.errstate(invalid="ignore", over="ignore"):
        top = wx[0] * z64[0][0] + wx[1] * z64[0][1]
        bottom = wx[0] * z64[1][0] + wx[1] * z64[1][1]
        blend = (wy[0] * top + wy[1] * bottom + np.float64(dz)).astype(np.float32)
    one_x = ((wx[0] == 1.0) & (wx[1] == 0.0)) | ((wx[0] == 0.0) & (wx[1] == 1.0))
    one_y = ((wy[0] == 1.0) & (wy[1] == 0.0)) | ((wy[0] == 0.0) & (wy[1] == 1.0))
    tap = np.where(wy[0] == 1.0, np.where(wx[0] == 1.0, z[0][0], z[0][1]), np.where(wx[0] == 1.0, z[1][0], z[1][1])).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        single = tap if dz == 0.0 else (tap.astype(np.float64) + np.float64(dz)).astype(np.float32)
    out = np.where(one_x & one_y, single, blend).astype(np.float32)
    out[~ok] = nd
    return out


def regrid_loop(src, gs, gd, mode="bilinear", dz=0.0, nodata=-999.0):
    """The same rules cell by cell in Python floats."""
    src = np.asarray(src, np.float32)
    ghs, gws = src.shape
    nd = float(np.float32(nodata))
    out = np.empty((gd.height, gd.width), np.float32)
    for r in range(gd.height):
        for c in range(gd.width):
            E, N = float(gd.e0) + c * float(gd.xres), float(gd.n0) - r * float(gd.yres)
            u, v = (E - float(gs.e0)) / float(gs.xres), (float(gs.n0) - N) / float(gs.yres)
            if mode == "nearest":
                i, j, wx, wy = math.floor(u + 0.5), math.floor(v + 0.5), (1.0, 0.0), (1.0, 0.0)
            else:
                i, j = math.floor(u), math.floor(v)
                wx, wy = (1.0 - (u - i), u - i), (1.0 - (v - j), v - j)
            taps, good = {}, True
            for dj in (0, 1):
                for di in (0, 1):
                    taps[dj, di] = np.float32(0.0)
                    if wx[di] == 0.0 or wy[dj] == 0.0:
                        continue
                    if not (0 <= j + dj < ghs and 0 <= i + di < gws):
                        good = False
                        continue
                    t = src[j + dj, i + di]
                    if not math.isfinite(float(t)) or float(t) == nd:
                        good = False
                    taps[dj, di] = t
            if not good:
                out[r, c] = np.float32(nodata)
                continue
            if sorted(wx) == [0.0, 1.0] and sorted(wy) == [0.0, 1.0]:
                t = taps[wy.index(1.0), wx.index(1.0)]
                out[r, c] = t if dz == 0.0 else np.float32(float(t) + float(dz))
            else:
                top = wx[0] * float(taps[0, 0]) + wx[1] * float(taps[0, 1])
                bottom = wx[0] * float(taps[1, 0]) + wx[1] * float(taps[1, 1])
                with np.errstate(over="ignore"):
                    out[r, c] = np.float32(wy[0] * top + wy[1] * bottom + float(dz))
    return out


# ---- the selection rule --------------------------------------------------------------------------------------------------------
def best_shift(stats, min_overlap=0.5):
    """The rule of satmvs_amd.dsm.best_shift over exact fractions: -> None, or (sx, sy, dx, dy, n, sum_q)."""
    st = np.asarray(stats)
    R = st.shape[0] // 2
    n = {(sx, sy): int(st[sy + R, sx + R, 0]) for sy in range(-R, R + 1) for sx in range(-R, R + 1)}
    need = max(2, math.ceil(min_overlap * max(n.values())))
    var = {}
    for (sx, sy), k in n.items():
        if k >= need:
            s1, s2 = int(st[sy + R, sx + R, 1]), int(st[sy + R, sx + R, 2])
            var[sx, sy] = Fraction(k * s2 - s1 * s1, k * k)
    if not var:
        return None
    sx, sy = min(var, key=lambda s: (var[s], s[0] ** 2 + s[1] ** 2, s[1], s[0]))

    def vertex(lo, hi):
        if lo not in var or hi not in var:
            return 0.0
        c0, cl, ch = (float(x.numerator) / float(x.denominator) for x in (var[sx, sy], var[lo], var[hi]))
        bend = cl - 2.0 * c0 + ch
        return min(0.5, max(-0.5, 0.5 * (cl - ch) / bend)) if bend > 0.0 else 0.0

    return (sx, sy, vertex((sx - 1, sy), (sx + 1, sy)), vertex((sx, sy - 1), (sx, sy + 1)), n[sx, sy], int(st[sy + R, sx + R, 1]))


def best_shift_float(stats, min_overlap=0.5):
    """The argmin as a float64 user would write it (Var = E[q^2] - E[q]^2): what the exact rule is held against."""
    st = np.asarray(stats).astype(np.float64)
    R = st.shape[0] // 2
    n = st[..., 0]
    need = max(2.0, math.ceil(min_overlap * n.max()))
    with np.errstate(invalid="ignore", divide="ignore"):
        var = st[..., 2] / n - (st[..., 1] / n) ** 2
    var[n < need] = np.inf
    sy, sx = np.unravel_index(np.argmin(var), var.shape)
    return int(sx) - R, int(sy) - R, var
