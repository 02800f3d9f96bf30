"""The numpy statements of the horizon rule (include/satmvs.h, "Horizon"), stated twice: an O(n^2) search over pairs of cells
with fractions.Fraction, and the stack walk along every line (all lines of a direction at once, a numpy row at a time, int64
cross-multiplication); and the float64 statements of sky_view_factor, horizon_lit and the exposure sum.  numpy and fractions
only.  `plant` puts a known mistake into the walk (tests/test_dsm_horizon_cpu.py)."""
import math
from fractions import Fraction

import numpy as np

import dsm_sun_oracle as so

MAX_Z = np.float32(32768.0)
QNAN = np.array([0x7fc00000], np.uint32).view(np.float32)[0]


def valid(z, nodata):
    z = np.asarray(z, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(z) & (z != np.float32(nodata)) & (np.abs(z) <= MAX_Z)


def heights(z, nodata):
    """(ok, q): q = rint((double)z 256), halves to even, 0 at invalid cells."""
    ok = valid(z, nodata)
    return ok, np.rint(np.where(ok, z, np.float32(0.0)).astype(np.float64) * 256.0).astype(np.int64)


def positions(gh, gw, a, b):
    """P(r, c) = rint(a c + b r): two products and their sum, each rounded by itself, then the rint (halves to even)."""
    r, c = np.mgrid[0:gh, 0:gw].astype(np.float64)
    return np.rint(np.float64(a) * c + np.float64(b) * r).astype(np.int64)


def tangent(dq, dp):
    """(float)((double)dq / (double)dp)."""
    return (np.asarray(dq, np.int64).astype(np.float64) / np.asarray(dp, np.int64).astype(np.float64)).astype(np.float32)


# ---- the rule as a search over pairs --------------------------------------------------------------------------------------------
def horizon_brute(z, nodata, direction):
    """O(n^2), for tiny grids: every valid cell against every valid cell of its line that lies towards the azimuth, the
    slopes compared as exact rationals."""
    z = np.asarray(z, np.float32)
    gh, gw = z.shape
    ucol, urow, a, b = direction
    row_major, s, ascending = so.lines(gh, gw, ucol, urow)
    ok, q = heights(z, nodata)
    P = positions(gh, gw, a, b)
    out = np.full((gh, gw), QNAN, np.float32)
    cells = {}
    for r in range(gh):
        for c in range(gw):
            if ok[r, c]:
                line, pos = (c - int(s[r]), r) if row_major else (r - int(s[c]), c)
                cells.setdefault(line, []).append((pos if ascending else -pos, int(q[r, c]), int(P[r, c]), r, c))
    for members in cells.values():
        members.sort()
        for n, (_, qi, Pi, r, c) in enumerate(members):
            best = None
            for _, qj, Pj, _, _ in members[:n]:
                assert Pj - Pi > 0, "P must be strictly monotone along a line"
                f = Fraction(qj - qi, Pj - Pi)
                if best is None or f > best[0]:
                    best = (f, qj - qi, Pj - Pi)
            out[r, c] = -np.inf if best is None else tangent(best[1], best[2])
    return out


def _float_slope(dq, dp):
    return dq.astype(np.float32) * (np.float32(1.0) / dp.astype(np.float32))


# ---- the rule as a stack along every line ---------------------------------------------------------------------------------------
def _walk_rows(ok, q, P, s, ascending, plant):
    """The walk on a working grid (H rows along the scan, W columns): per line L = c - s(r) a stack of (q, P), every line of
    the grid advanced together one row at a time."""
    H, W = q.shape
    smax, smin = max(int(s.max()), 0), min(int(s.min()), 0)
    nl = W + smax - smin
    sq, sp = np.zeros((H + 1, nl), np.int64), np.zeros((H + 1, nl), np.int64)
    depth = np.zeros(nl, np.int64)
    out = np.full((H, W), QNAN, np.float32)
    for r in (range(H) if ascending else range(H - 1, -1, -1)):
        act = np.ones(W, bool) if plant == "invalid occlude" else ok[r]
        cols = np.nonzero(act)[0]
        if cols.size == 0:
            continue
        idx = cols - int(s[r]) + smax
        qi, Pi = q[r, cols], P[r, cols]
        while True:
            d = depth[idx]
            can = d >= 2
            if not can.any():
                break
            jt, ju = np.maximum(d - 1, 0), np.maximum(d - 2, 0)
            qt, Pt, qu, Pu = sq[jt, idx], sp[jt, idx], sq[ju, idx], sp[ju, idx]
            if plant == "float pop":                          # rounded float32 quotients (a product with the reciprocal) decide
                with np.errstate(divide="ignore", invalid="ignore"):
                    drop = (can & (_float_slope(qu - qi, Pu - Pi) >= _float_slope(qt - qi, Pt - Pi))).astype(np.int64)
            else:
                lhs, rhs = (qu - qi) * (Pt - Pi), (qt - qi) * (Pu - Pi)
                if plant == "keep ties":                      # not a mistake: the other tie policy, a tied top stays
                    drop = (can & (lhs > rhs)).astype(np.int64)
                elif plant == "strict":                       # pops on "greater" only, and a tie drops two
                    drop = np.where(can & (lhs > rhs), 1, np.where(can & (lhs == rhs), 2, 0))
                else:
                    drop = (can & (lhs >= rhs)).astype(np.int64)
            if not drop.any():
                break
            depth[idx] = d - drop
        d = depth[idx]
        has = d >= 1
        jt = np.maximum(d - 1, 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            T = np.where(has, tangent(sq[jt, idx] - qi, np.where(has, sp[jt, idx] - Pi, 1)), np.float32(-np.inf)).astype(np.float32)
        if plant == "inclusive":                              # the cell stands in its own way, at slope 0
            T = np.maximum(T, np.float32(0.0))
        keep = ok[r, cols]
        out[r, cols[keep]] = T[keep]
        sq[d, idx], sp[d, idx] = qi, Pi
        depth[idx] = d + 1
    return out


def horizon_walk(z, nodata, direction, plant=None):
    """The rule as the stack walk: pop the top while the slope from the cell to the element under it is >= the slope to the
    top (exact int64 cross-multiplication), read the tangent off the top, push the cell.  The column-major directions on the
    transposed grid with (ucol, urow) and (a, b) swapped."""
    z = np.asarray(z, np.float32)
    ucol, urow, a, b = direction
    if abs(urow) < abs(ucol):
        return np.ascontiguousarray(horizon_walk(np.ascontiguousarray(z.T), nodata, (urow, ucol, b, a), plant).T)
    gh, gw = z.shape
    _, s, ascending = so.lines(gh, gw, ucol, urow, "rint" if plant == "rint" else None)
    ok, q = heights(z, nodata)
    return _walk_rows(ok, q, positions(gh, gw, a, b), s, ascending, plant)


def horizon(z, nodata, directions, plant=None):
    """(K, gh, gw) float32: horizon_walk of every direction."""
    return np.stack([horizon_walk(z, nodata, d, plant) for d in directions])


def terms(grid, azimuth):
    """dsm.horizon_terms, restated: (ucol, urow, a, b)."""
    sA, cA = math.sin(math.radians(azimuth)), math.cos(math.radians(azimuth))
    return sA / grid.xres, -cA / grid.yres, 256.0 * grid.xres * sA, -256.0 * grid.yres * cA


# ---- what the Python layer builds on the maps -----------------------------------------------------------------------------------
def sky_view_factor(tan_h):
    """The float64 mean in list order of 1 / (1 + max(t, 0)^2); NaN at invalid cells."""
    t = np.asarray(tan_h, np.float32).astype(np.float64)
    total = np.zeros(t.shape[1:], np.float64)
    for k in range(t.shape[0]):
        x = np.where(t[k] > 0.0, t[k], 0.0)
        total = total + 1.0 / (1.0 + x * x)
    return np.where(np.isnan(t).any(axis=0), np.nan, total / float(t.shape[0]))


def bracket(azimuths, azimuth, interp="linear"):
    """[(index, weight)]: the listed azimuth itself (weight None) if the asked one is in the list modulo 360 or interp is
    "nearest" (then the one nearest around the circle, the earlier of two); else the listed ones below and above it around the
    circle with weights 1 - w and w."""
    mods = [a % 360.0 for a in azimuths]
    x = azimuth % 360.0
    for i, m in enumerate(mods):
        if m == x:
            return [(i, None)]
    if interp == "nearest":
        dist = [abs((m - x + 180.0) % 360.0 - 180.0) for m in mods]
        return [(int(np.argmin(dist)), None)]
    lo = hi = None
    for i, m in enumerate(mods):
        for cand in (m - 360.0, m, m + 360.0):
            if cand < x and (lo is None or cand > lo[0]):
                lo = (cand, i)
            if cand > x and (hi is None or cand < hi[0]):
                hi = (cand, i)
    w = (x - lo[0]) / (hi[0] - lo[0])
    return [(lo[1], 1.0 - w), (hi[1], w)]


def horizon_lit(tan_h, azimuths, azimuth, elevation, interp="linear"):
    """uint8: 0 invalid, 2 where T > tan(elevation), else 1; T as bracket() says, in float64."""
    t = np.asarray(tan_h, np.float32)
    pick = bracket(azimuths, azimuth, interp)
    with np.errstate(invalid="ignore"):
        if len(pick) == 1:
            T = t[pick[0][0]].astype(np.float64)
        else:
            (i, wi), (j, wj) = pick
            T = wi * t[i].astype(np.float64) + wj * t[j].astype(np.float64)
        code = np.where(T > math.tan(math.radians(elevation)), 2, 1).astype(np.uint8)
    return np.where(np.isnan(t[0]), 0, code).astype(np.uint8)


def exposure(tan_h, azimuths, suns, weights, dzde, dzdn, incidence=True, interp="linear"):
    """The float64 sum in list order of w lit (cos i or 1), lit from horizon_lit; NaN at invalid cells."""
    t = np.asarray(tan_h, np.float32)
    total = np.zeros(t.shape[1:], np.float64)
    for (az, el), w in zip(suns, weights):
        lit = horizon_lit(t, azimuths, az, el, interp) != 2
        total += np.where(lit, w * (so.cos_incidence(dzde, dzdn, az, el) if incidence else 1.0), 0.0)
    return np.where(np.isnan(t[0]), np.nan, total)
