"""The numpy statements of the viewshed rule (include/satmvs.h, "Viewshed"), stated twice: a loop over pairs in Python ints
with fractions.Fraction for M (`line`, `viewshed_loop`), and arrays -- all lines of a call at once, stepping i, int64
cross-multiplication (`lines`, `viewshed`, `los`).  numpy, math and fractions only.  `plant` puts a known mistake into the
array statement (tests/test_dsm_viewshed_cpu.py)."""
import math
from fractions import Fraction

import numpy as np

MAX_Z = np.float32(32768.0)
MAX_UNITS = 1 << 23
PLANTS = ("rint", "half down", "strict", "voids occlude", "ends occlude", "no target drop", "drop added", "float quotients")


def valid(z, nodata):
    z = np.asarray(z, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(z) & (z != np.float32(nodata)) & (np.abs(z) <= MAX_Z)


def heights(z, nodata):
    """(ok, q): q = rint(256 (double)z), halves to even, 0 at invalid cells."""
    ok = valid(z, nodata)
    return ok, np.rint(np.where(ok, z, np.float32(0.0)).astype(np.float64) * 256.0).astype(np.int64)


def terms(grid, curvature=True, refraction=0.13, earth_radius=6371008.8, max_distance=None):
    """dsm.viewshed_terms, restated: (xres, yres, c256, r2max)."""
    c256 = 256.0 * (1.0 - refraction) / (2.0 * earth_radius) if curvature else 0.0
    return float(grid.xres), float(grid.yres), c256, math.inf if max_distance is None else float(max_distance) * float(max_distance)


def units(h):
    """A height [m] in units of 2^-8 m, as the Python layer takes it."""
    return int(np.rint(256.0 * float(h)))


def dist2(t, dc, dr):
    """((double)dc xres) ((double)dc xres) + ((double)dr yres) ((double)dr yres), every operation rounded by itself."""
    x, y = np.asarray(dc, np.float64) * np.float64(t[0]), np.asarray(dr, np.float64) * np.float64(t[1])
    return x * x + y * y


def drop(t, dc, dr):
    return np.rint(np.float64(t[2]) * dist2(t, dc, dr)).astype(np.int64)


def minor(i, dm, n):
    """floor((2 i dm + n) / (2 n)): Python's and numpy's // are floor divisions."""
    return (2 * i * dm + n) // (2 * n)


def above_of(code, need, nodata):
    """The float32 `above` of codes and needs: +0.0 seen, (float)((double)need / 256.0) hidden, (float)nodata otherwise."""
    code, need = np.asarray(code), np.asarray(need, np.int64)
    out = np.full(code.shape, np.float32(nodata), np.float32)
    out[code == 1] = np.float32(0.0)
    out[code == 2] = (need[code == 2].astype(np.float64) / 256.0).astype(np.float32)
    return out


# ---- the rule as a loop over pairs ---------------------------------------------------------------------------------------------
def _dist2_py(t, dc, dr):
    x, y = float(dc) * t[0], float(dr) * t[1]                 # Python floats are IEEE doubles, every operation rounded by itself
    return x * x + y * y


def _drop_py(t, dc, dr):
    return round(t[2] * _dist2_py(t, dc, dr))                 # round() of a float goes to even at halves


def line(ok, q, t, co, ro, eye, mode, ct, rt, tgt):
    """One line of sight in Python ints -> (code, need): need is None unless the target is valid and in range, and -inf
    (float) with no valid intermediate sample."""
    gh, gw = q.shape
    if not (0 <= co < gw and 0 <= ro < gh and 0 <= ct < gw and 0 <= rt < gh and mode in (0, 1)):
        return 0, None
    if not ((-MAX_UNITS if mode else 0) <= eye <= MAX_UNITS and 0 <= tgt <= MAX_UNITS):
        return 0, None
    if (mode == 0 and not ok[ro, co]) or not ok[rt, ct]:
        return 0, None
    E = eye if mode == 1 else int(q[ro, co]) + eye
    dx, dy = ct - co, rt - ro
    if not _dist2_py(t, dx, dy) <= t[3]:
        return 3, None
    n = max(abs(dx), abs(dy))
    rows = abs(dy) >= abs(dx)
    dm = dx if rows else dy
    sg = (1 if dy > 0 else -1) if rows else (1 if dx > 0 else -1)
    M = None
    for i in range(1, n):
        m = minor(i, dm, n)
        dc, dr = (m, i * sg) if rows else (i * sg, m)
        if ok[ro + dr, co + dc]:
            slope = Fraction((int(q[ro + dr, co + dc]) - _drop_py(t, dc, dr) - E) * n, i)
            M = slope if M is None or slope > M else M
    if M is None:
        return 1, -math.inf
    need = math.ceil(M) - (int(q[rt, ct]) - _drop_py(t, dx, dy) - E)
    return (1 if need <= tgt else 2), need


def viewshed_loop(z, nodata, t, obs):
    """One observer (col, row, eye, mode, tgt), for tiny grids -> (seen, above, status)."""
    ok, q = heights(z, nodata)
    gh, gw = q.shape
    code, need = np.zeros((gh, gw), np.uint8), np.zeros((gh, gw), np.int64)
    for r in range(gh):
        for c in range(gw):
            k, nd = line(ok, q, t, obs[0], obs[1], obs[2], obs[3], c, r, obs[4])
            code[r, c] = k
            need[r, c] = nd if k == 2 else 0
    return code, above_of(code, need, nodata), int(obs[3] == 1 or bool(ok[obs[1], obs[0]]))


# ---- the rule on arrays ----------------------------------------------------------------------------------------------------------
def _float_slope(num, den):
    """A float32 quotient formed with a reciprocal: what an inexact kernel would compare."""
    return np.asarray(num).astype(np.float32) * (np.float32(1.0) / np.asarray(den).astype(np.float32))


def lines(ok, q, t, co, ro, eye, mode, ct, rt, tgt, plant=None):
    """All lines at once; every argument after t is an int64 array of one length (or a number) -> (code uint8, need int64,
    0 where the code is not 2)."""
    gh, gw = q.shape
    co, ro, eye, mode, ct, rt, tgt = np.broadcast_arrays(*[np.asarray(a, np.int64) for a in (co, ro, eye, mode, ct, rt, tgt)])
    fields = ((co >= 0) & (co < gw) & (ro >= 0) & (ro < gh) & (ct >= 0) & (ct < gw) & (rt >= 0) & (rt < gh) & ((mode == 0) | (mode == 1)) &
              (eye <= MAX_UNITS) & (eye >= np.where(mode == 0, 0, -MAX_UNITS)) & (tgt >= 0) & (tgt <= MAX_UNITS))
    co, ro, ct, rt = (np.where(fields, a, 0) for a in (co, ro, ct, rt))
    live = fields & ((mode == 1) | ok[ro, co]) & ok[rt, ct]
    E = np.where(mode == 1, eye, q[ro, co] + eye)
    dx, dy = ct - co, rt - ro
    rows = np.abs(dy) >= np.abs(dx)
    n, dm = np.where(rows, np.abs(dy), np.abs(dx)), np.where(rows, dx, dy)
    sg = np.where(np.where(rows, dy, dx) < 0, -1, 1)
    near = dist2(t, dx, dy) <= t[3]
    sign = 1 if plant == "drop added" else -1
    top = q[rt, ct] + (0 if plant == "no target drop" else sign * drop(t, dx, dy)) + tgt - E
    act = live & near
    best_num, best_i = np.zeros(n.shape, np.int64), np.zeros(n.shape, np.int64)
    blocked = np.zeros(n.shape, bool)                         # the plants that cannot be said as a pair
    first, last = (0, 1) if plant == "ends occlude" else (1, 0)
    for i in range(first, int(n[act].max()) + last if act.any() else 0):
        k = np.nonzero(act & (n + last > i) & (n > 0))[0]
        if plant == "rint":
            m = np.rint(i * dm[k] / n[k]).astype(np.int64)
        elif plant == "half down":
            m = -((n[k] - 2 * i * dm[k]) // (2 * n[k]))
        else:
            m = minor(i, dm[k], n[k])
        dc, dr = np.where(rows[k], m, i * sg[k]), np.where(rows[k], i * sg[k], m)
        r, c = ro[k] + dr, co[k] + dc
        num = q[r, c] + sign * drop(t, dc, dr) - E[k]
        v = ok[r, c]
        if plant == "voids occlude":
            num, v = np.where(v, num, MAX_UNITS - E[k]), np.ones_like(v)
        if i == 0:                                            # "ends occlude": the observer's cell stands at distance 0
            blocked[k[v & (num > 0)]] = True
            continue
        if plant == "float quotients":
            better = v & ((best_i[k] == 0) | (_float_slope(num, i) > _float_slope(best_num[k], np.maximum(best_i[k], 1))))
        else:
            better = v & ((best_i[k] == 0) | (num * best_i[k] > best_num[k] * i))
        best_num[k[better]], best_i[k[better]] = num[better], i
    some = act & (best_i > 0)
    if plant == "strict":
        hidden = some & (best_num * n >= top * best_i)
    elif plant == "float quotients":
        hidden = some & (_float_slope(best_num, np.maximum(best_i, 1)) > _float_slope(top, np.maximum(n, 1)))
    else:
        hidden = some & (best_num * n > top * best_i)
    hidden |= act & blocked
    ceil = -((-best_num * n) // np.maximum(best_i, 1))
    code = np.where(hidden, 2, np.where(act, 1, np.where(live, 3, 0))).astype(np.uint8)
    return code, np.where(hidden, ceil - (top - tgt), 0)


def viewshed(z, nodata, t, observers, plant=None):
    """smvs_dsm_viewshed: observers is a list of (col, row, eye, mode, tgt) -> (seen (m, gh, gw) uint8, above (m, gh, gw)
    float32, status (m) int32)."""
    ok, q = heights(z, nodata)
    gh, gw = q.shape
    rt, ct = (a.ravel() for a in np.mgrid[0:gh, 0:gw])
    seen, above, status = [], [], []
    for col, row, eye, mode, tgt in observers:
        code, need = lines(ok, q, t, col, row, eye, mode, ct, rt, tgt, plant)
        seen.append(code.reshape(gh, gw))
        above.append(above_of(code, need, nodata).reshape(gh, gw))
        status.append(int(mode == 1 or bool(ok[row, col])))
    return np.stack(seen), np.stack(above), np.array(status, np.int32)


def los(z, nodata, t, pairs, plant=None):
    """smvs_dsm_los: pairs (n, 7) of (col_o, row_o, eye, mode, col_t, row_t, tgt) -> (seen (n) uint8, above (n) float32)."""
    ok, q = heights(z, nodata)
    p = np.asarray(pairs, np.int64).reshape(-1, 7)
    code, need = lines(ok, q, t, p[:, 0], p[:, 1], p[:, 2], p[:, 3], p[:, 4], p[:, 5], p[:, 6], plant)
    return code, above_of(code, need, nodata)


def needs(z, nodata, t, obs):
    """(code, need) grids of one observer: need in units at hidden cells, 0 elsewhere."""
    ok, q = heights(z, nodata)
    gh, gw = q.shape
    rt, ct = (a.ravel() for a in np.mgrid[0:gh, 0:gw])
    code, need = lines(ok, q, t, obs[0], obs[1], obs[2], obs[3], ct, rt, obs[4])
    return code.reshape(gh, gw), need.reshape(gh, gw)


def visibility_count(seen):
    return (np.asarray(seen) == 1).sum(axis=0).astype(np.int32)
