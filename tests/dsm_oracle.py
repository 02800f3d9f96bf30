"""Test-local numpy oracle of DSM production: the Transverse Mercator series in the operation order of the reference's numpy
code (pinned against tests/golden/tm.npz), the bin rule and a per-cell reduce by np.lexsort."""
import numpy as np

from dsm_testkit import f2key as keys  # noqa: F401  (re-exported)

PI = 3.14159265358979323846


def _consts(tm7):
    a, inv_f, lat0, lon0, k0, fe, fn = [float(v) for v in tm7]
    f = 1.0 / inv_f
    e = np.sqrt(2 * f - f * f)
    e2 = e * e
    e4, e6 = e2 * e2, e2 * e2 * e2
    sec_e = np.sqrt((e * e) / (1 - e * e))
    m = (1 - e2 / 4 - 3 * e4 / 64 - 5 * e6 / 256, 3 * e2 / 8 + 3 * e4 / 32 + 45 * e6 / 1024, 15 * e4 / 256 + 45 * e6 / 1024,
         35 * e6 / 3072)
    phi0, lam0 = lat0 / 180 * PI, lon0 / 180 * PI
    m0 = a * (m[0] * phi0 - m[1] * np.sin(2 * phi0) + m[2] * np.sin(4 * phi0) - m[3] * np.sin(6 * phi0))
    return dict(a=a, e=e, e2=e2, sec_e=sec_e, m=m, m0=m0, lam0=lam0, k0=k0, fe=fe, fn=fn)


def tm_forward(tm7, lat, lon):
    c = _consts(tm7)
    phi, lam = np.asarray(lat, np.float64) / 180 * PI, np.asarray(lon, np.float64) / 180 * PI
    e2, se, a, m = c["e2"], c["sec_e"], c["a"], c["m"]
    cp, sp, tp = np.cos(phi), np.sin(phi), np.tan(phi)
    T = tp * tp
    C = e2 * cp * cp / (1 - e2)
    A = (lam - c["lam0"]) * cp
    nu = a / np.sqrt(1 - e2 * sp * sp)
    M = a * (m[0] * phi - m[1] * np.sin(2 * phi) + m[2] * np.sin(4 * phi) - m[3] * np.sin(6 * phi))
    A2, A3 = A * A, A * A * A
    E = c["fe"] + c["k0"] * nu * (A + (1 - T + C) * A3 / 6 + (5 - 18 * T + T * T + 72 * C - 58 * se * se) * A2 * A3 / 120)
    N = c["fn"] + c["k0"] * (M - c["m0"] + nu * tp * (A2 / 2 + (5 - T + 9 * C + 4 * C * C) * A2 * A2 / 24 +
                                                       (61 - 58 * T + T * T + 600 * C - 330 * se * se) * A3 * A3 / 720))
    return E, N


def tm_inverse(tm7, E, N):
    c = _consts(tm7)
    e, e2, a, m, k0 = c["e"], c["e2"], c["a"], c["m"], c["k0"]
    E, N = np.asarray(E, np.float64), np.asarray(N, np.float64)
    r = np.sqrt(1 - e * e)
    e1 = (1 - r) / (1 + r)
    e1s = e1 * e1
    mu = (c["m0"] + (N - c["fn"]) / k0) / (a * m[0])
    phi1 = (mu + (3 * e1 / 2 - 27 * e1s * e1 / 32) * np.sin(2 * mu) + (21 * e1s / 16 - 55 * e1s * e1s / 32) * np.sin(4 * mu)
            + (151 * e1s * e1 / 96) * np.sin(6 * mu) + (1097 * e1s * e1s / 512) * np.sin(8 * mu))
    q = np.sqrt(1 - e2 * np.sin(phi1) * np.sin(phi1))
    nu1 = a / q
    rho1 = a * (1 - e2) / (q * q * q)
    T1 = np.tan(phi1) * np.tan(phi1)
    C1 = c["sec_e"] * np.cos(phi1)
    C1 = C1 * C1
    D = (E - c["fe"]) / (nu1 * k0)
    D2, D3 = D * D, D * D * D
    s2 = c["sec_e"] * c["sec_e"]
    phi = phi1 - (nu1 * np.tan(phi1) / rho1) * (D2 / 2 - (5 + 3 * T1 + 10 * C1 - 4 * C1 * C1 - 9 * s2) * D2 * D2 / 24 +
                                               (61 + 90 * T1 + 298 * C1 + 45 * T1 * T1 - 252 * s2 - 3 * C1 * C1) * D3 * D3 / 720)
    lam = c["lam0"] + (D - (1 + 2 * T1 + C1) * D3 / 6 +
                       (5 - 2 * C1 + 28 * T1 - 3 * C1 * C1 + 8 * s2 + 24 * T1 * T1) * D2 * D3 / 120) / np.cos(phi1)
    return phi * 180 / PI, lam * 180 / PI


def cells(east, north, grid4, gw, gh):
    """The bin rule on given E / N: row * gw + col, or -1 off the grid / non-finite."""
    e0, n0, xr, yr = [float(v) for v in grid4]
    with np.errstate(invalid="ignore"):
        col = np.floor((east - e0) / xr + 0.5)
        row = np.floor((n0 - north) / yr + 0.5)
        ok = (col >= 0) & (col < gw) & (row >= 0) & (row < gh)
    out = np.full(np.shape(east), -1, np.int64)
    out[ok] = (row[ok].astype(np.int64) * gw + col[ok].astype(np.int64))
    return out


def reduce(cell, height, ncells, mode, nodata):
    """Per-cell median / mean / min / max of the heights sorted on their uint32 keys; empty cells -> nodata.  float32."""
    cell = np.asarray(cell).reshape(-1)
    height = np.asarray(height, np.float32).reshape(-1)
    ok = (cell >= 0) & (cell < ncells)
    c, h = cell[ok], height[ok]
    order = np.lexsort((keys(h), c))
    c, h = c[order], h[order]
    out = np.full(ncells, np.float32(nodata), np.float32)
    count = np.bincount(c, minlength=ncells)
    starts = np.concatenate([[0], np.cumsum(count)])
    for cc in np.nonzero(count)[0]:
        v = h[starts[cc]:starts[cc + 1]]
        n = v.size
        if mode == "min":
            out[cc] = v[0]
        elif mode == "max":
            out[cc] = v[-1]
        elif mode == "mean":
            out[cc] = np.float32(v.astype(np.float64).sum() / n)
        elif n % 2:
            out[cc] = v[n // 2]
        else:
            out[cc] = np.float32(0.5 * (np.float64(v[n // 2 - 1]) + np.float64(v[n // 2])))
    return out, count
