// dsm_geo.h -- the geometry that DSM production (dsm.hip) and DSM rendering (dsm_render.hip) share: the
// Transverse Mercator projection, the georeference of a grid, the bilinear surface of a DSM with the step counts of a ray march
// through it, and the host-side parsing of the arguments that carry them (tm7, grid4, a view's tile).
#pragma once
#include <limits.h>
#include <math.h>

#include "dsm_common.h"

namespace smvs {

// ---- Transverse Mercator ---------------------------------------------------------------------------------------------------
// Constants of one projection, derived once on the host (IEEE float64, no contraction) in the operation order of the reference's
// numpy code, so host-side mirrors reproduce the same bits.
struct TmConst {
    double a, e2, sec_e, sece2, k0, fe, fn, lat0, lon0;
    double m1, m2, m3, m4, m0;          // meridional arc: M = a (m1 phi - m2 sin 2phi + m3 sin 4phi - m4 sin 6phi)
    double e1, f1, f2, f3, f4;          // footpoint latitude series of the inverse
};

static const double TM_PI = 3.14159265358979323846;

static bool tm_setup(const double* tm7, TmConst& t)
{
    const double a = tm7[0], inv_f = tm7[1];
    if (!(a > 0.0) || !(inv_f > 1.0) || !(tm7[4] > 0.0) || !isfinite(a) || !isfinite(inv_f)) return false;
    for (int i = 2; i < 7; ++i)
        if (!isfinite(tm7[i])) return false;
    const double f = 1.0 / inv_f;
    const double e = sqrt(2 * f - f * f);
    t.a = a;
    t.e2 = e * e;
    t.sec_e = sqrt((e * e) / (1 - e * e));
    t.sece2 = t.sec_e * t.sec_e;
    t.lat0 = tm7[2] / 180 * TM_PI;
    t.lon0 = tm7[3] / 180 * TM_PI;
    t.k0 = tm7[4];
    t.fe = tm7[5];
    t.fn = tm7[6];
    const double e2 = t.e2, e4 = e2 * e2, e6 = e2 * e2 * e2;
    t.m1 = 1 - e2 / 4 - 3 * e4 / 64 - 5 * e6 / 256;
    t.m2 = 3 * e2 / 8 + 3 * e4 / 32 + 45 * e6 / 1024;
    t.m3 = 15 * e4 / 256 + 45 * e6 / 1024;
    t.m4 = 35 * e6 / 3072;
    t.m0 = a * (t.m1 * t.lat0 - t.m2 * sin(2 * t.lat0) + t.m3 * sin(4 * t.lat0) - t.m4 * sin(6 * t.lat0));
    const double r = sqrt(1 - e * e);
    const double e1 = (1 - r) / (1 + r), e1s = e1 * e1;
    t.e1 = e1;
    t.f1 = 3 * e1 / 2 - 27 * e1s * e1 / 32;
    t.f2 = 21 * e1s / 16 - 55 * e1s * e1s / 32;
    t.f3 = 151 * e1s * e1 / 96;
    t.f4 = 1097 * e1s * e1s / 512;
    return true;
}

// (lat, lon) [deg] -> (E, N) [m]; Snyder (8-9), (8-10), (3-21), (4-20), (8-12..8-15).
__device__ __forceinline__ void tm_forward(const TmConst& t, double lat_deg, double lon_deg, double& E, double& N)
{
    const double phi = lat_deg / 180 * TM_PI, lam = lon_deg / 180 * TM_PI;
    double s, c;
    sincos(phi, &s, &c);
    const double tn = tan(phi);
    const double T = tn * tn;
    const double C = t.e2 * c * c / (1 - t.e2);
    const double A = (lam - t.lon0) * c;
    const double nu = t.a / sqrt(1 - t.e2 * s * s);
    const double M = t.a * (t.m1 * phi - t.m2 * sin(2 * phi) + t.m3 * sin(4 * phi) - t.m4 * sin(6 * phi));
    const double A2 = A * A, A3 = A * A * A;
    E = t.fe + t.k0 * nu * (A + (1 - T + C) * A3 / 6 + (5 - 18 * T + T * T + 72 * C - 58 * t.sec_e * t.sec_e) * A2 * A3 / 120);
    N = t.fn + t.k0 * (M - t.m0 + nu * tn * (A2 / 2 + (5 - T + 9 * C + 4 * C * C) * A2 * A2 / 24 +
                                              (61 - 58 * T + T * T + 600 * C - 330 * t.sec_e * t.sec_e) * A3 * A3 / 720));
}

// (E, N) [m] -> (lat, lon) [deg]; Snyder (8-20), (7-19), (3-26), (8-21..8-26).
__device__ __forceinline__ void tm_inverse(const TmConst& t, double E, double N, double& lat_deg, double& lon_deg)
{
    const double M1 = t.m0 + (N - t.fn) / t.k0;
    const double mu = M1 / (t.a * t.m1);
    const double phi1 = mu + t.f1 * sin(2 * mu) + t.f2 * sin(4 * mu) + t.f3 * sin(6 * mu) + t.f4 * sin(8 * mu);
    double s1, c1;
    sincos(phi1, &s1, &c1);
    const double tn1 = tan(phi1);
    const double q = sqrt(1 - t.e2 * s1 * s1);
    const double nu1 = t.a / q;
    const double rho1 = t.a * (1 - t.e2) / (q * q * q);
    const double T1 = tn1 * tn1;
    double C1 = t.sec_e * c1;
    C1 = C1 * C1;
    const double D = (E - t.fe) / (nu1 * t.k0);
    const double D2 = D * D, D3 = D2 * D;
    const double phi = phi1 - (nu1 * tn1 / rho1) * (D2 / 2 - (5 + 3 * T1 + 10 * C1 - 4 * C1 * C1 - 9 * t.sece2) * D2 * D2 / 24 +
                                                   (61 + 90 * T1 + 298 * C1 + 45 * T1 * T1 - 252 * t.sece2 - 3 * C1 * C1) * D3 * D3 / 720);
    const double lam = t.lon0 + (D - (1 + 2 * T1 + C1) * D3 / 6 +
                                 (5 - 2 * C1 + 28 * T1 - 3 * C1 * C1 + 8 * t.sece2 + 24 * T1 * T1) * D2 * D3 / 120) / c1;
    lat_deg = phi * 180 / TM_PI;
    lon_deg = lam * 180 / TM_PI;
}

// ---- the grid and its surface --------------------------------------------------------------------------------------------------
// Georeference of a DSM, world-file convention: (e0, n0) = centre of cell (0, 0), xres and yres the cell size.
struct DsmGrid { double e0, n0, xres, yres; };

constexpr int RENDER_MAX_STEPS = 4096, RENDER_MAX_BISECT = 60;

// S(E, N): bilinear over the cells floor(u) .. floor(u)+1 x floor(v) .. floor(v)+1, written as three lerps so that a flat patch
// gives its height exactly.  False where one of the four is off the grid, non-finite or nodata (never extrapolated).
__device__ __forceinline__ bool dsm_surface(const float* __restrict__ z, int gw, int gh, float nodata, const DsmGrid& g,
                                            double E, double N, double& S)
{
    const double u = (E - g.e0) / g.xres, v = (g.n0 - N) / g.yres;
    const double cu = floor(u), cv = floor(v);
    if (!(cu >= 0.0 && cu < (double)(gw - 1) && cv >= 0.0 && cv < (double)(gh - 1))) return false;    // NaN fails too
    const float* p = z + (size_t)(int)cv * gw + (int)cu;
    const float z00 = p[0], z01 = p[1], z10 = p[gw], z11 = p[gw + 1];
    if (!(dsm_cell_valid(z00, nodata) && dsm_cell_valid(z01, nodata) && dsm_cell_valid(z10, nodata) && dsm_cell_valid(z11, nodata)))
        return false;
    const double du = u - cu, dv = v - cv;
    const double a = (double)z00 + du * ((double)z01 - (double)z00);
    const double b = (double)z10 + du * ((double)z11 - (double)z10);
    S = a + dv * (b - a);
    return true;
}

// K = clamp(ceil(2 D), 1, RENDER_MAX_STEPS), D = the ray's travel in cells over [h_lo, h_hi] (NaN -> 1).
__device__ __forceinline__ int render_march_steps(const DsmGrid& g, double E_hi, double N_hi, double E_lo, double N_lo)
{
    const double dE = fabs(E_hi - E_lo) / g.xres, dN = fabs(N_hi - N_lo) / g.yres;
    const double c = ceil(2.0 * (dE > dN ? dE : dN));
    return c >= (double)RENDER_MAX_STEPS ? RENDER_MAX_STEPS : c >= 1.0 ? (int)c : 1;
}

// B = clamp(ceil(log2(dh / tol)), 0, RENDER_MAX_BISECT), exactly: the least b with dh * 2^-b <= tol (halving is exact).
__device__ __forceinline__ int render_bisect_steps(double dh, double tol)
{
    int b = 0;
    while (dh > tol && b < RENDER_MAX_BISECT) { dh *= 0.5; ++b; }
    return b;
}

// ---- host-side argument parsing: a message for fail(SMVS_ERR_ARG, "%s", ...) or nullptr, like grid_check -------------------------
static const char* tm_parse(const double* tm7, TmConst& t)
{
    return tm_setup(tm7, t) ? nullptr : "bad projection parameters (a > 0, inverse flattening > 1, k0 > 0, all finite)";
}

static const char* dsm_grid_parse(const double* grid4, DsmGrid& g)
{
    g = DsmGrid{grid4[0], grid4[1], grid4[2], grid4[3]};
    if (!isfinite(g.e0) || !isfinite(g.n0) || !(g.xres > 0.0) || !(g.yres > 0.0) || !isfinite(g.xres) || !isfinite(g.yres))
        return "bad grid: E0, N0 finite, xres and yres positive and finite";
    return nullptr;
}

// The tile [y0, y0 + H) x [x0, x0 + W) of a view, for an entry that also takes a gw x gh grid: the size of the grid is checked
// between the size of the tile and its origin, the order in which the render and the orthophoto have always reported them.
static const char* tile_check(int H, int W, int x0, int y0, int gw, int gh)
{
    if (H < 1 || W < 1) return "non-positive dimension";
    if ((long long)H * W >= (1ll << 31)) return "view too large: H * W must be below 2^31 pixels";
    if (const char* msg = grid_check(gw, gh)) return msg;
    if (x0 < 0 || y0 < 0) return "negative origin";
    if ((long long)x0 + W > INT_MAX || (long long)y0 + H > INT_MAX) return "origin + size does not fit in an int";
    return nullptr;
}

}  // namespace smvs
