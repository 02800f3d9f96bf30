// dsm_sun.hip -- the sun over a DSM ("Sun"; include/satmvs.h for the rules).
//
//   smvs_dsm_shadow    cast shadows: an exclusive running maximum of g = z - (a c + b r) along sheared lines towards the sun
//   smvs_dsm_gradient  Horn's 3 x 3 gradient, one lane per cell
//
// Shadow.  The kernels know one orientation, the row-major one: the scan runs along the rows of a (H, W) grid, the line of
// cell (r, c) is c - s(r), and a lane owns one line, so at row r a wave touches the consecutive columns L + s(r).  The
// column-major directions run the same kernels on the transposed grid with (ucol, urow) and (a, b) swapped -- the rule is
// symmetric under that swap because IEEE addition commutes -- between tile transposes through LDS (pitch 65: a column read
// of the tile walks the banks), so every global access of a wave is along a row in both orientations.
// The scan axis is cut into bands of SUN_BAND rows.  dsm_sun_shifts writes s(r) once (the one place the floor rule lives);
// dsm_sun_band_max takes, per (band, line), the maximum of g over the band's valid cells; dsm_sun_carry runs, per line, an
// exclusive scan of those maxima over the bands the line crosses, in sunward order, in place; dsm_sun_march walks every band
// from its carried maximum and writes shade and depth.  A band of B rows meets at most W + B lines (|m| <= 1), so the table is
// (bands, W + B + 1) and a line finds its slot in a band as L + (the band's largest s); the bands a line crosses are found by
// bisection in s, which is monotone.  The carry is exact, not a warm-up: shadows have no cap.
// Maxima are taken over the order-preserving int64 image of the doubles (-0.0 below +0.0), so the result does not depend on
// the order of the operands, zeros included: equal bits from run to run and to the numpy statement.  The float64 operations
// are __dmul_rn / __dadd_rn / __dsub_rn / __ddiv_rn, and the library is built with -ffp-contract=off besides.  No atomics,
// no host synchronisation; every kernel writes every element it owns.
#include <math.h>
#include <stdint.h>

#include "dsm_common.h"
#include "smvs_host.h"

namespace smvs {

constexpr int SUN_THREADS = 256;
constexpr int SUN_BAND = 32;                         // rows of a line that one lane scans
constexpr int SUN_TILE = 64, SUN_PITCH = SUN_TILE + 1;   // the transposes' tile and its odd pitch in LDS
constexpr double SUN_MAX_TERM = 0x1p900;             // |a|, |b| up to here keep g finite: |a c + b r| < 2^932

__device__ __forceinline__ long long d2key(double g)
{
    const long long u = __double_as_longlong(g);
    return u ^ ((u >> 63) & 0x7fffffffffffffffll);   // signed order = the doubles' order, -0.0 below +0.0
}

__device__ __forceinline__ double key2d(long long k) { return __longlong_as_double(k ^ ((k >> 63) & 0x7fffffffffffffffll)); }

__device__ __forceinline__ double sun_key(float z, double a, double b, int r, long long c)
{
    return __dsub_rn((double)z, __dadd_rn(__dmul_rn(a, (double)c), __dmul_rn(b, (double)r)));
}

// s(r) = floor(m r + 0.5)
__global__ __launch_bounds__(SUN_THREADS)
void dsm_sun_shifts(double m, int H, int* __restrict__ s)
{
    const unsigned r = blockIdx.x * (unsigned)SUN_THREADS + threadIdx.x;
    if (r < (unsigned)H) s[r] = (int)floor(__dadd_rn(__dmul_rn(m, (double)r), 0.5));
}

// blockIdx.x = band * nbx + (block of 256 slots); slot t of a band is the line L = t - (the band's largest s).
struct SunSlot { int r0, r1; long long L; size_t at; bool live; };

__device__ __forceinline__ SunSlot sun_slot(const int* __restrict__ s, int H, long long TS, unsigned nbx)
{
    SunSlot q;
    const unsigned band = blockIdx.x / nbx;
    const long long t = (long long)(blockIdx.x % nbx) * SUN_THREADS + threadIdx.x;
    q.r0 = (int)((long long)band * SUN_BAND);
    q.r1 = (int)min((long long)H, (long long)q.r0 + SUN_BAND);
    q.L = t - (long long)max(s[q.r0], s[q.r1 - 1]);
    q.at = (size_t)band * (size_t)TS + (size_t)t;
    q.live = t < TS;
    return q;
}

__global__ __launch_bounds__(SUN_THREADS)
void dsm_sun_band_max(const float* __restrict__ z, int W, int H, float nodata, double a, double b, const int* __restrict__ s,
                      long long TS, unsigned nbx, long long* __restrict__ M)
{
    const SunSlot q = sun_slot(s, H, TS, nbx);
    if (!q.live) return;
    long long K = d2key(-INFINITY);
#pragma unroll 8
    for (int r = q.r0; r < q.r1; ++r) {
        const long long c = q.L + s[r];
        if (c < 0 || c >= W) continue;
        const float v = z[(size_t)r * W + (size_t)c];
        if (dsm_cell_valid(v, nodata)) K = max(K, d2key(sun_key(v, a, b, r, c)));
    }
    M[q.at] = K;
}

// The first row of [0, H) whose u = sg s is >= v (H if none); u does not decrease.
__device__ __forceinline__ int sun_first(const int* __restrict__ s, int H, int sg, long long v)
{
    int lo = 0, hi = H;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if ((long long)sg * s[mid] >= v) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// One lane per line: M[band][slot] becomes the maximum over the bands before it in sunward order.
__global__ __launch_bounds__(SUN_THREADS)
void dsm_sun_carry(const int* __restrict__ s, int W, int H, int smax, long long nl, int sg, int ascending, long long TS, long long* __restrict__ M)
{
    const long long q = (long long)blockIdx.x * SUN_THREADS + threadIdx.x;
    if (q >= nl) return;
    const long long L = q - smax;
    // the rows with 0 <= L + s(r) < W
    const long long lo = sg > 0 ? -L : L - W + 1, hi = sg > 0 ? (long long)W - 1 - L : L;
    const int ra = sun_first(s, H, sg, lo), rb = sun_first(s, H, sg, hi + 1) - 1;
    if (ra > rb) return;
    const int ba = ra / SUN_BAND, bb = rb / SUN_BAND;
    long long carry = d2key(-INFINITY);
    for (int i = 0; i <= bb - ba; ++i) {
        const int band = ascending ? ba + i : bb - i;
        const int r0 = band * SUN_BAND, r1 = (int)min((long long)H, (long long)r0 + SUN_BAND);
        const long long t = L + (long long)max(s[r0], s[r1 - 1]);
        if (t < 0 || t >= TS) continue;                      // cannot happen: a band of B rows spans at most B shifts
        const size_t at = (size_t)band * (size_t)TS + (size_t)t;
        const long long own = M[at];
        M[at] = carry;
        carry = max(carry, own);
    }
}

__global__ __launch_bounds__(SUN_THREADS)
void dsm_sun_march(const float* __restrict__ z, int W, int H, float nodata, double a, double b, double tol, const int* __restrict__ s,
                   int ascending, long long TS, unsigned nbx, const long long* __restrict__ M, unsigned char* __restrict__ shade, float* __restrict__ depth)
{
    const SunSlot q = sun_slot(s, H, TS, nbx);
    if (!q.live) return;
    long long K = M[q.at];
    const int n = q.r1 - q.r0;
#pragma unroll 4
    for (int i = 0; i < n; ++i) {
        const int r = ascending ? q.r0 + i : q.r1 - 1 - i;
        const long long c = q.L + s[r];
        if (c < 0 || c >= W) continue;
        const size_t cell = (size_t)r * W + (size_t)c;
        const float v = z[cell];
        unsigned char sh = 0;
        float dp = nodata;
        if (dsm_cell_valid(v, nodata)) {
            const double g = sun_key(v, a, b, r, c);
            const double d = __dsub_rn(key2d(K), g);
            sh = d > tol ? 2 : 1;
            dp = (float)d;
            K = max(K, d2key(g));
        }
        shade[cell] = sh;
        if (depth) depth[cell] = dp;
    }
}

// out (W, H) = the transpose of in (H, W); blockIdx.x = (tile row) * ntx + (tile column).
template <typename T>
__global__ __launch_bounds__(SUN_THREADS)
void dsm_sun_transpose(const T* __restrict__ in, int W, int H, unsigned ntx, T* __restrict__ out)
{
    __shared__ T tile[SUN_TILE * SUN_PITCH];
    const int r0 = (int)(blockIdx.x / ntx) * SUN_TILE, c0 = (int)(blockIdx.x % ntx) * SUN_TILE;
    const int x = threadIdx.x % SUN_TILE, y0 = threadIdx.x / SUN_TILE;
    for (int y = y0; y < SUN_TILE; y += SUN_THREADS / SUN_TILE)
        if (r0 + y < H && c0 + x < W) tile[y * SUN_PITCH + x] = in[(size_t)(r0 + y) * W + (size_t)(c0 + x)];
    __syncthreads();
    for (int y = y0; y < SUN_TILE; y += SUN_THREADS / SUN_TILE)
        if (c0 + y < W && r0 + x < H) out[(size_t)(c0 + y) * H + (size_t)(r0 + x)] = tile[x * SUN_PITCH + y];
}

// ---- gradient --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SUN_THREADS)
void dsm_sun_gradient(const float* __restrict__ z, int gw, int gh, float nodata, double ex, double ey, unsigned cells,
                      float* __restrict__ dzde, float* __restrict__ dzdn)
{
    const unsigned cell = blockIdx.x * (unsigned)SUN_THREADS + threadIdx.x;
    if (cell >= cells) return;
    const int r = (int)(cell / (unsigned)gw), c = (int)(cell % (unsigned)gw);
    const float zc = z[cell];
    if (!dsm_cell_valid(zc, nodata)) {
        dzde[cell] = nodata;
        dzdn[cell] = nodata;
        return;
    }
    double n[3][3];                                          // n[dr + 1][dc + 1]; off the grid or invalid: the centre
#pragma unroll
    for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
        for (int dc = -1; dc <= 1; ++dc) {
            const int rr = r + dr, cc = c + dc;
            float v = zc;
            if ((dr || dc) && rr >= 0 && rr < gh && cc >= 0 && cc < gw) {
                const float t = z[(size_t)rr * gw + cc];
                if (dsm_cell_valid(t, nodata)) v = t;
            }
            n[dr + 1][dc + 1] = (double)v;
        }
    const double east = __dadd_rn(__dadd_rn(n[0][2], __dmul_rn(2.0, n[1][2])), n[2][2]);
    const double west = __dadd_rn(__dadd_rn(n[0][0], __dmul_rn(2.0, n[1][0])), n[2][0]);
    const double north = __dadd_rn(__dadd_rn(n[0][0], __dmul_rn(2.0, n[0][1])), n[0][2]);
    const double south = __dadd_rn(__dadd_rn(n[2][0], __dmul_rn(2.0, n[2][1])), n[2][2]);
    dzde[cell] = (float)__ddiv_rn(__dsub_rn(east, west), ex);
    dzdn[cell] = (float)__ddiv_rn(__dsub_rn(north, south), ey);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// The workspace: the shifts, the band table, then the transposed grid, shade and depth of the column-major directions.
struct SunPlan { size_t shifts, table, zt, shade_t, depth_t, total; };

static size_t sun_table_bytes(int W, int H)
{
    const size_t bands = ((size_t)H + SUN_BAND - 1) / SUN_BAND;
    return bands * ((size_t)W + SUN_BAND + 1) * sizeof(long long);
}

static SunPlan sun_plan(int gw, int gh)
{
    SunPlan p;
    const size_t cells = (size_t)gw * gh;
    size_t at = 0;
    p.shifts = at;  at += align256((size_t)(gw > gh ? gw : gh) * sizeof(int));
    p.table = at;   at += align256(sun_table_bytes(gw, gh) > sun_table_bytes(gh, gw) ? sun_table_bytes(gw, gh) : sun_table_bytes(gh, gw));
    p.zt = at;      at += align256(cells * sizeof(float));
    p.depth_t = at; at += align256(cells * sizeof(float));
    p.shade_t = at; at += align256(cells);
    p.total = at;
    return p;
}

template <typename T>
static int sun_transpose(const T* in, int W, int H, T* out, hipStream_t s, const char* what)
{
    const unsigned ntx = (unsigned)((W + SUN_TILE - 1) / SUN_TILE), nty = (unsigned)((H + SUN_TILE - 1) / SUN_TILE);
    hipLaunchKernelGGL(dsm_sun_transpose<T>, dim3(ntx * nty), dim3(SUN_THREADS), 0, s, in, W, H, ntx, out);
    return check_launch(what);
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT size_t smvs_dsm_shadow_workspace_bytes(int gw, int gh)
{
    using namespace smvs;
    if (grid_check(gw, gh)) return 0;
    return sun_plan(gw, gh).total;
}

SMVS_EXPORT int smvs_dsm_shadow(const float* dsm, int gw, int gh, float nodata, double ucol, double urow, double a, double b, double tol,
                                unsigned char* shade, float* depth, void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!dsm || !shade || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (!isfinite(ucol) || !isfinite(urow) || (ucol == 0.0 && urow == 0.0))
        return fail(SMVS_ERR_ARG, "the direction (ucol, urow) must be finite and not (0, 0), got (%g, %g)", ucol, urow);
    if (!isfinite(a) || !isfinite(b) || fabs(a) > SUN_MAX_TERM || fabs(b) > SUN_MAX_TERM)
        return fail(SMVS_ERR_ARG, "a and b must be finite and at most 2^900 in size, got %g, %g", a, b);
    if (!(isfinite(tol) && tol >= 0.0)) return fail(SMVS_ERR_ARG, "tol must be finite and >= 0, got %g", tol);
    const size_t ncells = (size_t)gw * gh;
    if (dsm_overlap(dsm, ncells * 4, shade, ncells)) return fail(SMVS_ERR_ARG, "shade aliases dsm");
    if (depth && (dsm_overlap(dsm, ncells * 4, depth, ncells * 4) || dsm_overlap(shade, ncells, depth, ncells * 4)))
        return fail(SMVS_ERR_ARG, "depth aliases dsm or shade");
    const SunPlan p = sun_plan(gw, gh);
    if (workspace_bytes < p.total) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, p.total);
    if (dsm_overlap(dsm, ncells * 4, workspace, p.total) || dsm_overlap(shade, ncells, workspace, p.total) ||
        (depth && dsm_overlap(depth, ncells * 4, workspace, p.total)))
        return fail(SMVS_ERR_ARG, "workspace aliases dsm, shade or depth");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int* s = (int*)(ws + p.shifts);
    long long* M = (long long*)(ws + p.table);
    float* zt = (float*)(ws + p.zt);
    float* depth_t = (float*)(ws + p.depth_t);
    unsigned char* shade_t = (unsigned char*)(ws + p.shade_t);

    const bool rows = fabs(urow) >= fabs(ucol);              // a tie is row-major
    // the working grid (H rows along the scan, W columns) and the rule's numbers on it
    const int W = rows ? gw : gh, H = rows ? gh : gw;
    const double along = rows ? urow : ucol, across = rows ? ucol : urow;
    const double m = across / along;
    const double wa = rows ? a : b, wb = rows ? b : a;
    const int ascending = along < 0.0 ? 1 : 0;
    const float* zin = dsm;
    unsigned char* sh = shade;
    float* dp = depth;
    if (!rows) {
        if (int rc = sun_transpose(dsm, gw, gh, zt, st, "dsm_sun_transpose (in)")) return rc;
        zin = zt;
        sh = shade_t;
        dp = depth ? depth_t : nullptr;
    }
    // s is monotone from s(0) = 0, so its extremes are 0 and s(H - 1), computed here as the kernel computes it
    const double last = floor(m * (double)(H - 1) + 0.5);    // -ffp-contract=off: a product, a sum, a floor
    const int s_last = (int)last, smax = s_last > 0 ? s_last : 0, smin = s_last < 0 ? s_last : 0;
    const long long nl = (long long)W + smax - smin;
    const int sg = m < 0.0 ? -1 : 1;
    const long long TS = (long long)W + SUN_BAND + 1;
    const unsigned nbands = (unsigned)((H + SUN_BAND - 1) / SUN_BAND), nbx = (unsigned)((TS + SUN_THREADS - 1) / SUN_THREADS);
    hipLaunchKernelGGL(dsm_sun_shifts, dim3((unsigned)((H + SUN_THREADS - 1) / SUN_THREADS)), dim3(SUN_THREADS), 0, st, m, H, s);
    if (int rc = check_launch("dsm_sun_shifts")) return rc;
    hipLaunchKernelGGL(dsm_sun_band_max, dim3(nbands * nbx), dim3(SUN_THREADS), 0, st, zin, W, H, nodata, wa, wb, s, TS, nbx, M);
    if (int rc = check_launch("dsm_sun_band_max")) return rc;
    hipLaunchKernelGGL(dsm_sun_carry, dim3((unsigned)((nl + SUN_THREADS - 1) / SUN_THREADS)), dim3(SUN_THREADS), 0, st, s, W, H, smax, nl, sg, ascending, TS, M);
    if (int rc = check_launch("dsm_sun_carry")) return rc;
    hipLaunchKernelGGL(dsm_sun_march, dim3(nbands * nbx), dim3(SUN_THREADS), 0, st, zin, W, H, nodata, wa, wb, tol, s, ascending, TS, nbx, M, sh, dp);
    if (int rc = check_launch("dsm_sun_march")) return rc;
    if (!rows) {
        if (int rc = sun_transpose(shade_t, W, H, shade, st, "dsm_sun_transpose (shade)")) return rc;
        if (depth)
            if (int rc = sun_transpose(depth_t, W, H, depth, st, "dsm_sun_transpose (depth)")) return rc;
    }
    return SMVS_OK;
}

SMVS_EXPORT int smvs_dsm_gradient(const float* dsm, int gw, int gh, float nodata, double xres, double yres,
                                  float* dzde, float* dzdn, void* stream)
{
    using namespace smvs;
    if (!dsm || !dzde || !dzdn) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (!(isfinite(xres) && xres > 0.0) || !(isfinite(yres) && yres > 0.0))
        return fail(SMVS_ERR_ARG, "the resolutions must be finite and > 0, got %g, %g", xres, yres);
    const size_t nb = (size_t)gw * gh * 4;
    if (dsm_overlap(dsm, nb, dzde, nb) || dsm_overlap(dsm, nb, dzdn, nb) || dsm_overlap(dzde, nb, dzdn, nb))
        return fail(SMVS_ERR_ARG, "dzde and dzdn must be distinct from dsm and from each other");
    const unsigned cells = (unsigned)((size_t)gw * gh);
    hipLaunchKernelGGL(dsm_sun_gradient, dim3((cells + SUN_THREADS - 1u) / SUN_THREADS), dim3(SUN_THREADS), 0, (hipStream_t)stream,
                       dsm, gw, gh, nodata, 8.0 * xres, 8.0 * yres, cells, dzde, dzdn);
    return check_launch("dsm_sun_gradient");
}

}  // extern "C"
