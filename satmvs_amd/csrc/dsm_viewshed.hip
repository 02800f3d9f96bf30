// dsm_viewshed.hip -- viewsheds of a DSM ("Viewshed"; include/satmvs.h for the rule).
//
//   smvs_dsm_viewshed   for up to 64 observers at once, which cells an eye on or above the surface sees: one exact line of
//                       sight per (observer, target cell), with earth curvature and refraction as a drop in height
//   smvs_dsm_los        the same rule for a device list of (observer, target) pairs
//
// One device function, vs_line, walks a line for both entries: the major coordinate moves a cell per step towards the target,
// the minor one follows floor((2 i dm + n) / (2 n)) through an integer error accumulator (no division per step), and every
// valid cell met is compared with the target by an int64 cross-multiplication of two int32 factors.  With `above` the walk
// keeps the steepest sample as a pair (numerator, step) and takes one integer ceiling division at the end; without it a lane
// stops at the first sample that hides its target, and a wave ends when all its lanes have.  The viewshed reads the heights
// as int32 q = rint(256 z) that dsm_viewshed_quantise writes once per call (VS_VOID where a cell is invalid); the list of
// lines quantises the floats it meets.  A wave of the viewshed is a VS_TILE_H x VS_TILE_W block of neighbouring targets:
// their lines meet in the observer and pass through nearly the same cells, so the gathers of a step fall into few cache
// lines.  All observers of a call walk in one launch (blockIdx.y).
// No atomics, no host synchronisation, no LDS; every kernel writes every element it owns.
#include <math.h>
#include <stdint.h>

#include "dsm_common.h"
#include "smvs_host.h"

namespace smvs {

constexpr int VS_THREADS = 256;
constexpr int VS_WAVES = VS_THREADS / 64;                // the waves of a workgroup lie side by side along a row
#ifndef VS_TILE_H
#define VS_TILE_H 8                                      // 8: a wave is an 8 x 8 block of cells; 1: 64 cells of a row (DESIGN.md has both times)
#endif                                                   // the switch exists only to reproduce that timing (tools/bench_dsm_viewshed.py
                                                         // --variant-lib, which holds the bits equal); no test builds the other value
constexpr int VS_TILE_W = 64 / VS_TILE_H;
static_assert(VS_TILE_H * VS_TILE_W == 64, "a wave holds 64 targets");
constexpr int VS_MAX_OBS = 64;                           // observers of one call: they walk side by side in one launch
constexpr int VS_VOID = INT32_MIN;                       // q of an invalid cell
constexpr int VS_MAX_SIDE = 65536;                       // n < 2^16, so (q' - E) n and (q' - E) i stay below 2^47
constexpr int VS_MAX_HEIGHT = 1 << 23;                   // |eye| and tgt, in units of 2^-8 m
constexpr double VS_MAX_DROP = 0x1p30;

struct VsObs { int col, row, eye, mode, tgt; };
struct VsTable { VsObs o[VS_MAX_OBS]; };
struct VsTerms { double xres, yres, c256, r2max; };

__device__ __forceinline__ int vs_quantise(float v, float nodata)
{
    int q;
    return dsm_quantum(v, nodata, q) ? q : VS_VOID;
}

// Where a line reads its heights: the quantised grid of the workspace, or the floats themselves.
struct VsFromQ {
    const int* __restrict__ q;
    __device__ __forceinline__ int operator()(int cell) const { return q[cell]; }
};
struct VsFromZ {
    const float* __restrict__ z;
    float nodata;
    __device__ __forceinline__ int operator()(int cell) const { return vs_quantise(z[cell], nodata); }
};

// The sum of squares of an offset of (a, b) cells of (ra, rb) metres: every product and the sum rounded by themselves.
__device__ __forceinline__ double vs_dist2(int a, double ra, int b, double rb)
{
    const double x = __dmul_rn((double)a, ra), y = __dmul_rn((double)b, rb);
    return __dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y));
}

// D fits an int under the limit c256 ((gw xres)^2 + (gh yres)^2) < 2^30
__device__ __forceinline__ int vs_drop(double c256, double d2) { return __double2int_rn(__dmul_rn(c256, d2)); }

// One line of sight from the eye E over cell (ro, co) to the valid cell (rt, ct) of height qt, both on the grid.
// -> 1 seen, 2 hidden, 3 out of range; with ABOVE and 2, *need = what must stand on the target to be seen, in units.
template <bool ABOVE, bool CURV, class Heights>
__device__ __forceinline__ int vs_line(const Heights& heights, int gw, const VsTerms& t, int co, int ro, int E, int ct, int rt, int qt,
                                       int tgt, long long* need)
{
    const int dx = ct - co, dy = rt - ro;
    const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    const bool rows = ay >= ax;                                     // a tie steps along the rows
    const int n = rows ? ay : ax, dm = rows ? dx : dy;
    const double d2 = vs_dist2(dx, t.xres, dy, t.yres);
    if (!(d2 <= t.r2max)) return 3;
    int top = qt - E + tgt;                                         // q'_t + tgt - E: below 2^31 in size under the limits
    if (CURV) top -= vs_drop(t.c256, d2);
    const int sg = (rows ? dy : dx) < 0 ? -1 : 1;
    const int major = rows ? sg * gw : sg, minor = rows ? 1 : gw;   // what a step adds to the cell index
    const double res_major = rows ? t.yres : t.xres, res_minor = rows ? t.xres : t.yres;
    const int two_n = 2 * n, two_dm = 2 * dm;
    int cell = ro * gw + co, acc = n, m = 0;                        // acc = (2 i dm + n) mod 2 n, m = its quotient
    int best_num = 0, best_i = 0;                                   // the steepest sample so far, (q'_j - E) / i_j; best_i 0 = none
    bool hidden = false;
    for (int i = 1; i < n; ++i) {
        acc += two_dm;
        const int carry = (acc >= two_n ? 1 : 0) - (acc < 0 ? 1 : 0);      // |dm| <= n: one carry a step at most
        acc -= carry * two_n;
        m += carry;
        cell += major + carry * minor;
        const int qj = heights(cell);
        if (qj == VS_VOID) continue;
        int num = qj - E;
        if (CURV) num -= vs_drop(t.c256, vs_dist2(i, res_major, m, res_minor));      // a sum commutes and a square loses the sign
        if (ABOVE) {
            if (best_i == 0 || (long long)num * best_i > (long long)best_num * i) { best_num = num; best_i = i; }
        } else if ((long long)num * n > (long long)top * i) {
            hidden = true;
            break;
        }
    }
    if (ABOVE && best_i != 0) {
        const long long a = (long long)best_num * n;
        if (a > (long long)top * best_i) {
            hidden = true;
            const long long quot = a / best_i;                      // a > top best_i; the ceiling of the exact quotient
            *need = quot + (a % best_i > 0 ? 1 : 0) - (long long)(top - tgt);
        }
    }
    return hidden ? 2 : 1;
}

__device__ __forceinline__ float vs_above(int code, long long need, float nodata)
{
    return code == 1 ? 0.0f : code == 2 ? __double2float_rn(__ddiv_rn((double)need, 256.0)) : nodata;
}

__global__ __launch_bounds__(VS_THREADS)
void dsm_viewshed_quantise(const float* __restrict__ z, unsigned cells, float nodata, int* __restrict__ q)
{
    const unsigned cell = blockIdx.x * VS_THREADS + threadIdx.x;
    if (cell < cells) q[cell] = vs_quantise(z[cell], nodata);
}

// blockIdx.y = the observer; blockIdx.x = (tile row) * ntx + (tile column) of tiles VS_TILE_H rows by VS_WAVES * VS_TILE_W columns.
template <bool ABOVE, bool CURV>
__global__ __launch_bounds__(VS_THREADS)
void dsm_viewshed_walk(const int* __restrict__ q, int gw, int gh, float nodata, const VsTerms t, const VsTable table, unsigned ntx,
                       size_t cells, unsigned char* __restrict__ seen, float* __restrict__ above, int* __restrict__ status)
{
    const VsObs o = table.o[blockIdx.y];
    const int qo = q[o.row * gw + o.col];
    const bool stands = o.mode == 1 || qo != VS_VOID;
    if (blockIdx.x == 0 && threadIdx.x == 0) status[blockIdx.y] = stands ? 1 : 0;
    const unsigned wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const unsigned r = (blockIdx.x / ntx) * VS_TILE_H + lane / VS_TILE_W;
    const unsigned c = ((blockIdx.x % ntx) * VS_WAVES + wave) * VS_TILE_W + lane % VS_TILE_W;
    if (r >= (unsigned)gh || c >= (unsigned)gw) return;
    const int cell = (int)(r * (unsigned)gw + c);
    const int qt = q[cell];
    int code = 0;
    long long need = 0;
    if (stands && qt != VS_VOID)
        code = vs_line<ABOVE, CURV>(VsFromQ{q}, gw, t, o.col, o.row, o.mode == 1 ? o.eye : qo + o.eye, (int)c, (int)r, qt, o.tgt, &need);
    const size_t at = (size_t)blockIdx.y * cells + (size_t)cell;
    seen[at] = (unsigned char)code;
    if (ABOVE) above[at] = vs_above(code, need, nodata);
}

// One lane per pair (col_o, row_o, eye, mode, col_t, row_t, tgt); a pair with a field out of range reads nothing and gets 0.
template <bool ABOVE, bool CURV>
__global__ __launch_bounds__(VS_THREADS)
void dsm_los_walk(const float* __restrict__ z, int gw, int gh, float nodata, const VsTerms t, const int* __restrict__ pairs, unsigned n_pairs,
                  unsigned char* __restrict__ seen, float* __restrict__ above)
{
    const unsigned k = blockIdx.x * VS_THREADS + threadIdx.x;
    if (k >= n_pairs) return;
    const int* p = pairs + 7 * (size_t)k;
    const int co = p[0], ro = p[1], eye = p[2], mode = p[3], ct = p[4], rt = p[5], tgt = p[6];
    const bool fields = co >= 0 && co < gw && ro >= 0 && ro < gh && ct >= 0 && ct < gw && rt >= 0 && rt < gh && (mode == 0 || mode == 1) &&
                        eye <= VS_MAX_HEIGHT && eye >= (mode == 0 ? 0 : -VS_MAX_HEIGHT) && tgt >= 0 && tgt <= VS_MAX_HEIGHT;
    int code = 0;
    long long need = 0;
    if (fields) {
        const VsFromZ heights{z, nodata};
        const int qo = mode == 1 ? 0 : heights(ro * gw + co), qt = heights(rt * gw + ct);
        if (qo != VS_VOID && qt != VS_VOID)
            code = vs_line<ABOVE, CURV>(heights, gw, t, co, ro, qo + eye, ct, rt, qt, tgt, &need);
    }
    seen[k] = (unsigned char)code;
    if (ABOVE) above[k] = vs_above(code, need, nodata);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// The limits both entries put on the grid and the four doubles; a message, or null.
static const char* vs_terms_check(int gw, int gh, double xres, double yres, double c256, double r2max, char* buf, size_t len)
{
    if (const char* msg = grid_check(gw, gh)) return msg;
    if (gw > VS_MAX_SIDE || gh > VS_MAX_SIDE) return "grid too long: gw and gh must be at most 65536";
    if (!isfinite(xres) || !isfinite(yres) || !(xres > 0.0) || !(yres > 0.0)) {
        snprintf(buf, len, "xres and yres must be finite and > 0, got (%g, %g)", xres, yres);
        return buf;
    }
    if (!isfinite(c256) || !(c256 >= 0.0)) {
        snprintf(buf, len, "c256 must be finite and >= 0, got %g", c256);
        return buf;
    }
    const double w = (double)gw * xres, h = (double)gh * yres;
    if (!(c256 * (w * w + h * h) < VS_MAX_DROP)) {
        snprintf(buf, len, "c256 ((gw xres)^2 + (gh yres)^2) must stay below 2^30, got %g", c256 * (w * w + h * h));
        return buf;
    }
    if (!(r2max > 0.0)) {                                    // NaN fails too; +inf passes
        snprintf(buf, len, "r2max must be > 0 or +inf, got %g", r2max);
        return buf;
    }
    return nullptr;
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT size_t smvs_dsm_viewshed_workspace_bytes(int gw, int gh, int n_obs)
{
    using namespace smvs;
    if (grid_check(gw, gh) || gw > VS_MAX_SIDE || gh > VS_MAX_SIDE || n_obs < 1 || n_obs > VS_MAX_OBS) return 0;
    return align256((size_t)gw * gh * 4);
}

SMVS_EXPORT int smvs_dsm_viewshed(const float* dsm, int gw, int gh, float nodata, double xres, double yres, double c256, double r2max,
                                  const int* obs, int n_obs, unsigned char* seen, float* above, int* status,
                                  void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    char buf[160];
    if (!dsm || !obs || !seen || !status || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = vs_terms_check(gw, gh, xres, yres, c256, r2max, buf, sizeof buf)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (n_obs < 1 || n_obs > VS_MAX_OBS) return fail(SMVS_ERR_ARG, "n_obs must be 1 .. %d, got %d", VS_MAX_OBS, n_obs);
    VsTable table = {};
    for (int k = 0; k < n_obs; ++k) {
        const VsObs o = {obs[5 * k], obs[5 * k + 1], obs[5 * k + 2], obs[5 * k + 3], obs[5 * k + 4]};
        if (o.col < 0 || o.col >= gw || o.row < 0 || o.row >= gh)
            return fail(SMVS_ERR_ARG, "observer %d: (col %d, row %d) is off the %d x %d grid", k, o.col, o.row, gw, gh);
        if (o.mode != 0 && o.mode != 1) return fail(SMVS_ERR_ARG, "observer %d: mode must be 0 or 1, got %d", k, o.mode);
        if (o.eye > VS_MAX_HEIGHT || o.eye < (o.mode == 0 ? 0 : -VS_MAX_HEIGHT))
            return fail(SMVS_ERR_ARG, "observer %d: eye must be %s 2^23 units of 2^-8 m, got %d", k, o.mode == 0 ? "0 .." : "within +-", o.eye);
        if (o.tgt < 0 || o.tgt > VS_MAX_HEIGHT) return fail(SMVS_ERR_ARG, "observer %d: tgt must be 0 .. 2^23 units of 2^-8 m, got %d", k, o.tgt);
        table.o[k] = o;
    }
    const size_t cells = (size_t)gw * gh, need = align256(cells * 4), maps = (size_t)n_obs * cells;
    if (workspace_bytes < need) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    const void* bufs[5] = {dsm, seen, above, status, workspace};
    const size_t sizes[5] = {cells * 4, maps, maps * 4, (size_t)n_obs * 4, need};
    for (int i = 0; i < 5; ++i)
        for (int j = i + 1; j < 5; ++j)
            if (bufs[i] && bufs[j] && dsm_overlap(bufs[i], sizes[i], bufs[j], sizes[j]))
                return fail(SMVS_ERR_ARG, "dsm, seen, above, status and workspace must not overlap");
    hipStream_t st = (hipStream_t)stream;
    int* q = (int*)workspace;
    const VsTerms t = {xres, yres, c256, r2max};
    hipLaunchKernelGGL(dsm_viewshed_quantise, dim3((unsigned)((cells + VS_THREADS - 1) / VS_THREADS)), dim3(VS_THREADS), 0, st,
                       dsm, (unsigned)cells, nodata, q);
    if (int rc = check_launch("dsm_viewshed_quantise")) return rc;
    const unsigned ntx = (unsigned)((gw + VS_WAVES * VS_TILE_W - 1) / (VS_WAVES * VS_TILE_W)), nty = (unsigned)((gh + VS_TILE_H - 1) / VS_TILE_H);
    const dim3 blocks(ntx * nty, (unsigned)n_obs), threads(VS_THREADS);
    const bool curved = c256 != 0.0;
#define VS_LAUNCH(A, C) hipLaunchKernelGGL((dsm_viewshed_walk<A, C>), blocks, threads, 0, st, q, gw, gh, nodata, t, table, ntx, cells, seen, above, status)
    if (above) { if (curved) VS_LAUNCH(true, true); else VS_LAUNCH(true, false); }
    else { if (curved) VS_LAUNCH(false, true); else VS_LAUNCH(false, false); }
#undef VS_LAUNCH
    return check_launch("dsm_viewshed_walk");
}

SMVS_EXPORT int smvs_dsm_los(const float* dsm, int gw, int gh, float nodata, double xres, double yres, double c256, double r2max,
                             const int* pairs, int n_pairs, unsigned char* seen, float* above, void* stream)
{
    using namespace smvs;
    char buf[160];
    if (!dsm || !pairs || !seen) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = vs_terms_check(gw, gh, xres, yres, c256, r2max, buf, sizeof buf)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (n_pairs < 1) return fail(SMVS_ERR_ARG, "n_pairs must be 1 .. 2^31 - 1, got %d", n_pairs);
    const size_t cells = (size_t)gw * gh, np = (size_t)n_pairs;
    const void* bufs[4] = {dsm, pairs, seen, above};
    const size_t sizes[4] = {cells * 4, np * 28, np, np * 4};
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (bufs[i] && bufs[j] && dsm_overlap(bufs[i], sizes[i], bufs[j], sizes[j]))
                return fail(SMVS_ERR_ARG, "dsm, pairs, seen and above must not overlap");
    hipStream_t st = (hipStream_t)stream;
    const VsTerms t = {xres, yres, c256, r2max};
    const dim3 blocks((unsigned)((np + VS_THREADS - 1) / VS_THREADS)), threads(VS_THREADS);
    const bool curved = c256 != 0.0;
#define VS_LAUNCH(A, C) hipLaunchKernelGGL((dsm_los_walk<A, C>), blocks, threads, 0, st, dsm, gw, gh, nodata, t, pairs, (unsigned)n_pairs, seen, above)
    if (above) { if (curved) VS_LAUNCH(true, true); else VS_LAUNCH(true, false); }
    else { if (curved) VS_LAUNCH(false, true); else VS_LAUNCH(false, false); }
#undef VS_LAUNCH
    return check_launch("dsm_los_walk");
}

}  // extern "C"
