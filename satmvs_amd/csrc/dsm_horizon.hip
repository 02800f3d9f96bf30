// dsm_horizon.hip -- horizon maps of a DSM ("Horizon"; include/satmvs.h for the rule).
//
//   smvs_dsm_horizon   for up to 64 azimuths at once, the tangent of the elevation of the highest thing that stands towards the
//                      azimuth: the maximum of (q_j - q_i) / (P_j - P_i) over the valid cells j of a cell's line that lie towards it
//
// The lines are those of smvs_dsm_shadow (dsm_sun.hip), and as there the kernels know one orientation, the row-major one: the
// scan runs along the rows of a (H, W) grid, the line of cell (r, c) is c - s(r), a lane owns one line of one direction, and
// at row r a wave touches the consecutive columns L + s(r).  The column-major directions walk the transposed heights with
// (ucol, urow) and (a, b) swapped -- P is a sum of two products and IEEE addition commutes -- and write a transposed map that
// dsm_horizon_untranspose turns back, so every global access of a wave along the walk runs along a row in both orientations.
// dsm_horizon_quantise writes the heights once as int32 q = rint(256 z) (HZ_VOID where a cell is invalid) and, through a
// 64 x 64 LDS tile at pitch 65, their transpose.
// The maximum is the tangent from cell i to the upper convex hull of the cells before it, kept as a stack along the walk: pop
// the top while the slope from i to the element under it is >= the slope from i to the top, read the tangent off the top,
// push i.  Both slopes are compared by exact int64 cross-multiplication (the host checks keep every product below 2^62), so
// the result is the O(n^2) maximum over all pairs and no rounded quotient ever decides anything; the one quotient taken is the
// result's.  The stack is a chain of links, not an array: when a cell is pushed, the row of the element under it is stored at
// the cell (4 bytes per cell and direction in flight), the top two elements and the row of the third live in registers, and a
// pop gathers one link and one q.  A lane reads only links it wrote itself earlier in the same call: garbage in the workspace
// does not matter.  What fills the machine is the direction axis: all directions of a call walk side by side in one launch.
// s(r) = floor(m r + 0.5) is computed where it is needed (hz_shift, the one place the floor rule lives here): a pop needs it
// at a row of its own, where a table would cost a second dependent gather.
// No atomics, no host synchronisation; every kernel writes every element it owns.
#include <math.h>
#include <stdint.h>

#include "dsm_common.h"
#include "smvs_host.h"

namespace smvs {

constexpr int HZ_THREADS = 256;                          // quantise and untranspose
constexpr int HZ_LANES = 64;                             // lines of a workgroup of the walk: one wave
constexpr int HZ_TILE = 64, HZ_PITCH = HZ_TILE + 1;      // the transposes' tile and its odd pitch in LDS
constexpr int HZ_PF = 4;                                 // rows of q a lane loads ahead of the walk
constexpr int HZ_MAX_DIRS = 64;                          // directions of one call: they walk side by side in one launch
constexpr int HZ_VOID = INT32_MIN;                       // q of an invalid cell
constexpr int HZ_OFF = INT32_MIN + 1;                    // a row of the walk at which the line is off the grid
constexpr double HZ_MIN_ALONG = 4.0, HZ_MAX_SPAN = 0x1p37;

// One direction on its working grid (H rows along the scan, W columns): wa the term per column, wb per row.
struct HzDir { double m, wa, wb; int smax, nl, ascending, transposed; };
struct HzDirs { HzDir d[HZ_MAX_DIRS]; };

__device__ __forceinline__ int hz_shift(double m, int r) { return (int)floor(__dadd_rn(__dmul_rn(m, (double)r), 0.5)); }

__device__ __forceinline__ long long hz_pos(double wa, double wb, int r, int c)
{
    return __double2ll_rn(__dadd_rn(__dmul_rn(wa, (double)c), __dmul_rn(wb, (double)r)));
}

// The first row of [0, H) whose sg s(r) is >= v (H if none); sg s does not decrease.
__device__ __forceinline__ int hz_first(double m, int H, int sg, long long v)
{
    int lo = 0, hi = H;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if ((long long)sg * hz_shift(m, mid) >= v) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// q (gh, gw) and, if qt is non-null, qt (gw, gh) = its transpose; blockIdx.x = (tile row) * ntx + (tile column).
__global__ __launch_bounds__(HZ_THREADS)
void dsm_horizon_quantise(const float* __restrict__ z, int gw, int gh, float nodata, unsigned ntx, int* __restrict__ q, int* __restrict__ qt)
{
    __shared__ int tile[HZ_TILE * HZ_PITCH];
    const int r0 = (int)(blockIdx.x / ntx) * HZ_TILE, c0 = (int)(blockIdx.x % ntx) * HZ_TILE;
    const int x = threadIdx.x % HZ_TILE, y0 = threadIdx.x / HZ_TILE;
    for (int y = y0; y < HZ_TILE; y += HZ_THREADS / HZ_TILE)
        if (r0 + y < gh && c0 + x < gw) {
            const size_t cell = (size_t)(r0 + y) * gw + (size_t)(c0 + x);
            int k;
            if (!dsm_quantum(z[cell], nodata, k)) k = HZ_VOID;
            q[cell] = k;
            tile[y * HZ_PITCH + x] = k;
        }
    if (!qt) return;
    __syncthreads();
    for (int y = y0; y < HZ_TILE; y += HZ_THREADS / HZ_TILE)
        if (c0 + y < gw && r0 + x < gh) qt[(size_t)(c0 + y) * gh + (size_t)(r0 + x)] = tile[x * HZ_PITCH + y];
}

// q of the cell of line L at row r, HZ_OFF where the row is outside [ra, rb] or the line is off the grid there.
__device__ __forceinline__ int hz_fetch(const int* __restrict__ Q, int W, double m, long long L, int r, int ra, int rb)
{
    if (r < ra || r > rb) return HZ_OFF;
    const long long c = L + hz_shift(m, r);
    return c < 0 || c >= W ? HZ_OFF : Q[(size_t)r * W + (size_t)c];
}

// The walk of one line.  block = the workgroup's index along the lines, lane = the lane's index in it.
__device__ __forceinline__ void hz_walk(const int* __restrict__ Q, int W, int H, const HzDir d, unsigned block, unsigned lane,
                                        int* link, float* __restrict__ out)
{
    const long long La = (long long)block * HZ_LANES - d.smax, Lb = La + HZ_LANES - 1, L = La + lane;
    if ((long long)block * HZ_LANES + lane >= d.nl) return;
    // the rows at which a line of this workgroup is on the grid: 0 <= L + s(r) < W for some L in [La, Lb]
    const int sg = d.m < 0.0 ? -1 : 1;
    const long long lo = sg > 0 ? -Lb : La - W + 1, hi = sg > 0 ? (long long)W - 1 - La : Lb;
    const int ra = hz_first(d.m, H, sg, lo), rb = hz_first(d.m, H, sg, hi + 1) - 1;
    const int n = rb - ra + 1, step = d.ascending ? 1 : -1, first = d.ascending ? ra : rb;
    // the stack's top (row t, q and P), the element under it (u), and the row under that (uu); -1 = none
    int t = -1, u = -1, uu = -1, qt = 0, qu = 0;
    long long Pt = 0, Pu = 0;
    int cur[HZ_PF], nxt[HZ_PF];
#pragma unroll
    for (int j = 0; j < HZ_PF; ++j) cur[j] = hz_fetch(Q, W, d.m, L, first + j * step, ra, rb);
    for (int base = 0; base < n; base += HZ_PF) {
#pragma unroll
        for (int j = 0; j < HZ_PF; ++j) nxt[j] = hz_fetch(Q, W, d.m, L, first + (base + HZ_PF + j) * step, ra, rb);
#pragma unroll
        for (int j = 0; j < HZ_PF; ++j) {
            const int qi = cur[j], r = first + (base + j) * step;
            if (qi == HZ_OFF) continue;
            const int c = (int)(L + hz_shift(d.m, r));
            const size_t cell = (size_t)r * W + (size_t)c;
            if (qi == HZ_VOID) {
                out[cell] = __int_as_float(0x7fc00000);
                continue;
            }
            const long long Pi = hz_pos(d.wa, d.wb, r, c);
            // pop while the slope from i to the element under the top is >= the slope from i to the top (both denominators > 0)
            while (u >= 0 && (long long)(qu - qi) * (Pt - Pi) >= (long long)(qt - qi) * (Pu - Pi)) {
                t = u; qt = qu; Pt = Pu;
                u = uu;
                if (u >= 0) {
                    const int cu = (int)(L + hz_shift(d.m, u));
                    const size_t under = (size_t)u * W + (size_t)cu;
                    qu = Q[under];
                    uu = link[under];
                    Pu = hz_pos(d.wa, d.wb, u, cu);
                }
            }
            out[cell] = t >= 0 ? __double2float_rn(__ddiv_rn((double)(qt - qi), (double)(Pt - Pi))) : -INFINITY;
            link[cell] = t;
            uu = u; u = t; qu = qt; Pu = Pt;
            t = r; qt = qi; Pt = Pi;
        }
#pragma unroll
        for (int j = 0; j < HZ_PF; ++j) cur[j] = nxt[j];
    }
}

// blockIdx.y = the direction, blockIdx.x = 64 of its lines.  links and out_t hold one grid per direction.
__global__ __launch_bounds__(HZ_LANES)
void dsm_horizon_walk(const int* __restrict__ q, const int* __restrict__ qt, int gw, int gh, const HzDirs table, size_t cells,
                      int* links, float* __restrict__ out_t, float* __restrict__ tan_h)
{
    const HzDir d = table.d[blockIdx.y];
    const size_t at = (size_t)blockIdx.y * cells;
    if (d.transposed) hz_walk(qt, gh, gw, d, blockIdx.x, threadIdx.x, links + at, out_t + at);
    else hz_walk(q, gw, gh, d, blockIdx.x, threadIdx.x, links + at, tan_h + at);
}

// tan_h (gh, gw) of every column-major direction = the transpose of its out_t (gw, gh); blockIdx.y = the direction.
__global__ __launch_bounds__(HZ_THREADS)
void dsm_horizon_untranspose(const float* __restrict__ out_t, int gw, int gh, const HzDirs table, size_t cells, unsigned ntx,
                             float* __restrict__ tan_h)
{
    __shared__ float tile[HZ_TILE * HZ_PITCH];
    if (!table.d[blockIdx.y].transposed) return;
    const float* in = out_t + (size_t)blockIdx.y * cells;    // (gw rows, gh columns)
    float* out = tan_h + (size_t)blockIdx.y * cells;
    const int r0 = (int)(blockIdx.x / ntx) * HZ_TILE, c0 = (int)(blockIdx.x % ntx) * HZ_TILE;      // of `in`
    const int x = threadIdx.x % HZ_TILE, y0 = threadIdx.x / HZ_TILE;
    for (int y = y0; y < HZ_TILE; y += HZ_THREADS / HZ_TILE)
        if (r0 + y < gw && c0 + x < gh) tile[y * HZ_PITCH + x] = in[(size_t)(r0 + y) * gh + (size_t)(c0 + x)];
    __syncthreads();
    for (int y = y0; y < HZ_TILE; y += HZ_THREADS / HZ_TILE)
        if (c0 + y < gh && r0 + x < gw) out[(size_t)(c0 + y) * gw + (size_t)(r0 + x)] = tile[x * HZ_PITCH + y];
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// The workspace: q, its transpose, then per direction the links and the transposed map.
struct HzPlan { size_t q, qt, links, out_t, total; };

static HzPlan hz_plan(int gw, int gh, int n_dirs)
{
    HzPlan p;
    const size_t grid = align256((size_t)gw * gh * 4), slots = (size_t)n_dirs;
    size_t at = 0;
    p.q = at;     at += grid;
    p.qt = at;    at += grid;
    p.links = at; at += align256(slots * (size_t)gw * gh * 4);
    p.out_t = at; at += align256(slots * (size_t)gw * gh * 4);
    p.total = at;
    return p;
}

// The rule's numbers of one direction v = (ucol, urow, a, b) on its working grid.
static HzDir hz_dir(const double* v, int gw, int gh)
{
    HzDir d;
    const bool rows = fabs(v[1]) >= fabs(v[0]);                  // a tie is row-major
    const int W = rows ? gw : gh, H = rows ? gh : gw;
    const double along = rows ? v[1] : v[0], across = rows ? v[0] : v[1];
    d.m = across / along;
    d.wa = rows ? v[2] : v[3];
    d.wb = rows ? v[3] : v[2];
    // s is monotone from s(0) = 0, so its extremes are 0 and s(H - 1), computed here as the kernel computes it
    const int s_last = (int)floor(d.m * (double)(H - 1) + 0.5);  // -ffp-contract=off: a product, a sum, a floor
    d.smax = s_last > 0 ? s_last : 0;
    d.nl = W + d.smax - (s_last < 0 ? s_last : 0);
    d.ascending = along < 0.0 ? 1 : 0;
    d.transposed = rows ? 0 : 1;
    return d;
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT size_t smvs_dsm_horizon_workspace_bytes(int gw, int gh, int n_dirs)
{
    using namespace smvs;
    if (grid_check(gw, gh) || n_dirs < 1 || n_dirs > HZ_MAX_DIRS) return 0;
    return hz_plan(gw, gh, n_dirs).total;
}

SMVS_EXPORT int smvs_dsm_horizon(const float* dsm, int gw, int gh, float nodata, const double* dirs, int n_dirs, float* tan_h,
                                 void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!dsm || !dirs || !tan_h || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (n_dirs < 1 || n_dirs > HZ_MAX_DIRS) return fail(SMVS_ERR_ARG, "n_dirs must be 1 .. %d, got %d", HZ_MAX_DIRS, n_dirs);
    for (int k = 0; k < n_dirs; ++k) {
        const double ucol = dirs[4 * k], urow = dirs[4 * k + 1], a = dirs[4 * k + 2], b = dirs[4 * k + 3];
        if (!isfinite(ucol) || !isfinite(urow) || !isfinite(a) || !isfinite(b))
            return fail(SMVS_ERR_ARG, "direction %d is not finite: (%g, %g, %g, %g)", k, ucol, urow, a, b);
        if (ucol == 0.0 && urow == 0.0) return fail(SMVS_ERR_ARG, "direction %d: (ucol, urow) must not be (0, 0)", k);
        if (!(a * ucol >= 0.0) || !(b * urow >= 0.0))
            return fail(SMVS_ERR_ARG, "direction %d: a and ucol, b and urow must not differ in sign, got (%g, %g, %g, %g)", k, ucol, urow, a, b);
        const double along = fabs(urow) >= fabs(ucol) ? fabs(b) : fabs(a);
        if (!(along >= HZ_MIN_ALONG))
            return fail(SMVS_ERR_ARG, "direction %d: the term along the scan must be at least 4 in size (units of 2^-8 m), got %g", k, along);
        if (!(fabs(a) * (double)gw + fabs(b) * (double)gh < HZ_MAX_SPAN))
            return fail(SMVS_ERR_ARG, "direction %d: |a| gw + |b| gh must stay below 2^37, got %g", k, fabs(a) * (double)gw + fabs(b) * (double)gh);
    }
    const size_t cells = (size_t)gw * gh;
    const HzPlan p = hz_plan(gw, gh, n_dirs);
    if (workspace_bytes < p.total) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, p.total);
    if (dsm_overlap(dsm, cells * 4, tan_h, (size_t)n_dirs * cells * 4) || dsm_overlap(dsm, cells * 4, workspace, p.total) ||
        dsm_overlap(tan_h, (size_t)n_dirs * cells * 4, workspace, p.total))
        return fail(SMVS_ERR_ARG, "dsm, tan_h and workspace must not overlap");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int* q = (int*)(ws + p.q);
    int* qt = (int*)(ws + p.qt);
    int* links = (int*)(ws + p.links);
    float* out_t = (float*)(ws + p.out_t);

    HzDirs table = {};
    int most = 0;
    bool any_t = false;
    for (int k = 0; k < n_dirs; ++k) {
        table.d[k] = hz_dir(dirs + 4 * (size_t)k, gw, gh);
        most = table.d[k].nl > most ? table.d[k].nl : most;
        any_t = any_t || table.d[k].transposed;
    }
    const unsigned ntx = (unsigned)((gw + HZ_TILE - 1) / HZ_TILE), nty = (unsigned)((gh + HZ_TILE - 1) / HZ_TILE);
    hipLaunchKernelGGL(dsm_horizon_quantise, dim3(ntx * nty), dim3(HZ_THREADS), 0, st, dsm, gw, gh, nodata, ntx, q, any_t ? qt : nullptr);
    if (int rc = check_launch("dsm_horizon_quantise")) return rc;
    hipLaunchKernelGGL(dsm_horizon_walk, dim3((unsigned)((most + HZ_LANES - 1) / HZ_LANES), (unsigned)n_dirs), dim3(HZ_LANES), 0, st,
                       q, qt, gw, gh, table, cells, links, out_t, tan_h);
    if (int rc = check_launch("dsm_horizon_walk")) return rc;
    if (any_t) {
        const unsigned utx = (unsigned)((gh + HZ_TILE - 1) / HZ_TILE), uty = (unsigned)((gw + HZ_TILE - 1) / HZ_TILE);
        hipLaunchKernelGGL(dsm_horizon_untranspose, dim3(utx * uty, (unsigned)n_dirs), dim3(HZ_THREADS), 0, st, out_t, gw, gh, table, cells, utx, tan_h);
        if (int rc = check_launch("dsm_horizon_untranspose")) return rc;
    }
    return SMVS_OK;
}

}  // extern "C"
