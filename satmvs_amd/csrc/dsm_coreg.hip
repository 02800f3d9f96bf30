// dsm_coreg.hip -- registration of one DSM to another ("Registration"; include/satmvs.h for the rules).
//
//   smvs_dsm_shift_stats  n, sum q, sum q^2 of the height differences of two grids under every integer shift of a square
//   smvs_dsm_regrid       one DSM resampled onto another grid, nearest or bilinear
//
// Shift statistics.  A persistent grid of workgroups walks the 64 x 16 tiles of b.  A workgroup stages its tile of b and the
// matching window of a with a halo of `radius` cells in LDS, invalid and off-grid cells as NaN, so the one comparison
// |d| <= trim rejects them.  The (2 radius + 1)^2 shifts are dealt to the lanes, NS per lane: lane t holds the shifts t,
// t + 256, ...  and keeps their three accumulators (n 32 bits, the sums 64 bits) in registers across every tile the
// workgroup visits.  For one cell of b, read by all lanes at one LDS address (a broadcast), lane t reads a at the cell's
// address + sy * pitch + sx; the pitch of the window is 64 + (2 radius + 1) floats, so that offset equals the shift's index
// modulo 64 and the 64 lanes of a wave fall on 64 different banks.  With 128 shifts or fewer (radius <= 5) the lanes are
// split into parts that take every P-th cell of the tile, and the parts are added up through LDS at the end.  Every
// workgroup writes its sums to its own slice of the workspace; dsm_shift_fold adds the slices in order and writes stats.
// No atomics, integers only: any order gives the same bits.
#include <stdint.h>

#include "dsm_common.h"
#include "smvs_host.h"

namespace smvs {

constexpr int SHIFT_TW = 64, SHIFT_TH = 16, SHIFT_THREADS = 256, SHIFT_CELLS = SHIFT_TW * SHIFT_TH;
constexpr int SHIFT_MAX_RADIUS = 32;
constexpr int SHIFT_MAX_GROUPS = 1024, SHIFT_MAX_GROUPS_WIDE = 512;     // persistent workgroups; WIDE: more than 5 shifts a lane

struct ShiftPlan { int side, nshift, per_lane, lanes_per_part, parts; unsigned ntx, nty, ntiles, groups; size_t lds_bytes, bytes; };

static int shift_per_lane(int nshift)
{
    const int need = (nshift + SHIFT_THREADS - 1) / SHIFT_THREADS;
    for (int ns : {1, 2, 3, 5, 9, 13, 17})
        if (ns >= need) return ns;
    return 0;
}

static ShiftPlan shift_plan(int gwb, int ghb, int radius)
{
    ShiftPlan p;
    p.side = 2 * radius + 1;
    p.nshift = p.side * p.side;
    p.per_lane = shift_per_lane(p.nshift);
    p.lanes_per_part = SHIFT_THREADS;
    if (p.per_lane == 1)
        for (p.lanes_per_part = 1; p.lanes_per_part < p.nshift; p.lanes_per_part *= 2) {}
    p.parts = SHIFT_THREADS / p.lanes_per_part;
    p.ntx = (unsigned)((gwb + SHIFT_TW - 1) / SHIFT_TW);
    p.nty = (unsigned)((ghb + SHIFT_TH - 1) / SHIFT_TH);
    p.ntiles = p.ntx * p.nty;                                // below 2^31 / 1024 + 2^16
    const unsigned cap = p.per_lane > 5 ? SHIFT_MAX_GROUPS_WIDE : SHIFT_MAX_GROUPS;
    p.groups = p.ntiles < cap ? p.ntiles : cap;
    p.lds_bytes = ((size_t)(SHIFT_TH + 2 * radius) * (SHIFT_TW + p.side) + SHIFT_CELLS) * sizeof(float);     // >= 8 KiB
    p.bytes = align256((size_t)p.groups * p.nshift * 3 * sizeof(long long));
    return p;
}

__device__ __forceinline__ float shift_staged(float z, float nodata) { return dsm_cell_valid(z, nodata) ? z : __builtin_nanf(""); }

template <int NS>
__global__ __launch_bounds__(SHIFT_THREADS)
void dsm_shift_acc(const float* __restrict__ a, int gwa, int gha, const float* __restrict__ b, int gwb, int ghb, float nodata,
                   int ox, int oy, int radius, double dz0, double trim, unsigned ntx, unsigned ntiles, int lanes_per_part,
                   long long* __restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int side = 2 * radius + 1, nshift = side * side;
    const int pitch = SHIFT_TW + side, ah = SHIFT_TH + 2 * radius, aw = SHIFT_TW + 2 * radius;
    float* A = lds;                                          // ah rows of `pitch` floats: a's window, halo included
    float* B = lds + ah * pitch;                             // the tile of b, 16 x 64
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int parts = SHIFT_THREADS / lanes_per_part;        // NS > 1: one part
    const int part = tid / lanes_per_part, s0 = tid % lanes_per_part;
    int off[NS];
    unsigned n[NS];
    long long sq[NS];
    unsigned long long sqq[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int s = s0 + k * SHIFT_THREADS;
        off[k] = s < nshift ? (s / side) * pitch + s % side : 0;          // a lane without a shift adds up pairs nobody reads
        n[k] = 0; sq[k] = 0; sqq[k] = 0;
    }
    for (unsigned t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tx0 = (int)(t % ntx) * SHIFT_TW, ty0 = (int)(t / ntx) * SHIFT_TH;
        const long long ya0 = (long long)ty0 + oy - radius, xa0 = (long long)tx0 + ox - radius;       // a's cell under A[0]
        if (ya0 >= gha || ya0 + ah <= 0 || xa0 >= gwa || xa0 + aw <= 0) continue;      // the window misses a: no pair (the whole workgroup skips)
        __syncthreads();                                     // the last tile's reads are over
        for (int i = tid; i < SHIFT_CELLS; i += SHIFT_THREADS) {
            const int x = tx0 + (i & (SHIFT_TW - 1)), y = ty0 + i / SHIFT_TW;
            B[i] = x < gwb && y < ghb ? shift_staged(b[(size_t)y * gwb + x], nodata) : __builtin_nanf("");
        }
        for (int r = wave; r < ah; r += SHIFT_THREADS / 64) {
            const long long ya = ya0 + r;
            const bool row_in = ya >= 0 && ya < gha;
            for (int c = lane; c < aw; c += 64) {
                const long long xa = xa0 + c;
                A[r * pitch + c] = row_in && xa >= 0 && xa < gwa ? shift_staged(a[(size_t)ya * gwa + (size_t)xa], nodata) : __builtin_nanf("");
            }
        }
        __syncthreads();
        for (int i = part; i < SHIFT_CELLS; i += parts) {
            const float bv = B[i];
            if (bv != bv) continue;                          // one part: every lane of the workgroup reads this cell
            const double bd = (double)bv;
            const float* at = A + (i / SHIFT_TW) * pitch + (i & (SHIFT_TW - 1));
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const double d = ((double)at[off[k]] - bd) - dz0;
                const bool ok = fabs(d) <= trim;             // false for a NaN
                const int q = (int)rint((ok ? d : 0.0) * 256.0);          // |q| <= 2^16
                n[k] += ok ? 1u : 0u;
                sq[k] += q;
                sqq[k] += (unsigned long long)((long long)q * q);          // up to 2^32: the product in 64 bits
            }
        }
    }
    __syncthreads();
    long long* mine = partial + (size_t)blockIdx.x * nshift * 3;
    if (NS > 1 || parts == 1) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int s = s0 + k * SHIFT_THREADS;
            if (s < nshift) {
                mine[3 * s] = (long long)n[k];
                mine[3 * s + 1] = sq[k];
                mine[3 * s + 2] = (long long)sqq[k];
            }
        }
    } else {                                                 // the parts of a shift, added up through LDS (3 x 256 x 8 bytes <= 8 KiB)
        long long* L = (long long*)lds;
        L[tid] = (long long)n[0];
        L[SHIFT_THREADS + tid] = sq[0];
        L[2 * SHIFT_THREADS + tid] = (long long)sqq[0];
        __syncthreads();
        if (tid < nshift) {                                  // nshift <= lanes_per_part: tid is s0 of part 0
            long long v0 = 0, v1 = 0, v2 = 0;
            for (int p = 0; p < parts; ++p) {
                v0 += L[p * lanes_per_part + tid];
                v1 += L[SHIFT_THREADS + p * lanes_per_part + tid];
                v2 += L[2 * SHIFT_THREADS + p * lanes_per_part + tid];
            }
            mine[3 * tid] = v0;
            mine[3 * tid + 1] = v1;
            mine[3 * tid + 2] = v2;
        }
    }
}

// stats[j] = the sum of the workgroups' partial[g][j], g in order; this is what initialises stats.
__global__ __launch_bounds__(SHIFT_THREADS)
void dsm_shift_fold(const long long* __restrict__ partial, unsigned groups, unsigned nvalues, long long* __restrict__ stats)
{
    const unsigned j = blockIdx.x * (unsigned)SHIFT_THREADS + threadIdx.x;
    if (j >= nvalues) return;
    long long v = 0;
    for (unsigned g = 0; g < groups; ++g) v += partial[(size_t)g * nvalues + j];
    stats[j] = v;
}

// ---- regrid ----------------------------------------------------------------------------------------------------------------
struct Grid4 { double e0, n0, xres, yres; };

// The source cell (row, col), given as float64 integers that may lie anywhere: -> whether it is on the grid and valid.
__device__ __forceinline__ bool regrid_tap(const float* __restrict__ src, int gws, int ghs, float nodata, double row, double col, float& z)
{
    if (!(row >= 0.0 && row < (double)ghs && col >= 0.0 && col < (double)gws)) return false;          // a NaN is off the grid
    z = src[(size_t)row * gws + (size_t)col];
    return dsm_cell_valid(z, nodata);
}

__global__ __launch_bounds__(256)
void dsm_regrid(const float* __restrict__ src, int gws, int ghs, Grid4 gs, float nodata, Grid4 gd, int gwd, int ghd, int mode,
                double dz, float* __restrict__ out)
{
    const unsigned cell = blockIdx.x * 256u + threadIdx.x;
    if (cell >= (unsigned)gwd * (unsigned)ghd) return;
    const int r = (int)(cell / (unsigned)gwd), c = (int)(cell % (unsigned)gwd);
    const double E = gd.e0 + (double)c * gd.xres, N = gd.n0 - (double)r * gd.yres;
    const double u = (E - gs.e0) / gs.xres, v = (gs.n0 - N) / gs.yres;
    double i, j, wx0 = 1.0, wx1 = 0.0, wy0 = 1.0, wy1 = 0.0;                  // the weights of column i, i + 1, row j, j + 1
    if (mode == 0) {
        i = floor(u + 0.5); j = floor(v + 0.5);
    } else {
        i = floor(u); j = floor(v);
        wx1 = u - i; wx0 = 1.0 - wx1;
        wy1 = v - j; wy0 = 1.0 - wy1;
    }
    float z00 = 0.0f, z01 = 0.0f, z10 = 0.0f, z11 = 0.0f;    // a tap that is not read stands as 0.0
    bool ok = true;
    if (wx0 != 0.0 && wy0 != 0.0) ok = regrid_tap(src, gws, ghs, nodata, j, i, z00) && ok;
    if (wx1 != 0.0 && wy0 != 0.0) ok = regrid_tap(src, gws, ghs, nodata, j, i + 1.0, z01) && ok;
    if (wx0 != 0.0 && wy1 != 0.0) ok = regrid_tap(src, gws, ghs, nodata, j + 1.0, i, z10) && ok;
    if (wx1 != 0.0 && wy1 != 0.0) ok = regrid_tap(src, gws, ghs, nodata, j + 1.0, i + 1.0, z11) && ok;
    float res = nodata;
    if (ok) {
        const bool x_first = wx0 == 1.0 && wx1 == 0.0, x_second = wx0 == 0.0 && wx1 == 1.0;
        const bool y_first = wy0 == 1.0 && wy1 == 0.0, y_second = wy0 == 0.0 && wy1 == 1.0;
        if ((x_first || x_second) && (y_first || y_second)) {                 // one tap with the weight 1
            const float t = y_first ? (x_first ? z00 : z01) : (x_first ? z10 : z11);
            res = dz == 0.0 ? t : (float)((double)t + dz);
        } else {
            const double top = wx0 * (double)z00 + wx1 * (double)z01;
            const double bottom = wx0 * (double)z10 + wx1 * (double)z11;
            res = (float)(wy0 * top + wy1 * bottom + dz);
        }
    }
    out[cell] = res;
}

static const char* grid4_check(const double* g)
{
    if (!isfinite(g[0]) || !isfinite(g[1])) return "grid origin must be finite";
    if (!(isfinite(g[2]) && isfinite(g[3]) && g[2] > 0.0 && g[3] > 0.0)) return "grid resolutions must be finite and > 0";
    return nullptr;
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT size_t smvs_dsm_shift_workspace_bytes(int gwa, int gha, int gwb, int ghb, int radius)
{
    using namespace smvs;
    if (grid_check(gwa, gha) || grid_check(gwb, ghb) || radius < 0 || radius > SHIFT_MAX_RADIUS) return 0;
    return shift_plan(gwb, ghb, radius).bytes;
}

SMVS_EXPORT int smvs_dsm_shift_stats(const float* a, int gwa, int gha, const float* b, int gwb, int ghb, float nodata,
                                     int ox, int oy, int radius, double dz0, double trim,
                                     long long* stats, void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!a || !b || !stats || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = grid_check(gwa, gha)) return fail(SMVS_ERR_ARG, "a: %s", msg);
    if (const char* msg = grid_check(gwb, ghb)) return fail(SMVS_ERR_ARG, "b: %s", msg);
    if (radius < 0 || radius > SHIFT_MAX_RADIUS) return fail(SMVS_ERR_ARG, "radius must be in 0 .. %d, got %d", SHIFT_MAX_RADIUS, radius);
    if (ox <= -(1 << 30) || ox >= (1 << 30) || oy <= -(1 << 30) || oy >= (1 << 30))
        return fail(SMVS_ERR_ARG, "offset out of range: |ox|, |oy| must be below 2^30, got %d, %d", ox, oy);
    if (!isfinite(dz0)) return fail(SMVS_ERR_ARG, "dz0 must be finite");
    if (!(trim > 0.0 && trim <= 256.0)) return fail(SMVS_ERR_ARG, "trim must be in (0, 256], got %g", trim);
    const ShiftPlan p = shift_plan(gwb, ghb, radius);
    if (workspace_bytes < p.bytes) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, p.bytes);
    const size_t na = (size_t)gwa * gha * 4, nb = (size_t)gwb * ghb * 4, ns = (size_t)p.nshift * 3 * sizeof(long long);
    if (dsm_overlap(stats, ns, a, na) || dsm_overlap(stats, ns, b, nb)) return fail(SMVS_ERR_ARG, "stats aliases a or b");
    if (dsm_overlap(workspace, p.bytes, a, na) || dsm_overlap(workspace, p.bytes, b, nb) || dsm_overlap(workspace, p.bytes, stats, ns))
        return fail(SMVS_ERR_ARG, "workspace aliases a, b or stats");
    hipStream_t s = (hipStream_t)stream;
    long long* partial = (long long*)workspace;
    const dim3 grid(p.groups), block(SHIFT_THREADS);
#define SMVS_SHIFT_LAUNCH(NS)                                                                                                   \
    hipLaunchKernelGGL(dsm_shift_acc<NS>, grid, block, p.lds_bytes, s, a, gwa, gha, b, gwb, ghb, nodata, ox, oy, radius, dz0,   \
                       trim, p.ntx, p.ntiles, p.lanes_per_part, partial)
    switch (p.per_lane) {
        case 1: SMVS_SHIFT_LAUNCH(1); break;
        case 2: SMVS_SHIFT_LAUNCH(2); break;
        case 3: SMVS_SHIFT_LAUNCH(3); break;
        case 5: SMVS_SHIFT_LAUNCH(5); break;
        case 9: SMVS_SHIFT_LAUNCH(9); break;
        case 13: SMVS_SHIFT_LAUNCH(13); break;
        default: SMVS_SHIFT_LAUNCH(17); break;
    }
#undef SMVS_SHIFT_LAUNCH
    int rc;
    if ((rc = check_launch("dsm_shift_acc"))) return rc;
    const unsigned nvalues = (unsigned)p.nshift * 3u;
    hipLaunchKernelGGL(dsm_shift_fold, dim3((nvalues + SHIFT_THREADS - 1) / SHIFT_THREADS), block, 0, s, partial, p.groups, nvalues, stats);
    return check_launch("dsm_shift_fold");
}

SMVS_EXPORT int smvs_dsm_regrid(const float* src, int gws, int ghs, const double* grid4_src, float nodata,
                                const double* grid4_dst, int gwd, int ghd, int mode, double dz, float* out, void* stream)
{
    using namespace smvs;
    if (!src || !grid4_src || !grid4_dst || !out) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = grid_check(gws, ghs)) return fail(SMVS_ERR_ARG, "source: %s", msg);
    if (const char* msg = grid_check(gwd, ghd)) return fail(SMVS_ERR_ARG, "destination: %s", msg);
    if (const char* msg = grid4_check(grid4_src)) return fail(SMVS_ERR_ARG, "source %s", msg);
    if (const char* msg = grid4_check(grid4_dst)) return fail(SMVS_ERR_ARG, "destination %s", msg);
    if (mode != 0 && mode != 1) return fail(SMVS_ERR_ARG, "mode must be 0 (nearest) or 1 (bilinear), got %d", mode);
    if (!isfinite(dz)) return fail(SMVS_ERR_ARG, "dz must be finite");
    if (dsm_overlap(src, (size_t)gws * ghs * 4, out, (size_t)gwd * ghd * 4)) return fail(SMVS_ERR_ARG, "out aliases src");
    const Grid4 gs = {grid4_src[0], grid4_src[1], grid4_src[2], grid4_src[3]}, gd = {grid4_dst[0], grid4_dst[1], grid4_dst[2], grid4_dst[3]};
    const unsigned cells = (unsigned)gwd * (unsigned)ghd;
    hipLaunchKernelGGL(dsm_regrid, dim3((cells + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, src, gws, ghs, gs, nodata, gd, gwd, ghd,
                       mode, dz, out);
    return check_launch("dsm_regrid");
}

}  // extern "C"
