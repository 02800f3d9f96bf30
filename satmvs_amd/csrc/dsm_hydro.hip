// dsm_hydro.hip -- hydrology of a DTM on integer heights, exact ("Hydrology"; include/satmvs.h for the
// rule): depression filling as a flood key per cell, D8 directions from the keys, and accumulation and basins over any
// direction grid.
//
//   smvs_dsm_flood_begin      the keys as the relaxation starts: outlets final, the other valid cells +infinity, invalid all ones
//   smvs_dsm_flood_rounds     `rounds` global rounds; status <- the tiles that changed in the last one
//   smvs_dsm_flood_read       keys -> filled, depth, flat_dist
//   smvs_dsm_flow_dir         keys and the eight distances -> codes, one lane per cell
//   smvs_dsm_flow_accumulate  receivers, roots by pointer doubling, an Euler tour of the forest ranked by one more doubling
//   smvs_dsm_flow_basins      receivers, roots by pointer doubling, the roots numbered by a scan
//
// The flood.  A key is ((w + 2^31) << 32) | d, so the order of the pairs is the order of the words.  A round is one workgroup
// per tile of 32 x 32 cells: it loads the tile and a halo of one cell into LDS, lowers every cell that is neither an outlet nor
// invalid to max((q, 0), min over its neighbours of key + 1) until no cell of the tile moves (__syncthreads_or), and writes
// back the interior if anything moved.  Keys only fall and never pass below the solution, so a stale key read from a
// neighbouring tile, or from another wave in LDS, is an upper bound like any other; a key moves as one aligned 64-bit access.
// A round in which no tile moved has read final halos only: the grid is at the fixed point, which is unique.
// Every launch has one counter of the tiles that moved, cleared by the entry before its first launch.
//
// The forest.  recv[c] is the cell c drains into, D8_ROOT or D8_INVALID, and up[c] the root of every cell that has one; a cell
// whose up[c] is not a root is on a cycle or drains into one (dsm_flow.h has both and says why).  The tour: cell c has the elements
// 2 c (down) and 2 c + 1 (up); the successors follow from recv of the cell's and its receiver's neighbours alone; the weight
// sits on down.  A Wyllie doubling between two copies of (successor, suffix sum) runs ceil(log2(2 cells)) rounds, and
// acc(c) = S(down) - S(up).  The sums are unsigned 64-bit words (they wrap like the int64 they stand for); no atomics but an
// integer OR into the flag.  Workspace: 16 KB for the flood; 56 bytes per cell for the forest (recv 4, up 4, two copies of the
// tour's int32 successors 16 and of its 64-bit sums 32), of which the basins use the first 12 (their numbering takes the place
// of the tour) plus the scan's block sums.  No kernel uses scratch.
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "dsm_common.h"
#include "dsm_flow.h"
#include "dsm_scan.h"
#include "smvs_host.h"

namespace smvs {

typedef unsigned long long u64;

constexpr int HY_THREADS = D8_THREADS;
constexpr int HY_TILE = 32, HY_SPAN = HY_TILE + 2, HY_PITCH = HY_SPAN + 1;         // interior, with halo, LDS row in keys
constexpr int HY_ROWS = HY_THREADS / HY_TILE, HY_PER_THREAD = HY_TILE / HY_ROWS;  // 8 rows of lanes, 4 cells a lane
constexpr int HY_MAX_ROUNDS = 4096;
constexpr u64 HY_INVALID = ~0ull, HY_INF = 0xfffffffeull << 32;
constexpr int FL_END = -1;

__device__ __forceinline__ u64 hy_key(int w, unsigned d) { return (u64)((unsigned)w + 0x80000000u) << 32 | d; }
__device__ __forceinline__ int hy_w(u64 key) { return (int)((unsigned)(key >> 32) - 0x80000000u); }

// ---- the flood -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HY_THREADS)
void hy_begin(const float* __restrict__ dsm, int gw, int gh, float nodata, u64* __restrict__ keys)
{
    const unsigned n = (unsigned)gw * (unsigned)gh, i = blockIdx.x * (unsigned)HY_THREADS + threadIdx.x;
    if (i >= n) return;
    const int r = (int)(i / (unsigned)gw), c = (int)(i % (unsigned)gw);
    int q, qn;
    if (!dsm_quantum(dsm[i], nodata, q)) { keys[i] = HY_INVALID; return; }
    bool outlet = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int rr = r + d8_dr(k), cc = c + d8_dc(k);
        if (rr < 0 || rr >= gh || cc < 0 || cc >= gw) outlet = true;
        else if (!dsm_quantum(dsm[(size_t)rr * gw + cc], nodata, qn)) outlet = true;
    }
    keys[i] = outlet ? hy_key(q, 0) : HY_INF;
}

__global__ __launch_bounds__(HY_THREADS)
void hy_round(const float* __restrict__ dsm, int gw, int gh, float nodata, u64* keys, int* __restrict__ moved)
{
    __shared__ u64 tile[HY_SPAN * HY_PITCH];
    const unsigned across = ((unsigned)gw + HY_TILE - 1) / HY_TILE;               // the tiles in a row of tiles; the grid is 1-D
    const int r0 = (int)(blockIdx.x / across) * HY_TILE - 1, c0 = (int)(blockIdx.x % across) * HY_TILE - 1;       // the halo's corner
    for (int t = threadIdx.x; t < HY_SPAN * HY_SPAN; t += HY_THREADS) {
        const int lr = t / HY_SPAN, lc = t % HY_SPAN, r = r0 + lr, c = c0 + lc;
        tile[lr * HY_PITCH + lc] = (r >= 0 && r < gh && c >= 0 && c < gw) ? keys[(size_t)r * gw + c] : HY_INVALID;
    }
    __syncthreads();
    const int lc = 1 + (int)(threadIdx.x % HY_TILE), lrow = 1 + (int)(threadIdx.x / HY_TILE);
    u64 own[HY_PER_THREAD], floor_key[HY_PER_THREAD];
    bool open[HY_PER_THREAD];                                // neither invalid nor an outlet: the cells that move
#pragma unroll
    for (int j = 0; j < HY_PER_THREAD; ++j) {
        const int lr = lrow + j * HY_ROWS, at = lr * HY_PITCH + lc, r = r0 + lr, c = c0 + lc;
        own[j] = tile[at];
        bool all = own[j] != HY_INVALID;
#pragma unroll
        for (int k = 0; k < 8; ++k) all = all && tile[at + d8_dr(k) * HY_PITCH + d8_dc(k)] != HY_INVALID;
        int q = 0;
        open[j] = all && r < gh && c < gw && dsm_quantum(dsm[(size_t)r * gw + c], nodata, q);
        floor_key[j] = hy_key(q, 0);
    }
    bool any = false;
    int busy;
    do {
        busy = 0;
#pragma unroll
        for (int j = 0; j < HY_PER_THREAD; ++j) {
            if (!open[j]) continue;
            const int at = (lrow + j * HY_ROWS) * HY_PITCH + lc;
            u64 low = HY_INVALID;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const u64 v = tile[at + d8_dr(k) * HY_PITCH + d8_dc(k)];
                low = v < low ? v : low;
            }
            low += 1;                                        // one step more: no neighbour of an open cell is all ones, d < 2^30
            const u64 key = low > floor_key[j] ? low : floor_key[j];
            if (key < own[j]) {
                own[j] = key;
                tile[at] = key;
                busy = 1;
            }
        }
        any = any || busy;
        busy = __syncthreads_or(busy);
    } while (busy);
    const int tile_moved = __syncthreads_or(any);
    if (!tile_moved) return;
#pragma unroll
    for (int j = 0; j < HY_PER_THREAD; ++j)
        if (open[j]) keys[(size_t)(r0 + lrow + j * HY_ROWS) * gw + (c0 + lc)] = own[j];
    if (threadIdx.x == 0) atomicAdd(moved, 1);
}

__global__ void hy_status(const int* __restrict__ moved, int* __restrict__ status)
{
    if (threadIdx.x == 0) *status = *moved;
}

__global__ __launch_bounds__(HY_THREADS)
void hy_read(const float* __restrict__ dsm, int gw, int gh, float nodata, const u64* __restrict__ keys,
             float* __restrict__ filled, float* __restrict__ depth, int* __restrict__ flat_dist)
{
    const unsigned n = (unsigned)gw * (unsigned)gh, i = blockIdx.x * (unsigned)HY_THREADS + threadIdx.x;
    if (i >= n) return;
    const float z = dsm[i];
    const u64 key = keys[i];
    int q;
    const bool valid = dsm_quantum(z, nodata, q) && key != HY_INVALID;
    const int w = hy_w(key);
    if (filled) filled[i] = !valid ? nodata : w == q ? z : (float)((double)w / 256.0);
    if (depth) depth[i] = !valid ? nodata : (float)((double)((long long)w - q) / 256.0);
    if (flat_dist) flat_dist[i] = valid ? (int)(unsigned)key : -1;
}

// ---- directions ----------------------------------------------------------------------------------------------------------------
struct HyDist { double d[8]; };

__global__ __launch_bounds__(HY_THREADS)
void hy_dir(const u64* __restrict__ keys, int gw, int gh, HyDist dist, unsigned char* __restrict__ dir)
{
    const unsigned n = (unsigned)gw * (unsigned)gh, i = blockIdx.x * (unsigned)HY_THREADS + threadIdx.x;
    if (i >= n) return;
    const int r = (int)(i / (unsigned)gw), c = (int)(i % (unsigned)gw);
    const u64 own = keys[i];
    if (own == HY_INVALID) { dir[i] = 255; return; }
    const int w = hy_w(own);
    bool outlet = false;
    double steepest = 0.0;
    unsigned nearest = 0xffffffffu;
    int down = 0, level = 0;                                 // code of the steepest lower neighbour, of the nearest level one
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int rr = r + d8_dr(k), cc = c + d8_dc(k);
        const u64 v = (rr < 0 || rr >= gh || cc < 0 || cc >= gw) ? HY_INVALID : keys[(size_t)rr * gw + cc];
        if (v == HY_INVALID) { outlet = true; continue; }
        const int wn = hy_w(v);
        if (wn < w) {
            const double slope = __ddiv_rn((double)((long long)w - wn), dist.d[k]);
            if (slope > steepest) { steepest = slope; down = k + 1; }
        } else if (wn == w && (unsigned)v < nearest) {
            nearest = (unsigned)v;
            level = k + 1;
        }
    }
    dir[i] = outlet ? 0 : down ? down : level;               // no lower or level neighbour (not a fixed point's keys): a root
}

// ---- the forest ----------------------------------------------------------------------------------------------------------------
// Whether cell i has a code and a root; else what it is.
enum { FL_TREE = 0, FL_VOID, FL_CYCLIC };
__device__ __forceinline__ int fl_kind(const int* __restrict__ recv, const int* __restrict__ up, unsigned n, unsigned i, unsigned& root)
{
    if (recv[i] == D8_INVALID) return FL_VOID;
    root = (unsigned)up[i];
    return root < n && recv[root] == D8_ROOT ? FL_TREE : FL_CYCLIC;
}

// ---- accumulation --------------------------------------------------------------------------------------------------------------
// The first neighbour of cell p from direction k0 on that drains into p, as its down element; FL_END if there is none.
__device__ __forceinline__ int fl_child_from(const int* __restrict__ recv, int gw, int gh, int p, int k0)
{
    const int r = p / gw, c = p % gw;
    int found = FL_END;
#pragma unroll
    for (int k = 7; k >= 0; --k) {
        const int rr = r + d8_dr(k), cc = c + d8_dc(k);
        if (k < k0 || rr < 0 || rr >= gh || cc < 0 || cc >= gw) continue;
        const int child = rr * gw + cc;
        if (recv[child] == p) found = 2 * child;
    }
    return found;
}

__global__ __launch_bounds__(HY_THREADS)
void fl_tour(const unsigned char* __restrict__ dir, const int* __restrict__ weight, int gw, int gh,
             const int* __restrict__ recv, const int* __restrict__ up, int* __restrict__ succ, u64* __restrict__ sum)
{
    const unsigned n = (unsigned)gw * (unsigned)gh, i = blockIdx.x * (unsigned)HY_THREADS + threadIdx.x;
    if (i >= n) return;
    unsigned root;
    int after_down = FL_END, after_up = FL_END;
    u64 w = 0;
    if (fl_kind(recv, up, n, i, root) == FL_TREE) {
        w = weight ? (u64)(long long)weight[i] : 1ull;
        const int first = fl_child_from(recv, gw, gh, (int)i, 0);
        after_down = first != FL_END ? first : (int)(2 * i + 1);
        const int p = recv[i];
        if (p >= 0) {
            const int from_parent = ((int)dir[i] - 1 + 4) & 7;                  // the direction in which the receiver sees this cell
            const int sibling = fl_child_from(recv, gw, gh, p, from_parent + 1);
            after_up = sibling != FL_END ? sibling : 2 * p + 1;
        }
    }
    succ[2 * (size_t)i] = after_down;
    succ[2 * (size_t)i + 1] = after_up;
    sum[2 * (size_t)i] = w;
    sum[2 * (size_t)i + 1] = 0;
}

// One Wyllie round from one copy into the other: S'(e) = S(e) + S(succ e), succ'(e) = succ(succ e).
__global__ __launch_bounds__(HY_THREADS)
void fl_double(unsigned m, const int* __restrict__ succ, const u64* __restrict__ sum, int* __restrict__ succ_out, u64* __restrict__ sum_out)
{
    const unsigned e = blockIdx.x * (unsigned)HY_THREADS + threadIdx.x;
    if (e >= m) return;
    const unsigned s = (unsigned)succ[e];
    const bool on = s < m;
    sum_out[e] = sum[e] + (on ? sum[s] : 0ull);
    succ_out[e] = on ? succ[s] : FL_END;
}

__global__ __launch_bounds__(HY_THREADS)
void fl_acc(unsigned n, const int* __restrict__ recv, const int* __restrict__ up, const u64* __restrict__ sum,
            long long* __restrict__ acc, int* flag)
{
    const unsigned i = blockIdx.x * (unsigned)HY_THREADS + threadIdx.x;
    unsigned root;
    const int kind = i < n ? fl_kind(recv, up, n, i, root) : FL_VOID;
    if (__any(kind == FL_CYCLIC) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
    if (i >= n) return;
    acc[i] = kind == FL_VOID ? 0 : kind == FL_CYCLIC ? -1 : (long long)(sum[2 * (size_t)i] - sum[2 * (size_t)i + 1]);
}

// ---- basins --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HY_THREADS)
void fl_numbered(unsigned n, const unsigned char* __restrict__ pour, const int* __restrict__ recv, int* __restrict__ number)
{
    const unsigned i = blockIdx.x * (unsigned)HY_THREADS + threadIdx.x;
    if (i < n) number[i] = recv[i] == D8_ROOT && (!pour || pour[i]);
}

__global__ __launch_bounds__(HY_THREADS)
void fl_basin(unsigned n, const unsigned char* __restrict__ pour, const int* __restrict__ recv, const int* __restrict__ up,
              const int* __restrict__ number, int* __restrict__ basin, int* flag)
{
    const unsigned i = blockIdx.x * (unsigned)HY_THREADS + threadIdx.x;
    unsigned root = 0;
    const int kind = i < n ? fl_kind(recv, up, n, i, root) : FL_VOID;
    if (__any(kind == FL_CYCLIC) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
    if (i >= n) return;
    basin[i] = kind == FL_TREE && (!pour || pour[root]) ? number[root] + 1 : 0;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct FlowWorkspace { size_t recv, up, number, s1, s2, succ, sum, bytes; };

static FlowWorkspace flow_workspace(size_t n)
{
    FlowWorkspace w;
    const size_t nb1 = (n + OL_BLOCK - 1) / OL_BLOCK, nb2 = (nb1 + OL_BLOCK - 1) / OL_BLOCK;
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t here = at; at += align256(bytes); return here; };
    w.recv = take(n * 4);
    w.up = take(n * 4);
    w.s1 = take(nb1 * 4);
    w.s2 = take(nb2 * 4);
    w.number = at;                                           // the basins' numbering lies where the tour's first copy does
    w.succ = take(2 * n * 4 * 2);
    w.sum = take(2 * n * 8 * 2);
    w.bytes = at;
    return w;
}

// What the entries check alike: the grid, and that no two of the buffers given (null ones skipped; past the grid check none is
// empty) share a byte.
static int hydro_check(int gw, int gh, const DsmBuf* buf, int n_buf)
{
    if (const char* msg = d8_grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s (got %d x %d)", msg, gw, gh);
    const char* other = nullptr;
    if (const char* name = dsm_first_alias(buf, n_buf, other)) return fail(SMVS_ERR_ARG, "%s aliases %s", name, other);
    return SMVS_OK;
}

static size_t flood_workspace(void) { return align256((size_t)HY_MAX_ROUNDS * 4); }

}  // namespace smvs

extern "C" {

SMVS_EXPORT size_t smvs_dsm_flood_workspace_bytes(int gw, int gh)
{
    using namespace smvs;
    return d8_grid_check(gw, gh) ? 0 : flood_workspace();
}

SMVS_EXPORT int smvs_dsm_flood_begin(const float* dsm, int gw, int gh, float nodata, unsigned long long* keys,
                                     void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!dsm || !keys || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    const size_t n = gw > 0 && gh > 0 ? (size_t)gw * gh : 0;
    const DsmBuf buf[] = {{dsm, n * 4, "dsm"}, {keys, n * 8, "keys"}, {workspace, flood_workspace(), "workspace"}};
    if (int rc = hydro_check(gw, gh, buf, 3)) return rc;
    if (workspace_bytes < flood_workspace()) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, flood_workspace());
    hipStream_t s = (hipStream_t)stream;
    DSM_LAUNCH(hy_begin, n, HY_THREADS, s, dsm, gw, gh, nodata, keys);
    return SMVS_OK;
}

SMVS_EXPORT int smvs_dsm_flood_rounds(const float* dsm, int gw, int gh, float nodata, unsigned long long* keys, int rounds,
                                      int* status, void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!dsm || !keys || !status || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (rounds < 1 || rounds > HY_MAX_ROUNDS) return fail(SMVS_ERR_ARG, "rounds must be in 1 .. %d, got %d", HY_MAX_ROUNDS, rounds);
    const size_t n = gw > 0 && gh > 0 ? (size_t)gw * gh : 0;
    const DsmBuf buf[] = {{dsm, n * 4, "dsm"}, {keys, n * 8, "keys"}, {status, 4, "status"}, {workspace, flood_workspace(), "workspace"}};
    if (int rc = hydro_check(gw, gh, buf, 4)) return rc;
    if (workspace_bytes < flood_workspace()) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, flood_workspace());
    hipStream_t s = (hipStream_t)stream;
    int* moved = (int*)workspace;
    if (hipMemsetAsync(moved, 0, (size_t)rounds * 4, s) != hipSuccess) return check_launch("dsm_flood_rounds (clearing the counters)");
    const size_t tiles = (size_t)((gw + HY_TILE - 1) / HY_TILE) * (size_t)((gh + HY_TILE - 1) / HY_TILE);     // a workgroup each
    for (int k = 0; k < rounds; ++k) DSM_LAUNCH(hy_round, tiles * HY_THREADS, HY_THREADS, s, dsm, gw, gh, nodata, keys, moved + k);
    DSM_LAUNCH(hy_status, 1, 64, s, (const int*)(moved + rounds - 1), status);
    return SMVS_OK;
}

SMVS_EXPORT int smvs_dsm_flood_read(const float* dsm, int gw, int gh, float nodata, const unsigned long long* keys,
                                    float* filled, float* depth, int* flat_dist, void* stream)
{
    using namespace smvs;
    if (!dsm || !keys) return fail(SMVS_ERR_ARG, "null pointer argument");
    const size_t n = gw > 0 && gh > 0 ? (size_t)gw * gh : 0;
    const DsmBuf buf[] = {{dsm, n * 4, "dsm"}, {keys, n * 8, "keys"}, {filled, n * 4, "filled"}, {depth, n * 4, "depth"}, {flat_dist, n * 4, "flat_dist"}};
    if (int rc = hydro_check(gw, gh, buf, 5)) return rc;
    DSM_LAUNCH(hy_read, n, HY_THREADS, (hipStream_t)stream, dsm, gw, gh, nodata, keys, filled, depth, flat_dist);
    return SMVS_OK;
}

SMVS_EXPORT int smvs_dsm_flow_dir(const unsigned long long* keys, int gw, int gh, const double* dist, unsigned char* dir, void* stream)
{
    using namespace smvs;
    if (!keys || !dist || !dir) return fail(SMVS_ERR_ARG, "null pointer argument");
    HyDist d;
    for (int k = 0; k < 8; ++k) {
        if (!(isfinite(dist[k]) && dist[k] > 0.0)) return fail(SMVS_ERR_ARG, "dist[%d] must be finite and > 0, got %g", k, dist[k]);
        d.d[k] = dist[k];
    }
    const size_t n = gw > 0 && gh > 0 ? (size_t)gw * gh : 0;
    const DsmBuf buf[] = {{keys, n * 8, "keys"}, {dir, n, "dir"}};
    if (int rc = hydro_check(gw, gh, buf, 2)) return rc;
    DSM_LAUNCH(hy_dir, n, HY_THREADS, (hipStream_t)stream, keys, gw, gh, d, dir);
    return SMVS_OK;
}

SMVS_EXPORT size_t smvs_dsm_flow_workspace_bytes(int gw, int gh)
{
    using namespace smvs;
    return d8_grid_check(gw, gh) ? 0 : flow_workspace((size_t)gw * gh).bytes;
}

SMVS_EXPORT int smvs_dsm_flow_accumulate(const unsigned char* dir, const int* weight, int gw, int gh, long long* acc, int* flag,
                                         void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!dir || !acc || !flag || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    const size_t n = gw > 0 && gh > 0 ? (size_t)gw * gh : 0;
    const FlowWorkspace w = flow_workspace(n);
    const DsmBuf buf[] = {{dir, n, "dir"}, {weight, n * 4, "weight"}, {acc, n * 8, "acc"}, {flag, 4, "flag"}, {workspace, w.bytes, "workspace"}};
    if (int rc = hydro_check(gw, gh, buf, 5)) return rc;
    if (workspace_bytes < w.bytes) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, w.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)workspace;
    int *recv = (int*)(base + w.recv), *up = (int*)(base + w.up);
    int* succ[2] = {(int*)(base + w.succ), (int*)(base + w.succ) + 2 * n};
    u64* sum[2] = {(u64*)(base + w.sum), (u64*)(base + w.sum) + 2 * n};
    if (hipMemsetAsync(flag, 0, 4, s) != hipSuccess) return check_launch("dsm_flow_accumulate (clearing the flag)");
    int rc;
    if ((rc = d8_roots(dir, nullptr, gw, gh, recv, up, s))) return rc;
    DSM_LAUNCH(fl_tour, n, HY_THREADS, s, dir, weight, gw, gh, (const int*)recv, (const int*)up, succ[0], sum[0]);
    int at = 0;
    for (int k = 0, rounds = dsm_ceil_log2(2 * n); k < rounds; ++k, at ^= 1)
        DSM_LAUNCH(fl_double, 2 * n, HY_THREADS, s, (unsigned)(2 * n), (const int*)succ[at], (const u64*)sum[at], succ[at ^ 1], sum[at ^ 1]);
    DSM_LAUNCH(fl_acc, n, HY_THREADS, s, (unsigned)n, (const int*)recv, (const int*)up, (const u64*)sum[at], acc, flag);
    return SMVS_OK;
}

SMVS_EXPORT int smvs_dsm_flow_basins(const unsigned char* dir, const unsigned char* pour, int gw, int gh, int* basin, int* n_out,
                                     int* flag, void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!dir || !basin || !n_out || !flag || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    const size_t n = gw > 0 && gh > 0 ? (size_t)gw * gh : 0;
    const FlowWorkspace w = flow_workspace(n);
    const DsmBuf buf[] = {{dir, n, "dir"}, {pour, n, "pour"}, {basin, n * 4, "basin"}, {n_out, 4, "n_out"}, {flag, 4, "flag"}, {workspace, w.bytes, "workspace"}};
    if (int rc = hydro_check(gw, gh, buf, 6)) return rc;
    if (workspace_bytes < w.bytes) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, w.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)workspace;
    int *recv = (int*)(base + w.recv), *up = (int*)(base + w.up), *number = (int*)(base + w.number);
    if (hipMemsetAsync(flag, 0, 4, s) != hipSuccess) return check_launch("dsm_flow_basins (clearing the flag)");
    int rc;
    if ((rc = d8_roots(dir, pour, gw, gh, recv, up, s))) return rc;
    DSM_LAUNCH(fl_numbered, n, HY_THREADS, s, (unsigned)n, pour, (const int*)recv, number);
    if ((rc = ol_scan_exclusive(number, (unsigned)n, nullptr, (int*)(base + w.s1), (int*)(base + w.s2), n_out, s, "ol_scan (roots)"))) return rc;
    DSM_LAUNCH(fl_basin, n, HY_THREADS, s, (unsigned)n, pour, (const int*)recv, (const int*)up, (const int*)number, basin, flag);
    return SMVS_OK;
}

}  // extern "C"
