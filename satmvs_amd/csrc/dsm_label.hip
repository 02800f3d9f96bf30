// dsm_label.hip -- connected objects of a mask on a DSM's grid and their statistics ("Objects";
// include/satmvs.h for the rules).
//
//   smvs_dsm_label        mask (gh, gw) uint8 -> labels 1 .. n in raster order of every component's first cell, 0 = background
//   smvs_dsm_label_stats  area, bounding box, row / column sums and, with a value grid, count, lowest, highest and the exact
//                         fixed-point sum of the valid values of every label
//
// Labelling is a union-find over linear cell indices whose parent array is the `labels` buffer itself: parent[c] <= c at every
// moment, -1 at background cells.  (a) dsm_label_tile: a workgroup labels a 64 x 16 tile in LDS, row runs first (one ballot
// per row), then the runs of adjacent rows united with LDS min atomics; every foreground cell gets the global index of the
// first cell of its tile-local component.  (b) dsm_label_border: one lane per cell beside a tile edge unites it with its
// neighbours across the edge (the corner diagonals included) by 32-bit min atomics, the higher root under the lower.  (c)
// dsm_label_flatten: every cell takes its root.  (d) roots are flagged, ranked by a three-level exclusive scan of 2048-cell
// blocks (2048^3 > 2^31), and every cell takes rank[root] + 1.
// A union only ever lowers a parent and every component ends as one tree, so its root is its lowest index, the first cell in
// raster order, under any order of the atomics; the ranks are integer prefix sums in raster order.  The result depends on the
// mask alone.
//
// The loops are bounded by construction: a find follows parents and every step must strictly lower the index (parent < cell
// for a cell that is not its own root), so a find from cell x ends within x steps; a union lowers max(a, b) with every
// retry, so it ends within max(a, b) steps.  A step that does not lower the index (a parent above its cell, or a negative
// one) can only come from a damaged parent array: the lane stops there, sets the error word, and dsm_label_final writes
// n = -1.  No loop can spin and no index leaves [0, cell].
#include <limits.h>
#include <stdint.h>

#include "dsm_common.h"
#include "dsm_unionfind.h"
#include "smvs_host.h"

namespace smvs {

constexpr int LABEL_TW = 64, LABEL_TH = 16, LABEL_THREADS = 256;        // a tile row is one wave: the row runs come from a ballot
constexpr int SCAN_PER_THREAD = 8, SCAN_BLOCK = LABEL_THREADS * SCAN_PER_THREAD;     // 2048 cells per workgroup
constexpr int STATS_ROWS = 16;                               // rows of the 64-column strip one wave of the statistics walks down

// label_find and label_union (dsm_unionfind.h) are the loops the paragraph above argues about.

// (a) One 64 x 16 tile.  Wave w labels rows w, w + 4, ... : lane = column.
__global__ __launch_bounds__(LABEL_THREADS)
void dsm_label_tile(const unsigned char* __restrict__ mask, int gw, int gh, int conn8, int* __restrict__ parent, int* err)
{
    __shared__ int L[LABEL_TW * LABEL_TH];
    const unsigned ntx = (unsigned)((gw + LABEL_TW - 1) / LABEL_TW);
    const int tx0 = (int)(blockIdx.x % ntx) * LABEL_TW, ty0 = (int)(blockIdx.x / ntx) * LABEL_TH;
    const int lx = threadIdx.x % LABEL_TW, x = tx0 + lx;
    for (int ly = threadIdx.x / LABEL_TW; ly < LABEL_TH; ly += LABEL_THREADS / LABEL_TW) {
        const int y = ty0 + ly;
        const bool fg = x < gw && y < gh && mask[(size_t)y * gw + x] != 0;
        const unsigned long long row = __ballot(fg);
        const unsigned long long gaps = ~row & ((1ull << lx) - 1ull);                // background cells left of this one
        const int start = gaps ? 64 - __clzll((long long)gaps) : 0;                  // first cell of this cell's run
        L[ly * LABEL_TW + lx] = fg ? ly * LABEL_TW + start : -1;
    }
    __syncthreads();
    // a run meets the row above: once per stretch of common columns (N), and at its ends over the diagonals (NW, NE)
    for (int i = threadIdx.x + LABEL_TW; i < LABEL_TW * LABEL_TH; i += LABEL_THREADS) {
        if (L[i] < 0) continue;                              // the sign of a cell never changes
        const bool n = L[i - LABEL_TW] >= 0;
        const bool w = lx > 0 && L[i - 1] >= 0, nw = lx > 0 && L[i - LABEL_TW - 1] >= 0;
        const bool ne = lx < LABEL_TW - 1 && L[i - LABEL_TW + 1] >= 0;
        if (n && !(w && nw)) label_union<true>(L, i, i - LABEL_TW, err);
        if (conn8 && !n) {
            if (nw && !w) label_union<true>(L, i, i - LABEL_TW - 1, err);
            if (ne) label_union<true>(L, i, i - LABEL_TW + 1, err);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < LABEL_TW * LABEL_TH; i += LABEL_THREADS) {
        const int y = ty0 + i / LABEL_TW;
        if (x >= gw || y >= gh) continue;
        int p = -1;
        if (L[i] >= 0) {
            const int r = label_find<true>(L, i, err);       // the lowest local index is the lowest global index of the tile
            p = (ty0 + r / LABEL_TW) * gw + tx0 + r % LABEL_TW;
        }
        parent[(size_t)y * gw + x] = p;
    }
}

// (b) Lanes 0 .. nh - 1: the cells of the first row of every tile row but the topmost, united with N (and NW, NE).  Lanes nh
// .. nh + nv - 1: the cells of the first column of every tile column but the leftmost, united with W (and NW, SW).  Every
// pair of adjacent cells in different tiles is one of these.
__global__ __launch_bounds__(LABEL_THREADS)
void dsm_label_border(int* parent, int gw, int gh, int conn8, unsigned nh, unsigned nv, int* err)
{
    const unsigned t = blockIdx.x * (unsigned)LABEL_THREADS + threadIdx.x;
    if (t >= nh + nv) return;
    int x, y;
    const bool horizontal = t < nh;
    if (horizontal) {
        y = (int)(t / (unsigned)gw + 1u) * LABEL_TH;
        x = (int)(t % (unsigned)gw);
    } else {
        const unsigned u = t - nh;
        x = (int)(u / (unsigned)gh + 1u) * LABEL_TW;
        y = (int)(u % (unsigned)gh);
    }
    const int c = y * gw + x;
    if (parent[c] < 0) return;                               // tile roots from (a): written before this launch, never negative later
    if (horizontal) {
        const int up = c - gw;
        if (parent[up] >= 0) label_union<false>(parent, c, up, err);
        if (conn8) {
            if (x > 0 && parent[up - 1] >= 0) label_union<false>(parent, c, up - 1, err);
            if (x + 1 < gw && parent[up + 1] >= 0) label_union<false>(parent, c, up + 1, err);
        }
    } else {
        if (parent[c - 1] >= 0) label_union<false>(parent, c, c - 1, err);
        if (conn8) {
            if (y > 0 && parent[c - gw - 1] >= 0) label_union<false>(parent, c, c - gw - 1, err);
            if (y + 1 < gh && parent[c + gw - 1] >= 0) label_union<false>(parent, c, c + gw - 1, err);
        }
    }
}

// (c) Every cell takes its root.  Other lanes may read this cell's parent meanwhile: they see the old parent or the root,
// both in the tree and both below the cell, and a root's own entry is never written.
__global__ __launch_bounds__(LABEL_THREADS)
void dsm_label_flatten(int* parent, unsigned ncells, int* err)
{
    const unsigned c = blockIdx.x * (unsigned)LABEL_THREADS + threadIdx.x;
    if (c >= ncells) return;
    const int p = ld_agent(parent + c);
    if (p < 0 || p == (int)c) return;
    const int r = label_find<false>(parent, p, err);
    if (r != p) __hip_atomic_store(parent + c, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Exclusive scan of the workgroup's 256 per-thread counts; the total comes back in every lane.
__device__ __forceinline__ int block_exclusive(int v, int& total)
{
    __shared__ int wave_sum[LABEL_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < LABEL_THREADS / 64; ++k) {
        const int s = wave_sum[k];
        if (k < wave) before += s;
        total += s;
    }
    return before + inc - v;
}

// (d1) Flags of 2048 cells (cell == its parent), ranked within the block; rank is written at the roots only.
__global__ __launch_bounds__(LABEL_THREADS)
void dsm_label_rank(const int* __restrict__ parent, unsigned ncells, int* __restrict__ rank, int* __restrict__ sums)
{
    const unsigned c0 = blockIdx.x * (unsigned)SCAN_BLOCK + threadIdx.x * (unsigned)SCAN_PER_THREAD;
    int p[SCAN_PER_THREAD];
    if (c0 < ncells && ncells - c0 >= (unsigned)SCAN_PER_THREAD && ((uintptr_t)parent & 15) == 0) {       // c0 is a multiple of 8
        const int4 a = *(const int4*)(parent + c0), b = *(const int4*)(parent + c0 + 4);
        p[0] = a.x; p[1] = a.y; p[2] = a.z; p[3] = a.w; p[4] = b.x; p[5] = b.y; p[6] = b.z; p[7] = b.w;
    } else {
#pragma unroll
        for (int k = 0; k < SCAN_PER_THREAD; ++k) p[k] = (c0 < ncells && (unsigned)k < ncells - c0) ? parent[c0 + k] : -1;
    }
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < SCAN_PER_THREAD; ++k) cnt += p[k] == (int)(c0 + k);
    int total;
    int at = block_exclusive(cnt, total);
#pragma unroll
    for (int k = 0; k < SCAN_PER_THREAD; ++k)
        if (p[k] == (int)(c0 + k)) rank[c0 + k] = at++;
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// (d2) In-place exclusive scan of n sums in blocks of 2048; the block totals go one level up.
__global__ __launch_bounds__(LABEL_THREADS)
void dsm_label_scan(int* __restrict__ a, unsigned n, int* __restrict__ sums)
{
    const unsigned c0 = blockIdx.x * (unsigned)SCAN_BLOCK + threadIdx.x * (unsigned)SCAN_PER_THREAD;
    int v[SCAN_PER_THREAD], cnt = 0;
#pragma unroll
    for (int k = 0; k < SCAN_PER_THREAD; ++k) {
        v[k] = (c0 < n && (unsigned)k < n - c0) ? a[c0 + k] : 0;
        cnt += v[k];
    }
    int total;
    int at = block_exclusive(cnt, total);
#pragma unroll
    for (int k = 0; k < SCAN_PER_THREAD; ++k) {
        if (c0 < n && (unsigned)k < n - c0) a[c0 + k] = at;
        at += v[k];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// (d3) label = rank of the root in raster order + 1, in place over the parents; n, or -1 after a bounded loop gave up.
__global__ __launch_bounds__(LABEL_THREADS)
void dsm_label_final(int* __restrict__ labels, unsigned ncells, const int* __restrict__ rank, const int* __restrict__ s1,
                     const int* __restrict__ s2, const int* __restrict__ total_err, int* __restrict__ n_out)
{
    const unsigned c = blockIdx.x * (unsigned)LABEL_THREADS + threadIdx.x;
    if (c == 0) *n_out = total_err[1] ? -1 : total_err[0];
    if (c >= ncells) return;
    const int p = labels[c];                                 // this lane's own cell: no other lane reads or writes it
    int lab = 0;
    if (p >= 0 && (unsigned)p <= c) lab = rank[p] + s1[(unsigned)p / SCAN_BLOCK] + s2[(unsigned)p / SCAN_BLOCK / SCAN_BLOCK] + 1;
    labels[c] = lab;
}

// ---- statistics ------------------------------------------------------------------------------------------------------------
// What a lane holds of one label: sums, extremes, counts.  Integers only, so any grouping gives the same bits.
struct LabelAcc {
    int area, r0, c0, r1, c1, nvalid;
    unsigned kmin, kmax;
    long long rs, cs, q;

    __device__ __forceinline__ void clear()
    {
        area = 0; r0 = INT_MAX; c0 = INT_MAX; r1 = -1; c1 = -1; nvalid = 0;
        kmin = 0xffffffffu; kmax = 0u; rs = 0; cs = 0; q = 0;
    }
    __device__ __forceinline__ void add(const LabelAcc& o)
    {
        area += o.area; r0 = min(r0, o.r0); c0 = min(c0, o.c0); r1 = max(r1, o.r1); c1 = max(c1, o.c1); nvalid += o.nvalid;
        kmin = min(kmin, o.kmin); kmax = max(kmax, o.kmax); rs += o.rs; cs += o.cs; q += o.q;
    }
    __device__ __forceinline__ LabelAcc down(int d) const
    {
        LabelAcc o;
        o.area = __shfl_down(area, d); o.r0 = __shfl_down(r0, d); o.c0 = __shfl_down(c0, d); o.r1 = __shfl_down(r1, d);
        o.c1 = __shfl_down(c1, d); o.nvalid = __shfl_down(nvalid, d); o.kmin = __shfl_down(kmin, d); o.kmax = __shfl_down(kmax, d);
        o.rs = __shfl_down(rs, d); o.cs = __shfl_down(cs, d); o.q = __shfl_down(q, d);
        return o;
    }
};

struct LabelStatsOut {
    int *area, *bbox;
    unsigned long long *rc_sum, *qsum;
    int* nvalid;
    unsigned *kmin, *kmax;                                   // vmin / vmax hold keys until dsm_label_stats_finish
};

// Hand the accumulators of the lanes in `give` to memory.  Lanes side by side that give the same label form a run; the run is
// reduced onto its first lane (steps of 1, 2, ... 32 lanes: a lane d further on belongs to the run iff it has the same run
// start, runs being contiguous) and that lane alone goes to memory.  A wave whose lanes all give one label -- the inside of an
// object -- is one run: one atomic per field and wave.
__device__ __forceinline__ void label_stats_flush(LabelAcc& acc, int lab, bool give, bool has_values, const LabelStatsOut& o)
{
    const int lane = threadIdx.x & 63;
    const int prev = __shfl_up(lab, 1);
    const unsigned long long gives = __ballot(give);
    const bool head = give && (lane == 0 || !((gives >> (lane - 1)) & 1ull) || prev != lab);
    const unsigned long long heads = __ballot(head);
    const unsigned long long upto = heads & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));      // heads at or before this lane
    const int start = give && upto ? 63 - __clzll((long long)upto) : -1 - lane;                  // lanes that give nothing: unique
    LabelAcc r = acc;
    if (!give) r.clear();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const LabelAcc n = r.down(d);
        const int nstart = __shfl_down(start, d);
        if (lane + d < 64 && nstart == start) r.add(n);
    }
    if (head && r.area > 0) {
        const int k = lab - 1;
        atomicAdd(o.area + k, r.area);
        atomicMin(o.bbox + 4 * k, r.r0);
        atomicMin(o.bbox + 4 * k + 1, r.c0);
        atomicMax(o.bbox + 4 * k + 2, r.r1);
        atomicMax(o.bbox + 4 * k + 3, r.c1);
        atomicAdd(o.rc_sum + 2 * k, (unsigned long long)r.rs);
        atomicAdd(o.rc_sum + 2 * k + 1, (unsigned long long)r.cs);
        if (has_values && r.nvalid > 0) {
            atomicAdd(o.nvalid + k, r.nvalid);
            atomicMin(o.kmin + k, r.kmin);
            atomicMax(o.kmax + k, r.kmax);
            atomicAdd(o.qsum + k, (unsigned long long)r.q);
        }
    }
    if (give) acc.clear();
}

__global__ __launch_bounds__(LABEL_THREADS)
void dsm_label_stats_init(int n, bool has_values, LabelStatsOut o)
{
    const int k = blockIdx.x * LABEL_THREADS + threadIdx.x;
    if (k >= n) return;
    o.area[k] = 0;
    o.bbox[4 * k] = INT_MAX; o.bbox[4 * k + 1] = INT_MAX; o.bbox[4 * k + 2] = -1; o.bbox[4 * k + 3] = -1;
    o.rc_sum[2 * k] = 0; o.rc_sum[2 * k + 1] = 0;
    if (has_values) {
        o.nvalid[k] = 0; o.kmin[k] = 0xffffffffu; o.kmax[k] = 0u; o.qsum[k] = 0;
    }
}

// A wave walks down a strip of 64 columns and STATS_ROWS rows, lane = column.  A lane keeps accumulating while the label in
// its column stays; the lanes whose label changes flush what they hold first (label_stats_flush), and every lane at the end.
__global__ __launch_bounds__(LABEL_THREADS)
void dsm_label_stats_acc(const int* __restrict__ labels, const float* __restrict__ values, int gw, int gh, float nodata, int n, LabelStatsOut o)
{
    const unsigned nsx = (unsigned)((gw + 63) / 64);
    const unsigned strip = blockIdx.x * (unsigned)(LABEL_THREADS / 64) + (threadIdx.x >> 6);
    const int x = (int)(strip % nsx) * 64 + (int)(threadIdx.x & 63), y0 = (int)(strip / nsx) * STATS_ROWS;
    if (y0 >= gh) return;                                    // whole waves only
    const bool has_values = values != nullptr;
    LabelAcc acc;
    acc.clear();
    int held = 0;
    const int y1 = min(y0 + STATS_ROWS, gh);
    for (int y = y0; y < y1; ++y) {
        int lab = 0;
        float v = 0.0f;
        if (x < gw) {
            const size_t c = (size_t)y * gw + x;
            lab = labels[c];
            if ((unsigned)lab - 1u >= (unsigned)n) lab = 0;              // 0, negative, above n: nothing
            else if (has_values) v = values[c];
        }
        const bool change = lab != held;
        if (__any(change && held != 0)) label_stats_flush(acc, held, change && held != 0, has_values, o);
        held = lab;
        if (lab != 0) {
            LabelAcc one;
            one.area = 1; one.r0 = one.r1 = y; one.c0 = one.c1 = x; one.rs = y; one.cs = x;
            one.nvalid = 0; one.kmin = 0xffffffffu; one.kmax = 0u; one.q = 0;
            if (has_values && dsm_cell_valid(v, nodata)) {
                one.nvalid = 1;
                one.kmin = one.kmax = f2key(v);
                one.q = __double2ll_rn(fmin(fmax((double)v, -2097152.0), 2097152.0) * 1024.0);
            }
            acc.add(one);
        }
    }
    if (__any(held != 0)) label_stats_flush(acc, held, held != 0, has_values, o);
}

__global__ __launch_bounds__(LABEL_THREADS)
void dsm_label_stats_finish(int n, float nodata, const int* __restrict__ nvalid, unsigned* kmin, unsigned* kmax)
{
    const int k = blockIdx.x * LABEL_THREADS + threadIdx.x;
    if (k >= n) return;
    const bool any = nvalid[k] > 0;
    const float lo = any ? key2f(kmin[k]) : nodata, hi = any ? key2f(kmax[k]) : nodata;
    ((float*)kmin)[k] = lo;
    ((float*)kmax)[k] = hi;
}

struct LabelWorkspace { size_t rank, s1, s2, tail, bytes; unsigned nb1, nb2; };

static LabelWorkspace label_workspace(size_t ncells)
{
    LabelWorkspace w;
    w.nb1 = (unsigned)((ncells + SCAN_BLOCK - 1) / SCAN_BLOCK);
    w.nb2 = (w.nb1 + SCAN_BLOCK - 1) / SCAN_BLOCK;           // <= 512: the third level is one block
    w.rank = 0;
    w.s1 = w.rank + align256(ncells * sizeof(int));
    w.s2 = w.s1 + align256((size_t)w.nb1 * sizeof(int));
    w.tail = w.s2 + align256((size_t)w.nb2 * sizeof(int));   // [0] the total, [1] the error word
    w.bytes = w.tail + 256;
    return w;
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT size_t smvs_dsm_label_workspace_bytes(int gw, int gh)
{
    using namespace smvs;
    if (grid_check(gw, gh)) return 0;
    return label_workspace((size_t)gw * gh).bytes;
}

SMVS_EXPORT int smvs_dsm_label(const unsigned char* mask, int gw, int gh, int connectivity, int* labels, int* n_out,
                               void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!mask || !labels || !n_out || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (connectivity != 4 && connectivity != 8) return fail(SMVS_ERR_ARG, "connectivity must be 4 or 8, got %d", connectivity);
    const size_t ncells = (size_t)gw * gh;
    const LabelWorkspace w = label_workspace(ncells);
    if (workspace_bytes < w.bytes) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, w.bytes);
    if (dsm_overlap(mask, ncells, labels, ncells * 4)) return fail(SMVS_ERR_ARG, "labels aliases mask");
    if (dsm_overlap(mask, ncells, n_out, 4) || dsm_overlap(labels, ncells * 4, n_out, 4)) return fail(SMVS_ERR_ARG, "n_out aliases mask or labels");
    if (dsm_overlap(mask, ncells, workspace, w.bytes) || dsm_overlap(labels, ncells * 4, workspace, w.bytes) || dsm_overlap(n_out, 4, workspace, w.bytes))
        return fail(SMVS_ERR_ARG, "workspace aliases mask, labels or n_out");
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)workspace;
    int *rank = (int*)(base + w.rank), *s1 = (int*)(base + w.s1), *s2 = (int*)(base + w.s2), *tail = (int*)(base + w.tail);
    int* err = tail + 1;
    const int conn8 = connectivity == 8;
    if (hipMemsetAsync(tail, 0, 2 * sizeof(int), s) != hipSuccess) return check_launch("dsm_label (clearing the error word)");
    const unsigned ntx = (unsigned)((gw + LABEL_TW - 1) / LABEL_TW), nty = (unsigned)((gh + LABEL_TH - 1) / LABEL_TH);
    int rc;
    hipLaunchKernelGGL(dsm_label_tile, dim3(ntx * nty), dim3(LABEL_THREADS), 0, s, mask, gw, gh, conn8, labels, err);
    if ((rc = check_launch("dsm_label_tile"))) return rc;
    const unsigned nh = (nty - 1) * (unsigned)gw, nv = (ntx - 1) * (unsigned)gh;         // both below 2^31 / 16
    if (nh + nv) {
        hipLaunchKernelGGL(dsm_label_border, dim3((nh + nv + LABEL_THREADS - 1) / LABEL_THREADS), dim3(LABEL_THREADS), 0, s, labels, gw, gh, conn8, nh, nv, err);
        if ((rc = check_launch("dsm_label_border"))) return rc;
    }
    const unsigned cell_blocks = (unsigned)((ncells + LABEL_THREADS - 1) / LABEL_THREADS);
    hipLaunchKernelGGL(dsm_label_flatten, dim3(cell_blocks), dim3(LABEL_THREADS), 0, s, labels, (unsigned)ncells, err);
    if ((rc = check_launch("dsm_label_flatten"))) return rc;
    hipLaunchKernelGGL(dsm_label_rank, dim3(w.nb1), dim3(LABEL_THREADS), 0, s, labels, (unsigned)ncells, rank, s1);
    if ((rc = check_launch("dsm_label_rank"))) return rc;
    hipLaunchKernelGGL(dsm_label_scan, dim3(w.nb2), dim3(LABEL_THREADS), 0, s, s1, w.nb1, s2);
    if ((rc = check_launch("dsm_label_scan (block sums)"))) return rc;
    hipLaunchKernelGGL(dsm_label_scan, dim3(1), dim3(LABEL_THREADS), 0, s, s2, w.nb2, tail);
    if ((rc = check_launch("dsm_label_scan (top)"))) return rc;
    hipLaunchKernelGGL(dsm_label_final, dim3(cell_blocks), dim3(LABEL_THREADS), 0, s, labels, (unsigned)ncells, rank, s1, s2, tail, n_out);
    return check_launch("dsm_label_final");
}

SMVS_EXPORT int smvs_dsm_label_stats(const int* labels, const float* values, int gw, int gh, float nodata, int n,
                                     int* area, int* bbox, long long* rc_sum,
                                     int* nvalid, float* vmin, float* vmax, long long* qsum, void* stream)
{
    using namespace smvs;
    if (!labels || !area || !bbox || !rc_sum) return fail(SMVS_ERR_ARG, "null pointer argument");
    const bool has_values = values != nullptr;
    if (has_values && (!nvalid || !vmin || !vmax || !qsum)) return fail(SMVS_ERR_ARG, "values without nvalid, vmin, vmax and qsum");
    if (!has_values && (nvalid || vmin || vmax || qsum)) return fail(SMVS_ERR_ARG, "nvalid, vmin, vmax or qsum without values");
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (n < 0) return fail(SMVS_ERR_ARG, "n must be >= 0, got %d", n);
    if (n == 0) return SMVS_OK;
    const size_t ncells = (size_t)gw * gh, m = (size_t)n;
    const struct { const void* p; size_t bytes; const char* name; } buf[] = {
        {labels, ncells * 4, "labels"}, {values, has_values ? ncells * 4 : 0, "values"},
        {area, m * 4, "area"}, {bbox, m * 16, "bbox"}, {rc_sum, m * 16, "rc_sum"},
        {nvalid, m * 4, "nvalid"}, {vmin, m * 4, "vmin"}, {vmax, m * 4, "vmax"}, {qsum, m * 8, "qsum"}};
    const int nbuf = has_values ? 9 : 5;
    for (int i = 2; i < nbuf; ++i)
        for (int j = 0; j < i; ++j)
            if (buf[j].p && dsm_overlap(buf[i].p, buf[i].bytes, buf[j].p, buf[j].bytes))
                return fail(SMVS_ERR_ARG, "%s aliases %s", buf[i].name, buf[j].name);
    hipStream_t s = (hipStream_t)stream;
    LabelStatsOut o = {area, bbox, (unsigned long long*)rc_sum, (unsigned long long*)qsum, nvalid, (unsigned*)vmin, (unsigned*)vmax};
    const unsigned label_blocks = ((unsigned)n + LABEL_THREADS - 1) / LABEL_THREADS;
    int rc;
    hipLaunchKernelGGL(dsm_label_stats_init, dim3(label_blocks), dim3(LABEL_THREADS), 0, s, n, has_values, o);
    if ((rc = check_launch("dsm_label_stats_init"))) return rc;
    const unsigned long long strips = (unsigned long long)((gw + 63) / 64) * (unsigned long long)((gh + STATS_ROWS - 1) / STATS_ROWS);
    hipLaunchKernelGGL(dsm_label_stats_acc, dim3((unsigned)((strips + LABEL_THREADS / 64 - 1) / (LABEL_THREADS / 64))), dim3(LABEL_THREADS), 0, s,
                       labels, values, gw, gh, nodata, n, o);
    if ((rc = check_launch("dsm_label_stats_acc"))) return rc;
    if (has_values) {
        hipLaunchKernelGGL(dsm_label_stats_finish, dim3(label_blocks), dim3(LABEL_THREADS), 0, s, n, nodata, nvalid, (unsigned*)vmin, (unsigned*)vmax);
        if ((rc = check_launch("dsm_label_stats_finish"))) return rc;
    }
    return SMVS_OK;
}

}  // extern "C"
