// dsm.hip -- DSM production: per-view height maps (image space, RPC) -> one height grid in map coordinates.
//
//   smvs_tm_project   Transverse Mercator (USGS series, Snyder, "Map Projections -- A Working Manual", pp. 60-64), float64,
//                     both directions; pinned by tests/golden/tm.npz (the reference's tools/Transverse_Mercator.py).
//   smvs_rpc_dsm_bin  one lane per pixel: (x, y, h) -> (lat, lon) through the inverse RPC the filter uses (rpc_photo2obj),
//                     -> (E, N) through the TM forward, -> grid cell; counts per cell accumulated with atomics.
//   smvs_dsm_reduce   exclusive scan of the counts, scatter of the heights into per-cell buckets, sort of every bucket on the
//                     order-preserving uint32 image of the float, then median / mean / min / max of the sorted bucket.
//
// Determinism: the only order-dependent steps are the atomics (which slot of its bucket a height lands in, which position a cell
// takes in a tier list).  Every bucket is sorted before it is reduced, equal keys are equal bits, and the reduction order of a
// bucket depends on its size alone, so the DSM is bit-identical from run to run and under any permutation of points or maps.
#include <math.h>

#include <algorithm>

#include "dsm_geo.h"
#include "smvs_device.h"
#include "smvs_host.h"

namespace smvs {

__global__ __launch_bounds__(256)
void tm_project_kernel(TmConst t, const double* __restrict__ a, const double* __restrict__ b,
                       double* __restrict__ o0, double* __restrict__ o1, size_t n, int dir)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double u, v;
    if (dir == 0) tm_forward(t, a[i], b[i], u, v);
    else tm_inverse(t, a[i], b[i], u, v);
    o0[i] = u;
    o1[i] = v;
}

// ---- wave helpers ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned lane_id() { return __lane_id(); }

// Runs of equal `key` among consecutive lanes: bit L of the result is set where lane L starts a run.
__device__ __forceinline__ unsigned long long run_heads(int key)
{
    const int prev = __shfl_up(key, 1);
    return __ballot(lane_id() == 0 || prev != key);
}

// Length of the run that starts at this lane (call on heads only).
__device__ __forceinline__ unsigned run_length(unsigned long long heads)
{
    const unsigned L = lane_id();
    const unsigned long long later = (L == 63) ? 0ull : (heads >> (L + 1)) << (L + 1);
    const unsigned next = later ? (unsigned)__builtin_ctzll(later) : 64u;
    return next - L;
}

// The lane that heads this lane's run.
__device__ __forceinline__ unsigned run_head(unsigned long long heads)
{
    const unsigned L = lane_id();
    const unsigned long long upto = (L == 63) ? heads : heads & ((2ull << L) - 1);
    return 63u - (unsigned)__builtin_clzll(upto);
}

// ---- bin pass --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void dsm_bin_kernel(const float* __restrict__ height, const unsigned char* __restrict__ mask, const double* __restrict__ rpc,
                    int H, int W, TmConst t, DsmGrid g, int gw, int gh,
                    int* __restrict__ cell, unsigned* __restrict__ count, double* __restrict__ east, double* __restrict__ north)
{
    const size_t n = (size_t)H * W;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = i < n;                       // no early return: the whole wave takes part in the run aggregation
    int c = -1;
    if (in) {
        const float hf = height[i];
        double E = __builtin_nan(""), N = __builtin_nan("");
        if (isfinite(hf) && (!mask || mask[i])) {
            const int y = (int)(i / W), x = (int)(i % W);
            const cgeo_t r = as_cgeo(rpc);
            double lat, lon;
            rpc_photo2obj(r, rpc_inv_image(r), (double)x, (double)y, (double)hf, lat, lon);
            tm_forward(t, lat, lon, E, N);
            // world-file convention, (e0, n0) = centre of cell (0, 0); IEEE quotients so numpy reproduces the cell from E / N
            const double col = floor((E - g.e0) / g.xres + 0.5);
            const double row = floor((g.n0 - N) / g.yres + 0.5);
            if (col >= 0.0 && col < (double)gw && row >= 0.0 && row < (double)gh)      // NaN fails every comparison
                c = (int)row * gw + (int)col;
        }
        cell[i] = c;
        if (east) { east[i] = E; north[i] = N; }
    }
    const unsigned long long heads = run_heads(c);
    if (c >= 0 && ((heads >> lane_id()) & 1ull)) atomicAdd(&count[c], run_length(heads));
}

// ---- reduce pass -----------------------------------------------------------------------------------------------------------
constexpr int SCAN_THREADS = 256, SCAN_ITEMS = 16, SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;
constexpr int TIER0_MAX = 32;         // one lane per cell, sorting network in registers
constexpr int TIER1_MAX = 4096;       // one workgroup per cell, bitonic sort in LDS
constexpr int TIER1_THREADS = 256, TIER2_THREADS = 1024, TIER2_WAVES = TIER2_THREADS / 64;
constexpr int TIER1_BLOCKS = 2048, TIER2_BLOCKS = 256;

// Bucket of cell c: [lo, lo + m) of the key array.  Clamped so that counts which do not match the cells (or that wrap) can
// neither read nor write outside the arrays: m never exceeds the slots the scatter could fill.
__device__ __forceinline__ unsigned bucket(const unsigned* __restrict__ offs, const unsigned* __restrict__ cursor, int c,
                                           unsigned n, unsigned& m)
{
    const unsigned lo = min(offs[c], n), hi = min(offs[c + 1], n);
    const unsigned size = hi > lo ? hi - lo : 0u;
    const unsigned filled = cursor[c] - offs[c];
    m = min(filled, size);
    return lo;
}

// Inclusive scan over the 64 lanes of a wave.
__device__ __forceinline__ unsigned wave_scan(unsigned v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(v, d);
        if ((int)lane_id() >= d) v += o;
    }
    return v;
}

// Exclusive scan of one 256-thread block's per-thread values; returns the block total via `total`.
__device__ __forceinline__ unsigned block_exclusive_scan(unsigned v, unsigned* wsum, unsigned& total)
{
    const unsigned inc = wave_scan(v);
    const int w = threadIdx.x / 64;
    if (lane_id() == 63) wsum[w] = inc;
    __syncthreads();
    unsigned base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < SCAN_THREADS / 64; ++k) {
        const unsigned s = wsum[k];
        base += (k < w) ? s : 0u;
        tot += s;
    }
    total = tot;
    return base + inc - v;
}

// scan 1/3: the sum of every tile of SCAN_TILE counts
__global__ __launch_bounds__(SCAN_THREADS)
void dsm_scan_tiles(const unsigned* __restrict__ count, unsigned ncells, unsigned* __restrict__ tile_sum)
{
    __shared__ unsigned wsum[SCAN_THREADS / 64];
    const size_t base = (size_t)blockIdx.x * SCAN_TILE;
    unsigned s = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const size_t c = base + (size_t)k * SCAN_THREADS + threadIdx.x;
        if (c < ncells) s += count[c];
    }
    unsigned total;
    block_exclusive_scan(s, wsum, total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// scan 2/3: exclusive scan of the tile sums (one block, carried across chunks); the grand total closes the offsets.
__global__ __launch_bounds__(SCAN_THREADS)
void dsm_scan_sums(unsigned* __restrict__ tile_sum, unsigned ntiles, unsigned* __restrict__ offs, unsigned ncells,
                   unsigned* __restrict__ list_count)
{
    __shared__ unsigned wsum[SCAN_THREADS / 64];
    unsigned carry = 0;
    for (unsigned b0 = 0; b0 < ntiles; b0 += SCAN_THREADS) {
        const unsigned b = b0 + threadIdx.x;
        const unsigned v = b < ntiles ? tile_sum[b] : 0u;
        unsigned total;
        const unsigned ex = block_exclusive_scan(v, wsum, total);
        if (b < ntiles) tile_sum[b] = carry + ex;
        carry += total;
        __syncthreads();                                     // wsum is reused by the next chunk
    }
    if (threadIdx.x == 0) {
        offs[ncells] = carry;
        list_count[0] = 0;
        list_count[1] = 0;
    }
}

// scan 3/3: offsets of every cell, and the scatter cursors (a copy of them)
__global__ __launch_bounds__(SCAN_THREADS)
void dsm_scan_cells(const unsigned* __restrict__ count, unsigned ncells, const unsigned* __restrict__ tile_sum,
                    unsigned* __restrict__ offs, unsigned* __restrict__ cursor)
{
    __shared__ unsigned tile[SCAN_TILE];
    __shared__ unsigned wsum[SCAN_THREADS / 64];
    const size_t base = (size_t)blockIdx.x * SCAN_TILE;
    for (int k = 0; k < SCAN_ITEMS; ++k) {                    // coalesced load, striped
        const int j = k * SCAN_THREADS + threadIdx.x;
        tile[j] = (base + j < ncells) ? count[base + j] : 0u;
    }
    __syncthreads();
    unsigned v[SCAN_ITEMS], s = 0;                           // each thread: SCAN_ITEMS consecutive cells
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) { v[k] = tile[threadIdx.x * SCAN_ITEMS + k]; s += v[k]; }
    unsigned total;
    unsigned run = tile_sum[blockIdx.x] + block_exclusive_scan(s, wsum, total);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) { tile[threadIdx.x * SCAN_ITEMS + k] = run; run += v[k]; }
    __syncthreads();
    for (int k = 0; k < SCAN_ITEMS; ++k) {                    // coalesced store
        const int j = k * SCAN_THREADS + threadIdx.x;
        if (base + j < ncells) { offs[base + j] = tile[j]; cursor[base + j] = tile[j]; }
    }
}

// Heights -> key slots of their cells' buckets.  Runs of one cell in a wave take their slots with one returning atomic.
__global__ __launch_bounds__(256)
void dsm_scatter(const int* __restrict__ cell, const float* __restrict__ height, unsigned n, unsigned ncells,
                 const unsigned* __restrict__ offs, unsigned* __restrict__ cursor, unsigned* __restrict__ keys)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    int c = -1;
    float h = 0.0f;
    if (i < n) {
        c = cell[i];
        if (c < 0 || (unsigned)c >= ncells) c = -1;
        else h = height[i];
    }
    const unsigned long long heads = run_heads(c);
    const unsigned L = lane_id();
    const unsigned head = run_head(heads);
    unsigned base = 0;
    if (c >= 0 && head == L) base = atomicAdd(&cursor[c], run_length(heads));
    base = __shfl(base, (int)head);
    if (c >= 0) {
        const unsigned slot = base + (L - head);
        if (slot >= offs[c] && slot < offs[c + 1] && slot < n) keys[slot] = f2key(h);
    }
}

// Median / mean / min / max of a sorted bucket whose k-th key is get(k).
template <typename Get>
__device__ __forceinline__ float reduce_sorted(int mode, unsigned m, double sum, Get get)
{
    if (mode == 2) return key2f(get(0));
    if (mode == 3) return key2f(get(m - 1));
    if (mode == 1) return (float)(sum / (double)m);
    if (m & 1u) return key2f(get(m / 2));
    return (float)(0.5 * ((double)key2f(get(m / 2 - 1)) + (double)key2f(get(m / 2))));
}

// tier 0 and classification: one lane per cell.  Empty cells get nodata; buckets of up to TIER0_MAX keys are sorted by a bitonic
// network in registers (static indices only: no scratch); larger ones are listed for the workgroup tiers.
__global__ __launch_bounds__(256)
void dsm_cells_small(const unsigned* __restrict__ offs, const unsigned* __restrict__ cursor, const unsigned* __restrict__ keys,
                     unsigned n, unsigned ncells, int mode, float nodata, float* __restrict__ dsm,
                     unsigned* __restrict__ list_count, int* __restrict__ list1, int* __restrict__ list2)
{
    const size_t ci = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ci >= ncells) return;
    const int c = (int)ci;
    unsigned m;
    const unsigned lo = bucket(offs, cursor, c, n, m);
    if (m == 0) { dsm[c] = nodata; return; }
    if (m > TIER0_MAX) {
        if (m <= TIER1_MAX) list1[atomicAdd(&list_count[0], 1u)] = c;
        else list2[atomicAdd(&list_count[1], 1u)] = c;
        return;
    }
    unsigned v[TIER0_MAX];
#pragma unroll
    for (int k = 0; k < TIER0_MAX; ++k) v[k] = ((unsigned)k < m) ? keys[lo + k] : 0xffffffffu;
    bitonic_net<TIER0_MAX, 2, 1>(v);
    double sum = 0.0;
    if (mode == 1) {
#pragma unroll
        for (int k = 0; k < TIER0_MAX; ++k)
            if ((unsigned)k < m) sum += (double)key2f(v[k]);
    }
    // the two keys a mode may need, picked by selects (an indexed load would send v[] to scratch)
    const unsigned ia = (mode == 2) ? 0u : (mode == 3) ? m - 1 : (m & 1u) ? m / 2 : m / 2 - 1, ib = m / 2;
    unsigned ka = v[0], kb = v[0];
#pragma unroll
    for (int k = 1; k < TIER0_MAX; ++k) {
        ka = ((unsigned)k == ia) ? v[k] : ka;
        kb = ((unsigned)k == ib) ? v[k] : kb;
    }
    dsm[c] = reduce_sorted(mode, m, sum, [=](unsigned k) { return k == ia ? ka : kb; });
}

// Deterministic float64 sum of a block's per-thread partials (fixed tree over the block).
template <int NT>
__device__ __forceinline__ double block_sum(double s, double* red)
{
    red[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int w = NT / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// tier 1: one workgroup per listed cell, bitonic sort of the padded bucket in LDS
__global__ __launch_bounds__(TIER1_THREADS)
void dsm_cells_bitonic(const unsigned* __restrict__ offs, const unsigned* __restrict__ cursor, const unsigned* __restrict__ keys,
                       unsigned n, int mode, float* __restrict__ dsm, const unsigned* __restrict__ list_count,
                       const int* __restrict__ list1)
{
    __shared__ unsigned s[TIER1_MAX];
    __shared__ double red[TIER1_THREADS];
    const unsigned nlist = list_count[0];
    for (unsigned li = blockIdx.x; li < nlist; li += gridDim.x) {
        const int c = list1[li];
        unsigned m;
        const unsigned lo = bucket(offs, cursor, c, n, m);
        unsigned P = 1;
        while (P < m) P <<= 1;
        for (unsigned k = threadIdx.x; k < P; k += TIER1_THREADS) s[k] = k < m ? keys[lo + k] : 0xffffffffu;
        __syncthreads();
        for (unsigned size = 2; size <= P; size <<= 1)
            for (unsigned stride = size / 2; stride > 0; stride >>= 1) {
                for (unsigned t = threadIdx.x; t < P / 2; t += TIER1_THREADS) {
                    const unsigned k = 2 * t - (t & (stride - 1)), p = k + stride;
                    const unsigned a = s[k], b = s[p];
                    const bool up = (k & size) == 0;
                    if (up ? (a > b) : (a < b)) { s[k] = b; s[p] = a; }
                }
                __syncthreads();
            }
        double part = 0.0;
        if (mode == 1)
            for (unsigned k = threadIdx.x; k < m; k += TIER1_THREADS) part += (double)key2f(s[k]);
        const double sum = (mode == 1) ? block_sum<TIER1_THREADS>(part, red) : 0.0;
        if (threadIdx.x == 0) dsm[c] = reduce_sorted(mode, m, sum, [&](unsigned k) { return s[k]; });
        __syncthreads();                                     // s[] is reused by the next cell
    }
}

// tier 2: one workgroup per listed cell, stable LSD radix sort (4 passes of 8 bits) between the bucket and its twin in `alt`;
// after an even number of passes the sorted keys are back in the bucket.  Within a tile of TIER2_THREADS keys the rank of a key
// among equal digits is its wave-local rank (ballots on the 8 digit bits) plus the counts of the same digit in earlier waves.
__global__ __launch_bounds__(TIER2_THREADS)
void dsm_cells_radix(const unsigned* __restrict__ offs, const unsigned* __restrict__ cursor, unsigned* __restrict__ keys,
                     unsigned* __restrict__ alt, unsigned n, int mode, float* __restrict__ dsm,
                     const unsigned* __restrict__ list_count, const int* __restrict__ list2)
{
    __shared__ unsigned hist[256];
    __shared__ unsigned wcnt[TIER2_WAVES][256];
    __shared__ double red[TIER2_THREADS];
    const unsigned nlist = list_count[1];
    const unsigned L = lane_id(), w = threadIdx.x / 64;
    const unsigned long long lt = (1ull << L) - 1ull;
    for (unsigned li = blockIdx.x; li < nlist; li += gridDim.x) {
        const int c = list2[li];
        unsigned m;
        const unsigned lo = bucket(offs, cursor, c, n, m);
        unsigned* src = keys + lo;
        unsigned* dst = alt + lo;
        for (int shift = 0; shift < 32; shift += 8) {
            for (unsigned d = threadIdx.x; d < 256; d += TIER2_THREADS) hist[d] = 0;
            __syncthreads();
            for (unsigned k = threadIdx.x; k < m; k += TIER2_THREADS) atomicAdd(&hist[(src[k] >> shift) & 255u], 1u);
            __syncthreads();
            if (threadIdx.x < 64) {                              // exclusive scan of the 256 digit counts, 4 per lane
                unsigned h[4], s = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) { h[q] = hist[4 * L + q]; s += h[q]; }
                unsigned run = wave_scan(s) - s;
#pragma unroll
                for (int q = 0; q < 4; ++q) { hist[4 * L + q] = run; run += h[q]; }
            }
            __syncthreads();
            for (unsigned t0 = 0; t0 < m; t0 += TIER2_THREADS) {
                for (unsigned j = threadIdx.x; j < TIER2_WAVES * 256; j += TIER2_THREADS) (&wcnt[0][0])[j] = 0;
                __syncthreads();
                const unsigned k = t0 + threadIdx.x;
                const bool valid = k < m;
                const unsigned key = valid ? src[k] : 0u;
                const unsigned d = (key >> shift) & 255u;
                unsigned long long peers = __ballot(valid);
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const unsigned long long bits = __ballot((d >> b) & 1u);
                    peers &= ((d >> b) & 1u) ? bits : ~bits;
                }
                const unsigned rank = (unsigned)__popcll(peers & lt);
                if (valid && rank == 0) wcnt[w][d] = (unsigned)__popcll(peers);
                __syncthreads();
                if (threadIdx.x < 256) {                         // per digit: running base over the waves of the tile
                    const unsigned dd = threadIdx.x;
                    unsigned run = hist[dd];
                    for (int q = 0; q < TIER2_WAVES; ++q) { const unsigned x = wcnt[q][dd]; wcnt[q][dd] = run; run += x; }
                    hist[dd] = run;
                }
                __syncthreads();
                if (valid) {
                    const unsigned pos = wcnt[w][d] + rank;
                    if (pos < m) dst[pos] = key;
                }
                __syncthreads();
            }
            unsigned* tmp = src; src = dst; dst = tmp;
        }
        double part = 0.0;
        if (mode == 1)
            for (unsigned k = threadIdx.x; k < m; k += TIER2_THREADS) part += (double)key2f(src[k]);
        const double sum = (mode == 1) ? block_sum<TIER2_THREADS>(part, red) : 0.0;
        if (threadIdx.x == 0) dsm[c] = reduce_sorted(mode, m, sum, [&](unsigned k) { return src[k]; });
        __syncthreads();
    }
}

// ---- workspace layout --------------------------------------------------------------------------------------------------------
struct DsmWs { size_t offs, cursor, keys, alt, tiles, lcount, list1, list2, bytes; };

static DsmWs dsm_ws(size_t n, size_t ncells)
{
    DsmWs w;
    const size_t ntiles = (ncells + SCAN_TILE - 1) / SCAN_TILE;
    const size_t l1 = std::min(ncells, n / (TIER0_MAX + 1) + 1), l2 = std::min(ncells, n / (TIER1_MAX + 1) + 1);
    size_t o = 0;
    w.offs = o;   o += align256((ncells + 1) * 4);
    w.cursor = o; o += align256(ncells * 4);
    w.keys = o;   o += align256(std::max<size_t>(n, 1) * 4);
    w.alt = o;    o += align256(std::max<size_t>(n, 1) * 4);
    w.tiles = o;  o += align256(ntiles * 4);
    w.lcount = o; o += 256;
    w.list1 = o;  o += align256(l1 * 4);
    w.list2 = o;  o += align256(l2 * 4);
    w.bytes = o;
    return w;
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT int smvs_tm_project(const double* tm7, const double* a, const double* b, double* o0, double* o1, size_t n, int dir,
                                void* stream)
{
    using namespace smvs;
    if (!tm7 || !a || !b || !o0 || !o1) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (dir != 0 && dir != 1) return fail(SMVS_ERR_ARG, "dir must be 0 (lat/lon -> E/N) or 1 (E/N -> lat/lon)");
    TmConst t;
    if (const char* msg = tm_parse(tm7, t)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (n == 0) return SMVS_OK;
    hipLaunchKernelGGL(tm_project_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, t, a, b, o0, o1, n, dir);
    return check_launch("tm_project");
}

SMVS_EXPORT int smvs_rpc_dsm_bin(const float* height, const unsigned char* mask, const double* rpc170, int H, int W,
                                 const double* tm7, const double* grid4, int gw, int gh,
                                 int* cell, unsigned* count, double* east, double* north, void* stream)
{
    using namespace smvs;
    if (!height || !rpc170 || !tm7 || !grid4 || !cell || !count) return fail(SMVS_ERR_ARG, "null pointer argument");
    if ((east == nullptr) != (north == nullptr)) return fail(SMVS_ERR_ARG, "east and north go together");
    if (H < 1 || W < 1) return fail(SMVS_ERR_ARG, "non-positive dimension");
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s", msg);
    DsmGrid g;
    if (const char* msg = dsm_grid_parse(grid4, g)) return fail(SMVS_ERR_ARG, "%s", msg);
    TmConst t;
    if (const char* msg = tm_parse(tm7, t)) return fail(SMVS_ERR_ARG, "%s", msg);
    const size_t n = (size_t)H * W;
    hipLaunchKernelGGL(dsm_bin_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       height, mask, rpc170, H, W, t, g, gw, gh, cell, count, east, north);
    return check_launch("dsm_bin");
}

SMVS_EXPORT size_t smvs_dsm_workspace_bytes(size_t n, int gw, int gh)
{
    using namespace smvs;
    if (n >= (1ull << 31) || grid_check(gw, gh)) return 0;
    return dsm_ws(n, (size_t)gw * gh).bytes;
}

SMVS_EXPORT int smvs_dsm_reduce(const int* cell, const float* height, size_t n, const unsigned* count, int gw, int gh,
                                int mode, float nodata, float* dsm, void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!cell || !height || !count || !dsm || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (mode < 0 || mode > 3) return fail(SMVS_ERR_ARG, "mode must be 0 (median), 1 (mean), 2 (min) or 3 (max)");
    if (n >= (1ull << 31)) return fail(SMVS_ERR_ARG, "too many points: n must be below 2^31 per reduce");
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s", msg);
    const size_t ncells = (size_t)gw * gh;
    const DsmWs w = dsm_ws(n, ncells);
    if (workspace_bytes < w.bytes) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, w.bytes);
    char* ws = (char*)workspace;
    unsigned* offs = (unsigned*)(ws + w.offs);
    unsigned* cursor = (unsigned*)(ws + w.cursor);
    unsigned* keys = (unsigned*)(ws + w.keys);
    unsigned* alt = (unsigned*)(ws + w.alt);
    unsigned* tiles = (unsigned*)(ws + w.tiles);
    unsigned* lcount = (unsigned*)(ws + w.lcount);
    int* list1 = (int*)(ws + w.list1);
    int* list2 = (int*)(ws + w.list2);
    hipStream_t s = (hipStream_t)stream;
    const unsigned nc = (unsigned)ncells, nn = (unsigned)n;
    const unsigned ntiles = (unsigned)((ncells + SCAN_TILE - 1) / SCAN_TILE);
    int rc;
    hipLaunchKernelGGL(dsm_scan_tiles, dim3(ntiles), dim3(SCAN_THREADS), 0, s, count, nc, tiles);
    if ((rc = check_launch("dsm_scan_tiles"))) return rc;
    hipLaunchKernelGGL(dsm_scan_sums, dim3(1), dim3(SCAN_THREADS), 0, s, tiles, ntiles, offs, nc, lcount);
    if ((rc = check_launch("dsm_scan_sums"))) return rc;
    hipLaunchKernelGGL(dsm_scan_cells, dim3(ntiles), dim3(SCAN_THREADS), 0, s, count, nc, tiles, offs, cursor);
    if ((rc = check_launch("dsm_scan_cells"))) return rc;
    if (n > 0) {
        hipLaunchKernelGGL(dsm_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, cell, height, nn, nc, offs, cursor, keys);
        if ((rc = check_launch("dsm_scatter"))) return rc;
    }
    hipLaunchKernelGGL(dsm_cells_small, dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, s,
                       offs, cursor, keys, nn, nc, mode, nodata, dsm, lcount, list1, list2);
    if ((rc = check_launch("dsm_cells_small"))) return rc;
    if (n > (size_t)TIER0_MAX) {
        hipLaunchKernelGGL(dsm_cells_bitonic, dim3(TIER1_BLOCKS), dim3(TIER1_THREADS), 0, s, offs, cursor, keys, nn, mode, dsm, lcount, list1);
        if ((rc = check_launch("dsm_cells_bitonic"))) return rc;
    }
    if (n > (size_t)TIER1_MAX) {
        hipLaunchKernelGGL(dsm_cells_radix, dim3(TIER2_BLOCKS), dim3(TIER2_THREADS), 0, s, offs, cursor, keys, alt, nn, mode, dsm, lcount, list2);
        if ((rc = check_launch("dsm_cells_radix"))) return rc;
    }
    return SMVS_OK;
}

}  // extern "C"
