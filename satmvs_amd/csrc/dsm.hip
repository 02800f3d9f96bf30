// dsm.hip -- DSM production: per-view height maps (image space, RPC) -> one height grid in map coordinates.
//
//   smvs_tm_project   Transverse Mercator (USGS series, Snyder, "Map Projections -- A Working Manual", pp. 60-64), float64,
//                     both directions; pinned by tests/golden/tm.npz (the reference's tools/Transverse_Mercator.py).
//   smvs_rpc_dsm_bin  one lane per pixel: (x, y, h) -> (lat, lon) through the inverse RPC the filter uses (rpc_photo2obj),
//                     -> (E, N) through the TM forward, -> grid cell; counts per cell accumulated with atomics.
//   smvs_dsm_reduce   exclusive scan of the counts, scatter of the heights into per-cell buckets, sort of every bucket on the
//                     order-preserving uint32 image of the float, then median / mean / min / max of the sorted bucket.
//   smvs_rpc_dsm_render  the reverse direction: one lane per pixel of a view marches its ray (x, y, h) down through the
//                     bilinear surface of a DSM, then bisects the crossing; the first crossing from above is the pixel's height.
//   smvs_rpc_ortho    the orthophoto: one lane per DSM cell projects the cell's point into a view, marches the ray up to test
//                     occlusion, and samples the image bilinearly; a mosaic fills each cell from the first view that sees it.
//
// Determinism: the only order-dependent steps are the atomics (which slot of its bucket a height lands in, which position a cell
// takes in a tier list).  Every bucket is sorted before it is reduced, equal keys are equal bits, and the reduction order of a
// bucket depends on its size alone, so the DSM is bit-identical from run to run and under any permutation of points or maps.
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "dsm_common.h"
#include "smvs_device.h"
#include "smvs_host.h"

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
struct DsmGrid { double e0, n0, xres, yres; };

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

// ---- render pass: DSM -> one view's image-space heights (include/satmvs.h) -----------------------------
constexpr int RENDER_TILE = 16;                      // 16 x 16 pixels per workgroup: each wave covers 16 columns x 4 rows
constexpr int RENDER_MAX_STEPS = 4096, RENDER_MAX_BISECT = 60;
constexpr unsigned RENDER_MAX_BLOCKS = 1u << 20;     // grid-stride over tiles beyond this

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

// One lane per pixel.  The march (h_k = h_hi - k (h_hi - h_lo) / K, h_K = h_lo; first k with f(h_k) = S(G(h_k)) - h_k defined and >= 0)
// and the bisection of [h_k, h_{k-1}] run as ONE loop whose body is one evaluation photo2obj -> TM -> bilinear; the lane's
// state picks the next height, so lanes in different phases share the body instead of running it twice under divergence.
__global__ __launch_bounds__(RENDER_TILE * RENDER_TILE)
void dsm_render_kernel(const float* __restrict__ z, int gw, int gh, DsmGrid g, float nodata, TmConst t,
                       const double* __restrict__ rpc, int H, int W, int x0, int y0, double h_lo, double h_hi, double tol,
                       float* __restrict__ out)
{
    const unsigned nbx = (unsigned)(W + RENDER_TILE - 1) / RENDER_TILE, nby = (unsigned)(H + RENDER_TILE - 1) / RENDER_TILE;
    const unsigned ntiles = nbx * nby;
    const cgeo_t r = as_cgeo(rpc);
    const RpcInv rn = rpc_inv_image(r);
    for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int j = (int)(tile % nbx) * RENDER_TILE + (int)(threadIdx.x % RENDER_TILE);
        const int i = (int)(tile / nbx) * RENDER_TILE + (int)(threadIdx.x / RENDER_TILE);
        if (i >= H || j >= W) continue;
        const double x = (double)(x0 + j), y = (double)(y0 + i);
        double lat, lon, E_lo, N_lo;
        rpc_photo2obj(launder(r), rn, x, y, h_lo, lat, lon);
        tm_forward(t, lat, lon, E_lo, N_lo);
        double h = h_hi, h_prev = h_hi, a = 0.0, b = 0.0, step = 0.0;
        int k = 0, K = 1, left = -1;                 // left < 0: marching; else bisection steps still to take
        bool prev_ok = false;
        float res = __builtin_nanf("");
        for (;;) {
            double E, N, S;
            rpc_photo2obj(launder(r), rn, x, y, h, lat, lon);
            tm_forward(t, lat, lon, E, N);
            const bool ok = dsm_surface(z, gw, gh, nodata, g, E, N, S);
            const bool below = ok && S - h >= 0.0;   // f(h) defined and >= 0
            if (left < 0) {
                if (k == 0) {
                    K = render_march_steps(g, E, N, E_lo, N_lo);
                    step = (h_hi - h_lo) / (double)K;
                }
                if (!below) {
                    if (k == K) break;               // no sample qualifies: invalid
                    prev_ok = ok;
                    h_prev = h;
                    ++k;
                    h = (k == K) ? h_lo : h_hi - (double)k * step;     // the last sample is h_lo exactly, whatever the rounding
                    continue;
                }
                if (k == 0) { res = (float)h_hi; break; }
                if (!prev_ok) break;                 // came out of a hole or off the grid: invalid
                a = h;
                b = h_prev;
                left = render_bisect_steps(step, tol);
            } else {
                if (!ok) break;                      // a midpoint where f is undefined: invalid
                if (below) a = h;
                else b = h;
                --left;
            }
            if (left == 0) { res = (float)(0.5 * (a + b)); break; }
            h = 0.5 * (a + b);
        }
        out[(size_t)i * W + j] = res;
    }
}

// ---- orthophoto pass: one view's image resampled onto the DSM grid, with occlusion (include/satmvs.h) --
constexpr int ORTHO_MAX_CHANNELS = 16;
enum : unsigned char { ORTHO_NO_HEIGHT = 0, ORTHO_OUTSIDE = 1, ORTHO_OCCLUDED = 2, ORTHO_VISIBLE = 3 };

// Whether the ray up from the cell's point (x, y, zc) passes under the surface: samples h_k = zc + k (h_hi - zc) / K,
// k = 1 .. K - 1, and h_K = h_hi exactly, K from the travel between G(zc) and G(h_hi) as in the render.  A sample occludes where
// f(h_k) = S(G(h_k)) - h_k is defined and > occ_tol; undefined samples (holes, off the grid) do not.  ONE loop whose body is one
// evaluation photo2obj -> TM -> bilinear, as in the render: G(zc) first (only for K), then h_K = h_hi (its G sets K; the order
// of the samples does not change whether one of them occludes), then h_1 .. h_{K-1}.
__device__ __forceinline__ bool ortho_occluded(const float* __restrict__ z, int gw, int gh, float nodata, const DsmGrid& g,
                                               const TmConst& t, cgeo_t r, const RpcInv& rn, double x, double y, double zc,
                                               double h_hi, double occ_tol)
{
    if (!(zc < h_hi)) return false;
    double h = zc, E_z = 0.0, N_z = 0.0, step = 0.0;
    int k = -1, K = 1;                               // k = -1: G(zc); k = 0: h_K; then k = 1 .. K - 1, K <= RENDER_MAX_STEPS
    for (;;) {
        double lat, lon, E, N, S;
        rpc_photo2obj(launder(r), rn, x, y, h, lat, lon);
        tm_forward(t, lat, lon, E, N);
        if (k < 0) {
            E_z = E;
            N_z = N;
            k = 0;
            h = h_hi;
            continue;
        }
        if (dsm_surface(z, gw, gh, nodata, g, E, N, S) && S - h > occ_tol) return true;
        if (k == 0) {
            K = render_march_steps(g, E, N, E_z, N_z);
            step = (h_hi - zc) / (double)K;
        }
        if (++k >= K) return false;
        h = zc + (double)k * step;
    }
}

// One lane per DSM cell, 16 x 16-cell workgroups (neighbouring rays read the same DSM lines), grid-stride past
// RENDER_MAX_BLOCKS.  Height -> TM inverse -> rpc_obj2photo -> bounds -> occlusion march -> bilinear image sample; ortho and
// source are written where the cell is visible and source < 0 on entry.  Without a state map, cells already filled by an
// earlier view are skipped whole.
__global__ __launch_bounds__(RENDER_TILE * RENDER_TILE)
void dsm_ortho_kernel(const float* __restrict__ z, int gw, int gh, DsmGrid g, float nodata, TmConst t,
                      const double* __restrict__ rpc, const float* __restrict__ image, int H, int W, int C, int x0, int y0,
                      double h_hi, int occlusion, double occ_tol, int view,
                      float* __restrict__ ortho, int* __restrict__ source, unsigned char* __restrict__ state)
{
    const unsigned nbx = (unsigned)(gw + RENDER_TILE - 1) / RENDER_TILE, nby = (unsigned)(gh + RENDER_TILE - 1) / RENDER_TILE;
    const unsigned ntiles = nbx * nby;
    const cgeo_t r = as_cgeo(rpc);
    const RpcInv rg = rpc_inv_ground(r), ri = rpc_inv_image(r);
    for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int c = (int)(tile % nbx) * RENDER_TILE + (int)(threadIdx.x % RENDER_TILE);
        const int row = (int)(tile / nbx) * RENDER_TILE + (int)(threadIdx.x / RENDER_TILE);
        if (row >= gh || c >= gw) continue;
        const size_t cell = (size_t)row * gw + c;
        if (!state && source[cell] >= 0) continue;   // filled by an earlier view; nothing else to write
        const float zf = z[cell];
        unsigned char st = ORTHO_NO_HEIGHT;
        double u = 0.0, v = 0.0;
        if (dsm_cell_valid(zf, nodata)) {
            const double E = g.e0 + (double)c * g.xres, N = g.n0 - (double)row * g.yres;
            double lat, lon, x, y;
            tm_inverse(t, E, N, lat, lon);
            rpc_obj2photo(launder(r), rg, lat, lon, (double)zf, x, y);
            u = x - (double)x0;
            v = y - (double)y0;
            if (!(u >= 0.0 && u <= (double)(W - 1) && v >= 0.0 && v <= (double)(H - 1))) st = ORTHO_OUTSIDE;   // NaN fails
            else if (occlusion && ortho_occluded(z, gw, gh, nodata, g, t, r, ri, x, y, (double)zf, h_hi, occ_tol)) st = ORTHO_OCCLUDED;
            else st = ORTHO_VISIBLE;
        }
        if (state) state[cell] = st;
        if (st != ORTHO_VISIBLE || !source || source[cell] >= 0) continue;
        if (ortho) {
            // pixel centres on integers; the last column / row is reached with du = 1 (dv = 1) from the one before it
            const int c0 = W > 1 ? min((int)floor(u), W - 2) : 0, r0 = H > 1 ? min((int)floor(v), H - 2) : 0;
            const int c1 = W > 1 ? c0 + 1 : 0, r1 = H > 1 ? r0 + 1 : 0;
            const double du = W > 1 ? u - (double)c0 : 0.0, dv = H > 1 ? v - (double)r0 : 0.0;
            const float* p00 = image + ((size_t)r0 * W + c0) * C;
            const float* p01 = image + ((size_t)r0 * W + c1) * C;
            const float* p10 = image + ((size_t)r1 * W + c0) * C;
            const float* p11 = image + ((size_t)r1 * W + c1) * C;
            float* o = ortho + cell * C;
            for (int ch = 0; ch < ORTHO_MAX_CHANNELS && ch < C; ++ch) {
                const double a = (double)p00[ch] + du * ((double)p01[ch] - (double)p00[ch]);
                const double b = (double)p10[ch] + du * ((double)p11[ch] - (double)p10[ch]);
                o[ch] = (float)(a + dv * (b - a));
            }
        }
        source[cell] = view;
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
    if (!tm_setup(tm7, t)) return fail(SMVS_ERR_ARG, "bad projection parameters (a > 0, inverse flattening > 1, k0 > 0, all finite)");
    if (n == 0) return SMVS_OK;
    hipLaunchKernelGGL(tm_project_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, t, a, b, o0, o1, n, dir);
    return check_launch_dsm("tm_project");
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
    const DsmGrid g{grid4[0], grid4[1], grid4[2], grid4[3]};
    if (!isfinite(g.e0) || !isfinite(g.n0) || !(g.xres > 0.0) || !(g.yres > 0.0) || !isfinite(g.xres) || !isfinite(g.yres))
        return fail(SMVS_ERR_ARG, "bad grid: E0, N0 finite, xres and yres positive and finite");
    TmConst t;
    if (!tm_setup(tm7, t)) return fail(SMVS_ERR_ARG, "bad projection parameters (a > 0, inverse flattening > 1, k0 > 0, all finite)");
    const size_t n = (size_t)H * W;
    hipLaunchKernelGGL(dsm_bin_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       height, mask, rpc170, H, W, t, g, gw, gh, cell, count, east, north);
    return check_launch_dsm("dsm_bin");
}

SMVS_EXPORT int smvs_rpc_dsm_render(const float* dsm, int gw, int gh, const double* grid4, float nodata, const double* tm7,
                                    const double* rpc170, int H, int W, int x0, int y0, double h_lo, double h_hi, double tol,
                                    float* height, void* stream)
{
    using namespace smvs;
    if (!dsm || !grid4 || !tm7 || !rpc170 || !height) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (H < 1 || W < 1) return fail(SMVS_ERR_ARG, "non-positive dimension");
    if ((long long)H * W >= (1ll << 31)) return fail(SMVS_ERR_ARG, "view too large: H * W must be below 2^31 pixels");
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (x0 < 0 || y0 < 0) return fail(SMVS_ERR_ARG, "negative origin");
    if ((long long)x0 + W > INT_MAX || (long long)y0 + H > INT_MAX) return fail(SMVS_ERR_ARG, "origin + size does not fit in an int");
    const DsmGrid g{grid4[0], grid4[1], grid4[2], grid4[3]};
    if (!isfinite(g.e0) || !isfinite(g.n0) || !(g.xres > 0.0) || !(g.yres > 0.0) || !isfinite(g.xres) || !isfinite(g.yres))
        return fail(SMVS_ERR_ARG, "bad grid: E0, N0 finite, xres and yres positive and finite");
    TmConst t;
    if (!tm_setup(tm7, t)) return fail(SMVS_ERR_ARG, "bad projection parameters (a > 0, inverse flattening > 1, k0 > 0, all finite)");
    if (!isfinite(h_lo) || !isfinite(h_hi) || !(h_lo <= h_hi)) return fail(SMVS_ERR_ARG, "height bracket: h_lo <= h_hi, both finite");
    if (!(tol > 0.0) || !isfinite(tol)) return fail(SMVS_ERR_ARG, "tol must be positive and finite");
    const unsigned ntiles = (unsigned)((W + RENDER_TILE - 1) / RENDER_TILE) * (unsigned)((H + RENDER_TILE - 1) / RENDER_TILE);
    hipLaunchKernelGGL(dsm_render_kernel, dim3(std::min(ntiles, RENDER_MAX_BLOCKS)), dim3(RENDER_TILE * RENDER_TILE), 0,
                       (hipStream_t)stream, dsm, gw, gh, g, nodata, t, rpc170, H, W, x0, y0, h_lo, h_hi, tol, height);
    return check_launch_dsm("dsm_render");
}

SMVS_EXPORT int smvs_rpc_ortho(const float* dsm, int gw, int gh, const double* grid4, float nodata, const double* tm7,
                               const double* rpc170, const float* image, int H, int W, int C, int x0, int y0,
                               double h_hi, int occlusion, double occ_tol, int view,
                               float* ortho, int* source, unsigned char* state, void* stream)
{
    using namespace smvs;
    if (!dsm || !grid4 || !tm7 || !rpc170) return fail(SMVS_ERR_ARG, "null pointer argument");
    if ((image == nullptr) != (ortho == nullptr)) return fail(SMVS_ERR_ARG, "null pointer argument: image and ortho go together");
    if (ortho && !source) return fail(SMVS_ERR_ARG, "null pointer argument: ortho needs source (the mosaic rule reads it)");
    if (!source && !state) return fail(SMVS_ERR_ARG, "null pointer argument: nothing to write (give source or state)");
    if (C < 1 || C > ORTHO_MAX_CHANNELS) return fail(SMVS_ERR_ARG, "channel count C must be in 1 .. %d", ORTHO_MAX_CHANNELS);
    if (H < 1 || W < 1) return fail(SMVS_ERR_ARG, "non-positive dimension");
    if ((long long)H * W >= (1ll << 31)) return fail(SMVS_ERR_ARG, "view too large: H * W must be below 2^31 pixels");
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (x0 < 0 || y0 < 0) return fail(SMVS_ERR_ARG, "negative origin");
    if ((long long)x0 + W > INT_MAX || (long long)y0 + H > INT_MAX) return fail(SMVS_ERR_ARG, "origin + size does not fit in an int");
    const DsmGrid g{grid4[0], grid4[1], grid4[2], grid4[3]};
    if (!isfinite(g.e0) || !isfinite(g.n0) || !(g.xres > 0.0) || !(g.yres > 0.0) || !isfinite(g.xres) || !isfinite(g.yres))
        return fail(SMVS_ERR_ARG, "bad grid: E0, N0 finite, xres and yres positive and finite");
    TmConst t;
    if (!tm_setup(tm7, t)) return fail(SMVS_ERR_ARG, "bad projection parameters (a > 0, inverse flattening > 1, k0 > 0, all finite)");
    if (!isfinite(h_hi)) return fail(SMVS_ERR_ARG, "h_hi must be finite");
    if (!(occ_tol >= 0.0) || !isfinite(occ_tol)) return fail(SMVS_ERR_ARG, "occ_tol must be finite and >= 0");
    if (view < 0) return fail(SMVS_ERR_ARG, "view must be non-negative");
    const unsigned ntiles = (unsigned)((gw + RENDER_TILE - 1) / RENDER_TILE) * (unsigned)((gh + RENDER_TILE - 1) / RENDER_TILE);
    hipLaunchKernelGGL(dsm_ortho_kernel, dim3(std::min(ntiles, RENDER_MAX_BLOCKS)), dim3(RENDER_TILE * RENDER_TILE), 0,
                       (hipStream_t)stream, dsm, gw, gh, g, nodata, t, rpc170, image, H, W, C, x0, y0, h_hi, occlusion, occ_tol,
                       view, ortho, source, state);
    return check_launch_dsm("dsm_ortho");
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
    if ((rc = check_launch_dsm("dsm_scan_tiles"))) return rc;
    hipLaunchKernelGGL(dsm_scan_sums, dim3(1), dim3(SCAN_THREADS), 0, s, tiles, ntiles, offs, nc, lcount);
    if ((rc = check_launch_dsm("dsm_scan_sums"))) return rc;
    hipLaunchKernelGGL(dsm_scan_cells, dim3(ntiles), dim3(SCAN_THREADS), 0, s, count, nc, tiles, offs, cursor);
    if ((rc = check_launch_dsm("dsm_scan_cells"))) return rc;
    if (n > 0) {
        hipLaunchKernelGGL(dsm_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, cell, height, nn, nc, offs, cursor, keys);
        if ((rc = check_launch_dsm("dsm_scatter"))) return rc;
    }
    hipLaunchKernelGGL(dsm_cells_small, dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, s,
                       offs, cursor, keys, nn, nc, mode, nodata, dsm, lcount, list1, list2);
    if ((rc = check_launch_dsm("dsm_cells_small"))) return rc;
    if (n > (size_t)TIER0_MAX) {
        hipLaunchKernelGGL(dsm_cells_bitonic, dim3(TIER1_BLOCKS), dim3(TIER1_THREADS), 0, s, offs, cursor, keys, nn, mode, dsm, lcount, list1);
        if ((rc = check_launch_dsm("dsm_cells_bitonic"))) return rc;
    }
    if (n > (size_t)TIER1_MAX) {
        hipLaunchKernelGGL(dsm_cells_radix, dim3(TIER2_BLOCKS), dim3(TIER2_THREADS), 0, s, offs, cursor, keys, alt, nn, mode, dsm, lcount, list2);
        if ((rc = check_launch_dsm("dsm_cells_radix"))) return rc;
    }
    return SMVS_OK;
}

}  // extern "C"
