// dsm_focal.hip -- focal (moving-window) statistics of a DSM from exact summed-area tables ("Focal
// statistics"; include/satmvs.h for the rule).
//
//   smvs_dsm_focal_build   one buffer per DSM: a header (range, count, centre) and the prefix tables N, S1, S2
//   smvs_dsm_focal_query   any window that is a signed sum of rectangles, at any stride: n, S1, S2, mean, variance per cell
//
// The build is seven launches, memory-bound, all integer:
//   dsm_focal_init / dsm_focal_range / dsm_focal_header   qmin, qmax and the count of the valid cells: a grid-stride walk, a wave reduction by
//                     shuffles and LDS, one integer min / max / add atomic per workgroup (the only atomics of this file); one lane then
//                     writes the centre c = (qmin + qmax) >> 1 and D = max(c - qmin, qmax - c)
//   dsm_focal_band_totals the column pass is cut into bands of FOCAL_BAND rows: a lane per (band, column) sums its band's 1, d, d^2
//                     from the floats themselves (4 bytes a cell; the tables are not touched yet)
//   dsm_focal_band_scan   a lane per column turns the band totals into the carry of every band (an exclusive scan down the bands)
//   dsm_focal_columns     a lane per (band, column) walks its rows from the band's exact carry and writes the column prefixes into
//                     the tables, lanes side by side on columns side by side
//   dsm_focal_rows        a workgroup per table row scans it in place in segments of FOCAL_SEG entries, four consecutive entries a
//                     lane, a wave scan by shuffles, the waves through LDS, the segment's total carried in registers
// Column pass before row pass: the band totals then come from 4-byte cells, not from 20-byte table entries.  Sums are integers
// (S2 modulo 2^64), so neither the order nor the launch geometry can change a bit.
//
// The query is one lane per output cell looping over the rectangle list (wave-uniform reads of packed records); each rectangle
// is clipped to the grid by clamping its corners, so an empty intersection reads four equal entries and adds nothing; the four
// corner reads per table are coalesced across the lanes of a row of output cells.
#include <stdint.h>

#include "dsm_common.h"
#include "smvs_host.h"

namespace smvs {

typedef long long i64;
typedef unsigned long long u64;
typedef unsigned __int128 u128;

constexpr int FOCAL_THREADS = 256, FOCAL_WAVES = FOCAL_THREADS / 64;
constexpr int FOCAL_BAND = 16;                               // rows of one band of the column pass
constexpr int FOCAL_SEG = FOCAL_THREADS * 4;                 // table entries of one step of the row pass
constexpr int FOCAL_HEADER_BYTES = 256, FOCAL_HEADER_WORDS = 8;
constexpr int FOCAL_MAX_RECTS = 1024, FOCAL_MAX_OFFSET = 4096, FOCAL_CHUNK = 128;
constexpr i64 FOCAL_MAX_AREA = 1ll << 24;
constexpr unsigned FOCAL_RANGE_BLOCKS = 256;                 // workgroups of the range pass: as many sets of atomics
constexpr int FOCAL_SCAN_BATCH = 16;                         // bands whose totals a lane of the band scan loads at once

enum { FH_QMIN = 0, FH_QMAX = 1, FH_NVALID = 2, FH_CENTRE = 3, FH_MAXABS = 4 };

struct FocalLayout { size_t n, s1, s2, tn, t1, t2, rects, bytes; };

// header | N int32 | S1 int64 | S2 uint64 over (gh + 1) (gw + 1) entries | the band totals | the rectangle list of the last query
static FocalLayout focal_layout(int gw, int gh)
{
    const size_t e = (size_t)(gw + 1) * (size_t)(gh + 1);
    const size_t t = (size_t)((gh + FOCAL_BAND - 1) / FOCAL_BAND) * (size_t)gw;
    FocalLayout l;
    l.n = FOCAL_HEADER_BYTES;
    l.s1 = l.n + align256(e * 4);
    l.s2 = l.s1 + align256(e * 8);
    l.tn = l.s2 + align256(e * 8);
    l.t1 = l.tn + align256(t * 4);
    l.t2 = l.t1 + align256(t * 8);
    l.rects = l.t2 + align256(t * 8);
    l.bytes = l.rects + (size_t)FOCAL_MAX_RECTS * 8;
    return l;
}

static const char* focal_grid_check(int gw, int gh)
{
    if (gw < 1 || gh < 1) return "non-positive grid size";
    if ((long long)(gw + 1ll) * (gh + 1ll) >= (1ll << 31)) return "grid too large: (gw + 1) * (gh + 1) must be below 2^31";
    return nullptr;
}

// d = q - c of a valid cell; false: the cell adds nothing.
__device__ __forceinline__ bool focal_cell(float z, float nodata, i64 c, i64& d)
{
    int q;
    if (!dsm_quantum(z, nodata, q)) return false;
    d = (i64)q - c;
    return true;
}

__device__ __forceinline__ int focal_up(int v, int by) { return __shfl_up(v, by); }
__device__ __forceinline__ u64 focal_up(u64 v, int by)
{
    const int lo = __shfl_up((int)(unsigned)v, by), hi = __shfl_up((int)(unsigned)(v >> 32), by);
    return ((u64)(unsigned)hi << 32) | (u64)(unsigned)lo;
}

// ---- the range -------------------------------------------------------------------------------------------------------------------
__global__ void dsm_focal_init(i64* __restrict__ hdr)
{
    if (threadIdx.x >= FOCAL_HEADER_WORDS) return;
    hdr[threadIdx.x] = threadIdx.x == FH_QMIN ? INT64_MAX : threadIdx.x == FH_QMAX ? INT64_MIN : 0;
}

// One set of atomics per workgroup: all of them meet on three words, so their number, not the walk, is what this pass costs.
__global__ __launch_bounds__(FOCAL_THREADS)
void dsm_focal_range(const float* __restrict__ dsm, unsigned ncells, float nodata, i64* __restrict__ hdr)
{
    __shared__ int w_lo[FOCAL_WAVES], w_hi[FOCAL_WAVES], w_cnt[FOCAL_WAVES];
    int lo = INT32_MAX, hi = INT32_MIN, cnt = 0;
#pragma unroll 4
    for (size_t i = (size_t)blockIdx.x * FOCAL_THREADS + threadIdx.x; i < ncells; i += (size_t)gridDim.x * FOCAL_THREADS) {
        int q;
        if (dsm_quantum(dsm[i], nodata, q)) {
            lo = min(lo, q);
            hi = max(hi, q);
            ++cnt;
        }
    }
#pragma unroll
    for (int by = 32; by >= 1; by >>= 1) {
        lo = min(lo, __shfl_xor(lo, by));
        hi = max(hi, __shfl_xor(hi, by));
        cnt += __shfl_xor(cnt, by);
    }
    if ((threadIdx.x & 63) == 0) {
        w_lo[threadIdx.x >> 6] = lo;
        w_hi[threadIdx.x >> 6] = hi;
        w_cnt[threadIdx.x >> 6] = cnt;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int w = 1; w < FOCAL_WAVES; ++w) {
        lo = min(lo, w_lo[w]);
        hi = max(hi, w_hi[w]);
        cnt += w_cnt[w];
    }
    if (cnt > 0) {
        atomicMin(hdr + FH_QMIN, (i64)lo);
        atomicMax(hdr + FH_QMAX, (i64)hi);
        atomicAdd((u64*)(hdr + FH_NVALID), (u64)cnt);
    }
}

__global__ void dsm_focal_header(i64* __restrict__ hdr)
{
    if (threadIdx.x != 0) return;
    const bool some = hdr[FH_NVALID] > 0;
    const i64 lo = some ? hdr[FH_QMIN] : 0, hi = some ? hdr[FH_QMAX] : 0;
    const i64 c = (lo + hi) >> 1;
    hdr[FH_QMIN] = lo;
    hdr[FH_QMAX] = hi;
    hdr[FH_CENTRE] = c;
    hdr[FH_MAXABS] = max(c - lo, hi - c);
}

// ---- the column pass -------------------------------------------------------------------------------------------------------------
struct FocalTotals { int* n; i64* s1; u64* s2; };

__global__ __launch_bounds__(FOCAL_THREADS)
void dsm_focal_band_totals(const float* __restrict__ dsm, int gw, int gh, float nodata, const i64* __restrict__ hdr, FocalTotals t)
{
    const unsigned cw = ((unsigned)gw + FOCAL_THREADS - 1) / FOCAL_THREADS;
    const int band = (int)(blockIdx.x / cw), col = (int)(blockIdx.x % cw) * FOCAL_THREADS + threadIdx.x;
    if (col >= gw) return;
    const i64 c = hdr[FH_CENTRE];
    const int r0 = band * FOCAL_BAND;
    int n = 0;
    i64 s1 = 0;
    u64 s2 = 0;
#pragma unroll
    for (int k = 0; k < FOCAL_BAND; ++k) {
        i64 d;
        if (r0 + k < gh && focal_cell(dsm[(size_t)(r0 + k) * gw + col], nodata, c, d)) {
            ++n;
            s1 += d;
            s2 += (u64)(d * d);
        }
    }
    const size_t at = (size_t)band * gw + col;
    t.n[at] = n;
    t.s1[at] = s1;
    t.s2[at] = s2;
}

__global__ __launch_bounds__(FOCAL_THREADS)
void dsm_focal_band_scan(int gw, int bands, FocalTotals t)
{
    const int col = blockIdx.x * FOCAL_THREADS + threadIdx.x;
    if (col >= gw) return;
    int n = 0;
    i64 s1 = 0;
    u64 s2 = 0;
    for (int b0 = 0; b0 < bands; b0 += FOCAL_SCAN_BATCH) {   // a batch's loads are in flight together: the walk waits once per batch
        int dn[FOCAL_SCAN_BATCH];
        i64 d1[FOCAL_SCAN_BATCH];
        u64 d2[FOCAL_SCAN_BATCH];
#pragma unroll
        for (int k = 0; k < FOCAL_SCAN_BATCH; ++k) {
            const bool in = b0 + k < bands;
            const size_t at = (size_t)(in ? b0 + k : b0) * gw + col;
            dn[k] = in ? t.n[at] : 0;
            d1[k] = in ? t.s1[at] : 0;
            d2[k] = in ? t.s2[at] : 0;
        }
#pragma unroll
        for (int k = 0; k < FOCAL_SCAN_BATCH; ++k) {
            if (b0 + k < bands) {
                const size_t at = (size_t)(b0 + k) * gw + col;
                t.n[at] = n;
                t.s1[at] = s1;
                t.s2[at] = s2;
                n += dn[k];
                s1 += d1[k];
                s2 += d2[k];
            }
        }
    }
}

__global__ __launch_bounds__(FOCAL_THREADS)
void dsm_focal_columns(const float* __restrict__ dsm, int gw, int gh, float nodata, const i64* __restrict__ hdr, FocalTotals t,
                   int* __restrict__ N, i64* __restrict__ S1, u64* __restrict__ S2)
{
    const unsigned cw = ((unsigned)gw + FOCAL_THREADS - 1) / FOCAL_THREADS;
    const int band = (int)(blockIdx.x / cw), col = (int)(blockIdx.x % cw) * FOCAL_THREADS + threadIdx.x;
    if (col >= gw) return;
    const i64 c = hdr[FH_CENTRE];
    const int r0 = band * FOCAL_BAND;
    const size_t at = (size_t)band * gw + col;
    int n = t.n[at];
    i64 s1 = t.s1[at];
    u64 s2 = t.s2[at];
    float z[FOCAL_BAND];
#pragma unroll
    for (int k = 0; k < FOCAL_BAND; ++k) z[k] = r0 + k < gh ? dsm[(size_t)(r0 + k) * gw + col] : nodata;
#pragma unroll
    for (int k = 0; k < FOCAL_BAND; ++k) {
        if (r0 + k >= gh) break;
        i64 d;
        if (focal_cell(z[k], nodata, c, d)) {
            ++n;
            s1 += d;
            s2 += (u64)(d * d);
        }
        const size_t e = (size_t)(r0 + k + 1) * (gw + 1) + (col + 1);
        N[e] = n;
        S1[e] = s1;
        S2[e] = s2;
    }
}

// ---- the row pass ----------------------------------------------------------------------------------------------------------------
// Table row blockIdx.x, entries 1 .. gw scanned in place; entry 0 and all of row 0 are the zeros a query at the grid's edge reads.
__global__ __launch_bounds__(FOCAL_THREADS)
void dsm_focal_rows(int gw, int* __restrict__ N, i64* __restrict__ S1, u64* __restrict__ S2)
{
    __shared__ int w_n[FOCAL_WAVES];
    __shared__ u64 w_1[FOCAL_WAVES], w_2[FOCAL_WAVES];
    const size_t row = (size_t)blockIdx.x * (gw + 1);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x == 0) {
        for (int e = threadIdx.x; e <= gw; e += FOCAL_THREADS) {
            N[e] = 0;
            S1[e] = 0;
            S2[e] = 0;
        }
        return;
    }
    if (threadIdx.x == 0) {
        N[row] = 0;
        S1[row] = 0;
        S2[row] = 0;
    }
    int cn = 0;                                              // the carry: the sums of the segments before this one
    u64 c1 = 0, c2 = 0;                                      // S1 as its two's complement image: the sums wrap alike
    for (int base = 1; base <= gw; base += FOCAL_SEG) {
        const int e0 = base + (int)threadIdx.x * 4;
        int a[4];
        u64 b[4], c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = e0 + k <= gw;
            a[k] = in ? N[row + e0 + k] : 0;
            b[k] = in ? (u64)S1[row + e0 + k] : 0;
            c[k] = in ? S2[row + e0 + k] : 0;
        }
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            a[k] += a[k - 1];
            b[k] += b[k - 1];
            c[k] += c[k - 1];
        }
        int sn = a[3];                                       // inclusive over the lanes of the wave
        u64 s1 = b[3], s2 = c[3];
#pragma unroll
        for (int by = 1; by < 64; by <<= 1) {
            const int un = focal_up(sn, by);
            const u64 u1 = focal_up(s1, by), u2 = focal_up(s2, by);
            if (lane >= by) {
                sn += un;
                s1 += u1;
                s2 += u2;
            }
        }
        __syncthreads();                                     // the last step's readers are done with w_*
        if (lane == 63) {
            w_n[wave] = sn;
            w_1[wave] = s1;
            w_2[wave] = s2;
        }
        __syncthreads();
        int on = cn + sn - a[3];                             // what lies before this lane's first entry
        u64 o1 = c1 + s1 - b[3], o2 = c2 + s2 - c[3];
#pragma unroll
        for (int w = 0; w < FOCAL_WAVES; ++w) {
            if (w < wave) {
                on += w_n[w];
                o1 += w_1[w];
                o2 += w_2[w];
            }
            cn += w_n[w];
            c1 += w_1[w];
            c2 += w_2[w];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (e0 + k <= gw) {
                N[row + e0 + k] = on + a[k];
                S1[row + e0 + k] = (i64)(o1 + b[k]);
                S2[row + e0 + k] = o2 + c[k];
            }
        }
    }
}

// ---- the query -------------------------------------------------------------------------------------------------------------------
// A record in 57 bits: the four offsets + 4096 in 14 bits each (dx0, dx1, dy0, dy1 from bit 0), bit 56 set for sign -1.
struct FocalChunk { u64 v[FOCAL_CHUNK]; };

__global__ __launch_bounds__(FOCAL_CHUNK)
void dsm_focal_upload(FocalChunk chunk, int count, u64* __restrict__ rects)
{
    if ((int)threadIdx.x < count) rects[threadIdx.x] = chunk.v[threadIdx.x];
}

struct FocalQuery {
    const i64* hdr;
    const int* N;
    const i64* S1;
    const u64* S2;
    const u64* rects;
    int gw, gh, n_rects, ow, oh, c0, r0, sx, sy, min_valid;
    i64 area;                                                // W+: the unclipped cells of the positive rectangles
    int* n;
    i64* s1;
    u64* s2;
    double* mean;
    double* var;
    int* status;
};

__global__ __launch_bounds__(FOCAL_THREADS)
void dsm_focal_query(FocalQuery a)
{
    const size_t i = (size_t)blockIdx.x * FOCAL_THREADS + threadIdx.x;
    if (i == 0) {
        const u128 D = (u128)(u64)a.hdr[FH_MAXABS];
        a.status[0] = (u128)(u64)a.area * D * D >= ((u128)1 << 63) ? 1 : 0;
    }
    if (i >= (size_t)a.ow * a.oh) return;
    const int R = (int)(i / a.ow), C = (int)(i % a.ow);
    const int r = a.r0 + R * a.sy, c = a.c0 + C * a.sx;
    const int pitch = a.gw + 1;
    int n = 0;
    u64 s1 = 0, s2 = 0;
    for (int k = 0; k < a.n_rects; ++k) {
        const u64 rec = a.rects[k];
        const int dx0 = (int)(rec & 0x3fff) - FOCAL_MAX_OFFSET, dx1 = (int)((rec >> 14) & 0x3fff) - FOCAL_MAX_OFFSET;
        const int dy0 = (int)((rec >> 28) & 0x3fff) - FOCAL_MAX_OFFSET, dy1 = (int)((rec >> 42) & 0x3fff) - FOCAL_MAX_OFFSET;
        const bool minus = (rec >> 56) & 1;
        const int x0 = min(max(c + dx0, 0), a.gw), y0 = min(max(r + dy0, 0), a.gh);              // table columns and rows
        const int x1 = max(min(max(c + dx1 + 1, 0), a.gw), x0), y1 = max(min(max(r + dy1 + 1, 0), a.gh), y0);
        const size_t e00 = (size_t)y0 * pitch + x0, e01 = (size_t)y0 * pitch + x1;
        const size_t e10 = (size_t)y1 * pitch + x0, e11 = (size_t)y1 * pitch + x1;
        const int dn = a.N[e11] - a.N[e01] - a.N[e10] + a.N[e00];
        const u64 d1 = (u64)a.S1[e11] - (u64)a.S1[e01] - (u64)a.S1[e10] + (u64)a.S1[e00];
        const u64 d2 = a.S2[e11] - a.S2[e01] - a.S2[e10] + a.S2[e00];
        n += minus ? -dn : dn;
        s1 += minus ? (u64)0 - d1 : d1;
        s2 += minus ? (u64)0 - d2 : d2;
    }
    const i64 t1 = (i64)s1;
    if (a.n) a.n[i] = n;
    if (a.s1) a.s1[i] = t1;
    if (a.s2) a.s2[i] = s2;
    if (!a.mean && !a.var) return;
    const bool some = n >= max(a.min_valid, 1);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double dn = (double)n;
    if (a.mean) a.mean[i] = some ? ((double)a.hdr[FH_CENTRE] + (double)t1 / dn) * 0.00390625 : nan;
    if (a.var) {
        const u64 m = (u64)(t1 < 0 ? -t1 : t1);
        const u128 V = (u128)(u64)(unsigned)n * (u128)s2 - (u128)m * (u128)m;
        const double Vd = (double)(u64)(V >> 64) * 18446744073709551616.0 + (double)(u64)V;
        a.var[i] = some ? Vd / (dn * dn) * 0.0000152587890625 : nan;
    }
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT size_t smvs_dsm_focal_table_bytes(int gw, int gh)
{
    using namespace smvs;
    if (focal_grid_check(gw, gh)) return 0;
    return focal_layout(gw, gh).bytes;
}

SMVS_EXPORT int smvs_dsm_focal_build(const float* dsm, int gw, int gh, float nodata, void* tables, size_t table_bytes, void* stream)
{
    using namespace smvs;
    if (!dsm || !tables) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = focal_grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s, got %d x %d", msg, gw, gh);
    const FocalLayout l = focal_layout(gw, gh);
    if (table_bytes < l.bytes) return fail(SMVS_ERR_ARG, "table buffer too small: %zu < %zu bytes", table_bytes, l.bytes);
    const size_t ncells = (size_t)gw * gh;
    if (dsm_overlap(tables, l.bytes, dsm, ncells * 4)) return fail(SMVS_ERR_ARG, "tables aliases dsm");
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)tables;
    i64* hdr = (i64*)base;
    int* N = (int*)(base + l.n);
    i64* S1 = (i64*)(base + l.s1);
    u64* S2 = (u64*)(base + l.s2);
    const FocalTotals t = {(int*)(base + l.tn), (i64*)(base + l.t1), (u64*)(base + l.t2)};
    const int bands = (gh + FOCAL_BAND - 1) / FOCAL_BAND;
    const size_t band_lanes = (size_t)bands * dsm_blocks((size_t)gw, FOCAL_THREADS) * FOCAL_THREADS;
    DSM_LAUNCH(dsm_focal_init, 64, 64, s, hdr);
    const unsigned range_blocks = min(dsm_blocks(ncells, FOCAL_THREADS), FOCAL_RANGE_BLOCKS);
    DSM_LAUNCH(dsm_focal_range, (size_t)range_blocks * FOCAL_THREADS, FOCAL_THREADS, s, dsm, (unsigned)ncells, nodata, hdr);
    DSM_LAUNCH(dsm_focal_header, 64, 64, s, hdr);
    DSM_LAUNCH(dsm_focal_band_totals, band_lanes, FOCAL_THREADS, s, dsm, gw, gh, nodata, (const i64*)hdr, t);
    DSM_LAUNCH(dsm_focal_band_scan, (size_t)gw, FOCAL_THREADS, s, gw, bands, t);
    DSM_LAUNCH(dsm_focal_columns, band_lanes, FOCAL_THREADS, s, dsm, gw, gh, nodata, (const i64*)hdr, t, N, S1, S2);
    DSM_LAUNCH(dsm_focal_rows, (size_t)(gh + 1) * FOCAL_THREADS, FOCAL_THREADS, s, gw, N, S1, S2);
    return SMVS_OK;
}

SMVS_EXPORT int smvs_dsm_focal_query(const void* tables, int gw, int gh, const int* rects, int n_rects, int ow, int oh, int c0, int r0,
                                     int sx, int sy, int min_valid, int* n, long long* s1, long long* s2, double* mean, double* var,
                                     int* status, void* stream)
{
    using namespace smvs;
    if (!tables || !rects || !status) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = focal_grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s, got %d x %d", msg, gw, gh);
    if (n_rects < 1 || n_rects > FOCAL_MAX_RECTS) return fail(SMVS_ERR_ARG, "n_rects must be in 1 .. %d, got %d", FOCAL_MAX_RECTS, n_rects);
    i64 area = 0;
    for (int k = 0; k < n_rects; ++k) {
        const int* q = rects + 5 * k;
        for (int j = 0; j < 4; ++j)
            if (q[j] < -FOCAL_MAX_OFFSET || q[j] > FOCAL_MAX_OFFSET)
                return fail(SMVS_ERR_ARG, "rectangle %d: offset %d outside -%d .. %d", k, q[j], FOCAL_MAX_OFFSET, FOCAL_MAX_OFFSET);
        if (q[0] > q[1] || q[2] > q[3]) return fail(SMVS_ERR_ARG, "rectangle %d: empty bounds (dx0 <= dx1 and dy0 <= dy1)", k);
        if (q[4] != 1 && q[4] != -1) return fail(SMVS_ERR_ARG, "rectangle %d: sign must be +1 or -1, got %d", k, q[4]);
        if (q[4] > 0) area += (i64)(q[1] - q[0] + 1) * (i64)(q[3] - q[2] + 1);
    }
    if (area > FOCAL_MAX_AREA) return fail(SMVS_ERR_ARG, "window too large: %lld positive cells, at most 2^24", area);
    if (sx < 1 || sy < 1 || ow < 1 || oh < 1) return fail(SMVS_ERR_ARG, "strides and output sizes must be >= 1");
    if (c0 < 0 || r0 < 0 || (i64)c0 + (i64)(ow - 1) * sx > (i64)gw - 1 || (i64)r0 + (i64)(oh - 1) * sy > (i64)gh - 1)
        return fail(SMVS_ERR_ARG, "an output centre lies outside the grid");
    if (min_valid < 0) return fail(SMVS_ERR_ARG, "min_valid must be >= 0, got %d", min_valid);
    const FocalLayout l = focal_layout(gw, gh);
    const size_t cells = (size_t)ow * (size_t)oh;
    const DsmBuf buf[] = {{tables, l.bytes, "tables"}, {n, cells * 4, "n"}, {s1, cells * 8, "s1"}, {s2, cells * 8, "s2"},
                          {mean, cells * 8, "mean"}, {var, cells * 8, "var"}, {status, 4, "status"}};
    const char* other;
    if (const char* name = dsm_first_alias(buf, 7, other)) return fail(SMVS_ERR_ARG, "%s aliases %s", name, other);
    hipStream_t s = (hipStream_t)stream;
    const char* base = (const char*)tables;
    u64* list = (u64*)(base + l.rects);                      // the buffer's tail: this query's records
    for (int k0 = 0; k0 < n_rects; k0 += FOCAL_CHUNK) {
        FocalChunk chunk;
        const int count = min(FOCAL_CHUNK, n_rects - k0);
        for (int k = 0; k < FOCAL_CHUNK; ++k) {
            const int* q = rects + 5 * (k0 + min(k, count - 1));
            chunk.v[k] = (u64)(q[0] + FOCAL_MAX_OFFSET) | (u64)(q[1] + FOCAL_MAX_OFFSET) << 14 | (u64)(q[2] + FOCAL_MAX_OFFSET) << 28 |
                         (u64)(q[3] + FOCAL_MAX_OFFSET) << 42 | (u64)(q[4] < 0) << 56;
        }
        DSM_LAUNCH(dsm_focal_upload, FOCAL_CHUNK, FOCAL_CHUNK, s, chunk, count, list + k0);
    }
    FocalQuery a;
    a.hdr = (const i64*)base;
    a.N = (const int*)(base + l.n);
    a.S1 = (const i64*)(base + l.s1);
    a.S2 = (const u64*)(base + l.s2);
    a.rects = list;
    a.gw = gw; a.gh = gh; a.n_rects = n_rects; a.ow = ow; a.oh = oh; a.c0 = c0; a.r0 = r0; a.sx = sx; a.sy = sy; a.min_valid = min_valid;
    a.area = area;
    a.n = n; a.s1 = s1; a.s2 = (u64*)s2; a.mean = mean; a.var = var; a.status = status;
    DSM_LAUNCH(dsm_focal_query, cells, FOCAL_THREADS, s, a);
    return SMVS_OK;
}

}  // extern "C"
