// dsm_rank.hip -- focal (moving-window) order statistics of a DSM: exact medians, quantiles and counts over any window within
// +-32 cells ("Focal order statistics"; include/satmvs.h for the rule).
//
//   smvs_dsm_focal_select  per cell, the order statistics of up to 4 quantile levels among the valid cells of its window
//   smvs_dsm_focal_count   per cell, how many valid cells of its window lie below a threshold and how many equal it
//
// One kernel each, no workspace, no atomics.  A workgroup of RANK_THREADS lanes owns a tile of RANK_TILE x RANK_TILE output cells
// and stages the tile plus the window's reach (at most 32 cells a side) into LDS: the order-preserving key of every cell, and
// RANK_VOID, which no finite float maps to, for a cell that is not valid or lies off the grid -- so a lane never clips its window.
// In deviation mode the staged word is the float itself (RANK_NOVALUE for a cell that is not valid) and the key of
// d = (float)fabs((double)v - (double)centre) is formed on every read.  The window is a list of row runs {dy, dx0, dx1} packed
// into 4 bytes each and passed by value in the kernel arguments (wave-uniform scalar reads), so two calls with different windows
// run side by side on two streams.
//
// A lane then selects for its own cells, one after the other: a pass over the window counts the valid cells, and for every level
// a most-significant-digit-first radix descent over the 32 key bits, RANK_BITS bits a round, finds the key of rank lo_rank.  A
// round counts, by compare-and-add into 2^RANK_BITS - 1 registers, the window cells that continue the prefix with a digit <= j;
// the digit of the rank is the number of counters that do not exceed it.  `hi` needs no second descent: one more pass counts the
// cells <= key(lo) and finds the smallest key above it.  Every result is a selection or a count: the bits depend on the inputs
// alone.
#include <stdint.h>

#include "dsm_common.h"
#include "smvs_host.h"

// Bits of one round of the descent: 1, 2 or 4.  tools/bench_dsm_rank.py builds the library a second time with another value to
// time the two formulations against each other (DESIGN.md section 9 has the table).
#ifndef SMVS_RANK_BITS
#define SMVS_RANK_BITS 2
#endif

namespace smvs {

constexpr int RANK_TILE = SMVS_DSM_RANK_TILE, RANK_THREADS = 256;
constexpr int RANK_CELLS = RANK_TILE * RANK_TILE / RANK_THREADS;  // output cells of one lane, RANK_ROWS rows apart
constexpr int RANK_ROWS = RANK_THREADS / RANK_TILE;
constexpr int RANK_MAX_RUNS = 130, RANK_MAX_OFFSET = 32, RANK_MAX_LEVELS = 4, RANK_MAX_DEN = 1 << 16;
constexpr int RANK_BITS = SMVS_RANK_BITS;
constexpr unsigned RANK_VOID = 0xffffffffu;                  // the key of float bits 0x7fffffff, a NaN: above every finite key
constexpr unsigned RANK_NOVALUE = 0x7fffffffu;               // that NaN itself, staged in deviation mode
static_assert(RANK_BITS == 1 || RANK_BITS == 2 || RANK_BITS == 4, "a round takes 1, 2 or 4 bits");
static_assert(RANK_TILE * RANK_TILE % RANK_THREADS == 0 && RANK_THREADS % RANK_TILE == 0, "whole rows of the tile per pass");

// Run k of the window, offsets measured from the staged region's corner: dy - dy_min | (dx0 - dx_min) << 7 | (dx1 - dx_min) << 14.
struct RankRuns { unsigned v[RANK_MAX_RUNS]; };

struct RankWindow {
    RankRuns runs;
    int n_runs, dy_min, dx_min, rows, pitch;                 // the staged region: rows x pitch words about a tile
};

struct RankLevels { int n, num[RANK_MAX_LEVELS], den[RANK_MAX_LEVELS]; };

// The key a staged word stands for.  DEV: the word is the float, the key that of its deviation from the centre.
template <bool DEV>
__device__ __forceinline__ unsigned rank_key(unsigned w, double centre)
{
    if constexpr (DEV) {
        if (w == RANK_NOVALUE) return RANK_VOID;
        return f2key((float)fabs(__dsub_rn((double)__uint_as_float(w), centre)));
    } else {
        return w;
    }
}

// f(word) over the window of the cell whose staged region starts at `cell`.
template <class F>
__device__ __forceinline__ void rank_walk(const RankWindow& w, const unsigned* cell, F&& f)
{
    for (int k = 0; k < w.n_runs; ++k) {
        const unsigned rec = w.runs.v[k];
        const unsigned* row = cell + (rec & 127u) * w.pitch;
        const int x1 = (int)((rec >> 14) & 127u);
#pragma unroll 4
        for (int x = (int)((rec >> 7) & 127u); x <= x1; ++x) f(row[x]);
    }
}

// The tile's region into LDS: `word(z)` for a cell of the grid, `off` beyond it.
template <class F>
__device__ __forceinline__ void rank_stage(const float* __restrict__ dsm, int gw, int gh, const RankWindow& w, int r0, int c0,
                                           unsigned* lds, unsigned off, F&& word)
{
    const int total = w.rows * w.pitch;
    for (int i = threadIdx.x; i < total; i += RANK_THREADS) {
        const int rr = i / w.pitch, cc = i - rr * w.pitch;
        const int r = r0 + w.dy_min + rr, c = c0 + w.dx_min + cc;
        lds[i] = (r >= 0 && r < gh && c >= 0 && c < gw) ? word(dsm[(size_t)r * gw + c]) : off;
    }
    __syncthreads();
}

// The key of 0-based rank k among the window's keys, k below the number of valid cells (RANK_VOID never continues a prefix with a
// digit below the highest, so it is never counted).
template <bool DEV>
__device__ __forceinline__ unsigned rank_descend(const RankWindow& w, const unsigned* cell, double centre, int k)
{
    constexpr int D = (1 << RANK_BITS) - 1;
    unsigned prefix = 0;
    for (int b = 32 - RANK_BITS; b >= 0; b -= RANK_BITS) {
        int cnt[D];
#pragma unroll
        for (int j = 0; j < D; ++j) cnt[j] = 0;
        rank_walk(w, cell, [&](unsigned word) {
            const unsigned t = (rank_key<DEV>(word, centre) ^ prefix) >> b;      // < 2^RANK_BITS iff the key continues the prefix
#pragma unroll
            for (int j = 0; j < D; ++j) cnt[j] += t <= (unsigned)j ? 1 : 0;
        });
        unsigned digit = 0;
        int skip = 0;
#pragma unroll
        for (int j = 0; j < D; ++j)
            if (k >= cnt[j]) {
                digit = j + 1;
                skip = cnt[j];
            }
        k -= skip;
        prefix |= digit << b;
    }
    return prefix;
}

struct RankSelect {
    const float* dsm;
    const float* centre;
    int* n_out;
    float* lo;
    float* hi;
    int gw, gh, tiles_x;
    float nodata;
};

template <bool DEV>
__global__ __launch_bounds__(RANK_THREADS)
void dsm_rank_select(RankSelect a, RankLevels lv, RankWindow w)
{
    extern __shared__ unsigned rank_lds[];
    const int r0 = (int)(blockIdx.x / a.tiles_x) * RANK_TILE, c0 = (int)(blockIdx.x % a.tiles_x) * RANK_TILE;
    const float nodata = a.nodata;
    if constexpr (DEV)
        rank_stage(a.dsm, a.gw, a.gh, w, r0, c0, rank_lds, RANK_NOVALUE,
                   [nodata](float z) { return dsm_cell_valid(z, nodata) ? __float_as_uint(z) : RANK_NOVALUE; });
    else
        rank_stage(a.dsm, a.gw, a.gh, w, r0, c0, rank_lds, RANK_VOID,
                   [nodata](float z) { return dsm_cell_valid(z, nodata) ? f2key(z) : RANK_VOID; });
    const int lx = threadIdx.x % RANK_TILE, ly = threadIdx.x / RANK_TILE;
    const size_t cells = (size_t)a.gw * a.gh;
    for (int q = 0; q < RANK_CELLS; ++q) {
        const int r = r0 + ly + q * RANK_ROWS, c = c0 + lx;
        if (r >= a.gh || c >= a.gw) continue;
        const size_t p = (size_t)r * a.gw + c;
        const unsigned* cell = rank_lds + (ly + q * RANK_ROWS) * w.pitch + lx;
        double centre = 0.0;
        bool open = true;                                    // a centre that is not finite closes the window: n = 0
        if constexpr (DEV) {
            const float cf = a.centre[p];
            open = isfinite(cf);
            centre = (double)cf;
        }
        int n = 0;
        if (open) rank_walk(w, cell, [&](unsigned word) { n += word != (DEV ? RANK_NOVALUE : RANK_VOID) ? 1 : 0; });
        if (a.n_out) a.n_out[p] = n;
        for (int j = 0; j < lv.n; ++j) {
            float lo = nodata, hi = nodata;
            if (n > 0) {
                const int h = (n - 1) * lv.num[j];           // below 2^13 * 2^16
                const int lo_rank = h / lv.den[j];
                const unsigned klo = rank_descend<DEV>(w, cell, centre, lo_rank);
                unsigned khi = klo;
                if (a.hi && h % lv.den[j] > 0) {
                    int upto = 0;                            // the cells <= key(lo); the next rank is past them, or among them
                    unsigned above = RANK_VOID;
                    rank_walk(w, cell, [&](unsigned word) {
                        const unsigned key = rank_key<DEV>(word, centre);
                        upto += key <= klo ? 1 : 0;
                        above = key > klo ? min(above, key) : above;
                    });
                    if (upto == lo_rank + 1) khi = above;
                }
                lo = key2f(klo);
                hi = key2f(khi);
            }
            a.lo[(size_t)j * cells + p] = lo;
            if (a.hi) a.hi[(size_t)j * cells + p] = hi;
        }
    }
}

struct RankCount {
    const float* dsm;
    const float* t;
    int* n_out;
    int* below;
    int* equal;
    int gw, gh, tiles_x;
    float nodata;
};

__global__ __launch_bounds__(RANK_THREADS)
void dsm_rank_count(RankCount a, RankWindow w)
{
    extern __shared__ unsigned rank_lds[];
    const int r0 = (int)(blockIdx.x / a.tiles_x) * RANK_TILE, c0 = (int)(blockIdx.x % a.tiles_x) * RANK_TILE;
    const float nodata = a.nodata;
    rank_stage(a.dsm, a.gw, a.gh, w, r0, c0, rank_lds, RANK_VOID,
               [nodata](float z) { return dsm_cell_valid(z, nodata) ? f2key(z) : RANK_VOID; });
    const int lx = threadIdx.x % RANK_TILE, ly = threadIdx.x / RANK_TILE;
    for (int q = 0; q < RANK_CELLS; ++q) {
        const int r = r0 + ly + q * RANK_ROWS, c = c0 + lx;
        if (r >= a.gh || c >= a.gw) continue;
        const size_t p = (size_t)r * a.gw + c;
        const unsigned* cell = rank_lds + (ly + q * RANK_ROWS) * w.pitch + lx;
        const float t = a.t[p];
        const unsigned tk = f2key(t);                        // RANK_VOID is above it, or t is a NaN and nothing is counted
        int n = 0, below = 0, equal = 0;
        rank_walk(w, cell, [&](unsigned key) {
            n += key != RANK_VOID ? 1 : 0;
            below += key < tk ? 1 : 0;
            equal += key == tk ? 1 : 0;
        });
        if (a.n_out) a.n_out[p] = n;
        a.below[p] = isnan(t) ? -1 : below;
        a.equal[p] = isnan(t) ? -1 : equal;
    }
}

// The checks of a window, and its packed form about the region it makes a tile stage.
static int rank_window(const int* runs, int n_runs, RankWindow& w)
{
    if (n_runs < 1 || n_runs > RANK_MAX_RUNS) return fail(SMVS_ERR_ARG, "n_runs must be in 1 .. %d, got %d", RANK_MAX_RUNS, n_runs);
    int dy_min = RANK_MAX_OFFSET, dy_max = -RANK_MAX_OFFSET, dx_min = RANK_MAX_OFFSET, dx_max = -RANK_MAX_OFFSET;
    for (int k = 0; k < n_runs; ++k) {
        const int* q = runs + 3 * k;
        for (int j = 0; j < 3; ++j)
            if (q[j] < -RANK_MAX_OFFSET || q[j] > RANK_MAX_OFFSET)
                return fail(SMVS_ERR_ARG, "run %d: offset %d outside -%d .. %d", k, q[j], RANK_MAX_OFFSET, RANK_MAX_OFFSET);
        if (q[1] > q[2]) return fail(SMVS_ERR_ARG, "run %d: empty bounds (dx0 <= dx1)", k);
        if (k > 0) {
            const int* o = q - 3;
            if (q[0] < o[0] || (q[0] == o[0] && q[1] <= o[2] + 1))
                return fail(SMVS_ERR_ARG, "run %d: runs are sorted by (dy, dx0), and the runs of one row neither overlap nor touch", k);
        }
        dy_min = min(dy_min, q[0]); dy_max = max(dy_max, q[0]);
        dx_min = min(dx_min, q[1]); dx_max = max(dx_max, q[2]);
    }
    w.n_runs = n_runs;
    w.dy_min = dy_min;
    w.dx_min = dx_min;
    w.rows = RANK_TILE + dy_max - dy_min;
    w.pitch = RANK_TILE + dx_max - dx_min;
    for (int k = 0; k < RANK_MAX_RUNS; ++k) {
        const int* q = runs + 3 * min(k, n_runs - 1);
        w.runs.v[k] = (unsigned)(q[0] - dy_min) | (unsigned)(q[1] - dx_min) << 7 | (unsigned)(q[2] - dx_min) << 14;
    }
    return SMVS_OK;
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT int smvs_dsm_focal_select(const float* dsm, int gw, int gh, float nodata, const int* runs, int n_runs, const int* levels,
                                      int n_levels, const float* centre, int* n_out, float* lo, float* hi, void* stream)
{
    using namespace smvs;
    if (!dsm || !runs || !levels || !lo) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s, got %d x %d", msg, gw, gh);
    RankWindow w;
    if (int rc = rank_window(runs, n_runs, w)) return rc;
    if (n_levels < 1 || n_levels > RANK_MAX_LEVELS) return fail(SMVS_ERR_ARG, "n_levels must be in 1 .. %d, got %d", RANK_MAX_LEVELS, n_levels);
    RankLevels lv = {};
    lv.n = n_levels;
    for (int j = 0; j < n_levels; ++j) {
        const int num = levels[2 * j], den = levels[2 * j + 1];
        if (den < 1 || den > RANK_MAX_DEN || num < 0 || num > den)
            return fail(SMVS_ERR_ARG, "level %d: 0 <= num <= den and 1 <= den <= 2^16, got %d / %d", j, num, den);
        lv.num[j] = num;
        lv.den[j] = den;
    }
    const size_t cells = (size_t)gw * gh;
    const DsmBuf buf[] = {{dsm, cells * 4, "dsm"}, {centre, cells * 4, "centre"}, {n_out, cells * 4, "n_out"},
                          {lo, cells * 4 * n_levels, "lo"}, {hi, cells * 4 * n_levels, "hi"}};
    const char* other;
    if (const char* name = dsm_first_alias(buf, 5, other)) return fail(SMVS_ERR_ARG, "%s aliases %s", name, other);
    const int tiles_x = (gw + RANK_TILE - 1) / RANK_TILE, tiles_y = (gh + RANK_TILE - 1) / RANK_TILE;
    const RankSelect a = {dsm, centre, n_out, lo, hi, gw, gh, tiles_x, nodata};
    const dim3 grid((unsigned)((size_t)tiles_x * tiles_y)), block(RANK_THREADS);
    const size_t lds = (size_t)w.rows * w.pitch * 4;
    if (centre) hipLaunchKernelGGL(dsm_rank_select<true>, grid, block, lds, (hipStream_t)stream, a, lv, w);
    else hipLaunchKernelGGL(dsm_rank_select<false>, grid, block, lds, (hipStream_t)stream, a, lv, w);
    return check_launch("dsm_rank_select");
}

SMVS_EXPORT int smvs_dsm_focal_count(const float* dsm, int gw, int gh, float nodata, const int* runs, int n_runs, const float* t,
                                     int* n_out, int* below, int* equal, void* stream)
{
    using namespace smvs;
    if (!dsm || !runs || !t || !below || !equal) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s, got %d x %d", msg, gw, gh);
    RankWindow w;
    if (int rc = rank_window(runs, n_runs, w)) return rc;
    const size_t cells = (size_t)gw * gh;
    // t may be the DSM itself (the elevation percentile): both are only read
    const DsmBuf buf[] = {{dsm, cells * 4, "dsm"}, {n_out, cells * 4, "n_out"}, {below, cells * 4, "below"}, {equal, cells * 4, "equal"}};
    const DsmBuf tbuf[] = {{t, cells * 4, "t"}, {n_out, cells * 4, "n_out"}, {below, cells * 4, "below"}, {equal, cells * 4, "equal"}};
    const char* other;
    if (const char* name = dsm_first_alias(buf, 4, other)) return fail(SMVS_ERR_ARG, "%s aliases %s", name, other);
    if (const char* name = dsm_first_alias(tbuf, 4, other)) return fail(SMVS_ERR_ARG, "%s aliases %s", name, other);
    const int tiles_x = (gw + RANK_TILE - 1) / RANK_TILE, tiles_y = (gh + RANK_TILE - 1) / RANK_TILE;
    const RankCount a = {dsm, t, n_out, below, equal, gw, gh, tiles_x, nodata};
    hipLaunchKernelGGL(dsm_rank_count, dim3((unsigned)((size_t)tiles_x * tiles_y)), dim3(RANK_THREADS), (size_t)w.rows * w.pitch * 4,
                       (hipStream_t)stream, a, w);
    return check_launch("dsm_rank_count");
}

}  // extern "C"
