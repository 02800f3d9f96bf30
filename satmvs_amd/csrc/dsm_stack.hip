// dsm_stack.hip -- order statistics along the layer axis of a stack of DSMs ("Stack fusion";
// include/satmvs.h for the rules).
//
//   smvs_dsm_stack_select  per destination cell, the order statistics of up to 8 quantile levels among the layers valid there
//   smvs_dsm_stack_fuse    per destination cell, the linear median, the MAD about it, and the mean of the layers within
//                          max(kmad mad, floor) of the median, with the layers' membership and inlier bits
//
// Shape.  One lane per destination cell, 256 lanes a workgroup, flattened cells and the layer table in the kernel arguments as
// in dsm_mosaic.hip.  A lane keeps the keys of the layers valid at its cell in a column of dynamic LDS, keys[j * 256 + lane],
// n_layers KiB a workgroup: lanes are the fast index, so the 64 lanes of a wave always read 64 consecutive words, and a lane
// touches no column but its own, so there is no barrier.  The column is kept sorted by insertion while the layers are read, so
// the work follows the m layers actually present (m^2 / 4 moves on average); a 64-entry array in registers would spill, and the
// column costs no register at all.  The place of a new key is found by bisection and the entries above it then move up in a loop
// of known length, whose reads run ahead of its writes: a compare-and-move loop, one dependent LDS round trip a step, measured
// 1.15 x slower at 7 layers and 2.45 x at 64.  Every level, and the median, is then one LDS read.
// The MAD needs no second column and no second sort: about a centre c that lies between the two middle order statistics, the
// deviations (float)|z - c| do not fall along the sorted column below c going down, nor above c going up (a rounding is
// monotone), so the deviations in ascending order are a merge of those two arms outwards from the middle, read in place, and
// the merge stops at the rank asked for, (m - 1) / 2 + 1 steps.  The inlier pass reads the layers again in ascending k, the
// order the sum is defined in (the second read of a cell's layers hits L2; the membership bits skip what was void).
// The float64 operations are IEEE operations rounded one by one (__dsub_rn, __dadd_rn, __dmul_rn, __ddiv_rn) and the library
// is built with -ffp-contract=off besides.  No atomics, no workspace, no state, no host read-back: the result depends on the
// arguments alone.
#include <math.h>
#include <stdint.h>

#include "dsm_common.h"
#include "smvs_host.h"

namespace smvs {

constexpr int STACK_MAX_LAYERS = 64, STACK_THREADS = 256, STACK_MAX_LEVELS = 8, STACK_MAX_DEN = 1 << 16;

struct StackTable { smvs_dsm_layer layer[STACK_MAX_LAYERS]; };       // 2 KiB of kernel arguments
struct StackLevels { int n, num[STACK_MAX_LEVELS], den[STACK_MAX_LEVELS]; };

// The height of layer L on destination cell (R, C); false where the layer does not reach the cell or holds no height there.
__device__ __forceinline__ bool stack_read(const smvs_dsm_layer& L, int R, int C, float nodata, float& z)
{
    const long long r = (long long)R - L.oy, c = (long long)C - L.ox;
    if (r < 0 || r >= L.gh || c < 0 || c >= L.gw) return false;
    z = L.z[(size_t)r * (size_t)L.gw + (size_t)c];
    return dsm_cell_valid(z, nodata);
}

// key into the sorted column of m entries (stride STACK_THREADS); the caller counts it.
__device__ __forceinline__ void stack_insert(unsigned* col, int m, unsigned key)
{
    int at = 0, end = m;                                     // at: the first entry above `key`, by bisection
    while (at < end) {
        const int mid = (at + end) >> 1;
        if (col[mid * STACK_THREADS] <= key) at = mid + 1;
        else end = mid;
    }
#pragma unroll 4
    for (int j = m; j > at; --j) col[j * STACK_THREADS] = col[(j - 1) * STACK_THREADS];      // a known trip count: the reads run ahead of the writes
    col[at * STACK_THREADS] = key;
}

__device__ __forceinline__ float stack_dev(float z, double centre) { return (float)fabs(__dsub_rn((double)z, centre)); }

// a + (b - a) (rem / 2): the linear quantile at 1/2 between its two order statistics.
__device__ __forceinline__ double stack_middle(float a, float b, int rem)
{
    return __dadd_rn((double)a, __dmul_rn(__dsub_rn((double)b, (double)a), rem ? 0.5 : 0.0));
}

template <bool DEV>
__global__ __launch_bounds__(STACK_THREADS)
void dsm_stack_select(const StackTable t, int n_layers, float nodata, const StackLevels lv, const float* __restrict__ centre, int gw,
                      unsigned cells, unsigned char* __restrict__ count, float* __restrict__ lo, float* __restrict__ hi)
{
    extern __shared__ unsigned stack_lds[];
    const unsigned cell = blockIdx.x * (unsigned)STACK_THREADS + threadIdx.x;
    if (cell >= cells) return;
    unsigned* col = stack_lds + threadIdx.x;
    const int R = (int)(cell / (unsigned)gw), C = (int)(cell % (unsigned)gw);
    double cd = 0.0;
    bool open = true;                                        // a centre that is not finite closes the cell: m = 0
    if constexpr (DEV) {
        const float cf = centre[cell];
        open = isfinite(cf);
        cd = (double)cf;
    }
    int m = 0;
    if (open)
        for (int k = 0; k < n_layers; ++k) {
            float z;
            if (!stack_read(t.layer[k], R, C, nodata, z)) continue;
            stack_insert(col, m, f2key(DEV ? stack_dev(z, cd) : z));
            ++m;
        }
    if (count) count[cell] = (unsigned char)m;
    for (int j = 0; j < lv.n; ++j) {
        float a = nodata, b = nodata;
        if (m > 0) {
            const int h = (m - 1) * lv.num[j];               // below 2^6 * 2^16
            const int lo_rank = h / lv.den[j];
            a = key2f(col[lo_rank * STACK_THREADS]);
            b = h % lv.den[j] > 0 ? key2f(col[(lo_rank + 1) * STACK_THREADS]) : a;
        }
        lo[(size_t)j * cells + cell] = a;
        if (hi) hi[(size_t)j * cells + cell] = b;
    }
}

struct StackFuse {
    float* out;
    float* median;
    float* mad;
    unsigned char* count;
    unsigned char* n_in;
    long long* members;
    long long* inliers;
    double kmad, floor;
    int min_count, gw;
    unsigned cells;
    float nodata;
};

__global__ __launch_bounds__(STACK_THREADS)
void dsm_stack_fuse(const StackTable t, int n_layers, const StackFuse a)
{
    extern __shared__ unsigned stack_lds[];
    const unsigned cell = blockIdx.x * (unsigned)STACK_THREADS + threadIdx.x;
    if (cell >= a.cells) return;
    unsigned* col = stack_lds + threadIdx.x;
    const int R = (int)(cell / (unsigned)a.gw), C = (int)(cell % (unsigned)a.gw);
    const float nodata = a.nodata;
    int m = 0;
    unsigned long long members = 0ull;
    for (int k = 0; k < n_layers; ++k) {
        float z;
        if (!stack_read(t.layer[k], R, C, nodata, z)) continue;
        stack_insert(col, m, f2key(z));
        members |= 1ull << k;
        ++m;
    }
    float out = nodata, med32 = nodata, mad32 = nodata;
    unsigned long long inliers = 0ull;
    int n_in = 0;
    if (m >= max(a.min_count, 1)) {
        const int mid = (m - 1) / 2, rem = (m - 1) % 2;
        med32 = (float)stack_middle(key2f(col[mid * STACK_THREADS]), key2f(col[(mid + rem) * STACK_THREADS]), rem);
        // the deviations in ascending order: the arm below the median going down from `mid`, the arm above going up from
        // mid + 1, merged; d_lo and d_hi are the order statistics mid and mid + rem of them
        const double c = (double)med32;
        int i = mid, j = mid + 1;
        float di = stack_dev(key2f(col[i * STACK_THREADS]), c);
        float dj = j < m ? stack_dev(key2f(col[j * STACK_THREADS]), c) : 0.0f;
        float d_lo = 0.0f, d_hi = 0.0f;
        for (int s = 0; s <= mid + rem; ++s) {
            const bool left = i >= 0 && (j >= m || di <= dj);    // one arm always has an entry left: s < m
            const float d = left ? di : dj;
            if (left) {
                --i;
                if (i >= 0) di = stack_dev(key2f(col[i * STACK_THREADS]), c);
            } else {
                ++j;
                if (j < m) dj = stack_dev(key2f(col[j * STACK_THREADS]), c);
            }
            if (s == mid) d_lo = d;
            d_hi = d;
        }
        mad32 = (float)stack_middle(d_lo, d_hi, rem);
        const double thr = fmax(__dmul_rn(a.kmad, (double)mad32), a.floor);    // a NaN product loses
        double S = 0.0;
        for (int k = 0; k < n_layers; ++k) {
            if (!(members >> k & 1ull)) continue;
            float z;
            stack_read(t.layer[k], R, C, nodata, z);
            if (!((double)stack_dev(z, c) <= thr)) continue;
            S = n_in ? __dadd_rn(S, (double)z) : (double)z;
            inliers |= 1ull << k;
            ++n_in;
        }
        out = n_in ? (float)__ddiv_rn(S, (double)n_in) : med32;
    } else {
        members = 0ull;
    }
    a.out[cell] = out;
    if (a.median) a.median[cell] = med32;
    if (a.mad) a.mad[cell] = mad32;
    if (a.count) a.count[cell] = (unsigned char)m;
    if (a.n_in) a.n_in[cell] = (unsigned char)n_in;
    if (a.members) a.members[cell] = (long long)members;
    if (a.inliers) a.inliers[cell] = (long long)inliers;
}

// The checks the two entries share: the layer table and the buffers.  buf[first_out ..] are the outputs, which no layer may
// share a byte with; what stands before them is read only (a centre may well be one of the layers).
static int stack_table(const smvs_dsm_layer* layers, int n_layers, int gw, int gh, const DsmBuf* buf, int first_out, int n_buf, StackTable& t)
{
    if (n_layers < 1 || n_layers > STACK_MAX_LAYERS) return fail(SMVS_ERR_ARG, "n_layers must be in 1 .. %d, got %d", STACK_MAX_LAYERS, n_layers);
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "destination: %s", msg);
    const char* other;
    if (const char* name = dsm_first_alias(buf, n_buf, other)) return fail(SMVS_ERR_ARG, "%s aliases %s", name, other);
    for (int k = 0; k < n_layers; ++k) {
        const smvs_dsm_layer& L = layers[k];
        if (!L.z) return fail(SMVS_ERR_ARG, "layer %d: null z", k);
        if (const char* msg = grid_check(L.gw, L.gh)) return fail(SMVS_ERR_ARG, "layer %d: %s", k, msg);
        if (L.ox <= -(1 << 30) || L.ox >= (1 << 30) || L.oy <= -(1 << 30) || L.oy >= (1 << 30))
            return fail(SMVS_ERR_ARG, "layer %d: offset out of range: |ox|, |oy| must be below 2^30, got %d, %d", k, L.ox, L.oy);
        const size_t nl = (size_t)L.gw * L.gh * 4;
        for (int i = first_out; i < n_buf; ++i)
            if (buf[i].p && dsm_overlap(buf[i].p, buf[i].bytes, L.z, nl))
                return fail(SMVS_ERR_ARG, "%s aliases z of layer %d", buf[i].name, k);
        t.layer[k] = L;
        t.layer[k].d2 = nullptr;                             // not read here
    }
    return SMVS_OK;
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT int smvs_dsm_stack_select(const smvs_dsm_layer* layers, int n_layers, float nodata, const int* levels, int n_levels,
                                      const float* centre, int gw, int gh, unsigned char* count, float* lo, float* hi, void* stream)
{
    using namespace smvs;
    if (!layers || !levels || !lo) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (n_levels < 1 || n_levels > STACK_MAX_LEVELS) return fail(SMVS_ERR_ARG, "n_levels must be in 1 .. %d, got %d", STACK_MAX_LEVELS, n_levels);
    StackLevels lv = {};
    lv.n = n_levels;
    for (int j = 0; j < n_levels; ++j) {
        const int num = levels[2 * j], den = levels[2 * j + 1];
        if (den < 1 || den > STACK_MAX_DEN || num < 0 || num > den)
            return fail(SMVS_ERR_ARG, "level %d: 0 <= num <= den and 1 <= den <= 2^16, got %d / %d", j, num, den);
        lv.num[j] = num;
        lv.den[j] = den;
    }
    const size_t ncells = (size_t)(gw > 0 ? gw : 0) * (size_t)(gh > 0 ? gh : 0);
    // centre is only read, but an output on it would change what later cells read
    const DsmBuf buf[] = {{centre, ncells * 4, "centre"}, {count, ncells, "count"}, {lo, ncells * 4 * n_levels, "lo"}, {hi, ncells * 4 * n_levels, "hi"}};
    StackTable t = {};
    if (int rc = stack_table(layers, n_layers, gw, gh, buf, 1, 4, t)) return rc;
    const unsigned cells = (unsigned)ncells;
    const dim3 grid(dsm_blocks(cells, STACK_THREADS)), block(STACK_THREADS);
    const size_t lds = (size_t)n_layers * STACK_THREADS * 4;
    if (centre) hipLaunchKernelGGL(dsm_stack_select<true>, grid, block, lds, (hipStream_t)stream, t, n_layers, nodata, lv, centre, gw, cells, count, lo, hi);
    else hipLaunchKernelGGL(dsm_stack_select<false>, grid, block, lds, (hipStream_t)stream, t, n_layers, nodata, lv, centre, gw, cells, count, lo, hi);
    return check_launch("dsm_stack_select");
}

SMVS_EXPORT int smvs_dsm_stack_fuse(const smvs_dsm_layer* layers, int n_layers, float nodata, double kmad, double floor, int min_count,
                                    int gw, int gh, float* out, float* median, float* mad, unsigned char* count, unsigned char* n_in,
                                    long long* members, long long* inliers, void* stream)
{
    using namespace smvs;
    if (!layers || !out) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (!(isfinite(kmad) && kmad >= 0.0) || !(isfinite(floor) && floor >= 0.0))
        return fail(SMVS_ERR_ARG, "kmad and floor must be finite and >= 0, got %g and %g", kmad, floor);
    if (min_count < 0 || min_count > STACK_MAX_LAYERS) return fail(SMVS_ERR_ARG, "min_count must be in 0 .. %d, got %d", STACK_MAX_LAYERS, min_count);
    const size_t ncells = (size_t)(gw > 0 ? gw : 0) * (size_t)(gh > 0 ? gh : 0);
    const DsmBuf buf[] = {{out, ncells * 4, "out"}, {median, ncells * 4, "median"}, {mad, ncells * 4, "mad"}, {count, ncells, "count"},
                          {n_in, ncells, "n_in"}, {members, ncells * 8, "members"}, {inliers, ncells * 8, "inliers"}};
    StackTable t = {};
    if (int rc = stack_table(layers, n_layers, gw, gh, buf, 0, 7, t)) return rc;
    const unsigned cells = (unsigned)ncells;
    const StackFuse a = {out, median, mad, count, n_in, members, inliers, kmad, floor, min_count, gw, cells, nodata};
    hipLaunchKernelGGL(dsm_stack_fuse, dim3(dsm_blocks(cells, STACK_THREADS)), dim3(STACK_THREADS), (size_t)n_layers * STACK_THREADS * 4,
                       (hipStream_t)stream, t, n_layers, a);
    return check_launch("dsm_stack_fuse");
}

}  // extern "C"
