// dsm_post.hip -- cleaning a DSM between production and rendering / orthorectification ("Cleaning a DSM").
//
//   smvs_dsm_despike  removes speckles: a valid cell goes where its (2 radius + 1)^2 window holds fewer than min_valid valid
//                     cells, or where it lies more than thresh from the window's median.
//   smvs_dsm_fill     fills voids: every invalid cell looks along eight directions for the first valid cell within max_steps and,
//                     with at least min_hits of them, takes their inverse-distance mean, the nearest or the lowest.
//
// Both are out of place and read the INPUT grid only, so no result depends on the order in which cells are processed, and both
// are selections and copies (plus, for the inverse-distance mean, a fixed sequence of IEEE float64 operations): bit-identical
// from run to run and to the numpy statement of the rules.
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "dsm_common.h"
#include "smvs_host.h"

namespace smvs {

constexpr unsigned POST_MAX_BLOCKS = 1u << 20;       // grid-stride over tiles beyond this

// ---- despike -----------------------------------------------------------------------------------------------------------------
// One lane per cell over a 64 x 16 tile staged once in LDS with its halo, as order-preserving keys; key 0 (no finite float has
// it) marks a cell that is invalid or off the grid.  The window's P = 16 / 32 / 64 slots (9 / 25 / 49 cells and P - N pads) are
// sorted by the bitonic network in registers.  Pads and invalid cells become sentinels below and above every height, taken in
// turn (above first), so that with n valid cells the P - n sentinels split into floor((P - n) / 2) below and the rest above:
// the valid keys sit in the middle and the median is at a fixed place, slot P/2 - 1 for odd n, slots P/2 - 1 and P/2 for even n.
// Every index is static, so the window stays in registers.
constexpr int SPIKE_TW = 64, SPIKE_TH = 16, SPIKE_THREADS = 256;

template <int R>
__global__ __launch_bounds__(SPIKE_THREADS)
void dsm_despike_kernel(const float* __restrict__ in, int gw, int gh, float nodata, double thresh, int min_valid,
                        float* __restrict__ out, unsigned char* __restrict__ removed)
{
    constexpr int N = (2 * R + 1) * (2 * R + 1), P = R == 1 ? 16 : R == 2 ? 32 : 64;
    constexpr int LW = SPIKE_TW + 2 * R, LH = SPIKE_TH + 2 * R;
    __shared__ unsigned tile[LH * LW];
    const unsigned nbx = (unsigned)(gw + SPIKE_TW - 1) / SPIKE_TW, nby = (unsigned)(gh + SPIKE_TH - 1) / SPIKE_TH;
    const unsigned ntiles = nbx * nby;
    for (unsigned t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int c0 = (int)(t % nbx) * SPIKE_TW, r0 = (int)(t / nbx) * SPIKE_TH;
        for (int i = threadIdx.x; i < LH * LW; i += SPIKE_THREADS) {
            const int r = r0 - R + i / LW, c = c0 - R + i % LW;
            unsigned k = 0u;
            if (r >= 0 && r < gh && c >= 0 && c < gw) {
                const float z = in[(size_t)r * gw + c];
                if (dsm_cell_valid(z, nodata)) k = f2key(z);
            }
            tile[i] = k;
        }
        __syncthreads();
        const int lx = threadIdx.x % SPIKE_TW;
        for (int ly = threadIdx.x / SPIKE_TW; ly < SPIKE_TH; ly += SPIKE_THREADS / SPIKE_TW) {
            const int r = r0 + ly, c = c0 + lx;
            if (r >= gh || c >= gw) continue;
            const size_t cell = (size_t)r * gw + c;
            const float z = in[cell];
            bool rm = false;
            if (dsm_cell_valid(z, nodata)) {
                unsigned v[P];
#pragma unroll
                for (int k = 0; k < P - N; ++k) v[k] = (k & 1) ? 0u : 0xffffffffu;
                int inv = P - N;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const unsigned key = tile[(ly + k / (2 * R + 1)) * LW + lx + k % (2 * R + 1)];
                    const bool bad = key == 0u;
                    v[P - N + k] = bad ? ((inv & 1) ? 0u : 0xffffffffu) : key;
                    inv += bad ? 1 : 0;
                }
                const int n = P - inv;
                if (n < min_valid) rm = true;
                else {
                    bitonic_net<P, 2, 1>(v);
                    const float lo = key2f(v[P / 2 - 1]);
                    const float m = (n & 1) ? lo : (float)(0.5 * ((double)lo + (double)key2f(v[P / 2])));
                    rm = fabs((double)z - (double)m) > thresh;
                }
            }
            out[cell] = rm ? nodata : z;
            if (removed) removed[cell] = rm ? 1 : 0;
        }
        __syncthreads();                                     // the tile is reused by the next one
    }
}

// ---- fill --------------------------------------------------------------------------------------------------------------------
// Directions as (dcol, drow), rows running south: E, NE, N, NW, W, SW, S, SE.
__device__ __forceinline__ int fill_dcol(int d) { return (d == 0 || d == 1 || d == 7) ? 1 : (d == 2 || d == 6) ? 0 : -1; }
__device__ __forceinline__ int fill_drow(int d) { return (d >= 1 && d <= 3) ? -1 : (d >= 5) ? 1 : 0; }

constexpr int FILL_THREADS = 256;
constexpr int FILL_MIN_BAND = 32;
constexpr int FILL_NO_HIT = 1 << 20;                 // "no valid cell seen on this line yet", above every max_steps
constexpr int FILL_PLANES = 6;                       // NE, N, NW, SW, S, SE: the directions that cross rows

// The hit of direction d is a state carried along the line of d: marching AGAINST d, a lane counts the steps since the last
// valid cell it passed and hands every invalid cell that count, its k_d (0: no hit within max_steps).  Only the count is
// stored; the combine reads the height at p + k d from the input, so the state is never computed with.  A lane owns one line
// (a column for N and S, a diagonal for the others: at step t it is in column j + t mc, so the lanes of a wave read consecutive
// columns of one row) within one band of rows; it starts max_steps rows before the band to warm its state up, and a diagonal
// that enters the grid from outside starts with no hit.  blockIdx.y = band, blockIdx.z = plane.
__global__ __launch_bounds__(FILL_THREADS)
void dsm_fill_march(const float* __restrict__ in, int gw, int gh, float nodata, int max_steps, int band,
                    unsigned short* __restrict__ planes, size_t plane_stride)
{
    const int p = blockIdx.z;
    const int d = p < 3 ? p + 1 : p + 2;
    const int mr = -fill_drow(d), mc = -fill_dcol(d);
    const int b0 = (int)blockIdx.y * band, b1 = min(gh, b0 + band);
    // rows rs, rs + mr, ... (T of them) end on the band's far row; the first |b - rs| of them only warm up
    const int rs = mr > 0 ? max(0, b0 - max_steps) : min(gh - 1, b1 - 1 + max_steps);
    const int T = mr > 0 ? b1 - rs : rs - b0 + 1;
    const long long lane = (long long)blockIdx.x * FILL_THREADS + threadIdx.x;
    if (lane >= (long long)gw + (mc != 0 ? T - 1 : 0)) return;
    const int j = (int)(mc > 0 ? lane - (T - 1) : lane);
    unsigned short* __restrict__ plane = planes + (size_t)p * plane_stride;
    int since = FILL_NO_HIT;
#pragma unroll 4
    for (int t = 0; t < T; ++t) {
        const int r = rs + t * mr, c = j + t * mc;
        const bool on = c >= 0 && c < gw;
        const size_t cell = (size_t)r * gw + min(max(c, 0), gw - 1);
        const bool valid = on && dsm_cell_valid(in[cell], nodata);
        since = min(since + 1, FILL_NO_HIT);
        if (on && !valid && r >= b0 && r < b1) plane[cell] = (unsigned short)(since <= max_steps ? since : 0);
        since = valid ? 0 : on ? since : FILL_NO_HIT;
    }
}

// The first valid cell east and west of every lane's cell, along the row: a wave holds 64 consecutive columns, a ballot of
// their validity answers for the cells inside the wave, and the lanes that find nothing there look at the next 64 columns at a
// time (the first chunk with a valid cell answers for all of them).  k = 0: no hit within max_steps.
__device__ __forceinline__ void fill_row_hits(const float* __restrict__ row, int gw, float nodata, int max_steps, int c, bool valid,
                                              int& kE, int& kW)
{
    const unsigned L = __lane_id();
    const int w0 = c - (int)L;                               // the wave's first column
    const unsigned long long mask = __ballot(valid);
    const unsigned long long east = L == 63 ? 0ull : mask & ~((2ull << L) - 1ull);
    const unsigned long long west = mask & ((1ull << L) - 1ull);
    kE = east ? __builtin_ctzll(east) - (int)L : 0;
    kW = west ? (int)L - (63 - __builtin_clzll(west)) : 0;
    const bool want = !valid && c < gw;
    for (int base = w0 + 64; base < gw && base - (w0 + 63) <= max_steps && __ballot(want && kE == 0); base += 64) {
        const int cc = base + (int)L;
        const unsigned long long m = __ballot(cc < gw && dsm_cell_valid(row[min(cc, gw - 1)], nodata));
        if (m) {
            if (kE == 0) kE = base + __builtin_ctzll(m) - c;
            break;
        }
    }
    for (int base = w0 - 64; base + 63 >= 0 && w0 - (base + 63) <= max_steps && __ballot(want && kW == 0); base -= 64) {
        const int cc = base + (int)L;
        const unsigned long long m = __ballot(cc >= 0 && dsm_cell_valid(row[max(cc, 0)], nodata));
        if (m) {
            if (kW == 0) kW = c - (base + 63 - __builtin_clzll(m));
            break;
        }
    }
    if (kE > max_steps) kE = 0;
    if (kW > max_steps) kW = 0;
}

// One lane per cell, a workgroup on 256 consecutive columns of one row.  Valid cells are copied.  An invalid cell gathers its
// eight hits (E and W from the row, the others from the march planes), and with at least min_hits of them takes the value of
// `method` over the hit directions in their fixed order: 0 inverse-distance mean in float64 (w = 1 / d2, d2 = k^2, doubled on a
// diagonal; num and den summed from 0.0), 1 the smallest d2, 2 the lowest height; ties keep the earlier direction.
__global__ __launch_bounds__(FILL_THREADS)
void dsm_fill_combine(const float* __restrict__ in, int gw, int gh, float nodata, int max_steps, int min_hits, int method,
                      const unsigned short* __restrict__ planes, size_t plane_stride,
                      float* __restrict__ out, unsigned char* __restrict__ hits_out)
{
    const unsigned nbx = (unsigned)(gw + FILL_THREADS - 1) / FILL_THREADS;
    const unsigned ntiles = nbx * (unsigned)gh;
    for (unsigned t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int r = (int)(t / nbx), c = (int)(t % nbx) * FILL_THREADS + (int)threadIdx.x;
        const float* row = in + (size_t)r * gw;
        const float z = c < gw ? row[c] : 0.0f;
        const bool valid = c < gw && dsm_cell_valid(z, nodata);
        int k[8];
        k[0] = k[4] = 0;
        if (__ballot(!valid && c < gw)) fill_row_hits(row, gw, nodata, max_steps, c, valid, k[0], k[4]);
        if (c >= gw) continue;
        const size_t cell = (size_t)r * gw + c;
        if (valid) {
            out[cell] = z;
            if (hits_out) hits_out[cell] = 255;
            continue;
        }
#pragma unroll
        for (int p = 0; p < FILL_PLANES; ++p) k[p < 3 ? p + 1 : p + 2] = planes[(size_t)p * plane_stride + cell];
        int hits = 0;
        double num = 0.0, den = 0.0;
        long long best_d2 = LLONG_MAX;
        float pick = z;
        bool first = true;
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            if (k[d] == 0) continue;
            const int hr = r + k[d] * fill_drow(d), hc = c + k[d] * fill_dcol(d);
            if (hr < 0 || hr >= gh || hc < 0 || hc >= gw) continue;      // cannot happen: a count never leaves the grid
            const float zd = in[(size_t)hr * gw + hc];
            ++hits;
            const long long d2 = (long long)k[d] * k[d] * ((d & 1) ? 2 : 1);
            if (method == 0) {
                const double w = 1.0 / (double)d2;
                num += w * (double)zd;
                den += w;
            } else if (method == 1) {
                if (d2 < best_d2) { best_d2 = d2; pick = zd; }
            } else if (first || zd < pick) {
                pick = zd;
                first = false;
            }
        }
        const bool fill = hits >= min_hits;
        out[cell] = !fill ? z : method == 0 ? (float)(num / den) : pick;
        if (hits_out) hits_out[cell] = (unsigned char)hits;
    }
}

// Rows per band of the march: at least max_steps, so that a lane warms up over no more rows than it serves, and enough that
// the bands fit the launch grid.
static int fill_band(int gh, int max_steps) { return std::max({FILL_MIN_BAND, max_steps, (gh + 65534) / 65535}); }

}  // namespace smvs

extern "C" {

SMVS_EXPORT int smvs_dsm_despike(const float* dsm, int gw, int gh, float nodata, int radius, double thresh, int min_valid,
                                 float* out, unsigned char* removed, void* stream)
{
    using namespace smvs;
    if (!dsm || !out) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (radius < 1 || radius > 3) return fail(SMVS_ERR_ARG, "radius must be 1, 2 or 3");
    if (!(thresh >= 0.0) || !isfinite(thresh)) return fail(SMVS_ERR_ARG, "thresh must be finite and >= 0");
    const int window = (2 * radius + 1) * (2 * radius + 1);
    if (min_valid < 1 || min_valid > window) return fail(SMVS_ERR_ARG, "min_valid must be in 1 .. %d (the window of radius %d)", window, radius);
    const size_t ncells = (size_t)gw * gh;
    if (dsm_overlap(dsm, ncells * 4, out, ncells * 4)) return fail(SMVS_ERR_ARG, "out aliases dsm: the operation is out of place");
    if (removed && (dsm_overlap(dsm, ncells * 4, removed, ncells) || dsm_overlap(out, ncells * 4, removed, ncells)))
        return fail(SMVS_ERR_ARG, "removed aliases dsm or out");
    const unsigned ntiles = (unsigned)((gw + SPIKE_TW - 1) / SPIKE_TW) * (unsigned)((gh + SPIKE_TH - 1) / SPIKE_TH);
    const dim3 grid(std::min(ntiles, POST_MAX_BLOCKS)), block(SPIKE_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (radius == 1) hipLaunchKernelGGL(dsm_despike_kernel<1>, grid, block, 0, s, dsm, gw, gh, nodata, thresh, min_valid, out, removed);
    else if (radius == 2) hipLaunchKernelGGL(dsm_despike_kernel<2>, grid, block, 0, s, dsm, gw, gh, nodata, thresh, min_valid, out, removed);
    else hipLaunchKernelGGL(dsm_despike_kernel<3>, grid, block, 0, s, dsm, gw, gh, nodata, thresh, min_valid, out, removed);
    return check_launch("dsm_despike");
}

SMVS_EXPORT size_t smvs_dsm_fill_workspace_bytes(int gw, int gh, int max_steps)
{
    using namespace smvs;
    if (grid_check(gw, gh) || max_steps < 1 || max_steps > 4096) return 0;
    return FILL_PLANES * align256((size_t)gw * gh * sizeof(unsigned short));
}

SMVS_EXPORT int smvs_dsm_fill(const float* dsm, int gw, int gh, float nodata, int max_steps, int min_hits, int method,
                              float* out, unsigned char* hits, void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!dsm || !out || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (max_steps < 1 || max_steps > 4096) return fail(SMVS_ERR_ARG, "max_steps must be in 1 .. 4096");
    if (min_hits < 1 || min_hits > 8) return fail(SMVS_ERR_ARG, "min_hits must be in 1 .. 8");
    if (method < 0 || method > 2) return fail(SMVS_ERR_ARG, "method must be 0 (idw), 1 (nearest) or 2 (min)");
    const size_t ncells = (size_t)gw * gh;
    if (dsm_overlap(dsm, ncells * 4, out, ncells * 4)) return fail(SMVS_ERR_ARG, "out aliases dsm: the operation is out of place");
    if (hits && (dsm_overlap(dsm, ncells * 4, hits, ncells) || dsm_overlap(out, ncells * 4, hits, ncells)))
        return fail(SMVS_ERR_ARG, "hits aliases dsm or out");
    const size_t need = smvs_dsm_fill_workspace_bytes(gw, gh, max_steps);
    if (workspace_bytes < need) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    if (dsm_overlap(dsm, ncells * 4, workspace, need) || dsm_overlap(out, ncells * 4, workspace, need) || (hits && dsm_overlap(hits, ncells, workspace, need)))
        return fail(SMVS_ERR_ARG, "workspace aliases dsm, out or hits");
    hipStream_t s = (hipStream_t)stream;
    unsigned short* planes = (unsigned short*)workspace;
    const size_t plane_stride = need / FILL_PLANES / sizeof(unsigned short);
    const int band = fill_band(gh, max_steps);
    const int nbands = (gh + band - 1) / band;
    const long long lanes = (long long)gw + band + max_steps - 1;      // a diagonal band has gw + T - 1 lines, T <= band + max_steps
    int rc;
    hipLaunchKernelGGL(dsm_fill_march, dim3((unsigned)((lanes + FILL_THREADS - 1) / FILL_THREADS), (unsigned)nbands, FILL_PLANES),
                       dim3(FILL_THREADS), 0, s, dsm, gw, gh, nodata, max_steps, band, planes, plane_stride);
    if ((rc = check_launch("dsm_fill_march"))) return rc;
    const unsigned ntiles = (unsigned)((gw + FILL_THREADS - 1) / FILL_THREADS) * (unsigned)gh;
    hipLaunchKernelGGL(dsm_fill_combine, dim3(std::min(ntiles, POST_MAX_BLOCKS)), dim3(FILL_THREADS), 0, s,
                       dsm, gw, gh, nodata, max_steps, min_hits, method, planes, plane_stride, out, hits);
    return check_launch("dsm_fill_combine");
}

}  // extern "C"
