// dsm_mosaic.hip -- putting DSM tiles together ("Mosaic"; include/satmvs.h for the rules).
//
//   smvs_dsm_dist    the exact squared Euclidean distance of every cell to the nearest background cell of a mask, capped
//   smvs_dsm_mosaic  up to 64 integer-aligned layers combined into one grid: first / last / min / max / mean / feathered blend
//
// Distance.  d2(r, c) = min over columns c' of (c - c')^2 + g(r, c')^2 with g(r, c') the distance in rows to the nearest
// background cell of column c'.  Two kernels.  dsm_dist_cols: a lane owns one column within one band of rows and carries
// "rows since the last background cell" down and then up it, starting `cap` rows outside the band to warm the state up (the
// marches of dsm_post.hip); g <= cap <= 1024 is kept as uint16 in the workspace.  dsm_dist_rows: a workgroup stages g^2 of
// one row piece of 2048 cells and a halo of `cap` columns at both ends in LDS (off-grid columns 0 with a border, else cap^2)
// and lane c takes min over k of k^2 + min(g^2[c - k], g^2[c + k]) outwards from k = 0 while k^2 is below its current
// minimum; the lanes that are done drop out of the exec mask, so a wave runs as long as its largest minimum asks for, and
// all lanes read at one k: consecutive lanes on consecutive banks.  Integers only, every value a minimum: no order to
// depend on.  No atomics, no host synchronisation; both kernels write every cell they own, so neither the workspace nor
// the output needs initialising.
//
// Mosaic.  One lane per destination cell, the layer table in the kernel arguments (64 x 32 bytes), a loop over the layers
// in ascending order.  The float64 sums are IEEE operations rounded one by one: __dmul_rn, __dadd_rn, __dsqrt_rn and
// __ddiv_rn below, and the library is built with -ffp-contract=off besides (build.py), so no product is fused into a sum;
// the square root and the quotient are the correctly rounded ones (no fast-math flag is set).  No workspace, atomics or
// state: the result depends on the arguments alone.
#include <math.h>
#include <stdint.h>

#include "dsm_common.h"
#include "smvs_host.h"

namespace smvs {

constexpr int DIST_THREADS = 256;
constexpr int DIST_MAX = 1024;                       // the cap's limit: g fits 16 bits, g^2 and k^2 + g^2 fit 32
constexpr int DIST_ROW_SEG = 2048;                   // cells of a row that one workgroup writes
constexpr int DIST_ROW_CELLS = DIST_ROW_SEG + 2 * DIST_MAX;          // 16 KiB of LDS
constexpr int DIST_MIN_BAND = 32, DIST_MAX_BAND = 256;               // rows of a column that one lane writes: the cap between these

static int dist_band(int cap) { return cap < DIST_MIN_BAND ? DIST_MIN_BAND : cap > DIST_MAX_BAND ? DIST_MAX_BAND : cap; }

// g(r, c) for the rows of one band: blockIdx.x = band * nbx + (block of 256 columns).
__global__ __launch_bounds__(DIST_THREADS)
void dsm_dist_cols(const unsigned char* __restrict__ mask, int gw, int gh, int border, int cap, int band, unsigned nbx,
                   unsigned short* __restrict__ g)
{
    const int c = (int)(blockIdx.x % nbx) * DIST_THREADS + (int)threadIdx.x;
    if (c >= gw) return;
    const long long b0l = (long long)(blockIdx.x / nbx) * band;
    const int b0 = (int)b0l, b1 = (int)min((long long)gh, b0l + band);
    const int edge = border ? 0 : cap;                       // the state on the row just off the grid
    // down: a background cell more than cap rows above the band is as good as none
    const int rs = max(0, b0 - cap);
    int since = rs == 0 ? edge : cap;
#pragma unroll 4
    for (int r = rs; r < b1; ++r) {
        const size_t cell = (size_t)r * gw + c;
        since = mask[cell] ? min(since + 1, cap) : 0;
        if (r >= b0) g[cell] = (unsigned short)since;
    }
    // up: the lane reads back what it wrote itself
    const int re = (int)min((long long)gh - 1, (long long)b1 - 1 + cap);
    since = re == gh - 1 ? edge : cap;
#pragma unroll 4
    for (int r = re; r >= b0; --r) {
        const size_t cell = (size_t)r * gw + c;
        since = mask[cell] ? min(since + 1, cap) : 0;
        if (r < b1) g[cell] = (unsigned short)min((int)g[cell], since);
    }
}

// d2 of one row piece: blockIdx.x = row * nseg + piece.
__global__ __launch_bounds__(DIST_THREADS)
void dsm_dist_rows(const unsigned short* __restrict__ g, int gw, int border, int cap, unsigned nseg, int* __restrict__ d2)
{
    __shared__ int g2[DIST_ROW_CELLS];
    const size_t row = (size_t)(blockIdx.x / nseg) * gw;
    const int p0 = (int)(blockIdx.x % nseg) * DIST_ROW_SEG;
    const int nout = min(DIST_ROW_SEG, gw - p0);
    const int n = nout + 2 * cap, cap2 = cap * cap;          // staged: columns p0 - cap .. p0 + nout + cap - 1
    const int off = border ? 0 : cap2;
    for (int i = threadIdx.x; i < n; i += DIST_THREADS) {
        const int col = p0 - cap + i;
        int v = off;
        if (col >= 0 && col < gw) {
            const int t = (int)g[row + col];
            v = t * t;
        }
        g2[i] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nout; i += DIST_THREADS) {
        const int* __restrict__ at = g2 + cap + i;
        int best = at[0];                                    // <= cap^2, so k stays within the halo: k^2 < best gives k < cap
        for (int k = 1; k * k < best; ++k) best = min(best, k * k + min(at[-k], at[k]));
        d2[row + p0 + i] = best;
    }
}

// ---- mosaic ----------------------------------------------------------------------------------------------------------------
constexpr int MOSAIC_MAX_LAYERS = 64, MOSAIC_THREADS = 256;
enum { MOSAIC_FIRST = 0, MOSAIC_LAST = 1, MOSAIC_MIN = 2, MOSAIC_MAX = 3, MOSAIC_MEAN = 4, MOSAIC_FEATHER = 5 };

struct MosaicTable { smvs_dsm_layer layer[MOSAIC_MAX_LAYERS]; };     // 2 KiB of kernel arguments

__global__ __launch_bounds__(MOSAIC_THREADS)
void dsm_mosaic(const MosaicTable t, int n_layers, float nodata, int mode, int feather2, int gw, unsigned cells,
                float* __restrict__ out, unsigned char* __restrict__ count, unsigned char* __restrict__ source, float* __restrict__ spread)
{
    const unsigned cell = blockIdx.x * (unsigned)MOSAIC_THREADS + threadIdx.x;
    if (cell >= cells) return;
    const int R = (int)(cell / (unsigned)gw), C = (int)(cell % (unsigned)gw);
    int m = 0, src = 255;
    float pick = nodata;                                     // modes 0 .. 3: the bits taken
    unsigned pick_key = 0u, lo = 0u, hi = 0u;
    double S = 0.0, W = 0.0, wbest = 0.0;
    for (int k = 0; k < n_layers; ++k) {
        const smvs_dsm_layer& L = t.layer[k];
        const long long r = (long long)R - L.oy, c = (long long)C - L.ox;
        if (r < 0 || r >= L.gh || c < 0 || c >= L.gw) continue;
        const size_t at = (size_t)r * (size_t)L.gw + (size_t)c;
        const float z = L.z[at];
        if (!dsm_cell_valid(z, nodata)) continue;
        const unsigned key = f2key(z);
        const bool first = m == 0;
        lo = first ? key : min(lo, key);
        hi = first ? key : max(hi, key);
        if (mode == MOSAIC_FEATHER) {
            const double w = __dsqrt_rn((double)min(max(L.d2[at], 1), feather2));
            const double wz = __dmul_rn(w, (double)z);
            S = first ? wz : __dadd_rn(S, wz);
            W = first ? w : __dadd_rn(W, w);
            if (first || w > wbest) { wbest = w; src = k; }
        } else if (mode == MOSAIC_MEAN) {
            S = first ? (double)z : __dadd_rn(S, (double)z);
            if (first) src = k;
        } else {
            const bool take = first || mode == MOSAIC_LAST || (mode == MOSAIC_MIN && key < pick_key) || (mode == MOSAIC_MAX && key > pick_key);
            if (take) { pick = z; pick_key = key; src = k; }
        }
        ++m;
    }
    float res = nodata;
    if (m) res = mode == MOSAIC_FEATHER ? (float)__ddiv_rn(S, W) : mode == MOSAIC_MEAN ? (float)__ddiv_rn(S, (double)m) : pick;
    out[cell] = res;
    if (count) count[cell] = (unsigned char)m;
    if (source) source[cell] = (unsigned char)src;
    if (spread) spread[cell] = m ? (float)__dadd_rn((double)key2f(hi), -(double)key2f(lo)) : nodata;
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT size_t smvs_dsm_dist_workspace_bytes(int gw, int gh, int max_dist)
{
    using namespace smvs;
    if (grid_check(gw, gh) || max_dist < 1 || max_dist > DIST_MAX) return 0;
    return align256((size_t)gw * gh * sizeof(unsigned short));
}

SMVS_EXPORT int smvs_dsm_dist(const unsigned char* mask, int gw, int gh, int border, int max_dist, int* d2,
                              void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!mask || !d2 || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (border != 0 && border != 1) return fail(SMVS_ERR_ARG, "border must be 0 or 1, got %d", border);
    if (max_dist < 1 || max_dist > DIST_MAX) return fail(SMVS_ERR_ARG, "max_dist must be in 1 .. %d, got %d", DIST_MAX, max_dist);
    const size_t ncells = (size_t)gw * gh;
    if (dsm_overlap(mask, ncells, d2, ncells * 4)) return fail(SMVS_ERR_ARG, "d2 aliases mask");
    const size_t need = smvs_dsm_dist_workspace_bytes(gw, gh, max_dist);
    if (workspace_bytes < need) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    if (dsm_overlap(mask, ncells, workspace, need) || dsm_overlap(d2, ncells * 4, workspace, need))
        return fail(SMVS_ERR_ARG, "workspace aliases mask or d2");
    hipStream_t s = (hipStream_t)stream;
    unsigned short* g = (unsigned short*)workspace;
    const int band = dist_band(max_dist);
    const unsigned nbx = (unsigned)((gw + DIST_THREADS - 1) / DIST_THREADS), nbands = (unsigned)((gh + band - 1) / band);
    hipLaunchKernelGGL(dsm_dist_cols, dim3(nbx * nbands), dim3(DIST_THREADS), 0, s, mask, gw, gh, border, max_dist, band, nbx, g);
    if (int rc = check_launch("dsm_dist_cols")) return rc;
    const unsigned nseg = (unsigned)((gw + DIST_ROW_SEG - 1) / DIST_ROW_SEG);
    hipLaunchKernelGGL(dsm_dist_rows, dim3(nseg * (unsigned)gh), dim3(DIST_THREADS), 0, s, g, gw, border, max_dist, nseg, d2);
    return check_launch("dsm_dist_rows");
}

SMVS_EXPORT int smvs_dsm_mosaic(const smvs_dsm_layer* layers, int n_layers, float nodata, int mode, int feather,
                                int gw, int gh, float* out, unsigned char* count, unsigned char* source, float* spread, void* stream)
{
    using namespace smvs;
    if (!layers || !out) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (n_layers < 1 || n_layers > MOSAIC_MAX_LAYERS) return fail(SMVS_ERR_ARG, "n_layers must be in 1 .. %d, got %d", MOSAIC_MAX_LAYERS, n_layers);
    if (mode < 0 || mode > 5) return fail(SMVS_ERR_ARG, "mode must be 0 (first), 1 (last), 2 (min), 3 (max), 4 (mean) or 5 (feather), got %d", mode);
    if (mode == MOSAIC_FEATHER && (feather < 1 || feather > DIST_MAX)) return fail(SMVS_ERR_ARG, "feather must be in 1 .. %d, got %d", DIST_MAX, feather);
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "destination: %s", msg);
    const size_t ncells = (size_t)gw * gh;
    const void* outs[4] = {out, count, source, spread};
    const size_t out_bytes[4] = {ncells * 4, ncells, ncells, ncells * 4};
    static const char* const out_names[4] = {"out", "count", "source", "spread"};
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (outs[i] && outs[j] && dsm_overlap(outs[i], out_bytes[i], outs[j], out_bytes[j]))
                return fail(SMVS_ERR_ARG, "%s aliases %s", out_names[j], out_names[i]);
    MosaicTable t = {};
    for (int k = 0; k < n_layers; ++k) {
        const smvs_dsm_layer& L = layers[k];
        if (!L.z) return fail(SMVS_ERR_ARG, "layer %d: null z", k);
        if (const char* msg = grid_check(L.gw, L.gh)) return fail(SMVS_ERR_ARG, "layer %d: %s", k, msg);
        if (L.ox <= -(1 << 30) || L.ox >= (1 << 30) || L.oy <= -(1 << 30) || L.oy >= (1 << 30))
            return fail(SMVS_ERR_ARG, "layer %d: offset out of range: |ox|, |oy| must be below 2^30, got %d, %d", k, L.ox, L.oy);
        if (mode == MOSAIC_FEATHER && !L.d2) return fail(SMVS_ERR_ARG, "layer %d: feather mode needs d2", k);
        const size_t nl = (size_t)L.gw * L.gh * 4;
        for (int i = 0; i < 4; ++i)
            if (outs[i] && (dsm_overlap(outs[i], out_bytes[i], L.z, nl) || (L.d2 && dsm_overlap(outs[i], out_bytes[i], L.d2, nl))))
                return fail(SMVS_ERR_ARG, "%s aliases a buffer of layer %d", out_names[i], k);
        t.layer[k] = L;
    }
    const unsigned cells = (unsigned)ncells;
    hipLaunchKernelGGL(dsm_mosaic, dim3((cells + MOSAIC_THREADS - 1u) / MOSAIC_THREADS), dim3(MOSAIC_THREADS), 0, (hipStream_t)stream,
                       t, n_layers, nodata, mode, mode == MOSAIC_FEATHER ? feather * feather : 1, gw, cells, out, count, source, spread);
    return check_launch("dsm_mosaic");
}

}  // extern "C"
