// sgm.hip -- heights without a network ("Census plane sweep and SGM"; include/satmvs.h for the rules).
//
//   smvs_sgm_census_cost   census matching cost of a chunk of planes from the warped [image, coverage] volumes of the sources
//   smvs_sgm_aggregate     4 or 8 path semi-global aggregation of a (B, H, W, D) uint16 cost volume
//   smvs_sgm_select        winner, uniqueness test, support and the sub-plane height
//
// Census: a workgroup is an 8 x 32 tile of pixels and a group of 8 planes.  Per (plane, source) the tile with its halo goes into
// LDS as pairs (image, covered); a lane is a pixel, reads its window from LDS, and keeps the 8 costs of its group to write them
// as one 16-byte store where the volume's layout allows it.  The census of ref comes from the workspace, written once per call.
// Aggregation: one launch per direction, one wave per line of that direction, the planes across the lanes in blocks of
// K = ceil(D / 64) (so all d +- 1 neighbours but two stay in the lane), the previous L in registers.  A step is a two-lane
// exchange (DPP wave shifts), a few integer min / add and a wave-wide minimum (a DPP scan and one read of lane 63); the cost,
// sum and guide loads of the next SG_AHEAD steps are issued before the chain of the current ones, since they do not depend on
// it.  The first direction stores sum, the others add to it: no atomics, and no two directions in one launch.
// Select: a lane per pixel, two passes over its D sums.
#include <math.h>
#include <stdint.h>

#include "dsm_common.h"
#include "smvs_host.h"

namespace smvs {

constexpr int SG_MAX_D = 256;
constexpr int SG_MAX_SRC = 7;
constexpr int SG_VOID = 0xFFFF;
constexpr int SG_TILE_H = 8, SG_TILE_W = 32;             // the census tile: 256 lanes, lanes along W
constexpr int SG_THREADS = SG_TILE_H * SG_TILE_W;
constexpr int SG_GROUP = 8;                              // planes of one census workgroup: 8 uint16 = one 16-byte store
constexpr int SG_MAX_R = 3;
constexpr int SG_AHEAD = 4;                              // steps whose loads are in flight ahead of the aggregation chain
constexpr int SG_BIG = 0x3fffffff;                       // L of a plane that does not exist: + P1 and + P2 stay in an int

struct SgSources { const float* p[SG_MAX_SRC]; };
struct SgTap { float v; unsigned ok; };                  // one LDS entry: the warped image and whether the voxel is covered (off the grid: NaN, 1)

// ---- census --------------------------------------------------------------------------------------------------------------------
// The bits of the window of `at` in row-major order of (dy, dx), the centre left out; `covered`: the AND of the ok fields.
template <int R, class At>
__device__ __forceinline__ unsigned long long sg_census(const At& at, float centre, unsigned& covered)
{
    unsigned long long bits = 0;
    unsigned ok = 1;
    int k = 0;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy)
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
            if (dy == 0 && dx == 0) continue;
            const SgTap t = at(dy, dx);
            bits |= (unsigned long long)(t.v < centre ? 1 : 0) << k;
            ok &= t.ok;
            ++k;
        }
    covered = ok;
    return bits;
}

template <int R>
__global__ __launch_bounds__(SG_THREADS)
void sgm_census_ref(const float* __restrict__ ref, int H, int W, unsigned pixels, unsigned long long* __restrict__ census)
{
    const unsigned p = blockIdx.x * SG_THREADS + threadIdx.x;
    if (p >= pixels) return;
    const int x = (int)(p % (unsigned)W), y = (int)((p / (unsigned)W) % (unsigned)H);
    const float* img = ref + (size_t)(p - (unsigned)(y * W + x));
    const auto at = [&](int dy, int dx) {
        const int yy = y + dy, xx = x + dx;
        const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
        return SgTap{in ? img[yy * W + xx] : NAN, 1u};
    };
    unsigned covered;
    census[p] = sg_census<R>(at, img[y * W + x], covered);
}

// blockIdx.x = (b * tiles_y + tile row) * tiles_x + tile column; blockIdx.y = the group of SG_GROUP planes of the chunk.
template <int R>
__global__ __launch_bounds__(SG_THREADS)
void sgm_census_cost(const unsigned long long* __restrict__ census, const SgSources src, int n_src, float cov_min,
                     unsigned short* __restrict__ cost, int H, int W, int d_begin, int Dc, int D, unsigned tiles_x, unsigned tiles_y, int wide)
{
    constexpr int TH = SG_TILE_H + 2 * R, TW = SG_TILE_W + 2 * R;
    __shared__ SgTap tile[TH * TW];
    const unsigned tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, b = blockIdx.x / (tiles_x * tiles_y);
    const int x0 = (int)tx * SG_TILE_W, y0 = (int)ty * SG_TILE_H;
    const int lx = (int)threadIdx.x % SG_TILE_W, ly = (int)threadIdx.x / SG_TILE_W;
    const int x = x0 + lx, y = y0 + ly;
    const bool mine = x < W && y < H;
    const size_t plane = (size_t)H * W;
    const size_t pixel = (size_t)b * plane + (size_t)(mine ? y * W + x : 0);
    const unsigned long long cref = mine ? census[pixel] : 0ull;
    const int g0 = (int)blockIdx.y * SG_GROUP;            // first plane of the group, within the chunk
    unsigned res[SG_GROUP];
#pragma unroll
    for (int j = 0; j < SG_GROUP; ++j) {
        res[j] = SG_VOID;
        if (g0 + j >= Dc) continue;                       // uniform over the workgroup
        int ham = 0, n = 0;
        for (int s = 0; s < n_src; ++s) {
            const float* img = src.p[s] + ((size_t)b * 2 * Dc + (size_t)(g0 + j)) * plane;
            const float* cov = img + (size_t)Dc * plane;
            __syncthreads();                              // the previous window reads are done
            for (int e = (int)threadIdx.x; e < TH * TW; e += SG_THREADS) {
                const int yy = y0 - R + e / TW, xx = x0 - R + e % TW;
                SgTap t{NAN, 1u};
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                    t.v = img[yy * W + xx];
                    t.ok = cov[yy * W + xx] >= cov_min ? 1u : 0u;
                }
                tile[e] = t;
            }
            __syncthreads();
            const SgTap* c = tile + (ly + R) * TW + lx + R;
            const auto at = [&](int dy, int dx) { return c[dy * TW + dx]; };
            unsigned covered;
            const unsigned long long bits = sg_census<R>(at, c->v, covered);
            if (covered & c->ok) {
                ham += __popcll(bits ^ cref);
                ++n;
            }
        }
        if (n > 0) res[j] = (unsigned)(16 * ham) / (unsigned)n;
    }
    if (!mine) return;
    unsigned short* out = cost + pixel * (size_t)D + (size_t)(d_begin + g0);
    if (wide && (d_begin + g0) % SG_GROUP == 0 && g0 + SG_GROUP <= Dc) {                  // wide: D % 8 == 0 and cost is 16-byte aligned
        uint4 v;
        v.x = res[0] | res[1] << 16; v.y = res[2] | res[3] << 16; v.z = res[4] | res[5] << 16; v.w = res[6] | res[7] << 16;
        *reinterpret_cast<uint4*>(out) = v;
    } else {
#pragma unroll
        for (int j = 0; j < SG_GROUP; ++j)
            if (g0 + j < Dc) out[j] = (unsigned short)res[j];
    }
}

// ---- aggregation ---------------------------------------------------------------------------------------------------------------
struct SgPen { int P1, P2, p2_min, alpha, cost_max, void_cost; };

// lane i <- lane i - 1 (lane 0 <- SG_BIG) and lane i <- lane i + 1 (lane 63 <- SG_BIG): the DPP wave shifts of GFX9
__device__ __forceinline__ int sg_from_below(int v) { return __builtin_amdgcn_update_dpp(SG_BIG, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ int sg_from_above(int v) { return __builtin_amdgcn_update_dpp(SG_BIG, v, 0x130, 0xf, 0xf, false); }

// The minimum over the 64 lanes, in every lane: an inclusive DPP scan (row_shr 1, 2, 4, 8, row_bcast 15 and 31) whose last lane
// holds the whole wave's; lanes that a step does not write keep the identity.
__device__ __forceinline__ int sg_wave_min(int v)
{
    v = min(v, __builtin_amdgcn_update_dpp(SG_BIG, v, 0x111, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(SG_BIG, v, 0x112, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(SG_BIG, v, 0x114, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(SG_BIG, v, 0x118, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(SG_BIG, v, 0x142, 0xa, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(SG_BIG, v, 0x143, 0xc, 0xf, false));
    return __builtin_amdgcn_readlane(v, 63);
}

// What a step reads from memory: K costs, K sums (not in the first direction) and the guide byte of its pixel.
template <int K> struct SgLoad { int c[K], s[K], g; };

// One wave per (batch, line) of direction (ry, rx); lines: rows (ry = 0), columns (rx = 0), or the W + H - 1 diagonals that start
// on the first row met and on the side column.  No lane leaves before the end: the DPP steps read all 64.
template <int K, bool FIRST, bool GUIDE>
__global__ __launch_bounds__(256)
void sgm_path(const unsigned short* __restrict__ cost, const unsigned char* __restrict__ guide, unsigned short* __restrict__ sum,
              int B, int H, int W, int D, int ry, int rx, int n_lines, const SgPen pen)
{
    const int wave = (int)blockIdx.x * 4 + (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
    if (wave >= B * n_lines) return;                      // uniform over the wave
    const int b = wave / n_lines, l = wave % n_lines;
    int y, x, n;
    if (ry == 0) { y = l; x = rx > 0 ? 0 : W - 1; n = W; }
    else if (rx == 0) { x = l; y = ry > 0 ? 0 : H - 1; n = H; }
    else {
        if (l < W) { y = ry > 0 ? 0 : H - 1; x = l; }
        else { y = ry > 0 ? l - W + 1 : H - 2 - (l - W); x = rx > 0 ? 0 : W - 1; }
        n = min(ry > 0 ? H - y : y + 1, rx > 0 ? W - x : x + 1);
    }
    const long long pix0 = ((long long)b * H + y) * W + x, step = (long long)ry * W + rx;
    const int d0 = lane * K;

    const auto load = [&](int i, SgLoad<K>& v) {
        if (i >= n) return;
        const long long pix = pix0 + i * step;
        const size_t at = (size_t)pix * (size_t)D + (size_t)d0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            v.c[k] = d0 + k < D ? (int)cost[at + k] : 0;
            if (!FIRST) v.s[k] = d0 + k < D ? (int)sum[at + k] : 0;
        }
        if (GUIDE) v.g = (int)guide[pix];
    };

    int prev[K], m = 0, g_prev = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) prev[k] = SG_BIG;
    const auto advance = [&](int i, const SgLoad<K>& v) {
        if (i >= n) return;
        int cur[K];
        int p2 = pen.P2;
        if (GUIDE) {
            const int dg = v.g - g_prev;
            p2 = max(pen.p2_min, pen.P2 - pen.alpha * (dg < 0 ? -dg : dg));
        }
        const int below = sg_from_below(prev[K - 1]), above = sg_from_above(prev[0]);
        const int jump = m + p2;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int c = v.c[k] == SG_VOID ? pen.void_cost : min(v.c[k], pen.cost_max);
            const int lo = k > 0 ? prev[k - 1] : below, hi = k < K - 1 ? prev[k + 1] : above;
            const int best = min(min(prev[k], min(lo, hi) + pen.P1), jump);
            const int L = i == 0 ? c : c + best - m;
            cur[k] = d0 + k < D ? L : SG_BIG;
        }
        int least = cur[0];
#pragma unroll
        for (int k = 1; k < K; ++k) least = min(least, cur[k]);
        m = sg_wave_min(least);
        const size_t at = (size_t)(pix0 + i * step) * (size_t)D + (size_t)d0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (d0 + k < D) sum[at + k] = (unsigned short)(FIRST ? cur[k] : v.s[k] + cur[k]);
            prev[k] = cur[k];
        }
        if (GUIDE) g_prev = v.g;
    };

    SgLoad<K> now[SG_AHEAD], next[SG_AHEAD];
#pragma unroll
    for (int u = 0; u < SG_AHEAD; ++u) load(u, now[u]);
    for (int base = 0; base < n; base += SG_AHEAD) {
#pragma unroll
        for (int u = 0; u < SG_AHEAD; ++u) load(base + SG_AHEAD + u, next[u]);
#pragma unroll
        for (int u = 0; u < SG_AHEAD; ++u) advance(base + u, now[u]);
#pragma unroll
        for (int u = 0; u < SG_AHEAD; ++u) now[u] = next[u];
    }
}

// ---- select --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void sgm_select(const unsigned short* __restrict__ sum, const unsigned short* __restrict__ cost, const float* __restrict__ depth,
                int is4d, int uniq, int min_support, int* __restrict__ index, float* __restrict__ height,
                unsigned short* __restrict__ min_sum, unsigned short* __restrict__ support, unsigned pixels, unsigned plane, int D)
{
    const unsigned p = blockIdx.x * 256 + threadIdx.x;
    if (p >= pixels) return;
    const unsigned short* s = sum + (size_t)p * D;
    int best = s[0], d0 = 0;
    for (int d = 1; d < D; ++d) {
        const int v = s[d];
        if (v < best) { best = v; d0 = d; }
    }
    bool keep = true;
    const int bar = best * 100, w = 100 - uniq;
    for (int d = 0; d < D; ++d)
        if ((d < d0 - 1 || d > d0 + 1) && (int)s[d] * w < bar) keep = false;
    if (cost) {
        const unsigned short* c = cost + (size_t)p * D;
        int n = 0;
        for (int d = 0; d < D; ++d) n += c[d] != SG_VOID ? 1 : 0;
        if (support) support[p] = (unsigned short)n;
        if (n < min_support) keep = false;
    }
    if (min_sum) min_sum[p] = (unsigned short)best;
    float h = __int_as_float(0x7fc00000);
    if (keep) {
        const unsigned b = p / plane, at = p % plane;
        const auto z = [&](int d) {
            return (double)(is4d ? depth[((size_t)b * D + d) * plane + at] : depth[(size_t)b * D + d]);
        };
        const double h0 = z(d0);
        double t = 0.0;
        int den = 0;
        if (d0 > 0 && d0 < D - 1) den = (int)s[d0 - 1] + (int)s[d0 + 1] - 2 * best;
        if (den != 0) t = __ddiv_rn((double)((int)s[d0 - 1] - (int)s[d0 + 1]), (double)(2 * den));
        double v = h0;
        if (den != 0) {
            const double span = t >= 0.0 ? __dsub_rn(z(d0 + 1), h0) : __dsub_rn(h0, z(d0 - 1));
            v = __dadd_rn(h0, __dmul_rn(t, span));
        }
        h = __double2float_rn(v);
        if (h != h) h = __int_as_float(0x7fc00000);
    }
    index[p] = keep ? d0 : -1;
    height[p] = h;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// The limits all three entries put on the sizes; a message, or null.
static const char* sg_sizes_check(int B, int H, int W, int D, char* buf, size_t len)
{
    if (B < 1 || H < 1 || W < 1) {
        snprintf(buf, len, "B, H and W must be >= 1, got (%d, %d, %d)", B, H, W);
        return buf;
    }
    if (D < 1 || D > SG_MAX_D) {
        snprintf(buf, len, "D must be 1 .. %d, got %d", SG_MAX_D, D);
        return buf;
    }
    if ((double)B * H * W * D >= 2147483648.0) return "volume too large: B H W D must be below 2^31";
    return nullptr;
}

template <int K, bool FIRST>
static void sg_launch_path(bool guided, dim3 blocks, hipStream_t st, const unsigned short* cost, const unsigned char* guide,
                           unsigned short* sum, int B, int H, int W, int D, int ry, int rx, int n_lines, const SgPen& pen)
{
    if (guided) hipLaunchKernelGGL((sgm_path<K, FIRST, true>), blocks, dim3(256), 0, st, cost, guide, sum, B, H, W, D, ry, rx, n_lines, pen);
    else hipLaunchKernelGGL((sgm_path<K, FIRST, false>), blocks, dim3(256), 0, st, cost, guide, sum, B, H, W, D, ry, rx, n_lines, pen);
}

template <int K>
static void sg_launch_dir(bool first, bool guided, dim3 blocks, hipStream_t st, const unsigned short* cost, const unsigned char* guide,
                          unsigned short* sum, int B, int H, int W, int D, int ry, int rx, int n_lines, const SgPen& pen)
{
    if (first) sg_launch_path<K, true>(guided, blocks, st, cost, guide, sum, B, H, W, D, ry, rx, n_lines, pen);
    else sg_launch_path<K, false>(guided, blocks, st, cost, guide, sum, B, H, W, D, ry, rx, n_lines, pen);
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT size_t smvs_sgm_census_workspace_bytes(int B, int H, int W)
{
    using namespace smvs;
    if (B < 1 || H < 1 || W < 1 || (double)B * H * W >= 2147483648.0) return 0;
    return align256((size_t)B * H * W * 8);
}

SMVS_EXPORT int smvs_sgm_census_cost(const float* ref, const float* const* warped, int n_src, int radius, float cov_min,
                                     unsigned short* cost, int B, int H, int W, int d_begin, int Dc, int D,
                                     void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    char buf[160];
    if (!ref || !warped || !cost || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (n_src < 1 || n_src > SG_MAX_SRC) return fail(SMVS_ERR_ARG, "n_src must be 1 .. %d, got %d", SG_MAX_SRC, n_src);
    if (radius < 1 || radius > SG_MAX_R) return fail(SMVS_ERR_ARG, "radius must be 1, 2 or 3, got %d", radius);
    if (cov_min != cov_min) return fail(SMVS_ERR_ARG, "cov_min must not be NaN");
    if (const char* msg = sg_sizes_check(B, H, W, D, buf, sizeof buf)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (d_begin < 0 || Dc < 1 || d_begin > D - Dc)
        return fail(SMVS_ERR_ARG, "planes %d .. %d + %d - 1 do not lie in 0 .. %d", d_begin, d_begin, Dc, D - 1);
    const size_t pixels = (size_t)B * H * W, need = align256(pixels * 8), vol = pixels * 2 * (size_t)Dc * 4;
    if (workspace_bytes < need) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    DsmBuf bufs[3 + SG_MAX_SRC] = {{ref, pixels * 4, "ref"}, {cost, pixels * (size_t)D * 2, "cost"}, {workspace, need, "workspace"}};
    SgSources src = {};
    for (int s = 0; s < n_src; ++s) {
        if (!warped[s]) return fail(SMVS_ERR_ARG, "warped[%d] is null", s);
        src.p[s] = warped[s];
        bufs[3 + s] = DsmBuf{warped[s], vol, "a warped volume"};
    }
    const char* other = nullptr;
    if (const char* name = dsm_first_alias(bufs, 3 + n_src, other)) return fail(SMVS_ERR_ARG, "%s overlaps %s", name, other);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* census = (unsigned long long*)workspace;
    const unsigned tiles_x = (unsigned)((W + SG_TILE_W - 1) / SG_TILE_W), tiles_y = (unsigned)((H + SG_TILE_H - 1) / SG_TILE_H);
    const dim3 blocks((unsigned)B * tiles_x * tiles_y, (unsigned)((Dc + SG_GROUP - 1) / SG_GROUP));
    const int wide = D % SG_GROUP == 0 && (uintptr_t)cost % 16 == 0 ? 1 : 0;
#define SG_CENSUS(R)                                                                                                              \
    do {                                                                                                                          \
        DSM_LAUNCH((sgm_census_ref<R>), pixels, SG_THREADS, st, ref, H, W, (unsigned)pixels, census);                             \
        hipLaunchKernelGGL((sgm_census_cost<R>), blocks, dim3(SG_THREADS), 0, st, census, src, n_src, cov_min, cost, H, W,        \
                           d_begin, Dc, D, tiles_x, tiles_y, wide);                                                               \
    } while (0)
    if (radius == 1) SG_CENSUS(1);
    else if (radius == 2) SG_CENSUS(2);
    else SG_CENSUS(3);
#undef SG_CENSUS
    return check_launch("sgm_census_cost");
}

SMVS_EXPORT int smvs_sgm_aggregate(const unsigned short* cost, const unsigned char* guide, unsigned short* sum,
                                   int B, int H, int W, int D, int P1, int P2, int p2_min, int alpha, int cost_max, int void_cost,
                                   int paths, void* stream)
{
    using namespace smvs;
    char buf[160];
    if (!cost || !sum) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = sg_sizes_check(B, H, W, D, buf, sizeof buf)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (paths != 4 && paths != 8) return fail(SMVS_ERR_ARG, "paths must be 4 or 8, got %d", paths);
    if (P1 < 0 || P1 > p2_min || p2_min > P2) return fail(SMVS_ERR_ARG, "need 0 <= P1 <= p2_min <= P2, got (%d, %d, %d)", P1, p2_min, P2);
    if (alpha < 0 || alpha > 65535) return fail(SMVS_ERR_ARG, "alpha must be 0 .. 65535, got %d", alpha);
    if (void_cost < 0 || void_cost > cost_max) return fail(SMVS_ERR_ARG, "need 0 <= void_cost <= cost_max, got (%d, %d)", void_cost, cost_max);
    if ((long long)paths * ((long long)cost_max + P2) > 65535)
        return fail(SMVS_ERR_ARG, "paths (cost_max + P2) must be at most 65535, got %d (%d + %d)", paths, cost_max, P2);
    const size_t pixels = (size_t)B * H * W, cells = pixels * (size_t)D;
    const DsmBuf bufs[3] = {{cost, cells * 2, "cost"}, {guide, pixels, "guide"}, {sum, cells * 2, "sum"}};
    const char* other = nullptr;
    if (const char* name = dsm_first_alias(bufs, 3, other)) return fail(SMVS_ERR_ARG, "%s overlaps %s", name, other);
    hipStream_t st = (hipStream_t)stream;
    const SgPen pen = {P1, P2, p2_min, alpha, cost_max, void_cost};
    static const int dirs[8][2] = {{0, 1}, {0, -1}, {1, 0}, {-1, 0}, {1, 1}, {1, -1}, {-1, 1}, {-1, -1}};
    const int K = (D + 63) / 64;
    for (int r = 0; r < paths; ++r) {
        const int ry = dirs[r][0], rx = dirs[r][1];
        const int n_lines = ry == 0 ? H : rx == 0 ? W : W + H - 1;
        const dim3 blocks(dsm_blocks((size_t)B * n_lines, 4));
        const bool first = r == 0, guided = guide != nullptr;
        if (K == 1) sg_launch_dir<1>(first, guided, blocks, st, cost, guide, sum, B, H, W, D, ry, rx, n_lines, pen);
        else if (K == 2) sg_launch_dir<2>(first, guided, blocks, st, cost, guide, sum, B, H, W, D, ry, rx, n_lines, pen);
        else if (K == 3) sg_launch_dir<3>(first, guided, blocks, st, cost, guide, sum, B, H, W, D, ry, rx, n_lines, pen);
        else sg_launch_dir<4>(first, guided, blocks, st, cost, guide, sum, B, H, W, D, ry, rx, n_lines, pen);
        if (int rc = check_launch("sgm_path")) return rc;
    }
    return SMVS_OK;
}

SMVS_EXPORT int smvs_sgm_select(const unsigned short* sum, const unsigned short* cost, const float* depth, int depth_is_4d,
                                int uniqueness, int min_support, int* index, float* height, unsigned short* min_sum,
                                unsigned short* support, int B, int H, int W, int D, void* stream)
{
    using namespace smvs;
    char buf[160];
    if (!sum || !depth || !index || !height) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = sg_sizes_check(B, H, W, D, buf, sizeof buf)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (depth_is_4d != 0 && depth_is_4d != 1) return fail(SMVS_ERR_ARG, "depth_is_4d must be 0 or 1, got %d", depth_is_4d);
    if (uniqueness < 0 || uniqueness > 99) return fail(SMVS_ERR_ARG, "uniqueness must be 0 .. 99, got %d", uniqueness);
    if (min_support < 0) return fail(SMVS_ERR_ARG, "min_support must be >= 0, got %d", min_support);
    if (support && !cost) return fail(SMVS_ERR_ARG, "support needs cost");
    const size_t pixels = (size_t)B * H * W, cells = pixels * (size_t)D;
    const DsmBuf bufs[7] = {{sum, cells * 2, "sum"}, {cost, cells * 2, "cost"}, {depth, (depth_is_4d ? cells : (size_t)B * D) * 4, "depth"},
                            {index, pixels * 4, "index"}, {height, pixels * 4, "height"}, {min_sum, pixels * 2, "min_sum"},
                            {support, pixels * 2, "support"}};
    const char* other = nullptr;
    for (int i = 3; i < 7; ++i)                            // sum and cost may be one volume; an output overlaps nothing
        for (int j = 0; j < i; ++j)
            if (bufs[i].p && bufs[j].p && dsm_overlap(bufs[i].p, bufs[i].bytes, bufs[j].p, bufs[j].bytes))
                return fail(SMVS_ERR_ARG, "%s overlaps %s", bufs[i].name, bufs[j].name);
    (void)other;
    hipStream_t st = (hipStream_t)stream;
    DSM_LAUNCH(sgm_select, pixels, 256, st, sum, cost, depth, depth_is_4d, uniqueness, min_support, index, height, min_sum, support,
               (unsigned)pixels, (unsigned)((size_t)H * W), D);
    return SMVS_OK;
}

}  // extern "C"
