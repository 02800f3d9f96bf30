// dsm_common.h -- what the DSM sources (dsm.hip, dsm_render.hip, dsm_post.hip, dsm_morph.hip, dsm_label.hip, dsm_coreg.hip,
// dsm_mosaic.hip, dsm_stack.hip, dsm_sun.hip, dsm_horizon.hip, dsm_viewshed.hip, dsm_outline.hip, dsm_simplify.hip, dsm_contour.hip, dsm_hydro.hip,
// dsm_stream.hip, dsm_cost.hip, dsm_watershed.hip, dsm_mesh.hip, dsm_facet.hip, dsm_zonal.hip, dsm_focal.hip, dsm_rank.hip) and the headers dsm_geo.h, dsm_chain.h and dsm_flow.h share: the validity test of a cell, the order-preserving uint32 image of a float, the register sorting
// network, the height quantum of the exact tools, and on the host the grid-size and aliasing checks, the round and block counts and
// the launch macro.
#pragma once
#include <math.h>
#include <stdint.h>

#include "smvs_host.h"

namespace smvs {

// A cell holds a height iff it is finite and differs from (float)nodata (a NaN nodata leaves finiteness alone).
__device__ __forceinline__ bool dsm_cell_valid(float z, float nodata) { return isfinite(z) && z != nodata; }

// The height of a cell in units of 2^-8 m, as the exact tools (contours, hydrology, horizon, viewshed) take it: q = rn(256 z) of
// a valid cell with |z| <= DSM_MAX_Z.  256 z is exact in a double and |q| <= 2^23, so __double2int_rn here and the
// (int)__double2ll_rn that three of the tools used to spell out give the same q.  false: no height; q is left alone (each tool
// has its own void value).
constexpr float DSM_MAX_Z = 32768.0f;

__device__ __forceinline__ bool dsm_quantum(float z, float nodata, int& q)
{
    if (!(dsm_cell_valid(z, nodata) && fabsf(z) <= DSM_MAX_Z)) return false;
    q = __double2int_rn(__dmul_rn((double)z, 256.0));
    return true;
}

__device__ __forceinline__ unsigned f2key(float f)
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float key2f(unsigned k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Bitonic sorting network over a register array, every index a compile-time constant (template recursion: a loop nest of this
// depth is not always unrolled, and one dynamic index sends the whole array to scratch).
template <int N, int SIZE, int STRIDE>
__device__ __forceinline__ void bitonic_net(unsigned (&v)[N])
{
    if constexpr (SIZE <= N) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const int p = k ^ STRIDE;
            if (p > k) {
                const unsigned a = v[k], b = v[p];
                const bool up = (k & SIZE) == 0;
                v[k] = up ? min(a, b) : max(a, b);
                v[p] = up ? max(a, b) : min(a, b);
            }
        }
        if constexpr (STRIDE > 1) bitonic_net<N, SIZE, STRIDE / 2>(v);
        else bitonic_net<N, SIZE * 2, SIZE>(v);
    }
}

static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// Whether two buffers share a byte (the out-of-place entries reject aliased arguments).
static bool dsm_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// A table of an entry's buffers, and its first pair that shares a byte: the later entry's name, the earlier one's in `other`;
// nullptr if there is none.  Entries that are null or empty are skipped.
struct DsmBuf { const void* p; size_t bytes; const char* name; };

static const char* dsm_first_alias(const DsmBuf* buf, int n_buf, const char*& other)
{
    for (int i = 1; i < n_buf; ++i)
        for (int j = 0; j < i; ++j)
            if (buf[i].p && buf[j].p && buf[i].bytes && buf[j].bytes && dsm_overlap(buf[i].p, buf[i].bytes, buf[j].p, buf[j].bytes)) {
                other = buf[j].name;
                return buf[i].name;
            }
    return nullptr;
}

static int dsm_ceil_log2(size_t n)
{
    int r = 0;
    while (((size_t)1 << r) < n) ++r;
    return r;
}

static unsigned dsm_blocks(size_t count, unsigned threads) { return (unsigned)((count + threads - 1) / threads); }

// One lane per element: `kernel` over ceil(count / threads) workgroups (count = threads * blocks where the kernel wants blocks) on
// `stream`; a launch that fails returns from the calling function with the kernel's name in the message.  A templated kernel's
// name goes in parentheses.
#define DSM_LAUNCH(kernel, count, threads, stream, ...)                                                          \
    do {                                                                                                         \
        hipLaunchKernelGGL(kernel, dim3(smvs::dsm_blocks(count, threads)), dim3(threads), 0, stream, __VA_ARGS__); \
        if (int rc_ = smvs::check_launch(#kernel)) return rc_;                                                   \
    } while (0)

static const char* grid_check(int gw, int gh)
{
    if (gw < 1 || gh < 1) return "non-positive grid size";
    if ((long long)gw * gh >= (1ll << 31)) return "grid too large: gw * gh must be below 2^31 cells";
    return nullptr;
}

}  // namespace smvs
