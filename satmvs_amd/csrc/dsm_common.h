// dsm_common.h -- what the DSM sources (dsm.hip, dsm_render.hip, dsm_post.hip, dsm_morph.hip, dsm_label.hip, dsm_coreg.hip,
// dsm_mosaic.hip, dsm_sun.hip, dsm_horizon.hip, dsm_viewshed.hip, dsm_outline.hip, dsm_contour.hip, dsm_hydro.hip, dsm_stream.hip) share: the validity test of a cell, the order-preserving uint32 image of a float, the register sorting
// network, and the host-side grid-size and aliasing checks.
#pragma once
#include <math.h>
#include <stdint.h>

#include "smvs_host.h"

namespace smvs {

// A cell holds a height iff it is finite and differs from (float)nodata (a NaN nodata leaves finiteness alone).
__device__ __forceinline__ bool dsm_cell_valid(float z, float nodata) { return isfinite(z) && z != nodata; }

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

static const char* grid_check(int gw, int gh)
{
    if (gw < 1 || gh < 1) return "non-positive grid size";
    if ((long long)gw * gh >= (1ll << 31)) return "grid too large: gw * gh must be below 2^31 cells";
    return nullptr;
}

}  // namespace smvs
