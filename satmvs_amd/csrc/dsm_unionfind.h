// dsm_unionfind.h -- the bounded find and union over a parent array of cell indices that dsm_label.hip (objects of a mask) and
// dsm_facet.hip (planar facets of a DSM) share.  parent[c] <= c at every moment, -1 at cells outside every tree.
//
// The loops are bounded by construction: a find follows parents and every step must strictly lower the index (parent < cell
// for a cell that is not its own root), so a find from cell x ends within x steps; a union lowers max(a, b) with every
// retry, so it ends within max(a, b) steps.  A step that does not lower the index (a parent above its cell, or a negative
// one) can only come from a damaged parent array: the lane stops there and sets the error word.  No loop can spin and no
// index leaves [0, cell].
#pragma once
#include "smvs_host.h"

namespace smvs {

__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int ld_lds(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// Root of a (LDS == false: across workgroups, every load at agent scope past the CU's L1).  At most a steps.
template <bool LDS>
__device__ __forceinline__ int label_find(const int* P, int a, int* err)
{
    for (;;) {
        const int p = LDS ? ld_lds(P + a) : ld_agent(P + a);
        if (p == a) return a;
        if (p < 0 || p > a) {                                // not a step down: the array is damaged
            atomicOr(err, 1);
            return a;
        }
        a = p;
    }
}

// Unite the trees of a and b: the higher root goes under the lower.  atomicMin answers what the parent was: the root itself
// = linked; anything else is lower than a, and the union goes on from there.  At most max(a, b) retries.
template <bool LDS>
__device__ __forceinline__ void label_union(int* P, int a, int b, int* err)
{
    a = label_find<LDS>(P, a, err);
    b = label_find<LDS>(P, b, err);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(P + a, b);
        if (old == a) break;
        if (old < 0 || old > a) {
            atomicOr(err, 1);
            break;
        }
        a = old;
    }
}

}  // namespace smvs
