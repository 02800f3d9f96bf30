// dsm_scan.h -- the exclusive scan of an int array on the device that dsm_outline.hip and dsm_contour.hip (through dsm_chain.h, whose
// sort is a scan per bit), dsm_simplify.hip, dsm_hydro.hip, dsm_stream.hip and dsm_mesh.hip share: three levels of
// 2048-element blocks (256 lanes of 8 elements), so any length below 2^31.  Every kernel is static: each source that includes
// this header has its own copy.
#pragma once
#include <limits.h>

#include "smvs_host.h"

namespace smvs {

constexpr int OL_THREADS = 256, OL_PER_THREAD = 8, OL_BLOCK = OL_THREADS * OL_PER_THREAD;    // 2048 elements per workgroup of a scan

// ---- the scan ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ol_block_exclusive(int v, int& total)
{
    __shared__ int wave_sum[OL_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < OL_THREADS / 64; ++k) {
        const int s = wave_sum[k];
        if (k < wave) before += s;
        total += s;
    }
    return before + inc - v;
}

// In-place exclusive scan of the first n elements of a in blocks of 2048 (n = min(*n_dev, cap), or cap without n_dev); the
// block totals go one level up.
static __global__ __launch_bounds__(OL_THREADS)
void ol_scan(int* __restrict__ a, unsigned cap, const int* __restrict__ n_dev, int* __restrict__ sums)
{
    unsigned n = cap;
    if (n_dev) n = (unsigned)max(0, min(*n_dev, (int)min(cap, (unsigned)INT_MAX)));
    const unsigned c0 = blockIdx.x * (unsigned)OL_BLOCK + threadIdx.x * (unsigned)OL_PER_THREAD;
    int v[OL_PER_THREAD], cnt = 0;
#pragma unroll
    for (int k = 0; k < OL_PER_THREAD; ++k) {
        v[k] = (c0 < n && (unsigned)k < n - c0) ? a[c0 + k] : 0;
        cnt += v[k];
    }
    int total;
    int at = ol_block_exclusive(cnt, total);
#pragma unroll
    for (int k = 0; k < OL_PER_THREAD; ++k) {
        if (c0 < n && (unsigned)k < n - c0) a[c0 + k] = at;
        at += v[k];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

static __global__ __launch_bounds__(OL_THREADS)
void ol_scan_add(int* __restrict__ a, unsigned cap, const int* __restrict__ n_dev, const int* __restrict__ s1, const int* __restrict__ s2)
{
    unsigned n = cap;
    if (n_dev) n = (unsigned)max(0, min(*n_dev, (int)min(cap, (unsigned)INT_MAX)));
    const unsigned i = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    if (i >= n) return;
    a[i] += s1[i / OL_BLOCK] + s2[i / OL_BLOCK / OL_BLOCK];
}

// a[0 .. n) <- its exclusive prefix sums, *total <- the sum.  cap < 2^31, so the third level is one block.
static int ol_scan_exclusive(int* a, unsigned cap, const int* n_dev, int* s1, int* s2, int* total, hipStream_t s, const char* what)
{
    const unsigned nb1 = (cap + OL_BLOCK - 1) / OL_BLOCK, nb2 = (nb1 + OL_BLOCK - 1) / OL_BLOCK;
    int rc;
    hipLaunchKernelGGL(ol_scan, dim3(nb1), dim3(OL_THREADS), 0, s, a, cap, n_dev, s1);
    if ((rc = check_launch(what))) return rc;
    hipLaunchKernelGGL(ol_scan, dim3(nb2), dim3(OL_THREADS), 0, s, s1, nb1, (const int*)nullptr, s2);
    if ((rc = check_launch(what))) return rc;
    hipLaunchKernelGGL(ol_scan, dim3(1), dim3(OL_THREADS), 0, s, s2, nb2, (const int*)nullptr, total);
    if ((rc = check_launch(what))) return rc;
    hipLaunchKernelGGL(ol_scan_add, dim3((cap + OL_THREADS - 1) / OL_THREADS), dim3(OL_THREADS), 0, s, a, cap, n_dev, (const int*)s1, (const int*)s2);
    return check_launch(what);
}

}  // namespace smvs
