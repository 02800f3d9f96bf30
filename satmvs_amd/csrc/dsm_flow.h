// dsm_flow.h -- the forest of a D8 direction grid, which dsm_hydro.hip (accumulation, basins) and dsm_stream.hip (stream
// networks) share: the neighbour tables, the receiver of a cell, and the root of every cell by pointer doubling.  Every kernel
// is static, as in dsm_scan.h: each source that includes this header has its own copy.  dsm_cost.hip takes the neighbour tables
// alone: its back-links are codes in this numbering, so the forest below is what reads them.
//
// recv[c] is the cell c drains into, D8_ROOT or D8_INVALID.  up[c] starts as recv[c] (a root as itself) and is squared
// ceil(log2(cells)) + 1 times IN PLACE: a lane that reads a word another lane has squared already only jumps further along the
// same path, so after the fixed number of rounds up[c] is the root of every cell that has one, and a cell whose up[c] is not a
// root is on a cycle or drains into one, whatever the order of the lanes.
#pragma once
#include "dsm_common.h"

namespace smvs {

constexpr int D8_THREADS = 256;
constexpr int D8_ROOT = -1, D8_INVALID = -2;

// Neighbour k = 0 .. 7 is E, SE, S, SW, W, NW, N, NE (include/satmvs.h, "Hydrology"), columns east and rows south: dc = 1, 1, 0,
// -1, -1, -1, 0, 1 and dr = 0, 1, 1, 1, 0, -1, -1, -1, two bits each (+ 1) in one word, so that a direction read from memory
// indexes no table.
__host__ __device__ constexpr int d8_dc(int k) { return (int)((0x901au >> (2 * k)) & 3u) - 1; }
__host__ __device__ constexpr int d8_dr(int k) { return (int)((0x01a9u >> (2 * k)) & 3u) - 1; }
static_assert(d8_dc(0) == 1 && d8_dc(1) == 1 && d8_dc(2) == 0 && d8_dc(3) == -1 && d8_dc(4) == -1 && d8_dc(5) == -1 && d8_dc(6) == 0 && d8_dc(7) == 1, "dc");
static_assert(d8_dr(0) == 0 && d8_dr(1) == 1 && d8_dr(2) == 1 && d8_dr(3) == 1 && d8_dr(4) == 0 && d8_dr(5) == -1 && d8_dr(6) == -1 && d8_dr(7) == -1, "dr");

// The cell a code sends cell (r, c) to; D8_ROOT for code 0 and for a target off the grid or without a code; D8_INVALID for 9 ..
// 255.  With a pour mask (it may be null) a marked cell that has a code is a root.
__device__ __forceinline__ int d8_receiver(const unsigned char* __restrict__ dir, const unsigned char* __restrict__ pour,
                                           int gw, int gh, int r, int c)
{
    const size_t i = (size_t)r * gw + c;
    const unsigned code = dir[i];
    if (code > 8) return D8_INVALID;
    if (code == 0 || (pour && pour[i])) return D8_ROOT;
    const int rr = r + d8_dr(code - 1), cc = c + d8_dc(code - 1);
    if (rr < 0 || rr >= gh || cc < 0 || cc >= gw) return D8_ROOT;
    const size_t t = (size_t)rr * gw + cc;
    return dir[t] > 8 ? D8_ROOT : (int)t;
}

static __global__ __launch_bounds__(D8_THREADS)
void d8_receivers(const unsigned char* __restrict__ dir, const unsigned char* __restrict__ pour, int gw, int gh,
                  int* __restrict__ recv, int* __restrict__ up)
{
    const unsigned n = (unsigned)gw * (unsigned)gh, i = blockIdx.x * (unsigned)D8_THREADS + threadIdx.x;
    if (i >= n) return;
    const int to = d8_receiver(dir, pour, gw, gh, (int)(i / (unsigned)gw), (int)(i % (unsigned)gw));
    recv[i] = to;
    up[i] = to >= 0 ? to : (int)i;
}

// up <- up o up, in place (the header comment says why that is sound).  Every word is a cell index written by d8_receivers.
static __global__ __launch_bounds__(D8_THREADS)
void d8_jump(unsigned n, int* up)
{
    const unsigned i = blockIdx.x * (unsigned)D8_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned a = (unsigned)up[i];
    if (a >= n) return;
    const unsigned b = (unsigned)up[a];
    if (b < n && b != a) up[i] = (int)b;
}

// Cell indices and twice the cells (the elements of an Euler tour) stay int32.
static const char* d8_grid_check(int gw, int gh)
{
    if (gw < 1 || gh < 1) return "non-positive grid size";
    if ((long long)gw * gh >= (1ll << 30)) return "grid too large: gw * gh must be below 2^30 cells";
    return nullptr;
}

// recv and up of a direction grid (and a pour mask, or null), then the roots: receivers, then ceil(log2 n) + 1 jumps.
static int d8_roots(const unsigned char* dir, const unsigned char* pour, int gw, int gh, int* recv, int* up, hipStream_t s)
{
    const size_t n = (size_t)gw * gh;
    DSM_LAUNCH(d8_receivers, n, D8_THREADS, s, dir, pour, gw, gh, recv, up);
    for (int k = 0, rounds = dsm_ceil_log2(n) + 1; k < rounds; ++k) DSM_LAUNCH(d8_jump, n, D8_THREADS, s, (unsigned)n, up);
    return SMVS_OK;
}

}  // namespace smvs
