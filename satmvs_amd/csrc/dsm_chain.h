// dsm_chain.h -- ordering the elements of chains that are known by their predecessors only, which dsm_outline.hip (boundary
// edges into rings) and dsm_contour.hip (crossings into open chains and rings) share: the first words of the workspace's tail,
// the windowed pointer doubling over a predecessor array, the stable sort of the chains' first elements by a small key, the
// table "first chain of key k", and the counts handed to the caller.  Every kernel is static, as in dsm_scan.h: each source that
// includes this header has its own copy.
//
// The doubling carries a 64-bit word (key << 32 | steps) per element: the lowest key of the window that ends at the element,
// and how many elements back it stands.  A round joins the window of an element with the window of the element `add` places
// back, so after ceil(log2(n)) rounds the window of an element of a ring is the whole ring, and the window of an element of an
// open chain (whose first element has the predecessor CH_NONE) reaches the chain's start.
#pragma once
#include "dsm_common.h"
#include "dsm_scan.h"

namespace smvs {

typedef unsigned long long u64;

// The first words of the tail: the elements, the chains, the vertices, the error word, the total of the scan that ran last.
enum { CH_N = 0, CH_LINES = 1, CH_VERTICES = 2, CH_ERR = 3, CH_TOTAL = 4 };
constexpr unsigned CH_NONE = 0xffffffffu;                    // no predecessor: the start of an open chain

// One round of the doubling.  Limit()(tail, cap) is the number of elements the kernels past the count work on (each source has
// its own rule for more elements than room).  Without SENTINEL every element has a predecessor and no word is compared with
// CH_NONE.  An index that is out of range (a damaged workspace) sets the error word, and the lane goes on as the start of an
// open chain (SENTINEL) or with its own index.  Where the element's own word is read differs on purpose: at once with
// SENTINEL, where the start of an open chain needs nothing else, and with the predecessor's word without; on a 2199 x 2158
// grid either kernel lost 1 % (rings) to 10 % (open chains) of the whole count with the other's order.
template <bool SENTINEL, class Limit>
static __global__ __launch_bounds__(OL_THREADS)
void chain_double(const unsigned* __restrict__ pin, const u64* __restrict__ vin, unsigned* __restrict__ pout, u64* __restrict__ vout,
                  unsigned add, unsigned cap, int* tail)
{
    const unsigned j = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    const unsigned n = (unsigned)Limit()(tail, cap);
    if (j >= n) return;
    unsigned p = pin[j], q;
    u64 a;
    if constexpr (SENTINEL) {
        a = vin[j];
        if (p != CH_NONE && p >= n) { atomicOr(tail + CH_ERR, 1); p = CH_NONE; }
        if (p == CH_NONE) {
            vout[j] = a;
            pout[j] = CH_NONE;
            return;
        }
        q = pin[p];
        if (q != CH_NONE && q >= n) { atomicOr(tail + CH_ERR, 1); q = CH_NONE; }
    } else {
        if (p >= n) { atomicOr(tail + CH_ERR, 1); p = j; }
        q = pin[p];
        if (q >= n) { atomicOr(tail + CH_ERR, 1); q = j; }
        a = vin[j];
    }
    const u64 b = vin[p] + add;
    vout[j] = a < b ? a : b;
    pout[j] = q;
}

static int chain_rounds(unsigned cap)
{
    int rounds = 0;
    while (rounds < 31 && (1u << rounds) < cap) ++rounds;
    return rounds;
}

// All rounds for room of cap elements: (pred[0], val[0]) -> (pred[1], val[1]) -> (pred[2], val[0]) -> (pred[1], val[1]) ..., so
// pred[0] stays what the links were.  *result <- which val holds the words after the last round: chain_rounds(cap) % 2.
template <bool SENTINEL, class Limit>
static int chain_order(unsigned* const pred[3], u64* const val[2], unsigned cap, int* tail, hipStream_t s, int* result)
{
    const int rounds = chain_rounds(cap);
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL((chain_double<SENTINEL, Limit>), dim3(dsm_blocks(cap, OL_THREADS)), dim3(OL_THREADS), 0, s,
                           (const unsigned*)pred[r == 0 ? 0 : 1 + (r + 1) % 2], (const u64*)val[r % 2], pred[1 + r % 2], val[(r + 1) % 2],
                           1u << r, cap, tail);
        if (int rc = check_launch("chain_double")) return rc;
    }
    *result = rounds % 2;
    return SMVS_OK;
}

// ---- the stable sort of (key, value) pairs by key, one split per bit ---------------------------------------------------------
static __global__ __launch_bounds__(OL_THREADS)
void chain_sort_flag(const int* __restrict__ skey, int* __restrict__ spos, unsigned n, int bit)
{
    const unsigned i = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    if (i < n) spos[i] = !(((unsigned)skey[i] >> bit) & 1u);
}

// The stable split on one bit: the keys without the bit keep their order in front, the others theirs behind.
static __global__ __launch_bounds__(OL_THREADS)
void chain_sort_scatter(const int* __restrict__ kin, const int* __restrict__ vin, const int* __restrict__ spos, int* tail,
                        int* __restrict__ kout, int* __restrict__ vout, unsigned n, int bit)
{
    const unsigned i = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    if (i >= n) return;
    const int k = kin[i];
    const unsigned before = (unsigned)spos[i], zeros = (unsigned)tail[CH_TOTAL];
    unsigned d = (((unsigned)k >> bit) & 1u) ? zeros + (i - before) : before;
    if (d >= n) { atomicOr(tail + CH_ERR, 1); d = i; }
    kout[d] = k;
    vout[d] = vin[i];
}

// The n pairs of (skey[0], sval[0]) sorted by the low `bits` bits of the key, equal keys in the order they came in; *result <-
// which of the two buffers holds them: bits % 2.
static int chain_sort(int* const skey[2], int* const sval[2], int* spos, unsigned n, int bits, int* s1, int* s2, int* tail,
                      hipStream_t s, int* result)
{
    for (int b = 0; b < bits; ++b) {
        DSM_LAUNCH(chain_sort_flag, n, OL_THREADS, s, (const int*)skey[b % 2], spos, n, b);
        if (int rc = ol_scan_exclusive(spos, n, nullptr, s1, s2, tail + CH_TOTAL, s, "ol_scan (sort)")) return rc;
        DSM_LAUNCH(chain_sort_scatter, n, OL_THREADS, s, (const int*)skey[b % 2], (const int*)sval[b % 2], (const int*)spos, tail,
                   skey[(b + 1) % 2], sval[(b + 1) % 2], n, b);
    }
    *result = bits % 2;
    return SMVS_OK;
}

// first[k], k = 0 .. n_keys: the first of the n chains, sorted by key, whose key is key0 + k or above; n if there is none.
static __global__ __launch_bounds__(OL_THREADS)
void chain_first(const int* __restrict__ skey, unsigned n, int n_keys, unsigned key0, int* __restrict__ first)
{
    const unsigned k = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    if (k > (unsigned)n_keys) return;
    unsigned lo = 0, hi = n;
    for (int step = 0; step < 32 && lo < hi; ++step) {
        const unsigned mid = lo + (hi - lo) / 2;
        if ((unsigned)skey[mid] < key0 + k) lo = mid + 1;
        else hi = mid;
    }
    first[k] = (int)lo;
}

// The three counts to the caller, -1 each if the error word is set.
static __global__ void chain_counts_out(const int* __restrict__ tail, int* __restrict__ counts)
{
    if (threadIdx.x < 3) counts[threadIdx.x] = tail[CH_ERR] ? -1 : tail[threadIdx.x];
}

}  // namespace smvs
