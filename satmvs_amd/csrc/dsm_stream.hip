// dsm_stream.hip -- the stream network of a direction grid and a stream mask, exact ("Stream network";
// include/satmvs.h for the rule): Strahler orders, links with their topology and polylines, and the flow length of every cell.
//
//   smvs_dsm_stream_order   the network pass, then the order map, the link map and the four counts
//   smvs_dsm_stream_write   the network pass AGAIN (nothing of an earlier call is read), then the per-link tables
//   smvs_dsm_flow_length    step counts to the root by one pointer doubling with sums over the forest itself
//
// The network pass, every step one lane per cell or per tour element, 256 lanes a workgroup:
//   1. receivers and roots of the whole grid (dsm_flow.h: up <- up o up in place, ceil(log2 n) + 1 rounds), so
//      that S = masked cells that reach a root; srecv = the receiver if it is in S, D8_ROOT at a mouth, D8_INVALID outside S.
//   2. the mouths numbered in row-major order by a scan and listed; the Euler tour of the induced forest (elements 2 c down and
//      2 c + 1 up, as fl_tour builds it) with the up element of a mouth leading to the down element of the next mouth: one list
//      of 2 |S| elements.  One Wyllie doubling of ceil(log2(2 n)) rounds between two copies ranks it; an element is one 64-bit
//      word (successor | suffix count << 32), so a round is one gather.  pos = 2 |S| - rank.
//   3. order rounds k = 1 .. min(30, floor(log2 n)): mark J_k (cells with two inflowing cells of order >= k) at the tour position
//      of the cell's down element, scan the marks exclusively, and promote to k + 1 every cell of order k whose span of the tour
//      holds a mark (scan[up] - scan[down] > 0: the cell or something upstream of it is in J_k).  The scan's total is the device
//      counter: after the first empty J_k the rounds that follow leave at once and scan a length of 0.  Launches stay fixed.
//   4. in(c) and heads; the heads numbered by a scan (the link numbers); (head, distance to it) per cell by doubling the pointer
//      "the one cell flowing into me" IN PLACE, ceil(log2 n) + 1 rounds.  A word is (ancestor | distance << 32) and moves as one
//      aligned 64-bit access; every word ever stored is a true (ancestor, distance) pair, so a lane that reads a word another lane
//      has advanced already only jumps further, and the fixed point (head, distance) is the same whatever the order of the lanes.
// Atomics: integer adds of wave popcounts into the counts, integer adds of 1 into a link's three step counts, an integer OR
// into the flag: sums and ORs of integers, whatever their order.  Workspace per cell: srecv 4, tour positions 8, order 1,
// in-degree 1, 8 that hold the whole grid's receivers and roots and then the mouth list, and 32 that hold the two copies of the
// tour and then the marks (8), the link pointers (8) and the head numbers (4); plus the scans' block sums and 512 bytes of
// counters.  Flow length takes the 32 alone.  No kernel uses scratch.
#include <limits.h>
#include <stdint.h>

#include "dsm_common.h"
#include "dsm_flow.h"
#include "dsm_scan.h"
#include "smvs_host.h"

namespace smvs {

typedef unsigned long long u64;

constexpr int ST_THREADS = D8_THREADS;
constexpr unsigned ST_END = 0xffffffffu;
constexpr int ST_MAX_ROUNDS = 30;
// the counters at the end of the workspace, ints: the four counts, the mouths, the length of the offsets' scan, then per order
// round the length of its scan and its total
enum { ST_CELLS = 0, ST_LINKS, ST_VERTICES, ST_TOP, ST_MOUTHS, ST_WLEN, ST_LEN, ST_TOT = ST_LEN + ST_MAX_ROUNDS + 2, ST_WORDS = 128 };

__device__ __forceinline__ u64 st_pair(unsigned low, u64 high) { return (u64)low | high << 32; }

// 0 E-W, 1 N-S, 2 diagonal: the kind of the step a code 1 .. 8 takes.
__device__ __forceinline__ int st_step_kind(unsigned code) { return (code & 1u) ? (int)(((code - 1) >> 1) & 1u) : 2; }

// ---- 1. the whole grid's forest (dsm_flow.h), then the induced one --------------------------------------------------------------
__global__ __launch_bounds__(ST_THREADS)
void st_induced(const unsigned char* __restrict__ mask, unsigned n, const int* __restrict__ recv, const int* __restrict__ up,
                int* __restrict__ srecv, int* __restrict__ mouth, int* words, int* flag)
{
    const unsigned i = blockIdx.x * (unsigned)ST_THREADS + threadIdx.x;
    bool cyclic = false, in_s = false;
    int to = D8_INVALID;
    if (i < n && recv[i] != D8_INVALID) {
        const unsigned root = (unsigned)up[i];
        cyclic = !(root < n && recv[root] == D8_ROOT);
        in_s = !cyclic && mask[i] != 0;
        if (in_s) {
            const int down = recv[i];                        // a tree cell's receiver is a tree cell: the mask decides
            to = down >= 0 && mask[down] != 0 ? down : D8_ROOT;
        }
    }
    if (__any(cyclic) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
    const int cells = __popcll(__ballot(in_s));
    if (cells && (threadIdx.x & 63) == 0) {
        atomicAdd(words + ST_CELLS, cells);
        atomicAdd(words + ST_VERTICES, cells);               // every cell is a vertex of its link; the junctions come in st_maps
    }
    if (i >= n) return;
    srecv[i] = to;
    mouth[i] = to == D8_ROOT;
}

// ---- 2. the tour ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ST_THREADS)
void st_mouth_list(unsigned n, const int* __restrict__ srecv, const int* __restrict__ mouth_at, int* __restrict__ list)
{
    const unsigned i = blockIdx.x * (unsigned)ST_THREADS + threadIdx.x;
    if (i < n && srecv[i] == D8_ROOT) list[mouth_at[i]] = (int)i;
}

// The first neighbour of cell p from direction k0 on that flows into p, as its down element; ST_END if there is none.
__device__ __forceinline__ unsigned st_child_from(const int* __restrict__ srecv, int gw, int gh, int p, int k0)
{
    const int r = p / gw, c = p % gw;
    unsigned found = ST_END;
#pragma unroll
    for (int k = 7; k >= 0; --k) {
        const int rr = r + d8_dr(k), cc = c + d8_dc(k);
        if (k < k0 || rr < 0 || rr >= gh || cc < 0 || cc >= gw) continue;
        const int child = rr * gw + cc;
        if (srecv[child] == p) found = 2u * (unsigned)child;
    }
    return found;
}

__global__ __launch_bounds__(ST_THREADS)
void st_tour(const unsigned char* __restrict__ dir, int gw, int gh, const int* __restrict__ srecv, const int* __restrict__ mouth_at,
             const int* __restrict__ list, const int* __restrict__ words, u64* __restrict__ tour)
{
    const unsigned n = (unsigned)gw * (unsigned)gh, i = blockIdx.x * (unsigned)ST_THREADS + threadIdx.x;
    if (i >= n) return;
    const int p = srecv[i];
    if (p == D8_INVALID) {
        tour[2 * (size_t)i] = tour[2 * (size_t)i + 1] = st_pair(ST_END, 0);
        return;
    }
    const unsigned first = st_child_from(srecv, gw, gh, (int)i, 0);
    const unsigned after_down = first != ST_END ? first : 2u * i + 1u;
    unsigned after_up;
    if (p >= 0) {
        const int from_parent = ((int)dir[i] - 1 + 4) & 7;  // the direction in which the receiver sees this cell
        const unsigned sibling = st_child_from(srecv, gw, gh, p, from_parent + 1);
        after_up = sibling != ST_END ? sibling : 2u * (unsigned)p + 1u;
    } else {
        const int next = mouth_at[i] + 1;                    // the trees one after another, in row-major order of their mouths
        after_up = next < words[ST_MOUTHS] ? 2u * (unsigned)list[next] : ST_END;
    }
    tour[2 * (size_t)i] = st_pair(after_down, 1);
    tour[2 * (size_t)i + 1] = st_pair(after_up, 1);
}

// One Wyllie round from one copy into the other: count'(e) = count(e) + count(succ e), succ'(e) = succ(succ e).  A latency-bound
// gather of one 64-bit word per lane (fl_double takes two, successor and sum apart): with 6 VGPRs nothing but the number of
// waves in flight hides the latency, and workgroups of 256 lanes fill a CU's eight waves per SIMD.
__global__ __launch_bounds__(ST_THREADS)
void st_rank(unsigned m, const u64* __restrict__ in, u64* __restrict__ out)
{
    const unsigned e = blockIdx.x * (unsigned)ST_THREADS + threadIdx.x;
    if (e >= m) return;
    const u64 a = in[e];
    const unsigned s = (unsigned)a;
    if (s >= m) { out[e] = a; return; }
    const u64 b = in[s];
    out[e] = st_pair((unsigned)b, (a >> 32) + (b >> 32));
}

__global__ __launch_bounds__(ST_THREADS)
void st_positions(unsigned n, const int* __restrict__ srecv, const u64* __restrict__ tour, const int* __restrict__ words,
                  int2* __restrict__ pos, unsigned char* __restrict__ ord)
{
    const unsigned i = blockIdx.x * (unsigned)ST_THREADS + threadIdx.x;
    if (i >= n) return;
    const bool in_s = srecv[i] != D8_INVALID;
    const int total = 2 * words[ST_CELLS], last = (int)(2 * n) - 1;
    const int down = total - (int)(tour[2 * (size_t)i] >> 32), up = total - (int)(tour[2 * (size_t)i + 1] >> 32);
    // a list of 2 |S| elements ranks to 0 .. 2 |S| - 1; the clamp keeps every later index on the marks whatever happens
    pos[i] = in_s ? make_int2(min(max(down, 0), last), min(max(up, 0), last)) : make_int2(0, 0);
    ord[i] = in_s;
}

// ---- 3. an order round ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ST_THREADS)
void st_mark(int gw, int gh, int k, const int* __restrict__ srecv, const unsigned char* __restrict__ ord, const int2* __restrict__ pos,
             int* __restrict__ marks, int* words)
{
    const unsigned n = (unsigned)gw * (unsigned)gh, i = blockIdx.x * (unsigned)ST_THREADS + threadIdx.x;
    const bool active = k == 1 || words[ST_TOT + k - 1] > 0;
    if (i == 0) words[ST_LEN + k] = active ? 2 * words[ST_CELLS] : 0;
    if (!active || i >= n || srecv[i] == D8_INVALID) return;
    const int r = (int)(i / (unsigned)gw), c = (int)(i % (unsigned)gw);
    int inflow = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int rr = r + d8_dr(j), cc = c + d8_dc(j);
        if (rr < 0 || rr >= gh || cc < 0 || cc >= gw) continue;
        const int u = rr * gw + cc;
        inflow += srecv[u] == (int)i && ord[u] == k;
    }
    const int2 at = pos[i];
    marks[at.x] = inflow >= 2;
    marks[at.y] = 0;
}

__global__ __launch_bounds__(ST_THREADS)
void st_promote(unsigned n, int k, const int2* __restrict__ pos, const int* __restrict__ marks, const int* __restrict__ words,
                unsigned char* __restrict__ ord)
{
    const unsigned i = blockIdx.x * (unsigned)ST_THREADS + threadIdx.x;
    if (words[ST_TOT + k] == 0 || i >= n || ord[i] != k) return;
    const int2 at = pos[i];
    if (marks[at.y] - marks[at.x] > 0) ord[i] = (unsigned char)(k + 1);
}

// ---- 4. links ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ST_THREADS)
void st_heads(int gw, int gh, const int* __restrict__ srecv, unsigned char* __restrict__ inflow, u64* __restrict__ lp, int* __restrict__ head_at)
{
    const unsigned n = (unsigned)gw * (unsigned)gh, i = blockIdx.x * (unsigned)ST_THREADS + threadIdx.x;
    if (i >= n) return;
    if (srecv[i] == D8_INVALID) {
        inflow[i] = 255;
        lp[i] = st_pair(i, 0);
        head_at[i] = 0;
        return;
    }
    const int r = (int)(i / (unsigned)gw), c = (int)(i % (unsigned)gw);
    int count = 0;
    unsigned from = i;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int rr = r + d8_dr(j), cc = c + d8_dc(j);
        if (rr < 0 || rr >= gh || cc < 0 || cc >= gw) continue;
        const int u = rr * gw + cc;
        if (srecv[u] == (int)i) { ++count; from = (unsigned)u; }
    }
    inflow[i] = (unsigned char)count;
    lp[i] = count == 1 ? st_pair(from, 1) : st_pair(i, 0);
    head_at[i] = count != 1;
}

// lp <- lp o lp with the distances added, in place (the header comment says why that is sound).
__global__ __launch_bounds__(ST_THREADS)
void st_link_jump(unsigned n, u64* lp)
{
    const unsigned i = blockIdx.x * (unsigned)ST_THREADS + threadIdx.x;
    if (i >= n) return;
    const u64 a = lp[i];
    const unsigned p = (unsigned)a;
    if (p >= n || p == i) return;
    const u64 b = lp[p];
    const unsigned q = (unsigned)b;
    if (q < n && q != p) lp[i] = st_pair(q, (a >> 32) + (b >> 32));
}

// Whether cell i of S, flowing into `down`, is the last of its link.
__device__ __forceinline__ bool st_link_ends(const unsigned char* __restrict__ inflow, int down) { return down < 0 || inflow[down] >= 2; }

__global__ __launch_bounds__(ST_THREADS)
void st_maps(unsigned n, const int* __restrict__ srecv, const unsigned char* __restrict__ inflow, const u64* __restrict__ lp,
             const int* __restrict__ head_at, const unsigned char* __restrict__ ord, unsigned char* __restrict__ order,
             int* __restrict__ link_map, int* words)
{
    const unsigned i = blockIdx.x * (unsigned)ST_THREADS + threadIdx.x;
    const int down = i < n ? srecv[i] : D8_INVALID;
    const int junctions = __popcll(__ballot(down >= 0 && st_link_ends(inflow, down)));    // a link's closing vertex
    if (junctions && (threadIdx.x & 63) == 0) atomicAdd(words + ST_VERTICES, junctions);
    if (i >= n) return;
    if (order) order[i] = ord[i];
    if (link_map) link_map[i] = down != D8_INVALID ? head_at[(unsigned)lp[i]] + 1 : 0;
}

// The highest order = 1 + the rounds that promoted a cell; then the counts to the caller.
__global__ void st_counts(int rounds, int* words, int* __restrict__ counts)
{
    if (threadIdx.x != 0) return;
    int top = words[ST_CELLS] > 0;
    for (int k = 1; k <= rounds; ++k) top += words[ST_TOT + k] > 0;
    words[ST_TOP] = top;
    if (counts)
        for (int k = 0; k < 4; ++k) counts[k] = words[k];
}

__device__ __forceinline__ bool st_counts_match(const int* __restrict__ words, int n_links, int n_vertices)
{
    return words[ST_LINKS] == n_links && words[ST_VERTICES] == n_vertices;
}

__global__ __launch_bounds__(ST_THREADS)
void st_tables(const unsigned char* __restrict__ dir, unsigned n, const int* __restrict__ srecv, const unsigned char* __restrict__ inflow,
               const u64* __restrict__ lp, const int* __restrict__ head_at, const unsigned char* __restrict__ ord, int* words,
               int n_links, int n_vertices, int* __restrict__ head, int* __restrict__ link_order, int* __restrict__ next_link,
               int* __restrict__ offset, int* steps)
{
    const unsigned i = blockIdx.x * (unsigned)ST_THREADS + threadIdx.x;
    const bool match = st_counts_match(words, n_links, n_vertices);
    if (i == 0) words[ST_WLEN] = match ? n_links : 0;
    if (!match || i >= n) return;
    const int down = srecv[i];
    if (down == D8_INVALID) return;
    const u64 a = lp[i];
    const unsigned h = (unsigned)a;
    const int link = head_at[h];
    if (link < 0 || link >= n_links) return;                // cannot be: the counts match
    if (h == i) {
        head[link] = (int)i;
        link_order[link] = ord[i];
    }
    if (down >= 0) atomicAdd(steps + 3 * (size_t)link + st_step_kind(dir[i]), 1);
    if (st_link_ends(inflow, down)) {
        next_link[link] = down >= 0 ? head_at[down] : -1;
        offset[link] = (int)(a >> 32) + 1 + (down >= 0);     // the vertices of the link; the scan turns them into offsets
    }
}

__global__ __launch_bounds__(ST_THREADS)
void st_vertices(int gw, unsigned n, const int* __restrict__ srecv, const unsigned char* __restrict__ inflow, const u64* __restrict__ lp,
                 const int* __restrict__ head_at, const int* __restrict__ words, int n_links, int n_vertices, int* offset,
                 int2* __restrict__ vertices)
{
    const unsigned i = blockIdx.x * (unsigned)ST_THREADS + threadIdx.x;
    if (!st_counts_match(words, n_links, n_vertices)) {
        if (i == 0) offset[n_links] = -1;
        return;
    }
    if (i >= n) return;
    const int down = srecv[i];
    if (down == D8_INVALID) return;
    const u64 a = lp[i];
    const int link = head_at[(unsigned)a];
    if (link < 0 || link >= n_links) return;
    const long long at = (long long)offset[link] + (long long)(a >> 32);
    if (at < 0 || at >= n_vertices) return;                  // cannot be: offsets and distances of one pass
    vertices[at] = make_int2((int)(i % (unsigned)gw), (int)(i / (unsigned)gw));
    if (down >= 0 && st_link_ends(inflow, down) && at + 1 < n_vertices)
        vertices[at + 1] = make_int2(down % gw, down / gw);
}

__global__ void st_no_links(const int* __restrict__ words, int n_vertices, int* __restrict__ offset)
{
    if (threadIdx.x == 0) offset[0] = st_counts_match(words, 0, n_vertices) ? 0 : -1;
}

// ---- flow length ---------------------------------------------------------------------------------------------------------------
// A cell is two words: (receiver | diagonal steps << 32) and (E-W steps | N-S steps << 32); counts stay below 2^30.
__global__ __launch_bounds__(ST_THREADS)
void st_length_begin(const unsigned char* __restrict__ dir, int gw, int gh, u64* __restrict__ to, u64* __restrict__ steps)
{
    const unsigned n = (unsigned)gw * (unsigned)gh, i = blockIdx.x * (unsigned)ST_THREADS + threadIdx.x;
    if (i >= n) return;
    const int down = d8_receiver(dir, nullptr, gw, gh, (int)(i / (unsigned)gw), (int)(i % (unsigned)gw));
    const int kind = down >= 0 ? st_step_kind(dir[i]) : -1;
    to[i] = st_pair(down >= 0 ? (unsigned)down : ST_END, kind == 2);
    steps[i] = st_pair(kind == 0, kind == 1);
}

__global__ __launch_bounds__(ST_THREADS)
void st_length_double(unsigned n, const u64* __restrict__ to, const u64* __restrict__ steps, u64* __restrict__ to_out, u64* __restrict__ steps_out)
{
    const unsigned i = blockIdx.x * (unsigned)ST_THREADS + threadIdx.x;
    if (i >= n) return;
    const u64 a = to[i], s = steps[i];
    const unsigned p = (unsigned)a;
    if (p >= n) { to_out[i] = a; steps_out[i] = s; return; }
    const u64 b = to[p];
    to_out[i] = st_pair((unsigned)b, (a >> 32) + (b >> 32));
    steps_out[i] = s + steps[p];
}

__global__ __launch_bounds__(ST_THREADS)
void st_length_end(const unsigned char* __restrict__ dir, unsigned n, const u64* __restrict__ to, const u64* __restrict__ steps,
                   int* __restrict__ out, int* flag)
{
    const unsigned i = blockIdx.x * (unsigned)ST_THREADS + threadIdx.x;
    const bool coded = i < n && dir[i] <= 8;
    const u64 a = coded ? to[i] : st_pair(ST_END, 0);
    const bool cyclic = (unsigned)a != ST_END;               // still on its way after 2^rounds >= n steps
    if (__any(cyclic) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
    if (i >= n) return;
    const bool tree = coded && !cyclic;
    const u64 s = tree ? steps[i] : 0;
    out[3 * (size_t)i] = tree ? (int)(unsigned)s : -1;
    out[3 * (size_t)i + 1] = tree ? (int)(s >> 32) : -1;
    out[3 * (size_t)i + 2] = tree ? (int)(a >> 32) : -1;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct StreamWorkspace { size_t srecv, pos, ord, inflow, pair, tour, s1, s2, words, bytes, length_bytes; };

static StreamWorkspace stream_workspace(size_t n)
{
    StreamWorkspace w;
    const size_t nb1 = (2 * n + OL_BLOCK - 1) / OL_BLOCK, nb2 = (nb1 + OL_BLOCK - 1) / OL_BLOCK;
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t here = at; at += align256(bytes); return here; };
    w.tour = take(n * 32);                                   // first, so that flow length finds its two copies of two words here
    w.length_bytes = at;
    w.srecv = take(n * 4);
    w.pos = take(n * 8);
    w.ord = take(n);
    w.inflow = take(n);
    w.pair = take(n * 8);
    w.s1 = take(nb1 * 4);
    w.s2 = take(nb2 * 4);
    w.words = take(ST_WORDS * 4);
    w.bytes = at;
    return w;
}

// What the entries check alike: the grid, and that no two of the buffers given (null or empty ones skipped) share a byte.
static int stream_check(int gw, int gh, const DsmBuf* buf, int n_buf)
{
    if (const char* msg = d8_grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s (got %d x %d)", msg, gw, gh);
    const char* other = nullptr;
    if (const char* name = dsm_first_alias(buf, n_buf, other)) return fail(SMVS_ERR_ARG, "%s aliases %s", name, other);
    return SMVS_OK;
}

static int stream_order_rounds(size_t n)                     // an order k needs 2^(k - 1) sources: k <= floor(log2 n) + 1, and 30 at 2^30 cells
{
    int r = 0;
    while (((size_t)2 << r) <= n) ++r;
    return r < ST_MAX_ROUNDS ? r : ST_MAX_ROUNDS;
}

// The network pass: everything the two entries share.  order, link_map and counts may be null.
static int stream_pass(const unsigned char* dir, const unsigned char* mask, int gw, int gh, unsigned char* order, int* link_map,
                       int* counts, int* flag, char* base, const StreamWorkspace& w, hipStream_t s)
{
    const size_t n = (size_t)gw * gh;
    int* srecv = (int*)(base + w.srecv);
    int2* pos = (int2*)(base + w.pos);
    unsigned char *ord = (unsigned char*)(base + w.ord), *inflow = (unsigned char*)(base + w.inflow);
    int *recv = (int*)(base + w.pair), *up = recv + n, *list = recv;          // the mouth list once the whole grid's forest is done with
    u64* tour[2] = {(u64*)(base + w.tour), (u64*)(base + w.tour) + 2 * n};
    int* mouth_at = (int*)tour[1];                           // dead before the first round of the ranking writes the second copy
    int* marks = (int*)(base + w.tour);                      // after the ranking: 2 n marks, n link pointers, n head numbers
    u64* lp = (u64*)(base + w.tour) + n;
    int* head_at = (int*)((u64*)(base + w.tour) + 2 * n);
    int *s1 = (int*)(base + w.s1), *s2 = (int*)(base + w.s2), *words = (int*)(base + w.words);
    int rc;
    if (hipMemsetAsync(words, 0, ST_WORDS * 4, s) != hipSuccess) return check_launch("dsm_stream (clearing the counters)");
    if (flag && hipMemsetAsync(flag, 0, 4, s) != hipSuccess) return check_launch("dsm_stream (clearing the flag)");
    int* flag_word = flag ? flag : words + ST_WORDS - 1;
    if ((rc = d8_roots(dir, nullptr, gw, gh, recv, up, s))) return rc;
    DSM_LAUNCH(st_induced, n, ST_THREADS, s, mask, (unsigned)n, (const int*)recv, (const int*)up, srecv, mouth_at, words, flag_word);
    if ((rc = ol_scan_exclusive(mouth_at, (unsigned)n, nullptr, s1, s2, words + ST_MOUTHS, s, "ol_scan (mouths)"))) return rc;
    DSM_LAUNCH(st_mouth_list, n, ST_THREADS, s, (unsigned)n, (const int*)srecv, (const int*)mouth_at, list);
    DSM_LAUNCH(st_tour, n, ST_THREADS, s, dir, gw, gh, (const int*)srecv, (const int*)mouth_at, (const int*)list, (const int*)words, tour[0]);
    int at = 0;
    for (int k = 0, rounds = dsm_ceil_log2(2 * n); k < rounds; ++k, at ^= 1) DSM_LAUNCH(st_rank, 2 * n, ST_THREADS, s, (unsigned)(2 * n), (const u64*)tour[at], tour[at ^ 1]);
    DSM_LAUNCH(st_positions, n, ST_THREADS, s, (unsigned)n, (const int*)srecv, (const u64*)tour[at], (const int*)words, pos, ord);
    const int rounds = stream_order_rounds(n);
    for (int k = 1; k <= rounds; ++k) {
        DSM_LAUNCH(st_mark, n, ST_THREADS, s, gw, gh, k, (const int*)srecv, (const unsigned char*)ord, (const int2*)pos, marks, words);
        if ((rc = ol_scan_exclusive(marks, (unsigned)(2 * n), words + ST_LEN + k, s1, s2, words + ST_TOT + k, s, "ol_scan (marks)"))) return rc;
        DSM_LAUNCH(st_promote, n, ST_THREADS, s, (unsigned)n, k, (const int2*)pos, (const int*)marks, (const int*)words, ord);
    }
    DSM_LAUNCH(st_heads, n, ST_THREADS, s, gw, gh, (const int*)srecv, inflow, lp, head_at);
    if ((rc = ol_scan_exclusive(head_at, (unsigned)n, nullptr, s1, s2, words + ST_LINKS, s, "ol_scan (heads)"))) return rc;
    for (int k = 0, jumps = dsm_ceil_log2(n) + 1; k < jumps; ++k) DSM_LAUNCH(st_link_jump, n, ST_THREADS, s, (unsigned)n, lp);
    DSM_LAUNCH(st_maps, n, ST_THREADS, s, (unsigned)n, (const int*)srecv, (const unsigned char*)inflow, (const u64*)lp, (const int*)head_at,
              (const unsigned char*)ord, order, link_map, words);
    DSM_LAUNCH(st_counts, 1, 64, s, rounds, words, counts);
    return SMVS_OK;
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT size_t smvs_dsm_stream_workspace_bytes(int gw, int gh)
{
    using namespace smvs;
    return d8_grid_check(gw, gh) ? 0 : stream_workspace((size_t)gw * gh).bytes;
}

SMVS_EXPORT int smvs_dsm_stream_order(const unsigned char* dir, const unsigned char* mask, int gw, int gh, unsigned char* order,
                                      int* link_map, int* counts, int* flag, void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!dir || !mask || !order || !counts || !flag || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    const size_t n = gw > 0 && gh > 0 ? (size_t)gw * gh : 0;
    const StreamWorkspace w = stream_workspace(n);
    const DsmBuf buf[] = {{dir, n, "dir"}, {mask, n, "mask"}, {order, n, "order"}, {link_map, n * 4, "link_map"}, {counts, 16, "counts"},
                         {flag, 4, "flag"}, {workspace, w.bytes, "workspace"}};
    if (int rc = stream_check(gw, gh, buf, 7)) return rc;
    if (workspace_bytes < w.bytes) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, w.bytes);
    return stream_pass(dir, mask, gw, gh, order, link_map, counts, flag, (char*)workspace, w, (hipStream_t)stream);
}

SMVS_EXPORT int smvs_dsm_stream_write(const unsigned char* dir, const unsigned char* mask, int gw, int gh, int n_links, int n_vertices,
                                      int* head, int* link_order, int* next_link, int* offset, int* vertices, int* steps,
                                      void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!dir || !mask || !head || !link_order || !next_link || !offset || !vertices || !steps || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (n_links < 0 || n_vertices < 0) return fail(SMVS_ERR_ARG, "negative count: n_links %d, n_vertices %d", n_links, n_vertices);
    const size_t n = gw > 0 && gh > 0 ? (size_t)gw * gh : 0, nl = (size_t)n_links, nv = (size_t)n_vertices;
    if (n && (nl > n || nv > 2 * n)) return fail(SMVS_ERR_ARG, "more links (%d) than cells or more vertices (%d) than twice the cells (%zu)", n_links, n_vertices, n);
    const StreamWorkspace w = stream_workspace(n);
    const DsmBuf buf[] = {{dir, n, "dir"}, {mask, n, "mask"}, {head, nl * 4, "head"}, {link_order, nl * 4, "link_order"}, {next_link, nl * 4, "next_link"},
                         {offset, (nl + 1) * 4, "offset"}, {vertices, nv * 8, "vertices"}, {steps, nl * 12, "steps"}, {workspace, w.bytes, "workspace"}};
    if (int rc = stream_check(gw, gh, buf, 9)) return rc;
    if (workspace_bytes < w.bytes) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, w.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)workspace;
    if (int rc = stream_pass(dir, mask, gw, gh, nullptr, nullptr, nullptr, nullptr, base, w, s)) return rc;
    int* words = (int*)(base + w.words);
    if (n_links == 0) {
        DSM_LAUNCH(st_no_links, 1, 64, s, (const int*)words, n_vertices, offset);
        return SMVS_OK;
    }
    const int* srecv = (const int*)(base + w.srecv);
    const unsigned char *ord = (const unsigned char*)(base + w.ord), *inflow = (const unsigned char*)(base + w.inflow);
    const u64* lp = (const u64*)(base + w.tour) + n;
    const int* head_at = (const int*)((const u64*)(base + w.tour) + 2 * n);
    if (hipMemsetAsync(steps, 0, nl * 12, s) != hipSuccess) return check_launch("dsm_stream_write (clearing the step counts)");
    DSM_LAUNCH(st_tables, n, ST_THREADS, s, dir, (unsigned)n, srecv, inflow, lp, head_at, ord, words, n_links, n_vertices, head, link_order, next_link, offset, steps);
    if (int rc = ol_scan_exclusive(offset, (unsigned)n_links, words + ST_WLEN, (int*)(base + w.s1), (int*)(base + w.s2), offset + n_links, s, "ol_scan (offsets)")) return rc;
    DSM_LAUNCH(st_vertices, n, ST_THREADS, s, gw, (unsigned)n, srecv, inflow, lp, head_at, (const int*)words, n_links, n_vertices, offset, (int2*)vertices);
    return SMVS_OK;
}

SMVS_EXPORT int smvs_dsm_flow_length(const unsigned char* dir, int gw, int gh, int* steps, int* flag,
                                     void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!dir || !steps || !flag || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    const size_t n = gw > 0 && gh > 0 ? (size_t)gw * gh : 0;
    const StreamWorkspace w = stream_workspace(n);
    const DsmBuf buf[] = {{dir, n, "dir"}, {steps, n * 12, "steps"}, {flag, 4, "flag"}, {workspace, w.bytes, "workspace"}};
    if (int rc = stream_check(gw, gh, buf, 4)) return rc;
    if (workspace_bytes < w.bytes) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, w.bytes);
    hipStream_t s = (hipStream_t)stream;
    u64* to[2] = {(u64*)workspace, (u64*)workspace + 2 * n};
    u64* sum[2] = {to[0] + n, to[1] + n};
    if (hipMemsetAsync(flag, 0, 4, s) != hipSuccess) return check_launch("dsm_flow_length (clearing the flag)");
    DSM_LAUNCH(st_length_begin, n, ST_THREADS, s, dir, gw, gh, to[0], sum[0]);
    int at = 0;
    for (int k = 0, rounds = dsm_ceil_log2(n); k < rounds; ++k, at ^= 1)
        DSM_LAUNCH(st_length_double, n, ST_THREADS, s, (unsigned)n, (const u64*)to[at], (const u64*)sum[at], to[at ^ 1], sum[at ^ 1]);
    DSM_LAUNCH(st_length_end, n, ST_THREADS, s, dir, (unsigned)n, (const u64*)to[at], (const u64*)sum[at], steps, flag);
    return SMVS_OK;
}

}  // extern "C"
