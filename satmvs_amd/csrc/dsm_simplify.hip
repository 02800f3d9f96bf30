// dsm_simplify.hip -- Douglas-Peucker on closed rings of integer vertices, exact ("Simplified outlines";
// include/satmvs.h for the rule).
//
//   smvs_dsm_simplify_begin   checks the rings (flag), finds the two anchors of every ring, sets up the segments
//   smvs_dsm_simplify_rounds  `rounds` rounds: every live segment finds its farthest vertex and splits there or dies
//   smvs_dsm_simplify_count   compacts the kept vertices, takes the shoelace sums, decides the fall-back -> n_vertices_out
//   smvs_dsm_simplify_write   the new offset table, vertices, area2, kept and simplified into buffers sized from that count
//
// A ring of m vertices at begin .. end - 1 of the vertex list is the chain of positions begin .. end, position end standing for
// the ring's first vertex again.  The state of a vertex that is neither kept nor dropped yet is its segment: the positions of
// its kept neighbours on the left and on the right.  The vertices of a segment are neighbours in the vertex list, so the lanes
// of a wave that share a segment (or, in the sums, a ring) stand side by side: they combine by a shuffle that stops at the run's
// end, and the run's first lane makes the one atomic.  The slots of a segment are those of its left anchor.  A round:
//   sp_keys    key of every live vertex; atomicMax into kmax[left]; the segment's first lane resets kmin[left]
//   sp_pick    among the lanes whose key is the maximum, atomicMin of (|2 i - a - b| << 32 | i) into kmin[left]; the segment's
//              first lane copies the maximum to kdec[left]
//   sp_decide  the winner is kept if the key passes the tolerance, the others move their left or right to it; else the whole
//              segment is dropped; the segment's first lane resets kmax[left]
// No slot is read and written by different lanes of one kernel.  Integer atomics only (max, min, add): the bits do not depend
// on their order.  Every index read back from the workspace is checked before it is used; a bad one sets the error word, the
// lane stops, and the status / the count / offset[n_rings] come back as -1.
#include <limits.h>
#include <stdint.h>

#include "dsm_common.h"
#include "dsm_scan.h"
#include "smvs_host.h"

namespace smvs {

constexpr int SP_THREADS = OL_THREADS;
constexpr int SP_MAX_COORD = 32767, SP_MAX_TOL16 = 65535, SP_MAX_ROUNDS = 4096;
enum { SP_ERR = 0, SP_SPLIT, SP_LAST, SP_ROUNDS, SP_DONE, SP_OPEN, SP_NKEPT, SP_NOUT };           // the workspace's tail words

typedef unsigned long long u64;
typedef long long i64;

struct SpState {
    int *tail, *vring, *left, *right, *keep, *pos, *klist, *rcount;
    u64 *vkey, *kmax, *kmin, *kdec, *anchor;
    i64 *a2in, *a2out;
    unsigned char* simp;
};

// ---- lanes side by side that share a key ---------------------------------------------------------------------------------------
__device__ __forceinline__ bool sp_run_head(int key)
{
    const int before = __shfl_up(key, 1);
    return (threadIdx.x & 63) == 0 || before != key;
}

// v of the run's first lane <- op over the run.  Every lane of the wave calls this.
template <class T, class Op>
__device__ __forceinline__ T sp_run_reduce(T v, int key, Op op)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_down(v, d);
        const int k = __shfl_down(key, d);
        if (lane + d < 64 && k == key) v = op(v, o);
    }
    return v;
}

struct SpMax { __device__ u64 operator()(u64 a, u64 b) const { return a > b ? a : b; } };
struct SpMin { __device__ u64 operator()(u64 a, u64 b) const { return a < b ? a : b; } };
struct SpAdd { __device__ i64 operator()(i64 a, i64 b) const { return a + b; } };

// A coordinate as the arithmetic takes it: 15 bits, so that no product overflows whatever the vertex list holds (a value outside
// 0 .. 32767 is flag bit 0, and the caller does not use the result).
__device__ __forceinline__ void sp_xy(const int* __restrict__ vertices, unsigned i, int& x, int& y)
{
    x = vertices[2 * (size_t)i] & SP_MAX_COORD;
    y = vertices[2 * (size_t)i + 1] & SP_MAX_COORD;
}

// The ring of vertex i as the workspace has it, and its span; false (and the error word) if either is not what it can be.
__device__ __forceinline__ bool sp_ring_of(const SpState& st, const int* __restrict__ offset, unsigned nr, unsigned nv, unsigned i,
                                           unsigned& r, unsigned& begin, unsigned& end)
{
    r = (unsigned)st.vring[i];
    if (r < nr) {
        begin = (unsigned)offset[r];
        end = (unsigned)offset[r + 1];
        if (begin <= i && i < end && end <= nv) return true;
    }
    atomicOr(st.tail + SP_ERR, 1);
    return false;
}

// ---- begin ---------------------------------------------------------------------------------------------------------------------
// One lane per vertex, and one per entry of the offset table: the checks, the ring of the vertex, and the far anchor's vote.
__global__ __launch_bounds__(SP_THREADS)
void sp_init(const int* __restrict__ vertices, const int* __restrict__ offset, unsigned nr, unsigned nv, SpState st, int* flag)
{
    const unsigned i = blockIdx.x * (unsigned)SP_THREADS + threadIdx.x;
    if (i < nr && (offset[i] < 0 || offset[i] > offset[i + 1])) atomicOr(flag, 2);
    if (i == 0 && (offset[0] != 0 || (unsigned)offset[nr] != nv)) atomicOr(flag, 2);
    int run = -1;
    u64 vote = 0;
    if (i < nv) {
        unsigned lo = 0, hi = nr;                            // the last ring whose offset is <= i
        for (int step = 0; step < 32 && lo < hi; ++step) {
            const unsigned mid = lo + (hi - lo) / 2;
            if ((unsigned)offset[mid] <= i) lo = mid + 1;
            else hi = mid;
        }
        const unsigned r = lo - 1;                           // lo == 0 gives r >= nr
        const unsigned begin = r < nr ? (unsigned)offset[r] : 0, end = r < nr ? (unsigned)offset[r + 1] : 0;
        if (r >= nr || begin > i || end <= i || end > nv) atomicOr(flag, 2);
        else {
            st.vring[i] = (int)r;
            if ((unsigned)vertices[2 * (size_t)i] > (unsigned)SP_MAX_COORD || (unsigned)vertices[2 * (size_t)i + 1] > (unsigned)SP_MAX_COORD) atomicOr(flag, 1);
            int x, y, x0, y0;
            sp_xy(vertices, i, x, y);
            sp_xy(vertices, begin, x0, y0);
            const u64 d2 = (u64)((i64)(x - x0) * (x - x0) + (i64)(y - y0) * (y - y0));     // < 2^31
            vote = d2 << 32 | (u64)(unsigned)~(i - begin);                                // ties to the lowest index
            run = (int)r;
        }
    }
    const u64 best = sp_run_reduce(vote, run, SpMax());
    if (sp_run_head(run) && run >= 0) atomicMax(st.anchor + run, best);
}

// One lane per vertex: kept if it is one of its ring's two anchors, else in the segment on its side of the far anchor.  A ring
// of fewer than three vertices, or with all vertices equal, keeps everything.
__global__ __launch_bounds__(SP_THREADS)
void sp_segments(const int* __restrict__ offset, unsigned nr, unsigned nv, SpState st)
{
    const unsigned i = blockIdx.x * (unsigned)SP_THREADS + threadIdx.x;
    if (i >= nv) return;
    if (st.vring[i] < 0) return;                             // no ring: begin has said so in the flag
    unsigned r, begin, end;
    if (!sp_ring_of(st, offset, nr, nv, i, r, begin, end)) return;
    const u64 word = st.anchor[r];
    const unsigned m = end - begin, far = ~(unsigned)word, li = i - begin;
    if (m < 3 || (word >> 32) == 0) { st.keep[i] = 1; return; }
    if (far == 0 || far >= m) { atomicOr(st.tail + SP_ERR, 1); return; }
    if (li == 0 || li == far) { st.keep[i] = 1; return; }
    st.left[i] = (int)(li < far ? begin : begin + far);
    st.right[i] = (int)(li < far ? begin + far : end);
}

// ---- a round -------------------------------------------------------------------------------------------------------------------
// The book-keeping of the round that has just ended, by one lane before the next begins (or by the status kernel).
__device__ __forceinline__ void sp_close_round(int* tail)
{
    if (!tail[SP_OPEN]) return;
    tail[SP_OPEN] = 0;
    if (!tail[SP_DONE]) {
        ++tail[SP_ROUNDS];
        if (tail[SP_SPLIT] == 0) tail[SP_DONE] = 1;
    }
    tail[SP_LAST] = tail[SP_SPLIT];
    tail[SP_SPLIT] = 0;
}

// The segment of a live vertex: positions a < i < b of one ring.  false: the vertex is not live (or its state is damaged).
__device__ __forceinline__ bool sp_segment_of(const SpState& st, const int* __restrict__ offset, unsigned nr, unsigned nv, unsigned i,
                                              unsigned& a, unsigned& b, unsigned& begin, unsigned& end)
{
    const int left = st.left[i];
    if (left < 0) return false;
    unsigned r;
    if (!sp_ring_of(st, offset, nr, nv, i, r, begin, end)) return false;
    a = (unsigned)left;
    b = (unsigned)st.right[i];
    if (a < begin || a >= i || b <= i || b > end) { atomicOr(st.tail + SP_ERR, 1); return false; }
    return true;
}

// |v_i - segment (v_a, v_b)|^2 |v_b - v_a|^2, or |v_i - v_a|^2 if the two ends are one point; L <- |v_b - v_a|^2.
__device__ __forceinline__ u64 sp_key(int xa, int ya, int xb, int yb, int xi, int yi)
{
    const i64 dx = xb - xa, dy = yb - ya, ux = xi - xa, uy = yi - ya;
    const i64 L = dx * dx + dy * dy, t = ux * dx + uy * dy, uu = ux * ux + uy * uy;
    if (L == 0) return (u64)uu;
    if (t <= 0) return (u64)uu * (u64)L;
    if (t >= L) {
        const i64 wx = xi - xb, wy = yi - yb;
        return (u64)(wx * wx + wy * wy) * (u64)L;
    }
    const i64 cross = dx * uy - dy * ux;
    return (u64)(cross * cross);
}

__global__ __launch_bounds__(SP_THREADS)
void sp_keys(const int* __restrict__ vertices, const int* __restrict__ offset, unsigned nr, unsigned nv, SpState st)
{
    const unsigned i = blockIdx.x * (unsigned)SP_THREADS + threadIdx.x;
    if (i == 0) {
        sp_close_round(st.tail);
        st.tail[SP_OPEN] = 1;
    }
    int run = -1;
    u64 key = 0;
    unsigned a, b, begin, end;
    if (i < nv && sp_segment_of(st, offset, nr, nv, i, a, b, begin, end)) {
        int xa, ya, xb, yb, xi, yi;
        sp_xy(vertices, a, xa, ya);
        sp_xy(vertices, b == end ? begin : b, xb, yb);
        sp_xy(vertices, i, xi, yi);
        key = sp_key(xa, ya, xb, yb, xi, yi);
        st.vkey[i] = key;
        if (i == a + 1) st.kmin[a] = ~0ull;
        run = (int)a;
    }
    const u64 best = sp_run_reduce(key, run, SpMax());
    if (sp_run_head(run) && run >= 0) atomicMax(st.kmax + run, best);
}

__global__ __launch_bounds__(SP_THREADS)
void sp_pick(const int* __restrict__ offset, unsigned nr, unsigned nv, SpState st)
{
    const unsigned i = blockIdx.x * (unsigned)SP_THREADS + threadIdx.x;
    int run = -1;
    u64 bid = ~0ull;
    unsigned a, b, begin, end;
    if (i < nv && sp_segment_of(st, offset, nr, nv, i, a, b, begin, end)) {
        const u64 top = st.kmax[a];
        if (i == a + 1) st.kdec[a] = top;
        if (st.vkey[i] == top) {
            const i64 off = 2 * (i64)i - (i64)a - (i64)b;                     // nearest the middle first, then the lower index
            bid = (u64)(off < 0 ? -off : off) << 32 | (u64)i;
        }
        run = (int)a;
    }
    const u64 best = sp_run_reduce(bid, run, SpMin());
    if (sp_run_head(run) && run >= 0 && best != ~0ull) atomicMin(st.kmin + run, best);
}

__global__ __launch_bounds__(SP_THREADS)
void sp_decide(const int* __restrict__ vertices, const int* __restrict__ offset, unsigned nr, unsigned nv, unsigned tol16, SpState st)
{
    const unsigned i = blockIdx.x * (unsigned)SP_THREADS + threadIdx.x;
    bool won = false;
    unsigned a, b, begin, end;
    if (i < nv && sp_segment_of(st, offset, nr, nv, i, a, b, begin, end)) {
        const u64 top = st.kdec[a];
        const unsigned w = (unsigned)st.kmin[a];
        int xa, ya, xb, yb;
        sp_xy(vertices, a, xa, ya);
        sp_xy(vertices, b == end ? begin : b, xb, yb);
        const i64 dx = xb - xa, dy = yb - ya;
        const u64 L = (u64)(dx * dx + dy * dy), t2 = (u64)tol16 * tol16;     // t2 < 2^32, L < 2^31
        const u64 bound = (L ? t2 * L : t2) >> 8;
        if (i == a + 1) st.kmax[a] = 0;
        if (top <= bound) st.left[i] = -1;                   // within the tolerance: the segment's vertices are dropped
        else if (w <= a || w >= b) { atomicOr(st.tail + SP_ERR, 1); st.left[i] = -1; }
        else if (i == w) { st.keep[i] = 1; st.left[i] = -1; won = true; }
        else if (i < w) st.right[i] = (int)w;
        else st.left[i] = (int)w;
    }
    const int cnt = __popcll(__ballot(won));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(st.tail + SP_SPLIT, cnt);
}

// status[0] <- the segments that split in the last round, status[1] <- the rounds run up to and with the first that split none.
__global__ void sp_status(SpState st, int* __restrict__ status)
{
    if (threadIdx.x != 0) return;
    sp_close_round(st.tail);
    const bool bad = st.tail[SP_ERR] != 0;
    status[0] = bad ? -1 : st.tail[SP_LAST];
    status[1] = bad ? -1 : st.tail[SP_ROUNDS];
}

// ---- count ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_THREADS)
void sp_flags(unsigned nv, SpState st)
{
    const unsigned i = blockIdx.x * (unsigned)SP_THREADS + threadIdx.x;
    if (i < nv) st.pos[i] = st.keep[i] != 0;
}

__global__ __launch_bounds__(SP_THREADS)
void sp_list(unsigned nv, SpState st)
{
    const unsigned i = blockIdx.x * (unsigned)SP_THREADS + threadIdx.x;
    if (i >= nv || !st.keep[i]) return;
    const unsigned j = (unsigned)st.pos[i];
    if (j >= nv) { atomicOr(st.tail + SP_ERR, 1); return; }
    st.klist[j] = (int)i;
}

// The shoelace terms of the ring as given and of its kept vertices, added up per ring: x1 y0 - x0 y1, north up.
__global__ __launch_bounds__(SP_THREADS)
void sp_areas(const int* __restrict__ vertices, const int* __restrict__ offset, unsigned nr, unsigned nv, SpState st)
{
    const unsigned i = blockIdx.x * (unsigned)SP_THREADS + threadIdx.x;
    int run = -1;
    i64 tin = 0, tout = 0;
    unsigned r, begin, end;
    if (i < nv && st.vring[i] >= 0 && sp_ring_of(st, offset, nr, nv, i, r, begin, end)) {
        int x, y, xn, yn;
        sp_xy(vertices, i, x, y);
        sp_xy(vertices, i + 1 < end ? i + 1 : begin, xn, yn);
        tin = (i64)xn * y - (i64)x * yn;
        if (st.keep[i]) {
            const unsigned nk = (unsigned)max(0, min(st.tail[SP_NKEPT], (int)min(nv, (unsigned)INT_MAX)));
            const unsigned j = (unsigned)st.pos[i];
            unsigned next = j + 1 < nk ? (unsigned)st.klist[j + 1] : end;                // the next kept vertex, of whichever ring
            if (j >= nk || (next <= i && j + 1 < nk)) { atomicOr(st.tail + SP_ERR, 1); next = end; }
            sp_xy(vertices, next < end ? next : begin, xn, yn);
            tout = (i64)xn * y - (i64)x * yn;
        }
        run = (int)r;
    }
    const i64 sin = sp_run_reduce(tin, run, SpAdd()), sout = sp_run_reduce(tout, run, SpAdd());
    if (sp_run_head(run) && run >= 0) {
        atomicAdd((u64*)st.a2in + run, (u64)sin);
        atomicAdd((u64*)st.a2out + run, (u64)sout);
    }
}

// One lane per ring: simplified, or all its vertices back (fewer than 3 kept, no area, or the area's sign turned).
__global__ __launch_bounds__(SP_THREADS)
void sp_rings(const int* __restrict__ offset, unsigned nr, unsigned nv, SpState st)
{
    const unsigned r = blockIdx.x * (unsigned)SP_THREADS + threadIdx.x;
    if (r >= nr) return;
    const unsigned begin = (unsigned)offset[r], end = (unsigned)offset[r + 1];
    st.simp[r] = 0;
    st.rcount[r] = 0;
    if (begin > end || end > nv) return;                     // flag bit 1 of begin
    const unsigned nk = (unsigned)max(0, min(st.tail[SP_NKEPT], (int)min(nv, (unsigned)INT_MAX)));
    const unsigned pb = begin < nv ? (unsigned)st.pos[begin] : nk, pe = end < nv ? (unsigned)st.pos[end] : nk;
    const unsigned m = end - begin, k = pe - pb;
    if (pb > pe || k > m) { atomicOr(st.tail + SP_ERR, 1); st.rcount[r] = (int)m; return; }
    const i64 before = st.a2in[r], after = st.a2out[r];
    const bool ok = k >= 3 && after != 0 && before != 0 && (after > 0) == (before > 0);
    st.simp[r] = ok;
    st.rcount[r] = (int)(ok ? k : m);
}

__global__ void sp_count_out(SpState st, int* __restrict__ n_out)
{
    if (threadIdx.x == 0) *n_out = st.tail[SP_ERR] ? -1 : st.tail[SP_NOUT];
}

// ---- write ---------------------------------------------------------------------------------------------------------------------
struct SpOut { int *offset, *vertices, *kept; i64* area2; unsigned char* simplified; };

__global__ __launch_bounds__(SP_THREADS)
void sp_write_vertices(const int* __restrict__ vertices, const int* __restrict__ offset, unsigned nr, unsigned nv, unsigned n_out, SpState st, SpOut o)
{
    const unsigned i = blockIdx.x * (unsigned)SP_THREADS + threadIdx.x;
    if (i == 0 && (unsigned)st.tail[SP_NOUT] != n_out) atomicOr(st.tail + SP_ERR, 1);
    if (i >= nv || st.vring[i] < 0) return;
    unsigned r, begin, end;
    if (!sp_ring_of(st, offset, nr, nv, i, r, begin, end)) return;
    unsigned at = (unsigned)st.rcount[r];
    if (st.simp[r]) {
        if (!st.keep[i]) return;
        at += (unsigned)st.pos[i] - (unsigned)st.pos[begin];
    } else at += i - begin;
    if (at >= n_out) { atomicOr(st.tail + SP_ERR, 1); return; }
    o.vertices[2 * (size_t)at] = vertices[2 * (size_t)i];
    o.vertices[2 * (size_t)at + 1] = vertices[2 * (size_t)i + 1];
    o.kept[at] = (int)i;
}

__global__ __launch_bounds__(SP_THREADS)
void sp_write_rings(unsigned nr, SpState st, SpOut o)
{
    const unsigned r = blockIdx.x * (unsigned)SP_THREADS + threadIdx.x;
    if (r >= nr) return;
    const bool ok = st.simp[r] != 0;
    o.offset[r] = st.rcount[r];
    o.area2[r] = ok ? st.a2out[r] : st.a2in[r];
    o.simplified[r] = ok;
}

__global__ void sp_finish(SpState st, unsigned nr, unsigned n_out, int* __restrict__ offset)
{
    if (threadIdx.x == 0) offset[nr] = st.tail[SP_ERR] ? -1 : (int)n_out;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct SimplifyWorkspace { size_t tail, s1, s2, anchor, a2in, a2out, rcount, simp, vring, left, right, keep, pos, klist, vkey, kmax, kmin, kdec, bytes; };

static SimplifyWorkspace simplify_workspace(size_t nr, size_t nv)
{
    SimplifyWorkspace w;
    const size_t top = nr > nv ? nr : nv;
    const size_t nb1 = (top + OL_BLOCK - 1) / OL_BLOCK, nb2 = (nb1 + OL_BLOCK - 1) / OL_BLOCK;
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t here = at; at += align256(bytes); return here; };
    w.tail = take(256);
    w.s1 = take(nb1 * 4);
    w.s2 = take(nb2 * 4);
    w.anchor = take(nr * 8); w.a2in = take(nr * 8); w.a2out = take(nr * 8); w.rcount = take(nr * 4); w.simp = take(nr);
    w.vring = take(nv * 4); w.left = take(nv * 4); w.right = take(nv * 4); w.keep = take(nv * 4); w.pos = take(nv * 4); w.klist = take(nv * 4);
    w.vkey = take(nv * 8); w.kmax = take(nv * 8); w.kmin = take(nv * 8); w.kdec = take(nv * 8);
    w.bytes = at;
    return w;
}

static SpState simplify_state(void* workspace, const SimplifyWorkspace& w)
{
    char* base = (char*)workspace;
    SpState st;
    st.tail = (int*)(base + w.tail);
    st.vring = (int*)(base + w.vring); st.left = (int*)(base + w.left); st.right = (int*)(base + w.right); st.keep = (int*)(base + w.keep);
    st.pos = (int*)(base + w.pos); st.klist = (int*)(base + w.klist); st.rcount = (int*)(base + w.rcount);
    st.vkey = (u64*)(base + w.vkey); st.kmax = (u64*)(base + w.kmax); st.kmin = (u64*)(base + w.kmin); st.kdec = (u64*)(base + w.kdec);
    st.anchor = (u64*)(base + w.anchor);
    st.a2in = (i64*)(base + w.a2in); st.a2out = (i64*)(base + w.a2out);
    st.simp = (unsigned char*)(base + w.simp);
    return st;
}

// What the four entries check alike: the counts, the ring table, the workspace, and that no two buffers share a byte.
static int simplify_check(const int* vertices, const int* offset, int n_rings, int n_vertices, const void* workspace, size_t workspace_bytes,
                          const DsmBuf* extra, int n_extra)
{
    if (n_rings < 0 || n_vertices < 0) return fail(SMVS_ERR_ARG, "n_rings and n_vertices must be in 0 .. 2^31 - 1, got %d and %d", n_rings, n_vertices);
    if (n_vertices > 0 && n_rings == 0) return fail(SMVS_ERR_ARG, "vertices without rings (n_rings == 0)");
    if (!workspace || (n_rings > 0 && !offset) || (n_vertices > 0 && !vertices)) return fail(SMVS_ERR_ARG, "null pointer argument");
    const SimplifyWorkspace w = simplify_workspace((size_t)n_rings, (size_t)n_vertices);
    if (workspace_bytes < w.bytes) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, w.bytes);
    DsmBuf buf[9] = {{vertices, (size_t)n_vertices * 8, "vertices"}, {offset, n_rings ? ((size_t)n_rings + 1) * 4 : 0, "offset"}, {workspace, w.bytes, "workspace"}};
    for (int k = 0; k < n_extra; ++k) {
        if (extra[k].bytes && !extra[k].p) return fail(SMVS_ERR_ARG, "null pointer argument");
        buf[3 + k] = extra[k];
    }
    const char* other = nullptr;
    if (const char* name = dsm_first_alias(buf, 3 + n_extra, other)) return fail(SMVS_ERR_ARG, "%s aliases %s", name, other);
    return SMVS_OK;
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT size_t smvs_dsm_simplify_workspace_bytes(int n_rings, int n_vertices)
{
    using namespace smvs;
    if (n_rings < 0 || n_vertices < 0 || (n_vertices > 0 && n_rings == 0)) return 0;
    return simplify_workspace((size_t)n_rings, (size_t)n_vertices).bytes;
}

SMVS_EXPORT int smvs_dsm_simplify_begin(const int* vertices, const int* offset, int n_rings, int n_vertices, int* flag,
                                        void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    const DsmBuf extra[] = {{flag, 4, "flag"}};
    if (!flag) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (int rc = simplify_check(vertices, offset, n_rings, n_vertices, workspace, workspace_bytes, extra, 1)) return rc;
    const SimplifyWorkspace w = simplify_workspace((size_t)n_rings, (size_t)n_vertices);
    const SpState st = simplify_state(workspace, w);
    hipStream_t s = (hipStream_t)stream;
    const size_t nr = (size_t)n_rings, nv = (size_t)n_vertices;
    bool ok = hipMemsetAsync(flag, 0, 4, s) == hipSuccess && hipMemsetAsync(st.tail, 0, 256, s) == hipSuccess;
    if (nr) ok = ok && hipMemsetAsync(st.anchor, 0, w.rcount - w.anchor, s) == hipSuccess;                    // anchor, a2in, a2out
    if (nv) {
        ok = ok && hipMemsetAsync(st.vring, 0xff, w.keep - w.vring, s) == hipSuccess;                         // vring, left, right: none
        ok = ok && hipMemsetAsync(st.keep, 0, nv * 4, s) == hipSuccess;
        ok = ok && hipMemsetAsync(st.kmax, 0, nv * 8, s) == hipSuccess && hipMemsetAsync(st.kmin, 0xff, nv * 8, s) == hipSuccess;
    }
    if (!ok) return check_launch("dsm_simplify_begin (clearing the workspace)");
    if (!nr) return SMVS_OK;
    const unsigned lanes = (unsigned)(nv > nr ? nv : nr);
    DSM_LAUNCH(sp_init, lanes, SP_THREADS, s, vertices, offset, (unsigned)nr, (unsigned)nv, st, flag);
    if (!nv) return SMVS_OK;
    DSM_LAUNCH(sp_segments, nv, SP_THREADS, s, offset, (unsigned)nr, (unsigned)nv, st);
    return SMVS_OK;
}

SMVS_EXPORT int smvs_dsm_simplify_rounds(const int* vertices, const int* offset, int n_rings, int n_vertices, int tol16, int rounds,
                                         int* status, void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    const DsmBuf extra[] = {{status, 8, "status"}};
    if (!status) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (tol16 < 0 || tol16 > SP_MAX_TOL16) return fail(SMVS_ERR_ARG, "tol16 must be in 0 .. %d, got %d", SP_MAX_TOL16, tol16);
    if (rounds < 0 || rounds > SP_MAX_ROUNDS) return fail(SMVS_ERR_ARG, "rounds must be in 0 .. %d, got %d", SP_MAX_ROUNDS, rounds);
    if (int rc = simplify_check(vertices, offset, n_rings, n_vertices, workspace, workspace_bytes, extra, 1)) return rc;
    const SimplifyWorkspace w = simplify_workspace((size_t)n_rings, (size_t)n_vertices);
    const SpState st = simplify_state(workspace, w);
    hipStream_t s = (hipStream_t)stream;
    const unsigned nr = (unsigned)n_rings, nv = (unsigned)n_vertices;
    for (int k = 0; k < rounds && nv; ++k) {
        DSM_LAUNCH(sp_keys, nv, SP_THREADS, s, vertices, offset, nr, nv, st);
        DSM_LAUNCH(sp_pick, nv, SP_THREADS, s, offset, nr, nv, st);
        DSM_LAUNCH(sp_decide, nv, SP_THREADS, s, vertices, offset, nr, nv, (unsigned)tol16, st);
    }
    DSM_LAUNCH(sp_status, 1, 64, s, st, status);
    return SMVS_OK;
}

SMVS_EXPORT int smvs_dsm_simplify_count(const int* vertices, const int* offset, int n_rings, int n_vertices, int* n_out,
                                        void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    const DsmBuf extra[] = {{n_out, 4, "n_out"}};
    if (!n_out) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (int rc = simplify_check(vertices, offset, n_rings, n_vertices, workspace, workspace_bytes, extra, 1)) return rc;
    const SimplifyWorkspace w = simplify_workspace((size_t)n_rings, (size_t)n_vertices);
    const SpState st = simplify_state(workspace, w);
    hipStream_t s = (hipStream_t)stream;
    const unsigned nr = (unsigned)n_rings, nv = (unsigned)n_vertices;
    if (!nr || !nv) {
        if (hipMemsetAsync(n_out, 0, 4, s) != hipSuccess || hipMemsetAsync(st.tail + SP_NOUT, 0, 4, s) != hipSuccess)
            return check_launch("dsm_simplify_count (clearing the count)");
        return SMVS_OK;
    }
    char* base = (char*)workspace;
    int *s1 = (int*)(base + w.s1), *s2 = (int*)(base + w.s2);
    int rc;
    DSM_LAUNCH(sp_flags, nv, SP_THREADS, s, nv, st);
    if ((rc = ol_scan_exclusive(st.pos, nv, nullptr, s1, s2, st.tail + SP_NKEPT, s, "ol_scan (kept vertices)"))) return rc;
    DSM_LAUNCH(sp_list, nv, SP_THREADS, s, nv, st);
    if (hipMemsetAsync(st.a2in, 0, w.rcount - w.a2in, s) != hipSuccess) return check_launch("dsm_simplify_count (clearing the sums)");
    DSM_LAUNCH(sp_areas, nv, SP_THREADS, s, vertices, offset, nr, nv, st);
    DSM_LAUNCH(sp_rings, nr, SP_THREADS, s, offset, nr, nv, st);
    if ((rc = ol_scan_exclusive(st.rcount, nr, nullptr, s1, s2, st.tail + SP_NOUT, s, "ol_scan (rings)"))) return rc;
    DSM_LAUNCH(sp_count_out, 1, 64, s, st, n_out);
    return SMVS_OK;
}

SMVS_EXPORT int smvs_dsm_simplify_write(const int* vertices, const int* offset, int n_rings, int n_vertices, int n_out,
                                        int* out_offset, int* out_vertices, long long* area2, int* kept, unsigned char* simplified,
                                        void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (n_out < 0 || n_out > n_vertices) return fail(SMVS_ERR_ARG, "n_out must be in 0 .. n_vertices = %d, got %d", n_vertices, n_out);
    if (!out_offset) return fail(SMVS_ERR_ARG, "null pointer argument");
    const size_t m = n_rings > 0 ? (size_t)n_rings : 0, k = (size_t)n_out;
    const DsmBuf extra[] = {{out_offset, (m + 1) * 4, "out_offset"}, {out_vertices, k * 8, "out_vertices"}, {area2, m * 8, "area2"},
                           {kept, k * 4, "kept"}, {simplified, m, "simplified"}};
    if (int rc = simplify_check(vertices, offset, n_rings, n_vertices, workspace, workspace_bytes, extra, 5)) return rc;
    const SimplifyWorkspace w = simplify_workspace((size_t)n_rings, (size_t)n_vertices);
    const SpState st = simplify_state(workspace, w);
    hipStream_t s = (hipStream_t)stream;
    const unsigned nr = (unsigned)n_rings, nv = (unsigned)n_vertices;
    if (!nr || !nv) {                                        // no vertex: every ring is empty
        bool ok = hipMemsetAsync(out_offset, 0, (m + 1) * 4, s) == hipSuccess;
        if (m) ok = ok && hipMemsetAsync(area2, 0, m * 8, s) == hipSuccess && hipMemsetAsync(simplified, 0, m, s) == hipSuccess;
        if (!ok) return check_launch("dsm_simplify_write (empty tables)");
        return SMVS_OK;
    }
    const SpOut o = {out_offset, out_vertices, kept, area2, simplified};
    DSM_LAUNCH(sp_write_vertices, nv, SP_THREADS, s, vertices, offset, nr, nv, (unsigned)n_out, st, o);
    DSM_LAUNCH(sp_write_rings, nr, SP_THREADS, s, nr, st, o);
    DSM_LAUNCH(sp_finish, 1, 64, s, st, nr, (unsigned)n_out, out_offset);
    return SMVS_OK;
}

}  // extern "C"
