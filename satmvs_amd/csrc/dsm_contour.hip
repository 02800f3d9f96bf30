// dsm_contour.hip -- the contour lines of a DSM at many levels in one call, as ordered float64 vertex lists: open chains that end
// at voids and at the grid's edge, and closed rings ("Contours"; include/satmvs.h for the rule).
//
//   smvs_dsm_contour_count  dsm (gh, gw) float32 + levels -> n_cross, n_lines, n_vertices on the device, the lines in the workspace
//   smvs_dsm_contour_write  the line table and the vertex list into buffers the caller sized from those counts
//
// A candidate vertex is a crossing (level, lattice edge).  The levels that cross an edge are a contiguous range [lo, hi) of the
// sorted level table, which every workgroup keeps in LDS (at most 16 KB), so a lane per edge finds hi - lo by two binary
// searches, and the exclusive scan of hi - lo over the edges in eid order (three levels of 2048-element blocks, dsm_scan.h)
// numbers the crossings by (eid, level): crossing (K_l, e) has the id base[e] + l - lo[e], and lo[e] is recomputed from the two
// heights wherever it is needed, so the workspace holds 4 bytes per edge and nothing else per edge.
// The link kernel spreads the crossings of the 64 edges of a wave over its 64 lanes (a wave-level scan of the counts, then a
// 6-step search through the lanes per crossing), so an edge at a cliff that carries 4096 crossings costs its wave 64 rounds and
// not one lane 4096.  Every crossing finds its successor from the four corners of the square it enters and writes its own id at
// the successor's place: the predecessor array, which starts full of the sentinel ~0, so a crossing nobody links to keeps it.
// One pointer doubling backwards over the predecessors carries a 64-bit word (key << 32 | steps): key = the crossing's id, with
// bit 31 set iff it has a predecessor, so the start of an open chain is below every other key of its line and the smallest eid
// of a ring is its smallest id (one level per line).  The sentinel stops the window at an open chain's start.  After
// ceil(log2(max_cross)) rounds every crossing knows the id of its line's first vertex and its own rank from it.  Starts are
// numbered by a second scan (id order), sorted stably by level (one split per bit of n_levels - 1, each a scan), the lengths
// (rank of the last vertex of an open chain, of the start's predecessor in a ring, plus one) are scanned into the offsets, and
// every crossing writes its vertex at offset[line] + rank: a 16-byte store per lane, scattered, which is what the write costs.
// Integer atomics only (add, or): the bits do not depend on their order.
//
// Every loop is bounded by a number the host knows.  Every index read from the workspace is checked against its array before it
// is used; one that is out of range sets the error word and the counts come back as -1 (count) or offset[n_lines] as -1 (write).
// The workspace per crossing: three predecessor arrays (12), two doubling words (16), the edge (4), the level (2), the successor
// flag (1), and per two crossings (a line has at least two vertices) six sort and table words (24): 47 bytes; per lattice edge
// 4 bytes (8 per cell); the level table 16 KB; the scan's block sums.
#include <limits.h>
#include <stdint.h>

#include "dsm_chain.h"
#include "dsm_common.h"
#include "smvs_host.h"

namespace smvs {

enum { CT_CAP = 5, CT_SUM64 = 6 };                           // the tail words past dsm_chain.h's five (6, 7: a 64-bit sum)
constexpr int CT_MAX_LEVELS = 4096, CT_CHUNK = 512;

struct CtChunk { int v[CT_CHUNK]; };                         // a piece of the host's level table, passed by value

__device__ __forceinline__ bool ct_node(const float* __restrict__ dsm, size_t i, float nodata, int& q) { return dsm_quantum(dsm[i], nodata, q); }

// The first level above x (x even, the levels odd: never equal).
__device__ __forceinline__ int ct_first_above(const int* lev, int n, int x)
{
    int lo = 0, hi = n;
    for (int step = 0; step < 13 && lo < hi; ++step) {
        const int mid = (lo + hi) >> 1;
        if (lev[mid] > x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// The number of crossings the kernels past the count work on: none if there are more than the caller made room for.
struct CtLimit {
    __device__ __forceinline__ int operator()(const int* tail, unsigned cap) const
    {
        const int v = tail[CH_N];
        return *(const u64*)(tail + CT_SUM64) > (u64)cap || v < 0 || (unsigned)v > cap ? 0 : v;
    }
};

// The two ends of lattice edge e, if it exists and both hold a height: a the end the eid names, b the other.
__device__ __forceinline__ bool ct_edge(const float* __restrict__ dsm, int gw, int gh, float nodata, unsigned e, int& r, int& c, int& o, int& qa, int& qb)
{
    const unsigned cell = e >> 1;
    o = (int)(e & 1u);
    r = (int)(cell / (unsigned)gw);
    c = (int)(cell - (unsigned)r * (unsigned)gw);
    if (o == 0 ? c + 1 >= gw : r + 1 >= gh) return false;
    return ct_node(dsm, cell, nodata, qa) && ct_node(dsm, o == 0 ? (size_t)cell + 1 : (size_t)cell + (size_t)gw, nodata, qb);
}

__device__ __forceinline__ void ct_levels_to_lds(const int* __restrict__ lev, int nl, int* lev_s)
{
    for (int i = threadIdx.x; i < nl; i += OL_THREADS) lev_s[i] = lev[i];
    __syncthreads();
}

// ---- count -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OL_THREADS)
void ct_upload(CtChunk chunk, int at, int n, int* __restrict__ lev)
{
    const int i = blockIdx.x * OL_THREADS + threadIdx.x;
    if (i < n) lev[at + i] = chunk.v[i];
}

// One lane per lattice edge: the number of levels that cross it.
__global__ __launch_bounds__(OL_THREADS)
void ct_edges(const float* __restrict__ dsm, int gw, int gh, float nodata, const int* __restrict__ lev, int nl, unsigned n_edges,
              int* __restrict__ base, int* tail)
{
    __shared__ int lev_s[CT_MAX_LEVELS];
    ct_levels_to_lds(lev, nl, lev_s);
    const unsigned e = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    int cnt = 0;
    if (e < n_edges) {
        int r, c, o, qa, qb;
        if (ct_edge(dsm, gw, gh, nodata, e, r, c, o, qa, qb))
            cnt = ct_first_above(lev_s, nl, 2 * max(qa, qb)) - ct_first_above(lev_s, nl, 2 * min(qa, qb));
        base[e] = cnt;
    }
    int sum = cnt;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd((u64*)(tail + CT_SUM64), (u64)sum);
}

// The crossings must fit an int32 and, past the count-only call, the room the caller made.
__global__ void ct_room(unsigned cap, int* tail)
{
    if (threadIdx.x != 0) return;
    const u64 all = *(const u64*)(tail + CT_SUM64);
    if (all > (u64)INT_MAX || (int)all != tail[CH_N] || (cap > 0 && all > cap)) tail[CH_ERR] = 1;
    tail[CT_CAP] = (int)cap;
}

// One lane per lattice edge for the counts, then the wave's crossings dealt out to its lanes: the edge, the level and the
// successor flag of every crossing, and its id at its successor's place.
__global__ __launch_bounds__(OL_THREADS)
void ct_link(const float* __restrict__ dsm, int gw, int gh, float nodata, const int* __restrict__ lev, int nl, unsigned n_edges,
             const int* __restrict__ base, unsigned cap, int* tail, int* __restrict__ cedge, unsigned short* __restrict__ clev,
             unsigned char* __restrict__ cflag, unsigned* __restrict__ pred)
{
    __shared__ int lev_s[CT_MAX_LEVELS];
    ct_levels_to_lds(lev, nl, lev_s);
    const unsigned nc = (unsigned)CtLimit()(tail, cap);       // the same for every lane: no kernel of this launch writes these words
    if (nc == 0) return;                                     // more crossings than room: nothing is written
    const unsigned e = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int cnt = 0, lo = 0;
    unsigned b0 = 0;
    if (e < n_edges) {
        int r, c, o, qa, qb;
        if (ct_edge(dsm, gw, gh, nodata, e, r, c, o, qa, qb)) {
            lo = ct_first_above(lev_s, nl, 2 * min(qa, qb));
            cnt = ct_first_above(lev_s, nl, 2 * max(qa, qb)) - lo;
        }
        b0 = (unsigned)base[e];
        if (cnt && (b0 > nc || (unsigned)cnt > nc - b0)) { atomicOr(tail + CH_ERR, 1); cnt = 0; }
    }
    int inc = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(inc, d);
        if (lane >= d) inc += up;
    }
    const int total = __shfl(inc, 63);
    const unsigned e_wave = e - (unsigned)lane;
    for (int i0 = 0; i0 < total; i0 += 64) {                 // at most 64 rounds of 64 crossings: 4096 levels on every edge
        const int i = min(i0 + lane, total - 1);
        int k = 0;                                           // the owner: the first lane whose inclusive count is above i
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1)
            if (__shfl(inc, k + step - 1) <= i) k += step;
        const int within = i - (__shfl(inc, k) - __shfl(cnt, k));
        const int l = __shfl(lo, k) + within;
        const unsigned id = __shfl(b0, k) + (unsigned)within;
        if (i0 + lane >= total) continue;
        const unsigned ek = e_wave + (unsigned)k;
        int r, c, o, qa, qb;
        if (id >= nc || ek >= n_edges || !ct_edge(dsm, gw, gh, nodata, ek, r, c, o, qa, qb) || (unsigned)l >= (unsigned)nl) { atomicOr(tail + CH_ERR, 1); continue; }
        const int K = lev_s[l];
        const bool a_above = 2 * qa > K;
        // H the end above, L the other; the line passes with H on its left, so it heads from the edge by (dr, dc)
        const int br = o == 0 ? r : r + 1, bc = o == 0 ? c + 1 : c;
        const int hr = a_above ? r : br, hc = a_above ? c : bc, lr = a_above ? br : r, lc = a_above ? bc : c;
        const int qh = a_above ? qa : qb, ql = a_above ? qb : qa;
        const int dr = o == 0 ? (a_above ? -1 : 1) : 0, dc = o == 1 ? (a_above ? 1 : -1) : 0;
        const int h2r = hr + dr, h2c = hc + dc, l2r = lr + dr, l2c = lc + dc;
        int qh2 = 0, ql2 = 0;
        bool succ = (unsigned)h2r < (unsigned)gh && (unsigned)h2c < (unsigned)gw;      // L' is on the lattice with H'
        if (succ) succ = ct_node(dsm, (size_t)h2r * gw + h2c, nodata, qh2) && ct_node(dsm, (size_t)l2r * gw + l2c, nodata, ql2);
        if (succ) {
            const bool h2_above = 2 * qh2 > K, l2_above = 2 * ql2 > K;
            int way;                                         // 0 left (H - H'), 1 straight (H' - L'), 2 right (L - L')
            if (!h2_above) way = l2_above && qh + ql + qh2 + ql2 > 2 * K ? 2 : 0;
            else way = l2_above ? 2 : 1;
            const int pr = way == 2 ? lr : way == 1 ? h2r : hr, pc = way == 2 ? lc : way == 1 ? h2c : hc;
            const int sr = way == 0 ? h2r : l2r, sc = way == 0 ? h2c : l2c;
            const int qp = way == 2 ? ql : way == 1 ? qh2 : qh, qs = way == 0 ? qh2 : ql2;
            const unsigned e2 = 2u * ((unsigned)min(pr, sr) * (unsigned)gw + (unsigned)min(pc, sc)) + (pr != sr ? 1u : 0u);
            const int lo2 = ct_first_above(lev_s, nl, 2 * min(qp, qs));
            const unsigned id2 = (unsigned)base[e2] + (unsigned)(l - lo2);
            if (l < lo2 || id2 >= nc) { atomicOr(tail + CH_ERR, 1); succ = false; }
            else pred[id2] = id;
        }
        cedge[id] = (int)ek;
        clev[id] = (unsigned short)l;
        cflag[id] = succ ? 1 : 0;
    }
}

// The first doubling word: the crossing's id, bit 31 set iff somebody linked to it; 0 steps.
__global__ __launch_bounds__(OL_THREADS)
void ct_init(const unsigned* __restrict__ pred, u64* __restrict__ val, unsigned cap, const int* tail)
{
    const unsigned j = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    if (j >= (unsigned)CtLimit()(tail, cap)) return;
    val[j] = (u64)(j | (pred[j] != CH_NONE ? 0x80000000u : 0u)) << 32;
}

// What a crossing is after the doubling: 0 dropped (neither predecessor nor successor), 1 inside a line, 2 its first vertex,
// 3 the last vertex of an open chain (2 | 1 cannot happen: a line has two vertices).
__device__ __forceinline__ int ct_role(u64 v, unsigned p0, int has_succ)
{
    if (p0 == CH_NONE && !has_succ) return 0;
    if ((unsigned)v == 0u) return 2;
    return has_succ ? 1 : 3;
}

// Starts flagged for the scan that numbers the lines; the vertices counted; an open chain's length left at its start.
__global__ __launch_bounds__(OL_THREADS)
void ct_starts(const u64* __restrict__ val, const unsigned* __restrict__ pred0, const unsigned char* __restrict__ cflag,
               int* __restrict__ lscan, int* __restrict__ llen, unsigned cap, int* tail)
{
    const unsigned j = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    const unsigned nc = (unsigned)CtLimit()(tail, cap);
    bool vertex = false;
    if (j < nc) {
        const u64 v = val[j];
        const int role = ct_role(v, pred0[j], cflag[j] & 1);
        vertex = role != 0;
        lscan[j] = role == 2;
        if (role == 3) {
            const unsigned start = (unsigned)(v >> 32) & 0x7fffffffu;
            if (start >= nc) atomicOr(tail + CH_ERR, 1);
            else llen[start] = (int)((unsigned)v + 1u);
        }
    }
    const int cnt = __popcll(__ballot(vertex));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(tail + CH_VERTICES, cnt);
}

// ---- write -------------------------------------------------------------------------------------------------------------------
// The counts the caller sized its buffers from must be the ones the workspace holds; every start hands its level and itself to
// the sort, at its number in id order.
__global__ __launch_bounds__(OL_THREADS)
void ct_line_init(const u64* __restrict__ val, const unsigned* __restrict__ pred0, const unsigned char* __restrict__ cflag,
                  const unsigned short* __restrict__ clev, const int* __restrict__ lscan, unsigned nc, unsigned nl, unsigned nv, int n_levels,
                  int* tail, int* __restrict__ skey, int* __restrict__ sval)
{
    const unsigned j = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    if (j == 0 && ((unsigned)tail[CH_N] != nc || (unsigned)tail[CH_LINES] != nl || (unsigned)tail[CH_VERTICES] != nv || (unsigned)tail[CT_CAP] != nc))
        atomicOr(tail + CH_ERR, 1);                          // the layout of the workspace follows max_cross: it must have been n_cross
    if (j >= nc || ct_role(val[j], pred0[j], cflag[j] & 1) != 2) return;
    const unsigned q = (unsigned)lscan[j], l = clev[j];
    if (q >= nl || l >= (unsigned)n_levels) { atomicOr(tail + CH_ERR, 1); return; }
    skey[q] = (int)l;
    sval[q] = (int)j;
}

// One lane per line in its final place: its level, whether it is closed, its length, and its place written where its
// crossings find it: at its start's id.
__global__ __launch_bounds__(OL_THREADS)
void ct_line_table(const int* __restrict__ skey, const int* __restrict__ sval, const u64* __restrict__ val, const unsigned* __restrict__ pred0,
                   const int* __restrict__ llen, int* __restrict__ lline, int* __restrict__ ebase, unsigned nc, unsigned nl, unsigned nv,
                   int* tail, int* __restrict__ line_level, unsigned char* __restrict__ line_closed)
{
    const unsigned r = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    if (r >= nl) return;
    line_level[r] = skey[r];
    const unsigned j0 = (unsigned)sval[r];
    unsigned len = 0;
    bool closed = false;
    if (j0 >= nc) atomicOr(tail + CH_ERR, 1);
    else {
        lline[j0] = (int)r;
        const unsigned p = pred0[j0];
        closed = p != CH_NONE;
        if (!closed) len = (unsigned)llen[j0];
        else if (p >= nc) atomicOr(tail + CH_ERR, 1);
        else len = (unsigned)val[p] + 1u;
        if (len < 2 || len > nv) { atomicOr(tail + CH_ERR, 1); len = 0; }
    }
    line_closed[r] = closed ? 1 : 0;
    ebase[r] = (int)len;
}

// Every crossing of a line: its vertex at (offset of its line + its rank).
__global__ __launch_bounds__(OL_THREADS)
void ct_vertices(const float* __restrict__ dsm, int gw, int gh, float nodata, const int* __restrict__ lev, int n_levels, unsigned n_edges,
                 const u64* __restrict__ val, const unsigned* __restrict__ pred0, const unsigned char* __restrict__ cflag,
                 const int* __restrict__ cedge, const unsigned short* __restrict__ clev, const int* __restrict__ lline,
                 const int* __restrict__ ebase, unsigned nc, unsigned nl, unsigned nv, int* tail,
                 double* __restrict__ vertices, int* __restrict__ vertex_edge)
{
    const unsigned j = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    if (j >= nc) return;
    const u64 v = val[j];
    if (ct_role(v, pred0[j], cflag[j] & 1) == 0) return;
    const unsigned start = (unsigned)(v >> 32) & 0x7fffffffu, rank = (unsigned)v;
    const unsigned line = start < nc ? (unsigned)lline[start] : nl;
    const unsigned at = line < nl ? (unsigned)ebase[line] + rank : nv;
    const unsigned e = (unsigned)cedge[j], l = clev[j];
    int r, c, o, qa, qb;
    if (line >= nl || at >= nv || at < rank || e >= n_edges || l >= (unsigned)n_levels || !ct_edge(dsm, gw, gh, nodata, e, r, c, o, qa, qb) || qa == qb) {
        atomicOr(tail + CH_ERR, 1);
        return;
    }
    const double t = __ddiv_rn((double)(lev[l] - 2 * qa), (double)(2 * qb - 2 * qa));
    vertices[2 * (size_t)at] = o == 0 ? __dadd_rn((double)c, t) : (double)c;
    vertices[2 * (size_t)at + 1] = o == 0 ? (double)r : __dadd_rn((double)r, t);
    if (vertex_edge) vertex_edge[at] = (int)e;
}

__global__ __launch_bounds__(OL_THREADS)
void ct_offsets(const int* __restrict__ ebase, unsigned nl, unsigned nv, int* tail, int* __restrict__ offset)
{
    const unsigned r = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    if (r == 0 && (unsigned)tail[CH_TOTAL] != nv) atomicOr(tail + CH_ERR, 1);
    if (r < nl) offset[r] = ebase[r];
}

__global__ void ct_finish(const int* __restrict__ tail, unsigned nl, unsigned nv, int* __restrict__ offset)
{
    if (threadIdx.x == 0) offset[nl] = tail[CH_ERR] ? -1 : (int)nv;
}

// ---- host --------------------------------------------------------------------------------------------------------------------
struct ContourWorkspace {
    size_t tail, s1, s2, lev, base, pred0, preda, predb, vala, valb, cedge, clev, cflag, skeya, skeyb, svala, svalb, spos, ebase, bytes;
    unsigned n_edges;
};

static ContourWorkspace contour_workspace(int gw, int gh, size_t max_cross)
{
    ContourWorkspace w;
    const size_t ne = 2 * (size_t)gw * (size_t)gh, top = ne > max_cross ? ne : max_cross, x = max_cross, half = max_cross / 2 + 1;
    const size_t nb1 = (top + OL_BLOCK - 1) / OL_BLOCK, nb2 = (nb1 + OL_BLOCK - 1) / OL_BLOCK;
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t here = at; at += align256(bytes); return here; };
    w.n_edges = (unsigned)ne;
    w.tail = take(256);
    w.s1 = take(nb1 * 4);
    w.s2 = take(nb2 * 4);
    w.lev = take((size_t)CT_MAX_LEVELS * 4);
    w.base = take(ne * 4);
    w.pred0 = take(x * 4); w.preda = take(x * 4); w.predb = take(x * 4);
    w.vala = take(x * 8); w.valb = take(x * 8);
    w.cedge = take(x * 4); w.clev = take(x * 2); w.cflag = take(x);
    w.skeya = take(half * 4); w.skeyb = take(half * 4); w.svala = take(half * 4); w.svalb = take(half * 4); w.spos = take(half * 4);
    w.ebase = take(half * 4);
    w.bytes = at;
    return w;
}

static const char* contour_check(int gw, int gh, int n_levels, long long max_cross)
{
    if (gw < 1 || gh < 1) return "non-positive grid size";
    if ((long long)gw * gh >= (1ll << 29)) return "grid too large: gw * gh must be below 2^29 cells";
    if (n_levels < 1 || n_levels > CT_MAX_LEVELS) return "n_levels must be 1 .. 4096";
    if (max_cross < 0 || max_cross > (long long)INT_MAX) return "max_cross must be in 0 .. 2^31 - 1";
    return nullptr;
}

static const char* levels_check(const int* levels, int n_levels)
{
    for (int k = 0; k < n_levels; ++k) {
        if (!(levels[k] & 1)) return "levels must be odd (units of 2^-9 m: no node lies on a level)";
        if (levels[k] <= -(1 << 25) || levels[k] >= (1 << 25)) return "levels must be below 2^25 in magnitude";
        if (k && levels[k] <= levels[k - 1]) return "levels must rise strictly";
    }
    return nullptr;
}

// The host's level table into the workspace, 512 levels a launch through the kernel arguments: no copy from pageable memory.
static int contour_upload(const int* levels, int n_levels, int* lev, hipStream_t s)
{
    for (int at = 0; at < n_levels; at += CT_CHUNK) {
        CtChunk chunk;
        const int n = n_levels - at < CT_CHUNK ? n_levels - at : CT_CHUNK;
        for (int i = 0; i < CT_CHUNK; ++i) chunk.v[i] = i < n ? levels[at + i] : 0;
        DSM_LAUNCH(ct_upload, CT_CHUNK, OL_THREADS, s, chunk, at, n, lev);
    }
    return SMVS_OK;
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT size_t smvs_dsm_contour_workspace_bytes(int gw, int gh, int n_levels, int max_cross)
{
    using namespace smvs;
    if (contour_check(gw, gh, n_levels, max_cross)) return 0;
    return contour_workspace(gw, gh, (size_t)max_cross).bytes;
}

SMVS_EXPORT int smvs_dsm_contour_count(const float* dsm, int gw, int gh, float nodata, const int* levels, int n_levels, int max_cross,
                                       int* counts, void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!dsm || !levels || !counts || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = contour_check(gw, gh, n_levels, max_cross)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (const char* msg = levels_check(levels, n_levels)) return fail(SMVS_ERR_ARG, "%s", msg);
    const ContourWorkspace w = contour_workspace(gw, gh, (size_t)max_cross);
    if (workspace_bytes < w.bytes) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, w.bytes);
    const DsmBuf buf[] = {{dsm, (size_t)gw * gh * 4, "dsm"}, {counts, 12, "counts"}, {workspace, w.bytes, "workspace"}};
    const char* other = nullptr;
    if (const char* name = dsm_first_alias(buf, 3, other)) return fail(SMVS_ERR_ARG, "%s aliases %s", name, other);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int *tail = (int*)(ws + w.tail), *s1 = (int*)(ws + w.s1), *s2 = (int*)(ws + w.s2), *lev = (int*)(ws + w.lev), *base = (int*)(ws + w.base);
    if (hipMemsetAsync(tail, 0, 256, s) != hipSuccess) return check_launch("dsm_contour_count (clearing the counts)");
    int rc;
    if ((rc = contour_upload(levels, n_levels, lev, s))) return rc;
    const unsigned cap = (unsigned)max_cross;
    DSM_LAUNCH(ct_edges, w.n_edges, OL_THREADS, s, dsm, gw, gh, nodata, (const int*)lev, n_levels, w.n_edges, base, tail);
    if ((rc = ol_scan_exclusive(base, w.n_edges, nullptr, s1, s2, tail + CH_N, s, "ol_scan (crossings)"))) return rc;
    DSM_LAUNCH(ct_room, 1, 64, s, cap, tail);
    if (max_cross > 0) {
        unsigned* pred[3] = {(unsigned*)(ws + w.pred0), (unsigned*)(ws + w.preda), (unsigned*)(ws + w.predb)};
        u64* val[2] = {(u64*)(ws + w.vala), (u64*)(ws + w.valb)};
        int* cedge = (int*)(ws + w.cedge);
        unsigned short* clev = (unsigned short*)(ws + w.clev);
        unsigned char* cflag = (unsigned char*)(ws + w.cflag);
        if (hipMemsetAsync(pred[0], 0xff, (size_t)cap * 4, s) != hipSuccess) return check_launch("dsm_contour_count (clearing the predecessors)");
        DSM_LAUNCH(ct_link, w.n_edges, OL_THREADS, s, dsm, gw, gh, nodata, (const int*)lev, n_levels, w.n_edges, (const int*)base, cap, tail,
                   cedge, clev, cflag, pred[0]);
        DSM_LAUNCH(ct_init, cap, OL_THREADS, s, (const unsigned*)pred[0], val[0], cap, (const int*)tail);
        int at;
        if ((rc = chain_order<true, CtLimit>(pred, val, cap, tail, s, &at))) return rc;
        // the two later predecessor arrays have done their work: the start flags and the open chains' lengths live there
        int *lscan = (int*)pred[1], *llen = (int*)pred[2];
        DSM_LAUNCH(ct_starts, cap, OL_THREADS, s, (const u64*)val[at], (const unsigned*)pred[0], (const unsigned char*)cflag, lscan, llen, cap, tail);
        if ((rc = ol_scan_exclusive(lscan, cap, tail + CH_N, s1, s2, tail + CH_LINES, s, "ol_scan (lines)"))) return rc;
    }
    DSM_LAUNCH(chain_counts_out, 1, 64, s, (const int*)tail, counts);
    return SMVS_OK;
}

SMVS_EXPORT int smvs_dsm_contour_write(const float* dsm, int gw, int gh, float nodata, const int* levels, int n_levels,
                                       int n_cross, int n_lines, int n_vertices, int* line_level, unsigned char* line_closed,
                                       int* offset, int* first_line, double* vertices, int* vertex_edge,
                                       void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!dsm || !levels || !offset || !first_line || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = contour_check(gw, gh, n_levels, n_cross)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (const char* msg = levels_check(levels, n_levels)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (n_lines < 0 || n_vertices < 0 || n_vertices > n_cross || 2ll * n_lines > n_vertices || (n_lines > 0) != (n_vertices > 0))
        return fail(SMVS_ERR_ARG, "n_lines (%d) and n_vertices (%d) must be both 0, or 2 n_lines <= n_vertices <= n_cross (%d)", n_lines, n_vertices, n_cross);
    if (n_lines > 0 && (!line_level || !line_closed || !vertices)) return fail(SMVS_ERR_ARG, "null pointer argument");
    const ContourWorkspace w = contour_workspace(gw, gh, (size_t)n_cross);
    if (workspace_bytes < w.bytes) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, w.bytes);
    const size_t m = (size_t)n_lines, nvb = (size_t)n_vertices;
    const DsmBuf buf[] = {{dsm, (size_t)gw * gh * 4, "dsm"}, {workspace, w.bytes, "workspace"}, {line_level, m * 4, "line_level"},
                         {line_closed, m, "line_closed"}, {offset, (m + 1) * 4, "offset"}, {first_line, ((size_t)n_levels + 1) * 4, "first_line"},
                         {vertices, nvb * 16, "vertices"}, {vertex_edge, nvb * 4, "vertex_edge"}};
    const char* other = nullptr;
    if (const char* name = dsm_first_alias(buf, 8, other)) return fail(SMVS_ERR_ARG, "%s aliases %s", name, other);
    hipStream_t s = (hipStream_t)stream;
    if (n_lines == 0) {                                      // no line: the two tables that still have entries
        if (hipMemsetAsync(first_line, 0, ((size_t)n_levels + 1) * 4, s) != hipSuccess || hipMemsetAsync(offset, 0, 4, s) != hipSuccess)
            return check_launch("dsm_contour_write (empty tables)");
        return SMVS_OK;
    }
    char* ws = (char*)workspace;
    int *tail = (int*)(ws + w.tail), *s1 = (int*)(ws + w.s1), *s2 = (int*)(ws + w.s2), *lev = (int*)(ws + w.lev);
    const int rounds = chain_rounds((unsigned)n_cross);
    const u64* val = (const u64*)(ws + (rounds % 2 ? w.valb : w.vala));
    int* lline = (int*)(ws + (rounds % 2 ? w.vala : w.valb));                // the doubling word that does not hold the result
    const unsigned* pred0 = (const unsigned*)(ws + w.pred0);
    const int *lscan = (const int*)(ws + w.preda), *llen = (const int*)(ws + w.predb), *cedge = (const int*)(ws + w.cedge);
    const unsigned short* clev = (const unsigned short*)(ws + w.clev);
    const unsigned char* cflag = (const unsigned char*)(ws + w.cflag);
    int *skey[2] = {(int*)(ws + w.skeya), (int*)(ws + w.skeyb)}, *sval[2] = {(int*)(ws + w.svala), (int*)(ws + w.svalb)};
    int *spos = (int*)(ws + w.spos), *ebase = (int*)(ws + w.ebase);
    const unsigned nc = (unsigned)n_cross, nl = (unsigned)n_lines, nv = (unsigned)n_vertices;
    int rc;
    if ((rc = contour_upload(levels, n_levels, lev, s))) return rc;
    DSM_LAUNCH(ct_line_init, nc, OL_THREADS, s, val, pred0, cflag, clev, lscan, nc, nl, nv, n_levels, tail, skey[0], sval[0]);
    int bits = 0, at;
    while (bits < 12 && ((unsigned)(n_levels - 1) >> bits)) ++bits;
    if ((rc = chain_sort(skey, sval, spos, nl, bits, s1, s2, tail, s, &at))) return rc;
    const int *keys = skey[at], *starts = sval[at];
    DSM_LAUNCH(ct_line_table, nl, OL_THREADS, s, keys, starts, val, pred0, llen, lline, ebase, nc, nl, nv, tail, line_level, line_closed);
    DSM_LAUNCH(chain_first, (size_t)n_levels + 1, OL_THREADS, s, keys, nl, n_levels, 0u, first_line);    // entry n_levels is n_lines
    if ((rc = ol_scan_exclusive(ebase, nl, nullptr, s1, s2, tail + CH_TOTAL, s, "ol_scan (line lengths)"))) return rc;
    DSM_LAUNCH(ct_vertices, nc, OL_THREADS, s, dsm, gw, gh, nodata, (const int*)lev, n_levels, w.n_edges, val, pred0, cflag, cedge, clev,
               (const int*)lline, (const int*)ebase, nc, nl, nv, tail, vertices, vertex_edge);
    DSM_LAUNCH(ct_offsets, nl, OL_THREADS, s, (const int*)ebase, nl, nv, tail, offset);
    DSM_LAUNCH(ct_finish, 1, 64, s, (const int*)tail, nl, nv, offset);
    return SMVS_OK;
}

}  // extern "C"
