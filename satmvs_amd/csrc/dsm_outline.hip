// dsm_outline.hip -- the outlines of the labels of a label map as oriented rings of lattice corners, and rings burnt back
// into a label map ("Outlines"; include/satmvs.h for the rules).
//
//   smvs_dsm_outline_count  labels (gh, gw) int32 -> n_edges, n_rings, n_vertices on the device, the rings in the workspace
//   smvs_dsm_outline_write  the ring table and the vertex list into buffers the caller sized from those counts
//   smvs_dsm_burn           rings -> labels (gh, gw) int32 by the even-odd rule at cell centres
//   smvs_dsm_burn_polygons  the same for rings whose edges have any direction
//
// A boundary edge leaves exactly one lattice corner (its tail) with one of four headings, so the edges are kept per corner: a
// lane per corner builds the 4-bit mask of the edges that leave it (bit s = the edge on side s of its own cell), and an
// exclusive scan of the masks' bit counts (three levels of 2048-element blocks, dsm_scan.h) numbers the edges in the
// order (tail corner y, x, side).  The successor of an edge leaves the corner the edge arrives at and is chosen there, right
// first, from the two cells ahead; every edge writes its own number at its successor's place, which gives the predecessor
// array: a permutation of the edges whose cycles are the rings.
// One pointer doubling over the predecessors carries a 64-bit word (key << 32 | steps): key = 2 * tail corner + (side == 0),
// steps = how many edges back the lowest key of the window stands.  After ceil(log2(n_edges)) rounds the window of every edge
// covers its whole ring, so the word holds the ring's lowest key (the ring's name: its start corner and whether it is a hole)
// and the edge's rank from the start edge.  The lowest corner of a ring is passed once, so the name is unique and the start
// edge is the one edge of the ring with 0 steps.  Start edges are numbered by a second scan (corner order), sorted stably by
// label (one split per bit of n, each a scan), every edge goes to (first edge of its ring + rank), and a last scan over the
// edges in that order numbers the vertices (the edges whose predecessor has another side).
// Integer atomics only (add, xor): the bits do not depend on their order.
//
// Every loop is bounded by a number the host knows: the doubling runs ceil(log2(max_edges)) rounds, the sort one split per bit
// of n, the burn at most gh rows per edge.  Every index read from the workspace is checked against its array before it is
// used; one that is out of range (a damaged workspace) sets the error word, the lane goes on with its own index, and the
// counts come back as -1 (smvs_dsm_outline_count) or offset[n_rings] as -1 (smvs_dsm_outline_write).
#include <limits.h>
#include <stdint.h>

#include "dsm_chain.h"
#include "dsm_common.h"
#include "smvs_host.h"

namespace smvs {

__device__ __forceinline__ int ol_label(const int* __restrict__ L, int gw, int gh, int n, int x, int y)
{
    if ((unsigned)x >= (unsigned)gw || (unsigned)y >= (unsigned)gh) return 0;
    const int v = L[(size_t)y * gw + x];
    return (unsigned)v - 1u < (unsigned)n ? v : 0;
}

// The cell whose side s leaves corner (x, y): s = 0 south side of NE, 1 east side of NW, 2 north side of SW, 3 west side of SE.
__device__ __forceinline__ void ol_cell_of(int x, int y, int s, int& cx, int& cy)
{
    cx = (s == 0 || s == 3) ? x : x - 1;
    cy = (s == 2 || s == 3) ? y : y - 1;
}

// The number of edges the kernels past the count work on: no more than the caller made room for.
struct OlLimit {
    __device__ __forceinline__ int operator()(const int* tail, unsigned cap) const
    {
        const int v = tail[CH_N];
        return v < 0 ? 0 : (unsigned)v > cap ? (int)cap : v;
    }
};

// ---- count -------------------------------------------------------------------------------------------------------------------
// One lane per corner: the mask of the edges that leave it and their number.
__global__ __launch_bounds__(OL_THREADS)
void ol_corners(const int* __restrict__ L, int gw, int gh, int n, unsigned nc, unsigned char* __restrict__ cmask, int* __restrict__ cbase)
{
    const unsigned t = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    if (t >= nc) return;
    const int x = (int)(t % (unsigned)(gw + 1)), y = (int)(t / (unsigned)(gw + 1));
    const int nw = ol_label(L, gw, gh, n, x - 1, y - 1), ne = ol_label(L, gw, gh, n, x, y - 1);
    const int sw = ol_label(L, gw, gh, n, x - 1, y), se = ol_label(L, gw, gh, n, x, y);
    const int m = (ne != 0 && se != ne ? 1 : 0) | (nw != 0 && ne != nw ? 2 : 0) | (sw != 0 && nw != sw ? 4 : 0) | (se != 0 && sw != se ? 8 : 0);
    cmask[t] = (unsigned char)m;
    cbase[t] = __popc(m);
}

// One lane per corner, every edge that leaves it: its tail, its first doubling word, and its number at its successor's place.
__global__ __launch_bounds__(OL_THREADS)
void ol_edges(const int* __restrict__ L, int gw, int gh, int n, unsigned nc, const unsigned char* __restrict__ cmask,
              const int* __restrict__ cbase, unsigned cap, int* tail, int* __restrict__ ecorner, u64* __restrict__ val,
              unsigned* __restrict__ pred, unsigned char* __restrict__ eside)
{
    const unsigned t = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    if (t >= nc) return;
    if (tail[CH_N] < 0 || (unsigned)tail[CH_N] > cap) {    // more edges than the caller made room for
        if (t == 0) atomicOr(tail + CH_ERR, 1);
        return;
    }
    const unsigned ne = (unsigned)tail[CH_N];
    const int m = cmask[t];
    if (!m) return;
    const int x = (int)(t % (unsigned)(gw + 1)), y = (int)(t / (unsigned)(gw + 1));
    const int hx[4] = {1, 0, -1, 0}, hy[4] = {0, -1, 0, 1};  // the heading of side s; the way out across side s is heading (s + 3) % 4
    unsigned j = (unsigned)cbase[t];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if (!((m >> s) & 1)) continue;
        int ax, ay;
        ol_cell_of(x, y, s, ax, ay);
        const int k = ol_label(L, gw, gh, n, ax, ay);
        const int bx = ax + hx[s], by = ay + hy[s], cx = bx + hx[(s + 3) & 3], cy = by + hy[(s + 3) & 3];
        int s2 = (s + 1) & 3;                                // left, on the cell itself
        if (ol_label(L, gw, gh, n, cx, cy) == k) s2 = (s + 3) & 3;           // right first, on the cell diagonally ahead
        else if (ol_label(L, gw, gh, n, bx, by) == k) s2 = s;                // straight on, on the cell ahead
        const unsigned h = (unsigned)((y + hy[s]) * (gw + 1) + x + hx[s]);   // the corner the edge arrives at: on the lattice
        const int hm = cmask[h];
        const unsigned j2 = (unsigned)cbase[h] + (unsigned)__popc(hm & ((1 << s2) - 1));
        if (j >= ne || j2 >= ne || !((hm >> s2) & 1)) {
            atomicOr(tail + CH_ERR, 1);
        } else {
            ecorner[j] = (int)t;
            val[j] = (u64)(2u * t + (s == 0 ? 1u : 0u)) << 32;
            pred[j2] = j;
            eside[j2] = (unsigned char)(s2 | (s2 != s ? 4 : 0));
        }
        ++j;
    }
}

// Start edges flagged for the scan that numbers the rings; the vertices counted.
__global__ __launch_bounds__(OL_THREADS)
void ol_starts(const u64* __restrict__ val, const unsigned char* __restrict__ eside, int* __restrict__ rscan, unsigned cap, int* tail)
{
    const unsigned j = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    const unsigned ne = (unsigned)OlLimit()(tail, cap);
    bool turn = false;
    if (j < ne) {
        rscan[j] = (unsigned)val[j] == 0u;
        turn = (eside[j] & 4) != 0;
    }
    const int cnt = __popcll(__ballot(turn));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(tail + CH_VERTICES, cnt);
}

// ---- write -------------------------------------------------------------------------------------------------------------------
struct OlRings { int *label, *edges; long long* area2; };   // the per-ring outputs the kernels write through one argument

// The counts the caller sized its buffers from must be the ones the workspace holds; every start edge hands its label and
// itself to the sort, at its number in corner order.
__global__ __launch_bounds__(OL_THREADS)
void ol_ring_init(const int* __restrict__ L, int gw, int gh, int n, const u64* __restrict__ val, const int* __restrict__ rscan,
                  const int* __restrict__ ecorner, const unsigned char* __restrict__ eside, unsigned ne, unsigned nr, unsigned nv,
                  unsigned nc, int* tail, int* __restrict__ skey, int* __restrict__ sval)
{
    const unsigned j = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    if (j == 0 && ((unsigned)tail[CH_N] != ne || (unsigned)tail[CH_LINES] != nr || (unsigned)tail[CH_VERTICES] != nv)) atomicOr(tail + CH_ERR, 1);
    if (j >= ne || (unsigned)val[j] != 0u) return;
    const unsigned q = (unsigned)rscan[j], t = (unsigned)ecorner[j];
    if (q >= nr || t >= nc) { atomicOr(tail + CH_ERR, 1); return; }
    int ax, ay;
    ol_cell_of((int)(t % (unsigned)(gw + 1)), (int)(t / (unsigned)(gw + 1)), eside[j] & 3, ax, ay);
    skey[q] = ol_label(L, gw, gh, n, ax, ay);
    sval[q] = (int)j;
}

// One lane per ring in its final place: its label, its length (the rank of the start edge's predecessor + 1), zeroed sums,
// and its place written where the edges find it: at its start edge.
__global__ __launch_bounds__(OL_THREADS)
void ol_ring_table(const int* __restrict__ skey, const int* __restrict__ sval, const u64* __restrict__ val, const unsigned* __restrict__ pred,
                   int* __restrict__ rscan, int* __restrict__ ebase, unsigned ne, unsigned nr, int* tail, OlRings o)
{
    const unsigned r = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    if (r >= nr) return;
    o.label[r] = skey[r];
    o.area2[r] = 0;
    o.edges[2 * r] = 0;
    o.edges[2 * r + 1] = 0;
    const unsigned j0 = (unsigned)sval[r];
    unsigned len = 1;
    if (j0 >= ne) atomicOr(tail + CH_ERR, 1);
    else {
        rscan[j0] = (int)r;
        const unsigned p = pred[j0];
        if (p >= ne) atomicOr(tail + CH_ERR, 1);
        else len = (unsigned)val[p] + 1u;
        if (len > ne) { atomicOr(tail + CH_ERR, 1); len = 1; }
    }
    ebase[r] = (int)len;
}

// Every edge to its place in (ring, rank) order, and its share of the ring's sums.  The lanes of a wave that belong to one
// ring add up among themselves first, so a ring of a million edges does not mean a million atomics on one word.
__global__ __launch_bounds__(OL_THREADS)
void ol_place(int gw, const u64* __restrict__ val, const int* __restrict__ ecorner, const unsigned char* __restrict__ eside,
              const unsigned char* __restrict__ cmask, const int* __restrict__ cbase, const int* __restrict__ rscan,
              const int* __restrict__ ebase, unsigned ne, unsigned nr, unsigned nc, int* tail,
              int* __restrict__ ocorner, int* __restrict__ vpos, OlRings o)
{
    const unsigned j = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    bool live = j < ne;
    unsigned r = 0;
    long long term = 0;
    int counts = 0;
    if (live) {
        const u64 v = val[j];
        const unsigned key = (unsigned)(v >> 32), rank = (unsigned)v, t0 = key >> 1;
        live = false;
        if (t0 >= nc) atomicOr(tail + CH_ERR, 1);
        else {
            const unsigned j0 = (unsigned)cbase[t0] + (unsigned)__popc(cmask[t0] & ((key & 1u) ? 0 : 7));
            r = j0 < ne ? (unsigned)rscan[j0] : nr;
            const unsigned g = r < nr ? (unsigned)ebase[r] + rank : ne;
            const unsigned t = (unsigned)ecorner[j];
            if (r >= nr || g >= ne || g < rank || t >= nc) atomicOr(tail + CH_ERR, 1);
            else {
                const int e = eside[j], s = e & 3;
                const int x = (int)(t % (unsigned)(gw + 1)), y = (int)(t / (unsigned)(gw + 1));
                ocorner[g] = (e & 4) ? (int)t : ~(int)t;
                vpos[g] = (e & 4) ? 1 : 0;
                term = s == 0 ? y : s == 1 ? x : s == 2 ? -y : -x;          // x1 y0 - x0 y1 of a unit edge, north up
                counts = (s & 1) ? 1 << 16 : 1;
                live = true;
            }
        }
    }
    const int lane = threadIdx.x & 63;
    u64 todo = __ballot(live);
    for (int round = 0; round < 64 && todo; ++round) {
        const int lead = __ffsll((long long)todo) - 1;
        const unsigned lr = (unsigned)__shfl((int)r, lead);
        const bool mine = live && r == lr;
        long long a = mine ? term : 0;
        int c = mine ? counts : 0;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            a += __shfl_xor(a, d);
            c += __shfl_xor(c, d);
        }
        if (lane == lead) {
            atomicAdd((u64*)o.area2 + lr, (u64)a);
            if (c & 0xffff) atomicAdd(o.edges + 2 * lr, c & 0xffff);
            if (c >> 16) atomicAdd(o.edges + 2 * lr + 1, c >> 16);
        }
        todo &= ~__ballot(mine);
    }
}

__global__ __launch_bounds__(OL_THREADS)
void ol_vertices(int gw, const int* __restrict__ ocorner, const int* __restrict__ vpos, unsigned ne, unsigned nv, unsigned nc,
                 int* tail, int* __restrict__ vertices)
{
    const unsigned g = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    if (g >= ne) return;
    const int t = ocorner[g];
    if (t < 0) return;
    const unsigned v = (unsigned)vpos[g];
    if (v >= nv || (unsigned)t >= nc) { atomicOr(tail + CH_ERR, 1); return; }
    vertices[2 * v] = (int)((unsigned)t % (unsigned)(gw + 1));
    vertices[2 * v + 1] = (int)((unsigned)t / (unsigned)(gw + 1));
}

__global__ __launch_bounds__(OL_THREADS)
void ol_offsets(const int* __restrict__ ebase, const int* __restrict__ vpos, unsigned ne, unsigned nr, unsigned nv, int* tail, int* __restrict__ offset)
{
    const unsigned r = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    if (r == 0 && (unsigned)tail[CH_TOTAL] != nv) atomicOr(tail + CH_ERR, 1);
    if (r >= nr) return;
    const unsigned g = (unsigned)ebase[r];
    if (g >= ne) { atomicOr(tail + CH_ERR, 1); offset[r] = 0; return; }
    offset[r] = vpos[g];
}

__global__ void ol_finish(const int* __restrict__ tail, unsigned nr, unsigned nv, int* __restrict__ offset)
{
    if (threadIdx.x == 0) offset[nr] = tail[CH_ERR] ? -1 : (int)nv;
}

// ---- burn --------------------------------------------------------------------------------------------------------------------
// The offset table checked by the first n_rings lanes, and the edge of lane i: from vertex i to the next vertex of its ring.
// false: no edge (a lane past the vertices, or an offset table that is not what it should be: flag bit 1).
__device__ __forceinline__ bool ol_burn_edge(const int* __restrict__ vertices, const int* __restrict__ offset, unsigned nr, unsigned nv,
                                             unsigned i, int* flag, unsigned& r, int& x0, int& y0, int& x1, int& y1)
{
    if (i < nr && (offset[i] < 0 || offset[i] > offset[i + 1])) atomicOr(flag, 2);
    if (i == 0 && (offset[0] != 0 || (unsigned)offset[nr] != nv)) atomicOr(flag, 2);
    if (i >= nv) return false;
    unsigned lo = 0, hi = nr;                                // the last ring whose offset is <= i
    for (int step = 0; step < 32 && lo < hi; ++step) {
        const unsigned mid = lo + (hi - lo) / 2;
        if ((unsigned)offset[mid] <= i) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0) { atomicOr(flag, 2); return false; }
    r = lo - 1;
    const unsigned end = (unsigned)offset[r + 1], begin = (unsigned)offset[r];
    if (end <= i || end > nv) { atomicOr(flag, 2); return false; }           // begin <= i by the search
    const unsigned i2 = i + 1 == end ? begin : i + 1;
    x0 = vertices[2 * i], y0 = vertices[2 * i + 1], x1 = vertices[2 * i2], y1 = vertices[2 * i2 + 1];
    return true;
}

// One lane per vertex = the edge from it to the next vertex of its ring; the first n_rings lanes also check the offset table.
__global__ __launch_bounds__(OL_THREADS)
void ol_burn_edges(const int* __restrict__ vertices, const int* __restrict__ offset, const int* __restrict__ ring_label,
                   unsigned nr, unsigned nv, int gw, int gh, int* __restrict__ out, int* flag)
{
    const unsigned i = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    unsigned r;
    int x0, y0, x1, y1;
    if (!ol_burn_edge(vertices, offset, nr, nv, i, flag, r, x0, y0, x1, y1)) return;
    if (x0 != x1) {
        if (y0 != y1) atomicOr(flag, 1);
        return;
    }
    if (x0 >= gw) return;
    const int x = max(x0, 0), ya = max(min(y0, y1), 0), yb = min(max(y0, y1), gh), k = ring_label[r];
    for (int y = ya; y < yb; ++y) atomicXor(out + (size_t)y * gw + x, k);
}

// The same lanes for edges of any direction: in every row the edge spans, the first column whose centre lies strictly right of
// the edge's crossing of the row's centre line, floor(x_c + 1/2) as one exact floor division.
__global__ __launch_bounds__(OL_THREADS)
void ol_burn_polygon_edges(const int* __restrict__ vertices, const int* __restrict__ offset, const int* __restrict__ ring_label,
                           unsigned nr, unsigned nv, int gw, int gh, int* __restrict__ out, int* flag)
{
    const unsigned i = blockIdx.x * (unsigned)OL_THREADS + threadIdx.x;
    unsigned r;
    int x0, y0, x1, y1;
    if (!ol_burn_edge(vertices, offset, nr, nv, i, flag, r, x0, y0, x1, y1)) return;
    const int lim = 1 << 20;
    if (x0 <= -lim || x0 >= lim || y0 <= -lim || y0 >= lim || x1 <= -lim || x1 >= lim || y1 <= -lim || y1 >= lim) {
        atomicOr(flag, 4);
        return;
    }
    if (y0 == y1) return;
    const int ya = max(min(y0, y1), 0), yb = min(max(y0, y1), gh), k = ring_label[r];
    const long long sign = y1 > y0 ? 1 : -1, den = sign * 2 * (y1 - y0), dx = sign * (x1 - x0);          // den > 0
    const long long base = den * x0 + den / 2;                                                          // (2 D x0 + D) sign
    for (int y = ya; y < yb; ++y) {
        const long long num = base + dx * (2 * y + 1 - 2 * y0);
        long long c = num / den;
        if (num % den < 0) --c;                              // the floor of a negative quotient
        if (c < gw) atomicXor(out + (size_t)y * gw + (c < 0 ? 0 : (int)c), k);
    }
}

// The running XOR along a row, a wave per row.
__global__ __launch_bounds__(OL_THREADS)
void ol_burn_rows(int* __restrict__ out, int gw, int gh)
{
    const unsigned row = blockIdx.x * (unsigned)(OL_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= (unsigned)gh) return;                         // whole waves only
    const int lane = threadIdx.x & 63;
    int* p = out + (size_t)row * gw;
    int carry = 0;
    for (int x0 = 0; x0 < gw; x0 += 64) {
        const int x = x0 + lane;
        int v = x < gw ? p[x] : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(v, d);
            if (lane >= d) v ^= u;
        }
        v ^= carry;
        if (x < gw) p[x] = v;
        carry = __shfl(v, 63);
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
struct OutlineWorkspace {
    size_t tail, s1, s2, cmask, cbase, pred0, preda, predb, vala, valb, ecorner, eside, rscan, skeya, skeyb, svala, svalb, spos, ebase, ocorner, vpos, bytes;
    unsigned nc;
};

static OutlineWorkspace outline_workspace(int gw, int gh, size_t max_edges)
{
    OutlineWorkspace w;
    const size_t nc = ((size_t)gw + 1) * ((size_t)gh + 1), top = nc > max_edges ? nc : max_edges, e = max_edges;
    const size_t nb1 = (top + OL_BLOCK - 1) / OL_BLOCK, nb2 = (nb1 + OL_BLOCK - 1) / OL_BLOCK;
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t here = at; at += align256(bytes); return here; };
    w.nc = (unsigned)nc;
    w.tail = take(256);
    w.s1 = take(nb1 * 4);
    w.s2 = take(nb2 * 4);
    w.cmask = take(nc);
    w.cbase = take(nc * 4);
    w.pred0 = take(e * 4); w.preda = take(e * 4); w.predb = take(e * 4);
    w.vala = take(e * 8); w.valb = take(e * 8);
    w.ecorner = take(e * 4); w.eside = take(e); w.rscan = take(e * 4);
    w.skeya = take(e * 4); w.skeyb = take(e * 4); w.svala = take(e * 4); w.svalb = take(e * 4); w.spos = take(e * 4);
    w.ebase = take(e * 4); w.ocorner = take(e * 4); w.vpos = take(e * 4);
    w.bytes = at;
    return w;
}

static const char* outline_check(int gw, int gh, int n, long long max_edges)
{
    if (gw < 1 || gh < 1) return "non-positive grid size";
    if ((long long)gw * gh >= (1ll << 29)) return "grid too large: gw * gh must be below 2^29 cells";
    if (n < 0) return "n must be >= 0";
    if (max_edges < 0 || max_edges > 4ll * gw * gh) return "max_edges must be in 0 .. 4 gw gh";
    return nullptr;
}

static int burn_entry(bool lattice, const int* vertices, const int* offset, const int* ring_label, int n_rings, int n_vertices,
                      int gw, int gh, int* out, int* flag, void* stream)
{
    if (!out || !flag) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (n_rings < 0 || n_vertices < 0) return fail(SMVS_ERR_ARG, "n_rings and n_vertices must be >= 0, got %d and %d", n_rings, n_vertices);
    const bool some = n_rings > 0 && n_vertices > 0;
    if (some && (!vertices || !offset || !ring_label)) return fail(SMVS_ERR_ARG, "null pointer argument");
    const size_t ncells = (size_t)gw * gh;
    const DsmBuf buf[] = {{out, ncells * 4, "out"}, {flag, 4, "flag"}, {vertices, some ? (size_t)n_vertices * 8 : 0, "vertices"},
                         {offset, some ? ((size_t)n_rings + 1) * 4 : 0, "offset"}, {ring_label, some ? (size_t)n_rings * 4 : 0, "ring_label"}};
    const char* other = nullptr;
    if (const char* name = dsm_first_alias(buf, 2, other)) return fail(SMVS_ERR_ARG, "%s aliases %s", name, other);
    for (int i = 2; i < 5; ++i)
        for (int j = 0; j < 2; ++j)
            if (buf[i].bytes && dsm_overlap(buf[i].p, buf[i].bytes, buf[j].p, buf[j].bytes))
                return fail(SMVS_ERR_ARG, "%s aliases %s", buf[j].name, buf[i].name);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(out, 0, ncells * 4, s) != hipSuccess || hipMemsetAsync(flag, 0, 4, s) != hipSuccess)
        return check_launch("dsm_burn (clearing the grid)");
    if (!some) return SMVS_OK;
    const unsigned lanes = (unsigned)(n_vertices > n_rings ? n_vertices : n_rings);     // a lane per vertex, and one per entry of the offset table
    const unsigned nr = (unsigned)n_rings, nv = (unsigned)n_vertices;
    if (lattice) DSM_LAUNCH(ol_burn_edges, lanes, OL_THREADS, s, vertices, offset, ring_label, nr, nv, gw, gh, out, flag);
    else DSM_LAUNCH(ol_burn_polygon_edges, lanes, OL_THREADS, s, vertices, offset, ring_label, nr, nv, gw, gh, out, flag);
    DSM_LAUNCH(ol_burn_rows, (size_t)gh * 64, OL_THREADS, s, out, gw, gh);            // a wave per row
    return SMVS_OK;
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT size_t smvs_dsm_outline_workspace_bytes(int gw, int gh, int max_edges)
{
    using namespace smvs;
    if (outline_check(gw, gh, 0, max_edges)) return 0;
    return outline_workspace(gw, gh, (size_t)max_edges).bytes;
}

SMVS_EXPORT int smvs_dsm_outline_count(const int* labels, int gw, int gh, int n, int max_edges, int* counts,
                                       void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!labels || !counts || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = outline_check(gw, gh, n, max_edges)) return fail(SMVS_ERR_ARG, "%s", msg);
    const OutlineWorkspace w = outline_workspace(gw, gh, (size_t)max_edges);
    if (workspace_bytes < w.bytes) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, w.bytes);
    const DsmBuf buf[] = {{labels, (size_t)gw * gh * 4, "labels"}, {counts, 12, "counts"}, {workspace, w.bytes, "workspace"}};
    const char* other = nullptr;
    if (const char* name = dsm_first_alias(buf, 3, other)) return fail(SMVS_ERR_ARG, "%s aliases %s", name, other);
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)workspace;
    int* tail = (int*)(base + w.tail);
    if (hipMemsetAsync(tail, 0, 256, s) != hipSuccess) return check_launch("dsm_outline_count (clearing the counts)");
    if (n == 0) {
        if (hipMemsetAsync(counts, 0, 12, s) != hipSuccess) return check_launch("dsm_outline_count (clearing the counts)");
        return SMVS_OK;
    }
    int *s1 = (int*)(base + w.s1), *s2 = (int*)(base + w.s2), *cbase = (int*)(base + w.cbase);
    unsigned char* cmask = (unsigned char*)(base + w.cmask);
    int rc;
    DSM_LAUNCH(ol_corners, w.nc, OL_THREADS, s, labels, gw, gh, n, w.nc, cmask, cbase);
    if ((rc = ol_scan_exclusive(cbase, w.nc, nullptr, s1, s2, tail + CH_N, s, "ol_scan (edges)"))) return rc;
    if (max_edges > 0) {
        const unsigned cap = (unsigned)max_edges;
        unsigned* pred[3] = {(unsigned*)(base + w.pred0), (unsigned*)(base + w.preda), (unsigned*)(base + w.predb)};
        u64* val[2] = {(u64*)(base + w.vala), (u64*)(base + w.valb)};
        int *ecorner = (int*)(base + w.ecorner), *rscan = (int*)(base + w.rscan);
        unsigned char* eside = (unsigned char*)(base + w.eside);
        DSM_LAUNCH(ol_edges, w.nc, OL_THREADS, s, labels, gw, gh, n, w.nc, (const unsigned char*)cmask, (const int*)cbase, cap, tail,
                   ecorner, val[0], pred[0], eside);
        int at;
        if ((rc = chain_order<false, OlLimit>(pred, val, cap, tail, s, &at))) return rc;
        DSM_LAUNCH(ol_starts, cap, OL_THREADS, s, (const u64*)val[at], (const unsigned char*)eside, rscan, cap, tail);
        if ((rc = ol_scan_exclusive(rscan, cap, tail + CH_N, s1, s2, tail + CH_LINES, s, "ol_scan (rings)"))) return rc;
    }
    DSM_LAUNCH(chain_counts_out, 1, 64, s, (const int*)tail, counts);
    return SMVS_OK;
}

SMVS_EXPORT int smvs_dsm_outline_write(const int* labels, int gw, int gh, int n, int n_edges, int n_rings, int n_vertices,
                                       int* ring_label, long long* area2, int* edges, int* offset, int* first_ring, int* vertices,
                                       void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!labels || !offset || !first_ring || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = outline_check(gw, gh, n, n_edges)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (n_rings < 0 || n_rings > n_edges || n_vertices < 0 || n_vertices > n_edges || (n_edges > 0) != (n_rings > 0) || (n_edges > 0) != (n_vertices > 0))
        return fail(SMVS_ERR_ARG, "n_rings (%d) and n_vertices (%d) must be in 1 .. n_edges (%d), or all three 0", n_rings, n_vertices, n_edges);
    if (n_edges > 0 && n == 0) return fail(SMVS_ERR_ARG, "edges without labels (n == 0)");
    if (n_edges > 0 && (!ring_label || !area2 || !edges || !vertices)) return fail(SMVS_ERR_ARG, "null pointer argument");
    const OutlineWorkspace w = outline_workspace(gw, gh, (size_t)n_edges);
    if (workspace_bytes < w.bytes) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, w.bytes);
    const size_t m = (size_t)n_rings;
    const DsmBuf buf[] = {{labels, (size_t)gw * gh * 4, "labels"}, {workspace, w.bytes, "workspace"}, {ring_label, m * 4, "ring_label"},
                         {area2, m * 8, "area2"}, {edges, m * 8, "edges"}, {offset, (m + 1) * 4, "offset"},
                         {first_ring, ((size_t)n + 1) * 4, "first_ring"}, {vertices, (size_t)n_vertices * 8, "vertices"}};
    const char* other = nullptr;
    if (const char* name = dsm_first_alias(buf, 8, other)) return fail(SMVS_ERR_ARG, "%s aliases %s", name, other);
    hipStream_t s = (hipStream_t)stream;
    if (n_edges == 0) {                                      // no ring: the two tables that still have entries
        if (hipMemsetAsync(first_ring, 0, ((size_t)n + 1) * 4, s) != hipSuccess || hipMemsetAsync(offset, 0, 4, s) != hipSuccess)
            return check_launch("dsm_outline_write (empty tables)");
        return SMVS_OK;
    }
    char* base = (char*)workspace;
    int *tail = (int*)(base + w.tail), *s1 = (int*)(base + w.s1), *s2 = (int*)(base + w.s2), *cbase = (int*)(base + w.cbase);
    const unsigned char *cmask = (const unsigned char*)(base + w.cmask), *eside = (const unsigned char*)(base + w.eside);
    const u64* val = (const u64*)(base + (chain_rounds((unsigned)n_edges) % 2 ? w.valb : w.vala));
    const unsigned* pred0 = (const unsigned*)(base + w.pred0);
    const int* ecorner = (const int*)(base + w.ecorner);
    int *rscan = (int*)(base + w.rscan), *skey[2] = {(int*)(base + w.skeya), (int*)(base + w.skeyb)};
    int *sval[2] = {(int*)(base + w.svala), (int*)(base + w.svalb)}, *spos = (int*)(base + w.spos);
    int *ebase = (int*)(base + w.ebase), *ocorner = (int*)(base + w.ocorner), *vpos = (int*)(base + w.vpos);
    const unsigned ne = (unsigned)n_edges, nr = (unsigned)n_rings, nv = (unsigned)n_vertices;
    const OlRings o = {ring_label, edges, area2};
    int rc;
    DSM_LAUNCH(ol_ring_init, ne, OL_THREADS, s, labels, gw, gh, n, val, (const int*)rscan, ecorner, eside, ne, nr, nv, w.nc, tail, skey[0], sval[0]);
    int bits = 0, at;
    while (bits < 31 && ((unsigned)n >> bits)) ++bits;
    if ((rc = chain_sort(skey, sval, spos, nr, bits, s1, s2, tail, s, &at))) return rc;
    const int *keys = skey[at], *starts = sval[at];
    DSM_LAUNCH(ol_ring_table, nr, OL_THREADS, s, keys, starts, val, pred0, rscan, ebase, ne, nr, tail, o);
    DSM_LAUNCH(chain_first, (size_t)n + 1, OL_THREADS, s, keys, nr, n, 1u, first_ring);       // the first ring of label k + 1; entry n is n_rings
    if ((rc = ol_scan_exclusive(ebase, nr, nullptr, s1, s2, tail + CH_TOTAL, s, "ol_scan (ring lengths)"))) return rc;
    DSM_LAUNCH(ol_place, ne, OL_THREADS, s, gw, val, ecorner, eside, cmask, (const int*)cbase, (const int*)rscan, (const int*)ebase, ne, nr, w.nc,
               tail, ocorner, vpos, o);
    if ((rc = ol_scan_exclusive(vpos, ne, nullptr, s1, s2, tail + CH_TOTAL, s, "ol_scan (vertices)"))) return rc;
    DSM_LAUNCH(ol_vertices, ne, OL_THREADS, s, gw, (const int*)ocorner, (const int*)vpos, ne, nv, w.nc, tail, vertices);
    DSM_LAUNCH(ol_offsets, nr, OL_THREADS, s, (const int*)ebase, (const int*)vpos, ne, nr, nv, tail, offset);
    DSM_LAUNCH(ol_finish, 1, 64, s, (const int*)tail, nr, nv, offset);
    return SMVS_OK;
}

SMVS_EXPORT int smvs_dsm_burn(const int* vertices, const int* offset, const int* ring_label, int n_rings, int n_vertices,
                              int gw, int gh, int* out, int* flag, void* stream)
{
    return smvs::burn_entry(true, vertices, offset, ring_label, n_rings, n_vertices, gw, gh, out, flag, stream);
}

SMVS_EXPORT int smvs_dsm_burn_polygons(const int* vertices, const int* offset, const int* ring_label, int n_rings, int n_vertices,
                                       int gw, int gh, int* out, int* flag, void* stream)
{
    return smvs::burn_entry(false, vertices, offset, ring_label, n_rings, n_vertices, gw, gh, out, flag, stream);
}

}  // extern "C"
