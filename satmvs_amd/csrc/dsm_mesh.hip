// dsm_mesh.hip -- error-bounded triangle meshes of a DSM ("Meshes"; include/satmvs.h for the rule): the
// longest-side bisection hierarchy (RTIN) over the lattice of cell centres, refined where the EXACT error of a triangle -- the
// largest deviation of any lattice vertex in it from its plane -- exceeds the tolerance.  All integers, no float but the heights
// written at the end.
//
//   smvs_dsm_mesh_errors   dsm -> the saturated error of every lattice vertex, int64 in units of 2^-8 m / S
//   smvs_dsm_mesh_count    errors, threshold -> the emitted triangles per hypotenuse midpoint, the used vertices, their scans
//   smvs_dsm_mesh_write    the workspace of count -> triangles, levels, vertices, heights
//   smvs_dsm_mesh_heights  errors, threshold -> the mesh's height (and deviation) at every lattice vertex
//
// Where a vertex stands.  With t = ctz(r | c) < k a vertex (r, c) that is no root corner splits triangles of ONE level: of level
// 2 j (j = k - t - 1) if r and c both have bit t set -- it is the centre of a square of side h = 2^(t+1) and splits the two halves
// of that square -- and of level 2 j + 1 otherwise -- it is the middle of a side of such a square and splits the triangle on
// either side of it.  The square's diagonal runs through the centre of the square of side 2 h around it (the root's from its
// upper-left corner), so everything about a triangle follows from its split vertex and the side its apex is on.
//
// Errors.  me_init writes +infinity where one of a vertex's triangles leaves the grid and 0 elsewhere.  me_deviate is one lane
// per lattice vertex p, a wave an 8 x 8 block, the levels in a loop: per level the lane finds the squares (even levels) or the
// diamonds (odd levels: the two triangles of a split vertex together) whose closed area holds p -- one, or up to four when p
// lies on their rims -- forms h q_p - h plane(p) from the three corners' quanta and raises the split vertex's word by a 64-bit
// integer max atomic; a void p raises it to +infinity.  From h = 8 up every lane of a wave stands in the same square, so the
// wave's lanes that share a split vertex combine by a butterfly of shuffles and one lane makes the atomic; below that the
// addresses of a wave are spread and each lane makes its own.  A deviation of 0 makes none.  me_saturate is one gather pass per
// level, finest first, over the vertices of that level alone: no atomics, every word read was final before the launch.  The
// maximum is order-free: equal bits from run to run.
//
// Emission.  The order key of a triangle is (row, col) of a + b and its side, so the slots are laid out in that order: row 2 r
// holds the lattice vertices of row r (the triangles they split), row 2 r + 1 the cells between rows r and r + 1 (the finest
// triangles).  mc_emit is one lane per slot pair: a mask of the two sides, their number for the scan (dsm_scan.h), and a mark
// on the three corners of every emitted triangle (plain stores of 1).  The two scans give every triangle's and every vertex's
// place; mw_triangles and mw_vertices write from the mask and the scans alone.  mh_walk descends from the root triangle by the
// active flags, at most 2 k steps, and interpolates in the triangle it stops in; a walk that ends in a finest triangle with a
// void corner takes the vertex's own height if the vertex is marked (see include/satmvs.h for why that is all that is left).
// No kernel uses scratch or LDS beyond the scan's.  Workspace: 14 bytes per cell and the scans' block sums.
#include <limits.h>
#include <stdint.h>

#include "dsm_common.h"
#include "dsm_scan.h"
#include "smvs_host.h"

namespace smvs {

typedef long long i64;
typedef unsigned long long u64;

constexpr int ME_THREADS = 256;
constexpr i64 ME_INF = LLONG_MAX;
constexpr long long ME_MAX_CELLS = 1ll << 29;                // slots < 2^30, an int32 scan

struct MeGrid { int gw, gh, k, S, ch, cw; };                 // ch, cw: the cover's extent in cells, multiples of S, at least S

__device__ __forceinline__ bool me_on(const MeGrid& g, int r, int c) { return r >= 0 && c >= 0 && r < g.gh && c < g.gw; }

// The quantum of an on-grid vertex; false: a void.
__device__ __forceinline__ bool me_q(const float* __restrict__ dsm, const MeGrid& g, float nodata, int r, int c, int& q)
{
    return dsm_quantum(dsm[(size_t)r * g.gw + c], nodata, q);
}

__device__ __forceinline__ bool me_active(const i64* __restrict__ errors, const MeGrid& g, i64 thr, int r, int c)
{
    if (((r | c) & (g.S - 1)) == 0) return true;             // a root corner
    if (!me_on(g, r, c)) return true;
    return errors[(size_t)r * g.gw + c] > thr;
}

// ---- errors --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ME_THREADS)
void me_init(MeGrid g, i64* __restrict__ errors)
{
    const unsigned i = blockIdx.x * (unsigned)ME_THREADS + threadIdx.x;
    if (i >= (unsigned)g.gw * (unsigned)g.gh) return;
    const int r = (int)(i / (unsigned)g.gw), c = (int)(i % (unsigned)g.gw);
    i64 e = 0;
    if ((r | c) & (g.S - 1)) {
        const int t = __ffs(r | c) - 1, half = 1 << t;
        bool out;
        if ((r & c) >> t & 1) out = r + half > g.gh - 1 || c + half > g.gw - 1;                         // a square
        else if ((r >> t & 1) == 0) out = c + half > g.gw - 1 || (r < g.ch && r + half > g.gh - 1);     // a hypotenuse along the row
        else out = r + half > g.gh - 1 || (c < g.cw && c + half > g.gw - 1);                            // along the column
        e = out ? ME_INF : 0;
    }
    errors[i] = e;
}

__device__ __forceinline__ i64 me_wave_max(i64 v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const i64 o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

// errors[key] <- max(errors[key], val) for every lane with key >= 0 and val > 0.  `together`: wave-uniform; the lanes that share
// a key combine first.  Every lane of the wave calls this.
__device__ __forceinline__ void me_raise(i64* errors, int key, i64 val, bool together)
{
    bool pending = key >= 0 && val > 0;
    if (!together) {
        if (pending) atomicMax((u64*)errors + key, (u64)val);
        return;
    }
    const int lane = threadIdx.x & 63;
    u64 left = __ballot(pending);
    while (left) {
        const int leader = __ffsll((long long)left) - 1;
        const int k = __shfl(key, leader);
        const bool mine = pending && key == k;
        const i64 top = me_wave_max(mine ? val : 0);
        if (lane == leader) atomicMax((u64*)errors + k, (u64)top);
        pending = pending && !mine;
        left = __ballot(pending);
    }
}

__global__ __launch_bounds__(ME_THREADS)
void me_deviate(const float* __restrict__ dsm, MeGrid g, float nodata, i64* errors)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned across = ((unsigned)g.gw + 15) / 16;
    const int r = (int)(blockIdx.x / across) * 16 + (wave >> 1) * 8 + (lane >> 3);
    const int c = (int)(blockIdx.x % across) * 16 + (wave & 1) * 8 + (lane & 7);
    const bool on = r < g.gh && c < g.gw;
    int qp = 0;
    const bool valid = on && me_q(dsm, g, nodata, r, c, qp);
    for (int j = 0; j < g.k; ++j) {
        const int h = g.S >> j, half = h >> 1;
        const bool together = h >= 8;
        const int R0 = r / h, C0 = c / h;
        const bool rim_r = r % h == 0 && r > 0, rim_c = c % h == 0 && c > 0;
        // level 2 j: the squares of side h that hold p
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int R = R0 - (s >> 1), C = C0 - (s & 1);
            int key = -1;
            i64 val = 0;
            const bool there = on && ((s >> 1) == 0 || rim_r) && ((s & 1) == 0 || rim_c) && R * h < g.ch && C * h < g.cw;
            if (there && (R + 1) * h <= g.gh - 1 && (C + 1) * h <= g.gw - 1) {       // a square that leaves the grid is +infinity already
                key = (R * h + half) * g.gw + C * h + half;
                if (!valid) val = ME_INF;
                else {
                    const int u = r - R * h, v = c - C * h, top = R * h, left = C * h;
                    const bool main_diag = j == 0 || ((R ^ C) & 1) == 0;
                    int ar, ac, xr, xc, yr, yc, sx, sy;      // apex, the ends of its legs, p's steps along the legs
                    if (main_diag) {
                        if (u >= v) { ar = top + h; ac = left; xr = top; xc = left; yr = top + h; yc = left + h; sx = h - u; sy = v; }
                        else { ar = top; ac = left + h; xr = top; xc = left; yr = top + h; yc = left + h; sx = h - v; sy = u; }
                    } else {
                        if (u + v <= h) { ar = top; ac = left; xr = top; xc = left + h; yr = top + h; yc = left; sx = v; sy = u; }
                        else { ar = top + h; ac = left + h; xr = top + h; xc = left; yr = top; yc = left + h; sx = h - v; sy = h - u; }
                    }
                    int qa, qx, qy;
                    if (me_q(dsm, g, nodata, ar, ac, qa) && me_q(dsm, g, nodata, xr, xc, qx) && me_q(dsm, g, nodata, yr, yc, qy)) {
                        const i64 n = (i64)h * qp - ((i64)h * qa + (i64)(qx - qa) * sx + (i64)(qy - qa) * sy);
                        val = (n < 0 ? -n : n) << j;
                    } else key = -1;                         // the void corner's own lane raises this square
                }
            }
            me_raise(errors, key, val, together);
        }
        // level 2 j + 1: the diamonds round the middles of the squares' sides that hold p; s < 4 hypotenuses along a row
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const bool row_hyp = s < 4;
            const int along = row_hyp ? c : r, across_p = row_hyp ? r : c;          // p along the hypotenuse's line and across it
            const int A0 = row_hyp ? C0 : R0, B0 = row_hyp ? R0 : C0;
            const bool rim_a = row_hyp ? rim_c : rim_r;
            const int A = A0 - (s & 1), B = B0 + ((s >> 1) & 1);                     // the hypotenuse's square index along, its line across
            const int m_along = A * h + half, m_across = B * h;
            const int cover_along = row_hyp ? g.cw : g.ch, cover_across = row_hyp ? g.ch : g.cw;
            const int n_along = row_hyp ? g.gw : g.gh, n_across = row_hyp ? g.gh : g.gw;
            int key = -1;
            i64 val = 0;
            const int x = along - m_along, y = across_p - m_across, ay = y < 0 ? -y : y;
            const bool there = on && ((s & 1) == 0 || rim_a) && A * h < cover_along && m_across <= cover_across &&
                               (x < 0 ? -x : x) + ay <= half;
            if (there && m_along + half <= n_along - 1 && m_across <= n_across - 1) {
                const int mr = row_hyp ? m_across : m_along, mc = row_hyp ? m_along : m_across;
                key = mr * g.gw + mc;
                if (!valid) val = ME_INF;
                else {
                    const int apex_across = m_across + (y < 0 ? -half : half);
                    int qa, qb, qc = 0;
                    bool ok = me_q(dsm, g, nodata, row_hyp ? mr : m_along - half, row_hyp ? m_along - half : mc, qa) &&
                              me_q(dsm, g, nodata, row_hyp ? mr : m_along + half, row_hyp ? m_along + half : mc, qb);
                    if (ok && y != 0) {
                        ok = apex_across >= 0 && apex_across <= n_across - 1 &&
                             me_q(dsm, g, nodata, row_hyp ? apex_across : m_along, row_hyp ? m_along : apex_across, qc);
                    }
                    if (ok) {
                        // on the hypotenuse (ay = 0) both triangles' planes agree and the apex does not count
                        const i64 n = (i64)h * qp - ((i64)(qa + qb) * half + (i64)(qb - qa) * x + (i64)(2 * qc - qa - qb) * ay);
                        val = (n < 0 ? -n : n) << j;
                    } else key = -1;
                }
            }
            me_raise(errors, key, val, together);
        }
    }
}

// The vertices of level lv gather from those of level lv + 1: e(apex) <- max(e(apex), e(split vertex)) over the triangles of
// level lv + 1, whose apex splits their parent.  One lane per vertex of level lv.
__global__ __launch_bounds__(ME_THREADS)
void me_saturate(MeGrid g, int lv, i64* errors)
{
    const int j = lv >> 1, h = g.S >> j, half = h >> 1;
    const unsigned nr = (unsigned)(g.ch / h), nc = (unsigned)(g.cw / h);
    const unsigned i = blockIdx.x * (unsigned)ME_THREADS + threadIdx.x;
    int r, c, dr[4], dc[4];
    if ((lv & 1) == 0) {
        if (i >= nr * nc) return;
        r = (int)(i / nc) * h + half;
        c = (int)(i % nc) * h + half;
        dr[0] = -half; dc[0] = 0; dr[1] = half; dc[1] = 0; dr[2] = 0; dc[2] = -half; dr[3] = 0; dc[3] = half;
    } else {
        const unsigned rows = (nr + 1) * nc;                 // hypotenuses along a row first, then along a column
        if (i >= rows + nr * (nc + 1)) return;
        if (i < rows) { r = (int)(i / nc) * h; c = (int)(i % nc) * h + half; }
        else { r = (int)((i - rows) / (nc + 1)) * h + half; c = (int)((i - rows) % (nc + 1)) * h; }
        const int q = half >> 1;
        dr[0] = -q; dc[0] = -q; dr[1] = -q; dc[1] = q; dr[2] = q; dc[2] = -q; dr[3] = q; dc[3] = q;
    }
    if (!me_on(g, r, c)) return;
    i64 e = errors[(size_t)r * g.gw + c];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int rr = r + dr[n], cc = c + dc[n];
        if (rr < 0 || cc < 0 || rr > g.ch || cc > g.cw) continue;                  // no triangle on that side of the cover's rim
        const i64 o = me_on(g, rr, cc) ? errors[(size_t)rr * g.gw + cc] : ME_INF;
        e = o > e ? o : e;
    }
    errors[(size_t)r * g.gw + c] = e;
}

// ---- emission ------------------------------------------------------------------------------------------------------------------
struct MeTri { int ar, ac, br, bc, cr, cc, level; bool exists; };            // hypotenuse a - b, apex c

// The triangle of side `side` (0: the apex that is lexicographically smaller) that the vertex (r, c), no root corner, splits.
__device__ __forceinline__ MeTri me_split_triangle(const MeGrid& g, int r, int c, int side)
{
    MeTri T;
    const int t = __ffs(r | c) - 1, half = 1 << t, j = g.k - t - 1;
    T.exists = true;
    if ((r & c) >> t & 1) {
        const int R = (r - half) >> (t + 1), C = (c - half) >> (t + 1);
        const bool main_diag = j == 0 || ((R ^ C) & 1) == 0;
        T.level = 2 * j;
        if (main_diag) {
            T.ar = r - half; T.ac = c - half; T.br = r + half; T.bc = c + half;
            T.cr = side ? r + half : r - half; T.cc = side ? c - half : c + half;
        } else {
            T.ar = r - half; T.ac = c + half; T.br = r + half; T.bc = c - half;
            T.cr = side ? r + half : r - half; T.cc = side ? c + half : c - half;
        }
    } else if ((r >> t & 1) == 0) {
        T.level = 2 * j + 1;
        T.ar = r; T.ac = c - half; T.br = r; T.bc = c + half;
        T.cr = side ? r + half : r - half; T.cc = c;
        T.exists = side ? r < g.ch : r > 0;
    } else {
        T.level = 2 * j + 1;
        T.ar = r - half; T.ac = c; T.br = r + half; T.bc = c;
        T.cr = r; T.cc = side ? c + half : c - half;
        T.exists = side ? c < g.cw : c > 0;
    }
    return T;
}

// The finest triangle of side `side` in the cell whose upper-left vertex is (r, c).
__device__ __forceinline__ MeTri me_cell_triangle(const MeGrid& g, int r, int c, int side)
{
    MeTri T;
    T.level = 2 * g.k;
    T.exists = true;
    if (((r ^ c) & 1) == 0) {
        T.ar = r; T.ac = c; T.br = r + 1; T.bc = c + 1;
        T.cr = side ? r + 1 : r; T.cc = side ? c : c + 1;
    } else {
        T.ar = r; T.ac = c + 1; T.br = r + 1; T.bc = c;
        T.cr = side ? r + 1 : r; T.cc = side ? c + 1 : c;
    }
    return T;
}

__device__ __forceinline__ bool me_tri_on(const MeGrid& g, const MeTri& T)
{
    return me_on(g, T.ar, T.ac) && me_on(g, T.br, T.bc) && me_on(g, T.cr, T.cc);
}

// Slot pair i of the order: rows of 2 gw - 1 pairs, gw vertices and the gw - 1 cells under them.  false: no such pair.
__device__ __forceinline__ bool me_slot(const MeGrid& g, unsigned i, int& r, int& c, bool& cell)
{
    const unsigned per = 2u * (unsigned)g.gw - 1;
    r = (int)(i / per);
    const int x = (int)(i % per);
    cell = x >= g.gw;
    c = cell ? x - g.gw : x;
    return r < g.gh && !(cell && r >= g.gh - 1);
}

// The two sides' emission as a mask.
__device__ __forceinline__ int me_emitted(const float* __restrict__ dsm, const i64* __restrict__ errors, const MeGrid& g, float nodata,
                                          i64 thr, int r, int c, bool cell)
{
    int mask = 0;
    if (cell) {
        int q;
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const MeTri T = me_cell_triangle(g, r, c, side);
            if (me_active(errors, g, thr, T.cr, T.cc) && me_q(dsm, g, nodata, T.ar, T.ac, q) && me_q(dsm, g, nodata, T.br, T.bc, q) &&
                me_q(dsm, g, nodata, T.cr, T.cc, q))
                mask |= 1 << side;
        }
        return mask;
    }
    if (((r | c) & (g.S - 1)) == 0 || me_active(errors, g, thr, r, c)) return 0;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const MeTri T = me_split_triangle(g, r, c, side);
        // a vertex with a finite error has its triangles on the grid; an error map that says otherwise emits nothing there
        if (T.exists && me_tri_on(g, T) && me_active(errors, g, thr, T.cr, T.cc)) mask |= 1 << side;
    }
    return mask;
}

__global__ __launch_bounds__(ME_THREADS)
void mc_emit(const float* __restrict__ dsm, const i64* __restrict__ errors, MeGrid g, float nodata, i64 thr, unsigned n_slots,
             int* __restrict__ count, unsigned char* __restrict__ masks, int* used)
{
    const unsigned i = blockIdx.x * (unsigned)ME_THREADS + threadIdx.x;
    if (i >= n_slots) return;
    int r, c;
    bool cell;
    int mask = 0;
    if (me_slot(g, i, r, c, cell)) mask = me_emitted(dsm, errors, g, nodata, thr, r, c, cell);
    if (count) count[i] = (mask & 1) + (mask >> 1);
    if (masks) masks[i] = (unsigned char)mask;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        if (!(mask >> side & 1)) continue;
        const MeTri T = cell ? me_cell_triangle(g, r, c, side) : me_split_triangle(g, r, c, side);
        used[(size_t)T.ar * g.gw + T.ac] = 1;                 // an emitted triangle's corners are on the grid
        used[(size_t)T.br * g.gw + T.bc] = 1;
        used[(size_t)T.cr * g.gw + T.cc] = 1;
    }
}

__global__ void mc_totals(const int* __restrict__ totals, int* __restrict__ counts)
{
    if (threadIdx.x < 2) counts[threadIdx.x] = totals[threadIdx.x];
}

// ---- write ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ME_THREADS)
void mw_triangles(MeGrid g, unsigned n_slots, const int* __restrict__ totals, int nt, int nv, const int* __restrict__ first,
                  const unsigned char* __restrict__ masks, const int* __restrict__ id, int* __restrict__ triangles,
                  unsigned char* __restrict__ tri_level, int* __restrict__ status)
{
    const unsigned i = blockIdx.x * (unsigned)ME_THREADS + threadIdx.x;
    const bool same = totals[0] == nt && totals[1] == nv;
    if (i == 0) *status = same ? nt : -1;
    if (i >= n_slots) return;
    int r, c;
    bool cell;
    if (!me_slot(g, i, r, c, cell)) return;
    const int mask = masks[i];
    int at = first[i];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        if (!(mask >> side & 1)) continue;
        if (!same || at < 0 || at >= nt) return;
        const MeTri T = cell ? me_cell_triangle(g, r, c, side) : me_split_triangle(g, r, c, side);
        if (!me_tri_on(g, T)) return;                        // a mask that count did not write
        // counter-clockwise seen from above, east right and north up: x = col, y = -row
        const int cross = (T.bc - T.ac) * (T.ar - T.cr) - (T.ar - T.br) * (T.cc - T.ac);
        const int a = id[(size_t)T.ar * g.gw + T.ac], b = id[(size_t)T.br * g.gw + T.bc];
        triangles[3 * (size_t)at] = cross > 0 ? a : b;
        triangles[3 * (size_t)at + 1] = cross > 0 ? b : a;
        triangles[3 * (size_t)at + 2] = id[(size_t)T.cr * g.gw + T.cc];
        tri_level[at] = (unsigned char)T.level;
        ++at;
    }
}

__global__ __launch_bounds__(ME_THREADS)
void mw_vertices(const float* __restrict__ dsm, MeGrid g, const int* __restrict__ totals, int nt, int nv, const int* __restrict__ id,
                 int* __restrict__ vertices, float* __restrict__ z)
{
    const unsigned n = (unsigned)g.gw * (unsigned)g.gh, i = blockIdx.x * (unsigned)ME_THREADS + threadIdx.x;
    if (i >= n || totals[0] != nt || totals[1] != nv) return;
    const int at = id[i], next = i + 1 < n ? id[i + 1] : totals[1];
    if (next == at || at < 0 || at >= nv) return;
    vertices[2 * (size_t)at] = (int)(i % (unsigned)g.gw);
    vertices[2 * (size_t)at + 1] = (int)(i / (unsigned)g.gw);
    z[at] = dsm[i];
}

// ---- heights -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ME_THREADS)
void mh_walk(const float* __restrict__ dsm, const i64* __restrict__ errors, MeGrid g, float nodata, i64 thr, const int* __restrict__ used,
             float* __restrict__ heights, i64* __restrict__ dev)
{
    const unsigned i = blockIdx.x * (unsigned)ME_THREADS + threadIdx.x;
    if (i >= (unsigned)g.gw * (unsigned)g.gh) return;
    const int r = (int)(i / (unsigned)g.gw), c = (int)(i % (unsigned)g.gw);
    int qp;
    float out = nodata;
    i64 d = ME_INF;
    if (me_q(dsm, g, nodata, r, c, qp)) {
        const int r0 = min(r / g.S * g.S, g.ch - g.S), c0 = min(c / g.S * g.S, g.cw - g.S);
        int ar, ac, br, bc, cr, cc;
        if (r - r0 >= c - c0) { ar = r0; ac = c0; br = r0 + g.S; bc = c0 + g.S; cr = r0 + g.S; cc = c0; }
        else { ar = r0 + g.S; ac = c0 + g.S; br = r0; bc = c0; cr = r0; cc = c0 + g.S; }
        bool stopped = false;
        for (int level = 0; level < 2 * g.k; ++level) {
            const int mr = (ar + br) >> 1, mc = (ac + bc) >> 1;
            if (!me_active(errors, g, thr, mr, mc)) { stopped = true; break; }
            // the child (c, a, m) if p is on a's side of the line c - m or on it, else (b, c, m)
            const int lr = mr - cr, lc = mc - cc;
            const int dp = lr * (c - cc) - lc * (r - cr), da = lr * (ac - cc) - lc * (ar - cr);
            const int pr = cr, pc = cc;
            if (dp == 0 || (dp > 0) == (da > 0)) { br = ar; bc = ac; ar = pr; ac = pc; }
            else { ar = br; ac = bc; br = pr; bc = pc; }
            cr = mr;
            cc = mc;
        }
        int qa, qb, qc;
        const bool whole = me_on(g, ar, ac) && me_on(g, br, bc) && me_on(g, cr, cc) && me_q(dsm, g, nodata, ar, ac, qa) &&
                           me_q(dsm, g, nodata, br, bc, qb) && me_q(dsm, g, nodata, cr, cc, qc);
        i64 plane = 0;                                       // S plane(p) in units of 2^-8 m
        bool covered = false;
        if (whole) {                                         // a triangle the walk stopped in is whole by its finite error
            const int xr = ar - cr, xc = ac - cc, yr = br - cr, yc = bc - cc;
            const i64 D = (i64)xr * xr + (i64)xc * xc;       // |a - c|^2 = |b - c|^2, a power of two
            const i64 s = (i64)(r - cr) * xr + (i64)(c - cc) * xc, t = (i64)(r - cr) * yr + (i64)(c - cc) * yc;
            const i64 pd = (i64)qc * D + (i64)(qa - qc) * s + (i64)(qb - qc) * t;
            plane = (pd * (i64)g.S) >> (__ffsll(D) - 1);     // exact: the plane's denominators divide S, so the arithmetic shift drops zeros
            covered = true;
        } else if (!stopped && used[i]) {
            plane = (i64)qp * g.S;
            covered = true;
        }
        if (covered) {
            out = (float)__ddiv_rn((double)plane, (double)((i64)g.S * 256));
            d = (i64)qp * g.S - plane;
        }
    }
    heights[i] = out;
    if (dev) dev[i] = d;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct MeshWorkspace { size_t count, masks, used, s1, s2, totals, bytes; size_t n_slots; };

static bool mesh_tile_ok(int tile) { return tile >= 2 && tile <= 1024 && (tile & (tile - 1)) == 0; }

static const char* mesh_grid_check(int gw, int gh, int tile)
{
    if (gw < 1 || gh < 1) return "non-positive grid size";
    if ((long long)gw * gh >= ME_MAX_CELLS) return "grid too large: gw * gh must be below 2^29 cells";
    if (!mesh_tile_ok(tile)) return "tile must be a power of two in 2 .. 1024";
    return nullptr;
}

static MeGrid mesh_grid(int gw, int gh, int tile)
{
    MeGrid g;
    g.gw = gw;
    g.gh = gh;
    g.S = tile;
    g.k = dsm_ceil_log2((size_t)tile);
    g.ch = (gh > 1 ? (gh - 1 + tile - 1) / tile : 1) * tile;  // a single row or column still stands in one root square
    g.cw = (gw > 1 ? (gw - 1 + tile - 1) / tile : 1) * tile;
    return g;
}

static MeshWorkspace mesh_workspace(int gw, int gh)
{
    MeshWorkspace w;
    const size_t n = (size_t)gw * gh;
    w.n_slots = (size_t)gh * (2 * (size_t)gw - 1);
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t here = at; at += align256(bytes); return here; };
    const size_t nb1 = (w.n_slots + OL_BLOCK - 1) / OL_BLOCK, nb2 = (nb1 + OL_BLOCK - 1) / OL_BLOCK;
    w.count = take(w.n_slots * 4);
    w.masks = take(w.n_slots);
    w.used = take(n * 4);
    w.s1 = take(nb1 * 4);
    w.s2 = take(nb2 * 4);
    w.totals = take(16);
    w.bytes = at;
    return w;
}

// What the entries check alike; the workspace, if any, is the last entry of the table.
static int mesh_check(int gw, int gh, int tile, const DsmBuf* buf, int n_buf, bool has_workspace, size_t workspace_bytes)
{
    if (const char* msg = mesh_grid_check(gw, gh, tile)) return fail(SMVS_ERR_ARG, "%s (got %d x %d, tile %d)", msg, gw, gh, tile);
    const char* other = nullptr;
    if (const char* name = dsm_first_alias(buf, n_buf, other)) return fail(SMVS_ERR_ARG, "%s aliases %s", name, other);
    if (has_workspace && workspace_bytes < buf[n_buf - 1].bytes)
        return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, buf[n_buf - 1].bytes);
    return SMVS_OK;
}

// The marks of the used vertices (and, with count and masks, the emission of every slot pair).
static int mesh_emit(const float* dsm, const i64* errors, const MeGrid& g, float nodata, i64 thr, const MeshWorkspace& w, char* base,
                     bool slots, hipStream_t s)
{
    int* used = (int*)(base + w.used);
    if (hipMemsetAsync(used, 0, (size_t)g.gw * g.gh * 4, s) != hipSuccess) return check_launch("dsm_mesh (clearing the marks)");
    DSM_LAUNCH(mc_emit, w.n_slots, ME_THREADS, s, dsm, errors, g, nodata, thr, (unsigned)w.n_slots, slots ? (int*)(base + w.count) : nullptr,
               slots ? (unsigned char*)(base + w.masks) : nullptr, used);
    return SMVS_OK;
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT size_t smvs_dsm_mesh_workspace_bytes(int gw, int gh, int tile)
{
    using namespace smvs;
    return mesh_grid_check(gw, gh, tile) ? 0 : mesh_workspace(gw, gh).bytes;
}

SMVS_EXPORT int smvs_dsm_mesh_errors(const float* dsm, int gw, int gh, float nodata, int tile, long long* errors, void* stream)
{
    using namespace smvs;
    if (!dsm || !errors) return fail(SMVS_ERR_ARG, "null pointer argument");
    const size_t n = gw > 0 && gh > 0 ? (size_t)gw * gh : 0;
    const DsmBuf buf[] = {{dsm, n * 4, "dsm"}, {errors, n * 8, "errors"}};
    if (int rc = mesh_check(gw, gh, tile, buf, 2, false, 0)) return rc;
    const MeGrid g = mesh_grid(gw, gh, tile);
    hipStream_t s = (hipStream_t)stream;
    DSM_LAUNCH(me_init, n, ME_THREADS, s, g, errors);
    const size_t tiles = (size_t)((gw + 15) / 16) * (size_t)((gh + 15) / 16);
    DSM_LAUNCH(me_deviate, tiles * ME_THREADS, ME_THREADS, s, dsm, g, nodata, errors);
    for (int lv = 2 * g.k - 2; lv >= 0; --lv) {
        const size_t h = (size_t)(g.S >> (lv >> 1)), nr = g.ch / h, nc = g.cw / h;
        const size_t lanes = (lv & 1) ? (nr + 1) * nc + nr * (nc + 1) : nr * nc;
        DSM_LAUNCH(me_saturate, lanes, ME_THREADS, s, g, lv, errors);
    }
    return SMVS_OK;
}

SMVS_EXPORT int smvs_dsm_mesh_count(const long long* errors, const float* dsm, int gw, int gh, float nodata, int tile,
                                    long long threshold, int* counts, void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!errors || !dsm || !counts || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (threshold < 0) return fail(SMVS_ERR_ARG, "threshold must be >= 0, got %lld", threshold);
    const size_t n = gw > 0 && gh > 0 ? (size_t)gw * gh : 0;
    const MeshWorkspace w = mesh_workspace(gw > 0 ? gw : 1, gh > 0 ? gh : 1);
    const DsmBuf buf[] = {{errors, n * 8, "errors"}, {dsm, n * 4, "dsm"}, {counts, 8, "counts"}, {workspace, w.bytes, "workspace"}};
    if (int rc = mesh_check(gw, gh, tile, buf, 4, true, workspace_bytes)) return rc;
    const MeGrid g = mesh_grid(gw, gh, tile);
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)workspace;
    if (int rc = mesh_emit(dsm, errors, g, nodata, threshold, w, base, true, s)) return rc;
    int* totals = (int*)(base + w.totals);
    if (int rc = ol_scan_exclusive((int*)(base + w.count), (unsigned)w.n_slots, nullptr, (int*)(base + w.s1), (int*)(base + w.s2), totals, s,
                                   "dsm_mesh_count (triangle scan)"))
        return rc;
    if (int rc = ol_scan_exclusive((int*)(base + w.used), (unsigned)n, nullptr, (int*)(base + w.s1), (int*)(base + w.s2), totals + 1, s,
                                   "dsm_mesh_count (vertex scan)"))
        return rc;
    DSM_LAUNCH(mc_totals, 64, 64, s, (const int*)totals, counts);
    return SMVS_OK;
}

SMVS_EXPORT int smvs_dsm_mesh_write(const float* dsm, int gw, int gh, int tile, int n_triangles, int n_vertices, int* triangles,
                                    unsigned char* tri_level, int* vertices, float* z, int* status, void* workspace,
                                    size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!dsm || !status || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (n_triangles < 0 || n_vertices < 0) return fail(SMVS_ERR_ARG, "negative counts (%d triangles, %d vertices)", n_triangles, n_vertices);
    if ((n_triangles && (!triangles || !tri_level)) || (n_vertices && (!vertices || !z))) return fail(SMVS_ERR_ARG, "null pointer argument");
    const size_t n = gw > 0 && gh > 0 ? (size_t)gw * gh : 0;
    const MeshWorkspace w = mesh_workspace(gw > 0 ? gw : 1, gh > 0 ? gh : 1);
    const size_t nt = (size_t)n_triangles, nv = (size_t)n_vertices;
    const DsmBuf buf[] = {{dsm, n * 4, "dsm"}, {triangles, nt * 12, "triangles"}, {tri_level, nt, "tri_level"}, {vertices, nv * 8, "vertices"},
                          {z, nv * 4, "z"}, {status, 4, "status"}, {workspace, w.bytes, "workspace"}};
    if (int rc = mesh_check(gw, gh, tile, buf, 7, true, workspace_bytes)) return rc;
    if (nt > 2 * n || nv > n) return fail(SMVS_ERR_ARG, "more triangles or vertices than the grid holds (%d, %d)", n_triangles, n_vertices);
    const MeGrid g = mesh_grid(gw, gh, tile);
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)workspace;
    const int* totals = (const int*)(base + w.totals);
    DSM_LAUNCH(mw_triangles, w.n_slots, ME_THREADS, s, g, (unsigned)w.n_slots, totals, n_triangles, n_vertices, (const int*)(base + w.count),
               (const unsigned char*)(base + w.masks), (const int*)(base + w.used), triangles, tri_level, status);
    DSM_LAUNCH(mw_vertices, n, ME_THREADS, s, dsm, g, totals, n_triangles, n_vertices, (const int*)(base + w.used), vertices, z);
    return SMVS_OK;
}

SMVS_EXPORT int smvs_dsm_mesh_heights(const long long* errors, const float* dsm, int gw, int gh, float nodata, int tile,
                                      long long threshold, float* heights, long long* dev, void* workspace, size_t workspace_bytes,
                                      void* stream)
{
    using namespace smvs;
    if (!errors || !dsm || !heights || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (threshold < 0) return fail(SMVS_ERR_ARG, "threshold must be >= 0, got %lld", threshold);
    const size_t n = gw > 0 && gh > 0 ? (size_t)gw * gh : 0;
    const MeshWorkspace w = mesh_workspace(gw > 0 ? gw : 1, gh > 0 ? gh : 1);
    const DsmBuf buf[] = {{errors, n * 8, "errors"}, {dsm, n * 4, "dsm"}, {heights, n * 4, "heights"}, {dev, n * 8, "dev"},
                          {workspace, w.bytes, "workspace"}};
    if (int rc = mesh_check(gw, gh, tile, buf, 5, true, workspace_bytes)) return rc;
    const MeGrid g = mesh_grid(gw, gh, tile);
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)workspace;
    if (int rc = mesh_emit(dsm, errors, g, nodata, threshold, w, base, false, s)) return rc;
    DSM_LAUNCH(mh_walk, n, ME_THREADS, s, dsm, errors, g, nodata, threshold, (const int*)(base + w.used), heights, dev);
    return SMVS_OK;
}

}  // extern "C"
