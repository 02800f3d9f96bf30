// dsm_facet.hip -- planar facets of a DSM and the least-squares plane of every facet ("Facets";
// include/satmvs.h for the rule).
//
//   smvs_dsm_facet_normals  the 3 x 3 integer gradient (Gx, Gy) of every cell and whether its window is planar within T
//   smvs_dsm_facet_label    facets = classes of the transitive closure of pairwise links between planar neighbours, numbered
//                           1 .. n in raster order of their first planar cell; optionally one round of growth onto the rim
//   smvs_dsm_facet_planes   per facet: exact int64 moments about an integer centre, the plane in float64, its residuals
//
// Labelling has the structure of dsm_label.hip: dsm_facet_cells (the kernel of smvs_dsm_facet_normals) leaves q, Gx, Gy and the
// planar flag of every cell in the workspace; (a) dsm_facet_tile labels a 64 x 16 tile in LDS, row runs from one ballot per row
// of the bit "linked to my west neighbour", then every link to the row above united with LDS min atomics; (b) dsm_facet_border
// unites the linked pairs across tile edges with 32-bit min atomics on the parent array, which is the labels buffer; (c)
// dsm_facet_flatten; (d) roots flagged, ranked by the three-level scan of dsm_scan.h, every cell takes rank[root] + 1; (e)
// dsm_facet_grow, one lane per cell.  A union only lowers a parent, so a facet's root is its first planar cell in raster order
// under any order of the atomics, and the result depends on the inputs alone.  Unlike foreground adjacency a link is not
// transitive over a 2 x 2 block, so (a) tests every pair and skips none; label_union finds both roots first and touches no
// atomic where they agree.  The find and union loops are bounded by construction (dsm_unionfind.h); a lane that meets a
// damaged parent array sets the error word and dsm_facet_final writes n = -1.
//
// The tile holds q, Gx, Gy and the parents of its own 1024 cells, 16 KB of LDS and no halo: a link inside the tile reads
// nothing beyond it, and the pairs across an edge are read from the workspace by (b).  Row-major with lane = column, so every
// LDS access of a wave is 64 consecutive words.
//
// Integer widths: |q| <= 2^23, so |Gx|, |Gy| <= 2^26; the planarity residual |8 (q_k - q_p) - (Gx dx + Gy dy)| <= 2^28 and the
// link residual |16 (q_n - q_p) - ((Gx_p + Gx_n) dx + (Gy_p + Gy_n) dy)| <= 2^29 + 2^28; with T <= 2^26 every term fits an int32.
#include <limits.h>
#include <stdint.h>

#include "dsm_common.h"
#include "dsm_flow.h"
#include "dsm_scan.h"
#include "dsm_unionfind.h"
#include "smvs_host.h"

namespace smvs {

constexpr int FACET_TW = 64, FACET_TH = 16, FACET_THREADS = 256;         // a tile row is one wave
constexpr int FACET_VOID = INT_MIN;                                      // q of a cell without a height
constexpr int FACET_MAX_TERM = 1 << 26;                                  // T, Ax, Ay
constexpr int FACET_ROWS = 16;                                           // rows of the 64-column strip one wave of the moments walks down
constexpr int FACET_MAX_SIDE = 32768, FACET_MAX_CELLS = 1 << 24;         // smvs_dsm_facet_planes (include/satmvs.h has the sum)

struct FacetTerms { int T8, T16, Ax, Ay; };

__device__ __forceinline__ bool facet_height(const float* __restrict__ dsm, const unsigned char* __restrict__ mask, size_t i, float nodata, int& q)
{
    if (mask && mask[i] == 0) return false;
    return dsm_quantum(dsm[i], nodata, q);
}

// The link of two planar neighbours, (dx, dy) the offset from p to n; symmetric under swapping them.
__device__ __forceinline__ bool facet_link(int qp, int gxp, int gyp, int qn, int gxn, int gyn, int dx, int dy, const FacetTerms& t)
{
    return abs(gxp - gxn) <= t.Ax && abs(gyp - gyn) <= t.Ay && abs(16 * (qn - qp) - ((gxp + gxn) * dx + (gyp + gyn) * dy)) <= t.T16;
}

// One lane per cell: the window, Gx, Gy and the planar flag; with Q, the cell's own q (FACET_VOID without a height).
__global__ __launch_bounds__(FACET_THREADS)
void dsm_facet_cells(const float* __restrict__ dsm, const unsigned char* __restrict__ mask, int gw, int gh, float nodata, int T8,
                 int* __restrict__ Q, int* __restrict__ Gx, int* __restrict__ Gy, unsigned char* __restrict__ planar)
{
    const unsigned ncells = (unsigned)gw * (unsigned)gh, c = blockIdx.x * (unsigned)FACET_THREADS + threadIdx.x;
    if (c >= ncells) return;
    const int y = (int)(c / (unsigned)gw), x = (int)(c % (unsigned)gw);
    int q[9];                                                // NW N NE, W p E, SW S SE
    bool all = true, own = false;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
        q[k] = 0;
        const bool ok = yy >= 0 && yy < gh && xx >= 0 && xx < gw && facet_height(dsm, mask, (size_t)yy * gw + xx, nodata, q[k]);
        all = all && ok;
        if (k == 4) own = ok;
    }
    int gx = 0, gy = 0;
    bool pl = false;
    if (all) {
        gx = (q[2] + 2 * q[5] + q[8]) - (q[0] + 2 * q[3] + q[6]);
        gy = (q[6] + 2 * q[7] + q[8]) - (q[0] + 2 * q[1] + q[2]);
        pl = true;
#pragma unroll
        for (int k = 0; k < 9; ++k)
            if (k != 4 && abs(8 * (q[k] - q[4]) - (gx * (k % 3 - 1) + gy * (k / 3 - 1))) > T8) pl = false;
    }
    if (Q) Q[c] = own ? q[4] : FACET_VOID;
    Gx[c] = gx;
    Gy[c] = gy;
    planar[c] = pl ? 1 : 0;
}

// (a) One 64 x 16 tile.  Wave w labels rows w, w + 4, ... : lane = column.
__global__ __launch_bounds__(FACET_THREADS)
void dsm_facet_tile(const int* __restrict__ Q, const int* __restrict__ Gx, const int* __restrict__ Gy, const unsigned char* __restrict__ planar,
                int gw, int gh, int conn8, FacetTerms t, int* __restrict__ parent, int* err)
{
    __shared__ int L[FACET_TW * FACET_TH], sq[FACET_TW * FACET_TH], sgx[FACET_TW * FACET_TH], sgy[FACET_TW * FACET_TH];
    const unsigned ntx = (unsigned)((gw + FACET_TW - 1) / FACET_TW);
    const int tx0 = (int)(blockIdx.x % ntx) * FACET_TW, ty0 = (int)(blockIdx.x / ntx) * FACET_TH;
    const int lx = threadIdx.x % FACET_TW, x = tx0 + lx;
    for (int ly = threadIdx.x / FACET_TW; ly < FACET_TH; ly += FACET_THREADS / FACET_TW) {
        const int y = ty0 + ly;
        const size_t c = (size_t)y * gw + x;
        const bool pl = x < gw && y < gh && planar[c] != 0;
        const int q = pl ? Q[c] : 0, gx = pl ? Gx[c] : 0, gy = pl ? Gy[c] : 0;
        const int wq = __shfl_up(q, 1), wgx = __shfl_up(gx, 1), wgy = __shfl_up(gy, 1), wpl = __shfl_up((int)pl, 1);
        const bool west = pl && lx > 0 && wpl && facet_link(wq, wgx, wgy, q, gx, gy, 1, 0, t);
        const unsigned long long linked = __ballot(west);
        const unsigned long long clear = ~linked & (lx == 63 ? ~0ull : ((2ull << lx) - 1ull));   // bit 0 is always clear
        const int start = 63 - __clzll((long long)clear);    // the highest cell at or left of this one that is not linked westwards
        const int i = ly * FACET_TW + lx;
        L[i] = pl ? ly * FACET_TW + start : -1;
        sq[i] = q;
        sgx[i] = gx;
        sgy[i] = gy;
    }
    __syncthreads();
    for (int i = threadIdx.x + FACET_TW; i < FACET_TW * FACET_TH; i += FACET_THREADS) {
        if (L[i] < 0) continue;                              // the sign of a cell never changes
        const int q = sq[i], gx = sgx[i], gy = sgy[i];
        int j = i - FACET_TW;
        if (L[j] >= 0 && facet_link(q, gx, gy, sq[j], sgx[j], sgy[j], 0, -1, t)) label_union<true>(L, i, j, err);
        if (conn8) {
            j = i - FACET_TW - 1;
            if (lx > 0 && L[j] >= 0 && facet_link(q, gx, gy, sq[j], sgx[j], sgy[j], -1, -1, t)) label_union<true>(L, i, j, err);
            j = i - FACET_TW + 1;
            if (lx < FACET_TW - 1 && L[j] >= 0 && facet_link(q, gx, gy, sq[j], sgx[j], sgy[j], 1, -1, t)) label_union<true>(L, i, j, err);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < FACET_TW * FACET_TH; i += FACET_THREADS) {
        const int y = ty0 + i / FACET_TW;
        if (x >= gw || y >= gh) continue;
        int p = -1;
        if (L[i] >= 0) {
            const int r = label_find<true>(L, i, err);       // the lowest local index is the lowest global index of the tile
            p = (ty0 + r / FACET_TW) * gw + tx0 + r % FACET_TW;
        }
        parent[(size_t)y * gw + x] = p;
    }
}

struct FacetCells { const int *Q, *Gx, *Gy; };

// c and nb = c + dy gw + dx, both on the grid: united if nb is planar and the link holds (c is planar).
__device__ __forceinline__ void facet_join(int* parent, const FacetCells& f, int c, int nb, int dx, int dy, const FacetTerms& t, int* err)
{
    if (parent[nb] >= 0 && facet_link(f.Q[c], f.Gx[c], f.Gy[c], f.Q[nb], f.Gx[nb], f.Gy[nb], dx, dy, t)) label_union<false>(parent, c, nb, err);
}

// (b) Lanes 0 .. nh - 1: the cells of the first row of every tile row but the topmost, with N (and NW, NE).  Lanes nh .. nh +
// nv - 1: the cells of the first column of every tile column but the leftmost, with W (and NW, SW).  Every pair of adjacent
// cells in different tiles is one of these.
__global__ __launch_bounds__(FACET_THREADS)
void dsm_facet_border(int* parent, FacetCells f, int gw, int gh, int conn8, FacetTerms t, unsigned nh, unsigned nv, int* err)
{
    const unsigned id = blockIdx.x * (unsigned)FACET_THREADS + threadIdx.x;
    if (id >= nh + nv) return;
    int x, y;
    const bool horizontal = id < nh;
    if (horizontal) {
        y = (int)(id / (unsigned)gw + 1u) * FACET_TH;
        x = (int)(id % (unsigned)gw);
    } else {
        const unsigned u = id - nh;
        x = (int)(u / (unsigned)gh + 1u) * FACET_TW;
        y = (int)(u % (unsigned)gh);
    }
    const int c = y * gw + x;
    if (parent[c] < 0) return;                               // tile roots from (a): written before this launch, never negative later
    if (horizontal) {
        facet_join(parent, f, c, c - gw, 0, -1, t, err);
        if (conn8) {
            if (x > 0) facet_join(parent, f, c, c - gw - 1, -1, -1, t, err);
            if (x + 1 < gw) facet_join(parent, f, c, c - gw + 1, 1, -1, t, err);
        }
    } else {
        facet_join(parent, f, c, c - 1, -1, 0, t, err);
        if (conn8) {
            if (y > 0) facet_join(parent, f, c, c - gw - 1, -1, -1, t, err);
            if (y + 1 < gh) facet_join(parent, f, c, c + gw - 1, -1, 1, t, err);
        }
    }
}

// (c) Every cell takes its root.  Other lanes may read this cell's parent meanwhile: they see the old parent or the root,
// both in the tree and both below the cell, and a root's own entry is never written.
__global__ __launch_bounds__(FACET_THREADS)
void dsm_facet_flatten(int* parent, unsigned ncells, int* err)
{
    const unsigned c = blockIdx.x * (unsigned)FACET_THREADS + threadIdx.x;
    if (c >= ncells) return;
    const int p = ld_agent(parent + c);
    if (p < 0 || p == (int)c) return;
    const int r = label_find<false>(parent, p, err);
    if (r != p) __hip_atomic_store(parent + c, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (d1) 1 at every root, for the scan.
__global__ __launch_bounds__(FACET_THREADS)
void dsm_facet_roots(const int* __restrict__ parent, unsigned ncells, int* __restrict__ rank)
{
    const unsigned c = blockIdx.x * (unsigned)FACET_THREADS + threadIdx.x;
    if (c < ncells) rank[c] = parent[c] == (int)c;
}

// (d2) label = rank of the root in raster order + 1, in place over the parents; n, or -1 after a bounded loop gave up.
__global__ __launch_bounds__(FACET_THREADS)
void dsm_facet_final(int* __restrict__ labels, unsigned ncells, const int* __restrict__ rank, const int* __restrict__ total_err, int* __restrict__ n_out)
{
    const unsigned c = blockIdx.x * (unsigned)FACET_THREADS + threadIdx.x;
    if (c == 0) *n_out = total_err[1] ? -1 : total_err[0];
    if (c >= ncells) return;
    const int p = labels[c];                                 // this lane's own cell: no other lane reads or writes it
    labels[c] = (p >= 0 && (unsigned)p <= c) ? rank[p] + 1 : 0;
}

// (e) One round of growth: a cell with a height that is not planar takes the label of its first neighbour k = 0 .. 7 (d8_dc,
// d8_dr) that is planar and whose plane passes within T of it.  Reads the labels of planar cells only and writes those of
// the others only, so in place.
__global__ __launch_bounds__(FACET_THREADS)
void dsm_facet_grow(int* labels, FacetCells f, const unsigned char* __restrict__ planar, int gw, int gh, int T8)
{
    const unsigned ncells = (unsigned)gw * (unsigned)gh, c = blockIdx.x * (unsigned)FACET_THREADS + threadIdx.x;
    if (c >= ncells) return;
    const int qu = f.Q[c];
    if (qu == FACET_VOID || planar[c]) return;
    const int y = (int)(c / (unsigned)gw), x = (int)(c % (unsigned)gw);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int yy = y + d8_dr(k), xx = x + d8_dc(k);
        if (yy < 0 || yy >= gh || xx < 0 || xx >= gw) continue;
        const int p = yy * gw + xx;
        if (!planar[p]) continue;
        if (abs(8 * (qu - f.Q[p]) - (f.Gx[p] * -d8_dc(k) + f.Gy[p] * -d8_dr(k))) <= T8) {   // the offset from p to u is minus k's
            labels[c] = labels[p];
            return;
        }
    }
}

struct FacetWorkspace { size_t Q, Gx, Gy, planar, rank, s1, s2, tail, bytes; };

static FacetWorkspace facet_workspace(size_t ncells)
{
    FacetWorkspace w;
    const size_t nb1 = (ncells + OL_BLOCK - 1) / OL_BLOCK, nb2 = (nb1 + OL_BLOCK - 1) / OL_BLOCK;
    w.Q = 0;
    w.Gx = w.Q + align256(ncells * sizeof(int));
    w.Gy = w.Gx + align256(ncells * sizeof(int));
    w.planar = w.Gy + align256(ncells * sizeof(int));
    w.rank = w.planar + align256(ncells);
    w.s1 = w.rank + align256(ncells * sizeof(int));
    w.s2 = w.s1 + align256(nb1 * sizeof(int));
    w.tail = w.s2 + align256(nb2 * sizeof(int));             // [0] the total, [1] the error word
    w.bytes = w.tail + 256;
    return w;
}

// ---- planes --------------------------------------------------------------------------------------------------------------------
// What a lane holds of one label: NV int64 sums and a maximum.  Integers only, so any grouping gives the same bits.
template <int NV>
struct FacetAcc {
    long long v[NV];
    int mx;

    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = 0;
        mx = 0;
    }
    __device__ __forceinline__ void add(const FacetAcc& o)
    {
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] += o.v[j];
        mx = max(mx, o.mx);
    }
    __device__ __forceinline__ FacetAcc down(int d) const
    {
        FacetAcc o;
#pragma unroll
        for (int j = 0; j < NV; ++j) o.v[j] = __shfl_down(v[j], d);
        o.mx = __shfl_down(mx, d);
        return o;
    }
};

// Hand the accumulators of the lanes in `give` to memory, as label_stats_flush of dsm_label.hip does: lanes side by side that
// give the same label form a run, the run is reduced onto its first lane and that lane alone goes to memory.
template <int NV>
__device__ __forceinline__ void facet_flush(FacetAcc<NV>& acc, int lab, bool give, unsigned long long* __restrict__ out, int* __restrict__ out_max)
{
    const int lane = threadIdx.x & 63;
    const int prev = __shfl_up(lab, 1);
    const unsigned long long gives = __ballot(give);
    const bool head = give && (lane == 0 || !((gives >> (lane - 1)) & 1ull) || prev != lab);
    const unsigned long long heads = __ballot(head);
    const unsigned long long upto = heads & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));      // heads at or before this lane
    const int start = give && upto ? 63 - __clzll((long long)upto) : -1 - lane;                  // lanes that give nothing: unique
    FacetAcc<NV> r = acc;
    if (!give) r.clear();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const FacetAcc<NV> n = r.down(d);
        const int nstart = __shfl_down(start, d);
        if (lane + d < 64 && nstart == start) r.add(n);
    }
    if (head) {
        const size_t k = (size_t)(lab - 1);
#pragma unroll
        for (int j = 0; j < NV; ++j)
            if (r.v[j] != 0) atomicAdd(out + NV * k + j, (unsigned long long)r.v[j]);
        if (out_max && r.mx > 0) atomicMax(out_max + k, r.mx);
    }
    if (give) acc.clear();
}

// MODE 0: n, sum c, sum r, sum q.  MODE 1: the eight sums of dc, dr, dq, dc^2, dc dr, dr^2, dc dq, dr dq about the integer
// centre.  MODE 2: sum e^2 and max |e| of e = q - rn(h0 + a dc + b dr), clamped.  A wave walks down a strip of 64 columns and
// FACET_ROWS rows, lane = column; a lane keeps accumulating while the label in its column stays.
template <int MODE>
__global__ __launch_bounds__(FACET_THREADS)
void dsm_facet_moments(const int* __restrict__ labels, const float* __restrict__ dsm, int gw, int gh, float nodata, int n,
                   const int* __restrict__ centre, const double* __restrict__ plane, unsigned long long* __restrict__ out, int* __restrict__ out_max)
{
    constexpr int NV = MODE == 0 ? 4 : MODE == 1 ? 8 : 1;
    const unsigned nsx = (unsigned)((gw + 63) / 64);
    const unsigned strip = blockIdx.x * (unsigned)(FACET_THREADS / 64) + (threadIdx.x >> 6);
    const int x = (int)(strip % nsx) * 64 + (int)(threadIdx.x & 63), y0 = (int)(strip / nsx) * FACET_ROWS;
    if (y0 >= gh) return;                                    // whole waves only
    FacetAcc<NV> acc;
    acc.clear();
    int held = 0, cb = 0, rb = 0, qb = 0;
    double a = 0.0, b = 0.0, h0 = 0.0;
    const int y1 = min(y0 + FACET_ROWS, gh);
    for (int y = y0; y < y1; ++y) {
        int lab = 0, q = 0;
        if (x < gw) {
            const size_t c = (size_t)y * gw + x;
            lab = labels[c];
            if ((unsigned)lab - 1u >= (unsigned)n || !dsm_quantum(dsm[c], nodata, q)) lab = 0;   // 0, negative, above n, no height: nothing
        }
        const bool change = lab != held;
        if (__any(change && held != 0)) facet_flush<NV>(acc, held, change && held != 0, out, out_max);
        held = lab;
        if (lab == 0) continue;
        if constexpr (MODE >= 1) if (change) {
            cb = centre[3 * (size_t)(lab - 1)]; rb = centre[3 * (size_t)(lab - 1) + 1]; qb = centre[3 * (size_t)(lab - 1) + 2];
        }
        if constexpr (MODE == 2) if (change) {
            a = plane[3 * (size_t)(lab - 1)]; b = plane[3 * (size_t)(lab - 1) + 1]; h0 = plane[3 * (size_t)(lab - 1) + 2];
        }
        if constexpr (MODE == 0) {
            acc.v[0] += 1; acc.v[1] += x; acc.v[2] += y; acc.v[3] += q;
        } else if constexpr (MODE == 1) {
            const long long dc = x - cb, dr = y - rb, dq = (long long)q - qb;
            acc.v[0] += dc; acc.v[1] += dr; acc.v[2] += dq; acc.v[3] += dc * dc; acc.v[4] += dc * dr; acc.v[5] += dr * dr;
            acc.v[6] += dc * dq; acc.v[7] += dr * dq;
        } else if (h0 == h0) {                               // a NaN plane has no residuals
            const double at = (h0 + a * (double)(x - cb)) + b * (double)(y - rb);
            const long long e = min(max((long long)q - __double2ll_rn(fmin(fmax(at, -1099511627776.0), 1099511627776.0)), -65536ll), 65536ll);
            acc.v[0] += e * e;
            acc.mx = max(acc.mx, (int)(e < 0 ? -e : e));
        }
    }
    if (__any(held != 0)) facet_flush<NV>(acc, held, held != 0, out, out_max);
}

__device__ __forceinline__ long long floor_div(long long a, long long b)                         // b > 0
{
    const long long q = a / b;
    return (a % b < 0) ? q - 1 : q;
}

// centre[k] = floor(sum c / n), floor(sum r / n), floor(sum q / n); zeros for a label without a cell.
__global__ __launch_bounds__(FACET_THREADS)
void dsm_facet_centre(int n, const long long* __restrict__ sums, int* __restrict__ centre)
{
    const int k = blockIdx.x * FACET_THREADS + threadIdx.x;
    if (k >= n) return;
    const long long m = sums[4 * (size_t)k];
#pragma unroll
    for (int j = 0; j < 3; ++j) centre[3 * (size_t)k + j] = m > 0 ? (int)floor_div(sums[4 * (size_t)k + 1 + j], m) : 0;
}

// The plane of every label from n and the eight centred sums, in the operation order of include/satmvs.h (no contraction).
__global__ __launch_bounds__(FACET_THREADS)
void dsm_facet_fit(int n, const long long* __restrict__ sums, const int* __restrict__ centre, const long long* __restrict__ mom, double* __restrict__ plane)
{
    const int k = blockIdx.x * FACET_THREADS + threadIdx.x;
    if (k >= n) return;
    const long long* m = mom + 8 * (size_t)k;
    const double N = (double)sums[4 * (size_t)k];
    const double Sx = (double)m[0], Sy = (double)m[1], Sz = (double)m[2], Sxx = (double)m[3], Sxy = (double)m[4], Syy = (double)m[5];
    const double Sxz = (double)m[6], Syz = (double)m[7];
    const double cxx = Sxx - (Sx * Sx) / N, cxy = Sxy - (Sx * Sy) / N, cyy = Syy - (Sy * Sy) / N;
    const double cxz = Sxz - (Sx * Sz) / N, cyz = Syz - (Sy * Sz) / N;
    const double det = cxx * cyy - cxy * cxy;
    double a = __builtin_nan(""), b = a, h0 = a;
    if (det > 0.0) {
        a = (cxz * cyy - cyz * cxy) / det;
        b = (cyz * cxx - cxz * cxy) / det;
        h0 = (double)centre[3 * (size_t)k + 2] + ((Sz / N - a * (Sx / N)) - b * (Sy / N));
    }
    plane[3 * (size_t)k] = a;
    plane[3 * (size_t)k + 1] = b;
    plane[3 * (size_t)k + 2] = h0;
}

static const char* facet_terms_check(int T, int Ax, int Ay)
{
    if (T < 0 || T > FACET_MAX_TERM) return "T must be in 0 .. 2^26";
    if (Ax < 0 || Ax > FACET_MAX_TERM || Ay < 0 || Ay > FACET_MAX_TERM) return "Ax and Ay must be in 0 .. 2^26";
    return nullptr;
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT int smvs_dsm_facet_normals(const float* dsm, const unsigned char* mask, int gw, int gh, float nodata, int T,
                                       int* Gx, int* Gy, unsigned char* planar, void* stream)
{
    using namespace smvs;
    if (!dsm || !Gx || !Gy || !planar) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (const char* msg = facet_terms_check(T, 0, 0)) return fail(SMVS_ERR_ARG, "%s, got %d", msg, T);
    const size_t ncells = (size_t)gw * gh;
    const DsmBuf buf[] = {{dsm, ncells * 4, "dsm"}, {mask, ncells, "mask"}, {Gx, ncells * 4, "Gx"}, {Gy, ncells * 4, "Gy"}, {planar, ncells, "planar"}};
    const char* other;
    if (const char* name = dsm_first_alias(buf, 5, other)) return fail(SMVS_ERR_ARG, "%s aliases %s", name, other);
    hipStream_t s = (hipStream_t)stream;
    DSM_LAUNCH(dsm_facet_cells, ncells, FACET_THREADS, s, dsm, mask, gw, gh, nodata, 8 * T, (int*)nullptr, Gx, Gy, planar);
    return SMVS_OK;
}

SMVS_EXPORT size_t smvs_dsm_facet_workspace_bytes(int gw, int gh)
{
    using namespace smvs;
    if (grid_check(gw, gh)) return 0;
    return facet_workspace((size_t)gw * gh).bytes;
}

SMVS_EXPORT int smvs_dsm_facet_label(const float* dsm, const unsigned char* mask, int gw, int gh, float nodata, int T, int Ax, int Ay,
                                     int connectivity, int grow, int* labels, int* n_out,
                                     void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!dsm || !labels || !n_out || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (const char* msg = facet_terms_check(T, Ax, Ay)) return fail(SMVS_ERR_ARG, "%s, got T %d, Ax %d, Ay %d", msg, T, Ax, Ay);
    if (connectivity != 4 && connectivity != 8) return fail(SMVS_ERR_ARG, "connectivity must be 4 or 8, got %d", connectivity);
    if (grow != 0 && grow != 1) return fail(SMVS_ERR_ARG, "grow must be 0 or 1, got %d", grow);
    const size_t ncells = (size_t)gw * gh;
    const FacetWorkspace w = facet_workspace(ncells);
    if (workspace_bytes < w.bytes) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, w.bytes);
    const DsmBuf buf[] = {{dsm, ncells * 4, "dsm"}, {mask, ncells, "mask"}, {labels, ncells * 4, "labels"}, {n_out, 4, "n_out"}, {workspace, w.bytes, "workspace"}};
    const char* other;
    if (const char* name = dsm_first_alias(buf, 5, other)) return fail(SMVS_ERR_ARG, "%s aliases %s", name, other);
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)workspace;
    int *Q = (int*)(base + w.Q), *Gx = (int*)(base + w.Gx), *Gy = (int*)(base + w.Gy), *rank = (int*)(base + w.rank);
    int *s1 = (int*)(base + w.s1), *s2 = (int*)(base + w.s2), *tail = (int*)(base + w.tail), *err = tail + 1;
    unsigned char* planar = (unsigned char*)(base + w.planar);
    const FacetCells cells = {Q, Gx, Gy};
    const FacetTerms t = {8 * T, 16 * T, Ax, Ay};
    const int conn8 = connectivity == 8;
    if (hipMemsetAsync(tail, 0, 2 * sizeof(int), s) != hipSuccess) return check_launch("dsm_facet_label (clearing the error word)");
    DSM_LAUNCH(dsm_facet_cells, ncells, FACET_THREADS, s, dsm, mask, gw, gh, nodata, t.T8, Q, Gx, Gy, planar);
    const unsigned ntx = (unsigned)((gw + FACET_TW - 1) / FACET_TW), nty = (unsigned)((gh + FACET_TH - 1) / FACET_TH);
    DSM_LAUNCH(dsm_facet_tile, (size_t)ntx * nty * FACET_THREADS, FACET_THREADS, s, (const int*)Q, (const int*)Gx, (const int*)Gy, (const unsigned char*)planar,
               gw, gh, conn8, t, labels, err);
    const unsigned nh = (nty - 1) * (unsigned)gw, nv = (ntx - 1) * (unsigned)gh;         // both below 2^31 / 16
    if (nh + nv) DSM_LAUNCH(dsm_facet_border, (size_t)nh + nv, FACET_THREADS, s, labels, cells, gw, gh, conn8, t, nh, nv, err);
    DSM_LAUNCH(dsm_facet_flatten, ncells, FACET_THREADS, s, labels, (unsigned)ncells, err);
    DSM_LAUNCH(dsm_facet_roots, ncells, FACET_THREADS, s, (const int*)labels, (unsigned)ncells, rank);
    if (int rc = ol_scan_exclusive(rank, (unsigned)ncells, nullptr, s1, s2, tail, s, "dsm_facet_label (scan)")) return rc;
    DSM_LAUNCH(dsm_facet_final, ncells, FACET_THREADS, s, labels, (unsigned)ncells, (const int*)rank, (const int*)tail, n_out);
    if (grow) DSM_LAUNCH(dsm_facet_grow, ncells, FACET_THREADS, s, labels, cells, (const unsigned char*)planar, gw, gh, t.T8);
    return SMVS_OK;
}

SMVS_EXPORT int smvs_dsm_facet_planes(const int* labels, const float* dsm, int gw, int gh, float nodata, int n,
                                      long long* sums, int* centre, long long* moments, double* plane,
                                      long long* sse, int* max_abs, void* stream)
{
    using namespace smvs;
    if (!labels || !dsm || !sums || !centre || !moments || !plane || !sse || !max_abs) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (gw < 1 || gh < 1) return fail(SMVS_ERR_ARG, "non-positive grid size");
    if (gw > FACET_MAX_SIDE || gh > FACET_MAX_SIDE || (long long)gw * gh >= FACET_MAX_CELLS)
        return fail(SMVS_ERR_ARG, "grid too large: gw, gh <= 32768 and gw * gh < 2^24, got %d x %d", gw, gh);
    if (n < 0) return fail(SMVS_ERR_ARG, "n must be >= 0, got %d", n);
    if (n == 0) return SMVS_OK;
    const size_t ncells = (size_t)gw * gh, m = (size_t)n;
    const DsmBuf buf[] = {{labels, ncells * 4, "labels"}, {dsm, ncells * 4, "dsm"}, {sums, m * 32, "sums"}, {centre, m * 12, "centre"},
                          {moments, m * 64, "moments"}, {plane, m * 24, "plane"}, {sse, m * 8, "sse"}, {max_abs, m * 4, "max_abs"}};
    const char* other;
    if (const char* name = dsm_first_alias(buf, 8, other)) return fail(SMVS_ERR_ARG, "%s aliases %s", name, other);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(sums, 0, m * 32, s) != hipSuccess || hipMemsetAsync(moments, 0, m * 64, s) != hipSuccess ||
        hipMemsetAsync(sse, 0, m * 8, s) != hipSuccess || hipMemsetAsync(max_abs, 0, m * 4, s) != hipSuccess)
        return check_launch("dsm_facet_planes (clearing the sums)");
    const unsigned long long strips = (unsigned long long)((gw + 63) / 64) * (unsigned long long)((gh + FACET_ROWS - 1) / FACET_ROWS);
    const size_t lanes = (size_t)strips * 64;
    const double* no_plane = nullptr;
    const int* no_centre = nullptr;
    int* no_max = nullptr;
    DSM_LAUNCH((dsm_facet_moments<0>), lanes, FACET_THREADS, s, labels, dsm, gw, gh, nodata, n, no_centre, no_plane, (unsigned long long*)sums, no_max);
    DSM_LAUNCH(dsm_facet_centre, m, FACET_THREADS, s, n, (const long long*)sums, centre);
    DSM_LAUNCH((dsm_facet_moments<1>), lanes, FACET_THREADS, s, labels, dsm, gw, gh, nodata, n, (const int*)centre, no_plane, (unsigned long long*)moments, no_max);
    DSM_LAUNCH(dsm_facet_fit, m, FACET_THREADS, s, n, (const long long*)sums, (const int*)centre, (const long long*)moments, plane);
    DSM_LAUNCH((dsm_facet_moments<2>), lanes, FACET_THREADS, s, labels, dsm, gw, gh, nodata, n, (const int*)centre, (const double*)plane, (unsigned long long*)sse, max_abs);
    return SMVS_OK;
}

}  // extern "C"
