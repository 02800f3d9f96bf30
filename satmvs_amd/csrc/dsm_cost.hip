// dsm_cost.hip -- cost distance over a DSM grid on integers, exact ("Cost distance"; include/satmvs.h for
// the rule): the accumulated cost of the cheapest 8-connected trip from every cell to a source, and its back-links in the
// library's D8 codes, so that dsm_hydro.hip and dsm_stream.hip take the result as a flow forest.
//
//   smvs_dsm_cost_begin   the keys as the relaxation starts: sources 0, barriers all ones, the rest +infinity; n_sources
//   smvs_dsm_cost_rounds  `rounds` global rounds; status <- the tiles that changed in the last one
//   smvs_dsm_cost_read    keys -> raw, cost, backlink
//
// The relaxation.  A key is D, a uint64 in units of 2^-15 cost metre; all ones is a barrier and all ones - 1 is +infinity.  A
// round is one workgroup per tile of 32 x 32 cells: it loads the keys, the friction and (with a slope table) the heights of the
// tile and a halo of one cell into LDS, works out the eight step costs of each of a lane's four cells ONCE, and lowers every
// passable cell to min(own, min over the allowed steps of neighbour + w) until no cell of the tile moves (__syncthreads_or);
// the interior goes back to memory only if something moved.  The flood's argument (dsm_hydro.hip) carries over word for word.
// Keys start at or above the solution (sources at 0, which is their solution; the rest at +infinity) and a step replaces a key
// by neighbour + w, where the neighbour's key is at or above ITS solution: by induction no key ever passes below the solution,
// and keys only fall.  A stale key read from a neighbouring tile, or from another wave in LDS, is therefore an upper bound like
// any other, and a key moves as one aligned 64-bit access, so a torn value cannot appear.  A round in which no tile moved has
// read final halos only and found every cell at min(own, neighbour + w): the grid is at a fixed point of the key equation.
// Every step costs at least 1, so D strictly falls along any chain of minimising steps, which ends at a source: the fixed
// point below +infinity is the shortest-path cost and is unique; what the order of tiles and waves changes is the number of
// rounds, never a bit of the result.  A synchronous sweep finalises at least one more cell a round (the cheapest unfinished
// one), and a tile round does no less than a sweep, so gw gh + 2 rounds bound any grid.
//
// Choices.  (1) The step costs live in registers.  They do not change while a tile relaxes, the inner loop runs once per cell
// of the longest chain through the tile (tens of times), and a cost is an integer division, a dependent LDS look-up and a
// 64-bit product; recomputing it would put all three into that loop.  (2) The table-free form is its own instantiation: there
// T = 256 and w = max(1, (f_c + f_n) L >> 2) < 2^30, so a step cost is one 32-bit word instead of two and the tile needs
// neither heights nor table in LDS.  The compiler reports 96 VGPRs and 17 472 bytes of LDS with the table, 94 VGPRs and 11 824
// bytes without (it spends the words saved on keeping more LDS reads in flight): 5 waves a SIMD either way, set by the
// registers (512 / 96), that is 5 workgroups a CU where the LDS would hold 9 and 13.  (3) The LDS row pitch is the plain 34 keys.  A wave's
// ds_read_b64 is served in two groups of 32 lanes and ds_write_b64 in four of 16; a lane group reads 32 (writes 16) consecutive
// keys of one row, 256 (128) contiguous bytes, which is every bank once whatever the pitch, so padding buys nothing.  The
// int32 heights and the uint16 friction are read at setup only.  No kernel uses scratch; the only atomic is the per-launch
// counter of moved tiles.  Workspace: 16 KB of round counters, 1 KB for the table, 4 bytes per 256 cells for the source counts.
#include <limits.h>
#include <stdint.h>

#include <type_traits>

#include "dsm_common.h"
#include "dsm_flow.h"
#include "smvs_host.h"

namespace smvs {

typedef unsigned long long u64;

constexpr int CD_THREADS = D8_THREADS;
constexpr int CD_TILE = 32, CD_SPAN = CD_TILE + 2, CD_PITCH = CD_SPAN;              // interior, with halo, LDS row in keys
constexpr int CD_ROWS = CD_THREADS / CD_TILE, CD_PER_THREAD = CD_TILE / CD_ROWS;  // 8 rows of lanes, 4 cells a lane
constexpr int CD_MAX_ROUNDS = 4096, CD_TABLE = 256;
constexpr long long CD_MAX_CELLS = 1ll << 24;
constexpr u64 CD_BARRIER = ~0ull, CD_INF = ~0ull - 1;

struct CdTerms { int L[8]; int reverse; };                   // the eight step lengths [2^-8 m], passed by value
struct CdTable { int v[CD_TABLE]; };                         // the host's slope table, passed by value to cd_upload

// Whether cell i can be walked on; f its friction (256 without a grid) and q its height (0 without a DSM).
__device__ __forceinline__ bool cd_passable(const unsigned short* __restrict__ friction, const float* __restrict__ dsm, size_t i,
                                            float nodata, int& f, int& q)
{
    f = friction ? (int)friction[i] : 256;
    q = 0;
    return f != 0 && (!dsm || dsm_quantum(dsm[i], nodata, q));
}

// The table's bin of a step that rises by delta quanta over a length of len: clamp(floor(32 delta / len), -128, 127) + 128.
// |delta| <= 2^24, so 32 delta fits an int; the division truncates and the floor is put right.
__device__ __forceinline__ int cd_bin(int delta, int len)
{
    const int num = 32 * delta;
    int b = num / len;
    if (num % len < 0) --b;
    return min(max(b, -128), 127) + 128;
}

// The cost of the step c -> n over a length of len, 0 if the table forbids it.  `table` is null for T = 256.
__device__ __forceinline__ u64 cd_step(int fc, int fn, int qc, int qn, int len, int reverse, const int* table)
{
    u64 t = 256;
    if (table) {
        t = (u64)table[cd_bin(reverse ? qc - qn : qn - qc, len)];
        if (t == 0) return 0;
    }
    const u64 w = ((u64)(unsigned)(fc + fn) * (u64)(unsigned)len * t) >> 10;
    return w ? w : 1;
}

// ---- begin ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CD_THREADS)
void cd_begin(const unsigned short* __restrict__ friction, const unsigned char* __restrict__ sources, const float* __restrict__ dsm,
              unsigned n, float nodata, u64* __restrict__ keys, int* __restrict__ partial)
{
    const unsigned i = blockIdx.x * (unsigned)CD_THREADS + threadIdx.x;
    int source = 0;
    if (i < n) {
        int f, q;
        const bool open = cd_passable(friction, dsm, i, nodata, f, q);
        source = open && sources[i] != 0;
        keys[i] = !open ? CD_BARRIER : source ? 0ull : CD_INF;
    }
    const int count = __syncthreads_count(source);
    if (threadIdx.x == 0) partial[blockIdx.x] = count;
}

// One workgroup: the sum of the blocks' counts, in a fixed order.
__global__ __launch_bounds__(CD_THREADS)
void cd_count(const int* __restrict__ partial, unsigned n_partial, int* __restrict__ n_sources)
{
    __shared__ int part[CD_THREADS];
    int sum = 0;
    for (unsigned i = threadIdx.x; i < n_partial; i += CD_THREADS) sum += partial[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int half = CD_THREADS / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) part[threadIdx.x] += part[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_sources = part[0];
}

__global__ __launch_bounds__(CD_TABLE)
void cd_upload(CdTable t, int* __restrict__ table)
{
    table[threadIdx.x] = t.v[threadIdx.x];
}

// ---- a round -------------------------------------------------------------------------------------------------------------------
template <bool TABLE>
__global__ __launch_bounds__(CD_THREADS)
void cd_round(const unsigned short* __restrict__ friction, const float* __restrict__ dsm, int gw, int gh, float nodata, CdTerms terms,
              const int* __restrict__ table, u64* keys, int* __restrict__ moved)
{
    typedef typename std::conditional<TABLE, u64, unsigned>::type W;              // a step cost: below 2^38, without a table below 2^30
    __shared__ u64 tile[CD_SPAN * CD_PITCH];
    __shared__ unsigned short fric[CD_SPAN * CD_SPAN];
    __shared__ int height[TABLE ? CD_SPAN * CD_SPAN : 1];
    __shared__ int slope[TABLE ? CD_TABLE : 1];
    const unsigned across = ((unsigned)gw + CD_TILE - 1) / CD_TILE;               // the tiles in a row of tiles; the grid is 1-D
    const int r0 = (int)(blockIdx.x / across) * CD_TILE - 1, c0 = (int)(blockIdx.x % across) * CD_TILE - 1;       // the halo's corner
    for (int t = threadIdx.x; t < CD_SPAN * CD_SPAN; t += CD_THREADS) {
        const int lr = t / CD_SPAN, lc = t % CD_SPAN, r = r0 + lr, c = c0 + lc;
        const bool in = r >= 0 && r < gh && c >= 0 && c < gw;
        const size_t i = in ? (size_t)r * gw + c : 0;
        tile[lr * CD_PITCH + lc] = in ? keys[i] : CD_BARRIER;
        fric[t] = in ? (friction ? friction[i] : (unsigned short)256) : (unsigned short)0;
        if constexpr (TABLE) {
            int q = 0;
            if (in) dsm_quantum(dsm[i], nodata, q);          // a cell without a height is a barrier by its key; its q is never used
            height[t] = q;
        }
    }
    if constexpr (TABLE) slope[threadIdx.x] = table[threadIdx.x];      // CD_THREADS == CD_TABLE
    __syncthreads();
    const int lc = 1 + (int)(threadIdx.x % CD_TILE), lrow = 1 + (int)(threadIdx.x / CD_TILE);
    u64 own[CD_PER_THREAD];
    W w[CD_PER_THREAD][8];                                   // 0: no such step (a barrier beyond it, or the table says no)
    bool open[CD_PER_THREAD];                                // not a barrier: the cells that may move (a source never does)
#pragma unroll
    for (int j = 0; j < CD_PER_THREAD; ++j) {
        const int lr = lrow + j * CD_ROWS, at = lr * CD_PITCH + lc, fat = lr * CD_SPAN + lc;
        own[j] = tile[at];
        open[j] = own[j] != CD_BARRIER;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int nat = at + d8_dr(k) * CD_PITCH + d8_dc(k), nfat = fat + d8_dr(k) * CD_SPAN + d8_dc(k);
            u64 step = 0;
            if (open[j] && tile[nat] != CD_BARRIER)
                step = cd_step(fric[fat], fric[nfat], TABLE ? height[fat] : 0, TABLE ? height[nfat] : 0, terms.L[k], terms.reverse,
                               TABLE ? slope : nullptr);
            w[j][k] = (W)step;
        }
    }
    bool any = false;
    int busy;
    do {
        busy = 0;
#pragma unroll
        for (int j = 0; j < CD_PER_THREAD; ++j) {
            if (!open[j]) continue;
            const int at = (lrow + j * CD_ROWS) * CD_PITCH + lc;
            u64 low = own[j];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const u64 v = tile[at + d8_dr(k) * CD_PITCH + d8_dc(k)];
                const u64 through = v + (u64)w[j][k];        // v < CD_INF is below 2^62: no wrap
                low = (w[j][k] != 0 && v < CD_INF && through < low) ? through : low;
            }
            if (low < own[j]) {
                own[j] = low;
                tile[at] = low;
                busy = 1;
            }
        }
        any = any || busy;
        busy = __syncthreads_or(busy);
    } while (busy);
    const int tile_moved = __syncthreads_or(any);
    if (!tile_moved) return;
#pragma unroll
    for (int j = 0; j < CD_PER_THREAD; ++j)
        if (open[j]) keys[(size_t)(r0 + lrow + j * CD_ROWS) * gw + (c0 + lc)] = own[j];
    if (threadIdx.x == 0) atomicAdd(moved, 1);
}

__global__ void cd_status(const int* __restrict__ moved, int* __restrict__ status)
{
    if (threadIdx.x == 0) *status = *moved;
}

// ---- read ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CD_THREADS)
void cd_read(const unsigned short* __restrict__ friction, const float* __restrict__ dsm, int gw, int gh, float nodata, CdTerms terms,
             const int* __restrict__ table, const u64* __restrict__ keys, u64 max_cost, long long* __restrict__ raw,
             double* __restrict__ cost, unsigned char* __restrict__ backlink)
{
    const unsigned n = (unsigned)gw * (unsigned)gh, i = blockIdx.x * (unsigned)CD_THREADS + threadIdx.x;
    if (i >= n) return;
    const u64 own = keys[i];
    const bool barrier = own == CD_BARRIER, reached = own < CD_INF && own <= max_cost;
    if (raw) raw[i] = reached ? (long long)own : -1ll;
    if (cost) cost[i] = barrier ? __longlong_as_double(0x7ff8000000000000ll) : !reached ? __longlong_as_double(0x7ff0000000000000ll)
                                : __ddiv_rn((double)own, 32768.0);
    if (!backlink) return;
    if (!reached || own == 0) { backlink[i] = reached ? 0 : 255; return; }
    const int r = (int)(i / (unsigned)gw), c = (int)(i % (unsigned)gw);
    int fc, qc;
    cd_passable(friction, dsm, i, nodata, fc, qc);
    u64 low = CD_INF;
    int code = 255;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int rr = r + d8_dr(k), cc = c + d8_dc(k);
        if (rr < 0 || rr >= gh || cc < 0 || cc >= gw) continue;
        const size_t t = (size_t)rr * gw + cc;
        const u64 v = keys[t];
        if (v >= CD_INF) continue;
        int fn, qn;
        cd_passable(friction, dsm, t, nodata, fn, qn);
        const u64 step = cd_step(fc, fn, qc, qn, terms.L[k], terms.reverse, table);
        if (step != 0 && v + step < low) { low = v + step; code = k + 1; }
    }
    backlink[i] = (unsigned char)code;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct CostWorkspace { size_t moved, table, partial, bytes; };

static CostWorkspace cost_workspace(size_t n)
{
    CostWorkspace w;
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t here = at; at += align256(bytes); return here; };
    w.moved = take((size_t)CD_MAX_ROUNDS * 4);
    w.table = take((size_t)CD_TABLE * 4);
    w.partial = take(dsm_blocks(n, CD_THREADS) * (size_t)4);
    w.bytes = at;
    return w;
}

static const char* cost_grid_check(int gw, int gh)
{
    if (gw < 1 || gh < 1) return "non-positive grid size";
    if ((long long)gw * gh > CD_MAX_CELLS) return "grid too large: gw * gh must be at most 2^24 cells";
    return nullptr;
}

// What the entries check alike: the grid, the workspace's size, and that no two of the buffers given (null ones skipped) share
// a byte.  The workspace is the last entry of the table.
static int cost_check(int gw, int gh, const DsmBuf* buf, int n_buf, size_t workspace_bytes)
{
    if (const char* msg = cost_grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s (got %d x %d)", msg, gw, gh);
    const char* other = nullptr;
    if (const char* name = dsm_first_alias(buf, n_buf, other)) return fail(SMVS_ERR_ARG, "%s aliases %s", name, other);
    const size_t need = buf[n_buf - 1].bytes;
    if (workspace_bytes < need) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    return SMVS_OK;
}

// L, table and reverse of the rounds and the read, checked and copied.
static int cost_terms(const float* dsm, const int* L, const int* table, int reverse, CdTerms& terms, CdTable& slope)
{
    if (!L) return fail(SMVS_ERR_ARG, "null pointer argument");
    if ((dsm != nullptr) != (table != nullptr)) return fail(SMVS_ERR_ARG, "dsm and table go together: both or neither");
    if (reverse != 0 && reverse != 1) return fail(SMVS_ERR_ARG, "reverse must be 0 or 1, got %d", reverse);
    for (int k = 0; k < 8; ++k) {
        if (L[k] < 1 || L[k] > 32767) return fail(SMVS_ERR_ARG, "L[%d] must be in 1 .. 32767, got %d", k, L[k]);
        terms.L[k] = L[k];
    }
    terms.reverse = reverse;
    for (int b = 0; table && b < CD_TABLE; ++b) {
        if (table[b] < 0 || table[b] > 65535) return fail(SMVS_ERR_ARG, "table[%d] must be in 0 .. 65535, got %d", b, table[b]);
        slope.v[b] = table[b];
    }
    return SMVS_OK;
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT size_t smvs_dsm_cost_workspace_bytes(int gw, int gh)
{
    using namespace smvs;
    return cost_grid_check(gw, gh) ? 0 : cost_workspace((size_t)gw * gh).bytes;
}

SMVS_EXPORT int smvs_dsm_cost_begin(const unsigned short* friction, const unsigned char* sources, const float* dsm, int gw, int gh,
                                    float nodata, unsigned long long* keys, int* n_sources, void* workspace, size_t workspace_bytes,
                                    void* stream)
{
    using namespace smvs;
    if (!sources || !keys || !n_sources || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    const size_t n = gw > 0 && gh > 0 ? (size_t)gw * gh : 0;
    const CostWorkspace w = cost_workspace(n);
    const DsmBuf buf[] = {{friction, n * 2, "friction"}, {sources, n, "sources"}, {dsm, n * 4, "dsm"}, {keys, n * 8, "keys"},
                          {n_sources, 4, "n_sources"}, {workspace, w.bytes, "workspace"}};
    if (int rc = cost_check(gw, gh, buf, 6, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    int* partial = (int*)((char*)workspace + w.partial);
    DSM_LAUNCH(cd_begin, n, CD_THREADS, s, friction, sources, dsm, (unsigned)n, nodata, keys, partial);
    DSM_LAUNCH(cd_count, CD_THREADS, CD_THREADS, s, (const int*)partial, dsm_blocks(n, CD_THREADS), n_sources);
    return SMVS_OK;
}

SMVS_EXPORT int smvs_dsm_cost_rounds(const unsigned short* friction, const float* dsm, int gw, int gh, float nodata, const int* L,
                                     const int* table, int reverse, unsigned long long* keys, int rounds, int* status,
                                     void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!keys || !status || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (rounds < 1 || rounds > CD_MAX_ROUNDS) return fail(SMVS_ERR_ARG, "rounds must be in 1 .. %d, got %d", CD_MAX_ROUNDS, rounds);
    CdTerms terms;
    CdTable slope;
    if (int rc = cost_terms(dsm, L, table, reverse, terms, slope)) return rc;
    const size_t n = gw > 0 && gh > 0 ? (size_t)gw * gh : 0;
    const CostWorkspace w = cost_workspace(n);
    const DsmBuf buf[] = {{friction, n * 2, "friction"}, {dsm, n * 4, "dsm"}, {keys, n * 8, "keys"}, {status, 4, "status"},
                          {workspace, w.bytes, "workspace"}};
    if (int rc = cost_check(gw, gh, buf, 5, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    int* moved = (int*)((char*)workspace + w.moved);
    int* dev_table = (int*)((char*)workspace + w.table);
    if (hipMemsetAsync(moved, 0, (size_t)rounds * 4, s) != hipSuccess) return check_launch("dsm_cost_rounds (clearing the counters)");
    if (table) DSM_LAUNCH(cd_upload, CD_TABLE, CD_TABLE, s, slope, dev_table);
    const size_t tiles = (size_t)((gw + CD_TILE - 1) / CD_TILE) * (size_t)((gh + CD_TILE - 1) / CD_TILE);     // a workgroup each
    for (int k = 0; k < rounds; ++k) {
        if (table) DSM_LAUNCH((cd_round<true>), tiles * CD_THREADS, CD_THREADS, s, friction, dsm, gw, gh, nodata, terms, (const int*)dev_table, keys, moved + k);
        else DSM_LAUNCH((cd_round<false>), tiles * CD_THREADS, CD_THREADS, s, friction, dsm, gw, gh, nodata, terms, (const int*)nullptr, keys, moved + k);
    }
    DSM_LAUNCH(cd_status, 1, 64, s, (const int*)(moved + rounds - 1), status);
    return SMVS_OK;
}

SMVS_EXPORT int smvs_dsm_cost_read(const unsigned short* friction, const float* dsm, int gw, int gh, float nodata, const int* L,
                                   const int* table, int reverse, const unsigned long long* keys, unsigned long long max_cost,
                                   long long* raw, double* cost, unsigned char* backlink, void* workspace, size_t workspace_bytes,
                                   void* stream)
{
    using namespace smvs;
    if (!keys || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    CdTerms terms;
    CdTable slope;
    if (int rc = cost_terms(dsm, L, table, reverse, terms, slope)) return rc;
    const size_t n = gw > 0 && gh > 0 ? (size_t)gw * gh : 0;
    const CostWorkspace w = cost_workspace(n);
    const DsmBuf buf[] = {{friction, n * 2, "friction"}, {dsm, n * 4, "dsm"}, {keys, n * 8, "keys"}, {raw, n * 8, "raw"},
                          {cost, n * 8, "cost"}, {backlink, n, "backlink"}, {workspace, w.bytes, "workspace"}};
    if (int rc = cost_check(gw, gh, buf, 7, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    int* dev_table = (int*)((char*)workspace + w.table);
    if (table) DSM_LAUNCH(cd_upload, CD_TABLE, CD_TABLE, s, slope, dev_table);
    DSM_LAUNCH(cd_read, n, CD_THREADS, s, friction, dsm, gw, gh, nodata, terms, (const int*)(table ? dev_table : nullptr), keys,
               (u64)max_cost, raw, cost, backlink);
    return SMVS_OK;
}

}  // extern "C"
