// dsm_watershed.hip -- the seeded flood of a DSM on integer heights, exact ("Seeded flood"; include/satmvs.h
// for the rule): grey-scale geodesic reconstruction as a flood key per cell, and the flood's back-links in the library's D8
// codes, so that dsm_hydro.hip's forest (basins, accumulation, flow length) reads them as a marker watershed.
//
//   smvs_dsm_seed_begin   the keys as the relaxation starts: seeds at their level, other valid cells +infinity, invalid all ones
//   smvs_dsm_seed_rounds  `rounds` global rounds; status <- the tiles that changed in the last one
//   smvs_dsm_seed_read    keys -> surface, level_steps, backlink, n_unreached
//
// The relaxation is the flood's (dsm_hydro.hip) with other ends.  A key is ((w + 2^31) << 32) | d; a round is one workgroup per
// tile of 32 x 32 cells, which lowers every valid cell of the tile in LDS to max((g, 0), min over its valid neighbours of key + 1)
// until no cell of the tile moves (__syncthreads_or), and writes the interior back if anything moved.  What differs:
//   every valid cell is open, the seeds included: a seed starts at S = (s, 0) and another seed may undercut it.  Because a key
//     only falls, min(S, .) of the rule needs no word of its own after the begin: the rounds never see the marker;
//   invalid and off-grid neighbours are walls: they hold all ones and drop out of the minimum, and nothing is an outlet;
//   +infinity + 1 = +infinity.  A cell whose neighbours are all at +infinity (or walls) is left alone, so a component without a
//     seed stays at exactly 0xfffffffe00000000 however many rounds run; the flood's unconditional `low += 1` would creep there,
//     and on a cell walled in on all sides it would wrap all ones to 0.
// Keys start at or above the solution and a step replaces a key by max(floor, neighbour + 1) with the neighbour at or above ITS
// solution: no key passes below the solution, keys only fall, so a stale key from another tile or wave is an upper bound like
// any other, and a key moves as one aligned 64-bit access.  A round in which no tile moved found every cell at the rule's value:
// the fixed point, which is unique (every step strictly raises its argument, so a finite key hangs on a chain that ends at a
// seed).  The LDS row pitch is SPAN + 1 keys.  No kernel uses scratch; the only atomic is the per-launch counter of moved tiles;
// the two counts (seeds, unreached cells) are block counts summed in a fixed order.  Workspace: 16 KB of round counters and 4
// bytes per 256 cells.
#include <limits.h>
#include <stdint.h>

#include "dsm_common.h"
#include "dsm_flow.h"
#include "smvs_host.h"

namespace smvs {

typedef unsigned long long u64;

constexpr int SD_THREADS = D8_THREADS;
constexpr int SD_TILE = 32, SD_SPAN = SD_TILE + 2, SD_PITCH = SD_SPAN + 1;         // interior, with halo, LDS row in keys
constexpr int SD_ROWS = SD_THREADS / SD_TILE, SD_PER_THREAD = SD_TILE / SD_ROWS;  // 8 rows of lanes, 4 cells a lane
constexpr int SD_MAX_ROUNDS = 4096, SD_MAX_OFFSET = 1 << 25;
constexpr u64 SD_INVALID = ~0ull, SD_INF = 0xfffffffeull << 32;

__device__ __forceinline__ u64 sd_key(int w, unsigned d) { return (u64)((unsigned)w + 0x80000000u) << 32 | d; }
__device__ __forceinline__ int sd_w(u64 key) { return (int)((unsigned)(key >> 32) - 0x80000000u); }

// Whether cell i takes part, and g = polarity q of it.
__device__ __forceinline__ bool sd_cell(const float* __restrict__ dsm, const unsigned char* __restrict__ domain, size_t i, float nodata,
                                        int polarity, int& g)
{
    int q;
    if ((domain && !domain[i]) || !dsm_quantum(dsm[i], nodata, q)) return false;
    g = polarity * q;
    return true;
}

// Whether a valid cell with height g is a seed, and its level s = max(g, polarity q(marker) + offset).
__device__ __forceinline__ bool sd_seed(const float* __restrict__ marker, size_t i, float nodata, int polarity, int offset, int g, int& s)
{
    int qm;
    if (!dsm_quantum(marker[i], nodata, qm)) return false;
    s = max(g, polarity * qm + offset);
    return true;
}

// One workgroup: the sum of the blocks' counts, in a fixed order.
__global__ __launch_bounds__(SD_THREADS)
void sd_count(const int* __restrict__ partial, unsigned n_partial, int* __restrict__ total)
{
    __shared__ int part[SD_THREADS];
    int sum = 0;
    for (unsigned i = threadIdx.x; i < n_partial; i += SD_THREADS) sum += partial[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int half = SD_THREADS / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) part[threadIdx.x] += part[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = part[0];
}

// ---- begin ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SD_THREADS)
void sd_begin(const float* __restrict__ dsm, const float* __restrict__ marker, const unsigned char* __restrict__ domain, unsigned n,
              float nodata, int polarity, int offset, u64* __restrict__ keys, int* __restrict__ partial)
{
    const unsigned i = blockIdx.x * (unsigned)SD_THREADS + threadIdx.x;
    int seed = 0;
    if (i < n) {
        int g = 0, s = 0;
        const bool valid = sd_cell(dsm, domain, i, nodata, polarity, g);
        seed = valid && sd_seed(marker, i, nodata, polarity, offset, g, s);
        keys[i] = !valid ? SD_INVALID : seed ? sd_key(s, 0) : SD_INF;
    }
    const int count = __syncthreads_count(seed);
    if (threadIdx.x == 0) partial[blockIdx.x] = count;
}

// ---- a round -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SD_THREADS)
void sd_round(const float* __restrict__ dsm, int gw, int gh, float nodata, int polarity, u64* keys, int* __restrict__ moved)
{
    __shared__ u64 tile[SD_SPAN * SD_PITCH];
    const unsigned across = ((unsigned)gw + SD_TILE - 1) / SD_TILE;               // the tiles in a row of tiles; the grid is 1-D
    const int r0 = (int)(blockIdx.x / across) * SD_TILE - 1, c0 = (int)(blockIdx.x % across) * SD_TILE - 1;       // the halo's corner
    for (int t = threadIdx.x; t < SD_SPAN * SD_SPAN; t += SD_THREADS) {
        const int lr = t / SD_SPAN, lc = t % SD_SPAN, r = r0 + lr, c = c0 + lc;
        tile[lr * SD_PITCH + lc] = (r >= 0 && r < gh && c >= 0 && c < gw) ? keys[(size_t)r * gw + c] : SD_INVALID;
    }
    __syncthreads();
    const int lc = 1 + (int)(threadIdx.x % SD_TILE), lrow = 1 + (int)(threadIdx.x / SD_TILE);
    u64 own[SD_PER_THREAD], floor_key[SD_PER_THREAD];
    bool open[SD_PER_THREAD];                                // valid: every such cell may move, a seed too
#pragma unroll
    for (int j = 0; j < SD_PER_THREAD; ++j) {
        const int lr = lrow + j * SD_ROWS, r = r0 + lr, c = c0 + lc;
        own[j] = tile[lr * SD_PITCH + lc];                   // all ones beyond the grid, as the load above left it
        int q = 0;
        open[j] = own[j] != SD_INVALID && dsm_quantum(dsm[(size_t)r * gw + c], nodata, q);
        floor_key[j] = sd_key(polarity * q, 0);
    }
    bool any = false;
    int busy;
    do {
        busy = 0;
#pragma unroll
        for (int j = 0; j < SD_PER_THREAD; ++j) {
            if (!open[j]) continue;
            const int at = (lrow + j * SD_ROWS) * SD_PITCH + lc;
            u64 low = SD_INVALID;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const u64 v = tile[at + d8_dr(k) * SD_PITCH + d8_dc(k)];
                low = v < low ? v : low;
            }
            if (low >= SD_INF) continue;                     // walls and +infinity only: +infinity + 1 = +infinity, nothing to take
            low += 1;                                        // one step more: d < 2^30
            const u64 key = low > floor_key[j] ? low : floor_key[j];
            if (key < own[j]) {
                own[j] = key;
                tile[at] = key;
                busy = 1;
            }
        }
        any = any || busy;
        busy = __syncthreads_or(busy);
    } while (busy);
    const int tile_moved = __syncthreads_or(any);
    if (!tile_moved) return;
#pragma unroll
    for (int j = 0; j < SD_PER_THREAD; ++j)
        if (open[j]) keys[(size_t)(r0 + lrow + j * SD_ROWS) * gw + (c0 + lc)] = own[j];
    if (threadIdx.x == 0) atomicAdd(moved, 1);
}

__global__ void sd_status(const int* __restrict__ moved, int* __restrict__ status)
{
    if (threadIdx.x == 0) *status = *moved;
}

// ---- read ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SD_THREADS)
void sd_read(const float* __restrict__ dsm, const float* __restrict__ marker, const unsigned char* __restrict__ domain, int gw, int gh,
             float nodata, int polarity, int offset, const u64* __restrict__ keys, float* __restrict__ surface,
             int* __restrict__ level_steps, unsigned char* __restrict__ backlink, int* __restrict__ partial)
{
    const unsigned n = (unsigned)gw * (unsigned)gh, i = blockIdx.x * (unsigned)SD_THREADS + threadIdx.x;
    int unreached = 0;
    if (i < n) {
        const u64 own = keys[i];
        int g = 0;
        const bool valid = sd_cell(dsm, domain, i, nodata, polarity, g) && own != SD_INVALID;
        const bool reached = valid && own < SD_INF;
        unreached = valid && !reached;
        const int w = sd_w(own);
        if (surface) surface[i] = !reached ? nodata : w == g ? dsm[i] : (float)((double)(polarity * w) / 256.0);
        if (level_steps) level_steps[i] = reached ? (int)(unsigned)own : -1;
        if (backlink) {
            int code = 255, s = 0;
            if (reached && sd_seed(marker, i, nodata, polarity, offset, g, s) && own == sd_key(s, 0)) code = 0;      // the seed wins a tie
            else if (reached) {
                const int r = (int)(i / (unsigned)gw), c = (int)(i % (unsigned)gw);
                u64 low = own;
                code = 0;                                    // no lower neighbour (not a fixed point's keys): a root
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int rr = r + d8_dr(k), cc = c + d8_dc(k);
                    if (rr < 0 || rr >= gh || cc < 0 || cc >= gw) continue;
                    const u64 v = keys[(size_t)rr * gw + cc];
                    if (v < low) { low = v; code = k + 1; }
                }
            }
            backlink[i] = (unsigned char)code;
        }
    }
    const int count = __syncthreads_count(unreached);
    if (partial && threadIdx.x == 0) partial[blockIdx.x] = count;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct SeedWorkspace { size_t moved, partial, bytes; };

static SeedWorkspace seed_workspace(size_t n)
{
    SeedWorkspace w;
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t here = at; at += align256(bytes); return here; };
    w.moved = take((size_t)SD_MAX_ROUNDS * 4);
    w.partial = take(dsm_blocks(n, SD_THREADS) * (size_t)4);
    w.bytes = at;
    return w;
}

// What the entries check alike: the polarity, the grid, the workspace's size, and that no buffer written (the entries of the
// table from `first_out` on; the workspace is the last) shares a byte with any other.  The inputs may share theirs: h-maxima
// give the DSM as its own marker.
static int seed_check(int gw, int gh, int polarity, const DsmBuf* buf, int n_buf, int first_out, size_t workspace_bytes)
{
    if (polarity != 1 && polarity != -1) return fail(SMVS_ERR_ARG, "polarity must be +1 or -1, got %d", polarity);
    if (const char* msg = d8_grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s (got %d x %d)", msg, gw, gh);
    for (int i = first_out; i < n_buf; ++i)
        for (int j = 0; j < i; ++j)
            if (buf[i].p && buf[j].p && dsm_overlap(buf[i].p, buf[i].bytes, buf[j].p, buf[j].bytes))
                return fail(SMVS_ERR_ARG, "%s aliases %s", buf[i].name, buf[j].name);
    const size_t need = buf[n_buf - 1].bytes;
    if (workspace_bytes < need) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    return SMVS_OK;
}

static int seed_offset_check(int offset)
{
    if (offset > SD_MAX_OFFSET || offset < -SD_MAX_OFFSET) return fail(SMVS_ERR_ARG, "offset must be within +-2^25 quanta, got %d", offset);
    return SMVS_OK;
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT size_t smvs_dsm_seed_workspace_bytes(int gw, int gh)
{
    using namespace smvs;
    return d8_grid_check(gw, gh) ? 0 : seed_workspace((size_t)gw * gh).bytes;
}

SMVS_EXPORT int smvs_dsm_seed_begin(const float* dsm, const float* marker, const unsigned char* domain, int gw, int gh, float nodata,
                                    int polarity, int offset, unsigned long long* keys, int* n_seeds, void* workspace,
                                    size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!dsm || !marker || !keys || !n_seeds || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (int rc = seed_offset_check(offset)) return rc;
    const size_t n = gw > 0 && gh > 0 ? (size_t)gw * gh : 0;
    const SeedWorkspace w = seed_workspace(n);
    const DsmBuf buf[] = {{dsm, n * 4, "dsm"}, {marker, n * 4, "marker"}, {domain, n, "domain"}, {keys, n * 8, "keys"},
                          {n_seeds, 4, "n_seeds"}, {workspace, w.bytes, "workspace"}};
    if (int rc = seed_check(gw, gh, polarity, buf, 6, 3, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    int* partial = (int*)((char*)workspace + w.partial);
    DSM_LAUNCH(sd_begin, n, SD_THREADS, s, dsm, marker, domain, (unsigned)n, nodata, polarity, offset, keys, partial);
    DSM_LAUNCH(sd_count, SD_THREADS, SD_THREADS, s, (const int*)partial, dsm_blocks(n, SD_THREADS), n_seeds);
    return SMVS_OK;
}

SMVS_EXPORT int smvs_dsm_seed_rounds(const float* dsm, int gw, int gh, float nodata, int polarity, unsigned long long* keys, int rounds,
                                     int* status, void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!dsm || !keys || !status || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (rounds < 1 || rounds > SD_MAX_ROUNDS) return fail(SMVS_ERR_ARG, "rounds must be in 1 .. %d, got %d", SD_MAX_ROUNDS, rounds);
    const size_t n = gw > 0 && gh > 0 ? (size_t)gw * gh : 0;
    const SeedWorkspace w = seed_workspace(n);
    const DsmBuf buf[] = {{dsm, n * 4, "dsm"}, {keys, n * 8, "keys"}, {status, 4, "status"}, {workspace, w.bytes, "workspace"}};
    if (int rc = seed_check(gw, gh, polarity, buf, 4, 1, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    int* moved = (int*)((char*)workspace + w.moved);
    if (hipMemsetAsync(moved, 0, (size_t)rounds * 4, s) != hipSuccess) return check_launch("dsm_seed_rounds (clearing the counters)");
    const size_t tiles = (size_t)((gw + SD_TILE - 1) / SD_TILE) * (size_t)((gh + SD_TILE - 1) / SD_TILE);     // a workgroup each
    for (int k = 0; k < rounds; ++k) DSM_LAUNCH(sd_round, tiles * SD_THREADS, SD_THREADS, s, dsm, gw, gh, nodata, polarity, keys, moved + k);
    DSM_LAUNCH(sd_status, 1, 64, s, (const int*)(moved + rounds - 1), status);
    return SMVS_OK;
}

SMVS_EXPORT int smvs_dsm_seed_read(const float* dsm, const float* marker, const unsigned char* domain, int gw, int gh, float nodata,
                                   int polarity, int offset, const unsigned long long* keys, float* surface, int* level_steps,
                                   unsigned char* backlink, int* n_unreached, void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!dsm || !marker || !keys || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (int rc = seed_offset_check(offset)) return rc;
    const size_t n = gw > 0 && gh > 0 ? (size_t)gw * gh : 0;
    const SeedWorkspace w = seed_workspace(n);
    const DsmBuf buf[] = {{dsm, n * 4, "dsm"}, {marker, n * 4, "marker"}, {domain, n, "domain"}, {keys, n * 8, "keys"},
                          {surface, n * 4, "surface"}, {level_steps, n * 4, "level_steps"}, {backlink, n, "backlink"},
                          {n_unreached, 4, "n_unreached"}, {workspace, w.bytes, "workspace"}};
    if (int rc = seed_check(gw, gh, polarity, buf, 9, 4, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    int* partial = n_unreached ? (int*)((char*)workspace + w.partial) : nullptr;
    DSM_LAUNCH(sd_read, n, SD_THREADS, s, dsm, marker, domain, gw, gh, nodata, polarity, offset, keys, surface, level_steps, backlink, partial);
    if (n_unreached) DSM_LAUNCH(sd_count, SD_THREADS, SD_THREADS, s, (const int*)partial, dsm_blocks(n, SD_THREADS), n_unreached);
    return SMVS_OK;
}

}  // extern "C"
