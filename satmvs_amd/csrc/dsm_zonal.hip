// dsm_zonal.hip -- exact order statistics of the labels of a zone map ("Zonal order statistics";
// include/satmvs.h for the rule).
//
//   smvs_dsm_label_select  for every label and each of up to 8 ranks, the value of that rank among the label's valid cells
//
// A radix descent over the 32 bits of the order-preserving keys, the highest first, all (label, rank) slots side by side.  A
// slot keeps in the workspace the bits of its answer fixed so far (`prefix`, the lower bits 0) and the rank that remains among
// the keys that share them (`rem`).  A round is two launches: dsm_zonal_count walks the cells once and counts, per slot, the
// valid cells of the slot's label whose key continues the prefix with a 0 at the round's bit; dsm_zonal_fix, one lane per
// slot, stays on the 0 side if rem < count and else sets the bit and lowers rem by the count.  After bit 0 the prefix is the
// key of the answer.  The first count also counts the valid cells per label, which dsm_zonal_finish holds the ranks against.
// 2 + 64 launches whatever n, the grid and the data; integer atomics without a return value only, so the bits do not depend on
// their order; no read of the device.
//
// The count is a flat walk over gw * gh cells, a workgroup 4096 consecutive ones, a lane four consecutive cells per step (16-byte
// loads where both grids are 16-byte aligned), the next step's loads in flight under the current one's counting.  The four
// cells of a lane are taken one after the other; for each, the wave's 64 lanes either carry one label -- the inside of a zone:
// the slots' prefixes sit in scalar registers, a slot's count of the step is one ballot, and the wave sums in registers for
// as long as the label stays -- or several: then lanes side by side with one label are a run (the idiom of dsm_label.hip), a
// slot's count of a run is the ballot under the run's mask, and the run's first lane sends it; a step with such a cell
// fetches the prefixes of all its four cells at once.  What the waves of a workgroup
// still hold at the end is combined by label in LDS, so a zone that covers the grid costs one atomic per slot and workgroup.
#include <stdint.h>

#include "dsm_common.h"
#include "smvs_host.h"

namespace smvs {

constexpr int ZONAL_THREADS = 256, ZONAL_WAVES = ZONAL_THREADS / 64, ZONAL_STEPS = 4;
constexpr int ZONAL_CELLS = ZONAL_THREADS * 4 * ZONAL_STEPS;              // cells of one workgroup
constexpr int ZONAL_MAX_RANKS = 8;
constexpr long long ZONAL_MAX_SLOTS = 1ll << 28;                          // n * n_ranks stays below it

struct ZonalArgs {
    const int* labels;
    const float* values;
    const float* centre;                                     // null: the values themselves
    const unsigned* prefix;
    unsigned* cnt;
    int* nv;
    unsigned ncells;
    float nodata;
    int n, nr, bit;
};

// What a wave holds of one label while its steps stay inside it; every member is wave-uniform.  acc[8]: the valid cells.
struct ZonalWave {
    int held;
    float ctr;
    unsigned pre[ZONAL_MAX_RANKS];
    unsigned acc[ZONAL_MAX_RANKS + 1];
};

// The key a cell is selected by, false if the cell does not count.  With a centre: d = (float)fabs((double)v - (double)ctr).
__device__ __forceinline__ bool zonal_key(float v, float nodata, bool deviation, float ctr, unsigned& key)
{
    if (!dsm_cell_valid(v, nodata)) return false;
    if (deviation) {
        if (!isfinite(ctr)) return false;
        v = __double2float_rn(fabs(__dsub_rn((double)v, (double)ctr)));
    }
    key = f2key(v);
    return true;
}

template <bool FIRST>
__device__ __forceinline__ void zonal_flush(ZonalWave& w, const ZonalArgs& a)
{
    if (w.held != 0 && (threadIdx.x & 63) == 0) {
        unsigned* c = a.cnt + (size_t)(w.held - 1) * a.nr;
#pragma unroll
        for (int j = 0; j < ZONAL_MAX_RANKS; ++j)
            if (j < a.nr && w.acc[j]) atomicAdd(c + j, w.acc[j]);
        if (FIRST && w.acc[ZONAL_MAX_RANKS]) atomicAdd(a.nv + (w.held - 1), (int)w.acc[ZONAL_MAX_RANKS]);
    }
#pragma unroll
    for (int j = 0; j <= ZONAL_MAX_RANKS; ++j) w.acc[j] = 0;
}

struct ZonalCells { int lab[4]; float v[4]; };               // a lane's four consecutive cells; lab 0: no label of 1 .. n, or past the grid

// One cell per lane, every lane the label `lab` (wave-uniform).
template <bool FIRST>
__device__ __forceinline__ void zonal_uniform(ZonalWave& w, int lab, float v, const ZonalArgs& a)
{
    const bool deviation = a.centre != nullptr;
    if (lab != w.held) {
        zonal_flush<FIRST>(w, a);
        w.held = lab;
        if (lab != 0) {
            w.ctr = deviation ? a.centre[lab - 1] : 0.0f;
            const unsigned* p = a.prefix + (size_t)(lab - 1) * a.nr;
#pragma unroll
            for (int j = 0; j < ZONAL_MAX_RANKS; ++j) w.pre[j] = j < a.nr ? p[j] : 0u;
        }
    }
    if (lab == 0) return;
    unsigned key = 0;
    const bool valid = zonal_key(v, a.nodata, deviation, w.ctr, key);
#pragma unroll
    for (int j = 0; j < ZONAL_MAX_RANKS; ++j)
        if (j < a.nr) w.acc[j] += (unsigned)__popcll(__ballot(valid && ((key ^ w.pre[j]) >> a.bit) == 0u));
    if (FIRST) w.acc[ZONAL_MAX_RANKS] += (unsigned)__popcll(__ballot(valid));
}

// Four cells per lane, labels of any kind, regrouped so that a run of cells with one label is a run of lanes.  The prefixes of all four cells are fetched before the first is used (a lane
// without a label reads slot 0 and counts nothing), so the wave waits for memory once per step, not once per cell.
template <bool FIRST>
__device__ __forceinline__ void zonal_mixed(const ZonalCells& own, const ZonalArgs& a)
{
    const int lane = threadIdx.x & 63;
    const bool deviation = a.centre != nullptr;
    // lanes side by side take cells side by side: cell 64 k + lane of the wave's 256 is cell (lane & 3) of lane 16 k + lane / 4
    ZonalCells z;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int src = 16 * k + (lane >> 2), sel = lane & 3;
        const int l0 = __shfl(own.lab[0], src), l1 = __shfl(own.lab[1], src), l2 = __shfl(own.lab[2], src), l3 = __shfl(own.lab[3], src);
        const float v0 = __shfl(own.v[0], src), v1 = __shfl(own.v[1], src), v2 = __shfl(own.v[2], src), v3 = __shfl(own.v[3], src);
        z.lab[k] = sel == 0 ? l0 : sel == 1 ? l1 : sel == 2 ? l2 : l3;
        z.v[k] = sel == 0 ? v0 : sel == 1 ? v1 : sel == 2 ? v2 : v3;
    }
    size_t slot[4];
    float ctr[4];
    unsigned pre[4][ZONAL_MAX_RANKS];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        slot[k] = z.lab[k] != 0 ? (size_t)(z.lab[k] - 1) * a.nr : 0;
        ctr[k] = deviation ? a.centre[z.lab[k] != 0 ? z.lab[k] - 1 : 0] : 0.0f;
#pragma unroll
        for (int j = 0; j < ZONAL_MAX_RANKS; ++j) pre[k][j] = j < a.nr ? a.prefix[slot[k] + j] : 0u;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int lab = z.lab[k];
        const int prev = __shfl_up(lab, 1);
        const bool head = lane == 0 || prev != lab;
        const unsigned long long heads = __ballot(head);
        const unsigned long long above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);   // the heads after this lane
        const unsigned long long upto = above ? (1ull << __builtin_ctzll(above)) - 1ull : ~0ull; // lanes before the next head
        const unsigned long long run = upto & ~((1ull << lane) - 1ull);                          // of a head: its run
        const bool sends = head && lab != 0;
        unsigned key = 0;
        const bool valid = lab != 0 && zonal_key(z.v[k], a.nodata, deviation, ctr[k], key);
#pragma unroll
        for (int j = 0; j < ZONAL_MAX_RANKS; ++j) {
            if (j < a.nr) {
                const unsigned long long hit = __ballot(valid && ((key ^ pre[k][j]) >> a.bit) == 0u);
                const unsigned c = (unsigned)__popcll(hit & run);
                if (sends && c) atomicAdd(a.cnt + slot[k] + j, c);
            }
        }
        if (FIRST) {
            const int c = __popcll(__ballot(valid) & run);
            if (sends && c) atomicAdd(a.nv + (lab - 1), c);
        }
    }
}

// One step of a wave: 256 cells, four per lane, taken as four rounds of one cell per lane.
template <bool FIRST>
__device__ __forceinline__ void zonal_step(ZonalWave& w, const ZonalCells& z, const ZonalArgs& a)
{
    int first[4];
    bool same = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        first[k] = __builtin_amdgcn_readfirstlane(z.lab[k]);
        same = same && z.lab[k] == first[k];
    }
    if (__all(same)) {
#pragma unroll
        for (int k = 0; k < 4; ++k) zonal_uniform<FIRST>(w, first[k], z.v[k], a);
        return;
    }
    zonal_flush<FIRST>(w, a);
    w.held = 0;
    zonal_mixed<FIRST>(z, a);
}

template <bool VEC>
__device__ __forceinline__ ZonalCells zonal_load(const ZonalArgs& a, size_t c0)
{
    ZonalCells z;
    if (VEC && c0 + 4 <= a.ncells) {
        const int4 l = *(const int4*)(a.labels + c0);
        const float4 f = *(const float4*)(a.values + c0);
        z.lab[0] = l.x; z.lab[1] = l.y; z.lab[2] = l.z; z.lab[3] = l.w;
        z.v[0] = f.x; z.v[1] = f.y; z.v[2] = f.z; z.v[3] = f.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = c0 + k < a.ncells;
            z.lab[k] = in ? a.labels[c0 + k] : 0;
            z.v[k] = in ? a.values[c0 + k] : 0.0f;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if ((unsigned)z.lab[k] - 1u >= (unsigned)a.n) z.lab[k] = 0;      // 0, negative, above n: nothing
    return z;
}

// VEC: labels and values are 16-byte aligned.  FIRST: the round of bit 31, which also counts the valid cells per label.
template <bool VEC, bool FIRST>
__global__ __launch_bounds__(ZONAL_THREADS)
void dsm_zonal_count(ZonalArgs a)
{
    __shared__ int s_held[ZONAL_WAVES];
    __shared__ unsigned s_acc[ZONAL_WAVES][ZONAL_MAX_RANKS + 1];
    const size_t wg0 = (size_t)blockIdx.x * ZONAL_CELLS;
    ZonalWave w;
    w.held = 0;
    w.ctr = 0.0f;
#pragma unroll
    for (int j = 0; j < ZONAL_MAX_RANKS; ++j) w.pre[j] = 0u;
#pragma unroll
    for (int j = 0; j <= ZONAL_MAX_RANKS; ++j) w.acc[j] = 0u;
    ZonalCells cur = zonal_load<VEC>(a, wg0 + (size_t)threadIdx.x * 4);
#pragma unroll 1
    for (int it = 0; it < ZONAL_STEPS; ++it) {
        ZonalCells nxt = cur;
        if (it + 1 < ZONAL_STEPS) nxt = zonal_load<VEC>(a, wg0 + ((size_t)(it + 1) * ZONAL_THREADS + threadIdx.x) * 4);
        zonal_step<FIRST>(w, cur, a);
        cur = nxt;
    }
    // what the waves still hold, combined by label: the first wave of a label sends the sum of all that hold it
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_held[wave] = w.held;
#pragma unroll
        for (int j = 0; j <= ZONAL_MAX_RANKS; ++j) s_acc[wave][j] = w.acc[j];
    }
    __syncthreads();
    if (threadIdx.x >= ZONAL_WAVES * (ZONAL_MAX_RANKS + 1)) return;
    const int wv = threadIdx.x / (ZONAL_MAX_RANKS + 1), j = threadIdx.x % (ZONAL_MAX_RANKS + 1);
    const int lab = s_held[wv];
    if (lab == 0 || !(j < a.nr || (FIRST && j == ZONAL_MAX_RANKS))) return;
    unsigned sum = 0;
    for (int o = 0; o < ZONAL_WAVES; ++o) {
        if (s_held[o] != lab) continue;
        if (o < wv) return;                                  // an earlier wave sends this label
        sum += s_acc[o][j];
    }
    if (sum == 0) return;
    if (j < ZONAL_MAX_RANKS) atomicAdd(a.cnt + (size_t)(lab - 1) * a.nr + j, sum);
    else atomicAdd(a.nv + (lab - 1), (int)sum);
}

__global__ __launch_bounds__(ZONAL_THREADS)
void dsm_zonal_init(int n, int nr, const int* __restrict__ ranks, unsigned* __restrict__ prefix, int* __restrict__ rem,
                    unsigned* __restrict__ cnt, int* __restrict__ nv)
{
    const unsigned s = blockIdx.x * (unsigned)ZONAL_THREADS + threadIdx.x;
    if (s >= (unsigned)n * (unsigned)nr) return;
    prefix[s] = 0u;
    rem[s] = ranks[s];
    cnt[s] = 0u;
    if (s < (unsigned)n) nv[s] = 0;
}

// A rank below 0 never leaves the 0 side and one at or above the number of valid cells never leaves the 1 side: rem never
// wraps, and dsm_zonal_finish gives such a slot nodata.
__global__ __launch_bounds__(ZONAL_THREADS)
void dsm_zonal_fix(unsigned slots, int bit, unsigned* __restrict__ prefix, int* __restrict__ rem, unsigned* __restrict__ cnt)
{
    const unsigned s = blockIdx.x * (unsigned)ZONAL_THREADS + threadIdx.x;
    if (s >= slots) return;
    const unsigned c = cnt[s];                               // below 2^31: a count of cells
    cnt[s] = 0u;
    const int r = rem[s];
    if (r >= (int)c) {
        prefix[s] |= 1u << bit;
        rem[s] = r - (int)c;
    }
}

__global__ __launch_bounds__(ZONAL_THREADS)
void dsm_zonal_finish(int n, int nr, float nodata, const int* __restrict__ ranks, const unsigned* __restrict__ prefix,
                      const int* __restrict__ nv, float* __restrict__ out, int* __restrict__ nvalid)
{
    const unsigned s = blockIdx.x * (unsigned)ZONAL_THREADS + threadIdx.x;
    if (s >= (unsigned)n * (unsigned)nr) return;
    const int m = nv[s / (unsigned)nr], r = ranks[s];
    out[s] = (r >= 0 && r < m) ? key2f(prefix[s]) : nodata;
    if (nvalid && s < (unsigned)n) nvalid[s] = nv[s];
}

struct ZonalWorkspace { size_t prefix, rem, cnt, nv, bytes; };

static ZonalWorkspace zonal_workspace(size_t n, size_t nr)
{
    ZonalWorkspace w;
    w.prefix = 0;
    w.rem = w.prefix + align256(n * nr * 4);
    w.cnt = w.rem + align256(n * nr * 4);
    w.nv = w.cnt + align256(n * nr * 4);
    w.bytes = w.nv + align256(n * 4) + 256;                  // never 0 for supported arguments, n == 0 included
    return w;
}

static const char* zonal_check(int n, int n_ranks)
{
    if (n < 0) return "n must be >= 0";
    if (n_ranks < 1 || n_ranks > ZONAL_MAX_RANKS) return "n_ranks must be in 1 .. 8";
    if ((long long)n * n_ranks >= ZONAL_MAX_SLOTS) return "n * n_ranks must be below 2^28";
    return nullptr;
}

template <bool VEC>
static int zonal_rounds(const ZonalArgs& a0, int* rem, hipStream_t s)
{
    ZonalArgs a = a0;
    const unsigned slots = (unsigned)a.n * (unsigned)a.nr;
    const dim3 blocks(dsm_blocks(a.ncells, ZONAL_CELLS)), threads(ZONAL_THREADS);
    for (int bit = 31; bit >= 0; --bit) {
        a.bit = bit;
        if (bit == 31) hipLaunchKernelGGL((dsm_zonal_count<VEC, true>), blocks, threads, 0, s, a);
        else hipLaunchKernelGGL((dsm_zonal_count<VEC, false>), blocks, threads, 0, s, a);
        if (int rc = check_launch("dsm_zonal_count")) return rc;
        DSM_LAUNCH(dsm_zonal_fix, slots, ZONAL_THREADS, s, slots, bit, (unsigned*)a.prefix, rem, a.cnt);
    }
    return SMVS_OK;
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT size_t smvs_dsm_label_select_workspace_bytes(int n, int n_ranks)
{
    using namespace smvs;
    if (zonal_check(n, n_ranks)) return 0;
    return zonal_workspace((size_t)n, (size_t)n_ranks).bytes;
}

SMVS_EXPORT int smvs_dsm_label_select(const int* labels, const float* values, int gw, int gh, float nodata, int n,
                                      const float* centre, const int* ranks, int n_ranks,
                                      float* out, int* nvalid, void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!labels || !values || !ranks || !out || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (const char* msg = zonal_check(n, n_ranks)) return fail(SMVS_ERR_ARG, "%s, got n = %d, n_ranks = %d", msg, n, n_ranks);
    const size_t ncells = (size_t)gw * gh, m = (size_t)n, slots = m * (size_t)n_ranks;
    const ZonalWorkspace w = zonal_workspace(m, (size_t)n_ranks);
    if (workspace_bytes < w.bytes) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, w.bytes);
    const DsmBuf buf[] = {{labels, ncells * 4, "labels"}, {values, ncells * 4, "values"}, {centre, m * 4, "centre"}, {ranks, slots * 4, "ranks"},
                          {out, slots * 4, "out"}, {nvalid, m * 4, "nvalid"}, {workspace, w.bytes, "workspace"}};
    for (int i = 4; i < 7; ++i)                              // the outputs and the workspace against everything before them
        for (int j = 0; j < i; ++j)
            if (buf[i].p && buf[j].p && buf[i].bytes && buf[j].bytes && dsm_overlap(buf[i].p, buf[i].bytes, buf[j].p, buf[j].bytes))
                return fail(SMVS_ERR_ARG, "%s aliases %s", buf[i].name, buf[j].name);
    if (n == 0) return SMVS_OK;
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)workspace;
    unsigned *prefix = (unsigned*)(base + w.prefix), *cnt = (unsigned*)(base + w.cnt);
    int *rem = (int*)(base + w.rem), *nv = (int*)(base + w.nv);
    DSM_LAUNCH(dsm_zonal_init, slots, ZONAL_THREADS, s, n, n_ranks, ranks, prefix, rem, cnt, nv);
    const ZonalArgs a = {labels, values, centre, prefix, cnt, nv, (unsigned)ncells, nodata, n, n_ranks, 31};
    const bool vec = (((uintptr_t)labels | (uintptr_t)values) & 15) == 0;
    if (int rc = vec ? zonal_rounds<true>(a, rem, s) : zonal_rounds<false>(a, rem, s)) return rc;
    DSM_LAUNCH(dsm_zonal_finish, slots, ZONAL_THREADS, s, n, n_ranks, nodata, ranks, prefix, nv, out, nvalid);
    return SMVS_OK;
}

}  // extern "C"
