// mfma_conv.h -- float32 MFMA implicit-GEMM convolution shared by the regularisers (red.hip 2-D, costreg.hip 3-D).
//
// For the levels whose channel counts reach the matrix-core tile (Cout >= 32) the convolution is the GEMM
//   D[cout][pos] = sum_kk W[cout][kk] * X[kk][pos],   kk = (input channel, tap),
// on v_mfma_f32_32x32x2_f32 (exact float32: the result is a k-ordered fmaf chain, so numerics stay in the
// same class as the direct kernels).  Rows (M) are 32 output channels, columns (N) 32 consecutive output
// positions along x -- so every accumulator register of a lane belongs to ONE output position and the store
// of a register across lanes is a coalesced 128-B row -- and K advances two (channel, tap) pairs per MFMA.
//   * 27 taps (3-D): X operand: one buffer load per lane and MFMA (lane -> position l&31, k-slot l>>5); the per-lane
//     tap offsets (zero padding = out-of-range offset) are fixed per tile, the channel pair rides in the scalar
//     offset: no vector ALU work in the K loop.  W operand: one coalesced load per lane and MFMA from a buffer
//     pre-packed in exactly the order the lanes consume it ([channel pair][step][cout tile][k-slot][32]).
//   * 9 taps (2-D): a CU's texture path, not the matrix pipe, bounded that scheme on the small grids (18 dword loads
//     per 9 MFMAs and wave: measured ~1700 clocks per batch against 576 of MFMA issue).  So k-slot = CHANNEL of the
//     pair and step = tap: a lane's nine X values are three rows of three consecutive floats = 3 dwordx3 loads (edge
//     columns fixed up with selects), its nine weights are contiguous = 3 dwordx4 loads
//     ([channel pair][cout tile][k-slot][32][12]): 6 loads per batch instead of 18.
//   * The coarse levels are tiny (a few thousand positions), so a workgroup's 4 waves split K (input
//     channels) four ways and reduce through LDS: 4x the waves in flight for the same tile.
// Epilogue (wave 0): bias / BatchNorm scale-shift, ReLU, skip add, GroupNorm statistics.
#pragma once
#include <type_traits>

#include "smvs_device.h"
#include "../../include/satmvs.h"

namespace smvs {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float mf32x3 __attribute__((ext_vector_type(3)));
typedef float mf32x4 __attribute__((ext_vector_type(4)));
__device__ mf32x3 llvm_raw_buffer_load_v3f32(i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v3f32");
__device__ mf32x4 llvm_raw_buffer_load_v4f32(i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v4f32");
constexpr int MFMA9_WSLOT = 12;              // 9-tap weights: a lane's 9 taps padded to three float4
constexpr int MFMA_PREFETCH = 2;             // 9-tap kernels, one cout tile per workgroup: channel pairs in flight per wave

struct MfmaConvArgs {
    const float* inA; int CA;                // first CA input channels (must be even)
    const float* inB; int CB;                // next CB channels (concat input), or null/0
    const float* w;                          // packed [ (CA+CB)/2 ][ TAPS ][ NT ][ 2 ][ 32 ]
    const float* bias;                       // (Cout) or null
    const float* scale; const float* shift;  // (Cout) BatchNorm inference affine, or null
    const float* skip;                       // same shape as out, added after ReLU, or null
    float* out;
    double* stats; int ngroups; int nslot;   // GroupNorm partial sums (see red.hip), or null
    int Cout, relu, stride;
    int Di, Hi, Wi, Do, Ho, Wo;              // 2-D: Di = Do = 1
    float scaleA;                            // multiplies the A-tensor inputs (-1 feeds -cost)
    int ntiles;                              // tiles of 32 positions in the launch (KS < NW variants: decode / bound of the flat unit index)
    const float* init;                       // same shape as out, or null: added to the sums before statistics / activation
};

// W pack kernel: src (Cout, Cin, TAPS) [conv] -> dst [cip][p][nt][h][32]
// step p of channel pair cip covers kk = 2p + h in the 2*TAPS-long (ci0 taps..., ci1 taps...) list.
// adjoint = 1: src is an nn.Conv2d / nn.Conv3d weight (cin, cout, 3, 3[, 3]) -- of the layer whose ADJOINT (gradient with respect to its input:
// the correlation of the output gradient with the transposed, tap-flipped weights) is packed: W'[co][ci][t] = src[ci][co][8 - t].
static __global__ void mfma_pack_kernel(const float* __restrict__ src, float* __restrict__ dst, int cin, int cout, int taps, int adjoint)
{
    const int nt = (cout + 31) / 32;
    if (taps == 9) {                             // [cip][nt][h][32][12]: step p = tap p, k-slot h = channel 2*cip + h
        const int n9 = (cin / 2) * nt * 64 * MFMA9_WSLOT;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n9; i += gridDim.x * blockDim.x) {
            const int t = i % MFMA9_WSLOT, j = (i / MFMA9_WSLOT) & 31, h = (i / (MFMA9_WSLOT * 32)) & 1;
            const int tl = (i / (MFMA9_WSLOT * 64)) % nt, cip = i / (MFMA9_WSLOT * 64 * nt);
            const int co = tl * 32 + j, ci = 2 * cip + h;
            dst[i] = (t < 9 && co < cout) ? (adjoint ? src[((size_t)ci * cout + co) * 9 + (8 - t)] : src[((size_t)co * cin + ci) * 9 + t]) : 0.0f;
        }
        return;
    }
    const int n = (cin / 2) * taps * nt * 64;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int j = i & 31, h = (i >> 5) & 1, t = (i >> 6) % nt, p = (i / (64 * nt)) % taps, cip = i / (64 * nt * taps);
        const int kk = 2 * p + h;
        const int ci = 2 * cip + (kk >= taps ? 1 : 0), tap = kk >= taps ? kk - taps : kk;
        const int co = t * 32 + j;
        dst[i] = co < cout ? (adjoint ? src[((size_t)ci * cout + co) * taps + (taps - 1 - tap)] : src[((size_t)co * cin + ci) * taps + tap]) : 0.0f;
    }
}

// NT = cout tiles per workgroup (blockIdx.y walks the rest), NW = waves per workgroup, KS = waves that split the K range of
// one (tile, cout tile) unit and reduce through LDS.
// KS = NW (default; latency regime: a few hundred tiles on 256 CUs): one unit per workgroup, (bx, by) = (tile, cout tile block).
// KS < NW (throughput regime, round 3): NW/KS units per workgroup, unit = bx * NW/KS + wave / KS of a flat
//   (cout tile block, tile) index.  With K split four ways a 32-channel layer of the full-resolution stage is 36 MFMAs per
//   wave -- all prologue -- and three of four waves idle through the epilogue (MFMA pipe 20 % busy,
//   profiles/r03_mfma_utilisation.txt); KS = 1 / 2 gives 144-288 MFMAs per wave at 4-5 resident waves per SIMD.
// smem: (NW - NW/KS)*NT*16*64 floats.
template <int TAPS, int NT, int NW, int KS = NW>
__device__ __forceinline__ void mfma_conv_body(const MfmaConvArgs& a, int bx, int by, float* smem)
{
    static_assert(NW % KS == 0, "waves per unit");
    constexpr int TW = NW / KS;                            // units per workgroup
    constexpr int KD = TAPS == 27 ? 3 : 1;
    float (*red)[NT * 16][64] = (float (*)[NT * 16][64])smem;   // partial accumulators of waves 1..NW-1
    const int nt_all = (a.Cout + 31) / 32;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kw = KS == NW ? wave : wave % KS, tw = KS == NW ? 0 : wave / KS;   // K share, unit inside the workgroup
    const int unit = bx * TW + tw;
    const bool unit_ok = KS == NW || unit < a.ntiles * (nt_all / NT);          // the last workgroup may hold fewer units
    const int nt0 = (KS == NW ? by : unit / a.ntiles) * NT;
    const int j = lane & 31, h = lane >> 5;
    // tile -> (b, od, oy, x0)
    const int xt = (a.Wo + 31) / 32;
    int t = KS == NW ? bx : unit % a.ntiles;
    const int x0 = (t % xt) * 32; t /= xt;
    const int oy = t % a.Ho; t /= a.Ho;
    const int od = t % a.Do;
    const int b = t / a.Do;
    const int ox = x0 + j;
    const bool pos_ok = unit_ok && ox < a.Wo;
    const int HWi = a.Hi * a.Wi;
    const size_t vol_i = (size_t)a.Di * HWi;
    const int Cin = a.CA + a.CB;

    // per-lane offsets in consumption order: step p -> kk = 2p + h -> (channel of the pair, tap)
    uint32_t off[TAPS];
#pragma unroll
    for (int p = 0; p < TAPS; ++p) {
        const int kkA = 2 * p, kkB = 2 * p + 1;            // compile-time for each half
        const int tapA = kkA >= TAPS ? kkA - TAPS : kkA, chA = kkA >= TAPS ? 1 : 0;
        const int tapB = kkB >= TAPS ? kkB - TAPS : kkB, chB = kkB >= TAPS ? 1 : 0;
        const int tap = h ? tapB : tapA, ch = h ? chB : chA;
        const int kd = tap / 9 % 3, ky = (TAPS == 27 ? tap % 9 : tap) / 3, kx = tap % 3;
        const int id = od * a.stride - (KD == 3 ? 1 : 0) + (KD == 3 ? kd : 0);
        const int iy = oy * a.stride - 1 + ky, ix = ox * a.stride - 1 + kx;
        const bool in = pos_ok && id >= 0 && id < a.Di && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi;
        off[p] = in ? (uint32_t)(((size_t)ch * vol_i + (size_t)(id * a.Hi + iy) * a.Wi + ix) * 4) : SMVS_OOB;
    }
    const BufRsrc rA = make_rsrc(a.inA + (size_t)b * a.CA * vol_i, (uint32_t)((size_t)a.CA * vol_i * 4));
    const BufRsrc rB = make_rsrc(a.CB ? a.inB + (size_t)b * a.CB * vol_i : a.inA, (uint32_t)((size_t)a.CB * vol_i * 4));
    const BufRsrc rW = make_rsrc(a.w, (uint32_t)((size_t)(Cin / 2) * (TAPS == 9 ? MFMA9_WSLOT : TAPS) * nt_all * 64 * 4));

    f32x16 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.0f;

    // K loop, split over the 4 waves by input-channel pairs.  A wave walks its channel pairs in batches
    // of BS steps (BS X loads + NT*BS W loads), double-buffered: the loads of batch q+1 are in flight
    // while the BS*NT MFMAs of batch q issue.  These levels have only a few hundred tiles, so there is
    // no occupancy to hide latency with -- the prefetch is what keeps the matrix pipe fed.
    constexpr int BS = (TAPS == 27) ? 9 : 9;               // steps per batch (TAPS is a multiple of 9)
    constexpr int NB = TAPS / BS;                          // batches per channel pair
    const int ncip = Cin / 2, per = ncip / KS;
    const int q_end = per * NB;
    struct Batch { float x[BS]; float w[NT][BS]; float sx; };
    // explicit variants so that every off[] / register index is a compile-time constant
#define SMVS_LOAD_BATCH(G, BT, Q)                                                                        \
    {                                                                                                    \
        const int cip_ = kw * per + (Q) / NB;                                                            \
        const bool fromA_ = 2 * cip_ < a.CA;                      /* wave-uniform: scalar selects */    \
        const int choff_ = (int)((size_t)(fromA_ ? 2 * cip_ : 2 * cip_ - a.CA) * vol_i * 4);            \
        i32x4 rx_;                                                                                       \
        rx_.x = fromA_ ? rA.v.x : rB.v.x; rx_.y = fromA_ ? rA.v.y : rB.v.y;                              \
        rx_.z = fromA_ ? rA.v.z : rB.v.z; rx_.w = rA.v.w;                                                \
        const float sx_ = fromA_ ? a.scaleA : 1.0f;                                                      \
        _Pragma("unroll") for (int s_ = 0; s_ < BS; ++s_) {                                              \
            BT.x[s_] = llvm_raw_buffer_load_f32(rx_, (int)off[(G) * BS + s_], choff_, 0);                \
            _Pragma("unroll") for (int n_ = 0; n_ < NT; ++n_)                                            \
                BT.w[n_][s_] = llvm_raw_buffer_load_f32(rW.v, lane * 4, ((cip_ * TAPS + (G) * BS + s_) * nt_all + nt0 + n_) * 256, 0); \
        }                                                                                                \
        BT.sx = sx_;                                              /* applied at MMA time: no wait on the loads here */ \
    }
#define SMVS_MMA_BATCH(BT)                                                                               \
    _Pragma("unroll") for (int s_ = 0; s_ < BS; ++s_)                                                    \
        _Pragma("unroll") for (int n_ = 0; n_ < NT; ++n_)                                                \
            acc[n_] = __builtin_amdgcn_mfma_f32_32x32x2f32(BT.w[n_][s_], BT.x[s_] * BT.sx, acc[n_], 0, 0, 0);
    static_assert(NB == 1 || NB == 3, "batching assumes 9 or 27 taps");
    if (NB == 3) {
        // per channel pair: batches g = 0,1,2, two register sets used alternately; the loop body covers TWO pairs so that the
        // sets are back in their roles at the back edge (no register rotation: copying a set waits for its loads).  All
        // loads are unconditional (see the 9-tap loop); past the end they fetch the last pair again and the MFMAs are skipped.
        Batch b0, b1;
        const int qe = q_end - 3;                                  // first batch of the last pair
        SMVS_LOAD_BATCH(0, b0, 0)
        for (int q = 0; q < q_end; q += 6) {
            SMVS_LOAD_BATCH(1, b1, q + 1)
            __builtin_amdgcn_sched_barrier(0);
            SMVS_MMA_BATCH(b0)
            __builtin_amdgcn_sched_barrier(0);
            SMVS_LOAD_BATCH(2, b0, q + 2)
            __builtin_amdgcn_sched_barrier(0);
            SMVS_MMA_BATCH(b1)
            __builtin_amdgcn_sched_barrier(0);
            SMVS_LOAD_BATCH(0, b1, min(q + 3, qe))
            __builtin_amdgcn_sched_barrier(0);
            SMVS_MMA_BATCH(b0)
            __builtin_amdgcn_sched_barrier(0);
            const bool second = q + 3 < q_end;                      // wave-uniform
            SMVS_LOAD_BATCH(1, b0, min(q + 4, qe + 1))
            __builtin_amdgcn_sched_barrier(0);
            if (second) SMVS_MMA_BATCH(b1)
            __builtin_amdgcn_sched_barrier(0);
            SMVS_LOAD_BATCH(2, b1, min(q + 5, qe + 2))
            __builtin_amdgcn_sched_barrier(0);
            if (second) SMVS_MMA_BATCH(b0)
            __builtin_amdgcn_sched_barrier(0);
            SMVS_LOAD_BATCH(0, b0, min(q + 6, qe))
            __builtin_amdgcn_sched_barrier(0);
            if (second) SMVS_MMA_BATCH(b1)
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
        // 9 taps: one batch per channel pair = 3 row loads (X) + 3*NT weight loads, NPF-1 pairs in flight while one is
        // multiplied.  Lane (j, h): position x0 + j, channel 2*cip + h of the pair.
        constexpr int NPF = NT == 1 ? MFMA_PREFETCH : 2;
        const int ix0 = ox * a.stride - 1;                       // column of the west tap
        const bool padL = ix0 < 0, padR = ix0 + 2 >= a.Wi;       // west / east tap is zero padding
        uint32_t roff[3];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy * a.stride - 1 + ky;
            const bool in = pos_ok && iy >= 0 && iy < a.Hi;
            roff[ky] = in ? (uint32_t)(((size_t)h * vol_i + (size_t)iy * a.Wi + (padL ? 0 : ix0)) * 4) : SMVS_OOB;
        }
        struct Batch9 { mf32x3 x[3]; mf32x4 w[NT][2]; float w8[NT]; float sx; };   // no dead load components: the compiler would reuse them
                                                                                    // as scratch and then has to wait for the load in flight
        Batch9 bb[NPF];
        // X operand of channel pair cip (A half or B half)
        auto load9 = [&](Batch9& B, int cip) {
            const bool fromA = 2 * cip < a.CA;                      // wave-uniform: scalar selects
            const int choff = (int)((size_t)(fromA ? 2 * cip : 2 * cip - a.CA) * vol_i * 4);
            i32x4 rx;
            rx.x = fromA ? rA.v.x : rB.v.x; rx.y = fromA ? rA.v.y : rB.v.y;
            rx.z = fromA ? rA.v.z : rB.v.z; rx.w = rA.v.w;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) B.x[ky] = llvm_raw_buffer_load_v3f32(rx, (int)roff[ky], choff, 0);
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const int wo = (cip * nt_all + nt0 + n) * (64 * MFMA9_WSLOT * 4);
                B.w[n][0] = llvm_raw_buffer_load_v4f32(rW.v, lane * (MFMA9_WSLOT * 4), wo, 0);
                B.w[n][1] = llvm_raw_buffer_load_v4f32(rW.v, lane * (MFMA9_WSLOT * 4) + 16, wo, 0);
                B.w8[n] = llvm_raw_buffer_load_f32(rW.v, lane * (MFMA9_WSLOT * 4) + 32, wo, 0);
            }
            B.sx = fromA ? a.scaleA : 1.0f;                         // applied at MMA time: no wait on the loads here
        };
        auto mma9 = [&](const Batch9& B) {
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                // loaded columns start at max(ix0, 0): shift right by one where the west tap is padding, drop the east one
                const float l0 = B.x[ky].x, l1 = B.x[ky].y, l2 = B.x[ky].z;
                float xv[3];
                xv[0] = padL ? 0.0f : l0;
                xv[1] = padL ? l0 : l1;
                xv[2] = padR ? 0.0f : (padL ? l1 : l2);
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int p = ky * 3 + kx;
#pragma unroll
                    for (int n = 0; n < NT; ++n)
                        acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(p < 8 ? B.w[n][(p >> 2) & 1][p & 3] : B.w8[n], xv[kx] * B.sx, acc[n], 0, 0, 0);
                }
            }
        };
        // Every load is UNCONDITIONAL (past the end: the last pair again, unused): a load under a branch makes the number
        // of outstanding operations unknown at the join, and the compiler then waits with vmcnt(0) before every batch of
        // MFMAs -- i.e. also for the batch it has just issued, and the prefetch hides nothing (that was the case until
        // round 2: ~1900 clocks per batch against 576 of MFMA issue).
        // Channel pairs [c_lo, c_hi) of this wave, in order
        const int c_lo = kw * per, c_hi = c_lo + q_end;
#pragma unroll
        for (int i = 0; i < NPF - 1; ++i) load9(bb[i], min(c_lo + i, c_hi - 1));
        for (int q = c_lo; q < c_hi; q += NPF) {
#pragma unroll
            for (int i = 0; i < NPF; ++i) {
                load9(bb[(i + NPF - 1) % NPF], min(q + i + NPF - 1, c_hi - 1));
                __builtin_amdgcn_sched_barrier(0);
                if (q + i < c_hi) mma9(bb[i]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
#undef SMVS_LOAD_BATCH
#undef SMVS_MMA_BATCH

    // ---- split-K reduction through LDS: waves 1..3 publish, wave 0 sums and finishes -----------------
    if (KS > 1) {
        if (kw > 0) {
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[tw * (KS - 1) + kw - 1][n * 16 + r][lane] = acc[n][r];
        }
        __syncthreads();
        if (kw > 0) return;
#pragma unroll 1
        for (int k = 0; k < KS - 1; ++k)     // one partial at a time: 16*NT loads in flight, not 16*NT*(KS-1)
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[n][r] += red[tw * (KS - 1) + k][n * 16 + r][lane];
    }
    if (!unit_ok) return;                    // (after the barrier) nothing to finish: the per-channel vectors below are indexed by the unit

    // D layout of 32x32 MFMA: register r of lane l holds row (r&3) + 8*(r>>2) + 4*(l>>5), column l&31
    const size_t vol_o = (size_t)a.Do * a.Ho * a.Wo;
    const size_t pos = ((size_t)od * a.Ho + oy) * a.Wo + ox;
    float s1 = 0.0f, s2 = 0.0f, t1 = 0.0f, t2 = 0.0f;     // stats of norm group 0 / 1
    // Every load of the epilogue is issued before the first use: on these small grids a wave sees the full memory
    // latency of each dependent access, and a load -> add -> store chain per register cost 16 round trips (measured:
    // the epilogue took as long as the K loop).  Cout is a multiple of 32 (mfma_conv_ok), so every row of the tile is
    // a real channel and the per-channel vectors are read as aligned float4 (rows r..r+3 are consecutive channels).
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int cb = (nt0 + n) * 32 + 4 * h;                      // channel of register 0; register r: cb + (r&3) + 8*(r>>2)
        float bi[16], sc[16], sh[16], sk[16], ini[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f), one = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
            const float4 tb = a.bias ? *reinterpret_cast<const float4*>(a.bias + cb + 8 * g) : zero;
            const float4 ts = a.scale ? *reinterpret_cast<const float4*>(a.scale + cb + 8 * g) : one;
            const float4 th = a.scale ? *reinterpret_cast<const float4*>(a.shift + cb + 8 * g) : zero;
            bi[4 * g] = tb.x; bi[4 * g + 1] = tb.y; bi[4 * g + 2] = tb.z; bi[4 * g + 3] = tb.w;
            sc[4 * g] = ts.x; sc[4 * g + 1] = ts.y; sc[4 * g + 2] = ts.z; sc[4 * g + 3] = ts.w;
            sh[4 * g] = th.x; sh[4 * g + 1] = th.y; sh[4 * g + 2] = th.z; sh[4 * g + 3] = th.w;
        }
        const size_t o0 = ((size_t)b * a.Cout + cb) * vol_o + pos;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            sk[r] = (a.skip && pos_ok) ? a.skip[o0 + (size_t)((r & 3) + 8 * (r >> 2)) * vol_o] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            ini[r] = (a.init && pos_ok) ? a.init[o0 + (size_t)((r & 3) + 8 * (r >> 2)) * vol_o] : 0.0f;
        if (pos_ok) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = cb + (r & 3) + 8 * (r >> 2);
                float v = acc[n][r];
                if (a.init) v += ini[r];
                if (a.bias) v += bi[r];
                if (a.scale) v = fmaf(v, sc[r], sh[r]);
                if (a.stats) {
                    if (a.ngroups == 2 && co >= a.Cout / 2) { t1 += v; t2 = fmaf(v, v, t2); }
                    else { s1 += v; s2 = fmaf(v, v, s2); }
                }
                if (a.relu) v = fmaxf(v, 0.0f);
                if (a.skip) v = sk[r] + v;
                a.out[o0 + (size_t)((r & 3) + 8 * (r >> 2)) * vol_o] = v;
            }
        }
    }
    if (a.stats) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            s1 += __shfl_xor(s1, m, 64); s2 += __shfl_xor(s2, m, 64);
            t1 += __shfl_xor(t1, m, 64); t2 += __shfl_xor(t2, m, 64);
        }
        if (lane == 0) {
            const int slot = (KS == NW ? bx : unit) % a.nslot;
            double* st = a.stats + (((size_t)b * a.ngroups + 0) * a.nslot + slot) * 2;
            atomicAdd(st, (double)s1);
            atomicAdd(st + 1, (double)s2);
            if (a.ngroups == 2) {
                double* su = a.stats + (((size_t)b * a.ngroups + 1) * a.nslot + slot) * 2;
                atomicAdd(su, (double)t1);
                atomicAdd(su + 1, (double)t2);
            }
        }
    }
}

template <int TAPS, int NT, int NW, int KS = NW>
__global__ __launch_bounds__(NW * 64)
void mfma_conv_kernel(const MfmaConvArgs a)
{
    __shared__ float smem[KS > 1 ? (NW - NW / KS) * NT * 16 * 64 : 1];
    mfma_conv_body<TAPS, NT, NW, KS>(a, blockIdx.x, blockIdx.y, smem);
}

// true if the MFMA kernel serves this layer
inline bool mfma_conv_ok(int CA, int CB, int Cout)
{
    const int Cin = CA + CB;
    return (Cout == 32 || Cout == 64 || Cout == 128) && Cin % 8 == 0 && CA % 2 == 0 && Cin >= 8;
}

inline size_t mfma_packed_floats(int cin, int cout, int taps) { return (size_t)(cin / 2) * (taps == 9 ? MFMA9_WSLOT : taps) * ((cout + 31) / 32) * 64; }

// Which instantiation serves a layer the MFMA kernel takes (mfma_conv_ok), from the geometry alone: `tiles_h` = tiles of 32 output positions
// of the batch the variant is chosen for, nt = Cout / 32, ncip = input channel pairs.  The values are the low digit of the MFMA codes of
// smvs_conv3x3_variant / smvs_conv3d_variant (include/satmvs.h).
// Few tiles (the coarse levels): latency, not throughput, sets the time -- one cout tile per workgroup
// and as many K-splitting waves as the channel count divides into.  Many tiles: one workgroup carries
// every cout tile so the X operand is loaded once.
// (at most 8 waves per workgroup)
enum MfmaForm { MFMA_FORM_K8 = SMVS_MFMA_K8, MFMA_FORM_K4 = SMVS_MFMA_K4, MFMA_FORM_NT1 = SMVS_MFMA_NT1, MFMA_FORM_NT2 = SMVS_MFMA_NT2, MFMA_FORM_NT4 = SMVS_MFMA_NT4 };
constexpr int MFMA_SMALL = 1024;             // tiles below which one cout tile per workgroup runs
inline long long mfma_conv_tiles(int Wo, int Ho, int Do, int B) { return (long long)((Wo + 31) / 32) * Ho * Do * B; }
inline MfmaForm mfma_conv_form(long long tiles_h, int nt, int ncip)
{
    if (tiles_h < MFMA_SMALL) return ncip % 8 == 0 ? MFMA_FORM_K8 : MFMA_FORM_K4;
    return nt == 1 ? MFMA_FORM_NT1 : nt == 2 ? MFMA_FORM_NT2 : MFMA_FORM_NT4;
}

template <int TAPS>
inline void mfma_conv_launch(const MfmaConvArgs& a, int B, hipStream_t st, int Bh = 0)   // Bh: batch the variant is chosen for (0 = B)
{
    const int tiles = (int)mfma_conv_tiles(a.Wo, a.Ho, a.Do, B);
    const int nt = a.Cout / 32, ncip = (a.CA + a.CB) / 2;
    switch (mfma_conv_form(mfma_conv_tiles(a.Wo, a.Ho, a.Do, Bh > 0 ? Bh : B), nt, ncip)) {
    case MFMA_FORM_K8:  hipLaunchKernelGGL((mfma_conv_kernel<TAPS, 1, 8>), dim3(tiles, nt), dim3(512), 0, st, a); break;
    case MFMA_FORM_K4:  hipLaunchKernelGGL((mfma_conv_kernel<TAPS, 1, 4>), dim3(tiles, nt), dim3(256), 0, st, a); break;
    case MFMA_FORM_NT1: hipLaunchKernelGGL((mfma_conv_kernel<TAPS, 1, 4>), dim3(tiles), dim3(256), 0, st, a); break;
    case MFMA_FORM_NT2: hipLaunchKernelGGL((mfma_conv_kernel<TAPS, 2, 4>), dim3(tiles), dim3(256), 0, st, a); break;
    case MFMA_FORM_NT4: hipLaunchKernelGGL((mfma_conv_kernel<TAPS, 4, 4>), dim3(tiles), dim3(256), 0, st, a); break;
    }
}

}  // namespace smvs
