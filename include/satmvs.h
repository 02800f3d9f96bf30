/*
 * satmvs.h -- C ABI of the MI355X-native RPC plane-sweep cost-volume engine (libsatmvs_hip.so).
 *
 * The reference (WHU-GPCV/SatMVS) has no FFI layer: its boundary is the Python operator surface
 * of modules/warping.py and networks/casred.py.  Each entry point below names the reference
 * function(s) it replaces (file:line under /root/reference); satmvs_amd/modules/warping.py and
 * satmvs_amd/networks/casred.py bind them with ctypes under the reference's own names, and
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - The caller owns every buffer.  All pointers are DEVICE pointers (HBM) unless stated;
 *     tensors are contiguous, float32 features/volumes in NCHW / NCDHW order, float64 camera
 *     parameters.  Nothing is allocated or freed inside the library.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Work is enqueued
 *     on it and the call returns without synchronising.
 *   - Return value: SMVS_OK (0) or an SMVS_ERR_* code; smvs_last_error() then returns a
 *     thread-local message.  Nothing is written on an argument error.
 *   - Re-entrant.  The caller selects the device (hipSetDevice / torch.cuda.device) before
 *     calling; nothing is cached per thread.  The only process-wide state is the DEFAULT arithmetic (smvs_set_arith; a call may
 *     carry its own) and a mutex-guarded,
 *     per-device pool of helper streams/events that smvs_red_pred_planes / smvs_red_volume_planes
 *     borrow for the duration of a call (bounded by the peak number of concurrent calls on a device).
 *   - The library never reads the environment and has no tuning builds: every kernel variant and
 *     threshold is fixed at compile time.
 *   - Deliberate differences from SURVEY.md section 8b's sketch: the Python binding is ctypes over
 *     this header (satmvs_amd/_lib.py), not a torch.utils.cpp_extension shim -- no torch types or
 *     headers are needed to build or call the library; and there is no smvs_shard_allreduce(ncclComm_t):
 *     the one exchange of the path (a (3,B,H,W) float64 slab, 7 MB at 768x384) goes through
 *     torch.distributed (backend "nccl" = RCCL), satmvs_amd/shard.py, DESIGN.md section 5.
 *   - depth_is_4d: 1 = per-voxel heights (B,D,H,W); 0 = per-plane heights (B,D) -- both forms
 *     of `depth_values` accepted by modules/warping.py:329-332; bits 8-9 may carry SMVS_CALL_ARITH_* (see smvs_set_arith).
 */
#ifndef SATMVS_H
#define SATMVS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SMVS_OK = 0, SMVS_ERR_ARG = 1, SMVS_ERR_LAUNCH = 2, SMVS_ERR_UNSUPPORTED = 3 };

/* Library identification: "satmvs-hip <version> gfx950". */
const char* smvs_version(void);
/* Message of the last failing call on this thread ("" if none). */
const char* smvs_last_error(void);
/* The plane pipelines (smvs_red_pred_planes / smvs_red_volume_planes) normally fan out over two library-owned
 * non-blocking helper streams joined to the caller's stream by events.  smvs_red_set_streams(0) keeps every launch
 * of later calls on the caller's stream (slower, but legal inside hipStreamBeginCapture / hipGraph capture);
 * any other value restores the default.  Process-wide, thread-safe; returns the previous setting (0 or 2). */
int smvs_red_set_streams(int n);
/* Arithmetic of the variance build (smvs_*_costvol_fwd[_gen], and the plane pipelines that call them).
 *   SMVS_ARITH_EXACT  the reference's float32 rounding sequence operation for operation (sum, sum of squares, two true
 *                     divisions by the view count, mean^2, subtract: networks/casred.py:26-53): bit-identical to the
 *                     CPU oracle; what every bit-level test runs.
 *   SMVS_ARITH_FUSED  the same float64 geometry, float32 tap coordinates and bilinear weights, but the variance
 *                     is taken of the differences to the ref feature with its constant factors folded into the weights
 *                     (11 instead of 22 packed operations per plane and channel pair at 3 views).  Differs from the
 *                     reference by float32 rounding only -- |delta| <= 1e-5 * max(1, |v|) on the volume (SURVEY.md
 *                     section 8c; measured <= 3.1e-6 on unit-variance features).  Against a float64 evaluation of the same
 *                     taps it is 6x closer than the reference's own sequence on photo-consistent features (no
 *                     meansq - mean^2 cancellation), equal on independent random features at 2-3 views, 2-4x the
 *                     reference's rounding error at 4-8 views (tests/test_fused_arith.py).
 * Which one a call runs:
 *   - a call may carry its own: OR SMVS_CALL_ARITH_EXACT or SMVS_CALL_ARITH_FUSED into the `depth_is_4d` argument of
 *     smvs_*_costvol_fwd / smvs_red_pred_planes / smvs_red_volume_planes, or set smvs_height_gen.arith for the *_gen forms
 *     (two models, or nn.DataParallel replicas on their threads, can run different arithmetics without shared state);
 *   - the STAND-ALONE builds (smvs_*_costvol_fwd[_gen][_pc]) without a bit take the process default, which starts as
 *     SMVS_ARITH_FUSED and is moved by smvs_set_arith (thread-safe; returns the previous default, -1 for an unknown mode);
 *   - the PLANE PIPELINES (smvs_red_pred_planes / smvs_red_volume_planes[_gen]) without a bit run SMVS_ARITH_EXACT whatever
 *     the process default is (round 6): behind a peaky softmax the fused volume's 1e-5 can move a regressed height by more
 *     than north_star's 1e-3 m (2.1e-3 m at 3 of 294 912 pixels of the well-conditioned 768 x 384 cascade,
 *     profiles/r05_cascade_float64.txt), and the build is a few per cent of a pipeline's time.  The Python networks and
 *     compute_depth_* functions default the same way (satmvs_amd/_lib.py, pipeline_arith_scope).
 * Every other entry point that takes `depth_is_4d` ignores the two bits. */
enum { SMVS_ARITH_EXACT = 0, SMVS_ARITH_FUSED = 1 };
enum { SMVS_CALL_ARITH_EXACT = 0x100, SMVS_CALL_ARITH_FUSED = 0x200, SMVS_CALL_ARITH_MASK = 0x300 };
int smvs_set_arith(int mode);
int smvs_get_arith(void);
/* Releases what the library keeps between calls (the pooled helper streams and events of the plane pipelines).
 * Call with no library work in flight, e.g. before unloading; later calls re-create what they need.  Returns SMVS_OK. */
int smvs_shutdown(void);

/* ---- height hypotheses generated inside the kernels ----------------------------
 * Stages 2 and 3 of the cascades derive their hypotheses from the previous stage's height map:
 * networks/casred.py:134-145 (bilinear resize to the image size, trilinear resize of the samples to the stage
 * size) + modules/depth_range.py:4-20 (cur -/+ ndepth/2*interval, ndepth samples).  The *_gen entry points below
 * take this description instead of a (B,D,H,W) tensor and evaluate it per pixel, with ATen's rounding.
 * `interval` is a double because the reference multiplies python floats before the single cast to float32.
 * Stage 1 needs no generator: its hypotheses are (B,D) planes (depth_is_4d = 0), exactly. */
typedef struct smvs_height_gen {
    const float* prev_height;   /* device, (B, prev_h, prev_w) float32: the previous stage's "depth" output */
    int prev_h, prev_w;
    int img_h, img_w;           /* image size; img / stage size must be 1 or 2 */
    int ndepth;                 /* D of this stage */
    double interval;            /* depth_inteval_pixel = depth_interals_ratio[stage] * min_interval */
    /* UCS-Net sampler (modules/depth_range.py:45-86 behind the two bilinear resizes of networks/ucs.py:49-58) when prev_var is
     * not null: hypotheses span prev_height -+ prev_var (both resized to this stage's grid, so img_h, img_w = the stage size),
     * clamped to [range_min[b], range_max[b]]; `interval` is ignored.  All three null: the interval sampler above. */
    const float* prev_var;      /* device, (B, prev_h, prev_w): the previous stage's "variance" output */
    const float* range_min;     /* device, (B): depth_values[:, 0] */
    const float* range_max;     /* device, (B): depth_values[:, -1] */
    int arith;                  /* 0, SMVS_CALL_ARITH_EXACT or SMVS_CALL_ARITH_FUSED: arithmetic of the variance build of THIS call */
} smvs_height_gen;
/* The hypotheses as a tensor (what the reference materialises), out (B,ndepth,H,W): training path and tests. */
int smvs_height_hypotheses(const smvs_height_gen* gen, float* out, int B, int H, int W, void* stream);

/* ---- fused warp + variance cost volume ----------------------------------------------------
 * Replaces the per-source loop  rpc_warping() + volume_sum/volume_sq_sum + variance
 *   modules/warping.py:310-365 (rpc_warping), networks/casred.py:22-53 (train, whole volume),
 *   networks/casred.py:191-212 (pred, one plane), networks/casmvs.py:26-59, networks/ucs.py:27-58.
 * ref_fea (B,C,H,W); src_fea: HOST array of n_src device pointers, each (B,C,H,W), in view order;
 * rpc (B,V,170) float64 with V = n_src+1 and view 0 = reference -- the layout of
 * `proj_matrices` before torch.unbind(.,1) (casred.py:13); depth per depth_is_4d.
 * Builds planes [d_begin,d_end) of the D hypotheses; plane d is written to plane index
 * d - d_begin + d_out_off of out_var (B,C,D_out,H,W).  (Whole volume: 0,D,D,0.  One plane of the
 * pred loop: d,d+1,1,0.  Depth shard g of G: g*D/G,(g+1)*D/G,D/G,0.)
 * variance = sq/V - (sum/V)^2 in float32, accumulated ref, src0, src1, ... like the reference. */
int smvs_rpc_costvol_fwd(const float* ref_fea, const float* const* src_fea, int n_src,
                         const double* rpc, const float* depth, int depth_is_4d, float* out_var,
                         int B, int C, int D, int H, int W,
                         int d_begin, int d_end, int D_out, int d_out_off, void* stream);

/* Same with the pinhole homography of modules/warping.py:6-44 (geo_model="pinhole").
 * proj (B,n_src,4,4) float64 = src_proj @ inverse(ref_proj) per source view, as produced by
 * smvs_homo_compose. */
int smvs_homo_costvol_fwd(const float* ref_fea, const float* const* src_fea, int n_src,
                          const double* proj, const float* depth, int depth_is_4d, float* out_var,
                          int B, int C, int D, int H, int W,
                          int d_begin, int d_end, int D_out, int d_out_off, void* stream);
/* ---- plane-constant heights: collapsed source cubics (round 6) -------------------------------------
 * Stage 1 of every reference cascade sweeps PLANE-CONSTANT heights (networks/casred.py:138-149,
 * modules/depth_range.py:23-42; modules/warping.py:329-332 accepts the (B,D) form, and the broadcast (B,D,H,W)
 * form carries the same numbers).  With a plane's height fixed, RPC_Obj2Photo's four trivariate cubics per source
 * view (modules/warping.py:218-252, RPC_PLH_COEF :183-207) are bivariate in (lat, lon): 10 coefficients instead of 20.
 *   smvs_rpc_plane_coef        folds them once per (batch item, plane, source) into `plane_coef`, a caller-owned device
 *                              buffer of smvs_rpc_plane_coef_bytes(B, n_src, D) bytes, 64-byte aligned (doubles: the planes'
 *                              heights -- depth[b,d], or depth[b,d,0,0] of a 4-D tensor -- at b D + d, padded to a multiple
 *                              of 8; 24 doubles per batch item: the views' reciprocal scales, divided once; then
 *                              [b][source][cubic][d][6]: the H-dependent 6 of the 10 bivariate coefficients of each
 *                              cubic); only planes [d_begin, d_end) are written (a plane-at-a-time caller folds what it builds).
 *   smvs_rpc_costvol_fwd_pc    = smvs_rpc_costvol_fwd with that buffer (NULL: identical to smvs_rpc_costvol_fwd).  A wave
 *                              runs its source-view geometry from the folded records (heights, scales and cubics all
 *                              come from the workspace, so nothing waits on the depth tensor) and THEN compares its own
 *                              heights with the folded planes'; if any differs (per-voxel hypotheses, a jittered pixel,
 *                              NaN) it discards that work and evaluates the trivariate cubics on its own heights -- the
 *                              result never depends on trusting the caller, but heights that are not plane-constant pay
 *                              for both (cfg2 tile: 0.73 vs 0.58 ms), so send those to smvs_rpc_costvol_fwd.
 * Same polynomials re-associated: source coordinates move by float64 rounding (~1e-13 px), volumes stay inside every
 * tolerance of smvs_rpc_costvol_fwd.  `plane_coef` must have been prepared from the same rpc / depth / D; it can be
 * reused for any number of launches (plane windows, shards) of that geometry.  rpc (B,V,170), V = n_src + 1. */
size_t smvs_rpc_plane_coef_bytes(int B, int n_src, int D);
int smvs_rpc_plane_coef(const double* rpc, const float* depth, int depth_is_4d, double* plane_coef,
                        int B, int n_src, int D, int H, int W, int d_begin, int d_end, void* stream);
int smvs_rpc_costvol_fwd_pc(const float* ref_fea, const float* const* src_fea, int n_src,
                            const double* rpc, const float* depth, int depth_is_4d, const double* plane_coef,
                            float* out_var, int B, int C, int D, int H, int W,
                            int d_begin, int d_end, int D_out, int d_out_off, void* stream);

/* The same two launches with the heights generated in the kernel (see smvs_height_gen above). */
int smvs_rpc_costvol_fwd_gen(const float* ref_fea, const float* const* src_fea, int n_src,
                             const double* rpc, const smvs_height_gen* gen, float* out_var,
                             int B, int C, int D, int H, int W,
                             int d_begin, int d_end, int D_out, int d_out_off, void* stream);
int smvs_homo_costvol_fwd_gen(const float* ref_fea, const float* const* src_fea, int n_src,
                              const double* proj, const smvs_height_gen* gen, float* out_var,
                              int B, int C, int D, int H, int W,
                              int d_begin, int d_end, int D_out, int d_out_off, void* stream);

/* ---- stand-alone warps (the operator surface itself) ------------------------------------------
 * smvs_rpc_warp_fwd  = rpc_warping(src_fea, src_rpc, ref_rpc, depth_values, coef)
 *                      modules/warping.py:310-365 (coef is not needed); also serves
 *                      rpc_warping_enisum (:139-178) after the QC tensors are mapped back to the
 *                      20 coefficients on the host.  src_rpc, ref_rpc (B,170); out (B,C,D,H,W).
 * smvs_rpc_warp_bwd  = its autograd w.r.t. src_fea (the grid is built under no_grad,
 *                      warping.py:322): grad_src (B,C,H,W) must be zero-filled by the caller,
 *                      contributions are accumulated with float32 atomics. */
int smvs_rpc_warp_fwd(const float* src_fea, const double* src_rpc, const double* ref_rpc,
                      const float* depth, int depth_is_4d, float* out,
                      int B, int C, int D, int H, int W, void* stream);
int smvs_rpc_warp_bwd(const float* grad_out, const double* src_rpc, const double* ref_rpc,
                      const float* depth, int depth_is_4d, float* grad_src,
                      int B, int C, int D, int H, int W, void* stream);

/* homo_warping(src_fea, src_proj, ref_proj, depth_values), modules/warping.py:6-44.
 * proj (B,4,4) = src_proj @ inverse(ref_proj) from smvs_homo_compose. */
int smvs_homo_warp_fwd(const float* src_fea, const double* proj, const float* depth, int depth_is_4d,
                       float* out, int B, int C, int D, int H, int W, void* stream);
int smvs_homo_warp_bwd(const float* grad_out, const double* proj, const float* depth, int depth_is_4d,
                       float* grad_src, int B, int C, int D, int H, int W, void* stream);
/* out[b] = src_proj[b] @ inverse(ref_proj[b]) (warping.py:19), 4x4 float64, n matrices. */
int smvs_homo_compose(const double* src_proj, const double* ref_proj, double* out, int n, void* stream);

/* ---- backward of the fused volume (train.py:284 loss.backward through casred.py:22-53) -------
 * grad_var (B,C,D,H,W) -> grad_ref (B,C,H,W) and grad_src[s] (B,C,H,W), all ACCUMULATED with
 * float32 atomics (zero-filled by the caller; grad_src is a HOST array of n_src device pointers).  geo_kind 0 = rpc (B,V,170), 1 = homography
 * (B,n_src,4,4).  Recomputes the taps instead of saving a warped volume.  Where the taps of a wave's 32 x 2 pixels x 8
 * planes fall into a 64 x 8-cell box of every source view (up to four source views) the contributions are summed in
 * float64 in LDS first and reach memory as one float32 atomic per touched cell; summation order is not fixed either way
 * (atomics), values differ from a sequential float32 sum by rounding only.  Limits: C*H*W*4 < 2 GiB, H, W <= 32766. */
int smvs_costvol_bwd(int geo_kind, const float* grad_var, const float* ref_fea, const float* const* src_fea,
                     int n_src, const double* geo, const float* depth, int depth_is_4d,
                     float* grad_ref, float* const* grad_src,
                     int B, int C, int D, int H, int W, void* stream);

/* ---- batch projectors --------------------------------------------------------------------------
 * RPC_Photo2Obj / RPC_Obj2Photo (modules/warping.py:255-307, :218-252) and the offline-tool twins
 * tools/RPCCore.py:424-489, tools/rpc_tensor.py:109-165 on flat float64 arrays.
 * dir 0: (samp, line, h) -> (lat, lon);  dir 1: (lat, lon, h) -> (samp, line).
 * rpc170: one 170-vector (device).  a, b, h, o0, o1: n doubles each (device). */
int smvs_rpc_project(const double* rpc170, const double* a, const double* b, const double* h,
                     double* o0, double* o1, size_t n, int dir, void* stream);

/* ---- geometric-consistency check (post-processing) ---------------------------------
 * One (reference, source) pair of tools/rpc_filter.py:11-70 (reproject_with_depth + check_geometric_consistency):
 * reference pixel + height -> ground -> source image (float64); the source height map sampled there like
 * cv2.remap(INTER_LINEAR, BORDER_CONSTANT, -999) on float32 coordinates; back to the ground with the sampled
 * height and into the reference image; mask = (|reprojected - pixel| < p_ratio) & (|sampled - height| < d_ratio).
 * depth_ref (H,W), depth_src (Hs,Ws) float32; rpc_* 170 float64; mask (H,W) uint8; depth_reproj (H,W) float32: 0 outside
 * the mask when x_back/y_back are NULL (check_geometric_consistency), the raw sampled height everywhere when they are
 * given (reproject_with_depth); x_src, y_src (H,W) float64 source-image coordinates; x_back, y_back (H,W) float64 or
 * both NULL. */
int smvs_rpc_geo_consistency(const float* depth_ref, const double* rpc_ref, const float* depth_src,
                             const double* rpc_src, int H, int W, int Hs, int Ws, double p_ratio, double d_ratio,
                             unsigned char* mask, float* depth_reproj, double* x_src, double* y_src,
                             double* x_back, double* y_back, void* stream);

/* The pinhole twin: one (reference, source) pair of tools/pinhole_filter.py:7-67 (reproject_with_depth +
 * check_geometric_consistency).  mats (device): P_ref, inverse(P_ref), P_src, inverse(P_src), row-major 4 x 4 float64 with
 * P = [K @ E[:3]; 0 0 0 1] (:17-24; formed and inverted by the caller, on the host like the reference).  Reference pixel * depth
 * -> world -> source pixel in float64, float32 coordinates into cv2.remap(INTER_LINEAR, default border: constant 0), the
 * sampled depth back into the reference view; mask = (|reprojected - pixel| < p_thre) & (|sampled - depth| / depth <
 * float32(relative_d_thre)).  depth_ref (H,W), depth_src (Hs,Ws) float32; mask uint8; depth_reproj float32 (0 outside the
 * mask when x_back / y_back are NULL, the raw sampled depth when they are given); x_src, y_src, x_back, y_back (H,W) float32. */
int smvs_pinhole_geo_consistency(const float* depth_ref, const float* depth_src, const double* mats,
                                 int H, int W, int Hs, int Ws, double p_thre, double relative_d_thre,
                                 unsigned char* mask, float* depth_reproj, float* x_src, float* y_src,
                                 float* x_back, float* y_back, void* stream);

/* ---- GroupNorm(1, C) of the recurrent regulariser, training path -------------------------------------
 * reference: modules/module.py:15-20 (three nn.GroupNorm(1, C, 1e-5) per ConvGRU cell) and :38-52 (sigmoid / tanh of
 * the normalised gates); differentiated by train.py:284.  x (B,C,HW) float32 with batch stride x_batch_stride elements
 * (>= C*HW: the two gate halves of a (B,2C,H,W) tensor are normalised where they lie); act 0 none, 1 sigmoid, 2 tanh:
 *   y = act((x - mean_b) * rstd_b * gamma_c + beta_c),   mean / variance over the C*HW values of sample b.
 * mean_rstd (B,2) float32 out (kept for the backward); workspace: 2*B*ceil(C*HW/4096) doubles (forward), 2*B*C*ceil(HW/4096) doubles
 * (backward), caller-owned, contents irrelevant on entry.  Backward: dx (batch stride dx_batch_stride), dgamma (C),
 * dbeta (C) are overwritten; y = the forward's output (needed when act != 0).  Statistics and the reductions of the
 * backward are accumulated in float64, without atomics (fixed order: deterministic). */
int smvs_groupnorm1_fwd(const float* x, long long x_batch_stride, const float* gamma, const float* beta, float eps,
                        int act, float* y, float* mean_rstd, double* workspace, int B, int C, int HW, void* stream);
int smvs_groupnorm1_bwd(const float* dy, const float* x, long long x_batch_stride, const float* y, const float* gamma,
                        const float* mean_rstd, int act, float* dx, long long dx_batch_stride, float* dgamma,
                        float* dbeta, double* workspace, int B, int C, int HW, void* stream);

/* Weight and bias gradient of a 3x3, stride-1, pad-1 convolution (the ConvGRU cells' gate_conv / output_conv, modules/module.py:13-14
 * under loss.backward(), train.py:284):  dw[co][ci][ky][kx] += sum_{b,y,x} dy[b][co][y][x] * x[b][ci][y+ky-1][x+kx-1],
 * db[co] += sum dy[b][co][y][x].  x (B,Cin,H,W), dy (B,Cout,H,W), dw (Cout,Cin,3,3), db (Cout) or NULL; dw and db are ACCUMULATED
 * with float atomics -- the caller zero-fills them for a plain gradient. */
int smvs_conv3x3_wgrad(const float* x, const float* dy, float* dw, float* db, int B, int Cin, int Cout, int H, int W, void* stream);
/* The same correlation with the window tensor read at `stride` 1 or 2 -- the weight gradient of every 3x3 layer of the RED
 * regulariser (modules/module.py:595-693 under loss.backward()):
 *   dw[g][c][ky][kx] += sum_{b,y,x} grid[b][g][y][x] * window[b][c][stride*y + ky - 1][stride*x + kx - 1]
 * grid (B,Cgrid,H,W), window (B,Cwin,stride*H,stride*W), dw (Cgrid,Cwin,3,3); dgrid_sum (Cgrid) += sum of grid, or NULL.
 *   nn.Conv2d(stride s, pad 1): window = input, grid = output gradient -> dw = weight gradient (Cout,Cin,3,3), dgrid_sum = bias gradient;
 *   nn.ConvTranspose2d(stride s, pad 1, output_padding s-1): window = output gradient, grid = input -> dw = weight gradient
 *   (Cin_layer,Cout_layer,3,3) (its bias gradient is the plain sum of the output gradient: not computed here). */
int smvs_conv3x3_wgrad_strided(const float* window, const float* grid, float* dw, float* dgrid_sum,
                               int B, int Cwin, int Cgrid, int H, int W, int stride, void* stream);
/* smvs_conv3x3_wgrad for a convolution over cat(xA, xB) without the concatenated tensor: xA (B,CA,H,W), xB (B,CB,H,W) (CB = 0: xA only;
 * CA even otherwise), dw (Cout, CA+CB, 3, 3). */
int smvs_conv3x3_wgrad_cat(const float* xA, int CA, const float* xB, int CB, const float* dy, float* dw, float* db,
                           int B, int Cout, int H, int W, void* stream);
/* The same sums over a LIST of n tensors (host arrays of n device pointers each; win2 NULL when CB = 0) of Bper samples each -- the planes
 * of a training step's plane loop, whose activations and gradients are separate allocations: one launch per layer and step instead of one
 * per layer and plane.  window tensors (Bper, CA [+ CB], stride*H, stride*W), grid tensors (Bper, Cgrid, H, W); dw (Cgrid, CA+CB, 3, 3)
 * and dgrid_sum (Cgrid, or NULL) are accumulated into (the caller zeroes them). */
int smvs_conv3x3_wgrad_list(const float* const* win, const float* const* win2, const float* const* grid, int n,
                            float* dw, float* dgrid_sum, int Bper, int CA, int CB, int Cgrid, int H, int W, int stride, void* stream);
/* How the four entries above cut a launch over B samples in all (the list form: n * Bper per launch of at most 64 tensors) into waves --
 * the function the launcher itself asks.  Host code only: no HIP call, usable without a GPU.  SMVS_ERR_ARG exactly where the launcher
 * rejects the dimensions.  plan = {bchunk, nbc, rows, nrc, nxs, waves}: a wave owns 2 window channels x 8 grid channels x one of nxs strips
 * of 64 columns x one of nrc chunks of `rows` rows x one of nbc chunks of `bchunk` samples (row chunks only at one sample per wave). */
int smvs_conv3x3_wgrad_plan(int B, int Cin, int Cout, int H, int W, int stride, int plan[6]);

/* Weight gradient of the 3x3x3 / pad 1 layers of the 3-D regulariser CostRegNet (modules/module.py:324-410, 546-577 under
 * loss.backward(), train.py:284 with --model casmvs / ucs) -- the 2-D correlation above with a depth axis:
 *   dw[g][c][kd][ky][kx] += sum_{b,d,y,x} grid[b][g][d][y][x] * window[b][c][s*d + kd - 1][s*y + ky - 1][s*x + kx - 1]
 * grid (B,Cgrid,D,H,W), window (B,Cwin,s*D,s*H,s*W), dw (Cgrid,Cwin,3,3,3) ACCUMULATED into (the caller zero-fills it), s = stride 1 or 2.
 *   nn.Conv3d(stride s, pad 1): window = input, grid = output gradient -> dw = weight gradient (Cout,Cin,3,3,3);
 *   nn.ConvTranspose3d(stride 2, pad 1, output_padding 1): window = output gradient, grid = input -> dw = weight gradient
 *   (Cin_layer,Cout_layer,3,3,3).  Volumes are read in place through their (B,C,D,H,W) strides; a channel of either tensor must stay
 *   below 2^31 bytes (SMVS_ERR_ARG otherwise: callers keep torch's operator).
 *   workspace: NULL -- the waves add their partial sums to dw with float atomics (order-dependent rounding; the ~100-400 waves that
 *   share 144 weights serialise on five cache lines) -- or smvs_conv3d_wgrad_workspace_floats(...) floats of scratch: the waves store their
 *   partial sums there and a second kernel adds them to dw in a fixed order (deterministic, and what the shipped training path uses). */
size_t smvs_conv3d_wgrad_workspace_floats(int B, int Cwin, int Cgrid, int D, int H, int W);
int smvs_conv3d_wgrad(const float* window, const float* grid, float* dw, float* workspace, size_t workspace_floats, int B, int Cwin,
                      int Cgrid, int D, int H, int W, int stride, void* stream);
/* The split smvs_conv3d_wgrad takes, atomic form (two_stage = 0) or with a workspace (two_stage != 0) -- the function the launcher itself
 * asks; host code only, SMVS_ERR_ARG exactly where the launcher rejects the dimensions.  plan = {dchunk, ndc, rows, nrc, nxs, waves}: a
 * wave owns 2 window channels x 8 grid channels (1 when Cgrid = 1) x one depth tap x one of nxs column strips x one of nrc row chunks x
 * one of ndc chunks of `dchunk` grid planes of one sample; waves (all of them) saturates at INT_MAX.  The workspace holds 144 floats per
 * wave: smvs_conv3d_wgrad_workspace_floats = ceil(Cwin/2) * ceil(Cgrid/8) * 3 * (B * ndc * nxs * nrc) * 144 of the two-stage plan. */
int smvs_conv3d_wgrad_plan(int B, int Cwin, int Cgrid, int D, int H, int W, int stride, int two_stage, int plan[6]);

/* A single 3x3x3 / pad 1 layer of CostRegNet as a stand-alone call on the kernels of smvs_costreg_fwd (direct or MFMA by channel
 * count) WITHOUT the folded BatchNorm -- the TRAINING forward of its convolutions (modules/module.py:324-410 under autograd, batch
 * statistics follow as a separate operator) and their input gradients, which are the adjoint layers on the same kernels:
 *   smvs_conv3d_packed_floats(cin, cout)  floats of the packed weights of a layer from cin to cout channels
 *   smvs_conv3d_pack(w, packed, cin, cout, layout): weights read from w as
 *       layout 0: w[co][ci][27]       an nn.Conv3d weight (kinds 0 / 1); the input gradient of an nn.ConvTranspose3d of weight (cout,cin,27)
 *       layout 1: w[ci][co][27]       scatter taps for kind 2: an nn.ConvTranspose3d(stride 2) weight; the input gradient of a stride-2
 *                                     nn.Conv3d of weight (cin, cout, 27)
 *       layout 2: w[ci][co][26 - k]   the input gradient of a stride-1 nn.Conv3d of weight (cin, cout, 27) as a correlation (kind 0)
 *   smvs_conv3d_fwd(kind, ...)  out = [relu](layer(in (B,Cin,Di,Hi,Wi))) [+ skip]
 *       kind 0: correlation, stride 1, out (B,Cout,Di,Hi,Wi);   kind 1: correlation, stride 2 (even dims), out (B,Cout,Di/2,Hi/2,Wi/2);
 *       kind 2: transposed convolution, stride 2, output_padding 1, out (B,Cout,2Di,2Hi,2Wi).   skip: NULL or a tensor of out's shape. */
size_t smvs_conv3d_packed_floats(int cin, int cout);
int smvs_conv3d_pack(const float* w, float* packed, int cin, int cout, int layout, void* stream);
int smvs_conv3d_fwd(int kind, const float* in, const float* packed, const float* skip, float* out, int B, int Cin, int Cout,
                    int Di, int Hi, int Wi, int relu, void* stream);
/* Which kernel smvs_conv3d_fwd runs for these arguments (Di, Hi, Wi: the INPUT volume) -- the function the launcher itself asks.  Host code
 * only: no HIP call, usable without a GPU.  Negative: smvs_conv3d_fwd rejects the arguments (SMVS_ERR_ARG).
 *   SMVS_CONV3D_S1_COT2     stride-1 row kernel on 62-column tiles, 2 output channels per lane (Cout <= 2)
 *   SMVS_CONV3D_S1_COT8     the same, 8 output channels per lane
 *   SMVS_CONV3D_S2          stride-2 direct gathers
 *   SMVS_CONV3D_T_SPLIT     transposed, linear voxels, input channels split over 4 waves (below 512 workgroups)
 *   SMVS_CONV3D_T_UNSPLIT   transposed, 64 x 4 input rows per workgroup
 *   SMVS_CONV3D_MFMA_S1 / SMVS_CONV3D_MFMA_S2 + SMVS_MFMA_*   the MFMA kernel (Cout 32 / 64 / 128, Cin a multiple of 8), stride 1 / 2 */
enum { SMVS_CONV3D_S1_COT2 = 0, SMVS_CONV3D_S1_COT8 = 1, SMVS_CONV3D_S2 = 2, SMVS_CONV3D_T_SPLIT = 3, SMVS_CONV3D_T_UNSPLIT = 4,
       SMVS_CONV3D_MFMA_S1 = 10, SMVS_CONV3D_MFMA_S2 = 20 };
/* form of an MFMA launch, added to SMVS_CONV3D_MFMA_S* / SMVS_CONV3X3_MFMA_S*.  Below 1024 tiles of 32 output positions: one tile of 32 output
 * channels per workgroup, input channels split over 8 waves (K8; (Cin / 2) % 8 == 0) or 4 (K4).  From 1024 tiles: 4 waves, every cout tile in
 * one workgroup: NT1 / NT2 / NT4 for Cout 32 / 64 / 128. */
enum { SMVS_MFMA_K8 = 0, SMVS_MFMA_K4 = 1, SMVS_MFMA_NT1 = 2, SMVS_MFMA_NT2 = 3, SMVS_MFMA_NT4 = 4 };
int smvs_conv3d_variant(int kind, int B, int Cin, int Cout, int Di, int Hi, int Wi);

/* nn.BatchNorm3d in TRAINING form (batch statistics over (B, N = D*H*W) per channel) with the block's ReLU -- the normalisation of every
 * Conv3d / Deconv3d block of CostRegNet under autograd (modules/module.py:324-410):
 *   fwd: y = [relu]((x - mean) * rstd * gamma + beta);  saved_mean_rstd (C,2) for the backward (an opaque pair: the mean is kept
 *        relative to the channel's first element, which both directions re-read from x, so that |mean| >> std loses nothing);  running_mean / running_var (or NULL, NULL)
 *        updated like torch.nn.functional.batch_norm(training=True): (1 - momentum) * running + momentum * batch (unbiased variance);
 *        num_batches_tracked (int64 scalar on the device, or NULL) += 1 like nn.BatchNorm's forward
 *   bwd: dx, dgamma (C), dbeta (C) from dy, the layer's INPUT x and saved_mean_rstd; with relu != 0 the gradient passes where the forward's
 *        output was positive (recomputed from x: neither a mask nor the output is kept)
 * x, y, dy, dx: (B,C,N) contiguous float32; workspace: 2*C doubles of scratch, cleared by the call unless `relu` carries
 * SMVS_BN_WORKSPACE_ZERO (the caller hands over zeroed memory: one fill for all the layers of a forward).  relu: bit 0 = apply ReLU.
 * Neither direction runs in place: y == x (forward) and dx == x (backward) are SMVS_ERR_ARG, because every block of a channel re-reads
 * the channel's first element of x while the channel's first block would be overwriting it.  saved_mean_rstd[2c] + x[0, c, 0] is the
 * batch mean of channel c, saved_mean_rstd[2c + 1] its 1 / sqrt(var + eps). */
#define SMVS_BN_WORKSPACE_ZERO 2
int smvs_batchnorm_train_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                             long long* num_batches_tracked, float momentum, float eps, int relu, float* y, float* saved_mean_rstd,
                             double* workspace, int B, int C, long long N, void* stream);
int smvs_batchnorm_train_bwd(const float* dy, const float* x, const float* gamma, const float* beta, const float* saved_mean_rstd, int relu,
                             float* dx, float* dgamma, float* dbeta, double* workspace, int B, int C, long long N, void* stream);

/* A single 3x3 / pad 1 layer of the RED regulariser as a stand-alone call on the kernels of the plane loop -- the TRAINING forward of
 * its convolutions (modules/module.py:34-57, :625-644 under autograd) and their input gradients:
 *   smvs_conv3x3_packed_floats(cin, cout)  floats of the packed weights
 *   smvs_conv3x3_pack(w, packed, cin, cout, layout): the correlation from cin to cout channels whose weights are read from w as
 *       layout 0: w[co][ci][ky][kx]      an nn.Conv2d weight (stride 1 / 2); the input gradient of an nn.ConvTranspose2d of weight (cout,cin,3,3)
 *       layout 1: w[ci][co][ky][kx] kept as scatter taps for kind 2: an nn.ConvTranspose2d(stride 2) weight; the input gradient of a
 *                                        stride-2 nn.Conv2d of weight (cin, cout, 3, 3)
 *       layout 2: w[ci][co][2-ky][2-kx]  a stride-1 nn.ConvTranspose2d as a correlation; the input gradient of a stride-1 nn.Conv2d of
 *                                        weight (cin, cout, 3, 3)
 *   smvs_conv3x3_fwd(kind, ...)  out = [relu](layer(cat(xA (B,CA,H,W), xB (B,CB,H,W) or NULL)) + bias (Cout) or NULL)
 *       kind 0: correlation, stride 1, out (B,Cout,H,W);   kind 1: correlation, stride 2 (H, W even), out (B,Cout,H/2,W/2);
 *       kind 2: transposed convolution, stride 2, pad 1, output_padding 1 (layout-1 weights; one operand, no bias), out (B,Cout,2H,2W)
 * float32; accumulation in input-channel order (direct kernels) or as a k-ordered fmaf chain on v_mfma_f32_32x32x2_f32 (correlations
 * with 32 / 64 / 128 output channels): same class of rounding as torch's direct convolution, 2e-5 relative in the tests. */
size_t smvs_conv3x3_packed_floats(int cin, int cout);
int smvs_conv3x3_pack(const float* w, float* packed, int cin, int cout, int layout, void* stream);
int smvs_conv3x3_fwd(int kind, const float* xA, int CA, const float* xB, int CB, const float* packed, const float* bias, const float* init,
                     float* out, int B, int Cout, int H, int W, int relu, void* stream);
/* init (kinds 0 / 1; same shape as out, or NULL; may be out itself): added to the sums before bias / ReLU -- an input gradient that continues
 * the contributions already collected for that tensor (whole-cell ConvGRU backward). */
/* Which kernel smvs_conv3x3_fwd runs for these arguments (H, W: the INPUT plane; bias_aligned: no bias, or a 16-byte aligned one) -- the
 * function the launchers themselves ask.  Host code only: no HIP call, usable without a GPU.  Negative: smvs_conv3x3_fwd rejects the
 * dimensions (SMVS_ERR_ARG).  Workgroups are counted as 64 x 4 output pixels (transposed: input pixels) x groups of 8 output channels:
 *   SMVS_CONV3X3_SPLIT_S1 / _S2      direct, stride 1 / 2, 4 waves split the input channels (below 512 workgroups in the batch)
 *   SMVS_CONV3X3_UNSPLIT_S1 / _S2    direct, stride 1 / 2, 64 x 4 output pixels per workgroup
 *   SMVS_CONV3X3_ROWS4               direct, stride 1, four output rows per lane (from 1024 workgroups in ONE sample)
 *   SMVS_CONV3X3_T_SPLIT / _T_UNSPLIT    transposed, below / from 512 workgroups
 *   SMVS_CONV3X3_MFMA_S1 / SMVS_CONV3X3_MFMA_S2 + SMVS_MFMA_*   the MFMA kernel (Cout 32 / 64 / 128, CA + CB a multiple of 8, CA even, bias
 *                                    aligned), stride 1 / 2, forms as above */
enum { SMVS_CONV3X3_SPLIT_S1 = 0, SMVS_CONV3X3_SPLIT_S2 = 1, SMVS_CONV3X3_UNSPLIT_S1 = 2, SMVS_CONV3X3_UNSPLIT_S2 = 3, SMVS_CONV3X3_ROWS4 = 4,
       SMVS_CONV3X3_T_SPLIT = 5, SMVS_CONV3X3_T_UNSPLIT = 6, SMVS_CONV3X3_MFMA_S1 = 10, SMVS_CONV3X3_MFMA_S2 = 20 };
int smvs_conv3x3_variant(int kind, int B, int CA, int CB, int Cout, int H, int W, int bias_aligned);

/* Both gate norms of a ConvGRU cell in one call (modules/module.py:15-16, :37-40): x (B, 2C, HW) contiguous = the gate
 * convolution's output; channels [0, C) are normalised with (gamma, beta), channels [C, 2C) with (gamma2, beta2), each half
 * over its own C*HW values, then the activation.  y and dx (B, 2C, HW); mean_rstd (2B, 2) (sample 2b + half); workspace
 * as for smvs_groupnorm1_* with 2B samples (4*B*ceil(C*HW/4096) / 4*B*C*ceil(HW/4096) doubles). */
int smvs_groupnorm1_pair_fwd(const float* x, const float* gamma, const float* beta, const float* gamma2, const float* beta2,
                             float eps, int act, float* y, float* mean_rstd, double* workspace, int B, int C, int HW,
                             void* stream);
/* The same two forwards with the cell's next step folded into the apply pass (one launch per step and cell less, each):
 *   _fwd_blend:      additionally out = u * h + (1 - u) * y (modules/module.py:57); u (B,C,HW) at batch stride u_batch_stride elements
 *                    (the u half of the (B,2C,H,W) gate tensor), h and out (B,C,HW) contiguous; y is written as well (the backward needs it);
 *   _pair_fwd_mul:   additionally rh = y[:, :C] * h (modules/module.py:43: the second operand of the candidate convolution, which
 *                    smvs_conv3x3_fwd takes as (x, rh): no concatenation); h, rh (B,C,HW) contiguous. */
int smvs_groupnorm1_fwd_blend(const float* x, long long x_batch_stride, const float* gamma, const float* beta, float eps,
                              int act, float* y, float* mean_rstd, double* workspace, const float* u, long long u_batch_stride,
                              const float* h, float* out, int B, int C, int HW, void* stream);
int smvs_groupnorm1_pair_fwd_mul(const float* x, const float* gamma, const float* beta, const float* gamma2, const float* beta2,
                                 float eps, int act, float* y, float* mean_rstd, double* workspace, const float* h, float* rh,
                                 int B, int C, int HW, void* stream);
int smvs_groupnorm1_pair_bwd(const float* dy, const float* x, const float* y, const float* gamma, const float* gamma2,
                             const float* mean_rstd, int act, float* dx, float* dgamma, float* dbeta, float* dgamma2,
                             float* dbeta2, double* workspace, int B, int C, int HW, void* stream);

/* The ConvGRU cell's element-wise steps (modules/module.py:43-44 and :57), training path, one launch each way:
 *   smvs_gru_mul_cat:  out (B, Cx+Ch, HW) = cat(x (B,Cx,HW), r * h (B,Ch,HW));   backward: dr = dcat[:, Cx:] * h, dh = dcat[:, Cx:] * r
 *                      (dx is the first Cx channels of dcat as they are)
 *   smvs_gru_blend:    out = u * h + (1 - u) * y over n contiguous floats (pointers 16-byte aligned);
 *                      backward: du = dy (h - y), dh = dy u, dcand = dy (1 - u). */
int smvs_gru_mul_cat_fwd(const float* x, const float* r, const float* h, float* out, int B, int Cx, int Ch, int HW, void* stream);
int smvs_gru_mul_cat_bwd(const float* dcat, const float* r, const float* h, float* dr, float* dh, int B, int Cx, int Ch, int HW, void* stream);
/* the same with the state gradient accumulated and stored in place: dcat[:, Cx:] <- dcat[:, Cx:] * r + dh_acc; dr = dcat[:, Cx:] * h */
int smvs_gru_mul_cat_bwd_acc(float* dcat, const float* r, const float* h, const float* dh_acc, float* dr, int B, int Cx, int Ch, int HW, void* stream);
int smvs_gru_blend_fwd(const float* u, const float* h, const float* y, float* out, long long n, void* stream);
int smvs_gru_blend_bwd(const float* dy, const float* u, const float* h, const float* y, float* du, float* dh, float* dcand, long long n, void* stream);

/* ---- regression ----------------------------------------------------------------------------------
 * Train path: softmax over D + expected height + max probability,
 *   networks/casred.py:58-62 and modules/module.py:433-439 (depth_regression).
 * reg (B,D,H,W) float32 regulariser output; out_depth, out_conf (B,H,W). */
int smvs_softmax_regress_fwd(const float* reg, const float* depth, int depth_is_4d,
                             float* out_depth, float* out_conf, int B, int D, int H, int W, void* stream);
/* CascadeMVSNet / UCSNet flavour: softmax over D + expected height + the probability mass of the four hypotheses
 * around the expected index (networks/casmvs.py:66-74: F.pad(.,(1,2)) + 4*avg_pool3d((4,1,1)) gathered at
 * clamp(trunc(E[index]))), and, when out_var is not NULL, UCSNet's lamb * sqrt(sum p*(h - depth)^2)
 * (networks/ucs.py:73-74).  reg (B,D,H,W); out_depth, out_conf, out_var (B,H,W). */
int smvs_window_regress_fwd(const float* reg, const float* depth, int depth_is_4d,
                            float* out_depth, float* out_conf, float* out_var, float lamb,
                            int B, int D, int H, int W, void* stream);
/* softmax / window regression with the heights generated in the kernel (smvs_height_gen, gen->ndepth == D) */
int smvs_softmax_regress_fwd_gen(const float* reg, const smvs_height_gen* gen,
                                 float* out_depth, float* out_conf, int B, int D, int H, int W, void* stream);
int smvs_window_regress_fwd_gen(const float* reg, const smvs_height_gen* gen,
                                float* out_depth, float* out_conf, float* out_var, float lamb,
                                int B, int D, int H, int W, void* stream);
/* Pred path, one plane d: prob = exp(double(reg)); max_prob = max(.,prob); depth_img += h*prob;
 * exp_sum += prob (networks/casred.py:218-231).  Accumulators (B,H,W) float64, zeroed by the
 * caller before plane 0.  reg_plane (B,H,W). */
int smvs_stream_regress_step(const float* reg_plane, const float* depth, int depth_is_4d,
                             double* exp_sum, double* depth_img, double* max_prob,
                             int B, int D, int H, int W, int d, void* stream);
/* depth = depth_img/(exp_sum+1e-10), conf = max_prob/(exp_sum+1e-10) -> float32
 * (networks/casred.py:234-236).  n = B*H*W. */
int smvs_stream_regress_final(const double* exp_sum, const double* depth_img, const double* max_prob,
                              float* out_depth, float* out_conf, size_t n, void* stream);
/* Reduce step of the plane-sharded regression's exchange (satmvs_amd/shard.py; north_star's "RCCL all-reduce of the per-plane
 * cost slab", networks/casred.py:176-236 sharded over height planes): recv holds `world` copies [rank][chunk] (one per rank, in
 * rank order) of `chunk` consecutive elements, starting at element `first`, of the flattened (3,B,H,W) float64 accumulators
 * [exp_sum | depth_img | max_prob] (row_len = B*H*W); out[i] = sum over ranks for elements of the first two rows, max for the
 * third, folded in rank order.  out may be the slab position the following all-gather sends from. */
int smvs_regress_fold(const double* recv, double* out, int world, size_t chunk, size_t first, size_t row_len, void* stream);

/* ---- recurrent encoder-decoder regulariser (RED), one height plane per call ----------------------
 * Replaces slice_RED_Regularization.forward (modules/module.py:672-693) and the loop body of
 * RED_Regularization.forward (:625-644) incl. ConvGRUCell2 (:6-58).  Hidden sizes 8/16/32/64 as in
 * the reference (:617-620); C = input (feature) channels.
 *
 * smvs_red_pack_weights: params = HOST array of 48 device pointers, the module's parameters in this
 * order -- for conv_gru1..4: gate_conv.weight, gate_conv.bias, reset_gate_norm.weight, .bias,
 * update_gate_norm.weight, .bias, output_conv.weight, .bias, output_norm.weight, .bias; then
 * conv1.conv.weight, conv2.conv.weight, conv3.conv.weight, upconv1.conv.weight, upconv2.conv.weight,
 * upconv3.conv.weight, upconv2d.weight, upconv2d.bias.  packed: smvs_red_packed_floats(C) floats,
 * owned by the caller; repack whenever the parameters change.
 * smvs_red_step_fwd: cost (B,C,H,W) = the variance plane (the network consumes -cost); state1..4
 * (B,8,H,W) (B,16,H/2,W/2) (B,32,H/4,W/4) (B,64,H/8,W/8) updated in place; reg_out (B,1,H,W);
 * workspace of smvs_red_workspace_bytes(B,C,H,W) bytes; H, W multiples of 8. */
size_t smvs_red_packed_floats(int C);
size_t smvs_red_workspace_bytes(int B, int C, int H, int W);
int smvs_red_pack_weights(const float* const* params, int C, float* packed, void* stream);
int smvs_red_step_fwd(const float* packed, const float* cost, float* state1, float* state2, float* state3,
                      float* state4, float* reg_out, void* workspace, size_t workspace_bytes,
                      int B, int C, int H, int W, void* stream);

/* The plane loop of compute_depth_when_pred (networks/casred.py:191-231) for planes [d_begin,d_end) in
 * one call: per plane  fused warp+variance of that plane -> RED step -> float64 streaming regression,
 * enqueued back to back.  acc (3,B,H,W) float64 = [exp_sum, depth_img, max_prob] (zeroed by the caller
 * before plane 0; finish with smvs_stream_regress_final, or all-reduce it first when planes are sharded
 * over GPUs).  geo: rpc (B,V,170) for geo_kind 0, composed homographies (B,n_src,4,4) for geo_kind 1.
 * workspace: smvs_red_pred_workspace_bytes(B,C,H,W) bytes. */
size_t smvs_red_pred_workspace_bytes(int B, int C, int H, int W);
int smvs_red_pred_planes(int geo_kind, const float* ref_fea, const float* const* src_fea, int n_src,
                         const double* geo, const float* depth, int depth_is_4d, const float* packed,
                         float* state1, float* state2, float* state3, float* state4, double* acc,
                         void* workspace, size_t workspace_bytes,
                         int B, int C, int D, int H, int W, int d_begin, int d_end, void* stream);

/* Same plane pipeline with the regularised planes written to reg_volume (B,D,H,W) instead of the regression
 * accumulators: the whole-volume network's path (compute_depth_when_train under no_grad: networks/casred.py:22-62
 * with RED_Regularization.forward, modules/module.py:625-647) without materialising the (B,C,D,H,W) variance
 * volume; follow with smvs_softmax_regress_fwd. */
int smvs_red_volume_planes(int geo_kind, const float* ref_fea, const float* const* src_fea, int n_src,
                           const double* geo, const float* depth, int depth_is_4d, const float* packed,
                           float* state1, float* state2, float* state3, float* state4, float* reg_volume,
                           void* workspace, size_t workspace_bytes,
                           int B, int C, int D, int H, int W, int d_begin, int d_end, void* stream);
/* Both plane pipelines with the heights generated in the kernels (smvs_height_gen, gen->ndepth == D). */
int smvs_red_pred_planes_gen(int geo_kind, const float* ref_fea, const float* const* src_fea, int n_src,
                             const double* geo, const smvs_height_gen* gen, const float* packed,
                             float* state1, float* state2, float* state3, float* state4, double* acc,
                             void* workspace, size_t workspace_bytes,
                             int B, int C, int D, int H, int W, int d_begin, int d_end, void* stream);
int smvs_red_volume_planes_gen(int geo_kind, const float* ref_fea, const float* const* src_fea, int n_src,
                               const double* geo, const smvs_height_gen* gen, const float* packed,
                               float* state1, float* state2, float* state3, float* state4, float* reg_volume,
                               void* workspace, size_t workspace_bytes,
                               int B, int C, int D, int H, int W, int d_begin, int d_end, void* stream);

/* ---- 3-D convolutional cost regulariser (CostRegNet), inference form ---------------------------------
 * Replaces CostRegNet.forward (modules/module.py:546-577; Conv3d :324, Deconv3d :369) for
 * CascadeMVSNet (networks/casmvs.py) and UCSNet (networks/ucs.py); base_channels = 8.  BatchNorm3d uses
 * its running statistics (eval mode), folded into a per-channel scale/shift.
 * smvs_costreg_pack_weights: params = HOST array of 51 device pointers -- for conv0, conv1, conv2, conv3,
 * conv4, conv5, conv6, conv7, conv9, conv11: conv.weight, bn.weight, bn.bias, bn.running_mean,
 * bn.running_var; then prob.weight.  packed: smvs_costreg_packed_floats(C) floats owned by the caller.
 * smvs_costreg_fwd: vol (B,C,D,H,W) variance volume -> out (B,1,D,H,W); D, H, W multiples of 8;
 * workspace of smvs_costreg_workspace_bytes bytes. */
size_t smvs_costreg_packed_floats(int C);
size_t smvs_costreg_workspace_bytes(int B, int C, int D, int H, int W);
int smvs_costreg_pack_weights(const float* const* params, int C, float* packed, void* stream);
int smvs_costreg_fwd(const float* packed, const float* vol, float* out, void* workspace, size_t workspace_bytes,
                     int B, int C, int D, int H, int W, void* stream);

/* ---- feature extractor (FeatureNet), inference form ---------------------------------------------------
 * Replaces FeatureNet.forward (modules/module.py:442-543; num_stage 3; Conv2d :19-60, Deconv2d :62-114,
 * DeConv2dFuse :117-140) applied to every view (networks/casred.py:116-121): all views of all samples in one
 * call (N = B*V images).  arch 0 = arch_mode "unet" (casred, ucs), arch 1 = arch_mode "fpn" (casmvs: 1x1
 * laterals added to the nearest-upsampled coarser level, module.py:527-536).  BatchNorm2d uses its running
 * statistics, folded into a per-channel scale/shift.
 * smvs_featnet_pack_weights: params = HOST array of device pointers.  Both variants: for conv0.0, conv0.1,
 * conv1.0, conv1.1, conv1.2, conv2.0, conv2.1, conv2.2: conv.weight, bn.weight, bn.bias, bn.running_mean,
 * bn.running_var (40).  arch 0 continues with the same five for deconv1.deconv, deconv1.conv, deconv2.deconv,
 * deconv2.conv, then out1.weight, out2.weight, out3.weight (63 in all); arch 1 with out1.weight,
 * inner1.weight, inner1.bias, out2.weight, inner2.weight, inner2.bias, out3.weight (47 in all).
 * packed: smvs_featnet_packed_floats(base_channels, arch) floats owned by the caller.
 * smvs_featnet_fwd: imgs (N,3,H,W) -> stage1 (N,4c,H/4,W/4), stage2 (N,2c,H/2,W/2), stage3 (N,c,H,W);
 * H, W multiples of 4; workspace of smvs_featnet_workspace_bytes bytes. */
size_t smvs_featnet_packed_floats(int base_channels, int arch);
size_t smvs_featnet_workspace_bytes(int N, int H, int W, int base_channels, int arch);
int smvs_featnet_pack_weights(const float* const* params, int base_channels, int arch, float* packed, void* stream);
int smvs_featnet_fwd(const float* packed, const float* imgs, float* stage1, float* stage2, float* stage3,
                     void* workspace, size_t workspace_bytes, int N, int H, int W, int base_channels, int arch,
                     void* stream);

/* ---- DSM production ------------------------------------------------------------------------
 * Per-view height maps in image space -> one height grid in map coordinates (Transverse Mercator, e.g. UTM).
 * tm7 (HOST array): ellipsoid a [m], inverse flattening, lat0 [deg], lon0 [deg], k0, false easting, false northing [m].
 * smvs_tm_project: USGS series (Snyder), float64.  dir 0: (lat, lon) [deg] -> (E, N) [m]; dir 1: (E, N) -> (lat, lon).
 *   a, b, o0, o1: n doubles each (device).
 * smvs_rpc_dsm_bin: one height map (H,W) float32 with its 170-vector; pixel (x, y) = column x, row y.  A pixel is valid where
 *   mask (uint8, nullable) is non-zero and the height is finite; (x, y, h) -> (lat, lon) by the inverse RPC (as
 *   smvs_rpc_project dir 0) -> (E, N).  grid4 (HOST array): E0, N0 = centre of cell (0, 0), xres, yres [m];
 *   col = floor((E - E0) / xres + 0.5), row = floor((N0 - N) / yres + 0.5) (IEEE quotients).  cell (H*W) int32 = row * gw + col,
 *   or -1 (invalid or off the grid); count (gw*gh) uint32 ACCUMULATED over calls (zero-filled by the caller once per DSM);
 *   east / north (H*W) float64, both or neither, NaN where the pixel is invalid.
 * smvs_dsm_reduce: cell / height = the concatenated outputs of every bin call of one DSM (n points), count = their counts.
 *   Every cell's heights are sorted on the order-preserving uint32 image of the float and reduced: mode 0 median (mean of the
 *   two middle values in float64 for even counts), 1 mean (float64 sum in an order fixed by the count), 2 min, 3 max; empty
 *   cells get nodata.  dsm (gh, gw) float32.  The result is bit-identical from run to run and under any permutation of the
 *   points.  workspace: smvs_dsm_workspace_bytes(n, gw, gh) bytes (0 = unsupported sizes).
 * smvs_rpc_dsm_render: the reverse direction, a DSM rendered into one view's image-space heights.  dsm (gh, gw) float32
 *   (device) on grid4 (HOST, as above: cell centres on integer u = (E - E0) / xres, v = (N0 - N) / yres); rpc170 (device) the
 *   view's 170-vector; height (H, W) float32 (device) = view pixels (x0 + j, y0 + i), x = column, y = row (as smvs_rpc_dsm_bin).
 *   Every step is float64.  S(E, N) = bilinear over the cells floor(u) .. floor(u)+1 x floor(v) .. floor(v)+1, as three lerps
 *   (a = z00 + du (z01 - z00), b = z10 + du (z11 - z10), S = a + dv (b - a)); DEFINED only where all four cells are on the grid,
 *   finite and != nodata, never extrapolated.  G(h) = TM_forward(rpc_photo2obj(x, y, h)); f(h) = S(G(h)) - h.
 *   [h_lo, h_hi] = min / max of the valid cells (the caller's).  D = max(|dE| / xres, |dN| / yres) between G(h_hi) and G(h_lo);
 *   K = clamp(ceil(2 D), 1, 4096) (a step moves at most half a cell; 4096 is reached only by absurd inputs; NaN D gives 1);
 *   samples h_k = h_hi - k (h_hi - h_lo) / K, k = 0 .. K - 1, and h_K = h_lo exactly (so ground at the lowest valid cell is
 *   always reached whatever the rounding of k (h_hi - h_lo) / K); the hit is the first k with f(h_k) defined and >= 0.
 *   k = 0 -> h_hi.  No hit, or f(h_{k-1}) undefined (the ray left a hole or the grid) -> invalid.  Otherwise B bisection steps
 *   on [a, b] = [h_k, h_{k-1}], B = clamp(ceil(log2(dh / tol)), 0, 60) with dh = (h_hi - h_lo) / K, computed exactly as the
 *   least B with dh 2^-B <= tol: m = 0.5 (a + b); f(m) undefined -> invalid; f(m) >= 0 -> a = m, else b = m.  The result is
 *   0.5 (a + b) of the final bracket, rounded to float32; invalid pixels are NaN.  No atomics: bit-identical from run to run,
 *   and a tile rendered with its origin equals the same crop of a whole-view render bit for bit.
 * smvs_rpc_ortho: one view's image resampled onto the DSM grid (a true orthophoto: occlusion by the DSM itself).  dsm, grid4,
 *   nodata, tm7, rpc170 as for the render; image (H, W, C) float32 channels-last (device), 1 <= C <= 16, pixel (i, j) = view
 *   column x0 + j, row y0 + i; ortho (gh, gw, C) float32, source (gh, gw) int32, state (gh, gw) uint8 or null (all device).
 *   image and ortho go together and may both be null (a visibility-only call); ortho needs source; source or state is given.
 *   Every step is float64, one lane per cell (r, c):
 *   1. E = E0 + c xres, N = N0 - r yres; z = the float32 cell.  z not finite or == nodata -> state 0 (no height).
 *   2. (lat, lon) = TM_inverse(E, N); (x, y) = rpc_obj2photo(lat, lon, z), x = sample = column, y = line = row; u = x - x0,
 *      v = y - y0.  Unless 0 <= u <= W - 1 and 0 <= v <= H - 1 (NaN fails) -> state 1 (outside the image).
 *   3. occlusion != 0 only: G(h) = TM_forward(rpc_photo2obj(x, y, h)), f(h) = S(G(h)) - h with the render's surface S.  No
 *      samples if z >= h_hi.  Else D = max(|dE| / xres, |dN| / yres) between G(z) and G(h_hi), K = clamp(ceil(2 D), 1, 4096)
 *      (NaN D gives 1), samples h_k = z + k (h_hi - z) / K, k = 1 .. K - 1, and h_K = h_hi exactly.  Some sample with f(h_k)
 *      defined and > occ_tol -> state 2 (occluded); the lane stops there.  Undefined samples (holes, off the grid) do NOT
 *      occlude (unlike the render, where leaving a hole invalidates the pixel).
 *   4. Otherwise state 3 (visible): c0 = min(floor(u), W - 2), du = u - c0 (W = 1: c0 = 0, du = 0, both taps column 0); rows
 *      alike; a = p00 + du (p01 - p00), b = p10 + du (p11 - p10), value = a + dv (b - a) from float32 taps in float64, rounded
 *      to float32 per channel.
 *   5. Mosaic rule: ortho (C values) and source (= view) are written only where the state is 3 and source < 0 on entry.
 *      Without state, cells with source >= 0 on entry skip steps 2 - 4; state, when given, is written for every cell whatever
 *      source holds.  No atomics: bit-identical from run to run.
 * Limits: n < 2^31 per reduce, gw * gh < 2^31 cells, H * W < 2^31 pixels, x0, y0 >= 0 with x0 + W and y0 + H fitting in an int,
 * positive sizes and resolutions, h_lo <= h_hi finite, tol > 0 finite; smvs_rpc_ortho: h_hi finite, occ_tol >= 0 finite,
 * view >= 0.
 *
 * Cleaning a DSM (csrc/dsm_post.hip).  dsm, out (gh, gw) float32 (device), out distinct from dsm (aliasing is rejected); both
 * operations read dsm only, so no result depends on the order in which cells are processed.  A cell is valid iff it is finite
 * and != nodata, as above.  Every output is bit-identical from run to run.
 * smvs_dsm_despike: for every valid cell, V = the valid cells of the (2 radius + 1)^2 window around it clipped at the grid
 *   border (the centre included), n = |V|.  n < min_valid -> removed.  Otherwise m = the median of V as in smvs_dsm_reduce
 *   (v[n / 2] of the sorted values, or (float)(0.5 ((double)v[n / 2 - 1] + (double)v[n / 2])) for even n) and the cell is
 *   removed iff |(double)z - (double)m| > thresh.  Removed cells are written as nodata; every other cell, valid or not, is
 *   copied bit for bit.  removed (gh, gw) uint8 or null: 1 where a cell was removed, else 0.
 *   radius 1, 2 or 3; thresh finite and >= 0; 1 <= min_valid <= (2 radius + 1)^2.
 * smvs_dsm_fill: eight directions (dcol, drow), rows running south, in this order: E (1,0), NE (1,-1), N (0,-1), NW (-1,-1),
 *   W (-1,0), SW (-1,1), S (0,1), SE (1,1).  For an invalid cell p the hit of direction d is the first cell p + k d,
 *   1 <= k <= max_steps, on the grid and valid in dsm: its float32 height z_d and k_d.  hits = the number of directions with a
 *   hit.  The cell is filled iff hits >= min_hits, otherwise copied; valid cells are copied.  The value, over the hit
 *   directions in the order above: method 0 (inverse distance) d2 = (double)k_d^2, doubled on a diagonal, w = 1.0 / d2,
 *   num = sum of w (double)z_d, den = sum of w, both from 0.0, value = (float)(num / den), IEEE float64 without contraction;
 *   method 1 (nearest) z_d of the smallest d2; method 2 (min) the lowest z_d; ties keep the earlier direction.
 *   hits (gh, gw) uint8 or null: 255 where the input cell was valid, else the number of hits.
 *   1 <= max_steps <= 4096, 1 <= min_hits <= 8; workspace: smvs_dsm_fill_workspace_bytes(gw, gh, max_steps) bytes (0 =
 *   unsupported arguments), distinct from the other buffers.
 *
 * Ground extraction (csrc/dsm_morph.hip).  dsm (gh, gw) float32 (device), read only; a cell is valid iff it is finite and
 * != nodata, as above.  Values are ordered by their keys (a float's bits, complemented if negative, else with the sign bit
 * set): the order of <, with -0.0 below +0.0, so "lowest" and "highest" name one bit pattern.
 *   Window of a cell = the (2 r + 1)^2 square around it clipped at the grid border.  A field F is a value or "none" per cell
 *   (the field of a grid: its valid cells).  erode(F, r)(p) = the lowest value of F in p's window, dilate(F, r)(p) = the
 *   highest, "none" iff the window holds no value: cells without a value are transparent, and the result is defined at every
 *   cell whose window holds one, valid in the grid or not.  open(F, r) = dilate(erode(F, r), r), close(F, r) =
 *   erode(dilate(F, r), r).  Clipped windows are symmetric (q in p's window iff p in q's), so open(F, r)(p) <= F(p) <=
 *   close(F, r)(p) wherever F has a value.
 * smvs_dsm_morph: op 0 erode, 1 dilate, 2 open, 3 close of the grid's field with radius r; out (gh, gw) float32 gets the
 *   result at valid cells (it is defined there: a valid cell is in its own window) and the input's bits at invalid cells.
 * smvs_dsm_ground: the progressive morphological filter over n_levels windows.  radii (int) and thresholds (double) are HOST
 *   arrays of n_levels entries.  S_0 = the grid's field, every valid cell classed ground.  For k = 0 .. n_levels - 1:
 *   O_k = open(S_k, radii[k]); a valid cell still classed ground with (double)S_k(p) - (double)O_k(p) > thresholds[k] is
 *   classed removed at level k; S_(k+1) = O_k at the valid cells, none elsewhere.  cls (gh, gw) uint8: 0 invalid input cell,
 *   1 ground, 2 + k removed at level k.  dtm (gh, gw) float32: the input's bits at ground and at invalid cells, nodata at
 *   removed cells.  The levels run on the stream without host synchronisation.
 * Limits (SMVS_ERR_ARG, checked before any HIP call): 1 <= radius, radii[k] <= 256, radii strictly increasing,
 *   1 <= n_levels <= 16, thresholds finite and >= 0, gw * gh < 2^31; out / dtm / cls / workspace distinct from dsm and from
 *   each other; workspace: smvs_dsm_morph_workspace_bytes(gw, gh, the largest radius) bytes (0 = unsupported arguments).
 *   No atomics, every value a selection: bit-identical from run to run and to the numpy statement of these rules.
 *
 * Objects (csrc/dsm_label.hip).  mask (gh, gw) uint8 (device), read only: non-zero cells are foreground.  Two foreground cells
 *   are adjacent iff they differ by one step E, N, W or S (connectivity 4) or by one of those or a diagonal step
 *   (connectivity 8); a component is a class of the transitive closure of adjacency.  Components are ordered by the linear
 *   index row * gw + col of their first cell in raster order.
 * smvs_dsm_label: labels (gh, gw) int32 gets 1 .. n in that order (the numbering of scipy.ndimage.label), 0 at background
 *   cells; n_out (device, one int) gets n, or -1 if a union-find loop gave up at its bound (a damaged parent array: never on
 *   a sound device; labels are undefined then).  The result depends on the mask alone: equal bits from run to run.  The
 *   labels buffer holds the parent array while the entry runs.  No host synchronisation.
 * smvs_dsm_label_stats: per label k + 1, k = 0 .. n - 1, over the cells of `labels` that carry it (cells with a label outside
 *   1 .. n contribute to nothing): area[k] int32 the number of cells; bbox[4 k ..] int32 r0, c0, r1, c1, inclusive
 *   (INT_MAX, INT_MAX, -1, -1 if the label has no cell); rc_sum[2 k ..] int64 the sums of the rows and of the columns.  With
 *   values (gh, gw) float32, a cell valid iff finite and != (float)nodata: nvalid[k] int32 the valid cells; vmin[k], vmax[k]
 *   float32 the lowest and highest valid value by the order of the keys above (-0.0 below +0.0), nodata where nvalid is 0;
 *   qsum[k] int64 the sum over the valid cells of q(v) = llrint(min(max((double)v, -2^21), 2^21) * 1024), halves to even:
 *   heights in units of 2^-10 m (0.98 mm), summed exactly, |qsum| < 2^62.  mean = qsum / 1024 / nvalid and volume =
 *   qsum / 1024 * xres * yres are the caller's, in float64.  Integer atomics only, so the bits do not depend on their order.
 *   The entry initialises its outputs; n == 0 returns SMVS_OK without a launch.  values null <=> nvalid, vmin, vmax, qsum null.
 * Limits (SMVS_ERR_ARG, checked before any HIP call): non-null pointers, gw, gh >= 1, gw * gh < 2^31, connectivity 4 or 8,
 *   n >= 0; labels, n_out and workspace distinct from mask and from each other; every statistics output distinct from labels,
 *   values and the other outputs; workspace: smvs_dsm_label_workspace_bytes(gw, gh) bytes (0 = unsupported arguments).
 *
 * Zonal order statistics (csrc/dsm_zonal.hip).  labels (gh, gw) int32 and values (gh, gw) float32 (device), read only.  A cell
 *   counts for label k + 1 iff its label is k + 1 with 0 <= k < n and its value is finite and != (float)nodata; labels need not
 *   be connected: any zone map will do.  Values are ordered by the keys of smvs_dsm_label_stats' vmin / vmax: the
 *   order-preserving uint32 image of the float32 bits, -0.0 below +0.0.  They are never converted: a result is one of the
 *   input values with its own bits.
 * smvs_dsm_label_select: with m_k the number of cells that count for label k + 1, out[k n_ranks + j] (float32) is the value
 *   whose key is the ranks[k n_ranks + j]-th smallest, 0-based, duplicates counted, among them, and (float)nodata if that rank
 *   is outside 0 .. m_k - 1.  ranks (n, n_ranks) int32 (device), 1 <= n_ranks <= 8; equal ranks in a row are allowed.
 *   nvalid[k] (int32, may be null) gets m_k.  Deviation mode: with centre non-null, (n) float32 (device), the selection runs on
 *   d = (float)fabs((double)v - (double)centre[k]) in place of v: one float64 subtraction, one fabs, one rounding to float32,
 *   not contracted.  Whether a cell counts is still decided on v (d itself is not held against nodata, and a d that rounds to
 *   +Inf is selected as such); a label whose centre is not finite has no cell that counts.
 *   The result depends on the inputs alone: equal bits from run to run, on any stream, for any grouping of ranks into calls,
 *   and with the numpy statement of this rule (integer atomics only).  The entry initialises all it writes, enqueues 66
 *   launches for every n_ranks (2 + 2 per key bit), whatever n, the grid and the data, and never reads the device back;
 *   n == 0 returns SMVS_OK without a launch.
 * Limits (SMVS_ERR_ARG, checked before any HIP call): non-null labels, values, ranks, out and workspace; gw, gh >= 1,
 *   gw * gh < 2^31; n >= 0; 1 <= n_ranks <= 8; n * n_ranks < 2^28; out, nvalid and workspace distinct from labels, values,
 *   centre and ranks and from each other; workspace: smvs_dsm_label_select_workspace_bytes(n, n_ranks) bytes (0 = unsupported
 *   arguments; never 0 for supported ones, n == 0 included).
 *
 * Focal statistics (csrc/dsm_focal.hip).  dsm (gh, gw) float32 (device), read only.  A cell is valid iff it is finite,
 *   != (float)nodata and |z| <= 32768; q = llrint((double)z * 256), halves to even: its height in units of 2^-8 m.
 * smvs_dsm_focal_build: writes one table buffer for the DSM.  It starts with a header of 8 int64 words (256 bytes), written on
 *   the device: [0] qmin and [1] qmax over the valid cells, [2] n_valid, [3] c = (qmin + qmax) >> 1, the centre heights are
 *   measured from, [4] D = max(c - qmin, qmax - c), [5 .. 7] 0; with no valid cell all of them are 0.  Behind it, each starting
 *   on a multiple of 256 bytes, lie three inclusive 2-D prefix tables over (gh + 1) x (gw + 1) entries, entry (y, x) the sum
 *   over the valid cells (r, c) with r < y and c < x, so row 0 and column 0 are zero and a query never branches at the grid's
 *   edge: N int32 the count, S1 int64 the sum of d = q - c, S2 uint64 the sum of d^2 MODULO 2^64.  A difference of wrapped
 *   prefixes is the window's sum modulo 2^64, so it is exact whenever the true sum of the window fits, however far the
 *   prefixes themselves have wrapped: that is what lets +-32768 m heights on large grids work.  The rest of the buffer is
 *   working space: the build's band totals and the rectangle list of the latest query.  All sums are integers, the only
 *   atomics are the integer min / max / add of the range: equal bits from run to run, for any launch geometry, and with the
 *   numpy statement of this rule.  Seven launches, no read of the device.
 * smvs_dsm_focal_query: rects is a HOST array of n_rects records {dx0, dx1, dy0, dy1, sign}, bounds inclusive, sign +-1; the
 *   window of a cell is the signed sum of these rectangles about it (a box is one record, a disc one per run of rows of equal
 *   half-width, an annulus a disc minus a disc).  Output cell (R, C) of the (oh, ow) result sits at input cell
 *   (r0 + R sy, c0 + C sx); every rectangle is clipped to the grid per cell, so cells outside add nothing.  Every output may
 *   be null: n int32, s1 int64, s2 (the low 64 bits) the exact integers of the window; mean and var float64 (device), in this
 *   order of IEEE operations, not contracted: mean = ((double)c + (double)S1 / (double)n) * 2^-8;
 *   V = n S2 - S1 S1 as an unsigned 128-bit integer (>= 0 by Cauchy-Schwarz), Vd = (double)(uint64)(V >> 64) * 2^64 +
 *   (double)(uint64)V, var = Vd / ((double)n * (double)n) * 2^-16, the population variance [m^2]; both NaN where
 *   n < max(min_valid, 1).  status[0] (device int32) becomes 1 iff W+ D^2 >= 2^63 in 128-bit integers, else 0, W+ the sum of the
 *   positive rectangles' unclipped areas: the sums may then have wrapped and no result is to be trusted.  The records are
 *   written into the table buffer's tail by the call, so queries on one buffer belong on one stream at a time.
 * Limits (SMVS_ERR_ARG, checked before any HIP call, nothing written): non-null dsm, tables, rects, status; gw, gh >= 1,
 *   (gw + 1) (gh + 1) < 2^31; tables: smvs_dsm_focal_table_bytes(gw, gh) bytes (0 = unsupported sizes), not overlapping dsm;
 *   1 <= n_rects <= 1024; every offset within +-4096, dx0 <= dx1, dy0 <= dy1, sign +-1; W+ <= 2^24; sx, sy, ow, oh >= 1;
 *   every output centre inside the grid; min_valid >= 0; the outputs overlap neither each other nor the tables.
 *
 * Focal order statistics (csrc/dsm_rank.hip).  dsm (gh, gw) float32 (device), read only.  Cells and order are those of the zonal
 *   order statistics: a cell is valid iff it is finite and != (float)nodata; values are ordered by the order-preserving uint32
 *   image of their bits, -0.0 below +0.0; they are never converted: a selected value is one of the input values with its own
 *   bits.  runs is a HOST array of n_runs records {dy, dx0, dx1}, bounds inclusive: the window of cell (r, c) is the SET of the
 *   cells (r + dy, c + dx), dx0 <= dx <= dx1, over all records (no signs: an annulus is two runs a row), clipped at the grid, so
 *   cells outside add nothing.  The records travel in the kernel's arguments: no workspace, no buffer tail, and calls with
 *   different windows may run on different streams at once.
 * smvs_dsm_focal_select: levels is a HOST array of n_levels pairs (num, den).  For every cell p, n = the number of valid cells
 *   of p's window, and for level j, in integers as dsm.quantile_ranks states them: h = (n - 1) num, lo_rank = h / den,
 *   hi_rank = lo_rank + (h % den > 0).  lo[j][p] and hi[j][p], float32 (n_levels, gh, gw), are the order statistics of those
 *   0-based ranks among the window's valid cells, duplicates counted; both are (float)nodata where n = 0.  n_out (int32
 *   (gh, gw)) gets n; n_out and hi may be null.  Deviation mode: with centre non-null, (gh, gw) float32 (device), the selection
 *   at p runs on d = (float)fabs((double)v - (double)centre[p]): one float64 subtraction, one fabs, one rounding, not
 *   contracted.  Validity is still decided on v (a d that rounds to +Inf is selected as such); a p whose centre is not finite
 *   has n = 0.
 * smvs_dsm_focal_count: t (gh, gw) float32 (device), a threshold per cell.  below[p] is the number of valid cells of p's window
 *   whose key is below key(t[p]), equal[p] the number whose key equals it, both int32, both -1 where t[p] is a NaN; n_out as
 *   above.  t may be dsm itself (the elevation percentile of a cell in its neighbourhood); with t a selected value it gives that
 *   value's certificate, below <= rank < below + equal.
 *   No atomics, every result a selection or a count: equal bits from run to run, on any stream, for any launch geometry, and
 *   with the numpy statement of this rule.  One launch per call over tiles of SMVS_DSM_RANK_TILE x SMVS_DSM_RANK_TILE cells;
 *   neither entry reads the device back.
 * Limits (SMVS_ERR_ARG, checked before any HIP call, nothing written): non-null dsm, runs, levels, lo (select); dsm, runs, t,
 *   below, equal (count); gw, gh >= 1, gw * gh < 2^31; 1 <= n_runs <= 130; every offset within +-32; dx0 <= dx1; runs sorted by
 *   (dy, dx0), the runs of one row disjoint and not touching; 1 <= n_levels <= 4; 0 <= num <= den, 1 <= den <= 2^16; the
 *   outputs distinct from the inputs and from each other.
 *
 * Registration (csrc/dsm_coreg.hip).  A cell is valid iff it is finite and != (float)nodata, as above.
 * smvs_dsm_shift_stats: a (gha, gwa), the moving grid, and b (ghb, gwb), the fixed one, float32 (device), read only, of equal
 *   cell sizes (the caller's business).  For every shift (sx, sy) in [-radius, radius]^2, cell (r, c) of b is paired with cell
 *   (r + oy + sy, c + ox + sx) of a; a partner off a's grid is no pair.  d = ((double)a - (double)b) - dz0, two IEEE float64
 *   subtractions in this order, not contracted.  The pair counts iff both cells are valid and |d| <= trim (inclusive).
 *   q = llrint(d * 256), halves to even: the difference in units of 2^-8 m (3.9 mm).  stats (device, int64, (2 radius + 1)^2
 *   x 3): stats[((sy + radius) (2 radius + 1) + (sx + radius)) 3 + {0, 1, 2}] = n, the sum of q, the sum of q^2 over the
 *   counted pairs.  trim <= 256 gives |q| <= 2^16, so the sum of q^2 stays below 2^63 for any grid accepted.  Integer sums:
 *   the bits do not depend on the order of the additions, are equal from run to run and equal the numpy statement of these
 *   rules.  The entry writes every element of stats (no atomics: per-workgroup partial sums in the workspace, folded by a
 *   second kernel in a fixed order).  No host synchronisation.
 *   Limits (SMVS_ERR_ARG, checked before any HIP call): non-null pointers; sizes >= 1, gwa * gha and gwb * ghb < 2^31;
 *   0 <= radius <= 32; |ox|, |oy| < 2^30; dz0 finite; 0 < trim <= 256; stats and workspace distinct from a, b and each
 *   other; workspace: smvs_dsm_shift_workspace_bytes(gwa, gha, gwb, ghb, radius) bytes (0 = unsupported arguments).
 * smvs_dsm_regrid: src (ghs, gws) float32 (device) on the grid grid4_src = (e0, n0, xres, yres) (HOST doubles, the centre of
 *   cell (0, 0) and the cell sizes, as in smvs_rpc_dsm_render) resampled onto the (ghd, gwd) grid grid4_dst.  For the
 *   destination cell (r, c): E = e0d + c xresd, N = n0d - r yresd, u = (E - e0s) / xress, v = (n0s - N) / yress, IEEE
 *   float64, not contracted (the cell rule of smvs_rpc_dsm_bin).  A tap is a source cell; a tap off the grid or invalid
 *   makes the cell nodata.
 *   mode 0 (nearest): the one tap (floor(v + 0.5), floor(u + 0.5)).
 *   mode 1 (bilinear): i = floor(u), j = floor(v), fx = u - i, fy = v - j; column i has the weight 1 - fx, column i + 1 fx,
 *   row j 1 - fy, row j + 1 fy; a tap whose column or row weight is exactly 0 is NOT read (so a regrid onto an
 *   integer-aligned grid is a crop) and stands as 0.0 in the value (float)((1 - fy) ((1 - fx) z00 + fx z01) + fy ((1 - fx) z10
 *   + fx z11) + dz), float64 operations in this order, z00 = (j, i), z01 = (j, i + 1), z10 = (j + 1, i), z11 = (j + 1, i + 1).
 *   A cell that takes one tap with the weight 1 (always in mode 0) gets (float)((double)z + dz), and with dz == 0 the tap's
 *   bits.
 *   Limits (SMVS_ERR_ARG, checked before any HIP call): non-null pointers; sizes >= 1, gws * ghs and gwd * ghd < 2^31;
 *   finite origins, finite resolutions > 0; mode 0 or 1; dz finite; out distinct from src.
 *
 * Mosaic (csrc/dsm_mosaic.hip).
 * smvs_dsm_dist: the exact squared Euclidean distance transform.  mask (gh, gw) uint8 (device), read only: non-zero cells are
 *   foreground, any non-zero byte.  The background set B holds the zero cells and, with border = 1, every cell off the grid
 *   (the whole plane outside).  d2 (gh, gw) int32: d2[r][c] = min(cap^2, min over (r', c') in B of (r - r')^2 + (c - c')^2),
 *   cap = max_dist; an empty B gives cap^2 everywhere; a value of cap^2 means "at least cap".  These are the squares of
 *   scipy.ndimage.distance_transform_edt(mask), capped; with border = 1 the same on the mask padded by one ring of zeros,
 *   cropped back.  Integers only, every value a minimum: equal bits from run to run and to the numpy statement of this rule.
 *   The entry writes every element of d2 and of the part of the workspace it reads (a workspace full of anything will do);
 *   no atomics, no host synchronisation.  The cap is part of the contract: it bounds every halo.
 *   Limits (SMVS_ERR_ARG, checked before any HIP call): non-null pointers; gw, gh >= 1, gw * gh < 2^31; border 0 or 1;
 *   1 <= max_dist <= 1024; d2 and workspace distinct from mask and from each other; workspace:
 *   smvs_dsm_dist_workspace_bytes(gw, gh, max_dist) bytes (0 = unsupported arguments).
 * smvs_dsm_mosaic: n_layers layers (a HOST array of smvs_dsm_layer; z (gh, gw) float32 and d2 (gh, gw) int32 on the device,
 *   read only) combined into the (gh, gw) destination.  Layer k's cell (r, c) lies on destination cell (r + oy_k, c + ox_k);
 *   what falls off the destination is ignored, and a layer that misses it altogether contributes nothing.  A layer cell is
 *   valid iff it is finite and != (float)nodata, as above.  For a destination cell V is the list of the layers valid there, in
 *   ascending k, m = |V|.  out (gh, gw) float32 gets (float)nodata where V is empty, else by mode:
 *   0 first: the bits of the first of V.  1 last: the bits of the last of V.
 *   2 min / 3 max: the bits of the lowest / highest of V by the order of the keys above (-0.0 below +0.0); ties keep the
 *     earlier layer.
 *   4 mean: (float)(S / m), S the float64 sum of (double)z over V in ascending k, STARTED FROM THE FIRST TERM (not from 0.0).
 *   5 feather: (float)(S / W), S = sum of w_k (double)z_k, W = sum of w_k over V in ascending k, both started from their
 *     first terms, w_k = sqrt((double)min(max(d2_k, 1), feather^2)): the weight ramps up over `feather` cells from the tile's
 *     edge and voids when d2 is smvs_dsm_dist of the layer's validity mask with border = 1, and a wrong d2 can never give a
 *     zero or NaN weight.
 *   The float64 operations are IEEE, each product, sum, square root and quotient rounded by itself to nearest, nothing
 *   contracted.  Starting from the first term makes a mosaic of one layer that layer's bits in every mode (-0.0 included:
 *   w z / w is within a float64 rounding or two of z, far inside half a float32 ulp).
 *   Optional outputs (each may be null; the entry writes every element): count (gh, gw) uint8 = m; source (gh, gw) uint8 =
 *   the layer taken in modes 0 .. 3, the layer with the largest weight in modes 4 and 5 (ties to the earlier layer; in mode 4
 *   the first of V), 255 where V is empty; spread (gh, gw) float32 = (float)((double)hi - (double)lo), hi and lo the highest
 *   and lowest of V, 0 for one layer, (float)nodata where V is empty.
 *   One launch, one lane per destination cell, the layer table in the kernel arguments; no workspace, atomics or state.
 *   Limits (SMVS_ERR_ARG, checked before any HIP call): non-null layers, out and every z; 1 <= n_layers <= 64; every size
 *   >= 1 and below 2^31 cells; |ox|, |oy| < 2^30; mode 0 .. 5; in mode 5 1 <= feather <= 1024 and every d2 non-null (feather
 *   and d2 are ignored otherwise); out, count, source and spread distinct from each other and from every layer buffer.
 *
 * Stack fusion (csrc/dsm_stack.hip): order statistics along the layer axis.  Layers are smvs_dsm_layer records exactly as
 *   smvs_dsm_mosaic takes them: a HOST array of 1 .. 64 layers, z on the device and read only, d2 ignored (it may be null);
 *   layer k's cell (r, c) lies on destination cell (r + oy_k, c + ox_k), |ox|, |oy| < 2^30, and what falls off the destination
 *   is ignored.  A layer cell is valid iff it is finite and != (float)nodata.  For a destination cell V is the list of the
 *   layers valid there in ascending k, m = |V|.  Order is that of the keys of the zonal and focal order statistics (-0.0 below
 *   +0.0), duplicates count, and a selected value is one of the input values with its own bits.
 * smvs_dsm_stack_select: levels is a HOST array of n_levels pairs (num, den).  For level j, in integers as dsm.quantile_ranks
 *   states them: h = (m - 1) num, lo_rank = h / den, hi_rank = lo_rank + (h % den > 0).  lo[j] and hi[j], float32 (n_levels,
 *   gh, gw), are the values of those 0-based ranks among V, (float)nodata where m = 0.  count (uint8 (gh, gw)) gets m; count
 *   and hi may be null.  Deviation mode: with centre non-null, (gh, gw) float32 (device), the selection at cell p runs on
 *   d = (float)fabs((double)z - (double)centre[p]): one float64 subtraction, one fabs, one rounding, not contracted.  Validity
 *   is still decided on z (a d that rounds to +Inf is selected as such); a p whose centre is not finite has m = 0.  This is
 *   smvs_dsm_focal_select's deviation rule.
 * smvs_dsm_stack_fuse: the robust fusion of the stack, in this operation order.  With a and b the order statistics (m - 1) / 2
 *   and (m - 1) / 2 + rem of V, rem = (m - 1) % 2: M64 = a + (b - a) (rem / 2) in float64, each operation rounded by itself
 *   (the "linear" quantile at 1/2); med32 = (float)M64.  d_k = (float)fabs((double)z_k - (double)med32) for k in V; D64 is the
 *   same linear median over the d_k, mad32 = (float)D64 (a NaN where both middle deviations are +Inf).  thr = fmax(kmad
 *   (double)mad32, floor): a NaN product loses, as in C fmax.  Layer k of V is an inlier iff (double)d_k <= thr; n_in counts
 *   them.  S is the float64 sum of (double)z_k over the inliers in ascending k, STARTED FROM ITS FIRST TERM; out = (float)(S /
 *   n_in), and med32 if n_in = 0 (even m, two different middle values and a small threshold).  One layer alone therefore comes
 *   back bit for bit in out.  out, median = med32 and mad = mad32 are float32 (gh, gw); count = m and n_in are uint8; members
 *   and inliers are int64 with bit k set for "layer k is valid here" and "layer k is an inlier here".  Where m < max(min_count,
 *   1): out, median and mad get (float)nodata, n_in, members and inliers 0, count still m.  Every output but out may be null;
 *   the entry writes every element of those given.
 *   Both entries: one launch, one lane per destination cell, the layer table in the kernel arguments, the lane's sorted keys in
 *   n_layers KiB of LDS per workgroup; no workspace, atomics, state or host read-back, any stream; selections and sums in a
 *   fixed order: equal bits from run to run and with the numpy statement of this rule.
 *   Limits (SMVS_ERR_ARG, checked before any HIP call, nothing written): non-null layers, every z, levels and lo (select), out
 *   (fuse); 1 <= n_layers <= 64; 1 <= n_levels <= 8, 0 <= num <= den, 1 <= den <= 2^16; kmad and floor finite and >= 0;
 *   0 <= min_count <= 64; every size >= 1 and below 2^31 cells; |ox|, |oy| < 2^30; the outputs distinct from each other, from
 *   centre and from every layer's z.
 *
 * Sun (csrc/dsm_sun.hip).
 * smvs_dsm_shadow: cast shadows as an exclusive running maximum along lines of cells that run towards the sun.  dsm (gh, gw)
 *   float32 (device), read only; a cell is valid iff it is finite and != (float)nodata, as above.  (ucol, urow) is the
 *   horizontal direction TOWARDS the sun in cell-index units (columns run east, rows south), finite, not both 0.  There is
 *   no trigonometry in the library: the caller derives ucol, urow, a and b (dsm.sun_terms: a = tan(elevation) xres sin(az),
 *   b = -tan(elevation) yres cos(az), so that a c + b r is tan(elevation) times the distance along the sun's direction).
 *   Lines.  If |urow| >= |ucol| (a tie included) the grid is row-major: m = ucol / urow (one IEEE division, |m| <= 1),
 *   s(r) = floor(m (double)r + 0.5) (a product, then a sum, then a floor, not contracted), the line of cell (r, c) is
 *   L = c - s(r), so a row holds at most one cell of a line, and sunward order is ascending r if urow < 0, descending r if
 *   urow > 0.  Otherwise it is column-major: m = urow / ucol, s(c) = floor(m (double)c + 0.5), L = r - s(c), ascending c if
 *   ucol < 0, descending c if ucol > 0.
 *   Key.  g(r, c) = (double)z - (a (double)c + b (double)r): two products, their sum, then the difference, each rounded by
 *   itself.
 *   Result.  For a valid cell G is the maximum of g over the VALID cells of its line that come before it in sunward order
 *   (an exclusive scan; -inf if there are none; of two zeros +0.0 is the greater, the keys' order above), and d = G - g,
 *   one float64 subtraction.  shade (gh, gw) uint8: 0 at an invalid cell, 2 if d > tol, else 1.  depth, if non-null,
 *   (gh, gw) float32: (float)d at valid cells (-inf where nothing lies sunward), (float)nodata at invalid cells.  Invalid
 *   cells neither occlude nor receive.  A maximum does not depend on the order of its operands, so the bits are equal from
 *   run to run, for any decomposition of the scan, and equal to the numpy statement of this rule.
 *   A line follows the true ray to within less than one cell across it (s(i) - m i lies in (-1/2, 1/2] at both cells);
 *   the distance along the ray is exact.
 *   The entry writes every element of its outputs and of the part of the workspace it reads; no atomics, no host
 *   synchronisation.  The workspace size depends on (gw, gh) alone and covers every direction.
 *   Limits (SMVS_ERR_ARG, checked before any HIP call): non-null dsm, shade and workspace; gw, gh >= 1, gw * gh < 2^31;
 *   finite ucol, urow, not both 0; a, b finite and at most 2^900 in size (so that every g is finite); tol finite and >= 0;
 *   shade, depth and workspace distinct from dsm and from each other; workspace: smvs_dsm_shadow_workspace_bytes(gw, gh)
 *   bytes (0 = unsupported sizes).
 * smvs_dsm_gradient: Horn's 3 x 3 gradient.  A neighbour that is off the grid or invalid takes the centre's value.  For a
 *   valid cell, with z as doubles:
 *   dzde = (float)((((z[r-1,c+1] + 2 z[r,c+1]) + z[r+1,c+1]) - ((z[r-1,c-1] + 2 z[r,c-1]) + z[r+1,c-1])) / (8 xres))
 *   dzdn = (float)((((z[r-1,c-1] + 2 z[r-1,c]) + z[r-1,c+1]) - ((z[r+1,c-1] + 2 z[r+1,c]) + z[r+1,c+1])) / (8 yres))
 *   in this order, every operation rounded by itself (8 xres and 8 yres are one product each); invalid cells get
 *   (float)nodata in both outputs.  One lane per cell; bit-identical to its numpy statement.
 *   Limits (SMVS_ERR_ARG, checked before any HIP call): non-null pointers; gw, gh >= 1, gw * gh < 2^31; finite
 *   resolutions > 0; dzde and dzdn distinct from dsm and from each other.
 *
 * Horizon (csrc/dsm_horizon.hip).
 * smvs_dsm_horizon: for n_dirs azimuths in one call, the tangent of the elevation angle of the highest thing that stands
 *   towards the azimuth, for every cell.  dsm (gh, gw) float32 (device), read only.
 *   Validity and heights.  A cell is valid iff it is finite, != (float)nodata and |z| <= 32768.  q = llrint((double)z 256),
 *   halves to even: the height in units of 2^-8 m, as in the registration.
 *   Directions.  dirs is a HOST array of n_dirs x 4 doubles (ucol, urow, a, b).  (ucol, urow) is the horizontal direction
 *   TOWARDS the azimuth in cell-index units (columns run east, rows south), exactly as for smvs_dsm_shadow; (a, b) =
 *   (256 xres sin A, -256 yres cos A).  There is no trigonometry in the library: dsm.horizon_terms derives the four doubles.
 *   Lines.  The orientation, s(i) = floor(m i + 0.5), the line L of a cell and the order "towards the azimuth" are those of
 *   smvs_dsm_shadow with "sun" read as "azimuth": row-major iff |urow| >= |ucol| (a tie included), m = ucol / urow,
 *   L = c - s(r), ascending r if urow < 0, descending r if urow > 0; otherwise column-major, m = urow / ucol, L = r - s(c),
 *   ascending c if ucol < 0, descending c if ucol > 0.  A cell's predecessors are the cells of its line that come before it
 *   in that order: they lie towards the azimuth.
 *   Positions.  P(r, c) = llrint(a (double)c + b (double)r), halves to even: two products and their sum, each rounded by
 *   itself, then the rint.  P is the position along the azimuth in units of 2^-8 m.
 *   The tangent.  For a valid cell i, T(i) is the maximum over the VALID predecessors j of the exact rational
 *   (q_j - q_i) / (P_j - P_i), whose denominator is positive, and tan_h = (float)((double)(q_j - q_i) / (double)(P_j - P_i))
 *   for a j that attains it: one IEEE float64 division, then one conversion.  Equal rationals give equal bits, so the
 *   choice among tied j does not matter.  With no valid predecessor tan_h = -inf; at an invalid cell tan_h = the quiet NaN
 *   0x7fc00000.  Invalid cells neither occlude nor receive.  tan_h is (n_dirs, gh, gw) float32 (device), in the order of dirs.
 *   Exactness.  The maximum is the tangent from i to the upper convex hull of its predecessors, kept as a stack along the
 *   line: pop the top while the slope from i to the element under it is >= the slope from i to the top, read T off the
 *   top, push i.  Every comparison that prunes a candidate is an exact int64 cross-multiplication, (q1 - q_i)(P2 - P_i)
 *   against (q2 - q_i)(P1 - P_i), never a comparison of rounded quotients, and the limits below keep every product below
 *   2^62: the result equals the O(n^2) maximum over all pairs.  The bits are equal from run to run, on any stream, for any
 *   batching of the directions, and equal to the numpy statement of this rule.  The reach is unbounded.
 *   The entry writes every element of tan_h; every workspace word a kernel reads was written by a kernel of the same call
 *   (a workspace full of anything will do); no atomics, no host synchronisation.
 *   Limits (SMVS_ERR_ARG, checked before any HIP call): non-null dsm, dirs, tan_h and workspace; gw, gh >= 1,
 *   gw * gh < 2^31; 1 <= n_dirs <= 64; every direction finite; (ucol, urow) not (0, 0); a ucol >= 0 and b urow >= 0; the
 *   term along the scan, |b| if row-major else |a|, >= 4 (this keeps the rounded P strictly monotone along a line: cells
 *   of at least 1/64 m); |a| gw + |b| gh < 2^37 (with |q_j - q_i| <= 2^24 this bounds the products); dsm, tan_h and
 *   workspace do not overlap; workspace: smvs_dsm_horizon_workspace_bytes(gw, gh, n_dirs) bytes (0 = unsupported
 *   arguments): 8 bytes per cell and 8 more per cell and direction, because all directions of a call are in flight at once;
 *   a caller short of memory passes fewer directions per call, the bits do not depend on it.
 *
 * Viewshed (csrc/dsm_viewshed.hip).
 * smvs_dsm_viewshed: for n_obs observers in one call, which cells an eye on or above the surface sees: one exact line of
 *   sight per observer and target cell.  dsm (gh, gw) float32 (device), read only.
 *   Heights.  A cell is valid iff it is finite, != (float)nodata and |z| <= 32768.  q = llrint(256 (double)z), halves to
 *   even, as for smvs_dsm_horizon.
 *   Curvature.  The cell at offset (dc, dr) from the observer has the drop D = llrint(c256 (((double)dc xres) ((double)dc
 *   xres) + ((double)dr yres) ((double)dr yres))): every product and the sum rounded by themselves, nothing contracted.
 *   c256 is a HOST double >= 0 that the caller derives (dsm.viewshed_terms: c256 = 256 (1 - refraction) / (2 R)); 0 means a
 *   flat earth.  The effective height q' = q - D is used for intermediate cells and for the target alike; D is 0 at the
 *   observer.  The same sum of squares d2 serves the range test: a cell is in range iff d2 <= r2max, a HOST double, +inf
 *   for no limit.
 *   Observer.  obs is a HOST array of n_obs x 5 int32 (col, row, eye, mode, tgt).  mode 0: the eye is E = q_o + eye, in
 *   units of 2^-8 m above the observer's own cell; eye is not negative and the cell must be valid.  mode 1: E = eye is
 *   absolute and the cell may be invalid.  tgt >= 0 is the height added to every target.  The observer's cell lies on the
 *   grid.
 *   The line.  For a target (ct, rt): dx = ct - col, dy = rt - row, n = max(|dx|, |dy|).  The line steps along rows iff
 *   |dy| >= |dx|, a tie included, as the sheared lines of smvs_dsm_shadow; otherwise along columns.  At step i = 1 .. n - 1
 *   the major coordinate has moved i cells towards the target and, with dm the signed minor difference, the minor
 *   coordinate has moved floor((2 i dm + n) / (2 n)): floor division of integers, halves towards +inf.  The cell found this
 *   way is intermediate sample j.  Neither the observer's cell nor the target occludes; invalid samples neither occlude nor
 *   receive, as in smvs_dsm_horizon.
 *   The test.  M is the maximum over the valid intermediate samples of the exact rational (q'_j - E) n / i_j, -inf with no
 *   valid sample; need = ceil(M) - (q'_t - E), an integer (-inf with M).  The target is seen iff need <= tgt, which is
 *   (q'_j - E) n <= (q'_t + tgt - E) i_j for every j: grazing counts as seen.  Every comparison that decides M is an int64
 *   cross-multiplication, never a comparison of rounded quotients; under the limits below |q' - E| < 2^31 and n, i < 2^16,
 *   so every product stays below 2^47.
 *   Outputs (device).  seen (n_obs, gh, gw) uint8 and above (n_obs, gh, gw) float32 (may be null): 0 and (float)nodata at
 *   an invalid target; 1 and +0.0 at a seen one; 2 and (float)((double)need / 256.0), what must stand on the cell to be
 *   seen (one exact division, one conversion), at a hidden one; 3 and (float)nodata at a valid one out of range.  The
 *   observer's own cell (n = 0) is 1 if valid.  status (n_obs) int32: 0 for a mode-0 observer on an invalid cell, whose maps
 *   are 0 and (float)nodata everywhere; otherwise 1.
 *   The entry writes every element of its outputs; every workspace word a kernel reads was written by a kernel of the same
 *   call; no atomics, no host synchronisation.  The bits are equal from run to run, on any stream, for any batching of the
 *   observers, and equal to the numpy statement of this rule.
 *   Limits (SMVS_ERR_ARG with a message, checked before any HIP call; nothing is written): non-null dsm, obs, seen, status
 *   and workspace; 1 <= gw, gh <= 65536, gw * gh < 2^31; 1 <= n_obs <= 64; every observer on the grid, mode 0 or 1,
 *   |eye| <= 2^23 with eye >= 0 in mode 0, 0 <= tgt <= 2^23; xres, yres finite and > 0; c256 finite and >= 0 with
 *   c256 ((gw xres)^2 + (gh yres)^2) < 2^30, so that D fits; r2max > 0 or +inf, not NaN; no overlap among the buffers;
 *   workspace: smvs_dsm_viewshed_workspace_bytes(gw, gh, n_obs) bytes (0 = unsupported arguments): 4 bytes per cell.
 * smvs_dsm_los: the same rule, by the same device function, for a DEVICE list of n_pairs x 7 int32 (col_o, row_o, eye,
 *   mode, col_t, row_t, tgt), each pair with its own target height: seen (n_pairs) uint8, above (n_pairs) float32 (may be
 *   null).  Code 0 also covers an invalid mode-0 observer and a pair with a field out of range (a cell off the grid, a mode
 *   other than 0 and 1, eye or tgt beyond their limits): the kernel tests the fields before it reads a cell.  No workspace:
 *   q is taken straight from the floats.  Limits: those of smvs_dsm_viewshed on the grid and the four doubles; non-null
 *   dsm, pairs and seen; 1 <= n_pairs < 2^31; no overlap among the buffers.
 *
 * Outlines (csrc/dsm_outline.hip).  labels (gh, gw) int32 (device), read only.  A cell has label k iff its value is k and
 *   1 <= k <= n; every other value and every cell off the grid counts as 0.  Lattice corner (x, y), 0 <= x <= gw,
 *   0 <= y <= gh, is the upper-left corner of cell (row y, col x).  Side s of a cell with label k (s = 0 south, 1 east,
 *   2 north, 3 west) is a boundary edge of k iff the cell across it does not have label k; it is directed with its own cell on
 *   the left, north up: south side heading east, east side north, north side west, west side south.  The successor of edge
 *   (A, s) with heading h: B = A + h, C = B + one step across side s away from A; side (s + 3) % 4 of C if C has label k, else
 *   side s of B if B has label k, else side (s + 1) % 4 of A (right first: cells of one label that meet at a corner are
 *   joined).  The successor is a permutation of the boundary edges and its cycles are the rings.  A ring's vertices are the
 *   tail corners of those of its edges whose predecessor has another side; the list starts at the ring's smallest corner by
 *   (y, x), which it passes once, and follows the ring: an exterior ring leaves it heading south (counter-clockwise north up),
 *   a hole heading east (clockwise).  Rings are ordered by (label, start y, start x).
 * smvs_dsm_outline_count: counts (device, 3 ints) gets n_edges, n_rings, n_vertices, or -1, -1, -1 if the labels hold more
 *   than max_edges boundary edges or an index read back from the workspace was out of range (a damaged workspace: never on a
 *   sound device).  max_edges == 0 counts the edges only (n_edges, 0, 0) in a workspace of
 *   smvs_dsm_outline_workspace_bytes(gw, gh, 0) bytes; the caller reads n_edges and calls again with max_edges = n_edges and a
 *   workspace of that size, which then holds the rings.  n == 0 clears counts without a launch.  The doubling runs
 *   ceil(log2(max_edges)) rounds whatever the workspace holds.  No host synchronisation.
 * smvs_dsm_outline_write: with the three counts read from the device and the workspace as the second count call left it:
 *   ring_label[r] int32; area2[r] int64 the shoelace sum north up in cells (> 0 exterior, < 0 hole); edges[2 r ..] int32 the
 *   unit edges heading E or W and those heading N or S; offset[r] int32, n_rings + 1 entries, into vertices; first_ring[k]
 *   int32, n + 1 entries, the first ring of label k + 1 (a label without a cell has none: first_ring[k] == first_ring[k + 1]);
 *   vertices[2 v ..] int32 x, y.  offset[n_rings] is n_vertices, or -1 if the counts differ from the workspace's or an index
 *   was out of range.  All three counts 0: first_ring and offset[0] are cleared without a launch.  Integer atomics (add)
 *   only: everything depends on labels and n alone, equal bits from run to run.
 * smvs_dsm_burn: out (gh, gw) int32 is zeroed; every vertical edge (x, y0) - (x, y1) between consecutive vertices of a ring
 *   (the last to the first) XORs ring_label[r] into out[row, max(x, 0)] for min(y0, y1) <= row < max(y0, y1), rows clipped to
 *   the grid, nothing for x >= gw; then every row takes its running XOR: the even-odd rule at cell centres.  Horizontal edges
 *   do nothing.  flag (device, one int): bit 0 an edge whose ends differ in both coordinates, bit 1 an offset table that is
 *   not 0 = offset[0] <= ... <= offset[n_rings] = n_vertices.  Integer atomics (xor) only.
 * Limits (SMVS_ERR_ARG, checked before any HIP call): non-null pointers (the ring outputs may be null when the counts are 0,
 *   the burn's inputs when n_rings or n_vertices is 0); gw, gh >= 1; gw * gh < 2^29 (outline; 4 gw gh edges fit an int32) or
 *   < 2^31 (burn); n >= 0; 0 <= max_edges <= 4 gw gh; 1 <= n_rings, n_vertices <= n_edges or all three 0; outputs and
 *   workspace distinct from the inputs and from each other; workspace: smvs_dsm_outline_workspace_bytes(gw, gh, max_edges)
 *   bytes (0 = unsupported arguments): 5 bytes per corner and 61 per edge.
 * smvs_dsm_burn_polygons: smvs_dsm_burn for edges of any direction, same arguments.  An edge (x0, y0) - (x1, y1) with
 *   D = y1 - y0 != 0 visits every row r with min(y0, y1) <= r < max(y0, y1), clipped to the grid; it crosses the row's centre
 *   line y = r + 1/2 at x_c = x0 + (x1 - x0)(2 r + 1 - 2 y0) / (2 D), and the first toggled column is c = floor(x_c + 1/2), the
 *   first cell whose centre lies strictly right of the edge: floor((2 D x0 + (x1 - x0)(2 r + 1 - 2 y0) + D) / (2 D)) as one
 *   int64 floor division, the sign of D taken out first.  ring_label[r] is XORed into out[r, max(c, 0)], nothing for c >= gw;
 *   then the running XOR of every row.  A cell centre exactly on an edge shared by two polygons is in exactly one of them.  On
 *   rings whose edges run along the lattice the result is smvs_dsm_burn's bit for bit.  Vertices may lie off the grid,
 *   |x|, |y| < 2^20 (the numerator fits an int64).  flag: bit 0 is never set, bit 1 as in smvs_dsm_burn, bit 2 a coordinate
 *   outside |x|, |y| < 2^20 (the edge is left out).  Limits as for smvs_dsm_burn.
 *
 * Simplified outlines (csrc/dsm_simplify.hip): Douglas-Peucker on closed rings in exact integers.  Rings as smvs_dsm_outline_write
 *   gives them, or any: vertices (n_vertices, 2) int32 x, y with 0 <= x, y <= 32767 (every product below stays under 2^63),
 *   offset (n_rings + 1) int32 rising from 0 to n_vertices, both on the device, read only.  tol16 = floor(16 tol), tol in
 *   cells, 0 <= tol16 <= 65535.  A ring v_0 .. v_(m-1) is the open chain v_0 .. v_m with v_m = v_0.
 *   Anchors: v_0 is kept, and v_j for the j that maximises |v_j - v_0|^2, ties to the lowest j.  A ring with m < 3 or with all
 *   vertices equal keeps every vertex.
 *   Key of vertex i in the segment (a, b), a < i < b, d = v_b - v_a, u = v_i - v_a, L = |d|^2, t = u . d:
 *   |u|^2 L if t <= 0; |v_i - v_b|^2 L if t >= L; (d x u)^2 otherwise; |u|^2 if L == 0 (a ring that touches itself): the
 *   squared distance to the segment, not to the line, times L.  All keys are below 2^62.
 *   Split: i* maximises the key, ties to the smallest |2 i - a - b| (nearest the segment's middle), then to the lower i.  The
 *   segment splits at i* (i* is kept) iff key > (tol16^2 L) >> 8, for L == 0 iff key > tol16^2 >> 8: the distance is strictly
 *   above tol16 / 16.  Otherwise every vertex strictly between a and b is dropped.  Segments are independent, so the kept set
 *   does not depend on the order; a round treats every live segment once.
 *   Fall-back: the twice-area of a ring is the shoelace sum of x1 y0 - x0 y1 over its edges (north up, as area2 of the
 *   outlines).  A ring of which fewer than 3 vertices are kept, or whose kept vertices have twice-area 0 or one of another
 *   sign than the ring as given, keeps all its vertices and has simplified[r] = 0.  n_rings and the ring order never change.
 *   Nothing else is repaired: a large tolerance can make a ring cross itself or its neighbour.
 * smvs_dsm_simplify_begin: flag (device, one int) <- bit 0 a coordinate outside 0 .. 32767, bit 1 an offset table that is not
 *   0 = offset[0] <= ... <= offset[n_rings] = n_vertices; the anchors and the first two segments of every ring in the
 *   workspace.  With a flag set the later entries stay in bounds and their results mean nothing.
 * smvs_dsm_simplify_rounds: `rounds` rounds (0 .. 4096) on the workspace as begin or an earlier call left it; status (device,
 *   2 ints) <- the number of segments that split in the call's last round, and the number of rounds run since begin up to and
 *   with the first in which none split (it stops counting there; further rounds find nothing to do).  -1, -1 if an index
 *   read back from the workspace was out of range.  The caller repeats the call until status[0] == 0; a ring of m vertices
 *   needs at most m rounds.  No host synchronisation.
 * smvs_dsm_simplify_count: n_out (device, one int) <- the number of vertices of the result, the fall-back applied, or -1.
 * smvs_dsm_simplify_write: with n_out read from the device: out_offset (n_rings + 1) int32, out_vertices (n_out, 2) int32,
 *   area2 (n_rings) int64 of the rings as written, kept (n_out) int32 the index of every output vertex in the input list,
 *   simplified (n_rings) uint8.  out_offset[n_rings] is n_out, or -1 if n_out differs from the workspace's or an index was
 *   out of range.  Without vertices the tables are cleared without a launch.
 *   Integer atomics (max, min, add) only: equal bits from run to run.
 * Limits (SMVS_ERR_ARG, checked before any HIP call): non-null pointers (vertices and the vertex outputs may be null when
 *   their counts are 0, offset, area2 and simplified when n_rings is 0); 0 <= n_rings, n_vertices < 2^31, no vertices without
 *   rings; 0 <= tol16 <= 65535; 0 <= rounds <= 4096; 0 <= n_out <= n_vertices; outputs, inputs and workspace distinct;
 *   workspace: smvs_dsm_simplify_workspace_bytes(n_rings, n_vertices) bytes (0 = unsupported arguments): 56 bytes per vertex
 *   and 29 per ring.
 *
 * Contours (csrc/dsm_contour.hip): the isolines of dsm (gh, gw) float32 (device, read only) at n_levels levels in one call.
 *   Nodes, validity, heights.  Node (r, c) is the centre of cell (r, c); its position in index units is x = c, y = r.  A node
 *   is valid iff it is finite, != (float)nodata and |z| <= 32768.  q = llrint((double)z 256), halves to even, as in the
 *   registration and the horizon.
 *   Levels.  A level is an odd integer K in units of 2^-9 m: levels sit on half quanta, so no node ever lies on a contour.
 *   Node a is ABOVE iff 2 q_a > K.  levels is a HOST array of n_levels int32, odd, strictly rising, |K| < 2^25,
 *   1 <= n_levels <= 4096; more levels go through several calls, the bits do not depend on the batching.  (dsm.contours maps
 *   a level in metres to K = 2 floor(256 level) + 1 and reports K / 512.)
 *   Lattice edges.  eid = 2 (r gw + c) + o: o = 0 the edge from node (r, c) to (r, c + 1) (c < gw - 1), o = 1 the edge from
 *   (r, c) to (r + 1, c) (r < gh - 1).
 *   Crossings.  Edge e is crossed at level K iff both ends are valid and exactly one is above; a crossing (K, e) is a
 *   candidate vertex.  With a the end the eid names and b the other, t = (double)(K - 2 q_a) / (double)(2 q_b - 2 q_a), one
 *   IEEE division of two exactly representable integers, 0 < t < 1; the vertex is (x, y) = ((double)c + t, (double)r) for
 *   o = 0 and ((double)c, (double)r + t) for o = 1: one addition.
 *   Squares.  Square (r, c), 0 <= r < gh - 1, 0 <= c < gw - 1, has the corner nodes (r, c), (r, c + 1), (r + 1, c + 1),
 *   (r + 1, c); it is live iff all four are valid.
 *   Direction.  A line runs with the higher ground on its LEFT, north up, which fixes how it passes a crossed edge: o = 0,
 *   west end above: it heads north, out of square (r, c) into (r - 1, c); o = 0, east end above: south, out of (r - 1, c) into
 *   (r, c); o = 1, north end above: east, out of (r, c - 1) into (r, c); o = 1, south end above: west, out of (r, c) into
 *   (r, c - 1).
 *   Successor.  The crossing enters square S.  If S is off the lattice or not live it has no successor.  Otherwise let H
 *   (above) and L be the ends of the entry edge, H' the corner of S next to H and L' the one next to L.  H' and L' not above:
 *   leave through edge H - H' (left).  H' above, L' not: through H' - L' (straight).  Both above: through L - L' (right).  H'
 *   not above and L' above, the saddle: through L - L' iff the q of the four corners sum to > 2 K (the mean of the corners is
 *   above, strictly), else through H - H'.  The successor is the crossing (K, exit edge), crossed by construction.  The
 *   successor is injective, so the crossings of a level fall into open chains and closed rings.
 *   Lines.  A crossing with neither predecessor nor successor is dropped, so an open chain has at least 2 vertices and a ring
 *   at least 4.  An open line starts at its crossing without a predecessor; a closed line starts at its smallest eid and is
 *   NOT repeated at the end.  Consecutive vertices lie on different edges of one square: no segment has zero length.  Lines
 *   are ordered by (level index, eid of the first vertex), a unique key.  Nothing is smoothed, simplified or joined across
 *   voids.
 * smvs_dsm_contour_count: counts (device, 3 ints) gets n_cross (all crossings, the dropped ones included), n_lines,
 *   n_vertices, or -1, -1, -1 if there are more crossings than max_cross (or than an int32 holds), or an index read back from
 *   the workspace was out of range.  max_cross == 0 counts the crossings only (n_cross, 0, 0) in a workspace of
 *   smvs_dsm_contour_workspace_bytes(gw, gh, n_levels, 0) bytes; the caller reads n_cross and calls again with max_cross =
 *   n_cross and a workspace of that size, which then holds the lines.  The doubling runs ceil(log2(max_cross)) rounds
 *   whatever the workspace holds.  The level table reaches the device through kernel arguments, 512 levels a launch.  No
 *   host synchronisation.
 * smvs_dsm_contour_write: with the three counts read from the device, the same dsm and levels, and the workspace as a count
 *   call with max_cross == n_cross left it (the layout follows max_cross): line_level[i] int32, the index into levels;
 *   line_closed[i] uint8; offset[i] int32, n_lines + 1 entries, into vertices; first_line[k] int32, n_levels + 1 entries, the
 *   first line of level k (a level without a line: first_line[k] == first_line[k + 1]); vertices[2 v ..] float64 x, y;
 *   vertex_edge[v] int32, the eid (may be null).  offset[n_lines] is n_vertices, or -1 if the counts or max_cross differ from
 *   the workspace's or an index was out of range.  n_lines == 0: first_line and offset[0] are cleared without a launch.  The
 *   call leaves the workspace as it found it but for its own tables, so it may be repeated.
 *   Every workspace word a kernel reads was written by a kernel of the count call or of the write call (a workspace full of
 *   anything will do); integer atomics (add, or) only: everything depends on dsm, nodata and levels alone, equal bits from run
 *   to run and on any stream, and equal to the numpy statement of this rule, the float64 coordinates included.
 * Limits (SMVS_ERR_ARG, checked before any HIP call): non-null pointers (the line and vertex outputs may be null when
 *   n_lines is 0, vertex_edge always); gw, gh >= 1, gw * gh < 2^29; levels as above; 0 <= max_cross, n_cross < 2^31; n_lines
 *   and n_vertices both 0 or 2 n_lines <= n_vertices <= n_cross; inputs, outputs and workspace do not overlap; workspace:
 *   smvs_dsm_contour_workspace_bytes(gw, gh, n_levels, max_cross) bytes (0 = unsupported arguments): 8 bytes per cell (4 per
 *   lattice edge), 47 per crossing, the 16 KB level table and the scans' block sums. */
/* Hydrology ("Hydrology"): depression filling, D8 directions, accumulation and basins on integer heights.
 *   Cells, heights.  A cell is valid iff it is finite, != (float)nodata and |z| <= 32768.  q = llrint((double)z * 256), halves
 *   to even.  The neighbours of a cell are numbered k = 0 .. 7: E, SE, S, SW, W, NW, N, NE; columns run east and rows south.  A
 *   valid cell is an OUTLET iff one of its eight neighbours is off the grid or invalid: water leaves at the grid's edge and
 *   into voids.
 *   Flood key.  Every valid cell gets K = (w, d), ordered lexicographically: w the filled height in quanta, d a step count
 *   within flats.  K is the unique solution of K(c) = (q_c, 0) at an outlet and K(c) = max((q_c, 0), min over the eight
 *   neighbours n of (w_n, d_n + 1)) elsewhere: the priority-flood with an epsilon per step (Barnes et al. 2014) on integer
 *   pairs.  The step is monotone and strictly raises its argument, so the solution is unique, and Dijkstra from the outlets
 *   and any chaotic downward relaxation from +infinity reach it.  w is the classical filled surface (the lowest surface >= q
 *   without pits, 8-connected); d = 0 exactly at outlets and at cells with a strictly lower neighbour in w, elsewhere one more
 *   than the smallest d among the neighbours of equal w.  A key is the uint64 ((uint64)(w + 2^31) << 32) | d; an invalid
 *   cell is all ones; +infinity, the start of the relaxation, is 0xfffffffe00000000.
 *   Filled DTM.  filled: the cell's own z bits where w == q (untouched cells come back bit for bit), else (float)(w / 256.0),
 *   exact.  depth: (float)((w - q) / 256.0), exact.  flat_dist: int32 d.  Invalid cells get (float)nodata, (float)nodata, -1.
 *   D8 direction.  uint8: 255 invalid, 0 outlet, else k + 1 for the receiver k.  If some neighbour has w_n < w_c the receiver
 *   is the one with the greatest slope (double)(w_c - w_n) / dist[k], one IEEE float64 division per neighbour compared as
 *   doubles, ties to the lowest k; dist is a HOST array of 8 positive finite doubles (xres, hypot, yres, hypot, ... for a
 *   DSMGrid; the library takes no square root).  Otherwise (a flat) the receiver is the neighbour with w_n == w_c and the
 *   smallest d_n, ties to the lowest k; the key equation guarantees one with d_n = d_c - 1.  Along a flow step (w, d) strictly
 *   falls, so the directions of a fixed point's keys form a forest rooted at the outlets.  (Keys that are no fixed point may
 *   leave a cell with no lower or level neighbour: it gets 0.)
 *   Receivers of an arbitrary direction grid.  Accumulation and basins take any uint8 grid: codes 9 .. 254 count as 255; a
 *   cell with code 1 .. 8 whose target is off the grid or has code 255 is a root, like code 0; a cell that reaches no root is
 *   CYCLIC (on a cycle or draining into one).  Roots are found by a pointer doubling of a fixed ceil(log2(gw gh)) + 1 rounds:
 *   a cycle costs nothing extra and nothing can spin.
 *   Accumulation.  acc int64 = the sum of weight over the cell and everything upstream of it; weight int32 (device) or null
 *   for 1 per cell; invalid cells get 0; cyclic cells get -1 and set flag bit 0.  Exact integer sums (they wrap as int64 does).
 *   Basins.  basin int32 = the number of the cell's root, the roots numbered 1 .. n in row-major order of the root cell.  With
 *   a pour mask (uint8, non-zero = pour point) the pour cells that have a code 0 .. 8 are cut from their receivers and are the
 *   only numbered roots; every other tree is 0.  Invalid cells are 0; cyclic cells are 0 and set flag bit 0.  n goes to a
 *   device int.
 * smvs_dsm_flood_begin writes the keys the relaxation starts from: outlets final, other valid cells +infinity, invalid cells
 *   all ones.  smvs_dsm_flood_rounds runs `rounds` (1 .. 4096) global rounds and leaves in status (a device int) how many
 *   tiles changed in the last one: 0 means the keys are the solution.  A round is one workgroup per tile of 32 x 32 cells,
 *   which relaxes the tile in LDS against a halo of one cell until the tile is at its own fixed point, and writes the
 *   interior back.  Keys only fall and never below the solution, so a round reads its neighbours' keys as they are.  The
 *   caller loops; a synchronous relaxation finalises at least one cell a round, so gw gh + 2 rounds bound any grid.
 *   smvs_dsm_flood_read turns keys into filled, depth and flat_dist (each may be null).
 * smvs_dsm_flow_dir: keys and dist -> codes, one lane per cell.
 * smvs_dsm_flow_accumulate ranks an Euler tour of the forest (two elements per cell, successors from the codes of the cell's
 *   and its receiver's neighbours, children in the order of k) by one pointer doubling with int64 suffix sums of
 *   ceil(log2(2 gw gh)) rounds, whatever the grid holds: the number of launches grows with log(gw gh), not with the longest
 *   river.  smvs_dsm_flow_basins numbers the roots by a scan.  No host synchronisation in any entry.  Every workspace word a
 *   kernel reads was written by a kernel of the same call (a workspace full of anything will do); the only atomic is an
 *   integer OR into the flag: everything depends on the inputs alone, equal bits from run to run and on any stream, and equal
 *   to the Python statement of this rule.
 * Limits (SMVS_ERR_ARG, checked before any HIP call): non-null pointers (filled, depth, flat_dist, weight and pour may be
 *   null); gw, gh >= 1, gw * gh < 2^30 (the tour's 2 gw gh elements are int32); 1 <= rounds <= 4096; dist finite and > 0;
 *   inputs, outputs and workspace do not overlap; workspace: smvs_dsm_flood_workspace_bytes(gw, gh) = 16 KB of round
 *   counters for the flood, smvs_dsm_flow_workspace_bytes(gw, gh) for accumulate and basins (0 = unsupported arguments): 56
 *   bytes per cell (receiver 4, root pointer 4, two copies of the tour's successors 16 and sums 32) and the scan's block
 *   sums.  No kernel uses scratch. */
/* Stream network ("Stream network"): Strahler orders, links and flow length over a direction grid.
 *   Inputs.  dir (gh, gw) uint8 "index" codes with the meaning smvs_dsm_flow_accumulate gives them: codes 9 .. 254 count as
 *   255, a target off the grid or invalid makes a root, edited grids with cycles are allowed.  mask (gh, gw) uint8, non-zero =
 *   a stream cell; any mask is taken, not only acc >= t.
 *   Stream cells.  S = the cells with mask != 0 that are tree cells (a code 0 .. 8 and a root).  Cyclic cells are never in S;
 *   if the grid holds a cyclic cell, masked or not, flag bit 0 is set, as in accumulate.
 *   Induced forest.  down(c) = c's receiver if that is in S; otherwise c has none and is a MOUTH.  in(c) = the number of cells
 *   u in S with down(u) = c.  A gap in the mask cuts the network: nothing upstream of a gap counts below it.
 *   Strahler order.  order(c) = 1 if in(c) = 0.  Otherwise let m be the greatest order among the cells flowing into c:
 *   order(c) = m + 1 if at least two of them have order m, else m.  The order map is uint8, 0 outside S; below 2^30 cells the
 *   order is at most 30.
 *   Links.  A cell of S is a HEAD iff in(c) != 1 (a source or a junction); every head starts one link.  A cell with in = 1
 *   belongs to the link of the one cell that flows into it.  A link's cells are listed downstream from the head; its last
 *   cell e has no down (a mouth) or in(down(e)) >= 2.  next_link = the link that down(e) heads, or -1.  Links are numbered
 *   0 .. n_links - 1 in row-major order of their head cells.
 *   Vertices.  int32 (col, row) of the link's cells, head first, then down(e) when it exists: adjacent links share the
 *   junction and the lines connect.  A link of one cell at a mouth has one vertex; it stays in the tables.
 *   Per link: head (the cell index), order, next_link, offset (n_links + 1 entries into the vertices), steps int32
 *   (n_links, 3) = the E-W, N-S and diagonal segments of its polyline, the closing one included.  link map int32 (gh, gw):
 *   link number + 1 on S, 0 elsewhere.  counts, a device int[4]: stream cells, links, vertices, highest order.
 *   Flow length.  steps int32 (gh, gw, 3): the E-W, N-S and diagonal steps of the cell's path to its root over the whole
 *   direction grid; a root has (0, 0, 0); invalid and cyclic cells get -1, cyclic ones set flag bit 0.  The length in metres
 *   is the caller's: (n_ew xres + n_ns yres) + n_diag hypot(xres, yres); the library handles the integers only.
 * smvs_dsm_stream_order runs the network pass and writes order, link_map (may be null) and counts.  The host reads counts
 *   once, allocates, and calls smvs_dsm_stream_write with n_links = counts[1] and n_vertices = counts[2].  WRITE REDOES THE
 *   PASS: it reads nothing of an earlier call, so the workspace may be another one or may have been used in between, and a
 *   workspace full of anything will do for both.  If n_links or n_vertices differ from the network's counts (too small, for
 *   one) it writes -1 into offset[n_links] and nothing else; the return value is SMVS_OK, as nothing is read back.
 *   The pass: receivers and roots as in accumulate; an Euler tour of the induced forest, the trees chained in row-major order
 *   of their mouths, ranked by one doubling of ceil(log2(2 gw gh)) rounds; at most min(30, floor(log2(gw gh))) order rounds of
 *   one mark kernel, one scan of the marks at their tour positions and one promotion (a cell rises to k + 1 iff it or
 *   something upstream of it has two inflowing cells of order >= k), which leave at once on a device counter after the first
 *   round without a mark; heads numbered by a scan; (head, distance) per cell by ceil(log2(gw gh)) + 1 rounds of an in-place
 *   doubling.  smvs_dsm_flow_length is one doubling of ceil(log2(gw gh)) rounds with the three counts as sums.  The number
 *   of launches depends on gw gh alone, never on the longest river or link.  No host synchronisation in any entry; every
 *   workspace word a kernel reads was written by a kernel of the same call; integer atomics only (adds into the counts and
 *   the links' step counts, an OR into the flag), so everything is equal bits from run to run and on any stream.
 * Limits (SMVS_ERR_ARG, checked before any HIP call): non-null pointers (link_map may be null); gw, gh >= 1, gw * gh < 2^30;
 *   0 <= n_links <= gw gh, 0 <= n_vertices <= 2 gw gh; inputs, outputs and workspace do not overlap; workspace:
 *   smvs_dsm_stream_workspace_bytes(gw, gh) for all three (0 = unsupported arguments): 54 bytes per cell, the scans' block
 *   sums and 512 bytes of counters; flow length uses the first 32 per cell.  No kernel uses scratch. */
/* Cost distance ("Cost distance"): the accumulated cost of the cheapest trip from every cell to a source
 * over a grid that is not uniformly passable, and its back-links as a D8 direction grid.  Integer arithmetic throughout.
 *   Inputs.  friction (gh, gw) uint16, device: 0 a barrier, 1 .. 65535 the cost per metre in units of 2^-8; null = 256
 *   everywhere.  sources (gh, gw) uint8, non-zero = a source; a source on a barrier is no source.  dsm (gh, gw) float32 with
 *   nodata, or null; table a HOST int32[256] with entries 0 .. 65535 in units of 2^-8, or null; dsm and table come together or
 *   not at all.  With a DSM a cell without a height (the test and q of "Hydrology": finite, != nodata, |z| <= 32768, q =
 *   llrint(256 z)) is a barrier.  L a HOST int32[8], 1 <= L[k] <= 32767: the step lengths towards the neighbours k = 0 .. 7 (E,
 *   SE, S, SW, W, NW, N, NE, as in "Hydrology") in units of 2^-8 m; the library takes no square root.  reverse is 0 or 1.
 *   Step cost.  For a passable cell c and its passable neighbour n in direction k: x = (f_c + f_n) L[k] T in int64.  Without a
 *   table T = 256.  With one, delta = q_n - q_c (with reverse q_c - q_n: travel FROM the sources), bin = clamp(floor(32 delta /
 *   L[k]), -128, 127) + 128 with the floor towards -infinity (tan(slope) in steps of 1/32 out to +-4), T = table[bin], and T = 0
 *   forbids the step.  w = max(1, floor(x / 2^10)) in units of 2^-15 cost metre.  Every step costs at least 1.  A diagonal
 *   step does not look at the two cells beside it.
 *   Keys.  D(c) = 0 at a passable source, else the minimum over the allowed steps c -> n of D(n) + w: because w >= 1 the
 *   solution is unique and is the cost of the cheapest path.  A key is the uint64 D; a barrier is all ones; a cell not
 *   reached yet, or not reachable, is all ones - 1.  gw gh <= 2^24 and w < 2^38 keep D below 2^62.
 *   Back-link.  uint8 in the direction codes of "Hydrology": 0 at a source, 255 at barriers and unreachable cells, else k + 1
 *   for the k that attains the minimum, ties to the lowest k.  D falls strictly along a back-link, so the grid is a forest
 *   rooted at the sources, and smvs_dsm_flow_basins (the allocation), smvs_dsm_flow_length, smvs_dsm_flow_accumulate and
 *   smvs_dsm_stream_* (the least-cost paths as links) take it as it is.
 *   Reading.  raw int64 = D, -1 at barriers and unreachable cells.  cost float64 = (double)D / 32768.0, one conversion and one
 *   IEEE division; +Inf where unreachable, NaN (0x7ff8000000000000) on barriers.  With max_cost (all ones for none) a cell
 *   with D > max_cost reads as unreachable, back-link 255; everything upstream of it costs more, so the forest stays closed.
 * smvs_dsm_cost_begin writes the keys the relaxation starts from (sources 0, barriers all ones, the rest all ones - 1) and the
 *   number of passable sources to n_sources, a device int (block counts summed in a fixed order, no atomics).
 *   smvs_dsm_cost_rounds runs `rounds` (1 .. 4096) global rounds and leaves in status (a device int) how many tiles changed
 *   in the last one: 0 means the keys are the solution.  A round is one workgroup per tile of 32 x 32 cells, which lowers the
 *   tile's cells in LDS against a halo of one cell until the tile is at its own fixed point and writes the interior back if
 *   anything moved.  Keys only fall and never below the solution, so a round reads its neighbours' keys as they are; gw gh + 2
 *   rounds bound any grid.  smvs_dsm_cost_read turns keys into raw, cost and backlink (each may be null).  All three take
 *   the same friction and dsm; rounds and read the same L, table and reverse.  No host synchronisation in any entry.  Every
 *   workspace word a kernel reads was written by a kernel of the same call; the only atomic is the per-launch counter of moved
 *   tiles: equal bits from run to run, for any batching of the rounds, on any stream, and equal to the Python statement of
 *   this rule (tests/dsm_cost_oracle.py).
 * Limits (SMVS_ERR_ARG, checked before any HIP call): non-null sources, keys, n_sources, status, L and workspace; dsm and
 *   table both or neither; gw, gh >= 1, gw * gh <= 2^24; 1 <= rounds <= 4096; L and table in range; reverse 0 or 1; inputs,
 *   outputs and workspace do not overlap; workspace: smvs_dsm_cost_workspace_bytes(gw, gh) (0 = unsupported arguments): 16 KB
 *   of round counters, 1 KB for the table and 4 bytes per 256 cells.  No kernel uses scratch. */
/* Seeded flood ("Seeded flood"): grey-scale geodesic reconstruction, a flood from chosen cells at chosen
 * levels, and its back-links as a D8 direction grid: the marker watershed.  Integer arithmetic throughout.
 *   Cells, heights.  As in "Hydrology": a cell is valid iff it is finite, != (float)nodata, |z| <= 32768, and its domain byte is
 *   non-zero when a domain (gh, gw) uint8 is given.  q = llrint(256 z), halves to even; g = polarity q with polarity +1 or -1.
 *   The neighbours are k = 0 .. 7 as there.  Invalid and off-grid neighbours are WALLS; they are not outlets.
 *   Seeds.  marker (gh, gw) float32 with the same validity rule (finite, != nodata, |m| <= 32768).  A valid cell with a valid
 *   marker is a seed at level s = max(g_c, polarity q(marker_c) + offset); offset is an int32 in quanta, |offset| <= 2^25.
 *   Key.  K = (w, d), packed as the flood packs it, is the unique solution of
 *     K(c) = max((g_c, 0), min(S_c, min over the valid neighbours n of K(n) + 1))
 *   with S_c = (s, 0) at a seed and +infinity elsewhere, and +infinity + 1 = +infinity (saturating): a component without a seed
 *   stays at exactly 0xfffffffe00000000 however many rounds run.  Every step strictly raises its argument, so no finite cycle
 *   supports itself: a finite key hangs on a chain of strictly lower keys that ends at a seed with K = S, the solution is
 *   unique, and Dijkstra from the seeds and any chaotic downward relaxation from (S, +infinity) reach it.  With polarity +1, w is
 *   the reconstruction by erosion of the marker (clamped to the surface from above) over the surface; with polarity -1, -w is the
 *   reconstruction by dilation of the marker (clamped from below) under it.
 *   Back-link.  uint8 in the direction codes of "Hydrology": 255 at an invalid or unreached cell; 0 at a ROOT, a seed with
 *   K(c) == S_c (the seed wins a tie against a neighbour); otherwise k + 1 for the neighbour with the least key, ties to the
 *   lowest k.  Keys fall strictly along a link, so the links form a forest rooted at the roots, and smvs_dsm_flow_basins,
 *   smvs_dsm_flow_accumulate and smvs_dsm_flow_length take it as it is.  (Keys that are no fixed point may leave a cell with no
 *   lower neighbour: it gets 0.)
 *   Reading.  surface: the cell's own z bits where w == g (untouched cells come back bit for bit), else (float)(polarity w /
 *   256.0), exact.  level_steps: int32 d.  Invalid and unreached cells get (float)nodata, -1 and 255.  n_unreached, a device
 *   int: the valid cells still at +infinity.
 * smvs_dsm_seed_begin writes the keys the relaxation starts from (seeds (s, 0), other valid cells +infinity, invalid cells all
 *   ones) and the number of seeds to n_seeds, a device int (block counts summed in a fixed order, no atomics).
 *   smvs_dsm_seed_rounds runs `rounds` (1 .. 4096) global rounds and leaves in status (a device int) how many tiles changed in
 *   the last one: 0 means the keys are the solution.  A round is one workgroup per tile of 32 x 32 cells, which relaxes the tile
 *   in LDS against a halo of one cell until the tile is at its own fixed point and writes the interior back if anything moved.
 *   Unlike the flood, all valid cells are open, seeds included, because another seed may undercut them; as keys only fall, the
 *   rounds need no marker.  gw gh + 2 rounds bound any grid.  smvs_dsm_seed_read turns keys into surface, level_steps, backlink
 *   and n_unreached (each may be null).  The three take the same dsm, nodata and polarity; begin and read the same marker,
 *   domain and offset.  No host synchronisation in any entry.  Every workspace word a kernel reads was written by a kernel of
 *   the same call; the only atomic is the per-launch counter of moved tiles: equal bits from run to run, for any batching of
 *   the rounds, on any stream, and equal to the Python statement of this rule (tests/dsm_watershed_oracle.py).
 * Limits (SMVS_ERR_ARG, checked before any HIP call): non-null dsm, marker, keys, n_seeds, status and workspace; polarity +1
 *   or -1; gw, gh >= 1, gw * gh < 2^30; |offset| <= 2^25; 1 <= rounds <= 4096; no buffer written overlaps another buffer (the
 *   inputs may overlap one another: h-maxima give the DSM as its own marker); workspace: smvs_dsm_seed_workspace_bytes(gw, gh)
 *   (0 = unsupported arguments): 16 KB of round counters and 4 bytes per 256 cells.  No kernel uses scratch. */
/* Meshes ("Meshes"): an error-bounded triangle mesh of a DSM, the adaptive right-triangulated irregular
 *   network (RTIN: longest-side bisection) over the lattice of cell centres, in integers throughout.
 *   Lattice.  The vertices are the cell centres (row r, col c) of a (gh, gw) float32 DSM with the heights of the exact tools:
 *   q = rn(256 z), valid iff finite, != (float)nodata and |z| <= 32768.  Root squares of side S = tile = 2^k cells (1 <= k <= 10)
 *   cover the lattice from (0, 0): max(1, ceil((gh - 1) / S)) by max(1, ceil((gw - 1) / S)) of them.  Vertices beyond the grid
 *   are invalid; there is no triangle beyond the cover.
 *   Hierarchy.  A triangle is (a, b, c): hypotenuse a -> b, right angle at its apex c.  The root square at (r0, c0) holds
 *   ((r0, c0), (r0 + S, c0 + S), (r0 + S, c0)) and ((r0 + S, c0 + S), (r0, c0), (r0, c0 + S)).  With m = (a + b) / 2, the split
 *   vertex, the children of (a, b, c) are (c, a, m) and (b, c, m).  Levels 0 .. 2 k; the triangles of level 2 k have legs of one
 *   cell and are not split.  Every vertex that is no root corner splits the triangles of exactly one level, one or two of them.
 *   Exact error.  E(T) = +infinity if a lattice vertex in the closed triangle T is invalid, else the maximum over the lattice
 *   vertices p in closed T of |q_p - plane_T(p)|.  Every barycentric weight has a denominator that divides S (a leg of T is h
 *   or h / 2 lattice steps long, straight or diagonal, h = S / 2^j), so errors are exact integers in units of 2^-8 m / S, below
 *   2^37; +infinity is 2^63 - 1.  This is the error of the whole triangle, not of its hypotenuse's midpoint alone.
 *   Vertex error.  e(m) = max E(T) over the triangles that m splits.  Saturation: from the finest split level to the coarsest,
 *   e(apex of T) <- max(e(apex of T), e(m(T))), an m beyond the grid counting as +infinity; the root triangles' apexes are root
 *   corners, which hold 0.
 *   Active.  A vertex is active iff e > threshold = floor(256 tol) S (strict); every root corner and every vertex beyond the
 *   grid is active.  Emission.  A triangle of a level below 2 k is emitted iff its apex is active and its split vertex is not; a
 *   triangle of level 2 k iff its apex is active and its three corners are valid.  It follows that the mesh is conforming (no
 *   vertex strictly inside an edge), that it covers exactly the half-cells of level 2 k with three valid corners (voids and
 *   the grid's outside are holes, refined down to single cells along their rim), and that every lattice vertex in an emitted
 *   triangle deviates from its plane by at most floor(256 tol) quanta; tol = 0 is lossless in the quantised heights.
 *   Order.  Vertices: the lattice vertices of the emitted triangles in row-major order.  Triangles: sorted by (row of a + b,
 *   col of a + b, side), a unique key: a + b is twice the split vertex, for level 2 k twice a cell's middle; side is 0 for the
 *   triangle whose apex is the lexicographically smaller (row, col) of the two that can share the hypotenuse, 1 for the other
 *   (also where only one of them lies in the cover).  Each is written a, b, c with a and b swapped where needed so that it is
 *   counter-clockwise seen from above, east right and north up (x = col, y = -row).
 * smvs_dsm_mesh_errors: errors[r gw + c] int64 <- the saturated e of every vertex of the grid.  One launch clears, one finds the
 *   deviations of all levels (a lane per vertex, 64-bit integer max atomics, the lanes of a wave that share a split vertex
 *   combined first), 2 k - 1 gather passes saturate.  No workspace.  The maximum is order-free: equal bits from run to run.
 * smvs_dsm_mesh_count: with errors, the same dsm, nodata and tile and threshold = floor(256 tol) S in the errors' units:
 *   counts (device, 2 ints) <- n_triangles, n_vertices; the workspace keeps, per slot pair of the order (gh rows of gw vertices
 *   and gw - 1 cells), the two sides' emission and the exclusive scan of their number, and the scan of the used vertices.  No host
 *   synchronisation; the caller reads counts.
 * smvs_dsm_mesh_write: with the workspace as smvs_dsm_mesh_count left it and its two counts: triangles int32 (3 per triangle,
 *   indices into the vertex list), tri_level uint8, vertices int32 (col, row per vertex), z float32, the DSM's own bits.  status
 *   (device, 1 int) <- n_triangles, or -1 with nothing else written if n_triangles or n_vertices differ from the workspace's
 *   counts (arrays one too small, say).  The workspace is left as found: the call may be repeated.
 * smvs_dsm_mesh_heights: heights[r gw + c] float32 <- the mesh's height at every vertex, nodata where the vertex is invalid or in
 *   no emitted triangle; dev (may be null) int64 <- S q_p - S plane(p) in the errors' units, 2^63 - 1 where uncovered.  A lane per
 *   vertex walks down from its root triangle (the one under the root's diagonal if p lies on it; the root square to the right
 *   and below if p lies on a rim between two) into the child (c, a, m) if p lies on a's side of the line c - m or on it, else
 *   into (b, c, m), while the split vertex is active: at most 2 k steps.  height = fl32(fl64(S plane) / fl64(256 S)), one IEEE
 *   division of two exact doubles.  A walk that ends in a triangle of level 2 k with an invalid corner gives the vertex its own
 *   q if an emitted triangle uses the vertex, else nodata.  All triangles that hold p agree on its height: a mesh vertex is
 *   exact in each; p strictly inside an edge shared by two emitted triangles is interpolated along the edge's two ends by
 *   both; and if a walk runs past an emitted triangle T that holds p, p is the split vertex of a descendant of T and active, so
 *   by saturation T's split vertex is active and T is not emitted -- so a walk that reaches level 2 k without stopping has
 *   passed no emitted triangle with p inside it or inside an edge, and only triangles with p as a corner are left.
 *   Every workspace word a kernel reads was written by a kernel of the same call or, for write, of the count call (a
 *   workspace full of anything will do).  No kernel uses scratch.
 * Limits (SMVS_ERR_ARG with a message, before any HIP call; nothing is written): non-null pointers (dev may be null; the
 *   outputs of write may be null where their count is 0); gw, gh >= 1, gw * gh < 2^29; tile a power of two in 2 .. 1024;
 *   threshold >= 0; 0 <= n_triangles <= 2 gw gh, 0 <= n_vertices <= gw gh; inputs, outputs and workspace do not overlap;
 *   workspace: smvs_dsm_mesh_workspace_bytes(gw, gh, tile) bytes (0 = unsupported arguments): 14 bytes per cell (two slot pairs
 *   of 4 + 1 bytes and a 4-byte vertex mark) and the scans' block sums. */
/* Facets ("Facets"): a DSM segmented into planar facets (roof faces, flat ground) and the plane of every
 *   facet, in exact integers up to the plane's float64 coefficients.
 *   Heights.  A cell is valid iff it is finite, != (float)nodata and |z| <= 32768; q = rn(256 z), halves to even, in units of
 *   2^-8 m.  With a mask (uint8, non-zero = inside; may be null) a cell outside the mask is invalid everywhere below.
 *   Local plane of a cell p: defined only if p and its eight neighbours are on the grid and valid.  Rows grow southwards.
 *     Gx = (q[NE] + 2 q[E] + q[SE]) - (q[NW] + 2 q[W] + q[SW]),  Gy = (q[SW] + 2 q[S] + q[SE]) - (q[NW] + 2 q[N] + q[NE]),
 *   8 x the height step per column and per row; both are written as 0 where the local plane is undefined.  p is planar iff
 *   |8 (q[k] - q[p]) - (Gx dx_k + Gy dy_k)| <= 8 T for each of the eight neighbours k at offset (dx, dy); T = floor(256 tol).
 *   Adjacency.  Two planar neighbours p and n, (dx, dy) the offset from p to n, are linked iff |Gx_p - Gx_n| <= Ax and
 *   |Gy_p - Gy_n| <= Ay and |16 (q_n - q_p) - ((Gx_p + Gx_n) dx + (Gy_p + Gy_n) dy)| <= 16 T; neighbours are the 4 or the 8 of
 *   `connectivity`; Ax = floor(2048 slope_tol xres), Ay = floor(2048 slope_tol yres), slope_tol a difference of tan(slope).
 *   The test is symmetric in p and n.  (Between two planar cells the third condition cannot fail: its left side is the
 *   difference of the two cells' planarity residuals towards each other, each at most 8 T.  It is part of the rule all the same.)
 *   A facet is a class of the transitive closure of links; facets are numbered 1 .. n in
 *   raster order of their first planar cell (smvs_dsm_label's numbering).  Widths: |q| <= 2^23, so |Gx|, |Gy| <= 2^26, the
 *   planarity residual is below 2^28 + 2^27 and the link residual below 2^29 + 2^28; with 0 <= T, Ax, Ay <= 2^26 nothing wraps
 *   in an int32.
 *   Growth (grow = 1, one round).  A valid cell u that is not planar takes the label of the first of its neighbours p, in
 *   the order k = 0 .. 7 of E, SE, S, SW, W, NW, N, NE ("Hydrology"), that is planar and has
 *   |8 (q_u - q_p) - (Gx_p dx + Gy_p dy)| <= 8 T, (dx, dy) the offset from p to u.  Always all eight neighbours; it reads only
 *   labels and gradients of planar cells and never renumbers.  Everything else gets 0: invalid cells, cells outside the mask,
 *   non-planar cells that were not grown.
 *   Known property.  Links are pairwise, so a gently curved surface (a dome, rolling terrain) chains into one facet; its rms
 *   and max_abs say so, and callers reject by them.  A face needs at least one cell whose whole 3 x 3 window lies in it.
 * smvs_dsm_facet_normals: Gx, Gy int32 and planar uint8 (gh, gw) of every cell.  One lane per cell, no workspace.
 * smvs_dsm_facet_label: labels (gh, gw) int32; n_out (device, one int) <- n, or -1 if a union-find loop reached its bound
 *   (cannot happen on an undamaged labels buffer: every find and union strictly lowers an index with each step).  The
 *   workspace keeps q, Gx, Gy and the planar flag of every cell, the roots' ranks and the scan's block sums; every word a
 *   kernel reads was written by a kernel of the same call.  The result depends on the inputs alone: equal bits from run to
 *   run, on any stream, and to the numpy statement of the rule (tests/dsm_facet_oracle.py).
 * smvs_dsm_facet_planes: per label k + 1, k = 0 .. n - 1, over the cells of `labels` that carry it and are valid (no mask):
 *   sums int64 (n, 4): n_k, sum c, sum r, sum q; centre int32 (n, 3): cb = floor(sum c / n_k), rb = floor(sum r / n_k),
 *   qb = floor(sum q / n_k) (zeros where n_k = 0); with dc = c - cb, dr = r - rb, dq = q - qb, moments int64 (n, 8): the sums
 *   Sx, Sy, Sz, Sxx, Sxy, Syy, Sxz, Syz of dc, dr, dq, dc^2, dc dr, dr^2, dc dq, dr dq.
 *   Bound: gw, gh <= 32768 and gw gh < 2^24, so |dc|, |dr| < 2^15 and |dq| <= 2^24: a term is below 2^39 and a sum of fewer
 *   than 2^24 terms below 2^63.  Larger scenes go through tiles.
 *   plane float64 (n, 3): a (units per column), b (units per row), h0 (the plane's height at (cb, rb), in units), every
 *   operation an IEEE double operation by itself (the library is built with -ffp-contract=off), N and the sums converted
 *   to double first (round to nearest):
 *     cxx = Sxx - (Sx Sx) / N, cxy = Sxy - (Sx Sy) / N, cyy = Syy - (Sy Sy) / N, cxz = Sxz - (Sx Sz) / N, cyz = Syz - (Sy Sz) / N,
 *     det = cxx cyy - cxy cxy, a = (cxz cyy - cyz cxy) / det, b = (cyz cxx - cxz cxy) / det,
 *     h0 = (double)qb + ((Sz / N - a (Sx / N)) - b (Sy / N)).
 *   !(det > 0) gives NaN for all three: fewer than three cells, or cells on one line.  An 8-connected collinear set is a row,
 *   a column or a diagonal; for a row or a column Sy = Sxy = Syy = 0 (Sx = Sxy = Sxx = 0), for a diagonal dr = dc and for an
 *   anti-diagonal dr = -dc or 1 - dc, for which cxx, cyy and |cxy| are the same exactly representable number: det is exactly 0.
 *   Residuals: e = q - rn((h0 + a dc) + b dr), the sum clamped to +-2^40 before rounding and e to +-2^16; sse int64 (n) = sum
 *   e^2 and max_abs int32 (n) = max |e|; both 0 for a NaN plane.  Integer atomics only, after a reduction along a wave's rows
 *   and columns on chip: equal bits from run to run and to the numpy statement, float64 coefficients included.
 *   n == 0 returns SMVS_OK without a launch.
 * Limits (SMVS_ERR_ARG with a message, before any HIP call; nothing is written): non-null pointers (mask may be null); gw, gh
 *   >= 1 and gw gh < 2^31 (planes: the bound above); 0 <= T, Ax, Ay <= 2^26; connectivity 4 or 8; grow 0 or 1; n >= 0; inputs,
 *   outputs and workspace do not overlap; workspace: smvs_dsm_facet_workspace_bytes(gw, gh) bytes (0 = unsupported arguments),
 *   17 bytes per cell and the scan's block sums.  Every entry takes a stream, does no host synchronisation and initialises
 *   every output it owns.  No kernel uses scratch. */
typedef struct smvs_dsm_layer {
    const float* z;              /* (gh, gw) float32, device */
    const int* d2;               /* (gh, gw) int32, device; may be null outside mode 5 */
    int gw, gh, ox, oy;
} smvs_dsm_layer;

int smvs_tm_project(const double* tm7, const double* a, const double* b, double* o0, double* o1, size_t n, int dir, void* stream);
int smvs_rpc_dsm_bin(const float* height, const unsigned char* mask, const double* rpc170, int H, int W,
                     const double* tm7, const double* grid4, int gw, int gh,
                     int* cell, unsigned* count, double* east, double* north, void* stream);
int smvs_rpc_dsm_render(const float* dsm, int gw, int gh, const double* grid4, float nodata, const double* tm7,
                        const double* rpc170, int H, int W, int x0, int y0, double h_lo, double h_hi, double tol,
                        float* height, void* stream);
int smvs_rpc_ortho(const float* dsm, int gw, int gh, const double* grid4, float nodata, const double* tm7,
                   const double* rpc170, const float* image, int H, int W, int C, int x0, int y0,
                   double h_hi, int occlusion, double occ_tol, int view,
                   float* ortho, int* source, unsigned char* state, void* stream);
size_t smvs_dsm_workspace_bytes(size_t n, int gw, int gh);
int smvs_dsm_reduce(const int* cell, const float* height, size_t n, const unsigned* count, int gw, int gh,
                    int mode, float nodata, float* dsm, void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_despike(const float* dsm, int gw, int gh, float nodata, int radius, double thresh, int min_valid,
                     float* out, unsigned char* removed, void* stream);
size_t smvs_dsm_fill_workspace_bytes(int gw, int gh, int max_steps);
int smvs_dsm_fill(const float* dsm, int gw, int gh, float nodata, int max_steps, int min_hits, int method,
                  float* out, unsigned char* hits, void* workspace, size_t workspace_bytes, void* stream);
size_t smvs_dsm_morph_workspace_bytes(int gw, int gh, int max_radius);
int smvs_dsm_morph(const float* dsm, int gw, int gh, float nodata, int radius, int op, float* out,
                   void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_ground(const float* dsm, int gw, int gh, float nodata, const int* radii, const double* thresholds, int n_levels,
                    float* dtm, unsigned char* cls, void* workspace, size_t workspace_bytes, void* stream);
size_t smvs_dsm_label_workspace_bytes(int gw, int gh);
int smvs_dsm_label(const unsigned char* mask, int gw, int gh, int connectivity, int* labels, int* n_out,
                   void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_label_stats(const int* labels, const float* values, int gw, int gh, float nodata, int n,
                         int* area, int* bbox, long long* rc_sum,
                         int* nvalid, float* vmin, float* vmax, long long* qsum, void* stream);
size_t smvs_dsm_label_select_workspace_bytes(int n, int n_ranks);
int smvs_dsm_label_select(const int* labels, const float* values, int gw, int gh, float nodata, int n,
                          const float* centre /* may be null */, const int* ranks /* device, n x n_ranks */, int n_ranks,
                          float* out, int* nvalid /* may be null */, void* workspace, size_t workspace_bytes, void* stream);
size_t smvs_dsm_focal_table_bytes(int gw, int gh);
int smvs_dsm_focal_build(const float* dsm, int gw, int gh, float nodata, void* tables, size_t table_bytes, void* stream);
int smvs_dsm_focal_query(const void* tables, int gw, int gh, const int* rects /* host, n_rects x 5 */, int n_rects,
                         int ow, int oh, int c0, int r0, int sx, int sy, int min_valid,
                         int* n, long long* s1, long long* s2, double* mean, double* var /* each may be null */,
                         int* status, void* stream);
#define SMVS_DSM_RANK_TILE 32 /* side of the square tile of output cells one workgroup of the focal order statistics owns */
int smvs_dsm_focal_select(const float* dsm, int gw, int gh, float nodata, const int* runs /* host, n_runs x 3 */, int n_runs,
                          const int* levels /* host, n_levels x 2 */, int n_levels, const float* centre /* may be null */,
                          int* n_out /* may be null */, float* lo, float* hi /* may be null */, void* stream);
int smvs_dsm_focal_count(const float* dsm, int gw, int gh, float nodata, const int* runs /* host, n_runs x 3 */, int n_runs,
                         const float* t, int* n_out /* may be null */, int* below, int* equal, void* stream);
size_t smvs_dsm_shift_workspace_bytes(int gwa, int gha, int gwb, int ghb, int radius);
int smvs_dsm_shift_stats(const float* a, int gwa, int gha, const float* b, int gwb, int ghb, float nodata,
                         int ox, int oy, int radius, double dz0, double trim,
                         long long* stats, void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_regrid(const float* src, int gws, int ghs, const double* grid4_src, float nodata,
                    const double* grid4_dst, int gwd, int ghd, int mode, double dz, float* out, void* stream);
size_t smvs_dsm_dist_workspace_bytes(int gw, int gh, int max_dist);
int smvs_dsm_dist(const unsigned char* mask, int gw, int gh, int border, int max_dist,
                  int* d2, void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_mosaic(const smvs_dsm_layer* layers, int n_layers, float nodata, int mode, int feather,
                    int gw, int gh, float* out, unsigned char* count, unsigned char* source, float* spread, void* stream);
int smvs_dsm_stack_select(const smvs_dsm_layer* layers, int n_layers, float nodata,
                          const int* levels /* host, n_levels x 2: num, den */, int n_levels,
                          const float* centre /* device (gh, gw), may be null */,
                          int gw, int gh, unsigned char* count /* may be null */,
                          float* lo, float* hi /* (n_levels, gh, gw); hi may be null */, void* stream);
int smvs_dsm_stack_fuse(const smvs_dsm_layer* layers, int n_layers, float nodata,
                        double kmad, double floor, int min_count, int gw, int gh,
                        float* out, float* median, float* mad, unsigned char* count, unsigned char* n_in,
                        long long* members, long long* inliers /* all but out may be null */, void* stream);
size_t smvs_dsm_shadow_workspace_bytes(int gw, int gh);
int smvs_dsm_shadow(const float* dsm, int gw, int gh, float nodata,
                    double ucol, double urow, double a, double b, double tol,
                    unsigned char* shade, float* depth, void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_gradient(const float* dsm, int gw, int gh, float nodata, double xres, double yres,
                      float* dzde, float* dzdn, void* stream);
size_t smvs_dsm_horizon_workspace_bytes(int gw, int gh, int n_dirs);
int smvs_dsm_horizon(const float* dsm, int gw, int gh, float nodata,
                     const double* dirs /* HOST, n_dirs x 4: ucol, urow, a, b */, int n_dirs,
                     float* tan_h /* device, (n_dirs, gh, gw) */,
                     void* workspace, size_t workspace_bytes, void* stream);
size_t smvs_dsm_viewshed_workspace_bytes(int gw, int gh, int n_obs);
int smvs_dsm_viewshed(const float* dsm, int gw, int gh, float nodata, double xres, double yres, double c256, double r2max,
                      const int* obs /* HOST, n_obs x 5: col, row, eye, mode, tgt */, int n_obs,
                      unsigned char* seen, float* above /* may be NULL */, int* status,
                      void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_los(const float* dsm, int gw, int gh, float nodata, double xres, double yres, double c256, double r2max,
                 const int* pairs /* DEVICE, n_pairs x 7: col_o, row_o, eye, mode, col_t, row_t, tgt */, int n_pairs,
                 unsigned char* seen, float* above /* may be NULL */, void* stream);
size_t smvs_dsm_outline_workspace_bytes(int gw, int gh, int max_edges);
int smvs_dsm_outline_count(const int* labels, int gw, int gh, int n, int max_edges, int* counts,
                           void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_outline_write(const int* labels, int gw, int gh, int n, int n_edges, int n_rings, int n_vertices,
                           int* ring_label, long long* area2, int* edges, int* offset, int* first_ring, int* vertices,
                           void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_burn(const int* vertices, const int* offset, const int* ring_label, int n_rings, int n_vertices,
                  int gw, int gh, int* out, int* flag, void* stream);
int smvs_dsm_burn_polygons(const int* vertices, const int* offset, const int* ring_label, int n_rings, int n_vertices,
                           int gw, int gh, int* out, int* flag, void* stream);
size_t smvs_dsm_simplify_workspace_bytes(int n_rings, int n_vertices);
int smvs_dsm_simplify_begin(const int* vertices, const int* offset, int n_rings, int n_vertices, int* flag,
                            void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_simplify_rounds(const int* vertices, const int* offset, int n_rings, int n_vertices, int tol16, int rounds,
                             int* status, void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_simplify_count(const int* vertices, const int* offset, int n_rings, int n_vertices, int* n_out,
                            void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_simplify_write(const int* vertices, const int* offset, int n_rings, int n_vertices, int n_out,
                            int* out_offset, int* out_vertices, long long* area2, int* kept, unsigned char* simplified,
                            void* workspace, size_t workspace_bytes, void* stream);
size_t smvs_dsm_contour_workspace_bytes(int gw, int gh, int n_levels, int max_cross);
int smvs_dsm_contour_count(const float* dsm, int gw, int gh, float nodata,
                           const int* levels /* HOST, n_levels odd int32 in units of 2^-9 m, rising */, int n_levels,
                           int max_cross, int* counts, void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_contour_write(const float* dsm, int gw, int gh, float nodata, const int* levels /* HOST */, int n_levels,
                           int n_cross, int n_lines, int n_vertices, int* line_level, unsigned char* line_closed,
                           int* offset, int* first_line, double* vertices, int* vertex_edge /* may be null */,
                           void* workspace, size_t workspace_bytes, void* stream);
size_t smvs_dsm_flood_workspace_bytes(int gw, int gh);
int smvs_dsm_flood_begin(const float* dsm, int gw, int gh, float nodata, unsigned long long* keys,
                         void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_flood_rounds(const float* dsm, int gw, int gh, float nodata, unsigned long long* keys, int rounds,
                          int* status, void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_flood_read(const float* dsm, int gw, int gh, float nodata, const unsigned long long* keys,
                        float* filled /* may be null */, float* depth /* may be null */, int* flat_dist /* may be null */,
                        void* stream);
int smvs_dsm_flow_dir(const unsigned long long* keys, int gw, int gh, const double* dist /* HOST, 8 */,
                      unsigned char* dir, void* stream);
size_t smvs_dsm_flow_workspace_bytes(int gw, int gh);
int smvs_dsm_flow_accumulate(const unsigned char* dir, const int* weight /* may be null */, int gw, int gh,
                             long long* acc, int* flag, void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_flow_basins(const unsigned char* dir, const unsigned char* pour /* may be null */, int gw, int gh,
                         int* basin, int* n_out, int* flag, void* workspace, size_t workspace_bytes, void* stream);
size_t smvs_dsm_stream_workspace_bytes(int gw, int gh);
int smvs_dsm_stream_order(const unsigned char* dir, const unsigned char* mask, int gw, int gh, unsigned char* order,
                          int* link_map /* may be null */, int* counts /* device, 4 */, int* flag,
                          void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_stream_write(const unsigned char* dir, const unsigned char* mask, int gw, int gh, int n_links, int n_vertices,
                          int* head, int* link_order, int* next_link, int* offset, int* vertices, int* steps,
                          void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_flow_length(const unsigned char* dir, int gw, int gh, int* steps, int* flag,
                         void* workspace, size_t workspace_bytes, void* stream);
size_t smvs_dsm_cost_workspace_bytes(int gw, int gh);
int smvs_dsm_cost_begin(const unsigned short* friction /* may be null */, const unsigned char* sources,
                        const float* dsm /* may be null */, int gw, int gh, float nodata, unsigned long long* keys,
                        int* n_sources, void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_cost_rounds(const unsigned short* friction /* may be null */, const float* dsm /* may be null */, int gw, int gh,
                         float nodata, const int* L /* HOST, 8 */, const int* table /* HOST, 256; null iff dsm is */,
                         int reverse, unsigned long long* keys, int rounds, int* status,
                         void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_cost_read(const unsigned short* friction /* may be null */, const float* dsm /* may be null */, int gw, int gh,
                       float nodata, const int* L /* HOST, 8 */, const int* table /* HOST, 256; null iff dsm is */,
                       int reverse, const unsigned long long* keys, unsigned long long max_cost,
                       long long* raw /* may be null */, double* cost /* may be null */, unsigned char* backlink /* may be null */,
                       void* workspace, size_t workspace_bytes, void* stream);
size_t smvs_dsm_seed_workspace_bytes(int gw, int gh);
int smvs_dsm_seed_begin(const float* dsm, const float* marker, const unsigned char* domain /* may be null */, int gw, int gh,
                        float nodata, int polarity, int offset, unsigned long long* keys, int* n_seeds,
                        void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_seed_rounds(const float* dsm, int gw, int gh, float nodata, int polarity, unsigned long long* keys, int rounds,
                         int* status, void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_seed_read(const float* dsm, const float* marker, const unsigned char* domain /* may be null */, int gw, int gh,
                       float nodata, int polarity, int offset, const unsigned long long* keys,
                       float* surface /* may be null */, int* level_steps /* may be null */,
                       unsigned char* backlink /* may be null */, int* n_unreached /* may be null */,
                       void* workspace, size_t workspace_bytes, void* stream);
size_t smvs_dsm_mesh_workspace_bytes(int gw, int gh, int tile);
int smvs_dsm_mesh_errors(const float* dsm, int gw, int gh, float nodata, int tile, long long* errors, void* stream);
int smvs_dsm_mesh_count(const long long* errors, const float* dsm, int gw, int gh, float nodata, int tile, long long threshold,
                        int* counts /* device, 2 */, void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_mesh_write(const float* dsm, int gw, int gh, int tile, int n_triangles, int n_vertices, int* triangles,
                        unsigned char* tri_level, int* vertices, float* z, int* status /* device, 1 */,
                        void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_mesh_heights(const long long* errors, const float* dsm, int gw, int gh, float nodata, int tile,
                          long long threshold, float* heights, long long* dev /* may be null */,
                          void* workspace, size_t workspace_bytes, void* stream);
size_t smvs_dsm_facet_workspace_bytes(int gw, int gh);
int smvs_dsm_facet_normals(const float* dsm, const unsigned char* mask /* may be null */, int gw, int gh, float nodata, int T,
                           int* Gx, int* Gy, unsigned char* planar, void* stream);
int smvs_dsm_facet_label(const float* dsm, const unsigned char* mask /* may be null */, int gw, int gh, float nodata,
                         int T, int Ax, int Ay, int connectivity, int grow, int* labels, int* n_out /* device, 1 */,
                         void* workspace, size_t workspace_bytes, void* stream);
int smvs_dsm_facet_planes(const int* labels, const float* dsm, int gw, int gh, float nodata, int n,
                          long long* sums, int* centre, long long* moments, double* plane, long long* sse, int* max_abs,
                          void* stream);

/* ---- heights without a network: census plane sweep and semi-global matching (sgm.hip) ----------------
 * Three entries over plane-minor uint16 volumes (B, H, W, D): the D planes of a pixel are contiguous.  1 <= D <= 256 and
 * B H W D < 2^31.  Everything is integer arithmetic but the census comparisons (float32 `<`) and the sub-plane height (float64,
 * every operation rounded by itself), so every output is equal bits from run to run, on any stream, and to the numpy statement
 * of tests/sgm_oracle.py.  No atomics, no host synchronisation.
 *
 * smvs_sgm_census_cost: the matching cost of planes d_begin .. d_begin + Dc - 1 of `cost`; the other planes are left alone.
 *   ref (B, H, W) float32; warped: HOST array of n_src DEVICE pointers, each (B, 2, Dc, H, W) float32 -- what smvs_rpc_warp_fwd /
 *   smvs_homo_warp_fwd write for the 2-channel feature [grey image, ones]: channel 0 the warped image, channel 1 its coverage.
 *   The window is (2 radius + 1)^2 without its centre: 8, 24 or 48 bits.  The bit of image I at (y, x) for the offset (dy, dx)
 *   is I(y + dy, x + dx) < I(y, x) in float32 (strict, false with a NaN); an offset that leaves the H x W grid gives 0 in every
 *   image, which is the mask M of the rule.  Source s is valid at (d, y, x) iff its coverage is >= cov_min at the centre and at
 *   every window position on the grid.  ham_s = popcount(census_ref ^ census_s); with n valid sources
 *   cost = floor(16 sum_valid ham_s / n) (<= 768), and 0xFFFF ("void") with n = 0.  The census of ref is computed once per call,
 *   into the workspace (8 bytes per pixel: smvs_sgm_census_workspace_bytes(B, H, W), 0 = unsupported sizes).
 *   Limits (SMVS_ERR_ARG with a message, before any HIP call; nothing is written): non-null pointers; 1 <= n_src <= 7;
 *   radius 1, 2 or 3; cov_min not NaN; B, H, W >= 1; 1 <= D <= 256; 0 <= d_begin, 1 <= Dc, d_begin + Dc <= D; B H W D < 2^31;
 *   the workspace large enough; ref, cost, workspace and every warped volume do not overlap.
 *
 * smvs_sgm_aggregate: sum = sum over the directions r of L_r.  C'(p, d) = void_cost where cost == 0xFFFF, else
 *   min(cost, cost_max).  Directions, each with q = p - r: paths 4: (0, +-1), (+-1, 0); paths 8: those and (+-1, +-1).
 *   q off the grid: L_r(p, d) = C'(p, d).  Otherwise, with m = min_k L_r(q, k) and the d +- 1 terms only where those planes exist,
 *     L_r(p, d) = C'(p, d) + min(L_r(q, d), L_r(q, d - 1) + P1, L_r(q, d + 1) + P1, m + P2') - m
 *   P2' = P2 without a guide; with guide (B, H, W) uint8: P2' = max(p2_min, P2 - alpha |G(p) - G(q)|).
 *   The bound: by induction L_r(p, .) >= C'(p, .) >= 0 (every term of the min is >= m), and the min is <= m + P2', so
 *   L_r <= C' + P2' <= cost_max + P2.  With paths (cost_max + P2) <= 65535 neither an L_r nor the sum of all of them leaves
 *   uint16: nothing wraps and nothing saturates.
 *   Limits (SMVS_ERR_ARG): non-null cost and sum, which do not overlap each other or the guide; sizes as above; paths 4 or 8;
 *   0 <= P1 <= p2_min <= P2; 0 <= alpha <= 65535; 0 <= void_cost <= cost_max; paths (cost_max + P2) <= 65535.
 *
 * smvs_sgm_select: per pixel the winner d0 = the smallest index of the minimum of sum, a uniqueness test and a sub-plane height.
 *   depth: (B, D) or, with depth_is_4d, (B, D, H, W) float32.  support = the number of planes whose cost is not 0xFFFF.
 *   Rejected (index -1, height NaN): cost given and support < min_support; or some d with |d - d0| > 1 has
 *   sum[d] (100 - uniqueness) < sum[d0] 100 (int32).  Otherwise a, b, c = sum[d0 - 1], sum[d0], sum[d0 + 1], den = a + c - 2 b;
 *   t = 0 at an end plane or with den = 0, else t = (double)(a - c) / (double)(2 den), one IEEE division (|t| <= 1/2);
 *   height = (float)(h0 + t (h+ - h0)) for t >= 0, (float)(h0 + t (h0 - h-)) for t < 0, the operands widened to double, a
 *   difference, a product and a sum each rounded once.  A NaN height is written as the quiet NaN 0x7FC00000.
 *   min_sum = sum[d0] and support are written for every pixel, rejected or not.
 *   Limits (SMVS_ERR_ARG): non-null sum, depth, index, height; sizes as above; 0 <= uniqueness <= 99; min_support >= 0;
 *   support needs cost; no output overlaps an input or another output. */
size_t smvs_sgm_census_workspace_bytes(int B, int H, int W);
int smvs_sgm_census_cost(const float* ref, const float* const* warped /* HOST, n_src device pointers */, int n_src,
                         int radius, float cov_min, unsigned short* cost, int B, int H, int W, int d_begin, int Dc, int D,
                         void* workspace, size_t workspace_bytes, void* stream);
int smvs_sgm_aggregate(const unsigned short* cost, const unsigned char* guide /* may be NULL */, unsigned short* sum,
                       int B, int H, int W, int D, int P1, int P2, int p2_min, int alpha, int cost_max, int void_cost,
                       int paths, void* stream);
int smvs_sgm_select(const unsigned short* sum, const unsigned short* cost /* may be NULL */, const float* depth, int depth_is_4d,
                    int uniqueness, int min_support, int* index, float* height, unsigned short* min_sum /* may be NULL */,
                    unsigned short* support /* may be NULL */, int B, int H, int W, int D, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SATMVS_H */
