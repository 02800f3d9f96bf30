// dsm_render.hip -- from a DSM back to the views: ray marching through the bilinear surface of a height grid.
//
//   smvs_rpc_dsm_render  one lane per pixel of a view marches its ray (x, y, h) down through the bilinear surface of a DSM, then
//                     bisects the crossing; the first crossing from above is the pixel's height.
//   smvs_rpc_ortho    the orthophoto: one lane per DSM cell projects the cell's point into a view, marches the ray up to test
//                     occlusion, and samples the image bilinearly; a mosaic fills each cell from the first view that sees it.
//
// The projection, the grid and the surface come from dsm_geo.h, which dsm.hip (the forward direction: views -> DSM) shares.
#include <algorithm>

#include "dsm_geo.h"
#include "smvs_device.h"
#include "smvs_host.h"

namespace smvs {

// ---- render pass: DSM -> one view's image-space heights (include/satmvs.h) -----------------------------
constexpr int RENDER_TILE = 16;                      // 16 x 16 pixels per workgroup: each wave covers 16 columns x 4 rows
constexpr unsigned RENDER_MAX_BLOCKS = 1u << 20;     // grid-stride over tiles beyond this

// One lane per pixel.  The march (h_k = h_hi - k (h_hi - h_lo) / K, h_K = h_lo; first k with f(h_k) = S(G(h_k)) - h_k defined and >= 0)
// and the bisection of [h_k, h_{k-1}] run as ONE loop whose body is one evaluation photo2obj -> TM -> bilinear; the lane's
// state picks the next height, so lanes in different phases share the body instead of running it twice under divergence.
__global__ __launch_bounds__(RENDER_TILE * RENDER_TILE)
void dsm_render_kernel(const float* __restrict__ z, int gw, int gh, DsmGrid g, float nodata, TmConst t,
                       const double* __restrict__ rpc, int H, int W, int x0, int y0, double h_lo, double h_hi, double tol,
                       float* __restrict__ out)
{
    const unsigned nbx = (unsigned)(W + RENDER_TILE - 1) / RENDER_TILE, nby = (unsigned)(H + RENDER_TILE - 1) / RENDER_TILE;
    const unsigned ntiles = nbx * nby;
    const cgeo_t r = as_cgeo(rpc);
    const RpcInv rn = rpc_inv_image(r);
    for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int j = (int)(tile % nbx) * RENDER_TILE + (int)(threadIdx.x % RENDER_TILE);
        const int i = (int)(tile / nbx) * RENDER_TILE + (int)(threadIdx.x / RENDER_TILE);
        if (i >= H || j >= W) continue;
        const double x = (double)(x0 + j), y = (double)(y0 + i);
        double lat, lon, E_lo, N_lo;
        rpc_photo2obj(launder(r), rn, x, y, h_lo, lat, lon);
        tm_forward(t, lat, lon, E_lo, N_lo);
        double h = h_hi, h_prev = h_hi, a = 0.0, b = 0.0, step = 0.0;
        int k = 0, K = 1, left = -1;                 // left < 0: marching; else bisection steps still to take
        bool prev_ok = false;
        float res = __builtin_nanf("");
        for (;;) {
            double E, N, S;
            rpc_photo2obj(launder(r), rn, x, y, h, lat, lon);
            tm_forward(t, lat, lon, E, N);
            const bool ok = dsm_surface(z, gw, gh, nodata, g, E, N, S);
            const bool below = ok && S - h >= 0.0;   // f(h) defined and >= 0
            if (left < 0) {
                if (k == 0) {
                    K = render_march_steps(g, E, N, E_lo, N_lo);
                    step = (h_hi - h_lo) / (double)K;
                }
                if (!below) {
                    if (k == K) break;               // no sample qualifies: invalid
                    prev_ok = ok;
                    h_prev = h;
                    ++k;
                    h = (k == K) ? h_lo : h_hi - (double)k * step;     // the last sample is h_lo exactly, whatever the rounding
                    continue;
                }
                if (k == 0) { res = (float)h_hi; break; }
                if (!prev_ok) break;                 // came out of a hole or off the grid: invalid
                a = h;
                b = h_prev;
                left = render_bisect_steps(step, tol);
            } else {
                if (!ok) break;                      // a midpoint where f is undefined: invalid
                if (below) a = h;
                else b = h;
                --left;
            }
            if (left == 0) { res = (float)(0.5 * (a + b)); break; }
            h = 0.5 * (a + b);
        }
        out[(size_t)i * W + j] = res;
    }
}

// ---- orthophoto pass: one view's image resampled onto the DSM grid, with occlusion (include/satmvs.h) --
constexpr int ORTHO_MAX_CHANNELS = 16;
enum : unsigned char { ORTHO_NO_HEIGHT = 0, ORTHO_OUTSIDE = 1, ORTHO_OCCLUDED = 2, ORTHO_VISIBLE = 3 };

// Whether the ray up from the cell's point (x, y, zc) passes under the surface: samples h_k = zc + k (h_hi - zc) / K,
// k = 1 .. K - 1, and h_K = h_hi exactly, K from the travel between G(zc) and G(h_hi) as in the render.  A sample occludes where
// f(h_k) = S(G(h_k)) - h_k is defined and > occ_tol; undefined samples (holes, off the grid) do not.  ONE loop whose body is one
// evaluation photo2obj -> TM -> bilinear, as in the render: G(zc) first (only for K), then h_K = h_hi (its G sets K; the order
// of the samples does not change whether one of them occludes), then h_1 .. h_{K-1}.
__device__ __forceinline__ bool ortho_occluded(const float* __restrict__ z, int gw, int gh, float nodata, const DsmGrid& g,
                                               const TmConst& t, cgeo_t r, const RpcInv& rn, double x, double y, double zc,
                                               double h_hi, double occ_tol)
{
    if (!(zc < h_hi)) return false;
    double h = zc, E_z = 0.0, N_z = 0.0, step = 0.0;
    int k = -1, K = 1;                               // k = -1: G(zc); k = 0: h_K; then k = 1 .. K - 1, K <= RENDER_MAX_STEPS
    for (;;) {
        double lat, lon, E, N, S;
        rpc_photo2obj(launder(r), rn, x, y, h, lat, lon);
        tm_forward(t, lat, lon, E, N);
        if (k < 0) {
            E_z = E;
            N_z = N;
            k = 0;
            h = h_hi;
            continue;
        }
        if (dsm_surface(z, gw, gh, nodata, g, E, N, S) && S - h > occ_tol) return true;
        if (k == 0) {
            K = render_march_steps(g, E, N, E_z, N_z);
            step = (h_hi - zc) / (double)K;
        }
        if (++k >= K) return false;
        h = zc + (double)k * step;
    }
}

// One lane per DSM cell, 16 x 16-cell workgroups (neighbouring rays read the same DSM lines), grid-stride past
// RENDER_MAX_BLOCKS.  Height -> TM inverse -> rpc_obj2photo -> bounds -> occlusion march -> bilinear image sample; ortho and
// source are written where the cell is visible and source < 0 on entry.  Without a state map, cells already filled by an
// earlier view are skipped whole.
__global__ __launch_bounds__(RENDER_TILE * RENDER_TILE)
void dsm_ortho_kernel(const float* __restrict__ z, int gw, int gh, DsmGrid g, float nodata, TmConst t,
                      const double* __restrict__ rpc, const float* __restrict__ image, int H, int W, int C, int x0, int y0,
                      double h_hi, int occlusion, double occ_tol, int view,
                      float* __restrict__ ortho, int* __restrict__ source, unsigned char* __restrict__ state)
{
    const unsigned nbx = (unsigned)(gw + RENDER_TILE - 1) / RENDER_TILE, nby = (unsigned)(gh + RENDER_TILE - 1) / RENDER_TILE;
    const unsigned ntiles = nbx * nby;
    const cgeo_t r = as_cgeo(rpc);
    const RpcInv rg = rpc_inv_ground(r), ri = rpc_inv_image(r);
    for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int c = (int)(tile % nbx) * RENDER_TILE + (int)(threadIdx.x % RENDER_TILE);
        const int row = (int)(tile / nbx) * RENDER_TILE + (int)(threadIdx.x / RENDER_TILE);
        if (row >= gh || c >= gw) continue;
        const size_t cell = (size_t)row * gw + c;
        if (!state && source[cell] >= 0) continue;   // filled by an earlier view; nothing else to write
        const float zf = z[cell];
        unsigned char st = ORTHO_NO_HEIGHT;
        double u = 0.0, v = 0.0;
        if (dsm_cell_valid(zf, nodata)) {
            const double E = g.e0 + (double)c * g.xres, N = g.n0 - (double)row * g.yres;
            double lat, lon, x, y;
            tm_inverse(t, E, N, lat, lon);
            rpc_obj2photo(launder(r), rg, lat, lon, (double)zf, x, y);
            u = x - (double)x0;
            v = y - (double)y0;
            if (!(u >= 0.0 && u <= (double)(W - 1) && v >= 0.0 && v <= (double)(H - 1))) st = ORTHO_OUTSIDE;   // NaN fails
            else if (occlusion && ortho_occluded(z, gw, gh, nodata, g, t, r, ri, x, y, (double)zf, h_hi, occ_tol)) st = ORTHO_OCCLUDED;
            else st = ORTHO_VISIBLE;
        }
        if (state) state[cell] = st;
        if (st != ORTHO_VISIBLE || !source || source[cell] >= 0) continue;
        if (ortho) {
            // pixel centres on integers; the last column / row is reached with du = 1 (dv = 1) from the one before it
            const int c0 = W > 1 ? min((int)floor(u), W - 2) : 0, r0 = H > 1 ? min((int)floor(v), H - 2) : 0;
            const int c1 = W > 1 ? c0 + 1 : 0, r1 = H > 1 ? r0 + 1 : 0;
            const double du = W > 1 ? u - (double)c0 : 0.0, dv = H > 1 ? v - (double)r0 : 0.0;
            const float* p00 = image + ((size_t)r0 * W + c0) * C;
            const float* p01 = image + ((size_t)r0 * W + c1) * C;
            const float* p10 = image + ((size_t)r1 * W + c0) * C;
            const float* p11 = image + ((size_t)r1 * W + c1) * C;
            float* o = ortho + cell * C;
            for (int ch = 0; ch < ORTHO_MAX_CHANNELS && ch < C; ++ch) {
                const double a = (double)p00[ch] + du * ((double)p01[ch] - (double)p00[ch]);
                const double b = (double)p10[ch] + du * ((double)p11[ch] - (double)p10[ch]);
                o[ch] = (float)(a + dv * (b - a));
            }
        }
        source[cell] = view;
    }
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT int smvs_rpc_dsm_render(const float* dsm, int gw, int gh, const double* grid4, float nodata, const double* tm7,
                                    const double* rpc170, int H, int W, int x0, int y0, double h_lo, double h_hi, double tol,
                                    float* height, void* stream)
{
    using namespace smvs;
    if (!dsm || !grid4 || !tm7 || !rpc170 || !height) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = tile_check(H, W, x0, y0, gw, gh)) return fail(SMVS_ERR_ARG, "%s", msg);
    DsmGrid g;
    if (const char* msg = dsm_grid_parse(grid4, g)) return fail(SMVS_ERR_ARG, "%s", msg);
    TmConst t;
    if (const char* msg = tm_parse(tm7, t)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (!isfinite(h_lo) || !isfinite(h_hi) || !(h_lo <= h_hi)) return fail(SMVS_ERR_ARG, "height bracket: h_lo <= h_hi, both finite");
    if (!(tol > 0.0) || !isfinite(tol)) return fail(SMVS_ERR_ARG, "tol must be positive and finite");
    const unsigned ntiles = (unsigned)((W + RENDER_TILE - 1) / RENDER_TILE) * (unsigned)((H + RENDER_TILE - 1) / RENDER_TILE);
    hipLaunchKernelGGL(dsm_render_kernel, dim3(std::min(ntiles, RENDER_MAX_BLOCKS)), dim3(RENDER_TILE * RENDER_TILE), 0,
                       (hipStream_t)stream, dsm, gw, gh, g, nodata, t, rpc170, H, W, x0, y0, h_lo, h_hi, tol, height);
    return check_launch("dsm_render");
}

SMVS_EXPORT int smvs_rpc_ortho(const float* dsm, int gw, int gh, const double* grid4, float nodata, const double* tm7,
                               const double* rpc170, const float* image, int H, int W, int C, int x0, int y0,
                               double h_hi, int occlusion, double occ_tol, int view,
                               float* ortho, int* source, unsigned char* state, void* stream)
{
    using namespace smvs;
    if (!dsm || !grid4 || !tm7 || !rpc170) return fail(SMVS_ERR_ARG, "null pointer argument");
    if ((image == nullptr) != (ortho == nullptr)) return fail(SMVS_ERR_ARG, "null pointer argument: image and ortho go together");
    if (ortho && !source) return fail(SMVS_ERR_ARG, "null pointer argument: ortho needs source (the mosaic rule reads it)");
    if (!source && !state) return fail(SMVS_ERR_ARG, "null pointer argument: nothing to write (give source or state)");
    if (C < 1 || C > ORTHO_MAX_CHANNELS) return fail(SMVS_ERR_ARG, "channel count C must be in 1 .. %d", ORTHO_MAX_CHANNELS);
    if (const char* msg = tile_check(H, W, x0, y0, gw, gh)) return fail(SMVS_ERR_ARG, "%s", msg);
    DsmGrid g;
    if (const char* msg = dsm_grid_parse(grid4, g)) return fail(SMVS_ERR_ARG, "%s", msg);
    TmConst t;
    if (const char* msg = tm_parse(tm7, t)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (!isfinite(h_hi)) return fail(SMVS_ERR_ARG, "h_hi must be finite");
    if (!(occ_tol >= 0.0) || !isfinite(occ_tol)) return fail(SMVS_ERR_ARG, "occ_tol must be finite and >= 0");
    if (view < 0) return fail(SMVS_ERR_ARG, "view must be non-negative");
    const unsigned ntiles = (unsigned)((gw + RENDER_TILE - 1) / RENDER_TILE) * (unsigned)((gh + RENDER_TILE - 1) / RENDER_TILE);
    hipLaunchKernelGGL(dsm_ortho_kernel, dim3(std::min(ntiles, RENDER_MAX_BLOCKS)), dim3(RENDER_TILE * RENDER_TILE), 0,
                       (hipStream_t)stream, dsm, gw, gh, g, nodata, t, rpc170, image, H, W, C, x0, y0, h_hi, occlusion, occ_tol,
                       view, ortho, source, state);
    return check_launch("dsm_ortho");
}

}  // extern "C"
