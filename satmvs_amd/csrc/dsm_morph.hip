// dsm_morph.hip -- grey-scale morphology on a DSM and the progressive morphological ground filter built on it (DESIGN.md
// section 9, "Ground extraction"; include/satmvs.h for the rules).
//
//   smvs_dsm_morph   erode / dilate / open / close with a (2 radius + 1)^2 square clipped at the grid border; invalid cells are
//                    transparent.
//   smvs_dsm_ground  openings with growing radii; a valid cell that an opening lowers by more than the level's threshold is
//                    classed "removed at that level"; the DTM keeps the ground cells.
//
// Everything is a maximum of order-preserving uint32 keys (dsm_common.h f2key) with key 0 = "invalid / none", the identity
// of max: a dilation takes the keys as they are, an erosion their complements (~key of a valid key is never 0).  A square
// window is a row pass followed by a column pass, so every operation is a chain of line passes by ONE kernel: a workgroup
// stages a piece of NL lines with a halo of `radius` cells at both ends in LDS, builds M[i] = max over [i, i + 2^j) by j
// doubling steps (2^j <= window < 2^(j+1)) and writes max(M[p - radius], M[p + radius + 1 - 2^j]) for every cell p of the
// piece.  No step depends on the order of anything: bit-identical from run to run and to the numpy statement.  No atomics.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "dsm_common.h"
#include "smvs_host.h"

namespace smvs {

constexpr int MORPH_THREADS = 256, MORPH_THREADS_LARGE = 1024;       // the 128 KiB piece is alone on its CU: 16 waves hide its LDS latency
constexpr int MORPH_MAX_RADIUS = 256, MORPH_MAX_LEVELS = 16;
constexpr int MORPH_PLANES = 3;                      // two ping-pong key planes and the filter's surface S_k

// What a pass reads (how a cell becomes a key) and what it writes.
enum { MORPH_IN_FLOAT = 0, MORPH_IN_FLOAT_INV = 1, MORPH_IN_KEY = 2, MORPH_IN_KEY_INV = 3 };
enum { MORPH_OUT_KEY = 0, MORPH_OUT_FLOAT = 1, MORPH_OUT_FLOAT_INV = 2, MORPH_OUT_GROUND = 3 };

struct MorphPass {
    const float* dsm;            // the float32 input grid (MORPH_IN_FLOAT*, and the cells every float / ground output copies)
    const unsigned* kin;         // MORPH_IN_KEY*: the key plane read
    unsigned* kout;              // MORPH_OUT_KEY: the key plane written
    float* fout;                 // MORPH_OUT_FLOAT*: the result grid; MORPH_OUT_GROUND with `last`: the DTM
    unsigned* surf;              // MORPH_OUT_GROUND: S_k as keys, read (unless `first`) and replaced by S_(k+1) at the lane's own cell
    unsigned char* cls;          // MORPH_OUT_GROUND: the classes, read (unless `first`) and written at the lane's own cell
    double thresh;               // MORPH_OUT_GROUND: t_k
    int gw, gh;
    float nodata;
    int radius, w2, seg;         // w2 = 2^j <= 2 radius + 1; seg = cells of a line that one workgroup writes
    int in_mode, out_mode;
    int level, first, last;      // MORPH_OUT_GROUND: k, k == 0, k == K - 1
};

__device__ __forceinline__ unsigned morph_flip(unsigned k) { return k ? ~k : 0u; }

// One line pass.  COLS: the lines are columns (NL consecutive columns per workgroup, so a row of the piece is NL consecutive
// floats), else rows (NL = 1).  The piece lives in LDS as [position along the line][line], and the doubling and the output
// only shift flat indices by multiples of NL, so consecutive lanes are on consecutive banks in both directions.
// CELLS >= (seg + 2 radius) NL is the host's duty (morph_launch).
template <int NL, int CELLS, bool COLS, int THREADS>
__global__ __launch_bounds__(THREADS)
void dsm_morph_pass(const MorphPass a)
{
    __shared__ unsigned buf[2][CELLS];
    const int gw = a.gw, gh = a.gh, r = a.radius;
    const int len = COLS ? gh : gw, nlines = COLS ? gw : gh;
    const unsigned nseg = (unsigned)((len + a.seg - 1) / a.seg);
    const int line0 = (int)(blockIdx.x / nseg) * NL, p0 = (int)(blockIdx.x % nseg) * a.seg;
    const int nout = min(a.seg, len - p0);
    const int n = (nout + 2 * r) * NL;                       // staged cells: positions p0 - r .. p0 + nout + r - 1
    for (int i = threadIdx.x; i < n; i += THREADS) {
        const int ln = line0 + i % NL, p = p0 - r + i / NL;
        unsigned k = 0u;
        if (ln < nlines && p >= 0 && p < len) {
            const size_t cell = COLS ? (size_t)p * gw + ln : (size_t)ln * gw + p;
            if (a.in_mode >= MORPH_IN_KEY) {
                k = a.kin[cell];
                if (a.in_mode == MORPH_IN_KEY_INV) k = morph_flip(k);
            } else {
                const float z = a.dsm[cell];
                if (dsm_cell_valid(z, a.nodata)) k = a.in_mode == MORPH_IN_FLOAT_INV ? ~f2key(z) : f2key(z);
            }
        }
        buf[0][i] = k;
    }
    __syncthreads();
    int cur = 0;
    for (int s = 1; s < a.w2; s <<= 1) {                     // [i, i + s) -> [i, i + 2 s); runs cut short by the end are never used
        for (int i = threadIdx.x; i < n; i += THREADS) {
            unsigned v = buf[cur][i];
            const int q = i + s * NL;
            if (q < n) v = max(v, buf[cur][q]);
            buf[cur ^ 1][i] = v;
        }
        __syncthreads();
        cur ^= 1;
    }
    const int second = (2 * r + 1 - a.w2) * NL;              // the two runs of w2 cells that cover the window of 2 r + 1
    for (int i = threadIdx.x; i < nout * NL; i += THREADS) {
        const int ln = line0 + i % NL, p = p0 + i / NL;
        if (ln >= nlines) continue;
        const unsigned v = max(buf[cur][i], buf[cur][i + second]);
        const size_t cell = COLS ? (size_t)p * gw + ln : (size_t)ln * gw + p;
        if (a.out_mode == MORPH_OUT_KEY) {
            a.kout[cell] = v;
        } else if (a.out_mode != MORPH_OUT_GROUND) {         // a valid cell has itself in its window, so v != 0 there
            const float z = a.dsm[cell];
            a.fout[cell] = dsm_cell_valid(z, a.nodata) ? key2f(a.out_mode == MORPH_OUT_FLOAT_INV ? ~v : v) : z;
        } else {
            const float z = a.dsm[cell];
            unsigned sk;
            unsigned char c;
            if (a.first) {
                sk = dsm_cell_valid(z, a.nodata) ? f2key(z) : 0u;
                c = sk ? 1 : 0;
            } else {
                sk = a.surf[cell];
                c = a.cls[cell];
            }
            if (c == 1 && (double)key2f(sk) - (double)key2f(v) > a.thresh) c = (unsigned char)(2 + a.level);
            a.surf[cell] = sk ? v : 0u;                      // S_(k+1) = O_k at valid cells; invalid cells stay transparent
            a.cls[cell] = c;
            if (a.last) a.fout[cell] = c >= 2 ? a.nodata : z;
        }
    }
}

// Piece sizes.  Rows: one row, up to 2048 + 2 radius cells (20 KiB of LDS).  Columns: 16 columns (64 contiguous bytes per
// row of the piece); 256 rows (32 KiB) up to radius 64, 1024 rows (128 KiB, one workgroup of 1024 threads per CU) beyond.
constexpr int MORPH_ROW_CELLS = 2048 + 2 * MORPH_MAX_RADIUS;
constexpr int MORPH_COL_NL = 16, MORPH_COL_SMALL = 256, MORPH_COL_LARGE = 1024, MORPH_COL_SMALL_RADIUS = 64;

static int morph_launch(MorphPass a, bool cols, hipStream_t s)
{
    const int w = 2 * a.radius + 1;
    a.w2 = 1;
    while (a.w2 * 2 <= w) a.w2 *= 2;
    if (!cols) {
        a.seg = MORPH_ROW_CELLS - 2 * a.radius;
        const unsigned nseg = (unsigned)((a.gw + a.seg - 1) / a.seg);
        hipLaunchKernelGGL((dsm_morph_pass<1, MORPH_ROW_CELLS, false, MORPH_THREADS>), dim3(nseg * (unsigned)a.gh), dim3(MORPH_THREADS), 0, s, a);
        return check_launch("dsm_morph_pass (rows)");
    }
    const bool small = a.radius <= MORPH_COL_SMALL_RADIUS;
    a.seg = (small ? MORPH_COL_SMALL : MORPH_COL_LARGE) - 2 * a.radius;
    const unsigned nseg = (unsigned)((a.gh + a.seg - 1) / a.seg);
    const dim3 grid(nseg * (unsigned)((a.gw + MORPH_COL_NL - 1) / MORPH_COL_NL));
    if (small) hipLaunchKernelGGL((dsm_morph_pass<MORPH_COL_NL, MORPH_COL_SMALL * MORPH_COL_NL, true, MORPH_THREADS>), grid, dim3(MORPH_THREADS), 0, s, a);
    else hipLaunchKernelGGL((dsm_morph_pass<MORPH_COL_NL, MORPH_COL_LARGE * MORPH_COL_NL, true, MORPH_THREADS_LARGE>), grid, dim3(MORPH_THREADS_LARGE), 0, s, a);
    return check_launch("dsm_morph_pass (columns)");
}

// The four passes of an opening of the surface `in_mode` describes (a closing with the complements swapped): rows and columns
// of the erosion into planes, the dilation's columns, and its rows into whatever `last` asks for.  An erosion or a dilation
// alone is the first two with the output on the second.
static int morph_chain(MorphPass base, int op, unsigned* p1, unsigned* p2, const MorphPass& last, hipStream_t s)
{
    int rc;
    MorphPass a = base;
    a.out_mode = MORPH_OUT_KEY;
    a.kout = p1;
    if ((rc = morph_launch(a, false, s))) return rc;
    a.in_mode = MORPH_IN_KEY;
    a.kin = p1;
    if (op < 2) {
        MorphPass b = last;
        b.in_mode = MORPH_IN_KEY;
        b.kin = p1;
        return morph_launch(b, true, s);
    }
    a.kout = p2;
    if ((rc = morph_launch(a, true, s))) return rc;
    a.in_mode = MORPH_IN_KEY_INV;
    a.kin = p2;
    a.kout = p1;
    if ((rc = morph_launch(a, true, s))) return rc;
    MorphPass b = last;
    b.in_mode = MORPH_IN_KEY;
    b.kin = p1;
    return morph_launch(b, false, s);
}

}  // namespace smvs

extern "C" {

SMVS_EXPORT size_t smvs_dsm_morph_workspace_bytes(int gw, int gh, int max_radius)
{
    using namespace smvs;
    if (grid_check(gw, gh) || max_radius < 1 || max_radius > MORPH_MAX_RADIUS) return 0;
    return MORPH_PLANES * align256((size_t)gw * gh * sizeof(unsigned));
}

SMVS_EXPORT int smvs_dsm_morph(const float* dsm, int gw, int gh, float nodata, int radius, int op, float* out,
                               void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!dsm || !out || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (radius < 1 || radius > MORPH_MAX_RADIUS) return fail(SMVS_ERR_ARG, "radius must be in 1 .. %d", MORPH_MAX_RADIUS);
    if (op < 0 || op > 3) return fail(SMVS_ERR_ARG, "op must be 0 (erode), 1 (dilate), 2 (open) or 3 (close)");
    const size_t ncells = (size_t)gw * gh;
    if (dsm_overlap(dsm, ncells * 4, out, ncells * 4)) return fail(SMVS_ERR_ARG, "out aliases dsm: the operation is out of place");
    const size_t need = smvs_dsm_morph_workspace_bytes(gw, gh, radius);
    if (workspace_bytes < need) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    if (dsm_overlap(dsm, ncells * 4, workspace, need) || dsm_overlap(out, ncells * 4, workspace, need))
        return fail(SMVS_ERR_ARG, "workspace aliases dsm or out");
    const size_t plane = need / MORPH_PLANES / sizeof(unsigned);
    unsigned* p1 = (unsigned*)workspace;
    MorphPass a = {};
    a.dsm = dsm;
    a.gw = gw;
    a.gh = gh;
    a.nodata = nodata;
    a.radius = radius;
    const bool erode_first = op == 0 || op == 2;
    a.in_mode = erode_first ? MORPH_IN_FLOAT_INV : MORPH_IN_FLOAT;
    MorphPass last = a;
    last.fout = out;
    // the last pass of an erosion or a closing leaves complements, that of a dilation or an opening the keys themselves
    last.out_mode = (op == 0 || op == 3) ? MORPH_OUT_FLOAT_INV : MORPH_OUT_FLOAT;
    return morph_chain(a, op, p1, p1 + plane, last, (hipStream_t)stream);
}

SMVS_EXPORT int smvs_dsm_ground(const float* dsm, int gw, int gh, float nodata, const int* radii, const double* thresholds,
                                int n_levels, float* dtm, unsigned char* cls, void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace smvs;
    if (!dsm || !radii || !thresholds || !dtm || !cls || !workspace) return fail(SMVS_ERR_ARG, "null pointer argument");
    if (const char* msg = grid_check(gw, gh)) return fail(SMVS_ERR_ARG, "%s", msg);
    if (n_levels < 1 || n_levels > MORPH_MAX_LEVELS) return fail(SMVS_ERR_ARG, "n_levels must be in 1 .. %d", MORPH_MAX_LEVELS);
    for (int k = 0; k < n_levels; ++k) {
        if (radii[k] < 1 || radii[k] > MORPH_MAX_RADIUS) return fail(SMVS_ERR_ARG, "radii[%d] must be in 1 .. %d", k, MORPH_MAX_RADIUS);
        if (k && radii[k] <= radii[k - 1]) return fail(SMVS_ERR_ARG, "radii must be strictly increasing");
        if (!(thresholds[k] >= 0.0) || !isfinite(thresholds[k])) return fail(SMVS_ERR_ARG, "thresholds[%d] must be finite and >= 0", k);
    }
    const size_t ncells = (size_t)gw * gh;
    if (dsm_overlap(dsm, ncells * 4, dtm, ncells * 4)) return fail(SMVS_ERR_ARG, "dtm aliases dsm: the operation is out of place");
    if (dsm_overlap(dsm, ncells * 4, cls, ncells) || dsm_overlap(dtm, ncells * 4, cls, ncells)) return fail(SMVS_ERR_ARG, "cls aliases dsm or dtm");
    const size_t need = smvs_dsm_morph_workspace_bytes(gw, gh, radii[n_levels - 1]);
    if (workspace_bytes < need) return fail(SMVS_ERR_ARG, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    if (dsm_overlap(dsm, ncells * 4, workspace, need) || dsm_overlap(dtm, ncells * 4, workspace, need) || dsm_overlap(cls, ncells, workspace, need))
        return fail(SMVS_ERR_ARG, "workspace aliases dsm, dtm or cls");
    const size_t plane = need / MORPH_PLANES / sizeof(unsigned);
    unsigned* p1 = (unsigned*)workspace;
    unsigned* surf = p1 + 2 * plane;
    for (int k = 0; k < n_levels; ++k) {                     // one stream, no host synchronisation between the levels
        MorphPass a = {};
        a.dsm = dsm;
        a.gw = gw;
        a.gh = gh;
        a.nodata = nodata;
        a.radius = radii[k];
        a.in_mode = k == 0 ? MORPH_IN_FLOAT_INV : MORPH_IN_KEY_INV;      // S_0 is the input, S_k the surface plane
        a.kin = surf;
        MorphPass last = a;
        last.out_mode = MORPH_OUT_GROUND;
        last.fout = dtm;
        last.surf = surf;
        last.cls = cls;
        last.thresh = thresholds[k];
        last.level = k;
        last.first = k == 0;
        last.last = k == n_levels - 1;
        if (int rc = morph_chain(a, 2, p1, p1 + plane, last, (hipStream_t)stream)) return rc;
    }
    return SMVS_OK;
}

}  // extern "C"
