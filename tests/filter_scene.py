"""Scenes, stage oracles and parity checks for the geometric-consistency filters (csrc/filter.hip) -- numpy only, shared by
tests/test_filter_cpu.py, tests/test_filter_gpu.py and tests/fuzz/fuzz_filter.py.

Scenes: V views of ONE smooth surface, each with its own (H_v, W_v); every view's map solves "the point this pixel sees
lies on the surface" by fixed-point iteration in float64 until the change is below 1e-6, so the maps are mutually
consistent by construction.  A blunder patch in the last view and a low-confidence corner make both mask values occur.

Checks (each returns a list of messages, empty = passed; `orc` is oracle.oracle, `mod` is satmvs_amd.rpc_filter /
pinhole_filter, or the oracle itself for the CPU tests):
  stages(...)      every stage of reproject_with_depth / check_geometric_consistency against the oracle applied to the
                   implementation's OWN output of the stage before, so no rounding boundary can excuse a difference;
  end_to_end(...)  implementation against oracle from the same inputs: a pixel may differ only if it is AT RISK, i.e. if
                   moving the oracle's source coordinate by the stage-1 bound changes its fixed-point (sx, sy).
Bounds: coordinates 1e-8 px (RPC, float64) resp. one float32 ulp (pinhole); the remap's weights are multiples of 1/1024,
exact in float32, so two evaluations differ only in how four products are summed (contracted or not):
|difference| <= 8 * 2^-24 * max|tap|, border taps counted; back-projection 1e-6 px (RPC), 5e-4 px or one float32 ulp of the
result (pinhole, where the sample is finite and positive); the mask rule is equal except within 4 ulp of a threshold."""
import functools

import numpy as np

from satmvs_amd import rpc_synth

SIZES = ((1, 1), (1, 70), (67, 3), (64, 96), (255, 257), (257, 301), (384, 768))
# (reference, source) pairs of the shape matrix: a same-size source for every size, a smaller and a larger source (neither
# dimension equal to the reference's) for three of them
PAIRS = tuple((s, s) for s in SIZES) + (((64, 96), (40, 61)), ((64, 96), (90, 131)), ((255, 257), (131, 180)),
                                         ((255, 257), (300, 333)), ((1, 70), (5, 33)), ((67, 3), (80, 9)))
BIG = ((2048, 2304), (2048, 2304))
RPC_CAP, PIN_CAP = 1e-3, 2e-3                # the project's caps on the share of pixels on a 1/32-px rounding boundary
RPC_PARAMS, PIN_PARAMS = (1.0, 2.5), (1.0, 0.01)
_TILTS = (0.0, 0.05, -0.05, 0.08, -0.08, 0.03, -0.03)
_LAT0, _LON0 = 30.0, 114.0
_F32, _EPS32 = np.float32, 2.0 ** -24


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def rpc_surface(lat, lon):
    """h = f(lat, lon) [m]: a smooth surface with wavelengths of a few kilometres, the same for every view size."""
    y = (np.asarray(lat, np.float64) - _LAT0) * 111320.0
    x = (np.asarray(lon, np.float64) - _LON0) * 111320.0 * np.cos(np.deg2rad(_LAT0))
    return 200.0 + 30.0 * np.sin(x / 400.0 + 0.2) * np.cos(y / 330.0 - 0.4)


def rpc_heights(rpc, H, W, tol=1e-6, max_iter=60, rows=256):
    """The float64 height map of one view: h = f(photo2obj(x, y, h)) per pixel, iterated until the change is below tol."""
    out = np.empty((H, W))
    for r0 in range(0, H, rows):
        yy, xx = np.meshgrid(np.arange(r0, min(H, r0 + rows), dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        h = np.full(yy.shape, 200.0)
        for _ in range(max_iter):
            lat, lon = rpc_synth.photo2obj(rpc, xx, yy, h)
            new = rpc_surface(lat, lon)
            delta = np.abs(new - h).max()
            h = new
            if delta < tol:
                break
        else:
            raise RuntimeError("the height iteration did not converge (last change %g m)" % delta)
        out[r0:r0 + rows] = h
    return out


def rpc_residual(rpc, h):
    """|h - f(photo2obj(x, y, h))| per pixel [m]."""
    H, W = h.shape
    res = np.empty((H, W))
    for r0 in range(0, H, 256):
        yy, xx = np.meshgrid(np.arange(r0, min(H, r0 + 256), dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        lat, lon = rpc_synth.photo2obj(rpc, xx, yy, h[r0:r0 + 256])
        res[r0:r0 + 256] = np.abs(rpc_surface(lat, lon) - h[r0:r0 + 256])
    return res


def patch(H, W):
    """The blunder patch of an (H, W) map (empty for the degenerate sizes)."""
    return slice(H // 6, H // 3), slice(W // 3, W // 2)


@functools.lru_cache(maxsize=64)
def _rpc_view(H, W, seed, v, lon0):
    rpc = rpc_synth.make_view_rpcs(1, H, W, seed=seed * 16 + v, tilts=(_TILTS[v % len(_TILTS)],), lat0=_LAT0, lon0=lon0)[0]
    return rpc, rpc_heights(rpc, H, W)


def rpc_scene(sizes, seed=0, blunder=7.3, away=False):
    """-> (depths: list of float32 (H_v, W_v), rpcs (V, 170) float64, prob float32 (H_0, W_0), float64 maps).  View 0 is the
    reference.  blunder [m] is added to a patch of the last view; prob has a low-confidence corner.  away=True moves the last
    view half a degree east, so it does not overlap the reference at all."""
    V = len(sizes)
    views = [_rpc_view(H, W, seed, v, _LON0 + (0.5 if away and v == V - 1 else 0.0)) for v, (H, W) in enumerate(sizes)]
    depths = [h.astype(np.float32) for _, h in views]
    if blunder:
        depths[V - 1][patch(*sizes[V - 1])] += np.float32(blunder)
    H, W = sizes[0]
    prob = np.random.default_rng(seed).uniform(0.2, 1.0, (H, W)).astype(np.float32)
    prob[:H // 8, :W // 8] = 0.05
    return depths, np.stack([r for r, _ in views]), prob, [h for _, h in views]


def pin_surface(X, Y):
    return 6.0 * np.sin(0.012 * X + 0.5) * np.cos(0.010 * Y - 0.1) + 2.0 * np.sin(0.03 * X - 0.01 * Y)


def _proj(K, E):
    return np.concatenate((np.matmul(np.asarray(K, np.float64), np.asarray(E, np.float64)[:3]), np.array([[0.0, 0.0, 0.0, 1.0]])), axis=0)


@functools.lru_cache(maxsize=64)
def _pin_view(H, W, H0, W0, seed, v, away):
    rng = np.random.default_rng(seed * 16 + v)
    f = 1.15 * max(W0, 64)                         # from the reference's width for every view: one ground resolution
    near = min(1.0, W0 / 96.0, H0 / 64.0)          # the degenerate sizes move their cameras less, so that the views still overlap
    K = np.array([[f, 0.0, W / 2.0 + 0.5 * v], [0.0, f, H / 2.0 - 0.25 * v], [0.0, 0.0, 1.0]])
    a = 0.03 * v * (-1) ** v + (rng.normal(0.0, 0.01) if v else 0.0)
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]) @ np.diag([1.0, -1.0, -1.0])
    C = np.array([18.0 * v * (-1) ** v, 7.0 * v, 0.0]) + (np.append(rng.normal(0.0, 3.0, 2), 0.0) if v else 0.0)
    C = near * C + np.array([0.0, 0.0, 400.0 + 0.5 * v])
    if away:
        C[0] += 1.0e4
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = R, -R @ C
    Pi = np.linalg.inv(_proj(K, E))
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.full((H, W), 400.0)
    for _ in range(200):                           # the depth along the ray at which the point lies on the surface
        Xw = Pi @ np.vstack(((d * uu).ravel(), (d * vv).ravel(), d.ravel(), np.ones(H * W)))
        new = (R @ np.vstack((Xw[0], Xw[1], pin_surface(Xw[0], Xw[1]))) + E[:3, 3:4])[2].reshape(H, W)
        delta = np.abs(new - d).max()
        d = new
        if delta < 1e-6:
            break
    else:
        raise RuntimeError("the depth iteration did not converge (last change %g)" % delta)
    return K, E, d


def pinhole_scene(sizes, seed=0, blunder=1.03, away=False):
    """-> (depths: list of float32 (H_v, W_v), K (V, 3, 3), E (V, 4, 4)).  Cameras look straight down from about 400 above the
    surface, a little apart and rotated about their axes; the last view's patch is multiplied by `blunder`."""
    V = len(sizes)
    views = [_pin_view(H, W, sizes[0][0], sizes[0][1], seed, v, bool(away and v == V - 1)) for v, (H, W) in enumerate(sizes)]
    depths = [d.astype(np.float32) for _, _, d in views]
    if blunder:
        depths[V - 1][patch(*sizes[V - 1])] *= np.float32(blunder)
    return depths, np.stack([k for k, _, _ in views]), np.stack([e for _, e, _ in views])


# ---- the remap, tap by tap ------------------------------------------------------------------------------------------------------
def fixed(c):
    """cvRound(c * 32) of float32 coordinates as int64 (non-finite -> the most negative integer, as x86 converts)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.rint(np.asarray(c, np.float32) * np.float32(32)).astype(np.int64)


def taps(img, x, y, border):
    """The four taps (float32, border value outside the image) and their weights (float32 multiples of 1/1024)."""
    img = np.asarray(img, np.float32)
    H, W = img.shape
    sx, sy = fixed(x), fixed(y)
    ix, iy = sx >> 5, sy >> 5
    ax, ay = (sx & 31).astype(np.float32) / _F32(32), (sy & 31).astype(np.float32) / _F32(32)

    def at(yy, xx):
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        return np.where(ok, img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], _F32(border)).astype(np.float32)
    one = _F32(1)
    t = np.stack([at(iy, ix), at(iy, ix + 1), at(iy + 1, ix), at(iy + 1, ix + 1)])
    w = np.stack([(one - ax) * (one - ay), ax * (one - ay), (one - ax) * ay, ax * ay])
    return t, w


def remap_bound(img, x, y, border):
    """8 * 2^-24 * max|tap| per pixel (float64; non-finite where a tap is)."""
    t, _ = taps(img, x, y, border)
    with np.errstate(invalid="ignore"):
        return 8.0 * _EPS32 * np.abs(t.astype(np.float64)).max(axis=0)


def _sample_diff(got, want, bound):
    """Pixels where two float32 samples differ: beyond the bound where the expected one is finite, in kind (NaN / +inf / -inf)
    elsewhere."""
    got, want = np.asarray(got), np.asarray(want)
    fin = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        bad = fin & (got != want) & ~(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= bound)
    return bad | (~fin & ~((np.isnan(got) & np.isnan(want)) | (got == want)))


def _coord_diff(got, want, tol):
    """Pixels where two coordinate maps differ by more than tol; a non-finite coordinate has one meaning (all four taps take
    the border), so two non-finite values agree."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        return ~((np.abs(got - want) <= tol) | (~np.isfinite(got) & ~np.isfinite(want)))


def _ulp32(c):
    with np.errstate(invalid="ignore"):
        return np.spacing(np.abs(np.asarray(c, np.float32))).astype(np.float64)


# ---- stage oracles ------------------------------------------------------------------------------------------------------------------
class Rpc:
    """The RPC filter's stages on the oracle's C projector."""
    kind, border, cap = "rpc", -999.0, RPC_CAP

    def back_tol(self, want):
        return 1e-6

    def __init__(self, orc, ref, src):
        self.orc, (self.rpc_ref, self.rpc_src) = orc, (np.asarray(ref, np.float64), np.asarray(src, np.float64))
        self.geo = (self.rpc_ref, self.rpc_src)

    def coords(self, depth_ref):
        H, W = depth_ref.shape
        xr, yr = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        h = np.asarray(depth_ref, np.float32).reshape(-1).astype(np.float64)
        lat, lon = self.orc.rpc_project(self.rpc_ref, xr.reshape(-1), yr.reshape(-1), h, 0)
        xs, ys = self.orc.rpc_project(self.rpc_src, lat, lon, h, 1)
        return xs.reshape(H, W), ys.reshape(H, W)

    def coord_tol(self, c):
        return 1e-8

    def back(self, depth_ref, xs, ys, sampled):
        H, W = sampled.shape
        sh = sampled.reshape(-1).astype(np.float64)
        lat, lon = self.orc.rpc_project(self.rpc_src, np.asarray(xs, np.float64).reshape(-1), np.asarray(ys, np.float64).reshape(-1), sh, 0)
        xb, yb = self.orc.rpc_project(self.rpc_ref, lat, lon, sh, 1)
        return xb.reshape(H, W), yb.reshape(H, W)

    def back_valid(self, sampled):
        return np.ones(sampled.shape, bool)

    def rule(self, depth_ref, sampled, xb, yb, p, d):
        """-> (mask, pixels within 4 ulp of a threshold, distance, height difference), numpy's arithmetic."""
        H, W = sampled.shape
        xr, yr = np.meshgrid(np.arange(W), np.arange(H))
        with np.errstate(invalid="ignore"):
            dist = np.sqrt((xb - xr) ** 2 + (yb - yr) ** 2)
            dd = np.abs(sampled - np.asarray(depth_ref, np.float32))
            mask = np.logical_and(dist < p, dd < d)
            near = (np.abs(dist - p) <= 4 * np.spacing(np.float64(p))) | (np.abs(dd.astype(np.float64) - d) <= 4 * np.spacing(np.float32(d)))
        return mask, near, dist, dd

    def at_risk(self, depth_ref, xs, ys):
        r = np.zeros(xs.shape, bool)
        for c in (xs, ys):
            r |= fixed((c - 1e-8).astype(np.float32)) != fixed((c + 1e-8).astype(np.float32))
        return r

    def oracle_reproject(self, depth_ref, depth_src):
        with np.errstate(all="ignore"):
            return self.orc.reproject_with_depth(depth_ref, self.rpc_ref, depth_src, self.rpc_src)

    def oracle_check(self, depth_ref, depth_src, p, d):
        with np.errstate(all="ignore"):
            return self.orc.check_geometric_consistency(depth_ref, self.rpc_ref, depth_src, self.rpc_src, p, d)

    def run_reproject(self, mod, depth_ref, depth_src):
        return mod.reproject_with_depth(depth_ref, self.rpc_ref, depth_src, self.rpc_src)

    def run_check(self, mod, depth_ref, depth_src, p, d):
        return mod.check_geometric_consistency(depth_ref, self.rpc_ref, depth_src, self.rpc_src, p, d)


class Pinhole:
    """The pinhole filter's stages in numpy (float64 matrix products, float32 coordinates)."""
    kind, border, cap = "pinhole", 0.0, PIN_CAP

    def back_tol(self, want):
        """5e-4 px; the outputs are float32, so beyond 4096 px (a sample much nearer than the reference depth goes back far
        outside the image) no implementation can be closer than one ulp of the result, and that takes over."""
        return np.maximum(5e-4, _ulp32(want))

    def __init__(self, orc, ref, src):
        self.orc, self.ref, self.src = orc, ref, src                     # (K, E) each
        self.P_ref, self.P_src = _proj(*ref), _proj(*src)
        self.inv_ref, self.inv_src = np.linalg.inv(self.P_ref), np.linalg.inv(self.P_src)

    def coords(self, depth_ref):
        H, W = depth_ref.shape
        row, col = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        d = np.asarray(depth_ref, np.float32).reshape(1, -1)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            tmp = np.vstack((d * col.reshape(1, -1), d * row.reshape(1, -1), d, np.ones((1, H * W))))
            xy = np.matmul(self.P_src, np.matmul(self.inv_ref, tmp))
            xy = xy[:2] / xy[2]
        return xy[0].reshape(H, W), xy[1].reshape(H, W)

    def coord_tol(self, c):
        return _ulp32(c)

    def back(self, depth_ref, xs, ys, sampled):
        """The reference (and the kernel) go back from the UNROUNDED float64 coordinates, which no entry returns; stage 1 ties
        the float32 (xs, ys) given here to them, so the oracle's own float64 pair stands in: going back from the float32 pair
        would add up to half an ulp of the coordinate times the magnification of a near sample, which is not the kernel's error."""
        H, W = sampled.shape
        xs, ys = self.coords(depth_ref)
        sv = sampled.reshape(1, -1).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            tmp = np.vstack((sv * np.asarray(xs, np.float64).reshape(1, -1), sv * np.asarray(ys, np.float64).reshape(1, -1), sv, np.ones((1, H * W))))
            b = np.matmul(self.P_ref, np.matmul(self.inv_src, tmp))
            b = b[:2] / b[2]
        return b[0].reshape(H, W), b[1].reshape(H, W)

    def back_valid(self, sampled):
        with np.errstate(invalid="ignore"):
            return np.isfinite(sampled) & (sampled > 0)

    def rule(self, depth_ref, sampled, xb, yb, p, d):
        H, W = sampled.shape
        xr, yr = np.meshgrid(np.arange(W), np.arange(H))
        depth_ref = np.asarray(depth_ref, np.float32)
        with np.errstate(invalid="ignore", divide="ignore"):
            dist = np.sqrt((xb - xr) ** 2 + (yb - yr) ** 2)
            rel = np.abs(sampled - depth_ref) / depth_ref
            mask = np.logical_and(dist < p, rel < np.float32(d))
            near = (np.abs(dist - p) <= 4 * np.spacing(np.float64(p))) | (np.abs(rel - np.float32(d)) <= 4 * np.spacing(np.float32(d)))
        return mask, near, dist, rel

    def coord_err(self, depth_ref):
        """A forward-error bound of the float64 source coordinates: each 4-term product sum errs by at most
        8 * 2^-53 * (|M| |x|), carried through both products and the division."""
        H, W = depth_ref.shape
        gam = 8.0 * 2.0 ** -53
        row, col = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        d = np.asarray(depth_ref, np.float32).reshape(1, -1)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            tmp = np.vstack((d * col.reshape(1, -1), d * row.reshape(1, -1), d, np.ones((1, H * W))))
            v = np.matmul(self.inv_ref, tmp)
            e1 = gam * np.matmul(np.abs(self.inv_ref), np.abs(tmp))
            w = np.matmul(self.P_src, v)
            e2 = gam * np.matmul(np.abs(self.P_src), np.abs(v)) + np.matmul(np.abs(self.P_src), e1)
            ex = (e2[0] + np.abs(w[0] / w[2]) * e2[2]) / np.abs(w[2]) + 2.0 ** -52 * np.abs(w[0] / w[2])
            ey = (e2[1] + np.abs(w[1] / w[2]) * e2[2]) / np.abs(w[2]) + 2.0 ** -52 * np.abs(w[1] / w[2])
        return ex.reshape(H, W), ey.reshape(H, W)

    def at_risk(self, depth_ref, xs, ys):
        """Two float64 evaluations of one coordinate (numpy's BLAS, the kernel) differ by at most twice coord_err; a pixel is
        at risk if moving the coordinate that far changes the float32 value's fixed-point.  This set lies inside the one that
        moving the float32 coordinate by one ulp gives (at_risk_ulp) -- that one holds 2 * 32 * ulp(c) of the pixels per
        coordinate whatever the implementation, which passes the cap of 2e-3 from about 250 pixels on."""
        r = np.zeros(xs.shape, bool)
        for c, e in zip((xs, ys), self.coord_err(depth_ref)):
            with np.errstate(invalid="ignore", over="ignore"):
                r |= fixed((c - 2 * e).astype(np.float32)) != fixed((c + 2 * e).astype(np.float32))
        return r

    def at_risk_ulp(self, xs, ys):
        r = np.zeros(xs.shape, bool)
        for c in (xs, ys):
            with np.errstate(invalid="ignore", over="ignore"):
                c = np.asarray(c).astype(np.float32)
                r |= fixed(np.nextafter(c, _F32(-np.inf))) != fixed(np.nextafter(c, _F32(np.inf)))
        return r

    def oracle_reproject(self, depth_ref, depth_src):
        with np.errstate(all="ignore"):
            return self.orc.pinhole_reproject_with_depth(depth_ref, *self.ref, depth_src, *self.src)

    def oracle_check(self, depth_ref, depth_src, p, d):
        with np.errstate(all="ignore"):
            return self.orc.pinhole_check_geometric_consistency(depth_ref, *self.ref, depth_src, *self.src, p, d)

    def run_reproject(self, mod, depth_ref, depth_src):
        return mod.reproject_with_depth(depth_ref, *self.ref, depth_src, *self.src)

    def run_check(self, mod, depth_ref, depth_src, p, d):
        return mod.check_geometric_consistency(depth_ref, *self.ref, depth_src, *self.src, p, d)


class OracleModule:
    """The oracle under the product modules' names: lets the CPU tests run the checks on the oracle itself."""
    def __init__(self, orc, kind):
        pre = "" if kind == "rpc" else "pinhole_"
        self.reproject_with_depth = getattr(orc, pre + "reproject_with_depth")
        self.check_geometric_consistency = getattr(orc, pre + "check_geometric_consistency")


def _n(a):
    return int(np.count_nonzero(a))


# ---- the checks -----------------------------------------------------------------------------------------------------------------------
def stages(g, mod, depth_ref, depth_src, p, d, tag=""):
    """Stage-by-stage parity with no excepted pixels; -> messages."""
    depth_ref, depth_src = np.asarray(depth_ref, np.float32), np.asarray(depth_src, np.float32)
    keep = depth_ref.copy(), depth_src.copy()
    msgs = []
    dep, xb, yb, xs, ys = g.run_reproject(mod, depth_ref, depth_src)
    m, dm, xs2, ys2 = g.run_check(mod, depth_ref, depth_src, p, d)
    cdt = np.float64 if g.kind == "rpc" else np.float32
    if not (dep.dtype == dm.dtype == np.float32 and m.dtype == np.bool_ and all(a.dtype == cdt for a in (xb, yb, xs, ys, xs2, ys2))
            and all(a.shape == depth_ref.shape for a in (dep, xb, yb, xs, ys, m, dm, xs2, ys2))):
        return ["%s%s: output dtypes / shapes" % (g.kind, tag)]
    if not (np.array_equal(xs, xs2, equal_nan=True) and np.array_equal(ys, ys2, equal_nan=True)):
        msgs.append("source coordinates of the two entries differ")
    # 1. source coordinates
    oxs, oys = g.coords(depth_ref)
    for name, got, want in (("x_src", xs, oxs), ("y_src", ys, oys)):
        bad = _coord_diff(got, want, g.coord_tol(want))
        if bad.any():
            msgs.append("stage 1 %s: %d pixels beyond the bound (worst %.3g)" % (name, _n(bad), np.nanmax(np.abs(got - want)[bad])))
    # 2. the remap at the implementation's own coordinates
    x32, y32 = xs.astype(np.float32), ys.astype(np.float32)
    with np.errstate(all="ignore"):
        want = g.orc.remap_linear_const(depth_src, x32, y32, g.border)
    bad = _sample_diff(dep, want, remap_bound(depth_src, x32, y32, g.border))
    if bad.any():
        i = np.argwhere(bad)[0]
        msgs.append("stage 2 sampled: %d pixels differ, first at %s: %r, expected %r" % (_n(bad), tuple(i), dep[tuple(i)], want[tuple(i)]))
    # 3. back-projection of the implementation's own (x_src, y_src, sampled)
    oxb, oyb = g.back(depth_ref, xs, ys, dep)
    ok = g.back_valid(dep)
    for name, got, want in (("x_back", xb, oxb), ("y_back", yb, oyb)):
        bad = _coord_diff(got, want, g.back_tol(want)) & ok
        if bad.any():
            msgs.append("stage 3 %s: %d pixels beyond the bound (worst %.3g)" % (name, _n(bad), np.nanmax(np.abs(got - want)[bad])))
    # 4. the rule on the implementation's own back-projection and sample
    wm, near, _, _ = g.rule(depth_ref, dep, xb, yb, p, d)
    bad = (m != wm) & ~near
    if bad.any():
        msgs.append("stage 4 mask: %d pixels differ from the rule (first %s)" % (_n(bad), tuple(np.argwhere(bad)[0])))
    wdm = np.where(m, dep, np.float32(0))
    if not np.array_equal(dm.view(np.uint32), wdm.view(np.uint32)):
        msgs.append("stage 4 masked sample: %d pixels are not (mask ? sampled : 0)" % _n(dm.view(np.uint32) != wdm.view(np.uint32)))
    if np.isnan(dm).any():
        msgs.append("stage 4 masked sample holds NaN")
    if not (np.array_equal(depth_ref.view(np.uint32), keep[0].view(np.uint32)) and np.array_equal(depth_src.view(np.uint32), keep[1].view(np.uint32))):
        msgs.append("the inputs were modified")
    return ["%s%s %s" % (g.kind, tag, s) for s in msgs]


def end_to_end(g, mod, depth_ref, depth_src, p, d, tag="", cap=True):
    """Implementation against oracle from the same inputs: differing pixels are a subset of the at-risk pixels, whose share
    stays under the cap; -> (messages, at-risk share, differing pixels)."""
    depth_ref, depth_src = np.asarray(depth_ref, np.float32), np.asarray(depth_src, np.float32)
    msgs = []
    dep, xb, yb, xs, ys = g.run_reproject(mod, depth_ref, depth_src)
    m, dm, _, _ = g.run_check(mod, depth_ref, depth_src, p, d)
    od, oxb, oyb, oxs, oys = g.oracle_reproject(depth_ref, depth_src)
    om, odm, _, _ = g.oracle_check(depth_ref, depth_src, p, d)
    cx, cy = g.coords(depth_ref)                                    # the oracle's coordinates before any cast
    risk = g.at_risk(depth_ref, cx, cy)
    for name, got, want in (("x_src", xs, cx), ("y_src", ys, cy)):
        bad = _coord_diff(got, want, g.coord_tol(want))
        if bad.any():
            msgs.append("%s: %d pixels beyond the bound" % (name, _n(bad)))
    bound = remap_bound(depth_src, oxs.astype(np.float32), oys.astype(np.float32), g.border)
    ok = g.back_valid(od) & g.back_valid(dep)
    diff = _sample_diff(dep, od, bound) | _sample_diff(dm, odm, bound) | (m != om)
    diff |= (_coord_diff(xb, oxb, g.back_tol(oxb)) | _coord_diff(yb, oyb, g.back_tol(oyb))) & ok
    stray = diff & ~risk
    if stray.any():
        i = tuple(np.argwhere(stray)[0])
        msgs.append("%d differing pixels are not at risk (first %s: sampled %r / %r, mask %r / %r)" % (_n(stray), i, dep[i], od[i], m[i], om[i]))
    share = float(risk.mean())
    if cap and share > g.cap:
        msgs.append("at-risk share %.3g above the cap %g" % (share, g.cap))
    return ["%s%s end to end: %s" % (g.kind, tag, s) for s in msgs], share, diff


def near_threshold(g, depth_ref, depth_src, p, d):
    """Pixels of the ORACLE's run that lie close to a threshold of the rule -- with margins far wider than the 4 ulp the
    stage-4 check excepts and than what the end-to-end bounds can move (1e-5 px / 1e-3 m for RPC; 2e-3 px / 1e-5 relative for
    pinhole): scenes are chosen so that this is empty, which keeps both exceptions empty."""
    od, oxb, oyb, _, _ = g.oracle_reproject(depth_ref, depth_src)
    _, _, dist, dd = g.rule(depth_ref, od, oxb, oyb, p, d)
    mp, md = (1e-5, 1e-3) if g.kind == "rpc" else (2e-3, 1e-5)
    with np.errstate(invalid="ignore"):
        return (np.abs(dist - p) <= mp) | (np.abs(dd.astype(np.float64) - float(np.float32(d) if g.kind == "pinhole" else d)) <= md)


# ---- remap known answers through the pinhole entry ----------------------------------------------------------------------------------
SHIFTS = ((1 / 64, 3 / 64), (33 / 64, 17 / 64), (2 + 31 / 64, 1 + 63 / 64),          # every pixel on a tie of the 1/32-px rounding
          (-1 / 64, -33 / 64), (-3 - 17 / 64, -63 / 64), (-1.0, -1.0),                    # negative: sx < 0, ix = -1
          (0.5, 0.5), (33 / 64, 0.0),                                                     # the last row / column half out
          (1000.0 + 1 / 64, 0.25), (0.0, -(1000.0 + 3 / 64)), (-2000.0, 3000.0))          # farther than any image here: all border
SHIFT_SIZES = (((9, 13), (9, 13)), ((9, 13), (5, 21)), ((33, 70), (40, 37)), ((1, 1), (1, 1)), ((17, 257), (19, 300)))


def shift_case(ref_hw, src_hw, tx, ty, seed=0, depth=4.0):
    """Identity reference camera, source with a pure principal-point shift, constant power-of-two depth: x_src = x + tx and
    y_src = y + ty exactly; the source map holds small integers, so every product and sum of the remap is exact.
    -> (depth_ref, (K, E) ref, depth_src, (K, E) src, x_src, y_src float32, sampled float32 written out from the four taps)."""
    (H, W), (Hs, Ws) = ref_hw, src_hw
    K = np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]])
    src = np.random.default_rng(seed).integers(1, 200, (Hs, Ws)).astype(np.float32)
    xs = (np.arange(W, dtype=np.float64) + tx)[None, :].repeat(H, 0)
    ys = (np.arange(H, dtype=np.float64) + ty)[:, None].repeat(W, 1)
    assert np.array_equal(xs.astype(np.float32), xs) and np.array_equal(ys.astype(np.float32), ys)
    sx, sy = np.rint(xs * 32).astype(np.int64), np.rint(ys * 32).astype(np.int64)             # exact products; ties go to even
    ix, iy = np.floor_divide(sx, 32), np.floor_divide(sy, 32)
    ax, ay = (sx - 32 * ix) / 32.0, (sy - 32 * iy) / 32.0

    def at(yy, xx):
        ok = (xx >= 0) & (xx < Ws) & (yy >= 0) & (yy < Hs)
        return np.where(ok, src[np.clip(yy, 0, Hs - 1), np.clip(xx, 0, Ws - 1)].astype(np.float64), 0.0)
    val = at(iy, ix) * (1 - ax) * (1 - ay) + at(iy, ix + 1) * ax * (1 - ay) + at(iy + 1, ix) * (1 - ax) * ay + at(iy + 1, ix + 1) * ax * ay
    assert np.array_equal(val.astype(np.float32), val)                                       # exact in float32 too
    return (np.full((H, W), depth, np.float32), (np.eye(3), np.eye(4)), src, (K, np.eye(4)),
            xs.astype(np.float32), ys.astype(np.float32), val.astype(np.float32))


# ---- non-finite and degenerate inputs ----------------------------------------------------------------------------------------------
def spoil(depth, what, where):
    """A copy of the map with `what` written to a patch ("patch") or everywhere ("all")."""
    out = np.array(depth, np.float32, copy=True)
    H, W = out.shape
    if where == "all":
        out[:] = what
    else:
        out[H // 4:H // 2, W // 5:W // 2] = what
        out[0, 0] = out[H - 1, W - 1] = what
    return out


# ---- the scenes the GPU tests run (tests/test_filter_cpu.py checks the caps and the empty exception sets on every one) -----------
def pair(kind, orc, ref_hw, src_hw, seed=1, away=False):
    """-> (stage oracle, depth_ref, depth_src, p, d) of a two-view scene: view 0 the reference, view 1 the source."""
    if kind == "rpc":
        depths, rpcs, _, _ = rpc_scene((tuple(ref_hw), tuple(src_hw)), seed, away=away)
        return (Rpc(orc, rpcs[0], rpcs[1]), depths[0], depths[1]) + RPC_PARAMS
    depths, K, E = pinhole_scene((tuple(ref_hw), tuple(src_hw)), seed, away=away)
    return (Pinhole(orc, (K[0], E[0]), (K[1], E[1])), depths[0], depths[1]) + PIN_PARAMS


FILTER_VIEWS = {2: ((64, 96), (70, 101)), 3: ((67, 131), (67, 131), (50, 160)),
                5: ((96, 128), (96, 128), (80, 150), (120, 100), (101, 131))}
SPOILS = (np.nan, np.inf, -np.inf, -999.0, 0.0, -3.0)
