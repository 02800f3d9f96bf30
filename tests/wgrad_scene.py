"""Cases, float64 reference, per-weight error bound, a float32 model and a checker for the weight-gradient entries of
csrc/conv_wgrad.hip: smvs_conv3x3_wgrad, _strided, _cat, _list and smvs_conv3d_wgrad (atomic and two-stage form).  Shared by
tests/test_wgrad_cpu.py (which asserts, without a GPU, what the GPU tests assume about these cases, the reference and the bound) and
tests/test_wgrad_gpu.py.  Nothing here imports the kernels: the split a launch takes comes from the library's own plan queries
(smvs_conv3x3_wgrad_plan, smvs_conv3d_wgrad_plan), handed in by the caller as plain functions.

The definition (include/satmvs.h), s = stride, window (B, Cwin, s * dims), grid (B, Cgrid, dims):
    dw[g][c][k] += sum_{b, p} grid[b][g][p] * window[b][c][s * p + k - 1]      (terms whose window position is outside: absent)
    db[g]       += sum_{b, p} grid[b][g][p]                                      (2-D, where given)
Conv (stride s, pad 1): window = layer input, grid = output gradient.  Transposed conv (stride s, pad 1, output_padding s - 1):
window = output gradient, grid = layer input -- the same sums.

Two kinds of scene per case:
  * integer: every value of window, grid and the initial dw / db is one of -3, -2, -1, 1, 2, 3 (no zeros: a dropped, doubled or
    misplaced term changes the sum).  Every product and every partial sum in ANY order is an integer of magnitude at most
    |init| + sum |terms| < 2^24, so float32 arithmetic is exact whatever the lane reduction, the arrival order of the atomics or the
    fold order: the result must EQUAL the float64 reference.  scene() asserts the magnitude condition per case.
  * real: randn, the last window channel and the last grid channel moved to 100 +- 1.  Per weight
        |got - ref| <= (n + 2) 2^-24 (|init| + sum |terms|) + n 2^-126          (conv_scene.bound_from)
    with n the number of terms of THAT weight and the magnitudes summed in float64: it holds for any summation order of correctly
    rounded fused multiply-adds and additions (adding an exact zero rounds nothing), so it needs no mirror of the split.
"""
import functools
import itertools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import conv_scene

U32 = conv_scene.U32
LIST_MAX = 64                         # tensors per launch of the list form (csrc/conv_wgrad.hip: WGRAD_LIST_MAX)
INT_LIMIT = 2.0 ** 24
VALUES = (-3, -2, -1, 1, 2, 3)

# entry: "wgrad" / "strided" / "cat" / "list" / "3d";  role: "conv" / "transposed" (which layer the sums are the weight gradient of);
# B: samples (None for the list form), n / Bper: the list (None otherwise);  CA (+ CB: second window operand) window channels, Cgrid grid
# channels;  dims: the GRID plane (H, W) or volume (D, H, W);  db: the bias gradient is asked for;  dw0: "zero" / "nonzero" initial dw
# (and db);  form: None (2-D) / "atomic" / "two_stage"
Case = namedtuple("Case", "name entry stride role B n Bper CA CB Cgrid dims db dw0 form")


def _c2(name, entry, stride, CA, CB, Cgrid, dims, B=None, lst=None, db=True, dw0="zero", role="conv"):
    n, Bper = lst if lst else (None, None)
    assert (B is None) != (lst is None) and (entry == "list") == (lst is not None)
    return Case(name, entry, stride, role, B, n, Bper, CA, CB, Cgrid, tuple(dims), db, dw0, None)


def _c3(name, stride, B, Cwin, Cgrid, dims, form, dw0="zero", role="conv"):
    return Case(name, "3d", stride, role, B, None, None, Cwin, 0, Cgrid, tuple(dims), False, dw0, form)


# Each case is the smallest shape that reaches its class; the split in the comments is what the plan query reports (asserted through
# the query in tests/test_wgrad_cpu.py, never through a copy of the rule).
CASES_2D = [
    _c2("1x1-cin1-cout1", "wgrad", 1, 1, 0, 1, (1, 1), B=1),
    _c2("h2-w63-cin3-cout3-b2", "wgrad", 1, 3, 0, 3, (2, 63), B=2, db=False, dw0="nonzero"),
    _c2("h16-w64-cout8", "strided", 1, 2, 0, 8, (16, 64), B=1, dw0="nonzero"),
    _c2("h17-w65-cout9", "wgrad", 1, 2, 0, 9, (17, 65), B=1),                                    # rows 9 + 8, two column strips
    _c2("h33-w127-t", "strided", 1, 3, 0, 1, (33, 127), B=1, db=False, role="transposed"),       # rows 9, 9, 9, 6
    _c2("h18-w128-b2", "wgrad", 1, 1, 0, 3, (18, 128), B=2),                                     # rows 9 + 9
    _c2("h1-w129", "strided", 1, 2, 0, 8, (1, 129), B=1, db=False),                              # three column strips
    _c2("s2-odd-b2", "strided", 2, 3, 0, 9, (5, 7), B=2, dw0="nonzero"),
    _c2("s2-t-h17-w65", "strided", 2, 2, 0, 3, (17, 65), B=1, db=False, role="transposed"),
    _c2("s2-1x1", "strided", 2, 1, 0, 1, (1, 1), B=1),
    _c2("cat-cb3", "cat", 1, 2, 3, 9, (3, 65), B=2, dw0="nonzero"),
    _c2("cat-cb2-h17", "cat", 1, 2, 2, 8, (17, 5), B=1, db=False),
    _c2("cat-cb0", "cat", 1, 3, 0, 3, (2, 3), B=1),
    _c2("bchunk2", "wgrad", 1, 128, 0, 64, (4, 8), B=9),                                         # samples 2, 2, 2, 2, 1 per wave
    _c2("list-n1-cat", "list", 1, 2, 3, 3, (3, 5), lst=(1, 2)),
    _c2("list-n3-straddle", "list", 1, 128, 0, 64, (4, 8), lst=(3, 3), dw0="nonzero"),           # chunk {2, 3}: tensors 0 and 1
    _c2("list-n64-s2", "list", 2, 2, 0, 3, (2, 3), lst=(64, 1), db=False),
    _c2("list-n65", "list", 1, 3, 0, 9, (2, 3), lst=(65, 1), dw0="nonzero"),                     # 64 + 1: a second launch
    _c2("list-s2-t-cat", "list", 2, 2, 2, 8, (3, 5), lst=(3, 2), db=False, role="transposed"),
]
CASES_3D = [
    _c3("gc1-s1-h5", 1, 1, 3, 1, (2, 5, 7), "atomic"),
    _c3("gc1-s2-d1-b2", 2, 2, 2, 1, (1, 3, 5), "atomic", dw0="nonzero"),
    _c3("gc1-two-ndc5-nrc2", 2, 1, 1, 1, (5, 17, 3), "two_stage"),                               # 10 waves per group: 8 + a tail of 2
    _c3("cg8-h4-w65", 1, 1, 1, 8, (2, 4, 65), "two_stage"),                                      # 4 waves per group: no tail
    _c3("cg9-h6-d5", 1, 1, 3, 9, (5, 6, 3), "two_stage", dw0="nonzero"),                         # 5 waves per group: 4 + a tail of 1
    _c3("h7-w63-b2", 1, 2, 2, 3, (1, 7, 63), "atomic"),
    _c3("dchunk2", 1, 1, 64, 64, (8, 4, 8), "atomic"),                                           # atomic: planes 2, 2, 2, 2 per wave
    _c3("dchunk4-two", 1, 1, 64, 64, (8, 4, 8), "two_stage", dw0="nonzero"),                     # two-stage: planes 4 + 4
    _c3("atomic-nrc2", 1, 1, 1, 2, (2, 17, 5), "atomic", dw0="nonzero"),                         # rows 9 + 8
    _c3("two-nrc2-d1", 1, 1, 2, 8, (1, 17, 5), "two_stage"),                                     # 2 waves per group: tail only
    _c3("s2-t-odd", 2, 1, 3, 9, (3, 5, 7), "atomic", role="transposed"),
    _c3("two-b2-d2", 1, 2, 3, 3, (2, 5, 4), "two_stage"),
    _c3("two-s2-b3-d5", 2, 3, 2, 9, (5, 2, 2), "two_stage", dw0="nonzero", role="transposed"),   # 15 waves per group: 12 + a tail of 3
]
CASES = CASES_2D + CASES_3D
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def cwin(c):
    return c.CA + c.CB


def total_B(c):
    return c.B if c.B is not None else c.n * c.Bper


def launches(c):
    """sample count of every launch the entry makes: one, or one per 64 tensors of a list"""
    if c.entry != "list":
        return [c.B]
    return [min(LIST_MAX, c.n - i) * c.Bper for i in range(0, c.n, LIST_MAX)]


def plans(c, plan2, plan3, form=None):
    """The plan of every launch of case c through the library's queries: plan2(B, Cin, Cout, H, W, stride) and
    plan3(B, Cwin, Cgrid, D, H, W, stride, two_stage) -> (status, [6 ints])."""
    out = []
    for B in launches(c):
        if c.entry == "3d":
            rc, p = plan3(B, cwin(c), c.Cgrid, c.dims[0], c.dims[1], c.dims[2], c.stride, 1 if (form or c.form) == "two_stage" else 0)
        else:
            rc, p = plan2(B, cwin(c), c.Cgrid, c.dims[0], c.dims[1], c.stride)
        assert rc == 0, (c.name, "the plan query rejects the case", rc)
        out.append(list(p))
    return out


def waves_per_group(c, plan):
    """two-stage 3-D form: the waves whose partial sums the fold adds for one group of 144 weights"""
    return c.B * plan[1] * plan[4] * plan[3]


def workspace_floats(c, plan):
    return ((cwin(c) + 1) // 2) * ((c.Cgrid + 7) // 8) * 3 * waves_per_group(c, plan) * 144


# ---- census ---------------------------------------------------------------------------------------------------------------------
def classes(c, plan2, plan3):
    """The classes a case reaches, as tags; everything about the split is read from the plan queries."""
    t = set()
    pl = plans(c, plan2, plan3)
    ci, s = cwin(c), c.stride
    if c.entry != "3d":
        H, W = c.dims
        t.update({"W=%d" % W, "H=%d" % H, "Cout=%d" % c.Cgrid, "stride=%d" % s, "entry=" + c.entry, "role=" + c.role})
        t.add("Cin=1" if ci == 1 else "Cin-odd" if ci % 2 else "Cin-even")
        if H == 1 and W == 1:
            t.add("1x1")
        if s == 2 and H % 2 and W % 2:
            t.add("s2-odd-HW")
        for (bchunk, nbc, rows, nrc, nxs, waves), B in zip(pl, launches(c)):
            if bchunk > 1 and B % bchunk:
                t.add("bchunk>1-ragged")
            if nrc > 1:
                t.add("nrc>1-ragged" if H % rows else "nrc>1-even")
                t.add("row-chunks=" + "+".join(str(min(rows, H - r * rows)) for r in range(nrc)))
            if nxs > 1:
                t.add("nxs>1")
            if c.entry == "list" and bchunk > 1 and any((k * bchunk) // c.Bper != (min(B, (k + 1) * bchunk) - 1) // c.Bper for k in range(nbc)):
                t.add("list-chunk-straddles")
        if c.CB:
            t.add("two-operand-CA=%d-CB-%s" % (c.CA, "odd" if c.CB % 2 else "even"))
        if c.entry == "list":
            t.add("list-n=%d" % c.n)
        t.add("db-given" if c.db else "db-null")
        if c.dw0 == "nonzero":
            t.add("nonzero-init")
    else:
        D, H, W = c.dims
        (dchunk, ndc, rows, nrc, nxs, waves), = pl
        t.update({"Cgrid=%d" % c.Cgrid, "D=%d" % D, "stride=%d" % s, "form=" + c.form})
        if c.Cgrid == 1:
            t.add("GC1-s%d" % s)
        t.add("Cwin=1" if ci == 1 else "Cwin-odd" if ci % 2 else "Cwin-even")
        if s == 1:
            t.update("s1-rows%%4=%d" % (min(rows, H - r * rows) % 4) for r in range(nrc))
            if nrc == 1:
                t.add("s1-H%%4=%d" % (H % 4))
        if c.B > 1:
            t.add("B>1")
        if dchunk > 1:
            t.add(c.form + "-dchunk>1")
        if ndc > 1:
            t.add(c.form + "-ndc>1")
        if nrc > 1:
            t.add(c.form + "-nrc>1")
        if nxs > 1:
            t.add("nxs>1")
        if c.form == "two_stage":
            w = waves_per_group(c, pl[0])
            t.add("fold-waves=%d" % w)
            if w >= 5 and w % 4:
                t.add("fold-whole-groups-and-tail")
            if w % 4 == 0:
                t.add("fold-no-tail")
            if w < 4:
                t.add("fold-tail-only")
        if c.dw0 == "nonzero":
            t.add("nonzero-init-" + c.form)
    return t


REQUIRED_2D = ({"W=%d" % w for w in (1, 63, 64, 65, 127, 128, 129)} | {"H=%d" % h for h in (1, 2, 16, 17, 33)}
               | {"1x1", "Cin=1", "Cin-odd", "Cin-even", "Cout=1", "Cout=3", "Cout=8", "Cout=9", "stride=1", "stride=2", "s2-odd-HW",
                  "bchunk>1-ragged", "nrc>1-ragged", "nrc>1-even", "row-chunks=9+8", "row-chunks=9+9+9+6", "nxs>1",
                  "two-operand-CA=2-CB-odd", "two-operand-CA=2-CB-even", "list-n=1", "list-n=3", "list-n=64", "list-n=65",
                  "list-chunk-straddles", "db-given", "db-null", "nonzero-init", "role=conv", "role=transposed",
                  "entry=wgrad", "entry=strided", "entry=cat", "entry=list"})
REQUIRED_3D = {"GC1-s1", "GC1-s2", "Cgrid=8", "Cgrid=9", "Cwin=1", "Cwin-odd", "D=1", "D=2", "D=5",
               "s1-H%4=0", "s1-H%4=1", "s1-H%4=2", "s1-H%4=3", "B>1", "atomic-dchunk>1", "atomic-nrc>1", "two_stage-ndc>1",
               "two_stage-nrc>1", "fold-whole-groups-and-tail", "fold-no-tail", "fold-tail-only", "two_stage-dchunk>1",
               "nonzero-init-atomic", "nonzero-init-two_stage", "nxs>1", "stride=1", "stride=2", "form=atomic", "form=two_stage"}


def covered(cases, plan2, plan3):
    got = set()
    for c in cases:
        got |= classes(c, plan2, plan3)
    return got


# ---- the definition in float64 ---------------------------------------------------------------------------------------------------
def wgrad(win, grid, s):
    """dw (Cgrid, Cwin, 3, 3[, 3]) of the definition in the dtype of the operands (float64 in every use here), without an initial
    value.  win (B, Cwin, s * dims), grid (B, Cgrid, dims).  The window is padded by one zero: an absent term is an exact 0."""
    nd = grid.dim() - 2
    dims = tuple(grid.shape[2:])
    assert tuple(win.shape[2:]) == tuple(s * d for d in dims) and win.shape[0] == grid.shape[0]
    xp = F.pad(win, (1, 1) * nd)
    out = torch.zeros((grid.shape[1], win.shape[1]) + (3,) * nd, dtype=win.dtype)
    for k in itertools.product(range(3), repeat=nd):
        sl = tuple(slice(ki, ki + s * (d - 1) + 1, s) for ki, d in zip(k, dims))       # padded index of s * p + k - 1 is s * p + k
        out[(slice(None), slice(None)) + k] = torch.einsum("bg...,bc...->gc", grid, xp[(slice(None), slice(None)) + sl])
    return out


def loop_wgrad(win, grid, s):
    """The definition term by term in numpy float64 (tiny shapes): no padding, no library contraction."""
    win, grid = np.asarray(win, np.float64), np.asarray(grid, np.float64)
    nd = grid.ndim - 2
    dims, wd = grid.shape[2:], win.shape[2:]
    out = np.zeros((grid.shape[1], win.shape[1]) + (3,) * nd)
    for b, g, ch in itertools.product(range(grid.shape[0]), range(grid.shape[1]), range(win.shape[1])):
        for k in itertools.product(range(3), repeat=nd):
            for p in itertools.product(*[range(d) for d in dims]):
                q = tuple(s * pi + ki - 1 for pi, ki in zip(p, k))
                if all(0 <= qi < d for qi, d in zip(q, wd)):
                    out[(g, ch) + k] += grid[(b, g) + p] * win[(b, ch) + q]
    return out


def autograd_wgrad(c, win, grid):
    """The weight gradient autograd gives for the layer the case's role names, float64: conv: d/dw of <conv(win, w), grid>;
    transposed: d/dw of <conv_transpose(grid, w), win> (its weight is (Cin_layer, Cout_layer, ...) = (Cgrid, Cwin, ...))."""
    nd = len(c.dims)
    conv, convT = (F.conv2d, F.conv_transpose2d) if nd == 2 else (F.conv3d, F.conv_transpose3d)
    w = torch.zeros((grid.shape[1], win.shape[1]) + (3,) * nd, dtype=torch.float64, requires_grad=True)
    if c.role == "conv":
        y, dy = conv(win, w, stride=c.stride, padding=1), grid
    else:
        y, dy = convT(grid, w, stride=c.stride, padding=1, output_padding=c.stride - 1), win
    assert y.shape == dy.shape, (c.name, tuple(y.shape), tuple(dy.shape))
    return torch.autograd.grad(y, w, dy)[0]


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def _seed(c, kind):
    return (sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)) + (7919 if kind == "int" else 0)) % (2 ** 31)


def _draw(shape, kind, g):
    if kind == "int":
        return torch.tensor(VALUES, dtype=torch.float32)[torch.randint(0, len(VALUES), shape, generator=g)]
    return torch.randn(shape, generator=g)


Scene = namedtuple("Scene", "wins grids dw0 db0")      # lists of float32 tensors (one per tensor of a list, else one), initial dw / db


@functools.lru_cache(maxsize=None)
def scene(c, kind):
    """The float32 CPU tensors of case c, kind "int" / "real".  Shared: do not modify (clone first)."""
    g = torch.Generator().manual_seed(_seed(c, kind))
    n = c.n or 1
    Bt = c.Bper if c.n else c.B
    wd = tuple(c.stride * d for d in c.dims)
    wins = [_draw((Bt, cwin(c)) + wd, kind, g) for _ in range(n)]
    grids = [_draw((Bt, c.Cgrid) + c.dims, kind, g) for _ in range(n)]
    if kind == "real":
        for w_, g_ in zip(wins, grids):
            w_[:, -1] += 100.0
            g_[:, -1] += 100.0
    wshape = (c.Cgrid, cwin(c)) + (3,) * len(c.dims)
    if c.dw0 == "nonzero":
        dw0, db0 = _draw(wshape, kind, g), _draw((c.Cgrid,), kind, g)
    else:
        dw0, db0 = torch.zeros(wshape), torch.zeros((c.Cgrid,))
    return Scene(wins, grids, dw0, db0)


Ref = namedtuple("Ref", "dw db dw_bound db_bound")     # float64; db / db_bound None where the case asks for no bias gradient


def reference_of(c, sc, kind, calls=1):
    """Reference and bound of `calls` successive calls on scene sc (each adds the same sums).  Integer scenes: asserts the
    magnitude condition and returns zero bounds (the result must be equal)."""
    win, grid = torch.cat(sc.wins).double(), torch.cat(sc.grids).double()
    dw = sc.dw0.double() + calls * wgrad(win, grid, c.stride)
    A = calls * wgrad(win.abs(), grid.abs(), c.stride)
    one = wgrad(torch.ones_like(win[:, :1]), torch.ones_like(grid[:, :1]), c.stride)       # terms per weight, by tap
    n = calls * one.expand_as(dw)
    db = dbA = None
    nb = calls * grid.shape[0] * int(np.prod(c.dims))
    if c.db:
        red = tuple(i for i in range(grid.dim()) if i != 1)
        db = sc.db0.double() + calls * grid.sum(red)
        dbA = calls * grid.abs().sum(red)
    if kind == "int":
        top = float(torch.nan_to_num(A + sc.dw0.double().abs()).max())       # (a scene with a planted NaN: the finite sums)
        assert top < INT_LIMIT, (c.name, "integer scene leaves the exact range", top)
        if c.db:
            assert float(torch.nan_to_num(dbA + sc.db0.double().abs()).max()) < INT_LIMIT
        return Ref(dw, db, torch.zeros_like(dw), torch.zeros_like(db) if c.db else None)
    return Ref(dw, db, conv_scene.bound_from(n, A, sc.dw0), conv_scene.bound_from(nb, dbA, sc.db0) if c.db else None)


@functools.lru_cache(maxsize=None)
def reference(c, kind):
    """reference_of the case's own scene, one call.  Computed once per (case, kind) and shared; do not modify."""
    return reference_of(c, scene(c, kind), kind)


# ---- checker --------------------------------------------------------------------------------------------------------------------
Report = namedtuple("Report", "ok ratio where first message")


def check(got, ref, bound, what="dw"):
    """got (float32 or float64 tensor) against ref within bound, element by element.  -> Report: ok, the worst err / bound (0 / 0 = 0:
    an exact scene passes with ratio 0, any difference under a zero bound counts as infinite; so does a non-finite value where the
    reference is finite, and a finite one where it is not), its indices, the first offender's indices and a message naming it."""
    got = got.double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    fin = torch.isfinite(ref)
    err = (got - ref).abs()
    err = torch.where(fin, torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf"))),
                      torch.where(torch.isnan(got) == torch.isnan(ref), torch.zeros_like(err), torch.full_like(err, float("inf"))))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(0.0))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    flat = ratio.flatten()
    i = int(torch.argmax(flat))
    where = tuple(int(v) for v in np.unravel_index(i, tuple(ratio.shape)))
    bad = torch.nonzero(flat > 1.0)
    if len(bad) == 0:
        return Report(True, float(flat[i]), where, None, "")
    first = tuple(int(v) for v in np.unravel_index(int(bad[0]), tuple(ratio.shape)))
    msg = "%s%s: got %r, reference %r, error %.3e, bound %.3e (%d of %d outside; worst ratio %.3g at %s)" % (
        what, list(first), float(got[first]), float(ref[first]), float(err[first]), float(bound[first]), len(bad), flat.numel(), float(flat[i]), list(where))
    return Report(False, float(flat[i]), where, first, msg)


def check_case(c, kind, dw, db, ref=None):
    """dw (and db where the case gives one) of case c against its reference.  -> (ok, worst ratio over both, message)"""
    ref = ref or reference(c, kind)
    r = check(dw, ref.dw, ref.dw_bound, c.name + " dw")
    ok, ratio, msg = r.ok, r.ratio, r.message
    if c.db:
        rb = check(db, ref.db, ref.db_bound, c.name + " db")
        ok, ratio, msg = ok and rb.ok, max(ratio, rb.ratio), msg or rb.message
    return ok, ratio, msg


# ---- a float32 model of the kernels' summation, following the plan ---------------------------------------------------------------
def _fma32(a, b, acc):
    return (a.astype(np.float64) * b.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def _lane_tree(a):
    """pairwise sum over the last axis (64 lanes), float32: lane i + lane i + 32, then + 16, ... like the swap / DPP network"""
    h = a.shape[-1]
    while h > 1:
        h //= 2
        a = a[..., :h] + a[..., h:2 * h]
    return a[..., 0]


def model_f32(c, sc, plan_list, seed=0, form=None):
    """What float32 hardware following the plan may return: per wave and lane (= column of a 64-column strip) a sequential chain of
    fused multiply-adds over the wave's samples / planes and rows, a pairwise reduction over the 64 lanes, then the waves' sums added
    onto dw one by one in a shuffled order (atomic forms), or per group in wave order on four accumulators and a tail,
    (s0 + s1) + (s2 + s3), then onto dw (two-stage form).  -> (dw, db or None) float32 tensors."""
    rng = np.random.RandomState(seed)
    form = form or c.form
    s, nd = c.stride, len(c.dims)
    win = np.concatenate([w.numpy() for w in sc.wins]).astype(np.float32)
    grid = np.concatenate([g.numpy() for g in sc.grids]).astype(np.float32)
    if nd == 2:                                                     # a volume of one plane whose depth tap is always the middle one
        win, grid = win[:, :, None], grid[:, :, None]
    D, H, W = grid.shape[2:]
    xp = np.pad(win, ((0, 0), (0, 0), (1, 1) if nd == 3 else (0, 0), (1, 1), (1, 1)))
    Cg, Cw = grid.shape[1], win.shape[1]
    kds = range(3) if nd == 3 else [0]
    partial = {kd: [] for kd in kds}                                # kd -> the waves' sums (Cg, Cw, 3, 3), in wave order
    bpartial = []
    b_base = 0
    for (c0, n0, rows, nrc, nxs, _), Bl in zip(plan_list, launches(c)):
        if nd == 2:
            bchunk, dchunk = c0, 1
        else:
            bchunk, dchunk = 1, c0
        for b0 in range(0, Bl, bchunk):
            for d0 in range(0, D, dchunk):
                for xs in range(nxs):
                    x0, x1 = xs * 64, min(W, xs * 64 + 64)
                    for rc in range(nrc):
                        y0, y1 = rc * rows, min(H, rc * rows + rows)
                        bacc = np.zeros((Cg, 64), np.float32)
                        for kd in kds:
                            acc = np.zeros((Cg, Cw, 3, 3, 64), np.float32)
                            for b in range(b_base + b0, b_base + min(Bl, b0 + bchunk)):
                                for d in range(d0, min(D, d0 + dchunk)):
                                    zd = s * d + kd if nd == 3 else 0                  # padded plane index of s d + kd - 1
                                    for y in range(y0, y1):
                                        g = grid[b, :, d, y, x0:x1]                    # (Cg, lanes)
                                        w9 = np.stack([np.stack([xp[b, :, zd, s * y + ky, s * x0 + kx:s * (x1 - 1) + kx + 1:s] for kx in range(3)], 1)
                                                       for ky in range(3)], 1)          # (Cw, 3, 3, lanes)
                                        L = x1 - x0
                                        acc[..., :L] = _fma32(g[:, None, None, None, :], w9[None], acc[..., :L])
                                        if kd == kds[0] and c.db:
                                            bacc[:, :L] = bacc[:, :L] + g
                            partial[kd].append(_lane_tree(acc))
                        bpartial.append(_lane_tree(bacc))
        b_base += Bl
    dw = sc.dw0.numpy().astype(np.float32).copy()
    if nd == 2:
        dw = dw[:, :, None]
    for kd in kds:
        ps = partial[kd]
        if form == "two_stage":
            s4 = [np.zeros_like(ps[0]) for _ in range(4)]
            whole = len(ps) - len(ps) % 4
            for i, p in enumerate(ps):
                j = i % 4 if i < whole else 0
                s4[j] = s4[j] + p
            dw[:, :, kd] = dw[:, :, kd] + ((s4[0] + s4[1]) + (s4[2] + s4[3]))
        else:
            for i in rng.permutation(len(ps)):
                dw[:, :, kd] = dw[:, :, kd] + ps[i]
    if nd == 2:
        dw = dw[:, :, 0]
    db = None
    if c.db:
        db = sc.db0.numpy().astype(np.float32).copy()
        for i in rng.permutation(len(bpartial)):
            db = db + bpartial[i]
        db = torch.from_numpy(db)
    return torch.from_numpy(np.ascontiguousarray(dw)), db


# ---- planted errors: wrong results a kernel of this design could return, for the checker to catch --------------------------------
def _masked(grid, **keep):
    """grid with everything outside the kept index ranges set to 0: the definition restricted to a region of the grid"""
    m = torch.zeros_like(grid)
    idx = [slice(None)] * grid.dim()
    for axis, rng_ in keep.items():
        idx[int(axis[1:])] = rng_
    m[tuple(idx)] = grid[tuple(idx)]
    return m


PLANTS = ("border-row-twice", "border-column-left-out", "taps-kx-swapped", "odd-pair-second-channel-published", "list-tensor-skipped",
          "initial-dw-overwritten", "fold-tail-wave-lost")


def applicable(c, plant, plan_list):
    if plant == "taps-kx-swapped":                      # (a one-column window has neither tap: both sums are empty)
        return c.stride * c.dims[-1] > 1
    if plant == "odd-pair-second-channel-published":
        return cwin(c) % 2 == 1 and c.Cgrid > 1
    if plant == "list-tensor-skipped":
        return c.entry == "list" and c.n > 1
    if plant == "initial-dw-overwritten":
        return c.dw0 == "nonzero"
    if plant == "fold-tail-wave-lost":
        return c.form == "two_stage" and waves_per_group(c, plan_list[0]) % 4 != 0
    return True


def planted(c, kind, plant, plan_list):
    """dw (float32) of case c's scene with the named error in it.  float64 throughout, rounded once: the error alone separates it
    from the reference."""
    sc = scene(c, kind)
    s, nd = c.stride, len(c.dims)
    win, grid = torch.cat(sc.wins).double(), torch.cat(sc.grids).double()
    dw0 = sc.dw0.double()
    true = wgrad(win, grid, s)
    ya, xa = "a%d" % (grid.dim() - 2), "a%d" % (grid.dim() - 1)
    H, W = c.dims[-2:]
    if plant == "border-row-twice":                    # the last row of the grid enters once more
        out = dw0 + true + wgrad(win, _masked(grid, **{ya: slice(H - 1, H)}), s)
    elif plant == "border-column-left-out":            # the first column of the grid never enters
        out = dw0 + true - wgrad(win, _masked(grid, **{xa: slice(0, 1)}), s)
    elif plant == "taps-kx-swapped":
        out = dw0 + true.flip(-1)
    elif plant == "odd-pair-second-channel-published":
        # the last pair's absent second channel (the 3-D kernel re-reads the first) is added where its index points: the next grid
        # channel's window channel 0 (the last grid channel's lands behind dw: the GPU test's sentinel)
        out = dw0 + true
        out[1:, 0] += true[:-1, -1]
    elif plant == "list-tensor-skipped":
        keep = [i for i in range(c.n) if i != 1]
        out = dw0 + wgrad(torch.cat([sc.wins[i] for i in keep]).double(), torch.cat([sc.grids[i] for i in keep]).double(), s)
    elif plant == "initial-dw-overwritten":
        out = true
    elif plant == "fold-tail-wave-lost":               # the last wave (b, dc, xs, rc) of group (cog 0, pair 0, depth tap 1) never folded
        dchunk, ndc, rows, nrc, nxs, _ = plan_list[0]
        D = c.dims[0]
        lost = wgrad(win, _masked(grid, a0=slice(c.B - 1, c.B), a2=slice((ndc - 1) * dchunk, D), a3=slice((nrc - 1) * rows, H),
                                  a4=slice((nxs - 1) * 64, W)), s)
        out = dw0 + true
        out[:8, :2, 1] -= lost[:8, :2, 1]
    else:
        raise ValueError(plant)
    return out.float()
