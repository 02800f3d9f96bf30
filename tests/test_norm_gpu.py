"""The normalisation and GRU element-wise entries on the MI355X, called at the C ABI, against tests/norm_scene.py: every smvs_groupnorm1_*
entry, the five smvs_gru_* and smvs_batchnorm_train_fwd / _bwd, one case per class of the kernels' branch rules, forward against the
float64 reference and its per-element bound, then the backward fed with that forward's own outputs.  Exact scenes must EQUAL the
reference; the GRU entries and the fused epilogues must give the bits of their float32 expressions.  Every input is a slice inside an
allocation of NaN; every output, and a workspace of exactly the size the header states, lies between sentinel words that must not move.

SMVS_NORM_RATIOS=<file>: the largest err / bound per entry, scene kind and output is written there when the module finishes
(profiles/norm_bound_ratios.txt is such a file)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import norm_scene as S

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF                                # bits of a quiet NaN no kernel produces
GUARD = 67
LEAD = 64                                            # floats of NaN in front of every input (a multiple of 4: the offsets below decide alignment)
GN_ALL = S.GN_CASES + S.PAIR_CASES
RATIOS = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("these tests need the MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from satmvs_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def ratio_table():
    yield
    path = os.environ.get("SMVS_NORM_RATIOS")
    lines = ["%-28s %-14s %-14s %.4f" % (k + (v,)) for k, v in sorted(RATIOS.items())]
    print("\n".join("norm-ratio " + l for l in lines))
    if path and lines:
        with open(path, "w") as f:
            f.write("# largest err / bound per entry, scene kind and output (tests/test_norm_gpu.py); act-allowance: the share of the\n"
                    "# activation's evaluation allowance (8u y sigmoid, 10u |y| tanh) used beyond the propagated part of the bound\n")
            f.write("\n".join(lines) + "\n")


def note(entry, kind, verdict):
    assert verdict.ok, verdict.messages[0]
    for k, r in verdict.ratios.items():
        RATIOS[(entry, kind, k)] = max(RATIOS.get((entry, kind, k), 0.0), r)


def inside_nan(a, dev, off=0, span=None, starts=None):
    """numpy float32 `a` on the device inside an allocation of NaN, its first element `off` floats past a 16-byte boundary.  With
    span / starts: the rows of a (rows, m) array at the float offsets `starts` of a region of `span` floats (NaN between them)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    span = span or a.size
    host = np.full((LEAD + off + span + LEAD,), np.nan, np.float32)
    if starts is None:
        host[LEAD + off:LEAD + off + a.size] = a.reshape(-1)
    else:
        for row, s in zip(a.reshape(len(starts), -1), starts):
            host[LEAD + off + s:LEAD + off + s + row.size] = row
    buf = torch.from_numpy(host).to(dev)
    assert buf.data_ptr() % 16 == 0
    return buf[LEAD + off:LEAD + off + span]


class Guarded:
    """Outputs as interior slices of one int32 allocation of sentinels: [guard | out | guard | out | ...], every output `off` words past
    a 16-byte boundary.  read() asserts that no word outside the declared writable words changed."""

    def __init__(self, dev, specs):
        pos, self.at = GUARD, {}
        for name, words, off in specs:
            pos = (pos + 3) // 4 * 4 + off
            self.at[name] = (pos, words)
            pos += words + GUARD
        self.big = torch.full((pos,), SENTINEL, dtype=torch.int32, device=dev)
        self.writable = {name: None for name in self.at}

    def f32(self, name):
        o, w = self.at[name]
        return self.big[o:o + w].view(torch.float32)

    def f64(self, name):
        o, w = self.at[name]
        return self.big[o:o + w].view(torch.float64)

    def i64(self, name):
        o, w = self.at[name]
        return self.big[o:o + w].view(torch.int64)

    def ptr(self, name, shift=0):
        return C.c_void_p(self.big.data_ptr() + 4 * (self.at[name][0] + shift))

    def read(self, what):
        bits = self.big.cpu().numpy()
        keep = np.ones(bits.size, bool)
        for name, (o, w) in self.at.items():
            keep[o:o + w] = False if self.writable[name] is None else ~self.writable[name]
        moved = np.flatnonzero(bits[keep] != SENTINEL)
        assert len(moved) == 0, "%s: %d words outside the outputs were written, the first at guarded index %d" % (what, len(moved), int(moved[0]))
        return {name: bits[o:o + w].copy() for name, (o, w) in self.at.items()}


def f32(words):
    return words.view(np.float32)


def stream_of(dev):
    from satmvs_amd import _lib
    return _lib.current_stream(dev)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ---- GroupNorm --------------------------------------------------------------------------------------------------------------------
def gn_inputs(c, sc, dev):
    L = S.gn_layout(c)
    Bi, n = S.internal_B(c), c.C * c.HW
    d = dict(x=inside_nan(sc.x, dev, c.off, span=(Bi - 1) * L.xbs + n + (L.x - c.off), starts=[L.x - c.off + b * L.xbs for b in range(Bi)]),
             dy=inside_nan(sc.dy, dev, c.off), gamma=inside_nan(sc.gamma, dev, 1), beta=inside_nan(sc.beta, dev, 2))
    d["xp"] = C.c_void_p(d["x"].data_ptr() + 4 * (L.x - c.off))
    if c.pair:
        d["gamma2"], d["beta2"] = inside_nan(sc.gamma2, dev, 3), inside_nan(sc.beta2, dev, 1)
    return d


def gn_forward(lib, dev, c, sc, act, inp, epilogue=None, u_odd=False):
    """One forward call of the case's entry (or of its fused form).  -> dict y (Bi, C, HW), mr (Bi, 2)[, out / rh], numpy float32"""
    from satmvs_amd import _lib
    L = S.gn_layout(c)
    Bi, n = S.internal_B(c), c.C * c.HW
    specs = [("y", Bi * n, c.off), ("mr", 2 * Bi, 1), ("ws", 2 * 2 * Bi * S.cdiv(n, S.GN_ELEMS), 0)]
    if epilogue:
        specs.append(("e", (Bi if epilogue == "blend" else c.B) * n, c.off))
    out = Guarded(dev, specs)
    out.f64("ws").fill_(float("nan"))
    st = stream_of(dev)
    head = (inp["xp"],) + (() if c.pair else (L.xbs,)) + (P(inp["gamma"]), P(inp["beta"])) + ((P(inp["gamma2"]), P(inp["beta2"])) if c.pair else ())
    tail = (c.B, c.C, c.HW, st)
    mid = (sc.eps, act, out.ptr("y"), out.ptr("mr"), out.ptr("ws"))
    if epilogue == "blend":
        if u_odd:
            u, ubs, up = inside_nan(sc.u, dev, 1), n, None
        else:                                              # u = the second half of a (Bi, 2C, HW) tensor
            u, ubs = inside_nan(sc.u, dev, c.off, span=2 * n * Bi, starts=[n + 2 * n * b for b in range(Bi)]), 2 * n
            up = C.c_void_p(u.data_ptr() + 4 * n)
        h = inside_nan(sc.h, dev, c.off)
        _lib.call("smvs_groupnorm1_fwd_blend", *head, *mid, up or P(u), ubs, P(h), out.ptr("e"), *tail)
    elif epilogue == "mul":
        h = inside_nan(sc.hm, dev, 0)
        _lib.call("smvs_groupnorm1_pair_fwd_mul", *head, *mid, P(h), out.ptr("e"), *tail)
    else:
        _lib.call("smvs_groupnorm1_pair_fwd" if c.pair else "smvs_groupnorm1_fwd", *head, *mid, *tail)
    torch.cuda.synchronize()
    got = out.read(c.name + " forward")
    res = dict(y=f32(got["y"]).reshape(Bi, c.C, c.HW), mr=f32(got["mr"]).reshape(Bi, 2))
    if epilogue:
        res["e"] = f32(got["e"]).reshape(-1, c.C, c.HW)
    return res


def gn_backward(lib, dev, c, sc, act, inp, y_k, mr_k, y_null=False):
    from satmvs_amd import _lib
    L = S.gn_layout(c)
    Bi, n = S.internal_B(c), c.C * c.HW
    lead = L.dx - c.off                                    # the other half in front of a sliced dx
    span = lead + (Bi - 1) * L.dxbs + n
    specs = [("dx", span, c.off), ("dgamma", c.C, 1), ("dbeta", c.C, 2), ("ws", 2 * 2 * Bi * c.C * S.cdiv(c.HW, S.GN_ELEMS), 0)]
    if c.pair:
        specs += [("dgamma2", c.C, 3), ("dbeta2", c.C, 0)]
    out = Guarded(dev, specs)
    w = np.zeros(span, bool)
    for b in range(Bi):
        w[lead + b * L.dxbs:lead + b * L.dxbs + n] = True
    out.writable["dx"] = w
    out.f64("ws").fill_(float("nan"))
    y = None if y_null else inside_nan(y_k, dev, c.off)
    mr = inside_nan(mr_k, dev, 1)
    st = stream_of(dev)
    if c.pair:
        _lib.call("smvs_groupnorm1_pair_bwd", P(inp["dy"]), inp["xp"], P(y), P(inp["gamma"]), P(inp["gamma2"]), P(mr), act, out.ptr("dx"),
                  out.ptr("dgamma"), out.ptr("dbeta"), out.ptr("dgamma2"), out.ptr("dbeta2"), out.ptr("ws"), c.B, c.C, c.HW, st)
    else:
        _lib.call("smvs_groupnorm1_bwd", P(inp["dy"]), inp["xp"], L.xbs, P(y), P(inp["gamma"]), P(mr), act, out.ptr("dx", lead), L.dxbs,
                  out.ptr("dgamma"), out.ptr("dbeta"), out.ptr("ws"), c.B, c.C, c.HW, st)
    torch.cuda.synchronize()
    got = out.read(c.name + " backward")
    dx = f32(got["dx"])
    res = {k: f32(got[k]) for k in got if k not in ("dx", "ws")}
    res["dx"] = np.stack([dx[lead + b * L.dxbs:lead + b * L.dxbs + n] for b in range(Bi)]).reshape(Bi, c.C, c.HW)
    return res


def same(a, b):
    return all(S.same_bits(a[k], b[k]) for k in a)


@pytest.mark.parametrize("c", GN_ALL, ids=[c.name for c in GN_ALL])
def test_groupnorm_forward_then_backward(lib, dev, c):
    """Every scene kind, every activation of the case: forward against reference and bound (equal on the exact scenes), the backward on
    the forward's outputs against the float64 backward of exactly those; act 0 also with y NULL.  On the real scene both calls are
    repeated and give the same bits (fixed order of the folds)."""
    entry = "groupnorm1_pair" if c.pair else "groupnorm1"
    for kind in S.GN_KINDS:
        if not S.gn_scene_applies(c, kind):
            continue
        sc = S.gn_scene(c, kind)
        inp = gn_inputs(c, sc, dev)
        for act in c.acts:
            f = gn_forward(lib, dev, c, sc, act, inp)
            note(entry + "_fwd", kind, S.gn_judge_fwd(c, kind, act, f["y"], f["mr"]))
            b = gn_backward(lib, dev, c, sc, act, inp, f["y"], f["mr"])
            note(entry + "_bwd", kind, S.gn_judge_bwd(c, kind, act, f["y"], f["mr"], b))
            if act == 0:
                b0 = gn_backward(lib, dev, c, sc, act, inp, f["y"], f["mr"], y_null=True)
                assert same(b, b0), "y == NULL changes the act 0 backward"
            if kind == "real":
                assert same(f, gn_forward(lib, dev, c, sc, act, inp)), "two forward calls differ"
                assert same(b, gn_backward(lib, dev, c, sc, act, inp, f["y"], f["mr"])), "two backward calls differ"


BLEND = [("2x4x1024", False), ("2x4x1024", True), ("1x2x4098", False), ("3x8x100-sliced", False), ("1x2x3", True)]


@pytest.mark.parametrize("name,u_odd", BLEND, ids=["%s-%s" % (n, "u-odd" if o else "u-half") for n, o in BLEND])
def test_groupnorm_fwd_blend_is_the_model_and_the_separate_launches(lib, dev, name, u_odd):
    """tanh, as the cell uses it.  y and mean_rstd: the bits of the plain entry; out: the bits of u h + (1 - u) y on the kernel's y, from
    the float32 expression and from smvs_gru_blend_fwd."""
    c = S.GN_BY_NAME[name]
    sc = S.gn_scene(c, "real")
    inp = gn_inputs(c, sc, dev)
    plain = gn_forward(lib, dev, c, sc, 2, inp)
    fused = gn_forward(lib, dev, c, sc, 2, inp, epilogue="blend", u_odd=u_odd)
    assert S.same_bits(fused["y"], plain["y"]) and S.same_bits(fused["mr"], plain["mr"])
    assert S.same_bits(fused["e"], S.blend_fwd32(sc.u, sc.h, plain["y"]))
    sep = blend_run(lib, dev, sc.dy.reshape(-1), sc.u.reshape(-1), sc.h.reshape(-1), plain["y"].reshape(-1))["out"]
    assert S.same_bits(fused["e"].reshape(-1), sep)
    assert same(fused, gn_forward(lib, dev, c, sc, 2, inp, epilogue="blend", u_odd=u_odd)), "two calls differ"


MUL = ["pair-2x4x1024", "pair-2x3x1366", "pair-3x5x7", "pair-1x8x4100"]


@pytest.mark.parametrize("name", MUL)
def test_groupnorm_pair_fwd_mul_is_the_model_and_the_separate_launches(lib, dev, name):
    """sigmoid.  y: the bits of the pair entry; rh: y[:, :C] * h on the kernel's y, from the float32 expression and from smvs_gru_mul_cat_fwd."""
    c = S.GN_BY_NAME[name]
    sc = S.gn_scene(c, "real")
    inp = gn_inputs(c, sc, dev)
    plain = gn_forward(lib, dev, c, sc, 1, inp)
    fused = gn_forward(lib, dev, c, sc, 1, inp, epilogue="mul")
    assert S.same_bits(fused["y"], plain["y"]) and S.same_bits(fused["mr"], plain["mr"])
    r = np.ascontiguousarray(plain["y"][0::2])
    assert S.same_bits(fused["e"], (r * sc.hm).astype(np.float32))
    sep = mulcat_run(lib, dev, (c.B, 0, c.C, c.HW), np.zeros((c.B, 0, c.HW), np.float32), r, sc.hm, None, None)["out"]
    assert S.same_bits(fused["e"], sep)
    assert same(fused, gn_forward(lib, dev, c, sc, 1, inp, epilogue="mul")), "two calls differ"


def test_groupnorm_nan_stays_in_its_sample(lib, dev):
    c = S.GN_BY_NAME["2x4x1024"]
    sc = S.gn_scene(c, "real")
    clean_in = gn_inputs(c, sc, dev)
    clean = gn_forward(lib, dev, c, sc, 0, clean_in)
    cb = gn_backward(lib, dev, c, sc, 0, clean_in, clean["y"], clean["mr"])
    x = sc.x.copy()
    x[1, 2, 5] = np.nan
    bad = sc._replace(x=x)
    inp = gn_inputs(c, bad, dev)
    f = gn_forward(lib, dev, c, bad, 0, inp)
    assert np.isnan(f["y"][1]).all() and np.isnan(f["mr"][1]).all()
    assert S.same_bits(f["y"][0], clean["y"][0]) and S.same_bits(f["mr"][0], clean["mr"][0])
    b = gn_backward(lib, dev, c, bad, 0, inp, f["y"], f["mr"])
    assert np.isnan(b["dx"][1]).all() and S.same_bits(b["dx"][0], cb["dx"][0])
    assert np.isnan(b["dgamma"]).all()                                         # (a sum over the batch of dy * xhat)
    assert S.same_bits(b["dbeta"], cb["dbeta"])                                # (the sum of dy: x does not enter)


# ---- GRU element-wise entries -------------------------------------------------------------------------------------------------------
def blend_run(lib, dev, dy, u, h, y, backward=False):
    from satmvs_amd import _lib
    n = u.size
    ins = [inside_nan(a, dev) for a in (dy, u, h, y)]
    out = Guarded(dev, [("out", n, 0)] if not backward else [("du", n, 0), ("dh", n, 0), ("dc", n, 0)])
    if backward:
        _lib.call("smvs_gru_blend_bwd", *[P(a) for a in ins], out.ptr("du"), out.ptr("dh"), out.ptr("dc"), n, stream_of(dev))
    else:
        _lib.call("smvs_gru_blend_fwd", *[P(a) for a in ins[1:]], out.ptr("out"), n, stream_of(dev))
    torch.cuda.synchronize()
    return {k: f32(v) for k, v in out.read("gru_blend n=%d" % n).items()}


@pytest.mark.parametrize("n", S.BLEND_N)
def test_gru_blend_gives_the_bits_of_its_expressions(lib, dev, n):
    dy, u, h, y = S.blend_scene(n)
    f = blend_run(lib, dev, dy, u, h, y)
    assert S.same_bits(f["out"], S.blend_fwd32(u, h, y))
    b = blend_run(lib, dev, dy, u, h, y, backward=True)
    for k, want in zip(("du", "dh", "dc"), S.blend_bwd32(dy, u, h, y)):
        assert S.same_bits(b[k], want), k
    assert same(f, blend_run(lib, dev, dy, u, h, y)) and same(b, blend_run(lib, dev, dy, u, h, y, backward=True))


def mulcat_run(lib, dev, m, x, r, h, dcat, dh_acc, which="fwd"):
    from satmvs_amd import _lib
    B, Cx, Ch, HW = m
    nh, nc = B * Ch * HW, B * (Cx + Ch) * HW
    rr, hh = inside_nan(r, dev, 1), inside_nan(h, dev, 2)
    st = stream_of(dev)
    if which == "fwd":
        xx = inside_nan(x if x.size else np.zeros(1, np.float32), dev, 3)
        out = Guarded(dev, [("out", nc, 1)])
        _lib.call("smvs_gru_mul_cat_fwd", P(xx), P(rr), P(hh), out.ptr("out"), B, Cx, Ch, HW, st)
    elif which == "bwd":
        out = Guarded(dev, [("dr", nh, 1), ("dh", nh, 3)])
        _lib.call("smvs_gru_mul_cat_bwd", P(inside_nan(dcat, dev, 3)), P(rr), P(hh), out.ptr("dr"), out.ptr("dh"), B, Cx, Ch, HW, st)
    else:
        out = Guarded(dev, [("dcat", nc, 3), ("dr", nh, 1)])
        out.f32("dcat").copy_(torch.from_numpy(dcat.reshape(-1)))
        _lib.call("smvs_gru_mul_cat_bwd_acc", out.ptr("dcat"), P(rr), P(hh), P(inside_nan(dh_acc, dev, 0)), out.ptr("dr"), B, Cx, Ch, HW, st)
    torch.cuda.synchronize()
    got = {k: f32(v) for k, v in out.read("gru_mul_cat %s %r" % (which, m)).items()}
    for k in got:
        got[k] = got[k].reshape(B, -1, HW)
    return got


@pytest.mark.parametrize("m", S.MULCAT, ids=["x".join(map(str, m)) for m in S.MULCAT])
def test_gru_mul_cat_gives_the_bits_of_its_expressions(lib, dev, m):
    x, r, h, dcat, dh_acc = S.mulcat_scene(m)
    Cx = m[1]
    f = mulcat_run(lib, dev, m, x, r, h, dcat, dh_acc)
    assert S.same_bits(f["out"], S.mulcat_fwd32(x, r, h))
    b = mulcat_run(lib, dev, m, x, r, h, dcat, dh_acc, "bwd")
    dr, dh = S.mulcat_bwd32(dcat, r, h, Cx)
    assert S.same_bits(b["dr"], dr) and S.same_bits(b["dh"], dh)
    a = mulcat_run(lib, dev, m, x, r, h, dcat, dh_acc, "acc")
    dr, ref, bound = S.mulcat_bwd_acc64(dcat, r, h, dh_acc, Cx)
    assert S.same_bits(a["dr"], dr)
    assert S.same_bits(a["dcat"][:, :Cx], dcat[:, :Cx]), "bwd_acc touched dx"
    rep = S.check(a["dcat"][:, Cx:], ref, bound, "bwd_acc dcat")
    assert rep.ok, rep.message
    RATIOS[("gru_mul_cat_bwd_acc", "real", "dcat")] = max(RATIOS.get(("gru_mul_cat_bwd_acc", "real", "dcat"), 0.0), rep.ratio)
    for which, first in (("fwd", f), ("bwd", b), ("acc", a)):
        assert same(first, mulcat_run(lib, dev, m, x, r, h, dcat, dh_acc, which)), which + ": two calls differ"


# ---- BatchNorm ----------------------------------------------------------------------------------------------------------------------
def bn_inputs(c, sc, dev):
    return dict(x=inside_nan(sc.x, dev, c.off), dy=inside_nan(sc.dy, dev, c.off), gamma=inside_nan(sc.gamma, dev, 1), beta=inside_nan(sc.beta, dev, 3))


def bn_forward(lib, dev, c, sc, relu, inp, running=True, flag=False):
    from satmvs_amd import _lib
    n = c.B * c.C * c.N
    out = Guarded(dev, [("y", n, c.off), ("saved", 2 * c.C, 1), ("rm", c.C, 1), ("rv", c.C, 3), ("nbt", 2, 0), ("ws", 2 * 2 * c.C, 0)])
    if running:
        out.f32("rm").copy_(torch.from_numpy(sc.rm))
        out.f32("rv").copy_(torch.from_numpy(sc.rv))
        out.i64("nbt").fill_(7)
    out.f64("ws").fill_(0.0 if flag else float("nan"))       # with the flag the caller zeroes; without it the call clears whatever is there
    if not running:
        for k in ("rm", "rv", "nbt"):
            out.writable[k] = np.zeros(out.at[k][1], bool)
    _lib.call("smvs_batchnorm_train_fwd", P(inp["x"]), P(inp["gamma"]), P(inp["beta"]), out.ptr("rm") if running else None,
              out.ptr("rv") if running else None, out.ptr("nbt") if running else None, sc.momentum, sc.eps,
              relu | (S.BN_WORKSPACE_ZERO if flag else 0), out.ptr("y"), out.ptr("saved"), out.ptr("ws"), c.B, c.C, c.N, stream_of(dev))
    torch.cuda.synchronize()
    got = out.read("bn %s forward" % c.name)
    res = dict(y=f32(got["y"]).reshape(c.B, c.C, c.N), saved=f32(got["saved"]).reshape(c.C, 2))
    if running:
        res.update(rm=f32(got["rm"]), rv=f32(got["rv"]))
        assert int(got["nbt"].view(np.int64)[0]) == 8, "num_batches_tracked"
    return res


def bn_backward(lib, dev, c, sc, relu, inp, saved_k, flag=False):
    from satmvs_amd import _lib
    n = c.B * c.C * c.N
    out = Guarded(dev, [("dx", n, c.off), ("dgamma", c.C, 1), ("dbeta", c.C, 2), ("ws", 2 * 2 * c.C, 0)])
    out.f64("ws").fill_(0.0 if flag else float("nan"))
    saved = inside_nan(saved_k, dev, 1)
    _lib.call("smvs_batchnorm_train_bwd", P(inp["dy"]), P(inp["x"]), P(inp["gamma"]), P(inp["beta"]), P(saved),
              relu | (S.BN_WORKSPACE_ZERO if flag else 0), out.ptr("dx"), out.ptr("dgamma"), out.ptr("dbeta"), out.ptr("ws"), c.B, c.C, c.N,
              stream_of(dev))
    torch.cuda.synchronize()
    got = out.read("bn %s backward" % c.name)
    return dict(dx=f32(got["dx"]).reshape(c.B, c.C, c.N), dgamma=f32(got["dgamma"]), dbeta=f32(got["dbeta"]))


@pytest.mark.parametrize("c", S.BN_CASES, ids=[c.name for c in S.BN_CASES])
def test_batchnorm_forward_then_backward(lib, dev, c):
    """Every scene kind with and without ReLU: once with running statistics and num_batches_tracked and a NaN workspace the call clears,
    once without them and with SMVS_BN_WORKSPACE_ZERO on a workspace the caller zeroed; the real scene also the two other pairings."""
    for kind in S.BN_KINDS:
        if not S.bn_scene_applies(c, kind):
            continue
        sc = S.bn_scene(c, kind)
        inp = bn_inputs(c, sc, dev)
        for relu in (0, 1):
            ref = S.bn_ref_fwd(sc, relu)
            for running, flag in [(True, False), (False, True)] + ([(True, True), (False, False)] if kind == "real" else []):
                f = bn_forward(lib, dev, c, sc, relu, inp, running, flag)
                note("batchnorm_train_fwd", kind, S.bn_judge_fwd(c, kind, relu, f, running, ref))
                b = bn_backward(lib, dev, c, sc, relu, inp, f["saved"], flag)
                note("batchnorm_train_bwd", kind, S.bn_judge_bwd(c, kind, relu, f["y"], f["saved"], b))


def test_batchnorm_nan_stays_in_its_channel(lib, dev):
    c = S.BN_BY_NAME["3x5x4100"]
    sc = S.bn_scene(c, "real")
    x = sc.x.copy()
    x[1, 1, 77] = np.nan
    bad = sc._replace(x=x)
    inp = bn_inputs(c, bad, dev)
    ref = S.bn_ref_fwd(sc, 1)
    f = bn_forward(lib, dev, c, bad, 1, inp)
    others = [k for k in range(c.C) if k != 1]
    assert np.isnan(f["y"][:, 1]).all() and np.isnan(f["saved"][1]).all() and np.isnan(f["rm"][1]) and np.isnan(f["rv"][1])
    for name, got, r, e in (("y", f["y"][:, others], ref["y"][:, others], ref["E_y"][:, others]),
                            ("rstd", f["saved"][others, 1], ref["rstd"][others], ref["E_rstd"][others]),
                            ("running_mean", f["rm"][others], ref["rm"][others], ref["E_rm"][others]),
                            ("running_var", f["rv"][others], ref["rv"][others], ref["E_rv"][others])):
        rep = S.check(got, r, e, "bn nan " + name)
        assert rep.ok, rep.message
    b = bn_backward(lib, dev, c, bad, 1, inp, f["saved"])
    back = S.bn_ref_bwd(sc, 1, f["y"], np.nan_to_num(f["saved"]))
    assert np.isnan(b["dx"][:, 1]).all() and np.isnan(b["dgamma"][1])
    assert b["dbeta"][1] == 0.0                            # (the ReLU mask of a NaN output is closed: no dy passes, and x does not enter)
    for k in ("dgamma", "dbeta"):
        rep = S.check(b[k][others], back[k][others], back["E_" + k][others], "bn nan " + k)
        assert rep.ok, rep.message
    rep = S.check(b["dx"][:, others], back["dx"][:, others], back["E_dx"][:, others], "bn nan dx")
    assert rep.ok, rep.message


# ---- a side stream ------------------------------------------------------------------------------------------------------------------
def test_one_case_of_each_family_on_a_side_stream(lib, dev):
    """The entries take their stream from the argument: the same verdicts with the calls on a stream of their own."""
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        c = S.GN_BY_NAME["1x2x4098"]
        sc = S.gn_scene(c, "real")
        inp = gn_inputs(c, sc, dev)
        f = gn_forward(lib, dev, c, sc, 1, inp)
        assert S.gn_judge_fwd(c, "real", 1, f["y"], f["mr"]).ok
        assert S.gn_judge_bwd(c, "real", 1, f["y"], f["mr"], gn_backward(lib, dev, c, sc, 1, inp, f["y"], f["mr"])).ok
        c = S.GN_BY_NAME["pair-2x3x1366"]
        sc = S.gn_scene(c, "real")
        inp = gn_inputs(c, sc, dev)
        f = gn_forward(lib, dev, c, sc, 1, inp)
        assert S.gn_judge_fwd(c, "real", 1, f["y"], f["mr"]).ok
        assert S.gn_judge_bwd(c, "real", 1, f["y"], f["mr"], gn_backward(lib, dev, c, sc, 1, inp, f["y"], f["mr"])).ok
        dy, u, h, y = S.blend_scene(2051)
        assert S.same_bits(blend_run(lib, dev, dy, u, h, y)["out"], S.blend_fwd32(u, h, y))
        m = S.MULCAT[4]
        x, r, h, dcat, dh_acc = S.mulcat_scene(m)
        assert S.same_bits(mulcat_run(lib, dev, m, x, r, h, dcat, dh_acc)["out"], S.mulcat_fwd32(x, r, h))
        c = S.BN_BY_NAME["3x2x16388"]
        sc = S.bn_scene(c, "real")
        inp = bn_inputs(c, sc, dev)
        f = bn_forward(lib, dev, c, sc, 1, inp)
        assert S.bn_judge_fwd(c, "real", 1, f).ok
        assert S.bn_judge_bwd(c, "real", 1, f["y"], f["saved"], bn_backward(lib, dev, c, sc, 1, inp, f["saved"])).ok
    torch.cuda.synchronize()
