"""The weight-gradient entries of csrc/conv_wgrad.hip on the MI355X, called at the C ABI: smvs_conv3x3_wgrad, _strided, _cat, _list and
smvs_conv3d_wgrad in its atomic and its two-stage form, one case per class of the split (tests/wgrad_scene.py).  Integer scenes must
EQUAL the float64 reference (every partial sum is an integer below 2^24: no order of lanes, atomics or fold can round); real scenes are
held weight by weight to
    |got - ref| <= (n + 2) 2^-24 (|init| + sum |terms|) + n 2^-126
and nothing else.  Every operand is a slice inside a larger allocation: NaN around the inputs (an over-read stays in owned memory and
shows if it reaches a published sum), a sentinel around dw, db and the workspace."""
import ctypes as C

import numpy as np
import pytest
import torch

import wgrad_scene as S

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF                                # bits of a quiet NaN no kernel produces
GUARD = 67                                           # guard words around every output (odd: the outputs are 4-byte aligned only)
IDS = [c.name for c in S.CASES]
IDS_3D = [c.name for c in S.CASES_3D]


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


@pytest.fixture(scope="module")
def queries(lib):
    def plan2(*a):
        p = (C.c_int * 6)()
        return lib.smvs_conv3x3_wgrad_plan(*a, p), list(p)

    def plan3(*a):
        p = (C.c_int * 6)()
        return lib.smvs_conv3d_wgrad_plan(*a, p), list(p)
    return plan2, plan3


def inside_nan(t, dev):
    """t on the device as a slice in the interior of an allocation filled with NaN: eight channels (planes / volumes) and 65 floats
    of NaN on either side -- further than any descriptor of the kernels reaches past its operand."""
    if t is None:
        return None
    pad = 8 * int(np.prod(t.shape[2:])) + 65
    buf = torch.full((pad + t.numel() + pad,), float("nan"), dtype=torch.float32, device=dev)
    buf[pad:pad + t.numel()] = t.reshape(-1).to(dev)
    return buf[pad:pad + t.numel()].view(t.shape)


class Outputs:
    """dw, db and (two-stage form) the workspace as interior slices of one int32 allocation of sentinels:
    [guard | dw | guard | db | guard | workspace | guard]; the workspace prefilled with NaN."""

    def __init__(self, c, dw0, db0, ws_floats, dev):
        self.n_dw, self.n_db, self.n_ws = dw0.numel(), c.Cgrid, ws_floats
        self.o_dw = GUARD
        self.o_db = self.o_dw + self.n_dw + GUARD
        self.o_ws = self.o_db + self.n_db + GUARD
        self.big = torch.full((self.o_ws + self.n_ws + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        f = self.big.view(torch.float32)
        self.dw = f[self.o_dw:self.o_dw + self.n_dw].view(dw0.shape)
        self.dw.copy_(dw0.to(dev))
        self.db = None
        if c.db:
            self.db = f[self.o_db:self.o_db + self.n_db]
            self.db.copy_(db0.to(dev))
        self.ws = None
        if ws_floats:
            self.ws = f[self.o_ws:self.o_ws + self.n_ws]
            self.ws.fill_(float("nan"))
        self.has_db = c.db

    def read(self, name):
        """-> (dw, db or None) float32 on the CPU, after asserting that nothing but dw, db (where given) and the workspace changed"""
        bits = self.big.cpu()
        keep = torch.ones(bits.numel(), dtype=torch.bool)
        keep[self.o_dw:self.o_dw + self.n_dw] = False
        if self.has_db:
            keep[self.o_db:self.o_db + self.n_db] = False
        keep[self.o_ws:self.o_ws + self.n_ws] = False
        moved = torch.nonzero(bits[keep] != SENTINEL)
        assert len(moved) == 0, "%s: %d words beside dw / db / the workspace were written, the first at guarded index %d" % (name, len(moved), int(moved[0]))
        f = bits.view(torch.float32)
        dw = f[self.o_dw:self.o_dw + self.n_dw].view(self.dw.shape).clone()
        return dw, (f[self.o_db:self.o_db + self.n_db].clone() if self.has_db else None)


def run(lib, c, sc, dev, queries, form=None, calls=1):
    """`calls` calls of case c's entry on scene sc.  -> (dw, db or None) on the CPU."""
    from satmvs_amd import _lib
    form = form or c.form
    ws_floats = 0
    if form == "two_stage":
        D, H, W = c.dims
        ws_floats = lib.smvs_conv3d_wgrad_workspace_floats(c.B, S.cwin(c), c.Cgrid, D, H, W)
        assert ws_floats == S.workspace_floats(c, S.plans(c, *queries, form="two_stage")[0]) > 0
    out = Outputs(c, sc.dw0, sc.db0, ws_floats, dev)
    if c.CB:
        wins = [inside_nan(w[:, :c.CA].contiguous(), dev) for w in sc.wins]
        wins2 = [inside_nan(w[:, c.CA:].contiguous(), dev) for w in sc.wins]
    else:
        wins, wins2 = [inside_nan(w, dev) for w in sc.wins], None
    grids = [inside_nan(g, dev) for g in sc.grids]
    st = _lib.current_stream(dev)
    p = lambda v: _lib.ptr(v) if v is not None else None
    H, W = c.dims[-2:]
    for _ in range(calls):
        if c.entry == "wgrad":
            _lib.call("smvs_conv3x3_wgrad", p(wins[0]), p(grids[0]), p(out.dw), p(out.db), c.B, c.CA, c.Cgrid, H, W, st)
        elif c.entry == "strided":
            _lib.call("smvs_conv3x3_wgrad_strided", p(wins[0]), p(grids[0]), p(out.dw), p(out.db), c.B, c.CA, c.Cgrid, H, W, c.stride, st)
        elif c.entry == "cat":
            _lib.call("smvs_conv3x3_wgrad_cat", p(wins[0]), c.CA, p(wins2[0]) if wins2 else None, c.CB, p(grids[0]), p(out.dw), p(out.db),
                      c.B, c.Cgrid, H, W, st)
        elif c.entry == "list":
            _lib.call("smvs_conv3x3_wgrad_list", _lib.ptr_array(wins), _lib.ptr_array(wins2) if wins2 else None, _lib.ptr_array(grids), c.n,
                      p(out.dw), p(out.db), c.Bper, c.CA, c.CB, c.Cgrid, H, W, c.stride, st)
        else:
            _lib.call("smvs_conv3d_wgrad", p(wins[0]), p(grids[0]), p(out.dw), p(out.ws), ws_floats, c.B, c.CA, c.Cgrid, c.dims[0], H, W,
                      c.stride, st)
    torch.cuda.synchronize()
    return out.read(c.name)


def bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("c", S.CASES, ids=IDS)
def test_integer_scenes_equal_the_reference(lib, dev, queries, c):
    """Every case, every entry: dw (and db where given) equal the float64 reference rounded to float32; the words around dw and db keep
    their bits, and with db NULL the place of db as well (Outputs.read asserts both)."""
    ref = S.reference(c, "int")
    dw, db = run(lib, c, S.scene(c, "int"), dev, queries)
    ok, ratio, msg = S.check_case(c, "int", dw, db)
    assert ok, msg
    assert torch.equal(dw, ref.dw.float())
    assert (db is None) == (not c.db)
    if c.db:
        assert torch.equal(db, ref.db.float())


@pytest.mark.parametrize("c", S.CASES, ids=IDS)
def test_real_scenes_inside_the_bound(lib, dev, queries, c):
    """Every case: every weight (and bias sum) inside its own bound.  Prints the worst err / bound of the case."""
    dw, db = run(lib, c, S.scene(c, "real"), dev, queries)
    ok, ratio, msg = S.check_case(c, "real", dw, db)
    print("wgrad-ratio %-24s %-9s %.4f" % (c.name, c.form or "-", ratio))
    assert ok, msg


@pytest.mark.parametrize("c", S.CASES, ids=IDS)
def test_two_calls_accumulate(lib, dev, queries, c):
    """dw and db are added to: two calls on an integer scene give exactly the initial value plus twice the sums."""
    sc = S.scene(c, "int")
    ref = S.reference_of(c, sc, "int", calls=2)
    dw, db = run(lib, c, sc, dev, queries, calls=2)
    assert torch.equal(dw, ref.dw.float()), S.check(dw, ref.dw, ref.dw_bound, c.name + " dw").message
    if c.db:
        assert torch.equal(db, ref.db.float()), S.check(db, ref.db, ref.db_bound, c.name + " db").message


def test_list_of_65_equals_65_single_calls(lib, dev, queries):
    """The list form continues past one launch's table of 64 tensors: on an integer scene its result equals, exactly, 65 single calls
    that hand dw and db on from one to the next."""
    c = S.BY_NAME["list-n65"]
    sc = S.scene(c, "int")
    assert c.n == 65 and c.db
    listed = run(lib, c, sc, dev, queries)
    one = c._replace(entry="strided", B=c.Bper, n=None, Bper=None)
    dw, db = sc.dw0, sc.db0
    for w, g in zip(sc.wins, sc.grids):
        dw, db = run(lib, one, S.Scene([w], [g], dw, db), dev, queries)
    assert torch.equal(listed[0], dw) and torch.equal(listed[1], db)
    assert torch.equal(dw, S.reference(c, "int").dw.float())


@pytest.mark.parametrize("c", S.CASES_3D, ids=IDS_3D)
def test_two_stage_form(lib, dev, queries, c):
    """Every 3-D case with a workspace of exactly smvs_conv3d_wgrad_workspace_floats floats, prefilled with NaN, between sentinels (run
    and Outputs.read assert the size and the sentinels): exact on the integer scene and equal to the atomic form there; on the real
    scene inside the bound, and two runs give equal bits."""
    sc = S.scene(c, "int")
    ref = S.reference(c, "int")
    two, _ = run(lib, c, sc, dev, queries, form="two_stage")
    assert torch.equal(two, ref.dw.float()), S.check(two, ref.dw, ref.dw_bound, c.name + " two-stage dw").message
    atomic, _ = run(lib, c, sc, dev, queries, form="atomic")
    assert torch.equal(bits(atomic), bits(two)), S.check(atomic, ref.dw, ref.dw_bound, c.name + " atomic dw").message
    real = S.scene(c, "real")
    a, _ = run(lib, c, real, dev, queries, form="two_stage")
    b, _ = run(lib, c, real, dev, queries, form="two_stage")
    assert torch.equal(bits(a), bits(b)), "two runs of the two-stage form differ"
    ok, ratio, msg = S.check_case(c, "real", a, None)
    print("wgrad-ratio %-24s %-9s %.4f" % (c.name, "two_stage", ratio))
    assert ok, msg
    if c.form == "two_stage":                          # (the real-scene test above ran the case's own form; here is the other)
        a, _ = run(lib, c, real, dev, queries, form="atomic")
        ok, ratio, msg = S.check_case(c, "real", a, None)
        print("wgrad-ratio %-24s %-9s %.4f" % (c.name, "atomic", ratio))
        assert ok, msg


# 2-D with a single and a two-operand window (several row chunks and column strips; a list across tensors), 3-D with one and with
# eight grid channels per wave, in both forms
LOCAL = [("h17-w65-cout9", None), ("cat-cb3", None), ("list-s2-t-cat", None), ("gc1-s1-h5", "atomic"), ("gc1-two-ndc5-nrc2", "two_stage"),
         ("cg9-h6-d5", "two_stage"), ("s2-t-odd", "atomic")]


@pytest.mark.parametrize("name,form", LOCAL, ids=[n for n, _ in LOCAL])
def test_non_finite_values_stay_local(lib, dev, queries, name, form):
    """Integer scene.  A NaN at an interior and at a corner position of one window channel (the last: the second operand's where there
    are two): NaN exactly the weights the float64 reference makes NaN -- that channel's taps that reach the position -- and every other
    weight, and db, exact.  A NaN at an interior position of one grid channel: NaN that channel's rows of dw and its db, the rest exact."""
    c = S.BY_NAME[name]
    sc = S.scene(c, "int")
    li = len(sc.wins) - 1
    wd = tuple(sc.wins[0].shape[2:])
    for pos in (tuple(d // 2 for d in wd), tuple(d - 1 for d in wd), (0,) * len(wd)):
        wins = [w.clone() for w in sc.wins]
        wins[li][(0, S.cwin(c) - 1) + pos] = float("nan")
        bad = S.Scene(wins, sc.grids, sc.dw0, sc.db0)
        ref = S.reference_of(c, bad, "int")
        want = torch.isnan(ref.dw)
        assert bool(want.any()) and not bool(want[:, :-1].any()) and bool((want == want[:1]).all())
        dw, db = run(lib, c, bad, dev, queries, form=form)
        assert torch.equal(torch.isnan(dw), want), (name, pos, int(torch.isnan(dw).sum()), int(want.sum()))
        assert torch.equal(dw[~want], ref.dw.float()[~want])
        if c.db:
            assert torch.equal(db, ref.db.float())
    grids = [g.clone() for g in sc.grids]
    gch = c.Cgrid // 2
    gpos = tuple(min(1, d - 1) for d in c.dims)
    grids[0][(0, gch) + gpos] = float("nan")
    bad = S.Scene(sc.wins, grids, sc.dw0, sc.db0)
    ref = S.reference_of(c, bad, "int")
    want = torch.zeros_like(ref.dw, dtype=torch.bool)
    want[gch] = True
    # the taps that have a term at the position must be NaN; a tap whose window position there is outside has none (the kernel
    # multiplies the zero of a row or column outside, which makes NaN too, and skips a plane outside, which does not): NaN or exact
    must = torch.zeros_like(want)
    for k in np.ndindex(*(3,) * len(c.dims)):
        if all(0 <= c.stride * p_ + k_ - 1 < c.stride * d for p_, k_, d in zip(gpos, k, c.dims)):
            must[(gch, slice(None)) + k] = True
    assert bool(must.any())
    dw, db = run(lib, c, bad, dev, queries, form=form)
    got = torch.isnan(dw)
    assert bool((got & ~want).sum() == 0) and bool((must & ~got).sum() == 0), (name, "grid", int(got.sum()), int(must.sum()), int(want.sum()))
    exact = S.reference(c, "int").dw.float()
    assert torch.equal(dw[~got], torch.where(want, exact, ref.dw.float())[~got])
    if c.db:
        assert bool(torch.isnan(db[gch])) and int(torch.isnan(db).sum()) == 1
        keep = torch.arange(c.Cgrid) != gch
        assert torch.equal(db[keep], ref.db.float()[keep])
