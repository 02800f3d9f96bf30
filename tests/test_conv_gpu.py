"""smvs_conv3x3_fwd (csrc/red.hip, csrc/mfma_conv.h) and smvs_conv3d_fwd (csrc/costreg.hip) on the MI355X, one case per kernel variant and
remainder class (tests/conv_scene.py), each held element by element to the float64 layer under the derived bound
    |got - ref| <= (n + 2) 2^-24 (A + |init| + |bias|) + n 2^-126
(no element excused), with the variant that ran asserted through the library's own selection functions.  Operands are the last floats of
their tensors behind 4-byte offsets (the caching allocator still pads behind them, see at_end); `out` lies between guard words inside a larger buffer filled with a NaN of known payload."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_scene as S

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF                                # bits of a quiet NaN no kernel produces
WORST = {}                                           # (entry, variant code) -> largest err / bound seen by the forward test


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
def _report_worst_ratios():
    """Prints (it asserts nothing: the forward test does) the largest err / bound per variant over the forward cases that ran --
    the table the README quotes."""
    yield
    for (nd, code), r in sorted(WORST.items()):
        print("conv-worst %dd %-24s %.3f" % (nd, (S.NAMES_2D if nd == 2 else S.NAMES_3D)[code], r))


def at_end(t, dev, lead):
    """t on the device as the LAST numel floats of a tensor of lead + numel floats: a storage offset of `lead` floats (4-byte aligned
    only when lead is odd) and nothing requested behind it.  torch's caching allocator rounds blocks to 512 bytes and carves them out
    of larger segments, so this is NOT the end of a device allocation: an over-read of a few floats lands in mapped memory and shows
    in no trace.  What does catch one here: every kernel reads its features through buffer descriptors sized to the operand, so a
    read past the end returns zero and the result leaves the bound."""
    if t is None:
        return None
    buf = torch.empty(lead + t.numel(), dtype=torch.float32, device=dev)
    buf[lead:] = t.reshape(-1).to(dev)
    return buf[lead:].view(t.shape)


def variant(lib, c, bias_aligned=True):
    if len(c.dims) == 2:
        return lib.smvs_conv3x3_variant(c.kind, c.B, c.CA, c.CB, c.Cout, c.dims[0], c.dims[1], 1 if bias_aligned else 0)
    return lib.smvs_conv3d_variant(c.kind, c.B, c.CA, c.Cout, *c.dims)


def pack(lib, c, w, dev):
    from satmvs_amd import _lib
    nd = len(c.dims)
    cin = c.CA + c.CB
    name = "smvs_conv3x3" if nd == 2 else "smvs_conv3d"
    packed = torch.empty(getattr(lib, name + "_packed_floats")(cin, c.Cout), dtype=torch.float32, device=dev)
    wd = w.to(dev).contiguous()
    _lib.call(name + "_pack", _lib.ptr(wd), _lib.ptr(packed), cin, c.Cout, c.layout, _lib.current_stream(dev))
    return packed


def run(lib, c, t, dev, alias_init=False, relu=None, check=True):
    """One call of the entry for case c on the CPU tensors t.  -> out (CPU float32).  Asserts the guard words around `out` and that
    the call wrote every element of it."""
    from satmvs_amd import _lib
    nd = len(c.dims)
    relu = c.relu if relu is None else relu
    od = (c.B, c.Cout) + S.out_dims(c)
    n = int(np.prod(od))
    guard = 64 if (c.kind == 2 or nd == 3) else 67           # the transposed kernels store float2: `out` stays 8-byte aligned there
    big = torch.full((guard + n + guard,), SENTINEL, dtype=torch.int32, device=dev)
    out = big[guard:guard + n].view(torch.float32).view(od)
    xa = at_end(t["xa"], dev, 1)
    xb = at_end(t["xb"], dev, 3)
    packed = pack(lib, c, t["w"], dev)
    init = t["init"]
    if alias_init:
        out.copy_(init.to(dev))
        init_d = out
    else:
        init_d = at_end(init, dev, 2 if nd == 3 else 5)      # 3-D `skip` is read as float2 by the transposed kernels
    bias_d = None
    if t["bias"] is not None:
        bbuf = torch.zeros(c.Cout + 4, dtype=torch.float32, device=dev)
        lead = 1 if c.bias == "off4" else 0
        assert bbuf.data_ptr() % 16 == 0
        bias_d = bbuf[lead:lead + c.Cout]
        bias_d.copy_(t["bias"].to(dev))
    st = _lib.current_stream(dev)
    p = lambda v: _lib.ptr(v) if v is not None else None
    if nd == 2:
        _lib.call("smvs_conv3x3_fwd", c.kind, p(xa), c.CA, p(xb), c.CB, p(packed), p(bias_d), p(init_d), p(out), c.B, c.Cout,
                  c.dims[0], c.dims[1], 1 if relu else 0, st)
    else:
        _lib.call("smvs_conv3d_fwd", c.kind, p(xa), p(packed), p(init_d), p(out), c.B, c.CA, c.Cout, c.dims[0], c.dims[1], c.dims[2],
                  1 if relu else 0, st)
    torch.cuda.synchronize()
    bits = big.cpu()
    if check:
        assert bool((bits[:guard] == SENTINEL).all()) and bool((bits[guard + n:] == SENTINEL).all()), "guard words around out were written"
        assert not bool((bits[guard:guard + n] == SENTINEL).any()), "elements of out were not written"
    return bits[guard:guard + n].view(torch.float32).view(od).clone()


ALL = [c for c in S.CASES_2D] + [c for c in S.CASES_3D]
IDS = [("2d-" if len(c.dims) == 2 else "3d-") + c.name for c in ALL]


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_forward_every_element_inside_the_bound(lib, dev, c):
    """Every case: the variant meant ran, every element inside the bound, guard words untouched, `out` fully written, and a second call
    returns the same bits."""
    assert variant(lib, c, c.bias != "off4") == c.expect
    t = S.inputs(c)
    ref, bound = S.reference(c)
    got = run(lib, c, t, dev)
    ratio, where = S.worst_ratio(got, ref, bound)
    key = (len(c.dims), c.expect)
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print("conv-ratio %s %-28s %.4f at %s" % ("2d" if len(c.dims) == 2 else "3d", c.name, ratio, where))
    assert ratio <= 1.0, (c.name, ratio, where, float(got[where]), float(ref[where]), float(bound[where]))
    again = run(lib, c, t, dev)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two calls differ"


@pytest.mark.parametrize("c", [c for c in S.CASES_2D if c.init], ids=[c.name for c in S.CASES_2D if c.init])
def test_init_may_alias_out(lib, dev, c):
    """`init` in a buffer of its own and `init` = `out`: equal bits, both inside the bound."""
    t = S.inputs(c)
    ref, bound = S.reference(c)
    sep = run(lib, c, t, dev)
    ali = run(lib, c, t, dev, alias_init=True, check=False)
    assert torch.equal(sep.view(torch.int32), ali.view(torch.int32))
    assert S.worst_ratio(ali, ref, bound)[0] <= 1.0


def _first_per_variant(cases, pred=lambda c: True):
    seen, out = set(), []
    for c in cases:
        if c.expect not in seen and pred(c):
            seen.add(c.expect)
            out.append(c)
    return out


OPTION_CASES = _first_per_variant(S.CASES_2D, lambda c: c.kind != 2 and min(c.dims) > 2)


@pytest.mark.parametrize("c", OPTION_CASES, ids=[c.name for c in OPTION_CASES])
def test_relu_and_bias_on_and_off(lib, dev, c):
    """The four combinations of ReLU and bias (aligned) on one case of every 2-D correlation variant."""
    t0 = S.inputs(c)
    g = torch.Generator().manual_seed(5)
    for relu in (False, True):
        for has_bias in (False, True):
            cc = c._replace(relu=relu, bias="aligned" if has_bias else None)
            t = dict(t0, bias=torch.randn((c.Cout,), generator=g) if has_bias else None)
            assert c.bias != "off4" and variant(lib, cc) == c.expect
            ref = S.layer(cc, t)
            x = t["xa"] if t["xb"] is None else torch.cat([t["xa"], t["xb"]], 1)
            A = S.linear_part(c.kind, c.layout, x.double().abs(), t["w"].double().abs())
            bound = S.bound_from(S.taps(c), A, t["init"], t["bias"])
            got = run(lib, cc, t, dev)
            assert S.worst_ratio(got, ref, bound)[0] <= 1.0, (c.name, relu, has_bias)
            if relu:
                assert float(got.min()) >= 0.0


# layer, dims of x, (Ci, Co) of the layer whose input gradient is taken: direct and MFMA adjoints
# ... and the variant each adjoint call must run
ADJOINTS = [("c1", (7, 65), 3, 5, S.SPLIT_S1), ("c1", (6, 33), 32, 8, S.MFMA_S1 + S.K4), ("c2", (6, 130), 3, 5, S.T_SPLIT),
            ("t2", (5, 33), 5, 3, S.SPLIT_S2), ("t2", (5, 33), 32, 8, S.MFMA_S2 + S.K4),
            ("c1", (3, 4, 63), 3, 2, S.D3_S1_COT8), ("c1", (3, 3, 33), 32, 8, S.MFMA_S1 + S.K4), ("c2", (4, 6, 66), 3, 9, S.D3_T_SPLIT),
            ("t2", (2, 3, 33), 9, 3, S.D3_S2), ("t2", (2, 3, 33), 32, 8, S.MFMA_S2 + S.K4)]


@pytest.mark.parametrize("name,dims,ci,co,expect", ADJOINTS, ids=["%s-%dd-ci%d-co%d" % (a[0], len(a[1]), a[2], a[3]) for a in ADJOINTS])
def test_input_gradient_through_the_adjoint_layouts(lib, dev, name, dims, ci, co, expect):
    """The input gradient of each layer kind as the library's backward computes it -- the entry with layouts 2 (stride-1 correlation), 1
    (stride-2 correlation) and 0 (stride-2 transposed layer) -- against the float64 input gradient, n from the channels of dy."""
    nd = len(dims)
    g = torch.Generator().manual_seed(11 * ci + co + nd)
    w = torch.randn(((ci, co) if name == "t2" else (co, ci)) + (3,) * nd, generator=g) / (3.0 ** nd * co) ** 0.5
    x_shape = (2, ci) + tuple(dims)
    dy = torch.randn(S.forward_of(name, torch.zeros(x_shape), w).shape, generator=g)
    ref, bound = S.adjoint_reference(name, x_shape, w, dy)
    kind, layout = S.ADJOINT_OF[name]
    c = S.Case("adjoint", kind, layout, 2, co, 0, ci, tuple(dy.shape[2:]), None, False, False, False, expect)
    assert variant(lib, c) == expect
    got = run(lib, c, {"xa": dy, "xb": None, "w": w, "bias": None, "init": None}, dev)
    assert got.shape == ref.shape
    ratio, where = S.worst_ratio(got, ref, bound)
    assert ratio <= 1.0, (ratio, where)


# per variant the first hot case whose last tile of a row is partial, so that the Inf in the last column sits next to idle lanes
LOCAL_CASES = _first_per_variant(S.CASES_2D, lambda c: c.hot and S.ragged(c)) + _first_per_variant(S.CASES_3D, lambda c: c.hot and S.ragged(c))
assert len(LOCAL_CASES) == len(S.ALL_CODES_2D) + len(S.ALL_CODES_3D)


@pytest.mark.parametrize("c", LOCAL_CASES, ids=[("2d-" if len(c.dims) == 2 else "3d-") + c.name for c in LOCAL_CASES])
def test_non_finite_values_stay_local(lib, dev, c):
    """One NaN in x: NaN exactly the outputs whose window contains it, in every output channel, every other output keeps its bits.
    One Inf in the last column (next to the ragged tile edge): non-finite exactly the outputs whose window contains it; the guard
    words beside `out` stay as they were (run() asserts that)."""
    t0 = S.inputs(c)
    base = run(lib, c, t0, dev, relu=False)
    x0 = t0["xa"]
    for value, pos in ((float("nan"), tuple(d // 2 for d in c.dims)), (float("inf"), tuple(d - 1 for d in c.dims))):
        idx = (c.B - 1, 0) + pos
        xa = x0.clone()
        xa[idx] = value
        ind = torch.zeros((c.B, c.CA + c.CB) + c.dims, dtype=torch.float64)
        ind[idx] = 1.0
        hit = S.linear_part(c.kind, c.layout, ind, torch.ones_like(t0["w"], dtype=torch.float64)) > 0
        assert bool(hit.any()) and bool((hit == hit[:, :1]).all())
        got = run(lib, c, dict(t0, xa=xa), dev, relu=False)
        bad = torch.isnan(got) if value != value else ~torch.isfinite(got)
        assert torch.equal(bad, hit), (c.name, value, int(bad.sum()), int(hit.sum()))
        assert torch.equal(got.view(torch.int32)[~hit], base.view(torch.int32)[~hit])


def test_four_rows_kernel_has_the_nine_tap_kernels_bits(lib, dev):
    """csrc/red.hip: the four-rows kernel accumulates per output in the (channel, tap) order of the nine-tap kernel.  The first Hc - 1
    output rows of a tall four-rows case equal, bit for bit, those of the unsplit nine-tap kernel on the crop to Hc rows (row Hc - 1
    sees the crop's bottom padding)."""
    c = S.BY_NAME_2D["rows4-h277-w257"]
    Hc = 200
    crop = c._replace(dims=(Hc, c.dims[1]))
    assert variant(lib, c) == S.ROWS4 and variant(lib, crop) == S.UNSPLIT_S1
    t = S.inputs(c)
    tall = run(lib, c, t, dev)
    short = run(lib, crop, dict(t, xa=t["xa"][:, :, :Hc].contiguous()), dev)
    assert torch.equal(tall[:, :, :Hc - 1].view(torch.int32), short[:, :, :Hc - 1].view(torch.int32))


def test_unsplit_threshold_pair_differing_in_batch_only(lib, dev):
    """B = 1 runs the channel-split form, B = 2 of the same layer the unsplit one.  With one input channel the split form's other three
    waves contribute exact zeros, so sample 0 must come out with equal bits from both kernels."""
    a, b = S.BY_NAME_2D["split1-256-b1"], S.BY_NAME_2D["unsplit1-512-b2"]
    assert variant(lib, a) == S.SPLIT_S1 and variant(lib, b) == S.UNSPLIT_S1 and a.CA + a.CB == 1
    tb = S.inputs(b)
    two = run(lib, b, tb, dev)
    one = run(lib, a, dict(tb, xa=tb["xa"][:1].contiguous()), dev)
    assert torch.equal(one.view(torch.int32), two[:1].view(torch.int32))


def test_rejected_arguments_leave_out_untouched(lib, dev):
    """Every rejection of the two entries answers SMVS_ERR_ARG before any launch: odd sizes at stride 2, a second operand / bias / init
    with the transposed layer, planes of 2^31 bytes given by dimensions only, batch x channel groups beyond 65535, null pointers."""
    ERR_ARG = 1
    buf = torch.full((4096,), SENTINEL, dtype=torch.int32, device=dev)
    x = torch.zeros(4096, dtype=torch.float32, device=dev)
    d, o, st = C.c_void_p(x.data_ptr()), C.c_void_p(buf.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    f2, f3 = lib.smvs_conv3x3_fwd, lib.smvs_conv3d_fwd
    # (kind, xA, CA, xB, CB, packed, bias, init, out, B, Cout, H, W, relu, stream)
    bad2 = [(1, d, 2, None, 0, d, None, None, o, 1, 2, 5, 4), (1, d, 2, None, 0, d, None, None, o, 1, 2, 4, 5),
            (2, d, 2, d, 2, d, None, None, o, 1, 2, 4, 4), (2, d, 2, None, 0, d, d, None, o, 1, 2, 4, 4), (2, d, 2, None, 0, d, None, d, o, 1, 2, 4, 4),
            (0, d, 8, None, 0, d, None, None, o, 1, 1, 8192, 8192), (0, d, 1, None, 0, d, None, None, o, 1, 8, 8192, 8192),
            (2, d, 1, None, 0, d, None, None, o, 1, 2, 8192, 8192),
            (0, d, 1, None, 0, d, None, None, o, 65536, 1, 1, 1), (0, d, 1, None, 0, d, None, None, o, 8192, 64, 1, 1),
            (0, None, 2, None, 0, d, None, None, o, 1, 2, 4, 4), (0, d, 2, None, 2, d, None, None, o, 1, 2, 4, 4),
            (0, d, 2, None, 0, None, None, None, o, 1, 2, 4, 4), (0, d, 2, None, 0, d, None, None, None, 1, 2, 4, 4),
            (3, d, 2, None, 0, d, None, None, o, 1, 2, 4, 4), (0, d, 0, None, 0, d, None, None, o, 1, 2, 4, 4), (0, d, 2, None, 0, d, None, None, o, 1, 2, 0, 4)]
    for a in bad2:
        assert f2(*a, 0, st) == ERR_ARG, a
        assert lib.smvs_last_error().decode() != ""
    # (kind, in, packed, skip, out, B, Cin, Cout, Di, Hi, Wi, relu, stream)
    bad3 = [(1, d, d, None, o, 1, 2, 2, 3, 4, 4), (1, d, d, None, o, 1, 2, 2, 4, 4, 5), (0, d, d, None, o, 1, 8, 8, 1024, 1024, 128),
            (2, d, d, None, o, 1, 1, 8, 256, 256, 256), (0, d, d, None, o, 1, 1, 1, 1024, 1024, 1), (0, d, d, None, o, 65536, 1, 1, 1, 1, 1),
            (0, None, d, None, o, 1, 2, 2, 4, 4, 4), (0, d, None, None, o, 1, 2, 2, 4, 4, 4), (0, d, d, None, None, 1, 2, 2, 4, 4, 4),
            (3, d, d, None, o, 1, 2, 2, 4, 4, 4), (0, d, d, None, o, 1, 0, 2, 4, 4, 4)]
    for a in bad3:
        assert f3(*a, 0, st) == ERR_ARG, a
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
