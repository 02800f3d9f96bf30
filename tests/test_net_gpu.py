"""smvs_featnet_fwd (csrc/featnet.hip), smvs_costreg_fwd (csrc/costreg.hip) and smvs_red_step_fwd (csrc/red.hip) on the MI355X, judged
layer by layer (tests/net_scene.py): one call, every intermediate tensor read back from the caller-owned workspace, each layer evaluated
in float64 on the float32 input the GPU itself produced and held per element to the derived bound -- no propagated error, no element
excused.  Parameters lie behind odd storage offsets, the workspace has exactly the bytes asked for, and the packed buffer, the
workspace and the outputs lie between guard words in buffers filled with a NaN of known payload."""
import ctypes as C

import numpy as np
import pytest
import torch

import net_scene as S

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF                                # bits of a quiet NaN no kernel produces
GUARD = 64
WORST = {}                                           # (network, layer kind) -> largest err / bound seen
ERR_ARG, ERR_UNSUPPORTED = 1, 3


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
    """Prints (it asserts nothing: the tests do) the largest err / bound per (network, layer kind) -- the table the README quotes."""
    yield
    for (net, kind), r in sorted(WORST.items()):
        print("net-worst %-8s %-14s %.3f" % (net, kind, r))


def at_end(t, dev, lead):
    """t on the device as the last numel floats of a tensor of lead + numel floats (tests/test_conv_gpu.py: at_end)"""
    buf = torch.empty(lead + t.numel(), dtype=torch.float32, device=dev)
    buf[lead:] = t.reshape(-1).to(dev)
    return buf[lead:].view(t.shape)


class Guarded:
    """n floats between GUARD sentinel words on each side, everything filled with the sentinel."""

    def __init__(self, n, dev):
        self.n = n
        self.big = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        self.t = self.big[GUARD:GUARD + n].view(torch.float32)

    def read(self, what, ranges=None):
        """-> the n floats on the CPU.  Asserts the guards untouched and every element (of `ranges`, else all) written."""
        bits = self.big.cpu()
        assert bool((bits[:GUARD] == SENTINEL).all()) and bool((bits[GUARD + self.n:] == SENTINEL).all()), "guard words around %s were written" % what
        body = bits[GUARD:GUARD + self.n]
        for lo, hi in (ranges if ranges is not None else [(0, self.n)]):
            assert not bool((body[lo:hi] == SENTINEL).any()), "elements of %s were not written" % what
        return body.view(torch.float32).clone()

    def untouched(self):
        return bool((self.big == SENTINEL).all())


def fn_pack(case, P, dev, stream=None):
    """smvs_featnet_pack_weights on the scene's parameters, each behind an odd storage offset.  -> Guarded packed buffer"""
    from satmvs_amd import _lib
    names = S.fn_param_names(case.c, case.arch)
    held = [at_end(P[k], dev, 1 + 2 * (i % 3)) for i, k in enumerate(names)]
    packed = Guarded(S.fn_packed_layout(case.c, case.arch)[1], dev)
    torch.cuda.synchronize()                      # operands were built on the current stream; the call may run on another
    _lib.call("smvs_featnet_pack_weights", _lib.ptr_array(held), case.c, case.arch, _lib.ptr(packed.t), stream or _lib.current_stream(dev))
    torch.cuda.synchronize()
    return packed


def fn_run(case, packed, imgs, dev, stream=None):
    """One smvs_featnet_fwd.  -> (T, bits): the tensors of net_scene.fn_tensors, and all of them as one int32 vector."""
    from satmvs_amd import _lib
    lay, total = S.fn_workspace(*case)
    ws = Guarded(total, dev)
    shapes = S.fn_out_shapes(case)
    outs = {k: Guarded(int(np.prod(v)), dev) for k, v in shapes.items()}
    x = at_end(imgs, dev, 3)
    torch.cuda.synchronize()                      # operands were built on the current stream; the call may run on another
    _lib.call("smvs_featnet_fwd", _lib.ptr(packed.t), _lib.ptr(x), _lib.ptr(outs["stage1"].t), _lib.ptr(outs["stage2"].t), _lib.ptr(outs["stage3"].t),
              _lib.ptr(ws.t), 4 * total, case.N, case.H, case.W, case.c, case.arch, stream or _lib.current_stream(dev))
    torch.cuda.synchronize()
    wsv = ws.read("the workspace", [(o, o + int(np.prod(s))) for o, s in lay.values()])
    got = {k: outs[k].read(k).view(shapes[k]) for k in shapes}
    T = S.fn_tensors(case, imgs, wsv, got)
    bits = torch.cat([T[k].reshape(-1).view(torch.int32) for k in sorted(T) if k != "imgs"])
    return T, bits


def fn_assert_layers(case, P, packed_cpu, T):
    for name, kind, ratio, where in S.fn_judge(case, P, packed_cpu, T):
        key = ("featnet", kind)
        WORST[key] = max(WORST.get(key, 0.0), ratio)
        print("net-ratio featnet %-28s %-16s %-12s %.4f at %s" % (S.fn_id(case), name, kind, ratio, where))
        assert ratio <= 1.0, (S.fn_id(case), name, kind, ratio, where)


FN_IDS = [S.fn_id(c) for c in S.FN_CASES]


@pytest.mark.parametrize("case", S.FN_CASES, ids=FN_IDS)
def test_featnet_every_layer_inside_its_bound(lib, dev, case):
    """The packed buffer bit for bit, every element of every layer inside its bound, the workspace sized exactly, guards untouched, every
    tensor fully written, and a second call with equal bits."""
    assert lib.smvs_featnet_workspace_bytes(*case) == 4 * S.fn_workspace(*case)[1]
    P = S.fn_params(case.c, case.arch)
    packed = fn_pack(case, P, dev)
    pk = packed.read("the packed buffer")
    want = S.fn_pack_reference(P, case.c, case.arch)
    assert torch.equal(pk.view(torch.int32), want.view(torch.int32)), "packed buffer differs at %s" % (torch.nonzero(pk.view(torch.int32) != want.view(torch.int32))[:8].flatten().tolist(),)
    imgs = S.fn_images(case)
    T, bits = fn_run(case, packed, imgs, dev)
    fn_assert_layers(case, P, pk, T)
    _, again = fn_run(case, packed, imgs, dev)
    assert torch.equal(bits, again), "two calls differ"


@pytest.mark.parametrize("arch", [0, 1], ids=["unet", "fpn"])
def test_featnet_nan_in_one_image_leaves_the_others_bits(lib, dev, arch):
    """A NaN in image 1 of 3: every tensor of images 0 and 2 keeps the bits of the run without it; image 1's first layer saw it (the
    kernels' ReLU is fmaxf(r, 0), which answers 0 for a NaN, so it does not travel further)."""
    case = S.FnCase(3, 8, 260, 8, arch)
    assert case in S.FN_CASES
    P = S.fn_params(case.c, arch)
    packed = fn_pack(case, P, dev)
    imgs = S.fn_images(case)
    base, _ = fn_run(case, packed, imgs, dev)
    bad = imgs.clone()
    bad[1, 2, 5, 131] = float("nan")
    T, _ = fn_run(case, packed, bad, dev)
    for k in base:
        if k == "imgs":
            continue
        for n in (0, 2):
            assert torch.equal(T[k][n].view(torch.int32), base[k][n].view(torch.int32)), (k, n)
    assert not torch.equal(T["t0"][1].view(torch.int32), base["t0"][1].view(torch.int32))


@pytest.mark.parametrize("arch", [0, 1], ids=["unet", "fpn"])
def test_featnet_on_a_side_stream(lib, dev, arch):
    """Packing and the forward on a stream of the caller's: the bits of the default-stream run."""
    case = S.FnCase(1, 20, 64, 5, arch)
    assert case in S.FN_CASES
    P = S.fn_params(case.c, arch)
    imgs = S.fn_images(case)
    _, base = fn_run(case, fn_pack(case, P, dev), imgs, dev)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    st = C.c_void_p(side.cuda_stream)
    packed = fn_pack(case, P, dev, stream=st)
    _, bits = fn_run(case, packed, imgs, dev, stream=st)
    assert torch.equal(bits, base)


def test_featnet_rejections_leave_everything_untouched(lib, dev):
    """H or W off the multiple of 4, a workspace one byte short, a null among the pointers, and base_channels = 17 at pack time
    (SMVS_ERR_UNSUPPORTED): refused before any launch."""
    case = S.FnCase(1, 8, 8, 8, 0)
    P = S.fn_params(case.c, case.arch)
    packed = fn_pack(case, P, dev)
    total = S.fn_workspace(*case)[1]
    ws, o1, o2, o3 = Guarded(total, dev), Guarded(4096, dev), Guarded(4096, dev), Guarded(4096, dev)
    x = torch.zeros(3 * 64 * 4, dtype=torch.float32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    f = lib.smvs_featnet_fwd
    good = [p(packed.t), p(x), p(o1.t), p(o2.t), p(o3.t), p(ws.t), 4 * total, 1, 8, 8, 8, 0, st]

    def changed(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return a
    bad = [changed(_8=6), changed(_9=6), changed(_8=10, _9=8), changed(_6=4 * total - 1), changed(_11=2), changed(_7=0), changed(_10=0)]
    bad += [changed(**{"_%d" % i: None}) for i in range(6)]
    for a in bad:
        assert f(*a) == ERR_ARG, a
        assert lib.smvs_last_error().decode() != ""
    # pack: a null among the 63 pointers, a null array, a null destination, arch 2; 4c = 68 folded channels are unsupported
    names = S.fn_param_names(case.c, case.arch)
    held = [P[k].to(dev) for k in names]
    dst = Guarded(S.fn_packed_layout(case.c, case.arch)[1], dev)
    for hole in (0, 41, 62):
        arr = (C.c_void_p * 63)(*[None if i == hole else t.data_ptr() for i, t in enumerate(held)])
        assert lib.smvs_featnet_pack_weights(arr, case.c, 0, p(dst.t), st) == ERR_ARG, hole
    arr = (C.c_void_p * 63)(*[t.data_ptr() for t in held])
    assert lib.smvs_featnet_pack_weights(None, case.c, 0, p(dst.t), st) == ERR_ARG
    assert lib.smvs_featnet_pack_weights(arr, case.c, 0, None, st) == ERR_ARG
    assert lib.smvs_featnet_pack_weights(arr, case.c, 2, p(dst.t), st) == ERR_ARG
    assert lib.smvs_featnet_pack_weights(arr, 0, 0, p(dst.t), st) == ERR_ARG
    torch.cuda.synchronize()
    assert dst.untouched()
    # base_channels = 17: conv2.0 would fold 68 channels; refused before the first layers (cout 17, 34) are packed
    P17 = {}
    for l in S.fn_layers(17, 0):
        keys = S._layer_keys(l)
        P17[keys[0]] = torch.zeros((l.cin, l.cout, l.k, l.k) if l.transposed else (l.cout, l.cin, l.k, l.k))
        for k in keys[1:]:
            P17[k] = torch.ones(l.cout)
    held17 = [P17[k].to(dev) for k in S.fn_param_names(17, 0)]
    dst17 = Guarded(lib.smvs_featnet_packed_floats(17, 0), dev)
    arr17 = (C.c_void_p * 63)(*[t.data_ptr() for t in held17])
    assert lib.smvs_featnet_pack_weights(arr17, 17, 0, p(dst17.t), st) == ERR_UNSUPPORTED
    assert "17" in lib.smvs_last_error().decode()
    torch.cuda.synchronize()
    assert all(g.untouched() for g in (ws, o1, o2, o3, dst17))


def _module(case, P, dev, eps=None):
    from satmvs_amd.modules.module import FeatureNet
    net = FeatureNet(base_channels=case.c, stride=4, num_stage=3, arch_mode="unet" if case.arch == 0 else "fpn").eval()
    missing, unexpected = net.load_state_dict(P, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    if eps is not None:
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.eps = eps
    return net.to(dev)


@pytest.mark.parametrize("case", [S.FnCase(1, 12, 68, 4, 0), S.FnCase(1, 12, 68, 4, 1), S.FnCase(2, 12, 132, 16, 0), S.FnCase(2, 12, 132, 16, 1)],
                         ids=lambda c: S.fn_id(c))
def test_featnet_module_gives_the_bits_of_the_c_entry(lib, dev, case):
    """FeatureNet carrying the scene's parameters (every tensor distinct, net_scene.fn_params) = the C entry called with the pointer
    order include/satmvs.h states: pins the 63- and 47-pointer orders of the Python layer."""
    assert case in S.FN_CASES
    P = S.fn_params(case.c, case.arch)
    imgs = S.fn_images(case)
    T, _ = fn_run(case, fn_pack(case, P, dev), imgs, dev)
    net = _module(case, P, dev)
    x = imgs.to(dev)
    with torch.no_grad():
        assert net._use_native(x)
        y = net(x)
    for k in ("stage1", "stage2", "stage3"):
        assert torch.equal(y[k].cpu().view(torch.int32), T[k].view(torch.int32)), k


@pytest.mark.parametrize("arch", [0, 1], ids=["unet", "fpn"])
def test_featnet_module_with_another_eps_matches_float64(lib, dev, arch):
    """BatchNorm eps = 1e-3 instead of the 1e-5 the pack kernel folds.  One channel per layer has the running variance 1e-4, so its
    scale differs by the factor sqrt(1.1e-3 / 1.1e-4) = 3.2 between the two eps: a module that packed its parameters for the native
    path would be wrong by the size of the values.  Against the float64 module on the CPU, per output within 1e-4 of the output's
    largest magnitude: generous for any float32 evaluation of 15 layers of at most 576 products (sqrt(576) 2^-24 = 1.4e-6 per layer),
    and four orders of magnitude below the error of the wrong eps."""
    case = S.FnCase(1, 12, 68, 4, arch)
    P = S.fn_params(case.c, arch)
    imgs = S.fn_images(case)
    net = _module(case, P, dev, eps=1e-3)
    ref_net = _module(case, P, torch.device("cpu"), eps=1e-3).double()
    wrong_net = _module(case, P, torch.device("cpu")).double()
    with torch.no_grad():
        y = net(imgs.to(dev))
        ref = ref_net(imgs.double())
        wrong = wrong_net(imgs.double())
    for k in ("stage1", "stage2", "stage3"):
        scale = float(ref[k].abs().max())
        err = float((y[k].cpu().double() - ref[k]).abs().max())
        print("net-eps featnet %s %s: |module - float64| = %.3g, |eps 1e-5 - eps 1e-3| = %.3g, largest |value| %.3g"
              % (S.fn_id(case), k, err, float((wrong[k] - ref[k]).abs().max()), scale))
        assert float((wrong[k] - ref[k]).abs().max()) > 1e-2 * scale          # the case can tell the two eps apart
        assert err <= 1e-4 * scale, (k, err, scale)


# ---- costreg ----------------------------------------------------------------------------------------------------------------------
def cr_pack(case, P, dev, stream=None):
    from satmvs_amd import _lib
    held = [at_end(P[k], dev, 1 + 2 * (i % 3)) for i, k in enumerate(S.cr_param_names())]
    packed = Guarded(S.cr_packed_layout(case.C)[1], dev)
    torch.cuda.synchronize()                      # operands were built on the current stream; the call may run on another
    _lib.call("smvs_costreg_pack_weights", _lib.ptr_array(held), case.C, _lib.ptr(packed.t), stream or _lib.current_stream(dev))
    torch.cuda.synchronize()
    return packed


def cr_run(case, packed, vol, dev, stream=None):
    """One smvs_costreg_fwd.  -> (T, bits)."""
    from satmvs_amd import _lib
    lay, total = S.cr_workspace(case.B, case.D, case.H, case.W)
    ws = Guarded(total, dev)
    oshape = (case.B, 1, case.D, case.H, case.W)
    out = Guarded(int(np.prod(oshape)), dev)
    x = at_end(vol, dev, 1)
    torch.cuda.synchronize()                      # operands were built on the current stream; the call may run on another
    _lib.call("smvs_costreg_fwd", _lib.ptr(packed.t), _lib.ptr(x), _lib.ptr(out.t), _lib.ptr(ws.t), 4 * total, *case, stream or _lib.current_stream(dev))
    torch.cuda.synchronize()
    wsv = ws.read("the workspace", [(o, o + int(np.prod(s))) for o, s in lay.values()])
    T = S.cr_tensors(case, vol, wsv, out.read("out").view(oshape))
    bits = torch.cat([T[k].reshape(-1).view(torch.int32) for k in sorted(T) if k != "vol"])
    return T, bits


CR_IDS = [S.cr_id(c) for c in S.CR_CASES]


@pytest.mark.parametrize("case", S.CR_CASES, ids=CR_IDS)
def test_costreg_every_layer_inside_its_bound(lib, dev, case):
    assert lib.smvs_costreg_workspace_bytes(*case) == 4 * S.cr_workspace(case.B, case.D, case.H, case.W)[1]
    P = S.cr_params(case.C)
    packed = cr_pack(case, P, dev)
    pk = packed.read("the packed buffer")
    want = S.cr_pack_reference(P, case.C)
    assert torch.equal(pk.view(torch.int32), want.view(torch.int32)), "packed buffer differs at %s" % (torch.nonzero(pk.view(torch.int32) != want.view(torch.int32))[:8].flatten().tolist(),)
    vol = S.cr_volume(case)
    T, bits = cr_run(case, packed, vol, dev)
    for name, kind, ratio, where in S.cr_judge(case, P, pk, T):
        key = ("costreg", kind)
        WORST[key] = max(WORST.get(key, 0.0), ratio)
        print("net-ratio costreg %-20s %-8s %-12s %.4f at %s" % (S.cr_id(case), name, kind, ratio, where))
        assert ratio <= 1.0, (S.cr_id(case), name, kind, ratio, where)
    _, again = cr_run(case, packed, vol, dev)
    assert torch.equal(bits, again), "two calls differ"


def test_costreg_nan_in_one_sample_leaves_the_others_bits(lib, dev):
    case = S.CR_CASES[1]
    assert case.B == 2
    P = S.cr_params(case.C)
    packed = cr_pack(case, P, dev)
    vol = S.cr_volume(case)
    base, _ = cr_run(case, packed, vol, dev)
    bad = vol.clone()
    bad[1, 3, 4, 7, 61] = float("nan")
    T, _ = cr_run(case, packed, bad, dev)
    for k in base:
        if k != "vol":
            assert torch.equal(T[k][0].view(torch.int32), base[k][0].view(torch.int32)), k
    assert not torch.equal(T["c0"][1].view(torch.int32), base["c0"][1].view(torch.int32))          # sample 1 saw it (and its ReLU answered 0)


def test_costreg_on_a_side_stream(lib, dev):
    case = S.CR_CASES[3]
    P = S.cr_params(case.C)
    vol = S.cr_volume(case)
    _, base = cr_run(case, cr_pack(case, P, dev), vol, dev)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    st = C.c_void_p(side.cuda_stream)
    _, bits = cr_run(case, cr_pack(case, P, dev, stream=st), vol, dev, stream=st)
    assert torch.equal(bits, base)


def test_costreg_rejections_leave_everything_untouched(lib, dev):
    """D, H or W off the multiple of 8, a workspace one byte short, null pointers: refused before any launch."""
    case = S.CR_CASES[0]
    P = S.cr_params(case.C)
    packed = cr_pack(case, P, dev)
    total = S.cr_workspace(case.B, case.D, case.H, case.W)[1]
    ws, out = Guarded(total, dev), Guarded(4096, dev)
    x = torch.zeros(8 * 16 * 16 * 16, dtype=torch.float32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    good = [p(packed.t), p(x), p(out.t), p(ws.t), 4 * total, 1, 8, 8, 8, 8, st]

    def changed(i, v):
        a = list(good)
        a[i] = v
        return a
    bad = [changed(7, 12), changed(8, 12), changed(9, 12), changed(7, 4), changed(4, 4 * total - 1), changed(5, 0), changed(6, 0)]
    bad += [changed(i, None) for i in range(4)]
    for a in bad:
        assert lib.smvs_costreg_fwd(*a) == ERR_ARG, a
        assert lib.smvs_last_error().decode() != ""
    held = [P[k].to(dev) for k in S.cr_param_names()]
    dst = Guarded(S.cr_packed_layout(case.C)[1], dev)
    for hole in (0, 26, 50):
        arr = (C.c_void_p * 51)(*[None if i == hole else t.data_ptr() for i, t in enumerate(held)])
        assert lib.smvs_costreg_pack_weights(arr, case.C, p(dst.t), st) == ERR_ARG, hole
    arr = (C.c_void_p * 51)(*[t.data_ptr() for t in held])
    assert lib.smvs_costreg_pack_weights(None, case.C, p(dst.t), st) == ERR_ARG
    assert lib.smvs_costreg_pack_weights(arr, case.C, None, st) == ERR_ARG
    assert lib.smvs_costreg_pack_weights(arr, 0, p(dst.t), st) == ERR_ARG
    torch.cuda.synchronize()
    assert all(g.untouched() for g in (ws, out, dst))


def _cr_module(case, P, dev, eps=None):
    from satmvs_amd.modules.module import CostRegNet
    net = CostRegNet(case.C, 8).eval()
    missing, unexpected = net.load_state_dict(P, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    if eps is not None:
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm3d):
                m.eps = eps
    return net.to(dev)


@pytest.mark.parametrize("case", [S.CR_CASES[0], S.CR_CASES[3]], ids=S.cr_id)
def test_costreg_module_gives_the_bits_of_the_c_entry(lib, dev, case):
    """CostRegNet carrying the scene's parameters = the C entry with the 51 pointers in the order include/satmvs.h states."""
    P = S.cr_params(case.C)
    vol = S.cr_volume(case)
    T, _ = cr_run(case, cr_pack(case, P, dev), vol, dev)
    net = _cr_module(case, P, dev)
    x = vol.to(dev)
    with torch.no_grad():
        assert net._use_native(x)
        y = net(x)
    assert torch.equal(y.cpu().view(torch.int32), T["out"].view(torch.int32))


def test_costreg_module_with_another_eps_matches_float64(lib, dev):
    """As test_featnet_module_with_another_eps_matches_float64, for BatchNorm3d: 11 layers of at most 1728 products."""
    case = S.CR_CASES[0]
    P = S.cr_params(case.C)
    vol = S.cr_volume(case)
    net = _cr_module(case, P, dev, eps=1e-3)
    with torch.no_grad():
        y = net(vol.to(dev)).cpu().double()
        ref = _cr_module(case, P, torch.device("cpu"), eps=1e-3).double()(vol.double())
        wrong = _cr_module(case, P, torch.device("cpu")).double()(vol.double())
    scale = float(ref.abs().max())
    err = float((y - ref).abs().max())
    print("net-eps costreg %s: |module - float64| = %.3g, |eps 1e-5 - eps 1e-3| = %.3g, largest |value| %.3g" % (S.cr_id(case), err, float((wrong - ref).abs().max()), scale))
    assert float((wrong - ref).abs().max()) > 1e-2 * scale
    assert err <= 1e-4 * scale, (err, scale)


# ---- RED: the eps the plane kernels hard-code -----------------------------------------------------------------------------------------
def _red_module(eps, dev, dtype=torch.float32):
    """slice_RED_Regularization(8, 8) with seeded parameters: GroupNorm weights and biases random and distinct per norm, the gate and
    candidate convolutions scaled down so that their raw outputs have a variance near 1e-3 -- there eps = 1e-3 against 1e-5 changes
    every normalised gate by tens of per cent."""
    from satmvs_amd.modules.module import slice_RED_Regularization
    torch.manual_seed(3)
    reg = slice_RED_Regularization(8, 8).eval()
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for name, p in reg.named_parameters():
            if "_norm." in name:
                p.copy_(0.5 * torch.randn(p.shape, generator=g) + (1.0 if name.endswith("weight") else 0.0))
            elif "gate_conv." in name or "output_conv." in name:
                p.mul_(0.03)
    norms = [m for m in reg.modules() if isinstance(m, torch.nn.GroupNorm)]
    assert len(norms) == 12
    for m in norms:
        m.eps = eps
    return reg.to(device=dev, dtype=dtype)


def test_red_module_with_another_eps_matches_float64(lib, dev):
    """GroupNorm eps = 1e-3 instead of the 1e-5f of gru_gate_apply_body / gru_combine_body, two consecutive planes (state carried),
    against the float64 module on the CPU: output and states within 1e-4 of the largest magnitude (states are blends of tanh values:
    at most 1), far above any float32 evaluation's error and two orders below what the wrong eps does."""
    B, H, W = 2, 16, 72
    g = torch.Generator().manual_seed(9)
    x1, x2 = torch.randn((B, 8, H, W), generator=g), torch.randn((B, 8, H, W), generator=g)
    runs = {}
    for key, eps, d, dt in (("gpu", 1e-3, dev, torch.float32), ("ref", 1e-3, torch.device("cpu"), torch.float64), ("wrong", 1e-5, torch.device("cpu"), torch.float64)):
        reg = _red_module(eps, d, dt)
        with torch.no_grad():
            r1 = reg(x1.to(device=d, dtype=dt), *reg.initial_states(B, H, W, d, dt))
            out1 = r1[0].clone()
            r2 = reg(x2.to(device=d, dtype=dt), *r1[1:])
        runs[key] = [out1.cpu().double()] + [t.cpu().double() for t in r2]
    for i, (got, ref, wrong) in enumerate(zip(runs["gpu"], runs["ref"], runs["wrong"])):
        scale = float(ref.abs().max())
        err, sep = float((got - ref).abs().max()), float((wrong - ref).abs().max())
        print("net-eps red tensor %d: |module - float64| = %.3g, |eps 1e-5 - eps 1e-3| = %.3g, largest |value| %.3g" % (i, err, sep, scale))
        assert sep > 1e-2 * scale, i
        assert err <= 1e-4 * scale, (i, err, scale)


# ---- RED: one plane step, stage by stage ----------------------------------------------------------------------------------------------
def red_pack(C_in, P, dev, stream=None):
    from satmvs_amd import _lib
    held = [at_end(P[k], dev, 1 + 2 * (i % 3)) for i, k in enumerate(S.red_param_names())]
    want, written = S.red_pack_reference(P, C_in)
    packed = Guarded(want.numel(), dev)
    torch.cuda.synchronize()                      # operands were built on the current stream; the call may run on another
    _lib.call("smvs_red_pack_weights", _lib.ptr_array(held), C_in, _lib.ptr(packed.t), stream or _lib.current_stream(dev))
    torch.cuda.synchronize()
    return packed


def red_run(case, packed, cost, h_old, dev, stream=None, ws=None):
    """One smvs_red_step_fwd from the states h_old (held in guarded buffers and updated in place).  -> (T, bits, ws): the tensors of
    net_scene.red_tensors, every float32 tensor of them as one int32 vector, the guarded workspace."""
    from satmvs_amd import _lib
    lay, stats, total = S.red_workspace(*case)
    ws = ws or Guarded(total, dev)
    assert ws.n >= total
    shapes = S.red_state_shapes(case)
    st = [Guarded(int(np.prod(s)), dev) for s in shapes]
    for gd, h in zip(st, h_old):
        gd.t.copy_(h.reshape(-1).to(dev))
    oshape = (case.B, 1, case.H, case.W)
    out = Guarded(int(np.prod(oshape)), dev)
    x = at_end(cost, dev, 1)
    torch.cuda.synchronize()                      # operands were built on the current stream; the call may run on another
    _lib.call("smvs_red_step_fwd", _lib.ptr(packed.t), _lib.ptr(x), *[_lib.ptr(g.t) for g in st], _lib.ptr(out.t), _lib.ptr(ws.t), 4 * ws.n, *case,
              stream or _lib.current_stream(dev))
    torch.cuda.synchronize()
    nstat = case.B * 4 * 3 * S.RED_NSLOT * 2 * 2
    wsv = ws.read("the workspace", [(o, o + int(np.prod(s))) for o, s in lay.values()] + [(stats, stats + nstat)])[:total]
    states = [g.read("state %d" % (i + 1)).view(s) for i, (g, s) in enumerate(zip(st, shapes))]
    T = S.red_tensors(case, cost, h_old, wsv, states, out.read("reg_out").view(oshape))
    bits = torch.cat([T[k].reshape(-1).view(torch.int32) for k in sorted(T) if k not in ("cost", "stats") and not (k[0] == "h" and k[1:].isdigit())])
    return T, bits, ws


def red_assert_stages(case, P, T, tag=""):
    for name, label, ratio, where in S.red_judge(case, P, T):
        key = ("red", label)
        WORST[key] = max(WORST.get(key, 0.0), ratio)
        print("net-ratio red %-16s%s %-12s %-14s %.4f at %s" % (S.red_id(case), tag, name, label, ratio, where))
        assert ratio <= 1.0, (S.red_id(case), tag, name, label, ratio, where)


RED_RUNS = [(c, False) for c in S.RED_CASES] + [(c, True) for c in S.RED_HOT_CASES]


@pytest.mark.parametrize("case,hot", RED_RUNS, ids=[S.red_id(c) + ("-hot" if h else "") for c, h in RED_RUNS])
def test_red_every_stage_inside_its_bound(lib, dev, case, hot):
    """The packed buffer bit for bit; every stage of the plane inside its bound on the GPU's own inputs, the GroupNorm partial sums
    included; states updated in place and equal to their snapshots; a second step from the first's states judged again; guards
    untouched; two calls from the same states give equal bits."""
    assert lib.smvs_red_workspace_bytes(*case) == 4 * S.red_workspace(*case)[2]
    P = S.red_params_hot(case) if hot else S.red_params(case.C)
    packed = red_pack(case.C, P, dev)
    want, written = S.red_pack_reference(P, case.C)
    pk = packed.read("the packed buffer", [])                      # guards here; what is written and what is not, below
    assert torch.equal(pk.view(torch.int32)[written], want.view(torch.int32)[written])
    assert bool((pk.view(torch.int32)[~written] == SENTINEL).all())
    cost, h = S.red_inputs(case)
    T, bits, _ = red_run(case, packed, cost, h, dev)
    red_assert_stages(case, P, T)
    _, again, _ = red_run(case, packed, cost, h, dev)
    assert torch.equal(bits, again), "two calls differ"
    h2 = [T["state%d" % g] for g in range(4)]
    T2, _, _ = red_run(case, packed, S.red_inputs(case, 1)[0], h2, dev)
    red_assert_stages(case, P, T2, " step 2")


def test_red_small_case_after_a_large_one_in_the_same_workspace(lib, dev):
    big, small = S.RedCase(3, 32, 24, 136), S.RedCase(2, 8, 8, 72)
    _, _, ws = red_run(big, red_pack(big.C, S.red_params(big.C), dev), *S.red_inputs(big), dev)
    P = S.red_params(small.C)
    packed = red_pack(small.C, P, dev)
    cost, h = S.red_inputs(small)
    _, fresh, _ = red_run(small, packed, cost, h, dev)
    T, used, _ = red_run(small, packed, cost, h, dev, ws=ws)
    assert torch.equal(fresh, used)
    red_assert_stages(small, P, T, " reused ws")


def test_red_nan_in_one_sample_leaves_the_others_bits(lib, dev):
    """NaN in the plane of sample 1 of 3: every tensor of samples 0 and 2 keeps its bits, their statistics stay what they were (the
    float64 slot sums up to the order of the atomics), and sample 1's new states carry the NaN."""
    case = S.RedCase(3, 32, 24, 136)
    P = S.red_params(case.C)
    packed = red_pack(case.C, P, dev)
    cost, h = S.red_inputs(case)
    base, _, _ = red_run(case, packed, cost, h, dev)
    bad = cost.clone()
    bad[1, 7, 11, 67] = float("nan")
    T, _, _ = red_run(case, packed, bad, h, dev)
    for k in base:
        if k in ("cost", "stats") or (k[0] == "h" and k[1:].isdigit()):
            continue
        for b in (0, 2):
            assert torch.equal(T[k][b].view(torch.int32), base[k][b].view(torch.int32)), (k, b)
    # equal float32 partial sums enter the float64 atomics of both runs in an order of their own: each run within
    # red_f64_depth(n) 2^-53 (sum |r|, sum r^2) of the exact sum of those partials
    for g, ((g0, o0), (g1, o1)) in enumerate(zip(S.red_stats_view(base["stats"], 3), S.red_stats_view(T["stats"], 3))):
        mag = torch.cat([S.red_group_sums(base["gates%d" % g], 2)[:, :, 2:], S.red_group_sums(base["cand%d" % g], 1)[:, :, 2:]], 1)   # (B, 3, 2)
        tol = 2 * S.red_f64_depth(base["cand%d" % g][0].numel()) * 2.0 ** -53 * mag
        for b in (0, 2):
            a0, a1 = torch.cat([g0[b].sum(1), o0[b].sum(0)[None]]), torch.cat([g1[b].sum(1), o1[b].sum(0)[None]])                      # (3, 2)
            assert bool(torch.isfinite(a1).all()) and bool(((a0 - a1).abs() <= tol[b]).all()), (g, b)
    assert bool(torch.isnan(T["state0"][1]).any())      # level 1 reads the plane itself; the encoder's ReLU (fmaxf) answers 0 for the NaN


def test_red_on_a_side_stream(lib, dev):
    case = S.RedCase(1, 5, 16, 64)
    P = S.red_params(case.C)
    cost, h = S.red_inputs(case)
    _, base, _ = red_run(case, red_pack(case.C, P, dev), cost, h, dev)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    st = C.c_void_p(side.cuda_stream)
    _, bits, _ = red_run(case, red_pack(case.C, P, dev, stream=st), cost, h, dev, stream=st)
    assert torch.equal(bits, base)


def test_red_rejections_leave_everything_untouched(lib, dev):
    case = S.RedCase(1, 8, 8, 8)
    P = S.red_params(case.C)
    packed = red_pack(case.C, P, dev)
    total = S.red_workspace(*case)[2]
    ws, out = Guarded(total, dev), Guarded(256, dev)
    sts = [Guarded(4096, dev) for _ in range(4)]
    x = torch.zeros(8 * 16 * 16, dtype=torch.float32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    good = [p(packed.t), p(x)] + [p(g.t) for g in sts] + [p(out.t), p(ws.t), 4 * total, 1, 8, 8, 8, st]

    def changed(i, v):
        a = list(good)
        a[i] = v
        return a
    bad = [changed(11, 12), changed(12, 12), changed(11, 4), changed(8, 4 * total - 1), changed(9, 0), changed(10, 0)] + [changed(i, None) for i in range(8)]
    for a in bad:
        assert lib.smvs_red_step_fwd(*a) == ERR_ARG, a
        assert lib.smvs_last_error().decode() != ""
    held = [P[k].to(dev) for k in S.red_param_names()]
    dst = Guarded(S.red_pack_reference(P, case.C)[0].numel(), dev)
    for hole in (0, 23, 47):
        arr = (C.c_void_p * 48)(*[None if i == hole else t.data_ptr() for i, t in enumerate(held)])
        assert lib.smvs_red_pack_weights(arr, case.C, p(dst.t), st) == ERR_ARG, hole
    arr = (C.c_void_p * 48)(*[t.data_ptr() for t in held])
    assert lib.smvs_red_pack_weights(None, case.C, p(dst.t), st) == ERR_ARG
    assert lib.smvs_red_pack_weights(arr, case.C, None, st) == ERR_ARG
    assert lib.smvs_red_pack_weights(arr, 0, p(dst.t), st) == ERR_ARG
    torch.cuda.synchronize()
    assert all(g.untouched() for g in [ws, out, dst] + sts)


def _red_scene_module(case, P, dev, dtype=torch.float32):
    from satmvs_amd.modules.module import slice_RED_Regularization
    reg = slice_RED_Regularization(case.C, 8).eval()
    reg.load_state_dict(P)
    return reg.to(device=dev, dtype=dtype)


@pytest.mark.parametrize("case", [S.RedCase(2, 8, 8, 72), S.RedCase(1, 5, 16, 64)], ids=S.red_id)
def test_red_module_gives_the_bits_of_the_c_entry(lib, dev, case):
    """slice_RED_Regularization carrying the scene's parameters (the three norms of every cell distinct) = the C entry with the 48
    pointers in the order include/satmvs.h states."""
    P = S.red_params(case.C)
    cost, h = S.red_inputs(case)
    T, _, _ = red_run(case, red_pack(case.C, P, dev), cost, h, dev)
    reg = _red_scene_module(case, P, dev)
    x = cost.to(dev)
    with torch.no_grad():
        assert reg._use_native(x)
        r = reg(x, *[t.to(dev) for t in h])
    for got, want in zip(r, [T["out"]] + [T["state%d" % g] for g in range(4)]):
        assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("case", S.RED_HOT_CASES, ids=S.red_id)
def test_red_hot_scene_statistics_finding(lib, dev, case):
    """Records (prints; the stage test above asserts) at a scene whose raw gates have mean / std = 30: the largest error of the new states
    against the float64 module, of the native step and of a float32 CPU evaluation of the same module (torch's group_norm), and their
    ratio -- the figures behind the README's note on the float32 partial sums of the GroupNorm statistics."""
    P = S.red_params_hot(case)
    cost, h = S.red_inputs(case)
    T, _, _ = red_run(case, red_pack(case.C, P, dev), cost, h, dev)
    cpu = torch.device("cpu")
    with torch.no_grad():
        ref = _red_scene_module(case, P, cpu, torch.float64)(cost.double(), *[t.double() for t in h])
        f32 = _red_scene_module(case, P, cpu)(cost, *[t.clone() for t in h])
    native = max(float((T["state%d" % g].double() - ref[1 + g]).abs().max()) for g in range(4))
    comp = max(float((f32[1 + g].double() - ref[1 + g]).abs().max()) for g in range(4))
    print("net-hot red %s: native %.3g, float32 composite %.3g, ratio %.2f" % (S.red_id(case), native, comp, native / comp))
    assert native <= 1e-4 and comp <= 1e-4          # both are float32 evaluations of values below 1; the finding is the ratio printed
