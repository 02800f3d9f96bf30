"""What tests/test_net_gpu.py assumes about tests/net_scene.py, checked without a GPU: every case passes the mirrored argument rules
and the library's own size queries agree with the mirrored layouts, the cases reach every remainder class of the featnet kernels and
every job kind of RED's level-batched launches, the packing reference is the definition, a correct float32 evaluation of the network passes the layer-by-layer judge at every layer and
planted kernel faults do not."""
import numpy as np
import pytest
import torch

import net_scene as S


@pytest.fixture(scope="module")
def lib():
    from satmvs_amd import build, _lib
    build.build()
    return _lib.load()


FN_IDS = [S.fn_id(c) for c in S.FN_CASES]


@pytest.mark.parametrize("case", S.FN_CASES, ids=FN_IDS)
def test_featnet_case_is_accepted_and_layouts_match_the_library(lib, case):
    assert S.fn_accepts(*case)
    lay, total = S.fn_workspace(*case)
    assert lib.smvs_featnet_workspace_bytes(*case) == 4 * total
    assert lib.smvs_featnet_packed_floats(case.c, case.arch) == S.fn_packed_layout(case.c, case.arch)[1]
    assert len(S.fn_param_names(case.c, case.arch)) == (63 if case.arch == 0 else 47)
    # every offset a multiple of 4 floats, tensors back to back in take() order
    end = 0
    for name, (o, shape) in lay.items():
        assert o % 4 == 0 and o == end, name
        n = 1
        for d in shape:
            n *= d
        end = o + ((n + 3) & ~3)
    assert end == total
    # every tensor a step names exists, with the channel counts the layer wants
    shapes = dict({k: v[1] for k, v in lay.items()}, imgs=(case.N, 3, case.H, case.W), **S.fn_out_shapes(case))
    for l, st in zip(S.fn_layers(case.c, case.arch), S.fn_steps(case.c, case.arch)):
        assert shapes[st.inA][1] + (shapes[st.inB][1] if st.inB else 0) == l.cin and shapes[st.out][1] == l.cout, l.name
        assert (st.CB == shapes[st.inB][1]) if st.inB else st.CB == 0
        assert shapes[st.inA][2:] == (case.H >> st.lin, case.W >> st.lin) and shapes[st.out][2:] == (case.H >> st.lout, case.W >> st.lout)
        if st.up:
            assert shapes[st.up] == (case.N, l.cout, shapes[st.out][2] // 2, shapes[st.out][3] // 2)


def test_featnet_rejections_are_mirrored(lib):
    for a in [(1, 6, 8, 8, 0), (1, 8, 6, 8, 0), (1, 0, 8, 8, 0), (0, 8, 8, 8, 0), (1, 8, 8, 0, 1), (1, 8, 8, 8, 2), (1, 8192, 8192, 8, 0),
              (65536, 4, 4, 2, 0)]:
        assert lib.smvs_featnet_workspace_bytes(*a) == 0 and not S.fn_accepts(*a), a
    assert not S.fn_accepts(1, 8, 8, 17, 0) and S.fn_accepts(1, 8, 8, 16, 0)            # 4c > 64: refused at pack time


def test_featnet_cases_reach_every_remainder_class():
    tags = set().union(*[S.fn_classes(c) for c in S.FN_CASES])
    kinds = {k for k, _ in tags}
    assert kinds == {"conv1x1 s1", "conv3x3 s1", "conv5x5 s2", "convT"}
    want = {"W<64", "W=64", "W=65", "H<4", "H=4", "H=5", "Cout%8=0", "Cout%8=4", "Cout%8=5", "Cin odd", "Cin even"}
    assert want <= {t for _, t in tags}
    # per kernel: everything but what the network cannot give it.  The transposed and the 5 x 5 layers have Cin = 2c or 4c (even; the
    # 5 x 5 one also c, odd with c = 5) and the 5 x 5 layers Cout = 2c or 4c (never 5 mod 8); their planes are the halves and quarters
    # of the image, 64 columns wide only for W = 128 or 256, which the case list does not hold (it holds 65 = 64 + 1 and 66).
    absent = {"convT": {"Cin odd", "W=64"}, "conv5x5 s2": {"Cout%8=5", "W=64"}, "conv3x3 s1": set(), "conv1x1 s1": set()}
    for k in kinds:
        missing = {t for t in want - absent[k] if (k, t) not in tags}
        assert not missing, (k, sorted(missing))
        assert not {t for t in absent[k] if (k, t) in tags}
    assert ("conv3x3 s1", "CA odd") in tags and ("conv3x3 s1", "CA even") in tags           # the concat layers
    assert {c.c for c in S.FN_CASES} >= {4, 5, 8, 12, 16} and {c.N for c in S.FN_CASES} >= {1, 2, 3}


def test_featnet_parameters_are_what_the_docstring_says():
    for c, arch in sorted({(k.c, k.arch) for k in S.FN_CASES}):
        P = S.fn_params(c, arch)
        for l in S.fn_layers(c, arch):
            keys = S._layer_keys(l)
            if l.bn:
                gamma, beta, mean, var = [P[k] for k in keys[1:]]
                assert int((gamma == 0).sum()) == 1 and bool((gamma > 0).any()) and bool((gamma < 0).any()), l.name
                assert float(var.min()) == pytest.approx(1e-4) and int((var < 0.01).sum()) == 1
                assert float(beta.abs().min()) > 0 and float(mean.abs().min()) > 0
            elif l.bias:
                assert float(P[keys[1]].abs().min()) > 0
        # norm parameters differ between layers of equal shape: a swap in the pointer order changes the packed buffer
        packed = S.fn_pack_reference(P, c, arch)
        names = S.fn_param_names(c, arch)
        for i in range(len(names)):
            for j in range(i + 1, len(names)):
                if P[names[i]].shape == P[names[j]].shape:
                    assert not torch.equal(P[names[i]], P[names[j]]), (names[i], names[j])
        assert packed.numel() == S.fn_packed_layout(c, arch)[1]


def test_featnet_pack_reference_is_the_definition():
    """Index by index from the definition: packed[w + ((cog * cin + ci) * kk + tap) * 8 + j] = weight[cog * 8 + j][ci][tap]."""
    for c, arch in ((5, 0), (5, 1)):
        P = S.fn_params(c, arch)
        packed = S.fn_pack_reference(P, c, arch)
        lay, _ = S.fn_packed_layout(c, arch)
        for l, (wo, so, to) in zip(S.fn_layers(c, arch), lay):
            keys = S._layer_keys(l)
            w = P[keys[0]]
            kk = l.k * l.k
            ncog = (l.cout + 7) // 8
            for cog in range(ncog):
                for ci in (0, l.cin - 1):
                    for tap in (0, kk - 1):
                        for j in range(8):
                            co = cog * 8 + j
                            want = 0.0 if co >= l.cout else float(w[ci, co].reshape(-1)[tap] if l.transposed else w[co, ci].reshape(-1)[tap])
                            assert float(packed[wo + ((cog * l.cin + ci) * kk + tap) * 8 + j]) == want
            s, t = packed[so:so + ncog * 8], packed[to:to + ncog * 8]
            assert bool((s[l.cout:] == 1).all()) and bool((t[l.cout:] == 0).all())
            if l.bn:
                gamma, beta, mean, var = [P[k].double() for k in keys[1:]]
                sd = gamma / (var + 1e-5).sqrt()
                assert torch.equal(s[:l.cout], sd.float()) and torch.equal(t[:l.cout], (beta - mean * sd).float())
            elif l.bias:
                assert bool((s == 1).all()) and torch.equal(t[:l.cout], P[keys[1]])
            else:
                assert bool((s == 1).all()) and bool((t == 0).all())


@pytest.mark.parametrize("case", S.FN_CASES, ids=FN_IDS)
def test_featnet_float32_model_passes_the_judge_at_every_layer(case):
    P = S.fn_params(case.c, case.arch)
    packed = S.fn_pack_reference(P, case.c, case.arch)
    T = S.fn_model32(case, P, packed, S.fn_images(case))
    res = S.fn_judge(case, P, packed, T)
    assert len(res) == (15 if case.arch == 0 else 13)
    for name, kind, ratio, where in res:
        assert ratio <= 1.0, (name, kind, ratio, where)
    # the activations stay alive: no layer's output is all zero, and the last trunk layer still varies
    for k, v in T.items():
        assert float(v.abs().max()) > 0 and bool(torch.isfinite(v).all()), k
    assert float(T["c2"].std()) > 1e-3


@pytest.mark.parametrize("case", [S.FnCase(1, 20, 64, 5, 0), S.FnCase(1, 20, 64, 5, 1), S.FnCase(1, 4, 4, 8, 0), S.FnCase(1, 4, 4, 8, 1)], ids=S.fn_id)
def test_featnet_model_is_the_module(case):
    """The layer list, the tensor routing and the parameter names of the scene against the project's own FeatureNet (its PyTorch
    composite, on the CPU) carrying the scene's parameters: outputs within 1e-5 of the largest magnitude -- two float32 evaluations
    of the same 15 layers; a wrong route or name moves them by the size of the values."""
    from satmvs_amd.modules.module import FeatureNet
    P = S.fn_params(case.c, case.arch)
    net = FeatureNet(base_channels=case.c, stride=4, num_stage=3, arch_mode="unet" if case.arch == 0 else "fpn").eval()
    missing, unexpected = net.load_state_dict(P, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    assert net._names() == S.fn_param_names(case.c, case.arch)
    imgs = S.fn_images(case)
    with torch.no_grad():
        y = net(imgs)
    T = S.fn_model32(case, P, S.fn_pack_reference(P, case.c, case.arch), imgs)
    for k in ("stage1", "stage2", "stage3"):
        assert float((y[k] - T[k]).abs().max()) <= 1e-5 * float(T[k].abs().max()), k


def _case(N, H, W, c, arch):
    k = S.FnCase(N, H, W, c, arch)
    assert k in S.FN_CASES
    return k


# fault, case, layer: the judge must reject the planted layer and only that one (every layer is judged on the inputs it was given)
PLANTS = [("tile-column-zero", _case(1, 20, 64, 5, 0), "conv0.1"), ("tile-column-zero", _case(2, 12, 132, 16, 0), "deconv2.deconv"),
          ("tile-column-zero", _case(3, 8, 260, 8, 1), "inner2"), ("tile-column-zero", _case(3, 8, 260, 8, 0), "conv1.0"),
          ("shift-mod-8", _case(1, 4, 4, 8, 0), "conv1.1"), ("shift-mod-8", _case(1, 36, 72, 12, 1), "inner1"),
          ("shift-mod-8", _case(1, 36, 72, 12, 0), "deconv1.deconv"),
          ("concat-swapped", _case(1, 20, 64, 5, 0), "deconv1.conv"), ("concat-swapped", _case(1, 4, 4, 8, 0), "deconv2.conv"),
          ("lateral-row-stride", _case(1, 12, 68, 4, 1), "inner1"), ("lateral-row-stride", _case(1, 4, 4, 8, 1), "inner2")]


@pytest.mark.parametrize("fault,case,layer", PLANTS, ids=["%s-%s-%s" % (f, S.fn_id(c), l) for f, c, l in PLANTS])
def test_featnet_planted_faults_fail_the_judge(fault, case, layer):
    assert fault in S.FN_FAULTS
    P = S.fn_params(case.c, case.arch)
    packed = S.fn_pack_reference(P, case.c, case.arch)
    names = [l.name for l in S.fn_layers(case.c, case.arch)]
    T = S.fn_model32(case, P, packed, S.fn_images(case), fault=fault, at=names.index(layer))
    res = {name: ratio for name, kind, ratio, where in S.fn_judge(case, P, packed, T)}
    assert res[layer] > 1.0, (fault, res[layer])
    assert all(r <= 1.0 for n, r in res.items() if n != layer), res
    assert {f for f, _, _ in PLANTS} == set(S.FN_FAULTS)


# ---- costreg ----------------------------------------------------------------------------------------------------------------------
CR_IDS = [S.cr_id(c) for c in S.CR_CASES]


@pytest.mark.parametrize("case", S.CR_CASES, ids=CR_IDS)
def test_costreg_case_is_accepted_and_layouts_match_the_library(lib, case):
    """An odd channel count (C = 5) is accepted by the entry: only conv0 sees it, on the direct row kernel."""
    assert S.cr_accepts(*case)
    lay, total = S.cr_workspace(case.B, case.D, case.H, case.W)
    assert lib.smvs_costreg_workspace_bytes(*case) == 4 * total
    assert lib.smvs_costreg_packed_floats(case.C) == S.cr_packed_layout(case.C)[1]
    assert len(S.cr_param_names()) == 51
    end = 0
    for name, (o, shape) in lay.items():
        assert o % 4 == 0 and o == end, name
        n = 1
        for d in shape:
            n *= d
        end = o + ((n + 3) & ~3)
    assert end == total
    shapes = dict({k: v[1] for k, v in lay.items()}, vol=tuple(case), out=(case.B, 1, case.D, case.H, case.W))
    for l, st in zip(S.cr_layers(case.C), S.cr_steps()):
        assert shapes[st.inp][1] == l.cin and shapes[st.out][1] == l.cout, l.name
        assert shapes[st.inp][2:] == tuple(d >> st.lin for d in case[2:]) and shapes[st.out][2:] == tuple(d >> st.lout for d in case[2:])
        assert st.lout == st.lin + (1 if l.stride == 2 and not l.transposed else -1 if l.transposed else 0)
        if st.skip:
            assert shapes[st.skip] == shapes[st.out]
    for a in [(1, 8, 12, 8, 8), (1, 8, 8, 12, 8), (1, 8, 8, 8, 12), (0, 8, 8, 8, 8), (1, 0, 8, 8, 8), (1, 8, 0, 8, 8), (1, 8, 512, 512, 8)]:
        assert lib.smvs_costreg_workspace_bytes(*a) == 0 and not S.cr_accepts(*a), a


def test_costreg_cases_reach_every_kernel_and_remainder():
    """Kernels by layer (csrc/costreg.hip: cr_variant): the 62-column row kernel with 8 and with 2 channels per lane, the stride-2 gather
    kernel, the channel-split transposed kernel (the unsplit form takes over from 512 workgroups of 64 input voxels, i.e. from 262144 voxels
    of the volume: beyond these cases; tests/test_conv_gpu.py holds it per element as a single layer), the MFMA kernel at both strides.  Widths
    against the 62-column tile: below (8), one tile and a rest (72 = 62 + 10), two tiles and a rest (136 = 124 + 12); MFMA tiles of 32
    columns: ragged (9, 17, 18, 34, 36, 68) and exact is not reachable with these widths below 256."""
    kinds, tsplit, widths = set(), set(), set()
    for case in S.CR_CASES:
        for l, st in zip(S.cr_layers(case.C), S.cr_steps()):
            kinds.add(S.cr_kind(l) + ("" if l.cout > 2 or l.transposed or l.stride == 2 else " cot2"))
            if l.transposed:
                vox = (case.D >> st.lin) * (case.H >> st.lin) * (case.W >> st.lin)
                tsplit.add(-(-vox // 64) * case.B * -(-l.cout // 8) < 512)
            if S.cr_kind(l) == "conv3d s1":
                widths.add("<62" if case.W < 62 else "62..124" if case.W <= 124 else ">124")
    assert kinds == {"conv3d s1", "conv3d s1 cot2", "conv3d s2", "convT3d", "mfma s1", "mfma s2"}
    assert tsplit == {True} and widths == {"<62", "62..124", ">124"}
    assert {c.C for c in S.CR_CASES} >= {5, 8, 32} and {c.B for c in S.CR_CASES} == {1, 2}


def test_costreg_pack_reference_is_the_definition():
    for C in (5, 8):
        P = S.cr_params(C)
        packed = S.cr_pack_reference(P, C)
        lay, total = S.cr_packed_layout(C)
        assert packed.numel() == total
        for l, (wo, so, to, wm) in zip(S.cr_layers(C), lay):
            keys = S._cr_keys(l)
            w = P[keys[0]]
            ncog = (l.cout + 7) // 8
            for cog in range(ncog):
                for ci in (0, l.cin - 1):
                    for tap in (0, 13, 26):
                        for j in range(8):
                            co = cog * 8 + j
                            want = 0.0 if co >= l.cout else float((w[ci, co] if l.transposed else w[co, ci]).reshape(-1)[tap])
                            assert float(packed[wo + ((cog * l.cin + ci) * 27 + tap) * 8 + j]) == want
            s, t = packed[so:so + ncog * 8], packed[to:to + ncog * 8]
            if l.bn:
                gamma, beta, mean, var = [P[k] for k in keys[1:]]
                assert int((gamma == 0).sum()) == 1 and bool((gamma > 0).any()) and bool((gamma < 0).any()) and int((var < 0.01).sum()) == 1
                # float32 step by step, through numpy scalars
                for c in range(l.cout):
                    sv = np.float32(gamma[c].item()) / np.sqrt(np.float32(var[c].item()) + np.float32(1e-5), dtype=np.float32)
                    assert float(s[c]) == float(sv) and float(t[c]) == float(np.float32(beta[c].item()) - np.float32(mean[c].item()) * sv)
            else:
                assert float(s[0]) == 1 and float(t[0]) == 0
            assert bool((s[l.cout:] == 1).all()) and bool((t[l.cout:] == 0).all())
            assert (wm is not None) == (l.name in ("conv3", "conv4", "conv5", "conv6"))
            if wm is not None:
                nt = l.cout // 32
                for cip in (0, l.cin // 2 - 1):
                    for p in (0, 13, 14, 26):
                        for h in (0, 1):
                            kk = 2 * p + h
                            ci, tap = 2 * cip + (1 if kk >= 27 else 0), kk % 27
                            for co in (0, 31, l.cout - 1):
                                i = (((cip * 27 + p) * nt + co // 32) * 2 + h) * 32 + co % 32
                                assert float(packed[wm + i]) == float(w[co, ci].reshape(-1)[tap])


@pytest.mark.parametrize("case", S.CR_CASES, ids=CR_IDS)
def test_costreg_float32_model_passes_the_judge_at_every_layer(case):
    P = S.cr_params(case.C)
    packed = S.cr_pack_reference(P, case.C)
    T = S.cr_model32(case, P, packed, S.cr_volume(case))
    res = S.cr_judge(case, P, packed, T)
    assert len(res) == 11
    for name, kind, ratio, where in res:
        assert ratio <= 1.0, (name, kind, ratio, where)
    for k, v in T.items():
        assert float(v.abs().max()) > 0 and bool(torch.isfinite(v).all()), k
    assert float(T["out"].std()) > 1e-3


def test_costreg_model_is_the_module():
    from satmvs_amd.modules.module import CostRegNet
    case = S.CR_CASES[3]
    P = S.cr_params(case.C)
    net = CostRegNet(case.C, 8).eval()
    missing, unexpected = net.load_state_dict(P, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    assert net._names() == S.cr_param_names()
    vol = S.cr_volume(case)
    with torch.no_grad():
        y = net(vol)
    T = S.cr_model32(case, P, S.cr_pack_reference(P, case.C), vol)
    assert float((y - T["out"]).abs().max()) <= 1e-5 * float(T["out"].abs().max())


CR_PLANTS = [("tile-column-zero", S.CR_CASES[1], "conv0"), ("tile-column-zero", S.CR_CASES[2], "prob"), ("tile-column-zero", S.CR_CASES[2], "conv11"),
             ("shift-mod-8", S.CR_CASES[0], "conv2"), ("shift-mod-8", S.CR_CASES[3], "conv5"), ("shift-mod-8", S.CR_CASES[0], "conv9"),
             ("skip-from-input", S.CR_CASES[0], "conv7"), ("skip-from-input", S.CR_CASES[3], "conv9")]


@pytest.mark.parametrize("fault,case,layer", CR_PLANTS, ids=["%s-%s-%s" % (f, S.cr_id(c), l) for f, c, l in CR_PLANTS])
def test_costreg_planted_faults_fail_the_judge(fault, case, layer):
    P = S.cr_params(case.C)
    packed = S.cr_pack_reference(P, case.C)
    names = [l.name for l in S.cr_layers(case.C)]
    T = S.cr_model32(case, P, packed, S.cr_volume(case), fault=fault, at=names.index(layer))
    res = {name: ratio for name, kind, ratio, where in S.cr_judge(case, P, packed, T)}
    assert res[layer] > 1.0, (fault, res[layer])
    assert all(r <= 1.0 for n, r in res.items() if n != layer), res
    assert {f for f, _, _ in CR_PLANTS} == set(S.CR_FAULTS)


# ---- RED: packed parameters and workspace size ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.RED_CASES, ids=[S.red_id(c) for c in S.RED_CASES])
def test_red_case_is_accepted_and_sizes_match_the_library(lib, case):
    assert S.red_accepts(*case)
    assert lib.smvs_red_workspace_bytes(*case) == 4 * S.red_workspace_floats(*case)
    packed, written = S.red_pack_reference(S.red_params(case.C), case.C)
    assert lib.smvs_red_packed_floats(case.C) == packed.numel() == written.numel()
    assert int((~written).sum()) == 7
    assert len(S.red_param_names()) == 48


def test_red_rejections_and_chunks_are_mirrored(lib):
    for a in [(1, 8, 12, 8), (1, 8, 8, 12), (0, 8, 8, 8), (1, 0, 8, 8), (1, 8, 0, 8), (1, 8, 16384, 16384)]:
        assert lib.smvs_red_workspace_bytes(*a) == 0 and not S.red_accepts(*a), a
    # both chunk lengths and the 2^30-byte cap, against the library's own workspace size
    for a in [(1, 8, 256, 512), (1, 8, 264, 512), (2, 32, 1024, 1024), (1, 64, 2048, 1024)]:
        assert lib.smvs_red_workspace_bytes(*a) == 4 * S.red_workspace_floats(*a), a
    assert [S.red_chunk(*a) for a in [(1, 8, 256, 512), (1, 8, 264, 512), (2, 32, 1024, 1024), (1, 64, 2048, 1024)]] == [8, 4, 4, 1]


def test_red_pack_reference_is_the_definition():
    """Spot checks index by index from the definitions of pack_conv_kernel (modes 0, 1, 2) and mfma_pack_kernel (9 taps), at the offsets
    red_layout gives (recomputed here from the channel counts alone)."""
    C = 5
    P = S.red_params(C)
    packed, _ = S.red_pack_reference(P, C)
    pc = lambda cin, cout: ((cout + 7) // 8) * cin * 72
    o = 0
    w = P["conv1.conv.weight"]                                      # mode 0 at offset 0: [cog][ci][tap][8]
    for co, ci, k in ((0, 0, 0), (15, 4, 8), (9, 2, 5)):
        assert float(packed[o + (((co // 8) * C + ci) * 9 + k) * 8 + co % 8]) == float(w[co, ci].reshape(-1)[k])
    o += pc(C, 16) + pc(16, 32) + pc(32, 64)
    xin = (C, 16, 32, 64)
    names = S.red_param_names()
    for g, hc in enumerate(S.RED_HID):
        cin = xin[g] + hc
        q = names[g * 10:(g + 1) * 10]
        wg = P[q[0]]
        assert float(packed[o + (((2 * hc - 1) // 8 * cin + cin - 1) * 9 + 4) * 8 + 7]) == float(wg[2 * hc - 1, cin - 1, 1, 1])
        o += pc(cin, 2 * hc)
        for k in q[1:6]:
            assert torch.equal(packed[o:o + P[k].numel()], P[k]), k
            o += P[k].numel()
        o += pc(cin, hc)
        for k in q[7:10]:
            assert torch.equal(packed[o:o + P[k].numel()], P[k]), k
            o += P[k].numel()
    for i, (ci_n, co_n) in enumerate(((16, 8), (32, 16), (64, 32))):   # mode 1: src[ci][co][k]
        w = P["upconv%d.conv.weight" % (i + 1)]
        for co, ci, k in ((0, 0, 0), (co_n - 1, ci_n - 1, 8), (3, 7, 2)):
            assert float(packed[o + (((co // 8) * ci_n + ci) * 9 + k) * 8 + co % 8]) == float(w[ci, co].reshape(-1)[k])
        o += pc(ci_n, co_n)
    w = P["upconv2d.weight"]                                         # mode 2: src[ci][0][8 - k], cout 1 padded to 8 with zeros
    for ci, k in ((0, 0), (7, 8), (3, 2)):
        assert float(packed[o + (ci * 9 + k) * 8]) == float(w[ci, 0].reshape(-1)[8 - k])
        assert float(packed[o + (ci * 9 + k) * 8 + 1]) == 0.0
    o += pc(8, 1)
    assert float(packed[o]) == float(P["upconv2d.bias"][0])
    o += 8
    # MFMA order, first such layer (conv2, 16 -> 32): dst[((((cip * nt + tl) * 2 + h) * 32 + j) * 12 + t] = w[tl * 32 + j][2 cip + h][t]
    w = P["conv2.conv.weight"]
    for cip, h, j, t in ((0, 0, 0, 0), (7, 1, 31, 8), (3, 1, 5, 4)):
        assert float(packed[o + (((cip * 1 + 0) * 2 + h) * 32 + j) * 12 + t]) == float(w[j, 2 * cip + h].reshape(-1)[t])
    assert float(packed[o + 9]) == 0.0 and float(packed[o + 11]) == 0.0
    # norm parameters are distinct per norm
    for g in range(4):
        q = names[g * 10:(g + 1) * 10]
        assert not torch.equal(P[q[2]], P[q[4]]) and not torch.equal(P[q[4]], P[q[8]]) and not torch.equal(P[q[3]], P[q[5]]) and not torch.equal(P[q[5]], P[q[9]])


# ---- RED: the plane step stage by stage ------------------------------------------------------------------------------------------------
RED_IDS = [S.red_id(c) for c in S.RED_CASES]


def test_red_workspace_mirror_and_job_kinds(lib):
    """The offsets mirror sums to the library's size for every case; the six job kinds are each chosen by some layer of some case: the
    tall case puts the level-1 gate on kind 6, the level-1 and level-2 candidates on kind 0 and its MFMA jobs on kinds 3 and 4, the small
    cases give kinds 1 and 2."""
    seen = set()
    for case in S.RED_CASES:
        lay, stats, total = S.red_workspace(*case)
        assert 4 * total == lib.smvs_red_workspace_bytes(*case) and stats % 2 == 0
        for name, (o, shape) in lay.items():
            assert o % 4 == 0, name
        seen |= set(S.red_job_kinds(case).values())
    assert seen == {0, 1, 2, 3, 4, 6}
    tall = S.red_job_kinds(S.RedCase(1, 8, 2048, 8))
    assert tall[("gate", 0)] == 6 and tall[("cand", 0)] == 0 and tall[("cand", 1)] == 0
    assert {tall[(s, g)] for s in ("gate", "cand") for g in (1, 2, 3)} - {0} == {3, 4}
    for case in S.RED_CASES[:4]:
        assert set(S.red_job_kinds(case).values()) == {1, 2}
    assert all(c in S.RED_CASES for c in S.RED_HOT_CASES)


@pytest.mark.parametrize("case,hot", [(c, False) for c in S.RED_CASES] + [(c, True) for c in S.RED_HOT_CASES],
                         ids=RED_IDS + [S.red_id(c) + "-hot" for c in S.RED_HOT_CASES])
def test_red_float32_model_passes_the_judge_at_every_stage(case, hot):
    P = S.red_params_hot(case) if hot else S.red_params(case.C)
    cost, h = S.red_inputs(case)
    T = S.red_model32(case, P, cost, h)
    res = S.red_judge(case, P, T)
    assert len(res) == 3 + 4 * (1 + 2 + 1 + 1 + 2 + 1 + 1) + 3 + 1
    for name, label, ratio, where in res:
        assert ratio <= 1.0, (name, label, ratio, where)
    if hot:
        # The scene is what it says, on a float64 evaluation of the raw outputs: the biases are set from the statistics pooled over the
        # batch (of the float32 model), so the pooled ratio is 30 to a part in a thousand; one sample's own mean and spread differ from
        # the pooled ones (the level-4 plane of a sample is 3 x 17), which the window 24 .. 37.5 allows for.
        R = S.red_raw64(case, P, cost, h)
        for g, hc in enumerate(S.RED_HID):
            for t in (R["gates%d" % g][:, :hc], R["gates%d" % g][:, hc:], R["cand%d" % g]):
                assert abs(float(t.mean() / t.std()) - S.RED_HOT) <= 1e-3 * S.RED_HOT, (g, float(t.mean() / t.std()))
                for b in range(case.B):
                    assert 0.8 * S.RED_HOT <= float(t[b].mean() / t[b].std()) <= 1.25 * S.RED_HOT, (g, b, float(t[b].mean() / t[b].std()))
    for g in range(4):                                              # the step moves the states, and they stay alive
        assert float((T["state%d" % g] - T["h%d" % g]).abs().max()) > 1e-2


def test_red_model_is_the_module():
    from satmvs_amd.modules.module import slice_RED_Regularization
    case = S.RedCase(1, 5, 16, 64)
    P = S.red_params(case.C)
    reg = slice_RED_Regularization(case.C, 8).eval()
    reg.load_state_dict(P)
    assert list(reg._PARAM_ORDER) == S.red_param_names()
    cost, h = S.red_inputs(case)
    with torch.no_grad():
        r = reg(cost, *[t.clone() for t in h])
    T = S.red_model32(case, P, cost, h)
    for got, want in zip(r, [T["out"]] + [T["state%d" % g] for g in range(4)]):
        assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())


RED_PLANTS = [(f, c, g) for f, c, g in [
    ("stats-swapped", S.RedCase(1, 8, 8, 8), 0), ("stats-swapped", S.RedCase(1, 5, 16, 64), 3),
    ("affine-swapped", S.RedCase(1, 8, 8, 8), 1), ("affine-swapped", S.RedCase(2, 8, 8, 72), 2),
    ("stats-of-sample-0", S.RedCase(2, 8, 8, 72), 0), ("stats-of-sample-0", S.RedCase(3, 32, 24, 136), 3),
    ("hsnap-stale", S.RedCase(1, 8, 8, 8), 3), ("hsnap-stale", S.RedCase(1, 5, 16, 64), 0),
    ("skip-from-old-state", S.RedCase(1, 8, 8, 8), 2), ("skip-from-old-state", S.RedCase(1, 5, 16, 64), 0),
    ("update-inverted", S.RedCase(1, 8, 8, 8), 0), ("update-inverted", S.RedCase(2, 8, 8, 72), 3)]]


@pytest.mark.parametrize("fault,case,level", RED_PLANTS, ids=["%s-%s-level%d" % (f, S.red_id(c), g + 1) for f, c, g in RED_PLANTS])
def test_red_planted_faults_fail_the_judge(fault, case, level):
    assert case in S.RED_CASES and {f for f, _, _ in RED_PLANTS} == set(S.RED_FAULTS)
    P = S.red_params(case.C)
    cost, h = S.red_inputs(case)
    res = S.red_judge(case, P, S.red_model32(case, P, cost, h, fault=fault, at=level))
    failed = {name for name, label, ratio, where in res if ratio > 1.0}
    want = {"stats-swapped": {"apply%d" % level, "combine%d" % level}, "affine-swapped": {"apply%d" % level, "combine%d" % level},
            "stats-of-sample-0": {"apply%d" % level}, "hsnap-stale": {"hsnap%d" % level}, "skip-from-old-state": {"upconv%d" % (level + 1)},
            "update-inverted": {"combine%d" % level}}[fault]
    assert failed == want, (fault, failed)


def test_native_paths_ask_for_the_kernels_eps():
    """The gate of the three _use_native: every norm at 1e-5, as a Python float or as the float32 value RED's kernels use; any other
    eps, on any one norm, sends the model to the composite."""
    from satmvs_amd.modules import module as M
    for make, kind in ((lambda: M.FeatureNet(8), torch.nn.BatchNorm2d), (lambda: M.CostRegNet(8, 8), torch.nn.BatchNorm3d),
                       (lambda: M.slice_RED_Regularization(8, 8), torch.nn.GroupNorm)):
        net = make()
        norms = [m for m in net.modules() if isinstance(m, kind)]
        assert norms and M._norm_eps_native(net)
        norms[-1].eps = float(np.float32(1e-5))
        assert norms[-1].eps != 1e-5 and M._norm_eps_native(net)
        norms[-1].eps = 1e-3
        assert not M._norm_eps_native(net)
        norms[-1].eps, norms[0].eps = 1e-5, 1.1e-5
        assert not M._norm_eps_native(net)
