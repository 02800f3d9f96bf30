"""What tests/test_conv_gpu.py assumes about tests/conv_scene.py, checked without a GPU: every case selects the kernel variant it
records (asked from the library's own selection functions), the matrix reaches every variant with every remainder class, the
threshold pairs straddle, the float64 reference is the definition, a correct float32 result passes the derived bound and planted
kernel errors do not."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_scene as S

ALL = [("2d", c) for c in S.CASES_2D] + [("3d", c) for c in S.CASES_3D]


@pytest.fixture(scope="module")
def lib():
    from satmvs_amd import build, _lib
    build.build()
    return _lib.load()


def query(lib, c, B=None):
    if len(c.dims) == 2:
        return lib.smvs_conv3x3_variant(c.kind, B or c.B, c.CA, c.CB, c.Cout, c.dims[0], c.dims[1], 0 if c.bias == "off4" else 1)
    return lib.smvs_conv3d_variant(c.kind, B or c.B, c.CA, c.Cout, *c.dims)


def test_case_names_are_unique_and_layers_exist():
    for cases in (S.CASES_2D, S.CASES_3D):
        assert len({c.name for c in cases}) == len(cases)
        for c in cases:
            assert (c.kind, c.layout) in ((0, 0), (1, 0), (2, 1), (0, 2)), c.name
            assert not (c.kind == 2 and (c.CB or c.bias)), c.name
            assert not (len(c.dims) == 3 and (c.CB or c.bias)), c.name
            assert not (len(c.dims) == 2 and c.kind == 2 and c.init), c.name


@pytest.mark.parametrize("c", [c for _, c in ALL], ids=[d + "-" + c.name for d, c in ALL])
def test_case_selects_its_variant(lib, c):
    assert query(lib, c) == c.expect


def test_every_variant_meets_every_remainder_class():
    for codes, cases, required, names in ((S.ALL_CODES_2D, S.CASES_2D, S.REQUIRED_2D, S.NAMES_2D),
                                          (S.ALL_CODES_3D, S.CASES_3D, S.REQUIRED_3D, S.NAMES_3D)):
        got = S.covered(cases)
        assert sorted(got) == sorted(codes), "variants without a case: %s" % [names[k] for k in set(codes) - set(got)]
        assert sorted(required) == sorted(codes)
        for code in codes:
            missing = required[code] - got[code]
            assert not missing, "%s lacks %s" % (names[code], sorted(missing))
    got = S.covered(S.CASES_2D)
    for stride in (S.MFMA_S1, S.MFMA_S2):
        assert S.REQUIRED_MFMA_SPLITS <= set().union(*[got[stride + f] for f in range(5)])
    # edge planes: 1 x 1, 1 x W and H x 1 for kinds 0 and 2, 2 x 2 for kind 1
    shapes = {(c.kind, c.dims if max(c.dims) <= 2 else tuple(min(d, 2) for d in c.dims)) for c in S.CASES_2D}
    for kind in (0, 2):
        assert {(kind, (1, 1)), (kind, (1, 2)), (kind, (2, 1))} <= shapes
    assert (1, (2, 2)) in {(c.kind, c.dims) for c in S.CASES_2D}


def test_threshold_pairs_straddle(lib):
    for pairs, by_name in ((S.PAIRS_2D, S.BY_NAME_2D), (S.PAIRS_3D, S.BY_NAME_3D)):
        for lo, hi in pairs:
            a, b = by_name[lo], by_name[hi]
            assert query(lib, a) == a.expect and query(lib, b) == b.expect and a.expect != b.expect, (lo, hi)
    # the counts the names claim, from the tiling include/satmvs.h documents
    def wg(c):
        h, w = c.dims if c.kind == 2 else S.out_dims(c)
        return -(-w // 64) * -(-h // 4) * c.B * -(-c.Cout // 8)

    def tiles(c):
        o = S.out_dims(c)
        return -(-o[-1] // 32) * int(np.prod(o[:-1])) * c.B
    n2 = S.BY_NAME_2D
    assert [wg(n2[k]) for k in ("split1-511", "unsplit1-512", "split2-511", "unsplit2-512", "tsplit-511", "tunsplit-512")] == [511, 512] * 3
    assert [wg(n2[k]) for k in ("split1-256-b1", "unsplit1-512-b2", "unsplit1-1023", "rows4-1024")] == [256, 512, 1023, 1024]
    assert n2["split1-256-b1"]._replace(name="", B=2, expect=0) == n2["unsplit1-512-b2"]._replace(name="", expect=0)   # batch only
    assert [tiles(n2[k]) for k in ("mfma1-k4-1022", "mfma1-k4-1023", "mfma1-nt1-1024", "mfma2-k4-1022", "mfma2-nt1-1024")] == [1022, 1023, 1024, 1022, 1024]
    n3 = S.BY_NAME_3D
    assert [tiles(n3[k]) for k in ("mfma3-1-k4-1023", "mfma3-1-nt1-1024")] == [1023, 1024]
    vol = lambda c: -(-int(np.prod(c.dims)) // 64) * c.B * -(-c.Cout // 8)
    assert [vol(n3[k]) for k in ("tsplit3-511", "tunsplit3-512")] == [511, 512]


@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("kind,layout", [(0, 0), (1, 0), (2, 1), (0, 2)])
def test_reference_is_the_definition(nd, kind, layout):
    """torch's float64 convolutions, as conv_scene.linear_part calls them, against the tap-by-tap numpy loop: every kind, all three
    weight layouts, 2-D and 3-D, at tiny shapes with odd and even sizes."""
    g = torch.Generator().manual_seed(10 * nd + 3 * kind + layout)
    dims = ((4, 6), (2, 4)) if kind == 1 else ((3, 5), (1, 2))
    for base in dims:
        d = ((2,) if kind == 1 else (3,)) * (nd - 2) + base if nd == 3 else base
        cin, cout = 3, 2
        x = torch.randn((2, cin) + d, generator=g, dtype=torch.float64)
        w = torch.randn(((cout, cin) if layout == 0 else (cin, cout)) + (3,) * nd, generator=g, dtype=torch.float64)
        want = S.loop_layer(kind, layout, x.numpy(), w.numpy())
        got = S.linear_part(kind, layout, x, w).numpy()
        assert got.shape == want.shape
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


@pytest.mark.parametrize("name", ["c1", "c2", "t2"])
@pytest.mark.parametrize("nd", [2, 3])
def test_adjoint_reference_is_the_adjoint_layer(name, nd):
    """The float64 input gradient by autograd equals the adjoint LAYER conv_scene.linear_part evaluates for the (kind, layout) the
    library's backward uses -- so the GPU adjoint test holds the entry to the gradient, and the layouts mean what the header says."""
    g = torch.Generator().manual_seed(7 + nd)
    dims = (4, 6) if nd == 2 else (2, 4, 6)
    ci, co = 3, 2
    w = torch.randn(((ci, co) if name == "t2" else (co, ci)) + (3,) * nd, generator=g, dtype=torch.float64)
    x = torch.zeros((2, ci) + dims, dtype=torch.float64)
    dy = torch.randn(S.forward_of(name, x, w).shape, generator=g, dtype=torch.float64)
    ref, bound = S.adjoint_reference(name, x.shape, w, dy)
    kind, layout = S.ADJOINT_OF[name]
    got = S.linear_part(kind, layout, dy, w)
    assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert bool((bound > 0).all())


@pytest.mark.parametrize("c", [c for _, c in ALL], ids=[d + "-" + c.name for d, c in ALL])
def test_float32_convolution_passes_the_bound(c):
    """A correct float32 evaluation (torch's CPU convolution, epilogue in float32) lies inside the bound at every element."""
    ref, bound = S.reference(c)
    got = S.layer(c, S.inputs(c), torch.float32)
    assert got.dtype == torch.float32 and got.shape == ref.shape
    ratio, where = S.worst_ratio(got, ref, bound)
    assert ratio <= 1.0, (c.name, ratio, where)


# ---- planted errors ----------------------------------------------------------------------------------------------------------
PLANT = S.BY_NAME_2D["rows4-h273-w319-cat"]          # stride 1, cat input, init, no ReLU: Ho % 16 = 1, Cout 24 = three groups of 8


def _exceeds(got, where):
    ref, bound = S.reference(PLANT)
    err = (got.float().double() - ref).abs()          # through float32, as a kernel would store it
    assert bool((err[where] > bound[where]).all()), float((err[where] / bound[where]).min())
    rest = torch.ones_like(err, dtype=torch.bool)
    rest[where] = False
    assert bool((err[rest] <= bound[rest]).all())


def test_planted_dropped_tap_at_a_corner():
    t = S.inputs(PLANT)
    ref, _ = S.reference(PLANT)
    x = torch.cat([t["xa"], t["xb"]], 1).double()
    got = ref.clone()
    got[:, :, 0, 0] -= torch.einsum("bi,oi->bo", x[:, :, 0, 0], t["w"].double()[:, :, 1, 1])       # the centre tap of pixel (0, 0)
    _exceeds(got, (slice(None), slice(None), 0, 0))


def test_planted_dropped_last_input_channel():
    t = dict(S.inputs(PLANT))
    t["xb"], t["w"] = t["xb"][:, :-1], t["w"][:, :-1]
    got = S.layer(PLANT, t)
    ref, bound = S.reference(PLANT)
    err = (got.float().double() - ref).abs()
    assert float((err > bound).double().mean()) > 0.999          # everywhere but where the channel's nine products happen to cancel


def test_planted_swapped_output_channels_of_the_tail_group():
    ref, _ = S.reference(PLANT)
    got = ref.clone()
    got[:, -1], got[:, -2] = ref[:, -2], ref[:, -1]
    ref2, bound = S.reference(PLANT)
    err = (got.float().double() - ref2).abs()
    assert float((err[:, -2:] > bound[:, -2:]).double().mean()) > 0.999 and bool((err[:, :-2] <= bound[:, :-2]).all())


def test_planted_west_tap_wraps_to_the_previous_row():
    t = S.inputs(PLANT)
    x = torch.cat([t["xa"], t["xb"]], 1).double()
    xp = F.pad(x, (1, 1, 1, 1))
    xp[:, :, 2:-1, 0] = x[:, :, :-1, -1]                 # the pad left of row iy holds the float just before it in memory: x[iy-1][W-1]
    got = F.conv2d(xp, t["w"].double()) + t["init"].double()
    ref, bound = S.reference(PLANT)
    err = (got.float().double() - ref).abs()
    assert float((err[..., 0] > bound[..., 0]).double().mean()) > 0.999 and bool((err[..., 1:] <= bound[..., 1:]).all())


def test_planted_row_of_the_last_block_left_at_init():
    ref, _ = S.reference(PLANT)
    got = ref.clone()
    got[:, :, -1] = S.inputs(PLANT)["init"][:, :, -1].double()
    ref2, bound = S.reference(PLANT)
    err = (got.float().double() - ref2).abs()
    assert float((err[:, :, -1] > bound[:, :, -1]).double().mean()) > 0.999 and bool((err[:, :, :-1] <= bound[:, :, :-1]).all())


# ---- rejected arguments --------------------------------------------------------------------------------------------------------
def test_queries_answer_rejected_arguments_with_a_negative_value(lib):
    q2, q3 = lib.smvs_conv3x3_variant, lib.smvs_conv3d_variant
    assert q2(0, 1, 8, 0, 8, 16, 16, 1) >= 0 and q3(0, 1, 8, 8, 4, 4, 4) >= 0
    bad2 = [(3, 1, 8, 0, 8, 16, 16, 1), (-1, 1, 8, 0, 8, 16, 16, 1), (0, 0, 8, 0, 8, 16, 16, 1), (0, 1, 0, 0, 8, 16, 16, 1),
            (0, 1, 8, -1, 8, 16, 16, 1), (0, 1, 8, 0, 0, 16, 16, 1), (0, 1, 8, 0, 8, 0, 16, 1), (0, 1, 8, 0, 8, 16, 0, 1),
            (1, 1, 8, 0, 8, 15, 16, 1), (1, 1, 8, 0, 8, 16, 15, 1),                   # odd H / W at stride 2
            (2, 1, 8, 8, 8, 16, 16, 1),                                                # second operand with the transposed layer
            (0, 1, 8, 0, 8, 8192, 8192, 1), (0, 1, 1, 0, 8, 8192, 8192, 1),            # input / output plane of 2^31 bytes
            (2, 1, 1, 0, 2, 8192, 8192, 1),                                            # ... of the doubled output
            (0, 65536, 1, 0, 1, 1, 1, 1), (0, 8192, 1, 0, 64, 1, 1, 1)]                # batch x groups of 8 channels > 65535
    for a in bad2:
        assert q2(*a) < 0, a
    assert q2(0, 65535, 1, 0, 8, 1, 1, 1) >= 0 and q2(0, 1, 1, 0, 1, 8192, 8191, 1) >= 0
    bad3 = [(3, 1, 8, 8, 4, 4, 4), (0, 0, 8, 8, 4, 4, 4), (0, 1, 0, 8, 4, 4, 4), (0, 1, 8, 0, 4, 4, 4), (0, 1, 8, 8, 0, 4, 4),
            (1, 1, 8, 8, 3, 4, 4), (1, 1, 8, 8, 4, 4, 5),                             # odd dimension at stride 2
            (0, 1, 8, 8, 1024, 1024, 128), (2, 1, 1, 8, 256, 256, 256),               # 4 GiB input / output per sample
            (0, 1, 1, 1, 1024, 1024, 1), (0, 65536, 1, 1, 1, 1, 1)]                   # rows / batch beyond one launch grid
    for a in bad3:
        assert q3(*a) < 0, a
