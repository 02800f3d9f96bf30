"""Cases, float64 reference and per-element error bound for the single-layer convolution entries smvs_conv3x3_fwd (csrc/red.hip,
csrc/mfma_conv.h) and smvs_conv3d_fwd (csrc/costreg.hip).  Shared by tests/test_conv_cpu.py (which asserts, without a GPU, what the GPU
tests assume about these cases, the reference and the bound) and tests/test_conv_gpu.py.

A layer is (kind, layout, weight):
    layout 0, kind 0 / 1: correlation, stride 1 / 2, pad 1, weight (Cout, Cin, 3, 3[, 3])
    layout 1, kind 2:     transposed convolution, stride 2, pad 1, output_padding 1, weight (Cin, Cout, 3, 3[, 3])
    layout 2, kind 0:     transposed convolution, stride 1, pad 1 (a correlation with flipped taps), weight (Cin, Cout, 3, 3[, 3])
With layouts 1 and 2 these are also the input gradients of the stride-2 and stride-1 correlations; layout 0, kind 1 that of the
stride-2 transposed layer.

Every case is the smallest shape that selects its kernel variant together with one remainder class of that variant's tiling, and
records the variant code the library's query must report for it (include/satmvs.h).  Nothing here imports the kernels."""
import functools
import itertools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24            # unit roundoff of float32
TINY = 2.0 ** -126          # smallest normal float32: an underflowing product loses at most this

# variant codes of include/satmvs.h
SPLIT_S1, SPLIT_S2, UNSPLIT_S1, UNSPLIT_S2, ROWS4, T_SPLIT, T_UNSPLIT, MFMA_S1, MFMA_S2 = 0, 1, 2, 3, 4, 5, 6, 10, 20
D3_S1_COT2, D3_S1_COT8, D3_S2, D3_T_SPLIT, D3_T_UNSPLIT = 0, 1, 2, 3, 4
K8, K4, NT1, NT2, NT4 = 0, 1, 2, 3, 4
ALL_CODES_2D = [SPLIT_S1, SPLIT_S2, UNSPLIT_S1, UNSPLIT_S2, ROWS4, T_SPLIT, T_UNSPLIT] + [s + f for s in (MFMA_S1, MFMA_S2) for f in range(5)]
ALL_CODES_3D = [D3_S1_COT2, D3_S1_COT8, D3_S2, D3_T_SPLIT, D3_T_UNSPLIT] + [s + f for s in (MFMA_S1, MFMA_S2) for f in range(5)]
NAMES_2D = {SPLIT_S1: "direct split s1", SPLIT_S2: "direct split s2", UNSPLIT_S1: "direct unsplit s1", UNSPLIT_S2: "direct unsplit s2",
            ROWS4: "direct four rows", T_SPLIT: "transposed split", T_UNSPLIT: "transposed unsplit"}
NAMES_3D = {D3_S1_COT2: "3-D s1 cot2", D3_S1_COT8: "3-D s1 cot8", D3_S2: "3-D s2", D3_T_SPLIT: "3-D transposed split",
            D3_T_UNSPLIT: "3-D transposed unsplit"}
for _s, _sn in ((MFMA_S1, "s1"), (MFMA_S2, "s2")):
    for _f, _fn in enumerate(("K8", "K4", "NT1", "NT2", "NT4")):
        NAMES_2D[_s + _f] = "mfma %s %s" % (_sn, _fn)
        NAMES_3D[_s + _f] = "3-D mfma %s %s" % (_sn, _fn)

# dims = the INPUT plane (H, W) or volume (D, H, W).  bias: None / "aligned" / "off4" (pointer 4 bytes past a 16-byte boundary);
# init: the tensor added to the sums (2-D `init`, 3-D `skip`); hot: one input channel with |mean| >> std; expect: variant code
Case = namedtuple("Case", "name kind layout B CA CB Cout dims bias init relu hot expect")


def _c(name, kind, B, CA, CB, Cout, dims, expect, bias=None, init=False, relu=False, hot=False, layout=None):
    return Case(name, kind, (1 if kind == 2 else 0) if layout is None else layout, B, CA, CB, Cout, tuple(dims), bias, init, relu, hot, expect)


# ---- 2-D --------------------------------------------------------------------------------------------------------------------------
# Workgroups of a direct launch: ceil(Wo/64) * ceil(Ho/4) * B * ceil(Cout/8) (transposed: of the input plane); below 512 the
# channel-split forms run; stride 1 with >= 1024 workgroups in ONE sample runs four rows per lane.  MFMA tiles: ceil(Wo/32) * Ho * B.
CASES_2D = [
    # direct, channel-split, stride 1
    _c("split1-1x1", 0, 1, 1, 0, 1, (1, 1), SPLIT_S1, bias="aligned"),
    _c("split1-1xW", 0, 1, 2, 0, 3, (1, 70), SPLIT_S1, init=True),
    _c("split1-Hx1", 0, 3, 3, 0, 9, (9, 1), SPLIT_S1, relu=True),
    _c("split1-w65", 0, 1, 1, 0, 1, (5, 65), SPLIT_S1, bias="aligned", relu=True, hot=True),
    _c("split1-w63-b3", 0, 3, 2, 0, 3, (3, 63), SPLIT_S1, init=True),
    _c("split1-w64-ca3", 0, 1, 3, 0, 9, (7, 64), SPLIT_S1, bias="off4"),
    _c("split1-w127-cat", 0, 1, 2, 3, 24, (6, 127), SPLIT_S1, bias="aligned", init=True, relu=True),
    _c("split1-cin7", 0, 1, 4, 3, 8, (5, 33), SPLIT_S1),
    _c("split1-t1-layout2", 0, 1, 5, 0, 3, (6, 65), SPLIT_S1, bias="aligned", layout=2),
    _c("split1-mfma-shape-bias-off4", 0, 1, 16, 0, 32, (5, 33), SPLIT_S1, bias="off4"),     # the MFMA kernel wants an aligned bias
    _c("split1-511", 0, 7, 2, 0, 8, (291, 63), SPLIT_S1, hot=True),                          # 1 * 73 * 7 * 1 = 511
    _c("split1-256-b1", 0, 1, 1, 0, 8, (512, 100), SPLIT_S1),                                # 2 * 128 * 1: the batch pair of "b2" below
    # direct, channel-split, stride 2
    _c("split2-2x2", 1, 1, 2, 0, 1, (2, 2), SPLIT_S2, bias="aligned"),
    _c("split2-w65", 1, 1, 1, 0, 3, (10, 130), SPLIT_S2, init=True, hot=True),
    _c("split2-w63-b3-cat", 1, 3, 2, 3, 9, (6, 126), SPLIT_S2, bias="off4", relu=True),
    _c("split2-w64-cin7", 1, 1, 7, 0, 24, (4, 128), SPLIT_S2),
    _c("split2-cin3", 1, 1, 3, 0, 3, (6, 70), SPLIT_S2, relu=True),
    _c("split2-511", 1, 7, 2, 0, 8, (582, 126), SPLIT_S2),
    # direct, unsplit, stride 1 (>= 512 workgroups, < 1024 in one sample)
    _c("unsplit1-512", 0, 8, 2, 0, 8, (253, 64), UNSPLIT_S1),                                # 1 * 64 * 8 * 1 = 512
    _c("unsplit1-512-b2", 0, 2, 1, 0, 8, (512, 100), UNSPLIT_S1),
    _c("unsplit1-w63-h225-b3", 0, 3, 3, 0, 24, (225, 63), UNSPLIT_S1, bias="aligned", relu=True, hot=True),   # 57 * 3 * 3 = 513
    _c("unsplit1-w65-h511-cat", 0, 1, 2, 3, 9, (511, 65), UNSPLIT_S1, init=True),            # 2 * 128 * 2 = 512
    _c("unsplit1-w128-h341-b3-cin7", 0, 3, 4, 3, 1, (341, 128), UNSPLIT_S1, bias="off4"),    # 2 * 86 * 3 = 516
    _c("unsplit1-w192-h683-cin1", 0, 1, 1, 0, 3, (683, 192), UNSPLIT_S1),                    # 3 * 171 = 513
    _c("unsplit1-1023", 0, 1, 2, 0, 8, (372, 704), UNSPLIT_S1),                              # 11 * 93 = 1023
    # direct, unsplit, stride 2
    _c("unsplit2-512", 1, 8, 2, 0, 8, (506, 128), UNSPLIT_S2),
    _c("unsplit2-w63-h225-b3-cat", 1, 3, 2, 3, 24, (450, 126), UNSPLIT_S2, bias="aligned", init=True, hot=True),
    _c("unsplit2-w65-h511-cin1", 1, 1, 1, 0, 9, (1022, 130), UNSPLIT_S2, relu=True),
    _c("unsplit2-w128-h341-b3-ca7", 1, 3, 7, 0, 1, (682, 256), UNSPLIT_S2),
    _c("unsplit2-w192-h683-cin3", 1, 1, 3, 0, 3, (1366, 384), UNSPLIT_S2, bias="off4"),
    # direct, four rows per lane
    _c("rows4-1024", 0, 1, 2, 0, 8, (256, 1024), ROWS4),                                     # 16 * 64 = 1024
    _c("rows4-h277-w257", 0, 1, 3, 0, 24, (277, 257), ROWS4, bias="aligned", relu=True, hot=True),   # 5 * 70 * 3 = 1050
    _c("rows4-h273-w319-cat", 0, 1, 2, 3, 24, (273, 319), ROWS4, init=True),                 # 5 * 69 * 3 = 1035
    _c("rows4-h287-w320-b3", 0, 3, 1, 0, 17, (287, 320), ROWS4, bias="off4", init=True),     # 5 * 72 * 3 = 1080
    _c("rows4-cin7-cout9", 0, 1, 4, 3, 9, (415, 321), ROWS4),                                # 6 * 104 * 2 = 1248
    _c("rows4-cout1", 0, 1, 2, 0, 1, (64, 4096), ROWS4, bias="aligned"),                     # 64 * 16 = 1024
    _c("rows4-cout3", 0, 1, 3, 0, 3, (65, 4033), ROWS4, relu=True),                          # 64 * 17 = 1088
    # transposed
    _c("tsplit-1x1", 2, 1, 1, 0, 1, (1, 1), T_SPLIT),
    _c("tsplit-1xW", 2, 1, 2, 0, 3, (1, 70), T_SPLIT),
    _c("tsplit-Hx1", 2, 3, 3, 0, 9, (9, 1), T_SPLIT, relu=True),
    _c("tsplit-w65", 2, 1, 3, 0, 9, (5, 65), T_SPLIT, hot=True),
    _c("tsplit-w63-b3", 2, 3, 5, 0, 24, (3, 63), T_SPLIT),
    _c("tsplit-511", 2, 7, 2, 0, 8, (291, 63), T_SPLIT),
    _c("tunsplit-512", 2, 8, 2, 0, 8, (253, 64), T_UNSPLIT),
    _c("tunsplit-w63-h225-b3", 2, 3, 7, 0, 24, (225, 63), T_UNSPLIT, relu=True, hot=True),
    _c("tunsplit-w65-h511", 2, 1, 1, 0, 9, (511, 65), T_UNSPLIT),
    _c("tunsplit-Hx1", 2, 1, 2, 0, 8, (2045, 1), T_UNSPLIT),                                 # 1 * 512 = 512
    _c("tunsplit-1xW", 2, 1, 2, 0, 3, (1, 32705), T_UNSPLIT),                                # 512 * 1 = 512
    # MFMA, stride 1: below 1024 tiles K8 ((Cin/2) % 8 == 0) / K4, from 1024 tiles NT = Cout / 32
    _c("mfma1-k8-w33", 0, 1, 16, 0, 32, (5, 33), MFMA_S1 + K8, bias="aligned", hot=True),
    _c("mfma1-k8-w95-ca8", 0, 1, 8, 8, 64, (4, 95), MFMA_S1 + K8, init=True, relu=True),
    _c("mfma1-k8-ca6", 0, 3, 6, 10, 32, (3, 64), MFMA_S1 + K8),
    _c("mfma1-k4-w31-ca2-b3", 0, 3, 2, 6, 64, (7, 31), MFMA_S1 + K4, bias="aligned", relu=True, hot=True),
    _c("mfma1-k4-w64-ca6", 0, 1, 6, 2, 128, (3, 64), MFMA_S1 + K4, init=True),
    _c("mfma1-k4-layout2", 0, 1, 8, 0, 32, (6, 33), MFMA_S1 + K4, layout=2),
    _c("mfma1-k4-1022", 0, 1, 8, 0, 32, (511, 33), MFMA_S1 + K4),
    _c("mfma1-k4-1023", 0, 1, 8, 0, 32, (341, 65), MFMA_S1 + K4),
    _c("mfma1-nt1-1024", 0, 1, 8, 0, 32, (512, 33), MFMA_S1 + NT1, bias="aligned", hot=True),
    _c("mfma1-nt1-b3", 0, 3, 2, 6, 32, (171, 64), MFMA_S1 + NT1, init=True, relu=True),
    _c("mfma1-nt2-w63", 0, 1, 2, 6, 64, (512, 63), MFMA_S1 + NT2, bias="aligned", init=True, hot=True),
    _c("mfma1-nt4-w64", 0, 1, 8, 8, 128, (512, 64), MFMA_S1 + NT4, relu=True, hot=True),
    _c("mfma1-nt1-w31", 0, 1, 8, 0, 32, (1024, 31), MFMA_S1 + NT1),
    _c("mfma1-nt2-w33", 0, 1, 8, 0, 64, (512, 33), MFMA_S1 + NT2, relu=True),
    _c("mfma1-nt2-w64", 0, 1, 8, 8, 64, (512, 64), MFMA_S1 + NT2),
    _c("mfma1-nt4-w33", 0, 1, 6, 2, 128, (512, 33), MFMA_S1 + NT4, bias="aligned", hot=True),
    _c("mfma1-nt4-w31", 0, 1, 8, 0, 128, (1024, 31), MFMA_S1 + NT4, init=True),
    # MFMA, stride 2
    _c("mfma2-k8-w31", 1, 1, 8, 8, 32, (8, 62), MFMA_S2 + K8, relu=True),
    _c("mfma2-k8-w64", 1, 1, 16, 0, 32, (6, 128), MFMA_S2 + K8),
    _c("mfma2-k4-w32", 1, 1, 2, 6, 64, (8, 64), MFMA_S2 + K4, bias="aligned"),
    _c("mfma2-nt1-w31", 1, 1, 8, 0, 32, (2048, 62), MFMA_S2 + NT1),
    _c("mfma2-nt1-w64", 1, 1, 2, 6, 32, (1024, 128), MFMA_S2 + NT1, init=True),
    _c("mfma2-nt2-w33", 1, 1, 8, 0, 64, (1024, 66), MFMA_S2 + NT2, init=True, hot=True),
    _c("mfma2-nt2-w31", 1, 1, 8, 0, 64, (2048, 62), MFMA_S2 + NT2, relu=True),
    _c("mfma2-nt4-w33", 1, 1, 8, 0, 128, (1024, 66), MFMA_S2 + NT4),
    _c("mfma2-nt4-w64", 1, 1, 8, 8, 128, (1024, 128), MFMA_S2 + NT4, bias="aligned", relu=True),
    _c("mfma2-k8-w33", 1, 1, 16, 0, 32, (10, 66), MFMA_S2 + K8, bias="aligned", hot=True),
    _c("mfma2-k4-w31", 1, 3, 4, 4, 64, (12, 62), MFMA_S2 + K4, init=True, hot=True),
    _c("mfma2-k4-1022", 1, 1, 8, 0, 32, (1022, 66), MFMA_S2 + K4),
    _c("mfma2-nt1-1024", 1, 1, 8, 0, 32, (1024, 66), MFMA_S2 + NT1, relu=True, hot=True),
    _c("mfma2-nt2-w64", 1, 1, 6, 2, 64, (1024, 128), MFMA_S2 + NT2, bias="aligned", hot=True),
    _c("mfma2-nt4-w31", 1, 1, 8, 0, 128, (2048, 62), MFMA_S2 + NT4, init=True, hot=True),
]
# (below, at-or-above) the 512-workgroup, the 1024-workgroup and the 1024-tile thresholds: members must report different codes
PAIRS_2D = [("split1-511", "unsplit1-512"), ("split2-511", "unsplit2-512"), ("split1-256-b1", "unsplit1-512-b2"),
            ("unsplit1-1023", "rows4-1024"), ("tsplit-511", "tunsplit-512"),
            ("mfma1-k4-1022", "mfma1-nt1-1024"), ("mfma1-k4-1023", "mfma1-nt1-1024"), ("mfma2-k4-1022", "mfma2-nt1-1024")]

# ---- 3-D --------------------------------------------------------------------------------------------------------------------------
# Stride-1 rows run on 62-column tiles, 4 (d, y) rows per workgroup; the transposed layer splits below 512 workgroups of 64 linear
# input voxels: ceil(Di*Hi*Wi/64) * B * ceil(Cout/8); MFMA tiles: ceil(Wo/32) * Ho * Do * B.
CASES_3D = [
    _c("s1cot2-w63", 0, 1, 3, 0, 1, (3, 3, 63), D3_S1_COT2, init=True, hot=True),
    _c("s1cot2-w61-d1", 0, 1, 2, 0, 2, (1, 5, 61), D3_S1_COT2, relu=True),
    _c("s1cot2-w62-b3", 0, 3, 1, 0, 1, (2, 3, 62), D3_S1_COT2),
    _c("s1cot2-1x1x1", 0, 1, 1, 0, 1, (1, 1, 1), D3_S1_COT2),
    _c("s1cot8-w63-cout3", 0, 1, 2, 0, 3, (2, 3, 63), D3_S1_COT8, relu=True, hot=True),
    _c("s1cot8-w123-cout9-d1", 0, 1, 3, 0, 9, (1, 7, 123), D3_S1_COT8, init=True),
    _c("s1cot8-w124-b3", 0, 3, 5, 0, 8, (3, 2, 124), D3_S1_COT8),
    _c("s1cot8-layout2", 0, 1, 4, 0, 3, (3, 3, 65), D3_S1_COT8, layout=2),
    _c("s2-odd-halves", 1, 1, 3, 0, 3, (6, 10, 130), D3_S2, init=True, hot=True),
    _c("s2-w63-b3-cout9", 1, 3, 2, 0, 9, (2, 2, 126), D3_S2, relu=True),
    _c("s2-cout1-2x2x2", 1, 1, 1, 0, 1, (2, 2, 2), D3_S2),
    _c("tsplit3-1x1x1", 2, 1, 1, 0, 1, (1, 1, 1), D3_T_SPLIT),
    _c("tsplit3-odd", 2, 1, 3, 0, 9, (3, 5, 7), D3_T_SPLIT, init=True, relu=True, hot=True),
    _c("tsplit3-511", 2, 7, 2, 0, 8, (3, 19, 81), D3_T_SPLIT),                               # 73 * 7 = 511
    _c("tunsplit3-512", 2, 8, 2, 0, 8, (3, 17, 80), D3_T_UNSPLIT),                           # 64 * 8 = 512
    _c("tunsplit3-w65-cout9", 2, 1, 2, 0, 9, (5, 51, 65), D3_T_UNSPLIT, init=True, hot=True),   # 259 * 2 = 518
    _c("mfma3-1-k8", 0, 1, 16, 0, 32, (3, 5, 33), MFMA_S1 + K8, init=True, hot=True),
    _c("mfma3-1-k4-b3", 0, 3, 8, 0, 64, (2, 3, 31), MFMA_S1 + K4, relu=True, hot=True),
    _c("mfma3-1-k4-1023", 0, 1, 8, 0, 32, (31, 33, 32), MFMA_S1 + K4),
    _c("mfma3-1-nt1-1024", 0, 1, 8, 0, 32, (32, 16, 33), MFMA_S1 + NT1, init=True, hot=True),
    _c("mfma3-1-nt2", 0, 1, 8, 0, 64, (32, 16, 33), MFMA_S1 + NT2, relu=True, hot=True),
    _c("mfma3-1-nt4", 0, 1, 8, 0, 128, (16, 32, 63), MFMA_S1 + NT4, hot=True),
    _c("mfma3-1-layout2", 0, 1, 8, 0, 32, (3, 3, 33), MFMA_S1 + K4, layout=2),
    _c("mfma3-2-k8", 1, 1, 16, 0, 32, (4, 6, 66), MFMA_S2 + K8, hot=True),
    _c("mfma3-2-k4", 1, 1, 8, 0, 64, (2, 6, 62), MFMA_S2 + K4, init=True, hot=True),
    _c("mfma3-2-nt1", 1, 1, 8, 0, 32, (64, 32, 66), MFMA_S2 + NT1, hot=True),
    _c("mfma3-2-nt2", 1, 1, 8, 0, 64, (32, 64, 126), MFMA_S2 + NT2, relu=True, hot=True),
    _c("mfma3-2-nt4", 1, 1, 8, 0, 128, (32, 64, 126), MFMA_S2 + NT4, init=True, hot=True),
]
PAIRS_3D = [("tsplit3-511", "tunsplit3-512"), ("mfma3-1-k4-1023", "mfma3-1-nt1-1024")]

BY_NAME_2D = {c.name: c for c in CASES_2D}
BY_NAME_3D = {c.name: c for c in CASES_3D}


def stride_of(c):
    return 2 if c.kind else 1


def out_dims(c):
    return tuple(d // 2 if c.kind == 1 else d * 2 if c.kind == 2 else d for d in c.dims)


# ---- remainder classes a case covers, and the classes each variant must be seen with ------------------------------------------
def classes(c):
    """The tiling remainders, channel counts and operand splits a case exercises, as tags."""
    nd = len(c.dims)
    o = out_dims(c)
    cin = c.CA + c.CB
    t = set()
    if nd == 2:
        Ho, Wo = o
        if c.expect >= MFMA_S1:
            t.add("Wo%%32=%d" % (Wo % 32))
            t.add("pairs%8=0" if (cin // 2) % 8 == 0 else "pairs%8!=0")
            if c.CB:
                t.add("CA=%d" % c.CA)
        elif c.kind == 2:
            Hi, Wi = c.dims
            t.update({"Wi%%64=%d" % (Wi % 64), "Hi%4!=0" if Hi % 4 else "Hi%4=0"})
            if Hi == 1 or Wi == 1:
                t.add("far-taps-outside")
        else:
            t.add("Wo%%64=%d" % (Wo % 64))
            t.add("Ho%%16=%d" % (Ho % 16) if c.expect == ROWS4 else "Ho%%4=%d" % (Ho % 4))
            t.update({"Cout=%d" % c.Cout, "Cin=%d" % cin})
            if c.CA % 2 and not c.CB:
                t.add("CA-odd-alone")
            if c.CB and c.CA % 2 == 0:
                t.add("CA-even-cat")
            if c.bias == "off4":
                t.add("bias-off4")
    else:
        Do, Ho, Wo = o
        if c.expect >= MFMA_S1:
            t.add("Wo%32!=0" if Wo % 32 else "Wo%32=0")
        elif c.kind == 0:
            t.update({"Wo%%62=%d" % (Wo % 62), "Cout=%d" % c.Cout})
            if (Ho * Do) % 4:
                t.add("rows%4!=0")
            if c.dims[0] == 1:
                t.add("Di=1")
        elif c.kind == 1:
            if all(d % 2 for d in o):
                t.add("odd-halves")
    t.add("B=%d" % c.B)
    if c.hot:
        t.add("hot")
    return t


# Derived from the lists per variant group, not from what the matrix holds.  Every direct correlation form: all column remainders, its
# row remainders, Cout 1 / 3 / 9 / 24 (Cout % 8 != 0), Cin 1 / 2 / 3 / 5 / 7, an odd operand alone, an even one with a second, B = 1 and 3.
# Every MFMA code: all three column remainders.  Classes a variant cannot meet, and so are absent on purpose:
#   K8 runs only with (Cin / 2) % 8 == 0 and K4 (below 1024 tiles) only otherwise -- that IS the selection between them;
#   the four-rows form has no stride 2; the 2 x 2 plane of kind 1 and the 1 x 1 / 1 x W / H x 1 planes of kind 0 give too few
#   workgroups for anything but the split forms (the transposed unsplit form does reach Hi = 1 and Wi = 1, and must).
_DIRECT = {"Wo%64=1", "Wo%64=63", "Wo%64=0", "Cout=1", "Cout=3", "Cout=9", "Cout=24", "Cin=1", "Cin=2", "Cin=3", "Cin=5", "Cin=7",
           "CA-odd-alone", "CA-even-cat", "B=1", "B=3", "hot"}
_MFMA = {"Wo%32=1", "Wo%32=31", "Wo%32=0", "hot"}
REQUIRED_2D = {
    SPLIT_S1: _DIRECT | {"bias-off4"},       # the MFMA-shaped layer whose bias is not 16-byte aligned lands here
    SPLIT_S2: _DIRECT,
    UNSPLIT_S1: _DIRECT | {"Ho%4=1", "Ho%4=3"},
    UNSPLIT_S2: _DIRECT | {"Ho%4=1", "Ho%4=3"},
    ROWS4: _DIRECT | {"Ho%16=1", "Ho%16=5", "Ho%16=15"},
    T_SPLIT: {"Wi%64=1", "Wi%64=63", "Hi%4!=0", "far-taps-outside", "B=1", "B=3", "hot"},
    T_UNSPLIT: {"Wi%64=1", "Wi%64=63", "Hi%4!=0", "far-taps-outside", "B=1", "B=3", "hot"},
    MFMA_S1 + K8: _MFMA | {"pairs%8=0"}, MFMA_S1 + K4: _MFMA | {"pairs%8!=0", "B=3"},
    MFMA_S1 + NT1: _MFMA | {"B=3"}, MFMA_S1 + NT2: _MFMA | {"pairs%8=0", "pairs%8!=0"}, MFMA_S1 + NT4: _MFMA | {"pairs%8=0", "pairs%8!=0"},
    MFMA_S2 + K8: _MFMA | {"pairs%8=0"}, MFMA_S2 + K4: _MFMA | {"pairs%8!=0", "B=3"},
    MFMA_S2 + NT1: _MFMA, MFMA_S2 + NT2: _MFMA, MFMA_S2 + NT4: _MFMA | {"pairs%8=0", "pairs%8!=0"},
}
# ... and over the MFMA codes of each stride together: the boundary between the two operands at 2, 6 and 8 channels
REQUIRED_MFMA_SPLITS = {"CA=2", "CA=6", "CA=8"}
REQUIRED_3D = {
    D3_S1_COT2: {"Wo%62=1", "Wo%62=61", "Wo%62=0", "Cout=1", "Cout=2", "rows%4!=0", "Di=1", "B=3", "hot"},
    D3_S1_COT8: {"Wo%62=1", "Wo%62=61", "Wo%62=0", "Cout=3", "Cout=9", "rows%4!=0", "Di=1", "B=3", "hot"},
    D3_S2: {"odd-halves", "B=3", "hot"},
    D3_T_SPLIT: {"hot"}, D3_T_UNSPLIT: {"hot"},          # the pair of PAIRS_3D puts them on both sides of the 512 threshold
}
for _code in range(5):                                  # the five MFMA forms, both strides, each at a ragged last tile
    REQUIRED_3D[MFMA_S1 + _code] = {"hot", "Wo%32!=0"}
    REQUIRED_3D[MFMA_S2 + _code] = {"hot", "Wo%32!=0"}


def ragged(c):
    """the last tile of a row is partial (2-D: 64 columns, MFMA 32; 3-D MFMA: 32)"""
    Wo = out_dims(c)[-1]
    if c.expect >= MFMA_S1:
        return Wo % 32 != 0
    return len(c.dims) == 3 or (c.dims[-1] if c.kind == 2 else Wo) % 64 != 0


def covered(cases):
    """variant code -> union of the classes of the cases that expect it"""
    got = {}
    for c in cases:
        got.setdefault(c.expect, set()).update(classes(c))
    return got


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _seed(c):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)) % (2 ** 31)


@functools.lru_cache(maxsize=None)
def inputs(c):
    """-> dict of float32 CPU tensors: xa, xb (or None), w, bias (or None), init (or None).  Seeded randn; a hot case carries
    100 +- 1 on the last channel of xa (|mean| >> std: cancellation against the other channels' sums)."""
    g = torch.Generator().manual_seed(_seed(c))
    nd = len(c.dims)
    cin = c.CA + c.CB
    xa = torch.randn((c.B, c.CA) + c.dims, generator=g)
    if c.hot:
        xa[:, -1] += 100.0
    xb = torch.randn((c.B, c.CB) + c.dims, generator=g) if c.CB else None
    wshape = ((c.Cout, cin) if c.layout == 0 else (cin, c.Cout)) + (3,) * nd
    w = torch.randn(wshape, generator=g) / (3.0 ** nd * cin) ** 0.5
    bias = torch.randn((c.Cout,), generator=g) if c.bias else None
    init = torch.randn((c.B, c.Cout) + out_dims(c), generator=g) if c.init else None
    return {"xa": xa, "xb": xb, "w": w, "bias": bias, "init": init}


# ---- the layer in float64 -------------------------------------------------------------------------------------------------------
def linear_part(kind, layout, x, w):
    """The convolution itself, in the dtype of x / w; x (B, Cin, *dims), w as the layout says."""
    nd = x.dim() - 2
    conv, convT = (F.conv2d, F.conv_transpose2d) if nd == 2 else (F.conv3d, F.conv_transpose3d)
    if layout == 0 and kind in (0, 1):
        return conv(x, w, stride=kind + 1, padding=1)
    if layout == 1 and kind == 2:
        return convT(x, w, stride=2, padding=1, output_padding=1)
    if layout == 2 and kind == 0:
        return convT(x, w, stride=1, padding=1)
    raise ValueError("no layer with kind %d and layout %d" % (kind, layout))


def layer(c, t, dtype=torch.float64):
    """out of the entry for case c on the tensors t (inputs(c) or a modified copy), evaluated in `dtype` on the CPU.
    2-D: relu(conv(cat(xa, xb)) + init + bias);  3-D: relu(conv(x)) + skip (init is the entry's `skip`)."""
    x = t["xa"] if t["xb"] is None else torch.cat([t["xa"], t["xb"]], 1)
    y = linear_part(c.kind, c.layout, x.to(dtype), t["w"].to(dtype))
    nd = len(c.dims)
    if nd == 2:
        if t["init"] is not None:
            y = y + t["init"].to(dtype)
        if t["bias"] is not None:
            y = y + t["bias"].to(dtype).view((1, -1) + (1,) * nd)
        return F.relu(y) if c.relu else y
    y = F.relu(y) if c.relu else y
    return y + t["init"].to(dtype) if t["init"] is not None else y


def taps(c):
    """n of the bound: products summed into one output (an upper count: the transposed forms use at most this many)"""
    return 3 ** len(c.dims) * (c.CA + c.CB)


def bound_from(n, A, init=None, bias=None):
    """|got - ref| <= (n + 2) u (A + |init| + |bias|) + n 2^-126 per element.  A = the same linear layer in float64 on |x|, |w|.
    Any summation order of n correctly rounded fused multiply-adds (or of products and sums: each product then carries one more
    rounding, still within the n + 2 budget's first-order slack used here) onto the running sum, followed by the additions of init
    and bias, moves the result by at most gamma_{n+2} times the sum of the magnitudes; n * 2^-126 covers products that underflow.
    ReLU is 1-Lipschitz."""
    m = A.clone()
    if init is not None:
        m = m + init.double().abs()
    if bias is not None:
        m = m + bias.double().abs().view((1, -1) + (1,) * (A.dim() - 2))
    return (n + 2) * U32 * m + n * TINY


@functools.lru_cache(maxsize=None)
def reference(c):
    """-> (ref float64, bound float64), both of the output's shape.  Computed once per case and shared; do not modify."""
    t = inputs(c)
    ref = layer(c, t)
    x = t["xa"] if t["xb"] is None else torch.cat([t["xa"], t["xb"]], 1)
    A = linear_part(c.kind, c.layout, x.double().abs(), t["w"].double().abs())
    return ref, bound_from(taps(c), A, t["init"], t["bias"])


def worst_ratio(got, ref, bound):
    """largest err / bound and where; a non-finite `got` where ref is finite counts as infinite"""
    err = (got.double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    r = err / bound
    i = int(torch.argmax(r))
    return float(r.flatten()[i]), tuple(int(v) for v in np.unravel_index(i, tuple(r.shape)))


# ---- the adjoint use of the entries: input gradients ---------------------------------------------------------------------------
# layer kind -> (entry kind, layout) of its input gradient (modules/train_fns.py: _NATIVE_KINDS)
ADJOINT_OF = {"c1": (0, 2), "c2": (2, 1), "t2": (1, 0)}


def forward_of(name, x, w):
    nd = x.dim() - 2
    conv, convT = (F.conv2d, F.conv_transpose2d) if nd == 2 else (F.conv3d, F.conv_transpose3d)
    if name == "c1":
        return conv(x, w, stride=1, padding=1)
    if name == "c2":
        return conv(x, w, stride=2, padding=1)
    return convT(x, w, stride=2, padding=1, output_padding=1)


def adjoint_reference(name, x_shape, w, dy):
    """float64 input gradient of layer `name` with weight w at output gradient dy, and its bound (n from the adjoint's own channel
    count = channels of dy), both by autograd through the float64 forward (the bound: through the forward on |w| with |dy|)."""
    def grad(wv, dyv):
        x = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
        y = forward_of(name, x, wv)
        return torch.autograd.grad(y, x, dyv)[0]
    ref = grad(w.double(), dy.double())
    A = grad(w.double().abs(), dy.double().abs())
    n = 3 ** (len(x_shape) - 2) * dy.shape[1]
    return ref, bound_from(n, A)


# ---- an independent plain loop (tiny cases only) -----------------------------------------------------------------------------
def loop_layer(kind, layout, x, w):
    """The definition, tap by tap in numpy float64: no library convolution.  x (B, Cin, *dims), w as the layout says."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    nd = x.ndim - 2
    B, cin = x.shape[:2]
    dims = x.shape[2:]
    cout = w.shape[0] if layout == 0 else w.shape[1]
    s = 2 if kind else 1
    od = tuple(d // 2 if kind == 1 else d * 2 if kind == 2 else d for d in dims)
    out = np.zeros((B, cout) + od)
    for b, co, ci in itertools.product(range(B), range(cout), range(cin)):
        for k in itertools.product(range(3), repeat=nd):
            for p in itertools.product(*[range(d) for d in (od if layout == 0 else dims)]):
                if layout == 0:          # gather: out[p] += x[p * s - 1 + k] * w[co, ci, k]
                    q = tuple(pi * s - 1 + ki for pi, ki in zip(p, k))
                    if all(0 <= qi < d for qi, d in zip(q, dims)):
                        out[(b, co) + p] += x[(b, ci) + q] * w[(co, ci) + k]
                else:                    # scatter: out[p * s - 1 + k] += x[p] * w[ci, co, k]
                    q = tuple(pi * s - 1 + ki for pi, ki in zip(p, k))
                    if all(0 <= qi < d for qi, d in zip(q, od)):
                        out[(b, co) + q] += x[(b, ci) + p] * w[(ci, co) + k]
    return out
