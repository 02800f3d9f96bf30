"""DSM clean-up, the parts that run without a GPU: known answers of the numpy oracle (tests/dsm_post_oracle.py), its agreement
with an independent per-cell formulation, and the argument checks of smvs_dsm_despike / smvs_dsm_fill (rejected before any
HIP call) and of dsm.despike / dsm.fill_voids (before any device work)."""
import ctypes as C

import numpy as np
import pytest

import dsm_post_oracle as po
from dsm_testkit import lib  # noqa: F401  (fixtures)

ND = np.float32(-999.0)


def _plane(gh, gw):
    rows, cols = np.mgrid[0:gh, 0:gw]
    return (100.0 + 0.5 * cols - 0.25 * rows).astype(np.float32)          # exact in float32


# ---- fill: known answers -------------------------------------------------------------------------------------------------------
def test_symmetric_holes_in_a_plane_take_the_planes_value():
    z = _plane(21, 23)
    one = z.copy()
    one[10, 11] = ND
    out, hits = po.fill(one, max_steps=4)
    assert hits[10, 11] == 8 and po.same_bits(out, z)
    three = z.copy()
    three[9:12, 10:13] = np.nan
    out, hits = po.fill(three, max_steps=4)
    assert hits[10, 11] == 8 and out[10, 11] == z[10, 11]                 # the centre's hits are symmetric: k = 2 everywhere
    assert po.valid(out, ND).all()
    assert (hits[three == three] == 255).all()


def test_constant_dsm_with_a_slot_is_filled_with_the_constant():
    z = np.full((30, 40), 123.25, np.float32)
    slot = z.copy()
    slot[10:14] = ND                                                       # four whole rows: no E / W hit
    for method in po.METHODS:
        out, hits = po.fill(slot, max_steps=8, method=method)
        assert po.same_bits(out, z), method
        assert hits[10:14].max() <= 6 and hits[10:14].min() >= 3          # rows next to a corner lose diagonals to the border


def test_deep_void_interior_stays_void():
    z = _plane(60, 64)
    z[10:50, 12:52] = ND
    out, hits = po.fill(z, max_steps=6, min_hits=1)
    inner = (slice(16, 44), slice(18, 46))                                 # more than 6 cells from every edge of the void
    assert (hits[inner] == 0).all() and (out[inner] == ND).all()
    assert (hits[10:50, 12:52][0] >= 3).all() and po.valid(out[10], ND).all()
    # min_hits decides: the void's corner cell sees N, NW, W at k = 1 and NE, SW further away
    assert hits[10, 12] == 5
    assert po.fill(z, max_steps=6, min_hits=6)[0][10, 12] == ND


def test_nearest_tie_goes_to_the_earlier_direction():
    z = np.full((5, 5), ND, np.float32)
    z[2, 4], z[2, 0], z[0, 2], z[4, 2] = 10.0, 20.0, 30.0, 40.0            # E, W, N, S at k = 2; no diagonal
    out, hits = po.fill(z, max_steps=4, min_hits=1, method="nearest")
    assert hits[2, 2] == 4 and out[2, 2] == 10.0                           # E comes first
    z[1, 3] = 50.0                                                         # NE at k = 1: d2 = 2 < 4
    assert po.fill(z, max_steps=4, min_hits=1, method="nearest")[0][2, 2] == 50.0
    z[2, 3] = 60.0                                                         # E at k = 1: d2 = 1, and it hides (2, 4)
    assert po.fill(z, max_steps=4, min_hits=1, method="nearest")[0][2, 2] == 60.0


def test_min_picks_the_lowest_hit_and_idw_weights_by_distance():
    z = np.full((7, 7), ND, np.float32)
    z[3, 4], z[3, 0], z[0, 3] = 12.0, 6.0, 9.0                             # E k=1, W k=3, N k=3
    out, hits = po.fill(z, max_steps=3, min_hits=3, method="min")
    assert hits[3, 3] == 3 and out[3, 3] == 6.0
    idw = po.fill(z, max_steps=3, min_hits=3, method="idw")[0][3, 3]
    num = 0.0 + 1.0 * 12.0 + (1.0 / 9.0) * 9.0 + (1.0 / 9.0) * 6.0         # E, then N, then W
    den = 0.0 + 1.0 + 1.0 / 9.0 + 1.0 / 9.0
    assert idw == np.float32(num / den)
    assert po.fill(z, max_steps=2, min_hits=1, method="idw")[0][3, 3] == 12.0      # W and N out of reach
    assert po.fill(z, max_steps=3, min_hits=4)[1][3, 3] == 3 and po.fill(z, max_steps=3, min_hits=4)[0][3, 3] == ND


def test_fill_reads_the_input_only_and_copies_everything_else():
    z = po.scene(40, 37, seed=2)
    out, hits = po.fill(z, max_steps=1, min_hits=8)
    ok = po.valid(z, ND)
    assert np.array_equal(out.view(np.uint32)[ok], z.view(np.uint32)[ok]) and (hits[ok] == 255).all()
    stay = ~ok & (hits < 8)
    assert stay.any() and np.array_equal(out.view(np.uint32)[stay], z.view(np.uint32)[stay])      # NaN stays NaN, nodata nodata
    assert (hits == 8).any() and po.valid(out[~ok & (hits == 8)], ND).all()


# ---- despike: known answers ----------------------------------------------------------------------------------------------------
def test_spike_is_removed_and_its_neighbours_are_not():
    z = _plane(20, 20)
    z[8, 9] += 50.0
    z[15, 3] -= 50.0
    for radius in (1, 2, 3):
        out, removed = po.despike(z, radius=radius, thresh=10.0, min_valid=3)
        assert removed.sum() == 2 and removed[8, 9] == 1 and removed[15, 3] == 1
        assert out[8, 9] == ND and out[15, 3] == ND
        keep = removed == 0
        assert np.array_equal(out.view(np.uint32)[keep], z.view(np.uint32)[keep])


def test_isolated_cell_is_removed_by_min_valid():
    z = np.full((15, 15), np.nan, np.float32)
    z[7, 7] = 100.0
    z[2, 2:4] = 100.0                                                      # a pair: n = 2
    z[11:13, 11:13] = 100.0                                                # a square: n = 4
    out, removed = po.despike(z, radius=2, thresh=10.0, min_valid=3)
    assert removed[7, 7] == 1 and removed[2, 2:4].all() and not removed[11:13, 11:13].any()
    assert removed.sum() == 3 and np.isnan(out[0, 0]) and out[7, 7] == ND
    assert po.despike(z, radius=2, thresh=10.0, min_valid=1)[1].sum() == 0


def test_even_median_rule_on_a_border_window():
    z = np.array([[1.0, 2.0, 100.0], [4.0, 8.0, 100.0], [100.0, 100.0, 100.0]], np.float32)
    # the corner cell (0, 0), radius 1: window {1, 2, 4, 8}, n = 4, m = 0.5 (2 + 4) = 3; |1 - 3| = 2
    assert po.despike(z, radius=1, thresh=2.0, min_valid=1)[1][0, 0] == 0           # not above thresh
    assert po.despike(z, radius=1, thresh=1.9999, min_valid=1)[1][0, 0] == 1
    # the rounding of the even median: float32(0.5 (a + b)) in float64
    a, b = np.float32(1.0), np.float32(1.0) + np.float32(2.0 ** -23)
    w = np.array([[a, b]], np.float32)
    m = np.float32(0.5 * (float(a) + float(b)))                            # rounds to even: 1.0
    assert m == a
    assert po.despike(w, radius=1, thresh=0.0, min_valid=1)[1].tolist() == [[0, 1]]
    # thresh = 0 keeps exactly the cells equal to their median
    flat = np.full((6, 6), 5.0, np.float32)
    assert po.despike(flat, thresh=0.0)[1].sum() == 0


# ---- the vectorised oracle against the per-cell formulation ---------------------------------------------------------------
@pytest.mark.parametrize("shape,seed", [((40, 37), 0), ((1, 1), 1), ((1, 29), 2), ((31, 2), 3), ((23, 40), 4)])
def test_oracle_equals_the_per_cell_formulation(shape, seed):
    z = po.scene(*shape, seed=seed, voids=0.25, salt=0.05)
    for radius in (1, 2, 3):
        for thresh, min_valid in ((10.0, 3), (0.0, 1), (4.0, (2 * radius + 1) ** 2)):
            a, ra = po.despike(z, radius=radius, thresh=thresh, min_valid=min_valid, band=16)
            b, rb = po.despike_brute(z, radius=radius, thresh=thresh, min_valid=min_valid)
            assert po.same_bits(a, b) and np.array_equal(ra, rb), (radius, thresh, min_valid)
    for method in po.METHODS:
        for max_steps, min_hits in ((1, 1), (3, 3), (7, 8), (64, 2)):
            a, ha = po.fill(z, max_steps=max_steps, min_hits=min_hits, method=method)
            b, hb = po.fill_brute(z, max_steps=max_steps, min_hits=min_hits, method=method)
            assert po.same_bits(a, b) and np.array_equal(ha, hb), (method, max_steps, min_hits)


def test_crop_property_of_the_oracle():
    z = po.scene(70, 90, seed=5, voids=0.3)
    ms, R = 6, 3
    r0, r1, c0, c1 = 20, 45, 30, 70
    whole, hw = po.fill(z, max_steps=ms)
    crop, hc = po.fill(z[r0 - ms:r1 + ms, c0 - ms:c1 + ms], max_steps=ms)
    assert po.same_bits(crop[ms:-ms, ms:-ms], whole[r0:r1, c0:c1]) and np.array_equal(hc[ms:-ms, ms:-ms], hw[r0:r1, c0:c1])
    whole, rw = po.despike(z, radius=R)
    crop, rc = po.despike(z[r0 - R:r1 + R, c0 - R:c1 + R], radius=R)
    assert po.same_bits(crop[R:-R, R:-R], whole[r0:r1, c0:c1]) and np.array_equal(rc[R:-R, R:-R], rw[r0:r1, c0:c1])


# ---- argument checks -----------------------------------------------------------------------------------------------------------
def test_despike_entry_rejects_bad_arguments_without_a_gpu(lib):
    from satmvs_amd import _lib
    a, b, m = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20)

    def call(dsm=a, gw=8, gh=8, radius=2, thresh=10.0, min_valid=3, out=b, removed=m):
        _lib.call("smvs_dsm_despike", dsm, gw, gh, -999.0, radius, thresh, min_valid, out, removed, None)

    for kw in ({"dsm": None}, {"out": None}):
        with pytest.raises(_lib.SatMVSNativeError, match="null pointer"):
            call(**kw)
    with pytest.raises(_lib.SatMVSNativeError, match="non-positive grid"):
        call(gw=0)
    with pytest.raises(_lib.SatMVSNativeError, match="grid too large"):
        call(gw=65536, gh=32768)
    for r in (0, 4, -1):
        with pytest.raises(_lib.SatMVSNativeError, match="radius must be"):
            call(radius=r)
    for t in (-0.5, np.nan, np.inf):
        with pytest.raises(_lib.SatMVSNativeError, match="thresh must be"):
            call(thresh=t)
    for r, mv in ((1, 0), (1, 10), (2, 26), (3, 50), (3, -1)):
        with pytest.raises(_lib.SatMVSNativeError, match="min_valid must be"):
            call(radius=r, min_valid=mv)
    with pytest.raises(_lib.SatMVSNativeError, match="out aliases dsm"):
        call(out=a)
    with pytest.raises(_lib.SatMVSNativeError, match="out aliases dsm"):
        call(out=C.c_void_p((1 << 20) + 8 * 8 * 4 - 4))                    # the last cell of dsm
    with pytest.raises(_lib.SatMVSNativeError, match="removed aliases"):
        call(removed=C.c_void_p((2 << 20) + 16))


def test_fill_entry_rejects_bad_arguments_without_a_gpu(lib):
    from satmvs_amd import _lib
    a, b, m, w = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20), C.c_void_p(4 << 20)
    need = lib.smvs_dsm_fill_workspace_bytes(8, 8, 32)
    assert need >= 6 * 8 * 8 * 2
    assert lib.smvs_dsm_fill_workspace_bytes(0, 8, 32) == 0 and lib.smvs_dsm_fill_workspace_bytes(65536, 32768, 32) == 0
    assert lib.smvs_dsm_fill_workspace_bytes(8, 8, 0) == 0 and lib.smvs_dsm_fill_workspace_bytes(8, 8, 4097) == 0
    assert lib.smvs_dsm_fill_workspace_bytes(8, 8, 4096) > 0

    def call(dsm=a, gw=8, gh=8, max_steps=32, min_hits=3, method=0, out=b, hits=m, ws=w, nbytes=need):
        _lib.call("smvs_dsm_fill", dsm, gw, gh, -999.0, max_steps, min_hits, method, out, hits, ws, nbytes, None)

    for kw in ({"dsm": None}, {"out": None}, {"ws": None}):
        with pytest.raises(_lib.SatMVSNativeError, match="null pointer"):
            call(**kw)
    with pytest.raises(_lib.SatMVSNativeError, match="non-positive grid"):
        call(gh=-3)
    with pytest.raises(_lib.SatMVSNativeError, match="grid too large"):
        call(gw=46341, gh=46341)
    for s in (0, 4097, -1):
        with pytest.raises(_lib.SatMVSNativeError, match="max_steps must be"):
            call(max_steps=s)
    for h in (0, 9):
        with pytest.raises(_lib.SatMVSNativeError, match="min_hits must be"):
            call(min_hits=h)
    for mth in (-1, 3):
        with pytest.raises(_lib.SatMVSNativeError, match="method must be"):
            call(method=mth)
    with pytest.raises(_lib.SatMVSNativeError, match="out aliases dsm"):
        call(out=a)
    with pytest.raises(_lib.SatMVSNativeError, match="hits aliases"):
        call(hits=a)
    with pytest.raises(_lib.SatMVSNativeError, match="workspace too small"):
        call(nbytes=need - 1)
    with pytest.raises(_lib.SatMVSNativeError, match="workspace aliases"):
        call(ws=b)


def test_python_entries_validate_before_the_gpu():
    import torch
    from satmvs_amd import dsm
    z = np.zeros((4, 6), np.float32)
    spike_cases = [
        (dict(dsm=np.zeros((2, 4, 6), np.float32)), r"\(gh, gw\)"),
        (dict(dsm=np.zeros(6, np.float32)), r"\(gh, gw\)"),
        (dict(dsm=np.zeros((0, 6), np.float32)), "positive sizes"),
        (dict(dsm=z.astype(np.float64)), "float32"),
        (dict(dsm=torch.zeros((4, 6), dtype=torch.float16)), "float32"),
        (dict(dsm=z.astype(np.int32)), "float32"),
        (dict(radius=0), "radius"), (dict(radius=4), "radius"), (dict(radius=2.0), "radius"), (dict(radius=True), "radius"),
        (dict(thresh=-1.0), "thresh"), (dict(thresh=float("nan")), "thresh"), (dict(thresh=float("inf")), "thresh"),
        (dict(min_valid=0), "min_valid"), (dict(min_valid=26), "min_valid"), (dict(radius=1, min_valid=10), "min_valid"),
    ]
    for kw, msg in spike_cases:
        args = dict(dsm=z)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            dsm.despike(**args)
    fill_cases = [
        (dict(dsm=np.zeros((2, 4, 6), np.float32)), r"\(gh, gw\)"),
        (dict(dsm=z.astype(np.float64)), "float32"),
        (dict(dsm=torch.zeros((4, 6), dtype=torch.float64)), "float32"),
        (dict(method="linear"), "method must be"), (dict(method=0), "method must be"),
        (dict(max_steps=0), "max_steps"), (dict(max_steps=4097), "max_steps"), (dict(max_steps=8.0), "max_steps"),
        (dict(min_hits=0), "min_hits"), (dict(min_hits=9), "min_hits"),
    ]
    for kw, msg in fill_cases:
        args = dict(dsm=z)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            dsm.fill_voids(**args)
