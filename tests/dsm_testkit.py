"""What the DSM test files (test_dsm_*, test_ortho_*) and their numpy oracles share: the fixtures, the comparisons, the
order-preserving keys and the synthetic scene.  A plain module: the test files import the fixtures by name.  Nothing here
imports satmvs_amd or torch at import time (the fixtures do when they run), so the numpy-only oracles can import it."""
import numpy as np
import pytest


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the GPU suite needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def proj():
    from satmvs_amd.transverse_mercator import whu_tlc_projection
    return whu_tlc_projection()


@pytest.fixture(scope="module")
def tm7():
    from satmvs_amd.transverse_mercator import whu_tlc_projection
    return whu_tlc_projection().tm7()


@pytest.fixture(scope="module")
def lib():
    from satmvs_amd import _lib, build
    build.build()
    return _lib.load()


def views_fixture(H, W, seed, shifts=(0.0, 0.4, -0.4)):
    """`views = views_fixture(H, W, seed)` in a test file: {shift: rpc} of synthetic H x W views."""
    @pytest.fixture(scope="module")
    def views():
        import dsm_render_oracle as ro
        return {s: ro.view_rpc(H, W, s, seed=seed) for s in shifts}
    return views


def tilted_fixture(H, W, seed, shift=0.4):
    """`tilted = tilted_fixture(H, W, seed)` in a test file: one view about 22 degrees off nadir."""
    @pytest.fixture(scope="module")
    def tilted():
        import dsm_render_oracle as ro
        return ro.view_rpc(H, W, shift, seed=seed)
    return tilted


# ---- validity, bits and keys ---------------------------------------------------------------------------------------------------
def valid(z, nodata):
    z = np.asarray(z, np.float32)
    return np.isfinite(z) & (z != np.float32(nodata))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def f2key(z):
    """The order-preserving uint32 image of float32 values (-0.0 below +0.0)."""
    u = np.ascontiguousarray(z, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key2f(k):
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(np.float32)


def same(got, want, what):
    """Equal bits (so equal NaN positions and payloads) for float32 grids, equal values for uint8 maps."""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.dtype == np.float32:
        g, w = got.view(np.uint32), want.view(np.uint32)
        assert np.array_equal(np.isnan(got), np.isnan(want)), what
    else:
        g, w = got, want
    assert np.array_equal(g, w), (what, int((g != w).sum()), np.argwhere(g != w)[:5].tolist())


# ---- the scene -----------------------------------------------------------------------------------------------------------------
def scene(E, N, blocks=True, holes=True, seed=None, voids=0.0, salt=0.0, base=130.0, amp=20.0):
    """Terrain base + amp sin(E / 53) cos(N / 71) over the cell centres (E, N) [m]; with `blocks` two blocks (+40 m, +25 m) about
    the centre; with `holes` a NaN hole and a nodata (-999) hole beside the first block; with a `seed`, salt noise of both signs
    (30 - 80 m) on a share `salt` of the cells and random voids (NaN and nodata mixed) on a share `voids`.  -> (gh, gw) float32."""
    gh, gw = E.shape
    rng = None if seed is None else np.random.default_rng(seed)
    z = (base + amp * np.sin(E / 53.0) * np.cos(N / 71.0)).astype(np.float32)
    r0, c0 = gh // 2 - 3, gw // 2 - 3
    if blocks:
        z[max(r0, 0):r0 + 6, max(c0, 0):c0 + 6] += 40.0
        z[max(r0 - 12, 0):max(r0 - 8, 0), c0 + 10:c0 + 14] += 25.0
    if rng is not None:
        spikes = rng.random((gh, gw)) < salt
        z[spikes] += (rng.uniform(30.0, 80.0, (gh, gw)) * rng.choice([-1.0, 1.0], (gh, gw)))[spikes].astype(np.float32)
    if holes:
        z[max(r0, 0):r0 + 3, c0 + 6:c0 + 8] = np.nan
        z[r0 + 6:r0 + 8, max(c0, 0):c0 + 4] = -999.0
    if rng is not None:
        gone = rng.random((gh, gw)) < voids
        z[gone] = np.where(rng.random((gh, gw)) < 0.5, np.float32(np.nan), np.float32(-999.0))[gone]
    return z
