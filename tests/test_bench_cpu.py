"""bench.py --dump-outputs: the written sample is fixed, float32, and bounded (host side; the sampling runs on any device)."""
import os

import numpy as np
import torch


def test_dump_outputs_fixed_bounded_sample(tmp_path):
    import bench
    out = torch.randn((1, 4, 3, 20, 70), generator=torch.Generator().manual_seed(1))
    bench.dump_outputs(str(tmp_path / "a"), out)
    bench.dump_outputs(str(tmp_path / "b"), out)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["volume_corner.npy", "volume_sample.npy"]
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.array_equal(a, b)
    r, c = bench.DUMP_CORNER
    assert np.array_equal(np.load(tmp_path / "a" / "volume_corner.npy"), out[0, :, :, :r, :c].numpy())
    sample = np.load(tmp_path / "a" / "volume_sample.npy")
    assert sample.shape == (out.numel(),) and np.isin(sample, out.numpy()).all()
    # the headline volume's dump stays within 64 MB
    V, C, D, H, W = bench.WORKLOADS["cfg2_rpc_3view_768x384x64_c32"]
    assert 4 * (bench.DUMP_SAMPLE + C * D * r * c) <= 64 << 20
