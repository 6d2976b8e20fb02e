"""CPU: bench.py --dump-outputs -- what dump_outputs writes for a workload's captured outputs: one <name>.npy per array,
float32 / float64 only, larger arrays as a fixed seeded sample, the same files from run to run, 64 MB at most."""
import os
import types

import numpy as np
import torch


def _workload():
    g = torch.Generator().manual_seed(0)
    capture = {"msda_fwd_enc_bs1_Lq10": torch.rand(1, 10, 256, generator=g),
               "msda_bwd_enc_bs1_Lq10_grad_value": torch.rand(3_000_000, generator=g),
               "hungarian_0_gt_inds": torch.randint(-1, 9, (7, 900), generator=g),
               "pseudo_counts": torch.tensor([3, 0, 5])}
    return types.SimpleNamespace(capture=capture, teacher=[torch.rand(100, generator=g), torch.rand(700_000, generator=g)])


def test_dump_outputs_files_types_sampling(tmp_path):
    import bench
    wl = _workload()
    n, total = bench.dump_outputs(wl, str(tmp_path / "a"))
    bench.dump_outputs(wl, str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert n == 5 and names == sorted(k + ".npy" for k in list(wl.capture) + ["ema_teacher"])
    assert total <= 64 << 20
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(a, b)
    small = np.load(tmp_path / "a" / "msda_fwd_enc_bs1_Lq10.npy")
    assert small.shape == (1, 10, 256) and small.dtype == np.float32
    np.testing.assert_array_equal(small, wl.capture["msda_fwd_enc_bs1_Lq10"].numpy())
    ints = np.load(tmp_path / "a" / "hungarian_0_gt_inds.npy")
    assert ints.dtype == np.float64 and np.array_equal(ints, wl.capture["hungarian_0_gt_inds"].numpy())
    big = np.load(tmp_path / "a" / "msda_bwd_enc_bs1_Lq10_grad_value.npy")
    assert big.shape == (bench.DUMP_SAMPLE,)
    assert np.isin(big, wl.capture["msda_bwd_enc_bs1_Lq10_grad_value"].numpy()).all()      # a sample, not a recomputation
    teacher = np.load(tmp_path / "a" / "ema_teacher.npy")
    assert teacher.shape == (bench.DUMP_SAMPLE,)
