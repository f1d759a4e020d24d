"""bench.py's command line: a plain run measures the headline figure only, --full
switches every other measurement on (each --no-* option drops one again), and
--dump-outputs writes what the last step computed as float32 .npy files."""
import os
import warnings

import pytest


def test_plain_run_measures_only_the_headline():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 3)
    assert not a.full and a.dump_outputs is None
    assert a.no_kernel_profile and a.no_fp32 and a.no_side and a.no_cpu_baseline
    # the parts' own switches mean nothing without --full
    a = bench.parse_args(["--no-side"])
    assert a.no_kernel_profile and a.no_fp32 and a.no_side and a.no_cpu_baseline


def test_full_switches_every_part_on_and_no_options_drop_one():
    import bench
    a = bench.parse_args(["--full", "--dump-outputs", "somewhere"])
    assert a.full and a.dump_outputs == "somewhere"
    assert not (a.no_kernel_profile or a.no_fp32 or a.no_side or a.no_cpu_baseline)
    a = bench.parse_args(["--full", "--no-side", "--no-cpu-baseline"])
    assert a.no_side and a.no_cpu_baseline and not a.no_kernel_profile and not a.no_fp32


@pytest.mark.gpu
def test_dump_outputs_writes_the_last_steps_arrays(tmp_path):
    """One eager bf16 step at batch 2, then dump_outputs twice: float32 files of the
    documented names and shapes, under 64 MB in all, holding the trainer's loss /
    predictions, and the same sampled elements in both dumps (fixed seeded indices)."""
    import numpy as np
    import torch
    import bench
    from models.pose_net_rgbd_geometric import PoseNetRGBDGeometric
    from pose6d.train import RGBDGeometricTrainer
    warnings.simplefilter("ignore")
    B = 2
    torch.manual_seed(0)
    dev = torch.device("cuda")
    tr = RGBDGeometricTrainer(PoseNetRGBDGeometric(pretrained=False).to(dev), B, dtype=torch.bfloat16)
    tr.step(bench.synth_batch(B, dev, seed=3))
    torch.cuda.synchronize()
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    for d in dirs:
        bench.dump_outputs(tr, d)
    names = {"loss", "rot", "trans", "grad_norm", "bn_running_stats", "params_sample", "grads_sample"}
    assert {f for f in os.listdir(dirs[0])} == {n + ".npy" for n in names}
    a, b = ({n: np.load(os.path.join(d, n + ".npy")) for n in names} for d in dirs)
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 * 1024 * 1024
    assert a["loss"].shape == (1,) and a["grad_norm"].shape == (1,)
    assert a["rot"].shape == (B, 4) and a["trans"].shape == (B, 3)
    n = min(bench.DUMP_SAMPLE, tr.arena.numel)
    assert a["params_sample"].shape == (n,) and a["grads_sample"].shape == (n,)
    for k in names:
        assert np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k], b[k]), k
    assert a["loss"][0] == tr.loss.item() and a["grad_norm"][0] > 0
    assert np.array_equal(a["rot"], tr.rot.cpu().numpy())
    np.testing.assert_allclose(np.linalg.norm(a["rot"], axis=1), 1.0, rtol=1e-5)
    assert np.abs(a["params_sample"]).max() > 0 and np.abs(a["grads_sample"]).max() > 0
