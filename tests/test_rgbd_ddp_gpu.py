"""RGBDTrainer's bucketed data-parallel step on the GPU box (the heads, the fusion core and two
ResNet50 backwards feed one bucket plan): 2 ranks on one MI355X over gloo
(tests/rgbd_ddp_worker.py), each on its own batch of 2, against the 1-process update from the
averaged gradients -- eager and graph-segmented replay.  The one case: it builds five trainers
per rank and most of its time is process start-up."""
import os
import subprocess
import sys
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESNET50_RUNNING = 2 * 26560   # running_mean + running_var over the 53 BatchNorms of one ResNet50


def _report(r):
    err = r.stderr.splitlines()
    flagged = [ln for ln in err if any(k in ln for k in ("Error", "error", "Watchdog", "watchdog", "abort", "Abort"))]
    return ("--- stderr head ---\n" + "\n".join(err[:60]) + "\n--- error lines ---\n" + "\n".join(flagged[:80])
            + "\n--- stdout tail ---\n" + r.stdout[-3000:] + "\n--- stderr tail ---\n" + r.stderr[-3000:])


@pytest.mark.gpu
def test_rgbd_ddp_bucketed_step_matches_mean_gradient_update():
    world, batch, bucket_mb = 2, 2, 8.0
    out = os.path.join(tempfile.mkdtemp(), "rgbd_ddp")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", "29751",
           os.path.join(REPO, "tests", "rgbd_ddp_worker.py"), out, str(batch), str(bucket_mb)]
    r = subprocess.run(cmd, env=env, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, _report(r)
    for rank in range(world):
        f = open(f"{out}.{rank}").read().split()
        (same, diff, graph_same, run_eager, drun_eager, run_graph, drun_graph, agree, nb, nsegs, distinct, n_rgb,
         n_depth) = f
        assert int(distinct) == 1, "the two ranks' batches must give different gradients"
        assert int(nb) > 3 and int(nsegs) > 1, "expected several buckets and graph segments"
        assert same == "1", f"rank {rank}: DDP step != AdamW on the mean gradient (max |diff| {diff})"
        assert graph_same == "1", f"rank {rank}: graph-segmented DDP step != eager DDP step"
        assert int(n_rgb) == int(n_depth) == RESNET50_RUNNING, "a trunk's running statistics were not compared"
        assert run_eager == "1" and run_graph == "1", f"rank {rank}: local BN running stats differ (rgb trunk)"
        assert drun_eager == "1" and drun_graph == "1", f"rank {rank}: local BN running stats differ (depth trunk)"
        assert agree == "1", "ranks hold different parameters"
