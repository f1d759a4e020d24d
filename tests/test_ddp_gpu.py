"""Bucketed data-parallel training step on the GPU box: 2 and 3 ranks on one MI355X
over gloo (tests/ddp_worker.py), each on its own batch, against the 1-process
update from the averaged gradients -- eager and graph-segmented replay (3 ranks:
the non-power-of-two world size averages the gradient in a pass of its own)."""
import os
import subprocess
import sys
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _report(r):
    """A failed subprocess's output for the assertion message: the head of stderr (a
    watchdog or collective error is printed first, then buried under the launcher's
    per-rank tracebacks), every line naming an error, and the tails."""
    err = r.stderr.splitlines()
    flagged = [ln for ln in err if any(k in ln for k in ("Error", "error", "Watchdog", "watchdog", "abort", "Abort"))]
    return ("--- stderr head ---\n" + "\n".join(err[:60]) + "\n--- error lines ---\n" + "\n".join(flagged[:80])
            + "\n--- stdout tail ---\n" + r.stdout[-3000:] + "\n--- stderr tail ---\n" + r.stderr[-3000:])


@pytest.mark.gpu
@pytest.mark.parametrize("world,batch,bucket_mb", [(2, 4, 2.0), (3, 4, 2.0), (2, 32, 25.0)],
                         ids=["w2-b4", "w3-b4", "w2-b32-configs4"])
def test_ddp_bucketed_step_matches_mean_gradient_update(world, batch, bucket_mb):
    """w2-b32-configs4: BASELINE configs[4]'s per-rank workload -- bs32 per rank, bf16,
    the default 25 MB gradient buckets and the segmented graphs bench.py --gpus N builds."""
    out = os.path.join(tempfile.mkdtemp(), "ddp")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(29631 + world + batch),
           os.path.join(REPO, "tests", "ddp_worker.py"), out, str(batch), str(bucket_mb)]
    r = subprocess.run(cmd, env=env, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, _report(r)
    for rank in range(world):
        f = open(f"{out}.{rank}").read().split()
        same, diff, graph_same, run_eager, run_graph, agree, nb, nsegs, distinct = f
        assert int(distinct) == 1, "the two ranks' batches must give different gradients"
        assert int(nb) > 3 and int(nsegs) > 1, "expected several buckets and graph segments"
        assert same == "1", f"rank {rank}: DDP step != AdamW on the mean gradient (max |diff| {diff})"
        assert graph_same == "1", f"rank {rank}: graph-segmented DDP step != eager DDP step"
        assert run_eager == "1" and run_graph == "1", f"rank {rank}: local BN running stats differ"
        assert agree == "1", "ranks hold different parameters"


@pytest.mark.gpu
@pytest.mark.parametrize("profile", [False, True], ids=["plain", "with-roofline"])
def test_bench_world2_json_line(profile):
    """bench.py's N > 1 path end to end (configs[4] per rank: bs32, 25 MB buckets,
    segmented graphs), 2 ranks sharing the box's one GPU over gloo
    (POSE6D_BENCH_SHARE_GPU=1; RCCL needs a GPU per rank): the JSON line reports the
    whole job -- n_gpus 2, global batch 64, value = 64 crops x steps / max-over-ranks time.
    with-roofline: rank 0 also runs the in-step roofline capture after the timed loop
    (the line an 8-GPU run prints), while rank 1 leaves."""
    import json
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", POSE6D_BENCH_SHARE_GPU="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(29671 + int(profile)), os.path.join(REPO, "bench.py"),
           "--gpus", "2", "--steps", "3", "--warmup", "1", "--no-side", "--no-fp32", "--no-cpu-baseline"]
    # the roofline is one of the measurements behind --full; a plain run prints the headline line only
    cmd.append("--full" if profile else "--no-kernel-profile")
    r = subprocess.run(cmd, env=env, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, _report(r)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["config"]["global_batch"] == 64 and res["config"]["per_gpu_batch"] == 32
    assert res["config"]["parallelism"] == "dp2" and res["scaling"] == "weak"
    assert res["value"] > 0 and abs(res["value"] - 64 * 1e3 / res["ms_per_step"]) < 1e-3 * res["value"] + 0.1
    if profile:
        assert res["roofline"].get("kernel", "").startswith("conv_bwd"), res["roofline"]
        assert res["roofline"]["frac"] > 0 and res["breakdown"]["kernels_per_step"] > 100
    else:
        assert "roofline" not in res and "breakdown" not in res


@pytest.mark.gpu
def test_rccl_world1_bucketed_step():
    """The RCCL branch itself (backend 'nccl' with device_id, as bench.py initialises it
    for N > 1): one rank under torch.distributed.run, the trainer forced onto the
    bucketed path (25 MB buckets, comm stream, async all-reduce handles around the
    segmented-graph replay).  A one-rank all-reduce returns its input, so two eager and
    two replayed steps equal the plain one-GPU steps bit for bit.  Then bench.py's
    in-step roofline capture (pose6d.steptime) runs once under the same live group, with
    an all-reduce in flight for the RCCL watchdog to poll.  Scaling over xGMI stays
    unmeasured here (one GPU per box)."""
    out = os.path.join(tempfile.mkdtemp(), "rccl")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
           "--master-addr", "127.0.0.1", "--master-port", "29691", os.path.join(REPO, "tests", "rccl_worker.py"), out]
    r = subprocess.run(cmd, env=env, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, _report(r)
    eager_same, graph_same, nb, nsegs, backend, timed = open(out).read().split()
    assert backend == "nccl"
    # the in-step roofline capture (pose6d.steptime, thread-local capture mode) ran once
    # under the live RCCL group with an all-reduce in flight: its kernel records came back
    assert int(timed) > 100, f"steptime under RCCL recorded {timed} kernels"
    assert int(nb) >= 4 and int(nsegs) >= 3, "expected several 25 MB buckets and graph segments"
    assert eager_same == "1", "eager bucketed RCCL step != plain one-GPU step"
    assert graph_same == "1", "segmented-graph RCCL step != plain one-GPU step"
