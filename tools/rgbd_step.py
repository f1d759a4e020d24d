"""ms per PoseNetRGBD training step at bs32, fp32 and bf16, three ways in one process:

  (a) autograd: models.PoseNetRGBD in train mode + models.pose_loss.PoseLoss(1, 10, 'geodesic')
      + backward() + clip_grad_norm_(1.0) + torch.optim.AdamW(lr=1e-4, weight_decay=1e-4) -- the
      reference's loop body (train_rgbd.py:97-110) on the drop-in module;
  (b) pose6d.train.RGBDTrainer, hipGraph replay (fused_fusion=True: paired LayerNorm, stacked
      K|V projection);
  (c) pose6d.train.RGBDTrainer(fused_fusion=False), hipGraph replay: the same step with the
      fusion core's 7-forward / 14-backward launch chain that (a) runs.

All are warmed up, then timed in alternating blocks (a, b, c, a, b, c, ...) of --block steps
each, every block between two device events and ended by a synchronise; the record holds the
per-step time of every block, and per path the median and the spread (min, 10th / 90th
percentile, max) over the blocks.  Then, per dtype and for (b) and (c), pose6d.steptime times
every launch inside the captured step: the record holds the node count and in-step time of the
fusion core's launches (FusionEngine.forward + backward) and, for (b), the step by kernel
symbol.  Needs the GPU: there is no CPU fallback.  Writes one JSON file (default
profiles/rgbd_step.json) and prints it."""
import argparse
import json
import os
import statistics
import sys
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "6d-pose-estimation_amd")]

import torch  # noqa: E402

B = 32


def _autograd_path(dtype, data, dev):
    from models.pose_loss import PoseLoss
    from models.pose_net_rgbd import PoseNetRGBD
    torch.manual_seed(0)
    model = PoseNetRGBD(pretrained=False).to(dev).set_compute_dtype(dtype).train()
    crit = PoseLoss(1.0, 10.0, "geodesic")
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
    rgb, depth, gt_rot, gt_trans = data

    def step():
        opt.zero_grad()
        rot, trans = model(rgb, depth)
        loss = crit(rot, trans, gt_rot, gt_trans)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
    return step


def _trainer(dtype, dev, fused):
    from models.pose_net_rgbd import PoseNetRGBD
    from pose6d.train import RGBDTrainer
    torch.manual_seed(0)
    return RGBDTrainer(PoseNetRGBD(pretrained=False).to(dev), B, dtype=dtype, lr=1e-4, weight_decay=1e-4,
                       fused_fusion=fused)


def _block_ms(step, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def _summary(ms):
    q = statistics.quantiles(ms, n=10)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "p10_ms": round(q[0], 4),
            "p90_ms": round(q[-1], 4), "max_ms": round(max(ms), 4), "blocks_ms": [round(v, 4) for v in ms]}


def _in_step(tr, data, dev, plain_ms, symbols):
    """pose6d.steptime over the trainer's step_body: the fusion core's nodes (between the node
    counts before and after FusionEngine.forward / backward) and the step by kernel symbol."""
    from pose6d import steptime
    spans = []
    fwd, bwd = tr.fusion.forward, tr.fusion.backward

    def spy(fn):
        def run(*a, **k):
            log = steptime._CallLog(torch.cuda.current_stream().cuda_stream)
            n0 = log.node_count()
            out = fn(*a, **k)
            if n0 is not None:                                  # (None: the warm-up run, no capture)
                spans.append((n0, log.node_count()))
            return out
        return run

    tr.fusion.forward, tr.fusion.backward = spy(fwd), spy(bwd)
    try:
        timer = steptime.StepTimer(lambda: tr.step_body(data), dev)
    finally:
        tr.fusion.forward, tr.fusion.backward = fwd, bwd
    recs = timer.run(reps=20, plain_ms=plain_ms)
    timer.close()
    core = [r for r in recs if any(lo <= r["node"] < hi for lo, hi in spans)]
    (f0, f1), (b0, b1) = spans
    out = {"step_nodes": len(recs), "step_in_graph_ms": round(sum(r["us"] for r in recs) / 1e3, 4),
           "event_overhead_us_per_node": round(timer.overhead_us, 3),
           "fusion_core_nodes": len(core), "fusion_core_nodes_forward": f1 - f0, "fusion_core_nodes_backward": b1 - b0,
           "fusion_core_us": round(sum(r["us"] for r in core), 2),
           "fusion_core_kernels": [[r["call"], r["kernel"], round(r["us"], 2)] for r in core]}
    if symbols:
        total = sum(r["us"] for r in recs)
        out["by_symbol"] = [{"kernel": k, "launches": v["launches"], "us": round(v["time_us"], 1),
                             "share": round(v["time_us"] / total, 4)}
                            for k, v in list(steptime.by_symbol(recs).items())[:16]]
    return out


def measure(dtype, dev, blocks, block, warmup):
    from bench import synth_batch
    d = synth_batch(B, dev, seed=1000)
    data = (d[0], d[1].unsqueeze(1), d[4], d[5])               # rgb, depth (B, 1, H, W), gt_rot, gt_trans
    trainers = {"graph": _trainer(dtype, dev, True), "graph_unfused": _trainer(dtype, dev, False)}
    for tr in trainers.values():
        tr.capture(data)
    paths = {"autograd": _autograd_path(dtype, data, dev), **{k: tr.step for k, tr in trainers.items()}}
    for step in paths.values():
        for _ in range(warmup):
            step()
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(blocks):
        for k, step in paths.items():
            ms[k].append(_block_ms(step, block))
    out = {k: _summary(v) for k, v in ms.items()}
    a, g, u = out["autograd"], out["graph"], out["graph_unfused"]
    out["graph_faster_beyond_spread"] = g["max_ms"] < a["min_ms"]
    out["autograd_over_graph_median"] = round(a["median_ms"] / g["median_ms"], 3)
    # the fused fusion chain against the unfused one: a gain only if the medians differ by more
    # than the blocks of either path scatter
    out["fused_minus_unfused_median_ms"] = round(g["median_ms"] - u["median_ms"], 4)
    out["fused_faster_beyond_spread"] = g["max_ms"] < u["min_ms"]
    out["fused_median_below_unfused_beyond_spread"] = (
        u["median_ms"] - g["median_ms"] > max(g["max_ms"] - g["min_ms"], u["max_ms"] - u["min_ms"]))
    out["in_step"] = {k: _in_step(tr, data, dev, out[k]["median_ms"], symbols=(k == "graph"))
                      for k, tr in trainers.items()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=8, help="timed blocks per path (alternating)")
    ap.add_argument("--block", type=int, default=50, help="steps per block (at least 50)")
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps per path")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rgbd_step.json"))
    a = ap.parse_args()
    if a.block < 50 or a.blocks < 2:
        ap.error("time at least two blocks of at least 50 steps per path (--blocks, --block)")
    if not torch.cuda.is_available():
        sys.exit("tools/rgbd_step.py needs the MI355X: no GPU found, and there is no CPU fallback")
    warnings.simplefilter("ignore")
    dev = torch.device("cuda", 0)
    res = {"workload": "PoseNetRGBD training step, batch 32, 224x224", "device": torch.cuda.get_device_name(0),
           "steps_per_path": a.blocks * a.block, "block_steps": a.block, "warmup_steps": a.warmup,
           "paths": {"autograd": "models.PoseNetRGBD + PoseLoss(1, 10, geodesic) + backward + clip_grad_norm_(1.0) + "
                                 "torch.optim.AdamW(lr=1e-4, weight_decay=1e-4)",
                     "graph": "pose6d.train.RGBDTrainer (fused_fusion=True), hipGraph replay",
                     "graph_unfused": "pose6d.train.RGBDTrainer(fused_fusion=False), hipGraph replay"}}
    for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        res[name] = measure(dtype, dev, a.blocks, a.block, a.warmup)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
