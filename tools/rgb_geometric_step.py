"""ms per PoseNetRGBGeometric training step at bs32, fp32 and bf16, two ways in one process:

  (a) autograd: models.PoseNetRGBGeometric in train mode + models.pose_loss.PoseLoss(1, 10,
      'geodesic') + backward() + clip_grad_norm_(1.0) + torch.optim.AdamW(lr=1e-4,
      weight_decay=1e-4) -- the reference's loop body (train_rgb_geometric.py:97-110) on the
      drop-in module;
  (b) pose6d.train.RGBGeometricTrainer, hipGraph replay.

Both are warmed up, then timed in alternating blocks (a, b, a, b, ...) of --block steps each,
every block between two device events and ended by a synchronise; the record holds the
per-step time of every block, and per path the median and the spread (min, 10th / 90th
percentile, max) over the blocks.  Needs the GPU: there is no CPU fallback.  Writes one JSON
file (default profiles/rgb_geometric_step.json) and prints it."""
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
    from models.pose_net_rgb_geometric import PoseNetRGBGeometric
    torch.manual_seed(0)
    model = PoseNetRGBGeometric(pretrained=False).to(dev).set_compute_dtype(dtype).train()
    crit = PoseLoss(1.0, 10.0, "geodesic")
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
    rgb, bbox, K, gt_rot, gt_trans = data

    def step():
        opt.zero_grad()
        rot, trans = model(rgb, bbox, K)
        loss = crit(rot, trans, gt_rot, gt_trans)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
    return step


def _graph_path(dtype, data, dev):
    from models.pose_net_rgb_geometric import PoseNetRGBGeometric
    from pose6d.train import RGBGeometricTrainer
    torch.manual_seed(0)
    tr = RGBGeometricTrainer(PoseNetRGBGeometric(pretrained=False).to(dev), B, dtype=dtype, lr=1e-4,
                             weight_decay=1e-4)
    tr.capture(data)
    return tr.step


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


def measure(dtype, dev, blocks, block, warmup):
    from bench import synth_batch
    d = synth_batch(B, dev, seed=1000)
    data = (d[0], d[2], d[3], d[4], d[5])                      # rgb, bbox_center, K, gt_rot, gt_trans
    paths = {"autograd": _autograd_path(dtype, data, dev), "graph": _graph_path(dtype, data, dev)}
    for step in paths.values():
        for _ in range(warmup):
            step()
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(blocks):
        for k, step in paths.items():
            ms[k].append(_block_ms(step, block))
    out = {k: _summary(v) for k, v in ms.items()}
    a, g = out["autograd"], out["graph"]
    out["graph_faster_beyond_spread"] = g["max_ms"] < a["min_ms"]
    out["autograd_over_graph_median"] = round(a["median_ms"] / g["median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=8, help="timed blocks per path (alternating)")
    ap.add_argument("--block", type=int, default=50, help="steps per block (at least 50)")
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps per path")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rgb_geometric_step.json"))
    a = ap.parse_args()
    if a.block < 50 or a.blocks < 2:
        ap.error("time at least two blocks of at least 50 steps per path (--blocks, --block)")
    if not torch.cuda.is_available():
        sys.exit("tools/rgb_geometric_step.py needs the MI355X: no GPU found, and there is no CPU fallback")
    warnings.simplefilter("ignore")
    dev = torch.device("cuda", 0)
    res = {"workload": "PoseNetRGBGeometric training step, batch 32, 224x224", "device": torch.cuda.get_device_name(0),
           "steps_per_path": a.blocks * a.block, "block_steps": a.block, "warmup_steps": a.warmup,
           "paths": {"autograd": "models.PoseNetRGBGeometric + PoseLoss(1, 10, geodesic) + backward + clip_grad_norm_(1.0) + "
                                 "torch.optim.AdamW(lr=1e-4, weight_decay=1e-4)",
                     "graph": "pose6d.train.RGBGeometricTrainer, hipGraph replay"}}
    for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        res[name] = measure(dtype, dev, a.blocks, a.block, a.warmup)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
