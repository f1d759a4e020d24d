"""ms per validation batch of PoseNetRGBDGeometric (bs32, bf16, 20 batches of synth_batch
inputs, 13 synthetic meshes of 500 points), two routes alternated in one process and timed
with device events:

  (a) the drop-in route: model.sync_weights() once, then per batch model(...) under no_grad
      plus ADDLoss.eval_metrics (a device-to-host copy per batch), the means on the host;
  (b) pose6d.validate.Validator captured on the trainer's own engines: begin(), 20 x batch(),
      finish() -- its one device-to-host copy -- inside the timed window.

Both routes give the same metrics (asserted).  usage: python tools/val_time.py [--out FILE]
[--rounds N]; writes the figures to FILE (default profiles/val_time.txt) and prints them."""
import argparse
import os
import statistics
import sys
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "6d-pose-estimation_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

B, NBATCH = 32, 20
KEYS = ("add_mean", "add_s_mean", "add_01d_acc")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "val_time.txt"))
    ap.add_argument("--rounds", type=int, default=10)
    args = ap.parse_args()
    from models.add_loss import ADDLoss
    from models.pose_net_rgbd_geometric import PoseNetRGBDGeometric
    from pose6d.train import RGBDGeometricTrainer
    from pose6d.validate import Validator
    from tests.synth import LINEMOD_OBJ_IDS, synthetic_meshes
    warnings.simplefilter("ignore")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = PoseNetRGBDGeometric(pretrained=False).to(dev)
    tr = RGBDGeometricTrainer(model, B, dtype=torch.bfloat16)
    model.set_compute_dtype(torch.bfloat16)
    train_data = bench.synth_batch(B, dev, seed=1)
    tr.capture(train_data)
    tr.step()

    pts, diam = synthetic_meshes(500)
    crit = ADDLoss.__new__(ADDLoss)
    torch.nn.Module.__init__(crit)
    crit.points = {k: torch.from_numpy(v).to(dev) for k, v in pts.items()}
    crit.diameters, crit.device, crit._table = diam, dev, None
    rng = np.random.default_rng(0)
    batches = []
    for k in range(NBATCH):
        ids = torch.from_numpy(rng.choice(LINEMOD_OBJ_IDS, B)).to(dev)
        batches.append((bench.synth_batch(B, dev, seed=100 + k), ids))

    def route_a():
        model.eval()
        model.sync_weights()
        sums = {k: 0.0 for k in KEYS}
        with torch.no_grad():
            for (rgb, depth_raw, bbox, K, gt_rot, gt_trans), ids in batches:
                rot, trans = model(rgb, None, depth_raw, bbox, K)
                m = crit.eval_metrics(rot, trans, gt_rot, gt_trans, ids)
                for k in KEYS:
                    sums[k] += m[k]
        model.train()
        return {k: sums[k] / NBATCH for k in KEYS}

    val = Validator(tr, crit, max_samples=B * NBATCH)
    val.capture(*batches[0])

    def route_b():
        val.begin()
        for data, ids in batches:
            val.batch(data, ids)
        return val.finish()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / NBATCH, out

    for fn in (route_a, route_b, route_a, route_b):      # warm up every shape both routes use
        fn()
    ta, tb = [], []
    for _ in range(args.rounds):                          # alternated: both see the same machine
        ms, ma = timed(route_a)
        ta.append(ms)
        ms, mb = timed(route_b)
        tb.append(ms)
        assert all(ma[k] == mb[k] for k in KEYS), (ma, mb)
    fmt = lambda t: "median %.3f  min %.3f  max %.3f ms/batch" % (statistics.median(t), min(t), max(t))
    lines = ["validation pass, PoseNetRGBDGeometric bs32 bf16, %d batches, 13 meshes x 500 points, %d alternated "
             "rounds, device events" % (NBATCH, args.rounds),
             "(a) drop-in module + eval_metrics per batch (sync_weights once): " + fmt(ta),
             "(b) captured Validator on the trainer's engines, finish() in the window: " + fmt(tb),
             "ratio of medians (a) / (b): %.2f" % (statistics.median(ta) / statistics.median(tb)),
             "metrics equal on both routes: add_mean %.6f mm, add_01d_acc %.4f %%" % (mb["add_mean"], mb["add_01d_acc"])]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
