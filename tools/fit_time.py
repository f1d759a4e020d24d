"""us per training step of PoseNetRGBDGeometric (B = 32, bf16) on a synthetic frame store
(tools/feed_time.py's: 640 x 480 RGB-D frames, LineMOD-sized boxes with the bbox jitter), three
routes, each without and with the train transform (TrainAugment):

  (p) the planned epoch of pose6d.fit: EpochPlan.build() (host draws + ONE upload), then per
      step one replay of the graph plan_next -> indexed crop -> step -> loss_append, then the
      epoch's one device-to-host copy -- everything inside the timed window;
  (e) the EpochFeeder loop: per step the host's range check, bbox jitter and two uploads, the
      crop launch(es), one replay of the captured step, loss.item() -- the only way before
      pose6d.fit;
  (0) the floor: the bare replay of the captured step on static inputs, one sync at the end.

One trainer, one process: the routes alternate inside every repeat (each is one epoch of
len(store) // B steps), wall clock around a window that starts and ends synchronised; the median
and min .. max of --repeats repeats are reported.  The lr is 0-like (1e-9) so that hundreds of
steps on noise labels stay finite.

usage: python tools/fit_time.py [--out FILE] [--frames N] [--repeats R]"""
import argparse
import os
import statistics
import sys
import time
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "6d-pose-estimation_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

B = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fit_time.txt"))
    ap.add_argument("--frames", type=int, default=2048)   # 3.1 GB of frames, 64 steps (~0.3 s) per timed epoch
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    from models.pose_net_rgbd_geometric import PoseNetRGBDGeometric
    from pose6d.data import TrainAugment
    from pose6d.fit import Fit
    from pose6d.store import EpochFeeder
    from pose6d.train import RGBDGeometricTrainer
    from tools.feed_time import synth_store
    assert torch.cuda.is_available(), "fit_time.py measures on the GPU"
    warnings.simplefilter("ignore")
    dev = torch.device("cuda", 0)
    store = synth_store(args.frames, dev)
    torch.manual_seed(0)
    tr = RGBDGeometricTrainer(PoseNetRGBDGeometric(pretrained=False).to(dev), B, dtype=torch.bfloat16, lr=1e-9)
    quiet = lambda s: None
    fits, graphs = {}, {}
    for aug in (False, True):     # the two planned graphs (each Fit rewinds the trainer after its capture)
        fits[aug] = Fit(tr, store, None, None, 1, augment=TrainAugment(seed=1) if aug else None, log=quiet,
                        generator=torch.Generator().manual_seed(1), rng=np.random.RandomState(1))
        graphs[aug] = (tr.graphs, tr._before, tr._after)
    inputs, data = fits[True].inputs, fits[True].data
    snap = tr.snapshot()
    tr.capture(data)              # the bare step, on the same input tensors
    tr.restore(snap)
    bare = (tr.graphs, None, None)
    steps = fits[True].plan.steps
    epoch_no = [1]

    def use(g):
        tr.graphs, tr._before, tr._after = g

    def planned(aug):
        use(graphs[aug])
        f = fits[aug]
        f.begin_epoch(epoch_no[0])
        epoch_no[0] += 1
        f.run_steps()
        got = f.read_epoch(epoch_no[0])
        assert got["refused"] == 0 and got["status"] == 0 and len(got["losses"]) == steps
        return got["losses"]

    feed_aug = TrainAugment(seed=2)
    feed_gen, feed_rng = torch.Generator().manual_seed(2), np.random.RandomState(2)

    def feeder(aug):
        use(bare)
        losses = []
        for _ in EpochFeeder(store, B, generator=feed_gen, rng=feed_rng, augment=feed_aug if aug else None).into(inputs):
            tr.step()
            losses.append(tr.loss.item())
        return losses

    def floor(aug):
        use(bare)
        for _ in range(steps):
            tr.step()

    def timed(fn, aug):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(aug)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / steps

    routes = (("p", planned), ("e", feeder), ("0", floor))
    res = {}
    for aug in (False, True):
        for _, fn in routes:      # warm up every route once
            fn(aug)
        t = {k: [] for k, _ in routes}
        for _ in range(args.repeats):
            for k, fn in routes:
                t[k].append(timed(fn, aug))
        for k, _ in routes:
            res[(k, aug)] = t[k]
        # the plan alone: host draws + upload of one epoch
        t0 = time.perf_counter()
        fits[aug].plan.build()
        torch.cuda.synchronize()
        res[("build", aug)] = (time.perf_counter() - t0) * 1e6
    assert bool(torch.isfinite(tr.loss))

    names = {"p": "(p) planned epoch (pose6d.fit)", "e": "(e) EpochFeeder + step() + loss.item()",
             "0": "(0) bare replay, static inputs"}
    lines = [f"fit_time: PoseNetRGBDGeometric B={B} bf16, store of {args.frames} frames 480x640 RGB-D with bbox jitter, "
             f"{steps} steps per epoch, {args.repeats} alternated repeats, wall clock; us per step median [min .. max]"]
    for aug in (False, True):
        for k, _ in routes:
            v = res[(k, aug)]
            lines.append(f"{names[k]:42s} {'train' if aug else 'val  '} transform: {statistics.median(v):9.1f} us "
                         f"[{min(v):.1f} .. {max(v):.1f}]")
    for aug in (False, True):
        med = {k: statistics.median(res[(k, aug)]) for k, _ in routes}
        lines.append(f"{'train' if aug else 'val'} transform: (p) - (0) = {med['p'] - med['0']:+.1f} us, (e) - (0) = "
                     f"{med['e'] - med['0']:+.1f} us, (e) - (p) = {med['e'] - med['p']:+.1f} us per step; "
                     f"EpochPlan.build() of {steps} steps: {res[('build', aug)]:.0f} us per epoch "
                     f"({res[('build', aug)] / steps:.1f} us per step, inside (p))")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
