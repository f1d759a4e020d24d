"""What the ADD / ADD-S criterion costs inside the whole-step trainer: ms per captured
PoseNetRGBDGeometric training step at bs32 in bf16 (pose6d.train.RGBDGeometricTrainer,
hipGraph replay) on synthetic 500-point meshes (tests.synth.synthetic_meshes), for

  off            add_loss=None: PoseLoss(1, 10) alone, the step as it was
  mixed          PoseLoss(1, 10) + 1.0 * ADDLoss, object ids cycling over the 13 objects
  pure_add       rot_weight = trans_weight = 0, the same ids
  all_symmetric  the mixed trainer's graph with every id symmetric (9 / 10): the ADD-S search
                 runs for every sample, the worst case (the graph reads the ids at run time)

and, alone, the route the criterion replaces:

  eager          ADDLoss.forward(...) + .backward() on leaf (B, 4) / (B, 3) tensors, the same
                 meshes and ids (mixed and all-symmetric)

Everything is warmed up, then timed in alternating blocks (off, mixed, pure_add, ..., off, ...)
of --block steps each, every block between two device events and ended by a synchronise.  Per
variant: the median and the spread (min, 10th / 90th percentile, max) over the blocks; the
criterion's added time per step is a variant's median minus `off`'s of the same run.  Needs the
GPU: there is no CPU fallback.  Writes a text file (default profiles/add_step.txt) and prints
it."""
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
N_POINTS = 500


def _criterion(dev):
    from models.add_loss import ADDLoss
    from tests.synth import synthetic_meshes
    pts, diam = synthetic_meshes(N_POINTS, seed=0)
    crit = ADDLoss.__new__(ADDLoss)
    torch.nn.Module.__init__(crit)
    crit.points = {k: torch.from_numpy(v).to(dev) for k, v in pts.items()}
    crit.diameters, crit.device, crit._table = diam, dev, None
    return crit


def _trainer(dev, **kw):
    from models.pose_net_rgbd_geometric import PoseNetRGBDGeometric
    from pose6d.train import RGBDGeometricTrainer
    torch.manual_seed(0)
    tr = RGBDGeometricTrainer(PoseNetRGBDGeometric(pretrained=False).to(dev), B, dtype=torch.bfloat16, lr=1e-4,
                              weight_decay=1e-4, **kw)
    return tr


def _eager(crit, data, ids):
    gt_rot, gt_trans = data[4], data[5]
    g = torch.Generator().manual_seed(1)
    rot = torch.nn.functional.normalize(gt_rot.cpu() + 0.05 * torch.randn(B, 4, generator=g), dim=1)
    rot = rot.to(gt_rot.device).requires_grad_(True)
    trans = (gt_trans.cpu() + 0.005 * torch.randn(B, 3, generator=g)).to(gt_rot.device).requires_grad_(True)

    def step():
        rot.grad = trans.grad = None
        crit(rot, trans, gt_rot, gt_trans, ids).backward()
    return step


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
            "p90_ms": round(q[-1], 4), "max_ms": round(max(ms), 4)}


def measure(dev, blocks, block, warmup):
    from bench import synth_batch
    from tests.synth import LINEMOD_OBJ_IDS
    data = synth_batch(B, dev, seed=1000)
    crit = _criterion(dev)
    ids_mixed = torch.tensor([LINEMOD_OBJ_IDS[i % 13] for i in range(B)], dtype=torch.int64, device=dev)
    ids_sym = torch.tensor([9 + i % 2 for i in range(B)], dtype=torch.int64, device=dev)
    off = _trainer(dev)
    mixed = _trainer(dev, add_loss=crit, add_weight=1.0)
    pure = _trainer(dev, add_loss=crit, add_weight=1.0, rot_weight=0.0, trans_weight=0.0)
    for tr in (mixed, pure):
        tr.obj_ids.copy_(ids_mixed)
    for tr in (off, mixed, pure):
        tr.capture(data)
    paths = {"off": off.step, "mixed": lambda: mixed.step(obj_ids=ids_mixed), "pure_add": pure.step,
             "all_symmetric": lambda: mixed.step(obj_ids=ids_sym), "eager_mixed_ids": _eager(crit, data, ids_mixed),
             "eager_all_symmetric": _eager(crit, data, ids_sym)}
    for step in paths.values():
        for _ in range(warmup):
            step()
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(blocks):
        for k, step in paths.items():
            ms[k].append(_block_ms(step, block))
    out = {k: _summary(v) for k, v in ms.items()}
    base = out["off"]["median_ms"]
    for k in ("mixed", "pure_add", "all_symmetric"):
        out[k]["added_ms"] = round(out[k]["median_ms"] - base, 4)
    out["off"]["spread_ms"] = round(out["off"]["p90_ms"] - out["off"]["p10_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=12, help="timed blocks per variant (alternating)")
    ap.add_argument("--block", type=int, default=10, help="steps per block")
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps per variant")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "add_step.txt"))
    a = ap.parse_args()
    if a.blocks * a.block < 50:
        ap.error("time at least 50 steps per variant (--blocks x --block)")
    if not torch.cuda.is_available():
        sys.exit("tools/add_step.py needs the MI355X: no GPU found, and there is no CPU fallback")
    warnings.simplefilter("ignore")
    dev = torch.device("cuda", 0)
    res = measure(dev, a.blocks, a.block, a.warmup)
    lines = [f"PoseNetRGBDGeometric training step, batch {B}, bf16, 224x224, {N_POINTS}-point meshes, "
             f"{torch.cuda.get_device_name(0)}",
             f"{a.blocks} alternating blocks of {a.block} steps per variant after {a.warmup} warm-up steps; ms per step",
             f"{'variant':<22}{'median':>9}{'min':>9}{'p10':>9}{'p90':>9}{'max':>9}{'added':>9}"]
    for k, v in res.items():
        added = f"{v['added_ms']:>9.4f}" if "added_ms" in v else f"{'-':>9}"
        lines.append(f"{k:<22}{v['median_ms']:>9.4f}{v['min_ms']:>9.4f}{v['p10_ms']:>9.4f}{v['p90_ms']:>9.4f}"
                     f"{v['max_ms']:>9.4f}{added}")
    lines.append("added = median minus `off`'s median (the captured step without the criterion); eager_* = "
                 "ADDLoss.forward + backward alone, the route the criterion replaces")
    lines.append(json.dumps(res))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
