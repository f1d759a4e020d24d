"""Worker of tests/test_validation.py::test_ddp_validation_equals_global_batches (launched by
torch.distributed.run, 2 ranks on ONE GPU over gloo: RCCL needs a GPU per rank).
argv: OUT MESH_DIR.  Each rank builds an RGBDGeometricTrainer (bf16, B = 4 per rank) with the
process group, trains one eager step on its own batch, and validates its shard of three
global batches through a captured pose6d.validate.Validator; in the last batch rank 1's shard
is short (2 samples).  The ground truth is built from the rank's own eval predictions (a tiny
offset on the even rows, a rotation change and a 0.2 m offset on the odd ones), so the 0.1 d
test sees both outcomes.  Each rank saves its per-batch predictions, ground truth, object ids
and the dict finish() returned to OUT.<rank>.pt; the test rebuilds the global batches."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "6d-pose-estimation_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

# per rank, per global batch; ids 2 and 6 have no mesh, 9 / 10 are symmetric, 13 has 6 points
IDS = [[[9, 13, 2, 0], [10, 1, 6, 4], [0, 9, 5, 11]],
       [[1, 10, 4, 2], [13, 0, 8, 9], [10, 5]]]


def main():
    out, mesh_dir = sys.argv[1], sys.argv[2]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    from bench import synth_batch
    from models.add_loss import ADDLoss
    from models.pose_net_rgbd_geometric import PoseNetRGBDGeometric
    from pose6d.train import RGBDGeometricTrainer
    from pose6d.validate import Validator
    B = 4
    np.random.seed(1234)
    crit = ADDLoss(mesh_dir, "cuda")
    torch.manual_seed(0)
    model = PoseNetRGBDGeometric(pretrained=False).to(dev)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.eval()
    tr = RGBDGeometricTrainer(model, B, dtype=torch.bfloat16, process_group=dist.group.WORLD, bucket_mb=2.0)
    tr.step_eager(synth_batch(B, dev, seed=77 + rank))
    torch.cuda.synchronize()

    val = Validator(tr, crit)
    ids = [torch.tensor(x, dtype=torch.int64, device=dev) for x in IDS[rank]]
    datas = [synth_batch(len(x), dev, seed=100 + 10 * rank + k) for k, x in enumerate(ids)]
    val.capture(datas[0], ids[0])
    # first pass: the predictions the ground truth is built from
    val.begin()
    saved = {"rot": [], "trans": [], "gt_rot": [], "gt_trans": [], "ids": []}
    for d, oid in zip(datas, ids):
        n = len(oid)
        val.batch(d, oid)
        rot, trans = tr.rot[:n].clone(), tr.trans[:n].clone()
        g = torch.Generator().manual_seed(int(oid.sum()))
        gt_rot, gt_trans = rot.clone(), trans + 1e-4
        gt_rot[1::2] = torch.nn.functional.normalize(
            rot[1::2] + 0.3 * torch.randn(rot[1::2].shape, generator=g).to(dev), dim=1)
        gt_trans[1::2] += 0.2
        d[4], d[5] = gt_rot, gt_trans
        for key, t in zip(saved, (rot, trans, gt_rot, gt_trans, oid)):
            saved[key].append(t.cpu())
    val.finish()
    # the epoch under test
    val.begin()
    for k, (d, oid) in enumerate(zip(datas, ids)):
        val.batch(d, oid)
        n = len(oid)
        assert torch.equal(tr.rot[:n].cpu(), saved["rot"][k]) and torch.equal(tr.trans[:n].cpu(), saved["trans"][k])
    metrics = val.finish()
    saved["metrics"] = {k: (float(v) if isinstance(v, float) else int(v)) for k, v in metrics.items()}
    torch.save(saved, f"{out}.{rank}.pt")
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
