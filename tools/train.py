"""Train a PoseNet on LineMOD: the command line of the reference's four
scripts/training/train_*.py on pose6d.fit.

    python tools/train.py --model rgbd_geometric --data-root .../Linemod_preprocessed/data \
        --mesh-dir .../Linemod_preprocessed/models [--save-dir weights_rgbd_geometric]

The scripts' own settings are the defaults: 75 epochs of batch 32, AdamW(lr 1e-4, weight decay
1e-4), PoseLoss(1, 10, geodesic), gradient clip 1.0, ReduceLROnPlateau(max, 0.5, patience 5;
train_rgb.py: min_lr 1e-7), ColorJitter(0.3, 0.3, 0.3, 0.05) + RandomErasing(p=0.2,
scale=(0.02, 0.1)) and the bbox jitter on the train split, validation on the val split with
ADDLoss, last_pose_model.pth every epoch and best_pose_model.pth on a new best ADD-0.1d, resume
from last_pose_model.pth when it is there.  Every frame of both splits is decoded once into
device memory (pose6d.store.FrameStore); an epoch is then one upload, one graph replay per step
and one read-back.  --criterion add trains on the ADD / ADD-S loss alone (rot / trans weight 0).
--seed makes the run reproducible (sampler, bbox jitter, train transform, model init, dropout);
without it the streams are torch's and numpy's global ones, as in the scripts.
ImageNet weights: POSE6D_RESNET50_WEIGHTS (pose6d/resnet.py).
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "6d-pose-estimation_amd")]

MODELS = ("rgb", "rgb_geometric", "rgbd", "rgbd_geometric")


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", required=True, choices=MODELS)
    ap.add_argument("--data-root", default=os.path.join(REPO, "datasets", "Linemod_preprocessed", "data"))
    ap.add_argument("--mesh-dir", default=os.path.join(REPO, "datasets", "Linemod_preprocessed", "models"))
    ap.add_argument("--save-dir", default=None, help="default: weights_<model> in the repository root")
    ap.add_argument("--epochs", type=int, default=75)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--weight-decay", type=float, default=1e-4)
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--criterion", choices=("pose", "add"), default="pose")
    ap.add_argument("--objects", default=None, help="comma-separated object folders to keep, e.g. 01,06")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--no-resume", action="store_true")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse(argv)
    import numpy as np
    import torch

    import models.pose_net_rgb as m_rgb
    import models.pose_net_rgb_geometric as m_rgbg
    import models.pose_net_rgbd as m_rgbd
    import models.pose_net_rgbd_geometric as m_rgbdg
    from models.add_loss import ADDLoss
    from pose6d import train as T
    from pose6d.data import TrainAugment
    from pose6d.fit import fit
    from pose6d.linemod import LineMODSet
    from pose6d.store import FrameStore
    from pose6d.validate import PlateauLR

    model_cls, trainer_cls, rgbd = {
        "rgb": (m_rgb.PoseNetRGB, T.RGBTrainer, False),
        "rgb_geometric": (m_rgbg.PoseNetRGBGeometric, T.RGBGeometricTrainer, False),
        "rgbd": (m_rgbd.PoseNetRGBD, T.RGBDTrainer, True),
        "rgbd_geometric": (m_rgbdg.PoseNetRGBDGeometric, T.RGBDGeometricTrainer, True)}[a.model]
    assert torch.cuda.is_available(), "tools/train.py trains on the GPU"
    dev = torch.device("cuda", 0)
    save_dir = a.save_dir or os.path.join(REPO, "weights_" + a.model)
    print(f"Training {a.model} model on {dev}")
    generator, rng = None, np.random
    if a.seed is not None:
        torch.manual_seed(a.seed)
        generator, rng = torch.Generator().manual_seed(a.seed), np.random.RandomState(a.seed)
    aug_seed = a.seed if a.seed is not None else int(torch.empty((), dtype=torch.int64).random_().item())
    objects = a.objects.split(",") if a.objects else None
    train_set = LineMODSet(a.data_root, "train", rgbd=rgbd, augment_bbox=True, objects=objects)
    val_set = LineMODSet(a.data_root, "val", rgbd=rgbd, augment_bbox=False, objects=objects)
    print(f"Train: {len(train_set)}, Val: {len(val_set)} samples")
    train_store, val_store = FrameStore.from_linemod(train_set, dev), FrameStore.from_linemod(val_set, dev)

    model = model_cls(pretrained=True).to(dev)
    print(f"Model parameters: {sum(p.numel() for p in model.parameters()) / 1e6:.2f}M")
    crit = ADDLoss(a.mesh_dir, dev)
    kw = {}
    if a.criterion == "add":
        kw = dict(add_loss=crit, add_weight=1.0, rot_weight=0.0, trans_weight=0.0)
    trainer = trainer_cls(model, a.batch, dtype=torch.bfloat16 if a.dtype == "bf16" else torch.float32, lr=a.lr,
                          weight_decay=a.weight_decay, max_norm=1.0, **kw)
    scheduler = PlateauLR(trainer, min_lr=1e-7 if a.model == "rgb" else 0.0)       # train_rgb.py:71
    fit(trainer, train_store, val_store, crit, a.epochs, save_dir=save_dir, scheduler=scheduler,
        augment=TrainAugment(seed=aug_seed), resume=not a.no_resume, generator=generator, rng=rng)
    return 0


if __name__ == "__main__":
    sys.exit(main())
