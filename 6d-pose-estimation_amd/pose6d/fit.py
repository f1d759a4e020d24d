"""The epoch driver: the reference's train() (scripts/training/train_rgbd_geometric.py:73-166,
and the same lines of train_rgb.py, train_rgb_geometric.py, train_rgbd.py) on the whole-step
trainers of pose6d.train, the frame store of pose6d.store and the validation pass of
pose6d.validate.

The epoch is what the step already is: planned once on the host, replayed on the device,
read back once.

EpochPlan  the host draws the whole epoch with EpochFeeder's own code -- the sampler's order,
           the rank's index batches, the bbox jitter, one TrainAugment seed per batch -- and
           uploads it in ONE copy; pose6d_plan_next then hands row after row to the step at a
           device-resident cursor, and the indexed crop (its train variant reading the seed
           from device memory) fills the trainer's inputs.  All of it is capturable.
Fit / fit  per training step one replay of ONE graph (plan.next -> the step -> pose6d_loss_append),
           no upload and no host read; per epoch one device-to-host copy of the loss table, the
           two state words and the store's status word; then the validation epoch, the plateau
           schedule, the reference's log line and its two checkpoint files.

DEPARTURE from the reference, kept from EpochFeeder: drop_last=True.  The step is captured at
one batch size, so the DataLoader's short last batch is not trained on; the `len(train_loader)`
of the reference's average (train_rgbd_geometric.py:117) is the number of steps run.
"""
import math
import os

import numpy as np
import torch

from ._lib import Pose6dError, call, stream
from .data import jitter_bboxes
from .store import EpochFeeder
from .validate import PlateauLR, Validator

CKPT_LAST, CKPT_BEST = "last_pose_model.pth", "best_pose_model.pth"

# the store's collated tuple (FrameStore.crop's order) and each trainer's data tuple, by name
STORE_TUPLE = {True: ("rgb", "depth", "depth_raw", "quat", "trans", "obj_id", "center", "K"),
               False: ("rgb", "quat", "trans", "obj_id", "center", "K")}
DATA_TUPLE = {"RGBTrainer": ("rgb", "quat", "trans"),
              "RGBGeometricTrainer": ("rgb", "center", "K", "quat", "trans"),
              "RGBDTrainer": ("rgb", "depth", "quat", "trans"),
              "RGBDGeometricTrainer": ("rgb", "depth_raw", "center", "K", "quat", "trans")}


def data_tuple(trainer, rgbd, batch):
    """The trainer's data tuple picked out of a store batch (DATA_TUPLE; the most derived
    trainer class that has a row decides)."""
    names = next((DATA_TUPLE[c.__name__] for c in type(trainer).__mro__ if c.__name__ in DATA_TUPLE), None)
    if names is None:
        raise Pose6dError(f"fit: no data tuple known for {type(trainer).__name__}")
    have = STORE_TUPLE[bool(rgbd)]
    missing = [n for n in names if n not in have]
    if missing:
        raise Pose6dError(f"fit: {type(trainer).__name__} needs {missing} -- an RGB-D frame store")
    return tuple(batch[have.index(n)] for n in names)


class EpochPlan:
    """One epoch of training batches, planned on the host and stepped through on the device.

    build() -- run by the constructor for the first epoch, then once per epoch -- walks
    EpochFeeder's own code (order(), index_batches() with drop_last=True, jitter_bboxes per
    batch in batch order when the store's set has augment_bbox, one augment.next_seed() per
    batch), so the torch generator, the numpy stream and TrainAugment.calls advance exactly as
    an EpochFeeder loop over the same `steps` batches would; checks every index on the host;
    uploads the tables in one copy into device tables allocated once; and zeroes the cursor.
    steps (default: the whole epoch, len(feeder)) plans the epoch's first `steps` batches.

    next(out) launches pose6d_plan_next and the indexed crop into `out` (FrameStore.crop's
    tuple): no upload, no allocation, capturable.  state (device int64[2]) = {cursor, steps
    refused}: a call past the plan's end changes no input and counts itself in state[1].
    host_idx (steps, B) int64, host_bbox (steps, B, 4) int32 or None, host_seed (steps,) uint64
    or None are the host tables of the last build()."""

    def __init__(self, store, batch_size, steps=None, shuffle=True, rank=0, world=1, generator=None, rng=np.random,
                 augment=None):
        self.store, self.B, self.augment, self.rng = store, int(batch_size), augment, rng
        self.feeder = EpochFeeder(store, batch_size, shuffle=shuffle, drop_last=True, rank=rank, world=world,
                                  generator=generator, rng=rng, augment=augment)
        cap = len(self.feeder)
        self.steps = cap if steps is None else int(steps)
        if not 0 < self.steps <= cap:
            raise Pose6dError(f"EpochPlan: {self.steps} steps, the epoch has {cap} whole batches of "
                              f"{self.B} x {world} from {len(store)} samples")
        B, n, dev = self.B, self.steps, store.device
        self.jitter = bool(store.augment_bbox)
        # one buffer of int64 words = one upload: idx [n][B] | seed [n] | bbox [n][B][4] int32
        n_idx, n_seed, n_box = n * B, n if augment is not None else 0, 2 * n * B if self.jitter else 0
        self._host = torch.zeros(n_idx + n_seed + n_box, dtype=torch.int64, pin_memory=dev.type == "cuda")
        self._dev = torch.zeros(n_idx + n_seed + n_box, dtype=torch.int64, device=dev)

        def views(buf):
            return (buf[:n_idx].view(n, B), buf[n_idx:n_idx + n_seed] if n_seed else None,
                    buf[n_idx + n_seed:].view(torch.int32).view(n, B, 4) if n_box else None)

        hi, hs, hb = views(self._host)
        self.host_idx = hi.numpy()
        self.host_seed = None if hs is None else hs.numpy().view(np.uint64)
        self.host_bbox = None if hb is None else hb.numpy()
        self.idx_tab, self.seed_tab, self.bbox_tab = views(self._dev)
        self.state = torch.zeros(2, dtype=torch.int64, device=dev)
        # what the step's crop reads: the cursor's row, copied here by pose6d_plan_next
        self.idx = torch.zeros(B, dtype=torch.int64, device=dev)
        self.bbox = torch.zeros(B, 4, dtype=torch.int32, device=dev) if self.jitter else None
        self.seed = torch.zeros(1, dtype=torch.int64, device=dev) if augment is not None else None
        if augment is not None and dev.type == "cuda":
            store.reserve_train(B)
        self.build()

    def build(self):
        store, n_samples = self.store, len(self.store)
        k = 0
        for idx in self.feeder.index_batches():
            if k == self.steps:
                break
            if len(idx) != self.B or idx.min() < 0 or idx.max() >= n_samples:
                raise Pose6dError(f"EpochPlan: batch {k} holds {len(idx)} indices in [{idx.min()}, {idx.max()}]; "
                                  f"want {self.B} in [0, {n_samples})")
            self.host_idx[k] = idx
            if self.jitter:
                self.host_bbox[k] = jitter_bboxes(store.host_bbox[idx], self.feeder.rgbd, self.rng)
            if self.augment is not None:
                self.host_seed[k] = self.augment.next_seed()
            k += 1
        if k != self.steps:
            raise Pose6dError(f"EpochPlan: the feeder gave {k} batches, {self.steps} were planned")
        self._dev.copy_(self._host)     # the epoch's one upload (it returns when the host buffer is free again)
        self.state.zero_()
        return self

    def next(self, out):
        call("plan_next", self.idx_tab, self.bbox_tab, self.seed_tab, self.steps, self.B, self.state, self.idx,
             self.bbox, self.seed, stream())
        return self.store.crop_planned(self.idx, self.bbox, out, augment=self.augment, seed=self.seed)


class Fit:
    """fit()'s state and steps; `Fit(...).run()` is `fit(...)`.

    The constructor resumes (resume=True and save_dir holds last_pose_model.pth), plans the
    first epoch and captures the trainer's step with the plan's next batch in front and the
    loss append behind.  Capturing warms up with real optimizer steps that also advance the
    cursor: the trainer is snapshotted before and restored after, and the cursor and the loss
    table are reset, so training starts from the weights it was given.

    steps: train on the first `steps` batches of every epoch (default: the whole epoch).
    Under a process group (trainer.pg) each rank plans its shard, rank 0 writes the files and
    every rank gets the Validator's global metrics; a resume hands every rank the random
    streams rank 0 saved."""

    def __init__(self, trainer, train_store, val_store, add_loss, epochs, save_dir=None, scheduler=None, augment=None,
                 resume=True, generator=None, rng=np.random, log=print, steps=None):
        self.trainer, self.train_store, self.val_store, self.add_loss = trainer, train_store, val_store, add_loss
        self.epochs, self.save_dir, self.augment = int(epochs), save_dir, augment
        self.generator, self.rng, self.log, self.steps = generator, rng, log, steps
        self.scheduler = scheduler if scheduler is not None else PlateauLR(trainer)
        self.history, self.best_acc, self.start_epoch = [], 0.0, 0
        pg = getattr(trainer, "pg", None)
        self.rank = torch.distributed.get_rank(pg) if pg is not None else 0
        self.world = torch.distributed.get_world_size(pg) if pg is not None else 1
        self.validator = None
        if save_dir is not None and self.rank == 0:
            os.makedirs(save_dir, exist_ok=True)
        if resume and save_dir is not None:
            self._resume()
        self._prepare()

    # ------------------------------------------------------------- resume
    def _resume_state(self, best_acc):
        g = self.generator
        return {"torch_generator": (g.get_state() if g is not None else torch.get_rng_state()).clone(),
                "numpy_rng": self.rng.get_state(),
                "augment_calls": None if self.augment is None else int(self.augment.calls),
                "dropout_seed": int(self.trainer.seed.item()), "best_acc": best_acc,
                "history": [dict(r) for r in self.history]}

    def _resume(self):
        """train_rgbd_geometric.py:73-89.  A file that does not load, or does not fit the
        model, is logged and training starts fresh, as the script's try / except does (here
        the trainer is also put back to what it was given).  With the `pose6d_resume` entry the
        run continues bit for bit; without it (a checkpoint the reference wrote) the random
        streams are the fresh ones and the lr is the optimizer state's."""
        path = os.path.join(self.save_dir, CKPT_LAST)
        if not os.path.exists(path):
            self.log("Starting training from scratch")
            return
        self.log(f"Resuming from checkpoint: {path}")
        tr, snap = self.trainer, self.trainer.snapshot()
        try:
            ckpt = torch.load(path, map_location=tr.dev, weights_only=False)
            start = tr.load_checkpoint(ckpt)
            best = ckpt.get("best_acc", 0.0)
            if "scheduler_state_dict" in ckpt:
                self.scheduler.load_state_dict(ckpt["scheduler_state_dict"])
            elif isinstance(self.scheduler, PlateauLR):   # a fresh scheduler on the loaded optimizer's lr
                self.scheduler.optimizer.param_groups[0]["lr"] = float(tr.hp[0])
            extra = ckpt.get("pose6d_resume")
            if extra is not None:
                if self.generator is not None:
                    self.generator.set_state(extra["torch_generator"].cpu())
                else:
                    torch.set_rng_state(extra["torch_generator"].cpu())
                self.rng.set_state(extra["numpy_rng"])
                if self.augment is not None and extra["augment_calls"] is not None:
                    self.augment.calls = int(extra["augment_calls"])
                tr.seed.fill_(int(extra["dropout_seed"]))
                best = extra["best_acc"]
                self.history = [dict(r) for r in extra["history"]]
            self.start_epoch, self.best_acc = int(start), best
            self.log(f"Resumed at epoch {self.start_epoch}, best accuracy: {self.best_acc:.2f}%")
        except Exception as e:   # noqa: BLE001 -- the script's bare except
            tr.restore(snap)
            self.history, self.best_acc, self.start_epoch = [], 0.0, 0
            self.log(f"Checkpoint not usable ({type(e).__name__}: {e}), starting fresh")

    # ------------------------------------------------------------- capture
    def _prepare(self):
        tr, store, B = self.trainer, self.train_store, self.trainer.B
        self.plan = EpochPlan(store, B, steps=self.steps, rank=self.rank, world=self.world, generator=self.generator,
                              rng=self.rng, augment=self.augment)
        self._planned_for = self.start_epoch
        names = STORE_TUPLE[store.rgbd]
        self.inputs = list(store._outputs(B))
        if getattr(tr, "add_loss", None) is not None:    # the ADD criterion reads the crop's ids where they land
            self.inputs[names.index("obj_id")] = tr.obj_ids
        self.inputs = tuple(self.inputs)
        self.data = data_tuple(tr, store.rgbd, self.inputs)
        n = self.plan.steps
        # ONE allocation, read back in one copy per epoch (int64 words):
        # plan state [2] | loss state [3] | store status [1] | loss table [n] fp32
        self._buf = torch.zeros(6 + (n + 1) // 2, dtype=torch.int64, device=tr.dev)
        self.loss_state = self._buf[2:5]
        self.loss_table = self._buf[6:].view(torch.float32)
        snap = tr.snapshot()
        tr.capture(self.data, before=self._next_batch, after=self._append_loss)
        tr.restore(snap)
        self.plan.state.zero_()
        self.loss_state.zero_()

    def _next_batch(self):
        self.plan.next(self.inputs)

    def _append_loss(self):
        call("loss_append", self.trainer.loss, self.loss_table, self.plan.steps, self.loss_state, stream())

    # ------------------------------------------------------------- the epoch
    def begin_epoch(self, epoch):
        """The epoch's plan (the constructor built the first one), cursor and loss table at 0."""
        if self._planned_for != epoch:
            self.plan.build()
            self._planned_for = epoch
        self.loss_state.zero_()

    def run_steps(self):
        """The epoch's training steps: one graph replay each, no upload, no host read."""
        for _ in range(self.plan.steps):
            self.trainer.step()

    def train_epoch(self, epoch):
        """begin_epoch, run_steps, read_epoch."""
        self.begin_epoch(epoch)
        self.run_steps()
        return self.read_epoch(epoch)

    def read_epoch(self, epoch):
        """The epoch's one device-to-host copy.  Returns the step losses (Python floats, in
        order), the refused count of both tables, the non-finite count and the store's status
        word."""
        plan, n = self.plan, self.plan.steps
        self._buf[0:2].copy_(plan.state)
        self._buf[5:6].copy_(self.train_store._status)
        host = self._buf.cpu()
        cursor, plan_refused, rows, loss_refused, nonfinite, status = (int(v) for v in host[:6])
        losses = host[6:].view(torch.float32)[:n].tolist()
        if (cursor, rows) != (n, n) and not (plan_refused or loss_refused):
            raise Pose6dError(f"fit: epoch {epoch} ran {n} steps, the plan's cursor is at {cursor} and the loss "
                              f"table holds {rows} rows")
        return {"losses": losses, "refused": plan_refused + loss_refused, "nonfinite": nonfinite, "status": status}

    def validate(self):
        """One validation epoch (train_rgbd_geometric.py:119-144): Validator over the val
        store in index order, the short last batch included, the batch body captured once."""
        tr, store, B = self.trainer, self.val_store, self.trainer.B
        n_batches = max(1, math.ceil(len(store) / (B * self.world)))
        if self.validator is None:
            self.validator = Validator(tr, self.add_loss, max_samples=n_batches * B)
            self._val_out = store._outputs(B)
        val, obj = self.validator, STORE_TUPLE[store.rgbd].index("obj_id")
        feeder = EpochFeeder(store, B, shuffle=False, drop_last=False, rank=self.rank, world=self.world)
        val.begin()
        k, data = 0, None
        for batch in feeder.into(self._val_out):
            data = data_tuple(tr, store.rgbd, batch)
            if val.graph is None:
                val.capture(data, batch[obj])
            val.batch(data, batch[obj])
            k += 1
        while k < n_batches and data is not None:   # a rank whose shard ends one batch early: an empty batch
            val.batch(tuple(t[:0] for t in data), batch[obj][:0])
            k += 1
        return val.finish()

    def run(self):
        for epoch in range(self.start_epoch, self.epochs):
            self.run_epoch(epoch)
        self.log(f"\nTraining complete. Best ADD-0.1d: {self.best_acc:.2f}%")
        return self.history

    def run_epoch(self, epoch):
        got = self.train_epoch(epoch)
        self.train_store.check(status=got["status"])
        if got["refused"]:
            raise Pose6dError(f"fit: epoch {epoch}: {got['refused']} step(s) ran past the epoch's plan or its loss "
                              "table")
        train_loss = 0.0
        for v in got["losses"]:      # the reference's `train_loss += loss.item()`, in step order
            train_loss += v
        avg_train_loss = train_loss / len(got["losses"])
        m = self.validate()
        val_add, val_acc = m["add_mean"], m["add_01d_acc"]
        self.scheduler.step(val_acc)
        lr = self.scheduler.lr if hasattr(self.scheduler, "lr") else float(self.trainer.hp[0])
        rec = {"epoch": epoch, "train_loss": avg_train_loss, "val_add": val_add, "val_acc": val_acc, "lr": lr,
               "steps": len(got["losses"]), "nonfinite": got["nonfinite"]}
        self.history.append(rec)
        self.log(f"Epoch {epoch + 1}/{self.epochs}")
        self.log(f"  Loss: {avg_train_loss:.4f} | ADD: {val_add:.1f}mm | ADD-0.1d: {val_acc:.1f}% | LR: {lr:.2e}")
        if got["nonfinite"]:
            self.log(f"  {got['nonfinite']} of {rec['steps']} step losses were not finite")
        better = val_acc > self.best_acc
        saving = self.save_dir is not None and self.rank == 0
        ckpt = None
        if saving:      # train_rgbd_geometric.py:150-158: `best_acc` in the last file is the one before this epoch
            extra = {"pose6d_resume": self._resume_state(val_acc if better else self.best_acc)}
            if hasattr(self.scheduler, "state_dict"):
                extra["scheduler_state_dict"] = self.scheduler.state_dict()
            ckpt = self.trainer.checkpoint(epoch, best_acc=self.best_acc, curr_acc=val_acc, **extra)
            self._save(ckpt, CKPT_LAST)
        if better:
            self.best_acc = val_acc
            if saving:
                ckpt["best_acc"] = self.best_acc
                self._save(ckpt, CKPT_BEST)
            self.log(f"  New best model saved (ADD-0.1d: {self.best_acc:.2f}%)")
        return rec

    def _save(self, ckpt, name):
        path = os.path.join(self.save_dir, name)
        torch.save(ckpt, path + ".tmp")
        os.replace(path + ".tmp", path)      # a killed run leaves the previous file, not half of a new one


def fit(trainer, train_store, val_store, add_loss, epochs, save_dir=None, scheduler=None, augment=None, resume=True,
        generator=None, rng=np.random, log=print, steps=None):
    """Train `trainer` (any of pose6d.train's four) for `epochs` epochs on `train_store`,
    validating on `val_store` with `add_loss` (a models.add_loss.ADDLoss) after each: the
    reference's train().  scheduler: default PlateauLR(trainer) (train_rgb.py passes
    min_lr=1e-7); augment: a TrainAugment for the train transform; save_dir: where
    last_pose_model.pth / best_pose_model.pth go (None: nothing is written or resumed).
    Returns the epoch records: epoch, train_loss, val_add, val_acc, lr, steps, nonfinite."""
    return Fit(trainer, train_store, val_store, add_loss, epochs, save_dir=save_dir, scheduler=scheduler,
               augment=augment, resume=resume, generator=generator, rng=rng, log=log, steps=steps).run()
