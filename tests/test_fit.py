"""pose6d.fit: the epoch driver (the reference's train(), train_rgbd_geometric.py:73-166) on
the whole-step trainers -- planned epoch == EpochFeeder loop bit for bit, the weights across
the capture, resume, checkpoint interchange, the epoch's control flow on stubs, tools/train.py.

GPU tests run at the trainers' test size: B = 4 at 224^2, pretrained=False, frames from
tests.synth.write_linemod_tree (120 x 160), meshes from write_mesh_dir.  Every comparison of
training state is torch.equal and every comparison of losses / records is == on Python floats:
both routes replay the same captured launches on the same inputs."""
import os
import shutil
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from tests.synth import write_linemod_tree, write_mesh_dir

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 4
STEPS = 3


# ------------------------------------------------------------------ CPU: control flow on stubs
class _StubTrainer:
    """What Fit touches outside the three methods the stub Fit below replaces."""
    dev, B = "cpu", B

    def __init__(self, lr=1e-4):
        self.hp, self.lrs, self.restored = [lr], [], 0
        self.seed = torch.tensor([41])

    def set_lr(self, lr):
        self.hp[0] = lr
        self.lrs.append(lr)

    def snapshot(self):
        return list(self.hp)

    def restore(self, snap):
        self.hp[:] = snap
        self.restored += 1

    def checkpoint(self, epoch, best_acc=0.0, curr_acc=0.0, **extra):
        return {"epoch": epoch, "model_state_dict": {}, "optimizer_state_dict": {"lr": self.hp[0]},
                "best_acc": best_acc, "curr_acc": curr_acc, **extra}

    def load_checkpoint(self, ckpt):
        self.hp[0] = ckpt["optimizer_state_dict"]["lr"]
        return ckpt["epoch"] + 1


class _StubStore:
    def __init__(self):
        self.checked = []

    def check(self, status=None):
        self.checked.append(status)


def _stub_fit(accs, refused_at=None, **kw):
    """A Fit whose capture, training epoch and validation pass are stubs: the epoch's losses
    are (epoch + 1, epoch + 2), its validation accuracy the scripted one."""
    from pose6d.fit import Fit

    class StubFit(Fit):
        saved = []

        def _prepare(self):
            self.seen = []

        def train_epoch(self, epoch):
            return {"losses": [epoch + 1.0, epoch + 2.0], "refused": int(epoch == refused_at), "nonfinite": 0,
                    "status": 0}

        def validate(self):
            acc = accs[len(self.history)]
            self.seen.append(acc)
            return {"add_mean": 100.0 - acc, "add_s_mean": 1.0, "add_01d_acc": acc}

        def _save(self, ckpt, name):
            self.saved.append((ckpt["epoch"], name, ckpt["best_acc"]))
            super()._save(ckpt, name)

    StubFit.saved = []
    return StubFit(_StubTrainer(), _StubStore(), None, None, **kw)


# best 20 after epoch 1, then six epochs without improvement (patience 5 -> the lr halves at
# epoch 7), a new best at epoch 8, an equal value at epoch 9 (not a strict improvement)
_ACCS = [10.0, 20.0, 15.0, 15.0, 20.0, 15.0, 15.0, 15.0, 30.0, 30.0]


def _torch_lrs(lr):
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([p], lr=lr)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="max", factor=0.5, patience=5)
    out = []
    for a in _ACCS:
        sched.step(a)
        out.append(opt.param_groups[0]["lr"])
    return out


def test_epoch_control_flow_on_stubs(tmp_path):
    from pose6d.fit import CKPT_BEST, CKPT_LAST
    d = str(tmp_path)
    lines = []
    f = _stub_fit(_ACCS, epochs=len(_ACCS), save_dir=d, log=lines.append)
    assert lines == ["Starting training from scratch"] and f.start_epoch == 0
    hist = f.run()
    assert f.seen == _ACCS                                          # scheduler / validation: each value once
    want_lr = _torch_lrs(1e-4)
    assert want_lr[6] == 1e-4 and want_lr[7] == 5e-5                # the plateau is in the script
    assert [r["lr"] for r in hist] == want_lr and f.trainer.lrs == [5e-5] and f.trainer.hp[0] == 5e-5
    assert [r["val_acc"] for r in hist] == _ACCS and [r["epoch"] for r in hist] == list(range(len(_ACCS)))
    assert [r["train_loss"] for r in hist] == [(2 * e + 3.0) / 2 for e in range(len(_ACCS))]
    assert f.train_store.checked == [0] * len(_ACCS)
    # last every epoch (carrying the best accuracy from BEFORE the epoch, as the script does),
    # best on strict improvement only
    assert [(e, b) for e, n, b in f.saved if n == CKPT_LAST] == \
        [(0, 0.0), (1, 10.0)] + [(e, 20.0) for e in range(2, 9)] + [(9, 30.0)]
    assert [(e, b) for e, n, b in f.saved if n == CKPT_BEST] == [(0, 10.0), (1, 20.0), (8, 30.0)]
    assert f.best_acc == 30.0
    assert "  Loss: 1.5000 | ADD: 90.0mm | ADD-0.1d: 10.0% | LR: 1.00e-04" in lines
    assert sum(l.startswith("  New best model saved") for l in lines) == 3
    last = torch.load(os.path.join(d, CKPT_LAST), weights_only=False)
    assert {"epoch", "model_state_dict", "optimizer_state_dict", "best_acc", "curr_acc", "scheduler_state_dict",
            "pose6d_resume"} == set(last)
    assert set(last["pose6d_resume"]) == {"torch_generator", "numpy_rng", "augment_calls", "dropout_seed",
                                          "best_acc", "history"}
    assert not [n for n in os.listdir(d) if n.endswith(".tmp")]

    # resume: epoch + 1, the best accuracy, the history, the scheduler and its lr
    lines2 = []
    g = _stub_fit(_ACCS + [25.0, 40.0], epochs=len(_ACCS) + 2, save_dir=d, log=lines2.append)
    assert g.start_epoch == len(_ACCS) and g.best_acc == 30.0 and g.history == hist
    assert g.trainer.hp[0] == 5e-5 and g.scheduler.lr == 5e-5
    assert lines2[-1] == "Resumed at epoch 10, best accuracy: 30.00%"
    more = g.run()
    assert [r["epoch"] for r in more] == list(range(len(_ACCS) + 2)) and g.best_acc == 40.0
    assert [(e, n) for e, n, b in g.saved] == [(10, CKPT_LAST), (11, CKPT_LAST), (11, CKPT_BEST)]
    # resume=False ignores the file
    assert _stub_fit(_ACCS, epochs=1, save_dir=d, resume=False, log=lines.append).start_epoch == 0


def test_refused_steps_raise():
    from pose6d._lib import Pose6dError
    f = _stub_fit(_ACCS, refused_at=1, epochs=3, log=lambda s: None)
    with pytest.raises(Pose6dError, match="ran past"):
        f.run()
    assert len(f.history) == 1 and f.seen == _ACCS[:1]              # epoch 1 never reached its validation


def test_corrupt_checkpoint_logs_and_starts_fresh(tmp_path):
    from pose6d.fit import CKPT_LAST
    with open(tmp_path / CKPT_LAST, "wb") as fh:
        fh.write(b"not a checkpoint")
    lines = []
    f = _stub_fit(_ACCS, epochs=2, save_dir=str(tmp_path), log=lines.append)
    assert f.start_epoch == 0 and f.best_acc == 0.0 and f.history == [] and f.trainer.restored == 1
    assert lines[0].startswith("Resuming from checkpoint") and "starting fresh" in lines[1]
    assert len(f.run()) == 2


def test_data_tuples():
    """The issue's table: each trainer's data tuple out of the store's collated tuple."""
    from pose6d import train as T
    from pose6d._lib import Pose6dError
    from pose6d.fit import data_tuple
    rgbd = ("rgb", "depth", "depth_raw", "quat", "trans", "obj_id", "center", "K")
    rgb = ("rgb", "quat", "trans", "obj_id", "center", "K")
    mk = lambda cls: cls.__new__(cls)
    assert data_tuple(mk(T.RGBTrainer), False, rgb) == ("rgb", "quat", "trans")
    assert data_tuple(mk(T.RGBTrainer), True, rgbd) == ("rgb", "quat", "trans")
    assert data_tuple(mk(T.RGBGeometricTrainer), False, rgb) == ("rgb", "center", "K", "quat", "trans")
    assert data_tuple(mk(T.RGBDTrainer), True, rgbd) == ("rgb", "depth", "quat", "trans")
    assert data_tuple(mk(T.RGBDGeometricTrainer), True, rgbd) == ("rgb", "depth_raw", "center", "K", "quat", "trans")
    with pytest.raises(Pose6dError, match="RGB-D"):
        data_tuple(mk(T.RGBDTrainer), False, rgb)


def test_train_tool_help_runs_without_a_gpu():
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "train.py"), "--help"], capture_output=True,
                       text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stderr
    for flag in ("--model", "--data-root", "--mesh-dir", "--save-dir", "--epochs", "--batch", "--lr", "--weight-decay",
                 "--dtype", "--criterion", "--objects", "--seed", "--no-resume"):
        assert flag in r.stdout


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("linemod_fit"))
    write_linemod_tree(root, n_frames=30)
    return root


@pytest.fixture(scope="module")
def mesh_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("meshes_fit"))
    write_mesh_dir(d, n_vertices=700, seed=11)
    return d


@pytest.fixture(scope="module")
def crit(mesh_dir):
    from models.add_loss import ADDLoss
    np.random.seed(1234)
    return ADDLoss(mesh_dir, "cuda")


def _store(tree, split, rgbd):
    from pose6d.linemod import LineMODSet
    from pose6d.store import FrameStore
    return FrameStore.from_linemod(LineMODSet(tree, split, rgbd=rgbd), "cuda")


def _trainer(kind, dtype, **kw):
    from pose6d import train as T
    if kind == "rgbd_geometric":
        from models.pose_net_rgbd_geometric import PoseNetRGBDGeometric as M
        cls = T.RGBDGeometricTrainer
    else:
        from models.pose_net_rgb import PoseNetRGB as M
        cls = T.RGBTrainer
    warnings.simplefilter("ignore")
    torch.manual_seed(0)
    return cls(M(pretrained=False).cuda(), B, dtype=dtype, **kw)


def _bufs(tr):
    return [b for n, b in tr.model.named_buffers() if "running" in n or "num_batches" in n]


def _train_state(tr):
    return [t.clone() for t in (tr.arena.flat, tr.m, tr.v, tr.hp, tr.seed, *_bufs(tr))]


def _streams(augmented):
    from pose6d.data import TrainAugment
    return dict(generator=torch.Generator().manual_seed(7), rng=np.random.RandomState(5),
                augment=TrainAugment(seed=3) if augmented else None)


def _sync_debug_raises():
    """Whether this build's sync debug mode turns a device-to-host read into an error."""
    probe = torch.zeros((), device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        probe.item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,dtype,augmented", [("rgbd_geometric", torch.bfloat16, True),
                                                  ("rgb", torch.float32, False)], ids=["rgbd_geo-bf16-aug", "rgb-fp32"])
def test_planned_epoch_equals_feeder_loop(tree, kind, dtype, augmented):
    """One epoch of 3 steps from identically seeded models.  Route (i): EpochFeeder.into(inputs),
    trainer.step(), loss.item().  Route (ii): the planned epoch, one graph replay per step
    (under the sync debug mode's "error" setting when this build enforces it)."""
    from pose6d.fit import Fit, data_tuple
    from pose6d.store import EpochFeeder
    rgbd = kind == "rgbd_geometric"
    stores = [_store(tree, "train", rgbd), _store(tree, "train", rgbd)]
    for s in stores:
        assert s.augment_bbox and len(s) >= STEPS * B
        s.augment_bbox = augmented              # the RGB / fp32 case: neither jitter nor transform

    tr = _trainer(kind, dtype)
    init = tr.arena.flat.clone()
    inputs = stores[0]._outputs(B)
    data = data_tuple(tr, rgbd, inputs)
    snap = tr.snapshot()
    tr.capture(data)
    tr.restore(snap)
    losses = []
    feeder = EpochFeeder(stores[0], B, **_streams(augmented)).into(inputs)
    for _, batch in zip(range(STEPS), feeder):
        assert batch is inputs
        tr.step()
        losses.append(tr.loss.item())
    stores[0].check()                           # status word 0
    want = _train_state(tr)
    del tr, feeder

    tr = _trainer(kind, dtype)
    f = Fit(tr, stores[1], None, None, 1, steps=STEPS, log=lambda s: None, **_streams(augmented))
    assert torch.equal(tr.arena.flat, init)     # capture's warm-up steps were rewound
    assert len(tr.graphs) == 1
    f.begin_epoch(0)
    enforced = _sync_debug_raises()
    print("sync debug mode enforced:", enforced)
    if enforced:
        torch.cuda.set_sync_debug_mode("error")
    try:
        f.run_steps()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = f.read_epoch(0)
    assert got["losses"] == losses and all(np.isfinite(losses)) and len(set(losses)) == STEPS
    assert (got["refused"], got["nonfinite"], got["status"]) == (0, 0, 0)
    stores[1].check()
    for i, (a, b) in enumerate(zip(_train_state(tr), want)):
        assert torch.equal(a, b), i
    assert not torch.equal(tr.arena.flat, init)
    # a step past the plan changes no input and is counted
    before = [t.clone() for t in f.inputs]
    f.plan.next(f.inputs)
    assert f.plan.state.tolist() == [STEPS, 1] and all(torch.equal(a, b) for a, b in zip(before, f.inputs))


@pytest.mark.gpu
def test_weights_survive_capture(tree):
    """fit's capture warms up with real optimizer steps on the plan's first batches; afterwards
    everything a step changes is what it was, and cursor and loss table are at zero."""
    from pose6d.fit import Fit
    store = _store(tree, "train", False)
    tr = _trainer("rgb", torch.bfloat16)
    init = _train_state(tr)
    f = Fit(tr, store, None, None, 1, steps=2, log=lambda s: None, **_streams(True))
    for i, (a, b) in enumerate(zip(_train_state(tr), init)):
        assert torch.equal(a, b), i
    assert f.plan.state.tolist() == [0, 0] and f.loss_state.tolist() == [0, 0, 0]
    assert f.plan.seed is not None and f.plan.bbox is not None and f.augment.calls == 2


def _fit_run(tree_stores, crit, epochs, save_dir, **kw):
    """Everything but the (stateless) stores rebuilt from scratch: model, trainer, random
    streams, scheduler, plan, validator."""
    from pose6d.fit import Fit
    tr = _trainer("rgbd_geometric", torch.bfloat16)
    lines = []
    f = Fit(tr, tree_stores[0], tree_stores[1], crit, epochs, save_dir=save_dir, steps=2, log=lines.append,
            **_streams(True), **kw)
    f.lines = lines
    return f


@pytest.fixture(scope="module")
def rgbd_stores(tree):
    return _store(tree, "train", True), _store(tree, "val", True)


@pytest.fixture(scope="module")
def one_epoch(rgbd_stores, crit, tmp_path_factory):
    """Run B's first half: one epoch into a fresh save_dir."""
    d = str(tmp_path_factory.mktemp("weights_fit"))
    f = _fit_run(rgbd_stores, crit, 1, d)
    hist = f.run()
    assert len(hist) == 1 and f.lines[0] == "Starting training from scratch"
    return d, [dict(r) for r in hist]


@pytest.mark.gpu
def test_resume_is_bit_identical(rgbd_stores, crit, one_epoch, tmp_path):
    from pose6d.fit import CKPT_BEST, CKPT_LAST
    d, first = one_epoch
    d = shutil.copytree(d, str(tmp_path / "weights"))               # run B's second half writes here
    a = _fit_run(rgbd_stores, crit, 2, None)
    hist_a = a.run()
    assert len(hist_a) == 2 and hist_a[0] == first[0]
    assert all(r["steps"] == 2 and r["nonfinite"] == 0 and np.isfinite(r["train_loss"]) for r in hist_a)
    assert os.path.exists(os.path.join(d, CKPT_LAST))
    b = _fit_run(rgbd_stores, crit, 2, d)
    assert b.start_epoch == 1 and b.history == first and b.lines[-1].startswith("Resumed at epoch 1")
    hist_b = b.run()
    assert hist_b == hist_a
    for i, (x, y) in enumerate(zip(_train_state(b.trainer), _train_state(a.trainer))):
        assert torch.equal(x, y), i
    assert b.scheduler.lr == a.scheduler.lr and float(b.trainer.hp[0]) == float(a.trainer.hp[0])
    last = torch.load(os.path.join(d, CKPT_LAST), weights_only=False)
    assert last["epoch"] == 1
    assert os.path.exists(os.path.join(d, CKPT_BEST)) == (max(r["val_acc"] for r in hist_a) > 0.0)


@pytest.mark.gpu
def test_resume_from_a_reference_checkpoint(rgbd_stores, crit, one_epoch, tmp_path):
    """Without `pose6d_resume` / `scheduler_state_dict` (what the reference's script writes):
    epoch + 1, fresh random streams, the lr of the optimizer state."""
    from pose6d.fit import CKPT_LAST
    d, first = one_epoch
    ckpt = torch.load(os.path.join(d, CKPT_LAST), weights_only=False)
    del ckpt["pose6d_resume"], ckpt["scheduler_state_dict"]
    assert set(ckpt) == {"epoch", "model_state_dict", "optimizer_state_dict", "best_acc", "curr_acc"}
    ckpt["optimizer_state_dict"]["param_groups"][0]["lr"] = 2.5e-5
    torch.save(ckpt, str(tmp_path / CKPT_LAST))
    f = _fit_run(rgbd_stores, crit, 2, str(tmp_path))
    lr = float(torch.tensor(2.5e-5, dtype=torch.float32))
    assert f.start_epoch == 1 and f.history == [] and f.best_acc == ckpt["best_acc"]
    assert float(f.trainer.hp[0]) == lr and f.scheduler.lr == lr
    assert f.augment.calls == 2                      # a fresh TrainAugment: only the first plan drew from it
    hist = f.run()
    assert [r["epoch"] for r in hist] == [1] and hist[0]["lr"] == lr and np.isfinite(hist[0]["train_loss"])


@pytest.mark.gpu
def test_checkpoint_interchange(one_epoch):
    """last_pose_model.pth is the reference's file: torch.load reads it, its five keys are there,
    the drop-in model and a real torch AdamW load its state dicts."""
    from models.pose_net_rgbd_geometric import PoseNetRGBDGeometric
    from pose6d.fit import CKPT_LAST
    d, first = one_epoch
    ckpt = torch.load(os.path.join(d, CKPT_LAST), map_location="cpu", weights_only=False)
    assert {"epoch", "model_state_dict", "optimizer_state_dict", "best_acc", "curr_acc"} <= set(ckpt)
    assert ckpt["epoch"] == 0 and ckpt["curr_acc"] == first[0]["val_acc"] and ckpt["best_acc"] == 0.0
    warnings.simplefilter("ignore")
    model = PoseNetRGBDGeometric(pretrained=False)
    assert not model.load_state_dict(ckpt["model_state_dict"]).missing_keys
    opt = torch.optim.AdamW(model.parameters())
    opt.load_state_dict(ckpt["optimizer_state_dict"])
    assert opt.param_groups[0]["lr"] == float(torch.tensor(1e-4, dtype=torch.float32))
    steps = {float(s["step"]) for s in opt.state.values()}
    assert steps == {2.0} and len(opt.state) == len(list(model.parameters()))
    res = ckpt["pose6d_resume"]
    assert res["augment_calls"] == 2 and len(res["history"]) == 1 and res["history"][0] == first[0]


@pytest.mark.gpu
def test_train_tool_writes_both_checkpoints(tree, mesh_dir, tmp_path):
    env = dict(os.environ, POSE6D_ALLOW_RANDOM_INIT="1")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "train.py"), "--model", "rgbd_geometric",
                        "--epochs", "1", "--batch", "4", "--data-root", tree, "--mesh-dir", mesh_dir, "--save-dir",
                        str(tmp_path / "w"), "--seed", "0"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "  Loss: " in r.stdout and "Training complete." in r.stdout
    last = tmp_path / "w" / "last_pose_model.pth"
    assert last.exists()
    ckpt = torch.load(str(last), map_location="cpu", weights_only=False)
    assert ckpt["epoch"] == 0
    # best_pose_model.pth is written on a strict improvement over 0 % (the script's rule)
    assert (tmp_path / "w" / "best_pose_model.pth").exists() == (ckpt["curr_acc"] > 0.0)
