"""pose6d.validate: the validation pass of the reference's epoch (train_rgbd_geometric.py:
119-146) on the whole-step trainers' own engines -- pose6d_val_append, the trainers'
_forward_eval, Validator (eager and captured, short last batch, overflow, mesh change, two
ranks) and PlateauLR.  GPU tests run at the trainers' test size: B = 4 at 224^2,
pretrained=False, meshes from tests.synth.write_mesh_dir (500 points kept).

Every comparison of predictions and metrics is exact (torch.equal / ==): the eval forward's
sub-paths are each documented bit-identical to the drop-in module's (packed weights:
tests/test_adamw_packed.py; fused eval epilogues and pose6d_gemm_f32_bn_eval: tests/
test_inference.py), and the epoch table stores doubles as they are."""
import os
import subprocess
import sys
import tempfile
import warnings

import numpy as np
import pytest
import torch

from tests.synth import write_mesh_dir

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 4
KEYS = ("add_mean", "add_s_mean", "add_01d_acc")


# ------------------------------------------------------------------ CPU: merge_rank_tables
def _rows(rng, n, n_valid):
    """n table rows, the first n_valid valid (random add / adds / correct), the rest what the
    ADD kernels write for an unknown object: zeros."""
    t = np.zeros((n, 4))
    t[:n_valid, 0] = rng.random(n_valid)
    t[:n_valid, 1] = rng.random(n_valid) * 0.5
    t[:n_valid, 2] = 1.0
    t[:n_valid, 3] = rng.integers(0, 2, n_valid)
    return t


def test_merge_rank_tables_regroups_by_global_batch():
    from models.add_loss import ADDLoss
    from pose6d.validate import merge_rank_tables
    rng = np.random.default_rng(3)
    # 2 ranks x 3 batches x B = 4; rank 0's last batch half invalid, rank 1's all invalid
    per_rank = [[_rows(rng, 4, 4), _rows(rng, 4, 4), _rows(rng, 4, 2)],
                [_rows(rng, 4, 4), _rows(rng, 4, 4), _rows(rng, 4, 0)]]
    tables = [torch.from_numpy(np.concatenate(r)) for r in per_rank]
    merged = merge_rank_tables(tables, 4)
    assert merged.shape == (24, 4) and merged.dtype == torch.float64
    for k in range(3):
        want = np.concatenate([per_rank[0][k], per_rank[1][k]])           # rank order within a batch
        got = merged[8 * k:8 * k + 8]
        assert np.array_equal(got.numpy(), want), k
        a = ADDLoss.aggregate(*(got[:, c] for c in range(4)))
        b = ADDLoss.aggregate(*(torch.from_numpy(want[:, c].copy()) for c in range(4)))
        assert a == b and set(a) == set(KEYS)
    last = ADDLoss.aggregate(*(merged[16:, c] for c in range(4)))
    assert last["add_mean"] == np.mean(per_rank[0][2][:2, 0].tolist()) * 1000     # two valid rows of eight
    one = merge_rank_tables([tables[0]], 4)                                     # one rank: unchanged
    assert torch.equal(one, tables[0])


def test_merge_rank_tables_rejects_ragged_tables():
    from pose6d import Pose6dError
    from pose6d.validate import merge_rank_tables
    with pytest.raises(Pose6dError):
        merge_rank_tables([torch.zeros(8, 4), torch.zeros(4, 4)], 4)
    with pytest.raises(Pose6dError):
        merge_rank_tables([torch.zeros(6, 4)], 4)


# ------------------------------------------------------------------ CPU: PlateauLR on a stub
class _Stub:
    def __init__(self, lr):
        self.hp = [lr]
        self.calls = []

    def set_lr(self, lr):
        self.calls.append(lr)


# mode 'max', patience 2: a rise, three flat epochs (-> halve), a rise, three flat (-> halve,
# clamped by min_lr = 3e-5), then flat for good (already at the clamp: no further change)
_METRICS = [10.0, 20.0, 20.0, 20.0, 20.0, 30.0, 30.0, 30.0, 30.0, 30.0, 30.0, 30.0, 30.0, 30.0]
_PLATEAU = dict(mode="max", factor=0.5, patience=2, min_lr=3e-5)


def _torch_trajectory(lr):
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([p], lr=lr)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, **_PLATEAU)
    out = []
    for m in _METRICS:
        sched.step(m)
        out.append(opt.param_groups[0]["lr"])
    return out


def test_plateau_lr_follows_torch_on_a_stub_trainer():
    from pose6d.validate import PlateauLR
    lr0 = 1e-4
    want = _torch_trajectory(lr0)
    assert sorted(set(want), reverse=True) == [1e-4, 5e-5, 3e-5]               # two plateaus, the second clamped
    stub = _Stub(lr0)
    sched = PlateauLR(stub, **_PLATEAU)
    assert sched.lr == lr0
    got = [sched.step(m) for m in _METRICS]
    assert got == want and sched.lr == want[-1]
    changes = [b for a, b in zip([lr0] + want[:-1], want) if b != a]
    assert stub.calls == changes == [5e-5, 3e-5]
    # state_dict round trip in the middle of the first plateau (two bad epochs counted)
    cut = 4
    first = PlateauLR(_Stub(lr0), **_PLATEAU)
    for m in _METRICS[:cut]:
        first.step(m)
    sd = first.state_dict()
    assert sd["num_bad_epochs"] == 2
    stub2 = _Stub(lr0)
    second = PlateauLR(stub2, **_PLATEAU)
    second.load_state_dict(sd)
    assert [second.step(m) for m in _METRICS[cut:]] == want[cut:]
    assert stub2.calls == [5e-5, 3e-5]
    # ... and after the first reduction: the loaded lr reaches the trainer
    cut = 6
    for m in _METRICS[cut - 2:cut]:
        first.step(m)
    assert first.lr == 5e-5
    stub3 = _Stub(lr0)
    third = PlateauLR(stub3, **_PLATEAU)
    third.load_state_dict(first.state_dict())
    assert third.lr == 5e-5 and stub3.calls == [5e-5]
    assert [third.step(m) for m in _METRICS[cut:]] == want[cut:]


def test_val_append_arguments_checked_without_gpu():
    from pose6d import _lib
    lib = _lib.load()
    buf = (torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64),
           torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int32))
    table, state = torch.zeros(8, 4, dtype=torch.float64), torch.zeros(2, dtype=torch.int64)
    p = [t.data_ptr() for t in buf]
    for args in ((*p, -1, table.data_ptr(), 8, state.data_ptr(), None),
                 (*p, 65536, table.data_ptr(), 8, state.data_ptr(), None),
                 (*p, 4, table.data_ptr(), -1, state.data_ptr(), None),
                 (*p, 4, None, 8, state.data_ptr(), None),
                 (*p, 4, table.data_ptr(), 8, None, None)):
        assert lib.pose6d_val_append(*args) == 1
        assert b"pose6d_val_append" in lib.pose6d_last_error()
    assert lib.pose6d_val_append(None, None, None, None, 0, None, 8, None, None) == 0   # B == 0: nothing to do


def test_shared_camera_matrix_is_told_from_a_batch_of_three():
    """A (3, 3) camera matrix has no batch dimension; the ground-truth translation of a short
    batch of 3 samples is (3, 3) too and sits at the tuple's end."""
    from pose6d.validate import Validator
    data = (torch.zeros(3, 3, 224, 224), torch.zeros(3, 2), torch.zeros(3, 3), torch.zeros(3, 4), torch.zeros(3, 3))
    assert [Validator._shared(t, i >= len(data) - 2) for i, t in enumerate(data)] == [False, False, True, False, False]
    batched = (torch.zeros(3, 3, 224, 224), torch.zeros(3, 2), torch.zeros(3, 3, 3), torch.zeros(3, 4), torch.zeros(3, 3))
    assert not any(Validator._shared(t, i >= len(batched) - 2) for i, t in enumerate(batched))


# ------------------------------------------------------------------ GPU helpers
def _cfg(kind):
    """(model class, trainer class, synth_batch -> training tuple, training tuple -> model args)"""
    from pose6d import train
    if kind == "rgbd_geometric":
        from models.pose_net_rgbd_geometric import PoseNetRGBDGeometric as M
        return (M, train.RGBDGeometricTrainer, lambda d: (d[0], d[1], d[2], d[3], d[4], d[5]),
                lambda t: (t[0], None, t[1], t[2], t[3]))
    if kind == "rgb":
        from models.pose_net_rgb import PoseNetRGB as M
        return M, train.RGBTrainer, lambda d: (d[0], d[4], d[5]), lambda t: (t[0],)
    if kind == "rgb_geometric":
        from models.pose_net_rgb_geometric import PoseNetRGBGeometric as M
        return (M, train.RGBGeometricTrainer, lambda d: (d[0], d[2], d[3], d[4], d[5]),
                lambda t: (t[0], t[1], t[2]))
    from models.pose_net_rgbd import PoseNetRGBD as M
    return M, train.RGBDTrainer, lambda d: (d[0], d[1].unsqueeze(1), d[4], d[5]), lambda t: (t[0], t[1])


def _data(kind, seed, n=B):
    from bench import synth_batch
    return _cfg(kind)[2](synth_batch(n, torch.device("cuda"), seed=seed))


def _make(kind, dtype, seed=0, dropout=False, **kw):
    """A trainer on the torch.manual_seed(seed) model, after ONE replayed step from its
    initial state (the packed weights were written by the AdamW launch)."""
    M, T = _cfg(kind)[:2]
    warnings.simplefilter("ignore")
    torch.manual_seed(seed)
    tr = T(M(pretrained=False).cuda(), B, dtype=dtype, **kw)
    if not dropout:
        for mod in tr.model.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.eval()
    snap = tr.snapshot()
    tr.train_data = _data(kind, 2024)                # kept alive: the captured step reads these tensors
    tr.capture(tr.train_data, warmup=1)
    tr.restore(snap)
    tr.step()
    torch.cuda.synchronize()
    return tr


def _fresh_predictions(kind, tr, dtype, data):
    """The drop-in module's eval forward: a fresh model loaded from the trainer's state_dict."""
    M, _, _, args = _cfg(kind)
    fresh = M(pretrained=False).cuda().set_compute_dtype(dtype)
    fresh.load_state_dict(tr.model.state_dict())
    fresh.eval()
    with torch.no_grad():
        rot, trans = fresh(*args(data))
    return rot.clone(), trans.clone()


def _bufs(tr):
    return [b for n, b in tr.model.named_buffers() if "running" in n or "num_batches" in n]


def _train_state(tr):
    return [t.clone() for t in (tr.arena.flat, tr.m, tr.v, tr.hp, tr.seed, *_bufs(tr))]


@pytest.fixture(scope="module")
def mesh_dir():
    d = tempfile.mkdtemp()
    write_mesh_dir(d, n_vertices=700, seed=11)
    return d


def _crit(mesh_dir):
    from models.add_loss import ADDLoss
    np.random.seed(1234)
    return ADDLoss(mesh_dir, "cuda")


@pytest.fixture(scope="module")
def crit(mesh_dir):
    """Shared and never modified (the mesh-change test builds its own)."""
    return _crit(mesh_dir)


@pytest.fixture(scope="module")
def geo():
    """One RGBDGeometricTrainer (bf16) after a replayed step, shared by the tests that only
    validate on it: validation leaves the training state alone (tested below)."""
    return _make("rgbd_geometric", torch.bfloat16)


# three batches of 4, 4 and a short 2; a symmetric object (9, 10), the 6-point mesh (13) and
# ids without a mesh (2, 6) among them: 8 known samples
_IDS = ([9, 13, 2, 0], [10, 1, 6, 4], [9, 5])
_KNOWN = 8


def _epoch_batches(val, tr, kind="rgbd_geometric", seeds=(31, 32, 33), ids=_IDS):
    """[(training tuple, obj_ids)] whose ground truth is built from the model's OWN eval
    predictions (one eager pass through `val`): a tiny offset on the even rows (correct under
    the 0.1 d test), a rotation change and a 0.2 m offset on the odd rows (not correct)."""
    out = []
    val.begin()
    for seed, oid in zip(seeds, ids):
        n = len(oid)
        data = list(_data(kind, seed, n))
        oid = torch.tensor(oid, dtype=torch.int64, device="cuda")
        val.batch(data, oid)
        rot, trans = tr.rot[:n].clone(), tr.trans[:n].clone()
        gt_rot, gt_trans = rot.clone(), trans + 1e-4
        g = torch.Generator().manual_seed(seed)
        far = torch.nn.functional.normalize(rot[1::2] + 0.3 * torch.randn(rot[1::2].shape, generator=g).cuda(), dim=1)
        gt_rot[1::2] = far
        gt_trans[1::2] += 0.2
        data[-2], data[-1] = gt_rot, gt_trans
        out.append((tuple(data), oid, rot, trans))
    val.finish()
    return out


def _reference_loop(crit, batches):
    """The reference's validation loop written out (train_rgbd_geometric.py:121-144) on the
    given predictions: eval_metrics per batch, sum, / batches."""
    sums = {k: 0.0 for k in KEYS}
    for data, oid, rot, trans in batches:
        m = crit.eval_metrics(rot, trans, data[-2], data[-1], oid)
        for k in KEYS:
            sums[k] += m[k]
    return {k: sums[k] / len(batches) for k in KEYS}


# ------------------------------------------------------------------ GPU: the kernel alone
@pytest.mark.gpu
def test_val_append_kernel():
    from pose6d import _lib
    from pose6d._lib import call, stream
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(5)
    n, cap, fill = 5, 12, -7.0
    batches = []
    for valid, correct in (([1, 0, 1, 1, 0], [1, 0, 0, 1, 0]), ([0, 1, 1, 0, 1], [0, 0, 1, 0, 1]),
                           ([1, 1, 1, 1, 1], [1, 1, 1, 1, 1])):
        batches.append((torch.rand(n, generator=g, dtype=torch.float64).to(dev),
                        (torch.rand(n, generator=g, dtype=torch.float64) / 3).to(dev),
                        torch.tensor(valid, dtype=torch.int32, device=dev),
                        torch.tensor(correct, dtype=torch.int32, device=dev)))
    table = torch.full((cap, 4), fill, dtype=torch.float64, device=dev)
    state = torch.zeros(2, dtype=torch.int64, device=dev)
    rows = lambda b: torch.stack([b[0], b[1], b[2].double(), b[3].double()], dim=1)
    for b in batches[:2]:
        call("val_append", *b, n, table, cap, state, stream())
    torch.cuda.synchronize()
    assert torch.equal(table[:5], rows(batches[0])) and torch.equal(table[5:10], rows(batches[1]))
    assert bool((table[10:] == fill).all())
    assert state.tolist() == [10, 0]
    before = table.clone()
    call("val_append", *batches[2], n, table, cap, state, stream())     # rows 10 .. 14 do not fit 12
    torch.cuda.synchronize()
    assert torch.equal(table, before) and state.tolist() == [10, 1]
    call("val_append", None, None, None, None, 0, None, cap, None, stream())   # B == 0: a no-op
    torch.cuda.synchronize()
    assert torch.equal(table, before) and state.tolist() == [10, 1]
    lib = _lib.load()
    for bad_B, tab in ((-1, table), (65536, table), (n, None)):
        with pytest.raises(_lib.Pose6dError, match="pose6d_val_append"):
            call("val_append", *batches[0], bad_B, tab, cap, state, stream())
        assert b"pose6d_val_append" in lib.pose6d_last_error()
    torch.cuda.synchronize()
    assert torch.equal(table, before) and state.tolist() == [10, 1]


# ------------------------------------------------------------------ GPU: predictions
@pytest.mark.gpu
@pytest.mark.parametrize("kind,dtype", [("rgbd_geometric", torch.bfloat16), ("rgb", torch.bfloat16),
                                        ("rgb_geometric", torch.bfloat16), ("rgbd", torch.bfloat16),
                                        ("rgbd_geometric", torch.float32)],
                         ids=["rgbd_geometric-bf16", "rgb-bf16", "rgb_geometric-bf16", "rgbd-bf16",
                              "rgbd_geometric-fp32"])
def test_predictions_equal_the_drop_in_eval_forward(kind, dtype, crit):
    from pose6d.validate import Validator
    tr = _make(kind, dtype)
    data = _data(kind, 9)
    val = Validator(tr, crit)
    val.begin()
    val.batch(data, torch.tensor([0, 1, 9, 13]))
    rot, trans = tr.rot.clone(), tr.trans.clone()
    m = val.finish()
    assert m["batches"] == 1 and m["samples"] == 4
    rot2, trans2 = _fresh_predictions(kind, tr, dtype, data)
    assert bool(torch.isfinite(rot).all()) and bool(torch.isfinite(trans).all())
    assert rot.shape == (B, 4) and trans.shape == (B, 3)
    assert torch.equal(rot, rot2), (rot - rot2).abs().max().item()
    assert torch.equal(trans, trans2), (trans - trans2).abs().max().item()


# ------------------------------------------------------------------ GPU: metrics
@pytest.mark.gpu
def test_metrics_equal_the_reference_loop_eager_and_captured(geo, crit):
    from pose6d.validate import Validator
    tr = geo
    val = Validator(tr, crit)
    batches = _epoch_batches(val, tr)
    # the 0.1 d test must see both outcomes, or add_01d_acc compares 0 with 0
    correct = []
    for data, oid, rot, trans in batches:
        s = crit.per_sample(rot, trans, data[-2], data[-1], oid)
        correct += s["correct"][s["valid"] > 0].tolist()
    assert len(correct) == _KNOWN and 0 < sum(correct) < _KNOWN, correct
    want = _reference_loop(crit, batches)
    assert 0 < want["add_01d_acc"] < 100 and want["add_mean"] > 0 and want["add_s_mean"] > 0

    def epoch(v):
        v.begin()
        for i, (data, oid, rot, trans) in enumerate(batches):
            v.batch(data, oid)
            n = len(oid)
            assert torch.equal(tr.rot[:n], rot) and torch.equal(tr.trans[:n], trans), i
        return v.finish()

    eager = epoch(val)
    print("reference loop", want, "validator", eager)
    for k in KEYS:
        assert eager[k] == want[k], (k, eager[k], want[k])
    assert eager["batches"] == 3 and eager["samples"] == _KNOWN
    cap = Validator(tr, crit)
    cap.capture(batches[0][0], batches[0][1])
    assert cap.graph is not None
    captured = epoch(cap)
    assert captured == eager
    assert epoch(cap) == eager                       # a second epoch on the same graph
    empty = Validator(tr, crit)
    empty.begin()
    assert empty.finish() == {"add_mean": 0, "add_s_mean": 0, "add_01d_acc": 0, "batches": 0, "samples": 0}


# ------------------------------------------------------------------ GPU: stale weights
@pytest.mark.gpu
def test_second_epoch_reads_the_current_weights(crit):
    """step, validate, step, validate: the trainer's AdamW launch writes the fp32 masters
    through raw pointers, which no version counter sees; the second validation must still
    run on the weights of the second step."""
    from pose6d.validate import Validator
    kind, dtype = "rgbd_geometric", torch.bfloat16
    tr = _make(kind, dtype)                          # (the first step)
    data = _data(kind, 9)
    oid = torch.tensor([0, 1, 9, 13])
    val = Validator(tr, crit)
    val.capture(data, oid)
    preds = []
    for epoch in range(2):
        if epoch:
            tr.step()
        val.begin()
        val.batch(data, oid)
        preds.append((tr.rot.clone(), tr.trans.clone()))
        val.finish()
        rot2, trans2 = _fresh_predictions(kind, tr, dtype, data)
        assert torch.equal(preds[-1][0], rot2) and torch.equal(preds[-1][1], trans2), epoch
    assert not torch.equal(preds[0][0], preds[1][0])  # the second step did move the weights


# ------------------------------------------------------------------ GPU: training untouched
@pytest.mark.gpu
def test_validation_leaves_training_alone(crit):
    from pose6d.validate import Validator
    kind, dtype = "rgbd", torch.bfloat16             # heads, fusion MLP and attention all have dropout
    a = _make(kind, dtype, seed=5, dropout=True)
    b = _make(kind, dtype, seed=5, dropout=True)
    for tr in (a, b):
        tr.model.rot_head[3].eval()                  # mixed flags: one Dropout off
    flags = [m.training for m in a.model.modules()]
    assert any(flags) and not all(flags)
    val = Validator(a, crit)
    d1, d2 = _data(kind, 41), _data(kind, 42, 2)
    val.capture(d1, torch.tensor([0, 1, 9, 13]))
    val.begin()
    val.batch(d1, torch.tensor([0, 1, 9, 13]))
    val.batch(d2, torch.tensor([10, 2]))
    m = val.finish()
    assert m["batches"] == 2 and m["samples"] == 5
    assert [mod.training for mod in a.model.modules()] == flags
    for tr in (a, b):
        tr.step()
    torch.cuda.synchronize()
    for x, y in zip(_train_state(a), _train_state(b)):
        assert torch.equal(x, y)
    assert float(a.hp[5]) == 2.0


# ------------------------------------------------------------------ GPU: overflow
@pytest.mark.gpu
def test_table_overflow_raises(geo, crit):
    from pose6d import Pose6dError
    from pose6d.validate import Validator
    val = Validator(geo, crit, max_samples=B)
    assert val.capacity == B
    data, oid = _data("rgbd_geometric", 9), torch.tensor([0, 1, 9, 13])
    val.begin()
    val.batch(data, oid)
    val.batch(data, oid)
    with pytest.raises(Pose6dError, match="max_samples"):
        val.finish()
    assert val.state.tolist() == [B, 1]
    val.begin()                                      # the next epoch starts clean
    val.batch(data, oid)
    assert val.finish()["batches"] == 1
    assert Validator(geo, crit, max_samples=B + 1).capacity == 2 * B


# ------------------------------------------------------------------ GPU: one camera matrix for the batch
@pytest.mark.gpu
def test_shared_camera_matrix_equals_the_batched_one(geo, crit):
    """A (3, 3) camera matrix (the trainers accept both forms) through a short batch of 3,
    where the ground-truth translation is (3, 3) as well."""
    from pose6d.validate import Validator
    rgb, depth_raw, bbox, K, gt_rot, gt_trans = _data("rgbd_geometric", 61, 3)
    oid = torch.tensor([0, 9, 13])
    out = []
    for cam in (K[0].contiguous(), K[:1].expand(3, 3, 3).contiguous()):
        val = Validator(geo, crit)
        val.begin()
        val.batch((rgb, depth_raw, bbox, cam, gt_rot, gt_trans), oid)
        out.append((geo.rot[:3].clone(), geo.trans[:3].clone(), val.finish()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2] and out[0][2]["samples"] == 3
    assert not torch.equal(out[0][1][0], out[0][1][1])       # the translations do depend on the sample


# ------------------------------------------------------------------ GPU: mesh table change
@pytest.mark.gpu
def test_mesh_change_recaptures(geo, mesh_dir):
    from pose6d.validate import Validator
    tr, own = geo, _crit(mesh_dir)
    val = Validator(tr, own)
    (data, oid, rot, trans), = _epoch_batches(val, tr, seeds=(51,), ids=([1, 0, 9, 0],))
    val.capture(data, oid)
    g0 = val.graph

    def epoch():
        val.begin()
        val.batch(data, oid)
        return val.finish()

    m0 = epoch()
    assert val.graph is g0 and {k: m0[k] for k in KEYS} == _reference_loop(own, [(data, oid, rot, trans)])
    own.points[0] = (own.points[0] * 3.0).contiguous()      # object 0 three times as large
    m1 = epoch()
    assert val.graph is not g0, "the graph still holds the old mesh table's pointers"
    assert {k: m1[k] for k in KEYS} == _reference_loop(own, [(data, oid, rot, trans)])
    assert m1["add_mean"] > m0["add_mean"]                   # rows 1 and 3 are rotated: ADD grows with the mesh


# ------------------------------------------------------------------ GPU: PlateauLR
@pytest.mark.gpu
def test_plateau_lr_drives_the_captured_step():
    from pose6d.validate import PlateauLR
    kind, dtype = "rgbd_geometric", torch.bfloat16
    a, b = _make(kind, dtype), _make(kind, dtype)
    snap_a, snap_b = a.snapshot(), b.snapshot()
    lr0 = float(a.hp[0])
    a.step()
    torch.cuda.synchronize()
    at_lr0 = a.arena.flat.clone()
    a.restore(snap_a)
    sched = PlateauLR(a, mode="max", factor=0.5, patience=1)
    assert sched.lr == lr0
    for metric in (50.0, 40.0):
        assert sched.step(metric) == lr0 and float(a.hp[0]) == lr0
    assert sched.step(40.0) == lr0 / 2                       # the second epoch without improvement
    assert float(a.hp[0]) == lr0 / 2
    b.restore(snap_b)
    b.set_lr(lr0 / 2)
    for tr in (a, b):
        tr.step()
    torch.cuda.synchronize()
    for x, y in zip(_train_state(a), _train_state(b)):
        assert torch.equal(x, y)
    assert not torch.equal(a.arena.flat, at_lr0)             # the replayed step did read the new lr


# ------------------------------------------------------------------ GPU: two ranks
@pytest.mark.gpu
def test_ddp_validation_equals_global_batches(mesh_dir, crit):
    """2 gloo ranks sharing the GPU (tests/validation_ddp_worker.py): both ranks' finish()
    return the dict of eval_metrics per GLOBAL batch -- the rank-order concatenation of the
    ranks' own saved predictions -- then the mean over the three batches."""
    out = os.path.join(tempfile.mkdtemp(), "val")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", "29771",
           os.path.join(REPO, "tests", "validation_ddp_worker.py"), out, mesh_dir]
    r = subprocess.run(cmd, env=env, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "--- stdout ---\n" + r.stdout[-3000:] + "\n--- stderr ---\n" + r.stderr[-6000:]
    ranks = [torch.load(f"{out}.{k}.pt", weights_only=True) for k in range(2)]
    assert ranks[0]["metrics"] == ranks[1]["metrics"]
    assert [len(x) for x in ranks[1]["ids"]] == [4, 4, 2] and [len(x) for x in ranks[0]["ids"]] == [4, 4, 4]
    batches = []
    for k in range(3):
        cat = lambda key: torch.cat([ranks[0][key][k], ranks[1][key][k]]).cuda()
        batches.append(((cat("gt_rot"), cat("gt_trans")), cat("ids"), cat("rot"), cat("trans")))
    want = _reference_loop(crit, batches)
    got = ranks[0]["metrics"]
    print("global batches", want, "ranks", got)
    for k in KEYS:
        assert got[k] == want[k], (k, got[k], want[k])
    assert 0 < want["add_01d_acc"] < 100
    assert got["batches"] == 3
    assert got["samples"] == sum(int(i in crit.points) for r in ranks for x in r["ids"] for i in x.tolist())
