"""pose6d.train.RGBTrainer: the whole PoseNetRGB training step (forward + PoseLoss(1, 10,
geodesic) + backward + clip_grad_norm_(1.0) + AdamW, train_rgb.py:95-141) as one captured
chain.  B = 4 at 224^2 (the trunk engine's input size); Dropout modules in eval unless a
test says otherwise (their RNG differs from torch's by construction)."""
import io
import warnings

import numpy as np
import pytest
import torch

from oracle import pose_loss as OP
from oracle import resnet as OR

pytestmark = pytest.mark.gpu

B = 4


def _data(seed=2024, batch=B):
    from bench import synth_batch
    d = synth_batch(batch, torch.device("cuda"), seed=seed)
    return (d[0], d[4], d[5])                                  # rgb, gt_rot, gt_trans


def _make(dtype, dropout=False, seed=0):
    from models.pose_net_rgb import PoseNetRGB
    from pose6d.train import RGBTrainer
    warnings.simplefilter("ignore")
    torch.manual_seed(seed)
    m = PoseNetRGB(pretrained=False)
    P0 = {k: v.clone() for k, v in m.state_dict().items()}
    tr = RGBTrainer(m.cuda(), B, dtype=dtype)                   # (puts the model in train mode)
    if not dropout:
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.eval()
    return tr, P0


def _bufs(tr):
    return [b for n, b in tr.model.named_buffers() if "running" in n or "num_batches" in n]


def _state(tr):
    return [t.clone() for t in (tr.arena.flat, tr.m, tr.v, tr.hp, tr.loss, *_bufs(tr))]


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def _frob(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def _oracle_step(P0, data, dtype):
    rgb, gr, gt = (t.cpu().to(dtype) for t in data)
    P = {k: (v.clone().to(dtype).requires_grad_(True) if v.is_floating_point() and "running" not in k
             else (v.clone().to(dtype) if v.is_floating_point() else v.clone())) for k, v in P0.items()}
    rot, trans = OR.forward_rgb(P, rgb, training=True)
    loss = OP.pose_loss(rot, trans, gr, gt, 1.0, 10.0)
    loss.backward()
    return rot.detach(), trans.detach(), loss.detach(), P


def _check_adamw(tr, before):
    """The fused clip-norm + AdamW against torch on our own gradients."""
    params = [torch.nn.Parameter(before[o:o + p.numel()].view_as(p).clone())
              for p, o in zip(tr.arena.params, tr.arena.offsets)]
    for q, p, o in zip(params, tr.arena.params, tr.arena.offsets):
        q.grad = tr.arena.grad[o:o + p.numel()].view_as(p).clone()
    torch.nn.utils.clip_grad_norm_(params, 1.0)
    torch.optim.AdamW(params, lr=1e-4, weight_decay=1e-4).step()
    for q, p in zip(params, tr.arena.params):
        np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().cpu().numpy(), rtol=1e-6, atol=1e-9)


def test_arena_order_and_engines():
    tr, _ = _make(torch.bfloat16)
    m = tr.model
    n_rot, n_trans = len(list(m.rot_head.parameters())), len(list(m.trans_head.parameters()))
    ids = [id(p) for p in tr.arena.params]
    assert set(ids[:n_rot]) == {id(p) for p in m.rot_head.parameters()}
    assert set(ids[n_rot:n_rot + n_trans]) == {id(p) for p in m.trans_head.parameters()}
    assert set(ids[n_rot + n_trans:]) == {id(p) for p in m.backbone.parameters()}
    assert len(ids) == len(set(ids)) == len(list(m.parameters()))
    assert tr.head.seq is m.rot_head and tr.trans_head.seq is m.trans_head


def test_fp32_step_against_oracle():
    """The replayed fp32 step against oracle.resnet.forward_rgb(training=True) +
    oracle.pose_loss.pose_loss(1, 10), judged against a float64 run of the oracle (the scheme
    of test_configs2_trainer_bs32_fp32_end_to_end), then the fused clip + AdamW against torch."""
    tr, P0 = _make(torch.float32)
    data = _data()
    snap = tr.snapshot()
    tr.capture(data, warmup=1)
    tr.restore(snap)
    before = tr.arena.flat.clone()
    tr.step()
    torch.cuda.synchronize()
    r32, t32, L32, P32 = _oracle_step(P0, data, torch.float32)
    r64, t64, L64, P64 = _oracle_step(P0, data, torch.float64)

    def check(ours, ref32, ref64, what):
        e, e_ref = _rel(ours, ref64), _rel(ref32, ref64)
        print(f"{what}: ours {e:.2e} vs exact, reference fp32 {e_ref:.2e}")
        assert e <= max(1e-4, 3 * e_ref), f"{what}: ours {e:.2e} vs exact, reference fp32 {e_ref:.2e}"

    check(tr.rot, r32, r64, "rotation")
    check(tr.trans, t32, t64, "translation")
    check(tr.loss, L32, L64, "loss")
    named = dict(tr.model.named_parameters())
    ours, ref = [], []
    for k, v in P64.items():
        if isinstance(v, torch.Tensor) and v.grad is not None:
            ours.append(_frob(tr.arena.grad_of(named[k]), v.grad))
            ref.append(_frob(P32[k].grad, v.grad))
    assert len(ours) == len(named)
    ours, ref = np.array(ours), np.array(ref)
    print("gradient Frobenius errors: ours median %.2e max %.2e, reference fp32 median %.2e max %.2e"
          % (np.median(ours), ours.max(), np.median(ref), ref.max()))
    assert np.median(ours) <= 2 * np.median(ref) + 1e-5, (np.median(ours), np.median(ref))
    assert ours.max() <= 3 * ref.max() + 1e-5, (ours.max(), ref.max())
    sd = tr.model.state_dict()
    for k in P0:
        if "running" in k:
            check(sd[k], P32[k], P64[k], k)
        elif "num_batches" in k:
            assert int(sd[k]) == int(P32[k]), k
    _check_adamw(tr, before)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_graph_replay_equals_eager(dtype):
    tr, _ = _make(dtype)
    data = _data()
    snap = tr.snapshot()
    tr.capture(data, warmup=1)
    assert len(tr.graphs) == 1
    tr.restore(snap)
    step0, seed0 = float(tr.hp[5]), int(tr.seed)
    for i in (1, 2):
        tr.step()
        torch.cuda.synchronize()
        assert float(tr.hp[5]) == step0 + i and int(tr.seed) == seed0 + i
    replayed = _state(tr)
    tr.restore(snap)
    for _ in range(2):
        tr.step_eager(data)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.loss))
    for a, b in zip(replayed, _state(tr)):
        assert torch.equal(a, b)
    assert not torch.equal(replayed[0], snap[0])


def test_dropout_on_bf16_is_reproducible():
    data = _data()
    flats = []
    for _ in range(2):
        tr, _ = _make(torch.bfloat16, dropout=True, seed=5)
        tr.capture(data, warmup=1)
        for _ in range(2):
            tr.step()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(tr.loss))
        for eng in (tr.head, tr.trans_head):                  # the dropout did run in both heads
            assert bool((eng.stages[1].mask == 0).any()) and bool((eng.stages[1].mask == 1).any())
        flats.append(tr.arena.flat.clone())
    assert torch.equal(flats[0], flats[1])


def test_checkpoint_round_trip():
    from models.pose_net_rgb import PoseNetRGB
    from pose6d.train import RGBTrainer
    tr, _ = _make(torch.bfloat16)
    data = _data()
    tr.step(data)
    ck = tr.checkpoint(epoch=3)
    buf = io.BytesIO()
    torch.save(ck, buf)
    buf.seek(0)
    ck = torch.load(buf, weights_only=True)
    assert list(ck["model_state_dict"].keys()) == list(PoseNetRGB(pretrained=False).state_dict().keys())
    m2 = PoseNetRGB(pretrained=False).cuda()
    tr2 = RGBTrainer(m2, B, dtype=torch.bfloat16)
    for mod in m2.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.eval()
    assert tr2.load_checkpoint(ck) == 4
    opt = torch.optim.AdamW(m2.parameters(), lr=1e-4, weight_decay=1e-4)
    opt.load_state_dict(ck["optimizer_state_dict"])
    assert all(float(opt.state[p]["step"]) == 1.0 for p in m2.parameters())
    for t in (tr, tr2):
        t.step(data)
    torch.cuda.synchronize()
    for a, b in zip(_state(tr), _state(tr2)):
        assert torch.equal(a, b)


def test_eval_after_training_reads_the_updated_weights():
    from models.pose_net_rgb import PoseNetRGB
    dtype = torch.bfloat16
    tr, _ = _make(dtype)
    data = _data()
    tr.capture(data, warmup=1)
    tr.step()
    torch.cuda.synchronize()
    x = _data(seed=9, batch=2)[0]
    model = tr.model.set_compute_dtype(dtype).eval()
    fresh = PoseNetRGB(pretrained=False).cuda().set_compute_dtype(dtype)
    fresh.load_state_dict(model.state_dict())
    fresh.eval()
    with torch.no_grad():
        rot, trans = model(x)
        rot2, trans2 = fresh(x)
    assert bool(torch.isfinite(rot).all()) and bool(torch.isfinite(trans).all())
    assert torch.equal(rot, rot2) and torch.equal(trans, trans2)


# kernel nodes in RGBDGeometricTrainer's captured one-GPU step (B = 4, bf16, pack_in_adamw),
# counted once with pose6d.steptime.StepTimer on the commit before RGBTrainer existed
RGBD_GEOMETRIC_KERNEL_NODES = 330


def test_rgbd_geometric_trainer_untouched():
    from bench import synth_batch
    from models.pose_net_rgbd_geometric import PoseNetRGBDGeometric
    from pose6d import steptime as ST
    from pose6d.train import RGBDGeometricTrainer
    warnings.simplefilter("ignore")
    torch.manual_seed(0)
    m = PoseNetRGBDGeometric(pretrained=False).cuda()
    tr = RGBDGeometricTrainer(m, B, dtype=torch.bfloat16)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.eval()
    data = synth_batch(B, torch.device("cuda"), seed=2024)
    snap = tr.snapshot()
    tr.step_eager(data)
    torch.cuda.synchronize()
    eager = tr.arena.flat.clone()
    tr.restore(snap)
    tr.capture(data, warmup=1)
    tr.restore(snap)
    tr.step()
    torch.cuda.synchronize()
    assert torch.equal(tr.arena.flat, eager)
    timer = ST.StepTimer(lambda: tr.step_body(data), torch.device("cuda"))
    nodes = sum(r["type"] == 0 for r in timer.records)
    timer.close()
    assert nodes == RGBD_GEOMETRIC_KERNEL_NODES, nodes
