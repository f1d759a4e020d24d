"""pose6d.train.RGBGeometricTrainer: the whole PoseNetRGBGeometric training step (forward +
PoseLoss(1, 10, geodesic) + backward + clip_grad_norm_(1.0) + AdamW,
train_rgb_geometric.py:97-110) as one captured chain over two trunks.  B = 4 at 224^2 (the
trunk engines' input size); Dropout modules in eval unless a test says otherwise (their RNG
differs from torch's by construction)."""
import io
import warnings

import numpy as np
import pytest
import torch

from oracle import pose_loss as OP
from oracle import resnet as OR

pytestmark = pytest.mark.gpu

B = 4
# bench.synth_batch seed of every test here.  Checked on the CPU from the oracle alone (fp32
# and float64 runs of _oracle_step on the torch.manual_seed(0) model; seeds 2025 and 7 give
# the same picture): min |trans - gt| = 5.6e-3, so no sign of the L1 translation term is
# within 1e-4 of a rounding edge.  The fp32 oracle's own gradient error against float64
# (relative Frobenius, per parameter): z_predictor ~1e-7, z-CNN ~2e-6, rot_head 1e-4 .. 1e-3,
# ResNet50 2.7e-3 .. 2.4e-2 (train-mode BatchNorm over B = 4 is ill-conditioned), median
# over all 1.7e-2 -- so the bounds of test_fp32_step_against_oracle sit near 3.5e-2 / 7e-2,
# far below the O(1) error of a wrong gradient.  Six biases (the Linear / conv biases right
# ahead of a train-mode BatchNorm) have an exactly zero gradient: float64 gives ~1e-16,
# fp32 ~1e-7, their relative error is rounding noise over rounding noise (1e8 .. 1e9) and
# it alone decides a maximum over all parameters; the test therefore also bounds the
# maximum over the other parameters
DATA_SEED = 2024
ZERO_GRAD = 1e-9   # float64 gradient norm below which a parameter's exact gradient is zero


def _data(seed=DATA_SEED, batch=B):
    from bench import synth_batch
    d = synth_batch(batch, torch.device("cuda"), seed=seed)
    return (d[0], d[2], d[3], d[4], d[5])                      # rgb, bbox_center, K, gt_rot, gt_trans


def _make(dtype, dropout=False, seed=0, **kw):
    from models.pose_net_rgb_geometric import PoseNetRGBGeometric
    from pose6d.train import RGBGeometricTrainer
    warnings.simplefilter("ignore")
    torch.manual_seed(seed)
    m = PoseNetRGBGeometric(pretrained=False)
    P0 = {k: v.clone() for k, v in m.state_dict().items()}
    tr = RGBGeometricTrainer(m.cuda(), B, dtype=dtype, **kw)    # (puts the model in train mode)
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
    rgb, bbox, K, gr, gt = (t.cpu().to(dtype) for t in data)
    P = {k: (v.clone().to(dtype).requires_grad_(True) if v.is_floating_point() and "running" not in k
             else (v.clone().to(dtype) if v.is_floating_point() else v.clone())) for k, v in P0.items()}
    rot, trans = OR.forward_rgb_geometric(P, rgb, bbox, K, training=True)
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
    groups = [m.rot_head, m.z_predictor, m.z_backbone, m.rgb_backbone]
    ids = [id(p) for p in tr.arena.params]
    lo = 0
    for mod in groups:                                         # four contiguous groups, in this order
        n = len(list(mod.parameters()))
        assert set(ids[lo:lo + n]) == {id(p) for p in mod.parameters()}, type(mod)
        lo += n
    assert lo == len(ids) == len(set(ids)) == len(list(m.parameters()))
    # within its group each trunk keeps its own gradient-completion order
    nz = len(list(m.z_backbone.parameters()))
    nh = lo - nz - len(list(m.rgb_backbone.parameters()))
    assert ids[nh:nh + nz] == [id(p) for p in tr.z_trunk.params_in_grad_order()]
    assert ids[nh + nz:] == [id(p) for p in tr.trunk.params_in_grad_order()]
    assert tr.head.seq is m.rot_head and tr.z_head.seq is m.z_predictor
    assert tr.trunk.seq is m.rgb_backbone and tr.z_trunk.seq is m.z_backbone and tr.z_trunk.kind == "zcnn"
    assert tr.trunks == [tr.z_trunk, tr.trunk]
    assert tr.trunk.dtype == tr.z_trunk.dtype == torch.bfloat16 and tr.trunk.B == tr.z_trunk.B == B
    assert tuple(tr.dz.shape) == (B, 1)


def test_shared_input_needs_matching_buffers():
    """TrunkEngine.forward(input_from=): refuses an engine whose input buffer differs in
    dtype or shape, and one that has not run."""
    from pose6d._lib import Pose6dError
    from pose6d.trunk import TrunkEngine
    tr, _ = _make(torch.bfloat16)
    rgb = _data()[0]
    other = TrunkEngine(tr.model.z_backbone, 3, kind="zcnn")
    with pytest.raises(Pose6dError, match="input_from"):
        tr.z_trunk.forward(rgb, True, pack=False, input_from=other)          # no forward yet
    other.set_dtype(torch.float32)
    other.forward(rgb, True)
    with pytest.raises(Pose6dError, match="input_from"):
        tr.z_trunk.forward(rgb, True, pack=False, input_from=other)          # fp32 vs bf16
    other.set_dtype(torch.bfloat16)
    other.forward(rgb[:2], True)
    with pytest.raises(Pose6dError, match="input_from"):
        tr.z_trunk.forward(rgb, True, pack=False, input_from=other)          # batch 2 vs 4
    torch.cuda.synchronize()


def test_fp32_step_against_oracle():
    """The replayed fp32 step against oracle.resnet.forward_rgb_geometric(training=True) +
    oracle.pose_loss.pose_loss(1, 10), judged against a float64 run of the oracle (the scheme
    of test_rgb_trainer.test_fp32_step_against_oracle), then the fused clip + AdamW against
    torch."""
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
    margin = (t64 - data[4].cpu().double()).abs().min().item()
    print(f"min |trans - gt| = {margin:.2e}")
    assert margin >= 1e-4, "a translation sign sits on a rounding edge: pick another DATA_SEED"

    def check(ours, ref32, ref64, what):
        e, e_ref = _rel(ours, ref64), _rel(ref32, ref64)
        print(f"{what}: ours {e:.2e} vs exact, reference fp32 {e_ref:.2e}")
        assert e <= max(1e-4, 3 * e_ref), f"{what}: ours {e:.2e} vs exact, reference fp32 {e_ref:.2e}"

    check(tr.rot, r32, r64, "rotation")
    check(tr.trans, t32, t64, "translation")
    check(tr.loss, L32, L64, "loss")
    named = dict(tr.model.named_parameters())
    ours, ref, live = [], [], []
    for k, v in P64.items():
        if isinstance(v, torch.Tensor) and v.grad is not None:
            ours.append(_frob(tr.arena.grad_of(named[k]), v.grad))
            ref.append(_frob(P32[k].grad, v.grad))
            live.append(v.grad.norm().item() > ZERO_GRAD)
            if not live[-1]:
                print("exactly zero gradient %s: |g| ours %.2e, reference fp32 %.2e, float64 %.2e"
                      % (k, tr.arena.grad_of(named[k]).norm().item(), P32[k].grad.norm().item(),
                         v.grad.norm().item()))
    assert len(ours) == len(named)
    ours, ref, live = np.array(ours), np.array(ref), np.array(live)
    print("gradient Frobenius errors: ours median %.2e max %.2e, reference fp32 median %.2e max %.2e"
          % (np.median(ours), ours.max(), np.median(ref), ref.max()))
    print("  over the %d parameters with a non-zero gradient: ours max %.2e, reference fp32 max %.2e"
          % (live.sum(), ours[live].max(), ref[live].max()))
    # (the fp32 oracle's own error must leave the bounds far below a wrong gradient's O(1))
    assert np.median(ref) <= 0.05 and ref[live].max() <= 0.1, (np.median(ref), ref[live].max())
    assert np.median(ours) <= 2 * np.median(ref) + 1e-5, (np.median(ours), np.median(ref))
    assert ours.max() <= 3 * ref.max() + 1e-5, (ours.max(), ref.max())
    assert ours[live].max() <= 3 * ref[live].max() + 1e-5, (ours[live].max(), ref[live].max())
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
        for eng in (tr.head, tr.z_head):                       # the dropout did run in both heads
            assert bool((eng.stages[1].mask == 0).any()) and bool((eng.stages[1].mask == 1).any())
        flats.append(tr.arena.flat.clone())
    assert torch.equal(flats[0], flats[1])


def test_launch_shape():
    """The step's launches by entry point: one fused head + loss, one input conversion for
    the two trunks, one norm-partials and one packed AdamW launch over the whole arena, and
    none of the launches those replace."""
    from pose6d import _lib
    tr, _ = _make(torch.bfloat16)
    data = _data()
    names = []
    ob = lambda name, args: names.append(name)
    _lib.observers.append(ob)
    try:
        tr.step_body(data)
    finally:
        _lib.observers.remove(ob)
    torch.cuda.synchronize()
    for one in ("zgeo_head_loss", "nchw_to_nhwc", "sumsq_partial_step", "adamw_step_packed"):
        assert names.count(one) == 1, (one, names.count(one))
    gone = [n for n in names if n.startswith(("rownorm_", "pinhole_z_", "pose_loss_")) or n == "pack_conv_weights"]
    assert not gone, gone
    # both trunks ran forward and backward inside the one chain: 4 + 53 convs each way
    assert names.count("avgpool_fwd") == 2 and names.count("avgpool_bwd") == 2
    assert names.count("conv2d_fwd") == len(tr.trunk.convs) + len(tr.z_trunk.convs) == 57
    assert names.index("zgeo_head_loss") < names.index("avgpool_bwd") < names.index("sumsq_partial_step")
    assert names[-1] == "adamw_step_packed"


def test_pack_in_adamw_off_is_bit_identical():
    data = _data()
    flats = []
    for packed in (True, False):
        tr, _ = _make(torch.bfloat16, pack_in_adamw=packed)
        tr.capture(data, warmup=1)
        snapshots_differ = tr.arena.flat.clone()
        for _ in range(2):
            tr.step()
        torch.cuda.synchronize()
        assert not torch.equal(tr.arena.flat, snapshots_differ)
        flats.append((tr.arena.flat.clone(), tr.m.clone(), tr.v.clone()))
    for a, b in zip(*flats):
        assert torch.equal(a, b)


def test_pack_in_adamw_off_packs_once_per_trunk():
    from pose6d import _lib
    tr, _ = _make(torch.bfloat16, pack_in_adamw=False)
    names = []
    ob = lambda name, args: names.append(name)
    _lib.observers.append(ob)
    try:
        tr.step_body(_data())
    finally:
        _lib.observers.remove(ob)
    torch.cuda.synchronize()
    assert names.count("pack_conv_weights") == 2 and names.count("adamw_step") == 1
    assert names.count("adamw_step_packed") == 0


def test_checkpoint_round_trip():
    from models.pose_net_rgb_geometric import PoseNetRGBGeometric
    from pose6d.train import RGBGeometricTrainer
    tr, _ = _make(torch.bfloat16)
    data = _data()
    tr.step(data)
    ck = tr.checkpoint(epoch=3)
    buf = io.BytesIO()
    torch.save(ck, buf)
    buf.seek(0)
    ck = torch.load(buf, weights_only=True)
    assert list(ck["model_state_dict"].keys()) == list(PoseNetRGBGeometric(pretrained=False).state_dict().keys())
    m2 = PoseNetRGBGeometric(pretrained=False).cuda()
    tr2 = RGBGeometricTrainer(m2, B, dtype=torch.bfloat16)
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
    """After a replayed step the trainer's own engines hold packed weights equal to a fresh
    packing of the updated masters, in both trunks, and the module's eval forward equals a
    fresh module loaded from its state_dict."""
    from models.pose_net_rgb_geometric import PoseNetRGBGeometric
    dtype = torch.bfloat16
    tr, _ = _make(dtype)
    data = _data()
    tr.capture(data, warmup=1)
    tr.step()
    torch.cuda.synchronize()
    for eng in tr.trunks:                                       # written by the AdamW launch ...
        packed = [(op.wp.clone(), op.wt.clone() if op.wt is not None else None) for op in eng.convs]
        eng.pack_weights(force=True)                            # ... == a packing pass over the masters
        torch.cuda.synchronize()
        for op, (wp, wt) in zip(eng.convs, packed):
            assert torch.equal(op.wp, wp), op.name
            assert wt is None or torch.equal(op.wt, wt), op.name
    d = _data(seed=9, batch=2)
    x, bbox, K = d[0], d[1], d[2]
    model = tr.model.set_compute_dtype(dtype).eval()
    fresh = PoseNetRGBGeometric(pretrained=False).cuda().set_compute_dtype(dtype)
    fresh.load_state_dict(model.state_dict())
    fresh.eval()
    with torch.no_grad():
        rot, trans = model(x, bbox, K)
        rot2, trans2 = fresh(x, bbox, K)
    assert bool(torch.isfinite(rot).all()) and bool(torch.isfinite(trans).all())
    assert torch.equal(rot, rot2) and torch.equal(trans, trans2)
