"""pose6d.train.RGBDTrainer: the whole PoseNetRGBD training step (forward + PoseLoss(1, 10,
geodesic) + backward + clip_grad_norm_(1.0) + AdamW, train_rgbd.py:97-110) as one captured
chain over two ResNet50 trunks, the cross-modal fusion core, the fusion MLP and two GELU
heads.  B = 4 at 224^2 (the trunk engines' input size); Dropout modules in eval unless a test
says otherwise (their RNG differs from torch's by construction).  The cases follow
tests/test_rgb_geometric_trainer.py."""
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
# and float64 runs of _oracle_step on the torch.manual_seed(0) model, 354 parameters):
# min |trans - gt| = 1.16e-2 (seeds 2025 and 7: 1.1e-1), so no sign of the L1 translation term
# is within 1e-4 of a rounding edge, and NO parameter has an exactly-zero gradient (the
# smallest float64 gradient norm is 0.1): no zero-gradient carve-out.  The fp32 oracle's own
# gradient error against float64 (relative Frobenius, per parameter): median 1.8e-2, max
# 3.2e-2; the two trunks 8e-4 .. 3.2e-2 (train-mode BatchNorm over B = 4 is ill-conditioned),
# the norms / attention / fusion MLP / heads 1.4e-4 .. 2.7e-4, trans_head down to 2e-8.  The
# trunks' 3e-2 would hide a wrong attention gradient, so the parameters outside the two
# backbones are bounded by themselves as well
DATA_SEED = 2024


def _data(seed=DATA_SEED, batch=B):
    from bench import synth_batch
    d = synth_batch(batch, torch.device("cuda"), seed=seed)
    return (d[0], d[1].unsqueeze(1), d[4], d[5])               # rgb, depth (B, 1, H, W), gt_rot, gt_trans


def _dropouts_eval(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.eval()


def _make(dtype, dropout=False, seed=0, **kw):
    from models.pose_net_rgbd import PoseNetRGBD
    from pose6d.train import RGBDTrainer
    warnings.simplefilter("ignore")
    torch.manual_seed(seed)
    m = PoseNetRGBD(pretrained=False)
    P0 = {k: v.clone() for k, v in m.state_dict().items()}
    tr = RGBDTrainer(m.cuda(), B, dtype=dtype, **kw)            # (puts the model in train mode)
    if not dropout:
        _dropouts_eval(m)
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
    rgb, depth, gr, gt = (t.cpu().to(dtype) for t in data)
    P = {k: (v.clone().to(dtype).requires_grad_(True) if v.is_floating_point() and "running" not in k
             else (v.clone().to(dtype) if v.is_floating_point() else v.clone())) for k, v in P0.items()}
    rot, trans = OR.forward_rgbd(P, rgb, depth, training=True)
    loss = OP.pose_loss(rot, trans, gr, gt, 1.0, 10.0)
    loss.backward()
    return rot.detach(), trans.detach(), loss.detach(), P


_ORACLE = {}


def _oracle(P0, data):
    """The fp32 and float64 oracle steps on (the seed-0 model, DATA_SEED): computed once, shared
    by the tests that need them, never modified."""
    if not _ORACLE:
        _ORACLE[32] = _oracle_step(P0, data, torch.float32)
        _ORACLE[64] = _oracle_step(P0, data, torch.float64)
    return _ORACLE[32], _ORACLE[64]


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


def _one_replayed_step(tr, data):
    snap = tr.snapshot()
    tr.capture(data, warmup=1)
    tr.restore(snap)
    before = tr.arena.flat.clone()
    tr.step()
    torch.cuda.synchronize()
    return before


def _grad_errors(tr, P32, P64):
    """Per-parameter Frobenius errors against float64: (names, ours, the fp32 oracle's)."""
    named = dict(tr.model.named_parameters())
    keys = [k for k, v in P64.items() if isinstance(v, torch.Tensor) and v.grad is not None]
    assert len(keys) == len(named) == 354
    ours = np.array([_frob(tr.arena.grad_of(named[k]), P64[k].grad) for k in keys])
    ref = np.array([_frob(P32[k].grad, P64[k].grad) for k in keys])
    return keys, ours, ref


def test_arena_order_and_engines():
    tr, _ = _make(torch.bfloat16)
    m = tr.model
    core = torch.nn.ModuleList([m.cross_attention, m.rgb_norm, m.depth_norm])
    groups = [m.rot_head, m.trans_head, m.fusion, core, m.depth_backbone, m.rgb_backbone]
    ids = [id(p) for p in tr.arena.params]
    lo, start = 0, []
    for mod in groups:                                         # six contiguous groups, in this order
        n = len(list(mod.parameters()))
        assert set(ids[lo:lo + n]) == {id(p) for p in mod.parameters()}, type(mod)
        start.append(lo)
        lo += n
    assert lo == len(ids) == len(set(ids)) == len(list(m.parameters())) == 354
    # within its group each trunk keeps its own gradient-completion order
    assert ids[start[4]:start[5]] == [id(p) for p in tr.depth_trunk.params_in_grad_order()]
    assert ids[start[5]:] == [id(p) for p in tr.trunk.params_in_grad_order()]
    # the fusion core: out_proj, q_proj, k | v weights, k | v biases, the two norms
    a = m.cross_attention
    want = [a.out_proj.weight, a.out_proj.bias, a.q_proj.weight, a.q_proj.bias, a.k_proj.weight, a.v_proj.weight,
            a.k_proj.bias, a.v_proj.bias, m.rgb_norm.weight, m.rgb_norm.bias, m.depth_norm.weight, m.depth_norm.bias]
    assert ids[start[3]:start[4]] == [id(p) for p in want]
    for k, v in ((a.k_proj.weight, a.v_proj.weight), (a.k_proj.bias, a.v_proj.bias)):   # adjacent, no gap
        assert v.data_ptr() == k.data_ptr() + 4 * k.numel()
        gk, gv = tr.arena.grad_of(k), tr.arena.grad_of(v)
        assert gv.data_ptr() == gk.data_ptr() + 4 * gk.numel()
    assert tr.head.seq is m.rot_head and tr.trans_head.seq is m.trans_head and tr.fusion_mlp.seq is m.fusion
    assert tr.fusion.attn is a and tr.fusion.rgb_norm is m.rgb_norm and tr.fusion.depth_norm is m.depth_norm
    assert tr.fusion.stacked and tr.fused_fusion
    assert tr.trunk.seq is m.rgb_backbone and tr.depth_trunk.seq is m.depth_backbone
    assert tr.trunk.in_channels == 3 and tr.depth_trunk.in_channels == 1
    assert tr.trunks == [tr.depth_trunk, tr.trunk]
    assert tr.trunk.dtype == tr.depth_trunk.dtype == torch.bfloat16 and tr.trunk.B == tr.depth_trunk.B == B


def test_fp32_step_against_oracle():
    """The replayed fp32 step against oracle.resnet.forward_rgbd(training=True) +
    oracle.pose_loss.pose_loss(1, 10), judged against a float64 run of the oracle (the scheme
    of test_rgb_geometric_trainer.test_fp32_step_against_oracle), then the fused clip + AdamW
    against torch."""
    tr, P0 = _make(torch.float32)
    data = _data()
    before = _one_replayed_step(tr, data)
    (r32, t32, L32, P32), (r64, t64, L64, P64) = _oracle(P0, data)
    margin = (t64 - data[3].cpu().double()).abs().min().item()
    print(f"min |trans - gt| = {margin:.2e}")
    assert margin >= 1e-4, "a translation sign sits on a rounding edge: pick another DATA_SEED"

    def check(ours, ref32, ref64, what, show=True):
        e, e_ref = _rel(ours, ref64), _rel(ref32, ref64)
        if show:
            print(f"{what}: ours {e:.2e} vs exact, reference fp32 {e_ref:.2e}")
        assert e <= max(1e-4, 3 * e_ref), f"{what}: ours {e:.2e} vs exact, reference fp32 {e_ref:.2e}"
        return e

    check(tr.rot, r32, r64, "rotation")
    check(tr.trans, t32, t64, "translation")
    check(tr.loss, L32, L64, "loss")
    keys, ours, ref = _grad_errors(tr, P32, P64)
    head = np.array(["backbone" not in k for k in keys])       # everything outside the two trunks
    assert head.sum() == 36
    print("gradient Frobenius errors: ours median %.2e max %.2e, reference fp32 median %.2e max %.2e"
          % (np.median(ours), ours.max(), np.median(ref), ref.max()))
    print("  over the %d parameters outside the trunks: ours max %.2e, reference fp32 max %.2e"
          % (head.sum(), ours[head].max(), ref[head].max()))
    for k, e, r in zip(keys, ours, ref):
        if "backbone" not in k:
            print(f"  {k}: ours {e:.2e}, reference fp32 {r:.2e}")
    # (the fp32 oracle's own error must leave the bounds far below a wrong gradient's O(1))
    assert np.median(ref) <= 0.05 and ref.max() <= 0.1, (np.median(ref), ref.max())
    assert np.median(ours) <= 2 * np.median(ref) + 1e-5, (np.median(ours), np.median(ref))
    assert ours.max() <= 3 * ref.max() + 1e-5, (ours.max(), ref.max())
    assert ours[head].max() <= 3 * ref[head].max() + 1e-5, (ours[head].max(), ref[head].max())
    sd = tr.model.state_dict()
    running = []
    for k in P0:
        if "running" in k:
            running.append(check(sd[k], P32[k], P64[k], k, show=False))
        elif "num_batches" in k:
            assert int(sd[k]) == int(P32[k]), k
    assert len(running) == 2 * 2 * 53                          # mean + var of 53 BatchNorms in each trunk
    print("running statistics of both trunks: ours max %.2e vs exact" % max(running))
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
        # the dropout did run: in both heads and the fusion MLP (their LayerNorm / GELU / Dropout
        # stage) and in the attention (8 x 8 probabilities per sample)
        masks = [eng.stages[1].mask for eng in (tr.head, tr.trans_head, tr.fusion_mlp)] + [tr.fusion.mask]
        for mk in masks:
            assert bool((mk == 0).any()) and bool((mk == 1).any())
        flats.append(tr.arena.flat.clone())
    assert torch.equal(flats[0], flats[1])


def _observe(tr, data):
    from pose6d import _lib
    names = []
    ob = lambda name, args: names.append(name)
    _lib.observers.append(ob)
    try:
        tr.step_body(data)
    finally:
        _lib.observers.remove(ob)
    torch.cuda.synchronize()
    return names


def test_launch_shape():
    """The step's launches by entry point: one fused head + loss, the paired LayerNorm and the
    strided attention once each way, both trunks inside the one chain, one norm-partials and
    one packed AdamW launch over the whole arena, and none of the launches those replace."""
    from pose6d import _lib
    tr, _ = _make(torch.bfloat16)
    data = _data()
    names = _observe(tr, data)
    for one in ("quat_head_loss", "layernorm_pair_fwd", "layernorm_pair_bwd", "xattn_fwd_strided",
                "xattn_bwd_strided", "sumsq_partial_step", "adamw_step_packed"):
        assert names.count(one) == 1, (one, names.count(one))
    gone = [n for n in names if n.startswith(("rownorm_", "pose_loss_")) or n in ("pack_conv_weights", "xattn_fwd",
                                                                                   "xattn_bwd")]
    assert not gone, gone
    assert names.count("nchw_to_nhwc") == 2
    assert names.count("avgpool_fwd") == 2 and names.count("avgpool_bwd") == 2
    assert names.count("conv2d_fwd") == len(tr.trunk.convs) + len(tr.depth_trunk.convs) == 106
    assert names.index("quat_head_loss") < names.index("avgpool_bwd") < names.index("sumsq_partial_step")
    assert names[-1] == "adamw_step_packed"
    # the fusion core by itself: 5 calls forward (pair-LN, q, kv, attention, out_proj), 8 backward
    # (out_proj wgrad + dgrad, attention, q wgrad + dgrad, kv wgrad + dgrad, pair-LN)
    f, b = [], []
    fwd, bwd = tr.fusion.forward, tr.fusion.backward

    def spy(fn, into):
        ob = lambda name, args: into.append(name)

        def run(*a, **k):
            _lib.observers.append(ob)
            try:
                return fn(*a, **k)
            finally:
                _lib.observers.remove(ob)
        return run

    tr.fusion.forward, tr.fusion.backward = spy(fwd, f), spy(bwd, b)
    try:
        tr.step_body(data)
    finally:
        tr.fusion.forward, tr.fusion.backward = fwd, bwd
    torch.cuda.synchronize()
    assert f == ["layernorm_pair_fwd", "gemm_f32", "gemm_f32", "xattn_fwd_strided", "gemm_f32"], f
    assert b == ["linear_wgrad", "gemm_f32", "xattn_bwd_strided", "linear_wgrad", "gemm_f32", "linear_wgrad",
                 "gemm_f32", "layernorm_pair_bwd"], b
    assert (f + b).count("linear_wgrad") == 3 and f.count("gemm_f32") == 3 and b.count("gemm_f32") == 3


def test_unfused_fusion_agrees():
    """fused_fusion=False (the autograd path's 7 / 14-launch fusion chain) and True from the same
    start: the stacked GEMMs sum in another order, so the two are compared through their errors
    against the float64 oracle, gradient by gradient."""
    data = _data()
    errs, P0 = {}, None
    for fused in (False, True):
        tr, P0 = _make(torch.float32, fused_fusion=fused)
        assert tr.fusion.stacked == fused
        if not fused:
            snap = tr.snapshot()
            names = _observe(tr, data)                          # today's chain, entry point by entry point
            tr.restore(snap)
            assert names.count("layernorm_pair_fwd") == names.count("xattn_fwd_strided") == 0
            assert names.count("xattn_fwd") == names.count("xattn_bwd") == 1
            assert names.count("layernorm_fwd") == 2 + 4       # the two norms + fusion MLP (2) and heads (1 + 1)
        _one_replayed_step(tr, data)
        assert bool(torch.isfinite(tr.loss))
        (_, _, _, P32), (_, _, _, P64) = _oracle(P0, data)
        keys, errs[fused], _ = _grad_errors(tr, P32, P64)
    for k, e_un, e_f in zip(keys, errs[False], errs[True]):
        if "backbone" not in k:
            print(f"{k}: unfused {e_un:.2e}, fused {e_f:.2e} vs float64")
    print("all %d gradients: unfused median %.2e max %.2e, fused median %.2e max %.2e"
          % (len(keys), np.median(errs[False]), errs[False].max(), np.median(errs[True]), errs[True].max()))
    bad = [(k, e_un, e_f) for k, e_un, e_f in zip(keys, errs[False], errs[True]) if not e_f <= 3 * e_un + 1e-5]
    assert not bad, bad[:5]


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
    tr, _ = _make(torch.bfloat16, pack_in_adamw=False)
    names = _observe(tr, _data())
    assert names.count("pack_conv_weights") == 2 and names.count("adamw_step") == 1
    assert names.count("adamw_step_packed") == 0


def test_checkpoint_round_trip():
    from models.pose_net_rgbd import PoseNetRGBD
    from pose6d.train import RGBDTrainer
    tr, _ = _make(torch.bfloat16)
    data = _data()
    tr.step(data)
    ck = tr.checkpoint(epoch=3)
    buf = io.BytesIO()
    torch.save(ck, buf)
    buf.seek(0)
    ck = torch.load(buf, weights_only=True)
    keys = list(ck["model_state_dict"].keys())
    assert len(keys) == 672 and keys == list(PoseNetRGBD(pretrained=False).state_dict().keys())
    m2 = PoseNetRGBD(pretrained=False).cuda()
    tr2 = RGBDTrainer(m2, B, dtype=torch.bfloat16)
    _dropouts_eval(m2)
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
    from models.pose_net_rgbd import PoseNetRGBD
    dtype = torch.bfloat16
    tr, _ = _make(dtype)
    data = _data()
    tr.capture(data, warmup=1)
    tr.step()
    torch.cuda.synchronize()
    assert len(tr.trunks) == 2
    for eng in tr.trunks:                                       # written by the AdamW launch ...
        packed = [(op.wp.clone(), op.wt.clone() if op.wt is not None else None) for op in eng.convs]
        eng.pack_weights(force=True)                            # ... == a packing pass over the masters
        torch.cuda.synchronize()
        for op, (wp, wt) in zip(eng.convs, packed):
            assert torch.equal(op.wp, wp), op.name
            assert wt is None or torch.equal(op.wt, wt), op.name
    x, depth = _data(seed=9, batch=2)[:2]
    model = tr.model.set_compute_dtype(dtype).eval()
    fresh = PoseNetRGBD(pretrained=False).cuda().set_compute_dtype(dtype)
    fresh.load_state_dict(model.state_dict())
    fresh.eval()
    with torch.no_grad():
        rot, trans = model(x, depth)
        rot2, trans2 = fresh(x, depth)
    assert bool(torch.isfinite(rot).all()) and bool(torch.isfinite(trans).all())
    assert torch.equal(rot, rot2) and torch.equal(trans, trans2)
