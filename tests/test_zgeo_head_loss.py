"""pose6d_zgeo_head_loss (PoseNetRGBGeometric's head + loss in one single-block launch:
normalise with ||q|| + 1e-8, differentiable pinhole of the predicted depth, PoseLoss forward
and backward for dloss = 1, pinhole and normalise backward) against the six separate entry
points it replaces, its edge rows, a float64 CPU restatement, and its argument checks."""
import numpy as np
import pytest
import torch

from pose6d import _lib

GEO_EPS = 1e-8   # rownorm mode 1: x / (n + eps)


def _inputs(B, seed, k_batched, zero_row=True):
    """Rows with a role: B // 2 has an all-zero raw (zero_row); B - 1 has gt_trans z ==
    predicted z exactly; 0 has its bbox centre far outside [0, 223]."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(B, 4, generator=g) * 3
    z = torch.rand(B, 1, generator=g) * 1.2 + 0.3
    bbox = torch.rand(B, 2, generator=g) * 223
    bbox[0] = torch.tensor([-57.5, 391.25])
    s = 224.0 / (torch.rand(B, generator=g) * 200 + 100)
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0] = 572.4 * s
    K[:, 1, 1] = 573.6 * s
    K[:, 0, 2] = torch.rand(B, generator=g) * 224
    K[:, 1, 2] = torch.rand(B, generator=g) * 224
    K[:, 2, 2] = 1.0
    if not k_batched:
        K = K[0].clone()
    gr = torch.nn.functional.normalize(torch.randn(B, 4, generator=g), dim=1)
    gt = torch.randn(B, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 0.8])
    zero = B // 2 if zero_row else -1
    if zero_row:
        raw[zero] = 0.0                              # zero-norm row: the eps branch of the normalise
    gt[B - 1, 2] = z[B - 1, 0]
    return [t.cuda().contiguous() for t in (raw, z, bbox, K, gr, gt)], zero


def _fused(raw, z, bbox, K, gr, gt, rot_mode, wr=1.0, wt=10.0):
    from pose6d._lib import call, stream
    B = raw.shape[0]
    f = lambda *s: torch.empty(*s, device="cuda")
    rot, trans, loss, draw, dz = f(B, 4), f(B, 3), f(()), f(B, 4), f(B, 1)
    call("zgeo_head_loss", raw, z, bbox, K, 1 if K.dim() == 3 else 0, gr, gt, B, wr, wt, rot_mode, rot, trans, loss,
         draw, dz, stream())
    return rot, trans, loss, draw, dz


@pytest.mark.gpu
@pytest.mark.parametrize("B,zero_row", [(1, True), (1, False), (65, True), (257, True)])
@pytest.mark.parametrize("k_batched", [True, False], ids=["Kb", "K1"])
@pytest.mark.parametrize("rot_mode", [0, 1])
def test_zgeo_head_loss_matches_separate_calls(B, zero_row, k_batched, rot_mode):
    """B = 1: one thread (its row all zero, and once an ordinary row); 65: crosses a wave; 257:
    crosses the 256-thread block (the strided loop, all four per-wave partials).
    == rownorm_fwd (mode 1) -> pinhole_z_fwd ->
    pose_loss_fwd -> pose_loss_bwd (dloss = 1) -> pinhole_z_bwd + rownorm_bwd (mode 1): rot,
    trans and loss bit for bit; grad_raw and grad_z to rtol 1e-6 / atol 1e-9 (the compiler
    may contract these differently).  Edge rows: the all-zero raw row (rot = 0, grad_raw =
    drot / 1e-8, bit-identical to rownorm_bwd), the row whose gt z equals the predicted z
    (sign(0) = 0: nothing from the z component), and the bbox centre outside [0, 223] (no
    clamp)."""
    from pose6d._lib import call, stream
    (raw, z, bbox, K, gr, gt), zero = _inputs(B, 100 * B + 10 * int(k_batched) + rot_mode, k_batched, zero_row)
    kb = 1 if K.dim() == 3 else 0
    rot, trans, loss, draw, dz = _fused(raw, z, bbox, K, gr, gt, rot_mode)
    f = lambda *s: torch.empty(*s, device="cuda")
    rot2, trans2, loss2, drot2, dtr2, draw2, dz2 = f(B, 4), f(B, 3), f(()), f(B, 4), f(B, 3), f(B, 4), f(B, 1)
    one = torch.ones((), device="cuda")
    call("rownorm_fwd", raw, rot2, B, 4, 1, stream())
    call("pinhole_z_fwd", z, bbox, K, kb, B, trans2, stream())
    call("pose_loss_fwd", rot2, trans2, gr, gt, B, 1.0, 10.0, rot_mode, loss2, stream())
    call("pose_loss_bwd", rot2, trans2, gr, gt, B, 1.0, 10.0, rot_mode, one, drot2, dtr2, stream())
    call("pinhole_z_bwd", dtr2, bbox, K, kb, B, dz2, stream())
    call("rownorm_bwd", raw, drot2, draw2, B, 4, 1, stream())
    torch.cuda.synchronize()
    for a, b, what in ((rot, rot2, "rot"), (trans, trans2, "trans"), (loss, loss2, "loss")):
        assert torch.equal(a, b), (what, (a - b).abs().max().item())
    assert bool(torch.isfinite(loss))
    keep = torch.arange(B, device="cuda") != zero
    torch.testing.assert_close(draw[keep], draw2[keep], rtol=1e-6, atol=1e-9)
    torch.testing.assert_close(dz, dz2, rtol=1e-6, atol=1e-9)
    # no clamp: row 0's bbox centre lies outside [0, 223] and is used as it is
    Kh = K.cpu() if kb else K.cpu().expand(B, 3, 3)
    u, v, z0 = bbox[0, 0].cpu(), bbox[0, 1].cpu(), z[0, 0].cpu()
    assert float(u) < 0 and float(v) > 223
    np.testing.assert_allclose(float(trans[0, 0]), float((u.double() - Kh[0, 0, 2]) * z0 / Kh[0, 0, 0]), rtol=1e-6)
    np.testing.assert_allclose(float(trans[0, 1]), float((v.double() - Kh[0, 1, 2]) * z0 / Kh[0, 1, 1]), rtol=1e-6)
    assert float(trans[0, 2]) == float(z0)
    # gt z == predicted z: the z component's sign is 0, grad_z is the x / y terms alone
    b = B - 1
    assert float(trans[b, 2]) == float(gt[b, 2]) and float(dtr2[b, 2]) == 0.0
    d64 = dtr2[b].double().cpu()
    want = d64[0] * (bbox[b, 0].double().cpu() - Kh[b, 0, 2].double()) / Kh[b, 0, 0].double() \
        + d64[1] * (bbox[b, 1].double().cpu() - Kh[b, 1, 2].double()) / Kh[b, 1, 1].double()
    # (each term is c * O(1) with c = wt / (3 B), a few fp32 roundings each: 1e-6 c absolute)
    np.testing.assert_allclose(float(dz[b, 0]), float(want), rtol=0, atol=1e-6 * 10.0 / (3 * B))
    if not zero_row:
        return
    # the zero-norm row: no gradient reaches the norm, grad_raw = drot / eps
    assert bool(torch.isfinite(draw[zero]).all())
    assert torch.equal(draw2[zero], drot2[zero] / torch.full_like(drot2[zero], GEO_EPS))
    assert torch.equal(draw[zero], draw2[zero])
    assert torch.equal(rot[zero], torch.zeros(4, device="cuda"))


@pytest.mark.gpu
@pytest.mark.parametrize("k_batched", [True, False], ids=["Kb", "K1"])
def test_zgeo_head_loss_matches_cpu_restatement(k_batched):
    """Against r / (||r|| + 1e-8), oracle.resnet.pinhole_rgb_geometric and
    oracle.pose_loss.pose_loss in float64 under torch autograd w.r.t. raw and z on the CPU
    (B = 5, geodesic): 1e-4 relative.  Every |trans - gt| > 1e-3, so no sign sits on a
    rounding edge."""
    from oracle import pose_loss as OP
    from oracle import resnet as OR
    g = torch.Generator().manual_seed(13)   # min |trans - gt| = 1.8e-2 (K batched), 3.3e-2 (one K)
    B = 5
    raw = torch.randn(B, 4, generator=g) * 3
    z = torch.rand(B, 1, generator=g) * 1.2 + 0.3
    bbox = torch.rand(B, 2, generator=g) * 223
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0] = 572.4 + torch.rand(B, generator=g) * 100
    K[:, 1, 1] = 573.6 + torch.rand(B, generator=g) * 100
    K[:, 0, 2] = torch.rand(B, generator=g) * 224
    K[:, 1, 2] = torch.rand(B, generator=g) * 224
    K[:, 2, 2] = 1.0
    if not k_batched:
        K = K[0].clone()
    gr = torch.nn.functional.normalize(torch.randn(B, 4, generator=g), dim=1)
    gt = torch.randn(B, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 0.8])
    x = raw.double().requires_grad_(True)
    zz = z.double().requires_grad_(True)
    q = x / (torch.norm(x, dim=1, keepdim=True) + 1e-8)
    t = OR.pinhole_rgb_geometric(zz, bbox.double(), K.double())
    assert float((t.detach() - gt.double()).abs().min()) > 1e-3
    ref_loss = OP.pose_loss(q, t, gr.double(), gt.double(), 1.0, 10.0)
    ref_loss.backward()
    rot, trans, loss, draw, dz = _fused(*[a.cuda().contiguous() for a in (raw, z, bbox, K, gr, gt)], 0)
    np.testing.assert_allclose(rot.cpu().numpy(), q.detach().numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(trans.cpu().numpy(), t.detach().numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(loss.item(), ref_loss.item(), rtol=1e-4)
    ref = x.grad.numpy()
    np.testing.assert_allclose(draw.cpu().numpy(), ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())
    ref = zz.grad.numpy()
    np.testing.assert_allclose(dz.cpu().numpy(), ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())


def test_zgeo_head_loss_invalid_args_reported_without_gpu():
    lib = _lib.load()
    ok = dict(B=4, rot_mode=0)
    for bad, word in ((dict(B=0), b"empty batch"), (dict(rot_mode=2), b"rot_mode")):
        a = dict(ok, **bad)
        rc = lib.pose6d_zgeo_head_loss(None, None, None, None, 1, None, None, a["B"], 1.0, 10.0, a["rot_mode"], None,
                                       None, None, None, None, None)
        assert rc == 1, bad
        err = lib.pose6d_last_error()
        assert b"pose6d_zgeo_head_loss" in err and word in err, (bad, err)
