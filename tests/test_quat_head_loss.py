"""pose6d_quat_head_loss (PoseNetRGB's head + loss in one single-block launch: normalise,
PoseLoss forward and backward for dloss = 1, normalise backward) against the four separate
entry points it replaces, against the CPU restatement, and its argument checks."""
import numpy as np
import pytest
import torch

from pose6d import _lib

EPS = {0: 1e-12, 1: 1e-8}   # rownorm mode 0: x / max(n, eps);  mode 1: x / (n + eps)


def _inputs(B, seed, zero_row=True):
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(B, 4, generator=g) * 3
    zero = B // 2 if zero_row else -1
    if zero_row:
        raw[zero] = 0.0                              # zero-norm row: the eps branch of both normalises
    trans = torch.randn(B, 3, generator=g)
    gr = torch.nn.functional.normalize(torch.randn(B, 4, generator=g), dim=1)
    gt = torch.randn(B, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 0.8])
    trans[B - 1, 1] = gt[B - 1, 1]                   # sign(0) = 0 -> zero gradient
    return [t.cuda().contiguous() for t in (raw, trans, gr, gt)], zero


def _fused(raw, trans, gr, gt, rot_mode, norm_mode, wr=1.0, wt=10.0):
    from pose6d._lib import call, stream
    B = raw.shape[0]
    f = lambda *s: torch.empty(*s, device="cuda")
    rot, loss, draw, dtr = f(B, 4), f(()), f(B, 4), f(B, 3)
    call("quat_head_loss", raw, trans, gr, gt, B, wr, wt, rot_mode, norm_mode, rot, loss, draw, dtr, stream())
    return rot, loss, draw, dtr


@pytest.mark.gpu
@pytest.mark.parametrize("B,zero_row", [(1, True), (1, False), (65, True), (257, True)])
@pytest.mark.parametrize("norm_mode", [0, 1])
@pytest.mark.parametrize("rot_mode", [0, 1])
def test_quat_head_loss_matches_separate_calls(B, zero_row, norm_mode, rot_mode):
    """B = 1: one thread (its row all zero, and once an ordinary row); 65: crosses a wave; 257:
    crosses the 256-thread block (the strided loop, all four per-wave partials).
    == rownorm_fwd -> pose_loss_fwd -> pose_loss_bwd (dloss = 1) -> rownorm_bwd: rot, loss and
    grad_trans bit for bit; grad_raw to 1e-6 (the compiler may contract the normalise
    backward differently), its zero-norm row equal to rownorm_bwd's drot / eps."""
    from pose6d._lib import call, stream
    (raw, trans, gr, gt), zero = _inputs(B, 100 * B + 10 * norm_mode + rot_mode, zero_row)
    rot, loss, draw, dtr = _fused(raw, trans, gr, gt, rot_mode, norm_mode)
    f = lambda *s: torch.empty(*s, device="cuda")
    rot2, loss2, drot2, draw2, dtr2 = f(B, 4), f(()), f(B, 4), f(B, 4), f(B, 3)
    one = torch.ones((), device="cuda")
    call("rownorm_fwd", raw, rot2, B, 4, norm_mode, stream())
    call("pose_loss_fwd", rot2, trans, gr, gt, B, 1.0, 10.0, rot_mode, loss2, stream())
    call("pose_loss_bwd", rot2, trans, gr, gt, B, 1.0, 10.0, rot_mode, one, drot2, dtr2, stream())
    call("rownorm_bwd", raw, drot2, draw2, B, 4, norm_mode, stream())
    torch.cuda.synchronize()
    for a, b, what in ((rot, rot2, "rot"), (loss, loss2, "loss"), (dtr, dtr2, "grad_trans")):
        assert torch.equal(a, b), (what, (a - b).abs().max().item())
    assert float(dtr[B - 1, 1]) == 0.0
    keep = torch.arange(B, device="cuda") != zero
    torch.testing.assert_close(draw[keep], draw2[keep], rtol=1e-6, atol=1e-9)
    if not zero_row:
        return
    # the zero-norm row: no gradient reaches the norm, grad_raw = drot / eps
    assert bool(torch.isfinite(draw[zero]).all())
    assert torch.equal(draw2[zero], drot2[zero] / torch.full_like(drot2[zero], EPS[norm_mode]))
    assert torch.equal(draw[zero], draw2[zero])
    assert torch.equal(rot[zero], torch.zeros(4, device="cuda"))


@pytest.mark.gpu
def test_quat_head_loss_matches_cpu_restatement():
    """loss and gradients against oracle.pose_loss.pose_loss_and_grads composed with a float64
    F.normalize under torch autograd on the CPU (B = 5, geodesic, norm_mode 0): 1e-4 relative."""
    from oracle import pose_loss as OP
    g = torch.Generator().manual_seed(7)
    B = 5
    raw = torch.randn(B, 4, generator=g) * 3
    trans = torch.randn(B, 3, generator=g)
    gr = torch.nn.functional.normalize(torch.randn(B, 4, generator=g), dim=1)
    gt = torch.randn(B, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 0.8])
    rot, loss, draw, dtr = _fused(raw.cuda(), trans.cuda(), gr.cuda(), gt.cuda(), 0, 0)
    x = raw.double().requires_grad_(True)
    q = x / torch.linalg.vector_norm(x, dim=1, keepdim=True).clamp_min(1e-12)
    ref_loss, g_rot, g_trans = OP.pose_loss_and_grads(q.detach(), trans, gr, gt, rot_weight=1.0, trans_weight=10.0)
    q.backward(g_rot.double())                       # the oracle's d loss / d rot back through the normalise
    np.testing.assert_allclose(rot.cpu().numpy(), q.detach().numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(loss.item(), ref_loss.item(), rtol=1e-4)
    np.testing.assert_allclose(dtr.cpu().numpy(), g_trans.numpy(), rtol=1e-4, atol=1e-6)
    ref = x.grad.numpy()
    np.testing.assert_allclose(draw.cpu().numpy(), ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())


def test_quat_head_loss_invalid_args_reported_without_gpu():
    lib = _lib.load()
    ok = dict(B=4, rot_mode=0, norm_mode=0)
    for bad, word in ((dict(B=0), b"empty batch"), (dict(rot_mode=2), b"rot_mode"), (dict(norm_mode=2), b"norm_mode")):
        a = dict(ok, **bad)
        rc = lib.pose6d_quat_head_loss(None, None, None, None, a["B"], 1.0, 10.0, a["rot_mode"], a["norm_mode"], None,
                                       None, None, None, None)
        assert rc == 1, bad
        err = lib.pose6d_last_error()
        assert b"pose6d_quat_head_loss" in err and word in err, (bad, err)
