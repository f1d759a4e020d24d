"""pose6d_layernorm_* and pose6d_xattn_* (csrc/fusion.hip) at the edges of their launch
shapes, against float64 torch on the same fp32 operands and the kernels' own dropout
masks (the masks themselves: tests/test_dropout_masks.py).  Tolerances are those of
tests/test_fusion_kernels.py: 1e-4 relative to the tensor's scale, 1e-5 for the softmax
probabilities."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _close(got, ref, rtol, what):
    """test_fusion_kernels._close, with a floor of 1e-12 for the fp64 reference's own rounding:
    at D = 1 the exact dx and dgamma are 0 (x - mean == 0), the kernel returns 0 and autograd
    returns ~1e-16, which would otherwise be the scale everything is measured against."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs()
    bad = err > rtol * ref.abs() + rtol * scale + 1e-12
    assert not bool(bad.any()), f"{what}: max err {err.max().item():.3e} (scale {scale:.3e})"


def _act(z, act):
    return {0: z, 1: F.relu(z), 2: F.gelu(z)}[act]


# a workgroup of 256 threads per row: D = 1 (one live lane, zero variance), 255 / 257 (one
# lane short of / past one trip), 64 (one wave's worth; B = 33 rows).  ld == D: rows back to
# back.  shift: rows of mean 1e3 and unit spread (a one-pass E[x^2] - E[x]^2 variance would
# lose every digit there).  dy2: the second incoming gradient; acc: accumulate_dx and
# accumulate (onto nonzero dx / dgamma / dbeta).
LN_CASES = [
    dict(B=1, D=1, ld=1, shift=0.0, dy2=False, acc=False, p=0.0),
    dict(B=3, D=255, ld=260, shift=0.0, dy2=True, acc=True, p=0.0),
    dict(B=2, D=257, ld=257, shift=0.0, dy2=False, acc=True, p=0.0),
    dict(B=33, D=64, ld=72, shift=0.0, dy2=True, acc=False, p=0.2),
    dict(B=3, D=255, ld=260, shift=1e3, dy2=False, acc=False, p=0.0),
]


@pytest.mark.parametrize("case", LN_CASES, ids=lambda c: f"B{c['B']}-D{c['D']}-ld{c['ld']}-shift{int(c['shift'])}")
@pytest.mark.parametrize("act", [0, 2])
def test_layernorm_edges(act, case):
    from pose6d._lib import call, stream
    B, D, ld, p, acc = case["B"], case["D"], case["ld"], case["p"], case["acc"]
    g = torch.Generator().manual_seed(B * 1000 + D + act)
    x = (torch.randn(B, ld, generator=g) + case["shift"]) if case["shift"] else torch.randn(B, ld, generator=g) * 3 + 1
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
    dy, dy2 = torch.randn(B, ld, generator=g), torch.randn(B, ld, generator=g)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    y = torch.full((B, ld), 9.0, device=DEV)
    y2 = torch.empty(B, D, device=DEV)
    mask = torch.full((B, D), 7, device=DEV, dtype=torch.uint8)
    mean, rstd = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    seed = torch.tensor([(1 << 33) + 9], dtype=torch.int64, device=DEV)
    call("layernorm_fwd", xd, ld, y, ld, y2, B, D, gd, bd, 1e-5, act, p, seed, 77, mask, mean, rstd, stream())
    m = mask.cpu().double() if p > 0 else torch.ones(B, D, dtype=torch.float64)
    xr = x[:, :D].double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    yr = _act(F.layer_norm(xr, (D,), gr, br, 1e-5), act) * m / (1 - p)
    _close(y[:, :D], yr, 1e-4, "y")
    _close(y2, yr, 1e-4, "y2")
    assert bool((y[:, D:] == 9.0).all())   # nothing written past D
    _close(mean, x[:, :D].double().mean(1), 1e-4, "saved mean")
    _close(rstd, 1.0 / torch.sqrt(x[:, :D].double().var(1, unbiased=False) + 1e-5), 1e-4, "saved rstd")
    gin = dy[:, :D].double() + (dy2[:, :D].double() if case["dy2"] else 0)
    yr.backward(gin)
    dx = torch.full((B, ld), 5.0, device=DEV)
    dgam, dbet = torch.full((D,), 1.0, device=DEV), torch.full((D,), 2.0, device=DEV)
    call("layernorm_bwd", dy.to(DEV), ld, dy2.to(DEV) if case["dy2"] else None, ld if case["dy2"] else 0, xd, ld, B,
         D, gd, bd, mean, rstd, act, p, mask, dx, ld, int(acc), dgam, dbet, int(acc), stream())
    _close(dx[:, :D] - (5.0 if acc else 0.0), xr.grad, 1e-4, "dx")
    _close(dgam - (1.0 if acc else 0.0), gr.grad, 1e-4, "dgamma")
    _close(dbet - (2.0 if acc else 0.0), br.grad, 1e-4, "dbeta")
    assert bool((dx[:, D:] == 5.0).all())


def test_layernorm_empty_batch():
    from pose6d._lib import call, stream
    D = 64
    t = lambda *s: torch.full(s, 3.0, device=DEV)
    y, dx, dg, db = t(1, D), t(1, D), t(D), t(D)
    call("layernorm_fwd", None, D, y, D, None, 0, D, t(D), t(D), 1e-5, 2, 0.0, None, 0, None, None, None, stream())
    call("layernorm_bwd", None, D, None, 0, None, D, 0, D, t(D), t(D), None, None, 2, 0.0, None, dx, D, 0, dg, db, 0,
         stream())
    torch.cuda.synchronize()
    for buf in (y, dx, dg, db):
        assert bool((buf == 3.0).all())


def _xattn_ref(q, k, v, m, B, H, hd, scale, p):
    """the expression of test_cross_attention_core, in fp64"""
    qr, kr, vr = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    a = ((qr.view(B, H, hd) @ kr.view(B, H, hd).transpose(-2, -1)) * scale).softmax(-1)
    out = ((a * m / (1 - p)) @ vr.view(B, H, hd)).reshape(B, H * hd)
    return qr, kr, vr, a, out


# H = 16: the limit (H * H = the 256 threads of the workgroup, the LDS tiles full); H = 1: a
# softmax over one logit; (3, 5): a head shorter than a wave, nothing a power of two;
# (8, 70): a head of one full wave trip and a 6-lane one
@pytest.mark.parametrize("H,hd,p", [(16, 64, 0.0), (16, 64, 0.2), (1, 8, 0.0), (3, 5, 0.0), (8, 70, 0.0)])
def test_xattn_edges(H, hd, p):
    from pose6d._lib import call, stream
    B, D = 3, H * hd
    g = torch.Generator().manual_seed(H * 100 + hd)
    q, k, v, dout = (torch.randn(B, D, generator=g) for _ in range(4))
    out = torch.empty(B, D, device=DEV)
    probs = torch.empty(B, H, H, device=DEV)
    mask = torch.full((B, H, H), 7, device=DEV, dtype=torch.uint8)
    seed = torch.tensor([(1 << 34) + 3], dtype=torch.int64, device=DEV)
    scale = hd ** -0.5
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    call("xattn_fwd", qd, kd, vd, out, B, H, hd, scale, p, seed, 5, probs, mask, stream())
    m = mask.cpu().double() if p > 0 else torch.ones(B, H, H, dtype=torch.float64)
    qr, kr, vr, a, ref = _xattn_ref(q, k, v, m, B, H, hd, scale, p)
    _close(probs, a, 1e-5, "softmax probabilities")
    _close(out, ref, 1e-4, "attention output")
    ref.backward(dout.double())
    dq, dk, dv = (torch.empty(B, D, device=DEV) for _ in range(3))
    call("xattn_bwd", dout.to(DEV), qd, kd, vd, probs, mask, B, H, hd, scale, p, dq, dk, dv, stream())
    _close(dq, qr.grad, 1e-4, "dq")
    _close(dk, kr.grad, 1e-4, "dk")
    _close(dv, vr.grad, 1e-4, "dv")


def test_xattn_large_logits():
    """q and k of standard deviation 8: logits of standard deviation 64, +-200 at the ends --
    exp() of them overflows fp32 without the row-max subtraction."""
    from pose6d._lib import call, stream
    B, H, hd = 3, 16, 64
    D = H * hd
    g = torch.Generator().manual_seed(77)
    q, k, v = torch.randn(B, D, generator=g) * 8, torch.randn(B, D, generator=g) * 8, torch.randn(B, D, generator=g)
    out, probs = torch.empty(B, D, device=DEV), torch.empty(B, H, H, device=DEV)
    scale = hd ** -0.5
    call("xattn_fwd", q.to(DEV), k.to(DEV), v.to(DEV), out, B, H, hd, scale, 0.0, None, 0, probs, None, stream())
    _, _, _, a, ref = _xattn_ref(q, k, v, torch.ones(B, H, H, dtype=torch.float64), B, H, hd, scale, 0.0)
    logits = (q.double().view(B, H, hd) @ k.double().view(B, H, hd).transpose(-2, -1)) * scale
    assert logits.abs().max().item() > 150 and logits.max().item() > 89   # exp(89) > FLT_MAX
    assert bool(torch.isfinite(probs).all()) and bool(torch.isfinite(out).all())
    # H probabilities of at most 2^-24 relative rounding each, and the division by their sum
    assert float((probs.double().sum(-1) - 1).abs().max()) <= 1e-5
    _close(probs, a, 1e-5, "softmax probabilities")
    _close(out, ref, 1e-4, "attention output")


def test_xattn_rejects_17_heads():
    from pose6d._lib import Pose6dError, call, stream
    B, H, hd = 1, 17, 8
    D = H * hd
    t = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(Pose6dError, match="need 0 < H <= 16"):
        call("xattn_fwd", t(B, D), t(B, D), t(B, D), t(B, D), B, H, hd, 1.0, 0.0, None, 0, t(B, H, H), None, stream())
    with pytest.raises(Pose6dError, match="need 0 < H <= 16"):
        call("xattn_bwd", t(B, D), t(B, D), t(B, D), t(B, D), t(B, H, H), None, B, H, hd, 1.0, 0.0, t(B, D), t(B, D),
             t(B, D), stream())
