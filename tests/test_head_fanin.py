"""HeadEngine.backward(dx_out=..., dx_accumulate=True): two heads that read one feature sum
their input gradients in the second head's data-gradient GEMM (beta = 1), as RGBTrainer
does for PoseNetRGB's rotation and translation heads."""
import copy

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu


def _seq(in_dim, hid, out):
    return nn.Sequential(nn.Linear(in_dim, hid), nn.BatchNorm1d(hid), nn.ReLU(), nn.Linear(hid, out))


def _grads(seq):
    return {id(p): torch.zeros_like(p) for p in seq.parameters()}


# (256, 128): one launch; (2048, 1024): the first stage's data gradient takes pose6d_gemm_f32's
# split-K path (weight >= 2^20 elements, 128 column groups), whose reduce launch applies beta
@pytest.mark.parametrize("in_dim,hid", [(256, 128), (2048, 1024)])
def test_two_heads_accumulate_input_gradient(in_dim, hid):
    from pose6d.head import HeadEngine
    torch.manual_seed(0)
    B = 4
    heads = [_seq(in_dim, hid, 4).cuda().train(), _seq(in_dim, hid, 3).cuda().train()]
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, in_dim, generator=g).cuda()
    dys = [torch.randn(B, 4, generator=g).cuda(), torch.randn(B, 3, generator=g).cuda()]
    engs = [HeadEngine(h) for h in heads]
    grads = [_grads(h) for h in heads]
    for e in engs:
        e.forward(x, True)
    dx = engs[0].backward(dys[0], lambda p: grads[0][id(p)])
    first = dx.clone()
    out = engs[1].backward(dys[1], lambda p: grads[1][id(p)], dx_out=dx, dx_accumulate=True)
    torch.cuda.synchronize()
    assert out.data_ptr() == dx.data_ptr()

    # torch autograd in float64 on copies of the two heads
    ref = [copy.deepcopy(h).double() for h in heads]
    xr = x.double().requires_grad_(True)
    (ref[0](xr) * dys[0].double()).sum().backward(retain_graph=False)
    d0 = xr.grad.clone()
    (ref[1](xr) * dys[1].double()).sum().backward()
    # dx = W^T (gamma * invstd * (dy' - mean(dy') - xhat * mean(dy' * xhat))) cancels to ~0 for tiny
    # batches: the absolute tolerance is scaled by the factors' magnitudes, as for bn1d_bwd in
    # tests/test_head_kernels.py, not by |dx|
    scale = 0.0
    for h, dy in zip(heads, dys):
        bn, w0, w1 = h[1], h[0].weight, h[3].weight
        with torch.no_grad():
            var = h[0](x).var(0, unbiased=False)
        inv = (var + bn.eps).rsqrt()
        dyp = (dy @ w1).abs().max()
        scale += ((bn.weight * inv).max() * dyp * w0.abs().sum(0).max()).item()
    torch.testing.assert_close(first.double(), d0, rtol=1e-4, atol=1e-5 * scale)
    torch.testing.assert_close(dx.double(), xr.grad, rtol=1e-4, atol=1e-5 * scale)
    # the accumulating call is the plain one plus the add: the second head's own input gradient
    # and parameter gradients are those of a call without dx_out, and beta = 1 adds exactly
    alone = HeadEngine(copy.deepcopy(heads[1]))
    ga = _grads(alone.seq)
    alone.forward(x, True)
    second = alone.backward(dys[1], lambda p: ga[id(p)])
    assert torch.equal(dx, first + second)
    for p, q in zip(heads[1].parameters(), alone.seq.parameters()):
        assert torch.equal(grads[1][id(p)], ga[id(q)])


def test_defaults_change_nothing():
    """With dx_out / dx_accumulate left out the call is today's: dx and every parameter
    gradient are bit-identical between a call that omits them and one that passes the
    defaults; dx_out alone (beta = 0) stores the same bits into the caller's buffer."""
    from pose6d._lib import Pose6dError
    from pose6d.head import HeadEngine
    torch.manual_seed(0)
    B = 4
    head = _seq(256, 128, 4).cuda().train()
    g = torch.Generator().manual_seed(12)
    x = torch.randn(B, 256, generator=g).cuda()
    dy = torch.randn(B, 4, generator=g).cuda()
    res = []
    for kw in ({}, dict(dx_out=None, dx_accumulate=False), dict(dx_out=torch.full((B, 256), 7.0, device="cuda"))):
        eng = HeadEngine(copy.deepcopy(head))
        grads = _grads(eng.seq)
        eng.forward(x, True)
        dx = eng.backward(dy, lambda p: grads[id(p)], **kw)
        torch.cuda.synchronize()
        if "dx_out" in kw and kw["dx_out"] is not None:
            assert dx is kw["dx_out"]
        else:
            assert dx.data_ptr() == eng.stages[0].dx.data_ptr()
        res.append((dx.clone(), [grads[id(p)].clone() for p in eng.seq.parameters()]))
    for dx, gs in res[1:]:
        assert torch.equal(dx, res[0][0])
        for a, b in zip(gs, res[0][1]):
            assert torch.equal(a, b)
    eng = HeadEngine(copy.deepcopy(head))
    eng.forward(x, True)
    with pytest.raises(Pose6dError):
        eng.backward(dy, lambda p: torch.zeros_like(p), dx_accumulate=True)
