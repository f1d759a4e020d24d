"""pose6d_xattn_fwd_strided / _bwd_strided against the contiguous entry points on copies of
the same data: k and v (and dk | dv) are the two halves of a (B, 2 D) buffer, q is
contiguous; outputs, probs, the dropout mask (p = 0.1, fixed seed: its index does not depend
on the strides) and dq / dk / dv must be bit-equal.  hd = 40 is no multiple of the 64 lanes,
H = 3 is an odd head count."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,H,hd", [(3, 8, 40), (2, 3, 256)])
def test_strided_equals_contiguous(B, H, hd, p):
    from pose6d._lib import call, stream
    D = H * hd
    g = torch.Generator().manual_seed(B * 100 + H)
    q = torch.randn(B, D, generator=g).cuda()
    kv = torch.randn(B, 2 * D, generator=g).cuda()
    dout = torch.randn(B, D, generator=g).cuda()
    k, v = kv[:, :D], kv[:, D:]
    kc, vc = k.contiguous(), v.contiguous()
    scale = hd ** -0.5
    seed = torch.tensor([4321], dtype=torch.int64, device="cuda")
    new = lambda *s, dt=torch.float32: torch.full(s, 3, device="cuda", dtype=dt)

    out_c, probs_c, mask_c = new(B, D), new(B, H, H), new(B, H, H, dt=torch.uint8)
    call("xattn_fwd", q, kc, vc, out_c, B, H, hd, scale, p, seed, 5, probs_c, mask_c, stream())
    # out strided too: the left half of a (B, 2 D) buffer whose right half must stay untouched
    out_s, probs_s, mask_s = new(B, 2 * D), new(B, H, H), new(B, H, H, dt=torch.uint8)
    call("xattn_fwd_strided", q, D, k, 2 * D, v, 2 * D, out_s, 2 * D, B, H, hd, scale, p, seed, 5, probs_s, mask_s,
         stream())
    torch.cuda.synchronize()
    assert torch.equal(out_s[:, :D], out_c) and bool((out_s[:, D:] == 3).all())
    assert torch.equal(probs_s, probs_c)
    if p > 0:
        assert torch.equal(mask_s, mask_c)
        assert bool((mask_c == 0).any()) and bool((mask_c == 1).any())
    assert bool(torch.isfinite(out_c).all()) and not torch.equal(out_c, torch.full_like(out_c, 3))

    dq_c, dk_c, dv_c = new(B, D), new(B, D), new(B, D)
    call("xattn_bwd", dout, q, kc, vc, probs_c, mask_c, B, H, hd, scale, p, dq_c, dk_c, dv_c, stream())
    dq_s, dkv = new(B, D), new(B, 2 * D)
    call("xattn_bwd_strided", dout, D, q, D, k, 2 * D, v, 2 * D, probs_s, mask_s, B, H, hd, scale, p, dq_s, D,
         dkv[:, :D], 2 * D, dkv[:, D:], 2 * D, stream())
    torch.cuda.synchronize()
    assert torch.equal(dq_s, dq_c)
    assert torch.equal(dkv[:, :D], dk_c) and torch.equal(dkv[:, D:], dv_c)
    assert bool(torch.isfinite(dkv).all()) and bool((dkv != 3).any())


def test_stride_below_row_is_an_error():
    from pose6d._lib import Pose6dError, call, stream
    B, H, hd = 2, 3, 40
    D = H * hd
    t = lambda *s: torch.zeros(*s, device="cuda")
    probs, mask = t(B, H, H), torch.zeros(B, H, H, device="cuda", dtype=torch.uint8)
    with pytest.raises(Pose6dError, match="row stride"):
        call("xattn_fwd_strided", t(B, D), D, t(B, D), D - 1, t(B, D), D, t(B, D), D, B, H, hd, 1.0, 0.0, None, 0,
             probs, mask, stream())
    with pytest.raises(Pose6dError, match="row stride"):
        call("xattn_bwd_strided", t(B, D), D, t(B, D), D, t(B, D), D, t(B, D), D, probs, mask, B, H, hd, 1.0, 0.0,
             t(B, D), D, t(B, D), D, t(B, D), D - 1, stream())
    call("xattn_fwd_strided", None, D, None, D, None, D, None, D, 0, H, hd, 1.0, 0.0, None, 0, probs, mask, stream())
