"""pose6d_avgpool_fwd / _bwd (csrc/pool.hip: nn.AdaptiveAvgPool2d(1) + view(B, -1) on NHWC)
in fp32 and bf16 against the float64 mean of the same (bf16-rounded) input.

Forward block = 64 channel chunks (16 bytes: 4 fp32 / 8 bf16 channels) x 4 pixel groups,
grid (ceil(chunks / 64), N); each group strides the pixels by 4, four at a time while
p + 12 < HW, then one at a time:
  (1, 1, 8)      one pixel: groups 1..3 add nothing; 2 chunks (fp32) / 1 (bf16)
  (2, 3, 64)     fewer pixels than groups
  (2, 17, 520)   group 0: one unrolled trip (pixels 0, 4, 8, 12) then pixel 16; 130 fp32 chunks =
                 3 workgroups, 65 bf16 chunks = one lane in a second workgroup
  (2, 49, 2048)  the product's shape: 3 unrolled trips per group, then pixel 48 for group 0
  (1, 64, 32)    HW a multiple of 16: no tail
Tolerance 1e-6 of the tensor's scale (tests/test_conv_kernels.py uses it for the fp32
pool; the bf16 input is rounded before both sides see it, and the sum is fp32 either way).
dx in bf16 is the fp64 quotient rounded once: relative 2^-8."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(1, 1, 8), (2, 3, 64), (2, 17, 520), (2, 49, 2048), (1, 64, 32)]
DTYPES = [(0, torch.float32), (1, torch.bfloat16)]


def _close(got, ref, rtol, what):
    got, ref = got.double().cpu(), ref.double().cpu()
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs()
    bad = err > rtol * ref.abs() + rtol * scale
    assert not bool(bad.any()), f"{what}: max err {err.max().item():.3e} (scale {scale:.3e}), {int(bad.sum())} bad"


@pytest.mark.parametrize("N,HW,C", SHAPES)
@pytest.mark.parametrize("dt,dtype", DTYPES, ids=["fp32", "bf16"])
def test_avgpool_fwd(dt, dtype, N, HW, C):
    from pose6d._lib import call, stream
    g = torch.Generator().manual_seed(N * 1000 + HW + C)
    x = (torch.randn(N, HW, C, generator=g) + 0.25).to(dtype).to(DEV)   # NHWC, rounded to the dtype first
    outs = []
    for _ in range(2):
        y = torch.full((N, C), float("nan"), device=DEV)
        call("avgpool_fwd", dt, x, y, N, HW, C, stream())
        outs.append(y)
    _close(outs[0], x.double().mean(1), 1e-6, "avgpool_fwd")
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("N,HW,C", SHAPES)
@pytest.mark.parametrize("dt,dtype", DTYPES, ids=["fp32", "bf16"])
def test_avgpool_bwd(dt, dtype, N, HW, C):
    from pose6d._lib import call, stream
    g = torch.Generator().manual_seed(N * 1000 + HW + C + 1)
    dy = torch.randn(N, C, generator=g).to(DEV)
    dx = torch.full((N, HW, C), float("nan"), device=DEV, dtype=dtype)   # sentinel: every element is written
    call("avgpool_bwd", dt, dy, dx, N, HW, C, stream())
    assert bool(torch.isfinite(dx).all())
    ref = (dy.double() / HW)[:, None, :].expand(N, HW, C)
    if dtype == torch.float32:
        _close(dx, ref, 1e-6, "avgpool_bwd")
    else:
        torch.testing.assert_close(dx.double(), ref, rtol=2.0 ** -8, atol=0)
    assert torch.equal(dx, dx[:, :1, :].expand(N, HW, C))   # the same value at every pixel
