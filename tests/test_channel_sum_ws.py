"""pose6d_channel_sum_ws (the conv-bias gradient over long NHWC tensors in two deterministic
passes) against exact integer sums, against pose6d_channel_sum where it falls back to it,
and its argument checks.  Inputs are small integers (exact in bf16, partial and total sums
below 2^24 and so exact in fp32): every summation order gives the same bits, and a row that
is skipped or counted twice shows as a wrong integer."""
import pytest
import torch

from pose6d import _lib

DT = {torch.float32: 0, torch.bfloat16: 1}


def _x(M, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (M, C), generator=g).to(dtype).cuda()


def _sum_ws(x, acc=None, ws_floats=1 << 17):
    from pose6d._lib import call, stream
    M, C = x.shape
    out = torch.full((C,), float("nan"), device="cuda") if acc is None else acc.clone()
    ws = torch.empty(max(ws_floats, 1), device="cuda")
    call("channel_sum_ws", DT[x.dtype], x, M, C, out, 0 if acc is None else 1, ws, ws_floats, stream())
    torch.cuda.synchronize()
    return out


# (M, C): the z-CNN's four biases at batch 4 (112^2 x 32 ... 14^2 x 256: 1 to 32 chunks per row
# in fp32, 1/2 to 16 in bf16); rows that do not divide into the row blocks or the rows of a
# trip; fewer rows than one trip; one row
SHAPES = [(4 * 112 * 112, 32), (4 * 56 * 56, 64), (4 * 28 * 28, 128), (4 * 14 * 14, 256), (5003, 64), (4099, 8),
          (37, 32), (1, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("M,C", SHAPES)
def test_channel_sum_ws_is_exact_on_integers(M, C, dtype):
    x = _x(M, C, dtype, 7 * M + C)
    want = x.long().sum(0).float()
    assert torch.equal(_sum_ws(x), want)
    base = torch.arange(C, device="cuda", dtype=torch.float32) - 3.0
    assert torch.equal(_sum_ws(x, acc=base), want + base)      # accumulate = 1


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_channel_sum_ws_workspace_bounds_the_row_blocks(dtype):
    """Any workspace size gives the same (exact) sums: room for 512, 3 and 2 row blocks, and
    for fewer than two (the one-launch kernel)."""
    M, C = 40000, 32
    x = _x(M, C, dtype, 3)
    want = x.long().sum(0).float()
    for ws_floats in (1 << 17, 3 * C + 5, 2 * C, 2 * C - 1, 0):
        assert torch.equal(_sum_ws(x, ws_floats=ws_floats), want), ws_floats


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [3, 12, 24, 100])
def test_channel_sum_ws_falls_back_for_other_channel_counts(C, dtype):
    """C that is not a power-of-two number of 16-byte chunks: pose6d_channel_sum's result, bit
    for bit (non-integer data: the summation order is that kernel's)."""
    from pose6d._lib import call, stream
    M = 3001
    g = torch.Generator().manual_seed(C)
    x = torch.randn(M, C, generator=g).to(dtype).cuda()
    ref = torch.empty(C, device="cuda")
    call("channel_sum", DT[dtype], x, M, C, ref, 0, stream())
    assert torch.equal(_sum_ws(x), ref)


@pytest.mark.gpu
def test_zcnn_bias_gradient_through_the_trunk_engine():
    """TrunkEngine(kind='zcnn').backward writes each conv bias's gradient = the channel sums of
    that conv's output gradient (the engine's own buffer), in fp32 and bf16."""
    from models.pose_net_rgb_geometric import PoseNetRGBGeometric
    from pose6d.trunk import TrunkEngine
    torch.manual_seed(0)
    m = PoseNetRGBGeometric(pretrained=False).cuda().train()
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(1)).cuda()
    for dtype in (torch.float32, torch.bfloat16):
        eng = TrunkEngine(m.z_backbone, 3, kind="zcnn")
        eng.set_dtype(dtype)
        feat = eng.forward(x, True)
        grads = {id(p): torch.zeros_like(p) for p in m.z_backbone.parameters()}
        eng.backward(torch.randn(feat.shape, generator=torch.Generator().manual_seed(2)).cuda(),
                     lambda p: grads[id(p)])
        torch.cuda.synchronize()
        for op in eng.convs:
            want = op.out.g.double().sum((0, 1, 2))
            mag = op.out.g.double().abs().sum((0, 1, 2))
            got = grads[id(op.conv.bias)].double()
            # fp32 sums of M = 2 Ho Wo terms in chains of under 1024 adds: 1024 * 2^-24 * sum |x|
            assert bool(((got - want).abs() <= 1024 * 2.0 ** -24 * mag + 1e-30).all()), (op.name, dtype)


def test_channel_sum_ws_invalid_args_reported_without_gpu():
    lib = _lib.load()
    for bad in (dict(dtype=2), dict(C=0), dict(M=-1), dict(ws=-1)):
        a = dict(dict(dtype=0, M=8, C=32, ws=0), **bad)
        rc = lib.pose6d_channel_sum_ws(a["dtype"], None, a["M"], a["C"], None, 0, None, a["ws"], None)
        assert rc == 1, bad
        assert b"pose6d_channel_sum_ws" in lib.pose6d_last_error(), bad
