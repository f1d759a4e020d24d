"""FusionEngine(stacked=True) -- the paired LayerNorm and k_proj | v_proj as one stacked Linear
-- against a float64 torch restatement (oracle.resnet.cross_attention with F.layer_norm,
backward by autograd), judged by the unstacked engine's own error against the same float64
result.  B = 4 at the model's dimensions (D = 2048, H = 8: the engine needs D = H * hd and the
stacked path the real adjacency sizes); the parameters live in a small FlatArena in the
trainer's order."""
import pytest
import torch
import torch.nn.functional as F

from oracle import resnet as OR

pytestmark = pytest.mark.gpu

B, D, H = 4, 2048, 8


def _modules(seed=0):
    from models.pose_net_rgbd import CrossModalAttention
    torch.manual_seed(seed)
    attn = CrossModalAttention(D, num_heads=H, dropout=0.1)
    rn, dn = torch.nn.LayerNorm(D), torch.nn.LayerNorm(D)
    with torch.no_grad():
        for ln in (rn, dn):                                   # non-trivial affine parts
            ln.weight.add_(0.2 * torch.randn(D))
            ln.bias.add_(0.2 * torch.randn(D))
        for lin in (attn.q_proj, attn.k_proj, attn.v_proj, attn.out_proj):
            lin.bias.add_(0.1 * torch.randn(D))
    mods = torch.nn.ModuleDict({"cross_attention": attn, "rgb_norm": rn, "depth_norm": dn}).eval()
    g = torch.Generator().manual_seed(seed + 1)
    x = [torch.randn(B, D, generator=g) * 2 + 0.5 for _ in range(2)]
    dout = torch.randn(B, 2 * D, generator=g)
    return mods, x, dout


@pytest.fixture(scope="module")
def exact():
    """The float64 result, computed once: out, (d_rgb, d_depth), {name: grad}."""
    mods, x, dout = _modules()
    P = {k: v.detach().double().requires_grad_(True) for k, v in mods.state_dict().items()}
    xr, xd = (t.double().requires_grad_(True) for t in x)
    r = F.layer_norm(xr, (D,), P["rgb_norm.weight"], P["rgb_norm.bias"], 1e-5)
    d = F.layer_norm(xd, (D,), P["depth_norm.weight"], P["depth_norm.bias"], 1e-5)
    out = torch.cat([r + OR.cross_attention(r, d, P, heads=H), d], dim=1)
    (out * dout.double()).sum().backward()
    return out.detach(), (xr.grad, xd.grad), {k: v.grad for k, v in P.items()}


def _run(stacked, order=None):
    """One forward + backward of the engine on the GPU -> (out, (d_rgb, d_depth), {name: grad})."""
    from pose6d.fusion import FusionEngine
    from pose6d.train import FlatArena
    mods, x, dout = _modules()
    mods = mods.cuda()
    eng = FusionEngine(mods["cross_attention"], mods["rgb_norm"], mods["depth_norm"], stacked=stacked)
    arena = FlatArena(order(eng) if order else eng.params_in_grad_order(), torch.device("cuda"))
    assert len(arena.params) == len(list(mods.parameters())) == 12
    out = eng.forward(x[0].cuda(), x[1].cuda(), False).clone()
    dx = tuple(t.clone() for t in eng.backward(dout.cuda(), arena.grad_of))
    torch.cuda.synchronize()
    return out, dx, {k: arena.grad_of(p).clone() for k, p in mods.named_parameters()}, eng


def _err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def test_stacked_against_float64(exact):
    out64, dx64, g64 = exact
    res = {s: _run(s) for s in (False, True)}
    assert res[True][3].stacked and not res[False][3].stacked
    rows = [("out", lambda r: r[0], out64), ("d_rgb", lambda r: r[1][0], dx64[0]),
            ("d_depth", lambda r: r[1][1], dx64[1])]
    rows += [(k, (lambda r, k=k: r[2][k]), g) for k, g in g64.items()]
    assert len(rows) == 15
    for what, pick, ref in rows:
        e_un, e_st = _err(pick(res[False]), ref), _err(pick(res[True]), ref)
        print(f"{what}: unstacked {e_un:.2e}, stacked {e_st:.2e} vs float64 (|ref| {ref.norm().item():.2e})")
        assert ref.norm().item() > 1e-6, what                 # (no exactly-zero gradient: errors are relative)
        assert e_un < 1e-4, (what, e_un)
        assert e_st <= 3 * e_un + 1e-6, (what, e_st, e_un)


def test_paired_norms_are_bit_identical_to_separate():
    """What the stacked mode does not re-order stays bit-equal to the unstacked engine: the
    normalised features (the right half of `out`), and the norms' statistics."""
    un, st = _run(False), _run(True)
    assert torch.equal(un[0][:, D:], st[0][:, D:])
    assert torch.equal(un[3].stats, st[3].stats) and torch.equal(un[3].R, st[3].R)


def test_non_adjacent_arena_raises():
    from pose6d._lib import Pose6dError

    def gap_order(eng):                                       # q_proj's bias between k and v weights
        a = eng.attn
        return [a.out_proj.weight, a.out_proj.bias, a.q_proj.weight, a.k_proj.weight, a.q_proj.bias,
                a.v_proj.weight, a.k_proj.bias, a.v_proj.bias, eng.rgb_norm.weight, eng.rgb_norm.bias,
                eng.depth_norm.weight, eng.depth_norm.bias]

    with pytest.raises(Pose6dError, match="not adjacent"):
        _run(True, order=gap_order)
    _run(False, order=gap_order)                              # the unstacked engine does not care

    def bias_gap(eng):                                        # weights adjacent, biases not
        o = eng.params_in_grad_order()
        o[6], o[8] = o[8], o[6]                               # k bias <-> rgb_norm weight
        return o

    with pytest.raises(Pose6dError, match="not adjacent"):
        _run(True, order=bias_gap)
    torch.cuda.synchronize()
