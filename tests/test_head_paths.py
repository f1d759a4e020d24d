"""The fp32 head kernels (csrc/head.hip) on the paths the models run, each against a
float64 reference of the same operation on the same fp32 operands.

pose6d_gemm_f32 picks its kernel and its K split on the host (gemm_f32_impl):

  skinny MFMA kernel   M <= 32, sak == 1 and (sbk == 1 or sbn == 1); one workgroup per
                       16 columns (groups = ceil(N / 16)).  With a workspace, groups < 256
                       and N * K >= 2^20:
                         slices = min(ceil(256 / groups), K // 256, ws_floats // (M * N))
                         kchunk = ceil(ceil(K / slices) / 16) * 16, slices = ceil(K / kchunk)
                       slices > 1: raw partial sums to the workspace ([slices][M][N]) and
                       gemm_splitk_reduce_kernel applies alpha / bias / beta (/ eval BN).
                       VEC (16-byte loads) needs A 16-byte aligned, sam % 4 == 0, K % 4 == 0
                       (and for sbk == 1 the same of B / sbn).
  generic tiled kernel everything else (32 x 64 tiles, tiles = ceil(N / 64) * ceil(M / 32)).
                       With a workspace and tiles < 256:
                         splits = min(ceil(256 / tiles), ceil(K / 128), ws_floats // (M * N))
                         kchunk = ceil(ceil(K / splits) / 32) * 32, splits = ceil(K / kchunk)

The comment beside each shape derives what that shape takes; the split cases also check
it on the workspace itself (NaN-filled before the call: exactly slices * M * N floats are
written, and a partial that was read but never written would surface as a NaN).

Tolerances are the ones tests/test_head_kernels.py already uses for the same operator:
GEMM and weight gradients rtol 1e-5 with atol 1e-5 * max|ref|; bn1d y rtol = atol = 1e-5,
running statistics rtol 1e-5 / atol 1e-6, dx rtol 1e-4 with atol 1e-5 * max(gamma *
invstd) * max|dy|."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, device=DEV, generator=g)


def _gemm_close(got, ref):
    torch.testing.assert_close(got.double(), ref, rtol=1e-5, atol=1e-5 * ref.abs().max().item())


def _nan_ws(n):
    return torch.full((n,), NAN, device=DEV)


def _written(ws):
    return int((~torch.isnan(ws)).sum().item())


def _gemm(A, sam, sak, B, sbk, sbn, C, ldc, bias, M, N, K, alpha=1.0, beta=0.0, ws=None, ws_floats=None):
    from pose6d._lib import call, stream
    if ws_floats is None:
        ws_floats = ws.numel() if ws is not None else 0
    call("gemm_f32", A, sam, sak, B, sbk, sbn, C, ldc, bias, M, N, K, alpha, beta, ws, ws_floats, stream())


def _linear_operands(seed, M, N, K):
    g = _gen(seed)
    return _randn(g, M, K), _randn(g, N, K) * 0.05, _randn(g, N)


# ---- 1. pose6d_gemm_f32: the skinny kernel with K slices -----------------------------
def test_skinny_splitk_forward():
    # M=32 sak=1 sbk=1 -> skinny, VEC on.  groups = 512/16 = 32 < 256, N*K = 2^20:
    # slices = min(ceil(256/32)=8, 2048//256=8, 16) = 8, kchunk = ceil(256/16)*16 = 256,
    # slices = 2048/256 = 8; each wave of a slice takes kc = 16
    M, N, K, slices = 32, 512, 2048, 8
    x, w, b = _linear_operands(1, M, N, K)
    ref = x.double() @ w.double().T + b.double()
    outs = []
    for _ in range(2):
        ws, y = _nan_ws(16 * M * N), _nan_ws(M * N).view(M, N)
        _gemm(x, K, 1, w, 1, K, y, N, b, M, N, K, ws=ws)
        assert _written(ws) == slices * M * N and not bool(torch.isnan(ws[:slices * M * N]).any())
        assert bool(torch.isfinite(y).all())
        _gemm_close(y, ref)
        outs.append(y)
    assert torch.equal(outs[0], outs[1])   # fixed reduce order


def test_skinny_splitk_ragged_scalar_loads():
    # M=17 sak=1 sbk=1 -> skinny; K % 4 = 2 -> VEC off (scalar loads, every k bounds-checked).
    # groups = ceil(520/16) = 33 (the last group has 8 of its 16 columns), N*K = 1066000 >= 2^20:
    # slices = min(ceil(256/33)=8, 2050//256=8, 16) = 8, kchunk = ceil(ceil(2050/8)=257 / 16)*16 = 272,
    # slices = ceil(2050/272) = 8: seven slices of 272 (kc = 32: waves 0..7 full, wave 8 half, the
    # rest empty) and a last one of 2050 - 7*272 = 146 (kc = 16: wave 9 ends 2 into its chunk)
    M, N, K, slices = 17, 520, 2050, 8
    x, w, b = _linear_operands(2, M, N, K)
    ref = x.double() @ w.double().T + b.double()
    outs = []
    for _ in range(2):
        ws, y = _nan_ws(16 * M * N), _nan_ws(M * N).view(M, N)
        _gemm(x, K, 1, w, 1, K, y, N, b, M, N, K, ws=ws)
        assert _written(ws) == slices * M * N
        assert bool(torch.isfinite(y).all())
        _gemm_close(y, ref)
        outs.append(y)
    assert torch.equal(outs[0], outs[1])


def test_skinny_splitk_misaligned_a():
    # A starts 2 floats into rows of 4098: 8-byte aligned, sam % 4 = 2 -> VEC off; N*K = 2^20,
    # groups = 32 -> 8 slices of 256 as in test_skinny_splitk_forward
    M, N, K, slices = 32, 512, 2048, 8
    g = _gen(3)
    big = _randn(g, M, 4098)
    x = big[:, 2:2050]
    w, b = _randn(g, N, K) * 0.05, _randn(g, N)
    ws, y = _nan_ws(16 * M * N), _nan_ws(M * N).view(M, N)
    _gemm(x, 4098, 1, w, 1, K, y, N, b, M, N, K, ws=ws)
    assert _written(ws) == slices * M * N
    _gemm_close(y, x.double() @ w.double().T + b.double())


@pytest.mark.parametrize("ws_rows,slices", [(3, 3), (1, 1)])
def test_skinny_workspace_limits_the_slices(ws_rows, slices):
    # as test_skinny_splitk_forward, but ws_floats // (M*N) caps the 8 slices:
    # 3 -> kchunk = ceil(ceil(2048/3)=683 / 16)*16 = 688, slices = ceil(2048/688) = 3 (688, 688, 672)
    # 1 -> no split: one launch, the workspace is not touched
    M, N, K = 32, 512, 2048
    x, w, b = _linear_operands(4, M, N, K)
    ws, y = _nan_ws(16 * M * N), _nan_ws(M * N).view(M, N)
    _gemm(x, K, 1, w, 1, K, y, N, b, M, N, K, ws=ws, ws_floats=ws_rows * M * N)
    assert _written(ws) == (slices * M * N if slices > 1 else 0)
    assert bool(torch.isnan(ws[ws_rows * M * N:]).all())   # nothing past what the caller offered
    _gemm_close(y, x.double() @ w.double().T + b.double())


def test_skinny_splitk_data_gradient():
    # dx (32 x 2048) = 0.5 * dy (32 x 1024) W (1024 x 2048) + dx: the call's N = 2048, K = 1024,
    # sbk = 2048, sbn = 1 -> skinny, BKC off.  groups = 128 < 256, N*K = 2^21:
    # slices = min(ceil(256/128)=2, 1024//256=4, 16) = 2, kchunk = 512, slices = 2
    M, Kin, Nout, slices = 32, 2048, 1024, 2
    g = _gen(5)
    dy, w, dx = _randn(g, M, Nout), _randn(g, Nout, Kin) * 0.05, _randn(g, M, Kin)
    ref = 0.5 * (dy.double() @ w.double()) + dx.double()
    ws = _nan_ws(16 * M * Kin)
    _gemm(dy, Nout, 1, w, Kin, 1, dx, Kin, None, M, Kin, Nout, alpha=0.5, beta=1.0, ws=ws)
    assert _written(ws) == slices * M * Kin
    _gemm_close(dx, ref)


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("with_bias", [False, True])
def test_splitk_reduce_epilogue(beta, with_bias):
    # 8 slices as in test_skinny_splitk_forward: alpha, bias, beta and the ldc > N store all
    # happen in gemm_splitk_reduce_kernel
    M, N, K, ldc, alpha = 32, 512, 2048, 520, 0.75
    x, w, b = _linear_operands(6, M, N, K)
    bias = b if with_bias else None
    c0 = _randn(_gen(7), M, N)
    C = torch.full((M + 1, ldc), 7.0, device=DEV)          # sentinel: columns >= N, row M
    C[:M, :N] = c0 if beta != 0 else NAN                   # beta == 0 must not read C
    ref = alpha * (x.double() @ w.double().T) + (b.double() if with_bias else 0) + beta * c0.double()
    ws = _nan_ws(16 * M * N)
    _gemm(x, K, 1, w, 1, K, C, ldc, bias, M, N, K, alpha=alpha, beta=beta, ws=ws)
    assert _written(ws) == 8 * M * N
    assert bool(torch.isfinite(C).all())
    _gemm_close(C[:M, :N], ref)
    assert bool((C[:M, N:] == 7.0).all()) and bool((C[M] == 7.0).all())


# ---- the generic tiled kernel ---------------------------------------------------------
# no workspace -> splits = 1, kchunk = K, one launch of gemm_f32_kernel:
#   (33, 100, 70)   M > 32 -> generic; 2 x 2 tiles, one row in the second row tile, K tail 100 - 96 = 4
#   (64, 256, 130)  2 row tiles x 3 column tiles (2 columns in the last), K a multiple of 32
#   (100, 37, 5)    4 row tiles (4 rows in the last), one column tile of 5, K = 32 + 5
@pytest.mark.parametrize("M,K,N", [(33, 100, 70), (64, 256, 130), (100, 37, 5)])
def test_generic_gemm(M, K, N):
    x, w, b = _linear_operands(M + N, M, N, K)
    y = _nan_ws(M * N).view(M, N)
    _gemm(x, K, 1, w, 1, K, y, N, b, M, N, K)
    _gemm_close(y, x.double() @ w.double().T + b.double())
    # data-gradient form (sbn = 1) onto an existing dx
    g = _gen(M)
    dy, dx = _randn(g, M, N), _randn(g, M, K)
    ref = dy.double() @ w.double() + dx.double()
    _gemm(dy, N, 1, w, K, 1, dx, K, None, M, K, N, beta=1.0)
    _gemm_close(dx, ref)


@pytest.mark.parametrize("b_kmajor", [False, True])
def test_generic_gemm_a_kmajor(b_kmajor):
    # M = 16 <= 32 but sak = M != 1 -> generic kernel (A's m-fastest load order); B as the
    # nn.Linear weight [N][K] (sbk = 1) or as [K][N] (sbn = 1)
    M, K, N = 16, 100, 70
    g = _gen(11)
    at, w, b = _randn(g, K, M), _randn(g, N, K) * 0.05, _randn(g, N)    # A(m, k) = at[k][m]
    ref = at.double().T @ w.double().T + b.double()
    y = _nan_ws(M * N).view(M, N)
    if b_kmajor:
        _gemm(at, 1, M, w.T.contiguous(), N, 1, y, N, b, M, N, K)
    else:
        _gemm(at, 1, M, w, 1, K, y, N, b, M, N, K)
    _gemm_close(y, ref)


# with a workspace of 16 * M * N floats:
#   (64, 2048, 1024)  tiles = 16 * 2 = 32: splits = min(ceil(256/32)=8, ceil(2048/128)=16, 16) = 8,
#                     kchunk = ceil(256/32)*32 = 256, splits = 8
#   (33, 300, 70)     tiles = 2 * 2 = 4: splits = min(64, ceil(300/128)=3, 16) = 3,
#                     kchunk = ceil(100/32)*32 = 128, splits = ceil(300/128) = 3 (128, 128, 44: ragged,
#                     and 44 is no multiple of the 32-deep tile)
@pytest.mark.parametrize("M,K,N,splits", [(64, 2048, 1024, 8), (33, 300, 70, 3)])
def test_generic_gemm_splitk(M, K, N, splits):
    x, w, b = _linear_operands(M + K, M, N, K)
    ref = x.double() @ w.double().T + b.double()
    outs = []
    for _ in range(2):
        ws, y = _nan_ws(16 * M * N), _nan_ws(M * N).view(M, N)
        _gemm(x, K, 1, w, 1, K, y, N, b, M, N, K, ws=ws)
        assert _written(ws) == splits * M * N
        assert bool(torch.isfinite(y).all())
        _gemm_close(y, ref)
        outs.append(y)
    assert torch.equal(outs[0], outs[1])


def test_gemm_degenerate_sizes():
    g = _gen(13)
    K = 64
    w, b = _randn(g, 8, K), _randn(g, 8)
    C = torch.full((4, 8), 7.0, device=DEV)
    ws = _nan_ws(1024)
    _gemm(torch.empty(0, K, device=DEV), K, 1, w, 1, K, C, 8, b, 0, 8, K, ws=ws)          # M = 0
    _gemm(_randn(g, 4, K), K, 1, torch.empty(0, K, device=DEV), 1, K, C, 8, None, 4, 0, K, ws=ws)   # N = 0
    assert bool((C == 7.0).all()) and _written(ws) == 0
    # M = 1 (the drop-in modules at batch 1): the 8 slices of test_skinny_splitk_forward, and one launch
    M, N, K = 1, 512, 2048
    x, w, b = _linear_operands(14, M, N, K)
    ref = x.double() @ w.double().T + b.double()
    for ws in (_nan_ws(16 * M * N), None):
        y = _nan_ws(N).view(M, N)
        _gemm(x, K, 1, w, 1, K, y, N, b, M, N, K, ws=ws)
        assert ws is None or _written(ws) == 8 * M * N
        _gemm_close(y, ref)


# ---- 2. pose6d_gemm_f32_bn_eval -------------------------------------------------------
# (2048, 1024): groups = 64, N*K = 2^21 -> slices = min(4, 8, 16) = 4, kchunk = 512: the eval
# BatchNorm runs in the reduce kernel.  (512, 256): N*K = 2^17 < 2^20 -> one launch, the
# BatchNorm runs in the skinny kernel's own epilogue.
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("K,N,slices", [(2048, 1024, 4), (512, 256, 1)])
@pytest.mark.parametrize("M", [1, 32])
def test_gemm_bn_eval(M, K, N, slices, relu):
    from pose6d._lib import call, stream
    eps, ldc = 1e-5, N + 8
    g = _gen(M + K + relu)
    x, w, b = _randn(g, M, K), _randn(g, N, K) * 0.05, _randn(g, N)
    gamma = torch.rand(N, device=DEV, generator=g) + 0.5
    beta, rm = _randn(g, N), _randn(g, N) * 0.1
    rv = torch.rand(N, device=DEV, generator=g) + 0.5
    tiny = torch.arange(N, device=DEV) % 5 == 0
    rv[tiny] = 1e-7                                         # running_var near 0: 1/sqrt(var + eps) ~ 314
    C = torch.full((M + 1, ldc), 7.0, device=DEV)
    C[:M, :N] = NAN
    ws = _nan_ws(16 * M * N)
    call("gemm_f32_bn_eval", x, K, w, C, ldc, b, M, N, K, gamma, beta, rm, rv, eps, relu, ws, ws.numel(), stream())
    assert _written(ws) == (slices * M * N if slices > 1 else 0)
    assert bool((C[:M, N:] == 7.0).all()) and bool((C[M] == 7.0).all())
    got = C[:M, :N]
    # (a) fp64 of relu(bn_eval(x W^T + b)); the channels of ordinary variance once more by
    # themselves, so that the ~314 x larger near-zero-variance channels do not set their scale
    z = x.double() @ w.double().T + b.double()
    ref = (z - rm.double()) / torch.sqrt(rv.double() + eps) * gamma.double() + beta.double()
    if relu:
        ref = torch.relu(ref)
    _gemm_close(got, ref)
    _gemm_close(got[:, ~tiny], ref[:, ~tiny])
    # (b) the header's claim: pose6d_gemm_f32 (same workspace) + pose6d_bn1d_fwd(training = 0), bit for bit
    y_lin, y_bn = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
    sm, si = torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    _gemm(x, K, 1, w, 1, K, y_lin, N, b, M, N, K, ws=ws)
    call("bn1d_fwd", y_lin, y_bn, M, N, gamma, beta, rm, rv, None, 0.1, eps, 0, relu, 0.0, None, 0, None, sm, si,
         stream())
    assert torch.equal(got, y_bn)


def test_gemm_bn_eval_rejects_batch_above_32():
    from pose6d._lib import Pose6dError, call, stream
    M, K, N = 33, 64, 16
    t = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(Pose6dError, match="batch must be 1..32"):
        call("gemm_f32_bn_eval", t(M, K), K, t(N, K), t(M, N), N, t(N), M, N, K, t(N), t(N), t(N), t(N) + 1, 1e-5, 0,
             None, 0, stream())


def _head_seq():
    """the Sequential of test_eval_head_backward_through_autograd, with the same statistics"""
    torch.manual_seed(0)
    seq = torch.nn.Sequential(torch.nn.Linear(256, 128), torch.nn.BatchNorm1d(128), torch.nn.ReLU(),
                              torch.nn.Dropout(0.3), torch.nn.Linear(128, 4)).cuda()
    g = torch.Generator().manual_seed(21)
    bn = seq[1]
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(128, generator=g).cuda() * 0.1)
        bn.running_var.copy_(torch.rand(128, generator=g).cuda() + 0.5)
        bn.weight.copy_(torch.rand(128, generator=g).cuda() + 0.5)
    return seq, g


def _calls_of(fn):
    from pose6d import _lib
    names = []
    ob = lambda name, args: names.append(name)
    _lib.observers.append(ob)
    try:
        out = fn()
    finally:
        _lib.observers.remove(ob)
    return out, names


@pytest.mark.parametrize("B,fused", [(32, True), (33, False)])
def test_head_engine_eval_forward(B, fused):
    """HeadEngine in eval mode, no backward to follow: batch 32 stores Linear + BatchNorm1d +
    ReLU through pose6d_gemm_f32_bn_eval, batch 33 runs the generic GEMM and bn1d_fwd."""
    from pose6d.head import HeadEngine
    seq, g = _head_seq()
    seq.eval()
    x = torch.randn(B, 256, generator=g).cuda()
    out, names = _calls_of(lambda: HeadEngine(seq).forward(x, False, inference=True).clone())
    assert (names == ["gemm_f32_bn_eval", "gemm_f32"]) if fused else (names == ["gemm_f32", "bn1d_fwd", "gemm_f32"])
    ref = copy.deepcopy(seq).double()(x.double())
    torch.testing.assert_close(out.double(), ref, rtol=1e-5, atol=1e-5)


def test_head_engine_train_batch_48():
    """Training forward + backward at a batch above 32 (generic GEMM both ways, bn1d with two
    apply trips) against torch autograd in fp64; dropout off (p = 0)."""
    from pose6d import autograd
    from pose6d.head import HeadEngine
    B = 48
    seq, g = _head_seq()
    seq.train()
    seq[3].p = 0.0
    ref_seq = copy.deepcopy(seq).double()
    x = torch.randn(B, 256, generator=g).cuda().requires_grad_(True)
    dy = torch.randn(B, 4, generator=g).cuda()
    out = autograd.run(HeadEngine(seq), x, True, list(seq.parameters()))
    grads = torch.autograd.grad(out, [x] + list(seq.parameters()), dy)
    xr = x.detach().double().requires_grad_(True)
    h = ref_seq[0](xr)                       # (kept: its gradient scales the first bias gradient's tolerance)
    ref = ref_seq[1:](h)
    rgrads = torch.autograd.grad(ref, [xr] + list(ref_seq.parameters()) + [h], dy.double())
    dh = rgrads[-1]
    torch.testing.assert_close(out.double(), ref, rtol=1e-5, atol=1e-5)
    names = ["x"] + [n for n, _ in seq.named_parameters()]
    for name, a, b in zip(names, grads, rgrads):
        scale = b.abs().max().item()
        if name == "0.bias":
            # a training BatchNorm1d follows: its input gradient sums to exactly 0 over the batch, so
            # this gradient is 0 and the fp64 reference returns its own rounding noise (~1e-21).  What
            # is summed is dh[m][c]: the same 1e-5, of the largest column of |dh| instead of max|ref|
            scale = dh.abs().sum(0).max().item()
        torch.testing.assert_close(a.double(), b, rtol=1e-4, atol=1e-5 * scale)
    bn, rbn = seq[1], ref_seq[1]
    torch.testing.assert_close(bn.running_mean.double(), rbn.running_mean, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(bn.running_var.double(), rbn.running_var, rtol=1e-5, atol=1e-6)
    assert int(bn.num_batches_tracked) == int(rbn.num_batches_tracked) == 1


# ---- 3. act, bn1d, colsum, linear_wgrad -----------------------------------------------
SPECIAL = [0.0, 1e-3, -1e-3, 6.0, -6.0, 12.0, -12.0]


def _act64(z, act):
    return {0: z, 1: torch.relu(z), 2: F.gelu(z)}[act]   # F.gelu: the exact (erf) form


@pytest.mark.parametrize("n", [1, 257, 1000])
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_act_fwd_bwd(act, p, n):
    """Tolerance: rtol 1e-5, atol 2e-6.  Identity, ReLU and the dropout scale are one fp32
    rounding each (rtol).  GELU = 0.5 x (1 + erf(x / sqrt 2)): 1 + erf carries an absolute
    error of a few 2^-24 (erff is good to a few ulp of a value near 1, and the sum rounds
    once more), which the factor 0.5 |x| <= 6 turns into at most ~4 * 6 * 2^-24 = 1.4e-6 where
    the exact value has cancelled to almost nothing (x = -6: -5.9e-9); the derivative
    Phi(x) + x phi(x) carries the same 2^-24-sized error times |dy| / (1 - p) <= 4.3."""
    from pose6d._lib import call, stream
    g = _gen(act * 100 + n)
    x = _randn(g, n) * 2
    k = min(n, len(SPECIAL))
    x[:k] = torch.tensor(SPECIAL[:k], device=DEV)
    dy = _randn(g, n).clamp(-3, 3)
    seed = torch.tensor([(1 << 40) + 17], dtype=torch.int64, device=DEV)
    y, dx = _nan_ws(n), _nan_ws(n)
    mask = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    call("act_fwd", x, y, n, act, p, seed, 9, mask, stream())
    if p > 0:
        assert bool((mask <= 1).all())
    m = mask.double() if p > 0 else torch.ones(n, device=DEV, dtype=torch.float64)
    xr = x.double().requires_grad_(True)
    ref = _act64(xr, act) * m / (1 - p)
    tol = dict(rtol=1e-5, atol=2e-6)
    torch.testing.assert_close(y.double(), ref.detach(), **tol)
    ref.backward(dy.double())
    call("act_bwd", dy, x, dx, n, act, p, mask if p > 0 else None, stream())
    torch.testing.assert_close(dx.double(), xr.grad, **tol)
    through = dy.double() * m / (1 - p)      # the gradient reaching the activation
    if act == 1:
        assert dx[0].item() == 0.0           # ReLU'(0) = 0 (x[0] == 0)
    if act == 2 and n > 6:
        assert bool(torch.isfinite(dx[:7]).all())
        torch.testing.assert_close(dx[5].double(), through[5], **tol)                    # GELU'(12) = 1
        torch.testing.assert_close(dx[6].double(), torch.zeros_like(through[6]), **tol)  # GELU'(-12) = 0


def _bn_operands(g, M, C):
    x = _randn(g, M, C) * 2 + 0.5
    gamma = torch.rand(C, device=DEV, generator=g) + 0.5
    beta, rm = _randn(g, C), _randn(g, C) * 0.1
    rv = torch.rand(C, device=DEV, generator=g) + 0.5
    return x, gamma, beta, rm, rv


# (37, 65): rows 32..36 take a second apply trip of which group 0 has 2 rows and the others 1,
# and column 64 sits alone in a second block; (2, 1): the smallest training batch; (32, 128):
# the product's one full trip
@pytest.mark.parametrize("M,C", [(2, 1), (37, 65), (32, 128)])
@pytest.mark.parametrize("relu", [0, 1])
def test_bn1d_train_dropout_fwd_bwd(relu, M, C):
    from pose6d._lib import call, stream
    p, mom, eps = 0.3, 0.1, 1e-5
    g = _gen(M * 3 + C + relu)
    x, gamma, beta, rm, rv = _bn_operands(g, M, C)
    rm0, rv0 = rm.double().clone(), rv.double().clone()
    nbt = torch.full((1,), 3, device=DEV, dtype=torch.int64)
    seed = torch.tensor([(1 << 35) + 5], dtype=torch.int64, device=DEV)
    y = _nan_ws(M * C).view(M, C)
    mask = torch.full((M, C), 7, dtype=torch.uint8, device=DEV)
    sm, si = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    call("bn1d_fwd", x, y, M, C, gamma, beta, rm, rv, nbt, mom, eps, 1, relu, p, seed, 11, mask, sm, si, stream())
    assert bool((mask <= 1).all())
    m = mask.double()
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z = F.batch_norm(xr, None, None, gr, br, True, mom, eps)
    ref = (torch.relu(z) if relu else z) * m / (1 - p)
    torch.testing.assert_close(y.double(), ref.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(rm.double(), (1 - mom) * rm0 + mom * x.double().mean(0), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(rv.double(), (1 - mom) * rv0 + mom * x.double().var(0, unbiased=True), rtol=1e-5,
                               atol=1e-6)
    assert int(nbt.item()) == 4
    # backward with the forward's mask, parameter gradients accumulated onto what is there
    dy = _randn(g, M, C)
    ref.backward(dy.double())
    dg0, db0 = _randn(g, C), _randn(g, C)
    dg, db = dg0.clone(), db0.clone()
    dx = _nan_ws(M * C).view(M, C)
    call("bn1d_bwd", dy, x, y, M, C, gamma, sm, si, 1, relu, p, mask, dx, dg, db, 1, stream())
    scale = ((gamma * si).max() * dy.abs().max()).item()
    torch.testing.assert_close(dx.double(), xr.grad, rtol=1e-4, atol=1e-5 * scale)
    for got, ref_g in ((dg, gr.grad + dg0.double()), (db, br.grad + db0.double())):
        torch.testing.assert_close(got.double(), ref_g, rtol=1e-5, atol=1e-5 * ref_g.abs().max().item())


@pytest.mark.parametrize("M,C", [(1, 70), (37, 65)])
@pytest.mark.parametrize("relu", [0, 1])
def test_bn1d_eval_fwd_bwd(relu, M, C):
    from pose6d._lib import call, stream
    eps = 1e-5
    g = _gen(M + C + relu)
    x, gamma, beta, rm, rv = _bn_operands(g, M, C)
    rm0, rv0 = rm.clone(), rv.clone()
    nbt = torch.full((1,), 3, device=DEV, dtype=torch.int64)
    y = _nan_ws(M * C).view(M, C)
    sm, si = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    call("bn1d_fwd", x, y, M, C, gamma, beta, rm, rv, nbt, 0.1, eps, 0, relu, 0.0, None, 0, None, sm, si, stream())
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0) and int(nbt.item()) == 3
    assert torch.equal(sm, rm0)
    torch.testing.assert_close(si.double(), 1.0 / torch.sqrt(rv0.double() + eps), rtol=1e-6, atol=0)
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z = F.batch_norm(xr, rm0.double(), rv0.double(), gr, br, False, 0.1, eps)
    ref = torch.relu(z) if relu else z
    torch.testing.assert_close(y.double(), ref.detach(), rtol=1e-5, atol=1e-5)
    dy = _randn(g, M, C)
    ref.backward(dy.double())
    dx = _nan_ws(M * C).view(M, C)
    dg, db = _nan_ws(C), _nan_ws(C)
    call("bn1d_bwd", dy, x, y, M, C, gamma, sm, si, 0, relu, 0.0, None, dx, dg, db, 0, stream())
    # dx = gamma * invstd * dz: no cancellation, yet the same form as the training test
    scale = ((gamma * si).max() * dy.abs().max()).item()
    torch.testing.assert_close(dx.double(), xr.grad, rtol=1e-4, atol=1e-5 * scale)
    dz = dy.double() * (ref.detach() > 0) if relu else dy.double()
    torch.testing.assert_close(dx.double(), gamma.double() * si.double() * dz, rtol=1e-6, atol=0)
    for got, ref_g in ((dg, gr.grad), (db, br.grad)):
        torch.testing.assert_close(got.double(), ref_g, rtol=1e-5, atol=1e-5 * ref_g.abs().max().item())


def test_bn1d_training_rejects_batch_1():
    from pose6d._lib import Pose6dError, call, stream
    C = 8
    t = lambda *s: torch.ones(*s, device=DEV)
    with pytest.raises(Pose6dError, match="more than 1 value per channel"):
        call("bn1d_fwd", t(1, C), t(1, C), 1, C, t(C), t(C), t(C), t(C), None, 0.1, 1e-5, 1, 0, 0.0, None, 0, None,
             t(C), t(C), stream())


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("M,N,ldy", [(5, 3, 3), (32, 300, 512), (0, 7, 7)])
def test_colsum(M, N, ldy, acc):
    from pose6d._lib import call, stream
    g = _gen(M + N + acc)
    dy, db0 = _randn(g, M, ldy), _randn(g, N)
    db = db0.clone()
    call("colsum_f32", dy, ldy, db, M, N, acc, stream())
    if M == 0:
        assert torch.equal(db, db0 if acc else torch.zeros_like(db0))
        return
    ref = dy[:, :N].double().sum(0) + (db0.double() if acc else 0)
    _gemm_close(db, ref)


# (13, 260, 18): 13 rows = one 8-row unrolled trip + 5 single rows; K = 256 + 4: the second column
# block holds one 4-wide chunk (the K tail); N = 18: the second row block has 2 of 16 rows, and
# 18 is no multiple of the 4 rows a thread owns
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("form", ["contiguous", "strided", "x_offset", "no_db"])
def test_linear_wgrad_tails(form, acc):
    from pose6d._lib import call, stream
    Bn, K, N = 13, 260, 18
    g = _gen(17 + acc)
    ldy, ldx = (24, 264) if form == "strided" else (N, K)
    dy_buf = _randn(g, Bn, ldy)
    if form == "x_offset":     # 8-byte aligned x: the scalar-load path (xvec = 0) with ldx % 4 == 0
        flat = _randn(g, Bn * K + 2)
        x = flat[2:].view(Bn, K)
        assert x.data_ptr() % 16 == 8
    else:
        x = _randn(g, Bn, ldx)[:, :K]
    dy = dy_buf[:, :N]
    dw0, db0 = _randn(g, N, K), _randn(g, N)
    dw, db = dw0.clone(), db0.clone()
    call("linear_wgrad", dy_buf, ldy, x, ldx, dw, None if form == "no_db" else db, N, K, Bn, acc, stream())
    ref_w = dy.double().T @ x.double() + (dw0.double() if acc else 0)
    _gemm_close(dw, ref_w)
    if form == "no_db":
        assert torch.equal(db, db0)
    else:
        _gemm_close(db, dy.double().sum(0) + (db0.double() if acc else 0))


@pytest.mark.parametrize("acc", [0, 1])
def test_linear_wgrad_empty_batch(acc):
    from pose6d._lib import call, stream
    K, N = 260, 18
    g = _gen(19)
    dw0, db0 = _randn(g, N, K), _randn(g, N)
    dw, db = dw0.clone(), db0.clone()
    call("linear_wgrad", torch.empty(0, N, device=DEV), N, torch.empty(0, K, device=DEV), K, dw, db, N, K, 0, acc,
         stream())
    if acc:
        assert torch.equal(dw, dw0) and torch.equal(db, db0)
    else:
        assert not bool(dw.any()) and not bool(db.any())
