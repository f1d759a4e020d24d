"""The dropout masks are a documented function, mask = uniform01(seed ^ salt, index) >= p
with p6::uniform01 the splitmix64 finaliser of csrc/common.h: resumed training draws the
same masks only while the index of every kernel (bn1d m*C+c, act i, layernorm b*D+d,
attention b*H*H+i*H+j) and the way the salt is mixed in stay what they are.  The host
restatement (tests/synth.py) is checked on the CPU first, then every kernel's mask must
equal it bit for bit."""
import numpy as np
import pytest
import torch

from tests.synth import dropout_keep, uniform01

# one word below 2^32, one that uses the high half (a kernel that truncated the seed or
# the salt to 32 bits would draw another mask: test_high_bits_matter)
SEEDS = (1234, 0x5DEECE66D1234567)
SALTS = (0, 0xABCDEF012345)
PS = (0.1, 0.5)


# ---- the host function itself (CPU) ------------------------------------------------
def _splitmix_int(seed, i):
    """the same finaliser in Python integers (no wrapping arithmetic to get wrong)"""
    M = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15 * (i + 1)) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    z ^= z >> 31
    return (z >> 40) / float(1 << 24)


def test_host_uniform_matches_integer_arithmetic():
    idx = [0, 1, 2, 255, 256, 65535, 2 ** 31 - 1, 2 ** 31, 2 ** 32 + 5, 2 ** 40 + 3]
    for seed in SEEDS + (0, 2 ** 64 - 1):
        got = uniform01(seed, np.array(idx, np.uint64))
        assert got.dtype == np.float32
        want = np.array([_splitmix_int(seed, i) for i in idx], np.float64)
        assert np.array_equal(got.astype(np.float64), want)   # 24-bit values: exact in fp32


@pytest.mark.parametrize("p", PS)
def test_host_uniform_range_and_keep_rate(p):
    n = 1 << 20
    idx = np.arange(n, dtype=np.uint64)
    # binomial: the kept fraction of n independent draws has standard deviation
    # sqrt(p (1 - p) / n); 6 sigma (the 2^-24 grid of u moves P(u >= p) by < 6e-8)
    bound = 6.0 * np.sqrt(p * (1.0 - p) / n)
    for seed in SEEDS:
        for salt in SALTS:
            u = uniform01(seed ^ salt, idx)
            assert float(u.min()) >= 0.0 and float(u.max()) < 1.0
            keep = dropout_keep(seed, salt, idx, p)
            assert keep.dtype == np.uint8 and np.array_equal(keep, (u >= np.float32(p)).astype(np.uint8))
            assert abs(float(keep.mean()) - (1.0 - p)) <= bound, (seed, salt, float(keep.mean()))


def test_high_bits_matter():
    """What the GPU cases below rely on: the words that differ only above bit 32, the two
    salts and neighbouring indices all give different masks."""
    idx = np.arange(4096, dtype=np.uint64)
    big = SEEDS[1]
    assert not np.array_equal(dropout_keep(big, 0, idx, 0.5), dropout_keep(big & 0xFFFFFFFF, 0, idx, 0.5))
    assert not np.array_equal(dropout_keep(big, SALTS[1], idx, 0.5),
                              dropout_keep(big, SALTS[1] & 0xFFFFFFFF, idx, 0.5))
    assert not np.array_equal(dropout_keep(big, SALTS[0], idx, 0.5), dropout_keep(big, SALTS[1], idx, 0.5))
    assert not np.array_equal(dropout_keep(big, 0, idx, 0.5), dropout_keep(big, 0, idx + np.uint64(1), 0.5))


# ---- the kernels' masks (GPU) ------------------------------------------------------
def _words():
    for seed in SEEDS:
        for salt in SALTS:
            yield seed, salt, torch.tensor([seed], dtype=torch.int64, device="cuda")


def _new_mask(*shape):
    return torch.full(shape, 7, dtype=torch.uint8, device="cuda")   # 7: neither kept nor dropped


def _same(mask, seed, salt, p, what):
    want = dropout_keep(seed, salt, np.arange(mask.numel(), dtype=np.uint64), p).reshape(tuple(mask.shape))
    got = mask.cpu().numpy()
    assert np.array_equal(got, want), f"{what}: seed {seed:#x} salt {salt:#x} p {p}: {int((got != want).sum())} differ"


@pytest.mark.gpu
@pytest.mark.parametrize("p", PS)
def test_bn1d_mask(p):
    from pose6d._lib import call, stream
    M, C = 37, 65    # two apply trips, a ragged row group, a second (one-lane) column block
    x = torch.randn(M, C, generator=torch.Generator().manual_seed(1)).cuda()
    for seed, salt, sd in _words():
        y, mask = torch.empty_like(x), _new_mask(M, C)
        f = lambda v: torch.full((C,), v, device="cuda")
        call("bn1d_fwd", x, y, M, C, f(1.0), f(0.0), f(0.0), f(1.0), None, 0.1, 1e-5, 1, 0, p, sd, salt, mask,
             f(0.0), f(0.0), stream())
        _same(mask, seed, salt, p, "bn1d (index m*C+c)")
        assert torch.equal(y == 0, mask == 0)    # (a normalised N(0,1) sample is never exactly 0)


@pytest.mark.gpu
@pytest.mark.parametrize("p", PS)
def test_act_mask(p):
    from pose6d._lib import call, stream
    n = 1000
    x = torch.randn(n, generator=torch.Generator().manual_seed(2)).cuda()
    for seed, salt, sd in _words():
        y, mask = torch.empty_like(x), _new_mask(n)
        call("act_fwd", x, y, n, 0, p, sd, salt, mask, stream())
        _same(mask, seed, salt, p, "act (index i)")
        assert torch.equal(y == 0, mask == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("p", PS)
def test_layernorm_mask(p):
    from pose6d._lib import call, stream
    B, D, ldx, ldy = 3, 255, 260, 264   # the index is b*D+d whatever the row strides
    x = torch.randn(B, ldx, generator=torch.Generator().manual_seed(3)).cuda()
    gamma, beta = torch.ones(D, device="cuda"), torch.zeros(D, device="cuda")
    for seed, salt, sd in _words():
        y, mask = torch.zeros(B, ldy, device="cuda"), _new_mask(B, D)
        mean, rstd = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
        call("layernorm_fwd", x, ldx, y, ldy, None, B, D, gamma, beta, 1e-5, 0, p, sd, salt, mask, mean, rstd,
             stream())
        _same(mask, seed, salt, p, "layernorm (index b*D+d)")
        assert torch.equal(y[:, :D] == 0, mask == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("p", PS)
def test_xattn_mask(p, strided):
    from pose6d._lib import call, stream
    B, H, hd = 3, 5, 8
    D = H * hd
    ld = D + 3 if strided else D
    g = torch.Generator().manual_seed(4)
    q, k, v = (torch.randn(B, ld, generator=g).cuda() for _ in range(3))
    for seed, salt, sd in _words():
        out, probs, mask = torch.empty(B, ld, device="cuda"), torch.empty(B, H, H, device="cuda"), _new_mask(B, H, H)
        if strided:
            call("xattn_fwd_strided", q, ld, k, ld, v, ld, out, ld, B, H, hd, hd ** -0.5, p, sd, salt, probs, mask,
                 stream())
        else:
            call("xattn_fwd", q, k, v, out, B, H, hd, hd ** -0.5, p, sd, salt, probs, mask, stream())
        _same(mask, seed, salt, p, "xattn (index b*H*H+i*H+j)")
