"""pose6d_layernorm_pair_fwd / _bwd (two LayerNorms in one launch each way) against two calls
of pose6d_layernorm_fwd / _bwd: the same device functions per row and per column, so every
output must be bit-equal.  B = 3, D = 300: D is no multiple of the 256 threads, so the last
column block is partial and the row loops have tails; the outputs are the two halves of a
(B, 2 D) buffer (row stride 2 D > D) plus the contiguous copy."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = (1e-5, 3e-5)   # each norm has its own eps


def _inputs(B, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    return {"x": (r(B, D) * 3 + 1, r(B, D) * 0.5 - 2), "gamma": (r(D), r(D)), "beta": (r(D), r(D)),
            "dy": (r(B, D), r(B, D)), "dy2": r(B, 2 * D)}


def _separate_fwd(t, B, D):
    from pose6d._lib import call, stream
    out = torch.zeros(B, 2 * D, device="cuda")
    y2 = torch.zeros(B, D, device="cuda")
    stats = torch.zeros(4, B, device="cuda")
    for k in (0, 1):
        call("layernorm_fwd", t["x"][k], D, out[:, k * D:], 2 * D, y2 if k == 0 else None, B, D, t["gamma"][k],
             t["beta"][k], EPS[k], 0, 0.0, None, 0, None, stats[2 * k], stats[2 * k + 1], stream())
    return out, y2, stats


def _pair_fwd(t, B, D):
    from pose6d._lib import call, stream
    out = torch.zeros(B, 2 * D, device="cuda")
    y2 = torch.zeros(B, D, device="cuda")
    stats = torch.zeros(4, B, device="cuda")
    call("layernorm_pair_fwd",
         t["x"][0], D, out[:, :D], 2 * D, y2, t["gamma"][0], t["beta"][0], EPS[0], stats[0], stats[1],
         t["x"][1], D, out[:, D:], 2 * D, None, t["gamma"][1], t["beta"][1], EPS[1], stats[2], stats[3],
         B, D, stream())
    return out, y2, stats


def _fill(D):
    """Pre-filled parameter gradients (accumulate = 1 adds onto them, 0 overwrites)."""
    g = torch.Generator().manual_seed(99)
    return [torch.randn(D, generator=g).cuda() for _ in range(4)]


def _bwd(t, stats, B, D, with_dy2, accumulate, paired):
    from pose6d._lib import call, stream
    dx = [torch.full((B, D), 7.0, device="cuda") for _ in range(2)]
    dga, dba, dgb, dbb = _fill(D)
    dy2 = [t["dy2"][:, :D], t["dy2"][:, D:]] if with_dy2 else [None, None]
    ld2 = 2 * D if with_dy2 else 0
    if paired:
        call("layernorm_pair_bwd",
             t["dy"][0], D, dy2[0], ld2, t["x"][0], D, t["gamma"][0], t["beta"][0], stats[0], stats[1], dx[0], D,
             dga, dba,
             t["dy"][1], D, dy2[1], ld2, t["x"][1], D, t["gamma"][1], t["beta"][1], stats[2], stats[3], dx[1], D,
             dgb, dbb, B, D, accumulate, stream())
    else:
        for k, (dg, db) in enumerate(((dga, dba), (dgb, dbb))):
            call("layernorm_bwd", t["dy"][k], D, dy2[k], ld2, t["x"][k], D, B, D, t["gamma"][k], t["beta"][k],
                 stats[2 * k], stats[2 * k + 1], 0, 0.0, None, dx[k], D, 0, dg, db, accumulate, stream())
    torch.cuda.synchronize()
    return dx + [dga, dba, dgb, dbb]


def _check_fwd(B, D):
    t = _inputs(B, D)
    ref, got = _separate_fwd(t, B, D), _pair_fwd(t, B, D)
    torch.cuda.synchronize()
    for a, b, what in zip(got, ref, ("out", "y2", "mean / rstd")):
        assert torch.equal(a, b), what
    assert bool(got[0].abs().sum() > 0) and bool(got[2].abs().min() > 0)
    return t, ref[2]


def test_forward_equals_two_calls():
    _check_fwd(3, 300)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("with_dy2", [False, True], ids=["dy", "dy+dy2"])
def test_backward_equals_two_calls(with_dy2, accumulate):
    B, D = 3, 300
    t, stats = _check_fwd(B, D)
    ref = _bwd(t, stats, B, D, with_dy2, accumulate, paired=False)
    got = _bwd(t, stats, B, D, with_dy2, accumulate, paired=True)
    for a, b, what in zip(got, ref, ("dx a", "dx b", "dgamma a", "dbeta a", "dgamma b", "dbeta b")):
        assert torch.equal(a, b), what
    # the pre-fill is kept exactly when accumulate says so
    fill = _fill(D)
    plain = _bwd(t, stats, B, D, with_dy2, 0, paired=True)
    for a, p, f in zip(got[2:], plain[2:], fill):
        assert torch.equal(a, f + p if accumulate else p)
        assert not torch.equal(p, torch.zeros_like(p))


def test_real_shape():
    B, D = 32, 2048
    t, stats = _check_fwd(B, D)
    ref = _bwd(t, stats, B, D, True, 0, paired=False)
    got = _bwd(t, stats, B, D, True, 0, paired=True)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


def test_argument_checks():
    from pose6d._lib import Pose6dError, call, stream
    B, D = 3, 300
    t = _inputs(B, D)
    out = torch.zeros(B, 2 * D, device="cuda")
    stats = torch.zeros(4, B, device="cuda")
    dx = torch.zeros(B, D, device="cuda")
    pg = _fill(D)

    def fwd(B_, ldy_b):
        call("layernorm_pair_fwd",
             t["x"][0], D, out[:, :D], 2 * D, None, t["gamma"][0], t["beta"][0], 1e-5, stats[0], stats[1],
             t["x"][1], D, out[:, D:], ldy_b, None, t["gamma"][1], t["beta"][1], 1e-5, stats[2], stats[3],
             B_, D, stream())

    def bwd(B_, lddx_a, ld2=2 * D):
        call("layernorm_pair_bwd",
             t["dy"][0], D, t["dy2"][:, :D], ld2, t["x"][0], D, t["gamma"][0], t["beta"][0], stats[0], stats[1], dx,
             lddx_a, pg[0], pg[1],
             t["dy"][1], D, None, 0, t["x"][1], D, t["gamma"][1], t["beta"][1], stats[2], stats[3], dx, D,
             pg[2], pg[3], B_, D, 0, stream())

    with pytest.raises(Pose6dError, match="bad shape"):
        fwd(B, D - 1)                      # an output row stride below D
    with pytest.raises(Pose6dError, match="bad shape"):
        bwd(B, D - 1)
    with pytest.raises(Pose6dError, match="lddy2"):
        bwd(B, D, ld2=D - 1)               # dy2 given with a stride below D
    fwd(0, 2 * D)                          # B = 0: OK, nothing launched
    bwd(0, D)
    torch.cuda.synchronize()
    assert bool((out == 0).all())
