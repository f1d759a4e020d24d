"""The BatchNorm2d kernels of csrc/bn.hip, called directly through the C ABI and compared
with a numpy restatement of the formulas of the BN section of include/pose6d.h:
  * bn_stats_finalize_kernel / bn_stats_finalize2_kernel  (pose6d_bn_finalize, _dual)
  * bn_eval_finalize_kernel / bn_eval_fold_kernel         (pose6d_bn_finalize eval, pose6d_bn_eval_fold)
  * bn_act_kernel                                         (pose6d_bn_act_fwd_mask)
  * bn_fin_act_kernel                                     (pose6d_bn_finalize_act, flags and fallback)
  * bn_bwd_reduce2_kernel / bn_bwd_finalize_wg_kernel / bn_bwd_apply_kernel
        (pose6d_bn_bwd in its three mask forms, _mask, _mask_dual, _partials)

Yardstick.  Every *_ref function takes a dtype: np.float64 is the reference, np.float32
evaluates the same operations in fp32 (numpy's order of summation).  The statistics
partials handed to a kernel are formed in fp64 and rounded to fp32, and both evaluations
start from those fp32 values, so the rounding of a kernel's inputs is not charged to it.
  * elementwise outputs (out, dy, scale, shift, save_mean, save_invstd, running statistics):
        E = max over channels c of  max_m |x[m, c] - ref[m, c]| / max_m |ref[m, c]|,
    and a kernel must satisfy E(kernel) <= 4 * E(fp32 evaluation) for the same inputs (the
    factor of test_optim_kernels.py: both round the same operations, it absorbs another
    order, an fma, a differently rounded divide or square root).  For bf16 tensors both
    evaluations round to bf16 last; an fp32 tensor's fp64 reference is left in fp64.
  * summed outputs (dgamma, dbeta, the coef rows): |x - ref| <= 1e-5 * sum|terms| + 1e-6
    per channel, the form test_backward_bn_reduce_partials uses for the same sums.
  * exact: dz = dout where the mask is set and +0 elsewhere; mask bits = stored out > 0;
    num_batches_tracked; accumulate = 1 minus accumulate = 0 is the initial value within one
    fp32 rounding of the accumulated result.
  * ceiling: no output, summed ones and coef rows included, exceeds test_bn_act_and_backward's
    tolerances (1e-5 running statistics, 1e-4 fp32, 3e-2 bf16, of the tensor-wide maximum).
test_every_mutant_is_separated shows on the CPU that these bounds tell the formulas from
fifteen near misses.  The recomputed ReLU mask (pose6d_bn_bwd with relu_scale / relu_shift)
is tested with y nudged until |y s + b| >= 2^-6 (|y s| + |b|) everywhere, so the sign of
round_T(fma(y, s, b)) is the fp64 sign for every element: none is left out.

Holes of the earlier coverage and the case that closes each (all against the reference):
  * bn_bwd_reduce2_kernel with grid.x > 1: test_bn_bwd at (530, 1024) (2 channel groups in
    bf16, 4 in fp32) and (4133, 512) fp32 (2), and test_bn_bwd_mask_dual at the same shapes.
  * bn_stats_fold's four-way unrolled loop, short last row in the unrolled body / in the
    tail, rows == 1, M == 1: test_bn_finalize_training at M = 24 609 (770 rows), 32 741
    (1024 rows, 5-pixel last row in the unrolled body), 32 955 (1030 rows, 27-pixel last
    row in the tail), 8193 (257 rows), 5 / 31 / 32 (one row), 33 (1-pixel last row), 1.
  * bn_bwd_finalize_wg_kernel's two-row loop: test_bn_bwd_partials at rows = 257 and 600.
  * ill-conditioned statistics (|mean| 100..1000, std 0.01..1): the "ill" family of
    test_bn_finalize_training; the fp32 E[x^2] - E[x]^2 mutant is caught there only.
  * eval paths: test_bn_finalize_eval, test_bn_eval_fold (C = 8 / 304 / 2048, max_c = 2048
    and 256: the grid-stride loop).
  * res_scale / res_shift, relu = 0: test_bn_act_fwd_mask; accumulate = 1: test_bn_bwd,
    test_bn_bwd_mask_dual, test_bn_bwd_partials; momentum / eps / initial running
    statistics: FIN_HP and fin_inputs.

Measured on an MI355X.  E(kernel) is the family's largest, E(fp32 eval) that of the same case
and output; the ratio is the family's largest E(kernel) / E(fp32 evaluation) over every
output but shift, then over shift; the last column is the largest summed error over its bound.
    family              E(kernel)   E(fp32 eval)   ratio   shift ratio   summed / bound
    finalize/centred    3.570e-06   1.721e-06      1.14    2.07          -
    finalize/ill        4.007e-06   1.087e-05      1.63    1.19          -
    finalize/constant   1.218e-05   1.218e-05      1.00    1.02          -
    finalize_dual       1.029e-06   1.029e-06      1.15    1.00          -
    eval/finalize       5.241e-06   1.692e-05      1.00    0.37          -
    eval/fold           6.568e-05   6.664e-05      1.00    20.05 (a)     -
    act/bf16            4.651e-03   4.651e-03      1.00    -             -
    act/fp32            2.277e-07   2.951e-07      1.00    -             -
    finalize_act/bf16   4.167e-04   5.274e-04      1.00 (b)  4.11 (a)    -
    finalize_act/fp32   2.033e-05   2.033e-05      3.62    1.00          -
    bwd/bf16            3.984e-03   3.984e-03      2.38    -             0.010
    bwd/fp32            2.828e-07   2.828e-07      1.03    -             0.011
    bwd_dual/bf16       3.165e-03   3.165e-03      1.00    -             0.010
    bwd_dual/fp32       1.685e-07   1.714e-07      0.98    -             0.009
    bwd_partials/bf16   2.199e-06   7.716e-04      0.003   -             0.005
    bwd_partials/fp32   1.337e-07   2.823e-07      0.56    -             0.005
(a) shift misses the factor 4 in two cases (eval fold C = 8: 1.901e-06 against 9.479e-08;
    finalize_act bf16 C = 64, M = 1000: 6.536e-06 against 1.591e-06) because beta - mean * scale
    cancels in one channel and the fp32 evaluation's roundings happened to cancel there (scale
    has the evaluation's bits in the first case); both meet shift_excess's operation-count
    bound.  shift_excess is applied to shift in EVERY finalize and eval case, not only these
    two: shift always passes by either bound (the mutants are judged by the same rule); and
    bf16_within likewise to every bf16 `out` of finalize_act.
(b) the bf16 `out` of finalize_act at C = 64, M = 1000 without residual: the fp32 evaluation
    rounds all 64 000 elements as the reference does (E = 0) and the kernel one element the
    other way (3.551e-04 of its channel); it meets bf16_within's bound, under which 0.04 %
    of the elements may differ by one step at all.
The largest ratio under the factor 4 is 3.62 (finalize_act fp32, C = 64, M = 37, `out`: 8.645e-07
against 2.390e-07).  Slowest case: test_bn_bwd at (4133, 512) in bf16, 0.5 s.
"""
import ctypes

import numpy as np
import pytest
import torch

F32, F64 = np.float32, np.float64
GUARD = 4096      # sentinel elements on each side of a guarded buffer
SENTINEL = 12345  # (0xA5 in a byte buffer)
FACTOR = 4.0
CEIL_RUNNING, CEIL_F32, CEIL_BF16 = 1e-5, 1e-4, 3e-2

FIN_M = (1, 5, 31, 32, 33, 8193, 24609, 32741, 32955)
FIN_CASES = [(8, m) for m in FIN_M] + [(72, 1000)]
FIN_FAMILIES = ("centred", "ill", "constant")
FIN_HP = {"default": (0.1, 1e-5), "slow_big_eps": (0.01, 1e-3), "momentum_one": (1.0, 1e-5)}   # momentum, eps
FIN_OUTPUTS = ("scale", "shift", "mean", "invstd", "running_mean", "running_var")
ACT_SHAPES = [(1, 8), (37, 64), (530, 1024)]
ACT_MODES = ("none", "res", "res_affine")
BWD_SHAPES = [(1, 8), (5, 8), (37, 64), (4133, 16), (530, 1024), (4133, 512)]
BWD_FORMS = ("none", "out", "recompute", "bits")
DUAL_SHAPES = [(37, 64), (530, 1024), (4133, 512)]
DTYPES_T = [torch.bfloat16, torch.float32]

# mutant -> the reference function it changes
MUTANTS = {
    "running_var_biased": "fin", "eps_outside_sqrt": "fin", "eps_missing": "fin", "momentum_swapped": "fin",
    "var_ex2_fp32": "fin", "last_row_32": "fin", "shift_no_mean": "fin",
    "res_before_scale": "act", "res_scale_ignored": "act", "relu_before_res": "act",
    "dy_no_mean_dz": "bwd", "dy_no_xhat_term": "bwd", "dgamma_no_invstd": "bwd", "mask_ignored": "bwd",
    "accumulate_overwrites": "bwd",
}


# ------------------------------------------------------------------ number formats
def bf16_round(x):
    """x rounded to bf16 (nearest even, what a kernel's bf16 store does), in x's dtype."""
    x = np.asarray(x)
    r = torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).bfloat16().float().numpy()
    return r.astype(x.dtype)


def _store(v, out_dtype):
    return bf16_round(v) if out_dtype == torch.bfloat16 else v


def _elems(dtype):
    return 8 if dtype == torch.bfloat16 else 4


# ------------------------------------------------------------------ the reference
def partials_ref(y):
    """[2][C][ceil(M / 32)]: per 32 rows of y [M][C] the sum and the M2 about the block's
    mean, formed in fp64 and rounded to fp32: what the conv epilogue hands the finalize."""
    y = np.asarray(y, F64)
    M, C = y.shape
    full, rows = M // 32, -(-M // 32)
    out = np.zeros((2, C, rows), F64)
    if full:
        b = y[:full * 32].reshape(full, 32, C)
        out[0, :, :full] = b.sum(1).T
        out[1, :, :full] = ((b - b.mean(1, keepdims=True)) ** 2).sum(1).T
    if M % 32:
        b = y[full * 32:]
        out[0, :, full] = b.sum(0)
        out[1, :, full] = ((b - b.mean(0)) ** 2).sum(0)
    return out.astype(F32)


def finalize_ref(part, M, gamma, beta, rm, rv, nbt, momentum, eps, dtype, mutant=None):
    """Training finalize from the fp32 partials, every operation in `dtype`: the pooled mean and
    biased variance (Chan's combination of the blocks), invstd, scale, shift, the running
    statistics (unbiased variance when M > 1) and nbt + 1.  momentum / eps are the fp32
    values the kernel is passed."""
    T = np.dtype(dtype).type
    S, Q = np.asarray(part[0], T), np.asarray(part[1], T)
    rows = S.shape[1]
    n = np.full(rows, 32, T)
    if mutant != "last_row_32":
        n[-1] = M - 32 * (rows - 1)
    N, one, mom, e = T(M), T(1), T(F32(momentum)), T(F32(eps))
    g, b, rm, rv = (np.asarray(a, T) for a in (gamma, beta, rm, rv))
    with np.errstate(all="ignore"):
        mean = S.sum(1) / N
        if mutant == "var_ex2_fp32":
            var = (Q + S * S / n).sum(1) / N - mean * mean
        else:
            d = S / n - mean[:, None]
            var = (Q.sum(1) + (n * d * d).sum(1)) / N
        var = np.maximum(var, T(0))
        if mutant == "eps_outside_sqrt":
            inv = one / (np.sqrt(var) + e)
        elif mutant == "eps_missing":
            inv = one / np.sqrt(var)
        else:
            inv = one / np.sqrt(var + e)
        scale = g * inv
        shift = b if mutant == "shift_no_mean" else b - mean * scale
        unb = var if (M <= 1 or mutant == "running_var_biased") else var * N / (N - one)
        a_old, a_new = (mom, one - mom) if mutant == "momentum_swapped" else (one - mom, mom)
        res = dict(scale=scale, shift=shift, mean=mean, invstd=inv, running_mean=a_old * rm + a_new * mean,
                   running_var=a_old * rv + a_new * unb)
    assert all(v.dtype == np.dtype(T) for v in res.values())
    res["nbt"] = None if nbt is None else int(nbt) + 1
    return res


def eval_ref(gamma, beta, rm, rv, eps, dtype):
    T = np.dtype(dtype).type
    g, b, rm, rv = (np.asarray(a, T) for a in (gamma, beta, rm, rv))
    inv = T(1) / np.sqrt(rv + T(F32(eps)))
    scale = g * inv
    return dict(scale=scale, shift=b - rm * scale, mean=rm, invstd=inv)


def act_ref(y, scale, shift, res, rscale, rshift, relu, out_dtype, dtype, mutant=None):
    """act(y * scale + shift [+ res | + res * rscale + rshift]) in `dtype`, rounded to bf16 at the
    end when out_dtype is bf16."""
    T = np.dtype(dtype).type
    y, scale, shift = (np.asarray(a, T) for a in (y, scale, shift))
    if res is not None:
        res = np.asarray(res, T)
    if rscale is not None:
        rscale, rshift = np.asarray(rscale, T), np.asarray(rshift, T)
    if mutant == "res_before_scale" and res is not None:
        v = (y + res) * scale + shift
    else:
        v = y * scale + shift
        if mutant == "relu_before_res" and relu:
            v = np.maximum(v, T(0))
        if res is not None:
            if rscale is None:
                v = v + res
            elif mutant == "res_scale_ignored":
                v = v + (res + rshift)
            else:
                v = v + (res * rscale + rshift)
    if relu and mutant != "relu_before_res":
        v = np.maximum(v, T(0))
    assert v.dtype == np.dtype(T)
    return _store(v, out_dtype)


def bwd_ref(dout, mask, y, mean, invstd, gamma, dg0, db0, accumulate, out_dtype, dtype, mutant=None):
    """dz = dout * mask, dbeta = sum dz, dgamma = sum dz * xhat (on top of dg0 / db0 when
    accumulating), dy = gamma * invstd * (dz - mean(dz) - xhat * mean(dz * xhat)), with the
    fp32 mean / invstd the kernel is handed.  Also the coef rows of pose6d_bn_bwd_partials
    and sum|terms| of the two sums (for the summed outputs' bound)."""
    T = np.dtype(dtype).type
    dout, y, mean, invstd, gamma, dg0, db0 = (np.asarray(a, T) for a in (dout, y, mean, invstd, gamma, dg0, db0))
    dz = dout if mutant == "mask_ignored" else np.where(mask, dout, T(0))
    xhat = (y - mean) * invstd
    t = dz * xhat
    sb, sg = dz.sum(0), t.sum(0)
    M = T(y.shape[0])
    m1, m2 = sb / M, sg / M
    inner = dz
    if mutant != "dy_no_mean_dz":
        inner = inner - m1
    if mutant != "dy_no_xhat_term":
        inner = inner - xhat * m2
    dy = (gamma * invstd) * inner
    dgam = (dz * (y - mean)).sum(0) if mutant == "dgamma_no_invstd" else sg
    dbeta = sb
    terms_g, terms_b = np.abs(t).sum(0), np.abs(dz).sum(0)
    if accumulate:
        terms_g, terms_b = terms_g + np.abs(dg0), terms_b + np.abs(db0)
        if mutant != "accumulate_overwrites":
            dgam, dbeta = dg0 + dgam, db0 + dbeta
    assert dy.dtype == dgam.dtype == np.dtype(T)
    return dict(dz=dz, dy=_store(dy, out_dtype), dgamma=dgam, dbeta=dbeta, coef=np.stack([gamma * invstd, m1, m2]),
                terms_g=terms_g, terms_b=terms_b,
                terms_coef=np.stack([np.abs(gamma * invstd), np.abs(dz).sum(0) / M, np.abs(t).sum(0) / M]))


# ------------------------------------------------------------------ error measures
def chan_err(x, ref):
    """E of the module docstring: the worst channel's max|x - ref| / max|ref| (channels last);
    a non-finite x, or an error where the reference channel is all zero, counts as inf."""
    ref = np.asarray(ref, F64)
    x = np.asarray(x, F64).reshape(-1, ref.shape[-1])
    ref = ref.reshape(-1, ref.shape[-1])
    with np.errstate(all="ignore"):
        d = np.abs(x - ref)
        d[~np.isfinite(d)] = np.inf
        d, s = d.max(0), np.abs(ref).max(0)
        e = np.where(d == 0, 0.0, d / s)
    return float(e.max())


def sum_excess(x, ref, terms):
    """worst channel's |x - ref| / (1e-5 * sum|terms| + 1e-6): <= 1 passes."""
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(x, F64) - np.asarray(ref, F64))
        d[~np.isfinite(d)] = np.inf
    return float((d / (1e-5 * np.asarray(terms, F64) + 1e-6)).max())


def _ratio(e, bound):
    return e / bound if bound > 0 else (0.0 if e == 0 else float("inf"))


def shift_excess(x, ref):
    """shift = beta - mean * scale cancels, and E is relative to what is left, so one channel's
    luck decides E(kernel) / E(fp32 evaluation) (measured: 20 x and 4.1 x where the fp32
    evaluation's product rounding happened to cancel its scale's).  Its own bound, from the
    operation count: at most five roundings reach mean * scale ahead of the subtraction
    (eval: rv + eps, sqrt, divide, gamma * invstd, the product; training: four) and one the
    difference, so |x - ref| <= 2^-24 * (5 |mean * scale| + |shift|).  ref: the fp64 results."""
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(x, F64) - ref["shift"])
        d[~np.isfinite(d)] = np.inf
        bound = 2.0 ** -24 * (5 * np.abs(ref["mean"] * ref["scale"]) + np.abs(ref["shift"])) + 1e-300
        return float((d / bound).max())


def bf16_within(x, v, delta, relu):
    """A bf16 tensor's error is whole bf16 steps, so where the fp32 evaluation happens to round
    every element as the reference does (measured: 64 000 elements, E(fp32 evaluation) = 0)
    the factor 4 allows no step at all, while a kernel whose fp32 value differs in the last
    bits may round one element the other way.  Its own bound: every stored element is the
    bf16 rounding of some value within `delta` (the operation count's fp32 error) of the
    unrounded fp64 result v, i.e. lies between the roundings of act(v - delta) and
    act(v + delta).  That allows a step only where v is within delta of a rounding boundary."""
    lo, hi = v - delta, v + delta
    if relu:
        lo, hi = np.maximum(lo, 0), np.maximum(hi, 0)
    return bool(((bf16_round(lo) <= x) & (x <= bf16_round(hi))).all())


def check_elem(family, case, name, got, ref, e32, ceiling, also_ok=False):
    """E(kernel) <= 4 * E(fp32 evaluation) (or also_ok: shift within shift_excess's bound, a
    fused bf16 output within bf16_within's), and the tensor-wide ceiling."""
    ek = chan_err(got, ref)
    print(f"BN-E | {family} | {case} | {name} | E32 {e32:.3e} | Ek {ek:.3e}")
    assert ek <= FACTOR * e32 or also_ok, \
        f"{family} {case} {name}: E(kernel) {ek:.3e} > 4 * E(fp32 evaluation) {e32:.3e}"
    ref = np.asarray(ref, F64)
    worst = np.abs(np.asarray(got, F64).reshape(ref.shape) - ref).max()
    assert worst <= ceiling * np.abs(ref).max(), f"{family} {case} {name}: {worst:.3e} over the ceiling {ceiling}"


def check_sum(family, case, name, got, ref, terms, ceiling):
    """|x - ref| <= 1e-5 * sum|terms| + 1e-6 per channel, and the tensor-wide ceiling (at M = 4133
    the summed bound alone is up to 3.4 x looser than the fp32 ceiling)."""
    x = sum_excess(got, ref, terms)
    ref = np.asarray(ref, F64)
    worst, scale = np.abs(np.asarray(got, F64) - ref).max(), np.abs(ref).max()
    print(f"BN-S | {family} | {case} | {name} | excess {x:.3e} | of max {worst / (scale + 1e-300):.3e}")
    assert x <= 1.0, f"{family} {case} {name}: {x:.3f} x the bound 1e-5 * sum|terms| + 1e-6"
    assert worst <= ceiling * scale, f"{family} {case} {name}: {worst:.3e} over the ceiling {ceiling} of {scale:.3e}"


# ------------------------------------------------------------------ inputs (built once, read-only)
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        v = make()
        for a in (v.values() if isinstance(v, dict) else v):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def _signs(rng, n):
    return rng.choice(np.array([-1.0, 1.0]), n)


def fin_inputs(family, C, M, out_dtype=torch.float32):
    """partials of a [M][C] tensor of the family (values representable in out_dtype), gamma,
    beta and random initial running statistics."""
    def make():
        rng = np.random.default_rng([FIN_FAMILIES.index(family), C, M])
        if family == "ill":         # |mean| >> std: E[x^2] - E[x]^2 cancels in fp32
            y = _signs(rng, C) * rng.uniform(100, 1000, C) + 10.0 ** rng.uniform(-2, 0, C) * rng.standard_normal((M, C))
        else:
            y = 0.5 + 2.0 * rng.standard_normal((M, C))
        y = _store(y.astype(F32), out_dtype)
        if family == "constant":    # even channels: multiples of 1/8, every block sum exact, variance exactly 0
            y[:, 0::2] = (rng.integers(1, 40, (C + 1) // 2) * _signs(rng, (C + 1) // 2) / 8.0).astype(F32)
        return dict(y=y, part=partials_ref(y), gamma=(_signs(rng, C) * (rng.random(C) + 0.5)).astype(F32),
                    beta=rng.standard_normal(C).astype(F32), rm=rng.standard_normal(C).astype(F32),
                    rv=(rng.random(C) + 0.5).astype(F32))
    return _cached(("fin", family, C, M, out_dtype), make)


def fin_refs(inp, M, momentum, eps, nbt=None, rm=None, rv=None):
    """(fp64 reference, fp32 evaluation, {output: E(fp32 evaluation)}) of a training finalize."""
    out = []
    for T in (F64, F32):
        out.append(finalize_ref(inp["part"], M, inp["gamma"], inp["beta"], inp["rm"] if rm is None else rm[T],
                                inp["rv"] if rv is None else rv[T], nbt, momentum, eps, T))
    return out[0], out[1], {k: chan_err(out[1][k], out[0][k]) for k in FIN_OUTPUTS}


def act_inputs(M, C, dtype):
    def make():
        rng = np.random.default_rng([7, M, C, _elems(dtype)])
        r = lambda *s: rng.standard_normal(s).astype(F32)
        return dict(y=_store(2 * r(M, C), dtype), res=_store(r(M, C), dtype),
                    scale=(_signs(rng, C) * (rng.random(C) + 0.5)).astype(F32), shift=r(C),
                    rscale=(_signs(rng, C) * (rng.random(C) + 0.5)).astype(F32), rshift=r(C))
    return _cached(("act", M, C, dtype), make)


def act_mode_args(inp, mode):
    return (inp["res"] if mode != "none" else None, inp["rscale"] if mode == "res_affine" else None,
            inp["rshift"] if mode == "res_affine" else None)


def sign_margin_ok(y, rs, rb):
    a, b = np.asarray(y, F64) * np.asarray(rs, F64), np.asarray(rb, F64)
    return np.abs(a + b) >= 2.0 ** -6 * (np.abs(a) + np.abs(b))


def unpack_bits(bits, M, C, E):
    return ((bits.astype(np.int64)[:, None] >> np.arange(E)) & 1).reshape(M, C).astype(bool)


def bwd_inputs(M, C, dtype, seed=0):
    """dout, y (nudged so the recomputed ReLU sign is unambiguous everywhere), the fp32 mean /
    invstd / gamma handed to the kernel, a forward output and mask bytes, relu_scale / shift
    and initial dgamma / dbeta."""
    def make():
        E = _elems(dtype)
        rng = np.random.default_rng([11, M, C, E, seed])
        r = lambda *s: rng.standard_normal(s).astype(F32)
        rs, rb = (_signs(rng, C) * (rng.random(C) + 0.5)).astype(F32), r(C)
        y = _store(0.3 + 2 * r(M, C), dtype)
        for _ in range(8):   # nudge, never skip: an offending y moves by half its size
            bad = ~sign_margin_ok(y, rs, rb)
            if not bad.any():
                break
            y[bad] = _store((y[bad] * F32(1.5)).astype(F32), dtype)
        assert sign_margin_ok(y, rs, rb).all()
        return dict(dout=_store(r(M, C), dtype), y=y, mean=(0.3 * r(C)).astype(F32),
                    invstd=(rng.random(C) + 0.5).astype(F32),
                    gamma=(_signs(rng, C) * (rng.random(C) + 0.5)).astype(F32),
                    out=_store(np.maximum(r(M, C), 0), dtype),
                    bits=rng.integers(0, 256, M * C // E, dtype=np.uint8), rs=rs, rb=rb, dg0=r(C), db0=r(C))
    return _cached(("bwd", M, C, dtype, seed), make)


def bwd_mask(inp, form, dtype):
    M, C = inp["y"].shape
    if form == "none":
        return np.ones((M, C), bool)
    if form == "out":
        return inp["out"] > 0
    if form == "recompute":
        return np.asarray(inp["y"], F64) * np.asarray(inp["rs"], F64) + np.asarray(inp["rb"], F64) > 0
    return unpack_bits(inp["bits"], M, C, _elems(dtype))


def bwd_refs(inp, mask, dtype, key):
    """(fp64 reference, fp32 evaluation) of a backward, accumulating: the overwriting results are
    its sums without dg0 / db0."""
    def make():
        a = (inp["dout"], mask, inp["y"], inp["mean"], inp["invstd"], inp["gamma"], inp["dg0"], inp["db0"], 1, dtype)
        return [bwd_ref(*a, T) for T in (F64, F32)]
    return _cached(("bwdref",) + key, make)


def bwd_expected(ref, inp, acc):
    """dgamma, dbeta and their sum|terms| of the fp64 reference for accumulate = acc."""
    if acc:
        return ref["dgamma"], ref["dbeta"], ref["terms_g"], ref["terms_b"]
    dg0, db0 = np.asarray(inp["dg0"], F64), np.asarray(inp["db0"], F64)
    return ref["dgamma"] - dg0, ref["dbeta"] - db0, ref["terms_g"] - np.abs(dg0), ref["terms_b"] - np.abs(db0)


# ------------------------------------------------------------------ A: CPU only
def test_reference_matches_torch_batch_norm():
    """The fp64 reference is F.batch_norm + residual + ReLU and its autograd in double."""
    import torch.nn.functional as F
    M, C = 37, 64
    fi, ai = fin_inputs("centred", C, M), act_inputs(M, C, torch.float32)
    fin = finalize_ref(fi["part"], M, fi["gamma"], fi["beta"], fi["rm"], fi["rv"], 3, 0.01, 1e-3, F64)
    out = act_ref(fi["y"], fin["scale"], fin["shift"], ai["res"], None, None, 1, torch.float32, F64)
    dout = bwd_inputs(M, C, torch.float32)["dout"]
    bw = bwd_ref(dout, out > 0, fi["y"], fin["mean"], fin["invstd"], fi["gamma"], 0 * fi["gamma"], 0 * fi["gamma"], 0,
                 torch.float32, F64)
    t = lambda a: torch.from_numpy(np.asarray(a, F64))
    y, g, b = (t(a).requires_grad_(True) for a in (fi["y"], fi["gamma"], fi["beta"]))
    rm, rv = t(fi["rm"]).clone(), t(fi["rv"]).clone()
    o = F.relu(F.batch_norm(y, rm, rv, g, b, True, float(F32(0.01)), float(F32(1e-3))) + t(ai["res"]))
    o.backward(t(dout))
    # the fp32 partials carry 2^-24 of the block sums: that, not 1e-12, is the agreement
    for got, want in ((out, o.detach()), (bw["dy"], y.grad), (bw["dgamma"], g.grad), (bw["dbeta"], b.grad),
                      (fin["running_mean"], rm), (fin["running_var"], rv)):
        assert chan_err(got, want.numpy()) < 2e-6
    assert fin["nbt"] == 4


def test_fp32_evaluation_is_close():
    """The yardstick itself is small wherever the data is well conditioned: a handful of fp32
    roundings, under 1e-5 of a channel's largest value (ill-conditioned statistics are the
    exception by design: there the fp32 evaluation's variance is only good to ~1e-4)."""
    for family in FIN_FAMILIES:
        inp = fin_inputs(family, 8, 8193)
        e32 = fin_refs(inp, 8193, *FIN_HP["default"])[2]
        print(f"E(fp32 evaluation) finalize {family}: " + "  ".join(f"{k} {v:.2e}" for k, v in e32.items()))
        assert max(e32.values()) < (1e-3 if family == "ill" else 1e-5)
    inp = bwd_inputs(37, 64, torch.float32)
    ref, ev = bwd_refs(inp, bwd_mask(inp, "bits", torch.float32), torch.float32, (37, 64, torch.float32, "bits", 0))
    assert 0 < chan_err(ev["dy"], ref["dy"]) < 1e-5


def _mutant_cases(kind):
    """name -> function(mutant) giving the worst factor by which the mutated fp32 evaluation
    exceeds a bound of the module docstring in that case family."""
    cases = {}
    f32 = torch.float32
    if kind == "fin":
        for family in FIN_FAMILIES:
            for hp, (mom, eps) in FIN_HP.items():
                for M in (33, 8193):
                    def run(mut, family=family, mom=mom, eps=eps, M=M):
                        inp = fin_inputs(family, 8, M)
                        ref, _, e32 = fin_refs(inp, M, mom, eps)
                        got = finalize_ref(inp["part"], M, inp["gamma"], inp["beta"], inp["rm"], inp["rv"], None, mom,
                                           eps, F32, mutant=mut)
                        r = {k: _ratio(chan_err(got[k], ref[k]), FACTOR * e32[k]) for k in FIN_OUTPUTS}
                        r["shift"] = min(r["shift"], shift_excess(got["shift"], ref))   # (either bound passes)
                        return max(r.values())
                    cases[f"{family}/{hp}/M{M}"] = run
    elif kind == "act":
        inp = act_inputs(37, 64, f32)
        for mode in ACT_MODES:
            for relu in (0, 1):
                def run(mut, mode=mode, relu=relu):
                    a = (inp["y"], inp["scale"], inp["shift"]) + act_mode_args(inp, mode) + (relu, f32)
                    ref = act_ref(*a, F64)
                    return _ratio(chan_err(act_ref(*a, F32, mutant=mut), ref), FACTOR * chan_err(act_ref(*a, F32), ref))
                cases[f"{mode}/relu{relu}"] = run
    else:
        inp = bwd_inputs(37, 64, f32)
        for form in BWD_FORMS:
            for acc in (0, 1):
                def run(mut, form=form, acc=acc):
                    mask = bwd_mask(inp, form, f32)
                    a = (inp["dout"], mask, inp["y"], inp["mean"], inp["invstd"], inp["gamma"], inp["dg0"], inp["db0"],
                         acc, f32)
                    ref, ev, got = bwd_ref(*a, F64), bwd_ref(*a, F32), bwd_ref(*a, F32, mutant=mut)
                    return max(_ratio(chan_err(got["dy"], ref["dy"]), FACTOR * chan_err(ev["dy"], ref["dy"])),
                               float("inf") if not np.array_equal(got["dz"], ref["dz"]) else 0.0,
                               sum_excess(got["dgamma"], ref["dgamma"], ref["terms_g"]),
                               sum_excess(got["dbeta"], ref["dbeta"], ref["terms_b"]))
                cases[f"{form}/acc{acc}"] = run
    return cases


def test_every_mutant_is_separated():
    """Every mutant of the fp32 evaluation exceeds a bound of the module docstring by more than
    10 x in at least one case family; the unmutated evaluation exceeds none.  The fp32
    E[x^2] - E[x]^2 variance is caught by the ill-conditioned family and by no other."""
    cases = {kind: _mutant_cases(kind) for kind in ("fin", "act", "bwd")}
    for kind, cs in cases.items():
        for name, run in cs.items():
            assert run(None) <= 1.0, (kind, name, run(None))
    for mut, kind in MUTANTS.items():
        ratio = {name: run(mut) for name, run in cases[kind].items()}
        best = max(ratio, key=ratio.get)
        print(f"{mut:22s} separated by {best:28s} {ratio[best]:10.3g} x the bound")
        assert ratio[best] > 10, (mut, best, ratio[best])
        if mut == "var_ex2_fp32":
            assert best.startswith("ill/")
            assert all(v <= 1 for k, v in ratio.items() if not k.startswith("ill/")), ratio


# ------------------------------------------------------------------ GPU helpers
class Guarded:
    """n elements in the middle of a larger allocation (the view starts 16-byte aligned) with
    sentinel bands of GUARD elements on both sides."""

    def __init__(self, n, dtype=torch.float32, init=None):
        self.n = n
        fill = 0xA5 if dtype == torch.uint8 else SENTINEL
        self.whole = torch.full((n + 2 * GUARD,), fill, device="cuda", dtype=dtype)
        self.fill = self.whole[0].clone()
        self.t = self.whole[GUARD:GUARD + n]
        assert self.t.data_ptr() % 16 == 0
        if init is not None:
            self.t.copy_(init if isinstance(init, torch.Tensor) else torch.from_numpy(np.array(init)))

    def intact(self):
        return bool((self.whole[:GUARD] == self.fill).all()) and bool((self.whole[GUARD + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.whole == self.fill).all())

    def np(self, *shape):
        t = self.t.float() if self.t.is_floating_point() else self.t
        return t.cpu().numpy().reshape(*shape) if shape else t.cpu().numpy()


def _settle(*bufs):
    torch.cuda.synchronize()
    for b in bufs:
        assert b is None or b.intact(), "guard band overwritten"


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).cuda()   # (a copy: the shared inputs are read-only)
    return t if dtype is None else t.to(dtype)


def _ceil(dtype):
    return CEIL_BF16 if dtype == torch.bfloat16 else CEIL_F32


def _tname(dtype):
    return "bf16" if dtype == torch.bfloat16 else "fp32"


def _fin_outputs(C):
    return {k: Guarded(C) for k in ("scale", "shift", "mean", "invstd")}


def _check_fin(family, case, ref, e32, outs, rm, rv, stats_ceiling=CEIL_F32):
    got = {k: o.np() for k, o in outs.items()}
    got.update(running_mean=rm.np(), running_var=rv.np())
    for k in FIN_OUTPUTS:
        check_elem(family, case, k, got[k], ref[k], e32[k], CEIL_RUNNING if k.startswith("running") else stats_ceiling,
                   also_ok=k == "shift" and shift_excess(got[k], ref) <= 1)


# ------------------------------------------------------------------ B: training finalize
@pytest.mark.gpu
@pytest.mark.parametrize("C,M", FIN_CASES)
@pytest.mark.parametrize("family", FIN_FAMILIES)
def test_bn_finalize_training(family, C, M):
    from pose6d._lib import call, stream
    inp = fin_inputs(family, C, M)
    rows = inp["part"].shape[2]
    assert rows == -(-M // 32)
    part, gamma, beta = _dev(inp["part"]), _dev(inp["gamma"]), _dev(inp["beta"])
    for hp, (mom, eps) in FIN_HP.items():
        ref, _, e32 = fin_refs(inp, M, mom, eps, nbt=41)
        for with_nbt in (True, False):
            outs = _fin_outputs(C)
            rm, rv = Guarded(C, init=inp["rm"]), Guarded(C, init=inp["rv"])
            nbt = Guarded(1, torch.int64, init=[41]) if with_nbt else None
            call("bn_finalize", part, rows, C, M, gamma, beta, rm.t, rv.t, nbt.t if with_nbt else None, mom, eps, 1,
                 outs["scale"].t, outs["shift"].t, outs["mean"].t, outs["invstd"].t, None, stream())
            _settle(rm, rv, nbt, *outs.values())
            _check_fin(f"finalize/{family}", f"C{C} M{M} {hp}", ref, e32, outs, rm, rv)
            assert nbt is None or int(nbt.t.item()) == ref["nbt"] == 42
            if family == "constant":   # variance exactly 0: invstd is 1 / sqrt(eps) to the last bit
                want = F32(1.0 / np.sqrt(np.float64(F32(eps))))
                assert (outs["invstd"].np()[0::2] == want).all()


@pytest.mark.gpu
def test_bn_finalize_dual():
    """Two BatchNorms of different C, momentum and eps in one launch, each against the reference."""
    from pose6d._lib import call, stream
    from pose6d.trunk import _BnStats
    M, rows = 1000, 32
    bns = [("centred", 64, 0.1, 1e-5, 7), ("ill", 8, 0.01, 1e-3, None)]
    keep, structs, state = [], [], []
    for family, C, mom, eps, nbt0 in bns:
        inp = fin_inputs(family, C, M)
        outs = _fin_outputs(C)
        rm, rv = Guarded(C, init=inp["rm"]), Guarded(C, init=inp["rv"])
        nbt = Guarded(1, torch.int64, init=[nbt0]) if nbt0 is not None else None
        dev = [_dev(inp[k]) for k in ("part", "gamma", "beta")]
        keep.append(dev)
        structs.append(_BnStats(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), rm.t.data_ptr(),
                                rv.t.data_ptr(), nbt.t.data_ptr() if nbt else None, outs["scale"].t.data_ptr(),
                                outs["shift"].t.data_ptr(), outs["mean"].t.data_ptr(), outs["invstd"].t.data_ptr(),
                                mom, eps, C))
        state.append((outs, rm, rv, nbt))
    call("bn_finalize_dual", ctypes.addressof(structs[0]), ctypes.addressof(structs[1]), rows, M, stream())
    for (family, C, mom, eps, nbt0), (outs, rm, rv, nbt) in zip(bns, state):
        _settle(rm, rv, nbt, *outs.values())
        ref, _, e32 = fin_refs(fin_inputs(family, C, M), M, mom, eps, nbt=nbt0)
        _check_fin("finalize_dual", f"{family} C{C}", ref, e32, outs, rm, rv)
        assert nbt is None or int(nbt.t.item()) == nbt0 + 1


# ------------------------------------------------------------------ C: eval
def _eval_inputs(C, seed):
    rng = np.random.default_rng([13, C, seed])
    return dict(gamma=(_signs(rng, C) * (rng.random(C) + 0.5)).astype(F32), beta=rng.standard_normal(C).astype(F32),
                rm=rng.standard_normal(C).astype(F32), rv=(10.0 ** rng.uniform(-3, 1, C)).astype(F32))


def _check_eval(family, case, inp, eps, outs, rm, rv):
    ref, ev = (eval_ref(inp["gamma"], inp["beta"], inp["rm"], inp["rv"], eps, T) for T in (F64, F32))
    for k, o in outs.items():
        check_elem(family, case, k, o.np(), ref[k], chan_err(ev[k], ref[k]), CEIL_F32,
                   also_ok=k == "shift" and shift_excess(o.np(), ref) <= 1)
    assert np.array_equal(rm.np().view(np.int32), inp["rm"].view(np.int32)), "running_mean changed in eval"
    assert np.array_equal(rv.np().view(np.int32), inp["rv"].view(np.int32)), "running_var changed in eval"


@pytest.mark.gpu
@pytest.mark.parametrize("C", [8, 257 * 8])
def test_bn_finalize_eval(C):
    from pose6d._lib import call, stream
    inp, eps = _eval_inputs(C, 0), 1e-3
    outs = _fin_outputs(C)
    rm, rv = Guarded(C, init=inp["rm"]), Guarded(C, init=inp["rv"])
    nbt = Guarded(1, torch.int64, init=[5])
    call("bn_finalize", None, 0, C, 0, _dev(inp["gamma"]), _dev(inp["beta"]), rm.t, rv.t, nbt.t, 0.1, eps, 0,
         outs["scale"].t, outs["shift"].t, outs["mean"].t, outs["invstd"].t, None, stream())
    _settle(rm, rv, nbt, *outs.values())
    _check_eval("eval/finalize", f"C{C}", inp, eps, outs, rm, rv)
    assert int(nbt.t.item()) == 5


@pytest.mark.gpu
@pytest.mark.parametrize("max_c", [2048, 256])
def test_bn_eval_fold(max_c):
    """A three-entry table with its own C and eps per entry; with max_c = 256 below two entries'
    C the grid-stride loop must still cover every channel."""
    from pose6d._lib import call, query, stream
    from pose6d.trunk import _FOLD
    assert query("bn_fold_desc_size") == _FOLD.itemsize
    table = [(8, 1e-5), (304, 1e-3), (2048, 1e-2)]
    rec = np.zeros(len(table), dtype=_FOLD)
    state = []
    for i, (C, eps) in enumerate(table):
        inp = _eval_inputs(C, 1 + i)
        outs = _fin_outputs(C)
        rm, rv = Guarded(C, init=inp["rm"]), Guarded(C, init=inp["rv"])
        g, b = _dev(inp["gamma"]), _dev(inp["beta"])
        rec[i] = (g.data_ptr(), b.data_ptr(), rm.t.data_ptr(), rv.t.data_ptr(), outs["scale"].t.data_ptr(),
                  outs["shift"].t.data_ptr(), outs["mean"].t.data_ptr(), outs["invstd"].t.data_ptr(), eps, C)
        state.append((inp, outs, rm, rv, g, b))
    descs = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    call("bn_eval_fold", descs, len(table), max_c, stream())
    for (C, eps), (inp, outs, rm, rv, _, _) in zip(table, state):
        _settle(rm, rv, *outs.values())
        _check_eval("eval/fold", f"C{C} max_c{max_c}", inp, eps, outs, rm, rv)


# ------------------------------------------------------------------ D: apply forward
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES_T)
@pytest.mark.parametrize("M,C", ACT_SHAPES)
def test_bn_act_fwd_mask(M, C, dtype):
    from pose6d._lib import call, stream
    from pose6d.trunk import DTYPES
    inp, E = act_inputs(M, C, dtype), _elems(dtype)
    y, scale, shift = _dev(inp["y"], dtype), _dev(inp["scale"]), _dev(inp["shift"])
    dev = dict(res=_dev(inp["res"], dtype), rscale=_dev(inp["rscale"]), rshift=_dev(inp["rshift"]))
    for mode in ACT_MODES:
        res, rscale, rshift = act_mode_args(dev, mode)
        for relu in (0, 1):
            a = (inp["y"], inp["scale"], inp["shift"]) + act_mode_args(inp, mode) + (relu, dtype)
            ref = act_ref(*a, F64)
            e32 = chan_err(act_ref(*a, F32), ref)
            for with_mask in (True, False):
                out = Guarded(M * C, dtype)
                mb = Guarded(M * C // E, torch.uint8) if with_mask else None
                call("bn_act_fwd_mask", DTYPES[dtype], y, scale, shift, res, rscale, rshift, relu, out.t,
                     mb.t if with_mask else None, M, C, stream())
                _settle(out, mb)
                check_elem(f"act/{_tname(dtype)}", f"M{M} C{C} {mode} relu{relu}", "out", out.np(M, C), ref, e32,
                           _ceil(dtype))
                if with_mask:   # the bits are the sign of what was stored, exactly
                    assert np.array_equal(unpack_bits(mb.np(), M, C, E), out.np(M, C) > 0)
                    assert relu or (out.np() < 0).any()


# ------------------------------------------------------------------ E: finalize + apply in one launch
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES_T)
@pytest.mark.parametrize("M", [37, 1000])
@pytest.mark.parametrize("C", [64, 192])
def test_bn_finalize_act(C, M, dtype):
    """The fused launch against the reference, with and without residual, with the ready flags
    (epoch 0, 1) and through the apply workgroups' own fold (epoch -5, -4); the second call
    on the same flags continues the running statistics of the first."""
    from pose6d._lib import call, query, stream
    from pose6d.trunk import DTYPES, _BnStats
    inp, E = fin_inputs("centred", C, M, dtype), _elems(dtype)
    rows, (mom, eps) = inp["part"].shape[2], FIN_HP["slow_big_eps"]
    res_h = act_inputs(1000, 1024, dtype)["res"][:M, :C]
    part, gamma, beta, y, res_d = (_dev(inp["part"]), _dev(inp["gamma"]), _dev(inp["beta"]), _dev(inp["y"], dtype),
                                   _dev(res_h, dtype))
    nflags = query("bn_finalize_act_flags", rows, C)
    assert nflags >= 1
    for with_res in (False, True):
        for epoch0 in (0, -5):
            outs = _fin_outputs(C)
            rm, rv = Guarded(C, init=inp["rm"]), Guarded(C, init=inp["rv"])
            nbt = Guarded(1, torch.int64, init=[0])
            flags = Guarded(nflags, torch.int32, init=np.zeros(nflags, np.int32))
            epoch = torch.full((1,), epoch0, device="cuda", dtype=torch.int64)
            st = _BnStats(part.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm.t.data_ptr(), rv.t.data_ptr(),
                          nbt.t.data_ptr(), outs["scale"].t.data_ptr(), outs["shift"].t.data_ptr(),
                          outs["mean"].t.data_ptr(), outs["invstd"].t.data_ptr(), mom, eps, C)
            run = {F64: inp["rm"], F32: inp["rm"]}, {F64: inp["rv"], F32: inp["rv"]}
            for k in range(2):
                ref, ev, e32 = fin_refs(inp, M, mom, eps, nbt=k, rm=run[0], rv=run[1])
                run = ({F64: ref["running_mean"], F32: ev["running_mean"]},
                       {F64: ref["running_var"], F32: ev["running_var"]})
                tail = (res_h if with_res else None, None, None, 1, dtype)
                oref = act_ref(inp["y"], ref["scale"], ref["shift"], *tail, F64)
                oe32 = chan_err(act_ref(inp["y"], ev["scale"], ev["shift"], *tail, F32), oref)
                out, mb = Guarded(M * C, dtype), Guarded(M * C // E, torch.uint8)
                call("bn_finalize_act", DTYPES[dtype], ctypes.addressof(st), rows, M, y, res_d if with_res else None,
                     1, out.t, mb.t, flags.t, epoch, stream())
                _settle(rm, rv, nbt, flags, out, mb, *outs.values())
                fam = f"finalize_act/{_tname(dtype)}"
                case = f"C{C} M{M} res{int(with_res)} epoch{epoch0 + k}"
                _check_fin(fam, case, ref, e32, outs, rm, rv)
                ok = False
                if dtype == torch.bfloat16:
                    # fp32 error ahead of the bf16 store, in units of 2^-24: scale carries two roundings
                    # (invstd, gamma * invstd) into y * scale, shift its own bound (shift_excess), the
                    # fma and the residual add one each of the result
                    v = act_ref(inp["y"], ref["scale"], ref["shift"], tail[0], None, None, 0, torch.float32, F64)
                    delta = 2.0 ** -24 * (2 * np.abs(inp["y"] * ref["scale"]) + 5 * np.abs(ref["mean"] * ref["scale"])
                                          + np.abs(ref["shift"]) + 2 * np.abs(v))
                    ok = bf16_within(out.np(M, C), v, delta, 1)
                check_elem(fam, case, "out", out.np(M, C), oref, oe32, _ceil(dtype), also_ok=ok)
                assert np.array_equal(unpack_bits(mb.np(), M, C, E), out.np(M, C) > 0)
                assert int(nbt.t.item()) == k + 1
                epoch += 1


# ------------------------------------------------------------------ F: backward
def _bwd_dev(inp, dtype):
    d = {k: _dev(inp[k], dtype) for k in ("dout", "y", "out")}
    d.update({k: _dev(inp[k]) for k in ("mean", "invstd", "gamma", "bits", "rs", "rb")})
    return d


def _check_bwd(family, case, inp, ref, ev, acc, dtype, dy, dg, db, dz=None):
    M, C = inp["y"].shape
    check_elem(family, case, "dy", dy.np(M, C), ref["dy"], chan_err(ev["dy"], ref["dy"]), _ceil(dtype))
    want_g, want_b, terms_g, terms_b = bwd_expected(ref, inp, acc)
    check_sum(family, case, "dgamma", dg.np(), want_g, terms_g, _ceil(dtype))
    check_sum(family, case, "dbeta", db.np(), want_b, terms_b, _ceil(dtype))
    if dz is not None:   # exact: dout where the mask is set, +0 elsewhere
        assert np.array_equal(dz.np(M, C).view(np.int32), np.asarray(ref["dz"], F32).view(np.int32)), f"{case}: dz"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES_T)
@pytest.mark.parametrize("M,C", BWD_SHAPES)
def test_bn_bwd(M, C, dtype):
    """pose6d_bn_bwd without mask, with the forward output read, with the mask recomputed from y,
    and pose6d_bn_bwd_mask; written and accumulated, with and without dz_out."""
    from pose6d._lib import call, query, stream
    from pose6d.trunk import DTYPES
    inp = bwd_inputs(M, C, dtype)
    d, dt = _bwd_dev(inp, dtype), DTYPES[dtype]
    nws = (query("bn_bwd_workspace_rows", M) * 2 + 3) * C
    assert sign_margin_ok(inp["y"], inp["rs"], inp["rb"]).all()   # share of excluded elements: 0
    for form in BWD_FORMS:
        mask = bwd_mask(inp, form, dtype)
        ref, ev = bwd_refs(inp, mask, dtype, (M, C, dtype, form, 0))
        results = {}
        for acc in (0, 1):
            for with_dz in (True, False):
                dy, dz = Guarded(M * C, dtype), Guarded(M * C, dtype) if with_dz else None
                dg, db, ws = Guarded(C, init=inp["dg0"]), Guarded(C, init=inp["db0"]), Guarded(nws)
                tail = (d["y"], d["mean"], d["invstd"], d["gamma"], dg.t, db.t, acc, dy.t, dz.t if with_dz else None,
                        ws.t, M, C, stream())
                if form == "bits":
                    call("bn_bwd_mask", dt, d["dout"], d["bits"], *tail)
                else:
                    call("bn_bwd", dt, d["dout"], d["out"] if form == "out" else None,
                         d["rs"] if form == "recompute" else None, d["rb"] if form == "recompute" else None, *tail)
                _settle(dy, dz, dg, db, ws)
                _check_bwd(f"bwd/{_tname(dtype)}", f"M{M} C{C} {form} acc{acc} dz{int(with_dz)}", inp, ref, ev, acc,
                           dtype, dy, dg, db, dz)
                results[acc, with_dz] = (dg.np().astype(F64), db.np().astype(F64))
        # accumulated - written = the initial value within one rounding: the kernel adds the same fp64
        # sum, rounded to fp32 once (got0 is that addend exactly), to the initial value, so
        # got1 = fl(init + got0) and only that last addition's half ulp of got1 is charged
        for with_dz in (True, False):
            for got1, got0, init in zip(results[1, with_dz], results[0, with_dz], (inp["dg0"], inp["db0"])):
                assert (np.abs(got1 - got0 - init) <= 2.0 ** -24 * np.abs(got1)).all(), (form, with_dz)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES_T)
@pytest.mark.parametrize("M,C", DUAL_SHAPES)
def test_bn_bwd_mask_dual(M, C, dtype):
    """Both BatchNorms of the dual backward against the reference (not against each other); the
    second has its own y / mean / invstd / gamma."""
    from pose6d._lib import call, query, stream
    from pose6d.trunk import DTYPES
    a, b = bwd_inputs(M, C, dtype), dict(bwd_inputs(M, C, dtype, seed=1))
    b.update(dout=a["dout"], bits=a["bits"])
    da, db_ = _bwd_dev(a, dtype), _bwd_dev(b, dtype)
    mask = bwd_mask(a, "bits", dtype)
    refs = [bwd_refs(a, mask, dtype, (M, C, dtype, "bits", 0)), bwd_refs(b, mask, dtype, (M, C, dtype, "bits", 1))]
    nws = 2 * (query("bn_bwd_workspace_rows", M) * 2 + 3) * C
    for acc in (0, 1):
        o = [(Guarded(M * C, dtype), Guarded(C, init=i["dg0"]), Guarded(C, init=i["db0"])) for i in (a, b)]
        ws = Guarded(nws)
        call("bn_bwd_mask_dual", DTYPES[dtype], da["dout"], da["bits"], da["y"], da["mean"], da["invstd"], da["gamma"],
             o[0][1].t, o[0][2].t, o[0][0].t, db_["y"], db_["mean"], db_["invstd"], db_["gamma"], o[1][1].t, o[1][2].t,
             o[1][0].t, acc, ws.t, M, C, stream())
        _settle(ws, *o[0], *o[1])
        for i, (inp, (ref, ev)) in enumerate(zip((a, b), refs)):
            _check_bwd(f"bwd_dual/{_tname(dtype)}", f"M{M} C{C} bn{i + 1} acc{acc}", inp, ref, ev, acc, dtype, *o[i])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,C", [(torch.float32, 12), (torch.bfloat16, 12), (torch.float32, 24),
                                     (torch.bfloat16, 768)])
def test_bn_bwd_refuses_unsupported_channel_counts(dtype, C):
    """C that is no multiple of 8, or whose 16-byte chunks per row do not tile a workgroup, is
    refused before any launch: every output keeps its sentinels."""
    from pose6d._lib import Pose6dError, call, stream
    from pose6d.trunk import DTYPES
    M, dt = 5, DTYPES[dtype]
    x = torch.ones(M * C, device="cuda", dtype=dtype)
    v = torch.ones(C, device="cuda")
    bits = torch.zeros(M * C, device="cuda", dtype=torch.uint8)
    outs = [Guarded(M * C, dtype), Guarded(M * C, dtype), Guarded(M * C, dtype), Guarded(C), Guarded(C), Guarded(C),
            Guarded(C), Guarded(2 * 5 * C)]
    dy, dz, dy2, dg, db, dg2, db2, ws = (o.t for o in outs)
    with pytest.raises(Pose6dError):
        call("bn_bwd", dt, x, None, None, None, x, v, v, v, dg, db, 0, dy, dz, ws, M, C, stream())
    with pytest.raises(Pose6dError):
        call("bn_bwd", dt, x, x, None, None, x, v, v, v, dg, db, 1, dy, dz, ws, M, C, stream())
    with pytest.raises(Pose6dError):
        call("bn_bwd_mask", dt, x, bits, x, v, v, v, dg, db, 0, dy, dz, ws, M, C, stream())
    with pytest.raises(Pose6dError):
        call("bn_bwd_mask_dual", dt, x, bits, x, v, v, v, dg, db, dy, x, v, v, v, dg2, db2, dy2, 0, ws, M, C, stream())
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)


# ------------------------------------------------------------------ G: backward from given partials
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES_T)
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 600])
def test_bn_bwd_partials(rows, dtype):
    """pose6d_bn_bwd_partials fed partials made here: the M rows split into `rows` contiguous
    groups of unequal size, each group's (sum dz, sum dz * xhat) formed in fp64 and rounded
    to fp32.  rows = 257 and 600 reach the finalize's two-row loop, which pose6d_bn_bwd's
    own reduce (at most 256 row blocks) never does."""
    from pose6d._lib import call, stream
    from pose6d.trunk import DTYPES
    M, C = 1200, 64
    a, b = bwd_inputs(M, C, dtype), dict(bwd_inputs(M, C, dtype, seed=1))
    b.update(dout=a["dout"], bits=a["bits"])
    da, db_ = _bwd_dev(a, dtype), _bwd_dev(b, dtype)
    rng = np.random.default_rng(rows)
    starts = np.concatenate([[0], np.sort(rng.choice(np.arange(1, M), rows - 1, replace=False))]).astype(np.int64)
    assert len(set(np.diff(np.append(starts, M)))) > 1 or rows == 1

    def partials(inp, mask):
        dz = np.where(mask, inp["dout"], 0).astype(F64)
        xhat = (inp["y"].astype(F64) - inp["mean"].astype(F64)) * inp["invstd"].astype(F64)
        p = np.stack([np.add.reduceat(dz, starts, axis=0).T, np.add.reduceat(dz * xhat, starts, axis=0).T])
        assert p.shape == (2, C, rows)
        return _dev(np.ascontiguousarray(p.astype(F32)))

    for kind in ("bits", "recompute", "dual"):
        form = "recompute" if kind == "recompute" else "bits"
        mask = bwd_mask(a, form, dtype)
        refs = [bwd_refs(a, mask, dtype, (M, C, dtype, form, 0))]
        parts = [partials(a, mask)]
        if kind == "dual":
            refs.append(bwd_refs(b, mask, dtype, (M, C, dtype, "bits", 1)))
            parts.append(partials(b, mask))
        for acc in (0, 1):
            o = [(Guarded(M * C, dtype), Guarded(C, init=i["dg0"]), Guarded(C, init=i["db0"])) for i in (a, b)]
            coef = Guarded(6 * C if kind == "dual" else 3 * C)
            dual = kind == "dual"
            call("bn_bwd_partials", DTYPES[dtype], parts[0], rows, da["dout"], da["bits"] if form == "bits" else None,
                 None if form == "bits" else da["rs"], None if form == "bits" else da["rb"], da["y"], da["mean"],
                 da["invstd"], da["gamma"], o[0][1].t, o[0][2].t, o[0][0].t, parts[1] if dual else None,
                 db_["y"] if dual else None, db_["mean"] if dual else None, db_["invstd"] if dual else None,
                 db_["gamma"] if dual else None, o[1][1].t if dual else None, o[1][2].t if dual else None,
                 o[1][0].t if dual else None, acc, coef.t, M, C, stream())
            _settle(coef, *o[0], *o[1])
            if not dual:   # nothing of a second BatchNorm is written
                assert o[1][0].untouched()
                assert np.array_equal(o[1][1].np(), b["dg0"]) and np.array_equal(o[1][2].np(), b["db0"])
            for i, (inp, (ref, ev)) in enumerate(zip((a, b), refs)):
                fam, case = f"bwd_partials/{_tname(dtype)}", f"rows{rows} {kind} bn{i + 1} acc{acc}"
                _check_bwd(fam, case, inp, ref, ev, acc, dtype, *o[i])
                got = coef.np()[3 * C * i:3 * C * (i + 1)].reshape(3, C)
                for j, name in enumerate(("coef_scale", "coef_mean_dz", "coef_mean_dz_xhat")):
                    check_sum(fam, case, name, got[j], ref["coef"][j], ref["terms_coef"][j], _ceil(dtype))
