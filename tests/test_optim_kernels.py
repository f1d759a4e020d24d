"""The optimiser kernels of csrc/optim.hip, called directly through the C ABI and
compared with a numpy restatement of the formulas documented in include/pose6d.h:
  * sumsq_kernel        (pose6d_sumsq_partial, pose6d_sumsq_partial_step)
  * adamw_kernel        (pose6d_adamw_step)
  * adamw_packed_kernel (pose6d_adamw_step_packed + pose6d_adamw_packed_jobs), bf16 / fp32

Yardstick.  adamw_reference(..., np.float64) is the reference; the same function with
np.float32 evaluates the kernel's operations in the kernel's order in fp32.  Errors are
measured per tensor against the fp64 reference,
    E_p = max|x - ref| / max|ref - p0|   (relative to the update, not to the weight)
    E_m = max|x - ref| / max|ref|        (and the same for E_v),   E = max(E_p, E_m, E_v)
and a kernel must satisfy E(kernel) <= 4 * E(fp32 evaluation), the latter computed in
the test for the same inputs: both round the same operations, the factor absorbs a
differently rounded pow / divide / square root and the norm's summation order.
test_every_mutant_is_separated shows (on the CPU) that this bound tells a correct
kernel from one with a dropped weight decay, an L2 decay, eps under the root, a missing
bias correction, swapped betas or a wrong clip, in at least one of HP_SETS.

Measured (n = 20 003, 4 steps): E(fp32 evaluation) per set and E(kernel) on an MI355X
(adamw_kernel reproduces the fp32 evaluation to the printed digits):
    set              E(fp32 eval)   E(kernel)   E(kernel) / E(fp32 eval)
    default          1.252e-03      1.252e-03   1.00
    big_lr_wd_clip   6.712e-05      6.712e-05   1.00
    clip_inactive    6.356e-05      6.356e-05   1.00
    t1000            2.078e-07      2.078e-07   1.00
The largest E(kernel) is 1.252e-03 (default point: the update is 1e-4 of the weight).
Every mutant lands above 700 x the bound in its best set (no_decay: 0.08 x at the default
point, 701 x at big_lr_wd_clip).  The sum of squares stays below 1e-6 relative (n = 300 001
in one block, bound 7e-5).  Slowest GPU case: the bf16 synthetic packed table, 0.5 s; the
64 Mi + 4099 element grid-cap case takes under 10 ms.
"""
import ctypes
import math
import time

import numpy as np
import pytest
import torch

# hp = {lr, beta1, beta2, eps, weight_decay, step counter before the first step,
#       grad scale (0 reads as 1), max_norm (<= 0: no clipping)}
HP_SETS = {
    "default": (1e-4, 0.9, 0.999, 1e-8, 1e-4, 0, 1.0, 1.0),          # the trainers' point: clip active
    "big_lr_wd_clip": (3e-3, 0.8, 0.95, 1e-6, 5e-2, 0, 0.5, 1.0),    # decay visible, scaled grad, clip active
    "clip_inactive": (3e-3, 0.8, 0.95, 1e-6, 5e-2, 0, 0.125, 1e4),   # norm << max_norm: coefficient exactly 1
    "t1000": (1e-2, 0.9, 0.999, 1e-3, 1e-2, 1000, 0, 0.0),           # large t, hp[6] = 0, no clipping
}
MUTANTS = ("no_decay", "l2_decay", "eps_in_sqrt", "no_bc1", "no_bc2", "betas_swapped", "clip_unscaled",
           "clip_no_min")
N_MAIN = 20003
STEPS = 4
NPART = 1024      # the trainers' partial count
GUARD = 4096      # sentinel floats on each side of a guarded buffer
SENTINEL = 12345.0


def adamw_reference(p0, m0, v0, grads, hp, dtype, mutant=None):
    """clip_grad_norm_ + AdamW over len(grads) steps, every operation in `dtype`
    (np.float64: the reference; np.float32: the kernel's operations in its order).
    Returns (p, m, v, [the gradient norm of each step]).  The hyper-parameters are the
    fp32 values the kernel reads, the norm's sum of squares and the bias corrections
    1 - beta^t are taken in double (as the kernel does) and then rounded to `dtype`."""
    T = np.dtype(dtype).type
    lr, b1, b2, eps, wd, t0, gs, max_norm = (T(np.float32(x)) for x in hp)
    one = T(1)
    if gs == 0:
        gs = one
    if mutant == "betas_swapped":
        b1, b2 = b2, b1
    p, m, v = (np.array(x, dtype=T) for x in (p0, m0, v0))
    norms = []
    for k, g in enumerate(grads):
        t = float(t0) + k + 1
        bc1 = T(1.0 - float(b1) ** t)
        bc2 = T(1.0 - float(b2) ** t)
        root = T(math.sqrt(float(np.sum(np.asarray(g, np.float64) ** 2))))
        norm = gs * root
        norms.append(float(norm))
        c = one
        if max_norm > 0:
            c = max_norm / ((root if mutant == "clip_unscaled" else norm) + T(1e-6))
            if mutant != "clip_no_min" and c > one:
                c = one
        coef = c * gs
        step_size = lr if mutant == "no_bc1" else lr / bc1
        bc2s = one if mutant == "no_bc2" else np.sqrt(bc2)
        decay = one if mutant in ("no_decay", "l2_decay") else one - lr * wd
        gi = np.asarray(g, T) * coef
        if mutant == "l2_decay":
            gi = gi + wd * p
        p = p * decay
        m = m + (one - b1) * (gi - m)
        v = v * b2 + ((one - b2) * gi) * gi
        if mutant == "eps_in_sqrt":
            denom = np.sqrt(v / (bc2s * bc2s) + eps)
        else:
            denom = np.sqrt(v) / bc2s + eps
        p = p - step_size * (m / denom)
        assert p.dtype == m.dtype == v.dtype == np.dtype(T)
    return p, m, v, norms


def error(got, ref, p0):
    """E of the module docstring: got / ref are (p, m, v, ...) triples, ref in fp64."""
    p0 = np.asarray(p0, np.float64)
    d = [np.abs(np.asarray(got[i], np.float64) - ref[i]).max() for i in range(3)]
    return max(d[0] / np.abs(ref[0] - p0).max(), d[1] / np.abs(ref[1]).max(), d[2] / np.abs(ref[2]).max())


_INPUTS = {}


def inputs(name):
    """(p0, m0, v0, grads) of a hyper-parameter set: unit-scale parameters, gradients
    spread over four decades of magnitude, moments zero but for the mid-training set."""
    if name not in _INPUTS:
        rng = np.random.default_rng(sorted(HP_SETS).index(name) + 1)
        p0 = rng.standard_normal(N_MAIN).astype(np.float32)
        grads = [(rng.standard_normal(N_MAIN) * 10.0 ** rng.uniform(-2, 2, N_MAIN)).astype(np.float32)
                 for _ in range(STEPS)]
        if name == "t1000":
            m0 = (0.3 * rng.standard_normal(N_MAIN)).astype(np.float32)
            v0 = ((0.3 * rng.standard_normal(N_MAIN)) ** 2).astype(np.float32)
        else:
            m0 = np.zeros(N_MAIN, np.float32)
            v0 = np.zeros(N_MAIN, np.float32)
        for a in (p0, m0, v0, *grads):
            a.setflags(write=False)
        _INPUTS[name] = (p0, m0, v0, grads)
    return _INPUTS[name]


_REFS = {}


def references(name):
    """(fp64 reference, E of the fp32 evaluation) of a set, computed once."""
    if name not in _REFS:
        p0, m0, v0, grads = inputs(name)
        ref = adamw_reference(p0, m0, v0, grads, HP_SETS[name], np.float64)
        e32 = error(adamw_reference(p0, m0, v0, grads, HP_SETS[name], np.float32), ref, p0)
        _REFS[name] = (ref, e32)
    return _REFS[name]


# ------------------------------------------------------------------ A: CPU only
@pytest.mark.parametrize("name", list(HP_SETS))
def test_reference_matches_torch_adamw(name):
    """The fp64 reference is clip_grad_norm_ + torch.optim.AdamW in double (the calls the
    kernels replace), with the gradient scaled first."""
    p0, m0, v0, grads = inputs(name)
    lr, b1, b2, eps, wd, t0, gs, max_norm = (float(np.float32(x)) for x in HP_SETS[name])
    p = torch.nn.Parameter(torch.from_numpy(p0.astype(np.float64)))
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    opt.state[p] = {"step": torch.tensor(float(t0)), "exp_avg": torch.from_numpy(m0.astype(np.float64)),
                    "exp_avg_sq": torch.from_numpy(v0.astype(np.float64))}
    for g in grads:
        p.grad = torch.from_numpy(g.astype(np.float64)) * (gs if gs != 0 else 1.0)
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([p], max_norm)
        opt.step()
    ref, e32 = references(name)
    st = opt.state[p]
    e = error((p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()), ref, p0)
    assert e <= 1e-6 * e32, (e, e32)


def test_fp32_evaluation_is_close():
    """The yardstick itself is small.  Worst case: three roundings of a weight of magnitude
    <= 5 per step, 4 steps, over the default point's update of 4e-4: 12 * 5 * 2^-24 / 4e-4
    < 1e-2 of the update."""
    for name in HP_SETS:
        e32 = references(name)[1]
        print(f"E(fp32 evaluation) {name}: {e32:.3e}")
        assert 0 < e32 < 1e-2, (name, e32)


def test_every_mutant_is_separated():
    """Every mutant of the reference exceeds 10 x the bound 4 * E(fp32 evaluation) in at
    least one hyper-parameter set; weight decay dropped does NOT at the default point."""
    ratio = {}
    for name in HP_SETS:
        p0, m0, v0, grads = inputs(name)
        ref, e32 = references(name)
        for mut in MUTANTS:
            e = error(adamw_reference(p0, m0, v0, grads, HP_SETS[name], np.float64, mutant=mut), ref, p0)
            ratio[mut, name] = e / (4 * e32)
    for mut in MUTANTS:
        best = max(HP_SETS, key=lambda s: ratio[mut, s])
        print(f"{mut:14s} " + "  ".join(f"{s} {ratio[mut, s]:9.3g}" for s in HP_SETS))
        assert ratio[mut, best] > 10, (mut, best, ratio[mut, best])
    assert ratio["no_decay", "default"] < 1    # why the default point alone is not enough


# ------------------------------------------------------------------ E: argument check
def test_sumsq_rejects_misaligned_grad_before_launch():
    """grad is read as float4: a pointer that is not 16-byte aligned is refused before
    any launch (nothing here is dereferenced); n = 0 reads nothing, so it passes the check."""
    from pose6d import _lib
    lib = _lib.load()
    bad, ok = ctypes.c_void_p(0x1004), ctypes.c_void_p(0x1000)
    assert lib.pose6d_sumsq_partial(bad, 8, ok, 4, None) == 1
    assert b"16-byte aligned" in lib.pose6d_last_error()
    assert lib.pose6d_sumsq_partial_step(bad, 8, ok, 4, None, None, None) == 1
    assert b"16-byte aligned" in lib.pose6d_last_error()
    # n = 0 with an aligned pointer is a valid call: its launch zeroes the partials, so they
    # are real memory where a device exists; without one the launch itself is what fails
    have_gpu = torch.cuda.is_available()
    part = torch.full((4,), 7.0, device="cuda") if have_gpu else None
    pp = ctypes.c_void_p(part.data_ptr()) if have_gpu else ok
    for rc in (lib.pose6d_sumsq_partial(ok, 0, pp, 4, None),
               lib.pose6d_sumsq_partial_step(ok, 0, pp, 4, None, None, None)):
        if have_gpu:
            assert rc == 0, lib.pose6d_last_error()
        else:
            assert rc in (0, 2) and (rc == 0 or b"device" in lib.pose6d_last_error()), lib.pose6d_last_error()
    if have_gpu:
        torch.cuda.synchronize()
        assert bool((part == 0).all())


# ------------------------------------------------------------------ GPU helpers
def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the shared inputs are read-only)


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _guarded(n, dtype=torch.float32, guard=GUARD, fill=SENTINEL):
    """(whole, view): n elements in the middle of a larger allocation (the view starts
    16-byte aligned), sentinel bands of `guard` elements on both sides."""
    whole = torch.full((n + 2 * guard,), fill, device="cuda", dtype=dtype)
    view = whole[guard:guard + n]
    assert view.data_ptr() % 16 == 0
    return whole, view


def _guards_intact(whole, n, guard=GUARD, fill=SENTINEL):
    return bool((whole[:guard] == fill).all()) and bool((whole[guard + n:] == fill).all())


def _sumsq_tol(n, nparts):
    # non-negative terms: relative error <= (roundings on the longest path) * 2^-24; the
    # longest per-thread chain is L = ceil(n / (nparts * 256)), 12 covers the wave and block adds
    return (math.ceil(n / (nparts * 256)) + 12) * 2.0 ** -24


def _gpu_steps(p0, m0, v0, grads, hp, n=None, nparts=NPART, partials=None, guarded=False):
    """len(grads) steps of sumsq_partial_step (advancing hp[5] on the device) + adamw_step
    on the first n elements.  partials: use these instead of the launch's own (the step
    counter is then advanced by hand).  Returns numpy (p, m, v), the norm_out of every
    step, the final hp[5], and whether the guard bands survived."""
    from pose6d._lib import call, stream
    n = len(p0) if n is None else n
    bufs = [_guarded(n) if guarded else (None, torch.empty(n, device="cuda")) for _ in range(4)]
    (_, p), (_, m), (_, v), (_, g) = bufs
    for dst, src in ((p, p0), (m, m0), (v, v0)):
        dst.copy_(_dev(src[:n]))
    hpd = torch.tensor(hp, dtype=torch.float32, device="cuda")
    part = torch.empty(nparts, device="cuda") if partials is None else partials
    norm = torch.full((1,), float("nan"), device="cuda")
    norms = []
    for gk in grads:
        g.copy_(_dev(gk[:n]))
        if partials is None:
            call("sumsq_partial_step", g, n, part, nparts, hpd[5:], None, stream())
        else:
            hpd[5] += 1
        call("adamw_step", p, g, m, v, n, part, nparts, hpd, norm, stream())
        norms.append(norm.item())
    torch.cuda.synchronize()
    ok = all(_guards_intact(w, n) for w, _ in bufs) if guarded else True
    return (p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()), norms, hpd[5].item(), ok


# ------------------------------------------------------------------ B: sum of squares
@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1023, 4099, 300001])
def test_sumsq_partial(n):
    from pose6d._lib import call, stream
    rng = np.random.default_rng(n)
    gh = (rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 2, n)).astype(np.float32)
    ref = float(np.sum(gh.astype(np.float64) ** 2))
    g = _dev(gh)
    step = torch.tensor([5.0], device="cuda")
    seed = torch.tensor([41], device="cuda", dtype=torch.int64)
    launches = 0
    for nparts in (1, 3, 256, 1000, 1024):
        outs = []
        for variant in ("plain", "step", "step_null"):
            whole, part = _guarded(nparts, guard=64)
            if variant == "plain":
                call("sumsq_partial", g, n, part, nparts, stream())
            elif variant == "step":
                call("sumsq_partial_step", g, n, part, nparts, step, seed, stream())
                launches += 1
            else:
                call("sumsq_partial_step", g, n, part, nparts, None, None, stream())
            torch.cuda.synchronize()
            assert _guards_intact(whole, nparts, guard=64)
            outs.append(part)
        part = outs[0]
        assert _same_bits(outs[1], part) and _same_bits(outs[2], part)
        got = float(part.double().sum().item())
        tol = _sumsq_tol(n, nparts)
        print(f"sumsq n {n} nparts {nparts}: rel err {abs(got - ref) / (ref + 1e-300):.2e} tol {tol:.2e}")
        assert abs(got - ref) <= tol * ref, (n, nparts, got, ref)
        # block b reads float4 chunk b * 256 first; the < 4 tail elements go to block 0
        nwork = max(math.ceil((n // 4) / 256), 1 if n % 4 else 0)
        assert bool((_bits(part[nwork:]) == 0).all()), (n, nparts)
        assert step.item() == 5.0 + launches and seed.item() == 41 + launches
    assert launches == 5


# ------------------------------------------------------------------ C: adamw_step
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HP_SETS))
def test_adamw_step_matches_reference(name):
    p0, m0, v0, grads = inputs(name)
    ref, e32 = references(name)
    got, norms, t_end, _ = _gpu_steps(p0, m0, v0, grads, HP_SETS[name])
    assert t_end == HP_SETS[name][5] + STEPS
    ek = error(got, ref, p0)
    print(f"adamw_step {name}: E(kernel) {ek:.3e}  E(fp32 evaluation) {e32:.3e}  ratio {ek / e32:.2f}")
    assert ek <= 4 * e32, (name, ek, e32)
    if HP_SETS[name][7] > 0:   # norm_out is defined only when clipping
        for k in range(STEPS):
            assert abs(norms[k] - ref[3][k]) <= _sumsq_tol(N_MAIN, NPART) * ref[3][k], (k, norms[k], ref[3][k])


def _one_step_hp():
    hp = list(HP_SETS["big_lr_wd_clip"])
    hp[5] = 2.0    # advanced to t = 3 by the step
    return hp


_FULL = {}


def _full_run():
    """One step at n = 20 003 with its own partials; shorter runs must reproduce its
    leading elements when given the same partials."""
    if not _FULL:
        from pose6d._lib import call, stream
        p0, m0, v0, grads = inputs("t1000")   # non-zero moments
        part = torch.empty(NPART, device="cuda")
        call("sumsq_partial", _dev(grads[0]), N_MAIN, part, NPART, stream())
        torch.cuda.synchronize()
        got, _, _, ok = _gpu_steps(p0, m0, v0, grads[:1], _one_step_hp(), partials=part, guarded=True)
        assert ok
        _FULL.update(part=part, got=got)
    return _FULL["part"], _FULL["got"]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4099])
def test_adamw_step_lengths(n):
    """The float4 trips, their clamped loads and the scalar tail: every element equals the
    n = 20 003 run's bit for bit (the update is elementwise once the partials are fixed),
    and nothing outside [0, n) is written."""
    part, full = _full_run()
    p0, m0, v0, grads = inputs("t1000")
    got, _, _, ok = _gpu_steps(p0, m0, v0, grads[:1], _one_step_hp(), n=n, partials=part, guarded=True)
    assert ok, "guard band overwritten"
    for x, y, what in zip(got, full, "pmv"):
        assert np.array_equal(x.view(np.int32), y[:n].view(np.int32)), what
    assert not np.array_equal(got[0], p0[:n])


@pytest.mark.gpu
def test_adamw_step_inactive_clip_is_exactly_no_clip():
    p0, m0, v0, grads = inputs("clip_inactive")
    hp = list(HP_SETS["clip_inactive"])
    a, norms, _, _ = _gpu_steps(p0, m0, v0, grads[:2], hp)
    assert max(norms) < 0.5 * hp[7]
    hp[7] = 0.0
    b, _, _, _ = _gpu_steps(p0, m0, v0, grads[:2], hp)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))


@pytest.mark.gpu
def test_adamw_step_zero_grad_scale_reads_as_one():
    p0, m0, v0, grads = inputs("default")
    hp = list(HP_SETS["big_lr_wd_clip"])
    out = []
    for gs in (0.0, 1.0):
        hp[6] = gs
        out.append(_gpu_steps(p0, m0, v0, grads[:2], hp))
    assert out[0][1] == out[1][1]   # norm_out
    for x, y in zip(out[0][0], out[1][0]):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))


@pytest.mark.gpu
def test_adamw_step_grid_cap_second_trip():
    """n = 16384 * 4096 + 4099: the grid is capped at 16384 blocks, so the first 1024
    float4 positions take a second loop trip, and the tail is 3 scalars.  Constant inputs:
    every element must equal the first, and the first the bits of an n = 4 run on the same
    constants and partials.  AdamW is not idempotent, so an element skipped or updated
    twice shows.  (Under 10 ms on an MI355X, allocation and checks included.)"""
    from pose6d._lib import call, stream
    t0 = time.perf_counter()
    n = 16384 * 4096 + 4099
    consts = (0.75, -0.03125, 0.01, 1e-4)   # p, g, m, v
    part = torch.zeros(NPART, device="cuda")
    part[3] = 9.0      # norm 3 * grad scale 0.5: clip coefficient 2/3
    hp = torch.tensor(_one_step_hp(), device="cuda")
    hp[5] = 3.0
    small = [torch.full((4,), c, device="cuda") for c in consts]
    call("adamw_step", small[0], small[1], small[2], small[3], 4, part, NPART, hp, None, stream())
    big = [torch.full((n,), c, device="cuda") for c in consts]
    call("adamw_step", big[0], big[1], big[2], big[3], n, part, NPART, hp, None, stream())
    torch.cuda.synchronize()
    for i in (0, 2, 3):
        assert small[i][0].item() != consts[i]
        assert bool((big[i] == big[i][0]).all()), i
        assert _same_bits(big[i][:4], small[i])
    assert bool((big[1] == consts[1]).all())
    del big
    print(f"grid-cap case: {(time.perf_counter() - t0) * 1e3:.1f} ms")


# ------------------------------------------------------------------ D: adamw_step_packed
# name, O, I, k, Ip, stride, pad, wt   -- the branches of adamw_packed_kernel each selects:
PACKED_CONVS = [
    # 1x1 float4 update, 4-entry wp stores straight from registers, 8-filter wt stores
    ("c1_64", 64, 64, 1, 64, 1, 0, True),
    # 1x1: second channel group is partial (32 of 64), second filter block is 8 rows
    ("c1_96", 72, 96, 1, 96, 1, 0, True),
    # 1x1 scalar update (R % 4 != 0), per-element wp stores, K padding 30 -> 32
    ("c1_30", 64, 30, 1, 30, 1, 0, True),
    # 1x1 without wt: returns before the barrier; partial filter block (40 rows)
    ("c1_nowt", 40, 64, 1, 64, 1, 0, False),
    # 3x3 float4 update, LDS-staged taps, last group of 4 channels (per-element wp runs), 48 filter
    # rows; bf16: Ip = 20 puts odd taps' runs off 16-byte alignment, so store8 and per-element both run
    ("c3_48_20", 48, 20, 3, 20, 1, 1, True),
    # 3x3: O % 8 != 0 -> per-element wt stores; last filter block of 36 rows; store8 wp runs
    ("c3_100_72", 100, 72, 3, 72, 1, 1, True),
    # row-tap stem: KWp = 8, Ip = 4 > I (channel padding), 2-channel groups + a last group of 1, no wt
    ("stem", 64, 3, 7, 4, 2, 3, False),
    # 5x5: cw = 5 (W = 125: scalar update), last group of 2 channels
    ("c5_64_32", 64, 32, 5, 32, 1, 2, True),
    # 5x5: last group of 4 channels has W = 100: float4 update after scalar groups; 8 filter rows
    ("c5_8_24", 8, 24, 5, 24, 1, 2, True),
    # 11x11: cw = 1 (121 taps); odd master length (a plain range of 1 follows); O % 8 != 0
    ("c11_a", 15, 5, 11, 5, 1, 5, True),
    # 11x11 with channel padding Ip = 8 > I outside the row-tap layout, no wt; odd master length
    ("c11_b", 11, 3, 11, 8, 1, 5, False),
]
# the flat buffer: plain ranges (ints) and conv masters (names) in address order
PACKED_LAYOUT = [4096, "c1_64", 9000, "c1_96", "c1_30", "c1_nowt", "c3_48_20", "c11_a", 1, "c3_100_72", "c11_b", 3,
                 "stem", "c5_64_32", "c5_8_24", 37]
WGUARD = 256      # sentinel elements around every wp / wt
PAD_MARK = 3.0    # written into wp's padding after the initial pack: "padding is never written"


def _layout(w, I, Ip, k, kwp, Kpad, dtype):
    """(wp, its non-padding mask, wt) of an OIHW fp32 master, laid out by torch."""
    O = w.shape[0]
    ref = torch.zeros(O, k, kwp, Ip, device=w.device)
    mask = torch.zeros(O, k, kwp, Ip, device=w.device, dtype=torch.bool)
    ref[:, :, kwp - k:, :I] = w.permute(0, 2, 3, 1)
    mask[:, :, kwp - k:, :I] = True
    full = torch.zeros(O, Kpad, device=w.device)
    fmask = torch.zeros(O, Kpad, device=w.device, dtype=torch.bool)
    full[:, :k * kwp * Ip] = ref.reshape(O, -1)
    fmask[:, :k * kwp * Ip] = mask.reshape(O, -1)
    return full.to(dtype), fmask, w.permute(1, 2, 3, 0).contiguous().to(dtype)


def _pack_table(convs, dtype, masters):
    """Guarded wp / wt buffers and the (host) descriptor table for `convs` over `masters`
    (name -> fp32 view).  Returned per conv: dict(wp, wt, wp_whole, wt_whole, kwp, Kpad)."""
    from pose6d.trunk import _DESC, pack_geom
    rec = np.zeros(len(convs), dtype=_DESC)
    bufs = {}
    for i, (name, O, I, k, Ip, stride, pad, with_t) in enumerate(convs):
        kwp, Kpad = pack_geom(dtype, Ip, k, stride, pad)
        wp_whole, wp = _guarded(O * Kpad, dtype, WGUARD)
        wt_whole, wt = _guarded(I * k * k * O, dtype, WGUARD) if with_t else (None, None)
        assert not with_t or Ip == I
        rec[i] = (masters[name].data_ptr(), wp.data_ptr(), wt.data_ptr() if with_t else 0, O, I, Ip, k, k, Kpad,
                  kwp, 0, 0)
        bufs[name] = dict(wp=wp.view(O, Kpad), wt=wt.view(I, k, k, O) if with_t else None, wp_whole=wp_whole,
                          wt_whole=wt_whole, kwp=kwp, Kpad=Kpad)
    return rec, bufs


def _pack(rec, dtype):
    from pose6d._lib import call, stream
    from pose6d.trunk import DTYPES
    d = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    call("pack_conv_weights", DTYPES[dtype], d, len(rec), 0, stream())
    torch.cuda.synchronize()
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_adamw_step_packed_synthetic_table(dtype):
    from pose6d._lib import call, query, stream
    from pose6d.trunk import DTYPES
    convs = {c[0]: c for c in PACKED_CONVS}
    offs, off = {}, 0
    for item in PACKED_LAYOUT:
        if isinstance(item, str):
            _, O, I, k = convs[item][:4]
            assert off % 4 == 0, item
            offs[item] = (off, O * I * k * k)
            off += O * I * k * k
        else:
            off += item
    n = off
    assert len(offs) == len(PACKED_CONVS)
    gen = torch.Generator(device="cuda").manual_seed(5)
    pw, p = _guarded(n)
    mw, m = _guarded(n)
    vw, v = _guarded(n)
    p.copy_(torch.randn(n, device="cuda", generator=gen) * 0.2)
    m.copy_(torch.randn(n, device="cuda", generator=gen) * 1e-4)
    v.copy_(torch.rand(n, device="cuda", generator=gen) * 1e-8)
    grads = [torch.randn(n, device="cuda", generator=gen) * 10.0 ** (4 * torch.rand(n, device="cuda", generator=gen) - 2)
             for _ in range(3)]
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    p_init = p.clone()
    order = np.random.default_rng(0).permutation(len(PACKED_CONVS))   # the job builder sorts by address
    clist = [PACKED_CONVS[i] for i in order]
    masters = {name: p[o:o + ln] for name, (o, ln) in offs.items()}
    rec, bufs = _pack_table(clist, dtype, masters)

    def expected(name, src):
        _, O, I, k, Ip = convs[name][:5]
        o, ln = offs[name]
        return _layout(src[o:o + ln].view(O, I, k, k), I, Ip, k, bufs[name]["kwp"], bufs[name]["Kpad"], dtype)

    # the initial pack (the contract) overwrites the whole of wp, padding included, with zeros there
    for b in bufs.values():
        b["wp"].fill_(PAD_MARK)
    descs = _pack(rec, dtype)
    n_pad = 0
    for name, b in bufs.items():
        wp, mask, wt = expected(name, p)
        assert _same_bits(b["wp"], wp), f"initial pack: {name} wp"
        assert b["wt"] is None or _same_bits(b["wt"], wt), f"initial pack: {name} wt"
        # mark the padding: the packed AdamW must leave it alone (a zero written there would not show)
        b["wp"][~mask] = PAD_MARK
        n_pad += int((~mask).sum())
    assert n_pad > 0

    args = (rec.ctypes.data, len(rec), p.data_ptr(), n)
    n_jobs = query("adamw_packed_jobs", *args, None, 0)
    assert n_jobs > 0
    jobs_h = np.zeros((n_jobs, 4), dtype=np.int32)
    assert query("adamw_packed_jobs", *args, jobs_h.ctypes.data, n_jobs) == n_jobs
    jobs = torch.from_numpy(jobs_h).cuda()

    hp_h = list(HP_SETS["big_lr_wd_clip"])
    hp, hp2 = (torch.tensor(hp_h, device="cuda") for _ in range(2))
    part, part2 = torch.empty(NPART, device="cuda"), torch.empty(NPART, device="cuda")
    norm, norm2 = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    for g in grads:
        call("sumsq_partial_step", g, n, part, NPART, hp[5:], None, stream())
        call("adamw_step_packed", p, g, m, v, part, NPART, hp, norm, DTYPES[dtype], descs, jobs, n_jobs, stream())
        call("sumsq_partial_step", g, n, part2, NPART, hp2[5:], None, stream())
        call("adamw_step", p2, g, m2, v2, n, part2, NPART, hp2, norm2, stream())
    torch.cuda.synchronize()
    assert hp[5].item() == 3 and hp2[5].item() == 3

    # the same update, bit for bit, and nothing written outside the buffers
    assert _same_bits(p, p2), "masters differ"
    assert _same_bits(m, m2) and _same_bits(v, v2), "moments differ"
    assert _same_bits(norm, norm2)
    assert all(_guards_intact(w, n) for w in (pw, mw, vw)), "guard band of a flat buffer overwritten"
    assert not torch.equal(p, p_init)

    # the packed copies: torch's layout of the updated masters, the padding still marked
    for name, b in bufs.items():
        wp, mask, wt = expected(name, p2)
        assert _same_bits(b["wp"], torch.where(mask, wp, torch.full_like(wp, PAD_MARK))), f"{name}: wp"
        assert _guards_intact(b["wp_whole"], b["wp"].numel(), WGUARD), f"{name}: wp guard"
        if b["wt"] is not None:
            assert _same_bits(b["wt"], wt), f"{name}: wt"
            assert _guards_intact(b["wt_whole"], b["wt"].numel(), WGUARD), f"{name}: wt guard"

    # and a fresh pose6d_pack_conv_weights of the updated masters (zeros in its padding)
    masters2 = {name: p2[o:o + ln] for name, (o, ln) in offs.items()}
    rec2, fresh = _pack_table(clist, dtype, masters2)
    _pack(rec2, dtype)
    for name, b in bufs.items():
        mask = expected(name, p2)[1]
        f = fresh[name]
        assert _same_bits(torch.where(mask, b["wp"], torch.zeros_like(b["wp"])), f["wp"]), f"{name}: wp vs fresh pack"
        if b["wt"] is not None:
            assert _same_bits(b["wt"], f["wt"]), f"{name}: wt vs fresh pack"
