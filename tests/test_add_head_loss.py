"""pose6d_add_head_loss through the C ABI (no trunk): the ADD / ADD-S term that the whole-step
trainers add to their head + PoseLoss launch.

Reference.  torch-CPU fp64 autograd of add_weight * L, L = oracle.add_loss.forward_torch's
computation (add_loss.py:101-150) on normalize(raw) and the step's translation, with the
normalise written out for both norm_modes and, for trans_mode 2, the pinhole of the predicted
depth.  ADD-S is discontinuous in the nearest index, so a symmetric sample's reference pairs
every point with a FIXED ground-truth index: the one the golden-pinned
ADDLoss.per_sample(..., want_points=True)["argmin"] returns for the same normalize(raw) and
translation (_fixed_loss; test_fixed_loss_restates_forward_torch ties it to forward_torch on
the CPU).  The reference result of an accumulated output is preload + contribution.

Yardstick.  The same computation in torch-CPU fp32 (preload + contribution rounded to fp32),
under the rule of tests/test_bn_kernels.py for summed outputs: per output tensor
    max|kernel - fp64| <= 4 * max|fp32 evaluation - fp64| + 1e-6
(that file's factor, and the absolute floor of its summed outputs; the preloads are N(0, 1)
and add_weight = 2.5, so the outputs are O(1) and the floor is ~8 fp32 steps).  Every case
prints its figures before it asserts.

Exact checks: `nearest` equals pose6d_add_eval's argmin on symmetric samples and arange on the
others, with no neighbour table, the kNN table and a garbage table (all outputs identical
bits); unknown samples (-1, >= n_slots, a slot without points) get per = 0 and untouched
gradient rows; add_weight = 0 changes nothing; a repeated call repeats its bits; a prediction
identical to the ground truth adds exact zeros; a batch without a known object writes only
per = 0.

Measured on an MI355X (largest over each case's mode combinations; kernel = max|kernel - fp64|,
fp32 = max|fp32 evaluation - fp64| of the same case and output, printed as "ADD-E" lines):
    case      output       kernel      fp32
    mixed67   loss         4.004e-08   4.004e-08
    mixed67   grad_raw     1.218e-07   1.218e-07
    mixed67   grad_trans   2.040e-07   2.040e-07
    mixed67   per          1.275e-08   4.926e-09
    sym2049   loss         1.472e-08   1.472e-08
    sym2049   grad_raw     3.949e-08   3.949e-08
    sym2049   grad_trans   3.392e-07   2.200e-07
    sym2049   per          2.003e-09   9.653e-10
    b300n8    loss         8.398e-09   3.820e-08
    b300n8    grad_raw     1.187e-07   1.187e-07
    b300n8    grad_trans   1.135e-07   1.135e-07
    b300n8    per          1.896e-08   1.921e-08
Where the two columns agree to every digit, both errors are the one fp32 rounding of the
accumulated result (preload + contribution) at the same element.  The largest kernel / fp32
ratio of any single case is 2.6 (mixed67 norm 1 trans 2, per: 1.275e-08 against 4.926e-09).
"""
import tempfile

import numpy as np
import pytest
import torch

from tests.synth import LINEMOD_OBJ_IDS, make_poses, write_mesh_dir

SYM = (9, 10)
ADD_WEIGHT = 2.5
FACTOR, FLOOR = 4.0, 1e-6


# ------------------------------------------------------------------ reference (CPU)
def _q2m(q):
    """add_loss.py:203-215 (oracle.add_loss.forward_torch's q2m)."""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    x2, y2, z2 = x * x, y * y, z * z
    xy, xz, yz = x * y, x * z, y * z
    wx, wy, wz = w * x, w * y, w * z
    r0 = torch.stack([1 - 2 * y2 - 2 * z2, 2 * xy - 2 * wz, 2 * xz + 2 * wy], dim=1)
    r1 = torch.stack([2 * xy + 2 * wz, 1 - 2 * x2 - 2 * z2, 2 * yz - 2 * wx], dim=1)
    r2 = torch.stack([2 * xz - 2 * wy, 2 * yz + 2 * wx, 1 - 2 * x2 - 2 * y2], dim=1)
    return torch.stack([r0, r1, r2], dim=1)


def _fixed_loss(points, pred_r, pred_t, gt_r, gt_t, obj_ids, index):
    """forward_torch with the ADD-S minimum replaced by the pairing index[b] (None: k with k);
    returns (loss, per-sample values with 0 for unknown samples)."""
    pR, gR = _q2m(pred_r), _q2m(gt_r)
    per = []
    for i in range(pred_r.shape[0]):
        oid = int(obj_ids[i])
        if oid not in points or points[oid].shape[0] == 0:
            per.append(None)
            continue
        P = points[oid].to(pred_r.dtype)
        Ps = P if index[i] is None else P[torch.as_tensor(index[i], dtype=torch.long)]
        G = Ps @ gR[i].T + gt_t[i]
        Q = P @ pR[i].T + pred_t[i]
        per.append(torch.norm(Q - G, dim=1).mean())
    known = [p for p in per if p is not None]
    total = torch.zeros((), dtype=pred_r.dtype)
    for p in known:
        total = total + p
    loss = total / len(known) if known else total
    return loss, [0.0 if p is None else float(p.detach()) for p in per]


def _normalize(raw, norm_mode):
    n = raw.norm(dim=1, keepdim=True)
    return raw / n.clamp_min(1e-12) if norm_mode == 0 else raw / (n + 1e-8)


def _pinhole_z(z, bbox, K):
    """pose_net_rgb_geometric.py:93-109; K (B, 3, 3) or (3, 3)."""
    Kb = K if K.dim() == 3 else K.unsqueeze(0).expand(z.shape[0], 3, 3)
    x = (bbox[:, 0] - Kb[:, 0, 2]) * z / Kb[:, 0, 0]
    y = (bbox[:, 1] - Kb[:, 1, 2]) * z / Kb[:, 1, 1]
    return torch.stack([x, y, z], dim=1)


def _evaluate(case, index, dtype):
    """preload + add_weight * L and its gradients in `dtype` on the CPU: loss, grad_raw,
    grad_trans ((B, 3), (B,) for trans_mode 2, the preload for trans_mode 1), per."""
    c = case
    f = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    raw = f(c["raw"]).requires_grad_(True)
    if c["trans_mode"] == 2:
        leaf = f(c["trans"][:, 2]).requires_grad_(True)
        t = _pinhole_z(leaf, f(c["bbox"]), f(c["K"]))
    else:
        leaf = f(c["trans"]).requires_grad_(True)
        t = leaf
    pts = {o: torch.from_numpy(p) for o, p in c["points"].items()}
    L, per = _fixed_loss(pts, _normalize(raw, c["norm_mode"]), t, f(c["gt_rot"]), f(c["gt_trans"]), c["ids"], index)
    loss = f(c["add_weight"]) * L
    if loss.requires_grad:
        loss.backward()
    zero = lambda x: torch.zeros_like(x) if x.grad is None else x.grad
    out = {"loss": f(c["pre_loss"]) + loss.detach(), "grad_raw": f(c["pre_raw"]) + zero(raw), "per": per}
    out["grad_trans"] = f(c["pre_trans"]) if c["trans_mode"] == 1 else f(c["pre_trans"]) + zero(leaf)
    return {k: (np.asarray(v, np.float64) if k == "per" else v.double().numpy()) for k, v in out.items()}


def test_fixed_loss_restates_forward_torch():
    """_fixed_loss is oracle.add_loss.forward_torch with the minimum's index made explicit:
    equal values with the index of the fp64 minimum, and for asymmetric objects as it is."""
    from oracle import add_loss as OA
    rng = np.random.default_rng(0)
    pts = {o: torch.from_numpy((rng.standard_normal((37, 3)) * 0.04).astype(np.float32)) for o in (0, 9, 10)}
    ids = np.array([0, 9, 10, -1, 99, 9], np.int64)
    pr, pt, gr, gt = (torch.from_numpy(a).double() for a in make_poses(rng, len(ids), sigma_q=0.3, sigma_t=0.02))
    index = []
    for b, o in enumerate(ids):
        if int(o) not in SYM:
            index.append(None)
            continue
        P = pts[int(o)].double()
        Q, G = P @ _q2m(pr)[b].T + pt[b], P @ _q2m(gr)[b].T + gt[b]
        index.append(torch.norm(Q[:, None] - G[None], dim=2).argmin(dim=1).numpy())
    want = OA.forward_torch(pts, pr, pt, gr, gt, ids).item()
    got, per = _fixed_loss(pts, pr, pt, gr, gt, ids, index)
    assert abs(got.item() - want) <= 1e-15
    assert per[3] == 0.0 and per[4] == 0.0 and min(per[:3]) > 0


# ------------------------------------------------------------------ cases
def _crit_from(points):
    from models.add_loss import ADDLoss
    crit = ADDLoss.__new__(ADDLoss)
    torch.nn.Module.__init__(crit)
    crit.points = {k: torch.from_numpy(v).cuda() for k, v in points.items()}
    crit.diameters, crit.device, crit._table = {k: 0.1 for k in points}, "cuda", None
    return crit


def _case(name, seed, ids, points, norm_mode=0, trans_mode=0, K_batched=True, add_weight=ADD_WEIGHT):
    """Seeded inputs: unit gt quaternions, raw = a perturbed gt scaled by 0.5 .. 3 (the
    normalise matters), N(0, 1) preloads.  trans_mode 2: trans is the fp32 pinhole of a
    predicted depth, as the trainer's head + loss launch leaves it."""
    rng = np.random.default_rng(seed)
    B = len(ids)
    pr, pt, gr, gt = make_poses(rng, B, sigma_q=0.2, sigma_t=0.01)
    raw = (pr * rng.uniform(0.5, 3.0, (B, 1))).astype(np.float32)
    c = {"name": name, "ids": np.asarray(ids, np.int64), "points": points, "norm_mode": norm_mode,
         "trans_mode": trans_mode, "add_weight": np.float32(add_weight), "raw": raw, "gt_rot": gr, "gt_trans": gt,
         "bbox": None, "K": None}
    if trans_mode == 2:
        bbox = rng.uniform(20, 200, (B, 2)).astype(np.float32)
        K = np.zeros((B, 3, 3), np.float32)
        K[:, 0, 0], K[:, 1, 1] = rng.uniform(400, 800, B), rng.uniform(400, 800, B)
        K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = rng.uniform(80, 144, B), rng.uniform(80, 144, B), 1.0
        if not K_batched:
            K = K[0].copy()
        z = pt[:, 2].copy()
        pt = _pinhole_z(torch.from_numpy(z), torch.from_numpy(bbox), torch.from_numpy(K)).numpy()
        c["bbox"], c["K"] = bbox, K
    c["trans"] = np.ascontiguousarray(pt, np.float32)
    c["pre_loss"] = np.float32(rng.standard_normal())
    c["pre_raw"] = rng.standard_normal((B, 4)).astype(np.float32)
    c["pre_trans"] = rng.standard_normal((B,) if trans_mode == 2 else (B, 3)).astype(np.float32)
    return c


def _mesh(rng, n):
    return (rng.standard_normal((n, 3)) * 0.04).astype(np.float32)


def _points67():
    rng = np.random.default_rng(67)
    return {o: _mesh(rng, 67) for o in (0, 9, 10)}          # slots 1..8 hold no points, n_slots = 11


def _run(case, crit, nbr="table", add_weight=None, zero_preload=False):
    """One pose6d_add_head_loss call on the case; nbr: "table" (the mesh table's own kNN
    table), None, or a (tensor, K) pair.  Returns the outputs as numpy arrays."""
    from pose6d._lib import call, stream
    c = case
    T = crit._mesh_table(torch.device("cuda"))
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    B = len(c["ids"])
    pre = (lambda a: np.zeros_like(a)) if zero_preload else (lambda a: a)
    loss = dev(np.asarray(pre(c["pre_loss"])).reshape(1))
    graw, gtr = dev(pre(c["pre_raw"])), dev(pre(c["pre_trans"]))
    per = torch.full((B,), 7.0, device="cuda", dtype=torch.float64)
    mx = max(T.max_npts, 1)
    nearest = torch.full((B, mx), -7, device="cuda", dtype=torch.int32)
    tab, K = (T.nbr, T.K) if nbr == "table" else ((None, 0) if nbr is None else nbr)
    Kc = dev(c["K"])
    call("add_head_loss", dev(c["raw"]), c["norm_mode"], dev(c["trans"]), dev(c["gt_rot"]), dev(c["gt_trans"]),
         dev(c["ids"]), B, T.points, T.off, T.npts, T.sym, T.n_slots, T.max_npts, tab, K,
         float(c["add_weight"] if add_weight is None else add_weight), c["trans_mode"], dev(c["bbox"]), Kc,
         0 if Kc is None else int(Kc.dim() == 3), loss, graw, gtr, per, nearest, stream())
    torch.cuda.synchronize()
    return {"loss": loss.cpu().numpy()[0], "grad_raw": graw.cpu().numpy(), "grad_trans": gtr.cpu().numpy(),
            "per": per.cpu().numpy(), "nearest": nearest.cpu().numpy()}


def _eval_argmin(case, crit):
    """The golden-pinned search's index (pose6d_add_eval) for the kernel's own normalize(raw)
    (pose6d_rownorm_fwd: the same bits) and translation."""
    from pose6d._lib import call, stream
    c = case
    raw = torch.from_numpy(c["raw"]).cuda()
    q = torch.empty_like(raw)
    call("rownorm_fwd", raw, q, raw.shape[0], 4, c["norm_mode"], stream())
    s = crit.per_sample(q, torch.from_numpy(c["trans"]).cuda(), torch.from_numpy(c["gt_rot"]).cuda(),
                        torch.from_numpy(c["gt_trans"]).cuda(), torch.from_numpy(c["ids"]).cuda(), want_points=True)
    return s["argmin"].cpu().numpy(), s["valid"].cpu().numpy()


def _same_bits(a, b, keys=("loss", "grad_raw", "grad_trans", "per", "nearest")):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys)


def _check(case, crit):
    """The exact checks and the yardstick for one case; returns {output: (err, err32)}."""
    c = case
    B = len(c["ids"])
    got = _run(c, crit)
    amin, valid = _eval_argmin(c, crit)
    npts = {o: p.shape[0] for o, p in c["points"].items()}
    index = []
    for b in range(B):
        o = int(c["ids"][b])
        n = npts.get(o, 0)
        if n == 0:
            assert valid[b] == 0 and got["per"][b] == 0.0
            assert (got["nearest"][b] == -7).all(), "an unknown sample's row of `nearest` was written"
            assert got["grad_raw"][b].tobytes() == c["pre_raw"][b].tobytes()
            assert got["grad_trans"][b].tobytes() == c["pre_trans"][b].tobytes()
            index.append(None)
            continue
        want = amin[b, :n] if o in SYM else np.arange(n)
        np.testing.assert_array_equal(got["nearest"][b, :n], want, err_msg=f"{c['name']}: nearest of sample {b}")
        assert (got["nearest"][b, n:] == -7).all()
        index.append(want if o in SYM else None)
    if c["trans_mode"] == 1:
        assert got["grad_trans"].tobytes() == c["pre_trans"].tobytes(), "trans_mode 1 wrote a translation gradient"
    # the index does not depend on the neighbour table, nor does any other bit
    T = crit._mesh_table(torch.device("cuda"))
    junk = np.random.default_rng(1).integers(0, 65536, (T.points.shape[0], 16)).astype(np.uint16).view(np.int16)
    for name, nbr in (("no table", None), ("garbage table", (torch.from_numpy(junk).cuda(), 16))):
        assert _same_bits(got, _run(c, crit, nbr=nbr)), f"{c['name']}: {name} changes the result"
    assert _same_bits(got, _run(c, crit)), f"{c['name']}: a repeated call differs"
    same = _run(c, crit, add_weight=0.0)
    for k, pre in (("loss", c["pre_loss"]), ("grad_raw", c["pre_raw"]), ("grad_trans", c["pre_trans"])):
        assert np.asarray(same[k]).tobytes() == np.asarray(pre).tobytes(), f"{c['name']}: add_weight 0 changed {k}"
    # the yardstick
    r64, r32 = _evaluate(c, index, torch.float64), _evaluate(c, index, torch.float32)
    res = {}
    for k in ("loss", "grad_raw", "grad_trans", "per"):
        err = float(np.abs(np.asarray(got[k], np.float64) - r64[k]).max())
        e32 = float(np.abs(r32[k] - r64[k]).max())
        print(f"ADD-E | {c['name']} | norm {c['norm_mode']} trans {c['trans_mode']} | {k} | E32 {e32:.3e} | Ek {err:.3e}")
        res[k] = (err, e32)
    for k, (err, e32) in res.items():
        assert np.isfinite(np.asarray(got[k], np.float64)).all()
        assert err <= FACTOR * e32 + FLOOR, \
            f"{c['name']} {k}: kernel error {err:.3e} > 4 * fp32 evaluation's {e32:.3e} + 1e-6"
    return res


# ------------------------------------------------------------------ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("norm_mode,trans_mode,K_batched",
                         [(n, t, True) for n in (0, 1) for t in (0, 1, 2)] + [(0, 2, False), (1, 2, False)])
def test_mixed_batch_67_points(norm_mode, trans_mode, K_batched):
    """B = 5, ids [0, 9, 10, -1, 99] on 67-point meshes (not a multiple of a wavefront): an
    asymmetric, two symmetric and two unknown samples, in every mode; the intrinsics (read in
    trans_mode 2 only) per sample and shared."""
    pts = _points67()
    c = _case("mixed67", 100 + 10 * norm_mode + trans_mode, [0, 9, 10, -1, 99], pts, norm_mode, trans_mode, K_batched)
    _check(c, _crit_from(pts))


@pytest.mark.gpu
@pytest.mark.parametrize("modes", [(0, 0), (1, 2)], ids=["n0t0", "n1t2"])
def test_one_symmetric_sample_2049_points(modes):
    """One symmetric sample on a 2049-point mesh: one point past the 2048-point LDS tile."""
    pts = {9: _mesh(np.random.default_rng(2049), 2049)}
    c = _case("sym2049", 200 + modes[0], [9], pts, modes[0], modes[1])
    _check(c, _crit_from(pts))


@pytest.mark.gpu
@pytest.mark.parametrize("modes", [(0, 0), (1, 2)], ids=["n0t0", "n1t2"])
def test_300_samples_8_points(modes):
    """B = 300 on 8-point meshes: more samples than the 256 threads that count them, the
    small-mesh rounding of torch.mm (n < 11), and unknown ids of every kind (-1, >= n_slots,
    slot 3 without points)."""
    rng = np.random.default_rng(8)
    pts = {o: _mesh(rng, 8) for o in (0, 1, 9, 10)}
    pts[3] = np.zeros((0, 3), np.float32)
    ids = np.array([[0, 9, 3, 10, -1, 1, 99][i % 7] for i in range(300)], np.int64)
    c = _case("b300n8", 300 + modes[0], ids, pts, modes[0], modes[1])
    _check(c, _crit_from(pts))


@pytest.mark.gpu
@pytest.mark.parametrize("norm_mode", [0, 1])
def test_prediction_equal_to_ground_truth(norm_mode):
    """gt_rot = the kernel's own normalize(raw), trans = gt_trans: every distance is 0, so the
    loss and every gradient are exact zeros (no 0 / 0)."""
    from pose6d._lib import call, stream
    pts = _points67()
    crit = _crit_from(pts)
    c = _case("identity", 400 + norm_mode, [0, 9, 10, -1, 99], pts, norm_mode, 0)
    raw = torch.from_numpy(c["raw"]).cuda()
    q = torch.empty_like(raw)
    call("rownorm_fwd", raw, q, raw.shape[0], 4, norm_mode, stream())
    c["gt_rot"], c["gt_trans"] = q.cpu().numpy(), c["trans"].copy()
    got = _run(c, crit, zero_preload=True)
    assert got["loss"] == 0.0 and not got["grad_raw"].any() and not got["grad_trans"].any()
    assert not got["per"].any()
    assert (got["nearest"][:3, :67] == np.arange(67)).all()    # every point's nearest is its own, at 0
    pre = _run(c, crit)
    for k, p in (("loss", c["pre_loss"]), ("grad_raw", c["pre_raw"]), ("grad_trans", c["pre_trans"])):
        assert np.asarray(pre[k]).tobytes() == np.asarray(p).tobytes()


@pytest.mark.gpu
def test_batch_without_a_known_object():
    pts = _points67()
    c = _case("unknown", 500, [-1, 99, 5, 11], pts, 0, 0)
    got = _run(c, _crit_from(pts))
    assert not got["per"].any() and (got["nearest"] == -7).all()
    for k, p in (("loss", c["pre_loss"]), ("grad_raw", c["pre_raw"]), ("grad_trans", c["pre_trans"])):
        assert np.asarray(got[k]).tobytes() == np.asarray(p).tobytes(), k


def _golden_crit(g, tag):
    from models.add_loss import ADDLoss
    d = tempfile.mkdtemp()
    write_mesh_dir(d, n_vertices=700, seed=11)
    np.random.seed(1234)
    crit = ADDLoss(d, "cuda")
    if tag != "n500":
        for o in LINEMOD_OBJ_IDS:
            crit.points[o] = torch.from_numpy(g[f"{tag}/points/{o}"]).cuda()
    return crit


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["n500", "n2000", "ties"])
def test_pure_add_against_the_reference_goldens(golden, tag):
    """raw = the golden pred_rot, add_weight 1 onto zeros: the loss is the reference's own
    ADDLoss.forward value (rtol 1e-5, test_add_loss_backward_vs_torch_autograd's bound for the
    same quantity), `ties` -- stored without a forward value -- against the mean of the
    reference's per-sample ADD / ADD-S; the symmetric samples' indices are the reference's."""
    g = golden["add_loss"]
    crit = _golden_crit(g, tag)
    ids = g[f"{tag}/obj_ids"]
    c = {"name": tag, "ids": ids, "norm_mode": 0, "trans_mode": 0, "add_weight": np.float32(1.0),
         "raw": g[f"{tag}/pred_rot"], "trans": g[f"{tag}/pred_trans"], "gt_rot": g[f"{tag}/gt_rot"],
         "gt_trans": g[f"{tag}/gt_trans"], "bbox": None, "K": None, "pre_loss": np.float32(0),
         "pre_raw": np.zeros((len(ids), 4), np.float32), "pre_trans": np.zeros((len(ids), 3), np.float32)}
    got = _run(c, crit)
    vi = np.nonzero(g[f"{tag}/valid"])[0]
    sym = np.isin(ids[vi], g["symmetric_ids"])
    per_ref = np.where(sym, g[f"{tag}/adds"], g[f"{tag}/add"])
    want = g[f"{tag}/forward"] if f"{tag}/forward" in g else per_ref.mean()
    np.testing.assert_allclose(got["loss"], want, rtol=1e-5)
    np.testing.assert_allclose(got["per"][vi], per_ref, rtol=1e-5)
    assert not got["per"][g[f"{tag}/valid"] == 0].any()
    rows = np.cumsum([0] + list(g[f"{tag}/npts"]))
    for i, b in enumerate(vi):
        if sym[i]:
            np.testing.assert_array_equal(got["nearest"][b, :g[f"{tag}/npts"][i]],
                                          g[f"{tag}/argmin"][rows[i]:rows[i + 1]])


@pytest.mark.gpu
def test_refused_arguments():
    from pose6d._lib import Pose6dError, load
    pts = _points67()
    crit = _crit_from(pts)
    base = _case("refused", 600, [0, 9], pts, 1, 2)

    def refused(what, **kw):
        c = dict(base, **{k: v for k, v in kw.items() if k in base})
        with pytest.raises(Pose6dError) as e:
            _run(c, crit, **{k: v for k, v in kw.items() if k not in base})
        assert "pose6d_add_head_loss" in str(e.value) and what in str(e.value), str(e.value)
        assert what in load().pose6d_last_error().decode()

    refused("norm_mode", norm_mode=2)
    refused("trans_mode", trans_mode=3)
    refused("trans_mode 2 needs", bbox=None)
    refused("trans_mode 2 needs", K=None)
    refused("batch", ids=np.zeros(0, np.int64), raw=np.zeros((0, 4), np.float32))
    T = crit._mesh_table(torch.device("cuda"))
    refused("neighbour table", nbr=(T.nbr, 12))
