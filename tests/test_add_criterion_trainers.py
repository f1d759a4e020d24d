"""The ADD / ADD-S criterion inside the four whole-step trainers of pose6d.train
(add_loss=ADDLoss, add_weight): pose6d_add_head_loss right after the head + PoseLoss launch,
object ids in the trainer-owned device buffer tr.obj_ids that a replayed graph reads.
B = 4 at 224^2, Dropout modules in eval, as the trainers' own test files."""
import warnings

import numpy as np
import pytest
import torch

from tests.synth import synthetic_meshes

pytestmark = pytest.mark.gpu

B = 4
DATA_SEED = 2024
ADD_WEIGHT = 0.7
IDS_A = [0, 9, 10, -1]        # asymmetric, two symmetric, unknown
IDS_B = [9, 1, 3, 10]
KINDS = ["rgbd_geometric", "rgb", "rgbd", "rgb_geometric"]


def _model_and_trainer(kind):
    import models.pose_net_rgb as m_rgb
    import models.pose_net_rgb_geometric as m_rgbg
    import models.pose_net_rgbd as m_rgbd
    import models.pose_net_rgbd_geometric as m_rgbdg
    from pose6d import train as T
    return {"rgbd_geometric": (m_rgbdg.PoseNetRGBDGeometric, T.RGBDGeometricTrainer),
            "rgb": (m_rgb.PoseNetRGB, T.RGBTrainer),
            "rgbd": (m_rgbd.PoseNetRGBD, T.RGBDTrainer),
            "rgb_geometric": (m_rgbg.PoseNetRGBGeometric, T.RGBGeometricTrainer)}[kind]


def _data(kind, seed=DATA_SEED):
    from bench import synth_batch
    rgb, depth_raw, bbox, K, gr, gt = synth_batch(B, torch.device("cuda"), seed=seed)
    return {"rgbd_geometric": (rgb, depth_raw, bbox, K, gr, gt), "rgb": (rgb, gr, gt),
            "rgbd": (rgb, depth_raw.unsqueeze(1), gr, gt), "rgb_geometric": (rgb, bbox, K, gr, gt)}[kind]


def _dropouts_eval(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.eval()


def _crit(n_points=200):
    from models.add_loss import ADDLoss
    pts, diam = synthetic_meshes(n_points, seed=0)
    crit = ADDLoss.__new__(ADDLoss)
    torch.nn.Module.__init__(crit)
    crit.points = {k: torch.from_numpy(v).cuda() for k, v in pts.items()}
    crit.diameters, crit.device, crit._table = diam, "cuda", None
    return crit


def _make(kind, dtype, seed=0, **kw):
    model_cls, trainer_cls = _model_and_trainer(kind)
    warnings.simplefilter("ignore")
    torch.manual_seed(seed)
    m = model_cls(pretrained=False)
    P0 = {k: v.clone() for k, v in m.state_dict().items()}
    tr = trainer_cls(m.cuda(), B, dtype=dtype, **kw)            # (puts the model in train mode)
    _dropouts_eval(m)
    return tr, P0


def _ids(v):
    return torch.tensor(v, dtype=torch.int64, device="cuda")


def _bufs(tr):
    return [b for n, b in tr.model.named_buffers() if "running" in n or "num_batches" in n]


def _state(tr):
    return [t.clone() for t in (tr.arena.flat, tr.m, tr.v, tr.hp, tr.loss, tr.arena.grad, *_bufs(tr))]


def _grad_trans(tr, kind):
    return tr.dz if kind == "rgb_geometric" else tr.dtrans


@pytest.mark.parametrize("kind", KINDS)
def test_forward_loss_is_the_two_launches(kind):
    """fp32, PoseLoss(1, 10) + 0.7 ADD: after _forward_loss, loss / draw / dtrans (dz) are
    bit-identical to the existing head + loss entry point followed by pose6d_add_head_loss on
    that raw, called directly."""
    from pose6d._lib import call, stream
    crit = _crit()
    tr, _ = _make(kind, torch.float32, add_loss=crit, add_weight=ADD_WEIGHT)
    data = _data(kind)
    gr, gt = data[-2], data[-1]
    tr.obj_ids.copy_(_ids(IDS_A))
    raw = tr._forward_loss(*data)
    torch.cuda.synchronize()
    got = [t.clone() for t in (tr.loss, tr.draw, _grad_trans(tr, kind))]
    rot, trans = torch.empty(B, 4, device="cuda"), torch.empty(B, 3, device="cuda")
    loss, draw = torch.full((), 7.0, device="cuda"), torch.full((B, 4), 7.0, device="cuda")
    st = stream()
    T = crit._mesh_table(torch.device("cuda"))
    per = torch.empty(B, device="cuda", dtype=torch.float64)

    def add(norm_mode, trans_mode, trans_in, gtr, bbox=None, K=None):
        call("add_head_loss", raw, norm_mode, trans_in, gr, gt, tr.obj_ids, B, T.points, T.off, T.npts, T.sym,
             T.n_slots, T.max_npts, T.nbr, T.K, ADD_WEIGHT, trans_mode, bbox, K, 0 if K is None else int(K.dim() == 3),
             loss, draw, gtr, per, None, st)

    if kind == "rgbd_geometric":
        _, depth_raw, bbox, K, _, _ = data
        gtr = torch.full((B, 3), 7.0, device="cuda")
        call("geo_head_loss", raw, depth_raw, depth_raw.shape[1], depth_raw.shape[2], bbox, K, 1, gr, gt, B, 1.0, 10.0,
             0, rot, trans, loss, draw, gtr, st)
        add(0, 1, trans, None)
    elif kind in ("rgb", "rgbd"):
        gtr = torch.full((B, 3), 7.0, device="cuda")
        call("quat_head_loss", raw, tr.trans, gr, gt, B, 1.0, 10.0, 0, 0, rot, loss, draw, gtr, st)
        add(0, 0, tr.trans, gtr)
    else:
        _, bbox, K, _, _ = data
        z = tr.trans[:, 2].contiguous()                       # the pinhole's third component is z itself
        gtr = torch.full((B, 1), 7.0, device="cuda")
        call("zgeo_head_loss", raw, z, bbox, K, 1, gr, gt, B, 1.0, 10.0, 0, rot, trans, loss, draw, gtr, st)
        add(1, 2, trans, gtr, bbox, K)
    torch.cuda.synchronize()
    for name, a, b in zip(("loss", "draw", "dtrans / dz"), got, (loss, draw, gtr)):
        assert torch.equal(a, b), name
    # ... and the ADD term is in there: the three known samples have a per-sample value
    assert bool((tr.add_per[:3] > 0).all()) and float(tr.add_per[3]) == 0.0
    assert torch.equal(tr.add_per, per)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_graph_replay_equals_eager_and_follows_obj_ids(kind, dtype):
    """Two captured replays with different tr.obj_ids written between them are bit-identical
    to two eager steps, and differ from two replays on the first ids: the graph reads the
    buffer at run time."""
    tr, _ = _make(kind, dtype, add_loss=_crit(), add_weight=ADD_WEIGHT)
    data = _data(kind)
    snap = tr.snapshot()
    tr.obj_ids.copy_(_ids(IDS_A))
    tr.capture(data, warmup=1)
    assert len(tr.graphs) == 1

    def two_steps(step, second):
        tr.restore(snap)
        tr.obj_ids.copy_(_ids(IDS_A))
        step()
        step(obj_ids=_ids(second))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(tr.loss))
        return _state(tr)

    replayed = two_steps(tr.step, IDS_B)
    same_ids = two_steps(tr.step, IDS_A)
    tr.graphs = None                                           # step() now runs step_eager
    eager = two_steps(lambda obj_ids=None: tr.step(data, obj_ids=obj_ids), IDS_B)
    for a, b in zip(replayed, eager):
        assert torch.equal(a, b)
    assert not torch.equal(replayed[0], snap[0])
    assert not torch.equal(replayed[0], same_ids[0]) and not torch.equal(replayed[4], same_ids[4])


def _rel_frob(pairs):
    num = sum(float((a.double() - b.double()).pow(2).sum()) for a, b in pairs)
    den = sum(float(b.double().pow(2).sum()) for _, b in pairs)
    return (num / den) ** 0.5


def test_rgb_gradients_against_autograd():
    """RGBTrainer, fp32: the arena gradients after forward + backward against autograd through
    the drop-in PoseNetRGB under PoseLoss(1, 10) + 0.7 * ADDLoss.forward (relative Frobenius
    error over all parameters).  The yardstick is the same comparison without the criterion
    (add_loss=None, the behaviour before it existed); the mixed criterion must stay within
    2 x that (the margin covers the second loss term's own fp32 rounding).  Measured on an
    MI355X: 2.872e-06 under PoseLoss alone, 2.858e-06 with the ADD term."""
    from models.pose_loss import PoseLoss
    from models.pose_net_rgb import PoseNetRGB
    crit = _crit()
    data = _data("rgb")
    rgb, gr, gt = data
    ids = _ids(IDS_A)
    errs = {}
    for name, kw in (("pose", {"add_loss": None}), ("mixed", {"add_loss": crit, "add_weight": ADD_WEIGHT})):
        tr, P0 = _make("rgb", torch.float32, **kw)
        if name == "mixed":
            tr.obj_ids.copy_(ids)
        tr._forward_loss(*data)
        tr._trunk_backward(tr._head_backward())
        ref = PoseNetRGB(pretrained=False).cuda().set_compute_dtype(torch.float32)
        ref.load_state_dict(P0)
        ref.train()
        _dropouts_eval(ref)
        rot, trans = ref(rgb)
        loss = PoseLoss(1.0, 10.0, "geodesic")(rot, trans, gr, gt)
        if name == "mixed":
            loss = loss + ADD_WEIGHT * crit(rot, trans, gr, gt, ids)
        loss.backward()
        torch.cuda.synchronize()
        np.testing.assert_allclose(float(tr.loss), float(loss), rtol=1e-5)
        ours = dict(tr.model.named_parameters())
        errs[name] = _rel_frob([(tr.arena.grad_of(ours[k]), p.grad) for k, p in ref.named_parameters()])
        del tr, ref
    msg = f"relative Frobenius gradient error: PoseLoss alone {errs['pose']:.3e}, with the ADD term {errs['mixed']:.3e}"
    print(msg)
    assert errs["mixed"] <= 2 * errs["pose"], msg


def test_pure_add_step_rgbd_geometric():
    """rot_weight = trans_weight = 0: the step is ADDLoss.train_loss alone.  It moves the
    parameters, the (not learned) pinhole translation gets no gradient, and with every id -1
    (tr.obj_ids' initial value: no known object) the gradients are exactly zero."""
    tr, _ = _make("rgbd_geometric", torch.bfloat16, rot_weight=0.0, trans_weight=0.0, add_loss=_crit(),
                  add_weight=1.0)
    data = _data("rgbd_geometric")
    assert tr.obj_ids.dtype == torch.int64 and tr.obj_ids.tolist() == [-1] * B
    tr.step_eager(data)
    torch.cuda.synchronize()
    assert float(tr.loss) == 0.0 and bool((tr.arena.grad == 0).all())
    before = tr.arena.flat.clone()
    tr.step(data, obj_ids=_ids(IDS_A))
    torch.cuda.synchronize()
    assert float(tr.loss) > 0 and bool(torch.isfinite(tr.arena.grad).all())
    assert bool((tr.dtrans == 0).all())
    assert bool((tr.draw[:3] != 0).any()) and bool((tr.draw[3] == 0).all())
    assert bool((tr.arena.grad != 0).any()) and not torch.equal(tr.arena.flat, before)


def test_mesh_table_guard():
    """A captured graph bakes the mesh table's pointers in: editing ADDLoss.points after
    capture() makes step() raise; capture() again binds the new table."""
    from pose6d._lib import Pose6dError
    crit = _crit()
    tr, _ = _make("rgb", torch.bfloat16, add_loss=crit, add_weight=ADD_WEIGHT)
    data = _data("rgb")
    tr.obj_ids.copy_(_ids(IDS_A))
    tr.capture(data, warmup=1)
    tr.step()
    crit.points[0] = crit.points[0] * 1.5
    with pytest.raises(Pose6dError, match="mesh table changed"):
        tr.step()
    tr.capture(data, warmup=1)
    tr.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.loss))


def test_defaults_leave_the_trainer_as_it_was():
    """add_loss=None: no obj_ids buffer exists (so none is read), and the step runs."""
    tr, _ = _make("rgb", torch.bfloat16, add_loss=None)
    assert tr.add_loss is None and not hasattr(tr, "obj_ids")
    data = _data("rgb")
    before = tr.arena.flat.clone()
    tr.step(data)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.loss)) and not torch.equal(tr.arena.flat, before)
