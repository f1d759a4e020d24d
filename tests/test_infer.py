"""Detection-to-pose inference on the GPU (pose6d/infer.py): pose6d_crop_detections bit for
bit against tests/infer_ref.py (the numpy restatement of the reference's inference
scripts), pose6d_pose_project against the fixture recorded from the reference's own
project_points (tests/golden/infer.npz), and PoseEstimator against its parts.

All crops: 480 x 640 frames, F = 2, S = 224."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import infer_ref as IR

pytestmark = pytest.mark.gpu

H, W, F, S = 480, 640, 2, 224
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "infer.npz")

# (x1, y1, x2, y2): interior; left / top padding (the two K modes differ); right / bottom
# padding; crop side 14 (16x upscale); 448 = the exact-2x path, unpadded; exact-2x with right
# padding; half-pixel centre; crop side 224 (identity resize); the first box on frame 1
BOXES = [(200, 150, 320, 240), (-20, -30, 80, 110), (600, 430, 690, 500), (310, 220, 319, 232), (100, 60, 474, 400),
         (266, 100, 640, 420), (101, 50, 180, 111), (100, 100, 287, 250), (200, 150, 320, 240)]
FRAME_OF = [0, 0, 0, 0, 0, 0, 0, 0, 1]
IDENTITY = 7
NAMES = ("rgb", "depth", "depth_raw", "center_crop", "K_crop", "center_img", "K_img")


@functools.lru_cache(maxsize=None)
def _frames():
    rng = np.random.default_rng(11)
    rgb = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    depth = rng.integers(300, 1600, (F, H, W), dtype=np.uint16)
    depth[rng.random((F, H, W)) < 0.05] = 0
    return rgb, depth


def _K_frames():
    return np.stack([IR.DEFAULT_K, IR.DEFAULT_K * np.array([[1.01, 1, 0.98], [1, 0.99, 1.03], [1, 1, 1]])])


@functools.lru_cache(maxsize=None)
def _ref(depth_on=True, bgr=False, normalize=True, k_mode=0, per_frame=False):
    """The helper's outputs for BOXES, stacked; computed once per variant and shared."""
    rgb, depth = _frames()
    Ks = _K_frames()
    outs = []
    for box, f in zip(BOXES, FRAME_OF):
        img = rgb[f][..., ::-1] if bgr else rgb[f]
        kw = {} if normalize else {"mean": None}
        outs.append(IR.crop_detection(np.ascontiguousarray(img), depth[f] if depth_on else None, box,
                                      Ks[f] if per_frame else IR.DEFAULT_K, S, k_mode=k_mode, **kw))
    ref = [np.stack([o[i] for o in outs]) for i in range(7)]
    for a in ref:
        a.setflags(write=False)
    return ref


def _dev_frames():
    rgb, depth = _frames()
    return torch.from_numpy(rgb).cuda(), torch.from_numpy(depth.astype(np.int32)).cuda().to(torch.uint16)


def _float_boxes():
    # fractional parts pointing AWAY from zero: int() must truncate toward zero, not floor
    return [tuple(v + (0.7 if v >= 0 else -0.7) for v in b) for b in BOXES]


VARIANTS = {
    "default": {},
    "no_depth": {"depth_on": False},
    "bgr": {"bgr": True},
    "no_normalize": {"normalize": False},
    "dataset_K": {"k_mode": 1},
    "K_per_frame": {"per_frame": True},
    "float_boxes": {},
    "device_boxes": {},
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_crops_bit_exact(variant):
    from pose6d.infer import CropDetections
    kw = VARIANTS[variant]
    rgb, depth = _dev_frames()
    crop = CropDetections(S, normalize=kw.get("normalize", True), bgr=kw.get("bgr", False),
                          dataset_intrinsics=bool(kw.get("k_mode", 0)))
    boxes, frame_of = BOXES, FRAME_OF
    if variant == "float_boxes":
        boxes = _float_boxes()
        assert boxes[1][0] == -20.7 and boxes[1][2] == 80.7
    if variant == "device_boxes":
        boxes = torch.tensor(BOXES, dtype=torch.int32).cuda()
        frame_of = torch.tensor(FRAME_OF, dtype=torch.int32).cuda()
    K = _K_frames() if kw.get("per_frame") else IR.DEFAULT_K
    got = crop(rgb, depth if kw.get("depth_on", True) else None, boxes, frame_of, K)
    torch.cuda.synchronize()
    crop.check()
    ref = _ref(**kw)
    for name, g, r in zip(NAMES, got, ref):
        r = torch.tensor(r.reshape(g.shape))   # (a copy: the shared reference is read-only)
        assert g.dtype == torch.float32
        assert torch.equal(g.cpu(), r), (variant, name, (g.cpu() - r).abs().max().item())
    if variant == "dataset_K":   # where a box is padded on the left / top the two modes differ
        r0 = _ref()
        assert not np.array_equal(r0[4][1], ref[4][1]) and np.array_equal(r0[4][0], ref[4][0])


def test_single_frame_without_frame_of():
    from pose6d.infer import CropDetections
    rgb, depth = _dev_frames()
    got = CropDetections(S)(rgb[0], depth[0], BOXES[:3])
    ref = _ref()
    for g, r in zip(got, ref):
        assert torch.equal(g.cpu(), torch.tensor(r[:3].reshape(g.shape)))


def test_bad_frame_index_zero_fills_and_reports():
    from pose6d import Pose6dError
    from pose6d.infer import CropDetections
    rgb, depth = _dev_frames()
    crop = CropDetections(S)
    bx = torch.tensor(BOXES, dtype=torch.int32).cuda()
    fo = torch.tensor(FRAME_OF, dtype=torch.int32).cuda()
    fo[2], fo[5] = -1, F
    out = crop.empty_outputs(len(BOXES), rgb.device)
    for t in out:
        t.fill_(7.0)
    got = crop(rgb, depth, bx, fo, out=out)
    ref = _ref()
    for g, r in zip(got, ref):
        g = g.cpu()
        r = torch.tensor(r.reshape(g.shape))
        r[2], r[5] = 0, 0
        assert torch.equal(g, r)
    with pytest.raises(Pose6dError, match=r"frame_of\[5\]"):   # the highest bad position + 1
        crop.check()
    crop.check()   # reset
    with pytest.raises(Pose6dError):   # host-side lists are refused before any launch
        crop(rgb, depth, BOXES, [0] * 8 + [2])
    with pytest.raises(Pose6dError):
        crop(rgb, depth, [(10, 10, 10, 30)], [0])


def test_depth_is_the_float_path_not_crop_rgbd():
    """Against CropRGBD (the dataset's 16U resize, rounded to whole millimetres) on the same
    boxes: every crop's depth differs, except the identity resize (crop side 224: every
    weight is 0 or 1, so both paths return the source pixels) where they must agree."""
    from pose6d.data import CropRGBD
    rgb, depth = _dev_frames()
    idx = torch.tensor(FRAME_OF).cuda()
    xywh = torch.tensor([(a, b, c - a, d - b) for a, b, c, d in BOXES], dtype=torch.int32).cuda()
    K = torch.from_numpy(np.tile(IR.DEFAULT_K.astype(np.float32), (len(BOXES), 1, 1))).cuda()
    dsel = depth.view(torch.int16)[idx].view(torch.uint16)   # (indexing has no uint16 kernel)
    _, d16, raw16, _, _ = CropRGBD(S)(rgb[idx], dsel, xywh, xywh, K)
    ref = _ref()
    d32, raw32 = torch.tensor(ref[1]).cuda(), torch.tensor(ref[2]).cuda()
    for i in range(len(BOXES)):
        same = torch.equal(raw16[i], raw32[i]), torch.equal(d16[i], d32[i])
        assert same == ((True, True) if i == IDENTITY else (False, False)), (i, same)
    # and the RGB crop is the same 8U path
    rgb16 = CropRGBD(S)(rgb[idx], dsel, xywh, xywh, K)[0]
    assert torch.equal(rgb16.cpu(), torch.tensor(ref[0]))


# ----------------------------------------------------------------- projection
@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def _project(gold, **kw):
    from pose6d.infer import pose_project
    n = gold["quat"].shape[0]
    out = pose_project(torch.from_numpy(gold["quat"]).cuda(), torch.from_numpy(gold["trans"]).cuda(), gold["K"],
                       torch.zeros(n, dtype=torch.int64).cuda(), torch.from_numpy(gold["corners"][None]).cuda(), **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def test_projection_against_the_reference_fixture(gold):
    trans, pts, pix, valid = _project(gold)
    assert pts.dtype == np.float64 and pix.dtype == np.int64 and trans.dtype == np.float64
    assert np.all(valid == 1)
    assert np.array_equal(trans, gold["trans"].astype(np.float64))
    p3 = np.concatenate([gold["corners"], gold["axes"]])
    worst = 0.0
    for i in range(len(pts)):
        bound = IR.projection_bound(p3, gold["quat"][i], gold["trans"][i], gold["K"])
        err = np.abs(pts[i] - gold["pts"][i])
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (i, float((err / bound).max()))
    print(f"projection: worst error / bound = {worst:.3f}")
    assert np.array_equal(pix, gold["pix"])       # every element, the clipped points included
    assert np.array_equal(pix, pts.astype(np.int64))


def test_translation_correction_with_and_without_boxes(gold):
    n = gold["quat"].shape[0]
    rng = np.random.default_rng(5)
    x1, y1 = rng.integers(-50, 500, n), rng.integers(-50, 400, n)
    boxes = np.stack([x1, y1, x1 + rng.integers(1, 200, n), y1 + rng.integers(1, 200, n)], 1).astype(np.int32)
    trans, pts, pix, valid = _project(gold, boxes=torch.from_numpy(boxes).cuda())
    K = gold["K"]
    z = gold["trans"][:, 2].astype(np.float64)
    cx, cy = (boxes[:, 0] + boxes[:, 2]) / 2, (boxes[:, 1] + boxes[:, 3]) / 2
    exp = np.stack([(cx - K[0, 2]) * z / K[0, 0], (cy - K[1, 2]) * z / K[1, 1], z], 1)
    assert np.array_equal(trans, exp)
    # the projection uses the corrected translation: the origin lands on the box centre
    assert np.abs(pts[:, 8, 0] - cx).max() < 1e-9 and np.abs(pts[:, 8, 1] - cy).max() < 1e-9
    # per-frame K: row frame_of[i]
    Ks = np.stack([K, K * 1.5])
    fo = torch.from_numpy((np.arange(n) % 2).astype(np.int32)).cuda()
    t2, p2, _, _ = _project({**{k: gold[k] for k in gold.files}, "K": Ks}, frame_of=fo)
    t1, p1, _, _ = _project(gold)
    assert np.array_equal(p2[0::2], p1[0::2]) and not np.array_equal(p2[1::2], p1[1::2])


def test_projection_valid_flags(gold):
    from pose6d.infer import pose_project
    quat = torch.from_numpy(gold["quat"][:5].copy()).cuda()
    quat[2] = 0
    trans = torch.from_numpy(gold["trans"][:5]).cuda()
    obj = torch.tensor([0, -1, 0, 1, 0]).cuda()
    out = pose_project(quat, trans, gold["K"], obj, torch.from_numpy(gold["corners"][None]).cuda())
    trans_o, pts, pix, valid = [t.cpu().numpy() for t in out]
    assert valid.tolist() == [1, 0, 0, 0, 1]
    for i in (1, 2, 3):
        assert not trans_o[i].any() and not pts[i].any() and not pix[i].any()
    assert np.array_equal(pix[[0, 4]], gold["pix"][[0, 4]])


# ----------------------------------------------------------------- PoseEstimator
KINDS = ("PoseNetRGB", "PoseNetRGBD", "PoseNetRGBGeometric", "PoseNetRGBDGeometric")
_MODELS = {}


def _model(kind, dtype):
    """One random-weight model per kind for the whole module (BatchNorm statistics moved off
    their initial values), switched to the compute dtype asked for."""
    from tests.test_models import _models
    m = _MODELS.get(kind)
    if m is None:
        torch.manual_seed(0)
        m = _models()[kind](pretrained=False)
        g = torch.Generator().manual_seed(17)
        for mod in m.modules():
            if isinstance(mod, (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d)):
                mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.05)
                mod.running_var.copy_(torch.rand(mod.num_features, generator=g) * 0.5 + 0.75)
        m = _MODELS[kind] = m.cuda().eval()
    return m.set_compute_dtype(dtype)


def _corners(gold):
    # class 0 and class 2 have a mesh, class 1 has none
    return {"01": gold["corners"], "02": None, "04": gold["corners"] * 1.25}


CLASS_TO_OBJ = {0: "01", 1: "02", 2: "04"}
DET = [BOXES[0], BOXES[1], BOXES[6]]
DET_CLS = [0, 2, 0]


def _same(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("quat", "trans", "trans_cam", "points", "pixels",
                                                                    "valid"))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_estimator_equals_its_parts(kind, dtype, gold):
    from pose6d.infer import CropDetections, PoseEstimator, _KINDS, pose_project
    model = _model(kind, dtype)
    rgb, depth = _dev_frames()
    est = PoseEstimator(model, _corners(gold), class_to_obj=CLASS_TO_OBJ, max_frames=F, graph=True)
    eager = PoseEstimator(model, _corners(gold), class_to_obj=CLASS_TO_OBJ, max_frames=F, graph=False)
    fo = [0, 1, 0]
    res = est(rgb, depth, DET, DET_CLS, fo).clone()
    assert res.quat.shape == (3, 4) and res.trans.shape == (3, 3) and res.box2d.shape == (3, 8, 2)
    assert res.axes2d.shape == (3, 4, 2) and res.points.shape == (3, 12, 2) and res.box2d.dtype == torch.int64
    assert res.valid.tolist() == [True, True, True]
    # the parts, on the same padded 4-detection batch (detection 0 repeated)
    pad_boxes, pad_fo = DET + [DET[0]], fo + [fo[0]]
    crops = CropDetections(S)(rgb, depth, pad_boxes, pad_fo)
    bk = est._buckets[(4, True)]
    for a, b in zip(bk.crops, crops):
        assert torch.equal(a, b)
    with torch.no_grad():
        quat, trans = model(*_KINDS[kind][0](crops))
    assert torch.equal(res.quat, quat[:3]) and torch.equal(res.trans, trans.reshape(4, 3)[:3])
    corrects = kind in ("PoseNetRGB", "PoseNetRGBD")
    assert est.corrects_translation == corrects
    obj = torch.tensor([0, 1, 0, 0]).cuda()   # rows of the table built from the dict: "01" -> 0, "04" -> 1
    bx = torch.tensor(pad_boxes, dtype=torch.int32).cuda()
    t_cam, pts, pix, valid = pose_project(quat, trans.reshape(4, 3), IR.DEFAULT_K, obj, est.corners,
                                          boxes=bx if corrects else None)
    assert torch.equal(res.trans_cam, t_cam[:3]) and torch.equal(res.points, pts[:3])
    assert torch.equal(res.pixels, pix[:3]) and torch.equal(res.box2d, pix[:3, :8])
    if corrects:   # x, y from the box centre's ray at the predicted z
        z = res.trans[:, 2].double().cpu().numpy()
        c = np.array([((a + c_) / 2, (b + d) / 2) for a, b, c_, d in DET])
        K = IR.DEFAULT_K
        exp = np.stack([(c[:, 0] - K[0, 2]) * z / K[0, 0], (c[:, 1] - K[1, 2]) * z / K[1, 1], z], 1)
        assert np.array_equal(res.trans_cam.cpu().numpy(), exp)
    else:
        assert torch.equal(res.trans_cam, res.trans.double())
    # graph == no graph, bit for bit, also after new frame and box contents
    assert _same(res, eager(rgb, depth, DET, DET_CLS, fo))
    rgb2, depth2 = rgb.flip(0).contiguous(), depth.view(torch.int16).flip(0).contiguous().view(torch.uint16)
    det2 = [BOXES[2], BOXES[3], BOXES[5]]
    a = est(rgb2, depth2, det2, [2, 0, 0], [1, 1, 0])
    b = eager(rgb2, depth2, det2, [2, 0, 0], [1, 1, 0])
    assert _same(a, b) and not torch.equal(a.quat, res.quat)
    host = a.cpu()
    assert not host.quat.is_cuda and torch.equal(host.pixels, a.pixels.cpu()) and host.valid.tolist() == [True] * 3
    est.check()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_estimator_buckets_padding_and_refresh(kind, dtype, gold):
    from pose6d import Pose6dError
    from pose6d.infer import PoseEstimator
    model = _model(kind, dtype)
    rgb, depth = _dev_frames()
    mk = lambda: PoseEstimator(model, _corners(gold), class_to_obj=CLASS_TO_OBJ, max_frames=F, graph=True)
    est = mk()
    fo = [0, 1, 0]
    r4 = est(rgb, depth, DET, DET_CLS, fo).clone()
    # the padding row repeats detection 0; making detection 0 another box changes rows 1, 2 not at all
    alt = est(rgb, depth, [BOXES[4]] + DET[1:], DET_CLS, fo).clone()
    for k in ("quat", "trans", "trans_cam", "points", "pixels"):
        assert torch.equal(getattr(alt, k)[1:], getattr(r4, k)[1:]), k
    assert not torch.equal(alt.quat[0], r4.quat[0])
    # buckets 4 -> 1 -> 8 -> 4: each has its own graph and engines; results do not depend on the order
    r1 = est(rgb, depth, DET[:1], DET_CLS[:1], fo[:1]).clone()
    r8 = est(rgb, depth, (DET * 2)[:5], (DET_CLS * 2)[:5], (fo * 2)[:5]).clone()
    assert sorted(b for b, _ in est._buckets) == [1, 4, 8]
    assert r1.quat.shape == (1, 4) and r8.quat.shape == (5, 4) and r8.points.shape == (5, 12, 2)
    assert _same(est(rgb, depth, DET, DET_CLS, fo), r4)
    assert torch.equal(r8.pixels[3], r8.pixels[0]) and torch.equal(r8.quat[4], r8.quat[1])
    # a class without a mesh: valid False, rows zero, the others untouched
    rv = est(rgb, depth, DET, [0, 1, 0], fo)
    assert rv.valid.tolist() == [True, False, True] and not rv.pixels[1].any() and not rv.points[1].any()
    assert torch.equal(rv.pixels[0], r4.pixels[0]) and torch.equal(rv.quat, r4.quat)
    # N = 0: empty tensors, no launch; N = 33 raises
    r0 = est(rgb, depth, [], [])
    assert r0.quat.shape == (0, 4) and r0.box2d.shape == (0, 8, 2) and r0.points.shape == (0, 12, 2)
    assert r0.valid.shape == (0,) and sorted(b for b, _ in est._buckets) == [1, 4, 8]
    with pytest.raises(Pose6dError, match="max_detections"):
        est(rgb, depth, [BOXES[0]] * 33, [0] * 33)
    # without depth: a graph of its own
    if kind in ("PoseNetRGB", "PoseNetRGBGeometric"):
        assert torch.equal(est(rgb, None, DET, DET_CLS, fo).quat, r4.quat)
        assert (4, False) in est._buckets
    # an in-place weight write is taken over by refresh(), and matches a fresh estimator
    w = model.rot_head[0].weight
    c = next(p for n, p in model.named_parameters() if n.endswith("backbone.0.weight"))
    keep = w.detach().clone(), c.detach().clone()
    try:
        with torch.no_grad():
            w.mul_(1.5)
            c.mul_(0.5)
        after = est.refresh()(rgb, depth, DET, DET_CLS, fo).clone()
        assert not torch.equal(after.quat, r4.quat)
        assert _same(after, mk()(rgb, depth, DET, DET_CLS, fo))
    finally:
        with torch.no_grad():
            w.copy_(keep[0])
            c.copy_(keep[1])
    assert _same(est.refresh()(rgb, depth, DET, DET_CLS, fo), r4)
    # a model in training mode is refused
    model.train()
    try:
        with pytest.raises(Pose6dError, match="training"):
            mk()
        with pytest.raises(Pose6dError, match="training"):
            est(rgb, depth, DET, DET_CLS, fo)
    finally:
        model.eval()


def test_infer_pose_command_line(gold, tmp_path):
    """tools/infer_pose.py end to end, in process: PNG frame + detections JSON + checkpoint ->
    the poses PoseEstimator gives for the same inputs."""
    import json
    from PIL import Image
    from pose6d.infer import PoseEstimator
    from tools import infer_pose
    model = _model("PoseNetRGBDGeometric", torch.float32)
    rgb, depth = _frames()
    Image.fromarray(rgb[0]).save(tmp_path / "f.png")
    Image.fromarray(depth[0]).save(tmp_path / "d.png")
    torch.save({"epoch": 1, "model_state_dict": model.state_dict()}, tmp_path / "w.pth")
    IR.write_ply(tmp_path / "obj_01.ply", gold["mesh_verts_mm"])
    dets = [{"xyxy": [200.7, 150.2, 320.9, 240.1], "cls": 0, "conf": 0.9}, {"xyxy": [-20, -30, 80, 110], "cls": 1,
                                                                            "conf": 0.5}]
    (tmp_path / "dets.json").write_text(json.dumps(dets))
    rc = infer_pose.main(["--model", "RGBD-Geometric", "--weights", str(tmp_path / "w.pth"), "--image",
                          str(tmp_path / "f.png"), "--depth", str(tmp_path / "d.png"), "--detections",
                          str(tmp_path / "dets.json"), "--mesh-dir", str(tmp_path), "--out", str(tmp_path / "o.json")])
    assert rc == 0
    poses = json.loads((tmp_path / "o.json").read_text())["poses"]
    assert [p["valid"] for p in poses] == [True, False] and [p["obj"] for p in poses] == ["01", "02"]
    from pose6d.infer import load_mesh_corners
    est = PoseEstimator(model, {"01": load_mesh_corners(str(tmp_path), "01")}, graph=False)
    ref = est(rgb[0], depth[0], [BOXES[0], BOXES[1]], ["01", "02"]).cpu()
    assert poses[0]["box2d"] == ref.box2d[0].tolist() and poses[0]["axes2d"] == ref.axes2d[0].tolist()
    assert poses[0]["quat_xyzw"] == ref.quat[0].tolist() and poses[1]["quat_xyzw"] == ref.quat[1].tolist()
    assert poses[0]["xyxy"] == [200, 150, 320, 240]
