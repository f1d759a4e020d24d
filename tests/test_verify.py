"""Pose verification on the GPU (pose6d_pose_verify through pose6d.infer.PoseVerifier and
PoseEstimator(verify=...)) against the fp64 numpy restatement tests/verify_ref.py.

Frames are tests/refine_ref.py's 480 x 640 renders of a 0.10 x 0.06 x 0.04 m box; the meshes
are verify_ref.box_mesh's (12, 768 and 27 648 triangles).  The z-buffer, the classes, the
counts, fit and agree must EQUAL the restatement's (`==`); resid is a sum of at most 4096
non-negative terms in another order, so it may differ by a relative 4096 x 2^-52."""
import numpy as np
import pytest
import torch

from tests import refine_ref as RR
from tests import verify_ref as VR

pytestmark = pytest.mark.gpu

K = RR.DEFAULT_K
TAU = 0.1
RESID_RTOL = 4096 * 2.0 ** -52


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))   # (a copy: the shared scenes are read-only)
    return (t if dtype is None else t.to(dtype)).cuda()


def _depth_dev(frames):
    return _dev(np.stack(frames).astype(np.int32)).to(torch.uint16)


def _call(ver, frames, boxes, slots, quat, trans, frame_of=None, maps=True):
    out = ver(_depth_dev(frames), _dev(np.asarray(boxes, np.int32)), _dev(np.asarray(slots, np.int64)),
              _dev(np.asarray(quat, np.float32)), _dev(np.asarray(trans, np.float64)),
              frame_of=None if frame_of is None else _dev(np.asarray(frame_of, np.int32)), K=K, maps=maps)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out._asdict().items()}


def _same(o, n, want, what):
    """Row n of the launch's outputs against one restatement result."""
    assert np.array_equal(o["zbuf"][n], want["zbuf"]), what          # +inf == +inf
    assert np.array_equal(o["cls"][n], want["cls"]), what
    assert np.array_equal(o["counts"][n], want["counts"]), what
    assert o["fit"][n] == want["fit"] and o["agree"][n] == want["agree"], what
    assert abs(o["resid"][n] - want["resid"]) <= RESID_RTOL * want["resid"], (what, o["resid"][n], want["resid"])
    assert o["verified"][n] == want["verified"], what


def _zero_row(o, n):
    return (o["verified"][n] == 0 and not o["counts"][n].any() and o["fit"][n] == 0 and o["agree"][n] == 0
            and o["resid"][n] == 0 and np.isposinf(o["zbuf"][n]).all() and not o["cls"][n].any())


# ----------------------------------------------------------------- 1. bit equality
@pytest.mark.parametrize("n,G", [(8, 1), (8, 8), (8, 32), (8, 64), (1, 32), (48, 32)])
def test_equals_the_restatement(n, G):
    """Scene 100 at its initial pose (every class but 1 occurs) and scene 101 at the truth, one
    launch: G = 1 .. 64 on the 768-triangle mesh; 12 triangles that cover hundreds of samples
    each; 27 648 sub-sample triangles, 27 per lane."""
    from pose6d.infer import PoseVerifier
    verts, faces = VR.box_mesh(n)
    ver = PoseVerifier({"a": (verts, faces)}, {"a": RR.DIAMETER}, grid=G, tau=TAU)
    sc = [RR.scene(100), RR.scene(101)]
    quat = np.stack([sc[0]["q0"], sc[1]["q_gt"].astype(np.float32) * -3.0])   # need not be unit, nor have w >= 0
    trans = np.stack([sc[0]["t0"], sc[1]["t_gt"]])
    o = _call(ver, [s["depth"] for s in sc], [s["box"] for s in sc], [0, 0], quat, trans, [0, 1])
    assert o["zbuf"].shape == (2, G * G) and o["cls"].dtype == np.uint8 and o["counts"].shape == (2, 5)
    hits = 0
    for i, s in enumerate(sc):
        want = VR.verify(s["depth"], K, s["box"], verts, faces, RR.DIAMETER, quat[i], trans[i], G=G, tau=TAU)
        _same(o, i, want, (n, G, i))
        hits += int((want["cls"] > 0).sum())
    assert hits > 0 or G == 1
    if G == 32:
        assert (o["counts"][0, 2:] > 0).all() and o["fit"][1] >= 0.9


def test_batch_with_two_slots_and_every_edge():
    """One launch, two slots (768 and 12 triangles, different diameters).  Rows: 0 a box
    hanging over the frame's left and top edges; 1 a pose behind the camera (all class 0); 2 a
    pose whose mesh straddles z = 0.001; 3 obj = -1; 4 a NaN quaternion; 5 frame_of outside
    [0, F); 6 a zero quaternion; 7 obj past the table.  (Six kinds of row are asked for: the
    batch has more than five rows.)"""
    from pose6d.infer import PoseVerifier
    meshes = {"a": VR.box_mesh(8), "b": VR.box_mesh(1)}
    diam = {"a": RR.DIAMETER, "b": 0.2}
    ver = PoseVerifier(meshes, diam, grid=32, tau=TAU)
    s = RR.scene(100)
    corner = RR.scene(100, t_gt=(-0.40, -0.29, 0.8))   # the same object in the frame's top left corner
    over = (-31, -23, corner["box"][2], corner["box"][3])
    frames = [s["depth"], corner["depth"]]
    keys = ["a", "b", "b", "a", "a", "a", "b", "a"]
    slots = [0, 1, 1, -1, 0, 0, 1, 2]
    frame_of = [1, 0, 0, 0, 0, 2, 0, 0]
    boxes = [over] + [s["box"]] * 7
    quat = np.stack([corner["q0"]] + [s["q0"]] * 7)
    trans = np.stack([corner["t0"]] + [s["t0"]] * 7)
    trans[1] = [0.0, 0.0, -0.8]
    trans[2] = [0.002, -0.001, 0.01]
    quat[4, 2] = np.nan
    quat[6] = 0
    o = _call(ver, frames, boxes, slots, quat, trans, frame_of)
    u, v = RR.sample_pixels(over, 32)
    assert (u < 0).any() and (v < 0).any()
    for i in (0, 1, 2):
        vt, fc = meshes[keys[i]]
        want = VR.verify(frames[frame_of[i]], K, boxes[i], vt, fc, diam[keys[i]], quat[i], trans[i], G=32, tau=TAU)
        _same(o, i, want, i)
    # over the edges: a hit outside the frame has no depth
    off = (u < 0) | (v < 0)
    assert (o["cls"][0][off & np.isfinite(o["zbuf"][0])] == 1).all() and (o["cls"][0][off] == 1).any()
    assert o["counts"][0][2] > 100
    # behind the camera: verified, nothing rendered
    assert o["verified"][1] == 1 and o["counts"][1].tolist() == [1024, 0, 0, 0, 0] and o["fit"][1] == 0
    # straddling: some triangles are skipped, the others render
    z = VR.project_vertices(meshes["b"][0], quat[2], trans[2], K)[2]
    assert (z <= 0.001).any() and (z[meshes["b"][1]] > 0.001).all(1).any() and o["verified"][2] == 1
    for i in (3, 4, 5, 6, 7):
        assert _zero_row(o, i), i
    # without the maps: the same results
    o2 = _call(ver, frames, boxes, slots, quat, trans, frame_of, maps=False)
    assert o2["zbuf"] is None and o2["cls"] is None
    for k in ("counts", "fit", "agree", "resid", "verified"):
        assert np.array_equal(o2[k], o[k]), k


# ----------------------------------------------------------------- 2. a bad face in the table
def test_face_with_an_index_outside_the_mesh_is_skipped():
    """Injected into the packed table after construction (the constructor refuses it): the
    result is the restatement's without those faces."""
    from pose6d.infer import PoseVerifier
    verts, faces = VR.box_mesh(8)
    ver = PoseVerifier({"x": VR.box_mesh(1), "a": (verts, faces)}, {"x": 0.2, "a": RR.DIAMETER}, grid=32, tau=TAU)
    s = RR.scene(100)
    q, t = s["q_gt"].astype(np.float32), s["t_gt"]
    whole = VR.scene_fit(100, "true")
    # the faces the true pose shows nearest at some sample: dropping one changes the z-buffer
    T = ver.table(torch.device("cuda", torch.cuda.current_device()))
    base = 12   # slot 1's first triangle
    assert T[4].tolist() == [0, base] and T[2].tolist() == [0, 24] and T[3].tolist() == [24, len(verts)]
    bad = [5, 300, 301, 767]
    T[1][base + 5, 1] = len(verts)          # one past the mesh's vertices
    T[1][base + 300, 0] = -1
    T[1][base + 301, 2] = 2 ** 31 - 1
    T[1][base + 767, 0] = -(2 ** 31)
    o = _call(ver, [s["depth"]], [s["box"]], [1], q[None], t[None])
    want = VR.verify(s["depth"], K, s["box"], verts, np.delete(faces, bad, axis=0), RR.DIAMETER, q, t, G=32, tau=TAU)
    _same(o, 0, want, "bad faces")
    assert o["verified"][0] == 1
    assert not np.array_equal(want["zbuf"], whole["zbuf"])   # the dropped faces were visible ones


# ----------------------------------------------------------------- 3. determinism
def test_same_call_twice_same_bytes():
    from pose6d.infer import PoseVerifier
    sc = [RR.scene(s) for s in RR.SEEDS[:3]]
    ver = PoseVerifier({"a": VR.box_mesh(48)}, {"a": RR.DIAMETER}, grid=64, tau=TAU)
    args = ([s["depth"] for s in sc], [s["box"] for s in sc], [0, 0, 0], np.stack([s["q0"] for s in sc]),
            np.stack([s["t0"] for s in sc]), [0, 1, 2])
    a, b = _call(ver, *args), _call(ver, *args)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["verified"].tolist() == [1, 1, 1] and (a["counts"][:, 2] > 0).all()


# ----------------------------------------------------------------- 4. the ranking, whole path
def test_refined_pose_fits_better_on_the_twelve_scenes():
    """DepthRefiner then PoseVerifier on the GPU, the 12 scenes as one N = 12 call each:
    fit(refined) > fit(initial) on every scene, and both equal the restatement's on its own
    poses wherever the refinement picked the restatement's pairs."""
    from pose6d.infer import DepthRefiner, PoseVerifier
    sc = [RR.scene(s) for s in RR.SEEDS]
    ref = DepthRefiner({i: s["mesh"] for i, s in enumerate(sc)}, {i: s["diam"] for i, s in enumerate(sc)})
    ver = PoseVerifier({"a": VR.box_mesh(8)}, {"a": RR.DIAMETER}, grid=32, tau=TAU)
    depth = _depth_dev([s["depth"] for s in sc])
    boxes = _dev(np.asarray([s["box"] for s in sc], np.int32))
    fo = _dev(np.arange(12, dtype=np.int32))
    q0, t0 = _dev(np.stack([s["q0"] for s in sc])), _dev(np.stack([s["t0"] for s in sc]))
    r = ref(depth, boxes, _dev(np.arange(12, dtype=np.int64)), q0, t0, frame_of=fo, K=K)
    slots = _dev(np.zeros(12, np.int64))
    before = ver(depth, boxes, slots, q0, t0, frame_of=fo, K=K)
    after = ver(depth, boxes, slots, r.quat32, r.trans, frame_of=fo, K=K)
    torch.cuda.synchronize()
    assert r.refined.bool().all() and before.verified.bool().all() and after.verified.bool().all()
    fb, fa = before.fit.cpu().numpy(), after.fit.cpu().numpy()
    for i, seed in enumerate(RR.SEEDS):
        print(f"seed {seed}: fit {fb[i]:.4f} -> {fa[i]:.4f} (restatement {VR.scene_fit(seed, 'initial')['fit']:.4f} -> "
              f"{VR.scene_fit(seed, 'refined')['fit']:.4f})")
        assert fb[i] == VR.scene_fit(seed, "initial")["fit"], seed
        assert fa[i] > fb[i], seed


# ----------------------------------------------------------------- 5. PoseEstimator(verify=...)
_FIELDS = ("quat", "trans", "trans_cam", "points", "pixels", "valid")
_REF_FIELDS = ("quat_ref", "trans_ref", "points_ref", "pixels_ref", "n_corr", "rms", "refined")
_VER_FIELDS = ("fit", "agree", "counts", "resid", "verified")


def test_estimator_with_verification():
    """N = 3 detections in bucket 4 (the padded row must not leak), a model whose last layers
    emit scene 100's perturbed pose (weights 0, bias = the pose), so that there is something to
    verify and to refine."""
    from pose6d import Pose6dError
    from pose6d.infer import DepthRefiner, PoseEstimator, PoseVerifier, RefinedPoseResult
    from tests.test_models import _models
    torch.manual_seed(0)
    model = _models()["PoseNetRGB"](pretrained=False).cuda().eval()
    sc = [RR.scene(100), RR.scene(101)]
    with torch.no_grad():
        model.rot_head[-1].weight.zero_()
        model.rot_head[-1].bias.copy_(torch.from_numpy(sc[0]["q0"].copy()))
        model.trans_head[-1].weight.zero_()
        model.trans_head[-1].bias.copy_(torch.from_numpy(sc[0]["t0"].astype(np.float32)))
    rng = np.random.default_rng(2)
    rgb = torch.from_numpy(rng.integers(0, 256, (2, RR.H, RR.W, 3), dtype=np.uint8)).cuda()
    depth = _depth_dev([s["depth"] for s in sc])
    lo, hi = -RR.BOX / 2, RR.BOX / 2
    box8 = np.array([[(lo, hi)[(i >> a) & 1][a] for a in range(3)] for i in (0, 1, 3, 2, 4, 5, 7, 6)])
    corners = {"a": box8, "b": None}
    mk_ref = lambda: DepthRefiner({"a": sc[0]["mesh"]}, {"a": RR.DIAMETER}, iters=3)
    mk_ver = lambda: PoseVerifier({"a": VR.box_mesh(8)}, {"a": RR.DIAMETER}, grid=32, tau=TAU)
    boxes, classes, fo = [sc[0]["box"], sc[1]["box"], sc[0]["box"]], ["a", "a", "b"], [0, 1, 0]
    kw = {"max_frames": 2}
    plain = PoseEstimator(model, corners, graph=True, **kw)
    with_ref = PoseEstimator(model, corners, graph=True, refine=mk_ref(), **kw)
    p = plain(rgb, depth, boxes, classes, fo).clone()
    pr = with_ref(rgb, depth, boxes, classes, fo).clone()
    assert type(p).__name__ == "PoseResult" and type(pr).__name__ == "RefinedPoseResult"
    assert not hasattr(p, "fit") and not hasattr(pr, "best")

    # ---- verify alone
    est = PoseEstimator(model, corners, graph=True, verify=mk_ver(), **kw)
    eager = PoseEstimator(model, corners, graph=False, verify=mk_ver(), **kw)
    res = est(rgb, depth, boxes, classes, fo).clone()
    assert type(res).__name__ == "VerifiedPoseResult" and not isinstance(res, RefinedPoseResult)
    assert res.fit.shape == (3,) and res.fit.dtype == torch.float64 and res.counts.shape == (3, 5)
    assert res.counts.dtype == torch.int32 and res.verified.dtype == torch.bool and not hasattr(res, "best")
    for _ in range(2):   # the second call is a pure replay
        g, e = est(rgb, depth, boxes, classes, fo), eager(rgb, depth, boxes, classes, fo)
        for k in _FIELDS + _VER_FIELDS:
            assert torch.equal(getattr(g, k), getattr(e, k)), k
            assert torch.equal(getattr(g, k), getattr(res, k)), k
    for k in _FIELDS:   # every earlier field is what an estimator without verify= gives
        assert torch.equal(getattr(res, k), getattr(p, k)), k
    # the new fields are PoseVerifier on (quat, trans_cam) of the three detections
    ver = mk_ver()
    bx = torch.tensor(boxes, dtype=torch.int32).cuda()
    fo_d = torch.tensor(fo, dtype=torch.int32).cuda()
    slots = torch.from_numpy(ver.slots(classes)).cuda()
    d = ver(depth, bx, slots, res.quat, res.trans_cam, frame_of=fo_d)
    for k in _VER_FIELDS:
        want = getattr(d, k).bool() if k == "verified" else getattr(d, k)
        assert torch.equal(want, getattr(res, k)), k
    assert res.verified.tolist() == [True, True, False] and not res.counts[2].any() and res.fit[2] == 0
    print("verify alone: fit", res.fit.tolist(), "counts", res.counts.tolist())
    assert res.counts[0, 2] > 0    # the emitted pose is 3-8 degrees and millimetres off scene 100's truth
    host = res.cpu()
    assert type(host) is type(res) and torch.equal(host.fit, res.fit.cpu()) and host.counts.shape == (3, 5)

    # ---- with refine= as well
    both = PoseEstimator(model, corners, graph=True, refine=mk_ref(), verify=mk_ver(), **kw)
    both_eager = PoseEstimator(model, corners, graph=False, refine=mk_ref(), verify=mk_ver(), **kw)
    rb = both(rgb, depth, boxes, classes, fo).clone()
    assert type(rb).__name__ == "VerifiedRefinedPoseResult" and isinstance(rb, RefinedPoseResult)
    ref_fields = tuple(k + "_ref" for k in _VER_FIELDS)
    for _ in range(2):
        g, e = both(rgb, depth, boxes, classes, fo), both_eager(rgb, depth, boxes, classes, fo)
        for k in _FIELDS + _REF_FIELDS + _VER_FIELDS + ref_fields + ("best",):
            assert torch.equal(getattr(g, k), getattr(e, k)), k
            assert torch.equal(getattr(g, k), getattr(rb, k)), k
    for k in _FIELDS + _REF_FIELDS:   # what an estimator with refine= alone gives
        assert torch.equal(getattr(rb, k), getattr(pr, k)), k
    for k in _VER_FIELDS:             # and the first verification is the one above
        assert torch.equal(getattr(rb, k), getattr(res, k)), k
    d2 = ver(depth, bx, slots, rb.quat_ref.float(), rb.trans_ref, frame_of=fo_d)
    for k in _VER_FIELDS:
        want = getattr(d2, k).bool() if k == "verified" else getattr(d2, k)
        assert torch.equal(want, getattr(rb, k + "_ref")), k
    want_best = rb.refined & rb.verified_ref & (rb.fit_ref >= rb.fit)
    assert rb.best.dtype == torch.uint8 and torch.equal(rb.best.bool(), want_best)
    print("with refine: fit", rb.fit.tolist(), "fit_ref", rb.fit_ref.tolist(), "best", rb.best.tolist())
    assert rb.best[2] == 0 and not rb.verified_ref[2]
    assert rb.refined[0] and rb.fit_ref[0] > rb.fit[0] and rb.best[0] == 1   # scene 100's own pose, refined
    # verify= without depth raises; N = 0 gives an empty result of the same class
    for e_ in (est, both):
        with pytest.raises(Pose6dError, match="depth"):
            e_(rgb, None, boxes, classes, fo)
    r0 = both(rgb, depth, [], [])
    assert type(r0) is type(rb) and r0.fit.shape == (0,) and r0.counts_ref.shape == (0, 5) and r0.best.shape == (0,)
    est.check()
