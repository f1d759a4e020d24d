"""The front end pose6d_depth_refine and pose6d_pose_verify share (csrc/pose_geom.h: the
detection header, the sample grid, the depth read), on the cases tests/test_refine.py and
tests/test_verify.py leave out, against the restatements tests/refine_ref.py and
tests/verify_ref.py exactly as those tests compare.

One small batch for both launches: two 48 x 64 frames with a K row each, G = 8, a 64-point
mesh and the 12-triangle box.  Detection 0 (frame 0): a box with negative x1, y1 and odd
width and height, where x1 + floor(r) and trunc(x1 + r) differ.  Detection 1 (frame 1, whose
K row differs from row 0): a quaternion that is not unit and has w < 0."""
import functools

import numpy as np
import pytest
import torch

from tests import refine_ref as RR
from tests import verify_ref as VR

pytestmark = pytest.mark.gpu

H, W, G = 48, 64, 8
KS = np.array([[[80.0, 0.0, 32.0], [0.0, 80.0, 24.0], [0.0, 0.0, 1.0]],
               [[70.0, 0.0, 30.0], [0.0, 75.0, 22.0], [0.0, 0.0, 1.0]]])
BOXES = [(-5, -3, 20, 18), (22, 14, 45, 34)]
T_GT = [(-0.15, -0.106, 0.5), (0.02, 0.01, 0.45)]
GATE, TRIM, TAU, MIN_POINTS, ITERS = 0.75, 0.25, 0.1, 6, 3


@functools.lru_cache(maxsize=None)
def _batch():
    rng = np.random.default_rng(3)
    mesh = RR.box_surface(64, rng).astype(np.float32)
    frames, quat, trans = [], [], []
    for f in range(2):
        q_gt = RR.normalise_quat(rng.normal(size=4))
        cam = RR.box_surface(20000, rng) @ RR.quat_to_mat(q_gt).T + np.array(T_GT[f])
        frames.append(RR.render_depth(cam, K=KS[f], h=H, w=W)[0])
        dq = RR.axis_angle_quat(rng.normal(size=3), np.deg2rad(4.0))
        quat.append(RR.normalise_quat(RR.quat_mul(dq, q_gt)).astype(np.float32))
        trans.append(np.array(T_GT[f]) + rng.normal(0.0, 0.004, 3))
    quat[1] = quat[1] * np.float32(-2.5 if quat[1][3] > 0 else 2.5)
    assert quat[1][3] < 0 and abs(np.linalg.norm(quat[1]) - 1) > 1
    return mesh, frames, np.stack(quat), np.stack(trans)


def _dev(a, dtype):
    return torch.from_numpy(np.array(a)).to(dtype).cuda()


def _args(frames, slots, quat, trans):
    return (_dev(np.stack(frames).astype(np.int32), torch.uint16), _dev(BOXES, torch.int32), _dev(slots, torch.int64),
            _dev(quat, torch.float32), _dev(trans, torch.float64))


def test_refine_and_verify_on_the_same_grid():
    from pose6d.infer import DepthRefiner, PoseVerifier
    mesh, frames, quat, trans = _batch()
    verts, faces = VR.box_mesh(1)
    (x1, y1, x2, y2), i = BOXES[0], np.arange(G)
    u, v = RR.sample_pixels(BOXES[0], G)
    assert (x2 - x1) % 2 == 1 and (y2 - y1) % 2 == 1 and (u < 0).any() and (v < 0).any()
    assert (np.trunc(x1 + (2 * i + 1) * (x2 - x1) / (2 * G)) != u[:G]).any()
    assert (np.trunc(y1 + (2 * i + 1) * (y2 - y1) / (2 * G)) != v[::G]).any()
    fo = _dev([0, 1], torch.int32)
    ref = DepthRefiner({"a": mesh}, {"a": RR.DIAMETER}, grid=G, iters=ITERS, gate=GATE, trim=TRIM,
                       min_points=MIN_POINTS)
    ver = PoseVerifier({"a": (verts, faces)}, {"a": RR.DIAMETER}, grid=G, tau=TAU)
    args = _args(frames, [0, 0], quat, trans)
    r = ref(*args, frame_of=fo, K=KS, trace=True)
    o = ver(*args, frame_of=fo, K=KS, maps=True)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in r._asdict().items()}
    o = {k: v.cpu().numpy() for k, v in o._asdict().items()}
    for n in range(2):
        # refine: the samples are the restatement's bit for bit, the first trace row is the
        # normalised input pose
        pts, kept = RR.samples(frames[n], KS[n], BOXES[n], G, trans[n], GATE, RR.DIAMETER)
        assert kept.sum() >= 2 * MIN_POINTS, (n, kept.sum())
        assert np.array_equal(np.isnan(r["samples"][n]), np.isnan(pts)), n
        assert np.array_equal(r["samples"][n][kept], pts[kept]), n
        assert np.array_equal(r["pose_trace"][n, 0, :4], RR.normalise_quat(quat[n]))
        assert np.array_equal(r["pose_trace"][n, 0, 4:], trans[n]) and r["pose_trace"][n, 0, 3] >= 0
        c = r["corr"][n, 0]
        assert (c[~kept] == -1).all() and (c[kept] >= -1).all() and r["refined"][n] == 1
        # verify: everything equals the restatement's (resid: a sum in another order)
        want = VR.verify(frames[n], KS[n], BOXES[n], verts, faces, RR.DIAMETER, quat[n], trans[n], G=G, tau=TAU)
        assert np.array_equal(o["zbuf"][n], want["zbuf"]) and np.array_equal(o["cls"][n], want["cls"]), n
        assert np.array_equal(o["counts"][n], want["counts"]), n
        assert o["fit"][n] == want["fit"] and o["agree"][n] == want["agree"] and o["verified"][n] == 1, n
        assert abs(o["resid"][n] - want["resid"]) <= G * G * 2.0 ** -52 * want["resid"], n
        # one grid: a sample refine kept is a pixel with depth, so verify classed it >= 2 where
        # the render hit it, and as consistent exactly when the two depths are within tau x diameter
        u, v = RR.sample_pixels(BOXES[n], G)
        hit = np.isfinite(o["zbuf"][n])
        both = kept & hit
        assert both.sum() >= MIN_POINTS and (o["cls"][n][both] >= 2).all(), n
        z_obs = frames[n][v[both], u[both]] * 0.001
        assert np.array_equal(r["samples"][n][both, 2], z_obs), n
        assert np.array_equal(o["cls"][n][both] == 2, np.abs(z_obs - o["zbuf"][n][both]) <= TAU * RR.DIAMETER), n
        off = (u < 0) | (v < 0) | (u >= W) | (v >= H)
        assert np.isnan(r["samples"][n][off]).all() and (o["cls"][n][off & hit] == 1).all(), n
    # detection 1 read K's row 1: with row 0 its samples would differ
    wrong, _ = RR.samples(frames[1], KS[0], BOXES[1], G, trans[1], GATE, RR.DIAMETER)
    assert not np.array_equal(np.nan_to_num(wrong), np.nan_to_num(r["samples"][1]))
