"""Writes tests/golden/infer.npz: recorded results of the reference's OWN
utils/visualization.py project_points and utils/mesh_utils.py load_mesh_corners, for
tests/test_infer_ref.py (CPU) and tests/test_infer.py (GPU).  Runs on the CPU; never run
by a test.  The reference checkout is found through POSE6D_REFERENCE, as gen_goldens.py
finds it.

Both reference modules import with an empty stand-in `cv2` module in sys.modules:
project_points and load_mesh_corners use only numpy and scipy (recorded with scipy 1.15.3,
numpy 2.2.6).

(a) project_points: 64 seeded poses -- float32 quaternions from a normal draw,
    translations with x, y in +-0.2 m and z in 0.3-1.5 m -- times the 8 corners of a seeded
    box, and the four axis points (origin, 0.1 m along x, y, z) through the same function
    as draw_axes does.  The LAST pose's translation z is replaced by a few centimetres so
    that some of its corners lie behind the camera (the z clip at 0.001).  The float values before
    astype(int) are recomputed with the same numpy expressions and stored too; every one
    of them must be at least 1e-6 from an integer (asserted), so a kernel within the
    tests' rounding bound truncates to the same integer, and every camera-space z at least
    0.01 from the clip's kink.
(b) load_mesh_corners: a synthetic ASCII ply (300 vertices in mm, 40 of them beyond
    0.3 m) and an all-outlier ply, written to a temporary directory; the vertices and the
    returned corners are recorded.
The fixture holds arrays only.
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.environ.get("POSE6D_REFERENCE", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden", "infer.npz")

K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])


def _load(modname, relpath):
    spec = importlib.util.spec_from_file_location(modname, os.path.join(REF, relpath))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    sys.path.insert(0, REPO)
    from tests.infer_ref import write_ply
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    viz = _load("ref_visualization", "utils/visualization.py")
    mesh = _load("ref_mesh_utils", "utils/mesh_utils.py")
    from scipy.spatial.transform import Rotation

    rng = np.random.default_rng(20240611)
    n = 64
    quat = rng.normal(size=(n, 4)).astype(np.float32)
    trans = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), rng.uniform(0.3, 1.5, n)], 1)
    trans = trans.astype(np.float32)
    lo = -rng.uniform(0.03, 0.12, 3)
    hi = rng.uniform(0.03, 0.12, 3)
    corners = np.array([[lo[0], lo[1], lo[2]], [hi[0], lo[1], lo[2]], [hi[0], hi[1], lo[2]], [lo[0], hi[1], lo[2]],
                        [lo[0], lo[1], hi[2]], [hi[0], lo[1], hi[2]], [hi[0], hi[1], hi[2]], [lo[0], hi[1], hi[2]]])
    axes = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1]], dtype=np.float64)
    # the last pose close to the camera: the first z of a fixed list that puts a corner behind
    # it and no point within 0.01 of the clip's kink
    r_last = Rotation.from_quat(quat[-1]).as_matrix()
    for tz in np.arange(0.015, 0.08, 0.0025):
        zs = (np.concatenate([corners, axes]) @ r_last.T)[:, 2] + np.float32(tz)
        if np.all(np.abs(zs - 0.001) >= 0.011) and np.any(zs[:8] < 0):
            trans[-1, 2] = np.float32(tz)
            break
    else:
        raise SystemExit("no candidate z for the behind-the-camera pose")
    pix = np.zeros((n, 12, 2), np.int64)
    pts = np.zeros((n, 12, 2), np.float64)
    behind = 0
    for i in range(n):
        pix[i, :8] = viz.project_points(corners, quat[i], trans[i], K)
        for j in range(4):   # draw_axes: one project_points call per axis point
            pix[i, 8 + j] = viz.project_points(axes[j:j + 1], quat[i], trans[i], K)[0]
        # the same numpy expressions, without the final astype(int)
        r_mat = Rotation.from_quat(quat[i]).as_matrix()
        for sl, p3 in ((slice(0, 8), corners),) + tuple((slice(8 + j, 9 + j), axes[j:j + 1]) for j in range(4)):
            p_cam = (r_mat @ p3.T).T + trans[i]
            assert np.all(np.abs(p_cam[:, 2] - 0.001) >= 0.01), "a camera-space z too close to the clip's kink"
            behind += int(np.sum(p_cam[:, 2] < 0.001))
            z = np.clip(p_cam[:, 2], 0.001, None)
            f = np.zeros((p3.shape[0], 2))
            f[:, 0] = (p_cam[:, 0] * K[0, 0] / z) + K[0, 2]
            f[:, 1] = (p_cam[:, 1] * K[1, 1] / z) + K[1, 2]
            pts[i, sl] = f
    assert np.array_equal(pts.astype(int), pix), "the recomputed floats do not truncate to the reference's ints"
    dist = np.abs(pts - np.rint(pts)).min()
    assert dist >= 1e-6, f"a projected float is {dist:.3e} from an integer"
    assert behind > 0, "no corner behind the camera"
    print(f"project_points: {n} poses, closest distance to an integer {dist:.3e}, {behind} clipped points")

    vr = np.random.default_rng(7)
    verts = vr.normal(size=(300, 3)) * np.array([40.0, 60.0, 25.0])          # mm
    verts[:40] = vr.normal(size=(40, 3)) * 30.0 + np.array([400.0, -350.0, 320.0])   # beyond 0.3 m
    far = vr.normal(size=(20, 3)) * 10.0 + np.array([500.0, 500.0, 500.0])
    with tempfile.TemporaryDirectory() as d:
        write_ply(os.path.join(d, "obj_01.ply"), verts)
        write_ply(os.path.join(d, "obj_02.ply"), far)
        mesh_corners = mesh.load_mesh_corners(d, "01")
        assert mesh.load_mesh_corners(d, "02") is None and mesh.load_mesh_corners(d, "03") is None
    assert mesh_corners.shape == (8, 3)
    np.savez(OUT, quat=quat, trans=trans, corners=corners, axes=axes, K=K, pix=pix, pts=pts, mesh_verts_mm=verts,
             mesh_far_mm=far, mesh_corners=mesh_corners)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
