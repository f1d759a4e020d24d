"""tools/infer_pose.py --verify end to end, in process, on a synthetic image, depth and mesh
tree: the JSON gains fit / agree / counts / resid_m / verified per detection and, with
--refine, their _ref forms and `best`, equal to what PoseEstimator(verify=PoseVerifier(
load_mesh_triangles(...))) gives; without the flag the JSON is what it was."""
import json

import numpy as np
import pytest
import torch

from tests import refine_ref as RR
from tests import verify_ref as VR

pytestmark = pytest.mark.gpu

OLD_KEYS = {"obj", "cls", "conf", "xyxy", "valid", "quat_xyzw", "trans_m", "box2d", "axes2d"}
REF_KEYS = {"quat_ref_xyzw", "trans_ref_m", "box2d_ref", "axes2d_ref", "n_corr", "rms_m", "refined"}
VER_KEYS = {"fit", "agree", "counts", "resid_m", "verified"}


def _write_ply(path, verts_mm, faces):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(verts_mm), len(faces)))
        for v in verts_mm:
            f.write("%r %r %r\n" % (float(v[0]), float(v[1]), float(v[2])))
        for t in faces:
            f.write("3 %d %d %d\n" % tuple(int(i) for i in t))


def test_verify_flag_adds_the_verification(tmp_path):
    from PIL import Image
    from models.pose_net_rgb import PoseNetRGB
    from pose6d.infer import (DepthRefiner, PoseEstimator, PoseVerifier, load_mesh_corners, load_mesh_points,
                              load_mesh_triangles)
    from tools import infer_pose
    torch.manual_seed(0)
    model = PoseNetRGB(pretrained=False).cuda().eval()
    s = RR.scene(100)
    with torch.no_grad():   # a pose worth verifying: scene 100's perturbed one
        model.rot_head[-1].weight.zero_()
        model.rot_head[-1].bias.copy_(torch.from_numpy(s["q0"].copy()))
        model.trans_head[-1].weight.zero_()
        model.trans_head[-1].bias.copy_(torch.from_numpy(s["t0"].astype(np.float32)))
    rng = np.random.default_rng(4)
    rgb = rng.integers(0, 256, (RR.H, RR.W, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "f.png")
    Image.fromarray(s["depth"]).save(tmp_path / "d.png")
    torch.save({"epoch": 1, "model_state_dict": model.state_dict()}, tmp_path / "w.pth")
    verts, faces = VR.box_mesh(8)
    _write_ply(tmp_path / "obj_01.ply", verts.astype(np.float64) * 1000.0, faces)
    dets = [{"xyxy": list(s["box"]), "cls": 0, "conf": 0.9}, {"xyxy": [10, 20, 90, 100], "cls": 1, "conf": 0.4}]
    (tmp_path / "dets.json").write_text(json.dumps(dets))
    base = ["--model", "RGB", "--weights", str(tmp_path / "w.pth"), "--image", str(tmp_path / "f.png"), "--depth",
            str(tmp_path / "d.png"), "--detections", str(tmp_path / "dets.json"), "--mesh-dir", str(tmp_path)]
    assert infer_pose.main(base + ["--out", str(tmp_path / "plain.json")]) == 0
    assert infer_pose.main(base + ["--out", str(tmp_path / "ver.json"), "--verify", "--verify-tau", "0.08"]) == 0
    assert infer_pose.main(base + ["--out", str(tmp_path / "both.json"), "--verify", "--refine", "--refine-iters", "3",
                                   "--refine-points", "700"]) == 0
    plain = json.loads((tmp_path / "plain.json").read_text())["poses"]
    ver = json.loads((tmp_path / "ver.json").read_text())["poses"]
    both = json.loads((tmp_path / "both.json").read_text())["poses"]
    assert all(set(p) == OLD_KEYS for p in plain)
    assert all(set(p) == OLD_KEYS | VER_KEYS for p in ver)
    assert all(set(p) == OLD_KEYS | REF_KEYS | VER_KEYS | {k + "_ref" for k in VER_KEYS} | {"best"} for p in both)
    for a, b, c in zip(plain, ver, both):   # the old keys keep their values
        assert all(a[k] == b[k] == c[k] for k in OLD_KEYS)
    # --verify without --depth is refused
    assert infer_pose.main(base[:6] + base[8:] + ["--verify"]) == 1
    tri = load_mesh_triangles(str(tmp_path), "01")
    assert np.array_equal(tri[1], faces) and np.abs(tri[0] - verts).max() < 1e-7
    corners = {"01": load_mesh_corners(str(tmp_path), "01")}
    est = PoseEstimator(model, corners, graph=False, verify=PoseVerifier({"01": tri[:2]}, {"01": tri[2]}, tau=0.08))
    want = est(rgb, s["depth"], [d["xyxy"] for d in dets], ["01", "02"]).cpu()
    for i, p in enumerate(ver):
        assert p["fit"] == float(want.fit[i]) and p["agree"] == float(want.agree[i])
        assert p["counts"] == want.counts[i].tolist() and p["resid_m"] == float(want.resid[i])
        assert p["verified"] == bool(want.verified[i])
    assert ver[0]["verified"] is True and ver[0]["counts"][2] > 0 and sum(ver[0]["counts"]) == 1024
    assert ver[1]["verified"] is False and ver[1]["valid"] is False and ver[1]["fit"] == 0.0
    pts, diam = load_mesh_points(str(tmp_path), "01", n_points=700)
    est = PoseEstimator(model, corners, graph=False, refine=DepthRefiner({"01": pts}, {"01": diam}, iters=3),
                        verify=PoseVerifier({"01": tri[:2]}, {"01": tri[2]}))
    want = est(rgb, s["depth"], [d["xyxy"] for d in dets], ["01", "02"]).cpu()
    for i, p in enumerate(both):
        assert p["fit"] == float(want.fit[i]) and p["fit_ref"] == float(want.fit_ref[i])
        assert p["agree_ref"] == float(want.agree_ref[i]) and p["counts_ref"] == want.counts_ref[i].tolist()
        assert p["resid_m_ref"] == float(want.resid_ref[i]) and p["verified_ref"] == bool(want.verified_ref[i])
        assert p["best"] == bool(want.best[i]) == (p["refined"] and p["verified_ref"] and p["fit_ref"] >= p["fit"])
    assert both[1]["best"] is False
