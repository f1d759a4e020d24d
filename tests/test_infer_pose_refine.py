"""tools/infer_pose.py --refine end to end, in process, on a synthetic image, depth and mesh
tree: the JSON gains the refined pose and n_corr / rms / refined per detection, equal to
what PoseEstimator(refine=DepthRefiner(load_mesh_points(...))) gives; without the flag the
JSON is what it was."""
import json

import numpy as np
import pytest
import torch

from tests import refine_ref as RR

pytestmark = pytest.mark.gpu

OLD_KEYS = {"obj", "cls", "conf", "xyxy", "valid", "quat_xyzw", "trans_m", "box2d", "axes2d"}
NEW_KEYS = {"quat_ref_xyzw", "trans_ref_m", "box2d_ref", "axes2d_ref", "n_corr", "rms_m", "refined"}


def test_refine_flag_adds_the_refined_pose(tmp_path):
    from PIL import Image
    from models.pose_net_rgb import PoseNetRGB
    from pose6d.infer import DepthRefiner, PoseEstimator, load_mesh_corners, load_mesh_points
    from tests.infer_ref import write_ply
    from tools import infer_pose
    torch.manual_seed(0)
    model = PoseNetRGB(pretrained=False).cuda().eval()
    s = RR.scene(100)
    rng = np.random.default_rng(4)
    rgb = rng.integers(0, 256, (RR.H, RR.W, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "f.png")
    Image.fromarray(s["depth"]).save(tmp_path / "d.png")
    torch.save({"epoch": 1, "model_state_dict": model.state_dict()}, tmp_path / "w.pth")
    write_ply(tmp_path / "obj_01.ply", RR.box_surface(2000, rng) * 1000.0)
    dets = [{"xyxy": list(s["box"]), "cls": 0, "conf": 0.9}, {"xyxy": [10, 20, 90, 100], "cls": 1, "conf": 0.4}]
    (tmp_path / "dets.json").write_text(json.dumps(dets))
    base = ["--model", "RGB", "--weights", str(tmp_path / "w.pth"), "--image", str(tmp_path / "f.png"), "--depth",
            str(tmp_path / "d.png"), "--detections", str(tmp_path / "dets.json"), "--mesh-dir", str(tmp_path)]
    assert infer_pose.main(base + ["--out", str(tmp_path / "plain.json")]) == 0
    assert infer_pose.main(base + ["--out", str(tmp_path / "ref.json"), "--refine", "--refine-iters", "3",
                                   "--refine-points", "700"]) == 0
    plain = json.loads((tmp_path / "plain.json").read_text())["poses"]
    ref = json.loads((tmp_path / "ref.json").read_text())["poses"]
    assert all(set(p) == OLD_KEYS for p in plain)
    assert all(set(p) == OLD_KEYS | NEW_KEYS for p in ref)
    for a, b in zip(plain, ref):   # the old keys keep their values
        assert all(a[k] == b[k] for k in OLD_KEYS)
    # --refine without --depth is refused
    assert infer_pose.main(base[:6] + base[8:] + ["--refine"]) == 1
    pts, diam = load_mesh_points(str(tmp_path), "01", n_points=700)
    est = PoseEstimator(model, {"01": load_mesh_corners(str(tmp_path), "01")}, graph=False,
                        refine=DepthRefiner({"01": pts}, {"01": diam}, iters=3))
    want = est(rgb, s["depth"], [d["xyxy"] for d in dets], ["01", "02"]).cpu()
    for i, p in enumerate(ref):
        assert p["quat_ref_xyzw"] == want.quat_ref[i].tolist() and p["trans_ref_m"] == want.trans_ref[i].tolist()
        assert p["box2d_ref"] == want.box2d_ref[i].tolist() and p["axes2d_ref"] == want.axes2d_ref[i].tolist()
        assert p["n_corr"] == int(want.n_corr[i]) and p["rms_m"] == want.rms[i].tolist()
        assert p["refined"] == bool(want.refined[i])
    assert ref[1]["refined"] is False and ref[1]["valid"] is False
