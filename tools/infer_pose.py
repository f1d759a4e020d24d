"""Detections -> 6D poses and projected 3D boxes for one image: the command line of the
reference's scripts/inference/inference_*.py without YOLO and without the drawing.

    python tools/infer_pose.py --model RGBD-Geometric --weights best_pose_model.pth \
        --image 0042.png [--depth 0042_depth.png] --detections dets.json \
        --mesh-dir .../Linemod_preprocessed/models [--out poses.json] [--dataset-intrinsics]

dets.json: a list of {"xyxy": [x1, y1, x2, y2], "cls": int, "conf": float} -- what the
scripts read off each YOLO box (box.xyxy[0], box.cls[0], box.conf[0]).  Classes map to
meshes as the scripts' CLASS_ID_TO_OBJ_NAME (an unknown class falls back to "01").  Images
are decoded with PIL as pose6d/linemod.py does (PNG is lossless: the bytes equal
cv2.imread's); a missing depth image gives zeros like the scripts.  The checkpoint is the
reference's torch.save dict, opened with weights_only=True.  Output: JSON, one entry per
detection with the quaternion (x, y, z, w), the translation the projection used, the 8
projected box corners, the 4 axis points (origin, x, y, z) and `valid` (false: no mesh).
--refine (needs --depth) refines every pose against the depth frame (pose6d.infer.DepthRefiner:
point-to-point ICP on --refine-points mesh points for --refine-iters iterations) and adds
per detection `quat_ref_xyzw`, `trans_ref_m`, `box2d_ref`, `axes2d_ref`, `n_corr`, `rms_m`
(first and last iteration) and `refined`; without the flag the output is unchanged.
--verify (needs --depth) renders every object's triangle mesh at its pose and compares it with
the depth frame (pose6d.infer.PoseVerifier, tolerance --verify-tau of the diameter) and adds
per detection `fit`, `agree`, `counts` (no hit, no depth, consistent, occluded, violated),
`resid_m` and `verified`; with --refine also their `_ref` forms for the refined pose and
`best` (true: use the refined pose).
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "6d-pose-estimation_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

# inference_rgbd_geometric.py:28-31
CLASS_ID_TO_OBJ_NAME = {0: "01", 1: "02", 2: "04", 3: "05", 4: "06", 5: "08", 6: "09", 7: "10", 8: "11", 9: "12",
                        10: "13", 11: "14", 12: "15"}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", required=True, choices=("RGB", "RGB-Geometric", "RGBD", "RGBD-Geometric"))
    ap.add_argument("--weights", required=True)
    ap.add_argument("--image", required=True)
    ap.add_argument("--depth", default=None)
    ap.add_argument("--detections", required=True)
    ap.add_argument("--mesh-dir", required=True)
    ap.add_argument("--out", default=None, help="JSON file (default: stdout)")
    ap.add_argument("--dataset-intrinsics", action="store_true",
                    help="feed the model the training dataset's crop intrinsics, not the scripts'")
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--refine", action="store_true", help="refine the poses against the depth frame (ICP)")
    ap.add_argument("--refine-iters", type=int, default=10)
    ap.add_argument("--refine-points", type=int, default=1500, help="mesh points per object")
    ap.add_argument("--verify", action="store_true", help="render-and-compare every pose against the depth frame")
    ap.add_argument("--verify-tau", type=float, default=0.1, help="depth tolerance, a fraction of the diameter")
    a = ap.parse_args(argv)
    from pose6d.infer import (DEFAULT_K, DepthRefiner, PoseEstimator, PoseVerifier, load_mesh_corners, load_mesh_points,
                              load_mesh_triangles)
    from pose6d.linemod import load_depth, load_rgb
    from tools.compare_models import load_model

    with open(a.detections) as f:
        dets = json.load(f)
    rgb = load_rgb(a.image)
    depth = load_depth(a.depth, rgb.shape[:2]) if a.depth else None
    if a.refine and depth is None:
        print("Error: --refine needs --depth", file=sys.stderr)
        return 1
    if a.verify and depth is None:
        print("Error: --verify needs --depth", file=sys.stderr)
        return 1
    if a.model in ("RGBD", "RGBD-Geometric") and depth is None:
        print("Warning: no depth image, using zeros", file=sys.stderr)
        depth = np.zeros(rgb.shape[:2], np.uint16)
    dev = torch.device("cuda", 0)
    model = load_model(a.model, a.weights, dev)
    if model is None:
        return 1
    if a.bf16:
        model.set_compute_dtype(torch.bfloat16)
    corners = {name: load_mesh_corners(a.mesh_dir, name) for name in sorted(set(CLASS_ID_TO_OBJ_NAME.values()))}
    names = [CLASS_ID_TO_OBJ_NAME.get(int(d["cls"]), "01") for d in dets]
    refine = None
    if a.refine:
        meshes = {name: load_mesh_points(a.mesh_dir, name, n_points=a.refine_points) for name in corners}
        meshes = {k: v for k, v in meshes.items() if v is not None}
        refine = DepthRefiner({k: v[0] for k, v in meshes.items()}, {k: v[1] for k, v in meshes.items()},
                              iters=a.refine_iters)
    verify = None
    if a.verify:
        tri = {name: load_mesh_triangles(a.mesh_dir, name) for name in corners}
        tri = {k: v for k, v in tri.items() if v is not None}
        verify = PoseVerifier({k: v[:2] for k, v in tri.items()}, {k: v[2] for k, v in tri.items()}, tau=a.verify_tau)
    est = PoseEstimator(model, corners, K=DEFAULT_K, max_detections=32, graph=False,
                        dataset_intrinsics=a.dataset_intrinsics, refine=refine, verify=verify)
    out = []
    for s in range(0, len(dets), 32):   # the scripts have no limit; the estimator takes 32 at a time
        part = dets[s:s + 32]
        res = est(rgb, depth, [d["xyxy"] for d in part], names[s:s + 32]).cpu()
        for i, d in enumerate(part):
            out.append({"obj": names[s + i], "cls": int(d["cls"]), "conf": float(d.get("conf", 0.0)),
                        "xyxy": [int(v) for v in d["xyxy"]], "valid": bool(res.valid[i]),
                        "quat_xyzw": res.quat[i].tolist(), "trans_m": res.trans_cam[i].tolist(),
                        "box2d": res.box2d[i].tolist(), "axes2d": res.axes2d[i].tolist()})
            if a.refine:
                out[-1].update({"quat_ref_xyzw": res.quat_ref[i].tolist(), "trans_ref_m": res.trans_ref[i].tolist(),
                                "box2d_ref": res.box2d_ref[i].tolist(), "axes2d_ref": res.axes2d_ref[i].tolist(),
                                "n_corr": int(res.n_corr[i]), "rms_m": res.rms[i].tolist(),
                                "refined": bool(res.refined[i])})
            if a.verify:
                for sfx in ("", "_ref") if a.refine else ("",):
                    get = lambda name: getattr(res, name + sfx)[i]
                    out[-1].update({"fit" + sfx: float(get("fit")), "agree" + sfx: float(get("agree")),
                                    "counts" + sfx: get("counts").tolist(), "resid_m" + sfx: float(get("resid")),
                                    "verified" + sfx: bool(get("verified"))})
                if a.refine:
                    out[-1]["best"] = bool(res.best[i])
    est.check()
    text = json.dumps({"image": a.image, "model": a.model, "poses": out}, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
