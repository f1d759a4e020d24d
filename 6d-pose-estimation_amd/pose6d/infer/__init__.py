"""Detection-to-pose inference: what the reference's scripts/inference/inference_*.py do
around the model, on the device.

The scripts take a frame and a detector's boxes and, per detection, (1) cut a square
crop x1.2 around the box, resize it to 224 and build the model inputs
(inference_rgbd_geometric.py:110-182), (2) run the model, (3) for the RGB and RGBD
models replace the predicted x, y by the box centre's ray at the predicted z
(inference_rgb.py:99-104, inference_rgbd.py:159-164) and (4) project the object's 3D box
and axes with the original intrinsics (utils/visualization.py:8-32,
utils/mesh_utils.py:7-53).  Here:

  CropDetections   (1) for all N detections of F frames in ONE launch
                   (pose6d_crop_detections);
  PoseEstimator    (1) -> eval forward of one of the four drop-in models -> (3) + (4) in
                   one fp64 launch (pose6d_pose_project), replayed from one hipGraph per
                   detection-count bucket;
  load_mesh_corners / DEFAULT_K   the host helpers the scripts import;
  DepthRefiner     (not in the reference) point-to-point ICP of the N poses against the
                   depth frame in ONE launch (pose6d_depth_refine); PoseEstimator(refine=)
                   appends it and a projection of the refined pose to the same graph;
  PoseVerifier     (not in the reference) render-and-compare of the N poses against the depth
                   frame in ONE launch (pose6d_pose_verify): a confidence per pose and, with
                   refine=, the choice between the network's pose and the refined one;
                   PoseEstimator(verify=) appends it to the same graph.

This is NOT CropRGBD on a detector box.  The scripts differ from the training dataset
(data/dataset_rgbd.py) in three ways, all kept:
  * depth is resized as float32 (no rounding to whole millimetres);
  * the crop centre and intrinsics run in Python double and round to float32 once
    (the dataset computes them in float32);
  * the script's cx_crop = (cx + pad_l - crop_x1) * scale subtracts the UNPADDED crop
    origin after adding the pad, pad_l * scale more than the dataset's (cx - crop_x1) *
    scale on a box that hangs over the left edge (likewise at the top).  The models were
    trained on the dataset's value: `dataset_intrinsics=True` feeds them that instead.

No detector is built (YOLO stays out of scope: DESIGN.md); boxes come from the caller.
"""
from .crop import DEFAULT_K, CropDetections, DetectionCrops, _host_boxes, _host_frame_of, _k_dev  # noqa: F401
from .depth_stages import DepthRefiner, PoseVerifier, RefineOutput, VerifyOutput  # noqa: F401
from .estimator import _KINDS, BUCKETS, PoseEstimator  # noqa: F401
from .mesh import load_mesh_corners, load_mesh_points, load_mesh_triangles  # noqa: F401
from .project import N_POINTS, PoseResult, RefinedPoseResult, pose_project  # noqa: F401
