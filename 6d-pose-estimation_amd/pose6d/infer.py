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
import functools
import os
from collections import namedtuple

import numpy as np
import torch

from ._lib import Pose6dError, call, require_device, stream
from .data import IMAGENET_MEAN, IMAGENET_STD

# utils/camera.py:8-12 (float64)
DEFAULT_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], dtype=np.float64)

BUCKETS = (1, 2, 4, 8, 16, 32)
N_POINTS = 12   # 8 box corners, origin, x / y / z axis tips

# inputs of the four model kinds and whether the scripts correct the translation by the
# box centre (inference_rgb.py:99-104, inference_rgbd.py:159-164) -- the two geometric
# models compute a metric translation themselves
_KINDS = {
    "PoseNetRGB": (lambda c: (c.rgb,), True),
    "PoseNetRGBD": (lambda c: (c.rgb, c.depth), True),
    "PoseNetRGBGeometric": (lambda c: (c.rgb, c.center_img, c.K_img), False),
    "PoseNetRGBDGeometric": (lambda c: (c.rgb, c.depth, c.depth_raw, c.center_crop, c.K_crop), False),
}


def load_mesh_corners(mesh_dir, obj_id_str):
    """The 8 corners (metres) of an object's robust bounding box, as
    utils/mesh_utils.py:7-53: vertices of the ASCII `obj_<id>.ply` in mm -> m, those
    0.3 m or more from the origin dropped, the box spanned by the 1st and 99th
    percentile per axis; corner order (min, min, min), (max, min, min), (max, max, min),
    (min, max, min), then the same four at max z.  None for a missing mesh or one whose
    vertices are all outliers."""
    path = os.path.join(mesh_dir, f"obj_{obj_id_str}.ply")
    if not os.path.exists(path):
        return None
    rows, body = [], False
    with open(path, "r") as f:
        for line in f:
            if not body:
                body = "end_header" in line
                continue
            v = line.split()
            if len(v) >= 3:   # vertex lines (and, as in the reference, face lines: "3 i j k")
                rows.append((float(v[0]), float(v[1]), float(v[2])))
    verts = np.array(rows, dtype=np.float64).reshape(-1, 3) / 1000.0
    verts = verts[np.linalg.norm(verts, axis=1) < 0.3]
    if len(verts) == 0:
        return None
    lo = np.percentile(verts, 1, axis=0)
    hi = np.percentile(verts, 99, axis=0)
    sel = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))
    ends = (lo, hi)
    return np.array([[ends[s[a]][a] for a in range(3)] for s in sel])


def load_mesh_points(mesh_dir, obj_id_str, n_points=1500, seed=0):
    """(points (n, 3) float32 metres, diameter metres) of an object for DepthRefiner, from
    the `obj_<id>.ply` load_mesh_corners reads: the header's `element vertex` count of
    vertex lines (all lines of three or more numbers when the header gives none), mm -> m,
    a seeded subsample of n_points without replacement when the mesh has more.  The
    diameter is models_info.yml's (mm) when the file lists the object, else the exact
    largest pairwise distance of the subsample.  None for a missing or empty mesh."""
    path = os.path.join(mesh_dir, f"obj_{obj_id_str}.ply")
    if not os.path.exists(path):
        return None
    rows, body, count = [], False, None
    with open(path, "r") as f:
        for line in f:
            if not body:
                v = line.split()
                if len(v) == 3 and v[0] == "element" and v[1] == "vertex":
                    count = int(v[2])
                body = "end_header" in line
                continue
            if count is not None and len(rows) >= count:
                break
            v = line.split()
            if len(v) >= 3:
                rows.append((float(v[0]), float(v[1]), float(v[2])))
    verts = np.array(rows, dtype=np.float64).reshape(-1, 3) / 1000.0
    if len(verts) == 0:
        return None
    if len(verts) > n_points:
        verts = verts[np.random.default_rng(seed).choice(len(verts), int(n_points), replace=False)]
    pts = verts.astype(np.float32)
    diameter = _info_diameter(mesh_dir, obj_id_str)
    if diameter is None:
        diameter = _largest_distance(pts)
    return pts, diameter


def _info_diameter(mesh_dir, obj_id_str):
    """The object's diameter (m) from mesh_dir/models_info.yml (mm), None when the file or the
    entry is missing."""
    diameter = None
    info_path = os.path.join(mesh_dir, "models_info.yml")
    if os.path.exists(info_path):
        import yaml
        with open(info_path, "r") as f:
            info = yaml.safe_load(f) or {}
        for key, data in info.items():
            try:
                if int(key) == int(obj_id_str) and "diameter" in data:
                    diameter = float(data["diameter"]) / 1000.0
            except (TypeError, ValueError):
                pass
    return diameter


def _largest_distance(pts):
    """The exact largest pairwise distance of fp32 points, in double."""
    p = pts.astype(np.float64)
    return max(float(np.sqrt(((p[s:s + 256, None] - p[None]) ** 2).sum(-1).max())) for s in range(0, len(p), 256))


def load_mesh_triangles(mesh_dir, obj_id_str):
    """(verts (V, 3) float32 metres, faces (T, 3) int32, diameter metres) of an object for
    PoseVerifier, from the ASCII `obj_<id>.ply`: the header's `element vertex` count of vertex
    lines (mm -> m), then its `element face` count of face lines `k i0 i1 ... i(k-1)`; a
    polygon of more than three vertices is fanned from its first, (i0, ij, ij+1).  The
    diameter is load_mesh_points': models_info.yml's when the file lists the object, else the
    exact largest pairwise vertex distance.  None for a missing mesh or one without vertices
    or faces."""
    path = os.path.join(mesh_dir, f"obj_{obj_id_str}.ply")
    if not os.path.exists(path):
        return None
    counts, body, rows, tris = {"vertex": 0, "face": 0}, False, [], []
    n_face_lines = 0
    with open(path, "r") as f:
        for line in f:
            v = line.split()
            if not body:
                if len(v) == 3 and v[0] == "element" and v[1] in counts:
                    counts[v[1]] = int(v[2])
                body = "end_header" in line
                continue
            if not v:
                continue
            if len(rows) < counts["vertex"]:
                rows.append((float(v[0]), float(v[1]), float(v[2])))
            elif n_face_lines < counts["face"]:
                n_face_lines += 1
                k = int(v[0])
                idx = [int(x) for x in v[1:1 + k]]
                tris.extend((idx[0], idx[j], idx[j + 1]) for j in range(1, len(idx) - 1))
            else:
                break
    if not rows or not tris:
        return None
    verts = (np.array(rows, dtype=np.float64).reshape(-1, 3) / 1000.0).astype(np.float32)
    faces = np.array(tris, dtype=np.int32).reshape(-1, 3)
    diameter = _info_diameter(mesh_dir, obj_id_str)
    if diameter is None:
        diameter = _largest_distance(verts)
    return verts, faces, diameter


def _host_boxes(boxes):
    """Host boxes -> (N, 4) int64 numpy, floats truncated toward zero as the scripts'
    map(int, box.xyxy[0]); empty or inverted boxes are refused."""
    if isinstance(boxes, torch.Tensor):
        boxes = boxes.numpy()
    a = np.asarray(boxes)
    if a.size == 0:
        return np.zeros((0, 4), np.int64)
    if a.ndim != 2 or a.shape[1] != 4:
        raise Pose6dError(f"boxes must be (N, 4) (x1, y1, x2, y2), got {a.shape}")
    if not np.issubdtype(a.dtype, np.integer):
        if not np.all(np.isfinite(a)):
            raise Pose6dError("boxes must be finite")
        a = np.trunc(a.astype(np.float64))
    if np.any(np.abs(a) >= 2 ** 30):
        raise Pose6dError("box coordinates must be below 2^30")
    a = a.astype(np.int64)
    bad = np.nonzero((a[:, 2] <= a[:, 0]) | (a[:, 3] <= a[:, 1]))[0]
    if len(bad):
        raise Pose6dError(f"box {int(bad[0])} is empty or inverted (x2 <= x1 or y2 <= y1): {a[bad[0]].tolist()}")
    return a


def _host_frame_of(frame_of, N, F):
    a = np.asarray(frame_of.numpy() if isinstance(frame_of, torch.Tensor) else frame_of).astype(np.int64).reshape(-1)
    if a.shape[0] != N:
        raise Pose6dError(f"frame_of must have one entry per box ({N}), got {a.shape[0]}")
    bad = np.nonzero((a < 0) | (a >= F))[0]
    if len(bad):
        raise Pose6dError(f"frame_of[{int(bad[0])}] = {int(a[bad[0]])} is outside [0, {F})")
    return a


def _is_dev(t):
    return isinstance(t, torch.Tensor) and t.is_cuda


def _k_dev(K, dev):
    """K (3, 3) / (9,) or (F, 3, 3) / (F, 9) -> (float64 device tensor, K_per_frame)."""
    t = K.detach() if isinstance(K, torch.Tensor) else torch.from_numpy(np.asarray(K, dtype=np.float64))
    t = t.to(device=dev, dtype=torch.float64)
    if t.numel() == 9 and t.dim() <= 2:
        return t.reshape(9).contiguous(), 0
    if t.dim() >= 2 and t[0].numel() == 9:
        return t.reshape(t.shape[0], 9).contiguous(), 1
    raise Pose6dError(f"K must be (3, 3) or (F, 3, 3), got {tuple(t.shape)}")


DetectionCrops = namedtuple("DetectionCrops", "rgb depth depth_raw center_crop K_crop center_img K_img")


class CropDetections:
    """N detector boxes over F frames -> the model inputs, one pose6d_crop_detections launch.

    __call__(frames, depth, boxes, frame_of=None, K=DEFAULT_K, out=None)
      frames (F, H, W, 3) or (H, W, 3) uint8 device tensor (RGB; BGR with bgr=True);
      depth (F, H, W) / (H, W) uint16 mm (int16 / int32 are converted) or None (zeros);
      boxes (N, 4) (x1, y1, x2, y2): a host list / array / CPU tensor -- int, or float
      truncated toward zero as the scripts' map(int, box.xyxy[0]); empty or inverted
      boxes are refused -- or an int32 device tensor, used as it is and read at kernel
      time; frame_of: N frame indices (a host sequence is range-checked here; a device
      int32 tensor is checked by the kernel: see check()), None = all on frame 0;
      K: (3, 3) or (F, 3, 3), taken as float64.
    Returns DetectionCrops(rgb (N,3,S,S), depth (N,1,S,S), depth_raw (N,S,S),
    center_crop (N,2), K_crop (N,3,3), center_img (N,2), K_img (N,3,3)), fp32.
    dataset_intrinsics=False: K_crop is the script's (inference_rgbd_geometric.py:156-167);
    True: the dataset's (dataset_rgbd.py:159-169), which the models were trained on (the
    module docstring has the difference).
    """

    def __init__(self, img_size=224, normalize=True, bgr=False, dataset_intrinsics=False, mean=IMAGENET_MEAN,
                 std=IMAGENET_STD):
        self.img_size = int(img_size)
        self.normalize = normalize
        self.bgr = bgr
        self.dataset_intrinsics = bool(dataset_intrinsics)
        self._ms = torch.tensor(list(mean) + list(std), dtype=torch.float32)
        self._ms_dev = {}
        self._status = {}

    def _mean_std(self, dev):
        if not self.normalize:
            return None
        t = self._ms_dev.get(dev)
        if t is None:
            t = self._ms_dev[dev] = self._ms.to(dev)
        return t

    def _status_of(self, dev):
        t = self._status.get(dev)
        if t is None:
            t = self._status[dev] = torch.zeros(1, dtype=torch.int32, device=dev)
        return t

    def empty_outputs(self, N, dev):
        S = self.img_size
        e = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        return DetectionCrops(e(N, 3, S, S), e(N, 1, S, S), e(N, S, S), e(N, 2), e(N, 3, 3), e(N, 2), e(N, 3, 3))

    def __call__(self, frames, depth, boxes, frame_of=None, K=DEFAULT_K, out=None):
        require_device(frames, depth)
        if frames.dim() == 3:
            frames = frames[None]
            depth = depth[None] if depth is not None and depth.dim() == 2 else depth
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
            raise Pose6dError(f"CropDetections: frames must be (F, H, W, 3) uint8, got {tuple(frames.shape)} "
                              f"{frames.dtype}")
        F, H, W, _ = frames.shape
        dev = frames.device
        if depth is not None:
            if tuple(depth.shape) != (F, H, W):
                raise Pose6dError(f"CropDetections: depth must be (F, H, W) = {(F, H, W)}, got {tuple(depth.shape)}")
            if depth.dtype != torch.uint16:
                depth = depth.to(torch.int32).clamp_(0, 65535).to(torch.uint16)
            depth = depth.contiguous()
        if _is_dev(boxes):
            if boxes.dim() != 2 or boxes.shape[1] != 4:
                raise Pose6dError(f"CropDetections: boxes must be (N, 4), got {tuple(boxes.shape)}")
            bx = boxes.to(torch.int32).contiguous()   # a float tensor truncates toward zero
        else:
            bx = torch.from_numpy(_host_boxes(boxes).astype(np.int32)).to(dev)
        N = bx.shape[0]
        if frame_of is None:
            fo = None
        elif _is_dev(frame_of):
            fo = frame_of.to(torch.int32).contiguous()
            if fo.numel() != N:
                raise Pose6dError(f"CropDetections: frame_of must have one entry per box ({N}), got {fo.numel()}")
        else:
            fo = torch.from_numpy(_host_frame_of(frame_of, N, F).astype(np.int32)).to(dev)
        Kd, per_frame = K if isinstance(K, tuple) else _k_dev(K, dev)
        if per_frame and Kd.shape[0] != F:
            raise Pose6dError(f"CropDetections: per-frame K must have {F} rows, got {Kd.shape[0]}")
        if out is None:
            out = self.empty_outputs(N, dev)
        call("crop_detections", frames.contiguous(), int(self.bgr), depth, F, H, W, fo, bx, N, Kd, per_frame,
             self.img_size, self._mean_std(dev), int(self.dataset_intrinsics), *out, self._status_of(dev), stream())
        return out

    def check(self):
        """Read the status word of every launch since the last check and reset it; raise
        if a device-side frame_of entry was outside [0, F) (that detection's outputs are
        zeros).  One host sync."""
        for st in self._status.values():
            v = int(st.item())
            if v:
                st.zero_()
                raise Pose6dError(f"CropDetections.check: frame_of[{v - 1}] was outside the frames given (that "
                                  f"detection's outputs are zeros)")


def pose_project(quat, trans, K, obj, corners, boxes=None, frame_of=None, axis_scale=0.1, out=None):
    """pose6d_pose_project on device tensors: quat (N, 4) fp32 (x, y, z, w), trans (N, 3)
    fp32, K float64 (3, 3) / (F, 3, 3) (or _k_dev's pair), obj (N,) int64 rows of corners
    (n_obj, 8, 3) float64; boxes (N, 4) int32 (x1, y1, x2, y2) switches the bbox-centre
    translation correction on; frame_of (N,) int32 picks K's row.
    Returns (trans (N, 3) f64, points (N, 12, 2) f64, pixels (N, 12, 2) i64, valid (N,) u8)."""
    require_device(quat, trans, obj, corners, boxes, frame_of)
    dev = quat.device
    N = quat.shape[0]
    Kd, per_frame = K if isinstance(K, tuple) else _k_dev(K, dev)
    F = Kd.shape[0] if per_frame else 1
    q = quat.detach().to(torch.float32).contiguous()
    t = trans.detach().to(torch.float32).contiguous()
    if q.shape != (N, 4) or t.shape != (N, 3) or obj.numel() != N:
        raise Pose6dError("pose_project: quat (N, 4), trans (N, 3) and obj (N,) must agree")
    c = corners.to(torch.float64).contiguous()
    if c.dim() != 3 or c.shape[1:] != (8, 3):
        raise Pose6dError(f"pose_project: corners must be (n_obj, 8, 3), got {tuple(c.shape)}")
    bx = boxes.to(torch.int32).contiguous() if boxes is not None else None
    fo = frame_of.to(torch.int32).contiguous() if frame_of is not None else None
    if out is None:
        out = (torch.empty(N, 3, device=dev, dtype=torch.float64),
               torch.empty(N, N_POINTS, 2, device=dev, dtype=torch.float64),
               torch.empty(N, N_POINTS, 2, device=dev, dtype=torch.int64),
               torch.empty(N, device=dev, dtype=torch.uint8))
    call("pose_project", q, t, bx, Kd, per_frame, fo, F, obj.to(torch.int64).contiguous(), c, c.shape[0],
         float(axis_scale), N, *out, stream())
    return out


class PoseResult:
    """Poses of N detections.  quat (N, 4) / trans (N, 3): the model's fp32 outputs;
    trans_cam (N, 3) f64: the translation the projection used (bbox-centre corrected for the
    RGB and RGBD models, else trans); points (N, 12, 2) f64 and their truncation pixels
    (N, 12, 2) i64 -- box2d = pixels[:, :8] (project_points of the 8 corners), axes2d =
    pixels[:, 8:] (origin, x, y, z tips: draw_axes); valid (N,) bool: False (rows zero)
    for a class without a mesh or a zero quaternion.
    From a PoseEstimator these are views of its output buffer, valid until its next call:
    .cpu() (one device-to-host copy) or .clone() keeps them."""

    _FIELDS = (("quat", torch.float32, (4,)), ("trans", torch.float32, (3,)), ("trans_cam", torch.float64, (3,)),
               ("points", torch.float64, (N_POINTS, 2)), ("pixels", torch.int64, (N_POINTS, 2)),
               ("valid", torch.uint8, ()))

    def __init__(self, buf, bucket, n):
        self._buf, self._bucket, self.n = buf, bucket, n
        off = 0
        for name, dt, shape in self._FIELDS:
            cnt = bucket * int(np.prod(shape, dtype=np.int64))
            nbytes = cnt * torch.empty((), dtype=dt).element_size()
            setattr(self, "_" + name, buf[off:off + nbytes].view(dt).view(bucket, *shape))
            off += (nbytes + 7) // 8 * 8

    @classmethod
    def nbytes(cls, bucket):
        off = 0
        for _, dt, shape in cls._FIELDS:
            off += (bucket * int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dt).element_size() + 7) // 8 * 8
        return off

    quat = property(lambda s: s._quat[:s.n])
    trans = property(lambda s: s._trans[:s.n])
    trans_cam = property(lambda s: s._trans_cam[:s.n])
    points = property(lambda s: s._points[:s.n])
    pixels = property(lambda s: s._pixels[:s.n])
    box2d = property(lambda s: s._pixels[:s.n, :8])
    axes2d = property(lambda s: s._pixels[:s.n, 8:])
    valid = property(lambda s: s._valid[:s.n].bool())

    def cpu(self):
        return type(self)(self._buf.cpu(), self._bucket, self.n)

    def clone(self):
        return type(self)(self._buf.clone(), self._bucket, self.n)


RefineOutput = namedtuple("RefineOutput", "quat trans quat32 trans32 n_corr rms refined pose_trace corr samples")


class DepthRefiner:
    """Point-to-point ICP of estimated poses against the depth frame, one
    pose6d_depth_refine launch for N detections (DESIGN.md "Depth refinement").

    points: {key: (n, 3) metres}, diameters: {key: metres} (load_mesh_points' results), the
    keys those of the estimator's `corners` dict.  grid: samples per box side (G, P = G * G
    per box, 1..32); iters: fixed iteration count (1..64); gate / trim: fractions of the
    object's diameter -- samples farther than gate * diameter from the initial translation
    are background, pairs farther apart than trim * diameter are dropped; min_points: the
    fewest accepted pairs an update needs (>= 3).  The mesh table is packed in
    models.add_loss._MeshTable's layout, once per device.

    __call__(depth, boxes, obj, quat, trans, frame_of=None, K=DEFAULT_K, trace=False, out=None),
    all device tensors: depth (F, H, W) / (H, W) uint16; boxes (N, 4) int32; obj (N,) int64
    slots (slots(keys) maps keys, -1 = no mesh); quat (N, 4) fp32 (x, y, z, w); trans (N, 3)
    float64; frame_of (N,) int32 or None; K (3, 3) / (F, 3, 3) or _k_dev's pair.  Returns a
    RefineOutput: quat (N, 4) / trans (N, 3) f64, their fp32 casts quat32 / trans32, n_corr
    (N,) i32, rms (N, 2) f64, refined (N,) u8 and, with trace=True, pose_trace (N, iters + 1,
    7) f64, corr (N, iters, P) i32 and samples (N, P, 3) f64 (None otherwise).  out: the
    seven result tensors to write into (a captured graph's static buffers)."""

    def __init__(self, points, diameters, grid=32, iters=10, gate=0.75, trim=0.25, min_points=16, depth_scale=0.001):
        keys = [k for k, v in points.items() if v is not None]
        self._slot = {k: i for i, k in enumerate(keys)}
        self._points = [np.array(points[k], np.float32).reshape(-1, 3) for k in keys]   # (copies)
        missing = [k for k in keys if k not in diameters]
        if missing:
            raise Pose6dError(f"DepthRefiner: no diameter for {missing}")
        self._diam = [float(diameters[k]) for k in keys]
        self.grid, self.iters, self.min_points = int(grid), int(iters), int(min_points)
        self.gate, self.trim, self.depth_scale = float(gate), float(trim), float(depth_scale)
        self._tables = {}

    def slots(self, keys):
        """Mesh-table slots (int64 array) of a sequence of keys; -1 for a key without a mesh."""
        return np.array([self._slot.get(k, -1) for k in keys], np.int64)

    def table(self, dev):
        T = self._tables.get(dev)
        if T is None:
            from models.add_loss import _MeshTable
            pts = {i: torch.from_numpy(p) for i, p in enumerate(self._points)}
            T = self._tables[dev] = _MeshTable(pts, dict(enumerate(self._diam)), dev)
        return T

    def empty_outputs(self, N, dev):
        e = lambda dt, *s: torch.empty(*s, device=dev, dtype=dt)
        return (e(torch.float64, N, 4), e(torch.float64, N, 3), e(torch.float32, N, 4), e(torch.float32, N, 3),
                e(torch.int32, N), e(torch.float64, N, 2), e(torch.uint8, N))

    def __call__(self, depth, boxes, obj, quat, trans, frame_of=None, K=DEFAULT_K, trace=False, out=None):
        require_device(depth, boxes, obj, quat, trans, frame_of)
        dev = quat.device
        if depth.dim() == 2:
            depth = depth[None]
        if depth.dtype != torch.uint16 or depth.dim() != 3:
            raise Pose6dError(f"DepthRefiner: depth must be (F, H, W) uint16, got {tuple(depth.shape)} {depth.dtype}")
        F, H, W = depth.shape
        N = quat.shape[0]
        q = quat.detach().to(torch.float32).contiguous()
        t = trans.detach().to(torch.float64).contiguous()
        if q.shape != (N, 4) or t.shape != (N, 3) or obj.numel() != N or tuple(boxes.shape) != (N, 4):
            raise Pose6dError("DepthRefiner: boxes (N, 4), obj (N,), quat (N, 4) and trans (N, 3) must agree")
        fo = frame_of.to(torch.int32).contiguous() if frame_of is not None else None
        if fo is not None and fo.numel() != N:
            raise Pose6dError(f"DepthRefiner: frame_of must have one entry per box ({N}), got {fo.numel()}")
        Kd, per_frame = K if isinstance(K, tuple) else _k_dev(K, dev)
        if per_frame and Kd.shape[0] < F:
            raise Pose6dError(f"DepthRefiner: per-frame K must have {F} rows, got {Kd.shape[0]}")
        T = self.table(dev)
        if out is None:
            out = self.empty_outputs(N, dev)
        P = self.grid * self.grid
        dbg = (None, None, None)
        if trace:
            dbg = (torch.empty(N, self.iters + 1, 7, device=dev, dtype=torch.float64),
                   torch.empty(N, self.iters, P, device=dev, dtype=torch.int32),
                   torch.empty(N, P, 3, device=dev, dtype=torch.float64))
        call("depth_refine", depth.contiguous(), F, H, W, self.depth_scale, Kd, per_frame,
             boxes.to(torch.int32).contiguous(), fo, obj.to(torch.int64).contiguous(), T.points, T.off, T.npts, T.diam,
             T.n_slots, q, t, N, self.grid, self.iters, self.gate, self.trim, self.min_points, *out, *dbg, stream())
        return RefineOutput(*out, *dbg)


class RefinedPoseResult(PoseResult):
    """A PoseResult plus the depth-refined pose (PoseEstimator(refine=...)): quat_ref (N, 4)
    f64 (x, y, z, w; unit, w >= 0) and trans_ref (N, 3) f64; points_ref / pixels_ref (and
    box2d_ref, axes2d_ref): the projection of the refined pose; n_corr (N,) i32 accepted
    pairs of the last iteration, rms (N, 2) f64 their root-mean-square distance in the first
    and the last iteration (m), refined (N,) bool: False where the refinement had nothing to
    work with (no mesh, zero depth in the box, too few pairs) -- quat_ref / trans_ref are
    then the network's pose.  A buffer layout of its own: PoseResult's fields first."""

    _FIELDS = PoseResult._FIELDS + (
        ("quat_ref", torch.float64, (4,)), ("trans_ref", torch.float64, (3,)),
        ("points_ref", torch.float64, (N_POINTS, 2)), ("pixels_ref", torch.int64, (N_POINTS, 2)),
        ("n_corr", torch.int32, ()), ("rms", torch.float64, (2,)), ("refined", torch.uint8, ()),
        ("quat32_ref", torch.float32, (4,)), ("trans32_ref", torch.float32, (3,)))   # what the projection read

    quat_ref = property(lambda s: s._quat_ref[:s.n])
    trans_ref = property(lambda s: s._trans_ref[:s.n])
    points_ref = property(lambda s: s._points_ref[:s.n])
    pixels_ref = property(lambda s: s._pixels_ref[:s.n])
    box2d_ref = property(lambda s: s._pixels_ref[:s.n, :8])
    axes2d_ref = property(lambda s: s._pixels_ref[:s.n, 8:])
    n_corr = property(lambda s: s._n_corr[:s.n])
    rms = property(lambda s: s._rms[:s.n])
    refined = property(lambda s: s._refined[:s.n].bool())


VerifyOutput = namedtuple("VerifyOutput", "counts fit agree resid verified zbuf cls")


class PoseVerifier:
    """Render-and-compare verification of estimated poses against the depth frame, one
    pose6d_pose_verify launch for N detections (DESIGN.md "Pose verification").

    meshes: {key: (verts (V, 3) metres, faces (T, 3))}, diameters: {key: metres}
    (load_mesh_triangles' results), the keys those of the estimator's `corners` dict; a face
    index outside its mesh's vertices is refused here.  grid: samples per box side (G, P = G * G
    per box, 1..64); tau: the tolerance as a fraction of the object's diameter.  The triangle
    table is packed once per device.

    __call__(depth, boxes, obj, quat, trans, frame_of=None, K=DEFAULT_K, maps=False, out=None),
    all device tensors, as DepthRefiner takes them (obj: slots(keys), -1 = no mesh).  Returns a
    VerifyOutput: counts (N, 5) i32 (no hit, hit without depth, consistent, occluded, violated),
    fit (N,) f64 = consistent / (consistent + occluded + violated), agree (N,) f64 = consistent
    / (consistent + violated), resid (N,) f64 mean |z_obs - z| of the consistent samples (m),
    verified (N,) u8 and, with maps=True, zbuf (N, P) f64 (+inf: no hit) and cls (N, P) u8 (None
    otherwise).  out: the five result tensors to write into (a captured graph's static
    buffers).  choose=(base_fit (N,) f64, base_flag (N,) u8, best (N,) u8): the same launch
    also writes best = base_flag & verified & (fit >= base_fit)."""

    def __init__(self, meshes, diameters, grid=32, tau=0.1, depth_scale=0.001):
        keys = [k for k, v in meshes.items() if v is not None]
        missing = [k for k in keys if k not in diameters]
        if missing:
            raise Pose6dError(f"PoseVerifier: no diameter for {missing}")
        self._slot = {k: i for i, k in enumerate(keys)}
        self._verts = [np.array(meshes[k][0], np.float32).reshape(-1, 3) for k in keys]   # (copies)
        self._faces = [np.array(meshes[k][1], np.int64).reshape(-1, 3) for k in keys]
        for k, v, f in zip(keys, self._verts, self._faces):
            if f.size and (f.min() < 0 or f.max() >= len(v)):
                raise Pose6dError(f"PoseVerifier: mesh {k!r} has a face index outside [0, {len(v)})")
        self._diam = [float(diameters[k]) for k in keys]
        self.grid, self.tau, self.depth_scale = int(grid), float(tau), float(depth_scale)
        self._tables = {}

    def slots(self, keys):
        """Triangle-table slots (int64 array) of a sequence of keys; -1 for a key without a mesh."""
        return np.array([self._slot.get(k, -1) for k in keys], np.int64)

    def table(self, dev):
        """(verts, faces, voff, nverts, toff, ntri, diam, n_slots) on dev."""
        T = self._tables.get(dev)
        if T is None:
            nv = np.array([len(v) for v in self._verts], np.int64)
            nt = np.array([len(f) for f in self._faces], np.int64)
            i32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.int32)).to(dev)
            cat = lambda parts, dt, w: np.concatenate(parts).astype(dt) if parts else np.zeros((0, w), dt)
            T = self._tables[dev] = (
                torch.from_numpy(cat(self._verts, np.float32, 3)).to(dev),
                torch.from_numpy(cat(self._faces, np.int32, 3)).to(dev),
                i32(np.cumsum(nv) - nv), i32(nv), i32(np.cumsum(nt) - nt), i32(nt),
                torch.tensor(self._diam, dtype=torch.float64, device=dev), len(nv))
        return T

    def empty_outputs(self, N, dev):
        e = lambda dt, *s: torch.empty(*s, device=dev, dtype=dt)
        return (e(torch.int32, N, 5), e(torch.float64, N), e(torch.float64, N), e(torch.float64, N),
                e(torch.uint8, N))

    def __call__(self, depth, boxes, obj, quat, trans, frame_of=None, K=DEFAULT_K, maps=False, out=None, choose=None):
        require_device(depth, boxes, obj, quat, trans, frame_of)
        dev = quat.device
        if depth.dim() == 2:
            depth = depth[None]
        if depth.dtype != torch.uint16 or depth.dim() != 3:
            raise Pose6dError(f"PoseVerifier: depth must be (F, H, W) uint16, got {tuple(depth.shape)} {depth.dtype}")
        F, H, W = depth.shape
        N = quat.shape[0]
        q = quat.detach().to(torch.float32).contiguous()
        t = trans.detach().to(torch.float64).contiguous()
        if q.shape != (N, 4) or t.shape != (N, 3) or obj.numel() != N or tuple(boxes.shape) != (N, 4):
            raise Pose6dError("PoseVerifier: boxes (N, 4), obj (N,), quat (N, 4) and trans (N, 3) must agree")
        fo = frame_of.to(torch.int32).contiguous() if frame_of is not None else None
        if fo is not None and fo.numel() != N:
            raise Pose6dError(f"PoseVerifier: frame_of must have one entry per box ({N}), got {fo.numel()}")
        Kd, per_frame = K if isinstance(K, tuple) else _k_dev(K, dev)
        if per_frame and Kd.shape[0] < F:
            raise Pose6dError(f"PoseVerifier: per-frame K must have {F} rows, got {Kd.shape[0]}")
        if out is None:
            out = self.empty_outputs(N, dev)
        P = self.grid * self.grid
        dbg = (None, None)
        if maps:
            dbg = (torch.empty(N, P, device=dev, dtype=torch.float64),
                   torch.empty(N, P, device=dev, dtype=torch.uint8))
        if choose is not None and not (choose[0].dtype == torch.float64 and choose[1].dtype == torch.uint8
                                       and choose[2].dtype == torch.uint8
                                       and all(c.numel() == N and c.is_contiguous() for c in choose)):
            raise Pose6dError("PoseVerifier: choose must be (base_fit f64, base_flag u8, best u8), N entries each")
        call("pose_verify", depth.contiguous(), F, H, W, self.depth_scale, Kd, per_frame,
             boxes.to(torch.int32).contiguous(), fo, obj.to(torch.int64).contiguous(), *self.table(dev), q, t, N,
             self.grid, self.tau, *out, *dbg, *(choose or (None, None, None)), stream())
        return VerifyOutput(*out, *dbg)


_VERIFY_FIELDS = (("fit", torch.float64, ()), ("agree", torch.float64, ()), ("counts", torch.int32, (5,)),
                  ("resid", torch.float64, ()), ("verified", torch.uint8, ()))


@functools.lru_cache(maxsize=None)
def _result_type(refined, verified):
    """The result class of a PoseEstimator from its options: PoseResult, RefinedPoseResult, or
    one of them extended by the verification's fields (PoseEstimator(verify=...)) -- fit, agree
    (N,) f64, counts (N, 5) i32, resid (N,) f64, verified (N,) bool of the network's pose and,
    with refine=, fit_ref ... verified_ref of the refined pose and best (N,) uint8: 1 where
    refined, verified_ref and fit_ref >= fit all hold (use the refined pose).  The earlier
    fields keep their places in the buffer."""
    base = RefinedPoseResult if refined else PoseResult
    if not verified:
        return base
    fields = _VERIFY_FIELDS
    if refined:
        fields = fields + tuple((n + "_ref", dt, sh) for n, dt, sh in _VERIFY_FIELDS) + (("best", torch.uint8, ()),)
    ns = {"_FIELDS": base._FIELDS + fields, "__doc__": base.__doc__ + "\n\n" + _result_type.__doc__}
    for name, _, _ in fields:
        view = (lambda s, a="_" + name: getattr(s, a)[:s.n])
        ns[name] = property((lambda s, v=view: v(s).bool()) if name.startswith("verified") else view)
    return type("Verified" + base.__name__, (base,), ns)


class _Bucket:
    """The static buffers and (graph=True) the captured graph of one (detections bucket,
    depth present) pair."""

    def __init__(self, B, dev, cropper, result=PoseResult, refine=False, verify=False):
        self.B = B
        self.boxes = torch.zeros(B, 4, dtype=torch.int32, device=dev)
        self.frame_of = torch.zeros(B, dtype=torch.int32, device=dev)
        self.obj = torch.zeros(B, dtype=torch.int64, device=dev)
        if refine:   # the refiner's mesh-table slots
            self.obj_ref = torch.zeros(B, dtype=torch.int64, device=dev)
        if verify:   # the verifier's triangle-table slots
            self.obj_ver = torch.zeros(B, dtype=torch.int64, device=dev)
        self.crops = cropper.empty_outputs(B, dev)
        self.out = torch.zeros(result.nbytes(B), dtype=torch.uint8, device=dev)
        self.res = result(self.out, B, B)
        self.engines = {}    # this bucket's own engines: their buffers are sized by the batch
        self.graph = None


class PoseEstimator:
    """Frame(s) + detector boxes -> poses and projected 3D boxes, on the device.

    model: one of the four drop-in modules (PoseNetRGB, PoseNetRGBD, PoseNetRGBGeometric,
    PoseNetRGBDGeometric) in eval mode, on the device.  Its kind decides the inputs the
    forward gets and whether the bbox-centre translation correction applies, as the four
    inference scripts do.  corners: (n_obj, 8, 3) array, or a dict {key: (8, 3) or None}
    (load_mesh_corners' results; a None is an object without a mesh).  class_to_obj: dict
    detector class -> corners key / row (None: the class is the key); a class without
    corners gives valid = False.  K: (3, 3) float64 for every frame, or (max_frames, 3, 3).

    __call__(rgb, depth, boxes, classes, frame_of=None): rgb (H, W, 3) or (F, H, W, 3)
    uint8 (host array or device tensor), F <= max_frames; depth (H, W) / (F, H, W) uint16
    or None; boxes / classes / frame_of: N host entries (boxes as CropDetections takes
    them).  Returns a PoseResult.  The N detections are padded to the next of 1, 2, 4, 8,
    16, 32 by repeating detection 0, with and without a graph (so both run the same
    launches and agree bit for bit); N = 0 returns empty tensors without a launch, N >
    max_detections raises.
    graph=True: frames, boxes and indices are copied into static buffers and ONE hipGraph
    per (bucket, depth present) replays crop -> eval forward -> projection.  Each bucket
    owns its engines (activation buffers and packed weights are sized per batch), so a
    graph's pointers stay valid while other buckets run.
    Weights: packed copies are synchronised on construction and on refresh(); call
    refresh() after writing the model's weights (a replay runs no Python that could notice).
    The model stays usable on its own: the estimator swaps a bucket's engines in around
    each of its calls and restores the model's own afterwards.
    refine: a DepthRefiner (keyed like `corners`) or None.  With one, the body becomes crop
    -> forward -> projection -> refinement of (quat, trans_cam) against the depth frame ->
    projection of the refined pose, all in the same graph, and the result is a
    RefinedPoseResult; a call without depth raises.  None: nothing changes.
    verify: a PoseVerifier (keyed like `corners`) or None.  With one, a render-and-compare
    launch on (quat, trans_cam) joins the graph and the result gains fit, agree, counts, resid
    and verified; with refine= as well, a second launch on the refined pose adds fit_ref ...
    verified_ref and best (1: use the refined pose); the result's class is _result_type's.  A
    call without depth raises.  None: nothing is allocated or launched differently.
    """

    def __init__(self, model, corners, K=DEFAULT_K, class_to_obj=None, max_detections=32, max_frames=1, graph=True,
                 dataset_intrinsics=False, img_size=224, bgr=False, axis_scale=0.1, refine=None, verify=None):
        kind = type(model).__name__
        if kind not in _KINDS:
            raise Pose6dError(f"PoseEstimator: model must be one of {sorted(_KINDS)}, got {kind}")
        if model.training:
            raise Pose6dError("PoseEstimator: the model is in training mode; call model.eval() first "
                              "(inference uses the BatchNorm running statistics and no dropout)")
        p = next(model.parameters())
        if not p.is_cuda:
            raise Pose6dError("PoseEstimator: the model must be on the ROCm device")
        if not 1 <= int(max_detections) <= BUCKETS[-1]:
            raise Pose6dError(f"PoseEstimator: max_detections must be in [1, {BUCKETS[-1]}]")
        self.model, self.kind = model, kind
        self._inputs, self.corrects_translation = _KINDS[kind]
        self.device = p.device
        self.max_detections, self.max_frames = int(max_detections), int(max_frames)
        self.graph = bool(graph)
        self.axis_scale = float(axis_scale)
        if refine is not None and not isinstance(refine, DepthRefiner):
            raise Pose6dError("PoseEstimator: refine must be a DepthRefiner or None")
        if verify is not None and not isinstance(verify, PoseVerifier):
            raise Pose6dError("PoseEstimator: verify must be a PoseVerifier or None")
        self.refine, self.verify = refine, verify
        self._result = _result_type(refine is not None, verify is not None)
        self.cropper = CropDetections(img_size, True, bgr, dataset_intrinsics)
        if isinstance(corners, dict):
            keys = [k for k, v in corners.items() if v is not None]
            tab = np.stack([np.asarray(corners[k], np.float64).reshape(8, 3) for k in keys]) if keys else \
                np.zeros((0, 8, 3))
            self._row = {k: i for i, k in enumerate(keys)}
        else:
            tab = np.asarray(corners, np.float64)
            if tab.ndim != 3 or tab.shape[1:] != (8, 3):
                raise Pose6dError(f"PoseEstimator: corners must be (n_obj, 8, 3), got {tab.shape}")
            self._row = {i: i for i in range(tab.shape[0])}
        self.corners = torch.from_numpy(np.ascontiguousarray(tab)).to(self.device)
        self.class_to_obj = class_to_obj
        self._K = _k_dev(K, self.device)
        if self._K[1] and self._K[0].shape[0] != self.max_frames:
            raise Pose6dError(f"PoseEstimator: per-frame K must have max_frames = {self.max_frames} rows")
        self._frames = self._depth = None
        self._buckets = {}
        self._param_ptrs = self._ptrs()
        self.refresh()

    def _ptrs(self):
        return tuple(t.data_ptr() for t in list(self.model.parameters()) + list(self.model.buffers()))

    def refresh(self):
        """Take over weights written since construction (or the last refresh): re-pack the
        compute-dtype conv weights of every bucket's engines.  If a parameter or buffer
        moved in memory (model.to(), a re-assigned Parameter) the captured graphs and the
        engines are dropped and rebuilt on the next call."""
        if self.model.training:
            raise Pose6dError("PoseEstimator.refresh: the model is in training mode")
        ptrs = self._ptrs()
        if ptrs != self._param_ptrs:
            self._param_ptrs = ptrs
            self._buckets = {}
            return self
        for bk in self._buckets.values():
            own, self.model._p6_engines = self.model._p6_engines, bk.engines
            try:
                self.model.sync_weights()
            finally:
                self.model._p6_engines = own
        return self

    def check(self):
        """Read and reset the crop kernel's status word (raises on a bad frame index)."""
        self.cropper.check()

    def _objs(self, classes, N):
        c = np.asarray(classes.cpu().numpy() if isinstance(classes, torch.Tensor) else classes).reshape(-1)
        if c.shape[0] != N:
            raise Pose6dError(f"PoseEstimator: classes must have one entry per box ({N}), got {c.shape[0]}")
        rows = np.full(N, -1, np.int64)
        for i, k in enumerate(c.tolist()):
            key = k if self.class_to_obj is None else self.class_to_obj.get(k)
            rows[i] = self._row.get(key, -1)
        return rows

    def _slots(self, engine, classes):
        """The refiner's or the verifier's table slot of every detection (-1: no mesh)."""
        c = np.asarray(classes.cpu().numpy() if isinstance(classes, torch.Tensor) else classes).reshape(-1)
        return engine.slots([k if self.class_to_obj is None else self.class_to_obj.get(k) for k in c.tolist()])

    def _stage_frames(self, rgb, depth):
        dev = self.device
        rgb = rgb if isinstance(rgb, torch.Tensor) else torch.from_numpy(np.require(rgb, requirements="CW"))
        if rgb.dim() == 3:
            rgb = rgb[None]
        if rgb.dtype != torch.uint8 or rgb.dim() != 4 or rgb.shape[-1] != 3:
            raise Pose6dError(f"PoseEstimator: rgb must be (F, H, W, 3) uint8, got {tuple(rgb.shape)} {rgb.dtype}")
        F, H, W, _ = rgb.shape
        if F > self.max_frames:
            raise Pose6dError(f"PoseEstimator: {F} frames given, max_frames = {self.max_frames}")
        if self._frames is None or self._frames.shape[1:3] != (H, W):
            # a new frame size: new static buffers, so graphs captured on the old ones go
            self._frames = torch.zeros(self.max_frames, H, W, 3, dtype=torch.uint8, device=dev)
            self._depth = torch.zeros(self.max_frames, H, W, dtype=torch.int16, device=dev).view(torch.uint16)
            for bk in self._buckets.values():
                bk.graph = None
        self._frames[:F].copy_(rgb, non_blocking=True)
        if depth is not None:
            depth = depth if isinstance(depth, torch.Tensor) else torch.from_numpy(np.require(depth, requirements="CW"))
            if depth.dim() == 2:
                depth = depth[None]
            if tuple(depth.shape) != (F, H, W):
                raise Pose6dError(f"PoseEstimator: depth must be (F, H, W) = {(F, H, W)}, got {tuple(depth.shape)}")
            if depth.dtype != torch.uint16:
                depth = depth.to(torch.int32).clamp_(0, 65535).to(torch.uint16)
            self._depth[:F].copy_(depth, non_blocking=True)
        return F

    def _run(self, bk, has_depth):
        """crop -> eval forward -> projection on bucket bk's buffers (the graph's body)."""
        crops = self.cropper(self._frames, self._depth if has_depth else None, bk.boxes, bk.frame_of, self._K,
                             out=bk.crops)
        quat, trans = self.model(*self._inputs(crops))
        res = bk.res
        res._quat.copy_(quat)
        res._trans.copy_(trans.reshape(bk.B, 3))
        pose_project(res._quat, res._trans, self._K, bk.obj, self.corners,
                     boxes=bk.boxes if self.corrects_translation else None, frame_of=bk.frame_of,
                     axis_scale=self.axis_scale, out=(res._trans_cam, res._points, res._pixels, res._valid))
        if self.refine is not None:
            # the network's pose (the translation the projection used) against the depth frame,
            # then the projection of the refined pose: two more launches in the same graph
            self.refine(self._depth, bk.boxes, bk.obj_ref, res._quat, res._trans_cam, frame_of=bk.frame_of, K=self._K,
                        out=(res._quat_ref, res._trans_ref, res._quat32_ref, res._trans32_ref, res._n_corr, res._rms,
                             res._refined))
            pose_project(res._quat32_ref, res._trans32_ref, self._K, bk.obj, self.corners, boxes=None,
                         frame_of=bk.frame_of, axis_scale=self.axis_scale,
                         out=(None, res._points_ref, res._pixels_ref, None))
        if self.verify is not None:
            # render-and-compare of the network's pose and, with refine=, of the refined one: one
            # launch each, the second also writing the choice between the two
            self.verify(self._depth, bk.boxes, bk.obj_ver, res._quat, res._trans_cam, frame_of=bk.frame_of, K=self._K,
                        out=(res._counts, res._fit, res._agree, res._resid, res._verified))
            if self.refine is not None:
                self.verify(self._depth, bk.boxes, bk.obj_ver, res._quat32_ref, res._trans_ref, frame_of=bk.frame_of,
                            K=self._K, out=(res._counts_ref, res._fit_ref, res._agree_ref, res._resid_ref,
                                            res._verified_ref), choose=(res._fit, res._refined, res._best))

    def __call__(self, rgb, depth, boxes, classes, frame_of=None):
        if self.model.training:
            raise Pose6dError("PoseEstimator: the model is in training mode; call model.eval() first")
        bx = _host_boxes(boxes.cpu() if isinstance(boxes, torch.Tensor) else boxes)
        N = bx.shape[0]
        if N > self.max_detections:
            raise Pose6dError(f"PoseEstimator: {N} detections, max_detections = {self.max_detections}")
        if self.refine is not None and depth is None:
            raise Pose6dError("PoseEstimator: refine= needs the depth frame (depth=None given)")
        if self.verify is not None and depth is None:
            raise Pose6dError("PoseEstimator: verify= needs the depth frame (depth=None given)")
        if N == 0:
            return self._result(torch.zeros(self._result.nbytes(1), dtype=torch.uint8, device=self.device), 1, 0)
        B = next(b for b in BUCKETS if b >= N)
        rgb_frames = rgb.shape[0] if rgb.ndim == 4 else 1
        fo = np.zeros(N, np.int64) if frame_of is None else _host_frame_of(frame_of, N, rgb_frames)
        rows = self._objs(classes, N)
        ref_rows = self._slots(self.refine, classes) if self.refine is not None else None
        ver_rows = self._slots(self.verify, classes) if self.verify is not None else None
        F = self._stage_frames(rgb, depth)
        assert F == rgb_frames
        has_depth = depth is not None
        bk = self._buckets.get((B, has_depth))
        if bk is None:
            bk = self._buckets[(B, has_depth)] = _Bucket(B, self.device, self.cropper, self._result,
                                                         self.refine is not None, self.verify is not None)
        # pad by repeating detection 0; one small host -> device copy per table
        pad = lambda a: np.concatenate([a, np.repeat(a[:1], B - N, axis=0)]) if B > N else a
        bk.boxes.copy_(torch.from_numpy(pad(bx).astype(np.int32)), non_blocking=True)
        bk.frame_of.copy_(torch.from_numpy(pad(fo).astype(np.int32)), non_blocking=True)
        bk.obj.copy_(torch.from_numpy(pad(rows)), non_blocking=True)
        if ref_rows is not None:
            bk.obj_ref.copy_(torch.from_numpy(pad(ref_rows)), non_blocking=True)
        if ver_rows is not None:
            bk.obj_ver.copy_(torch.from_numpy(pad(ver_rows)), non_blocking=True)
        own, self.model._p6_engines = self.model._p6_engines, bk.engines
        try:
            with torch.no_grad():
                if not self.graph:
                    self._run(bk, has_depth)
                else:
                    if bk.graph is None:
                        self._capture(bk, has_depth)
                    bk.graph.replay()
        finally:
            self.model._p6_engines = own
        return self._result(bk.out, B, N)

    def _capture(self, bk, has_depth):
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._run(bk, has_depth)   # warm-up: builds this bucket's engines, packs their weights
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            self._run(bk, has_depth)
        bk.graph = g
