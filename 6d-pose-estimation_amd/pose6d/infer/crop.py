"""One-launch detection crops (pose6d_crop_detections) and the host-side conversions of
boxes, frame indices and intrinsics that every inference stage shares."""
from collections import namedtuple

import numpy as np
import torch

from .._lib import Pose6dError, call, require_device, stream
from ..data import IMAGENET_MEAN, IMAGENET_STD

# utils/camera.py:8-12 (float64)
DEFAULT_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], dtype=np.float64)


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

