"""The fp64 projection launch (pose6d_pose_project) and the result classes of a PoseEstimator:
views of one output buffer, one field list per stage."""
import functools

import numpy as np
import torch

from .._lib import Pose6dError, call, require_device, stream
from .crop import _k_dev

N_POINTS = 12   # 8 box corners, origin, x / y / z axis tips


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


# (name, dtype, shape per detection) of every field, in buffer order; each starts on a multiple of 8 bytes
_BASE_FIELDS = (("quat", torch.float32, (4,)), ("trans", torch.float32, (3,)), ("trans_cam", torch.float64, (3,)),
                ("points", torch.float64, (N_POINTS, 2)), ("pixels", torch.int64, (N_POINTS, 2)),
                ("valid", torch.uint8, ()))
_REFINE_FIELDS = (("quat_ref", torch.float64, (4,)), ("trans_ref", torch.float64, (3,)),
                  ("points_ref", torch.float64, (N_POINTS, 2)), ("pixels_ref", torch.int64, (N_POINTS, 2)),
                  ("n_corr", torch.int32, ()), ("rms", torch.float64, (2,)), ("refined", torch.uint8, ()))
# what the projection of the refined pose read: in the buffer, without a property
_REFINE_SCRATCH = (("quat32_ref", torch.float32, (4,)), ("trans32_ref", torch.float32, (3,)))
_VERIFY_FIELDS = (("fit", torch.float64, ()), ("agree", torch.float64, ()), ("counts", torch.int32, (5,)),
                  ("resid", torch.float64, ()), ("verified", torch.uint8, ()))


def _nbytes(bucket, dt, shape):
    return bucket * int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dt).element_size()


class _ResultBuffer:
    """`bucket` detections' fields as views of one uint8 buffer, the first n of them in use."""
    _FIELDS = ()

    def __init__(self, buf, bucket, n):
        self._buf, self._bucket, self.n = buf, bucket, n
        off = 0
        for name, dt, shape in self._FIELDS:
            nbytes = _nbytes(bucket, dt, shape)
            setattr(self, "_" + name, buf[off:off + nbytes].view(dt).view(bucket, *shape))
            off += (nbytes + 7) // 8 * 8

    @classmethod
    def nbytes(cls, bucket):
        return sum((_nbytes(bucket, dt, shape) + 7) // 8 * 8 for _, dt, shape in cls._FIELDS)

    def cpu(self):
        return type(self)(self._buf.cpu(), self._bucket, self.n)

    def clone(self):
        return type(self)(self._buf.clone(), self._bucket, self.n)


def _with_fields(fields, scratch=()):
    """Class decorator: `fields` (and `scratch`) join the end of the base's buffer, with one
    property per field: its first n rows -- as bool for valid, refined and verified*; a pixels
    field also gives box2d (its 8 corners) and axes2d (origin, x, y, z tips)."""
    def extend(cls):
        cls._FIELDS = cls.__bases__[0]._FIELDS + fields + scratch
        for field, _, _ in fields:
            view = (lambda s, a="_" + field: getattr(s, a)[:s.n])
            as_bool = field in ("valid", "refined") or field.startswith("verified")
            setattr(cls, field, property((lambda s, v=view: v(s).bool()) if as_bool else view))
            if field.startswith("pixels"):
                setattr(cls, "box2d" + field[6:], property(lambda s, v=view: v(s)[:, :8]))
                setattr(cls, "axes2d" + field[6:], property(lambda s, v=view: v(s)[:, 8:]))
        return cls
    return extend


@_with_fields(_BASE_FIELDS)
class PoseResult(_ResultBuffer):
    """Poses of N detections.  quat (N, 4) / trans (N, 3): the model's fp32 outputs;
    trans_cam (N, 3) f64: the translation the projection used (bbox-centre corrected for the
    RGB and RGBD models, else trans); points (N, 12, 2) f64 and their truncation pixels
    (N, 12, 2) i64 -- box2d = pixels[:, :8] (project_points of the 8 corners), axes2d =
    pixels[:, 8:] (origin, x, y, z tips: draw_axes); valid (N,) bool: False (rows zero)
    for a class without a mesh or a zero quaternion.
    From a PoseEstimator these are views of its output buffer, valid until its next call:
    .cpu() (one device-to-host copy) or .clone() keeps them."""


@_with_fields(_REFINE_FIELDS, _REFINE_SCRATCH)
class RefinedPoseResult(PoseResult):
    """A PoseResult plus the depth-refined pose (PoseEstimator(refine=...)): quat_ref (N, 4)
    f64 (x, y, z, w; unit, w >= 0) and trans_ref (N, 3) f64; points_ref / pixels_ref (and
    box2d_ref, axes2d_ref): the projection of the refined pose; n_corr (N,) i32 accepted
    pairs of the last iteration, rms (N, 2) f64 their root-mean-square distance in the first
    and the last iteration (m), refined (N,) bool: False where the refinement had nothing to
    work with (no mesh, zero depth in the box, too few pairs) -- quat_ref / trans_ref are
    then the network's pose.  A buffer layout of its own: PoseResult's fields first."""


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
    doc = base.__doc__ + "\n\n" + _result_type.__doc__
    return _with_fields(fields)(type("Verified" + base.__name__, (base,), {"__doc__": doc}))
