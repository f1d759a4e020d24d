"""PoseEstimator: crop -> eval forward -> projection (-> refinement -> verification) of one
frame batch's detections, replayed from one hipGraph per detection-count bucket."""
import numpy as np
import torch

from .._lib import Pose6dError
from .crop import DEFAULT_K, CropDetections, _host_boxes, _host_frame_of, _k_dev
from .depth_stages import DepthRefiner, PoseVerifier
from .project import PoseResult, _result_type, pose_project

BUCKETS = (1, 2, 4, 8, 16, 32)

# inputs of the four model kinds and whether the scripts correct the translation by the
# box centre (inference_rgb.py:99-104, inference_rgbd.py:159-164) -- the two geometric
# models compute a metric translation themselves
_KINDS = {
    "PoseNetRGB": (lambda c: (c.rgb,), True),
    "PoseNetRGBD": (lambda c: (c.rgb, c.depth), True),
    "PoseNetRGBGeometric": (lambda c: (c.rgb, c.center_img, c.K_img), False),
    "PoseNetRGBDGeometric": (lambda c: (c.rgb, c.depth, c.depth_raw, c.center_crop, c.K_crop), False),
}


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

    def _keys(self, classes, N):
        """The key of every detection's class: what `corners` and the refiner's and the verifier's
        tables are looked up by."""
        c = np.asarray(classes.cpu().numpy() if isinstance(classes, torch.Tensor) else classes).reshape(-1)
        if c.shape[0] != N:
            raise Pose6dError(f"PoseEstimator: classes must have one entry per box ({N}), got {c.shape[0]}")
        return [k if self.class_to_obj is None else self.class_to_obj.get(k) for k in c.tolist()]

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
        keys = self._keys(classes, N)
        rows = np.array([self._row.get(k, -1) for k in keys], np.int64)   # -1: no corners, no mesh
        ref_rows = self.refine.slots(keys) if self.refine is not None else None
        ver_rows = self.verify.slots(keys) if self.verify is not None else None
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
