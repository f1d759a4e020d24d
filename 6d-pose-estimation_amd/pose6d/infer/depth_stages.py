"""The two stages that hold estimated poses against the depth frame, one launch each for N
detections: DepthRefiner (pose6d_depth_refine) and PoseVerifier (pose6d_pose_verify)."""
from collections import namedtuple

import numpy as np
import torch

from .._lib import Pose6dError, call, require_device, stream
from .crop import DEFAULT_K, _k_dev


class _DepthStage:
    """What the two stages share: the key -> table-slot map, the per-device table cache and the
    checks and conversions of the leading arguments of both entry points.  Error texts carry the
    class's name."""

    def __init__(self, keys, diameters, depth_scale):
        missing = [k for k in keys if k not in diameters]
        if missing:
            raise Pose6dError(f"{type(self).__name__}: no diameter for {missing}")
        self._slot = {k: i for i, k in enumerate(keys)}
        self._diam = [float(diameters[k]) for k in keys]
        self.depth_scale = float(depth_scale)
        self._tables = {}

    def slots(self, keys):
        """Table slots (int64 array) of a sequence of keys; -1 for a key without a mesh."""
        return np.array([self._slot.get(k, -1) for k in keys], np.int64)

    def table(self, dev):
        """The packed mesh table on dev (_pack's result), built once per device."""
        T = self._tables.get(dev)
        if T is None:
            T = self._tables[dev] = self._pack(dev)
        return T

    def _prepare(self, depth, boxes, obj, quat, trans, frame_of, K):
        """-> (depth, F, H, W, depth_scale, K, per_frame, boxes, frame_of, obj), (q, t, N): both
        entry points' leading arguments, and the pose and the count that follow their tables."""
        who = type(self).__name__
        require_device(depth, boxes, obj, quat, trans, frame_of)
        if depth.dim() == 2:
            depth = depth[None]
        if depth.dtype != torch.uint16 or depth.dim() != 3:
            raise Pose6dError(f"{who}: depth must be (F, H, W) uint16, got {tuple(depth.shape)} {depth.dtype}")
        F, H, W = depth.shape
        N = quat.shape[0]
        q = quat.detach().to(torch.float32).contiguous()
        t = trans.detach().to(torch.float64).contiguous()
        if q.shape != (N, 4) or t.shape != (N, 3) or obj.numel() != N or tuple(boxes.shape) != (N, 4):
            raise Pose6dError(f"{who}: boxes (N, 4), obj (N,), quat (N, 4) and trans (N, 3) must agree")
        fo = frame_of.to(torch.int32).contiguous() if frame_of is not None else None
        if fo is not None and fo.numel() != N:
            raise Pose6dError(f"{who}: frame_of must have one entry per box ({N}), got {fo.numel()}")
        Kd, per_frame = K if isinstance(K, tuple) else _k_dev(K, quat.device)
        if per_frame and Kd.shape[0] < F:
            raise Pose6dError(f"{who}: per-frame K must have {F} rows, got {Kd.shape[0]}")
        return (depth.contiguous(), F, H, W, self.depth_scale, Kd, per_frame, boxes.to(torch.int32).contiguous(), fo,
                obj.to(torch.int64).contiguous()), (q, t, N)


RefineOutput = namedtuple("RefineOutput", "quat trans quat32 trans32 n_corr rms refined pose_trace corr samples")


class DepthRefiner(_DepthStage):
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
        self._points = [np.array(points[k], np.float32).reshape(-1, 3) for k in keys]   # (copies)
        super().__init__(keys, diameters, depth_scale)
        self.grid, self.iters, self.min_points = int(grid), int(iters), int(min_points)
        self.gate, self.trim = float(gate), float(trim)

    def _pack(self, dev):
        from models.add_loss import _MeshTable
        pts = {i: torch.from_numpy(p) for i, p in enumerate(self._points)}
        return _MeshTable(pts, dict(enumerate(self._diam)), dev)

    def empty_outputs(self, N, dev):
        e = lambda dt, *s: torch.empty(*s, device=dev, dtype=dt)
        return (e(torch.float64, N, 4), e(torch.float64, N, 3), e(torch.float32, N, 4), e(torch.float32, N, 3),
                e(torch.int32, N), e(torch.float64, N, 2), e(torch.uint8, N))

    def __call__(self, depth, boxes, obj, quat, trans, frame_of=None, K=DEFAULT_K, trace=False, out=None):
        head, (q, t, N) = self._prepare(depth, boxes, obj, quat, trans, frame_of, K)
        dev = quat.device
        T = self.table(dev)
        if out is None:
            out = self.empty_outputs(N, dev)
        P = self.grid * self.grid
        dbg = (None, None, None)
        if trace:
            dbg = (torch.empty(N, self.iters + 1, 7, device=dev, dtype=torch.float64),
                   torch.empty(N, self.iters, P, device=dev, dtype=torch.int32),
                   torch.empty(N, P, 3, device=dev, dtype=torch.float64))
        call("depth_refine", *head, T.points, T.off, T.npts, T.diam, T.n_slots, q, t, N, self.grid, self.iters,
             self.gate, self.trim, self.min_points, *out, *dbg, stream())
        return RefineOutput(*out, *dbg)


VerifyOutput = namedtuple("VerifyOutput", "counts fit agree resid verified zbuf cls")


class PoseVerifier(_DepthStage):
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
        super().__init__(keys, diameters, depth_scale)
        self._verts = [np.array(meshes[k][0], np.float32).reshape(-1, 3) for k in keys]   # (copies)
        self._faces = [np.array(meshes[k][1], np.int64).reshape(-1, 3) for k in keys]
        for k, v, f in zip(keys, self._verts, self._faces):
            if f.size and (f.min() < 0 or f.max() >= len(v)):
                raise Pose6dError(f"PoseVerifier: mesh {k!r} has a face index outside [0, {len(v)})")
        self.grid, self.tau = int(grid), float(tau)

    def _pack(self, dev):
        """(verts, faces, voff, nverts, toff, ntri, diam, n_slots) on dev."""
        nv = np.array([len(v) for v in self._verts], np.int64)
        nt = np.array([len(f) for f in self._faces], np.int64)
        i32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.int32)).to(dev)
        cat = lambda parts, dt, w: np.concatenate(parts).astype(dt) if parts else np.zeros((0, w), dt)
        return (torch.from_numpy(cat(self._verts, np.float32, 3)).to(dev),
                torch.from_numpy(cat(self._faces, np.int32, 3)).to(dev),
                i32(np.cumsum(nv) - nv), i32(nv), i32(np.cumsum(nt) - nt), i32(nt),
                torch.tensor(self._diam, dtype=torch.float64, device=dev), len(nv))

    def empty_outputs(self, N, dev):
        e = lambda dt, *s: torch.empty(*s, device=dev, dtype=dt)
        return (e(torch.int32, N, 5), e(torch.float64, N), e(torch.float64, N), e(torch.float64, N),
                e(torch.uint8, N))

    def __call__(self, depth, boxes, obj, quat, trans, frame_of=None, K=DEFAULT_K, maps=False, out=None, choose=None):
        head, (q, t, N) = self._prepare(depth, boxes, obj, quat, trans, frame_of, K)
        dev = quat.device
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
        call("pose_verify", *head, *self.table(dev), q, t, N, self.grid, self.tau, *out, *dbg,
             *(choose or (None, None, None)), stream())
        return VerifyOutput(*out, *dbg)
