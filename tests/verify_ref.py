"""fp64 numpy restatement of the render-and-compare pose verification (pose6d_pose_verify,
csrc/verify.hip) and the triangle meshes its tests run on.  The reference project has no
such step, so this file is the yardstick: brute force, every triangle against every sample,
in chunks of triangles.  The scenes are tests/refine_ref.py's, as they are.

Every step is the kernel's, product by product (numpy rounds each elementwise operation on
its own; nothing here goes through a matmul, which may fuse):
  vertices   c = R m + t, each row ((R0 mx + R1 my) + R2 mz) + t; pu = c.x * fx / c.z + cx;
  samples    refine_ref.sample_pixels;
  coverage   e(a, b, p) = (b.u - a.u)(p.v - a.v) - (b.v - a.v)(p.u - a.u), w0 = e(v1, v2, p),
             w1 = e(v2, v0, p), w2 = e(v0, v1, p), s = (w0 + w1) + w2; covered when all three
             w >= 0 and s > 0 or all three <= 0 and s < 0, and p inside the triangle's pixel
             bounding box (implied by the edge functions in exact arithmetic; stated, with
             exact comparisons, so that culling by the box is exact in floating point too);
             z = s / ((w0 / z0 + w1 / z1) + w2 / z2), kept when finite and positive;
  z-buffer   the minimum z per sample (a minimum has no order);
  classes    0 no hit, 1 hit without depth, 2 consistent, 3 occluded, 4 violated.
Vertices are fp32 data (the packed table's): they enter here as those values in double.
"""
import functools

import numpy as np

from tests import refine_ref as RR

CHUNK = 1 << 21   # (triangles x samples) elements per chunk


# ----------------------------------------------------------------- meshes
@functools.lru_cache(maxsize=None)
def box_mesh(n, size=tuple(RR.BOX)):
    """(verts (6 (n + 1)^2, 3) float32 m, faces (12 n^2, 3) int32) of the box of `size` centred
    at the origin, each face split n x n, two triangles per quad.  Faces do not share
    vertices.  Read-only (shared)."""
    size = np.asarray(size, np.float64)
    g = np.arange(n + 1, dtype=np.float64) / n - 0.5
    a, b = np.meshgrid(g, g, indexing="ij")
    verts, faces = [], []
    r, c = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    i00 = (r * (n + 1) + c).reshape(-1)
    quad = np.stack([i00, i00 + (n + 1), i00 + (n + 2), i00, i00 + (n + 2), i00 + 1], 1).reshape(-1, 3)
    for fidx in range(6):
        ax, sign = fidx // 2, (1.0 if fidx % 2 else -1.0)
        o = [k for k in range(3) if k != ax]
        v = np.empty(((n + 1) ** 2, 3))
        v[:, ax] = sign * size[ax] / 2
        v[:, o[0]] = a.reshape(-1) * size[o[0]]
        v[:, o[1]] = b.reshape(-1) * size[o[1]]
        faces.append(quad + fidx * (n + 1) ** 2)
        verts.append(v)
    verts = np.concatenate(verts).astype(np.float32)
    faces = np.concatenate(faces).astype(np.int32)
    verts.setflags(write=False)
    faces.setflags(write=False)
    return verts, faces


# ----------------------------------------------------------------- the restatement
def project_vertices(verts, quat, trans, K):
    """(pu, pv, z) (V,) double each of the fp32 vertices under the pose; None for a zero, NaN or
    infinite quaternion."""
    q = np.asarray(quat, np.float64)
    qn = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    if not (qn > 0.0 and qn < np.inf):
        return None
    R = RR.quat_to_mat(RR.normalise_quat(quat))
    t = np.asarray(trans, np.float64)
    m = np.asarray(verts, np.float64)
    mx, my, mz = m[:, 0], m[:, 1], m[:, 2]
    with np.errstate(all="ignore"):
        cx = ((R[0, 0] * mx + R[0, 1] * my) + R[0, 2] * mz) + t[0]
        cy = ((R[1, 0] * mx + R[1, 1] * my) + R[1, 2] * mz) + t[1]
        cz = ((R[2, 0] * mx + R[2, 1] * my) + R[2, 2] * mz) + t[2]
        pu = cx * K[0, 0] / cz + K[0, 2]
        pv = cy * K[1, 1] / cz + K[1, 2]
    return pu, pv, cz


def zbuffer(pu, pv, z, nverts, faces, u, v):
    """The minimum rendered depth (P,) double of every sample pixel (u, v), +inf without a hit.
    A face with an index outside [0, nverts), a vertex at z <= 0.001 or a projected coordinate
    that is not finite is skipped."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < nverts)).all(1)
    faces = faces[ok]
    faces = faces[(z[faces] > 0.001).all(1)]
    faces = faces[(np.isfinite(pu[faces]) & np.isfinite(pv[faces])).all(1)]
    pu_s, pv_s = u.astype(np.float64)[None, :], v.astype(np.float64)[None, :]
    zbuf = np.full(len(u), np.inf)
    step = max(1, CHUNK // max(1, len(u)))
    for s0 in range(0, len(faces), step):
        f = faces[s0:s0 + step]
        u0, u1, u2 = (pu[f[:, k]][:, None] for k in range(3))
        v0, v1, v2 = (pv[f[:, k]][:, None] for k in range(3))
        z0, z1, z2 = (z[f[:, k]][:, None] for k in range(3))
        with np.errstate(all="ignore"):
            w0 = (u2 - u1) * (pv_s - v1) - (v2 - v1) * (pu_s - u1)
            w1 = (u0 - u2) * (pv_s - v2) - (v0 - v2) * (pu_s - u2)
            w2 = (u1 - u0) * (pv_s - v0) - (v1 - v0) * (pu_s - u0)
            sm = (w0 + w1) + w2
            cov = ((w0 >= 0) & (w1 >= 0) & (w2 >= 0) & (sm > 0)) | ((w0 <= 0) & (w1 <= 0) & (w2 <= 0) & (sm < 0))
            zr = sm / ((w0 / z0 + w1 / z1) + w2 / z2)
            cov &= (zr > 0) & (zr < np.inf)
            cov &= (pu_s >= np.minimum(np.minimum(u0, u1), u2)) & (pu_s <= np.maximum(np.maximum(u0, u1), u2))
            cov &= (pv_s >= np.minimum(np.minimum(v0, v1), v2)) & (pv_s <= np.maximum(np.maximum(v0, v1), v2))
        zbuf = np.minimum(zbuf, np.where(cov, zr, np.inf).min(0))
    return zbuf


def verify(depth, K, box, verts, faces, diam, quat, trans, G=32, tau=0.1, depth_scale=0.001):
    """The whole verification of one detection.  Returns a dict: zbuf (P,) double (+inf no
    hit), cls (P,) uint8, counts (5,) int32, fit, agree, resid (float), verified (0 / 1)."""
    P = G * G
    out = {"zbuf": np.full(P, np.inf), "cls": np.zeros(P, np.uint8), "counts": np.zeros(5, np.int32), "fit": 0.0,
           "agree": 0.0, "resid": 0.0, "verified": 0}
    proj = project_vertices(verts, quat, trans, K)
    if proj is None or len(faces) == 0:
        return out
    u, v = RR.sample_pixels(box, G)
    zbuf = zbuffer(*proj, len(verts), faces, u, v)
    h, w = depth.shape
    inside = (u >= 0) & (u < w) & (v >= 0) & (v < h)
    d = np.zeros(P, np.float64)
    d[inside] = depth[v[inside], u[inside]]
    hit = np.isfinite(zbuf)
    thr = tau * diam
    with np.errstate(invalid="ignore"):
        diff = d * depth_scale - zbuf
    cls = np.zeros(P, np.uint8)
    cls[hit & (d == 0)] = 1
    seen = hit & (d > 0)
    cls[seen & (np.abs(diff) <= thr)] = 2
    cls[seen & (diff < -thr)] = 3
    cls[seen & (diff > thr)] = 4
    counts = np.bincount(cls, minlength=5).astype(np.int32)
    n2, n3, n4 = int(counts[2]), int(counts[3]), int(counts[4])
    out.update(zbuf=zbuf, cls=cls, counts=counts, verified=1,
               fit=n2 / (n2 + n3 + n4) if n2 + n3 + n4 else 0.0, agree=n2 / (n2 + n4) if n2 + n4 else 0.0,
               resid=float(np.abs(diff[cls == 2]).sum() / n2) if n2 else 0.0)
    return out


@functools.lru_cache(maxsize=None)
def scene_fit(seed, pose, n=8, G=32, tau=0.1):
    """verify() on refine_ref.scene(seed) with the n x n box mesh, computed once.  pose: "true",
    "initial", "refined" (the restatement's ICP result, its quaternion cast to fp32 as the
    estimator's second launch reads it) or "shifted" (the truth moved 30 mm along z)."""
    s = RR.scene(seed)
    if pose == "true":
        q, t = s["q_gt"].astype(np.float32), s["t_gt"]
    elif pose == "initial":
        q, t = s["q0"], s["t0"]
    elif pose == "refined":
        r = RR.scene_result(seed)
        q, t = r["quat"].astype(np.float32), r["trans"]
    else:
        q, t = s["q_gt"].astype(np.float32), s["t_gt"] + np.array([0.0, 0.0, 0.030])
    verts, faces = box_mesh(n)
    return verify(s["depth"], RR.DEFAULT_K, s["box"], verts, faces, s["diam"], q, t, G=G, tau=tau)
