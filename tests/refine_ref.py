"""fp64 numpy restatement of the depth refinement (pose6d_depth_refine, csrc/refine.hip)
and the synthetic scenes its tests run on.  The reference project has no refinement step,
so this file is the yardstick: sampling, back-projection, gate, brute-force nearest point,
trim and Horn's closed form through numpy.linalg.eigh, every step in double.

What is shared with the kernel bit for bit (each product rounded on its own, as numpy
does): the sample pixels, the back-projection and the gate.  What is not: the kernel
searches on fp32 differences and solves Horn by Jacobi sweeps; tests/test_refine.py
bounds both against the functions here.

Mesh points are fp32 data (the packed mesh table's): they enter here as those values in
double.
"""
import functools

import numpy as np

DEFAULT_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
H, W = 480, 640
BOX = np.array([0.10, 0.06, 0.04])
DIAMETER = float(np.sqrt((BOX ** 2).sum()))   # 0.1233 m
SEEDS = tuple(range(100, 112))


# ----------------------------------------------------------------- rotations
def quat_to_mat(q):
    """Unit quaternion (x, y, z, w) -> 3 x 3."""
    x, y, z, w = (float(v) for v in q)
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    return np.array([[x2 - y2 - z2 + w2, 2.0 * (xy - zw), 2.0 * (xz + yw)],
                     [2.0 * (xy + zw), -x2 + y2 - z2 + w2, 2.0 * (yz - xw)],
                     [2.0 * (xz - yw), 2.0 * (yz + xw), -x2 - y2 + z2 + w2]])


def normalise_quat(q):
    """Double, unit, w >= 0 (what the kernel does to its fp32 input)."""
    q = np.asarray(q, np.float64)
    q = q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return -q if q[3] < 0 else q


def axis_angle_quat(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.concatenate([axis * np.sin(angle / 2), [np.cos(angle / 2)]])


def quat_mul(a, b):
    """The quaternion of R(a) R(b), (x, y, z, w)."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def rotation_angle(Ra, Rb):
    """Angle (rad) of Ra^T Rb, from the skew part (accurate near zero)."""
    D = Ra.T @ Rb
    s = 0.5 * np.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
    return float(np.arctan2(s, 0.5 * (np.trace(D) - 1.0)))


# ----------------------------------------------------------------- steps 1 and 2
def sample_pixels(box, G):
    """(u (P,), v (P,)) int64 of the G x G samples of box (x1, y1, x2, y2); sample k = j G + i."""
    x1, y1, x2, y2 = (int(v) for v in box)
    i = np.arange(G, dtype=np.int64)
    u = x1 + ((2 * i + 1) * (x2 - x1)) // (2 * G)     # floor division
    v = y1 + ((2 * i + 1) * (y2 - y1)) // (2 * G)
    return np.tile(u, G), np.repeat(v, G)


def samples(depth, K, box, G, trans0, gate, diam, depth_scale=0.001):
    """(points (P, 3) double, kept (P,) bool): the back-projected samples and which of them
    are valid and within gate * diam of the initial translation (NaN rows elsewhere)."""
    u, v = sample_pixels(box, G)
    h, w = depth.shape
    inside = (u >= 0) & (u < w) & (v >= 0) & (v < h)
    d = np.zeros(u.shape, np.float64)
    d[inside] = depth[v[inside], u[inside]]
    valid = inside & (d > 0)
    z = d * depth_scale
    x = (u.astype(np.float64) - K[0, 2]) * z / K[0, 0]
    y = (v.astype(np.float64) - K[1, 2]) * z / K[1, 1]
    dx, dy, dz = x - trans0[0], y - trans0[1], z - trans0[2]
    with np.errstate(invalid="ignore"):
        kept = valid & (np.sqrt(dx * dx + dy * dy + dz * dz) <= gate * diam)
    pts = np.stack([x, y, z], 1)
    pts[~kept] = np.nan
    return pts, kept


def to_model(pts, R, t):
    """q = R^T (p - t) per row."""
    return (pts - t) @ R


def nearest(q, mesh):
    """Brute force in double: (first-index argmin (n,), its distance (n,)) of mesh (m, 3)."""
    idx = np.empty(len(q), np.int64)
    dist = np.empty(len(q), np.float64)
    m64 = np.asarray(mesh, np.float64)
    for s in range(0, len(q), 256):
        d2 = ((q[s:s + 256, None, :] - m64[None]) ** 2).sum(-1)
        idx[s:s + 256] = d2.argmin(1)
        dist[s:s + 256] = np.sqrt(d2.min(1))
    return idx, dist


def horn(m, p):
    """Horn's closed form: (unit quaternion (x, y, z, w) with w >= 0, R, t) of the rigid
    motion taking the points m (n, 3) onto p (n, 3) in the least-squares sense."""
    mb, pb = m.mean(0), p.mean(0)
    S = (m - mb).T @ (p - pb)
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    Nm = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                   [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                   [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                   [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    _, vec = np.linalg.eigh(Nm)
    e = vec[:, -1]
    q = normalise_quat([e[1], e[2], e[3], e[0]])
    R = quat_to_mat(q)
    return q, R, pb - R @ mb


def kabsch(m, p):
    """The same motion by SVD (a second fp64 solver: its disagreement with horn() measures
    what double precision gives on these pairs)."""
    mb, pb = m.mean(0), p.mean(0)
    U, _, Vt = np.linalg.svd((p - pb).T @ (m - mb))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    return R, pb - R @ mb


def icp(depth, K, box, mesh, diam, quat, trans, G=32, iters=10, gate=0.75, trim=0.25, min_points=16,
        depth_scale=0.001):
    """The whole refinement of one detection.  Returns a dict: trace (iters + 1, 7), corr
    (iters, P) (mesh index, -1, or -2 for an iteration that did not complete), n_corr, rms
    (2,), refined, samples (P, 3), kept (P,)."""
    P = G * G
    trans = np.asarray(trans, np.float64)
    q = normalise_quat(quat)
    t = trans.copy()
    pts, kept = samples(depth, K, box, G, trans, gate, diam, depth_scale)
    mesh64 = np.asarray(mesh, np.float64)
    trace = np.empty((iters + 1, 7))
    trace[0] = np.concatenate([q, t])
    corr = np.full((iters, P), -2, np.int64)
    n_corr, rms, done = 0, [0.0, 0.0], 0
    for it in range(iters):
        R = quat_to_mat(q)
        idx, dist = nearest(to_model(pts[kept], R, t), mesh64)
        acc = dist <= trim * diam
        if acc.sum() < min_points:
            break
        c = np.full(P, -1, np.int64)
        c[np.nonzero(kept)[0][acc]] = idx[acc]
        corr[it] = c
        q, R, t = horn(mesh64[idx[acc]], pts[kept][acc])
        r = float(np.sqrt((dist[acc] ** 2).mean()))
        if it == 0:
            rms[0] = r
        rms[1], n_corr, done = r, int(acc.sum()), it + 1
        trace[it + 1] = np.concatenate([q, t])
    trace[done + 1:] = trace[done]
    return {"trace": trace, "corr": corr, "n_corr": n_corr, "rms": np.array(rms), "refined": done > 0,
            "samples": pts, "kept": kept, "quat": trace[-1, :4].copy(), "trans": trace[-1, 4:].copy()}


def add_metric(mesh, q_a, t_a, q_b, t_b):
    """ADD (m): mean distance between the mesh under the two poses."""
    m = np.asarray(mesh, np.float64)
    a = m @ quat_to_mat(normalise_quat(q_a)).T + t_a
    b = m @ quat_to_mat(normalise_quat(q_b)).T + t_b
    return float(np.sqrt(((a - b) ** 2).sum(1)).mean())


# ----------------------------------------------------------------- scenes
def box_surface(n, rng, size=BOX):
    """n area-uniform points on the surface of the box of `size`, centred at the origin."""
    a, b, c = size
    area = np.array([b * c, b * c, a * c, a * c, a * b, a * b])
    face = rng.choice(6, n, p=area / area.sum())
    uv = rng.random((n, 2)) - 0.5
    pts = np.empty((n, 3))
    for fidx in range(6):
        ax, sign = fidx // 2, (1.0 if fidx % 2 else -1.0)
        sel = face == fidx
        o = [k for k in range(3) if k != ax]
        pts[sel, ax] = sign * size[ax] / 2
        pts[sel, o[0]] = uv[sel, 0] * size[o[0]]
        pts[sel, o[1]] = uv[sel, 1] * size[o[1]]
    return pts


def render_depth(pts_cam, K=DEFAULT_K, h=H, w=W, background=1200):
    """uint16 depth (mm): every point lands on its nearest pixel, which keeps the minimum z."""
    u = np.rint(pts_cam[:, 0] * K[0, 0] / pts_cam[:, 2] + K[0, 2]).astype(np.int64)
    v = np.rint(pts_cam[:, 1] * K[1, 1] / pts_cam[:, 2] + K[1, 2]).astype(np.int64)
    ok = (u >= 0) & (u < w) & (v >= 0) & (v < h)
    zbuf = np.full(h * w, np.inf)
    np.minimum.at(zbuf, v[ok] * w + u[ok], pts_cam[ok, 2])
    hit = np.isfinite(zbuf)
    depth = np.full(h * w, background, np.uint16)
    depth[hit] = np.rint(zbuf[hit] * 1000.0).astype(np.uint16)
    box = (int(u[ok].min()) - 6, int(v[ok].min()) - 6, int(u[ok].max()) + 6, int(v[ok].max()) + 6)
    return depth.reshape(h, w), box


@functools.lru_cache(maxsize=None)
def scene(seed, t_gt=None, n_mesh=1500, n_render=400000):
    """One synthetic RGB-D detection: a 0.10 x 0.06 x 0.04 m box under a random pose,
    rendered from n_render surface points; an independent n_mesh-point fp32 mesh; an initial
    pose 3-8 degrees and N(0, 6 mm) per axis off the truth.  t_gt (a tuple) replaces the
    drawn translation, every other draw staying the same.  Arrays are read-only (shared)."""
    rng = np.random.default_rng(seed)
    q_gt = normalise_quat(rng.normal(size=4))
    drawn = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.10, 0.10), rng.uniform(0.6, 1.0)])
    t_gt = drawn if t_gt is None else np.array(t_gt, np.float64)
    cam = box_surface(n_render, rng) @ quat_to_mat(q_gt).T + t_gt
    depth, box = render_depth(cam)
    mesh = box_surface(n_mesh, rng).astype(np.float32)
    dq = axis_angle_quat(rng.normal(size=3), np.deg2rad(rng.uniform(3.0, 8.0)))
    q0 = normalise_quat(quat_mul(dq, q_gt)).astype(np.float32)
    t0 = t_gt + rng.normal(0.0, 0.006, 3)
    out = {"depth": depth, "box": box, "mesh": mesh, "diam": DIAMETER, "q_gt": q_gt, "t_gt": t_gt, "q0": q0, "t0": t0}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def scene_result(seed, G=32, iters=10):
    """The restatement on scene(seed) with the default gate and trim, computed once."""
    s = scene(seed)
    r = icp(s["depth"], DEFAULT_K, s["box"], s["mesh"], s["diam"], s["q0"], s["t0"], G=G, iters=iters)
    r["add_before"] = add_metric(s["mesh"], s["q0"], s["t0"], s["q_gt"], s["t_gt"])
    r["add_after"] = add_metric(s["mesh"], r["quat"], r["trans"], s["q_gt"], s["t_gt"])
    return r
