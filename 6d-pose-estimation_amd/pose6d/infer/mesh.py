"""The host helpers that read an object's ASCII `obj_<id>.ply`: the robust box corners the
reference's scripts import, and the points and triangles of the two depth stages."""
import os

import numpy as np


def _read_ply(mesh_dir, obj_id_str):
    """`obj_<id>.ply` read once -> (counts, rows): the header's `element vertex` / `element face`
    counts (None where it gives none) and every non-blank body line as a list of floats; no rows
    for a missing file."""
    path = os.path.join(mesh_dir, f"obj_{obj_id_str}.ply")
    counts, rows, body = {"vertex": None, "face": None}, [], False
    if not os.path.exists(path):
        return counts, rows
    with open(path, "r") as f:
        for line in f:
            v = line.split()
            if body:
                if v:
                    rows.append([float(x) for x in v])
                continue
            if len(v) == 3 and v[0] == "element" and v[1] in counts:
                counts[v[1]] = int(v[2])
            body = "end_header" in line
    return counts, rows


def _metres(rows):
    """The first three numbers of every row, mm -> m, (n, 3) float64."""
    return np.array([r[:3] for r in rows], dtype=np.float64).reshape(-1, 3) / 1000.0


def load_mesh_corners(mesh_dir, obj_id_str):
    """The 8 corners (metres) of an object's robust bounding box, as
    utils/mesh_utils.py:7-53: vertices of the ASCII `obj_<id>.ply` in mm -> m, those
    0.3 m or more from the origin dropped, the box spanned by the 1st and 99th
    percentile per axis; corner order (min, min, min), (max, min, min), (max, max, min),
    (min, max, min), then the same four at max z.  None for a missing mesh or one whose
    vertices are all outliers."""
    _, rows = _read_ply(mesh_dir, obj_id_str)
    # the header's counts are ignored: vertex lines and, as in the reference, face lines ("3 i j k")
    verts = _metres([r for r in rows if len(r) >= 3])
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
    counts, rows = _read_ply(mesh_dir, obj_id_str)
    verts = _metres([r for r in rows if len(r) >= 3][:counts["vertex"]])
    if len(verts) == 0:
        return None
    if len(verts) > n_points:
        verts = verts[np.random.default_rng(seed).choice(len(verts), int(n_points), replace=False)]
    pts = verts.astype(np.float32)
    return pts, _diameter(mesh_dir, obj_id_str, pts)


def _diameter(mesh_dir, obj_id_str, pts):
    """The object's diameter (m): mesh_dir/models_info.yml's (mm) when the file lists the object,
    else the exact largest pairwise distance of the fp32 points pts, in double."""
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
    if diameter is None:
        p = pts.astype(np.float64)
        diameter = max(float(np.sqrt(((p[s:s + 256, None] - p[None]) ** 2).sum(-1).max()))
                       for s in range(0, len(p), 256))
    return diameter


def load_mesh_triangles(mesh_dir, obj_id_str):
    """(verts (V, 3) float32 metres, faces (T, 3) int32, diameter metres) of an object for
    PoseVerifier, from the ASCII `obj_<id>.ply`: the header's `element vertex` count of vertex
    lines (mm -> m), then its `element face` count of face lines `k i0 i1 ... i(k-1)`; a
    polygon of more than three vertices is fanned from its first, (i0, ij, ij+1).  The
    diameter is load_mesh_points': models_info.yml's when the file lists the object, else the
    exact largest pairwise vertex distance.  None for a missing mesh or one without vertices
    or faces."""
    counts, rows = _read_ply(mesh_dir, obj_id_str)
    nv, nf = counts["vertex"] or 0, counts["face"] or 0
    tris = []
    for r in rows[nv:nv + nf]:
        idx = [int(x) for x in r[1:1 + int(r[0])]]
        tris.extend((idx[0], idx[j], idx[j + 1]) for j in range(1, len(idx) - 1))
    if not rows[:nv] or not tris:
        return None
    verts = _metres(rows[:nv]).astype(np.float32)
    faces = np.array(tris, dtype=np.int32).reshape(-1, 3)
    return verts, faces, _diameter(mesh_dir, obj_id_str, verts)
