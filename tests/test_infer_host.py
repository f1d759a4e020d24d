"""CPU pins of pose6d.infer's host side that no device is needed for: the three mesh loaders
on one ASCII PLY, and the byte layout of the estimator's result buffer."""
import numpy as np
import pytest
import torch

PLY = """ply
format ascii 1.0
element vertex 6
property float x
property float y
property float z
element face 4
property list uchar int vertex_indices
end_header
-40 -30 -20
40 -30 -20.5
40 30 -20

-40 30 20
0 0 25 7 7 7
350 10 10
3 0 1 2
4 0 1 2 3
3 2 3 4
3 0 4 5
"""
VERTS = np.array([[-40, -30, -20], [40, -30, -20.5], [40, 30, -20], [-40, 30, 20], [0, 0, 25], [350, 10, 10]],
                 np.float64)
# what load_mesh_corners takes for vertices as well, as the reference does: the first three numbers of a face line
FACE_ROWS = np.array([[3, 0, 1], [4, 0, 1], [3, 2, 3], [3, 0, 4]], np.float64)
FANNED = np.array([[0, 1, 2], [0, 1, 2], [0, 2, 3], [2, 3, 4], [0, 4, 5]], np.int32)


def test_one_ply_through_the_three_loaders(tmp_path):
    """A header with counts, a blank line, a vertex line with extra numbers, a vertex beyond
    0.3 m, triangles and one quad."""
    from pose6d.infer import load_mesh_corners, load_mesh_points, load_mesh_triangles
    (tmp_path / "obj_07.ply").write_text(PLY)
    d = str(tmp_path)
    # corners: every line of three or more numbers, the 0.35 m vertex cut, the 1st / 99th percentile
    rows = np.concatenate([VERTS, FACE_ROWS]) / 1000.0
    rows = rows[np.linalg.norm(rows, axis=1) < 0.3]
    assert len(rows) == len(VERTS) + len(FACE_ROWS) - 1
    lo, hi = np.percentile(rows, 1, axis=0), np.percentile(rows, 99, axis=0)
    want = np.array([[(lo, hi)[s][a] for a, s in enumerate(sel)] for sel in
                     ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))])
    assert np.array_equal(load_mesh_corners(d, "07"), want)
    # points: exactly the header's vertices (the outlier included), in order, when n_points >= V
    v32 = (VERTS / 1000.0).astype(np.float32)
    diam = float(np.sqrt(((v32.astype(np.float64)[:, None] - v32.astype(np.float64)[None]) ** 2).sum(-1).max()))
    for n_points in (6, 1500):
        pts, dm = load_mesh_points(d, "07", n_points=n_points)
        assert pts.dtype == np.float32 and np.array_equal(pts, v32) and dm == diam
    sub, _ = load_mesh_points(d, "07", n_points=4, seed=2)
    assert np.array_equal(sub, v32[np.random.default_rng(2).choice(6, 4, replace=False)])
    # triangles: the vertices, and the faces with the quad fanned from its first vertex
    verts, faces, dm = load_mesh_triangles(d, "07")
    assert verts.dtype == np.float32 and np.array_equal(verts, v32)
    assert faces.dtype == np.int32 and np.array_equal(faces, FANNED) and dm == diam
    # models_info.yml's diameter (mm) wins
    (tmp_path / "models_info.yml").write_text("7: {diameter: 123.5}\n")
    assert load_mesh_points(d, "07")[1] == 0.1235 and load_mesh_triangles(d, "07")[2] == 0.1235
    assert load_mesh_corners(d, "08") is None and load_mesh_points(d, "08") is None
    assert load_mesh_triangles(d, "08") is None


# (name, byte offset, dtype, shape per detection) of every field of the result buffer and its size, per
# (refine, verify, bucket).  Recorded by running the classes of the commit before pose6d.infer became a
# package (its _result_type(refine, verify)) on a CPU uint8 buffer -- not taken from the code under test.
_F4, _F8, _I4, _I8, _U1 = "float32", "float64", "int32", "int64", "uint8"
_BASE = {1: [("quat", 0, _F4, (4,)), ("trans", 16, _F4, (3,)), ("trans_cam", 32, _F8, (3,)),
             ("points", 56, _F8, (12, 2)), ("pixels", 248, _I8, (12, 2)), ("valid", 440, _U1, ())],
         32: [("quat", 0, _F4, (4,)), ("trans", 512, _F4, (3,)), ("trans_cam", 896, _F8, (3,)),
              ("points", 1664, _F8, (12, 2)), ("pixels", 7808, _I8, (12, 2)), ("valid", 13952, _U1, ())]}
_REF = {1: [("quat_ref", 448, _F8, (4,)), ("trans_ref", 480, _F8, (3,)), ("points_ref", 504, _F8, (12, 2)),
            ("pixels_ref", 696, _I8, (12, 2)), ("n_corr", 888, _I4, ()), ("rms", 896, _F8, (2,)),
            ("refined", 912, _U1, ()), ("quat32_ref", 920, _F4, (4,)), ("trans32_ref", 936, _F4, (3,))],
        32: [("quat_ref", 13984, _F8, (4,)), ("trans_ref", 15008, _F8, (3,)), ("points_ref", 15776, _F8, (12, 2)),
             ("pixels_ref", 21920, _I8, (12, 2)), ("n_corr", 28064, _I4, ()), ("rms", 28192, _F8, (2,)),
             ("refined", 28704, _U1, ()), ("quat32_ref", 28736, _F4, (4,)), ("trans32_ref", 29248, _F4, (3,))]}
LAYOUTS = {
    (False, False, 1): (448, _BASE[1]),
    (False, False, 32): (13984, _BASE[32]),
    (False, True, 1): (504, _BASE[1] + [("fit", 448, _F8, ()), ("agree", 456, _F8, ()), ("counts", 464, _I4, (5,)),
                                        ("resid", 488, _F8, ()), ("verified", 496, _U1, ())]),
    (False, True, 32): (15424, _BASE[32] + [("fit", 13984, _F8, ()), ("agree", 14240, _F8, ()),
                                            ("counts", 14496, _I4, (5,)), ("resid", 15136, _F8, ()),
                                            ("verified", 15392, _U1, ())]),
    (True, False, 1): (952, _BASE[1] + _REF[1]),
    (True, False, 32): (29632, _BASE[32] + _REF[32]),
    (True, True, 1): (1072, _BASE[1] + _REF[1] + [
        ("fit", 952, _F8, ()), ("agree", 960, _F8, ()), ("counts", 968, _I4, (5,)), ("resid", 992, _F8, ()),
        ("verified", 1000, _U1, ()), ("fit_ref", 1008, _F8, ()), ("agree_ref", 1016, _F8, ()),
        ("counts_ref", 1024, _I4, (5,)), ("resid_ref", 1048, _F8, ()), ("verified_ref", 1056, _U1, ()),
        ("best", 1064, _U1, ())]),
    (True, True, 32): (32544, _BASE[32] + _REF[32] + [
        ("fit", 29632, _F8, ()), ("agree", 29888, _F8, ()), ("counts", 30144, _I4, (5,)), ("resid", 30784, _F8, ()),
        ("verified", 31040, _U1, ()), ("fit_ref", 31072, _F8, ()), ("agree_ref", 31328, _F8, ()),
        ("counts_ref", 31584, _I4, (5,)), ("resid_ref", 32224, _F8, ()), ("verified_ref", 32480, _U1, ()),
        ("best", 32512, _U1, ())]),
}


@pytest.mark.parametrize("refine,verify,bucket", sorted(LAYOUTS))
def test_result_buffer_layout(refine, verify, bucket):
    from pose6d.infer import PoseResult, RefinedPoseResult
    from pose6d.infer.project import _result_type
    cls = _result_type(refine, verify)
    if not verify:
        assert cls is (RefinedPoseResult if refine else PoseResult)
    nbytes, fields = LAYOUTS[(refine, verify, bucket)]
    assert cls.nbytes(bucket) == nbytes
    buf = torch.zeros(nbytes, dtype=torch.uint8)
    res = cls(buf, bucket, bucket)
    assert [f[0] for f in cls._FIELDS] == [f[0] for f in fields]
    for name, off, dtype, shape in fields:
        t = getattr(res, "_" + name)
        assert (t.data_ptr() - buf.data_ptr(), str(t.dtype), tuple(t.shape)) == \
            (off, "torch." + dtype, (bucket,) + shape), name
    # the properties: the first n rows, valid / refined / verified* as bool
    part = cls(buf, bucket, 1)
    for name, _, dtype, shape in fields:
        if name in ("quat32_ref", "trans32_ref"):
            continue
        v = getattr(part, name)
        flag = name in ("valid", "refined") or name.startswith("verified")
        assert tuple(v.shape) == (1,) + shape and str(v.dtype) == ("torch.bool" if flag else "torch." + dtype), name
    assert part.box2d.shape == (1, 8, 2) and part.axes2d.shape == (1, 4, 2)
    if refine:
        assert part.box2d_ref.data_ptr() == part.pixels_ref.data_ptr() and part.axes2d_ref.shape == (1, 4, 2)
