"""CPU checks of the pose verification's yardstick (tests/verify_ref.py) and of the host
pieces that need no device: the fp64 restatement separates right poses from wrong ones on the
12 scenes by itself, an occluder lowers `fit` and leaves `agree`, load_mesh_triangles reads
what it says, PoseVerifier refuses a face index outside its mesh, and the entry point refuses
arguments outside its ranges before any launch."""
import ctypes

import numpy as np
import pytest

from tests import refine_ref as RR
from tests import verify_ref as VR


def test_restatement_ranks_the_poses_on_the_twelve_scenes():
    """G = 32, tau = 0.1, the 8 x 8 box mesh.  fit >= 0.9 at the true pose, fit(refined) >
    fit(initial) on every scene, fit <= 0.05 with the truth moved 30 mm along z.
    Re-derived here (CPU): true pose minimum 0.949; restatement-refined pose minimum 0.878
    (seed 107; 0.905 is the next, seed 103); initial pose maximum 0.807; moved truth exactly 0
    on all twelve."""
    fits = {p: [VR.scene_fit(s, p)["fit"] for s in RR.SEEDS] for p in ("true", "refined", "initial", "shifted")}
    for i, seed in enumerate(RR.SEEDS):
        print(f"seed {seed}: " + ", ".join(f"{p} {fits[p][i]:.4f}" for p in fits))
    print("true min %.4f, refined min %.4f, initial max %.4f, shifted max %.4f" % (
        min(fits["true"]), min(fits["refined"]), max(fits["initial"]), max(fits["shifted"])))
    for i, seed in enumerate(RR.SEEDS):
        assert VR.scene_fit(seed, "true")["verified"] == 1
        assert fits["true"][i] >= 0.9, seed
        assert fits["refined"][i] > fits["initial"][i], seed
        assert fits["shifted"][i] <= 0.05, seed


def test_counts_and_ratios_follow_from_the_classes():
    r = VR.scene_fit(100, "initial")
    c = r["counts"]
    assert c.sum() == 1024 and np.array_equal(c, np.bincount(r["cls"], minlength=5))
    assert r["fit"] == c[2] / (c[2] + c[3] + c[4]) and r["agree"] == c[2] / (c[2] + c[4])
    assert np.array_equal(np.isfinite(r["zbuf"]), r["cls"] > 0) and (r["zbuf"] > 0).all()
    assert 0.0 < r["resid"] <= 0.1 * RR.DIAMETER


def test_an_occluder_lowers_fit_and_leaves_agree():
    """The left half of the box's depth overwritten with 300 (mm): the model's samples there
    become class 3; agree stays >= 0.9, fit drops below 0.7."""
    s = RR.scene(100)
    x1, y1, x2, y2 = s["box"]
    depth = s["depth"].copy()
    depth[y1:y2, x1:(x1 + x2) // 2] = 300
    verts, faces = VR.box_mesh(8)
    q, t = s["q_gt"].astype(np.float32), s["t_gt"]
    free = VR.scene_fit(100, "true")
    occ = VR.verify(depth, RR.DEFAULT_K, s["box"], verts, faces, s["diam"], q, t)
    u, _ = RR.sample_pixels(s["box"], 32)
    left = u < (x1 + x2) // 2
    assert np.array_equal(occ["zbuf"], free["zbuf"])                       # the render does not see the frame
    assert (occ["cls"][left & (free["cls"] > 0)] == 3).all() and (left & (free["cls"] > 0)).sum() > 100
    assert np.array_equal(occ["cls"][~left], free["cls"][~left])
    print(f"free fit {free['fit']:.4f}; occluded: fit {occ['fit']:.4f}, agree {occ['agree']:.4f}, "
          f"counts {occ['counts']}")
    assert occ["agree"] >= 0.9 and occ["fit"] < 0.7


def test_box_meshes():
    for n, nt in ((1, 12), (8, 768), (48, 27648)):
        verts, faces = VR.box_mesh(n)
        assert faces.shape == (nt, 3) and verts.shape == (6 * (n + 1) ** 2, 3) and verts.dtype == np.float32
        assert faces.min() == 0 and faces.max() == len(verts) - 1
        v = verts.astype(np.float64)[faces]
        area = 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)
        a, b, c = RR.BOX
        assert abs(area.sum() - 2 * (a * b + b * c + a * c)) < 1e-8 and (area > 0).all()


def test_load_mesh_triangles(tmp_path):
    from pose6d.infer import load_mesh_triangles
    verts = np.array([[0, 0, 0], [100, 0, 0], [100, 50, 0], [0, 50, 0], [50, 25, 80.5]], np.float64)
    with open(tmp_path / "obj_03.ply", "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 5\nproperty float x\nproperty float y\n"
                "property float z\nelement face 4\nproperty list uchar int vertex_indices\nend_header\n")
        for v in verts:
            f.write("%r %r %r\n" % tuple(float(x) for x in v))
        f.write("4 0 1 2 3\n3 0 1 4\n3 1 2 4\n5 0 1 2 3 4\n")
        f.write("3 2 3 4\n")   # beyond the header's face count: not read
    assert load_mesh_triangles(str(tmp_path), "07") is None
    v, fc, diam = load_mesh_triangles(str(tmp_path), "03")
    assert v.dtype == np.float32 and fc.dtype == np.int32
    assert np.array_equal(v, (verts / 1000.0).astype(np.float32))
    assert fc.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4], [0, 1, 2], [0, 2, 3], [0, 3, 4]]
    p = v.astype(np.float64)
    assert diam == np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1).max()) and 0.11 < diam < 0.12
    (tmp_path / "models_info.yml").write_text("3: {diameter: 131.5, min_x: 0.0}\n6: {diameter: 99.0}\n")
    assert load_mesh_triangles(str(tmp_path), "03")[2] == 131.5 / 1000.0
    # vertices only: no triangles to render
    with open(tmp_path / "obj_04.ply", "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
                "end_header\n0 0 0\n1 1 1\n")
    assert load_mesh_triangles(str(tmp_path), "04") is None


def test_verifier_refuses_a_face_outside_its_mesh():
    from pose6d import Pose6dError
    from pose6d.infer import PoseVerifier
    verts, faces = VR.box_mesh(1)
    ver = PoseVerifier({"a": (verts, faces), "b": None}, {"a": RR.DIAMETER})
    assert ver.slots(["a", "b", "c"]).tolist() == [0, -1, -1]
    for bad in (len(verts), -1):
        f = faces.copy()
        f[7, 2] = bad
        with pytest.raises(Pose6dError, match="face index"):
            PoseVerifier({"a": (verts, f)}, {"a": RR.DIAMETER})
    with pytest.raises(Pose6dError, match="diameter"):
        PoseVerifier({"a": (verts, faces)}, {})


def test_entry_point_refuses_bad_arguments_without_gpu():
    from pose6d import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)

    def rc(G=32, tau=0.1, scale=0.001, N=1, F=1, H=480, W=640, depth=one, counts=one, verts=one, best=None):
        return lib.pose6d_pose_verify(depth, F, H, W, scale, one, 0, one, None, one, verts, one, one, one, one, one,
                                      one, 1, one, one, N, G, tau, counts, one, one, one, one, None, None, None, None,
                                      best, None)
    for kw, msg in (({"G": 0}, b"G must be in [1, 64]"), ({"G": 65}, b"G must be in [1, 64]"), ({"tau": 0.0}, b"tau"),
                    ({"tau": -0.1}, b"tau"), ({"tau": float("nan")}, b"tau"), ({"scale": 0.0}, b"depth_scale"),
                    ({"scale": -1.0}, b"depth_scale"), ({"N": -1}, b"bad shape"), ({"F": -1}, b"bad shape"),
                    ({"H": -1}, b"bad shape"), ({"W": -1}, b"bad shape"), ({"depth": None}, b"null input"),
                    ({"verts": None}, b"null triangle table"), ({"counts": None}, b"null output"),
                    ({"best": one}, b"best needs")):
        assert rc(**kw) == 1, kw
        assert msg in lib.pose6d_last_error(), (kw, lib.pose6d_last_error())
    assert rc(N=0) == 0 and rc(N=0, depth=None, counts=None) == 0   # nothing to do: no launch
