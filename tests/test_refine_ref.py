"""CPU checks of the depth refinement's yardstick (tests/refine_ref.py) and of the host
pieces that need no device: the fp64 restatement meets the end-to-end conditions of
tests/test_refine.py on the 12 scenes by itself, its two Horn solvers agree, the entry
point refuses arguments outside its ranges before any launch, and load_mesh_points reads
what it says."""
import ctypes

import numpy as np

from tests import refine_ref as RR


def test_restatement_meets_the_end_to_end_condition():
    worst = 0.0
    for seed in RR.SEEDS:
        r = RR.scene_result(seed)
        ratio = r["add_after"] / r["add_before"]
        worst = max(worst, ratio)
        print(f"seed {seed}: kept {int(r['kept'].sum())}, pairs {r['n_corr']}, ADD {r['add_before'] * 1e3:.2f} -> "
              f"{r['add_after'] * 1e3:.2f} mm (ratio {ratio:.3f})")
        assert r["refined"] and r["n_corr"] >= 16
        assert ratio <= 0.5, (seed, ratio)
    print(f"worst ratio after / before: {worst:.3f}")


def test_sample_pixels_floor_division_and_order():
    u, v = RR.sample_pixels((-7, -5, 10, 4), 4)
    # (2i + 1) * 17 // 8 = 2, 6, 10, 14; (2j + 1) * 9 // 8 = 1, 3, 5, 7
    assert u[:4].tolist() == [-5, -1, 3, 7] and v[::4].tolist() == [-4, -2, 0, 2]
    assert u[4:8].tolist() == u[:4].tolist() and v[:4].tolist() == [-4] * 4
    # an inverted box: floor, not truncation
    u, _ = RR.sample_pixels((10, 0, 7, 4), 2)
    assert u[:2].tolist() == [10 + (-3 // 4), 10 + (-9 // 4)] == [9, 7]


def test_horn_and_kabsch_agree_and_give_proper_rotations():
    rng = np.random.default_rng(3)
    for k in range(40):
        n = int(rng.integers(4, 200))
        m = rng.normal(size=(n, 3)) * 0.05
        if k % 2:
            m[:, 2] = 0.02   # coplanar
        q = RR.normalise_quat(rng.normal(size=4))
        t = rng.normal(size=3)
        p = m @ RR.quat_to_mat(q).T + t + rng.normal(size=(n, 3)) * 1e-3
        qh, Rh, th = RR.horn(m, p)
        Rk, tk = RR.kabsch(m, p)
        assert RR.rotation_angle(Rh, Rk) < 1e-12 and np.abs(th - tk).max() < 1e-12
        assert abs(np.linalg.det(Rh) - 1.0) < 1e-12 and qh[3] >= 0
        assert RR.rotation_angle(Rh, RR.quat_to_mat(q)) < 0.1


def test_entry_point_refuses_bad_arguments_without_gpu():
    from pose6d import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)

    def rc(G=32, iters=10, min_points=16, gate=0.75, trim=0.25, scale=0.001):
        return lib.pose6d_depth_refine(one, 1, 480, 640, scale, one, 0, one, None, one, one, one, one, one, 1, one, one,
                                       1, G, iters, gate, trim, min_points, one, one, None, None, one, one, one, None,
                                       None, None, None)
    for kw, msg in (({"G": 0}, b"G must be in [1, 32]"), ({"G": 33}, b"G must be in [1, 32]"),
                    ({"iters": 0}, b"iters must be in [1, 64]"), ({"iters": 65}, b"iters must be in [1, 64]"),
                    ({"min_points": 2}, b"min_points must be at least 3"), ({"gate": 0.0}, b"gate and trim"),
                    ({"trim": float("nan")}, b"gate and trim"), ({"scale": -1.0}, b"depth_scale")):
        assert rc(**kw) == 1, kw
        assert msg in lib.pose6d_last_error(), (kw, lib.pose6d_last_error())


def test_load_mesh_points(tmp_path):
    from pose6d.infer import load_mesh_points
    from tests.infer_ref import write_ply
    rng = np.random.default_rng(0)
    verts = RR.box_surface(4000, rng) * 1000.0
    write_ply(tmp_path / "obj_05.ply", verts)
    with open(tmp_path / "obj_05.ply", "a") as f:   # face lines are not vertices
        f.write("3 0 1 2\n3 2 3 4\n")
    assert load_mesh_points(str(tmp_path), "07") is None
    pts, diam = load_mesh_points(str(tmp_path), "05", n_points=600, seed=1)
    assert pts.shape == (600, 3) and pts.dtype == np.float32
    m = (verts / 1000.0).astype(np.float32)
    assert all((m == p).all(1).any() for p in pts[:50])          # a subsample of the vertices, in metres
    again, _ = load_mesh_points(str(tmp_path), "05", n_points=600, seed=1)
    other, _ = load_mesh_points(str(tmp_path), "05", n_points=600, seed=2)
    assert np.array_equal(pts, again) and not np.array_equal(pts, other)
    p64 = pts.astype(np.float64)
    exact = np.sqrt(((p64[:, None] - p64[None]) ** 2).sum(-1).max())
    assert diam == exact and 0.10 < diam <= RR.DIAMETER + 1e-6
    whole, _ = load_mesh_points(str(tmp_path), "05", n_points=5000)
    assert whole.shape == (4000, 3) and np.array_equal(whole, m)
    (tmp_path / "models_info.yml").write_text("5: {diameter: 123.3, min_x: -50.0}\n6: {diameter: 99.0}\n")
    assert load_mesh_points(str(tmp_path), "05", n_points=600)[1] == 123.3 / 1000.0
