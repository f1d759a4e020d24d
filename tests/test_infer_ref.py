"""CPU pins of the detection-to-pose helper (tests/infer_ref.py), of the fixture
tests/golden/infer.npz (recorded from the reference's own project_points and
load_mesh_corners by tools/gen_infer_goldens.py) and of pose6d.infer's host side."""
import os

import numpy as np
import pytest

from oracle import crop as OC
from tests import infer_ref as IR

H, W = 480, 640
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "infer.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


# ----------------------------------------------------------------- helper: geometry
def test_centre_and_both_K_hand_computed_on_a_left_top_padded_box():
    # box (-30, -20, 64, 60): w = 94, h = 80, centre (17, 20), size = 112.8 -> crop side 112,
    # origin (int(-39.4), int(-36.4)) = (-39, -36): pad_l = 39, pad_t = 36, scale = 2 exactly
    K = np.array([[572.5, 0, 325.25], [0, 573.5, 242.125], [0, 0, 1]])
    g0 = IR.centre_and_K((-30, -20, 64, 60), K, H, W, 224, k_mode=0)
    g1 = IR.centre_and_K((-30, -20, 64, 60), K, H, W, 224, k_mode=1)
    assert (g0["pad_l"], g0["pad_t"], g0["scale"]) == (39, 36, 2.0)
    # centre: (17 + 39 - 0) * 2, (20 + 36 - 0) * 2
    assert np.array_equal(g0["centre"], np.array([112.0, 112.0], np.float32))
    assert np.array_equal(g0["centre_img"], np.array([17.0, 20.0], np.float32))
    # script: (cx + pad_l - crop_x1) * scale = (325.25 + 39 + 39) * 2; dataset: (cx - crop_x1) * scale
    assert g0["cx_crop_f64"] == 806.5 and g1["cx_crop_f64"] == 728.5
    assert g0["cy_crop_f64"] == (242.125 + 72) * 2 and g1["cy_crop_f64"] == (242.125 + 36) * 2
    # the script's value is exactly pad * scale larger, before the cast
    assert g0["cx_crop_f64"] - g1["cx_crop_f64"] == g0["pad_l"] * g0["scale"] == 78.0
    assert g0["cy_crop_f64"] - g1["cy_crop_f64"] == g0["pad_t"] * g0["scale"] == 72.0
    assert g0["K_crop"][0, 0] == np.float32(1145.0) and g0["K_crop"][1, 1] == np.float32(1147.0)
    assert g0["K_crop"][0, 2] == np.float32(806.5) and g1["K_crop"][0, 2] == np.float32(728.5)
    assert g0["K_crop"].dtype == np.float32 and g0["K_crop"][2, 2] == 1 and g0["K_crop"][0, 1] == 0


def test_K_modes_on_the_default_intrinsics():
    # (-20, -30, 80, 110): 100 x 140, size 168, origin (-54, -44), scale 4 / 3 (inexact):
    # the two formulas differ by pad * scale up to the roundings of the two products
    g0 = IR.centre_and_K((-20, -30, 80, 110), IR.DEFAULT_K, H, W, 224, 0)
    g1 = IR.centre_and_K((-20, -30, 80, 110), IR.DEFAULT_K, H, W, 224, 1)
    assert (g0["pad_l"], g0["pad_t"]) == (54, 44)
    assert abs((g0["cx_crop_f64"] - g1["cx_crop_f64"]) - 54 * g0["scale"]) <= 4 * np.spacing(600.0)
    assert abs((g0["cy_crop_f64"] - g1["cy_crop_f64"]) - 44 * g0["scale"]) <= 4 * np.spacing(600.0)
    # an interior box: no pad, the two agree bit for bit
    a = IR.centre_and_K((200, 150, 320, 240), IR.DEFAULT_K, H, W, 224, 0)
    b = IR.centre_and_K((200, 150, 320, 240), IR.DEFAULT_K, H, W, 224, 1)
    assert np.array_equal(a["K_crop"], b["K_crop"]) and a["pad_l"] == a["pad_t"] == 0
    # double, then ONE cast
    x1 = OC.crop_geometry((200, 150, 120, 90), H, W)[0]
    assert x1 == 188 and a["K_crop"][0, 2] == np.float32((325.2611 - 188) * (224 / 144))


def test_trunc_boxes_toward_zero():
    assert IR.trunc_boxes([(-20.7, -0.9, 80.9, 110.5)]) == [(-20, 0, 80, 110)]


# ----------------------------------------------------------------- helper: float resize
def test_float_weights_2_to_1_column():
    src = np.array([[0, 200], [0, 200]], np.float32)
    # dsize 4: fx = (d + 0.5) / 2 - 0.5 = -0.25, 0.25, 0.75, 1.25 -> edges reset to weight 0
    assert np.array_equal(IR.resize_linear_f32(src, 4)[0], np.array([0, 50, 150, 200], np.float32))
    out = IR.resize_linear_f32(src, 224)[0]
    assert out[0] == 0 and out[-1] == 200 and np.all(np.diff(out) >= 0)
    f = np.float32((111 + 0.5) * (1.0 / (224 / 2)) - 0.5)
    assert out[111] == np.float32(200) * f and out[111] != np.rint(out[111])
    # identity at 224 and constants at any size
    rng = np.random.default_rng(1)
    d = rng.integers(0, 65536, (224, 224)).astype(np.float32)
    assert np.array_equal(IR.resize_linear_f32(d), d)
    for n in (37, 301, 449):
        assert np.all(IR.resize_linear_f32(np.full((n, n), 1234, np.float32)) == 1234)


def test_float_2x_mean():
    src = np.array([[1, 2, 10, 20], [3, 5, 30, 41], [0, 0, 65535, 65535], [0, 1, 65535, 65535]], np.float32)
    assert np.array_equal(IR.resize_linear_f32(src, 2), np.array([[2.75, 25.25], [0.25, 65535.0]], np.float32))


def test_float_path_differs_from_rint_on_half_a_millimetre():
    src = np.array([[1000, 1001], [1000, 1001]], np.uint16)
    big = np.array([[1000, 1001, 7, 7], [1000, 1001, 7, 8], [5, 5, 5, 5], [5, 5, 5, 5]], np.uint16)
    f = IR.resize_linear_f32(big.astype(np.float32), 2)
    u = OC.resize_linear_u16(big, 2)
    assert f[0, 0] == 1000.5 and u[0, 0] == 1001      # (4002 + 2) >> 2
    assert f[0, 1] == 7.25 and u[0, 1] == 7
    fl = IR.resize_linear_f32(src.astype(np.float32), 4)[0]
    ul = OC.resize_linear_u16(src, 4)[0]
    assert np.array_equal(fl, np.array([1000, 1000.25, 1000.75, 1001], np.float32))
    assert np.array_equal(ul, np.array([1000, 1000, 1001, 1001], np.uint16))
    dn, raw = IR.depth_outputs(fl)
    assert raw[1] == np.float32(1000.25) / np.float32(1000) and raw[1] != np.float32(1.0)
    assert dn[1] == (raw[1] - np.float32(0.1)) / np.float32(1.5)
    assert IR.depth_outputs(np.array([9.5, 10.5], np.float32))[0].tolist() == [0.0, 0.0]   # < 0.01 m, then clip


def test_crop_detection_shapes_and_padding():
    rng = np.random.default_rng(2)
    rgb = rng.integers(1, 256, (H, W, 3), dtype=np.uint8)
    depth = rng.integers(300, 1600, (H, W), dtype=np.uint16)
    x, d, raw, c, Kc, ci, Ki = IR.crop_detection(rgb, depth, (-20, -30, 80, 110), IR.DEFAULT_K, mean=None)
    assert x.shape == (3, 224, 224) and d.shape == (1, 224, 224) and raw.shape == (224, 224)
    assert all(a.dtype == np.float32 for a in (x, d, raw, c, Kc, ci, Ki))
    # rows above the frame (44 of 168 crop rows -> 58 output rows) are zero padding
    assert np.all(x[:, :57] == 0) and np.all(raw[:57] == 0) and np.any(x[:, 60:, 80:] != 0)
    assert np.array_equal(Ki, IR.DEFAULT_K.astype(np.float32)) and np.array_equal(ci, np.array([30, 40], np.float32))


# ----------------------------------------------------------------- fixture
def test_projection_restatement_reproduces_the_fixture(gold):
    quat, trans, K = gold["quat"], gold["trans"], gold["K"]
    assert quat.dtype == np.float32 and trans.dtype == np.float32 and gold["pix"].dtype == np.int64
    assert quat.shape == (64, 4) and gold["pix"].shape == (64, 12, 2)
    p3 = np.concatenate([gold["corners"], gold["axes"]])
    behind = 0
    for i in range(64):
        pts = np.concatenate([IR.project_points_f64(gold["corners"], quat[i], trans[i], K)]
                             + [IR.project_points_f64(gold["axes"][j:j + 1], quat[i], trans[i], K) for j in range(4)])
        assert np.array_equal(pts, gold["pts"][i])
        assert np.array_equal(pts.astype(int), gold["pix"][i])
        R = IR.quat_to_matrix(quat[i])
        behind += int(np.sum((p3 @ R.T + trans[i])[:, 2] < 0.001))
        # the plain-Python restatement of scipy's matrix agrees to rounding
        from scipy.spatial.transform import Rotation
        assert np.abs(R - Rotation.from_quat(quat[i]).as_matrix()).max() <= 4 * 2.0 ** -52
    assert behind > 0                                                   # the z clip is exercised
    assert np.abs(gold["pts"] - np.rint(gold["pts"])).min() >= 1e-6     # the generator's guard


def test_load_mesh_corners_against_the_fixture(gold, tmp_path):
    from pose6d.infer import load_mesh_corners
    IR.write_ply(tmp_path / "obj_01.ply", gold["mesh_verts_mm"])
    IR.write_ply(tmp_path / "obj_02.ply", gold["mesh_far_mm"])
    got = load_mesh_corners(str(tmp_path), "01")
    assert got.shape == (8, 3) and got.dtype == np.float64
    assert np.abs(got - gold["mesh_corners"]).max() <= 1e-12
    assert np.sum(np.linalg.norm(gold["mesh_verts_mm"] / 1000.0, axis=1) >= 0.3) >= 30   # the filter has work
    assert load_mesh_corners(str(tmp_path), "02") is None     # all outliers
    assert load_mesh_corners(str(tmp_path), "03") is None     # no such mesh


def test_default_K_is_the_reference_float64():
    from pose6d.infer import DEFAULT_K
    assert DEFAULT_K.dtype == np.float64 and np.array_equal(DEFAULT_K, IR.DEFAULT_K)


# ----------------------------------------------------------------- host-side checks
def test_host_box_and_frame_checks():
    from pose6d import Pose6dError
    from pose6d.infer import _host_boxes, _host_frame_of
    assert _host_boxes([(-20.7, -0.9, 80.9, 110.5)]).tolist() == [[-20, 0, 80, 110]]
    assert _host_boxes(np.array([[1, 2, 3, 4]], np.int32)).dtype == np.int64
    assert _host_boxes([]).shape == (0, 4)
    for bad in ([(10, 10, 10, 20)], [(10, 10, 20, 5)], [(0.2, 0, 0.9, 5)], [(0, 0, float("nan"), 5)], [(1, 2, 3)]):
        with pytest.raises(Pose6dError):
            _host_boxes(bad)
    assert _host_frame_of([0, 1, 1], 3, 2).tolist() == [0, 1, 1]
    for bad in ([0, 2, 0], [-1, 0, 0], [0, 0]):
        with pytest.raises(Pose6dError):
            _host_frame_of(bad, 3, 2)
