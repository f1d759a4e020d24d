"""Helper (not a test): numpy restatement of the per-detection body of the reference's
scripts/inference/inference_rgbd_geometric.py:110-182 (the other three scripts use subsets
of it), used to check pose6d_crop_detections bit for bit, and of utils/visualization.py's
project_points.

Line by line:
  * :111      x1, y1, x2, y2 = map(int, box.xyxy[0])         -> `trunc_boxes`
  * :118-135  square crop x1.2 around the box, zero padding  -> oracle.crop.crop_geometry on
              (x1, y1, x2 - x1, y2 - y1): (x1 + x2) / 2 == x1 + (x2 - x1) / 2 exactly in double
  * :141      cv2.resize(crop_rgb, (224, 224))               -> oracle.crop.resize_linear_u8
  * :142      cv2.resize(crop_depth.astype(np.float32), ...) -> `resize_linear_f32`: OpenCV's 32F
              INTER_LINEAR (the 16U path's float coefficients, mul + add, no rounding to an
              integer, no saturation); the exact 2x case is INTER_AREA's (a + b + c + d) * 0.25f
  * :145-153  centre in the resized crop: Python double, ONE cast to float32, then the clip
  * :156-167  K_crop: Python double, one cast.  cx_crop = (cx + pad_l - crop_x1) * scale uses the
              UNPADDED origin crop_x1; the dataset (data/dataset_rgbd.py:138-139,161) subtracts
              the origin with the pad added back, (cx + pad_l - (x1 + pad_l)) = cx - x1.  The
              script's value is pad_l * scale larger (`k_mode` 0 = script, 1 = dataset).
  * :170-173  depth_meters = resized / 1000.0 (float32), (d - 0.1) / (1.6 - 0.1) clipped to [0, 1]
              (1.6 - 0.1 == 1.5 in double), zero where depth_meters < 0.01
  * :176      ToPILImage / ToTensor / Normalize              -> (u8 / 255 - mean) / std in fp32
  * inference_rgb_geometric.py:105-106  centre and K of the ORIGINAL image as float32

PARITY NOTE: run_inference itself cannot be executed here (cv2 and ultralytics are absent),
so the resize stays PARITY-UNPINNED exactly as in oracle/crop.py: it is checked against
hand-computed cases (tests/test_infer_ref.py), not against cv2's own output.  The geometry
follows the cited lines.
"""
import numpy as np

from oracle import crop as OC

DEFAULT_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])


def write_ply(path, verts_mm):
    """A minimal ASCII ply; repr() round-trips every double."""
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "end_header\n" % len(verts_mm))
        for v in verts_mm:
            f.write("%r %r %r\n" % (float(v[0]), float(v[1]), float(v[2])))


def trunc_boxes(boxes):
    """map(int, box.xyxy[0]): truncation toward zero."""
    return [tuple(int(v) for v in b) for b in boxes]


def resize_linear_f32(src, dsize=224):
    """cv2.resize(src (n, n) float32, (dsize, dsize)) INTER_LINEAR."""
    src = np.asarray(src, np.float32)
    n = src.shape[0]
    if n == 2 * dsize:
        s = ((src[0::2, 0::2] + src[0::2, 1::2]).astype(np.float32) + src[1::2, 0::2]).astype(np.float32)
        return ((s + src[1::2, 1::2]).astype(np.float32) * np.float32(0.25)).astype(np.float32)
    sx, fx = OC._coeffs(dsize, n, True)
    sy, fy = OC._coeffs(dsize, n, False)
    ax0, ax1 = np.float32(1.0) - fx, fx
    by0, by1 = np.float32(1.0) - fy, fy
    sx1 = np.minimum(sx + 1, n - 1)
    edge = sx >= n - 1
    hrow = np.where(edge[None, :], src[:, sx] * np.float32(1.0),
                    (src[:, sx] * ax0[None, :]).astype(np.float32) + (src[:, sx1] * ax1[None, :]).astype(np.float32))
    hrow = hrow.astype(np.float32)
    r0 = np.clip(sy, 0, n - 1)
    r1 = np.clip(sy + 1, 0, n - 1)
    return ((hrow[r0] * by0[:, None]).astype(np.float32) + (hrow[r1] * by1[:, None]).astype(np.float32)).astype(
        np.float32)


def centre_and_K(box, K, h_img, w_img, img_size=224, k_mode=0):
    """(:145-167) -> dict of the DOUBLE values before the cast (`*_f64`) and the float32
    outputs; `pad_l`, `pad_t`, `scale` for the tests."""
    x1, y1, x2, y2 = (int(v) for v in box)
    K = np.asarray(K, np.float64).reshape(3, 3)
    c_x_box, c_y_box = (x1 + x2) / 2, (y1 + y2) / 2
    crop_x1, crop_y1, crop_size, pad_l, pad_t, _, _ = OC.crop_geometry((x1, y1, x2 - x1, y2 - y1), h_img, w_img)
    adj_x1, adj_y1 = crop_x1 + pad_l, crop_y1 + pad_t
    scale = img_size / crop_size
    cc = ((c_x_box + pad_l - adj_x1) * scale, (c_y_box + pad_t - adj_y1) * scale)
    centre = np.clip(np.array(cc, dtype=np.float32), 0, img_size - 1)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    if k_mode == 0:
        cx_crop, cy_crop = (cx + pad_l - crop_x1) * scale, (cy + pad_t - crop_y1) * scale
    else:
        cx_crop, cy_crop = (cx - crop_x1) * scale, (cy - crop_y1) * scale
    K_crop = np.array([[fx * scale, 0, cx_crop], [0, fy * scale, cy_crop], [0, 0, 1]], dtype=np.float32)
    return {"centre": centre, "K_crop": K_crop, "cx_crop_f64": cx_crop, "cy_crop_f64": cy_crop, "pad_l": pad_l,
            "pad_t": pad_t, "scale": scale, "centre_img": np.array([c_x_box, c_y_box], dtype=np.float32),
            "K_img": K.astype(np.float32)}


def depth_outputs(resized_mm):
    """(:170-173) float32 resized depth in mm -> (depth_normalized, depth_meters)."""
    raw = (np.asarray(resized_mm, np.float32) / np.float32(1000.0)).astype(np.float32)
    dn = ((raw - np.float32(0.1)) / np.float32(1.5)).astype(np.float32)
    dn = np.clip(dn, np.float32(0), np.float32(1))
    dn[raw < np.float32(0.01)] = 0
    return dn.astype(np.float32), raw


def crop_detection(rgb, depth, box, K, img_size=224, mean=OC.IMAGENET_MEAN, std=OC.IMAGENET_STD, k_mode=0):
    """One detection.  rgb (H, W, 3) uint8 RGB, depth (H, W) uint16 or None.  Returns rgb
    (3, S, S), depth (1, S, S), depth_raw (S, S), centre (2,), K_crop (3, 3), centre_img (2,),
    K_img (3, 3), all float32.  mean=None: ToTensor only."""
    h_img, w_img = rgb.shape[:2]
    if depth is None:
        depth = np.zeros((h_img, w_img), np.uint16)
    x1, y1, x2, y2 = (int(v) for v in box)
    cx1, cy1, n, _, _, _, _ = OC.crop_geometry((x1, y1, x2 - x1, y2 - y1), h_img, w_img)
    rgb_r = OC.resize_linear_u8(OC.crop_pixels(rgb, cx1, cy1, n), img_size)
    d_r = resize_linear_f32(OC.crop_pixels(depth, cx1, cy1, n).astype(np.float32), img_size)
    dn, raw = depth_outputs(d_r)
    x = rgb_r.astype(np.float32).transpose(2, 0, 1) / np.float32(255.0)
    if mean is not None:
        m = np.array(mean, np.float32)[:, None, None]
        s = np.array(std, np.float32)[:, None, None]
        x = ((x - m) / s).astype(np.float32)
    g = centre_and_K(box, K, h_img, w_img, img_size, k_mode)
    return x.astype(np.float32), dn[None], raw, g["centre"], g["K_crop"], g["centre_img"], g["K_img"]


def quat_to_matrix(q):
    """scipy Rotation.from_quat(q).as_matrix() restated: float64, normalise, unit-quaternion matrix."""
    x, y, z, w = (float(v) for v in np.asarray(q, np.float64))
    nrm = np.sqrt(x * x + y * y + z * z + w * w)
    x, y, z, w = x / nrm, y / nrm, z / nrm, w / nrm
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    return np.array([[x2 - y2 - z2 + w2, 2 * (xy - zw), 2 * (xz + yw)],
                     [2 * (xy + zw), -x2 + y2 - z2 + w2, 2 * (yz - xw)],
                     [2 * (xz - yw), 2 * (yz + xw), -x2 - y2 + z2 + w2]])


def project_points_f64(points_3d, quat, translation, K):
    """utils/visualization.py:21-31 restated with scipy, before the astype(int)."""
    from scipy.spatial.transform import Rotation
    r_mat = Rotation.from_quat(quat).as_matrix()
    p_cam = (r_mat @ points_3d.T).T + translation
    z = np.clip(p_cam[:, 2], 0.001, None)
    pts = np.zeros((points_3d.shape[0], 2))
    pts[:, 0] = (p_cam[:, 0] * K[0, 0] / z) + K[0, 2]
    pts[:, 1] = (p_cam[:, 1] * K[1, 1] / z) + K[1, 2]
    return pts


def projection_bound(points_3d, quat, translation, K):
    """Per coordinate, 16 * 2^-52 * (sum of the absolute values of the terms of that
    coordinate): |R_i0 c_0| + |R_i1 c_1| + |R_i2 c_2| + |t_i|, carried through * K / z, plus
    |K_i2|.  Each coordinate takes at most eight roundings past R's entries."""
    R = np.abs(quat_to_matrix(quat))
    c = np.abs(np.asarray(points_3d, np.float64))
    t = np.abs(np.asarray(translation, np.float64))
    mag = c @ R.T + t
    Rs = quat_to_matrix(quat)
    z = np.clip((np.asarray(points_3d, np.float64) @ Rs.T + translation)[:, 2], 0.001, None)
    out = np.zeros((len(c), 2))
    out[:, 0] = mag[:, 0] * abs(K[0, 0]) / z + abs(K[0, 2])
    out[:, 1] = mag[:, 1] * abs(K[1, 1]) / z + abs(K[1, 2])
    return 16 * 2.0 ** -52 * out
