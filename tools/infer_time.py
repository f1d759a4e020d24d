"""ms per frame of detection-to-pose inference with PoseNetRGBDGeometric (fp32 and bf16) on
one 640 x 480 RGB-D frame already on the device, N = 1, 4 and 13 detections, three routes
alternated in one process and timed with device events (the host work between the events
is inside the window):

  (a) the route available without pose6d.infer, in the structure of the reference's
      scripts/inference/inference_rgbd_geometric.py: per detection a B = 1 CropRGBD call (its
      box uploaded from the host) and a B = 1 forward of the drop-in module, a device-to-host
      copy of the pose, and the projection of the 3D box and axes in numpy / scipy on the
      host.  Its numerics are the dataset's, not the scripts' (16U depth resize, float32
      intrinsics): a TIME baseline only;
  (b) pose6d.infer.PoseEstimator with graph=True: tables uploaded, ONE graph replay (crop ->
      eval forward -> projection), PoseResult.cpu();
  (c) the same with graph=False.

usage: python tools/infer_time.py [--out FILE] [--rounds N] [--reps R]; writes the table to
FILE (default profiles/infer_time.txt) and prints it."""
import argparse
import os
import statistics
import sys
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "6d-pose-estimation_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W = 480, 640
AXES = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1]], dtype=np.float64)


def detections(n, rng):
    """n plausible detector boxes inside the frame, some hanging over its edges."""
    out = []
    for _ in range(n):
        w, h = int(rng.integers(40, 180)), int(rng.integers(40, 180))
        x, y = int(rng.integers(-20, W - w + 20)), int(rng.integers(-20, H - h + 20))
        out.append((x, y, x + w, y + h))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "infer_time.txt"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    from models.pose_net_rgbd_geometric import PoseNetRGBDGeometric
    from pose6d.data import CropRGBD
    from pose6d.infer import DEFAULT_K, PoseEstimator
    from tests.infer_ref import project_points_f64
    warnings.simplefilter("ignore")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    rgb = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
    depth = torch.from_numpy(rng.integers(300, 1600, (H, W)).astype(np.int32)).to(dev).to(torch.uint16)
    lo, hi = np.array([-0.05, -0.08, -0.06]), np.array([0.05, 0.06, 0.06])
    corners = np.array([[(lo, hi)[(i >> a) & 1][a] for a in range(3)] for i in (0, 1, 3, 2, 4, 5, 7, 6)])
    K32 = torch.from_numpy(DEFAULT_K.astype(np.float32))[None].to(dev)
    crop1 = CropRGBD(224)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    lines = ["detection-to-pose, PoseNetRGBDGeometric, one 640x480 RGB-D frame on the device, ms per frame "
             "(median [min, max] of %d alternated rounds of %d frames, device events, result on the host)"
             % (args.rounds, args.reps),
             "(a) per detection: B=1 CropRGBD + B=1 drop-in forward + D2H + numpy projection   "
             "(b) PoseEstimator graph=True   (c) PoseEstimator graph=False",
             "%-5s %3s  %-24s %-24s %-24s %s" % ("dtype", "N", "(a)", "(b)", "(c)", "(a)/(b)")]
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        torch.manual_seed(0)
        model = PoseNetRGBDGeometric(pretrained=False).to(dev).set_compute_dtype(dt).eval()
        est_g = PoseEstimator(model, corners[None], graph=True)
        est_e = PoseEstimator(model, corners[None], graph=False)
        for n in (1, 4, 13):
            boxes = detections(n, rng)
            cls = [0] * n

            def route_a():
                out = []
                with torch.no_grad():
                    for x1, y1, x2, y2 in boxes:
                        bb = torch.tensor([[x1, y1, x2 - x1, y2 - y1]], dtype=torch.int32, device=dev)
                        c = crop1(rgb[None], depth[None], bb, bb, K32)
                        quat, trans = model(*c)
                        q, t = quat.cpu().numpy()[0], trans.cpu().numpy().reshape(3)
                        box2d = project_points_f64(corners, q, t, DEFAULT_K).astype(int)
                        axes2d = [project_points_f64(AXES[j:j + 1], q, t, DEFAULT_K).astype(int)[0] for j in range(4)]
                        out.append((q, t, box2d, axes2d))
                return out

            route_b = lambda: est_g(rgb, depth, boxes, cls).cpu()
            route_c = lambda: est_e(rgb, depth, boxes, cls).cpu()
            routes = (route_a, route_b, route_c)
            for fn in routes * 2:                     # warm up every shape the routes use
                fn()
            t = [[], [], []]
            for _ in range(args.rounds):              # alternated: all see the same machine
                for k, fn in enumerate(routes):
                    t[k].append(timed(fn, args.reps))
            fmt = lambda v: "%.3f [%.3f, %.3f]" % (statistics.median(v), min(v), max(v))
            lines.append("%-5s %3d  %-24s %-24s %-24s %.2f" % (name, n, fmt(t[0]), fmt(t[1]), fmt(t[2]),
                                                               statistics.median(t[0]) / statistics.median(t[1])))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
