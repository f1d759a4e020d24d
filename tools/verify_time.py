"""What the pose verification costs: ms per frame of pose6d.infer.PoseEstimator graph replay
without and with verify=PoseVerifier(...), and of the pose6d_pose_verify launch alone, at
N = 1, 8 and 32 detections, G = 32 (1024 samples per box), a box mesh of 27 648 triangles
(tests/verify_ref.py's n = 48: a LineMOD-sized face count, every triangle smaller than a
sample), PoseNetRGBDGeometric in bf16 on 640 x 480 RGB-D frames already on the device.

The frames are tools/refine_time.py's: tests/refine_ref.py's box under one rotation at 12
translations (detection k sits on frame k mod 12), the model's last rotation layer set to
weight 0 and bias = the scene's perturbed quaternion, the translation the model's own.  The
launch alone runs from the scenes' own initial poses.  The samples the render hit and the
fits of both are printed with the times: a launch that rendered nothing would be cheap for
the wrong reason.  (The geometric model's own translation is a point on the visible surface,
2-5 cm in front of the object's centre and so beyond tau x diameter = 12 mm: its render hits
as many samples and costs the same, but none of them is consistent.)

The two estimator routes are alternated in one process and timed with device events, the
host work between the events (table upload, replay, result to the host) inside the window,
as tools/infer_time.py does; the launch alone is R back-to-back launches between two events.

usage: python tools/verify_time.py [--out FILE] [--rounds N] [--reps R] [--mesh-n n]; writes
the table to FILE (default profiles/verify_time.txt) and prints it."""
import argparse
import os
import statistics
import sys
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "6d-pose-estimation_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

TRANSLATIONS = [(x, y, z) for z in (0.7, 0.9) for y in (-0.08, 0.08) for x in (-0.12, 0.0, 0.12)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "verify_time.txt"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--mesh-n", type=int, default=48, help="box faces split n x n (12 n^2 triangles)")
    args = ap.parse_args()
    from models.pose_net_rgbd_geometric import PoseNetRGBDGeometric
    from pose6d.infer import DEFAULT_K, PoseEstimator, PoseVerifier
    from tests import refine_ref as RR
    from tests import verify_ref as VR
    warnings.simplefilter("ignore")
    dev = torch.device("cuda", 0)
    scenes = [RR.scene(100, t_gt=t) for t in TRANSLATIONS]
    F = len(scenes)
    rng = np.random.default_rng(0)
    rgb = torch.from_numpy(rng.integers(0, 256, (F, RR.H, RR.W, 3), dtype=np.uint8)).to(dev)
    depth = torch.from_numpy(np.stack([s["depth"] for s in scenes]).astype(np.int32)).to(dev).to(torch.uint16)
    lo, hi = -RR.BOX / 2, RR.BOX / 2
    corners = np.array([[(lo, hi)[(i >> a) & 1][a] for a in range(3)] for i in (0, 1, 3, 2, 4, 5, 7, 6)])
    torch.manual_seed(0)
    model = PoseNetRGBDGeometric(pretrained=False).to(dev).set_compute_dtype(torch.bfloat16).eval()
    with torch.no_grad():
        model.rot_head[-1].weight.zero_()
        model.rot_head[-1].bias.copy_(torch.from_numpy(scenes[0]["q0"]))
    mesh = VR.box_mesh(args.mesh_n)
    mk_ver = lambda: PoseVerifier({0: mesh}, {0: RR.DIAMETER}, grid=32, tau=0.1)
    est_plain = PoseEstimator(model, corners[None], max_frames=F, graph=True)
    est_ver = PoseEstimator(model, corners[None], max_frames=F, graph=True, verify=mk_ver())
    alone = mk_ver()

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    fmt = lambda v: "%.3f [%.3f, %.3f]" % (statistics.median(v), min(v), max(v))
    lines = ["pose verification, G = 32, %d triangles, PoseNetRGBDGeometric bf16, 640x480 RGB-D frames on the device, "
             "ms (median [min, max] of %d alternated rounds of %d)" % (len(mesh[1]), args.rounds, args.reps),
             "(a) PoseEstimator graph=True   (b) the same with verify=   (c) pose6d_pose_verify alone, back-to-back "
             "launches;  hits = samples the render covered (min-max over the detections), fit likewise",
             "%3s  %-24s %-24s %-9s %-24s %-30s %s" % ("N", "(a)", "(b)", "(b)-(a)", "(c)", "(b) hits, fit",
                                                        "(c) hits, fit")]
    for n in (1, 8, 32):
        idx = [k % F for k in range(n)]
        boxes = [scenes[k]["box"] for k in idx]
        cls = [0] * n
        bx = torch.tensor(boxes, dtype=torch.int32, device=dev)
        fo = torch.tensor(idx, dtype=torch.int32, device=dev)
        obj = torch.zeros(n, dtype=torch.int64, device=dev)
        q0 = torch.from_numpy(np.stack([scenes[k]["q0"] for k in idx])).to(dev)
        t0 = torch.from_numpy(np.stack([scenes[k]["t0"] for k in idx])).to(dev)
        out = alone.empty_outputs(n, dev)
        route_a = lambda: est_plain(rgb, depth, boxes, cls, idx).cpu()
        route_b = lambda: est_ver(rgb, depth, boxes, cls, idx).cpu()
        route_c = lambda: alone(depth, bx, obj, q0, t0, frame_of=fo, K=DEFAULT_K, out=out)
        routes = (route_a, route_b, route_c)
        for fn in routes * 2:
            fn()
        t = [[], [], []]
        for _ in range(args.rounds):
            for k, fn in enumerate(routes):
                t[k].append(timed(fn, args.reps))
        rb = route_b()
        rc = route_c()
        torch.cuda.synchronize()
        hits = lambda c: c[:, 1:].sum(1)
        told = lambda c, f: "%d-%d, %.3f-%.3f" % (int(hits(c).min()), int(hits(c).max()), float(f.min()),
                                                   float(f.max()))
        lines.append("%3d  %-24s %-24s %-9.3f %-24s %-30s %s" % (
            n, fmt(t[0]), fmt(t[1]), statistics.median(t[1]) - statistics.median(t[0]), fmt(t[2]),
            told(rb.counts, rb.fit), told(rc.counts.cpu(), rc.fit.cpu())))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
