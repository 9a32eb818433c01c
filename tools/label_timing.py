"""Training labels for a batch of end-effector crops: the batched device calls (utils.data.key_point_labels_batch:
sv_key_points + sv_radius_labels; utils.data.vote_labels_batch: sv_line_topk) against the same labels from the host
numpy restated below (per frame: get_key_points, collect_closest_points and the label write of load_key_points,
get_ee_cross_section_idx; utils/data.py:106-252,338-342, data/alivev2.py:212-268), then the copy to the device.

B frames of a synthetic gripper of EE-crop size (--points rows each, float32), float64 poses.  Per side: wall-clock ms
per batch from the crops (device side: already on the device, as ee_crop_batch leaves them; host side: host arrays) to
both label tensors on the device (median over --calls after --warmup, device synchronised at both ends), and kernel
launches per batch (torch.profiler device events of one batch).  No speed-up is asserted anywhere.

  python tools/label_timing.py [--batch 16] [--points 4000] [--calls 20] [--warmup 3]
Every side runs in a child process of its own under --timeout seconds; the first failure stops the run.
  python tools/label_timing.py --only device      # one measurement, in this process
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def gripper(rng, n):
    """n rows: a box body, two fingers, a rod along the x axis and background, posed; (float32 points, pose w first)"""
    import numpy as np

    from mrcc_amd.utils.transformation import get_quaternion_rotation_matrix

    nb, nf, nr = n * 6 // 10, n // 10, n // 20
    body = rng.uniform([-0.03, -0.1, 0.0], [0.03, 0.1, 0.075], size=(nb, 3))
    fingers = rng.uniform([-0.01, 0.03, 0.075], [0.01, 0.06, 0.12], size=(2 * nf, 3))
    fingers[nf:, 1] *= -1
    ang, rad = rng.uniform(0, 2 * np.pi, nr), rng.uniform(0, 0.003, nr)
    rod = np.stack([rng.uniform(-0.05, 0.05, nr), rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    rest = rng.uniform([-0.05, -0.11, -0.006], [0.05, 0.11, 0.12], size=(n - nb - 2 * nf - nr, 3))
    ee = np.concatenate([body, fingers, rod, rest])[rng.permutation(n)]
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    pos = rng.uniform(-0.5, 0.5, 3)
    R = get_quaternion_rotation_matrix(q, switch_w=False)
    return (ee @ R.T + pos).astype(np.float32), np.concatenate([pos, q])


def host_labels(points, pose, ignore=-100):
    """(key-point labels, vote labels) of one crop on the host, numpy as the reference writes it"""
    import numpy as np

    from mrcc_amd.utils.transformation import get_quaternion_rotation_matrix, select_closest_points_to_line

    R = get_quaternion_rotation_matrix(pose[3:], switch_w=False)
    q = (R.T @ np.concatenate((points, pose[:3].reshape(1, 3))).reshape((-1, 3, 1))).reshape((-1, 3))
    q = q[:-1] - q[-1:]
    kp = np.array([[0.02, 0.09, 0], [0.02, -0.09, 0], [0.014, 0.095, 0.07], [0.014, -0.095, 0.07], [0, 0.048, 0.12],
                   [0, -0.048, 0.12], [-0.022, 0.09, 0], [-0.022, -0.09, 0], [-0.014, 0.095, 0.07], [-0.014, -0.095, 0.07]])
    idx = np.zeros(10, dtype=np.int64) + ignore

    def closest(target, rows):
        d = np.linalg.norm(q[rows] - target, axis=1)
        return rows[d.argmin()], d.min()

    front, back = np.where(q[:, 0] > 0.005)[0], np.where(q[:, 0] < -0.01)[0]
    for s, dx in enumerate((-0.04, -0.04, -0.03, -0.03)):
        if len(front):
            i, d = closest(kp[s], front)
            if d < 0.018:
                kp[s], idx[s], kp[6 + s] = q[i], i, q[i] + [dx, 0, 0]
    for s in range(4):
        if len(back):
            i, d = closest(kp[6 + s], back)
            if d < 0.018:
                kp[6 + s], idx[6 + s] = q[i], i
    grip = np.where(q[:, 2] > 0.08)[0]
    for g, (rows, y) in enumerate(((grip[q[grip, 1] > 0], 0.01), (grip[q[grip, 1] < 0], -0.01))):
        if len(rows):
            i = closest(np.array([0, y, q[rows, 2].max()]), rows)[0]
            idx[4 + g] = grip[np.searchsorted(rows, i)]  # the reference's index: the side's position looked up in `grip`
    labels = np.zeros(len(points), dtype=np.int64) + ignore
    real = idx > -1
    norms = np.linalg.norm(points[idx[real]].reshape(-1, 1, 3) - points, axis=2)
    pcls, pidx = np.where(norms < 0.006)
    labels[pidx] = np.arange(10)[real][pcls]
    moved = np.array(points, copy=True)
    moved -= pose[:3]
    ql = (R.T @ moved.reshape((-1, 3, 1))).reshape((-1, 3))
    _, cs = select_closest_points_to_line(ql, np.array([-0.05, 0, 0]), np.array([0.05, 0, 0]), count=32, cutoff=0.004)
    vote = np.zeros(len(points), dtype=np.int64)
    vote[cs] = 1
    return labels, vote


def measure(side, args):
    import numpy as np
    import torch

    import mrcc_amd
    from mrcc_amd.utils.data import key_point_labels_batch, vote_labels_batch

    mrcc_amd._lib.load()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    frames = [gripper(rng, args.points) for _ in range(args.batch)]
    pts, poses = [f[0] for f in frames], np.stack([f[1] for f in frames])
    pts_d = torch.from_numpy(np.concatenate(pts)).to(dev)
    off_d = torch.arange(args.batch + 1, dtype=torch.int32, device=dev) * args.points

    def device_batch():
        labels, _, _ = key_point_labels_batch(pts_d, off_d, poses, generator="10")
        return labels, vote_labels_batch(pts_d, off_d, poses, value=1)

    def host_batch():
        both = [host_labels(p, pose) for p, pose in zip(pts, poses)]
        return (torch.from_numpy(np.concatenate([b[0] for b in both])).to(dev),
                torch.from_numpy(np.concatenate([b[1] for b in both])).to(dev))

    fn = device_batch if side == "device" else host_batch
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    launches = sum(e.count for e in prof.key_averages() if e.device_time_total > 0)
    print(f"{side:6s} B={args.batch} x {args.points} points: {statistics.median(ms):9.3f} ms/batch (min {min(ms):.3f})  "
          f"{launches:4d} launches/batch  {int((out[0] >= 0).sum())} key-point rows, {int(out[1].sum())} vote rows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=120)
    ap.add_argument("--only", default=None, help="device or host: measure in this process")
    args = ap.parse_args()
    if args.only:
        measure(args.only, args)
        return 0
    print(f"# key-point (10) and vote labels of one batch: {args.batch} end-effector crops of {args.points} points")
    sys.stdout.flush()
    for side in ("device", "host"):
        cmd = [sys.executable, os.path.abspath(__file__), "--only", side, "--batch", str(args.batch), "--points",
               str(args.points), "--calls", str(args.calls), "--warmup", str(args.warmup)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"{side}: no result within {args.timeout} s; stopping")
            return 124
        if rc != 0:  # a failed measurement ends the run: nothing more is started on the device
            print(f"{side}: exit status {rc}; stopping")
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
