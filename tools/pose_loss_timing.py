"""Point-matching pose criteria, forward + backward: this build (one sv_pose_match_loss call per batch) against the
reference-style torch loop over the batch (utils/loss.py:166-249, restated below on the same GPU tensors).

Per loss type and side: ms per call (median over --calls after --warmup, torch.cuda.Event around criterion + backward),
kernel launches per call (torch.profiler device events of one call), peak memory of one call above what was allocated
before it.  shape_match's reference builds an [n, 3, n] difference tensor per instance: it shows in the peak.

  python tools/pose_loss_timing.py [--batch 16] [--voxels 4096] [--calls 20] [--warmup 3] [--types pose,shape_match,...]
Every (type, side) runs in a child process of its own under --timeout seconds; the first failure stops the run.
  python tools/pose_loss_timing.py --only shape_match:torch      # one measurement, in this process
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TYPES = ["pose", "shape_match", "pose_match", "kp_pose_match"]


def shell_voxels(rng, n, radii):
    import numpy as np

    got = np.zeros((0, 3), np.int64)
    while len(got) < n:
        d = rng.normal(size=(4 * n, 3))
        c = np.rint(d / np.linalg.norm(d, axis=1, keepdims=True) * radii * rng.uniform(0.9, 1.1, (4 * n, 1)))
        got = np.unique(np.concatenate([got, c.astype(np.int64)]), axis=0)
    return got[rng.permutation(len(got))[:n]].astype(np.int32)


def reference_loop(name, y, y_pred, x, labels, ignore_label, to_matrix):
    """utils/loss.py:166-249 with reduction "mean", op for op"""
    import torch

    rot_mat, rot_mat_pred = to_matrix(y[:, 3:]), to_matrix(y_pred[:, 3:])
    total = 0.0
    if name == "kp_pose_match":
        for i in range(len(x)):
            kp_mask = labels[i] > ignore_label
            coords = x[i][kp_mask, :3]
            a = torch.matmul(rot_mat[i], coords.transpose(0, 1)) + y[i, :3].view(3, -1)
            b = torch.matmul(rot_mat_pred[i], coords.transpose(0, 1)) + y_pred[i, :3].view(3, -1)
            norms = torch.linalg.norm(b - a, dim=0)
            total = total + torch.pow(x[i][kp_mask, -1] * norms, 2).sum() / (2 * norms.size()[0])
        return total / len(x)
    decomposed = x.decomposed_coordinates
    for i, coords in enumerate(decomposed):
        c = torch.transpose(coords.float(), 0, 1)
        a, b = torch.matmul(rot_mat[i], c), torch.matmul(rot_mat_pred[i], c)
        if name == "pose":
            norms = torch.linalg.norm(b - a, dim=0)
            total = total + torch.pow(norms, 2).sum() / (2 * norms.size()[0])
        elif name == "shape_match":
            diff = b.view(3, 1, -1).permute((2, 0, 1)) - a  # [n, 3, n]
            norms = torch.linalg.norm(diff, dim=1)
            total = total + torch.pow(norms, 2).min(dim=1).values.sum() / (2 * len(coords))
        else:
            a, b = a + y[i, :3].view(3, -1), b + y_pred[i, :3].view(3, -1)
            total = total + torch.linalg.norm(b - a, dim=0, ord=1).sum() / len(coords)
    total = total / len(decomposed)
    return total * 1e3 if name == "pose" else total


def measure(name, side, args):
    import numpy as np
    import torch

    import mrcc_amd
    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd.utils.config import Config
    from mrcc_amd.utils.loss import LossType, get_criterion
    from mrcc_amd.utils.transformation import get_quaternion_rotation_matrix_torch

    mrcc_amd._lib.load()
    dev = torch.device("cuda:0")
    Config().update({"DATA": {"center_at_origin": False, "voxelize_position": True}})
    rng = np.random.default_rng(0)
    B, n = args.batch, args.voxels
    q = rng.normal(size=(B, 4))
    y = torch.from_numpy(np.concatenate([rng.uniform(-1, 1, (B, 3)), q], 1).astype(np.float32)).to(dev)
    y_pred = torch.from_numpy(np.concatenate([rng.uniform(-1, 1, (B, 3)), q + 0.1 * rng.normal(size=(B, 4))],
                                             1).astype(np.float32)).to(dev)
    labels = None
    if name == "kp_pose_match":
        x = torch.from_numpy(np.concatenate([rng.uniform(-0.3, 0.3, (B, n, 3)), rng.uniform(0.05, 1, (B, n, 1))],
                                            2).astype(np.float32)).to(dev)
        labels = torch.from_numpy(rng.integers(0, 6, (B, n))).to(dev)
        labels[torch.from_numpy(rng.uniform(size=(B, n)) < 0.2).to(dev)] = -100
    else:
        crops = [shell_voxels(rng, int(n * f), np.array([40.0, 28.0, 20.0])) for f in rng.uniform(0.9, 1.1, B)]
        coords4 = np.concatenate([np.concatenate([np.full((len(c), 1), b, np.int32), c], 1) for b, c in enumerate(crops)])
        x = ME.SparseTensor(torch.zeros(len(coords4), 3), coordinates=torch.from_numpy(coords4).int(), device=dev)
    if side == "hip":
        crit = get_criterion(loss_type=LossType(name), reduction="mean")
        kw = {"labels": labels} if labels is not None else {}
        fn = lambda p: crit(y, p, x=x, **kw)  # noqa: E731
    else:
        fn = lambda p: reference_loop(name, y, p, x, labels, -100, get_quaternion_rotation_matrix_torch)  # noqa: E731

    def call():
        p = y_pred.clone().requires_grad_(True)
        loss = fn(p)
        loss.backward()
        return loss.detach(), p.grad

    for _ in range(args.warmup):
        first = call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.calls):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        call()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    again = call()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2**20
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        call()
        torch.cuda.synchronize()
    launches = sum(e.count for e in prof.key_averages() if e.device_time_total > 0)
    same = torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    print(f"{name:14s} {side:5s} B={B} rows/instance~{n}: {statistics.median(ms):8.3f} ms/call (min {min(ms):.3f})  "
          f"{launches:5d} launches/call  peak +{peak:8.1f} MiB  loss {float(again[0]):.6g}  same bits twice: {same}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--voxels", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--types", default=",".join(TYPES))
    ap.add_argument("--timeout", type=int, default=120)
    ap.add_argument("--only", default=None, help="TYPE:SIDE (side = hip or torch): measure in this process")
    args = ap.parse_args()
    if args.only:
        name, side = args.only.split(":")
        measure(name, side, args)
        return 0
    print(f"# forward + backward of the criterion, B = {args.batch} instances of about {args.voxels} rows, reduction mean; "
          f"{args.calls} timed calls after {args.warmup}")
    sys.stdout.flush()
    for name in args.types.split(","):
        for side in ("hip", "torch"):
            cmd = [sys.executable, os.path.abspath(__file__), "--only", f"{name}:{side}", "--batch", str(args.batch),
                   "--voxels", str(args.voxels), "--calls", str(args.calls), "--warmup", str(args.warmup)]
            try:
                rc = subprocess.run(cmd, timeout=args.timeout).returncode
            except subprocess.TimeoutExpired:
                print(f"{name} {side}: no result within {args.timeout} s; stopping")
                return 124
            if rc != 0:  # a failed measurement ends the run: nothing more is started on the device
                print(f"{name} {side}: exit status {rc}; stopping")
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
