"""Criterion and per-step metrics of a segmentation training step: this build (SegmentationCriterion: one
sv_seg_criterion call for loss, gradient and confusion counts; StepMetrics.to_host) against the reference formulation on
the same GPU tensors: torch CrossEntropyLoss(ignore_index) forward + backward plus compute_accuracies as
train_segmentation.py:34-46 words it (an arg-max over all rows and a float(...) per frame).  --vote adds
compute_center_dists (train_vote.py:48-65: per frame a label count, a full descending sort of the votes, a copy of the
selection to the host) against compute_center_dists_batch.

Per side: ms per step (--repeats medians over --calls steps after --warmup, torch.cuda.Event around the step, the step
ends in its own read-backs; min .. max over the repeats is the side's spread), kernel launches per step (torch.profiler
device events of one step) and host waits per step (counted where the step's code reads back).  The logits stand for
out.features of a batch of --batch frames of --voxels rows (defaults: the two Cfg-2 frames of tools/train_timing.py, 88 000
voxels each, 3 classes); a quarter of the labels are the ignore label.

  python tools/seg_criterion_timing.py [--batch 2] [--voxels 88000] [--classes 3] [--calls 20] [--vote] [--out FILE]
Each side runs in a child process of its own under --timeout seconds; the first failure stops the run.
  python tools/seg_criterion_timing.py --only fused      # one measurement, in this process
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WAITS = [0]


def reference_accuracies(out, labels, others):
    """train_segmentation.py:34-46, op for op"""
    WAITS[0] += len(others)  # one float(...) per frame
    return [float((out[oi["offset"][0]:oi["offset"][1]].max(1)[1] == labels[oi["offset"][0]:oi["offset"][1]]).sum())
            / (oi["offset"][1] - oi["offset"][0]) for oi in others]


def reference_center_dists(out, labels, coords, poses, others, quantization_size, ee_r, to_matrix):
    """train_vote.py:48-65 with utils/output.py:45-64 get_pred_center, op for op; coords and poses are the loader's host
    tensors, as in the trainer"""
    import torch

    results = []
    for i, oi in enumerate(others):
        lo, hi = oi["offset"]
        WAITS[0] += 1
        if (labels[lo:hi] == 1).sum().item() < 1:
            continue
        coords_ins = coords[lo:hi][:, 1:] * quantization_size
        pose_ins = poses[i]
        sel = out[lo:hi].clone().detach()[:, 1].sort(descending=True)[1][:8]
        WAITS[0] += 1
        center = coords_ins[sel.cpu().numpy()].mean(axis=0)
        center = center + torch.matmul(to_matrix(pose_ins[3:].view(1, -1))[0], torch.tensor([-ee_r, 0, 0]))
        results.append(torch.linalg.norm(center - pose_ins[:3], ord=2).item())
    return results


def measure(side, args):
    import numpy as np
    import torch

    import mrcc_amd
    from mrcc_amd.utils.loss import SegmentationCriterion
    from mrcc_amd.utils.metrics import compute_center_dists_batch
    from mrcc_amd.utils.transformation import get_quaternion_rotation_matrix_torch

    mrcc_amd._lib.load()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    B, C = args.batch, args.classes
    lengths = (args.voxels * rng.uniform(0.9, 1.1, B)).astype(np.int64)
    bounds = np.concatenate([[0], np.cumsum(lengths)])
    N = int(bounds[-1])
    others = [{"offset": (int(lo), int(hi))} for lo, hi in zip(bounds[:-1], bounds[1:])]
    logits = torch.from_numpy(rng.normal(0, 3, size=(N, C)).astype(np.float32)).to(dev)
    lab = rng.integers(0, C, size=N)
    lab[rng.uniform(size=N) < 0.25] = -100
    labels = torch.from_numpy(lab).to(dev)
    coords = torch.from_numpy(np.concatenate([np.repeat(np.arange(B), lengths)[:, None],
                                              rng.integers(-60, 60, size=(N, 3))], 1).astype(np.int32))
    poses = torch.from_numpy(np.concatenate([rng.uniform(-1, 1, (B, 3)), rng.normal(size=(B, 4))], 1).astype(np.float32))
    qs, ee_r = 0.02, 0.03
    fused = SegmentationCriterion(ignore_index=-100, reduction="mean")
    plain = torch.nn.CrossEntropyLoss(ignore_index=-100, reduction="mean")
    coords_dev, poses_dev = coords.to(dev), poses.to(dev)

    def step():
        x = logits.clone().requires_grad_(True)  # stands for out.features of the forward pass
        WAITS[0] = 0
        if side == "fused":
            loss, m = fused(x, labels, offsets=others, return_metrics=True)
            loss.backward()
            WAITS[0] += 2
            value, acc = loss.item(), m.to_host()["accuracies"]
            dists = None
            if args.vote:
                dist, valid = compute_center_dists_batch(x.detach(), labels, coords_dev, poses_dev, others, qs, ee_r)
                WAITS[0] += 1
                both = torch.stack([dist, valid.to(torch.float32)]).cpu().numpy()
                dists = both[0][both[1] > 0]
        else:
            loss = plain(x, labels)
            loss.backward()
            WAITS[0] += 1
            value = loss.item()
            acc = reference_accuracies(x, labels, others)
            dists = None
            if args.vote:
                dists = reference_center_dists(x, labels, coords, poses, others, qs, ee_r,
                                               get_quaternion_rotation_matrix_torch)
        return value, float(np.mean(acc)), x.grad, dists

    for _ in range(args.warmup):
        first = step()
    torch.cuda.synchronize()
    medians = []
    for _ in range(args.repeats):
        ms = []
        for _ in range(args.calls):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            step()
            ev[1].record()
            torch.cuda.synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        medians.append(statistics.median(ms))
    waits = WAITS[0]
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        again = step()
        torch.cuda.synchronize()
    launches = sum(e.count for e in prof.key_averages() if e.device_time_total > 0)
    same = first[0] == again[0] and torch.equal(first[2], again[2])
    print(f"{side:5s} B={B} N={N} C={C}{' vote' if args.vote else ''}: {statistics.median(medians):8.3f} ms/step "
          f"(min {min(medians):.3f}, max {max(medians):.3f} over {args.repeats} repeats of {args.calls} steps)  "
          f"{launches:4d} launches/step  {waits:3d} host waits/step  loss {again[0]:.6g}  accuracy {again[1]:.6g}"
          + (f"  center_dist {float(np.mean(again[3])):.6g}" if args.vote and len(again[3]) else "")
          + f"  same bits twice: {same}")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--voxels", type=int, default=88000)
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vote", action="store_true", help="add compute_center_dists (train_vote.py)")
    ap.add_argument("--timeout", type=int, default=120)
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    ap.add_argument("--only", default=None, help="fused or torch: measure in this process")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats: at least 5 (the torch side's min .. max over them is the spread the comparison uses)")
    if args.only:
        measure(args.only, args)
        return 0
    lines = [f"# criterion forward + backward and step metrics, B = {args.batch} frames of about {args.voxels} rows, "
             f"{args.classes} classes, reduction mean{', with center distances' if args.vote else ''}; "
             f"{args.repeats} x {args.calls} timed steps after {args.warmup}"]
    print(lines[0])
    sys.stdout.flush()
    for side in ("fused", "torch"):
        cmd = [sys.executable, os.path.abspath(__file__), "--only", side, "--batch", str(args.batch), "--voxels",
               str(args.voxels), "--classes", str(args.classes), "--calls", str(args.calls), "--repeats", str(args.repeats),
               "--warmup", str(args.warmup)] + (["--vote"] if args.vote else [])
        try:
            done = subprocess.run(cmd, timeout=args.timeout, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print(f"{side}: no result within {args.timeout} s; stopping")
            return 124
        sys.stdout.write(done.stdout)
        sys.stdout.flush()
        lines.append(done.stdout.rstrip("\n"))
        if done.returncode != 0:  # a failed measurement ends the run: nothing more is started on the device
            print(f"{side}: exit status {done.returncode}; stopping")
            return done.returncode
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
