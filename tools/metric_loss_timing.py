"""The criterion of a feature-extractor training step (train_feature-extractor.py:65-81), forward and backward: this
build (utils.metric_learning.mined_triplet_loss: one sv_mined_triplet_step call) against a torch restatement of what
pytorch_metric_learning does per step on the same GPU tensors - the cosine matrix, two masked copies, two row sorts, two
torch.where, the two len() the trainer takes, truncation and randperm, convert_to_triplets' [P, N] comparison and its
torch.where, the distance matrix and the mean over the non-zero triplets.  The library itself is not available; the
restatement is the one of tests/metric_helpers.py, in torch on the device.

Per side: ms per step (--repeats medians over --calls steps after --warmup, torch.cuda.Event around the step, which ends in
loss.item() as the trainer's does), kernel launches per step (torch.profiler device events of one step), host waits per step
(counted where the step's code reads back or calls an operator whose result size is data dependent) and the peak of
torch.cuda.max_memory_allocated over a step.  The embeddings stand for out.features of --batch frames: unit normal rows of
--dim floats around one centre per class, --classes classes.
The third side, `pool`, is the Python loop of nn.global_pool_train (one slice and one mean per frame, existing behaviour) on
--batch frames of --voxels rows, forward and backward: what the step pays just before the criterion.

  python tools/metric_loss_timing.py [--batch 256] [--dim 512] [--classes 16] [--max-pairs 131072] [--out FILE]
Each side runs in a child process of its own under --timeout seconds; the first failure stops the run.
  python tools/metric_loss_timing.py --only fused      # one measurement, in this process
"""
import argparse
import os
import statistics
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WAITS = [0]


def library_step(x, labels, max_pairs, epsilon, margin):
    """the library's steps in torch, op for op as far as memory of it goes; -> loss"""
    import torch

    u = torch.nn.functional.normalize(x, dim=1)
    mat = u @ u.t()
    same = labels[:, None] == labels[None, :]
    eye = torch.eye(len(labels), dtype=torch.bool, device=x.device)
    pos_mask, neg_mask = same & ~eye, ~same
    WAITS[0] += 2  # get_all_pairs_indices: two torch.where
    a1_all, _ = torch.where(pos_mask)
    a2_all, _ = torch.where(neg_mask)
    if len(a1_all) == 0 or len(a2_all) == 0:
        return x.sum() * 0
    mat_pos = mat.masked_fill(~pos_mask, float("inf"))
    mat_neg = mat.masked_fill(~neg_mask, float("-inf"))
    pos_sorted, pos_idx = torch.sort(mat_pos, dim=1)
    neg_sorted, neg_idx = torch.sort(mat_neg, dim=1)
    WAITS[0] += 2
    hard_pos = torch.where(pos_sorted - epsilon < neg_sorted[:, -1:])
    hard_neg = torch.where(neg_sorted + epsilon > pos_sorted[:, :1])
    a1, p = hard_pos[0], pos_idx[hard_pos[0], hard_pos[1]]
    a2, n = hard_neg[0], neg_idx[hard_neg[0], hard_neg[1]]
    # the trainer: len() of both lists (sizes are known on the host after torch.where), truncation, randperm
    pos_perm, neg_perm = torch.randperm(min(len(a1), max_pairs)), torch.randperm(min(len(a2), max_pairs))
    a1, p, a2, n = a1[pos_perm], p[pos_perm], a2[neg_perm], n[neg_perm]
    WAITS[0] += 1  # convert_to_triplets: torch.where on [P, N]
    pi, ni = torch.where(a1.unsqueeze(1) == a2)
    a, pp, nn_ = a1[pi], p[pi], n[ni]
    dist = torch.cdist(u, u)
    viol = torch.relu(dist[a, pp] - dist[a, nn_] + margin)
    nonzero = (viol > 0).sum()
    return viol.sum() / nonzero.clamp(min=1)


def measure(side, args):
    import numpy as np
    import torch

    import mrcc_amd
    from mrcc_amd import nn as svnn
    from mrcc_amd.utils.metric_learning import mined_triplet_loss

    mrcc_amd._lib.load()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    B, E = args.batch, args.dim
    lab = rng.integers(0, args.classes, size=B)
    centres = rng.standard_normal((args.classes, E))
    emb = torch.from_numpy((centres[lab] * 0.5 + rng.standard_normal((B, E))).astype(np.float32)).to(dev)
    labels = torch.from_numpy(lab.astype(np.int32)).to(dev)  # int32: the YCB collate's dtype
    bounds = [b * args.voxels for b in range(B + 1)]
    rows = torch.randn(bounds[-1], E, device=dev) if side == "pool" else None
    pooled_in = types.SimpleNamespace(tensor_stride=1, coordinate_manager=types.SimpleNamespace(batch_bounds=lambda s: bounds))

    def step():
        WAITS[0] = 0
        if side == "pool":
            pooled_in.F = rows.clone().requires_grad_(True)
            out = svnn.global_pool_train(pooled_in, mrcc_amd._lib.SV_POOL_AVG)
            out.sum().backward()
            WAITS[0] += 1
            return float(out[0, 0].detach()), pooled_in.F.grad
        x = emb.clone().requires_grad_(True)  # stands for out.features of the forward pass
        if side == "fused":
            loss = mined_triplet_loss(x, labels, args.max_pairs, args.epsilon, args.margin)
        else:
            loss = library_step(x, labels, args.max_pairs, args.epsilon, args.margin)
        loss.backward()
        WAITS[0] += 1
        return loss.item(), x.grad

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
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2**20
    waits = WAITS[0]
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        again = step()
        torch.cuda.synchronize()
    launches = sum(e.count for e in prof.key_averages() if e.device_time_total > 0)
    same = first[0] == again[0] and torch.equal(first[1], again[1])
    what = f"B={B} frames of {args.voxels} rows, C={E}" if side == "pool" else f"B={B} E={E} classes={args.classes} max_pairs={args.max_pairs}"
    print(f"{side:5s} {what}: {statistics.median(medians):8.3f} ms/step (min {min(medians):.3f}, max {max(medians):.3f} over "
          f"{args.repeats} repeats of {args.calls} steps)  {launches:5d} launches/step  {waits:2d} host waits/step  "
          f"peak {peak:8.1f} MiB above the inputs  value {again[0]:.6g}  same bits twice: {same}")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--max-pairs", type=int, default=131072)
    ap.add_argument("--epsilon", type=float, default=0.1)
    ap.add_argument("--margin", type=float, default=0.05)
    ap.add_argument("--voxels", type=int, default=300, help="rows per frame of the pooling side")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=150)
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    ap.add_argument("--only", default=None, help="fused, torch or pool: measure in this process")
    args = ap.parse_args()
    if args.only:
        measure(args.only, args)
        return 0
    lines = [f"# criterion of the feature-extractor step, forward + backward + loss.item(): B = {args.batch}, E = {args.dim}, "
             f"{args.classes} classes, max_pairs = {args.max_pairs}, epsilon = {args.epsilon}, margin = {args.margin}; "
             f"{args.repeats} x {args.calls} timed steps after {args.warmup}; pool = nn.global_pool_train alone"]
    print(lines[0])
    sys.stdout.flush()
    for side in ("fused", "torch", "pool"):
        cmd = [sys.executable, os.path.abspath(__file__), "--only", side]
        for k in ("batch", "dim", "classes", "max_pairs", "epsilon", "margin", "voxels", "calls", "repeats", "warmup"):
            cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
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
