"""Training-step timing of RobotNetSegmentation(MinkUNet18D) on the autograd path (nn.SparseConvFunction).

Cfg-1 (80 000-point room, L = 1.5 m) and Cfg-2 (200 000 points, L = 2.4 m), 2 cm voxels, one frame and two frames in one
sparse tensor.  Reports per step: forward / backward / optimizer ms (CUDA events), peak GPU memory, and per conv / linear
layer the sv_conv_wgrad time with its TFLOP/s and share of the 157.3 TFLOP/s fp32 matrix peak beside the same layer's
forward kernel; then the cross-entropy loss over a short Adam run on synth.gen_scene frames.  Random-init weights.
--precision fp32,bf16 runs each training precision (nn.set_training_precision) in the same process; bf16 ops are rated
against the 2516.6 TFLOP/s bf16 matrix peak, fp32 ones against the fp32 peak.
Usage: python tools/train_timing.py [--steps N] [--precision fp32,bf16] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mrcc_amd  # noqa: E402
from mrcc_amd import MinkowskiEngine as ME  # noqa: E402
from mrcc_amd import nn as svnn  # noqa: E402
from mrcc_amd.model.robotnet_segmentation import RobotNetSegmentation  # noqa: E402

PEAK_FP32_MATRIX = 157.3e12
PEAK_BF16_MATRIX = 16 * PEAK_FP32_MATRIX
dev = torch.device("cuda:0")
LOG = []  # (kind, K, Cin, Cout, pairs (device scalar or int), start event, end event, bf16, layer key)
_IN_BACKWARD = [False]
_LAYER = [None]  # autograd context of the layer whose op runs (forward and backward share it)
_orig_forward, _orig_wgrad = svnn.conv_forward, svnn.conv_wgrad
_orig_fn_forward, _orig_backward = svnn.SparseConvFunction.forward, svnn.SparseConvFunction.backward


def _pairs(plan, rows):
    return plan.pairs_device() if plan is not None else rows


def _timed_forward(feats, weight3, plan, V_out, *a, **kw):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = _orig_forward(feats, weight3, plan, V_out, *a, **kw)
    e1.record()
    K, Cin, Cout = weight3.shape
    LOG.append(("dgrad" if _IN_BACKWARD[0] else "fwd", K, Cin, Cout, _pairs(plan, V_out), e0, e1,
                kw.get("weight_bf16") is not None, _LAYER[0]))
    return out


def _timed_wgrad(feats, dy, plan, K, Cin, Cout, bf16=False, used=None):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    used = set() if used is None else used
    e0.record()
    out = _orig_wgrad(feats, dy, plan, K, Cin, Cout, bf16=bf16, used=used)
    e1.record()
    LOG.append(("wgrad", K, Cin, Cout, _pairs(plan, dy.shape[0]), e0, e1, "sv_conv_wgrad_bf16" in used, _LAYER[0]))
    return out


def _flagged_forward(ctx, *a):
    _LAYER[0] = id(ctx)
    return _orig_fn_forward(ctx, *a)


def _flagged_backward(ctx, dy):
    _IN_BACKWARD[0] = True
    _LAYER[0] = id(ctx)
    try:
        return _orig_backward(ctx, dy)
    finally:
        _IN_BACKWARD[0] = False


def frames_for(cfg, n):
    pts_n, L = {"Cfg-1": (80_000, 1.5), "Cfg-2": (200_000, 2.4)}[cfg]
    out = []
    for s in range(n):
        pts, rgb, _ = mrcc_amd.synth.gen_room(pts_n, L, s)
        c4 = np.concatenate([np.full((len(pts), 1), s, np.float32), pts * np.float32(50)], axis=1)
        out.append((c4, rgb))
    c4 = torch.from_numpy(np.concatenate([f[0] for f in out]))
    rgb = torch.from_numpy(np.concatenate([f[1] for f in out]))
    return c4, rgb


def step_timing(model, opt, c4, rgb, steps, lines):
    def one(record):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        field = ME.TensorField(rgb, c4, device=dev)
        x = field.sparse()
        labels = torch.randint(0, 3, (x.F.shape[0],), device=dev)
        ev[0].record()
        out = model(x)
        loss = torch.nn.functional.cross_entropy(out.F, labels)
        ev[1].record()
        opt.zero_grad()
        loss.backward()
        ev[2].record()
        opt.step()
        ev[3].record()
        return ev, x.F.shape[0]

    for _ in range(2):
        one(False)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    LOG.clear()
    svnn.conv_forward, svnn.conv_wgrad = _timed_forward, _timed_wgrad
    svnn.SparseConvFunction.forward = staticmethod(_flagged_forward)
    svnn.SparseConvFunction.backward = staticmethod(_flagged_backward)
    evs = []
    V = 0
    t0 = time.perf_counter()
    for i in range(steps):
        if i == steps - 1:
            LOG.clear()  # per-layer table of the last step only
        ev, V = one(True)
        evs.append(ev)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps * 1e3
    svnn.conv_forward, svnn.conv_wgrad = _orig_forward, _orig_wgrad
    svnn.SparseConvFunction.forward = staticmethod(_orig_fn_forward)
    svnn.SparseConvFunction.backward = staticmethod(_orig_backward)
    fwd = np.mean([e[0].elapsed_time(e[1]) for e in evs])
    bwd = np.mean([e[1].elapsed_time(e[2]) for e in evs])
    optm = np.mean([e[2].elapsed_time(e[3]) for e in evs])
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    lines.append(f"  voxels {V}: step {fwd + bwd + optm:.2f} ms (wall {wall:.2f}) = forward {fwd:.2f} + backward {bwd:.2f} "
                 f"+ optimizer {optm:.2f} ms; backward / forward {bwd / fwd:.2f}; peak memory {peak:.2f} GiB")
    # per-layer table: forward, input gradient and weight gradient of each layer (keyed by its autograd context)
    layers = {}
    for kind, K, Cin, Cout, p, e0, e1, bf16, key in LOG:
        if kind == "dgrad":
            Cin, Cout = Cout, Cin
        row = layers.setdefault(key, {"shape": (K, Cin, Cout), "pairs": int(p.item()) if torch.is_tensor(p) else int(p)})
        t = row.get(kind, (0.0, bf16))
        row[kind] = (t[0] + e0.elapsed_time(e1), bf16)

    def rate(flops, ms, bf16):
        tf = flops / ms / 1e9
        return f"{ms:7.3f} {tf:6.1f} {100 * tf * 1e12 / (PEAK_BF16_MATRIX if bf16 else PEAK_FP32_MATRIX):5.1f}{'b' if bf16 else 'f'}"

    tot = {k: sum(r[k][0] for r in layers.values() if k in r) for k in ("fwd", "dgrad", "wgrad")}
    lines.append(f"  conv/linear kernels: forward {tot['fwd']:.2f} ms, input gradient {tot['dgrad']:.2f} ms, "
                 f"weight gradient {tot['wgrad']:.2f} ms")
    lines.append("  layer (K Cin->Cout, pairs)      fwd: ms  TF/s  %peak | dX: ms  TF/s  %peak | dW: ms  TF/s  %peak"
                 "  (b = bf16 kernel, share of the bf16 peak; f = fp32)")
    order = sorted(layers.values(), key=lambda r: -sum(r[k][0] for k in ("fwd", "dgrad", "wgrad") if k in r))
    for r in order[:14]:
        K, Cin, Cout = r["shape"]
        fl = 2.0 * r["pairs"] * Cin * Cout
        cols = [rate(fl, *r[k]) if k in r else f"{'-':>7s} {'-':>6s} {'-':>6s}" for k in ("fwd", "dgrad", "wgrad")]
        lines.append(f"  k{K:<2d} {Cin:4d}->{Cout:<4d} {r['pairs']:9d}   " + " | ".join(cols))


def loss_run(steps, lines, precision):
    torch.manual_seed(0)
    model = RobotNetSegmentation(in_channels=3, num_classes=3).to(dev).train()
    svnn.set_training_precision(model, precision)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    crit = torch.nn.CrossEntropyLoss(ignore_index=-100)
    batch = []
    for s in range(2):
        sc = mrcc_amd.synth.gen_scene(s, keyed_colors=True)
        c, f, lab = ME.utils.sparse_quantize(sc["points"], sc["rgb"], labels=sc["segmentation"], quantization_size=0.02)
        batch.append((torch.from_numpy(np.asarray(c)), np.asarray(f), np.asarray(lab)))
    coords = ME.utils.batched_coordinates([b[0] for b in batch])
    feats = torch.from_numpy(np.concatenate([b[1] for b in batch]).astype(np.float32))
    labels = torch.from_numpy(np.concatenate([b[2] for b in batch]).astype(np.int64)).to(dev)
    losses = []
    for _ in range(steps):
        out = model(ME.SparseTensor(feats, coordinates=coords, device=dev))
        opt.zero_grad()
        loss = crit(out.F, labels)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    lines.append(f"{precision} loss over {steps} Adam steps (lr 1e-3) on 2 gen_scene frames ({feats.shape[0]} voxels): "
                 + " ".join(f"{v:.3f}" for v in losses))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--cfgs", default="Cfg-1,Cfg-2")
    ap.add_argument("--loss-steps", type=int, default=20)
    ap.add_argument("--precision", default="fp32", help="training precisions to run, comma-separated: fp32, bf16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    precisions = args.precision.split(",")
    lines = [f"train_timing: RobotNetSegmentation(MinkUNet18D), {' and '.join(precisions)} training, Adam; "
             f"{torch.cuda.get_device_name(0)}"]
    for precision in precisions:
        torch.manual_seed(0)
        model = RobotNetSegmentation(in_channels=3, num_classes=3).to(dev).train()
        marked = svnn.set_training_precision(model, precision)
        opt = torch.optim.Adam(model.parameters(), lr=1e-4)
        lines.append(f"== {precision} training ({len(marked)} layers marked)")
        for cfg in args.cfgs.split(","):
            for n in (1, 2):
                c4, rgb = frames_for(cfg, n)
                lines.append(f"{cfg}, {n} frame{'s' if n > 1 else ''} in one tensor, {precision}:")
                step_timing(model, opt, c4, rgb, args.steps, lines)
                print("\n".join(lines[-18:]), flush=True)
        del model, opt
        torch.cuda.empty_cache()
    for precision in precisions:
        loss_run(args.loss_steps, lines, precision)
        print(lines[-1])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
