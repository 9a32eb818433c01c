"""fp32 against the opt-in bf16 path (nn.set_compute_precision), in one process, on the seeded Cfg-2 frames (200k points,
2 cm, bench.build_model's weights):
  * the dominant layer (level 0, 384 -> 384, 3x3x3, three offset-range passes) at 1 and 4 frames per launch,
  * frames/s of the group-of-4, 3-stream frame pipeline (bench.run_frames),
  * bf16 TFLOP/s as a share of the 2.5 PF bf16 peak, and the label agreement of the bf16 network with fp32.
Features are random (BF16 loops on zeros hold a higher clock).
    python tools/precision_timing.py [--iters 100] [--steps 48]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import mrcc_amd  # noqa: E402
from mrcc_amd import MinkowskiEngine as ME  # noqa: E402
from mrcc_amd import nn as svnn  # noqa: E402
from mrcc_amd.app.pipeline import FramePipeline  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0
PEAK_FP32_MFMA_TFLOPS = 157.3

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--steps", type=int, default=48)
ap.add_argument("--group", type=int, default=4)
ap.add_argument("--streams", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda:0")
result = {}


def layer_times(frames):
    coords4 = torch.cat([f[0] for f in frames]).clone()
    for b in range(len(frames)):
        n = frames[0][0].shape[0]
        coords4[b * n:(b + 1) * n, 0] = b
    x = ME.TensorField(torch.cat([f[1] for f in frames]), coords4, device=dev).sparse()
    cm = x.coordinate_manager
    plan = cm.plan_k3_split(1, (9, 18))
    V = cm.stride_map(1).V
    pairs = sum(int(sub.num_pairs()) for _, _, sub in plan.parts)
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(V, 384, generator=g).to(dev)
    W = (torch.randn(27, 384, 384, generator=g) * 0.05).to(dev)
    wp = svnn.pack_weights_bf16(W)
    out = {}
    for prec, w in (("fp32", None), ("bf16", wp), ("fp32_again", None), ("bf16_again", wp)):
        for _ in range(3):
            svnn.conv_forward(feats, W, plan, V, weight_bf16=w)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(args.iters):
            svnn.conv_forward(feats, W, plan, V, weight_bf16=w)
        e.record()
        torch.cuda.synchronize()
        ms = s.elapsed_time(e) / args.iters
        out[prec] = {"ms": round(ms, 4), "tflops": round(2.0 * pairs * 384 * 384 / ms / 1e9, 1),
                     "instance": mrcc_amd._lib.conv_last_instance()[0]}
    out["bf16"]["share_of_bf16_peak"] = round(out["bf16"]["tflops"] / PEAK_BF16_TFLOPS, 4)
    out["fp32"]["share_of_fp32_peak"] = round(out["fp32"]["tflops"] / PEAK_FP32_MFMA_TFLOPS, 4)
    out["speedup_bf16"] = round(min(out["fp32"]["ms"], out["fp32_again"]["ms"]) /
                                min(out["bf16"]["ms"], out["bf16_again"]["ms"]), 3)
    out["voxels"] = V
    return out


with torch.no_grad():
    frames = [bench.make_frame(s, dev) for s in range(8)]
    result["layer_level0_384x384_1frame"] = layer_times(frames[:1])
    result["layer_level0_384x384_4frames"] = layer_times(frames[:4])
    model = bench.build_model(dev)
    # label agreement on frame 0
    f0 = frames[0]
    field = ME.TensorField(f0[1], f0[0], quantization_mode=ME.SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE, device=dev)
    ref = model(field.sparse())
    lab32, _ = ref.slice_argmax(field)
    svnn.set_compute_precision(model, "bf16")
    out = model(field.sparse())
    lab16, _ = out.slice_argmax(field)
    result["label_agreement"] = round((lab16 == lab32).double().mean().item(), 5)
    result["logits_rel_frobenius"] = round((torch.linalg.norm(out.F.double() - ref.F.double()) /
                                            torch.linalg.norm(ref.F.double())).item(), 5)
    pipe = FramePipeline(dev, levels=4, compute_streams=args.streams)
    fps = {}
    for prec in ("fp32", "bf16", "fp32", "bf16"):  # alternating, the better of two per precision
        svnn.set_compute_precision(model, prec)
        bench.run_frames(model, pipe, frames, 2 * args.group, group=args.group)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bench.run_frames(model, pipe, frames, args.steps, group=args.group)
        pipe.drain()
        torch.cuda.synchronize()
        fps[prec] = max(fps.get(prec, 0.0), args.steps / (time.perf_counter() - t0))
    result["pipeline_frames_per_s"] = {k: round(v, 2) for k, v in fps.items()}
    result["pipeline_speedup_bf16"] = round(fps["bf16"] / fps["fp32"], 3)
print(json.dumps(result))
