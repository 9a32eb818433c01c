"""Timing of the `pointnet2` key-point stage (KEY_POINTS.backbone = "pointnet2", the reference's shipped configuration):
  * per-crop key-point time: the per-frame predict_key_points (host draw, one forward, host selection) against the
    batched enqueue (_pointnet_kp_enqueue: G crops, one forward, device selection) for G = 1, 4, 16;
  * kernel launches per PointNet2SSG forward (torch profiler, B = 1);
  * predict_stream frames/s (group 4) with the pointnet2 configuration.
Usage: python tools/pointnet2_timing.py [--reps R]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mrcc_amd  # noqa: E402
from mrcc_amd.app.dto import PointCloudDTO  # noqa: E402
from mrcc_amd.app.inference_engine import InferenceEngine  # noqa: E402
from mrcc_amd.utils import preprocess  # noqa: E402
from mrcc_amd.utils.config import Config  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    Config.reset()
    Config().update({"INFERENCE": {"SEGMENTATION": {"scale": 50}, "ROTATION": {"scale": 100},
                                   "KEY_POINTS": {"backbone": "pointnet2", "conf_threshold": 0.0},
                                   "ee_point_counts_threshold": 64, "SANITY": {"min_num_of_ee_points": 64}}})
    eng = InferenceEngine(allow_random_init=True, seed=3)
    mrcc_amd.synth.wire_color_keyed_labels(eng._segmentation_model)
    scenes = [mrcc_amd.synth.gen_scene(s, n_bg=20000, n_arm=2000, n_ee=3000 + 100 * s, keyed_colors=True)
              for s in range(16)]
    crops = [(sc["points"][sc["segmentation"] == 2], preprocess.normalize_colors(sc["rgb"])[sc["segmentation"] == 2])
             for sc in scenes]
    th = 0.75

    def per_frame(k):
        for p, c in crops[:k]:
            eng.predict_key_points(p, torch.from_numpy(c).to(torch.float32), conf_th=th)

    def batched(k):
        host, ev, _ = eng._pointnet_kp_enqueue([p for p, _ in crops[:k]], [c for _, c in crops[:k]], th)
        ev.synchronize()

    def timed(fn, k):
        for _ in range(3):
            fn(k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn(k)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.reps / k * 1e3

    print(f"per-frame predict_key_points: {timed(per_frame, 4):.3f} ms per crop")
    for k in (1, 4, 16) if hasattr(eng, "_pointnet_kp_enqueue") else ():
        print(f"batched G = {k:2d}: {timed(batched, k):.3f} ms per crop")
    # launches per forward
    net = eng._key_points_model
    x = torch.rand(1, 6, 2048, device="cuda") * 0.2
    with torch.no_grad():
        net(x)
        torch.cuda.synchronize()
        try:
            from torch.profiler import ProfilerActivity, profile

            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                net(x)
                torch.cuda.synchronize()
            n = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
            print(f"kernel launches per PointNet2SSG forward (B = 1): {n}")
        except Exception as e:  # the profiler is optional here
            print(f"kernel launches per forward: profiler unavailable ({type(e).__name__}: {e})")
    # streamed frames/s
    dtos = [PointCloudDTO(points=sc["points"], rgb=sc["rgb"], ee2base_pose=sc["ee2base_pose"]) for sc in scenes]
    list(eng.predict_stream(iter(dtos[:4]), group=4))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = list(eng.predict_stream(iter(dtos), group=4))
    dt = time.perf_counter() - t0
    print(f"predict_stream (group 4, pointnet2 key points): {len(out) / dt:.1f} frames/s over {len(out)} frames")
    t0 = time.perf_counter()
    for d in dtos:
        eng.predict(d)
    dt = time.perf_counter() - t0
    print(f"per-frame predict (pointnet2 key points): {len(dtos) / dt:.1f} frames/s")


if __name__ == "__main__":
    main()
