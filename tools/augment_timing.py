"""A training batch from host frames: the device builder (utils.augmentation.augment_quantize_batch: sv_elastic_field,
sv_augment_points, sv_quantise_points, sv_voxelize) against the reference's host data path restated below (per frame:
augment_segmentation with scipy, center_at_origin, ME.utils.sparse_quantize; then collate and the copy to the device;
utils/augmentation.py:108-138, data/alivev2.py:199-208,290-296,358-365).

B frames of Cfg-2 size (synth.gen_room, 200 000 points each), every augmentation firing.  Per side: wall-clock ms per
batch from host arrays in to device tensors out (median over --calls after --warmup, device synchronised at both ends;
the random draws are part of the batch and are timed), and kernel launches per batch (torch.profiler device events of
one batch).  No speed-up is asserted anywhere; the sides draw from different generators, so their batches differ.

  python tools/augment_timing.py [--batch 4] [--points 200000] [--scale 200] [--calls 10] [--warmup 2]
Every side runs in a child process of its own under --timeout seconds; the first failure stops the run.
  python tools/augment_timing.py --only device      # one measurement, in this process
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLAGS = dict(elastic=True, noise=True, transform=True, flip=True, gravity=True)


def host_distort_elastic(x, gran, mag):
    """the elastic distortion of utils/augmentation.py:14-33 with the same scipy calls (np.random draws)"""
    import numpy as np
    import scipy.interpolate
    import scipy.ndimage

    blurs = [np.ones(s).astype("float32") / 3 for s in ((3, 1, 1), (1, 3, 1), (1, 1, 3))]
    bb = np.abs(x).max(0).astype(np.int32) // gran + 3
    noise = [np.random.randn(bb[0], bb[1], bb[2]).astype("float32") for _ in range(3)]
    for k in blurs + blurs:
        noise = [scipy.ndimage.convolve(n, k, mode="constant", cval=0) for n in noise]
    ax = [np.linspace(-(b - 1) * gran, (b - 1) * gran, b) for b in bb]
    interp = [scipy.interpolate.RegularGridInterpolator(ax, n, bounds_error=0, fill_value=0) for n in noise]
    return x + np.hstack([i(x)[:, None] for i in interp]) * mag


def host_augment_segmentation(points, scale):
    """utils/augmentation.py:108-138 with every flag set and probability 1"""
    import numpy as np
    from scipy.stats import special_ortho_group

    p = np.array(points, copy=True)
    p = host_distort_elastic(p, 6 * scale // 50, 40 * scale / 50)
    p = host_distort_elastic(p, 20 * scale // 50, 160 * scale / 50)
    p = p + np.clip(0.0016 * np.random.randn(*p.shape), -0.005, 0.005)
    tr, rot = np.random.rand() * 0.04, special_ortho_group.rvs(3)
    p = (p @ rot + np.array([[tr, 0, 0]])) @ rot.T
    p = np.matmul(p, np.diag([float(np.random.randint(0, 2) * 2 - 1), 1.0, 1.0]))
    angle = np.random.rand() * 2 * np.pi
    c, s = np.cos(angle), np.sin(angle)
    return (np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]]) @ p.T).T


def measure(side, args):
    import numpy as np
    import torch

    import mrcc_amd
    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd.utils.augmentation import augment_quantize_batch

    mrcc_amd._lib.load()
    dev = torch.device("cuda:0")
    frames = [mrcc_amd.synth.gen_room(args.points, 2.4, seed) for seed in range(args.batch)]
    pts, feats, labels = [f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames]
    qsize = 1.0 / args.scale
    rng = np.random.default_rng(0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    np.random.seed(0)

    def device_batch():
        return augment_quantize_batch(pts, feats, labels, scale=args.scale, quantization_size=qsize, probability=1.0,
                                      center_at_origin=True, ignore_label=-100, rng=rng, generator=gen, device=dev,
                                      **FLAGS)

    def host_batch():
        cs, fs, ls = [], [], []
        for p, f, l in zip(pts, feats, labels):
            a = host_augment_segmentation(p, args.scale)
            a = a - (a.max(axis=0) + a.min(axis=0)) / 2
            c, uf, ul = ME.utils.sparse_quantize(coordinates=a, features=f, labels=l, quantization_size=qsize,
                                                 ignore_label=-100)
            cs.append(c), fs.append(uf), ls.append(ul)
        coords = ME.utils.batched_coordinates(cs)
        f_b = torch.from_numpy(np.concatenate(fs, 0)).to(dtype=torch.float32)
        l_b = torch.from_numpy(np.concatenate(ls, 0)).long()
        return coords.to(dev), f_b.to(dev), l_b.to(dev)

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
    print(f"{side:6s} B={args.batch} x {args.points} points, scale {args.scale}: {statistics.median(ms):9.2f} ms/batch "
          f"(min {min(ms):.2f})  {launches:4d} launches/batch  {out[0].shape[0]} voxels")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--scale", type=int, default=200)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-calls", type=int, default=3, help="timed batches of the host side (seconds each)")
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--only", default=None, help="device or host: measure in this process")
    args = ap.parse_args()
    if args.only:
        measure(args.only, args)
        return 0
    print(f"# one training batch, host frames in -> device tensors out: {args.batch} frames of {args.points} points, "
          f"scale {args.scale}, every augmentation firing, center_at_origin")
    sys.stdout.flush()
    for side in ("device", "host"):
        calls, warmup = (args.calls, args.warmup) if side == "device" else (args.host_calls, 1)
        cmd = [sys.executable, os.path.abspath(__file__), "--only", side, "--batch", str(args.batch), "--points",
               str(args.points), "--scale", str(args.scale), "--calls", str(calls), "--warmup", str(warmup)]
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
