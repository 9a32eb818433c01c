"""Timing of PointNet2MSGEncoder (the reference's pointnet2 encode-only pose regressor) on [B, 6, 2048] clouds:
  * ms per eval forward from device events over warmed iterations, fused multi-scale layers (sv_pointnet_sa_msg) against
    the forced unfused path (PointNetSetAbstractionMsg.fused = False), for B = 1, 8, 32;
  * kernel launches per forward (torch profiler);
  * algorithmic GFLOP (shared-MLP and head matmuls, 2 * rows * Cin * Cout) over time, and that rate as a share of the
    fp32 matrix peak (157.3 TFLOP/s);
  * the launch choice of the multi-scale kernel: one launch over all scales against one launch per scale (the same entry
    called with R = 1, LDS sized for that scale), per layer.
Usage: python tools/pointnet2_msg_timing.py [--iters I] [--batches 1 8 32]"""
import argparse
import os
import sys
from ctypes import c_int, c_void_p

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mrcc_amd  # noqa: E402,F401
from mrcc_amd import _lib  # noqa: E402
from mrcc_amd.model import pointnet2_utils as P2  # noqa: E402
from mrcc_amd.model.pointnet2 import PointNet2MSGEncoder  # noqa: E402

PEAK_FP32 = 157.3e12
N = 2048


def flops(net, B):
    """2 * rows * Cin * Cout summed over every shared-MLP layer and the head"""
    total = 0
    for sa in (net.sa1, net.sa2):
        for K, convs in zip(sa.nsample_list, sa.conv_blocks):
            total += sum(2 * B * sa.npoint * K * c.in_channels * c.out_channels for c in convs)
    total += sum(2 * B * 128 * c.in_channels * c.out_channels for c in net.sa3.mlp_convs)
    total += sum(2 * B * fc.in_features * fc.out_features for fc in (net.fc1, net.fc2, net.fc3))
    return total


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def launches(fn):
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


def layer_launch_choice(sa, xyz, points, iters):
    """ms of one sv_pointnet_sa_msg launch over all scales vs one launch per scale (R = 1 each, own LDS size)"""
    x = xyz.permute(0, 2, 1).contiguous()
    p = points.permute(0, 2, 1).contiguous() if points is not None else None
    B, D = x.shape[0], (p.shape[2] if p is not None else 0)
    start = torch.zeros(B, dtype=torch.int64, device=x.device)
    nx = P2.index_points(x, P2.farthest_point_sample(x, sa.npoint, start=start)).contiguous()
    idxs = P2.query_ball_point_multi(sa.radius_list, sa.nsample_list, x, nx)
    folds = sa._folded()
    _, packed, _ = folds
    lib = _lib.load()
    outs = [torch.empty((B, sa.npoint, c[-1].out_channels), device=x.device) for c in sa.conv_blocks]
    singles = []
    for r, convs in enumerate(sa.conv_blocks):
        w = [convs[0].in_channels] + [c.out_channels for c in convs]
        singles.append(((c_int * 1)(sa.nsample_list[r]), (c_void_p * 1)(idxs[r].data_ptr()),
                        (c_void_p * 1)(packed[r].data_ptr()), (c_int * len(w))(*w), (c_int * 1)(len(convs))))

    def per_scale():
        for (ns, ix, pr, w, nl), o in zip(singles, outs):
            rc = lib.sv_pointnet_sa_msg(_lib.ptr(x), _lib.ptr(p), _lib.ptr(nx), B, x.shape[1], D, sa.npoint, 1, ns, ix,
                                        pr, w, nl, _lib.ptr(o), _lib.stream_ptr())
            _lib._check(rc, "sv_pointnet_sa_msg")

    return (timed(lambda: sa._fused(x, p, nx, idxs, folds), iters), timed(per_scale, iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = PointNet2MSGEncoder(7).to(dev).eval()
    for B in args.batches:
        x = torch.cat([torch.rand(B, 3, N, device=dev) - 0.5, torch.rand(B, 3, N, device=dev) * 2 - 1], dim=1)
        starts = torch.stack([torch.randint(0, n, (B,), device=dev) for n in (N, 512)])
        gflop = flops(net, B) / 1e9
        res = {}
        with torch.no_grad():
            for fused in (True, False):
                net.sa1.fused = net.sa2.fused = fused
                fn = lambda: net(x, fps_starts=starts)  # noqa: E731
                ms = timed(fn, args.iters)
                res[fused] = (ms, launches(fn))
            net.sa1.fused = net.sa2.fused = True
            for fused in (True, False):
                ms, n = res[fused]
                rate = gflop / ms  # GFLOP per ms = TFLOP/s
                print(f"B = {B:2d} {'fused  ' if fused else 'unfused'}: {ms:8.3f} ms/forward, {n:4d} launches, "
                      f"{gflop:7.1f} GFLOP, {rate:6.2f} TFLOP/s = {100 * rate * 1e12 / PEAK_FP32:5.1f} % of fp32 peak")
            print(f"B = {B:2d} fused / unfused: {res[True][0] / res[False][0]:.3f}")
            l1_xyz, l1 = net.sa1(x[:, :3], x[:, 3:], fps_start=starts[0])
            for name, sa, xyz, pts in (("sa1", net.sa1, x[:, :3], x[:, 3:]), ("sa2", net.sa2, l1_xyz, l1)):
                one, per = layer_launch_choice(sa, xyz, pts, args.iters)
                print(f"B = {B:2d} {name}: one launch over the scales {one:.3f} ms, one launch per scale {per:.3f} ms")


if __name__ == "__main__":
    main()
