"""PointNet++ training step timing: the "torch" and the "hip" training path (set_training_path) in one process.

Per network and path: forward / backward / optimizer (Adam) ms per step (median over --steps after two warm-up steps,
torch.cuda.Event around each phase), peak memory, whether two identical steps give identical gradient bits, and the top
kernels of one step by device time (torch.profiler).

  python tools/pointnet2_train_timing.py [--steps 10] [--batch 32] [--msg-batch 16] [--points 2048] [--paths torch,hip]
                                         [--nets ssg,msg] [--single-step]
--single-step: exactly one training step (forward, backward, Adam) per network and path after building the model, no
warm-up, timing or checks - the process to run under `rocprofv3 --kernel-trace --stats -- ...`.
SSG: PointNet2SSG(6, in_channels=6) on [B, 6, N] crops with CrossEntropyLoss over 6 classes (train_key_points.py);
MSG: PointNet2MSGEncoder(7) on [B, 6, N] with MSELoss (train.py)."""
import argparse
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import mrcc_amd  # noqa: E402
from mrcc_amd.model.pointnet2 import PointNet2MSGEncoder, PointNet2SSG, set_training_path  # noqa: E402


def build(net, B, N, dev):
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    xyz = torch.rand(B, 3, N, generator=g)
    if net == "ssg":
        m = PointNet2SSG(6, in_channels=6)
        x = torch.cat([xyz, xyz - 0.5], 1)
        y = torch.randint(0, 6, (B, N), generator=g)
        fps = torch.randint(0, N, (4, B), generator=g)
        loss = lambda out: nn.functional.cross_entropy(out.reshape(-1, 6), y_d.reshape(-1))  # noqa: E731
    else:
        m = PointNet2MSGEncoder(7)
        x = torch.cat([xyz, nn.functional.normalize(torch.randn(B, 3, N, generator=g), dim=1)], 1)
        y = torch.randn(B, 7, generator=g)
        fps = torch.randint(0, N, (2, B), generator=g)
        loss = lambda out: nn.functional.mse_loss(out, y_d)  # noqa: E731
    y_d = y.to(dev)
    return m.to(dev), x.to(dev), fps.to(dev), loss


def step(m, opt, x, fps, loss, ev=None):
    if ev:
        ev[0].record()
    out, _ = m(x, fps_starts=fps)
    lo = loss(out)
    if ev:
        ev[1].record()
    lo.backward()
    if ev:
        ev[2].record()
    if opt is not None:
        opt.step()
    if ev:
        ev[3].record()
    return lo


def run(net, path, args, dev):
    B = args.batch if net == "ssg" else args.msg_batch
    m, x, fps, loss = build(net, B, args.points, dev)
    set_training_path(m, path)
    m.train()
    if args.single_step:
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        step(m, opt, x, fps, loss)
        torch.cuda.synchronize()
        print(f"{net} B={B} N={args.points} path={path}: one training step")
        return
    # identical gradient bits: two steps from the same state, no optimizer step in between
    sd = copy.deepcopy(m.state_dict())
    grads = []
    for _ in range(2):
        m.load_state_dict(sd)
        m.zero_grad(set_to_none=True)
        torch.manual_seed(1)  # the same dropout masks
        step(m, None, x, fps, loss)
        grads.append([p.grad.clone() for p in m.parameters()])
    same = all(torch.equal(a, b) for a, b in zip(*grads))
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        step(m, opt, x, fps, loss)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fw, bw, op = [], [], []
    for _ in range(args.steps):
        opt.zero_grad(set_to_none=True)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        step(m, opt, x, fps, loss, ev)
        torch.cuda.synchronize()
        fw.append(ev[0].elapsed_time(ev[1]))
        bw.append(ev[1].elapsed_time(ev[2]))
        op.append(ev[2].elapsed_time(ev[3]))
    peak = torch.cuda.max_memory_allocated() / 2**20
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        opt.zero_grad(set_to_none=True)
        step(m, opt, x, fps, loss)
        torch.cuda.synchronize()
    kern = sorted(((e.key, e.device_time_total, e.count) for e in prof.key_averages() if e.device_time_total > 0),
                  key=lambda t: -t[1])
    med = statistics.median
    print(f"{net} B={B} N={args.points} path={path}: forward {med(fw):.2f} ms  backward {med(bw):.2f} ms  "
          f"optimizer {med(op):.2f} ms  step {med(fw) + med(bw) + med(op):.2f} ms  peak {peak:.0f} MiB  "
          f"identical gradient bits: {same}")
    total = sum(t for _, t, _ in kern)
    for name, t, c in kern[: args.top]:
        print(f"    {t / 1e3:8.3f} ms {100 * t / max(total, 1):5.1f}%  x{c:<4d} {name[:110]}")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--msg-batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--paths", default="torch,hip")
    ap.add_argument("--nets", default="ssg,msg")
    ap.add_argument("--top", type=int, default=12)
    ap.add_argument("--single-step", action="store_true")
    args = ap.parse_args()
    mrcc_amd._lib.load()
    dev = torch.device("cuda:0")
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {args.steps} timed steps after 2 warm-up")
    for net in args.nets.split(","):
        for path in args.paths.split(","):
            run(net, path, args, dev)


if __name__ == "__main__":
    main()
