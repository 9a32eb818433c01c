"""What a classification ResNet forward costs on the Cfg-2 cloud (bench.py's synthetic 200k-point room at 2 cm voxels), and what
the three kernel families added for it - strided coordinate / kernel maps, local pooling, instance normalisation - take of it.
Each measurement (network x batch size) runs in a child process of its own under `timeout`, one after the other; the first
that fails ends the run.

    python tools/resnet_timing.py [--steps 10] [--nets ResNet14,ResNet50,ResFieldNet14,ResFieldNet50] [--batches 1,4]

Per measurement: the first forward of a fresh tensor (it builds the coordinate maps, kernel maps and conv plans), the mean of
`--steps` further forwards on that tensor (maps cached), and, from one more cold and one more warm forward with a pair of
stream events around every library call, the device time inside the entries of each family.  eval(), random weights.
A ResFieldNet takes the TensorField itself and is measured twice, each time in a child of its own: with FUSE_FIELD on (each
field network one sv_field_stage call) and off (module by module); besides the whole forward it reports the two field
networks alone on a field that is already voxelised, and the device time inside sv_field_stage / sv_sinusoidal.
No figure is a pass condition: nothing comparable existed before these networks."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POINTS, ROOM, SCALE = 200_000, 2.4, 50  # bench.py's Cfg-2
LIMIT_S = 240
FAMILIES = {
    "maps": ("sv_stride_map_general", "sv_kernel_map_probe"),
    "pool": ("sv_pool_local", "sv_pool_local_backward"),
    "norm": ("sv_instance_norm", "sv_instance_norm_backward"),
    "field": ("sv_sinusoidal", "sv_field_stage"),
}


def make_input(batch, dev):
    import torch

    import mrcc_amd
    from mrcc_amd import MinkowskiEngine as ME

    parts = [mrcc_amd.synth.gen_room(POINTS, ROOM, b) for b in range(batch)]
    coords = np.concatenate([np.concatenate([np.full((len(p[0]), 1), b, np.float32), p[0] * np.float32(SCALE)], 1)
                             for b, p in enumerate(parts)])
    rgb = np.concatenate([p[1] for p in parts])
    field = ME.TensorField(torch.from_numpy(rgb), torch.from_numpy(coords),
                           quantization_mode=ME.SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE, device=dev)
    return field


class CallTimer:
    """stream events around every library call made through nn.call / sparse.call, and around sv_field_stage, which
    nn.field_stage calls on the library object itself (it reads the status); read after a synchronise"""

    def __init__(self):
        self.spans = []

    def __enter__(self):
        import torch

        from mrcc_amd import nn as svnn
        from mrcc_amd import sparse

        self.mods, self.orig = (svnn, sparse), svnn.call

        def timed(name, *args):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            self.orig(name, *args)
            b.record()
            self.spans.append((name, a, b))

        for m in self.mods:
            m.call = timed
        from mrcc_amd import _lib

        self.lib, self.stage = _lib.load(), _lib.load().sv_field_stage

        def timed_stage(*args):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = self.stage(*args)
            b.record()
            self.spans.append(("sv_field_stage", a, b))
            return rc

        self.lib.sv_field_stage = timed_stage
        return self

    def __exit__(self, *exc):
        for m in self.mods:
            m.call = self.orig
        self.lib.sv_field_stage = self.stage

    def by_family(self):
        import torch

        torch.cuda.synchronize()
        out = {f: [0.0, 0] for f in FAMILIES}
        out["conv / linear"], out["other"] = [0.0, 0], [0.0, 0]
        for name, a, b in self.spans:
            fam = next((f for f, names in FAMILIES.items() if name in names), None)
            if fam is None:
                fam = "conv / linear" if name.startswith("sv_conv") else "other"
            out[fam][0] += a.elapsed_time(b)
            out[fam][1] += 1
        return out


def child_field(net, batch, steps, fuse):
    """a ResFieldNet on the field: whole forwards (fresh field / voxelised field with cached maps), the two field networks
    alone, and the device time inside the library calls"""
    import torch

    from mrcc_amd.model.backbone import resnet

    dev = torch.device("cuda")
    torch.manual_seed(0)
    cls = getattr(resnet, net)
    cls.FUSE_FIELD = fuse
    model = cls(3, 10).to(dev).eval()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def front(f):
        return model._run_field(model.field_network2, f, model._run_field(model.field_network, f))

    with torch.no_grad():
        timed(lambda: model(make_input(batch, dev)))  # first use of every kernel: not reported
        field = make_input(batch, dev)
        cold_ms, out = timed(lambda: model(field))
        warm = [timed(lambda: model(field))[0] for _ in range(steps)]
        front_ms = [timed(lambda: front(field))[0] for _ in range(steps)]
        with CallTimer() as calls:
            timed(lambda: model(field))
        split = calls.by_family()
    cm = field.coordinate_manager
    assert out.shape == (batch, 10) and torch.isfinite(out).all()
    print(f"{net} B = {batch}, FUSE_FIELD = {fuse}, on {torch.cuda.get_device_name(0)}, torch {torch.__version__}: {len(field)} points, "
          f"{cm.maps[1].V} voxels")
    print(f"  forward, fresh field (voxelises, builds maps and plans): {cold_ms:.3f} ms; field voxelised, maps cached: "
          f"{np.mean(warm):.3f} ms (min {min(warm):.3f}, {steps} forwards)")
    print(f"  the two field networks alone, field voxelised: {np.mean(front_ms):.3f} ms (min {min(front_ms):.3f}, {steps} runs)")
    cells = ", ".join(f"{f} {ms:.3f} ms in {n} calls" for f, (ms, n) in split.items())
    print(f"  device time inside library calls, cached: {cells}")


def child(net, batch, steps):
    import torch

    from mrcc_amd.model.backbone import resnet

    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = getattr(resnet, net)(3, 10).to(dev).eval()
    field = make_input(batch, dev)

    def forward(x):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model(x)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    with torch.no_grad():
        forward(field.sparse())  # first use of every kernel: not reported
        x = field.sparse()
        cold_ms, out = forward(x)
        warm = [forward(x)[0] for _ in range(steps)]
        with CallTimer() as cold_calls:
            forward(field.sparse())
        cold_split = cold_calls.by_family()
        with CallTimer() as warm_calls:
            forward(x)
        warm_split = warm_calls.by_family()
    cm = x.coordinate_manager
    sizes = ", ".join(f"{s}: {m.V}" for s, m in sorted(cm.maps.items()))
    assert out.shape == (batch, 10) and torch.isfinite(out).all()
    print(f"{net} B = {batch} on {torch.cuda.get_device_name(0)}, torch {torch.__version__}: {x.F.shape[0]} voxels; voxels per tensor stride {{{sizes}}}")
    print(f"  forward, fresh tensor (builds maps and plans): {cold_ms:.3f} ms; maps cached: {np.mean(warm):.3f} ms "
          f"(min {min(warm):.3f}, {steps} forwards)")
    for label, split in (("fresh", cold_split), ("cached", warm_split)):
        cells = ", ".join(f"{f} {ms:.3f} ms in {n} calls" for f, (ms, n) in split.items())
        print(f"  device time inside library calls, {label}: {cells}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--nets", default="ResNet14,ResNet50")
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        net, batch, *fuse = args.child.split(":")
        if fuse:
            return child_field(net, int(batch), args.steps, fuse[0] == "fused")
        return child(net, int(batch), args.steps)
    print(f"# Cfg-2 cloud: {POINTS} points, {100 / SCALE:.0f} cm voxels; one run", flush=True)  # the GPU is opened by the children only
    for net in args.nets.split(","):
        for batch in args.batches.split(","):
            for mode in (("",) if not net.startswith("ResFieldNet") else (":fused", ":modules")):
                subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child",
                                f"{net}:{batch}{mode}", "--steps", str(args.steps)], check=True)


if __name__ == "__main__":
    main()
