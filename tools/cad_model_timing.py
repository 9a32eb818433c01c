"""Time of building the ICP model from a mesh file (utils/mesh.py on sv_mesh_sample and sv_sample_eliminate) at the
reference's size: 16384 surface samples thinned to 8192.  Each measurement runs in a child process of its own, one after
the other.

    python tools/cad_model_timing.py [--mesh tests/golden/hand_notblender.obj] [--sections sample,table,loop,startup]

sample:  ms of one sv_mesh_sample call (16384 samples).
table:   ms of one sv_sample_eliminate call with n_keep = N: the neighbour table, the initial weights and the write-out,
         no deletion.
loop:    ms of one sv_sample_eliminate call 16384 -> 8192; less `table` it is the 8192 deletions.
startup: wall-clock ms of load_cad_model(mesh) in a fresh process, file parsing and read-backs included: what an engine
         with a cad_name adds to its start-up (first call, then a second one in the same process).
The launches per call do not depend on the sizes: sv_mesh_sample enqueues one memset and three kernels, sv_sample_eliminate
one memset and two kernels (table, then the one workgroup that runs the whole loop)."""
import argparse
import os
import subprocess
import sys
import time
from ctypes import c_double, c_int, c_int64, c_size_t

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECTIONS = ("sample", "table", "loop", "startup")
N_INIT, N_KEEP = 16384, 8192


def timed(fn, reps=10, warmup=3):
    """ms per call between two stream events"""
    import torch

    for _ in range(warmup):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def sample(mesh_path):
    import torch

    from mrcc_amd import _lib
    from mrcc_amd._lib import call, ptr, stream_ptr
    from mrcc_amd.utils.mesh import read_triangle_mesh

    mesh = read_triangle_mesh(mesh_path)
    dev = torch.device("cuda")
    verts, tris = torch.as_tensor(mesh.vertices).to(dev), torch.as_tensor(mesh.triangles).to(dev)
    draws = torch.as_tensor(np.random.default_rng(0).random((N_INIT, 3))).to(dev)
    F = tris.shape[0]
    ws_bytes = _lib.load().sv_mesh_sample_workspace_bytes(c_int64(F))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    points, normals = (torch.empty((N_INIT, 3), dtype=torch.float64, device=dev) for _ in range(2))
    tri = torch.empty(N_INIT, dtype=torch.int32, device=dev)
    area = torch.empty(1, dtype=torch.float64, device=dev)
    counters = torch.empty(1, dtype=torch.int32, device=dev)
    ms = timed(lambda: call("sv_mesh_sample", ptr(verts), c_int64(verts.shape[0]), ptr(tris), c_int64(F), ptr(draws),
                            c_int64(N_INIT), ptr(ws), c_size_t(ws_bytes), ptr(points), ptr(normals), ptr(tri), ptr(area),
                            ptr(counters), stream_ptr()))
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, 10 timed calls after 3 warm-up")
    print(f"sample:  sv_mesh_sample, {F} triangles, {N_INIT} samples: {ms:.3f} ms per call (area {area.item():.9f} m^2)")


def eliminate(mesh_path, n_keep, label):
    import torch

    from mrcc_amd import _lib
    from mrcc_amd._lib import call, ptr, stream_ptr
    from mrcc_amd.utils.mesh import DEFAULT_DEGREE, eliminate_radii, read_triangle_mesh

    pcl = read_triangle_mesh(mesh_path).sample_points_uniformly(N_INIT)
    r_max, r_min = eliminate_radii(pcl.surface_area, N_INIT, N_KEEP)
    dev = pcl.points.device
    ws_bytes = _lib.load().sv_sample_eliminate_workspace_bytes(c_int64(N_INIT), c_int(DEFAULT_DEGREE))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    kept = torch.empty(n_keep, dtype=torch.int32, device=dev)
    order = torch.empty(max(N_INIT - n_keep, 1), dtype=torch.int32, device=dev)
    counters = torch.empty(1, dtype=torch.int32, device=dev)
    ms = timed(lambda: call("sv_sample_eliminate", ptr(pcl.points), c_int64(N_INIT), c_int64(n_keep), c_double(r_max),
                            c_double(r_min), c_int(DEFAULT_DEGREE), ptr(ws), c_size_t(ws_bytes), ptr(kept), ptr(order),
                            ptr(counters), stream_ptr()))
    print(f"{label} sv_sample_eliminate, {N_INIT} -> {n_keep}, r_max {r_max * 1e3:.3f} mm, max_degree {DEFAULT_DEGREE}: "
          f"{ms:.3f} ms per call (largest neighbour count {counters.item()}, workspace {ws_bytes / 2**20:.1f} MiB)")


def startup(mesh_path):
    import torch

    from mrcc_amd.utils.mesh import load_cad_model

    torch.zeros(1, device="cuda")  # the context is the engine's anyway
    torch.cuda.synchronize()
    for label in ("first call", "second call"):
        t0 = time.perf_counter()
        points, _ = load_cad_model(mesh_path)
        print(f"startup: load_cad_model, {N_INIT} -> {N_KEEP}, {label}: {(time.perf_counter() - t0) * 1e3:.1f} ms wall clock, "
              f"{len(points)} model points kept")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--mesh", default=os.path.join(ROOT, "tests", "golden", "hand_notblender.obj"))
    ap.add_argument("--sections", default=",".join(SECTIONS))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        import mrcc_amd  # noqa: F401

        {"sample": lambda: sample(args.mesh), "table": lambda: eliminate(args.mesh, N_INIT, "table:  "),
         "loop": lambda: eliminate(args.mesh, N_KEEP, "loop:   "), "startup": lambda: startup(args.mesh)}[args.child]()
        return
    for section in args.sections.split(","):
        if section not in SECTIONS:
            ap.error(f"unknown section {section!r}")
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--mesh", args.mesh, "--child", section]).returncode
        if rc != 0:  # one child at a time
            sys.exit(f"{section} ended with status {rc}; nothing further is started")


if __name__ == "__main__":
    main()
