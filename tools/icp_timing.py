"""Timing of the ICP refinements (8192 CAD points against an end-effector crop, <= 30 updates) and one synthetic
partial-view case, for both objectives in one process.

    python tools/icp_timing.py [--method point2point,point2plane]

Per method: ms per call and updates to convergence on two random-cloud cases; for point-to-plane the normal estimation's ms
separately.  Then the partial view: model points on a closed surface (an ellipsoid), target = the half facing +z with
0.5 mm noise, initial pose off by 5 mm / 2 degrees; final translation and rotation error per method."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mrcc_amd  # noqa: E402,F401
from mrcc_amd.utils import icp as I  # noqa: E402

METHODS = ("point2point", "point2plane")


def timed(fn, reps=10, warmup=3):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, out


def run(method, src, tgt, init, normals=None, **kw):
    if method == "point2point":
        return I.icp_point2point(src, tgt, init, **kw)
    return I.icp_point2plane(src, tgt, normals, init, **kw)


def random_cloud_cases(methods):
    rng = np.random.default_rng(0)
    src = rng.uniform(-0.1, 0.1, size=(8192, 3)).astype(np.float32)
    t = np.array([0.01, -0.005, 0.004], dtype=np.float32)
    for nt in (2000, 8000):
        tgt = (src[rng.choice(8192, nt)] + t + rng.normal(size=(nt, 3)).astype(np.float32) * 1e-3).astype(np.float32)
        s_d, t_d = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
        for method in methods:
            normals = None
            if method == "point2plane":
                ms_n, (normals, counts) = timed(lambda: I.estimate_normals(t_d))
                print(f"{nt} target points: normals {ms_n:.2f} ms per call (radius 0.02, max_nn 30, "
                      f"mean neighbours {counts.float().mean().item():.1f})")
            ms, out = timed(lambda: run(method, s_d, t_d, np.eye(4), normals))
            print(f"{nt} target points: {method} {ms:.2f} ms per ICP call, {out[3]} updates, fitness {out[1]:.3f}, "
                  f"rmse {out[2] * 1e3:.2f} mm")


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def partial_view_case(methods):
    """the model is in its true pose when T = identity, so the errors are read off the result directly"""
    rng = np.random.default_rng(1)
    u = rng.normal(size=(8192, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    model = (u * np.array([0.05, 0.11, 0.065])).astype(np.float32)  # closed surface: an ellipsoid of gripper size
    grad = u / np.array([0.05, 0.11, 0.065])
    facing = grad[:, 2] / np.linalg.norm(grad, axis=1) > 0.0  # the half whose outward normal faces +z
    view = model[facing][rng.permutation(int(facing.sum()))[:3000]]
    tgt = (view + rng.normal(size=view.shape) * 5e-4).astype(np.float32)
    init = np.eye(4)
    init[:3, :3] = rotation(rng.normal(size=3), np.deg2rad(2.0))
    d = rng.normal(size=3)
    init[:3, 3] = d / np.linalg.norm(d) * 5e-3
    s_d, t_d = torch.from_numpy(model).cuda(), torch.from_numpy(tgt).cuda()
    print(f"partial view: {len(model)} model points on an ellipsoid, {len(tgt)} target points on the half facing +z, "
          f"0.5 mm noise, initial pose off by 5.00 mm / 2.00 deg, max distance 0.02 m")
    for method in methods:
        normals = I.estimate_normals(t_d)[0] if method == "point2plane" else None
        ms, (T, fit, rmse, n) = timed(lambda: run(method, s_d, t_d, init, normals, max_distance=0.02))
        ang = np.rad2deg(np.arccos(np.clip((np.trace(T[:3, :3]) - 1) / 2, -1, 1)))
        print(f"partial view: {method} {ms:.2f} ms, {n} updates, fitness {fit:.3f}, rmse {rmse * 1e3:.2f} mm, "
              f"final error {np.linalg.norm(T[:3, 3]) * 1e3:.2f} mm / {ang:.2f} deg")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--method", default=",".join(METHODS), help="comma-separated: point2point, point2plane")
    methods = ap.parse_args().method.split(",")
    for m in methods:
        if m not in METHODS:
            ap.error(f"unknown method {m!r}")
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, 10 timed calls after 3 warm-up")
    random_cloud_cases(methods)
    partial_view_case(methods)


if __name__ == "__main__":
    main()
