"""Batched ICP (sv_icp_batched) against the loop of single calls, and the joint calibration refinement against the
average of per-frame refinements.  Each side of each comparison runs in a child process of its own, one after the other.

    python tools/icp_batch_timing.py [--sections problems,stream,calibration]

problems:    8 and 32 registrations of an 8192-point model to crops of 2000-4000 points (a group of 4 / 16 frames, two
             poses each), both objectives: ms per group and host waits (device -> host copies) per group.
stream:      InferenceEngine.predict_stream frames/s with INFERENCE.icp_enabled, icp_batched False against True (random-
             init networks on the synthetic scenes of the engine tests, group 4).
calibration: an asymmetric model, M = 8 one-sided noisy views at seeded ee2base poses, start 5 mm / 2 degrees off: final
             error of the joint refinement (utils/calibration.py refine_base_pose) and of the average of the per-frame
             refinements (each frame's ee pose refined alone, turned into a base pose, compute_poses_average)."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METHODS = ("point2point", "point2plane")
SECTIONS = {"problems": ("loop", "batched"), "stream": ("loop", "batched"), "calibration": ("average", "joint")}


class HostWaits:
    """counts device -> host copies (Tensor.cpu of a device tensor), the points where the host waits for the stream"""

    def __init__(self):
        import torch

        self.n = 0
        cpu = torch.Tensor.cpu

        def counted(t, *a, **kw):
            self.n += int(t.is_cuda)
            return cpu(t, *a, **kw)

        torch.Tensor.cpu = counted


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def rigid(rng, shift):
    T = np.eye(4)
    T[:3, :3] = rotation(rng.normal(size=3), rng.uniform(0, np.pi))
    T[:3, 3] = rng.uniform(-shift, shift, 3)
    return T


def egg(rng, n):
    """n points on an asymmetric closed surface of gripper size (an ellipsoid whose +x and +y halves are stretched by
    1.4 and 0.7) and their outward unit normals, float64"""
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    scale = np.array([0.05, 0.11, 0.065]) * np.where(u > 0, [1.4, 0.7, 1.0], 1.0)
    grad = u / scale
    return u * scale, grad / np.linalg.norm(grad, axis=1, keepdims=True)


def timed(fn, reps=10, warmup=3):
    import torch

    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, out


# ---- problems -------------------------------------------------------------------------------------------------------
def problems(side):
    import torch

    from mrcc_amd.utils import icp as I
    from mrcc_amd.utils.transformation import get_pose_from_matrix

    waits = HostWaits()
    rng = np.random.default_rng(0)
    model, _ = egg(rng, 8192)
    for frames in (4, 16):
        crops, poses = [], []
        for f in range(frames):
            T = rigid(rng, 0.3)
            n = int(rng.integers(2000, 4001))
            crop = (model[rng.choice(8192, n)] @ T[:3, :3].T + T[:3, 3] + rng.normal(size=(n, 3)) * 5e-4).astype(np.float32)
            for _ in range(2):  # two poses per frame, 5 mm / 2 degrees off, on the same crop
                off = np.eye(4)
                off[:3, :3] = rotation(rng.normal(size=3), np.deg2rad(2.0))
                off[:3, 3] = rng.normal(size=3) * 0.003
                crops.append(crop)
                poses.append(get_pose_from_matrix(T @ off))
        for method in METHODS:
            match = (I.get_point2plane_matcher if method == "point2plane" else I.get_point2point_matcher)(
                model.astype(np.float32))
            if side == "loop" and method == "point2plane":  # the engine's loop: normals once per frame

                def run():
                    out = []
                    for f in range(frames):
                        crop = torch.as_tensor(crops[2 * f]).cuda()
                        normals = match.crop_normals(crop)
                        out += [match(crop, poses[2 * f], normals), match(crop, poses[2 * f + 1], normals)]
                    return out
            elif side == "loop":
                run = lambda: [match(c, p) for c, p in zip(crops, poses)]
            else:
                run = lambda: match.many(crops, poses)
            ms, out = timed(run)
            before = waits.n
            run()
            digest = float(np.abs(np.stack(out)).sum())
            print(f"problems: {2 * frames:2d} registrations ({frames} frames), {method}, {side}: {ms:.2f} ms per group, "
                  f"{waits.n - before} host waits per group, sum |pose| {digest:.12f}")


# ---- stream ---------------------------------------------------------------------------------------------------------
def stream(side):
    import mrcc_amd
    from mrcc_amd.app.dto import PointCloudDTO
    from mrcc_amd.app.inference_engine import InferenceEngine
    from mrcc_amd.utils.config import Config

    Config.reset()
    Config().update({"INFERENCE": {"SEGMENTATION": {"scale": 50}, "ROTATION": {"scale": 100},
                                   "KEY_POINTS": {"scale": 100, "conf_threshold": 0.0}, "ee_point_counts_threshold": 64,
                                   "SANITY": {"min_num_of_ee_points": 64}, "icp_enabled": True}})
    rng = np.random.default_rng(77)
    cad = (rng.uniform(-0.5, 0.5, size=(8192, 3)) * np.array([0.10, 0.22, 0.13]) + np.array([0.0, 0.0, 0.06])).astype(
        np.float32)
    scenes = [mrcc_amd.synth.gen_scene(s, n_bg=20000, n_arm=2000, n_ee=3000, keyed_colors=True) for s in range(8)]
    frames = [PointCloudDTO(points=sc["points"], rgb=sc["rgb"], ee2base_pose=sc["ee2base_pose"]) for sc in scenes] * 4
    for method in METHODS:
        eng = InferenceEngine(allow_random_init=True, seed=3, cad_points=cad, icp_method=method,
                              icp_batched=(side == "batched"))
        mrcc_amd.synth.wire_color_keyed_labels(eng._segmentation_model)
        list(eng.predict_stream(iter(frames[:8]), group=4))  # warm-up
        best = 0.0
        for _ in range(3):
            t0 = time.perf_counter()
            out = list(eng.predict_stream(iter(frames), group=4))
            best = max(best, len(frames) / (time.perf_counter() - t0))
        refined = sum(r.ee_pose is not None for r in out) + sum(r.key_points_pose is not None for r in out)
        print(f"stream: {len(frames)} frames of 25000 points, group 4, {method}, icp_batched={side == 'batched'}: "
              f"{best:.1f} frames/s (best of 3), {refined} poses refined")


# ---- calibration ----------------------------------------------------------------------------------------------------
def pose_error(T, true_T):
    D = np.linalg.inv(true_T) @ T
    ang = np.rad2deg(np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1)))
    return np.linalg.norm(T[:3, 3] - true_T[:3, 3]) * 1e3, ang


def calibration(side):
    from mrcc_amd.utils import icp as I
    from mrcc_amd.utils.calibration import compute_poses_average, refine_base_pose
    from mrcc_amd.utils.transformation import get_pose_from_matrix, get_transformation_matrix

    rng = np.random.default_rng(2)
    model, normals = egg(rng, 8192)
    cad = model.astype(np.float32)
    base2cam = rigid(rng, 0.5)
    M, crops, ee2base = 8, [], []
    for i in range(M):
        pre = rigid(rng, 0.4)
        view = rng.normal(size=3)
        view /= np.linalg.norm(view)
        seen = np.flatnonzero(normals @ view > 0.2)  # one side of the model
        rows = seen[rng.permutation(len(seen))[:3000]]
        T = base2cam @ pre
        crops.append((model[rows] @ T[:3, :3].T + T[:3, 3] + rng.normal(size=(len(rows), 3)) * 5e-4).astype(np.float32))
        ee2base.append(get_pose_from_matrix(pre))
    centre = np.concatenate(crops).astype(np.float64).mean(0)
    off = np.eye(4)
    off[:3, :3] = rotation(rng.normal(size=3), np.deg2rad(2.0))
    d = rng.normal(size=3)
    off[:3, 3] = centre - off[:3, :3] @ centre + d / np.linalg.norm(d) * 5e-3
    start = get_pose_from_matrix(off @ base2cam)
    e0 = pose_error(get_transformation_matrix(start), base2cam)
    if side == "average":
        print(f"calibration: {M} one-sided views of {[len(c) for c in crops]} points, 0.5 mm noise, start off by "
              f"{e0[0]:.2f} mm / {e0[1]:.2f} deg (rotation about the crops' centroid), max distance 0.02 m")
    for method in METHODS:
        if side == "joint":
            pose, info = refine_base_pose(cad, crops, ee2base, start, method=method, icp_threshold=0.02)
            note = f"{info['updates']} updates, pooled fitness {info['fitness']:.3f}, rmse {info['rmse'] * 1e3:.2f} mm"
        else:
            match = (I.get_point2plane_matcher if method == "point2plane" else I.get_point2point_matcher)(
                cad, icp_threshold=0.02)
            start_T = get_transformation_matrix(start)
            inits = [get_pose_from_matrix(start_T @ get_transformation_matrix(p)) for p in ee2base]
            refined = match.many(crops, inits)
            per_frame = [get_pose_from_matrix(get_transformation_matrix(r) @ np.linalg.inv(get_transformation_matrix(p)))
                         for r, p in zip(refined, ee2base)]
            pose = compute_poses_average(np.array(per_frame, dtype=np.float32))
            worst = max(pose_error(get_transformation_matrix(p), base2cam)[0] for p in per_frame)
            note = f"worst single frame {worst:.2f} mm"
        e = pose_error(get_transformation_matrix(pose), base2cam)
        print(f"calibration: {method}, {side}: final error {e[0]:.2f} mm / {e[1]:.3f} deg ({note})")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sections", default=",".join(SECTIONS))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        import torch

        import mrcc_amd  # noqa: F401

        section, side = args.child.split(":")
        if section == "problems" and side == "loop":
            print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, 10 timed calls after 3 warm-up")
        {"problems": problems, "stream": stream, "calibration": calibration}[section](side)
        return
    for section in args.sections.split(","):
        if section not in SECTIONS:
            ap.error(f"unknown section {section!r}")
        for side in SECTIONS[section]:  # one child per side, one at a time
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{section}:{side}"]).returncode
            if rc != 0:
                sys.exit(f"{section}:{side} ended with status {rc}; nothing further is started")


if __name__ == "__main__":
    main()
