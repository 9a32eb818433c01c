"""ICP refinement with the reference's interface (utils/icp.py:13-83) on libsvhip.

    match = get_point2point_matcher(cad_points)       # the reference samples 8192 points from app/hand_files/*.obj
    pose = match(ee_points, pose_initial)             # (x, y, z, qw, qx, qy, qz) -> refined pose

Same registration as the reference's open3d call: point-to-point, max correspondence distance 0.1 m, at most 30
updates, relative fitness / rmse tolerance 1e-6, source = CAD points, target = end-effector crop, initial transform
from the predicted pose.  (The reference also estimates normals on the crop, which point-to-point ICP never reads.)

Opt-in, beyond the reference: the registration those normals were meant for.

    normals, counts = estimate_normals(ee_points)     # hybrid radius 0.02 m / 30-nearest search, PCA (sv_estimate_normals)
    match = get_point2plane_matcher(cad_points)
    pose = match(ee_points, pose_initial)             # or match(ee_points, pose_initial, normals) to reuse them

The definitions (include/sv_hip.h, block N3b) are Open3D's published algorithm; parity with Open3D binaries is by
construction and unverified.
"""
from ctypes import c_double, c_int, c_int64, c_size_t

import numpy as np
import torch

from .. import _lib
from .._lib import call, ptr, stream_ptr
from .transformation import get_pose_from_matrix, get_transformation_matrix


def icp_point2point(src, tgt, init_T=None, max_distance=0.1, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6,
                    device="cuda"):
    """src [S,3], tgt [T,3] (numpy or tensors) -> (T 4x4 float64 numpy, fitness, inlier rmse, updates)."""
    dev = torch.device(device)
    s = torch.as_tensor(np.ascontiguousarray(src, dtype=np.float32) if not torch.is_tensor(src) else src).to(
        device=dev, dtype=torch.float32).contiguous()
    t = torch.as_tensor(np.ascontiguousarray(tgt, dtype=np.float32) if not torch.is_tensor(tgt) else tgt).to(
        device=dev, dtype=torch.float32).contiguous()
    S, T = s.shape[0], t.shape[0]
    init = None if init_T is None else torch.as_tensor(np.ascontiguousarray(init_T, dtype=np.float64)).to(dev)
    ws_bytes = _lib.load().sv_icp_workspace_bytes(c_int64(S))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out_T = torch.empty(16, dtype=torch.float64, device=dev)
    stats = torch.empty(3, dtype=torch.float64, device=dev)
    call("sv_icp_point2point", ptr(s), c_int64(S), ptr(t), c_int64(T), ptr(init), c_double(max_distance),
         c_int(max_iterations), c_double(rel_fitness), c_double(rel_rmse), ptr(ws), c_size_t(ws_bytes), ptr(out_T),
         ptr(stats), stream_ptr())
    st = stats.cpu().numpy()
    return out_T.cpu().numpy().reshape(4, 4), float(st[0]), float(st[1]), int(st[2])


def get_point2point_matcher(cad_points, icp_threshold=0.1, max_iterations=30, device="cuda"):
    cad = torch.as_tensor(np.ascontiguousarray(cad_points, dtype=np.float32)).to(device)

    def match(ee_points, pose_initial):
        if ee_points is None or pose_initial is None:
            return pose_initial
        T0 = get_transformation_matrix(np.asarray(pose_initial, dtype=np.float64), switch_w=False)
        T, _, _, _ = icp_point2point(cad, ee_points, T0, icp_threshold, max_iterations, device=device)
        return get_pose_from_matrix(T)

    return match


def _cloud(x, name, dev):
    """[N,3] numpy array or tensor -> contiguous float32 tensor on dev; the shape is checked before anything moves."""
    shape = tuple(x.shape) if hasattr(x, "shape") else np.shape(x)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"{name} must be [N, 3], got {shape}")
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32))
    return x.to(device=dev, dtype=torch.float32).contiguous()


def _check_normals_args(n_points, radius, max_nn):
    if not 1 <= n_points <= 1 << 20:
        raise ValueError(f"points must hold 1 to 2^20 rows, got {n_points}")
    if not radius > 0:
        raise ValueError(f"radius must be positive, got {radius!r}")
    if not 3 <= int(max_nn) <= 64:
        raise ValueError(f"max_nn must lie in [3, 64], got {max_nn!r}")


def _normals_enqueue(pts, radius, max_nn):
    """pts: float32 [N,3] device tensor -> (normals [N,3] float32, counts [N] int32) on the device, no read-back."""
    N = pts.shape[0]
    ws_bytes = _lib.load().sv_normals_workspace_bytes(c_int64(N), c_int(max_nn))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pts.device)
    normals = torch.empty((N, 3), dtype=torch.float32, device=pts.device)
    counts = torch.empty(N, dtype=torch.int32, device=pts.device)
    call("sv_estimate_normals", ptr(pts), c_int64(N), c_double(radius), c_int(max_nn), ptr(ws), c_size_t(ws_bytes),
         ptr(normals), ptr(counts), stream_ptr())
    return normals, counts


def estimate_normals(points, radius=0.02, max_nn=30, device="cuda"):
    """points [N,3] -> (normals [N,3] float32, counts [N] int32): per point the PCA normal of its (at most max_nn
    nearest) neighbours within radius, counts = neighbours used.  A numpy input gives numpy outputs; a CUDA tensor gives
    tensors on its device."""
    is_tensor = torch.is_tensor(points)
    shape = tuple(points.shape) if hasattr(points, "shape") else np.shape(points)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"points must be [N, 3], got {shape}")
    _check_normals_args(shape[0], radius, max_nn)
    dev = points.device if is_tensor and points.is_cuda else torch.device(device)
    normals, counts = _normals_enqueue(_cloud(points, "points", dev), float(radius), int(max_nn))
    if is_tensor:
        return normals, counts
    return normals.cpu().numpy(), counts.cpu().numpy()


def _check_icp_args(S, T, n_normals, max_distance, max_iterations):
    if not 3 <= S < 1 << 24:
        raise ValueError(f"src must hold 3 to 2^24 - 1 points, got {S}")
    if not 1 <= T < 1 << 24:
        raise ValueError(f"tgt must hold 1 to 2^24 - 1 points, got {T}")
    if n_normals != T:
        raise ValueError(f"tgt_normals must hold one normal per target point ({T}), got {n_normals}")
    if not max_distance > 0:
        raise ValueError(f"max_distance must be positive, got {max_distance!r}")
    if int(max_iterations) < 0:
        raise ValueError(f"max_iterations must not be negative, got {max_iterations!r}")


def _point2plane_enqueue(s, t, tn, init, max_distance, max_iterations, rel_fitness, rel_rmse):
    """device tensors in, (out_T [16] float64, stats [3] float64) device tensors out, no read-back"""
    S, T = s.shape[0], t.shape[0]
    ws_bytes = _lib.load().sv_icp_point2plane_workspace_bytes(c_int64(S))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=s.device)
    out_T = torch.empty(16, dtype=torch.float64, device=s.device)
    stats = torch.empty(3, dtype=torch.float64, device=s.device)
    call("sv_icp_point2plane", ptr(s), c_int64(S), ptr(t), ptr(tn), c_int64(T), ptr(init), c_double(max_distance),
         c_int(max_iterations), c_double(rel_fitness), c_double(rel_rmse), ptr(ws), c_size_t(ws_bytes), ptr(out_T),
         ptr(stats), stream_ptr())
    return out_T, stats


def icp_point2plane(src, tgt, tgt_normals, init_T=None, max_distance=0.1, max_iterations=30, rel_fitness=1e-6,
                    rel_rmse=1e-6, device="cuda"):
    """src [S,3], tgt [T,3], tgt_normals [T,3] (numpy or tensors) -> (T 4x4 float64 numpy, fitness, inlier rmse,
    updates), as icp_point2point but minimising the distance to the target's tangent planes."""
    dev = torch.device(device)
    shapes = [tuple(x.shape) if hasattr(x, "shape") else np.shape(x) for x in (src, tgt, tgt_normals)]
    for name, shape in zip(("src", "tgt", "tgt_normals"), shapes):
        if len(shape) != 2 or shape[1] != 3:
            raise ValueError(f"{name} must be [N, 3], got {shape}")
    _check_icp_args(shapes[0][0], shapes[1][0], shapes[2][0], max_distance, max_iterations)
    if init_T is not None and np.shape(init_T) != (4, 4):
        raise ValueError(f"init_T must be 4x4, got {np.shape(init_T)}")
    s, t, tn = _cloud(src, "src", dev), _cloud(tgt, "tgt", dev), _cloud(tgt_normals, "tgt_normals", dev)
    init = None if init_T is None else torch.as_tensor(np.ascontiguousarray(init_T, dtype=np.float64)).to(dev)
    out_T, stats = _point2plane_enqueue(s, t, tn, init, float(max_distance), int(max_iterations), float(rel_fitness),
                                        float(rel_rmse))
    st = stats.cpu().numpy()
    return out_T.cpu().numpy().reshape(4, 4), float(st[0]), float(st[1]), int(st[2])


class PointToPlaneMatcher:
    """The point-to-plane counterpart of get_point2point_matcher's closure, for one CAD model.

        match = PointToPlaneMatcher(cad_points)
        pose = match(ee_points, pose_initial)               # estimates the crop's normals, then refines
        normals = match.crop_normals(ee_points)             # or: estimate once, refine several poses on one crop
        pose = match(ee_points, pose_initial, normals)

    Normal estimation and ICP are enqueued back to back on the stream, with one read-back at the end."""

    def __init__(self, cad_points, icp_threshold=0.1, max_iterations=30, normal_radius=0.02, normal_max_nn=30,
                 device="cuda"):
        _check_normals_args(1, normal_radius, normal_max_nn)
        self.device = torch.device(device)
        self.cad = _cloud(cad_points, "cad_points", self.device)
        self.icp_threshold, self.max_iterations = float(icp_threshold), int(max_iterations)
        self.normal_radius, self.normal_max_nn = float(normal_radius), int(normal_max_nn)

    def crop_normals(self, ee_points):
        """the normals __call__ would estimate for this crop, as a float32 [N,3] device tensor (no read-back)"""
        tgt = _cloud(ee_points, "ee_points", self.device)
        _check_normals_args(tgt.shape[0], self.normal_radius, self.normal_max_nn)
        return _normals_enqueue(tgt, self.normal_radius, self.normal_max_nn)[0]

    def __call__(self, ee_points, pose_initial, normals=None):
        """normals: the crop's (crop_normals' or estimate_normals' first result, numpy or device tensor); None estimates
        them.  A None crop or pose returns pose_initial, as the point-to-point matcher does."""
        if ee_points is None or pose_initial is None:
            return pose_initial
        shape = tuple(ee_points.shape) if hasattr(ee_points, "shape") else np.shape(ee_points)
        if len(shape) != 2 or shape[1] != 3:
            raise ValueError(f"ee_points must be [N, 3], got {shape}")
        n_normals = shape[0] if normals is None else len(normals)
        _check_icp_args(self.cad.shape[0], shape[0], n_normals, self.icp_threshold, self.max_iterations)
        T0 = get_transformation_matrix(np.asarray(pose_initial, dtype=np.float64), switch_w=False)
        tgt = _cloud(ee_points, "ee_points", self.device)
        tn = self.crop_normals(tgt) if normals is None else _cloud(normals, "normals", self.device)
        init = torch.as_tensor(np.ascontiguousarray(T0, dtype=np.float64)).to(self.device)
        out_T, _ = _point2plane_enqueue(self.cad, tgt, tn, init, self.icp_threshold, self.max_iterations, 1e-6, 1e-6)
        return get_pose_from_matrix(out_T.cpu().numpy().reshape(4, 4))


def get_point2plane_matcher(cad_points, icp_threshold=0.1, max_iterations=30, normal_radius=0.02, normal_max_nn=30,
                            device="cuda"):
    """-> match(ee_points, pose_initial, normals=None), a PointToPlaneMatcher: the same None handling as the
    point-to-point matcher; match.crop_normals(ee_points) gives the normals to share between several calls on one crop."""
    return PointToPlaneMatcher(cad_points, icp_threshold, max_iterations, normal_radius, normal_max_nn, device)
