"""Pose averaging with the reference's names (utils/calibration.py:69-139), eigen-solve on libsvhip.

compute_quaternions_weighted_average: principal eigenvector of sum w_i q_i q_i^T / sum w_i — the reference uses
np.linalg.eig and leaves the sign arbitrary; here the sign makes the largest-magnitude component positive.
"""
from ctypes import c_int

import numpy as np
import torch

from .._lib import call, ptr, stream_ptr


def compute_quaternions_weighted_average_batched(Q, w=None, M=None, device=None):
    """Q [B, Mmax, 4] (w,x,y,z); w [B, Mmax] (None: all 1); M int[B] in [1, Mmax] (None: Mmax).  Returns [B,4] float64.
    A NaN / inf in a problem's first M quaternions or weights, or a weight sum <= 0, gives NaN for that problem."""
    Q = np.asarray(Q, dtype=np.float64)
    if Q.ndim != 3 or Q.shape[2] != 4 or Q.shape[1] < 1:
        raise ValueError(f"Q must be B x Mmax x 4 with Mmax >= 1, got {Q.shape}")
    B, Mmax, _ = Q.shape
    if w is not None:
        w = np.asarray(w, dtype=np.float64)
        if w.shape != (B, Mmax):
            raise ValueError(f"w must have shape {(B, Mmax)}, got {w.shape}")
    if M is not None:
        M = np.asarray(M, dtype=np.int32)
        if M.shape != (B,):
            raise ValueError(f"M must have shape ({B},), got {M.shape}")
        if (M < 1).any() or (M > Mmax).any():
            raise ValueError(f"M out of range: every M[b] must lie in [1, {Mmax}]")
    dev = torch.device("cuda" if device is None else device)
    Qt = torch.as_tensor(np.ascontiguousarray(Q)).to(dev)
    wt = None if w is None else torch.as_tensor(np.ascontiguousarray(w)).to(dev)
    Mt = None if M is None else torch.as_tensor(M).to(dev)
    out = torch.empty((B, 4), dtype=torch.float64, device=dev)
    call("sv_quat_avg_batched", ptr(Qt), ptr(wt), ptr(Mt), c_int(Mmax), c_int(B), ptr(out), stream_ptr())
    return out.cpu().numpy()


def compute_quaternions_weighted_average(Q, w):
    Q = np.asarray(Q, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    return compute_quaternions_weighted_average_batched(Q[None], w[None])[0]


def compute_quaternions_average(Q):
    return compute_quaternions_weighted_average(Q, np.ones(np.asarray(Q).shape[0]))


def compute_translations_average(t, weights=None):
    t = np.asarray(t, dtype=np.float64)
    if weights is None:
        weights = np.ones(len(t))
    weights = np.asarray(weights, dtype=np.float64)
    return np.sum(t * weights.reshape(-1, 1), axis=0) / np.sum(weights)


def compute_poses_average(poses, weights=None):
    """poses Nx7 (x, y, z, qw, qx, qy, qz) -> 7-vector (utils/calibration.py:117-139)."""
    if poses is None or len(poses) == 0:
        return poses
    poses = np.asarray(poses, dtype=np.float64)
    if len(poses.shape) != 2:
        poses = np.array(poses.reshape(-1, 7), copy=True)
    if len(poses) == 1:
        return poses[0]
    if weights is None or len(weights) != len(poses):
        weights = np.ones(len(poses))
    out = np.zeros(7)
    out[:3] = compute_translations_average(poses[:, :3], weights=weights)
    out[3:] = compute_quaternions_weighted_average(poses[:, 3:], weights)
    return out


def remove_pose_outliers(poses):
    # the reference computes the outlier mask and then returns the input unchanged (utils/calibration.py:55-61)
    return poses


def refine_base_pose(cad_points, crops, ee2base_poses, base_pose, method="point2plane", normals=None, icp_threshold=0.1,
                     max_iterations=30, device="cuda"):
    """One registration over all frames with the camera<-base transform as the single unknown (utils/icp.py icp_joint,
    sv_icp_batched in shared mode): frame i sees the CAD model at ee2cam_i = base2cam . ee2base_i
    (transformation.get_base2cam_matrix), so the source of problem i is get_transformation_matrix(ee2base_poses[i]) .
    cad_points, its target crops[i], and the shared transform starts at get_transformation_matrix(base_pose).
    method: "point2point" or "point2plane"; for the latter `normals` holds the crops' normals, or None estimates them
    per crop (utils/icp.py estimate_normals' defaults).  -> (pose (x, y, z, qw, qx, qy, qz), info) with info = {"fitness",
    "rmse", "updates" (pooled), "frame_fitness", "frame_rmse" ([len(crops)] arrays)}."""
    from . import icp as I
    from .transformation import get_pose_from_matrix, get_transformation_matrix

    if method not in ("point2point", "point2plane"):
        raise ValueError(f"method must be 'point2point' or 'point2plane', got {method!r}")
    if len(crops) != len(ee2base_poses) or not crops:
        raise ValueError(f"need one ee2base pose per crop and at least one crop, got {len(crops)} crops and "
                         f"{len(ee2base_poses)} poses")
    if normals is not None and len(normals) != len(crops):
        raise ValueError(f"normals must hold one array per crop ({len(crops)}), got {len(normals)}")
    pre = np.stack([get_transformation_matrix(np.asarray(p, dtype=np.float64)) for p in ee2base_poses])
    init = get_transformation_matrix(np.asarray(base_pose, dtype=np.float64))
    if method == "point2plane" and normals is None:
        I._check_batch_shapes(cad_points, crops, None, init, pre, True, icp_threshold, max_iterations)
        dev = torch.device(device)
        crops = [I._cloud(c, "crops", dev) for c in crops]
        normals = [I.estimate_normals(c)[0] for c in crops]
    T, stats = I.icp_joint(cad_points, crops, init, normals if method == "point2plane" else None, pre, icp_threshold,
                           max_iterations, device=device)
    per_frame = stats[3:].reshape(-1, 2)
    info = {"fitness": float(stats[0]), "rmse": float(stats[1]), "updates": int(stats[2]),
            "frame_fitness": per_frame[:, 0].copy(), "frame_rmse": per_frame[:, 1].copy()}
    return get_pose_from_matrix(T), info
