"""ICP refinement with the reference's interface (utils/icp.py:13-83) on libsvhip.

    match = get_point2point_matcher(cad_points)       # points [P,3], or the mesh / .pcd file the reference reads:
    match = get_point2point_matcher("hand_notblender.obj")   # 16384 surface samples thinned to 8192 (utils/mesh.py)
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

Opt-in, many registrations of the one CAD model per call (sv_icp_batched, block N3c):

    poses = match.many(crops, poses)                  # every (crop, pose) pair refined as match(crop, pose) would,
                                                      # bit for bit, in one call with one read-back
    T, stats = icp_batched(src, tgts, init_Ts)        # P independent problems
    T, stats = icp_joint(src, tgts, init_T, pre=pre)  # ONE transform for all: source of problem p = pre[p] . src
"""
from ctypes import c_double, c_int, c_int64, c_size_t

import numpy as np
import torch

from .. import _lib
from .._lib import call, ptr, stream_ptr
from .transformation import get_pose_from_matrix, get_transformation_matrix


def _cad_model(cad_points, device):
    """what the matchers are given -> the model points: an array is passed on as it is, a str / os.PathLike is the
    reference's cad_name and is loaded as utils/icp.py:17-40 does (utils/mesh.py load_cad_model)"""
    from .mesh import is_path, load_cad_model

    if cad_points is None:
        raise ValueError("the matcher needs cad_points (the CAD model of the end effector, [P,3]) or the path of its "
                         "mesh / .pcd file")
    return load_cad_model(cad_points, device=device)[0] if is_path(cad_points) else cad_points


def _shape(x):
    return tuple(x.shape) if hasattr(x, "shape") else np.shape(x)


def _cloud(x, name, dev):
    """[N,3] numpy array or tensor -> contiguous float32 tensor on dev; the shape is checked before anything moves."""
    shape = _shape(x)
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
    shape = _shape(points)
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


def _matrix(m, dev):
    """None, or 4x4 matrices (numpy) -> float64 tensor on dev"""
    return None if m is None else torch.as_tensor(np.ascontiguousarray(m, dtype=np.float64)).to(dev)


def _icp_enqueue(s, t, tn, init, max_distance, max_iterations, rel_fitness, rel_rmse):
    """One problem, device tensors in: tn None is sv_icp_point2point, target normals are sv_icp_point2plane.
    -> float64 [19] device tensor (out_T 16, then fitness, rmse, updates), no read-back"""
    S, T = s.shape[0], t.shape[0]
    lib = _lib.load()
    ws_bytes = (lib.sv_icp_workspace_bytes if tn is None else lib.sv_icp_point2plane_workspace_bytes)(c_int64(S))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=s.device)
    out = torch.empty(19, dtype=torch.float64, device=s.device)
    normals = () if tn is None else (ptr(tn),)
    call("sv_icp_point2point" if tn is None else "sv_icp_point2plane", ptr(s), c_int64(S), ptr(t), *normals, c_int64(T),
         ptr(init), c_double(max_distance), c_int(max_iterations), c_double(rel_fitness), c_double(rel_rmse), ptr(ws),
         c_size_t(ws_bytes), ptr(out[:16]), ptr(out[16:]), stream_ptr())
    return out


def _icp_single(src, tgt, tgt_normals, init_T, max_distance, max_iterations, rel_fitness, rel_rmse, device):
    """what icp_point2point and icp_point2plane share: conversion, enqueue and the one read-back"""
    dev = torch.device(device)
    s, t = _cloud(src, "src", dev), _cloud(tgt, "tgt", dev)
    tn = None if tgt_normals is None else _cloud(tgt_normals, "tgt_normals", dev)
    out = _icp_enqueue(s, t, tn, _matrix(init_T, dev), max_distance, max_iterations, rel_fitness, rel_rmse).cpu().numpy()
    return out[:16].reshape(4, 4), float(out[16]), float(out[17]), int(out[18])


def icp_point2point(src, tgt, init_T=None, max_distance=0.1, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6,
                    device="cuda"):
    """src [S,3], tgt [T,3] (numpy or tensors) -> (T 4x4 float64 numpy, fitness, inlier rmse, updates)."""
    return _icp_single(src, tgt, None, init_T, max_distance, max_iterations, rel_fitness, rel_rmse, device)


def icp_point2plane(src, tgt, tgt_normals, init_T=None, max_distance=0.1, max_iterations=30, rel_fitness=1e-6,
                    rel_rmse=1e-6, device="cuda"):
    """src [S,3], tgt [T,3], tgt_normals [T,3] (numpy or tensors) -> (T 4x4 float64 numpy, fitness, inlier rmse,
    updates), as icp_point2point but minimising the distance to the target's tangent planes."""
    shapes = [_shape(x) for x in (src, tgt, tgt_normals)]
    for name, shape in zip(("src", "tgt", "tgt_normals"), shapes):
        if len(shape) != 2 or shape[1] != 3:
            raise ValueError(f"{name} must be [N, 3], got {shape}")
    _check_icp_args(shapes[0][0], shapes[1][0], shapes[2][0], max_distance, max_iterations)
    if init_T is not None and np.shape(init_T) != (4, 4):
        raise ValueError(f"init_T must be 4x4, got {np.shape(init_T)}")
    return _icp_single(src, tgt, tgt_normals, init_T, float(max_distance), int(max_iterations), float(rel_fitness),
                       float(rel_rmse), device)


class _Matcher:
    """What the two matchers share: the CAD model on the device, the threshold and the iteration cap."""

    def __init__(self, cad_points, icp_threshold=0.1, max_iterations=30, device="cuda"):
        self.device = torch.device(device)
        self.cad = _cloud(_cad_model(cad_points, self.device), "cad_points", self.device)
        self.icp_threshold, self.max_iterations = icp_threshold, max_iterations

    def _refine(self, tgt, pose_initial, tn):
        """tgt, tn: device tensors (tn None: point-to-point) -> the refined pose, with one read-back"""
        T0 = get_transformation_matrix(np.asarray(pose_initial, dtype=np.float64), switch_w=False)
        T = _icp_enqueue(self.cad, tgt, tn, _matrix(T0, self.device), self.icp_threshold, self.max_iterations, 1e-6, 1e-6)
        return get_pose_from_matrix(T[:16].cpu().numpy().reshape(4, 4))


class PointToPointMatcher(_Matcher):
    """match = PointToPointMatcher(cad_points); match(ee_points, pose_initial) refines one pose (a None crop or pose
    returns pose_initial); match.many(crops, poses) refines a list of them in one sv_icp_batched call."""

    def __call__(self, ee_points, pose_initial):
        if ee_points is None or pose_initial is None:
            return pose_initial
        return self._refine(_cloud(ee_points, "tgt", self.device), pose_initial, None)

    def many(self, crops, poses, normals=None):
        """[match(c, p) for c, p in zip(crops, poses)], bit for bit, with one read-back; normals are not read"""
        return _refine_many(self.cad, crops, poses, None, float(self.icp_threshold), int(self.max_iterations),
                            self.device)


def get_point2point_matcher(cad_points, icp_threshold=0.1, max_iterations=30, device="cuda"):
    """-> match(ee_points, pose_initial), a PointToPointMatcher; cad_points: the model points or its file's path"""
    return PointToPointMatcher(cad_points, icp_threshold, max_iterations, device)


class PointToPlaneMatcher(_Matcher):
    """The point-to-plane counterpart of get_point2point_matcher's closure, for one CAD model.

        match = PointToPlaneMatcher(cad_points)
        pose = match(ee_points, pose_initial)               # estimates the crop's normals, then refines
        normals = match.crop_normals(ee_points)             # or: estimate once, refine several poses on one crop
        pose = match(ee_points, pose_initial, normals)

    Normal estimation and ICP are enqueued back to back on the stream, with one read-back at the end."""

    def __init__(self, cad_points, icp_threshold=0.1, max_iterations=30, normal_radius=0.02, normal_max_nn=30,
                 device="cuda"):
        _check_normals_args(1, normal_radius, normal_max_nn)
        super().__init__(cad_points, float(icp_threshold), int(max_iterations), device)
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
        shape = _shape(ee_points)
        if len(shape) != 2 or shape[1] != 3:
            raise ValueError(f"ee_points must be [N, 3], got {shape}")
        n_normals = shape[0] if normals is None else len(normals)
        _check_icp_args(self.cad.shape[0], shape[0], n_normals, self.icp_threshold, self.max_iterations)
        tgt = _cloud(ee_points, "ee_points", self.device)
        tn = self.crop_normals(tgt) if normals is None else _cloud(normals, "normals", self.device)
        return self._refine(tgt, pose_initial, tn)

    def many(self, crops, poses, normals=None):
        """[self(c, p, n) for c, p, n in zip(crops, poses, normals)], bit for bit, in one sv_icp_batched call with one
        read-back.  normals: None, or a list with the normals of every crop or None; missing ones are estimated, once
        per distinct crop object."""
        if normals is not None and len(normals) != len(crops):
            raise ValueError(f"normals must hold one entry per crop ({len(crops)}), got {len(normals)}")

        def crop_normals(k, tgt):
            if normals is not None and normals[k] is not None:
                return _cloud(normals[k], "normals", self.device)
            _check_normals_args(tgt.shape[0], self.normal_radius, self.normal_max_nn)
            return _normals_enqueue(tgt, self.normal_radius, self.normal_max_nn)[0]

        return _refine_many(self.cad, crops, poses, crop_normals, self.icp_threshold, self.max_iterations, self.device)


def get_point2plane_matcher(cad_points, icp_threshold=0.1, max_iterations=30, normal_radius=0.02, normal_max_nn=30,
                            device="cuda"):
    """-> match(ee_points, pose_initial, normals=None), a PointToPlaneMatcher: the same None handling as the
    point-to-point matcher; match.crop_normals(ee_points) gives the normals to share between several calls on one crop."""
    return PointToPlaneMatcher(cad_points, icp_threshold, max_iterations, normal_radius, normal_max_nn, device)


# ---- many registrations per call (sv_icp_batched, include/sv_hip.h block N3c) ----------------------------------------
MAX_PROBLEMS = 64


def _check_batch_shapes(src, tgts, tgt_normals, init_Ts, pre, shared, max_distance, max_iterations):
    """everything icp_batched can reject without touching a device -> (S, [T_p])"""
    if len(_shape(src)) != 2 or _shape(src)[1] != 3:
        raise ValueError(f"src must be [N, 3], got {_shape(src)}")
    P = len(tgts)
    if not 1 <= P <= MAX_PROBLEMS:
        raise ValueError(f"tgts must hold 1 to {MAX_PROBLEMS} clouds, got {P}")
    if tgt_normals is not None and len(tgt_normals) != P:
        raise ValueError(f"tgt_normals must hold one array per target cloud ({P}), got {len(tgt_normals)}")
    for p, t in enumerate(tgts):
        if len(_shape(t)) != 2 or _shape(t)[1] != 3:
            raise ValueError(f"tgts[{p}] must be [N, 3], got {_shape(t)}")
        n = _shape(t)[0]
        if tgt_normals is not None:
            if len(_shape(tgt_normals[p])) != 2 or _shape(tgt_normals[p])[1] != 3:
                raise ValueError(f"tgt_normals[{p}] must be [N, 3], got {_shape(tgt_normals[p])}")
            n = _shape(tgt_normals[p])[0]
        _check_icp_args(_shape(src)[0], _shape(t)[0], n, max_distance, max_iterations)
    want = (4, 4) if shared else (P, 4, 4)
    if init_Ts is not None and np.shape(init_Ts) != want:
        raise ValueError(f"init_Ts must be {want}, got {np.shape(init_Ts)}")
    if pre is not None and np.shape(pre) != (P, 4, 4):
        raise ValueError(f"pre must be {(P, 4, 4)}, got {np.shape(pre)}")
    return _shape(src)[0], [_shape(t)[0] for t in tgts]


def _icp_batched_enqueue(s, t, tn, offsets, init, pre, shared, max_distance, max_iterations, rel_fitness, rel_rmse):
    """s [S,3], t / tn [sum T_p,3] float32 and init / pre float64 device tensors (tn, init, pre may be None), offsets a
    HOST int64 array [P+1] -> (out_T [P,16] or [16], stats [P,3] or [3 + 2 P]) float64 device tensors; nothing
    here waits for the device"""
    S, P = s.shape[0], len(offsets) - 1
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    ws_bytes = _lib.load().sv_icp_batched_workspace_bytes(c_int64(S), c_int(P))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=s.device)
    nT, nS = (16, 3 + 2 * P) if shared else (16 * P, 3 * P)
    out = torch.empty(nT + nS, dtype=torch.float64, device=s.device)
    out_T, stats = out[:nT], out[nT:]
    call("sv_icp_batched", ptr(s), c_int64(S), ptr(pre), ptr(t), ptr(tn), offsets.ctypes.data_as(_lib.c_void_p), c_int(P),
         ptr(init), c_int(1 if shared else 0), c_double(max_distance), c_int(max_iterations), c_double(rel_fitness),
         c_double(rel_rmse), ptr(ws), c_size_t(ws_bytes), ptr(out_T), ptr(stats), stream_ptr())
    return (out_T, stats) if shared else (out_T.view(P, 16), stats.view(P, 3))


def _concat(clouds, name, dev):
    """list of [N,3] arrays or tensors -> one float32 [sum N, 3] device tensor: host arrays are joined first and moved
    once"""
    if not any(torch.is_tensor(c) for c in clouds):
        return _cloud(np.concatenate([np.asarray(c, dtype=np.float32) for c in clouds]), name, dev)
    return torch.cat([_cloud(c, name, dev) for c in clouds])


def icp_batched(src, tgts, init_Ts=None, tgt_normals=None, pre=None, shared=False, max_distance=0.1, max_iterations=30,
                rel_fitness=1e-6, rel_rmse=1e-6, device="cuda"):
    """P registrations of the one source cloud src [S,3] in one call.  tgts: list of P [T_p,3] clouds; tgt_normals: None
    (point-to-point) or their normals (point-to-plane); pre: None or [P,4,4], the source of problem p is pre[p] . src.
    shared=False: P independent problems, init_Ts [P,4,4] or None -> (T [P,4,4], stats [P,3] = fitness, rmse, updates),
    each problem exactly as icp_point2point / icp_point2plane.  shared=True: one transform, init_Ts [4,4] or None ->
    (T [4,4], stats [3 + 2 P] = pooled fitness, rmse, updates, then fitness_p, rmse_p).  float64 numpy."""
    dev = torch.device(device)
    _check_batch_shapes(src, tgts, tgt_normals, init_Ts, pre, shared, max_distance, max_iterations)
    offsets = np.concatenate([[0], np.cumsum([_shape(t)[0] for t in tgts])]).astype(np.int64)
    s, t = _cloud(src, "src", dev), _concat(tgts, "tgts", dev)
    tn = None if tgt_normals is None else _concat(tgt_normals, "tgt_normals", dev)
    init, pre = _matrix(init_Ts, dev), _matrix(pre, dev)
    out_T, stats = _icp_batched_enqueue(s, t, tn, offsets, init, pre, shared, float(max_distance), int(max_iterations),
                                        float(rel_fitness), float(rel_rmse))
    host = torch.cat([out_T.reshape(-1), stats.reshape(-1)]).cpu().numpy()  # one read-back
    nT = out_T.numel()
    return (host[:nT].reshape((4, 4) if shared else (-1, 4, 4)),
            host[nT:] if shared else host[nT:].reshape(-1, 3))


def icp_joint(src, tgts, init_T=None, tgt_normals=None, pre=None, max_distance=0.1, max_iterations=30, rel_fitness=1e-6,
              rel_rmse=1e-6, device="cuda"):
    """icp_batched(..., shared=True): the one transform T that registers pre[p] . src to tgts[p] for all p at once"""
    return icp_batched(src, tgts, init_T, tgt_normals, pre, True, max_distance, max_iterations, rel_fitness, rel_rmse,
                       device)


def _refine_many(cad, crops, poses, crop_normals, icp_threshold, max_iterations, dev):
    """The matchers' many(): every (crop, pose) pair with neither None goes through sv_icp_batched (independent problems,
    at most MAX_PROBLEMS per call), the others keep their pose, as the single calls do.  A crop object that appears several
    times is moved to the device once and, with crop_normals(k, device crop) given, gets its normals once."""
    if len(crops) != len(poses):
        raise ValueError(f"crops and poses must have the same length, got {len(crops)} and {len(poses)}")
    live = [k for k, (c, p) in enumerate(zip(crops, poses)) if c is not None and p is not None]
    for k in live:
        if len(_shape(crops[k])) != 2 or _shape(crops[k])[1] != 3:
            raise ValueError(f"crops[{k}] must be [N, 3], got {_shape(crops[k])}")
        _check_icp_args(cad.shape[0], _shape(crops[k])[0], _shape(crops[k])[0], icp_threshold, max_iterations)
    out = list(poses)
    if not live:
        return out
    moved = {}  # id(crop) -> (device crop, device normals or None)
    for k in live:
        if id(crops[k]) not in moved:
            tgt = _cloud(crops[k], "crops", dev)
            tn = crop_normals(k, tgt) if crop_normals is not None else None
            if tn is not None and tn.shape != tgt.shape:
                raise ValueError(f"normals[{k}] must hold one normal per crop point {tuple(tgt.shape)}, "
                                 f"got {tuple(tn.shape)}")
            moved[id(crops[k])] = (tgt, tn)
    init = _matrix(np.stack([get_transformation_matrix(np.asarray(poses[k], dtype=np.float64), switch_w=False)
                             for k in live]), dev)
    Ts = []
    for a in range(0, len(live), MAX_PROBLEMS):
        part = [moved[id(crops[k])] for k in live[a:a + MAX_PROBLEMS]]
        offsets = np.concatenate([[0], np.cumsum([t.shape[0] for t, _ in part])])
        tn = torch.cat([n for _, n in part]) if crop_normals is not None else None
        Ts.append(_icp_batched_enqueue(cad, torch.cat([t for t, _ in part]), tn, offsets, init[a:a + MAX_PROBLEMS],
                                       None, False, icp_threshold, max_iterations, 1e-6, 1e-6)[0])
    Ts = torch.cat(Ts).cpu().numpy()  # the one read-back
    for k, T in zip(live, Ts):
        out[k] = get_pose_from_matrix(T.reshape(4, 4))
    return out
