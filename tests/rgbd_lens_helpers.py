"""Helpers of the lens-distortion tests: an independent numpy restatement of include/sv_hip.h N3g (forward model, ray table)
that shares no code with mrcc_amd/utils/rgbd.py, the cameras the tests use, and a direct caller of sv_lens_rays and
sv_rgbd_cloud_lens."""
import ctypes
import json
import os

import numpy as np

ROUNDS, TOL = 64, 1e-6
NAN = float("nan")


def pad8(D):
    out = np.zeros(8)
    out[:len(D)] = D
    return out


def forward(D, a, b):
    """F(a, b) -> (xd, yd), float64, every operation on its own"""
    k1, k2, p1, p2, k3, k4, k5, k6 = [np.float64(x) for x in pad8(D)]
    r2 = a * a + b * b
    num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2
    c = num / den
    ab = a * b
    dx = (2.0 * p1) * ab + p2 * (r2 + 2.0 * (a * a))
    dy = p1 * (r2 + 2.0 * (b * b)) + (2.0 * p2) * ab
    return a * c + dx, b * c + dy


def ray_table(K, D, H, W, rounds=ROUNDS):
    """-> (rays float64 [H, W, 2] with NaN at invalid pixels, valid bool [H, W], r2_max, residual in pixels [H, W])"""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    k1, k2, p1, p2, k3, k4, k5, k6 = [np.float64(x) for x in pad8(D)]
    u = np.tile(np.arange(W, dtype=np.float64), (H, 1))
    v = np.tile(np.arange(H, dtype=np.float64)[:, None], (1, W))
    with np.errstate(all="ignore"):
        x0 = (u - cx) * (1.0 / fx)
        y0 = (v - cy) * (1.0 / fy)
        x, y = x0.copy(), y0.copy()
        for _ in range(rounds):
            r2 = x * x + y * y
            ic = (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            xy = x * y
            dx = (2.0 * p1) * xy + p2 * (r2 + 2.0 * (x * x))
            dy = p1 * (r2 + 2.0 * (y * y)) + (2.0 * p2) * xy
            x = (x0 - dx) * ic
            y = (y0 - dy) * ic
        xd, yd = forward(D, x, y)
        eu, ev = np.abs((fx * xd + cx) - u), np.abs((fy * yd + cy) - v)
        valid = (eu <= TOL) & (ev <= TOL)
        r2 = x * x + y * y
    rays = np.full((H, W, 2), NAN)
    rays[valid, 0], rays[valid, 1] = x[valid], y[valid]
    r2_max = float(r2[valid].max()) if valid.any() else 0.0
    return rays, valid, r2_max, np.maximum(eu, ev)


def flat_table(K, D, H, W):
    """the double[H * W * 2 + 1] sv_lens_rays writes"""
    rays, _, r2_max, _ = ray_table(K, D, H, W)
    return np.concatenate([rays.reshape(-1), [r2_max]])


def _K(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])


def kinect1():
    """the reference's Kinect 1 colour camera scaled to 64 x 48 (K times 0.1; D is dimensionless)"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kinect1_rgb_camera.json")) as f:
        cam = json.load(f)
    K = np.array(cam["K"], dtype=np.float64).reshape(3, 3) * 0.1
    K[2, 2] = 1.0
    return K, np.array(cam["D"], dtype=np.float64), 48, 64


RATIONAL_D = (5.6, 3.6, 3.2e-4, -1.1e-4, 0.18, 5.93, 5.44, 1.0)  # an Azure-Kinect-like depth lens
BARREL_D = (-0.25, 0.05, 1e-3, -1e-3, 0.0)  # strong but invertible at f = 40 on 64 x 48
FOLD_D = (-0.5, 0.0, 0.0, 0.0)  # r * (1 - 0.5 r^2) turns back at r^2 = 2/3: most of this image has no ray


def barrel_K(H, W, f=40.0):
    return _K(f, f, (W - 1) / 2.0, (H - 1) / 2.0)


def cases():
    """name -> (K, D, H, W): the four cameras of the table tests"""
    return {
        "kinect1": kinect1(),
        "rational": (_K(50.4, 50.4, 31.5, 28.5), np.array(RATIONAL_D), 58, 64),
        "tiny": (_K(4.0, 4.5, 2.2, 0.9), np.array(BARREL_D), 3, 5),
        "fold": (_K(20.0, 20.0, 31.5, 23.5), np.array(FOLD_D), 48, 64),
    }


FOLD_VALID, FOLD_INVALID = 376, 2696  # of the 64 x 48 "fold" camera, counted with this file's ray_table

ALL_VALID = ("kinect1", "rational", "tiny")


def camera_info(K, D=None, model=None):
    from types import SimpleNamespace

    info = SimpleNamespace(K=tuple(float(x) for x in np.asarray(K).reshape(-1)))
    if D is not None:
        info.D = tuple(float(x) for x in D)
    if model is not None:
        info.distortion_model = model
    return info


# ---- direct callers (GPU) -----------------------------------------------------------------------------------------------
def lens_rays(K, D, H, W, device):
    """sv_lens_rays -> the table as a numpy array; the buffer starts as a pattern no table holds and carries a guard"""
    import torch

    from mrcc_amd._lib import call, ptr, stream_ptr

    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    n = H * W * 2 + 1
    buf = torch.full((n + 8,), -7.5, dtype=torch.float64, device=device)
    call("sv_lens_rays", (ctypes.c_double * 4)(K[0, 0], K[1, 1], K[0, 2], K[1, 2]), (ctypes.c_double * 8)(*pad8(D)),
         ctypes.c_int64(H), ctypes.c_int64(W), ptr(buf), stream_ptr())
    out = buf.cpu().numpy()
    assert (out[n:] == -7.5).all(), "sv_lens_rays wrote beyond its table"
    return out[:n]


def cloud(frame, device, entry="sv_rgbd_cloud_lens", box=None, lut=None, tables=None):
    """sv_rgbd_cloud_lens (or sv_rgbd_cloud) on `frame` -> dict of device tensors (points, points64, rgb, src, registered,
    count), not sliced.  tables: (depth_rays, color_rays, dist) to pass, device tensors / 8 floats or None each; default: what
    the frame's own lens asks for, from this file's flat_table."""
    import torch

    import mrcc_amd
    from mrcc_amd._lib import call, ptr, stream_ptr

    n = frame.Hc * frame.Wc
    d_bytes = torch.from_numpy(frame._bytes()).to(device)
    base = d_bytes.data_ptr()
    d_color = ctypes.c_void_p(base + frame.depth_nbytes) if frame.color is not None else None
    d_mask = ctypes.c_void_p(base + frame.depth_nbytes + frame.color_nbytes) if frame.mask is not None else None
    ws_bytes = mrcc_amd._lib.load().sv_rgbd_cloud_workspace_bytes(frame.Hd, frame.Wd, frame.Hc, frame.Wc)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    out = dict(points=torch.full((n, 3), -7.5, dtype=torch.float32, device=device),
               points64=torch.full((n, 3), -7.5, dtype=torch.float64, device=device),
               rgb=torch.full((n, 3), -7.5, dtype=torch.float32, device=device) if frame.color is not None else None,
               src=torch.full((n,), -7, dtype=torch.int32, device=device),
               registered=torch.full((n,), -7.5, dtype=torch.float64, device=device),
               count=torch.full((1,), -7, dtype=torch.int64, device=device))
    d_lut = None if lut is None else torch.from_numpy(np.asarray(lut, dtype=np.float32)).to(device)
    args = [ctypes.c_void_p(base), frame.depth_type, frame.Hd, frame.Wd, frame.depth_row_bytes, d_color, frame.Hc, frame.Wc,
            frame.color_row_bytes, d_mask, (ctypes.c_double * 21)(*frame.cam()), frame.filter_size, frame.filter_thresh,
            frame.flags(), None if box is None else (ctypes.c_double * 6)(*box), ptr(d_lut), ptr(ws), ws_bytes,
            ptr(out["points"]), ptr(out["points64"]), ptr(out["rgb"]), ptr(out["src"]), ptr(out["registered"]),
            ptr(out["count"])]
    if entry == "sv_rgbd_cloud_lens":
        if tables is None:
            up = lambda K, D, H, W: torch.from_numpy(flat_table(K, D, H, W)).to(device)  # noqa: E731
            depth_rays = None if (frame.aligned or frame.depth_D is None) else up(frame.depth_K, frame.depth_D, frame.Hd,
                                                                                  frame.Wd)
            color_rays = None if frame.color_D is None else up(frame.color_K, frame.color_D, frame.Hc, frame.Wc)
            dist = None if (frame.aligned or frame.color_D is None) else frame.color_D
            tables = (depth_rays, color_rays, dist)
        depth_rays, color_rays, dist = tables
        args += [ptr(depth_rays), ptr(color_rays), None if dist is None else (ctypes.c_double * 8)(*dist)]
    call(entry, *args, stream_ptr())
    return out


def sliced(out):
    """cloud()'s dict as numpy arrays cut to the count"""
    k = int(out["count"].item())
    host = {name: (None if t is None else t.cpu().numpy()) for name, t in out.items()}
    for name in ("points", "points64", "rgb", "src"):
        if host[name] is not None:
            host[name] = host[name][:k]
    host["count"] = k
    return host
