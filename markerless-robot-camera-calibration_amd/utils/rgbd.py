"""RGB-D frames: a depth image, a colour image and two intrinsic matrices, kept as the images the camera SDK hands over.

The reference turns them into a cloud on the host (scripts/ycb_generate_point_cloud.py:127-274: filterDiscontinuities,
registerDepthMap and registeredDepthMapToPointCloud, the last two as Python loops over every pixel); on the Kinect path
ROS depth_image_proc does it.  Here the images are uploaded as they are and `sv_rgbd_cloud` filters the raw depth,
registers it into the colour camera through a z-buffer and back-projects the registered map to an unorganised coloured
cloud with source indices (include/sv_hip.h N3f has the definitions and the order of the float64 arithmetic).
`decode_host` and `registered_host` restate those definitions in numpy.

Lens distortion (include/sv_hip.h N3g): a camera may carry the plumb-bob or rational coefficients of OpenCV and of a ROS
CameraInfo, D = (k1, k2, p1, p2, k3, k4, k5, k6).  `sv_lens_rays` inverts the model once per camera into a table of rays on
the device, which every frame of that camera shares, and `sv_rgbd_cloud_lens` back-projects along those rays and projects
through the forward model.  A frame without coefficients, or with all of them zero, takes `sv_rgbd_cloud` as before.

An RGBDFrame goes wherever a PackedFrame (utils/packed.py) goes: predict_segmentation_packed, the items of
predict_segmentation_stream, PackedCloudDTO(packed=...).  Its "records" are the colour image's pixels, j = v * Wc + u.
"""
from ctypes import c_double, c_int, c_int64, c_size_t, c_void_p

import numpy as np
import torch

from .. import _lib
from .._lib import call, ptr, stream_ptr
from .packed import check_box, color_table, device_lut_values

MAX_PIXELS = 1 << 24
FILTER_TILE = (8, 32)  # rows, columns of the filter kernel's tile (RG_TH, RG_TW of csrc/sv_rgbd.hip)
COMPACT_TILE = 256  # colour pixels per workgroup of the compaction (CP_THREADS of csrc/sv_compact.h)
KEEP = ("far", "near")
COLOR_ORDERS = ("rgb", "bgr")
_ENCODINGS = {"16UC1": (np.dtype("<u2"), 0.001), "32FC1": (np.dtype("<f4"), 1.0)}


def _rows(image, dtype, channels, what):
    """image -> an array of `dtype` [H, W] ([H, W, 3] for channels == 3) whose pixels are contiguous inside a row; the row
    stride is kept (a camera's `step`), anything else is copied"""
    a = np.asarray(image)
    if a.dtype != dtype:
        if dtype.kind == "u" and a.dtype.kind in "ui" and a.size and (a.min() < 0 or a.max() > np.iinfo(dtype).max):
            raise ValueError(f"{what} values do not fit {dtype}")
        a = a.astype(dtype)
    if a.ndim != (3 if channels == 3 else 2) or (channels == 3 and a.shape[2] != 3):
        raise ValueError(f"{what} must be [H, W{', 3' if channels == 3 else ''}], got {a.shape}")
    inner = (3 * dtype.itemsize, dtype.itemsize) if channels == 3 else (dtype.itemsize,)
    if a.strides[1:] != inner or a.strides[0] < a.shape[1] * channels * dtype.itemsize:
        a = np.ascontiguousarray(a)
    return a


def _K(K, what):
    K = np.asarray(K, dtype=np.float64).reshape(-1)
    if K.shape != (9,):
        raise ValueError(f"{what} must hold 9 values (a 3 x 3 intrinsic matrix)")
    return K.reshape(3, 3)


LENS_ROUNDS = 64  # rounds of the inverse model, no early exit (include/sv_hip.h N3g)
LENS_TOL = 1e-6  # pixels: a ray is valid iff the forward model brings it back to its pixel within this
DISTORTION_MODELS = ("plumb_bob", "rational_polynomial")
CAMERAS = ("depth", "color")
LENS_CACHE_SIZE = 8  # cameras whose tables are kept, on the host and on the device each
_host_tables, _device_tables = {}, {}
lens_table_builds = 0  # sv_lens_rays calls so far: a camera's frames share one table per device


def _D(D, what):
    """distortion coefficients -> float64 [8] (k1, k2, p1, p2, k3, k4, k5, k6), or None for a pinhole camera (no
    coefficients, or all of them zero)"""
    if D is None:
        return None
    D = np.asarray(D, dtype=np.float64).reshape(-1)
    if len(D) == 0:
        return None
    if len(D) not in (4, 5, 8):
        raise ValueError(f"{what} must hold 4, 5 or 8 coefficients (plumb-bob or rational), got {len(D)}: the thin-prism and "
                         f"tilted-sensor models are not supported")
    if not np.isfinite(D).all():
        raise ValueError(f"{what} must be finite")
    out = np.zeros(8)
    out[:len(D)] = D
    return out if out.any() else None


def _info_D(info, what):
    """D of a CameraInfo look-alike, read only when the attribute is there"""
    D = getattr(info, "D", None)
    if D is None or len(D) == 0 or not np.any(np.asarray(D, dtype=np.float64) != 0):
        return None
    model = getattr(info, "distortion_model", "plumb_bob")
    if model not in DISTORTION_MODELS:
        raise ValueError(f"{what}: distortion model {model!r} is not supported (only {', '.join(DISTORTION_MODELS)})")
    return D


def lens_forward(D, a, b):
    """the forward model F of include/sv_hip.h N3g: normalised direction (a, b) -> distorted normalised point (xd, yd)"""
    k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(x) for x in D)
    r2 = a * a + b * b
    num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2
    c = num / den
    dx = (2.0 * p1) * (a * b) + p2 * (r2 + 2.0 * (a * a))
    dy = p1 * (r2 + 2.0 * (b * b)) + (2.0 * p2) * (a * b)
    return a * c + dx, b * c + dy


def lens_rays_host(cam4, D, H, W):
    """the ray table sv_lens_rays writes, float64 [H * W * 2 + 1]: (x, y) per pixel, (NaN, NaN) where the inverse model
    does not come back to the pixel, then r2_max"""
    fx, fy, cx, cy = (np.float64(x) for x in cam4)
    k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(x) for x in D)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    with np.errstate(all="ignore"):
        x0, y0 = (u - cx) * (1.0 / fx), (v - cy) * (1.0 / fy)
        x, y = x0, y0
        for _ in range(LENS_ROUNDS):
            r2 = x * x + y * y
            ic = (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            dx = (2.0 * p1) * (x * y) + p2 * (r2 + 2.0 * (x * x))
            dy = p1 * (r2 + 2.0 * (y * y)) + (2.0 * p2) * (x * y)
            x, y = (x0 - dx) * ic, (y0 - dy) * ic
        xd, yd = lens_forward(D, x, y)
        valid = (np.abs((fx * xd + cx) - u) <= LENS_TOL) & (np.abs((fy * yd + cy) - v) <= LENS_TOL)
        r2 = (x * x + y * y)[valid]
    table = np.empty(H * W * 2 + 1)
    table[:-1] = np.stack((np.where(valid, x, np.nan), np.where(valid, y, np.nan)), axis=2).reshape(-1)
    table[-1] = r2.max() if len(r2) else 0.0
    return table


def _remember(cache, key, value):
    while len(cache) >= LENS_CACHE_SIZE:
        cache.pop(next(iter(cache)))
    cache[key] = value
    return value


class RGBDFrame:
    """One depth image ([Hd, Wd] uint16 or float32) with the colour image ([Hc, Wc, 3] uint8, or None) it belongs to.

    depth_K, color_K: 3 x 3 intrinsics.  color_from_depth: the 4 x 4 (or 3 x 4) transform from the depth camera's frame to
    the colour camera's; None = the depth image is already in the colour camera (aligned: no registration, the images have
    one size, and color_K defaults to depth_K).  depth_scale: metres (or whatever unit the cloud shall have) per depth
    unit.  mask: [Hc, Wc], a pixel with a non-zero value is dropped.  filter_size, filter_thresh: the discontinuity filter
    on raw uint16 depth (0 = off; the reference uses 7 and 1000).  keep: "far" keeps the largest depth where several
    depth pixels land on one colour pixel, which is what the reference does; "near" keeps the smallest.
    depth_D, color_D: distortion coefficients of the two cameras in the OpenCV / ROS order, 4, 5 (plumb-bob) or 8
    (rational) of them; None or all zeros = a pinhole camera.  In an aligned frame color_D defaults to depth_D as color_K
    does to depth_K, and the colour camera is the one used."""

    def __init__(self, depth, color, depth_K, color_K=None, color_from_depth=None, depth_scale=0.001, mask=None,
                 filter_size=0, filter_thresh=1000, keep="far", color_order="rgb", depth_D=None, color_D=None):
        d = np.asarray(depth)
        self.depth = _rows(d, np.dtype("<f4") if d.dtype.kind == "f" else np.dtype("<u2"), 1, "depth")
        self.depth_type = _lib.SV_DEPTH_F32 if self.depth.dtype.kind == "f" else _lib.SV_DEPTH_U16
        self.color = None if color is None else _rows(color, np.dtype("u1"), 3, "color")
        self.aligned = color_from_depth is None
        self.depth_K = _K(depth_K, "depth_K")
        self.color_K = self.depth_K if color_K is None else _K(color_K, "color_K")
        self.depth_D = _D(depth_D, "depth_D")
        self.color_D = _D(color_D, "color_D") if (color_D is not None or not self.aligned) else self.depth_D
        if self.aligned:
            self.H = np.eye(4)[:3]
        else:
            H = np.asarray(color_from_depth, dtype=np.float64)
            if H.shape not in ((4, 4), (3, 4)):
                raise ValueError("color_from_depth must be 4 x 4 or 3 x 4")
            self.H = np.ascontiguousarray(H[:3])
        self.depth_scale = float(depth_scale)
        self.Hd, self.Wd = self.depth.shape
        self.Hc, self.Wc = (self.Hd, self.Wd) if self.color is None else self.color.shape[:2]
        self.mask = None
        if mask is not None:
            m = np.asarray(mask)
            if m.shape != (self.Hc, self.Wc):
                raise ValueError(f"mask must be [{self.Hc}, {self.Wc}], got {m.shape}")
            self.mask = np.ascontiguousarray(m != 0).view(np.uint8)
        self.filter_size, self.filter_thresh = int(filter_size), int(filter_thresh)
        if keep not in KEEP:
            raise ValueError(f"keep must be one of {KEEP}, got {keep!r}")
        if color_order not in COLOR_ORDERS:
            raise ValueError(f"color_order must be one of {COLOR_ORDERS}, got {color_order!r}")
        self.keep, self.color_order = keep, color_order
        self._check()
        self._buf = self._registered = None

    def _check(self):
        if min(self.Hd, self.Wd, self.Hc, self.Wc) < 1:
            raise ValueError("an image needs at least one pixel")
        if self.Hd * self.Wd > MAX_PIXELS or self.Hc * self.Wc > MAX_PIXELS:
            raise ValueError("at most 2^24 pixels per image")
        if self.aligned and (self.Hd, self.Wd) != (self.Hc, self.Wc):
            raise ValueError("an aligned frame (color_from_depth=None) needs a depth and a colour image of one size")
        if self.filter_size != 0 and not (3 <= self.filter_size <= 15 and self.filter_size % 2 == 1):
            raise ValueError("filter_size must be 0 or odd and in 3..15")
        if self.filter_size != 0 and self.depth_type != _lib.SV_DEPTH_U16:
            raise ValueError("the discontinuity filter takes uint16 depth only")
        if self.filter_thresh < 0:
            raise ValueError("filter_thresh must not be negative")
        cam = self.cam()
        if not np.isfinite(cam).all():
            raise ValueError("intrinsics, transform and depth_scale must be finite")
        if (cam[[0, 1, 4, 5, 20]] == 0).any():
            raise ValueError("focal lengths and depth_scale must not be zero")

    def cam(self):
        """the double[21] of sv_rgbd_cloud: depth fx, fy, cx, cy; colour fx, fy, cx, cy; H rows; depth_scale"""
        kd, kc = self.depth_K, self.color_K
        return np.concatenate([[kd[0, 0], kd[1, 1], kd[0, 2], kd[1, 2], kc[0, 0], kc[1, 1], kc[0, 2], kc[1, 2]],
                               self.H.reshape(-1), [self.depth_scale]]).astype(np.float64)

    @property
    def has_lens(self):
        """whether a camera this frame uses is distorted (an aligned frame uses the colour camera only)"""
        return self.color_D is not None or (self.depth_D is not None and not self.aligned)

    def _lens_camera(self, which):
        """(fx, fy, cx, cy), D or None, H, W of the "depth" or the "color" camera"""
        if which not in CAMERAS:
            raise ValueError(f"which must be one of {CAMERAS}, got {which!r}")
        K, D, H, W = ((self.depth_K, self.depth_D, self.Hd, self.Wd) if which == "depth" else
                      (self.color_K, self.color_D, self.Hc, self.Wc))
        return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]]), D, H, W

    @staticmethod
    def _lens_key(cam4, D, H, W):
        return np.concatenate([cam4, D, [H, W]]).astype(np.float64).tobytes()

    def rays_host(self, which="color"):
        """the ray table of the "depth" or the "color" camera as sv_lens_rays defines it (lens_rays_host; shared by the
        frames of one camera), or None for a pinhole camera.  A lens without a single valid pixel is refused."""
        cam4, D, H, W = self._lens_camera(which)
        if D is None:
            return None
        key = self._lens_key(cam4, D, H, W)
        table = _host_tables.get(key)
        if table is None:
            table = lens_rays_host(cam4, D, H, W)
            if np.isnan(table[:-1]).all():
                raise ValueError(f"the {which} camera's distortion model has no valid pixel: the inverse model comes back "
                                 f"to no pixel of the {H} x {W} image within {LENS_TOL} px")
            table.setflags(write=False)
            _remember(_host_tables, key, table)
        return table

    def rays_device(self, which, device):
        """the same table on `device`, built on first use by sv_lens_rays on the current stream and waited for: set-up
        work, once per camera and device.  None for a pinhole camera."""
        global lens_table_builds
        cam4, D, H, W = self._lens_camera(which)
        if D is None:
            return None
        device = torch.device(device)
        index = torch.cuda.current_device() if device.index is None else device.index
        key = (self._lens_key(cam4, D, H, W), device.type, index)
        table = _device_tables.get(key)
        if table is None:
            table = torch.empty(H * W * 2 + 1, dtype=torch.float64, device=device)
            call("sv_lens_rays", (c_double * 4)(*cam4), (c_double * 8)(*D), c_int64(H), c_int64(W), ptr(table), stream_ptr())
            lens_table_builds += 1
            torch.cuda.current_stream(device).synchronize()
            valid, r2_max = int((table[:-1:2] == table[:-1:2]).sum().item()), float(table[-1].item())
            if valid == 0:
                raise ValueError(f"the {which} camera's distortion model has no valid pixel (r2_max {r2_max}): the inverse "
                                 f"model comes back to no pixel of the {H} x {W} image within {LENS_TOL} px")
            _remember(_device_tables, key, table)
        return table

    def flags(self):
        return ((_lib.SV_RGBD_ALIGNED if self.aligned else 0) | (_lib.SV_RGBD_NEAREST if self.keep == "near" else 0) |
                (_lib.SV_RGBD_BGR if self.color_order == "bgr" else 0))

    # ---- constructors ---------------------------------------------------------------------------------------------
    @classmethod
    def from_image_msgs(cls, depth_msg, color_msg, depth_info, color_info=None, color_from_depth=None, depth_scale=None,
                        **kw):
        """Any objects with the attributes of sensor_msgs/Image (height, width, encoding, is_bigendian, step, data) and of
        sensor_msgs/CameraInfo (K).  Depth encodings: 16UC1 (depth_scale 0.001: millimetres) and 32FC1 (1.0: metres);
        colour encodings: rgb8 and bgr8.  `step` becomes the row bytes; the pixel data is not copied here.  An info object
        that also has D and distortion_model gives the camera its lens: "plumb_bob" and "rational_polynomial" are taken, an
        empty or all-zero D is a pinhole camera, any other model with a non-zero D is refused."""

        def image(msg, dtype, channels, what):
            if msg.is_bigendian and dtype.itemsize > 1:
                raise ValueError(f"big-endian {what} images are not supported")
            h, w, step = int(msg.height), int(msg.width), int(msg.step)
            row = w * channels * dtype.itemsize
            if h < 1 or w < 1 or step < row:
                raise ValueError(f"the {what} image needs height, width >= 1 and step >= {row}")
            data = msg.data if isinstance(msg.data, np.ndarray) else np.frombuffer(msg.data, dtype=np.uint8)
            if data.dtype != np.uint8 or data.ndim != 1 or len(data) < (h - 1) * step + row:
                raise ValueError(f"the {what} image's data must be flat bytes covering height rows of step bytes")
            shape, inner = ((h, w, 3), (3, 1)) if channels == 3 else ((h, w), (dtype.itemsize,))
            return np.ndarray(shape=shape, dtype=dtype, buffer=data, strides=(step,) + inner)

        if depth_msg.encoding not in _ENCODINGS:
            raise ValueError(f"depth encoding must be one of {sorted(_ENCODINGS)}, got {depth_msg.encoding!r}")
        dtype, scale = _ENCODINGS[depth_msg.encoding]
        depth = image(depth_msg, dtype, 1, "depth")
        color = None
        if color_msg is not None:
            if color_msg.encoding not in ("rgb8", "bgr8"):
                raise ValueError(f"colour encoding must be 'rgb8' or 'bgr8', got {color_msg.encoding!r}")
            color = image(color_msg, np.dtype("u1"), 3, "colour")
            kw.setdefault("color_order", color_msg.encoding[:3])
        if "depth_D" not in kw:
            kw["depth_D"] = _info_D(depth_info, "depth_info")
        if "color_D" not in kw and color_info is not None:
            kw["color_D"] = _info_D(color_info, "color_info")
        return cls(depth, color, depth_info.K, None if color_info is None else color_info.K, color_from_depth,
                   scale if depth_scale is None else depth_scale, **kw)

    # ---- what PackedFrameStream and the engine read -------------------------------------------------------------------
    @property
    def height(self):
        return self.Hc

    @property
    def width(self):
        return self.Wc

    @property
    def n_records(self):
        return self.Hc * self.Wc

    @property
    def depth_row_bytes(self):
        return self.depth.strides[0]

    @property
    def color_row_bytes(self):
        return 0 if self.color is None else self.color.strides[0]

    @property
    def depth_nbytes(self):
        return (self.Hd - 1) * self.depth_row_bytes + self.Wd * self.depth.dtype.itemsize

    @property
    def color_nbytes(self):
        return 0 if self.color is None else (self.Hc - 1) * self.color_row_bytes + 3 * self.Wc

    @property
    def rgb_offset(self):
        """byte offset of the colour rows in _bytes(), -1 without a colour image"""
        return -1 if self.color is None else self.depth_nbytes

    @property
    def nbytes_used(self):
        return self.depth_nbytes + self.color_nbytes + (0 if self.mask is None else self.n_records)

    def _bytes(self):
        """depth rows, colour rows, mask, in one uint8 buffer (built once; bytes between rows are zero)"""
        if self._buf is None:
            buf = np.zeros(self.nbytes_used, dtype=np.uint8)
            np.ndarray(shape=self.depth.shape, dtype=self.depth.dtype, buffer=buf,
                       strides=self.depth.strides)[...] = self.depth
            if self.color is not None:
                np.ndarray(shape=self.color.shape, dtype=np.uint8, buffer=buf, offset=self.depth_nbytes,
                           strides=self.color.strides)[...] = self.color
            if self.mask is not None:
                buf[self.depth_nbytes + self.color_nbytes:] = self.mask.reshape(-1)
            self._buf = buf
        return self._buf

    # ---- host decoding (the definitions of include/sv_hip.h N3f in numpy) ---------------------------------------------
    def filtered_host(self):
        """the depth values after stage 1, as float64 (before depth_scale)"""
        if self.depth_type == _lib.SV_DEPTH_F32:
            f = self.depth
            return np.where(np.isfinite(f) & (f > 0), f, np.float32(0)).astype(np.float64)
        raw = self.depth.astype(np.int64)
        n, o = self.filter_size, self.filter_size // 2
        if n and self.Hd >= n and self.Wd >= n:
            win = np.lib.stride_tricks.sliding_window_view(raw, (n, n))
            mid = raw[o:self.Hd - o, o:self.Wd - o]
            mark = np.maximum(mid - win.min(axis=(2, 3)), win.max(axis=(2, 3)) - mid) > self.filter_thresh
            raw = raw.copy()
            raw[o:self.Hd - o, o:self.Wd - o][mark] = 0
        return raw.astype(np.float64)

    def registered_host(self):
        """the registered depth map, float64 [Hc, Wc] (cached)"""
        if self._registered is not None:
            return self._registered
        d = self.filtered_host() * np.float64(self.depth_scale)
        if self.aligned:
            self._registered = d
            return d
        cam, H = self.cam(), self.H
        v, u = np.nonzero(d != 0)
        d = d[v, u]
        with np.errstate(all="ignore"):
            if self.depth_D is not None:
                rays = self.rays_host("depth")[:-1].reshape(self.Hd, self.Wd, 2)
                x, y = rays[v, u, 0] * d, rays[v, u, 1] * d
            else:
                x = ((u - cam[2]) * d) * (1.0 / cam[0])
                y = ((v - cam[3]) * d) * (1.0 / cam[1])
            z = d
            X = ((H[0, 0] * x + H[0, 1] * y) + H[0, 2] * z) + H[0, 3]
            Y = ((H[1, 0] * x + H[1, 1] * y) + H[1, 2] * z) + H[1, 3]
            Z = ((H[2, 0] * x + H[2, 1] * y) + H[2, 2] * z) + H[2, 3]
            iz = 1.0 / Z
            if self.color_D is not None:
                a, b = X * iz, Y * iz
                xd, yd = lens_forward(self.color_D, a, b)
                ui = np.trunc(cam[4] * xd + cam[6] + 0.5)
                vi = np.trunc(cam[5] * yd + cam[7] + 0.5)
                inside = a * a + b * b <= self.rays_host("color")[-1]  # the radial fold-back bound; False for a NaN
            else:
                ui = np.trunc((cam[4] * X) * iz + cam[6] + 0.5)
                vi = np.trunc((cam[5] * Y) * iz + cam[7] + 0.5)
                inside = True
            ok = (ui >= 0) & (ui < self.Wc) & (vi >= 0) & (vi < self.Hc) & (Z > 0) & np.isfinite(Z) & inside
        idx = vi[ok].astype(np.int64) * self.Wc + ui[ok].astype(np.int64)
        if self.keep == "far":
            reg = np.zeros(self.Hc * self.Wc, dtype=np.float64)
            np.maximum.at(reg, idx, Z[ok])
        else:
            reg = np.full(self.Hc * self.Wc, np.inf)
            np.minimum.at(reg, idx, Z[ok])
            reg[np.isinf(reg)] = 0.0
        self._registered = reg.reshape(self.Hc, self.Wc)
        return self._registered

    def _cloud_host(self, box, idx=None):
        """(points64 [k, 3], points float32 [k, 3], src int64 [k]) of the kept pixels, or of the pixels idx unfiltered"""
        cam = self.cam()
        r = self.registered_host().reshape(-1)
        j = np.arange(self.n_records) if idx is None else idx
        r = r[j]
        v, u = j // self.Wc, j % self.Wc
        with np.errstate(all="ignore"):
            p64 = self._backproject_host(cam, u, v, j, r)
            p32 = p64.astype(np.float32)
            if idx is not None:
                return p64, p32, j
            keep = r > 0
            if self.color_D is not None:
                keep &= ~np.isnan(self.rays_host("color")[:-1:2])  # the pixel's ray is valid
            if self.mask is not None:
                keep &= self.mask.reshape(-1) == 0
            if box is not None:
                w = p32.astype(np.float64)
                keep &= np.all((box[:3] < w) & (w < box[3:]), axis=1)
        src = np.nonzero(keep)[0]
        return p64[src], p32[src], src

    def _backproject_host(self, cam, u, v, j, r):
        """stage 3's points64 of the colour pixels j = v * Wc + u with registered depth r"""
        if self.color_D is not None:
            rays = self.rays_host("color")[:-1].reshape(-1, 2)[j]
            return np.stack((rays[:, 0] * r, rays[:, 1] * r, r), axis=1)
        return np.stack((((u - cam[6]) * r) * (1.0 / cam[4]), ((v - cam[7]) * r) * (1.0 / cam[5]), r), axis=1)

    def _colors_host(self, src, color, lut):
        if self.color is None:
            return None
        table = color_table(color) if lut is None else np.asarray(lut)
        v, u = src // self.Wc, src % self.Wc
        c = self.color[v, u]
        return table[c[:, ::-1] if self.color_order == "bgr" else c]

    def decode_host(self, box=None, color="float64", lut=None):
        """-> (points float32 [k, 3], rgb [k, 3] or None, src int64 [k]): the kept colour pixels in ascending j, as
        sv_rgbd_cloud defines them.  rgb = lut[bytes] when a 256-entry lut is given, else the convention `color`
        (utils/packed.py)."""
        box = check_box(box)
        if lut is None:
            color_table(color)  # rejects an unknown convention, with or without a colour image
        _, p32, src = self._cloud_host(box)
        return p32, self._colors_host(src, color, lut), src

    def decode_host64(self, box=None):
        """-> (points float64 [k, 3], src int64 [k]): decode_host's points before the rounding to float32"""
        p64, _, src = self._cloud_host(check_box(box))
        return p64, src

    def take(self, src_idx, color="float64", lut=None):
        """-> (points float32 [m, 3], rgb [m, 3] or None) of the colour pixels src_idx only.  An aligned frame without the
        filter reads those pixels directly; any other frame runs the host registration (once, cached): a pixel's
        registered depth depends on the whole depth image."""
        idx = np.asarray(src_idx, dtype=np.int64).reshape(-1)
        if len(idx) and (idx.min() < 0 or idx.max() >= self.n_records):
            raise IndexError("pixel index outside the colour image")
        if self.aligned and self.filter_size == 0 and self._registered is None:
            cam = self.cam()
            v, u = idx // self.Wc, idx % self.Wc
            raw = self.depth[v, u]
            if self.depth_type == _lib.SV_DEPTH_F32:
                raw = np.where(np.isfinite(raw) & (raw > 0), raw, np.float32(0))
            r = raw.astype(np.float64) * np.float64(self.depth_scale)
            with np.errstate(all="ignore"):
                p32 = self._backproject_host(cam, u, v, idx, r).astype(np.float32)
        else:
            _, p32, _ = self._cloud_host(None, idx)
        return p32, self._colors_host(idx, color, lut)

    def scatter(self, labels, src, fill=-1):
        """per-point labels of the kept pixels -> an [Hc, Wc] image, `fill` where nothing was kept"""
        labels, src = np.asarray(labels), np.asarray(src, dtype=np.int64)
        if labels.shape != src.shape:
            raise ValueError("labels and src must have the same length")
        out = np.full(self.n_records, fill, dtype=labels.dtype)
        out[src] = labels
        return out.reshape(self.Hc, self.Wc)

    # ---- device decoding --------------------------------------------------------------------------------------------
    def unpack(self, d_bytes, box=None, lut=None, want_src=True, want_points64=False, want_registered=False):
        """sv_rgbd_cloud (sv_rgbd_cloud_lens with the cameras' cached ray tables when the frame has a lens: the first frame
        of a camera on a device builds them and waits, rays_device) on this frame's bytes (_bytes()) already on the device
        (uint8 CUDA tensor), on the current stream.
        -> (points [n, 3], rgb [n, 3] or None, src int32 [n] or None, count int64 [1]), n = Hc * Wc, all on the device and
        NOT sliced: rows at or beyond count are unspecified.  Nothing is read back.  want_points64 / want_registered append
        the float64 points [n, 3] / the registered map [Hc, Wc] to the tuple."""
        box = check_box(box)
        n = self.n_records
        if lut is not None and (lut.dtype != torch.float32 or lut.numel() != 256 or not lut.is_contiguous()):
            raise ValueError("lut must be a contiguous float32 tensor of 256 values")
        _lib.require_cuda(d_bytes, "the frame's bytes")
        if d_bytes.dtype != torch.uint8 or d_bytes.dim() != 1 or d_bytes.numel() < self.nbytes_used:
            raise ValueError("d_bytes must be a flat uint8 tensor covering the depth rows, the colour rows and the mask")
        dev = d_bytes.device
        ws_bytes = _lib.load().sv_rgbd_cloud_workspace_bytes(c_int64(self.Hd), c_int64(self.Wd), c_int64(self.Hc),
                                                             c_int64(self.Wc))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        points = torch.empty((n, 3), dtype=torch.float32, device=dev)
        rgb = torch.empty((n, 3), dtype=torch.float32, device=dev) if self.color is not None else None
        src = torch.empty(n, dtype=torch.int32, device=dev) if want_src else None
        count = torch.empty(1, dtype=torch.int64, device=dev)
        points64 = torch.empty((n, 3), dtype=torch.float64, device=dev) if want_points64 else None
        registered = torch.empty((self.Hc, self.Wc), dtype=torch.float64, device=dev) if want_registered else None
        base = d_bytes.data_ptr()
        d_color = c_void_p(base + self.depth_nbytes) if self.color is not None else None
        d_mask = c_void_p(base + self.depth_nbytes + self.color_nbytes) if self.mask is not None else None
        args = (c_void_p(base), c_int(self.depth_type), c_int64(self.Hd), c_int64(self.Wd),
                c_int64(self.depth_row_bytes), d_color, c_int64(self.Hc), c_int64(self.Wc), c_int64(self.color_row_bytes),
                d_mask, (c_double * 21)(*self.cam()), c_int(self.filter_size), c_int(self.filter_thresh), c_int(self.flags()),
                None if box is None else (c_double * 6)(*box), ptr(lut), ptr(ws), c_size_t(ws_bytes), ptr(points),
                ptr(points64), ptr(rgb), ptr(src), ptr(registered), ptr(count))
        if self.has_lens:
            depth_rays = None if self.aligned else self.rays_device("depth", dev)
            color_rays = self.rays_device("color", dev)
            dist = None if (self.aligned or self.color_D is None) else (c_double * 8)(*self.color_D)
            call("sv_rgbd_cloud_lens", *args, ptr(depth_rays), ptr(color_rays), dist, stream_ptr())
        else:
            call("sv_rgbd_cloud", *args, stream_ptr())
        out = (points, rgb, src, count)
        if want_points64:
            out += (points64,)
        if want_registered:
            out += (registered,)
        return out

    def decode_device(self, device, box=None, lut=None, stream=None):
        """Upload the images, decode on the device -> (points float32 [k, 3], rgb float32 [k, 3] or None, src int32 [k]) as
        CUDA tensors sliced to the number kept (one 8-byte read-back).  lut: None (byte values), a convention name
        ("float64", "float32": the engine's normalised colours, utils/packed.py device_lut_values) or a float32 CUDA tensor
        of 256 values."""
        box = check_box(box)
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.SvHipError(f"decode_device needs a GPU (got {device}); the HIP path has no CPU fallback")
        if isinstance(lut, str):
            values = device_lut_values(lut)
        host = torch.empty(self.nbytes_used, dtype=torch.uint8)
        host.numpy()[:] = self._bytes()
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(device)):
            if isinstance(lut, str):
                lut = torch.from_numpy(values).to(device)
            d_bytes = host.to(device)
            points, rgb, src, count = self.unpack(d_bytes, box=box, lut=lut)
            k = int(count.item())
        return points[:k], (None if rgb is None else rgb[:k]), src[:k]
