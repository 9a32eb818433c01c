"""Packed sensor frames: a ROS PointCloud2 message or the body of a binary .pcd file, kept as the bytes they arrive in.

Both are a strided array of fixed-layout records (record i at (i // width) * row_step + (i % width) * point_step).  The
reference turns them into two host arrays per frame (utils/ros_utils.py get_points_and_colors for the depth camera,
Open3D's reader in app/data_engine.py PCDDataEngine); here the raw bytes are uploaded once and `sv_unpack_points` decodes
the fields, drops the non-finite and out-of-box records in order, unpacks the colour and hands points, colours and source
indices to the pipeline (include/sv_hip.h N3e has the definitions).  `decode_host` restates those definitions in numpy.

Colour conventions (the reference has two): "float64" = byte / 255 in float64 (the freenect engine), "float32" =
float32(byte / 255) (PCDDataEngine, which casts Open3D's float64 colours); "bytes" = the byte values themselves (what
get_points_and_colors returns).
"""
import os
from collections import namedtuple
from ctypes import c_double, c_int, c_int64, c_size_t

import numpy as np
import torch

from .. import _lib
from .._lib import call, ptr, stream_ptr
from . import preprocess

# sensor_msgs/PointField datatype codes (rospy is not needed)
INT8, UINT8, INT16, UINT16, INT32, UINT32, FLOAT32, FLOAT64 = 1, 2, 3, 4, 5, 6, 7, 8
FIELD_DTYPES = {INT8: np.dtype("int8"), UINT8: np.dtype("uint8"), INT16: np.dtype("int16"), UINT16: np.dtype("uint16"),
                INT32: np.dtype("int32"), UINT32: np.dtype("uint32"), FLOAT32: np.dtype("float32"),
                FLOAT64: np.dtype("float64")}
_PCD_CODES = {("I", 1): INT8, ("U", 1): UINT8, ("I", 2): INT16, ("U", 2): UINT16, ("I", 4): INT32, ("U", 4): UINT32,
              ("F", 4): FLOAT32, ("F", 8): FLOAT64}
MAX_RECORDS = 1 << 24
MAX_POINT_STEP = 4096
COLORS = ("float64", "float32", "bytes")
DEFAULT_BOX = (-500.0, -500.0, -500.0, 500.0, 500.0, 500.0)  # get_roi_mask's defaults

Field = namedtuple("Field", "name offset datatype count", defaults=(1,))

# layouts PackedFrame.pack knows by name
LAYOUTS = {
    # the depth camera's organised cloud: x y z, 4 bytes of padding, rgb, 12 bytes of padding
    "kinect": {"point_step": 32, "x": 0, "y": 4, "z": 8, "rgb": 16, "xyz_type": FLOAT32, "rgb_type": FLOAT32},
    # what PCL writes for PointXYZRGB
    "pcd": {"point_step": 16, "x": 0, "y": 4, "z": 8, "rgb": 12, "xyz_type": FLOAT32, "rgb_type": FLOAT32},
}


def color_table(color):
    """the 256 values a colour byte can take under a convention"""
    if color == "float64":
        return np.arange(256, dtype=np.float64) / 255.0
    if color == "float32":
        return (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    if color == "bytes":
        return np.arange(256, dtype=np.uint8)
    raise ValueError(f"color must be one of {COLORS}, got {color!r}")


def normalized_color_table(color):
    """preprocess.normalize_colors of a convention's 256 values, in the convention's dtype.  Byte colours always land in
    [0, 1], so normalize_colors takes the same `- 0.5` branch for every frame and this table equals the per-frame result."""
    if color not in ("float64", "float32"):
        raise ValueError(f"color must be 'float64' or 'float32' here (the engine's conventions), got {color!r}")
    return preprocess.normalize_colors(color_table(color).reshape(256, 1)).reshape(256)


def device_lut_values(color):
    """the device table: the normalised colours rounded to float32 the way the staging copy rounds them"""
    return normalized_color_table(color).astype(np.float32)


def check_box(box):
    """box -> float64[6] (lo xyz, hi xyz) or None; NaN bounds and lo > hi are rejected"""
    if box is None:
        return None
    b = np.asarray(box, dtype=np.float64).reshape(-1)
    if b.shape != (6,):
        raise ValueError("box must hold 6 values: lo x, y, z, hi x, y, z")
    if np.isnan(b).any():
        raise ValueError("box bounds must not be NaN")
    if (b[:3] > b[3:]).any():
        raise ValueError("box needs lo <= hi on every axis")
    return b


class PackedFrame:
    """The raw records of one frame and their layout.  `data` (bytes, memoryview or a uint8 array) is never copied on
    construction."""

    def __init__(self, data, width, height, point_step, row_step, fields, is_bigendian=False):
        self.data = data
        self.width, self.height = int(width), int(height)
        self.point_step, self.row_step = int(point_step), int(row_step)
        self.is_bigendian = bool(is_bigendian)
        self.fields = [f if isinstance(f, Field) else Field(f.name, int(f.offset), int(f.datatype), int(getattr(f, "count", 1)))
                       for f in fields]
        self._check_layout()

    # ---- layout ---------------------------------------------------------------------------------------------------
    def _check_layout(self):
        if self.width < 0 or self.height < 0:
            raise ValueError("width and height must not be negative")
        if self.n_records > MAX_RECORDS:
            raise ValueError(f"at most 2^24 records per frame, got {self.n_records}")
        if not 1 <= self.point_step <= MAX_POINT_STEP:
            raise ValueError(f"point_step must lie in [1, {MAX_POINT_STEP}], got {self.point_step}")
        if self.row_step < self.width * self.point_step:
            raise ValueError(f"row_step {self.row_step} is smaller than width * point_step")
        by_name = {}
        for f in self.fields:
            if f.datatype not in FIELD_DTYPES:
                raise ValueError(f"field {f.name!r} has unknown datatype {f.datatype}")
            by_name[f.name] = f
        spans = []
        for name in "xyz":
            f = by_name.get(name)
            if f is None or f.count != 1:
                raise ValueError(f"no scalar field {name!r}")
            if f.datatype not in (FLOAT32, FLOAT64):
                raise ValueError(f"field {name!r} must be FLOAT32 or FLOAT64")
            spans.append((name, f.offset, FIELD_DTYPES[f.datatype].itemsize))
        if len({by_name[n].datatype for n in "xyz"}) != 1:
            raise ValueError("fields x, y and z must share one datatype")
        self.xyz_type = by_name["x"].datatype
        self.xyz_offsets = tuple(by_name[n].offset for n in "xyz")
        rgb = by_name.get("rgb") or by_name.get("rgba")
        self.rgb_offset = -1
        if rgb is not None:
            if rgb.count != 1 or FIELD_DTYPES[rgb.datatype].itemsize != 4:
                raise ValueError("the rgb field must be one 4-byte value")
            self.rgb_offset = rgb.offset
            spans.append(("rgb", rgb.offset, 4))
        for name, off, size in spans:
            if off < 0 or off + size > self.point_step:
                raise ValueError(f"field {name!r} lies outside the {self.point_step}-byte record")
        for i, (na, oa, sa) in enumerate(spans):
            for nb, ob, sb in spans[i + 1:]:
                if not (oa + sa <= ob or ob + sb <= oa):
                    raise ValueError(f"fields {na!r} and {nb!r} overlap")
        if self.n_records and self.nbytes_used > len(self._bytes()):
            raise ValueError(f"data holds {len(self._bytes())} bytes, the last record ends at {self.nbytes_used}")

    @property
    def n_records(self):
        return self.width * self.height

    @property
    def nbytes_used(self):
        """bytes up to the end of the last record"""
        if self.n_records == 0:
            return 0
        return (self.height - 1) * self.row_step + self.width * self.point_step

    def _bytes(self):
        d = self.data
        if isinstance(d, np.ndarray):
            if d.dtype != np.uint8 or d.ndim != 1 or not d.flags.c_contiguous:
                raise ValueError("data must be a flat contiguous uint8 array")
            return d
        return np.frombuffer(d, dtype=np.uint8)

    # ---- constructors ---------------------------------------------------------------------------------------------
    @classmethod
    def from_pointcloud2(cls, msg):
        """Any object with the attributes of sensor_msgs/PointCloud2: fields (name, offset, datatype, count), data,
        point_step, row_step, width, height, is_bigendian."""
        return cls(msg.data, msg.width, msg.height, msg.point_step, msg.row_step, msg.fields, msg.is_bigendian)

    @classmethod
    def from_pcd(cls, path):
        """A .pcd file.  `DATA binary`: the body is used as it is (memory-mapped).  `DATA ascii`: parsed on the host and
        repacked into 16-byte x, y, z, rgb records (float32 coordinates; a file without rgb gives 12-byte records)."""
        path = os.fspath(path)
        header, pos, kind = {}, 0, None
        with open(path, "rb") as fh:
            raw = fh.read(1 << 16)  # the header is a few hundred bytes
            while pos < len(raw):
                end = raw.find(b"\n", pos)
                end = len(raw) if end < 0 else end
                line = raw[pos:end].decode("ascii", "replace").strip()
                pos = end + 1
                if not line or line.startswith("#"):
                    continue
                key, _, rest = line.partition(" ")
                header[key.upper()] = rest.split()
                if key.upper() == "DATA":
                    kind = rest.strip().lower()
                    break
            if kind is None:
                raise ValueError(f"{path}: no DATA record (not a .pcd file)")
            if kind == "binary_compressed":
                raise NotImplementedError(f"{path}: DATA binary_compressed is not supported (ascii and binary are)")
            if kind not in ("ascii", "binary"):
                raise ValueError(f"{path}: unknown DATA kind {kind!r}")
            try:
                names = header["FIELDS"]
                sizes = [int(s) for s in header["SIZE"]]
                types = [t.upper() for t in header["TYPE"]]
                counts = [int(c) for c in header.get("COUNT", ["1"] * len(names))]
                width, height = int(header["WIDTH"][0]), int(header.get("HEIGHT", ["1"])[0])
                n = int(header["POINTS"][0]) if "POINTS" in header else width * height
            except (KeyError, IndexError, ValueError):
                raise ValueError(f"{path}: incomplete header (FIELDS, SIZE, TYPE, COUNT, WIDTH, POINTS)") from None
            if not len(names) == len(sizes) == len(types) == len(counts):
                raise ValueError(f"{path}: FIELDS, SIZE, TYPE and COUNT disagree in length")
            if width * height != n:
                width, height = n, 1
            if kind == "ascii":
                fh.seek(pos)
                text = fh.read().decode("ascii", "replace")
        fields, off = [], 0
        for name, size, typ, count in zip(names, sizes, types, counts):
            if (typ, size) not in _PCD_CODES:
                raise ValueError(f"{path}: field {name!r} has unsupported TYPE {typ} SIZE {size}")
            fields.append(Field(name, off, _PCD_CODES[(typ, size)], count))
            off += size * count
        if kind == "binary":
            data = np.memmap(path, dtype=np.uint8, mode="r", offset=pos, shape=(n * off,)) if n else np.zeros(0, np.uint8)
            return cls(data, width, height, off, width * off, fields)
        # ---- ascii: one text column per field element
        columns = np.concatenate([[0], np.cumsum(counts)])
        rows = [ln.split() for ln in text.splitlines() if ln.strip()]
        if len(rows) < n or any(len(r) < columns[-1] for r in rows[:n]):
            raise ValueError(f"{path}: fewer than {n} complete rows of data")
        col = {name: int(columns[i]) for i, name in enumerate(names)}
        for name in "xyz":
            if name not in col:
                raise ValueError(f"{path}: no scalar field {name!r}")
        points = np.array([[float(r[col[c]]) for c in "xyz"] for r in rows[:n]], dtype=np.float64).reshape(-1, 3)
        rgb_name = "rgb" if "rgb" in col else ("rgba" if "rgba" in col else None)
        packed_rgb = None
        if rgb_name is not None:
            if types[names.index(rgb_name)] == "F":  # PCL prints the float whose bits are the packed colour
                packed_rgb = np.array([float(r[col[rgb_name]]) for r in rows[:n]], dtype=np.float64).astype(np.float32).view(np.uint32)
            else:
                packed_rgb = np.array([int(r[col[rgb_name]]) & 0xFFFFFFFF for r in rows[:n]], dtype=np.uint32)
        layout = dict(LAYOUTS["pcd"]) if packed_rgb is not None else {"point_step": 12, "x": 0, "y": 4, "z": 8, "rgb": None,
                                                                       "xyz_type": FLOAT32}
        return cls.pack(points.astype(np.float32), packed_rgb, layout=layout, width=width, height=height)

    @classmethod
    def pack(cls, points, rgb_bytes=None, layout="kinect", width=None, height=1, row_pad=0, fill=0):
        """Write points [N, 3] and colours into records (a writer for tests and tools).  rgb_bytes: uint8 [N, 3] (r, g, b),
        or uint32 [N] already packed, or None.  layout: a name of LAYOUTS or a dict {"point_step", "x", "y", "z", "rgb" (offset
        or None), "xyz_type", "rgb_type", "bigendian"}.  float32 points are written as bits (a NaN keeps its payload).
        width * height must equal N (width defaults to N); row_pad bytes follow every row; unused bytes hold `fill`."""
        lay = dict(LAYOUTS[layout]) if isinstance(layout, str) else dict(layout)
        points = np.asarray(points)
        if points.ndim != 2 or points.shape[1] != 3:
            raise ValueError("points must be [N, 3]")
        n = len(points)
        width = n if width is None else int(width)
        if width * int(height) != n:
            raise ValueError(f"width * height = {width * int(height)} does not match {n} points")
        step = int(lay["point_step"])
        xyz_type = int(lay.get("xyz_type", FLOAT32))
        big = bool(lay.get("bigendian", False))
        order = ">" if big else "<"
        row_step = width * step + int(row_pad)
        buf = np.full(int(height) * row_step, fill, dtype=np.uint8)
        fields = [Field(name, int(lay[name]), xyz_type) for name in "xyz"]
        has_rgb = lay.get("rgb") is not None and rgb_bytes is not None
        if has_rgb:
            fields.append(Field("rgb", int(lay["rgb"]), int(lay.get("rgb_type", FLOAT32))))
        frame = cls(buf, width, height, step, row_step, fields, big)

        def slot(off, size):  # [N, size] writable view of one field's bytes
            v = np.lib.stride_tricks.as_strided(buf[off:], shape=(int(height), width, size),
                                                strides=(row_step, step, 1), writeable=True)
            return v

        if n:
            if xyz_type == FLOAT32:
                bits = points.astype(np.float32, copy=False).view(np.uint32) if points.dtype == np.float32 else \
                    points.astype(np.float32).view(np.uint32)
                vals, size = bits.astype(order + "u4"), 4
            else:
                vals, size = points.astype(np.float64).view(np.uint64).astype(order + "u8"), 8
            for c, name in enumerate("xyz"):
                slot(int(lay[name]), size)[...] = np.ascontiguousarray(vals[:, c]).view(np.uint8).reshape(int(height), width, size)
            if has_rgb:
                rgb_bytes = np.asarray(rgb_bytes)
                if rgb_bytes.ndim == 2:
                    c8 = rgb_bytes.astype(np.uint32)
                    v = (c8[:, 0] << 16) | (c8[:, 1] << 8) | c8[:, 2]
                else:
                    v = rgb_bytes.astype(np.uint32)
                slot(int(lay["rgb"]), 4)[...] = np.ascontiguousarray(v.astype(order + "u4")).view(np.uint8).reshape(
                    int(height), width, 4)
        return frame

    # ---- host decoding (the reference semantics) -------------------------------------------------------------------
    def _field_bytes(self, off, size, idx=None):
        """[n, size] bytes of one field, of every record or of the records idx"""
        buf = self._bytes()
        if idx is None:
            if self.n_records == 0:
                return np.zeros((0, size), np.uint8)
            v = np.lib.stride_tricks.as_strided(buf[off:], shape=(self.height, self.width, size),
                                                strides=(self.row_step, self.point_step, 1), writeable=False)
            return np.ascontiguousarray(v).reshape(-1, size)
        start = (idx // self.width) * self.row_step + (idx % self.width) * self.point_step + off
        return buf[start[:, None] + np.arange(size)]

    def _decode_fields(self, idx=None):
        """(points float32 [n, 3], finite bool [n], colour bytes uint8 [n, 3] or None)"""
        order = ">" if self.is_bigendian else "<"
        size = 8 if self.xyz_type == FLOAT64 else 4
        cols = [self._field_bytes(o, size, idx).view(order + ("f8" if size == 8 else "u4")).reshape(-1)
                for o in self.xyz_offsets]
        if size == 8:
            wide = np.stack(cols, axis=1).astype(np.float64)
            finite = np.isfinite(wide).all(axis=1)
            with np.errstate(over="ignore", invalid="ignore"):
                points = wide.astype(np.float32)  # round to nearest even; a finite value beyond FLT_MAX becomes inf
        else:
            points = np.stack(cols, axis=1).astype(np.uint32).view(np.float32)  # the bits, NaN payloads included
            finite = np.isfinite(points).all(axis=1)
        rgb = None
        if self.rgb_offset >= 0:
            v = self._field_bytes(self.rgb_offset, 4, idx).view(order + "u4").reshape(-1).astype(np.uint32)
            rgb = np.stack(((v >> 16) & 255, (v >> 8) & 255, v & 255), axis=1).astype(np.uint8)
        return points, finite, rgb

    def decode_host(self, box=None, keep_nonfinite=False, color="float64", lut=None):
        """-> (points float32 [k, 3], rgb [k, 3] or None, src int64 [k]): the kept records in record order, as
        sv_unpack_points defines them.  rgb = lut[bytes] when a 256-entry lut is given, else the convention `color`."""
        box = check_box(box)
        table = color_table(color) if lut is None else np.asarray(lut)
        points, finite, rgb = self._decode_fields()
        keep = np.ones(len(points), dtype=bool) if keep_nonfinite else finite
        if box is not None:
            with np.errstate(invalid="ignore"):
                p = points.astype(np.float64)
                keep = keep & np.all((box[:3] < p) & (p < box[3:]), axis=1)
        src = np.nonzero(keep)[0]
        return points[src], (None if rgb is None else table[rgb[src]]), src

    def take(self, src_idx, color="float64", lut=None):
        """-> (points float32 [m, 3], rgb [m, 3] or None) of the records src_idx only, decoded on the host"""
        idx = np.asarray(src_idx, dtype=np.int64).reshape(-1)
        if len(idx) and (idx.min() < 0 or idx.max() >= self.n_records):
            raise IndexError("record index outside the frame")
        table = color_table(color) if lut is None else np.asarray(lut)
        points, _, rgb = self._decode_fields(idx)
        return points, (None if rgb is None else table[rgb])

    def scatter(self, labels, src, fill=-1):
        """per-point labels of the kept records -> an [H, W] image of the organised cloud, `fill` where nothing was kept"""
        labels, src = np.asarray(labels), np.asarray(src, dtype=np.int64)
        if labels.shape != src.shape:
            raise ValueError("labels and src must have the same length")
        out = np.full(self.n_records, fill, dtype=labels.dtype)
        out[src] = labels
        return out.reshape(self.height, self.width)

    # ---- device decoding --------------------------------------------------------------------------------------------
    def flags(self, keep_nonfinite=False):
        return ((_lib.SV_UNPACK_BIGENDIAN if self.is_bigendian else 0) |
                (_lib.SV_UNPACK_KEEP_NONFINITE if keep_nonfinite else 0))

    def unpack(self, d_bytes, box=None, lut=None, keep_nonfinite=False, want_src=True):
        """sv_unpack_points on this frame's bytes already on the device (uint8 CUDA tensor), on the current stream.
        -> (points [n, 3], rgb [n, 3] or None, src int32 [n] or None, count int64 [1]), all on the device and NOT sliced:
        rows at or beyond count are unspecified.  Nothing is read back."""
        box = check_box(box)
        n = self.n_records
        if n < 1:
            raise ValueError("unpack needs at least one record")
        if lut is not None and (lut.dtype != torch.float32 or lut.numel() != 256 or not lut.is_contiguous()):
            raise ValueError("lut must be a contiguous float32 tensor of 256 values")
        _lib.require_cuda(d_bytes, "the frame's bytes")
        if d_bytes.dtype != torch.uint8 or d_bytes.dim() != 1 or d_bytes.numel() < self.nbytes_used:
            raise ValueError("d_bytes must be a flat uint8 tensor covering the last record")
        dev = d_bytes.device
        ws_bytes = _lib.load().sv_unpack_points_workspace_bytes(c_int64(n))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        points = torch.empty((n, 3), dtype=torch.float32, device=dev)
        rgb = torch.empty((n, 3), dtype=torch.float32, device=dev) if self.rgb_offset >= 0 else None
        src = torch.empty(n, dtype=torch.int32, device=dev) if want_src else None
        count = torch.empty(1, dtype=torch.int64, device=dev)
        call("sv_unpack_points", ptr(d_bytes), c_int64(d_bytes.numel()), c_int64(n), c_int64(self.width),
             c_int64(self.point_step), c_int64(self.row_step), c_int(self.xyz_offsets[0]), c_int(self.xyz_offsets[1]),
             c_int(self.xyz_offsets[2]), c_int(self.xyz_type), c_int(self.rgb_offset),
             c_int(self.flags(keep_nonfinite)), None if box is None else (c_double * 6)(*box), ptr(lut), ptr(ws),
             c_size_t(ws_bytes), ptr(points), ptr(rgb), ptr(src), ptr(count), stream_ptr())
        return points, rgb, src, count

    def decode_device(self, device, box=None, lut=None, stream=None, keep_nonfinite=False):
        """Upload the bytes, decode on the device -> (points float32 [k, 3], rgb float32 [k, 3] or None, src int32 [k]) as CUDA
        tensors sliced to the number kept (one 8-byte read-back).  lut: None (byte values), a convention name ("float64",
        "float32": the engine's normalised colours, device_lut_values) or a float32 CUDA tensor of 256 values."""
        box = check_box(box)
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.SvHipError(f"decode_device needs a GPU (got {device}); the HIP path has no CPU fallback")
        if isinstance(lut, str):
            values = device_lut_values(lut)
        if self.n_records == 0:
            empty = torch.empty((0, 3), dtype=torch.float32, device=device)
            return empty, (empty.clone() if self.rgb_offset >= 0 else None), torch.empty(0, dtype=torch.int32, device=device)
        host = torch.empty(self.nbytes_used, dtype=torch.uint8)
        host.numpy()[:] = self._bytes()[: self.nbytes_used]
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(device)):
            if isinstance(lut, str):
                lut = torch.from_numpy(values).to(device)
            d_bytes = host.to(device)
            points, rgb, src, count = self.unpack(d_bytes, box=box, lut=lut, keep_nonfinite=keep_nonfinite)
            k = int(count.item())
        return points[:k], (None if rgb is None else rgb[:k]), src[:k]
