"""A reference decoder of packed sensor records that shares no code with the package: records are read and written through
a numpy structured dtype built from names, formats, offsets and itemsize (">" formats for big-endian data), row padding is
removed by slicing the byte buffer, and the rules of include/sv_hip.h block N3e are applied literally."""
import numpy as np

F32, F64, U32 = 7, 8, 6  # PointField datatype codes
FLT_MAX = float(np.finfo(np.float32).max)
TILE = 256  # records per workgroup of the kernels: the record counts below sit around its multiples

# name -> step, offsets, coordinate format, declared rgb type (None: no rgb field), byte order
LAYOUTS = {
    "kinect32": dict(step=32, x=0, y=4, z=8, rgb=16, xyz="f4", rgb_type=F32, big=False),
    "pcd16": dict(step=16, x=0, y=4, z=8, rgb=12, xyz="f4", rgb_type=F32, big=False),
    "step19": dict(step=19, x=1, y=5, z=9, rgb=14, xyz="f4", rgb_type=F32, big=False),  # a uint8 field in front of x
    "f64_step28": dict(step=28, x=0, y=8, z=16, rgb=24, xyz="f8", rgb_type=F32, big=False),
    "bigendian": dict(step=16, x=0, y=4, z=8, rgb=12, xyz="f4", rgb_type=F32, big=True),
    "f64_bigendian": dict(step=30, x=1, y=9, z=17, rgb=25, xyz="f8", rgb_type=F32, big=True),
    "rgb_uint32": dict(step=16, x=0, y=4, z=8, rgb=12, xyz="f4", rgb_type=U32, big=False),
    "no_rgb": dict(step=12, x=0, y=4, z=8, rgb=None, xyz="f4", rgb_type=None, big=False),
    "shuffled": dict(step=24, x=16, y=4, z=20, rgb=9, xyz="f4", rgb_type=F32, big=False),  # fields out of order, rgb odd
}
COUNTS = (1, 63, 64, 65, 255, 256, 257, 2 * TILE + 1)
PATTERNS = ("all", "none", "first", "last", "alternating", "third_nan", "inf_one", "special")


def record_dtype(lay):
    """the structured dtype of one record; coordinates and colour are read as unsigned integers of the data's byte order"""
    o = ">" if lay["big"] else "<"
    width = "u8" if lay["xyz"] == "f8" else "u4"
    names, formats, offsets = ["x", "y", "z"], [o + width] * 3, [lay["x"], lay["y"], lay["z"]]
    if lay["rgb"] is not None:
        names.append("rgb")
        formats.append(o + "u4")
        offsets.append(lay["rgb"])
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": lay["step"]})


def fields(lay):
    """(name, offset, datatype) rows for a message's field list, in declaration order of the layout"""
    rows = [(n, lay[n], F64 if lay["xyz"] == "f8" else F32) for n in "xyz"]
    if lay["rgb"] is not None:
        rows.append(("rgb", lay["rgb"], lay["rgb_type"]))
    return rows


def coordinate_bits(lay, xyz):
    """xyz: float32 [N, 3] for f4 layouts, float64 [N, 3] for f8 ones -> the unsigned integers with the same bits"""
    want = np.float64 if lay["xyz"] == "f8" else np.float32
    assert xyz.dtype == want, (xyz.dtype, want)
    return np.ascontiguousarray(xyz).view(np.uint64 if want == np.float64 else np.uint32)


def build(lay, xyz, rgb_u32, width, height, row_pad=0, fill=0xA5, seed=0):
    """-> the byte buffer (uint8) of width * height records; padding bytes are random so that nothing can rely on them"""
    n = width * height
    assert len(xyz) == n
    rec = np.zeros(n, dtype=record_dtype(lay))
    raw = rec.view(np.uint8).reshape(n, lay["step"])
    raw[...] = np.random.default_rng(seed).integers(0, 256, size=raw.shape, dtype=np.uint8)
    bits = coordinate_bits(lay, xyz)
    for c, name in enumerate("xyz"):
        rec[name] = bits[:, c]
    if lay["rgb"] is not None:
        rec["rgb"] = rgb_u32
    row = width * lay["step"]
    buf = np.full(height * (row + row_pad), fill, dtype=np.uint8)
    buf.reshape(height, row + row_pad)[:, :row] = rec.view(np.uint8).reshape(height, row)
    return buf


def f64_to_f32_bits(u):
    """uint64 bits of doubles -> uint32 bits of the float32 nearest to each (ties to even); NaN: sign | 0x7fc00000 | the top
    22 payload bits"""
    d = u.view(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        out = d.astype(np.float32).view(np.uint32).copy()
    nan = np.isnan(d)
    out[nan] = (((u[nan] >> np.uint64(32)) & np.uint64(0x80000000)) | np.uint64(0x7FC00000) |
                ((u[nan] >> np.uint64(29)) & np.uint64(0x3FFFFF))).astype(np.uint32)
    return out


def decode(buf, lay, width, height, row_pad=0, box=None, keep_nonfinite=False, lut=None):
    """-> dict(points float32 [k, 3], rgb float32 [k, 3] or None, src int32 [k], count)"""
    row = width * lay["step"]
    body = np.ascontiguousarray(buf[: height * (row + row_pad)].reshape(height, row + row_pad)[:, :row]).reshape(-1)
    rec = np.frombuffer(body.tobytes(), dtype=record_dtype(lay))
    cols, finite = [], np.ones(len(rec), dtype=bool)
    for name in "xyz":
        if lay["xyz"] == "f8":
            u = rec[name].astype(np.uint64)
            finite &= np.isfinite(u.view(np.float64))  # as a double, before the rounding
            cols.append(f64_to_f32_bits(u))
        else:
            u = rec[name].astype(np.uint32)
            finite &= np.isfinite(u.view(np.float32))
            cols.append(u)  # the bits as they are
    points = np.stack(cols, axis=1).view(np.float32)
    keep = np.ones(len(rec), dtype=bool) if keep_nonfinite else finite
    if box is not None:
        lo, hi = np.asarray(box[:3], np.float64), np.asarray(box[3:], np.float64)
        with np.errstate(invalid="ignore"):
            p = points.astype(np.float64)
            keep = keep & ((lo < p) & (p < hi)).all(axis=1)
    src = np.flatnonzero(keep).astype(np.int32)
    rgb = None
    if lay["rgb"] is not None:
        v = rec["rgb"].astype(np.uint32)[src]
        channels = np.stack(((v >> 16) & 255, (v >> 8) & 255, v & 255), axis=1)
        rgb = channels.astype(np.float32) if lut is None else np.asarray(lut, np.float32)[channels]
    return {"points": points[src], "rgb": rgb, "src": src, "count": len(src)}


# ---- inputs ---------------------------------------------------------------------------------------------------------
def nan_bits32(i):
    """float32 NaNs with distinct payloads: quiet and signalling, both signs"""
    i = np.asarray(i, dtype=np.uint32)
    payload = (i * np.uint32(2654435761)) & np.uint32(0x3FFFFF) | np.uint32(1)
    quiet = np.where(i % 2 == 0, np.uint32(0x400000), np.uint32(0))
    sign = np.where(i % 3 == 0, np.uint32(0x80000000), np.uint32(0))
    return sign | np.uint32(0x7F800000) | quiet | payload


def coordinates(lay, n, pattern, seed=0):
    """xyz of n records in the layout's coordinate type, and the records the keep rule should keep (without a box)"""
    rng = np.random.default_rng(1000 + seed + n)
    wide = lay["xyz"] == "f8"
    xyz = rng.uniform(-3.0, 3.0, size=(n, 3)).astype(np.float32)
    if wide:
        xyz = xyz.astype(np.float64) + rng.uniform(-1e-9, 1e-9, size=(n, 3))  # not representable in float32
    bad = np.zeros(n, dtype=bool)
    if pattern == "none":
        bad[:] = True
    elif pattern == "first":
        bad[1:] = True
    elif pattern == "last":
        bad[:-1] = True
    elif pattern == "alternating":
        bad[1::2] = True
    elif pattern == "third_nan":
        bad = rng.uniform(size=n) < 1.0 / 3.0
    elif pattern == "inf_one":
        bad = rng.uniform(size=n) < 0.25
    rows = np.flatnonzero(bad)
    axis = rng.integers(0, 3, size=len(rows))
    if pattern == "inf_one":
        xyz[rows, axis] = np.where(rng.uniform(size=len(rows)) < 0.5, np.inf, -np.inf)  # one coordinate only
    elif wide:
        xyz[rows, axis] = (np.uint64(0x7FF0000000000000) | (rows.astype(np.uint64) * np.uint64(0x9E3779B97F4A7) &
                                                             np.uint64(0xFFFFFFFFFFFFF)) | np.uint64(1)).view(np.float64)
    else:
        bits = xyz.view(np.uint32)
        bits[rows, axis] = nan_bits32(rows)
    if pattern == "special":  # all of these are kept
        if wide:
            vals = np.array([-0.0, 1e-40, 1e-50, 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -40, 1.0 + 3 * 2.0 ** -24,
                             1e39, -1e39, FLT_MAX * (1 + 2.0 ** -26), 1.0 - 2.0 ** -25 - 2.0 ** -50, 2.0 ** -149 * 0.5,
                             2.0 ** -149 * 0.75, -(2.0 ** -126) * (1 - 2.0 ** -25)], dtype=np.float64)
        else:
            vals = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0],
                            dtype=np.uint32).view(np.float32)
        for c in range(3):
            xyz[:, c] = vals[(np.arange(n) + 3 * c) % len(vals)]
    return xyz, ~bad


def colours(n, seed=0):
    """packed colours with all 32 bits in use (the top byte is not part of the colour)"""
    return np.random.default_rng(2000 + seed + n).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)


class Message:
    """a duck-typed sensor_msgs/PointCloud2"""

    class PointField:
        def __init__(self, name, offset, datatype, count=1):
            self.name, self.offset, self.datatype, self.count = name, offset, datatype, count

    def __init__(self, buf, lay, width, height, row_pad=0, field_order=None):
        rows = fields(lay)
        if field_order is not None:
            rows = [rows[i] for i in field_order]
        self.fields = [self.PointField(*r) for r in rows]
        self.data = buf.tobytes()
        self.width, self.height = width, height
        self.point_step, self.row_step = lay["step"], width * lay["step"] + row_pad
        self.is_bigendian = lay["big"]
        self.is_dense = False
