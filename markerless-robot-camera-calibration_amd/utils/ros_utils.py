"""PointCloud2 messages as numpy record arrays, with the reference's names (utils/ros_utils.py) and without ROS: a message
is any object with `fields` (name, offset, datatype, count), `data`, `point_step`, `row_step`, `width`, `height` and
`is_bigendian`.  `get_points_and_colors(msg, device=...)` skips the host arrays altogether: the message's bytes are
decoded on the GPU (utils/packed.py, sv_unpack_points)."""
import numpy as np

from .packed import FIELD_DTYPES, PackedFrame

DUMMY_FIELD_PREFIX = "__"
pftype_to_nptype = dict(FIELD_DTYPES)
nptype_to_pftype = {dtype: code for code, dtype in FIELD_DTYPES.items()}
pftype_sizes = {code: dtype.itemsize for code, dtype in FIELD_DTYPES.items()}


def _padding(begin, end):
    return [(f"{DUMMY_FIELD_PREFIX}{at}", np.uint8) for at in range(begin, end)]


def fields_to_dtype(fields, point_step):
    """The record dtype of a message as a list of (name, dtype): the fields in the order given, one uint8 member named
    "__<offset>" for every byte between them and up to point_step."""
    members, at = [], 0
    for field in fields:
        members += _padding(at, field.offset)
        at = max(at, field.offset)
        dtype = pftype_to_nptype[field.datatype]
        members.append((field.name, dtype if field.count == 1 else np.dtype((dtype, field.count))))
        at += pftype_sizes[field.datatype] * field.count
    return members + _padding(at, point_step)


def pointcloud2_to_array(cloud_msg, squeeze=True):
    """The message's records as a structured array without the padding members, shaped (height, width), or (width,) when
    squeeze is set and the cloud has one row."""
    members = fields_to_dtype(cloud_msg.fields, cloud_msg.point_step)
    records = np.frombuffer(cloud_msg.data, np.dtype(members))
    records = records[[name for name, _ in members if not name.startswith(DUMMY_FIELD_PREFIX)]]
    if squeeze and cloud_msg.height == 1:
        return records.reshape(cloud_msg.width)
    return records.reshape(cloud_msg.height, cloud_msg.width)


def split_rgb_field(cloud_arr):
    """A record array with a packed 4-byte `rgb` member -> the same records with uint8 members r, g, b in its place
    (PCL keeps the three bytes in the bits of a float32)."""
    packed = np.ascontiguousarray(cloud_arr["rgb"]).view(np.uint32)
    members = [(name, cloud_arr.dtype.fields[name][0]) for name in cloud_arr.dtype.names if name != "rgb"]
    out = np.zeros(cloud_arr.shape, members + [("r", np.uint8), ("g", np.uint8), ("b", np.uint8)])
    for name, _ in members:
        out[name] = cloud_arr[name]
    out["r"], out["g"], out["b"] = (packed >> 16) & 255, (packed >> 8) & 255, packed & 255
    return out


def _finite(cloud_array):
    return np.isfinite(cloud_array["x"]) & np.isfinite(cloud_array["y"]) & np.isfinite(cloud_array["z"])


def _columns(cloud_array, names, dtype):
    out = np.zeros(cloud_array.shape + (len(names),), dtype=dtype)
    for c, name in enumerate(names):
        out[..., c] = cloud_array[name]
    return out


def get_xyz_points(cloud_array, remove_nans=True, dtype=float):
    if remove_nans:
        cloud_array = cloud_array[_finite(cloud_array)]
    return _columns(cloud_array, "xyz", dtype)


def get_points_and_colors(pointcloud, remove_nans=True, dtype=float, device=None):
    """-> (points, rgb): x, y, z and the colour bytes r, g, b (0..255, not scaled) as `dtype` arrays.  With `device` the
    message's bytes are uploaded and decoded there: float32 CUDA tensors [k, 3] with the same values (coordinates as the
    message's float32 bits), and `dtype` is not used."""
    if device is not None:
        points, rgb, _ = PackedFrame.from_pointcloud2(pointcloud).decode_device(device, keep_nonfinite=not remove_nans)
        return points, rgb
    cloud_array = pointcloud2_to_array(pointcloud)
    if remove_nans:
        cloud_array = cloud_array[_finite(cloud_array)]
    split = split_rgb_field(cloud_array)
    return _columns(split, "xyz", dtype), _columns(split, "rgb", dtype)
