"""sv_unpack_points against the numpy reference of tests/ingest_helpers.py, bit for bit: points and colours as int32 views,
source indices and the count.  Shapes are the smallest at which the kernels can go wrong: a tile is 256 records (four
waves), so the counts sit around 64, 256 and 512; 70 001 records make 274 tiles, more than the 256 threads of the scan's one
workgroup.  Every field is assembled from single bytes, so the 4-aligned layouts and the odd ones take one path."""
import numpy as np
import pytest

import ingest_helpers as H

pytestmark = pytest.mark.gpu

def _frame(buf, lay, width, height, row_pad=0):
    from mrcc_amd.utils.packed import Field, PackedFrame

    return PackedFrame(buf, width, height, lay["step"], width * lay["step"] + row_pad,
                       [Field(*r) for r in H.fields(lay)], lay["big"])


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _check(got, want, what):
    points, rgb, src = got
    assert len(src) == want["count"], what
    assert src.dtype.is_floating_point is False and np.array_equal(src.cpu().numpy(), want["src"]), what
    assert np.array_equal(_bits(points), want["points"].view(np.int32)), what
    if want["rgb"] is None:
        assert rgb is None, what
    else:
        assert np.array_equal(_bits(rgb), want["rgb"].view(np.int32)), what


def _run_case(gpu, name, n, pattern, width=None, height=1, row_pad=0, lut=None, **kw):
    import torch

    lay = H.LAYOUTS[name]
    width = n if width is None else width
    xyz, kept = H.coordinates(lay, n, pattern)
    buf = H.build(lay, xyz, H.colours(n), width, height, row_pad)
    frame = _frame(buf, lay, width, height, row_pad)
    want = H.decode(buf, lay, width, height, row_pad, lut=lut, **kw)
    if not kw:
        assert np.array_equal(want["src"], np.flatnonzero(kept))  # the pattern is what it says
    d_lut = None if lut is None else torch.from_numpy(lut).to(gpu)
    _check(frame.decode_device(gpu, lut=d_lut, **kw), want, (name, n, pattern, kw))
    return want


@pytest.mark.parametrize("pattern", H.PATTERNS)
@pytest.mark.parametrize("name", sorted(H.LAYOUTS))
def test_layouts_and_keep_patterns(gpu, name, pattern):
    for n in H.COUNTS:
        want = _run_case(gpu, name, n, pattern)
        if pattern == "none":
            assert want["count"] == 0
        if pattern in ("all", "special"):
            assert want["count"] == n
        if pattern in ("first", "last"):
            assert want["count"] == 1 and want["src"][0] == (0 if pattern == "first" else n - 1)


@pytest.mark.parametrize("name", sorted(H.LAYOUTS))
def test_many_tiles(gpu, name):
    """274 tiles: the scan's workgroup takes a second turn, and its carry reaches the later tiles"""
    want = _run_case(gpu, name, 70001, "third_nan")
    assert 40000 < want["count"] < 52000


@pytest.mark.parametrize("name", ("kinect32", "step19", "f64_step28", "f64_bigendian"))
def test_organised_cloud_with_row_padding(gpu, name):
    for width, height in ((7, 5), (7, 74)):  # 35 records; 518 records, rows straddling the tiles
        for pattern in ("all", "third_nan", "none"):
            _run_case(gpu, name, width * height, pattern, width=width, height=height, row_pad=12)


@pytest.mark.parametrize("name", sorted(H.LAYOUTS))
def test_keep_nonfinite_keeps_everything(gpu, name):
    for pattern in ("third_nan", "inf_one", "none"):
        want = _run_case(gpu, name, 257, pattern, keep_nonfinite=True)
        assert want["count"] == 257
    if H.LAYOUTS[name]["xyz"] == "f4":  # a float32 NaN's payload survives: distinct NaN bit patterns come back
        nan = np.isnan(want["points"])
        assert nan.sum() >= 257 and len(np.unique(want["points"].view(np.uint32)[nan])) > 200


def test_float64_rounding_cases(gpu):
    """the values the float64 'special' pattern holds round to different float32s under truncation and nearest-even, one
    finite value lies above FLT_MAX and becomes inf (kept: the finiteness test is on the double)"""
    lay = H.LAYOUTS["f64_step28"]
    xyz, _ = H.coordinates(lay, 64, "special")
    with np.errstate(over="ignore"):
        nearest = xyz.astype(np.float32)
        truncated = (np.ascontiguousarray(xyz).view(np.uint64) & ~np.uint64(0x1FFFFFFF)).view(np.float64).astype(np.float32)
    assert (nearest != truncated).any() and np.isinf(nearest).any() and np.isfinite(xyz).all()
    want = _run_case(gpu, "f64_step28", 64, "special")
    assert np.array_equal(want["points"].view(np.int32), nearest.view(np.int32)) and want["count"] == 64


def _box_cloud(lay, lo, hi):
    """one point inside, then a point exactly on each of the six bounds, then one outside on each side"""
    mid = (np.asarray(lo) + np.asarray(hi)) / 2
    rows = [mid.copy()]
    for a in range(3):
        for bound in (lo[a], hi[a]):
            p = mid.copy()
            p[a] = bound
            rows.append(p)
    for a in range(3):
        for bound in (lo[a] - 1.0, hi[a] + 1.0):
            p = mid.copy()
            p[a] = bound
            rows.append(p)
    rows.append(mid + 0.25)
    return np.array(rows, dtype=np.float64 if lay["xyz"] == "f8" else np.float32)


@pytest.mark.parametrize("name", ("kinect32", "step19", "f64_step28", "bigendian"))
def test_box_bounds_are_strict(gpu, name):
    lay = H.LAYOUTS[name]
    for box in ((-1.0, -2.0, 0.5, 1.0, 2.0, 4.5), (-500.0,) * 3 + (500.0,) * 3):  # the second is get_roi_mask's default
        xyz = _box_cloud(lay, box[:3], box[3:])
        n = len(xyz)
        buf = H.build(lay, xyz, H.colours(n), n, 1)
        want = H.decode(buf, lay, n, 1, box=box)
        assert list(want["src"]) == [0, n - 1]  # every point on a bound is dropped
        _check(_frame(buf, lay, n, 1).decode_device(gpu, box=box), want, (name, box))
    # a box inside a random cloud, with NaN records; then lo == hi, which keeps nothing
    box = (-1.5, -1.0, -2.0, 1.0, 2.5, 0.5)
    want = _run_case(gpu, name, 513, "third_nan", box=box)
    assert 0 < want["count"] < 200
    flat = (0.0, -3.0, -3.0, 0.0, 3.0, 3.0)
    assert _run_case(gpu, name, 257, "all", box=flat)["count"] == 0
    # the bound is compared with the float32 coordinate: a double just inside the bound that rounds onto it is dropped
    if lay["xyz"] == "f8":
        xyz = np.array([[1.0 - 2.0 ** -30, 0.0, 1.0], [0.5, 0.0, 1.0]])
        buf = H.build(lay, xyz, H.colours(2), 2, 1)
        want = H.decode(buf, lay, 2, 1, box=(-1.0, -2.0, 0.5, 1.0, 2.0, 4.5))
        assert list(want["src"]) == [1]
        _check(_frame(buf, lay, 2, 1).decode_device(gpu, box=(-1.0, -2.0, 0.5, 1.0, 2.0, 4.5)), want, name)


@pytest.mark.parametrize("name", ("kinect32", "step19", "bigendian", "rgb_uint32"))
def test_colour_table(gpu, name):
    lut = np.random.default_rng(4).normal(size=256).astype(np.float32)
    lut[7] = np.float32("inf")
    with_lut = _run_case(gpu, name, 257, "third_nan", lut=lut)
    without = _run_case(gpu, name, 257, "third_nan")
    assert np.array_equal(with_lut["rgb"].view(np.int32), lut[without["rgb"].astype(np.int64)].view(np.int32))
    assert without["rgb"].min() >= 0 and without["rgb"].max() <= 255 and len(np.unique(without["rgb"])) > 200


def test_repeated_calls_give_the_same_bits_and_count_is_on_the_device(gpu):
    import torch

    lay = H.LAYOUTS["step19"]
    n = 70001
    xyz, _ = H.coordinates(lay, n, "third_nan")
    buf = H.build(lay, xyz, H.colours(n), n, 1)
    frame = _frame(buf, lay, n, 1)
    want = H.decode(buf, lay, n, 1)
    d = torch.from_numpy(buf).to(gpu)
    outs = []
    for _ in range(3):
        points, rgb, src, count = frame.unpack(d)
        k = int(count.item())
        assert count.dtype == torch.int64 and k == want["count"] and points.shape == (n, 3) and src.dtype == torch.int32
        outs.append((_bits(points[:k]), _bits(rgb[:k]), src[:k].cpu().numpy()))
    for o in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(o, outs[0]))
    _check((points[:k], rgb[:k], src[:k]), want, "step19")
    # without source indices
    points, rgb, src, count = frame.unpack(d, want_src=False)
    assert src is None and np.array_equal(_bits(points[: int(count.item())]), want["points"].view(np.int32))


def test_buffer_at_an_odd_device_address(gpu):
    """the 4-aligned Kinect layout in a buffer that starts one to three bytes into an allocation"""
    import torch

    lay = H.LAYOUTS["kinect32"]
    n = 300
    xyz, _ = H.coordinates(lay, n, "third_nan")
    buf = H.build(lay, xyz, H.colours(n), n, 1)
    want = H.decode(buf, lay, n, 1)
    for shift in (1, 2, 3):
        d = torch.from_numpy(np.concatenate([np.zeros(shift, np.uint8), buf])).to(gpu)[shift:]
        assert d.data_ptr() % 4 == shift
        points, rgb, src, count = _frame(buf, lay, n, 1).unpack(d)
        k = int(count.item())
        _check((points[:k], rgb[:k], src[:k]), want, shift)


@pytest.mark.parametrize("color", ("float64", "float32"))
def test_decode_device_equals_decode_host(gpu, color):
    from mrcc_amd.utils import preprocess

    lay = H.LAYOUTS["kinect32"]
    width, height = 37, 9
    n = width * height
    xyz, _ = H.coordinates(lay, n, "third_nan")
    buf = H.build(lay, xyz, H.colours(n), width, height, 12)
    frame = _frame(buf, lay, width, height, 12)
    box = (-2.0, -2.5, -2.0, 2.5, 2.0, 2.5)
    points, rgb, src = frame.decode_host(box=box, color=color)
    assert 0 < len(src) < n - 100 and rgb.dtype == np.dtype(color)
    d_points, d_rgb, d_src = frame.decode_device(gpu, box=box, lut=color)
    assert np.array_equal(_bits(d_points), points.view(np.int32)) and np.array_equal(d_src.cpu().numpy(), src)
    # the device colours are what the engine's host path uploads: normalize_colors of the frame, rounded to float32
    staged = preprocess.normalize_colors(rgb).astype(np.float32)
    assert np.array_equal(_bits(d_rgb), staged.view(np.int32))
    # no table: the byte values, as get_points_and_colors gives them
    _, d_bytes, _ = frame.decode_device(gpu, box=box)
    assert np.array_equal(d_bytes.cpu().numpy(), frame.decode_host(box=box, color="bytes")[1].astype(np.float32))
    # an empty frame is handled in Python
    empty = _frame(np.zeros(0, np.uint8), lay, 0, 0).decode_device(gpu)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3) and empty[2].shape == (0,)


def test_ros_utils_on_the_device(gpu):
    from mrcc_amd.utils import ros_utils

    lay = H.LAYOUTS["kinect32"]
    width, height = 16, 5
    xyz, _ = H.coordinates(lay, width * height, "third_nan")
    msg = H.Message(H.build(lay, xyz, H.colours(width * height), width, height), lay, width, height)
    for remove_nans in (True, False):
        points, rgb = ros_utils.get_points_and_colors(msg, remove_nans=remove_nans, dtype=np.float32)
        d_points, d_rgb = ros_utils.get_points_and_colors(msg, remove_nans=remove_nans, device=gpu)
        assert np.array_equal(_bits(d_points), points.reshape(-1, 3).view(np.int32))
        assert np.array_equal(d_rgb.cpu().numpy(), rgb.reshape(-1, 3))


def test_scatter_places_labels_at_src(gpu):
    lay = H.LAYOUTS["kinect32"]
    width, height = 7, 5
    xyz, kept = H.coordinates(lay, 35, "third_nan")
    frame = _frame(H.build(lay, xyz, H.colours(35), width, height, 12), lay, width, height, 12)
    _, _, src = frame.decode_device(gpu)
    labels = np.arange(len(src), dtype=np.int64) % 3
    image = frame.scatter(labels, src.cpu().numpy())
    assert image.shape == (5, 7) and image.dtype == np.int64
    flat = image.reshape(-1)
    assert np.array_equal(flat[kept], labels) and (flat[~kept] == -1).all()
    assert (frame.scatter(labels, src.cpu().numpy(), fill=9).reshape(-1)[~kept] == 9).all()
