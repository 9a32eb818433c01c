"""Host side of the packed-frame ingest: PackedFrame's numpy decoder against the independent reference of
tests/ingest_helpers.py, the PointCloud2 and .pcd constructors, the ros_utils names, PCDDataEngine and the colour table.
No GPU needed."""
import os

import numpy as np
import pytest

import ingest_helpers as H
from conftest import GOLDEN


def _frame(buf, lay, width, height, row_pad=0):
    from mrcc_amd.utils.packed import Field, PackedFrame

    return PackedFrame(buf, width, height, lay["step"], width * lay["step"] + row_pad,
                       [Field(*r) for r in H.fields(lay)], lay["big"])


def _same(got, want):
    points, rgb, src = got
    assert points.dtype == np.float32 and np.array_equal(points.view(np.int32), want["points"].view(np.int32))
    assert np.array_equal(src, want["src"]) and len(src) == want["count"]
    if want["rgb"] is None:
        assert rgb is None
    else:
        assert np.array_equal(np.asarray(rgb, np.float32), want["rgb"])


@pytest.mark.parametrize("name", sorted(H.LAYOUTS))
def test_decode_host_and_take_against_the_reference(name):
    lay = H.LAYOUTS[name]
    for pattern in H.PATTERNS:
        for width, height, pad in ((65, 1, 0), (7, 5, 12)):
            n = width * height
            xyz, _ = H.coordinates(lay, n, pattern)
            buf = H.build(lay, xyz, H.colours(n), width, height, pad)
            frame = _frame(buf, lay, width, height, pad)
            assert frame.n_records == n and frame.nbytes_used == len(buf) - pad
            box = (-2.0, -2.5, -1.0, 2.5, 2.0, 2.5)
            for kw in ({}, {"keep_nonfinite": True}, {"box": box}, {"box": box, "keep_nonfinite": True}):
                _same(frame.decode_host(color="bytes", **kw), H.decode(buf, lay, width, height, pad, **kw))
            # take: any records, in any order, dropped ones included
            everything = H.decode(buf, lay, width, height, pad, keep_nonfinite=True)
            idx = np.random.default_rng(n).permutation(n)[: max(1, n // 3)]
            points, rgb = frame.take(idx, color="bytes")
            assert np.array_equal(points.view(np.int32), everything["points"][idx].view(np.int32))
            if lay["rgb"] is not None:
                assert np.array_equal(rgb, everything["rgb"][idx])
            assert frame.take([])[0].shape == (0, 3)


def test_colour_conventions_and_lut():
    from mrcc_amd.utils import packed, preprocess

    lay = H.LAYOUTS["kinect32"]
    n = 4000
    xyz, _ = H.coordinates(lay, n, "third_nan")
    buf = H.build(lay, xyz, H.colours(n), n, 1)
    frame = _frame(buf, lay, n, 1)
    raw = frame.decode_host(color="bytes")[1]
    assert raw.dtype == np.uint8 and len(np.unique(raw)) == 256
    c64, c32 = frame.decode_host(color="float64")[1], frame.decode_host(color="float32")[1]
    assert c64.dtype == np.float64 and np.array_equal(c64, raw / 255)
    assert c32.dtype == np.float32 and np.array_equal(c32, (raw / 255).astype(np.float32))
    # the table is normalize_colors applied per frame, in the convention's dtype and as the staging copy rounds it
    for color, host in (("float64", c64), ("float32", c32)):
        per_frame = preprocess.normalize_colors(host)
        table = packed.normalized_color_table(color)
        assert table.dtype == per_frame.dtype and np.array_equal(table[raw], per_frame)
        lut = packed.device_lut_values(color)
        assert lut.dtype == np.float32 and lut.shape == (256,)
        assert np.array_equal(lut[raw].view(np.int32), per_frame.astype(np.float32).view(np.int32))
        assert np.array_equal(frame.decode_host(lut=table)[1], per_frame)
        # a dark and a bright frame take the same branch as the whole table does
        for rows in (raw.max(axis=1) < 40, raw.min(axis=1) > 200):
            assert rows.sum() > 0
            assert np.array_equal(table[raw[rows]], preprocess.normalize_colors(host[rows]))
    assert packed.device_lut_values("float64")[0] == -0.5 and packed.device_lut_values("float32")[255] == 0.5


def test_from_pointcloud2_duck_typed_message():
    from mrcc_amd.utils.packed import PackedFrame

    for name, order in (("kinect32", None), ("shuffled", (3, 2, 0, 1)), ("f64_bigendian", (1, 0, 3, 2)), ("no_rgb", None)):
        lay = H.LAYOUTS[name]
        width, height, pad = 9, 4, 12
        xyz, _ = H.coordinates(lay, 36, "third_nan")
        buf = H.build(lay, xyz, H.colours(36), width, height, pad)
        msg = H.Message(buf, lay, width, height, pad, field_order=order)
        frame = PackedFrame.from_pointcloud2(msg)
        assert frame.data is msg.data  # not copied
        assert (frame.width, frame.height, frame.point_step, frame.row_step) == (9, 4, lay["step"], 9 * lay["step"] + 12)
        assert frame.is_bigendian == lay["big"] and frame.xyz_offsets == (lay["x"], lay["y"], lay["z"])
        assert frame.rgb_offset == (-1 if lay["rgb"] is None else lay["rgb"])
        _same(frame.decode_host(color="bytes"), H.decode(buf, lay, width, height, pad))


def test_pack_writes_what_the_reference_reads():
    from mrcc_amd.utils.packed import PackedFrame

    rng = np.random.default_rng(3)
    for name in sorted(H.LAYOUTS):
        lay = H.LAYOUTS[name]
        xyz, _ = H.coordinates(lay, 35, "third_nan")
        rgb = rng.integers(0, 256, size=(35, 3), dtype=np.uint8)
        layout = {"point_step": lay["step"], "x": lay["x"], "y": lay["y"], "z": lay["z"], "rgb": lay["rgb"],
                  "xyz_type": H.F64 if lay["xyz"] == "f8" else H.F32, "rgb_type": lay["rgb_type"], "bigendian": lay["big"]}
        frame = PackedFrame.pack(xyz, rgb, layout=layout, width=7, height=5, row_pad=12)
        want = H.decode(frame.data, lay, 7, 5, 12, keep_nonfinite=True)
        assert np.array_equal(want["points"].view(np.int32), H.decode(H.build(lay, xyz, np.zeros(35, np.uint32), 7, 5, 12),
                                                                      lay, 7, 5, 12, keep_nonfinite=True)["points"].view(np.int32))
        if lay["rgb"] is not None:
            assert np.array_equal(want["rgb"], rgb.astype(np.float32))
    kinect = PackedFrame.pack(np.zeros((6, 3), np.float32), np.zeros((6, 3), np.uint8))
    assert (kinect.point_step, kinect.xyz_offsets, kinect.rgb_offset, kinect.width, kinect.height) == (32, (0, 4, 8), 16, 6, 1)
    with pytest.raises(ValueError, match="width \\* height"):
        PackedFrame.pack(np.zeros((6, 3), np.float32), None, width=4, height=2)


# ---- .pcd files ---------------------------------------------------------------------------------------------------------
def _write_pcd(path, xyz, rgb_u32, data="binary", rgb_type="F", width=None, height=1):
    n = len(xyz)
    width = n if width is None else width
    head = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\n"
            f"TYPE F F F {rgb_type}\nCOUNT 1 1 1 1\nWIDTH {width}\nHEIGHT {height}\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\n"
            f"DATA {data}\n")
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        if data == "binary":
            fh.write(H.build(H.LAYOUTS["pcd16"], xyz, rgb_u32, n, 1).tobytes())
        else:
            for p, c in zip(xyz, rgb_u32):
                colour = repr(float(np.array([c], np.uint32).view(np.float32)[0])) if rgb_type == "F" else str(int(c))
                fh.write((" ".join(repr(float(v)) for v in p) + " " + colour + "\n").encode("ascii"))


def test_from_pcd_binary_and_ascii(tmp_path):
    from mrcc_amd.utils.packed import PackedFrame

    lay = H.LAYOUTS["pcd16"]
    xyz, _ = H.coordinates(lay, 40, "third_nan")
    xyz = np.where(np.isnan(xyz), np.float32("nan"), xyz)  # text cannot carry a payload
    rgb = H.colours(40) & np.uint32(0x00FFFFFF)  # as floats these are denormals or small normals: they print exactly
    want = H.decode(H.build(lay, xyz, rgb, 40, 1), lay, 40, 1)
    for data, rgb_type, shape in (("binary", "F", (40, 1)), ("binary", "U", (8, 5)), ("ascii", "F", (40, 1)),
                                  ("ascii", "U", (8, 5))):
        path = tmp_path / f"{data}_{rgb_type}.pcd"
        _write_pcd(path, xyz, rgb, data, rgb_type, *shape)
        frame = PackedFrame.from_pcd(path)
        assert (frame.width, frame.height, frame.point_step) == (shape[0], shape[1], 16)
        if data == "binary":
            assert isinstance(frame.data, np.memmap)  # the body as it is
        _same(frame.decode_host(color="bytes"), want)
    path = tmp_path / "compressed.pcd"
    path.write_bytes(b"VERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\nWIDTH 1\nHEIGHT 1\nPOINTS 1\n"
                     b"DATA binary_compressed\n\x00\x00")
    with pytest.raises(NotImplementedError, match="binary_compressed"):
        PackedFrame.from_pcd(path)
    (tmp_path / "text.pcd").write_bytes(b"hello\n")
    with pytest.raises(ValueError, match="DATA"):
        PackedFrame.from_pcd(tmp_path / "text.pcd")


def test_from_pcd_on_the_committed_hand_model():
    from mrcc_amd.utils.mesh import read_point_cloud
    from mrcc_amd.utils.packed import PackedFrame

    path = os.path.join(GOLDEN, "hand.pcd")
    frame = PackedFrame.from_pcd(path)
    assert frame.n_records == 4480 and frame.point_step == 16 and frame.rgb_offset == 12
    points, rgb, src = frame.decode_host(color="float32")
    assert np.array_equal(points.astype(np.float64), read_point_cloud(path)) and len(src) == 4480
    assert rgb.dtype == np.float32 and 0 <= rgb.min() and rgb.max() <= 1


# ---- the ros_utils names ---------------------------------------------------------------------------------------------------
def test_ros_utils_names_on_a_message():
    from mrcc_amd.utils import ros_utils

    lay = dict(H.LAYOUTS["kinect32"])
    width, height = 8, 3
    xyz, kept = H.coordinates(lay, 24, "third_nan")
    colours = H.colours(24)
    msg = H.Message(H.build(lay, xyz, colours, width, height), lay, width, height)
    members = ros_utils.fields_to_dtype(msg.fields, msg.point_step)
    names = [n for n, _ in members]
    assert names[:3] == ["x", "y", "z"] and names[3:7] == ["__12", "__13", "__14", "__15"] and names[7] == "rgb"
    assert names[8:] == [f"__{i}" for i in range(20, 32)] and np.dtype(members).itemsize == 32
    assert all(np.dtype(t) == (np.float32 if n in ("x", "y", "z", "rgb") else np.uint8) for n, t in members)
    records = ros_utils.pointcloud2_to_array(msg)
    assert records.shape == (3, 8) and records.dtype.names == ("x", "y", "z", "rgb")
    assert np.array_equal(records["y"].view(np.uint32).reshape(-1), xyz[:, 1].view(np.uint32))
    split = ros_utils.split_rgb_field(records)
    assert split.dtype.names == ("x", "y", "z", "r", "g", "b") and split["r"].dtype == np.uint8
    assert np.array_equal(split["r"].reshape(-1), (colours >> 16) & 255)
    assert np.array_equal(split["g"].reshape(-1), (colours >> 8) & 255) and np.array_equal(split["b"].reshape(-1), colours & 255)
    assert np.array_equal(ros_utils.get_xyz_points(records), xyz[kept].astype(np.float64))
    assert ros_utils.get_xyz_points(records, remove_nans=False, dtype=np.float32).shape == (3, 8, 3)
    want = H.decode(H.build(lay, xyz, colours, width, height), lay, width, height)
    points, rgb = ros_utils.get_points_and_colors(msg)
    assert points.dtype == np.float64 and rgb.dtype == np.float64
    assert np.array_equal(points, want["points"].astype(np.float64)) and np.array_equal(rgb, want["rgb"].astype(np.float64))
    points, rgb = ros_utils.get_points_and_colors(msg, remove_nans=False, dtype=np.float32)
    everything = H.decode(H.build(lay, xyz, colours, width, height), lay, width, height, keep_nonfinite=True)
    assert points.shape == (3, 8, 3) and np.array_equal(rgb.reshape(-1, 3), everything["rgb"])
    assert np.array_equal(np.isnan(points.reshape(-1, 3)), np.isnan(everything["points"]))
    # one row: squeezed
    flat = H.Message(H.build(lay, xyz, colours, 24, 1), lay, 24, 1)
    assert ros_utils.pointcloud2_to_array(flat).shape == (24,)
    assert ros_utils.pointcloud2_to_array(flat, squeeze=False).shape == (1, 24)
    # the freenect engine's colours are this divided by 255: the "float64" convention
    from mrcc_amd.utils.packed import PackedFrame

    assert np.array_equal(ros_utils.get_points_and_colors(msg)[1] / 255,
                          PackedFrame.from_pointcloud2(msg).decode_host(color="float64")[1])


# ---- PCDDataEngine -------------------------------------------------------------------------------------------------------
def _pcd_folder(tmp_path, numbers):
    lay = H.LAYOUTS["pcd16"]
    poses = {}
    for k in numbers:
        xyz, _ = H.coordinates(lay, 50, "third_nan", seed=k)
        xyz[5] = (600.0, 0.0, 0.0)  # outside the +-500 box
        xyz[6] = (0.0, -500.0, 0.0)  # on its bound
        _write_pcd(tmp_path / f"{k}.pcd", xyz, H.colours(50, seed=k))
        poses[k] = np.arange(7, dtype=np.float64) + k  # x y z qx qy qz qw
        np.save(tmp_path / f"{k}.npy", poses[k] + 100)
        np.save(tmp_path / f"{k}_robot2ee_pose.npy", poses[k])
    (tmp_path / "notes.txt").write_text("not a frame")
    return poses


def test_pcd_data_engine(tmp_path):
    from mrcc_amd.app.data_engine import PCDDataEngine, get_roi_mask
    from mrcc_amd.app.dto import PackedCloudDTO, PointCloudDTO

    numbers = (10, 2, 33, 1, 100, 7)
    poses = _pcd_folder(tmp_path, numbers)
    order = sorted(numbers)  # numeric: 2.pcd before 10.pcd
    engine = PCDDataEngine(str(tmp_path), cyclic=False, step=1)
    assert len(engine) == 6 and engine.run() is None and engine.exit() is None
    seen = []
    for k in order:
        dto = engine.get()
        assert isinstance(dto, PointCloudDTO) and dto.id == str(tmp_path / f"{k}.pcd") and dto.gt_pose is None
        assert dto.timestamp is not None
        p = poses[k]
        assert np.array_equal(dto.ee2base_pose, [p[0], p[1], p[2], p[6], p[3], p[4], p[5]])  # wxyz
        assert dto.points.dtype == np.float32 and dto.rgb.dtype == np.float32 and dto.points.shape == dto.rgb.shape
        assert get_roi_mask(dto.points).all() and np.isfinite(dto.points).all() and 20 < len(dto.points) < 49
        assert not (dto.points == np.float32(600)).any() and not (dto.points == np.float32(-500)).any()
        assert 0 <= dto.rgb.min() and dto.rgb.max() <= 1
        seen.append(dto)
    assert engine.get() is None and engine.get() is None  # exhausted
    # every third file, cyclic
    engine = PCDDataEngine(str(tmp_path), step=3)
    assert len(engine) == 2
    ids = [os.path.basename(engine.get().id) for _ in range(5)]
    assert ids == ["1.pcd", "10.pcd", "1.pcd", "10.pcd", "1.pcd"]
    assert len(PCDDataEngine(str(tmp_path))) == 1  # the reference's default step of 10
    # packed: the same frames, still packed
    engine = PCDDataEngine(str(tmp_path), cyclic=False, step=1, packed=True)
    for want in seen:
        dto = engine.get()
        assert isinstance(dto, PackedCloudDTO) and dto.points is None and dto.rgb is None
        assert dto.box == (-500.0, -500.0, -500.0, 500.0, 500.0, 500.0) and dto.color == "float32"
        assert dto.id == want.id and np.array_equal(dto.ee2base_pose, want.ee2base_pose) and dto.gt_pose is None
        host = dto.decoded()
        assert isinstance(host, PointCloudDTO) and host.id == want.id
        assert np.array_equal(host.points, want.points) and np.array_equal(host.rgb, want.rgb)
        assert host.rgb.dtype == np.float32 and np.array_equal(host.ee2base_pose, want.ee2base_pose)
    assert engine.get() is None


def test_packed_cloud_dto_fields():
    import dataclasses

    from mrcc_amd.app.dto import PackedCloudDTO, PointCloudDTO

    names = [f.name for f in dataclasses.fields(PackedCloudDTO)]
    assert names[: len(dataclasses.fields(PointCloudDTO))] == [f.name for f in dataclasses.fields(PointCloudDTO)]
    assert names[-3:] == ["packed", "box", "color"]
