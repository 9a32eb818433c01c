"""RGB-D ingest without a GPU: the numpy restatement (utils/rgbd.py decode_host, registered_host) against the reference's
own filterDiscontinuities, registerDepthMap and registeredDepthMapToPointCloud on tests/golden/rgbd_ycb.npz, bit for bit;
the argument checks of sv_rgbd_cloud, which all fail before any HIP call; image messages; scatter and take."""
import ctypes

import numpy as np
import pytest

import rgbd_helpers as H

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def ycb(golden):
    return golden("rgbd_ycb")


def _frame_b(g, **kw):
    from mrcc_amd.utils.rgbd import RGBDFrame

    return RGBDFrame(g["b_depth"], g["b_color"], g["b_depth_K"], g["b_color_K"], g["b_H"], float(g["b_depth_scale"]),
                     mask=g["b_mask"], **kw)


def test_the_fixture_is_not_trivial(ycb):
    depth = ycb["a_depth"]
    assert depth.shape == (480, 640) and depth.dtype == np.uint16
    assert 0.01 <= len(ycb["a_zeroed"]) / depth.size <= 0.30
    assert (depth.reshape(-1)[ycb["a_zeroed"]] != 0).all() and (depth == 0).any()
    hits, reg, mask = ycb["b_hits"], ycb["b_registered"], ycb["b_mask"]
    assert np.array_equal(hits > 0, reg > 0)
    assert (hits > 1).sum() >= 0.10 * (hits > 0).sum()  # the far / near choice is exercised
    assert (hits > 2).sum() >= 1  # a 3-way collision
    assert ((reg > 0) & (mask > 0)).sum() >= 100
    assert len(ycb["b_cloud"]) == ((reg > 0) & (mask == 0)).sum() >= 1000
    assert ycb["b_depth"].shape != reg.shape


def test_filter_equals_the_reference(ycb):
    frame = H.filter_frame(ycb["a_depth"], int(ycb["a_filter_size"]), int(ycb["a_filter_thresh"]))
    want = ycb["a_depth"].astype(np.float64).reshape(-1)
    want[ycb["a_zeroed"]] = 0.0
    assert H.same_bits(frame.filtered_host().reshape(-1), want)
    assert H.same_bits(frame.registered_host().reshape(-1), want)  # aligned, unit scale


def test_registration_and_cloud_equal_the_reference(ycb):
    frame = _frame_b(ycb)
    assert H.same_bits(frame.registered_host(), ycb["b_registered"])
    cloud = ycb["b_cloud"]
    points, rgb, src = frame.decode_host(color="bytes")
    assert points.dtype == np.float32 and H.same_bits(points, cloud[:, :3].astype(np.float32))
    assert rgb.dtype == np.uint8 and np.array_equal(rgb, cloud[:, 3:])
    keep = (ycb["b_registered"] > 0) & (ycb["b_mask"] == 0)
    assert src.dtype == np.int64 and np.array_equal(src, np.nonzero(keep.reshape(-1))[0])
    points64, src64 = frame.decode_host64()
    assert H.same_bits(points64, cloud[:, :3]) and np.array_equal(src64, src)
    # the colour conventions of utils/packed.py
    assert np.array_equal(frame.decode_host()[1], cloud[:, 3:] / 255.0)
    lut = np.linspace(-1, 1, 256).astype(np.float32)
    assert np.array_equal(frame.decode_host(lut=lut)[1], lut[cloud[:, 3:].astype(np.int64)])


def test_near_keeps_the_smallest_depth(ycb):
    far, near = _frame_b(ycb).registered_host(), _frame_b(ycb, keep="near").registered_host()
    hits = ycb["b_hits"]
    assert np.array_equal(far > 0, near > 0) and (near <= far).all()
    assert H.same_bits(far[hits == 1], near[hits == 1])
    assert (near[hits > 1] < far[hits > 1]).mean() > 0.5  # equal depths may collide, most do not


def test_argument_validation_without_gpu():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    p = ctypes.create_string_buffer(64)  # stands in for a non-null pointer: every call here fails its checks
    need = lib.sv_rgbd_cloud_workspace_bytes(48, 64, 60, 80)
    assert need >= 60 * 80 * 8 + 19 * 4 and lib.sv_rgbd_cloud_workspace_bytes(1 << 12, 1 << 12, 1 << 12, 1 << 12) >= 1 << 27
    good_cam = [58.0, 58.5, 31.5, 23.5, 52.0, 52.5, 40.2, 29.7, 1, 0, 0, 0.025, 0, 1, 0, 0, 0, 0, 1, 0, 0.001]

    def cloud(typ=H.U16, Hd=48, Wd=64, drow=128, Hc=60, Wc=80, crow=240, cam=good_cam, fsize=0, thresh=1000, flags=0,
              box=None, ws_bytes=need, **ptrs):
        a = dict(depth=p, color=p, mask=None, lut=None, ws=p, points=p, points64=None, rgb=p, src=None, registered=None,
                 count=p)
        a.update(ptrs)
        return lib.sv_rgbd_cloud(a["depth"], typ, Hd, Wd, drow, a["color"], Hc, Wc, crow, a["mask"],
                                 None if cam is None else (ctypes.c_double * 21)(*cam), fsize, thresh, flags,
                                 None if box is None else (ctypes.c_double * 6)(*box), a["lut"], a["ws"], ws_bytes,
                                 a["points"], a["points64"], a["rgb"], a["src"], a["registered"], a["count"], None)

    def rejected(word, **kw):
        assert cloud(**kw) == -1 and word in lib.sv_last_error(), (kw, lib.sv_last_error())

    def cam_with(i, value):
        return good_cam[:i] + [value] + good_cam[i + 1:]

    for kw in ({"Hd": 0}, {"Wd": -1}, {"Hc": 0}, {"Wc": 0}):
        rejected(b"dimensions", **kw)
    for kw in ({"Hd": 1 << 12, "Wd": (1 << 12) + 1, "drow": 1 << 14}, {"Hc": 1 << 24, "Wc": 2, "crow": 6},
               {"Hd": 1 << 40, "Wd": 1 << 40, "drow": 1 << 42}):
        rejected(b"2^24 pixels", **kw)
    for typ in (0, 2, 8):
        rejected(b"depth_type", typ=typ)
    for kw in ({"drow": 127}, {"drow": 0}, {"drow": -128}, {"typ": H.F32, "drow": 255}):
        rejected(b"depth_row_bytes", **kw)
    for crow in (239, 0, -240):
        rejected(b"color_row_bytes", crow=crow)
    for flags in (8, 16, -1):
        rejected(b"flags", flags=flags)
    for fsize in (1, 2, 4, 17, -3):
        rejected(b"filter_size", fsize=fsize)
    rejected(b"SV_DEPTH_U16 depth only", typ=H.F32, drow=256, fsize=7)
    rejected(b"filter_thresh", fsize=7, thresh=-1)
    rejected(b"cam_host", cam=None)
    for i in (0, 3, 7, 8, 19, 20):
        for bad in (NAN, INF, -INF):
            rejected(b"not finite", cam=cam_with(i, bad))
    for i in (0, 1, 4, 5):
        rejected(b"focal length", cam=cam_with(i, 0.0))
    rejected(b"depth_scale", cam=cam_with(20, 0.0))
    for kw in ({}, {"Hc": 48, "Wc": 80}, {"Hc": 64, "Wc": 48, "crow": 144}):
        rejected(b"SV_RGBD_ALIGNED", flags=H.ALIGNED, **kw)
    for box in ((NAN, 0, 0, 1, 1, 1), (0, 0, 0, 1, NAN, 1)):
        rejected(b"NaN", box=box)
    for box in ((2, 0, 0, 1, 1, 1), (0, 0, 1.5, 1, 1, 1)):
        rejected(b"lo <= hi", box=box)
    for name in ("depth", "ws", "points", "rgb", "count"):
        rejected(b"null pointer", **{name: None})
    for ws_bytes in (0, 8, need - 1):
        assert cloud(ws_bytes=ws_bytes) == -2 and b"workspace too small" in lib.sv_last_error(), ws_bytes
    assert b"sv_rgbd_cloud" in lib.sv_last_error()
    assert cloud(Hc=120, Wc=160, crow=480) == -2  # one size does not fit more


def test_frame_rejects_bad_arguments():
    from mrcc_amd._lib import SvHipError
    from mrcc_amd.utils.rgbd import RGBDFrame

    depth, color, K = np.ones((6, 8), np.uint16), np.zeros((6, 8, 3), np.uint8), np.eye(3)
    RGBDFrame(depth, color, K)
    cases = [
        (dict(color=np.zeros((5, 8, 3), np.uint8)), "one size"), (dict(depth=np.ones((6, 8, 1))), r"\[H, W\]"),
        (dict(color=np.zeros((6, 8, 4), np.uint8)), r"\[H, W, 3\]"), (dict(depth_K=np.eye(4)), "9 values"),
        (dict(color_from_depth=np.eye(3)), "4 x 4"), (dict(filter_size=4), "filter_size"), (dict(filter_size=17), "filter_size"),
        (dict(depth=np.ones((6, 8), np.float32), filter_size=3), "uint16"), (dict(filter_thresh=-1), "filter_thresh"),
        (dict(depth_scale=0.0), "zero"), (dict(depth_K=np.diag([0.0, 1, 1])), "zero"), (dict(depth_scale=NAN), "finite"),
        (dict(mask=np.zeros((6, 7))), "mask"), (dict(keep="nearest"), "keep"), (dict(color_order="gbr"), "color_order"),
        (dict(depth=np.full((6, 8), 70000)), "do not fit"),
    ]
    for change, word in cases:
        kw = dict(depth=depth, color=color, depth_K=K)
        kw.update(change)
        with pytest.raises(ValueError, match=word):
            RGBDFrame(**kw)
    frame = RGBDFrame(depth, color, K)
    for fn in (lambda: frame.decode_host(box=(0, 0, 0, 1, 1)), lambda: frame.unpack(None, box=(2, 0, 0, 1, 1, 1)),
               lambda: frame.decode_device("cuda:0", box=(NAN, 0, 0, 1, 1, 1))):
        with pytest.raises(ValueError, match="6 values|lo <= hi|NaN"):
            fn()
    with pytest.raises(SvHipError, match="no CPU fallback"):
        frame.decode_device("cpu")
    with pytest.raises(ValueError, match="color"):
        frame.decode_host(color="rgb")
    with pytest.raises(IndexError):
        frame.take([48])
    with pytest.raises(ValueError, match="same length"):
        frame.scatter(np.zeros(3), np.zeros(4, np.int64))


def test_from_image_msgs():
    from mrcc_amd.utils.rgbd import RGBDFrame

    rng = np.random.default_rng(5)
    d16 = rng.integers(0, 3000, size=(9, 13)).astype(np.uint16)
    d32 = (d16 * np.float32(0.001)).astype(np.float32)
    color = rng.integers(0, 256, size=(9, 13, 3), dtype=np.uint8)
    K = np.array([[11.0, 0, 6.2], [0, 11.5, 4.1], [0, 0, 1]])
    plain = RGBDFrame(d16, color, K)
    want = plain.decode_host(color="bytes")
    for dpad, cpad in ((0, 0), (3, 5)):
        f = RGBDFrame.from_image_msgs(H.image_msg(d16, "16UC1", dpad), H.image_msg(color, "rgb8", cpad), H.camera_info(K))
        assert f.aligned and f.depth_scale == 0.001 and f.color_order == "rgb"
        assert (f.depth_row_bytes, f.color_row_bytes) == (26 + dpad, 39 + cpad)
        assert f.n_records == 117 and f.rgb_offset == 8 * (26 + dpad) + 26
        assert f.nbytes_used == f.rgb_offset + 8 * (39 + cpad) + 39 == len(f._bytes())
        for a, b in zip(f.decode_host(color="bytes"), want):
            assert H.same_bits(a, b)
    # bgr8: the bytes are swapped on decoding
    f = RGBDFrame.from_image_msgs(H.image_msg(d16, "16UC1"), H.image_msg(color[:, :, ::-1], "bgr8", 2), H.camera_info(K))
    assert f.color_order == "bgr" and np.array_equal(f.decode_host(color="bytes")[1], want[1])
    # 32FC1: metres, scale 1
    f = RGBDFrame.from_image_msgs(H.image_msg(d32, "32FC1", 4), H.image_msg(color, "rgb8"), H.camera_info(K))
    assert f.depth_scale == 1.0 and f.depth.dtype == np.float32 and f.depth_row_bytes == 56
    assert H.same_bits(f.registered_host(), d32.astype(np.float64))
    assert np.array_equal(f.decode_host()[2], want[2])
    # two cameras: registered, the colour camera's own K
    Hm = np.eye(4)
    Hm[0, 3] = 0.01
    big = rng.integers(0, 256, size=(12, 16, 3), dtype=np.uint8)
    f = RGBDFrame.from_image_msgs(H.image_msg(d16, "16UC1", 2), H.image_msg(big, "rgb8", 1), H.camera_info(K),
                                  H.camera_info(K * 1.2), color_from_depth=Hm, keep="near")
    g = RGBDFrame(d16, big, K, K * 1.2, Hm, keep="near")
    assert not f.aligned and (f.Hc, f.Wc) == (12, 16) and H.same_bits(f.registered_host(), g.registered_host())
    # no colour image
    f = RGBDFrame.from_image_msgs(H.image_msg(d16, "16UC1"), None, H.camera_info(K))
    assert f.rgb_offset == -1 and f.decode_host()[1] is None
    for msgs, word in (((H.image_msg(d16, "16UC1", big=True), H.image_msg(color, "rgb8")), "big-endian"),
                       ((H.image_msg(d32, "32FC1", big=True), H.image_msg(color, "rgb8")), "big-endian"),
                       ((H.image_msg(d16, "mono16"), H.image_msg(color, "rgb8")), "depth encoding"),
                       ((H.image_msg(d16, "16UC1"), H.image_msg(color, "rgba8")), "colour encoding")):
        with pytest.raises(ValueError, match=word):
            RGBDFrame.from_image_msgs(*msgs, H.camera_info(K))
    short = H.image_msg(d16, "16UC1")
    short.data = short.data[:-1]
    with pytest.raises(ValueError, match="covering"):
        RGBDFrame.from_image_msgs(short, None, H.camera_info(K))


def test_scatter_and_take_round_trip():
    from mrcc_amd.utils.rgbd import RGBDFrame

    rng = np.random.default_rng(6)
    depth = rng.integers(0, 4, size=(10, 14)).astype(np.uint16) * 500
    color = rng.integers(0, 256, size=(10, 14, 3), dtype=np.uint8)
    K = np.array([[12.0, 0, 6.5], [0, 12.5, 4.5], [0, 0, 1]])
    lut = np.linspace(-0.5, 0.5, 256)
    Hm = np.eye(4)
    Hm[:3, 3] = (0.02, 0.0, 0.01)
    for frame in (RGBDFrame(depth, color, K), RGBDFrame(depth, color, K, filter_size=3, filter_thresh=600),
                  RGBDFrame(depth, color, K, K, Hm), RGBDFrame(depth, color, K, color_order="bgr")):
        points, rgb, src = frame.decode_host(lut=lut)
        assert 20 < len(src) < 140
        labels = rng.integers(0, 3, size=len(src))
        image = frame.scatter(labels, src)
        assert image.shape == (10, 14) and np.array_equal(image.reshape(-1)[src], labels)
        assert (image == -1).sum() == 140 - len(src) and (frame.scatter(labels, src, fill=9) == 9).sum() == 140 - len(src)
        pick = rng.permutation(len(src))[:15]
        tp, tc = frame.take(src[pick], lut=lut)
        assert H.same_bits(tp, points[pick]) and tc.dtype == np.float64 and np.array_equal(tc, rgb[pick])
        assert np.array_equal(frame.take(src[pick], color="float32")[1], frame.decode_host(color="float32")[1][pick])
        empty = frame.take(np.zeros(0, np.int64))
        assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3)
