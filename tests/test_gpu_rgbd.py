"""sv_rgbd_cloud on the device against the numpy restatement (RGBDFrame.decode_host / decode_host64 / registered_host,
pinned to the reference's own functions by tests/test_rgbd_cpu.py) and against the golden fixture directly.  Every
comparison is of bits; the designed cases also state their expectation outright, so the restatement is not the only witness.
Images are small: the sizes sit around the filter tile and the compaction tile the package exports."""
import numpy as np
import pytest

import rgbd_helpers as H

pytestmark = pytest.mark.gpu


def _frame(*a, **kw):
    from mrcc_amd.utils.rgbd import RGBDFrame

    return RGBDFrame(*a, **kw)


def _marked(out, depth):
    """flat indices of the pixels the device's filter zeroed (aligned frame, unit scale: registered = filtered depth)"""
    return np.nonzero((out["registered"].reshape(-1) == 0) & (np.asarray(depth).reshape(-1) != 0))[0]


# ---- stage 1: filter -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((37, 53), (64, 64)))
def test_filter_on_noisy_steps(gpu, shape):
    rng = np.random.default_rng(shape[0])
    v, u = np.mgrid[0:shape[0], 0:shape[1]]
    depth = (3000 + 40 * u + rng.integers(-300, 300, size=shape)).astype(np.uint16)
    depth[shape[0] // 3: shape[0] // 2, 5:30] = 800
    depth.reshape(-1)[rng.permutation(depth.size)[:12]] = 0
    out = H.check(H.filter_frame(depth, 7, 1000), gpu, depth_pad=3)
    assert 0.05 * depth.size < len(_marked(out, depth)) < 0.8 * depth.size


def test_filter_image_smaller_than_or_equal_to_the_window(gpu):
    for n, want in ((5, []), (7, [24])):
        depth = np.full((n, n), 4000, np.uint16)
        depth[0, 0] = 9000  # inside the one 7 x 7 window there is
        out = H.check(H.filter_frame(depth, 7, 1000), gpu)
        assert list(_marked(out, depth)) == want and out["count"] == n * n - len(want)


def test_filter_marks_reach_the_first_and_last_interior_rows_and_columns(gpu):
    depth = np.full((21, 45), 5000, np.uint16)
    depth[0, :] = depth[-1, :] = 9000  # the border itself never changes
    depth[:, 0] = depth[:, -1] = 9000
    out = H.check(H.filter_frame(depth, 7, 1000), gpu)
    reg = out["registered"]
    inner = np.zeros(depth.shape, bool)
    inner[3:-3, 3:-3] = True
    ring = inner.copy()
    ring[4:-4, 4:-4] = False  # the outermost interior pixels are the only ones whose window reaches the border
    assert np.array_equal(reg == 0, ring) and np.array_equal(reg[~ring], depth[~ring].astype(np.float64))


@pytest.mark.parametrize("size", (3, 7, 15))
def test_filter_step_edge_across_the_tile_seams(gpu, size):
    (th, tw), _ = H.tiles()
    o = size // 2
    rows, cols = 2 * th + 5, 2 * tw + 7
    for axis, seam, extent in ((1, tw, cols), (0, th, rows), (1, 2 * tw, cols), (0, 2 * th, rows)):
        for shift in (0, 1, -1):  # the edge on the seam and one pixel to either side of it
            edge = seam + shift
            depth = np.full((rows, cols), 3000, np.uint16)
            (depth[:, edge:] if axis == 1 else depth[edge:, :])[...] = 6000
            out = H.check(H.filter_frame(depth, size, 1000), gpu)
            want = np.zeros(depth.shape, bool)
            lo, hi = max(edge - o, o), min(edge + o, extent - o)  # windows that hold both sides, interior only
            if axis == 1:
                want[o:rows - o, lo:hi] = True
            else:
                want[lo:hi, o:cols - o] = True
            assert np.array_equal(out["registered"] == 0, want), (size, axis, edge)


def test_filter_threshold_is_strict(gpu):
    for extra, marked in ((0, 0), (1, 9)):
        depth = np.full((9, 11), 4000, np.uint16)
        depth[4, 5] = 4000 + 1000 + extra
        out = H.check(H.filter_frame(depth, 3, 1000), gpu)
        assert len(_marked(out, depth)) == marked
    for thresh, marked in ((65534, 25), (65535, 0)):  # 0 and 65535 in one window: the difference is taken in integers
        depth = np.full((9, 11), 65535, np.uint16)
        depth[4, 5] = 0
        out = H.check(H.filter_frame(depth, 5, thresh), gpu)
        assert (out["registered"] == 0).sum() == max(marked, 1) and len(_marked(out, depth)) == max(marked - 1, 0)


def test_filter_golden(gpu, golden):
    g = golden("rgbd_ycb")
    frame = H.filter_frame(g["a_depth"], int(g["a_filter_size"]), int(g["a_filter_thresh"]))
    out = H.run(frame, gpu, want64=False, want_src=False)
    assert np.array_equal(_marked(out, g["a_depth"]), g["a_zeroed"])
    want = g["a_depth"].astype(np.float64).reshape(-1)
    want[g["a_zeroed"]] = 0.0
    assert H.same_bits(out["registered"].reshape(-1), want) and out["count"] == (want > 0).sum()


# ---- stage 2: registration ---------------------------------------------------------------------------------------------
def _golden_frame(g, **kw):
    return _frame(g["b_depth"], g["b_color"], g["b_depth_K"], g["b_color_K"], g["b_H"], float(g["b_depth_scale"]),
                  mask=g["b_mask"], **kw)


def test_registration_golden_far_and_near(gpu, golden):
    g = golden("rgbd_ycb")
    out = H.check(_golden_frame(g), gpu, depth_pad=2, color_pad=1)
    cloud = g["b_cloud"]
    assert H.same_bits(out["registered"], g["b_registered"])
    assert H.same_bits(out["points64"], cloud[:, :3]) and H.same_bits(out["points"], cloud[:, :3].astype(np.float32))
    assert np.array_equal(out["rgb"], cloud[:, 3:].astype(np.float32))
    near = H.check(_golden_frame(g, keep="near"), gpu)
    multi = g["b_hits"] > 1
    assert (near["registered"][multi] < out["registered"][multi]).mean() > 0.5
    assert H.same_bits(near["registered"][~multi], out["registered"][~multi])


def test_registration_identity_maps_every_pixel_to_itself(gpu):
    rng = np.random.default_rng(3)
    depth = rng.integers(300, 5000, size=(40, 70)).astype(np.uint16)
    depth.reshape(-1)[rng.permutation(depth.size)[:200]] = 0
    K = np.array([[61.3, 0, 34.7], [0, 60.9, 19.2], [0, 0, 1]])
    out = H.check(_frame(depth, None, K, K, np.eye(4)), gpu)
    assert H.same_bits(out["registered"], depth.astype(np.float64) * 0.001)
    assert np.array_equal(out["src"], np.nonzero(depth.reshape(-1))[0])


def test_registration_drops_what_lies_behind_the_colour_camera(gpu):
    v, u = np.mgrid[0:24, 0:40]
    depth = (512 + 64 * u).astype(np.uint16)  # d = 0.5 ... 2.94 in steps of 1/16: column 8 is d == 1 exactly
    K = np.array([[30.0, 0, 20.0], [0, 30.0, 12.0], [0, 0, 1]])
    color_K = np.array([[30.0, 0, 50.0], [0, 30.0, 30.0], [0, 0, 1]])
    Hm = np.eye(4)
    Hm[2, 3] = -1.0  # Z = d - 1: negative left of column 8, exactly 0 on it (a plane through the colour camera's centre)
    color = np.zeros((60, 100, 3), np.uint8)
    out = H.check(_frame(depth, color, K, color_K, Hm, depth_scale=1.0 / 1024), gpu)
    d = depth.astype(np.float64) / 1024
    landed = out["registered"][out["registered"] > 0]
    assert out["count"] == len(landed) > 50 and (out["registered"] >= 0).all()
    assert set(landed) <= set((d - 1.0)[d > 1.0]) and landed.min() >= 1.0 / 16
    only_behind = _frame(depth[:, :9], color, K, color_K, Hm, depth_scale=1.0 / 1024)
    assert H.check(only_behind, gpu)["count"] == 0


def test_registration_rounds_like_int(gpu):
    """uu = (1 * (u + tx)) * 1 + 0 with u = 0: the candidate's column is trunc(tx + 0.5)"""
    eps = 2.0 ** -40
    Wc = 5
    for tx, column in ((-0.5, 0), (-1.5 + eps, 0), (-1.5, None), (-0.5 - eps, 0), (Wc - 0.5, None), (Wc - 0.5 - eps, Wc - 1),
                       (1.5, 2), (2.5 - eps, 2)):
        Hm = np.eye(4)
        Hm[0, 3] = tx
        for transpose in (False, True):  # the same along v
            if transpose:
                Hm = Hm[[1, 0, 2, 3]][:, [1, 0, 2, 3]]
            shape = (Wc, 1) if transpose else (1, Wc)
            frame = _frame(np.ones((1, 1), np.uint16), np.zeros(shape + (3,), np.uint8), H.SIMPLE_K, H.SIMPLE_K, Hm,
                           depth_scale=1.0)
            out = H.check(frame, gpu)
            assert list(out["src"]) == ([] if column is None else [column]), (tx, transpose)


def test_registration_three_way_collision(gpu):
    depth = np.array([[1, 2, 3, 0, 5]], np.uint16)
    color_K = np.array([[2.0 ** -10, 0, 2.0], [0, 1.0, 0], [0, 0, 1]])  # every ray lands on column 2
    for keep, z in (("far", 5.0), ("near", 1.0)):
        frame = _frame(depth, np.zeros((1, 4, 3), np.uint8), H.SIMPLE_K, color_K, np.eye(4), depth_scale=1.0, keep=keep)
        out = H.check(frame, gpu)
        assert list(out["src"]) == [2] and out["registered"][0, 2] == z and out["points64"][0, 2] == z


# ---- stage 3: cloud ----------------------------------------------------------------------------------------------------
def _aligned(depth, seed=0, **kw):
    rng = np.random.default_rng(seed)
    color = rng.integers(0, 256, size=np.shape(depth) + (3,), dtype=np.uint8)
    return _frame(depth, color, np.array([[20.5, 0, 7.25], [0, 21.0, 3.5], [0, 0, 1]]), **kw)


def test_cloud_kept_counts_and_tile_patterns(gpu):
    _, tile = H.tiles()
    none = H.check(_aligned(np.zeros((5, 100), np.uint16)), gpu)
    assert none["count"] == 0
    one = np.zeros((5, 100), np.uint16)
    one[3, 77] = 1234
    assert list(H.check(_aligned(one), gpu)["src"]) == [377]
    assert H.check(_aligned(np.full((5, 100), 900, np.uint16)), gpu)["count"] == 500
    # rows of one compaction tile each: full, every third pixel, full, empty, full but for its last pixel; then a short tile
    depth = np.full((6, tile), 1500, np.uint16)
    depth[1, np.arange(tile) % 3 != 0] = 0
    depth[3] = 0
    depth[4, -1] = 0
    depth = np.concatenate([depth.reshape(-1), np.full(37, 700, np.uint16)]).reshape(1, -1)
    out = H.check(_aligned(depth), gpu)
    assert out["count"] == 3 * tile + len(range(0, tile, 3)) + (tile - 1) + 37
    for w in (63, 64, 65, tile - 1, tile + 1):  # wave and tile boundaries
        rng = np.random.default_rng(w)
        H.check(_aligned((rng.integers(0, 2, size=(3, w)) * 1000).astype(np.uint16)), gpu)


def test_cloud_mask_box_lut_and_colour_order(gpu):
    rng = np.random.default_rng(11)
    depth = rng.integers(1, 8, size=(12, 50)).astype(np.uint16)
    mask = rng.random((12, 50)) < 0.3
    color = rng.integers(0, 256, size=(12, 50, 3), dtype=np.uint8)
    lut = np.linspace(-0.5, 0.5, 256).astype(np.float32)
    plain = _frame(depth, color, H.SIMPLE_K, depth_scale=1.0)
    out = H.check(_frame(depth, color, H.SIMPLE_K, depth_scale=1.0, mask=mask), gpu, lut=lut)
    assert np.array_equal(out["src"], np.nonzero(~mask.reshape(-1))[0])
    assert np.array_equal(out["rgb"], lut[color.reshape(-1, 3)[out["src"]]])
    # z is the raw integer: the bounds 2 and 5 are hit exactly and excluded; x = u * z likewise at 0 and 40
    box = (0.0, -1.0, 2.0, 40.0, 1000.0, 5.0)
    out = H.check(plain, gpu, box=box)
    v, u = np.mgrid[0:12, 0:50]
    keep = (depth > 2) & (depth < 5) & (u * depth > 0) & (u * depth < 40)
    assert np.array_equal(out["src"], np.nonzero(keep.reshape(-1))[0]) and 20 < out["count"] < 300
    assert ((u * depth == 40) & (depth > 2) & (depth < 5)).any() and (depth == 2).any() and (depth == 5).any()
    bgr = H.check(_frame(depth, color, H.SIMPLE_K, depth_scale=1.0, color_order="bgr"), gpu)
    rgb = H.check(plain, gpu)
    assert np.array_equal(bgr["rgb"], rgb["rgb"][:, ::-1]) and np.array_equal(rgb["rgb"], color.reshape(-1, 3).astype(np.float32))


def test_cloud_padded_rows_and_an_odd_colour_address(gpu):
    rng = np.random.default_rng(12)
    depth = rng.integers(0, 3000, size=(17, 33)).astype(np.uint16)
    frame = _aligned(depth, seed=1, mask=rng.random((17, 33)) < 0.2)
    want = H.check(frame, gpu)
    for layout in (dict(depth_pad=1), dict(color_pad=1), dict(depth_pad=6, color_pad=5), dict(color_shift=1),
                   dict(depth_pad=3, color_pad=2, color_shift=3)):
        out = H.check(frame, gpu, seed=7, **layout)
        assert all(H.same_bits(out[k], want[k]) for k in ("points", "points64", "rgb", "src", "registered"))
    filtered = _aligned(depth, seed=1, filter_size=5, filter_thresh=800)
    assert 0 < H.check(filtered, gpu, depth_pad=5)["count"] < (depth > 0).sum()


def test_cloud_float_depth(gpu):
    rng = np.random.default_rng(13)
    depth = rng.uniform(0.3, 4.0, size=(11, 40)).astype(np.float32)
    flat = depth.reshape(-1)
    flat[::7] = np.nan
    flat[1::7] = np.inf
    flat[2::7] = -np.inf
    flat[3::7] = -1.5
    flat[4::7] = 0.0
    flat[5] = -0.0
    flat[6] = np.float32(1e-42)  # a denormal is finite and positive
    valid = np.isfinite(flat) & (flat > 0)
    out = H.check(_aligned(depth, depth_scale=1.0), gpu, depth_pad=2)
    assert np.array_equal(out["src"], np.nonzero(valid)[0]) and 6 in out["src"]
    assert H.same_bits(out["registered"].reshape(-1), np.where(valid, flat, 0).astype(np.float64))
    Hm = np.eye(4)
    Hm[0, 3] = 0.03
    K = np.array([[20.5, 0, 7.25], [0, 21.0, 3.5], [0, 0, 1]])
    H.check(_frame(depth, None, K, K * 1.1, Hm, depth_scale=1.0), gpu)


def test_cloud_repeated_calls_and_optional_outputs(gpu, golden):
    g = golden("rgbd_ycb")
    frame = _golden_frame(g)
    first, second = H.run(frame, gpu), H.run(frame, gpu, seed=1)
    assert first["count_tensor"].is_cuda and first["count_tensor"].dtype.is_floating_point is False
    for k in ("points", "points64", "rgb", "src", "registered"):
        assert H.same_bits(first[k], second[k]), k
    bare = H.check(frame, gpu, want64=False, want_src=False, want_registered=False)
    assert bare["points64"] is None and bare["src"] is None and bare["registered"] is None
    assert H.same_bits(bare["points"], first["points"]) and H.same_bits(bare["rgb"], first["rgb"])


def test_frame_wrappers_leave_everything_on_the_device(gpu, golden):
    import torch

    g = golden("rgbd_ycb")
    frame = _golden_frame(g)
    d_bytes = torch.from_numpy(frame._bytes()).to(gpu)
    points, rgb, src, count, points64, registered = frame.unpack(d_bytes, want_points64=True, want_registered=True)
    assert all(t.is_cuda for t in (points, rgb, src, count, points64, registered))
    assert points.shape == rgb.shape == (4800, 3) and src.shape == (4800,) and count.shape == (1,)
    k = int(count.item())
    cloud = g["b_cloud"]
    assert k == len(cloud) and H.same_bits(points64[:k].cpu().numpy(), cloud[:, :3])
    assert H.same_bits(registered.cpu().numpy(), g["b_registered"])
    lut = np.linspace(0, 1, 256).astype(np.float32)
    p, c, s = frame.decode_device(gpu, lut=torch.from_numpy(lut).to(gpu))
    assert H.same_bits(p.cpu().numpy(), cloud[:, :3].astype(np.float32)) and s.dtype == torch.int32
    assert np.array_equal(c.cpu().numpy(), lut[cloud[:, 3:].astype(np.int64)])
    hs = frame.decode_host()[2]
    p, c, s = frame.decode_device(gpu, lut="float64", box=(-0.2, -1, 0, 0.3, 1, 1.05))
    want = frame.decode_host(box=(-0.2, -1, 0, 0.3, 1, 1.05))
    assert 0 < len(s) < k and np.array_equal(s.cpu().numpy(), want[2]) and H.same_bits(p.cpu().numpy(), want[0])
    from mrcc_amd.utils.packed import device_lut_values

    assert np.array_equal(c.cpu().numpy(), device_lut_values("float64")[cloud[:, 3:].astype(np.int64)][np.isin(hs, want[2])])
