"""Lens distortion of the RGB-D ingest without a GPU: the package's numpy restatement (RGBDFrame.rays_host, decode_host)
against the independent one of tests/rgbd_lens_helpers.py, the argument rules, the C ABI's host-side refusals, and a
rendered plane that only the lens brings back onto itself."""
import ctypes

import numpy as np
import pytest

import rgbd_lens_helpers as L

CASES = L.cases()


def _frame(*a, **kw):
    from mrcc_amd.utils.rgbd import RGBDFrame

    return RGBDFrame(*a, **kw)


def _aligned(K, D, H, W, depth=None):
    return _frame(np.ones((H, W), np.uint16) if depth is None else depth, None, K, depth_D=D)


@pytest.fixture(scope="module")
def tables():
    """name -> the helper's (rays, valid, r2_max, residual), computed once"""
    return {name: L.ray_table(*case) for name, case in CASES.items()}


# ---- 1, 2: the ray table ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_rays_host_equals_the_independent_restatement(name, tables):
    K, D, H, W = CASES[name]
    rays, valid, r2_max, _ = tables[name]
    frame = _aligned(K, D, H, W)
    got = frame.rays_host("color")
    assert got.dtype == np.float64 and got.shape == (H * W * 2 + 1,)
    want = np.concatenate([rays.reshape(-1), [r2_max]])
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    assert np.array_equal(frame.rays_host("depth").view(np.int64), want.view(np.int64))  # aligned: one camera
    assert _aligned(K, D, H, W).rays_host("color") is got  # frames of one camera share the table
    assert _frame(np.ones((H, W), np.uint16), None, K).rays_host("color") is None
    if name == "fold":
        assert valid.sum() == L.FOLD_VALID and (~valid).sum() == L.FOLD_INVALID
        assert np.isnan(got[:-1:2]).sum() == L.FOLD_INVALID and valid[H // 2, W // 2] and not valid[0, 0]


@pytest.mark.parametrize("name", L.ALL_VALID)
def test_round_trip_lands_on_the_pixel(name, tables):
    K, D, H, W = CASES[name]
    rays, valid, r2_max, residual = tables[name]
    assert valid.all() and residual.max() <= 1e-6
    xd, yd = L.forward(D, rays[..., 0], rays[..., 1])
    v, u = np.mgrid[0:H, 0:W]
    assert np.abs(K[0, 0] * xd + K[0, 2] - u).max() <= 1e-6 and np.abs(K[1, 1] * yd + K[1, 2] - v).max() <= 1e-6
    assert r2_max == (rays[..., 0] ** 2 + rays[..., 1] ** 2).max() > 0
    # the lens matters: the pinhole ray of a corner pixel is off by more than a hundredth of a pixel's angle
    pin = np.stack(((u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]), axis=2)
    assert np.abs(pin - rays).max() * K[0, 0] > 0.01


def test_five_rounds_are_not_enough():
    """OpenCV's default inverse stops after 5 rounds; on the rational lens that is not converged"""
    K, D, H, W = CASES["rational"]
    residual = L.ray_table(K, D, H, W, rounds=5)[3]
    assert residual.max() > 1e-3


# ---- 3: argument rules -------------------------------------------------------------------------------------------------
def test_distortion_argument_rules():
    K, D, H, W = CASES["kinect1"]
    depth = np.ones((H, W), np.uint16)
    for n in (4, 5, 8):
        f = _frame(depth, None, K, depth_D=np.arange(1, n + 1) * 1e-3)
        assert f.depth_D.shape == (8,) and np.array_equal(f.depth_D[:n], np.arange(1, n + 1) * 1e-3)
        assert not f.depth_D[n:].any() and f.color_D is f.depth_D and f.has_lens
    for n in (1, 3, 6, 7, 9, 12, 14):
        with pytest.raises(ValueError, match="4, 5 or 8"):
            _frame(depth, None, K, depth_D=np.ones(n))
        with pytest.raises(ValueError, match="4, 5 or 8"):
            _frame(depth, None, K, color_D=np.ones(n))
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="finite"):
            _frame(depth, None, K, depth_D=(0.1, bad, 0, 0, 0))
    # zero D is no D
    plain = _frame(depth, None, K)
    for zero in (np.zeros(5), (0, 0, 0, 0), [], np.zeros(8)):
        f = _frame(depth, None, K, depth_D=zero, color_D=zero)
        assert f.depth_D is None and f.color_D is None and not f.has_lens
        assert set(vars(f)) == set(vars(plain))
        assert np.array_equal(f.decode_host()[0].view(np.int32), plain.decode_host()[0].view(np.int32))
    # a registered frame's cameras are separate; an aligned frame's depth lens is the colour camera's
    reg = _frame(depth, None, K, K, np.eye(4), depth_D=D)
    assert reg.depth_D is not None and reg.color_D is None and reg.has_lens
    assert _frame(depth, None, K, color_D=D).color_D is not None
    with pytest.raises(ValueError, match="which"):
        reg.rays_host("colour")


def test_from_image_msgs_reads_the_lens():
    import rgbd_helpers as H
    from mrcc_amd.utils.rgbd import RGBDFrame

    K, D, h, w = CASES["kinect1"]
    d16 = np.ones((h, w), np.uint16)
    color = np.zeros((h, w, 3), np.uint8)
    msgs = (H.image_msg(d16, "16UC1"), H.image_msg(color, "rgb8"))
    bare = RGBDFrame.from_image_msgs(*msgs, H.camera_info(K))  # an info object with K alone
    assert bare.depth_D is None and not bare.has_lens
    f = RGBDFrame.from_image_msgs(*msgs, L.camera_info(K, D, "plumb_bob"))
    assert np.array_equal(f.depth_D[:5], D) and f.color_D is f.depth_D
    f = RGBDFrame.from_image_msgs(*msgs, L.camera_info(K, L.RATIONAL_D, "rational_polynomial"), L.camera_info(K, D, "plumb_bob"),
                                  color_from_depth=np.eye(4))
    assert np.array_equal(f.depth_D, L.RATIONAL_D) and np.array_equal(f.color_D[:5], D) and not f.color_D[5:].any()
    for info in (L.camera_info(K, (), "plumb_bob"), L.camera_info(K, np.zeros(5), "equidistant"), L.camera_info(K, (), "")):
        assert not RGBDFrame.from_image_msgs(*msgs, info).has_lens
    for model in ("equidistant", "fisheye", ""):
        with pytest.raises(ValueError, match=repr(model)):
            RGBDFrame.from_image_msgs(*msgs, L.camera_info(K, (0.1, 0.01, 0, 0), model))
        with pytest.raises(ValueError, match=repr(model)):
            RGBDFrame.from_image_msgs(*msgs, H.camera_info(K), L.camera_info(K, (0.1, 0.01, 0, 0), model),
                                      color_from_depth=np.eye(4))
    with pytest.raises(ValueError, match="4, 5 or 8"):
        RGBDFrame.from_image_msgs(*msgs, L.camera_info(K, np.ones(14), "rational_polynomial"))


def test_a_lens_without_a_valid_pixel_is_refused():
    # r * (1 - 50 r^2) turns back at r = 0.08; the principal point lies far outside the image, every pixel beyond that
    K = np.array([[20.0, 0, -100.0], [0, 20.0, -100.0], [0, 0, 1]])
    assert not L.ray_table(K, (-50.0, 0, 0, 0), 6, 8)[1].any()
    with pytest.raises(ValueError, match="no valid pixel"):
        _aligned(K, (-50.0, 0, 0, 0), 6, 8).rays_host("color")
    with pytest.raises(ValueError, match="no valid pixel"):
        _aligned(K, (-50.0, 0, 0, 0), 6, 8).decode_host()


# ---- 4: ABI ------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_bound_and_exported():
    import os

    import mrcc_amd

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sv_hip.h")).read()
    lib = mrcc_amd._lib.load()
    for name in ("sv_lens_rays", "sv_rgbd_cloud_lens"):
        assert f"int {name}(" in header and name in mrcc_amd._lib.SIGNATURES and hasattr(lib, name)
    assert "N3g" in header and lib.sv_abi_version() == 4


def test_host_side_refusals_need_no_gpu():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    cam4, dist = (ctypes.c_double * 4)(50.0, 50.0, 3.5, 2.5), (ctypes.c_double * 8)()
    fake = ctypes.c_void_p(256)  # never dereferenced: every call below is refused before any HIP call

    def rays(cam=cam4, D=dist, H=6, W=8, out=fake):
        return lib.sv_lens_rays(cam, D, H, W, out, None)

    def refused(rc, word):
        assert rc == -1 and word in lib.sv_last_error(), lib.sv_last_error()

    refused(rays(cam=None), b"null pointer")
    refused(rays(D=None), b"null pointer")
    refused(rays(out=None), b"null pointer")
    assert b"sv_lens_rays" in lib.sv_last_error()
    refused(rays(H=0), b"at least 1")
    refused(rays(W=-3), b"at least 1")
    refused(rays(H=4097, W=4096), b"2^24")
    refused(rays(H=1 << 40, W=1 << 40), b"2^24")
    refused(rays(cam=(ctypes.c_double * 4)(0.0, 50.0, 1, 1)), b"focal length")
    refused(rays(cam=(ctypes.c_double * 4)(50.0, 50.0, float("nan"), 1)), b"not finite")
    refused(rays(D=(ctypes.c_double * 8)(0, 0, 0, float("inf"))), b"not finite")

    cam = (ctypes.c_double * 21)(50, 50, 3.5, 2.5, 50, 50, 3.5, 2.5, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0.001)
    need = lib.sv_rgbd_cloud_workspace_bytes(6, 8, 6, 8)

    def cloud(depth=fake, flags=0, Hd=6, Wd=8, depth_rays=None, color_rays=None, color_dist=None, count=fake, ws_bytes=need):
        return lib.sv_rgbd_cloud_lens(depth, 4, Hd, Wd, 2 * Wd, None, 6, 8, 0, None, cam, 0, 0, flags, None, None, fake,
                                      ws_bytes, fake, None, None, None, None, count, depth_rays, color_rays, color_dist,
                                      None)

    refused(cloud(depth=None), b"null pointer")
    refused(cloud(count=None, color_rays=fake), b"null pointer")
    assert b"sv_rgbd_cloud_lens" in lib.sv_last_error()
    refused(cloud(Hd=4097, Wd=4096), b"2^24")
    refused(cloud(color_dist=dist), b"color_rays")
    refused(cloud(color_dist=dist, depth_rays=fake), b"color_rays")
    refused(cloud(flags=1, depth_rays=fake), b"SV_RGBD_ALIGNED")
    refused(cloud(flags=1, color_rays=fake, color_dist=dist), b"SV_RGBD_ALIGNED")
    refused(cloud(color_rays=fake, color_dist=(ctypes.c_double * 8)(float("nan"))), b"not finite")
    assert cloud(color_rays=fake, ws_bytes=need - 1) == -2 and b"sv_rgbd_cloud_lens: workspace too small" in lib.sv_last_error()


# ---- 5: geometry -------------------------------------------------------------------------------------------------------
# ten times the largest distance to the plane of the helper's own float64 points (its rays times the float32 depth),
# which measured 5.16e-8 m here: the rounding of the depth to float32 (2^-24 of 1.1 m) and the 1e-6 px validity bound
PLANE_BOUND = 5.2e-7


def test_a_rendered_plane_comes_back_flat_only_with_the_lens():
    H, W = 48, 64
    K = L.barrel_K(H, W)
    rays, valid, _, _ = L.ray_table(K, L.BARREL_D, H, W)
    assert valid.all()
    rx, ry = rays[..., 0], rays[..., 1]
    normal, offset = np.array([0.2, -0.1, -1.0]), 0.9  # z = 0.9 + 0.2 x - 0.1 y

    def off_plane(points):
        return np.abs(points.astype(np.float64) @ normal + offset) / np.linalg.norm(normal)

    depth = (offset / (1.0 - 0.2 * rx + 0.1 * ry)).astype(np.float32)  # along the pixel's ray (rx z, ry z, z)
    assert 0.6 < depth.min() and depth.max() < 1.6
    z = depth.astype(np.float64)
    own = off_plane(np.stack((rx * z, ry * z, z), axis=2).reshape(-1, 3)).max()
    print(f"helper residual {own:.3e} m, bound {PLANE_BOUND:.3e} m")
    assert own * 10 <= PLANE_BOUND * 1.05 and own > 0
    with_lens = _frame(depth, None, K, depth_scale=1.0, depth_D=L.BARREL_D)
    points, _, src = with_lens.decode_host()
    assert len(src) == H * W and points.dtype == np.float32
    print(f"with the lens {off_plane(points).max():.3e} m")
    assert off_plane(points).max() <= PLANE_BOUND
    assert off_plane(with_lens.decode_host64()[0]).max() <= PLANE_BOUND
    taken = with_lens.take(src[::7])[0]
    assert np.array_equal(taken.view(np.int32), points[::7].view(np.int32))
    fresh = _frame(depth, None, K, depth_scale=1.0, depth_D=L.BARREL_D)  # nothing cached: take's aligned fast path
    assert np.array_equal(fresh.take(src[::7])[0].view(np.int32), points[::7].view(np.int32)) and fresh._registered is None
    pinhole = off_plane(_frame(depth, None, K, depth_scale=1.0).decode_host()[0]).max()
    print(f"without it {pinhole:.3e} m")
    assert pinhole > 100 * PLANE_BOUND
