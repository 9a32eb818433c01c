"""Label synthesis without a GPU: the numpy restatement of tests/label_helpers.py against the reference's recorded
results (tests/golden/labels.npz, written by tools/make_golden.py labels), utils/transformation.py's three line
functions against the same fixture, and the host argument checks of the N6 entries and of utils/data.py's entry points
(nothing reaches a device).

Bounds: indices, masks and labels exact - the fixture's generator only writes a case whose every decision clears its
tipping point by more than 1e-9 (1e-6 where the reference computes in float32), far above what a different summation
order inside numpy's batched matmul can move a float64 value of this size (a few 1e-17).  Key points and distances
within 1e-12 (coordinates below 1 m: 4500 ulp of float64).
"""
import ctypes

import numpy as np
import pytest
import torch

import label_helpers as H

N6 = ("sv_ee_mask", "sv_key_points", "sv_line_topk", "sv_line_topk_workspace_bytes", "sv_radius_labels")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("labels")


def test_restatement_matches_the_reference_fixture(fx):
    assert int(fx["n_cases"]) == 4
    found10, found6, sections = set(), set(), []
    for ci in range(4):
        g = lambda k: fx[f"c{ci}_{k}"]  # noqa: E731
        points, pose = g("points"), g("pose")
        assert points.dtype == (np.float64 if ci == 3 else np.float32) and pose.dtype == np.float64
        ee = H.ee_idx(points, pose)
        assert np.array_equal(ee, g("ee_idx")) and 0 < len(ee) < len(points)
        crop = points[ee]
        dist, idx = H.cross_section(crop, pose, int(fx["count"]), float(fx["cutoff"]))
        assert np.array_equal(idx, g("cs_idx"))
        e_cs = float(np.abs(dist - g("cs_dists")).max())
        sections.append(len(idx))
        kp, kidx = H.key_points(crop, pose)
        assert np.array_equal(kidx, g("kp10_idx"))
        e10 = float(np.abs(kp - g("kp10")).max())
        kp6, kidx6, empty = H.six_key_points(crop, pose)
        assert not empty and np.array_equal(kidx6, g("kp6_idx"))
        e6 = float(np.abs(kp6 - g("kp6")).max())
        print(f"case {ci}: crop {len(crop)}, cross-section {len(idx)} (max err {e_cs:.1e}), key points err {e10:.1e} / {e6:.1e}")
        assert max(e_cs, e10, e6) <= 1e-12
        for name, k in (("10", kidx), ("6", kidx6)):
            pcls, pidx = H.collect_closest_points(k[k > -1], crop, float(fx["radius"]))
            assert np.array_equal(pcls, g("pcls" + name)) and np.array_equal(pidx, g("pidx" + name))
            assert np.array_equal(H.radius_labels(crop, k, float(fx["radius"])), g("labels" + name))
        found10.add(bool((kidx > -1).all()))
        found6.add(bool((kidx6 > -1).all()))
    assert found10 == {True, False} and False in found6  # both branches of the threshold test are in the fixture
    assert min(sections) < int(fx["count"]) == max(sections)  # fewer candidates than count, and more
    # the float64 copy of case 1 selects the same rows; its float32 twin rounds p - pos first, so the distances differ
    assert np.array_equal(fx["c1_cs_idx"], fx["c3_cs_idx"]) and not np.array_equal(fx["c1_cs_dists"], fx["c3_cs_dists"])


def test_line_functions_match_the_fixture(fx):
    from mrcc_amd.utils import transformation as T

    lp1, lp2, pts = fx["line_lp1"], fx["line_lp2"], fx["line_points"]
    d = T.compute_dists_to_line(pts, lp1, lp2)
    assert d.dtype == np.float64 and np.abs(d - fx["line_dists"]).max() <= 1e-12
    assert np.abs(H.dists_to_line(pts, lp1, lp2) - fx["line_dists"]).max() <= 1e-12
    assert abs(T.compute_vec_dist_to_line(pts[0], lp1, lp2) - float(fx["line_vec_dist"])) <= 1e-12
    sd, si = T.select_closest_points_to_line(pts, lp1, lp2, count=5, cutoff=float(fx["line_cutoff"]))
    assert np.array_equal(si, fx["line_sel_idx"]) and np.abs(sd - fx["line_sel_dists"]).max() <= 1e-12
    assert len(si) == 3  # the cutoff cuts inside the first `count`
    ad, ai = T.select_closest_points_to_line(pts, lp1, lp2, cutoff=1.0)  # count 0: every point
    assert len(ai) == len(pts)
    assert np.array_equal(ai, fx["line_all_idx"]) and np.abs(ad - fx["line_all_dists"]).max() <= 1e-12
    assert np.all(np.diff(ad) >= 0)


def test_host_functions(fx):
    from mrcc_amd.utils import data as D

    points, pose = fx["c1_points"], fx["c1_pose"]
    q = H.ee_frame_crop(points, pose)
    assert np.array_equal(np.where(D.get_roi_mask(q, **D.EE_DIM))[0], fx["c1_ee_idx"])
    assert D.get_roi_mask(q, min_x=0.0, offset=0.01).sum() == (q[:, 0] > -0.01).sum()
    q[3, 1] = np.nan
    assert not D.get_roi_mask(q)[3]
    assert D.get_closest_point([0, 0, 0], q[:0]) is None
    sub = q[10:60]
    k, p, d = D.get_closest_point([0.0, 0.01, 0.1], sub, maximize_dim=2)
    target = np.array([0.0, 0.01, sub[:, 2].max()])
    assert k == np.argmin(np.linalg.norm(sub - target, axis=1)) and np.array_equal(p, sub[k])
    assert d == np.linalg.norm(sub[k] - target)
    k, _, d = D.get_closest_point([0.0, 0.0, 0.0], q[:50])  # numpy's argmin: a NaN distance wins at its first index
    assert k == 3 and np.isnan(d)


def test_n6_is_declared_exported_and_bound():
    import os

    import mrcc_amd

    lib = mrcc_amd._lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sv_hip.h")).read()
    for name in N6:
        assert name + "(" in header and name in mrcc_amd._lib.SIGNATURES and hasattr(lib, name), name


def test_entry_point_argument_checks_without_gpu():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    p = ctypes.create_string_buffer(64)  # stands in for a non-null pointer: every call here fails its checks first
    err = lambda: lib.sv_last_error()  # noqa: E731
    N, B = 1000, 3
    dbl = ctypes.c_double
    lp1, lp2 = (dbl * 3)(0.05, 0, 0), (dbl * 3)(-0.05, 0, 0)

    def mask(points=p, offsets=p, N=N, B=B, pos=p, rot=p, out=p):
        return lib.sv_ee_mask(points, 0, offsets, N, B, pos, rot, None, out, None)

    def kps(points=p, offsets=p, N=N, B=B, pos=p, rot=p, mode=10, ignore=-100, kp=p, idx=p):
        return lib.sv_key_points(points, 0, offsets, N, B, pos, rot, mode, dbl(0.018), ignore, kp, idx, None, None)

    need = lib.sv_line_topk_workspace_bytes(N)
    assert need >= N * 8 and lib.sv_line_topk_workspace_bytes(4 * N) > need

    def topk(points=p, offsets=p, N=N, B=B, pos=p, rot=p, a=lp1, b=lp2, count=32, ws=p, ws_bytes=need, idx=p, dist=p, n=p):
        return lib.sv_line_topk(points, 0, offsets, N, B, pos, rot, a, b, count, dbl(0.004), ws, ws_bytes, idx, dist, n,
                                None)

    def radius(points=p, offsets=p, N=N, B=B, kp_idx=p, K=10, ignore=-100, labels=p):
        return lib.sv_radius_labels(points, 0, offsets, N, B, kp_idx, K, dbl(0.006), ignore, labels, None)

    for fn in (mask, kps, topk, radius):
        for b in (0, -1, 1025):
            assert fn(B=b) == -1 and b"1 to 1024 frames" in err(), (fn.__name__, b)
        for n in (-1, 1 << 29):
            assert fn(N=n) == -1 and b"2^29 points" in err(), (fn.__name__, n)
        for kw in ({"points": None}, {"offsets": None}):
            assert fn(**kw) == -1 and b"null pointer" in err(), (fn.__name__, kw)
    for kw in ({"pos": None}, {"rot": None}, {"out": None}):
        assert mask(**kw) == -1 and b"null pointer" in err(), kw
    for kw in ({"pos": None}, {"rot": None}, {"kp": None}, {"idx": None}):
        assert kps(**kw) == -1 and b"null pointer" in err(), kw
    for mode in (0, 4, 7, 12):
        assert kps(mode=mode) == -1 and b"mode must be 10 or 6" in err(), mode
    for fn in (kps, radius):
        for ig in (0, 5):
            assert fn(ignore=ig) == -1 and b"ignore_label must be negative" in err(), (fn.__name__, ig)
    for kw in ({"pos": None}, {"rot": None}, {"a": None}, {"b": None}, {"ws": None}, {"idx": None}, {"dist": None}, {"n": None}):
        assert topk(**kw) == -1 and b"null pointer" in err(), kw
    for count in (0, -3, 1025):
        assert topk(count=count) == -1 and b"count must be in [1, 1024]" in err(), count
    assert topk(b=lp1) == -1 and b"distinct finite points" in err()
    assert topk(a=(dbl * 3)(float("nan"), 0, 0)) == -1 and b"distinct finite points" in err()
    for ws_bytes in (0, 256, N * 8 - 1):
        assert topk(ws_bytes=ws_bytes) == -2 and b"workspace too small" in err(), ws_bytes
    for kw in ({"kp_idx": None}, {"labels": None}):
        assert radius(**kw) == -1 and b"null pointer" in err(), kw
    for K in (0, -1, 65):
        assert radius(K=K) == -1 and b"K must be in [1, 64]" in err(), K


def test_python_entry_points_refuse_without_gpu():
    from mrcc_amd._lib import SvHipError
    from mrcc_amd.utils import augmentation as A
    from mrcc_amd.utils import data as D

    pose = np.array([[0, 0, 0, 1, 0, 0, 0]], dtype=np.float64)
    pts = torch.zeros(4, 3)
    with pytest.raises(SvHipError, match="no CPU fallback"):
        D.key_point_labels_batch(pts, [0, 4], pose)
    with pytest.raises(SvHipError, match="no CPU fallback"):
        D.vote_labels_batch(pts, [0, 4], pose, value=1)
    with pytest.raises(SvHipError, match="no CPU fallback"):
        D.ee_crop_batch([np.zeros((4, 3))], None, None, pose, device="cpu")
    with pytest.raises(SvHipError, match="no CPU fallback"):
        D.get_ee_idx(np.zeros((4, 3)), pose[0], device="cpu")
    with pytest.raises(ValueError, match="at most 1024"):
        D.get_ee_cross_section_idx(np.zeros((2000, 3)), pose[0], count=0)
    with pytest.raises(ValueError):
        D.ee_crop_batch([np.zeros((4, 2))], None, None, pose)
    with pytest.raises(ValueError):
        D.ee_crop_batch([], None, None, pose)
    with pytest.raises(ValueError, match='"10" or "6"'):
        D.key_point_labels_batch(pts, [0, 4], pose, generator="8")
    d, i = D.get_ee_cross_section_idx(np.zeros((0, 3)), pose[0])
    assert d.shape == (0,) and i.shape == (0,) and i.dtype == np.int64
    a, b = D.collect_closest_points([], np.zeros((4, 3), dtype=np.float32))
    assert a.shape == (0,) and b.shape == (0,)
    with pytest.raises(IndexError):
        D.collect_closest_points([4], np.zeros((4, 3), dtype=np.float32))
    with pytest.raises(SvHipError, match="CUDA tensor"):
        A.augment_quantize_batch(pts, pts, torch.zeros(4), quantization_size=0.01, point_offsets=[0, 4])
    with pytest.raises(SvHipError, match="no CPU fallback"):
        A.augment_quantize_batch(pts, pts, torch.zeros(4), quantization_size=0.01, point_offsets=[0, 4], device="cpu")
