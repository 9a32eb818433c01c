"""The PointNet++ sampling and grouping kernels (sv_fps, sv_fps_segmented, sv_ball_query[_multi], sv_three_nn,
sv_three_nn_gather, sv_three_nn_interpolate) against the float32 emulations of oracle/sv_oracle.py, bit for bit: the
library is built with -ffp-contract=off and every kernel states its operation order, so indices must be equal and
weights / values must have the emulation's bits (tests/test_oracle_points.py pins the emulations to float64).  Sizes sit
on the edges of the kernels: every farthest-point instance and its boundary + 1, one wave, the 64-point step of the ball
query and its 4-centre workgroup, the 256-point staging chunk and the 64- / 256-query workgroups of the 3-NN kernels.
Last: what an out-of-range group index (an empty ball's N) does in the fused set abstractions and sv_group_rows."""
from ctypes import c_int

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P2(gpu):
    from mrcc_amd.model import pointnet2_utils

    return pointnet2_utils


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _same_bits(got, want):
    """float32 arrays with the same bits; a NaN matches a NaN (np.array_equal(equal_nan=True) plus the sign of zero)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != np.float32 or want.dtype != np.float32 or got.shape != want.shape:
        return False
    ng, nw = np.isnan(got), np.isnan(want)
    return np.array_equal(ng, nw) and np.array_equal(got.view(np.uint32)[~ng], want.view(np.uint32)[~nw])


# ----------------------------------------------------------------------------------------------------------------------
# farthest-point sampling.  launch_fps: fps_reg_kernel<4> N <= 4096, <8> <= 8192, <16> with the cloud in LDS <= 12800,
# <16> from global memory <= 16384, fps_kernel <= 38400.  Thread t owns points t, t + 1024, ...
# ----------------------------------------------------------------------------------------------------------------------
def _fps(P2, gpu, xyz, S, start):
    got = P2.farthest_point_sample(_dev(xyz, gpu), S, start=_dev(np.asarray(start, dtype=np.int64), gpu))
    return got.cpu().numpy()


def _fps_oracle(oracle, xyz, S, start):
    with np.errstate(invalid="ignore"):  # inf - inf of a non-finite point
        return oracle.farthest_point_sample(xyz, S, np.asarray(start, dtype=np.int64))


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 1023, 1024, 1025, 4096, 4097, 8192, 8193, 12800, 12801, 16384, 16385,
                               38400])
def test_fps_matches_oracle_at_instance_and_wave_edges(gpu, oracle, P2, N):
    """three distinct clouds per size, starts at both ends and inside; up to 65 points S = N + 3 > N (every point is
    taken, then index 0 repeats)"""
    S = N + 3 if N <= 65 else 48
    xyz = np.random.default_rng(N).uniform(-1, 1, size=(3, N, 3)).astype(np.float32)
    start = [0, N - 1, N // 3]
    want = _fps_oracle(oracle, xyz, S, start)
    if N <= 65:
        assert all(sorted(want[b, :N]) == list(range(N)) for b in range(3)) and (want[:, N:] == 0).all()
    assert np.array_equal(_fps(P2, gpu, xyz, S, start), want)


@pytest.mark.parametrize("N", [4096, 8192, 12800, 16384, 38400])
def test_fps_tie_between_far_twins_goes_to_the_lower_index(gpu, oracle, P2, N):
    """a tight cluster and two exact copies of one far point: the first argmax is a tie between the copies.  One cloud
    per ownership pattern: neighbouring lanes (i, i + 1), two waves (i, i + 64), one thread (i, i + 1024), and a pair
    whose lower index sits in the higher wave (700 in wave 10, 1029 in wave 0)."""
    pairs = [(700, 701), (700, 764), (700, 1724), (700, 1029)]
    rng = np.random.default_rng(N + 1)
    xyz = rng.uniform(-0.01, 0.01, size=(len(pairs), N, 3)).astype(np.float32)
    for b, (i, j) in enumerate(pairs):
        xyz[b, i] = xyz[b, j] = (5.0, -3.0, 2.0)
    start = [10, N - 1, N // 3, 2000]
    want = _fps_oracle(oracle, xyz, 8, start)
    assert (want[:, 1] == 700).all() and all((want[b] != j).all() for b, (_, j) in enumerate(pairs))
    assert np.array_equal(_fps(P2, gpu, xyz, 8, start), want)


@pytest.mark.parametrize("N", [2000, 17000])
def test_fps_all_identical_cloud_picks_index_0(gpu, oracle, P2, N):
    xyz = np.broadcast_to(np.array([0.25, -1.5, 3.0], dtype=np.float32), (3, N, 3)).copy()
    start = [0, N - 1, N // 3]
    got = _fps(P2, gpu, xyz, 10, start)
    assert np.array_equal(got[:, 0], start) and (got[:, 1:] == 0).all()
    assert np.array_equal(got, _fps_oracle(oracle, xyz, 10, start))


@pytest.mark.parametrize("N", [3000, 17000])
def test_fps_nan_and_inf_points(gpu, oracle, P2, N):
    """a point with a NaN or an infinite coordinate never gets a distance below the initial 1e10: it is the next pick
    and then stays the pick (register-resident and LDS instance)"""
    xyz = np.random.default_rng(N).uniform(-1, 1, size=(3, N, 3)).astype(np.float32)
    xyz[0, 1234, 1] = np.nan
    xyz[1, 77, 0] = np.inf
    xyz[2, 2100, 2] = -np.inf
    xyz[2, 2900, 0] = np.nan
    start = [0, N - 1, N // 3]
    want = _fps_oracle(oracle, xyz, 16, start)
    assert (want[0, 1:] == 1234).all() and (want[1, 1:] == 77).all() and (want[2, 1:] == 2100).all()
    assert np.array_equal(_fps(P2, gpu, xyz, 16, start), want)


@pytest.mark.parametrize("N", [700, 17000])
def test_fps_start_is_clamped_into_the_cloud(gpu, oracle, P2, N):
    xyz = np.random.default_rng(N + 2).uniform(-1, 1, size=(2, N, 3)).astype(np.float32)
    want = _fps_oracle(oracle, xyz, 32, [0, N - 1])
    assert np.array_equal(_fps(P2, gpu, xyz, 32, [-5, N + 7]), want)


def test_fps_segmented_matches_oracle_per_cloud(gpu, oracle):
    """G = 6 clouds (one empty, one of a single point) in one launch against the oracle on each cloud alone; then with
    max_n below the longest clouds, which are read as their first max_n points"""
    from mrcc_amd._lib import call, ptr, stream_ptr

    sizes, K = [300, 0, 1, 9000, 12800, 2048], 64
    rng = np.random.default_rng(5)
    clouds = [rng.uniform(-1, 1, size=(n, 3)).astype(np.float32) for n in sizes]
    clouds[5][1000:1040] = clouds[5][:40]  # exact duplicates: ties
    starts = [299, 0, 0, 4500, 17, 2047]
    xyz = _dev(np.concatenate(clouds), gpu)
    offs = _dev(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), gpu)
    ooffs = _dev(np.arange(len(sizes) + 1, dtype=np.int64) * K, gpu)
    st = _dev(np.asarray(starts, dtype=np.int64), gpu)
    for max_n in (12800, 8192):
        out = torch.full((len(sizes) * K,), -7, dtype=torch.int64, device=gpu)
        call("sv_fps_segmented", ptr(xyz), ptr(offs), ptr(ooffs), ptr(st), c_int(len(sizes)), c_int(max_n), ptr(out),
             stream_ptr())
        got = out.cpu().numpy().reshape(len(sizes), K)
        for g, (c, s) in enumerate(zip(clouds, starts)):
            want = _fps_oracle(oracle, c[None, :max_n], K, [s])[0] if len(c) else np.zeros(K, dtype=np.int64)
            assert np.array_equal(got[g], want), (max_n, g)


# ----------------------------------------------------------------------------------------------------------------------
# ball query: one wave per centre, 64 points per step, 4 centres per workgroup
# ----------------------------------------------------------------------------------------------------------------------
def _bq_oracle(oracle, radius, nsample, xyz, new_xyz):
    with np.errstate(invalid="ignore", over="ignore"):
        return oracle.query_ball_point(radius, nsample, xyz, new_xyz)


def _bq(P2, gpu, radius, nsample, xyz, new_xyz):
    return P2.query_ball_point(radius, nsample, _dev(xyz, gpu), _dev(new_xyz, gpu)).cpu().numpy()


def _random_case(N, B, S, seed=0):
    rng = np.random.default_rng(1000 * N + 10 * S + B + seed)
    xyz = rng.uniform(-1, 1, size=(B, N, 3)).astype(np.float32)
    new_xyz = np.stack([xyz[b, rng.integers(0, N, size=S)] for b in range(B)])
    return xyz, new_xyz


def _half_foreign_case():
    """N = 1000, (B, S) = (2, 64): every other centre is not a cloud point, so small balls are empty"""
    xyz, new_xyz = _random_case(1000, 2, 64, seed=1)
    new_xyz[:, 1::2] = np.random.default_rng(3).uniform(-1, 1, size=(2, 32, 3)).astype(np.float32)
    return xyz, new_xyz


def _empty_case():
    """N = 127, six centres: far ones (empty balls at any radius used here) mixed with cloud points inside the first
    workgroup of four, two far ones in the second, whose other two waves have no centre"""
    xyz, new_xyz = _random_case(127, 1, 6)
    new_xyz[0, [1, 4, 5]] = [[40, 0, 0], [0, -40, 0], [30, 30, 30]]
    return xyz, new_xyz


def _nonfinite_case():
    """a NaN and an infinite point in the cloud, a NaN centre among finite ones"""
    xyz, new_xyz = _random_case(129, 3, 5)
    xyz[0, 70, 1] = np.nan
    xyz[1, 3, 0] = np.inf
    xyz[2, 128, 2] = -np.inf
    xyz[2, 64, 0] = np.nan
    new_xyz[:, 2, 1] = np.nan
    return xyz, new_xyz


SPHERE = np.array([[.5, 0, 0], [-.5, 0, 0], [0, .5, 0], [0, -.5, 0], [0, 0, .5], [0, 0, -.5]], dtype=np.float32)
SPHERE_AT = [3, 40, 63, 64, 100, 128]  # both 64-point steps and the one-point tail step
R_BELOW = 0.4999999850988386  # (float)(r * r) is the float32 just below 0.25
R_NEXT = float(np.nextafter(0.5, 0))  # (float)(r * r) rounds to 0.25f


def _sphere_case():
    """coordinates on the 1/8 grid (every expanded distance is exact in float32), centre 0 of each cloud with six points
    exactly 0.5 away along the axes"""
    rng = np.random.default_rng(9)
    xyz = (rng.integers(-16, 17, size=(3, 129, 3)) / 8).astype(np.float32)
    new_xyz = (rng.integers(-12, 13, size=(3, 5, 3)) / 8).astype(np.float32)
    for b in range(3):
        xyz[b, SPHERE_AT] = new_xyz[b, 0] + SPHERE
    return xyz, new_xyz


@pytest.mark.parametrize("N,B,S,nsample,radius", [
    (1, 1, 1, 1, 0.5), (1, 3, 5, 16, 0.5), (63, 3, 5, 64, 4.0), (64, 2, 64, 65, 4.0), (64, 1, 1, 64, 4.0),
    (65, 1, 1, 128, 4.0), (65, 3, 5, 16, 0.6), (127, 3, 5, 200, 0.5), (127, 1, 1, 65, 0.9), (129, 2, 64, 16, 0.5),
    (129, 3, 5, 1, 0.5), (1000, 3, 5, 64, 0.4), (1000, 2, 64, 65, 0.6), (1000, 1, 1, 200, 0.7), (1000, 3, 5, 128, 0.25),
])
def test_ball_query_matches_oracle_across_sizes(gpu, oracle, P2, N, B, S, nsample, radius):
    """N around the 64-point step, B * S = 1, 15 (tail waves return early) and 128, nsample up to 200 > 64 (the padding
    loop strides) and > N; radius 4 covers the cloud (the ball holds all N points)"""
    xyz, new_xyz = _random_case(N, B, S)
    want = _bq_oracle(oracle, radius, nsample, xyz, new_xyz)
    if radius == 4.0:
        assert (want[..., :min(N, nsample)] == np.arange(min(N, nsample))).all() and (want[..., N:] == 0).all()
    assert np.array_equal(_bq(P2, gpu, radius, nsample, xyz, new_xyz), want)


@pytest.mark.parametrize("nsample", [16, 40])
def test_ball_query_ball_fills_inside_a_step(gpu, oracle, P2, nsample):
    """dense clusters: more than nsample hits inside points 0..50 (the ball fills in the middle of the first 64-point
    step) and inside points 100..160 (in the middle of the second and third)"""
    rng = np.random.default_rng(21)
    xyz = rng.uniform(-1, 1, size=(1, 300, 3)).astype(np.float32)
    ca, cb = np.array([0.5, 0.5, 0.5], np.float32), np.array([-0.5, 0.25, -0.5], np.float32)
    xyz[0, :51] = ca + rng.uniform(-0.01, 0.01, size=(51, 3)).astype(np.float32)
    xyz[0, 100:161] = cb + rng.uniform(-0.01, 0.01, size=(61, 3)).astype(np.float32)
    new_xyz = np.stack([ca, cb, xyz[0, 200], xyz[0, 20], xyz[0, 130]])[None]
    want = _bq_oracle(oracle, 0.05, nsample, xyz, new_xyz)
    assert (want[0, 0] == np.arange(nsample)).all() and (want[0, 1] == 100 + np.arange(nsample)).all()
    assert np.array_equal(_bq(P2, gpu, 0.05, nsample, xyz, new_xyz), want)


def test_ball_query_points_on_the_sphere(gpu, oracle, P2):
    """d == r^2 exactly: a hit (`not d > r^2`); the radius whose float32 square is the float below 0.25 misses them, the
    double just below 0.5, whose square rounds to 0.25f, hits them"""
    xyz, new_xyz = _sphere_case()
    every = np.broadcast_to(np.asarray(SPHERE_AT), (3, 5, 6))
    assert (oracle.three_nn_distances(new_xyz, xyz, every)[:, 0] == np.float32(0.25)).all()
    assert np.float32(R_BELOW * R_BELOW) == np.nextafter(np.float32(0.25), np.float32(0))
    assert R_NEXT < 0.5 and np.float32(R_NEXT * R_NEXT) == np.float32(0.25)
    for radius, hit in ((0.5, True), (R_BELOW, False), (R_NEXT, True)):
        want = _bq_oracle(oracle, radius, 129, xyz, new_xyz)
        for b in range(3):
            assert np.isin(SPHERE_AT, want[b, 0]).all() if hit else not np.isin(SPHERE_AT, want[b, 0]).any()
        assert np.array_equal(_bq(P2, gpu, radius, 129, xyz, new_xyz), want), radius


@pytest.mark.parametrize("nsample", [16, 65])
def test_ball_query_empty_balls_hold_the_index_N(gpu, oracle, P2, nsample):
    xyz, new_xyz = _empty_case()
    got = _bq(P2, gpu, 0.4, nsample, xyz, new_xyz)
    assert (got[0, [1, 4, 5]] == 127).all() and (got[0, [0, 2, 3]] < 127).all()
    assert np.array_equal(got, _bq_oracle(oracle, 0.4, nsample, xyz, new_xyz))


@pytest.mark.parametrize("nsample", [16, 200])
def test_ball_query_nan_centre_nan_and_inf_points(gpu, oracle, P2, nsample):
    """a NaN distance is a hit (`not d > r^2`): a NaN centre takes the points 0 .. nsample - 1, a NaN point is in every
    ball it is scanned for; an infinite point is what the arithmetic makes of it"""
    xyz, new_xyz = _nonfinite_case()
    want = _bq_oracle(oracle, 0.5, nsample, xyz, new_xyz)
    k = min(nsample, 129)
    assert (want[:, 2, :k] == np.arange(k)).all() and (want[:, 2, k:] == 0).all()
    assert (want[0] == 70).any(axis=-1).sum() >= 2  # the NaN point is in other centres' balls too
    assert np.array_equal(_bq(P2, gpu, 0.5, nsample, xyz, new_xyz), want)


MULTI_INPUTS = {"random": lambda: _random_case(1000, 2, 64), "foreign": _half_foreign_case, "empty": _empty_case,
                "nonfinite": _nonfinite_case, "sphere": _sphere_case, "one": lambda: _random_case(65, 1, 1)}


@pytest.mark.parametrize("inputs", sorted(MULTI_INPUTS))
def test_ball_query_multi_matches_oracle_per_radius(gpu, oracle, P2, inputs):
    """R = 1 .. 4 radii in one scan, each output against the oracle for its (radius, nsample): unsorted radii, two equal
    radii with different nsample, a radius that leaves some balls empty, the on-sphere radii"""
    xyz, new_xyz = MULTI_INPUTS[inputs]()
    N = xyz.shape[1]
    x, q = _dev(xyz, gpu), _dev(new_xyz, gpu)
    empties = 0
    for radii, ns in (([0.4], [16]), ([0.3, 0.3], [16, 65]), ([0.6, 0.1, 0.3], [64, 16, 128]),
                      ([0.5, 0.1, 0.8, 0.2], [200, 1, 64, 65]), ([R_NEXT, 0.5, R_BELOW], [129, 16, 129])):
        got = P2.query_ball_point_multi(radii, ns, x, q)
        assert len(got) == len(radii)
        for radius, k, o in zip(radii, ns, got):
            want = _bq_oracle(oracle, radius, k, xyz, new_xyz)
            assert np.array_equal(o.cpu().numpy(), want), (radii, radius, k)
            empties += int((want[..., 0] == N).sum())
            if radius == 0.1 and inputs == "foreign":  # some balls empty, some not
                assert (want[..., 0] == N).any() and (want[:, 1::2, 0] != N).any()
    if inputs in ("foreign", "empty"):
        assert empties > 0


# ----------------------------------------------------------------------------------------------------------------------
# 3-NN: sv_three_nn (256 queries a workgroup), sv_three_nn_interpolate (64 queries a workgroup), sources staged through
# LDS 256 at a time; sv_three_nn_gather
# ----------------------------------------------------------------------------------------------------------------------
def _check_three_nn(P2, oracle, gpu, xyz1, xyz2, pts2):
    """all three entries against the oracle, bit for bit; returns the oracle's (idx, w, out)"""
    want_idx, want_w = oracle.three_nn(xyz1, xyz2)
    want_out = oracle.three_nn_gather(pts2, want_idx, want_w)
    x1, x2, p2 = _dev(xyz1, gpu), _dev(xyz2, gpu), _dev(pts2, gpu)
    idx, w = P2.three_nn(x1, x2)
    assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), want_idx)
    assert _same_bits(w.cpu().numpy(), want_w)
    assert _same_bits(P2.three_nn_interpolate(x1, x2, p2).cpu().numpy(), want_out)
    assert _same_bits(P2.three_nn_gather(p2, idx, w).cpu().numpy(), want_out)
    return want_idx, want_w, want_out


@pytest.mark.parametrize("B,N,S,C", [(1, 1, 3, 1), (3, 63, 4, 5), (1, 64, 255, 33), (3, 65, 256, 257), (1, 255, 257, 5),
                                     (3, 256, 512, 1), (1, 257, 513, 33)])
def test_three_nn_matches_oracle_across_sizes(gpu, oracle, P2, B, N, S, C):
    rng = np.random.default_rng(100 * N + S)
    xyz1 = rng.uniform(-0.5, 0.5, size=(B, N, 3)).astype(np.float32)
    xyz2 = rng.uniform(-0.5, 0.5, size=(B, S, 3)).astype(np.float32)
    pts2 = rng.standard_normal((B, S, C)).astype(np.float32)
    _check_three_nn(P2, oracle, gpu, xyz1, xyz2, pts2)


def test_three_nn_ties_go_to_the_lower_index(gpu, oracle, P2):
    """exact duplicate sources at (10, 11), at (255, 256) across the staging chunk, and four copies of one point at 40, 90,
    200 and 290; the queries are the sources themselves (exact ties at distance 0) and jittered copies (ties at a
    distance above 0)"""
    rng = np.random.default_rng(31)
    S = 300
    xyz2 = rng.uniform(-0.5, 0.5, size=(2, S, 3)).astype(np.float32)
    xyz2[:, 11] = xyz2[:, 10]
    xyz2[:, 256] = xyz2[:, 255]
    xyz2[:, [90, 200, 290]] = xyz2[:, 40:41]
    jitter = rng.uniform(-1e-3, 1e-3, size=(2, S, 3)).astype(np.float32)
    xyz1 = np.concatenate([xyz2, xyz2 + jitter], axis=1)
    pts2 = rng.standard_normal((2, S, 5)).astype(np.float32)
    idx, _, _ = _check_three_nn(P2, oracle, gpu, xyz1, xyz2, pts2)
    for q in (0, S):  # exact and jittered queries
        assert (idx[:, q + 10, :2] == [10, 11]).all() and (idx[:, q + 11, :2] == [10, 11]).all()
        assert (idx[:, q + 255, :2] == [255, 256]).all() and (idx[:, q + 256, :2] == [255, 256]).all()
        for c in (40, 90, 200, 290):
            assert (idx[:, q + c] == [40, 90, 200]).all()


def test_three_nn_query_coinciding_with_a_source(gpu, oracle, P2):
    """feature propagation interpolates onto a superset of the source cloud: the expanded distance of a point to itself
    is exactly 0, that source comes first and takes (almost) all the weight"""
    rng = np.random.default_rng(32)
    S, N = 257, 300
    xyz2 = rng.uniform(-0.5, 0.5, size=(3, S, 3)).astype(np.float32)
    xyz1 = np.concatenate([xyz2, rng.uniform(-0.5, 0.5, size=(3, N - S, 3)).astype(np.float32)], axis=1)
    pts2 = rng.standard_normal((3, S, 33)).astype(np.float32)
    idx, w, _ = _check_three_nn(P2, oracle, gpu, xyz1, xyz2, pts2)
    assert (idx[:, :S, 0] == np.arange(S)).all()
    assert (oracle.three_nn_distances(xyz1, xyz2, idx)[:, :S, 0] == 0).all()
    assert (w[:, :S, 0] > 0.999).all()


def test_three_nn_negative_expanded_distances(gpu, oracle, P2):
    """queries one float32 step away from a source in [1, 2)^3: the expanded form cancels to a negative distance for many
    of the pairs and the weights go negative, as the reference formula's do - the kernels must give the emulation's bits"""
    rng = np.random.default_rng(33)
    S = 300
    xyz2 = rng.uniform(1, 2, size=(1, S, 3)).astype(np.float32)
    toward = np.where(rng.random((1, 2 * S, 3)) < 0.5, np.float32(0), np.float32(3))
    xyz1 = np.nextafter(np.concatenate([xyz2, xyz2], axis=1), toward).astype(np.float32)
    pts2 = rng.standard_normal((1, S, 5)).astype(np.float32)
    idx, w, out = _check_three_nn(P2, oracle, gpu, xyz1, xyz2, pts2)
    d = oracle.three_nn_distances(xyz1, xyz2, idx)
    negative = int((d[..., 0] < 0).sum())
    print(f"{negative} of {2 * S} nearest expanded distances are negative")
    assert negative >= 2 * S // 10 and (w < 0).any() and np.isfinite(out).all()


def test_three_nn_nan_sources_and_a_nan_query(gpu, oracle, P2):
    """NaN source rows (in both staging chunks, first and last index included) are never selected; a NaN query has
    indices 0 and NaN weights and values in its own row, every other row keeps the bits of the run without it"""
    rng = np.random.default_rng(34)
    S, N = 300, 130
    nan_rows = [0, 5, 255, 256, 299]
    xyz2 = rng.uniform(-0.5, 0.5, size=(2, S, 3)).astype(np.float32)
    xyz2[:, nan_rows, 1] = np.nan
    xyz1 = rng.uniform(-0.5, 0.5, size=(2, N, 3)).astype(np.float32)
    pts2 = rng.standard_normal((2, S, 5)).astype(np.float32)
    idx0, w0, out0 = _check_three_nn(P2, oracle, gpu, xyz1, xyz2, pts2)
    assert not np.isin(idx0, nan_rows).any() and np.isfinite(w0).all()
    xyz1n = xyz1.copy()
    xyz1n[:, 64, 2] = np.nan
    idx, w, out = _check_three_nn(P2, oracle, gpu, xyz1n, xyz2, pts2)
    assert (idx[:, 64] == 0).all() and np.isnan(w[:, 64]).all() and np.isnan(out[:, 64]).all()
    rest = np.arange(N) != 64
    assert np.array_equal(idx[:, rest], idx0[:, rest])
    assert _same_bits(w[:, rest], w0[:, rest]) and _same_bits(out[:, rest], out0[:, rest])
    # fewer than three finite sources: the unfilled slots keep index 0 and distance +inf (weight 0)
    few = xyz2[:, :8].copy()  # rows 0 and 5 are NaN already
    few[:, 3:, 0] = np.nan
    idx, w, _ = _check_three_nn(P2, oracle, gpu, xyz1, few, pts2[:, :8])
    assert (np.sort(idx[..., :2], axis=-1) == [1, 2]).all() and (idx[..., 2] == 0).all() and (w[..., 2] == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# an out-of-range group index (sv_ball_query's N for an empty ball) reads nothing: a NaN row in sv_group_rows and in the
# fused set abstractions alike, so that centroid's pooled output is NaN and no other centroid changes
# ----------------------------------------------------------------------------------------------------------------------
def _randomize(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / m.weight[0].numel() ** 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            elif isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.weight.copy_(torch.rand(n, generator=g) * 0.5 + 0.75)
                m.bias.copy_(torch.randn(n, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(n, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(n, generator=g) * 0.5 + 0.75)


def _foreign_centroid(P2, gpu, B=2, N=200, S=7, D=3, at=(1, 2)):
    """cloud, features, centroids from sv_fps, and the same centroids with one replaced by a far foreign point"""
    g = torch.Generator().manual_seed(40)
    xyz = (torch.rand(B, N, 3, generator=g) - 0.5).to(gpu)
    pts = torch.randn(B, N, D, generator=g).to(gpu) if D else None
    new_xyz = P2.index_points(xyz, P2.farthest_point_sample(xyz, S, start=torch.zeros(B, dtype=torch.long)))
    far = new_xyz.clone()
    far[at[0], at[1]] = torch.tensor([50.0, -50.0, 50.0], device=gpu)
    return xyz, pts, new_xyz.contiguous(), far.contiguous()


def _only_row_is_nan(got, base, at):
    """got [B, S, ...]: NaN everywhere in the row `at`, the bits of `base` in every other row"""
    keep = torch.ones(got.shape[:2], dtype=torch.bool, device=got.device)
    keep[at] = False
    return bool(torch.isnan(got[at]).all()) and not bool(torch.isnan(base).any()) and torch.equal(got[keep], base[keep])


@pytest.mark.parametrize("nsample", [16, 32, 64])
def test_fused_set_abstraction_empty_ball_gives_a_nan_centroid(gpu, P2, nsample):
    at, N = (1, 2), 200
    xyz, pts, new_xyz, far = _foreign_centroid(P2, gpu, N=N, at=at)
    sa = P2.PointNetSetAbstraction(7, 0.3, nsample, 6, [32, 48], False)
    _randomize(sa, 41)
    sa = sa.to(gpu).eval()
    idx = P2.query_ball_point(0.3, nsample, xyz, new_xyz)
    idx_far = P2.query_ball_point(0.3, nsample, xyz, far)
    assert (idx_far[at] == N).all() and (idx < N).all() and torch.equal(idx_far[0], idx[0])
    with torch.no_grad():
        base = sa._fused(xyz, pts, new_xyz, idx, sa._folded())
        got = sa._fused(xyz, pts, far, idx_far, sa._folded())
    assert base is not None and got is not None  # the fused kernel ran
    assert _only_row_is_nan(got, base, at)
    # a single out-of-range entry (below 0 or >= N) in an otherwise full group does the same
    for bad in (-1, N, N + 5):
        one = idx.clone()
        one[0, 5, nsample // 2] = bad
        with torch.no_grad():
            assert _only_row_is_nan(sa._fused(xyz, pts, new_xyz, one, sa._folded()), base, (0, 5))


@pytest.mark.parametrize("D", [0, 3])
def test_fused_msg_set_abstraction_empty_ball_gives_a_nan_centroid(gpu, P2, D):
    at, N = (1, 2), 200
    xyz, pts, new_xyz, far = _foreign_centroid(P2, gpu, N=N, D=D, at=at)
    radii, ns, mlps = [0.2, 0.3, 0.5], [16, 32, 128], [[32, 48], [16, 32], [32, 32]]
    sa = P2.PointNetSetAbstractionMsg(7, radii, ns, D, mlps)
    _randomize(sa, 42)
    sa = sa.to(gpu).eval()
    idxs = P2.query_ball_point_multi(radii, ns, xyz, new_xyz)
    idxs_far = P2.query_ball_point_multi(radii, ns, xyz, far)
    assert all((f[at] == N).all() and (i < N).all() for i, f in zip(idxs, idxs_far))
    with torch.no_grad():
        base = sa._fused(xyz, pts, new_xyz, idxs, sa._folded())
        got = sa._fused(xyz, pts, far, idxs_far, sa._folded())
    assert base is not None and got is not None
    assert _only_row_is_nan(got, base, at)
    # one scale's ball empty: that scale's columns of the centroid are NaN, everything else keeps its bits
    for r, (c0, c1) in enumerate(((0, 48), (48, 80), (80, 112))):
        one = [t.clone() for t in idxs]
        one[r][0, 5] = N
        with torch.no_grad():
            got = sa._fused(xyz, pts, new_xyz, one, sa._folded())
        assert torch.isnan(got[0, 5, c0:c1]).all()
        got[0, 5, c0:c1] = base[0, 5, c0:c1]
        assert torch.equal(got, base), r


@pytest.mark.parametrize("order,D", [(0, 3), (1, 3), (0, 0)])
def test_group_rows_empty_ball_gives_nan_rows(gpu, P2, order, D):
    at, N, K = (1, 2), 200, 16
    xyz, pts, new_xyz, far = _foreign_centroid(P2, gpu, N=N, D=D, at=at)
    idx = P2.query_ball_point(0.3, K, xyz, new_xyz)
    idx_far = P2.query_ball_point(0.3, K, xyz, far)
    assert (idx_far[at] == N).all()
    base = P2.group_rows(xyz, pts, new_xyz, idx, order)
    got = P2.group_rows(xyz, pts, far, idx_far, order)
    assert _only_row_is_nan(got.view(2, 7, K, 3 + D), base.view(2, 7, K, 3 + D), at)
    assert _only_row_is_nan(P2.group_max(got, K).view(2, 7, 3 + D), P2.group_max(base, K).view(2, 7, 3 + D), at)
