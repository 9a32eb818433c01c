"""Argument checks of the pose solves (sv_kabsch_batched, sv_quat_avg_batched, sv_add_metric_batched,
sv_icp_point2point) and of their Python wrappers: host code only, nothing reaches a device, no GPU needed.

The wrappers check counts and shapes before any tensor is moved to the device, so a bad count can never make a kernel
read past its problem.  To keep that true even if a check went missing, the library call is replaced by one that fails
the test."""
import ctypes

import numpy as np
import pytest

NAN = float("nan")


def _buf(n):
    """A host buffer standing in for a non-null pointer (never dereferenced: every call here fails its checks)."""
    return ctypes.create_string_buffer(n)


def test_kabsch_argument_checks_without_gpu():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    p = _buf(64)
    # (ref, tgt, K, Kmax, B, R, t, q, stream)
    rc = lib.sv_kabsch_batched(p, p, None, 6, -1, p, p, p, None)
    assert rc == -1 and b"bad shape" in lib.sv_last_error()
    rc = lib.sv_kabsch_batched(p, p, None, 0, 1, p, p, p, None)
    assert rc == -1 and b"bad shape" in lib.sv_last_error()
    assert lib.sv_kabsch_batched(None, None, None, 6, 0, None, None, None, None) == 0  # B = 0: nothing to do
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        ref, tgt, R, t = args
        rc = lib.sv_kabsch_batched(ref, tgt, None, 6, 1, R, t, None, None)
        assert rc == -1 and b"null pointer" in lib.sv_last_error()


def test_quat_avg_argument_checks_without_gpu():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    p = _buf(64)
    # (Q, w, M, Mmax, B, out, stream)
    rc = lib.sv_quat_avg_batched(p, p, None, 4, -1, p, None)
    assert rc == -1 and b"bad shape" in lib.sv_last_error()
    rc = lib.sv_quat_avg_batched(p, p, None, 0, 1, p, None)
    assert rc == -1 and b"bad shape" in lib.sv_last_error()
    assert lib.sv_quat_avg_batched(None, None, None, 4, 0, None, None) == 0
    for Q, out in ((None, p), (p, None)):
        rc = lib.sv_quat_avg_batched(Q, None, None, 4, 1, out, None)
        assert rc == -1 and b"null pointer" in lib.sv_last_error()


def test_add_metric_argument_checks_without_gpu():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    p = _buf(64)
    # (points, P, Pmax, gt, pred, B, out, stream)
    rc = lib.sv_add_metric_batched(p, None, 10, p, p, -1, p, None)
    assert rc == -1 and b"bad shape" in lib.sv_last_error()
    rc = lib.sv_add_metric_batched(p, None, 0, p, p, 1, p, None)
    assert rc == -1 and b"bad shape" in lib.sv_last_error()
    assert lib.sv_add_metric_batched(None, None, 10, None, None, 0, None, None) == 0
    for pts, gt, pr, out in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        rc = lib.sv_add_metric_batched(pts, None, 10, gt, pr, 1, out, None)
        assert rc == -1 and b"null pointer" in lib.sv_last_error()


def test_icp_argument_checks_without_gpu():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    p = _buf(64)
    S, T = 100, 50
    need = lib.sv_icp_workspace_bytes(S)
    assert need >= S * 8

    def icp(S=S, T=T, max_distance=0.1, max_iterations=30, src=p, tgt=p, ws=p, ws_bytes=need, out_T=p):
        # (src, S, tgt, T, init_T, max_distance, max_iterations, rel_fitness, rel_rmse, ws, ws_bytes, out_T, stats, stream)
        return lib.sv_icp_point2point(src, S, tgt, T, None, max_distance, max_iterations, 1e-6, 1e-6, ws, ws_bytes, out_T,
                                      None, None)

    for kw in ({"S": 2}, {"S": 0}, {"T": 0}, {"S": 1 << 24}, {"T": 1 << 24}):
        assert icp(**kw) == -1 and b"at least 3 source points" in lib.sv_last_error(), kw
    for kw in ({"max_distance": 0.0}, {"max_distance": -0.1}, {"max_distance": NAN}, {"max_iterations": -1}):
        assert icp(**kw) == -1 and b"bad parameters" in lib.sv_last_error(), kw
    for kw in ({"src": None}, {"tgt": None}, {"ws": None}, {"out_T": None}):
        assert icp(**kw) == -1 and b"null pointer" in lib.sv_last_error(), kw
    # a workspace without room for the two per-point arrays: SV_ERR_WORKSPACE before anything is launched
    for ws_bytes in (0, 256, 256 + S * 4):
        assert icp(ws_bytes=ws_bytes) == -2 and b"workspace too small" in lib.sv_last_error(), ws_bytes


@pytest.fixture
def no_launch(monkeypatch):
    """Replace the library call of the three wrappers: reaching it means a bad argument got past the checks."""
    from mrcc_amd.utils import calibration, metrics, transformation

    def fail(name, *args):
        raise AssertionError(f"{name} was called with arguments the wrapper should have rejected")

    for mod in (calibration, metrics, transformation):
        monkeypatch.setattr(mod, "call", fail)


def test_kabsch_wrapper_rejects_bad_shapes_and_counts(no_launch):
    from mrcc_amd.utils import transformation as T

    a = np.zeros((3, 6, 3))
    for K in ([0, 6, 6], [3, 7, 6], [-1, 3, 3], [3, 3], [[3, 3, 3]]):
        with pytest.raises(ValueError, match="K"):
            T.get_rigid_transform_3D_batched(a, a, K, device="cuda")
    for ref, tgt in ((a, a[:, :5]), (a[0], a[0]), (a[..., :2], a[..., :2]), (np.zeros((3, 0, 3)), np.zeros((3, 0, 3)))):
        with pytest.raises(ValueError):
            T.get_rigid_transform_3D_batched(ref, tgt, device="cuda")
    with pytest.raises(ValueError):  # the reference's single-problem API: 2 x N is not N x 3
        T.get_rigid_transform_3D(np.zeros((2, 5)), np.zeros((2, 5)))


def test_quaternion_average_wrapper_rejects_bad_shapes_and_counts(no_launch):
    from mrcc_amd.utils import calibration as C

    Q = np.zeros((2, 5, 4))
    w = np.ones((2, 5))
    for M in ([0, 5], [1, 6], [-3, 2], [5], [5, 5, 5]):
        with pytest.raises(ValueError, match="M"):
            C.compute_quaternions_weighted_average_batched(Q, w, M, device="cuda")
    for bad_w in (np.ones((2, 4)), np.ones((2, 6)), np.ones(5), np.ones((1, 5))):
        with pytest.raises(ValueError, match="w must"):
            C.compute_quaternions_weighted_average_batched(Q, bad_w, device="cuda")
    for bad_Q in (np.zeros((2, 5, 3)), np.zeros((5, 4)), np.zeros((2, 0, 4))):
        with pytest.raises(ValueError, match="Q must"):
            C.compute_quaternions_weighted_average_batched(bad_Q, None, device="cuda")
    with pytest.raises(ValueError):  # one weight per quaternion in the single-problem API too
        C.compute_quaternions_weighted_average(np.zeros((5, 4)), np.ones(4))


def test_add_wrapper_rejects_bad_shapes_and_counts(no_launch):
    from mrcc_amd.utils import metrics as Mt

    pts = np.zeros((3, 10, 3))
    pose = np.zeros((3, 7))
    for P in ([0, 10, 10], [1, 11, 10], [-1, 1, 1], [10, 10], [[10, 10, 10]]):
        with pytest.raises(ValueError, match="P"):
            Mt.compute_ADD_batched(pts, P, pose, pose, device="cuda")
    for gt, pred in ((pose[:2], pose), (pose, pose[:, :6]), (pose[0], pose[0]), (pose, np.zeros((3, 8)))):
        with pytest.raises(ValueError, match="pose"):
            Mt.compute_ADD_batched(pts, None, gt, pred, device="cuda")
    for bad in (np.zeros((3, 10, 2)), np.zeros((10, 3)), np.zeros((3, 0, 3))):
        with pytest.raises(ValueError, match="points"):
            Mt.compute_ADD_batched(bad, None, pose, pose, device="cuda")
    with pytest.raises(ValueError):  # the single-problem API: a pose of 6 numbers
        Mt.compute_ADD_np(np.zeros((10, 3)), np.zeros(7), np.zeros(6))
