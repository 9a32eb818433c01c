"""Argument checks of sv_estimate_normals and sv_icp_point2plane and of their Python wrappers (utils/icp.py): host code
only, nothing reaches a device, no GPU needed.  As tests/test_pose_solver_args.py: every library call here fails its
checks before any HIP call, and the wrappers reject bad arguments before a tensor is moved, which the `no_launch`
fixture enforces by replacing the library call."""
import ctypes

import numpy as np
import pytest

NAN = float("nan")


def _buf(n):
    """A host buffer standing in for a non-null pointer (never dereferenced: every call here fails its checks)."""
    return ctypes.create_string_buffer(n)


def test_normals_argument_checks_without_gpu():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    p = _buf(64)
    N = 1000
    need = lib.sv_normals_workspace_bytes(N, 30)
    assert need >= 1

    def normals(N=N, radius=0.02, max_nn=30, xyz=p, ws=p, ws_bytes=need, out=p, counts=p):
        # (xyz, N, radius, max_nn, workspace, workspace_bytes, normals, counts, stream)
        return lib.sv_estimate_normals(xyz, N, radius, max_nn, ws, ws_bytes, out, counts, None)

    for kw in ({"N": 0}, {"N": -1}, {"N": (1 << 20) + 1}):
        assert normals(**kw) == -1 and b"2^20 points" in lib.sv_last_error(), kw
    for kw in ({"radius": 0.0}, {"radius": -0.02}, {"radius": NAN}, {"radius": 1e-30}, {"radius": 1e30}):
        assert normals(**kw) == -1 and b"bad radius" in lib.sv_last_error(), kw
    for kw in ({"max_nn": 2}, {"max_nn": 0}, {"max_nn": -5}, {"max_nn": 65}, {"max_nn": 1 << 20}):
        assert normals(**kw) == -1 and b"max_nn" in lib.sv_last_error(), kw
    for kw in ({"xyz": None}, {"ws": None}, {"out": None}):
        assert normals(**kw) == -1 and b"null pointer" in lib.sv_last_error(), kw
    # the neighbour counts are optional, but a workspace one byte short is SV_ERR_WORKSPACE before anything is launched
    for ws_bytes in (0, need - 1):
        assert normals(ws_bytes=ws_bytes) == -2 and b"workspace too small" in lib.sv_last_error(), ws_bytes
        assert normals(ws_bytes=ws_bytes, counts=None) == -2


def test_icp_point2plane_argument_checks_without_gpu():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    p = _buf(64)
    S, T = 100, 50
    need = lib.sv_icp_point2plane_workspace_bytes(S)
    assert need >= S * 8

    def icp(S=S, T=T, max_distance=0.1, max_iterations=30, src=p, tgt=p, nrm=p, ws=p, ws_bytes=need, out_T=p):
        # (src, S, tgt, tgt_normals, T, init_T, max_distance, max_iterations, rel_fitness, rel_rmse, ws, ws_bytes, out_T,
        #  stats, stream)
        return lib.sv_icp_point2plane(src, S, tgt, nrm, T, None, max_distance, max_iterations, 1e-6, 1e-6, ws, ws_bytes,
                                      out_T, None, None)

    for kw in ({"S": 2}, {"S": 0}, {"S": -1}, {"T": 0}, {"S": 1 << 24}, {"T": 1 << 24}):
        assert icp(**kw) == -1 and b"at least 3 source points" in lib.sv_last_error(), kw
    for kw in ({"max_distance": 0.0}, {"max_distance": -0.1}, {"max_distance": NAN}, {"max_iterations": -1}):
        assert icp(**kw) == -1 and b"bad parameters" in lib.sv_last_error(), kw
    for kw in ({"src": None}, {"tgt": None}, {"nrm": None}, {"ws": None}, {"out_T": None}):
        assert icp(**kw) == -1 and b"null pointer" in lib.sv_last_error(), kw
    for ws_bytes in (0, 256, 256 + S * 4):
        assert icp(ws_bytes=ws_bytes) == -2 and b"workspace too small" in lib.sv_last_error(), ws_bytes
    # one byte short of what the state record and the two per-point arrays take at 256-byte alignment (the size function
    # rounds up and adds slack): 256 + align(4 S) + 4 S
    used = 256 + 512 + S * 4
    assert icp(ws_bytes=used - 1) == -2 and b"sv_icp_point2plane" in lib.sv_last_error()


@pytest.fixture
def no_launch(monkeypatch):
    """Replace the wrappers' library call: reaching it means a bad argument got past the checks."""
    from mrcc_amd.utils import icp

    def fail(name, *args):
        raise AssertionError(f"{name} was called with arguments the wrapper should have rejected")

    monkeypatch.setattr(icp, "call", fail)


def test_estimate_normals_wrapper_rejects_bad_arguments(no_launch):
    from mrcc_amd.utils import icp as I

    pts = np.zeros((100, 3), np.float32)
    for bad in (np.zeros((100, 2)), np.zeros(300), np.zeros((0, 3)), np.zeros((2, 100, 3))):
        with pytest.raises(ValueError, match="points"):
            I.estimate_normals(bad)
    for radius in (0.0, -0.02, NAN):
        with pytest.raises(ValueError, match="radius"):
            I.estimate_normals(pts, radius=radius)
    for max_nn in (0, 2, 65, -1):
        with pytest.raises(ValueError, match="max_nn"):
            I.estimate_normals(pts, max_nn=max_nn)


def test_icp_point2plane_wrapper_rejects_bad_arguments(no_launch):
    from mrcc_amd.utils import icp as I

    src, tgt = np.zeros((10, 3), np.float32), np.zeros((20, 3), np.float32)
    for s, t, n, word in ((src[:2], tgt, tgt, "src"), (src[:, :2], tgt, tgt, "src"), (src, tgt[:0], tgt[:0], "tgt"),
                          (src, np.zeros(60), tgt, "tgt"), (src, tgt, tgt[:19], "tgt_normals"),
                          (src, tgt, np.zeros((20, 4)), "tgt_normals")):
        with pytest.raises(ValueError, match=word):
            I.icp_point2plane(s, t, n)
    for kw in ({"max_distance": 0.0}, {"max_distance": -1.0}, {"max_distance": NAN}):
        with pytest.raises(ValueError, match="max_distance"):
            I.icp_point2plane(src, tgt, tgt, **kw)
    with pytest.raises(ValueError, match="max_iterations"):
        I.icp_point2plane(src, tgt, tgt, max_iterations=-1)
    with pytest.raises(ValueError, match="init_T"):
        I.icp_point2plane(src, tgt, tgt, init_T=np.eye(3))
    # the matcher checks its normal-search parameters when it is built, before the CAD points are moved
    for kw in ({"normal_radius": 0.0}, {"normal_radius": NAN}):
        with pytest.raises(ValueError, match="radius"):
            I.get_point2plane_matcher(src, **kw)
    for kw in ({"normal_max_nn": 2}, {"normal_max_nn": 65}):
        with pytest.raises(ValueError, match="max_nn"):
            I.get_point2plane_matcher(src, **kw)
    with pytest.raises(ValueError, match="cad_points"):
        I.get_point2plane_matcher(np.zeros((10, 2)))


def test_engine_rejects_an_unknown_icp_method():
    from mrcc_amd.app.inference_engine import InferenceEngine

    with pytest.raises(ValueError, match="icp_method"):
        InferenceEngine(calibration_only=True, icp_method="point2line")
    assert InferenceEngine(calibration_only=True).icp_method == "point2point"
    assert InferenceEngine(calibration_only=True, icp_method="point2plane").icp_method == "point2plane"
