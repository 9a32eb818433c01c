"""Argument checks of sv_icp_batched and of its Python wrappers (utils/icp.py icp_batched, icp_joint, the matchers'
many): host code only, no GPU needed.  As tests/test_icp_plane_abi.py: every library call here fails its checks before
any HIP call, and the wrappers reject bad arguments before a tensor is moved, which the `no_launch` fixture enforces."""
import ctypes

import numpy as np
import pytest

NAN = float("nan")


def _buf(n):
    """A host buffer standing in for a non-null pointer (never dereferenced: every call here fails its checks)."""
    return ctypes.create_string_buffer(n)


def _offsets(*values):
    return (ctypes.c_int64 * len(values))(*values)


def test_symbols_are_exported_and_declared():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    for name in ("sv_icp_batched_workspace_bytes", "sv_icp_batched"):
        assert name in mrcc_amd._lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert len(mrcc_amd._lib.SIGNATURES["sv_icp_batched"][1]) == 18
    assert lib.sv_abi_version() == 4


def test_workspace_grows_with_points_and_problems():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    size = lib.sv_icp_batched_workspace_bytes
    assert size(1000, 1) >= 1000 * 8
    assert size(2000, 1) > size(1000, 1)
    assert size(1000, 2) > size(1000, 1)
    assert size(8192, 64) >= 64 * 8192 * 8
    assert size(8192, 64) > size(8192, 63) > size(8191, 63) - 1


def test_icp_batched_argument_checks_without_gpu():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    p = _buf(64)
    S = 100
    good = _offsets(0, 50, 51, 120)
    need = lib.sv_icp_batched_workspace_bytes(S, 3)

    def icp(S=S, P=3, off=good, shared=0, max_distance=0.1, max_iterations=30, src=p, tgt=p, nrm=None, pre=None, ws=p,
            ws_bytes=need, out_T=p):
        # (src, S, pre, tgt, tgt_normals, tgt_offsets, P, init_T, shared, max_distance, max_iterations, rel_fitness,
        #  rel_rmse, workspace, workspace_bytes, out_T, out_stats, stream)
        return lib.sv_icp_batched(src, S, pre, tgt, nrm, off, P, None, shared, max_distance, max_iterations, 1e-6, 1e-6,
                                  ws, ws_bytes, out_T, None, None)

    many = _offsets(*range(66))
    for kw in ({"P": 0}, {"P": -1}, {"P": 65, "off": many}):
        assert icp(**kw) == -1 and b"1 to 64 problems" in lib.sv_last_error(), kw
    for kw in ({"S": 2}, {"S": 0}, {"S": -1}, {"S": 1 << 24}):
        assert icp(**kw) == -1 and b"source points" in lib.sv_last_error(), kw
    for kw in ({"max_distance": 0.0}, {"max_distance": -0.1}, {"max_distance": NAN}, {"max_iterations": -1},
               {"shared": 2}, {"shared": -1}):
        assert icp(**kw) == -1 and b"bad parameters" in lib.sv_last_error(), kw
    for kw in ({"src": None}, {"tgt": None}, {"off": None}, {"ws": None}, {"out_T": None}):
        assert icp(**kw) == -1 and b"null pointer" in lib.sv_last_error(), kw
    assert icp(off=_offsets(1, 50, 51, 120)) == -1 and b"start at 0" in lib.sv_last_error()
    for off in (_offsets(0, 50, 40, 120),        # descends
                _offsets(0, 50, 50, 120),        # an empty problem
                _offsets(0, 0, 51, 120),         # the first one empty
                _offsets(0, 50, 51, 51),         # the last one empty
                _offsets(0, 50, 51, 51 + (1 << 24))):  # too many target points
        assert icp(off=off) == -1 and b"target points" in lib.sv_last_error(), list(off)
    # both objectives and both modes get as far as the workspace check, which fails before anything is launched
    for kw in ({}, {"nrm": p}, {"shared": 1}, {"shared": 1, "nrm": p, "pre": p}):
        for ws_bytes in (0, 256, need // 2):
            assert icp(ws_bytes=ws_bytes, **kw) == -2 and b"workspace too small" in lib.sv_last_error(), (kw, ws_bytes)
    # one byte short of what the carving takes at 256-byte alignment: states, nn, d2, partial sums, per-problem stats
    # (the size function rounds up and adds slack)
    align = lambda n: (n + 255) // 256 * 256
    used = align(align(align(align(3 * 152) + 3 * S * 4) + 3 * S * 4) + 3 * 32 * 8) + 3 * 2 * 8
    assert used <= need
    assert icp(ws_bytes=used - 1) == -2 and b"sv_icp_batched" in lib.sv_last_error()


@pytest.fixture
def no_launch(monkeypatch):
    """Replace the wrappers' library call: reaching it means a bad argument got past the checks."""
    from mrcc_amd.utils import icp

    def fail(name, *args):
        raise AssertionError(f"{name} was called with arguments the wrapper should have rejected")

    monkeypatch.setattr(icp, "call", fail)


def test_icp_batched_wrapper_rejects_bad_arguments(no_launch):
    from mrcc_amd.utils import icp as I

    src, a, b = np.zeros((10, 3), np.float32), np.zeros((20, 3), np.float32), np.zeros((7, 3), np.float32)
    for s, tgts, word in ((src[:2], [a, b], "src"), (src[:, :2], [a, b], "src"), (np.zeros(30), [a, b], "src"),
                          (src, [], "tgts"), (src, [a] * 65, "tgts"), (src, [a, b[:0]], "tgt"),
                          (src, [a, np.zeros(21)], r"tgts\[1\]"), (src, [np.zeros((20, 4)), b], r"tgts\[0\]")):
        for fn in (I.icp_batched, I.icp_joint):
            with pytest.raises(ValueError, match=word):
                fn(s, tgts)
    for normals, word in (([a], "tgt_normals"), ([a, b, b], "tgt_normals"), ([a, b[:6]], "tgt_normals"),
                          ([a[:19], b], "tgt_normals"), ([a, np.zeros((7, 2))], r"tgt_normals\[1\]")):
        with pytest.raises(ValueError, match=word):
            I.icp_batched(src, [a, b], tgt_normals=normals)
    eye = np.eye(4)
    for init in (eye, np.stack([eye] * 3), np.zeros((2, 3, 4))):
        with pytest.raises(ValueError, match="init_Ts"):
            I.icp_batched(src, [a, b], init)
    with pytest.raises(ValueError, match="init_Ts"):
        I.icp_joint(src, [a, b], np.stack([eye] * 2))
    for pre in (eye, np.stack([eye] * 3)):
        with pytest.raises(ValueError, match="pre"):
            I.icp_joint(src, [a, b], pre=pre)
    for kw in ({"max_distance": 0.0}, {"max_distance": NAN}):
        with pytest.raises(ValueError, match="max_distance"):
            I.icp_batched(src, [a, b], **kw)
    with pytest.raises(ValueError, match="max_iterations"):
        I.icp_batched(src, [a, b], max_iterations=-1)


def test_matchers_many_rejects_bad_arguments(no_launch):
    """_refine_many is what both matchers' many() run; its checks come before the first crop is moved"""
    from mrcc_amd.utils import icp as I

    cad, a = np.zeros((10, 3), np.float32), np.zeros((20, 3), np.float32)
    pose = np.array([0, 0, 0, 1, 0, 0, 0.0])
    with pytest.raises(ValueError, match="same length"):
        I._refine_many(cad, [a, a], [pose], None, 0.1, 30, "cpu")
    with pytest.raises(ValueError, match=r"crops\[1\]"):
        I._refine_many(cad, [a, np.zeros((20, 2))], [pose, pose], None, 0.1, 30, "cpu")
    with pytest.raises(ValueError, match="tgt"):
        I._refine_many(cad, [a[:0]], [pose], None, 0.1, 30, "cpu")
    # pairs with a None crop or pose are not looked at and keep their pose
    out = I._refine_many(cad, [None, np.zeros(5)], [pose, None], None, 0.1, 30, "cpu")
    assert out[0] is pose and out[1] is None


def test_refine_base_pose_rejects_bad_arguments(no_launch):
    from mrcc_amd.utils.calibration import refine_base_pose

    cad, a = np.zeros((10, 3), np.float32), np.zeros((20, 3), np.float32)
    pose = np.array([0, 0, 0, 1, 0, 0, 0.0])
    with pytest.raises(ValueError, match="method"):
        refine_base_pose(cad, [a, a], [pose, pose], pose, method="point2line")
    with pytest.raises(ValueError, match="per crop"):
        refine_base_pose(cad, [a, a], [pose], pose)
    with pytest.raises(ValueError, match="per crop"):
        refine_base_pose(cad, [], [], pose)
    with pytest.raises(ValueError, match="normals"):
        refine_base_pose(cad, [a, a], [pose, pose], pose, normals=[a])
    with pytest.raises(ValueError, match=r"tgts\[1\]"):
        refine_base_pose(cad, [a, np.zeros((20, 2))], [pose, pose], pose)


def test_engine_takes_the_batched_flag_and_needs_cad_points_to_refine():
    from mrcc_amd.app.dto import CalibrationResultDTO
    from mrcc_amd.app.inference_engine import InferenceEngine

    assert InferenceEngine(calibration_only=True).icp_batched is False
    engine = InferenceEngine(calibration_only=True, icp_batched=True)
    assert engine.icp_batched is True
    with pytest.raises(ValueError, match="cad_points"):
        engine.refine_calibration(CalibrationResultDTO(pose_camera_link=np.array([0, 0, 0, 1, 0, 0, 0.0])), [], [])
