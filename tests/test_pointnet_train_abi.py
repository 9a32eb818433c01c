"""The PointNet++ training entries without a GPU: argument checks (host code, nothing launched), the group_all / D = 0
forms, workspace sizes, and set_training_path on CPU-built networks."""
import ctypes

import pytest

FAKE = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below fails its host-side checks first


def _lib():
    import mrcc_amd

    return mrcc_amd._lib.load()


def test_group_rows_checks():
    lib = _lib()
    # (xyz, points, new_xyz, idx, B, N, D, S, nsample, order, ld, out, stream)
    assert lib.sv_group_rows(None, FAKE, FAKE, FAKE, 2, 64, 4, 8, 16, 0, 7, FAKE, None) == -1
    assert b"null pointer" in lib.sv_last_error()
    assert lib.sv_group_rows(FAKE, None, FAKE, FAKE, 2, 64, 4, 8, 16, 0, 7, FAKE, None) == -1  # D > 0 needs points
    assert b"null pointer" in lib.sv_last_error()
    assert lib.sv_group_rows(FAKE, FAKE, None, FAKE, 2, 64, 4, 8, 16, 0, 7, FAKE, None) == -1  # ball groups need new_xyz
    assert b"null pointer" in lib.sv_last_error()
    assert lib.sv_group_rows(FAKE, FAKE, FAKE, FAKE, 2, 64, 4, 8, 16, 0, 7, None, None) == -1
    assert b"null pointer" in lib.sv_last_error()
    assert lib.sv_group_rows(FAKE, FAKE, FAKE, FAKE, 2, 64, 4, 8, 16, 0, 6, FAKE, None) == -1
    assert b"ld must be at least" in lib.sv_last_error()
    assert lib.sv_group_rows(FAKE, FAKE, FAKE, FAKE, 2, 64, 4, 8, 16, 2, 7, FAKE, None) == -1
    assert b"order" in lib.sv_last_error()
    for bad in [(2, 0, 4, 8, 16), (2, 64, -1, 8, 16), (2, 64, 4, 0, 16), (2, 64, 4, 8, 0), (-1, 64, 4, 8, 16)]:
        B, N, D, S, K = bad
        assert lib.sv_group_rows(FAKE, FAKE, FAKE, FAKE, B, N, D, S, K, 0, 3 + max(D, 0), FAKE, None) == -1
        assert b"bad shape" in lib.sv_last_error()
    # group_all (idx NULL): S = 1, nsample = N, SSG order; new_xyz may be NULL
    assert lib.sv_group_rows(FAKE, FAKE, None, None, 2, 64, 4, 2, 64, 0, 7, FAKE, None) == -1
    assert b"group_all" in lib.sv_last_error()
    assert lib.sv_group_rows(FAKE, FAKE, None, None, 2, 64, 4, 1, 32, 0, 7, FAKE, None) == -1
    assert b"group_all" in lib.sv_last_error()
    assert lib.sv_group_rows(FAKE, FAKE, None, None, 2, 64, 4, 1, 64, 1, 7, FAKE, None) == -1
    assert b"group_all" in lib.sv_last_error()
    # D = 0 needs no points; B = 0 launches nothing
    assert lib.sv_group_rows(FAKE, None, FAKE, FAKE, 0, 64, 0, 8, 16, 1, 3, FAKE, None) == 0
    assert lib.sv_group_rows(FAKE, None, None, None, 0, 64, 0, 1, 64, 0, 3, FAKE, None) == 0
    assert lib.sv_group_rows(FAKE, FAKE, FAKE, FAKE, 1 << 12, 1 << 12, 64, 1 << 12, 32, 0, 67, FAKE, None) == -1
    assert b"too many" in lib.sv_last_error()


def test_index_transpose_checks_and_workspace():
    lib = _lib()
    small = lib.sv_index_transpose_workspace_bytes(0, 0, 16)
    big = lib.sv_index_transpose_workspace_bytes(32, 1024 * 32, 2048)
    assert small > 0 and big >= 2 * 4 * 32 * 1024 * 32  # two key arrays at least
    assert lib.sv_index_transpose_workspace_bytes(32, 2048, 1) < big
    # (idx, idx_bytes, B, M, N, workspace, workspace_bytes, offsets, pos, stream)
    assert lib.sv_index_transpose(FAKE, 2, 2, 16, 8, FAKE, 1 << 20, FAKE, FAKE, None) == -1
    assert b"idx_bytes" in lib.sv_last_error()
    assert lib.sv_index_transpose(FAKE, 8, 2, 16, 0, FAKE, 1 << 20, FAKE, FAKE, None) == -1
    assert b"bad shape" in lib.sv_last_error()
    assert lib.sv_index_transpose(FAKE, 8, 2, -1, 8, FAKE, 1 << 20, FAKE, FAKE, None) == -1
    assert b"bad shape" in lib.sv_last_error()
    assert lib.sv_index_transpose(None, 8, 2, 16, 8, FAKE, 1 << 20, FAKE, FAKE, None) == -1
    assert b"null pointer" in lib.sv_last_error()
    assert lib.sv_index_transpose(FAKE, 4, 2, 16, 8, FAKE, 1 << 20, None, FAKE, None) == -1
    assert b"null pointer" in lib.sv_last_error()
    assert lib.sv_index_transpose(FAKE, 4, 2, 16, 8, FAKE, 1 << 20, FAKE, None, None) == -1
    assert b"null pointer" in lib.sv_last_error()
    need = lib.sv_index_transpose_workspace_bytes(2, 16, 8)
    assert lib.sv_index_transpose(FAKE, 8, 2, 16, 8, FAKE, need - 1, FAKE, FAKE, None) == -2
    assert b"workspace too small" in lib.sv_last_error()
    assert lib.sv_index_transpose(FAKE, 8, 2, 16, 8, None, need, FAKE, FAKE, None) == -2
    assert lib.sv_index_transpose(FAKE, 8, 1 << 16, 1 << 16, 8, FAKE, 1 << 40, FAKE, FAKE, None) == -1
    assert b"too many" in lib.sv_last_error()


def test_gather_transpose_checks():
    lib = _lib()
    # (offsets, pos, w, rows, ld_rows, col0, C, per_row, T, out, ld_out, stream)
    assert lib.sv_gather_transpose(None, FAKE, None, FAKE, 67, 3, 64, 1, 100, FAKE, 64, None) == -1
    assert b"null pointer" in lib.sv_last_error()
    assert lib.sv_gather_transpose(FAKE, None, None, FAKE, 67, 3, 64, 1, 100, FAKE, 64, None) == -1
    assert lib.sv_gather_transpose(FAKE, FAKE, None, None, 67, 3, 64, 1, 100, FAKE, 64, None) == -1
    assert lib.sv_gather_transpose(FAKE, FAKE, None, FAKE, 67, 3, 64, 1, 100, None, 64, None) == -1
    assert b"null pointer" in lib.sv_last_error()
    assert lib.sv_gather_transpose(FAKE, FAKE, None, FAKE, 66, 3, 64, 1, 100, FAKE, 64, None) == -1
    assert b"row strides" in lib.sv_last_error()
    assert lib.sv_gather_transpose(FAKE, FAKE, None, FAKE, 67, 3, 64, 1, 100, FAKE, 63, None) == -1
    assert b"row strides" in lib.sv_last_error()
    for col0, C, per_row, T in [(-1, 64, 1, 100), (3, 0, 1, 100), (3, 64, 0, 100), (3, 64, 1, -1)]:
        assert lib.sv_gather_transpose(FAKE, FAKE, None, FAKE, 67, col0, C, per_row, T, FAKE, 64, None) == -1
        assert b"bad shape" in lib.sv_last_error()
    assert lib.sv_gather_transpose(None, None, None, None, 67, 3, 64, 1, 0, None, 64, None) == 0  # T = 0: nothing


def test_group_max_checks():
    lib = _lib()
    # (rows, ld, G, nsample, C, out, arg, stream)
    assert lib.sv_group_max(None, 64, 10, 32, 64, FAKE, FAKE, None) == -1
    assert lib.sv_group_max(FAKE, 64, 10, 32, 64, None, FAKE, None) == -1
    assert lib.sv_group_max(FAKE, 64, 10, 32, 64, FAKE, None, None) == -1
    assert b"null pointer" in lib.sv_last_error()
    for ld, G, K, C in [(63, 10, 32, 64), (64, -1, 32, 64), (64, 10, 0, 64), (64, 10, 32, 0)]:
        assert lib.sv_group_max(FAKE, ld, G, K, C, FAKE, FAKE, None) == -1
        assert b"bad shape" in lib.sv_last_error()
    # group_all: G = B, nsample = N (any N)
    assert lib.sv_group_max(None, 1024, 0, 128, 1024, None, None, None) == 0
    # (dpooled, arg, G, nsample, C, drows, stream)
    assert lib.sv_group_max_backward(None, FAKE, 10, 32, 64, FAKE, None) == -1
    assert lib.sv_group_max_backward(FAKE, None, 10, 32, 64, FAKE, None) == -1
    assert lib.sv_group_max_backward(FAKE, FAKE, 10, 32, 64, None, None) == -1
    assert b"null pointer" in lib.sv_last_error()
    assert lib.sv_group_max_backward(FAKE, FAKE, 10, 0, 64, FAKE, None) == -1
    assert b"bad shape" in lib.sv_last_error()
    assert lib.sv_group_max_backward(FAKE, FAKE, 1 << 20, 1 << 10, 64, FAKE, None) == -1
    assert b"too many" in lib.sv_last_error()


def test_three_nn_checks():
    lib = _lib()
    # (xyz1, xyz2, B, N, S, idx, w, stream)
    assert lib.sv_three_nn(FAKE, FAKE, 2, 100, 2, FAKE, FAKE, None) == -1
    assert b"S >= 3" in lib.sv_last_error()
    assert lib.sv_three_nn(FAKE, FAKE, 2, 0, 16, FAKE, FAKE, None) == -1
    for args in [(None, FAKE, FAKE, FAKE), (FAKE, None, FAKE, FAKE), (FAKE, FAKE, None, FAKE), (FAKE, FAKE, FAKE, None)]:
        x1, x2, idx, w = args
        assert lib.sv_three_nn(x1, x2, 2, 100, 16, idx, w, None) == -1
        assert b"null pointer" in lib.sv_last_error()
    # (points2, idx, w, B, N, S, C, out, stream)
    assert lib.sv_three_nn_gather(FAKE, FAKE, FAKE, 2, 100, 16, 0, FAKE, None) == -1
    assert b"bad shape" in lib.sv_last_error()
    assert lib.sv_three_nn_gather(FAKE, FAKE, FAKE, 2, 100, 2, 8, FAKE, None) == -1
    for args in [(None, FAKE, FAKE, FAKE), (FAKE, None, FAKE, FAKE), (FAKE, FAKE, None, FAKE), (FAKE, FAKE, FAKE, None)]:
        p2, idx, w, out = args
        assert lib.sv_three_nn_gather(p2, idx, w, 2, 100, 16, 8, out, None) == -1
        assert b"null pointer" in lib.sv_last_error()


def test_set_training_path_names_and_validation():
    import mrcc_amd  # noqa: F401
    from mrcc_amd.model import pointnet2_utils as U
    from mrcc_amd.model.pointnet2 import PointNet2MSGEncoder, PointNet2SSG, set_training_path

    assert set_training_path is U.set_training_path
    ssg = PointNet2SSG(6, in_channels=6)
    assert set_training_path(ssg, "hip") == ["", "sa1", "sa2", "sa3", "sa4", "fp4", "fp3", "fp2", "fp1"]
    assert all(m.training_path == "hip" for _, m in ssg.named_modules() if getattr(type(m), "_hip_trainable", False))
    msg = PointNet2MSGEncoder(7)
    assert set_training_path(msg, "hip") == ["", "sa1", "sa2", "sa3"]
    assert msg.sa3.group_all and msg.sa3.training_path == "hip"
    with pytest.raises(ValueError):
        set_training_path(msg, "bf16")
    with pytest.raises(ValueError):
        set_training_path(msg, None)
    # not in state_dict; kept by train() / eval(), load_state_dict and .to()
    sd = msg.state_dict()
    assert not any("training_path" in k for k in sd)
    msg.eval().train()
    msg.load_state_dict(sd)
    msg.to("cpu")
    assert msg.sa1.training_path == "hip" and msg.training_path == "hip"
    assert set_training_path(msg, "torch") == ["", "sa1", "sa2", "sa3"]
    assert msg.sa2.training_path == "torch"
    # a single layer can be switched on its own
    fp = U.PointNetFeaturePropagation(128, [128])
    assert set_training_path(fp, "hip") == [""]


def test_default_training_path_is_torch():
    import mrcc_amd  # noqa: F401
    from mrcc_amd.model.pointnet2 import PointNet2SSG

    m = PointNet2SSG(6, in_channels=6).train()
    assert all(not _is_hip(mm) for mm in m.modules())


def _is_hip(m):
    from mrcc_amd.model.pointnet2_utils import _hip_train

    return _hip_train(m)
