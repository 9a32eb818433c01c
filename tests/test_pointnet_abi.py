"""Argument checks of the PointNet++ entries (sv_pointnet_sa, sv_fps_segmented): host code, no launch, no GPU."""
import ctypes


def _widths(*w):
    return (ctypes.c_int * len(w))(*w)


def test_pointnet_sa_argument_checks_without_gpu():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    unsupported = mrcc_amd._lib.SV_ERR_UNSUPPORTED
    # (xyz, points, new_xyz, idx, B, N, D, S, nsample, params, widths, L, out, stream)
    rc = lib.sv_pointnet_sa(None, None, None, None, 1, 2048, 6, 1024, 32, None, _widths(9, 32, 32, 64), 3, None, None)
    assert rc == -1 and b"null pointer" in lib.sv_last_error()
    rc = lib.sv_pointnet_sa(None, None, None, None, 1, 2048, 6, 1024, 32, None, None, 3, None, None)
    assert rc == -1 and b"null pointer" in lib.sv_last_error()
    rc = lib.sv_pointnet_sa(None, None, None, None, 1, 2048, 5, 1024, 32, None, _widths(9, 32, 32, 64), 3, None, None)
    assert rc == -1 and b"3 + D" in lib.sv_last_error()
    rc = lib.sv_pointnet_sa(None, None, None, None, 1, 0, 6, 1024, 32, None, _widths(9, 32, 32, 64), 3, None, None)
    assert rc == -1 and b"bad shape" in lib.sv_last_error()
    # shapes the fused kernel does not cover: SV_ERR_UNSUPPORTED before any pointer is looked at
    for ns in (8, 24, 128):
        rc = lib.sv_pointnet_sa(None, None, None, None, 1, 2048, 6, 1024, ns, None, _widths(9, 32, 32, 64), 3, None, None)
        assert rc == unsupported and b"nsample" in lib.sv_last_error()
    rc = lib.sv_pointnet_sa(None, None, None, None, 1, 2048, 6, 1024, 32, None, _widths(9, 32, 24, 64), 3, None, None)
    assert rc == unsupported and b"multiples of 16" in lib.sv_last_error()
    rc = lib.sv_pointnet_sa(None, None, None, None, 1, 2048, 6, 1024, 32, None, _widths(9, 32, 32, 64, 64, 64), 5,
                            None, None)
    assert rc == unsupported and b"layer count" in lib.sv_last_error()
    rc = lib.sv_pointnet_sa(None, None, None, None, 1, 64, 1021, 16, 32, None, _widths(1024, 1024, 64), 2, None, None)
    assert rc == unsupported and b"LDS" in lib.sv_last_error()
    # the SSG's largest set abstraction fits (259 -> 256 -> 256 -> 512 on a 64-row tile): only the pointers are missing
    rc = lib.sv_pointnet_sa(None, None, None, None, 1, 64, 256, 16, 32, None, _widths(259, 256, 256, 512), 3, None, None)
    assert rc == -1 and b"null pointer" in lib.sv_last_error()
    # B = 0: nothing to do
    assert lib.sv_pointnet_sa(None, None, None, None, 0, 64, 256, 16, 32, None, _widths(259, 256, 256, 512), 3, None,
                              None) == 0


def test_fps_argument_checks_without_gpu():
    """sv_fps beyond the LDS-resident distance array (N = 38401): an argument error before any pointer is looked at or
    anything is launched; N = 38400 passes that check (only the pointers are missing)."""
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    # (xyz, B, N, S, start, out, stream)
    rc = lib.sv_fps(None, 2, 38401, 16, None, None, None)
    assert rc == -1 and b"too large" in lib.sv_last_error()
    rc = lib.sv_fps(None, 2, 38400, 16, None, None, None)
    assert rc == -1 and b"null pointer" in lib.sv_last_error()
    rc = lib.sv_fps(None, 2, 0, 16, None, None, None)
    assert rc == -1 and b"bad shape" in lib.sv_last_error()
    assert lib.sv_fps(None, 0, 38400, 16, None, None, None) == 0


def test_fps_segmented_argument_checks_without_gpu():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    rc = lib.sv_fps_segmented(None, None, None, None, 3, 100000, None, None)
    assert rc == -1 and b"too large" in lib.sv_last_error()
    rc = lib.sv_fps_segmented(None, None, None, None, 3, 0, None, None)
    assert rc == -1 and b"bad shape" in lib.sv_last_error()
    rc = lib.sv_fps_segmented(None, None, None, None, 3, 2048, None, None)
    assert rc == -1 and b"null pointer" in lib.sv_last_error()
    assert lib.sv_fps_segmented(None, None, None, None, 0, 2048, None, None) == 0
