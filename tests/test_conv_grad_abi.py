"""sv_conv_wgrad without a GPU: argument checks (host code, nothing launched) and the workspace size."""
import ctypes

import pytest


def _wgrad(lib, Cin=64, Cout=64, K=27, V_out=10, Vpad=128, in_=None, dy=None, dW=None, ws=None, ws_bytes=0, plan=False,
           perm=None):
    # (in, V_in, in_ld, Cin, dy, V_out, dy_ld, Cout, K, perm, nbr_s, submask, Vpad, accumulate, workspace,
    #  workspace_bytes, dW, stream)
    p = ctypes.c_void_p(4096) if plan else None
    return lib.sv_conv_wgrad(in_, 10, max(Cin, 1), Cin, dy, V_out, max(Cout, 1), Cout, K, perm if perm is not None else p, p,
                             p, Vpad, 0, ws, ws_bytes, dW, None)


FAKE = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below fails its host-side checks first


def test_conv_wgrad_null_pointers():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    rc = _wgrad(lib, dW=None, in_=FAKE, dy=FAKE, plan=True)
    assert rc == -1 and b"null pointer" in lib.sv_last_error()
    rc = _wgrad(lib, dW=FAKE, in_=None, dy=FAKE, plan=True)
    assert rc == -1 and b"null pointer" in lib.sv_last_error()
    rc = _wgrad(lib, dW=FAKE, in_=FAKE, dy=None, plan=True)
    assert rc == -1 and b"null pointer" in lib.sv_last_error()
    # a plan needs all three arrays; K > 1 needs a plan
    rc = lib.sv_conv_wgrad(FAKE, 10, 64, 64, FAKE, 10, 64, 64, 27, FAKE, None, None, 128, 0, None, 0, FAKE, None)
    assert rc == -1 and b"together" in lib.sv_last_error()
    rc = _wgrad(lib, dW=FAKE, in_=FAKE, dy=FAKE, plan=False)
    assert rc == -1 and b"needs a plan" in lib.sv_last_error()


@pytest.mark.parametrize("Cin,Cout,K", [(0, 64, 27), (64, 0, 27), (-3, 64, 1), (64, 64, 0), (64, 64, 33)])
def test_conv_wgrad_bad_counts(Cin, Cout, K):
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    rc = _wgrad(lib, Cin, Cout, K, in_=FAKE, dy=FAKE, dW=FAKE, plan=True)
    assert rc == -1 and b"bad channel / kernel volume" in lib.sv_last_error()


def test_conv_wgrad_plan_shape_and_alignment():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    rc = _wgrad(lib, Vpad=100, in_=FAKE, dy=FAKE, dW=FAKE, plan=True)
    assert rc == -1 and b"multiple of 128" in lib.sv_last_error()
    rc = _wgrad(lib, V_out=300, Vpad=256, in_=FAKE, dy=FAKE, dW=FAKE, plan=True)
    assert rc == -1 and b"multiple of 128" in lib.sv_last_error()
    rc = _wgrad(lib, in_=FAKE, dy=FAKE, dW=FAKE, plan=True, perm=ctypes.c_void_p(4098))
    assert rc == -1 and b"aligned" in lib.sv_last_error()
    rc = lib.sv_conv_wgrad(FAKE, 10, 32, 64, FAKE, 10, 64, 64, 27, FAKE, FAKE, FAKE, 128, 0, None, 0, FAKE, None)
    assert rc == -1 and b"row strides" in lib.sv_last_error()


def test_conv_wgrad_workspace_too_small():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    need = lib.sv_conv_wgrad_workspace_bytes(128, 27, 64, 64)
    assert need >= 27 * 64 * 64 * 4
    for have in (0, need - 1):
        rc = _wgrad(lib, in_=FAKE, dy=FAKE, dW=FAKE, plan=True, ws=FAKE, ws_bytes=have)
        assert rc == -2 and b"workspace too small" in lib.sv_last_error()


def test_conv_wgrad_workspace_bytes_monotone_in_v():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    for K, Cin, Cout in ((27, 3, 32), (27, 32, 32), (27, 384, 384), (8, 64, 128), (1, 256, 1024), (1, 1024, 3)):
        last = 0
        for V in (1, 100, 128, 129, 1000, 5000, 26552, 88113, 200000, 1 << 22):
            b = lib.sv_conv_wgrad_workspace_bytes(V, K, Cin, Cout)
            assert b >= K * Cin * Cout * 4 and b >= last, (K, Cin, Cout, V, b, last)
            last = b
    assert lib.sv_conv_wgrad_workspace_bytes(0, 27, 64, 64) == 0
    assert lib.sv_conv_wgrad_workspace_bytes(128, 0, 64, 64) == 0


def test_conv_wgrad_empty_output_needs_no_workspace():
    """V_out = 0 has no pairs: the checks above still run, nothing is launched for accumulate = 1"""
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    rc = lib.sv_conv_wgrad(None, 0, 64, 64, None, 0, 64, 64, 27, FAKE, FAKE, FAKE, 0, 1, None, 0, FAKE, None)
    assert rc == 0
