"""sv_conv_wgrad_bf16 without a GPU: argument checks (host code, nothing launched), SV_ERR_UNSUPPORTED for the shapes it
does not cover, the workspace size, and nn.set_training_precision on a CPU-built RobotNetSegmentation(MinkUNet18D)."""
import ctypes

import pytest

FAKE = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below fails its host-side checks first


def _wgrad(lib, Cin=64, Cout=64, K=27, V_out=10, Vpad=128, in_=None, dy=None, dW=None, ws=None, ws_bytes=0, plan=False,
           perm=None, accumulate=0):
    # (in, V_in, in_ld, Cin, dy, V_out, dy_ld, Cout, K, perm, nbr_s, submask, Vpad, accumulate, workspace,
    #  workspace_bytes, dW, stream)
    p = ctypes.c_void_p(4096) if plan else None
    return lib.sv_conv_wgrad_bf16(in_, 10, max(Cin, 1), Cin, dy, V_out, max(Cout, 1), Cout, K,
                                  perm if perm is not None else p, p, p, Vpad, accumulate, ws, ws_bytes, dW, None)


def _lib():
    import mrcc_amd

    return mrcc_amd._lib.load()


def test_wgrad_bf16_null_pointers():
    lib = _lib()
    for kw in (dict(dW=None, in_=FAKE, dy=FAKE), dict(dW=FAKE, in_=None, dy=FAKE), dict(dW=FAKE, in_=FAKE, dy=None)):
        rc = _wgrad(lib, plan=True, **kw)
        assert rc == -1 and b"null pointer" in lib.sv_last_error(), kw
    rc = lib.sv_conv_wgrad_bf16(FAKE, 10, 64, 64, FAKE, 10, 64, 64, 27, FAKE, None, None, 128, 0, None, 0, FAKE, None)
    assert rc == -1 and b"together" in lib.sv_last_error()
    rc = _wgrad(lib, dW=FAKE, in_=FAKE, dy=FAKE, plan=False)
    assert rc == -1 and b"needs a plan" in lib.sv_last_error()


@pytest.mark.parametrize("Cin,Cout,K", [(0, 64, 27), (64, 0, 27), (-16, 64, 1), (64, 64, 0), (64, 64, 33)])
def test_wgrad_bf16_bad_counts(Cin, Cout, K):
    lib = _lib()
    rc = _wgrad(lib, Cin, Cout, K, in_=FAKE, dy=FAKE, dW=FAKE, plan=True)
    assert rc == -1 and b"bad channel / kernel volume" in lib.sv_last_error()


def test_wgrad_bf16_plan_shape_and_alignment():
    lib = _lib()
    rc = _wgrad(lib, Vpad=100, in_=FAKE, dy=FAKE, dW=FAKE, plan=True)
    assert rc == -1 and b"multiple of 128" in lib.sv_last_error()
    rc = _wgrad(lib, V_out=300, Vpad=256, in_=FAKE, dy=FAKE, dW=FAKE, plan=True)
    assert rc == -1 and b"multiple of 128" in lib.sv_last_error()
    rc = _wgrad(lib, in_=FAKE, dy=FAKE, dW=FAKE, plan=True, perm=ctypes.c_void_p(4098))
    assert rc == -1 and b"aligned" in lib.sv_last_error()
    rc = lib.sv_conv_wgrad_bf16(FAKE, 10, 32, 64, FAKE, 10, 64, 64, 27, FAKE, FAKE, FAKE, 128, 0, None, 0, FAKE, None)
    assert rc == -1 and b"row strides" in lib.sv_last_error()


def test_wgrad_bf16_unsupported_shapes_return_before_any_pointer():
    import mrcc_amd

    lib = _lib()
    unsupported = mrcc_amd._lib.SV_ERR_UNSUPPORTED
    for Cin, Cout, K in ((24, 64, 27), (64, 40, 27), (1024, 3, 1), (3, 32, 27), (64, 64, 28), (384, 384, 32)):
        # fake pointers everywhere, a workspace of 0 bytes: the shape is refused first
        rc = lib.sv_conv_wgrad_bf16(FAKE, 10, Cin, Cin, FAKE, 10, Cout, Cout, K, FAKE, FAKE, FAKE, 128, 0, FAKE, 0, FAKE,
                                    None)
        assert rc == unsupported, (Cin, Cout, K, rc)
        assert b"sv_conv_wgrad_bf16" in lib.sv_last_error() and b"sv_conv_wgrad" in lib.sv_last_error()
    # rows that are not 16-byte aligned (a column slice at an odd offset): the fp32 kernel's job
    rc = lib.sv_conv_wgrad_bf16(ctypes.c_void_p((1 << 20) + 4), 10, 64, 64, FAKE, 10, 64, 64, 27, FAKE, FAKE, FAKE, 128, 0,
                                FAKE, 1 << 30, FAKE, None)
    assert rc == unsupported and b"aligned" in lib.sv_last_error()
    rc = lib.sv_conv_wgrad_bf16(FAKE, 10, 66, 64, FAKE, 10, 64, 64, 27, FAKE, FAKE, FAKE, 128, 0, FAKE, 1 << 30, FAKE, None)
    assert rc == unsupported
    # the covered shapes of RobotNetSegmentation(MinkUNet18D) get as far as the null-pointer check
    for Cin, Cout, K in ((384, 384, 27), (416, 384, 27), (384, 384, 8), (256, 1024, 1), (32, 32, 27), (64, 96, 8)):
        rc = lib.sv_conv_wgrad_bf16(FAKE, 10, Cin, Cin, None, 10, Cout, Cout, K, FAKE, FAKE, FAKE, 128, 0, None, 0, FAKE,
                                    None)
        assert rc == -1 and b"null pointer" in lib.sv_last_error(), (Cin, Cout, K)


def test_wgrad_bf16_workspace_too_small():
    lib = _lib()
    need = lib.sv_conv_wgrad_bf16_workspace_bytes(128, 27, 64, 64)
    assert need >= 27 * 64 * 64 * 4
    for have in (0, need - 1):
        rc = _wgrad(lib, in_=FAKE, dy=FAKE, dW=FAKE, plan=True, ws=FAKE, ws_bytes=have)
        assert rc == -2 and b"workspace too small" in lib.sv_last_error()


def test_wgrad_bf16_workspace_bytes_monotone_in_v():
    lib = _lib()
    for K, Cin, Cout in ((27, 32, 32), (27, 384, 384), (27, 416, 384), (8, 384, 384), (8, 64, 128), (1, 256, 1024)):
        last = 0
        for V in (1, 100, 128, 129, 1000, 5000, 26552, 88113, 200000, 1 << 22):
            b = lib.sv_conv_wgrad_bf16_workspace_bytes(V, K, Cin, Cout)
            assert b >= K * Cin * Cout * 4 and b >= last, (K, Cin, Cout, V, b, last)
            last = b
    assert lib.sv_conv_wgrad_bf16_workspace_bytes(0, 27, 64, 64) == 0
    assert lib.sv_conv_wgrad_bf16_workspace_bytes(128, 0, 64, 64) == 0
    assert lib.sv_conv_wgrad_bf16_workspace_bytes(128, 27, 64, 0) == 0


def test_wgrad_bf16_empty_output_needs_no_workspace():
    """V_out = 0 has no pairs: the checks above still run, nothing is launched for accumulate = 1 (dW stays as it is)"""
    lib = _lib()
    rc = lib.sv_conv_wgrad_bf16(None, 0, 64, 64, None, 0, 64, 64, 27, FAKE, FAKE, FAKE, 0, 1, None, 0, FAKE, None)
    assert rc == 0


def _robotnet():
    import torch

    from mrcc_amd import nn as svnn
    from mrcc_amd.model.robotnet_segmentation import RobotNetSegmentation

    torch.manual_seed(0)
    model = RobotNetSegmentation(in_channels=3, num_classes=3)
    layers = {n: m for n, m in model.named_modules() if isinstance(m, (svnn._ConvBase, svnn.MinkowskiLinear))}
    return model, layers


def test_set_training_precision_marks_the_layers_set_compute_precision_marks():
    import torch

    from mrcc_amd import nn as svnn

    model, layers = _robotnet()
    assert len(layers) == 51
    assert all(m.training_precision == "fp32" for m in layers.values())
    before = {k: v.clone() for k, v in model.state_dict().items()}

    marked = svnn.set_training_precision(model, "bf16")
    assert len(marked) == 41
    for n, m in layers.items():
        assert m.training_precision == ("bf16" if n in marked else "fp32"), n
        assert m.compute_precision == "fp32", n  # the eval switch is untouched
    after = model.state_dict()
    assert list(after) == list(before)
    assert all(torch.equal(after[k], before[k]) for k in before)

    other, _ = _robotnet()
    assert svnn.set_compute_precision(other, "bf16") == marked

    assert len(svnn.set_training_precision(model, "fp32")) == 51
    assert all(m.training_precision == "fp32" for m in layers.values())
    for bad in ("fp16", "BF16", None, "tf32"):
        with pytest.raises(ValueError):
            svnn.set_training_precision(model, bad)
    assert all(m.training_precision == "fp32" for m in layers.values())


def test_set_compute_precision_leaves_training_precision_at_fp32():
    from mrcc_amd import nn as svnn

    model, layers = _robotnet()
    assert len(svnn.set_compute_precision(model, "bf16")) == 41
    assert all(m.training_precision == "fp32" for m in layers.values())
    assert len(svnn.set_training_precision(model, "bf16")) == 41
    assert len(svnn.set_compute_precision(model, "fp32")) == 51
    assert sum(m.training_precision == "bf16" for m in layers.values()) == 41
