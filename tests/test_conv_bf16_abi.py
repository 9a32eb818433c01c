"""bf16 conv path without a GPU: argument checks of sv_pack_weights_bf16 / sv_conv_fwd_bf16 (host code, no launch) and
nn.set_compute_precision on a CPU-built RobotNetSegmentation(MinkUNet18D)."""
import ctypes

import pytest


def _conv(lib, Cin, Cout, K=27, V_out=10):
    # (in, V_in, in_ld, Cin, Wp, K, Cout, perm, nbr_s, submask, tile_order, V_out, Vpad, acc_init, acc_ld, scale, shift,
    #  residual, res_ld, act, slope, out, out_ld, stream)
    return lib.sv_conv_fwd_bf16(None, 10, Cin, Cin, None, K, Cout, None, None, None, None, V_out, 128, None, 0, None, None,
                                None, 0, 0, ctypes.c_float(0.0), None, Cout, None)


def test_conv_bf16_argument_checks_without_gpu():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    unsupported = mrcc_amd._lib.SV_ERR_UNSUPPORTED
    for K in (1, 8, 27):
        rc = _conv(lib, 384, 384, K)
        assert rc == -1 and b"null pointer" in lib.sv_last_error()
    rc = _conv(lib, 256, 1024, 1)
    assert rc == -1 and b"null pointer" in lib.sv_last_error()
    # shapes the bf16 kernel does not cover: SV_ERR_UNSUPPORTED before any pointer is looked at
    for cin, cout in ((48, 384), (32, 64), (3, 32), (384, 4)):
        rc = _conv(lib, cin, cout)
        assert rc == unsupported, (cin, cout, rc)
        assert b"sv_conv_fwd_bf16" in lib.sv_last_error() and b"Cin" in lib.sv_last_error()
    rc = _conv(lib, 384, 384, 28)
    assert rc == unsupported and b"kernel volume" in lib.sv_last_error()
    # plan / stride checks after the shape checks
    rc = lib.sv_conv_fwd_bf16(None, 10, 384, 384, None, 27, 384, None, None, None, None, 10, 100, None, 0, None, None,
                              None, 0, 0, ctypes.c_float(0.0), None, 384, None)
    assert rc == -1 and b"multiple of 128" in lib.sv_last_error()
    # V_out = 0: nothing to do
    assert _conv(lib, 384, 384, 27, V_out=0) == 0


def test_pack_weights_bf16_argument_checks_without_gpu():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    rc = lib.sv_pack_weights_bf16(None, 27, 384, 384, None, None)
    assert rc == -1 and b"null pointer" in lib.sv_last_error()
    rc = lib.sv_pack_weights_bf16(None, 27, 48, 384, None, None)
    assert rc == mrcc_amd._lib.SV_ERR_UNSUPPORTED and b"Cin" in lib.sv_last_error()
    rc = lib.sv_pack_weights_bf16(None, 0, 64, 64, None, None)
    assert rc == -1 and b"kernel volume" in lib.sv_last_error()


FP32_LAYERS = {"conv0p1s1", "conv1p1s2", "conv2p2s2", "block1.0.conv1", "block1.0.conv2", "block1.1.conv1",
               "block1.1.conv2", "block2.0.conv1", "block2.0.downsample.0", "regression.2"}


def test_set_compute_precision_marks_the_wide_layers():
    import torch

    from mrcc_amd import nn as svnn
    from mrcc_amd.model.robotnet_segmentation import RobotNetSegmentation

    torch.manual_seed(0)
    model = RobotNetSegmentation(in_channels=3, num_classes=3)
    layers = {n: m for n, m in model.named_modules() if isinstance(m, (svnn._ConvBase, svnn.MinkowskiLinear))}
    assert len(layers) == 51
    assert all(m.compute_precision == "fp32" for m in layers.values())
    before = {k: v.clone() for k, v in model.state_dict().items()}

    marked = svnn.set_compute_precision(model, "bf16")
    assert len(marked) == 41 and set(marked) == set(layers) - FP32_LAYERS
    assert {"final", "regression.0", "block8.1.conv2", "convtr7p2s2", "conv3p4s2"} <= set(marked)
    for n, m in layers.items():
        assert m.compute_precision == ("fp32" if n in FP32_LAYERS else "bf16"), n
    after = model.state_dict()
    assert list(after) == list(before)
    assert all(torch.equal(after[k], before[k]) for k in before)

    assert len(svnn.set_compute_precision(model, "fp32")) == 51
    assert all(m.compute_precision == "fp32" for m in layers.values())
    for bad in ("fp16", "BF16", None):
        with pytest.raises(ValueError):
            svnn.set_compute_precision(model, bad)
    assert all(m.compute_precision == "fp32" for m in layers.values())
