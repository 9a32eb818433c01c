"""Argument checks of the multi-scale grouping entries (sv_ball_query_multi, sv_pointnet_sa_msg): host code, no launch,
no GPU."""
import ctypes

# PointNet2MSGEncoder's two multi-scale layers: (D, nsamples, per-scale widths)
SA1 = (3, [16, 32, 128], [[6, 32, 32, 64], [6, 64, 64, 128], [6, 64, 96, 128]])
SA2 = (320, [32, 64, 128], [[323, 64, 64, 128], [323, 128, 128, 256], [323, 128, 128, 256]])


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def _msg(lib, B=1, N=2048, D=3, S=512, nsamples=(16, 32, 128), widths=None, nlayers=None, R=None):
    """sv_pointnet_sa_msg with host arrays in place and every device pointer NULL"""
    widths = widths if widths is not None else [[3 + D, 32, 32, 64]] * len(nsamples)
    R = len(nsamples) if R is None else R
    flat = [w for ws in widths for w in ws]
    nl = nlayers if nlayers is not None else [len(ws) - 1 for ws in widths]
    idx = (ctypes.c_void_p * max(R, 1))()
    params = (ctypes.c_void_p * max(R, 1))()
    return lib.sv_pointnet_sa_msg(None, None, None, B, N, D, S, R, _ints(*nsamples), idx, params, _ints(*flat),
                                  _ints(*nl), None, None)


def test_pointnet_sa_msg_argument_checks_without_gpu():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    unsupported = mrcc_amd._lib.SV_ERR_UNSUPPORTED
    # both encoder layers fit (sa2's 323 -> 128 -> 128 -> 256 scale is the largest): only the device pointers are missing
    for D, ns, ws in (SA1, SA2):
        rc = _msg(lib, D=D, nsamples=ns, widths=ws)
        assert rc == -1 and b"null pointer" in lib.sv_last_error()
    # D = 0 (points NULL, normal_channel False)
    rc = _msg(lib, D=0, nsamples=[16, 32, 128], widths=[[3, 32, 32, 64], [3, 64, 64, 128], [3, 64, 96, 128]])
    assert rc == -1 and b"null pointer" in lib.sv_last_error()
    # NULL host arrays
    rc = lib.sv_pointnet_sa_msg(None, None, None, 1, 2048, 3, 512, 1, None, None, None, None, None, None, None)
    assert rc == -1 and b"null pointer" in lib.sv_last_error()
    # bad shapes
    for B, N, D, S in ((-1, 2048, 3, 512), (1, 0, 3, 512), (1, 2048, -1, 512), (1, 2048, 3, 0)):
        rc = _msg(lib, B=B, N=N, D=D, S=S, nsamples=[16], widths=[[6, 32]])
        assert rc == -1 and b"bad shape" in lib.sv_last_error()
    # widths[0] of a scale must be 3 + D
    rc = _msg(lib, D=3, nsamples=[16, 32], widths=[[6, 32], [5, 32]])
    assert rc == -1 and b"3 + D" in lib.sv_last_error()
    # shapes the kernel does not cover: SV_ERR_UNSUPPORTED before any device pointer is looked at
    for ns in (8, 24, 96, 256):
        rc = _msg(lib, nsamples=[16, ns], widths=[[6, 32], [6, 32]])
        assert rc == unsupported and b"nsample" in lib.sv_last_error()
    rc = _msg(lib, nsamples=[16, 32], widths=[[6, 32], [6, 32, 24]])
    assert rc == unsupported and b"multiples of 16" in lib.sv_last_error()
    rc = _msg(lib, nsamples=[16], widths=[[6, 32, 32, 32, 32, 32]])
    assert rc == unsupported and b"layer count" in lib.sv_last_error()
    rc = _msg(lib, nsamples=[16], widths=[[6]], nlayers=[0])
    assert rc == unsupported and b"layer count" in lib.sv_last_error()
    rc = _msg(lib, nsamples=[16] * 5, widths=[[6, 32]] * 5)
    assert rc == unsupported and b"scale count" in lib.sv_last_error()
    rc = _msg(lib, nsamples=[16], widths=[[6, 32]], R=0)
    assert rc == unsupported and b"scale count" in lib.sv_last_error()
    # LDS: 1021 features on the 64-row tile need more than 160 KiB; a 128-neighbour ball also keeps C_last running maxima
    rc = _msg(lib, D=1021, nsamples=[32], widths=[[1024, 1024, 64]])
    assert rc == unsupported and b"LDS" in lib.sv_last_error()
    # one layer 564 -> 1024: 64 x 564 + 4 x 1024 floats fit, the 1024 running maxima of a two-pass ball do not
    rc = _msg(lib, D=561, nsamples=[64], widths=[[564, 1024]])
    assert rc == -1 and b"null pointer" in lib.sv_last_error()
    rc = _msg(lib, D=561, nsamples=[128], widths=[[564, 1024]])
    assert rc == unsupported and b"LDS" in lib.sv_last_error()
    # B = 0: nothing to do
    for D, ns, ws in (SA1, SA2):
        assert _msg(lib, B=0, D=D, nsamples=ns, widths=ws) == 0


def test_ball_query_multi_argument_checks_without_gpu():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    unsupported = mrcc_amd._lib.SV_ERR_UNSUPPORTED

    def bq(B=1, N=2048, S=512, radii=(0.1, 0.2, 0.4), ns=(16, 32, 128), R=None, out=True):
        R = len(radii) if R is None else R
        o = (ctypes.c_void_p * max(R, 1))() if out else None
        return lib.sv_ball_query_multi(None, None, B, N, S, R, (ctypes.c_double * max(len(radii), 1))(*radii),
                                       _ints(*ns), o, None)

    assert bq() == -1 and b"null pointer" in lib.sv_last_error()
    assert bq(out=False) == -1 and b"null pointer" in lib.sv_last_error()
    for B, N, S in ((-1, 2048, 512), (1, 0, 512), (1, 2048, 0)):
        assert bq(B=B, N=N, S=S) == -1 and b"bad shape" in lib.sv_last_error()
    assert bq(ns=(16, 0, 128)) == -1 and b"bad shape" in lib.sv_last_error()
    assert bq(radii=(0.1,) * 5, ns=(16,) * 5) == unsupported and b"radius count" in lib.sv_last_error()
    assert bq(R=0) == unsupported and b"radius count" in lib.sv_last_error()
    assert bq(B=0) == 0


def test_sv_pointnet_sa_contract_unchanged():
    """the single-scale entry still declines nsample 128 (the multi-scale entry is the one that takes it)"""
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    rc = lib.sv_pointnet_sa(None, None, None, None, 1, 2048, 3, 512, 128, None, _ints(6, 64, 96, 128), 3, None, None)
    assert rc == mrcc_amd._lib.SV_ERR_UNSUPPORTED and b"nsample" in lib.sv_last_error()


def test_msg_modules_check_channels_without_gpu():
    """wrong channel counts raise ValueError before anything runs (the reference would fail inside torch)"""
    import pytest
    import torch

    from mrcc_amd.model.pointnet2 import PointNet2MSGEncoder
    from mrcc_amd.model.pointnet2_utils import PointNetSetAbstractionMsg

    net = PointNet2MSGEncoder(7).eval()
    with pytest.raises(ValueError):
        net(torch.zeros(1, 9, 64))  # use_point_normals-style 9 channels into the 6-channel encoder
    with pytest.raises(ValueError):
        PointNet2MSGEncoder(7, normal_channel=False).eval()(torch.zeros(1, 6, 64))
    with pytest.raises(ValueError):
        net.sa2(torch.zeros(1, 3, 64), torch.zeros(1, 300, 64))
    with pytest.raises(ValueError):
        PointNetSetAbstractionMsg(8, [0.1], [16], 0, [[32]])(torch.zeros(1, 3, 64), torch.zeros(1, 3, 64))


# state_dict keys of the three PointNet++ layer modules, in order, as checkpoints of the reference hold them
SA_KEYS = ["mlp_convs.0.weight", "mlp_convs.0.bias", "mlp_convs.1.weight", "mlp_convs.1.bias", "mlp_bns.0.weight",
    "mlp_bns.0.bias", "mlp_bns.0.running_mean", "mlp_bns.0.running_var", "mlp_bns.0.num_batches_tracked",
    "mlp_bns.1.weight", "mlp_bns.1.bias", "mlp_bns.1.running_mean", "mlp_bns.1.running_var",
    "mlp_bns.1.num_batches_tracked"]
MSG_KEYS = ["conv_blocks.0.0.weight", "conv_blocks.0.0.bias", "conv_blocks.0.1.weight", "conv_blocks.0.1.bias",
    "conv_blocks.1.0.weight", "conv_blocks.1.0.bias", "conv_blocks.1.1.weight", "conv_blocks.1.1.bias",
    "conv_blocks.1.2.weight", "conv_blocks.1.2.bias", "bn_blocks.0.0.weight", "bn_blocks.0.0.bias",
    "bn_blocks.0.0.running_mean", "bn_blocks.0.0.running_var", "bn_blocks.0.0.num_batches_tracked",
    "bn_blocks.0.1.weight", "bn_blocks.0.1.bias", "bn_blocks.0.1.running_mean", "bn_blocks.0.1.running_var",
    "bn_blocks.0.1.num_batches_tracked", "bn_blocks.1.0.weight", "bn_blocks.1.0.bias", "bn_blocks.1.0.running_mean",
    "bn_blocks.1.0.running_var", "bn_blocks.1.0.num_batches_tracked", "bn_blocks.1.1.weight", "bn_blocks.1.1.bias",
    "bn_blocks.1.1.running_mean", "bn_blocks.1.1.running_var", "bn_blocks.1.1.num_batches_tracked",
    "bn_blocks.1.2.weight", "bn_blocks.1.2.bias", "bn_blocks.1.2.running_mean", "bn_blocks.1.2.running_var",
    "bn_blocks.1.2.num_batches_tracked"]


def test_layer_modules_keep_their_state_dict_keys_and_training_switch():
    """parameter and buffer names (so checkpoints load by key) of the single-scale, multi-scale and feature-propagation
    layers, and the modules set_training_path switches in a container of the three"""
    import torch

    from mrcc_amd.model import pointnet2_utils as U

    sa = U.PointNetSetAbstraction(32, 0.2, 16, 6, [16, 32], False)
    msg = U.PointNetSetAbstractionMsg(32, [0.1, 0.2], [16, 32], 3, [[16, 32], [16, 16, 32]])
    fp = U.PointNetFeaturePropagation(48, [32, 16])
    assert list(sa.state_dict().keys()) == SA_KEYS
    assert list(msg.state_dict().keys()) == MSG_KEYS
    assert list(fp.state_dict().keys()) == SA_KEYS  # mlp_convs.i / mlp_bns.i, as the single-scale layer
    assert U.set_training_path(torch.nn.ModuleList([sa, msg, fp]), "hip") == ["0", "1", "2"]
