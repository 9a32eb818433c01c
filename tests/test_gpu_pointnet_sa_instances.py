"""The fused set abstraction (csrc/sv_pointnet.hip: sv_pointnet_sa, sv_pointnet_sa_msg) at every pn_layer<MR, NT>
instance, as an inner and as the last (pooling) layer, at the edges of the k-loop, at the widest layer, on both sides of
the 160 KiB LDS limit and at SV_PN_MAX_LAYERS / SV_PN_MAX_SCALES - bit for bit against the unfused eval path on the same
groups (sv_conv_fwd dense rows, torch.max, torch.cat).  The module falls back to the unfused path when the kernel
declines, so every case also proves which path ran: a spy on `_fused` (None = declined) or the entry's return code.

pn_layer_any: NT = 2 when cout % 32 == 0 else 1; MR = 1 / 2 / 4 for 1 / 2-3 / >= 4 column groups of 16 * NT channels:
16 -> <1,1>, 48 -> <2,1>, 80 -> <4,1>, 32 -> <1,2>, 96 -> <2,2>, 160 -> <4,2>.
Clouds are small: B = 1, N = 200, S = 5 centroids - the last workgroup of nsample 16 (4 centroids each) and 32 (2 each) is
partly filled."""
from ctypes import c_int, c_void_p

import pytest
import torch

pytestmark = pytest.mark.gpu

N, S, RADIUS = 200, 5, 0.35
LDS_MAX = 160 * 1024


@pytest.fixture(scope="module")
def P2(gpu):
    from mrcc_amd.model import pointnet2_utils

    return pointnet2_utils


def _randomize(model, seed):
    """conv weights ~ N(0, 1/fan_in), BatchNorm affine and running statistics random (torch generator, CPU): the recipe
    of tests/test_gpu_pointnet2.py"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (torch.nn.Conv1d, torch.nn.Conv2d)):
                fan_in = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / fan_in ** 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            elif isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                n = m.num_features
                m.weight.copy_(torch.rand(n, generator=g) * 0.5 + 0.75)
                m.bias.copy_(torch.randn(n, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(n, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(n, generator=g) * 0.5 + 0.75)


def _cloud(gpu, D, seed):
    g = torch.Generator().manual_seed(seed)
    xyz = ((torch.rand(1, 3, N, generator=g) - 0.5) * 0.8).to(gpu)
    pts = torch.randn(1, D, N, generator=g).to(gpu) if D else None
    return xyz, pts, torch.zeros(1, dtype=torch.int64, device=gpu)  # the first centroid is point 0


def _ssg(P2, gpu, D, mlp, nsample, seed=1):
    sa = P2.PointNetSetAbstraction(S, RADIUS, nsample, 3 + D, list(mlp), False)
    _randomize(sa, seed)
    return sa.to(gpu).eval()


def _msg(P2, gpu, D, mlps, nsamples, seed=2):
    radii = [RADIUS * (0.8 + 0.1 * r) for r in range(len(mlps))]
    sa = P2.PointNetSetAbstractionMsg(S, radii, list(nsamples), D, [list(m) for m in mlps])
    _randomize(sa, seed)
    return sa.to(gpu).eval()


def _same(a, b):
    """bit-for-bit equal values (the sign of zero counts), NaN where the other has NaN"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return (a.shape == b.shape and torch.equal(na, nb)
            and torch.equal(a[~na].contiguous().view(torch.int32), b[~nb].contiguous().view(torch.int32)))


def _run(sa, xyz, pts, start):
    """(fused-path output, unfused-path output, whether the fused kernel ran) - the module's forward twice, with a spy
    on `_fused` that records what the kernel wrapper returned (None: SV_ERR_UNSUPPORTED, nothing launched)"""
    returned = []
    fused = sa._fused

    def spy(*args, **kwargs):
        out = fused(*args, **kwargs)
        returned.append(out)
        return out

    sa._fused = spy
    try:
        with torch.no_grad():
            sa.fused = True
            nx, got = sa(xyz, pts, fps_start=start)
            assert len(returned) == 1
            sa.fused = False
            nx2, want = sa(xyz, pts, fps_start=start)
            assert len(returned) == 1  # the unfused forward does not reach the kernel
    finally:
        del sa._fused
        sa.fused = True
    assert torch.equal(nx, nx2)
    ran = returned[0] is not None
    if ran:
        assert returned[0].data_ptr() == got.data_ptr()  # the module returned the kernel's buffer
    return got, want, ran


def _runs_and_matches(sa, xyz, pts, start):
    got, want, ran = _run(sa, xyz, pts, start)
    assert ran, "the fused kernel declined"
    assert not torch.isnan(want).any() and (want > 0).any()
    assert _same(got, want), int((got != want).sum())
    return got


def _declines(sa, xyz, pts, start):
    got, want, ran = _run(sa, xyz, pts, start)
    assert not ran, "the fused kernel ran"
    assert _same(got, want)


# ---- 1. every pn_layer instance, last and inner ----------------------------------------------------------------------
WIDTHS = [16, 48, 80, 32, 96, 160]


@pytest.mark.parametrize("nsample", [16, 64])
@pytest.mark.parametrize("width", WIDTHS)
def test_every_instance_as_the_only_layer(P2, gpu, width, nsample):
    xyz, pts, start = _cloud(gpu, 3, width)
    got = _runs_and_matches(_ssg(P2, gpu, 3, [width], nsample), xyz, pts, start)
    assert got.shape == (1, width, S)


@pytest.mark.parametrize("nsample", [16, 64])
@pytest.mark.parametrize("width", WIDTHS)
def test_every_instance_as_the_middle_layer(P2, gpu, width, nsample):
    xyz, pts, start = _cloud(gpu, 3, width + 1)
    _runs_and_matches(_ssg(P2, gpu, 3, [32, width, 48], nsample), xyz, pts, start)


def test_four_layers_run_and_five_decline(P2, gpu):
    from mrcc_amd._lib import SV_PN_MAX_LAYERS

    assert SV_PN_MAX_LAYERS == 4
    xyz, pts, start = _cloud(gpu, 3, 7)
    _runs_and_matches(_ssg(P2, gpu, 3, [16, 80, 48, 160], 32), xyz, pts, start)
    _declines(_ssg(P2, gpu, 3, [16, 80, 48, 160, 32], 32), xyz, pts, start)


# ---- 2. input widths around the 16-wide k-round -----------------------------------------------------------------------
@pytest.mark.parametrize("first", [32, 80])
@pytest.mark.parametrize("D", [0, 1, 12, 13, 14, 17, 29])
def test_input_width_edges(P2, gpu, D, first):
    """cin = 3 + D = 3, 4, 15, 16, 17, 20, 32: below one 4-wide step, exactly one, one to three channels short of the
    16-wide round, exactly on it, just past it, a round and a step, two rounds - single-scale and two scales"""
    xyz, pts, start = _cloud(gpu, D, 10 * D + first)
    _runs_and_matches(_ssg(P2, gpu, D, [first, 48], 32), xyz, pts, start)
    _runs_and_matches(_msg(P2, gpu, D, [[first, 48], [first, 32]], [16, 128]), xyz, pts, start)


# ---- 3. the widest layer ---------------------------------------------------------------------------------------------
def test_width_1024_runs_and_wider_or_narrower_declines(P2, gpu):
    xyz, pts, start = _cloud(gpu, 3, 11)
    got = _runs_and_matches(_ssg(P2, gpu, 3, [64, 1024], 16), xyz, pts, start)
    assert got.shape == (1, 1024, S)
    _declines(_ssg(P2, gpu, 3, [64, 1040], 16), xyz, pts, start)
    _declines(_ssg(P2, gpu, 3, [8], 16), xyz, pts, start)
    _declines(_ssg(P2, gpu, 3, [64, 8], 16), xyz, pts, start)


# ---- 4. the LDS limit ------------------------------------------------------------------------------------------------
def _lds_bytes(widths, nsample):
    """the documented plan: two buffers of 64 rows whose row stride is the smallest 4 * odd >= the width; buffer 0 holds
    the gathered input and the outputs of layers 1, 3, buffer 1 those of layers 0, 2; the last layer's 4 * C_last partial
    maxima go to the buffer it does not read; nsample 128 adds C_last running maxima"""
    def stride(c):
        s = (c + 3) // 4
        return 4 * (s if s % 2 else s + 1)

    nlayers = len(widths) - 1
    need = [64 * stride(widths[0]), 0]
    for layer in range(nlayers):
        out = 64 * stride(widths[layer + 1]) if layer + 1 < nlayers else 4 * widths[-1]
        need[(layer + 1) & 1] = max(need[(layer + 1) & 1], out)
    return 4 * (need[0] + need[1] + (widths[-1] if nsample == 128 else 0))


def test_lds_limit_from_both_sides(P2, gpu):
    xyz, pts, start = _cloud(gpu, 3, 12)
    assert _lds_bytes([6, 624, 16], 64) == 163840 == LDS_MAX
    _runs_and_matches(_ssg(P2, gpu, 3, [624, 16], 64), xyz, pts, start)
    assert _lds_bytes([6, 640, 16], 64) == 167936
    _declines(_ssg(P2, gpu, 3, [640, 16], 64), xyz, pts, start)
    # the multi-scale entry: the same plan, plus the running maxima of a two-pass ball
    _runs_and_matches(_msg(P2, gpu, 3, [[624, 16]], [64]), xyz, pts, start)
    assert _lds_bytes([6, 624, 16], 128) == LDS_MAX + 4 * 16
    _declines(_msg(P2, gpu, 3, [[624, 16]], [128]), xyz, pts, start)
    assert _lds_bytes([6, 608, 16], 128) == 159808 <= LDS_MAX
    _runs_and_matches(_msg(P2, gpu, 3, [[608, 16]], [128]), xyz, pts, start)


# ---- 5. four scales --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [0, 3])
def test_four_scales_and_nothing_past_the_output(P2, gpu, D):
    from mrcc_amd._lib import SV_ERR_UNSUPPORTED, SV_PN_MAX_SCALES, load, ptr, stream_ptr

    assert SV_PN_MAX_SCALES == 4
    mlps, nsamples = [[32, 16], [32, 80], [48, 32], [64, 96]], [16, 32, 64, 128]
    xyz, pts, start = _cloud(gpu, D, 13 + D)
    sa = _msg(P2, gpu, D, mlps, nsamples)
    got = want = _runs_and_matches(sa, xyz, pts, start)  # the unfused path's bits, no NaN
    ctot = 16 + 80 + 32 + 96
    assert got.shape == (1, ctot, S)
    # the entry alone, into a guarded buffer
    x = xyz.permute(0, 2, 1).contiguous()
    p = pts.permute(0, 2, 1).contiguous() if D else None
    nx = P2.index_points(x, P2.farthest_point_sample(x, S, start=start)).contiguous()
    idxs = P2.query_ball_point_multi(sa.radius_list, sa.nsample_list, x, nx)
    _, _, (ns, params, widths, nlayers) = sa._folded()
    out = torch.full((S + 4, ctot), -3.0, device=gpu)
    tables = (c_void_p * 4)(*[t.data_ptr() for t in idxs])
    rc = load().sv_pointnet_sa_msg(ptr(x), ptr(p), ptr(nx), 1, N, D, S, 4, ns, tables, params, widths, nlayers, ptr(out),
                                   stream_ptr())
    assert rc == 0
    assert _same(out[:S].t()[None].contiguous(), want.contiguous())
    assert (out[S:] == -3.0).all()
    # a fifth scale: declined by the entry (nothing launched) and by the module
    five = (c_void_p * 5)(*[t.data_ptr() for t in idxs], idxs[0].data_ptr())
    rc = load().sv_pointnet_sa_msg(ptr(x), ptr(p), ptr(nx), 1, N, D, S, 5, (c_int * 5)(*ns, 16), five,
                                   (c_void_p * 5)(*params, params[0]), (c_int * 15)(*widths, *list(widths)[:3]),
                                   (c_int * 5)(*nlayers, 2), ptr(out), stream_ptr())
    assert rc == SV_ERR_UNSUPPORTED
    assert (out[S:] == -3.0).all() and _same(out[:S].t()[None].contiguous(), want.contiguous())
    _declines(_msg(P2, gpu, D, mlps + [[32, 16]], nsamples + [16]), xyz, pts, start)


# ---- 6. NaN through the new instances --------------------------------------------------------------------------------
@pytest.mark.parametrize("nsample", [16, 128])
@pytest.mark.parametrize("last", [16, 80])
def test_nan_reaches_its_centroids_only(P2, gpu, last, nsample):
    """a NaN feature on point 0, which is the first centroid (in its own ball, so that centroid is NaN); the farthest
    point from it is the second centroid, out of the NaN point's reach: the same NaN pattern as the unfused path"""
    xyz, pts, start = _cloud(gpu, 3, 14 + last)
    pts = pts.clone()
    pts[0, 1, 0] = float("nan")
    runs = [_msg(P2, gpu, 3, [[32, last]], [nsample])]
    if nsample <= 64:
        runs.append(_ssg(P2, gpu, 3, [32, last], nsample))
    for sa in runs:
        got, want, ran = _run(sa, xyz, pts, start)
        assert ran
        nan_centroid = torch.isnan(got[0]).all(dim=0)
        assert torch.equal(nan_centroid, torch.isnan(got[0]).any(dim=0))  # a NaN row reaches every channel
        assert nan_centroid[0] and nan_centroid.any() and not nan_centroid.all()
        assert _same(got, want)
