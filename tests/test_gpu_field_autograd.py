"""Gradients through the field front end in train(): TensorField.sparse() -> SparseTensor.cat_slice -> a field network
(Sinusoidal, BN with batch statistics, ReLU, Linear, BN, ReLU, per-voxel mean), against float64 autograd of a restatement.
The mean's backward is a slice divided by the count and the slice's backward a sequential per-voxel sum (sv_voxel_reduce,
SV_REDUCE_SUM): no atomics, so two backward passes give the same bits.  Tolerance: 1e-4 * max|want| per tensor."""
import numpy as np
import pytest
import torch

import field_helpers as FH

pytestmark = pytest.mark.gpu

REL_TOL = 1e-4


def _network(gpu):
    from mrcc_amd import MinkowskiEngine as ME

    torch.manual_seed(31)
    net = torch.nn.Sequential(ME.MinkowskiSinusoidal(6, 32), ME.MinkowskiBatchNorm(32), ME.MinkowskiReLU(inplace=True),
                              ME.MinkowskiLinear(32, 32), ME.MinkowskiBatchNorm(32), ME.MinkowskiReLU(inplace=True),
                              ME.MinkowskiToSparseTensor())
    g = torch.Generator().manual_seed(32)
    with torch.no_grad():
        for i in (1, 4):
            net[i].bn.weight.copy_(torch.rand(32, generator=g) + 0.5)
            net[i].bn.bias.copy_(torch.randn(32, generator=g) * 0.2)
    return net.to(gpu).train()


def _reference(F, inverse, V, params, gw):
    """float64: voxel mean -> [mean of the point's voxel, the point's own features] -> the network -> voxel mean"""
    import torch.nn.functional as fn

    F = F.double().requires_grad_(True)
    p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in params.items()}
    rows = torch.cat([FH.voxel_mean_ref(F, inverse, V)[inverse], F], 1)
    h = p["0.coef"] * torch.sin(rows @ p["0.kernel"] + p["0.bias"])
    h = torch.relu(fn.batch_norm(h, None, None, p["1.bn.weight"], p["1.bn.bias"], training=True, eps=1e-5))
    h = h @ p["3.linear.weight"].t() + p["3.linear.bias"]
    h = torch.relu(fn.batch_norm(h, None, None, p["4.bn.weight"], p["4.bn.bias"], training=True, eps=1e-5))
    out = FH.voxel_mean_ref(h, inverse, V)
    (out * gw.double()).sum().backward()
    return out.detach(), F.grad, {k: v.grad for k, v in p.items()}


def _run(gpu, net, pts, F, gw):
    from mrcc_amd import MinkowskiEngine as ME

    for q in net.parameters():
        q.grad = None
    feats = F.clone().to(gpu).requires_grad_(True)
    field = ME.TensorField(feats, torch.from_numpy(pts.astype(np.float32) + np.float32(0.5)), device=gpu)
    assert field.F is feats  # the leaf itself: its .grad is the field features' gradient
    voxels = field.sparse()
    out = net(voxels.cat_slice(field))
    assert out.coordinate_manager is voxels.coordinate_manager
    (out.F * gw.to(gpu)).sum().backward()
    return out.F.detach().cpu(), feats.grad.cpu(), {k: q.grad.cpu() for k, q in net.named_parameters()}


def test_gradients_match_float64_autograd_and_repeat_bit_for_bit(gpu):
    pts = FH.stage_cloud()
    inverse, V = FH.voxelize_ref(pts)
    g = torch.Generator().manual_seed(33)
    F = torch.randn(len(pts), 3, generator=g)
    gw = torch.randn(V, 32, generator=g)
    net = _network(gpu)
    params = dict(net.named_parameters())
    want_out, want_dF, want_dp = _reference(F, inverse, V, params, gw)
    stats = [b.clone() for b in net.buffers()]
    out, dF, dp = _run(gpu, net, pts, F, gw)
    assert float((out.double() - want_out).abs().max() / want_out.abs().max()) <= REL_TOL
    assert set(dp) == set(want_dp)
    for name, got, want in [("field features", dF, want_dF)] + [(k, dp[k], want_dp[k]) for k in sorted(dp)]:
        scale = want.abs().max()
        if name == "3.linear.bias":
            # a bias in front of a batch norm with batch statistics has NO gradient: the reference is exactly zero (float64
            # autograd gives its own rounding noise, 1e-15, checked here and then replaced by the zero).  The bias gradient is
            # the column sum of the gradient whose products with the layer's inputs sum to the weight gradient, so that
            # tensor's scale is the one the tolerance is taken from: |got| <= 1e-4 * max|d weight|.
            scale = want_dp["3.linear.weight"].abs().max()
            assert float(want.abs().max()) <= 1e-9 * float(scale)
            want = torch.zeros_like(want)
        err = float((got.double() - want).abs().max() / scale)
        print(f"field front end gradient {name}: error = {err:.3e}")
        assert err <= REL_TOL, name
    with torch.no_grad():  # the same starting point: train() moved the running statistics
        for b, s in zip(net.buffers(), stats):
            b.copy_(s)
    out2, dF2, dp2 = _run(gpu, net, pts, F, gw)
    assert torch.equal(FH.bits(out2), FH.bits(out)) and torch.equal(FH.bits(dF2), FH.bits(dF))
    for k in dp:
        assert torch.equal(FH.bits(dp2[k]), FH.bits(dp[k])), k


def test_nothing_differentiable_runs_without_a_graph(gpu):
    """features without a graph: sparse() and slice launch what they always launched (one reduce, one slice)"""
    import hostile_helpers as HH
    from mrcc_amd import MinkowskiEngine as ME

    pts = FH.stage_cloud()
    F = torch.randn(len(pts), 3)
    field = ME.TensorField(F, torch.from_numpy(pts.astype(np.float32)), device=gpu)
    with HH.entry_calls() as calls:
        st = field.sparse()
        st.slice(field)
        st.cat_slice(field)
    assert not st.F.requires_grad
    assert (calls["sv_voxelize"], calls["sv_voxel_reduce"], calls["sv_slice_rows"]) == (1, 1, 2)
