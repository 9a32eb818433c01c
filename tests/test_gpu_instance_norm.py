"""sv_instance_norm / sv_instance_norm_backward (include/sv_hip.h, block N8) against float64 restatements.

Forward bound: |got - want| <= 2^-23 |want| + 1e-12 - one fp32 rounding of the float64 result plus float64 summation-order
noise (numpy's pairwise sum is not the kernel's tree).  Backward: float64 torch autograd of the same formula at
1e-4 * max|want| per tensor (REL_TOL of tests/test_gpu_training.py); identical bits across two calls."""
import numpy as np
import pytest

import strided_helpers as H

pytestmark = pytest.mark.gpu

CHUNK = 256  # SV_NORM_CHUNK_ROWS: the frame sizes below straddle it
NONE, RELU, GELU = 0, 1, 3
EPS = 1e-8
REL_TOL = 1e-4
# B = 3, the empty frame first, in the middle, last; every size of 0, 1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 3 CHUNK + 5 occurs
FRAMES = [(0, 1, 2), (CHUNK - 1, 0, CHUNK), (CHUNK + 1, 3 * CHUNK + 5, 0), (0, CHUNK, 1), (2, 0, 3 * CHUNK + 5)]


def test_chunk_constant_is_the_headers():
    import mrcc_amd

    assert mrcc_amd._lib.SV_NORM_CHUNK_ROWS == CHUNK


def _case(sizes, C, seed):
    rng = np.random.default_rng(seed)
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    V = int(starts[-1])
    # per-(frame, channel) offsets and scales well away from 0 / 1: the mean matters, the variance differs by channel
    x = (rng.standard_normal((V, C)) * rng.uniform(0.1, 5.0, size=C) + rng.uniform(-10, 10, size=C)).astype(np.float32)
    x[:, 0] = np.float32(3.25)  # a constant channel: var = 0, the output is act(bias)
    w = rng.uniform(0.5, 2.0, size=C).astype(np.float32) * rng.choice([-1.0, 1.0], size=C).astype(np.float32)
    b = rng.uniform(-1.0, 1.0, size=C).astype(np.float32)
    return x, starts, w, b


@pytest.mark.parametrize("act", [NONE, RELU, GELU])
@pytest.mark.parametrize("C", [1, 64, 65])
@pytest.mark.parametrize("sizes", FRAMES)
def test_instance_norm_forward(gpu, sizes, C, act):
    import torch

    x, starts, w, b = _case(sizes, C, seed=C + 7 * act)
    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    y, mean, inv_std = H.gpu_instance_norm(t(x).reshape(-1, C), t(starts), t(w), t(b), EPS, act)
    want = H.instance_norm_ref(x, starts, w, b, EPS, act)
    got = y.cpu().numpy().astype(np.float64)
    err = np.abs(got - want)
    bound = 2.0 ** -23 * np.abs(want) + 1e-12
    print(f"instance norm sizes={sizes} C={C} act={act}: max err / bound = {(err / bound).max() if err.size else 0.0:.3f}")
    assert (err <= bound).all()
    # the constant channel is exactly act(bias); a frame of one row gives act(bias) in every channel
    want_b = H.instance_norm_ref(np.zeros((1, C), np.float32), np.array([0, 1], np.int32), w, b, EPS, act)[0].astype(np.float32)
    assert np.array_equal(y.cpu().numpy()[:, 0], np.full(len(x), want_b[0]))
    for f, n in enumerate(sizes):
        if n == 1:
            assert np.array_equal(y.cpu().numpy()[starts[f]], want_b)
        if n == 0:  # nothing to normalise: the statistics of an empty frame are written as zeros
            assert (mean[f] == 0).all() and (inv_std[f] == 0).all()
    again, _, _ = H.gpu_instance_norm(t(x).reshape(-1, C), t(starts), t(w), t(b), EPS, act)
    assert torch.equal(y, again)


def _torch_ref(x, starts, w, b, act, dy):
    """float64 torch autograd of the definition -> (dx, dweight, dbias)"""
    import torch

    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    wt = torch.from_numpy(w.astype(np.float64)).requires_grad_(True)
    bt = torch.from_numpy(b.astype(np.float64)).requires_grad_(True)
    parts = []
    for f in range(len(starts) - 1):
        seg = xt[starts[f]:starts[f + 1]]
        if seg.shape[0] == 0:
            continue
        mean = seg.mean(0)
        var = ((seg - mean) ** 2).mean(0)
        parts.append((seg - mean) / torch.sqrt(var + EPS) * wt + bt)
    y = torch.cat(parts)
    if act == RELU:
        y = torch.relu(y)
    elif act == GELU:
        y = torch.nn.functional.gelu(y)
    (y * torch.from_numpy(dy.astype(np.float64))).sum().backward()
    return xt.grad.numpy(), wt.grad.numpy(), bt.grad.numpy()


@pytest.mark.parametrize("act", [NONE, RELU, GELU])
@pytest.mark.parametrize("C", [1, 64, 65])
@pytest.mark.parametrize("sizes", FRAMES[1:])
def test_instance_norm_backward(gpu, sizes, C, act):
    """through the autograd Function the modules use (nn.InstanceNormFunction)"""
    import torch

    from mrcc_amd import nn as svnn

    x, starts, w, b = _case(sizes, C, seed=100 + C + 7 * act)
    x[:, 0] = np.random.default_rng(1).standard_normal(len(x)).astype(np.float32)  # var = 0 amplifies by 1 / sqrt(eps): not here
    dy = np.random.default_rng(2).standard_normal(x.shape).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    grads = []
    for _ in range(2):
        xt, wt, bt = t(x).requires_grad_(True), t(w).reshape(1, C).requires_grad_(True), t(b).reshape(1, C).requires_grad_(True)
        y = svnn.InstanceNormFunction.apply(xt, wt, bt, t(starts), len(sizes), EPS, act)
        y.backward(t(dy))
        grads.append((xt.grad, wt.grad, bt.grad))
    assert all(torch.equal(a, c) for a, c in zip(*grads))  # identical bits: fixed summation tree, no atomics
    assert grads[0][1].shape == (1, C) and grads[0][2].shape == (1, C)
    want = _torch_ref(x, starts, w, b, act, dy)
    for name, got, ref in zip(("dx", "dweight", "dbias"), grads[0], want):
        got = got.cpu().numpy().reshape(ref.shape).astype(np.float64)
        err, scale = np.abs(got - ref).max(), np.abs(ref).max()
        print(f"instance norm backward sizes={sizes} C={C} act={act} {name}: err {err:.3e} of max {scale:.3e}")
        assert err <= REL_TOL * scale, name


def test_instance_norm_module(gpu):
    """MinkowskiInstanceNorm on a two-frame sparse tensor: state-dict keys, parameter shapes, the frames are the tensor's"""
    import torch

    from mrcc_amd import MinkowskiEngine as ME

    rng = np.random.default_rng(3)
    pts = np.concatenate([np.concatenate([np.full((n, 1), b), H.blob_cloud(rng, n, [(0, 0, 0)], 5.0, (-30,) * 3, (30,) * 3)], 1)
                          for b, n in ((0, 300), (1, 41))])
    feats = rng.standard_normal((len(pts), 5)).astype(np.float32)
    x = ME.SparseTensor(torch.from_numpy(feats), coordinates=torch.from_numpy(pts.astype(np.int32)), device=gpu)
    m = ME.MinkowskiInstanceNorm(5).to(gpu).eval()
    assert list(m.state_dict()) == ["weight", "bias"] and m.weight.shape == (1, 5) and m.bias.shape == (1, 5)
    with torch.no_grad():
        m.weight.copy_(torch.tensor([[1.5, -0.5, 2.0, 1.0, 0.25]]))
        m.bias.copy_(torch.tensor([[0.1, 0.2, -0.3, 0.0, 1.0]]))
        y = m(x)
        yg = m.forward_fused(x, act=GELU)
    assert y.tensor_stride == 1 and y.coordinate_manager is x.coordinate_manager
    starts = np.array([0, 300, 341], np.int32)
    xf = x.F.cpu().numpy()
    w, b = m.weight.detach().cpu().numpy()[0], m.bias.detach().cpu().numpy()[0]
    for got, act in ((y, NONE), (yg, GELU)):
        want = H.instance_norm_ref(xf, starts, w, b, EPS, act)
        assert (np.abs(got.F.cpu().numpy() - want) <= 2.0 ** -23 * np.abs(want) + 1e-12).all()
    assert torch.equal(ME.MinkowskiGELU()(x).F, torch.nn.functional.gelu(x.F))
    drop = ME.MinkowskiDropout()
    assert drop.p == 0.5 and drop.eval()(x) is x
    torch.manual_seed(0)
    d = drop.train()(x).F
    assert ((d == 0) | (d == 2 * x.F)).all() and 0.3 < (d == 0).float().mean() < 0.7
