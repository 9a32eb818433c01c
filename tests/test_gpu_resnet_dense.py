"""The classification ResNets (model/backbone/resnet.py) against an independent dense-grid model, in the manner of
tests/test_gpu_dense_grid.py: the same network written with torch's conv3d / max_pool3d on a dense float64 grid, every layer
masked to the active voxel sets.  It shares no code with the HIP path or the oracle, so it pins the DEFINITIONS: a strided
convolution's output set is floor(c / stride) * stride, an odd kernel is centred on the output coordinate (conv3d with
padding 1), the even pooling kernel starts at it (max_pool3d(2, 2)), instance norm is per (frame, channel) with biased
variance and eps = 1e-8.

Geometry.  The network's total tensor stride is 2 * 2 * 2^4 * 3 = 192.  A dense strided conv lands on the sparse output
coordinates only when the grid's origin is a multiple of the output tensor stride, so the grid starts at (-128, -192, -128) -
a multiple of 64, every stride up to layer4's - and the stride-64 tensor gets one empty cell in front of x and z before conv5,
which moves its origin to (-192, -192, -192).  The voxels lie in x, z in [-128, 64) and y in [-192, -128): negative
coordinates on every axis, on a grid of 192 x 64 x 192 cells (a cloud centred on the origin would need 384^3).
conv5's kernel is centred on its output: the output at -192 sees the stride-64 cells -256, -192, -128 and the output at 0 sees
-64, 0, 64, so with this box a frame has up to four stride-192 rows WITH inputs (a row whose cell is occupied only at +128 has
none and is zero).  The set-up asks for at least three such rows per frame.  That is one more than the two rows the instance
norm needs not to be the one-row case, and for a reason: over two rows - or over one live row and zero rows - the
normalised values do not depend on the input at all, the gradient of everything before conv5 is then identically zero, and the
gradient case would compare rounding noise (the float32 dense model itself is then 1e-3 off its float64 gradients).

Bounds.  Logits: relative max-abs error <= max(1e-4, 8 * d32), d32 = the deviation of the SAME dense model evaluated in
float32 from its float64 evaluation (8: headroom for a different summation order; 1e-4: the project's floor).  Gradients:
1e-4 * max|want| per tensor against float64 autograd of the dense model."""
import numpy as np
import pytest

import strided_helpers as H

pytestmark = pytest.mark.gpu

ORIGIN = (-128, -192, -128)
SIZE = (192, 64, 192)
BOX_LO, BOX_HI = (-128, -192, -128), (64, -128, 64)
PAD_192 = (1, 0, 0, 0, 1, 0)  # F.pad of the stride-64 tensor (z, y, x from the back): the origin becomes a multiple of 192
REL_TOL = 1e-4


# ---- the dense model ------------------------------------------------------------------------------------------------
def _dense_w(kernel):
    """[K, Cin, Cout] (k = (dx+1) + 3 (dy+1) + 9 (dz+1), x fastest) -> conv3d weight [Cout, Cin, 3, 3, 3] on (x, y, z) grids"""
    if kernel.dim() == 2:
        return kernel.t()[:, :, None, None, None]
    K, cin, cout = kernel.shape
    return kernel.reshape(3, 3, 3, cin, cout).permute(4, 3, 2, 1, 0)


def _coarsen(mask, s):
    import torch.nn.functional as F

    return F.max_pool3d(mask, s, s, ceil_mode=True)


class Dense:
    """functional dense model over a parameter dict with the sparse model's state-dict names"""

    def __init__(self, params, bottleneck, training):
        self.p, self.bottleneck, self.training = params, bottleneck, training

    def conv(self, name, x, mask, stride=1):
        import torch.nn.functional as F

        w = _dense_w(self.p[name + ".kernel"])
        out_mask = _coarsen(mask, stride) if stride > 1 else mask
        y = F.conv3d(x, w, stride=stride, padding=1 if w.shape[-1] == 3 else 0)
        assert y.shape[2:] == out_mask.shape[2:]
        return y * out_mask, out_mask

    def inorm(self, name, x, mask):
        import torch

        n = mask.sum(dim=(2, 3, 4), keepdim=True)
        mean = (x * mask).sum(dim=(2, 3, 4), keepdim=True) / n
        var = (((x - mean) ** 2) * mask).sum(dim=(2, 3, 4), keepdim=True) / n
        w, b = self.p[name + ".weight"].reshape(1, -1, 1, 1, 1), self.p[name + ".bias"].reshape(1, -1, 1, 1, 1)
        return ((x - mean) / torch.sqrt(var + 1e-8) * w + b) * mask

    def bnorm(self, name, x, mask):
        import torch

        w, b = self.p[name + ".bn.weight"].reshape(1, -1, 1, 1, 1), self.p[name + ".bn.bias"].reshape(1, -1, 1, 1, 1)
        if self.training:  # batch statistics over every active voxel of every frame, biased variance
            n = mask.sum()
            mean = (x * mask).sum(dim=(0, 2, 3, 4), keepdim=True) / n
            var = (((x - mean) ** 2) * mask).sum(dim=(0, 2, 3, 4), keepdim=True) / n
        else:
            mean = self.p[name + ".bn.running_mean"].reshape(1, -1, 1, 1, 1)
            var = self.p[name + ".bn.running_var"].reshape(1, -1, 1, 1, 1)
        return ((x - mean) / torch.sqrt(var + 1e-5) * w + b) * mask

    def block(self, name, x, mask):
        import torch

        stride = 2  # every stage has one block, and it strides
        if self.bottleneck:
            y, m = self.conv(name + ".conv1", x, mask)
            y = torch.relu(self.bnorm(name + ".norm1", y, m))
            y, m = self.conv(name + ".conv2", y, m, stride)
            y = torch.relu(self.bnorm(name + ".norm2", y, m))
            y, m = self.conv(name + ".conv3", y, m)
            y = self.bnorm(name + ".norm3", y, m)
        else:
            y, m = self.conv(name + ".conv1", x, mask, stride)
            y = torch.relu(self.bnorm(name + ".norm1", y, m))
            y, m = self.conv(name + ".conv2", y, m)
            y = self.bnorm(name + ".norm2", y, m)
        r, rm = self.conv(name + ".downsample.0", x, mask, stride)
        assert torch.equal(rm, m)
        r = self.bnorm(name + ".downsample.1", r, m)
        return torch.relu(y + r), m

    def forward(self, x, mask):
        import torch
        import torch.nn.functional as F

        y, m = self.conv("conv1.0", x, mask, 2)
        y = torch.relu(self.inorm("conv1.1", y, m))
        y = F.max_pool3d(torch.where(m.bool(), y, torch.full_like(y, -float("inf"))), 2, 2)
        m = _coarsen(m, 2)
        y = torch.where(m.bool(), y, torch.zeros_like(y))
        for i in (1, 2, 3, 4):
            y, m = self.block(f"layer{i}.0", y, m)
        y, m = F.pad(y, PAD_192), F.pad(m, PAD_192)
        y, m = self.conv("conv5.1", y, m, 3)
        y = F.gelu(self.inorm("conv5.2", y, m)) * m
        self.last_mask = m
        pooled = torch.where(m.bool(), y, torch.full_like(y, -float("inf"))).amax(dim=(2, 3, 4))
        return pooled @ self.p["final.linear.weight"].t() + self.p["final.linear.bias"]


# ---- set-up ---------------------------------------------------------------------------------------------------------
def _live_top_rows(pts):
    """per frame: the stride-192 voxels that have a stride-64 voxel within the centred 3x3x3 kernel (numpy, set-up only)"""
    c64 = np.unique(np.concatenate([pts[:, :1], pts[:, 1:] // 64 * 64], 1), axis=0)
    top = np.unique(np.concatenate([pts[:, :1], pts[:, 1:] // 192 * 192], 1), axis=0)
    return [int(sum((np.abs(c64[c64[:, 0] == b][:, 1:] - o).max(1) <= 64).any() for o in top[top[:, 0] == b][:, 1:]))
            for b in (0, 1)]


def _cloud(seed):
    """two frames of a few thousand voxels in the box: four blobs per frame, one around each pair of (x, z) cells"""
    rng = np.random.default_rng(seed)
    frames = []
    for b, n in ((0, 3000), (1, 2200)):
        centres = [(x, -160 + 6 * b, z) for x in (-98 + 5 * b, 24) for z in (-95, 20 + 6 * b)]
        frames.append(np.concatenate([np.full((n, 1), b), H.blob_cloud(rng, n, centres, 9.0, BOX_LO, BOX_HI)], 1))
    pts = np.concatenate(frames).astype(np.int32)
    feats = rng.standard_normal((len(pts), 3)).astype(np.float32)
    live = _live_top_rows(pts)
    assert min(live) >= 3, f"seed {seed}: {live} stride-192 voxels with inputs per frame (pick another seed)"
    return pts, feats


def _dense_input(pts, feats, dtype):
    import torch

    x = torch.zeros((2, 3) + SIZE, dtype=dtype)
    mask = torch.zeros((2, 1) + SIZE, dtype=dtype)
    g = pts[:, 1:] - np.array(ORIGIN)
    assert (g >= 0).all() and (g < np.array(SIZE)).all()
    b = torch.from_numpy(pts[:, 0].astype(np.int64))
    gx, gy, gz = (torch.from_numpy(g[:, i].astype(np.int64)) for i in range(3))
    x[b, :, gx, gy, gz] = torch.from_numpy(feats).to(dtype)
    mask[b, 0, gx, gy, gz] = 1
    return x, mask


def _small_resnet(bottleneck):
    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd.model.backbone.resnet import ResNetBase

    class Small(ResNetBase):
        BLOCK = ME.Bottleneck if bottleneck else ME.BasicBlock
        LAYERS = (1, 1, 1, 1)
        INIT_DIM = 16
        PLANES = (16, 32, 32, 64)

    return Small


def _model(bottleneck, gpu, seed=0):
    import torch

    from mrcc_amd import MinkowskiEngine as ME

    torch.manual_seed(seed)
    model = _small_resnet(bottleneck)(3, 5).to(gpu)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, ME.MinkowskiBatchNorm):  # randomised running statistics and affine parameters
                n = m.bn.num_features
                m.bn.running_mean.copy_(torch.randn(n, generator=g) * 0.2)
                m.bn.running_var.copy_(torch.rand(n, generator=g) + 0.5)
                m.bn.weight.copy_(torch.rand(n, generator=g) + 0.5)
                m.bn.bias.copy_(torch.randn(n, generator=g) * 0.2)
            if isinstance(m, ME.MinkowskiInstanceNorm):
                m.weight.copy_(torch.rand(1, m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(1, m.num_features, generator=g) * 0.2)
    return model


def _sparse_input(pts, feats, gpu, requires_grad=False):
    import torch

    from mrcc_amd import MinkowskiEngine as ME

    return ME.SparseTensor(torch.from_numpy(feats), coordinates=torch.from_numpy(pts), device=gpu, requires_grad=requires_grad)


def _params(model, dtype, requires_grad=False):
    out = {}
    for k, v in model.state_dict().items():
        if v.is_floating_point():
            out[k] = v.detach().cpu().to(dtype).clone().requires_grad_(requires_grad and k in dict(model.named_parameters()))
    return out


@pytest.mark.parametrize("bottleneck", [False, True], ids=["BasicBlock", "Bottleneck"])
def test_resnet_logits_match_dense_model(gpu, bottleneck):
    import torch

    pts, feats = _cloud(seed=11)
    model = _model(bottleneck, gpu).eval()
    with torch.no_grad():
        x = _sparse_input(pts, feats, gpu)
        got = model(x).cpu().double()
        cm = x.coordinate_manager
        assert min(cm.batch_bounds(192)[i + 1] - cm.batch_bounds(192)[i] for i in range(2)) >= 3
        evals = {}
        for dtype in (torch.float64, torch.float32):
            dense = Dense(_params(model, dtype), bottleneck, training=False)
            evals[dtype] = dense.forward(*_dense_input(pts, feats, dtype)).double()
        assert int(dense.last_mask.sum()) == cm.stride_map(192).V  # the dense and the sparse output sets have the same size
    want = evals[torch.float64]
    assert got.shape == (2, 5) and torch.isfinite(got).all()
    scale = want.abs().max()
    d32 = float((evals[torch.float32] - want).abs().max() / scale)
    err = float((got - want).abs().max() / scale)
    print(f"resnet dense check ({'Bottleneck' if bottleneck else 'BasicBlock'}): d32 = {d32:.3e}, error = {err:.3e}, "
          f"bound = {max(REL_TOL, 8 * d32):.3e}")
    assert err <= max(REL_TOL, 8 * d32)


def test_resnet_gradients_match_dense_autograd(gpu):
    """train() with dropout p = 0 (batch-norm batch statistics, every layer on its autograd path), loss = sum of squared
    logits: every parameter gradient and the input-feature gradient"""
    import torch

    pts, feats = _cloud(seed=11)
    model = _model(False, gpu).train()
    model.conv5[0].p = 0.0
    params = _params(model, torch.float64, requires_grad=True)  # before the forward updates the running statistics
    x = _sparse_input(pts, feats, gpu, requires_grad=True)
    logits = model(x)
    (logits ** 2).sum().backward()
    dense = Dense(params, False, training=True)
    dx, mask = _dense_input(pts, feats, torch.float64)
    dx.requires_grad_(True)
    want_logits = dense.forward(dx, mask)
    (want_logits ** 2).sum().backward()
    err = float((logits.detach().cpu().double() - want_logits.detach()).abs().max() / want_logits.detach().abs().max())
    print(f"resnet train-mode logits: error = {err:.3e}")
    assert err <= REL_TOL
    named = dict(model.named_parameters())
    assert set(named) == {k for k, v in params.items() if v.requires_grad}
    # the same dense model and loss in float32: printed beside every figure to show what fp32 arithmetic alone costs here
    p32 = {k: v.detach().float().requires_grad_(v.requires_grad) for k, v in params.items()}
    x32 = dx.detach().float().requires_grad_(True)
    (Dense(p32, False, training=True).forward(x32, mask.float()) ** 2).sum().backward()
    errors = {}
    for name, p in named.items():
        assert p.grad is not None, name
        want, got = params[name].grad, p.grad.cpu().double()
        errors[name] = float((got - want).abs().max() / want.abs().max())
        d32 = float((p32[name].grad.double() - want).abs().max() / want.abs().max())
        print(f"resnet train-mode gradient {name}: error = {errors[name]:.3e} (dense float32: {d32:.3e})")
    c = x.C.cpu().numpy()
    g = c[:, 1:] - np.array(ORIGIN)
    at = (torch.from_numpy(c[:, 0].astype(np.int64)), slice(None), torch.from_numpy(g[:, 0].astype(np.int64)),
          torch.from_numpy(g[:, 1].astype(np.int64)), torch.from_numpy(g[:, 2].astype(np.int64)))
    want = dx.grad[at]
    errors["input features"] = float((x.F.grad.cpu().double() - want).abs().max() / want.abs().max())
    d32 = float((x32.grad[at].double() - want).abs().max() / want.abs().max())
    print(f"resnet train-mode gradient input features: error = {errors['input features']:.3e} (dense float32: {d32:.3e})")
    over = {k: v for k, v in errors.items() if not v <= REL_TOL}
    assert not over, over


RESNET14_KEYS = (
    ["conv1.0.kernel", "conv1.1.weight", "conv1.1.bias"]
    + [f"layer{i}.0.{n}" for i in (1, 2, 3, 4) for n in (
        ["conv1.kernel"] + [f"norm1.bn.{s}" for s in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
        + ["conv2.kernel"] + [f"norm2.bn.{s}" for s in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
        + ["downsample.0.kernel"]
        + [f"downsample.1.bn.{s}" for s in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")])]
    + ["conv5.1.kernel", "conv5.2.weight", "conv5.2.bias", "final.linear.weight", "final.linear.bias"])


def test_resnet14_builds_and_runs(gpu):
    import torch

    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd.model.backbone import resnet

    model = resnet.ResNet14(3, 5).to(gpu).eval()
    sd = model.state_dict()
    assert list(sd) == RESNET14_KEYS
    assert sd["conv1.0.kernel"].shape == (27, 3, 64) and sd["conv5.1.kernel"].shape == (27, 512, 512)
    assert sd["layer2.0.downsample.0.kernel"].shape == (64, 128) and sd["conv1.1.weight"].shape == (1, 64)
    assert (resnet.ResNet18.LAYERS, resnet.ResNet34.LAYERS) == ((2, 2, 2, 2), (3, 4, 6, 3))
    assert (resnet.ResNet50.BLOCK, resnet.ResNet50.LAYERS) == (ME.Bottleneck, (3, 4, 6, 3))
    assert (resnet.ResNet101.BLOCK, resnet.ResNet101.LAYERS) == (ME.Bottleneck, (3, 4, 23, 3))
    rng = np.random.default_rng(0)
    pts = np.concatenate([np.concatenate([np.full((n, 1), b), H.blob_cloud(rng, n, [(-40, 10, 0), (60, -30, 20)], 9.0, (-100,) * 3,
                                                                          (100,) * 3)], 1) for b, n in ((0, 900), (1, 700))])
    x = ME.SparseTensor(torch.from_numpy(rng.standard_normal((len(pts), 3)).astype(np.float32)),
                        coordinates=torch.from_numpy(pts.astype(np.int32)), device=gpu)
    with torch.no_grad():
        out = model(x)
    assert out.shape == (2, 5) and torch.isfinite(out).all()


def test_old_conv_shapes_keep_their_plans(gpu):
    """the four shapes the U-Nets use still get the plan objects they got before the strided routes were added"""
    import torch

    from mrcc_amd import MinkowskiEngine as ME

    rng = np.random.default_rng(1)
    pts = np.concatenate([np.zeros((800, 1), np.int64), H.blob_cloud(rng, 800, [(0, 0, 0)], 6.0, (-30,) * 3, (30,) * 3)], 1)
    x = ME.SparseTensor(torch.ones(len(pts), 4), coordinates=torch.from_numpy(pts.astype(np.int32)), device=gpu)
    cm = x.coordinate_manager
    k3 = ME.MinkowskiConvolution(4, 4, kernel_size=3, dimension=3)
    down = ME.MinkowskiConvolution(4, 4, kernel_size=2, stride=2, dimension=3)
    up = ME.MinkowskiConvolutionTranspose(4, 4, kernel_size=2, stride=2, dimension=3)
    k1 = ME.MinkowskiConvolution(4, 4, kernel_size=1, dimension=3)
    assert k3._plan(x) == (cm.plan_k3(1, 1), 1) and k3._plan(x)[0] is cm.plans[("k3", 1, 1)]
    assert down._plan(x)[0] is cm.plan_down(1) and down._plan(x)[1] == 2 and down._plan(x)[0] is cm.plans[("down", 1)]
    x2 = x.new(torch.ones(cm.stride_map(2).V, 4, device=gpu), tensor_stride=2)
    assert up._plan(x2)[0] is cm.plan_up(2) and up._plan(x2)[1] == 1 and up._plan(x2)[0] is cm.plans[("up", 2)]
    assert k1._plan(x) == (None, 1)
    assert down._grad_plan(x, down._plan(x)[0])() is cm.plan_up(2) and up._grad_plan(x2, None)() is cm.plan_down(1)
    p3 = k3._plan(x)[0]
    assert k3._grad_plan(x, p3)() is p3 and k1._grad_plan(x, None)() is None
    assert not any(k[0].startswith("strided") for k in cm.plans)
    with pytest.raises(NotImplementedError):
        ME.MinkowskiConvolution(4, 4, kernel_size=2, stride=1, dimension=3)._plan(x)
    with pytest.raises(NotImplementedError):
        ME.MinkowskiConvolutionTranspose(4, 4, kernel_size=3, stride=2, dimension=3)._plan(x)


def test_strided_conv_on_a_batch_equals_per_frame_results(gpu):
    """a k3 s2 conv on a B = 2 tensor equals the two per-frame results bit for bit"""
    import torch

    from mrcc_amd import MinkowskiEngine as ME

    rng = np.random.default_rng(2)
    frames = [H.blob_cloud(rng, n, [(-4, 3, 1), (7, -6, 2)], 4.0, (-25,) * 3, (25,) * 3) for n in (700, 450)]
    feats = [rng.standard_normal((len(f), 8)).astype(np.float32) for f in frames]
    torch.manual_seed(0)
    conv = ME.MinkowskiConvolution(8, 16, kernel_size=3, stride=2, dimension=3).to(gpu).eval()

    def run(coords, f):
        x = ME.SparseTensor(torch.from_numpy(f), coordinates=torch.from_numpy(coords.astype(np.int32)), device=gpu)
        with torch.no_grad():
            y = conv(x)
        assert y.tensor_stride == 2
        return y

    both = run(np.concatenate([np.concatenate([np.full((len(f), 1), b), f], 1) for b, f in enumerate(frames)]),
               np.concatenate(feats))
    bounds = both.coordinate_manager.batch_bounds(2)
    for b, (f, ft) in enumerate(zip(frames, feats)):
        one = run(np.concatenate([np.zeros((len(f), 1), np.int64), f], 1), ft)
        assert torch.equal(one.C[:, 1:], both.C[bounds[b]:bounds[b + 1], 1:])
        assert torch.equal(one.F, both.F[bounds[b]:bounds[b + 1]])


def _three_frames():
    """three frames of different sizes; the last is so small (a dozen voxels inside one stride-192 cell whose neighbours along
    the negative axes are empty) that its stride-192 map has exactly one voxel"""
    rng = np.random.default_rng(21)
    big = H.blob_cloud(rng, 2600, [(-98, -160, -95), (24, -150, 20), (30, 40, -60)], 9.0, (-128, -192, -128), (80, 64, 64))
    mid = H.blob_cloud(rng, 1100, [(-40, 10, 0), (60, -30, 20)], 9.0, (-100,) * 3, (100,) * 3)
    tiny = H.blob_cloud(rng, 12, [(70, 75, 80)], 3.0, (64,) * 3, (96,) * 3)
    frames = [big, mid, tiny]
    feats = [rng.standard_normal((len(f), 3)).astype(np.float32) for f in frames]
    return frames, feats


@pytest.mark.parametrize("bottleneck", [False, True], ids=["BasicBlock", "Bottleneck"])
def test_resnet_batched_logits_are_the_per_frame_bits(gpu, bottleneck):
    """eval(): every operator depends on a frame's own rows only (the instance-norm tree is cut relative to the frame's first
    row, every conv element is one fma chain whatever the instance or tile), so row b of the batched
    logits has the bits of frame b run alone"""
    import torch

    frames, feats = _three_frames()
    model = _model(bottleneck, gpu).eval()

    def run(fs, ft):
        pts = np.concatenate([np.concatenate([np.full((len(f), 1), b), f], 1) for b, f in enumerate(fs)]).astype(np.int32)
        x = _sparse_input(pts, np.concatenate(ft), gpu)
        with torch.no_grad():
            return model(x), x.coordinate_manager

    both, cm = run(frames, feats)
    bounds = cm.batch_bounds(192)
    assert len(bounds) == 4 and bounds[3] - bounds[2] == 1 and bounds[1] - bounds[0] > 1 and bounds[2] - bounds[1] > 1
    assert both.shape == (3, 5) and torch.isfinite(both).all()
    for b in range(3):
        one, _ = run(frames[b:b + 1], feats[b:b + 1])
        assert torch.equal(one[0], both[b]), (b, one[0].tolist(), both[b].tolist())


@pytest.mark.parametrize("bottleneck", [False, True], ids=["BasicBlock", "Bottleneck"])
def test_fused_instance_norm_relu_equals_the_plain_sequence(gpu, bottleneck):
    """ResNetBase._run fuses InstanceNorm -> ReLU into one call that applies ReLU in float64 before the one rounding; rounding is
    monotone and keeps 0, so relu(round(v)) == round(relu(v)) and the stem run as a plain nn.Sequential gives the same bits"""
    import torch

    frames, feats = _three_frames()
    model = _model(bottleneck, gpu).eval()
    pts = np.concatenate([np.concatenate([np.full((len(f), 1), b), f], 1) for b, f in enumerate(frames)]).astype(np.int32)
    with torch.no_grad():
        fused = model._run(model.conv1, _sparse_input(pts, np.concatenate(feats), gpu))
        plain = model.conv1(_sparse_input(pts, np.concatenate(feats), gpu))
    assert fused.tensor_stride == plain.tensor_stride == 4 and torch.equal(fused.C, plain.C)
    assert torch.equal(fused.F, plain.F) and (fused.F == 0).any() and (fused.F > 0).any()
