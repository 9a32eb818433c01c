"""Backward of every sparse layer kind (nn.SparseConvFunction: dX on sv_conv_fwd with mirrored weights, dW in
sv_conv_wgrad) against a float64 torch gather / index_add reference built from the RAW kernel maps (plan.raw: the
unsorted neighbour table), so the reference shares no arithmetic and no plan with the HIP kernels.

Bound per element: |got - want| <= C * 1e-7 * sum|terms| (+ 1e-30), where sum|terms| is the same reference evaluated on
|in|, |W| and |dY| - the size of the sum each element is, not of its result.  C = 16; the observed margin (largest
|err| / bound) is printed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C_BOUND = 16.0


def _cloud(seed, n, span=24):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    shell = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(span * 0.6, span * 0.7, size=(n, 1))
    slab = np.concatenate([rng.uniform(-span, span, size=(n // 2, 2)), rng.uniform(-2, 1, size=(n // 2, 1))], axis=1)
    c = np.unique(np.floor(np.concatenate([shell, slab])).astype(np.int64), axis=0)
    return c[rng.permutation(len(c))]


def _tensor(gpu, clouds, cin, seed=5):
    from mrcc_amd import MinkowskiEngine as ME

    coords = np.concatenate([np.concatenate([np.full((len(c), 1), b), c], 1) for b, c in enumerate(clouds)])
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(len(coords), cin, generator=g)
    return ME.SparseTensor(feats, coordinates=torch.from_numpy(coords).int(), device=gpu, requires_grad=True)


def _ref(fin, W, nbr, V_out):
    """out[o] = sum_k fin[nbr[k][o]] @ W[k] (float64, differentiable)"""
    out = torch.zeros((V_out, W.shape[2]), dtype=torch.float64, device=fin.device)
    for k in range(W.shape[0]):
        idx = nbr[k, :V_out].long()
        ok = idx >= 0
        out = out.index_add(0, torch.nonzero(ok).flatten(), fin[idx[ok]] @ W[k])
    return out


def _ref_grads(fin, W, nbr, V_out, dy):
    a = fin.double().detach().requires_grad_(True)
    w = W.double().detach().requires_grad_(True)
    _ref(a, w, nbr, V_out).backward(dy.double())
    aa = fin.double().abs().detach().requires_grad_(True)
    wa = W.double().abs().detach().requires_grad_(True)
    _ref(aa, wa, nbr, V_out).backward(dy.double().abs())
    return a.grad, w.grad, aa.grad, wa.grad


def _check(name, got, want, terms):
    err = (got.double() - want).abs()
    bound = C_BOUND * 1e-7 * terms + 1e-30
    margin = float((err / bound).max())
    print(f"{name}: max |err| {float(err.max()):.3e}, margin {margin:.3f} of the bound (C = {C_BOUND})")
    assert margin <= 1.0, (name, margin)


def _weight3_grad(layer):
    g = layer.kernel.grad
    return g if g.dim() == 3 else g.unsqueeze(0)


def _layer_case(gpu, cin, cout, ks=3, stride=1, transposed=False, bias=False, clouds=None, cat=0, dilation=1):
    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd import nn as svnn

    torch.manual_seed(cin * 1000 + cout)
    cls = ME.MinkowskiConvolutionTranspose if transposed else ME.MinkowskiConvolution
    layer = cls(cin, cout, kernel_size=ks, stride=stride, dilation=dilation, bias=bias, dimension=3).to(gpu).train()
    clouds = clouds or [_cloud(1, 1500)]
    x0 = _tensor(gpu, clouds, cin + cat)
    x = x0
    if cat:  # the input is the column slice of a concatenated buffer (decoder widths): a strided view
        x = x0.new(x0.F[:, :cin])
    if transposed:  # the coarse level must exist: run the matching down conv's map
        cm = x0.coordinate_manager
        cm.plan_down(1)
        f2 = torch.randn(cm.stride_map(2).V, cin, generator=torch.Generator().manual_seed(3)).to(gpu).requires_grad_(True)
        x = x0.new(f2, tensor_stride=2)
    plan, out_stride = layer._plan(x)  # (a strided layer's plan creates its output map)
    whole = plan.whole if isinstance(plan, svnn.SplitPlan) else plan
    V_out = x.coordinate_manager.stride_map(out_stride).V
    nbr = whole.raw[0] if whole is not None else torch.arange(V_out, device=gpu, dtype=torch.int32)[None]
    assert whole is None or (whole.V_out == V_out and nbr.shape[0] == ks ** 3)
    out = layer.forward_fused(x)
    dy = torch.randn(out.F.shape, generator=torch.Generator().manual_seed(9)).to(gpu)
    out.F.backward(dy)
    leaf = x.F if x.F.is_leaf else x0.F
    dx = leaf.grad[:, :cin] if cat else leaf.grad
    dw = _weight3_grad(layer)
    W = layer.weight3().detach()
    fin = x.F.detach()
    want_dx, want_dw, terms_dx, terms_dw = _ref_grads(fin, W, nbr, V_out, dy)
    tag = f"{cin}->{cout} k{ks} s{stride}{f' d{dilation}' if dilation > 1 else ''}{' tr' if transposed else ''}"
    _check(tag + " dX", dx, want_dx, terms_dx)
    _check(tag + " dW", dw, want_dw, terms_dw)
    if ks == 1 and stride > 1:
        # input rows that no output reads: the reference gives exactly 0, and so must the kernel (its plan tiles without a
        # single pair still write their rows)
        unseen = torch.ones(fin.shape[0], dtype=torch.bool, device=gpu)
        unseen[nbr[nbr >= 0].long()] = False
        assert int(unseen.sum()) * 2 > fin.shape[0] and bool((want_dx[unseen] == 0).all())
        assert bool((dx[unseen] == 0).all()), f"{tag}: {int((dx[unseen] != 0).sum())} nonzero elements in rows no output reads"
    if bias:
        assert torch.allclose(layer.bias.grad.double().flatten(), dy.double().sum(0), rtol=1e-5, atol=1e-4)
    # a second backward gives the same bits (no atomics in either gradient)
    layer.kernel.grad = None
    leaf.grad = None
    out2 = layer.forward_fused(x)
    out2.F.backward(dy)
    assert torch.equal(_weight3_grad(layer), dw)
    assert torch.equal(leaf.grad[:, :cin] if cat else leaf.grad, dx)
    return plan


@pytest.mark.parametrize("cin,cout", [(3, 32), (32, 32), (64, 64), (32, 64)])
def test_k3_layer_gradients(gpu, cin, cout):
    _layer_case(gpu, cin, cout)


def test_k3_wide_as_split_passes(gpu, monkeypatch):
    from mrcc_amd import nn as svnn

    monkeypatch.setattr(svnn, "SPLIT_RULES", [(0, (9, 18))])
    plan = _layer_case(gpu, 384, 384, clouds=[_cloud(4, 700)])
    assert isinstance(plan, svnn.SplitPlan)


def test_k3_decoder_cat_width(gpu):
    # the first conv after a concatenation reads its input as the left columns of a wider buffer (row stride 480)
    _layer_case(gpu, 416, 384, clouds=[_cloud(6, 500)], cat=64)


def test_k8_down_and_transposed_up(gpu):
    _layer_case(gpu, 32, 64, ks=2, stride=2)
    _layer_case(gpu, 64, 96, ks=2, stride=2, transposed=True)


def test_1x1_with_bias(gpu):
    _layer_case(gpu, 96, 20, ks=1, bias=True)


def test_batch_of_two_frames(gpu):
    _layer_case(gpu, 32, 64, clouds=[_cloud(7, 1200), _cloud(8, 800)])
    _layer_case(gpu, 32, 32, ks=2, stride=2, clouds=[_cloud(7, 1200), _cloud(8, 800)])


# ---- the strided, kernel_size 1 strided and dilated layers of the classification ResNets: dX on plan_strided_t with W[k]^T
#      (no mirror), dW on the forward plan; on the dilated stride-1 layer dX takes the mirror rule on a dilated map
@pytest.mark.parametrize("cin,cout", [(3, 64), (64, 64)])
def test_k3_stride2_layer_gradients(gpu, cin, cout):
    _layer_case(gpu, cin, cout, ks=3, stride=2)


def test_k3_stride3_layer_gradients(gpu):
    _layer_case(gpu, 64, 64, ks=3, stride=3)


def test_k1_stride2_with_bias(gpu):
    _layer_case(gpu, 64, 256, ks=1, stride=2, bias=True)


def test_k3_dilated_layer_gradients(gpu):
    _layer_case(gpu, 32, 32, ks=3, stride=1, dilation=2)
    _layer_case(gpu, 32, 64, ks=3, stride=2, dilation=2)


def test_strided_layers_batch_of_two_frames(gpu):
    _layer_case(gpu, 32, 64, ks=3, stride=2, clouds=[_cloud(7, 1200), _cloud(8, 800)])
    _layer_case(gpu, 64, 96, ks=1, stride=2, clouds=[_cloud(7, 1200), _cloud(8, 800)])


@pytest.mark.parametrize("cin,cout", [(256, 1024), (1024, 3)])
def test_linear_gradients(gpu, cin, cout):
    from mrcc_amd import MinkowskiEngine as ME

    torch.manual_seed(cin + cout)
    lin = ME.MinkowskiOps.MinkowskiLinear(cin, cout).to(gpu).train()
    x = _tensor(gpu, [_cloud(2, 900)], cin)
    out = lin.forward_fused(x)
    dy = torch.randn(out.F.shape, generator=torch.Generator().manual_seed(4)).to(gpu)
    out.F.backward(dy)
    W = lin.linear.weight.detach().t().unsqueeze(0)
    nbr = torch.arange(x.F.shape[0], device=gpu, dtype=torch.int32)[None]
    want_dx, want_dw, terms_dx, terms_dw = _ref_grads(x.F.detach(), W, nbr, x.F.shape[0], dy)
    _check(f"linear {cin}->{cout} dX", x.F.grad, want_dx, terms_dx)
    _check(f"linear {cin}->{cout} dW", lin.linear.weight.grad.t(), want_dw[0], terms_dw[0])
    assert torch.allclose(lin.linear.bias.grad.double(), dy.double().sum(0), rtol=1e-5, atol=1e-4)


def test_wgrad_accumulate_sums_in_order(gpu):
    """accumulate = 1 adds the new sum into dW: wgrad(dY_a) then wgrad(dY_b, accumulate) == dW_a + dW_b bit for bit"""
    from mrcc_amd import nn as svnn

    x = _tensor(gpu, [_cloud(3, 1500)], 64)
    plan = x.coordinate_manager.plan_k3(1)
    V = x.F.shape[0]
    g = torch.Generator().manual_seed(11)
    dya, dyb = torch.randn(V, 96, generator=g).to(gpu), torch.randn(V, 96, generator=g).to(gpu)
    fin = x.F.detach()
    dwa = svnn.conv_wgrad(fin, dya, plan, 27, 64, 96)
    dwb = svnn.conv_wgrad(fin, dyb, plan, 27, 64, 96)
    acc = dwa.clone()
    svnn._wgrad_one(fin, dyb, plan, 27, 64, 96, V, acc, True)
    assert torch.equal(acc, dwa + dwb)
    # and overwrite mode ignores what dW held
    junk = torch.full_like(dwa, float("nan"))
    svnn._wgrad_one(fin, dya, plan, 27, 64, 96, V, junk, False)
    assert torch.equal(junk, dwa)
