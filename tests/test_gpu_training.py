"""Training on the sparse path: whole networks' gradients against float64 autograd on a dense grid, the pose heads,
eval after training, eval with grad enabled, and the reference's train_epoch loop.

(a) The reference is the masked dense-grid float64 network of tests/test_gpu_dense_grid.py (conv3d / stride-2 conv3d /
conv_transpose3d masked to the active voxel sets), carried here with BatchNorm in TRAINING mode: batch statistics over
the active voxels of every frame of the batch only, running statistics updated with the unbiased variance (what
nn.BatchNorm1d does on the feature rows).  Its leaves are the model's state_dict tensors in float64; torch autograd gives
the reference gradients.  Tolerance: max |got - want| <= 1e-4 * max |want| per tensor - gradients, input-feature gradient, updated running
statistics (the worst tensors are printed)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

REL_TOL = 1e-4


def _dense_weights3(kernel, transposed=False):
    K, cin, cout = kernel.shape
    k = round(K ** (1 / 3))
    w = kernel.reshape(k, k, k, cin, cout)  # [z, y, x, ci, co]
    return w.permute(3, 4, 0, 1, 2) if transposed else w.permute(4, 3, 0, 1, 2)


class TrainDenseNet:
    """float64 leaves = the model's parameters; BN with batch statistics over the active voxels"""

    def __init__(self, sd, masks, frozen=()):
        self.sd = {k: v.detach().cpu().double().clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
        self.masks = masks
        self.frozen = set(frozen)  # BN modules left in eval() inside the training model: running statistics
        self.stats = {}

    def bn(self, x, name, m):
        g = lambda s: self.sd[f"{name}.bn.{s}"].view(1, -1, 1, 1, 1)  # noqa: E731
        if name in self.frozen:
            return (x - g("running_mean")) / torch.sqrt(g("running_var") + 1e-5) * g("weight") + g("bias")
        n = m.sum()
        mean = (x * m).sum((0, 2, 3, 4), keepdim=True) / n
        var = (((x - mean) ** 2) * m).sum((0, 2, 3, 4), keepdim=True) / n
        self.stats[name] = (mean.detach().flatten(), (var * n / (n - 1)).detach().flatten())
        return (x - mean) / torch.sqrt(var + 1e-5) * g("weight") + g("bias")

    def conv(self, x, name, level):
        w = self.sd[name + ".kernel"]
        if w.dim() == 2:
            out = F.conv3d(x, w.t().reshape(w.shape[1], w.shape[0], 1, 1, 1))
        else:
            out = F.conv3d(x, _dense_weights3(w), padding=1)
        return out * self.masks[level]

    def down(self, x, name, level):
        if x.shape[-1] % 2:  # a single coarse cell (deep AliveUNet levels): its 8 children, the others empty
            x = F.pad(x, (0, 1, 0, 1, 0, 1))
        return F.conv3d(x, _dense_weights3(self.sd[name + ".kernel"]), stride=2) * self.masks[level + 1]

    def up(self, x, name, level):
        out = F.conv_transpose3d(x, _dense_weights3(self.sd[name + ".kernel"], True), stride=2)
        S = self.masks[level - 1].shape[-1]
        return out[..., :S, :S, :S] * self.masks[level - 1]

    def cbr(self, x, conv, bn, level, relu=True):
        m = self.masks[level]
        y = self.bn(self.conv(x, conv, level), bn, m) * m
        return F.relu(y) * m if relu else y

    def block(self, x, name, level):
        m = self.masks[level]
        out = self.cbr(x, name + ".conv1", name + ".norm1", level)
        out = self.cbr(out, name + ".conv2", name + ".norm2", level, relu=False)
        res = x
        if name + ".downsample.0.kernel" in self.sd:
            res = self.cbr(x, name + ".downsample.0", name + ".downsample.1", level, relu=False)
        return F.relu(out + res) * m

    def stack(self, x, name, level):
        i = 0
        while f"{name}.{i}.conv1.kernel" in self.sd:
            x = self.block(x, f"{name}.{i}", level)
            i += 1
        return x

    def forward(self, x, n=4, alive=False, stop="full"):
        m = self.masks
        out = self.cbr(x, "conv0p1s1", "bn0", 0)
        skips = [out]
        for i in range(1, n + 1):
            y = self.down(out, f"conv{i}p{2 ** (i - 1)}s2", i - 1)
            out = F.relu(self.bn(y, f"bn{i}", m[i]) * m[i]) * m[i]
            out = self.stack(out, f"block{i}", i)
            skips.append(out)
        out = skips.pop()
        if stop == "encoder":
            return out
        for j in range(n, 2 * n):
            level = 2 * n - j
            name = f"convtr{j}" if alive else f"convtr{j}p{2 ** level}s2"
            y = self.up(out, name, level)
            out = F.relu(self.bn(y, f"bntr{j}", m[level - 1]) * m[level - 1]) * m[level - 1]
            out = torch.cat([out, skips.pop()], dim=1)
            out = self.stack(out, f"block{j + 1}", level - 1)
        if alive or stop == "except_final":
            return out
        w, b = self.sd["final.kernel"], self.sd["final.bias"].view(1, -1, 1, 1, 1)
        out = (F.conv3d(out, w.t().reshape(w.shape[1], w.shape[0], 1, 1, 1)) + b) * m[0]
        lin = lambda t, n_: F.conv3d(t, self.sd[f"regression.{n_}.linear.weight"][:, :, None, None, None],  # noqa: E731
                                     self.sd[f"regression.{n_}.linear.bias"])
        out = F.leaky_relu(out, 0.01)
        out = F.leaky_relu(lin(out, 0), 0.01)
        return lin(out, 2) * m[0]


def _cloud(seed, n, lo=-16, hi=16):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    mid, r = (lo + hi) / 2, (hi - lo) / 2
    shell = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.65 * r, 0.78 * r, size=(n, 1)) + mid
    slab = np.concatenate([rng.uniform(lo, hi, size=(n // 2, 2)), rng.uniform(mid - 3, mid - 1, size=(n // 2, 1))], 1)
    c = np.floor(np.concatenate([shell, slab])).astype(np.int64)
    c = np.unique(c[((c >= lo) & (c < hi)).all(axis=1)], axis=0)
    return c[rng.permutation(len(c))]


def _randomise_bn(net):
    g = torch.Generator().manual_seed(22)
    with torch.no_grad():
        for mod in net.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.weight.copy_(torch.rand(mod.num_features, generator=g) * 0.5 + 0.75)
                mod.bias.copy_(torch.randn(mod.num_features, generator=g) * 0.1)


def _setup(gpu, clouds, off, G, levels, seed=3):
    from mrcc_amd import MinkowskiEngine as ME

    rng = np.random.default_rng(seed)
    feats = [rng.uniform(-0.5, 0.5, size=(len(c), 3)).astype(np.float32) for c in clouds]
    coords4 = np.concatenate([np.concatenate([np.full((len(c), 1), b), c], 1) for b, c in enumerate(clouds)])
    x = ME.SparseTensor(torch.from_numpy(np.concatenate(feats)), coordinates=torch.from_numpy(coords4).int(), device=gpu,
                        requires_grad=True)
    dense = torch.zeros((len(clouds), 3, G, G, G), dtype=torch.float64)
    m0 = torch.zeros((len(clouds), 1, G, G, G), dtype=torch.float64)
    for b, (c, f) in enumerate(zip(clouds, feats)):
        s = c + off
        dense[b, :, s[:, 2], s[:, 1], s[:, 0]] = torch.from_numpy(f.astype(np.float64)).t()
        m0[b, 0, s[:, 2], s[:, 1], s[:, 0]] = 1.0
    masks = [m0]
    for _ in range(levels):
        masks.append(F.max_pool3d(masks[-1], 2, ceil_mode=True))
    dense.requires_grad_(True)
    return x, dense, masks


def _gather(dense, oc, off):
    return dense[oc[:, 0], :, oc[:, 3] + off, oc[:, 2] + off, oc[:, 1] + off]


def _compare(name, got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    rel = err / max(scale, 1e-30)
    return rel, f"{name}: rel {rel:.2e} (max |want| {scale:.2e})"


def _check_all(model, ref, x, dense_grad_rows, skip=()):
    worst, lines = 0.0, []
    for name, p in model.named_parameters():
        assert p.grad is not None, f"{name} has no gradient"
        want = ref.sd[name].grad
        rel, line = _compare(name, p.grad, want)
        worst = max(worst, rel)
        lines.append(line)
    rel, line = _compare("input features", x.F.grad, dense_grad_rows)
    worst = max(worst, rel)
    lines.append(line)
    for mname, mod in model.named_modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            key = mname[: -len(".bn")]
            if key in skip or key not in ref.stats:
                continue
            mean, var = ref.stats[key]
            rm = 0.9 * ref.sd[mname + ".running_mean"].detach() + 0.1 * mean
            rv = 0.9 * ref.sd[mname + ".running_var"].detach() + 0.1 * var
            for what, got, want in (("running_mean", mod.running_mean, rm), ("running_var", mod.running_var, rv)):
                rel, line = _compare(f"{mname}.{what}", got, want)
                worst = max(worst, rel)
                lines.append(line)
            assert int(mod.num_batches_tracked) == 1
    lines.sort(key=lambda l: -float(l.split("rel ")[1].split()[0]))
    print(f"worst relative max-abs error {worst:.2e} (tolerance {REL_TOL:.0e}) over {len(lines)} tensors; " +
          "; ".join(lines[:3]))
    assert worst <= REL_TOL, "\n".join(lines)


def test_segmentation_14a_gradients_match_float64(gpu):
    from mrcc_amd.model.backbone.minkunet import MinkUNet14A
    from mrcc_amd.model.robotnet_segmentation import _classification_head

    torch.manual_seed(21)
    model = _classification_head(MinkUNet14A, lambda: 3, "SegHead14A")(3, num_classes=3)
    _randomise_bn(model)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(gpu).train()
    clouds = [_cloud(1, 2500), _cloud(2, 900)]
    assert all(c.min() < -10 for c in clouds)
    x, dense, masks = _setup(gpu, clouds, 16, 32, 4)
    out = model(x)
    gw = torch.randn(out.F.shape, generator=torch.Generator().manual_seed(5))
    (out.F * gw.to(gpu)).sum().backward()
    ref = TrainDenseNet(sd0, masks)
    oc = out.C.cpu().numpy().astype(np.int64)
    want = _gather(ref.forward(dense), oc, 16)
    rel, line = _compare("logits", out.F, want)
    print(line)
    assert rel <= REL_TOL
    (want * gw.double()).sum().backward()
    xc = x.C.cpu().numpy().astype(np.int64)
    _check_all(model, ref, x, _gather(dense.grad, xc, 16))


def test_alive_unet_gradients_match_float64(gpu):
    from mrcc_amd.model.backbone.aliveunet import make_alive_unet

    torch.manual_seed(31)
    model = make_alive_unet(m=4, block_reps=1, bottleneck=False)(3, 20)
    _randomise_bn(model)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(gpu).train()
    # levels 4-7 hold 1-8 voxels per frame: batch statistics over 2-16 rows make BN's gradient ill-conditioned (it
    # amplifies float32 rounding by orders of magnitude), so their BN modules stay frozen - eval() inside a training
    # model, running statistics, still differentiable - which pins that path as well
    deep = [f"bn{i}" for i in range(4, 8)] + [f"bntr{j}" for j in range(7, 10)]
    frozen = set(deep)
    for name, mod in model.named_modules():
        top = name.split(".")[0]
        if isinstance(mod, type(model.bn0)) and (name in deep or top in {f"block{i}" for i in range(4, 11)}):
            mod.eval()
            frozen.add(name)
    clouds = [_cloud(3, 1800, 0, 32), _cloud(4, 700, 0, 32)]  # 7 levels: the deep ones are one cell of the dense grid
    x, dense, masks = _setup(gpu, clouds, 0, 32, 7)
    out = model(x)
    gw = torch.randn(out.F.shape, generator=torch.Generator().manual_seed(6))
    (out.F * gw.to(gpu)).sum().backward()
    ref = TrainDenseNet(sd0, masks, frozen)
    oc = out.C.cpu().numpy().astype(np.int64)
    want = _gather(ref.forward(dense, n=7, alive=True), oc, 0)
    (want * gw.double()).sum().backward()
    for name, p in model.named_parameters():  # `final` is never applied by AliveUNet.forward (reference :177-265)
        if name.startswith("final."):
            assert p.grad is None
            p.grad = torch.zeros_like(p)
            ref.sd[name].grad = torch.zeros_like(ref.sd[name])
    xc = x.C.cpu().numpy().astype(np.int64)
    _check_all(model, ref, x, _gather(dense.grad, xc, 0))


@pytest.mark.parametrize("kind", ["robotnet", "robotnet_encode"])
def test_pose_head_gradients_match_float64(gpu, kind):
    """RobotNet (max pool) / RobotNetEncode (avg pool) parameter gradients: dense float64 body, BN + ReLU, then an
    order-free pooling over each frame's active voxels (torch amax / mean over the gathered rows)"""
    from mrcc_amd.model.robotnet import make_robotnet, make_robotnet_encode

    torch.manual_seed(41)
    cls = (make_robotnet if kind == "robotnet" else make_robotnet_encode)(backbone="minkunet14A")
    model = cls(3, 9)
    _randomise_bn(model)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(gpu).train()
    clouds = [_cloud(5, 1500), _cloud(6, 1100)]
    x, dense, masks = _setup(gpu, clouds, 16, 32, 4)
    out = model(x)
    assert out.shape == (2, 9)
    gw = torch.randn(out.shape, generator=torch.Generator().manual_seed(7))
    (out * gw.to(gpu)).sum().backward()
    ref = TrainDenseNet(sd0, masks)
    level = 0 if kind == "robotnet" else 4
    body = ref.forward(dense, stop="except_final" if kind == "robotnet" else "encoder")
    m = masks[level]
    h = F.relu(ref.bn(body, "output_layer.0", m)) * m
    rows = []
    for b in range(2):
        sel = h[b][:, m[b, 0] > 0]  # [C, active voxels of frame b]
        rows.append(sel.amax(1) if kind == "robotnet" else sel.mean(1))
    pooled = torch.stack(rows)
    sd = ref.sd
    hh = F.leaky_relu(pooled @ sd["pose_regression.0.weight"].t() + sd["pose_regression.0.bias"], 0.01)
    o = hh @ sd["pose_regression.2.weight"].t() + sd["pose_regression.2.bias"]
    o = torch.cat([o[:, :7], torch.sigmoid(o[:, 7:])], 1)
    rel, line = _compare("pose output", out, o)
    print(line)
    assert rel <= REL_TOL
    (o * gw.double()).sum().backward()
    worst, lines = 0.0, []
    for name, p in model.named_parameters():
        if name.startswith("final.") or name.startswith("final_bn.") or (kind == "robotnet_encode" and (
                name.startswith("convtr") or name.startswith("bntr") or any(name.startswith(f"block{i}.") for i in (5, 6, 7, 8)))):
            assert p.grad is None, name  # not on the head's path
            continue
        rel, line = _compare(name, p.grad, sd[name].grad)
        worst = max(worst, rel)
        lines.append(line)
    print(f"{kind}: worst relative max-abs error {worst:.2e} over {len(lines)} parameters")
    assert worst <= REL_TOL, "\n".join(lines)


def _seg_model(gpu, seed=1):
    from mrcc_amd.model.backbone.minkunet import MinkUNet14A
    from mrcc_amd.model.robotnet_segmentation import _classification_head

    torch.manual_seed(seed)
    return _classification_head(MinkUNet14A, lambda: 3, "SegHead14A")(3, num_classes=3).to(gpu)


def test_eval_after_training_is_bit_identical_to_a_fresh_model(gpu):
    from mrcc_amd import MinkowskiEngine as ME

    model = _seg_model(gpu).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    clouds = [_cloud(8, 2000), _cloud(9, 1000)]
    x, _, _ = _setup(gpu, clouds, 16, 32, 0)
    feats, coords = x.F.detach().clone(), x.C.clone()
    model.eval()
    with torch.no_grad():
        before = model(ME.SparseTensor(feats, coordinates=coords, device=gpu)).F.clone()  # fills the eval caches
    model.train()
    labels = torch.randint(0, 3, (feats.shape[0],), generator=torch.Generator().manual_seed(1)).to(gpu)
    for _ in range(3):
        out = model(ME.SparseTensor(feats, coordinates=coords, device=gpu))
        opt.zero_grad()
        torch.nn.functional.cross_entropy(out.F, labels).backward()
        opt.step()
    model.eval()
    with torch.no_grad():
        got = model(ME.SparseTensor(feats, coordinates=coords, device=gpu)).F
    fresh = _seg_model(gpu, seed=99)
    fresh.load_state_dict(model.state_dict())
    fresh.eval()
    with torch.no_grad():
        want = fresh(ME.SparseTensor(feats, coordinates=coords, device=gpu)).F
    assert not torch.equal(got, before), "the optimizer steps changed nothing"
    assert torch.equal(got, want), "a cache (folded BN / transposed linear weights) kept the pre-step weights"


def test_eval_mode_with_grad_enabled_is_the_inference_path(gpu):
    from mrcc_amd import MinkowskiEngine as ME

    model = _seg_model(gpu).eval()
    x, _, _ = _setup(gpu, [_cloud(10, 2000)], 16, 32, 0)
    feats, coords = x.F.detach().clone(), x.C.clone()
    with torch.enable_grad():
        a = model(ME.SparseTensor(feats, coordinates=coords, device=gpu)).F
    with torch.no_grad():
        b = model(ME.SparseTensor(feats, coordinates=coords, device=gpu)).F
    assert a.requires_grad is False and a.grad_fn is None
    assert torch.equal(a, b)


def test_reference_train_epoch_loop_reduces_the_loss(gpu):
    """train_segmentation.py's train_epoch: ME.utils.sparse_quantize per frame (voxels whose points disagree get
    ignore_label), ME.utils.batched_coordinates, SparseTensor, CrossEntropyLoss(ignore_index), Adam - on gen_scene frames"""
    import mrcc_amd
    from mrcc_amd import MinkowskiEngine as ME

    model = _seg_model(gpu, seed=7).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    criterion = torch.nn.CrossEntropyLoss(ignore_index=-100)
    cs, fs, ls = [], [], []
    for seed in range(2):
        sc = mrcc_amd.synth.gen_scene(seed, n_bg=6000, n_arm=2000, n_ee=2000, keyed_colors=True)
        c, f, lab = ME.utils.sparse_quantize(sc["points"], sc["rgb"], labels=sc["segmentation"], ignore_label=-100,
                                             quantization_size=0.04)
        cs.append(torch.from_numpy(np.asarray(c)))
        fs.append(np.asarray(f) - 0.5)
        ls.append(np.asarray(lab))
    assert any((l == -100).any() for l in ls), "no ignore_label voxel in the batch"
    coords = ME.utils.batched_coordinates(cs)
    feats = torch.from_numpy(np.concatenate(fs).astype(np.float32))
    labels = torch.from_numpy(np.concatenate(ls).astype(np.int64)).to(gpu)  # canonical row order = the tensor's
    losses = []
    for _ in range(30):
        out = model(ME.SparseTensor(feats, coordinates=coords, device=gpu))
        opt.zero_grad()
        loss = criterion(out.F, labels)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(f"loss: first step {losses[0]:.4f}, after {len(losses)} steps {losses[-1]:.4f} "
          f"({losses[-1] / losses[0]:.2f} of the first)")
    assert losses[-1] < 0.5 * losses[0]
