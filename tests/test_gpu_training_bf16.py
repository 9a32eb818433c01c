"""bf16 mixed-precision training (nn.set_training_precision): sv_conv_wgrad_bf16 against a float64 gather sum of
bf16-rounded operands built from the RAW kernel maps (plan.raw), its determinism / accumulate / NaN contract, and whole
networks: bf16 gradients against fp32 gradients, which kernel each op of a step ran, the fallbacks, eval after bf16
training, and the reference's train_epoch loop.

Kernel bound per element: |got - want| <= 16e-7 * sum|terms| (+ 1e-30), the bound tests/test_gpu_conv_grad.py holds the
fp32 kernel to: bf16 x bf16 products are exact in fp32, so only the fp32 accumulation rounds."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C_BOUND = 16.0
NET_REL_TOL = 0.05  # the issue's aim per parameter: reported, not reachable at random init


def _cloud(seed, n, span=24):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    shell = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(span * 0.6, span * 0.7, size=(n, 1))
    slab = np.concatenate([rng.uniform(-span, span, size=(n // 2, 2)), rng.uniform(-2, 1, size=(n // 2, 1))], axis=1)
    c = np.unique(np.floor(np.concatenate([shell, slab])).astype(np.int64), axis=0)
    return c[rng.permutation(len(c))]


def _scatter_cloud(seed, n, span=200):
    """isolated voxels: most 16-row sub-tiles have no pair at most offsets (submask bits clear)"""
    rng = np.random.default_rng(seed)
    c = np.unique(rng.integers(-span, span, size=(n, 3)), axis=0)
    return c[rng.permutation(len(c))]


def _tensor(gpu, clouds, cin, seed=5):
    from mrcc_amd import MinkowskiEngine as ME

    coords = np.concatenate([np.concatenate([np.full((len(c), 1), b), c], 1) for b, c in enumerate(clouds)])
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(len(coords), cin, generator=g)
    return ME.SparseTensor(feats, coordinates=torch.from_numpy(coords).int(), device=gpu)


def _bf(t):
    return t.to(torch.bfloat16).double()


def _ref_wgrad(fin, dy, nbr, V_out):
    """dW[k] = sum over o with i = nbr[k][o] >= 0 of bf16(fin[i])^T bf16(dy[o]) in float64, and the same on |.|"""
    a, b = _bf(fin), _bf(dy)
    K = nbr.shape[0]
    want = torch.zeros((K, fin.shape[1], dy.shape[1]), dtype=torch.float64, device=fin.device)
    terms = torch.zeros_like(want)
    for k in range(K):
        idx = nbr[k, :V_out].long()
        ok = torch.nonzero(idx >= 0).flatten()
        want[k] = a[idx[ok]].t() @ b[ok]
        terms[k] = a[idx[ok]].abs().t() @ b[ok].abs()
    return want, terms


def _check(name, got, want, terms):
    err = (got.double() - want).abs()
    bound = C_BOUND * 1e-7 * terms + 1e-30
    margin = float((err / bound).max())
    print(f"{name}: max |err| {float(err.max()):.3e}, margin {margin:.3f} of the bound (C = {C_BOUND})")
    assert margin <= 1.0, (name, margin)


def _wgrad_bf16(fin, dy, plan, K, cin, cout):
    from mrcc_amd import nn as svnn

    used = set()
    dw = svnn.conv_wgrad(fin, dy, plan, K, cin, cout, bf16=True, used=used)
    assert used == {"sv_conv_wgrad_bf16"}, used
    return dw


def _case(gpu, name, fin, plan, V_out, cout, K, seed=9):
    whole = plan.whole if hasattr(plan, "whole") else plan
    nbr = whole.raw[0] if whole is not None else torch.arange(V_out, device=gpu, dtype=torch.int32)[None]
    dy = torch.randn((V_out, cout), generator=torch.Generator().manual_seed(seed)).to(gpu)
    dw = _wgrad_bf16(fin, dy, plan, K, fin.shape[1], cout)
    want, terms = _ref_wgrad(fin, dy, nbr, V_out)
    _check(name, dw, want, terms)
    return dw, dy


def test_k27_split_passes_against_float64(gpu):
    from mrcc_amd import nn as svnn

    for cin, cout, n in ((64, 64, 1500), (384, 384, 700)):
        x = _tensor(gpu, [_cloud(4, n)], cin)
        cm = x.coordinate_manager
        plan = cm.plan_k3_split(1, (9, 18))
        assert isinstance(plan, svnn.SplitPlan)
        _case(gpu, f"k27 {cin}->{cout} split", x.F, plan, x.F.shape[0], cout, 27)


def test_k27_decoder_cat_column_slice(gpu):
    x = _tensor(gpu, [_cloud(6, 500)], 480)
    fin = x.F[:, :416]  # the left columns of a concatenated buffer: row stride 480
    assert fin.stride(0) == 480
    _case(gpu, "k27 416->384 (slice of 480)", fin, x.coordinate_manager.plan_k3(1), x.F.shape[0], 384, 27)


def test_k8_down_and_transposed_up(gpu):
    x = _tensor(gpu, [_cloud(1, 1500)], 64)
    cm = x.coordinate_manager
    down = cm.plan_down(1)
    V2 = cm.stride_map(2).V
    _case(gpu, "k8 64->128 down", x.F, down, V2, 128, 8)
    f2 = torch.randn(V2, 96, generator=torch.Generator().manual_seed(3)).to(gpu)
    _case(gpu, "k8 96->64 up", f2, cm.plan_up(2), x.F.shape[0], 64, 8)


def test_dense_256_to_1024_and_odd_row_count(gpu):
    for V in (1037, 4099):
        assert V % 32 != 0
        fin = torch.randn(V, 256, generator=torch.Generator().manual_seed(V)).to(gpu)
        _case(gpu, f"dense 256->1024, {V} rows", fin, None, V, 1024, 1)


def test_two_frames_and_sparse_skipped_subtiles(gpu):
    x = _tensor(gpu, [_cloud(7, 1200), _cloud(8, 800)], 64)
    _case(gpu, "k27 64->96 two frames", x.F, x.coordinate_manager.plan_k3(1), x.F.shape[0], 96, 27)
    x = _tensor(gpu, [_scatter_cloud(2, 3000)], 128)
    plan = x.coordinate_manager.plan_k3(1)
    sm = plan.submask.view(-1, 27)[:, [k for k in range(27) if k != 13]] & 0xFF
    assert float((sm == 0).float().mean()) > 0.5, "the cloud is not sparse enough to skip sub-tiles"
    assert x.F.shape[0] % 32 != 0
    _case(gpu, "k27 128->64 scattered voxels", x.F, plan, x.F.shape[0], 64, 27)


def test_wgrad_bf16_deterministic_and_accumulate(gpu):
    from mrcc_amd import nn as svnn

    x = _tensor(gpu, [_cloud(3, 1500)], 64)
    plan = x.coordinate_manager.plan_k3(1)
    V = x.F.shape[0]
    g = torch.Generator().manual_seed(11)
    dya, dyb = torch.randn(V, 96, generator=g).to(gpu), torch.randn(V, 96, generator=g).to(gpu)
    fin = x.F.detach()
    dwa = _wgrad_bf16(fin, dya, plan, 27, 64, 96)
    assert torch.equal(_wgrad_bf16(fin, dya, plan, 27, 64, 96), dwa)
    dwb = _wgrad_bf16(fin, dyb, plan, 27, 64, 96)
    acc = dwa.clone()
    assert svnn._wgrad_one(fin, dyb, plan, 27, 64, 96, V, acc, True, bf16=True) == "sv_conv_wgrad_bf16"
    assert torch.equal(acc, dwa + dwb)
    junk = torch.full_like(dwa, float("nan"))
    svnn._wgrad_one(fin, dya, plan, 27, 64, 96, V, junk, False, bf16=True)
    assert torch.equal(junk, dwa)
    # the bf16 result differs from the fp32 kernel's (operands are rounded) - the path really is a different one
    assert not torch.equal(svnn.conv_wgrad(fin, dya, plan, 27, 64, 96), dwa)


def test_wgrad_bf16_nan_and_inf(gpu):
    x = _tensor(gpu, [_cloud(12, 1500)], 64)
    plan = x.coordinate_manager.plan_k3(1)
    nbr = plan.raw[0]
    V = x.F.shape[0]
    dy = torch.randn(V, 64, generator=torch.Generator().manual_seed(2)).to(gpu)
    counts = torch.zeros((27, V), dtype=torch.int64, device=gpu)
    for k in range(27):
        idx = nbr[k, :V].long()
        idx = idx[idx >= 0]
        counts[k].index_add_(0, idx, torch.ones_like(idx))
    # a row with pairs at some offsets but not all (a boundary voxel)
    part = ((counts > 0).sum(0) < 27) & ((counts > 0).sum(0) > 1)
    row = int(torch.nonzero(part)[0])
    fin = x.F.detach().clone()
    fin[row, 5] = float("nan")
    dw = _wgrad_bf16(fin, dy, plan, 27, 64, 64)
    want = torch.zeros_like(dw, dtype=torch.bool)
    want[:, 5, :] = (counts[:, row] > 0)[:, None]
    assert torch.equal(torch.isnan(dw), want)
    # inf in a row that has no pair at offset k: dW[k] stays finite
    k_free = int(torch.nonzero(counts[:, row] == 0)[0])
    fin = x.F.detach().clone()
    fin[row, :] = float("inf")
    dw = _wgrad_bf16(fin, dy, plan, 27, 64, 64)
    assert torch.isfinite(dw[k_free]).all()
    assert not torch.isfinite(dw[13]).all()  # the centre offset pairs every row with itself


# ---------------------------------------------------------------------------------------------------------------------
# whole networks
# ---------------------------------------------------------------------------------------------------------------------
def _seg_model(gpu, seed=1):
    from mrcc_amd.model.backbone.minkunet import MinkUNet14A
    from mrcc_amd.model.robotnet_segmentation import _classification_head

    torch.manual_seed(seed)
    return _classification_head(MinkUNet14A, lambda: 3, "SegHead14A")(3, num_classes=3).to(gpu)


def _input(gpu, clouds=None):
    clouds = clouds or [_cloud(8, 2000), _cloud(9, 1000)]
    coords = np.concatenate([np.concatenate([np.full((len(c), 1), b), c], 1) for b, c in enumerate(clouds)])
    feats = torch.rand(len(coords), 3, generator=torch.Generator().manual_seed(4)) - 0.5
    return feats, torch.from_numpy(coords).int()


def _grads(model, gpu, feats, coords, labels):
    from mrcc_amd import MinkowskiEngine as ME

    model.zero_grad(set_to_none=True)
    out = model(ME.SparseTensor(feats, coordinates=coords, device=gpu))
    torch.nn.functional.cross_entropy(out.F, labels).backward()
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def test_bf16_training_gradients_match_fp32(gpu):
    """bf16 against fp32 training gradients, same weights and input, batch-statistics BN.  A random-init U-Net amplifies
    any perturbation of this size: fp32 training on the input rounded to bf16 (one rounding of three channels) moves
    the gradients by 10-25 % per parameter, so the bound is relative to that control - the worst and the
    median relative Frobenius error of the bf16 gradients stay within 2.5x of the control's."""
    from mrcc_amd import nn as svnn

    feats, coords = _input(gpu)
    labels = torch.randint(0, 3, (feats.shape[0],), generator=torch.Generator().manual_seed(1)).to(gpu)
    ref, model, ctl = _seg_model(gpu).train(), _seg_model(gpu).train(), _seg_model(gpu).train()
    marked = svnn.set_training_precision(model, "bf16")
    assert marked
    want = _grads(ref, gpu, feats, coords, labels)
    assert all(torch.equal(want[n], g) for n, g in _grads(ref, gpu, feats, coords, labels).items()), "fp32 not repeatable"
    got = _grads(model, gpu, feats, coords, labels)
    control = _grads(ctl, gpu, feats.to(torch.bfloat16).float(), coords, labels)
    assert set(got) == set(want) == set(control)

    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))

    errs = sorted((rel(got[n], want[n]), n) for n in want)
    ctl_errs = sorted(rel(control[n], want[n]) for n in want)
    worst, median = errs[-1], errs[len(errs) // 2][0]
    print(f"{len(marked)} bf16 layers, {len(errs)} parameters: worst relative Frobenius error {worst[0]:.3e} ({worst[1]}), "
          f"median {median:.3e}; control (fp32, bf16-rounded input): worst {ctl_errs[-1]:.3e}, "
          f"median {ctl_errs[len(ctl_errs) // 2]:.3e}; {sum(e <= NET_REL_TOL for e, _ in errs)} parameters within "
          f"{NET_REL_TOL}")
    assert worst[0] <= 2.5 * ctl_errs[-1], worst
    assert median <= 2.5 * ctl_errs[len(ctl_errs) // 2], median


def _run_logged_step(gpu, model):
    from mrcc_amd import profiling

    feats, coords = _input(gpu)
    labels = torch.randint(0, 3, (feats.shape[0],), generator=torch.Generator().manual_seed(1)).to(gpu)
    profiling.TRAIN_LOG = []
    try:
        _grads(model, gpu, feats, coords, labels)
        return profiling.TRAIN_LOG
    finally:
        profiling.TRAIN_LOG = None


def test_dispatch_exactly_the_marked_layers_run_bf16(gpu):
    from mrcc_amd import nn as svnn

    model = _seg_model(gpu).train()
    marked = set(svnn.set_training_precision(model, "bf16"))
    names = {m: n for n, m in model.named_modules()}
    log = _run_logged_step(gpu, model)
    layers = {n for n, m in model.named_modules() if isinstance(m, (svnn._ConvBase, svnn.MinkowskiLinear))}
    seen = {}
    for layer, op, fn in log:
        seen.setdefault(names[layer], {})[op] = fn
    assert set(seen) == layers
    for n, ops in seen.items():
        m = model.get_submodule(n)
        cin, cout, K = svnn._layer_channels(m)
        if n in marked:
            assert ops["fwd"] == "sv_conv_fwd_bf16" and ops["dw"] == "sv_conv_wgrad_bf16", (n, ops)
            swapped_ok = (cout % 32 == 0 and cout >= 64 and cin % 16 == 0 and cin >= 64
                          and (cin % 128 == 0 or cin % 192 == 0))
            if "dx" in ops:
                assert ops["dx"] == ("sv_conv_fwd_bf16" if swapped_ok else "sv_conv_fwd_acc"), (n, ops)
        else:
            assert ops["fwd"] == "sv_conv_fwd_acc" and ops["dw"] == "sv_conv_wgrad", (n, ops)
            assert ops.get("dx", "sv_conv_fwd_acc") == "sv_conv_fwd_acc", (n, ops)
    assert sum("dx" in ops and ops["dx"] == "sv_conv_fwd_bf16" for ops in seen.values()) > 0
    # the fp32 default: nothing ran bf16
    ref = _seg_model(gpu).train()
    assert all("bf16" not in fn for _, _, fn in _run_logged_step(gpu, ref))


class _Thin(torch.nn.Module):
    """every layer 32 wide: nothing is bf16_eligible"""

    def __init__(self):
        super().__init__()
        from mrcc_amd import MinkowskiEngine as ME

        self.conv0 = ME.MinkowskiConvolution(3, 32, kernel_size=3, dimension=3)
        self.bn0 = ME.MinkowskiBatchNorm(32)
        self.relu = ME.MinkowskiReLU()
        self.conv1 = ME.MinkowskiConvolution(32, 32, kernel_size=3, dimension=3)
        self.down = ME.MinkowskiConvolution(32, 32, kernel_size=2, stride=2, dimension=3)
        self.up = ME.MinkowskiConvolutionTranspose(32, 32, kernel_size=2, stride=2, dimension=3)
        self.lin = ME.MinkowskiOps.MinkowskiLinear(32, 3)

    def forward(self, x):
        x = self.relu(self.bn0(self.conv0(x)))
        x = self.relu(self.conv1(x))
        return self.lin(self.up(self.down(x)))


def test_fallbacks_are_bit_identical_to_fp32(gpu):
    from mrcc_amd import nn as svnn

    feats, coords = _input(gpu)
    labels = torch.randint(0, 3, (feats.shape[0],), generator=torch.Generator().manual_seed(1)).to(gpu)
    torch.manual_seed(3)
    a = _Thin().to(gpu).train()
    torch.manual_seed(3)
    b = _Thin().to(gpu).train()
    assert svnn.set_training_precision(b, "bf16") == []
    ga, gb = _grads(a, gpu, feats, coords, labels), _grads(b, gpu, feats, coords, labels)
    assert set(ga) == set(gb) and all(torch.equal(ga[n], gb[n]) for n in ga)
    # set_compute_precision affects eval alone
    ref, model = _seg_model(gpu).train(), _seg_model(gpu).train()
    assert svnn.set_compute_precision(model, "bf16")
    ga, gb = _grads(ref, gpu, feats, coords, labels), _grads(model, gpu, feats, coords, labels)
    assert set(ga) == set(gb) and all(torch.equal(ga[n], gb[n]) for n in ga)


@pytest.mark.parametrize("eval_precision", ["fp32", "bf16"])
def test_eval_after_bf16_training_is_bit_identical_to_a_fresh_model(gpu, eval_precision):
    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd import nn as svnn

    model = _seg_model(gpu)
    svnn.set_training_precision(model, "bf16")
    svnn.set_compute_precision(model, eval_precision)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    feats, coords = _input(gpu)
    labels = torch.randint(0, 3, (feats.shape[0],), generator=torch.Generator().manual_seed(1)).to(gpu)
    model.eval()
    with torch.no_grad():
        before = model(ME.SparseTensor(feats, coordinates=coords, device=gpu)).F.clone()  # fills the eval caches
    model.train()
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
    svnn.set_compute_precision(fresh, eval_precision)
    fresh.eval()
    with torch.no_grad():
        want = fresh(ME.SparseTensor(feats, coordinates=coords, device=gpu)).F
    assert not torch.equal(got, before), "the optimizer steps changed nothing"
    assert torch.equal(got, want), "a packed-weight cache kept the pre-step weights"


def test_reference_train_epoch_loop_reduces_the_loss_in_bf16(gpu):
    """train_segmentation.py's train_epoch (as tests/test_gpu_training.py runs it) with set_training_precision("bf16")"""
    import mrcc_amd
    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd import nn as svnn

    cs, fs, ls = [], [], []
    for seed in range(2):
        sc = mrcc_amd.synth.gen_scene(seed, n_bg=6000, n_arm=2000, n_ee=2000, keyed_colors=True)
        c, f, lab = ME.utils.sparse_quantize(sc["points"], sc["rgb"], labels=sc["segmentation"], ignore_label=-100,
                                             quantization_size=0.04)
        cs.append(torch.from_numpy(np.asarray(c)))
        fs.append(np.asarray(f) - 0.5)
        ls.append(np.asarray(lab))
    coords = ME.utils.batched_coordinates(cs)
    feats = torch.from_numpy(np.concatenate(fs).astype(np.float32))
    labels = torch.from_numpy(np.concatenate(ls).astype(np.int64)).to(gpu)
    curves = {}
    for precision in ("fp32", "bf16"):
        model = _seg_model(gpu, seed=7).train()
        svnn.set_training_precision(model, precision)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        criterion = torch.nn.CrossEntropyLoss(ignore_index=-100)
        losses = []
        for _ in range(30):
            out = model(ME.SparseTensor(feats, coordinates=coords, device=gpu))
            opt.zero_grad()
            loss = criterion(out.F, labels)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        curves[precision] = losses
        print(f"{precision} loss: " + " ".join(f"{v:.3f}" for v in losses))
    losses = curves["bf16"]
    print(f"bf16: first step {losses[0]:.4f}, after {len(losses)} steps {losses[-1]:.4f} "
          f"({losses[-1] / losses[0]:.2f} of the first; fp32 {curves['fp32'][-1] / curves['fp32'][0]:.2f})")
    assert losses[-1] < 0.5 * losses[0]
