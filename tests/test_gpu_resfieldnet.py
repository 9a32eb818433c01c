"""ResFieldNet14 / ResFieldNet50 (model/backbone/resnet.py): two field networks on the points, then the ResNet trunk.

The cloud is three frames inside the box of tests/test_gpu_resnet_dense.py (it survives the trunk's total stride of 192 with
at least three live stride-192 rows per frame, so the last instance norm is not its degenerate case), two to three points
per voxel.  eval(): the fused path (one sv_field_stage per field network) against the module path and against a float64
restatement of the two stages, relative max-abs error <= max(1e-4, 8 * d32), d32 = the two stages evaluated by torch in
float32 on the CPU against float64."""
import numpy as np
import pytest
import torch

import field_helpers as FH
import hostile_helpers as HH
import strided_helpers as H

pytestmark = pytest.mark.gpu

BOX_LO, BOX_HI = (-128, -192, -128), (64, -128, 64)
NETS = ["ResFieldNet14", "ResFieldNet50"]
_cache = {}


def _cloud():
    if "cloud" not in _cache:
        rng = np.random.default_rng(11)
        frames = []
        for b, n in ((0, 1500), (1, 1100), (2, 1300)):
            centres = [(x, -160 + 6 * b, z) for x in (-98 + 5 * b, 24) for z in (-95, 20 + 6 * b)]
            vox = H.blob_cloud(rng, n, centres, 9.0, BOX_LO, BOX_HI)
            vox = np.concatenate([vox, vox[rng.permutation(n)[: n // 2]], vox[rng.permutation(n)[: n // 3]]])  # 1 to 3 points each
            frames.append(np.concatenate([np.full((len(vox), 1), b), vox], 1))
        pts = np.concatenate(frames).astype(np.int64)
        for b in range(3):  # the set-up of tests/test_gpu_resnet_dense.py: at least three stride-192 voxels with inputs per frame
            c = pts[pts[:, 0] == b][:, 1:]
            c64, top = np.unique(c // 64 * 64, axis=0), np.unique(c // 192 * 192, axis=0)
            assert sum((np.abs(c64 - o).max(1) <= 64).any() for o in top) >= 3
        pts = pts[rng.permutation(len(pts))]
        coords = pts.astype(np.float32)
        coords[:, 1:] += rng.uniform(0.05, 0.95, size=(len(pts), 3)).astype(np.float32)
        feats = rng.standard_normal((len(pts), 3)).astype(np.float32)
        _cache["cloud"] = (pts, torch.from_numpy(coords), torch.from_numpy(feats))
    return _cache["cloud"]


def _model(name, gpu):
    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd.model.backbone import resnet as R

    if name not in _cache:
        torch.manual_seed(3)
        model = getattr(R, name)(3, 5)
        g = torch.Generator().manual_seed(4)
        with torch.no_grad():
            for m in model.modules():
                if isinstance(m, ME.MinkowskiBatchNorm):
                    n = m.bn.num_features
                    m.bn.running_mean.copy_(torch.randn(n, generator=g) * 0.2)
                    m.bn.running_var.copy_(torch.rand(n, generator=g) + 0.5)
                    m.bn.weight.copy_(torch.rand(n, generator=g) + 0.5)
                    m.bn.bias.copy_(torch.randn(n, generator=g) * 0.2)
        _cache[name] = model.to(gpu).eval()
    return _cache[name]


def _field(gpu, rows=None):
    from mrcc_amd import MinkowskiEngine as ME

    _, coords, feats = _cloud()
    if rows is not None:
        coords, feats = coords[rows].clone(), feats[rows]
        coords[:, 0] = 0
    return ME.TensorField(feats, coords, device=gpu)


def _forward(model, field, fuse):
    """logits and the trunk's input features ([V, 64]) of one eval() forward, with the entry-point counts"""
    seen = []
    hook = model.conv1[0].register_forward_pre_hook(lambda mod, args: seen.append(args[0].F))
    type(model).FUSE_FIELD, before = fuse, type(model).FUSE_FIELD
    try:
        with torch.no_grad(), HH.entry_calls() as calls:
            logits = model(field)
    finally:
        type(model).FUSE_FIELD = before
        hook.remove()
    return logits.cpu(), seen[0].cpu(), calls


def _stage_params(model, net):
    sd = {k: v.detach().cpu() for k, v in getattr(model, net).state_dict().items()}
    bn = lambda i: dict(weight=sd[f"{i}.bn.weight"], bias=sd[f"{i}.bn.bias"], mean=sd[f"{i}.bn.running_mean"],  # noqa: E731
                        var=sd[f"{i}.bn.running_var"])
    return dict(kernel=sd["0.kernel"], bias=sd["0.bias"].reshape(-1), coef=sd["0.coef"].reshape(-1), bn1=bn(1),
                weight=sd["3.linear.weight"], lin_bias=sd["3.linear.bias"], bn2=bn(4))


def _stages_ref(model, dtype):
    pts, _, feats = _cloud()
    inverse, V = FH.voxelize_ref(pts)
    o1 = FH.stage_ref(feats, _stage_params(model, "field_network"), inverse, V, dtype)
    return FH.stage_ref(feats, _stage_params(model, "field_network2"), inverse, V, dtype, o1)


@pytest.mark.parametrize("name", NETS)
def test_fused_field_stages_match_the_module_path_and_float64(gpu, name):
    model = _model(name, gpu)
    fused, trunk_in, calls = _forward(model, _field(gpu), True)
    plain, plain_in, plain_calls = _forward(model, _field(gpu), False)
    assert calls["sv_field_stage"] == 2 and calls["sv_sinusoidal"] == 0 and calls["sv_voxelize"] == 1
    assert plain_calls["sv_field_stage"] == 0 and plain_calls["sv_sinusoidal"] == 2 and plain_calls["sv_voxelize"] == 1
    want = _stages_ref(model, torch.float64)
    d32 = float((_stages_ref(model, torch.float32).double() - want).abs().max() / want.abs().max())
    bound = max(1e-4, 8 * d32)
    err_in = float((trunk_in.double() - want).abs().max() / want.abs().max())
    err_plain_in = float((plain_in.double() - want).abs().max() / want.abs().max())
    err = float((fused.double() - plain.double()).abs().max() / plain.double().abs().max())
    print(f"{name}: d32 = {d32:.3e}, bound = {bound:.3e}; trunk input vs float64: fused {err_in:.3e}, modules {err_plain_in:.3e}; "
          f"logits fused vs modules: {err:.3e}")
    assert fused.shape == (3, 5) and torch.isfinite(fused).all() and trunk_in.shape == want.shape
    assert err_in <= bound and err_plain_in <= bound
    assert err <= bound


@pytest.mark.parametrize("name", NETS)
def test_batched_logits_are_each_frames_alone(gpu, name):
    model = _model(name, gpu)
    pts, _, _ = _cloud()
    batched, _, _ = _forward(model, _field(gpu), True)
    for b in range(3):
        alone, _, _ = _forward(model, _field(gpu, rows=np.nonzero(pts[:, 0] == b)[0]), True)
        assert torch.equal(FH.bits(alone[0]), FH.bits(batched[b])), f"frame {b}"


@pytest.mark.parametrize("name", NETS)
def test_state_dict_round_trip(gpu, name):
    from mrcc_amd.model.backbone import resnet as R

    model = _model(name, gpu)
    torch.manual_seed(99)
    other = getattr(R, name)(3, 5).to(gpu).eval()
    result = other.load_state_dict(model.state_dict())
    assert not result.missing_keys and not result.unexpected_keys
    a, _, _ = _forward(model, _field(gpu), True)
    b, _, _ = _forward(other, _field(gpu), True)
    assert torch.equal(FH.bits(a), FH.bits(b))


@pytest.mark.parametrize("name", NETS)
def test_train_forward_backward_fills_every_gradient(gpu, name):
    import copy

    model = copy.deepcopy(_model(name, gpu)).train()
    with HH.entry_calls() as calls:
        logits = model(_field(gpu))
        logits.square().sum().backward()
    assert calls["sv_field_stage"] == 0 and calls["sv_voxelize"] == 1  # train(): module by module, one voxelisation
    assert logits.shape == (3, 5) and torch.isfinite(logits).all()
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert float(model.field_network[0].kernel.grad.abs().max()) > 0 and float(model.field_network2[0].coef.grad.abs().max()) > 0


def test_unsupported_widths_take_the_module_path(gpu):
    """a field network the fused kernel does not cover (C = 48): SV_ERR_UNSUPPORTED, then module by module"""
    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd import nn as svnn
    from mrcc_amd.model.backbone.resnet import ResFieldNetBase

    torch.manual_seed(5)
    seq = torch.nn.Sequential(ME.MinkowskiSinusoidal(3, 48), ME.MinkowskiBatchNorm(48), ME.MinkowskiReLU(), ME.MinkowskiLinear(48, 48),
                              ME.MinkowskiBatchNorm(48), ME.MinkowskiReLU(), ME.MinkowskiToSparseTensor()).to(gpu).eval()
    assert svnn.is_field_stage(seq)
    with torch.no_grad(), HH.entry_calls() as calls:
        out = ResFieldNetBase._run_field(ResFieldNetBase, seq, _field(gpu))
    assert calls["sv_field_stage"] == 1 and calls.ok.get("sv_field_stage", 0) == 0 and calls["sv_sinusoidal"] == 1
    pts, _, feats = _cloud()
    inverse, V = FH.voxelize_ref(pts)
    sd = {k: v.detach().cpu() for k, v in seq.state_dict().items()}
    bn = lambda i: dict(weight=sd[f"{i}.bn.weight"], bias=sd[f"{i}.bn.bias"], mean=sd[f"{i}.bn.running_mean"],  # noqa: E731
                        var=sd[f"{i}.bn.running_var"])
    p = dict(kernel=sd["0.kernel"], bias=sd["0.bias"].reshape(-1), coef=sd["0.coef"].reshape(-1), bn1=bn(1), weight=sd["3.linear.weight"],
             lin_bias=sd["3.linear.bias"], bn2=bn(4))
    want = FH.stage_ref(feats, p, inverse, V, torch.float64)
    d32 = float((FH.stage_ref(feats, p, inverse, V, torch.float32).double() - want).abs().max() / want.abs().max())
    assert float((out.F.cpu().double() - want).abs().max() / want.abs().max()) <= max(1e-4, 8 * d32)
