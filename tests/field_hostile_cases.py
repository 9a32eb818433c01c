"""Hostile-environment cases of the field front end (sv_sinusoidal, sv_field_stage), in a file of their own: importing
this module registers them in the one table of tests/hostile_cases.py (its `case`), so tests/test_gpu_hostile_memory.py and
tests/test_gpu_side_stream.py run them like every other case and tests/test_hostile_cpu.py counts their entry points.

The table is complete only once this module has been imported.  tests/test_field_cpu.py imports it, and that file is collected
before the three modules that read the table (pytest collects a directory in name order, every file before any test runs), so a run
of the suite sees the cases; a run of tests/test_hostile_cpu.py alone does not, and its completeness test then names the two
entries as "without a case"."""
import numpy as np
import torch

from hostile_cases import CASES, _arm, _randomise_bn, _t, _two_frames, case

ENTRIES = ("sv_sinusoidal", "sv_field_stage")


# the sinusoidal layer on its own (N = 1025, 35 -> 64)
def _sin_build(gpu):
    g = torch.Generator().manual_seed(31)
    r = lambda *s: torch.randn(*s, generator=g).to(gpu)  # noqa: E731
    return dict(x=r(1025, 35) * 10, kernel=r(35, 64), bias=r(64), coef=r(64))


def _sin_run(i):
    from mrcc_amd import nn as svnn

    return (svnn.sinusoidal(i["x"], i["kernel"], i["bias"], i["coef"]),)


def _sin_ref(i, outs):
    import field_helpers as FH

    x, k, b, c = (i[n].cpu() for n in ("x", "kernel", "bias", "coef"))
    want = FH.sinusoidal_ref(x.double(), k.double(), b.double(), c.double())
    assert bool(((outs[0].double() - want).abs() <= FH.sinusoidal_bound(x, k, b, c, want)).all())


# both field networks of a ResFieldNet as fused stages on the two-frame batch of hostile_cases (3 -> 32, then 35 -> 64)
def _field_nets():
    from mrcc_amd import MinkowskiEngine as ME

    torch.manual_seed(32)
    nets = [torch.nn.Sequential(ME.MinkowskiSinusoidal(cin, c), ME.MinkowskiBatchNorm(c), ME.MinkowskiReLU(), ME.MinkowskiLinear(c, c),
                                ME.MinkowskiBatchNorm(c), ME.MinkowskiReLU(), ME.MinkowskiToSparseTensor()) for cin, c in ((3, 32), (35, 64))]
    for n, net in enumerate(nets):
        _randomise_bn(net, 33 + n)
    return nets


def _field_build(gpu):
    c, V = _two_frames()
    g = torch.Generator().manual_seed(35)
    return dict(coords=_t(c.astype(np.float32) + np.float32(0.5), gpu), feats=torch.randn(len(c), 3, generator=g).to(gpu),
                nets=[net.to(gpu).eval() for net in _field_nets()], V=V, ints=c)


def _field_run(i):
    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd import nn as svnn

    field = ME.TensorField(i["feats"], i["coords"], device=i["feats"].device)
    _, inverse, order, seg_start = field.voxelisation()
    _arm(i, i["feats"], order, seg_start)
    o1 = svnn.field_stage(i["nets"][0], field)
    _arm(i, i["feats"], o1.F, inverse, order, seg_start)
    o2 = svnn.field_stage(i["nets"][1], field, o1)
    return o1.F, o2.F


def _field_ref(i, outs):
    import field_helpers as FH

    inverse, V = FH.voxelize_ref(i["ints"])
    G, F = None, i["feats"].cpu()
    for net, got in zip(i["nets"], outs):
        sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
        bn = lambda j: dict(weight=sd[f"{j}.bn.weight"], bias=sd[f"{j}.bn.bias"], mean=sd[f"{j}.bn.running_mean"],  # noqa: E731
                            var=sd[f"{j}.bn.running_var"])
        p = dict(kernel=sd["0.kernel"], bias=sd["0.bias"].reshape(-1), coef=sd["0.coef"].reshape(-1), bn1=bn(1),
                 weight=sd["3.linear.weight"], lin_bias=sd["3.linear.bias"], bn2=bn(4))
        want = FH.stage_ref(F, p, inverse, V, torch.float64, G)
        d32 = float((FH.stage_ref(F, p, inverse, V, torch.float32, G).double() - want).abs().max() / want.abs().max())
        assert float((got.double() - want).abs().max() / want.abs().max()) <= max(1e-4, 8 * d32)
        G = want.float()  # the next stage's voxel features: the reference's own


if not any(c.name in ("sinusoidal", "field_stages") for c in CASES):  # once, however often the module is loaded
    case("sinusoidal", ["sv_sinusoidal"], _sin_build, _sin_run, late=("x", "kernel", "bias", "coef"), reference=_sin_ref)
    case("field_stages", ["sv_field_stage", "sv_voxelize"], _field_build, _field_run, late=("coords", "feats"), reference=_field_ref,
         steps=3)
