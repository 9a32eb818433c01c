"""The field front end without a GPU: host validation of sv_sinusoidal / sv_field_stage (it precedes every HIP call), the
ResFieldNets' state-dict layout, and the error bound of the sinusoidal tests held against a plain float32 evaluation."""
import torch

import field_helpers as FH
import field_hostile_cases as FC  # registers the field front end's cases in the hostile-environment table (see its docstring)


def _lib():
    import mrcc_amd

    return mrcc_amd._lib.load()


def _sin(lib, x=1, N=5, Cin=3, Cout=4, ld=None, out_ld=None, ptrs=1):
    a = 64 if ptrs else None  # any non-null address: validation fails before it is looked at
    return lib.sv_sinusoidal(a if x else None, Cin if ld is None else ld, Cin, N, a, a, a, Cout, a, Cout if out_ld is None else out_ld, None)


def _stage(lib, C=64, Cg=32, Cf=3, N=10, V=5, ptrs=0, G=None, f_ld=None):
    a = 64 if ptrs else None
    g = a if G is None else G
    return lib.sv_field_stage(a, Cf if f_ld is None else f_ld, Cf, N, g if Cg else None, Cg, Cg, g if Cg else None, a, a, a, a, a, a, None, a,
                              a, C, a, a, V, a, C, None)


def test_sinusoidal_host_validation():
    lib = _lib()
    assert _sin(lib, ptrs=0) == -1 and b"null pointer" in lib.sv_last_error()
    assert _sin(lib, x=0) == -1 and b"null pointer" in lib.sv_last_error()
    for bad in (dict(Cin=0), dict(Cout=0), dict(N=-1), dict(ld=2), dict(out_ld=3)):
        assert _sin(lib, **bad) == -1 and b"bad shape" in lib.sv_last_error(), bad
    assert _sin(lib, N=0, ptrs=0) == 0  # N = 0 is valid, whatever the pointers


def test_field_stage_host_validation():
    lib = _lib()
    assert _stage(lib) == -1 and b"null pointer" in lib.sv_last_error()
    assert _stage(lib, ptrs=1, G=0) == -1 and b"null pointer" in lib.sv_last_error()  # Cg > 0 needs G and inverse
    for bad in (dict(Cf=0), dict(Cg=-1), dict(C=0), dict(N=-1), dict(V=-1), dict(V=11), dict(f_ld=2)):
        assert _stage(lib, ptrs=1, **bad) == -1 and b"bad shape" in lib.sv_last_error(), bad
    assert _stage(lib, N=10, V=0) == -1 and _stage(lib, N=0, V=0) == 0  # an empty field is valid
    assert _stage(lib, Cg=0, N=0, V=0) == 0


def test_field_stage_unsupported_shapes_are_reported_before_anything_else():
    from mrcc_amd import _lib as L

    lib = _lib()
    assert _stage(lib, C=48) == L.SV_ERR_UNSUPPORTED == -5 and b"outside the fused kernel" in lib.sv_last_error()
    assert _stage(lib, Cg=126, Cf=3) == L.SV_ERR_UNSUPPORTED
    assert _stage(lib, Cg=125, Cf=3) == -1 and b"null pointer" in lib.sv_last_error()  # 128 inputs are covered
    assert _stage(lib, C=32, Cg=0) == -1 and b"null pointer" in lib.sv_last_error()


def test_reduce_sum_is_a_mode():
    from mrcc_amd import _lib as L

    lib = _lib()
    assert L.SV_REDUCE_SUM == 2
    assert lib.sv_voxel_reduce(None, 3, None, None, 4, L.SV_REDUCE_SUM, None, None) == -1 and b"null pointer" in lib.sv_last_error()
    assert lib.sv_voxel_reduce(None, 3, None, None, 4, 3, None, None) == -1 and b"bad mode" in lib.sv_last_error()


def test_resfieldnet_state_dict_layout():
    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd.model.backbone import resnet as R

    torch.manual_seed(0)
    model = R.ResFieldNet14(3, 5)
    keys = list(model.state_dict())
    bn = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
    field = (["0.kernel", "0.bias", "0.coef"] + [f"1.bn.{k}" for k in bn] + ["3.linear.weight", "3.linear.bias"]
             + [f"4.bn.{k}" for k in bn])
    want = [f"field_network.{k}" for k in field] + [f"field_network2.{k}" for k in field]
    assert keys[:len(want)] == want
    assert keys[len(want):] == list(R.ResNet14(64, 5).state_dict())
    sd = model.state_dict()
    assert sd["field_network.0.kernel"].shape == (3, 32) and sd["field_network.0.bias"].shape == (1, 32)
    assert sd["field_network.0.coef"].shape == (1, 32)
    assert model.field_network2[0].kernel.shape == (35, 64)
    assert isinstance(model.field_network[6], ME.MinkowskiToSparseTensor)
    for name, layers, block in (("ResFieldNet18", (2, 2, 2, 2), ME.BasicBlock), ("ResFieldNet34", (3, 4, 6, 3), ME.BasicBlock),
                                ("ResFieldNet50", (3, 4, 6, 3), ME.Bottleneck), ("ResFieldNet101", (3, 4, 23, 3), ME.Bottleneck)):
        cls = getattr(R, name)
        assert issubclass(cls, R.ResFieldNetBase) and cls.LAYERS == layers and cls.BLOCK is block and cls.FUSE_FIELD in (True, False)


def test_sinusoidal_parameters_are_drawn_in_order():
    from mrcc_amd import MinkowskiEngine as ME

    torch.manual_seed(5)
    m = ME.MinkowskiSinusoidal(3, 4)
    torch.manual_seed(5)
    want = [torch.randn(3, 4), torch.randn(1, 4), torch.randn(1, 4)]
    assert [n for n, _ in m.named_parameters()] == ["kernel", "bias", "coef"]
    assert all(torch.equal(p, w) for p, w in zip(m.parameters(), want))


def test_field_stage_recogniser():
    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd import nn as svnn
    from mrcc_amd.model.backbone.resnet import ResFieldNet14

    model = ResFieldNet14(3, 5).eval()
    assert svnn.is_field_stage(model.field_network) and svnn.is_field_stage(model.field_network2)
    assert not svnn.is_field_stage(model.conv1)
    assert not svnn.is_field_stage(torch.nn.Sequential(*list(model.field_network)[:6]))
    assert not svnn.is_field_stage(torch.nn.Sequential(*list(model.field_network)[:6], ME.MinkowskiReLU()))
    model.train()
    assert not svnn.is_field_stage(model.field_network)


def test_plain_float32_sinusoidal_stays_inside_the_bound():
    """the bound of tests/test_gpu_sinusoidal.py, checked on a plain float32 evaluation: sequential products and sums, the
    sine of the float32 argument rounded once, one rounding for the product"""
    g = torch.Generator().manual_seed(1)
    worst = {}
    for cin in (1, 3, 35, 67):
        for scale in (1.0, 100.0, 5000.0):
            x = torch.randn(300, cin, generator=g) * scale / max(cin, 1) ** 0.5
            k, b, c = torch.randn(cin, 33, generator=g), torch.randn(33, generator=g), torch.randn(33, generator=g)
            want = FH.sinusoidal_ref(x.double(), k.double(), b.double(), c.double())
            got = FH.sinusoidal_fp32_plain(x, k, b, c).double()
            ratio = float(((got - want).abs() / FH.sinusoidal_bound(x, k, b, c, want)).max())
            worst[cin] = max(worst.get(cin, 0.0), ratio)
    print("largest error / bound of a plain float32 evaluation, by Cin:", {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


def test_the_field_entries_have_hostile_cases_and_the_table_is_complete():
    """both new entry points are reached by a case of the shared table, and with them the table covers every launching entry
    point of _lib.SIGNATURES (what tests/test_hostile_cpu.py asks of it)"""
    import hostile_helpers as HH
    from mrcc_amd import _lib

    cases = {c.name: c for c in HH.CASES}
    assert set(FC.ENTRIES) <= set(cases["sinusoidal"].entries) | set(cases["field_stages"].entries)
    assert [c.name for c in HH.CASES].count("sinusoidal") == 1 and [c.name for c in HH.CASES].count("field_stages") == 1
    covered = set().union(*(c.entries for c in HH.CASES))
    assert covered == HH.launching_entries(_lib.SIGNATURES)
