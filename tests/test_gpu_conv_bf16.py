"""Opt-in bf16 matrix-core path of the wide conv layers (sv_pack_weights_bf16 / sv_conv_fwd_bf16): packing bit for bit,
layers against a float64 sum of the bf16-rounded operands, order independence bit for bit, the kernel report, the
network against fp32 and the engine switch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _cloud(gpu, n=40_000, L=2.4, scale=50, seeds=(0,)):
    import mrcc_amd
    from mrcc_amd import MinkowskiEngine as ME

    parts = []
    for b, sd in enumerate(seeds):
        p, _, _ = mrcc_amd.synth.gen_room(n, L, sd)
        parts.append(np.concatenate([np.full((len(p), 1), b, np.float32), p * np.float32(scale)], axis=1))
    coords4 = np.concatenate(parts)
    rgb = np.zeros((len(coords4), 3), np.float32)
    return ME.TensorField(torch.from_numpy(rgb), torch.from_numpy(coords4), device=gpu).sparse()


def _unpack(wp, K, Cin, Cout):
    """undo the documented fragment order: Wp[((k Cin/32 + cb) Cout/16 + t) 512 + 8 l + j] = W[k][32 cb + 8 (l >> 4) + j][16 t + (l & 15)]"""
    a = wp.reshape(K, Cin // 32, Cout // 16, 4, 16, 8)  # k, cb, t, l >> 4, l & 15, j
    return a.permute(0, 1, 3, 5, 2, 4).reshape(K, Cin, Cout)


def _nbr_table(plan, K, V_out):
    """nbr[k][o] (input row or -1) of a conv plan (None = dense rows)"""
    if plan is None:
        return torch.arange(V_out).reshape(1, V_out)
    perm = plan.perm.cpu().long()
    nbr_s = plan.nbr_s.cpu().long().reshape(K, -1)
    valid = perm >= 0
    nbr = torch.full((K, V_out), -1, dtype=torch.long)
    nbr[:, perm[valid]] = nbr_s[:, valid]
    return nbr


def _check_raw(x, W, plan, V_out, got, rows=2048, seed=0):
    """|gpu - ref| <= 2e-5 sum |a b| on sampled rows, ref = float64 sum of the bf16-rounded operands"""
    K, Cin, Cout = W.shape
    nbr = _nbr_table(plan, K, V_out)
    idx = torch.from_numpy(np.random.default_rng(seed).choice(V_out, size=min(rows, V_out), replace=False))
    xb = torch.cat([x.cpu().to(torch.bfloat16).double(), torch.zeros(1, Cin, dtype=torch.float64)])
    n = nbr[:, idx]
    n = torch.where(n >= 0, n, torch.full_like(n, xb.shape[0] - 1))
    A = xb[n.t()].reshape(len(idx), K * Cin)  # [rows, K Cin]
    Wb = W.cpu().to(torch.bfloat16).double().reshape(K * Cin, Cout)
    ref = A @ Wb
    bound = 2e-5 * (A.abs() @ Wb.abs())
    err = (got.cpu()[idx].double() - ref).abs()
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), f"max err {err.max().item():.3g}, worst err/bound {(err / bound.clamp_min(1e-30)).max().item():.3g}"
    return (err / bound.clamp_min(1e-30)).max().item()


def _weights(K, Cin, Cout, seed, gpu):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(K, Cin, Cout, generator=g) * (2.0 / (K * Cin)) ** 0.5).to(gpu)


def test_pack_weights_bf16_bit_exact(gpu):
    from mrcc_amd import nn as svnn

    K, Cin, Cout = 3, 64, 96
    g = torch.Generator().manual_seed(5)
    W = torch.randn(K, Cin, Cout, generator=g)
    bits = W.view(torch.int32).reshape(-1)
    special = torch.tensor([0x3F808000, 0x3F818000, 0xBF808000, 0x3F80C000, 0x7F7FFFFF,  # ties (to even both ways), max
                            0x7FC00000, 0x7F800000, 0xFF800000,                           # NaN, +Inf, -Inf
                            0x00000001, 0x00400000, 0x80008000, 0x007F8000, 0x00018000, 0x0, 0x80000000],  # denormals, zeros
                           dtype=torch.int64).to(torch.int32)
    bits[: len(special)] = special
    bits[100:100 + len(special)] = special
    wp = svnn.pack_weights_bf16(W.to(gpu))
    assert wp.dtype == torch.bfloat16 and wp.numel() == K * Cin * Cout
    got = _unpack(wp.cpu(), K, Cin, Cout).view(torch.int16)
    want = W.to(torch.bfloat16).view(torch.int16)
    # NaN stays NaN (the hardware convert writes the quiet NaN 0x7FC0 - torch's CPU conversion has a pattern of its own);
    # every other value, ties, infinities, denormals and signed zeros included, is torch's round to nearest even bit for bit
    nan = torch.isnan(W)
    assert torch.isnan(_unpack(wp.cpu(), K, Cin, Cout).float()[nan]).all() and nan.sum() == 2
    bad = ((got != want) & ~nan).reshape(-1).nonzero().reshape(-1)[:8]
    src = W.view(torch.int32).reshape(-1)
    assert bad.numel() == 0, [(hex(int(src[i]) & 0xFFFFFFFF), hex(int(got.reshape(-1)[i]) & 0xFFFF),
                               hex(int(want.reshape(-1)[i]) & 0xFFFF)) for i in bad]


LAYERS = [  # (name, kind, level, Cin, Cout)
    ("k27 level 0 416->384", "k3", 0, 416, 384),
    ("k27 level 1 384->384", "k3", 1, 384, 384),
    ("k27 level 2 448->384", "k3", 2, 448, 384),
    ("k8 down 256->384", "down", 1, 256, 384),
    ("k8 up 384->384", "up", 2, 384, 384),
    ("dense 256->1024", "dense", 0, 256, 1024),
    ("k27 level 1 128->64", "k3", 1, 128, 64),
]


def _plan(st, kind, level):
    cm = st.coordinate_manager
    ts = 2 ** level
    if kind == "k3":
        return cm.plan_k3(ts), ts, ts, 27
    if kind == "down":
        return cm.plan_down(ts // 2), ts // 2, ts, 8
    if kind == "up":
        return cm.plan_up(ts), ts, ts // 2, 8
    return None, ts, ts, 1


@pytest.mark.parametrize("layer", LAYERS, ids=[c[0] for c in LAYERS])
def test_bf16_layer_against_float64(gpu, layer):
    from mrcc_amd import _lib
    from mrcc_amd import nn as svnn

    _, kind, level, Cin, Cout = layer
    st = _cloud(gpu)
    cm = st.coordinate_manager
    for lv in (1, 2):  # the encoder's maps (a transposed conv writes onto one of them)
        cm.stride_map(2 ** lv)
    plan, ts_in, ts_out, K = _plan(st, kind, level)
    V_in, V_out = cm.stride_map(ts_in).V, cm.stride_map(ts_out).V
    g = torch.Generator().manual_seed(Cin + Cout + level)
    x = torch.randn(V_in, Cin, generator=g).to(gpu)
    W = _weights(K, Cin, Cout, Cin * Cout + K, gpu)
    wp = svnn.pack_weights_bf16(W)
    raw = svnn.conv_forward(x, W, plan, V_out, weight_bf16=wp)
    assert _lib.conv_last_instance()[0].startswith("conv_bf16_kernel")
    ratio = _check_raw(x, W, plan, V_out, raw)
    print(f"{layer[0]}: worst |err| / bound = {ratio:.3g}")
    # epilogues: exactly sv_conv_fwd's arithmetic on the raw accumulator (sv_affine_act is the same code path)
    scale = (torch.rand(Cout, generator=g) + 0.5).to(gpu)
    shift = torch.randn(Cout, generator=g).to(gpu)
    res = torch.randn(V_out, Cout, generator=g).to(gpu)
    for sc, sh, r, act in ((scale, shift, res, _lib.SV_ACT_RELU), (None, shift, None, _lib.SV_ACT_LEAKY_RELU),
                           (scale, shift, None, _lib.SV_ACT_NONE), (None, None, res, _lib.SV_ACT_RELU)):
        got = svnn.conv_forward(x, W, plan, V_out, sc, sh, r, act, 0.02, weight_bf16=wp)
        want = svnn.affine_act(raw, sc, sh, r, act, 0.02)
        assert torch.equal(got, want), (sc is None, sh is None, r is None, act)
    # output into the left columns of a concatenated buffer (out_ld != Cout), residual strided too
    buf = torch.full((V_out, Cout + 32), 7.0, device=gpu)
    svnn.conv_forward(x, W, plan, V_out, scale, shift, res, _lib.SV_ACT_RELU, out=buf[:, :Cout], weight_bf16=wp)
    assert torch.equal(buf[:, :Cout], svnn.affine_act(raw, scale, shift, res, _lib.SV_ACT_RELU))
    assert (buf[:, Cout:] == 7.0).all()


def test_bf16_passes_dispatch_and_frames_bit_exact(gpu):
    from mrcc_amd import _lib
    from mrcc_amd import nn as svnn

    Cin = Cout = 384
    W = _weights(27, Cin, Cout, 11, gpu)
    wp = svnn.pack_weights_bf16(W)
    st = _cloud(gpu, n=60_000)
    cm = st.coordinate_manager
    V = cm.stride_map(1).V
    g = torch.Generator().manual_seed(3)
    x = torch.randn(V, Cin, generator=g).to(gpu)
    scale = (torch.rand(Cout, generator=g) + 0.5).to(gpu)
    shift = torch.randn(Cout, generator=g).to(gpu)
    one = svnn.conv_forward(x, W, cm.plan_k3(1), V, scale, shift, None, _lib.SV_ACT_RELU, weight_bf16=wp)
    for cuts in (9, (9, 18), 14):
        split = svnn.conv_forward(x, W, cm.plan_k3_split(1, cuts), V, scale, shift, None, _lib.SV_ACT_RELU, weight_bf16=wp)
        assert torch.equal(split, one), cuts
    with _lib.conv_dispatch(1.0):
        again = svnn.conv_forward(x, W, cm.plan_k3(1), V, scale, shift, None, _lib.SV_ACT_RELU, weight_bf16=wp)
    assert torch.equal(again, one)
    # four frames in one tensor: each frame's rows equal the frame alone (rows are sorted by batch first)
    seeds = (4, 5, 6, 7)
    st4 = _cloud(gpu, n=30_000, seeds=seeds)
    cm4 = st4.coordinate_manager
    V4 = cm4.stride_map(1).V
    x4 = torch.randn(V4, Cin, generator=g).to(gpu)
    out4 = svnn.conv_forward(x4, W, cm4.plan_k3_split(1, (9, 18)), V4, weight_bf16=wp)
    bs = cm4.batch_offsets(1, 4).cpu().tolist()
    for b, sd in enumerate(seeds):
        stb = _cloud(gpu, n=30_000, seeds=(sd,))
        cmb = stb.coordinate_manager
        Vb = cmb.stride_map(1).V
        assert Vb == bs[b + 1] - bs[b]
        xb = x4[bs[b]:bs[b + 1]].contiguous()
        alone = svnn.conv_forward(xb, W, cmb.plan_k3(1), Vb, weight_bf16=wp)
        assert torch.equal(alone, out4[bs[b]:bs[b + 1]]), b


def _seeded_model(gpu):
    from mrcc_amd.model.robotnet_segmentation import RobotNetSegmentation

    torch.manual_seed(1)
    model = RobotNetSegmentation(in_channels=3, num_classes=3)
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.75)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.75)
    return model.to(gpu).eval()


def _field(gpu, n, seed, L=2.4, scale=50):
    import mrcc_amd
    from mrcc_amd import MinkowskiEngine as ME

    pts, rgb, _ = mrcc_amd.synth.gen_room(n, L, seed)
    coords4 = np.concatenate([np.zeros((len(pts), 1), np.float32), pts * np.float32(scale)], axis=1)
    return ME.TensorField(torch.from_numpy(rgb), torch.from_numpy(coords4),
                          quantization_mode=ME.SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE, device=gpu)


def test_instance_report_names_bf16_for_exactly_the_eligible_layers(gpu):
    from mrcc_amd import nn as svnn
    from mrcc_amd import profiling

    model = _seeded_model(gpu)
    field = _field(gpu, 40_000, 3)

    def launches():
        profiling.INSTANCE_LOG = []
        try:
            with torch.no_grad():
                model(field.sparse())
            torch.cuda.synchronize()
            return profiling.INSTANCE_LOG
        finally:
            profiling.INSTANCE_LOG = None

    log = launches()
    assert log and not any("bf16" in e[0] for e in log)
    svnn.set_compute_precision(model, "bf16")
    log = launches()
    n_bf16 = 0
    for name, _flags, K, Cin, Cout, _rows in log:
        eligible = Cin % 32 == 0 and Cin >= 64 and Cout % 16 == 0 and Cout >= 64
        assert ("bf16" in name) == eligible, (name, K, Cin, Cout)
        n_bf16 += eligible
    assert n_bf16 >= 41
    svnn.set_compute_precision(model, "fp32")
    assert not any("bf16" in e[0] for e in launches())


def test_network_bf16_against_fp32_cfg2(gpu):
    from mrcc_amd import nn as svnn

    model = _seeded_model(gpu)
    field = _field(gpu, 200_000, 0)
    with torch.no_grad():
        ref = model(field.sparse())
        ref_logits = ref.F.clone()
        ref_label, _ = ref.slice_argmax(field)
        svnn.set_compute_precision(model, "bf16")
        out = model(field.sparse())
        label, _ = out.slice_argmax(field)
    rel = (torch.linalg.norm(out.F.double() - ref_logits.double()) / torch.linalg.norm(ref_logits.double())).item()
    agree = (label == ref_label).double().mean().item()
    print(f"Cfg-2 bf16 vs fp32: relative Frobenius error {rel:.4g}, label agreement {agree:.5f}")
    assert rel <= 0.05 and agree >= 0.97


def test_engine_bf16_switch(gpu):
    import mrcc_amd
    from mrcc_amd.app.dto import PointCloudDTO
    from mrcc_amd.app.inference_engine import InferenceEngine
    from mrcc_amd.utils import preprocess
    from mrcc_amd.utils.config import Config

    Config.reset()
    Config().update({"INFERENCE": {"SEGMENTATION": {"scale": 50}, "ROTATION": {"scale": 100},
                                   "KEY_POINTS": {"scale": 100, "conf_threshold": 0.0},
                                   "ee_point_counts_threshold": 64, "SANITY": {"min_num_of_ee_points": 64}}})
    try:
        scenes = [mrcc_amd.synth.gen_scene(s, n_bg=5000 + 900 * s, n_arm=700, n_ee=1200 + 50 * s) for s in range(5)]
        frames = [(sc["points"], preprocess.normalize_colors(sc["rgb"])) for sc in scenes]
        fp32 = InferenceEngine(allow_random_init=True, seed=7)
        want32 = [fp32.predict_segmentation(p, c) for p, c in frames]
        del fp32
        eng = InferenceEngine(allow_random_init=True, seed=7, seg_precision="bf16")
        assert eng.seg_precision == "bf16"
        assert eng._segmentation_model.final.compute_precision == "bf16"
        assert eng._rotation_model.final.compute_precision == "fp32"
        want = [eng.predict_segmentation(p, c) for p, c in frames]
        got = list(eng.predict_segmentation_stream(iter(frames), compute_streams=3, group=4))
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w)
        agree = np.mean(np.concatenate([a == b for a, b in zip(want, want32)]))
        assert agree >= 0.9, agree
        for sc in scenes[:2]:
            r = eng.predict(PointCloudDTO(points=sc["points"], rgb=sc["rgb"], ee2base_pose=sc["ee2base_pose"]))
            assert r.segmentation is not None and len(r.segmentation) == len(sc["points"])
        del eng
        # the config key selects it too; a default engine afterwards is fp32 again
        Config().update({"INFERENCE": {"SEGMENTATION": {"precision": "bf16"}}})
        assert InferenceEngine(allow_random_init=True, seed=7, calibration_only=False).seg_precision == "bf16"
        Config().update({"INFERENCE": {"SEGMENTATION": {"precision": None}}})
        eng = InferenceEngine(allow_random_init=True, seed=7)
        assert eng.seg_precision == "fp32"
        again = [eng.predict_segmentation(p, c) for p, c in frames]
        for a, w in zip(again, want32):
            assert np.array_equal(a, w)
        with pytest.raises(ValueError):
            InferenceEngine(allow_random_init=True, seg_precision="fp16")
    finally:
        Config.reset()
