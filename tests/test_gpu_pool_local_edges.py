"""sv_pool_local / sv_pool_local_backward and the pooling modules at their edges: every pooling shape layer_maps(pooling=True)
promises beyond the stem's k2 s2, widths past one pass of the float4 kernel's channel loop, rows without neighbours that the
maps produce on their own, row tails of the four-rows-per-workgroup launch, and guard rows / columns around every output.

References (tests/strided_helpers.py; tests/test_resnet_ops_edges_cpu.py checks them against each other without a GPU):
the forward is float32 in the defined order (pool_ref, exact); the backward is bit-equal to the float32 ascending-k
restatement over the transposed table and within K * 2^-24 * sum_k |term| of the float64 one (K float32 additions of correctly
rounded terms; the average's one division per term is covered by K + 1); the modules are compared with torch's own pooling on a
dense float64 grid, which shares no code with kernel maps."""
import numpy as np
import pytest

import strided_helpers as H

pytestmark = pytest.mark.gpu

MAX, AVG, SUM = 0, 1, 2
SHAPES = ("k3s3", "k1s2", "k3s1", "k3s1d2", "k3s2d2", "k1s1")  # H.POOL_SHAPES; "k3s2" serves the row tails


@pytest.fixture(scope="module")
def maps(gpu):
    """the raw forward and transposed tables the pooling modules would use, on H.pool_edge_cloud: shape -> (nbr, nbr_t) on
    the device, from layer_maps(pooling=True) through CoordinateManager.layer_plans as nn._LocalPoolBase takes them"""
    import torch

    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd.sparse import layer_maps

    pts = H.pool_edge_cloud()
    x = ME.SparseTensor(torch.ones(len(pts), 1), coordinates=torch.from_numpy(pts.astype(np.int32)), device=gpu)
    cm = x.coordinate_manager
    out = {"cm": cm}
    for shape, (ks, st, dil) in H.POOL_SHAPES.items():
        plan, out_stride, t_plan, _ = cm.layer_plans(layer_maps(ks, st, dil, pooling=True), 1)
        assert out_stride == st
        out[shape] = (plan.raw[0][:, :plan.V_out], t_plan().raw[0][:, :cm.stride_map(1).V])
    return out


@pytest.mark.parametrize("shape", SHAPES + ("k3s2",))
def test_tables_are_the_restatements(gpu, maps, shape):
    fwd, tr, c_in, c_out = H.pool_tables_ref(shape)
    cm = maps["cm"]
    assert np.array_equal(cm.stride_map(1).coords.cpu().numpy(), c_in)
    assert np.array_equal(cm.stride_map(H.POOL_SHAPES[shape][1]).coords.cpu().numpy(), c_out)
    assert np.array_equal(maps[shape][0].cpu().numpy(), fwd) and np.array_equal(maps[shape][1].cpu().numpy(), tr)
    if shape in ("k3s3", "k1s2"):
        assert (fwd < 0).all(0).any()  # output rows with no neighbour, produced by the map itself
    if shape == "k3s1":
        assert (fwd >= 0).all(0).any()  # a row with all 27


def _variants(rng, V, C):
    """(mode, features): max and sum on the tie / NaN / inf pattern, all three on plain normals"""
    for mode, ties in ((MAX, True), (MAX, False), (AVG, False), (SUM, False), (SUM, True)):
        yield mode, ties, H.pool_features(rng, V, C, ties)


@pytest.mark.parametrize("C", [1, 4, 65, 260, 512, "260 of 264"])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_exact(gpu, maps, shape, C):
    import torch

    fwd = H.pool_tables_ref(shape)[0]
    V_in = maps[shape][1].shape[1]
    view = isinstance(C, str)  # columns 2 .. 262 of a wider buffer: 8 bytes off the alignment, the scalar kernel
    C = 260 if view else C
    rng = np.random.default_rng(C + 1000 * view)
    empty = (fwd < 0).all(0)
    for mode, ties, x in _variants(rng, V_in, C):
        if view:
            wide = torch.full((V_in, 264), 99.0, dtype=torch.float32, device=gpu)
            xt = wide[:, 2:262]
            xt.copy_(torch.from_numpy(x))
        else:
            xt = torch.from_numpy(x).to(gpu)
        got, arg, vec = H.gpu_pool_guarded(xt, maps[shape][0], mode, pad_cols=3 if C % 4 else 4)
        assert vec == (C % 4 == 0 and not view), (C, view)  # 260 and 512 take the float4 kernel, the view does not
        with np.errstate(invalid="ignore"):
            want, want_arg = H.pool_ref(x, fwd, mode)
        assert np.array_equal(got, want, equal_nan=True), (shape, C, mode, ties)
        assert (got[empty] == 0).all()
        if mode == MAX:
            assert np.array_equal(arg, want_arg), (shape, C, ties)
            assert (arg[empty] == -1).all() and (arg[~empty] >= 0).all()
            if ties and shape == "k3s1":
                assert np.isnan(want).any()


@pytest.mark.parametrize("C", [8, 5])
@pytest.mark.parametrize("V_out", [0, 1, 2, 3, 5, 6, 7])
def test_row_tails_and_guards(gpu, maps, V_out, C):
    """the first V_out rows of the k3 s2 table (ld unchanged) into out [V_out + 4, C + 4] and arg [V_out + 4, C]: the written
    rows are the reference's, every guard element keeps its sentinel (asserted in the helper); V_out = 0 writes nothing"""
    import torch

    fwd = H.pool_tables_ref("k3s2")[0]
    rng = np.random.default_rng(10 * V_out + C)
    for mode, ties, x in _variants(rng, len(H.pool_tables_ref("k3s2")[2]), C):
        got, arg, vec = H.gpu_pool_guarded(torch.from_numpy(x).to(gpu), maps["k3s2"][0], mode, V_out=V_out, pad_cols=4)
        assert vec == (C == 8)
        with np.errstate(invalid="ignore"):
            want, want_arg = H.pool_ref(x, fwd[:, :V_out], mode)
        assert got.shape == (V_out, C) and np.array_equal(got, want, equal_nan=True)
        if mode == MAX:
            assert np.array_equal(arg, want_arg)


@pytest.mark.parametrize("C", [1, 65, 260])
@pytest.mark.parametrize("shape", SHAPES)
def test_backward(gpu, maps, shape, C):
    import torch

    fwd, tr, c_in, c_out = H.pool_tables_ref(shape)
    V_in, V_out = len(c_in), len(c_out)
    rng = np.random.default_rng(200 + C)
    count = (fwd >= 0).sum(0)
    unread = (tr < 0).all(0)
    assert unread.any() == (shape in ("k3s3", "k1s2", "k3s2d2"))
    mask = torch.from_numpy(H.mask_of(fwd)).to(gpu)
    worst = 0.0
    for mode in (MAX, AVG, SUM):
        x = np.nan_to_num(H.pool_features(rng, V_in, C, ties=(mode == MAX)), nan=1.0, posinf=2.0, neginf=-2.0)
        arg = H.pool_ref(x, fwd, mode)[1]
        dy = rng.standard_normal((V_out, C)).astype(np.float32)
        wide = torch.full((V_out, C + 2), 55.0, dtype=torch.float32, device=gpu)  # dy_ld = C + 2
        wide[:, 1:C + 1] = torch.from_numpy(dy)
        argt = torch.from_numpy(arg).to(gpu)
        got = H.gpu_pool_backward_guarded(wide[:, 1:C + 1], maps[shape][1], mode, argt, mask)
        again = H.gpu_pool_backward_guarded(wide[:, 1:C + 1], maps[shape][1], mode, argt, mask)
        assert np.array_equal(got, again)  # a gather, no float atomics
        assert (wide[:, 0] == 55.0).all() and (wide[:, C + 1] == 55.0).all()
        assert np.array_equal(got, H.pool_backward32_ref(dy, tr, mode, arg, count)), (shape, C, mode)
        assert (got[unread] == 0).all()
        want = H.pool_backward_ref(dy, fwd, mode, arg, V_in)
        bound = H.pool_backward_bound(dy, tr, mode, arg, count)
        err = np.abs(got - want)
        assert (err <= bound).all(), (shape, C, mode)
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
    print(f"pool backward {shape} C={C}: max err / bound = {worst:.3f}")


@pytest.fixture(scope="module")
def dense_cloud(gpu):
    import torch

    from mrcc_amd import MinkowskiEngine as ME

    pts = H.dense_pool_cloud()
    x = ME.SparseTensor(torch.ones(len(pts), 1), coordinates=torch.from_numpy(pts.astype(np.int32)), device=gpu)
    cm = x.coordinate_manager
    c_in = cm.stride_map(1).coords.cpu().numpy()
    assert np.array_equal(c_in, H.canonical(pts)[0])
    return cm, c_in


@pytest.mark.parametrize("ks,st", H.DENSE_POOLS)
def test_modules_against_dense_grid(gpu, dense_cloud, ks, st):
    """MinkowskiMaxPooling / AvgPooling / SumPooling forward and .backward() against torch's max_pool3d / avg_pool3d on a dense
    float64 grid (H.dense_pool_ref): max exact; sum and avg within (K [+ 1]) 2^-24 * pooled |x| [/ count]; the input gradient
    within K_t 2^-24 * sum |term|, K_t = the transposed table's offsets (the same K; + 1 for avg), |term| from the dense
    gradient of |dy|.  Features are distinct per channel, so no window has a tie."""
    import torch

    from mrcc_amd import MinkowskiEngine as ME

    cm, c_in = dense_cloud
    C, K = 3, ks ** 3
    rng = np.random.default_rng(ks * 10 + st)
    x = rng.standard_normal((len(c_in), C)).astype(np.float32)
    assert all(len(np.unique(x[:, c])) == len(x) for c in range(C))
    c_out = H.stride_map_ref(c_in, st)[0] if st > 1 else c_in
    dy = rng.standard_normal((len(c_out), C)).astype(np.float32)
    for mode, cls in ((MAX, ME.MinkowskiMaxPooling), (AVG, ME.MinkowskiAvgPooling), (SUM, ME.MinkowskiSumPooling)):
        f = torch.from_numpy(x).to(gpu).requires_grad_(True)
        y = cls(kernel_size=ks, stride=st, dimension=3)(ME.SparseTensor(f, coordinate_manager=cm, tensor_stride=1))
        assert y.tensor_stride == st and np.array_equal(y.C.cpu().numpy(), c_out)
        d = H.dense_pool_ref(c_in, x, c_out, ks, st, mode, H.DENSE_ORIGIN, H.DENSE_SIZE, dy)
        got = y.F.detach().cpu().numpy()
        if mode == MAX:
            assert np.array_equal(got.astype(np.float64), d["out"])
        else:
            assert (np.abs(got - d["out"]) <= d["bound"]).all(), (ks, st, mode)
        assert (got[d["count"] == 0] == 0).all() and ((d["count"] == 0).any() == ((ks, st) == (3, 3)))
        y.F.backward(torch.from_numpy(dy).to(gpu))
        dx = f.grad.cpu().numpy()
        bound = (K + (mode == AVG)) * 2.0 ** -24 * d["dx_terms"]
        err = np.abs(dx - d["dx"])
        assert (err <= bound).all(), (ks, st, mode)
        r = float((err[bound > 0] / bound[bound > 0]).max())
        print(f"pooling module k{ks} s{st} mode {mode}: backward max err / bound = {r:.3f}")
