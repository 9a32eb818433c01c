"""sv_pool_local / sv_pool_local_backward and the MinkowskiMax/Avg/SumPooling modules against numpy restatements
(tests/strided_helpers.py): the forward in float32 in the defined order (exact), the backward against float64."""
import numpy as np
import pytest

import strided_helpers as H

pytestmark = pytest.mark.gpu

MAX, AVG, SUM = 0, 1, 2
TABLES = ("k2s2", "k3s2")
REL_TOL = 1e-4  # the project's: tests/test_gpu_training.py


@pytest.fixture(scope="module")
def maps(gpu):
    """one two-frame cloud, its k2 s2 and k3 s2 kernel maps (forward and transposed raw tables), shared by every test"""
    import torch

    from mrcc_amd import MinkowskiEngine as ME

    rng = np.random.default_rng(5)
    pts = np.concatenate([np.concatenate([np.full((260, 1), b), H.blob_cloud(rng, 260, [(-5, 2, 0), (6, -3, 4)], 3.0, (-20,) * 3,
                                                                              (20,) * 3)], 1) for b in (0, 1)])
    x = ME.SparseTensor(torch.ones(len(pts), 1), coordinates=torch.from_numpy(pts.astype(np.int32)), device=gpu)
    cm = x.coordinate_manager
    out = {"cm": cm, "V_in": cm.stride_map(1).V}
    for name, fwd, tr in (("k2s2", cm.plan_down(1), cm.plan_up(2)), ("k3s2", cm.plan_strided(1, 3, 2), cm.plan_strided_t(1, 3, 2))):
        out[name] = (fwd.raw[0], tr.raw[0], fwd.raw[2], fwd.raw[0].cpu().numpy(), tr.raw[0].cpu().numpy())
    assert out["V_in"] > 256 and out["k2s2"][3].shape[1] > 64
    return out


_features = H.pool_features


@pytest.mark.parametrize("C", [1, 3, 64, 65])
@pytest.mark.parametrize("table", TABLES)
def test_pool_forward_exact(gpu, maps, table, C):
    import torch

    nbr, _, _, nbr_np, _ = maps[table]
    rng = np.random.default_rng(C)
    for mode, ties in ((MAX, True), (MAX, False), (AVG, False), (SUM, False), (SUM, True)):
        x = _features(rng, maps["V_in"], C, ties)
        got, arg = H.gpu_pool(torch.from_numpy(x).to(gpu), nbr, mode)
        with np.errstate(invalid="ignore"):
            want, want_arg = H.pool_ref(x, nbr_np, mode)
        assert np.array_equal(got.cpu().numpy(), want, equal_nan=True), (table, C, mode, ties)
        if mode == MAX:
            assert np.array_equal(arg.cpu().numpy(), want_arg), (table, C, ties)
            if ties:
                assert np.isnan(want).any() and (want_arg >= 0).all()


def test_pool_forward_row_without_neighbours_and_strided_rows(gpu, maps):
    """the guarded empty case (no kernel map produces it): 0, arg -1; and input rows that are a column slice (in_ld > C)"""
    import torch

    nbr, _, _, nbr_np, _ = maps["k2s2"]
    nbr2 = nbr.clone()
    nbr2[:, 5] = -1
    nbr_np = nbr_np.copy()
    nbr_np[:, 5] = -1
    rng = np.random.default_rng(0)
    wide = torch.from_numpy(rng.standard_normal((maps["V_in"], 72)).astype(np.float32)).to(gpu)  # (0, 64): the float4 path
    for c0, C in ((0, 64), (3, 64), (2, 5)):
        x = wide[:, c0:c0 + C]
        for mode in (MAX, AVG, SUM):
            got, arg = H.gpu_pool(x, nbr2, mode)
            want, want_arg = H.pool_ref(x.cpu().numpy(), nbr_np, mode)
            assert np.array_equal(got.cpu().numpy(), want) and (got[5] == 0).all()
            if mode == MAX:
                assert np.array_equal(arg.cpu().numpy(), want_arg) and (arg[5] == -1).all()


@pytest.mark.parametrize("C", [1, 3, 64, 65])
@pytest.mark.parametrize("table", TABLES)
def test_pool_backward(gpu, maps, table, C):
    import torch

    nbr, nbr_t, mask, nbr_np, nbr_t_np = maps[table]
    rng = np.random.default_rng(100 + C)
    V_out = nbr_np.shape[1]
    for mode in (MAX, AVG, SUM):
        x = _features(rng, maps["V_in"], C, ties=(mode == MAX))
        x = np.nan_to_num(x, nan=1.0, posinf=2.0, neginf=-2.0)
        _, arg = H.gpu_pool(torch.from_numpy(x).to(gpu), nbr, mode)
        dy = rng.standard_normal((V_out, C)).astype(np.float32)
        dyt = torch.from_numpy(dy).to(gpu)
        got = H.gpu_pool_backward(dyt, nbr_t, mode, arg, mask)
        again = H.gpu_pool_backward(dyt, nbr_t, mode, arg, mask)
        assert torch.equal(got, again)  # identical bits: a gather, no float atomics
        want = H.pool_backward_ref(dy, nbr_np, mode, arg.cpu().numpy() if arg is not None else None, maps["V_in"])
        got = got.cpu().numpy()
        # float64 reference from the FORWARD table.  Where one fp32 value is routed (an input with a single window: every
        # input of k2 s2) sum and max are exact; an input of k3 s2 lies in up to 8 windows and the fp32 sum of their dy is
        # rounded, so there, and for avg, the bound is the project's 1e-4 * max|want|
        single = (nbr_t_np >= 0).sum(0) == 1
        assert single.any() and (table != "k2s2" or single.all())
        assert np.abs(got - want).max() <= REL_TOL * np.abs(want).max()
        if mode != AVG:
            assert np.array_equal(got[single].astype(np.float64), want[single])
        # and exactly the defined order in float32: ascending k over the transposed table
        acc = H.pool_backward32_ref(dy, nbr_t_np, mode, arg.cpu().numpy() if arg is not None else None, (nbr_np >= 0).sum(0))
        assert np.array_equal(got, acc)


@pytest.mark.parametrize("table,ks,st", [("k2s2", 2, 2), ("k3s2", 3, 2)])
def test_pooling_modules_autograd(gpu, maps, table, ks, st):
    """ME.MinkowskiMaxPooling / AvgPooling / SumPooling: forward and .backward() are the entry points' results"""
    import torch

    from mrcc_amd import MinkowskiEngine as ME

    nbr, nbr_t, mask, _, _ = maps[table]
    rng = np.random.default_rng(9)
    C = 8
    feats = torch.from_numpy(rng.standard_normal((maps["V_in"], C)).astype(np.float32)).to(gpu)
    dy = torch.from_numpy(rng.standard_normal((nbr.shape[1], C)).astype(np.float32)).to(gpu)
    for mode, cls in ((MAX, ME.MinkowskiMaxPooling), (AVG, ME.MinkowskiAvgPooling), (SUM, ME.MinkowskiSumPooling)):
        f = feats.clone().requires_grad_(True)
        x = ME.SparseTensor(f, coordinate_manager=maps["cm"], tensor_stride=1)
        y = cls(kernel_size=ks, stride=st, dimension=3)(x)
        assert y.tensor_stride == st
        want, arg = H.gpu_pool(feats, nbr, mode)
        assert torch.equal(y.F, want)
        y.F.backward(dy)
        assert torch.equal(f.grad, H.gpu_pool_backward(dy, nbr_t, mode, arg, mask))
    with pytest.raises(NotImplementedError):
        ME.MinkowskiMaxPooling(kernel_size=2, stride=1, dimension=3)(x)
