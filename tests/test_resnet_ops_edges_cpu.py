"""CPU twin of the edge tests of local pooling, instance norm and the general stride map (tests/test_gpu_pool_local_edges.py,
tests/test_gpu_instance_norm_edges.py, tests/test_gpu_strided_maps_edges.py): the references of tests/strided_helpers.py are
checked against each other, and the test inputs are shown to be what the GPU tests rely on, before any kernel is involved.  No
GPU, no library."""
import numpy as np
import pytest

import strided_helpers as H

EPS = 1e-8


# ---- instance norm: the cancellation inputs discriminate ---------------------------------------------------------------
def _one_pass(x, starts, w, b, dtype):
    """instance norm with statistics in `dtype` and the variance as E[x^2] - mean^2 (float64) or two-pass (float32)"""
    y = np.zeros(x.shape, np.float64)
    for f in range(len(starts) - 1):
        seg = x[starts[f]:starts[f + 1]].astype(dtype)
        n = dtype(len(seg))
        mean = seg.sum(0, dtype=dtype) / n
        if dtype is np.float64:
            var = np.maximum((seg * seg).sum(0) / n - mean * mean, 0.0)
        else:
            var = ((seg - mean) ** 2).sum(0, dtype=dtype) / n
        y[starts[f]:starts[f + 1]] = (seg - mean).astype(np.float64) / np.sqrt(var.astype(np.float64) + EPS) * w + b
    return y


def test_cancellation_inputs_discriminate():
    x, starts, k, base = H.cancellation_case()
    C = x.shape[1]
    assert set(np.unique(base)) == set(H.CANCEL_BASES) and np.diff(starts).tolist() == list(H.CANCEL_SIZES)
    w, b = np.linspace(0.5, 2.0, C).astype(np.float32), np.linspace(-1.0, 1.0, C).astype(np.float32)
    exact = H.cancellation_exact(k, starts, base, w, b, EPS)
    bound = H.norm_forward_bound(exact)
    ref = H.instance_norm_ref(x, starts, w, b, EPS, 0)
    assert (np.abs(ref - exact) <= bound).all()
    # the mean is exact: the same bits from the small integers as from the values
    mean, _ = H.instance_norm_stats_ref(x, starts, EPS)
    for f in range(len(starts) - 1):
        s, e = starts[f], starts[f + 1]
        u = np.array([H.ulp32(v) for v in base[f]])
        assert np.array_equal(mean[f], (base[f] * (e - s) + k[s:e].sum(0) * u) / (e - s))
    miss64 = (np.abs(_one_pass(x, starts, w, b, np.float64) - exact) / bound).max()
    miss32 = (np.abs(_one_pass(x, starts, w, b, np.float32) - exact) / bound).max()
    print(f"cancellation case: one-pass float64 misses the bound {miss64:.3g} times, float32 statistics {miss32:.3g} times")
    assert miss64 > 100 and miss32 > 1e4


def test_backward_reference_is_the_gradient_of_the_forward_reference():
    """instance_norm_backward_ref (the header's formula) against float64 torch autograd of the definition"""
    import torch

    rng = np.random.default_rng(0)
    starts = np.array([0, 5, 5, 40], np.int32)
    x = (rng.standard_normal((40, 3)) * 2.0 + 3.0).astype(np.float32)
    w, b = np.array([1.5, -0.7, 0.9], np.float32), np.array([0.1, -0.2, 0.3], np.float32)
    dy = rng.standard_normal(x.shape).astype(np.float32)
    mean, inv_std = H.instance_norm_stats_ref(x, starts, EPS)
    for act in (0, 1, 3):
        dx, dw, db, noise, dw_n, db_n = H.instance_norm_backward_ref(x, starts, w, b, mean, inv_std, act, dy)
        xt, wt, bt = (torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in (x, w, b))
        parts = []
        for s, e in ((0, 5), (5, 40)):
            seg = xt[s:e]
            m = seg.mean(0)
            parts.append((seg - m) / torch.sqrt(((seg - m) ** 2).mean(0) + EPS) * wt + bt)
        y = torch.cat(parts)
        y = torch.relu(y) if act == 1 else torch.nn.functional.gelu(y) if act == 3 else y
        (y * torch.from_numpy(dy.astype(np.float64))).sum().backward()
        assert np.allclose(dx, xt.grad.numpy(), rtol=0, atol=1e-12 * noise.max())
        assert np.allclose(dw, wt.grad.numpy(), rtol=0, atol=1e-12 * dw_n.max())
        assert np.allclose(db, bt.grad.numpy(), rtol=0, atol=1e-12 * db_n.max())


# ---- pooling: the tables have the rows the GPU tests count on; the dense grid agrees with the table reference ----------
def test_pool_tables_have_empty_and_full_rows():
    for shape in ("k3s3", "k1s2"):
        fwd, tr, c_in, c_out = H.pool_tables_ref(shape)
        empty = (fwd < 0).all(0)
        assert empty.any() and not empty.all(), shape
        assert (tr < 0).all(0).any(), shape  # input rows that no output reads
    fwd = H.pool_tables_ref("k3s1")[0]
    assert (fwd >= 0).all(0).any()  # some voxel has all 27 neighbours
    c_in = H.pool_tables_ref("k3s1")[2]
    assert 550 <= len(c_in) <= 650 and set(c_in[:, 0].tolist()) == {0, 1} and (c_in[:, 1:] < 0).any()
    for shape in H.POOL_SHAPES:  # transposed table = transpose of the forward table
        fwd, tr, _, _ = H.pool_tables_ref(shape)
        a = {(k, int(o), int(i)) for k in range(fwd.shape[0]) for o, i in enumerate(fwd[k]) if i >= 0}
        b = {(k, int(o), int(i)) for k in range(tr.shape[0]) for i, o in enumerate(tr[k]) if o >= 0}
        assert a == b, shape


@pytest.mark.parametrize("ks,st", H.DENSE_POOLS)
def test_dense_pool_reference_agrees_with_table_reference(ks, st):
    c_in = H.canonical(H.dense_pool_cloud())[0]
    c_out = H.stride_map_ref(c_in, st)[0] if st > 1 else c_in
    nbr = H.probe_ref(c_out, c_in, 3, 1) if ks == 3 else H.k2_table_ref(c_out, c_in)
    rng = np.random.default_rng(ks * 10 + st)
    x = rng.standard_normal((len(c_in), 3)).astype(np.float32)
    assert all(len(np.unique(x[:, c])) == len(x) for c in range(3))  # distinct: no window has a tie
    dy = rng.standard_normal((len(c_out), 3)).astype(np.float32)
    count = (nbr >= 0).sum(0)
    assert ((count == 0).any()) == ((ks, st) == (3, 3))
    for mode in (0, 1, 2):
        d = H.dense_pool_ref(c_in, x, c_out, ks, st, mode, H.DENSE_ORIGIN, H.DENSE_SIZE, dy)
        want, arg = H.pool_ref(x, nbr, mode)
        assert np.array_equal(d["count"], count)
        if mode == 0:
            assert np.array_equal(d["out"], want.astype(np.float64))
        else:
            assert (np.abs(d["out"] - want) <= d["bound"]).all()
        dx = H.pool_backward_ref(dy, nbr, mode, arg, len(c_in))
        assert np.allclose(d["dx"], dx, rtol=0, atol=1e-13 * max(np.abs(dx).max(), 1.0))
        # the magnitudes the backward bound is made of: the dense |dy| gradient is the table's sum of |term|
        terms = H.pool_backward_ref(np.abs(dy), nbr, mode, arg, len(c_in))
        assert np.allclose(d["dx_terms"], terms, rtol=0, atol=1e-13 * terms.max())


def test_pool_backward_float32_restatement_is_within_its_bound():
    fwd, tr, c_in, c_out = H.pool_tables_ref("k3s2")
    rng = np.random.default_rng(1)
    x = rng.standard_normal((len(c_in), 5)).astype(np.float32)
    dy = rng.standard_normal((len(c_out), 5)).astype(np.float32)
    count = (fwd >= 0).sum(0)
    for mode in (0, 1, 2):
        arg = H.pool_ref(x, fwd, mode)[1]
        got = H.pool_backward32_ref(dy, tr, mode, arg, count)
        want = H.pool_backward_ref(dy, fwd, mode, arg, len(c_in))
        assert (np.abs(got - want) <= H.pool_backward_bound(dy, tr, mode, arg, count)).all()


# ---- the general stride map: the whole-array restatement is the dict one; the extreme inputs are what they claim -------
def test_array_restatements_equal_the_dict_ones():
    rng = np.random.default_rng(2)
    rows = np.concatenate([rng.integers(0, 3, size=(400, 1)) * 511, rng.integers(-50, 50, size=(400, 3))], 1)
    rows = np.concatenate([rows, [[1023, H.HI, H.LO, 0], [0, H.LO, H.LO, H.LO], [5, H.LO + 1, 7, -1]]])
    c, k = H.canonical(rows)
    c2, k2 = H.canonical_np(rows)
    assert np.array_equal(c, c2) and np.array_equal(k, k2)
    for s in (3, 5, 192):
        a, b = H.stride_map_ref(c, s), H.stride_map_ref_np(c, s)
        assert a[3] == b[3] and (s == 192 or a[3] > 0)
        assert all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3])), s


@pytest.mark.parametrize("batch", [0, 1023])
def test_collapse_and_spread_inputs_are_what_they_claim(batch):
    c = H.canonical_np(H.collapse_voxels(batch))[0]
    out, _, parent, bad = H.stride_map_ref_np(c, 192)
    assert len(c) == 9000 and bad == 0 and out.tolist() == [[batch, -192, -192, -192]] and (parent == 0).all()
    c = H.canonical_np(H.spread_voxels(batch))[0]
    out, _, parent, bad = H.stride_map_ref_np(c, 3)
    assert len(c) == 9000 and bad == 0 and len(out) == 9000 and np.array_equal(np.sort(parent), np.arange(9000))
    assert (c[:, 1:] < 0).any() and (c[:, 1:] > 0).any() and (c[:, 0] == batch).all()
