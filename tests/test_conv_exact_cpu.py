"""The exact integer references of tests/conv_exact_helpers.py against independent formulations, on the CPU: the float64
gather / index_add / autograd reference tests/test_gpu_conv_grad.py uses, and a plain int64 einsum over explicit pairs -
on hand-made neighbour tables with absent neighbours (-1), for K = 1, 8 and 27."""
import pytest
import torch

import conv_exact_helpers as H


def _table(K, V_in, V_out, seed, ld_extra=3):
    """nbr int32 [K, V_out + ld_extra]: about a third of the entries absent, one output row with no neighbour at all,
    one offset with no pair, padding columns beyond V_out that must not be read"""
    g = torch.Generator().manual_seed(seed)
    nbr = torch.randint(0, V_in, (K, V_out + ld_extra), generator=g, dtype=torch.int32)
    nbr[torch.rand(nbr.shape, generator=g) < 0.35] = -1
    nbr[:, V_out // 2] = -1
    if K > 1:
        nbr[K // 2] = -1
    nbr[:, V_out:] = V_in + 1000  # beyond the table's rows: reading them would raise
    return nbr


def _float64_ref(fin, W, nbr, V_out):
    """tests/test_gpu_conv_grad.py _ref: out[o] = sum_k fin[nbr[k][o]] @ W[k], float64, differentiable"""
    out = torch.zeros((V_out, W.shape[2]), dtype=torch.float64)
    for k in range(W.shape[0]):
        idx = nbr[k, :V_out].long()
        ok = idx >= 0
        out = out.index_add(0, torch.nonzero(ok).flatten(), fin[idx[ok]] @ W[k])
    return out


@pytest.mark.parametrize("K", [1, 8, 27])
def test_int64_references_equal_float64_autograd_and_int64_einsum(K):
    V_in, V_out, Cin, Cout = 23, 19, 7, 5
    nbr = _table(K, V_in, V_out, seed=K)
    x = H.int_tensor((V_in, Cin), -4, 4, 1, zero_rows=0.2)
    W = H.int_tensor((K, Cin, Cout), -3, 3, 2)
    dy = H.int_tensor((V_out, Cout), -3, 3, 3)
    acc0 = H.int_tensor((V_out, Cout), -9, 9, 4)
    assert bool((x == 0).all(1).any())
    H.assert_exact_range(x, W, nbr, V_out)
    H.assert_exact_range(x, dy, nbr, V_out)

    a = x.double().requires_grad_(True)
    w = W.double().requires_grad_(True)
    out64 = _float64_ref(a, w, nbr, V_out)
    out64.backward(dy.double())
    fwd = H.ref_forward(x, W, nbr, V_out)
    assert fwd.dtype == torch.int64 and torch.equal(fwd.double(), out64.detach())
    assert torch.equal(H.ref_forward(x, W, nbr, V_out, acc0), fwd + acc0.long())
    dW = H.ref_wgrad(x, dy, nbr, V_out)
    assert dW.dtype == torch.int64 and torch.equal(dW.double(), w.grad)
    dX = H.ref_dgrad(dy, W, nbr, V_in, V_out)
    assert torch.equal(dX.double(), a.grad)

    # plain int64 arithmetic over the explicit pairs: no float anywhere
    xi, Wi, di = x.long(), W.long(), dy.long()
    fwd_i = torch.zeros((V_out, Cout), dtype=torch.int64)
    dW_i = torch.zeros((K, Cin, Cout), dtype=torch.int64)
    for k in range(K):
        for o in range(V_out):
            i = int(nbr[k, o])
            if i >= 0:
                fwd_i[o] += torch.einsum("c,cn->n", xi[i], Wi[k])
                dW_i[k] += torch.einsum("c,n->cn", xi[i], di[o])
    assert torch.equal(fwd, fwd_i) and torch.equal(dW, dW_i)
    if K > 1:
        assert not dW[K // 2].any()  # the offset without a pair


def test_dense_rows_are_the_one_offset_identity_table():
    V, Cin, Cout = 17, 6, 4
    x = H.int_tensor((V, Cin), -4, 4, 5)
    W = H.int_tensor((1, Cin, Cout), -3, 3, 6)
    dy = H.int_tensor((V, Cout), -3, 3, 7)
    nbr = H.dense_nbr(V)
    assert torch.equal(H.ref_forward(x, W, nbr, V), x.long() @ W[0].long())
    assert torch.equal(H.ref_wgrad(x, dy, nbr, V)[0], x.long().t() @ dy.long())


def test_assert_exact_range_raises_beyond_2_to_24():
    # one output row that sums 27 * 1024 products of 32 * 32 = 2^10 each: 27 * 2^20 > 2^24
    K, Cin = 27, 1024
    x = torch.full((1, Cin), 32.0)
    W = torch.full((K, Cin, 2), -32.0)
    nbr = torch.zeros((K, 1), dtype=torch.int32)
    with pytest.raises(AssertionError, match="2\\^24"):
        H.assert_exact_range(x, W, nbr, 1)
    # the signed sum cancels to 0: the precondition looks at the absolute terms
    W[:, ::2] = 32.0
    assert int(H.ref_forward(x, W, nbr, 1).abs().max()) == 0
    with pytest.raises(AssertionError, match="2\\^24"):
        H.assert_exact_range(x, W, nbr, 1)
    # the weight gradient's sums: 2^15 pairs of 2^5 * 2^5 = 2^25
    V = 1 << 15
    with pytest.raises(AssertionError, match="2\\^24"):
        H.assert_exact_range(torch.full((V, 1), 32.0), torch.full((V, 1), 32.0), H.dense_nbr(V), V)
    # just inside: the issue's widest case, |x| <= 4, |W| <= 3, K = 27, Cin = 448 -> 145 152
    x = torch.full((1, 448), 4.0)
    W = torch.full((27, 448, 1), -3.0)
    assert H.assert_exact_range(x, W, nbr, 1) == 145152
    # operands that are not bf16-exact integers, or no integers at all, are refused too
    with pytest.raises(AssertionError, match="bf16-exact"):
        H.assert_exact_range(torch.full((1, 4), 257.0), torch.ones(1, 4, 1), nbr[:1], 1)
    with pytest.raises(AssertionError, match="integer-valued"):
        H.assert_exact_range(torch.full((1, 4), 0.5), torch.ones(1, 4, 1), nbr[:1], 1)


def test_epilogue_reference_values_and_zeros():
    acc = torch.tensor([[-6, 0, 5, 3]], dtype=torch.int64)
    scale = torch.tensor([0.5, -1.0, 2.0, -0.5])
    shift = torch.tensor([1.0, 0.0, -10.0, 0.0])
    res = torch.tensor([[0.0, 0.0, 1.0, 0.0]])
    none = H.ref_epilogue(acc, scale, shift, res, 0)
    assert none.dtype == torch.float32 and none.tolist() == [[-2.0, 0.0, 1.0, -1.5]]
    assert H.ref_epilogue(acc, scale, shift, res, 1).tolist() == [[0.0, 0.0, 1.0, 0.0]]
    assert H.ref_epilogue(acc, scale, shift, res, 2).tolist() == [[-0.5, 0.0, 1.0, -0.375]]
    # 0 * (-1) + (+0) is +0, relu(negative) is +0: no negative zero comes out
    for act in (0, 1, 2):
        assert not (H.bits_of(H.ref_epilogue(acc, scale, shift, res, act)) == 0x80000000).any()
    with pytest.raises(AssertionError, match="epilogue"):
        H.ref_epilogue(torch.tensor([[1 << 20]]), torch.tensor([4.0]))


def test_generators_are_deterministic_and_shaped():
    c = H.int_cloud(1, 600)
    assert c.dtype.kind == "i" and c.shape[1] == 3 and 600 <= len(c) <= 1500
    assert (H.int_cloud(1, 600) == c).all() and len({tuple(r) for r in c.tolist()}) == len(c)
    s = H.scatter_cloud(2, 1200)
    assert 1000 <= len(s) <= 1200 and (H.scatter_cloud(2, 1200) == s).all()
    t = H.int_tensor((50, 8), -4, 4, 3, zero_rows=0.3)
    assert t.dtype == torch.float32 and bool((t == t.round()).all()) and float(t.abs().max()) == 4.0
    assert 5 <= int((t == 0).all(1).sum()) <= 30
    assert set(H.scale_tensor(200, 1).tolist()) == set(H.SCALES)
    # the rounding table: the ties go to the even neighbour, the largest finite value to Inf
    r = H.rne_bf16(H.from_bits(H.TIES + (H.MAX_FINITE,)))
    assert H.bits_of(r).tolist() == [0x3F800000, 0x3F820000, 0xBF800000, 0x3F810000, 0x7F800000]
