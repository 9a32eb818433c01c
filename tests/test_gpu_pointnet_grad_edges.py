"""The PointNet++ training kernels (csrc/sv_pointnet_grad.hip: sv_group_rows, sv_index_transpose, sv_gather_transpose,
sv_group_max, sv_group_max_backward, sv_three_nn_gather) and their autograd Functions against the numpy restatements of
tests/pointnet_grad_helpers.py (pinned by tests/test_pointnet_grad_cpu.py), on bit patterns and integers only: row strides
wider than the columns with canaries around every output, indices outside the cloud, both sides of the one-workgroup
sort's 8192-pair limit, many references to one target, the fixed ascending summation order on inputs that a descending
sum would change, and the max rule at NaN, ties, signed zeros and infinities."""
import numpy as np
import pytest
import torch

import pointnet_grad_helpers as H

pytestmark = pytest.mark.gpu

CANARY = -7.5
INT64_MIN = np.iinfo(np.int64).min


@pytest.fixture(scope="module")
def P2(gpu):
    from mrcc_amd.model import pointnet2_utils

    return pointnet2_utils


@pytest.fixture(scope="module")
def L(gpu):
    from mrcc_amd import _lib

    _lib.load()
    return _lib


def _dev(a, gpu):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _canary(shape, gpu, dtype=torch.float32):
    return torch.full(shape, CANARY if dtype == torch.float32 else -77, dtype=dtype, device=gpu)


def _untouched(t):
    return bool((t == (CANARY if t.dtype == torch.float32 else -77)).all())


# ---- 1. sv_group_rows ------------------------------------------------------------------------------------------------
def _mixed_table(rng, B, N, S, K):
    """valid indices with every third entry (from the second on) one of -1, N, N + 1, 2^32 + 2, INT64_MIN in turn"""
    idx = rng.integers(0, N, B * S * K).astype(np.int64)
    bad = [-1, N, N + 1, 2 ** 32 + 2, INT64_MIN]
    for n, i in enumerate(range(1, len(idx), 3)):
        idx[i] = bad[n % 5]
    return idx.reshape(B, S, K)


def _group_rows(L, gpu, xyz, pts, new_xyz, idx, order, ld, guard=3):
    B, N, _ = xyz.shape
    D = 0 if pts is None else pts.shape[2]
    S, K = (1, N) if idx is None else idx.shape[1:]
    R = B * S * K
    out = _canary((R + guard, ld), gpu)
    args = [_dev(a, gpu) for a in (xyz, pts, new_xyz, idx)]
    rc = L.load().sv_group_rows(*[L.ptr(a) for a in args], B, N, D, S, K, order, ld, L.ptr(out), L.stream_ptr())
    assert rc == 0
    assert _untouched(out[R:]), "rows past B * S * nsample were written"
    return out[:R].cpu().numpy()


@pytest.mark.parametrize("order", [H.SSG, H.MSG], ids=["ssg", "msg"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 7, 1, 1), (3, 130, 5, 16), (2, 300, 7, 33)], ids=str)
def test_group_rows_strides_and_out_of_range_indices(L, gpu, order, shape):
    B, N, S, K = shape
    for D in (0, 1, 5):
        rng = np.random.default_rng(100 * D + N + order)
        xyz = rng.random((B, N, 3), dtype=np.float32)
        pts = rng.standard_normal((B, N, D)).astype(np.float32) if D else None
        new_xyz = rng.random((B, S, 3), dtype=np.float32)
        idx = _mixed_table(rng, B, N, S, K)
        if B * S * K > 1:
            assert ((idx < 0) | (idx >= N)).any() and ((idx >= 0) & (idx < N)).any()
        for ld in (3 + D, 3 + D + 1, 3 + D + 5):
            got = _group_rows(L, gpu, xyz, pts, new_xyz, idx, order, ld)
            assert H.same_bits(got, H.group_rows_ref(xyz, pts, new_xyz, idx, order, ld)), (D, ld)


@pytest.mark.parametrize("D", [0, 7])
def test_group_rows_group_all_wide_rows(L, gpu, D):
    rng = np.random.default_rng(D)
    B, N = 2, 130
    xyz = rng.random((B, N, 3), dtype=np.float32)
    pts = rng.standard_normal((B, N, D)).astype(np.float32) if D else None
    for ld in (3 + D, 3 + D + 2):
        got = _group_rows(L, gpu, xyz, pts, None, None, H.SSG, ld)
        assert H.same_bits(got, H.group_rows_ref(xyz, pts, None, None, H.SSG, ld)), ld


# ---- 2. sv_index_transpose -------------------------------------------------------------------------------------------
def _transpose(L, gpu, idx, N):
    """(offsets, pos[:offsets[-1]]) of sv_index_transpose on the host table idx [B, M] (int32 or int64)"""
    B, M = idx.shape
    lib = L.load()
    nbytes = lib.sv_index_transpose_workspace_bytes(B, M, N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
    table = _dev(idx, gpu)
    offsets = _canary((B * N + 1 + 2,), gpu, torch.int32)
    pos = _canary((B * M + 2,), gpu, torch.int32)
    rc = lib.sv_index_transpose(L.ptr(table) if table.numel() else None, idx.dtype.itemsize, B, M, N, L.ptr(ws), nbytes,
                                L.ptr(offsets), L.ptr(pos), L.stream_ptr())
    assert rc == 0
    assert _untouched(offsets[B * N + 1:]) and _untouched(pos[B * M:])
    o = offsets[:B * N + 1].cpu().numpy()
    return o, pos[:int(o[-1])].cpu().numpy()


def _check_transpose(L, gpu, idx, N):
    want_o, want_p = H.index_transpose_ref(idx, N)
    got_o, got_p = _transpose(L, gpu, idx, N)
    assert got_o.dtype == np.int32 and np.array_equal(got_o, want_o)
    assert np.array_equal(got_p, want_p)
    return got_o, got_p


TABLES = [(1, 1, 1), (2, 37, 64), (1, 8192, 300), (1, 8193, 300), (2, 10000, 2048), (1, 20000, 70000)]


@pytest.mark.parametrize("dtype", [np.int32, np.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("shape", TABLES, ids=str)
def test_index_transpose_tables(L, gpu, shape, dtype):
    """the smallest table; B * N = 128, a power of two, where the sentinel key B * N needs one bit more than the targets;
    8192 and 8193 pairs, the two sides of the one-workgroup sort; several tiles with a partial last one; 17 key bits"""
    B, M, N = shape
    rng = np.random.default_rng(M + N)
    idx = rng.integers(0, N, (B, M)).astype(dtype)
    if M > 1:
        out = rng.random((B, M)) < 0.08
        bad = np.array([-1, N, N + 1, np.iinfo(dtype).min, np.iinfo(dtype).max], dtype=dtype)
        idx[out] = bad[rng.integers(0, 5, int(out.sum()))]
        assert out.any()
    o, p = _check_transpose(L, gpu, idx, N)
    assert o[-1] == ((idx >= 0) & (idx < N)).sum()
    o2, p2 = _transpose(L, gpu, idx, N)  # a second call: the same result
    assert np.array_equal(o, o2) and np.array_equal(p, p2)


@pytest.mark.parametrize("dtype", [np.int32, np.int64], ids=["int32", "int64"])
def test_index_transpose_degenerate_tables(L, gpu, dtype):
    N = 50
    nothing = np.full((2, 300), N, dtype=dtype)  # every entry out of range: every offset 0
    nothing[0, ::2] = -3
    o, p = _check_transpose(L, gpu, nothing, N)
    assert not o.any() and len(p) == 0
    one = np.full((1, 9000), 17, dtype=dtype)  # 9000 references to one target, on the multi-workgroup sort
    o, p = _check_transpose(L, gpu, one, N)
    assert np.array_equal(p, np.arange(9000)) and o[17] == 0 and o[18] == 9000
    few = np.full((1, 5000), 17, dtype=dtype)  # and on the one-workgroup sort
    few[0, 1::2] = 3
    o, p = _check_transpose(L, gpu, few, N)
    assert np.array_equal(p, np.concatenate([np.arange(1, 5000, 2), np.arange(0, 5000, 2)]))
    o, p = _check_transpose(L, gpu, np.zeros((2, 0), dtype=dtype), 5)  # M = 0
    assert o.shape == (11,) and not o.any()
    o, p = _check_transpose(L, gpu, np.zeros((0, 4), dtype=dtype), 5)  # B = 0
    assert o.shape == (1,) and o[0] == 0


def test_index_transpose_negative_int32_and_wide_int64(L, gpu):
    """int32 entries below zero are dropped, and so are int64 entries >= 2^32 whose low 32 bits are a valid index"""
    rng = np.random.default_rng(4)
    B, M, N = 2, 500, 40
    neg = rng.integers(-N, N, (B, M)).astype(np.int32)
    o, _ = _check_transpose(L, gpu, neg, N)
    assert o[-1] == (neg >= 0).sum() < B * M
    wide = rng.integers(0, N, (B, M)).astype(np.int64)
    high = rng.random((B, M)) < 0.3
    wide[high] += rng.integers(1, 2 ** 31, int(high.sum())).astype(np.int64) << 32
    assert ((wide[high] & 0xFFFFFFFF) < N).all()
    o, _ = _check_transpose(L, gpu, wide, N)
    assert o[-1] == (~high).sum()


# ---- 3. sv_gather_transpose ------------------------------------------------------------------------------------------
def _gather(L, gpu, d, case, T):
    C, ld_out = case["C"], case["C"] + case["pad_out"]
    offsets, pos, w, rows = (_dev(d[k], gpu) for k in ("offsets", "pos", "w", "rows"))  # alive until the call returns
    out = _canary((T + 2, ld_out), gpu)
    rc = L.load().sv_gather_transpose(L.ptr(offsets), L.ptr(pos), L.ptr(w), L.ptr(rows), d["ld_rows"], case["col0"], C,
                                      case["per_row"], T, L.ptr(out), ld_out, L.stream_ptr())
    assert rc == 0
    assert _untouched(out[T:]) and _untouched(out[:T, C:]), "written outside the [T, C] block"
    return out[:T, :C].cpu().numpy()


@pytest.mark.parametrize("case", H.GATHER_GRID + H.GATHER_BIG, ids=H.gather_id)
def test_gather_transpose_has_the_bits_of_the_ascending_sum(L, gpu, case):
    d = H.gather_case(case)
    T, C = H.GATHER_T, case["C"]
    assert (T * C) % 256 != 0
    got = _gather(L, gpu, d, case, T)
    want = H.gather_transpose_ref(d["offsets"], d["pos"], d["w"], d["rows"], case["col0"], C, case["per_row"])
    assert H.same_bits(got, want), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert np.array_equal(got[1].view(np.uint32), np.zeros(C, dtype=np.uint32))  # target 1 has no reference: +0.0
    # the NaN and the inf of `rows` reach the targets that reference their rows, in their columns, and nothing else
    assert {(int(t), int(c)) for t, c in zip(*np.nonzero(np.isnan(got)))} == d["nan_targets"]
    assert {(int(t), int(c)) for t, c in zip(*np.nonzero(np.isinf(got)))} == d["inf_targets"]
    assert d["nan_targets"]
    if case.get("big"):
        assert np.diff(d["offsets"]).max() > 1000


@pytest.mark.parametrize("weighted", [False, True])
def test_gather_transpose_negative_zeros_and_no_targets(L, gpu, weighted):
    """rows of -0.0 only: a target without a reference is +0.0 (not a row's value), and so is a sum that starts from +0.0;
    T = 0 returns OK without a launch"""
    case = dict(weighted=weighted, per_row=1, col0=0, C=5, pad_rows=0, pad_out=0)
    d = H.gather_case(case, specials=False)
    d["rows"] = np.full_like(d["rows"], -0.0)
    got = _gather(L, gpu, d, case, H.GATHER_T)
    assert np.array_equal(got.view(np.uint32), np.zeros(got.shape, dtype=np.uint32))
    assert H.same_bits(got, H.gather_transpose_ref(d["offsets"], d["pos"], d["w"], d["rows"], 0, 5, 1))
    out = _canary((4,), gpu)
    rc = L.load().sv_gather_transpose(None, None, None, None, 5, 0, 5, 1, 0, L.ptr(out), 5, L.stream_ptr())
    assert rc == 0 and _untouched(out)


# ---- 4. sv_group_max -------------------------------------------------------------------------------------------------
def _max_rows(G, K, C, rot):
    """[G * K, C] of small integers (many repeated maxima); column (g, c) follows pattern (3 g + c + rot) % 8: 0 plain,
    1 NaN at k = 0, 2 NaN in the middle and again later, 3 NaN at the last k, 4 / 5 +0.0 before -0.0 / -0.0 before +0.0
    over negatives, 6 all -inf, 7 +inf twice"""
    rng = np.random.default_rng(G * 7 + K * 3 + C + rot)
    v = rng.integers(-3, 4, (G, K, C)).astype(np.float32)
    g, c = np.meshgrid(np.arange(G), np.arange(C), indexing="ij")
    pat = (3 * g + c + rot) % 8
    mid, late, last = K // 2, min(K // 2 + 2, K - 1), K - 1

    def put(mask, k, val):
        gi, ci = np.nonzero(mask)
        v[gi, k, ci] = val

    put(pat == 1, 0, np.nan)
    put(pat == 2, mid, np.nan)
    put(pat == 2, late, np.nan)
    put(pat == 3, last, np.nan)
    for p, (first, second) in ((4, (0.0, -0.0)), (5, (-0.0, 0.0))):
        gi, ci = np.nonzero(pat == p)
        v[gi, :, ci] = -5.0
        put(pat == p, last, second)
        put(pat == p, mid if mid != last else 0, first)
    gi, ci = np.nonzero(pat == 6)
    v[gi, :, ci] = -np.inf
    put(pat == 7, mid, np.inf)
    put(pat == 7, last, np.inf)
    return v.reshape(G * K, C)


def _group_max(L, gpu, wide, col, C, K):
    """sv_group_max on columns col .. col + C of the device rows `wide` -> (values, arg)"""
    G = wide.shape[0] // K
    out, arg = _canary((G + 1, C), gpu), _canary((G + 1, C), gpu, torch.int32)
    view = wide[:, col:col + C]
    rc = L.load().sv_group_max(L.ptr(view), wide.stride(0), G, K, C, L.ptr(out), L.ptr(arg), L.stream_ptr())
    assert rc == 0 and view.data_ptr() == wide.data_ptr() + 4 * col
    assert _untouched(out[G:]) and _untouched(arg[G:])
    return out[:G].cpu().numpy(), arg[:G].cpu().numpy()


MAX_CASES = [(1, 1, 1), (5, 1, 65), (1, 2, 63), (5, 2, 64), (5, 16, 1), (1, 16, 1024), (5, 16, 65), (1, 128, 64),
             (5, 128, 63), (5, 128, 1024), (1, 1000, 65), (5, 1000, 1), (1, 1000, 1024)]


@pytest.mark.parametrize("case", MAX_CASES, ids=str)
def test_group_max_values_and_arg(L, P2, gpu, case):
    G, K, C = case
    for rot in (range(8) if G * C < 8 else (0,)):
        rows = _max_rows(G, K, C, rot)
        want_v, want_a = H.group_max_ref(rows, K)
        if K > 2 and G * C >= 8:
            assert np.isnan(want_v).any() and np.isinf(want_v).any() and (want_v == 0).any()
        for pad in (0, 3):  # ld = C and ld = C + 3 (the columns start one float into the wider row)
            wide = np.full((G * K, C + pad), 99.0, dtype=np.float32)  # a maximum the kernel must not see
            col = 1 if pad else 0
            wide[:, col:col + C] = rows
            dev = _dev(wide, gpu)
            got_v, got_a = _group_max(L, gpu, dev, col, C, K)
            assert H.same_bits(got_v, want_v) and got_a.dtype == np.int32 and np.array_equal(got_a, want_a), (rot, pad)
            fv, fa = P2.GroupMaxFunction.apply(dev[:, col:col + C], K, None)  # the Function on a column slice
            assert H.same_bits(fv.cpu().numpy(), want_v) and np.array_equal(fa.cpu().numpy(), want_a), (rot, pad)


# ---- 5. sv_group_max_backward ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(3, 1, 65), (5, 16, 1), (2, 33, 65), (7, 5, 1)], ids=str)
def test_group_max_backward(L, gpu, case):
    G, K, C = case
    assert (G * K * C) % 256 != 0
    rng = np.random.default_rng(G + K + C)
    dp = rng.standard_normal((G, C)).astype(np.float32)
    dp.reshape(-1)[::3] = -0.0
    dp.reshape(-1)[1::5] = np.nan
    arg = rng.integers(0, K, (G, C)).astype(np.int32)
    drows = _canary((G * K + 2, C), gpu)
    dp_d, arg_d = _dev(dp, gpu), _dev(arg, gpu)
    rc = L.load().sv_group_max_backward(L.ptr(dp_d), L.ptr(arg_d), G, K, C, L.ptr(drows), L.stream_ptr())
    assert rc == 0 and _untouched(drows[G * K:])
    got = drows[:G * K].cpu().numpy()
    assert H.same_bits(got, H.group_max_backward_ref(dp, arg, K))
    if K == 1:
        assert H.same_bits(got, dp)
    g3 = got.reshape(G, K, C)
    at = np.zeros((G, K, C), dtype=bool)
    at[np.arange(G)[:, None], arg, np.arange(C)[None]] = True
    assert H.same_bits(np.take_along_axis(g3, arg[:, None, :].astype(np.int64), axis=1)[:, 0], dp)  # -0.0, NaN as they are
    assert np.array_equal(g3[~at].view(np.uint32), np.zeros(int((~at).sum()), dtype=np.uint32))  # +0.0 elsewhere


# ---- 6. sv_three_nn_gather -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 33])
def test_three_nn_gather_out_of_range_rows_are_nan(L, gpu, oracle, C):
    B, N, S = 2, 50, 9
    assert (B * N * C) % 256 != 0
    rng = np.random.default_rng(C)
    p2 = rng.standard_normal((B, S, C)).astype(np.float32)
    w = rng.random((B, N, 3), dtype=np.float32)
    idx = rng.integers(0, S, (B, N, 3)).astype(np.int32)
    safe = idx.copy()
    bad_rows = np.zeros((B, N), dtype=bool)
    for n, (b, q) in enumerate([(0, 0), (0, 7), (0, 49), (1, 0), (1, 13), (1, 48), (1, 49)]):
        idx[b, q, n % 3] = (-1, S, 2 ** 30)[(n // 3 + n) % 3]
        bad_rows[b, q] = True
    out = _canary((B * N + 1, C), gpu)
    p2_d, idx_d, w_d = _dev(p2, gpu), _dev(idx, gpu), _dev(w, gpu)
    rc = L.load().sv_three_nn_gather(L.ptr(p2_d), L.ptr(idx_d), L.ptr(w_d), B, N, S, C, L.ptr(out), L.stream_ptr())
    assert rc == 0 and _untouched(out[B * N:])
    got = out[:B * N].cpu().numpy().reshape(B, N, C)
    want = oracle.three_nn_gather(p2, safe, w)
    assert {int(v) for v in idx[bad_rows].reshape(-1) if v < 0 or v >= S} == {-1, S, 2 ** 30}
    assert np.isnan(got[bad_rows]).all()
    assert H.same_bits(got[~bad_rows], want[~bad_rows])


# ---- 7. the autograd Functions ---------------------------------------------------------------------------------------
def _rows_grad(P2, gpu, c, idx, order, drows, new_xyz=None, grad=None):
    """points.grad of GroupRowsFunction for the upstream gradient drows (a device tensor, taken as it is)"""
    pts = _dev(c["points"], gpu).requires_grad_()
    nx = c["new_xyz"] if new_xyz is None else new_xyz
    rows = P2.group_rows(_dev(c["xyz"], gpu), pts, _dev(nx, gpu), _dev(idx, gpu), order)
    assert rows.shape == drows.shape
    g1, = torch.autograd.grad(rows, pts, drows, retain_graph=True)
    g2, = torch.autograd.grad(rows, pts, drows)  # a second backward: the same bits
    assert H.same_bits(g1.cpu().numpy(), g2.cpu().numpy())
    return rows.detach().cpu().numpy(), g1.cpu().numpy()


@pytest.mark.parametrize("order", [H.SSG, H.MSG], ids=["ssg", "msg"])
@pytest.mark.parametrize("D", [1, 5])
def test_group_rows_function_backward(P2, gpu, order, D):
    c = H.group_rows_grad_case(order, D)
    B, N, _ = c["xyz"].shape
    fwd, grad = _rows_grad(P2, gpu, c, c["idx"], order, _dev(c["drows"], gpu))
    assert H.same_bits(fwd, H.group_rows_ref(c["xyz"], c["points"], c["new_xyz"], c["idx"], order, 3 + D))
    want = H.gather_transpose_ref(*H.index_transpose_ref(c["idx"], N), None, c["drows"], c["col0"], D, 1)
    assert H.same_bits(grad.reshape(B * N, D), want)
    # an upstream gradient whose columns are not contiguous
    strided = _dev(np.ascontiguousarray(c["drows"].T), gpu).t()
    assert strided.stride(1) != 1
    assert H.same_bits(_rows_grad(P2, gpu, c, c["idx"], order, strided)[1], grad)


@pytest.mark.parametrize("order", [H.SSG, H.MSG], ids=["ssg", "msg"])
def test_group_rows_function_backward_with_an_empty_ball(P2, gpu, order):
    """a ball whose every entry is N (sv_ball_query's empty ball): its rows are NaN and take no part in the gradient -
    the gradient of the table without that ball"""
    D = 5
    c = H.group_rows_grad_case(order, D, seed=1)
    c = {k: (v[:1] if k in ("xyz", "points", "new_xyz", "idx") else v) for k, v in c.items()}
    N, (_, S, K) = c["xyz"].shape[1], c["idx"].shape
    drows = c["drows"][:S * K]
    idx = c["idx"].copy()
    idx[0, 2] = N
    fwd, grad = _rows_grad(P2, gpu, c, idx, order, _dev(drows, gpu))
    assert np.isnan(fwd[2 * K:3 * K]).all() and not np.isnan(np.delete(fwd, np.s_[2 * K:3 * K], axis=0)).any()
    keep = np.delete(np.arange(S), 2)
    _, without = _rows_grad(P2, gpu, c, c["idx"][:, keep], order, _dev(np.delete(drows, np.s_[2 * K:3 * K], axis=0), gpu),
                            new_xyz=c["new_xyz"][:, keep])
    assert H.same_bits(grad, without)
    want = H.gather_transpose_ref(*H.index_transpose_ref(idx, N), None, drows, c["col0"], D, 1)
    assert H.same_bits(grad.reshape(N, D), want) and not np.isnan(grad).any()


def test_group_rows_function_group_all_backward(P2, gpu):
    rng = np.random.default_rng(8)
    B, N, D = 2, 37, 4
    pts = _dev(rng.standard_normal((B, N, D)).astype(np.float32), gpu).requires_grad_()
    rows = P2.group_rows(_dev(rng.random((B, N, 3), dtype=np.float32), gpu), pts, None, None, H.SSG)
    drows = H.wide_values(rng, (B * N, 3 + D))
    g, = torch.autograd.grad(rows, pts, _dev(drows, gpu))
    assert H.same_bits(g.cpu().numpy(), drows.reshape(B, N, 3 + D)[:, :, 3:])


def test_three_nn_gather_function_backward(P2, gpu):
    c = H.three_nn_grad_case()
    B, N, C = c["dout"].shape
    S = c["points2"].shape[1]
    p2 = _dev(c["points2"], gpu).requires_grad_()
    out = P2.three_nn_gather(p2, _dev(c["idx"], gpu), _dev(c["w"], gpu))
    g1, = torch.autograd.grad(out, p2, _dev(c["dout"], gpu), retain_graph=True)
    g2, = torch.autograd.grad(out, p2, _dev(c["dout"], gpu))
    want = H.gather_transpose_ref(*H.index_transpose_ref(c["idx"].reshape(B, N * 3), S), c["w"].reshape(-1),
                                  c["dout"].reshape(B * N, C), 0, C, 3)
    assert H.same_bits(g1.cpu().numpy().reshape(B * S, C), want)
    assert H.same_bits(g1.cpu().numpy(), g2.cpu().numpy())
    assert not g1[:, S - 1].any()  # the source nothing references
