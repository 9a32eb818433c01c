"""The bf16 forward (sv_conv_fwd_bf16) and both weight-gradient kernels (sv_conv_wgrad, sv_conv_wgrad_bf16) against
exact integer references on EVERY element (tests/conv_exact_helpers.py): with small-integer operands every product and
every partial sum is exact in fp32 in any order, so the kernels must return the int64 gather / index_add result of the
raw kernel map bit for bit.  Covered: every column-block instance of the bf16 forward on every map kind (the strided maps
with whole plan tiles of rows without a neighbour included), dense row-count edges, offset-range
passes with empty workgroups, the in-register fp32 -> bf16 rounding of both kernels on a table of special values, odd
shapes and misaligned bases of the fp32 weight gradient, and batch-range launches (ConvPlan.chunks) of everything but
the fp32 forward.  Non-integer data stays under the tolerance tests (test_gpu_conv_bf16.py, test_gpu_conv_grad.py,
test_gpu_training_bf16.py)."""
import numpy as np
import pytest
import torch

import conv_exact_helpers as H
import strided_helpers as S

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
# Cout -> the column block TN = 16 NT of the instance sv_conv_fwd_bf16 picks (the widest of 24, 16, 12, 8, 6, 4, 2, 1
# column tiles that divides Cout / 16)
COUT_TN = {64: 64, 80: 16, 96: 96, 128: 128, 160: 32, 192: 192, 256: 256, 384: 384}
KINDS = ("k3", "down", "up", "dense")
# kernel maps of the strided layers: V_out < V_in, K = 1 with a plan, and the two transposed maps on which about 7 output rows
# of 8 have no neighbour at all (whole plan tiles of real rows with all-zero submask words)
STRIDED_KINDS = ("k3s2", "k1s2", "k1s2_t", "k3s2d2_t")

_frames = {}
_checked = set()


def _frame(gpu, name, clouds):
    """coordinate manager of a batch of integer clouds (an empty cloud leaves its batch index empty), built once"""
    if name not in _frames:
        from mrcc_amd import MinkowskiEngine as ME

        coords = np.concatenate([np.concatenate([np.full((len(c), 1), b), c], 1) for b, c in enumerate(clouds) if len(c)])
        st = ME.SparseTensor(torch.zeros(len(coords), 1), coordinates=torch.from_numpy(coords).int(), device=gpu)
        cm = st.coordinate_manager
        cm.plan_down(1)  # the coarse map and its parent table (a transposed conv writes onto an existing map)
        _frames[name] = cm
    return _frames[name]


def _one(gpu):
    return _frame(gpu, "one", [H.int_cloud(1, 600)])


def _two(gpu):
    return _frame(gpu, "two", [H.int_cloud(7, 800), H.int_cloud(8, 550)])


def _scatter(gpu):
    return _frame(gpu, "scatter", [H.scatter_cloud(2, 1200)])


def _map(cm, kind, V_dense=300):
    """(plan, nbr table, V_in, V_out, K) of a map kind on a frame"""
    V1, V2 = cm.stride_map(1).V, cm.stride_map(2).V
    if kind in STRIDED_KINDS:  # the strided maps of the ResNets (strided_helpers.MAP_KINDS), raw table held to probe_ref
        plan = S.kind_plan(cm, kind)
        if (id(cm), kind) not in _checked:
            nbr, V_in, V_out = S.kind_table_of(cm.stride_map(1).coords.cpu().numpy(), kind)
            assert (plan.V_out, cm.stride_map(plan.in_stride).V) == (V_out, V_in)
            assert np.array_equal(plan.raw[0][:, :V_out].cpu().numpy(), nbr)
            _checked.add((id(cm), kind))
        return plan, plan.raw[0], cm.stride_map(plan.in_stride).V, plan.V_out, plan.K
    if kind == "k3":
        plan = cm.plan_k3(1)
        return plan, plan.raw[0], V1, V1, 27
    if kind == "down":
        plan = cm.plan_down(1)
        return plan, plan.raw[0], V1, V2, 8
    if kind == "up":
        plan = cm.plan_up(2)
        return plan, plan.raw[0], V2, V1, 8
    return None, H.dense_nbr(V_dense, cm.device), V_dense, V_dense, 1


def _ints(gpu, shape, lo, hi, seed, zero_rows=0.0):
    return H.int_tensor(shape, lo, hi, seed, zero_rows).to(gpu)


def _exact(got, want_int):
    """every element equals the int64 reference (an fp32 holds it exactly)"""
    assert got.dtype == torch.float32
    same = torch.equal(got.double(), want_int.double())
    if not same:
        bad = (got.double() != want_int.double())
        first = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{int(bad.sum())} of {bad.numel()} elements differ, first at {first}: "
                             f"got {got[tuple(first)].item()}, want {want_int[tuple(first)].item()}")


def _bits(got, want, what=""):
    if not H.same_bits(got, want):
        bad = got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)
        first = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {first}: "
                             f"got {got[tuple(first)].item()!r}, want {want[tuple(first)].item()!r}")


# ---------------------------------------------------------------------------------------------------------------------
# a. bf16 forward: every column-block instance x every map kind, raw and with the whole epilogue on strided operands
# ---------------------------------------------------------------------------------------------------------------------
def _fwd_case(gpu, cm, kind, cin, cout, seed):
    from mrcc_amd import _lib
    from mrcc_amd import nn as svnn

    plan, nbr, V_in, V_out, K = _map(cm, kind)
    assert V_out % 16 != 0 or kind == "dense"  # a partial last sub-tile
    xbuf = _ints(gpu, (V_in, cin + 8), -4, 4, seed, zero_rows=0.2)
    x = xbuf[:, 4:4 + cin]  # a column slice at a 16-byte-aligned offset of a wider buffer
    assert x.data_ptr() % 16 == 0 and x.stride(0) == cin + 8
    W = _ints(gpu, (K, cin, cout), -3, 3, seed + 1)
    H.assert_exact_range(x, W, nbr, V_out)
    want = H.ref_forward(x, W, nbr, V_out)
    wp = svnn.pack_weights_bf16(W)
    name = f"conv_bf16_kernel<128, {COUT_TN[cout]}>"

    raw = svnn.conv_forward(x.contiguous(), W, plan, V_out, weight_bf16=wp)
    assert _lib.conv_last_instance()[0] == name, (_lib.conv_last_instance(), name)
    _exact(raw, want)

    scale = H.scale_tensor(cout, seed + 2).to(gpu)
    shift = _ints(gpu, (cout,), -8, 8, seed + 3)
    rbuf = _ints(gpu, (V_out, cout + 6), -8, 8, seed + 4, zero_rows=0.2)
    res = rbuf[:, 3:3 + cout]
    for act in (ACT_RELU, ACT_LEAKY):
        buf = torch.full((V_out, cout + 9), 7.0, device=gpu)
        out = buf[:, 5:5 + cout]
        svnn.conv_forward(x, W, plan, V_out, scale, shift, res, act, H.LEAKY_SLOPE, out=out, weight_bf16=wp)
        assert _lib.conv_last_instance()[0] == name
        _bits(out, H.ref_epilogue(want, scale, shift, res, act), f"{kind} {cin}->{cout} act {act}")
        assert (buf[:, :5] == 7.0).all() and (buf[:, 5 + cout:] == 7.0).all()


@pytest.mark.parametrize("cin", [64, 96])
@pytest.mark.parametrize("cout", sorted(COUT_TN))
def test_bf16_forward_every_instance_every_map_exact(gpu, cin, cout):
    cm = _one(gpu)
    for j, kind in enumerate(KINDS):
        _fwd_case(gpu, cm, kind, cin, cout, seed=1000 * cout + 10 * cin + j)


@pytest.mark.parametrize("cout", sorted(COUT_TN))
def test_bf16_forward_every_instance_every_strided_map_exact(gpu, cout):
    """every conv_bf16_kernel<128, TN> on the strided kinds; on the two transposed ones a tile of real rows without any pair
    must still write act(scale * 0 + shift + residual) over the sentinel"""
    cm = _one(gpu)
    for kind in ("k1s2_t", "k3s2d2_t"):
        all_empty, mixed = S.plan_tile_census(_map(cm, kind)[0])
        assert all_empty.any() and mixed.any(), kind
    for j, kind in enumerate(STRIDED_KINDS):
        _fwd_case(gpu, cm, kind, 64, cout, seed=2000 * cout + j)


@pytest.mark.parametrize("kind,cout", [("k3", 192), ("down", 80), ("up", 160), ("dense", 384)])
def test_bf16_forward_five_chunks_exact(gpu, kind, cout):
    _fwd_case(gpu, _one(gpu), kind, 160, cout, seed=77 + cout)


# ---------------------------------------------------------------------------------------------------------------------
# b. bf16 forward: dense row-count edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cout", [80, 384])
def test_bf16_forward_dense_row_edges_exact(gpu, cout):
    from mrcc_amd import _lib
    from mrcc_amd import nn as svnn

    W = _ints(gpu, (1, 64, cout), -3, 3, cout)
    wp = svnn.pack_weights_bf16(W)
    for V in (1, 15, 16, 17, 127, 128, 129, 300):
        x = _ints(gpu, (V, 64), -4, 4, V)
        nbr = H.dense_nbr(V, gpu)
        H.assert_exact_range(x, W, nbr, V)
        buf = torch.full((V + 2, cout), 7.0, device=gpu)  # a row beyond V_out must stay untouched
        svnn.conv_forward(x, W, None, V, out=buf[:V], weight_bf16=wp)
        assert _lib.conv_last_instance()[0] == f"conv_bf16_kernel<128, {COUT_TN[cout]}>"
        _exact(buf[:V], H.ref_forward(x, W, nbr, V))
        assert (buf[V:] == 7.0).all(), V


# ---------------------------------------------------------------------------------------------------------------------
# c. bf16 forward: offset-range passes, workgroups without any active offset
# ---------------------------------------------------------------------------------------------------------------------
def _empty_tiles(sub):
    """tiles of a plan whose sub-tile masks are clear at every offset (the workgroup's amask == 0)"""
    sm = sub.submask.view(-1, sub.K) & 0xFF
    return int((sm == 0).all(1).sum()), sm.shape[0]


@pytest.mark.parametrize("cloud,cin,cout", [("scatter", 64, 96), ("scatter", 96, 80), ("scatter", 384, 384),
                                            ("two", 64, 160), ("two", 96, 128)])
def test_bf16_forward_passes_and_empty_workgroups_exact(gpu, cloud, cin, cout):
    from mrcc_amd import nn as svnn

    cm = _scatter(gpu) if cloud == "scatter" else _two(gpu)
    whole = cm.plan_k3(1)
    V = cm.stride_map(1).V
    nbr = whole.raw[0]
    x = _ints(gpu, (V, cin), -4, 4, cin + cout, zero_rows=0.1)
    W = _ints(gpu, (27, cin, cout), -3, 3, cin * cout)
    H.assert_exact_range(x, W, nbr, V)
    want = H.ref_forward(x, W, nbr, V)
    wp = svnn.pack_weights_bf16(W)
    scale, shift = H.scale_tensor(cout, 5).to(gpu), _ints(gpu, (cout,), -8, 8, 6)
    res = _ints(gpu, (V, cout), -8, 8, 7)
    one_raw = svnn.conv_forward(x, W, whole, V, weight_bf16=wp)
    one_epi = svnn.conv_forward(x, W, whole, V, scale, shift, res, ACT_LEAKY, H.LEAKY_SLOPE, weight_bf16=wp)
    _exact(one_raw, want)
    want_epi = H.ref_epilogue(want, scale, shift, res, ACT_LEAKY)
    _bits(one_epi, want_epi, "one launch")
    for cuts in ((9, 18), 14):
        sp = cm.plan_k3_split(1, cuts)
        assert isinstance(sp, svnn.SplitPlan)
        if cloud == "scatter":
            # the passes without the centre offset: most tiles hold no pair at all, some do
            for k0, k1, sub in sp.parts:
                if not k0 <= 13 < k1:
                    empty, tiles = _empty_tiles(sub)
                    assert empty > tiles // 2 and empty < tiles, (k0, k1, empty, tiles)
        raw = svnn.conv_forward(x, W, sp, V, weight_bf16=wp)
        _exact(raw, want)
        assert torch.equal(raw, one_raw)
        epi = svnn.conv_forward(x, W, sp, V, scale, shift, res, ACT_LEAKY, H.LEAKY_SLOPE, weight_bf16=wp)
        _bits(epi, want_epi, f"cuts {cuts}")
        _bits(epi, one_epi, f"cuts {cuts} against one launch")


# ---------------------------------------------------------------------------------------------------------------------
# d. the activation rounding of sv_conv_fwd_bf16: W = identity gives bf16(x)
# ---------------------------------------------------------------------------------------------------------------------
def _rounding_input(rows, cols, seed):
    """normals with the finite part of the rounding table spread over rows 0..; returns (x, rows of the table)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g)
    finite = H.from_bits(H.TIES + H.ZEROS)
    for j, v in enumerate(finite):  # each value at several rows and columns: every lane quarter, both chunks
        for rep in range(4):
            x[(3 * j + 17 * rep) % rows, (j + 16 * rep + 5) % cols] = v
    return x


def _identity_run(gpu, x, act=ACT_NONE):
    from mrcc_amd import _lib
    from mrcc_amd import nn as svnn

    C = x.shape[1]
    W = torch.eye(C, device=gpu).reshape(1, C, C).contiguous()
    out = svnn.conv_forward(x.to(gpu), W, None, x.shape[0], None, None, None, act, weight_bf16=svnn.pack_weights_bf16(W))
    assert _lib.conv_last_instance()[0].startswith("conv_bf16_kernel")
    return out.cpu()


def _want_rounded(x):
    """RNE to bf16; a zero result is +0: the accumulator chain starts at +0 and x * 0 products are zeros, and an IEEE sum
    of zeros that are not all negative is +0 - so -0 (an input -0, or a value that rounds to -0) comes out as +0"""
    want = H.rne_bf16(x)
    return torch.where(want == 0, torch.zeros_like(want), want)


def test_bf16_forward_rounds_activations_to_nearest_even(gpu):
    x = _rounding_input(300, 64, 1)
    # non-finite values (the largest finite float rounds to Inf) in rows of their own, one per row: a second one in
    # the row would meet a 0 of the identity and turn the first into NaN
    special = H.from_bits((H.MAX_FINITE, H.P_INF, H.N_INF, H.Q_NAN))
    where = [(140, 3), (141, 35), (142, 63), (143, 20), (170, 9), (171, 40), (172, 0), (173, 31)]
    for j, (r, c) in enumerate(where):
        x[r, c] = special[j % 4]
    rows = torch.tensor([r for r, _ in where])
    plain = torch.ones(300, dtype=torch.bool)
    plain[rows] = False
    for act in (ACT_NONE, ACT_RELU):
        out = _identity_run(gpu, x, act)
        want = _want_rounded(x)
        if act == ACT_RELU:
            want = torch.where(want < 0, torch.zeros_like(want), want)
        _bits(out[plain], want[plain], f"finite rows, act {act}")
        for j, (r, c) in enumerate(where):
            got, w = out[r, c], want[r, c]
            if j % 4 == 3:
                assert torch.isnan(got), (r, c, got)  # NaN stays NaN, through ReLU too
            else:
                assert H.bits_of(got) == H.bits_of(w), (r, c, got, w)
    x_ties = H.from_bits(H.TIES)
    assert H.bits_of(_want_rounded(x_ties)).tolist() == [0x3F800000, 0x3F820000, 0xBF800000, 0x3F810000]


def test_bf16_forward_subnormal_activations(gpu):
    """Subnormal fp32 inputs: each output is the RNE-rounded value or a zero (flush); zeros are +0 (see _want_rounded).
    Measured on an MI355X: see DESIGN.md 4.5."""
    x = torch.zeros(32, 64)
    sub = H.from_bits(H.SUBNORMALS)
    pos = [(2 * j + 1, (7 * j + 3) % 64) for j in range(len(sub))]
    for (r, c), v in zip(pos, sub):
        x[r, c] = v
    out = _identity_run(gpu, x)
    want = _want_rounded(x)
    kept = flushed = 0
    for (r, c), v in zip(pos, sub):
        got, w = out[r, c], want[r, c]
        is_rne = H.bits_of(got) == H.bits_of(w)
        is_zero = H.bits_of(got) == 0
        print(f"subnormal {int(H.bits_of(v)):#010x}: device {int(H.bits_of(got)):#010x}, RNE {int(H.bits_of(w)):#010x}")
        assert is_rne or is_zero, (hex(int(H.bits_of(v))), hex(int(H.bits_of(got))))
        if w != 0:
            kept += int(is_rne)
            flushed += int(is_zero)
    print(f"subnormal activations: {kept} rounded to nearest even, {flushed} flushed to zero")
    mask = torch.ones_like(x, dtype=torch.bool)
    for r, c in pos:
        mask[r, c] = False
    assert (H.bits_of(out[mask]) == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# e. the same rounding for both operands of sv_conv_wgrad_bf16
# ---------------------------------------------------------------------------------------------------------------------
def _wgrad(fin, dy, plan, K, bf16, want_used=None):
    from mrcc_amd import nn as svnn

    used = set()
    dW = svnn.conv_wgrad(fin, dy, plan, K, fin.shape[1], dy.shape[1], bf16=bf16, used=used)
    want_used = want_used or ({"sv_conv_wgrad_bf16"} if bf16 else {"sv_conv_wgrad"})
    assert used == want_used, used
    return dW


def _want_products(a, b):
    """dW[c][n] = sum over rows p of bf16(a[p][c]) * bf16(b[p][n]) in float64, every product formed (0 * Inf = NaN)"""
    a, b = H.rne_bf16(a).double(), H.rne_bf16(b).double()
    return (a[:, :, None] * b[:, None, :]).sum(0)


@pytest.mark.parametrize("operand", ["in", "dy"])
def test_wgrad_bf16_rounds_both_operands_to_nearest_even(gpu, operand):
    V = 128
    eye = torch.eye(V)
    table = _rounding_input(V, 64, 2 if operand == "in" else 3)
    for run in ("finite", "inf", "nan"):
        t = table.clone()
        if run == "inf":
            t[5, 7], t[70, 40], t[100, 63] = H.from_bits((H.P_INF, H.N_INF, H.MAX_FINITE))
        elif run == "nan":
            t[9, 50] = float("nan")
        fin, dy = (t, eye) if operand == "in" else (eye, t)
        dW = _wgrad(fin.to(gpu), dy.to(gpu), None, 1, True)[0].cpu()
        got = dW.t() if operand == "in" else dW  # [row of the table][its column]
        if run == "finite":
            _bits(got, _want_rounded(t), f"{operand} finite")
            continue
        want = _want_products(fin, dy).float()
        want = want.t() if operand == "in" else want
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan), (operand, run)
        assert nan.any() and torch.isinf(want).sum() == (3 if run == "inf" else 0)
        _bits(torch.where(nan, torch.zeros_like(got), got), _want_rounded(torch.where(nan, torch.zeros_like(want), want)),
              f"{operand} {run}")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_wgrad_absent_pair_is_zero_against_inf(gpu, bf16):
    """an output row with an Inf in dy: the offsets at which it has no neighbour get exactly the sum without it"""
    cm = _one(gpu)
    plan, nbr, V, _, K = _map(cm, "k3")
    present = nbr[:, :V] >= 0
    n_present = present.sum(0)
    row = int(torch.nonzero((n_present > 1) & (n_present < 27))[0])
    fin = _ints(gpu, (V, 64), 1, 4, 1)  # no zeros: every product with the Inf is an Inf
    dy = _ints(gpu, (V, 64), -3, 3, 2)
    dy0 = dy.clone()
    dy0[row, 5] = 0.0
    dy[row, 5] = float("inf")
    want = H.ref_wgrad(fin, dy0, nbr, V)
    dW = _wgrad(fin, dy, plan, K, bf16)
    lacks = ~present[:, row]
    assert lacks.any() and not lacks[13]
    _exact(dW[lacks], want[lacks])
    has = torch.nonzero(~lacks).flatten()
    assert torch.isinf(dW[has][:, :, 5]).all()
    keep = torch.ones(64, dtype=torch.bool, device=gpu)
    keep[5] = False
    _exact(dW[has][:, :, keep], want[has][:, :, keep])


# ---------------------------------------------------------------------------------------------------------------------
# f. sv_conv_wgrad and sv_conv_wgrad_bf16 exact on every element
# ---------------------------------------------------------------------------------------------------------------------
FP32_SHAPES = [(7, 5), (130, 200), (66, 4), (3, 32), (64, 64)]
BF16_SHAPES = [(16, 16), (144, 80), (64, 96), (128, 128), (160, 384)]
WGRAD_MAPS = ["k3 one frame", "k3 two frames", "down", "up", "scatter", "split", "dense"]


def _wgrad_maps(gpu, which):
    """[(plan, nbr, V_in, V_out, K)] of a map case"""
    if which == "k3 one frame":
        return [_map(_one(gpu), "k3")]
    if which == "k3 two frames":
        return [_map(_two(gpu), "k3")]
    if which in ("down", "up"):
        return [_map(_two(gpu), which)]
    if which == "scatter":
        cm = _scatter(gpu)
        plan, nbr, V, _, K = _map(cm, "k3")
        live = torch.tensor([[bin(int(v)).count("1") for v in row] for row in (plan.submask.view(-1, 27) & 0xFF).cpu()])
        off_centre = [k for k in range(27) if k != 13]
        assert int(live[:, off_centre].sum()) < 0.5 * 8 * live.shape[0] * 26, "not sparse enough to skip most sub-tiles"
        assert bool((live.sum(0) % 2 == 1).any()), "no offset with an odd number of live sub-tiles (a lone last one)"
        return [(plan, nbr, V, V, K)]
    if which == "split":
        cm = _one(gpu)
        plan, nbr, V, _, K = _map(cm, "k3")
        return [(cm.plan_k3_split(1, (9, 18)), nbr, V, V, K)]
    return [_map(_one(gpu), "dense", V) for V in (1, 17, 128, 129, 1037)]


def _wgrad_exact(gpu, plan, nbr, V_in, V_out, K, cin, cout, bf16, seed):
    fin = _ints(gpu, (V_in, cin), -4, 4, seed, zero_rows=0.1)
    dy = _ints(gpu, (V_out, cout), -3, 3, seed + 1, zero_rows=0.1)
    H.assert_exact_range(fin, dy, nbr, V_out)
    _exact(_wgrad(fin, dy, plan, K, bf16), H.ref_wgrad(fin, dy, nbr, V_out))


@pytest.mark.parametrize("which", WGRAD_MAPS)
def test_wgrad_fp32_every_map_and_odd_shape_exact(gpu, which):
    for plan, nbr, V_in, V_out, K in _wgrad_maps(gpu, which):
        for cin, cout in FP32_SHAPES:
            _wgrad_exact(gpu, plan, nbr, V_in, V_out, K, cin, cout, False, seed=cin * cout + V_out)


@pytest.mark.parametrize("which", WGRAD_MAPS)
def test_wgrad_bf16_every_map_and_shape_exact(gpu, which):
    for plan, nbr, V_in, V_out, K in _wgrad_maps(gpu, which):
        for cin, cout in BF16_SHAPES:
            _wgrad_exact(gpu, plan, nbr, V_in, V_out, K, cin, cout, True, seed=cin * cout + V_out)


@pytest.mark.parametrize("which", ["k3 one frame", "down", "dense"])
def test_wgrad_fp32_misaligned_bases_exact(gpu, which):
    """64 channels read from buf[:, 1:65] of a 68-wide buffer: Cin % 4 == 0 and the row stride % 4 == 0, but the base is
    4 bytes past a 16-byte boundary, so the float4 loads are off (vec_a / vec_b false) - for in, for dy, for both"""
    plan, nbr, V_in, V_out, K = _wgrad_maps(gpu, which)[-1]
    abuf = _ints(gpu, (V_in, 68), -4, 4, 21, zero_rows=0.1)
    bbuf = _ints(gpu, (V_out, 68), -3, 3, 22, zero_rows=0.1)
    a_mis, b_mis = abuf[:, 1:65], bbuf[:, 1:65]
    assert a_mis.data_ptr() % 16 == 4 and b_mis.data_ptr() % 16 == 4 and a_mis.stride(0) == 68
    a_al, b_al = a_mis.contiguous(), b_mis.contiguous()
    assert a_al.data_ptr() % 16 == 0 and b_al.data_ptr() % 16 == 0
    H.assert_exact_range(a_al, b_al, nbr, V_out)
    want = H.ref_wgrad(a_al, b_al, nbr, V_out)
    for fin, dy in ((a_mis, b_al), (a_al, b_mis), (a_mis, b_mis)):
        _exact(_wgrad(fin, dy, plan, K, False), want)


@pytest.mark.parametrize("which", ["k3 one frame", "up", "dense"])
def test_wgrad_bf16_strided_input_and_misaligned_fallback_exact(gpu, which):
    plan, nbr, V_in, V_out, K = _wgrad_maps(gpu, which)[-1]
    abuf = _ints(gpu, (V_in, 72), -4, 4, 31, zero_rows=0.1)
    dy = _ints(gpu, (V_out, 96), -3, 3, 32)
    strided = abuf[:, 4:68]  # aligned column slice: the bf16 kernel takes it
    assert strided.data_ptr() % 16 == 0 and strided.stride(0) == 72
    H.assert_exact_range(strided, dy, nbr, V_out)
    _exact(_wgrad(strided, dy, plan, K, True), H.ref_wgrad(strided, dy, nbr, V_out))
    mis = abuf[:, 1:65]  # misaligned: sv_conv_wgrad_bf16 refuses it, the fp32 kernel runs and is exact as well
    assert mis.data_ptr() % 16 == 4
    _exact(_wgrad(mis, dy, plan, K, True, want_used={"sv_conv_wgrad"}), H.ref_wgrad(mis, dy, nbr, V_out))
    dbuf = _ints(gpu, (V_out, 100), -3, 3, 33)
    dmis = dbuf[:, 3:99]
    _exact(_wgrad(strided, dmis, plan, K, True, want_used={"sv_conv_wgrad"}), H.ref_wgrad(strided, dmis, nbr, V_out))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_wgrad_accumulate_onto_integers_exact(gpu, bf16):
    from mrcc_amd import nn as svnn

    fn = "sv_conv_wgrad_bf16" if bf16 else "sv_conv_wgrad"
    for plan, nbr, V_in, V_out, K in (_map(_two(gpu), "k3"), _map(_two(gpu), "down"), _map(_one(gpu), "dense", 129)):
        cin, cout = (144, 80) if bf16 else (66, 20)
        fin = _ints(gpu, (V_in, cin), -4, 4, 41)
        dy = _ints(gpu, (V_out, cout), -3, 3, 42)
        H.assert_exact_range(fin, dy, nbr, V_out)
        dW = _ints(gpu, (K, cin, cout), -1000, 1000, 43)
        want = H.ref_wgrad(fin, dy, nbr, V_out) + dW.long()
        assert svnn._wgrad_one(fin, dy, plan, K, cin, cout, V_out, dW, True, bf16=bf16) == fn
        _exact(dW, want)
        assert svnn._wgrad_one(fin, dy, plan, K, cin, cout, V_out, dW, False, bf16=bf16) == fn  # overwrite ignores dW
        _exact(dW, want - _ints(gpu, (K, cin, cout), -1000, 1000, 43).long())


# ---------------------------------------------------------------------------------------------------------------------
# g. batch ranges (ConvPlan.chunks) for everything but the fp32 forward
# ---------------------------------------------------------------------------------------------------------------------
FRAME_SIZES = (600, 100, 0, 840, 300, 520, 180)  # seven batch indices, one empty, not a power of two
LAYOUTS = {"empty in the middle": FRAME_SIZES, "batch index 0 empty": (0, 600, 100, 840, 300, 520, 180)}
LIMIT = 0x7fff0000 - 4096


def _batch(gpu, layout):
    cm = _frame(gpu, "batch " + layout, [H.int_cloud(50 + b, n) if n else np.zeros((0, 3), np.int64)
                                         for b, n in enumerate(LAYOUTS[layout])])
    assert len(cm.batch_bounds(1)) == 8 and len(cm.batch_bounds(2)) == 8
    return cm


def _frames_per_range(cm, plan, in_row_bytes, out_row_bytes, limit):
    """the number of batch indices per range ConvPlan.chunks must choose (None: the whole map fits): the largest power
    of two whose every range fits the limit on both sides - re-derived here from the documented rule"""
    bi, bo = cm.batch_bounds(plan.in_stride), cm.batch_bounds(plan.out_stride)
    B = len(bi) - 1
    if bi[B] * in_row_bytes < limit and bo[B] * out_row_bytes < limit:
        return None
    for f in (4, 2, 1):
        if all((bi[min(c + f, B)] - bi[c]) * in_row_bytes < limit and (bo[min(c + f, B)] - bo[c]) * out_row_bytes < limit
               for c in range(0, B, f)):
            return f
    raise AssertionError("a single frame beyond the limit")


class _Ranges:
    """lowers sparse.BUF_LIMIT so that the batch splits into ranges of one, two and four batch indices (or the next
    larger count that still fits: chunks() takes the largest); entries: [(ConvPlan, in row bytes, out row bytes)] as the
    code under test will ask.  After each step it checks that every entry really split, into the ranges the rule gives."""

    def __init__(self, monkeypatch, cm, entries):
        self.mp, self.cm, self.entries = monkeypatch, cm, entries
        self.seen = set()

    def _clear(self):
        for p, _, _ in self.entries:
            p._chunked.clear()

    def limits(self):
        from mrcc_amd import sparse

        for f in (1, 2, 4):  # the smallest limit that ranges of f batch indices fit, on every entry
            need = 0
            for p, ib, ob in self.entries:
                bi, bo = self.cm.batch_bounds(p.in_stride), self.cm.batch_bounds(p.out_stride)
                B = len(bi) - 1
                need = max(need, max(max((bi[min(c + f, B)] - bi[c]) * ib, (bo[min(c + f, B)] - bo[c]) * ob)
                                     for c in range(0, B, f)))
            self.mp.setattr(sparse, "BUF_LIMIT", need + 1)
            self._clear()
            yield f
            for p, ib, ob in self.entries:
                bo = self.cm.batch_bounds(p.out_stride)
                B = len(bo) - 1
                parts = p.chunks(ib, ob)
                assert parts is not None, f
                per = _frames_per_range(self.cm, p, ib, ob, need + 1)
                assert per is not None and per >= f
                assert len(parts) == sum(1 for c in range(0, B, per) if bo[min(c + per, B)] > bo[c])
                assert sum(o1 - o0 for _, _, _, o0, o1 in parts) == p.V_out
                assert [(o0, o1) for _, _, _, o0, o1 in parts] == [(bo[c], bo[min(c + per, B)]) for c in range(0, B, per)
                                                                  if bo[min(c + per, B)] > bo[c]]
                self.seen.add(per)
        self.mp.setattr(sparse, "BUF_LIMIT", LIMIT)
        self._clear()


def _range_plans(cm, kind):
    """(plan to launch, the ConvPlans that chunk, nbr, V_in, V_out, K)"""
    if kind == "split":
        plan, nbr, V_in, V_out, K = _map(cm, "k3")
        sp = cm.plan_k3_split(1, (9, 18))
        return sp, [sub for _, _, sub in sp.parts], nbr, V_in, V_out, K
    plan, nbr, V_in, V_out, K = _map(cm, kind)
    return plan, [plan], nbr, V_in, V_out, K


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_batch_ranges_bf16_forward_exact(gpu, monkeypatch, layout):
    from mrcc_amd import nn as svnn

    cm = _batch(gpu, layout)
    cin, cout = 64, 96
    seen = set()
    for kind in ("k3", "down", "up", "split"):
        plan, chunked, nbr, V_in, V_out, K = _range_plans(cm, kind)
        x = _ints(gpu, (V_in, cin), -4, 4, 1, zero_rows=0.1)
        W = _ints(gpu, (K, cin, cout), -3, 3, 2)
        scale, shift = H.scale_tensor(cout, 3).to(gpu), _ints(gpu, (cout,), -8, 8, 4)
        res = _ints(gpu, (V_out, cout), -8, 8, 5)
        H.assert_exact_range(x, W, nbr, V_out)
        want = H.ref_forward(x, W, nbr, V_out)
        want_epi = H.ref_epilogue(want, scale, shift, res, ACT_RELU)
        wp = svnn.pack_weights_bf16(W)
        assert all(p.chunks(4 * cin, 4 * cout) is None for p in chunked)
        whole_raw = svnn.conv_forward(x, W, plan, V_out, weight_bf16=wp)
        whole_epi = svnn.conv_forward(x, W, plan, V_out, scale, shift, res, ACT_RELU, weight_bf16=wp)
        _exact(whole_raw, want)
        _bits(whole_epi, want_epi, kind)
        r = _Ranges(monkeypatch, cm, [(p, 4 * cin, 4 * cout) for p in chunked])
        for f in r.limits():
            raw = svnn.conv_forward(x, W, plan, V_out, weight_bf16=wp)
            _exact(raw, want)
            assert torch.equal(raw, whole_raw), (kind, f)
            epi = svnn.conv_forward(x, W, plan, V_out, scale, shift, res, ACT_RELU, weight_bf16=wp)
            _bits(epi, whole_epi, f"{kind} ranges of {f}")
        seen |= r.seen
    # ranges of two and of four batch indices on both layouts; of one where no empty index pairs with the largest frame
    assert {2, 4} <= seen and (1 in seen or layout != "batch index 0 empty"), seen


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_batch_ranges_wgrad_exact(gpu, monkeypatch, layout, bf16):
    cm = _batch(gpu, layout)
    cin, cout = 64, 96
    seen = set()
    for kind in ("k3", "down", "up", "split"):
        plan, chunked, nbr, V_in, V_out, K = _range_plans(cm, kind)
        fin = _ints(gpu, (V_in, cin), -4, 4, 11, zero_rows=0.1)
        dy = _ints(gpu, (V_out, cout), -3, 3, 12, zero_rows=0.1)
        H.assert_exact_range(fin, dy, nbr, V_out)
        want = H.ref_wgrad(fin, dy, nbr, V_out)
        assert all(p.chunks(4 * cin, 4 * cout) is None for p in chunked)
        whole = _wgrad(fin, dy, plan, K, bf16)
        _exact(whole, want)
        r = _Ranges(monkeypatch, cm, [(p, 4 * cin, 4 * cout) for p in chunked])
        for f in r.limits():
            got = _wgrad(fin, dy, plan, K, bf16)
            _exact(got, want)
            assert torch.equal(got, whole), (kind, f)
        seen |= r.seen
    # ranges of two and of four batch indices on both layouts; of one where no empty index pairs with the largest frame
    assert {2, 4} <= seen and (1 in seen or layout != "batch index 0 empty"), seen


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_batch_ranges_full_backward_exact(gpu, monkeypatch, layout, precision):
    """SparseConvFunction forward + backward over ranges: out, dX (a forward launch of dY on the mirrored weights) and
    dW, fp32 and on the bf16 training kernels"""
    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd import nn as svnn
    from mrcc_amd import profiling
    from mrcc_amd.sparse import SparseTensor

    cm = _batch(gpu, layout)
    cin, cout = 128, 64  # dX runs on sv_conv_fwd_bf16 where Cin % 128 == 0
    seen = set()
    for kind in ("k3", "down"):
        plan, chunked, nbr, V_in, V_out, K = _range_plans(cm, kind)
        grad_plan = plan if kind == "k3" else cm.plan_up(2)
        layer = ME.MinkowskiConvolution(cin, cout, kernel_size=3 if kind == "k3" else 2, stride=1 if kind == "k3" else 2,
                                        dimension=3).to(gpu).train()
        svnn.set_training_precision(layer, precision)
        W = _ints(gpu, (K, cin, cout), -3, 3, 21)
        with torch.no_grad():
            layer.kernel.copy_(W)
        fin = _ints(gpu, (V_in, cin), -4, 4, 22, zero_rows=0.1)
        dy = _ints(gpu, (V_out, cout), -3, 3, 23, zero_rows=0.1)
        H.assert_exact_range(fin, W, nbr, V_out)
        H.assert_exact_range(fin, dy, nbr, V_out)
        assert int(H.ref_dgrad(dy.abs(), W.abs(), nbr, V_in, V_out).max()) < H.EXACT_LIMIT  # dX's sums of absolute terms
        want = (H.ref_forward(fin, W, nbr, V_out), H.ref_dgrad(dy, W, nbr, V_in, V_out), H.ref_wgrad(fin, dy, nbr, V_out))

        def run():
            layer.kernel.grad = None
            leaf = fin.clone().requires_grad_(True)
            x = SparseTensor(leaf, coordinate_manager=cm, tensor_stride=1)
            profiling.TRAIN_LOG = []
            try:
                out = layer.forward_fused(x)
                out.F.backward(dy)
                log = {op: fn for _, op, fn in profiling.TRAIN_LOG}
            finally:
                profiling.TRAIN_LOG = None
            return (out.F.detach(), leaf.grad, layer.kernel.grad.clone()), log

        whole, log = run()
        if precision == "bf16":
            assert log == {"fwd": "sv_conv_fwd_bf16", "dx": "sv_conv_fwd_bf16", "dw": "sv_conv_wgrad_bf16"}, log
        else:
            assert log == {"fwd": "sv_conv_fwd_acc", "dx": "sv_conv_fwd_acc", "dw": "sv_conv_wgrad"}, log
        for g, w in zip(whole, want):
            _exact(g, w)
        # the forward and dW ask the forward plan (feature rows in, dY rows out), dX the gradient plan (dY rows in)
        r = _Ranges(monkeypatch, cm, [(plan, 4 * cin, 4 * cout), (grad_plan, 4 * cout, 4 * cin)])
        for f in r.limits():
            got, log2 = run()
            assert log2 == log
            for g, w, wh in zip(got, want, whole):
                _exact(g, w)
                assert torch.equal(g, wh), (kind, f)
        seen |= r.seen
    assert {2, 4} <= seen and (1 in seen or layout != "batch index 0 empty"), seen
