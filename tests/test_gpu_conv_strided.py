"""The convolution kernels on the strided, kernel_size-1-with-a-plan, transposed and dilated kernel maps of the classification
ResNets (plan_strided / plan_strided_t / plan_k3 with a dilation), kernel by kernel.

These maps have what no earlier map had: OUTPUT ROWS WITHOUT ANY NEIGHBOUR.  On the transposed kernel_size 1 stride 2 map and on
the transposed dilation-2 stride-2 map only the voxels whose coordinates are all even have one, so about 7 rows of 8 are empty;
the plan sorts rows by mask, so they fill whole 128-row plan tiles whose submask words are all zero - with real rows
(perm >= 0) that must still receive act(scale * 0 + shift + residual) in an output nobody cleared.  And K = 1 comes with
perm / nbr_s / submask, the input gradient runs W[k]^T without the offset mirror, and batch ranges rebase rows between maps of
different strides.

Maps are compact blobs of integer coordinates (strided_helpers.FRAMES), the neighbour tables of every reference come from
strided_helpers.probe_ref (numpy), and each plan's raw table is held to it before anything runs on the plan.
 (a) fp32 forward: every row of strided_helpers.STRIDED_CASES bit-exact against oracle.conv, instance name and form asserted;
 (b) the special kernels at row edges V = 1 .. 129 of an empty-tile map;
 (c) is in tests/test_gpu_conv_exact.py (bf16 forward, every instance on the new kinds);
 (d) sv_conv_wgrad / sv_conv_wgrad_bf16 exact on the forward maps, 0 x inf included;
 (e) is in tests/test_gpu_conv_grad.py (layer gradients through the modules);
 (f) the bf16 training path of a strided k3 and a strided k1 layer, exact;
 (g) batch ranges (ConvPlan.chunks) between maps of different strides.
"""
import contextlib

import numpy as np
import pytest
import torch

import conv_exact_helpers as X
import conv_instance_helpers as H
import strided_helpers as S

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
ACT_RELU = 1
LIMIT = 0x7fff0000 - 4096
# rows that share a map and a shape are neighbours, so that the one-entry operand / oracle cache serves them
ROWS = sorted(S.STRIDED_CASES, key=lambda c: (c.frame, c.kind, c.Cin, c.Cout, S.strided_case_id(c)))

_managers, _plans = {}, {}


def _manager(gpu, coords4):
    from mrcc_amd import MinkowskiEngine as ME

    st = ME.SparseTensor(torch.zeros(len(coords4), 1), coordinates=torch.from_numpy(coords4).int(), device=gpu)
    return st.coordinate_manager


def _cm(gpu, frame):
    if frame not in _managers:
        _managers[frame] = _manager(gpu, S.frame_input(frame))
        assert _managers[frame].stride_map(1).V == len(S.frame_coords(frame))
    return _managers[frame]


def _check_raw(plan, nbr, V_in, V_out):
    """the plan's unsorted kernel map IS the numpy table (so a reference built from the table speaks about this plan)"""
    raw, ld, mask = plan.raw
    assert plan.V_out == V_out and plan.K == nbr.shape[0] and plan.Vpad == (V_out + 127) // 128 * 128
    assert np.array_equal(raw[:, :V_out].cpu().numpy(), nbr)
    assert np.array_equal(mask[:V_out].cpu().numpy(), S.mask_of(nbr))
    assert plan.cm().stride_map(plan.in_stride).V == V_in


def _plan(gpu, frame, kind):
    """(plan, nbr table, V_in, V_out) of a kind on a named frame; the raw table checked against probe_ref on first use"""
    if (frame, kind) not in _plans:
        nbr, V_in, V_out = S.kind_table(frame, kind)
        plan = S.kind_plan(_cm(gpu, frame), kind)
        _check_raw(plan, nbr, V_in, V_out)
        _plans[(frame, kind)] = (plan, nbr, V_in, V_out)
    return _plans[(frame, kind)]


def _misaligned_perm(plan):
    """a copy of the plan whose `perm` starts 4 bytes off a 16-byte boundary"""
    from mrcc_amd.sparse import ConvPlan

    buf = torch.empty(plan.Vpad + 1, dtype=torch.int32, device=plan.perm.device)
    buf[1:] = plan.perm
    perm = buf[1:1 + plan.Vpad]
    assert perm.data_ptr() % 16 == 4
    return ConvPlan(perm, plan.nbr_s, plan.submask, plan.tile_order, plan.V_out, plan.Vpad, plan.K)


# ---------------------------------------------------------------------------------------------------------------------
# the maps: what the tests below rely on, asserted on the plans themselves
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", ["one", "two"])
def test_plans_match_probe_ref_and_the_empty_tile_maps_have_all_empty_and_mixed_tiles(gpu, frame):
    for kind in S.MAP_KINDS:
        plan, nbr, V_in, V_out = _plan(gpu, frame, kind)
        if kind in ("k3s2", "k3s3"):
            assert V_out < V_in
        if kind.endswith("_t"):
            assert V_out > V_in
    for kind in S.EMPTY_TILE_KINDS:
        plan, nbr, V_in, V_out = _plan(gpu, frame, kind)
        empty_rows = int((nbr < 0).all(0).sum())
        all_empty, mixed = S.plan_tile_census(plan)
        print(f"{frame} {kind}: {empty_rows} of {V_out} rows without a neighbour, {int(all_empty.sum())} of {len(all_empty)} "
              f"plan tiles all-empty, {int(mixed.sum())} with live and empty sub-tiles")
        assert 2 * empty_rows >= V_out
        assert all_empty.any(), "no 128-row tile of real rows whose submask words are all zero"
        assert mixed.any(), "no tile that mixes live and empty 16-row sub-tiles"


# ---------------------------------------------------------------------------------------------------------------------
# a. fp32 forward: every row bit-exact against the oracle, on the instance and in the form the row names
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shapes(oracle):
    """(map key, nbr, V_in, V_out, Cin, Cout) -> host operands and the oracle's result; the last shape is kept"""
    last = {}

    def get(key, nbr, V_in, V_out, Cin, Cout):
        key = (key, Cin, Cout)
        if last.get("key") != key:
            last.clear()
            K = nbr.shape[0]
            rng = np.random.default_rng([K, Cin, Cout, V_out])
            # column slices of wider buffers: 16-byte aligned start and row stride wherever Cin allows float4 gathers
            in_off, in_ld = (4, Cin + 8) if Cin % 4 == 0 else (1, Cin + 2)
            xbuf = rng.standard_normal((V_in, in_ld), dtype=np.float32)
            W = rng.standard_normal((K, Cin, Cout), dtype=np.float32) * np.float32(0.1)
            scale = rng.uniform(0.5, 1.5, size=Cout).astype(np.float32)
            shift = rng.standard_normal(Cout, dtype=np.float32)
            resbuf = rng.standard_normal((V_out, Cout + 4), dtype=np.float32)
            x = np.ascontiguousarray(xbuf[:, in_off:in_off + Cin])
            res = np.ascontiguousarray(resbuf[:, :Cout])
            want = oracle.conv(x, W, nbr, V_out, scale, shift, res, oracle.ACT_RELU)
            # a row without a neighbour is relu(shift + residual): the accumulator is 0 and fma(0, scale, shift) = shift
            empty = (nbr < 0).all(0)
            assert np.array_equal(want[empty], np.maximum(shift[None] + res[empty], np.float32(0)))
            last.update(key=key, xbuf=xbuf, in_off=in_off, W=W, scale=scale, shift=shift, resbuf=resbuf, want=want)
        return last

    return get


def _run(gpu, ops, plan, Cin, Cout, V, scale=None):
    """(result, name, flags, the output buffer's other columns untouched) of one public call"""
    import mrcc_amd
    from mrcc_amd import nn as svnn

    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    x = t(ops["xbuf"])[:, ops["in_off"]:ops["in_off"] + Cin]
    res = t(ops["resbuf"])[:, :Cout]
    out_ld = (Cout + 3) // 4 * 4 + 8
    out_buf = torch.full((V, out_ld), SENTINEL, device=gpu)
    out = out_buf[:, 4:4 + Cout]  # 16-byte aligned start, row stride a multiple of four floats
    with (mrcc_amd._lib.conv_dispatch(scale) if scale is not None else contextlib.nullcontext()):
        svnn.conv_forward(x, t(ops["W"]), plan, V, t(ops["scale"]), t(ops["shift"]), res, 1, out=out)
        name, flags = mrcc_amd._lib.conv_last_instance()
    got = out.cpu().numpy()
    untouched = bool((out_buf[:, :4] == SENTINEL).all()) and bool((out_buf[:, 4 + Cout:] == SENTINEL).all())
    return got, name, flags, untouched


def _compare(got, want, nbr, what=""):
    if not np.array_equal(got, want):
        bad = (got != want).any(1)
        empty = (nbr < 0).all(0)
        raise AssertionError(f"{what}{int((got != want).sum())} of {want.size} elements differ in {int(bad.sum())} rows "
                             f"({int((bad & empty).sum())} of them rows without a neighbour), max abs diff "
                             f"{np.abs(got - want).max()}, {int((got == SENTINEL).sum())} elements still hold the sentinel")


@pytest.mark.parametrize("case", ROWS, ids=S.strided_case_id)
def test_strided_forward_instance_and_form_bit_exact(gpu, oracle, shapes, case):
    c = case
    plan, nbr, V_in, V_out = _plan(gpu, c.frame, c.kind)
    ops = shapes((c.frame, c.kind), nbr, V_in, V_out, c.Cin, c.Cout)
    if c.name == S.DUAL:
        # the tail body's plan tiles, the last tail128 of tile_order, include tiles of real rows without any pair
        n128 = plan.Vpad // 128
        tail128 = int(n128 * H.TAIL_DEFAULT)
        all_empty, _ = S.plan_tile_census(plan)
        tail = plan.tile_order.cpu().numpy()[n128 - tail128:]
        print(f"dual row: {int(all_empty.sum())} of {n128} plan tiles all-empty, {int(all_empty[tail].sum())} of the {tail128} "
              f"tail tiles all-empty")
        assert sorted(plan.tile_order.cpu().tolist()) == list(range(n128))
        assert all_empty[tail].any()
    got, name, flags, untouched = _run(gpu, ops, _misaligned_perm(plan) if c.mis else plan, c.Cin, c.Cout, V_out, c.scale)
    assert (name, flags) == (c.name, {"fast": c.fast, "ring": c.ring, "full": c.full})
    assert not name.startswith("linear_narrow")
    _compare(got, ops["want"], nbr)
    assert untouched, "columns beside the output slice were written"


# ---------------------------------------------------------------------------------------------------------------------
# b. row edges of the special kernels on an empty-tile map
# ---------------------------------------------------------------------------------------------------------------------
_edge = {}


def _edge_map(gpu, V):
    if V not in _edge:
        c4 = S.compact_blob(V, origin=(1, 1, 1))
        nbr, V_in, V_out = S.kind_table_of(S.canonical(c4)[0], "k3s2d2_t")
        cm = _manager(gpu, c4)
        plan = S.kind_plan(cm, "k3s2d2_t")
        _check_raw(plan, nbr, V_in, V_out)
        assert V_out == V
        _edge[V] = (plan, nbr, V_in, cm)  # (a plan holds its manager by a weak reference only)
    return _edge[V][:3]


@pytest.mark.parametrize("V", S.EDGE_V)
@pytest.mark.parametrize("spec", S.EDGE_SPECIAL, ids=lambda s: s[0].split("<")[0] + ("-alone" if s[4] else ""))
def test_special_kernels_at_row_edges_of_an_empty_tile_map(gpu, oracle, shapes, spec, V):
    """V = 1: the only row has no neighbour at all (and the kernel no active offset); 15 .. 17: fewer 16-row sub-tiles than a
    workgroup has waves; 127 .. 129: the last plan tile full, one row short, and a second tile of one row - on a map where
    about 7 rows of 8 are empty"""
    name_want, (fast, ring, full), Cin, Cout, scale, misaligned = spec
    plan, nbr, V_in = _edge_map(gpu, V)
    assert (V > 1) or (nbr < 0).all()
    ops = shapes(("edge", V), nbr, V_in, V, Cin, Cout)
    got, name, flags, untouched = _run(gpu, ops, _misaligned_perm(plan) if misaligned else plan, Cin, Cout, V, scale)
    assert (name, flags) == (name_want, {"fast": fast, "ring": ring, "full": full})
    _compare(got, ops["want"], nbr, f"V {V}: ")
    assert untouched, "columns beside the output slice were written"


# ---------------------------------------------------------------------------------------------------------------------
# d. weight gradients, exact integers, on the forward maps (the plan the weight gradient uses)
# ---------------------------------------------------------------------------------------------------------------------
def _ints(gpu, shape, lo, hi, seed, zero_rows=0.0):
    return X.int_tensor(shape, lo, hi, seed, zero_rows).to(gpu)


def _exact(got, want_int, what=""):
    assert got.dtype == torch.float32
    if not torch.equal(got.double(), want_int.double()):
        bad = got.double() != want_int.double()
        first = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {first}: "
                             f"got {got[tuple(first)].item()}, want {want_int[tuple(first)].item()}")


def _wgrad(fin, dy, plan, K, bf16):
    from mrcc_amd import nn as svnn

    used = set()
    dW = svnn.conv_wgrad(fin, dy, plan, K, fin.shape[1], dy.shape[1], bf16=bf16, used=used)
    assert used == ({"sv_conv_wgrad_bf16"} if bf16 else {"sv_conv_wgrad"}), used
    return dW


def _table(gpu, nbr):
    return torch.from_numpy(np.array(nbr)).to(gpu)


WGRAD_KINDS = ("k3s2", "k3s3", "k1s2", "k3s2d2")


@pytest.mark.parametrize("frame", ["one", "two"])
@pytest.mark.parametrize("kind", WGRAD_KINDS)
@pytest.mark.parametrize("cin,cout,bf16", [(3, 20, False), (64, 96, False), (64, 96, True)],
                         ids=["fp32-3x20", "fp32-64x96", "bf16-64x96"])
def test_wgrad_on_strided_maps_exact(gpu, frame, kind, cin, cout, bf16):
    plan, nbr, V_in, V_out = _plan(gpu, frame, kind)
    K, nbr_t = nbr.shape[0], _table(gpu, nbr)
    fin = _ints(gpu, (V_in, cin), -4, 4, cin * cout + V_out, zero_rows=0.1)
    dy = _ints(gpu, (V_out, cout), -3, 3, cin * cout + V_out + 1, zero_rows=0.1)
    X.assert_exact_range(fin, dy, nbr_t, V_out)
    _exact(_wgrad(fin, dy, plan, K, bf16), X.ref_wgrad(fin, dy, nbr_t, V_out), f"{frame} {kind}")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_wgrad_k1s2_input_row_no_output_sees_is_zero_against_inf(gpu, bf16):
    """kernel_size 1 stride 2: an input row with an odd coordinate is read by no output.  It holds Inf; a kernel that formed
    its product with a zero (or with any row's dY) would leave Inf or NaN in dW - dW is exactly the sum without it"""
    plan, nbr, V_in, V_out = _plan(gpu, "one", "k1s2")
    nbr_t = _table(gpu, nbr)
    seen = np.zeros(V_in, bool)
    seen[nbr[nbr >= 0]] = True
    assert seen.any() and 2 * int((~seen).sum()) > V_in
    unseen = torch.from_numpy(np.nonzero(~seen)[0]).to(gpu)
    fin = _ints(gpu, (V_in, 64), 1, 4, 1)
    dy = _ints(gpu, (V_out, 96), -3, 3, 2)
    fin0 = fin.clone()
    fin0[unseen] = 0.0
    fin[unseen] = float("inf")
    fin[unseen[::3], 5] = float("-inf")
    X.assert_exact_range(fin0, dy, nbr_t, V_out)
    dW = _wgrad(fin, dy, plan, 1, bf16)
    assert bool(torch.isfinite(dW).all())
    _exact(dW, X.ref_wgrad(fin0, dy, nbr_t, V_out), "k1s2 against inf")


# ---------------------------------------------------------------------------------------------------------------------
# f. the bf16 training path of a strided layer: fwd and dX on sv_conv_fwd_bf16 (dX: W[k]^T, no mirror), dW on
#    sv_conv_wgrad_bf16 - exact integers
# ---------------------------------------------------------------------------------------------------------------------
def _train_run(layer, cm, fin, dy):
    from mrcc_amd import profiling
    from mrcc_amd.sparse import SparseTensor

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
    g = layer.kernel.grad
    return (out.F.detach(), leaf.grad, (g if g.dim() == 3 else g.unsqueeze(0)).clone()), log


def _int_layer(gpu, cin, cout, ks, stride, precision, seed):
    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd import nn as svnn

    layer = ME.MinkowskiConvolution(cin, cout, kernel_size=ks, stride=stride, dimension=3).to(gpu).train()
    svnn.set_training_precision(layer, precision)
    W = _ints(gpu, (ks ** 3, cin, cout), -3, 3, seed)
    with torch.no_grad():
        layer.kernel.copy_(W if ks > 1 else W[0])
    return layer, W


def _exact_operands(gpu, nbr_t, V_in, V_out, W, seed):
    cin, cout = W.shape[1], W.shape[2]
    fin = _ints(gpu, (V_in, cin), -4, 4, seed, zero_rows=0.1)
    dy = _ints(gpu, (V_out, cout), -3, 3, seed + 1, zero_rows=0.1)
    X.assert_exact_range(fin, W, nbr_t, V_out)
    X.assert_exact_range(fin, dy, nbr_t, V_out)
    assert int(X.ref_dgrad(dy.abs(), W.abs(), nbr_t, V_in, V_out).max()) < X.EXACT_LIMIT  # dX's sums of absolute terms
    want = (X.ref_forward(fin, W, nbr_t, V_out), X.ref_dgrad(dy, W, nbr_t, V_in, V_out), X.ref_wgrad(fin, dy, nbr_t, V_out))
    return fin, dy, want


BF16_LOG = {"fwd": "sv_conv_fwd_bf16", "dx": "sv_conv_fwd_bf16", "dw": "sv_conv_wgrad_bf16"}
FP32_LOG = {"fwd": "sv_conv_fwd_acc", "dx": "sv_conv_fwd_acc", "dw": "sv_conv_wgrad"}


@pytest.mark.parametrize("frame", ["one", "two"])
@pytest.mark.parametrize("kind,cin,cout", [("k3s2", 128, 128), ("k1s2", 128, 256)])
def test_bf16_training_path_of_strided_layers_exact(gpu, frame, kind, cin, cout):
    ks, stride, _, _ = S.MAP_KINDS[kind]
    plan, nbr, V_in, V_out = _plan(gpu, frame, kind)
    _plan(gpu, frame, kind + "_t")  # the input gradient's plan: its raw table checked too
    nbr_t = _table(gpu, nbr)
    layer, W = _int_layer(gpu, cin, cout, ks, stride, "bf16", 21)
    fin, dy, want = _exact_operands(gpu, nbr_t, V_in, V_out, W, 22)
    got, log = _train_run(layer, _cm(gpu, frame), fin, dy)
    assert log == BF16_LOG, log
    for g, w, what in zip(got, want, ("out", "dX", "dW")):
        _exact(g, w, f"{frame} {kind} {what}")
    if kind == "k1s2":  # input rows no output reads: exactly zero
        seen = np.zeros(V_in, bool)
        seen[nbr[nbr >= 0]] = True
        assert bool((got[1][torch.from_numpy(~seen).to(gpu)] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# g. batch ranges (ConvPlan.chunks) where in_stride != out_stride, in either direction
# ---------------------------------------------------------------------------------------------------------------------
def _frames_per_range(bi, bo, in_row_bytes, out_row_bytes, limit):
    """the number of batch indices per range ConvPlan.chunks must choose (None: the whole map fits): the largest power of two
    whose every range fits the limit on both sides - re-derived from the documented rule"""
    B = len(bi) - 1
    if bi[B] * in_row_bytes < limit and bo[B] * out_row_bytes < limit:
        return None
    for f in (2, 1):
        if all((bi[min(c + f, B)] - bi[c]) * in_row_bytes < limit and (bo[min(c + f, B)] - bo[c]) * out_row_bytes < limit
               for c in range(0, B, f)):
            return f
    raise AssertionError("a single frame beyond the limit")


def _batch_ranges(monkeypatch, plans, bounds):
    """lowers sparse.BUF_LIMIT so that the four-frame batch splits into ranges of one and of two batch indices; plans:
    [(ConvPlan, in row bytes, out row bytes)] as the code under test will ask, bounds: stride -> the numpy batch bounds.  Yields
    the frames per range; after each step it checks that every plan split into exactly the ranges the bounds give."""
    from mrcc_amd import sparse

    def clear():
        for p, _, _ in plans:
            p._chunked.clear()

    for f in (1, 2):
        need = 0
        for p, ib, ob in plans:
            bi, bo = bounds[p.in_stride], bounds[p.out_stride]
            need = max(need, max(max((bi[min(c + f, 4)] - bi[c]) * ib, (bo[min(c + f, 4)] - bo[c]) * ob) for c in range(0, 4, f)))
        monkeypatch.setattr(sparse, "BUF_LIMIT", need + 1)
        clear()
        yield f
        for p, ib, ob in plans:
            bi, bo = bounds[p.in_stride], bounds[p.out_stride]
            assert _frames_per_range(bi, bo, ib, ob, need + 1) == f
            parts = p.chunks(ib, ob)
            assert parts is not None
            assert [(i0, i1, o0, o1) for _, i0, i1, o0, o1 in parts] == \
                [(bi[c], bi[min(c + f, 4)], bo[c], bo[min(c + f, 4)]) for c in range(0, 4, f) if bo[min(c + f, 4)] > bo[c]]
            assert len(parts) == (3 if f == 1 else 2), "one of the four batch indices is empty"
            assert all(sub.V_out == o1 - o0 for sub, _, _, o0, o1 in parts)
    monkeypatch.setattr(sparse, "BUF_LIMIT", LIMIT)
    clear()


def _batch(gpu, kind):
    """(cm, plan, nbr, V_in, V_out, numpy batch bounds by stride) of a kind on the four-frame batch"""
    cm = _cm(gpu, "batch")
    plan, nbr, V_in, V_out = _plan(gpu, "batch", kind)
    c1 = S.frame_coords("batch")
    bounds = {1: S.batch_bounds_ref(c1, 4), 2: S.batch_bounds_ref(S.stride_map_ref(c1, 2)[0], 4)}
    assert bounds[1][1] == bounds[1][2] and bounds[2][1] == bounds[2][2], "batch index 1 is empty"
    assert {plan.in_stride, plan.out_stride} == {1, 2}
    for s in (1, 2):
        assert cm.batch_bounds(s) == bounds[s]
    assert bounds[plan.in_stride][4] == V_in and bounds[plan.out_stride][4] == V_out
    return cm, plan, nbr, V_in, V_out, bounds


@pytest.mark.parametrize("kind", ["k3s2", "k1s2_t"])
def test_batch_ranges_forward_between_strides_same_bits(gpu, monkeypatch, kind):
    from mrcc_amd import nn as svnn

    cm, plan, nbr, V_in, V_out, bounds = _batch(gpu, kind)
    K, cin, cout, nbr_t = nbr.shape[0], 64, 128, _table(gpu, nbr)
    x = _ints(gpu, (V_in, cin), -4, 4, 1, zero_rows=0.1)
    W = _ints(gpu, (K, cin, cout), -3, 3, 2)
    scale, shift = X.scale_tensor(cout, 3).to(gpu), _ints(gpu, (cout,), -8, 8, 4)
    res = _ints(gpu, (V_out, cout), -8, 8, 5)
    X.assert_exact_range(x, W, nbr_t, V_out)
    want = X.ref_forward(x, W, nbr_t, V_out)
    want_epi = X.ref_epilogue(want, scale, shift, res, ACT_RELU)
    wp = svnn.pack_weights_bf16(W)
    assert plan.chunks(4 * cin, 4 * cout) is None

    def run():
        outs = []
        for kw in ({}, {"weight_bf16": wp}):
            raw = torch.full((V_out, cout), SENTINEL, device=gpu)
            epi = torch.full((V_out, cout), SENTINEL, device=gpu)
            svnn.conv_forward(x, W, plan, V_out, out=raw, **kw)
            svnn.conv_forward(x, W, plan, V_out, scale, shift, res, ACT_RELU, out=epi, **kw)
            outs += [raw, epi]
        return outs

    whole = run()
    for j, g in enumerate(whole):
        _exact(g, want if j % 2 == 0 else want_epi.double(), f"{kind} whole {j}")
    for f in _batch_ranges(monkeypatch, [(plan, 4 * cin, 4 * cout)], bounds):
        for j, (g, w) in enumerate(zip(run(), whole)):
            assert X.same_bits(g, w), (kind, f, ("fp32 raw", "fp32 epilogue", "bf16 raw", "bf16 epilogue")[j],
                                       int((g != w).sum()))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["k3s2", "k1s2_t"])
def test_batch_ranges_wgrad_between_strides_exact(gpu, monkeypatch, kind, bf16):
    cm, plan, nbr, V_in, V_out, bounds = _batch(gpu, kind)
    K, cin, cout, nbr_t = nbr.shape[0], 64, 96, _table(gpu, nbr)
    fin = _ints(gpu, (V_in, cin), -4, 4, 11, zero_rows=0.1)
    dy = _ints(gpu, (V_out, cout), -3, 3, 12, zero_rows=0.1)
    X.assert_exact_range(fin, dy, nbr_t, V_out)
    want = X.ref_wgrad(fin, dy, nbr_t, V_out)
    whole = _wgrad(fin, dy, plan, K, bf16)
    _exact(whole, want, kind)
    for f in _batch_ranges(monkeypatch, [(plan, 4 * cin, 4 * cout)], bounds):
        got = _wgrad(fin, dy, plan, K, bf16)
        _exact(got, want, f"{kind} ranges of {f}")
        assert torch.equal(got, whole), (kind, f)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,cin,cout", [("k3s2", 128, 64), ("k1s2", 128, 64)])
def test_batch_ranges_strided_layer_backward_exact(gpu, monkeypatch, kind, cin, cout, precision):
    """the whole layer over ranges: the forward and dW ask the forward plan (stride 1 rows in, stride 2 rows out), dX the
    transposed plan (stride 2 rows in, stride 1 rows out; on sv_conv_fwd_bf16 with W[k]^T packed, Cin % 128 == 0)"""
    ks, stride, _, _ = S.MAP_KINDS[kind]
    cm, plan, nbr, V_in, V_out, bounds = _batch(gpu, kind)
    grad_plan = _batch(gpu, kind + "_t")[1]
    nbr_t = _table(gpu, nbr)
    layer, W = _int_layer(gpu, cin, cout, ks, stride, precision, 31)
    fin, dy, want = _exact_operands(gpu, nbr_t, V_in, V_out, W, 32)
    whole, log = _train_run(layer, cm, fin, dy)
    assert log == (BF16_LOG if precision == "bf16" else FP32_LOG), log
    for g, w, what in zip(whole, want, ("out", "dX", "dW")):
        _exact(g, w, f"{kind} {what}")
    for f in _batch_ranges(monkeypatch, [(plan, 4 * cin, 4 * cout), (grad_plan, 4 * cout, 4 * cin)], bounds):
        got, log2 = _train_run(layer, cm, fin, dy)
        assert log2 == log
        for g, w, wh, what in zip(got, want, whole, ("out", "dX", "dW")):
            _exact(g, w, f"{kind} {what} ranges of {f}")
            assert torch.equal(g, wh), (kind, what, f)
