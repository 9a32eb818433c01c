"""The small post-conv kernels against torch on the CPU, at the shapes and values where they go wrong.

sv_batch_offsets, sv_global_pool, sv_slice_rows, sv_slice_argmax (csrc/sv_post.hip), sv_voxel_reduce (csrc/sv_coords.hip)
and sv_key_point_predictions[_batched] turn conv output into what the reference returns.  The C oracle states the same
semantics as the kernels, so it cannot show where both differ from torch; every expectation here is torch's own
formulation on the CPU (float64 where the value is numeric): NaN, +-inf, ties, empty batches, channel counts off the
64-lane slabs, both key-point template instances and strided (ld > C) views."""
import math
from ctypes import c_float, c_int, c_int64, c_size_t

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # float32 unit roundoff
SENTINEL = 3.0e38  # fills the columns around a strided view: a kernel that reads them shows it in any max or mean


def _lib():
    from mrcc_amd import _lib

    return _lib


def _device_view(x, gpu, pad):
    """x (CPU float32 [N, C]) on the device; with pad > 0 as the columns 1 .. C of a [N, C + pad] buffer (ld > C)"""
    if pad == 0:
        return x.to(gpu).contiguous()
    buf = torch.full((x.shape[0], x.shape[1] + pad), SENTINEL, device=gpu)
    buf[:, 1:1 + x.shape[1]] = x.to(gpu)
    return buf[:, 1:1 + x.shape[1]]


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------
# sv_batch_offsets
# ---------------------------------------------------------------------------------------------------------------------
def _keys_of(counts, oracle, rng):
    batch = np.repeat(np.arange(len(counts)), counts)
    xyz = rng.integers(-5000, 5000, size=(len(batch), 3))
    return np.sort(oracle.make_keys(np.concatenate([batch[:, None], xyz], axis=1)))


@pytest.mark.parametrize("counts", [
    [0, 5, 0, 0, 9, 0],  # empty first, middle and last batches
    [0, 0, 0, 0],  # V = 0
    [37],  # B = 1
    [1],
    "max_batch",  # B = SV_MAX_BATCH, random sizes with empty batches, batch 1023 occupied
], ids=["empty_edges", "V0", "B1", "B1_V1", "max_batch"])
def test_batch_offsets_equal_searchsorted(gpu, oracle, counts):
    L = _lib()
    rng = np.random.default_rng(11)
    if counts == "max_batch":
        counts = rng.integers(0, 4, size=L.SV_MAX_BATCH)
        counts[0], counts[-1] = 0, 3
    B = len(counts)
    keys = _keys_of(counts, oracle, rng)
    k = torch.from_numpy(keys.view(np.int64)).to(gpu)
    bs = torch.full((B + 2,), -7, dtype=torch.int32, device=gpu)  # one guard entry past B + 1
    L.call("sv_batch_offsets", L.ptr(k), c_int64(len(keys)), c_int(B), L.ptr(bs), L.stream_ptr())
    got = bs.cpu().numpy()
    want = np.searchsorted((keys >> np.uint64(54)).astype(np.int64), np.arange(B + 1), side="left")
    assert np.array_equal(got[:B + 1], want), f"first differing batch {np.flatnonzero(got[:B + 1] != want)[:8]}"
    assert got[B + 1] == -7


# ---------------------------------------------------------------------------------------------------------------------
# sv_global_pool (ME.MinkowskiGlobalMaxPooling / GlobalAvgPooling): MAX = torch.amax, AVG = the float64 mean
# ---------------------------------------------------------------------------------------------------------------------
def _pool_input(lengths, C, seed):
    """rows of len(lengths) batches; per non-empty batch k: a NaN in the last row of column 3k (the wave that holds it
    varies with the length), and with C >= 4 a +inf in the middle row of column 3k + 1, column 3k + 2 all -inf, and
    +inf / -inf in the first two rows of column 3k + 3 (NaN in the mean)"""
    g = torch.Generator().manual_seed(seed)
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    x = torch.randn(int(starts[-1]), C, generator=g)
    for k, n in enumerate(lengths):
        s = int(starts[k])
        if n == 0:
            continue
        x[s + n - 1, (3 * k) % C] = float("nan")
        if C >= 4:
            x[s + n // 2, (3 * k + 1) % C] = float("inf")
            x[s:s + n, (3 * k + 2) % C] = float("-inf")
            if n >= 2:
                x[s, (3 * k + 3) % C] = float("inf")
                x[s + 1, (3 * k + 3) % C] = float("-inf")
    return x, starts


def _global_pool(F, starts, mode, gpu):
    L = _lib()
    B, C = len(starts) - 1, F.shape[1]
    bs = torch.from_numpy(starts).to(gpu)
    out = torch.full((B + 1, C), -5.0, device=gpu)  # one guard row
    L.call("sv_global_pool", L.ptr(F), c_int64(F.stride(0)), c_int(C), L.ptr(bs), c_int(B), c_int(mode), L.ptr(out),
           L.stream_ptr())
    out = out.cpu()
    assert (out[B] == -5.0).all(), "global pool wrote past its [B, C] output"
    return out[:B]


@pytest.mark.parametrize("pad", [0, 5], ids=["contiguous", "ld_gt_C"])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 384, 1027])
def test_global_pool_matches_torch(gpu, C, pad):
    L = _lib()
    big = 100_003 if C <= 65 else 20_011  # the long segment; kept shorter at the wide C so the test stays ~1 s
    lengths = [0, 1, 2, 3, 4, 5, 63, big, 64, 65, 0]
    x, starts = _pool_input(lengths, C, seed=C + pad)
    F = _device_view(x, gpu, pad)
    mx = _global_pool(F, starts, L.SV_POOL_MAX, gpu)
    av = _global_pool(F, starts, L.SV_POOL_AVG, gpu)
    for b, n in enumerate(lengths):
        s, e = int(starts[b]), int(starts[b + 1])
        if n == 0:  # documented: an empty batch pools to 0 in both modes
            assert (mx[b] == 0).all() and (av[b] == 0).all(), f"empty batch {b} does not pool to 0"
            continue
        want = torch.amax(x[s:e], dim=0)
        same = (_bits(mx[b]) == _bits(want)) | (torch.isnan(mx[b]) & torch.isnan(want))
        bad = torch.nonzero(~same).flatten()[:6].tolist()
        assert not bad, f"MAX batch {b} (n={n}) columns {bad}: got {mx[b][bad].tolist()}, torch.amax {want[bad].tolist()}"
        xd = x[s:e].double()
        mean = xd.mean(0)
        fin = torch.isfinite(mean)
        got = av[b].double()
        bad = torch.nonzero(~fin & ~((got == mean) | (torch.isnan(got) & torch.isnan(mean)))).flatten()[:6].tolist()
        assert not bad, f"AVG batch {b} (n={n}) columns {bad}: got {got[bad].tolist()}, torch {mean[bad].tolist()}"
        bound = (math.ceil(n / 4) + 4) * U * xd.abs().sum(0) / n
        err = (got - mean).abs()
        bad = torch.nonzero(fin & ~(err <= bound)).flatten()[:6].tolist()
        assert not bad, f"AVG batch {b} (n={n}) columns {bad}: |err| {err[bad].tolist()} > bound {bound[bad].tolist()}"


def test_global_pool_nan_in_every_wave(gpu):
    """a NaN in any of the four waves' rows, alone or with +inf in another wave, decides the column"""
    L = _lib()
    x = torch.randn(40, 8, generator=torch.Generator().manual_seed(7))
    for c in range(4):
        x[20 + c, c] = float("nan")  # rows 20..23: one per wave
        if c < 3:
            x[21 + c, c] = float("inf")  # and +inf in the next wave
    x[:, 4] = float("-inf")
    x[7, 5] = float("inf")
    starts = np.array([0, 40], np.int32)
    got = _global_pool(_device_view(x, gpu, 0), starts, L.SV_POOL_MAX, gpu)[0]
    want = torch.amax(x, 0)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.isnan(want[:4]).all()
    assert torch.equal(got[4:], want[4:])


# ---------------------------------------------------------------------------------------------------------------------
# sv_slice_rows (SparseTensor.slice): a bit-exact gather
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 3], ids=["contiguous", "ld_gt_C"])
@pytest.mark.parametrize("C", [1, 3, 64, 1027])
def test_slice_rows_bit_exact_gather(gpu, C, pad):
    L = _lib()
    g = torch.Generator().manual_seed(C * 10 + pad)
    V = 1000
    x = torch.randn(V, C, generator=g)
    xb = x.view(torch.int32)
    xb[5, 0] = 0x7FC12345  # a NaN with a payload
    xb[6, C - 1] = 0x00000007  # a denormal
    xb[7, 0] = np.int32(-2 ** 31)  # -0.0
    x[8, C // 2] = float("-inf")
    F = _device_view(x, gpu, pad)
    for N in (0, 1, 255, 257, 300_000 if C <= 64 else 3_001):
        inv = torch.randint(0, V, (N,), generator=g)
        if N >= 4:
            inv[:4] = torch.tensor([5, 6, 7, 8])
        out = torch.full((N + 1, C), 9.0, device=gpu)  # one guard row
        L.call("sv_slice_rows", L.ptr(F), c_int64(F.stride(0)), c_int(C), L.ptr(inv.to(gpu)), c_int64(N), L.ptr(out),
               L.stream_ptr())
        out = out.cpu()
        assert torch.equal(_bits(out[:N]), _bits(x[inv])), f"N={N}: gather differs in {(_bits(out[:N]) != _bits(x[inv])).sum()} elements"
        assert (out[N] == 9.0).all(), f"N={N}: slice wrote past its [N, C] output"


# ---------------------------------------------------------------------------------------------------------------------
# sv_slice_argmax (slice + utils/output.py:67-73 `conf, preds = logits.max(1)`, sigmoid(conf))
# ---------------------------------------------------------------------------------------------------------------------
def _argmax_rows(C, g):
    """600 rows: 50 of small integers (ties), then NaN / inf / -inf patterns, then plain normals"""
    x = torch.randn(600, C, generator=g)
    x[:50] = torch.randint(-2, 3, (50, C), generator=g).float()
    nan, inf = float("nan"), float("inf")
    last, mid = C - 1, C // 2
    x[50, last] = nan  # NaN in the last column
    x[51, 0] = nan  # NaN in the first column
    x[52, mid] = nan  # two NaNs: the first one is the label
    x[52, last] = nan
    x[53, mid] = inf  # +inf twice: the first
    x[53, last] = inf
    x[54] = -inf  # all -inf: label 0, conf 0
    x[55] = -inf  # -inf and a NaN
    x[55, last] = nan
    x[56, min(1, last)] = inf  # +inf before a NaN: the NaN
    x[56, last] = nan
    x[57] = 0.25  # a whole row tied
    x[58, last] = 100.0  # the maximum in the last column
    x[59] = -inf  # -inf and one finite value
    x[59, mid] = -3.0
    return x


@pytest.mark.parametrize("pad", [0, 4], ids=["contiguous", "ld_gt_C"])
@pytest.mark.parametrize("C", [1, 2, 3, 9, 64, 1027])
def test_slice_argmax_matches_torch_max(gpu, C, pad):
    L = _lib()
    g = torch.Generator().manual_seed(100 + C + pad)
    x = _argmax_rows(C, g)
    V = x.shape[0]
    inverse = torch.cat([torch.arange(V), torch.randint(0, V, (1400,), generator=g)])
    inverse = inverse[torch.randperm(len(inverse), generator=g)]
    N = len(inverse)
    F = _device_view(x, gpu, pad)
    inv = inverse.to(gpu)
    want_v, want_i = x[inverse].max(1)
    for with_conf in (True, False):
        label = torch.full((N + 1,), -9, dtype=torch.int64, device=gpu)
        conf = torch.full((N + 1,), -9.0, device=gpu) if with_conf else None
        L.call("sv_slice_argmax", L.ptr(F), c_int64(F.stride(0)), c_int(C), L.ptr(inv), c_int64(N), L.ptr(label),
               L.ptr(conf), L.stream_ptr())
        label = label.cpu()
        bad = torch.nonzero(label[:N] != want_i).flatten()[:6]
        assert len(bad) == 0, (f"conf={with_conf}: labels of points {bad.tolist()} (rows {inverse[bad].tolist()}): got "
                               f"{label[bad].tolist()}, torch max(1) {want_i[bad].tolist()}")
        assert label[N] == -9
        if with_conf:
            conf = conf.cpu()
            assert conf[N] == -9.0
            got = conf[:N].double()
            assert torch.equal(torch.isnan(got), torch.isnan(want_v)), "conf is NaN exactly where torch's row max is"
            fin = ~torch.isnan(want_v)
            err = (got[fin] - torch.sigmoid(want_v[fin].double())).abs()
            assert err.max() <= 2.5e-7, f"conf off the float64 sigmoid by {err.max().item()}"


def test_slice_argmax_rejects_bad_shapes(gpu):
    L = _lib()
    F = torch.zeros(4, 3, device=gpu)
    inv = torch.zeros(2, dtype=torch.int64, device=gpu)
    out = torch.empty(2, dtype=torch.int64, device=gpu)
    for C, ld in ((0, 3), (4, 3)):
        with pytest.raises(L.SvHipError):
            L.call("sv_slice_argmax", L.ptr(F), c_int64(ld), c_int(C), L.ptr(inv), c_int64(2), L.ptr(out), None,
                   L.stream_ptr())


# ---------------------------------------------------------------------------------------------------------------------
# sv_voxel_reduce (ME UNWEIGHTED_AVERAGE quantisation / sparse_quantize's first point)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 7])
def test_voxel_reduce_matches_float64(gpu, C):
    L = _lib()
    rng = np.random.default_rng(C)
    g = torch.Generator().manual_seed(C)
    lengths = np.concatenate([[1, 2, 1000, 1, 2, 3, 1000, 2], rng.integers(1, 6, size=300)]).astype(np.int64)
    seg_start = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    P = int(seg_start[-1])
    perm = rng.permutation(P)
    order = np.concatenate([np.sort(perm[seg_start[v]:seg_start[v + 1]]) for v in range(len(lengths))]).astype(np.int32)
    feats = torch.randn(P, C, generator=g) * 3
    def seg(v):  # the points of voxel v
        return torch.from_numpy(order[seg_start[v]:seg_start[v + 1]].astype(np.int64))

    feats[seg(6)] += 1000.0  # 1000 duplicates far from 0: the sequential sum's rounding shows
    nan, inf = float("nan"), float("inf")
    feats[seg(0)[0], 0] = nan  # a single NaN point
    feats[seg(1)[1], 0] = nan  # NaN in the second of two
    feats[seg(2)[500], 0] = nan  # NaN among 1000 duplicates
    if C > 1:
        feats[seg(2)[10], C - 1] = inf
    feats[seg(4)[0], C - 1] = inf  # +inf with -inf: NaN
    feats[seg(4)[1], C - 1] = -inf
    feats[seg(5)[2], 0] = -inf  # -inf alone: -inf
    V = len(lengths)
    fg = feats.to(gpu)
    og = torch.from_numpy(order).to(gpu)
    sg = torch.from_numpy(seg_start).to(gpu)
    outs = {}
    for mode in (L.SV_REDUCE_MEAN, L.SV_REDUCE_FIRST):
        out = torch.full((V + 1, C), 4.0, device=gpu)
        L.call("sv_voxel_reduce", L.ptr(fg), c_int(C), L.ptr(og), L.ptr(sg), c_int64(V), c_int(mode), L.ptr(out),
               L.stream_ptr())
        out = out.cpu()
        assert (out[V] == 4.0).all(), "voxel_reduce wrote past its [V, C] output"
        outs[mode] = out[:V]
    assert torch.equal(_bits(outs[L.SV_REDUCE_FIRST]), _bits(feats[torch.from_numpy(order[seg_start[:-1]].astype(np.int64))]))
    fd = feats.double()
    mean = torch.stack([fd[seg(v)].mean(0) for v in range(V)])
    asum = torch.stack([fd[seg(v)].abs().sum(0) for v in range(V)])
    n = torch.from_numpy(lengths).double()[:, None]
    got = outs[L.SV_REDUCE_MEAN].double()
    fin = torch.isfinite(mean)
    assert torch.equal(torch.isnan(got), torch.isnan(mean)), "NaN features must give a NaN mean, and only they"
    assert torch.equal(got[~fin & ~torch.isnan(mean)], mean[~fin & ~torch.isnan(mean)])
    assert torch.isnan(mean[0, 0]) and torch.isnan(mean[2, 0]) and torch.isnan(mean[4, C - 1])
    err = (got - mean).abs()[fin]
    bound = ((n + 1) * U * asum / n).expand_as(mean)[fin]
    assert (err <= bound).all(), f"mean off the float64 mean by {(err / bound).max().item():.3f} x the bound"


# ---------------------------------------------------------------------------------------------------------------------
# sv_key_point_predictions (utils/output.py:81-87: softmax(1).max(0), > conf_th)
# ---------------------------------------------------------------------------------------------------------------------
def _kp_logits(N, C, variant, g):
    x = torch.randn(N, C, generator=g) * 2
    if N == 0:
        return x
    for c in range(C):  # a dominant row per class, half of them duplicated further down (an exact tie at the max)
        r = (c * 7919) % N
        x[r, c] += 8.0
        if c % 2 == 0 and N > 1:
            x[(r + N // 2) % N] = x[r]
    if C > 1:  # -inf entries, never a whole row (the column r % C of row r stays finite)
        mask = torch.rand(N, C, generator=g) < 0.05
        mask[torch.arange(N), torch.arange(N) % C] = False
        x[mask] = float("-inf")
    if variant == "nan_rows":
        for r in sorted({(2 * N) // 3, N // 3}):
            x[r, r % C] = float("nan")
    elif variant == "neg_inf_row":
        x[N // 2] = float("-inf")
    elif variant == "pos_inf":
        x[N // 4, C - 1] = float("inf")
    return x


def _threshold(p):
    """the middle of the widest gap between the per-class maxima (and 0, 1): far from every probability"""
    v = np.sort(np.concatenate([[0.0, 1.0], p[np.isfinite(p)]]))
    i = int(np.argmax(np.diff(v)))
    return float(v[i] + v[i + 1]) / 2


def _kp_call(F, C, N, th, gpu):
    L = _lib()
    ws = torch.empty(C, dtype=torch.int64, device=gpu)
    prob = torch.full((C,), -1.0, device=gpu)
    idx = torch.full((C,), -9, dtype=torch.int64, device=gpu)
    sel = torch.full((C,), -9, dtype=torch.int32, device=gpu)
    L.call("sv_key_point_predictions", L.ptr(F), c_int64(F.stride(0)), c_int(C), c_int64(N), c_float(th), L.ptr(ws),
           c_size_t(8 * C), L.ptr(prob), L.ptr(idx), L.ptr(sel), L.stream_ptr())
    return prob.cpu(), idx.cpu(), sel.cpu()


def _check_kp(x, prob, idx, sel, th, what):
    N, C = x.shape
    if N == 0:
        assert (prob == 0).all() and (idx == -1).all() and (sel == 0).all(), what
        return
    sm = x.double().softmax(1)
    pmax, pidx = sm.max(0)
    for c in range(C):
        tag = f"{what} class {c}"
        if torch.isnan(pmax[c]):
            assert torch.isnan(prob[c]), f"{tag}: torch's prob is NaN (row {pidx[c].item()}), got {prob[c].item()}"
            assert idx[c] == pidx[c], f"{tag}: idx {idx[c].item()}, torch's first NaN row {pidx[c].item()}"
            assert sel[c] == 0, f"{tag}: a NaN class is not selected"
            continue
        assert abs(prob[c].item() - pmax[c].item()) <= 1e-6 * pmax[c].item(), f"{tag}: prob {prob[c].item()} vs {pmax[c].item()}"
        tied = torch.nonzero(pmax[c] - sm[:, c] <= 2e-7 * pmax[c]).flatten()
        assert idx[c].item() in set(tied.tolist()), f"{tag}: idx {idx[c].item()} not among the maxima {tied[:6].tolist()}"
        assert sel[c] == int(pmax[c].item() > th), f"{tag}: selected {sel[c].item()} at threshold {th}"


@pytest.mark.parametrize("pad", [0, 3], ids=["contiguous", "ld_gt_C"])
@pytest.mark.parametrize("C", [1, 6, 8, 9, 17, 32])
def test_key_point_predictions_match_torch(gpu, C, pad):
    g = torch.Generator().manual_seed(1000 + 10 * C + pad)
    for N in (0, 1, 255, 256, 257, 300_000):
        for variant in ("finite", "nan_rows", "neg_inf_row", "pos_inf"):
            if N == 0 and variant != "finite":
                continue
            x = _kp_logits(N, C, variant, g)
            pm = x.double().softmax(1).max(0)[0].numpy() if N else np.zeros(C)
            th = _threshold(pm)
            prob, idx, sel = _kp_call(_device_view(x, gpu, pad), C, N, th, gpu)
            _check_kp(x, prob, idx, sel, th, f"N={N} {variant}")


def test_key_point_predictions_reject_more_than_32_classes(gpu):
    L = _lib()
    F = torch.zeros(10, 33, device=gpu)
    with pytest.raises(L.SvHipError):
        _kp_call(F, 33, 10, 0.5, gpu)
    ws = torch.empty(33 * 2, dtype=torch.int64, device=gpu)
    out = torch.empty(33 * 2, dtype=torch.int64, device=gpu)
    for G in (1, 0):
        segs = (c_int64 * (G + 1))(*([0, 10][:G + 1]))
        with pytest.raises(L.SvHipError):
            L.call("sv_key_point_predictions_batched", L.ptr(F), c_int64(33), c_int(33), segs, c_int(G), c_float(0.5),
                   L.ptr(ws), c_size_t(8 * 33 * 2), L.ptr(out), L.ptr(out), L.ptr(out), L.stream_ptr())


@pytest.mark.parametrize("C", [6, 9, 32])
def test_key_point_batched_equals_single_calls(gpu, C):
    L = _lib()
    g = torch.Generator().manual_seed(C)
    lengths = [0, 1, 300, 0, 257, 5000, 0]
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    x = torch.randn(int(starts[-1]), C, generator=g) * 3
    x[int(starts[2]) + 17, C // 2] = float("nan")  # a NaN row in segment 2
    x[int(starts[5]) + 4000] = float("-inf")  # an all -inf row in segment 5
    x[int(starts[4]) + 3] = x[int(starts[4]) + 200]  # a tie in segment 4
    F = _device_view(x, gpu, 2)
    G = len(lengths)
    ws = torch.empty(G * C, dtype=torch.int64, device=gpu)
    prob = torch.empty((G, C), device=gpu)
    idx = torch.empty((G, C), dtype=torch.int64, device=gpu)
    sel = torch.empty((G, C), dtype=torch.int32, device=gpu)
    th = 0.9
    segs = (c_int64 * (G + 1))(*starts.tolist())
    L.call("sv_key_point_predictions_batched", L.ptr(F), c_int64(F.stride(0)), c_int(C), segs, c_int(G), c_float(th),
           L.ptr(ws), c_size_t(8 * G * C), L.ptr(prob), L.ptr(idx), L.ptr(sel), L.stream_ptr())
    prob, idx, sel = prob.cpu(), idx.cpu(), sel.cpu()
    for k in range(G):
        s, e = int(starts[k]), int(starts[k + 1])
        p1, i1, s1 = _kp_call(F[s:e], C, e - s, th, gpu)
        assert torch.equal(_bits(prob[k]), _bits(p1)) and torch.equal(idx[k], i1) and torch.equal(sel[k], s1), f"segment {k}"
        _check_kp(x[s:e], prob[k], idx[k], sel[k], th, f"segment {k}")
    assert torch.isnan(prob[2]).all() and (idx[2] == 17).all() and torch.isnan(prob[5]).all() and (idx[5] == 4000).all()


def test_get_key_point_predictions_host_and_device_agree(gpu):
    """utils/output.get_key_point_predictions keeps the torch formulation for host tensors and calls the kernel for CUDA
    tensors: both must select the same classes and rows, NaN rows included"""
    from mrcc_amd.utils import output as Out

    g = torch.Generator().manual_seed(5)
    for C in (6, 9):
        N = 4000
        x = torch.randn(N, C, generator=g)
        for c in range(C - 1):  # classes 0 .. C - 2 have a clear winner above 0.999; class C - 1 stays below
            x[(c * 613) % N, c] += 20.0
        for variant in ("finite", "nan_row", "neg_inf_row"):
            y = x.clone()
            if variant == "nan_row":
                y[1234, 2] = float("nan")
            elif variant == "neg_inf_row":
                y[77] = float("-inf")
            hi, hc, hp = Out.get_key_point_predictions(y, conf_th=0.999)
            di, dc, dp = Out.get_key_point_predictions(y.to(gpu), conf_th=0.999)
            assert list(hc) == list(dc), f"C={C} {variant}: host classes {list(hc)}, device {list(dc)}"
            assert list(hi) == list(di), f"C={C} {variant}: host idx {list(hi)}, device {list(di)}"
            assert np.allclose(np.asarray(hp), np.asarray(dp), rtol=1e-6, atol=0)
            assert len(hc) == (C - 1 if variant == "finite" else 0)


# ---------------------------------------------------------------------------------------------------------------------
# end to end: a NaN colour through voxelisation, the U-Net and the fused slice + argmax
# ---------------------------------------------------------------------------------------------------------------------
def test_segmentation_with_nan_colours_matches_torch_max(gpu):
    import mrcc_amd
    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd.model.robotnet_segmentation import RobotNetSegmentation

    torch.manual_seed(1)
    model = RobotNetSegmentation(in_channels=3, num_classes=3).to(gpu).eval()
    # two clouds in one sparse tensor (batch column 0 and 1): convolutions never mix batches, so the NaN colours of
    # cloud 0 reach some points' logits and not all of them
    parts = []
    for b, seed in ((0, 3), (1, 4)):
        pts, rgb, _ = mrcc_amd.synth.gen_room(4000, 0.5, seed)
        parts.append((np.concatenate([np.full((len(pts), 1), b, np.float32), pts * np.float32(50)], axis=1), rgb))
    coords4 = np.concatenate([p[0] for p in parts])
    rgb = np.concatenate([p[1] for p in parts]).copy()
    rgb[[10, 500, 501], [0, 1, 2]] = np.nan
    with torch.no_grad():
        field = ME.TensorField(torch.from_numpy(rgb), torch.from_numpy(coords4),
                               quantization_mode=ME.SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE, device=gpu)
        out = model(field.sparse())
        label, conf = out.slice_argmax(field)
        logits = out.slice(field).F.cpu()
    want_v, want_i = logits.max(1)
    nan_pts = torch.isnan(logits).any(1)
    assert 0 < int(nan_pts.sum()) < len(nan_pts), f"{int(nan_pts.sum())} of {len(nan_pts)} points have NaN logits"
    assert torch.equal(label.cpu(), want_i)
    conf = conf.cpu()
    assert torch.equal(torch.isnan(conf), torch.isnan(want_v))
    fin = ~torch.isnan(want_v)
    assert (conf[fin].double() - torch.sigmoid(want_v[fin].double())).abs().max() <= 2.5e-7
