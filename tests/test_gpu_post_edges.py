"""The per-frame post-processing kernels at special values and structure edges: sv_topk_indices / sv_segment_topk (and
get_pred_center / get_pred_centers_batch over them), sv_col_stats / sv_center_scale (and normalize_points over them) and
sv_affine_act, each against a plain host restatement of its documented contract.

Expected results and bounds.
  top-k       tests/seg_loss_helpers.topk_rows: value based, NaN above +inf, equal values (-0.0 == +0.0, any two NaNs) by
              row.  Columns are written as uint32 bit patterns (tests/post_helpers.SPECIALS), so the sign and payload of
              every NaN and the sign of every zero are what the case says.  Exact.
  col_stats   min / max bit-equal to numpy's (which propagate NaN); the float64 sum against numpy's float64 sum within
              N * 2^-52 relative - the bound of any order of a float64 sum of N float32 addends of one sign ((N - 1) 2^-53
              each for the kernel and, at worst, the reference); twice the same bits.  The float32 max row norm bit-equal to
              np.linalg.norm(x - sub, axis=1).max() for 1 <= C <= 4.
  normalize_points   device against host within 1e-6 absolute on data in [-1, 1] (the mean is a float64 sum on the device
              and a pairwise float32 sum on the host: tests/test_gpu_dense.py uses the same tolerance).
  center_scale, affine_act   bit-equal to numpy float32 operations in the documented order / to oracle.affine_act (a NaN
              matches a NaN; the sign of zero counts), padding columns of the output untouched.
"""
import functools
import itertools
from ctypes import c_float, c_int, c_int64

import numpy as np
import pytest
import torch

import post_helpers as P
import seg_loss_helpers as H

pytestmark = pytest.mark.gpu

TOPK_CHUNK, SEGTOPK_CHUNK = 8192, 4096  # rows per stage-1 workgroup: csrc/sv_post.hip, csrc/sv_seg_loss.hip
NAN_BITS = list(P.NANS.values())
SENTINEL = -777.25


def _same_bits(got, want):
    """float32 arrays with the same bits; a NaN matches a NaN of any sign and payload"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != np.float32 or want.dtype != np.float32 or got.shape != want.shape:
        return False
    ng, nw = np.isnan(got), np.isnan(want)
    return np.array_equal(ng, nw) and np.array_equal(got.view(np.uint32)[~ng], want.view(np.uint32)[~nw])


# ---- A: the top-k order ---------------------------------------------------------------------------------------------------
def _rows(n, edges, count, rng):
    """`count` distinct rows (all n when there are fewer): the edge rows first, then random ones"""
    edges = [r for r in dict.fromkeys(edges) if 0 <= r < n]
    rest = np.setdiff1d(np.arange(n), edges)
    return (edges + rng.permutation(rest).tolist())[:count]


def _column(kind, n, k, edges, rng):
    """uint32 bit patterns of a column of n votes; the rows `edges` hold values that belong to the k largest"""
    bits = P.bits_of(rng.normal(size=n)).copy()
    if kind == "zeros":  # only zeros, alternating, -0.0 first
        bits = np.where(np.arange(n) % 2 == 0, P.SIGN, 0).astype(np.uint32)
    elif kind == "few_nans":  # fewer NaNs than k, mixed among +inf rows
        rows = sorted(_rows(n, edges, k // 2 + k, rng))
        nan_rows = set(rows[1::3][:k // 2])
        for j, r in enumerate(rows):
            bits[r] = NAN_BITS[j % len(NAN_BITS)] if r in nan_rows else P.SPECIALS["+inf"]
    elif kind == "many_nans":  # more NaNs than k, every sign and payload
        for j, r in enumerate(_rows(n, edges, 2 * k + 3, rng)):
            bits[r] = NAN_BITS[j % len(NAN_BITS)]
        for r in _rows(n, [], 3, rng):
            if (bits[r] & 0x7fffffff) <= 0x7f800000:
                bits[r] = P.SPECIALS["+inf"]
    elif kind == "all":  # every special value twice among random normals; NaNs of each kind on the edge rows
        values = NAN_BITS + list(P.SPECIALS.values()) * 2
        for j, r in enumerate(_rows(n, edges, len(values), rng)):
            bits[r] = values[j]
    else:
        raise ValueError(kind)
    return bits


KINDS = ("zeros", "few_nans", "many_nans", "all")


def _table(bits, gpu):
    """[n, 4] float32 device table with the column at index 1 (row stride 4), quiet NaNs around it"""
    t = np.full((len(bits), 4), 0x7fc00000, np.uint32)
    t[:, 1] = bits
    return torch.from_numpy(t.view(np.float32)).to(gpu)


def _topk_rows(col, k):
    with np.errstate(invalid="ignore"):  # the float64 cast of a signalling NaN
        return H.topk_rows(col, k)


@pytest.mark.parametrize("k", [1, 8, 64])
@pytest.mark.parametrize("n", [1, 5, TOPK_CHUNK - 1, TOPK_CHUNK, TOPK_CHUNK + 1, 3 * TOPK_CHUNK + 7])
def test_topk_indices_orders_special_values_as_documented(gpu, n, k):
    from mrcc_amd.utils.output import topk_indices

    rng = np.random.default_rng(100 * n + k)
    edges = [0, n - 1, TOPK_CHUNK - 1, TOPK_CHUNK]  # the column's ends and the two sides of the first chunk edge
    wrong = []  # every kind is run before the verdict, so a failure names all the kinds that are off
    for kind in KINDS:
        bits = _column(kind, n, k, edges, rng)
        col = P.f32(bits)
        want = _topk_rows(col, k)[:min(k, n)]
        if kind == "zeros":
            assert np.array_equal(want, np.arange(min(k, n)))
        if kind == "many_nans":
            assert np.array_equal(want, np.where(np.isnan(col))[0][:k])  # the lowest NaN rows in row order
        got = topk_indices(_table(bits, gpu)[:, 1], k)
        assert got.dtype == torch.int64
        if not np.array_equal(got.cpu().numpy(), want):
            wrong.append((kind, got.cpu().numpy()[:8], want[:8]))
    assert not wrong, wrong


@pytest.mark.parametrize("n", [1, TOPK_CHUNK + 1])
def test_topk_indices_selects_a_nan_in_row_0_whatever_its_bits(gpu, n):
    """row 0 has the all-ones index bits: with all-ones value bits above them a key would equal the selection's start value"""
    from mrcc_amd.utils.output import segment_topk_indices, topk_indices

    rng = np.random.default_rng(n)
    for pattern, k in itertools.product(NAN_BITS, (1, 8)):
        bits = P.bits_of(rng.normal(size=n)).copy()
        bits[0] = pattern
        want = _topk_rows(P.f32(bits), k)[:min(k, n)]
        assert want[0] == 0
        table = _table(bits, gpu)
        assert np.array_equal(topk_indices(table[:, 1], k).cpu().numpy(), want), hex(pattern)
        got = segment_topk_indices(table[:, 1], torch.tensor([0, n], dtype=torch.int32, device=gpu), k)
        assert np.array_equal(got.cpu().numpy()[0, :min(k, n)], want), hex(pattern)


def _frame_offsets(n):
    # fewer rows than k; an empty frame; a frame one row longer than a chunk; one of two chunks and a bit; the rest
    return [min(c, n) for c in (0, 3, 3, 3 + SEGTOPK_CHUNK + 1, 12300)] + [n]


@pytest.mark.parametrize("k", [1, 8, 64])
@pytest.mark.parametrize("n", [1, 5, TOPK_CHUNK + 1, 3 * TOPK_CHUNK + 7])
def test_segment_topk_orders_special_values_as_documented(gpu, n, k):
    from mrcc_amd.utils.output import segment_topk_indices, topk_indices

    rng = np.random.default_rng(100 * n + k + 1)
    off = _frame_offsets(n)
    B = len(off) - 1
    # first and last row of every frame, and both sides of every chunk edge inside a frame
    edges = [r for lo, hi in zip(off[:-1], off[1:])
             for r in (lo, hi - 1, *(lo + c - d for c in range(SEGTOPK_CHUNK, hi - lo, SEGTOPK_CHUNK) for d in (1, 0))) if lo <= r < hi]
    d_off = torch.tensor(off, dtype=torch.int32, device=gpu)
    wrong = []
    for kind in KINDS:
        bits = _column(kind, n, k, edges, rng)
        col = P.f32(bits)
        table = _table(bits, gpu)
        got = segment_topk_indices(table[:, 1], d_off, k)
        assert got.dtype == torch.int64 and got.shape == (B, k)
        host = got.cpu().numpy()
        with np.errstate(invalid="ignore"):
            want = H.segment_topk(col, off, k)
        if not np.array_equal(host, want):
            wrong.append((kind, [b for b in range(B) if not np.array_equal(host[b], want[b])]))
        for b, (lo, hi) in enumerate(zip(off[:-1], off[1:])):
            m = min(k, hi - lo)
            assert (host[b, m:] == -1).all()
            if hi > lo:  # frame by frame the single-column selection on the frame's slice
                assert np.array_equal(host[b, :m], topk_indices(table[lo:hi, 1], k).cpu().numpy()), (kind, b)
    assert not wrong, f"(kind, frames that differ): {wrong}"


def _votes(n, rng, nan_rows, zero_rows):
    """[n, 2] float32 bit patterns: negative votes, sign-set NaNs, and zeros that alternate starting with -0.0"""
    out = P.bits_of(-np.abs(rng.normal(size=(n, 2))) - 1.0).copy()
    out[nan_rows, 1] = P.SPECIALS["-nan"]
    out[zero_rows, 1] = np.where(np.arange(len(zero_rows)) % 2 == 0, P.SIGN, 0).astype(np.uint32)
    return out.view(np.float32)


def test_pred_center_takes_sign_set_nans_first_and_zeros_of_either_sign_by_row(gpu):
    from mrcc_amd.utils.output import get_pred_center

    rng = np.random.default_rng(21)
    n = 300
    out = _votes(n, rng, [17, 250], list(range(40, 50)))
    assert _topk_rows(out[:, 1], 8).tolist() == [17, 250, 40, 41, 42, 43, 44, 45]
    coords = rng.integers(-200, 200, size=(n, 3)).astype(np.float64)  # integers: the mean of eight is exact in any order
    got = get_pred_center(torch.from_numpy(out).to(gpu), coords)
    want = H.pred_centers(out, np.concatenate([np.zeros((n, 1)), coords], 1), [0, n], 1.0)[0]
    assert np.array_equal(got, want)


def test_pred_centers_batch_takes_sign_set_nans_first_and_zeros_of_either_sign_by_row(gpu):
    from mrcc_amd.utils.output import get_pred_centers_batch

    rng = np.random.default_rng(22)
    off = [0, 300, 305, 900]  # the middle frame has fewer than 8 rows
    n, qs = off[-1], 0.02
    out = _votes(n, rng, [17, 250, 301, 899], list(range(40, 50)) + [300, 302, 303] + list(range(600, 610)))
    coords = np.concatenate([np.zeros((n, 1)), rng.integers(-200, 200, size=(n, 3))], 1).astype(np.int32)
    got = get_pred_centers_batch(torch.from_numpy(out).to(gpu), torch.from_numpy(coords).to(gpu),
                                 torch.tensor(off, dtype=torch.int32, device=gpu), qs)
    with np.errstate(invalid="ignore"):
        want = H.pred_centers(out, coords, off, qs)
    assert got.dtype == torch.float32 and got.shape == (3, 3) and not np.isnan(want).any()
    gh = got.cpu().numpy().astype(np.float64)
    # one float32 rounding of a float64 value (tests/test_gpu_seg_loss.py)
    assert (np.abs(gh - want) <= 2.0 ** -23 * np.maximum(1.0, np.abs(want))).all()


# ---- B: normalize_points, device against host, every admitted width -----------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_normalize_points_device_path_agrees_with_the_host_path(gpu, C):
    from mrcc_amd.utils import preprocess as PP

    rng = np.random.default_rng(30 + C)
    x = rng.uniform(-1, 1, size=(5000, C)).astype(np.float32)
    last = (x * np.float32(0.25)).astype(np.float32)
    last[123, C - 1] = 1.0  # the largest norm comes from the last column alone
    for pts in (x, last):
        got = PP.normalize_points(torch.from_numpy(pts).to(gpu))
        want = PP.normalize_points(pts)
        assert got.shape == want.shape and got.dtype == torch.float32
        err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
        print(f"C={C}: max |device - host| = {err:.3e}")
        assert np.allclose(got.cpu().numpy(), want, atol=1e-6, rtol=0)
        # the max row norm itself: float32 operations in numpy's order, bit for bit
        sub = pts.mean(0).astype(np.float32)
        want_norm = np.linalg.norm(pts - sub, axis=1).max()
        assert want_norm.dtype == np.float32
        _, _, _, nm = PP._stats(torch.from_numpy(pts).to(gpu), torch.from_numpy(sub).to(gpu), want_norm=True)
        assert _same_bits(nm.cpu().numpy(), np.array([want_norm])), (nm.item(), want_norm)
    assert np.linalg.norm(last - last.mean(0).astype(np.float32), axis=1).argmax() == 123


# ---- C: sv_col_stats and sv_center_scale ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stat_base(N, C):
    """float32 [N, C], even columns in [1, 2), odd columns in (-2, -1]: each column's addends have one sign"""
    rng = np.random.default_rng(1000 * C + N)
    x = rng.uniform(1, 2, size=(N, C)).astype(np.float32)
    x[:, 1::2] *= -1
    x.setflags(write=False)
    return x


def _plant_variants(N, C):
    """lists of (kind, row, column): the unique minimum of one column in the last row, the unique maximum of another in
    row 0, and one of each on the first row of the last slab - in one array when the four cells and the columns of the two
    minima (and maxima) differ, else one array per plant"""
    blocks, rpb = P.stats_slabs(N)
    s = rpb * (blocks - 1)
    plants = [("min", N - 1, 0), ("max", 0, C - 1), ("min", s, C - 1), ("max", s, 0)]
    if C >= 2 and len({(r, c) for _, r, c in plants}) == 4:
        return [plants]
    return [[p] for p in plants]


def _planted(base, plants):
    x = base.copy()
    for kind, r, c in plants:
        x[r, c] = x[:, c].min() - np.float32(0.75) if kind == "min" else x[:, c].max() + np.float32(0.75)
        assert (x[:, c] == x[r, c]).sum() == 1 and x[r, c] == (x[:, c].min() if kind == "min" else x[:, c].max())
    return x


def _strided(x, gpu):
    """columns 1 : 1 + C of an [N, 6] device buffer of NaNs"""
    buf = torch.full((x.shape[0], 6), float("nan"), dtype=torch.float32, device=gpu)
    buf[:, 1:1 + x.shape[1]] = torch.from_numpy(x).to(gpu)
    return buf[:, 1:1 + x.shape[1]]


def _check_stats(x, view):
    from mrcc_amd.utils.preprocess import _stats

    N = x.shape[0]
    mn, mx, sm, _ = _stats(view)
    mn2, mx2, sm2, _ = _stats(view)
    with np.errstate(invalid="ignore"):
        want_mn, want_mx, want_sum = x.min(0), x.max(0), np.sum(x.astype(np.float64), axis=0)
    # bit-equal extrema (no planted or random value is a zero, so value equality is bit equality)
    assert np.array_equal(mn.cpu().numpy(), want_mn, equal_nan=True), (mn.cpu().numpy(), want_mn)
    assert np.array_equal(mx.cpu().numpy(), want_mx, equal_nan=True), (mx.cpu().numpy(), want_mx)
    got = sm.cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(np.isnan(got), np.isnan(want_sum))
    ok = ~np.isnan(want_sum)
    rel = np.abs(got[ok] - want_sum[ok]) / np.abs(want_sum[ok])
    print(f"N={N}: worst relative sum error {rel.max() if ok.any() else 0.0:.3e} (bound {N * 2.0 ** -52:.3e})")
    assert (rel <= N * 2.0 ** -52).all()
    assert torch.equal(sm.view(torch.int64), sm2.view(torch.int64))  # run to run: the same bits
    assert torch.equal(mn.view(torch.int32), mn2.view(torch.int32)) and torch.equal(mx.view(torch.int32), mx2.view(torch.int32))
    return mn.cpu().numpy(), mx.cpu().numpy(), got


@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193])
def test_col_stats_extrema_on_slab_and_wave_edges(gpu, N, C):
    for plants in _plant_variants(N, C):
        x = _planted(_stat_base(N, C), plants)
        _check_stats(x, _strided(x, gpu))


def test_col_stats_with_the_slab_count_capped(gpu):
    """N = 1024 * 4096 + 1: the grid stays at 1024 slabs and a slab has 4097 rows for the first time"""
    N, C = 1024 * 4096 + 1, 3
    assert P.stats_slabs(N) == (1024, 4097)
    (plants,) = _plant_variants(N, C)
    assert ("min", 4097 * 1023, C - 1) in plants
    x = _planted(_stat_base.__wrapped__(N, C), plants)  # 50 MB: not kept in the cache
    _check_stats(x, torch.from_numpy(x).to(gpu))


@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("N", [65, 4097, 8193])
def test_col_stats_nan_and_infinities(gpu, N, C):
    base = _stat_base(N, C)
    # a NaN only in the last row of the last slab: NaN extrema (and sum) in that column only
    x = base.copy()
    x[N - 1, C - 1] = np.nan
    mn, mx, sm = _check_stats(x, _strided(x, gpu))
    nan_cols = np.arange(C) == C - 1
    assert np.array_equal(np.isnan(mn), nan_cols) and np.array_equal(np.isnan(mx), nan_cols)
    assert np.array_equal(np.isnan(sm), nan_cols)
    # both infinities in one column
    x = base.copy()
    x[0, 0], x[N - 1, 0] = np.inf, -np.inf
    mn, mx, sm = _check_stats(x, _strided(x, gpu))
    assert mx[0] == np.inf and mn[0] == -np.inf and np.isnan(sm[0]) and not np.isnan(sm[1:]).any()


def _operand(C, special, which, rng):
    """a [C] float32 operand of sv_center_scale; `special`: a zero divisor, an inf subtrahend, a NaN addend"""
    v = rng.uniform(0.5, 2.0, size=C).astype(np.float32) * rng.choice(np.float32([-1, 1]), size=C)
    if special:
        v[{"sub": 2, "div": 1, "add": 0}[which] % C::3] = {"sub": np.inf, "div": 0.0, "add": np.nan}[which]
    return v


@pytest.mark.parametrize("C", [1, 3, 4, 7])
@pytest.mark.parametrize("N", [0, 1, 257])
def test_center_scale_every_operand_subset_strides_and_special_values(gpu, N, C):
    from mrcc_amd import _lib

    rng = np.random.default_rng(40 + 10 * N + C)
    ld, out_ld = C + 2, C + 3
    xin = np.full((N, ld), np.nan, np.float32)
    x = rng.uniform(-1, 1, size=(N, C)).astype(np.float32)
    for j, v in enumerate((np.inf, -np.inf, np.nan, 0.0, -0.0)):  # one special per row, walking through the columns
        if N:
            x[(3 * j) % N, j % C] = v
    xin[:, :C] = x
    d_x = torch.from_numpy(xin).to(gpu)
    for special, (use_sub, use_div, use_add) in itertools.product((False, True), itertools.product((False, True), repeat=3)):
        ops = {w: _operand(C, special, w, rng) if use else None
               for w, use in (("sub", use_sub), ("div", use_div), ("add", use_add))}
        dev = {w: None if v is None else torch.from_numpy(v).to(gpu) for w, v in ops.items()}
        out = torch.full((N, out_ld), SENTINEL, dtype=torch.float32, device=gpu)
        _lib.call("sv_center_scale", _lib.ptr(d_x), c_int64(ld), c_int64(N), c_int(C), _lib.ptr(dev["sub"]), _lib.ptr(dev["div"]),
                  _lib.ptr(dev["add"]), _lib.ptr(out), c_int64(out_ld), _lib.stream_ptr())
        got = out.cpu().numpy()
        want = x.copy()
        with np.errstate(all="ignore"):  # float32 operations in the documented order
            if use_sub:
                want = want - ops["sub"]
            if use_div:
                want = want / ops["div"]
            if use_add:
                want = want + ops["add"]
        assert want.dtype == np.float32
        assert (got[:, C:] == np.float32(SENTINEL)).all(), "padding columns of out were written"
        assert _same_bits(got[:, :C], want), (special, use_sub, use_div, use_add)
        if not (use_sub or use_div or use_add):  # a strided copy, bit for bit
            assert np.array_equal(got[:, :C].copy().view(np.uint32), x.view(np.uint32))


# ---- D: sv_affine_act --------------------------------------------------------------------------------------------------------
ACTS = [(0, 0.01), (1, 0.01)] + [(2, s) for s in (0.01, 0.0, -0.5, 2.0)]  # SV_ACT_NONE, SV_ACT_RELU, SV_ACT_LEAKY_RELU x slopes
X_CANCEL, S_CANCEL = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12)
B_CANCEL = np.float32(-(1 + 2.0 ** -11))  # fl(x s) = 1 + 2^-11 (a tie, to even): x s + b is 0 in two roundings, 2^-24 fused


@functools.lru_cache(maxsize=None)
def _affine_inputs(V, C):
    rng = np.random.default_rng(50 + 7 * V + C)
    x = rng.normal(size=(V, C)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, size=C).astype(np.float32) * rng.choice(np.float32([-1, 1]), size=C)
    shift = rng.normal(size=C).astype(np.float32)
    res = rng.normal(size=(V, C)).astype(np.float32)
    c0 = C - 1  # the cancelling column
    scale[c0], shift[c0] = S_CANCEL, B_CANCEL
    if V:
        x[::5, c0] = X_CANCEL
        res[::10, c0] = 0.0
        flat = x.reshape(-1)
        for j, v in enumerate((np.nan, np.inf, -np.inf, -0.0, 0.0)):
            flat[(7 * j + 3) % flat.size::max(flat.size // 4, 1) + 1] = v
        res.reshape(-1)[(11 % res.size)::max(res.size // 3, 1) + 2] = np.float32(-np.inf)
        res.reshape(-1)[(5 % res.size)::max(res.size // 3, 1) + 3] = np.float32(np.nan)
    for a in (x, scale, shift, res):
        a.setflags(write=False)
    return x, scale, shift, res


@pytest.mark.parametrize("V,C", [(0, 5), (1, 1), (257, 3), (300, 65), (129, 1027)])
def test_affine_act_every_branch_against_the_oracle_and_torch(gpu, oracle, V, C):
    from mrcc_amd import nn as svnn

    x, scale, shift, res = _affine_inputs(V, C)
    if V >= 5:
        assert np.float32(X_CANCEL * S_CANCEL) + B_CANCEL == 0 and np.float32(np.float64(X_CANCEL) * S_CANCEL + B_CANCEL) == np.float32(2.0 ** -24)
    t = lambda a: torch.tensor(a).to(gpu)
    xbuf = torch.full((V, C + 3), float("nan"), dtype=torch.float32, device=gpu)
    xbuf[:, :C] = t(x)
    d_x = xbuf[:, :C]  # input row stride C + 3
    rbuf = torch.full((V, C + 5), float("nan"), dtype=torch.float32, device=gpu)
    rbuf[:, 2:2 + C] = t(res)
    d_res = {"none": None, "dense": t(res), "strided": rbuf[:, 2:2 + C]}
    d_scale, d_shift = t(scale), t(shift)
    for use_scale, use_shift, res_kind, (act, slope) in itertools.product((False, True), (False, True), d_res, ACTS):
        case = (use_scale, use_shift, res_kind, act, slope)
        got = svnn.affine_act(d_x, d_scale if use_scale else None, d_shift if use_shift else None, d_res[res_kind], act, slope)
        got = got.cpu().numpy()
        want = oracle.affine_act(x, scale if use_scale else None, shift if use_shift else None,
                                 None if res_kind == "none" else res, act, slope)
        assert got.shape == (V, C) and _same_bits(got, want), case
        if not use_scale:  # plain float32 adds, then torch's own activation on the CPU; the sign of a zero is not compared
            with np.errstate(invalid="ignore"):
                y = x + shift if use_shift else x
                y = y + res if res_kind != "none" else y
            ty = torch.tensor(y)
            ref = ty if act == 0 else (torch.relu(ty) if act == 1 else torch.nn.functional.leaky_relu(ty, slope))
            assert np.array_equal(got, ref.numpy(), equal_nan=True), case
            assert np.array_equal(want, ref.numpy(), equal_nan=True), ("oracle.affine_act against torch", case)


def test_affine_act_leaves_the_padding_of_a_wider_output_alone(gpu, oracle):
    from mrcc_amd import _lib

    V, C = 257, 3
    x, scale, shift, res = _affine_inputs(V, C)
    t = lambda a: torch.tensor(a).to(gpu)
    d_x, d_scale, d_shift, d_res = t(x), t(scale), t(shift), t(res)
    out = torch.full((V, C + 4), SENTINEL, dtype=torch.float32, device=gpu)
    _lib.call("sv_affine_act", _lib.ptr(d_x), c_int64(C), c_int(C), c_int64(V), _lib.ptr(d_scale), _lib.ptr(d_shift),
              _lib.ptr(d_res), c_int64(C), c_int(_lib.SV_ACT_LEAKY_RELU), c_float(0.01), _lib.ptr(out), c_int64(C + 4),
              _lib.stream_ptr())
    got = out.cpu().numpy()
    assert (got[:, C:] == np.float32(SENTINEL)).all(), "padding columns of out were written"
    assert _same_bits(got[:, :C], oracle.affine_act(x, scale, shift, res, oracle.ACT_LEAKY, 0.01))
