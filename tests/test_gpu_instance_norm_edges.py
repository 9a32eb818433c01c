"""sv_instance_norm / sv_instance_norm_backward at their edges: up to SV_MAX_BATCH frames with runs of empty ones and frame
starts on and off the 256-row chunk grid, column views and row ranges inside sentinel buffers, inputs on which only a two-pass
float64 variance survives, NaN / Inf confinement, and the backward at the bound its arithmetic gives.

Bounds.  Forward: 2^-23 |want| + 1e-12 of instance_norm_ref (one float32 rounding plus float64 summation-order noise, the
bound of tests/test_gpu_instance_norm.py).  mean / inv_std: 2^-40 relative (order noise is n 2^-53 for n <= 1029 rows, with
margin; per-channel offsets of magnitude 2 to 10 keep every mean away from 0, so that a relative bound on it means something).
Backward: the kernel and the reference (the header's formula in float64 numpy, its three terms kept apart) are given the SAME
mean / inv_std, so the bound is one float32 rounding plus order noise of the sums: dx within 2^-23 |want| + 2^-40 inv_std
(|g| + |mean_b g| + |xhat mean_b(g xhat)|), dweight / dbias within 2^-23 |want| + 2^-40 sum |terms|."""
import numpy as np
import pytest

import strided_helpers as H

pytestmark = pytest.mark.gpu

CHUNK = 256
NONE, RELU, GELU = 0, 1, 3
EPS = 1e-8
CYCLE = (0, 0, 1, 2, 63, 0, 64, 65, 1, 0, 0, 0, 5)


def _many_frames(B):
    """B frame sizes: CYCLE repeated, with frames of 255, 256, 257 and 3 * 256 + 5 rows put in so that frame starts fall on
    multiples of 256 (one earlier frame is lengthened until the 256-row frame starts, and so ends, on one) and off them; the
    first frame is empty, the last one is not (the frame search of the apply kernels must reach it)"""
    sizes = [CYCLE[i % len(CYCLE)] for i in range(B)]
    sizes[B - 1] = 5
    sizes[3], sizes[B // 2], sizes[B // 2 + 1], sizes[B - 4] = CHUNK + 1, 3 * CHUNK + 5, CHUNK - 1, CHUNK
    starts = np.concatenate([[0], np.cumsum(sizes)])
    pad = int(-starts[B - 4] % CHUNK)
    sizes[4] += pad
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    assert starts[B - 4] % CHUNK == 0 and starts[B - 3] % CHUNK == 0 and sizes[B - 4] == CHUNK
    assert (starts[1:-1][np.array(sizes[1:]) > 0] % CHUNK != 0).any()
    assert any(sizes[i] == sizes[i + 1] == sizes[i + 2] == 0 for i in range(B - 2)) and sizes[0] == 0 and sizes[-1] > 0
    return tuple(sizes)


def _case(sizes, C, seed, lead=0, tail=0):
    """(x, starts, w, b): per-channel scales in [0.1, 5] and offsets of magnitude in [2, 10]; with more than one channel,
    channel 0 is constant (zero variance: inv_std = 1 / sqrt(eps) = 1e4).  lead / tail: rows before starts[0] / after
    starts[B] that belong to no frame."""
    rng = np.random.default_rng(seed)
    starts = (lead + np.concatenate([[0], np.cumsum(sizes)])).astype(np.int32)
    V = int(starts[-1]) + tail
    off = rng.uniform(2, 10, size=C) * rng.choice([-1.0, 1.0], size=C)
    x = (rng.standard_normal((V, C)) * rng.uniform(0.1, 5.0, size=C) + off).astype(np.float32)
    if C > 1:
        x[:, 0] = np.float32(3.25)
    w = rng.uniform(0.5, 2.0, size=C).astype(np.float32) * rng.choice([-1.0, 1.0], size=C).astype(np.float32)
    b = rng.uniform(-1.0, 1.0, size=C).astype(np.float32)
    return x, starts, w, b


def _ratio(err, bound):
    return float((err / bound).max()) if err.size else 0.0


def _check_stats(mean, inv_std, x, starts):
    want_m, want_i = H.instance_norm_stats_ref(x, starts, EPS)
    empty = np.diff(starts) == 0
    mean, inv_std = mean.cpu().numpy(), inv_std.cpu().numpy()
    assert (mean[empty] == 0).all() and (inv_std[empty] == 0).all()  # exactly 0, not the buffers' sentinel
    r = max(_ratio(np.abs(mean - want_m)[~empty], 2.0 ** -40 * np.abs(want_m)[~empty]),
            _ratio(np.abs(inv_std - want_i)[~empty], 2.0 ** -40 * np.abs(want_i)[~empty]))
    assert r <= 1.0, r
    return r


@pytest.mark.parametrize("act", [NONE, RELU, GELU])
@pytest.mark.parametrize("C", [1, 65])
@pytest.mark.parametrize("B", [37, 1024])
def test_many_frames(gpu, B, C, act):
    import torch

    import mrcc_amd

    assert mrcc_amd._lib.SV_MAX_BATCH == 1024 and mrcc_amd._lib.SV_NORM_CHUNK_ROWS == CHUNK
    sizes = _many_frames(B)
    x, starts, w, b = _case(sizes, C, seed=B + C + 7 * act)
    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    y, mean, inv_std = H.gpu_instance_norm(t(x), t(starts), t(w), t(b), EPS, act)
    want = H.instance_norm_ref(x, starts, w, b, EPS, act)
    err, bound = np.abs(y.cpu().numpy().astype(np.float64) - want), H.norm_forward_bound(want)
    rs = _check_stats(mean, inv_std, x, starts)
    print(f"instance norm B={B} V={len(x)} C={C} act={act}: max err / bound = {_ratio(err, bound):.3f}, statistics {rs:.3g}")
    assert (err <= bound).all()
    again = H.gpu_instance_norm(t(x), t(starts), t(w), t(b), EPS, act)
    assert all(torch.equal(p, q) for p, q in zip((y, mean, inv_std), again))


@pytest.mark.parametrize("act", [NONE, GELU])
@pytest.mark.parametrize("C", [5, 64])
def test_column_views_and_row_ranges(gpu, C, act):
    """x, y, dy, dx as columns 1 .. C of [V, C + 3] sentinel buffers, batch_start = [7, 300, 300, 520] of V = 533 rows: the bits
    of the contiguous call, sentinel columns and the rows of no frame untouched, the frames equal to the reference"""
    import torch

    x, starts, w, b = _case((293, 0, 220), C, seed=C + act, lead=7, tail=13)
    assert starts.tolist() == [7, 300, 300, 520] and len(x) == 533
    dy = np.random.default_rng(C).standard_normal(x.shape).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    S = 77.0

    def view(a=None):
        buf = torch.full((533, C + 3), S, dtype=torch.float32, device=gpu)
        if a is not None:
            buf[:, 1:C + 1] = t(a)
        return buf, buf[:, 1:C + 1]

    (xb, xv), (yb, yv), (dyb, dyv), (dxb, dxv) = view(x), view(), view(dy), view()
    st = t(starts)
    y0, mean0, inv0 = H.gpu_instance_norm(t(x), st, t(w), t(b), EPS, act)
    y1, mean1, inv1 = H.gpu_instance_norm(xv, st, t(w), t(b), EPS, act, y=yv)
    dx0, dw0, db0 = H.gpu_instance_norm_backward(t(x), st, t(w), t(b), mean0, inv0, act, t(dy))
    dx1, dw1, db1 = H.gpu_instance_norm_backward(xv, st, t(w), t(b), mean1, inv1, act, dyv, dx=dxv)
    assert torch.equal(mean0, mean1) and torch.equal(inv0, inv1) and torch.equal(dw0, dw1) and torch.equal(db0, db1)
    inside = slice(7, 520)
    assert torch.equal(y0[inside], y1[inside]) and torch.equal(dx0[inside], dx1[inside])
    for buf in (yb, dxb):
        assert (buf[:, 0] == S).all() and (buf[:, C + 1:] == S).all() and (buf[:7] == S).all() and (buf[520:] == S).all()
    assert (y0[:7] == H.SENTINEL).all() and (y0[520:] == H.SENTINEL).all()
    assert (dx0[:7] == H.SENTINEL).all() and (dx0[520:] == H.SENTINEL).all()
    assert (xb[:, 0] == S).all() and (dyb[:, C + 1:] == S).all()
    want = H.instance_norm_ref(x, starts, w, b, EPS, act)
    err = np.abs(y1.cpu().numpy().astype(np.float64) - want)[inside]
    assert (err <= H.norm_forward_bound(want)[inside]).all()
    _check_stats(mean1, inv1, x, starts)
    rdx, rdw, rdb, noise, nw, nb = H.instance_norm_backward_ref(x, starts, w, b, mean1.cpu().numpy(), inv1.cpu().numpy(), act, dy)
    assert (np.abs(dx1.cpu().numpy() - rdx)[inside] <= (2.0 ** -23 * np.abs(rdx) + 2.0 ** -40 * noise)[inside]).all()
    assert (np.abs(dw1.cpu().numpy() - rdw) <= 2.0 ** -23 * np.abs(rdw) + 2.0 ** -40 * nw).all()
    assert (np.abs(db1.cpu().numpy() - rdb) <= 2.0 ** -23 * np.abs(rdb) + 2.0 ** -40 * nb).all()


@pytest.mark.parametrize("act", [NONE, RELU, GELU])
def test_cancellation(gpu, act):
    """H.cancellation_case: the mean is exact in any order (the kernel's bits are the reference's), the variance is 2^-46 of
    the mean square.  tests/test_resnet_ops_edges_cpu.py shows that a one-pass float64 variance and float32 statistics miss
    this bound by many orders of magnitude."""
    import torch

    x, starts, k, base = H.cancellation_case()
    C = x.shape[1]
    w, b = np.linspace(0.5, 2.0, C).astype(np.float32), np.linspace(-1.0, 1.0, C).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    y, mean, inv_std = H.gpu_instance_norm(t(x), t(starts), t(w), t(b), EPS, act)
    want_m, want_i = H.instance_norm_stats_ref(x, starts, EPS)
    assert np.array_equal(mean.cpu().numpy(), want_m)
    assert (np.abs(inv_std.cpu().numpy() - want_i) <= 2.0 ** -40 * want_i).all()
    want = H.instance_norm_ref(x, starts, w, b, EPS, act)
    exact = H.cancellation_exact(k, starts, base, w, b, EPS)
    if act == NONE:
        assert (np.abs(want - exact) <= H.norm_forward_bound(exact)).all()
    err, bound = np.abs(y.cpu().numpy().astype(np.float64) - want), H.norm_forward_bound(want)
    print(f"instance norm cancellation act={act}: max err / bound = {_ratio(err, bound):.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("act", [NONE, RELU, GELU])
def test_special_values_stay_in_their_frame_and_channel(gpu, act):
    """one NaN, one +inf and an +inf / -inf pair, each in one (frame, channel) of a three-frame input: exactly those columns of y
    and dx are NaN (under ReLU too: the kernel keeps NaN) and those channels of dweight; every other element keeps the bits of
    the run without them.  dbias = sum dy act'(pre) is NaN there exactly when act' is (GELU; ReLU' and 1 are finite at NaN),
    and equals the reference's NaN pattern."""
    import torch

    sizes = (70, 300, 41)
    x, starts, w, b = _case(sizes, 6, seed=act)
    dy = np.random.default_rng(9).standard_normal(x.shape).astype(np.float32)
    bad = x.copy()
    cells = {(0, 1): [(5, np.nan)], (1, 3): [(299, np.inf)], (2, 4): [(0, np.inf), (40, -np.inf)]}
    hit = np.zeros(x.shape, bool)
    for (f, c), puts in cells.items():
        for r, v in puts:
            bad[starts[f] + r, c] = v
        hit[starts[f]:starts[f + 1], c] = True
    chans = sorted({c for _, c in cells})
    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    st = t(starts)
    runs = []
    for data in (x, bad):
        y, mean, inv_std = H.gpu_instance_norm(t(data), st, t(w), t(b), EPS, act)
        dx, dw, db = H.gpu_instance_norm_backward(t(data), st, t(w), t(b), mean, inv_std, act, t(dy))
        runs.append([a.cpu().numpy() for a in (y, dx, dw, db, mean, inv_std)])
    (y0, dx0, dw0, db0, m0, i0), (y1, dx1, dw1, db1, m1, i1) = runs
    assert np.isfinite(y0).all() and np.isfinite(dx0).all()
    for clean, dirty in ((y0, y1), (dx0, dx1)):
        assert np.array_equal(np.isnan(dirty), hit) and np.array_equal(dirty[~hit], clean[~hit])
    others = [c for c in range(6) if c not in chans]
    assert np.isnan(dw1[chans]).all() and np.array_equal(dw1[others], dw0[others]) and np.array_equal(db1[others], db0[others])
    with np.errstate(invalid="ignore", over="ignore"):
        ref = H.instance_norm_backward_ref(bad, starts, w, b, m1, i1, act, dy)
    assert np.array_equal(np.isnan(db1), np.isnan(ref[2])) and np.array_equal(np.isnan(dw1), np.isnan(ref[1]))
    assert np.isnan(db1[chans]).all() == (act == GELU)
    for f, c in cells:
        assert np.isnan(m1[f, c]) or np.isinf(m1[f, c])
        assert np.isnan(i1[f, c])


def test_eps_zero_constant_channel(gpu):
    """eps = 0 on a constant channel: 0 * inf, NaN as in the reference; the other channels are the reference's"""
    import torch

    x, starts, w, b = _case((70, 300), 4, seed=3)
    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    y, mean, inv_std = H.gpu_instance_norm(t(x), t(starts), t(w), t(b), 0.0, NONE)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = H.instance_norm_ref(x, starts, w, b, 0.0, NONE)
    y = y.cpu().numpy().astype(np.float64)
    assert np.isnan(want[:, 0]).all() and np.array_equal(np.isnan(y), np.isnan(want)) and np.isinf(inv_std.cpu().numpy()[:, 0]).all()
    assert (np.abs(y - want)[:, 1:] <= H.norm_forward_bound(want)[:, 1:]).all()


BACKWARD_SIZES = {"255-0-256": (CHUNK - 1, 0, CHUNK), "257-773-1": (CHUNK + 1, 3 * CHUNK + 5, 1), "B37": None}


@pytest.mark.parametrize("act", [NONE, RELU, GELU])
@pytest.mark.parametrize("C", [1, 65])
@pytest.mark.parametrize("name", list(BACKWARD_SIZES))
def test_backward_at_the_derived_bound(gpu, name, C, act):
    """sv_instance_norm_backward directly, the constant channel (zero variance, inv_std = 1e4) of C = 65 included.  Kernel and
    reference take the reference's float64 mean / inv_std.  ReLU pre-activations are away from 0 except in the constant
    channel and in one-row frames, where xhat is exactly 0 on both sides and the pre-activation exactly `bias`."""
    import torch

    sizes = BACKWARD_SIZES[name] or _many_frames(37)
    x, starts, w, b = _case(sizes, C, seed=300 + C + 7 * act)
    dy = np.random.default_rng(C + act).standard_normal(x.shape).astype(np.float32)
    mean, inv_std = H.instance_norm_stats_ref(x, starts, EPS)
    if C > 1:
        assert np.allclose(inv_std[np.diff(starts) > 0, 0], 1e4) and (mean[np.diff(starts) > 0, 0] == 3.25).all()
    pre = H.instance_norm_ref(x, starts, w, b, EPS, NONE)
    one_row = np.repeat(np.diff(starts) == 1, np.diff(starts))
    free = pre[~one_row][:, min(C - 1, 1):]
    assert free.size == 0 or np.abs(free).min() > 1e-9
    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    args = (t(x), t(starts), t(w), t(b), t(mean), t(inv_std), act, t(dy))
    dx, dw, db = H.gpu_instance_norm_backward(*args)
    again = H.gpu_instance_norm_backward(*args)
    assert all(torch.equal(p, q) for p, q in zip((dx, dw, db), again))
    rdx, rdw, rdb, noise, nw, nb = H.instance_norm_backward_ref(x, starts, w, b, mean, inv_std, act, dy)
    ratios = {}
    for key, got, ref, n in (("dx", dx, rdx, noise), ("dweight", dw, rdw, nw), ("dbias", db, rdb, nb)):
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        bound = 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * n
        ok = bound > 0
        assert (err[~ok] == 0).all()
        ratios[key] = _ratio(err[ok], bound[ok])
    print(f"instance norm backward {name} C={C} act={act}: max err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
