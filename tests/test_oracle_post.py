"""The C oracle's global pooling and slice + argmax against torch on the CPU (no GPU needed).

The GPU tests compare the kernels with this oracle bit for bit, so its NaN, inf and tie semantics must be torch's:
torch.amax propagates NaN, and `logits.max(1)` (utils/output.py:67-73) takes the first maximum of a row, where the first
NaN beats any number."""
import numpy as np
import torch

U = 2.0 ** -24


def _pool_case(seed):
    rng = np.random.default_rng(seed)
    counts = [0, 1, 2, 5, 64, 0, 300, 3, 0]
    coords = np.zeros((sum(counts), 4), np.int32)
    coords[:, 0] = np.repeat(np.arange(len(counts)), counts)
    x = rng.standard_normal((len(coords), 7)).astype(np.float32)
    starts = np.concatenate([[0], np.cumsum(counts)])
    nan, inf = np.float32("nan"), np.float32("inf")
    x[starts[1], 0] = nan  # the only row of batch 1
    x[starts[2] + 1, 1] = nan  # the second of two rows
    x[starts[4] + 40, 2] = nan  # inside 64 rows, with +inf before it
    x[starts[4] + 3, 2] = inf
    x[starts[6]:starts[7], 3] = -inf  # a whole column -inf
    x[starts[6] + 5, 4] = inf  # +inf with -inf: max +inf, mean NaN
    x[starts[6] + 9, 4] = -inf
    x[starts[3]:starts[4], 5] = 1.5  # ties
    return x, coords, counts, starts


def test_oracle_global_pool_matches_torch(oracle):
    x, coords, counts, starts = _pool_case(0)
    B = len(counts)
    mx = oracle.global_pool(x, coords, oracle.POOL_MAX, B)
    av = oracle.global_pool(x, coords, oracle.POOL_AVG, B)
    t = torch.from_numpy(x)
    for b, n in enumerate(counts):
        s, e = starts[b], starts[b + 1]
        if n == 0:
            assert (mx[b] == 0).all() and (av[b] == 0).all()
            continue
        want = torch.amax(t[s:e], 0).numpy()
        assert np.array_equal(mx[b], want, equal_nan=True), f"batch {b}: {mx[b]} vs torch.amax {want}"
        xd = t[s:e].double()
        mean = xd.mean(0).numpy()
        fin = np.isfinite(mean)
        assert np.array_equal(av[b][~fin], mean[~fin].astype(np.float32), equal_nan=True)
        bound = (n + 1) * U * xd.abs().sum(0).numpy() / n  # sequential float32 sum, then one division
        assert (np.abs(av[b][fin] - mean[fin]) <= bound[fin]).all()
    assert np.isnan(mx[1, 0]) and np.isnan(mx[2, 1]) and np.isnan(mx[4, 2]) and mx[6, 4] == np.inf and np.isnan(av[6, 4])


def test_oracle_slice_argmax_matches_torch_max(oracle):
    nan, inf = float("nan"), float("inf")
    rows = torch.tensor([
        [1.0, nan, 2.0, 0.0],  # NaN outside column 0 ...
        [nan, 5.0, 1.0, 0.0],
        [3.0, 3.0, 1.0, 0.0],  # ... and a tie
        [0.0, 1.0, nan, nan],  # two NaNs: the first
        [-inf, inf, 2.0, inf],  # two +inf: the first
        [-inf, -inf, -inf, -inf],  # all -inf: column 0
        [-inf, inf, -inf, nan],  # +inf before a NaN: the NaN
        [0.5, 0.5, 0.5, 0.5],
        [-1.0, -2.0, -3.0, 7.0],
    ])
    g = torch.Generator().manual_seed(3)
    ties = torch.randint(-1, 2, (200, 4), generator=g).float()
    F = torch.cat([rows, ties])
    inverse = torch.cat([torch.arange(len(F)), torch.randint(0, len(F), (500,), generator=g)])
    label, conf = oracle.slice_argmax(F.numpy(), inverse.numpy())
    want_v, want_i = F[inverse].max(1)
    assert np.array_equal(label, want_i.numpy()), f"rows {inverse[np.flatnonzero(label != want_i.numpy())[:6]].tolist()}"
    assert list(label[:3]) == [1, 0, 0]
    assert np.array_equal(np.isnan(conf), torch.isnan(want_v).numpy())
    fin = ~torch.isnan(want_v)
    assert np.abs(conf[fin.numpy()] - torch.sigmoid(want_v[fin].double()).numpy()).max() <= 2.5e-7
    one_col = oracle.slice_argmax(np.array([[nan], [2.0], [-inf]], np.float32), np.array([0, 1, 2]))
    assert list(one_col[0]) == [0, 0, 0] and np.isnan(one_col[1][0]) and one_col[1][2] == 0.0

