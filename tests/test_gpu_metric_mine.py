"""sv_ms_mine against the literal numpy restatement of MultiSimilarityMiner (tests/metric_helpers.py): the integer
outputs must be equal, so every test first asserts on the reference alone that each decision (hard or not, and the order of
two sort keys) clears float64 rounding by far: margins above 1e-9 against about (E + 4) 2^-53."""
import numpy as np
import pytest
import torch

import metric_helpers as MH

pytestmark = pytest.mark.gpu


def mine(gpu, x, E, labels, epsilon, max_pos=-1, max_neg=-1):
    """x [B, >= E] on the host: the kernel sees the column view x[:, :E] (ld > E, whatever the padding holds).
    -> ([a1, p, a2, n] up to the kept counts, counts, n_nonfinite)"""
    from mrcc_amd.utils import metric_learning as ML

    xt = torch.from_numpy(np.ascontiguousarray(x)).to(gpu)[:, :E]
    a1, p, a2, n, counts, nonfinite = ML.mine_call(xt, torch.from_numpy(labels).to(gpu), epsilon, max_pos, max_neg)
    c = counts.tolist()
    return [t[:k].cpu().numpy() for t, k in zip((a1, p, a2, n), (c[0], c[0], c[1], c[1]))], c, int(nonfinite)


def check(gpu, x, E, labels, epsilon, nonfinite=0, **margin_kw):
    decision, gap = MH.miner_margins(x[:, :E], labels, epsilon, **margin_kw)
    assert decision > 1e-9 and gap > 1e-9, (decision, gap)
    want = MH.miner_ref(x[:, :E], labels, epsilon)
    got, counts, bad = mine(gpu, x, E, labels, epsilon)
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and np.array_equal(g, w)
    assert counts == [len(want[0]), len(want[2]), len(want[0]), len(want[2])] and bad == nonfinite
    return want


@pytest.mark.parametrize("pattern", MH.PATTERNS)
@pytest.mark.parametrize("B,E", MH.SHAPES)
def test_matches_the_reference(gpu, B, E, pattern):
    x, y = MH.make_case(B, E, pattern)
    assert x.shape[1] > E and np.isnan(x[:, E:]).all()
    if B > 4 and pattern in ("two", "many"):
        assert (y < 0).any() and (y > 2**31).any()
    want = check(gpu, x, E, y, 0.1)
    if pattern in ("equal", "distinct"):  # no negative pair at all / no positive pair at all: the early return
        assert len(want[0]) == len(want[2]) == 0
    elif B >= 64:
        assert len(want[0]) > 0 and len(want[2]) > 0


@pytest.mark.parametrize("labels", ["int32", "uint8", "int16"])
def test_labels_of_any_integer_dtype(gpu, labels):
    from mrcc_amd.utils import metric_learning as ML

    x, _ = MH.make_case(65, 33, "many")
    y = (np.arange(65) % 7).astype(labels)
    want = MH.miner_ref(x[:, :33], y.astype(np.int64), 0.1)
    got = ML.MultiSimilarityMiner(epsilon=0.1)(torch.from_numpy(x).to(gpu)[:, :33], torch.from_numpy(y).to(gpu))
    assert [tuple(t.shape) for t in got] == [(len(w),) for w in want]  # exact lengths
    for g, w in zip(got, want):
        assert g.dtype == torch.int64 and np.array_equal(g.cpu().numpy(), w)


def test_bitwise_duplicate_rows_tie_to_the_lower_column(gpu):
    x, y = MH.make_case(65, 33, "two")
    x[11], y[11] = x[2], y[2]  # a duplicate among the positives of label y[2] and among the negatives of the other label
    x[40], x[20] = x[3], x[3]
    y[40], y[20] = y[3], y[3]
    want = check(gpu, x, 33, y, 0.1, duplicates=[(2, 11), (3, 20, 40)])
    S = MH.similarity(x[:, :33])
    ties = 0
    for a, b in ((want[0], want[1]), (want[2], want[3])):
        same = (a[1:] == a[:-1]) & (S[a[1:], b[1:]] == S[a[:-1], b[:-1]])
        assert (b[1:][same] > b[:-1][same]).all()
        ties += int(same.sum())
    assert ties > 20  # the order of equal keys was decided many times


def test_zero_row_takes_the_clamp(gpu):
    x, y = MH.make_case(65, 33, "two")
    x[5, :33] = 0.0  # u = 0 / 1e-12 = 0: S = 0 with every row; its own row is all ties, ordered by column
    decision, gap = MH.miner_margins(x[:, :33], y, 0.1, tied_rows=(5,))
    assert decision > 1e-9 and gap > 1e-9
    want = MH.miner_ref(x[:, :33], y, 0.1)
    got, counts, bad = mine(gpu, x, 33, y, 0.1)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and bad == 0
    assert (want[0] == 5).any() or (want[2] == 5).any()


def test_nonfinite_rows_join_no_pair_and_leave_the_others_alone(gpu):
    x, y = MH.make_case(65, 33, "many")
    x[7, 1] = np.nan
    x[9, 0] = np.inf
    x[30, 32] = -np.inf
    want = check(gpu, x, 33, y, 0.1, nonfinite=3)
    assert not np.isin(np.concatenate(want), (7, 9, 30)).any()
    keep = np.array([i for i in range(65) if i not in (7, 9, 30)])
    got, _, bad = mine(gpu, x[keep], 33, y[keep], 0.1)  # the same batch without those rows
    assert bad == 0 and all(np.array_equal(keep[g], w) for g, w in zip(got, want))


@pytest.mark.parametrize("pattern", ["two", "many"])
def test_epsilon_zero_and_three(gpu, pattern):
    x, y = MH.make_case(65, 33, pattern)
    loose = check(gpu, x, 33, y, 3.0)
    tight = check(gpu, x, 33, y, 0.0)
    every = MH.all_pairs(y)
    has_neg, has_pos = np.isin(every[0], every[2]), np.isin(every[2], every[0])
    assert len(loose[0]) == has_neg.sum() and len(loose[2]) == has_pos.sum()  # every pair of an anchor with both kinds
    assert 0 < len(tight[0]) < len(loose[0]) and 0 < len(tight[2]) < len(loose[2])


def test_caps_keep_the_first_pairs(gpu):
    x, y = MH.make_case(64, 16, "two")
    want = MH.miner_ref(x[:, :16], y, 0.1)
    assert min(MH.miner_margins(x[:, :16], y, 0.1)) > 1e-9
    tp, tn = len(want[0]), len(want[2])
    assert tp > 1 and tn > 1 and tp != tn
    for cp, cn in ((0, tn + 1), (1, tn), (tp, 1), (tp + 1, 0), (-1, 5), (7, -1)):
        got, counts, _ = mine(gpu, x, 16, y, 0.1, cp, cn)
        kp, kn = (tp if cp < 0 else min(tp, cp)), (tn if cn < 0 else min(tn, cn))
        assert counts == [kp, kn, tp, tn], (cp, cn, counts)
        for g, w, k in zip(got, want, (kp, kp, kn, kn)):
            assert np.array_equal(g, w[:k])


def test_two_calls_give_the_same_bits(gpu):
    x, y = MH.make_case(257, 513, "many")
    a, ca, _ = mine(gpu, x, 513, y, 0.1)
    b, cb, _ = mine(gpu, x, 513, y, 0.1)
    assert ca == cb and all(np.array_equal(u, v) for u, v in zip(a, b))
