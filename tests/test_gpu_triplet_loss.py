"""sv_triplet_margin and sv_mined_triplet_step against the float64 torch-autograd restatement of TripletMarginLoss
(tests/metric_helpers.py): sums within 1e-12 max(1, |value|); the float32 gradient within one float32 ulp of the reference
value plus 1e-12 of the largest entry; the triplet counts exactly, after asserting on the reference alone that no triplet
is within 1e-9 of the hinge."""
import numpy as np
import pytest
import torch

import hostile_helpers as HH
import metric_helpers as MH

pytestmark = pytest.mark.gpu
MARGIN = 0.05
EMPTY = tuple(np.zeros(0, dtype=np.int64) for _ in range(4))


def on_gpu(gpu, x, E):
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu)[:, :E]  # a column view: ld > E


def loss_call(gpu, x, E, tup, margin=MARGIN):
    """-> (sums [2], grad float64 [B, E] of the kernel's float32, n_triplets, n_invalid, raw grad tensor)"""
    from mrcc_amd.utils import metric_learning as ML

    counts = torch.tensor([len(tup[0]), len(tup[2])], dtype=torch.int64, device=gpu)
    sums, grad, n_triplets, n_invalid = ML.triplet_call(on_gpu(gpu, x, E), *[torch.from_numpy(t).to(gpu) for t in tup], counts,
                                                        margin)
    return sums.tolist(), grad.double().cpu().numpy(), int(n_triplets), int(n_invalid), grad


def check(gpu, x, E, tup, margin=MARGIN, invalid=0):
    ref = MH.loss_ref(x[:, :E], tup, margin)
    assert ref["margin"] > 1e-9, ref["margin"]
    sums, grad, n_triplets, n_invalid, _ = loss_call(gpu, x, E, tup, margin)
    print(f"sum {sums[0]!r} want {ref['sum']!r}; nonzero {sums[1]} of {n_triplets}; "
          f"grad err {np.abs(grad - ref['grad_sum']).max():.3e} of {np.abs(ref['grad_sum']).max():.3e}")
    assert MH.sums_close(sums[0], ref["sum"]), (sums[0], ref["sum"])
    assert sums[1] == ref["nonzero"] and n_triplets == ref["n_triplets"] and n_invalid == ref["n_invalid"] == invalid
    assert np.isfinite(grad).all() and (np.abs(grad - ref["grad_sum"]) <= MH.grad_bound(ref["grad_sum"])).all()
    return ref, sums, grad


@pytest.mark.parametrize("pairs", ["mined", "all"])
@pytest.mark.parametrize("pattern", MH.PATTERNS)
@pytest.mark.parametrize("B,E", MH.SHAPES)
def test_matches_the_reference(gpu, B, E, pattern, pairs):
    x, y = MH.make_case(B, E, pattern)
    tup = MH.miner_ref(x[:, :E], y, 0.1) if pairs == "mined" else MH.all_pairs(y)
    ref, sums, grad = check(gpu, x, E, tup)
    if B >= 64 and pattern in ("two", "many"):
        assert 0 < ref["nonzero"] < ref["n_triplets"] and np.abs(grad).max() > 0
    if pattern in ("equal", "distinct"):
        assert ref["n_triplets"] == 0 and sums == [0.0, 0.0] and not grad.any()


def test_module_and_backward(gpu):
    from mrcc_amd.utils import metric_learning as ML

    x, y = MH.make_case(65, 33, "many")
    tup = MH.miner_ref(x[:, :33], y, 0.1)
    ref = MH.loss_ref(x[:, :33], tup, MARGIN)
    for given in (tup, None):  # None: every triplet the labels allow
        want = ref if given is not None else MH.loss_ref(x[:, :33], MH.all_pairs(y), MARGIN)
        xt = on_gpu(gpu, x, 33).clone().requires_grad_(True)
        indices = None if given is None else tuple(torch.from_numpy(t).to(gpu) for t in given)
        loss = ML.TripletMarginLoss(margin=MARGIN)(xt, torch.from_numpy(y.astype(np.int64)).to(gpu), indices)
        assert loss.dtype == torch.float32 and loss.dim() == 0 and abs(float(loss.detach()) - want["loss"]) <= 1e-6 * want["loss"]
        (2.0 * loss).backward()
        g = 2.0 * want["grad_sum"] / want["nonzero"]
        assert np.abs(xt.grad.double().cpu().numpy() - g).max() <= 1e-6 * np.abs(g).max()


def test_empty_tuple_is_exactly_zero(gpu):
    x, _ = MH.make_case(65, 33, "two")
    sums, grad, n_triplets, n_invalid, _ = loss_call(gpu, x, 33, EMPTY)
    assert sums == [0.0, 0.0] and n_triplets == 0 and n_invalid == 0 and not grad.any()
    pos_only = MH.all_pairs(MH.make_case(65, 33, "two")[1])[:2] + EMPTY[:2]
    sums, grad, n_triplets, _, _ = loss_call(gpu, x, 33, pos_only)
    assert sums == [0.0, 0.0] and n_triplets == 0 and not grad.any()


def test_no_violation_is_exactly_zero(gpu):
    x, y = MH.make_case(65, 33, "two")
    tup = MH.all_pairs(y)
    sums, grad, n_triplets, _, _ = loss_call(gpu, x, 33, tup, margin=-10.0)
    assert sums == [0.0, 0.0] and n_triplets == MH.loss_ref(x[:, :33], tup, -10.0)["n_triplets"] > 0 and not grad.any()


def test_a_pair_given_twice_counts_twice(gpu):
    x, y = MH.make_case(65, 33, "many")
    a1, p, a2, n = MH.miner_ref(x[:, :33], y, 0.1)
    once, _, _ = check(gpu, x, 33, (a1, p, a2, n))
    twice = (np.append(a1, a1[:3]), np.append(p, p[:3]), np.concatenate([a2[-2:], a2, a2[-2:]]), np.concatenate([n[-2:], n, n[-2:]]))
    ref, _, _ = check(gpu, x, 33, twice)
    assert ref["n_triplets"] > once["n_triplets"] and ref["sum"] > once["sum"]


def test_zero_distance_has_zero_subgradient(gpu):
    x, y = MH.make_case(65, 33, "two")
    x[11], y[11] = x[2], y[2]  # d(2, 11) = 0: a positive pair at distance 0, which violates the margin
    x[20], y[20] = x[3], y[3] + 1  # a class of its own: (3, 20) is a negative pair at distance 0
    tup = MH.all_pairs(y)
    ref, _, grad = check(gpu, x, 33, tup)
    D, _ = MH.distances(x[:, :33])
    assert float(D[2, 11].detach()) == 0.0 and float(D[3, 20].detach()) == 0.0 and ref["nonzero"] > 0
    alone = (np.array([2]), np.array([11]), np.array([2, 2]), np.array([2, 11]))  # d_ap = d_an = 0: loss = margin, gradient 0
    sums, g, n_triplets, _, _ = loss_call(gpu, x, 33, alone)
    assert sums == [2 * MARGIN, 2.0] and n_triplets == 2 and not g.any()


def test_out_of_range_indices_are_skipped_and_counted(gpu):
    x, y = MH.make_case(65, 33, "many")
    a1, p, a2, n = MH.miner_ref(x[:, :33], y, 0.1)
    clean, sums0, grad0 = check(gpu, x, 33, (a1, p, a2, n))
    dirty = (np.concatenate([[65], a1, [0]]), np.concatenate([[0], p, [-1]]), np.append(a2, [2**40, 3]), np.append(n, [1, -2**40]))
    ref, sums, grad = check(gpu, x, 33, dirty, invalid=4)
    assert sums == sums0 and np.array_equal(grad, grad0)  # the valid pairs are the same multiset: the same bits


def test_permuted_tuple_and_repeated_call(gpu):
    x, y = MH.make_case(257, 513, "many")
    tup = MH.miner_ref(x[:, :513], y, 0.1)
    ref, sums, grad = check(gpu, x, 513, tup)
    rng = np.random.default_rng(5)
    pp, pn = rng.permutation(len(tup[0])), rng.permutation(len(tup[2]))
    check(gpu, x, 513, (tup[0][pp], tup[1][pp], tup[2][pn], tup[3][pn]))
    again = loss_call(gpu, x, 513, tup)
    assert again[0] == sums and np.array_equal(again[1], grad)


@pytest.mark.parametrize("B,E,pattern,cap", [(65, 33, "many", 40), (65, 33, "two", -1), (257, 513, "many", 1000), (3, 3, "two", 0),
                                             (1, 4, "equal", 5)])
def test_fused_step_is_bit_equal_to_mine_truncate_loss(gpu, B, E, pattern, cap):
    from mrcc_amd.utils import metric_learning as ML

    x, y = MH.make_case(B, E, pattern)
    xt, yt = on_gpu(gpu, x, E), torch.from_numpy(y).to(gpu)
    a1, p, a2, n, counts, nonfinite = ML.mine_call(xt, yt, 0.1, cap, cap)
    kp, kn = counts[:2].tolist()
    composed = ML.triplet_call(xt, a1[:kp], p[:kp], a2[:kn], n[:kn], counts, MARGIN)
    fused = ML.mined_step_call(xt, yt, cap, 0.1, MARGIN)
    HH.assert_same_bits((composed[0], composed[1], counts, composed[2], nonfinite), fused, f"fused step {B} x {E} {pattern}")
    want = MH.miner_ref(x[:, :E], y, 0.1)
    lens = [len(w) if cap < 0 else min(cap, len(w)) for w in (want[0], want[2])]
    assert [kp, kn] == lens
    ref = MH.loss_ref(x[:, :E], (want[0][:kp], want[1][:kp], want[2][:kn], want[3][:kn]), MARGIN)
    assert MH.sums_close(float(fused[0][0]), ref["sum"]) and float(fused[0][1]) == ref["nonzero"] and int(fused[3]) == ref["n_triplets"]


def test_mined_triplet_loss_is_one_entry_call_and_waits_for_nothing(gpu):
    from mrcc_amd.utils import metric_learning as ML

    x, y = MH.make_case(65, 33, "many")
    want = MH.miner_ref(x[:, :33], y, 0.1)
    ref = MH.loss_ref(x[:, :33], tuple(w[:40] for w in want), MARGIN)
    xt = on_gpu(gpu, x, 33).clone().requires_grad_(True)
    yt = torch.from_numpy(y.astype(np.int32) % 1000).to(gpu)  # int32, as the YCB collate delivers; the same classes
    assert len(np.unique(y.astype(np.int32) % 1000)) == len(np.unique(y))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # any synchronising call of torch raises from here on
    try:
        with HH.entry_calls() as calls:
            loss, stats = ML.mined_triplet_loss(xt, yt, 40, return_stats=True)
            loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    launched = {k: v for k, v in calls.items() if v and k in HH.launching_entries(calls)}
    assert launched == {"sv_mined_triplet_step": 1}, launched
    assert abs(float(loss) - ref["loss"]) <= 1e-6 * ref["loss"] and stats["counts"].tolist()[:2] == [40, 40]
    g = ref["grad_sum"] / ref["nonzero"]
    got = xt.grad.double().cpu().numpy()
    assert np.isfinite(got).all() and got.any() and np.abs(got - g).max() <= 1e-6 * np.abs(g).max()


def test_nonfinite_embedding_gives_nan_loss(gpu):
    from mrcc_amd.utils import metric_learning as ML

    x, y = MH.make_case(65, 33, "many")
    x[7, 1] = np.nan
    loss, stats = ML.mined_triplet_loss(on_gpu(gpu, x, 33), torch.from_numpy(y).to(gpu), 40, return_stats=True)
    assert np.isnan(float(loss)) and int(stats["n_nonfinite"]) == 1
