"""float64 references of the metric-learning criterion (include/sv_hip.h N10), independent of csrc/sv_metric.hip:

  miner_ref      pytorch_metric_learning's MultiSimilarityMiner restated literally in numpy: the full similarity matrix, the
                 two copies with ignore values, a (stable) sort of every row, torch.where's row-major order
  miner_brute    the same set from the per-pair definition (the self-check of miner_ref)
  loss_ref       TripletMarginLoss with the library's defaults in torch float64 autograd: explicit normalisation, pairwise
                 L2 distance, convert_to_triplets, mean over the non-zero triplets
  miner_margins / loss_margin   how far every decision of a case is from its tipping point: a test asserts these on the
                 reference alone before it compares a kernel to it
The library itself is not available; these restate its published algorithm from memory.
"""
import numpy as np
import torch

SHAPES = [(1, 4), (2, 1), (3, 3), (64, 16), (65, 33), (257, 513)]
PATTERNS = ["equal", "distinct", "two", "many"]
NORM_EPS = 1e-12


def class_value(c):
    """class id -> label value: negative up to class 3, above 2^31 from class 5 on"""
    return np.asarray(c, dtype=np.int64) * (2**31 + 12345) - 2**33


def make_labels(B, pattern, rng):
    if pattern == "equal":
        c = np.full(B, 5)
    elif pattern == "distinct":
        c = rng.permutation(B)
    elif pattern == "two":
        c = rng.integers(0, 2, size=B) * 7  # classes 0 and 7: a negative label and one above 2^31
        c[0] = 0
        c[-1] = 7 if B > 1 else 0
    else:  # many classes, some of them singletons
        c = rng.integers(0, max(2, B // 5), size=B)
        c[: min(3, B)] = np.arange(B, B + min(3, B))
    return class_value(c)


SEEDS = {(64, 16, "many"): 1}  # seed 0 leaves two sort keys of one row 1.7e-10 apart (tests/test_featurenet_cpu.py checks)


def make_case(B, E, pattern, seed=None, pad=3):
    """(x float32 [B, E + pad] whose padding columns hold NaN, labels int64 [B]); the embedding is x[:, :E]"""
    seed = SEEDS.get((B, E, pattern), 0) if seed is None else seed
    rng = np.random.default_rng([seed, B, E, PATTERNS.index(pattern)])
    x = np.full((B, E + pad), np.nan, dtype=np.float32)
    x[:, :E] = rng.standard_normal((B, E)).astype(np.float32)
    return x, make_labels(B, pattern, rng)


def normalise(x):
    x = np.asarray(x, dtype=np.float64)
    return x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), NORM_EPS)


def similarity(x):
    """S = u u^T row by row with numpy's own summation (no BLAS): two bitwise equal rows give bitwise equal columns"""
    u = normalise(x)
    return np.stack([(u * u[i]).sum(1) for i in range(len(u))]) if len(u) else np.zeros((0, 0))


def finite_rows(x):
    return np.isfinite(np.asarray(x, dtype=np.float64)).all(1)


def _sorting_matrices(x, labels):
    """the library's mat_pos_sorting / mat_neg_sorting: +inf / -inf where a column is not a positive / negative of the row;
    a non-finite row is ignored as anchor and as partner (this repository's rule)"""
    ok = finite_rows(x)
    S = similarity(np.where(ok[:, None], x, 0.0))
    y = np.asarray(labels)
    same = y[:, None] == y[None, :]
    live = ok[:, None] & ok[None, :]
    is_pos = same & ~np.eye(len(y), dtype=bool) & live
    is_neg = ~same & live
    return np.where(is_pos, S, np.inf), np.where(is_neg, S, -np.inf), is_pos, is_neg


def miner_ref(x, labels, epsilon):
    """-> (a1, p, a2, n) int64 in the library's order"""
    mat_pos, mat_neg, is_pos, is_neg = _sorting_matrices(x, labels)
    empty = np.zeros(0, dtype=np.int64)
    if not is_pos.any() or not is_neg.any():
        return empty, empty, empty, empty
    pos_idx = np.argsort(mat_pos, axis=1, kind="stable")
    neg_idx = np.argsort(mat_neg, axis=1, kind="stable")
    pos_sorted = np.take_along_axis(mat_pos, pos_idx, 1)
    neg_sorted = np.take_along_axis(mat_neg, neg_idx, 1)
    with np.errstate(invalid="ignore"):
        hard_pos = np.where(pos_sorted - epsilon < neg_sorted[:, -1:])
        hard_neg = np.where(neg_sorted + epsilon > pos_sorted[:, :1])
    a1, a2 = hard_pos[0], hard_neg[0]
    return (a1.astype(np.int64), pos_idx[a1, hard_pos[1]].astype(np.int64), a2.astype(np.int64),
            neg_idx[a2, hard_neg[1]].astype(np.int64))


def miner_brute(x, labels, epsilon):
    """the per-pair definition: sets of (anchor, partner)"""
    ok = finite_rows(x)
    S = similarity(np.where(ok[:, None], x, 0.0))
    B = len(labels)
    pos, neg = set(), set()
    for i in range(B):
        if not ok[i]:
            continue
        P = [j for j in range(B) if j != i and ok[j] and labels[j] == labels[i]]
        N = [j for j in range(B) if ok[j] and labels[j] != labels[i]]
        maxneg = max((S[i, j] for j in N), default=-np.inf)
        minpos = min((S[i, j] for j in P), default=np.inf)
        pos |= {(i, j) for j in P if S[i, j] - epsilon < maxneg}
        neg |= {(i, j) for j in N if S[i, j] + epsilon > minpos}
    return pos, neg


def miner_margins(x, labels, epsilon, duplicates=(), tied_rows=()):
    """(smallest |S - eps - maxneg| or |S + eps - minpos| over all pairs, smallest gap between adjacent sort keys of a row);
    `duplicates`: groups of rows that are bitwise equal on purpose - equal keys between their columns are not counted;
    `tied_rows`: anchors whose keys are equal on purpose (a zero row: S = 0 exactly) - their gaps are not counted"""
    mat_pos, mat_neg, is_pos, is_neg = _sorting_matrices(x, labels)
    group = np.arange(len(labels))
    for g in duplicates:
        group[list(g)] = min(g)
    decision, gap = np.inf, np.inf
    for mat, mask, sign in ((mat_pos, is_pos, -1.0), (mat_neg, is_neg, 1.0)):
        other = mat_neg.max(1) if sign < 0 else mat_pos.min(1)
        for i in range(len(labels)):
            cols = np.nonzero(mask[i])[0]
            if len(cols) == 0:
                continue
            v = mat[i, cols]
            if np.isfinite(other[i]):
                decision = min(decision, np.abs(v + sign * epsilon - other[i]).min())
            if i in tied_rows:
                continue
            order = np.argsort(v, kind="stable")
            d = np.diff(v[order])
            meant = group[cols[order]][1:] == group[cols[order]][:-1]
            if (~meant).any():
                gap = min(gap, d[~meant].min())
    return decision, gap


def _valid(a, b, B):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    keep = (a >= 0) & (a < B) & (b >= 0) & (b < B)
    return a[keep], b[keep], int((~keep).sum())


def distances(x):
    """(D [B, B] torch float64 with a graph to xt, xt): explicit normalisation and pairwise L2; d = 0 has gradient 0"""
    xt = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    u = xt / xt.norm(dim=1, keepdim=True).clamp_min(NORM_EPS)
    sq = ((u[:, None, :] - u[None, :, :]) ** 2).sum(-1)
    zero = sq == 0
    return torch.where(zero, torch.zeros_like(sq), torch.sqrt(torch.where(zero, torch.ones_like(sq), sq))), xt


def loss_ref(x, indices_tuple, margin):
    """-> dict(sum, nonzero, n_triplets, n_invalid, loss, grad_sum [B, E] = d sum / d x, margin = the smallest
    |d_ap - d_an + margin| over the triplets).  convert_to_triplets is the library's (a1[:, None] == a2) while that matrix
    is small, and the same triplets anchor by anchor otherwise."""
    B = len(x)
    a1, p, bad_p = _valid(indices_tuple[0], indices_tuple[1], B)
    a2, n, bad_n = _valid(indices_tuple[2], indices_tuple[3], B)
    D, xt = distances(x)
    if len(a1) * len(a2) <= 4_000_000:
        pi, ni = np.where(a1[:, None] == a2[None, :])
        viol = [D[a1[pi], p[pi]] - D[a2[ni], n[ni]] + margin]
    else:
        viol = []
        for a in np.unique(a1):
            ps, ns = p[a1 == a], n[a2 == a]
            if len(ns):
                viol.append((D[a, ps][:, None] - D[a, ns][None, :] + margin).reshape(-1))
    viol = torch.cat(viol) if viol else torch.zeros(0, dtype=torch.float64)
    losses = torch.relu(viol)
    total = losses.sum()
    grad = torch.zeros_like(xt)
    if viol.numel():
        (grad,) = torch.autograd.grad(total, xt)
    nonzero, total = int((losses > 0).sum()), float(total.detach())
    return dict(sum=total, nonzero=nonzero, n_triplets=int(viol.numel()), n_invalid=bad_p + bad_n,
                loss=total / nonzero if nonzero else 0.0, grad_sum=grad.numpy(),
                margin=float(viol.detach().abs().min()) if viol.numel() else np.inf)


def all_pairs(labels):
    """get_all_pairs_indices: every (anchor, positive) and (anchor, negative) the labels allow"""
    y = np.asarray(labels)
    same = y[:, None] == y[None, :]
    a1, p = np.where(same & ~np.eye(len(y), dtype=bool))
    a2, n = np.where(~same)
    return a1.astype(np.int64), p.astype(np.int64), a2.astype(np.int64), n.astype(np.int64)


def grad_bound(want):
    """one float32 ulp of the reference value plus 1e-12 of the largest gradient entry"""
    want = np.asarray(want, dtype=np.float64)
    return np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 1e-12 * (np.abs(want).max() if want.size else 0.0)


def sums_close(got, want):
    return abs(got - want) <= 1e-12 * max(1.0, abs(want))
