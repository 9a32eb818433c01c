"""The criterion of the feature-extractor trainers (train_feature-extractor.py:65-81 in the reference):
pytorch_metric_learning's MultiSimilarityMiner and TripletMarginLoss with their defaults, on the N10 entries of
include/sv_hip.h (csrc/sv_metric.hip).

    miner = MultiSimilarityMiner(epsilon=0.1);   a1, p, a2, n = miner(embeddings, labels)
    loss_func = TripletMarginLoss(margin=0.05);  loss = loss_func(embeddings, labels, (a1, p, a2, n))
    loss = mined_triplet_loss(embeddings, labels, max_pairs)      # mine, truncate, loss: one call, no host wait

The two classes keep the library's call shapes, so the miner returns tensors of exact length and reads four integers back
for that.  The trainer's step - mine, keep the first batch_size * max_pair pairs of each list, shuffle them, loss - is
mined_triplet_loss: the shuffle does not change the set of triplets, so the value is the same and nothing waits.
The semantics are the library's published algorithm restated from memory; the library is not available here, so parity
with it is by construction and unverified.  Embeddings live on the GPU: there is no CPU path.
"""
from ctypes import c_double, c_int, c_int64, c_size_t

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from .._lib import call, ptr, require_cuda, stream_ptr

ALL_PAIRS_EPSILON = 4.0  # |S| <= 1 up to rounding: with epsilon > 2 every pair of an anchor that has both kinds is hard


def _embeddings(x):
    """float32 [B, E] rows with unit column stride (a column view of a wider tensor is fine) -> (tensor, row stride)"""
    require_cuda(x, "embeddings")
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"embeddings must be [B, E] with B, E >= 1 (got {tuple(x.shape)})")
    if x.shape[0] > _lib.SV_MAX_BATCH:
        raise ValueError(f"at most {_lib.SV_MAX_BATCH} embeddings per call (got {x.shape[0]})")
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.float()
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    return x, x.stride(0)


def _labels(labels, B, dev):
    labels = torch.as_tensor(labels)
    if labels.is_floating_point() or labels.dtype == torch.bool or labels.numel() != B:
        raise ValueError(f"labels must be {B} integers (got {labels.dtype}, {tuple(labels.shape)})")
    return labels.reshape(B).to(device=dev, dtype=torch.int64).contiguous()


def _workspace(B, E, dev):
    nbytes = _lib.load().sv_metric_workspace_bytes(B, E)
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def mine_call(embeddings, labels, epsilon, max_pos=-1, max_neg=-1):
    """One sv_ms_mine call: (a1, p, a2, n int64 buffers of capacity min(B (B - 1), max_*), counts int64 [4] = kept
    positives, kept negatives, hard positives, hard negatives, n_nonfinite int32 [1]), all on the device; the buffers are
    defined up to the kept counts only.  No host wait."""
    x, ld = _embeddings(embeddings)
    B, E = x.shape
    y = _labels(labels, B, x.device)
    cap = [B * (B - 1) if m < 0 else min(B * (B - 1), int(m)) for m in (max_pos, max_neg)]
    lists = [torch.empty(c, dtype=torch.int64, device=x.device) for c in (cap[0], cap[0], cap[1], cap[1])]
    counts = torch.empty(4, dtype=torch.int64, device=x.device)
    nonfinite = torch.empty(1, dtype=torch.int32, device=x.device)
    ws, nbytes = _workspace(B, E, x.device)
    call("sv_ms_mine", ptr(x), c_int64(ld), c_int(B), c_int(E), ptr(y), c_double(epsilon), c_int64(max_pos), c_int64(max_neg),
         ptr(ws), c_size_t(nbytes), ptr(lists[0]), ptr(lists[1]), c_int64(cap[0]), ptr(lists[2]), ptr(lists[3]), c_int64(cap[1]),
         ptr(counts), ptr(nonfinite), stream_ptr())
    return lists[0], lists[1], lists[2], lists[3], counts, nonfinite


def triplet_call(embeddings, a1, p, a2, n, counts, margin, want_grad=True):
    """One sv_triplet_margin call on pair lists whose lengths are counts[0] / counts[1] on the device (at most the lists'
    sizes): (sums float64 [2], grad float32 [B, E] or None, n_triplets int64 [1], n_invalid int32 [1]).  No host wait."""
    x, ld = _embeddings(embeddings)
    B, E = x.shape
    dev = x.device
    idx = [torch.as_tensor(t).to(device=dev, dtype=torch.int64).reshape(-1).contiguous() for t in (a1, p, a2, n)]
    if idx[0].numel() != idx[1].numel() or idx[2].numel() != idx[3].numel():
        raise ValueError("indices_tuple: a1 / p and a2 / n must pair up")
    sums = torch.empty(2, dtype=torch.float64, device=dev)
    grad = torch.empty((B, E), dtype=torch.float32, device=dev) if want_grad else None
    n_triplets = torch.empty(1, dtype=torch.int64, device=dev)
    n_invalid = torch.empty(1, dtype=torch.int32, device=dev)
    ws, nbytes = _workspace(B, E, dev)
    call("sv_triplet_margin", ptr(x), c_int64(ld), c_int(B), c_int(E), ptr(idx[0]), ptr(idx[1]), c_int64(idx[0].numel()),
         ptr(idx[2]), ptr(idx[3]), c_int64(idx[2].numel()), ptr(counts), c_double(margin), ptr(ws), c_size_t(nbytes), ptr(sums),
         ptr(grad), ptr(n_triplets), ptr(n_invalid), stream_ptr())
    return sums, grad, n_triplets, n_invalid


def mined_step_call(embeddings, labels, max_pairs, epsilon, margin, want_grad=True):
    """One sv_mined_triplet_step call: (sums, grad or None, counts int64 [4], n_triplets int64 [1], n_nonfinite int32 [1]).
    No host wait."""
    x, ld = _embeddings(embeddings)
    B, E = x.shape
    dev = x.device
    y = _labels(labels, B, dev)
    sums = torch.empty(2, dtype=torch.float64, device=dev)
    grad = torch.empty((B, E), dtype=torch.float32, device=dev) if want_grad else None
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    n_triplets = torch.empty(1, dtype=torch.int64, device=dev)
    nonfinite = torch.empty(1, dtype=torch.int32, device=dev)
    ws, nbytes = _workspace(B, E, dev)
    call("sv_mined_triplet_step", ptr(x), c_int64(ld), c_int(B), c_int(E), ptr(y), c_double(epsilon), c_double(margin),
         c_int64(max_pairs), c_int64(max_pairs), ptr(ws), c_size_t(nbytes), ptr(sums), ptr(grad), ptr(counts), ptr(n_triplets),
         ptr(nonfinite), stream_ptr())
    return sums, grad, counts, n_triplets, nonfinite


def _reduce(sums, spoiled):
    """AvgNonZeroReducer: sums[0] / sums[1], 0 without a violating triplet; NaN where `spoiled` (a device flag) is set"""
    loss = torch.where(sums[1] > 0, sums[0] / sums[1].clamp(min=1.0), torch.zeros_like(sums[0]))
    return torch.where(spoiled, torch.full_like(loss, float("nan")), loss).to(torch.float32)


def _scaled(grad, sums, dloss, dtype):
    factor = dloss.to(torch.float64) / sums[1].clamp(min=1.0)
    return (grad * factor.to(torch.float32)).to(dtype)


class TripletLossFunction(torch.autograd.Function):
    """loss = mean over the violating triplets of max(d_ap - d_an + margin, 0).  The call also writes the unscaled gradient,
    which the backward divides by the number of violating triplets; the indices carry no gradient."""

    @staticmethod
    def forward(ctx, embeddings, a1, p, a2, n, counts, nonfinite, margin):
        want = ctx.needs_input_grad[0]
        sums, grad, _, n_invalid = triplet_call(embeddings, a1, p, a2, n, counts, margin, want)
        spoiled = n_invalid[0] != 0
        if nonfinite is not None:
            spoiled = spoiled | (nonfinite[0] != 0)
        ctx.in_dtype = embeddings.dtype
        if want:
            ctx.save_for_backward(grad, sums)
        return _reduce(sums, spoiled)

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss):
        if not ctx.needs_input_grad[0]:
            return (None,) * 8
        grad, sums = ctx.saved_tensors
        return (_scaled(grad, sums, dloss, ctx.in_dtype),) + (None,) * 7


class MinedTripletLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, embeddings, labels, max_pairs, epsilon, margin):
        want = ctx.needs_input_grad[0]
        sums, grad, counts, n_triplets, nonfinite = mined_step_call(embeddings, labels, max_pairs, epsilon, margin, want)
        ctx.in_dtype = embeddings.dtype
        if want:
            ctx.save_for_backward(grad, sums)
        ctx.mark_non_differentiable(counts, n_triplets, nonfinite)
        return _reduce(sums, nonfinite[0] != 0), counts, n_triplets, nonfinite

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss, *_):
        if not ctx.needs_input_grad[0]:
            return (None,) * 5
        grad, sums = ctx.saved_tensors
        return (_scaled(grad, sums, dloss, ctx.in_dtype),) + (None,) * 4


class MultiSimilarityMiner:
    """miners.MultiSimilarityMiner(epsilon) with the library's default CosineSimilarity.
    miner(embeddings, labels) -> (a1, p, a2, n): int64 tensors of exact length, anchors ascending and each anchor's pairs in
    ascending similarity (equal similarities by column).  Reads the two lengths back: one host wait."""

    def __init__(self, epsilon=0.1):
        self.epsilon = float(epsilon)

    def __call__(self, embeddings, labels):
        a1, p, a2, n, counts, _ = mine_call(embeddings, labels, self.epsilon)
        n_pos, n_neg = counts[:2].tolist()
        return a1[:n_pos], p[:n_pos], a2[:n_neg], n[:n_neg]


class TripletMarginLoss(torch.nn.Module):
    """losses.TripletMarginLoss(margin) with the library's defaults: L2 distance of the normalised embeddings, every triplet
    of the tuple, the mean over the triplets that violate the margin (0 when none does).
    loss(embeddings, labels, indices_tuple=None): without a tuple every triplet the labels allow.  An index outside the
    batch, or a non-finite embedding when the pairs come from the labels, gives NaN."""

    def __init__(self, margin=0.05):
        super().__init__()
        self.margin = float(margin)

    def forward(self, embeddings, labels, indices_tuple=None):
        if indices_tuple is None:
            a1, p, a2, n, counts, nonfinite = mine_call(embeddings, labels, ALL_PAIRS_EPSILON)
        else:
            if len(indices_tuple) != 4:
                raise ValueError("indices_tuple: (a1, p, a2, n); triplet tuples are not supported")
            a1, p, a2, n = indices_tuple
            counts = torch.tensor([len(a1), len(a2)], dtype=torch.int64).to(embeddings.device, non_blocking=True)
            nonfinite = None
        return TripletLossFunction.apply(embeddings, a1, p, a2, n, counts, nonfinite, self.margin)


def mined_triplet_loss(embeddings, labels, max_pairs, epsilon=0.1, margin=0.05, return_stats=False):
    """The feature-extractor trainers' criterion in one call: MultiSimilarityMiner(epsilon), the first max_pairs pairs of
    each list (max_pairs = batch_size * max_pair in the trainer; -1: all), TripletMarginLoss(margin).  0-dim float32 loss
    with a backward; NaN when an embedding is not finite.  No host wait.
    return_stats=True: (loss, {"counts": int64 [4] kept / hard pairs, "n_triplets": int64 [1], "n_nonfinite": int32 [1]})."""
    loss, counts, n_triplets, nonfinite = MinedTripletLossFunction.apply(embeddings, labels, int(max_pairs), float(epsilon),
                                                                         float(margin))
    if return_stats:
        return loss, {"counts": counts, "n_triplets": n_triplets, "n_nonfinite": nonfinite}
    return loss
