"""sv_seg_criterion and sv_segment_topk at frame counts up to the documented limit (B <= 1024) against the float64
restatement of tests/seg_loss_helpers.py, with the bounds of tests/test_gpu_seg_loss.py unchanged: loss within 2^-23 and
gradient within 2^-22 relative, confusion [B][C][C], ignored counts, compute_accuracies and the top-k selections exact.

seg_criterion_kernel finds a row's frame by a binary search over `offsets` and keeps the confusion counts of a tile's
first frame in the workgroup; a row of a later frame inside the tile adds straight to global memory.  tests/
test_gpu_seg_loss.py stops at B = 16, where that branch fires now and then.  Here N = 3000 rows are cut into 63, 64, 65
and 1024 frames (four to eight frames per 256-row tile, at 1024 some sixty), with an empty first frame, an empty last
frame and a run of ten empty frames in between."""
import functools

import numpy as np
import pytest
import torch

import seg_loss_helpers as H
from test_gpu_seg_loss import _close, _logits, _run, _vote_column

pytestmark = pytest.mark.gpu

BS = [63, 64, 65, 1024]
N_ROWS = 3000


def _cuts(rng, N, B):
    """offsets [B + 1] from 0 to N: frames 0, B - 1 and 20 .. 29 empty, the N rows dealt to the others by seeded weights
    (a multinomial draw: at B = 1024 it leaves further empty frames of its own)"""
    lens = np.zeros(B, np.int64)
    full = np.ones(B, bool)
    full[[0, B - 1]] = False
    full[20:30] = False
    w = rng.exponential(size=int(full.sum()))
    lens[full] = rng.multinomial(N, w / w.sum())
    return [0] + np.cumsum(lens).tolist()


@functools.lru_cache(maxsize=None)
def _case(C, B):
    """seeded inputs and the restatement's results, computed once per shape and left unchanged"""
    rng = np.random.default_rng(31 * C + B)
    N = N_ROWS
    x = rng.uniform(-20, 20, size=(N, C)).astype(np.float32)
    y = rng.integers(0, C, size=N)
    y[rng.uniform(size=N) < 0.1] = -100
    off = _cuts(rng, N, B)
    cm, ign = H.confusion(x, y, off)
    ref = {"x": x, "y": y, "off": off, "cm": cm, "ign": ign,
           "loss": {r: H.loss(x, y, r) for r in ("mean", "sum")},
           "grad": {r: H.grad(x, y, r) for r in ("mean", "sum")}}
    for v in (x, y, cm, ign, *ref["grad"].values()):
        v.setflags(write=False)
    return ref


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("C", [3, 32])
def test_criterion_at_frame_counts(gpu, C, pad, B):
    from mrcc_amd.utils.loss import SegmentationCriterion
    from mrcc_amd.utils.metrics import compute_accuracies

    ref = _case(C, B)
    N, off = N_ROWS, ref["off"]
    lens = np.diff(off)
    assert len(off) == B + 1 and off[-1] == N and lens[0] == 0 and lens[-1] == 0 and (lens[20:30] == 0).all()
    tiles = [len(set(np.searchsorted(off, np.arange(t, min(t + 256, N)), side="right"))) for t in range(0, N, 256)]
    assert min(tiles) >= 2 and np.median(tiles) >= max(4, B // 20), f"frames with rows in each 256-row tile: {tiles}"
    x, y = _logits(ref["x"], C + pad, gpu), torch.tensor(ref["y"]).to(gpu)
    assert x.stride(0) == C + pad
    for reduction in ("mean", "sum"):
        crit = SegmentationCriterion(ignore_index=-100, reduction=reduction)
        loss, g, m = _run(crit, x, y, off, gpu)
        assert loss.dtype == torch.float32 and loss.dim() == 0 and g.shape == (N, C)
        _close(loss.cpu().numpy(), ref["loss"][reduction], 2.0 ** -23, f"loss {reduction}")
        g_host = g.cpu().numpy()
        _close(g_host, ref["grad"][reduction], 2.0 ** -22, f"gradient {reduction}")
        assert (g_host[ref["y"] == -100] == 0).all()
        loss2, g2, m2 = _run(crit, x, y, off, gpu)  # a second call gives the same bits
        assert loss2.view(torch.int32).item() == loss.view(torch.int32).item()
        assert torch.equal(g2.view(torch.int32), g.view(torch.int32))
        assert torch.equal(m2.confusion, m.confusion) and torch.equal(m2.ignored, m.ignored)
        host = m.to_host()
        assert host["confusion"].shape == (B, C, C) and np.array_equal(host["confusion"], ref["cm"])
        assert np.array_equal(host["rows"], lens) and np.array_equal(host["ignored"], ref["ign"])
        assert host["invalid"] == 0
    others = [{"offset": (lo, hi)} for lo, hi in zip(off[:-1], off[1:])]
    acc = compute_accuracies(x, y, others)
    assert len(acc) == B and all(type(a) is float for a in acc)
    pred = H.argmax_rows(ref["x"])
    for b, (lo, hi) in enumerate(zip(off[:-1], off[1:])):
        if hi == lo:
            assert np.isnan(acc[b]), b
        else:
            assert acc[b] == float((pred[lo:hi] == ref["y"][lo:hi]).sum()) / (hi - lo), b
    dev_acc = m.accuracies()
    assert dev_acc.dtype == torch.float64 and np.array_equal(dev_acc.cpu().numpy(), np.array(acc), equal_nan=True)


@pytest.mark.parametrize("k", [1, 8, 64])
@pytest.mark.parametrize("B", BS)
def test_segment_topk_at_frame_counts(gpu, B, k):
    """frame lengths turn through empty, exactly k, k - 1, 1, k + 1, 3 k + 5, empty, empty, 130: frames shorter than k
    (padded with -1), of exactly k rows, longer ones, and runs of empty frames, the first frame among them"""
    from mrcc_amd.utils.output import segment_topk_indices

    cycle = [0, k, k - 1, 1, k + 1, 3 * k + 5, 0, 0, 130]
    lens = [cycle[b % len(cycle)] for b in range(B)]
    lens[-1] = 0
    off = [0] + np.cumsum(lens).tolist()
    N = off[-1]
    col = _vote_column(np.random.default_rng(B + k), N)
    table = torch.full((N, 3), 7.0, dtype=torch.float32, device=gpu)
    table[:, 1] = torch.from_numpy(col).to(gpu)
    got = segment_topk_indices(table[:, 1], torch.tensor(off, dtype=torch.int32, device=gpu), k)  # stride 3
    assert got.dtype == torch.int64 and got.shape == (B, k)
    host = got.cpu().numpy()
    assert np.array_equal(host, H.segment_topk(col, off, k))
    for b, n in enumerate(lens):
        assert (host[b, min(k, n):] == -1).all() and (host[b, :min(k, n)] >= 0).all(), b
