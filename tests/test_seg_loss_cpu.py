"""The segmentation criterion and step metrics without a GPU: the float64 restatement of tests/seg_loss_helpers.py pinned
to torch on the CPU and to this repository's confusion metrics; the four N7 symbols declared, exported and bound; the host
argument checks of sv_seg_criterion / sv_segment_topk (each returns -1 with a message before any HIP call); the
ValueError / SvHipError paths of the Python layer."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_loss_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N7 = ["sv_seg_criterion", "sv_seg_criterion_workspace_bytes", "sv_segment_topk", "sv_segment_topk_workspace_bytes"]


def _case(seed, N, C, lo=-20.0, hi=20.0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(lo, hi, size=(N, C))
    y = rng.integers(0, C, size=N)
    y[rng.uniform(size=N) < 0.25] = -100
    return x, y


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("N,C", [(1, 1), (7, 2), (65, 3), (300, 10), (129, 32)])
def test_restatement_matches_torch_cross_entropy(N, C, reduction):
    x, y = _case(N * 37 + C, N, C)
    y[0] = 0  # at least one counted row
    xt = torch.from_numpy(x).requires_grad_(True)
    want = F.cross_entropy(xt, torch.from_numpy(y), ignore_index=-100, reduction=reduction)
    want.backward()
    assert abs(H.loss(x, y, reduction) - float(want.detach())) <= 1e-12
    assert np.abs(H.grad(x, y, reduction) - xt.grad.numpy()).max() <= 1e-12
    assert (H.grad(x, y, reduction)[y == -100] == 0).all()


def test_restatement_edge_rows_match_torch():
    x, y = _case(5, 12, 3)
    y[:] = [0, 1, 2] * 4
    x[2, 1] = np.nan
    x[5, 0] = np.inf
    want = F.cross_entropy(torch.from_numpy(x), torch.from_numpy(y), reduction="none").numpy()
    got = H.row_losses(x, y)
    assert np.isnan(got[2]) and np.isnan(got[5]) and np.isnan(want[2]) and np.isnan(want[5])
    keep = ~np.isnan(want)
    assert keep.sum() == 10 and np.abs(got[keep] - want[keep]).max() <= 1e-12
    # no counted row: mean is NaN, sum is 0, as torch
    none = np.full(12, -100)
    for reduction in ("mean", "sum"):
        t = float(F.cross_entropy(torch.from_numpy(x[:, :2]), torch.from_numpy(none), reduction=reduction))
        h = H.loss(x[:, :2], none, reduction)
        assert (np.isnan(t) and np.isnan(h)) or t == h == 0.0
    assert np.isnan(H.loss(x, np.array([7] + [0] * 11), "mean")) and H.n_invalid(np.array([7, -100, 0, 3]), 3) == 2
    assert np.isnan(H.grad_unscaled(x, np.array([7] + [0] * 11))[0]).all()


def test_restatement_selections_match_torch():
    rng = np.random.default_rng(2)
    x = rng.integers(-3, 4, size=(400, 5)).astype(np.float32)  # many ties
    x[rng.uniform(size=x.shape) < 0.03] = np.nan
    x[rng.uniform(size=x.shape) < 0.03] = np.inf
    x[rng.uniform(size=x.shape) < 0.03] = -np.inf
    assert np.array_equal(H.argmax_rows(x), torch.from_numpy(x).max(1)[1].numpy())
    for col in (x[:, 0], x[:5, 1], x[:0, 2]):
        order = torch.from_numpy(col.copy()).sort(descending=True, stable=True)[1].numpy()
        for k in (1, 8, 64):
            got = H.topk_rows(col, k)
            assert np.array_equal(got[:min(k, len(col))], order[:k]) and (got[len(col):] == -1).all()
    offsets = [0, 0, 1, 130, 400]
    got = H.segment_topk(x[:, 3], offsets, 8)
    assert got.shape == (4, 8) and (got[0] == -1).all() and got[1, 0] == 0 and (got[1, 1:] == -1).all()


def test_restatement_confusion_matches_this_repositorys_metrics():
    import mrcc_amd  # noqa: F401
    from mrcc_amd.utils import metrics as M

    x, y = _case(9, 500, 3)
    offsets = [0, 200, 200, 500]
    cm, ign = H.confusion(x, y, offsets)
    pred = H.argmax_rows(x)
    for b in range(3):
        lo, hi = offsets[b], offsets[b + 1]
        assert np.array_equal(cm[b], M.confusion_matrix(pred[lo:hi], y[lo:hi], 3))
        assert ign[b] == (y[lo:hi] == -100).sum()
    acc = H.accuracies(x, y, [0, 200, 500])
    assert acc == [float(np.trace(c)) / n for c, n in ((cm[0], 200), (cm[2], 300))]
    # the batch form of the confusion metrics, and compute_segmentation_metrics on the counted rows
    got = M.segmentation_metrics_batch(cm)
    keep = y != -100
    total = M.segmentation_metrics_from_confusion(M.confusion_matrix(pred[keep], y[keep], 3))
    for key, want in total.items():
        assert np.array_equal(got["total"][key], want, equal_nan=True)
    for b in range(3):
        want = M.segmentation_metrics_from_confusion(cm[b])
        assert all(np.array_equal(got["frames"][b][k], want[k], equal_nan=True) for k in want)
    full = M.compute_segmentation_metrics(y[keep], pred[keep])
    tot = cm.sum(0)
    for ci, name in enumerate(("background", "arm", "ee")):
        tp, fp, fn = tot[ci, ci], tot[:, ci].sum() - tot[ci, ci], tot[ci].sum() - tot[ci, ci]
        assert full["class_results"][name]["precision"] == (1 if fp == 0 else tp / (tp + fp))
        assert full["class_results"][name]["recall"] == (1 if fn == 0 else tp / (tp + fn))
    assert full["miou"] == pytest.approx(total["miou"], abs=1e-15)


def test_symbols_declared_exported_and_bound():
    import mrcc_amd

    text = open(os.path.join(ROOT, "include", "sv_hip.h")).read()
    assert "N7" in text and "segmentation criterion and step metrics" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = mrcc_amd._lib.load()
    for name in N7:
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in include/sv_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in mrcc_amd._lib.SIGNATURES
    assert lib.sv_abi_version() == 4
    assert lib.sv_seg_criterion_workspace_bytes(0, 1, 1) > 0
    assert lib.sv_seg_criterion_workspace_bytes(10**6, 16, 3) >= 16
    assert lib.sv_segment_topk_workspace_bytes(10**5, 16, 8) >= 25 * 16 * 8 * 8


def test_host_argument_checks_reach_no_device():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    p = ctypes.c_void_p(256)  # never dereferenced: every call below fails its host checks
    big = ctypes.c_size_t(1 << 20)

    def crit(logits=p, ld=3, C=3, N=10, labels=p, offsets=p, B=2, ws=p, ws_bytes=big, sums=p, n_invalid=p):
        rc = lib.sv_seg_criterion(logits, ld, C, N, labels, -100, offsets, B, ws, ws_bytes, sums, None, None, None,
                                  n_invalid, None)
        return rc, lib.sv_last_error()

    def topk(x=p, ld=1, N=10, offsets=p, B=2, k=8, ws=p, ws_bytes=big, idx=p):
        rc = lib.sv_segment_topk(x, ld, N, offsets, B, k, ws, ws_bytes, idx, None)
        return rc, lib.sv_last_error()

    for kw, msg in (({"logits": None}, b"null pointer"), ({"labels": None}, b"null pointer"),
                    ({"offsets": None}, b"null pointer"), ({"ws": None}, b"null pointer"), ({"sums": None}, b"null pointer"),
                    ({"n_invalid": None}, b"null pointer"), ({"C": 0}, b"1 <= C <= 32"), ({"C": 33, "ld": 33}, b"1 <= C <= 32"),
                    ({"ld": 2}, b"ld >= C"), ({"B": 0}, b"1 to 1024 frames"), ({"B": 1025}, b"1 to 1024 frames"),
                    ({"N": -1}, b"0 <= N")):
        rc, err = crit(**kw)
        assert rc == -1 and msg in err and b"sv_seg_criterion" in err, (kw, rc, err)
    rc, err = crit(ws_bytes=ctypes.c_size_t(8))
    assert rc == -1 and b"workspace too small" in err
    for kw, msg in (({"x": None}, b"null pointer"), ({"offsets": None}, b"null pointer"), ({"ws": None}, b"null pointer"),
                    ({"idx": None}, b"null pointer"), ({"k": 0}, b"1 <= k <= 64"), ({"k": 65}, b"1 <= k <= 64"),
                    ({"B": 0}, b"1 to 1024 frames"), ({"B": 1025}, b"1 to 1024 frames"), ({"N": -1}, b"0 <= N"),
                    ({"ld": 0}, b"ld >= 1")):
        rc, err = topk(**kw)
        assert rc == -1 and msg in err and b"sv_segment_topk" in err, (kw, rc, err)
    rc, err = topk(ws_bytes=ctypes.c_size_t(8))
    assert rc == -1 and b"workspace too small" in err


def test_python_layer_refuses_what_it_does_not_support():
    import mrcc_amd
    from mrcc_amd._lib import SvHipError
    from mrcc_amd.model.robotnet_vote import get_criterion
    from mrcc_amd.utils import metrics as M
    from mrcc_amd.utils import output as O
    from mrcc_amd.utils.loss import SegmentationCriterion

    with pytest.raises(ValueError):
        SegmentationCriterion(reduction="none")
    crit = SegmentationCriterion(ignore_index=-100, reduction="mean")
    x, y = torch.zeros(4, 3, requires_grad=True), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(SvHipError):
        crit(x, y)
    with pytest.raises(SvHipError):
        crit(x, y, offsets=[0, 4], return_metrics=True)
    with pytest.raises(SvHipError):
        M.compute_accuracies(x, y, [{"offset": (0, 4)}])
    with pytest.raises(SvHipError):
        O.segment_topk_indices(x[:, 0], torch.tensor([0, 4], dtype=torch.int32), 8)
    with pytest.raises(SvHipError):
        O.get_pred_centers_batch(x, torch.zeros(4, 4), torch.tensor([0, 4], dtype=torch.int32), 0.02)
    with pytest.raises(SvHipError):
        M.compute_center_dists_batch(x, y, torch.zeros(4, 4), torch.zeros(1, 7), [0, 4], 0.02, 0.03)
    # the default criterion of the vote model is unchanged; fused=True is the same configuration on the new module
    assert type(get_criterion()) is torch.nn.CrossEntropyLoss
    fused = get_criterion(fused=True)
    assert isinstance(fused, SegmentationCriterion)
    assert (fused.ignore_index, fused.reduction) == (get_criterion().ignore_index, get_criterion().reduction)
