"""sv_seg_criterion / sv_segment_topk and the Python layer over them (SegmentationCriterion, StepMetrics,
compute_accuracies, segment_topk_indices, get_pred_centers_batch, compute_center_dists_batch) on the GPU against the
float64 restatement of tests/seg_loss_helpers.py (pinned to torch on the CPU by tests/test_seg_loss_cpu.py).

Bounds.  The loss is one float32 rounding of a float64 value (the float64 reordering error, N * 2^-53 relative, is far
below it): |loss - ref| <= 2^-23 |ref|.  The gradient has two float32 roundings (the cast of softmax - onehot and the
product with the scale): |g - ref| <= 2^-22 |ref| elementwise, ignored rows exactly 0.  Counts, selections and
compute_accuracies are exact.  A centre and a distance are each one float32 rounding of a float64 value:
|v - ref| <= 2^-23 max(1, |ref|).  Logits are uniform in [-20, 20]: every softmax entry is at least e^-40 / 32, far above
float32's subnormals."""
import functools

import numpy as np
import pytest
import torch

import seg_loss_helpers as H

pytestmark = pytest.mark.gpu

# csrc/sv_seg_loss.hip: SEG_TILE = 256 rows per tile, SEG_MAX_GROUPS = 512 workgroups per launch.  One row more than a
# single launch wave of workgroups covers (512 * 256 + 1) gives 513 tiles: the first workgroups walk two tiles each, the
# partials of 257 workgroups meet in the cross-workgroup reduction, and the frame cuts below fall inside a workgroup's rows.
SEG_TILE, SEG_MAX_GROUPS = 256, 512
N_WAVE = SEG_TILE * SEG_MAX_GROUPS + 1
NS = [0, 1, 63, 64, 65, 257, 1000, N_WAVE]
# frame cuts: lengths 0 and 1, frames ending one row past a tile / workgroup boundary (257, 513, 300 * 256 + 1)
CUTS = [0, 0, 1, 2, 2, 63, 64, 65, 129, 257, 300, 513, 700, 900, 1000, SEG_TILE * 300 + 1]


def _offsets(N, B):
    return [min(c, N) for c in (CUTS[:B] if B > 3 else [0, 0, 257][:B])] + [N]


@functools.lru_cache(maxsize=4)
def _case(N, C, B):
    """seeded inputs and the restatement's results, computed once per shape and left unchanged"""
    rng = np.random.default_rng(1000 * C + B + N)
    x = rng.uniform(-20, 20, size=(N, C)).astype(np.float32)
    y = rng.integers(0, C, size=N)
    y[rng.uniform(size=N) < 0.25] = -100
    off = _offsets(N, B)
    cm, ign = H.confusion(x, y, off)
    ref = {"x": x, "y": y, "off": off, "cm": cm, "ign": ign,
           "loss": {r: H.loss(x, y, r) for r in ("mean", "sum")},
           "grad": {r: H.grad(x, y, r) for r in ("mean", "sum")}}
    for v in (x, y, cm, ign, *ref["grad"].values()):
        v.setflags(write=False)
    return ref


def _close(got, ref, rel, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN pattern differs"
    ok = ~np.isnan(ref)
    err = np.abs(got[ok] - ref[ok])
    bound = rel * np.abs(ref[ok])
    worst = float((err / np.maximum(np.abs(ref[ok]), 1e-300)).max()) if ok.any() else 0.0
    print(f"{what}: worst relative error {worst:.3e} (bound {rel:.3e})")
    assert (err <= bound).all(), f"{what}: worst relative error {worst:.3e} > {rel:.3e}"


def _logits(x, ld, gpu):
    """[N, C] view with row stride ld of a NaN-filled [N, ld] buffer: the padding must never be read"""
    buf = torch.full((x.shape[0], ld), float("nan"), dtype=torch.float32, device=gpu)
    buf[:, :x.shape[1]] = torch.tensor(x).to(gpu)  # a copy: the cached reference arrays are read-only
    return buf[:, :x.shape[1]]


def _run(crit, x, y, off, gpu):
    logits = x.detach().requires_grad_(True)
    loss, m = crit(logits, y, offsets=off, return_metrics=True)
    loss.backward()
    return loss.detach(), logits.grad, m


@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("C", [1, 2, 3, 10, 32])
@pytest.mark.parametrize("N", NS)
def test_criterion_against_the_restatement(gpu, N, C, pad, B):
    from mrcc_amd.utils.loss import SegmentationCriterion
    from mrcc_amd.utils.metrics import compute_accuracies

    ref = _case(N, C, B)
    x, y, off = _logits(ref["x"], C + pad, gpu), torch.tensor(ref["y"]).to(gpu), ref["off"]
    assert x.stride(0) == C + pad or N <= 1
    for reduction in ("mean", "sum"):
        crit = SegmentationCriterion(ignore_index=-100, reduction=reduction)
        loss, g, m = _run(crit, x, y, off, gpu)
        assert loss.dtype == torch.float32 and loss.dim() == 0 and g.shape == (N, C)
        _close(loss.cpu().numpy(), ref["loss"][reduction], 2.0 ** -23, f"loss {reduction}")
        g_host = g.cpu().numpy()
        _close(g_host, ref["grad"][reduction], 2.0 ** -22, f"gradient {reduction}")
        assert (g_host[ref["y"] == -100] == 0).all()
        # determinism: a second call gives the same bits
        loss2, g2, m2 = _run(crit, x, y, off, gpu)
        assert loss2.view(torch.int32).item() == loss.view(torch.int32).item()
        assert torch.equal(g2.view(torch.int32), g.view(torch.int32))
        assert torch.equal(m2.confusion, m.confusion) and torch.equal(m2.ignored, m.ignored)
    host = m.to_host()
    assert host["confusion"].dtype == np.int64 and np.array_equal(host["confusion"], ref["cm"])
    assert np.array_equal(host["rows"], np.diff(off)) and np.array_equal(host["ignored"], ref["ign"])
    assert host["invalid"] == 0
    # compute_accuracies: the reference's per-frame formula as exactly the same Python floats; an empty frame (where the
    # reference raises ZeroDivisionError) gives NaN
    others = [{"offset": (lo, hi)} for lo, hi in zip(off[:-1], off[1:])]
    acc = compute_accuracies(x, y, others)
    assert len(acc) == B and all(type(a) is float for a in acc)
    pred = H.argmax_rows(ref["x"])
    for b, (lo, hi) in enumerate(zip(off[:-1], off[1:])):
        if hi == lo:
            assert np.isnan(acc[b])
        else:
            assert acc[b] == float((pred[lo:hi] == ref["y"][lo:hi]).sum()) / (hi - lo)
    dev_acc = m.accuracies()
    assert dev_acc.dtype == torch.float64 and np.array_equal(dev_acc.cpu().numpy(), np.array(acc), equal_nan=True)


def test_inputs_the_python_layer_converts(gpu):
    """int32 labels; offsets as a device tensor, a host sequence and the collate's dicts; no offsets: one frame; a
    transposed (non-unit column stride) logits tensor is made contiguous"""
    from mrcc_amd.utils.loss import SegmentationCriterion

    ref = _case(1000, 3, 3)
    crit = SegmentationCriterion()
    x, y = torch.tensor(ref["x"]).to(gpu), torch.tensor(ref["y"]).to(gpu)
    want, gw, mw = _run(crit, x, y, ref["off"], gpu)
    others = [{"offset": (lo, hi)} for lo, hi in zip(ref["off"][:-1], ref["off"][1:])]
    xt = x.t().contiguous().t()
    assert xt.stride(1) != 1
    for xx, yy, off in ((x, y.to(torch.int32), torch.tensor(ref["off"], dtype=torch.int32, device=gpu)), (x, y, others),
                        (xt, y, tuple(ref["off"]))):
        loss, g, m = _run(crit, xx, yy, off, gpu)
        assert torch.equal(loss, want) and torch.equal(g, gw) and torch.equal(m.confusion, mw.confusion)
    logits = x.clone().requires_grad_(True)
    loss = crit(logits, y)
    assert torch.is_tensor(loss) and torch.equal(loss.detach(), want)
    loss, m = crit(x, y, return_metrics=True)
    assert m.confusion.shape == (1, 3, 3) and torch.equal(m.confusion[0], mw.confusion.sum(0))
    with pytest.raises(ValueError):
        crit(x, y, offsets=[0, 10, 999])


def test_argmax_ties_and_nan_rows(gpu):
    from mrcc_amd.utils.loss import SegmentationCriterion

    rng = np.random.default_rng(3)
    N, C = 300, 6
    x = rng.integers(-4, 5, size=(N, C)).astype(np.float32)  # small integers: most rows have equal maxima
    y = rng.integers(0, C, size=N)
    x[5, 2] = x[5, 4] = 9.0  # two equal maxima: column 2 wins
    x[7, 3] = x[7, 5] = np.nan  # the first NaN is the prediction; the loss is NaN
    x[270, 1] = np.nan
    y[[5, 7, 270]] = [2, 3, 0]
    off = [0, 100, 257, 300]
    pred = H.argmax_rows(x)
    assert pred[5] == 2 and pred[7] == 3 and pred[270] == 1 and ((x == x.max(1, keepdims=True)).sum(1) > 1).sum() > 50
    loss, g, m = _run(SegmentationCriterion(), torch.from_numpy(x).to(gpu), torch.from_numpy(y).to(gpu), off, gpu)
    assert np.isnan(float(loss)) and np.isnan(H.loss(x, y, "mean"))
    assert np.array_equal(m.to_host()["confusion"], H.confusion(x, y, off)[0])
    assert m.to_host()["confusion"][0, 3, 3] >= 1 and m.to_host()["confusion"][2, 0, 1] >= 1
    _close(g.cpu().numpy(), H.grad(x, y, "mean"), 2.0 ** -22, "gradient")
    assert np.isnan(g[7].cpu().numpy()).all()
    # without the NaN rows the loss is finite and within the bound
    keep = np.ones(N, bool)
    keep[[7, 270]] = False
    loss, _, _ = _run(SegmentationCriterion(), torch.from_numpy(x[keep]).to(gpu), torch.from_numpy(y[keep]).to(gpu), None, gpu)
    _close(float(loss), H.loss(x[keep], y[keep], "mean"), 2.0 ** -23, "loss")
    # a row that holds +inf gives NaN, as torch's log-softmax
    x[9, 0] = np.inf
    loss, _, _ = _run(SegmentationCriterion(reduction="sum"), torch.from_numpy(x[keep]).to(gpu),
                      torch.from_numpy(y[keep]).to(gpu), None, gpu)
    assert np.isnan(float(loss))


def test_all_rows_ignored(gpu):
    from mrcc_amd.utils.loss import SegmentationCriterion

    ref = _case(257, 3, 3)
    x, y = torch.tensor(ref["x"]).to(gpu), torch.full((257,), -100, dtype=torch.int64, device=gpu)
    loss, g, m = _run(SegmentationCriterion(reduction="mean"), x, y, ref["off"], gpu)
    assert np.isnan(float(loss)) and (g == 0).all()
    loss, g, m = _run(SegmentationCriterion(reduction="sum"), x, y, ref["off"], gpu)
    assert float(loss) == 0.0 and (g == 0).all()
    host = m.to_host()
    assert (host["confusion"] == 0).all() and np.array_equal(host["ignored"], host["rows"])


def test_one_invalid_label_is_counted_not_faulted(gpu):
    """label 7 with C = 3 is a value the API defines: the row is not counted, n_invalid = 1, the loss is NaN"""
    from mrcc_amd.utils.loss import SegmentationCriterion

    ref = _case(1000, 3, 3)
    x = torch.tensor(ref["x"]).to(gpu)
    y = ref["y"].copy()
    y[600] = 7  # frame 2 (rows 257 .. 999)
    loss, g, m = _run(SegmentationCriterion(), x, torch.from_numpy(y).to(gpu), ref["off"], gpu)
    host = m.to_host()
    assert host["invalid"] == 1 and np.isnan(float(loss))
    assert np.array_equal(host["confusion"][:2], ref["cm"][:2])
    assert np.array_equal(host["confusion"], H.confusion(ref["x"], y, ref["off"])[0])
    gh = g.cpu().numpy()
    assert np.isnan(gh[600]).all() and not np.isnan(np.delete(gh, 600, axis=0)).any()


def _vote_column(rng, N):
    col = rng.integers(-5, 6, size=N).astype(np.float32)  # repeated values
    for value, frac in ((np.inf, 0.02), (-np.inf, 0.02), (np.nan, 0.02)):
        col[rng.uniform(size=N) < frac] = value
    return col


@pytest.mark.parametrize("k", [1, 8, 64])
@pytest.mark.parametrize("N,B", [(0, 1), (1, 3), (65, 16), (1000, 16), (9000, 3), (N_WAVE, 16)])
def test_segment_topk(gpu, N, B, k):
    from mrcc_amd.utils.output import segment_topk_indices, topk_indices

    rng = np.random.default_rng(N + k)
    col = _vote_column(rng, N)
    off = _offsets(N, B)
    table = torch.full((N, 3), 7.0, dtype=torch.float32, device=gpu)
    table[:, 1] = torch.from_numpy(col).to(gpu)
    got = segment_topk_indices(table[:, 1], torch.tensor(off, dtype=torch.int32, device=gpu), k)  # stride 3
    assert got.dtype == torch.int64 and got.shape == (B, k)
    host = got.cpu().numpy()
    assert np.array_equal(host, H.segment_topk(col, off, k))
    for b, (lo, hi) in enumerate(zip(off[:-1], off[1:])):
        n = min(k, hi - lo)
        assert (host[b, n:] == -1).all()
        if hi > lo:
            assert np.array_equal(host[b, :n], topk_indices(table[lo:hi, 1], k).cpu().numpy())


def test_pred_centers_and_center_dists(gpu):
    from mrcc_amd.utils.metrics import compute_center_dists_batch
    from mrcc_amd.utils.output import get_pred_centers_batch

    rng = np.random.default_rng(11)
    off = [0, 5, 5, 400, 1000]  # fewer than 8 rows; empty; frame 3 without a label-1 row
    N, B, qs, ee_r = off[-1], 4, 0.02, 0.03
    out = rng.uniform(-20, 20, size=(N, 2)).astype(np.float32)
    out[rng.uniform(size=N) < 0.3, 1] = 3.0  # ties among the votes
    coords = np.concatenate([np.zeros((N, 1)), rng.integers(-200, 200, size=(N, 3))], 1).astype(np.int32)
    labels = rng.integers(0, 2, size=N)
    labels[400:] = 0
    poses = np.concatenate([rng.uniform(-1, 1, (B, 3)), rng.normal(size=(B, 4))], 1).astype(np.float32)
    d_out, d_coords = torch.from_numpy(out).to(gpu), torch.from_numpy(coords).to(gpu)
    d_off = torch.tensor(off, dtype=torch.int32, device=gpu)
    d_poses = torch.from_numpy(poses).to(gpu)
    for q in (None, d_poses[:, 3:7]):
        got = get_pred_centers_batch(d_out, d_coords, d_off, qs, ee_r=ee_r, q=q)
        assert got.dtype == torch.float32 and got.shape == (B, 3)
        want = H.pred_centers(out, coords, off, qs, ee_r, None if q is None else poses[:, 3:7])
        assert np.isnan(want[1]).all() and not np.isnan(want[[0, 2, 3]]).any()
        gh = got.cpu().numpy().astype(np.float64)
        assert np.array_equal(np.isnan(gh), np.isnan(want))
        ok = ~np.isnan(want)
        assert (np.abs(gh[ok] - want[ok]) <= 2.0 ** -23 * np.maximum(1.0, np.abs(want[ok]))).all()
    dist, valid = compute_center_dists_batch(d_out, torch.from_numpy(labels).to(gpu), d_coords, d_poses, off, qs, ee_r)
    want, want_valid = H.center_dists(out, labels, coords, poses, off, qs, ee_r)
    assert dist.dtype == torch.float32 and valid.dtype == torch.bool
    assert np.array_equal(valid.cpu().numpy(), want_valid) and list(want_valid) == [True, False, True, False]
    dh = dist.cpu().numpy().astype(np.float64)
    assert np.isnan(dh[1]) and np.isnan(want[1])
    ok = ~np.isnan(want)
    assert (np.abs(dh[ok] - want[ok]) <= 2.0 ** -23 * np.maximum(1.0, np.abs(want[ok]))).all()


def test_training_step_matches_torch_cross_entropy(gpu):
    """RobotNetSegmentation in train() mode, two frames of a few hundred voxels: one step with SegmentationCriterion and
    one from the same state with torch.nn.CrossEntropyLoss; parameter gradients agree within the bound of
    tests/test_gpu_training.py (REL_TOL there: max |got - want| <= 1e-4 max |want| per tensor)."""
    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd.model.robotnet_segmentation import RobotNetSegmentation
    from mrcc_amd.utils.loss import SegmentationCriterion

    REL_TOL = 1e-4
    torch.manual_seed(4)
    model = RobotNetSegmentation(in_channels=3, num_classes=3).to(gpu).train()
    rng = np.random.default_rng(4)
    clouds = [np.unique(rng.integers(-6, 6, size=(n, 3)), axis=0) for n in (400, 250)]
    coords = torch.from_numpy(np.concatenate([np.concatenate([np.full((len(c), 1), b), c], 1)
                                              for b, c in enumerate(clouds)])).int()
    feats = torch.from_numpy(rng.uniform(-0.5, 0.5, size=(len(coords), 3)).astype(np.float32))
    labels = rng.integers(0, 3, size=len(coords))
    labels[rng.uniform(size=len(coords)) < 0.25] = -100
    labels = torch.from_numpy(labels).to(gpu)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    grads, losses = [], []
    for crit in (SegmentationCriterion(ignore_index=-100), torch.nn.CrossEntropyLoss(ignore_index=-100)):
        model.load_state_dict(state)
        model.zero_grad(set_to_none=True)
        out = model(ME.SparseTensor(feats, coordinates=coords, device=gpu))
        assert 200 < out.F.shape[0] == len(coords)
        loss = crit(out.F, labels)
        loss.backward()
        losses.append(float(loss.detach()))
        grads.append({n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None})
    print(f"loss fused {losses[0]:.7g}, torch {losses[1]:.7g}")
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 10
    worst = 0.0
    for name, want in grads[1].items():
        rel = float((grads[0][name] - want).abs().max()) / max(float(want.abs().max()), 1e-30)
        worst = max(worst, rel)
        assert rel <= REL_TOL, f"{name}: rel {rel:.2e}"
    print(f"worst relative max-abs error of a parameter gradient {worst:.2e} (tolerance {REL_TOL:.0e})")
