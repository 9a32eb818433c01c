"""sv_ee_mask, sv_key_points, sv_line_topk and sv_radius_labels at the limits their entry points document (B <= 1024 frames,
count <= 1024, K <= 64) against the numpy restatement of tests/label_helpers.py, through _run_batch / _check_batch of
tests/test_gpu_labels.py with that file's bounds unchanged: masks, indices, labels, votes and n_sel exact; key points
within 1e-12; cross-section distances within 1e-7 (float32 input) or 1e-12 (float64 input).

What the sizes are for.  ee_mask_kernel, line_dist_kernel and radius_labels_kernel find a row's frame by a binary search
over `offsets`: the frame lengths cycle through 0, 1, 63, 64, 65, 0, 0, 255, 256, 257, 3, so a batch opens with an empty
frame, holds runs of empty frames, and a 64-lane wave or a 256-row workgroup spans several frames (at B = 1024, where the
lengths stay at 64 rows or below, dozens).  line_topk_kernel runs `count` rounds of a block arg-min and pads the rest of a
row with a 256-thread stride loop: counts 255, 256, 257 and 1024 give that loop 0 to 3 trips after a frame that runs out.
sv_radius_labels walks K classes from the highest down: K = 1 and K = 64 are its two ends."""
import functools

import numpy as np
import pytest
import torch

import label_helpers as H
from test_gpu_labels import IGNORE, _bits, _check_batch, _D, _run_batch

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 63, 64, 65, 0, 0, 255, 256, 257, 3]
BS = [1, 2, 63, 64, 65, 1024]


@functools.lru_cache(maxsize=None)
def _batch(B):
    """(frames float32, poses [B, 7]): frame b is the first LENGTHS[b mod 11] rows of a gripper cloud of its own, posed by
    a pose of its own.  B = 1024 keeps the lengths of at most 64 rows (0, 1, 63, 64, 0, 0, 3) on clouds of 80 rows, so that
    the restatement of a thousand frames stays fast."""
    rng = np.random.default_rng(7000 + B)
    lengths = LENGTHS if B < 1024 else [n for n in LENGTHS if n <= 64]
    body = (160, 20, 60) if B < 1024 else (40, 10, 20)  # 280 / 80 rows per cloud
    frames, poses = [], []
    for b in range(B):
        p, pose, _ = H.gripper_cloud(rng, body[0], n_rod=body[1], n_bg=body[2])
        p = p[: lengths[b % len(lengths)]]
        p.setflags(write=False)
        frames.append(p)
        poses.append(pose)
    return tuple(frames), np.stack(poses)


def _same_bits(a, b):
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])) if a[k].dtype == np.float64 else np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("B", BS)
def test_frame_counts_against_restatement(gpu, B):
    frames, poses = _batch(B)
    got = _run_batch(list(frames), poses, gpu)
    _check_batch(frames, poses, got)
    if B >= 63:  # the batch is not a trivial one: rows inside the box, frames with key points, cross-sections
        assert got["mask"].sum() > B and (got["idx10"] != IGNORE).any(1).sum() > B // 4 and got["n_sel"].sum() > B
    _same_bits(got, _run_batch(list(frames), poses, gpu))  # two identical calls give identical bits


@pytest.mark.parametrize("B", [65, 1024])
def test_first_and_last_frame_empty(gpu, B):
    """the batch ends in an empty frame (the last offsets repeat N) and opens with one (as built it does already)"""
    frames, poses = _batch(B)
    assert len(frames[-1]) > 0
    cut = [frames[0][:0]] + list(frames[1:-1]) + [frames[-1][:0]]
    got = _run_batch(cut, poses, gpu)
    _check_batch(cut, poses, got)
    assert got["n_sel"][0] == 0 and got["n_sel"][-1] == 0


def test_frame_counts_float64(gpu):
    frames, poses = _batch(65)
    frames = [f.astype(np.float64) for f in frames]
    got = _run_batch(frames, poses, gpu)
    _check_batch(frames, poses, got)
    _same_bits(got, _run_batch(frames, poses, gpu))


def test_ee_crop_batch_of_65_frames(gpu):
    D = _D()
    frames, poses = _batch(65)
    pts, _, _, off, kept = D.ee_crop_batch([f.copy() for f in frames], None, None, poses)
    ref = [H.ee_idx(p, pose) for p, pose in zip(frames, poses)]
    counts = [len(r) for r in ref]
    assert sum(counts) > 65 and 0 in counts
    assert off.dtype == torch.int32 and off.cpu().tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert len(kept) == 65
    for b, (k, r) in enumerate(zip(kept, ref)):
        assert k.dtype == torch.int64 and np.array_equal(k.cpu().numpy(), r), b
    assert np.array_equal(pts.cpu().numpy(), np.concatenate([p[r] for p, r in zip(frames, ref)]))


@functools.lru_cache(maxsize=None)
def _topk_frames():
    """1100 rows that fill every count (six of them exact copies of the six rows nearest the line, one NaN row), 300 rows
    that run out, an empty frame"""
    rng = np.random.default_rng(77)
    long, pose0, _ = H.gripper_cloud(rng, 600, n_rod=50, n_bg=375)
    long = long[:1100].copy()
    order = H.cross_section(long, pose0, 1100, 10.0)[1]
    near, far = order[:6], order[-6:]
    long[far] = long[near]
    long[order[500], 1] = np.nan
    short, pose1, _ = H.gripper_cloud(rng, 600, n_rod=50, n_bg=375)
    _, pose2, _ = H.gripper_cloud(rng, 10)
    frames = (long, short[:300].copy(), short[:0].copy())
    for f in frames:
        f.setflags(write=False)
    return frames, np.stack([pose0, pose1, pose2]), (near, far, int(order[500]))


@pytest.mark.parametrize("count", [255, 256, 257, 1024])
def test_line_topk_counts(gpu, count):
    """the cutoff (an argument) is 10 m: every finite distance qualifies, so a frame's rounds end only at `count` or when
    its rows run out"""
    frames, poses, (near, far, nan_row) = _topk_frames()
    got = _run_batch(list(frames), poses, gpu, count=count, cutoff=10.0)
    _check_batch(frames, poses, got, count=count, cutoff=10.0)
    assert got["cs"].shape == (3, count) and got["n_sel"].tolist() == [count, min(count, 300), 0]
    assert (got["cs"][2] == -1).all() and np.isinf(got["dist"][2]).all()
    sel, dist = got["cs"][0], got["dist"][0]
    assert nan_row not in sel and np.all(np.diff(dist) >= 0)
    # the twelve nearest rows are six pairs of equal distance: each pair adjacent, the lower index first
    first = sel[:12].reshape(6, 2)
    assert np.array_equal(np.sort(first.reshape(-1)), np.sort(np.concatenate([near, far])))
    assert (first[:, 0] < first[:, 1]).all() and np.array_equal(dist[0:12:2], dist[1:12:2])
    for a, b in first:
        assert np.array_equal(frames[0][a], frames[0][b])


def _anchor_table(rng, lens, K, trial):
    """kp_idx [B, K]: valid rows, with ignore_label, -1, the frame's last row, an index equal to the frame's length, a
    repeated index and an index past the frame at seeded places (K = 1: one of these kinds per frame, turning with `trial`)"""
    table = np.empty((len(lens), K), np.int64)
    for b, n in enumerate(lens):
        row = rng.integers(0, max(n, 1), K)
        special = [IGNORE, -1, n - 1, n, int(row[0]), n + 5]
        if K == 1:
            row[0] = special[(trial + b) % len(special)]
        else:
            at = rng.permutation(K - 1)[: len(special)] + 1
            row[at] = special
            row[K - 1] = special[(b + 2) % 4]  # the highest class, the first one looked at, is a special entry too
        table[b] = row
    return table


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("K", [1, 64])
def test_radius_labels_class_counts(gpu, K, dtype):
    """The kernel's rule: a negative or out-of-frame index takes no part, the highest class within the radius wins.  The
    restatement gets the table with the out-of-frame entries made -1 (which it skips), every class at its place.  Radius
    20 mm, so that several anchors reach most rows of the gripper."""
    D = _D()
    rng = np.random.default_rng(100 + K)
    frames = [H.gripper_cloud(rng, 200, n_rod=20, n_bg=50)[0][:n].astype(dtype) for n in (300, 0, 257)]
    lens = [len(f) for f in frames]
    pts = torch.from_numpy(np.concatenate(frames)).to(gpu)
    off = np.concatenate([[0], np.cumsum(lens)])
    offsets = torch.from_numpy(off.astype(np.int32)).to(gpu)
    seen = set()
    for trial in range(6 if K == 1 else 2):
        table = _anchor_table(rng, lens, K, trial)
        got = D.radius_labels(pts, offsets, torch.from_numpy(table).to(gpu), 0.02, IGNORE)
        assert got.dtype == torch.int64 and got.shape == (sum(lens),)
        got = got.cpu().numpy()
        for b, f in enumerate(frames):
            inside = np.where((table[b] >= 0) & (table[b] < lens[b]), table[b], -1)
            want = H.radius_labels(f, inside, 0.02, IGNORE)
            assert np.array_equal(got[off[b]: off[b + 1]], want), (trial, b)
            seen.update(want.tolist())
    assert IGNORE in seen and (seen == {IGNORE, 0} if K == 1 else len(seen) > 20 and max(seen) < K)
