"""sv_ee_mask, sv_key_points, sv_line_topk, sv_radius_labels and utils/data.py on the GPU: the per-frame functions against
the reference's recorded results (tests/golden/labels.npz), the batched calls against the numpy restatement of
tests/label_helpers.py (which tests/test_labels_cpu.py pins to the same fixture).

Bounds: indices, masks and labels exact.  Against the fixture the generator's margin condition carries that (every
decision clears its tipping point by more than 1e-9, or 1e-6 where the reference computes in float32); against the
restatement both sides run the same float64 / float32 operations in the same order without fma, so they agree bit for
bit.  Key points within 1e-12; cross-section distances within 1e-12 for float64 input and 1e-7 for float32 input (the
rounding of p - pos to float32 is reproduced, so the figure measured is far below either).

A NaN row: any NaN coordinate makes all three EE-frame coordinates NaN (a product 0 * NaN is NaN), so every mask
comparison is false for it; it can therefore never enter a selection, and "a thresholded search leaves the key point
unfound" is checked as: the frame's only front-side row turned NaN leaves P1-P4 and their twins unfound.
"""
import numpy as np
import pytest
import torch

import label_helpers as H

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 257, 1000]
IGNORE = -100


def _D():
    from mrcc_amd.utils import data

    return data


@pytest.fixture(scope="module")
def fx(golden):
    return golden("labels")


@pytest.fixture(scope="module")
def cloud():
    """one posed gripper with 1175 rows in random order: (float32 points, pose, EE-frame float64 points)"""
    return H.gripper_cloud(np.random.default_rng(42), 600, n_rod=50, n_bg=375)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _ref_frame(points, pose, count=32, cutoff=0.004, value=7):
    """the restatement's results for one frame, run on the frame as it is (no crop)"""
    kp10, idx10 = H.key_points(points, pose)
    kp6, idx6, empty = H.six_key_points(points, pose)
    vote = np.zeros(len(points), dtype=np.int64)
    dist, cs = H.cross_section(points, pose, count, cutoff) if len(points) else (np.zeros(0), np.zeros(0, dtype=np.int64))
    vote[cs] = value
    return dict(mask=H.ee_mask(points, pose), kp10=kp10, idx10=idx10, kp6=kp6, idx6=idx6, empty=empty,
                labels10=H.radius_labels(points, idx10), labels6=H.radius_labels(points, idx6), vote=vote, cs=cs, dist=dist)


def _run_batch(frames, poses, gpu, count=32, cutoff=0.004, value=7):
    """the batched calls on the frames as they are -> numpy results, per frame where the restatement is per frame"""
    D = _D()
    lens = [len(f) for f in frames]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pts = torch.from_numpy(np.concatenate(frames)).to(gpu)
    offsets = torch.from_numpy(off.astype(np.int32)).to(gpu)
    pos, rot = D.pose_tables(poses, gpu)
    out = dict(mask=D.ee_mask(pts, offsets, pos, rot).cpu().numpy().astype(bool))
    for name in ("10", "6"):
        labels, kp, idx = D.key_point_labels_batch(pts, offsets, poses, generator=name)
        assert labels.dtype == torch.int64 and kp.dtype == torch.float64 and idx.dtype == torch.int64
        out["labels" + name], out["kp" + name], out["idx" + name] = labels.cpu().numpy(), kp.cpu().numpy(), idx.cpu().numpy()
    out["vote"] = D.vote_labels_batch(pts, offsets, poses, count=count, cutoff=cutoff, value=value).cpu().numpy()
    lp1, lp2 = D.CROSS_SECTION_LINE
    cs, dist, n_sel = D.line_topk(pts, offsets, pos, rot, lp2, lp1, count, cutoff)
    out["cs"], out["dist"], out["n_sel"] = cs.cpu().numpy(), dist.cpu().numpy(), n_sel.cpu().numpy()
    out["off"] = off
    return out


def _check_batch(frames, poses, got, count=32, cutoff=0.004, value=7):
    off = got["off"]
    for b, (f, pose) in enumerate(zip(frames, poses)):
        ref = _ref_frame(f, pose, count, cutoff, value)
        rows = slice(off[b], off[b + 1])
        assert np.array_equal(got["mask"][rows], ref["mask"]), b
        for name in ("10", "6"):
            assert np.array_equal(got["idx" + name][b], ref["idx" + name]), (b, name, got["idx" + name][b], ref["idx" + name])
            assert np.abs(got["kp" + name][b] - ref["kp" + name]).max() <= 1e-12, (b, name)
            assert np.array_equal(got["labels" + name][rows], ref["labels" + name]), (b, name)
        k = int(got["n_sel"][b])
        assert k == len(ref["cs"]) and np.array_equal(got["cs"][b, :k], ref["cs"]), b
        assert (got["cs"][b, k:] == -1).all() and np.isinf(got["dist"][b, k:]).all()
        if k:
            bound = 1e-12 if f.dtype == np.float64 else 1e-7
            assert np.abs(got["dist"][b, :k] - ref["dist"]).max() <= bound
        assert np.array_equal(got["vote"][rows], ref["vote"]), b


# ---------------------------------------------------------------------------------------------------------------------
# the reference's per-frame functions against its recorded results
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [0, 1, 2, 3])
def test_per_frame_functions_against_the_fixture(gpu, fx, ci):
    D = _D()
    g = lambda k: fx[f"c{ci}_{k}"]  # noqa: E731
    points, pose = g("points"), g("pose")
    xyzw = np.concatenate([pose[:3], pose[4:], pose[3:4]])  # the same pose with w last, for switch_w=True
    ee = D.get_ee_idx(points, pose, switch_w=False)
    assert ee.dtype == np.int64 and np.array_equal(ee, g("ee_idx"))
    assert np.array_equal(D.get_ee_idx(points, xyzw), g("ee_idx"))
    arm = g("ee_idx")[::2]
    assert np.array_equal(D.get_ee_idx(points, pose, switch_w=False, arm_idx=arm), arm)
    wide = D.get_ee_idx(points, pose, switch_w=False, ee_dim={"min_z": -0, "max_z": 0.13, "min_y": -0.14, "max_y": 0.14})
    assert np.array_equal(wide, H.ee_idx(points, pose, {"min_z": -0, "max_z": 0.13, "min_y": -0.14, "max_y": 0.14}))
    crop = points[ee]
    dist, idx = D.get_ee_cross_section_idx(crop, pose, count=int(fx["count"]), cutoff=float(fx["cutoff"]), switch_w=False)
    assert idx.dtype == np.int64 and dist.dtype == np.float64 and np.array_equal(idx, g("cs_idx"))
    err = float(np.abs(dist - g("cs_dists")).max())
    print(f"case {ci}: cross-section max err {err:.2e}")
    assert err <= (1e-12 if ci == 3 else 1e-7)
    kp, kidx = D.get_key_points(crop, pose, switch_w=False)
    assert kp.shape == (10, 3) and kidx.dtype == np.int64 and np.array_equal(kidx, g("kp10_idx"))
    kp6, kidx6 = D.get_6_key_points(crop, xyzw)
    assert kp6.shape == (6, 3) and np.array_equal(kidx6, g("kp6_idx"))
    e10, e6 = float(np.abs(kp - g("kp10")).max()), float(np.abs(kp6 - g("kp6")).max())
    print(f"case {ci}: key points max err {e10:.2e} / {e6:.2e}")
    assert max(e10, e6) <= 1e-12
    for name, k in (("10", kidx), ("6", kidx6)):
        pcls, pidx = D.collect_closest_points(k[k > -1], crop, float(fx["radius"]))
        assert np.array_equal(pcls, g("pcls" + name)) and np.array_equal(pidx, g("pidx" + name))
    # the batched form on the same crop gives the label array load_key_points writes
    for name in ("10", "6"):
        labels, _, bidx = D.key_point_labels_batch(crop, [0, len(crop)], pose[None], generator=name)
        assert np.array_equal(labels.cpu().numpy(), g("labels" + name))
        assert np.array_equal(bidx.cpu().numpy()[0], g(f"kp{name}_idx"))


# ---------------------------------------------------------------------------------------------------------------------
# the batched calls against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", SIZES)
def test_one_frame_against_restatement(gpu, cloud, n, dtype):
    points, pose, _ = cloud
    frames, poses = [points[:n].astype(dtype)], pose[None]
    _check_batch(frames, poses, _run_batch(frames, poses, gpu))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_five_frames_against_restatement(gpu, dtype):
    """B = 5 with an empty frame in the middle and a frame of a single point"""
    rng = np.random.default_rng(5)
    frames, poses = [], []
    for n in (257, 64, 0, 1, 1000):
        p, pose, _ = H.gripper_cloud(rng, 600, n_rod=50, n_bg=375)
        frames.append(p[:n].astype(dtype))
        poses.append(pose)
    poses = np.stack(poses)
    got = _run_batch(frames, poses, gpu)
    _check_batch(frames, poses, got)
    again = _run_batch(frames, poses, gpu)  # two identical calls give identical bits
    for k in got:
        a, b = got[k], again[k]
        assert np.array_equal(_bits(a), _bits(b)) if a.dtype == np.float64 else np.array_equal(a, b), k


def _posed(ee, pose, dtype=np.float32):
    return (H.rot(H.rotation(pose[3:]), ee) + pose[:3]).astype(dtype)


@pytest.mark.parametrize("which", ["front", "back", "gripper", "six"])
def test_empty_selections_give_the_defined_result(gpu, cloud, which):
    """a cloud cut (with 1 mm to spare for the float32 rounding) so that one mask selects nothing"""
    D = _D()
    _, pose, ee = cloud
    keep = {"front": ee[:, 0] < 0.004, "back": ee[:, 0] > -0.009, "gripper": ee[:, 2] < 0.079, "six": ee[:, 0] < -0.006}[which]
    frames, poses = [_posed(ee[keep], pose)], pose[None]
    got = _run_batch(frames, poses, gpu)
    _check_batch(frames, poses, got)
    template10 = H.rot(H.rotation(pose[3:]), H.KP10 + H.kp_frame(frames[0], pose)[1])
    if which == "front":  # the reference raises a TypeError here
        assert (got["idx10"][0][[0, 1, 2, 3]] == IGNORE).all()
        assert np.abs(got["kp10"][0][:4] - template10[:4]).max() <= 1e-12
        kp, idx = D.get_key_points(frames[0], pose, switch_w=False)
        assert np.array_equal(idx, got["idx10"][0])
    elif which == "back":
        assert (got["idx10"][0][6:] == IGNORE).all() and (got["idx10"][0][:4] != IGNORE).any()
    elif which == "gripper":
        assert (got["idx10"][0][4:6] == IGNORE).all() and (got["idx6"][0][4:] == IGNORE).all()
        assert np.abs(got["kp10"][0][4:6] - template10[4:6]).max() <= 1e-12
    else:
        assert (got["idx6"][0] == IGNORE).all()
        template6 = H.rot(H.rotation(pose[3:]), H.KP6 + H.kp_frame(frames[0], pose)[1])
        assert np.abs(got["kp6"][0] - template6).max() <= 1e-12
        kp, idx = D.get_6_key_points(frames[0], pose, switch_w=False)  # the per-frame wrapper keeps the empty arrays
        assert kp.shape == (0,) and idx.shape == (0,)
        assert (got["labels6"] == IGNORE).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_exact_ties_go_to_the_lower_index(gpu, cloud, dtype):
    """the end-effector crop followed by a copy of itself: every arg-min and every cross-section distance has an exact twin n rows on"""
    points, pose, _ = cloud
    crop = points[H.ee_idx(points, pose)]  # on the crop both generators find key points
    n = len(crop)
    frames, poses = [np.concatenate([crop, crop]).astype(dtype)], pose[None]
    got = _run_batch(frames, poses, gpu, count=32, cutoff=0.05)
    _check_batch(frames, poses, got, count=32, cutoff=0.05)
    for name in ("10", "6"):
        idx = got["idx" + name][0]
        searched = np.r_[idx[:4], idx[6:]]  # the gripper pair's index follows the reference's own rule
        assert (searched[searched != IGNORE] < n).all() and (searched != IGNORE).any()
    cs = got["cs"][0]
    assert got["n_sel"][0] == 32 and np.array_equal(cs[1::2], cs[0::2] + n) and (cs[0::2] < n).all()
    assert np.array_equal(got["dist"][0][0::2], got["dist"][0][1::2]) and np.all(np.diff(got["dist"][0][0::2]) > 0)


def test_nan_row(gpu, cloud):
    points, pose, ee = cloud
    rng = np.random.default_rng(9)
    others = [H.gripper_cloud(rng, 300) for _ in range(2)]
    frames = [others[0][0], points.copy(), others[1][0]]
    poses = np.stack([others[0][1], pose, others[1][1]])
    clean = _run_batch(frames, poses, gpu)
    target = int(clean["idx10"][1][0])  # the row P1 settled on
    assert target != IGNORE
    frames[1][target, 1] = np.nan
    got = _run_batch(frames, poses, gpu)
    _check_batch(frames, poses, got)
    row = got["off"][1] + target
    assert not got["mask"][row] and clean["mask"][row]
    assert got["labels10"][row] == IGNORE and got["labels6"][row] == IGNORE and got["vote"][row] == 0
    assert target not in got["idx10"][1][[0, 1, 2, 3, 6, 7, 8, 9]] and target not in got["cs"][1]
    for b in (0, 2):  # the other frames of the batch are unchanged bit for bit
        rows = slice(got["off"][b], got["off"][b + 1])
        for k in ("mask", "labels10", "labels6", "vote"):
            assert np.array_equal(got[k][rows], clean[k][rows]), (b, k)
        for k in ("idx10", "idx6", "cs", "n_sel"):
            assert np.array_equal(got[k][b], clean[k][b]), (b, k)
        for k in ("kp10", "kp6", "dist"):
            assert np.array_equal(_bits(got[k][b]), _bits(clean[k][b])), (b, k)
    # the frame's only front-side row turned NaN: P1 .. P4 and their twins on the back side stay unfound
    front = np.where(ee[:, 0] > 0.006)[0]
    near = front[np.argmin(H.norm3(ee[front] - H.KP10[0]))]
    lone = np.concatenate([ee[ee[:, 0] < 0.004], ee[near: near + 1]])
    f = _posed(lone, pose)
    found = _run_batch([f], pose[None], gpu)
    assert (found["idx10"][0][:4] == len(f) - 1).sum() >= 1
    f[-1, 2] = np.nan
    lost = _run_batch([f], pose[None], gpu)
    _check_batch([f], pose[None], lost)
    assert (lost["idx10"][0][:4] == IGNORE).all()


def test_radius_labels_classes(gpu):
    D = _D()
    # frame 0: rows 0 and 1 are anchors 4 mm apart, row 2 lies between them, row 3 near anchor 0 only, row 4 far away
    f0 = np.array([[0, 0, 0], [0.004, 0, 0], [0.002, 0, 0], [-0.004, 0, 0], [0.1, 0, 0]], dtype=np.float32)
    f1 = np.array([[0, 0, 0], [0.001, 0, 0]], dtype=np.float32)
    pts = torch.from_numpy(np.concatenate([f0, f1])).to(gpu)
    off = torch.tensor([0, 5, 7], dtype=torch.int32, device=gpu)
    kp_idx = torch.tensor([[0, IGNORE, 1], [IGNORE, IGNORE, IGNORE]], dtype=torch.int64, device=gpu)
    labels = D.radius_labels(pts, off, kp_idx, 0.006, IGNORE).cpu().numpy()
    # rows 0, 1, 2 lie within 6 mm of both anchors: the higher class (2) wins; row 3 is 8 mm from anchor 1
    assert labels.tolist() == [2, 2, 2, 0, IGNORE, IGNORE, IGNORE]
    for b, f in enumerate((f0, f1)):
        assert np.array_equal(labels[[0, 5][b]: [5, 7][b]], H.radius_labels(f, kp_idx[b].cpu().numpy()))
    # an index past the frame's end takes no part either (it must not read the next frame's rows)
    kp_idx[1, 0] = 2
    assert D.radius_labels(pts, off, kp_idx, 0.006, IGNORE).cpu().numpy()[5:].tolist() == [IGNORE, IGNORE]
    # the strict compare in the points' dtype: a row at exactly the float32 threshold is outside
    thr = np.float32(0.006)
    edge = torch.tensor([[0, 0, 0], [float(thr), 0, 0], [float(np.nextafter(thr, np.float32(0))), 0, 0]], dtype=torch.float32,
                        device=gpu)
    got = D.radius_labels(edge, torch.tensor([0, 3], dtype=torch.int32, device=gpu),
                          torch.tensor([[0]], dtype=torch.int64, device=gpu), 0.006, IGNORE).cpu().numpy()
    assert got.tolist() == [0, IGNORE, 0]


@pytest.mark.parametrize("count", [1, 32, 64])
def test_cross_section_counts(gpu, cloud, count):
    """count = 1, 32, and larger than the frame (40 rows, no cutoff to speak of: every row is selected, the rest padded)"""
    D = _D()
    points, pose, _ = cloud
    frames, poses = [points[:40], points[40:1040]], np.stack([pose, pose])
    got = _run_batch(frames, poses, gpu, count=count, cutoff=10.0)
    _check_batch(frames, poses, got, count=count, cutoff=10.0)
    assert got["n_sel"].tolist() == [min(count, 40), count]
    assert np.all(np.diff(got["dist"][1]) >= 0)
    dist, idx = D.get_ee_cross_section_idx(frames[0], pose, count=count, cutoff=10.0, switch_w=False)
    assert np.array_equal(idx, got["cs"][0][: len(idx)]) and len(idx) == min(count, 40)
    every, _ = D.get_ee_cross_section_idx(frames[0], pose, count=0, cutoff=10.0, switch_w=False)  # count <= 0: all rows
    assert len(every) == 40


def test_ee_crop_batch(gpu):
    D = _D()
    rng = np.random.default_rng(21)
    frames, poses, feats, labels = [], [], [], []
    for n in (900, 0, 1, 300):
        p, pose, _ = H.gripper_cloud(rng, 500)
        frames.append(p[:n])
        poses.append(pose)
        feats.append(rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32))
        labels.append(rng.integers(0, 3, n).astype(np.int64))
    poses = np.stack(poses)
    pts, f, l, off, kept = D.ee_crop_batch(frames, feats, labels, poses)
    ref = [H.ee_idx(p, pose) for p, pose in zip(frames, poses)]
    assert off.dtype == torch.int32 and off.cpu().tolist() == np.concatenate([[0], np.cumsum([len(r) for r in ref])]).tolist()
    assert len(kept) == 4 and all(np.array_equal(k.cpu().numpy(), r) for k, r in zip(kept, ref))
    assert len(ref[0]) > 100 and pts.dtype == torch.float32
    assert np.array_equal(pts.cpu().numpy(), np.concatenate([p[r] for p, r in zip(frames, ref)]))
    assert np.array_equal(f.cpu().numpy(), np.concatenate([x[r] for x, r in zip(feats, ref)]))
    assert np.array_equal(l.cpu().numpy(), np.concatenate([x[r] for x, r in zip(labels, ref)]))
    dim = {"min_z": -0, "max_z": 0.13, "min_y": -0.14, "max_y": 0.14}
    _, none_f, none_l, off2, kept2 = D.ee_crop_batch(frames, None, None, poses, ee_dim=dim)
    assert none_f is None and none_l is None
    assert all(np.array_equal(k.cpu().numpy(), H.ee_idx(p, pose, dim)) for k, p, pose in zip(kept2, frames, poses))


def test_composition_into_a_training_batch(gpu):
    """ee_crop_batch -> key_point_labels_batch -> augment_quantize_batch(device tensors, point_offsets=...) with every
    augmentation off equals the per-frame chain (restatement crop, restatement labels, the list form) exactly"""
    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd.utils import augmentation as A

    D = _D()
    rng = np.random.default_rng(33)
    frames, poses, feats = [], [], []
    for n_body in (400, 900, 250):
        p, pose, _ = H.gripper_cloud(rng, n_body)
        frames.append(p)
        poses.append(pose)
        feats.append(rng.uniform(-0.5, 0.5, (len(p), 3)).astype(np.float32))
    poses = np.stack(poses)
    pts, f, _, off, _ = D.ee_crop_batch(frames, feats, None, poses)
    labels, _, _ = D.key_point_labels_batch(pts, off, poses, generator="10")
    got = A.augment_quantize_batch(pts, f, labels, point_offsets=off, quantization_size=0.002, center_at_origin=True)
    ref_p, ref_f, ref_l = [], [], []
    for p, x, pose in zip(frames, feats, poses):
        idx = H.ee_idx(p, pose)
        ref_p.append(p[idx])
        ref_f.append(x[idx])
        ref_l.append(H.radius_labels(p[idx], H.key_points(p[idx], pose)[1]))
    assert sum((l >= 0).sum() for l in ref_l) > 20
    want = A.augment_quantize_batch(ref_p, ref_f, ref_l, quantization_size=0.002, center_at_origin=True)
    for a, b, name in zip(got, want, ("coordinates", "features", "labels", "offsets")):
        assert a.dtype == b.dtype and torch.equal(a, b), name
    assert (got[2] >= 0).any()
    st = ME.SparseTensor(got[1], coordinates=got[0])
    assert torch.equal(st.C, got[0]) and torch.equal(st.F, got[1])
    # host offsets and a list of host feature arrays beside device tensors give the same batch
    mixed = A.augment_quantize_batch(pts, ref_f, labels.reshape(-1, 1), point_offsets=off.cpu().tolist(),
                                     quantization_size=0.002, center_at_origin=True)
    assert all(torch.equal(a, b) for a, b in zip(mixed, want))
