"""utils/data.py of the reference on libsvhip: farthest point sampling (:13-34) and the per-frame training labels the
reference synthesises from a frame's pose (:58-342) - the end-effector crop, the vote head's cross-section, the key
points of the key-point network and their radius labels.

The reference's names keep their signatures and return types (host arrays in, numpy out, `switch_w` honoured):
get_roi_mask and get_closest_point are host numpy; get_ee_idx, get_ee_cross_section_idx, get_key_points,
get_6_key_points and collect_closest_points run a batch of one frame through sv_ee_mask / sv_line_topk / sv_key_points /
sv_radius_labels (include/sv_hip.h N6, where the dtype rules and the defined edge cases are written down).

Training should call the batched forms, which take and return device tensors and feed
utils.augmentation.augment_quantize_batch(..., point_offsets=...) directly:

    ee_crop_batch            frames -> cropped points / features / labels, new offsets, kept indices   (1 launch)
    key_point_labels_batch   crops -> per-point key-point class labels, key points, their indices       (2 launches)
    vote_labels_batch        crops -> labels with `value` on the cross-section                          (2 launches)

Poses are [B, 7] host arrays (x, y, z, qw, qx, qy, qz: the quaternion as the dataloader has it, switch_w=False), taken as
float64; the 9 doubles of a frame's rotation matrix are computed on the host and travel as a table.  Only ee_crop_batch
waits for the device (one read-back of the per-frame kept counts).
"""
from ctypes import c_double, c_int, c_int64, c_size_t

import numpy as np
import torch

from .. import _lib
from .._lib import SvHipError, call, ptr, stream_ptr
from ..model.pointnet2_utils import farthest_point_sample
from .transformation import get_quaternion_rotation_matrix

EE_DIM = {"min_z": -0.006, "max_z": 0.12, "min_x": -0.05, "max_x": 0.05, "min_y": -0.11, "max_y": 0.11}  # :79-86
CROSS_SECTION_LINE = (np.array([-0.05, 0.0, 0.0]), np.array([0.05, 0.0, 0.0]))  # :116-117
KEY_POINT_THRESHOLDS = {10: 0.018, 6: 0.03}  # :141, :255


def get_farthest_point_sample_idx(point, npoint, start=None):
    """point [N, D] (xyz in the first 3 columns) -> int32[npoint].  The reference draws the first index with
    np.random.randint(0, N); pass `start` to pin it."""
    point = np.asarray(point)
    N = point.shape[0]
    if start is None:
        start = np.random.randint(0, N)
    xyz = torch.from_numpy(np.ascontiguousarray(point[:, :3], dtype=np.float32)).cuda().unsqueeze(0)
    st = torch.tensor([int(start)], dtype=torch.int64, device=xyz.device)
    return farthest_point_sample(xyz, npoint, start=st)[0].cpu().numpy().astype(np.int32)


def get_farthest_point_sample(point, npoint):
    return point[get_farthest_point_sample_idx(point, npoint)]


# ---------------------------------------------------------------------------------------------------------------------
# device plumbing: tensors in, tensors out, nothing read back
# ---------------------------------------------------------------------------------------------------------------------
def _cuda_device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise SvHipError(f"the label kernels run on the GPU (got device {dev}); there is no CPU fallback")
    return dev


def _device_points(points, device="cuda"):
    """float32 / float64 [N, 3] on the device (a host array is uploaded; other dtypes become float64)"""
    if isinstance(points, torch.Tensor):
        if not points.is_cuda:
            raise SvHipError(f"points must be a host array or a CUDA tensor (got a {points.device} tensor); "
                             "the HIP path has no CPU fallback")
        t = points
    else:
        a = np.asarray(points)
        if a.dtype != np.float32:
            a = a.astype(np.float64)
        t = torch.from_numpy(np.ascontiguousarray(a)).to(_cuda_device(device))
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"points must be [N, 3], got {tuple(t.shape)}")
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    return t.contiguous()


def _device_offsets(offsets, N, dev):
    """int32 [B + 1] on the device; a host sequence is checked (non-decreasing from 0 to N) and uploaded"""
    if isinstance(offsets, torch.Tensor) and offsets.is_cuda:
        off = offsets.to(torch.int32).contiguous().reshape(-1)
    else:
        o = np.asarray(offsets.cpu() if isinstance(offsets, torch.Tensor) else offsets, dtype=np.int64).reshape(-1)
        if len(o) < 2 or o[0] != 0 or o[-1] != N or (np.diff(o) < 0).any():
            raise ValueError(f"offsets must rise from 0 to the number of points ({N})")
        off = torch.from_numpy(o.astype(np.int32)).to(dev)
    B = off.numel() - 1
    if not 1 <= B <= _lib.SV_MAX_BATCH:
        raise ValueError(f"need 1 to {_lib.SV_MAX_BATCH} frames, got {B}")
    return off, B


def pose_tables(poses, dev, switch_w=False):
    """poses [B, 7] (host) -> (pos float64 [B, 3], rot float64 [B, 9]) on the device; the rotation matrices come from
    get_quaternion_rotation_matrix on the host."""
    p = np.asarray(poses.detach().cpu() if isinstance(poses, torch.Tensor) else poses, dtype=np.float64)
    p = np.atleast_2d(p)
    if p.shape[1] != 7:
        raise ValueError(f"poses must be [B, 7], got {p.shape}")
    rot = np.stack([get_quaternion_rotation_matrix(row[3:], switch_w=switch_w).reshape(9) for row in p])
    return (torch.from_numpy(np.ascontiguousarray(p[:, :3])).to(dev), torch.from_numpy(np.ascontiguousarray(rot)).to(dev))


def _f64(points):
    return c_int(1 if points.dtype == torch.float64 else 0)


def _check_frames(pos, rot, B):
    if pos.shape[0] != B or rot.shape[0] != B:
        raise ValueError(f"{B} frames need {B} poses, got {pos.shape[0]}")


def ee_mask(points, offsets, pos, rot, ee_dim=None):
    """sv_ee_mask: uint8 [N], 1 inside the end-effector box of the row's frame (ee_dim updates the reference's defaults)"""
    N, B = points.shape[0], offsets.numel() - 1
    _check_frames(pos, rot, B)
    dim = dict(EE_DIM)
    if isinstance(ee_dim, dict):
        dim.update(ee_dim)
    box = (c_double * 6)(*(float(dim[k]) for k in ("min_x", "max_x", "min_y", "max_y", "min_z", "max_z")))
    mask = torch.empty(N, dtype=torch.uint8, device=points.device)
    call("sv_ee_mask", ptr(points), _f64(points), ptr(offsets), c_int64(N), c_int(B), ptr(pos), ptr(rot), box, ptr(mask),
         stream_ptr())
    return mask


def key_points(points, offsets, pos, rot, mode=10, euclidean_threshold=None, ignore_label=-100):
    """sv_key_points -> (key_points float64 [B, K, 3] in the camera frame, kp_idx int64 [B, K] within the frame,
    selection_empty int32 [B]: 1 where get_6_key_points would return empty arrays)"""
    N, B = points.shape[0], offsets.numel() - 1
    _check_frames(pos, rot, B)
    if mode not in KEY_POINT_THRESHOLDS:
        raise ValueError("mode must be 10 (get_key_points) or 6 (get_6_key_points)")
    thr = KEY_POINT_THRESHOLDS[mode] if euclidean_threshold is None else float(euclidean_threshold)
    dev = points.device
    kp = torch.empty((B, mode, 3), dtype=torch.float64, device=dev)
    idx = torch.empty((B, mode), dtype=torch.int64, device=dev)
    empty = torch.empty(B, dtype=torch.int32, device=dev)
    call("sv_key_points", ptr(points), _f64(points), ptr(offsets), c_int64(N), c_int(B), ptr(pos), ptr(rot), c_int(mode),
         c_double(thr), c_int64(int(ignore_label)), ptr(kp), ptr(idx), ptr(empty), stream_ptr())
    return kp, idx, empty


def line_topk(points, offsets, pos, rot, lp1, lp2, count, cutoff):
    """sv_line_topk with compute_dists_to_line's (lp1, lp2) -> (idx int64 [B, count] padded with -1, dist float64
    [B, count] padded with inf, n_sel int32 [B])"""
    lib = _lib.load()
    N, B = points.shape[0], offsets.numel() - 1
    _check_frames(pos, rot, B)
    dev = points.device
    idx = torch.empty((B, count), dtype=torch.int64, device=dev)
    dist = torch.empty((B, count), dtype=torch.float64, device=dev)
    n_sel = torch.empty(B, dtype=torch.int32, device=dev)
    ws_bytes = lib.sv_line_topk_workspace_bytes(c_int64(N))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    a = (c_double * 3)(*(float(v) for v in lp1))
    b = (c_double * 3)(*(float(v) for v in lp2))
    call("sv_line_topk", ptr(points), _f64(points), ptr(offsets), c_int64(N), c_int(B), ptr(pos), ptr(rot), a, b,
         c_int(int(count)), c_double(float(cutoff)), ptr(ws), c_size_t(ws_bytes), ptr(idx), ptr(dist), ptr(n_sel),
         stream_ptr())
    return idx, dist, n_sel


def radius_labels(points, offsets, kp_idx, euclidean_threshold=0.006, ignore_label=-100):
    """sv_radius_labels: int64 [N], the highest class k whose anchor row kp_idx[b, k] lies within the radius"""
    N, B = points.shape[0], offsets.numel() - 1
    kp_idx = kp_idx.to(torch.int64).contiguous()
    if kp_idx.dim() != 2 or kp_idx.shape[0] != B:
        raise ValueError(f"kp_idx must be [{B}, K], got {tuple(kp_idx.shape)}")
    labels = torch.empty(N, dtype=torch.int64, device=points.device)
    call("sv_radius_labels", ptr(points), _f64(points), ptr(offsets), c_int64(N), c_int(B), ptr(kp_idx),
         c_int(kp_idx.shape[1]), c_double(float(euclidean_threshold)), c_int64(int(ignore_label)), ptr(labels), stream_ptr())
    return labels


# ---------------------------------------------------------------------------------------------------------------------
# the batched forms
# ---------------------------------------------------------------------------------------------------------------------
def _cat_frames(frames, dev, dtype=None):
    """a list of per-frame host arrays or tensors -> (one device tensor of the concatenated rows, rows per frame)"""
    ts = [f.to(dev) if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in frames]
    lens = [int(t.shape[0]) for t in ts]
    cat = torch.cat([t.unsqueeze(1) if t.dim() == 1 else t for t in ts])
    return (cat if dtype is None else cat.to(dtype)), lens


def ee_crop_batch(points, feats, labels, poses, *, ee_dim=None, device="cuda"):
    """The end-effector crop of get_ee_idx (data/alivev2.py:135-169, data_type "ee_seg") for a batch of frames.

    points / feats / labels: lists of per-frame arrays [n_b, 3] / [n_b, C] / [n_b] (host arrays or tensors; feats and
    labels may be None); poses [B, 7].  Returns (points [M, 3], feats [M, C] or None, labels [M] or None, offsets int32
    [B + 1], kept): device tensors of the rows inside each frame's box, frame after frame in their original order, and
    kept = a list of B int64 device tensors, the kept rows' indices within their frame.  One launch (sv_ee_mask); the
    compaction is torch index arithmetic on the device and costs one read-back of the per-frame kept counts."""
    dev = _cuda_device(device)
    B = len(points)
    if not 1 <= B <= _lib.SV_MAX_BATCH:
        raise ValueError(f"need 1 to {_lib.SV_MAX_BATCH} frames, got {B}")
    frames = [np.asarray(p) if not isinstance(p, torch.Tensor) else p for p in points]
    for p in frames:
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError("every frame needs points [n, 3]")
    f32 = all(p.dtype in (np.float32, torch.float32) for p in frames)
    cat, lens = _cat_frames(frames, dev, torch.float32 if f32 else torch.float64)
    pts = _device_points(cat)
    N = pts.shape[0]
    extra = []
    for name, x in (("feats", feats), ("labels", labels)):
        if x is None:
            extra.append(None)
            continue
        t, ln = _cat_frames(list(x), dev)
        if ln != lens:
            raise ValueError(f"{name} need one row per point of every frame")
        extra.append(t if name == "feats" else t.reshape(-1))
    with torch.cuda.device(dev):
        off, _ = _device_offsets(np.concatenate([[0], np.cumsum(lens)]), N, dev)
        pos, rot = pose_tables(poses, dev)
        mask = ee_mask(pts, off, pos, rot, ee_dim)
        csum = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(mask, 0, dtype=torch.int64)])
        new_off = csum[off.long()]
        counts = (new_off[1:] - new_off[:-1]).cpu().tolist()  # the one wait
        M = int(sum(counts))
        # row j of the crop is the first row whose running count reaches j + 1
        rows = torch.searchsorted(csum[1:], torch.arange(1, M + 1, dtype=torch.int64, device=dev))
        frame = torch.repeat_interleave(torch.arange(B, device=dev), new_off[1:] - new_off[:-1], output_size=M)
        kept = list((rows - off.long()[frame]).split(counts))
        out = (pts[rows],) + tuple(None if t is None else t[rows] for t in extra)
    return out + (new_off.to(torch.int32), kept)


def key_point_labels_batch(points, offsets, poses, *, generator="10", euclidean_threshold=None, radius=0.006,
                           ignore_label=-100):
    """load_key_points (data/alivev2.py:212-238) for a batch of end-effector crops: points [N, 3] (device tensor or host
    array), offsets [B + 1], poses [B, 7]; generator "10" = get_key_points, "6" = get_6_key_points;
    euclidean_threshold None = the generator's default (0.018 / 0.03); radius = collect_closest_points' threshold.
    Returns device tensors (labels int64 [N]: the key-point class of every row within `radius` of a found key point's
    row, else ignore_label; key_points float64 [B, K, 3]; kp_idx int64 [B, K]).  Launches: sv_key_points,
    sv_radius_labels; no host wait."""
    mode = {"10": 10, "6": 6, 10: 10, 6: 6}.get(generator)
    if mode is None:
        raise ValueError('generator must be "10" or "6"')
    pts = _device_points(points)
    dev = pts.device
    with torch.cuda.device(dev):
        off, _ = _device_offsets(offsets, pts.shape[0], dev)
        pos, rot = pose_tables(poses, dev)
        kp, idx, _ = key_points(pts, off, pos, rot, mode, euclidean_threshold, ignore_label)
        labels = radius_labels(pts, off, idx, radius, ignore_label)
    return labels, kp, idx


def vote_labels_batch(points, offsets, poses, *, labels=None, count=32, cutoff=0.004, value):
    """The vote head's targets (data/alivev2.py:252-268) for a batch of end-effector crops: `value` written on the
    `count` rows of every frame closest to the gripper's x axis (get_ee_cross_section_idx), the rest of `labels` kept
    (labels None: zeros int64, the "ee_seg" case).  Returns a new device tensor shaped like labels ([N] when None).
    Launches: sv_line_topk (two kernels); no host wait."""
    pts = _device_points(points)
    dev, N = pts.device, pts.shape[0]
    with torch.cuda.device(dev):
        off, B = _device_offsets(offsets, N, dev)
        pos, rot = pose_tables(poses, dev)
        lp1, lp2 = CROSS_SECTION_LINE
        idx, _, _ = line_topk(pts, off, pos, rot, lp2, lp1, count, cutoff)  # select_closest_points_to_line swaps them
        if labels is None:
            out = torch.zeros(N, dtype=torch.int64, device=dev)
        else:
            out = (labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.asarray(labels))).to(dev).clone()
            if out.shape[0] != N:
                raise ValueError("labels need one row per point")
        if N == 0:
            return out
        # the padding (-1) goes to a spare slot past the end, so that nothing is compacted (and nothing waits)
        rows = torch.where(idx >= 0, idx + off[:-1].long()[:, None], torch.full_like(idx, N)).reshape(-1)
        flat = torch.cat([out.reshape(N, -1), out.new_zeros((1,) + tuple(out.reshape(N, -1).shape[1:]))])
        flat[rows] = value
        return flat[:N].reshape(out.shape)


# ---------------------------------------------------------------------------------------------------------------------
# the reference's per-frame functions
# ---------------------------------------------------------------------------------------------------------------------
def get_roi_mask(points, min_x=-500, max_x=500, min_y=-500, max_y=500, min_z=-500, max_z=500, offset=0.0):
    """:58-75 on the host: strict inequalities on every axis, the box grown by `offset`"""
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    mask = x > -500
    for v, lo, hi in ((x, min_x, max_x), (y, min_y, max_y), (z, min_z, max_z)):
        mask = mask & (v < hi + offset) & (v > lo - offset)
    return mask


def _one_frame(points, pose, switch_w, device):
    pts = _device_points(np.asarray(points), device)
    dev = pts.device
    off = torch.tensor([0, pts.shape[0]], dtype=torch.int32, device=dev)
    pos, rot = pose_tables(np.asarray(pose, dtype=np.float64).reshape(1, -1)[:, :7], dev, switch_w=switch_w)
    return pts, off, pos, rot


def get_ee_idx(points, pose, switch_w=True, ee_dim=None, arm_idx=None, *, device="cuda"):
    """:78-103: indices of the points inside the end-effector box of `pose` (in training switch_w = False)"""
    pts, off, pos, rot = _one_frame(points, pose, switch_w, device)
    with torch.cuda.device(pts.device):
        ee_idx = np.where(ee_mask(pts, off, pos, rot, ee_dim).cpu().numpy())[0]
    if arm_idx is not None:
        ee_idx = ee_idx[np.isin(ee_idx, arm_idx, assume_unique=True)]
    return ee_idx


def get_ee_cross_section_idx(ee_points, pose, count=32, cutoff=0.004, switch_w=True, *, device="cuda"):
    """:106-122 -> (dists float64, idx int64) of the at most `count` points closest to the gripper's x axis, ascending,
    those at or beyond `cutoff` dropped; count <= 0 takes every point (up to sv_line_topk's 1024)."""
    n = len(ee_points)
    count = min(count, n) if count > 0 else n
    if count < 1:
        return np.zeros(0, dtype=np.float64), np.zeros(0, dtype=np.int64)
    if count > 1024:
        raise ValueError("sv_line_topk returns at most 1024 points per frame")
    pts, off, pos, rot = _one_frame(ee_points, pose, switch_w, device)
    with torch.cuda.device(pts.device):
        lp1, lp2 = CROSS_SECTION_LINE
        idx, dist, n_sel = line_topk(pts, off, pos, rot, lp2, lp1, count, cutoff)
        k = int(n_sel.cpu()[0])
        return dist[0, :k].cpu().numpy(), idx[0, :k].cpu().numpy()


def get_closest_point(p, points, maximize_dim=None):
    """:125-138 on the host -> (index, point, distance) of the row of `points` nearest p, or None without rows; with
    maximize_dim that coordinate of p is first replaced by the rows' maximum"""
    if len(points) < 1:
        return None
    p = np.array(p, dtype=np.result_type(np.asarray(p).dtype, np.float64), copy=True)
    if maximize_dim is not None:
        p[maximize_dim] = points[:, maximize_dim].max()
    norms = np.linalg.norm(points - p, axis=1)
    k = norms.argmin()
    return k, points[k], norms.min()


def _key_points_one(ee_points, pose, switch_w, mode, euclidean_threshold, ignore_label, device):
    pts, off, pos, rot = _one_frame(ee_points, pose, switch_w, device)
    with torch.cuda.device(pts.device):
        kp, idx, empty = key_points(pts, off, pos, rot, mode, euclidean_threshold, ignore_label)
        return kp[0].cpu().numpy(), idx[0].cpu().numpy(), bool(empty.cpu()[0])


def get_key_points(ee_points, pose, switch_w=True, euclidean_threshold=0.018, ignore_label=-100, *, device="cuda"):
    """:141-252 -> (key points float64 [10, 3] in the camera frame, their indices int64 [10], ignore_label where not
    found).  Where the reference raises (no point on the front side) the search is simply "not found"."""
    kp, idx, _ = _key_points_one(ee_points, pose, switch_w, 10, euclidean_threshold, ignore_label, device)
    return kp, idx


def get_6_key_points(ee_points, pose, switch_w=True, euclidean_threshold=0.03, ignore_label=-100, *, device="cuda"):
    """:255-335 -> (key points float64 [6, 3], indices int64 [6]); two empty arrays when no point lies in the
    selection (x > -0.005, z < 0.09), as the reference returns."""
    kp, idx, empty = _key_points_one(ee_points, pose, switch_w, 6, euclidean_threshold, ignore_label, device)
    if empty:
        return np.array([]), np.array([])
    return kp, idx


def collect_closest_points(idx, points, euclidean_threshold=0.006, *, device="cuda"):
    """:338-342 -> (pcls_idx, p_idx): every pair (position k in idx, point i) with ||points[idx[k]] - points[i]|| <
    threshold in the points' dtype, ordered by k then i.  One sv_radius_labels launch over len(idx) copies of the cloud,
    copy k carrying the single anchor idx[k]."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    K, n = len(idx), len(points)
    if K == 0 or n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    if K > _lib.SV_MAX_BATCH:
        raise ValueError(f"at most {_lib.SV_MAX_BATCH} anchors per call")
    if (idx < 0).any() or (idx >= n).any():
        raise IndexError("idx out of range")
    pts = _device_points(np.asarray(points), device)
    dev = pts.device
    with torch.cuda.device(dev):
        off = torch.arange(K + 1, dtype=torch.int32, device=dev) * n
        labels = radius_labels(pts.repeat(K, 1), off, torch.from_numpy(idx).to(dev).reshape(K, 1), euclidean_threshold)
        return np.where(labels.reshape(K, n).cpu().numpy() == 0)
