"""Float64 restatement of the four point-matching pose losses and their gradients, written from the table of
include/sv_hip.h (N4) and sharing nothing with the package.

With n the number of unmasked rows p_j of an instance, a_j = R_pred p_j (+ t_pred) and b_j = R p_j (+ t):
    pose           r_j = a_j - b_j                              loss = sum w_j^2 |r_j|^2 / (2 n)
    shape_match    r_j = a_j - b_k*, k* = argmin_k |a_j - b_k|^2, lowest k on ties      sum w_j^2 |r_j|^2 / (2 n)
    pose_match     r_j = a_j - b_j                              loss = sum |r_j|_1 / n
    kp_pose_match  r_j = a_j - b_j                              loss = sum w_j^2 |r_j|^2 / (2 n)
    d loss / d R_pred = sum g_j p_j^T / n, d loss / d t_pred = sum g_j / n, g_j = w_j^2 r_j or sign(r_j)
"""
import numpy as np
import torch

POSE, SHAPE_MATCH, POSE_MATCH, KP_POSE_MATCH = 0, 1, 2, 3
MODES = {"pose": POSE, "shape_match": SHAPE_MATCH, "pose_match": POSE_MATCH, "kp_pose_match": KP_POSE_MATCH}


def shell_voxels(seed, n, radii=(14.0, 9.0, 6.0)):
    """n distinct integer voxel coordinates on an ellipsoid shell, int32 [n, 3]"""
    rng = np.random.default_rng(seed)
    got = np.zeros((0, 3), np.int64)
    scale = 1.0
    while len(got) < n:  # small shells run out of distinct voxels: widen
        d = rng.normal(size=(6 * n + 64, 3))
        c = np.rint(d / np.linalg.norm(d, axis=1, keepdims=True) * np.asarray(radii) * scale).astype(np.int64)
        got = np.unique(np.concatenate([got, c]), axis=0)
        scale *= 1.3
    return got[rng.permutation(len(got))[:n]].astype(np.int32)


def quat_matrix_np(q):
    """(4,) quaternion, real part first, not necessarily unit -> 3x3 float64"""
    r, i, j, k = np.asarray(q, np.float64)
    s = 2.0 / (r * r + i * i + j * j + k * k)
    return np.array([[1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r)],
                     [s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r)],
                     [s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)]])


def instance_loss_np(mode, pts, R, R_pred, t=None, t_pred=None, w=None, mask=None):
    """One instance in float64 numpy -> (loss, grad_R [3, 3], grad_t [3], match int [n_rows] (shape_match, -1 masked),
    gap: smallest relative gap between a row's best and second-best squared distance (shape_match, else None))"""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    keep = np.ones(len(pts), bool) if mask is None else np.asarray(mask).astype(bool)
    p = pts[keep]
    n = len(p)
    R, R_pred = np.asarray(R, np.float64).reshape(3, 3), np.asarray(R_pred, np.float64).reshape(3, 3)
    a, b = p @ R_pred.T, p @ R.T
    if t is not None:
        a, b = a + np.asarray(t_pred, np.float64), b + np.asarray(t, np.float64)
    w2 = np.ones(n) if w is None else np.asarray(w, np.float64)[keep] ** 2
    match, gap = None, None
    if mode == SHAPE_MATCH:
        d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
        k = d.argmin(1) if n else np.zeros(0, np.int64)  # first minimum
        if n > 1:
            two = np.partition(d, 1, axis=1)[:, :2]
            gap = float(((two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], 1e-300)).min())
        match = np.full(len(pts), -1, np.int64)
        match[keep] = np.flatnonzero(keep)[k]
        b = b[k]
    r = a - b
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == POSE_MATCH:
            g = np.sign(r)
            loss = np.abs(r).sum() / np.float64(n)
        else:
            g = w2[:, None] * r
            loss = (w2 * (r * r).sum(1)).sum() / np.float64(2 * n)
        grad_R = (g.T @ p) / np.float64(n)
        grad_t = g.sum(0) / np.float64(n)
    return loss, grad_R, grad_t, match, gap


def batch_loss_np(mode, pts, offsets, R, R_pred, t=None, t_pred=None, w=None, mask=None):
    """Every instance of a batch -> loss [B], grad_R [B, 3, 3], grad_t [B, 3], match [M] (instance-relative), gaps"""
    B = len(offsets) - 1
    loss, gR, gt, match, gaps = np.zeros(B), np.zeros((B, 3, 3)), np.zeros((B, 3)), np.full(len(pts), -1, np.int64), []
    for b in range(B):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        out = instance_loss_np(mode, pts[lo:hi], R[b], R_pred[b], None if t is None else t[b],
                               None if t is None else t_pred[b], None if w is None else w[lo:hi],
                               None if mask is None else mask[lo:hi])
        loss[b], gR[b], gt[b] = out[0], out[1], out[2]
        if out[3] is not None:
            match[lo:hi] = np.where(out[3] >= 0, out[3], -1)
        if out[4] is not None:
            gaps.append(out[4])
    return loss, gR, gt, match, gaps


def quat_matrix_torch(q):
    r, i, j, k = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    s = 2.0 / (q * q).sum(-1)
    rows = [1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r),
            s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r),
            s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)]
    return torch.stack(rows, -1).reshape(q.shape[:-1] + (3, 3))


def criterion_torch(name, y, y_pred, instances, weights=None, masks=None, reduction="mean", dtype=torch.float64):
    """The criterion `name` as a differentiable torch scalar in `dtype` (CPU): instances = list of [n_i, 3] arrays, weights /
    masks = lists of [n_i] arrays or None.  pose and shape_match use no translation; pose alone is x 1e3 under "mean"."""
    mode = MODES[name]
    y = torch.as_tensor(y).to(dtype)
    R, Rp = quat_matrix_torch(y[:, 3:7]), quat_matrix_torch(y_pred[:, 3:7].to(dtype))
    total = torch.zeros((), dtype=dtype)
    for b, pts in enumerate(instances):
        p = torch.as_tensor(np.asarray(pts)).to(dtype)
        w2 = torch.ones(len(p), dtype=dtype) if weights is None else torch.as_tensor(np.asarray(weights[b])).to(dtype) ** 2
        if masks is not None:
            keep = torch.as_tensor(np.asarray(masks[b]).astype(bool))
            p, w2 = p[keep], w2[keep]
        n = len(p)
        a, t = p @ Rp[b].T, p @ R[b].T
        if mode in (POSE_MATCH, KP_POSE_MATCH):
            a, t = a + y_pred[b, :3].to(dtype), t + y[b, :3]
        if mode == SHAPE_MATCH:
            k = ((a.detach()[:, None, :] - t.detach()[None, :, :]) ** 2).sum(-1).argmin(1)
            t = t[k]
        r = a - t
        if mode == POSE_MATCH:
            total = total + r.abs().sum() / n
        else:
            total = total + (w2 * (r * r).sum(1)).sum() / (2 * n)
    if reduction == "mean":
        total = total / len(instances)
        if name == "pose":
            total = total * 1e3
    return total


def criterion_value_and_grad(name, y, y_pred, instances, weights=None, masks=None, reduction="mean", dtype=torch.float64):
    """-> (loss float, d loss / d y_pred float64 numpy [B, 7]) of criterion_torch run in `dtype`"""
    p = torch.as_tensor(np.asarray(y_pred)[:, :7]).to(dtype).clone().requires_grad_(True)
    loss = criterion_torch(name, np.asarray(y)[:, :7], p, instances, weights, masks, reduction, dtype)
    loss.backward()
    return float(loss.detach()), p.grad.double().numpy()


def rel_err(got, want):
    """max |got - want| relative to max |want| (0 / 0 = 0)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max() if want.size else 0.0
    err = np.abs(got - want).max() if want.size else 0.0
    return float(err / scale) if scale > 0 else float(err)
