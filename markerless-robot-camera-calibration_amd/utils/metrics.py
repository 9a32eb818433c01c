"""Metric definitions of the reference (utils/metrics.py), ADD on libsvhip.

compute_ADD_np            utils/metrics.py:139-150   (the reported pose accuracy)
compute_rotational_diff   :153-165, compute_translational_diff :168-176
compute_pose_dist         :18-48     (the training loops' distances; the cos2 criterion's confidence targets)
compute_segmentation_metrics  :51-107 (accuracy / precision / recall per class, balanced accuracy) + mIoU, which the
                          reference never computes on this path (BASELINE.json asks for it).
"""
from ctypes import c_int

import numpy as np
import torch

from .._lib import call, ptr, require_cuda, stream_ptr


def compute_ADD_batched(points, P, gt_pose, pred_pose, device=None):
    """points [B,Pmax,3], P int[B] in [1, Pmax] (None: Pmax), poses [B,7] (x,y,z,qw,qx,qy,qz) -> ADD [B] float64."""
    points = np.asarray(points, dtype=np.float64)
    gt_pose = np.asarray(gt_pose, dtype=np.float64)
    pred_pose = np.asarray(pred_pose, dtype=np.float64)
    if points.ndim != 3 or points.shape[2] != 3 or points.shape[1] < 1:
        raise ValueError(f"points must be B x Pmax x 3 with Pmax >= 1, got {points.shape}")
    B, Pmax, _ = points.shape
    if gt_pose.shape != (B, 7) or pred_pose.shape != (B, 7):
        raise ValueError(f"gt_pose and pred_pose must both have shape {(B, 7)}, got {gt_pose.shape} and {pred_pose.shape}")
    if P is not None:
        P = np.asarray(P, dtype=np.int32)
        if P.shape != (B,):
            raise ValueError(f"P must have shape ({B},), got {P.shape}")
        if (P < 1).any() or (P > Pmax).any():
            raise ValueError(f"P out of range: every P[b] must lie in [1, {Pmax}]")
    dev = torch.device("cuda" if device is None else device)
    pts = torch.as_tensor(np.ascontiguousarray(points)).to(dev)
    Pt = None if P is None else torch.as_tensor(P).to(dev)
    gt = torch.as_tensor(np.ascontiguousarray(gt_pose)).to(dev)
    pr = torch.as_tensor(np.ascontiguousarray(pred_pose)).to(dev)
    out = torch.empty(B, dtype=torch.float64, device=dev)
    call("sv_add_metric_batched", ptr(pts), ptr(Pt), c_int(Pmax), ptr(gt), ptr(pr), c_int(B), ptr(out), stream_ptr())
    return out.cpu().numpy()


def compute_ADD_np(points, gt_pose, pred_pose):
    return float(compute_ADD_batched(np.asarray(points)[None], None, np.asarray(gt_pose)[None],
                                     np.asarray(pred_pose)[None])[0])


def compute_rotational_diff(q1, q2, degree=True):
    diff = 2 * np.arccos(min(1.0, abs(np.sum(np.asarray(q1) * np.asarray(q2)))))
    return diff * 57.2958 if degree else diff


def compute_translational_diff(t1, t2, cm=True, method="euclidean"):
    dist = np.linalg.norm(np.asarray(t1) - np.asarray(t2)) if method == "euclidean" else -1
    return dist * 100 if cm else dist


def compute_pose_dist(gt, pred, position_voxelization=1):
    """utils/metrics.py:18-48 on [B, >=7] torch poses: (pose distance, position distance, quaternion distance up to sign,
    rotation angle acos(2 dot^2 - 1)), positions scaled by position_voxelization first.  Unlike the reference, which
    scales `gt` and `pred` in place, the arguments are left as they were."""
    with torch.no_grad():
        position = gt[:, :3] * position_voxelization
        position_pred = pred[:, :3] * position_voxelization
        orientation, orientation_pred = gt[:, 3:7], pred[:, 3:7]
        gt_n = torch.nn.functional.normalize(orientation, p=2, dim=1)
        pred_n = torch.nn.functional.normalize(orientation_pred, p=2, dim=1)
        dist = torch.norm(torch.cat((position, gt[:, 3:]), dim=1) - torch.cat((position_pred, pred[:, 3:7]), dim=1), dim=1)
        dist_position = torch.norm(position - position_pred, dim=1)
        dist_orientation = torch.min(torch.norm(orientation - orientation_pred, dim=1),
                                     torch.norm(orientation + orientation_pred, dim=1))
        angle_diff = torch.acos(2 * (torch.sum(gt_n * pred_n, dim=1) ** 2) - 1)
        return dist, dist_position, dist_orientation, angle_diff


def _qmul(q, r):
    """Hamilton product, (w, x, y, z) (utils/quaternion.py qmul_np)."""
    w0, x0, y0, z0 = q
    w1, x1, y1, z1 = r
    return np.array([w0 * w1 - x0 * x1 - y0 * y1 - z0 * z1, w0 * x1 + x0 * w1 + y0 * z1 - z0 * y1,
                     w0 * y1 - x0 * z1 + y0 * w1 + z0 * x1, w0 * z1 + x0 * y1 - y0 * x1 + z0 * w1])


def compute_pose_metrics(gt, pred):
    """utils/metrics.py:110-127: position error (m) and the rotation angle of gt * conj(pred) (rad, in [0, pi])."""
    gt, pred = np.asarray(gt, dtype=np.float64), np.asarray(pred, dtype=np.float64)
    gt_rot = gt[3:7] / np.linalg.norm(gt[3:7])
    pred_rot = pred[3:7] / np.linalg.norm(pred[3:7])
    q = _qmul(gt_rot, pred_rot * np.array([1.0, -1.0, -1.0, -1.0]))
    angle = np.abs(2 * np.arctan2(np.linalg.norm(q[1:]), q[0]))
    return {"dist_position": float(np.linalg.norm(gt[:3] - pred[:3])),
            "angle_diff": float(min(angle, 2 * np.pi - angle))}


def compute_kp_error(gt_coords, kp_coords, kp_classes):
    """utils/metrics.py:130-136: mean distance between predicted key points and the ground-truth ones of their class;
    100 when fewer than two are available."""
    if len(gt_coords) < 2 or len(kp_coords) < 2 or len(kp_classes) < 2:
        return 100
    return float(np.linalg.norm(np.asarray(gt_coords)[np.asarray(kp_classes)] - np.asarray(kp_coords), axis=1).mean())


def confusion_matrix(pred, gt, num_classes):
    pred = np.asarray(pred).astype(np.int64)
    gt = np.asarray(gt).astype(np.int64)
    valid = (gt >= 0) & (gt < num_classes)
    return np.bincount(gt[valid] * num_classes + pred[valid], minlength=num_classes ** 2).reshape(num_classes,
                                                                                                  num_classes)


def segmentation_metrics_from_confusion(cm):
    """accuracy, per-class precision / recall / IoU, mIoU, balanced accuracy ((sens + spec) / 2, metrics.py:98-102)."""
    cm = np.asarray(cm, dtype=np.float64)
    tp = np.diag(cm)
    fp = cm.sum(axis=0) - tp
    fn = cm.sum(axis=1) - tp
    tn = cm.sum() - tp - fp - fn
    with np.errstate(divide="ignore", invalid="ignore"):
        prec = np.where(tp + fp > 0, tp / (tp + fp), 0.0)
        rec = np.where(tp + fn > 0, tp / (tp + fn), 0.0)
        iou = np.where(tp + fp + fn > 0, tp / (tp + fp + fn), np.nan)
        spec = np.where(tn + fp > 0, tn / (tn + fp), 0.0)
    return {"accuracy": float(tp.sum() / max(cm.sum(), 1)), "precision": prec, "recall": rec, "iou": iou,
            "miou": float(np.nanmean(iou)), "balanced_accuracy": (rec + spec) / 2}


def compute_segmentation_metrics(gt, pred, classes=("background", "arm", "ee")):
    """utils/metrics.py:51-107, quirks included: per class accuracy/precision/recall with precision = 1 when there is no
    false positive (recall = 1 when no false negative); overall "accuracy" = (sensitivity + specificity) / 2 over the
    summed one-vs-rest counts; overall precision / recall = plain means over classes.  `miou` is this build's addition
    (BASELINE.json asks for it; the reference never computes IoU on this path)."""
    gt = np.asarray(gt)
    pred = np.asarray(pred)
    n = len(gt)
    results = {"class_results": {}}
    precisions, recalls, ious = [], [], []
    tp_s = tn_s = fp_s = fn_s = 0
    for ci, cn in enumerate(classes):
        g = gt == ci
        p = pred == ci
        tp = int((g & p).sum())
        tn = int(n - (g | p).sum())
        fp = int(p.sum()) - tp
        fn = int(g.sum()) - tp
        tp_s, tn_s, fp_s, fn_s = tp_s + tp, tn_s + tn, fp_s + fp, fn_s + fn
        precision = 1 if fp == 0 else tp / (tp + fp)
        recall = 1 if fn == 0 else tp / (tp + fn)
        results["class_results"][cn] = {"accuracy": (tp + tn) / (tp + tn + fp + fn), "precision": precision,
                                        "recall": recall}
        precisions.append(precision)
        recalls.append(recall)
        if tp + fp + fn > 0:
            ious.append(tp / (tp + fp + fn))
    sensitivity = tp_s / (tp_s + fn_s)
    specificity = tn_s / (tn_s + fp_s)
    results["accuracy"] = (sensitivity + specificity) / 2
    results["precision"] = float(np.mean(precisions))
    results["recall"] = float(np.mean(recalls))
    results["miou"] = float(np.mean(ious)) if ious else float("nan")
    return results


def _logit_rows(out):
    """[N, C] logits of a SparseTensor (train_segmentation.py passes `out`) or of a tensor (train_vote.py: out.features)"""
    return out if torch.is_tensor(out) else out.F


def compute_accuracies(out, labels, others, ignore_index=None):
    """train_segmentation.py:34-46 / train_vote.py:35-45: per frame, rows whose arg-max equals the label over the frame's
    length (ignored rows count as wrong), as a list of B Python floats.  One sv_seg_criterion call and ONE read-back for
    the batch, where the reference takes the arg-max of all N rows once per frame and leaves the device once per frame.
    `others`: the collate's list of dicts with "offset", a host sequence of B + 1 offsets or an int32 device tensor.  An
    empty frame gives NaN (the reference raises ZeroDivisionError)."""
    from .config import Config
    from .loss import seg_criterion_call

    if ignore_index is None:
        ignore_index = Config().DATA.ignore_label
    _, _, m = seg_criterion_call(_logit_rows(out), labels, others, ignore_index, want_grad=False)
    return [float(a) for a in m.to_host()["accuracies"]]


def segmentation_metrics_batch(confusion):
    """segmentation_metrics_from_confusion per frame and for the sum over frames, from the [B, C, C] counts of a
    StepMetrics (device tensor: one read-back; numpy is taken as it is): {"frames": [B dicts], "total": dict}."""
    cm = confusion.cpu().numpy() if torch.is_tensor(confusion) else np.asarray(confusion)
    if cm.ndim != 3 or cm.shape[1] != cm.shape[2]:
        raise ValueError(f"confusion must be [B, C, C], got {cm.shape}")
    return {"frames": [segmentation_metrics_from_confusion(c) for c in cm],
            "total": segmentation_metrics_from_confusion(cm.sum(axis=0))}


def compute_center_dists_batch(out, labels, coords, poses, offsets, quantization_size, ee_r=0.03):
    """train_vote.py:48-65 for the whole batch without a host wait: (dist float32 [B], valid bool [B]).  dist[b] = distance
    between get_pred_centers_batch's centre of frame b (moved by the frame's quaternion poses[b, 3:7]) and poses[b, :3], in
    float64 and rounded once; valid[b] = the frame has a row with label 1 (the reference's `continue` otherwise: its list
    holds dist[valid])."""
    from .loss import _seg_offsets
    from .output import _pred_centers_f64

    logits = require_cuda(_logit_rows(out), "out")
    off = _seg_offsets(offsets, logits.shape[0], logits.device)
    poses = torch.as_tensor(poses).to(logits.device)
    centers = _pred_centers_f64(logits, coords, off, quantization_size, ee_r, poses[:, 3:7])
    d = centers - poses[:, :3].to(torch.float64)
    dist = torch.sqrt((d * d).sum(1)).to(torch.float32)
    ones = torch.cat([torch.zeros(1, dtype=torch.int64, device=logits.device), (labels == 1).cumsum(0)])
    idx = off.to(torch.int64)
    valid = (ones[idx[1:]] - ones[idx[:-1]]) > 0
    return dist, valid
