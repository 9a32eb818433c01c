"""Pose criteria of the reference (utils/loss.py:21-274): LossType and get_criterion.

The six dense criteria (mse, cos, angle, cos2, wgeodesic, smoothl1) are a few torch ops on [B, 7] tensors and are
restated in torch, oddities included.  The four point-matching criteria (pose, shape_match,
pose_match, kp_pose_match; :166-249), which the reference computes in a Python loop over the batch, are one
sv_pose_match_loss call for the whole batch: loss and gradient from the same float64 pass (include/sv_hip.h N4).  The
quaternion -> matrix step stays in torch, so autograd carries its Jacobian and non-unit quaternions behave as in the
reference.  No criterion waits on the device.

SegmentationCriterion is the criterion of the segmentation, vote and key-point trainers
(nn.CrossEntropyLoss(ignore_index, reduction) on out.features) as one sv_seg_criterion call that also yields the step's
per-frame confusion counts (StepMetrics; include/sv_hip.h N7).
"""
from ctypes import c_int, c_int64, c_size_t
from enum import Enum

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from .. import _lib
from .._lib import SvHipError, call, ptr, stream_ptr
from .config import Config
from .metrics import compute_pose_dist
from .transformation import get_quaternion_rotation_matrix_torch


class LossType(Enum):
    MSE = "mse"
    COS = "cos"
    ANGLE = "angle"
    COS2 = "cos2"
    WGEODESIC = "wgeodesic"
    SMOOTHL1 = "smoothl1"
    POSE = "pose"
    SHAPE_MATCH = "shape_match"
    POSE_MATCH = "pose_match"
    KP_POSE_MATCH = "kp_pose_match"


def qeuler(q, order="zyx", epsilon=0):
    """(*, 4) quaternions, real part first -> (*, 3) Euler angles (utils/quaternion.py:54-98; only the order the
    criteria use)."""
    if order != "zyx":
        raise NotImplementedError(f"qeuler order {order!r}: the criteria use 'zyx' only")
    assert q.shape[-1] == 4
    shape = list(q.shape)
    shape[-1] = 3
    q = q.reshape(-1, 4)
    q0, q1, q2, q3 = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    x = torch.atan2(2 * (q0 * q1 + q2 * q3), 1 - 2 * (q1 * q1 + q2 * q2))
    y = torch.asin(torch.clamp(2 * (q0 * q2 - q1 * q3), -1 + epsilon, 1 - epsilon))
    z = torch.atan2(2 * (q0 * q3 + q1 * q2), 1 - 2 * (q2 * q2 + q3 * q3))
    return torch.stack((x, y, z), dim=1).view(shape)


class PoseMatchLossFunction(torch.autograd.Function):
    """loss [B] = sv_pose_match_loss(rows, offsets, R, t; R_pred, t_pred).  The call also writes d loss[b] / d R_pred[b]
    and d t_pred[b], which the backward scales by the incoming gradient; nothing else gets a gradient."""

    @staticmethod
    def forward(ctx, R_pred, t_pred, R, t, rows, offsets, weights, mask, mode):
        B, M = R_pred.shape[0], rows.shape[0]
        dev = R_pred.device
        Rp = R_pred.detach().to(torch.float32).contiguous()
        tp = None if t_pred is None else t_pred.detach().to(torch.float32).contiguous()
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        grad_R = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
        grad_t = None if tp is None else torch.empty((B, 3), dtype=torch.float32, device=dev)
        nbytes = _lib.load().sv_pose_loss_workspace_bytes(M, B)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        call("sv_pose_match_loss", ptr(rows), ptr(offsets), c_int64(M), c_int(B), ptr(weights), ptr(mask), ptr(R), ptr(t),
             ptr(Rp), ptr(tp), c_int(mode), ptr(ws), c_size_t(nbytes), ptr(loss), ptr(grad_R), ptr(grad_t), None,
             stream_ptr())
        ctx.save_for_backward(grad_R, grad_t)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss):
        grad_R, grad_t = ctx.saved_tensors
        dR = grad_R * dloss.reshape(-1, 1, 1) if ctx.needs_input_grad[0] else None
        dt = grad_t * dloss.reshape(-1, 1) if grad_t is not None and ctx.needs_input_grad[1] else None
        return dR, dt, None, None, None, None, None, None, None


def _pinned_offsets(lengths, device):
    """int32 [len + 1] row offsets of host-known lengths, copied without a host wait"""
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32))
    return off.pin_memory().to(device, non_blocking=True)


def _check_poses(y, y_pred, x, name):
    if y.dim() != 2 or y_pred.dim() != 2 or len(y) != len(y_pred):
        raise ValueError(f"{name}: y and y_pred must be [B, >=7] with the same B, got {tuple(y.shape)} and "
                         f"{tuple(y_pred.shape)}")
    if y.shape[1] < 7 or y_pred.shape[1] < 7:
        raise ValueError(f"{name}: poses need 7 columns (x, y, z, qw, qx, qy, qz), got {y.shape[1]} and {y_pred.shape[1]}")
    if len(y) < 1 or len(y) > _lib.SV_MAX_BATCH:
        raise ValueError(f"{name}: batch of {len(y)} poses outside [1, {_lib.SV_MAX_BATCH}]")
    if x is None:
        raise ValueError(f"{name}: x (the model input the poses refer to) is required")
    if y.requires_grad:
        raise ValueError(f"{name}: the target y must not require grad (targets and points get no gradient)")
    _lib.require_cuda(y, "y")
    _lib.require_cuda(y_pred, "y_pred")


def _sparse_rows(x, B, name):
    """rows / offsets of a SparseTensor (or of a tuple holding one first: train.py:186 with joint angles) in canonical order"""
    from ..sparse import SparseTensor

    if isinstance(x, (tuple, list)) and len(x) and isinstance(x[0], SparseTensor):
        x = x[0]
    if not isinstance(x, SparseTensor):
        raise ValueError(f"{name}: x must be a SparseTensor (or a tuple starting with one), got {type(x).__name__}")
    rows = x.C[:, 1:].to(torch.float32).contiguous()
    return rows, x.coordinate_manager.batch_offsets(x.tensor_stride, B)


def _dense_rows(x, B, name):
    """rows / offsets of a [B, C, N] PointNet++ input: channels 0..2 are the coordinates"""
    if not torch.is_tensor(x) or x.dim() != 3 or x.shape[0] != B or x.shape[1] < 3:
        raise ValueError(f"{name}: with a pointnet backbone x must be a [B, >=3, N] tensor with B = {B}")
    _lib.require_cuda(x, "x")
    N = x.shape[2]
    rows = x[:, :3, :].detach().transpose(1, 2).to(torch.float32).reshape(B * N, 3).contiguous()
    return rows, torch.arange(B + 1, dtype=torch.int32, device=x.device) * N


def _kp_rows(x, labels, B, ignore_label, name):
    """rows, offsets, weights (last column) and mask (labels > ignore_label) of a [B, N, >=4] tensor or a list of
    [N_i, >=4] tensors; the mask goes to the kernel as it is: no boolean indexing, no row count read back"""
    if torch.is_tensor(x):
        if x.dim() != 3 or x.shape[0] != B or x.shape[2] < 4:
            raise ValueError(f"{name}: x must be [B, N, >=4] with B = {B} or a list of [N_i, >=4], got {tuple(x.shape)}")
        _lib.require_cuda(x, "x")
        flat = x.detach().reshape(B * x.shape[1], x.shape[2])
        offsets = torch.arange(B + 1, dtype=torch.int32, device=x.device) * x.shape[1]
    else:
        x = list(x)
        if len(x) != B or any(not torch.is_tensor(v) or v.dim() != 2 or v.shape[1] < 4 for v in x) or \
                len({v.shape[1] for v in x}) != 1:
            raise ValueError(f"{name}: x must be [B, N, >=4] or a list of B = {B} tensors [N_i, C >= 4] of one width")
        for v in x:
            _lib.require_cuda(v, "x")
        flat = torch.cat([v.detach() for v in x], dim=0)
        offsets = _pinned_offsets([v.shape[0] for v in x], flat.device)
    flat = flat.to(torch.float32)
    rows = flat[:, :3].contiguous()
    weights = flat[:, -1].contiguous()
    mask = None
    if labels is not None:
        lab = labels.reshape(-1) if torch.is_tensor(labels) else torch.cat([v.reshape(-1) for v in labels])
        if lab.shape[0] != rows.shape[0]:
            raise ValueError(f"{name}: labels hold {lab.shape[0]} entries for {rows.shape[0]} rows")
        mask = (_lib.require_cuda(lab, "labels") > ignore_label).to(torch.uint8).contiguous()
    return rows, offsets, weights, mask


def _batch_reduce(per_instance, reduction):
    return per_instance.sum() if reduction == "sum" else per_instance.sum() / per_instance.shape[0]


def get_criterion(device="cuda", loss_type=LossType.ANGLE, reduction="mean"):
    """utils/loss.py:34-274.  Returns f(y, y_pred, reduction=reduction, x=None) (kp_pose_match: also labels=None)."""
    _config = Config()
    loss_type = LossType(loss_type)
    regression_criterion = nn.MSELoss(reduction=reduction).to(device)
    cos_regression_criterion = nn.CosineSimilarity(dim=1, eps=1e-6)
    confidence_criterion = nn.BCELoss(reduction=reduction)
    smooth_l1_criterion = nn.SmoothL1Loss(reduction=reduction).to(device)

    confidence_enabled = _config()["STRUCTURE"].get("compute_confidence", False)

    gamma = 50
    gamma2 = 1

    def _reducer(reduction):
        return torch.sum if reduction == "sum" else torch.mean

    def compute_angle_loss(q_expected, q_pred, reduction=reduction, x=None):
        expected_euler = qeuler(q_expected, order="zyx", epsilon=1e-6)
        predicted_euler = qeuler(q_pred, order="zyx", epsilon=1e-6)
        angle_distance = torch.remainder(predicted_euler - expected_euler + np.pi, 2 * np.pi) - np.pi
        return _reducer(reduction)(torch.abs(angle_distance))

    def compute_cos_loss(y, y_pred, reduction=reduction, x=None):
        loss_coor = regression_criterion(y[:, :3], y_pred[:, :3])
        loss_rot = 1.0 - cos_regression_criterion(y[:, :3], y_pred[:, :3])  # columns :3 twice, as the reference
        return _reducer(reduction)(loss_rot) + loss_coor

    def compute_loss(y, y_pred, reduction=reduction, x=None):
        loss_coor = regression_criterion(y[:, :3], y_pred[:, :3])
        loss_quaternion = compute_angle_loss(y[:, 3:7], y_pred[:, 3:7])
        return gamma * loss_coor + gamma2 * loss_quaternion

    def compute_cos2_loss(y, y_pred, reduction=reduction, x=None):
        reduction_func = _reducer(reduction)
        structure = Config()()["STRUCTURE"]
        gamma_cos = 2

        loss_coor = 0
        if not structure.get("disable_position", False):
            loss_coor = regression_criterion(y[:, :3], y_pred[:, :3])

        loss_rot = 0
        if not structure.get("disable_orientation", False):
            if not structure.get("disable_position", False):
                loss_rot = reduction_func(1.0 - cos_regression_criterion(y[:, :7], y_pred[:, :7]))
            else:
                loss_rot = regression_criterion(y[:, 3:7], y_pred[:, 3:7])
            loss_rot = loss_rot * gamma_cos

        loss_confidence = 0
        if confidence_enabled:
            st = Config().STRUCTURE
            _, dist_position, _, angle_diff = compute_pose_dist(y, y_pred[:, :7])
            position_confidence_idx = (dist_position < st.position_threshold) + (dist_position > st.position_ignore_threshold)
            position_confidence = (dist_position < st.position_threshold).float()
            loss_confidence = loss_confidence + confidence_criterion(y_pred[:, 7][position_confidence_idx],
                                                                     position_confidence[position_confidence_idx])

            orientation_confidence_idx = (angle_diff < st.angle_diff_threshold) + (angle_diff > st.angle_diff_ignore_threshold)
            orientation_confidence = (angle_diff < st.angle_diff_threshold).float()
            loss_confidence = loss_confidence + confidence_criterion(y_pred[:, 8][orientation_confidence_idx],
                                                                     orientation_confidence[orientation_confidence_idx])

            overall_confidence_idx = position_confidence_idx * orientation_confidence_idx
            overall_confidence = position_confidence * orientation_confidence
            loss_confidence = loss_confidence + confidence_criterion(y_pred[:, 9][overall_confidence_idx],
                                                                     overall_confidence[overall_confidence_idx])

        return loss_rot + loss_coor + loss_confidence

    def _geodesic_family(coordinate_criterion):
        def compute(y, y_pred, reduction=reduction, x=None):
            structure = Config()()["STRUCTURE"]
            loss_coor = 0
            if not structure.get("disable_position", False):
                loss_coor = coordinate_criterion(y[:, :3], y_pred[:, :3])
            loss_rot = 0
            if not structure.get("disable_orientation", False):
                y_normalized = F.normalize(y[:, 3:7], p=2, dim=1)
                y_pred_normalized = F.normalize(y_pred[:, 3:7], p=2, dim=1)
                # acos((dot - 1) / 2), as the reference writes it (not the geodesic angle 2 acos|dot|)
                loss_rot = torch.acos((torch.sum(y_normalized * y_pred_normalized, dim=1) - 1) * 0.5)
                loss_rot = _reducer(reduction)(loss_rot)
            return loss_rot + loss_coor

        return compute

    def _point_matching(name, mode, with_translation, rows_of):
        def compute(y, y_pred, reduction, x, labels):
            _check_poses(y, y_pred, x, name)
            B = len(y)
            rows, offsets, weights, mask = rows_of(x, labels, B)
            # fp32 torch, as the reference: autograd carries the quaternion Jacobian from grad_R back to y_pred
            R = get_quaternion_rotation_matrix_torch(y[:, 3:7].detach().to(torch.float32)).contiguous()
            R_pred = get_quaternion_rotation_matrix_torch(y_pred[:, 3:7].to(torch.float32))
            t = t_pred = None
            if with_translation:
                t = y[:, :3].detach().to(torch.float32).contiguous()
                t_pred = y_pred[:, :3].to(torch.float32)
            per_instance = PoseMatchLossFunction.apply(R_pred, t_pred, R, t, rows, offsets, weights, mask, mode)
            loss = _batch_reduce(per_instance, reduction)
            if name == "pose" and reduction == "mean":
                loss = loss * 1e3  # the reference's guard against vanishing values (utils/loss.py:186), "mean" only
            return loss

        if name == "kp_pose_match":
            def compute_kp_pose_match_loss(y, y_pred, reduction=reduction, x=None, labels=None):
                return compute(y, y_pred, reduction, x, labels)

            return compute_kp_pose_match_loss

        def compute_point_loss(y, y_pred, reduction=reduction, x=None):
            return compute(y, y_pred, reduction, x, None)

        compute_point_loss.__name__ = f"compute_{name}_loss"
        return compute_point_loss

    def _pose_rows(x, labels, B):
        if str(Config().STRUCTURE.backbone).startswith("pointnet"):
            return _dense_rows(x, B, "pose") + (None, None)
        return _sparse_rows(x, B, "pose") + (None, None)

    def _kp_rows_of(x, labels, B):
        return _kp_rows(x, labels, B, Config().DATA.ignore_label, "kp_pose_match")

    if loss_type == LossType.COS:
        return compute_cos_loss
    if loss_type == LossType.MSE:
        return regression_criterion
    if loss_type == LossType.COS2:
        return compute_cos2_loss
    if loss_type == LossType.WGEODESIC:
        return _geodesic_family(regression_criterion)
    if loss_type == LossType.SMOOTHL1:
        return _geodesic_family(smooth_l1_criterion)
    if loss_type == LossType.POSE:
        return _point_matching("pose", _lib.SV_LOSS_POSE, False, _pose_rows)
    if loss_type == LossType.SHAPE_MATCH:
        assert not _config.DATA.center_at_origin
        return _point_matching("shape_match", _lib.SV_LOSS_SHAPE_MATCH, False,
                               lambda x, labels, B: _sparse_rows(x, B, "shape_match") + (None, None))
    if loss_type == LossType.POSE_MATCH:
        assert _config.DATA.voxelize_position
        return _point_matching("pose_match", _lib.SV_LOSS_POSE_MATCH, True,
                               lambda x, labels, B: _sparse_rows(x, B, "pose_match") + (None, None))
    if loss_type == LossType.KP_POSE_MATCH:
        return _point_matching("kp_pose_match", _lib.SV_LOSS_KP_POSE_MATCH, True, _kp_rows_of)
    return compute_loss


# ---- segmentation criterion and step metrics (train_segmentation.py / train_vote.py / train_key_points.py) -----------

def _seg_logits(logits):
    """float32 CUDA [N, C] with unit column stride; the row stride goes to the kernel as ld"""
    if not torch.is_tensor(logits) or logits.dim() != 2:
        raise ValueError(f"logits must be a [N, C] tensor, got {type(logits).__name__}"
                         f"{tuple(logits.shape) if torch.is_tensor(logits) else ''}")
    _lib.require_cuda(logits, "logits")
    x = logits.detach()
    N, C = x.shape
    if x.dtype != torch.float32 or (C > 1 and x.stride(1) != 1) or (N > 1 and x.stride(0) < C):
        x = x.to(torch.float32).contiguous()
    return x, (x.stride(0) if N > 1 and x.stride(0) >= C else C)


def _seg_labels(labels, N):
    if not torch.is_tensor(labels) or labels.dim() != 1 or labels.shape[0] != N:
        raise ValueError(f"labels must be a [{N}] tensor, one entry per row of logits")
    _lib.require_cuda(labels, "labels")
    if labels.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"labels must be int64 or int32, got {labels.dtype}")
    return labels.to(torch.int64).contiguous()


def _seg_offsets(offsets, N, device):
    """int32 CUDA [B + 1] row offsets from: None (one frame), an int32 device tensor, a host sequence of B + 1 offsets,
    or the `others` list of dicts with "offset" = (first row, end row) that the reference's collate yields"""
    if offsets is None:
        return _pinned_offsets([N], device)
    if torch.is_tensor(offsets) and offsets.is_cuda:
        if offsets.dim() != 1 or offsets.shape[0] < 2 or offsets.dtype not in (torch.int32, torch.int64):
            raise ValueError("offsets on the device must be an integer tensor of B + 1 >= 2 entries")
        return offsets.to(torch.int32).contiguous()
    if len(offsets) and isinstance(offsets[0], dict):
        seq = [int(oi["offset"][0]) for oi in offsets] + [int(offsets[-1]["offset"][1])]
    else:
        seq = [int(v) for v in offsets]
    if len(seq) < 2 or seq[0] != 0 or seq[-1] != N or any(b < a for a, b in zip(seq, seq[1:])):
        raise ValueError(f"offsets must rise from 0 to N = {N} over B + 1 >= 2 entries, got {seq}")
    if len(seq) - 1 > _lib.SV_MAX_BATCH:
        raise ValueError(f"{len(seq) - 1} frames: at most {_lib.SV_MAX_BATCH}")
    return _pinned_offsets(np.diff(seq), device)


class StepMetrics:
    """Per-frame counts of one criterion call, device tensors only: confusion int64 [B, C, C] ([b][gt][pred] over the
    counted rows), rows int64 [B] (frame lengths), ignored int64 [B], invalid int32 [1] (labels that are neither the ignore
    index nor a class)."""

    def __init__(self, confusion, rows, ignored, invalid):
        self.confusion, self.rows, self.ignored, self.invalid = confusion, rows, ignored, invalid

    def accuracies(self):
        """float64 [B]: trace / rows, the reference's compute_accuracies (ignored rows count as wrong); NaN for an empty
        frame, where the reference raises ZeroDivisionError"""
        trace = self.confusion.diagonal(dim1=1, dim2=2).sum(1)
        return trace.to(torch.float64) / self.rows.to(torch.float64)

    def to_host(self):
        """the one read-back: dict of numpy arrays (confusion, rows, ignored, invalid, accuracies)"""
        B, C, _ = self.confusion.shape
        flat = torch.cat([self.confusion.reshape(-1), self.rows, self.ignored, self.invalid.to(torch.int64)]).cpu().numpy()
        confusion = flat[:B * C * C].reshape(B, C, C)
        rows = flat[B * C * C:B * C * C + B]
        with np.errstate(divide="ignore", invalid="ignore"):
            acc = np.trace(confusion, axis1=1, axis2=2).astype(np.float64) / rows.astype(np.float64)
        return {"confusion": confusion, "rows": rows, "ignored": flat[B * C * C + B:B * C * C + 2 * B],
                "invalid": int(flat[-1]), "accuracies": acc}


def seg_criterion_call(logits, labels, offsets=None, ignore_index=-100, want_grad=True, want_metrics=True):
    """One sv_seg_criterion call: (sums float64 [2], grad float32 [N, C] or None, StepMetrics; its confusion and ignored are
    None without want_metrics).  No host wait."""
    x, ld = _seg_logits(logits)
    N, C = x.shape
    y = _seg_labels(labels, N)
    off = _seg_offsets(offsets, N, x.device)
    B = off.shape[0] - 1
    dev = x.device
    sums = torch.empty(2, dtype=torch.float64, device=dev)
    grad = torch.empty((N, C), dtype=torch.float32, device=dev) if want_grad else None
    ncell = B * C * C if want_metrics else 0
    counts = torch.empty(ncell + (B if want_metrics else 0) + 1, dtype=torch.int64, device=dev)
    confusion = counts[:ncell].view(B, C, C) if want_metrics else None
    ignored = counts[ncell:ncell + B] if want_metrics else None
    invalid = counts[-1:].view(torch.int32)[:1]
    nbytes = _lib.load().sv_seg_criterion_workspace_bytes(N, B, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    call("sv_seg_criterion", ptr(x), c_int64(ld), c_int(C), c_int64(N), ptr(y), c_int64(ignore_index), ptr(off), c_int(B),
         ptr(ws), c_size_t(nbytes), ptr(sums), ptr(grad), ptr(confusion), ptr(ignored), ptr(invalid), stream_ptr())
    rows = (off[1:] - off[:-1]).to(torch.int64) if want_metrics else None
    return sums, grad, StepMetrics(confusion, rows, ignored, invalid)


class SegmentationLossFunction(torch.autograd.Function):
    """loss = sum or mean over the counted rows of lse(x) - x[y].  The call also writes the unscaled d loss / d logits
    (softmax - onehot), which the backward multiplies by the reduction's factor and the incoming gradient; the integer
    outputs carry no gradient."""

    @staticmethod
    def forward(ctx, logits, labels, offsets, ignore_index, mean, want_metrics):
        sums, grad, m = seg_criterion_call(logits, labels, offsets, ignore_index, ctx.needs_input_grad[0], want_metrics)
        loss = sums[0] / sums[1] if mean else sums[0]  # 0 / 0: NaN, as torch's mean over no row
        loss = torch.where(m.invalid[0] != 0, torch.full_like(loss, float("nan")), loss).to(torch.float32)
        ctx.scale = 1.0 / sums[1].clamp(min=1.0) if mean else None  # no counted row: the gradient rows stay 0 (or NaN)
        ctx.in_dtype = logits.dtype
        if grad is not None:
            ctx.save_for_backward(grad)
        outs = (loss, m.invalid) + ((m.confusion, m.rows, m.ignored) if want_metrics else ())
        ctx.mark_non_differentiable(*outs[1:])
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss, *_):
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        (grad,) = ctx.saved_tensors
        factor = dloss if ctx.scale is None else dloss.to(torch.float64) * ctx.scale
        return ((grad * factor.to(torch.float32)).to(ctx.in_dtype),) + (None,) * 5


class SegmentationCriterion(nn.Module):
    """nn.CrossEntropyLoss(ignore_index=..., reduction=...) on [N, C] logits as one sv_seg_criterion call (include/sv_hip.h
    N7): loss, gradient and the per-frame confusion counts from one float64 pass, no host wait.
    forward(logits, labels) -> loss (0-dim float32); forward(logits, labels, offsets=..., return_metrics=True) ->
    (loss, StepMetrics)."""

    def __init__(self, ignore_index=-100, reduction="mean"):
        super().__init__()
        if reduction not in ("mean", "sum"):
            raise ValueError(f"reduction {reduction!r}: 'mean' or 'sum' (the trainers call .item() on the loss)")
        self.ignore_index, self.reduction = int(ignore_index), reduction

    def forward(self, logits, labels, offsets=None, return_metrics=False):
        out = SegmentationLossFunction.apply(logits, labels, offsets, self.ignore_index, self.reduction == "mean",
                                             bool(return_metrics))
        if not return_metrics:
            return out[0]
        return out[0], StepMetrics(out[2], out[3], out[4], out[1])
