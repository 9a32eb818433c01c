"""PointNet++ sampling / grouping with the reference's names (model/pointnet2_utils.py) on libsvhip.

farthest_point_sample(xyz [B,N,3], npoint) -> int64 [B,npoint]     reference :65-86 (python loop of npoint launches)
query_ball_point(radius, nsample, xyz, new_xyz) -> int64 [B,S,nsample]   reference :89-109 ([B,S,N] matrix + sort)
query_ball_point_multi(radii, nsamples, xyz, new_xyz) -> R of those      one scan for a multi-scale layer's radii
index_points, square_distance: thin torch helpers with the reference's semantics (:21-62).
set_training_path(model, "torch" | "hip"): which kernels the set abstraction / feature propagation layers and the
PointNet++ heads train on (default "torch": the reference's torch expressions).
"""
from ctypes import c_double, c_int, c_int64, c_void_p

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from .. import nn as svnn
from .._lib import (SV_ACT_RELU, SV_BQ_MAX_RADII, SV_GROUP_MSG, SV_GROUP_SSG, call, ptr, require_cuda,
                    stream_ptr)


def farthest_point_sample(xyz, npoint, start=None):
    require_cuda(xyz, "xyz")
    B, N, C = xyz.shape
    x = xyz[..., :3].to(torch.float32).contiguous()
    if start is None:  # the reference: torch.randint(0, N, (B,))
        start = torch.randint(0, N, (B,), dtype=torch.long, device=xyz.device)
    start = start.to(device=xyz.device, dtype=torch.int64).contiguous()
    out = torch.empty((B, npoint), dtype=torch.int64, device=xyz.device)
    call("sv_fps", ptr(x), c_int(B), c_int(N), c_int(npoint), ptr(start), ptr(out), stream_ptr())
    return out


def query_ball_point(radius, nsample, xyz, new_xyz):
    require_cuda(xyz, "xyz")
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    x = xyz.to(torch.float32).contiguous()
    q = new_xyz.to(torch.float32).contiguous()
    out = torch.empty((B, S, nsample), dtype=torch.int64, device=xyz.device)
    call("sv_ball_query", ptr(x), ptr(q), c_int(B), c_int(N), c_int(S), c_double(float(radius)), c_int(nsample),
         ptr(out), stream_ptr())
    return out


def query_ball_point_multi(radius_list, nsample_list, xyz, new_xyz):
    """[query_ball_point(radius_list[r], nsample_list[r], xyz, new_xyz) for r], the radii of one multi-scale layer in one
    scan over the cloud per launch (sv_ball_query_multi, up to SV_BQ_MAX_RADII radii a launch); bit-identical per radius."""
    require_cuda(xyz, "xyz")
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    x = xyz.to(torch.float32).contiguous()
    q = new_xyz.to(torch.float32).contiguous()
    outs = [torch.empty((B, S, k), dtype=torch.int64, device=xyz.device) for k in nsample_list]
    for r0 in range(0, len(outs), SV_BQ_MAX_RADII):
        rs = range(r0, min(r0 + SV_BQ_MAX_RADII, len(outs)))
        call("sv_ball_query_multi", ptr(x), ptr(q), c_int(B), c_int(N), c_int(S), c_int(len(rs)),
             (c_double * len(rs))(*[float(radius_list[r]) for r in rs]), (c_int * len(rs))(*[nsample_list[r] for r in rs]),
             (c_void_p * len(rs))(*[outs[r].data_ptr() for r in rs]), stream_ptr())
    return outs


def index_points(points, idx):
    B = points.shape[0]
    view = [B] + [1] * (idx.dim() - 1)
    batch = torch.arange(B, dtype=torch.long, device=points.device).view(view).expand_as(idx)
    return points[batch, idx, :]


def square_distance(src, dst):
    dist = -2 * torch.matmul(src, dst.permute(0, 2, 1))
    dist += torch.sum(src ** 2, -1).unsqueeze(-1)
    dist += torch.sum(dst ** 2, -1).unsqueeze(1)
    return dist


def sample_and_group_all(xyz, points):
    B, N, C = xyz.shape
    new_xyz = torch.zeros(B, 1, C, device=xyz.device)
    grouped = xyz.view(B, 1, N, C)
    new_points = grouped if points is None else torch.cat([grouped, points.view(B, 1, N, -1)], dim=-1)
    return new_xyz, new_points


def _group(xyz, points, new_xyz, idx, order):
    """the grouped tensor [B, S, nsample, 3 + D]: SV_GROUP_SSG [xyz[idx] - new_xyz, points[idx]] (reference :131-137) or
    SV_GROUP_MSG [points[idx], xyz[idx] - new_xyz] (the multi-scale grouping's order, features first, :245-250);
    idx None is group_all: every point once, as it is (:143-160)"""
    if idx is None:
        return sample_and_group_all(xyz, points)[1]
    B, S, C = new_xyz.shape
    grouped_xyz = index_points(xyz, idx) - new_xyz.view(B, S, 1, C)
    if points is None:
        return grouped_xyz
    feats = index_points(points, idx)
    return torch.cat([grouped_xyz, feats] if order == SV_GROUP_SSG else [feats, grouped_xyz], dim=-1)


def sample_and_group(npoint, radius, nsample, xyz, points, returnfps=False, fps_start=None):
    """reference :112-140.  fps_start int64 [B] pins the first centroids (None: drawn as the reference draws them)."""
    fps_idx = farthest_point_sample(xyz, npoint, start=fps_start)
    new_xyz = index_points(xyz, fps_idx)
    idx = query_ball_point(radius, nsample, xyz, new_xyz)
    new_points = _group(xyz, points, new_xyz, idx, SV_GROUP_SSG)
    if returnfps:
        return new_xyz, new_points, index_points(xyz, idx), fps_idx
    return new_xyz, new_points


# ----------------------------------------------------------------------------------------------------------------------
# set abstraction / feature propagation modules (reference :163-317).  Parameter names are the reference's
# (mlp_convs.i = nn.Conv2d / nn.Conv1d 1x1, mlp_bns.i = BatchNorm) so its checkpoints load by key; in eval mode the
# shared MLPs run as dense rows through the fp32-MFMA kernel with the BatchNorm folded into the epilogue.
# ----------------------------------------------------------------------------------------------------------------------
def _fold_conv_bn(conv, bn):
    """1x1 conv or Linear (+bias) followed by BatchNorm(eval) -> W[1,Cin,Cout], scale, shift with the bias folded in."""
    w = conv.weight.detach().reshape(conv.weight.shape[0], -1).t().contiguous().unsqueeze(0)  # Conv 1x1 or Linear
    g = bn.weight.detach().float().cpu().numpy()
    b = bn.bias.detach().float().cpu().numpy()
    mean = bn.running_mean.detach().float().cpu().numpy()
    var = bn.running_var.detach().float().cpu().numpy()
    scale = (g / np.sqrt(var + np.float32(bn.eps))).astype(np.float32)
    cb = conv.bias.detach().float().cpu().numpy() if conv.bias is not None else np.zeros_like(mean)
    shift = (b + (cb - mean) * scale).astype(np.float32)
    dev = conv.weight.device
    return w, torch.from_numpy(scale).to(dev), torch.from_numpy(shift).to(dev)


def _fold_mlp(convs, bns):
    return [_fold_conv_bn(conv, bn) for conv, bn in zip(convs, bns)]


def _mlp_rows(rows, convs, bns, folds=None):
    """rows [R, Cin] -> relu(bn(conv(.))) stack, one fused launch per layer (folds: the layers' _fold_conv_bn results)."""
    for w, scale, shift in folds if folds is not None else _fold_mlp(convs, bns):
        rows = svnn.conv_forward(rows, w, None, rows.shape[0], scale, shift, None, SV_ACT_RELU)
    return rows


class FoldCache(nn.Module):
    """Eval-mode modules whose Conv + BatchNorm pairs run folded (W, scale, shift): the folds are computed once (host
    arithmetic of _fold_conv_bn, i.e. one read-back of the BatchNorm tensors) and reused, so an eval forward after the
    first one has no host synchronisation.  Dropped on train() / eval(), load_state_dict and .to() / _apply; an in-place
    change of a parameter or buffer (its version counter) also rebuilds them."""

    def _folds_drop(self):
        self.__dict__["_fold_cache"] = None

    def _fold_get(self, build, modules=None):
        """build() once; rebuilt when a parameter or buffer of `modules` (default: the whole module) changed in place"""
        mods = (self,) if modules is None else modules
        ver = svnn._tensor_versions(*(t for m in mods for t in (*m.parameters(), *m.buffers())))
        cache = self.__dict__.get("_fold_cache")
        if cache is None or cache[0] != ver:
            cache = (ver, build())
            self.__dict__["_fold_cache"] = cache
        return cache[1]

    def train(self, mode=True):
        self._folds_drop()
        return super().train(mode)

    def _apply(self, fn, *args, **kwargs):
        self._folds_drop()
        return super()._apply(fn, *args, **kwargs)

    def _load_from_state_dict(self, *args, **kwargs):
        self._folds_drop()
        return super()._load_from_state_dict(*args, **kwargs)


# ----------------------------------------------------------------------------------------------------------------------
# training on libsvhip (set_training_path(model, "hip")): the grouped rows, the max over a group and the
# 3-NN interpolation are HIP kernels with fixed-order backwards (no atomics: bit-reproducible gradients); the shared
# MLPs stay rows [B*S*nsample, C] from the gather to the max, every 1x1 conv / linear layer on sv_conv_fwd /
# sv_conv_wgrad (nn.sparse_conv dense rows), BatchNorm as F.batch_norm on the rows, ReLU / Dropout torch ops.
# Coordinates are not differentiated: a call whose coordinates require grad runs the torch path (recorded).
# ----------------------------------------------------------------------------------------------------------------------
TRAINING_PATHS = ("torch", "hip")


def set_training_path(model, path):
    """Mark every PointNetSetAbstraction(Msg) / PointNetFeaturePropagation of `model` (itself included) and the heads of
    PointNet2SSG / PointNet2MSGEncoder to train on `path`: "torch" (the default, the reference's torch expressions) or
    "hip".  Affects train() alone (eval() keeps the fused kernels); a plain attribute, not in state_dict, kept by .to(),
    load_state_dict and train() / eval().  Returns the qualified names of the modules it switched."""
    if path not in TRAINING_PATHS:
        raise ValueError(f"training path must be one of {TRAINING_PATHS}, got {path!r}")
    names = []
    for name, m in model.named_modules():
        if getattr(type(m), "_hip_trainable", False):
            m.training_path = path
            names.append(name)
    return names


def _hip_train(module, *coords):
    """whether this call of `module` trains on the HIP path; coordinates that require grad take the torch path for the
    call, counted in module.train_fallbacks and recorded in profiling.TRAIN_LOG as (module, "fallback", "torch")"""
    if not module.training or module.__dict__.get("training_path", "torch") != "hip":
        return False
    if any(c is not None and c.requires_grad for c in coords):
        module.__dict__["train_fallbacks"] = module.__dict__.get("train_fallbacks", 0) + 1
        svnn._train_log(module, "fallback", "torch")
        return False
    return True


def _csr(idx, N, module):
    """sv_index_transpose: (offsets int32 [B*N + 1], pos int32 [B*M]) of the index table idx [B, ...] (values in [0, N))"""
    B = idx.shape[0]
    M = idx.numel() // max(B, 1)
    lib = _lib.load()
    nbytes = lib.sv_index_transpose_workspace_bytes(B, M, N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=idx.device)
    offsets = torch.empty(B * N + 1, dtype=torch.int32, device=idx.device)
    pos = torch.empty(max(B * M, 1), dtype=torch.int32, device=idx.device)
    _lib._check(lib.sv_index_transpose(ptr(idx), idx.element_size(), B, M, N, ptr(ws), nbytes, ptr(offsets), ptr(pos),
                                       stream_ptr()), "sv_index_transpose")
    svnn._train_log(module, "index_transpose", "sv_index_transpose")
    return offsets, pos


def _gather_transpose(csr, w, rows, col0, C, per_row, T, module):
    """out [T, C]: out[t] = sum over the CSR positions p of target t (ascending) of w[p] * rows[p / per_row, col0:col0+C]"""
    offsets, pos = csr
    out = torch.empty((T, C), dtype=torch.float32, device=rows.device)
    call("sv_gather_transpose", ptr(offsets), ptr(pos), ptr(w), ptr(rows), c_int64(rows.stride(0)), c_int(col0), c_int(C),
         c_int(per_row), c_int64(T), ptr(out), c_int64(C), stream_ptr())
    svnn._train_log(module, "gather_transpose", "sv_gather_transpose")
    return out


class GroupRowsFunction(torch.autograd.Function):
    """rows [B*S*nsample, 3 + D] = sv_group_rows (order SV_GROUP_SSG / SV_GROUP_MSG; idx None: group_all).  Backward to
    the point features only: the CSR of idx (sv_index_transpose, built once) and sv_gather_transpose over the feature
    columns; group_all's rows hold every point once, so its gradient is the column slice."""

    @staticmethod
    def forward(ctx, points, xyz, new_xyz, idx, order, module):
        B, N, _ = xyz.shape
        S, K = (1, N) if idx is None else (idx.shape[1], idx.shape[2])
        D = 0 if points is None else points.shape[2]
        x = xyz.detach().to(torch.float32).contiguous()
        p = points.detach().contiguous() if points is not None else None
        q = new_xyz.detach().to(torch.float32).contiguous() if idx is not None else None
        out = torch.empty((B * S * K, 3 + D), dtype=torch.float32, device=xyz.device)
        call("sv_group_rows", ptr(x), ptr(p), ptr(q), ptr(idx), c_int(B), c_int(N), c_int(D), c_int(S), c_int(K),
             c_int(order), c_int(3 + D), ptr(out), stream_ptr())
        svnn._train_log(module, "group_rows", "sv_group_rows")
        ctx.save_for_backward(idx)
        ctx.shape, ctx.col0, ctx.module = (B, N, D), (3 if order == SV_GROUP_SSG else 0), module
        return out

    @staticmethod
    def backward(ctx, drows):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        (idx,) = ctx.saved_tensors
        B, N, D = ctx.shape
        if drows.stride(1) != 1:
            drows = drows.contiguous()
        if idx is None:  # group_all: row (b, k) = [xyz[b][k], points[b][k]]
            dp = drows.view(B, N, 3 + D)[:, :, 3:]
        else:
            dp = _gather_transpose(_csr(idx, N, ctx.module), None, drows, ctx.col0, D, 1, B * N, ctx.module).view(B, N, D)
        return dp, None, None, None, None, None


class GroupMaxFunction(torch.autograd.Function):
    """pooled [G, C] = max over every group of nsample consecutive rows (sv_group_max: the first NaN wins, a tie goes to
    the lowest row); backward: the dense row gradient, dPooled at the argmax, in one pass (sv_group_max_backward)"""

    @staticmethod
    def forward(ctx, rows, nsample, module):
        R, C = rows.shape
        if rows.stride(1) != 1:
            rows = rows.contiguous()
        G = R // nsample
        out = torch.empty((G, C), dtype=torch.float32, device=rows.device)
        arg = torch.empty((G, C), dtype=torch.int32, device=rows.device)
        call("sv_group_max", ptr(rows), c_int64(rows.stride(0)), c_int64(G), c_int(nsample), c_int(C), ptr(out), ptr(arg),
             stream_ptr())
        svnn._train_log(module, "group_max", "sv_group_max")
        ctx.save_for_backward(arg)
        ctx.nsample, ctx.module = nsample, module
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, dpooled, _darg):
        (arg,) = ctx.saved_tensors
        G, C = arg.shape
        dp = dpooled.contiguous()
        drows = torch.empty((G * ctx.nsample, C), dtype=torch.float32, device=dp.device)
        call("sv_group_max_backward", ptr(dp), ptr(arg), c_int64(G), c_int(ctx.nsample), c_int(C), ptr(drows),
             stream_ptr())
        svnn._train_log(ctx.module, "group_max_backward", "sv_group_max_backward")
        return drows, None, None


class ThreeNNGatherFunction(torch.autograd.Function):
    """out [B, N, C] = (p2[i0] * w0 + p2[i1] * w1) + p2[i2] * w2 (sv_three_nn_gather: sv_three_nn_interpolate's bits);
    backward to points2: the CSR of idx (sv_index_transpose) and sv_gather_transpose with the weights"""

    @staticmethod
    def forward(ctx, points2, idx, w, module):
        B, N, _ = idx.shape
        S, C = points2.shape[1], points2.shape[2]
        p2 = points2.detach().contiguous()
        out = torch.empty((B, N, C), dtype=torch.float32, device=p2.device)
        call("sv_three_nn_gather", ptr(p2), ptr(idx), ptr(w), c_int(B), c_int(N), c_int(S), c_int(C), ptr(out),
             stream_ptr())
        svnn._train_log(module, "three_nn_gather", "sv_three_nn_gather")
        ctx.save_for_backward(idx, w)
        ctx.S, ctx.module = S, module
        return out

    @staticmethod
    def backward(ctx, dout):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        idx, w = ctx.saved_tensors
        B, N, _ = idx.shape
        d = dout.contiguous().view(B * N, -1)
        dp2 = _gather_transpose(_csr(idx, ctx.S, ctx.module), w, d, 0, d.shape[1], 3, B * ctx.S, ctx.module)
        return dp2.view(B, ctx.S, -1), None, None, None


def group_rows(xyz, points, new_xyz, idx, order, module=None):
    """differentiable sv_group_rows (gradient to `points` only) -> rows [B*S*nsample, 3 + D]"""
    if points is not None and points.dtype != torch.float32:
        points = points.to(torch.float32)
    return GroupRowsFunction.apply(points, xyz, new_xyz, idx, order, module)


def group_max(rows, nsample, module=None):
    """differentiable sv_group_max -> [R / nsample, C] (the argmax indices are kept for the backward)"""
    return GroupMaxFunction.apply(rows, nsample, module)[0]


def three_nn(xyz1, xyz2, module=None):
    """sv_three_nn: (idx int32 [B, N, 3], w float32 [B, N, 3]) of the 3-NN interpolation of xyz2 onto xyz1"""
    B, N, _ = xyz1.shape
    S = xyz2.shape[1]
    x1, x2 = (t.detach().to(torch.float32).contiguous() for t in (xyz1, xyz2))
    idx = torch.empty((B, N, 3), dtype=torch.int32, device=x1.device)
    w = torch.empty((B, N, 3), dtype=torch.float32, device=x1.device)
    call("sv_three_nn", ptr(x1), ptr(x2), c_int(B), c_int(N), c_int(S), ptr(idx), ptr(w), stream_ptr())
    svnn._train_log(module, "three_nn", "sv_three_nn")
    return idx, w


def three_nn_gather(points2, idx, w, module=None):
    """differentiable sv_three_nn_gather (gradient to points2)"""
    if points2.dtype != torch.float32:
        points2 = points2.to(torch.float32)
    return ThreeNNGatherFunction.apply(points2, idx, w, module)


def conv_rows_train(rows, layer):
    """1x1 Conv1d / Conv2d or Linear on rows [R, Cin] -> [R, Cout]: nn.sparse_conv dense rows (forward sv_conv_fwd, dX
    sv_conv_fwd with W^T, dW sv_conv_wgrad, d bias a column sum); the gradient flows back through the weight's view.
    profiling.TRAIN_LOG records its ops as (layer, "fwd" / "dx" / "dw", entry point)."""
    if rows.stride(1) != 1:
        rows = rows.contiguous()
    w = layer.weight.view(layer.weight.shape[0], -1).t().unsqueeze(0)
    return svnn.sparse_conv(rows, w, layer.bias, None, rows.shape[0], lambda: None, layer=layer)


def bn_rows_train(bn, rows):
    """BatchNorm1d / BatchNorm2d.forward on rows [R, C] (what the module computes on [B, C, ...] with R = the product of
    the other dimensions): the same num_batches_tracked / momentum=None bookkeeping, F.batch_norm with its parameters"""
    eaf = 0.0 if bn.momentum is None else bn.momentum
    if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
        eaf = 1.0 / float(bn.num_batches_tracked) if bn.momentum is None else bn.momentum
    batch_stats = bn.training or (bn.running_mean is None and bn.running_var is None)
    keep = not bn.training or bn.track_running_stats
    return F.batch_norm(rows, bn.running_mean if keep else None, bn.running_var if keep else None, bn.weight, bn.bias,
                        batch_stats, eaf, bn.eps)


def _mlp_rows_train(rows, convs, bns):
    for conv, bn in zip(convs, bns):
        rows = F.relu(bn_rows_train(bn, conv_rows_train(rows, conv)))
    return rows


def _cat(tensors, dim):
    return tensors[0] if len(tensors) == 1 else torch.cat(tensors, dim=dim)


class _SetAbstraction(FoldCache):
    """What PointNetSetAbstraction and PointNetSetAbstractionMsg share - everything but the parameter names and the fused
    entry point.  A layer is a list of scales (radius, nsample, convs, bns) around the same farthest-point centroids,
    grouped in the column order `_order`, the pooled features concatenated; single-scale is a list of one scale in the
    order SV_GROUP_SSG.  Eval on the GPU: sv_fps, the ball query, then the fused kernel (all scales in one launch); shapes
    it declines, `fused = False` or group_all run every scale's layers one launch each (sv_conv_fwd dense rows),
    torch.max and torch.cat - the same bits."""

    _hip_trainable = True  # set_training_path
    _order = SV_GROUP_SSG
    group_all = False  # one group of all points around the origin instead of sampled balls (single-scale only)

    def __init__(self):
        super().__init__()
        self.fused = True  # False: the unfused eval path (tests, timing)

    def _scales(self):
        """[(radius, nsample, convs, bns)]"""
        raise NotImplementedError

    def _launch_fused(self, x, p, q, idxs, B, N, D, S, packed, host, out):
        """the class's fused entry point on every scale -> its return code"""
        raise NotImplementedError

    def _folded(self):
        """(per-scale layer folds, per-scale packed parameters, host arrays (nsamples, params, widths, nlayers) of the
        fused entry point) - built once per weights / device"""
        def build():
            scales = self._scales()
            folds = [_fold_mlp(convs, bns) for _, _, convs, bns in scales]
            packed = [torch.cat([t.reshape(-1).to(torch.float32) for f in fs for t in f]).contiguous() for fs in folds]
            widths = [w for _, _, convs, _ in scales for w in [convs[0].in_channels] + [c.out_channels for c in convs]]
            R = len(scales)
            host = ((c_int * R)(*[k or 0 for _, k, _, _ in scales]), (c_void_p * R)(*[p.data_ptr() for p in packed]),
                    (c_int * len(widths))(*widths), (c_int * R)(*[len(convs) for _, _, convs, _ in scales]))
            return folds, packed, host

        return self._fold_get(build)

    def _fused(self, xyz, points, new_xyz, idxs, folds):
        """every scale's gather + shared MLP + max in one launch -> [B, S, sum C_r], or None where the kernel does not
        cover the shapes (SV_ERR_UNSUPPORTED: nothing was launched, the caller runs the layers one by one).  idxs: the
        scales' ball-query tables (a single scale's may come bare)."""
        _, packed, host = folds
        idxs = [idxs] if torch.is_tensor(idxs) else idxs
        B, N, _ = xyz.shape
        S = new_xyz.shape[1]
        x = xyz.to(torch.float32).contiguous()
        p = points.to(torch.float32).contiguous() if points is not None else None
        D = p.shape[2] if p is not None else 0
        if host[2][0] != 3 + D:
            raise ValueError(f"set abstraction expects {host[2][0] - 3} point features, got {D}")
        q = new_xyz.to(torch.float32).contiguous()
        ctot = sum(convs[-1].out_channels for _, _, convs, _ in self._scales())
        out = torch.empty((B, S, ctot), dtype=torch.float32, device=xyz.device)
        rc = self._launch_fused(x, p, q, idxs, B, N, D, S, packed, host, out)
        if rc == _lib.SV_ERR_UNSUPPORTED:
            return None
        _lib._check(rc, self._entry)
        return out

    # ---- one scale, from its ball-query table to its pooled features
    def _pool_eval(self, xyz, points, new_xyz, idx, convs, bns, folds):
        """unfused eval: the layers one launch each (dense rows), then torch.max -> [B, S, C']"""
        grouped = _group(xyz, points, new_xyz, idx, self._order)
        B, S, Kn, C = grouped.shape
        rows = _mlp_rows(grouped.reshape(B * S * Kn, C).contiguous(), convs, bns, folds)
        return rows.view(B, S, Kn, -1).max(dim=2)[0]

    def _pool_train_hip(self, xyz, points, new_xyz, idx, convs, bns):
        """train() on the HIP path: sv_group_rows -> shared MLP on rows -> sv_group_max -> [B, S, C']"""
        B, S = new_xyz.shape[0], new_xyz.shape[1]
        rows = group_rows(xyz, points, new_xyz, idx, self._order, self)
        rows = _mlp_rows_train(rows, convs, bns)
        return group_max(rows, rows.shape[0] // (B * S), self).view(B, S, -1)

    def _pool_train_torch(self, xyz, points, new_xyz, idx, convs, bns):
        """train() on the reference's torch expressions (:194-203 / :247-258) -> [B, C', S]"""
        t = _group(xyz, points, new_xyz, idx, self._order).permute(0, 3, 2, 1)
        for conv, bn in zip(convs, bns):
            t = F.relu(bn(conv(t)))
        return torch.max(t, 2)[0]

    def forward(self, xyz, points, fps_start=None):
        """xyz [B,3,N], points [B,D,N] or None -> new_xyz [B,3,S], new_points [B, sum C_r, S].  fps_start int64 [B] pins
        the first farthest-point centroids (None: drawn as the reference draws them, torch.randint on the device)."""
        hip = _hip_train(self, xyz)
        xyz = xyz.permute(0, 2, 1)
        if points is not None:
            points = points.permute(0, 2, 1)
        scales = self._scales()
        if self.group_all:
            new_xyz, idxs = torch.zeros(xyz.shape[0], 1, xyz.shape[2], device=xyz.device), [None]
        else:  # sampling and ball query on libsvhip, the same groups on every path
            new_xyz = index_points(xyz, farthest_point_sample(xyz, self.npoint, start=fps_start))
            if len(scales) == 1:
                idxs = [query_ball_point(scales[0][0], scales[0][1], xyz, new_xyz)]
            else:
                idxs = query_ball_point_multi([r for r, _, _, _ in scales], [k for _, k, _, _ in scales], xyz, new_xyz)
        args = [(xyz, points, new_xyz, idx, convs, bns) for idx, (_, _, convs, bns) in zip(idxs, scales)]
        if hip:
            pooled = _cat([self._pool_train_hip(*a) for a in args], -1)
        elif self.training:
            return new_xyz.permute(0, 2, 1), _cat([self._pool_train_torch(*a) for a in args], 1)
        else:
            folds = self._folded()
            fused = self.fused and not self.group_all and xyz.is_cuda
            pooled = self._fused(xyz, points, new_xyz, idxs, folds) if fused else None
            if pooled is None:
                pooled = _cat([self._pool_eval(*a, f) for a, f in zip(args, folds[0])], -1)
        return new_xyz.permute(0, 2, 1), pooled.permute(0, 2, 1)  # [B, D', S]


class PointNetSetAbstraction(_SetAbstraction):
    """reference :163-204; fused eval kernel sv_pointnet_sa"""

    _entry = "sv_pointnet_sa"

    def __init__(self, npoint, radius, nsample, in_channel, mlp, group_all):
        super().__init__()
        self.npoint, self.radius, self.nsample, self.group_all = npoint, radius, nsample, group_all
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last = in_channel
        for out in mlp:
            self.mlp_convs.append(nn.Conv2d(last, out, 1))
            self.mlp_bns.append(nn.BatchNorm2d(out))
            last = out

    def _scales(self):
        return [(self.radius, self.nsample, self.mlp_convs, self.mlp_bns)]

    def _launch_fused(self, x, p, q, idxs, B, N, D, S, packed, host, out):
        nsamples, _, widths, nlayers = host
        return _lib.load().sv_pointnet_sa(ptr(x), ptr(p), ptr(q), ptr(idxs[0]), B, N, D, S, nsamples[0], ptr(packed[0]),
                                          widths, nlayers[0], ptr(out), stream_ptr())


class PointNetSetAbstractionMsg(_SetAbstraction):
    """Multi-scale grouping (reference :207-264): R radii around the same farthest-point centroids, one shared MLP per
    radius.  Parameter names conv_blocks.i.j / bn_blocks.i.j as in the reference.  Fused eval kernel
    sv_pointnet_sa_msg, nsample up to 128."""

    _entry = "sv_pointnet_sa_msg"
    _order = SV_GROUP_MSG

    def __init__(self, npoint, radius_list, nsample_list, in_channel, mlp_list):
        super().__init__()
        self.npoint = npoint
        self.radius_list = list(radius_list)
        self.nsample_list = list(nsample_list)
        self.conv_blocks = nn.ModuleList()
        self.bn_blocks = nn.ModuleList()
        for mlp in mlp_list:
            convs, bns = nn.ModuleList(), nn.ModuleList()
            last = in_channel + 3
            for out in mlp:
                convs.append(nn.Conv2d(last, out, 1))
                bns.append(nn.BatchNorm2d(out))
                last = out
            self.conv_blocks.append(convs)
            self.bn_blocks.append(bns)

    def _scales(self):
        return list(zip(self.radius_list, self.nsample_list, self.conv_blocks, self.bn_blocks))

    def _launch_fused(self, x, p, q, idxs, B, N, D, S, packed, host, out):
        nsamples, params, widths, nlayers = host
        R = len(idxs)
        return _lib.load().sv_pointnet_sa_msg(ptr(x), ptr(p), ptr(q), B, N, D, S, R, nsamples,
                                              (c_void_p * R)(*[t.data_ptr() for t in idxs]), params, widths, nlayers,
                                              ptr(out), stream_ptr())

    def forward(self, xyz, points, fps_start=None):
        D = 0 if points is None else points.shape[1]
        want = self.conv_blocks[0][0].in_channels - 3
        if xyz.dim() != 3 or xyz.shape[1] != 3 or D != want:
            raise ValueError(f"multi-scale set abstraction expects xyz [B, 3, N] and {want} point features, got "
                             f"xyz {tuple(xyz.shape)} and {D} features")
        return super().forward(xyz, points, fps_start)


def three_nn_interpolate(xyz1, xyz2, points2):
    """[B,N,3], [B,S,3], [B,S,C] -> [B,N,C]: 3-NN inverse-distance interpolation on libsvhip (sv_three_nn_interpolate),
    replacing the reference's full [B,N,S] distance matrix + sort (model/pointnet2_utils.py:298-305)."""
    B, N, _ = xyz1.shape
    S, C = points2.shape[1], points2.shape[2]
    x1, x2, p2 = (t.to(torch.float32).contiguous() for t in (xyz1, xyz2, points2))
    out = torch.empty((B, N, C), dtype=torch.float32, device=x1.device)
    call("sv_three_nn_interpolate", ptr(x1), ptr(x2), ptr(p2), c_int(B), c_int(N), c_int(S), c_int(C), ptr(out),
         stream_ptr())
    return out


class PointNetFeaturePropagation(FoldCache):
    _hip_trainable = True  # set_training_path

    def __init__(self, in_channel, mlp):
        super().__init__()
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last = in_channel
        for out in mlp:
            self.mlp_convs.append(nn.Conv1d(last, out, 1))
            self.mlp_bns.append(nn.BatchNorm1d(out))
            last = out

    def forward(self, xyz1, xyz2, points1, points2):
        """3-NN inverse-distance interpolation of points2 (at xyz2) onto xyz1, concat points1, shared MLP."""
        hip = _hip_train(self, xyz1, xyz2)
        xyz1 = xyz1.permute(0, 2, 1)
        xyz2 = xyz2.permute(0, 2, 1)
        points2 = points2.permute(0, 2, 1)
        B, N, _ = xyz1.shape
        S = xyz2.shape[1]
        if S == 1:  # one source point: the torch broadcast
            interpolated = points2.repeat(1, N, 1)
        elif hip:  # the fused kernel in two launches: the neighbours and weights are kept for the backward
            idx, w = three_nn(xyz1, xyz2, self)
            interpolated = three_nn_gather(points2, idx, w, self)
        elif not self.training and xyz1.is_cuda and S >= 3:
            interpolated = three_nn_interpolate(xyz1, xyz2, points2)
        else:
            dists, idx = square_distance(xyz1, xyz2).topk(3, dim=-1, largest=False, sorted=True)
            recip = 1.0 / (dists + 1e-8)
            weight = recip / recip.sum(dim=2, keepdim=True)
            interpolated = torch.sum(index_points(points2, idx) * weight.view(B, N, 3, 1), dim=2)
        new_points = interpolated if points1 is None else torch.cat([points1.permute(0, 2, 1), interpolated], dim=-1)
        if self.training and not hip:
            t = new_points.permute(0, 2, 1)
            for conv, bn in zip(self.mlp_convs, self.mlp_bns):
                t = F.relu(bn(conv(t)))
            return t
        rows = new_points.reshape(B * N, -1)
        if hip:
            rows = _mlp_rows_train(rows, self.mlp_convs, self.mlp_bns)
        else:
            folds = self._fold_get(lambda: _fold_mlp(self.mlp_convs, self.mlp_bns))
            rows = _mlp_rows(rows.contiguous(), self.mlp_convs, self.mlp_bns, folds)
        return rows.view(B, N, -1).permute(0, 2, 1)
