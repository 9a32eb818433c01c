"""PointNet++ sampling / grouping with the reference's names (model/pointnet2_utils.py) on libsvhip.

farthest_point_sample(xyz [B,N,3], npoint) -> int64 [B,npoint]     reference :65-86 (python loop of npoint launches)
query_ball_point(radius, nsample, xyz, new_xyz) -> int64 [B,S,nsample]   reference :89-109 ([B,S,N] matrix + sort)
query_ball_point_multi(radii, nsamples, xyz, new_xyz) -> R of those      one scan for a multi-scale layer's radii
index_points, square_distance: thin torch helpers with the reference's semantics (:21-62).
"""
from ctypes import c_double, c_int

import torch

from .._lib import call, ptr, require_cuda, stream_ptr


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
    from ctypes import c_void_p

    from .._lib import SV_BQ_MAX_RADII

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


def _group(xyz, points, new_xyz, idx):
    """[xyz[idx] - new_xyz, points[idx]] -> [B, S, nsample, 3 + D] (reference :131-137)."""
    B, S, C = new_xyz.shape
    grouped_xyz = index_points(xyz, idx)
    grouped_xyz_norm = grouped_xyz - new_xyz.view(B, S, 1, C)
    new_points = grouped_xyz_norm if points is None else torch.cat([grouped_xyz_norm, index_points(points, idx)], -1)
    return grouped_xyz, new_points


def sample_and_group(npoint, radius, nsample, xyz, points, returnfps=False, fps_start=None):
    """reference :112-140.  fps_start int64 [B] pins the first centroids (None: drawn as the reference draws them)."""
    fps_idx = farthest_point_sample(xyz, npoint, start=fps_start)
    new_xyz = index_points(xyz, fps_idx)
    idx = query_ball_point(radius, nsample, xyz, new_xyz)
    grouped_xyz, new_points = _group(xyz, points, new_xyz, idx)
    if returnfps:
        return new_xyz, new_points, grouped_xyz, fps_idx
    return new_xyz, new_points


# ----------------------------------------------------------------------------------------------------------------------
# set abstraction / feature propagation modules (reference :163-317).  Parameter names are the reference's
# (mlp_convs.i = nn.Conv2d / nn.Conv1d 1x1, mlp_bns.i = BatchNorm) so its checkpoints load by key; in eval mode the
# shared MLPs run as dense rows through the fp32-MFMA kernel with the BatchNorm folded into the epilogue.
# ----------------------------------------------------------------------------------------------------------------------
import numpy as np  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from .. import nn as svnn  # noqa: E402
from .._lib import SV_ACT_RELU  # noqa: E402


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


def _mlp_rows(rows, convs, bns, folds=None):
    """rows [R, Cin] -> relu(bn(conv(.))) stack, one fused launch per layer (folds: the layers' _fold_conv_bn results)."""
    if folds is None:
        folds = [_fold_conv_bn(conv, bn) for conv, bn in zip(convs, bns)]
    for w, scale, shift in folds:
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


def sample_and_group_all(xyz, points):
    B, N, C = xyz.shape
    new_xyz = torch.zeros(B, 1, C, device=xyz.device)
    grouped = xyz.view(B, 1, N, C)
    new_points = grouped if points is None else torch.cat([grouped, points.view(B, 1, N, -1)], dim=-1)
    return new_xyz, new_points


class PointNetSetAbstraction(FoldCache):
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

    def _folded(self):
        """(per-layer folds, packed sv_pointnet_sa parameters, host widths) - built once per weights / device"""
        def build():
            folds = [_fold_conv_bn(conv, bn) for conv, bn in zip(self.mlp_convs, self.mlp_bns)]
            packed = torch.cat([t.reshape(-1).to(torch.float32) for f in folds for t in f]).contiguous()
            widths = [self.mlp_convs[0].in_channels] + [conv.out_channels for conv in self.mlp_convs]
            return folds, packed, (c_int * len(widths))(*widths)

        return self._fold_get(build)

    def _fused(self, xyz, points, new_xyz, idx, folds):
        """sv_pointnet_sa: gather + shared MLP + max in one launch -> [B, S, C_last], or None where the kernel does not
        cover the shape (SV_ERR_UNSUPPORTED: nothing was launched, the caller runs the layers one by one)."""
        from .. import _lib

        _, packed, widths = folds
        B, N, _ = xyz.shape
        S = new_xyz.shape[1]
        x = xyz.to(torch.float32).contiguous()
        p = points.to(torch.float32).contiguous() if points is not None else None
        D = p.shape[2] if p is not None else 0
        if widths[0] != 3 + D:
            raise ValueError(f"set abstraction expects {widths[0] - 3} point features, got {D}")
        q = new_xyz.to(torch.float32).contiguous()
        out = torch.empty((B, S, widths[len(widths) - 1]), dtype=torch.float32, device=xyz.device)
        lib = _lib.load()
        rc = lib.sv_pointnet_sa(ptr(x), ptr(p), ptr(q), ptr(idx), B, N, D, S, self.nsample, ptr(packed), widths,
                                len(widths) - 1, ptr(out), stream_ptr())
        if rc == _lib.SV_ERR_UNSUPPORTED:
            return None
        _lib._check(rc, "sv_pointnet_sa")
        return out

    def forward(self, xyz, points, fps_start=None):
        """xyz [B,3,N], points [B,D,N] -> new_xyz [B,3,S], new_points [B,D',S].  fps_start int64 [B] pins the first
        farthest-point centroids (None: drawn as the reference draws them, torch.randint on the device)."""
        xyz = xyz.permute(0, 2, 1)
        if points is not None:
            points = points.permute(0, 2, 1)
        if self.training or self.group_all:
            if self.group_all:
                new_xyz, new_points = sample_and_group_all(xyz, points)
            else:
                new_xyz, new_points = sample_and_group(self.npoint, self.radius, self.nsample, xyz, points,
                                                       fps_start=fps_start)
            if self.training:
                t = new_points.permute(0, 3, 2, 1)
                for conv, bn in zip(self.mlp_convs, self.mlp_bns):
                    t = F.relu(bn(conv(t)))
                return new_xyz.permute(0, 2, 1), torch.max(t, 2)[0]
            B, S, Kn, C = new_points.shape
            rows = _mlp_rows(new_points.reshape(B * S * Kn, C).contiguous(), self.mlp_convs, self.mlp_bns,
                             self._folded()[0])
            return new_xyz.permute(0, 2, 1), rows.view(B, S, Kn, -1).max(dim=2)[0].permute(0, 2, 1)
        # eval: sampling and ball query on libsvhip, then the fused set abstraction (sv_pointnet_sa)
        fps_idx = farthest_point_sample(xyz, self.npoint, start=fps_start)
        new_xyz = index_points(xyz, fps_idx)
        idx = query_ball_point(self.radius, self.nsample, xyz, new_xyz)
        folds = self._folded()
        pooled = self._fused(xyz, points, new_xyz, idx, folds) if xyz.is_cuda else None
        if pooled is None:  # shapes outside the fused kernel: the layers one launch each, then torch.max
            _, new_points = _group(xyz, points, new_xyz, idx)
            B, S, Kn, C = new_points.shape
            rows = _mlp_rows(new_points.reshape(B * S * Kn, C).contiguous(), self.mlp_convs, self.mlp_bns, folds[0])
            pooled = rows.view(B, S, Kn, -1).max(dim=2)[0]
        return new_xyz.permute(0, 2, 1), pooled.permute(0, 2, 1)  # [B, D', S]


def _group_msg(xyz, points, new_xyz, idx):
    """[points[idx], xyz[idx] - new_xyz] -> [B, S, nsample, D + 3]: the multi-scale grouping's order, features first
    (reference :245-250)."""
    B, S, C = new_xyz.shape
    grouped_xyz = index_points(xyz, idx) - new_xyz.view(B, S, 1, C)
    return grouped_xyz if points is None else torch.cat([index_points(points, idx), grouped_xyz], dim=-1)


class PointNetSetAbstractionMsg(FoldCache):
    """Multi-scale grouping (reference :207-264): R radii around the same farthest-point centroids, one shared MLP per
    radius, the pooled features concatenated.  Parameter names conv_blocks.i.j / bn_blocks.i.j as in the reference.  Eval
    on the GPU: sv_fps, sv_ball_query_multi, then sv_pointnet_sa_msg (all scales in one launch); shapes the fused kernel
    declines, or `fused = False`, run every scale's layers one launch each (sv_conv_fwd dense rows), torch.max and
    torch.cat - the same bits."""

    def __init__(self, npoint, radius_list, nsample_list, in_channel, mlp_list):
        super().__init__()
        self.npoint = npoint
        self.radius_list = list(radius_list)
        self.nsample_list = list(nsample_list)
        self.fused = True  # False: the unfused eval path (tests, timing)
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

    def _folded(self):
        """(per-scale layer folds, per-scale packed parameters, host arrays of sv_pointnet_sa_msg) - built once per
        weights / device"""
        from ctypes import c_void_p

        def build():
            folds = [[_fold_conv_bn(c, b) for c, b in zip(convs, bns)]
                     for convs, bns in zip(self.conv_blocks, self.bn_blocks)]
            packed = [torch.cat([t.reshape(-1).to(torch.float32) for f in fs for t in f]).contiguous() for fs in folds]
            widths = [w for convs in self.conv_blocks for w in [convs[0].in_channels] + [c.out_channels for c in convs]]
            R = len(folds)
            host = ((c_int * R)(*self.nsample_list), (c_void_p * R)(*[p.data_ptr() for p in packed]),
                    (c_int * len(widths))(*widths), (c_int * R)(*[len(convs) for convs in self.conv_blocks]))
            return folds, packed, host

        return self._fold_get(build)

    def _fused(self, xyz, points, new_xyz, idxs, folds):
        """sv_pointnet_sa_msg: every scale's gather + shared MLP + max in one launch -> [B, S, sum C_r], or None where the
        kernel does not cover the shapes (SV_ERR_UNSUPPORTED: nothing was launched)."""
        from ctypes import c_void_p

        from .. import _lib

        _, _, (nsamples, params, widths, nlayers) = folds
        B, N, _ = xyz.shape
        S = new_xyz.shape[1]
        x = xyz.to(torch.float32).contiguous()
        p = points.to(torch.float32).contiguous() if points is not None else None
        D = p.shape[2] if p is not None else 0
        q = new_xyz.to(torch.float32).contiguous()
        R = len(idxs)
        ctot = sum(convs[-1].out_channels for convs in self.conv_blocks)
        out = torch.empty((B, S, ctot), dtype=torch.float32, device=xyz.device)
        rc = _lib.load().sv_pointnet_sa_msg(ptr(x), ptr(p), ptr(q), B, N, D, S, R, nsamples,
                                            (c_void_p * R)(*[t.data_ptr() for t in idxs]), params, widths, nlayers,
                                            ptr(out), stream_ptr())
        if rc == _lib.SV_ERR_UNSUPPORTED:
            return None
        _lib._check(rc, "sv_pointnet_sa_msg")
        return out

    def _unfused(self, xyz, points, new_xyz, idxs, folds):
        """every scale: MSG-order gather, its layers one launch each (dense rows), torch.max; then torch.cat"""
        pooled = []
        for i, idx in enumerate(idxs):
            grouped = _group_msg(xyz, points, new_xyz, idx)
            B, S, Kn, C = grouped.shape
            rows = _mlp_rows(grouped.reshape(B * S * Kn, C).contiguous(), self.conv_blocks[i], self.bn_blocks[i],
                             folds[0][i])
            pooled.append(rows.view(B, S, Kn, -1).max(dim=2)[0])
        return torch.cat(pooled, dim=-1)

    def forward(self, xyz, points, fps_start=None):
        """xyz [B,3,N], points [B,D,N] or None -> new_xyz [B,3,S], new_points [B, sum C_r, S].  fps_start int64 [B] pins
        the first farthest-point centroids (None: drawn as the reference draws them)."""
        D = 0 if points is None else points.shape[1]
        want = self.conv_blocks[0][0].in_channels - 3
        if xyz.dim() != 3 or xyz.shape[1] != 3 or D != want:
            raise ValueError(f"multi-scale set abstraction expects xyz [B, 3, N] and {want} point features, got "
                             f"xyz {tuple(xyz.shape)} and {D} features")
        xyz = xyz.permute(0, 2, 1)
        if points is not None:
            points = points.permute(0, 2, 1)
        fps_idx = farthest_point_sample(xyz, self.npoint, start=fps_start)
        new_xyz = index_points(xyz, fps_idx)
        if self.training:  # the reference's torch path (:238-262)
            pooled = []
            for i, (radius, K) in enumerate(zip(self.radius_list, self.nsample_list)):
                idx = query_ball_point(radius, K, xyz, new_xyz)
                t = _group_msg(xyz, points, new_xyz, idx).permute(0, 3, 2, 1)
                for conv, bn in zip(self.conv_blocks[i], self.bn_blocks[i]):
                    t = F.relu(bn(conv(t)))
                pooled.append(torch.max(t, 2)[0])
            return new_xyz.permute(0, 2, 1), torch.cat(pooled, dim=1)
        idxs = query_ball_point_multi(self.radius_list, self.nsample_list, xyz, new_xyz)
        folds = self._folded()
        pooled = self._fused(xyz, points, new_xyz, idxs, folds) if self.fused and xyz.is_cuda else None
        if pooled is None:
            pooled = self._unfused(xyz, points, new_xyz, idxs, folds)
        return new_xyz.permute(0, 2, 1), pooled.permute(0, 2, 1)


def three_nn_interpolate(xyz1, xyz2, points2):
    """[B,N,3], [B,S,3], [B,S,C] -> [B,N,C]: 3-NN inverse-distance interpolation on libsvhip (sv_three_nn_interpolate),
    replacing the reference's full [B,N,S] distance matrix + sort (model/pointnet2_utils.py:298-305)."""
    from ctypes import c_int

    from .._lib import call, ptr, stream_ptr

    B, N, _ = xyz1.shape
    S, C = points2.shape[1], points2.shape[2]
    x1, x2, p2 = (t.to(torch.float32).contiguous() for t in (xyz1, xyz2, points2))
    out = torch.empty((B, N, C), dtype=torch.float32, device=x1.device)
    call("sv_three_nn_interpolate", ptr(x1), ptr(x2), ptr(p2), c_int(B), c_int(N), c_int(S), c_int(C), ptr(out),
         stream_ptr())
    return out


class PointNetFeaturePropagation(FoldCache):
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
        xyz1 = xyz1.permute(0, 2, 1)
        xyz2 = xyz2.permute(0, 2, 1)
        points2 = points2.permute(0, 2, 1)
        B, N, _ = xyz1.shape
        S = xyz2.shape[1]
        if S == 1:
            interpolated = points2.repeat(1, N, 1)
        elif not self.training and xyz1.is_cuda and S >= 3:
            interpolated = three_nn_interpolate(xyz1, xyz2, points2)
        else:
            dists, idx = square_distance(xyz1, xyz2).topk(3, dim=-1, largest=False, sorted=True)
            recip = 1.0 / (dists + 1e-8)
            weight = recip / recip.sum(dim=2, keepdim=True)
            interpolated = torch.sum(index_points(points2, idx) * weight.view(B, N, 3, 1), dim=2)
        new_points = interpolated if points1 is None else torch.cat([points1.permute(0, 2, 1), interpolated], dim=-1)
        if self.training:
            t = new_points.permute(0, 2, 1)
            for conv, bn in zip(self.mlp_convs, self.mlp_bns):
                t = F.relu(bn(conv(t)))
            return t
        folds = self._fold_get(lambda: [_fold_conv_bn(conv, bn) for conv, bn in zip(self.mlp_convs, self.mlp_bns)])
        rows = _mlp_rows(new_points.reshape(B * N, -1).contiguous(), self.mlp_convs, self.mlp_bns, folds)
        return rows.view(B, N, -1).permute(0, 2, 1)
