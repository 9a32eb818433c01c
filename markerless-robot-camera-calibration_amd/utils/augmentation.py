"""Training-time point augmentation of the reference (utils/augmentation.py:14-138) on the device, and the batch
builder that replaces augment_segmentation + centring + ME.utils.sparse_quantize + collate (data/alivev2.py:273-296,
358-365) with one call.

The reference's names are kept: distort_elastic, add_noise, transform_random, flip_random, rotate_along_gravity, augment,
augment_segmentation.  change_background is left out: it reads an image file through Open3D and recolours background
points; it is not on the point path.

Per-frame functions take a numpy array (float64 numpy comes back, as in the reference) or a CUDA tensor (a float64 CUDA
tensor comes back).  Without explicit draws they draw from the global np.random state with the reference's calls in the
reference's order (scipy.stats.special_ortho_group.rvs(3) included), so a run seeded like the reference applies the
same augmentation; the arithmetic is sv_elastic_field / sv_augment_points (include/sv_hip.h N5): float64, the
reference's operation order.  distort_elastic reads |x|.max(0) back to size its grid, as the reference does.  Every draw
can also be passed in (noise=, normals=, tr=, rot=, sign=, angle=).

The batch path (draw_augmentations + augment_quantize_batch) makes every random choice of a batch on the host before
anything is launched, so nothing is read back between the stages.  The second elastic stage's grid, which the reference
sizes from the cloud the first stage produced, is sized from the bound abs_max + mag1 * max|raw noise 1| instead (a blur
whose weights sum to at most 1 cannot exceed the raw maximum), and the draws come from a numpy Generator and, for the
per-point normals, from torch.randn on the device.  The batch path is therefore the same in distribution as the
reference, not stream-identical to it: a second-stage grid may be larger than the reference's (the field's interior
statistics do not depend on the grid's size; the zero-padded border cells lie further out), and the generators differ.
"""
from ctypes import c_double, c_int, c_int64, c_size_t, c_void_p
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np
import torch

from .. import _lib
from .._lib import SvHipError, call, ptr, stream_ptr

NOISE_SIGMA, NOISE_CLIP = 0.0016, 0.005  # add_noise's defaults (:49)


@dataclass
class ElasticStage:
    raw: np.ndarray  # float32 [3, bx, by, bz]: the unblurred normal draws of the three displacement components
    gran: float
    mag: float


@dataclass
class AugmentationDraws:
    """The random choices of one frame.  A stage that does not fire is None / empty / False."""
    elastic: List[ElasticStage] = field(default_factory=list)  # at most two stages, applied in order
    noise: bool = False
    normals: Optional[np.ndarray] = None  # float64 [n, 3] standard normal draws; None: drawn on the device
    sigma: float = NOISE_SIGMA
    clip: float = NOISE_CLIP
    transform: Optional[Tuple[float, np.ndarray]] = None  # (tr, rot [3, 3])
    flip: Optional[int] = None  # +1 / -1
    gravity: Optional[float] = None  # angle

    def fired(self):
        return {"elastic": bool(self.elastic), "noise": self.noise, "transform": self.transform is not None,
                "flip": self.flip is not None, "gravity": self.gravity is not None}


def elastic_grid_shape(abs_max, gran):
    """bb of distort_elastic:19 from the per-axis max |x|"""
    return tuple(int(v) for v in np.asarray(abs_max).astype(np.int32) // gran + 3)


def segmentation_stages(scale):
    """(gran, mag) of augment_segmentation's two distort_elastic calls (:122-123)"""
    return (6 * scale // 50, 40 * scale / 50), (20 * scale // 50, 160 * scale / 50)


def draw_augmentations(abs_max, *, scale=200, probability=0.2, elastic=False, noise=False, transform=False, flip=False,
                       gravity=False, rng=None):
    """The random choices of augment_segmentation for a batch, on the host: abs_max [B, 3] is the per-axis max |x| of
    every frame.  Returns one AugmentationDraws per frame.  Choices are made in the reference's order per frame; the
    second elastic stage's grid is sized from abs_max + mag1 * max|raw noise 1| (module docstring).  Needs no GPU."""
    from scipy.stats import special_ortho_group

    rng = np.random.default_rng() if rng is None else rng
    abs_max = np.asarray(abs_max, dtype=np.float64).reshape(-1, 3)
    out = []
    for am in abs_max:
        d = AugmentationDraws()
        if elastic and rng.random() < probability:
            bound = am
            for gran, mag in segmentation_stages(scale):
                raw = rng.standard_normal((3,) + elastic_grid_shape(bound, gran)).astype(np.float32)
                d.elastic.append(ElasticStage(raw, gran, mag))
                bound = bound + mag * float(np.abs(raw).max())
        if noise and rng.random() < probability:
            d.noise = True
        if transform and rng.random() < probability:
            tr = rng.random() * 0.04
            d.transform = (tr, special_ortho_group.rvs(3, random_state=rng))
        if flip and rng.random() < probability:
            d.flip = int(rng.integers(0, 2)) * 2 - 1
        if gravity and rng.random() < probability:
            d.gravity = rng.random() * 2 * np.pi
        out.append(d)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# device plumbing
# ---------------------------------------------------------------------------------------------------------------------
def _table_and_fields(draws):
    """([B, SV_AUG_STRIDE] float64 table, raw noise of every stage as one float32 array, int32 [F, 3] grid shapes)"""
    L = _lib
    table = np.zeros((len(draws), L.SV_AUG_STRIDE), dtype=np.float64)
    raws, dims, first = [], [], 0
    for row, d in zip(table, draws):
        if len(d.elastic) > 2:
            raise ValueError("at most two elastic stages per frame")
        for base, st in zip((L.SV_AUG_ELASTIC0, L.SV_AUG_ELASTIC1), d.elastic):
            raw = np.ascontiguousarray(st.raw, dtype=np.float32)
            if raw.ndim != 4 or raw.shape[0] != 3 or min(raw.shape[1:]) < 3:
                raise ValueError(f"elastic noise must be [3, bx, by, bz] with every b >= 3, got {raw.shape}")
            row[base + L.SV_AUG_E_ON] = 1
            row[base + L.SV_AUG_E_OFFSET] = first
            row[base + L.SV_AUG_E_BX: base + L.SV_AUG_E_BZ + 1] = raw.shape[1:]
            row[base + L.SV_AUG_E_GRAN], row[base + L.SV_AUG_E_MAG] = st.gran, st.mag
            raws.append(raw.reshape(-1))
            dims.append(raw.shape[1:])
            first += raw.size
        if d.noise:
            row[L.SV_AUG_NOISE_ON], row[L.SV_AUG_NOISE_SIGMA], row[L.SV_AUG_NOISE_CLIP] = 1, d.sigma, d.clip
        if d.transform is not None:
            tr, rot = d.transform
            row[L.SV_AUG_TRANSFORM_ON] = 1
            row[L.SV_AUG_ROT: L.SV_AUG_ROT + 9] = np.asarray(rot, dtype=np.float64).reshape(9)
            row[L.SV_AUG_TRANSLATION] = tr
        if d.flip is not None:
            if d.flip not in (1, -1):
                raise ValueError("flip sign must be +1 or -1")
            row[L.SV_AUG_FLIP_SIGN] = d.flip
        if d.gravity is not None:
            row[L.SV_AUG_GRAVITY_ON], row[L.SV_AUG_GRAVITY_ANGLE] = 1, d.gravity
            row[L.SV_AUG_GRAVITY_COS], row[L.SV_AUG_GRAVITY_SIN] = np.cos(d.gravity), np.sin(d.gravity)
    raw = np.concatenate(raws) if raws else np.zeros(0, dtype=np.float32)
    return table, raw, np.asarray(dims, dtype=np.int32).reshape(-1, 3)


def elastic_fields(raw, dims, device):
    """sv_elastic_field: raw (flat float32, the fields one after the other) and dims int32 [F, 3] on the host ->
    the blurred fields as one flat float32 device tensor"""
    lib = _lib.load()
    dims = np.ascontiguousarray(dims, dtype=np.int32).reshape(-1, 3)
    F = dims.shape[0]
    raw_d = torch.from_numpy(np.ascontiguousarray(raw, dtype=np.float32).reshape(-1)).to(device)
    if raw_d.numel() != int((3 * dims.astype(np.int64).prod(axis=1)).sum()):
        raise ValueError("raw does not hold 3 * bx * by * bz floats per field")
    out = torch.empty_like(raw_d)
    dims_p = dims.ctypes.data_as(c_void_p)
    ws_bytes = lib.sv_elastic_field_workspace_bytes(dims_p, c_int(F))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=device)
    call("sv_elastic_field", ptr(raw_d), dims_p, c_int(F), ptr(ws), c_size_t(ws_bytes), ptr(out), stream_ptr())
    return out


def augment_points(points, offsets, table, fields=None, normals=None):
    """sv_augment_points on device tensors: points float32 / float64 [N, 3], offsets int32 [B + 1], table float64
    [B, SV_AUG_STRIDE], fields flat float32 or None, normals float64 [N, 3] or None -> (float64 [N, 3], stats [B, 6])"""
    lib = _lib.load()
    dev = _lib.require_cuda(points, "points").device
    N, B = points.shape[0], table.shape[0]
    out = torch.empty((N, 3), dtype=torch.float64, device=dev)
    stats = torch.empty((B, 6), dtype=torch.float64, device=dev)
    ws_bytes = lib.sv_augment_points_workspace_bytes(c_int64(N), c_int(B))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    call("sv_augment_points", ptr(points), c_int(1 if points.dtype == torch.float64 else 0), ptr(offsets), c_int64(N),
         c_int(B), ptr(table), ptr(fields), c_int64(0 if fields is None else fields.numel()), ptr(normals), ptr(ws),
         c_size_t(ws_bytes), ptr(out), ptr(stats), stream_ptr())
    return out, stats


def quantise_points(points, offsets, stats, origin, quantization_size):
    """sv_quantise_points -> (coords int32 [N, 4], shifted float32 [N, 3], shift float64 [B, 3])"""
    dev = points.device
    N, B = points.shape[0], offsets.numel() - 1
    coords = torch.empty((N, 4), dtype=torch.int32, device=dev)
    shifted = torch.empty((N, 3), dtype=torch.float32, device=dev)
    shift = torch.empty((B, 3), dtype=torch.float64, device=dev)
    call("sv_quantise_points", ptr(points), ptr(offsets), c_int64(N), c_int(B), ptr(stats), c_int(origin),
         c_double(quantization_size), ptr(coords), ptr(shifted), ptr(shift), stream_ptr())
    return coords, shifted, shift


def _to_device_points(x, device):
    """(device tensor float32 / float64 [N, 3], is_numpy)"""
    if isinstance(x, torch.Tensor):
        if not x.is_cuda:
            raise SvHipError(f"points must be a numpy array or a CUDA tensor (got a {x.device} tensor); "
                             "the HIP path has no CPU fallback")
        t, is_np = x, False
    else:
        a = np.asarray(x)
        if a.dtype != np.float32:
            a = a.astype(np.float64)
        t, is_np = torch.from_numpy(np.ascontiguousarray(a)).to(device or "cuda"), True
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"points must be [N, 3], got {tuple(t.shape)}")
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    return t.contiguous(), is_np


def _apply(x, draws, device=None, return_abs_max=False):
    """One frame through sv_augment_points with the given draws; numpy in -> float64 numpy out."""
    t, is_np = _to_device_points(x, device)
    dev = t.device
    n = t.shape[0]
    table, raw, dims = _table_and_fields([draws])
    fields = elastic_fields(raw, dims, dev) if len(dims) else None
    normals = None
    if draws.noise:
        nd = draws.normals if draws.normals is not None else torch.randn((n, 3), dtype=torch.float64, device=dev)
        normals = (nd if isinstance(nd, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(nd, dtype=np.float64)))
        normals = normals.to(device=dev, dtype=torch.float64).contiguous()
        if tuple(normals.shape) != (n, 3):
            raise ValueError(f"normals must be [{n}, 3], got {tuple(normals.shape)}")
    offsets = torch.tensor([0, n], dtype=torch.int32, device=dev)
    out, stats = augment_points(t, offsets, torch.from_numpy(table).to(dev), fields, normals)
    res = out.cpu().numpy() if is_np else out
    if return_abs_max:
        s = stats.cpu().numpy()[0]
        return res, np.maximum(np.abs(s[:3]), np.abs(s[3:]))
    return res


def _abs_max(x):
    if isinstance(x, torch.Tensor):
        return x.detach().abs().amax(dim=0).cpu().numpy().astype(np.float64)
    return np.abs(np.asarray(x)).max(0)


# ---------------------------------------------------------------------------------------------------------------------
# the reference's per-frame functions
# ---------------------------------------------------------------------------------------------------------------------
def distort_elastic(x, gran, mag, *, noise=None, device=None):
    """x + mag * g(x), g the trilinear interpolant of three box-blurred normal noise grids (:14-33).  noise: the raw
    float32 grids [3, bx, by, bz]; drawn with np.random.randn like the reference when None."""
    if noise is None:
        bb = elastic_grid_shape(_abs_max(x), gran)
        noise = np.stack([np.random.randn(*bb).astype("float32") for _ in range(3)])
    return _apply(x, AugmentationDraws(elastic=[ElasticStage(np.asarray(noise), gran, mag)]), device)


def add_noise(x, sigma=NOISE_SIGMA, clip=NOISE_CLIP, *, normals=None, device=None):
    """x + clip(sigma * n, -clip, clip) (:49-51); normals [N, 3] are np.random.randn(*x.shape) when None"""
    if normals is None:
        normals = np.random.randn(*x.shape)
    return _apply(x, AugmentationDraws(noise=True, normals=normals, sigma=sigma, clip=clip), device)


def transform_random(pc, *, tr=None, rot=None, device=None):
    """(pc @ rot + [tr, 0, 0]) @ rot.T (:54-61)"""
    from scipy.stats import special_ortho_group

    if tr is None:
        tr = np.random.rand() * 0.04
    if rot is None:
        rot = special_ortho_group.rvs(3)
    return _apply(pc, AugmentationDraws(transform=(tr, rot)), device)


def flip_random(pc, *, sign=None, device=None):
    """pc @ diag(sign, 1, 1) (:64-67)"""
    if sign is None:
        sign = np.random.randint(0, 2) * 2 - 1
    return _apply(pc, AugmentationDraws(flip=int(sign)), device)


def rotate_along_gravity(pc, *, angle=None, device=None):
    """(rot_y(angle) @ pc.T).T (:70-75)"""
    if angle is None:
        angle = np.random.rand() * 2 * np.pi
    return _apply(pc, AugmentationDraws(gravity=float(angle)), device)


def _augment(points, stages, probability, elastic, noise, transform, flip, gravity, draws, device):
    """The shared body of augment / augment_segmentation.  With draws the frame goes through one launch sequence;
    without, the choices are made in the reference's order from np.random, which needs the cloud's extent after every
    elastic stage (a read-back per stage, as the reference's own |x|.max(0))."""
    from scipy.stats import special_ortho_group

    if draws is not None:
        return _apply(points, draws, device)
    t, is_np = _to_device_points(points, device)
    n = t.shape[0]
    if elastic and np.random.rand() < probability:
        am = _abs_max(t)
        for gran, mag in stages:
            bb = elastic_grid_shape(am, gran)
            raw = np.stack([np.random.randn(*bb).astype("float32") for _ in range(3)])
            t, am = _apply(t, AugmentationDraws(elastic=[ElasticStage(raw, gran, mag)]), return_abs_max=True)
    d = AugmentationDraws()
    if noise and np.random.rand() < probability:
        d.noise, d.normals = True, np.random.randn(n, 3)
    if transform and np.random.rand() < probability:
        tr = np.random.rand() * 0.04
        d.transform = (tr, special_ortho_group.rvs(3))
    if flip and np.random.rand() < probability:
        d.flip = int(np.random.randint(0, 2)) * 2 - 1
    if gravity and np.random.rand() < probability:
        d.gravity = np.random.rand() * 2 * np.pi
    out = _apply(t, d)
    return out.cpu().numpy() if is_np else out


def augment(points, probability=0.2, copy=False, elastic=False, noise=False, transform=False, flip=False, gravity=False,
            *, draws=None, device=None):
    """:78-105.  `copy` is accepted for the reference's signature: the input is never modified."""
    return _augment(points, ((1, 4),), probability, elastic, noise, transform, flip, gravity, draws, device)


def augment_segmentation(points, scale=200, probability=0.2, copy=False, elastic=False, noise=False, transform=False,
                         flip=False, gravity=False, *, draws=None, device=None):
    """:108-138: two elastic stages sized by `scale`, then noise, transform, flip, gravity."""
    return _augment(points, segmentation_stages(scale), probability, elastic, noise, transform, flip, gravity, draws,
                    device)


# ---------------------------------------------------------------------------------------------------------------------
# the batch builder
# ---------------------------------------------------------------------------------------------------------------------
def augment_quantize_batch(points, feats, labels, *, draws=None, scale=200, quantization_size, probability=0.2,
                           elastic=False, noise=False, transform=False, flip=False, gravity=False,
                           center_at_origin=False, base_at_origin=False, ignore_label=-100, rng=None, generator=None,
                           device="cuda", return_extras=False, point_offsets=None):
    """A training batch from the frames a dataset yields: augment_segmentation, centring (center_at_origin, else
    base_at_origin: data/alivev2.py:199-208), ME.utils.sparse_quantize and the collate of data/alivev2.py:358-365, on
    the device, for all frames at once.

    points / feats / labels: lists of host arrays [n_b, 3] / [n_b, C] / [n_b] (or [n_b, 1]).  draws: one
    AugmentationDraws per frame (draw_augmentations(...) with `rng` when None).  Per-point normals a frame's draws do not
    carry come from torch.randn(..., dtype=float64, generator=generator) on the device.

    With point_offsets ([B + 1], host or device) points / feats / labels may each instead be ONE CUDA tensor of the
    frames' concatenated rows ([N, 3] float32 or float64, [N, C], [N] or [N, 1]), e.g. what utils.data.ee_crop_batch and
    key_point_labels_batch return: nothing visits the host.  Device offsets are only read back when the host needs the
    frames' lengths: to draw augmentations (draws None with a stage enabled) or to place normals a draws object carries.

    Returns device tensors (coords_batch int32 [V, 4], feats_batch float32 [V, C], labels_batch int64 [V],
    voxel_offsets int32 [B + 1]), ready for ME.SparseTensor(feats_batch, coordinates=coords_batch).  Voxels are in
    canonical order, frame after frame, each frame's as ME.utils.sparse_quantize orders them; the lowest point index
    represents a voxel, conflicting labels give ignore_label.  With return_extras a dict follows: "origin_offset"
    float64 [B, 3] (what centring subtracted), "points" float32 [N, 3] (augmented, centred), "point_offsets" and
    "inverse" (voxel row of every point).

    Launches: sv_elastic_field (if any frame has an elastic stage), sv_augment_points, sv_quantise_points, sv_voxelize.
    The only host wait is sv_voxelize's voxel-count read-back."""
    dev = torch.device(device)
    if point_offsets is not None:
        if dev.type != "cuda":
            raise SvHipError(f"augment_quantize_batch runs on the GPU (got device {dev}); there is no CPU fallback")
        return _augment_quantize_device(points, feats, labels, point_offsets, dev, draws=draws, scale=scale,
                                        quantization_size=quantization_size, probability=probability,
                                        flags=dict(elastic=elastic, noise=noise, transform=transform, flip=flip,
                                                   gravity=gravity),
                                        center_at_origin=center_at_origin, base_at_origin=base_at_origin,
                                        ignore_label=ignore_label, rng=rng, generator=generator,
                                        return_extras=return_extras)
    B = len(points)
    if not (B == len(feats) == len(labels)) or not 1 <= B <= _lib.SV_MAX_BATCH:
        raise ValueError(f"need the same number (1 to {_lib.SV_MAX_BATCH}) of point, feature and label arrays")
    if dev.type != "cuda":
        raise SvHipError(f"augment_quantize_batch runs on the GPU (got device {dev}); there is no CPU fallback")
    pts = [np.asarray(p) for p in points]
    for p, f, l in zip(pts, feats, labels):
        if p.ndim != 2 or p.shape[1] != 3 or len(f) != len(p) or len(l) != len(p):
            raise ValueError("every frame needs points [n, 3] and one feature row and one label per point")
    if draws is None:
        abs_max = np.stack([np.abs(p).max(0) if len(p) else np.zeros(3) for p in pts])
        draws = draw_augmentations(abs_max, scale=scale, probability=probability, elastic=elastic, noise=noise,
                                   transform=transform, flip=flip, gravity=gravity, rng=rng)
    if len(draws) != B:
        raise ValueError("one draws object per frame")
    lens = np.array([len(p) for p in pts], dtype=np.int64)
    N = int(lens.sum())
    if N < 1:
        raise ValueError("the batch has no points")
    off_np = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    p_dtype = np.float32 if all(p.dtype == np.float32 for p in pts) else np.float64
    table, raw, dims = _table_and_fields(draws)
    cat = np.concatenate([p.astype(p_dtype, copy=False) for p in pts])
    f_cat = np.concatenate(_frame_rows(feats, np.float32))
    l_cat = np.concatenate([np.asarray(l).reshape(-1) for l in labels]).astype(np.int64)
    pts_d = torch.from_numpy(cat).to(dev, non_blocking=True)
    off_d = torch.from_numpy(off_np).to(dev, non_blocking=True)
    table_d = torch.from_numpy(table).to(dev, non_blocking=True)
    feats_d = torch.from_numpy(f_cat).to(dev, non_blocking=True)
    labels_d = torch.from_numpy(l_cat).to(dev, non_blocking=True)
    normals = None
    if any(d.noise for d in draws):
        if all(d.normals is not None or not d.noise for d in draws):
            nh = np.zeros((N, 3), dtype=np.float64)
            for b, d in enumerate(draws):
                if d.noise:
                    nh[off_np[b]: off_np[b + 1]] = np.asarray(d.normals, dtype=np.float64).reshape(int(lens[b]), 3)
            normals = torch.from_numpy(nh).to(dev, non_blocking=True)
        else:
            normals = torch.randn((N, 3), dtype=torch.float64, device=dev, generator=generator)
            for b, d in enumerate(draws):
                if d.noise and d.normals is not None:
                    normals[off_np[b]: off_np[b + 1]] = torch.from_numpy(
                        np.asarray(d.normals, dtype=np.float64).reshape(int(lens[b]), 3)).to(dev)
    return _augment_quantize_launch(pts_d, off_d, table_d, feats_d, labels_d, normals, raw, dims, B, dev,
                                    center_at_origin, base_at_origin, quantization_size, ignore_label, return_extras)


def _augment_quantize_launch(pts_d, off_d, table_d, feats_d, labels_d, normals, raw, dims, B, dev, center_at_origin,
                             base_at_origin, quantization_size, ignore_label, return_extras):
    """the launches of augment_quantize_batch on device tensors"""
    from ..MinkowskiEngine.utils import resolve_voxel_labels
    from ..sparse import _voxelize

    with torch.cuda.device(dev):
        fields = elastic_fields(raw, dims, dev) if len(dims) else None
        aug, stats = augment_points(pts_d, off_d, table_d, fields, normals)
        origin = _lib.SV_ORIGIN_CENTER if center_at_origin else (_lib.SV_ORIGIN_BASE if base_at_origin else _lib.SV_ORIGIN_NONE)
        coords, shifted, shift = quantise_points(aug, off_d, stats, origin, float(quantization_size))
        cmap, inverse, order, seg_start = _voxelize(coords, dev, coords_are_int=True)
        first = order[seg_start[:-1].long()].long()  # representative point of each voxel: its lowest index
        labels_batch = resolve_voxel_labels(labels_d, first, inverse, cmap.V, ignore_label)
        voxel_offsets = torch.empty(B + 1, dtype=torch.int32, device=dev)
        call("sv_batch_offsets", ptr(cmap.keys), c_int64(cmap.V), c_int(B), ptr(voxel_offsets), stream_ptr())
    res = (cmap.coords, feats_d[first], labels_batch, voxel_offsets)
    if return_extras:
        return res + ({"origin_offset": shift, "points": shifted, "point_offsets": off_d, "inverse": inverse},)
    return res


def _frame_rows(xs, dtype=None):
    """per-frame host arrays [n_b, ...] -> [n_b, C] each; a frame without rows has no width of its own (reshape(0, -1)
    is an error) and takes C from the frames that have rows"""
    arrs = [np.asarray(x, dtype=dtype) for x in xs]
    C = next((a.size // len(a) for a in arrs if len(a)), 1)
    return [a.reshape(len(a), C) for a in arrs]


def _rows_on_device(x, what, dev, dtype, N=None):
    """one CUDA tensor of concatenated rows, or a list of per-frame host arrays (concatenated and uploaded)"""
    if isinstance(x, torch.Tensor):
        if not x.is_cuda:
            raise SvHipError(f"{what} must be a CUDA tensor or a list of host arrays (got a {x.device} tensor)")
        t = x if dtype is None else x.to(dtype)
    else:
        a = np.concatenate(_frame_rows(x))
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        t = t if dtype is None else t.to(dtype)
    if N is not None and t.shape[0] != N:
        raise ValueError(f"{what} need one row per point ({N}), got {t.shape[0]}")
    return t


def _augment_quantize_device(points, feats, labels, point_offsets, dev, *, draws, scale, quantization_size, probability,
                             flags, center_at_origin, base_at_origin, ignore_label, rng, generator, return_extras):
    """augment_quantize_batch on concatenated device tensors with point_offsets"""
    pts_d = _rows_on_device(points, "points", dev, None)
    if pts_d.dim() != 2 or pts_d.shape[1] != 3:
        raise ValueError(f"points must be [N, 3], got {tuple(pts_d.shape)}")
    if pts_d.dtype not in (torch.float32, torch.float64):
        pts_d = pts_d.to(torch.float64)
    pts_d = pts_d.contiguous()
    N = pts_d.shape[0]
    if N < 1:
        raise ValueError("the batch has no points")
    feats_d = _rows_on_device(feats, "feats", dev, torch.float32, N).reshape(N, -1).contiguous()
    labels_d = _rows_on_device(labels, "labels", dev, torch.int64, N).reshape(-1).contiguous()
    if labels_d.numel() != N:
        raise ValueError("labels need one value per point")
    host_off = None
    if isinstance(point_offsets, torch.Tensor) and point_offsets.is_cuda:
        off_d = point_offsets.to(torch.int32).contiguous().reshape(-1)
    else:
        host_off = np.asarray(point_offsets, dtype=np.int64).reshape(-1)
        if len(host_off) < 2 or host_off[0] != 0 or host_off[-1] != N or (np.diff(host_off) < 0).any():
            raise ValueError(f"point_offsets must rise from 0 to the number of points ({N})")
        off_d = torch.from_numpy(host_off.astype(np.int32)).to(dev)
    B = off_d.numel() - 1
    if not 1 <= B <= _lib.SV_MAX_BATCH:
        raise ValueError(f"need 1 to {_lib.SV_MAX_BATCH} frames, got {B}")

    def offsets_on_host():
        nonlocal host_off
        if host_off is None:
            host_off = off_d.cpu().numpy().astype(np.int64)
        return host_off

    if draws is None:
        if any(flags.values()):
            o = offsets_on_host()
            abs_max = torch.stack([pts_d[o[b]: o[b + 1]].abs().amax(0) if o[b + 1] > o[b] else pts_d.new_zeros(3)
                                   for b in range(B)]).cpu().numpy()
            draws = draw_augmentations(abs_max, scale=scale, probability=probability, rng=rng, **flags)
        else:
            draws = [AugmentationDraws() for _ in range(B)]
    if len(draws) != B:
        raise ValueError("one draws object per frame")
    table, raw, dims = _table_and_fields(draws)
    normals = None
    if any(d.noise for d in draws):
        normals = torch.randn((N, 3), dtype=torch.float64, device=dev, generator=generator)
        for b, d in enumerate(draws):
            if d.noise and d.normals is not None:
                o = offsets_on_host()
                normals[o[b]: o[b + 1]] = torch.from_numpy(
                    np.asarray(d.normals, dtype=np.float64).reshape(int(o[b + 1] - o[b]), 3)).to(dev)
    table_d = torch.from_numpy(table).to(dev, non_blocking=True)
    return _augment_quantize_launch(pts_d, off_d, table_d, feats_d, labels_d, normals, raw, dims, B, dev,
                                    center_at_origin, base_at_origin, quantization_size, ignore_label, return_extras)
