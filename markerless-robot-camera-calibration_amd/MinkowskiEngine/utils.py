"""ME.utils: batched_coordinates, sparse_quantize, sparse_collate, kaiming_normal_ (data/alivev2.py:290-296,363,391;
resnet.py:89)."""
from ctypes import c_int, c_int64, c_size_t

import numpy as np
import torch

from .. import _lib
from ..nn import kaiming_normal_  # noqa: F401


def batched_coordinates(coords, dtype=torch.int32, device=None):
    """Prepend the batch index column: list of [N_i, 3] -> [sum N_i, 4] (batch, x, y, z).
    float dtypes keep the continuous coordinates (TensorField input, app/inference_engine.py:407-410)."""
    out = []
    for b, c in enumerate(coords):
        c = torch.as_tensor(c)
        if not dtype.is_floating_point:
            c = torch.floor(c) if c.dtype.is_floating_point else c
        bc = torch.full((c.shape[0], 1), b, dtype=dtype, device=c.device)
        out.append(torch.cat([bc, c.to(dtype)], dim=1))
    res = torch.cat(out, dim=0) if out else torch.zeros((0, 4), dtype=dtype)
    return res.to(device) if device is not None else res


def resolve_voxel_labels(lab, first, inverse, V, ignore_label):
    """Label of every voxel: its representative point's (lab[first]), or ignore_label where the voxel's points disagree.
    lab int64 [N], first int64 [V], inverse int64 [N], all on one device."""
    rep = lab[first]
    differs = torch.zeros(V, dtype=torch.bool, device=lab.device)
    differs.index_put_((inverse,), lab != rep[inverse], accumulate=True)
    return torch.where(differs, torch.full_like(rep, ignore_label), rep)


def sparse_collate(coords, feats, labels=None, dtype=torch.int32, device=None):
    """Lists of per-frame coordinates [N_i, 3], features [N_i, C] and (optionally) labels -> (batched coordinates
    [sum N_i, 4], concatenated features, concatenated labels), as data/alivev2.py:391 collate_sparse expects; without
    labels the pair (coordinates, features)."""
    if len(coords) != len(feats) or (labels is not None and len(labels) != len(coords)):
        raise ValueError("coords, feats and labels must list the same frames")
    for i, (c, f) in enumerate(zip(coords, feats)):
        if len(c) != len(f) or (labels is not None and len(labels[i]) != len(c)):
            raise ValueError(f"frame {i}: one feature row (and one label) per coordinate row")
    coords_batch = batched_coordinates(coords, dtype=dtype, device=device)

    def cat(xs):
        t = torch.cat([torch.as_tensor(x) for x in xs], dim=0)
        return t.to(device) if device is not None else t

    if labels is None:
        return coords_batch, cat(feats)
    return coords_batch, cat(feats), cat(labels)


def sparse_quantize(coordinates, features=None, labels=None, ignore_label=-100, return_index=False,
                    return_inverse=False, return_maps_only=False, quantization_size=None, device="cuda"):
    """floor(coordinates / quantization_size) -> unique voxels in canonical order; the lowest original point index
    represents a voxel; a voxel whose points carry different labels gets ignore_label (data/alivev2.py:290-296)."""
    from ..sparse import _voxelize

    is_np = isinstance(coordinates, np.ndarray)
    c = torch.as_tensor(coordinates)
    if quantization_size is not None:
        c = torch.floor(c.to(torch.float64) / quantization_size)
    elif c.dtype.is_floating_point:
        c = torch.floor(c)
    c = c.to(torch.int32)
    if c.shape[1] == 3:
        c = torch.cat([torch.zeros((c.shape[0], 1), dtype=torch.int32), c], dim=1)
    dev = torch.device(device)
    cd = c.to(dev).contiguous()
    cmap, inverse, order, seg_start = _voxelize(cd, dev, coords_are_int=True)
    first = order[seg_start[:-1].long()].long()  # representative point of each voxel
    discrete = cmap.coords[:, 1:] if coordinates.shape[1] == 3 else cmap.coords

    def back(t):
        t = t.cpu()
        return t.numpy() if is_np else t

    if return_maps_only:
        return (back(first), back(inverse)) if return_inverse else back(first)
    res = [back(discrete)]
    if features is not None:
        f = torch.as_tensor(features)
        res.append(back(f.to(dev)[first]) if not isinstance(features, np.ndarray) else features[first.cpu().numpy()])
    if labels is not None:
        out_lab = resolve_voxel_labels(torch.as_tensor(labels).to(dev).long(), first, inverse, cmap.V, ignore_label)
        res.append(back(out_lab.to(torch.as_tensor(labels).dtype)))
    if return_index:
        res.append(back(first))
    if return_inverse:
        res.append(back(inverse))
    return res[0] if len(res) == 1 else tuple(res)
