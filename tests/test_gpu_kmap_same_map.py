"""sv_kernel_map_k3 is the same-map case of sv_kernel_map_probe: on one map, queried and probed, the two entries give the
same table and mask, equal to the CPU reference - at sizes either side of one 256-thread block, with a tensor stride and a
dilation, on maps that hold the voxel whose key marks an empty hash slot and voxels on both faces of the key range next to
the voxels a wrapped neighbour key would find.  Integer data, every comparison exact."""
from ctypes import c_int, c_int64

import numpy as np
import pytest
import strided_helpers as H

pytestmark = pytest.mark.gpu

LO, HI = H.LO, H.HI
MARKER = (1023, HI, HI, HI)
UP, DOWN = 14, 12  # offsets (+1, 0, 0) and (-1, 0, 0)


def wrap(x):
    """where a coordinate outside [LO, HI] lands when only the 18 key bits of x + 2^17 are kept"""
    return (x + H.BIAS) % (1 << H.BITS) - H.BIAS


def edge_map(V, step):
    """canonical map of V voxels: the marker voxel and two of its neighbours at `step`; a voxel on the upper face, one on the
    lower face, and the voxels their out-of-range +-step neighbours wrap onto; a compact block on a `step` grid for the rest"""
    special = [MARKER, (1023, HI - step, HI, HI), (1023, HI, HI - step, HI - step),
               (3, HI, 5, 5), (3, wrap(HI + step), 5, 5), (3, LO, 9, 9), (3, wrap(LO - step), 9, 9)]
    block = H.compact_blob(V - len(special), batch=1)
    block[:, 1:] *= step
    coords, keys = H.canonical(np.concatenate([np.array(special, np.int64), block]))
    assert len(coords) == V
    return coords, keys


def gpu_k3(coords, keys, tensor_stride, dilation, dev, pad=3):
    """sv_hash_build + sv_kernel_map_k3 -> (nbr int32[27][V], mask int32[V]); ld = V + pad, the padding stays untouched"""
    import torch
    from mrcc_amd import _lib as L

    V, ld = len(coords), len(coords) + pad
    cap = 2
    while cap < 2 * V:
        cap *= 2
    k = torch.from_numpy(np.ascontiguousarray(keys)).to(dev)
    tk = torch.empty(cap, dtype=torch.int64, device=dev)
    tv = torch.empty(cap, dtype=torch.int32, device=dev)
    L.call("sv_hash_build", L.ptr(k), c_int64(V), L.ptr(tk), L.ptr(tv), c_int64(cap), L.stream_ptr())
    c = torch.from_numpy(np.ascontiguousarray(coords, np.int32)).to(dev)
    nbr = torch.full((27, ld), -9, dtype=torch.int32, device=dev)
    mask = torch.full((ld,), -9, dtype=torch.int32, device=dev)
    L.call("sv_kernel_map_k3", L.ptr(c), c_int64(V), c_int(tensor_stride), c_int(dilation), L.ptr(tk), L.ptr(tv), c_int64(cap),
           L.ptr(nbr), c_int64(ld), L.ptr(mask), L.stream_ptr())
    nbr, mask = nbr.cpu().numpy(), mask.cpu().numpy()
    assert (nbr[:, V:] == -9).all() and (mask[V:] == -9).all(), "sv_kernel_map_k3 wrote past V"
    return nbr[:, :V], mask[:V]


@pytest.mark.parametrize("ks", [1, 3])
def test_probe_of_an_empty_table_map(gpu, ks):
    """no voxel in the table's map: every neighbour is -1, also for a query whose neighbour has the marker key (the map has
    no last row to compare it with), and the padding columns stay as they were (H.gpu_probe asserts it)"""
    coords_q = H.canonical([MARKER, (1023, HI - 1, HI, HI), (0, 0, 0, 0), (0, LO, LO, LO), (5, 1, 2, 3)])[0]
    nbr, mask = H.gpu_probe(coords_q, np.zeros((0, 4), np.int32), np.zeros(0, np.int64), ks, 1, gpu)
    assert nbr.shape == (ks ** 3, 5) and (nbr == -1).all() and (mask == 0).all()


@pytest.mark.parametrize("tensor_stride,dilation", [(1, 1), (2, 1), (1, 2)])
@pytest.mark.parametrize("V", [255, 256, 257])
def test_k3_is_the_probe_of_a_map_with_itself(gpu, oracle, V, tensor_stride, dilation):
    step = tensor_stride * dilation
    coords, keys = edge_map(V, step)
    rows = {tuple(r): i for i, r in enumerate(coords.tolist())}
    want = oracle.kernel_map_k3(coords, tensor_stride) if dilation == 1 else H.probe_ref(coords, coords, 3, step)
    # the inputs hold what they are built for: the marker voxel as the last row, found by its neighbours ...
    assert tuple(coords[-1]) == MARKER and int(keys[-1]) == -1 and H.make_keys(coords[-1:])[0] == H.EMPTY_KEY
    assert want[13, V - 1] == V - 1 and want[UP, rows[(1023, HI - step, HI, HI)]] == V - 1 and (want == V - 1).sum() == 3
    # ... a voxel on the upper face whose +step neighbour leaves the key range, the voxel it would wrap onto in the map ...
    up, up_image = rows[(3, HI, 5, 5)], rows[(3, wrap(HI + step), 5, 5)]
    assert coords[up_image, 1] == LO + step - 1 and want[UP, up] == -1
    # ... and the same on the lower face
    down, down_image = rows[(3, LO, 9, 9)], rows[(3, wrap(LO - step), 9, 9)]
    assert coords[down_image, 1] == HI - step + 1 and want[DOWN, down] == -1
    # the keys an unguarded probe would look up are in the table
    assert H.make_keys([(3, HI + step, 5, 5), (3, LO - step, 9, 9)]) == H.make_keys(coords[[up_image, down_image]])

    nbr_k3, mask_k3 = gpu_k3(coords, keys, tensor_stride, dilation, gpu)
    nbr_probe, mask_probe = H.gpu_probe(coords, coords, keys, 3, step, gpu)
    assert np.array_equal(nbr_k3, nbr_probe) and np.array_equal(mask_k3, mask_probe)
    assert np.array_equal(nbr_k3, want) and np.array_equal(mask_k3, H.mask_of(want))
    if dilation == 1:  # the two references agree as well
        assert np.array_equal(want, H.probe_ref(coords, coords, 3, step))
