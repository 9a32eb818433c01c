"""sv_stride_map_general past one launch of the single-workgroup radix sort (RS_SMALL_MAX = 8192 keys) and a few blocks of the
unique scan, at its extreme outcomes and strides, and CoordinateManager's derived maps independent of which maps existed.
Integer data, np.array_equal against the restatements of tests/strided_helpers.py (the whole-array ones for tens of
thousands of voxels; tests/test_resnet_ops_edges_cpu.py holds them to the dict ones)."""
import numpy as np
import pytest

import strided_helpers as H
from coords_helpers import unsort

pytestmark = pytest.mark.gpu


def _check(keys, coords, s_in, s_out, gpu):
    want_c, want_k, want_p, bad = H.stride_map_ref_np(coords, s_out)
    assert bad == 0
    ko, vo, parent, cnt = H.gpu_stride_map_general(keys, s_in, s_out, gpu)
    assert cnt.tolist() == [len(want_c), 0, 0, 0]
    assert np.array_equal(ko, want_k) and np.array_equal(vo, want_c) and np.array_equal(parent, want_p)
    return vo, parent


@pytest.mark.parametrize("V_in", [8191, 8192, 8193, 40000])
@pytest.mark.parametrize("s_in,s_out", [(1, 3), (2, 6)])
def test_sizes_around_the_sort_threshold(gpu, s_in, s_out, V_in):
    """two frames drawn without replacement from the cells of a 40^3 box around the origin (both signs), at tensor stride s_in"""
    rng = np.random.default_rng(V_in + s_out)
    n0 = V_in // 2
    rows = []
    for b, n in ((0, n0), (1, V_in - n0)):
        cells = rng.choice(40 ** 3, size=n, replace=False)
        xyz = (np.stack([cells % 40, cells // 40 % 40, cells // 1600], 1) - 20) * s_in
        rows.append(np.concatenate([np.full((n, 1), b), xyz], 1))
    coords, keys = H.canonical_np(np.concatenate(rows))
    assert len(coords) == V_in and (coords[:, 1:] < 0).any() and (coords[:, 1:] > 0).any()
    vo, parent = _check(keys, coords, s_in, s_out, gpu)
    assert len(vo) > 8 * 256  # many blocks of the unique scan
    assert np.array_equal(vo[parent][:, 1:], coords[:, 1:] // s_out * s_out)


@pytest.mark.parametrize("batch", [0, 1023])
def test_everything_collapses_or_nothing_does(gpu, batch):
    coords, keys = H.canonical_np(H.collapse_voxels(batch))
    vo, parent = _check(keys, coords, 1, 192, gpu)
    assert len(vo) == 1 and (parent == 0).all() and vo.tolist() == [[batch, -192, -192, -192]]
    coords, keys = H.canonical_np(H.spread_voxels(batch))
    vo, parent = _check(keys, coords, 1, 3, gpu)
    assert len(vo) == len(coords) == 9000 and np.array_equal(np.sort(parent), np.arange(9000))


def test_strides_at_the_top_and_off_the_powers_of_two(gpu):
    s_in, s_out = 1 << 15, 3 << 15  # the coarsest lattice whose floor of a negative coordinate, -98304, stays in the key range
    g = np.arange(-3, 4) * s_in
    rows = np.array([(b, x, y, z) for b in (0, 5, 1023) for x in g for y in g for z in g])
    coords, keys = H.canonical_np(rows)
    vo, _ = _check(keys, coords, s_in, s_out, gpu)
    assert sorted(set(vo[:, 1].tolist())) == [-s_out, 0, s_out] and len(vo) == 3 * 27
    rng = np.random.default_rng(5)
    rows = np.concatenate([rng.integers(0, 2, size=(3000, 1)), rng.integers(-60, 60, size=(3000, 3))], 1)
    coords, keys = H.canonical_np(rows)
    vo, _ = _check(keys, coords, 1, 5, gpu)
    assert (vo[:, 1:] % 5 == 0).all() and vo[:, 1:].min() == -60


def test_stride_that_is_no_multiple_is_refused(gpu):
    import mrcc_amd

    coords, keys = H.canonical([(0, 0, 0, 0), (0, 4, -8, 12)])
    with pytest.raises(mrcc_amd._lib.SvHipError, match="s_out must be a multiple of s_in"):
        H.gpu_stride_map_general(keys, 4, 6, gpu)


def _manager(pts, gpu):
    import torch

    from mrcc_amd import MinkowskiEngine as ME

    x = ME.SparseTensor(torch.ones(len(pts), 1), coordinates=torch.from_numpy(pts.astype(np.int32)), device=gpu)
    return x.coordinate_manager


def test_stride_map_does_not_depend_on_the_maps_that_existed(gpu):
    """stride_map(12) from the stride-1 map alone, and after the maps at 2, 4 and 6 exist (then derived from 6, itself derived
    from 2): the same keys and coordinates, and the same parent of every stride-1 voxel when the chain's parents are composed"""
    pts = H.two_frame_cloud(31, 900, [(-16, 9, 0), (21, -18, 11)], 7.0, -60, 60)
    a, b = _manager(pts, gpu), _manager(pts, gpu)
    c1 = a.stride_map(1).coords.cpu().numpy()
    ma = a.stride_map(12)
    assert set(a.maps) == {1, 12} and set(a.general_parents) == {(1, 12)}
    for s in (2, 4, 6):
        b.stride_map(s)
    mb = b.stride_map(12)
    assert set(b.general_parents) == {(2, 6), (6, 12)}
    want_c, want_k, want_p, bad = H.stride_map_ref(c1, 12)
    assert bad == 0 and len(want_c) > 20
    for m in (ma, mb):
        assert m.V == len(want_c) and np.array_equal(m.coords.cpu().numpy(), want_c) and np.array_equal(m.keys.cpu().numpy(), want_k)
    pa = a.general_parents[(1, 12)].cpu().numpy()
    to2 = b.parents[1][0].cpu().numpy()
    to6, to12 = b.general_parents[(2, 6)].cpu().numpy(), b.general_parents[(6, 12)].cpu().numpy()
    assert np.array_equal(pa, want_p) and np.array_equal(to12[to6[to2]], want_p)
    for s in (2, 4, 6):
        assert np.array_equal(b.stride_map(s).coords.cpu().numpy(), H.stride_map_ref(c1, s)[0])


@pytest.mark.parametrize("ts,ks,st", [(1, 3, 4), (1, 1, 3), (2, 3, 3)])
def test_more_strided_plans(gpu, ts, ks, st):
    """plan_strided / plan_strided_t from tensor stride ts: raw tables and mask-sorted plans are the restatement's, and the _t
    table is the transpose"""
    pts = H.two_frame_cloud(37, 700, [(-6, 3, 0), (9, -8, 5)], 4.0, -40, 40)
    cm = _manager(pts, gpu)
    fwd, tr = cm.plan_strided(ts, ks, st), cm.plan_strided_t(ts, ks, st)
    c1 = cm.stride_map(1).coords.cpu().numpy()
    c_in = c1 if ts == 1 else H.stride_map_ref(c1, ts)[0]
    c_out = H.stride_map_ref(c_in, ts * st)[0]
    assert np.array_equal(cm.stride_map(ts).coords.cpu().numpy(), c_in)
    assert np.array_equal(cm.stride_map(ts * st).coords.cpu().numpy(), c_out)
    want, want_t = H.probe_ref(c_out, c_in, ks, ts), H.probe_ref(c_in, c_out, ks, -ts)
    got, got_t = fwd.raw[0].cpu().numpy()[:, :len(c_out)], tr.raw[0].cpu().numpy()[:, :len(c_in)]
    assert np.array_equal(got, want) and np.array_equal(unsort(fwd), want)
    assert np.array_equal(got_t, want_t) and np.array_equal(unsort(tr), want_t)
    assert (fwd.in_stride, fwd.out_stride, tr.in_stride, tr.out_stride) == (ts, ts * st, ts * st, ts)
    pairs = {(k, int(o), int(i)) for k in range(got.shape[0]) for o, i in enumerate(got[k]) if i >= 0}
    pairs_t = {(k, int(o), int(i)) for k in range(got_t.shape[0]) for i, o in enumerate(got_t[k]) if o >= 0}
    assert pairs == pairs_t and pairs
