"""sv_stride_map_general and sv_kernel_map_probe against numpy dict-lookup restatements (tests/strided_helpers.py): integer
data, compared with np.array_equal."""
import numpy as np
import pytest

import strided_helpers as H
from coords_helpers import unsort

pytestmark = pytest.mark.gpu


def _map_at(rng, s_in, s_out, n, batches, extra=()):
    """canonical map at tensor stride s_in: random voxels (negatives included) around the origin in `batches`, exact
    multiples of s_out, and the `extra` rows"""
    rows = [(int(b), *(int(v) * s_in for v in rng.integers(-40, 40, size=3))) for b in rng.choice(batches, size=n)]
    m = s_out // s_in
    rows += [(int(batches[0]), i * s_out, -j * s_out, 0) for i in range(-2, 3) for j in range(3)]
    rows += [(int(batches[-1]), s_out * 3 - s_in, -s_out * 3 + s_in * (m - 1), -s_in)]  # last / first voxel of a coarse cell
    rows += list(extra)
    return H.canonical(rows)


def _lowest_valid(s_out):
    return -((1 << 17) // s_out) * s_out  # the smallest output coordinate inside the key range


@pytest.mark.parametrize("s_in,s_out", [(2, 6), (1, 3), (64, 192)])
def test_stride_map_general_matches_restatement(gpu, s_in, s_out):
    rng = np.random.default_rng(s_out)
    hi = H.HI // s_in * s_in  # the upper key-range corner on this map's lattice (2^17 - 1 itself at tensor stride 1)
    low = _lowest_valid(s_out)
    extra = [(0, hi, hi, hi), (2, hi, 0, -s_in), (2, low, low + s_in, low), (0, low + s_out - s_in, 0, low)]
    coords, keys = _map_at(rng, s_in, s_out, 700, [0, 2], extra)  # frames 0 and 2: frame 1 is empty
    assert set(coords[:, 0].tolist()) == {0, 2} and coords[:, 1:].min() < 0 and (coords[:, 1:] % s_out == 0).all(1).any()
    want_c, want_k, want_p, bad = H.stride_map_ref(coords, s_out)
    assert bad == 0 and len(want_c) > 256  # more than one block of the unique / scatter kernels
    ko, vo, parent, cnt = H.gpu_stride_map_general(keys, s_in, s_out, gpu)
    assert cnt.tolist() == [len(want_c), 0, 0, 0]
    assert np.array_equal(ko, want_k) and np.array_equal(vo, want_c) and np.array_equal(parent, want_p)
    # parent is consistent with the keys: every input voxel floors onto the voxel its parent row names
    assert np.array_equal(vo[parent][:, 1:], coords[:, 1:] // s_out * s_out) and np.array_equal(vo[parent][:, 0], coords[:, 0])
    assert np.array_equal(np.unique(parent), np.arange(len(vo)))


@pytest.mark.parametrize("s_in,s_out", [(2, 6), (1, 3), (64, 192)])
def test_stride_map_general_lower_range_corner(gpu, s_in, s_out):
    """-2^17 is no multiple of 3: flooring it to a stride that is leaves the key range.  Such voxels are counted in
    counters[1] and get parent -1 (the caller must treat the count as an error, as sv_voxelize's); the others still find
    their voxels."""
    rng = np.random.default_rng(7)
    lo = H.LO
    extra = [(0, lo, 0, 0), (0, 0, lo, s_in), (2, s_in, 0, lo), (2, lo, lo, lo), (0, lo + s_in * 0, 5 * s_in, 0)]
    coords, keys = _map_at(rng, s_in, s_out, 300, [0, 2], extra)
    want_c, want_k, want_p, bad = H.stride_map_ref(coords, s_out)
    assert bad == int((coords[:, 1:] == lo).any(1).sum()) >= 4
    ko, vo, parent, cnt = H.gpu_stride_map_general(keys, s_in, s_out, gpu)
    assert cnt.tolist() == [len(want_c), bad, 0, 0]
    assert np.array_equal(ko, want_k) and np.array_equal(vo, want_c) and np.array_equal(parent, want_p)
    assert np.array_equal(parent == -1, (coords[:, 1:] == lo).any(1))


@pytest.mark.parametrize("s_in,s_out", [(2, 6), (1, 3), (64, 192)])
def test_stride_map_general_single_voxel_and_empty(gpu, s_in, s_out):
    for row in ((3, -s_in, 5 * s_in, 0), (0, 0, 0, 0), (1023, H.HI // s_in * s_in, -s_in, s_in)):
        coords, keys = H.canonical([row])
        ko, vo, parent, cnt = H.gpu_stride_map_general(keys, s_in, s_out, gpu)
        want_c, want_k, want_p, _ = H.stride_map_ref(coords, s_out)
        assert cnt.tolist() == [1, 0, 0, 0] and np.array_equal(vo, want_c) and np.array_equal(ko, want_k)
        assert parent.tolist() == [0]
    ko, vo, parent, cnt = H.gpu_stride_map_general(np.zeros(0, np.int64), s_in, s_out, gpu)
    assert cnt.tolist() == [0, 0, 0, 0] and len(ko) == 0


def _probe_sets(rng, ks, s_in, st, V_q):
    """V_q query rows, most of them on the s_in * st lattice, and a table map of voxels one step around them, with the range
    cases (the entry takes any coordinate rows, so these sit on the faces themselves): a query on the upper face whose +step
    neighbour would wrap onto a table voxel on the lower face, the same on the lower face, and the voxel whose key is the
    empty-slot marker (found as the table's last row)"""
    s_out, step = s_in * st, s_in
    q = {(0, H.HI, 0, 0), (1, H.LO, s_out, 0), (1023, H.HI - step, H.HI, H.HI), (1023, H.HI, H.HI, H.HI)}
    t = {(1023, H.HI, H.HI, H.HI), (1023, H.HI - step, H.HI, H.HI), (0, H.HI, 0, 0), (1, H.LO, s_out, 0),
         # where HI + step and LO - step land after wrapping by 2^18: a probe without the range guard finds these
         (0, H.HI + step - (1 << 18), 0, 0), (1, H.LO - step + (1 << 18), s_out, 0)}
    assert all(H.in_range(*r) for r in t)
    while len(q) < V_q:
        q.add((int(rng.integers(0, 2)), *(int(v) * s_out for v in rng.integers(-4, 4, size=3))))
    t |= set(sorted(q)[::3])
    for r in sorted(q)[::2]:
        for d in rng.integers(-1, 2, size=(6, 3)):
            c = (r[0], r[1] + int(d[0]) * step, r[2] + int(d[1]) * step, r[3] + int(d[2]) * step)
            if H.in_range(*c):
                t.add(c)
    cq, kq = H.canonical(sorted(q))
    ct, kt = H.canonical(sorted(t))
    assert len(cq) == V_q
    return cq, kq, ct, kt, step


@pytest.mark.parametrize("V_q", [255, 256, 257])
@pytest.mark.parametrize("ks,s_in,st", [(3, 1, 2), (3, 2, 3), (1, 1, 2), (3, 64, 3)])
def test_kernel_map_probe_forward_and_transposed(gpu, ks, s_in, st, V_q):
    rng = np.random.default_rng(1000 * ks + 10 * st + V_q)
    cq, kq, ct, kt, step = _probe_sets(rng, ks, s_in, st, V_q)
    nbr, mask = H.gpu_probe(cq, ct, kt, ks, step, gpu)
    want = H.probe_ref(cq, ct, ks, step)
    assert np.array_equal(nbr, want) and np.array_equal(mask, H.mask_of(want))
    assert (want >= 0).sum() >= V_q // 4
    nbr_t, mask_t = H.gpu_probe(ct, cq, kq, ks, -step, gpu)
    want_t = H.probe_ref(ct, cq, ks, -step)
    assert np.array_equal(nbr_t, want_t) and np.array_equal(mask_t, H.mask_of(want_t))
    # the transposed table is the transpose of the forward one: nbr[k][o] = i exactly when nbr_t[k][i] = o
    fwd = {(k, int(o), int(i)) for k in range(nbr.shape[0]) for o, i in enumerate(nbr[k]) if i >= 0}
    bwd = {(k, int(o), int(i)) for k in range(nbr_t.shape[0]) for i, o in enumerate(nbr_t[k]) if o >= 0}
    assert fwd == bwd
    if ks == 3:
        # range guard: the +x neighbour of the query on the upper face is absent although its wrapped key is in the table
        top = np.flatnonzero((cq == (0, H.HI, 0, 0)).all(1))[0]
        assert nbr[14, top] == -1 and nbr[13, top] >= 0
        bot = np.flatnonzero((cq == (1, H.LO, s_in * st, 0)).all(1))[0]
        assert nbr[12, bot] == -1  # -x of the query on the lower face
        # the empty-marker voxel is found (as the table's last row) from its -x neighbour, and finds itself at the centre
        last = len(ct) - 1
        assert tuple(ct[last]) == (1023, H.HI, H.HI, H.HI)
        src = np.flatnonzero((cq == (1023, H.HI - step, H.HI, H.HI)).all(1))[0]
        assert nbr[14, src] == last
        me = np.flatnonzero((cq == (1023, H.HI, H.HI, H.HI)).all(1))[0]
        assert nbr[13, me] == last


@pytest.mark.parametrize("ks,st", [(3, 2), (3, 3), (1, 2)])
def test_coordinate_manager_strided_plans(gpu, ks, st):
    """CoordinateManager.plan_strided / plan_strided_t on a two-frame tensor: the raw tables are the restatement's, the
    mask-sorted plans hold the same tables, batch_bounds works at the new stride"""
    import torch

    from mrcc_amd import MinkowskiEngine as ME

    rng = np.random.default_rng(ks * 10 + st)
    pts = np.concatenate([np.concatenate([np.full((900, 1), b), H.blob_cloud(rng, 900, [(-6, 3, 0), (9, -8, 5)], 4.0, (-40,) * 3,
                                                                              (40,) * 3)], 1) for b in (0, 1)])
    x = ME.SparseTensor(torch.ones(len(pts), 1), coordinates=torch.from_numpy(pts.astype(np.int32)), device=gpu)
    cm = x.coordinate_manager
    fwd, tr = cm.plan_strided(1, ks, st), cm.plan_strided_t(1, ks, st)
    c_in, c_out = cm.stride_map(1).coords.cpu().numpy(), cm.stride_map(st).coords.cpu().numpy()
    want_c, _, _, bad = H.stride_map_ref(c_in, st)
    assert bad == 0 and np.array_equal(c_out, want_c)
    want, want_t = H.probe_ref(c_out, c_in, ks, 1), H.probe_ref(c_in, c_out, ks, -1)
    assert np.array_equal(fwd.raw[0].cpu().numpy()[:, :len(c_out)], want) and np.array_equal(unsort(fwd), want)
    assert np.array_equal(tr.raw[0].cpu().numpy()[:, :len(c_in)], want_t) and np.array_equal(unsort(tr), want_t)
    assert (fwd.in_stride, fwd.out_stride, tr.in_stride, tr.out_stride) == (1, st, st, 1)
    assert cm.plan_strided(1, ks, st) is fwd and cm.plan_strided_t(1, ks, st) is tr  # cached in cm.plans
    bounds = cm.batch_bounds(st)
    assert bounds == [0, int((c_out[:, 0] == 0).sum()), len(c_out)]
    if (ks, st) == (3, 2):  # offsets 0 and +1 cover a stride-2 cell: every output voxel sees the voxel it is the floor of.  A
        assert (want >= 0).any(0).all()  # stride-3 cell's third voxel and a k1 kernel's off-lattice voxels are not seen
