"""The coordinate pipeline at its key-range and size edges: sv_voxelize, the radix sort of csrc/sv_sort.hip, sv_hash_build,
sv_stride_map, sv_kernel_map_* and sv_plan_build against the CPU oracle or a numpy restatement - integer work, so every
comparison is exact.  Inputs are built here with numpy: keys that use all 64 bits, sizes on and next to every threshold of
the sort (2048-row tiles, the 8192-pair single-workgroup path, a second 256-tile chunk of the scan) and of the
order-preserving unique (256-row blocks, a second 256-block chunk of its scan), voxels on the faces of the key range
[-2^17, 2^17 - 1], batch indices up to 1023, dilated kernel maps, a hash table at exactly the allowed load."""
from ctypes import c_int, c_int64, c_size_t

import numpy as np
import pytest
import torch
from coords_helpers import COORD_HI as HI
from coords_helpers import COORD_LO as LO
from coords_helpers import edge_cloud, gray_key, unsort

pytestmark = pytest.mark.gpu

BATCHES = (0, 1, 511, 1022, 1023)
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
SV_ERR_INVALID = -1


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


# ----------------------------------------------------------------------------------------------------------------------
# voxelise, sort and unique at the size thresholds
# ----------------------------------------------------------------------------------------------------------------------
def _threshold_cloud(oracle, N, order):
    """N int32 rows drawn from about N / 3 distinct voxels over the whole key range and the batches 0 .. 1023: duplicates,
    keys whose 64 bits all vary, runs of equal keys across the 256-row blocks and the 2048-row tiles of the sorted array"""
    rng = np.random.default_rng(N)
    P = max(1, N // 3)
    pool = np.concatenate([rng.choice(BATCHES, size=(P, 1)), rng.integers(LO, HI + 1, size=(P, 3))], axis=1).astype(np.int32)
    pool[: min(P, 4)] = [(1023, HI, HI, HI), (0, LO, LO, LO), (1023, LO, HI, LO), (0, HI, LO, HI)][: min(P, 4)]
    c = pool[rng.integers(0, P, size=N)]
    if order == "identical":
        c[:] = pool[min(P, 5) - 1]
    elif order != "random":
        by_key = np.argsort(oracle.make_keys(c), kind="stable")
        c = c[by_key if order == "sorted" else by_key[::-1]]
    return np.ascontiguousarray(c)


def _check_voxelize(ref, cmap, inverse, order, seg_start):
    assert cmap.V == len(ref["keys"])
    assert np.array_equal(_u64(cmap.keys), ref["keys"])
    assert np.array_equal(cmap.coords.cpu().numpy(), ref["coords"])
    assert np.array_equal(inverse.cpu().numpy(), ref["inverse"])
    assert np.array_equal(order.cpu().numpy(), ref["order"])
    assert np.array_equal(seg_start.cpu().numpy(), ref["seg_start"])


SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 8191, 8192, 8193, 65_537, 526_337)
CASES = [(n, "random") for n in SIZES] + [(n, o) for n in (8193, 65_537) for o in ("sorted", "descending", "identical")]


@pytest.mark.parametrize("N,order", CASES)
def test_voxelize_sort_and_unique_at_the_size_thresholds(gpu, oracle, N, order):
    """keys, coords, inverse, order and seg_start of both input types equal the oracle's stable argsort.  526 337 rows =
    257 tiles of 2048 + 1: the only size here whose sort takes a second chunk in radix_scan_kernel (oracle.voxelize on it:
    0.3 s of CPU time); 65 537 rows = 257 blocks of 256: the second chunk of unique_scan_kernel."""
    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd import sparse

    c = _threshold_cloud(oracle, N, order)
    ref = oracle.voxelize(c, coords_are_int=True)
    assert order != "random" or N < 64 or len(ref["keys"]) < 0.4 * N  # the pool makes duplicates
    _check_voxelize(ref, *sparse._voxelize(_dev(c, gpu), gpu, coords_are_int=True))
    # the float path on the same voxels (every coordinate is exact in float32)
    field = ME.TensorField(torch.zeros((N, 1)), torch.from_numpy(c.astype(np.float32)), device=gpu)
    st = field.sparse()
    _check_voxelize(ref, st.coordinate_map, field.inverse_mapping, field._order, field._seg_start)


# ----------------------------------------------------------------------------------------------------------------------
# the key range: [-2^17, 2^17 - 1] per axis, batch in [0, 1023]
# ----------------------------------------------------------------------------------------------------------------------
def _sv_voxelize_counters(coords, gpu):
    """sv_voxelize through the C entry point (the Python wrapper raises on counters[1]); returns the counters"""
    from mrcc_amd._lib import call, load, ptr, stream_ptr

    c = _dev(coords, gpu)
    N = c.shape[0]
    ws_bytes = load().sv_voxelize_workspace_bytes(c_int64(N))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=gpu)
    keys = torch.empty(N, dtype=torch.int64, device=gpu)
    vcoords = torch.empty((N, 4), dtype=torch.int32, device=gpu)
    inverse = torch.empty(N, dtype=torch.int64, device=gpu)
    order = torch.empty(N, dtype=torch.int32, device=gpu)
    seg_start = torch.empty(N + 1, dtype=torch.int32, device=gpu)
    counters = torch.full((4,), -7, dtype=torch.int32, device=gpu)
    call("sv_voxelize", ptr(c), c_int(1 if c.dtype == torch.int32 else 0), c_int64(N), ptr(ws), c_size_t(ws_bytes), ptr(keys),
         ptr(vcoords), ptr(inverse), ptr(order), ptr(seg_start), ptr(counters), stream_ptr())
    return counters.tolist()


def _rows_with(value_rows, base):
    """one row per (value, column): `base` with that column replaced"""
    out = []
    for col, values in value_rows:
        for v in values:
            r = list(base)
            r[col] = v
            out.append(r)
    return out


NEXT_BELOW_2_17 = np.nextafter(np.float32(131072), np.float32(0))  # 131071.99: the largest float32 inside the range
GOOD_FLOAT = np.array([[0, -131072.0, 0.5, 0.5], [0, 0.5, -131072.0, 0.5], [0, 0.5, 0.5, -131072.0],
                       [0, -131071.5, -131071.5, -131071.5],                           # floors to -131072
                       [0, NEXT_BELOW_2_17, 0.5, 0.5], [0, 0.5, NEXT_BELOW_2_17, 0.5], [0, 0.5, 0.5, NEXT_BELOW_2_17],
                       [0, -0.0, -1e-7, 0.99999994],                                   # voxel (0, -1, 0)
                       [1023.0, 1.5, 2.5, 3.5], [-0.0, 1.5, 2.5, 3.5], [1023.9, -131072.0, -131072.0, -131072.0],
                       [1023.0, NEXT_BELOW_2_17, NEXT_BELOW_2_17, NEXT_BELOW_2_17]],   # the all-ones key
                      np.float32)
BAD_FLOAT = np.array(_rows_with([(col, (131072.0, -131072.5, np.nan, np.inf, -np.inf, 1e30, -1e30)) for col in (1, 2, 3)]
                                + [(0, (-0.5, -1.0, 1024.0, -1e-7, np.nan, np.inf, -np.inf))], (3, 1.5, 2.5, 3.5)), np.float32)
GOOD_INT = np.array([[0, HI, 0, 0], [0, LO, 0, 0], [1, 0, HI, 0], [1, 0, LO, 0], [1023, 0, 0, HI], [1023, 0, 0, LO],
                     [1023, HI, HI, HI], [0, LO, LO, LO]], np.int32)
BAD_INT = np.array(_rows_with([(col, (HI + 1, LO - 1, INT32_MAX, INT32_MIN, INT32_MAX - HI, INT32_MIN + HI)) for col in (1, 2, 3)]
                              + [(0, (-1, 1024, INT32_MAX, INT32_MIN))], (3, 1, 2, 3)), np.int32)


def test_float_rows_on_the_key_range_boundary_are_accepted(gpu, oracle):
    from mrcc_amd import MinkowskiEngine as ME

    ref = oracle.voxelize(GOOD_FLOAT)
    assert ref["coords"].min() == LO and ref["coords"].max() == HI and ref["keys"][-1] == EMPTY
    assert _sv_voxelize_counters(GOOD_FLOAT, gpu) == [len(ref["keys"]), 0, 0, 0]
    for levels in (None, 2):  # sv_voxelize / the frame composite
        field = ME.TensorField(torch.zeros((len(GOOD_FLOAT), 1)), torch.from_numpy(GOOD_FLOAT), device=gpu)
        st = field.sparse(pyramid_levels=levels)
        _check_voxelize(ref, st.coordinate_map, field.inverse_mapping, field._order, field._seg_start)


def test_float_rows_outside_the_key_range_are_counted(gpu):
    import mrcc_amd
    from mrcc_amd import MinkowskiEngine as ME

    rows = np.concatenate([GOOD_FLOAT, BAD_FLOAT, GOOD_FLOAT[::-1]])[np.random.default_rng(0).permutation(2 * len(GOOD_FLOAT) + len(BAD_FLOAT))]
    assert _sv_voxelize_counters(rows, gpu)[1] == len(BAD_FLOAT) == 28
    for bad in BAD_FLOAT:  # every one of them alone, so that no row hides behind another
        assert _sv_voxelize_counters(np.concatenate([GOOD_FLOAT, bad[None]]), gpu)[1] == 1, bad
    for levels in (None, 2):
        with pytest.raises(mrcc_amd._lib.SvHipError, match="outside the key range"):
            ME.TensorField(torch.zeros((len(rows), 1)), torch.from_numpy(rows), device=gpu).sparse(pyramid_levels=levels)


def test_int_rows_at_and_outside_the_key_range(gpu, oracle):
    import mrcc_amd
    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd import sparse

    ref = oracle.voxelize(GOOD_INT, coords_are_int=True)
    _check_voxelize(ref, *sparse._voxelize(_dev(GOOD_INT, gpu), gpu, coords_are_int=True))
    st = ME.SparseTensor(torch.zeros((len(GOOD_INT), 1)), coordinates=torch.from_numpy(GOOD_INT), device=gpu)
    assert np.array_equal(st.C.cpu().numpy(), ref["coords"])
    rows = np.concatenate([GOOD_INT, BAD_INT, GOOD_INT])[np.random.default_rng(1).permutation(2 * len(GOOD_INT) + len(BAD_INT))]
    assert _sv_voxelize_counters(rows, gpu)[1] == len(BAD_INT) == 22
    for bad in BAD_INT:
        assert _sv_voxelize_counters(np.concatenate([GOOD_INT, bad[None]]), gpu)[1] == 1, bad
    with pytest.raises(mrcc_amd._lib.SvHipError, match="outside the key range"):
        ME.SparseTensor(torch.zeros((len(rows), 1)), coordinates=torch.from_numpy(rows), device=gpu)


# ----------------------------------------------------------------------------------------------------------------------
# kernel maps and the stride pyramid on the faces of the key range and across batches
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge(gpu, oracle):
    """the range-edge cloud voxelised on the device, its oracle frame with the 17 stride-2 maps the key has room for"""
    from mrcc_amd import MinkowskiEngine as ME

    vox = edge_cloud()
    st = ME.SparseTensor(torch.zeros((len(vox), 1)), coordinates=torch.from_numpy(vox), device=gpu)
    frame = oracle.Frame(oracle.voxelize(vox, coords_are_int=True)["coords"])
    for level in range(17):
        frame.down(1 << level)
    return st.coordinate_manager, frame


def test_k3_map_on_the_range_edge_cloud(gpu, oracle, edge):
    cm, frame = edge
    coords = frame.maps[1]
    assert np.array_equal(cm.stride_map(1).coords.cpu().numpy(), coords)
    nbr = unsort(cm.plan_k3(1))
    assert np.array_equal(nbr, frame.k3(1))
    # every neighbour stays in its batch, although the same block sits in batches 0, 1 and 1023
    k, o = np.nonzero(nbr >= 0)
    assert np.array_equal(coords[nbr[k, o], 0], coords[o, 0]) and len(np.unique(coords[:, 0])) == 3
    # no wrap-around: the 18-bit fields of the key alias 131071 + 1 with -131072
    for axis, (k_plus, k_minus) in enumerate([(14, 12), (16, 10), (22, 4)]):
        at_hi, at_lo = coords[:, 1 + axis] == HI, coords[:, 1 + axis] == LO
        assert at_hi.sum() >= 8 and at_lo.sum() >= 8
        assert (nbr[k_plus, at_hi] == -1).all() and (nbr[k_minus, at_lo] == -1).all()
        assert (nbr[k_minus, at_hi] >= 0).any() and (nbr[k_plus, at_lo] >= 0).any()
    # the voxel whose key is all ones (the hash's empty marker) is found by its neighbours, and finds them
    last = len(coords) - 1
    assert coords[last].tolist() == [1023, HI, HI, HI] and (nbr[:13, last] >= 0).sum() == 7
    assert (nbr == last).sum() == 8 and nbr[14, last - 1] == last


def test_stride_pyramid_of_the_range_edge_cloud(gpu, oracle, edge):
    import mrcc_amd

    cm, frame = edge
    for level in range(17):
        ts = 1 << level
        m = cm.stride_map(2 * ts)
        assert np.array_equal(m.coords.cpu().numpy(), frame.maps[2 * ts])
        assert np.array_equal(_u64(m.keys), oracle.make_keys(frame.maps[2 * ts]))
        parent, child_start = cm.parents[ts]
        assert np.array_equal(parent.cpu().numpy().astype(np.int64), frame.parent[ts])
        want = np.searchsorted(frame.parent[ts], np.arange(m.V + 1), side="left")  # parents are non-decreasing
        assert np.array_equal(child_start.cpu().numpy(), want)
    assert set(np.unique(frame.maps[1 << 17][:, 1:])) == {LO, 0}
    for level in (0, 1, 8, 16):
        ts = 1 << level
        assert np.array_equal(unsort(cm.plan_down(ts)), frame.kdown(ts))
        assert np.array_equal(unsort(cm.plan_up(2 * ts)), frame.kup(2 * ts))
    # tensor stride 2^16: the step is 65 536, so every +1 offset of a voxel at 65 536 leaves the range
    nbr = unsort(cm.plan_k3(1 << 16))
    assert np.array_equal(nbr, frame.k3(1 << 16))
    assert (nbr[14, frame.maps[1 << 16][:, 1] == 1 << 16] == -1).all() and ((nbr >= 0).sum(axis=0) > 1).any()
    with pytest.raises(mrcc_amd._lib.SvHipError):  # the key has no 19th bit to clear
        cm.stride_map(1 << 18)


# ----------------------------------------------------------------------------------------------------------------------
# dilation
# ----------------------------------------------------------------------------------------------------------------------
def test_dilated_kernel_maps_match_oracle(gpu, oracle):
    from mrcc_amd import MinkowskiEngine as ME

    rng = np.random.default_rng(7)
    g = np.arange(-12, 12)
    block = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    vox = np.concatenate([np.concatenate([np.full((m.sum(), 1), b), block[m]], axis=1)
                          for b, m in ((0, rng.random(len(block)) < 0.3), (3, rng.random(len(block)) < 0.3))]).astype(np.int32)
    vox = vox[rng.permutation(len(vox))]
    st = ME.SparseTensor(torch.zeros((len(vox), 1)), coordinates=torch.from_numpy(vox), device=gpu)
    cm = st.coordinate_manager
    frame = oracle.Frame(oracle.voxelize(vox, coords_are_int=True)["coords"])
    frame.down(1), frame.down(2)
    for ts, dilation in [(1, 2), (1, 3), (2, 2), (4, 3)]:
        got = unsort(cm.plan_k3(ts, dilation))
        want = oracle.kernel_map_k3(frame.maps[ts], ts, dilation)
        assert np.array_equal(got, want)
        assert (want >= 0).sum() > 2 * want.shape[1]  # neighbours beside the centre
        assert not np.array_equal(got, frame.k3(ts))  # and not the dilation-1 map
        assert cm.plan_k3(ts, dilation) is not cm.plan_k3(ts)


# ----------------------------------------------------------------------------------------------------------------------
# hash table at exactly the allowed load, with a probe chain that wraps past the last slot
# ----------------------------------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1


def _hash64_int(k):
    """hash64 of csrc/sv_common.h (the 64-bit finaliser of MurmurHash3) on Python ints"""
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & M64
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & M64
    k ^= k >> 33
    return k


def _hash64(keys):
    k = keys.astype(np.uint64)
    with np.errstate(over="ignore"):
        k = k ^ (k >> np.uint64(33))
        k = k * np.uint64(0xFF51AFD7ED558CCD)
        k = k ^ (k >> np.uint64(33))
        k = k * np.uint64(0xC4CEB9FE1A85EC53)
        k = k ^ (k >> np.uint64(33))
    return k


def _hash_build(keys, cap, gpu):
    from mrcc_amd._lib import call, ptr, stream_ptr

    dk = _dev(keys.view(np.int64), gpu)
    tk = torch.full((cap,), 5, dtype=torch.int64, device=gpu)
    tv = torch.full((cap,), -9, dtype=torch.int32, device=gpu)
    call("sv_hash_build", ptr(dk), c_int64(len(keys)), ptr(tk), ptr(tv), c_int64(cap), stream_ptr())
    return tk, tv


def _kernel_map_k3(coords, tk, tv, cap, gpu, tensor_stride=1, dilation=1):
    from mrcc_amd._lib import call, ptr, stream_ptr

    V, ld = len(coords), len(coords) + 3
    dc = _dev(coords.astype(np.int32), gpu)
    nbr = torch.full((27, ld), -5, dtype=torch.int32, device=gpu)
    mask = torch.full((V,), -5, dtype=torch.int32, device=gpu)
    call("sv_kernel_map_k3", ptr(dc), c_int64(V), c_int(tensor_stride), c_int(dilation), ptr(tk), ptr(tv), c_int64(cap),
         ptr(nbr), c_int64(ld), ptr(mask), stream_ptr())
    nbr = nbr.cpu().numpy()
    assert (nbr[:, V:] == -5).all()  # the padding columns of the table are not written
    bits = ((nbr[:, :V] >= 0).astype(np.int64) << np.arange(27)[:, None]).sum(axis=0)
    assert np.array_equal(mask.cpu().numpy().view(np.uint32).astype(np.int64), bits)
    return nbr[:, :V]


def _check_table(tk, tv, keys):
    """the table as a key -> row map: exactly the V keys, each with its row, every other slot empty"""
    tk, tv = _u64(tk), tv.cpu().numpy()
    by_key = np.argsort(tk, kind="stable")
    V = len(keys)
    assert np.array_equal(tk[by_key][:V], keys) and (tk[by_key][V:] == EMPTY).all()
    assert np.array_equal(tv[by_key][:V], np.arange(V))
    return tk


@pytest.mark.parametrize("present", [True, False])
def test_the_voxel_whose_key_is_the_empty_marker(gpu, oracle, present):
    """(1023, 131071, 131071, 131071) has the key 0xffff...f, which marks an empty hash slot.  The table must not hold it,
    and the kernel map must still resolve it: present -> its row (the last one), absent -> -1 and not the value of whatever
    empty slot a probe for it would stop at (the value array is pre-filled with -9 here, the key array with 5)."""
    cap = 128
    r3 = range(3)
    vox = np.array([(1023, HI - i, HI - j, HI - k) for i in r3 for j in r3 for k in r3 if present or i + j + k > 0]
                   + [(b, HI - i, HI, HI) for b in (0, 1022) for i in r3])
    # voxels whose home slots are the marker's own and the two behind it: whichever of them claims a slot first, the probe
    # sequence of the marker is occupied by real keys
    g = np.arange(-16, 16)
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    grid = np.concatenate([np.full((len(grid), 1), 7), grid], axis=1)
    home = (_hash64(oracle.make_keys(grid)) & np.uint64(cap - 1)).astype(np.int64)
    h = _hash64_int(M64) & (cap - 1)
    vox = np.concatenate([vox] + [grid[home == (h + d) % cap][:2] for d in range(3)])
    coords = oracle.voxelize(vox, coords_are_int=True)["coords"]
    keys = oracle.make_keys(coords)
    V = len(keys)
    assert (keys[-1] == EMPTY) == present and V == (27 if present else 26) + 6 + 6 and cap >= 2 * V
    tk, tv = _hash_build(keys, cap, gpu)
    _check_table(tk, tv, keys[keys != EMPTY])
    nbr = _kernel_map_k3(coords, tk, tv, cap, gpu)
    assert np.array_equal(nbr, oracle.kernel_map_k3(coords, 1))
    assert not present or (nbr == V - 1).sum() == 8  # its seven neighbours and itself


def test_hash64_in_numpy_is_the_murmur3_finaliser():
    ks = [0, 1, 2, 0x123456789ABCDEF, (1 << 54) - 1, 1023 << 54, M64 - 1, M64]
    assert [int(h) for h in _hash64(np.array(ks, np.uint64))] == [_hash64_int(k) for k in ks]
    assert _hash64_int(1) == 0xB456BCFC34C2CB2C and _hash64_int(0) == 0  # published values of fmix64


def test_hash_at_full_load_with_a_wrapping_probe_chain(gpu, oracle):
    """V = 512 keys that all hash into the last 64 slots of a 1024-slot table: every insertion collides, the chain runs
    past slot 1023 and continues at slot 0, and lookups walk up to ~500 slots"""
    cap, V = 1024, 512
    g = np.arange(-64, 64)
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    grid = np.concatenate([np.full((len(grid), 1), 5), grid], axis=1)
    keys = oracle.make_keys(grid)
    home = _hash64(keys) & np.uint64(cap - 1)
    cand = np.nonzero(home >= np.uint64(cap - 64))[0]
    pick = cand[np.argsort(keys[cand])[:V]]  # the first V in key order: a compact block, so that voxels have neighbours
    pick = pick[np.argsort(keys[pick])]
    keys, coords, home = keys[pick], grid[pick].astype(np.int32), home[pick].astype(np.int64)
    assert len(keys) == V and cap == 2 * V
    tk, tv = _hash_build(keys, cap, gpu)
    tk_np = _check_table(tk, tv, keys)
    # linear probing from homes inside [960, 1024): the occupied slots are one cyclic run that starts at the lowest home
    # (this also pins the numpy hash above to the device's)
    used = np.nonzero(tk_np != EMPTY)[0]
    assert np.array_equal(used, np.sort((home.min() + np.arange(V)) % cap)) and used[0] == 0 and used[-1] == cap - 1
    displacement = (used - home[np.searchsorted(keys, tk_np[used])]) % cap  # slots between a key's home and where it sits
    assert displacement.max() > 64  # chains far longer than a bounded probe would follow
    nbr = _kernel_map_k3(coords, tk, tv, cap, gpu)
    want = oracle.kernel_map_k3(coords, 1)
    assert np.array_equal(nbr, want) and (want >= 0).sum() > 1.5 * V


def test_hash_with_well_spread_keys_at_full_load(gpu, oracle):
    cap, V = 8192, 4096
    rng = np.random.default_rng(11)
    vox = np.concatenate([rng.choice(BATCHES, size=(2 * V, 1)), rng.integers(LO, HI + 1, size=(2 * V, 3))], axis=1)
    vox[:, 1:] = np.where(rng.random((2 * V, 3)) < 0.5, vox[:, 1:], vox[:, 1:] // 4096 * 4096 + rng.integers(0, 3, size=(2 * V, 3)))
    coords = oracle.voxelize(vox, coords_are_int=True)["coords"]
    coords = coords[np.sort(rng.choice(len(coords), V, replace=False))]
    keys = oracle.make_keys(coords)
    assert len(keys) == V and keys[-1] != EMPTY
    tk, tv = _hash_build(keys, cap, gpu)
    _check_table(tk, tv, keys)
    assert np.array_equal(_kernel_map_k3(coords, tk, tv, cap, gpu), oracle.kernel_map_k3(coords, 1))


@pytest.mark.parametrize("V,cap", [(512, 1023), (512, 512), (100, 300), (0, 0), (3, 6)])
def test_hash_build_rejects_a_table_that_is_too_small_or_no_power_of_two(gpu, V, cap):
    from mrcc_amd._lib import load, ptr, stream_ptr

    keys = torch.arange(max(V, 1), dtype=torch.int64, device=gpu)
    tk = torch.full((max(cap, 1),), 5, dtype=torch.int64, device=gpu)
    tv = torch.full((max(cap, 1),), -9, dtype=torch.int32, device=gpu)
    rc = load().sv_hash_build(ptr(keys), c_int64(V), ptr(tk), ptr(tv), c_int64(cap), stream_ptr())
    assert rc == SV_ERR_INVALID
    assert (tk == 5).all() and (tv == -9).all()  # rejected on the host: nothing was launched


# ----------------------------------------------------------------------------------------------------------------------
# sv_plan_build on synthetic neighbour tables: every mask bit varies, K beyond 8 and 27
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 8, 13, 27, 32])
@pytest.mark.parametrize("V", [1, 127, 128, 129, 8192, 8193, 20_000])
def test_plan_build_on_synthetic_tables(gpu, V, K):
    """perm is the stable argsort of the Gray key over ALL K mask bits (sort passes of 1 to 32 key bits; 8192 rows take
    the single-workgroup sort, 8193 the multi-workgroup one), nbr_s the gathered table rebased by nbr_base, submask and
    tile_order as include/sv_hip.h defines them."""
    from mrcc_amd._lib import call, load, ptr, stream_ptr

    rng = np.random.default_rng(1000 * K + V)
    mask = rng.integers(0, 1 << K, size=V, dtype=np.uint64).astype(np.uint32)  # uniform: every bit varies
    ld, V_in = V + 5, V + 17
    Vpad = (V + 127) // 128 * 128
    tiles = Vpad // 128
    key = gray_key(mask, K)
    want_perm = np.argsort(key, kind="stable")
    for nbr_base in (0, 1000):
        present = ((mask[None, :] >> np.arange(K, dtype=np.uint32)[:, None]) & 1).astype(bool)
        nbr = np.full((K, ld), 123456, np.int32)  # columns V .. ld - 1 are never read
        nbr[:, :V] = np.where(present, rng.integers(nbr_base, nbr_base + V_in, size=(K, V)), -1)
        d_nbr, d_mask = _dev(nbr, gpu), _dev(mask.view(np.int32), gpu)
        ws_bytes = load().sv_plan_workspace_bytes(c_int64(V))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=gpu)
        perm = torch.full((Vpad,), -7, dtype=torch.int32, device=gpu)
        nbr_s = torch.full((K, Vpad), -7, dtype=torch.int32, device=gpu)
        submask = torch.full((tiles, K), -7, dtype=torch.int32, device=gpu)
        tile_order = torch.full((tiles,), -7, dtype=torch.int32, device=gpu)
        call("sv_plan_build", ptr(d_nbr), c_int64(ld), ptr(d_mask), c_int(K), c_int64(V), c_int64(nbr_base), ptr(ws),
             c_size_t(ws_bytes), ptr(perm), ptr(nbr_s), ptr(submask), ptr(tile_order), c_int64(Vpad), stream_ptr())
        perm, nbr_s = perm.cpu().numpy(), nbr_s.cpu().numpy()
        assert np.array_equal(perm[:V], want_perm) and (perm[V:] == -1).all()
        want_s = np.full((K, Vpad), -1, np.int32)
        g = nbr[:, :V][:, want_perm]
        want_s[:, :V] = np.where(g >= 0, g - nbr_base, -1)
        assert np.array_equal(nbr_s, want_s)
        sub = (want_s >= 0).reshape(K, tiles, 8, 16).any(axis=3)  # [K, tiles, 8]: sub-tile s of tile t has offset k
        bits = (sub * (1 << np.arange(8))).sum(axis=2).T
        assert np.array_equal(submask.cpu().numpy().astype(np.int64), bits)
        cost = sub.sum(axis=(0, 2))
        assert np.array_equal(tile_order.cpu().numpy(), np.argsort(255 - np.minimum(cost, 255), kind="stable"))
    if V == 20_000:
        assert len(np.unique(key >> (K - 1))) == 2 and (K == 1 or len(np.unique(cost)) > 1)  # top key bit, tile costs vary


# ----------------------------------------------------------------------------------------------------------------------
# composite = piecewise on the range-edge cloud
# ----------------------------------------------------------------------------------------------------------------------
def test_frame_composites_equal_the_piecewise_calls_on_the_range_edge_cloud(gpu):
    """sv_frame_maps / sv_frame_plans on keys that use all 64 bits, batches up to 1023, six levels, offset-range plans"""
    from test_gpu_frame import check_composites_equal_piecewise

    vox = edge_cloud()
    f = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, size=(len(vox), 3)).astype(np.float32))
    check_composites_equal_piecewise(gpu, torch.from_numpy(vox.astype(np.float32)), f, levels=6, rules="100:14;20:9,18")
