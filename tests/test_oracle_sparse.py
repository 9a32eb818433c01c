"""Self-consistency of the sparse oracle (its parity with MinkowskiEngine is unpinned): the sparse
convolution must equal a dense torch conv3d on the active sites; BN fold vs torch BatchNorm1d; voxelisation laws."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F


def _random_sparse(rng, n=600, extent=12, batch=2, neg=True):
    c = rng.integers(-extent if neg else 0, extent, size=(n, 3))
    b = rng.integers(0, batch, size=(n, 1))
    return np.unique(np.concatenate([b, c], axis=1), axis=0).astype(np.int32)


def _to_dense(coords, feats, lo, size, batch):
    C = feats.shape[1]
    vol = torch.zeros(batch, C, size, size, size, dtype=torch.float64)
    idx = coords[:, 1:] - lo
    vol[coords[:, 0], :, idx[:, 2], idx[:, 1], idx[:, 0]] = torch.from_numpy(feats).double()  # [b, c, z, y, x]
    return vol


def test_k3_conv_equals_dense_conv3d(oracle):
    rng = np.random.default_rng(0)
    coords = _random_sparse(rng)
    vox = oracle.voxelize(np.concatenate([coords[:, :1], coords[:, 1:]], axis=1), coords_are_int=True)
    coords = vox["coords"]
    V, cin, cout = len(coords), 5, 7
    feats = rng.normal(size=(V, cin)).astype(np.float32)
    W = rng.normal(size=(27, cin, cout)).astype(np.float32)
    out = oracle.conv(feats, W, oracle.kernel_map_k3(coords, 1), V)
    lo, size = -14, 30
    vol = _to_dense(coords, feats, lo, size, 2)
    # offset index k = (dx+1) + 3(dy+1) + 9(dz+1)  ->  conv3d weight [cout, cin, kz, ky, kx]
    w = torch.from_numpy(W).double().reshape(3, 3, 3, cin, cout).permute(4, 3, 0, 1, 2)
    dense = F.conv3d(vol, w, padding=1)
    idx = coords[:, 1:] - lo
    want = dense[coords[:, 0], :, idx[:, 2], idx[:, 1], idx[:, 0]].numpy()
    assert np.abs(out - want).max() < 1e-4


def test_strided_and_transposed_conv_equal_dense(oracle):
    rng = np.random.default_rng(1)
    coords = oracle.voxelize(_random_sparse(rng, n=500, extent=8), coords_are_int=True)["coords"]
    frame = oracle.Frame(coords)
    coarse = frame.down(1)
    # floor semantics for negative coordinates
    assert np.array_equal(np.unique(np.concatenate([coords[:, :1], (coords[:, 1:] // 2) * 2], axis=1), axis=0),
                          coarse[np.lexsort(coarse.T[::-1])])
    cin, cout = 4, 6
    feats = rng.normal(size=(len(coords), cin)).astype(np.float32)
    W = rng.normal(size=(8, cin, cout)).astype(np.float32)
    down = oracle.conv(feats, W, frame.kdown(1), len(coarse))
    lo, size = -8, 16
    vol = _to_dense(coords, feats, lo, size, 2)
    w = torch.from_numpy(W).double().reshape(2, 2, 2, cin, cout).permute(4, 3, 0, 1, 2)  # k = dx + 2dy + 4dz
    dense = F.conv3d(vol, w, stride=2)
    ci = (coarse[:, 1:] - lo) // 2
    assert np.abs(down - dense[coarse[:, 0], :, ci[:, 2], ci[:, 1], ci[:, 0]].numpy()).max() < 1e-4
    # transposed: coarse -> the existing fine map
    featc = rng.normal(size=(len(coarse), cin)).astype(np.float32)
    up = oracle.conv(featc, W, frame.kup(2), len(coords))
    volc = torch.zeros(2, cin, size // 2, size // 2, size // 2, dtype=torch.float64)
    volc[coarse[:, 0], :, ci[:, 2], ci[:, 1], ci[:, 0]] = torch.from_numpy(featc).double()
    wt = torch.from_numpy(W).double().reshape(2, 2, 2, cin, cout).permute(3, 4, 0, 1, 2)  # [cin, cout, kz, ky, kx]
    dense_up = F.conv_transpose3d(volc, wt, stride=2)
    fi = coords[:, 1:] - lo
    assert np.abs(up - dense_up[coords[:, 0], :, fi[:, 2], fi[:, 1], fi[:, 0]].numpy()).max() < 1e-4


def test_bn_fold_linear_and_pool_vs_torch(oracle):
    rng = np.random.default_rng(2)
    x = rng.normal(size=(300, 16)).astype(np.float32)
    bn = torch.nn.BatchNorm1d(16).eval()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_()
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)
    s, b = oracle.fold_bn(bn.weight.detach().numpy(), bn.bias.detach().numpy(), bn.running_mean.numpy(), bn.running_var.numpy())
    got = oracle.affine_act(x, s, b, None, oracle.ACT_RELU)
    want = torch.relu(bn(torch.from_numpy(x))).detach().numpy()
    assert np.abs(got - want).max() < 1e-5
    lin = torch.nn.Linear(16, 9)
    got = oracle.conv(x, lin.weight.detach().numpy().T[None], None, 300, None, lin.bias.detach().numpy())
    assert np.abs(got - lin(torch.from_numpy(x)).detach().numpy()).max() < 1e-5
    coords = np.zeros((300, 4), np.int32)
    coords[:, 0] = np.sort(rng.integers(0, 3, size=300))
    mx = oracle.global_pool(x, coords, oracle.POOL_MAX)
    av = oracle.global_pool(x, coords, oracle.POOL_AVG)
    for bidx in range(3):
        m = coords[:, 0] == bidx
        assert np.array_equal(mx[bidx], x[m].max(axis=0)) and np.abs(av[bidx] - x[m].mean(axis=0)).max() < 1e-5


def test_voxelize_laws(oracle):
    import mrcc_amd

    pts, rgb, _ = mrcc_amd.synth.gen_room(5000, 0.6, 4)
    pts -= 0.3
    c4 = np.concatenate([np.zeros((len(pts), 1), np.float32), pts * 50], axis=1)
    v = oracle.voxelize(c4)
    q = np.floor(c4[:, 1:]).astype(np.int32)
    assert np.array_equal(v["coords"][v["inverse"]][:, 1:], q)  # every point lands in floor(coord)
    assert np.all(np.diff(v["keys"].astype(np.uint64)) > 0)  # canonical order, unique
    feats = oracle.voxel_reduce(rgb, v["order"], v["seg_start"], 0)
    sums = np.zeros_like(feats, dtype=np.float64)
    np.add.at(sums, v["inverse"], rgb.astype(np.float64))
    cnt = np.bincount(v["inverse"], minlength=len(feats))[:, None]
    assert np.abs(feats - sums / cnt).max() < 1e-6
    # idempotence: voxelising the voxel coordinates again is the identity
    v2 = oracle.voxelize(v["coords"], coords_are_int=True)
    assert np.array_equal(v2["coords"], v["coords"]) and np.array_equal(v2["inverse"], np.arange(len(feats)))
    # shuffling the points permutes `inverse` only
    perm = np.random.default_rng(0).permutation(len(pts))
    v3 = oracle.voxelize(c4[perm])
    assert np.array_equal(v3["keys"], v["keys"]) and np.array_equal(v3["inverse"], v["inverse"][perm])


# ------------------------------------------------------------------------------------------------------------------
# key range and key packing (include/sv_hip.h: voxel coordinates in [-2^17, 2^17 - 1] per axis, batch in [0, 1023])
# ------------------------------------------------------------------------------------------------------------------
LO, HI = -(1 << 17), (1 << 17) - 1


def _key_by_bits(b, x, y, z):
    """the key definition of include/sv_hip.h, bit by bit on Python ints (shares no code with the oracle)"""
    k = 0
    for j in range(18):
        k |= (((x + (1 << 17)) >> j) & 1) << (3 * j)
        k |= (((y + (1 << 17)) >> j) & 1) << (3 * j + 1)
        k |= (((z + (1 << 17)) >> j) & 1) << (3 * j + 2)
    return k | (b << 54)


def _full_range_voxels(rng, n):
    return np.concatenate([rng.choice([0, 1, 511, 1022, 1023], size=(n, 1)), rng.integers(LO, HI + 1, size=(n, 3))], axis=1)


def test_make_keys_equals_the_bitwise_definition(oracle):
    corners = [(b, x, y, z) for b in (0, 1023) for x in (LO, HI) for y in (LO, HI) for z in (LO, HI)]
    vox = np.concatenate([np.array(corners), _full_range_voxels(np.random.default_rng(0), 300)])
    got = oracle.make_keys(vox)
    assert got.dtype == np.uint64
    assert [int(k) for k in got] == [_key_by_bits(*map(int, v)) for v in vox]
    assert int(oracle.make_keys(np.array([[1023, HI, HI, HI]]))[0]) == (1 << 64) - 1  # every key bit is in use
    assert int(oracle.make_keys(np.array([[0, LO, LO, LO]]))[0]) == 0


def test_key_order_is_batch_then_morton(oracle):
    vox = np.unique(_full_range_voxels(np.random.default_rng(1), 400), axis=0)
    vox = vox[np.random.default_rng(2).permutation(len(vox))]
    morton = [_key_by_bits(0, *map(int, v[1:])) for v in vox]
    want = sorted(range(len(vox)), key=lambda i: (int(vox[i, 0]), morton[i]))
    assert np.argsort(oracle.make_keys(vox), kind="stable").tolist() == want
    assert np.array_equal(oracle.voxelize(vox, coords_are_int=True)["coords"], vox[want])


def test_key_range_edges_are_accepted(oracle):
    edge = np.array([[0, LO, HI, 0], [1023, HI, LO, LO]])
    assert np.array_equal(oracle.voxelize(edge, coords_are_int=True)["coords"], edge)
    f = np.array([[-0.0, -131072.0, -131071.5, np.nextafter(np.float32(131072), np.float32(0))],
                  [1023.0, -0.0, -1e-7, 0.99999994]], np.float32)
    assert np.array_equal(oracle.voxelize(f)["coords"], [[0, LO, LO, HI], [1023, 0, -1, 0]])


@pytest.mark.parametrize("row", [(0, HI + 1, 0, 0), (0, 0, LO - 1, 0), (0, 0, 0, HI + 1), (-1, 0, 0, 0), (1024, 0, 0, 0)])
def test_out_of_range_int_rows_raise(oracle, row):
    vox = np.array([[0, 1, 2, 3], row])
    with pytest.raises(ValueError):
        oracle.make_keys(vox)
    with pytest.raises(ValueError):
        oracle.voxelize(vox, coords_are_int=True)


@pytest.mark.parametrize("row", [(0, 131072.0, 0, 0), (0, 0, -131072.5, 0), (0, 0, 0, -131073.0), (-0.5, 0, 0, 0), (-1, 0, 0, 0),
                                 (1024, 0, 0, 0), (np.nan, 0, 0, 0), (0, np.nan, 0, 0), (0, 0, np.inf, 0), (0, 0, 0, -np.inf),
                                 (0, 1e30, 0, 0)])
def test_out_of_range_float_rows_raise(oracle, row):
    with pytest.raises(ValueError):
        oracle.voxelize(np.array([[0, 1.5, 2.5, 3.5], row], np.float32))


def test_kernel_map_does_not_wrap_at_the_range_edge(oracle):
    """the key holds 18 bits per axis: x = 131071 + 1 would alias x = -131072 if the range check were missing"""
    coords = oracle.voxelize(np.array([[3, HI, 7, -9], [3, LO, 7, -9], [3, HI - 1, 7, -9], [3, LO + 1, 7, -9]]),
                             coords_are_int=True)["coords"]
    nbr = oracle.kernel_map_k3(coords, 1)
    row = {tuple(c): i for i, c in enumerate(coords.tolist())}
    hi, lo = row[(3, HI, 7, -9)], row[(3, LO, 7, -9)]
    assert nbr[14, hi] == -1 and nbr[12, lo] == -1          # +x of the last voxel, -x of the first
    assert nbr[12, hi] == row[(3, HI - 1, 7, -9)] and nbr[14, lo] == row[(3, LO + 1, 7, -9)]
    assert (nbr[13] == np.arange(4)).all() and (nbr >= 0).sum() == 4 + 4


def _kernel_map_by_dict(coords, step):
    row = {tuple(c): i for i, c in enumerate(coords.tolist())}
    nbr = np.full((27, len(coords)), -1, np.int32)
    for o, (b, x, y, z) in enumerate(coords.tolist()):
        for k in range(27):
            nbr[k, o] = row.get((b, x + (k % 3 - 1) * step, y + (k // 3 % 3 - 1) * step, z + (k // 9 - 1) * step), -1)
    return nbr


@pytest.mark.parametrize("ts,dilation", [(1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (2, 3)])
def test_kernel_map_dilation_and_tensor_stride_equal_a_dictionary_lookup(oracle, ts, dilation):
    rng = np.random.default_rng(10 * ts + dilation)
    coords = _random_sparse(rng, n=900, extent=7)
    coords[:, 1:] *= ts
    coords = oracle.voxelize(coords, coords_are_int=True)["coords"]
    got = oracle.kernel_map_k3(coords, ts, dilation)
    assert np.array_equal(got, _kernel_map_by_dict(coords, ts * dilation))
    assert (got >= 0).sum() > 3 * len(coords)  # the lookup is not vacuous
    if dilation > 1:
        assert not np.array_equal(got, oracle.kernel_map_k3(coords, ts, 1))
