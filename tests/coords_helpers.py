"""Helpers shared by the coordinate tests (test_gpu_voxelize.py, test_gpu_coords_edges.py): the sort key of sv_plan_build
restated in numpy, and the inverse of a conv plan's row sort."""
import numpy as np


def gray_key(mask, K):
    """sort key of sv_plan_build (csrc/sv_coords.hip iota_key_kernel): rarest offsets (corners, edges, faces, centre) as
    the most significant bits, then the rank in reflected-Gray order."""
    m = mask.astype(np.int64)
    if K == 27:
        pos, rank = {}, 0
        for cls in (3, 2, 1, 0):
            for k in range(27):
                if abs(k % 3 - 1) + abs((k // 3) % 3 - 1) + abs(k // 9 - 1) == cls:
                    pos[k] = 26 - rank
                    rank += 1
        m2 = np.zeros_like(m)
        for k in range(27):
            m2 |= ((m >> k) & 1) << pos[k]
        m = m2
    for s in (1, 2, 4, 8, 16):
        m ^= m >> s
    return m


def unsort(plan):
    """Undo the mask sort: nbr in canonical output-row order."""
    perm = plan.perm.cpu().numpy()
    nbr_s = plan.nbr_s.cpu().numpy()
    valid = perm >= 0
    assert valid.sum() == plan.V_out and np.array_equal(np.sort(perm[valid]), np.arange(plan.V_out))
    out = np.full((plan.K, plan.V_out), -2, np.int32)
    out[:, perm[valid]] = nbr_s[:, valid]
    assert np.all(nbr_s[:, ~valid] == -1)
    # submask bit s of tile t for offset k <=> some row of that 16-row sub-tile has a neighbour at k
    sub = (nbr_s >= 0).reshape(plan.K, plan.Vpad // 128, 8, 16).any(axis=3)  # [K, tiles, 8]
    bits = (sub * (1 << np.arange(8))).sum(axis=2).T  # [tiles, K]
    assert np.array_equal(plan.submask.cpu().numpy().astype(np.int64), bits)
    # tile_order: a permutation of the plan tiles, work (active sub-tile slots) non-increasing
    order = plan.tile_order.cpu().numpy()
    assert np.array_equal(np.sort(order), np.arange(plan.Vpad // 128))
    work = sub.sum(axis=(0, 2))[order]
    assert np.all(np.diff(work) <= 0)
    return out


def check_plan_order(plan, K):
    """perm is EXACTLY the stable sort of the rows by the Gray key of their neighbour mask, tile_order the stable sort of
    the plan tiles by work, descending"""
    V = plan.V_out
    perm = plan.perm.cpu().numpy()
    nbr_s = plan.nbr_s.cpu().numpy()
    assert np.array_equal(np.sort(perm[:V]), np.arange(V)) and (perm[V:] == -1).all()
    mask_sorted = np.zeros(plan.Vpad, np.int64)
    for k in range(K):
        mask_sorted |= (nbr_s[k] >= 0).astype(np.int64) << k
    mask = np.zeros(V, np.int64)
    mask[perm[:V]] = mask_sorted[:V]
    want = np.argsort(gray_key(mask, K), kind="stable")
    assert np.array_equal(perm[:V], want)
    sub = plan.submask.cpu().numpy().astype(np.uint32)
    cost = np.array([[bin(int(v)).count("1") for v in row] for row in sub]).sum(axis=1)
    assert np.array_equal(plan.tile_order.cpu().numpy(), np.argsort(255 - np.minimum(cost, 255), kind="stable"))


COORD_LO, COORD_HI = -(1 << 17), (1 << 17) - 1  # the key range per axis (include/sv_hip.h)


def edge_cloud(seed=0):
    """A few hundred distinct voxels (int32 [n, 4], shuffled) on the edges of the key range: the eight range corners in
    batches 0 and 1023 (one of them has the all-ones key), runs of three voxels up to both faces of every axis, 3^3 blocks
    in two opposite corners, and the same partly occupied 5^3 block around the origin in batches 0, 1 and 1023."""
    lo, hi = COORD_LO, COORD_HI
    rows = [(b, x, y, z) for b in (0, 1023) for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)]
    for b in (0, 1023):
        for axis in range(3):
            for run in (range(hi - 2, hi + 1), range(lo, lo + 3)):
                for v in run:
                    c = [5, -7, 11]
                    c[axis] = v
                    rows.append((b, *c))
    r3 = range(3)
    rows += [(1023, hi - i, hi - j, hi - k) for i in r3 for j in r3 for k in r3]
    rows += [(0, lo + i, lo + j, lo + k) for i in r3 for j in r3 for k in r3]
    rng = np.random.default_rng(seed)
    block = [(x, y, z) for x in range(-2, 3) for y in range(-2, 3) for z in range(-2, 3) if rng.random() < 0.7]
    rows += [(b, *c) for b in (0, 1, 1023) for c in block]
    vox = np.unique(np.array(rows, np.int32), axis=0)
    return vox[rng.permutation(len(vox))]
