"""Device path of ClusterUtil.get_largest_cluster (csrc/sv_cluster.hip) against the oracle's flood fill
(oracle.single_linkage_roots, pinned against sklearn in tests/test_cluster_cpu.py) and the host k-d-tree path."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _scene(rng, n_blob=600, dtype=np.float32):
    blob = lambda c, n, s=0.02: rng.normal(0, s, size=(n, 3)) + np.asarray(c)
    chain = np.stack([np.arange(80) * 0.055, np.zeros(80), np.zeros(80)], axis=1) + [1.0, 1.0, 0.0]
    pts = np.concatenate([blob([0, 0, 0], n_blob), blob([0.3, 0, 0], n_blob // 3), blob([0, 0.4, 0.1], 50), chain,
                          rng.uniform(-1, 1, size=(40, 3))])
    return pts[rng.permutation(len(pts))].astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_roots_and_largest_cluster_match_the_oracle(dtype):
    from mrcc_amd.utils.output import ClusterUtil, single_linkage_roots
    from oracle import sv_oracle as O

    rng = np.random.default_rng(0)
    pts = _scene(rng, dtype=dtype)
    want = O.single_linkage_roots(pts, 0.06)
    root, best = single_linkage_roots(torch.from_numpy(pts).to(_dev()), 0.06)
    torch.cuda.synchronize()
    assert np.array_equal(root.cpu().numpy(), want)  # root = smallest member: identical labelling, not just partition
    u, c = np.unique(want, return_counts=True)
    assert best.cpu().tolist() == [int(u[c.argmax()]), int(c.max())]
    got = ClusterUtil().get_largest_cluster(torch.from_numpy(pts).to(_dev()))
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), O.largest_cluster(pts, 0.06))
    assert np.array_equal(got.cpu().numpy(), ClusterUtil().get_largest_cluster(pts))  # host path of the same class


def test_threshold_is_strict_ties_go_to_the_lowest_index_and_tiny_inputs():
    from mrcc_amd.utils.output import ClusterUtil, single_linkage_roots

    d = _dev()
    # exactly dist apart: not connected (sklearn merges below the threshold); one ulp closer: connected
    pts = torch.tensor([[0.0, 0, 0], [0.5, 0, 0], [2.0, 0, 0], [2.0, np.nextafter(0.5, 0), 0]], dtype=torch.float64, device=d)
    root, best = single_linkage_roots(pts, 0.5)
    assert root.cpu().tolist() == [0, 1, 2, 2] and best.cpu().tolist() == [2, 2]
    # two clusters of three: the one with the lowest index wins, wherever its points sit in the array
    pts = torch.tensor([[5, 5, 5], [0, 0, 0], [5.01, 5, 5], [0.01, 0, 0], [0, 0.01, 0], [5, 5.01, 5]], dtype=torch.float32, device=d)
    assert ClusterUtil().get_largest_cluster(pts).cpu().tolist() == [0, 2, 5]
    assert ClusterUtil().get_largest_cluster(pts[1:]).cpu().tolist() == [0, 2, 3]
    assert ClusterUtil().get_largest_cluster(pts[:1]).cpu().tolist() == [0]
    assert ClusterUtil().get_largest_cluster(pts[:0]).numel() == 0
    # duplicates are at distance 0 < dist
    dup = torch.zeros(300, 3, device=d)
    assert ClusterUtil().get_largest_cluster(dup).cpu().tolist() == list(range(300))


def test_index_indirection_and_a_dense_blob_of_several_tiles():
    """idx selects rows of a bigger cloud (the engine's EE points inside the frame); 5 000 points inside one 6-cm ball
    neighbourhood structure = millions of unions racing on the same forest; a long chain = deep trees."""
    from mrcc_amd.utils.output import ClusterUtil, single_linkage_roots
    from oracle import sv_oracle as O

    rng = np.random.default_rng(3)
    cloud = np.concatenate([rng.uniform([-0.05, -0.11, -0.065], [0.05, 0.11, 0.065], size=(5000, 3)),
                            np.stack([np.arange(3000) * 0.05, np.full(3000, 3.0), np.zeros(3000)], axis=1),
                            rng.uniform(-2, 2, size=(2000, 3))]).astype(np.float32)
    cloud = cloud[rng.permutation(len(cloud))]
    idx = np.sort(rng.choice(len(cloud), 7000, replace=False))
    sub = cloud[idx]
    root, best = single_linkage_roots(torch.from_numpy(cloud).to(_dev()), 0.06, idx=torch.from_numpy(idx).to(_dev()))
    want = O.single_linkage_roots(sub, 0.06)
    assert np.array_equal(root.cpu().numpy(), want)
    got = ClusterUtil().get_largest_cluster(torch.from_numpy(cloud).to(_dev()), idx=torch.from_numpy(idx).to(_dev()))
    assert np.array_equal(got.cpu().numpy(), O.largest_cluster(sub, 0.06))
    # run to run: the unions race, the result does not
    for _ in range(3):
        r2, _ = single_linkage_roots(torch.from_numpy(cloud).to(_dev()), 0.06, idx=torch.from_numpy(idx).to(_dev()))
        assert torch.equal(r2, root)


def test_select_equal_is_np_where():
    from mrcc_amd.utils.output import select_equal

    rng = np.random.default_rng(5)
    for n, dt in ((0, np.int64), (1, np.int64), (1023, np.int32), (1024, np.int64), (200_003, np.int64), (70_000, np.int32)):
        v = rng.integers(0, 3, size=n).astype(dt)
        t = torch.from_numpy(v).to(_dev())
        for value in (2, 7):
            got = select_equal(t, value)
            assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), np.where(v == value)[0])
        if n:
            got = select_equal(t, torch.tensor([1], dtype=torch.int32, device=_dev()))
            assert np.array_equal(got.cpu().numpy(), np.where(v == 1)[0])


# ---- structure edges: tile boundaries, non-finite rows, argmax ties beyond one pass of the reduction, strided float64 ------
# (a, b, offset of b from a along y): first and last thread of the diagonal tile; a link that exists only across two tiles;
# the same one tile further; the first point of the third tile.  Together: 512 - 0 - 255 - 256 - 511, a chain 0.4 apart.
PAIRS = [(0, 255, 0.4), (255, 256, 0.4), (256, 511, 0.4), (0, 512, -0.4)]


@pytest.mark.parametrize("n", [255, 256, 257, 512, 513])
def test_links_that_exist_only_across_or_inside_a_256_point_tile(n):
    import post_helpers as P
    from mrcc_amd.utils.output import single_linkage_roots
    from oracle import sv_oracle as O

    pairs = [p for p in PAIRS if p[1] < n]
    for chosen in [[]] + [[p] for p in pairs] + ([pairs] if len(pairs) > 1 else []):
        pts = P.lattice(n)
        want = np.arange(n)
        for a, b, step in chosen:  # in chain order: a is in place before b moves beside it
            P.link(pts, a, b, axis=1, step=step)
            want[b] = want[a]
        if len(chosen) == len(PAIRS):  # 0 - 255 - 256 - 511 and 0 - 512: one component
            assert set(np.where(want == 0)[0]) == {0, 255, 256, 511, 512}
        assert np.array_equal(O.single_linkage_roots(pts, 0.5), want), chosen  # the expected roots follow from the pairs
        root, best = single_linkage_roots(torch.from_numpy(pts).to(_dev()), 0.5)
        assert np.array_equal(root.cpu().numpy(), want), chosen
        size = np.bincount(want).max()
        assert best.cpu().tolist() == [int(np.bincount(want).argmax()), int(size)], chosen


def test_rows_with_nan_or_infinity_stay_singletons():
    import post_helpers as P
    from mrcc_amd.utils.output import ClusterUtil, single_linkage_roots
    from oracle import sv_oracle as O

    pts, bad = P.non_finite_scene()
    with np.errstate(invalid="ignore"):
        want = O.single_linkage_roots(pts, 0.5)
    for dtype in (np.float32, np.float64):
        root, best = single_linkage_roots(torch.from_numpy(pts.astype(dtype)).to(_dev()), 0.5)
        got = root.cpu().numpy()
        assert np.array_equal(got, want)
        assert all(got[r] == r and (got == r).sum() == 1 for r in bad)
        assert best.cpu().tolist() == [0, 3]
        assert ClusterUtil(dist=0.5).get_largest_cluster(torch.from_numpy(pts.astype(dtype)).to(_dev())).cpu().tolist() == [0, 5, 9]


@pytest.mark.parametrize("roots", [(3, 1500), (7, 1030)])
def test_argmax_ties_between_roots_held_by_different_threads(roots):
    """n = 3000 > 1024: cluster_argmax_kernel's thread t holds roots t, t + 1024, t + 2048, so the two roots meet in the
    cross-thread reduction; (7, 1030): the lower root sits in the higher thread"""
    import post_helpers as P
    from mrcc_amd.utils.output import ClusterUtil, single_linkage_roots
    from oracle import sv_oracle as O

    n, (lo, hi) = 3000, roots
    assert lo % 1024 != hi % 1024
    for size_lo, size_hi, winner in ((5, 5, lo), (5, 6, hi), (6, 5, lo)):
        pts = P.lattice(n)
        members = {lo: [lo] + list(range(2000, 2000 + size_lo - 1)), hi: [hi] + list(range(2500, 2500 + size_hi - 1))}
        for r, m in members.items():
            for j, b in enumerate(m[1:]):
                P.link(pts, r, b, axis=1, step=0.01 * (j + 1))
        want = O.single_linkage_roots(pts, 0.5)
        assert all((want == r).sum() == len(m) for r, m in members.items()) and len(np.unique(want)) == n - size_lo - size_hi + 2
        root, best = single_linkage_roots(torch.from_numpy(pts).to(_dev()), 0.5)
        assert np.array_equal(root.cpu().numpy(), want)
        assert best.cpu().tolist() == [winner, len(members[winner])]
        got = ClusterUtil(dist=0.5).get_largest_cluster(torch.from_numpy(pts).to(_dev()))
        assert got.cpu().tolist() == sorted(members[winner])


def test_strided_float64_rows_with_and_without_an_index():
    """a float64 [n, 6] table sliced [:, :3] (row stride 6) is read in place; idx holds a repeated row - the duplicates are
    at distance 0 and join"""
    from mrcc_amd.utils.output import single_linkage_roots
    from oracle import sv_oracle as O

    rng = np.random.default_rng(8)
    table = rng.uniform(-1, 1, size=(700, 6))
    table[:, :3] = _scene(rng, n_blob=400, dtype=np.float64)[:700]
    table[:, 3:] = np.nan  # never read
    dev = torch.from_numpy(table).to(_dev())
    view = dev[:, :3]
    assert view.dtype == torch.float64 and view.stride() == (6, 1)
    root, _ = single_linkage_roots(view, 0.06)
    assert np.array_equal(root.cpu().numpy(), O.single_linkage_roots(table[:, :3], 0.06))
    idx = np.sort(rng.choice(700, 400, replace=False))
    lonely = int(np.where(np.bincount(O.single_linkage_roots(table[:, :3], 0.06), minlength=700) == 1)[0][-1])
    idx = np.concatenate([idx[idx != lonely], [lonely, lonely, lonely]])  # a singleton of the scene, three times
    want = O.single_linkage_roots(table[idx, :3], 0.06)
    assert (want[-3:] == len(idx) - 3).all()
    root, best = single_linkage_roots(view, 0.06, idx=torch.from_numpy(idx).to(_dev()))
    assert np.array_equal(root.cpu().numpy(), want)
    u, c = np.unique(want, return_counts=True)
    assert best.cpu().tolist() == [int(u[c.argmax()]), int(c.max())]


def test_select_equal_negative_wide_and_strip_edge_values():
    from mrcc_amd.utils.output import select_equal

    d = _dev()
    rng = np.random.default_rng(9)
    # negative wanted values
    for dt in (np.int32, np.int64):
        v = rng.integers(-3, 4, size=3000).astype(dt)
        for value in (-2, -3, 0):
            assert np.array_equal(select_equal(torch.from_numpy(v).to(d), value).cpu().numpy(), np.where(v == value)[0])
    # int64 values whose low 32 bits are the wanted value
    big = 2**40 + 1
    v = np.array([1, big, 1, 0, big, big, -1, 2**32 - 1, 1 - 2**32, 2**32 + 1, 1], np.int64)
    t = torch.from_numpy(v).to(d)
    for value in (1, big, -1, 2**32 - 1, 2**32 + 1):
        assert np.array_equal(select_equal(t, value).cpu().numpy(), np.where(v == value)[0]), value
    assert select_equal(t, 1).cpu().tolist() == [0, 2, 10] and select_equal(t, big).cpu().tolist() == [1, 4, 5]
    one = torch.tensor([1], dtype=torch.int32, device=d)  # the device-value form against int64 data
    assert select_equal(t, one).cpu().tolist() == [0, 2, 10]
    assert select_equal(t, torch.tensor([-1], dtype=torch.int32, device=d)).cpu().tolist() == [6]
    # hits exactly on the 1024-strip edges and in the last row; every row; no row
    for n, dt in itertools.product((1023, 1024, 1025, 2048, 2049), (np.int32, np.int64)):
        hits = sorted({r for r in (1023, 1024, n - 1) if r < n})
        v = np.zeros(n, dt)
        v[hits] = -5
        t = torch.from_numpy(v).to(d)
        assert select_equal(t, -5).cpu().tolist() == hits
        assert select_equal(t, 0).cpu().tolist() == [r for r in range(n) if r not in hits]
        assert select_equal(t, 4).numel() == 0
        full = torch.full((n,), -5, dtype=t.dtype, device=d)
        assert select_equal(full, -5).cpu().tolist() == list(range(n))
        assert select_equal(full, torch.tensor([-5], dtype=torch.int32, device=d)).cpu().tolist() == list(range(n))
