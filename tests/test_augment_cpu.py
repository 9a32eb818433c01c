"""utils/augmentation.py without a GPU: the float64 restatement of tests/augment_helpers.py against the reference's
recorded results (tests/golden/augmentation.npz, written by tools/make_golden.py augmentation), draw_augmentations, the
host argument checks of sv_elastic_field / sv_augment_points / sv_quantise_points (nothing reaches a device) and
ME.utils.sparse_collate.

Bound against the fixture: both sides are float64 numpy with the same scipy calls under the same np.random seed.  The
worst relative error (max-abs difference over the recorded array's max-abs) measured on the CPU is 0 for every case, so
4 x measured is 0; as for the dense pose criteria (tests/test_pose_loss_cpu.py) the bound is 4 x one rounding of the
format instead (4 * 2^-53 = 4.4e-16: another host's BLAS may order the two three-term products differently), far
below the 1e-9 cap.
"""
import ctypes

import numpy as np
import pytest
import torch

import augment_helpers as H

FIXTURE_BOUND = min(4 * 2.0 ** -53, 1e-9)
FLAGS = dict(elastic=True, noise=True, transform=True, flip=True, gravity=True)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("augmentation")


def test_restatement_matches_the_reference_fixture(fx):
    """Every function alone, augment, and augment_segmentation (scale 200; probability 1.0 and 0.5; metre-sized cloud
    with 3^3 grids and voxel-sized cloud with 9^3 / 5^3 grids), each under the fixture's np.random seed.  Worst
    relative error measured: 0 in all 13 cases (bit-equal); bound 4.4e-16, see FIXTURE_BOUND."""
    worst = 0.0
    cloud_s = fx["cloud_s"]
    for name, seed in zip(fx["single_names"], fx["single_seeds"]):
        np.random.seed(int(seed))
        res, _ = H.seeded_single(str(name), np.array(cloud_s))
        e = H.rel_err(res, fx["single_" + str(name)])
        print(f"{name}: rel {e:.2e}")
        worst = max(worst, e)
        assert res.dtype == np.float64 and e <= FIXTURE_BOUND, (name, e)
    np.random.seed(2000)
    res, d = H.seeded_augment(cloud_s, ((1, 4),), 1.0, **FLAGS)
    e = H.rel_err(res, fx["augment_p1"])
    print(f"augment: rel {e:.2e}")
    worst = max(worst, e)
    assert e <= FIXTURE_BOUND and len(d["elastic"]) == 1
    fired = set()
    for ci, prob, seed in fx["seg_cases"]:
        cloud = fx[("cloud_m", "cloud_v")[int(ci)]]
        np.random.seed(int(seed))
        res, d = H.seeded_augment(cloud, H.stages(200), float(prob), **FLAGS)
        e = H.rel_err(res, fx[f"seg_{int(ci)}_{int(seed)}"])
        shapes = [raw.shape[1:] for raw, _, _ in d["elastic"]]
        print(f"augment_segmentation cloud {int(ci)} p={prob} seed {int(seed)}: rel {e:.2e}, grids {shapes}")
        worst = max(worst, e)
        assert e <= FIXTURE_BOUND, (ci, prob, seed, e)
        if int(ci) == 0:
            assert all(s == (3, 3, 3) for s in shapes)  # scale=200 on metre coordinates
        elif shapes:
            assert max(shapes[0]) > 3
        fired.add(bool(shapes))
    assert fired == {True, False}  # the probability-0.5 cases cover both
    print(f"worst relative error {worst:.2e} (bound {FIXTURE_BOUND:.1e})")


def test_draw_augmentations_grid_shapes(fx):
    """stage 1's grid is abs_max // gran + 3 exactly; stage 2's, sized from the bound abs_max + mag1 * max|raw 1|, is at
    least the grid the reference would size from the cloud stage 1 produced"""
    from mrcc_amd.utils.augmentation import draw_augmentations, segmentation_stages

    clouds = [fx["cloud_v"].astype(np.float64), fx["cloud_m"].astype(np.float64), fx["cloud_s"].astype(np.float64) * 9]
    abs_max = np.stack([np.abs(c).max(0) for c in clouds])
    (g1, m1), (g2, m2) = segmentation_stages(200)
    assert (g1, m1, g2, m2) == (24, 160.0, 80, 640.0) == H.stages(200)[0] + H.stages(200)[1]
    larger = 0
    for seed in range(4):
        draws = draw_augmentations(abs_max, scale=200, probability=1.0, elastic=True, rng=np.random.default_rng(seed))
        assert len(draws) == len(clouds)
        for cloud, am, d in zip(clouds, abs_max, draws):
            s1, s2 = d.elastic
            assert s1.raw.dtype == np.float32 and s1.raw.shape[0] == 3 and (s1.gran, s1.mag) == (g1, m1)
            assert (s2.gran, s2.mag) == (g2, m2)
            assert s1.raw.shape[1:] == tuple(am.astype(np.int32) // g1 + 3) == H.grid_shape(cloud, g1)
            ref2 = H.grid_shape(H.distort_elastic(cloud, g1, m1, s1.raw), g2)
            assert all(a >= b for a, b in zip(s2.raw.shape[1:], ref2)), (s2.raw.shape, ref2)
            larger += s2.raw.shape[1:] != ref2
    print(f"stage-2 grids larger than the reference's: {larger} of 12")


def test_draw_augmentations_probability_and_seed():
    from mrcc_amd.utils.augmentation import draw_augmentations

    abs_max = np.array([[100.0, 50.0, 20.0], [0.5, 0.5, 0.5], [300.0, 10.0, 10.0]])
    none = draw_augmentations(abs_max, probability=0.0, rng=np.random.default_rng(0), **FLAGS)
    assert all(not any(d.fired().values()) for d in none)
    every = draw_augmentations(abs_max, probability=1.0, rng=np.random.default_rng(0), **FLAGS)
    assert all(all(d.fired().values()) for d in every)
    off = draw_augmentations(abs_max, probability=1.0, rng=np.random.default_rng(0))  # no flag set
    assert all(not any(d.fired().values()) for d in off)
    for d in every:
        tr, rot = d.transform
        assert 0 <= tr < 0.04 and np.abs(rot @ rot.T - np.eye(3)).max() < 1e-12 and np.linalg.det(rot) > 0
        assert d.flip in (1, -1) and 0 <= d.gravity < 2 * np.pi and d.normals is None and len(d.elastic) == 2
    again = draw_augmentations(abs_max, probability=1.0, rng=np.random.default_rng(0), **FLAGS)
    other = draw_augmentations(abs_max, probability=1.0, rng=np.random.default_rng(1), **FLAGS)
    for a, b, c in zip(every, again, other):
        assert all(np.array_equal(x.raw, y.raw) for x, y in zip(a.elastic, b.elastic))
        assert a.transform[0] == b.transform[0] and np.array_equal(a.transform[1], b.transform[1])
        assert (a.flip, a.gravity) == (b.flip, b.gravity)
        assert a.gravity != c.gravity and not np.array_equal(a.elastic[0].raw, c.elastic[0].raw)
    half = draw_augmentations(np.tile(abs_max, (40, 1)), probability=0.5, rng=np.random.default_rng(2), **FLAGS)
    for k in FLAGS:
        n = sum(d.fired()[k] for d in half)
        assert 30 <= n <= 90, (k, n)  # 120 draws at 0.5: 5.5 sigma either side


def test_entry_point_argument_checks_without_gpu():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    p = ctypes.create_string_buffer(64)  # stands in for a non-null pointer: every call here fails its checks first
    err = lambda: lib.sv_last_error()  # noqa: E731
    dims = (ctypes.c_int32 * 6)(3, 4, 5, 40, 40, 40)
    floats = 3 * (3 * 4 * 5 + 40 * 40 * 40)
    need = lib.sv_elastic_field_workspace_bytes(dims, 2)
    assert need >= floats * 4

    def field(raw=p, dims=dims, F=2, ws=p, ws_bytes=need, out=p):
        return lib.sv_elastic_field(raw, dims, F, ws, ws_bytes, out, None)

    for kw in ({"raw": None}, {"dims": None}, {"ws": None}, {"out": None}):
        assert field(**kw) == -1 and b"null pointer" in err(), kw
    for F in (0, -1, 2 * 1024 + 1):
        assert field(F=F) == -1 and b"1 to 2048 fields" in err(), F
    for bad in ((2, 4, 5), (3, 0, 5), (3, 4, -1), (3, 4, 1025)):
        d = (ctypes.c_int32 * 6)(3, 3, 3, *bad)
        assert field(dims=d) == -1 and b"grid dimension" in err(), bad
        assert lib.sv_elastic_field_workspace_bytes(d, 2) == 0
    for ws_bytes in (0, 256, floats * 4 - 1):
        assert field(ws_bytes=ws_bytes) == -2 and b"workspace too small" in err(), ws_bytes

    N, B = 1000, 3
    need = lib.sv_augment_points_workspace_bytes(N, B)
    used = 256 + ((N + 255) // 256 + B) * 6 * 8
    assert need >= used and lib.sv_augment_points_workspace_bytes(4 * N, B) > need

    def augment(points=p, f64=0, offsets=p, N=N, B=B, table=p, fields=None, fields_len=0, noise=None, ws=p, ws_bytes=need,
                out=p, stats=p):
        return lib.sv_augment_points(points, f64, offsets, N, B, table, fields, fields_len, noise, ws, ws_bytes, out,
                                     stats, None)

    for kw in ({"points": None}, {"offsets": None}, {"table": None}, {"ws": None}, {"out": None}, {"stats": None}):
        assert augment(**kw) == -1 and b"null pointer" in err(), kw
    for b in (0, -1, 1025):
        assert augment(B=b) == -1 and b"1 to 1024 frames" in err(), b
    for n in (-1, 1 << 29):
        assert augment(N=n) == -1 and b"2^29 points" in err(), n
    assert augment(fields_len=10) == -1 and b"fields_len without fields" in err()
    assert augment(fields=p, fields_len=-1) == -1 and b"fields_len without fields" in err()
    for ws_bytes in (0, 256, used - 1):
        assert augment(ws_bytes=ws_bytes) == -2 and b"workspace too small" in err(), ws_bytes

    def quantise(points=p, offsets=p, N=N, B=B, stats=p, origin=1, size=0.005, coords=p, shifted=None, shift=None):
        return lib.sv_quantise_points(points, offsets, N, B, stats, origin, ctypes.c_double(size), coords, shifted, shift,
                                      None)

    for kw in ({"points": None}, {"offsets": None}, {"coords": None}, {"stats": None}, {"stats": None, "origin": 2},
               {"stats": None, "origin": 0, "shift": p}):
        assert quantise(**kw) == -1 and b"null pointer" in err(), kw
    for b in (0, -1, 1025):
        assert quantise(B=b) == -1 and b"1 to 1024 frames" in err(), b
    for origin in (-1, 3):
        assert quantise(origin=origin) == -1 and b"bad origin mode" in err(), origin
    for size in (0.0, -1.0, float("inf"), float("nan")):
        assert quantise(size=size) == -1 and b"quantization_size" in err(), size


def test_sparse_collate_against_batched_coordinates():
    from mrcc_amd import MinkowskiEngine as ME

    rng = np.random.default_rng(3)
    lens = (5, 1, 0, 17)
    coords = [rng.integers(-50, 50, size=(n, 3)).astype(np.int32) for n in lens]
    feats = [rng.normal(size=(n, 4)).astype(np.float32) for n in lens]
    labels = [rng.integers(0, 5, size=n).astype(np.int64) for n in lens]
    c, f, l = ME.utils.sparse_collate(coords, feats, labels)
    assert c.dtype == torch.int32 and torch.equal(c, ME.utils.batched_coordinates(coords))
    assert np.array_equal(c[:, 0].numpy(), np.repeat(np.arange(4), lens))
    assert np.array_equal(f.numpy(), np.concatenate(feats)) and f.dtype == torch.float32
    assert np.array_equal(l.numpy(), np.concatenate(labels)) and l.dtype == torch.int64
    # the reference's collate_sparse asks for float coordinates (data/alivev2.py:391-396); torch tensors are taken too
    c32, f2 = ME.utils.sparse_collate([torch.from_numpy(x) for x in coords], [torch.from_numpy(x) for x in feats],
                                      dtype=torch.float32)
    assert c32.dtype == torch.float32 and torch.equal(c32, ME.utils.batched_coordinates(coords, dtype=torch.float32))
    assert torch.equal(f2, f)
    with pytest.raises(ValueError):
        ME.utils.sparse_collate(coords, feats[:3], labels)
    with pytest.raises(ValueError):
        ME.utils.sparse_collate(coords, feats, [l[:-1] for l in labels[:1]] + labels[1:])


def test_quantise_restatement_against_the_per_frame_path():
    """H.quantise_np (what tests/test_gpu_augment_edges.py holds sv_quantise_points to) against the path it restates,
    frame by frame: centring as utils/preprocess.py (p - (max + min) / 2, p - min), then the float64 floor(p / size) of
    ME.utils.sparse_quantize in torch; and against hand-written values at the int32 edges.  Integer results: equal."""
    rng = np.random.default_rng(5)
    lens = (0, 7, 0, 0, 300, 1, 0)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    pts = rng.uniform(-150, 150, (sum(lens), 3))
    frames = [pts[a:b] for a, b in zip(offsets[:-1], offsets[1:])]
    stats = np.stack([np.concatenate([f.min(0), f.max(0)]) if len(f) else np.array([np.inf] * 3 + [-np.inf] * 3)
                      for f in frames])
    size = 40.0
    for origin in (H.ORIGIN_NONE, H.ORIGIN_CENTER, H.ORIGIN_BASE):
        coords, shifted, shift = H.quantise_np(pts, offsets, stats, origin, size)
        assert coords.dtype == np.int32 and shifted.dtype == np.float32 and shift.shape == (len(lens), 3)
        for b, f in enumerate(frames):
            if not len(f):
                want = {H.ORIGIN_NONE: 0.0, H.ORIGIN_BASE: np.inf}.get(origin)
                assert np.isnan(shift[b]).all() if want is None else (shift[b] == want).all()
                continue
            o = {H.ORIGIN_NONE: np.zeros(3), H.ORIGIN_CENTER: (f.max(0) + f.min(0)) / 2, H.ORIGIN_BASE: f.min(0)}[origin]
            s = f - o
            want = torch.floor(torch.from_numpy(s).to(torch.float64) / size).to(torch.int32).numpy()
            rows = slice(offsets[b], offsets[b + 1])
            assert np.array_equal(shift[b], o) and (coords[rows, 0] == b).all()
            assert np.array_equal(coords[rows, 1:], want) and np.array_equal(shifted[rows], s.astype(np.float32))
    # the int32 edges, size 2^-3: the largest and smallest quotients are kept, one further is out, as are inf, NaN, 1e300
    size, top = 0.125, 2.0 ** 31
    col = np.array([-0.5, -1e-300, -0.0, 0.0, 0.125, -0.125, (top - 1) * size, -top * size, top * size, (-top - 1) * size,
                    np.inf, -np.inf, np.nan, 1e300])
    want = [-4, -1, 0, 0, 1, -1, 2 ** 31 - 1, -2 ** 31] + [H.INT32_MIN] * 6
    p = np.stack([col, np.zeros_like(col), col[::-1]], axis=1)
    coords, shifted, shift = H.quantise_np(p, [0, len(p)], np.zeros((1, 6)), H.ORIGIN_NONE, size)
    assert coords[:, 1].tolist() == want and coords[:, 3].tolist() == want[::-1] and not coords[:, [0, 2]].any()
    with np.errstate(over="ignore"):
        assert np.array_equal(shifted, p.astype(np.float32), equal_nan=True) and not shift.any()
    # a NaN in one frame's stats under CENTER: that frame's column only
    st = np.array([[0, 0, 0, 2, 2, 2], [0, np.nan, 0, 2, 2, 2]], dtype=np.float64)
    coords, _, shift = H.quantise_np(np.ones((4, 3)), [0, 2, 4], st, H.ORIGIN_CENTER, 1.0)
    assert coords.tolist() == [[0, 0, 0, 0]] * 2 + [[1, 0, H.INT32_MIN, 0]] * 2 and np.isnan(shift[1, 1])


def test_frames_without_rows_concatenate():
    """the batch builder's per-frame feature arrays as [n_b, C]: a frame without rows, whatever its own shape, takes the
    width of the frames that have rows (reshape(0, -1) is an error in numpy)"""
    from mrcc_amd.utils.augmentation import _frame_rows

    feats = [np.ones((5, 3), np.float64), np.zeros((0, 3), np.float32), np.zeros(0), np.arange(6.0).reshape(2, 3)]
    rows = _frame_rows(feats, np.float32)
    assert [r.shape for r in rows] == [(5, 3), (0, 3), (0, 3), (2, 3)] and all(r.dtype == np.float32 for r in rows)
    assert np.concatenate(rows).shape == (7, 3) and np.array_equal(rows[3], feats[3])
    assert [r.shape for r in _frame_rows([np.zeros(4), np.zeros(0)])] == [(4, 1), (0, 1)]
    assert [r.shape for r in _frame_rows([np.zeros((0, 3))])] == [(0, 1)] and _frame_rows([np.zeros(2)])[0].dtype == np.float64


def test_no_cpu_fallback():
    from mrcc_amd._lib import SvHipError
    from mrcc_amd.utils import augmentation as A

    with pytest.raises(SvHipError, match="no CPU fallback"):
        A.flip_random(torch.zeros(4, 3), sign=1)
    with pytest.raises(SvHipError, match="no CPU fallback"):
        A.augment_quantize_batch([np.zeros((4, 3))], [np.zeros((4, 3))], [np.zeros(4)], quantization_size=0.01,
                                 device="cpu")
    with pytest.raises(ValueError):
        A.augment_quantize_batch([np.zeros((4, 3))], [np.zeros((3, 3))], [np.zeros(4)], quantization_size=0.01)
