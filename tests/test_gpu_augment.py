"""sv_elastic_field, sv_augment_points, sv_quantise_points and utils/augmentation.py on the GPU against the float64
numpy / scipy restatement of tests/augment_helpers.py (which tests/test_augment_cpu.py pins to the reference's recorded
results).

Bounds:
  field    4 * 2^-24 * max|raw noise|: six averaging passes, each rounded once to float32; an average of values bounded
           by max|raw| does not amplify an earlier pass's error
  elastic  1e-9 * (max|x| + mag * max|field|): float64 against float64 in the same operation order, the order of the
           project's golden dense solves; with two stages chained, the smaller of the two stages' terms
  noise, transform, flip, gravity   1e-12 * max|x|: three-term float64 products and sums
  batch builder   exact: coordinates, labels and offsets equal, features bit-equal
"""
import numpy as np
import pytest
import torch
from scipy.stats import special_ortho_group

import augment_helpers as H

pytestmark = pytest.mark.gpu


def _A():
    from mrcc_amd.utils import augmentation

    return augmentation


# ---------------------------------------------------------------------------------------------------------------------
# sv_elastic_field
# ---------------------------------------------------------------------------------------------------------------------
FIELD_CASES = {
    "3x3x3": [(3, 3, 3)],  # every cell at an edge in every axis
    "3x4x5": [(3, 4, 5)],
    "17x3x9": [(17, 3, 9)],
    "40x40x40": [(40, 40, 40)],
    "two_sizes": [(5, 9, 4), (12, 3, 7)],
    "34_fields": [(3, 3, 3)] * 33 + [(4, 3, 5)],  # more fields than one launch's table holds
}


@pytest.mark.parametrize("case", list(FIELD_CASES))
def test_elastic_field_against_scipy(gpu, case):
    A = _A()
    shapes = FIELD_CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    raws = [rng.standard_normal((3,) + s).astype(np.float32) for s in shapes]
    flat = np.concatenate([r.reshape(-1) for r in raws])
    out = A.elastic_fields(flat, np.array(shapes, dtype=np.int32), gpu).cpu().numpy()
    assert out.shape == flat.shape
    first = 0
    for raw in raws:
        ref = np.stack(H.blur_field(raw))
        got = out[first: first + raw.size].reshape(raw.shape)
        first += raw.size
        err, bound = float(np.abs(got - ref).max()), 4 * 2.0 ** -24 * float(np.abs(raw).max())
        print(f"{case} {raw.shape[1:]}: max abs err {err:.2e} (bound {bound:.2e}), bit-equal {np.mean(got == ref):.4f}")
        assert err <= bound


# ---------------------------------------------------------------------------------------------------------------------
# elastic stage on points
# ---------------------------------------------------------------------------------------------------------------------
def _elastic_points(rng, n, shape, gran):
    """points inside and around the grid; as n allows: on nodes, on both outermost nodes, just outside either end,
    one row with a NaN.  Returns (x, indices just outside, index of the NaN row or None)."""
    ext = np.array([(b - 1) * gran for b in shape], dtype=np.float64)
    x = rng.uniform(-1.05, 1.05, (n, 3)) * ext
    ax = H.axes_of(shape, gran)
    if n == 1:
        x[0] = rng.uniform(-0.9, 0.9, 3) * ext
    outside, nan_row = [], None
    if n >= 63:
        x[1:9] = np.stack([rng.choice(a, 8) for a in ax], axis=1)  # exactly on grid nodes
        x[9], x[10] = ext, -ext  # both outermost nodes: inside (the upper edge is inclusive)
        x[11, 0], x[12, 1], x[13, 2] = ext[0], -ext[1], ext[2]
        x[14] = np.nextafter(ext, np.inf)
        x[15] = np.nextafter(-ext, -np.inf)
        x[16] = rng.uniform(-0.5, 0.5, 3) * ext
        x[16, 2] = np.nextafter(ext[2], np.inf)
        x[17] = rng.uniform(-0.5, 0.5, 3) * ext
        x[17, 0] = np.nextafter(-ext[0], -np.inf)
        outside = [14, 15, 16, 17]
        nan_row = 20
        x[nan_row, 1] = np.nan
    return x, outside, nan_row


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_elastic_points_against_restatement(gpu, n):
    A = _A()
    rng = np.random.default_rng(100 + n)
    shape, gran, mag = (5, 3, 7), 24, 160.0
    raw = rng.standard_normal((3,) + shape).astype(np.float32)
    x, outside, nan_row = _elastic_points(rng, n, shape, gran)
    ref = H.distort_elastic(x, gran, mag, raw)
    got = A.distort_elastic(x, gran, mag, noise=raw)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == x.shape
    ok = np.ones(n, dtype=bool)
    if nan_row is not None:
        ok[nan_row] = False
        assert np.isnan(got[nan_row]).all() and np.isnan(ref[nan_row]).all()
    assert not np.isnan(got[ok]).any()
    field_max = float(np.abs(np.stack(H.blur_field(raw))).max())
    bound = 1e-9 * (float(np.abs(x[ok]).max()) + mag * field_max)
    err = float(np.abs(got[ok] - ref[ok]).max())
    print(f"n={n}: max abs err {err:.2e} (bound {bound:.2e}), bit-equal {np.mean(got[ok] == ref[ok]):.4f}")
    assert err <= bound
    for i in outside:  # just outside the grid on at least one axis: exactly zero displacement
        assert np.array_equal(got[i], x[i]) and np.array_equal(ref[i], x[i])
    if n >= 63:
        assert np.abs(got[9] - x[9]).max() > 0 and np.abs(got[10] - x[10]).max() > 0  # the outermost nodes are inside
    # a CUDA tensor in gives a float64 CUDA tensor out, with the same bits
    t = A.distort_elastic(torch.from_numpy(x).to(gpu), gran, mag, noise=raw)
    assert t.is_cuda and t.dtype == torch.float64
    assert np.array_equal(t.cpu().numpy().view(np.int64), got.view(np.int64))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_two_elastic_stages_chained(gpu, dtype):
    """the second stage is evaluated at the positions the first produced; float32 and float64 input"""
    A = _A()
    rng = np.random.default_rng(7)
    n = 1000
    x = rng.uniform(-150, 150, (n, 3)).astype(dtype)
    x[5, 0] = np.nan
    d = H.no_draws()
    d["elastic"] = [(rng.standard_normal((3, 9, 9, 9)).astype(np.float32), 24, 160.0),
                    (rng.standard_normal((3, 6, 7, 5)).astype(np.float32), 80, 640.0)]
    ref = H.apply_draws(x, d)
    got = A.augment_segmentation(x, draws=H.to_package_draws(d))
    ok = np.arange(n) != 5
    assert np.isnan(got[5]).all() and not np.isnan(got[ok]).any()
    terms = [mag * float(np.abs(np.stack(H.blur_field(raw))).max()) for raw, _, mag in d["elastic"]]
    bound = 1e-9 * (float(np.abs(x[ok]).max()) + min(terms))
    err = float(np.abs(got[ok] - ref[ok]).max())
    one_stage = H.distort_elastic(np.asarray(x, dtype=np.float64), *d["elastic"][0][1:], d["elastic"][0][0])
    print(f"{np.dtype(dtype).name}: max abs err {err:.2e} (bound {bound:.2e}); second stage moves points by up to "
          f"{np.abs(ref[ok] - one_stage[ok]).max():.1f}")
    assert err <= bound and np.abs(ref[ok] - one_stage[ok]).max() > 1


# ---------------------------------------------------------------------------------------------------------------------
# noise, transform, flip, gravity
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cloud():
    return np.random.default_rng(11).uniform(-1.5, 1.5, (1000, 3))


def _close(got, ref, x, what):
    bound = 1e-12 * float(np.abs(x).max())
    err = float(np.abs(got - ref).max())
    print(f"{what}: max abs err {err:.2e} (bound {bound:.2e}), bit-equal {np.mean(got == ref):.4f}")
    assert got.dtype == np.float64 and got.shape == ref.shape and err <= bound


def test_add_noise(gpu, cloud):
    A = _A()
    normals = np.random.default_rng(12).standard_normal(cloud.shape)
    normals[0] = [4.0, -4.0, 10.0]
    clipped = np.abs(H.SIGMA * normals) > H.CLIP
    assert 3 <= clipped.sum() < clipped.size // 10  # the clip is active on some draws
    got = A.add_noise(cloud, normals=normals)
    _close(got, H.add_noise(cloud, normals), cloud, "add_noise")
    assert np.array_equal(got[0], cloud[0] + np.array([H.CLIP, -H.CLIP, H.CLIP]))
    got = A.add_noise(cloud, 0.01, 0.02, normals=normals)
    _close(got, H.add_noise(cloud, normals, 0.01, 0.02), cloud, "add_noise(sigma=0.01, clip=0.02)")


def test_transform_random(gpu, cloud):
    A = _A()
    rot = special_ortho_group.rvs(3, random_state=np.random.default_rng(13))
    got = A.transform_random(cloud, tr=0.0317, rot=rot)
    ref = H.transform_random(cloud, 0.0317, rot)
    _close(got, ref, cloud, "transform_random")
    assert np.abs(got - cloud).max() > 1e-3  # it moved: a translation by tr along rot's first row


@pytest.mark.parametrize("sign", [1, -1])
def test_flip_random(gpu, cloud, sign):
    A = _A()
    got = A.flip_random(cloud, sign=sign)
    _close(got, H.flip_random(cloud, sign), cloud, f"flip_random({sign})")
    assert np.array_equal(got, cloud * np.array([sign, 1, 1]))


def test_rotate_along_gravity(gpu, cloud):
    A = _A()
    got = A.rotate_along_gravity(cloud, angle=2.2)
    _close(got, H.rotate_along_gravity(cloud, 2.2), cloud, "rotate_along_gravity")
    assert np.array_equal(got[:, 1], cloud[:, 1]) and np.abs(got[:, 0] - cloud[:, 0]).max() > 0.1


def test_seeded_like_the_reference(gpu, golden):
    """Without explicit draws the functions draw from np.random with the reference's calls in the reference's order: under
    the fixture's seeds they reproduce the reference's recorded results (float64 against float64: 1e-9 of the recorded
    array's max-abs, the order of the project's golden dense solves)."""
    A = _A()
    fx = golden("augmentation")
    flags = dict(elastic=True, noise=True, transform=True, flip=True, gravity=True)
    calls = {"distort_elastic_1_4": lambda x: A.distort_elastic(x, 1, 4),
             "distort_elastic_24_160": lambda x: A.distort_elastic(x, 24, 160.0), "add_noise": A.add_noise,
             "transform_random": A.transform_random, "flip_random": A.flip_random,
             "rotate_along_gravity": A.rotate_along_gravity}
    for name, seed in zip(fx["single_names"], fx["single_seeds"]):
        np.random.seed(int(seed))
        e = H.rel_err(calls[str(name)](np.array(fx["cloud_s"])), fx["single_" + str(name)])
        print(f"{name}: rel {e:.2e}")
        assert e <= 1e-9, name
    np.random.seed(2000)
    e = H.rel_err(A.augment(fx["cloud_s"], probability=1.0, **flags), fx["augment_p1"])
    print(f"augment: rel {e:.2e}")
    assert e <= 1e-9
    for ci, prob, seed in fx["seg_cases"]:
        np.random.seed(int(seed))
        got = A.augment_segmentation(fx[("cloud_m", "cloud_v")[int(ci)]], scale=200, probability=float(prob), **flags)
        e = H.rel_err(got, fx[f"seg_{int(ci)}_{int(seed)}"])
        print(f"augment_segmentation cloud {int(ci)} p={prob} seed {int(seed)}: rel {e:.2e}")
        assert got.dtype == np.float64 and e <= 1e-9, (ci, prob, seed)


# ---------------------------------------------------------------------------------------------------------------------
# the batch builder
# ---------------------------------------------------------------------------------------------------------------------
LENS = (1, 257, 1000)
QSIZE = 40.0
IGNORE = -100


def _origin(p, mode):
    if mode == "center":
        return (p.max(axis=0) + p.min(axis=0)) / 2
    return p.min(axis=0)


def _batch_inputs(mode):
    """Three frames (nothing fires / elastic + flip / everything fires), their draws, and the restated, centred points.
    A seed is skipped when a restated coordinate lies within 1e-6 cells of a cell border, so that a last-bit difference
    cannot move a point to another voxel.  Coordinates that are exactly 0 are exempt: they are the frame's own minimum
    under base_at_origin (and the lone point of frame 0 under center_at_origin), p - p on either side, whatever p's last
    bit.  No point is left out of the comparison."""
    for seed in range(20, 40):
        rng = np.random.default_rng(seed)
        pts = [rng.uniform(-150, 150, (n, 3)).astype(np.float32) for n in LENS]
        pts[2][7] = pts[2][3]  # two points of one voxel ...
        feats = [rng.normal(size=(n, 3)).astype(np.float32) for n in LENS]
        labels = [rng.integers(0, 4, size=n).astype(np.int64) for n in LENS]
        labels[2][3], labels[2][7] = 1, 2  # ... with different labels
        np.random.seed(seed)
        _, d1 = H.seeded_augment(pts[1], H.stages(200), 1.0, True, False, False, True, False)
        _, d2 = H.seeded_augment(pts[2], H.stages(200), 1.0, True, True, True, True, True)
        draws = [H.no_draws(), d1, d2]
        assert len(d1["elastic"]) == 2 and d1["flip"] is not None and d1["normals"] is None
        assert len(d2["elastic"]) == 2 and all(d2[k] is not None for k in ("normals", "transform", "flip", "gravity"))
        shifted = []
        for p, d in zip(pts, draws):
            r = H.apply_draws(p, d)
            shifted.append(r - _origin(r, mode))
        cells = np.concatenate(shifted) / QSIZE
        near = (np.abs(cells - np.rint(cells)) < 1e-6) & (np.concatenate(shifted) != 0.0)
        if not near.any():
            return pts, feats, labels, draws, shifted
    raise AssertionError("no seed without a point near a cell border")


@pytest.fixture(scope="module", params=["center", "base"])
def batch(gpu, request):
    from mrcc_amd import MinkowskiEngine as ME

    A = _A()
    mode = request.param
    pts, feats, labels, draws, shifted = _batch_inputs(mode)
    # the per-frame path: restatement, then the existing sparse_quantize per frame, then batched_coordinates
    ref_c, ref_f, ref_l = [], [], []
    for s, f, l in zip(shifted, feats, labels):
        c, uf, ul = ME.utils.sparse_quantize(coordinates=s, features=f, labels=l, quantization_size=QSIZE,
                                             ignore_label=IGNORE)
        ref_c.append(c), ref_f.append(uf), ref_l.append(ul)
    kw = dict(draws=[H.to_package_draws(d) for d in draws], quantization_size=QSIZE, ignore_label=IGNORE,
              center_at_origin=mode == "center", base_at_origin=mode == "base", device=gpu)
    out = A.augment_quantize_batch(pts, feats, labels, return_extras=True, **kw)
    again = A.augment_quantize_batch(pts, feats, labels, **kw)
    return {"mode": mode, "ref": (ME.utils.batched_coordinates(ref_c), np.concatenate(ref_f), np.concatenate(ref_l)),
            "ref_counts": [len(c) for c in ref_c], "shifted": shifted, "out": out, "again": again}


def test_batch_builder_against_per_frame_path(batch):
    ref_c, ref_f, ref_l = batch["ref"]
    coords, feats, labels, offsets, extras = batch["out"]
    assert coords.is_cuda and coords.dtype == torch.int32 and feats.dtype == torch.float32
    assert labels.dtype == torch.int64 and offsets.dtype == torch.int32
    V = ref_c.shape[0]
    print(f"{batch['mode']}: {sum(LENS)} points -> {V} voxels {batch['ref_counts']}, "
          f"{int((ref_l == IGNORE).sum())} voxels with conflicting labels")
    assert 1 < batch["ref_counts"][2] < LENS[2] and (ref_l == IGNORE).any() and (ref_l != IGNORE).any()
    assert torch.equal(coords.cpu(), ref_c)
    assert np.array_equal(feats.cpu().numpy().view(np.int32), ref_f.view(np.int32))
    assert np.array_equal(labels.cpu().numpy(), ref_l)
    assert offsets.cpu().tolist() == np.concatenate([[0], np.cumsum(batch["ref_counts"])]).tolist()
    # the extras: what centring subtracted and the continuous coordinates, against the restatement
    shifted = np.concatenate(batch["shifted"])
    got = extras["points"].cpu().numpy()
    assert got.dtype == np.float32 and np.abs(got - shifted).max() <= 2.0 ** -23 * np.abs(shifted).max()  # one float32 ulp
    assert extras["origin_offset"].shape == (3, 3) and extras["inverse"].shape == (sum(LENS),)
    assert torch.equal(coords[extras["inverse"]][:, 1:].cpu(), torch.from_numpy(np.floor(shifted / QSIZE).astype(np.int32)))


def test_batch_builder_is_deterministic(batch):
    for a, b in zip(batch["out"][:4], batch["again"]):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_batch_builder_feeds_a_sparse_tensor(batch):
    from mrcc_amd import MinkowskiEngine as ME

    coords, feats = batch["out"][:2]
    st = ME.SparseTensor(feats, coordinates=coords)
    assert torch.equal(st.C, coords) and torch.equal(st.F, feats)


def test_batch_builder_draws_on_its_own(gpu):
    """without draws the builder makes them (numpy rng on the host, per-point normals from torch.randn on the device):
    the same seeds give the same batch, and a frame's noise stays inside the clip"""
    A = _A()
    rng = np.random.default_rng(50)
    pts = [rng.uniform(-0.8, 0.8, (n, 3)).astype(np.float32) for n in (300, 64)]
    feats = [p.copy() for p in pts]
    labels = [np.zeros(len(p), dtype=np.int64) for p in pts]

    def run(seed, **kw):
        g = torch.Generator(device=gpu)
        g.manual_seed(seed)
        return A.augment_quantize_batch(pts, feats, labels, scale=200, quantization_size=1 / 200, probability=1.0,
                                        rng=np.random.default_rng(seed), generator=g, device=gpu, return_extras=True, **kw)

    a, b, c = run(1, noise=True), run(1, noise=True), run(2, noise=True)
    plain = run(1)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    assert torch.equal(a[4]["points"], b[4]["points"]) and not torch.equal(a[4]["points"], c[4]["points"])
    moved = (a[4]["points"] - plain[4]["points"]).abs().cpu().numpy()
    assert np.array_equal(plain[4]["points"].cpu().numpy(), np.concatenate(pts))
    assert 0 < moved.max() <= H.CLIP + 1e-6 and np.median(moved) > 1e-4
    every = run(3, elastic=True, noise=True, transform=True, flip=True, gravity=True, center_at_origin=True)
    assert every[3].tolist()[0] == 0 and every[3].tolist()[-1] == every[0].shape[0] and every[0].shape[0] > 2
