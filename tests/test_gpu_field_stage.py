"""sv_field_stage - Sinusoidal -> BN -> ReLU -> Linear -> BN -> ReLU -> per-voxel mean in one launch - on both stages of the
ResFieldNets (Cg = 0, Cf = 3, C = 32; Cg = 32, Cf = 3, C = 64) and the cloud of field_helpers.stage_cloud: single-point
voxels, a voxel of 1000 points, a segment across every multiple of the tile size up to 1024.

Accuracy: relative max-abs error against the float64 restatement <= max(1e-4, 8 * d32), d32 = the same stage evaluated by
torch in float32 on the CPU against float64 (the rule of tests/test_gpu_resnet_dense.py).  Order: a voxel's row is one
sequential sum over its points in ascending index, so it has the same bits whatever else is in the call - frames alone,
subsets of whole voxels, permutations that keep each voxel's order."""
import numpy as np
import pytest
import torch

import field_helpers as FH

pytestmark = pytest.mark.gpu

STAGES = {"stage1": (0, 3, 32), "stage2": (32, 3, 64)}
_cache = {}


def _case(gpu, name):
    """inputs, the kernel's result and the float64 / float32 references of a stage: computed once, never changed"""
    if name not in _cache:
        cg, cf, c = STAGES[name]
        pts = FH.stage_cloud()
        inverse, V = FH.voxelize_ref(pts)
        g = torch.Generator().manual_seed(7)
        F = torch.randn(len(pts), cf, generator=g)
        G = torch.randn(V, cg, generator=g) if cg else None
        p = FH.stage_params(cg + cf, c, seed=8)
        got, inv = FH.run_stage(gpu, F, pts, p, G)
        assert torch.equal(inv, inverse), "the reference voxelisation is not the library's"
        want = FH.stage_ref(F, p, inverse, V, torch.float64, G)
        w32 = FH.stage_ref(F, p, inverse, V, torch.float32, G).double()
        _cache[name] = dict(pts=pts, inverse=inverse, V=V, F=F, G=G, p=p, got=got, want=want, w32=w32)
    return _cache[name]


@pytest.mark.parametrize("name", list(STAGES))
def test_stage_matches_float64(gpu, name):
    k = _case(gpu, name)
    scale = k["want"].abs().max()
    d32 = float((k["w32"] - k["want"]).abs().max() / scale)
    err = float((k["got"].double() - k["want"]).abs().max() / scale)
    print(f"sv_field_stage {name}: d32 = {d32:.3e}, error = {err:.3e}, bound = {max(1e-4, 8 * d32):.3e}")
    assert k["got"].shape == (k["V"], STAGES[name][2]) and torch.isfinite(k["got"]).all()
    assert err <= max(1e-4, 8 * d32)
    again, _ = FH.run_stage(gpu, k["F"], k["pts"], k["p"], k["G"])
    assert torch.equal(FH.bits(again), FH.bits(k["got"])), "two calls differ"


@pytest.mark.parametrize("name", list(STAGES))
def test_without_linear_bias(gpu, name):
    k = _case(gpu, name)
    p = dict(k["p"], lin_bias=None)
    got, _ = FH.run_stage(gpu, k["F"], k["pts"], p, k["G"])
    want = FH.stage_ref(k["F"], p, k["inverse"], k["V"], torch.float64, k["G"])
    d32 = float((FH.stage_ref(k["F"], p, k["inverse"], k["V"], torch.float32, k["G"]).double() - want).abs().max() / want.abs().max())
    assert float((got.double() - want).abs().max() / want.abs().max()) <= max(1e-4, 8 * d32)


def _run_points(gpu, k, idx, G):
    """the stage on the points idx (ascending or permuted) with the voxel features G of their voxels, in canonical order"""
    return FH.run_stage(gpu, k["F"][idx], k["pts"][idx.numpy()], k["p"], G)[0]


@pytest.mark.parametrize("name", list(STAGES))
def test_each_frame_alone_gives_the_bits_of_the_batched_call(gpu, name):
    k = _case(gpu, name)
    batch = torch.from_numpy(k["pts"][:, 0].astype(np.int64))
    for b in (0, 1):
        idx = torch.nonzero(batch == b).reshape(-1)
        rows = torch.unique(k["inverse"][idx])
        got = _run_points(gpu, k, idx, k["G"][rows] if k["G"] is not None else None)
        assert torch.equal(FH.bits(got), FH.bits(k["got"][rows])), f"frame {b}"


@pytest.mark.parametrize("name", list(STAGES))
def test_any_subset_of_whole_voxels_gives_the_bits_of_its_rows(gpu, name):
    k = _case(gpu, name)
    rng = np.random.default_rng(5)
    big = int(torch.bincount(k["inverse"]).argmax())
    for trial, frac in enumerate((0.5, 0.1, 0.9)):
        keep_v = torch.from_numpy(rng.random(k["V"]) < frac)
        keep_v[big] = trial != 1  # with and without the 1000-point voxel
        idx = torch.nonzero(keep_v[k["inverse"]]).reshape(-1)
        rows = torch.nonzero(keep_v).reshape(-1)
        got = _run_points(gpu, k, idx, k["G"][rows] if k["G"] is not None else None)
        assert torch.equal(FH.bits(got), FH.bits(k["got"][rows])), f"subset {trial}"


@pytest.mark.parametrize("name", list(STAGES))
def test_a_permutation_that_keeps_each_voxels_order_gives_the_same_bits(gpu, name):
    k = _case(gpu, name)
    rng = np.random.default_rng(6)
    inv = k["inverse"].numpy()
    slots = rng.permutation(len(inv))  # point i would go to slot slots[i]; then each voxel's slots are handed out in order
    new_slot = np.empty(len(inv), np.int64)
    for v in range(k["V"]):
        members = np.nonzero(inv == v)[0]
        new_slot[members] = np.sort(slots[members])
    perm = torch.from_numpy(np.argsort(new_slot))  # the point at each slot
    assert not torch.equal(perm, torch.arange(len(inv)))
    got = _run_points(gpu, k, perm, k["G"])
    assert torch.equal(FH.bits(got), FH.bits(k["got"]))


@pytest.mark.parametrize("name", list(STAGES))
def test_a_nan_point_makes_exactly_its_voxels_row_nan(gpu, name):
    k = _case(gpu, name)
    counts = torch.bincount(k["inverse"])
    big = int(counts.argmax())
    for point in (int(torch.nonzero(k["inverse"] == big)[500]), int(torch.nonzero(counts[k["inverse"]] == 1)[3])):
        F = k["F"].clone()
        F[point, 1] = float("nan")
        got, _ = FH.run_stage(gpu, F, k["pts"], k["p"], k["G"])
        v = int(k["inverse"][point])
        assert torch.isnan(got[v]).all()
        keep = torch.arange(k["V"]) != v
        assert torch.equal(FH.bits(got[keep]), FH.bits(k["got"][keep]))


@pytest.mark.parametrize("name", list(STAGES))
@pytest.mark.parametrize("shape", ["one point", "one voxel"])
def test_smallest_inputs(gpu, name, shape):
    cg, cf, c = STAGES[name]
    n = 1 if shape == "one point" else 70  # one voxel of 70 points: longer than a tile
    pts = np.tile(np.array([[0, 3, -2, 5]], np.int32), (n, 1))
    g = torch.Generator().manual_seed(12)
    F = torch.randn(n, cf, generator=g)
    G = torch.randn(1, cg, generator=g) if cg else None
    p = FH.stage_params(cg + cf, c, seed=13)
    got, inv = FH.run_stage(gpu, F, pts, p, G)
    want = FH.stage_ref(F, p, inv, 1, torch.float64, G)
    d32 = float((FH.stage_ref(F, p, inv, 1, torch.float32, G).double() - want).abs().max() / want.abs().max())
    assert got.shape == (1, c)
    assert float((got.double() - want).abs().max() / want.abs().max()) <= max(1e-4, 8 * d32)


def test_reduce_sum_and_unweighted_sum(gpu):
    """sv_voxel_reduce(SV_REDUCE_SUM) on small integers is the exact integer sum; UNWEIGHTED_SUM voxelises through it, in
    TensorField.sparse() and in SparseTensor(coordinates=...), and equals count * mean where that is exact"""
    from mrcc_amd import MinkowskiEngine as ME

    pts = FH.stage_cloud()
    inverse, V = FH.voxelize_ref(pts)
    g = torch.Generator().manual_seed(14)
    F = torch.randint(-8, 9, (len(pts), 5), generator=g).float()
    want = torch.zeros(V, 5, dtype=torch.float64).index_add_(0, inverse, F.double())
    SUM, MEAN = ME.SparseTensorQuantizationMode.UNWEIGHTED_SUM, ME.SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE
    c = torch.from_numpy(pts)
    got = ME.TensorField(F, c.float() + 0.5, quantization_mode=SUM, device=gpu).sparse().F.cpu()
    assert torch.equal(got.double(), want)
    st = ME.SparseTensor(F, coordinates=c, quantization_mode=SUM, device=gpu)
    assert torch.equal(st.F.cpu().double(), want)
    # count * mean is exact where the count is a power of two (the division and the product are then exact)
    counts = torch.bincount(inverse, minlength=V)
    pow2 = (counts & (counts - 1)) == 0
    mean = ME.TensorField(F, c.float() + 0.5, quantization_mode=MEAN, device=gpu).sparse().F.cpu()
    assert int(pow2.sum()) > 100
    assert torch.equal((mean * counts.unsqueeze(1).float())[pow2], got[pow2])
