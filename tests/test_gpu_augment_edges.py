"""sv_augment_points and sv_quantise_points (csrc/sv_augment.hip) and the batch builder at the edges the feature's own
tests (tests/test_gpu_augment.py) do not reach: batches of 1 to 1024 frames with empty frames at either end and in the
middle (the 1024-thread plan scan across waves, the workgroup -> frame search, the per-frame stats), inf / huge / NaN
coordinates and draws through every stage and through the stats, table rows that point outside the field buffer, and
the quantise kernel on exact inputs (int32 edges, negative quotients, cell borders, the three origin modes, frames
without rows, more frames than rows, guard rows).

Reference: tests/augment_helpers.py (H.apply_draws per frame; H.quantise_np, which tests/test_augment_cpu.py pins).
Bounds are those tests/test_gpu_augment.py states and justifies:
  frames without an elastic stage   1e-12 * max|x|
  frames with one                   1e-9 * (max|x| + mag * max|field|), the smaller stage's term with two stages
  stats                             exact: min and max do not depend on the order
  a frame alone against the frame inside a batch, float32 against float64 input, a second call: the same bits
  sv_quantise_points                exact: dyadic points, a power-of-two size
"""
from ctypes import c_double, c_int, c_int64

import numpy as np
import pytest
import torch
from scipy.stats import special_ortho_group

import augment_helpers as H

pytestmark = pytest.mark.gpu


def _A():
    from mrcc_amd.utils import augmentation

    return augmentation


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _bits(a):
    """float64 array -> its bit patterns (NaN payloads and the sign of zero included)"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _min_max(rows):
    """numpy's (min xyz, max xyz) of a frame's rows, a NaN winning; (+inf, -inf) without rows"""
    if not len(rows):
        return np.array([np.inf] * 3 + [-np.inf] * 3)
    return np.concatenate([np.min(rows, axis=0), np.max(rows, axis=0)])


# ---------------------------------------------------------------------------------------------------------------------
# A. sv_augment_points across batch shapes
# ---------------------------------------------------------------------------------------------------------------------
LENS = (0, 1, 255, 256, 257, 0, 513, 64)
PHASE = {1: 2, 2: 4, 63: 0, 64: 5, 65: 1, 1024: 6}  # empty first frame: B = 63, 64; empty last frame: B = 2, 1024
BATCHES = list(PHASE)
STAGES = (((5, 3, 7), 24, 160.0), ((6, 7, 5), 80, 640.0))  # (grid, gran, mag) of the two shared elastic fields
# B = 1024: the first frame, the last frame with rows, and both neighbours of seven empty frames
ALONE_1024 = (0, 1, 3, 6, 8, 257, 259, 510, 512, 513, 515, 766, 768, 1017, 1019, 1022)


def _frame_draws(rng, j, n, raws):
    """Draws of the frame with running number j (deterministic in j): every eighth frame two elastic stages, every
    eighth one; the other four stages from four bits that run through all 16 values inside each of those classes."""
    d = H.no_draws()
    if j % 8 == 0:
        d["elastic"] = [(raws[0],) + STAGES[0][1:], (raws[1],) + STAGES[1][1:]]
    elif j % 8 == 4:
        k = (j // 8) % 2
        d["elastic"] = [(raws[k],) + STAGES[k][1:]]
    rest = (j * 7 + j // 16) % 16
    if rest & 1:  # sigma and clip at the cloud's scale, so that the clip is active on some draws
        d["normals"], d["sigma"], d["clip"] = rng.standard_normal((n, 3)), 0.5, 1.0
    if rest & 2:
        d["transform"] = (float(rng.uniform(0, 5)), special_ortho_group.rvs(3, random_state=rng))
    if rest & 4:
        d["flip"] = -1 if j % 3 else 1
    if rest & 8:
        d["gravity"] = float(rng.uniform(0, 2 * np.pi))
    return d


def _combo(d):
    return (len(d["elastic"]), d["normals"] is not None, d["transform"] is not None, d["flip"] is not None,
            d["gravity"] is not None)


class BatchCase:
    """B frames of float32 points, their draws, the restatement of every frame (once), and the device runs: float32
    input, the same call again, and the same values as float64 input."""

    def __init__(self, B, gpu):
        A = _A()
        rng = np.random.default_rng(1000 + B)
        self.B = B
        self.lens = [LENS[(PHASE[B] + b) % len(LENS)] for b in range(B)]
        self.offsets = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int32)
        N = int(self.offsets[-1])
        self.pts = rng.uniform(-150, 150, (N, 3)).astype(np.float32)
        raws = [rng.standard_normal((3,) + s[0]).astype(np.float32) for s in STAGES]
        self.field_term = [s[2] * float(np.abs(np.stack(H.blur_field(r))).max()) for s, r in zip(STAGES, raws)]
        self.draws, j = [], B
        for n in self.lens:
            self.draws.append(_frame_draws(rng, j, n, raws))
            j += n > 0  # frames without rows take draws too (their table row is never used) but no running number
        self.frames = [self.pts[lo:hi] for lo, hi in zip(self.offsets[:-1], self.offsets[1:])]
        self.ref = [H.apply_draws(x, d) for x, d in zip(self.frames, self.draws)]
        normals = np.zeros((N, 3))
        for b, d in enumerate(self.draws):
            if d["normals"] is not None:
                normals[self.offsets[b]: self.offsets[b + 1]] = d["normals"]
        table, raw, dims = A._table_and_fields([H.to_package_draws(d) for d in self.draws])
        self.fields_d = A.elastic_fields(raw, dims, gpu) if len(dims) else None
        self.table_d, self.off_d = _dev(table, gpu), _dev(self.offsets, gpu)
        self.pts_d, self.normals_d = _dev(self.pts, gpu), _dev(normals, gpu)
        self.pts64_d = _dev(self.pts.astype(np.float64), gpu)
        run = lambda p: tuple(t.cpu().numpy() for t in  # noqa: E731
                              A.augment_points(p, self.off_d, self.table_d, self.fields_d, self.normals_d))
        self.out, self.stats = run(self.pts_d)
        self.again = run(self.pts_d)
        self.from64 = run(self.pts64_d)

    def alone(self, b):
        """frame b as a B = 1 call on its slices of points and noise, its table row and the same fields buffer"""
        lo, hi = int(self.offsets[b]), int(self.offsets[b + 1])
        off = torch.tensor([0, hi - lo], dtype=torch.int32, device=self.pts_d.device)
        out, stats = _A().augment_points(self.pts_d[lo:hi], off, self.table_d[b: b + 1], self.fields_d,
                                         self.normals_d[lo:hi])
        return out.cpu().numpy(), stats.cpu().numpy()


@pytest.fixture(scope="module")
def case(request, gpu):
    return BatchCase(request.param, gpu)


def on_batches(*batches):
    return pytest.mark.parametrize("case", batches, indirect=True, ids=[f"B{b}" for b in batches])


@on_batches(*BATCHES)
def test_batch_against_the_restatement_frame_by_frame(case):
    assert case.out.dtype == np.float64 and case.out.shape == (len(case.pts), 3) and case.stats.shape == (case.B, 6)
    assert not np.isnan(case.out).any()
    combos = {_combo(d) for d, n in zip(case.draws, case.lens) if n}
    if case.B == 1024:  # every combination of the five stages, nothing firing and two elastic stages alone included
        assert {(min(c[0], 1),) + c[1:] for c in combos} == {(e, a, b, c, d) for e in (0, 1) for a in (False, True)
                                                              for b in (False, True) for c in (False, True)
                                                              for d in (False, True)}
        assert {c[1:] for c in combos if c[0] == 2} == {c[1:] for c in combos if c[0] == 0} and len(combos) == 48
        assert len(case.pts) == 128 * sum(LENS)
    worst = {"plain": 0.0, "elastic": 0.0}
    for b, (x, d, ref) in enumerate(zip(case.frames, case.draws, case.ref)):
        if not len(x):
            continue
        got = case.out[case.offsets[b]: case.offsets[b + 1]]
        err = float(np.abs(got - ref).max())
        if d["elastic"]:
            kind = "elastic"
            term = min(case.field_term[STAGES.index((raw.shape[1:], gran, mag))] for raw, gran, mag in d["elastic"])
            bound = 1e-9 * (float(np.abs(x).max()) + term)
        else:
            kind, bound = "plain", 1e-12 * float(np.abs(x).max())
        worst[kind] = max(worst[kind], err / bound)
        assert err <= bound, (b, len(x), _combo(d), err, bound)
    print(f"B={case.B}: {sum(n > 0 for n in case.lens)} frames with rows, {len(combos)} stage combinations; worst "
          f"error / bound: {worst['plain']:.2e} without an elastic stage, {worst['elastic']:.2e} with one")


@on_batches(*BATCHES)
def test_float32_and_float64_input_give_the_same_bits(case):
    assert np.array_equal(_bits(case.out), _bits(case.from64[0]))
    assert np.array_equal(_bits(case.stats), _bits(case.from64[1]))


@on_batches(*BATCHES)
def test_second_call_gives_the_same_bits(case):
    assert np.array_equal(_bits(case.out), _bits(case.again[0]))
    assert np.array_equal(_bits(case.stats), _bits(case.again[1]))


@on_batches(*BATCHES)
def test_stats_are_min_and_max_of_the_frames_own_rows(case):
    empty = np.array([np.inf] * 3 + [-np.inf] * 3)
    for b, n in enumerate(case.lens):
        want = _min_max(case.out[case.offsets[b]: case.offsets[b + 1]])
        assert np.array_equal(case.stats[b], want), (b, n)
        if n == 0:
            assert np.array_equal(case.stats[b], empty), b
    assert case.B < 63 or 0 in case.lens


@on_batches(65, 1024)
def test_frame_alone_equals_frame_inside_the_batch(case):
    frames = [b for b, n in enumerate(case.lens) if n] if case.B == 65 else list(ALONE_1024)
    if case.B == 1024:  # the picks: first and last frame with rows, and both neighbours of seven empty frames
        empties = [b for b in range(1, case.B - 1) if b - 1 in frames and b + 1 in frames and case.lens[b] == 0]
        assert len(empties) == 7 and case.lens[0] and not case.lens[1023] and not any(case.lens[1023:])
        assert all(case.lens[b] for b in frames) and frames[-1] == 1022
    for b in frames:
        out, stats = case.alone(b)
        assert np.array_equal(_bits(out), _bits(case.out[case.offsets[b]: case.offsets[b + 1]])), b
        assert np.array_equal(_bits(stats[0]), _bits(case.stats[b])), b
    print(f"B={case.B}: {len(frames)} frames alone, stage combinations {len({_combo(case.draws[b]) for b in frames})}")


# ---------------------------------------------------------------------------------------------------------------------
# B. special values through the stages and the stats
# ---------------------------------------------------------------------------------------------------------------------
SP_LEN, SP_B = 300, 4
SP_STAGE = ((5, 3, 7), 24, 160.0)
# rows of frame 1: lane 0, lane 63, lane 64 and the last row of its first workgroup
SP_PLANTED = {0: (0, np.inf), 63: (2, -np.inf), 64: (1, 1e300), 255: (1, np.nan)}


def _special_cloud(planted):
    rng = np.random.default_rng(77)
    ext = np.array([(b - 1) * SP_STAGE[1] for b in SP_STAGE[0]], dtype=np.float64)
    x = rng.uniform(-0.9, 0.9, (SP_B * SP_LEN, 3)) * ext  # every clean row inside the grid
    if planted:
        for row, (col, v) in SP_PLANTED.items():
            x[SP_LEN + row, col] = v
    return x


def _special_run(gpu, x, draws):
    """the 4 x 300 batch on float64 input -> (out [N, 3], stats [4, 6], the restatement's frames)"""
    A = _A()
    off = np.arange(SP_B + 1, dtype=np.int32) * SP_LEN
    table, raw, dims = A._table_and_fields([H.to_package_draws(d) for d in draws])
    fields = A.elastic_fields(raw, dims, gpu) if len(dims) else None
    normals = None
    if any(d["normals"] is not None for d in draws):
        normals = _dev(np.concatenate([d["normals"] for d in draws]), gpu)
    out, stats = A.augment_points(_dev(x, gpu), _dev(off, gpu), _dev(table, gpu), fields, normals)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = [H.apply_draws(x[b * SP_LEN: (b + 1) * SP_LEN], d) for b, d in enumerate(draws)]
    return out.cpu().numpy(), stats.cpu().numpy(), ref


def _special_draws(kind):
    rng = np.random.default_rng(78)
    draws = []
    for b in range(SP_B):
        d = H.no_draws()
        if kind == "elastic":
            d["elastic"] = [(rng.standard_normal((3,) + SP_STAGE[0]).astype(np.float32),) + SP_STAGE[1:]]
        elif kind == "rigid":
            d["transform"] = (float(rng.uniform(1, 5)), special_ortho_group.rvs(3, random_state=rng))
            d["flip"], d["gravity"] = (-1, 1)[b % 2], float(rng.uniform(0.3, 1.2))
        else:
            d["normals"], d["sigma"], d["clip"] = rng.standard_normal((SP_LEN, 3)), 0.5, 1.0
        draws.append(d)
    return draws


def _same_special_pattern(got, ref):
    """NaNs in the same places, infinities in the same places with the same sign"""
    return (np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
            and np.array_equal(np.sign(got[np.isinf(got)]), np.sign(ref[np.isinf(ref)])))


def _check_stats(out, stats):
    for b in range(SP_B):
        want = _min_max(out[b * SP_LEN: (b + 1) * SP_LEN])
        assert np.array_equal(stats[b], want, equal_nan=True), (b, stats[b], want)


@pytest.mark.parametrize("kind", ["elastic", "rigid", "noise"])
def test_special_values_through_the_stages_and_the_stats(gpu, kind):
    draws = _special_draws(kind)
    x, clean = _special_cloud(True), _special_cloud(False)
    nan_draw = (2 * SP_LEN + 5, 1)  # noise run: a NaN draw on a clean row of frame 2
    if kind == "noise":
        draws[2]["normals"][5, 1] = np.nan
    out, stats, ref = _special_run(gpu, x, draws)
    if kind == "noise":
        draws[2]["normals"][5, 1] = 0.25
    out_clean, stats_clean, _ = _special_run(gpu, clean, draws)
    ref = np.concatenate(ref)
    special = np.zeros(len(x), dtype=bool)
    special[[SP_LEN + r for r in SP_PLANTED]] = True
    if kind == "noise":
        special[nan_draw[0]] = True
    # the rows without a special value: the usual bound, frame by frame
    field_term = [d["elastic"][0][2] * float(np.abs(np.stack(H.blur_field(d["elastic"][0][0]))).max())
                  if d["elastic"] else None for d in draws]
    for b in range(SP_B):
        rows = np.flatnonzero(~special[b * SP_LEN: (b + 1) * SP_LEN]) + b * SP_LEN
        scale = float(np.abs(x[rows]).max())
        bound = 1e-12 * scale if field_term[b] is None else 1e-9 * (scale + field_term[b])
        err = float(np.abs(out[rows] - ref[rows]).max())
        print(f"{kind} frame {b}: max abs err {err:.2e} (bound {bound:.2e})")
        assert np.isfinite(out[rows]).all() and err <= bound
    # the rows with one: the restatement's NaN / inf pattern; finite entries within 1e-12 of the row's own scale
    assert _same_special_pattern(out, ref)
    for r in np.flatnonzero(special):
        fin = np.isfinite(ref[r])
        if fin.any():
            scale = float(np.abs(x[r][np.isfinite(x[r])]).max())
            assert np.abs(out[r][fin] - ref[r][fin]).max() <= (1e-9 if kind == "elastic" else 1e-12) * scale, r
    f1 = out[SP_LEN: 2 * SP_LEN]
    if kind == "elastic":
        # inf and 1e300 lie outside the grid: zero displacement, the input's bits, in scipy as in the kernel; NaN -> NaN
        for row in (0, 63, 64):
            assert np.array_equal(_bits(f1[row]), _bits(x[SP_LEN + row])), row
            assert np.array_equal(_bits(ref[SP_LEN + row]), _bits(x[SP_LEN + row])), row
        assert np.isnan(f1[255]).all() and np.isnan(ref[SP_LEN + 255]).all()
        assert np.isnan(stats[1]).all()  # the NaN row is NaN in every column here: every min and every max
    elif kind == "rigid":
        # the three-term products: inf * 0 is NaN, so an inf in one component spreads to the others, as in numpy
        assert np.isnan(f1[[0, 63, 255]]).any(axis=1).all() and np.isnan(ref[SP_LEN: 2 * SP_LEN][[0, 63]]).any(axis=1).all()
        assert np.isfinite(f1[64]).all() and np.abs(f1[64]).max() > 1e299
        assert np.isnan(stats[1]).all()
    else:
        assert np.array_equal(np.isnan(out[nan_draw[0]]), [False, True, False])
        assert np.isnan(stats[2, [1, 4]]).all() and np.isfinite(stats[2, [0, 2, 3, 5]]).all()
        assert f1[0, 0] == np.inf and f1[63, 2] == -np.inf and np.isnan(f1[255, 1]) and np.isfinite(f1[255, [0, 2]]).all()
        # y holds a NaN: both its min and its max; x and z hold only an inf each beside finite values: max x, min z
        assert np.isnan(stats[1, [1, 4]]).all() and stats[1, 3] == np.inf and stats[1, 2] == -np.inf
        assert np.isfinite(stats[1, [0, 5]]).all()
    _check_stats(out, stats)
    _check_stats(out_clean, stats_clean)
    assert np.isfinite(out_clean).all() and np.isfinite(stats_clean).all()
    # isolation: the clean frames do not see frame 1's rows (nor, in the noise run, more than the one row of frame 2)
    same = np.ones(len(x), dtype=bool)
    same[SP_LEN: 2 * SP_LEN] = False
    if kind == "noise":
        same[nan_draw[0]] = False
    assert np.array_equal(_bits(out[same]), _bits(out_clean[same]))
    assert np.array_equal(_bits(out[SP_LEN: 2 * SP_LEN][~special[SP_LEN: 2 * SP_LEN]]),
                          _bits(out_clean[SP_LEN: 2 * SP_LEN][~special[SP_LEN: 2 * SP_LEN]]))
    for b in ((0, 2, 3) if kind != "noise" else (0, 3)):
        assert np.array_equal(_bits(stats[b]), _bits(stats_clean[b])), b


@pytest.mark.parametrize("how", ["offset_negative", "offset_at_the_end", "field_overhangs_by_one", "dimension_one"])
def test_broken_table_row_makes_its_frame_nan_and_nothing_else(gpu, how):
    """a table row whose field does not lie inside [0, fields_len), or has a dimension below 2: the kernel tests the row
    before it forms an address, so nothing outside the buffer is read"""
    A = _A()
    L = A._lib
    rng = np.random.default_rng(79)
    lens = (64, 300, 65)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ext = np.array([(b - 1) * SP_STAGE[1] for b in SP_STAGE[0]], dtype=np.float64)
    x = rng.uniform(-0.9, 0.9, (sum(lens), 3)) * ext
    draws = []
    for _ in lens:
        d = H.no_draws()
        d["elastic"] = [(rng.standard_normal((3,) + SP_STAGE[0]).astype(np.float32),) + SP_STAGE[1:]]
        d["flip"] = -1
        draws.append(d)
    table, raw, dims = A._table_and_fields([H.to_package_draws(d) for d in draws])
    fields = A.elastic_fields(raw, dims, gpu)
    cells3 = 3 * int(np.prod(SP_STAGE[0]))
    assert fields.numel() == 3 * cells3 and table[1, L.SV_AUG_E_OFFSET] == cells3
    broken = table.copy()
    if how == "dimension_one":
        broken[1, L.SV_AUG_E_BX] = 1
    else:
        broken[1, L.SV_AUG_E_OFFSET] = {"offset_negative": -1, "offset_at_the_end": fields.numel(),
                                        "field_overhangs_by_one": fields.numel() - cells3 + 1}[how]
    x_d, off_d = _dev(x, gpu), _dev(off, gpu)
    good, good_stats = (t.cpu().numpy() for t in A.augment_points(x_d, off_d, _dev(table, gpu), fields))
    out, stats = (t.cpu().numpy() for t in A.augment_points(x_d, off_d, _dev(broken, gpu), fields))
    assert np.isfinite(good).all() and np.abs(good - x * [-1, 1, 1]).max() > 1.0  # the healthy run moved every frame
    assert np.isnan(out[off[1]: off[2]]).all() and np.isnan(stats[1]).all()
    for b in (0, 2):
        assert np.array_equal(_bits(out[off[b]: off[b + 1]]), _bits(good[off[b]: off[b + 1]]))
        assert np.array_equal(_bits(stats[b]), _bits(good_stats[b]))


# ---------------------------------------------------------------------------------------------------------------------
# C. sv_quantise_points directly
# ---------------------------------------------------------------------------------------------------------------------
QSIZE = 0.125
TOP = 2.0 ** 31
EMPTY_STATS = [np.inf] * 3 + [-np.inf] * 3


def _quantise(gpu, points, offsets, stats, origin, size=QSIZE):
    got = _A().quantise_points(_dev(np.asarray(points, np.float64), gpu), _dev(np.asarray(offsets, np.int32), gpu),
                               _dev(np.asarray(stats, np.float64), gpu), origin, size)
    return tuple(t.cpu().numpy() for t in got)


def _quantise_into(gpu, points, offsets, stats, origin, size, coords, shifted, shift):
    """sv_quantise_points into the caller's own buffers (device tensors, possibly views into larger ones)"""
    from mrcc_amd._lib import call, ptr, stream_ptr

    keep = [_dev(np.asarray(points, np.float64), gpu), _dev(np.asarray(offsets, np.int32), gpu),
            _dev(np.asarray(stats, np.float64), gpu)]
    call("sv_quantise_points", ptr(keep[0]), ptr(keep[1]), c_int64(len(points)), c_int(len(offsets) - 1), ptr(keep[2]),
         c_int(origin), c_double(size), ptr(coords), ptr(shifted), ptr(shift), stream_ptr())
    torch.cuda.synchronize()


def _expect(got, points, offsets, stats, origin, size=QSIZE):
    coords, shifted, shift = got
    want_c, want_f, want_s = H.quantise_np(points, offsets, stats, origin, size)
    assert coords.dtype == np.int32 and shifted.dtype == np.float32 and shift.dtype == np.float64
    assert np.array_equal(coords, want_c)
    assert np.array_equal(shifted.view(np.int32), want_f.view(np.int32))
    assert np.array_equal(shift, want_s, equal_nan=True)
    return want_c, want_f, want_s


def test_quantise_plain_values_and_int32_edges(gpu):
    col = np.array([-0.5, -1e-300, -0.0, 0.0, QSIZE, -QSIZE, 3 * QSIZE, -7 * QSIZE, 1024.0, (TOP - 1) * QSIZE,
                    -TOP * QSIZE, TOP * QSIZE, (-TOP - 1) * QSIZE, np.inf, -np.inf, np.nan, 1e300])
    cells = [-4, -1, 0, 0, 1, -1, 3, -7, 8192, 2 ** 31 - 1, -2 ** 31] + [H.INT32_MIN] * 6
    p = np.stack([col, np.roll(col, 5), col[::-1]], axis=1)
    # stats are read (shift_out is written) but nothing is subtracted under SV_ORIGIN_NONE: values that would show
    stats = np.array([[1.0, 2.0, 3.0, 5.0, 6.0, 7.0]])
    got = _quantise(gpu, p, [0, len(p)], stats, H.ORIGIN_NONE)
    _expect(got, p, [0, len(p)], stats, H.ORIGIN_NONE)
    coords, shifted, shift = got
    assert coords[:, 1].tolist() == cells and coords[:, 3].tolist() == cells[::-1]
    assert coords[:, 2].tolist() == np.roll(cells, 5).tolist() and not coords[:, 0].any() and not shift.any()
    with np.errstate(invalid="ignore"):
        finite = np.abs(p) < 1e6  # the plain values: np.floor(p / size) as it stands
    assert np.array_equal(coords[:, 1:][finite], np.floor(p / QSIZE)[finite].astype(np.int64))
    with np.errstate(over="ignore"):
        assert np.array_equal(shifted, p.astype(np.float32), equal_nan=True)  # float32(p): 1e300 -> inf, -0.0 kept
    assert np.signbit(shifted[2, 0]) and not np.signbit(shifted[3, 0])


@pytest.mark.parametrize("origin", [H.ORIGIN_NONE, H.ORIGIN_CENTER, H.ORIGIN_BASE])
def test_quantise_origin_modes_beside_empty_frames(gpu, origin):
    offsets = [0, 0, 5, 5, 5, 9, 9]  # empty frames first, in the middle (two) and last
    rng = np.random.default_rng(80)
    p = rng.integers(-4096, 4096, (9, 3)) / 64.0  # dyadic: every difference, quotient and rounding is exact
    p[2], p[6] = [0.0, -QSIZE, QSIZE], [-0.0, 2 * QSIZE, -2 * QSIZE]
    stats = np.array([EMPTY_STATS, _min_max(p[:5]), EMPTY_STATS, EMPTY_STATS, _min_max(p[5:]), EMPTY_STATS])
    got = _quantise(gpu, p, offsets, stats, origin)
    want_c, _, want_s = _expect(got, p, offsets, stats, origin)
    assert got[0][:, 0].tolist() == [1] * 5 + [4] * 4  # the owning frame of every row
    assert (want_c[:, 1:] != H.INT32_MIN).all()
    for b, (lo, hi) in ((1, (0, 5)), (4, (5, 9))):
        s = {H.ORIGIN_NONE: np.zeros(3), H.ORIGIN_CENTER: (p[lo:hi].max(0) + p[lo:hi].min(0)) / 2,
             H.ORIGIN_BASE: p[lo:hi].min(0)}[origin]
        assert np.array_equal(got[2][b], s)
        assert np.array_equal(got[0][lo:hi, 1:], np.floor((p[lo:hi] - s) / QSIZE).astype(np.int32))
    for b in (0, 2, 3, 5):  # (-inf + inf) / 2 under CENTER, min = +inf under BASE
        want = {H.ORIGIN_NONE: 0.0, H.ORIGIN_BASE: np.inf}.get(origin)
        assert np.isnan(got[2][b]).all() if want is None else (got[2][b] == want).all()
        assert np.array_equal(got[2][b], want_s[b], equal_nan=True)


def test_quantise_more_frames_than_rows(gpu):
    """B = 1024 frames and N = 5 rows: the grid is sized by the 3072 shift_out entries, not by N"""
    B, sentinel = 1024, 12345.0
    lens = np.zeros(B, dtype=np.int64)
    lens[[0, 500, 1023]] = 1, 3, 1
    offsets = np.concatenate([[0], np.cumsum(lens)])
    rng = np.random.default_rng(81)
    p = rng.integers(-4096, 4096, (5, 3)) / 64.0
    lo = rng.integers(-64, 64, (B, 3)) / 8.0
    stats = np.concatenate([lo, lo + rng.integers(0, 64, (B, 3)) / 4.0], axis=1)
    coords = torch.full((5, 4), -7, dtype=torch.int32, device=gpu)
    shifted = torch.full((5, 3), -7.0, dtype=torch.float32, device=gpu)
    shift = torch.full((B, 3), sentinel, dtype=torch.float64, device=gpu)
    _quantise_into(gpu, p, offsets, stats, H.ORIGIN_CENTER, QSIZE, coords, shifted, shift)
    got = (coords.cpu().numpy(), shifted.cpu().numpy(), shift.cpu().numpy())
    assert not (stats[:, 3:] + stats[:, :3] == 2 * sentinel).any()
    assert (got[2] != sentinel).all()  # all 3072 entries written
    _expect(got, p, offsets, stats, H.ORIGIN_CENTER)
    assert got[0][:, 0].tolist() == [0, 500, 500, 500, 1023]


def test_quantise_nan_centre_stays_in_its_frame(gpu):
    rng = np.random.default_rng(82)
    offsets = [0, 70, 370, 400]
    p = rng.integers(-4096, 4096, (400, 3)) / 64.0
    stats = np.array([_min_max(p[a:b]) for a, b in zip(offsets[:-1], offsets[1:])])
    base = _quantise(gpu, p, offsets, stats, H.ORIGIN_CENTER)
    _expect(base, p, offsets, stats, H.ORIGIN_CENTER)
    bad = stats.copy()
    bad[1, 4] = np.nan  # max y of frame 1, as sv_augment_points reports a NaN in the column
    got = _quantise(gpu, p, offsets, bad, H.ORIGIN_CENTER)
    _expect(got, p, offsets, bad, H.ORIGIN_CENTER)
    assert (got[0][70:370, 2] == H.INT32_MIN).all() and np.isnan(got[1][70:370, 1]).all() and np.isnan(got[2][1, 1])
    keep = np.ones((400, 3), dtype=bool)
    keep[70:370, 1] = False
    assert np.array_equal(got[0][:, 1:][keep], base[0][:, 1:][keep]) and np.array_equal(got[0][:, 0], base[0][:, 0])
    assert np.array_equal(got[1][keep], base[1][keep])


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_quantise_writes_its_rows_and_no_others(gpu, n):
    G = 64  # guard rows on either side of coords and shifted
    rng = np.random.default_rng(83 + n)
    p = rng.integers(-4096, 4096, (n, 3)) / 64.0
    stats = np.array([_min_max(p)])
    coords = torch.full((n + 2 * G, 4), -7, dtype=torch.int32, device=gpu)
    shifted = torch.full((n + 2 * G, 3), -7.0, dtype=torch.float32, device=gpu)
    shift = torch.full((1 + 2 * G, 3), -7.0, dtype=torch.float64, device=gpu)
    _quantise_into(gpu, p, [0, n], stats, H.ORIGIN_BASE, QSIZE, coords[G: G + n], shifted[G: G + n], shift[G: G + 1])
    c, f, s = coords.cpu().numpy(), shifted.cpu().numpy(), shift.cpu().numpy()
    _expect((c[G: G + n], f[G: G + n], s[G: G + 1]), p, [0, n], stats, H.ORIGIN_BASE)
    for a in (c, f, s):
        rows = n if a is not s else 1
        assert (a[:G] == -7).all() and (a[G + rows:] == -7).all()
    assert (c[G: G + n, 1:].min(axis=0) == 0).all()  # base at the origin: the frame's minimum lands in cell 0


# ---------------------------------------------------------------------------------------------------------------------
# D. the batch builder with frames without rows, and with a NaN point
# ---------------------------------------------------------------------------------------------------------------------
D_LENS = (300, 0, 64, 0)
D_QSIZE = 40.0
IGNORE = -100


def _builder_inputs():
    """float32 frames none of whose centred coordinates lies within 1e-6 cells of a cell border (exact zeros exempt), as
    tests/test_gpu_augment.py picks its seed"""
    for seed in range(90, 110):
        rng = np.random.default_rng(seed)
        pts = [rng.uniform(-150, 150, (n, 3)).astype(np.float32) for n in D_LENS]
        pts[0][7] = pts[0][3]  # two points of one voxel with different labels
        feats = [rng.normal(size=(n, 3)).astype(np.float32) for n in D_LENS]
        labels = [rng.integers(0, 4, size=n).astype(np.int64) for n in D_LENS]
        labels[0][3], labels[0][7] = 1, 2
        shifted = [p.astype(np.float64) - (p.astype(np.float64).max(0) + p.astype(np.float64).min(0)) / 2 if len(p)
                   else np.zeros((0, 3)) for p in pts]
        cells = np.concatenate(shifted) / D_QSIZE
        if not ((np.abs(cells - np.rint(cells)) < 1e-6) & (np.concatenate(shifted) != 0.0)).any():
            return pts, feats, labels, shifted
    raise AssertionError("no seed without a point near a cell border")


def test_batch_builder_with_empty_frames_and_a_nan_point(gpu):
    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd._lib import SvHipError

    A = _A()
    pts, feats, labels, shifted = _builder_inputs()
    kw = dict(quantization_size=D_QSIZE, ignore_label=IGNORE, center_at_origin=True, device=gpu)  # every stage off
    coords, f, l, voxel_offsets, extras = A.augment_quantize_batch(pts, feats, labels, return_extras=True, **kw)
    # the per-frame path of test_batch_builder_against_per_frame_path on the frames with rows
    ref_c, ref_f, ref_l = [], [], []
    for s, ft, lb in zip(shifted, feats, labels):
        if len(s):
            c, uf, ul = ME.utils.sparse_quantize(coordinates=s, features=ft, labels=lb, quantization_size=D_QSIZE,
                                                 ignore_label=IGNORE)
        else:
            c, uf, ul = np.zeros((0, 3), np.int32), ft, lb
        ref_c.append(c), ref_f.append(uf), ref_l.append(ul)
    counts = [len(c) for c in ref_c]
    assert counts[1] == counts[3] == 0 and 1 < counts[0] < D_LENS[0] and (np.concatenate(ref_l) == IGNORE).any()
    assert torch.equal(coords.cpu(), ME.utils.batched_coordinates(ref_c))
    assert np.array_equal(f.cpu().numpy().view(np.int32), np.concatenate(ref_f).view(np.int32))
    assert np.array_equal(l.cpu().numpy(), np.concatenate(ref_l))
    want_off = [0, counts[0], counts[0], counts[0] + counts[2], counts[0] + counts[2]]
    assert voxel_offsets.cpu().tolist() == want_off  # repeated across the frames without rows
    shift = extras["origin_offset"].cpu().numpy()
    assert np.isnan(shift[[1, 3]]).all() and np.isfinite(shift[[0, 2]]).all()
    # one NaN coordinate in frame 2: under center_at_origin its column's centre is NaN, so all 64 rows of the frame
    # quantise to INT32_MIN; sparse._voxelize documents an SvHipError with the count of rows outside the key range
    bad = [p.copy() for p in pts]
    bad[2][10, 1] = np.nan
    with pytest.raises(SvHipError, match=r"^64 points have coordinates outside the key range"):
        A.augment_quantize_batch(bad, feats, labels, **kw)
    # the builder raises, so frame 0 is observed one step earlier: what the builder hands to sv_voxelize for frame 0
    # (coordinates, shifted points, origin) has the same bits with and without the NaN, and sv_voxelize's representatives,
    # features and labels are functions of those rows alone (first assertions above)
    off_d = _dev(np.concatenate([[0], np.cumsum(D_LENS)]).astype(np.int32), gpu)
    table_d = _dev(A._table_and_fields([A.AugmentationDraws() for _ in D_LENS])[0], gpu)
    staged = []
    for frames in (pts, bad):
        aug, stats = A.augment_points(_dev(np.concatenate(frames), gpu), off_d, table_d)
        staged.append([t.cpu().numpy() for t in A.quantise_points(aug, off_d, stats, A._lib.SV_ORIGIN_CENTER, D_QSIZE)])
    (c0, s0, o0), (c1, s1, o1) = staged
    n0 = D_LENS[0]
    assert np.array_equal(c0[:n0], c1[:n0]) and np.array_equal(s0[:n0].view(np.int32), s1[:n0].view(np.int32))
    assert np.array_equal(_bits(o0[0]), _bits(o1[0]))
    assert (c1[n0:, 2] == H.INT32_MIN).all() and (c1[n0:, [1, 3]] != H.INT32_MIN).all()
    assert np.array_equal(c0[n0:, [0, 1, 3]], c1[n0:, [0, 1, 3]])
    inv = extras["inverse"].cpu().numpy()
    assert np.array_equal(coords.cpu().numpy()[inv[:n0]], c0[:n0])  # frame 0's voxels are those rows' cells
