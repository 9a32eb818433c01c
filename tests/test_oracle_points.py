"""The float32 emulations of the PointNet++ grouping primitives in oracle/sv_oracle.py (query_ball_point, three_nn,
three_nn_interpolate) against plain float64 brute force.  tests/test_gpu_points.py compares the HIP kernels with these
emulations bit for bit, so they are pinned first: wherever float64 leaves no doubt about the answer (every margin far
above float32 rounding) the emulation must give it, and on coordinates that float32 holds exactly it must be exact."""
import numpy as np

MARGIN = 1e-5  # squared-distance margin: > 10x the float32 rounding of an expanded distance of points in [-1, 1]^3


def _d64(q, p):
    """float64 squared distances [Q, P] of float32 points, difference form"""
    d = q.astype(np.float64)[:, None, :] - p.astype(np.float64)[None, :, :]
    return (d * d).sum(-1)


def test_ball_query_emulation_matches_float64_on_clear_rows(oracle):
    rng = np.random.default_rng(11)
    N, S, radius, nsample = 1000, 64, 0.3, 16
    xyz = rng.uniform(-1, 1, size=(1, N, 3)).astype(np.float32)
    new_xyz = xyz[:, rng.permutation(N)[:S]]
    got = oracle.query_ball_point(radius, nsample, xyz, new_xyz)[0]
    d = _d64(new_xyz[0], xyz[0])
    r2 = radius * radius
    clear = (np.abs(d - r2) > MARGIN).all(axis=1)
    share = clear.mean()
    print(f"ball query: {100 * share:.1f} % of rows have every float64 margin above {MARGIN}")
    assert share >= 0.95
    full = padded = 0
    for s in np.nonzero(clear)[0]:
        hits = np.nonzero(d[s] <= r2)[0]
        want = np.full(nsample, hits[0])  # the centre is a cloud point: never empty
        want[: min(nsample, len(hits))] = hits[:nsample]
        assert np.array_equal(got[s], want), s
        full += len(hits) >= nsample
        padded += len(hits) < nsample
    assert full > 0 and padded > 0  # truncated and first-hit padded balls both occur


def test_three_nn_emulation_matches_float64_on_clear_rows(oracle):
    rng = np.random.default_rng(12)
    N, S = 700, 300
    xyz1 = rng.uniform(-0.5, 0.5, size=(1, N, 3)).astype(np.float32)
    xyz2 = rng.uniform(-0.5, 0.5, size=(1, S, 3)).astype(np.float32)
    idx, w = oracle.three_nn(xyz1, xyz2)
    assert idx.dtype == np.int32 and idx.shape == (1, N, 3) and w.dtype == np.float32 and w.shape == (1, N, 3)
    d = _d64(xyz1[0], xyz2[0])
    order = np.argsort(d, axis=1, kind="stable")[:, :4]
    near = np.take_along_axis(d, order, axis=1)
    clear = (np.diff(near, axis=1) > MARGIN).all(axis=1)  # sorted: consecutive gaps bound every pairwise gap
    share = clear.mean()
    print(f"3-NN: {100 * share:.1f} % of rows have their four nearest float64 distances more than {MARGIN} apart")
    assert share >= 0.95
    assert np.array_equal(idx[0][clear], order[clear, :3])
    # weights: float64 arithmetic on the emulation's own float32 distances isolates the division and normalisation:
    # one add and one divide per w_i, two adds for ws, one divide -> at most 7 unit roundoffs
    d32 = oracle.three_nn_distances(xyz1, xyz2, idx)
    assert d32.dtype == np.float32 and (d32 > 0).all()
    recip = 1.0 / (d32.astype(np.float64) + np.float64(np.float32(1e-8)))
    want = recip / recip.sum(-1, keepdims=True)
    rel = np.abs(w.astype(np.float64) - want) / want
    print(f"3-NN weights: worst relative error {rel.max() / 2.0 ** -24:.2f} unit roundoffs")
    assert rel.max() <= 8 * 2.0 ** -24
    # the interpolation is the gather of those indices and weights, (p0*w0 + p1*w1) + p2*w2
    pts = rng.standard_normal((1, S, 5)).astype(np.float32)
    out = oracle.three_nn_interpolate(xyz1, xyz2, pts)
    assert out.dtype == np.float32 and out.shape == (1, N, 5)
    g = [pts[0][idx[0, :, k]] * w[0, :, k, None] for k in range(3)]
    assert np.array_equal(out[0], (g[0] + g[1]) + g[2])
    ref = (pts[0].astype(np.float64)[order[:, :3]] * want[0][:, :, None]).sum(1)
    assert np.abs(out[0] - ref)[clear].max() <= 16 * 2.0 ** -24 * np.abs(pts).max()


def test_three_nn_emulation_selection_rules(oracle):
    """ties keep the lower index, a NaN distance is never selected, unfilled slots keep index 0"""
    src = np.array([[[1, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1], [1, 0, 0], [1, 0, 0]]], dtype=np.float32)
    q = np.array([[[1, 0, 0], [0, 0, 0], [np.nan, 0, 0]]], dtype=np.float32)
    idx, w = oracle.three_nn(q, src)
    assert idx[0, 0].tolist() == [0, 2, 4]  # four copies: the three lowest indices, in order
    assert idx[0, 1].tolist() == [0, 1, 2]  # six sources at distance 1
    assert idx[0, 2].tolist() == [0, 0, 0] and np.isnan(w[0, 2]).all()
    assert w[0, 0, 0] == w[0, 0, 1] == w[0, 0, 2] and abs(float(w[0, 0].sum()) - 1) < 1e-6  # three distances of 0
    src[0, 0] = np.nan
    src[0, 4, 1] = np.inf
    idx, _ = oracle.three_nn(q[:, :2], src)
    assert idx[0, 0].tolist() == [2, 5, 1] and idx[0, 1].tolist() == [1, 2, 3]


def test_expanded_distance_is_exact_on_the_eighth_grid(oracle):
    """coordinates that are multiples of 1/8 in [-2, 2]: every product and sum of the expanded form is a multiple of 1/64
    below 2^6, exact in float32 - so the emulated distance IS the float64 distance and `d == r^2` cases can be placed"""
    rng = np.random.default_rng(13)
    q = (rng.integers(-16, 17, size=(1, 200, 3)) / 8).astype(np.float32)
    p = (rng.integers(-16, 17, size=(1, 300, 3)) / 8).astype(np.float32)
    p[0, :6] = q[0, 0] + np.array([[.5, 0, 0], [-.5, 0, 0], [0, .5, 0], [0, -.5, 0], [0, 0, .5], [0, 0, -.5]], np.float32)
    every = np.broadcast_to(np.arange(300), (1, 200, 300))
    d32 = oracle.three_nn_distances(q, p, every)[0]
    assert d32.dtype == np.float32
    assert np.array_equal(d32.astype(np.float64), _d64(q[0], p[0]))
    assert (d32[0, :6] == np.float32(0.25)).all()
    # the ball query's `not (d > r^2)` with r^2 = (float)(radius * radius), on both sides of 0.25f
    below = 0.4999999850988386
    assert np.float32(below * below) == np.nextafter(np.float32(0.25), np.float32(0))
    assert np.float32(np.nextafter(0.5, 0) ** 2) == np.float32(0.25)
    d = _d64(q[0], p[0])
    for radius in (0.5, below, float(np.nextafter(0.5, 0))):
        r2 = np.float64(np.float32(radius * radius))
        got = oracle.query_ball_point(radius, 300, p, q)[0]
        for s in range(200):
            hits = np.nonzero(d[s] <= r2)[0]
            want = np.full(300, hits[0] if len(hits) else 300)
            want[: len(hits)] = hits
            assert np.array_equal(got[s], want), (radius, s)
        on_sphere = np.isin(np.arange(6), got[0])
        assert on_sphere.all() if radius != below else not on_sphere.any()
