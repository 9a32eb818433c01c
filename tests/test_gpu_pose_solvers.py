"""The float64 pose solves (sv_kabsch_batched, sv_quat_avg_batched, sv_add_metric_batched, sv_icp_point2point)
against plain float64 references written from the math: SVD Kabsch with the reflection fix and scipy's
Rotation.align_vectors, scipy's Rotation.from_matrix for the quaternion (signed), numpy's eigh for the quaternion
average, the ADD formula, and an Open3D-style point-to-point ICP loop on scipy's cKDTree.

The shapes are the ones where one-wave-per-problem kernels go wrong: K = 3 (rank-2 H), K and M and P around the 64 lanes,
batch sizes off the 4 problems of a block, NaN padding past the counts, 180 degree rotations (the non-trace branches of
the quaternion extraction), NaN inputs, and for ICP source and target sizes around the 256-thread blocks and the
1024-point LDS tiles of the nearest-neighbour search."""
import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree
from scipy.spatial.transform import Rotation

pytestmark = pytest.mark.gpu

NAN = float("nan")


# ---- float64 references ------------------------------------------------------------------------------------------
def kabsch_ref(a, b):
    """argmin over proper rotations R and t of sum |R a_i + t - b_i|^2, by SVD of H = sum (a - ca)(b - cb)^T with the
    reflection fix; also returns the singular values of H."""
    ca, cb = a.mean(0), b.mean(0)
    H = (a - ca).T @ (b - cb)
    U, s, Vt = np.linalg.svd(H)
    d = -1.0 if np.linalg.det(Vt.T @ U.T) < 0 else 1.0
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, cb - R @ ca, s


def residual(R, t, a, b):
    return float((((a @ R.T + t) - b) ** 2).sum())


def scipy_q_wxyz(R):
    q = Rotation.from_matrix(R).as_quat()  # x, y, z, w
    return np.array([q[3], q[0], q[1], q[2]])


def rot_from_quat(q):
    """utils/transformation.py's get_quaternion_rotation_matrix(switch_w=False); q = (w, x, y, z), not normalised."""
    w, x, y, z = q
    return np.array([
        [2 * (w * w + x * x) - 1, 2 * (x * y - w * z), 2 * (x * z + w * y)],
        [2 * (x * y + w * z), 2 * (w * w + y * y) - 1, 2 * (y * z - w * x)],
        [2 * (x * z - w * y), 2 * (y * z + w * x), 2 * (w * w + z * z) - 1],
    ])


def add_ref(points, gt, pred):
    g = points @ rot_from_quat(gt[3:]).T + gt[:3]
    p = points @ rot_from_quat(pred[3:]).T + pred[:3]
    return float(np.sqrt(((g - p) ** 2).sum(1)).mean())


def icp_ref(src, tgt, init_T, max_distance, max_iterations, rel_fitness, rel_rmse):
    """Open3D's registration_icp point-to-point loop in float64: evaluate, then (while fewer than max_iterations updates
    and at least 3 correspondences) update by Kabsch and re-evaluate, stopping when fitness and inlier rmse both moved
    by less than the tolerances.  Nearest neighbour by cKDTree over the finite target points.  Also returns the
    smallest distance of any stopping decision from its threshold (the float32 kernel must take the same ones)."""
    s = np.asarray(src, np.float64)
    tg = np.asarray(tgt, np.float64)
    keep = np.flatnonzero(np.isfinite(tg).all(1))
    tree = cKDTree(tg[keep])
    T = np.eye(4) if init_T is None else np.array(init_T, np.float64)
    margin = np.inf
    prev, updates = None, 0
    for it in range(max_iterations + 1):
        p = s @ T[:3, :3].T + T[:3, 3]
        ok = np.isfinite(p).all(1)  # a NaN source point has no neighbour
        d, j = np.full(len(p), np.inf), np.zeros(len(p), np.int64)
        d[ok], j[ok] = tree.query(p[ok])
        inl = d <= max_distance
        n = int(inl.sum())
        fitness = n / len(s)
        rmse = float(np.sqrt((d[inl] ** 2).sum() / n)) if n else 0.0
        if prev is not None:
            margin = min(margin, abs(abs(prev[1] - rmse) - rel_rmse))
            if abs(prev[0] - fitness) < rel_fitness and abs(prev[1] - rmse) < rel_rmse:
                break
        prev = (fitness, rmse)
        if n < 3 or it == max_iterations:
            break
        R, t, _ = kabsch_ref(p[inl], tg[keep[j[inl]]])
        U = np.eye(4)
        U[:3, :3], U[:3, 3] = R, t
        T = U @ T
        updates += 1
    return T, fitness, rmse, updates, margin


# ---- Kabsch -------------------------------------------------------------------------------------------------------
def _rotation(rng):
    return Rotation.random(random_state=rng).as_matrix()


def _kabsch_problem(kind, K, rng):
    R = _rotation(rng)
    t = rng.uniform(-1, 1, 3)
    if kind == "offset":  # ~2 m from the origin, ~10 cm spread, and the same on the target side
        a = rng.uniform(-0.05, 0.05, (K, 3)) + np.array([1.2, -0.9, 1.3])
        t = np.array([0.4, 2.1, -0.3]) - R @ a.mean(0)
    else:
        a = rng.uniform(-0.1, 0.1, (K, 3))
    if kind == "coplanar":
        a[:, 2] = 0.25
    b = a @ R.T + t
    if kind == "noise":
        b += rng.normal(0, 1e-3, b.shape)
    if kind == "mirrored":
        b = (a * np.array([1.0, -1.0, 1.0])) @ R.T + t
    return a, b


def _pad(problems, Kmax, fill=NAN):
    B = len(problems)
    ref = np.full((B, Kmax, 3), fill)
    tgt = np.full((B, Kmax, 3), fill)
    K = np.zeros(B, np.int32)
    for i, (a, b) in enumerate(problems):
        K[i] = len(a)
        ref[i, : len(a)] = a
        tgt[i, : len(b)] = b
    return ref, tgt, K


@pytest.mark.parametrize("K", [3, 4, 6, 63, 64, 65, 1000])
@pytest.mark.parametrize("kind", ["random", "coplanar", "mirrored", "noise", "offset"])
def test_kabsch_matches_svd_and_align_vectors(gpu, K, kind):
    from mrcc_amd.utils import transformation as T

    rng = np.random.default_rng(K * 10 + len(kind))
    probs = [_kabsch_problem(kind, K, rng) for _ in range(5)]
    ref, tgt, Ks = _pad(probs, K + 3)  # NaN rows past K must never be read
    R, t, q = T.get_rigid_transform_3D_batched(ref, tgt, Ks, device=gpu)
    for i, (a, b) in enumerate(probs):
        Rr, tr, s = kabsch_ref(a, b)
        assert s[1] / s[0] > 1e-6
        assert np.abs(R[i] - Rr).max() < 1e-9, f"problem {i}: |R - R_svd| = {np.abs(R[i] - Rr).max():.3g}"
        assert np.abs(t[i] - tr).max() < 1e-9, f"problem {i}: |t - t_svd| = {np.abs(t[i] - tr).max():.3g}"
        Ra = Rotation.align_vectors(b - b.mean(0), a - a.mean(0))[0].as_matrix()
        assert np.abs(R[i] - Ra).max() < 1e-9, f"problem {i}: |R - align_vectors| = {np.abs(R[i] - Ra).max():.3g}"
        assert abs(np.linalg.det(R[i]) - 1) < 1e-12
        # the q output is scipy's quaternion of the R output, sign included
        assert np.abs(q[i] - scipy_q_wxyz(R[i])).max() < 1e-12, f"problem {i}: q {q[i]} vs scipy {scipy_q_wxyz(R[i])}"


def _check_optimal(R, t, q, a, b):
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
    assert np.abs(t - (b.mean(0) - R @ a.mean(0))).max() < 1e-12
    Rr, tr, _ = kabsch_ref(a, b)
    assert abs(residual(R, t, a, b) - residual(Rr, tr, a, b)) < 1e-12
    want = scipy_q_wxyz(R)  # R may sit on a branch tie here (axis-aligned lines): q up to sign
    assert min(np.abs(q - want).max(), np.abs(q + want).max()) < 1e-12


def test_kabsch_degenerate_sets_give_an_optimal_rotation(gpu):
    """K = 1 or 2 and exactly collinear points: the rotation is not unique; any proper one reaching the optimum will do."""
    from mrcc_amd.utils import transformation as T

    rng = np.random.default_rng(7)
    R0 = _rotation(rng)
    probs = []
    for K in (1, 2):
        a = rng.uniform(-0.1, 0.1, (K, 3))
        probs.append((a, a @ R0.T + rng.uniform(-1, 1, 3)))
        probs.append((a, rng.uniform(-0.1, 0.1, (K, 3))))  # K = 2 with a different length: residual > 0
    s = np.array([-0.5, -0.25, 0.0, 0.125, 0.75, 1.0])
    line = np.stack([s * 0.1 + 0.3, np.full(6, 0.25), np.full(6, -0.5)], 1)  # exactly collinear along x
    probs.append((line, line @ R0.T + 0.2))
    probs.append((line, line[:, [1, 0, 2]] * 1.1 - 0.05))  # collinear onto another line, with a scale: residual > 0
    probs.append((line, np.stack([s * 0.1, s * -0.07, s * 0.02], 1)))  # both collinear, not axis-aligned
    ref, tgt, K = _pad(probs, 8)
    R, t, q = T.get_rigid_transform_3D_batched(ref, tgt, K, device=gpu)
    for i, (a, b) in enumerate(probs):
        _check_optimal(R[i], t[i], q[i], a, b)


@pytest.mark.parametrize("B", [1, 3, 4, 5, 257])
def test_kabsch_result_independent_of_batch(gpu, B):
    """Each problem's R, t, q bits are those of solving it alone; q_wxyz = NULL changes neither R nor t."""
    from mrcc_amd._lib import call, ptr, stream_ptr
    from mrcc_amd.utils import transformation as T

    rng = np.random.default_rng(B)
    kinds = ["random", "coplanar", "mirrored", "noise", "offset"]
    probs = [_kabsch_problem(kinds[i % 5], int(rng.choice([3, 6, 64, 65])), rng) for i in range(B)]
    ref, tgt, K = _pad(probs, 70)
    R, t, q = T.get_rigid_transform_3D_batched(ref, tgt, K, device=gpu)
    for i in sorted({0, B // 2, B - 1}):
        a, b = probs[i]
        R1, t1, q1 = T.get_rigid_transform_3D_batched(a[None], b[None], device=gpu)
        assert np.array_equal(R1[0], R[i]) and np.array_equal(t1[0], t[i]) and np.array_equal(q1[0], q[i]), i
        Rr, tr, _ = kabsch_ref(a, b)
        assert np.abs(R[i] - Rr).max() < 1e-9 and np.abs(t[i] - tr).max() < 1e-9
    refd, tgtd = torch.from_numpy(ref).to(gpu), torch.from_numpy(tgt).to(gpu)
    Kd = torch.from_numpy(K).to(gpu)
    Rn = torch.full((B, 3, 3), NAN, dtype=torch.float64, device=gpu)
    tn = torch.full((B, 3), NAN, dtype=torch.float64, device=gpu)
    call("sv_kabsch_batched", ptr(refd), ptr(tgtd), ptr(Kd), 70, B, ptr(Rn), ptr(tn), None, stream_ptr())
    assert np.array_equal(Rn.cpu().numpy(), R) and np.array_equal(tn.cpu().numpy(), t)


# ---- rotation -> quaternion ----------------------------------------------------------------------------------------
def _axis_angle(axis, angle):
    axis = np.asarray(axis, np.float64)
    return Rotation.from_rotvec(axis / np.linalg.norm(axis) * angle).as_matrix()


def test_quaternion_from_matrix_signed_as_scipy(gpu):
    """All four branches of the extraction (trace, and the largest diagonal entry x / y / z near 180 degrees) give
    scipy's quaternion with scipy's sign, through get_q_from_matrix and through the q output of Kabsch."""
    from mrcc_amd.utils import transformation as T

    rng = np.random.default_rng(3)
    mats = [np.eye(3)] + [_rotation(rng) for _ in range(40)]
    for axis in np.eye(3):
        for eps in (1e-9, -1e-9, 1e-3):
            mats.append(_axis_angle(axis, np.pi - eps))
        mats.append(_axis_angle(axis + rng.normal(0, 0.05, 3), np.pi - 1e-9))
    branches = set()
    for R in mats:
        want = scipy_q_wxyz(R)
        d = [R[0, 0], R[1, 1], R[2, 2], np.trace(R)]
        branches.add(int(np.argmax(d)))
        got = T.get_q_from_matrix(R)
        assert np.abs(got - want).max() < 1e-12, f"branch {int(np.argmax(d))}: {got} vs scipy {want}"
    assert branches == {0, 1, 2, 3}
    # the same rotations as the Kabsch output of point problems, in one batch of 5-point problems
    a = rng.uniform(-0.1, 0.1, (len(mats), 5, 3))
    b = np.einsum("bij,bkj->bki", np.stack(mats), a) + 0.5
    R, _, q = T.get_rigid_transform_3D_batched(a, b, device=gpu)
    for i in range(len(mats)):
        assert np.abs(q[i] - scipy_q_wxyz(R[i])).max() < 1e-12, i
        assert np.abs(R[i] - mats[i]).max() < 1e-12


def test_quaternion_from_matrix_at_branch_ties(gpu):
    """Exact ties between branches: rounding in R may pick either, so only the quaternion up to sign is pinned."""
    from mrcc_amd.utils import transformation as T

    mats = [_axis_angle([1, 1, 0], np.pi), _axis_angle([0, 1, 1], np.pi), _axis_angle([1, 1, 1], np.pi),
            _axis_angle([1, 1, 1], 2 * np.pi / 3), _axis_angle([1, 0, 1], np.pi)]
    for R in mats:
        want = scipy_q_wxyz(R)
        got = T.get_q_from_matrix(R)
        assert min(np.abs(got - want).max(), np.abs(got + want).max()) < 1e-12, f"{got} vs scipy {want}"
        assert abs(np.linalg.norm(got) - 1) < 1e-12


# ---- quaternion average -------------------------------------------------------------------------------------------
def _avg_ref(Q, w):
    A = (w[:, None, None] * Q[:, :, None] * Q[:, None, :]).sum(0) / w.sum()
    vals, vecs = np.linalg.eigh(A)
    return vecs[:, -1], vals[-1], vals[-1] - vals[-2], A


def _check_avg(out, Q, w, label):
    v, lam, gap, A = _avg_ref(Q, w)
    assert abs(np.linalg.norm(out) - 1) < 1e-12, label
    big = int(np.argmax(np.abs(out)))
    assert out[big] > 0, f"{label}: largest-magnitude component {out} is not positive"
    if gap < 1e-9:
        assert abs(out @ A @ out - lam) < 1e-12, label
        return
    tol = 1e-11 + 1e-14 / gap
    err = min(np.abs(out - v).max(), np.abs(out + v).max())
    assert err < tol, f"{label}: {out} vs eigh {v} (gap {gap:.3g}): {err:.3g}"


def _quats(M, rng, kind):
    if kind == "cluster":  # calibration-like: poses around one orientation, some sign-flipped
        q0 = Rotation.random(random_state=rng).as_quat()
        Q = q0 + rng.normal(0, 0.05, (M, 4))
    else:
        Q = rng.normal(size=(M, 4))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    Q[rng.random(M) < 0.5] *= -1
    return Q[:, [3, 0, 1, 2]]


@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 200])
def test_quaternion_average_matches_eigh(gpu, M):
    from mrcc_amd.utils import calibration as C

    rng = np.random.default_rng(M)
    B, Mmax = 5, M + 2
    Q = np.full((B, Mmax, 4), NAN)
    W = np.full((B, Mmax), NAN)
    cases = []
    for b in range(B):
        q = _quats(M, rng, "cluster" if b % 2 == 0 else "uniform")
        w = rng.uniform(0.1, 2.0, M)
        if b == 3 and M > 1:
            w[rng.random(M) < 0.3] = 0.0
            w[0] = 1.0
        Q[b, :M], W[b, :M] = q, w
        cases.append((q, w))
    out = C.compute_quaternions_weighted_average_batched(Q, W, np.full(B, M, np.int32), device=gpu)
    for b, (q, w) in enumerate(cases):
        _check_avg(out[b], q, w, f"M={M} problem {b}")
    # w = None is the unweighted average; q and -q give the same answer
    Q1 = np.ascontiguousarray(Q[:, :M])
    out1 = C.compute_quaternions_weighted_average_batched(Q1, None, device=gpu)
    for b, (q, _) in enumerate(cases):
        _check_avg(out1[b], q, np.ones(M), f"M={M} problem {b}, w=None")
    flip = np.where(rng.random((B, M, 1)) < 0.5, -1.0, 1.0)
    assert np.array_equal(C.compute_quaternions_weighted_average_batched(Q1 * flip, None, device=gpu), out1)
    # the single-problem API (calibration.compute_poses_average's call)
    one = C.compute_quaternions_weighted_average(cases[0][0], cases[0][1])
    assert np.array_equal(one, out[0])


def test_quaternion_average_without_a_top_gap(gpu):
    """Two orthogonal quaternions with equal weight: a double top eigenvalue; any unit vector of its eigenspace will do."""
    from mrcc_amd.utils import calibration as C

    q = np.array([[0.5, 0.5, 0.5, 0.5], [0.5, -0.5, 0.5, -0.5]])
    for w in (np.ones(2), np.array([0.7, 0.7])):
        out = C.compute_quaternions_weighted_average(q, w)
        _check_avg(out, q, w, f"w={w}")


# ---- ADD ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 63, 64, 65, 5000])
def test_add_matches_float64_formula(gpu, P):
    from mrcc_amd.utils import metrics as Mt

    rng = np.random.default_rng(P)
    B, Pmax = 6, P + 3
    pts = np.full((B, Pmax, 3), NAN)
    Pc = np.full(B, P, np.int32)
    Pc[4] = max(1, P // 2)
    for b in range(B):
        pts[b, : Pc[b]] = rng.uniform(-0.2, 0.2, (Pc[b], 3)) + rng.uniform(-1, 1, 3)
    gt = np.concatenate([rng.uniform(-1, 1, (B, 3)), rng.normal(size=(B, 4))], 1)  # quaternions not normalised
    pred = np.concatenate([rng.uniform(-1, 1, (B, 3)), rng.normal(size=(B, 4)) * rng.uniform(0.5, 2, (B, 1))], 1)
    pred[2] = gt[2]  # identical poses
    add = Mt.compute_ADD_batched(pts, Pc, gt, pred, device=gpu)
    for b in range(B):
        want = add_ref(pts[b, : Pc[b]], gt[b], pred[b])
        assert abs(add[b] - want) <= 1e-12 * want, f"problem {b}: {add[b]!r} vs {want!r}"
    assert add[2] == 0.0
    assert Mt.compute_ADD_np(pts[1, :P], gt[1], pred[1]) == add[1]


# ---- NaN ----------------------------------------------------------------------------------------------------------
def test_kabsch_nan_point_gives_nan_for_its_problem_only(gpu):
    from mrcc_amd.utils import transformation as T

    rng = np.random.default_rng(11)
    probs = [_kabsch_problem("noise", 6, rng) for _ in range(6)]
    ref, tgt, K = _pad(probs, 6)
    R0, t0, q0 = T.get_rigid_transform_3D_batched(ref, tgt, K, device=gpu)
    bad = {1: ("ref", 2, 0, NAN), 2: ("tgt", 5, 2, NAN), 4: ("ref", 0, 1, np.inf), 5: ("tgt", 3, 0, -np.inf)}
    for b, (which, i, d, v) in bad.items():
        (ref if which == "ref" else tgt)[b, i, d] = v
    R, t, q = T.get_rigid_transform_3D_batched(ref, tgt, K, device=gpu)
    for b in range(6):
        if b in bad:
            assert np.isnan(R[b]).all() and np.isnan(t[b]).all() and np.isnan(q[b]).all(), \
                f"problem {b} with {bad[b][3]} in {bad[b][0]}: R {R[b].ravel()}, t {t[b]}, q {q[b]}"
        else:
            assert np.array_equal(R[b], R0[b]) and np.array_equal(t[b], t0[b]) and np.array_equal(q[b], q0[b]), b
    # get_q_from_matrix of a NaN matrix is NaN, not the identity quaternion
    assert np.isnan(T.get_q_from_matrix(np.full((3, 3), NAN))).all()


def test_quaternion_average_nan_and_zero_weights_give_nan(gpu):
    from mrcc_amd.utils import calibration as C

    rng = np.random.default_rng(12)
    B, M = 5, 70
    Q = np.stack([_quats(M, rng, "cluster") for _ in range(B)])
    W = rng.uniform(0.1, 1, (B, M))
    out0 = C.compute_quaternions_weighted_average_batched(Q, W, device=gpu)
    Q[1, 66, 2] = NAN  # in the second lane pass
    W[2] = 0.0
    W[3, 5] = NAN
    out = C.compute_quaternions_weighted_average_batched(Q, W, device=gpu)
    for b in range(B):
        if b in (1, 2, 3):
            assert np.isnan(out[b]).all(), f"problem {b}: {out[b]}"
        else:
            assert np.array_equal(out[b], out0[b]), b


def test_add_nan_point_gives_nan(gpu):
    from mrcc_amd.utils import metrics as Mt

    rng = np.random.default_rng(13)
    pts = rng.uniform(-0.2, 0.2, (3, 100, 3))
    poses = np.concatenate([rng.uniform(-1, 1, (3, 3)), rng.normal(size=(3, 4))], 1)
    add0 = Mt.compute_ADD_batched(pts, None, poses, poses[::-1].copy(), device=gpu)
    pts[1, 77, 1] = NAN
    add = Mt.compute_ADD_batched(pts, None, poses, poses[::-1].copy(), device=gpu)
    assert np.isnan(add[1]) and add[0] == add0[0] and add[2] == add0[2]


# ---- ICP ----------------------------------------------------------------------------------------------------------
def _grid_target(T, rng, centre=(0.05, -0.03, 0.08)):
    """T float32 points at least 6 mm apart: a jittered 8 mm grid (jitter <= 1 mm) around `centre`."""
    n = int(np.ceil(T ** (1 / 3))) + 1
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)
    g = g[rng.permutation(len(g))[:T]]
    p = (g - (n - 1) / 2) * 0.008 + rng.uniform(-0.001, 0.001, (T, 3)) + np.asarray(centre)
    return p.astype(np.float32)


def _icp_case(S, T, seed, identity_init=False, n_far=0):
    """Source points whose true partner is a target point (noise <= 0.5 mm), seen through an initial transform that is
    off by <= 0.8 mm, so every nearest neighbour is the partner by a wide margin in float32 and in float64.  The true
    partners include the last target point (the last, partial LDS tile).  n_far source points have no target within
    max_distance."""
    rng = np.random.default_rng(seed)
    tgt = _grid_target(T, rng)
    part = rng.integers(0, T, S)
    part[-1] = T - 1
    near = tgt[part].astype(np.float64) + rng.uniform(-2.8e-4, 2.8e-4, (S, 3))
    c = tgt.astype(np.float64).mean(0)
    off = np.eye(4)  # rotation of 2 mrad about the target centroid, 0.4 mm translation
    off[:3, :3] = _axis_angle(rng.normal(size=3), 0.002)
    off[:3, 3] = c - off[:3, :3] @ c + rng.normal(size=3) / np.sqrt(3) * 4e-4
    true_T = np.eye(4)
    if not identity_init:
        true_T[:3, :3] = _rotation(rng)
        true_T[:3, 3] = rng.uniform(-0.1, 0.1, 3)
    init = np.linalg.inv(off) @ true_T  # init maps src to `near` moved by off^-1
    src = ((near - true_T[:3, 3]) @ true_T[:3, :3]).astype(np.float32)  # true_T^-1 near
    if n_far:
        src[rng.choice(S - 1, n_far, replace=False)] += np.float32(0.5)
    return src, tgt, (None if identity_init else init)


def _icp_compare(gpu, src, tgt, init, max_distance=0.003, max_iterations=30, rel=1e-6):
    from mrcc_amd.utils import icp as I

    T, fit, rmse, n = I.icp_point2point(src, tgt, init, max_distance, max_iterations, rel, rel, device=gpu)
    Tr, fr, rr, nr, margin = icp_ref(src, tgt, init, max_distance, max_iterations, rel, rel)
    assert margin > 1e-7 or rel == 0, f"case too close to the rmse tolerance ({margin:.3g}) for a float32 comparison"
    assert n == nr, f"updates {n}, reference {nr}"
    assert fit == fr, f"fitness {fit!r}, reference {fr!r}"
    assert abs(rmse - rr) < 1e-7, f"rmse {rmse!r}, reference {rr!r}"
    assert np.abs(T - Tr).max() < 1e-9, f"|T - T_ref| = {np.abs(T - Tr).max():.3g}"
    return T, fit, rmse, n


# S on either side of the update kernels' reduction widths (512 threads point-to-plane, 1024 point-to-point)
ICP_WIDTH_SIZES = [(511, 700), (512, 700), (513, 700), (1023, 700), (1024, 700), (1025, 700)]
# seeds of the width cases, chosen on the CPU: the float64 loop settles in 2 updates at fitness (S - S // 10) / S with a
# stop margin of 1.0e-6 (limit 1e-7) and a nearest / second-nearest gap of 2.8e-5 .. 3.4e-5 m^2; every other size keeps
# S * 7 + T
ICP_SEEDS = {(511, 700): 4277, (512, 700): 4284, (513, 700): 4291, (1023, 700): 7861, (1024, 700): 7868, (1025, 700): 7875}


@pytest.mark.parametrize("S,T", [(3, 2500), (255, 1023), (256, 1024), (257, 1025), (3000, 2500), (3000, 1025),
                                 (255, 2500)] + ICP_WIDTH_SIZES)
def test_icp_matches_float64_open3d_loop(gpu, S, T):
    src, tgt, init = _icp_case(S, T, ICP_SEEDS.get((S, T), S * 7 + T), n_far=S // 10)
    _, fit, _, n = _icp_compare(gpu, src, tgt, init)
    assert fit == (S - S // 10) / S and 1 <= n < 30


@pytest.mark.parametrize("max_iterations", [0, 1, 2, 30])
def test_icp_iteration_counts(gpu, max_iterations):
    src, tgt, init = _icp_case(257, 1025, 5, n_far=20)
    _, _, _, n = _icp_compare(gpu, src, tgt, init, max_iterations=max_iterations)
    assert n <= max_iterations
    # zero tolerances never converge: the run ends at the cap
    _, _, _, n0 = _icp_compare(gpu, src, tgt, init, max_iterations=max_iterations, rel=0.0)
    assert n0 == max_iterations


def test_icp_identity_init(gpu):
    src, tgt, init = _icp_case(1000, 2500, 9, identity_init=True, n_far=3)
    assert init is None
    _icp_compare(gpu, src, tgt, None)


def _edge_both(gpu, oracle, src, tgt, init, max_distance, max_iterations=30):
    from mrcc_amd.utils import icp as I

    got = I.icp_point2point(src, tgt, init, max_distance, max_iterations, device=gpu)
    orc = oracle.icp_point2point(src, tgt, init, max_distance, max_iterations)
    ref = icp_ref(src, tgt, init, max_distance, max_iterations, 1e-6, 1e-6)[:4]
    for name, other in (("oracle", orc), ("float64 reference", ref)):
        assert got[3] == other[3] and got[1] == other[1], f"{name}: updates / fitness {got[1:]} vs {other[1:]}"
        assert abs(got[2] - other[2]) < 1e-7 and np.abs(got[0] - other[0]).max() < 1e-9, name
    return got


def test_icp_without_enough_inliers_returns_init(gpu, oracle):
    rng = np.random.default_rng(21)
    init = np.eye(4)
    init[:3, :3] = _rotation(rng)
    init[:3, 3] = [0.1, -0.2, 0.3]
    src = rng.uniform(-0.1, 0.1, (50, 3)).astype(np.float32)
    p = src.astype(np.float64) @ init[:3, :3].T + init[:3, 3]
    far = (p + 5.0).astype(np.float32)
    for k in (0, 1, 2):  # inliers
        tgt = far.copy()
        tgt[:k] = (p[:k] + 1e-4).astype(np.float32)
        T, fit, rmse, n = _edge_both(gpu, oracle, src, tgt, init, 0.002)
        assert n == 0 and np.array_equal(T, init) and fit == k / 50
        if k == 0:
            assert rmse == 0.0
    # a single target point (T = 1) with two source points near it
    T, fit, rmse, n = _edge_both(gpu, oracle, src, far[:1].copy(), init, 0.002)
    assert n == 0 and fit == 0.0 and np.array_equal(T, init)
    one = (p[:1] + 1e-4).astype(np.float32)
    src2 = src.copy()
    src2[1] = src2[0]
    T, fit, _, n = _edge_both(gpu, oracle, src2, one, init, 0.002)
    assert n == 0 and fit == 2 / 50 and np.array_equal(T, init)


def test_icp_point_at_exactly_max_distance_is_an_inlier(gpu, oracle):
    tgt = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32)
    src = np.array([[0.5, 0, 0], [4, 0.25, 0], [0, 4, 0.25]], np.float32)
    T, fit, rmse, n = _edge_both(gpu, oracle, src, tgt, None, 0.5, max_iterations=0)
    assert fit == 1.0 and rmse == np.sqrt(0.375 / 3) and n == 0
    src[0, 0] = np.nextafter(np.float32(0.5), np.float32(1))
    T, fit, rmse, n = _edge_both(gpu, oracle, src, tgt, None, 0.5, max_iterations=0)
    assert fit == 2 / 3 and n == 0


def test_icp_duplicate_and_nan_targets_change_nothing(gpu, oracle):
    from mrcc_amd.utils import icp as I

    src, tgt, init = _icp_case(300, 1100, 31, n_far=10)
    base = I.icp_point2point(src, tgt, init, 0.003, device=gpu)
    _edge_both(gpu, oracle, src, tgt, init, 0.003)
    rng = np.random.default_rng(32)
    dup = np.concatenate([tgt, tgt[rng.integers(0, len(tgt), 400)]])  # duplicates after their originals ...
    dup2 = np.concatenate([tgt[-50:], tgt])  # ... and before them
    bad = np.array([[NAN, NAN, NAN], [0.05, NAN, 0.08], [np.inf, 0.0, 0.0], [NAN, 0.0, -np.inf]], np.float32)
    nan_t = np.insert(tgt, [0, 500, 1024, len(tgt)], bad, axis=0)  # first row, tile boundary, last row
    for name, t2 in (("duplicates after", dup), ("duplicates before", dup2), ("NaN rows", nan_t)):
        got = I.icp_point2point(src, t2, init, 0.003, device=gpu)
        assert np.array_equal(got[0], base[0]) and got[1:] == base[1:], name
        _edge_both(gpu, oracle, src, t2, init, 0.003)
    # a NaN source point never matches either
    src_n = src.copy()
    src_n[-1] = np.float32(NAN)  # an inlier (the far points are never the last)
    got = _edge_both(gpu, oracle, src_n, tgt, init, 0.003)
    assert round(got[1] * 300) == round(base[1] * 300) - 1
