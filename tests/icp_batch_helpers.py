"""Cases and float64 references of tests/test_gpu_icp_batched.py.

The single-problem constructions (_corner_target, _case) are those of tests/test_gpu_icp_point2plane.py, copied; the
joint reference icp_joint_ref is written from include/sv_hip.h block N3c in the style of that file's icp_plane_ref:
Open3D-style evaluation on scipy's cKDTree per problem, pooled fitness / rmse / stop rule, and one update from the pooled
sums - numpy's SVD (point-to-point) or solve (point-to-plane).  It shares no code with the kernels and reports what a
comparison with a float32 search needs of the case: the smallest gap between the nearest and the second nearest squared
distance over all inliers, the smallest distance of a stop decision from its tolerance, the largest cond(A)."""
import numpy as np
from scipy.spatial import cKDTree
from scipy.spatial.transform import Rotation


def _euler_zyx(a, b, g):
    ca, sa, cb, sb, cg, sg = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(g), np.sin(g)
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _axis_angle(axis, angle):
    return Rotation.from_rotvec(np.asarray(axis, np.float64) / np.linalg.norm(axis) * angle).as_matrix()


def rigid(rng, max_shift):
    """a seeded rigid transform: uniformly random rotation, translation uniform in +-max_shift"""
    T = np.eye(4)
    T[:3, :3] = Rotation.random(random_state=rng).as_matrix()
    T[:3, 3] = rng.uniform(-max_shift, max_shift, 3)
    return T


def apply(T, x):
    return np.asarray(x, np.float64) @ T[:3, :3].T + T[:3, 3]


def pose_of(T):
    """4x4 -> (x, y, z, qw, qx, qy, qz)"""
    q = Rotation.from_matrix(T[:3, :3]).as_quat()  # x, y, z, w
    return np.concatenate([T[:3, 3], [q[3]], q[:3]])


# ---- float64 reference of the shared mode -------------------------------------------------------------------------
def icp_joint_ref(src, tgts, nrms, pre, init_T, max_distance, max_iterations, rel_fitness, rel_rmse):
    """One transform T for all problems: source of problem p = pre[p] . src (src itself with pre None), target tgts[p];
    nrms None = point-to-point, else the targets' normals = point-to-plane.  All inputs finite.
    -> dict(T, fitness, rmse, updates, frame_fitness, frame_rmse, gap, margin, cond)"""
    s = np.asarray(src, np.float64)
    P, S = len(tgts), len(s)
    srcs = [s if pre is None else apply(np.asarray(pre[p], np.float64), s) for p in range(P)]
    tg = [np.asarray(t, np.float64) for t in tgts]
    nr = None if nrms is None else [np.asarray(n, np.float64) for n in nrms]
    trees = [cKDTree(t) for t in tg]
    T = np.eye(4) if init_T is None else np.array(init_T, np.float64)
    gap, margin, cond = np.inf, np.inf, 0.0
    prev, updates = None, 0
    for it in range(max_iterations + 1):
        found = []
        for p in range(P):
            x = apply(T, srcs[p])
            k = min(2, len(tg[p]))
            d, j = trees[p].query(x, k=k)
            d, j = d.reshape(-1, k), j.reshape(-1, k)
            inl = d[:, 0] <= max_distance
            if inl.any() and k == 2:
                gap = min(gap, float((d[inl, 1] ** 2 - d[inl, 0] ** 2).min()))
            found.append((x[inl], j[inl, 0], d[inl, 0]))
        counts = np.array([len(x) for x, _, _ in found])
        errs = np.array([(d ** 2).sum() for _, _, d in found])
        n = int(counts.sum())
        fitness = n / (P * S)
        rmse = float(np.sqrt(errs.sum() / n)) if n else 0.0
        frame_fitness = counts / S
        frame_rmse = np.array([np.sqrt(e / c) if c else 0.0 for e, c in zip(errs, counts)])
        if prev is not None:
            margin = min(margin, abs(abs(prev[0] - fitness) - rel_fitness), abs(abs(prev[1] - rmse) - rel_rmse))
            if abs(prev[0] - fitness) < rel_fitness and abs(prev[1] - rmse) < rel_rmse:
                break
        prev = (fitness, rmse)
        if it == max_iterations:
            break
        x = np.concatenate([x for x, _, _ in found])
        q = np.concatenate([tg[p][j] for p, (_, j, _) in enumerate(found)])
        U = np.eye(4)
        if nr is None:
            if n < 3:
                break
            cx, cq = x.mean(0), q.mean(0)
            H = (x - cx).T @ (q - cq)
            u, _, vt = np.linalg.svd(H)
            R = vt.T @ u.T
            if np.linalg.det(R) < 0:
                vt[2] *= -1
                R = vt.T @ u.T
            U[:3, :3], U[:3, 3] = R, cq - R @ cx
        else:
            m = np.concatenate([nr[p][j] for p, (_, j, _) in enumerate(found)])
            if len(m) < 6:
                break
            r = ((x - q) * m).sum(1)
            J = np.concatenate([np.cross(x, m), m], 1)
            A, b = J.T @ J, J.T @ r
            try:
                np.linalg.cholesky(A)
            except np.linalg.LinAlgError:  # not positive definite: no update
                break
            cond = max(cond, float(np.linalg.cond(A)))
            sol = np.linalg.solve(A, -b)
            U[:3, :3], U[:3, 3] = _euler_zyx(*sol[:3]), sol[3:]
        T = U @ T
        updates += 1
    return dict(T=T, fitness=fitness, rmse=rmse, updates=updates, frame_fitness=frame_fitness, frame_rmse=frame_rmse,
                gap=gap, margin=margin, cond=cond)


# ---- single-problem cases (tests/test_gpu_icp_point2plane.py) -----------------------------------------------------
def _corner_target(T, rng, centre=(0.05, -0.03, 0.08)):
    """T float32 points on the three faces of a box corner at `centre`, each face bumped by 1.5 mm (a product of sines of
    10 cm period), and their analytic unit normals.  In a face the points are a jittered 8 mm grid (jitter <= 1 mm) that
    starts 7 mm from the edges, so any two points are at least 6 mm apart."""
    n = int(np.ceil(np.sqrt(T / 3))) + 1
    g = np.stack(np.meshgrid(np.arange(3), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3)
    g = g[rng.permutation(len(g))[:T]]
    face = g[:, 0]
    uv = 0.007 + g[:, 1:] * 0.008 + rng.uniform(-0.001, 0.001, (T, 2))
    pts, nrm = corner_surface(face, uv)
    return (pts + np.asarray(centre)).astype(np.float32), nrm.astype(np.float32)


def corner_surface(face, uv):
    """the bumped box corner of _corner_target as a function: face index [N] and in-face coordinates [N,2] -> float64
    points [N,3] (corner at the origin) and analytic unit normals"""
    N = len(face)
    amp, k = 0.0015, 2 * np.pi / 0.1
    phase = face * 0.7
    h = amp * np.sin(k * uv[:, 0] + phase) * np.sin(k * uv[:, 1])
    hu = amp * k * np.cos(k * uv[:, 0] + phase) * np.sin(k * uv[:, 1])
    hv = amp * k * np.sin(k * uv[:, 0] + phase) * np.cos(k * uv[:, 1])
    pts, nrm = np.zeros((N, 3)), np.zeros((N, 3))
    rows = np.arange(N)
    a, b, c = face, (face + 1) % 3, (face + 2) % 3  # the face's normal axis and its two in-plane axes
    pts[rows, a], pts[rows, b], pts[rows, c] = h, uv[:, 0], uv[:, 1]
    nrm[rows, a], nrm[rows, b], nrm[rows, c] = 1.0, -hu, -hv
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return pts, nrm


def _case(S, T, seed, identity_init=False, n_far=0):
    """As the point-to-point cases: every source point has a true partner among the targets (noise <= 0.28 mm), the initial
    transform is off by 2 mrad about the target centroid and 0.4 mm, the partners include the last target point (the last,
    partial LDS tile), n_far source points have no target within max_distance."""
    rng = np.random.default_rng(seed)
    tgt, nrm = _corner_target(T, rng)
    part = rng.integers(0, T, S)
    part[-1] = T - 1
    near = tgt[part].astype(np.float64) + rng.uniform(-2.8e-4, 2.8e-4, (S, 3))
    c = tgt.astype(np.float64).mean(0)
    off = np.eye(4)
    off[:3, :3] = _axis_angle(rng.normal(size=3), 0.002)
    off[:3, 3] = c - off[:3, :3] @ c + rng.normal(size=3) / np.sqrt(3) * 4e-4
    true_T = np.eye(4)
    if not identity_init:
        true_T[:3, :3] = Rotation.random(random_state=rng).as_matrix()
        true_T[:3, 3] = rng.uniform(-0.1, 0.1, 3)
    init = np.linalg.inv(off) @ true_T
    src = ((near - true_T[:3, 3]) @ true_T[:3, :3]).astype(np.float32)
    if n_far:
        src[rng.choice(S - 1, n_far, replace=False)] += np.float32(0.5)
    return src, tgt, nrm, (None if identity_init else init)


INDEPENDENT_MAX_DISTANCE = 0.01


def problem(src, init, T, kind, seed):
    """One problem of an independent batch on the source cloud and initial transform of a _case: a target of T points and
    an initial transform of its own.  The target is the source under init moved by a small rigid offset, subsampled (T <= S)
    or padded with rows 3 m away (T > S, shuffled, so that real points lie on both sides of every tile edge), plus 0.28 mm
    of noise; its normals are random unit vectors - the comparison is with the single CALL on the same inputs, not with a
    model of a surface.  kind: "near" (offset 2 mrad / 0.4 mm: converges in a few updates), "slow" (0.1 rad / 15 mm with
    INDEPENDENT_MAX_DISTANCE 10 mm: the inlier set keeps changing), "far" (target 7 m away and an unrelated initial
    transform: zero inliers), "flat" (near, all normals (0, 0, 1): no point-to-plane update).
    -> tgt, nrm float32 [T,3], init float64 [4,4]"""
    rng = np.random.default_rng(seed)
    S = len(src)
    slow = kind == "slow"
    off = np.eye(4)
    off[:3, :3] = _axis_angle(rng.normal(size=3), 0.1 if slow else 0.002)
    off[:3, 3] = rng.normal(size=3) * (0.015 if slow else 4e-4)
    x = apply(off @ init, src.astype(np.float64))
    rows = rng.permutation(S)[:T] if T <= S else np.concatenate([np.arange(S), rng.integers(0, S, T - S)])
    t = x[rows] + rng.uniform(-2.8e-4, 2.8e-4, (T, 3))
    if T > S:
        t[S:] += 3.0
        t = t[rng.permutation(T)]
    if kind == "far":
        t += 7.0
    n = rng.normal(size=(T, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    if kind == "flat":
        n[:] = [0.0, 0.0, 1.0]
    return t.astype(np.float32), n.astype(np.float32), (rigid(rng, 0.1) if kind == "far" else np.array(init))


# ---- shared-mode cases --------------------------------------------------------------------------------------------
def joint_case(S, sizes, seed):
    """One model, P = len(sizes) frames: the model is a _corner_target of max(sizes) points (>= 6 mm apart) with its
    normals; the source holds S points within 0.28 mm of model points; frame p's target is true_T . pre[p] applied to the
    first sizes[p] model points of a per-frame shuffle, with the rotated normals, so source points whose partner the frame
    lacks are out of reach at max_distance 3 mm.  init is off true_T by 2 mrad about the targets' centroid and 0.4 mm.
    -> src, tgts, nrms, pre [P,4,4], init, true_T"""
    rng = np.random.default_rng(seed)
    N = max(sizes)
    model, normals = _corner_target(N, rng, centre=(0.0, 0.0, 0.0))
    model, normals = model.astype(np.float64), normals.astype(np.float64)
    part = rng.integers(0, N, S)
    src = (model[part] + rng.uniform(-2.8e-4, 2.8e-4, (S, 3))).astype(np.float32)
    true_T = rigid(rng, 0.1)
    pre = np.stack([rigid(rng, 0.3) for _ in sizes])
    tgts, nrms = [], []
    for p, T in enumerate(sizes):
        rows = rng.permutation(N)[:T]
        M = true_T @ pre[p]
        tgts.append(apply(M, model[rows]).astype(np.float32))
        nrms.append((normals[rows] @ M[:3, :3].T).astype(np.float32))
    c = np.concatenate(tgts).astype(np.float64).mean(0)
    off = np.eye(4)
    off[:3, :3] = _axis_angle(rng.normal(size=3), 0.002)
    off[:3, 3] = c - off[:3, :3] @ c + rng.normal(size=3) / np.sqrt(3) * 4e-4
    return src, tgts, nrms, pre, np.linalg.inv(off) @ true_T, true_T


# the faces of the recovery model differ in size, so no rotation maps the model onto itself
RECOVERY_EXTENT = np.array([[0.25, 0.25], [0.25, 0.15], [0.15, 0.20]])
RECOVERY_MAX_DISTANCE = 0.02


def recovery_case(seed, M=5, S=1500, noise=5e-4, shift=0.005, angle=np.deg2rad(2.0)):
    """The calibration problem in small: an asymmetric S-point model (the bumped box corner with faces of three different
    sizes, points uniform on the faces), M one-sided views of it.  View i sees the model at true_T . pre[i] and only the
    faces turned towards a seeded direction (at least one, at most two); its crop samples them on a 60 mm grid that starts 45 mm
    from the face's edges (so points of two faces are no closer than points of one), jittered by 2 mm, with Gaussian noise of `noise` per coordinate, and carries the analytic normals.  Crop points are therefore more
    than 50 mm apart, 2.5 times RECOVERY_MAX_DISTANCE: an inlier's nearest crop point is unique by more than
    0.03^2 - 0.02^2 = 5e-4 m^2, which a float32 search cannot confuse.  The start is true_T moved by `shift` in a random
    direction and rotated by `angle` about the crops' centroid; the end effector poses pre[i] lie within 0.1 m of the
    origin per axis, so the misalignment stays below 5 mm + 0.035 * 0.35 m = 17 mm, inside max_distance.
    -> src, tgts, nrms, pre [M,4,4], init, true_T"""
    rng = np.random.default_rng(seed)
    face = rng.choice(3, S, p=RECOVERY_EXTENT.prod(1) / RECOVERY_EXTENT.prod(1).sum())
    model, _ = corner_surface(face, rng.uniform(0.0, 1.0, (S, 2)) * RECOVERY_EXTENT[face])
    src = model.astype(np.float32)
    true_T = rigid(rng, 0.1)
    pre = np.stack([rigid(rng, 0.1) for _ in range(M)])
    tgts, nrms = [], []
    for i in range(M):
        view = rng.normal(size=3)
        seen = np.argsort(-view)[:rng.integers(1, 3)]  # the one or two faces turned most towards the view direction
        f, uv = [], []
        for a in seen:
            gu, gv = (np.arange(0.045, e - 0.01, 0.06) for e in RECOVERY_EXTENT[a])
            g = np.stack(np.meshgrid(gu, gv, indexing="ij"), -1).reshape(-1, 2)
            f.append(np.full(len(g), a))
            uv.append(g + rng.uniform(-0.002, 0.002, g.shape))
        pts, nrm = corner_surface(np.concatenate(f), np.concatenate(uv))
        Mi = true_T @ pre[i]
        tgts.append((apply(Mi, pts) + rng.normal(size=pts.shape) * noise).astype(np.float32))
        nrms.append((nrm @ Mi[:3, :3].T).astype(np.float32))
    c = np.concatenate(tgts).astype(np.float64).mean(0)
    off = np.eye(4)
    off[:3, :3] = _axis_angle(rng.normal(size=3), angle)
    d = rng.normal(size=3)
    off[:3, 3] = c - off[:3, :3] @ c + d / np.linalg.norm(d) * shift
    return src, tgts, nrms, pre, off @ true_T, true_T


def pose_error(T, true_T):
    """-> (translation error in m, rotation error in degrees) of T against true_T"""
    D = np.linalg.inv(true_T) @ T
    return float(np.linalg.norm(T[:3, 3] - true_T[:3, 3])), float(np.rad2deg(np.linalg.norm(
        Rotation.from_matrix(D[:3, :3]).as_rotvec())))
