"""A numpy restatement of the reference's per-frame label synthesis (utils/data.py get_ee_idx, get_ee_cross_section_idx,
get_key_points, get_6_key_points, collect_closest_points; utils/transformation.py compute_dists_to_line,
select_closest_points_to_line), written from the definitions in include/sv_hip.h (block N6), with the operation order
fixed: three-term products and sums as (a + b) + c, norms as sqrt((x^2 + y^2) + z^2).  The pose is float64 (x, y, z, qw, qx,
qy, qz); points are float32 or float64.

dtype rules: ee_idx and the key points are float64 throughout; the cross-section rounds p - pos to the points' dtype
before the float64 rotation; the radius labels run entirely in the points' dtype.

Where the reference fails the restatement does what the HIP entries define: an empty selection of a search means "not
found" (index ignore_label, template coordinates kept); six_key_points with an empty selection returns the template key
points, all ignore_label, and empty = True.
"""
import numpy as np

EE_DIM = {"min_z": -0.006, "max_z": 0.12, "min_x": -0.05, "max_x": 0.05, "min_y": -0.11, "max_y": 0.11}
LP1, LP2 = np.array([-0.05, 0.0, 0.0]), np.array([0.05, 0.0, 0.0])  # get_ee_cross_section_idx's line

KP10 = np.array([[0.02, 0.09, 0], [0.02, -0.09, 0], [0.014, 0.095, 0.07], [0.014, -0.095, 0.07], [0, 0.048, 0.12],
                 [0, -0.048, 0.12], [-0.022, 0.09, 0], [-0.022, -0.09, 0], [-0.014, 0.095, 0.07], [-0.014, -0.095, 0.07]])
KP6 = np.array([[0.02, 0.09, 0], [0.01, -0.1, 0], [0.014, 0.095, 0.07], [0.014, -0.095, 0.07], [0, 0.048, 0.12],
                [0, -0.048, 0.12]])
BBOX6 = np.array([[0.24, 0.32, -0.2], [0.24, -0.32, -0.2], [0.24, 0.32, 0.2], [0.24, -0.32, 0.2]])


def rotation(q):
    """get_quaternion_rotation_matrix, w first"""
    q0, q1, q2, q3 = (float(v) for v in q)
    return np.array([
        [2 * (q0 * q0 + q1 * q1) - 1, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
        [2 * (q1 * q2 + q0 * q3), 2 * (q0 * q0 + q2 * q2) - 1, 2 * (q2 * q3 - q0 * q1)],
        [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), 2 * (q0 * q0 + q3 * q3) - 1],
    ])


def rot_t(R, v):
    """rows of v through R^T"""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    return np.stack([(R[0, c] * v[:, 0] + R[1, c] * v[:, 1]) + R[2, c] * v[:, 2] for c in range(3)], axis=1)


def rot(R, v):
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    return np.stack([(R[c, 0] * v[:, 0] + R[c, 1] * v[:, 1]) + R[c, 2] * v[:, 2] for c in range(3)], axis=1)


def norm3(d):
    d = np.asarray(d)
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def _pose(pose):
    pose = np.asarray(pose, dtype=np.float64)
    return pose[:3], rotation(pose[3:7])


def ee_frame_crop(points, pose):
    pos, R = _pose(pose)
    return rot_t(R, np.asarray(points).astype(np.float64) - pos)


def ee_mask(points, pose, ee_dim=None):
    dim = dict(EE_DIM)
    dim.update(ee_dim or {})
    q = ee_frame_crop(points, pose)
    with np.errstate(invalid="ignore"):
        return ((q[:, 0] > -500) & (q[:, 0] < dim["max_x"]) & (q[:, 0] > dim["min_x"]) & (q[:, 1] < dim["max_y"])
                & (q[:, 1] > dim["min_y"]) & (q[:, 2] < dim["max_z"]) & (q[:, 2] > dim["min_z"]))


def ee_idx(points, pose, ee_dim=None):
    return np.where(ee_mask(points, pose, ee_dim))[0]


def dists_to_line(p, lp1, lp2):
    """compute_dists_to_line with its argument order"""
    a = np.asarray(lp1, dtype=np.float64) - np.asarray(lp2, dtype=np.float64)
    d = a / np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    v = p - lp1
    t = (v[:, 0] * d[0] + v[:, 1] * d[1]) + v[:, 2] * d[2]
    return norm3((lp1 + t[:, None] * d) - p)


def line_frame(points, pose):
    points = np.asarray(points)
    pos, R = _pose(pose)
    return rot_t(R, (points.astype(np.float64) - pos).astype(points.dtype).astype(np.float64))


def cross_section(points, pose, count=32, cutoff=0.004):
    """(dists, idx) of get_ee_cross_section_idx; ties go to the lower index"""
    q = line_frame(points, pose)
    dist = dists_to_line(q, LP2, LP1)  # select_closest_points_to_line hands the two points over swapped
    count = min(count, len(q)) if count > 0 else len(q)
    order = np.argsort(dist, kind="stable")[:count]
    with np.errstate(invalid="ignore"):
        keep = dist[order] < cutoff
    return dist[order][keep], order[keep]


def kp_frame(points, pose):
    """(EE-frame points, offset, R) of the key-point generators"""
    pos, R = _pose(pose)
    off = rot_t(R, pos)[0]
    off = (off + off) / 2
    return rot_t(R, np.asarray(points).astype(np.float64)) - off, off, R


def _closest(target, q, mask):
    """(index in the frame, distance) of the selected row nearest target, numpy's argmin rule; (None, None) when empty"""
    idx = np.where(mask)[0]
    if len(idx) == 0:
        return None, None
    d = norm3(q[idx] - np.asarray(target, dtype=np.float64))
    k = int(np.argmin(d))
    return int(idx[k]), d[k]


def _gripper(q, kp, kidx):
    found = []
    with np.errstate(invalid="ignore"):
        sides = [(q[:, 2] > 0.08) & (q[:, 1] > 0), (q[:, 2] > 0.08) & (q[:, 1] < 0)]
    for g, (mask, y) in enumerate(zip(sides, (0.01, -0.01))):
        if mask.any():
            i, _ = _closest([0.0, y, q[mask, 2].max()], q, mask)
            # the reference's index: the winner's position within the side's subset, looked up among all rows with z > 0.08
            kp[4 + g], kidx[4 + g] = q[i], np.where(q[:, 2] > 0.08)[0][int(mask[:i].sum())]
        found.append(bool(mask.any()))
    if not found[0] and found[1]:
        kp[4] = kp[5] * [1, -1, 1]
    elif found[0] and not found[1]:
        kp[5] = kp[4] * [1, -1, 1]
    kp[4][2] = max(kp[4][2], kp[5][2])
    kp[5][2] = kp[4][2]


def key_points(points, pose, euclidean_threshold=0.018, ignore_label=-100):
    q, off, R = kp_frame(points, pose)
    kp = KP10.copy()
    kidx = np.zeros(10, dtype=np.int64) + ignore_label
    with np.errstate(invalid="ignore"):
        front, back = q[:, 0] > 0.005, q[:, 0] < -0.01
    for s, dx in enumerate((-0.04, -0.04, -0.03, -0.03)):
        i, d = _closest(kp[s], q, front)
        if i is not None and d < euclidean_threshold:
            kp[s], kidx[s] = q[i], i
            kp[6 + s] = q[i] + [dx, 0, 0]
    for s in range(4):
        i, d = _closest(kp[6 + s], q, back)
        if i is not None and d < euclidean_threshold:
            kp[6 + s], kidx[6 + s] = q[i], i
    _gripper(q, kp, kidx)
    return rot(R, kp + off), kidx


def six_key_points(points, pose, euclidean_threshold=0.03, ignore_label=-100):
    """(key points, indices, empty): empty is True where the reference returns two empty arrays"""
    q, off, R = kp_frame(points, pose)
    kp = KP6.copy()
    kidx = np.zeros(6, dtype=np.int64) + ignore_label
    with np.errstate(invalid="ignore"):
        sel = (q[:, 0] > -0.005) & (q[:, 2] < 0.09)
    if not sel.any():
        return rot(R, kp + off), kidx, True
    cand = [_closest(BBOX6[s], q, sel)[0] for s in range(4)]
    close = [norm3(kp[s] - q[cand[s]]) < euclidean_threshold for s in range(4)]
    for s in range(4):
        if close[s]:
            kp[s], kidx[s] = q[cand[s]], cand[s]
    _gripper(q, kp, kidx)
    return rot(R, kp + off), kidx, False


def collect_closest_points(idx, points, euclidean_threshold=0.006):
    """(pcls_idx, p_idx) in np.where's row-major order, computed in the points' dtype"""
    points = np.asarray(points)
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    d = points[idx].reshape(-1, 1, 3) - points
    with np.errstate(invalid="ignore"):
        return np.where(norm3(d) < points.dtype.type(euclidean_threshold))


def radius_labels(points, kp_idx, euclidean_threshold=0.006, ignore_label=-100):
    """the label write of load_key_points: classes of the key points with a non-negative index, the last write wins"""
    points = np.asarray(points)
    kp_idx = np.asarray(kp_idx, dtype=np.int64)
    labels = np.full(len(points), ignore_label, dtype=np.int64)
    real = kp_idx > -1
    classes = np.arange(len(kp_idx), dtype=np.int64)[real]
    pcls, pidx = collect_closest_points(kp_idx[real], points, euclidean_threshold)
    labels[pidx] = classes[pcls]
    return labels


def gripper_cloud(rng, n_body, n_rod=40, n_bg=300, dtype=np.float32):
    """The synthetic gripper of the labels fixture, posed: (points, pose [7] float64 w first, EE-frame points float64).
    Body uniform in x [-.03, .03], y [-.1, .1], z [0, .075]; two fingers x [-.01, .01], |y| [.03, .06], z [.075, .12]; a
    rod within 3 mm of the x axis for |x| < .05; background uniform in +-0.4."""
    body = rng.uniform([-0.03, -0.1, 0.0], [0.03, 0.1, 0.075], size=(n_body, 3))
    nf = max(n_body // 8, 4)
    fingers = rng.uniform([-0.01, 0.03, 0.075], [0.01, 0.06, 0.12], size=(2 * nf, 3))
    fingers[nf:, 1] *= -1
    ang, rad = rng.uniform(0, 2 * np.pi, n_rod), rng.uniform(0, 0.003, n_rod)
    rod = np.stack([rng.uniform(-0.05, 0.05, n_rod), rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    bg = rng.uniform(-0.4, 0.4, size=(n_bg, 3))
    ee = np.concatenate([body, fingers, rod, bg])
    ee = ee[rng.permutation(len(ee))]
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    pos = rng.uniform(-0.5, 0.5, 3)
    pose = np.concatenate([pos, q])
    pts = (rot(rotation(q), ee) + pos).astype(dtype)
    return pts, pose, ee
