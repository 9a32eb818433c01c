"""Generate tests/golden/*.npz by running the REFERENCE's own functions (imported from /root/reference) on seeded inputs.

Runs only in the build container (the reference never travels to the GPU box); the fixtures it writes are data:
inputs and the reference's outputs.  Two dev-only imports the reference drags in are satisfied with empty modules:
`ipdb` (utils/transformation.py:4, a debugger that is never called) and `turtle` (utils/calibration.py:1, an unused
`from turtle import pos`).  The reference's utils/output.py does `import MinkowskiEngine as ME` (for a type annotation):
MinkowskiEngine is not installable here, so this build's own ME-shaped namespace is registered under that name
(mrcc_amd.install_as_minkowski_engine() - the drop-in boundary doing its job); the two functions taken from that file,
get_pred_center and get_key_point_predictions, are pure torch/numpy and never touch ME.

    python tools/make_golden.py          # rewrites tests/golden/{kabsch,quat_avg,add,fps,ball_query,preprocess}.npz
    python tools/make_golden.py pointnet2_msg    # only the named fixtures

`pose_losses` imports the reference's utils/loss.py with `utils.config` replaced by a stub (_StubConfig) that carries the
keys the criteria read: the real module parses sys.argv and creates directories when it is imported.  `augmentation`
imports the reference's utils/augmentation.py with an empty `open3d` module beside the `ipdb` one (only
change_background, which is not recorded, uses it).  `labels` runs the reference's utils/data.py with `np.int = int` set
for the call (get_6_key_points uses the alias numpy removed).
"""
import os
import sys
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")

sys.modules.setdefault("ipdb", types.ModuleType("ipdb"))
_turtle = types.ModuleType("turtle")
_turtle.pos = None
sys.modules.setdefault("turtle", _turtle)
sys.path.insert(0, REF)

sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mrcc_amd  # noqa: E402

mrcc_amd.install_as_minkowski_engine()

from utils import transformation as T  # noqa: E402
from utils import output as Out  # noqa: E402
from utils import calibration as Cal  # noqa: E402
from utils import metrics as Mx  # noqa: E402
from utils import preprocess as Pre  # noqa: E402
from utils import data as Dat  # noqa: E402
import torch  # noqa: E402
from model import pointnet2_utils as P2  # noqa: E402

def read_reference_key_points():
    import re

    src = open(os.path.join(REF, "app", "inference_engine.py")).read()
    m = re.search(r"self\.reference_key_points\s*=\s*np\.array\(\s*\[(.*?)\]\s*,?\s*(dtype=[^)]*)?\)", src, re.S)
    rows = re.findall(r"\[\s*([-\d.eE+]+)\s*,\s*([-\d.eE+]+)\s*,\s*([-\d.eE+]+)\s*\]", m.group(1))
    return np.array(rows, dtype=np.float64)


def rand_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def gen_kabsch(rng):
    kp = read_reference_key_points()
    B, Kmax = 256, 6
    ref = np.zeros((B, Kmax, 3))
    tgt = np.zeros((B, Kmax, 3))
    K = np.zeros(B, dtype=np.int32)
    R = np.zeros((B, 3, 3))
    t = np.zeros((B, 3))
    q = np.zeros((B, 4))
    kind = np.zeros(B, dtype=np.int32)
    for b in range(B):
        k = int(rng.integers(4, 7))
        cls = np.sort(rng.choice(6, size=k, replace=False))
        a = kp[cls].copy()
        mode = b % 8
        Rgt = T.get_quaternion_rotation_matrix(rand_quat(rng), switch_w=False)
        tgt_pts = (Rgt @ a.T).T + rng.uniform(-1, 1, size=3)
        if mode == 1:  # noisy key points (1 mm)
            tgt_pts += rng.normal(0, 1e-3, size=tgt_pts.shape)
        elif mode == 2:  # heavy noise (2 cm)
            tgt_pts += rng.normal(0, 2e-2, size=tgt_pts.shape)
        elif mode == 3:  # mirrored target -> the SVD solution is a reflection, fixed by Vt[2] *= -1
            tgt_pts = tgt_pts * np.array([1.0, 1.0, -1.0]) + rng.normal(0, 1e-3, size=tgt_pts.shape)
        elif mode == 4:  # random (non key-point) reference sets
            a = rng.uniform(-0.2, 0.2, size=(k, 3))
            tgt_pts = (Rgt @ a.T).T + rng.uniform(-1, 1, size=3) + rng.normal(0, 1e-3, size=(k, 3))
        elif mode == 5:  # coplanar reference (z = 0) with noise on the target
            a = rng.uniform(-0.2, 0.2, size=(k, 3))
            a[:, 2] = 0.0
            tgt_pts = (Rgt @ a.T).T + rng.normal(0, 1e-3, size=(k, 3))
        elif mode == 6:  # large offsets (metres), tiny object
            a = a + 3.0
            tgt_pts = (Rgt @ a.T).T + 5.0
        Rr, tr = T.get_rigid_transform_3D(a, tgt_pts)
        qr = T.get_q_from_matrix(Rr)
        ref[b, :k], tgt[b, :k], K[b] = a, tgt_pts, k
        R[b], t[b], q[b], kind[b] = Rr, tr, qr, mode
    return dict(ref=ref, tgt=tgt, K=K, R=R, t=t, q=q, kind=kind, reference_key_points=kp)


def gen_quat_avg(rng):
    B, Mmax = 64, 20
    Q = np.zeros((B, Mmax, 4))
    W = np.zeros((B, Mmax))
    M = np.zeros(B, dtype=np.int32)
    out = np.zeros((B, 4))
    poses = np.zeros((B, Mmax, 7))
    pose_avg = np.zeros((B, 7))
    for b in range(B):
        m = int(rng.integers(2, Mmax + 1))
        base = rand_quat(rng)
        for i in range(m):
            qi = base + rng.normal(0, 0.05 if b % 2 else 0.3, size=4)
            qi /= np.linalg.norm(qi)
            if rng.random() < 0.3:
                qi = -qi
            Q[b, i] = qi
        W[b, :m] = rng.uniform(0.1, 1.0, size=m) if b % 3 else 1.0
        M[b] = m
        out[b] = Cal.compute_quaternions_weighted_average(Q[b, :m], W[b, :m])
        poses[b, :m, :3] = rng.uniform(-1, 1, size=(m, 3))
        poses[b, :m, 3:] = Q[b, :m]
        pose_avg[b] = Cal.compute_poses_average(poses[b, :m], W[b, :m])
    return dict(Q=Q, W=W, M=M, out=out, poses=poses, pose_avg=pose_avg)


def gen_add(rng):
    B, Pmax = 32, 512
    pts = np.zeros((B, Pmax, 3))
    P = np.zeros(B, dtype=np.int32)
    gt = np.zeros((B, 7))
    pr = np.zeros((B, 7))
    add = np.zeros(B)
    for b in range(B):
        p = int(rng.integers(16, Pmax + 1))
        pts[b, :p] = rng.uniform(-0.1, 0.1, size=(p, 3))
        gt[b, :3] = rng.uniform(-1, 1, size=3)
        gt[b, 3:] = rand_quat(rng)
        pr[b, :3] = gt[b, :3] + rng.normal(0, 0.01, size=3)
        qn = gt[b, 3:] + rng.normal(0, 0.02, size=4)
        pr[b, 3:] = qn / np.linalg.norm(qn)
        P[b] = p
        add[b] = Mx.compute_ADD_np(pts[b, :p], gt[b], pr[b])
    return dict(points=pts, P=P, gt=gt, pred=pr, add=add)


def gen_fps(rng):
    # numpy FPS (utils/data.py:13-34) on an EE-crop-like cloud; the random first index is recovered from the output
    n_np, s_np = 4096, 2048
    cloud = (rng.uniform(-0.5, 0.5, size=(n_np, 3)) * np.array([0.10, 0.22, 0.13])).astype(np.float32)
    np.random.seed(7)
    idx_np = Dat.get_farthest_point_sample_idx(cloud, s_np)
    # torch FPS (model/pointnet2_utils.py:65-86), batch of 3 clouds
    B, N, S = 3, 1024, 256
    xyz = rng.uniform(-1, 1, size=(B, N, 3)).astype(np.float32)
    torch.manual_seed(11)
    idx_t = P2.farthest_point_sample(torch.from_numpy(xyz), S).numpy()
    return dict(np_cloud=cloud, np_idx=idx_np.astype(np.int64), np_start=np.int64(idx_np[0]), t_xyz=xyz,
                t_idx=idx_t.astype(np.int64), t_start=idx_t[:, 0].astype(np.int64))


def gen_ball_query(rng):
    B, N, S, nsample, radius = 2, 1024, 128, 32, 0.2
    xyz = rng.uniform(-1, 1, size=(B, N, 3)).astype(np.float32)
    torch.manual_seed(3)
    t = torch.from_numpy(xyz)
    fps = P2.farthest_point_sample(t, S)
    new_xyz = P2.index_points(t, fps)
    idx = P2.query_ball_point(radius, nsample, t, new_xyz).numpy()
    # margin of every point to the ball surface, so a test can skip borderline points (matmul rounding is unspecified)
    d = P2.square_distance(new_xyz, t).numpy()
    return dict(xyz=xyz, new_xyz=new_xyz.numpy(), idx=idx.astype(np.int64), radius=np.float64(radius),
                nsample=np.int64(nsample), min_margin=np.float64(np.abs(d - np.float32(radius ** 2)).min()))


def gen_metrics(rng):
    n, B = 4000, 12
    gts = rng.integers(0, 3, size=(B, n))
    preds = gts.copy()
    acc = np.zeros(B); prec = np.zeros(B); rec = np.zeros(B); cls = np.zeros((B, 3, 3))
    for b in range(B):
        flip = rng.random(n) < (0.02 * b)
        preds[b, flip] = rng.integers(0, 3, size=flip.sum())
        if b == 3:
            preds[b, preds[b] == 2] = 1  # a class that is never predicted
        if b == 5:
            gts[b, gts[b] == 0] = 1  # a class absent from the ground truth
        r = Mx.compute_segmentation_metrics(gts[b], preds[b])
        acc[b], prec[b], rec[b] = r["accuracy"], r["precision"], r["recall"]
        for ci, cn in enumerate(["background", "arm", "ee"]):
            c = r["class_results"][cn]
            cls[b, ci] = [c["accuracy"], float(c["precision"]), float(c["recall"])]
    P = 64
    gt_pose = np.zeros((P, 7)); pr_pose = np.zeros((P, 7)); dpos = np.zeros(P); dang = np.zeros(P)
    for i in range(P):
        gt_pose[i, :3] = rng.uniform(-1, 1, 3); gt_pose[i, 3:] = rand_quat(rng)
        pr_pose[i, :3] = gt_pose[i, :3] + rng.normal(0, 0.05, 3)
        q = gt_pose[i, 3:] + rng.normal(0, 0.1 * (1 + i % 5), 4)
        pr_pose[i, 3:] = (q / np.linalg.norm(q)) * (1 if i % 2 else -1) * (1.0 if i % 3 else 2.5)  # sign / scale
        r = Mx.compute_pose_metrics(gt_pose[i], pr_pose[i])
        dpos[i], dang[i] = r["dist_position"], r["angle_diff"]
    kp_gt = rng.uniform(-0.1, 0.1, size=(6, 3)); kp_cls = np.array([0, 2, 3, 5]); kp_pred = kp_gt[kp_cls] + rng.normal(0, 0.01, (4, 3))
    return dict(seg_gt=gts, seg_pred=preds, seg_accuracy=acc, seg_precision=prec, seg_recall=rec, seg_class=cls,
                gt_pose=gt_pose, pred_pose=pr_pose, dist_position=dpos, angle_diff=dang, kp_gt=kp_gt, kp_cls=kp_cls,
                kp_pred=kp_pred, kp_error=np.float64(Mx.compute_kp_error(kp_gt, kp_pred, kp_cls)))


def gen_preprocess(rng):
    pts = rng.normal(size=(1000, 3)).astype(np.float32)
    centred, off = Pre.center_at_origin(pts)
    rgb255 = rng.integers(0, 256, size=(500, 3)).astype(np.float32)
    rgb01 = rng.uniform(0, 1, size=(500, 3)).astype(np.float32)
    return dict(points=pts, centred=centred, offset=off, rgb255=rgb255, rgb255_out=Pre.normalize_colors(rgb255),
                rgb01=rgb01, rgb01_out=Pre.normalize_colors(rgb01), norm_points=Pre.normalize_points(pts))


def gen_calib_chain(rng):
    """utils/transformation.py:225-266 (get_base2cam_pose, transform_pose2pose), :63-101 (matrix <-> pose helpers):
    the chain InferenceEngine.calibrate runs per frame (app/inference_engine.py:152-244)."""
    B = 48
    ee2cam = np.zeros((B, 7)); ee2robot = np.zeros((B, 7)); base2cam = np.zeros((B, 7)); p2p = np.zeros((B, 7))
    mat = np.zeros((B, 4, 4)); mat_inv = np.zeros((B, 4, 4)); pose_back = np.zeros((B, 7))
    for b in range(B):
        ee2cam[b, :3] = rng.uniform(-1, 1, 3); ee2cam[b, 3:] = rand_quat(rng)
        ee2robot[b, :3] = rng.uniform(-1, 1, 3); ee2robot[b, 3:] = rand_quat(rng)
        if b % 5 == 0:  # near-180-degree rotations exercise every branch of the matrix -> quaternion conversion
            ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
            ang = np.pi - 1e-3 * (b // 5)
            ee2cam[b, 3:] = np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * ax])
        base2cam[b] = T.get_base2cam_pose(ee2cam[b], ee2robot[b])
        p2p[b] = T.transform_pose2pose(ee2cam[b], ee2robot[b])
        mat[b] = T.get_transformation_matrix(ee2cam[b], switch_w=False)
        mat_inv[b] = T.get_transformation_matrix_inverse(mat[b])
        pose_back[b] = T.get_pose_from_matrix(mat[b])
    return dict(ee2cam=ee2cam, ee2robot=ee2robot, base2cam=base2cam, pose2pose=p2p, matrix=mat, matrix_inverse=mat_inv,
                pose_from_matrix=pose_back)


def gen_output_ops(rng):
    """utils/output.py:45-64 get_pred_center (top-8 vote mean, optional quaternion offset) and :81-87
    get_key_point_predictions (softmax over classes, max over points per class, threshold)."""
    n = 3000
    votes = rng.normal(size=(n, 2)).astype(np.float32)
    coords = rng.uniform(-0.5, 0.5, size=(n, 3)).astype(np.float32)
    centre = Out.get_pred_center(torch.from_numpy(votes), coords)
    q = rand_quat(rng).astype(np.float32)
    centre_q = Out.get_pred_center(torch.from_numpy(votes), coords.copy(), ee_r=0.03, q=q)
    m = 2500
    logits = (rng.normal(size=(m, 6)) * 2).astype(np.float32)
    for c, row in zip((0, 2, 3, 5), (17, 400, 1234, 2499)):  # four confident key points, two classes left uncertain
        logits[row, c] += 25.0
    idx, classes, probs = Out.get_key_point_predictions(torch.from_numpy(logits))
    idx9, classes9, probs9 = Out.get_key_point_predictions(torch.from_numpy(logits), conf_th=0.5)
    seg_logits = rng.normal(size=(2000, 3)).astype(np.float32)

    class _Field:
        features = torch.from_numpy(seg_logits)

    preds, conf = Out.get_segmentations_from_tensor_field(_Field())
    return dict(votes=votes, coords=coords, centre=np.asarray(centre, np.float64), q=q,
                centre_q=np.asarray(centre_q, np.float64), kp_logits=logits, kp_idx=np.asarray(idx, np.int64),
                kp_classes=np.asarray(classes, np.int64), kp_probs=np.asarray(probs, np.float32),
                kp_idx_th05=np.asarray(idx9, np.int64), kp_classes_th05=np.asarray(classes9, np.int64),
                kp_probs_th05=np.asarray(probs9, np.float32), seg_logits=seg_logits, seg_preds=preds.astype(np.int64),
                seg_conf=conf.astype(np.float32))


def _pointnet2_weights(sd, seed):
    """the fixture's weight recipe (tests/test_gpu_pointnet2.py restates it): every state_dict tensor except
    num_batches_tracked, in sorted-key order, from np.random.default_rng(seed) - conv weights N(0, 1/fan_in), conv biases
    and BatchNorm biases N(0, 0.1^2), BatchNorm weights U(0.75, 1.25), running means N(0, 0.1^2), running variances
    U(0.5, 1.5), the other conv weights N(0, 1.44/fan_in) but the head's conv1 / conv2 weights N(0, 9/fan_in); float32.  Returns (values, SHA-256 of the concatenated
    float32 bytes)."""
    import hashlib

    rng = np.random.default_rng(seed)
    vals = {}
    for k in sorted(sd):
        if k.endswith("num_batches_tracked"):
            continue
        shape = tuple(sd[k].shape)
        if k.endswith("running_var"):
            v = rng.uniform(0.5, 1.5, shape)
        elif k.endswith("running_mean"):
            v = rng.standard_normal(shape) * 0.1
        elif "bns" in k or k.startswith("bn"):
            v = rng.uniform(0.75, 1.25, shape) if k.endswith("weight") else rng.standard_normal(shape) * 0.1
        elif k.endswith("weight"):
            gain = 3.0 if k.startswith("conv") else 1.2
            v = rng.standard_normal(shape) * gain / np.sqrt(int(np.prod(shape[1:])))
        else:
            v = rng.standard_normal(shape) * 0.1
        vals[k] = v.astype(np.float32)
    blob = b"".join(vals[k].tobytes() for k in sorted(vals))
    return vals, hashlib.sha256(blob).hexdigest()


def gen_pointnet2(rng):
    """model/pointnet2.py:9-43 PointNet2SSG(num_classes=6, in_channels=6), eval, CPU, with the seeded weights of
    _pointnet2_weights (not stored: the test regenerates them and checks the hash) on three seeded inputs [B, 6, 2048];
    every FPS start the reference draws (torch.randint, model/pointnet2_utils.py:77) recorded as starts [4, B]; outputs
    logits [B, 2048, 6], l4_points and utils/output.py:81-87 get_key_point_predictions at conf_th = 0.75.
    With random statistics every BatchNorm leaves the head's input nearly the same at every point (the logits' spread over
    the points would be ~1e-3, key-point probabilities ~1/6, nothing selected); so bn1's running statistics are set to
    the per-channel mean / variance of conv1's output on a seeded calibration batch (stored: bn1_running_mean / _var), and
    the logits vary by ~1 over the points.  Inputs span [-1, 1] (xyz) and [-3, 3] (features): with end-effector-sized
    clouds the per-point part of the features is small against the BatchNorm shifts, and the calibrated bn1 would magnify
    plain fp32 rounding of the stages before it."""
    from model.pointnet2 import PointNet2SSG as RefSSG

    def cloud(B):
        xyz = rng.uniform(-1.0, 1.0, size=(B, 3, 2048)) * [[[1.0], [0.6], [1.2]]]
        feat = rng.uniform(-3.0, 3.0, size=(B, 3, 2048))
        return np.concatenate([xyz, feat], axis=1).astype(np.float32)

    seed = 2024
    net = RefSSG(num_classes=6, in_channels=6)
    sd = net.state_dict()
    assert len(sd) == 156
    vals, digest = _pointnet2_weights(sd, seed)
    net.load_state_dict({k: torch.from_numpy(vals[k]) if k in vals else sd[k] for k in sd})
    net.eval()
    seen = {}
    hook = net.conv1.register_forward_hook(lambda m, i, o: seen.__setitem__("conv1", o))
    torch.manual_seed(400)
    with torch.no_grad():
        net(torch.from_numpy(cloud(2)))
    hook.remove()
    h = seen["conv1"].double()
    bn_mean, bn_var = h.mean((0, 2)).float(), h.var((0, 2)).float()
    with torch.no_grad():
        net.bn1.running_mean.copy_(bn_mean)
        net.bn1.running_var.copy_(bn_var)
    out = dict(seed=np.int64(seed), weights_sha256=np.array(digest), n_cases=np.int64(3),
               bn1_running_mean=bn_mean.numpy(), bn1_running_var=bn_var.numpy())
    real_randint = torch.randint
    for i, B in enumerate((1, 2, 1)):
        x = cloud(B)
        drawn = []

        def recording_randint(*args, **kwargs):
            t = real_randint(*args, **kwargs)
            drawn.append(t.clone())
            return t

        torch.manual_seed(500 + i)
        torch.randint = recording_randint
        try:
            with torch.no_grad():
                logits, l4 = net(torch.from_numpy(x))
        finally:
            torch.randint = real_randint
        assert len(drawn) == 4 and all(d.shape == (B,) for d in drawn)
        out[f"x{i}"] = x
        out[f"starts{i}"] = torch.stack(drawn).numpy().astype(np.int64)
        out[f"logits{i}"] = logits.numpy().astype(np.float32)
        out[f"l4{i}"] = l4.numpy().astype(np.float32)
        for b in range(B):
            idx, classes, _ = Out.get_key_point_predictions(logits[b], conf_th=0.75)
            out[f"kp_idx{i}_{b}"] = np.asarray(idx, np.int64).reshape(-1)
            out[f"kp_cls{i}_{b}"] = np.asarray(classes, np.int64).reshape(-1)
            assert len(out[f"kp_cls{i}_{b}"]) >= 1, "the reference must select key points for the check to mean anything"
    return out


def _pointnet2_msg_weights(sd, seed):
    """the MSG fixture's weight recipe (tests/test_gpu_pointnet2_msg.py restates it): _pointnet2_weights' distributions
    with BatchNorm keys told apart by module ("bn_blocks" / "mlp_bns" / bn1, bn2) and every conv / fc weight
    N(0, 1.44/fan_in); float32.  Returns (values, SHA-256 of the concatenated float32 bytes)."""
    import hashlib

    rng = np.random.default_rng(seed)
    vals = {}
    for k in sorted(sd):
        if k.endswith("num_batches_tracked"):
            continue
        shape = tuple(sd[k].shape)
        if k.endswith("running_var"):
            v = rng.uniform(0.5, 1.5, shape)
        elif k.endswith("running_mean"):
            v = rng.standard_normal(shape) * 0.1
        elif ".bn_blocks." in k or ".mlp_bns." in k or k.startswith("bn"):
            v = rng.uniform(0.75, 1.25, shape) if k.endswith("weight") else rng.standard_normal(shape) * 0.1
        elif k.endswith("weight"):
            v = rng.standard_normal(shape) * 1.2 / np.sqrt(int(np.prod(shape[1:])))
        else:
            v = rng.standard_normal(shape) * 0.1
        vals[k] = v.astype(np.float32)
    blob = b"".join(vals[k].tobytes() for k in sorted(vals))
    return vals, hashlib.sha256(blob).hexdigest()


def gen_pointnet2_msg(rng):
    """model/pointnet2.py:46-77 PointNet2MSGEncoder(7) (normal_channel True), eval, CPU, with the seeded weights of
    _pointnet2_msg_weights (not stored: the test regenerates them and checks the hash) on two seeded inputs [B, 6, 2048]
    (B = 1, 2); every FPS start the reference draws (torch.randint, model/pointnet2_utils.py:77) recorded as starts
    [2, B], the FPS indices of sa1 / sa2 (int16), the reference's state_dict keys, outputs x [B, 7] and l3_points [B, 1024, 1], and the pooled features of
    the first 8 centroids of sa1 / sa2 (l1_head [B, 320, 8], l2_head [B, 640, 8]) to localise a difference.  Coordinates
    span a 1 x 0.6 x 1.2 box, so the 0.1-radius balls hold a few points (first-hit padding) and the 0.4 / 0.8 ones are
    full at 128."""
    from model.pointnet2 import PointNet2MSGEncoder as RefMSG

    def cloud(B):
        xyz = rng.uniform(-0.5, 0.5, size=(B, 3, 2048)) * [[[1.0], [0.6], [1.2]]]
        feat = rng.uniform(-1.0, 1.0, size=(B, 3, 2048))
        return np.concatenate([xyz, feat], axis=1).astype(np.float32)

    seed = 2025
    net = RefMSG(7)
    sd = net.state_dict()
    vals, digest = _pointnet2_msg_weights(sd, seed)
    net.load_state_dict({k: torch.from_numpy(vals[k]) if k in vals else sd[k] for k in sd})
    net.eval()
    # numbers only: the digest as its 32 bytes, the state_dict keys (in order) as the UTF-8 bytes of their "\n" join
    out = dict(seed=np.int64(seed), weights_sha256=np.frombuffer(bytes.fromhex(digest), np.uint8), n_cases=np.int64(2),
               state_dict_keys=np.frombuffer("\n".join(sd.keys()).encode(), np.uint8))
    real_randint, real_fps = torch.randint, P2.farthest_point_sample
    seen = {}
    hooks = [net.sa1.register_forward_hook(lambda m, i, o: seen.__setitem__("l1", o[1])),
             net.sa2.register_forward_hook(lambda m, i, o: seen.__setitem__("l2", o[1]))]
    for i, B in enumerate((1, 2)):
        x = cloud(B)
        drawn, fps = [], []

        def recording_randint(*args, **kwargs):
            t = real_randint(*args, **kwargs)
            drawn.append(t.clone())
            return t

        def recording_fps(*args, **kwargs):
            t = real_fps(*args, **kwargs)
            fps.append(t.clone())
            return t

        torch.manual_seed(600 + i)
        torch.randint, P2.farthest_point_sample = recording_randint, recording_fps
        try:
            with torch.no_grad():
                logits, l3 = net(torch.from_numpy(x))
        finally:
            torch.randint, P2.farthest_point_sample = real_randint, real_fps
        assert len(drawn) == 2 and all(d.shape == (B,) for d in drawn) and len(fps) == 2
        out[f"x{i}"] = x
        out[f"starts{i}"] = torch.stack(drawn).numpy().astype(np.int64)
        out[f"fps1_{i}"] = fps[0].numpy().astype(np.int16)
        out[f"fps2_{i}"] = fps[1].numpy().astype(np.int16)
        out[f"out{i}"] = logits.numpy().astype(np.float32)
        out[f"l3_{i}"] = l3.numpy().astype(np.float32)
        out[f"l1_head{i}"] = seen["l1"][:, :, :8].numpy().astype(np.float32)
        out[f"l2_head{i}"] = seen["l2"][:, :, :8].numpy().astype(np.float32)
    for h in hooks:
        h.remove()
    return out


class _StubConfig:
    """What the reference's utils/loss.py reads of utils.config.Config (the real module parses sys.argv and creates
    directories on import): `cfg()` -> dict, `cfg.STRUCTURE.x` / `cfg.DATA.x` -> attributes; one shared instance."""
    _d = {"STRUCTURE": {"compute_confidence": False, "disable_position": False, "disable_orientation": False,
                        "position_threshold": 0.03, "position_ignore_threshold": 0.05, "angle_diff_threshold": 0.24,
                        "angle_diff_ignore_threshold": 0.4, "backbone": "minkunet"},
          "DATA": {"ignore_label": -100, "center_at_origin": False, "voxelize_position": True}}

    def __call__(self):
        return self._d

    def __getattr__(self, name):
        return types.SimpleNamespace(**self._d[name])


def _ellipsoid_voxels(rng, n, radii):
    """n distinct integer voxel coordinates on an ellipsoid shell"""
    d = rng.normal(size=(4 * n, 3))
    c = np.unique(np.rint(d / np.linalg.norm(d, axis=1, keepdims=True) * radii).astype(np.int32), axis=0)
    return c[rng.permutation(len(c))[:n]]


def gen_pose_losses(rng):
    """The reference's ten criteria (utils/loss.py) and compute_pose_dist on CPU float32: loss and d loss / d y_pred for
    both reductions; cos2 with and without its confidence terms."""
    stub = types.ModuleType("utils.config")
    stub.Config = _StubConfig
    import utils as ref_utils

    saved = sys.modules.get("utils.config"), getattr(ref_utils, "config", None)
    sys.modules["utils.config"] = ref_utils.config = stub
    try:
        from utils import loss as L
    finally:
        if saved[0] is not None:
            sys.modules["utils.config"] = saved[0]
        if saved[1] is not None:
            ref_utils.config = saved[1]
    cfg = L._config
    B = 3
    # instance 0 close to its target (inside both confidence thresholds), 1 far (outside both ignore thresholds), 2 between
    q = np.stack([rand_quat(rng) for _ in range(B)])
    dq = rng.normal(size=(B, 4)) * np.array([0.02, 0.4, 0.12])[:, None]
    y = np.concatenate([rng.uniform(-0.3, 0.3, (B, 3)), q * rng.uniform(0.7, 1.4, (B, 1))], axis=1).astype(np.float32)
    dp = rng.normal(size=(B, 3))
    dp = dp / np.linalg.norm(dp, axis=1, keepdims=True) * np.array([0.01, 0.2, 0.04])[:, None]
    y_pred = np.concatenate([y[:, :3] + dp, (q + dq) * rng.uniform(0.7, 1.4, (B, 1))], axis=1).astype(np.float32)
    y_pred10 = np.concatenate([y_pred, rng.uniform(0.1, 0.9, (B, 3))], axis=1).astype(np.float32)
    coords = [_ellipsoid_voxels(rng, n, np.array([9.0, 6.0, 4.0])) for n in (300, 1, 157)]
    N = 64
    pn = rng.normal(size=(B, 7, N)).astype(np.float32)
    kp = np.concatenate([rng.uniform(-0.2, 0.2, (B, 40, 3)), rng.normal(size=(B, 40, 1)),
                         rng.uniform(0.05, 1.0, (B, 40, 1))], axis=2).astype(np.float32)
    kp_labels = rng.integers(0, 6, size=(B, 40)).astype(np.int64)
    kp_labels[rng.uniform(size=(B, 40)) < 0.3] = -100
    kp_labels[1, :3], kp_labels[1, -2:] = -100, -100
    out = {"y": y, "y_pred": y_pred, "y_pred10": y_pred10, "pointnet_x": pn, "kp_x": kp, "kp_labels": kp_labels,
           "coords_offsets": np.cumsum([0] + [len(c) for c in coords]).astype(np.int32),
           "coords": np.concatenate(coords).astype(np.int32)}
    sparse_x = types.SimpleNamespace(decomposed_coordinates=[torch.from_numpy(c) for c in coords])
    yt = torch.from_numpy(y)

    def run(name, loss_type, pred, **kw):
        for reduction in ("mean", "sum"):
            crit = L.get_criterion(device="cpu", loss_type=L.LossType(loss_type), reduction=reduction)
            p = torch.from_numpy(pred.copy()).requires_grad_(True)
            loss = crit(yt.clone(), p, **kw)
            loss.backward()
            out[f"{name}_{reduction}_loss"] = np.float32(loss.item())
            out[f"{name}_{reduction}_grad"] = p.grad.numpy().astype(np.float32)

    for lt in ("mse", "cos", "angle", "cos2", "wgeodesic", "smoothl1"):
        run(lt, lt, y_pred)
    # cos2 with confidence: the reference's compute_pose_dist scales its arguments in place (`position *= 1`), which
    # bumps the version of tensors the graph has saved, so its backward raises.  The forward value is taken as it is; for
    # the gradient the same criterion runs with compute_pose_dist handed clones (same value, asserted).
    cfg._d["STRUCTURE"]["compute_confidence"] = True
    as_is = {r: L.get_criterion(device="cpu", loss_type=L.LossType.COS2, reduction=r)(
        yt.clone(), torch.from_numpy(y_pred10.copy())).item() for r in ("mean", "sum")}
    ref_dist = L.compute_pose_dist
    L.compute_pose_dist = lambda gt, pred, **kw: ref_dist(gt.clone(), pred.clone(), **kw)
    try:
        run("cos2_confidence", "cos2", y_pred10)
    finally:
        L.compute_pose_dist = ref_dist
    assert all(np.float32(as_is[r]) == out[f"cos2_confidence_{r}_loss"] for r in as_is)
    cfg._d["STRUCTURE"]["compute_confidence"] = False
    for lt in ("pose", "shape_match", "pose_match"):
        run(lt, lt, y_pred, x=sparse_x)
    cfg._d["STRUCTURE"]["backbone"] = "pointnet2"
    run("pose_pointnet", "pose", y_pred, x=torch.from_numpy(pn))
    cfg._d["STRUCTURE"]["backbone"] = "minkunet"
    run("kp_pose_match", "kp_pose_match", y_pred, x=torch.from_numpy(kp), labels=torch.from_numpy(kp_labels))
    run("kp_pose_match_nolabels", "kp_pose_match", y_pred, x=torch.from_numpy(kp))
    for v in (1, 4):
        d = Mx.compute_pose_dist(yt.clone(), torch.from_numpy(y_pred10.copy()), position_voxelization=v)
        for k, a in zip(("dist", "dist_position", "dist_orientation", "angle_diff"), d):
            out[f"pose_dist_v{v}_{k}"] = a.numpy().astype(np.float32)
    return out


AUG_SINGLES = ("distort_elastic_1_4", "distort_elastic_24_160", "add_noise", "transform_random", "flip_random",
               "rotate_along_gravity")
AUG_FLAGS = dict(elastic=True, noise=True, transform=True, flip=True, gravity=True)


def gen_augmentation(rng):
    """The reference's utils/augmentation.py under fixed np.random seeds: every function alone, augment, and
    augment_segmentation with all flags at probability 1.0 and 0.5 with scale=200 on a metre-sized cloud (3^3 grids) and
    on a voxel-sized one (larger grids).  `open3d` (only change_background uses it) is an empty module."""
    sys.modules.setdefault("open3d", types.ModuleType("open3d"))
    from utils import augmentation as A

    cloud_m = rng.uniform(-0.8, 0.8, (600, 3)).astype(np.float32)
    cloud_v = rng.uniform(-150, 150, (400, 3)).astype(np.float32)
    cloud_s = rng.uniform(-40, 40, (250, 3)).astype(np.float32)
    out = {"cloud_m": cloud_m, "cloud_v": cloud_v, "cloud_s": cloud_s, "single_names": np.array(AUG_SINGLES)}
    calls = {"distort_elastic_1_4": lambda x: A.distort_elastic(x, 1, 4),
             "distort_elastic_24_160": lambda x: A.distort_elastic(x, 24, 160.0),
             "add_noise": A.add_noise, "transform_random": A.transform_random, "flip_random": A.flip_random,
             "rotate_along_gravity": A.rotate_along_gravity}
    seeds = []
    for i, name in enumerate(AUG_SINGLES):
        np.random.seed(1000 + i)
        seeds.append(1000 + i)
        out["single_" + name] = np.asarray(calls[name](np.array(cloud_s)), dtype=np.float64)
    out["single_seeds"] = np.array(seeds, dtype=np.int64)
    np.random.seed(2000)
    out["augment_p1"] = np.asarray(A.augment(np.array(cloud_s), probability=1.0, copy=True, **AUG_FLAGS), dtype=np.float64)
    cases = []
    for ci, cloud in enumerate((cloud_m, cloud_v)):
        for prob, seed in ((1.0, 3000), (0.5, 3001), (0.5, 3007)):  # under seed 3007 the elastic stage does not fire
            np.random.seed(seed)
            res = A.augment_segmentation(np.array(cloud), scale=200, probability=prob, copy=True, **AUG_FLAGS)
            out[f"seg_{ci}_{seed}"] = np.asarray(res, dtype=np.float64)
            cases.append((ci, prob, seed))
    out["seg_cases"] = np.array(cases, dtype=np.float64)
    return out


def _gap(d):
    """smallest minus second smallest of d (inf with fewer than two entries)"""
    d = np.sort(np.asarray(d, dtype=np.float64))
    return np.inf if len(d) < 2 else float(d[1] - d[0])


def _label_margins(points, crop, pose, cs_count, cs_cutoff, radius, kp_idx_sets):
    """The smallest distance of any decision the five functions take on this case to its tipping point, in the
    reference's own expressions: (float64 decisions, decisions computed in the points' dtype)."""
    R = T.get_quaternion_rotation_matrix(pose[3:], switch_w=False)
    m64, mT = [], []
    q = (R.T @ (points - pose[:3]).reshape((-1, 3, 1))).reshape((-1, 3))  # get_ee_idx
    for c, (lo, hi) in enumerate(((-0.05, 0.05), (-0.11, 0.11), (-0.006, 0.12))):
        m64 += [np.abs(q[:, c] - lo).min(), np.abs(q[:, c] - hi).min()]
    q = (R.T @ np.concatenate((crop, pose[:3].reshape(1, 3))).reshape((-1, 3, 1))).reshape((-1, 3))  # key points
    q = q[:-1] - q[-1:]
    for c, v in ((0, 0.005), (0, -0.01), (0, -0.005), (2, 0.08), (2, 0.09)):
        m64.append(np.abs(q[:, c] - v).min())
    grip = q[:, 2] > 0.08
    if grip.any():
        m64.append(np.abs(q[grip, 1]).min())

    def search(target, mask, thr=None):
        d = np.linalg.norm(q[mask] - target, axis=1)
        if len(d) == 0:
            return None
        m64.append(_gap(d))
        if thr is not None:
            m64.append(abs(d.min() - thr))
        return q[mask][d.argmin()], d.min()

    def gripper():
        for side, y in ((q[:, 1] > 0, 0.01), (q[:, 1] < 0, -0.01)):
            if (grip & side).any():
                search(np.array([0, y, q[grip & side, 2].max()]), grip & side)

    kp = np.array([[0.02, 0.09, 0], [0.02, -0.09, 0], [0.014, 0.095, 0.07], [0.014, -0.095, 0.07]])
    back = kp + [[-0.042, 0, 0], [-0.042, 0, 0], [-0.028, 0, 0], [-0.028, 0, 0]]
    for s, dx in enumerate((-0.04, -0.04, -0.03, -0.03)):  # get_key_points
        r = search(kp[s], q[:, 0] > 0.005, 0.018)
        if r is not None and r[1] < 0.018:
            back[s] = r[0] + [dx, 0, 0]
    for s in range(4):
        search(back[s], q[:, 0] < -0.01, 0.018)
    gripper()
    sel = (q[:, 0] > -0.005) & (q[:, 2] < 0.09)  # get_6_key_points
    kp6 = kp.copy()
    kp6[1] = [0.01, -0.1, 0]
    for s, corner in enumerate(([0.24, 0.32, -0.2], [0.24, -0.32, -0.2], [0.24, 0.32, 0.2], [0.24, -0.32, 0.2])):
        r = search(np.array(corner), sel)
        if r is not None:
            m64.append(abs(np.linalg.norm(kp6[s] - r[0]) - 0.03))
    # cross-section: the first count + 1 distances decide the result
    moved = np.array(crop, copy=True)
    moved -= pose[:3]
    ql = (R.T @ moved.reshape((-1, 3, 1))).reshape((-1, 3))
    d = np.sort(T.compute_dists_to_line(ql, np.array([0.05, 0, 0]), np.array([-0.05, 0, 0])))[:cs_count + 1]
    mT += [np.diff(d).min() if len(d) > 1 else np.inf, np.abs(d - cs_cutoff).min()]
    for kp_idx in kp_idx_sets:  # collect_closest_points
        real = kp_idx[kp_idx > -1]
        if len(real):
            n = np.linalg.norm(crop[real].reshape(-1, 1, 3) - crop, axis=2)
            mT.append(np.abs(n.astype(np.float64) - float(crop.dtype.type(radius))).min())
    return float(min(m64)), float(min(mT))


def gen_labels(rng):
    """utils/data.py get_ee_idx, get_ee_cross_section_idx, get_key_points, get_6_key_points and collect_closest_points
    (with load_key_points' label write, data/alivev2.py:227-236) on a synthetic gripper (tests/label_helpers.py
    gripper_cloud): body sizes 50 (12 rod points: fewer cross-section candidates than count), 400 and 3000 (60 rod points:
    more) as float32, and the 400 case again as float64; float64 pose, w first.  The crop points[ee_idx] feeds the other
    four functions.  utils/transformation.py's three line functions on a handful of float64 points.
    A case is written only when every decision in it clears its tipping point: arg-min gaps, mask and threshold
    comparisons by more than 1e-9 (1e-6 for what the reference computes in float32: collect_closest_points and the
    cross-section of float32 points), the deciding cross-section distances pairwise distinct by the same amount;
    otherwise the case is drawn again from the next seed."""
    sys.path.insert(0, os.path.dirname(OUT))
    from label_helpers import gripper_cloud

    count, cutoff, radius, ignore = 32, 0.004, 0.006, -100
    out = dict(count=np.int64(count), cutoff=np.float64(cutoff), radius=np.float64(radius), ignore_label=np.int64(ignore))
    had_int = hasattr(np, "int")
    np.int = int  # get_6_key_points:273 uses the alias numpy removed
    try:
        cases, seed = [(50, 12, np.float32), (400, 60, np.float32), (3000, 60, np.float32), (400, 60, np.float64)], 7000
        for ci, (n_body, n_rod, dtype) in enumerate(cases):
            while True:
                seed += 1
                if ci == 3:  # the float64 copy of case 1
                    points, pose = out["c1_points"].astype(np.float64), out["c1_pose"]
                else:
                    points, pose, _ = gripper_cloud(np.random.default_rng(seed), n_body, n_rod)
                try:
                    ee = Dat.get_ee_idx(points, pose, switch_w=False)
                    crop = points[ee]
                    cs_d, cs_i = Dat.get_ee_cross_section_idx(crop, pose, count=count, cutoff=cutoff, switch_w=False)
                    kp10, kp10_idx = Dat.get_key_points(crop, pose, switch_w=False, ignore_label=ignore)
                    kp6, kp6_idx = Dat.get_6_key_points(crop, pose, switch_w=False, ignore_label=ignore)
                except TypeError:  # get_key_points on an empty front side
                    assert ci != 3
                    continue
                m64, mT = _label_margins(points, crop, pose, count, cutoff, radius, (kp10_idx, kp6_idx))
                ok = m64 > 1e-9 and mT > (1e-6 if dtype == np.float32 else 1e-9)
                print(f"labels case {ci} seed {seed}: crop {len(crop)}, cross-section {len(cs_i)}, margins {m64:.2e} / "
                      f"{mT:.2e} -> {'kept' if ok else 'drawn again'}")
                if ok:
                    break
                assert ci != 3, "the float64 copy fails the margin condition: pick another seed range"
            rec = dict(points=points, pose=pose, ee_idx=ee.astype(np.int64), cs_dists=cs_d, cs_idx=cs_i.astype(np.int64),
                       kp10=kp10, kp10_idx=kp10_idx.astype(np.int64), kp6=kp6, kp6_idx=kp6_idx.astype(np.int64))
            for name, kidx in (("10", kp10_idx), ("6", kp6_idx)):
                real = kidx > -1
                pcls, pidx = Dat.collect_closest_points(kidx[real], crop, euclidean_threshold=radius)
                labels = np.zeros(len(crop), dtype=np.int64) + ignore
                labels[pidx] = np.arange(len(kidx), dtype=np.int64)[real][pcls]
                rec.update({f"pcls{name}": pcls.astype(np.int64), f"pidx{name}": pidx.astype(np.int64),
                            f"labels{name}": labels})
            out.update({f"c{ci}_{k}": v for k, v in rec.items()})
        out["n_cases"] = np.int64(len(cases))
    finally:
        if not had_int:
            del np.int
    lp1, lp2 = rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.1, 0.1, 3)
    pts = rng.uniform(-0.1, 0.1, (12, 3))
    d_sorted = np.sort(T.compute_dists_to_line(pts, lp2, lp1))
    line_cutoff = float((d_sorted[2] + d_sorted[3]) / 2)  # cuts inside the first `count`
    sel_d, sel_i = T.select_closest_points_to_line(pts, lp1, lp2, count=5, cutoff=line_cutoff)
    all_d, all_i = T.select_closest_points_to_line(pts, lp1, lp2, cutoff=1.0)  # count 0: every point
    out.update(line_lp1=lp1, line_lp2=lp2, line_points=pts, line_cutoff=np.float64(line_cutoff), line_dists=T.compute_dists_to_line(pts, lp1, lp2),
               line_vec_dist=np.float64(T.compute_vec_dist_to_line(pts[0], lp1, lp2)), line_sel_dists=sel_d,
               line_sel_idx=sel_i.astype(np.int64), line_all_dists=all_d, line_all_idx=all_i.astype(np.int64))
    return out


def _ycb_functions():
    """The reference's im2col, filterDiscontinuities, registerDepthMap and registeredDepthMapToPointCloud, lifted out of
    scripts/ycb_generate_point_cloud.py with `ast`: the script reads sys.argv and imports h5py, imageio and open3d at module
    level, so it cannot be imported.  `np.float` (removed from numpy) is aliased for the last of them."""
    import ast
    import math

    path = os.path.join(REF, "scripts", "ycb_generate_point_cloud.py")
    tree = ast.parse(open(path).read(), path)
    names = ("im2col", "filterDiscontinuities", "registerDepthMap", "registeredDepthMapToPointCloud")
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in body) == sorted(names)
    if not hasattr(np, "float"):
        np.float = float
    scope = {"np": np, "math": math}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), scope)
    return [scope[n] for n in names[1:]]


def _register_one(one, v, u, depth_K, color_K, Hm, register, color):
    """registerDepthMap of a map that holds the single pixel (v, u): only that row and column are handed over, with the
    principal point moved accordingly, which leaves every term of the function's arithmetic as it was"""
    K = depth_K.copy()
    K[0, 2] -= u
    K[1, 2] -= v
    return register(one[v:v + 1, u:u + 1], color, K, color_K, Hm)


def gen_rgbd(rng):
    """The reference's RGB-D steps (scripts/ycb_generate_point_cloud.py:127-274) on two designed frames.
    (a) filterDiscontinuities on a 480 x 640 uint16 map (the function hard-codes that size): a ramp 8000 + 2u + v, a
    120 x 150 block at 5000, a 20 x 60 hole and 0.1 % single-pixel holes; no per-pixel noise, so that the array compresses.
    Stored: the input and the flat indices of the pixels the filter newly zeroed.
    (b) registerDepthMap + registeredDepthMapToPointCloud(organized=False, mask) of a 48 x 64 depth map (float64 metres,
    two depth layers so that several depth pixels land on one colour pixel) into a 60 x 80 colour image, cameras 1.7 degrees
    rotated and 25 mm apart; a 10 % mask.  Stored: every input, the registered map and the cloud."""
    filt, register, to_cloud = _ycb_functions()
    # ---- (a)
    v, u = np.mgrid[0:480, 0:640]
    depth = (8000 + 2 * u + v).astype(np.uint16)
    depth[200:320, 300:450] = 5000
    depth[60:80, 100:160] = 0
    holes = rng.permutation(480 * 640)[: 480 * 640 // 1000]
    depth.reshape(-1)[holes] = 0
    out = np.asarray(filt(depth))
    assert out.shape == depth.shape and np.all((out == depth) | (out == 0))
    zeroed = np.nonzero((out.reshape(-1) == 0) & (depth.reshape(-1) != 0))[0]
    data = dict(a_depth=depth, a_zeroed=zeroed.astype(np.int32), a_filter_size=np.int64(7), a_filter_thresh=np.int64(1000))
    # ---- (b)
    Hd, Wd, Hc, Wc = 48, 64, 60, 80
    v, u = np.mgrid[0:Hd, 0:Wd]
    raw = (900 + 3 * u + 2 * v).astype(np.uint16)  # millimetres: a tilted wall ...
    raw[10:30, 15:40] = 450 + rng.integers(0, 20, size=(20, 25))  # ... and a box in front of it, which the baseline shifts
    raw.reshape(-1)[rng.permutation(Hd * Wd)[:150]] = 0
    depth_m = raw.astype(np.float64) * 0.001  # what the script hands to registerDepthMap
    depth_K = np.array([[58.0, 0, 31.5], [0, 58.5, 23.5], [0, 0, 1]])
    color_K = np.array([[52.0, 0, 40.2], [0, 52.5, 29.7], [0, 0, 1]])  # shorter than the depth camera: pixels collide
    a = np.deg2rad(1.7)
    Hm = np.eye(4)
    Hm[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Hm[:3, 3] = (0.025, 0.001, -0.002)
    color = rng.integers(0, 256, size=(Hc, Wc, 3), dtype=np.uint8)
    mask = (rng.random((Hc, Wc)) < 0.10).astype(np.uint8)
    registered = register(depth_m, color, depth_K, color_K, Hm)
    cloud = to_cloud(registered, color, color_K, organized=False, mask=mask)
    assert registered.dtype == np.float64 and cloud.dtype == np.float64 and cloud.shape[0] == 1
    # how many depth pixels land on every colour pixel (the reference keeps no such count): each depth pixel registered
    # alone marks the pixel it lands on; one call per depth row keeps this quick, the row's pixels told apart by their Z
    hits = np.zeros((Hc, Wc), dtype=np.int32)
    for vv in range(Hd):
        for uu in range(Wd):
            if depth_m[vv, uu] == 0:
                continue
            one = np.zeros_like(depth_m)
            one[vv, uu] = depth_m[vv, uu]
            hits += _register_one(one, vv, uu, depth_K, color_K, Hm, register, color) > 0
    assert np.array_equal(hits > 0, registered > 0)
    data.update(b_depth=raw, b_depth_scale=np.float64(0.001), b_depth_K=depth_K, b_color_K=color_K, b_H=Hm, b_color=color,
                b_mask=mask, b_registered=registered, b_cloud=cloud[0], b_hits=hits)
    return data


def gen_pointnet_kp(rng):
    """model/pointnet.py:8-36 PointNet(in_channel=6, out_channel=7, embedding_channel=64) (the regressor of
    train_kp_to_pose.py:286-291 with a narrow embedding, so that the fixture stays small), eval, CPU float32: a seeded
    state_dict with randomised BatchNorm statistics (stored under w_<key>, the ordered key list as the UTF-8 bytes of its
    newline join), inputs [B, 6, 6] at B = 1 and B = 3 and the outputs.  The reference's squeeze() drops the batch dimension
    of a single sample and BatchNorm1d then refuses the 1-D tensor: where the reference raises, raises<i> = 1 is stored in
    place of an output."""
    from model.pointnet import PointNet as RefPointNet

    torch.manual_seed(4100)
    net = RefPointNet(in_channel=6, out_channel=7, embedding_channel=64)
    sd = net.state_dict()
    vals = {}
    for k in sd:
        shape = tuple(sd[k].shape)
        if k.endswith("num_batches_tracked"):
            continue
        if k.endswith("running_var"):
            vals[k] = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        elif k.endswith("running_mean"):
            vals[k] = (rng.standard_normal(shape) * 0.1).astype(np.float32)
        elif k.startswith("bn"):
            vals[k] = (rng.uniform(0.75, 1.25, shape) if k.endswith("weight") else rng.standard_normal(shape) * 0.1).astype(np.float32)
        else:
            vals[k] = sd[k].numpy().astype(np.float32)  # torch's seeded initialisation
    net.load_state_dict({k: torch.from_numpy(vals[k]) if k in vals else sd[k] for k in sd})
    net.eval()
    out = {"w_" + k: v for k, v in vals.items()}
    out["state_dict_keys"] = np.frombuffer("\n".join(sd.keys()).encode(), np.uint8)
    out["embedding_channel"] = np.int64(64)
    for i, B in enumerate((1, 3)):
        x = rng.uniform(-0.2, 0.2, size=(B, 6, 6)).astype(np.float32)
        out[f"x{i}"] = x
        try:
            with torch.no_grad():
                out[f"out{i}"] = net(torch.from_numpy(x)).numpy().astype(np.float32)
            out[f"raises{i}"] = np.int64(0)
        except ValueError as e:
            print(f"pointnet_kp: the reference raises at B = {B}: {e}")
            out[f"raises{i}"] = np.int64(1)
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, fn, seed in [("kabsch", gen_kabsch, 100), ("quat_avg", gen_quat_avg, 101), ("add", gen_add, 102),
                           ("fps", gen_fps, 103), ("ball_query", gen_ball_query, 104),
                           ("preprocess", gen_preprocess, 105), ("metrics", gen_metrics, 106),
                           ("calib_chain", gen_calib_chain, 107), ("output_ops", gen_output_ops, 108),
                           ("pointnet2_ssg", gen_pointnet2, 109), ("pointnet2_msg", gen_pointnet2_msg, 110),
                           ("pose_losses", gen_pose_losses, 111), ("augmentation", gen_augmentation, 112),
                           ("labels", gen_labels, 113), ("rgbd_ycb", gen_rgbd, 114), ("pointnet_kp", gen_pointnet_kp, 115)]:
        if len(sys.argv) > 1 and name not in sys.argv[1:]:  # `make_golden.py NAME ...`: only those fixtures
            continue
        data = fn(np.random.default_rng(seed))
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **data)
        print(f"{path}: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
