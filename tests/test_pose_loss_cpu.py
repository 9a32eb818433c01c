"""utils/loss.py without a GPU: the float64 restatement of tests/loss_helpers.py and the six dense criteria against the
reference's recorded values (tests/golden/pose_losses.npz, written by tools/make_golden.py pose_losses on CPU float32),
compute_pose_dist, and the argument checks of sv_pose_match_loss and of the criteria (host code only: nothing reaches a
device).

Bounds against the fixture: the fixture is float32, so the error measured is the reference's own rounding.  Each bound
is 4x the worst relative error (max-abs difference over the tensor's max-abs) measured on the CPU, and no looser than 1e-4.
"""
import ctypes

import numpy as np
import pytest
import torch

import loss_helpers as H

# 4 x the worst measured relative error, capped at 1e-4 (measured values in the tests' docstrings).  The dense criteria
# measured 0 (same torch ops in the same order as the reference, on the host that wrote the fixture); another host's
# torch may vectorise a float32 sum differently, so their bound is 4 x one float32 rounding (2^-24 = 6e-8), not 0.
POINT_BOUND = min(4 * 6.34e-7, 1e-4)
DENSE_BOUND = min(4 * 6e-8, 1e-4)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("pose_losses")


@pytest.fixture
def config():
    from mrcc_amd.utils.config import Config

    Config.reset()
    yield Config()
    Config.reset()


def _instances(fx):
    off = fx["coords_offsets"]
    return [fx["coords"][off[b]: off[b + 1]] for b in range(len(off) - 1)]


def test_restatement_matches_the_reference_fixture(fx):
    """The float64 restatement, loss and d loss / d y_pred, for pose (sparse and pointnet input), shape_match, pose_match
    and kp_pose_match (with and without labels), both reductions.  Worst relative error measured: 6.34e-7 (the
    gradient of pose_match under "sum": the fixture's float32 quaternion Jacobian and sums); bound 4 x that = 2.5e-6."""
    y, y_pred = fx["y"], fx["y_pred"]
    kp, lab = fx["kp_x"], fx["kp_labels"]
    cases = {
        "pose": ("pose", _instances(fx), None, None),
        "shape_match": ("shape_match", _instances(fx), None, None),
        "pose_match": ("pose_match", _instances(fx), None, None),
        "pose_pointnet": ("pose", [x[:3].T for x in fx["pointnet_x"]], None, None),
        "kp_pose_match": ("kp_pose_match", [x[:, :3] for x in kp], [x[:, -1] for x in kp], [l > -100 for l in lab]),
        "kp_pose_match_nolabels": ("kp_pose_match", [x[:, :3] for x in kp], [x[:, -1] for x in kp], None),
    }
    worst = 0.0
    for key, (name, inst, w, m) in cases.items():
        for reduction in ("mean", "sum"):
            loss, grad = H.criterion_value_and_grad(name, y, y_pred, inst, w, m, reduction)
            e_l = H.rel_err(loss, fx[f"{key}_{reduction}_loss"])
            e_g = H.rel_err(grad, fx[f"{key}_{reduction}_grad"])
            print(f"{key} {reduction}: loss rel {e_l:.2e}, grad rel {e_g:.2e}")
            worst = max(worst, e_l, e_g)
            assert e_l <= POINT_BOUND and e_g <= POINT_BOUND, (key, reduction, e_l, e_g)
    print(f"worst relative error {worst:.2e} (bound {POINT_BOUND:.1e})")


def test_pose_times_1e3_only_under_mean(fx):
    """the reference multiplies `pose` by 1e3 after dividing by the batch, under "mean" only (utils/loss.py:184-186)"""
    B = len(fx["y"])
    assert abs(float(fx["pose_mean_loss"]) / (float(fx["pose_sum_loss"]) / B * 1e3) - 1) < 1e-6
    assert abs(float(fx["shape_match_mean_loss"]) / (float(fx["shape_match_sum_loss"]) / B) - 1) < 1e-6


@pytest.mark.parametrize("loss_type", ["mse", "cos", "angle", "cos2", "wgeodesic", "smoothl1", "cos2_confidence"])
def test_dense_criteria_match_the_reference_fixture(fx, config, loss_type):
    """The six dense criteria on CPU float32 tensors, loss and gradient, both reductions; cos2 also with its confidence
    terms.  Worst relative error measured: 0 (bit-equal); bound 4 x one float32 rounding = 2.4e-7, see DENSE_BOUND."""
    from mrcc_amd.utils.loss import LossType, get_criterion

    name, pred = loss_type, fx["y_pred"]
    if loss_type == "cos2_confidence":
        config.update({"STRUCTURE": {"compute_confidence": True}})
        name, pred = "cos2", fx["y_pred10"]
    for reduction in ("mean", "sum"):
        crit = get_criterion(device="cpu", loss_type=LossType(name), reduction=reduction)
        y = torch.from_numpy(fx["y"].copy())
        p = torch.from_numpy(pred.copy()).requires_grad_(True)
        loss = crit(y, p)
        loss.backward()
        e_l = H.rel_err(float(loss.detach()), fx[f"{loss_type}_{reduction}_loss"])
        e_g = H.rel_err(p.grad.numpy(), fx[f"{loss_type}_{reduction}_grad"])
        print(f"{loss_type} {reduction}: loss rel {e_l:.2e}, grad rel {e_g:.2e}")
        assert e_l <= DENSE_BOUND and e_g <= DENSE_BOUND, (reduction, e_l, e_g)
        assert np.array_equal(y.numpy(), fx["y"])


def test_cos2_reads_the_disable_switches(fx, config):
    from mrcc_amd.utils.loss import LossType, get_criterion

    y, p = torch.from_numpy(fx["y"].copy()), torch.from_numpy(fx["y_pred"].copy())
    crit = get_criterion(device="cpu", loss_type=LossType.COS2)
    both = float(crit(y, p))
    config.update({"STRUCTURE": {"disable_orientation": True}})
    assert float(crit(y, p)) == pytest.approx(float(torch.nn.functional.mse_loss(y[:, :3], p[:, :3])), rel=1e-6)
    config.update({"STRUCTURE": {"disable_orientation": False, "disable_position": True}})
    assert float(crit(y, p)) == pytest.approx(2 * float(torch.nn.functional.mse_loss(y[:, 3:7], p[:, 3:7])), rel=1e-6)
    assert both != float(crit(y, p))


def test_compute_pose_dist_matches_and_leaves_its_arguments(fx):
    """compute_pose_dist's four outputs against the reference for position_voxelization 1 and 4 (bound as the dense
    criteria; measured 0), and - unlike the reference - no in-place scaling of gt / pred"""
    from mrcc_amd.utils.metrics import compute_pose_dist

    for v in (1, 4):
        gt, pred = torch.from_numpy(fx["y"].copy()), torch.from_numpy(fx["y_pred10"].copy())
        out = compute_pose_dist(gt, pred, position_voxelization=v)
        assert len(out) == 4
        for k, a in zip(("dist", "dist_position", "dist_orientation", "angle_diff"), out):
            e = H.rel_err(a.numpy(), fx[f"pose_dist_v{v}_{k}"])
            print(f"v={v} {k}: rel {e:.2e}")
            assert e <= DENSE_BOUND, (v, k, e)
        assert np.array_equal(gt.numpy(), fx["y"]) and np.array_equal(pred.numpy(), fx["y_pred10"])


def test_loss_type_values():
    from mrcc_amd.utils.loss import LossType

    assert {m.name: m.value for m in LossType} == {
        "MSE": "mse", "COS": "cos", "ANGLE": "angle", "COS2": "cos2", "WGEODESIC": "wgeodesic", "SMOOTHL1": "smoothl1",
        "POSE": "pose", "SHAPE_MATCH": "shape_match", "POSE_MATCH": "pose_match", "KP_POSE_MATCH": "kp_pose_match"}
    assert LossType("pose_match") is LossType.POSE_MATCH


def test_mse_is_nn_mseloss(fx):
    from mrcc_amd.utils.loss import LossType, get_criterion

    y, p = torch.from_numpy(fx["y"].copy()), torch.from_numpy(fx["y_pred"].copy())
    for reduction in ("mean", "sum"):
        crit = get_criterion(device="cpu", loss_type=LossType.MSE, reduction=reduction)
        assert isinstance(crit, torch.nn.MSELoss) and crit.reduction == reduction
        assert torch.equal(crit(y, p), torch.nn.functional.mse_loss(y, p, reduction=reduction))


def test_qeuler_zyx_against_rotation_matrices():
    """qeuler('zyx') of a unit quaternion gives angles whose Rz Ry Rx product is the quaternion's matrix"""
    from mrcc_amd.utils.loss import qeuler

    rng = np.random.default_rng(5)
    q = rng.normal(size=(16, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    e = qeuler(torch.from_numpy(q), order="zyx", epsilon=1e-6).numpy()
    for qi, (x, y, z) in zip(q, e):
        cx, sx, cy, sy, cz, sz = np.cos(x), np.sin(x), np.cos(y), np.sin(y), np.cos(z), np.sin(z)
        Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        assert np.abs(Rz @ Ry @ Rx - H.quat_matrix_np(qi)).max() < 1e-9
    with pytest.raises(NotImplementedError):
        qeuler(torch.zeros(1, 4), order="xyz")


def test_pose_match_loss_argument_checks_without_gpu():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    p = ctypes.create_string_buffer(64)  # stands in for a non-null pointer: every call here fails its checks first
    M, B = 1000, 3
    need = lib.sv_pose_loss_workspace_bytes(M, B)
    assert need >= (B + 1) * 4 + M * 4 + ((M + 255) // 256 + B) * 14 * 8
    assert lib.sv_pose_loss_workspace_bytes(2 * M, B) > need and lib.sv_pose_loss_workspace_bytes(M, 2 * B) >= need

    def loss(M=M, B=B, mode=0, points=p, offsets=p, weights=None, mask=None, R=p, t=None, R_pred=p, t_pred=None, ws=p,
             ws_bytes=need, out=p, grad_R=p, grad_t=None, match=None):
        return lib.sv_pose_match_loss(points, offsets, M, B, weights, mask, R, t, R_pred, t_pred, mode, ws, ws_bytes, out,
                                      grad_R, grad_t, match, None)

    for kw in ({"B": 0}, {"B": -1}, {"B": 1025}):
        assert loss(**kw) == -1 and b"1 to 1024 instances" in lib.sv_last_error(), kw
    for kw in ({"M": -1}, {"M": 1 << 24}):
        assert loss(**kw) == -1 and b"2^24 rows" in lib.sv_last_error(), kw
    for kw in ({"mode": -1}, {"mode": 4}, {"mode": 1 << 20}):
        assert loss(**kw) == -1 and b"bad mode" in lib.sv_last_error(), kw
    for kw in ({"points": None}, {"offsets": None}, {"R": None}, {"R_pred": None}, {"out": None}, {"ws": None}):
        assert loss(**kw) == -1 and b"null pointer" in lib.sv_last_error(), kw
    for kw in ({"t": p}, {"t_pred": p}, {"t": p, "mode": 2}, {"t_pred": p, "mode": 3}):
        assert loss(**kw) == -1 and b"t and t_pred" in lib.sv_last_error(), kw
    assert loss(grad_t=p) == -1 and b"grad_t without a translation" in lib.sv_last_error()
    assert loss(mode=2, weights=p, t=p, t_pred=p) == -1 and b"no weights" in lib.sv_last_error()
    assert loss(mode=0, match=p) == -1 and b"SHAPE_MATCH only" in lib.sv_last_error()
    # one byte short of what the three arrays take at 256-byte alignment (the size function adds slack)
    used = 256 + ((((M + 255) // 256 + B) * 14 * 8 + 255) // 256) * 256 + M * 4
    for ws_bytes in (0, 256, used - 1):
        for mode in range(4):
            kw = {"t": p, "t_pred": p} if mode >= 2 else {}
            assert loss(ws_bytes=ws_bytes, mode=mode, **kw) == -2 and b"workspace too small" in lib.sv_last_error()
    assert used <= need


@pytest.fixture
def no_launch(monkeypatch):
    """Replace the criteria's library call: reaching it means a bad argument got past the checks."""
    from mrcc_amd.utils import loss

    def fail(name, *args):
        raise AssertionError(f"{name} was called with arguments the criterion should have rejected")

    monkeypatch.setattr(loss, "call", fail)


@pytest.mark.parametrize("loss_type", ["pose", "shape_match", "pose_match", "kp_pose_match"])
def test_point_matching_criteria_reject_bad_arguments(no_launch, config, loss_type):
    from mrcc_amd._lib import SvHipError
    from mrcc_amd.utils.loss import LossType, get_criterion

    config.update({"DATA": {"center_at_origin": False, "voxelize_position": True}})
    crit = get_criterion(loss_type=LossType(loss_type))
    y, p = torch.zeros(3, 7), torch.zeros(3, 7)
    x = torch.zeros(3, 8, 5)
    with pytest.raises(ValueError, match="same B"):
        crit(y, p[:2], x=x)
    with pytest.raises(ValueError, match="7 columns"):
        crit(y[:, :6], p, x=x)
    with pytest.raises(ValueError, match="7 columns"):
        crit(y, p[:, :4], x=x)
    with pytest.raises(ValueError, match="x .* is required"):
        crit(y, p)
    with pytest.raises(ValueError, match="must not require grad"):
        crit(y.clone().requires_grad_(True), p, x=x)
    with pytest.raises(SvHipError, match="no CPU fallback"):
        crit(y, p, x=x)


def test_config_asserts_of_the_reference(config):
    from mrcc_amd.utils.loss import LossType, get_criterion

    with pytest.raises(AssertionError):  # DATA.center_at_origin defaults to True
        get_criterion(loss_type=LossType.SHAPE_MATCH)
    with pytest.raises(AssertionError):  # DATA.voxelize_position defaults to False
        get_criterion(loss_type=LossType.POSE_MATCH)
    assert callable(get_criterion(loss_type=LossType.POSE)) and callable(get_criterion(loss_type="kp_pose_match"))
