"""sv_icp_batched at the widths and counts its kernels are built round (cases and references: tests/icp_batch_helpers.py).

The batch update kernels reduce over the source with 1024 threads (point-to-point) and 512 threads (point-to-plane):
S = 511, 512, 513, 1023, 1024, 1025 lie on either side of both.  ICP_MAX_PROBLEMS = 64 fills icp_joint_tail_kernel's one
wave (one lane per problem) and IcpOffsets to its last slot: P = 63 and 64, with 2 as the smallest batch.

Independent mode is compared bit for bit with the single calls on the same inputs, as
test_independent_problems_equal_the_single_calls_bit_for_bit does (np.array_equal, nothing less); the single calls at
these S are pinned to their float64 loops by test_icp_matches_float64_open3d_loop and
test_point2plane_matches_float64_loop.  Shared mode goes through _compare_joint of tests/test_gpu_icp_batched.py, its
preconditions on the reference and its bounds unchanged: updates, pooled fitness and all P per-problem fitness values
equal, |rmse - ref| < 1e-7, |T - T_ref| < 1e-9.  For the seeds below the reference reports (point-to-point /
point-to-plane) a nearest / second-nearest gap of 3.45e-5 / 3.45e-5 m^2 at P = 2, 2.38e-5 / 2.38e-5 at P = 63 and
2.50e-5 / 2.50e-5 at P = 64, stop margins of 1.0e-6 / 0.99e-6 throughout, and cond(A) of 285, 14.6 and 14.8."""
import functools

import numpy as np
import pytest

import icp_batch_helpers as H
from test_gpu_icp_batched import OBJECTIVES, _compare_joint

pytestmark = pytest.mark.gpu

MD = H.INDEPENDENT_MAX_DISTANCE
WIDTHS = [511, 512, 513, 1023, 1024, 1025]
WIDTH_PROBLEMS = [(700, "near", 2), (1025, "flat", 3), (1, "far", 1)]  # target points, kind, seed
S_COUNT = 257
T_CYCLE = [1, 2, 700, 1023, 1024, 1025]
KIND_CYCLE = ["far", "near", "flat", "slow", "near"]  # five kinds against six sizes: every pairing occurs within 30 problems
COUNTS = [2, 63, 64]
JOINT_SEEDS = {2: 0, 63: 0, 64: 0}  # the float64 loop meets _compare_joint's preconditions for these, both objectives


@functools.lru_cache(maxsize=None)
def _source(S):
    src, _, _, init = H._case(S, 1100, S)
    return src, init


@functools.lru_cache(maxsize=None)
def _problem(S, key):
    """problem `key` on the source of S points: key (T, kind, seed) -> (tgt, nrm, init)"""
    src, init = _source(S)
    return H.problem(src, init, *key)


def _count_keys(P):
    """P problems: sizes and kinds cycle, and the last problem is a far one as the first is (zero inliers: no update)"""
    keys = [(T_CYCLE[i % 6], KIND_CYCLE[i % 5], 100 + i) for i in range(P - 1)]
    return keys + [(1023, "far", 99)]


@functools.lru_cache(maxsize=None)
def _single(gpu, objective, S, key, max_iterations):
    from mrcc_amd.utils import icp as I

    tgt, nrm, init = _problem(S, key)
    if objective == "point2plane":
        return I.icp_point2plane(_source(S)[0], tgt, nrm, init, MD, max_iterations, device=gpu)
    return I.icp_point2point(_source(S)[0], tgt, init, MD, max_iterations, device=gpu)


def _batched(gpu, objective, S, keys, max_iterations):
    from mrcc_amd.utils import icp as I

    tgts, nrms, inits = zip(*[_problem(S, k) for k in keys])
    return I.icp_batched(_source(S)[0], list(tgts), np.stack(inits), list(nrms) if objective == "point2plane" else None,
                         max_distance=MD, max_iterations=max_iterations, device=gpu)


def _assert_equals_singles(gpu, objective, S, keys, max_iterations, T, stats):
    assert T.shape == (len(keys), 4, 4) and stats.shape == (len(keys), 3)
    for k, key in enumerate(keys):
        Ts, fit, rmse, n = _single(gpu, objective, S, key, max_iterations)
        assert np.array_equal(T[k], Ts), f"problem {key} at place {k}: out_T differs from the single call's"
        assert np.array_equal(stats[k], np.array([fit, rmse, n])), f"problem {key} at place {k}: {stats[k]} vs {(fit, rmse, n)}"


@pytest.mark.parametrize("max_iterations", [0, 30])
@pytest.mark.parametrize("S", WIDTHS)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_independent_batches_at_the_reduction_widths(gpu, objective, S, max_iterations):
    keys = WIDTH_PROBLEMS
    T, stats = _batched(gpu, objective, S, keys, max_iterations)
    _assert_equals_singles(gpu, objective, S, keys, max_iterations, T, stats)
    near, flat, far = range(3)
    assert stats[far, 0] == 0.0 and stats[far, 2] == 0 and np.array_equal(T[far], _problem(S, keys[far])[2])
    assert stats[near, 0] > 0.9 and stats[flat, 0] > 0.9
    if max_iterations == 0:
        assert (stats[:, 2] == 0).all()
    else:  # the near problem stops by the convergence rule; all normals (0, 0, 1) give no point-to-plane update
        assert 1 <= stats[near, 2] < 15
        assert stats[flat, 2] == 0 if objective == "point2plane" else 1 <= stats[flat, 2] < 15


@pytest.mark.parametrize("P", COUNTS)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_problem_counts_equal_the_single_calls_bit_for_bit(gpu, objective, P):
    keys = _count_keys(P)
    assert len(keys) == P and keys[0][1] == "far" and keys[-1][1] == "far"
    T, stats = _batched(gpu, objective, S_COUNT, keys, 30)
    _assert_equals_singles(gpu, objective, S_COUNT, keys, 30, T, stats)
    for end in (0, P - 1):
        assert stats[end, 0] * S_COUNT < 3 and stats[end, 2] == 0 and np.array_equal(T[end], _problem(S_COUNT, keys[end])[2])
    print(f"{objective} P={P}: updates {sorted(set(stats[:, 2].tolist()))}")
    assert P == 2 or len(set(stats[:, 2].tolist())) >= 3, "the problems should stop at different rounds"
    # the reversed batch gives every problem the same bits
    Tr, sr = _batched(gpu, objective, S_COUNT, keys[::-1], 30)
    assert np.array_equal(Tr[::-1], T) and np.array_equal(sr[::-1], stats)


@pytest.mark.parametrize("P", COUNTS)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_shared_mode_at_problem_counts(gpu, objective, P):
    """P = 64: every lane of the tail kernel's wave owns a problem.  Target sizes cycle through 1, 2, 700, 1023, 1024,
    1025 (P = 2: 700 and 1023), so most problems see only part of the model and the per-problem fitness values differ."""
    sizes = [700, 1023] if P == 2 else [T_CYCLE[p % 6] for p in range(P)]
    src, tgts, nrms, pre, init, true_T = H.joint_case(S_COUNT, sizes, JOINT_SEEDS[P])
    T, stats, ref = _compare_joint(gpu, (src, tgts, nrms, pre, init), objective, 0.003)
    assert ref["updates"] >= 1 and len(set(ref["frame_fitness"])) >= min(P, 10)
    assert H.pose_error(T, true_T)[0] < H.pose_error(init, true_T)[0]
