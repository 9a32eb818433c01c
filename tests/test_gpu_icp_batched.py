"""sv_icp_batched (utils.icp.icp_batched / icp_joint), cases and references in tests/icp_batch_helpers.py.

Independent mode is compared bit for bit with the single calls on the same inputs - the kernels share the single calls'
device functions, so nothing less than np.array_equal is asked.  Shared mode with one problem is the single call again;
with several it is compared with the float64 loop icp_joint_ref, after asserting of the REFERENCE what
tests/test_gpu_icp_point2plane.py asserts of its own: every inlier's nearest target beats the second nearest by more than
1e-6 m^2, every stop decision is at least 1e-7 from its tolerance, cond(A) < 1e6.  Then: updates, pooled and per-problem
fitness equal, |rmse - ref| < 1e-7, |T - T_ref| < 1e-9.

The single calls are themselves the P = 1 independent case of sv_icp_batched (one host routine; one independent problem
without pre takes the single-problem update kernels, from either entry point), so the P = 1 rows of
test_independent_problems_equal_the_single_calls_bit_for_bit hold by construction; the P = 3 and 5 rows and
test_order_and_repetition_change_no_bits pin the batch update kernels to the single calls and that a problem's bits do not
depend on its place in a batch.  What pins the single calls themselves is test_single_calls_give_the_recorded_bits: the
60 calls of _single against tests/golden/icp_single_bits.json, recorded from the separate single-problem kernels and host
loops before the host code was unified."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import icp_batch_helpers as H

pytestmark = pytest.mark.gpu

MD = H.INDEPENDENT_MAX_DISTANCE
# (target points, kind, seed) per source size: the slow problem's seed is one for which the float64 loop needs more than
# 30 updates with either objective.  Offsets 0, 2100, 2101, 2801, 3826, 4850: every target tile edge but the first lies
# inside the concatenated array.
PROBLEMS = {300: [(2100, "slow", 46), (1, "far", 1), (700, "near", 2), (1025, "flat", 3), (1024, "near", 4)],
            1030: [(2100, "slow", 58), (1, "far", 1), (700, "near", 2), (1025, "flat", 3), (1024, "near", 4)]}
OBJECTIVES = ("point2point", "point2plane")


@functools.lru_cache(maxsize=None)
def _problems(S):
    src, _, _, init = H._case(S, 1100, S)
    return src, [H.problem(src, init, T, kind, seed) for T, kind, seed in PROBLEMS[S]]


@functools.lru_cache(maxsize=None)
def _single(gpu, objective, S, p, max_iterations):
    """the single call on problem p: (T, fitness, rmse, updates)"""
    from mrcc_amd.utils import icp as I

    src, probs = _problems(S)
    tgt, nrm, init = probs[p]
    if objective == "point2plane":
        return I.icp_point2plane(src, tgt, nrm, init, MD, max_iterations, device=gpu)
    return I.icp_point2point(src, tgt, init, MD, max_iterations, device=gpu)


SINGLE_BITS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "icp_single_bits.json")
CAPS = (0, 1, 30)


def _bits_key(objective, S, p, max_iterations):
    return f"{objective}/S{S}/problem{p}/max_iterations{max_iterations}"


def _input_sha256(S, p):
    """SHA-256 of the bytes of problem p's src (float32), tgt, normals (float32) and init (float64), in this order"""
    src, probs = _problems(S)
    h = hashlib.sha256()
    for a in (src,) + tuple(probs[p]):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _single_bits(gpu, objective, S, p, max_iterations):
    """the single call's result as the golden file holds it: every double as float.hex()"""
    T, fit, rmse, n = _single(gpu, objective, S, p, max_iterations)
    return {"T": [float(v).hex() for v in np.asarray(T, np.float64).reshape(-1)],
            "stats": [float(fit).hex(), float(rmse).hex(), float(n).hex()], "sha256": _input_sha256(S, p)}


@pytest.mark.parametrize("max_iterations", CAPS)
@pytest.mark.parametrize("S", [300, 1030])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_single_calls_give_the_recorded_bits(gpu, objective, S, max_iterations):
    """A differing value is a bug in the code under test: the file is never re-recorded from it."""
    with open(SINGLE_BITS) as f:
        golden = json.load(f)
    assert len(golden) == len(OBJECTIVES) * len(PROBLEMS) * 5 * len(CAPS)
    for p in range(5):
        want = golden[_bits_key(objective, S, p, max_iterations)]
        assert _input_sha256(S, p) == want["sha256"], f"S={S} problem {p}: the generated INPUTS changed, not the kernels"
    for p in range(5):
        want = golden[_bits_key(objective, S, p, max_iterations)]
        got = _single_bits(gpu, objective, S, p, max_iterations)
        assert got["T"] == want["T"], f"{objective} S={S} problem {p}: out_T {got['T']} vs recorded {want['T']}"
        assert got["stats"] == want["stats"], f"{objective} S={S} problem {p}: {got['stats']} vs recorded {want['stats']}"


def _batched(gpu, objective, S, order, max_iterations, **kw):
    from mrcc_amd.utils import icp as I

    src, probs = _problems(S)
    tgts, nrms, inits = zip(*[probs[p] for p in order])
    return I.icp_batched(src, list(tgts), np.stack(inits), list(nrms) if objective == "point2plane" else None,
                         max_distance=MD, max_iterations=max_iterations, device=gpu, **kw)


def _assert_equals_singles(gpu, objective, S, order, max_iterations, T, stats):
    assert T.shape == (len(order), 4, 4) and stats.shape == (len(order), 3)
    for k, p in enumerate(order):
        Ts, fit, rmse, n = _single(gpu, objective, S, p, max_iterations)
        assert np.array_equal(T[k], Ts), f"problem {p} at place {k}: out_T differs from the single call's"
        assert np.array_equal(stats[k], np.array([fit, rmse, n])), f"problem {p} at place {k}: {stats[k]} vs {(fit, rmse, n)}"


@pytest.mark.parametrize("max_iterations", [0, 1, 30])
@pytest.mark.parametrize("P", [1, 3, 5])
@pytest.mark.parametrize("S", [300, 1030])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_independent_problems_equal_the_single_calls_bit_for_bit(gpu, objective, S, P, max_iterations):
    order = list(range(P))
    T, stats = _batched(gpu, objective, S, order, max_iterations)
    _assert_equals_singles(gpu, objective, S, order, max_iterations, T, stats)
    if P < 5:
        return
    # the call holds every kind of problem at once (what each one does is read off the single calls)
    print(f"{objective} S={S} max_iterations={max_iterations}: updates {stats[:, 2]}, fitness {stats[:, 0]}")
    inits = [prob[2] for prob in _problems(S)[1]]
    slow, far, near, flat, near2 = range(5)
    assert stats[slow, 2] == max_iterations, "the slow problem should use every iteration"
    assert stats[far, 0] == 0.0 and stats[far, 1] == 0.0 and stats[far, 2] == 0
    assert np.array_equal(T[far], inits[far]), "zero inliers: out_T is init_T bit for bit"
    for p in (near, near2):
        # at the cap of 30 a near problem has stopped by the convergence rule, well before the slow one
        assert stats[p, 0] > 0.9 and stats[p, 2] == min(max_iterations, stats[p, 2]) and stats[p, 2] < 15
        assert max_iterations == 0 or (stats[p, 2] >= 1 and not np.array_equal(T[p], inits[p]))
    if objective == "point2plane":
        assert stats[flat, 2] == 0 and stats[flat, 0] > 0.9 and np.array_equal(T[flat], inits[flat])
    elif max_iterations:
        assert stats[flat, 2] >= 1


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_order_and_repetition_change_no_bits(gpu, objective):
    S = 1030
    a = _batched(gpu, objective, S, [0, 1, 2, 3, 4], 30)
    b = _batched(gpu, objective, S, [0, 1, 2, 3, 4], 30)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for order in ([4, 3, 2, 1, 0], [2, 0, 4, 1, 3], [1, 1, 0, 0, 2]):
        T, stats = _batched(gpu, objective, S, order, 30)
        _assert_equals_singles(gpu, objective, S, order, 30, T, stats)


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_null_init_is_the_identity(gpu, objective):
    from mrcc_amd.utils import icp as I

    src, tgt, nrm, init = H._case(300, 1100, 9, identity_init=True, n_far=3)
    assert init is None
    tgts, nrms = [tgt, tgt[:700], tgt[5:]], [nrm, nrm[:700], nrm[5:]]
    normals = nrms if objective == "point2plane" else None
    T, stats = I.icp_batched(src, tgts, None, normals, max_distance=0.003, device=gpu)
    Te, se = I.icp_batched(src, tgts, np.stack([np.eye(4)] * 3), normals, max_distance=0.003, device=gpu)
    assert np.array_equal(T, Te) and np.array_equal(stats, se)
    for p in range(3):
        if objective == "point2plane":
            single = I.icp_point2plane(src, tgts[p], nrms[p], None, 0.003, device=gpu)
        else:
            single = I.icp_point2point(src, tgts[p], None, 0.003, device=gpu)
        assert np.array_equal(T[p], single[0]) and np.array_equal(stats[p], np.array(single[1:]))
        assert stats[p, 2] >= 1
    # shared mode: null init_T is the identity too
    Tj, sj = I.icp_joint(src, tgts, None, normals, max_distance=0.003, device=gpu)
    Tk, sk = I.icp_joint(src, tgts, np.eye(4), normals, max_distance=0.003, device=gpu)
    assert np.array_equal(Tj, Tk) and np.array_equal(sj, sk) and sj.shape == (9,)


# ---- shared mode --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iterations", [0, 30])
@pytest.mark.parametrize("S", [300, 1030])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_shared_mode_with_one_problem_is_the_single_call(gpu, objective, S, max_iterations):
    from mrcc_amd.utils import icp as I

    src, probs = _problems(S)
    for p in range(5):
        tgt, nrm, init = probs[p]
        T, stats = I.icp_joint(src, [tgt], init, [nrm] if objective == "point2plane" else None, max_distance=MD,
                               max_iterations=max_iterations, device=gpu)
        Ts, fit, rmse, n = _single(gpu, objective, S, p, max_iterations)
        assert np.array_equal(T, Ts), p
        assert np.array_equal(stats, np.array([fit, rmse, n, fit, rmse])), (p, stats)


def _compare_joint(gpu, case, objective, max_distance, max_iterations=30, rel=1e-6):
    from mrcc_amd.utils import icp as I

    src, tgts, nrms, pre, init = case
    normals = nrms if objective == "point2plane" else None
    ref = H.icp_joint_ref(src, tgts, normals, pre, init, max_distance, max_iterations, rel, rel)
    print(f"{objective} S={len(src)} T={[len(t) for t in tgts]}: reference updates {ref['updates']}, fitness "
          f"{ref['fitness']:.4f}, gap {ref['gap']:.3g}, stop margin {ref['margin']:.3g}, cond {ref['cond']:.3g}")
    assert ref["gap"] > 1e-6, f"nearest and second nearest target too close for a float32 search ({ref['gap']:.3g} m^2)"
    assert ref["margin"] > 1e-7, f"a stop decision too close to its tolerance ({ref['margin']:.3g})"
    assert ref["cond"] < 1e6, f"cond(A) = {ref['cond']:.3g}"
    T, stats = I.icp_joint(src, tgts, init, normals, pre, max_distance, max_iterations, rel, rel, device=gpu)
    P = len(tgts)
    assert T.shape == (4, 4) and stats.shape == (3 + 2 * P,)
    frames = stats[3:].reshape(P, 2)
    print(f"   updates {stats[2]:.0f}, |rmse - ref| {abs(stats[1] - ref['rmse']):.3g}, |T - T_ref| "
          f"{np.abs(T - ref['T']).max():.3g}, per-problem |rmse - ref| {np.abs(frames[:, 1] - ref['frame_rmse']).max():.3g}")
    assert stats[2] == ref["updates"], f"updates {stats[2]}, reference {ref['updates']}"
    assert stats[0] == ref["fitness"], f"pooled fitness {stats[0]!r}, reference {ref['fitness']!r}"
    assert abs(stats[1] - ref["rmse"]) < 1e-7, f"pooled rmse {stats[1]!r}, reference {ref['rmse']!r}"
    assert np.abs(T - ref["T"]).max() < 1e-9, f"|T - T_ref| = {np.abs(T - ref['T']).max():.3g}"
    assert np.array_equal(frames[:, 0], ref["frame_fitness"]), f"{frames[:, 0]} vs {ref['frame_fitness']}"
    assert np.abs(frames[:, 1] - ref["frame_rmse"]).max() < 1e-7
    return T, stats, ref


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_shared_mode_matches_the_float64_loop(gpu, objective):
    """P = 4, distinct pre, distinct target sizes round the 1024-point tile, S off the 256- and 1024-thread strides"""
    src, tgts, nrms, pre, init, true_T = H.joint_case(1030, [700, 1024, 1025, 2100], 0)
    T, stats, ref = _compare_joint(gpu, (src, tgts, nrms, pre, init), objective, 0.003)
    assert ref["updates"] >= 1 and len(set(ref["frame_fitness"])) == 4
    assert H.pose_error(T, true_T)[0] < H.pose_error(init, true_T)[0]
    # the iteration caps, and zero tolerances that never converge
    for max_iterations in (0, 1):
        _, s, _ = _compare_joint(gpu, (src, tgts, nrms, pre, init), objective, 0.003, max_iterations)
        assert s[2] == max_iterations
    # repeated runs give the same bits (fixed summation order, no atomics)
    from mrcc_amd.utils import icp as I

    normals = nrms if objective == "point2plane" else None
    again = I.icp_joint(src, tgts, init, normals, pre, 0.003, device=gpu)
    assert np.array_equal(again[0], T) and np.array_equal(again[1], stats)


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_identity_pre_agrees_with_no_pre(gpu, objective):
    from mrcc_amd.utils import icp as I

    src, probs = _problems(300)
    tgts, nrms = [probs[p][0] for p in (2, 4)], [probs[p][1] for p in (2, 4)]
    normals = nrms if objective == "point2plane" else None
    init = probs[2][2]
    a = I.icp_joint(src, tgts, init, normals, None, MD, device=gpu)
    b = I.icp_joint(src, tgts, init, normals, np.stack([np.eye(4)] * 2), MD, device=gpu)
    assert a[1][2] >= 1
    assert np.abs(a[0] - b[0]).max() < 1e-12 and np.abs(a[1] - b[1]).max() < 1e-12


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_joint_refinement_recovers_the_shared_transform(gpu, objective):
    """M = 5 one-sided views of an asymmetric 1500-point model, 0.5 mm noise, start 5 mm / 2 degrees off
    (icp_batch_helpers.recovery_case).  The GPU must equal the float64 loop; how close that loop itself comes to the
    true transform is printed and recorded in DESIGN.md, not asserted against a chosen number."""
    src, tgts, nrms, pre, init, true_T = H.recovery_case(1)
    assert len(src) == 1500 and len(tgts) == 5
    T, stats, ref = _compare_joint(gpu, (src, tgts, nrms, pre, init), objective, H.RECOVERY_MAX_DISTANCE)
    print(f"   start {H.pose_error(init, true_T)}, reference {H.pose_error(ref['T'], true_T)}, "
          f"GPU {H.pose_error(T, true_T)} (m, degrees)")
    assert ref["updates"] >= 1
