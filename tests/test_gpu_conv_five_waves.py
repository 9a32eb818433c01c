"""The WIDE step of the tiled sparse convolution (csrc/sv_conv.hip: 64 x 192 tiles and the 32-row tail body of the dual
launch) keeps a ring of FOUR k-steps of weights and HALF a step's gathers in registers.  What can go wrong there is the
ring's addressing at the edges of a step: the reload that crosses into the next step, a partial last channel chunk that
is shorter than, as long as, or one longer than the ring, a tile with one single step, and the mid-step LDS write.

Every comparison is bit-exact against oracle.conv on a map of a few thousand voxels, with scale, shift, residual and
ReLU.  A channel count stands for the number of valid k-steps of its last chunk on the 64-row tile (32 channels per step):
32 -> one chunk per offset (8), 388 -> 1, 400 -> 4 (the ring length), 404 -> 5, 416 -> 8 after 12 full chunks, 448 -> 14
full chunks; on the 32-row tail body (64 channels per step) the same counts leave 8, 1, 4, 5, 8 of 16 k-steps.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

COUT = 384
CINS = (32, 388, 400, 404, 416, 448)
MAIN, DUAL = "conv_fwd_kernel<64, 4, 3>", "conv_fwd_dual_kernel<64, 32, 4, 3>"


def _sparse(gpu, c4):
    from mrcc_amd import MinkowskiEngine as ME

    feats = np.zeros((len(c4), 3), np.float32)
    return ME.TensorField(torch.from_numpy(feats), torch.from_numpy(c4), device=gpu).sparse()


@pytest.fixture(scope="module")
def room(gpu, oracle):
    """one synthetic map (3 - 4 thousand voxels), its 3x3x3 and up plans, and one set of operands all cases slice"""
    import mrcc_amd

    pts, _, _ = mrcc_amd.synth.gen_room(6000, 0.5, 3)
    c4 = np.concatenate([np.zeros((len(pts), 1), np.float32), pts * np.float32(50)], axis=1)
    cm = _sparse(gpu, c4).coordinate_manager
    frame = oracle.Frame(oracle.voxelize(c4)["coords"])
    frame.down(1)
    V, V2 = cm.stride_map(1).V, cm.stride_map(2).V
    assert 2000 < V < 6000 and V2 == len(frame.maps[2])
    rng = np.random.default_rng(5)
    cmax = max(CINS)
    return dict(
        cm=cm, frame=frame, V=V, V2=V2,
        x=rng.normal(size=(V, cmax)).astype(np.float32),
        W=(rng.normal(size=(27, cmax, COUT)) * np.sqrt(2.0 / (27 * COUT))).astype(np.float32),
        scale=rng.uniform(0.5, 1.5, size=COUT).astype(np.float32),
        shift=rng.normal(size=COUT).astype(np.float32),
        res=rng.normal(size=(V, COUT)).astype(np.float32),
        want={},  # (kind, cin) -> oracle result, computed once
    )


def _operands(room, K, cin, V_in, V_out):
    """the first K offsets / cin channels / rows of the shared operands, contiguous"""
    c = np.ascontiguousarray
    return c(room["x"][:V_in, :cin]), c(room["W"][:K, :cin]), c(room["res"][:V_out])


def _launch(gpu, x, W, plan, V_out, room, res, force=None, dispatch=None):
    """(result, instance name) of one conv_forward with every epilogue operand; force = SV_CONV_FORCE, dispatch =
    (want_scale, tail_fraction) of the call"""
    import contextlib

    import mrcc_amd
    from mrcc_amd import nn as svnn

    t = lambda a: torch.from_numpy(a).to(gpu)
    if force:
        os.environ["SV_CONV_FORCE"] = force
    try:
        with (mrcc_amd._lib.conv_dispatch(*dispatch) if dispatch else contextlib.nullcontext()):
            got = svnn.conv_forward(t(x), t(W), plan, V_out, t(room["scale"]), t(room["shift"]), t(res), 1)
            name = mrcc_amd._lib.conv_last_instance()[0]
    finally:
        os.environ.pop("SV_CONV_FORCE", None)
    return got.cpu().numpy(), name


def _want(oracle, room, kind, cin, x, W, nbr, V_out, res):
    key = (kind, cin)
    if key not in room["want"]:
        room["want"][key] = oracle.conv(x, W, nbr, V_out, room["scale"], room["shift"], res, oracle.ACT_RELU)
    return room["want"][key]


def _check_both_bodies(gpu, oracle, room, kind, cin, plan, nbr, K, V_in, V_out):
    x, W, res = _operands(room, K, cin, V_in, V_out)
    want = _want(oracle, room, kind, cin, x, W, nbr, V_out, res)
    got, name = _launch(gpu, x, W, plan, V_out, room, res, force="64,4,3")
    assert name == MAIN
    assert np.array_equal(got, want), f"{MAIN} Cin {cin}: max abs diff {np.abs(got - want).max()}"
    # the dual launch with half of the plan tiles on the 32-row tail body
    got, name = _launch(gpu, x, W, plan, V_out, room, res, dispatch=(0.0, 0.5))
    assert name == DUAL
    assert np.array_equal(got, want), f"{DUAL} Cin {cin}: max abs diff {np.abs(got - want).max()}"


@pytest.mark.parametrize("cin", CINS)
def test_k27_channel_tails(gpu, oracle, room, cin):
    cm, V = room["cm"], room["V"]
    _check_both_bodies(gpu, oracle, room, "k3", cin, cm.plan_k3(1), room["frame"].k3(1), 27, V, V)


@pytest.mark.parametrize("cin", CINS)
def test_k8_up_plan_channel_tails(gpu, oracle, room, cin):
    cm = room["cm"]
    cm.plan_down(1)
    _check_both_bodies(gpu, oracle, room, "up", cin, cm.plan_up(2), room["frame"].kup(2), 8, room["V2"], room["V"])


@pytest.mark.parametrize("force", ["64,4,3", "32,4,3"])
@pytest.mark.parametrize("cin", CINS)
def test_dense_rows_tail_tiles_and_clamped_rows(gpu, oracle, room, cin, force):
    """K = 1 without a plan: the last tile is partial (rows past V_out are clamped gathers and dropped stores); "32,4,3"
    with a partial last chunk is the tail body of the dual launch as a launch of its own"""
    for V_out in (1, 63, 64, 65, 129):
        x, W, res = _operands(room, 1, cin, V_out, V_out)
        want = oracle.conv(x, W, None, V_out, room["scale"], room["shift"], res, oracle.ACT_RELU)
        got, name = _launch(gpu, x, W, None, V_out, room, res, force=force)
        assert name == f"conv_fwd_kernel<{force.replace(',', ', ')}>"
        assert np.array_equal(got, want), f"V_out {V_out}: max abs diff {np.abs(got - want).max()}"


@pytest.mark.parametrize("cin", [32, 64, 404])
def test_isolated_voxels_single_offset_tiles(gpu, oracle, room, cin):
    """voxels three cells apart have no neighbour but themselves: every tile visits the centre offset alone, and with one
    channel chunk (Cin 32 on the 64-row tile, 32 / 64 on the 32-row tile) its first step is its last"""
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
    c4 = np.concatenate([np.zeros((len(g), 1), np.float32), (3 * g + 0.5).astype(np.float32)], axis=1)
    cm = _sparse(gpu, c4).coordinate_manager
    V = cm.stride_map(1).V
    nbr = oracle.Frame(oracle.voxelize(c4)["coords"]).k3(1)
    assert V == 300 and (nbr[13] >= 0).all() and (np.delete(nbr, 13, axis=0) < 0).all()
    x, W, res = _operands(room, 27, cin, V, V)
    want = oracle.conv(x, W, nbr, V, room["scale"], room["shift"], res, oracle.ACT_RELU)
    for force in ("64,4,3", "32,4,3"):
        got, _ = _launch(gpu, x, W, cm.plan_k3(1), V, room, res, force=force)
        assert np.array_equal(got, want), f"{force}: max abs diff {np.abs(got - want).max()}"


@pytest.mark.parametrize("cin", [384, 416])
def test_offset_range_passes_equal_the_single_launch(gpu, oracle, room, cin):
    """three passes over offsets [0, 9), [9, 18), [18, 27): the accumulators handed over through memory are the C
    operands of the next pass's first matrix ops"""
    from mrcc_amd.sparse import SplitPlan

    cm, V = room["cm"], room["V"]
    sp = cm.plan_k3_split(1, (9, 18))
    assert isinstance(sp, SplitPlan) and [(a, b) for a, b, _ in sp.parts] == [(0, 9), (9, 18), (18, 27)]
    x, W, res = _operands(room, 27, cin, V, V)
    want = _want(oracle, room, "k3", cin, x, W, room["frame"].k3(1), V, res)
    one, _ = _launch(gpu, x, W, cm.plan_k3(1), V, room, res, force="64,4,3")
    for kw in (dict(force="64,4,3"), dict(dispatch=(0.0, 0.5))):
        passes, name = _launch(gpu, x, W, sp, V, room, res, **kw)
        assert name == (MAIN if "force" in kw else DUAL)
        assert np.array_equal(passes, one), f"{kw}: max abs diff {np.abs(passes - one).max()}"
    assert np.array_equal(one, want), f"max abs diff {np.abs(one - want).max()}"
