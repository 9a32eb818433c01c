"""FeatureNet's criterion and the key-point PointNet without a GPU: the N10 section declared, exported and bound; the host
argument checks of its three entries (each returns -1 with a message before any HIP call); the miner reference of
tests/metric_helpers.py held to the per-pair definition, and the cases of the GPU tests held to their margin preconditions;
the loss reference held to torch's own triplet loss; PointNet against the fixture recorded from the reference."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import metric_helpers as MH
import metric_hostile_cases as MC  # registers the criterion's case in the hostile-environment table (see its docstring)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N10 = ["sv_metric_workspace_bytes", "sv_ms_mine", "sv_triplet_margin", "sv_mined_triplet_step"]


def _lib():
    import mrcc_amd

    return mrcc_amd._lib.load()


def test_symbols_declared_exported_and_bound():
    import mrcc_amd
    import hostile_helpers as HH

    text = open(os.path.join(ROOT, "include", "sv_hip.h")).read()
    assert "N10" in text and "metric-learning criterion" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib()
    for name in N10:
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in include/sv_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in mrcc_amd._lib.SIGNATURES
    assert lib.sv_abi_version() == 4
    # two [B][E] float64 copies and the [B][B] matrices: 3 float64 and 3 int32 ones
    assert lib.sv_metric_workspace_bytes(256, 512) >= 2 * 256 * 512 * 8 + 256 * 256 * (3 * 8 + 3 * 4)
    assert lib.sv_metric_workspace_bytes(256, 512) < 8 << 20
    assert set(MC.ENTRIES) <= {e for c in HH.CASES for e in c.entries}


def test_host_argument_checks_reach_no_device():
    lib = _lib()
    a = ctypes.c_void_p(256)  # never dereferenced: every call below fails its host checks
    big = ctypes.c_size_t(1 << 30)

    def mine(x=a, ld=8, B=4, E=8, labels=a, max_pos=-1, max_neg=-1, ws=a, ws_bytes=big, a1=a, p=a, cap_pos=12, a2=a, n=a,
             cap_neg=12, counts=a, nonfinite=a):
        rc = lib.sv_ms_mine(x, ld, B, E, labels, 0.1, max_pos, max_neg, ws, ws_bytes, a1, p, cap_pos, a2, n, cap_neg, counts,
                            nonfinite, None)
        return rc, lib.sv_last_error()

    def loss(x=a, ld=8, B=4, E=8, a1=a, p=a, cap_pos=12, a2=a, n=a, cap_neg=12, counts=a, ws=a, ws_bytes=big, sums=a, grad=None,
             n_triplets=a, n_invalid=a):
        rc = lib.sv_triplet_margin(x, ld, B, E, a1, p, cap_pos, a2, n, cap_neg, counts, 0.05, ws, ws_bytes, sums, grad, n_triplets,
                                   n_invalid, None)
        return rc, lib.sv_last_error()

    def step(x=a, ld=8, B=4, E=8, labels=a, max_pos=-1, max_neg=-1, ws=a, ws_bytes=big, sums=a, counts=a, n_triplets=a,
             nonfinite=a):
        rc = lib.sv_mined_triplet_step(x, ld, B, E, labels, 0.1, 0.05, max_pos, max_neg, ws, ws_bytes, sums, None, counts,
                                       n_triplets, nonfinite, None)
        return rc, lib.sv_last_error()

    shape = (({"B": 0}, b"1 to 1024 embeddings"), ({"B": 1025}, b"1 to 1024 embeddings"), ({"E": 0, "ld": 0}, b"E >= 1"),
             ({"ld": 7}, b"ld >= E"), ({"x": None}, b"null pointer"), ({"ws": None}, b"null pointer"),
             ({"ws_bytes": ctypes.c_size_t(64)}, b"workspace too small"),
             ({"ws_bytes": ctypes.c_size_t(lib.sv_metric_workspace_bytes(4, 8) - 1)}, b"workspace too small"))
    caps = (({"max_pos": -2}, b"caps >= -1"), ({"max_neg": -2}, b"caps >= -1"))
    for fn, name, more in (
            (mine, b"sv_ms_mine", caps + (({"labels": None}, b"null pointer"), ({"counts": None}, b"null pointer"),
                                          ({"nonfinite": None}, b"null pointer"), ({"a1": None}, b"null pointer"),
                                          ({"n": None}, b"null pointer"), ({"cap_pos": -1}, b"capacities >= 0"))),
            (loss, b"sv_triplet_margin", (({"counts": None}, b"null pointer"), ({"sums": None}, b"null pointer"),
                                          ({"n_triplets": None}, b"null pointer"), ({"n_invalid": None}, b"null pointer"),
                                          ({"p": None}, b"null pointer"), ({"a2": None}, b"null pointer"),
                                          ({"cap_neg": -1}, b"capacities"), ({"cap_pos": 1 << 31}, b"capacities"))),
            (step, b"sv_mined_triplet_step", caps + (({"labels": None}, b"null pointer"), ({"sums": None}, b"null pointer"),
                                                     ({"counts": None}, b"null pointer"), ({"n_triplets": None}, b"null pointer"),
                                                     ({"nonfinite": None}, b"null pointer")))):
        for kw, msg in shape + more:
            rc, err = fn(**kw)
            assert rc == -1 and msg in err and name in err, (name, kw, rc, err)


def test_python_layer_refuses_what_it_does_not_support():
    import mrcc_amd  # noqa: F401
    from mrcc_amd._lib import SvHipError
    from mrcc_amd.model.featurenet import get_criterion
    from mrcc_amd.utils import metric_learning as ML

    loss_func, miner = get_criterion()
    assert isinstance(loss_func, ML.TripletMarginLoss) and isinstance(miner, ML.MultiSimilarityMiner)
    assert (loss_func.margin, miner.epsilon) == (0.05, 0.1)  # the library's defaults
    x, y = torch.zeros(4, 3, requires_grad=True), torch.zeros(4, dtype=torch.int32)
    for fn in (lambda: miner(x, y), lambda: loss_func(x, y), lambda: ML.mined_triplet_loss(x, y, 8)):
        with pytest.raises(SvHipError):  # CPU tensors: there is no fallback
            fn()


@pytest.mark.parametrize("epsilon", [0.0, 0.1, 3.0])
@pytest.mark.parametrize("pattern", MH.PATTERNS)
def test_miner_reference_equals_the_per_pair_definition(pattern, epsilon):
    for B, E in ((1, 4), (2, 1), (3, 3), (23, 5), (40, 16)):
        x, y = MH.make_case(B, E, pattern, seed=3)
        x = x[:, :E].copy()
        if B >= 23:
            x[5] = 0.0  # the clamp
            x[7, 1] = np.nan
            x[9, 0] = np.inf
            x[11] = x[2]  # a bitwise duplicate
            y[11] = y[2]
        a1, p, a2, n = MH.miner_ref(x, y, epsilon)
        pos, neg = MH.miner_brute(x, y, epsilon)
        assert set(zip(a1.tolist(), p.tolist())) == pos and len(a1) == len(pos)
        assert set(zip(a2.tolist(), n.tolist())) == neg and len(a2) == len(neg)
        S = MH.similarity(np.where(MH.finite_rows(x)[:, None], x, 0.0))
        for a, b in ((a1, p), (a2, n)):  # anchors ascending, then S ascending, then column ascending
            keys = list(zip(a.tolist(), S[a, b].tolist(), b.tolist()))
            assert keys == sorted(keys)
        if B >= 23:
            assert not ({7, 9} & set(np.concatenate([a1, p, a2, n]).tolist()))  # the NaN and the inf row join no pair
        if epsilon == 3.0:  # every pair of an anchor that has both kinds is hard
            want = MH.all_pairs(y)
            if B < 23 and len(want[0]) and len(want[2]):
                has = lambda a, other: np.isin(a, other)  # noqa: E731
                assert len(a1) == has(want[0], want[2]).sum() and len(a2) == has(want[2], want[0]).sum()


@pytest.mark.parametrize("pattern", MH.PATTERNS)
@pytest.mark.parametrize("B,E", MH.SHAPES)
def test_gpu_cases_clear_their_margins(B, E, pattern):
    """the seeds of the GPU tests, checked where the reference alone is needed"""
    x, y = MH.make_case(B, E, pattern)
    for epsilon in (0.0, 0.1):
        decision, gap = MH.miner_margins(x[:, :E], y, epsilon)
        assert decision > 1e-9 and gap > 1e-9, (decision, gap)


def test_hostile_case_is_capped_below_its_totals():
    x, y = MH.make_case(MC.B, MC.E, "many", seed=1, pad=0)
    a1, _, a2, _ = MH.miner_ref(x, y, MC.EPSILON)
    assert min(len(a1), len(a2)) > MC.MAX_PAIRS and min(MH.miner_margins(x, y, MC.EPSILON)) > 1e-9


def test_loss_reference_matches_torch_triplet_margin_loss():
    """on an explicit triplet list the reference's sum is torch's own F.triplet_margin_loss on normalised embeddings"""
    x, y = MH.make_case(23, 5, "two", seed=4)
    x = x[:, :5]
    tup = MH.all_pairs(y)
    ref = MH.loss_ref(x, tup, 0.05)
    u = torch.from_numpy(MH.normalise(x))
    pi, ni = np.where(tup[0][:, None] == tup[2][None, :])
    each = torch.nn.functional.triplet_margin_loss(u[tup[0][pi]], u[tup[1][pi]], u[tup[3][ni]], margin=0.05, eps=0.0,
                                                   reduction="none")
    assert ref["n_triplets"] == len(pi) and ref["nonzero"] == int((each > 0).sum()) and 0 < ref["nonzero"] < len(pi)
    assert abs(ref["sum"] - float(each.sum())) <= 1e-12 * float(each.sum())
    assert MH.loss_ref(x, tuple(np.zeros(0, np.int64) for _ in range(4)), 0.05)["loss"] == 0.0
    bad = MH.loss_ref(x, (np.append(tup[0], 23), np.append(tup[1], 0), tup[2], tup[3]), 0.05)
    assert bad["n_invalid"] == 1 and bad["sum"] == ref["sum"]


def _pointnet(fix):
    import mrcc_amd  # noqa: F401
    from mrcc_amd.model.pointnet import PointNet

    net = PointNet(in_channel=6, out_channel=7, embedding_channel=int(fix["embedding_channel"]))
    sd = net.state_dict()
    net.load_state_dict({k: torch.from_numpy(fix["w_" + k]) if "w_" + k in fix else sd[k] for k in sd})
    return net.eval()


def test_pointnet_state_dict_keys_are_the_references(golden):
    fix = golden("pointnet_kp")
    keys = bytes(fix["state_dict_keys"]).decode().split("\n")
    assert list(_pointnet(fix).state_dict().keys()) == keys and len(keys) == 38
    from mrcc_amd.model.pointnet import PointNet

    assert PointNet(9, 7).linear1.in_features == 1024  # the trainer's default width


def test_pointnet_matches_the_reference_outputs(golden):
    """B = 3 within 1e-6.  At B = 1 the reference's squeeze() drops the batch dimension and BatchNorm1d refuses the 1-D
    tensor (recorded in the fixture as raises0 = 1): that behaviour is kept, so there is no output to compare."""
    fix = golden("pointnet_kp")
    net = _pointnet(fix)
    for i, B in enumerate((1, 3)):
        x = torch.from_numpy(fix[f"x{i}"])
        assert x.shape == (B, 6, 6)
        if int(fix[f"raises{i}"]):
            with pytest.raises(ValueError):
                net(x)
            continue
        with torch.no_grad():
            got = net(x).numpy()
        assert got.shape == fix[f"out{i}"].shape == (B, 7)
        assert np.abs(got - fix[f"out{i}"]).max() <= 1e-6
    assert int(fix["raises1"]) == 0
