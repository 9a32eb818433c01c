"""Hostile-environment case of the metric-learning criterion (sv_ms_mine, sv_triplet_margin, sv_mined_triplet_step), in a
file of its own: importing this module registers it in the one table of tests/hostile_cases.py (its `case`), so
tests/test_gpu_hostile_memory.py and tests/test_gpu_side_stream.py run it like every other case and
tests/test_hostile_cpu.py counts its entry points.

The table is complete only once this module has been imported.  tests/test_featurenet_cpu.py imports it, and that file is
collected before the three modules that read the table (pytest collects a directory in name order, every file before any
test runs), so a run of the suite sees the case; a run of tests/test_hostile_cpu.py alone does not, and its completeness
test then names the three entries as "without a case"."""
import numpy as np

from hostile_cases import CASES, _arm, _t, _ws, case

ENTRIES = ("sv_ms_mine", "sv_triplet_margin", "sv_mined_triplet_step")
B, E, EPSILON, MARGIN, MAX_PAIRS = 65, 33, 0.1, 0.05, 40


def _metric_build(gpu):
    import metric_helpers as MH

    x, labels = MH.make_case(B, E, "many", seed=1, pad=0)
    return dict(x=_t(x, gpu), labels=_t(labels, gpu))


def _metric_run(i):
    from mrcc_amd.utils import metric_learning as ML

    x, y = i["x"], i["labels"]
    _arm(i, x, y)
    a1, p, a2, n, counts, nonfinite = ML.mine_call(x, y, EPSILON)
    n_pos, n_neg = counts[:2].tolist()  # entries past the kept counts are not defined
    pairs = (a1[:n_pos], p[:n_pos], a2[:n_neg], n[:n_neg])
    _arm(i, x, *pairs, counts)
    loss = ML.triplet_call(x, *pairs, counts, MARGIN)
    _arm(i, x, y)
    step = ML.mined_step_call(x, y, MAX_PAIRS, EPSILON, MARGIN)
    return pairs + (counts, nonfinite) + tuple(loss) + tuple(step)


def _metric_ref(i, outs):
    import metric_helpers as MH

    x, y = i["x"].cpu().numpy(), i["labels"].cpu().numpy()
    want = MH.miner_ref(x, y, EPSILON)
    assert min(MH.miner_margins(x, y, EPSILON)) > 1e-9
    for got, w in zip(outs[:4], want):
        assert np.array_equal(got.numpy(), w)
    assert outs[4].tolist() == [len(want[0]), len(want[2])] * 2 and int(outs[5]) == 0
    for tup, (sums, grad, n_triplets), cap in ((want, outs[6:9], None), (want, (outs[10], outs[11], outs[13]), MAX_PAIRS)):
        ref = MH.loss_ref(x, tuple(t[:cap] for t in tup), MARGIN)
        assert ref["margin"] > 1e-9 and ref["nonzero"] > 0
        assert MH.sums_close(float(sums[0]), ref["sum"]) and float(sums[1]) == ref["nonzero"] and int(n_triplets) == ref["n_triplets"]
        assert bool((np.abs(grad.double().numpy() - ref["grad_sum"]) <= MH.grad_bound(ref["grad_sum"])).all())
    assert int(outs[9]) == 0 and outs[12].tolist() == [MAX_PAIRS, MAX_PAIRS, len(want[0]), len(want[2])] and int(outs[14]) == 0


if not any(c.name == "metric_criterion" for c in CASES):  # once, however often the module is loaded
    case("metric_criterion", list(ENTRIES), _metric_build, _metric_run, late=("x", "labels"), reference=_metric_ref, steps=3,
         workspace=lambda i: [_ws("sv_metric_workspace_bytes", B, E)])
