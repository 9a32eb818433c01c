"""Every launching entry point on a side stream, behind inputs that arrive late (tests/hostile_helpers.py late_inplace).

Before EVERY wrapper call of a case (the `_arm` steps of tests/hostile_cases.py) the tensors that call reads - the case's
inputs, or what an earlier call of the run produced - are poisoned in place and restored on a fresh torch.cuda.Stream()
behind a measured 5 to 20 ms of torch matmuls; the wrapper is called inside `with torch.cuda.stream(stream)` right after
that was enqueued, so a read-back inside an earlier call does not use up a later call's delay.  A launch, memset or copy
that went to the null stream reads the poison and the result differs from the default-stream baseline; a control clone on
the default stream proves at every step that the poison was still there to be read.  The stream is one whose work really
runs beside the null stream's (hostile_helpers.side_stream).  Results are copied to the host on the side stream after
stream.synchronize() alone.  Wrappers that take host arrays run behind the same delay.  The whole networks run twice, on
two different side streams chosen beforehand, with the same inputs object and no device-wide wait between the turns (the
evaluation network and the engine share their model and its caches across the turns; the two training cases copy the
model inside run, so their turns share none); the
engine streaming case runs in hostile memory on a side stream as well."""
import pytest
import torch

import hostile_helpers as HH
from hostile_cases import CASES

pytestmark = pytest.mark.gpu


def _enqueue(case, inputs, stream, lates, device_sync=True):
    """the case on `stream`, every step behind its own delay -> its results, still on the device"""
    def arm(tensors, fills):
        lates.append(HH.late_inplace(stream, tensors, fills, device_sync))

    with torch.cuda.stream(stream):
        lates.append(HH.late_inplace(stream, [inputs[k] for k in case.late], [case.poison.get(k) for k in case.late], device_sync))
        return HH.run_case(case, dict(inputs, _arm=arm))


def _collect(stream, outs):
    stream.synchronize()  # this stream alone: what was enqueued on it is done, nothing else is waited for
    with torch.cuda.stream(stream):
        return HH.to_host(outs)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_side_stream(gpu, case):
    want = HH.baseline(case, gpu)
    inputs = case.build(gpu)
    lates = []
    try:
        first = HH.side_stream(gpu)
        if not case.network:
            got = [_collect(first, _enqueue(case, inputs, first, lates))]
        else:  # again on another stream with the same model object; nothing device-wide is waited for in between
            second = HH.side_stream(gpu, avoid=[first])
            again = dict(inputs, **{k: inputs[k].clone() for k in case.late})
            torch.cuda.synchronize()
            outs = [_enqueue(case, inputs, first, lates), _enqueue(case, again, second, lates, device_sync=False)]
            got = [_collect(s, o) for s, o in zip((first, second), outs)]
        for late in lates:
            late.check()
        assert len(lates) >= case.steps, f"{case.name}: {len(lates)} delays for {case.steps} wrapper calls"
        for turn, g in enumerate(got):
            HH.assert_same_bits(g, want, f"{case.name}, side stream, turn {turn}")
    finally:
        if case.cleanup is not None:
            case.cleanup(inputs)


def test_engine_stream_in_hostile_memory_on_a_side_stream(gpu, monkeypatch):
    case = next(c for c in CASES if c.name == "engine_stream")
    want = HH.baseline(case, gpu)
    inputs = case.build(gpu)
    lates = []
    try:
        stream = HH.side_stream(gpu)
        with HH.hostile_memory(0xFF, monkeypatch=monkeypatch):
            got = _collect(stream, _enqueue(case, inputs, stream, lates))
        lates[0].check()
        HH.assert_same_bits(got, want, "engine_stream, hostile memory on a side stream")
    finally:
        case.cleanup(inputs)
