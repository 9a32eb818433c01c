"""Every launching entry point in dirty, guarded memory (tests/hostile_helpers.py, tests/hostile_cases.py).

Each case runs on the default stream: plain (the baseline, held to the case's independent reference and repeated once),
then with torch.empty / torch.empty_like handing out memory full of 0xFF bytes (SV_EMPTY_KEY, a NaN as a float, -1 as an
index), of 0x5A bytes, and of 0xFF again once the allocator hands back the blocks that held 0x5A.  Every returned
tensor must equal the baseline bit for bit, every guard byte around every allocation must be intact, the case must have
reached its entry points inside the hostile block, and the block must hold an allocation of exactly the size each of the
case's *_workspace_bytes contracts returns.  No tolerance anywhere."""
import pytest
import torch

import hostile_helpers as HH
from hostile_cases import CASES

pytestmark = pytest.mark.gpu

FILLS = (("fill 0xFF", 0xFF), ("fill 0x5A", 0x5A), ("fill 0xFF over recycled 0x5A blocks", 0xFF))


def hostile_run(case, inputs, monkeypatch, fill, want, label):
    with HH.entry_calls() as calls, HH.hostile_memory(fill, monkeypatch=monkeypatch) as block:
        got = HH.to_host(HH.run_case(case, inputs))  # the copy to the host waits for the results
        sizes = set(block.sizes())
        need = [n for n in case.workspace(inputs) if n > 0] if case.workspace is not None else []
    HH.assert_same_bits(got, want, f"{case.name}, {label}")
    assert not calls.missing(case.entries), f"{case.name}, {label}: never reached {calls.missing(case.entries)}"
    lost = [n for n in need if n not in sizes]
    assert not lost, (f"{case.name}, {label}: no allocation of {lost} bytes, the size its *_workspace_bytes contract returns, "
                      f"went through torch.empty ({len(sizes)} distinct sizes did)")
    assert block.records, f"{case.name}, {label}: nothing was allocated through torch.empty"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_hostile_memory(gpu, monkeypatch, case):
    want = HH.baseline(case, gpu)
    built = []
    try:
        for label, fill in FILLS:
            if not built or not case.network:  # a network object is built once: its caches live across the fills
                built.append(case.build(gpu))
            hostile_run(case, built[-1], monkeypatch, fill, want, label)
            torch.cuda.synchronize()
    finally:
        if case.cleanup is not None:
            for inputs in built:
                case.cleanup(inputs)
