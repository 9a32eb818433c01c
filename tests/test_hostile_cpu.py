"""The harness of the hostile-environment tests, checked without a GPU (tests/hostile_helpers.py): the memory shim on CPU
tensors (its device filter is a parameter), the guard check, the bit comparison, the call-counting proxies, and the
completeness of the case table against _lib.SIGNATURES."""
import ctypes
import types

import numpy as np
import pytest
import torch

import hostile_helpers as HH


def always(t):
    return True


def _overrun(t, byte_offset):
    """write one byte at `byte_offset` from the tensor's first byte, as a kernel that leaves its buffer would"""
    ctypes.memset(t.data_ptr() + byte_offset, 0x11, 1)


@pytest.mark.parametrize("offset_of", [lambda n: -1, lambda n: n, lambda n: n + 511, lambda n: -512])
def test_a_byte_outside_the_tensor_is_reported_with_site_and_offset(monkeypatch, offset_of):
    with pytest.raises(AssertionError) as err:
        with HH.hostile_memory(0x5A, monkeypatch=monkeypatch, want=always):
            torch.empty(40, dtype=torch.float32)
            t = torch.empty((3, 7), dtype=torch.float64)  # the culprit's allocation: this line
            line = _line() - 1
            torch.empty(5, dtype=torch.uint8)
            _overrun(t, offset_of(t.numel() * 8))
    msg = str(err.value)
    assert f"test_hostile_cpu.py:{line}" in msg, msg
    assert "168 bytes" in msg and f"offset {offset_of(168)} " in msg and "0x11" in msg and "0x5a" in msg, msg


def _line():
    import sys

    return sys._getframe(1).f_lineno


def test_writes_inside_the_tensor_leave_the_guards_alone(monkeypatch):
    with HH.hostile_memory(0xFF, monkeypatch=monkeypatch, want=always) as block:
        t = torch.empty((4, 4), dtype=torch.int32)
        assert (t == -1).all()  # 0xFF bytes: -1 as an index
        f = torch.empty(8, dtype=torch.float32)
        assert torch.isnan(f).all()  # and a NaN as a float
        t.zero_()
        f.fill_(1.0)
        _overrun(t, 0)
        _overrun(t, 63)
    assert [r.nbytes for r in block.records] == [64, 32]


def test_the_patch_is_gone_after_the_block_even_when_it_raises(monkeypatch):
    before = (torch.empty, torch.empty_like)
    with pytest.raises(RuntimeError):
        with HH.hostile_memory(0x5A, monkeypatch=monkeypatch, want=always):
            assert torch.empty is not before[0]
            raise RuntimeError("inside")
    assert (torch.empty, torch.empty_like) == before


def _toy_kernel(out, x):
    """a numpy "kernel" that forgets the last element of its output"""
    out.numpy()[:-1] = x.numpy()[:-1] * 2


def test_an_unwritten_output_element_differs_between_the_fills_and_is_flagged(monkeypatch):
    x = torch.arange(16, dtype=torch.float32)
    results = []
    for fill in (0xFF, 0x5A):
        with HH.hostile_memory(fill, monkeypatch=monkeypatch, want=always):
            out = torch.empty(16, dtype=torch.float32)
            _toy_kernel(out, x)
            results.append(out.clone())
    baseline = torch.zeros(16)  # what fresh memory usually holds: the bug passes a plain test
    _toy_kernel(baseline, x)
    assert np.array_equal(HH.as_bits(results[0])[:-1], HH.as_bits(results[1])[:-1])
    for got in results:
        with pytest.raises(AssertionError, match="first at flat index 15"):
            HH.assert_same_bits((got,), (baseline,), "toy kernel")
    HH.assert_same_bits((results[0][:-1],), (baseline[:-1],), "toy kernel, defined part")


def test_bit_comparison_tells_nan_payloads_and_signed_zeros_apart():
    a = torch.tensor([0.0, float("nan")])
    b = torch.tensor([-0.0, float("nan")])
    c = a.clone()
    c.view(torch.int32)[1] |= 1  # another NaN payload
    HH.assert_same_bits((a, None), (a.clone(), None), "same")
    for other in (b, c):
        with pytest.raises(AssertionError):
            HH.assert_same_bits((a,), (other,), "differs")
    with pytest.raises(AssertionError, match="dtype"):
        HH.assert_same_bits((a,), (a.double(),), "dtype")
    with pytest.raises(AssertionError, match="shape"):
        HH.assert_same_bits((a,), (a[:1],), "shape")


@pytest.mark.parametrize("call,shape", [
    (lambda e: e((5,), dtype=torch.uint8), (5,)), (lambda e: e(5, dtype=torch.uint8), (5,)),
    (lambda e: e((3, 4), dtype=torch.float32, device="cpu"), (3, 4)), (lambda e: e(3, 4, dtype=torch.int64), (3, 4)),
    (lambda e: e(7, dtype=torch.float64, device=torch.device("cpu")), (7,)), (lambda e: e((2, 3, 5), dtype=torch.int32), (2, 3, 5)),
    (lambda e: e(6, dtype=torch.bfloat16), (6,)), (lambda e: e(size=(4, 2), dtype=torch.float32), (4, 2)),
    (lambda e: e(9), (9,)), (lambda e: e((2, 2), dtype=torch.float32, requires_grad=True), (2, 2))])
def test_every_call_form_the_package_uses_comes_back_right(monkeypatch, call, shape):
    plain = call(torch.empty)
    with HH.hostile_memory(0x5A, monkeypatch=monkeypatch, want=always) as block:
        t = call(torch.empty)
        like = torch.empty_like(t)
    for got in (t, like):
        assert tuple(got.shape) == shape and got.dtype == plain.dtype and got.device == plain.device
        assert got.is_contiguous() and got.data_ptr() % 16 == 0
        assert (HH.as_bits(got).view(np.uint8) == 0x5A).all()
    assert t.requires_grad == plain.requires_grad
    assert len(block.records) == 2 and all(r.parent.numel() == r.nbytes + 2 * HH.GUARD for r in block.records)


def test_results_the_shim_must_leave_alone(monkeypatch):
    with HH.hostile_memory(0x5A, monkeypatch=monkeypatch, want=always) as block:
        assert torch.empty(0, dtype=torch.float32).numel() == 0
        assert torch.empty((0, 3)).shape == (0, 3)
        cl = torch.empty((2, 3, 4, 5), memory_format=torch.channels_last)
        assert cl.is_contiguous(memory_format=torch.channels_last)
        buf = torch.zeros(4)
        assert torch.empty(4, out=buf) is buf
        base = torch.zeros(4, 6).t()  # not contiguous: empty_like preserves the strides
        assert torch.empty_like(base).stride() == base.stride()
    assert block.records == []
    with HH.hostile_memory(0x5A, monkeypatch=monkeypatch) as block:  # the default filter: GPU tensors only
        assert not (HH.as_bits(torch.zeros(3) + torch.empty(3).fill_(0)) != 0).any()
    assert block.records == []
    with pytest.raises(ValueError):
        with HH.hostile_memory(0x5A, guard=100, monkeypatch=monkeypatch):
            pass


def _fake_lib():
    calls = []
    lib = types.SimpleNamespace()

    def sv_a(x):
        calls.append(("a", x))
        return 0

    def sv_b(x):
        calls.append(("b", x))
        return -5

    sv_a.restype = sv_b.restype = ctypes.c_int
    sv_a.argtypes = sv_b.argtypes = [ctypes.c_int]
    lib.sv_a, lib.sv_b = sv_a, sv_b
    return lib, calls, (sv_a, sv_b)


def test_entry_calls_counts_forwards_and_restores():
    lib, calls, originals = _fake_lib()
    with HH.entry_calls(lib, ["sv_a", "sv_b"]) as counts:
        assert lib.sv_a is not originals[0] and lib.sv_a.__wrapped__ is originals[0]
        assert lib.sv_a(3) == 0 and lib.sv_a(4) == 0 and lib.sv_b(5) == -5
        assert originals[0].argtypes == [ctypes.c_int] and originals[0].restype is ctypes.c_int  # untouched
    assert counts == {"sv_a": 2, "sv_b": 1} and counts.ok == {"sv_a": 2}
    assert counts.missing(["sv_a", "sv_b"]) == ["sv_b"]  # reached, but never with SV_OK
    assert calls == [("a", 3), ("a", 4), ("b", 5)]
    assert (lib.sv_a, lib.sv_b) == originals


def test_entry_calls_takes_every_function_of_a_given_library_by_default():
    lib, _, originals = _fake_lib()
    with HH.entry_calls(lib) as counts:
        lib.sv_b(2)
    assert counts == {"sv_a": 0, "sv_b": 1} and (lib.sv_a, lib.sv_b) == originals


def test_poison_in_place_keeps_to_the_tensor_it_is_given():
    base = torch.zeros(4, 6)
    HH.poison_(base[:, 1])  # a strided column
    assert torch.isnan(base[:, 1]).all() and (base[:, 0] == 0).all() and (base[:, 2:] == 0).all()
    idx = torch.ones(5, dtype=torch.int64)
    HH.poison_(idx)
    assert (idx == 0).all()
    HH.poison_(idx, -1)
    assert (idx == -1).all()
    f, d, u, tab = torch.zeros(3), torch.zeros(3, dtype=torch.float64), torch.zeros(4, dtype=torch.uint8), torch.ones(4, dtype=torch.float64)
    for t in (f, d, u):
        HH.poison_(t)
    assert (HH.as_bits(f) == 0xFFFFFFFF).all() and torch.isnan(d).all() and (u == 255).all()
    HH.poison_(tab, 0)
    assert (tab == 0).all()


def test_entry_calls_restores_when_the_block_raises():
    lib, _, originals = _fake_lib()
    with pytest.raises(KeyError):
        with HH.entry_calls(lib, ["sv_a", "sv_b"]):
            lib.sv_a(1)
            raise KeyError("inside")
    assert (lib.sv_a, lib.sv_b) == originals


def test_entry_calls_on_the_loaded_library():
    """the real library object: a proxied size query returns what the function returns, and the proxies are gone after"""
    from mrcc_amd import _lib

    lib = _lib.load()
    before = {n: getattr(lib, n) for n in _lib.SIGNATURES}
    want = lib.sv_plan_workspace_bytes(1000)
    with HH.entry_calls() as counts:
        assert lib.sv_plan_workspace_bytes(1000) == want and lib.sv_abi_version() == _lib.ABI_VERSION
        assert _lib.conv_tiles()  # a wrapper that goes through getattr(lib, name)
    assert counts["sv_plan_workspace_bytes"] == 1 and counts["sv_abi_version"] == 1 and counts["sv_conv_tile_info"] > 1
    assert counts.ok.get("sv_abi_version", 0) == 0  # not a status: 4 is the ABI version
    assert all(getattr(lib, n) is f for n, f in before.items())


def test_every_launching_entry_point_has_a_case():
    """the union of the cases' entries is _lib.SIGNATURES minus the size queries and the host-only calls: an entry point
    added without a case fails here"""
    from mrcc_amd import _lib

    covered = set()
    for c in HH.CASES:
        assert c.name and callable(c.build) and callable(c.run)
        unknown = set(c.entries) - set(_lib.SIGNATURES)
        assert not unknown, (c.name, unknown)
        covered |= set(c.entries)
        assert set(c.poison) <= set(c.late), c.name
    assert set(HH.HOST_ONLY) <= set(_lib.SIGNATURES)
    want = HH.launching_entries(_lib.SIGNATURES)
    assert covered == want, f"without a case: {sorted(want - covered)}; not launching: {sorted(covered - want)}"
    names = [c.name for c in HH.CASES]
    assert len(set(names)) == len(names)
