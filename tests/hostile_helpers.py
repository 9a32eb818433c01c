"""Harness of the hostile-environment tests: every launching entry point of the library run in dirty, guarded memory
(hostile_memory), counted at the C ABI (entry_calls) and on a side stream behind inputs that arrive late (late_inplace).

  hostile_memory(fill, guard, monkeypatch=...)  torch.empty / torch.empty_like hand out the middle of a larger uint8 block
        whose every byte holds `fill`; on exit the guard bytes on both sides must still hold it.
  entry_calls()                                 counting proxies in front of the loaded library's functions.
  late_inplace(stream, tensors)                 what the next wrapper call reads holds poison until a delay on `stream` has passed.
  side_stream(device)                           a fresh stream that really runs beside the default stream.
  CASES (hostile_cases.py)                      one table of (name, entries, build, run) for both GPU test modules.
"""
import contextlib
import ctypes
import math
import os
import sys

import numpy as np
import torch

GUARD = 512
_HERE = os.path.abspath(__file__)
_TORCH_DIR = os.path.dirname(os.path.abspath(torch.__file__))
ROOT = os.path.dirname(os.path.dirname(_HERE))


# ---------------------------------------------------------------------------------------------------------------------
# hostile memory
# ---------------------------------------------------------------------------------------------------------------------
def on_gpu(t):
    return t.is_cuda


def _call_site():
    """file:line of the nearest caller outside this file and outside torch (the allocation's call site)"""
    f = sys._getframe(2)
    while f is not None:
        name = os.path.abspath(f.f_code.co_filename)
        if name != _HERE and not name.startswith(_TORCH_DIR) and "contextlib" not in name:
            return f"{os.path.relpath(name, ROOT)}:{f.f_lineno}"
        f = f.f_back
    return "<unknown>"


class Allocation:
    __slots__ = ("parent", "nbytes", "site")

    def __init__(self, parent, nbytes, site):
        self.parent, self.nbytes, self.site = parent, nbytes, site


class HostileBlock:
    """what `with hostile_memory(...) as block` yields: the allocations made so far (parents stay alive until exit)"""

    def __init__(self, fill, guard):
        self.fill, self.guard, self.records = fill, guard, []

    def sizes(self):
        return [r.nbytes for r in self.records]

    def check_guards(self):
        """AssertionError naming the call site, size and offset (relative to the tensor's first byte) of the first guard
        byte that no longer holds the fill"""
        g = self.guard
        for r in self.records:
            p = r.parent
            for base, part in ((-g, p[:g]), (r.nbytes, p[g + r.nbytes:])):
                bad = part != self.fill
                if bool(bad.any()):
                    first = int(bad.nonzero()[0, 0])
                    raise AssertionError(
                        f"guard byte overwritten: allocation of {r.nbytes} bytes at {r.site}, offset {base + first} "
                        f"(0 = the tensor's first byte, {r.nbytes} = one past its end) holds "
                        f"0x{int(part[first]):02x}, not the fill 0x{self.fill:02x}")


def _plain(kw):
    fmt = kw.get("memory_format")
    return ("out" not in kw and kw.get("layout") in (None, torch.strided)
            and fmt in (None, torch.contiguous_format, torch.preserve_format))


@contextlib.contextmanager
def hostile_memory(fill, guard=GUARD, *, monkeypatch, want=on_gpu):
    """Replace torch.empty and torch.empty_like (through the test's monkeypatch) for the block: a result that `want`
    accepts (default: GPU tensors) becomes the middle of a uint8 block of guard + nbytes + guard bytes that all hold
    `fill`, viewed as the requested dtype and shape.  On exit every guard must be intact (HostileBlock.check_guards)."""
    if not (0 <= fill <= 255) or guard <= 0 or guard % 512:
        raise ValueError("fill is one byte; guard a positive multiple of 512 (the alignment torch gives is kept)")
    orig_empty, orig_like = torch.empty, torch.empty_like
    block = HostileBlock(fill, guard)

    def dirty(t, kw):
        if not want(t) or t.numel() == 0 or not _plain(kw) or not t.is_contiguous():
            return t
        nbytes = t.numel() * t.element_size()
        parent = orig_empty(guard + nbytes + guard, dtype=torch.uint8, device=t.device)
        parent.fill_(fill)
        out = parent[guard:guard + nbytes].view(t.dtype).view(t.shape)
        # include/sv_hip.h: plan arrays and the conv operands are read with 16-byte accesses
        assert out.data_ptr() % 16 == 0 and out.data_ptr() == parent.data_ptr() + guard, "the shim lost the alignment"
        assert out.is_contiguous() and out.dtype == t.dtype and out.shape == t.shape and out.device == t.device
        if t.requires_grad:
            out.requires_grad_(True)
        block.records.append(Allocation(parent, nbytes, _call_site()))
        return out

    def empty(*args, **kw):
        return dirty(orig_empty(*args, **kw), kw)

    def empty_like(*args, **kw):
        return dirty(orig_like(*args, **kw), kw)

    with monkeypatch.context() as m:
        m.setattr(torch, "empty", empty)
        m.setattr(torch, "empty_like", empty_like)
        yield block
    if torch.cuda.is_available() and any(r.parent.is_cuda for r in block.records):
        torch.cuda.synchronize()
    block.check_guards()


# ---------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------
def as_bits(t):
    """a tensor or array as a flat host array of integers of its element size (NaN payloads and signed zeros count)"""
    a = t.detach().cpu().contiguous() if torch.is_tensor(t) else np.ascontiguousarray(t)
    if torch.is_tensor(a):
        if a.dtype == torch.bfloat16:
            a = a.view(torch.int16)
        elif a.dtype == torch.bool:
            a = a.view(torch.uint8)
        a = a.numpy()
    a = a.reshape(-1)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_same_bits(got, want, what):
    """tuples of tensors equal bit for bit, element by element; the message names the tensor and the first difference"""
    assert len(got) == len(want), f"{what}: {len(got)} results, the baseline has {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        if g is None or w is None:
            assert g is None and w is None, f"{what}: result {i} is None on one side only"
            continue
        assert tuple(g.shape) == tuple(w.shape), f"{what}: result {i} has shape {tuple(g.shape)}, baseline {tuple(w.shape)}"
        assert g.dtype == w.dtype, f"{what}: result {i} has dtype {g.dtype}, baseline {w.dtype}"
        gb, wb = as_bits(g), as_bits(w)
        diff = np.nonzero(gb != wb)[0]
        assert len(diff) == 0, (f"{what}: result {i} {tuple(g.shape)} {g.dtype} differs from the baseline in {len(diff)} of "
                                f"{len(gb)} elements, first at flat index {int(diff[0])}: 0x{int(gb[diff[0]]):x} != "
                                f"0x{int(wb[diff[0]]):x}")


def to_host(outs):
    return tuple(None if t is None else t.detach().cpu() for t in outs)


# ---------------------------------------------------------------------------------------------------------------------
# entry points reached
# ---------------------------------------------------------------------------------------------------------------------
class EntryCounts(dict):
    """{name: calls}; .ok = {name: calls that returned SV_OK} for the entries that return a status"""

    def __init__(self, *a):
        super().__init__(*a)
        self.ok = {}

    def missing(self, entries):
        """the entries of a case that were not reached with a call that returned SV_OK"""
        return [n for n in entries if self.ok.get(n, 0) == 0]


@contextlib.contextmanager
def entry_calls(lib=None, names=None):
    """Counting proxies in front of the functions `names` (default: every key of _lib.SIGNATURES) of the loaded library
    object (default: _lib.load()).  Yields {name: calls}.  A proxy calls the bound ctypes function it wraps - restype and
    argtypes stay where they were set - and the originals are back on exit, also when the block raises."""
    if lib is None:
        from mrcc_amd import _lib

        lib, names = _lib.load(), (list(_lib.SIGNATURES) if names is None else names)
    elif names is None:
        names = [n for n in vars(lib) if n.startswith("sv_") and callable(getattr(lib, n))]
    originals = {n: getattr(lib, n) for n in names}
    counts = EntryCounts((n, 0) for n in names)

    def proxy_of(name, fn):
        def proxy(*args):
            counts[name] += 1
            rc = fn(*args)
            if getattr(fn, "restype", None) is ctypes.c_int and rc == 0:
                counts.ok[name] = counts.ok.get(name, 0) + 1  # a status-returning entry that went through (SV_OK)
            return rc

        proxy.__name__ = name
        proxy.__wrapped__ = fn
        return proxy

    try:
        for n, fn in originals.items():
            setattr(lib, n, proxy_of(n, fn))
        yield counts
    finally:
        for n, fn in originals.items():
            setattr(lib, n, fn)


HOST_ONLY = ("sv_abi_version", "sv_last_error", "sv_conv_last_instance", "sv_conv_select", "sv_conv_tile_info",
             "sv_conv_set_dispatch")
SIZE_SUFFIXES = ("_workspace_bytes", "_arena_bytes", "_scratch_bytes")


def launching_entries(signatures):
    """the entry points a case must reach: every function of the table but the size queries and the host-only calls"""
    return {n for n in signatures if not n.endswith(SIZE_SUFFIXES) and n not in HOST_ONLY}


# ---------------------------------------------------------------------------------------------------------------------
# side stream
# ---------------------------------------------------------------------------------------------------------------------
DELAY_MS = (5.0, 20.0)
_delay = {}


def _chain(a, b, count):
    x = a
    for _ in range(count):
        x = x @ b
    return x


def _time_chain(a, b, count, stream):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        start.record()
        _chain(a, b, count)
        stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def delay_chain(device):
    """(a, b, count, measured ms): a chain of `count` torch matmuls that keeps a stream busy for a measured time inside
    DELAY_MS.  Measured with events once per process and device; nothing is hard-coded but the target."""
    key = torch.device(device).index or 0
    if key not in _delay:
        n = 2048
        a = torch.full((n, n), 1.0 / n, dtype=torch.float32, device=device)  # a @ a = a: the values stay finite
        b = a.clone()
        s = torch.cuda.Stream(device)
        torch.cuda.synchronize()
        _time_chain(a, b, 8, s)  # warm-up: the GEMM kernel's first launch loads its code
        per = max(_time_chain(a, b, 16, s) / 16, 1e-4)
        target = math.sqrt(DELAY_MS[0] * DELAY_MS[1])
        count = max(int(math.ceil(target / per)), 1)
        ms = _time_chain(a, b, count, s)
        if not DELAY_MS[0] <= ms <= DELAY_MS[1]:  # one correction from the chain's own time
            count = max(int(round(count * target / max(ms, 1e-3))), 1)
            ms = _time_chain(a, b, count, s)
        assert DELAY_MS[0] <= ms <= DELAY_MS[1], f"the delay chain of {count} matmuls took {ms:.2f} ms, outside {DELAY_MS}"
        _delay[key] = (a, b, count, ms)
    return _delay[key]


class Late:
    """late_inplace's result: the control clone and the poison it must have read; .check() after the run"""

    def __init__(self, control, poison, delay_ms):
        self._control, self._poison, self.delay_ms = control, poison, delay_ms

    def saw_poison(self):
        torch.cuda.synchronize()
        return bool((as_bits(self._control) == as_bits(self._poison)).all())

    def check(self):
        """the control clone, issued on the default stream right after the delay and the copies were enqueued on the side
        stream, must have read the poison: only then would a launch on the wrong stream have read it too"""
        assert self.saw_poison(), "the delay did not outlast the launch; this run proves nothing"


def poison_(t, value=None):
    """Poison written into t itself (any strides).  Default: 0xFF bytes for floats and bytes (a NaN as a float), 0 for
    int32 / int64 tensors, which the entry points read as indices, offsets or counts: in bounds for whatever they index.
    value: the fill where a case needs another one (-1 where an entry defines it as "absent"; 0 for a float table whose
    entries a kernel turns into offsets)."""
    if value is not None:
        t.fill_(value)
    elif t.dtype in (torch.int32, torch.int64, torch.int16):
        t.fill_(0)
    elif t.is_contiguous() and t.dtype != torch.bool:
        t.view(torch.uint8).fill_(0xFF)
    else:
        t.fill_(float("nan") if t.is_floating_point() else 255)


def late_inplace(stream, tensors, fills=None, device_sync=True):
    """The side-stream harness, armed before every wrapper call of a run: whatever that call reads - a case's inputs, or
    tensors an earlier call of the run produced - is saved, poisoned in place (fills: one value per tensor where poison_'s
    default is not right) and restored on `stream` behind the delay chain; then a control clone of the harness's own
    sentinel is issued on the default stream, which must still read the poison (Late.check).  device_sync=False orders the poison
    before the control with an event in place of a device-wide wait (nothing else is waited for).  -> Late (check later)."""
    device = stream.device
    a, b, count, ms = delay_chain(device)
    fills = list(fills) if fills is not None else [None] * len(tensors)
    with torch.cuda.stream(stream):
        targets = [torch.arange(1, 1025, dtype=torch.float32, device=device)] + list(tensors)
        saved = [t.clone() for t in targets]
        for t, f in zip(targets, [None] + fills):
            poison_(t, f)
        poison = targets[0].clone()
        if device_sync:
            torch.cuda.synchronize()
        else:
            ready = torch.cuda.Event()
            ready.record(stream)
        _chain(a, b, count)
        for t, s_ in zip(targets, saved):
            t.copy_(s_)
    with torch.cuda.stream(torch.cuda.default_stream(device)):
        if not device_sync:
            torch.cuda.default_stream(device).wait_event(ready)
        control = targets[0].clone()
    return Late(control, poison, ms)


def side_stream(device, avoid=(), tries=16):
    """A fresh torch.cuda.Stream() on which work really runs beside the default stream.  Some fresh streams run in
    submission order with the null stream: a launch on the wrong stream would then wait for the delay like a right one,
    and the experiment could show nothing.  So a candidate is taken only if the harness's own control - a clone on the
    default stream behind a delay on the candidate - reads the poison; every later use checks the same again.
    avoid: streams the new one must differ from."""
    for _ in range(tries):
        s = torch.cuda.Stream(device)
        if any(s.cuda_stream == a.cuda_stream for a in avoid):
            continue
        if late_inplace(s, []).saw_poison():
            return s
    raise AssertionError(f"none of {tries} fresh streams ran beside the default stream: no side-stream experiment is possible")


# ---------------------------------------------------------------------------------------------------------------------
# the case table and what both GPU modules do with a case
# ---------------------------------------------------------------------------------------------------------------------
def __getattr__(name):
    if name == "CASES":
        from hostile_cases import CASES

        return CASES
    raise AttributeError(name)


_baselines = {}


def run_case(case, inputs):
    """case.run as a tuple of tensors"""
    outs = case.run(inputs)
    assert isinstance(outs, tuple) and all(t is None or torch.is_tensor(t) for t in outs), "run returns a tuple of tensors"
    return outs


def baseline(case, gpu):
    """The plain run on the default stream, as host tensors: computed once per process from inputs of its own, held to the
    case's independent reference, shared by both modules and never changed.  A second plain run on the same inputs must
    repeat it bit for bit (a difference is a finding about the kernel, not about memory or streams)."""
    if case.name not in _baselines:
        inputs = case.build(gpu)
        try:
            first = to_host(run_case(case, inputs))
            torch.cuda.synchronize()
            if case.reference is not None:
                case.reference(inputs, first)
            assert_same_bits(to_host(run_case(case, inputs)), first, f"{case.name}: two plain runs")
        finally:
            if case.cleanup is not None:
                case.cleanup(inputs)
        _baselines[case.name] = first
    return _baselines[case.name]
