"""Live per-kernel timing with HIP events on the stream the kernels are launched on (torch's current stream).

bench.py installs a KernelTimer; nn.conv_forward reports each sv_conv_fwd launch to it with the quantities the
roofline needs (kernel offsets K, Cin, Cout, output rows, and the device-side pair count of the plan).  Which launches a
timer restricted to some kernels (`only`) times is decided by asking the library which instance it would launch
(conv_kernel_config); the name a record carries is the one the library reports after the launch.  Nothing is
read back inside the timed region: events and pair counts are resolved after the final synchronize.
"""
import math

import torch

from . import _lib

TIMER = None  # set by bench.py
# Optional list: nn.conv_forward appends (instance name, {"fast", "ring", "full"}, K, Cin, Cout, rows) per launch, as
# reported by the library itself (sv_conv_last_instance) - tests check which instances a configuration really ran on.
INSTANCE_LOG = None
# Optional list: every op of a training step's conv / linear layers (nn.SparseConvFunction) appends (layer, op, entry
# point): layer = the module (None for a plain nn.Linear through nn.linear_train), op "fwd" / "dx" / "dw", entry point the
# library function that ran it ("sv_conv_fwd_acc" / "sv_conv_fwd_bf16" for fwd and dx, "sv_conv_wgrad" / "sv_conv_wgrad_bf16"
# for dw) - tests check which layers a training precision really put on the bf16 kernels.
TRAIN_LOG = None


def conv_kernel_config(Cout, Vpad, Cin, K=1):
    """Name of the kernel instance the library would launch for a layer (sv_conv_select: the dispatch rules themselves,
    asked on the host) as nn.conv_forward calls it: a kernel map has a plan with its tile order and dense rows (K = 1) have
    none, the input allows float4 gathers iff Cin % 4 == 0, every operand is aligned and below the 2 GB buffer extent, the
    launch is a first pass (no acc_init), and the dispatch is this thread's (_lib.conv_dispatch)."""
    flags = _lib.SV_CONV_SEL_BUF_OK | _lib.SV_CONV_SEL_W_ALIGNED
    if K > 1:
        flags |= _lib.SV_CONV_SEL_PLAN | _lib.SV_CONV_SEL_TILE_ORDER
    if Cin % 4 == 0:
        flags |= _lib.SV_CONV_SEL_VEC_A
    return _lib.conv_instance(K, Cin, Cout, Vpad, flags).partition("|")[0]


class KernelTimer:
    def __init__(self, capacity=0):
        self.records = []
        self.enabled = True
        self.only = None  # optional set of kernel names to time (None = all)
        # events are created up front: creating ~250 of them per frame inside the timed region costs milliseconds
        self._pool = [torch.cuda.Event(enable_timing=True) for _ in range(capacity)]
        self._next = 0
        self._first_of_frame = False

    def _event(self):
        if self._next < len(self._pool):
            e = self._pool[self._next]
            self._next += 1
            return e
        return torch.cuda.Event(enable_timing=True)

    def want(self, kernel):
        return self.enabled and (self.only is None or kernel in self.only)

    def start(self):
        e = self._event()
        e.record()
        return e

    def stop(self, start_evt, kernel, K, Cin, Cout, V_out, pairs_dev, level=None, passes=1):
        e = self._event()
        e.record()
        self.records.append((kernel, K, Cin, Cout, V_out, pairs_dev, start_evt, e, self._first_of_frame, level, passes))
        self._first_of_frame = False

    def frame_boundary(self):
        """The next timed launch is the first of a frame: its event interval can absorb the wait for the prepared
        frame (cross-stream) or for the host, so summarize() leaves it out."""
        self._first_of_frame = True

    def clear(self):
        self.records = []

    @staticmethod
    def layer_key(kernel, K, Cin, Cout, V_out, level=None):
        """(kernel instance, layer shape): launches that process the same kind of unit - the same kernel volume and
        channel counts on the same pyramid level, named by the output's tensor stride ("s1", "s2", ...) where the launch
        has a plan; dense layers (no plan, hence no level) by their rows to the nearest power of two ("~2^17": the frames
        of a pool differ by < 1 % in voxel count, pyramid levels by 3-4x)."""
        where = f"s{level}" if level is not None else f"~2^{int(round(math.log2(max(V_out, 1))))}"
        return (kernel, K, Cin, Cout, where)

    def summarize(self, by_layer=False):
        """After torch.cuda.synchronize(): per-kernel {launches, ms, flops, gather_bytes} (SURVEY.md §8d formulas:
        flops = 2 P Cin Cout; gather-bytes = P (4 Cin + 8) + 4 N_out Cout + 4 K Cin Cout).  by_layer: keyed by
        layer_key() instead of the kernel name alone (an instance that serves several layer shapes has no one
        "flops per launch")."""
        out = {}
        for kernel, K, Cin, Cout, V_out, pairs_dev, s, e, first, level, passes in self.records:
            if first:
                continue
            P = int(pairs_dev.item()) if pairs_dev is not None else V_out
            ms = s.elapsed_time(e)
            key = self.layer_key(kernel, K, Cin, Cout, V_out, level) if by_layer else kernel
            d = out.setdefault(key, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0, "rows": 0.0, "kernel_launches": 0})
            d["rows"] += V_out
            d["launches"] += 1  # layers; a layer run as offset-range passes is several kernel launches
            d["kernel_launches"] += passes
            d["ms"] += ms
            d["flops"] += 2.0 * P * Cin * Cout
            d["bytes"] += P * (4.0 * Cin + 8) + 4.0 * V_out * Cout + 4.0 * K * Cin * Cout
        return out


def pass_gflop(fn):
    """Algorithmic GFLOP (2 P Cin Cout per conv / linear layer, P = kernel-map pairs or dense rows) of the
    sv_conv_fwd launches fn() makes - one forward pass's worth, counted by timing it once under a private KernelTimer."""
    global TIMER
    saved, TIMER = TIMER, KernelTimer()
    try:
        fn()
        torch.cuda.synchronize()
        return sum(d["flops"] for d in TIMER.summarize().values()) / 1e9
    finally:
        TIMER = saved
