"""Sparse-tensor runtime behind the MinkowskiEngine names the reference uses.

  TensorField(features, coordinates, quantization_mode, minkowski_algorithm, device).sparse() / .new(features)
  SparseTensor(features, coordinates=..., device=...)  / .F .C .slice(field) .cat_slice(field) .decomposed_coordinates
  CoordinateManager: per-frame coordinate maps (stride 1,2,4,...), hash tables, kernel maps and conv plans,
  shared by every tensor derived from one input (what ME calls the coordinate manager).

Reference call sites: app/inference_engine.py:405-417,446-454,540-551; test_segmentation.py:62-72;
train_segmentation.py:78; data/alivev2.py:363.  Everything numeric is a libsvhip.so call (include/sv_hip.h).
"""
import threading
import weakref
from ctypes import c_float, c_int, c_int32, c_int64, c_size_t, c_void_p
from enum import Enum
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import SV_TILE_ROWS, call, ptr, stream_ptr


class SparseTensorQuantizationMode(Enum):
    RANDOM_SUBSAMPLE = 0
    UNWEIGHTED_AVERAGE = 1
    UNWEIGHTED_SUM = 2
    NO_QUANTIZATION = 3


class MinkowskiAlgorithm(Enum):
    DEFAULT = 0
    MEMORY_EFFICIENT = 1
    SPEED_OPTIMIZED = 2


def _round_up(x, m):
    return (x + m - 1) // m * m


def _next_pow2(x):
    p = 1
    while p < x:
        p <<= 1
    return p


class CoordinateMap:
    """Canonical (key-sorted) voxel set at one tensor stride."""

    __slots__ = ("keys", "coords", "V", "stride", "_hash")

    def __init__(self, keys, coords, V, stride):
        self.keys = keys  # int64 tensor holding the uint64 keys, [V]
        self.coords = coords  # int32 [V,4] (batch,x,y,z)
        self.V = V
        self.stride = stride
        self._hash = None

    def hash(self):
        if self._hash is None:
            cap = _next_pow2(max(2 * self.V, 2))
            tkeys = torch.empty(cap, dtype=torch.int64, device=self.keys.device)
            tvals = torch.empty(cap, dtype=torch.int32, device=self.keys.device)
            call("sv_hash_build", ptr(self.keys), c_int64(self.V), ptr(tkeys), ptr(tvals), c_int64(cap), stream_ptr())
            self._hash = (tkeys, tvals, cap)
        return self._hash


BUF_LIMIT = 0x7fff0000 - 4096  # extent (bytes) the buffer-addressed conv instances take (csrc/sv_conv_params.h BUF_LIMIT)


class ConvPlan:
    """Mask-sorted execution plan of one kernel map (include/sv_hip.h sv_plan_build)."""

    __slots__ = ("perm", "nbr_s", "submask", "tile_order", "V_out", "Vpad", "K", "pairs", "cm", "in_stride",
                 "out_stride", "raw", "_chunked")

    def __init__(self, perm, nbr_s, submask, tile_order, V_out, Vpad, K):
        self.perm, self.nbr_s, self.submask, self.tile_order = perm, nbr_s, submask, tile_order
        self.V_out, self.Vpad, self.K = V_out, Vpad, K
        self.pairs = None  # number of (in,out) pairs, filled lazily for roofline accounting
        # set by the coordinate manager for plans of a whole kernel map: what chunks() needs to re-plan a batch range
        self.cm = None
        self.in_stride = self.out_stride = None
        self.raw = None  # (nbr int32[K, ld], ld, mask) - the unsorted kernel map
        self._chunked = {}

    def pairs_device(self):
        """Number of (in, out) pairs of the kernel map as a device scalar (no host sync)."""
        if self.pairs is None:
            self.pairs = (self.nbr_s >= 0).sum()
        return self.pairs

    def num_pairs(self):
        return int(self.pairs_device().item())

    def chunks(self, in_row_bytes, out_row_bytes):
        """Batched tensors whose feature tables exceed the 2 GB extent of the buffer-addressed conv instances (64 Cfg-2
        frames x 416 channels = 9 GB): rows are sorted by batch and the frames of a batch share no neighbours
        (data/alivev2.py:358-383), so the layer splits into batch ranges, each with its own plan, input rows rebased to
        the range's first row - the same (offset, channel) chain per output element, i.e. the same bits, on the FAST
        instances.  Returns [(plan, in0, in1, out0, out1)] or None when the whole map fits (or cannot be split: one
        frame alone beyond the extent, which then takes the guarded 64-bit form)."""
        cm = self.cm() if self.cm is not None else None  # weak reference: a plan must not keep its manager (and through it
        if cm is None or self.raw is None:               # every tensor of the frame) alive in a reference cycle
            return None
        V_in = cm.stride_map(self.in_stride).V
        if V_in * in_row_bytes < BUF_LIMIT and self.V_out * out_row_bytes < BUF_LIMIT:
            return None
        bi, bo = cm.batch_bounds(self.in_stride), cm.batch_bounds(self.out_stride)
        B = len(bi) - 1
        f = 1
        while f < B:
            f *= 2
        fits = lambda f: all((bi[min(c + f, B)] - bi[c]) * in_row_bytes < BUF_LIMIT and  # noqa: E731
                             (bo[min(c + f, B)] - bo[c]) * out_row_bytes < BUF_LIMIT for c in range(0, B, f))
        while f >= 1 and not fits(f):
            f //= 2
        if f < 1 or f >= B:
            return None
        if f not in self._chunked:
            nbr, ld, mask = self.raw
            parts = []
            for c in range(0, B, f):
                i0, i1, o0, o1 = bi[c], bi[min(c + f, B)], bo[c], bo[min(c + f, B)]
                if o1 > o0:
                    parts.append((cm._build_plan(nbr[:, o0:], ld, mask[o0:], self.K, o1 - o0, nbr_base=i0), i0, i1, o0, o1))
            self._chunked[f] = parts
        return self._chunked[f]


class SplitPlan:
    """A kernel map run as PASSES over ascending offset ranges, each range with its own plan - its own mask-sorted row
    order.  Rows that share their neighbours among 13-14 offsets group far better into 16-row matrix-op sub-tiles than rows
    that must agree on all 27: useful row slots 0.872 -> 0.960 on the 2 cm room level (0.936 -> 0.969 one level up; CPU
    count, tools/tile_experiment.py).  The passes hand the raw accumulators over through memory (sv_conv_fwd_acc), so every
    output element stays ONE fma chain over (offset ascending, channel ascending).  parts: [(k0, k1, ConvPlan)]."""

    __slots__ = ("parts", "whole")

    def __init__(self, parts, whole):
        self.parts, self.whole = parts, whole

    # what callers read off a plan
    @property
    def V_out(self):
        return self.whole.V_out

    @property
    def Vpad(self):
        return self.whole.Vpad

    @property
    def out_stride(self):
        return self.whole.out_stride

    def pairs_device(self):
        return self.whole.pairs_device()

    def num_pairs(self):
        return self.whole.num_pairs()


class LayerMaps(NamedTuple):
    """The kernel maps of one layer shape (layer_maps).  A map is (name, at, *args): CoordinateManager.plan_<name>(stride,
    *args) with stride = the layer's input ("in") or output ("out") tensor stride; None = dense rows, no plan."""
    forward: Optional[tuple]
    out_stride: tuple  # (mul, div): the output's tensor stride is ts * mul // div
    backward: Optional[tuple]  # conv input gradient / pooling backward; SAME_PLAN = the forward plan itself
    mirror: bool  # the input gradient runs on the offset-mirrored weights W[26 - k]^T (else W[k]^T)


SAME_PLAN = ("forward",)


def layer_maps(kernel_size, stride, dilation=1, transposed=False, pooling=False):
    """THE table from a layer's shape to its kernel maps - which map a convolution (or, pooling=True, a local pooling)
    runs on, its output stride, and the map of its backward pass:

      conv k1 s1                         dense rows         ts        the same        W^T
      conv k3 s1, any dilation           k3                 ts        the same plan   mirrored
      k2 s2 (pooling: dilation 1)        down               ts * 2    up of ts * 2
      conv k2 s2 transposed              up                 ts // 2   down of ts // 2
      k in {1, 3}, integer s >= 2        strided            ts * s    strided_t
      pooling k3 s1 / k1 s1              k3 / strided       ts        strided_t

    Pure: no tensors, no GPU.  Any other shape raises NotImplementedError."""
    ks, st, dil = kernel_size, stride, dilation
    strided = ks in (1, 3) and isinstance(st, int)
    if pooling:
        if ks == 2 and st == 2 and dil == 1:
            return LayerMaps(("down", "in"), (2, 1), ("up", "out"), False)
        if strided and st >= 1:
            fwd = ("k3", "in", dil) if (ks, st) == (3, 1) else ("strided", "in", ks, st, dil)
            return LayerMaps(fwd, (st, 1), ("strided_t", "in", ks, st, dil), False)
        raise NotImplementedError(f"pooling kernel_size={ks} stride={st} dilation={dil}: no kernel map of that shape")
    if transposed:
        if ks == 2 and st == 2:
            return LayerMaps(("up", "in"), (1, 2), ("down", "out"), False)
    elif ks == 1 and st == 1:
        return LayerMaps(None, (1, 1), SAME_PLAN, False)
    elif ks == 3 and st == 1:
        return LayerMaps(("k3", "in", dil), (1, 1), SAME_PLAN, True)
    elif ks == 2 and st == 2:
        return LayerMaps(("down", "in"), (2, 1), ("up", "out"), False)
    elif strided and st >= 2:  # the strided convs of the classification ResNets (model/backbone/resnet.py:53,76,99-105)
        return LayerMaps(("strided", "in", ks, st, dil), (st, 1), ("strided_t", "in", ks, st, dil), False)
    raise NotImplementedError(
        f"kernel_size={ks} stride={st} transposed={transposed}: not used by the reference's U-Nets")


class CoordinateManager:
    def __init__(self, device):
        self.device = device
        self.maps = {}  # stride -> CoordinateMap
        self.parents = {}  # fine stride -> (parent int32[V_fine], child_start int32[V_coarse+1])
        self.general_parents = {}  # (fine stride, coarse stride) -> parent int32[V_fine] of the maps of _stride_map_general
        self.plans = {}
        self._batch_offsets = {}
        self._batch_bounds = {}
        self.num_batches = None
        self.phase_hook = None  # set per frame by app/pipeline.py FramePipeline.run (see model/backbone/minkunet.py)
        self.split_rules = None  # [(min_rows, cuts)] of this frame's wide 3x3x3 layers; None = nn.SPLIT_RULES
        self.split_ready = None  # event: the offset-range plans, built on another stream while the encoder runs, are there
        self._arenas = []  # the frame composites' arenas (every map / plan array built by them is a view of one)

    def _own(self, plan, nbr, ld, mask, in_stride, out_stride):
        plan.cm, plan.raw, plan.in_stride, plan.out_stride = weakref.ref(self), (nbr, ld, mask), in_stride, out_stride
        return plan

    # ---- coordinate maps -------------------------------------------------------------------
    def stride_map(self, stride):
        """Map at tensor stride `stride`; created on demand: a power of two from the next finer one (sv_stride_map, key bits
        cleared), any other stride from the coarsest existing map whose stride divides it (sv_stride_map_general)."""
        if stride in self.maps:
            return self.maps[stride]
        if stride > 1 and (stride & (stride - 1)):
            return self._stride_map_general(stride)
        if stride <= 1:
            raise _lib.SvHipError(f"no coordinate map at tensor stride {stride}")
        fine = self.stride_map(stride // 2)
        child_start = torch.empty(fine.V + 1, dtype=torch.int32, device=self.device)
        m, parent = self._derive_map(fine, stride, "sv_stride_map", ((stride // 2).bit_length() - 1,), (child_start,))
        self.parents[stride // 2] = (parent, child_start[: m.V + 1])
        return m

    def _stride_map_general(self, stride):
        divisors = [s for s in self.maps if stride % s == 0]
        if not divisors:
            raise _lib.SvHipError(f"no coordinate map at tensor stride {stride}: no existing map's stride divides it")
        fine = self.maps[max(divisors)]
        bad = lambda n: _lib.SvHipError(f"{n} voxels leave the key range at tensor stride {stride} "  # noqa: E731
                                        f"(floor(c / {stride}) * {stride} < -2^17)")
        m, parent = self._derive_map(fine, stride, "sv_stride_map_general", (fine.stride, stride), bad=bad)
        self.general_parents[(fine.stride, stride)] = parent
        return m

    def _derive_map(self, fine, stride, fn, ints, more=(), bad=None):
        """The map at `stride` from `fine` by fn = sv_stride_map (ints: level; more: child_start) or sv_stride_map_general
        (ints: s_in, s_out; bad: the error for its count of voxels that leave the key range): workspace and outputs, the
        call, the size read-back, and the map registered.  Returns (map, parent int32[fine.V])."""
        dev, n = self.device, max(fine.V, 1)
        ws_bytes = getattr(_lib.load(), fn + "_workspace_bytes")(c_int64(fine.V))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        coords = torch.empty((n, 4), dtype=torch.int32, device=dev)
        parent = torch.empty(n, dtype=torch.int32, device=dev)
        counters = torch.empty(4, dtype=torch.int32, device=dev)
        call(fn, ptr(fine.keys), c_int64(fine.V), *map(c_int, ints), ptr(ws), c_size_t(ws_bytes),
             *map(ptr, (keys, coords, parent, *more, counters)), stream_ptr())
        V, n_bad = counters.tolist()[:2]
        if bad is not None and n_bad:
            raise bad(n_bad)
        m = self.maps[stride] = CoordinateMap(keys[:V], coords[:V], V, stride)
        return m, parent[:fine.V]

    # ---- plans -----------------------------------------------------------------------------
    def batches(self):
        """number of batch indices (largest + 1; 1 for an empty map): num_batches where the caller set it (app/pipeline.py
        knows its group size), else one read-back from the stride-1 map, cached"""
        if self.num_batches is None:
            m1 = self.stride_map(1)
            self.num_batches = int(m1.coords[:, 0].max().item()) + 1 if m1.V else 1
        return self.num_batches

    def batch_bounds(self, stride):
        """host copy of the first row of every batch at tensor stride `stride` ([B + 1] python ints; one read-back per
        level, cached) - the ranges batched launches are split at (ConvPlan.chunks)"""
        if stride not in self._batch_bounds:
            self._batch_bounds[stride] = self.batch_offsets(stride, self.batches()).tolist()
        return self._batch_bounds[stride]

    def _build_plan(self, nbr, ld, mask, K, V_out, nbr_base=0):
        dev = self.device
        Vpad = _round_up(max(V_out, 1), SV_TILE_ROWS)
        ws_bytes = _lib.load().sv_plan_workspace_bytes(c_int64(V_out))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        perm = torch.empty(Vpad, dtype=torch.int32, device=dev)
        nbr_s = torch.empty((K, Vpad), dtype=torch.int32, device=dev)
        submask = torch.empty((Vpad // SV_TILE_ROWS, K), dtype=torch.int32, device=dev)
        tile_order = torch.empty(Vpad // SV_TILE_ROWS, dtype=torch.int32, device=dev)
        call("sv_plan_build", ptr(nbr), c_int64(ld), ptr(mask), c_int(K), c_int64(V_out), c_int64(nbr_base), ptr(ws),
             c_size_t(ws_bytes),
             ptr(perm), ptr(nbr_s), ptr(submask), ptr(tile_order), c_int64(Vpad), stream_ptr())
        return ConvPlan(perm, nbr_s, submask, tile_order, V_out, Vpad, K)

    def _kmap_plan(self, key, K, V_out, in_stride, out_stride, fill):
        """The plan of a whole kernel map, cached under `key`: fill(nbr int32[K, ld], ld, mask int32[ld]) is the
        sv_kernel_map_* call that writes the table of the V_out output rows (ld = max(V_out, 1))."""
        if key not in self.plans:
            ld = max(V_out, 1)
            nbr = torch.empty((K, ld), dtype=torch.int32, device=self.device)
            mask = torch.empty(ld, dtype=torch.int32, device=self.device)
            fill(nbr, ld, mask)
            self.plans[key] = self._own(self._build_plan(nbr, ld, mask, K, V_out), nbr, ld, mask, in_stride, out_stride)
        return self.plans[key]

    def plan_k3(self, stride, dilation=1):
        m = self.stride_map(stride)

        def fill(nbr, ld, mask):
            tkeys, tvals, cap = m.hash()
            call("sv_kernel_map_k3", ptr(m.coords), c_int64(m.V), c_int(stride), c_int(dilation), ptr(tkeys), ptr(tvals),
                 c_int64(cap), ptr(nbr), c_int64(ld), ptr(mask), stream_ptr())

        return self._kmap_plan(("k3", stride, dilation), 27, m.V, stride, stride, fill)

    def plan_k3_split(self, stride, split=14):
        """The 3x3x3 map of `stride` as passes over ascending offset ranges (SplitPlan): split = 14 -> [0, 14) and [14, 27)
        (the centre offset in the first pass; the best two-pass split on the room levels, 13 equal); a tuple of split
        points gives more passes."""
        cuts = (split,) if isinstance(split, int) else tuple(split)
        key = ("k3split", stride, split)
        if key not in self.plans:
            whole = self.plan_k3(stride)
            nbr, ld, mask = whole.raw
            parts = []
            bounds = (0,) + cuts + (27,)
            for k0, k1 in zip(bounds[:-1], bounds[1:]):
                sub = ((mask >> k0) & ((1 << (k1 - k0)) - 1)).to(torch.int32)
                plan = self._build_plan(nbr[k0:k1], ld, sub, k1 - k0, whole.V_out)
                parts.append((k0, k1, self._own(plan, nbr[k0:k1], ld, sub, stride, stride)))
            self.plans[key] = SplitPlan(parts, whole)
        return self.plans[key]

    def plan_down(self, stride):
        """kernel_size 2, stride 2 convolution from tensor stride `stride` to 2*stride."""
        fine, coarse = self.stride_map(stride), self.stride_map(stride * 2)

        def fill(nbr, ld, mask):
            call("sv_kernel_map_down", ptr(fine.keys), ptr(self.parents[stride][0]), c_int64(fine.V),
                 c_int(stride.bit_length() - 1), c_int64(coarse.V), ptr(nbr), c_int64(ld), ptr(mask), stream_ptr())

        return self._kmap_plan(("down", stride), 8, coarse.V, stride, stride * 2, fill)

    def plan_up(self, stride):
        """transposed kernel_size 2, stride 2 convolution from tensor stride `stride` to stride/2 (existing map)."""
        fs = stride // 2
        if fs not in self.maps or fs not in self.parents:
            raise _lib.SvHipError(
                f"transposed conv to tensor stride {fs}: that coordinate map does not exist "
                "(ME semantics: the output reuses the encoder's map, model/backbone/minkunet.py:152-156)")
        fine = self.maps[fs]

        def fill(nbr, ld, mask):
            call("sv_kernel_map_up", ptr(fine.keys), ptr(self.parents[fs][0]), c_int64(fine.V), c_int(fs.bit_length() - 1),
                 ptr(nbr), c_int64(ld), ptr(mask), stream_ptr())

        return self._kmap_plan(("up", stride), 8, fine.V, stride, fs, fill)

    def _plan_probe(self, name, in_stride, kernel_size, stride, dilation):
        """kernel map between the maps at in_stride and in_stride * stride (sv_kernel_map_probe): the rows of one probe the
        table of the other, at +in_stride * dilation for the layer's own map, minus that for its transpose"""
        if kernel_size not in (1, 3) or stride < 1 or dilation < 1:
            raise _lib.SvHipError(f"plan_{name}: kernel_size {kernel_size} stride {stride} dilation {dilation}")
        t = self.stride_map(in_stride)  # the input map first: the output map is derived from the existing ones
        q, step = self.stride_map(in_stride * stride), in_stride * dilation
        if name == "strided_t":
            q, t, step = t, q, -step

        def fill(nbr, ld, mask):
            tkeys, tvals, cap = t.hash()
            call("sv_kernel_map_probe", ptr(q.coords), c_int64(q.V), c_int(kernel_size), c_int(step), ptr(t.coords),
                 c_int64(t.V), ptr(tkeys), ptr(tvals), c_int64(cap), ptr(nbr), c_int64(ld), ptr(mask), stream_ptr())

        return self._kmap_plan((name, in_stride, kernel_size, stride, dilation), kernel_size ** 3, q.V, t.stride, q.stride, fill)

    def plan_strided(self, in_stride, kernel_size, stride, dilation=1):
        """kernel_size 3 or 1 convolution (or pooling) of stride `stride` from tensor stride in_stride to in_stride * stride:
        the output map's rows probe the input map's table at +in_stride * dilation (the kernel is centred on the output)."""
        return self._plan_probe("strided", in_stride, kernel_size, stride, dilation)

    def plan_strided_t(self, in_stride, kernel_size, stride, dilation=1):
        """the transpose of plan_strided's map (input gradient of the conv, backward of the pooling): the input map's rows
        probe the output map's table at -in_stride * dilation; nbr[k][o] = i there exactly when nbr_t[k][i] = o here."""
        return self._plan_probe("strided_t", in_stride, kernel_size, stride, dilation)

    def layer_plans(self, maps, ts, plan=None):
        """A row of layer_maps applied at tensor stride ts: (forward plan, output stride, thunk of the backward plan,
        mirror).  plan: what the caller runs in place of the row's forward map (the offset-range split of a 3x3x3 layer);
        the backward plan is built when the thunk is called."""
        mul, div = maps.out_stride
        at = {"in": ts, "out": ts * mul // div}
        build = lambda name, where, *args: getattr(self, "plan_" + name)(at[where], *args)  # noqa: E731
        if plan is None and maps.forward is not None:
            plan = build(*maps.forward)
        backward = (lambda: plan) if maps.backward == SAME_PLAN else (lambda: build(*maps.backward))
        return plan, at["out"], backward, maps.mirror

    # ---- frame composites (sv_frame_plans): everything a U-Net asks for in one or two host calls ------------
    def split_cuts_for(self, rows):
        """split points of the wide 3x3x3 layers on a map of `rows` voxels (None = one pass)"""
        if self.split_rules is None:
            from . import nn as svnn

            return svnn.split_points_for(rows)
        for min_rows, cuts in self.split_rules:
            if rows >= min_rows:
                return cuts
        return None

    def build_plans(self, levels, k3=True, down=True, up=True, split=True):
        """Hash tables, kernel maps and conv plans of pyramid levels 0..levels through ONE sv_frame_plans call (what
        plan_k3 / plan_down / plan_up / plan_k3_split build piece by piece; the same arrays).  The maps of every level
        must exist (TensorField.sparse(pyramid_levels=...) or stride_map)."""
        lib = _lib.load()
        L = levels
        ms = [self.stride_map(1 << l) for l in range(L + 1)]
        V = (c_int64 * (L + 1))(*[m.V for m in ms])
        flags = ((_lib.SV_FRAME_K3 if k3 else 0) | (_lib.SV_FRAME_DOWN if down else 0) | (_lib.SV_FRAME_UP if up else 0))
        cuts_of = {}
        cuts_arr = (c_int32 * ((L + 1) * _lib.SV_FRAME_MAX_CUTS))()
        if split:
            for l in range(L + 1):
                cuts = self.split_cuts_for(ms[l].V)
                if cuts is None or ("k3split", 1 << l, cuts) in self.plans:
                    continue
                tup = (cuts,) if isinstance(cuts, int) else tuple(cuts)
                if len(tup) > _lib.SV_FRAME_MAX_CUTS:
                    continue  # more passes than the composite takes: plan_k3_split builds them piecewise on demand
                cuts_of[l] = cuts
                for i, c in enumerate(tup):
                    cuts_arr[l * _lib.SV_FRAME_MAX_CUTS + i] = c
            if cuts_of:
                flags |= _lib.SV_FRAME_SPLIT
        if flags == 0:
            return
        pv = lambda ts: (c_void_p * (L + 1))(*[(t.data_ptr() if t is not None else None) for t in ts])  # noqa: E731
        keys = pv([m.keys for m in ms])
        coords = pv([m.coords for m in ms])
        parent = pv([self.parents[1 << l][0] if (1 << l) in self.parents else None for l in range(L + 1)])
        k3n = k3m = None
        if (flags & _lib.SV_FRAME_SPLIT) and not k3:
            whole = [self.plan_k3(1 << l) if l in cuts_of else None for l in range(L + 1)]
            k3n = pv([w.raw[0] if w is not None else None for w in whole])
            k3m = pv([w.raw[2] if w is not None else None for w in whole])
        nbytes = lib.sv_frame_plans_arena_bytes(V, c_int(L), c_int(flags), cuts_arr)
        arena = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        sbytes = lib.sv_frame_plans_scratch_bytes(V, c_int(L))
        scratch = torch.empty(sbytes, dtype=torch.uint8, device=self.device)
        # every record sv_frame_plans can emit: a hash table, the 27-offset plan and up to SV_FRAME_MAX_CUTS + 1 offset ranges
        # on each of the L + 1 levels, a down and an up plan on all but the top one
        max_rec = (2 + (_lib.SV_FRAME_MAX_CUTS + 1)) * (L + 1) + 2 * L
        layout = (c_int64 * (_lib.SV_FRAME_RECORD * (1 + max_rec)))()
        call("sv_frame_plans", keys, coords, parent, V, c_int(L), c_int(flags), cuts_arr, k3n, k3m, ptr(arena), c_size_t(nbytes),
             ptr(scratch), c_size_t(sbytes), layout, c_int(max_rec), stream_ptr())
        self._arenas.append(arena)
        i32 = lambda off, n: arena[off: off + 4 * n].view(torch.int32)  # noqa: E731
        pending_split = {}
        for r in range(layout[1]):
            rec = layout[_lib.SV_FRAME_RECORD * (1 + r): _lib.SV_FRAME_RECORD * (2 + r)]
            kind, l, k0, k1, o_nbr, o_mask, o_perm, o_nbrs, o_sub, o_tile, V_out, Vpad, K, ld, o_tk, cap = rec
            stride = 1 << l
            if kind == _lib.SV_FRAME_REC_HASH:
                ms[l]._hash = (arena[o_tk: o_tk + 8 * cap].view(torch.int64), i32(o_nbr, cap), cap)
                continue
            plan = ConvPlan(i32(o_perm, Vpad), i32(o_nbrs, K * Vpad).view(K, Vpad), i32(o_sub, (Vpad // SV_TILE_ROWS) * K).view(-1, K),
                            i32(o_tile, Vpad // SV_TILE_ROWS), V_out, Vpad, K)
            mask = i32(o_mask, ld)
            if kind == _lib.SV_FRAME_REC_SPLIT:
                whole = self.plans[("k3", stride, 1)]
                nbr = i32(o_nbr, K * ld).view(K, ld) if o_nbr >= 0 else whole.raw[0][k0:k1]
                pending_split.setdefault(l, []).append((k0, k1, self._own(plan, nbr, ld, mask, stride, stride)))
                continue
            nbr = i32(o_nbr, K * ld).view(K, ld)
            if kind == _lib.SV_FRAME_REC_K3:
                self.plans[("k3", stride, 1)] = self._own(plan, nbr, ld, mask, stride, stride)
            elif kind == _lib.SV_FRAME_REC_DOWN:
                self.plans[("down", stride)] = self._own(plan, nbr, ld, mask, stride, stride * 2)
            elif kind == _lib.SV_FRAME_REC_UP:
                self.plans[("up", stride * 2)] = self._own(plan, nbr, ld, mask, stride * 2, stride)
        for l, parts in pending_split.items():
            self.plans[("k3split", 1 << l, cuts_of[l])] = SplitPlan(parts, self.plans[("k3", 1 << l, 1)])

    def batch_offsets(self, stride, B):
        key = (stride, B)
        if key not in self._batch_offsets:
            m = self.stride_map(stride)
            bs = torch.empty(B + 1, dtype=torch.int32, device=self.device)
            call("sv_batch_offsets", ptr(m.keys), c_int64(m.V), c_int(B), ptr(bs), stream_ptr())
            self._batch_offsets[key] = bs
        return self._batch_offsets[key]


def _as_device(device):
    if device is None:
        device = "cuda"
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.SvHipError(
            f"device {device}: the MI355X-native path runs on the GPU only (no CPU fallback by design)")
    return device


def _voxelize(coords, device, coords_are_int):
    """Run sv_voxelize; returns (CoordinateMap at stride 1, inverse int64[N], order int32[N], seg_start int32[V+1])."""
    N = coords.shape[0]
    lib = _lib.load()
    ws_bytes = lib.sv_voxelize_workspace_bytes(c_int64(N))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    n1 = max(N, 1)
    keys = torch.empty(n1, dtype=torch.int64, device=device)
    vcoords = torch.empty((n1, 4), dtype=torch.int32, device=device)
    inverse = torch.empty(n1, dtype=torch.int64, device=device)
    order = torch.empty(n1, dtype=torch.int32, device=device)
    seg_start = torch.empty(n1 + 1, dtype=torch.int32, device=device)
    counters = torch.empty(4, dtype=torch.int32, device=device)
    call("sv_voxelize", ptr(coords), c_int(1 if coords_are_int else 0), c_int64(N), ptr(ws), c_size_t(ws_bytes),
         ptr(keys), ptr(vcoords), ptr(inverse), ptr(order), ptr(seg_start), ptr(counters), stream_ptr())
    cnt = counters.tolist()
    V, bad = cnt[0], cnt[1]
    if bad:
        raise _lib.SvHipError(
            f"{bad} points have coordinates outside the key range (-2^17 <= voxel < 2^17 per axis, 0 <= batch < 1024)")
    return CoordinateMap(keys[:V], vcoords[:V], V, 1), inverse[:N], order[:N], seg_start[: V + 1]


_tls = threading.local()


def _pinned_counters(n):
    """per-thread pinned int32 buffer the frame composite reads its level sizes back through (the call synchronises on
    its own kernels before it returns, so one buffer per host thread is enough)"""
    buf = getattr(_tls, "counters", None)
    if buf is None or buf.numel() < n:
        buf = torch.empty(max(n, 64), dtype=torch.int32).pin_memory()
        _tls.counters = buf
    return buf


def _voxelize_frame(coords, device, coords_are_int, levels):
    """sv_frame_maps: voxelisation and the `levels` stride-2 maps of a frame in one host call.  Returns (CoordinateManager
    with maps 1 .. 2^levels and their parent tables, inverse, order, seg_start) - the arrays sv_voxelize + sv_stride_map
    produce piece by piece."""
    N = coords.shape[0]
    lib = _lib.load()
    abytes = lib.sv_frame_maps_arena_bytes(c_int64(N), c_int(levels))
    sbytes = lib.sv_frame_maps_scratch_bytes(c_int64(N))
    arena = torch.empty(abytes, dtype=torch.uint8, device=device)
    scratch = torch.empty(sbytes, dtype=torch.uint8, device=device)
    counters = _pinned_counters(4 * (levels + 2))
    layout = (c_int64 * (8 + 6 * (levels + 1)))()
    call("sv_frame_maps", ptr(coords), c_int(1 if coords_are_int else 0), c_int64(N), c_int(levels), ptr(arena), c_size_t(abytes),
         ptr(scratch), c_size_t(sbytes), c_void_p(counters.data_ptr()), layout, stream_ptr())
    cm = CoordinateManager(device)
    cm._arenas.append(arena)
    view = lambda off, nbytes, dt: arena[off: off + nbytes].view(dt)  # noqa: E731
    Vs = [layout[8 + 6 * l] for l in range(levels + 1)]
    for l in range(levels + 1):
        V = Vs[l]
        o_keys, o_coords, o_parent, o_child = layout[9 + 6 * l: 13 + 6 * l]
        cm.maps[1 << l] = CoordinateMap(view(o_keys, 8 * V, torch.int64), view(o_coords, 16 * V, torch.int32).view(V, 4), V, 1 << l)
        if l < levels:
            cm.parents[1 << l] = (view(o_parent, 4 * V, torch.int32), view(o_child, 4 * (Vs[l + 1] + 1), torch.int32))
    V0 = Vs[0]
    return (cm, view(layout[3], 8 * N, torch.int64), view(layout[4], 4 * N, torch.int32), view(layout[5], 4 * (V0 + 1), torch.int32))


def _voxel_reduce(feats, order, seg_start, V, mode):
    C = feats.shape[1]
    out = torch.empty((V, C), dtype=torch.float32, device=feats.device)
    call("sv_voxel_reduce", ptr(feats), c_int(C), ptr(order), ptr(seg_start), c_int64(V), c_int(mode), ptr(out),
         stream_ptr())
    return out


def _reduce_mode(quantization_mode):
    mode = {SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE: _lib.SV_REDUCE_MEAN,
            SparseTensorQuantizationMode.UNWEIGHTED_SUM: _lib.SV_REDUCE_SUM,
            SparseTensorQuantizationMode.RANDOM_SUBSAMPLE: _lib.SV_REDUCE_FIRST}.get(quantization_mode)
    if mode is None:
        raise NotImplementedError(f"quantization_mode {quantization_mode}")
    return mode


def _slice_rows(F, inverse):
    N, C = inverse.shape[0], F.shape[1]
    if F.stride(1) != 1:
        F = F.contiguous()
    out = torch.empty((N, C), dtype=torch.float32, device=F.device)
    call("sv_slice_rows", ptr(F), c_int64(F.stride(0)), c_int(C), ptr(inverse), c_int64(N), ptr(out), stream_ptr())
    return out


class VoxelReduceFunction(torch.autograd.Function):
    """points -> voxels (sv_voxel_reduce, mean or sum) with its backward: the voxel gradient (divided by the voxel's count
    for the mean) sliced back to the points - a gather (sv_slice_rows), the same bits on every run"""

    @staticmethod
    def forward(ctx, feats, inverse, order, seg_start, V, mode):
        ctx.inverse, ctx.seg_start, ctx.mode = inverse, seg_start, mode
        return _voxel_reduce(feats.contiguous(), order, seg_start, V, mode)

    @staticmethod
    def backward(ctx, dy):
        if ctx.mode == _lib.SV_REDUCE_MEAN:
            dy = dy / (ctx.seg_start[1:] - ctx.seg_start[:-1]).to(torch.float32).unsqueeze(1)
        return _slice_rows(dy, ctx.inverse), None, None, None, None, None


class SliceFunction(torch.autograd.Function):
    """voxels -> points (sv_slice_rows); backward: the point gradients summed per voxel in ascending point index
    (sv_voxel_reduce, SV_REDUCE_SUM) - no index_add_, the same bits on every run"""

    @staticmethod
    def forward(ctx, F, inverse, order, seg_start):
        ctx.order, ctx.seg_start, ctx.V = order, seg_start, F.shape[0]
        return _slice_rows(F, inverse)

    @staticmethod
    def backward(ctx, dy):
        return _voxel_reduce(dy.contiguous(), ctx.order, ctx.seg_start, ctx.V, _lib.SV_REDUCE_SUM), None, None, None


def _has_graph(t):
    return t.requires_grad and torch.is_grad_enabled()


class _Voxelisation:
    """what sv_voxelize made of a field's coordinates; ONE object shared by a field and every field derived from it
    with .new(), as ME shares a field's coordinate map through the coordinate manager"""

    __slots__ = ("coordinate_manager", "inverse_mapping", "order", "seg_start", "shared")

    def __init__(self, coordinate_manager=None, inverse_mapping=None):
        self.coordinate_manager, self.inverse_mapping = coordinate_manager, inverse_mapping
        self.order = self.seg_start = None
        self.shared = False


def _vox_attr(name):
    return property(lambda self: getattr(self._vox, name), lambda self, value: setattr(self._vox, name, value))


class TensorField:
    """ME.TensorField: per-point features + continuous (pre-scaled) coordinates [N, 1+3] = (batch, x, y, z)."""

    coordinate_manager = _vox_attr("coordinate_manager")
    inverse_mapping = _vox_attr("inverse_mapping")
    _order = _vox_attr("order")
    _seg_start = _vox_attr("seg_start")

    def __init__(self, features, coordinates=None, quantization_mode=SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE,
                 minkowski_algorithm=MinkowskiAlgorithm.DEFAULT, device=None, coordinate_manager=None,
                 inverse_mapping=None):
        device = _as_device(device if device is not None else (features.device if features.is_cuda else None))
        self.device = device
        self._F = features.to(device=device, dtype=torch.float32).contiguous()
        self.quantization_mode = quantization_mode
        self.minkowski_algorithm = minkowski_algorithm
        self._vox = _Voxelisation(coordinate_manager, inverse_mapping)
        if coordinates is not None:
            if coordinates.shape[0] != features.shape[0] or coordinates.shape[1] != 4:
                raise ValueError("coordinates must be [N, 4] = (batch, x, y, z) with one row per feature row")
            self._C = coordinates.to(device=device, dtype=torch.float32).contiguous()
        else:
            self._C = None

    @property
    def F(self):
        return self._F

    features = F

    @property
    def C(self):
        return self._C

    coordinates = C

    def __len__(self):
        return self._F.shape[0]

    def new(self, features):
        """A field with other features on the same points (what a layer applied to a field returns).  It shares this
        field's voxelisation - made before or after the call, by either field: sparse() on any of them runs sv_voxelize
        at most once, and their tensors live on one CoordinateManager.  A field without coordinates (the result of
        slice) hands on its manager and inverse mapping."""
        if features.shape[0] != self._F.shape[0]:
            raise ValueError("a field's features have one row per point")
        f = TensorField.__new__(TensorField)
        f.device = self.device
        f._F = features.to(device=self.device, dtype=torch.float32).contiguous()  # a graph stays attached
        f.quantization_mode, f.minkowski_algorithm = self.quantization_mode, self.minkowski_algorithm
        f._C = self._C
        f._vox = self._vox
        self._vox.shared = True
        return f

    def voxelisation(self, pyramid_levels=None, reuse=False):
        """(CoordinateManager, inverse, order, seg_start) of this field's points: sv_voxelize on a field of its own (every
        call, as sparse() always did), once for fields that share their voxelisation through new().  reuse: take the
        existing one of a field of its own as well (what goes on with tensors that came from it)."""
        if self._C is None:
            raise ValueError("TensorField has no coordinates")
        vox = self._vox
        if not ((vox.shared or reuse) and vox.order is not None):
            if pyramid_levels is not None and self._C.shape[0] > 0:
                cm, inverse, order, seg_start = _voxelize_frame(self._C, self.device, False, pyramid_levels)
            else:
                cmap, inverse, order, seg_start = _voxelize(self._C, self.device, coords_are_int=False)
                cm = CoordinateManager(self.device)
                cm.maps[1] = cmap
            vox.coordinate_manager, vox.inverse_mapping, vox.order, vox.seg_start = cm, inverse, order, seg_start
        return vox.coordinate_manager, vox.inverse_mapping, vox.order, vox.seg_start

    def sparse(self, pyramid_levels=None):
        """Voxelise: floor the coordinates, unique voxels in canonical order, per-voxel feature mean.
        pyramid_levels = n (this build's extension): the stride-2 maps of the next n pyramid levels are built in the same
        host call (sv_frame_maps) - what a U-Net's strided convolutions would otherwise ask for one by one, each with
        its own size read-back.  A field that shares its voxelisation (new) and finds it made takes it as it is: pyramid_levels
        then builds nothing ahead, and the coarser maps are made on demand (stride_map), with the same rows."""
        if self._C is None:
            raise ValueError("TensorField has no coordinates")
        mode = _reduce_mode(self.quantization_mode)
        cm, inverse, order, seg_start = self.voxelisation(pyramid_levels)
        V = cm.maps[1].V
        if _has_graph(self._F) and mode != _lib.SV_REDUCE_FIRST:  # differentiable: the mean / sum of features with a graph
            feats = VoxelReduceFunction.apply(self._F, inverse, order, seg_start, V, mode)
        else:
            feats = _voxel_reduce(self._F, order, seg_start, V, mode)
        return SparseTensor(feats, coordinate_manager=cm, tensor_stride=1, _internal=True)


class SparseTensor:
    """ME.SparseTensor: features [V, C] on a coordinate map of a CoordinateManager."""

    def __init__(self, features, coordinates=None, tensor_stride=1, coordinate_manager=None, device=None,
                 quantization_mode=SparseTensorQuantizationMode.RANDOM_SUBSAMPLE, requires_grad=False,
                 _internal=False):
        if _internal:
            self._F = features
            self.coordinate_manager = coordinate_manager
            self.tensor_stride = tensor_stride
            self.device = features.device
            self.inverse_mapping = None
            return
        device = _as_device(device if device is not None else (features.device if features.is_cuda else None))
        self.device = device
        if coordinates is None:
            if coordinate_manager is None:
                raise ValueError("either coordinates or a coordinate_manager is required")
            self._F = features.to(device=device, dtype=torch.float32).contiguous()
            if requires_grad and self._F.is_leaf:
                self._F.requires_grad_(True)
            self.coordinate_manager = coordinate_manager
            self.tensor_stride = tensor_stride
            self.inverse_mapping = None
            return
        # ME.SparseTensor(feats, coordinates=int coords [N,4]) — train_segmentation.py:78: already-quantised rows
        coords = coordinates.to(device=device, dtype=torch.int32).contiguous()
        feats = features.to(device=device, dtype=torch.float32).contiguous()
        if coords.shape[0] != feats.shape[0] or coords.shape[1] != 4:
            raise ValueError("coordinates must be [N, 4] = (batch, x, y, z) with one row per feature row")
        cmap, inverse, order, seg_start = _voxelize(coords, device, coords_are_int=True)
        cm = CoordinateManager(device)
        cm.maps[1] = cmap
        mode = {SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE: _lib.SV_REDUCE_MEAN,
                SparseTensorQuantizationMode.UNWEIGHTED_SUM: _lib.SV_REDUCE_SUM}.get(quantization_mode, _lib.SV_REDUCE_FIRST)
        self._F = _voxel_reduce(feats, order, seg_start, cmap.V, mode)
        if requires_grad:  # ME: the voxel features are a leaf of the graph; .F.grad holds dX after backward()
            self._F.requires_grad_(True)
        self.coordinate_manager = cm
        self.tensor_stride = 1
        self.inverse_mapping = inverse

    # ---- ME accessors ----------------------------------------------------------------------
    @property
    def F(self):
        return self._F

    features = F

    @property
    def coordinate_map(self):
        return self.coordinate_manager.stride_map(self.tensor_stride)

    @property
    def C(self):
        return self.coordinate_map.coords

    coordinates = C

    @property
    def shape(self):
        return self._F.shape

    def __len__(self):
        return self._F.shape[0]

    def _decomposed_bounds(self):
        """first row of every batch on this tensor's map ([B + 1] python ints); an empty tensor has no batch at all"""
        return self.coordinate_manager.batch_bounds(self.tensor_stride) if self.coordinate_map.V else [0]

    @property
    def decomposed_coordinates(self):
        m, bs = self.coordinate_map, self._decomposed_bounds()
        return [m.coords[bs[b]: bs[b + 1], 1:] for b in range(len(bs) - 1)]

    @property
    def decomposed_features(self):
        bs = self._decomposed_bounds()
        return [self._F[bs[b]: bs[b + 1]] for b in range(len(bs) - 1)]

    def new(self, features, tensor_stride=None):
        return SparseTensor(features, coordinate_manager=self.coordinate_manager,
                            tensor_stride=self.tensor_stride if tensor_stride is None else tensor_stride,
                            _internal=True)

    def _same_map(self, other):
        if not isinstance(other, SparseTensor):
            return NotImplemented
        if other.coordinate_manager is not self.coordinate_manager or other.tensor_stride != self.tensor_stride:
            raise ValueError("sparse tensor arithmetic needs both operands on the same coordinate map")
        return other

    def __add__(self, other):
        """ME.SparseTensor `+` on a shared coordinate map (the residual add of ME's resnet blocks: `out += residual`)."""
        o = self._same_map(other)
        return o if o is NotImplemented else self.new(self._F + o._F)

    __iadd__ = __add__

    def __sub__(self, other):
        o = self._same_map(other)
        return o if o is NotImplemented else self.new(self._F - o._F)

    def slice(self, field):
        """Voxel -> point broadcast: TensorField whose rows are this tensor's rows at field.inverse_mapping."""
        if self.tensor_stride != 1:
            raise ValueError("slice needs a tensor at tensor stride 1")
        inv = field.inverse_mapping
        if inv is None or field.coordinate_manager is not self.coordinate_manager:
            raise ValueError("the field was not voxelised into this tensor's coordinate manager")
        return TensorField(self._slice_features(field), coordinates=None, device=self._F.device,
                           coordinate_manager=self.coordinate_manager, inverse_mapping=inv)

    def _slice_features(self, field):
        """this tensor's rows at field.inverse_mapping; differentiable when the features carry a graph and the field holds
        its voxelisation's point order (a field without coordinates, the result of slice, does not: a plain gather, as before)"""
        if _has_graph(self._F) and field._order is not None:
            return SliceFunction.apply(self._F, field.inverse_mapping, field._order, field._seg_start)
        return _slice_rows(self._F, field.inverse_mapping)

    def cat_slice(self, field):
        """ME.SparseTensor.cat_slice: a field on `field`'s points whose rows are [this tensor's row of the point's voxel,
        the field's own features] - voxel features first (reference model/backbone/resnet.py:192)."""
        if self.tensor_stride != 1:
            raise ValueError("cat_slice needs a tensor at tensor stride 1")
        if field.inverse_mapping is None or field.coordinate_manager is not self.coordinate_manager:
            raise ValueError("the field was not voxelised into this tensor's coordinate manager")
        return field.new(torch.cat([self._slice_features(field), field.F], dim=1))

    def slice_argmax(self, field, with_conf=True):
        """Fused slice + utils/output.py:67-73: per-point label (first row maximum, a row's first NaN beating any number, as
        torch's max(1)) and sigmoid(max)."""
        inv = field.inverse_mapping
        if inv is None or field.coordinate_manager is not self.coordinate_manager:
            raise ValueError("the field was not voxelised into this tensor's coordinate manager")
        N, C = inv.shape[0], self._F.shape[1]
        label = torch.empty(N, dtype=torch.int64, device=self._F.device)
        conf = torch.empty(N, dtype=torch.float32, device=self._F.device) if with_conf else None
        call("sv_slice_argmax", ptr(self._F), c_int64(self._F.stride(0)), c_int(C), ptr(inv), c_int64(N), ptr(label),
             ptr(conf), stream_ptr())
        return label, conf

    # dense [B, C] results of global pooling are plain tensors in this build; `out[0][3:]` works on them directly


def cat(*tensors):
    """ME.cat: channel concatenation of tensors on the same coordinate map (model/backbone/minkunet.py:156)."""
    if len(tensors) == 1 and isinstance(tensors[0], (list, tuple)):
        tensors = tuple(tensors[0])
    first = tensors[0]
    for t in tensors[1:]:
        if t.coordinate_manager is not first.coordinate_manager or t.tensor_stride != first.tensor_stride:
            raise ValueError("ME.cat needs tensors on the same coordinate map")
    return first.new(torch.cat([t.F for t in tensors], dim=1))
