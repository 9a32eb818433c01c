"""nn.Module layers with MinkowskiEngine's names, parameters and state_dict layout, running on
libsvhip.so.  The path is chosen by each module's own `training` flag: in eval() a conv -> BN -> residual -> activation
chain is ONE fused launch with detached weights (no graph, the bits of the oracle); in train() the conv / linear layers
run as a torch.autograd.Function (SparseConvFunction: forward sv_conv_fwd, backward sv_conv_fwd on mirrored weights for
the input gradient and sv_conv_wgrad for the weight gradient) and BN (batch statistics), residual, activation and cat
follow as differentiable torch ops.

state_dict keys match ME 0.5.4 so utils/utils.py:87-126 checkpoint_restore-style loading works unchanged:
  MinkowskiConvolution(.Transpose): `kernel` [K, Cin, Cout] ([Cin, Cout] when K == 1), `bias` [1, Cout]
  MinkowskiBatchNorm: `bn.weight bn.bias bn.running_mean bn.running_var bn.num_batches_tracked`
  MinkowskiLinear: `linear.weight` [Cout, Cin], `linear.bias` [Cout]
  MinkowskiInstanceNorm: `weight` [1, C], `bias` [1, C] (from memory, unverified against ME)
  MinkowskiSinusoidal: `kernel` [Cin, Cout], `bias` [1, Cout], `coef` [1, Cout] (from memory, unverified)
Batch norm, the activations, MinkowskiLinear and MinkowskiSinusoidal take a TensorField as they take a SparseTensor: the same
kernels on its features, the result a field on the same points (TensorField.new).
Kernel-offset order inside `kernel` is this build's definition (include/sv_hip.h); `KERNEL_OFFSET_PERMUTATION` is the
single hook for adapting a real ME checkpoint if its order turns out to differ.
"""
import math
from ctypes import c_double, c_float, c_int, c_int64, c_size_t

import numpy as np
import torch
import torch.nn as nn

from . import _lib, profiling
from ._lib import SV_ACT_LEAKY_RELU, SV_ACT_NONE, SV_ACT_RELU, call, ptr, stream_ptr
from .sparse import SparseTensor, SplitPlan, TensorField, layer_maps

# Adapting a checkpoint written by a MinkowskiEngine build whose kernel-offset numbering differs from this build's
# (include/sv_hip.h: k = (dx+1) + 3 (dy+1) + 9 (dz+1), x fastest; k = dx + 2 dy + 4 dz for kernel_size 2):
# {kernel_volume: perm} with  this_build_kernel[k] = checkpoint_kernel[perm[k]].  Applied to every `kernel` of that
# volume inside load_state_dict (_ConvBase._load_from_state_dict); None = checkpoints already use this numbering.
KERNEL_OFFSET_PERMUTATION = None

# Wide 3x3x3 layers on big pyramid levels run as PASSES over ascending ranges of the kernel offsets (sparse.SplitPlan), each
# pass with its own row order: worth it where the matrix-op time saved by the better row grouping (~9 % of the slots at 88k
# voxels with two passes, ~12 % with three) exceeds the extra launches' fixed costs and the accumulator hand-over
# (measured inside the frame pipeline: tools/ab_split.sh).  MRCC_SPLIT_RULES = "min_rows:cut[,cut...];..." -
# the first rule whose min_rows the output map reaches applies; "" = never split.
import os as _os  # noqa: E402


def _parse_split_rules(text):
    rules = []
    for part in text.split(";"):
        if part.strip():
            rows, _, cuts = part.partition(":")
            cuts = tuple(int(v) for v in cuts.split(",") if v)
            rules.append((int(rows), cuts[0] if len(cuts) == 1 else cuts))
    return sorted(rules, key=lambda r: -r[0])


SPLIT_RULES = _parse_split_rules(_os.environ.get("MRCC_SPLIT_RULES", "20000:9,18"))
SPLIT_MIN_CHANNELS = int(_os.environ.get("MRCC_SPLIT_MIN_CHANNELS", "128"))


# one frame alone on the GPU (the per-frame InferenceEngine.predict call): level 1's launches are one round of workgroups
# already and LOSE with three passes when nothing else fills their tails (100.7 -> 95.5 TFLOP/s)
SPLIT_RULES_ONE_FRAME = _parse_split_rules(_os.environ.get("MRCC_SPLIT_RULES_ONE_FRAME", "50000:9,18"))


def split_points_for(rows):
    """split points of the 3x3x3 layers on an output map of `rows` voxels (None = one pass)"""
    for min_rows, cuts in SPLIT_RULES:
        if rows >= min_rows:
            return cuts
    return None


# ------------------------------------------------------------------------------------------------------------------
# functional layer: one libsvhip call per op
# ------------------------------------------------------------------------------------------------------------------
def conv_forward(feats, weight3, plan, V_out, scale=None, shift=None, residual=None, act=SV_ACT_NONE, slope=0.01,
                 out=None, weight_bf16=None):
    """out[o] = act(BN(sum_k in[nbr_k(o)] @ W[k]) + residual[o]); plan None = dense rows (kernel_size 1 / Linear).
    weight_bf16: pack_weights_bf16(weight3) - the layer then runs on the bf16 matrix-core path (sv_conv_fwd_bf16)."""
    K, Cin, Cout = weight3.shape
    if feats.shape[1] != Cin:
        raise ValueError(f"input has {feats.shape[1]} channels, kernel expects {Cin}")
    if feats.stride(1) != 1:
        feats = feats.contiguous()
    if out is None:
        out = torch.empty((V_out, Cout), dtype=torch.float32, device=feats.device)
    if isinstance(plan, SplitPlan):
        return _conv_forward_split(feats, weight3, plan, V_out, scale, shift, residual, act, slope, out, weight_bf16)
    return _conv_forward_one(feats, weight3, plan, V_out, scale, shift, residual, act, slope, out, None, wp=weight_bf16)


def pack_weights_bf16(weight3):
    """W float32 [K, Cin, Cout] (CUDA) -> bf16 [K * Cin * Cout] in the fragment order of sv_conv_fwd_bf16
    (sv_pack_weights_bf16: round to nearest even; offsets outermost, so offsets k0.. start at element k0 * Cin * Cout)."""
    K, Cin, Cout = weight3.shape
    w = weight3.detach().float().contiguous()
    wp = torch.empty(K * Cin * Cout, dtype=torch.bfloat16, device=w.device)
    call("sv_pack_weights_bf16", ptr(w), c_int(K), c_int(Cin), c_int(Cout), ptr(wp), stream_ptr())
    return wp


def _conv_forward_split(feats, weight3, plan, V_out, scale, shift, residual, act, slope, out, weight_bf16=None):
    """A layer as passes over ascending offset ranges (sparse.SplitPlan): every pass but the last writes the raw
    accumulators (no epilogue), the next one continues the chains from them (sv_conv_fwd_acc)."""
    K, Cin, Cout = weight3.shape
    timer = profiling.TIMER
    t0 = None
    if timer is not None:
        kname = profiling.conv_kernel_config(Cout, plan.Vpad, Cin, plan.parts[-1][1] - plan.parts[-1][0])
        if timer.want(kname):
            t0 = timer.start()
    if weight_bf16 is None and not weight3.is_contiguous():
        weight3 = weight3.contiguous()  # a pass takes the block W[k0:k1] by pointer
    acc = None
    for i, (k0, k1, sub) in enumerate(plan.parts):  # timed=False: the passes are ONE layer for the per-kernel table
        w = weight3[k0:k1]
        wp = weight_bf16[k0 * Cin * Cout:k1 * Cin * Cout] if weight_bf16 is not None else None
        if i == len(plan.parts) - 1:
            _conv_forward_one(feats, w, sub, V_out, scale, shift, residual, act, slope, out, acc, timed=False, wp=wp)
        else:
            nxt = torch.empty((V_out, Cout), dtype=torch.float32, device=feats.device)
            _conv_forward_one(feats, w, sub, V_out, None, None, None, SV_ACT_NONE, slope, nxt, acc, timed=False, wp=wp)
            acc = nxt
    if t0 is not None:
        timer.stop(t0, _lib.conv_last_instance()[0], K, Cin, Cout, V_out, plan.pairs_device(), level=plan.out_stride,
                   passes=len(plan.parts))
    return out


def _conv_forward_one(feats, weight3, plan, V_out, scale, shift, residual, act, slope, out, acc_init, timed=True, wp=None):
    K, Cin, Cout = weight3.shape
    if plan is None:
        Vpad = (max(V_out, 1) + _lib.SV_TILE_ROWS - 1) // _lib.SV_TILE_ROWS * _lib.SV_TILE_ROWS
    else:
        Vpad = plan.Vpad
    timer = profiling.TIMER if timed else None
    t0 = None
    if timer is not None:
        kname = profiling.conv_kernel_config(Cout, Vpad, Cin, K)
        if timer.want(kname):
            t0 = timer.start()
    res_ld = residual.stride(0) if residual is not None else 0

    log = profiling.INSTANCE_LOG

    acc_ld = acc_init.stride(0) if acc_init is not None else 0

    fn, w_arg = ("sv_conv_fwd_acc", weight3) if wp is None else ("sv_conv_fwd_bf16", wp)

    def launch(f, pl, o, r, v_out, v_pad, a=None):
        call(fn, ptr(f), c_int64(f.shape[0]), c_int64(f.stride(0)), c_int(Cin), ptr(w_arg), c_int(K),
             c_int(Cout), ptr(pl.perm if pl else None), ptr(pl.nbr_s if pl else None), ptr(pl.submask if pl else None),
             ptr(pl.tile_order if pl else None), c_int64(v_out), c_int64(v_pad), ptr(a), c_int64(acc_ld), ptr(scale), ptr(shift),
             ptr(r), c_int64(res_ld), c_int(act), c_float(slope), ptr(o), c_int64(o.stride(0)), stream_ptr())
        if log is not None:  # what the library really launched (sv_conv_last_instance), not a re-derivation
            log.append((*_lib.conv_last_instance(), K, Cin, Cout, v_out))

    # batched tensors beyond the 2 GB extent of the buffer-addressed instances run as batch ranges (ConvPlan.chunks)
    parts = plan.chunks(4 * feats.stride(0), 4 * max(out.stride(0), res_ld, acc_ld)) if plan is not None else None
    if parts is None:
        launch(feats, plan, out, residual, V_out, Vpad, acc_init)
    else:
        for sub, i0, i1, o0, o1 in parts:
            launch(feats[i0:i1], sub, out[o0:o1], residual[o0:o1] if residual is not None else None, o1 - o0, sub.Vpad,
                   acc_init[o0:o1] if acc_init is not None else None)
    if t0 is not None:
        # recorded under the instance the library reports (the prediction above only decides whether to time at all)
        timer.stop(t0, _lib.conv_last_instance()[0], K, Cin, Cout, V_out,
                   plan.pairs_device() if plan is not None else None,
                   level=plan.out_stride if plan is not None else None)
    return out


# ------------------------------------------------------------------------------------------------------------------
# backward: weight gradient (sv_conv_wgrad) and the autograd Function of a conv / linear layer
# ------------------------------------------------------------------------------------------------------------------
def _wgrad_one(feats, dy, plan, K, Cin, Cout, V_out, dW, accumulate, bf16=False):
    """one sv_conv_wgrad (bf16: sv_conv_wgrad_bf16, or sv_conv_wgrad where it returns SV_ERR_UNSUPPORTED) launch;
    returns the entry point that ran"""
    Vpad = (plan.Vpad if plan is not None
            else (max(V_out, 1) + _lib.SV_TILE_ROWS - 1) // _lib.SV_TILE_ROWS * _lib.SV_TILE_ROWS)
    lib = _lib.load()
    fn = "sv_conv_wgrad_bf16" if bf16 else "sv_conv_wgrad"
    nbytes = getattr(lib, fn + "_workspace_bytes")(c_int64(Vpad), c_int(K), c_int(Cin), c_int(Cout))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dy.device)
    rc = getattr(lib, fn)(ptr(feats), c_int64(feats.shape[0]), c_int64(feats.stride(0)), c_int(Cin), ptr(dy),
                          c_int64(V_out), c_int64(dy.stride(0)), c_int(Cout), c_int(K), ptr(plan.perm if plan else None),
                          ptr(plan.nbr_s if plan else None), ptr(plan.submask if plan else None), c_int64(Vpad),
                          c_int(1 if accumulate else 0), ptr(ws), c_size_t(nbytes), ptr(dW), stream_ptr())
    if bf16 and rc == _lib.SV_ERR_UNSUPPORTED:  # channel counts / row alignment the bf16 kernel does not cover
        return _wgrad_one(feats, dy, plan, K, Cin, Cout, V_out, dW, accumulate)
    _lib._check(rc, fn)
    return fn


def conv_wgrad(feats, dy, plan, K, Cin, Cout, bf16=False, used=None):
    """dW[k][c][n] = sum over the plan's (in i, out o) pairs at offset k of feats[i][c] * dy[o][n] (sv_conv_wgrad), the
    forward's plan: a SplitPlan writes each offset range's block, batch ranges (ConvPlan.chunks) accumulate.
    bf16: operands rounded to bf16, products summed in fp32 (sv_conv_wgrad_bf16; sv_conv_wgrad where it does not cover
    the shape).  used: a set that receives the entry points that ran."""
    if feats.stride(1) != 1:
        feats = feats.contiguous()
    if dy.stride(1) != 1:
        dy = dy.contiguous()
    V_out = dy.shape[0]
    dW = torch.empty((K, Cin, Cout), dtype=torch.float32, device=dy.device)
    used = set() if used is None else used
    if isinstance(plan, SplitPlan):
        for k0, k1, sub in plan.parts:
            _wgrad_plan(feats, dy, sub, k1 - k0, Cin, Cout, V_out, dW[k0:k1], bf16, used)
    else:
        _wgrad_plan(feats, dy, plan, K, Cin, Cout, V_out, dW, bf16, used)
    return dW


def _wgrad_plan(feats, dy, plan, K, Cin, Cout, V_out, dW, bf16=False, used=None):
    used = set() if used is None else used
    parts = plan.chunks(4 * feats.stride(0), 4 * dy.stride(0)) if plan is not None else None
    if parts is None:
        used.add(_wgrad_one(feats, dy, plan, K, Cin, Cout, V_out, dW, False, bf16))
        return
    for j, (sub, i0, i1, o0, o1) in enumerate(parts):  # batch ranges: partial sums of the same offsets
        used.add(_wgrad_one(feats[i0:i1], dy[o0:o1], sub, K, Cin, Cout, o1 - o0, dW, j > 0, bf16))


def _bf16_fwd_ok(rows, Cin, Cout, K):
    """what sv_conv_fwd_bf16 covers: bf16_eligible's channel rule, input rows 16-byte aligned"""
    return (Cin % 32 == 0 and Cin >= 64 and Cout % 16 == 0 and Cout >= 64 and K <= 27
            and rows.data_ptr() % 16 == 0 and rows.stride(0) % 4 == 0)


def _train_log(layer, op, fn):
    log = profiling.TRAIN_LOG
    if log is not None:
        log.append((layer, op, fn))


class SparseConvFunction(torch.autograd.Function):
    """out = conv(feats, W) + bias on `plan` (sv_conv_fwd, no epilogue).  Backward, fp32:
      dX = sv_conv_fwd(dY, W', grad_plan)   W'[k] = W[26 - k]^T on the 3x3x3 plan itself (offset 26 - k is the negation of
               offset k), W[k]^T on the up plan of a down conv / the down plan of a transposed conv / dense rows;
      dW = sv_conv_wgrad(feats, dY, plan);   d bias = column sum of dY.
    grad_plan: a callable giving the input-gradient plan (built only when the input needs a gradient).
    layer: the conv / linear module (None: a plain nn.Linear; a module without training precisions, such as the
    PointNet++ nn.Conv1d / nn.Conv2d, trains fp32 and only names the layer in TRAIN_LOG).  When its training_precision is
    "bf16" the forward runs on
    sv_conv_fwd_bf16 (bias as the fp32 shift), dX on sv_conv_fwd_bf16 with W' packed (where the swapped shape Cin' = Cout,
    Cout' = Cin is one sv_conv_fwd_bf16 covers) and dW on sv_conv_wgrad_bf16 (sv_conv_wgrad where it returns
    SV_ERR_UNSUPPORTED); activations and gradients stay fp32 in memory, d bias stays the fp32 column sum."""

    @staticmethod
    def forward(ctx, feats, weight3, bias, plan, V_out, grad_plan, mirror, layer=None):
        w = weight3.detach()
        if not w.is_contiguous():
            w = w.contiguous()
        bf16 = layer is not None and hasattr(layer, "_train_bf16") and layer._train_bf16()
        shift = bias.detach().reshape(-1) if bias is not None else None
        wp = layer.packed_weights_bf16() if bf16 and _bf16_fwd_ok(feats, w.shape[1], w.shape[2], w.shape[0]) else None
        out = conv_forward(feats.detach(), w, plan, V_out, None, shift, weight_bf16=wp)
        _train_log(layer, "fwd", "sv_conv_fwd_acc" if wp is None else "sv_conv_fwd_bf16")
        ctx.save_for_backward(feats, w)
        ctx.plan, ctx.grad_plan, ctx.mirror, ctx.layer, ctx.bf16 = plan, grad_plan, mirror, layer, bf16
        ctx.bias_shape = bias.shape if bias is not None else None
        return out

    @staticmethod
    def backward(ctx, dy):
        feats, w = ctx.saved_tensors
        K, Cin, Cout = w.shape
        if dy.stride(1) != 1:
            dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            # bf16 only where sv_conv_fwd_bf16 gets a column block of >= 128 channels (Cin % 128 or % 192 == 0): the
            # 416 / 448-wide decoder inputs split into 32 / 64-wide blocks that gather dY 13 / 7 times
            if ctx.bf16 and _bf16_fwd_ok(dy, Cout, Cin, K) and (Cin % 128 == 0 or Cin % 192 == 0):
                dx = conv_forward(dy, w.transpose(1, 2), ctx.grad_plan(), feats.shape[0],
                                  weight_bf16=ctx.layer.packed_grad_weights_bf16(ctx.mirror))
                _train_log(ctx.layer, "dx", "sv_conv_fwd_bf16")
            else:
                wt = (w.flip(0) if ctx.mirror else w).transpose(1, 2).contiguous()
                dx = conv_forward(dy, wt, ctx.grad_plan(), feats.shape[0])
                _train_log(ctx.layer, "dx", "sv_conv_fwd_acc")
        if ctx.needs_input_grad[1]:
            used = set()
            dw = conv_wgrad(feats.detach(), dy, ctx.plan, K, Cin, Cout, bf16=ctx.bf16, used=used)
            _train_log(ctx.layer, "dw", "+".join(sorted(used)))
        if ctx.bias_shape is not None and ctx.needs_input_grad[2]:
            db = dy.sum(0).reshape(ctx.bias_shape)
        return dx, dw, db, None, None, None, None, None


def sparse_conv(feats, weight3, bias, plan, V_out, grad_plan, mirror=False, layer=None):
    """differentiable sparse conv / linear layer (SparseConvFunction); weight3 [K, Cin, Cout] may be a view of the
    parameter (Linear: weight^T), its gradient flows back through the view.  layer: the module whose training_precision
    selects the kernels (None = fp32)"""
    return SparseConvFunction.apply(feats, weight3, bias, plan, V_out, grad_plan, mirror, layer)


def _act_torch(x, act, slope):
    if act == SV_ACT_RELU:
        return torch.relu(x)
    if act == SV_ACT_LEAKY_RELU:
        return torch.nn.functional.leaky_relu(x, slope)
    return x


def linear_train(linear, x, act=SV_ACT_NONE, slope=0.01, layer=None):
    """nn.Linear(x) (+ activation) on the autograd dense path: the weight gradient in sv_conv_wgrad, the input gradient
    in sv_conv_fwd - no torch GEMM.  layer: the MinkowskiLinear that owns `linear` (its training_precision applies);
    None for a plain nn.Linear, which trains fp32"""
    if x.stride(1) != 1:
        x = x.contiguous()
    out = sparse_conv(x, linear.weight.t().unsqueeze(0), linear.bias, None, x.shape[0], lambda: None, layer=layer)
    return _act_torch(out, act, slope)


def affine_act(feats, scale=None, shift=None, residual=None, act=SV_ACT_NONE, slope=0.01):
    V, C = feats.shape
    if feats.stride(1) != 1:
        feats = feats.contiguous()
    out = torch.empty((V, C), dtype=torch.float32, device=feats.device)
    call("sv_affine_act", ptr(feats), c_int64(feats.stride(0)), c_int(C), c_int64(V), ptr(scale), ptr(shift),
         ptr(residual), c_int64(residual.stride(0) if residual is not None else 0), c_int(act), c_float(slope),
         ptr(out), c_int64(C), stream_ptr())
    return out


def global_pool(x, mode):
    cm = x.coordinate_manager
    B = cm.batches()
    bs = cm.batch_offsets(x.tensor_stride, B)
    F = x.F
    C = F.shape[1]
    out = torch.empty((B, C), dtype=torch.float32, device=F.device)
    call("sv_global_pool", ptr(F), c_int64(F.stride(0)), c_int(C), ptr(bs), c_int(B), c_int(mode), ptr(out),
         stream_ptr())
    return out


def global_pool_train(x, mode):
    """global_pool as differentiable torch segment reductions over the batch ranges (training): amax (NaN propagates, a
    tie shares the gradient) / mean; an empty batch gives 0 as the kernel does"""
    bounds = x.coordinate_manager.batch_bounds(x.tensor_stride)
    F = x.F
    rows = []
    for b in range(len(bounds) - 1):
        seg = F[bounds[b]:bounds[b + 1]]
        if seg.shape[0] == 0:
            rows.append(F.new_zeros(F.shape[1]))
        else:
            rows.append(seg.amax(0) if mode == _lib.SV_POOL_MAX else seg.mean(0))
    return torch.stack(rows)


def fold_bn(bn):
    """BatchNorm1d(eval) as y = fmaf(x, scale, shift): scale = w / sqrt(var + eps), shift = b - mean * scale.
    Host-side, once per model, in numpy float32 (correctly rounded IEEE sqrt / divide; torch's vectorised CPU path
    is 1 ulp off), i.e. exactly the arithmetic oracle/sv_oracle.py:fold_bn defines."""
    n = bn.num_features
    w = bn.weight.detach().float().cpu().numpy() if bn.weight is not None else np.ones(n, np.float32)
    b = bn.bias.detach().float().cpu().numpy() if bn.bias is not None else np.zeros(n, np.float32)
    mean = bn.running_mean.detach().float().cpu().numpy()
    var = bn.running_var.detach().float().cpu().numpy()
    scale = (w / np.sqrt(var + np.float32(bn.eps))).astype(np.float32)
    shift = (b - mean * scale).astype(np.float32)
    dev = bn.running_mean.device
    return torch.from_numpy(scale).to(dev), torch.from_numpy(shift).to(dev)


def _tensor_versions(*ts):
    return tuple((t.data_ptr(), t._version) for t in ts if t is not None)


# ------------------------------------------------------------------------------------------------------------------
# compute precision of the conv / linear layers
# ------------------------------------------------------------------------------------------------------------------
PRECISIONS = ("fp32", "bf16")


def _layer_channels(m):
    if isinstance(m, MinkowskiLinear):
        return m.linear.in_features, m.linear.out_features, 1
    return m.in_channels, m.out_channels, m.kernel_volume


def bf16_eligible(m):
    """What sv_conv_fwd_bf16 covers: Cin % 32 == 0, Cin >= 64, Cout % 16 == 0, Cout >= 64, kernel volume <= 27."""
    cin, cout, kv = _layer_channels(m)
    return cin % 32 == 0 and cin >= 64 and cout % 16 == 0 and cout >= 64 and kv <= 27


def _mark_precision(module, precision, attr, what):
    if precision not in PRECISIONS:
        raise ValueError(f"{what} precision must be one of {PRECISIONS}, got {precision!r}")
    marked = []
    for name, m in module.named_modules():
        if isinstance(m, (_ConvBase, MinkowskiLinear)):
            p = precision if precision == "fp32" or bf16_eligible(m) else "fp32"
            setattr(m, attr, p)
            if p == precision:
                marked.append(name)
    return marked


def set_training_precision(module, precision):
    """set_compute_precision's twin for train(): "bf16" marks exactly the layers bf16_eligible() accepts for the bf16
    training path (forward and input gradient on sv_conv_fwd_bf16, weight gradient on sv_conv_wgrad_bf16; activations,
    gradients, BN, residual adds, activations, cat and pooling stay fp32), "fp32" marks every layer fp32 (the default).
    Returns the qualified names of the layers that now train at `precision`.  Independent of set_compute_precision (which
    affects eval() alone); parameters and state_dict are untouched."""
    return _mark_precision(module, precision, "training_precision", "training")


def set_compute_precision(module, precision):
    """Mark the conv / linear layers of `module` (itself included) for `precision`: "bf16" marks exactly the layers
    bf16_eligible() accepts (the rest stay fp32), "fp32" marks every layer fp32 (the default).  Returns the qualified
    names of the layers that now run at `precision`.  Parameters and state_dict are untouched."""
    return _mark_precision(module, precision, "compute_precision", "compute")


class _Bf16Weights:
    """Per-module cache of the packed bf16 weights (plain attributes, not buffers: state_dict does not change),
    re-packed when the weight tensor changes (the _tensor_versions pattern)."""

    def _packed_bf16(self, weight, weight3):
        ver = _tensor_versions(weight)
        if self.__dict__.get("_wp") is None or self.__dict__.get("_wp_ver") != ver:
            self._wp = pack_weights_bf16(weight3)
            self._wp_ver = ver
        return self._wp

    def _weight_bf16(self):
        """packed weights when this layer runs in bf16, else None"""
        if self.compute_precision == "fp32":
            return None
        if self.compute_precision != "bf16":
            raise ValueError(f"compute precision must be one of {PRECISIONS}, got {self.compute_precision!r}")
        return self.packed_weights_bf16()

    def _train_bf16(self):
        """whether this layer trains on the bf16 kernels (set_training_precision)"""
        p = self.__dict__.get("training_precision", "fp32")
        if p not in PRECISIONS:
            raise ValueError(f"training precision must be one of {PRECISIONS}, got {p!r}")
        return p == "bf16" and bf16_eligible(self)

    def packed_grad_weights_bf16(self, mirror):
        """W' of the input gradient, (W flipped over the offsets if mirror)^T packed for sv_conv_fwd_bf16, cached and
        re-packed when the weight changes (an optimizer steps it in place)"""
        weight = self.kernel if isinstance(self, _ConvBase) else self.linear.weight
        ver = (_tensor_versions(weight), mirror)
        if self.__dict__.get("_wpt") is None or self.__dict__.get("_wpt_ver") != ver:
            w = self.weight3().detach()
            self._wpt = pack_weights_bf16((w.flip(0) if mirror else w).transpose(1, 2).contiguous())
            self._wpt_ver = ver
        return self._wpt


# ------------------------------------------------------------------------------------------------------------------
# modules
# ------------------------------------------------------------------------------------------------------------------
class _ConvBase(_Bf16Weights, nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=-1, stride=1, dilation=1, bias=False, dimension=3,
                 transposed=False):
        super().__init__()
        if dimension != 3:
            raise NotImplementedError("only dimension=3 (the reference passes D=3 everywhere)")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.dilation = kernel_size, stride, dilation
        self.dimension = dimension
        self.transposed = transposed
        self.kernel_volume = kernel_size ** dimension
        if self.kernel_volume > 1:
            self.kernel = nn.Parameter(torch.empty(self.kernel_volume, in_channels, out_channels))
        else:
            self.kernel = nn.Parameter(torch.empty(in_channels, out_channels))
        self.bias = nn.Parameter(torch.empty(1, out_channels)) if bias else None
        self.compute_precision = "fp32"  # "bf16": sv_conv_fwd_bf16 (set_compute_precision)
        self.training_precision = "fp32"  # "bf16": the bf16 kernels in train() (set_training_precision)
        self.reset_parameters()

    def reset_parameters(self):
        # ME: uniform(-stdv, stdv), stdv = 1/sqrt(in_channels * kernel_volume) (out_channels for transposed)
        with torch.no_grad():
            n = (self.out_channels if self.transposed else self.in_channels) * self.kernel_volume
            stdv = 1.0 / math.sqrt(n)
            self.kernel.uniform_(-stdv, stdv)
            if self.bias is not None:
                self.bias.uniform_(-stdv, stdv)

    def weight3(self):
        w = self.kernel
        return w if w.dim() == 3 else w.unsqueeze(0)

    def packed_weights_bf16(self):
        return self._packed_bf16(self.kernel, self.weight3())

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        key = prefix + "kernel"
        perm_table = KERNEL_OFFSET_PERMUTATION
        if perm_table is not None and key in state_dict and state_dict[key].dim() == 3:
            perm = perm_table.get(state_dict[key].shape[0]) if isinstance(perm_table, dict) else perm_table
            if perm is not None and len(perm) == state_dict[key].shape[0]:
                if sorted(perm) != list(range(len(perm))):
                    raise ValueError(f"KERNEL_OFFSET_PERMUTATION for kernel volume {len(perm)} is not a permutation")
                state_dict[key] = state_dict[key][torch.as_tensor(list(perm), device=state_dict[key].device)]
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)

    def _maps(self, x, plan=None):
        """(plan, output stride, thunk of the input-gradient plan, mirror) of this layer on x's map (sparse.layer_maps).
        plan None: the forward plan is chosen here - a wide 3x3x3 layer on a big map runs as offset-range passes."""
        cm, ts = x.coordinate_manager, x.tensor_stride
        maps = layer_maps(self.kernel_size, self.stride, self.dilation, self.transposed)
        if (plan is None and maps.forward == ("k3", "in", 1) and self.in_channels >= SPLIT_MIN_CHANNELS
                and self.out_channels >= SPLIT_MIN_CHANNELS):
            cuts = cm.split_cuts_for(cm.stride_map(ts).V)  # the frame's own rules, else SPLIT_RULES
            if cuts is not None:
                if cm.split_ready is not None:
                    # the offset-range plans were built on the prep stream while this stream ran the encoder
                    torch.cuda.current_stream().wait_event(cm.split_ready)
                    cm.split_ready = None
                plan = cm.plan_k3_split(ts, cuts)
        return cm.layer_plans(maps, ts, plan)

    def _plan(self, x):
        return self._maps(x)[:2]

    def _grad_plan(self, x, plan):
        """plan of the input gradient (a forward conv from the output map back to the input map) of a layer whose forward
        ran on `plan`, as a thunk"""
        return self._maps(x, plan)[2]

    def forward_train(self, x, bn=None, residual=None, act=SV_ACT_NONE, slope=0.01, cat_with=None):
        """forward_fused's graph as differentiable ops: the autograd conv, then BN (batch statistics in train(),
        running statistics in eval()), + residual, activation, ME.cat"""
        plan, out_stride, grad_plan, mirror = self._maps(x)
        V_out = x.coordinate_manager.stride_map(out_stride).V
        out = sparse_conv(x.F, self.weight3(), self.bias, plan, V_out, grad_plan, mirror, layer=self)
        if bn is not None:
            out = bn.bn(out)
        if residual is not None:
            out = out + (residual.F if isinstance(residual, SparseTensor) else residual)
        out = _act_torch(out, act, slope)
        if cat_with is not None:
            if cat_with.coordinate_manager is not x.coordinate_manager or cat_with.tensor_stride != out_stride:
                raise ValueError("ME.cat needs tensors on the same coordinate map")
            out = torch.cat([out, cat_with.F], dim=1)
        return x.new(out, tensor_stride=out_stride)

    def forward_fused(self, x, bn=None, residual=None, act=SV_ACT_NONE, slope=0.01, cat_with=None):
        """conv (+ folded BN / bias) (+ residual) (+ activation) in one launch.  cat_with: a SparseTensor on the
        output's coordinate map - the result is ME.cat(conv(x), cat_with) (model/backbone/minkunet.py:152-156), with
        the conv writing straight into the left columns of the concatenated buffer instead of being copied there.
        In train() (this module's or its BN's) the same graph runs as differentiable ops (forward_train)."""
        if self.training or (bn is not None and bn.training):
            return self.forward_train(x, bn, residual, act, slope, cat_with)
        plan, out_stride = self._plan(x)
        V_out = x.coordinate_manager.stride_map(out_stride).V
        scale = shift = None
        if bn is not None:
            scale, shift = bn.folded()
            if self.bias is not None:
                raise NotImplementedError("conv bias followed by a fused BatchNorm")
        elif self.bias is not None:
            shift = self.bias.detach().reshape(-1)
        res = residual.F if isinstance(residual, SparseTensor) else residual
        wp = self._weight_bf16()
        bf16 = {} if wp is None else {"weight_bf16": wp}  # fp32 layers: the call conv_forward always got
        if cat_with is None:
            out = conv_forward(x.F, self.weight3().detach(), plan, V_out, scale, shift, res, act, slope, **bf16)
            return x.new(out, tensor_stride=out_stride)
        if cat_with.coordinate_manager is not x.coordinate_manager or cat_with.tensor_stride != out_stride:
            raise ValueError("ME.cat needs tensors on the same coordinate map")
        skip = cat_with.F
        C = self.out_channels
        buf = torch.empty((V_out, C + skip.shape[1]), dtype=torch.float32, device=x.F.device)
        conv_forward(x.F, self.weight3().detach(), plan, V_out, scale, shift, res, act, slope, out=buf[:, :C], **bf16)
        buf[:, C:].copy_(skip)
        return x.new(buf, tensor_stride=out_stride)

    def forward(self, x):
        return self.forward_fused(x)

    def extra_repr(self):
        return (f"in={self.in_channels}, out={self.out_channels}, kernel_size={self.kernel_size}, "
                f"stride={self.stride}, dilation={self.dilation}")


class MinkowskiConvolution(_ConvBase):
    def __init__(self, in_channels, out_channels, kernel_size=-1, stride=1, dilation=1, bias=False,
                 kernel_generator=None, expand_coordinates=False, convolution_mode=None, dimension=None):
        if dimension is None:
            raise ValueError("dimension is required")
        super().__init__(in_channels, out_channels, kernel_size, stride, dilation, bias, dimension, transposed=False)


class MinkowskiConvolutionTranspose(_ConvBase):
    def __init__(self, in_channels, out_channels, kernel_size=-1, stride=1, dilation=1, bias=False,
                 kernel_generator=None, expand_coordinates=False, convolution_mode=None, dimension=None):
        if dimension is None:
            raise ValueError("dimension is required")
        if expand_coordinates:
            raise NotImplementedError("expand_coordinates=True (generative transposed conv) is not on the hot path")
        super().__init__(in_channels, out_channels, kernel_size, stride, dilation, bias, dimension, transposed=True)


_TENSORS = (SparseTensor, TensorField)  # what a pointwise layer maps to the same kind of tensor (x.F -> x.new)


class MinkowskiBatchNorm(nn.Module):
    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
        super().__init__()
        self.bn = nn.BatchNorm1d(num_features, eps=eps, momentum=momentum, affine=affine,
                                 track_running_stats=track_running_stats)
        self._folded = None
        self._folded_ver = None

    def folded(self):
        if self.training:
            raise _lib.SvHipError("MinkowskiBatchNorm: training-mode statistics are out of scope (inference build); "
                                  "call model.eval()")
        ver = _tensor_versions(self.bn.weight, self.bn.bias, self.bn.running_mean, self.bn.running_var)
        if self._folded is None or self._folded_ver != ver:
            self._folded = fold_bn(self.bn)
            self._folded_ver = ver
        return self._folded

    def forward(self, x):
        # ME's BN: nn.BatchNorm1d on the features - batch statistics and running-stat update in train(); frozen (eval)
        # statistics on features that carry a graph stay differentiable (F.batch_norm with the running statistics)
        if self.training or (x.F.requires_grad and torch.is_grad_enabled()):
            return x.new(self.bn(x.F))
        scale, shift = self.folded()
        return x.new(affine_act(x.F, scale, shift))


class MinkowskiReLU(nn.Module):
    def __init__(self, inplace=False):
        super().__init__()

    def forward(self, x):
        if self.training:
            return x.new(torch.relu(x.F)) if isinstance(x, _TENSORS) else torch.relu(x)
        if isinstance(x, _TENSORS):
            return x.new(affine_act(x.F, act=SV_ACT_RELU))
        return affine_act(x, act=SV_ACT_RELU)


class MinkowskiLeakyReLU(nn.Module):
    def __init__(self, negative_slope=0.01, inplace=False):
        super().__init__()
        self.negative_slope = negative_slope

    def forward(self, x):
        if self.training:
            f = torch.nn.functional.leaky_relu
            return (x.new(f(x.F, self.negative_slope)) if isinstance(x, _TENSORS) else f(x, self.negative_slope))
        if isinstance(x, _TENSORS):
            return x.new(affine_act(x.F, act=SV_ACT_LEAKY_RELU, slope=self.negative_slope))
        return affine_act(x, act=SV_ACT_LEAKY_RELU, slope=self.negative_slope)


class MinkowskiSigmoid(nn.Module):
    # constructed by the heads (model/robotnet_segmentation.py:52) but never called in forward
    def forward(self, x):
        return x.new(torch.sigmoid(x.F))


class MinkowskiLinear(_Bf16Weights, nn.Module):
    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.linear = nn.Linear(in_features, out_features, bias=bias)
        self._wt = None
        self._wt_ver = None
        self.compute_precision = "fp32"  # "bf16": sv_conv_fwd_bf16 (set_compute_precision)
        self.training_precision = "fp32"  # "bf16": the bf16 kernels in train() (set_training_precision)

    def weight3(self):
        """[1, Cin, Cout] view of linear.weight^T, cached (the kernel wants W[k][c][n])."""
        ver = _tensor_versions(self.linear.weight)
        if self._wt is None or self._wt_ver != ver:
            self._wt = self.linear.weight.detach().t().contiguous().unsqueeze(0)
            self._wt_ver = ver
        return self._wt

    def packed_weights_bf16(self):
        return self._packed_bf16(self.linear.weight, self.weight3())

    def forward_fused(self, x, act=SV_ACT_NONE, slope=0.01):
        F = x.F if isinstance(x, _TENSORS) else x
        if self.training:
            out = linear_train(self.linear, F, act, slope, layer=self)
            return x.new(out) if isinstance(x, _TENSORS) else out
        shift = self.linear.bias.detach() if self.linear.bias is not None else None
        wp = self._weight_bf16()
        bf16 = {} if wp is None else {"weight_bf16": wp}  # fp32 layers: the call conv_forward always got
        out = conv_forward(F, self.weight3(), None, F.shape[0], None, shift, None, act, slope, **bf16)
        return x.new(out) if isinstance(x, _TENSORS) else out

    def forward(self, x):
        return self.forward_fused(x)


def sinusoidal(feats, kernel, bias, coef):
    """coef * sin(feats @ kernel + bias) (sv_sinusoidal): fp32 fma chain over the input channels, the sine in float64"""
    N, Cin = feats.shape
    Cout = kernel.shape[1]
    if feats.stride(1) != 1:
        feats = feats.contiguous()
    out = torch.empty((N, Cout), dtype=torch.float32, device=feats.device)
    call("sv_sinusoidal", ptr(feats), c_int64(feats.stride(0) if N else Cin), c_int(Cin), c_int64(N), ptr(kernel), ptr(bias),
         ptr(coef), c_int(Cout), ptr(out), c_int64(Cout), stream_ptr())
    return out


class MinkowskiSinusoidal(nn.Module):
    """ME.MinkowskiSinusoidal: coef * sin(F @ kernel + bias) on a SparseTensor or a TensorField (restated from memory)."""

    def __init__(self, in_channel, out_channel):
        super().__init__()
        self.in_channel, self.out_channel = in_channel, out_channel
        self.kernel = nn.Parameter(torch.randn(in_channel, out_channel))
        self.bias = nn.Parameter(torch.randn(1, out_channel))
        self.coef = nn.Parameter(torch.randn(1, out_channel))

    def packed(self):
        """(kernel [Cin, Cout], bias [Cout], coef [Cout]) as the kernels read them: detached, contiguous"""
        return self.kernel.detach().contiguous(), self.bias.detach().reshape(-1), self.coef.detach().reshape(-1)

    def forward(self, x):
        F = x.F
        if self.training or (F.requires_grad and torch.is_grad_enabled()):
            # torch.sin around the differentiable dense layer (sv_conv_fwd / sv_conv_wgrad: no GEMM with atomics)
            if F.stride(1) != 1:
                F = F.contiguous()
            arg = sparse_conv(F, self.kernel.unsqueeze(0), self.bias, None, F.shape[0], lambda: None)
            return x.new(self.coef * torch.sin(arg))
        return x.new(sinusoidal(F, *self.packed()))

    def extra_repr(self):
        return f"in={self.in_channel}, out={self.out_channel}"


class MinkowskiToSparseTensor(nn.Module):
    """ME.MinkowskiToSparseTensor on a TensorField: field.sparse() - the per-voxel mean under the field's quantisation mode
    (dense tensors, remove_zeros and coordinates= are not rebuilt)."""

    def __init__(self, remove_zeros=False, coordinates=None):
        super().__init__()
        if remove_zeros or coordinates is not None:
            raise NotImplementedError("MinkowskiToSparseTensor: only the TensorField form is built")

    def forward(self, x):
        if isinstance(x, TensorField):
            return x.sparse()
        if isinstance(x, SparseTensor):
            return x
        raise NotImplementedError("MinkowskiToSparseTensor takes a TensorField (dense tensors are not rebuilt)")


FIELD_STAGE = (MinkowskiSinusoidal, MinkowskiBatchNorm, MinkowskiReLU, MinkowskiLinear, MinkowskiBatchNorm, MinkowskiReLU,
               MinkowskiToSparseTensor)


def is_field_stage(seq):
    """exactly Sinusoidal -> BN -> ReLU -> Linear -> BN -> ReLU -> ToSparseTensor with matching widths, in eval()"""
    mods = list(seq)
    if len(mods) != len(FIELD_STAGE) or any(type(m) is not t for m, t in zip(mods, FIELD_STAGE)) or any(m.training for m in mods):
        return False
    C = mods[0].out_channel
    return (mods[1].bn.num_features == C and mods[3].linear.in_features == C and mods[3].linear.out_features == C
            and mods[4].bn.num_features == C and mods[3].compute_precision == "fp32")


def field_stage(seq, field, voxel=None):
    """One field network (is_field_stage) as ONE sv_field_stage call on the points of `field`, the input row of a point being
    [voxel.F[row of its voxel], field.F] (voxel = None: the field alone) - what seq(voxel.cat_slice(field)) computes module
    by module.  Returns the SparseTensor on the field's voxels, or None where the kernel does not cover the shape
    (SV_ERR_UNSUPPORTED): the caller then runs the modules."""
    sin, bn1, _, lin, bn2, _, _ = list(seq)
    cm, inverse, order, seg_start = field.voxelisation(reuse=True)  # a field voxelised before goes on with that manager
    V = cm.maps[1].V
    F = field.F
    G = voxel.F if voxel is not None else None
    if G is not None and (voxel.coordinate_manager is not cm or voxel.tensor_stride != 1):
        raise ValueError("the field was not voxelised into the voxel tensor's coordinate manager")
    if G is not None and G.stride(1) != 1:
        G = G.contiguous()
    N, Cf = F.shape
    Cg = G.shape[1] if G is not None else 0
    if sin.in_channel != Cg + Cf:
        raise ValueError(f"the field network takes {sin.in_channel} channels, the input rows have {Cg} + {Cf}")
    C = sin.out_channel
    kernel, bias, coef = sin.packed()
    (scale1, shift1), (scale2, shift2) = bn1.folded(), bn2.folded()
    lin_bias = lin.linear.bias.detach() if lin.linear.bias is not None else None
    out = torch.empty((V, C), dtype=torch.float32, device=F.device)
    rc = _lib.load().sv_field_stage(
        ptr(F), c_int64(F.stride(0) if N else Cf), c_int(Cf), c_int64(N), ptr(G), c_int64(G.stride(0) if Cg and V else Cg),
        c_int(Cg), ptr(inverse if Cg else None), ptr(kernel), ptr(bias), ptr(coef), ptr(scale1), ptr(shift1), ptr(lin.weight3()),
        ptr(lin_bias), ptr(scale2), ptr(shift2), c_int(C), ptr(order), ptr(seg_start), c_int64(V), ptr(out), c_int64(C),
        stream_ptr())
    if rc == _lib.SV_ERR_UNSUPPORTED:
        return None
    _lib._check(rc, "sv_field_stage")
    return SparseTensor(out, coordinate_manager=cm, tensor_stride=1, _internal=True)


class MinkowskiGlobalMaxPooling(nn.Module):
    def forward(self, x):
        if self.training:
            return PooledTensor(global_pool_train(x, _lib.SV_POOL_MAX))
        return PooledTensor(global_pool(x, _lib.SV_POOL_MAX))


class MinkowskiGlobalAvgPooling(nn.Module):
    def forward(self, x):
        if self.training:
            return PooledTensor(global_pool_train(x, _lib.SV_POOL_AVG))
        return PooledTensor(global_pool(x, _lib.SV_POOL_AVG))


class LocalPoolFunction(torch.autograd.Function):
    """out = pool(feats) over a kernel map's raw table (sv_pool_local); backward sv_pool_local_backward over the
    transposed table (t_plan: a callable, built only when the input needs a gradient) - a gather, no float atomics."""

    @staticmethod
    def forward(ctx, feats, plan, mode, t_plan):
        nbr, ld, mask = plan.raw
        f = feats.detach()
        if f.stride(1) != 1:
            f = f.contiguous()
        V_out, C = plan.V_out, f.shape[1]
        out = torch.empty((V_out, C), dtype=torch.float32, device=f.device)
        arg = torch.empty((V_out, C), dtype=torch.int32, device=f.device) if mode == _lib.SV_POOL_MAX else None
        call("sv_pool_local", ptr(f), c_int64(f.shape[0]), c_int64(f.stride(0)), c_int(C), ptr(nbr), c_int64(ld),
             c_int(plan.K), c_int64(V_out), c_int(mode), ptr(out), c_int64(C), ptr(arg), stream_ptr())
        ctx.plan, ctx.mode, ctx.t_plan, ctx.arg, ctx.V_in = plan, mode, t_plan, arg, f.shape[0]
        return out

    @staticmethod
    def backward(ctx, dy):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        if dy.stride(1) != 1:
            dy = dy.contiguous()
        nbr_t, ld_t, _ = ctx.t_plan().raw
        C = dy.shape[1]
        dx = torch.empty((ctx.V_in, C), dtype=torch.float32, device=dy.device)
        call("sv_pool_local_backward", ptr(dy), c_int64(dy.shape[0]), c_int64(dy.stride(0)), c_int(C), ptr(nbr_t),
             c_int64(ld_t), c_int(ctx.plan.K), c_int64(ctx.V_in), c_int(ctx.mode), ptr(ctx.arg), ptr(ctx.plan.raw[2]), ptr(dx),
             c_int64(C), stream_ptr())
        return dx, None, None, None


class _LocalPoolBase(nn.Module):
    """ME.MinkowskiMaxPooling / AvgPooling / SumPooling(kernel_size, stride, dilation, dimension) on the kernel maps the
    convolutions use: kernel_size 2 stride 2 on the down map, kernel_size 3 / 1 with any stride on the strided (stride 1: the
    3x3x3) maps.  An even kernel starts at the output coordinate, an odd one is centred on it."""
    MODE = None

    def __init__(self, kernel_size, stride=1, dilation=1, kernel_generator=None, dimension=None):
        super().__init__()
        if dimension != 3:
            raise NotImplementedError("only dimension=3 (the reference passes D=3 everywhere)")
        self.kernel_size, self.stride, self.dilation, self.dimension = kernel_size, stride, dilation, dimension

    def _plans(self, x):
        maps = layer_maps(self.kernel_size, self.stride, self.dilation, pooling=True)
        return x.coordinate_manager.layer_plans(maps, x.tensor_stride)[:3]

    def forward(self, x):
        plan, out_stride, t_plan = self._plans(x)
        return x.new(LocalPoolFunction.apply(x.F, plan, self.MODE, t_plan), tensor_stride=out_stride)

    def extra_repr(self):
        return f"kernel_size={self.kernel_size}, stride={self.stride}, dilation={self.dilation}"


class MinkowskiMaxPooling(_LocalPoolBase):
    MODE = _lib.SV_POOL_MAX


class MinkowskiAvgPooling(_LocalPoolBase):
    MODE = _lib.SV_POOL_AVG


class MinkowskiSumPooling(_LocalPoolBase):
    MODE = _lib.SV_POOL_SUM


def _frame_offsets(x):
    """(batch_start int32[B + 1] on the device, B) of a sparse tensor's map"""
    cm = x.coordinate_manager
    return cm.batch_offsets(x.tensor_stride, cm.batches()), cm.batches()


class InstanceNormFunction(torch.autograd.Function):
    """y = act(instance_norm(x) * weight + bias) per (frame, channel) in float64 (sv_instance_norm); backward
    sv_instance_norm_backward (dx, dweight, dbias through the same fixed summation tree)."""

    @staticmethod
    def forward(ctx, feats, weight, bias, batch_start, B, eps, act):
        f = feats.detach()
        if f.stride(1) != 1:
            f = f.contiguous()
        V, C = f.shape
        w, b = weight.detach().reshape(-1).contiguous(), bias.detach().reshape(-1).contiguous()
        nbytes = _lib.load().sv_instance_norm_workspace_bytes(c_int64(V), c_int(B), c_int(C))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=f.device)
        y = torch.empty((V, C), dtype=torch.float32, device=f.device)
        mean = torch.empty((B, C), dtype=torch.float64, device=f.device)
        inv_std = torch.empty((B, C), dtype=torch.float64, device=f.device)
        call("sv_instance_norm", ptr(f), c_int64(V), c_int64(f.stride(0)), c_int(C), ptr(batch_start), c_int(B), ptr(w), ptr(b),
             c_double(eps), c_int(act), ptr(ws), c_size_t(nbytes), ptr(y), c_int64(C), ptr(mean), ptr(inv_std), stream_ptr())
        ctx.save_for_backward(f, w, b, mean, inv_std, batch_start)
        ctx.B, ctx.act, ctx.wshape, ctx.bshape = B, act, weight.shape, bias.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        f, w, b, mean, inv_std, batch_start = ctx.saved_tensors
        if dy.stride(1) != 1:
            dy = dy.contiguous()
        V, C = f.shape
        nbytes = _lib.load().sv_instance_norm_workspace_bytes(c_int64(V), c_int(ctx.B), c_int(C))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=f.device)
        dx = torch.empty((V, C), dtype=torch.float32, device=f.device)
        dw = torch.empty(C, dtype=torch.float32, device=f.device)
        db = torch.empty(C, dtype=torch.float32, device=f.device)
        call("sv_instance_norm_backward", ptr(f), c_int64(V), c_int64(f.stride(0)), c_int(C), ptr(batch_start), c_int(ctx.B),
             ptr(w), ptr(b), ptr(mean), ptr(inv_std), c_int(ctx.act), ptr(dy), c_int64(dy.stride(0)), ptr(ws), c_size_t(nbytes),
             ptr(dx), c_int64(C), ptr(dw), ptr(db), stream_ptr())
        return dx, dw.reshape(ctx.wshape), db.reshape(ctx.bshape), None, None, None, None


class MinkowskiInstanceNorm(nn.Module):
    """ME.MinkowskiInstanceNorm(num_features): per (frame, channel) normalisation with biased variance, eps = 1e-8,
    `weight` / `bias` of shape [1, C] (ME 0.5.4 from memory - include/sv_hip.h).  forward_fused applies the activation that
    follows in the same call (SV_ACT_RELU / SV_ACT_GELU)."""

    def __init__(self, num_features):
        super().__init__()
        self.num_features = num_features
        self.eps = 1e-8
        self.weight = nn.Parameter(torch.ones(1, num_features))
        self.bias = nn.Parameter(torch.zeros(1, num_features))

    def forward_fused(self, x, act=SV_ACT_NONE):
        if x.F.shape[1] != self.num_features:
            raise ValueError(f"input has {x.F.shape[1]} channels, MinkowskiInstanceNorm expects {self.num_features}")
        bs, B = _frame_offsets(x)
        return x.new(InstanceNormFunction.apply(x.F, self.weight, self.bias, bs, B, self.eps, act))

    def forward(self, x):
        return self.forward_fused(x)

    def extra_repr(self):
        return f"{self.num_features}, eps={self.eps}"


class MinkowskiGELU(nn.Module):
    # exact (erf) GELU on the features; inside a ResNet in eval() it is fused into the instance norm before it
    def forward(self, x):
        f = torch.nn.functional.gelu
        return x.new(f(x.F)) if isinstance(x, SparseTensor) else f(x)


class MinkowskiDropout(nn.Module):
    def __init__(self, p=0.5, inplace=False):
        super().__init__()
        self.p = p

    def forward(self, x):
        if not self.training:
            return x
        return x.new(torch.dropout(x.F, self.p, True))


class PooledTensor:
    """Result of global pooling: one row per batch index; `.F/.features` as on ME's pooled SparseTensor."""

    def __init__(self, feats):
        self._F = feats

    @property
    def F(self):
        return self._F

    features = F


class BasicBlock(nn.Module):
    """MinkowskiEngine.modules.resnet_block.BasicBlock (expansion 1): conv3-BN-ReLU-conv3-BN-(+res)-ReLU."""
    expansion = 1
    NORM_TYPE = "BN"

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, bn_momentum=0.1, dimension=-1):
        super().__init__()
        assert dimension > 0
        self.conv1 = MinkowskiConvolution(inplanes, planes, kernel_size=3, stride=stride, dilation=dilation,
                                          dimension=dimension)
        self.norm1 = MinkowskiBatchNorm(planes, momentum=bn_momentum)
        self.conv2 = MinkowskiConvolution(planes, planes, kernel_size=3, stride=1, dilation=dilation,
                                          dimension=dimension)
        self.norm2 = MinkowskiBatchNorm(planes, momentum=bn_momentum)
        self.relu = MinkowskiReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        out = self.conv1.forward_fused(x, bn=self.norm1, act=SV_ACT_RELU)
        if self.downsample is not None:
            ds_conv, ds_bn = self.downsample[0], self.downsample[1]
            residual = ds_conv.forward_fused(x, bn=ds_bn)
        else:
            residual = x
        return self.conv2.forward_fused(out, bn=self.norm2, residual=residual, act=SV_ACT_RELU)


class Bottleneck(nn.Module):
    """MinkowskiEngine.modules.resnet_block.Bottleneck (expansion 4): 1x1-BN-ReLU-3x3-BN-ReLU-1x1-BN-(+res)-ReLU."""
    expansion = 4
    NORM_TYPE = "BN"

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, bn_momentum=0.1, dimension=-1):
        super().__init__()
        assert dimension > 0
        self.conv1 = MinkowskiConvolution(inplanes, planes, kernel_size=1, dimension=dimension)
        self.norm1 = MinkowskiBatchNorm(planes, momentum=bn_momentum)
        self.conv2 = MinkowskiConvolution(planes, planes, kernel_size=3, stride=stride, dilation=dilation,
                                          dimension=dimension)
        self.norm2 = MinkowskiBatchNorm(planes, momentum=bn_momentum)
        self.conv3 = MinkowskiConvolution(planes, planes * self.expansion, kernel_size=1, dimension=dimension)
        self.norm3 = MinkowskiBatchNorm(planes * self.expansion, momentum=bn_momentum)
        self.relu = MinkowskiReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        out = self.conv1.forward_fused(x, bn=self.norm1, act=SV_ACT_RELU)
        out = self.conv2.forward_fused(out, bn=self.norm2, act=SV_ACT_RELU)
        if self.downsample is not None:
            residual = self.downsample[0].forward_fused(x, bn=self.downsample[1])
        else:
            residual = x
        return self.conv3.forward_fused(out, bn=self.norm3, residual=residual, act=SV_ACT_RELU)


def kaiming_normal_(tensor, mode="fan_out", nonlinearity="relu"):
    """ME.utils.kaiming_normal_ on a [K, Cin, Cout] kernel (model/backbone/resnet.py:89):
    fan_in = K * Cin, fan_out = K * Cout, std = sqrt(2 / fan)."""
    if tensor.dim() == 3:
        K, cin, cout = tensor.shape
    else:
        K, (cin, cout) = 1, tensor.shape
    fan = K * cout if mode == "fan_out" else K * cin
    gain = nn.init.calculate_gain(nonlinearity)
    std = gain / math.sqrt(fan)
    with torch.no_grad():
        return tensor.normal_(0, std)
