"""CASES: one table of (name, entries, build, run) over every launching entry point of the library, for
tests/test_gpu_hostile_memory.py and tests/test_gpu_side_stream.py (harness: tests/hostile_helpers.py).

  build(gpu) -> dict of inputs: device tensors (the names in `late` arrive late on the side stream) and host objects.
  run(inputs) -> tuple of tensors: what the wrapper's docstring or include/sv_hip.h defines, nothing else (rows past a
                 returned count, padding rows of plans and capacity tails are sliced off).  Everything that allocates -
                 coordinate managers, plans, hash tables, ray tables, folded weights, weight packs - is built in here.
  steps        wrapper calls of run that sit behind a delay of their own on the side stream (_arm).
  poison       {name: value} for late tensors whose poison must not be the default (0xFF bytes for floats and bytes, 0 for
                 int32 / int64): -1 where an entry defines it as "absent", 0 for float tables that hold offsets.
  workspace(inputs) -> byte counts of the case's *_workspace_bytes contracts: each must be the exact size of an
                 allocation made inside the hostile block.
  reference(inputs, outs): holds the plain run to an independent reference where a tests/*_helpers.py module has one.
The two training networks copy their model inside run (a step changes it), so their second turn on another stream shares no
cache with the first: the cross-stream ordering of parameter-derived caches is tested by unet_eval and engine_stream.
Shapes are the smallest of the existing edge tests at which a kernel has more than one tile, block or pass."""
import copy
import ctypes
from collections import namedtuple
from ctypes import c_float, c_int, c_int64, c_size_t

import numpy as np
import torch

Case = namedtuple("Case", "name entries build run late poison workspace reference network cleanup steps")
CASES = []


def case(name, entries, build, run, late=(), poison=None, workspace=None, reference=None, network=False, cleanup=None,
         steps=1):
    CASES.append(Case(name, tuple(entries), build, run, tuple(late), dict(poison or {}), workspace, reference, network,
                      cleanup, steps))


def _arm(i, *tensors, fill=None, fills=None):
    """A step of a run: on the side stream the tensors the NEXT wrapper call reads are poisoned and restored behind a fresh
    delay (tests/test_gpu_side_stream.py puts the hook into the inputs); anywhere else this does nothing.  `steps` of a
    case = its _arm calls + 1."""
    hook = i.get("_arm")
    if hook is not None:
        keep = [j for j, t in enumerate(tensors) if t is not None]
        fills = [fill] * len(tensors) if fills is None else list(fills)  # fills: one poison value per tensor (None: the default)
        hook([tensors[j] for j in keep], [fills[j] for j in keep])


def _L():
    from mrcc_amd import _lib

    return _lib


def _ws(fn, *args):
    return int(getattr(_L().load(), fn)(*args))


def _t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


def _host(a):
    """a host result (numpy array or scalar) as a tensor, so that every case returns tensors"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a)))


def _ints(shape, lo, hi, seed, dev, zero_rows=0.0):
    import conv_exact_helpers as H

    return H.int_tensor(shape, lo, hi, seed, zero_rows).to(dev)


def _plan_arrays(plan):
    """what include/sv_hip.h defines of a plan: the raw table and mask of the V output rows, the sorted arrays up to V"""
    nbr, _, mask = plan.raw
    V = plan.V_out
    return [nbr[:, :V], mask[:V], plan.perm, plan.nbr_s[:, :V], plan.submask, plan.tile_order]  # perm: -1 in the padding


# =====================================================================================================================
# coordinates
# =====================================================================================================================
def _two_frames():
    """the two-frame batch of tests/strided_helpers.py (835 + 640 voxels, the second frame at negative coordinates) with 300
    of its rows repeated, so that the voxel reduction averages"""
    import strided_helpers as S

    c = S.frame_input("two")
    rng = np.random.default_rng(11)
    c = np.concatenate([c, c[rng.permutation(len(c))[:300]]])
    return c[rng.permutation(len(c))], 1475


def _coords_build(gpu):
    c, V = _two_frames()
    g = torch.Generator().manual_seed(3)
    return dict(coords=_t(c, gpu, torch.int32), feats=torch.rand(len(c), 3, generator=g).to(gpu), V=V, N=len(c))


def _coords_run(i):
    from mrcc_amd import MinkowskiEngine as ME

    st = ME.SparseTensor(i["feats"], coordinates=i["coords"], device=i["feats"].device,
                         quantization_mode=ME.SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE)
    cm = st.coordinate_manager
    m1 = cm.stride_map(1)
    _arm(i, m1.keys)
    m2 = cm.stride_map(2)
    _arm(i, m2.keys)
    m4 = cm.stride_map(4)
    _arm(i, m1.keys)
    m3 = cm.stride_map(3)
    plans = []
    for make in (lambda: cm.plan_k3(1), lambda: cm.plan_k3(1, 2), lambda: cm.plan_down(1), lambda: cm.plan_up(2),
                 lambda: cm.plan_strided(1, 3, 2), lambda: cm.plan_strided_t(1, 3, 2)):
        _arm(i, m1.keys, m1.coords, m2.keys, m2.coords, cm.parents[1][0])  # what the hash, the map kernel and the plan read
        plans.append(make())
    _arm(i, m1.keys, m2.keys)
    outs = [st.F, st.inverse_mapping, m1.keys, m1.coords, m2.keys, m2.coords, m4.keys, m4.coords, m3.keys, m3.coords,
            cm.parents[1][0], cm.parents[1][1], cm.parents[2][0], cm.general_parents[(1, 3)], cm.batch_offsets(1, 2),
            cm.batch_offsets(2, 2)]
    for p in plans:
        outs += _plan_arrays(p)
    return tuple(outs)


def _coords_ref(i, outs):
    import strided_helpers as S

    assert np.array_equal(outs[3].numpy(), S.frame_coords("two"))
    for at, kind in ((1, "k3d2"), (4, "k3s2"), (5, "k3s2_t")):
        nbr = outs[16 + 6 * at].numpy()
        assert np.array_equal(nbr, S.kind_table("two", kind)[0]), kind
    assert outs[14].tolist() == S.batch_bounds_ref(S.frame_coords("two"), 2)


case("coords_piecewise",
     ["sv_voxelize", "sv_voxel_reduce", "sv_hash_build", "sv_stride_map", "sv_stride_map_general", "sv_kernel_map_k3",
      "sv_kernel_map_down", "sv_kernel_map_up", "sv_kernel_map_probe", "sv_plan_build", "sv_batch_offsets"],
     _coords_build, _coords_run, late=("coords", "feats"), steps=11,
     workspace=lambda i: [_ws("sv_voxelize_workspace_bytes", i["N"]), _ws("sv_stride_map_workspace_bytes", i["V"]),
                          _ws("sv_stride_map_general_workspace_bytes", i["V"]), _ws("sv_plan_workspace_bytes", i["V"])],
     reference=_coords_ref)


def _frame_build(gpu):
    c, V = _two_frames()
    g = torch.Generator().manual_seed(4)
    return dict(coords=_t(c.astype(np.float32) + np.float32(0.25), gpu), feats=torch.rand(len(c), 3, generator=g).to(gpu),
                V=V, N=len(c))


def _frame_run(i):
    from mrcc_amd import MinkowskiEngine as ME

    field = ME.TensorField(i["feats"], i["coords"], device=i["feats"].device)
    x = field.sparse(pyramid_levels=3)
    cm = x.coordinate_manager
    cm.split_rules = [(1000, (9, 18))]  # the 1475-voxel level runs its wide 3x3x3 layers as three offset-range passes
    _arm(i, *[t for lv in range(4) for t in (cm.maps[1 << lv].keys, cm.maps[1 << lv].coords)], *[cm.parents[1 << lv][0] for lv in range(3)])
    cm.build_plans(3)
    outs = [x.F, field.inverse_mapping]
    for lv in range(4):
        m = cm.maps[1 << lv]
        outs += [m.keys, m.coords]
        if lv < 3:
            outs += list(cm.parents[1 << lv])
            outs += _plan_arrays(cm.plans[("down", 1 << lv)]) + _plan_arrays(cm.plans[("up", 2 << lv)])
        outs += _plan_arrays(cm.plans[("k3", 1 << lv, 1)])
    for _, _, sub in cm.plans[("k3split", 1, (9, 18))].parts:
        outs += _plan_arrays(sub)
    return tuple(outs)


def _frame_ref(i, outs):
    import strided_helpers as S

    assert np.array_equal(outs[3].numpy(), S.frame_coords("two"))


def _frame_ws(i):
    import strided_helpers as S

    c = S.frame_coords("two")
    V = (c_int64 * 4)(len(c), *[len(S.stride_map_ref(c, s)[0]) for s in (2, 4, 8)])  # the level sizes, from the reference
    cuts = (ctypes.c_int32 * (4 * _L().SV_FRAME_MAX_CUTS))()
    cuts[0], cuts[1] = 9, 18  # level 0 alone reaches the split rule
    flags = _L().SV_FRAME_K3 | _L().SV_FRAME_DOWN | _L().SV_FRAME_UP | _L().SV_FRAME_SPLIT
    return [_ws("sv_frame_maps_arena_bytes", i["N"], 3), _ws("sv_frame_maps_scratch_bytes", i["N"]),
            _ws("sv_frame_plans_arena_bytes", V, 3, flags, cuts), _ws("sv_frame_plans_scratch_bytes", V, 3)]


case("coords_frame", ["sv_frame_maps", "sv_frame_plans", "sv_voxel_reduce"], _frame_build, _frame_run,
     late=("coords", "feats"), workspace=_frame_ws, reference=_frame_ref, steps=2)


# =====================================================================================================================
# convolution forward: one shape per kernel family of the dispatch table, small-integer operands (exact)
# =====================================================================================================================
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
# (label, map, Cin, Cout, family of sv_conv_last_instance, epilogue)
CONV_SPECIAL = (("first", "k3", 3, 32, "conv_first_mfma_kernel", "bn_relu"), ("thin", "k3", 32, 32, "conv_thin_kernel", "raw"),
                ("dense", "dense", 64, 96, "conv_fwd_kernel", "bias"), ("narrow", "dense", 96, 3, "linear_narrow_kernel", "bias"))
CONV_TILES = (("tiled", "k3", 64, 64, "conv_fwd_kernel", "res_leaky"), ("wide_split", "k3split", 384, 384, "conv_fwd_kernel", "bn_relu"),
              ("down", "down", 32, 64, "conv_fwd_kernel", "raw"), ("up", "up", 64, 32, "conv_fwd_kernel", "bn_relu"),
              ("k3s2", "k3s2", 64, 64, "conv_fwd_kernel", "res_leaky"))
_MAP_K = {"k3": 27, "k3split": 27, "dense": 1, "down": 8, "up": 8, "k3s2": 27}
V_DENSE = 300  # rows of the dense (K = 1, no plan) shapes: three row tiles, the last one partial


def _conv_cm(coords, dev):
    from mrcc_amd import MinkowskiEngine as ME

    st = ME.SparseTensor(torch.zeros(coords.shape[0], 1, device=dev), coordinates=coords, device=dev)
    cm = st.coordinate_manager
    cm.plan_down(1)
    return cm


def _conv_map(cm, kind):
    """(plan, raw table, V_in, V_out) of a map kind on the frame"""
    import conv_exact_helpers as H

    V1, V2 = cm.stride_map(1).V, cm.stride_map(2).V
    if kind == "dense":
        return None, H.dense_nbr(V_DENSE, cm.device), V_DENSE, V_DENSE
    plan = {"k3": lambda: cm.plan_k3(1), "k3split": lambda: cm.plan_k3_split(1, 14), "down": lambda: cm.plan_down(1),
            "up": lambda: cm.plan_up(2), "k3s2": lambda: cm.plan_strided(1, 3, 2)}[kind]()
    whole = plan.whole if kind == "k3split" else plan
    V_in, V_out = {"k3": (V1, V1), "k3split": (V1, V1), "down": (V1, V2), "up": (V2, V1), "k3s2": (V1, V2)}[kind]
    assert whole.V_out == V_out
    return plan, whole.raw[0], V_in, V_out


def _conv_build(shapes):
    def build(gpu):
        import strided_helpers as S

        c = S.frame_input("two")
        V1, V2 = len(c), len(S.stride_map_ref(S.frame_coords("two"), 2)[0])
        i = dict(coords=_t(c, gpu, torch.int32))
        for j, (label, kind, cin, cout, _, epi) in enumerate(shapes):
            V_in, V_out = {"k3": (V1, V1), "k3split": (V1, V1), "down": (V1, V2), "up": (V2, V1), "k3s2": (V1, V2),
                           "dense": (V_DENSE, V_DENSE)}[kind]
            i[f"x_{label}"] = _ints((V_in, cin), -4, 4, 100 + j, gpu, zero_rows=0.2)
            i[f"W_{label}"] = _ints((_MAP_K[kind], cin, cout), -3, 3, 200 + j, gpu)
            i[f"shift_{label}"] = _ints((cout,), -8, 8, 300 + j, gpu)
            i[f"res_{label}"] = _ints((V_out, cout), -8, 8, 400 + j, gpu, zero_rows=0.2)
        import conv_exact_helpers as H

        i["scales"] = {label: H.scale_tensor(cout, 500 + j).to(gpu) for j, (label, _, _, cout, _, _) in enumerate(shapes)}
        return i

    return build


def _epilogue(i, label, epi):
    """(scale, shift, residual, act) of an epilogue name"""
    if epi == "raw":
        return None, None, None, ACT_NONE
    if epi == "bias":
        return None, i[f"shift_{label}"], None, ACT_NONE
    if epi == "bn_relu":
        return i["scales"][label], i[f"shift_{label}"], None, ACT_RELU
    return i["scales"][label], i[f"shift_{label}"], i[f"res_{label}"], ACT_LEAKY


def _conv_run(shapes, plain_entry):
    def run(i):
        import conv_exact_helpers as H
        from mrcc_amd import _lib
        from mrcc_amd import nn as svnn

        cm = _conv_cm(i["coords"], i["coords"].device)
        outs = []
        maps = {kind: _conv_map(cm, kind) for kind in {s[1] for s in shapes}}  # the plans first: their maps read sizes back
        for label, kind, cin, cout, family, epi in shapes:
            plan, _, V_in, V_out = maps[kind]
            scale, shift, res, act = _epilogue(i, label, epi)
            _arm(i, i[f"x_{label}"], i[f"W_{label}"], scale, shift, res)
            out = svnn.conv_forward(i[f"x_{label}"], i[f"W_{label}"], plan, V_out, scale, shift, res, act, H.LEAKY_SLOPE)
            name = _lib.conv_last_instance()[0]
            assert name.split("<")[0] == family, (label, name, family)
            outs.append(out)
        if plain_entry:  # sv_conv_fwd itself (no accumulator argument): the dense shape again, called as the header declares it
            x, W = i["x_dense"], i["W_dense"]
            _arm(i, x, W, i["shift_dense"])
            V, cout = x.shape[0], W.shape[2]
            out = torch.empty((V, cout), dtype=torch.float32, device=x.device)
            Vpad = (V + 127) // 128 * 128
            _lib.call("sv_conv_fwd", _lib.ptr(x), c_int64(V), c_int64(x.stride(0)), c_int(x.shape[1]), _lib.ptr(W), c_int(1),
                      c_int(cout), None, None, None, None, c_int64(V), c_int64(Vpad), None, _lib.ptr(i["shift_dense"]), None,
                      c_int64(0), c_int(ACT_NONE), c_float(0.0), _lib.ptr(out), c_int64(cout), _lib.stream_ptr())
            outs.append(out)
        return tuple(outs)

    return run


def _conv_ref(shapes, plain_entry):
    def ref(i, outs):
        import conv_exact_helpers as H

        cm = _conv_cm(i["coords"], i["coords"].device)
        for j, (label, kind, cin, cout, _, epi) in enumerate(shapes):
            _, nbr, V_in, V_out = _conv_map(cm, kind)
            x, W = i[f"x_{label}"], i[f"W_{label}"]
            H.assert_exact_range(x, W, nbr, V_out)
            scale, shift, res, act = _epilogue(i, label, epi)
            want = H.ref_epilogue(H.ref_forward(x, W, nbr, V_out), scale, shift, res, act).cpu()
            assert H.same_bits(outs[j], want), f"{label}: the plain run differs from the int64 reference"
        if plain_entry:
            assert H.same_bits(outs[-1], outs[[s[0] for s in shapes].index("dense")])

    return ref


def _conv_late(shapes):
    return ("coords",) + tuple(f"{p}_{s[0]}" for s in shapes for p in ("x", "W", "shift", "res"))


case("conv_fwd_special", ["sv_conv_fwd_acc", "sv_conv_fwd"], _conv_build(CONV_SPECIAL), _conv_run(CONV_SPECIAL, True),
     late=_conv_late(CONV_SPECIAL), reference=_conv_ref(CONV_SPECIAL, True), steps=6)
case("conv_fwd_tiles", ["sv_conv_fwd_acc"], _conv_build(CONV_TILES), _conv_run(CONV_TILES, False),
     late=_conv_late(CONV_TILES), reference=_conv_ref(CONV_TILES, False), steps=6)


# ---- bf16 forward and both weight gradients, 64 -> 96 at K = 27 ------------------------------------------------------
def _grad_build(gpu):
    import strided_helpers as S

    c = S.frame_input("two")
    V = len(c)
    return dict(coords=_t(c, gpu, torch.int32), x=_ints((V, 64), -4, 4, 1, gpu, zero_rows=0.2), W=_ints((27, 64, 96), -3, 3, 2, gpu),
                dy=_ints((V, 96), -3, 3, 3, gpu, zero_rows=0.2), dW0=_ints((27, 64, 96), -50, 50, 4, gpu), V=V)


def _grad_run(i):
    from mrcc_amd import _lib
    from mrcc_amd import nn as svnn

    cm = _conv_cm(i["coords"], i["coords"].device)
    plan = cm.plan_k3(1)
    V = plan.V_out
    _arm(i, i["W"])
    wp = svnn.pack_weights_bf16(i["W"])
    _arm(i, i["x"], wp)
    y = svnn.conv_forward(i["x"], i["W"], plan, V, weight_bf16=wp)
    assert _lib.conv_last_instance()[0].startswith("conv_bf16_kernel")
    outs = [wp, y]
    for bf16 in (False, True):
        used = set()
        _arm(i, i["x"], i["dy"])
        outs.append(svnn.conv_wgrad(i["x"], i["dy"], plan, 27, 64, 96, bf16=bf16, used=used))  # accumulate = 0
        assert used == {"sv_conv_wgrad_bf16" if bf16 else "sv_conv_wgrad"}, used
        acc = i["dW0"].clone()
        _arm(i, i["x"], i["dy"], acc)
        assert svnn._wgrad_one(i["x"], i["dy"], plan, 27, 64, 96, V, acc, True, bf16) == (  # accumulate = 1
            "sv_conv_wgrad_bf16" if bf16 else "sv_conv_wgrad")
        outs.append(acc)
    return tuple(outs)


def _grad_ref(i, outs):
    import conv_exact_helpers as H

    cm = _conv_cm(i["coords"], i["coords"].device)
    nbr, V = cm.plan_k3(1).raw[0], i["V"]
    H.assert_exact_range(i["x"], i["W"], nbr, V)
    H.assert_exact_range(i["x"], i["dy"], nbr, V)
    assert torch.equal(outs[1].double(), H.ref_forward(i["x"], i["W"], nbr, V).cpu().double())
    dW = H.ref_wgrad(i["x"], i["dy"], nbr, V).cpu().double()
    for j in (2, 4):
        assert torch.equal(outs[j].double(), dW) and torch.equal(outs[j + 1].double(), dW + i["dW0"].cpu().double())


def _grad_ws(i):
    Vpad = (i["V"] + 127) // 128 * 128
    return [_ws("sv_conv_wgrad_workspace_bytes", Vpad, 27, 64, 96), _ws("sv_conv_wgrad_bf16_workspace_bytes", Vpad, 27, 64, 96)]


case("conv_bf16_and_gradients", ["sv_pack_weights_bf16", "sv_conv_fwd_bf16", "sv_conv_wgrad", "sv_conv_wgrad_bf16"],
     _grad_build, _grad_run, late=("coords", "x", "W", "dy", "dW0"), workspace=_grad_ws, reference=_grad_ref, steps=7)


# =====================================================================================================================
# activation, pooling, norm, slicing, preprocessing (C = 96, B = 2, V = 1475)
# =====================================================================================================================
def _act_build(gpu):
    c, V = _two_frames()
    g = torch.Generator().manual_seed(6)
    r = lambda *s: torch.randn(*s, generator=g).to(gpu)  # noqa: E731
    return dict(coords=_t(c.astype(np.float32) + np.float32(0.5), gpu), feats=r(len(c), 3), F=r(V, 96), scale=r(96), shift=r(96),
                res=r(V, 96), points=r(1025, 3), V=V)


def _act_run(i):
    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd import _lib
    from mrcc_amd import nn as svnn
    from mrcc_amd.utils import preprocess

    field = ME.TensorField(i["feats"], i["coords"], device=i["feats"].device)
    x = field.sparse().new(i["F"])
    x.coordinate_manager.batches()  # the one size read-back of the pooling, before its delay
    steps = (lambda: x.slice_argmax(field), lambda: preprocess.center_at_origin(i["points"]),
             lambda: preprocess.base_at_origin(i["points"]),
             lambda: (svnn.affine_act(i["F"], i["scale"], i["shift"], i["res"], _lib.SV_ACT_LEAKY_RELU, 0.25),),
             lambda: (svnn.affine_act(i["F"], act=_lib.SV_ACT_RELU),), lambda: (svnn.global_pool(x, _lib.SV_POOL_MAX),),
             lambda: (svnn.global_pool(x, _lib.SV_POOL_AVG),), lambda: (x.slice(field).F,))
    outs = []
    for step in steps:
        _arm(i, i["F"], i["scale"], i["shift"], i["res"], i["points"], field.inverse_mapping, x.coordinate_manager.stride_map(1).keys)
        outs += list(step())
    return tuple(outs)


case("act_pool_slice_stats", ["sv_affine_act", "sv_global_pool", "sv_slice_rows", "sv_slice_argmax", "sv_col_stats",
                              "sv_center_scale", "sv_voxelize", "sv_voxel_reduce", "sv_batch_offsets"],
     _act_build, _act_run, late=("coords", "feats", "F", "scale", "shift", "res", "points"), steps=9,
     workspace=lambda i: [_ws("sv_col_stats_workspace_bytes", 1025)])


def _norm_build(gpu):
    import strided_helpers as S

    c = S.frame_input("two")
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g).to(gpu)  # noqa: E731
    V1, V2 = len(c), len(S.stride_map_ref(S.frame_coords("two"), 2)[0])
    return dict(coords=_t(c, gpu, torch.int32), F=r(V1, 96), dy_pool=r(V2, 96), dy_norm=r(V1, 96), weight=r(1, 96), bias=r(1, 96),
                V=V1)


def _norm_run(i):
    from mrcc_amd import MinkowskiEngine as ME
    from mrcc_amd import _lib
    from mrcc_amd import nn as svnn

    dev = i["F"].device
    st = ME.SparseTensor(torch.zeros(i["coords"].shape[0], 1, device=dev), coordinates=i["coords"], device=dev)
    outs = []
    pools = ((svnn.MinkowskiMaxPooling(3, 2, dimension=3), i["dy_pool"]), (svnn.MinkowskiAvgPooling(2, 2, dimension=3), i["dy_pool"]),
             (svnn.MinkowskiSumPooling(3, 1, dimension=3), i["dy_norm"]))
    st.coordinate_manager.stride_map(2)  # the coarse map's size read-back and every kernel map, before the delays
    for pool, _ in pools:
        pool._plans(st)[2]()
    for pool, dy in pools:
        f = i["F"].detach().clone().requires_grad_(True)
        _arm(i, f.detach())  # the pooling saves no input: its rows may be written to before the backward
        y = pool(st.new(f)).F
        _arm(i, dy)
        y.backward(dy)
        outs += [y.detach(), f.grad]
    f = i["F"].detach().clone().requires_grad_(True)
    w, b = i["weight"].detach().clone().requires_grad_(True), i["bias"].detach().clone().requires_grad_(True)
    x = st.new(f)
    bs, B = svnn._frame_offsets(x)
    _arm(i, f.detach(), w.detach(), b.detach(), bs)
    y = svnn.InstanceNormFunction.apply(f, w, b, bs, B, 1e-8, _lib.SV_ACT_RELU)
    _arm(i, i["dy_norm"])  # not what the forward saved: autograd refuses saved tensors that were written to
    mean, inv_std = y.grad_fn.saved_tensors[3:5]  # float64 [B, C], defined by the header: what the backward is given
    y.backward(i["dy_norm"])
    return tuple(outs + [y.detach(), f.grad, w.grad, b.grad, mean, inv_std])


def _transposed(fwd, V_in):
    """nbr_t[k][i] = o exactly when nbr[k][o] = i"""
    tr = np.full((fwd.shape[0], V_in), -1, np.int32)
    k, o = np.nonzero(fwd >= 0)
    tr[k, fwd[k, o]] = o
    return tr


def _norm_ref(i, outs):
    """tests/strided_helpers.py as tests/test_gpu_pool_local_edges.py and tests/test_gpu_instance_norm_edges.py use it: the
    pooling forward exact, its backward exact against the float32 restatement and within pool_backward_bound of float64;
    the instance norm within norm_forward_bound, its statistics within 2^-40, its gradients within the existing bounds"""
    import strided_helpers as S

    o = [t.numpy() for t in outs]
    x = i["F"].cpu().numpy()
    c1 = S.frame_coords("two")
    c2 = S.stride_map_ref(c1, 2)[0]
    tables = ((0, S.kind_table("two", "k3s2")[0], "dy_pool"), (1, S.k2_table_ref(c2, c1), "dy_pool"),
              (2, S.probe_ref(c1, c1, 3, 1), "dy_norm"))
    for at, (mode, fwd, dyk) in enumerate(tables):
        dy = i[dyk].cpu().numpy()
        want, arg = S.pool_ref(x, fwd, mode)
        assert np.array_equal(o[2 * at], want, equal_nan=True), mode
        tr, count = _transposed(fwd, len(c1)), (fwd >= 0).sum(0)
        assert np.array_equal(o[2 * at + 1], S.pool_backward32_ref(dy, tr, mode, arg, count)), mode
        err = np.abs(o[2 * at + 1] - S.pool_backward_ref(dy, fwd, mode, arg, len(c1)))
        assert (err <= S.pool_backward_bound(dy, tr, mode, arg, count)).all(), mode
    starts = np.array(S.batch_bounds_ref(c1, 2))
    w, b, dy = i["weight"].cpu().numpy().reshape(-1), i["bias"].cpu().numpy().reshape(-1), i["dy_norm"].cpu().numpy()
    y, dx, dw, db, mean, inv_std = o[6:12]
    want = S.instance_norm_ref(x, starts, w, b, 1e-8, 1)
    assert (np.abs(y.astype(np.float64) - want) <= S.norm_forward_bound(want)).all()
    want_m, want_i = S.instance_norm_stats_ref(x, starts, 1e-8)
    assert (np.abs(mean - want_m) <= 2.0 ** -40 * np.abs(want_m)).all() and (np.abs(inv_std - want_i) <= 2.0 ** -40 * np.abs(want_i)).all()
    rdx, rdw, rdb, noise, nw, nb = S.instance_norm_backward_ref(x, starts, w, b, mean, inv_std, 1, dy)
    assert (np.abs(dx - rdx) <= 2.0 ** -23 * np.abs(rdx) + 2.0 ** -40 * noise).all()
    assert (np.abs(dw.reshape(-1) - rdw) <= 2.0 ** -23 * np.abs(rdw) + 2.0 ** -40 * nw).all()
    assert (np.abs(db.reshape(-1) - rdb) <= 2.0 ** -23 * np.abs(rdb) + 2.0 ** -40 * nb).all()


case("pool_local_instance_norm", ["sv_pool_local", "sv_pool_local_backward", "sv_instance_norm", "sv_instance_norm_backward"],
     _norm_build, _norm_run, late=("coords", "F", "dy_pool", "dy_norm", "weight", "bias"), steps=9, reference=_norm_ref,
     workspace=lambda i: [_ws("sv_instance_norm_workspace_bytes", i["V"], 2, 96)])


# =====================================================================================================================
# post-processing and pose
# =====================================================================================================================
def _post_build(gpu):
    g = torch.Generator().manual_seed(8)
    N, C = 3000, 9
    out = torch.randn(N, 3, generator=g)
    out[5, 1] = out[1700, 1] = out[1701, 1]  # ties
    logits = torch.randn(N, C, generator=g) * 3
    lengths = [0, 1, 257, 0, 2742]
    pts = np.random.default_rng(20).uniform(-0.2, 0.2, (1200, 3)).astype(np.float32)  # no pair within 1e-6 of the threshold
    pts[:500] = pts[:500] * 0.15 + 0.5  # one dense blob: the largest cluster; the rest is scattered
    rng = np.random.default_rng(9)
    a = rng.uniform(-0.1, 0.1, size=(8, 6, 3))
    Rm = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    b = a @ (Rm * np.sign(np.linalg.det(Rm))).T + 0.3
    Q = rng.normal(size=(5, 7, 4))
    Q /= np.linalg.norm(Q, axis=2, keepdims=True)
    pose = lambda: np.concatenate([rng.uniform(-0.5, 0.5, (5, 3)), (lambda q: q / np.linalg.norm(q, axis=1, keepdims=True))(  # noqa: E731
        rng.normal(size=(5, 4)))], axis=1)
    return dict(votes=out.to(gpu), logits=logits.to(gpu), offsets=_t(np.array([0, 1200, 1200, 3000], np.int32), gpu),
                segs=np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), cloud=_t(pts, gpu), kab_a=_t(a, gpu), kab_b=_t(b, gpu),
                Q=Q, w=rng.uniform(0.1, 1.0, (5, 7)), M=np.array([7, 1, 3, 7, 5]), add_pts=rng.uniform(-0.1, 0.1, (5, 300, 3)),
                P=np.array([300, 1, 257, 300, 64]), gt=pose(), pr=pose())


def _post_run(i):
    from mrcc_amd import _lib as L
    from mrcc_amd.utils import calibration, metrics
    from mrcc_amd.utils import output as Out
    from mrcc_amd.utils import transformation as T

    votes, logits = i["votes"], i["logits"]
    dev = votes.device
    idx, classes, prob = Out.get_key_point_predictions(logits, conf_th=0.5)
    _arm(i, logits)
    G, C = len(i["segs"]) - 1, logits.shape[1]
    ws = torch.empty(G * C, dtype=torch.int64, device=dev)
    bp = torch.empty((G, C), dtype=torch.float32, device=dev)
    bi = torch.empty((G, C), dtype=torch.int64, device=dev)
    bsel = torch.empty((G, C), dtype=torch.int32, device=dev)
    segs = (c_int64 * (G + 1))(*i["segs"].tolist())
    L.call("sv_key_point_predictions_batched", L.ptr(logits), c_int64(logits.stride(0)), c_int(C), segs, c_int(G), c_float(0.5),
           L.ptr(ws), c_size_t(8 * G * C), L.ptr(bp), L.ptr(bi), L.ptr(bsel), L.stream_ptr())
    _arm(i, i["cloud"])
    root, best = Out.single_linkage_roots(i["cloud"], 0.06)
    _arm(i, i["cloud"])
    largest = Out.ClusterUtil(0.06).get_largest_cluster(i["cloud"])  # roots, then sv_select_equal with the root on the device
    _arm(i, i["kab_a"], i["kab_b"])
    R, t, q = T.get_rigid_transform_3D_batched(i["kab_a"], i["kab_b"], as_tensors=True)
    _arm(i, votes)
    top = Out.topk_indices(votes[:, 1], 8)
    _arm(i, votes, i["offsets"])
    seg = Out.segment_topk_indices(votes[:, 1], i["offsets"], 8)
    _arm(i)  # host arrays in: the wrapper's own upload and launch behind a delay
    qavg = calibration.compute_quaternions_weighted_average_batched(i["Q"], i["w"], i["M"])
    _arm(i)
    add = metrics.compute_ADD_batched(i["add_pts"], i["P"], i["gt"], i["pr"])
    return (top, seg, _host(idx), _host(classes), prob, bp, bi, bsel, root, best, largest, R, t, q, _host(qavg), _host(add))


def _post_ref(i, outs):
    import seg_loss_helpers as SL

    col = i["votes"][:, 1].cpu().numpy()
    assert np.array_equal(outs[0].numpy(), SL.topk_rows(col, 8))
    assert np.array_equal(outs[1].numpy(), SL.segment_topk(col, i["offsets"].cpu().tolist(), 8))
    pts = i["cloud"].cpu().numpy().astype(np.float64)  # single linkage: components of "distance < dist", smallest member as root
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    d = np.linalg.norm(pts[:, None] - pts[None], axis=2)
    assert np.abs(d - 0.06).min() > 1e-6  # a float32 distance decides every pair as this float64 one does
    d = d < 0.06
    lab = connected_components(coo_matrix(d), directed=False)[1]
    first = np.array([np.flatnonzero(lab == c)[0] for c in range(lab.max() + 1)])
    assert np.array_equal(outs[8].numpy(), first[lab].astype(np.int32))
    sizes = np.bincount(lab)
    big = int(np.argmax(sizes == sizes.max()))  # components are numbered by their first member: the lowest one among equals
    assert outs[9].tolist() == [int(first[big]), int(sizes[big])] and np.array_equal(outs[10].numpy(), np.flatnonzero(lab == big))
    assert sizes[big] >= 500


case("post_and_pose", ["sv_topk_indices", "sv_segment_topk", "sv_key_point_predictions", "sv_key_point_predictions_batched",
                       "sv_single_linkage_roots", "sv_select_equal", "sv_kabsch_batched", "sv_quat_avg_batched",
                       "sv_add_metric_batched"],
     _post_build, _post_run, late=("votes", "logits", "offsets", "cloud", "kab_a", "kab_b"), steps=9, reference=_post_ref,
     workspace=lambda i: [_ws("sv_topk_workspace_bytes", 3000, 8), _ws("sv_segment_topk_workspace_bytes", 3000, 3, 8),
                          _ws("sv_cluster_workspace_bytes", 1200)])


# =====================================================================================================================
# ICP, normals, mesh
# =====================================================================================================================
def _icp_build(gpu):
    import icp_batch_helpers as IH

    src, tgt, nrm, init = IH._case(600, 1500, 3)
    bsrc, tgts, nrms, pre, binit, _ = IH.joint_case(600, [1500, 700, 1100], 5)
    return dict(src=_t(src, gpu), tgt=_t(tgt, gpu), nrm=_t(nrm, gpu), init=init, bsrc=_t(bsrc, gpu),
                tgts=[_t(t, gpu) for t in tgts], nrms=[_t(n, gpu) for n in nrms], pre=pre, binit=binit)


def _icp_run(i):
    from mrcc_amd.utils import icp

    def flat(res):
        T, fitness, rmse, updates = res
        return _host(np.concatenate([np.asarray(T).reshape(-1), [fitness, rmse, updates]]))

    p2p = icp.icp_point2point(i["src"], i["tgt"], i["init"], max_distance=0.01, max_iterations=4)
    _arm(i, i["src"], i["tgt"], i["nrm"])
    p2l = icp.icp_point2plane(i["src"], i["tgt"], i["nrm"], i["init"], max_distance=0.01, max_iterations=4)
    _arm(i, i["bsrc"], *i["tgts"], *i["nrms"])
    Tj, sj = icp.icp_joint(i["bsrc"], i["tgts"], i["binit"], i["nrms"], i["pre"], max_distance=0.003, max_iterations=4)
    _arm(i, i["bsrc"], *i["tgts"])
    Tb, sb = icp.icp_batched(i["bsrc"], i["tgts"], np.stack([i["binit"] @ p for p in i["pre"]]), None, None, False, 0.003, 4)
    return flat(p2p), flat(p2l), _host(Tj), _host(sj), _host(Tb), _host(sb)


def _icp_ref(i, outs):
    """the shared-mode call against the float64 loop, with the existing test's preconditions and bounds"""
    import icp_batch_helpers as IH

    n = lambda t: t.cpu().numpy()  # noqa: E731
    tgts, nrms = [n(t) for t in i["tgts"]], [n(t) for t in i["nrms"]]
    ref = IH.icp_joint_ref(n(i["bsrc"]), tgts, nrms, i["pre"], i["binit"], 0.003, 4, 1e-6, 1e-6)
    assert ref["gap"] > 1e-6 and ref["margin"] > 1e-7 and ref["cond"] < 1e6, ref
    T, stats = outs[2].numpy(), outs[3].numpy()
    frames = stats[3:].reshape(3, 2)
    assert stats[2] == ref["updates"] and stats[0] == ref["fitness"] and abs(stats[1] - ref["rmse"]) < 1e-7
    assert np.abs(T - ref["T"]).max() < 1e-9 and np.array_equal(frames[:, 0], ref["frame_fitness"])
    assert np.abs(frames[:, 1] - ref["frame_rmse"]).max() < 1e-7


case("icp", ["sv_icp_point2point", "sv_icp_point2plane", "sv_icp_batched"], _icp_build, _icp_run, late=("src", "tgt", "nrm", "bsrc"), steps=4, reference=_icp_ref,
     workspace=lambda i: [_ws("sv_icp_workspace_bytes", 600), _ws("sv_icp_point2plane_workspace_bytes", 600),
                          _ws("sv_icp_batched_workspace_bytes", 600, 3)])


def _normals_build(gpu):
    rng = np.random.default_rng(12)
    uv = rng.uniform(-0.15, 0.15, (1025, 2))
    surf = np.stack([uv[:, 0], uv[:, 1], 0.02 * np.sin(20 * uv[:, 0]) * np.cos(15 * uv[:, 1])], 1)
    ang, rad = rng.uniform(0, 2 * np.pi, 600), 0.008 * np.sqrt(rng.uniform(0, 1, 600))
    disc = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-2e-4, 2e-4, 600)], 1)  # every point sees all 600
    return dict(surf=_t(surf.astype(np.float32), gpu), disc=_t(disc.astype(np.float32), gpu))


def _normals_run(i):
    from mrcc_amd.utils import icp

    first = icp.estimate_normals(i["surf"], radius=0.02, max_nn=30)
    _arm(i, i["disc"])
    return first + icp.estimate_normals(i["disc"], radius=0.02, max_nn=30)


case("normals", ["sv_estimate_normals"], _normals_build, _normals_run, late=("surf", "disc"), steps=2,
     workspace=lambda i: [_ws("sv_normals_workspace_bytes", 1025, 30), _ws("sv_normals_workspace_bytes", 600, 30)])


MESH_N, MESH_KEEP = 2048, 500


def _mesh_degree():
    from mrcc_amd.utils import mesh

    return mesh.DEFAULT_DEGREE  # the reference's largest neighbour count (55) fits: one sv_sample_eliminate call


def _mesh_build(gpu):
    import mesh_helpers as M

    verts, tris = M.hand_mesh()  # 2048 samples drawn with default_rng(0): the samples mesh_helpers keeps a reference of
    return dict(verts=np.asarray(verts), tris=np.asarray(tris), draws=np.random.default_rng(0).random((MESH_N, 3)), gpu=gpu)


def _mesh_run(i):
    from mrcc_amd.utils import mesh

    m = mesh.TriangleMesh(i["verts"], i["tris"])
    pcl = m.sample_points_uniformly(draws=i["draws"], device=i["gpu"])
    r_max, r_min = mesh.eliminate_radii(pcl.surface_area, MESH_N, MESH_KEEP)
    _arm(i, pcl.points)
    kept, order, degree = mesh.sample_eliminate(pcl.points, MESH_KEEP, r_max, r_min, device=i["gpu"])
    return pcl.points, pcl.normals, pcl.triangle, _host(pcl.surface_area), _host(kept), _host(order), _host(degree)


def _mesh_ref(i, outs):
    import mesh_helpers as M

    points, normals, tri, area = M.hand_samples(MESH_N)
    assert np.array_equal(M.bits(outs[0].numpy()), M.bits(points)) and np.array_equal(M.bits(outs[1].numpy()), M.bits(normals))
    assert np.array_equal(outs[2].numpy(), tri) and float(outs[3]) == area
    kept, order, degree = M.hand_eliminated(MESH_N, MESH_KEEP)
    assert np.array_equal(outs[4].numpy(), kept) and np.array_equal(outs[5].numpy(), order) and int(outs[6]) == degree


case("mesh", ["sv_mesh_sample", "sv_sample_eliminate"], _mesh_build, _mesh_run, reference=_mesh_ref,
     steps=2, workspace=lambda i: [_ws("sv_mesh_sample_workspace_bytes", len(i["tris"])),
                                   _ws("sv_sample_eliminate_workspace_bytes", MESH_N, _mesh_degree())])


# =====================================================================================================================
# ingest and RGB-D
# =====================================================================================================================
def _unpack_build(gpu):
    import ingest_helpers as I
    from mrcc_amd.utils.packed import PackedFrame

    lay = I.LAYOUTS["step19"]
    i = {}
    for n in (513, 70001):
        xyz, _ = I.coordinates(lay, n, "third_nan")
        buf = I.build(lay, xyz, I.colours(n), n, 1)
        i[f"frame{n}"] = PackedFrame.from_pointcloud2(I.Message(buf, lay, n, 1))
        i[f"buf{n}"], i[f"bytes{n}"] = buf, _t(buf, gpu)
    return i


def _unpack_run(i):
    outs = []
    for n in (513, 70001):
        _arm(i, i[f"bytes{n}"])
        points, rgb, src, count = i[f"frame{n}"].unpack(i[f"bytes{n}"])
        k = int(count.item())
        outs += [points[:k], rgb[:k], src[:k], count]
    return tuple(outs)


def _unpack_ref(i, outs):
    import ingest_helpers as I

    for j, n in enumerate((513, 70001)):
        want = I.decode(i[f"buf{n}"], I.LAYOUTS["step19"], n, 1)
        p, rgb, src, count = outs[4 * j:4 * j + 4]
        assert int(count) == want["count"] and np.array_equal(src.numpy(), want["src"])
        assert np.array_equal(p.numpy().view(np.uint32), want["points"].view(np.uint32))
        assert np.array_equal(rgb.numpy(), want["rgb"])


case("unpack_points", ["sv_unpack_points"], _unpack_build, _unpack_run, late=("bytes513", "bytes70001"), reference=_unpack_ref, steps=3,
     workspace=lambda i: [_ws("sv_unpack_points_workspace_bytes", 513), _ws("sv_unpack_points_workspace_bytes", 70001)])


RGBD_H, RGBD_W = 9, 33  # one row and one column past the 8 x 32 filter tile; 297 pixels: two compaction tiles


def _rgbd_frames():
    import rgbd_lens_helpers as RL
    from mrcc_amd.utils.rgbd import RGBDFrame

    rng = np.random.default_rng(14)
    depth = rng.integers(900, 1100, size=(RGBD_H, RGBD_W)).astype(np.uint16)
    depth[rng.uniform(size=depth.shape) < 0.1] = 0
    color = rng.integers(0, 256, size=(RGBD_H, RGBD_W, 3)).astype(np.uint8)
    mask = (rng.uniform(size=(RGBD_H, RGBD_W)) < 0.1)
    K = RL.barrel_K(RGBD_H, RGBD_W, 40.0)
    H = np.eye(4)
    H[:3, 3] = [0.012, -0.004, 0.002]
    common = dict(color_from_depth=H, mask=mask, filter_size=3, filter_thresh=150)
    return (RGBDFrame(depth, color, K, K, **common), RGBDFrame(depth, color, K, K, depth_D=RL.BARREL_D, color_D=RL.BARREL_D, **common))


def _rgbd_build(gpu):
    plain, lens = _rgbd_frames()
    return dict(plain=plain, lens=lens, bytes_plain=_t(plain._bytes(), gpu), bytes_lens=_t(lens._bytes(), gpu))


def _rgbd_run(i):
    from mrcc_amd.utils import rgbd

    rgbd._device_tables.clear()  # the lens tables are built in here (sv_lens_rays), not taken from an earlier run
    outs = []
    dev = i["bytes_lens"].device
    _arm(i)
    tables = [i["lens"].rays_device("depth", dev)]  # sv_lens_rays, waited for: the tables before the clouds' delays
    _arm(i)
    tables.append(i["lens"].rays_device("color", dev))
    for name in ("plain", "lens"):
        f = i[name]
        _arm(i, i[f"bytes_{name}"], *(tables if name == "lens" else []))
        points, rgb, src, count, points64, registered = f.unpack(i[f"bytes_{name}"], want_points64=True, want_registered=True)
        k = int(count.item())
        outs += [points[:k], rgb[:k], src[:k], count, points64[:k], registered]
    return tuple(outs + tables)


def _rgbd_ref(i, outs):
    import rgbd_helpers as RH

    for j, name in enumerate(("plain", "lens")):
        f = i[name]
        p32, rgb, src = f.decode_host(color="bytes")
        p64, _ = f.decode_host64()
        got = [t.numpy() for t in outs[6 * j:6 * j + 6]]
        assert int(got[3][0]) == len(src) and len(src) > 50 and np.array_equal(got[2], src.astype(np.int32)), name
        assert RH.same_bits(got[0], p32) and RH.same_bits(got[4], p64) and RH.same_bits(got[1], rgb.astype(np.float32)), name
        assert RH.same_bits(got[5], f.registered_host()), name


case("rgbd", ["sv_rgbd_cloud", "sv_lens_rays", "sv_rgbd_cloud_lens"], _rgbd_build, _rgbd_run, late=("bytes_plain", "bytes_lens"), steps=5,
     reference=_rgbd_ref, workspace=lambda i: [_ws("sv_rgbd_cloud_workspace_bytes", RGBD_H, RGBD_W, RGBD_H, RGBD_W)])


# =====================================================================================================================
# augmentation, labels, losses (B = 3, the middle frame empty)
# =====================================================================================================================
def _augment_build(gpu):
    from mrcc_amd.utils import augmentation as A

    rng = np.random.default_rng(15)
    lens = [700, 0, 450]
    N = sum(lens)
    pts = rng.uniform(-100, 100, (N, 3))
    off = np.concatenate([[0], np.cumsum(lens)])
    abs_max = np.stack([np.abs(pts[off[b]:off[b + 1]]).max(0) if lens[b] else np.ones(3) for b in range(3)])
    draws = A.draw_augmentations(abs_max, scale=200, probability=1.0, elastic=True, noise=True, transform=True, flip=True, gravity=True,
                                 rng=rng)
    table, raw, dims = A._table_and_fields(draws)
    normals = rng.standard_normal((N, 3))
    return dict(points=_t(pts, gpu), offsets=_t(off.astype(np.int32), gpu), table=_t(table, gpu), normals=_t(normals, gpu),
                raw=raw, dims=dims, N=N, draws=draws, host=(pts, off, normals))


def _augment_run(i):
    from mrcc_amd import _lib
    from mrcc_amd.utils import augmentation as A

    fields = A.elastic_fields(i["raw"], i["dims"], i["points"].device)
    _arm(i, i["points"], i["offsets"], i["normals"], fields, i["table"], fills=[None, None, None, None, 0])
    out, stats = A.augment_points(i["points"], i["offsets"], i["table"], fields, i["normals"])
    _arm(i, out, i["offsets"], stats)
    coords, shifted, shift = A.quantise_points(out, i["offsets"], stats, _lib.SV_ORIGIN_CENTER, 0.5)
    return fields, out, stats, coords, shifted, shift  # the empty frame's stats are (+inf, -inf), its shift their mean


def _augment_ws(i):
    dims = np.ascontiguousarray(i["dims"], dtype=np.int32)
    return [_ws("sv_elastic_field_workspace_bytes", dims.ctypes.data_as(ctypes.c_void_p), len(dims)),
            _ws("sv_augment_points_workspace_bytes", i["N"], 3)]


def _augment_ref(i, outs):
    """frame by frame against augment_helpers.apply_draws with the existing test's bound, quantise_np exactly"""
    import augment_helpers as AH

    pts, off, normals = i["host"]
    out, stats = outs[1].numpy(), outs[2].numpy()
    for b, d in enumerate(i["draws"]):
        lo, hi = off[b], off[b + 1]
        if hi == lo:
            assert np.array_equal(stats[b], [np.inf] * 3 + [-np.inf] * 3)
            continue
        x = pts[lo:hi]
        dd = dict(elastic=[(st.raw, st.gran, st.mag) for st in d.elastic], normals=normals[lo:hi] if d.noise else None, sigma=d.sigma,
                  clip=d.clip, transform=d.transform, flip=d.flip, gravity=d.gravity)
        term = min(st.mag * float(np.abs(np.stack(AH.blur_field(st.raw))).max()) for st in d.elastic)
        want = AH.apply_draws(x, dd)
        assert np.abs(out[lo:hi] - want).max() <= 1e-9 * (float(np.abs(x).max()) + term), b
        assert np.array_equal(stats[b], np.concatenate([out[lo:hi].min(0), out[lo:hi].max(0)])), b
    want_c, want_f, want_s = AH.quantise_np(out, off, stats, AH.ORIGIN_CENTER, 0.5)
    assert np.array_equal(outs[3].numpy(), want_c) and np.array_equal(outs[4].numpy().view(np.int32), want_f.view(np.int32))
    assert np.array_equal(outs[5].numpy(), want_s, equal_nan=True)


# the table's elastic rows hold offsets into `fields` and grid sizes as doubles: its poison is all zeros (every stage off)
case("augment", ["sv_elastic_field", "sv_augment_points", "sv_quantise_points"], _augment_build, _augment_run,
     late=("points", "offsets", "table", "normals"), poison={"table": 0}, workspace=_augment_ws, reference=_augment_ref, steps=3)


def _labels_build(gpu):
    import label_helpers as LH
    from mrcc_amd.utils import data as D

    rng = np.random.default_rng(42)
    a, pose_a, _ = LH.gripper_cloud(rng, 600, n_rod=50, n_bg=375)
    c, pose_c, _ = LH.gripper_cloud(rng, 300)
    poses = np.stack([pose_a, pose_a, pose_c])
    pos, rot = D.pose_tables(poses, gpu)
    return dict(points=_t(np.concatenate([a, c]), gpu), offsets=_t(np.array([0, len(a), len(a), len(a) + len(c)], np.int32), gpu),
                pos=pos, rot=rot, N=len(a) + len(c), frames=[a, a[:0], c], poses=poses)


def _labels_run(i):
    from mrcc_amd.utils import data as D

    p, off, pos, rot = i["points"], i["offsets"], i["pos"], i["rot"]
    outs = [D.ee_mask(p, off, pos, rot)]
    for mode in (10, 6):
        _arm(i, p, off, pos, rot)
        kp, idx, empty = D.key_points(p, off, pos, rot, mode)
        _arm(i, p, off, idx)
        outs += [kp, idx, empty, D.radius_labels(p, off, idx)]
    lp1, lp2 = D.CROSS_SECTION_LINE
    _arm(i, p, off, pos, rot)
    return tuple(outs) + D.line_topk(p, off, pos, rot, lp2, lp1, 32, 0.004)


def _labels_ref(i, outs):
    """the frames with rows against tests/label_helpers.py, as tests/test_gpu_labels.py holds the batched calls"""
    import label_helpers as LH

    o = [t.numpy() for t in outs]
    off = i["offsets"].cpu().numpy()
    for b, (f, pose) in enumerate(zip(i["frames"], i["poses"])):
        if not len(f):
            continue
        rows = slice(off[b], off[b + 1])
        assert np.array_equal(o[0][rows].astype(bool), LH.ee_mask(f, pose)), b
        kp10, idx10 = LH.key_points(f, pose)
        kp6, idx6, empty = LH.six_key_points(f, pose)
        for at, kp, idx in ((1, kp10, idx10), (5, kp6, idx6)):
            assert np.array_equal(o[at + 1][b], idx) and np.abs(o[at][b] - kp).max() <= 1e-12, (b, at)
            assert np.array_equal(o[at + 3][rows], LH.radius_labels(f, idx)), (b, at)
        dist, cs = LH.cross_section(f, pose, 32, 0.004)
        k = int(o[11][b])
        assert k == len(cs) and np.array_equal(o[9][b, :k], cs) and (o[9][b, k:] == -1).all() and np.isinf(o[10][b, k:]).all()
        assert k == 0 or np.abs(o[10][b, :k] - dist).max() <= 1e-7


case("labels", ["sv_ee_mask", "sv_key_points", "sv_radius_labels", "sv_line_topk"], _labels_build, _labels_run,
     late=("points", "offsets", "pos", "rot"), workspace=lambda i: [_ws("sv_line_topk_workspace_bytes", i["N"])],
     reference=_labels_ref, steps=6)


def _loss_build(gpu):
    import loss_helpers as LS

    rng = np.random.default_rng(16)
    lens = [700, 0, 300]
    rows = np.concatenate([LS.shell_voxels(1, 700), LS.shell_voxels(2, 300)]).astype(np.float32)
    M = len(rows)
    rot = lambda: torch.from_numpy(np.stack([LS.quat_matrix_np(rng.normal(size=4)) for _ in range(3)]).astype(np.float32)).to(gpu)  # noqa: E731
    g = torch.Generator().manual_seed(17)
    N, C = 1000, 5
    labels = torch.randint(0, C, (N,), generator=g)
    labels[torch.rand(N, generator=g) < 0.1] = -100
    return dict(rows=_t(rows, gpu), offsets=_t(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), gpu),
                weights=_t(rng.uniform(0.5, 1.5, M).astype(np.float32), gpu), mask=_t((rng.uniform(size=M) < 0.8).astype(np.uint8), gpu),
                R=rot(), R_pred=rot(), t=_t(rng.normal(size=(3, 3)).astype(np.float32), gpu),
                t_pred=_t(rng.normal(size=(3, 3)).astype(np.float32), gpu), logits=(torch.randn(N, C, generator=g) * 2).to(gpu),
                labels=labels.to(gpu), seg_offsets=_t(np.array([0, 600, 600, 1000], np.int32), gpu), M=M)


def _loss_run(i):
    from mrcc_amd import _lib
    from mrcc_amd.utils import loss as Lo

    outs = []
    for mode, kp in ((_lib.SV_LOSS_SHAPE_MATCH, False), (_lib.SV_LOSS_KP_POSE_MATCH, True), (_lib.SV_LOSS_POSE_MATCH, False)):
        with_t = mode != _lib.SV_LOSS_SHAPE_MATCH
        Rp = i["R_pred"].detach().clone().requires_grad_(True)
        tp = i["t_pred"].detach().clone().requires_grad_(True) if with_t else None
        _arm(i, i["rows"], i["offsets"], i["weights"], i["mask"], i["R"], i["t"], Rp.detach(), tp.detach() if with_t else None)
        loss = Lo.PoseMatchLossFunction.apply(Rp, tp, i["R"], i["t"] if with_t else None, i["rows"], i["offsets"],
                                              i["weights"] if kp else None, i["mask"] if kp else None, mode)
        live = torch.tensor([0, 2], device=loss.device)  # the empty instance's loss is 0 / 0
        loss[live].sum().backward()
        outs += [loss, Rp.grad] + ([tp.grad] if with_t else [])
    _arm(i, i["logits"], i["labels"], i["seg_offsets"])
    sums, grad, m = Lo.seg_criterion_call(i["logits"], i["labels"], i["seg_offsets"])
    return tuple(outs) + (sums, grad, m.confusion, m.rows, m.ignored, m.invalid)


def _loss_ref(i, outs):
    import seg_loss_helpers as SL

    cm, ign = SL.confusion(i["logits"].cpu().numpy(), i["labels"].cpu().numpy(), i["seg_offsets"].cpu().tolist())
    assert np.array_equal(outs[10].numpy(), cm) and np.array_equal(outs[12].numpy(), ign) and int(outs[13]) == 0
    assert outs[11].tolist() == [600, 0, 400]
    import loss_helpers as LS

    n = lambda k: i[k].cpu().numpy().astype(np.float64)  # noqa: E731
    off, live = i["offsets"].cpu().numpy(), np.array([True, False, True])
    at = 0
    for mode, kw in ((LS.SHAPE_MATCH, {}), (LS.KP_POSE_MATCH, dict(t=n("t"), t_pred=n("t_pred"), w=n("weights"), mask=n("mask"))),
                     (LS.POSE_MATCH, dict(t=n("t"), t_pred=n("t_pred")))):
        want = LS.batch_loss_np(mode, n("rows"), off, n("R").reshape(3, 3, 3), n("R_pred").reshape(3, 3, 3), **kw)
        got = outs[at:at + (3 if kw else 2)]
        for g, w in zip(got, want):  # loss, d loss / d R_pred, d loss / d t_pred: 1e-6 of the tensor's largest value
            g = g.double().numpy()
            assert np.isnan(g[~live]).all() and LS.rel_err(g[live], w[live]) <= 1e-6, (mode, LS.rel_err(g[live], w[live]))
        at += len(got)


case("losses", ["sv_pose_match_loss", "sv_seg_criterion"], _loss_build, _loss_run, reference=_loss_ref,
     late=("rows", "offsets", "weights", "mask", "R", "R_pred", "t", "t_pred", "logits", "labels", "seg_offsets"), steps=5,
     workspace=lambda i: [_ws("sv_pose_loss_workspace_bytes", i["M"], 3), _ws("sv_seg_criterion_workspace_bytes", 1000, 3, 5)])


# =====================================================================================================================
# PointNet++ (B = 2, N = 300, S = 65)
# =====================================================================================================================
PN_B, PN_N, PN_S, PN_D = 2, 300, 65, 6


def _pn_build(gpu):
    from mrcc_amd.model import pointnet2_utils as P2

    g = torch.Generator().manual_seed(18)
    B, N, S, D = PN_B, PN_N, PN_S, PN_D
    torch.manual_seed(19)
    sa = P2.PointNetSetAbstraction(S, 0.2, 32, D + 3, [32, 32, 64], False)
    msg = P2.PointNetSetAbstractionMsg(S, [0.1, 0.2, 0.4], [16, 32, 128], D, [[32, 32, 64], [64, 64, 128], [64, 96, 128]])
    for m in (sa, msg):
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
    sizes = [300, 0, 1, 257]
    return dict(xyz=torch.rand(B, N, 3, generator=g).to(gpu), feats=torch.randn(B, N, D, generator=g).to(gpu),
                start=torch.randint(0, N, (B,), generator=g).to(gpu), p2=torch.randn(B, S, 16, generator=g).to(gpu),
                dout=torch.randn(B, N, 16, generator=g).to(gpu), drows=torch.randn(B * S * 32, 3 + D, generator=g).to(gpu),
                rows=torch.randn(B * S * 32, 64, generator=g).to(gpu), dpool=torch.randn(B * S, 64, generator=g).to(gpu),
                seg_xyz=torch.rand(sum(sizes), 3, generator=g).to(gpu), seg_off=_t(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), gpu),
                seg_out=_t(np.arange(len(sizes) + 1, dtype=np.int64) * 16, gpu), seg_start=_t(np.array([299, 0, 0, 100], np.int64), gpu),
                sa=sa.to(gpu).eval(), msg=msg.to(gpu).eval(), G=len(sizes))


def _pn_run(i):
    from mrcc_amd import _lib as L
    from mrcc_amd.model import pointnet2_utils as P2

    xyz, feats = i["xyz"], i["feats"]
    B, N, S = PN_B, PN_N, PN_S
    fps = P2.farthest_point_sample(xyz, S, start=i["start"])
    new_xyz = P2.index_points(xyz, fps)
    _arm(i, i["seg_xyz"], i["seg_off"], i["seg_out"], i["seg_start"])
    seg = torch.empty(i["G"] * 16, dtype=torch.int64, device=xyz.device)
    L.call("sv_fps_segmented", L.ptr(i["seg_xyz"]), L.ptr(i["seg_off"]), L.ptr(i["seg_out"]), L.ptr(i["seg_start"]), c_int(i["G"]),
           c_int(300), L.ptr(seg), L.stream_ptr())
    _arm(i, xyz, new_xyz)
    bq = P2.query_ball_point(0.2, 32, xyz, new_xyz)
    _arm(i, xyz, new_xyz)
    multi = P2.query_ball_point_multi([0.1, 0.2, 0.4], [16, 32, 128], xyz, new_xyz)
    _arm(i, xyz, new_xyz)
    idx3, w3 = P2.three_nn(xyz, new_xyz)
    p2 = i["p2"].detach().clone().requires_grad_(True)
    _arm(i, i["p2"], idx3, w3)
    gathered = P2.three_nn_gather(p2, idx3, w3)
    _arm(i, i["dout"])  # the backward reads idx3 and w3 as saved tensors: only its incoming gradient can be late
    gathered.backward(i["dout"])
    _arm(i, xyz, new_xyz, i["p2"])
    interp = P2.three_nn_interpolate(xyz, new_xyz, i["p2"])
    pts = feats.detach().clone().requires_grad_(True)
    _arm(i, xyz, new_xyz, bq)
    rows = P2.group_rows(xyz, pts, new_xyz, bq, L.SV_GROUP_SSG)
    _arm(i, i["drows"])
    rows.backward(i["drows"])
    _arm(i, i["rows"])
    r = i["rows"].detach().clone().requires_grad_(True)
    pooled = P2.group_max(r, 32)
    _arm(i, i["dpool"])
    pooled.backward(i["dpool"])
    outs = [fps, seg, bq, *multi, idx3, w3, gathered.detach(), p2.grad,
            interp, rows.detach(), pts.grad, pooled.detach(), r.grad]
    with torch.no_grad():
        for m in (i["sa"], i["msg"]):
            m._folds_drop()  # the folded weights are built in here: their host arithmetic reads the parameters back
            m._folded()
            _arm(i, xyz, feats, i["start"])
            outs += list(m(xyz.permute(0, 2, 1), feats.permute(0, 2, 1), fps_start=i["start"]))
    return tuple(outs)


def _pn_ref(i, outs):
    import pointnet_grad_helpers as PG

    n = lambda k: i[k].cpu().numpy()  # noqa: E731
    fps, bq = outs[0].numpy(), outs[2].numpy()
    new_xyz = np.take_along_axis(n("xyz"), fps[:, :, None], axis=1)
    D = PN_D
    assert PG.same_bits(outs[11].numpy(), PG.group_rows_ref(n("xyz"), n("feats"), new_xyz, bq, PG.SSG, 3 + D))
    csr = PG.index_transpose_ref(bq, PN_N)
    dp = PG.gather_transpose_ref(*csr, None, n("drows"), 3, D, 1)
    assert PG.same_bits(outs[12].numpy().reshape(-1, D), dp)
    pooled, arg = PG.group_max_ref(n("rows"), 32)
    assert PG.same_bits(outs[13].numpy(), pooled) and PG.same_bits(outs[14].numpy(), PG.group_max_backward_ref(n("dpool"), arg, 32))
    assert PG.same_bits(outs[8].numpy(), outs[10].numpy())  # sv_three_nn + sv_three_nn_gather: sv_three_nn_interpolate's bits


case("pointnet2", ["sv_fps", "sv_fps_segmented", "sv_ball_query", "sv_ball_query_multi", "sv_three_nn", "sv_three_nn_gather",
                   "sv_three_nn_interpolate", "sv_pointnet_sa", "sv_pointnet_sa_msg", "sv_group_rows", "sv_index_transpose",
                   "sv_gather_transpose", "sv_group_max", "sv_group_max_backward"],
     _pn_build, _pn_run, reference=_pn_ref, steps=14,
     late=("xyz", "feats", "start", "p2", "dout", "drows", "rows", "dpool", "seg_xyz", "seg_off", "seg_out", "seg_start"),
     workspace=lambda i: [_ws("sv_index_transpose_workspace_bytes", PN_B, PN_S * 32, PN_N),
                          _ws("sv_index_transpose_workspace_bytes", PN_B, PN_N * 3, PN_S)])


# =====================================================================================================================
# whole networks: the Python layer's own caches and intermediate buffers (no new entry points)
# =====================================================================================================================
def _randomise_bn(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in net.modules():
            if isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                mod.weight.copy_(torch.rand(mod.num_features, generator=g) * 0.5 + 0.75)
                mod.bias.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
                mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)


def _unet_build(train):
    def build(gpu):
        import conv_exact_helpers as H
        from mrcc_amd.model.backbone.minkunet import MinkUNet14A
        from mrcc_amd.model.robotnet_segmentation import _classification_head

        torch.manual_seed(21)
        model = _classification_head(MinkUNet14A, lambda: 3, "SegHead14A")(3, num_classes=3)
        _randomise_bn(model, 22)
        clouds = [H.int_cloud(1, 700), H.int_cloud(2, 400)]
        coords = np.concatenate([np.concatenate([np.full((len(c), 1), b), c], 1) for b, c in enumerate(clouds)])
        g = torch.Generator().manual_seed(23)
        return dict(model=model.to(gpu).train(train), coords=_t(coords, gpu, torch.int32), feats=(torch.rand(len(coords), 3, generator=g) - 0.5).to(gpu),
                    gw=torch.randn(len(coords), 3, generator=g).to(gpu))

    return build


def _unet_eval_run(i):
    from mrcc_amd import MinkowskiEngine as ME

    with torch.no_grad():
        x = ME.SparseTensor(i["feats"], coordinates=i["coords"], device=i["feats"].device)
        out = i["model"](x)
    return out.F, out.C


def _unet_train_run(i):
    from mrcc_amd import MinkowskiEngine as ME

    model = copy.deepcopy(i["model"])  # the step changes the parameters: every run starts from the same ones
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    x = ME.SparseTensor(i["feats"], coordinates=i["coords"], device=i["feats"].device)
    out = model(x)
    assert out.F.shape == i["gw"].shape  # the input rows are distinct voxels
    (out.F * i["gw"]).sum().backward()
    grads = [p.grad.detach().clone() for p in model.parameters()]
    opt.step()
    return (out.F.detach(), *grads, *[p.detach() for p in model.parameters()], *[b.detach() for b in model.buffers()])


case("unet_eval", [], _unet_build(False), _unet_eval_run, late=("coords", "feats"), network=True)
case("unet_train_step", [], _unet_build(True), _unet_train_run, late=("coords", "feats", "gw"), network=True)


def _msg_build(gpu):
    from mrcc_amd.model import pointnet2 as P
    from mrcc_amd.model import pointnet2_utils as U

    torch.manual_seed(24)
    m = P.PointNet2MSGEncoder(7)
    m.drop1.p = m.drop2.p = 0.0
    U.set_training_path(m, "hip")
    g = torch.Generator().manual_seed(25)
    B, N = 2, 256
    x = torch.cat([torch.rand(B, 3, N, generator=g), torch.nn.functional.normalize(torch.randn(B, 3, N, generator=g), dim=1)], 1)
    return dict(model=m.to(gpu).train(), x=x.to(gpu), y=torch.randn(B, 7, generator=g).to(gpu),
                fps=torch.randint(0, 128, (2, B), generator=g).to(gpu))


def _msg_run(i):
    model = copy.deepcopy(i["model"])  # train(): the BatchNorm statistics move
    out, l3 = model(i["x"], fps_starts=i["fps"])
    torch.nn.functional.mse_loss(out, i["y"]).backward()
    return (out.detach(), l3.detach(), *[p.grad.detach().clone() for p in model.parameters()])


case("pointnet2_msg_train", [], _msg_build, _msg_run, late=("x", "y", "fps"), network=True)


def _engine_build(gpu):
    import mrcc_amd
    from mrcc_amd.app.inference_engine import InferenceEngine
    from mrcc_amd.utils import preprocess
    from mrcc_amd.utils.config import Config

    Config.reset()
    Config().update({"INFERENCE": {"SEGMENTATION": {"scale": 50}}})
    eng = InferenceEngine(allow_random_init=True, seed=3)
    mrcc_amd.synth.wire_color_keyed_labels(eng._segmentation_model)
    frames = []
    for s in range(3):
        sc = mrcc_amd.synth.gen_scene(s, n_bg=2500 + 300 * s, n_arm=400, n_ee=600, keyed_colors=True)
        frames.append((sc["points"], preprocess.normalize_colors(sc["rgb"])))
    return dict(engine=eng, frames=frames)


def _engine_run(i):
    return tuple(_host(lab) for lab in i["engine"].predict_segmentation_stream(iter(i["frames"]), compute_streams=2, group=2))


def _engine_cleanup(i):
    from mrcc_amd.utils.config import Config

    Config.reset()


case("engine_stream", [], _engine_build, _engine_run, network=True, cleanup=_engine_cleanup)
