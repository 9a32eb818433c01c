"""Which kernel instance, in which form, a public fp32 sparse-convolution call runs on - asked of the library itself - and
the table of cases that pins every reachable one (tests/test_conv_instances_cpu.py: completeness,
tests/test_gpu_conv_instances.py: bit-exactness against the oracle).

The rules live in csrc/sv_conv_select.h and nowhere else; sv_conv_select / sv_conv_tile_info answer on the host, so
everything here works without a GPU.
"""
from collections import namedtuple

import numpy as np

from mrcc_amd import _lib

PLAN_TILE = _lib.SV_TILE_ROWS
WANT_SCALE_DEFAULT = 0.3   # SV_CONV_WANT_SCALE_DEFAULT
TAIL_DEFAULT = 0.15        # SV_CONV_TAIL_DEFAULT

TileCfg = namedtuple("TileCfg", "MR TN GK KC PFD USE_FULL")
_TILES = {row[:4]: TileCfg(*row[4:9], bool(row[9])) for row in _lib.conv_tiles()}
# the instantiations of the tiled kernel, (TM, WAVES_N, NT, CPO): the rows of the library's tile table
INSTANTIATED = list(_TILES)


def tile_cfg(tm, wn, nt, cpo=0):
    """the per-tile constants of ConvCfg that decide a launch's form"""
    return _TILES[(tm, wn, nt, cpo)]


def _flags(has_plan, vec_a, buf_ok, acc_init, w_aligned=True):
    return ((_lib.SV_CONV_SEL_PLAN | _lib.SV_CONV_SEL_TILE_ORDER if has_plan else 0) | (_lib.SV_CONV_SEL_VEC_A if vec_a else 0) |
            (_lib.SV_CONV_SEL_BUF_OK if buf_ok else 0) | (_lib.SV_CONV_SEL_ACC_INIT if acc_init else 0) |
            (_lib.SV_CONV_SEL_W_ALIGNED if w_aligned else 0))


def _key(raw):
    return key(*_lib._parse_instance(raw))


def dispatch_key(K, Cin, Cout, Vpad, has_plan, vec_a, buf_ok, acc_init, want_scale=WANT_SCALE_DEFAULT,
                 tail_fraction=TAIL_DEFAULT, w_aligned=True):
    """(name, fast, ring, full) of sv_conv_last_instance() after the call.  vec_a: the input view allows float4 gathers
    (Cin and its row stride multiples of 4, 16-byte aligned start); buf_ok: every operand inside the 2 GB buffer extent
    and `perm` 16-byte aligned; want_scale >= 1 stands for conv_dispatch(1.0) - one frame alone on the GPU, which also
    moves the thin layers onto the LDS-weights kernel (w_aligned: the weight pointer is 16-byte aligned).  A plan comes
    with its tile order, as every plan nn.conv_forward passes does."""
    return _key(_lib.conv_instance(K, Cin, Cout, Vpad, _flags(has_plan, vec_a, buf_ok, acc_init, w_aligned), want_scale, tail_fraction))


def dispatch(*args, **kw):
    """the pair _lib.conv_last_instance() returns: (name, {"fast", "ring", "full"})"""
    name, fast, ring, full = dispatch_key(*args, **kw)
    return name, {"fast": fast, "ring": ring, "full": full}


def key(name, flags):
    return (name, flags["fast"], flags["ring"], flags["full"])


# ---- the sweep the completeness test runs --------------------------------------------------------------------------
SWEEP_SCALES = (WANT_SCALE_DEFAULT, 1.0)
SWEEP_K = (1, 8, 27)
# 3; not a multiple of 4 (7); a multiple of 4 but not of 32 (20); 32; 64; a multiple of 128; 416 = 3 * 128 + 32
SWEEP_CIN = (3, 7, 20, 32, 64, 128, 416)
# every candidate list of csrc/sv_conv_select.h, Cout % TN == 0 and not: at most 16 outputs (5, 16), at most 32 (20, 32), at
# most 64 (48, 64), the 128-column tiles (80; 128: a multiple of 64), the 192-column tiles (192, 288; 384: a multiple of
# 128), beyond 2048 (2052: the only kind of width the 192-column lists take that leaves <32, 2, 3> a partial column tile,
# 2176: the same for a multiple of 128), and the widths the narrow kernel takes (1, 3, 4)
SWEEP_COUT = (1, 3, 4, 5, 16, 20, 32, 48, 64, 80, 128, 192, 288, 384, 2052, 2176)
# every padded row count up to 136k: the last new combination appears at 131200 rows (more than 1024 workgroups of a 128-row
# tile), none between there and 300k
SWEEP_VPAD = tuple(range(128, 136 * 1024 + 1, 128))


def sweep():
    """{(name, fast, ring, full)} of every combination the public call reaches, each with the first shape that reaches it.
    K > 1 always comes with a plan.  K = 1 is swept WITHOUT one (dense rows: kernel_size 1 stride 1, Linear) and WITH one (the
    kernel_size 1 strided maps of plan_strided / plan_strided_t, tests/test_gpu_conv_strided.py).  vec_a is swept over both
    values where Cin allows it (a view whose row stride or start is not 16-byte aligned); buf_ok = False only with a plan (a
    `perm` off a 16-byte boundary; without a plan it takes a tensor beyond 2 GB, which sv_conv_fwd_acc splits into row ranges
    that fit).  One library call per (scale, K, plan, Cin, vec_a, Cout, buf_ok, acc_init) answers all its row counts."""
    seen = {}
    shapes = np.zeros((len(SWEEP_VPAD), 5), np.int64)
    shapes[:, 3] = SWEEP_VPAD
    for ws in SWEEP_SCALES:
        for K, has_plan in [(K, K > 1) for K in SWEEP_K] + [(1, True)]:
            for Cin in SWEEP_CIN:
                for vec_a in ((True, False) if Cin % 4 == 0 else (False,)):
                    for Cout in SWEEP_COUT:
                        for buf_ok in ((True, False) if has_plan else (True,)):
                            for acc_init in (False, True):
                                shapes[:, (0, 1, 2, 4)] = (K, Cin, Cout, _flags(has_plan, vec_a, buf_ok, acc_init))
                                raw = np.zeros(len(shapes), "S128")
                                _lib.call("sv_conv_select", len(shapes), shapes.ctypes.data, ws, TAIL_DEFAULT, raw.ctypes.data, 128)
                                names, first = np.unique(raw, return_index=True)
                                for i in np.argsort(first):
                                    seen.setdefault(_key(names[i].decode()), (K, Cin, Cout, SWEEP_VPAD[first[i]], has_plan, vec_a,
                                                                              buf_ok, acc_init, ws))
    return seen


# ---- the case table ------------------------------------------------------------------------------------------------
# kind: "dense" (K = 1, no plan), "up" (K = 8, the transposed stride-2 map onto the V-voxel map: one neighbour per row,
#       so the oracle costs what a dense layer costs) or "k3" (K = 27, the 3x3x3 map of the V-voxel blob);
# V: output rows; every V is 61 short of a multiple of 128, so the last plan tile holds 67 rows - its second 64-row tile
#    three live rows and three wholly dead 16-row sub-tiles;
# scale: None = the library's default dispatch, 1.0 = under conv_dispatch(1.0);
# reason: why a guarded (fast = 0) form is entered - "odd_cin" (Cin % 4 != 0), "cout_tail" (Cout % TN != 0, aligned vector
#         input) or "perm_misaligned" (a `perm` 4 bytes off a 16-byte boundary, everything else FAST-eligible); None on
#         FAST rows; on conv_first_layer_kernel what keeps the layer off the matrix-pipe kernel;
# split: None, or the split point of a two-pass SplitPlan - the row then pins the SECOND pass, which continues the first
#        one's accumulators (acc_init) over the last 27 - split offsets;
# name, fast, ring, full: what sv_conv_last_instance() must report, as literals.
Case = namedtuple("Case", "kind K Cin Cout V scale reason split name fast ring full")


def _rows(name, *rows):
    return [Case(*r[:8], name, *r[8:]) for r in rows]


CASES = (
    *_rows("conv_first_layer_kernel<3, 32>",
           ("k3", 27, 3, 32, 67, None, "perm_misaligned", None, 0, 0, 0)),
    *_rows("conv_first_mfma_kernel<3, 32>",
           ("up", 8, 3, 32, 67, None, None, None, 1, 0, 1)),
    *_rows("conv_fwd_dual_kernel<64, 32, 4, 3>",
           ("up", 8, 148, 384, 24003, None, None, None, 1, 0, 0)),
    *_rows("conv_fwd_kernel<128, 1, 1>",
           ("dense", 1, 148, 5, 22979, None, "cout_tail", None, 0, 1, 0),
           ("dense", 1, 131, 16, 22979, None, "odd_cin", None, 0, 1, 0),
           ("k3", 27, 36, 16, 22979, None, "perm_misaligned", None, 0, 1, 0),
           ("dense", 1, 148, 16, 22979, None, None, None, 1, 1, 0),
           ("dense", 1, 131, 16, 131139, None, "odd_cin", None, 0, 0, 0),
           ("dense", 1, 148, 16, 131139, None, None, None, 1, 0, 0)),
    *_rows("conv_fwd_kernel<128, 2, 1>",
           ("dense", 1, 148, 20, 57539, None, "cout_tail", None, 0, 1, 0),
           ("dense", 1, 131, 32, 57539, None, "odd_cin", None, 0, 1, 0),
           ("k3", 27, 4, 32, 57539, None, "perm_misaligned", None, 0, 1, 0),
           ("dense", 1, 148, 32, 57539, None, None, None, 1, 1, 0),
           ("dense", 1, 131, 32, 131139, None, "odd_cin", None, 0, 0, 0),
           ("dense", 1, 148, 32, 131139, None, None, None, 1, 0, 0)),
    *_rows("conv_fwd_kernel<128, 4, 2>",
           ("dense", 1, 148, 160, 24899, None, "cout_tail", None, 0, 0, 0),
           ("dense", 1, 131, 128, 49859, None, "odd_cin", None, 0, 0, 0),
           ("up", 8, 148, 128, 49859, None, "perm_misaligned", None, 0, 0, 0),
           ("dense", 1, 148, 128, 49859, None, None, None, 1, 0, 0)),
    *_rows("conv_fwd_kernel<16, 4, 1, fused 32>",
           ("k3", 27, 32, 64, 16451, 1.0, "perm_misaligned", None, 0, 0, 0),
           ("k3", 27, 32, 64, 67, None, "perm_misaligned", None, 0, 1, 0),
           ("k3", 27, 32, 64, 16451, 1.0, None, None, 1, 0, 0), ("up", 8, 32, 64, 16451, 1.0, None, None, 1, 0, 1),
           ("k3", 27, 32, 64, 67, None, None, None, 1, 1, 0), ("up", 8, 32, 64, 67, None, None, None, 1, 1, 1)),
    *_rows("conv_fwd_kernel<16, 4, 1, fused 64>",
           ("k3", 27, 64, 128, 8259, 1.0, "perm_misaligned", None, 0, 0, 0),
           ("k3", 27, 64, 64, 67, None, "perm_misaligned", None, 0, 1, 0),
           ("k3", 27, 64, 128, 8259, 1.0, None, None, 1, 0, 0), ("up", 8, 64, 128, 8259, 1.0, None, None, 1, 0, 1),
           ("k3", 27, 64, 64, 67, None, None, None, 1, 1, 0), ("up", 8, 64, 64, 67, None, None, None, 1, 1, 1)),
    *_rows("conv_fwd_kernel<16, 4, 1>",
           ("dense", 1, 148, 48, 16451, 1.0, "cout_tail", None, 0, 0, 0),
           ("dense", 1, 131, 128, 8259, None, "odd_cin", None, 0, 0, 0),
           ("k3", 27, 32, 128, 8259, None, "perm_misaligned", None, 0, 0, 0),
           ("dense", 1, 148, 48, 67, None, "cout_tail", None, 0, 1, 0),
           ("dense", 1, 131, 64, 67, None, "odd_cin", None, 0, 1, 0),
           ("k3", 27, 148, 64, 67, None, "perm_misaligned", None, 0, 1, 0),
           ("dense", 1, 148, 128, 8259, None, None, None, 1, 0, 0),
           ("dense", 1, 256, 128, 8259, None, None, None, 1, 0, 1), ("dense", 1, 148, 64, 67, None, None, None, 1, 1, 0),
           ("dense", 1, 256, 64, 67, None, None, None, 1, 1, 1)),
    *_rows("conv_fwd_kernel<16, 4, 3>",
           ("dense", 1, 148, 2176, 1347, 1.0, "cout_tail", None, 0, 0, 0),
           ("dense", 1, 131, 384, 8259, 1.0, "odd_cin", None, 0, 0, 0),
           ("k3", 27, 4, 384, 8259, 1.0, "perm_misaligned", None, 0, 0, 0),
           ("dense", 1, 148, 2176, 67, None, "cout_tail", None, 0, 1, 0),
           ("dense", 1, 131, 384, 67, None, "odd_cin", None, 0, 1, 0),
           ("k3", 27, 148, 384, 67, None, "perm_misaligned", None, 0, 1, 0),
           ("dense", 1, 148, 384, 8259, 1.0, None, None, 1, 0, 0), ("dense", 1, 256, 384, 8259, 1.0, None, None, 1, 0, 1),
           ("dense", 1, 148, 384, 67, None, None, None, 1, 1, 0), ("dense", 1, 256, 384, 67, None, None, None, 1, 1, 1),
           ("up", 8, 256, 384, 67, None, None, None, 1, 1, 1)),
    *_rows("conv_fwd_kernel<32, 2, 1, fused 32>",
           ("k3", 27, 32, 32, 32835, None, "perm_misaligned", None, 0, 0, 0),
           ("k3", 27, 32, 32, 67, None, "perm_misaligned", None, 0, 1, 0),
           ("k3", 27, 32, 32, 32835, None, None, 14, 1, 0, 0), ("k3", 27, 32, 32, 32835, None, None, 19, 1, 0, 1),
           ("k3", 27, 32, 32, 67, None, None, 14, 1, 1, 0), ("k3", 27, 32, 32, 67, None, None, 19, 1, 1, 1)),
    *_rows("conv_fwd_kernel<32, 2, 1, fused 3>",
           ("k3", 27, 3, 20, 32835, None, "odd_cin", None, 0, 0, 0),
           ("k3", 27, 3, 32, 32835, None, "odd_cin", 14, 0, 0, 0), ("k3", 27, 3, 20, 67, None, "odd_cin", None, 0, 1, 0),
           ("k3", 27, 3, 32, 67, None, "odd_cin", 14, 0, 1, 0)),
    *_rows("conv_fwd_kernel<32, 2, 1>",
           ("dense", 1, 148, 20, 32835, 1.0, "cout_tail", None, 0, 0, 0),
           ("dense", 1, 131, 32, 32835, 1.0, "odd_cin", None, 0, 0, 0),
           ("k3", 27, 64, 32, 32835, 1.0, "perm_misaligned", None, 0, 0, 0),
           ("dense", 1, 148, 20, 67, None, "cout_tail", None, 0, 1, 0),
           ("dense", 1, 131, 32, 67, None, "odd_cin", None, 0, 1, 0),
           ("k3", 27, 148, 32, 67, None, "perm_misaligned", None, 0, 1, 0),
           ("dense", 1, 148, 32, 32835, 1.0, None, None, 1, 0, 0), ("dense", 1, 256, 32, 32835, 1.0, None, None, 1, 0, 1),
           ("dense", 1, 148, 32, 67, None, None, None, 1, 1, 0), ("dense", 1, 256, 32, 67, None, None, None, 1, 1, 1)),
    *_rows("conv_fwd_kernel<32, 2, 2>",
           ("dense", 1, 148, 160, 10947, 1.0, "cout_tail", None, 0, 0, 0),
           ("dense", 1, 148, 80, 67, None, "cout_tail", None, 0, 1, 0),
           ("up", 8, 148, 80, 67, None, "cout_tail", None, 0, 1, 0)),
    *_rows("conv_fwd_kernel<32, 2, 3>",
           ("dense", 1, 148, 2052, 1475, 1.0, "cout_tail", None, 0, 0, 0),
           ("dense", 1, 131, 288, 10947, 1.0, "odd_cin", None, 0, 0, 0),
           ("k3", 27, 4, 288, 10947, 1.0, "perm_misaligned", None, 0, 0, 0),
           ("dense", 1, 148, 2052, 67, None, "cout_tail", None, 0, 1, 0),
           ("dense", 1, 131, 192, 67, None, "odd_cin", None, 0, 1, 0),
           ("k3", 27, 148, 192, 67, None, "perm_misaligned", None, 0, 1, 0),
           ("dense", 1, 148, 288, 10947, 1.0, None, None, 1, 0, 0), ("dense", 1, 148, 192, 67, None, None, None, 1, 1, 0)),
    *_rows("conv_fwd_kernel<32, 4, 1, fused 32>",
           ("k3", 27, 32, 64, 32835, None, "perm_misaligned", None, 0, 0, 0),
           ("k3", 27, 32, 64, 14403, None, "perm_misaligned", None, 0, 1, 0),
           ("k3", 27, 32, 64, 32835, None, None, None, 1, 0, 0), ("k3", 27, 32, 64, 14403, None, None, None, 1, 1, 0)),
    *_rows("conv_fwd_kernel<32, 4, 1, fused 64>",
           ("up", 8, 64, 128, 16451, None, "perm_misaligned", None, 0, 0, 0),
           ("k3", 27, 64, 128, 7235, None, "perm_misaligned", None, 0, 1, 0),
           ("up", 8, 64, 128, 16451, None, None, None, 1, 0, 0), ("k3", 27, 64, 128, 7235, None, None, None, 1, 1, 0)),
    *_rows("conv_fwd_kernel<32, 4, 1>",
           ("dense", 1, 148, 48, 47939, 1.0, "cout_tail", None, 0, 0, 0),
           ("dense", 1, 131, 64, 47939, 1.0, "odd_cin", None, 0, 0, 0),
           ("k3", 27, 4, 64, 47939, 1.0, "perm_misaligned", None, 0, 0, 0),
           ("dense", 1, 148, 48, 14403, None, "cout_tail", None, 0, 1, 0),
           ("dense", 1, 131, 64, 14403, None, "odd_cin", None, 0, 1, 0),
           ("k3", 27, 4, 64, 14403, None, "perm_misaligned", None, 0, 1, 0),
           ("dense", 1, 148, 64, 47939, 1.0, None, None, 1, 0, 0),
           ("dense", 1, 148, 64, 14403, None, None, None, 1, 1, 0)),
    *_rows("conv_fwd_kernel<32, 4, 2>",
           ("dense", 1, 148, 160, 24003, 1.0, "cout_tail", None, 0, 0, 0),
           ("dense", 1, 131, 128, 47939, 1.0, "odd_cin", None, 0, 0, 0),
           ("up", 8, 148, 128, 47939, 1.0, "perm_misaligned", None, 0, 0, 0),
           ("dense", 1, 148, 160, 7235, None, "cout_tail", None, 0, 1, 0),
           ("dense", 1, 131, 128, 14403, None, "odd_cin", None, 0, 1, 0),
           ("k3", 27, 32, 128, 14403, None, "perm_misaligned", None, 0, 1, 0),
           ("dense", 1, 148, 128, 47939, 1.0, None, None, 1, 0, 0),
           ("dense", 1, 148, 128, 14403, None, None, None, 1, 1, 0)),
    *_rows("conv_fwd_kernel<32, 4, 3>",
           ("dense", 1, 148, 2176, 963, None, "cout_tail", None, 0, 0, 0),
           ("dense", 1, 131, 384, 5699, None, "odd_cin", None, 0, 0, 0),
           ("k3", 27, 32, 384, 5699, None, "perm_misaligned", None, 0, 0, 0),
           ("dense", 1, 148, 384, 5699, None, None, None, 1, 0, 0),
           ("dense", 1, 256, 384, 5699, None, None, None, 1, 0, 1), ("up", 8, 256, 384, 5699, None, None, None, 1, 0, 1)),
    *_rows("conv_fwd_kernel<64, 1, 1>",
           ("dense", 1, 148, 5, 65603, 1.0, "cout_tail", None, 0, 0, 0),
           ("dense", 1, 131, 16, 65603, 1.0, "odd_cin", None, 0, 0, 0),
           ("k3", 27, 64, 16, 65603, 1.0, "perm_misaligned", None, 0, 0, 0),
           ("dense", 1, 148, 5, 67, None, "cout_tail", None, 0, 1, 0),
           ("dense", 1, 131, 16, 67, None, "odd_cin", None, 0, 1, 0),
           ("k3", 27, 148, 16, 67, None, "perm_misaligned", None, 0, 1, 0),
           ("dense", 1, 148, 16, 65603, 1.0, None, None, 1, 0, 0), ("dense", 1, 256, 16, 65603, 1.0, None, None, 1, 0, 1),
           ("dense", 1, 148, 16, 67, None, None, None, 1, 1, 0), ("dense", 1, 256, 16, 67, None, None, None, 1, 1, 1)),
    *_rows("conv_fwd_kernel<64, 2, 1, fused 32>",
           ("k3", 27, 32, 32, 65603, None, "perm_misaligned", None, 0, 0, 0),
           ("k3", 27, 32, 32, 57539, None, "perm_misaligned", None, 0, 1, 0),
           ("k3", 27, 32, 32, 65603, None, None, 14, 1, 0, 0), ("k3", 27, 32, 32, 57539, None, None, 14, 1, 1, 0)),
    *_rows("conv_fwd_kernel<64, 2, 1, fused 3>",
           ("k3", 27, 3, 20, 65603, None, "odd_cin", None, 0, 0, 0),
           ("k3", 27, 3, 32, 65603, None, "odd_cin", 14, 0, 0, 0),
           ("k3", 27, 3, 20, 57539, None, "odd_cin", None, 0, 1, 0),
           ("k3", 27, 3, 32, 57539, None, "odd_cin", 14, 0, 1, 0)),
    *_rows("conv_fwd_kernel<64, 2, 1>",
           ("dense", 1, 148, 20, 28739, None, "cout_tail", None, 0, 1, 0),
           ("dense", 1, 131, 32, 28739, None, "odd_cin", None, 0, 1, 0),
           ("k3", 27, 64, 32, 28739, None, "perm_misaligned", None, 0, 1, 0),
           ("dense", 1, 148, 32, 28739, None, None, None, 1, 1, 0),
           ("dense", 1, 131, 32, 95939, 1.0, "odd_cin", None, 0, 0, 0),
           ("dense", 1, 148, 32, 95939, 1.0, None, None, 1, 0, 0)),
    *_rows("conv_fwd_kernel<64, 4, 1>",
           ("dense", 1, 148, 48, 65603, None, "cout_tail", None, 0, 0, 0),
           ("dense", 1, 131, 64, 65603, None, "odd_cin", None, 0, 0, 0),
           ("k3", 27, 4, 64, 65603, None, "perm_misaligned", None, 0, 0, 0),
           ("dense", 1, 148, 48, 28739, None, "cout_tail", None, 0, 1, 0),
           ("dense", 1, 131, 64, 28739, None, "odd_cin", None, 0, 1, 0),
           ("k3", 27, 4, 64, 28739, None, "perm_misaligned", None, 0, 1, 0),
           ("dense", 1, 148, 64, 65603, None, None, None, 1, 0, 0),
           ("dense", 1, 148, 64, 28739, None, None, None, 1, 1, 0)),
    *_rows("conv_fwd_kernel<64, 4, 2>",
           ("dense", 1, 148, 160, 14403, None, "cout_tail", None, 0, 0, 0),
           ("dense", 1, 131, 384, 7619, None, "odd_cin", None, 0, 0, 0),
           ("k3", 27, 4, 384, 7619, None, "perm_misaligned", None, 0, 0, 0),
           ("dense", 1, 148, 384, 7619, None, None, None, 1, 0, 0), ("up", 8, 148, 384, 7619, None, None, None, 1, 0, 0)),
    *_rows("conv_fwd_kernel<64, 4, 3>",
           ("dense", 1, 148, 2176, 4035, None, "cout_tail", None, 0, 0, 0),
           ("dense", 1, 131, 384, 24003, None, "odd_cin", None, 0, 0, 0),
           ("up", 8, 148, 384, 24003, None, "perm_misaligned", None, 0, 0, 0),
           ("dense", 1, 148, 384, 24003, None, None, None, 1, 0, 0)),
    *_rows("conv_thin_kernel<32, 32>",
           ("up", 8, 32, 32, 67, None, None, None, 1, 0, 1)),
    *_rows("conv_thin_lds_kernel<32, 32>",
           ("up", 8, 32, 32, 67, 1.0, None, None, 1, 0, 1)),
    *_rows("linear_narrow_kernel<1>",
           ("dense", 1, 148, 1, 67, None, None, None, 0, 0, 0)),
    *_rows("linear_narrow_kernel<3>",
           ("dense", 1, 148, 3, 67, None, None, None, 0, 0, 0)),
    *_rows("linear_narrow_kernel<4>",
           ("dense", 1, 148, 4, 67, None, None, None, 0, 0, 0)),
)

# reachable combinations no row pins because their row faulted or hung on the GPU and the cause was not found: the
# completeness test carries them here, each with a comment, so that nothing is dropped silently.  Empty.
KNOWN_UNPINNED = frozenset()


def case_id(c):
    tile = c.name.replace("conv_", "").replace("_kernel", "").replace(" ", "")
    form = f"f{c.fast}r{c.ring}u{c.full}"
    how = c.reason or ("acc" if c.split else "plain")
    return f"{tile}-{form}-{how}-{c.kind}-{c.Cin}x{c.Cout}-V{c.V}" + ("-alone" if c.scale else "") + (f"-split{c.split}" if c.split else "")


def case_inputs(c):
    """the restatement's inputs of a row: (K, Cin, Cout, Vpad, has_plan, vec_a, buf_ok, acc_init, want_scale)"""
    Vpad = (c.V + PLAN_TILE - 1) // PLAN_TILE * PLAN_TILE
    K = c.K - c.split if c.split else c.K
    return (K, c.Cin, c.Cout, Vpad, c.kind != "dense", c.Cin % 4 == 0, c.reason != "perm_misaligned", c.split is not None,
            c.scale if c.scale is not None else WANT_SCALE_DEFAULT)
