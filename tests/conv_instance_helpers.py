"""Which kernel instance, in which form, a public fp32 sparse-convolution call runs on - restated from the C++ - and the
table of cases that pins every reachable one (tests/test_conv_instances_cpu.py: completeness, tests/test_gpu_conv_instances.py:
bit-exactness against the oracle).

The restatement follows sv_conv_fwd_acc (csrc/sv_conv.hip: the special-shape kernels), select_and_launch (the candidate
lists and their thresholds), launch_conv (the FAST / RING / FULL form of a tile) and launch_conv_dual.  It is written from
that code alone; profiling.conv_kernel_config is a second, older mirror of the names only, and the CPU test holds the two
against each other.
"""
from collections import namedtuple
from functools import lru_cache

PLAN_TILE = 128
WANT_SCALE_DEFAULT = 0.3   # SV_CONV_WANT_SCALE_DEFAULT
TAIL_DEFAULT = 0.15        # SV_CONV_TAIL_DEFAULT


# ---- ConvCfg<TM, WAVES_N, NT, CPO> -------------------------------------------------------------------------------
def chunk_for(tm, waves_n):
    if waves_n == 1:
        return 128 if tm <= 64 else 64
    if waves_n == 2:
        return 128 if tm <= 32 else (64 if tm <= 64 else 32)
    return 128 if tm <= 16 else (64 if tm <= 32 else 32)


def fused_offsets(cpo):
    if cpo == 0:
        return 1
    if cpo < 8:
        return 27
    return 128 // cpo if 128 // cpo > 0 else 1


TileCfg = namedtuple("TileCfg", "MR TN GK KC PFD USE_FULL")


@lru_cache(maxsize=None)
def tile_cfg(tm, wn, nt, cpo=0):
    """the per-tile constants of ConvCfg that decide a launch's form"""
    waves_m = 4 // wn
    mr = tm // waves_m // 16
    tn = wn * nt * 16
    gk = fused_offsets(cpo)
    kc = (gk * cpo + 3) // 4 * 4 if cpo else chunk_for(tm, wn)
    pfd_raw = 1 if mr * nt >= 6 else (8 + mr * nt - 1) // (mr * nt)
    pfd = min(pfd_raw, kc // 4)
    use_full = (mr * nt == 1) or (tm == 32 and wn == 4 and nt == 3) or (tm == 16 and nt == 3)
    return TileCfg(mr, tn, gk, kc, pfd, use_full)


# the 34 instantiations of launch_candidate(), (TM, WAVES_N, NT, CPO)
INSTANTIATED = (
    [(tm, wn, 3, 0) for tm, wn in ((128, 4), (128, 2), (128, 1), (64, 4), (64, 2), (64, 1), (32, 4), (32, 2), (16, 4))] +
    [(tm, wn, 2, 0) for tm, wn in ((128, 4), (128, 2), (128, 1), (64, 4), (64, 2), (64, 1), (32, 4), (32, 2), (16, 4))] +
    [(tm, wn, 1, 0) for tm, wn in ((64, 4), (32, 4), (16, 4), (128, 2), (64, 2), (32, 2), (128, 1), (64, 1))] +
    [(64, 2, 1, 3), (32, 2, 1, 3), (64, 2, 1, 32), (32, 2, 1, 32), (32, 4, 1, 32), (16, 4, 1, 32), (32, 4, 1, 64),
     (16, 4, 1, 64)])

# ---- select_and_launch: candidate lists (tm, wn, nt, want, cpo) ----------------------------------------------------
WIDE3 = [(64, 4, 3, 2500, 0), (32, 4, 3, 1500, 0), (32, 2, 3, 0, 0)]
WIDE3_128 = [(64, 4, 3, 2500, 0), (64, 4, 2, 1200, 0), (32, 4, 3, 1200, 0), (16, 4, 3, 0, 0)]
WIDE3_128_FULL = [(64, 4, 3, 2500, 0), (32, 4, 3, 1200, 0), (16, 4, 3, 0, 0)]
WIDE2 = [(128, 4, 2, 1300, 0), (64, 4, 2, 1500, 0), (32, 4, 2, 1500, 0), (32, 2, 2, 0, 0)]
WIDE2_64 = [(128, 4, 2, 1300, 0), (64, 4, 2, 1500, 0), (32, 4, 2, 1500, 0), (16, 4, 1, 0, 0)]
C64 = [(64, 4, 1, 1500, 0), (32, 4, 1, 1500, 0), (16, 4, 1, 0, 0)]
C32 = [(128, 2, 1, 1500, 0), (64, 2, 1, 1500, 0), (32, 2, 1, 0, 0)]
C16 = [(128, 1, 1, 600, 0), (64, 1, 1, 0, 0)]
F3 = [(64, 2, 1, 3000, 3), (32, 2, 1, 0, 3)]
F32_32 = [(64, 2, 1, 3000, 32), (32, 2, 1, 0, 32)]
F32_64 = [(32, 4, 1, 1500, 32), (16, 4, 1, 0, 32)]
F64_64 = [(32, 4, 1, 1500, 64), (16, 4, 1, 0, 64)]
ALL_LISTS = (WIDE3, WIDE3_128, WIDE3_128_FULL, WIDE2, WIDE2_64, C64, C32, C16, F3, F32_32, F32_64, F64_64)


@lru_cache(maxsize=None)
def candidate_list(K, Cin, Cout, vec_a):
    if Cout > 128 and (Cout % 192 == 0 or Cout % 96 == 0 or Cout > 2048):
        if Cout % 128 != 0:
            cands = WIDE3
        elif Cin % 128 == 0 and vec_a:
            cands = WIDE3_128_FULL
        else:
            cands = WIDE3_128
    elif Cout > 64:
        cands = WIDE2_64 if Cout % 64 == 0 else WIDE2
    elif Cout > 32:
        cands = C64
    elif Cout > 16:
        cands = C32
    else:
        cands = C16
    if K > 1:
        if Cin == 3 and 16 < Cout <= 32:
            cands = F3
        elif Cin == 32 and vec_a and Cout == 32:
            cands = F32_32
        elif Cin == 32 and vec_a and Cout == 64:
            cands = F32_64
        elif Cin == 64 and vec_a and Cout in (64, 128):
            cands = F64_64
    return cands


@lru_cache(maxsize=None)
def _tile_name(tm, wn, nt, cpo):
    return f"conv_fwd_kernel<{tm}, {wn}, {nt}, fused {cpo}>" if cpo else f"conv_fwd_kernel<{tm}, {wn}, {nt}>"


def _tile_launch(tm, wn, nt, cpo, K, Cin, Cout, Vpad, vec_a, buf_ok):
    """launch_conv<TM, WAVES_N, NT, CPO>: (name, fast, ring, full) as note_instance() writes them"""
    cfg = tile_cfg(tm, wn, nt, cpo)
    grid = (Vpad // tm) * ((Cout + cfg.TN - 1) // cfg.TN)
    fast = vec_a and buf_ok and Cout % cfg.TN == 0
    ring = cfg.PFD > 1 and grid <= 1024
    f = (cpo % 4 == 0) and fast
    full = cfg.USE_FULL and ((K % cfg.GK == 0) if cpo else (Cin % cfg.KC == 0))
    return _tile_name(tm, wn, nt, cpo), int(f), int(ring), int(f and full)


def dispatch_key(K, Cin, Cout, Vpad, has_plan, vec_a, buf_ok, acc_init, want_scale=WANT_SCALE_DEFAULT,
                 tail_fraction=TAIL_DEFAULT, w_aligned=True):
    """(name, fast, ring, full) of sv_conv_last_instance() after the call.  vec_a: the input view allows float4 gathers
    (Cin and its row stride multiples of 4, 16-byte aligned start); buf_ok: every operand inside the 2 GB buffer extent
    and `perm` 16-byte aligned; want_scale >= 1 stands for conv_dispatch(1.0) - one frame alone on the GPU, which also
    moves the thin layers onto the LDS-weights kernel (w_aligned: the weight pointer is 16-byte aligned)."""
    assert Vpad % PLAN_TILE == 0 and Vpad > 0 and 1 <= K <= 32 and (has_plan or K == 1)
    assert not vec_a or Cin % 4 == 0
    if has_plan and 1 < K <= 27 and Cin == 3 and Cout == 32 and not acc_init:
        if buf_ok:
            return "conv_first_mfma_kernel<3, 32>", 1, 0, 1
        return "conv_first_layer_kernel<3, 32>", 0, 0, 0
    if has_plan and K > 1 and Cin == 32 and Cout == 32 and vec_a and buf_ok and not acc_init:
        if want_scale >= 1.0 and K <= 27 and w_aligned:
            return "conv_thin_lds_kernel<32, 32>", 1, 0, 1
        return "conv_thin_kernel<32, 32>", 1, 0, 1
    if not has_plan and K == 1 and Cout <= 4 and vec_a and Cin >= 64 and not acc_init:
        return f"linear_narrow_kernel<{min(Cout, 4)}>", 0, 0, 0
    cands = candidate_list(K, Cin, Cout, vec_a)
    chosen = cands[-1]
    for c in cands:
        tm, wn, nt, want, cpo = c
        tn = wn * nt * 16
        if float((Vpad // tm) * ((Cout + tn - 1) // tn)) >= want_scale * float(want):
            chosen = c
            if tm == 64 and wn == 4 and nt == 3 and cpo == 0 and tail_fraction > 0.0:
                # launch_conv_dual<64, 32, 4, 3>: needs the FAST form, a plan's tile_order and a tail of 1 .. n128 - 1 tiles
                n128 = Vpad // PLAN_TILE
                tail128 = int(n128 * tail_fraction)
                if vec_a and buf_ok and Cout % tile_cfg(64, 4, 3).TN == 0 and has_plan and 1 <= tail128 < n128:
                    return "conv_fwd_dual_kernel<64, 32, 4, 3>", 1, 0, 0
            break
    tm, wn, nt, _, cpo = chosen
    return _tile_launch(tm, wn, nt, cpo, K, Cin, Cout, Vpad, vec_a, buf_ok)


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
# every list, Cout % TN == 0 and not: c16 (5, 16), c32 (20, 32), c64 (48, 64), wide2 (80), wide2_64 (128), wide3 (192, 288),
# wide3_128 (384), beyond 2048 (2052: the only kind of width the wide3 list takes that leaves <32, 2, 3> a partial column
# tile, 2176: the same for the 192-column tiles of the wide3_128 lists), and the widths the narrow kernel takes (1, 3, 4)
SWEEP_COUT = (1, 3, 4, 5, 16, 20, 32, 48, 64, 80, 128, 192, 288, 384, 2052, 2176)
# every padded row count up to 136k: the last new combination appears at 131200 rows (more than 1024 workgroups of a 128-row
# tile), none between there and 300k
SWEEP_VPAD = tuple(range(128, 136 * 1024 + 1, 128))


def sweep():
    """{(name, fast, ring, full)} of every combination the public call reaches.  has_plan = (K > 1): nn.conv_forward gives
    dense rows no plan and every kernel map one.  vec_a is swept over both values where Cin allows it (a view whose row
    stride or start is not 16-byte aligned); buf_ok = False only with a plan (a `perm` off a 16-byte boundary; without a
    plan it takes a tensor beyond 2 GB, which sv_conv_fwd_acc splits into row ranges that fit)."""
    seen = {}
    for ws in SWEEP_SCALES:
        for K in SWEEP_K:
            has_plan = K > 1
            for Cin in SWEEP_CIN:
                for vec_a in ((True, False) if Cin % 4 == 0 else (False,)):
                    for Cout in SWEEP_COUT:
                        for buf_ok in ((True, False) if has_plan else (True,)):
                            for acc_init in (False, True):
                                for Vpad in SWEEP_VPAD:
                                    k = dispatch_key(K, Cin, Cout, Vpad, has_plan, vec_a, buf_ok, acc_init, ws)
                                    if k not in seen:
                                        seen[k] = (K, Cin, Cout, Vpad, has_plan, vec_a, buf_ok, acc_init, ws)
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
