// Which kernel instance, in which form, an fp32 sparse-convolution call runs on: the tile table, the candidate lists and
// the rules, as pure host functions.  This is the ONLY statement of the dispatch: sv_conv_fwd_acc (sv_conv.hip) launches
// what conv_select() returns, sv_conv_select / sv_conv_tile_info (include/sv_hip.h) let Python and the tests ask the same
// code without a GPU.  Plain C++17, no HIP: nothing here makes a runtime call, reads the environment or touches a global.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "sv_hip.h"

namespace sv {

constexpr int PLAN_TILE = SV_TILE_ROWS;  // plans (perm / nbr_s / submask) are laid out in 128-row tiles

// ---- the tile table ----------------------------------------------------------------------------------------------
// Workgroup = 4 waves.  Tile = TM output rows (mask-sorted plan order) x TN output channels.
//   WAVES_N waves split the columns (NT 16-wide MFMA column tiles each), WAVES_M = 4 / WAVES_N split the rows.
// Thin layers (Cin = 3 / 16 / 32 / 64) FUSE several kernel offsets into one pipeline step (CPO = channels per offset,
// compile-time, = Cin): the A tile row of a step is the concatenation of GK neighbours' Cin channels, which is a
// contiguous run of GK * Cin rows of W[K][Cin][Cout] - the same ascending (k, c) accumulation chain in 27 * Cin / 128
// steps instead of 27.  CPO = 0 is the one-offset-per-step form used by the wide layers.

// input channels per pipeline step: short tiles (used on small pyramid levels, where a launch is bound by the latency
// of a tile's sequential step chain) take wider chunks, i.e. fewer barriers / gather round trips per tile
constexpr int chunk_for(int tm, int waves_n) {
  if (waves_n == 1) return tm <= 64 ? 128 : 64;  // tall-narrow tiles (small levels): few, fat steps
  if (waves_n == 2) return tm <= 32 ? 128 : (tm <= 64 ? 64 : 32);
  return tm <= 16 ? 128 : (tm <= 32 ? 64 : 32);
}
constexpr int fused_offsets(int cpo) { return cpo == 0 ? 1 : (cpo < 8 ? 27 : (128 / cpo > 0 ? 128 / cpo : 1)); }

// one instantiated <TM, WAVES_N, NT, CPO> and the constants that decide a launch's form (ConvCfg takes them from here)
struct ConvTile {
  int tm, wn, nt, cpo;
  int mr, tn;     // 16-row sub-tiles per wave, output channels per workgroup
  int gk, kc;     // kernel offsets and A columns per pipeline step
  int pfd;        // A-operand prefetch distance in k-steps (RING form)
  bool use_full;  // the tile has a FULL form
};
constexpr ConvTile conv_tile(int tm, int wn, int nt, int cpo = 0) {
  const int mr = tm / (4 / wn) / 16;
  const int gk = fused_offsets(cpo);
  const int kc = cpo ? (gk * cpo + 3) / 4 * 4 : chunk_for(tm, wn);
  // A-operand prefetch distance in k-steps: enough matrix work (MR * NT ops of 32 cycles) to cover ~250 cycles
  // (big tiles, MR * NT >= 6: one k-step, their waves hide the rest behind each other)
  const int pfd_raw = mr * nt >= 6 ? 1 : (8 + mr * nt - 1) / (mr * nt);
  const int pfd = pfd_raw > kc / 4 ? kc / 4 : pfd_raw;
  // the FULL form (see the kernel) pays where a k-step is one or two matrix ops and the per-k-step bookkeeping of
  // the general form dominates; on the 64-row tile it gained nothing and compiles to 107 VGPRs (four
  // waves per SIMD) where the general form's WIDE step fits five (94-95 VGPRs, conv_tile_body); on 16x128 tiles it
  // measured slower (profiles/r01_conv_full_form.txt)
  const bool use_full = (mr * nt == 1) || (tm == 32 && wn == 4 && nt == 3) || (tm == 16 && nt == 3);
  return {tm, wn, nt, cpo, mr, wn * nt * 16, gk, kc, pfd, use_full};
}

// every instantiation of the tiled kernel (sv_conv.hip builds one launcher per row); the ten rows no list below names are
// reached through the SV_CONV_FORCE* switches only
constexpr ConvTile CONV_TILES[] = {
    conv_tile(128, 4, 3), conv_tile(128, 2, 3), conv_tile(128, 1, 3), conv_tile(64, 4, 3), conv_tile(64, 2, 3),
    conv_tile(64, 1, 3), conv_tile(32, 4, 3), conv_tile(32, 2, 3), conv_tile(16, 4, 3),
    conv_tile(128, 4, 2), conv_tile(128, 2, 2), conv_tile(128, 1, 2), conv_tile(64, 4, 2), conv_tile(64, 2, 2),
    conv_tile(64, 1, 2), conv_tile(32, 4, 2), conv_tile(32, 2, 2), conv_tile(16, 4, 2),
    conv_tile(64, 4, 1), conv_tile(32, 4, 1), conv_tile(16, 4, 1), conv_tile(128, 2, 1), conv_tile(64, 2, 1),
    conv_tile(32, 2, 1), conv_tile(128, 1, 1), conv_tile(64, 1, 1),
    // fused-offset forms of the thin layers
    conv_tile(64, 2, 1, 3), conv_tile(32, 2, 1, 3), conv_tile(64, 2, 1, 32), conv_tile(32, 2, 1, 32),
    conv_tile(32, 4, 1, 32), conv_tile(16, 4, 1, 32), conv_tile(32, 4, 1, 64), conv_tile(16, 4, 1, 64)};
constexpr int N_CONV_TILES = (int)(sizeof(CONV_TILES) / sizeof(CONV_TILES[0]));
static_assert(N_CONV_TILES == 34, "the instantiated tiles");

constexpr int find_conv_tile(int tm, int wn, int nt, int cpo) {  // row of CONV_TILES, -1 = not instantiated
  for (int i = 0; i < N_CONV_TILES; ++i)
    if (CONV_TILES[i].tm == tm && CONV_TILES[i].wn == wn && CONV_TILES[i].nt == nt && CONV_TILES[i].cpo == cpo) return i;
  return -1;
}

// ---- what a call looks like to the rules, and what they choose ------------------------------------------------------
struct ConvShape {
  int K, Cin, Cout;
  int64_t Vpad;
  bool has_plan;        // perm / nbr_s / submask given (dense rows have none)
  bool has_tile_order;  // the plan carries its longest-first tile order
  bool vec_a;           // in_ld % 4 == 0 && Cin % 4 == 0 && `in` 16-byte aligned -> float4 gathers
  bool buf_ok;          // every operand inside the 2 GB buffer extent and `perm` 16-byte aligned
  bool has_acc_init;    // the launch continues an earlier pass's chains
  bool w_aligned;       // W 16-byte aligned
  bool alone;           // the caller said that the GPU holds one frame: sv_conv_set_dispatch(want_scale >= 1)
};

enum ConvKind { CONV_FIRST_MFMA, CONV_FIRST_LAYER, CONV_THIN, CONV_THIN_LDS, CONV_NARROW, CONV_TILE, CONV_DUAL };  // names: conv_choice_name

struct ConvChoice {
  ConvKind kind;
  int tm, tail_tm, wn, nt, cpo;  // CONV_TILE / CONV_DUAL: the tile (tail_tm: the dual launch's tail body); CONV_NARROW: nt = <n>
  bool fast, ring, full;
  int tail128 = 0;  // CONV_DUAL: plan tiles (the cheapest, at the end of tile_order) that the tail body runs
};

// Form of tile `t` for a shape.
// FAST: float4 gathers, Cout a multiple of TN, operands addressed through buffer descriptors; odd channel counts
//   (Cin = 3) only exist in the guarded form.
// RING: launches of at most ~4 workgroups per CU are bound by the latency of one wave's step chain, not by the matrix
//   pipe: their waves read the A operands several k-steps ahead (register ring); fuller launches hide that latency
//   behind co-resident waves and are a few % faster with the plain one-step-ahead read.
// FULL: no partial channel chunk anywhere in the layer.
inline ConvChoice conv_tile_form(const ConvTile& t, const ConvShape& s) {
  const int64_t grid = (s.Vpad / t.tm) * ((s.Cout + t.tn - 1) / t.tn);
  const bool fast = t.cpo % 4 == 0 && s.vec_a && s.buf_ok && s.Cout % t.tn == 0;
  const bool ring = t.pfd > 1 && grid <= 1024;
  const bool full = fast && t.use_full && (t.cpo ? s.K % t.gk == 0 : s.Cin % t.kc == 0);
  return {CONV_TILE, t.tm, 0, t.wn, t.nt, t.cpo, fast, ring, full};
}

// ---- the candidate lists --------------------------------------------------------------------------------------------
// A tile is processed sequentially (K * Cin / KC steps) and streams K*Cin*TN weights + its gathered rows through one CU,
// so the choice trades per-CU cache bandwidth (tall tiles, few column slices) against parallelism / tail (many tiles).
// Candidates are listed from least to most traffic; the first one that puts `want` workgroups on the chip wins,
// otherwise the one with the most workgroups.
struct Candidate {
  int tm, wn, nt;
  int64_t want;  // chosen when it yields at least this many workgroups (measured on the Cfg-2 pyramid, profiles/)
  int cpo = 0;   // fused-offset form for this Cin (0 = one offset per step)
};
struct CandidateList {
  const Candidate* c;
  int n;
  template <int N>
  constexpr CandidateList(const Candidate (&l)[N]) : c(l), n(N) {}
};
template <int N>
constexpr bool conv_list_ok(const Candidate (&l)[N]) {  // every candidate is instantiated; the last takes whatever is left
  for (int i = 0; i < N; ++i)
    if (find_conv_tile(l[i].tm, l[i].wn, l[i].nt, l[i].cpo) < 0) return false;
  return l[N - 1].want == 0;
}

// The last entry of a list serves the small pyramid levels, where a layer is a few hundred short workgroups and its
// duration is the serial (offset, chunk) chain of one of them: 16-row tiles with 128-channel chunks are fastest
// there (tools/sweep_small.sh, profiles/r01_conv_small_level_sweep.txt).
constexpr Candidate wide3[] = {{64, 4, 3, 2500}, {32, 4, 3, 1500}, {32, 2, 3, 0}};
// Cout % 128 == 0 (384): settled-clock sweeps of every level, profiles/r02_conv_instance_sweep.txt.  Below the
// chip-filling size the 16-row tile in its FULL form (Cin a multiple of its 128-channel step: 384, 512) wins at every
// level (level 1: 96.4 TFLOP/s against 90.1 for 64x128, level 3: 41 against 34 for 16x128); with a partial last chunk
// (Cin 416 / 448, the first conv after a concatenation) it only wins once 64x128 tiles no longer fill the chip
// ({32,4,3} between them: inside the frame pipeline level 2 - 432 workgroups of 32 x 192 - is 0.8 % of a frame faster on
// 32-row tiles although they are 25 % slower than the 16-row tiles alone: half the weight traffic beside the chip-filling
// launches of the other frames; 64.3 against 63.8 frames/s, three alternating runs, tools/ab_env.sh)
constexpr Candidate wide3_128[] = {{64, 4, 3, 2500}, {64, 4, 2, 1200}, {32, 4, 3, 1200}, {16, 4, 3, 0}};
constexpr Candidate wide3_128_full[] = {{64, 4, 3, 2500}, {32, 4, 3, 1200}, {16, 4, 3, 0}};
constexpr Candidate wide2[] = {{128, 4, 2, 1300}, {64, 4, 2, 1500}, {32, 4, 2, 1500}, {32, 2, 2, 0}};
constexpr Candidate wide2_64[] = {{128, 4, 2, 1300}, {64, 4, 2, 1500}, {32, 4, 2, 1500}, {16, 4, 1, 0}};  // % 64
constexpr Candidate c64[] = {{64, 4, 1, 1500}, {32, 4, 1, 1500}, {16, 4, 1, 0}};
constexpr Candidate c32[] = {{128, 2, 1, 1500}, {64, 2, 1, 1500}, {32, 2, 1, 0}};
constexpr Candidate c16[] = {{128, 1, 1, 600}, {64, 1, 1, 0}};
// thin layers: fused-offset forms (the input row is at most 256 B, so one offset per step would be all overhead)
constexpr Candidate f3[] = {{64, 2, 1, 3000, 3}, {32, 2, 1, 0, 3}};
constexpr Candidate f32_32[] = {{64, 2, 1, 3000, 32}, {32, 2, 1, 0, 32}};
constexpr Candidate f32_64[] = {{32, 4, 1, 1500, 32}, {16, 4, 1, 0, 32}};
constexpr Candidate f64_64[] = {{32, 4, 1, 1500, 64}, {16, 4, 1, 0, 64}};
static_assert(conv_list_ok(wide3), "wide3");
static_assert(conv_list_ok(wide3_128), "wide3_128");
static_assert(conv_list_ok(wide3_128_full), "wide3_128_full");
static_assert(conv_list_ok(wide2), "wide2");
static_assert(conv_list_ok(wide2_64), "wide2_64");
static_assert(conv_list_ok(c64), "c64");
static_assert(conv_list_ok(c32), "c32");
static_assert(conv_list_ok(c16), "c16");
static_assert(conv_list_ok(f3), "f3");
static_assert(conv_list_ok(f32_32), "f32_32");
static_assert(conv_list_ok(f32_64), "f32_64");
static_assert(conv_list_ok(f64_64), "f64_64");

inline CandidateList conv_list_for(const ConvShape& s) {
  const int Cout = s.Cout;
  if (s.K > 1) {
    if (s.Cin == 3 && Cout > 16 && Cout <= 32) return f3;
    if (s.Cin == 32 && s.vec_a && Cout == 32) return f32_32;
    if (s.Cin == 32 && s.vec_a && Cout == 64) return f32_64;
    if (s.Cin == 64 && s.vec_a && (Cout == 64 || Cout == 128)) return f64_64;
  }
  if (Cout > 128 && (Cout % 192 == 0 || Cout % 96 == 0 || Cout > 2048)) {
    if (Cout % 128 != 0) return wide3;
    if (s.Cin % 128 == 0 && s.vec_a) return wide3_128_full;
    return wide3_128;
  }
  if (Cout > 64 && Cout % 64 == 0) return wide2_64;
  if (Cout > 64) return wide2;
  if (Cout > 32) return c64;
  if (Cout > 16) return c32;
  return c16;
}

// library defaults of the two dispatch knobs (environment SV_CONV_WANT_SCALE / SV_CONV_TAIL, sv_conv_set_dispatch)
// The `want` figures of the lists were measured one launch at a time (profiles/*_conv_instance_sweep.txt).  Inside the
// two-stream frame pipeline the taller tile wins earlier: its weight traffic per flop is lower (level 1, 384 -> 384:
// 64-row tiles read W once per 64 rows, 16-row tiles once per 16 - alone on the GPU both run at ~107 TFLOP/s, with
// perfect weight locality the 16-row tile would gain 7 %), and the launch tail that costs the short grid alone is
// filled by the neighbour frame's kernels.  Scaling every threshold by 0.3 moves level 1 (830 workgroups of 64 x 192)
// onto the dual-body launch and leaves levels 2-4 where they were: frames/s 60.9 -> 62.0 (0.15: 62.1, 0.08: 61.1,
// 0.03: 60.7; three alternating runs each).
#ifndef SV_CONV_WANT_SCALE_DEFAULT
#define SV_CONV_WANT_SCALE_DEFAULT 0.3
#endif
#ifndef SV_CONV_TAIL_DEFAULT
#define SV_CONV_TAIL_DEFAULT 0.15  // share of the plan tiles (the cheapest) that chip-filling launches run as half-height tiles
#endif

// ---- the rules ------------------------------------------------------------------------------------------------------
// want_scale scales every list threshold; tail_fraction = share of the plan tiles a chip-filling 384-wide launch runs as
// 32-row tiles at the end of its grid (the dual-body launch).
inline ConvChoice conv_select(const ConvShape& s, double want_scale, double tail_fraction) {
  // special shapes first: the 3 -> 32 first layer, the thin 32 -> 32 layers, dense rows with <= 4 outputs
  if (s.has_plan && s.K > 1 && s.K <= 27 && s.Cin == 3 && s.Cout == 32 && !s.has_acc_init) {
    if (s.buf_ok) return {CONV_FIRST_MFMA, 0, 0, 0, 0, 0, true, false, true};
    return {CONV_FIRST_LAYER, 0, 0, 0, 0, 0, false, false, false};  // the thread-per-voxel kernel with 64-bit addresses
  }
  if (s.has_plan && s.K > 1 && s.K <= 32 && s.Cin == 32 && s.Cout == 32 && s.vec_a && s.buf_ok && !s.has_acc_init) {
    // the kernel with the layer's weights resident in LDS needs whole CUs (one 16-wave workgroup each, 27 offsets of
    // weights staged by float4): for a GPU that holds ONE frame only, see launch_conv_thin_lds (sv_conv_special.hip)
    const bool lds = s.alone && s.K <= 27 && s.w_aligned;
    return {lds ? CONV_THIN_LDS : CONV_THIN, 0, 0, 0, 0, 0, true, false, true};
  }
  if (!s.has_plan && s.K == 1 && s.Cout <= 4 && s.vec_a && s.Cin >= 64 && !s.has_acc_init)
    return {CONV_NARROW, 0, 0, 0, s.Cout, 0, false, false, false};
  const CandidateList list = conv_list_for(s);
  const Candidate* c = &list.c[list.n - 1];
  for (int i = 0; i < list.n; ++i) {
    const Candidate& ci = list.c[i];
    const int tn = ci.wn * ci.nt * 16;
    if ((double)((s.Vpad / ci.tm) * ((s.Cout + tn - 1) / tn)) >= want_scale * (double)ci.want) {
      c = &ci;
      break;
    }
  }
  const ConvChoice tile = conv_tile_form(CONV_TILES[find_conv_tile(c->tm, c->wn, c->nt, c->cpo)], s);
  // chip-filling 384-wide layers: 64-row tiles, and 32-row tiles for the cheapest plan tiles at the end of the grid -
  // in the FAST form only, and with a tile order to tell the cheapest tiles by
  if (c->tm == 64 && c->wn == 4 && c->nt == 3 && c->cpo == 0 && tail_fraction > 0.0) {
    const int n128 = (int)(s.Vpad / PLAN_TILE);
    const int tail128 = (int)(n128 * tail_fraction);
    if (tile.fast && s.has_tile_order && tail128 >= 1 && tail128 < n128) return {CONV_DUAL, 64, 32, 4, 3, 0, true, false, false, tail128};
  }
  return tile;
}

// "name|fast=F,ring=R,full=U": what sv_conv_last_instance() reports after the launch of `c`
inline void conv_choice_name(const ConvChoice& c, char* buf, size_t size) {
  static const char* const special[] = {"conv_first_mfma_kernel<3, 32>", "conv_first_layer_kernel<3, 32>",
                                        "conv_thin_kernel<32, 32>", "conv_thin_lds_kernel<32, 32>"};
  char name[64];
  if (c.kind <= CONV_THIN_LDS)
    snprintf(name, sizeof(name), "%s", special[c.kind]);
  else if (c.kind == CONV_NARROW)
    snprintf(name, sizeof(name), "linear_narrow_kernel<%d>", c.nt);
  else if (c.kind == CONV_DUAL)
    snprintf(name, sizeof(name), "conv_fwd_dual_kernel<%d, %d, %d, %d>", c.tm, c.tail_tm, c.wn, c.nt);
  else if (c.cpo)
    snprintf(name, sizeof(name), "conv_fwd_kernel<%d, %d, %d, fused %d>", c.tm, c.wn, c.nt, c.cpo);
  else
    snprintf(name, sizeof(name), "conv_fwd_kernel<%d, %d, %d>", c.tm, c.wn, c.nt);
  snprintf(buf, size, "%s|fast=%d,ring=%d,full=%d", name, (int)c.fast, (int)c.ring, (int)c.full);
}

}  // namespace sv
