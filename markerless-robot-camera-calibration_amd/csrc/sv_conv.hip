// K6/K7: output-stationary sparse convolution on fp32 MFMA (v_mfma_f32_16x16x4_f32) with fused epilogue.
//
// Replaces ME.MinkowskiConvolution / MinkowskiConvolutionTranspose / MinkowskiLinear followed by
// MinkowskiBatchNorm(eval) (+ residual) (+ ReLU / LeakyReLU): model/backbone/minkunet.py:125-187,
// model/backbone/resnet.py:95-127 (BasicBlock via ME), model/robotnet_segmentation.py:55-64.
//
// This file: the ABI entry points, the tiled kernel and its launchers; the special-shape kernels (thin layers, conv0, narrow
// linear) are in sv_conv_special.hip, what both share in sv_conv_params.h.  WHICH instance a call runs on - the tile table,
// the candidate lists, the rules - is in sv_conv_select.h and nowhere else.
//
// Work decomposition (details at ConvCfg / conv_fwd_kernel below, measurements in DESIGN.md 4.1)
//   * a workgroup (4 waves) owns one tile of TM output rows (in the plan's mask-sorted order) x TN output channels;
//   * it walks pipeline steps = (kernel offset k ASCENDING, input-channel chunk ascending); thin layers fuse several
//     offsets into one step;
//   * per step the gathered input rows (A, TM x KC) go global -> registers -> LDS (double buffered, one barrier per
//     step); the weights (B, KC x TN) go straight from L2/HBM to registers;
//   * each wave multiplies with v_mfma_f32_16x16x4_f32; a 16-row sub-tile is skipped for an offset when none of its rows
//     has a neighbour there (plan submask), which is what makes the mask-sorted row order pay.
// Numerics: every output element is ONE f32 fma chain over (k ascending, c ascending) — the MFMA is a k-ordered
// fmaf chain (MI355X guide §3) — so results are bitwise reproducible and match oracle/sv_oracle.c exactly.
// A missing neighbour contributes fma(0, w, acc) = acc.
#include <stdio.h>
#include <stdlib.h>
#include <array>
#include <utility>
#include <vector>

#include "sv_conv_params.h"

namespace sv {

// name of the kernel instance the last sv_conv_fwd call of this thread launched, "name|fast=F,ring=R,full=U"
// (conv_choice_name; sv_conv_last_instance(): tests and the bench's per-kernel records read it back)
static thread_local char g_last_instance[128] = "";
// per-thread override of the dispatch thresholds (sv_conv_set_dispatch): < 0 = the library default / environment
static thread_local double g_want_scale_override = -1.0;
static thread_local double g_tail_override = -1.0;

constexpr int lds_row_stride(int kc) {
  // smallest stride >= kc + 2 for which the 16x16x4 operand read (lane = row li, k-offset lq: word li * SA + lq)
  // touches 64 distinct LDS banks: SA mod 64 = 34, or SA = 4 * odd
  for (int sa = kc + 2;; ++sa)
    if (sa % 64 == 34 || (sa % 4 == 0 && (sa / 4) % 2 == 1)) return sa;
}

// Workgroup = 4 waves.  Tile = TM_ output rows (mask-sorted plan order) x TN output channels; the table of tiles and the
// constants selection reads (MR .. USE_FULL) are in sv_conv_select.h, the ones only the kernel needs here.
//   Column tiles are INTERLEAVED: MFMA column j of tile n is output channel n0 + wn*NT*16 + NT*j + n, so a lane's B
//   operands for its NT tiles are NT consecutive floats of a weight row (one dwordxNT load straight from L2/HBM into
//   registers — the weight slab is not shared between waves, an LDS round trip would be pure overhead) and the
//   epilogue stores NT consecutive floats per lane.
template <int TM_, int WAVES_N, int NT, int CPO = 0>
struct ConvCfg {
  static constexpr ConvTile T = conv_tile(TM_, WAVES_N, NT, CPO);
  static constexpr int WAVES_M = 4 / WAVES_N;
  static constexpr int MR = T.mr, TN = T.tn, GK = T.gk, KC = T.kc, PFD = T.pfd;
  static constexpr bool USE_FULL = T.use_full;
  static constexpr int SA = lds_row_stride(KC);  // A row stride in floats
  static constexpr int F4_PER_ROW = KC / 4;      // float4 per gathered row and step
  static constexpr int ROWS_PER_PASS = 256 / F4_PER_ROW;
  static constexpr int A_F4 = (TM_ + ROWS_PER_PASS - 1) / ROWS_PER_PASS;  // float4 gathers per thread and step
  static_assert(MR >= 1, "tile too small for the wave layout");
  static constexpr size_t lds_bytes(int K) { return (size_t)(2 * TM_ * SA + K * TM_) * sizeof(float); }
};

// One pipeline step = (kernel offset k, input-channel chunk c0), visited in ascending (k, c0) order (CPO > 0: GK
// consecutive offsets x all Cin channels per step).
//   A (gathered rows, TM_ x KC): global -> registers one step ahead -> LDS (double buffered), one barrier per step.
//   B (weights, KC x TN): global -> registers, re-loaded for the next step right after their last use.
// FAST: float4 gathers, Cout a multiple of TN -> every load is unconditional (out-of-range lanes read a safe address and
//   are zeroed afterwards), so the loop body is straight-line and hipcc can emit COUNTED vmcnt waits; the generic
//   variant keeps per-lane guards (odd channel counts such as Cin = 3 or Cout = 3).
// RING: A operands are read PFD k-steps ahead of the matrix ops through a register ring (launches of few workgroups).
// FULL: no partial chunk in the layer -> compile-time trip count and plain weight addressing in the matrix loop.
// conv_tile_body: one workgroup's tile.  bidx = index of the workgroup inside its body's range of the grid, tile_base =
// first entry of tile_order (plan tiles of 128 rows, longest first) that range starts at.
template <int TM_, int WAVES_N, int NT, bool FAST, int CPO = 0, bool RING = false, bool FULL = false>
__device__ __forceinline__ void conv_tile_body(const ConvParams& p, const int bidx, const int tile_base) {
  static_assert(FAST || !FULL, "FULL is a refinement of the FAST form");
  using Cfg = ConvCfg<TM_, WAVES_N, NT, CPO>;
  constexpr int MR = Cfg::MR, TN = Cfg::TN, A_F4 = Cfg::A_F4, KC = Cfg::KC, SA = Cfg::SA, GK = Cfg::GK;
  constexpr int PFD = RING ? Cfg::PFD : 1;  // RING: launches too small to fill the chip (see launch_conv)
  constexpr int ROWS_PER_PASS = Cfg::ROWS_PER_PASS;
  constexpr int SUBS = TM_ / 16;  // sub-tiles per tile
  // WIDE: the 384-column form of the chip-filling layers (64-row tile and the 32-row tail body of the dual launch).  Its
  // step keeps FOUR k-steps of weights and HALF a step's gathers in registers (see the step below), which is what lets
  // five waves per SIMD be resident (96 VGPRs)
  constexpr bool WIDE = FAST && !FULL && !RING && CPO == 0 && WAVES_N == 4 && NT == 3 && (TM_ == 64 || TM_ == 32);
  static_assert(!WIDE || A_F4 == 2, "the WIDE step moves a step's gathers in two halves");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* As = lds;                             // [2][TM_][SA]
  int* idx_s = (int*)(lds + 2 * TM_ * SA);     // [K][TM_] gathered input row of every (offset, tile row)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WAVES_N, wn = wid % WAVES_N;
  unsigned long long trace_t0 = 0, trace_t_loop = 0, trace_t_epi = 0;
  int trace_steps = 0;
  if (p.trace) trace_t0 = wall_clock64();
  // 1-D grid, longest tiles first (list scheduling): plan tiles are visited in the plan's tile_order (sorted by active
  // (offset, sub-tile) slots, descending); without one, in reverse plan order (rows are sorted by neighbour key, so
  // the tiles with the most neighbour offsets sit at the end).
  const int ny = (p.Cout + TN - 1) / TN;
  constexpr int SUB_PER_PLAN_TILE = PLAN_TILE / TM_;
  const int t_lin = bidx / ny;
  const int t128 = tile_base + t_lin / SUB_PER_PLAN_TILE;
  const int p128 = p.tile_order ? p.tile_order[t128] : ((int)(p.Vpad / PLAN_TILE) - 1 - t128);
  const int tile = p128 * SUB_PER_PLAN_TILE + (t_lin % SUB_PER_PLAN_TILE);
  const int n0 = (bidx % ny) * TN;
  const int64_t row0 = (int64_t)tile * TM_;
  const int li = lane & 15, lq = lane >> 4;
  const int K = p.K, Cin = p.Cin, Cout = p.Cout;
  const int col0 = n0 + wn * NT * 16 + NT * li;  // this lane's first output channel
  const bool cols_full = col0 + NT <= Cout;

  f32x4 acc[MR][NT];
#pragma unroll
  for (int s = 0; s < MR; ++s)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[s][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // ---- continue an earlier pass's chains: C operands from acc_init, addressed through `perm` like the epilogue's rows
  if (p.acc_init) {
    if constexpr (FAST) {
      const __amdgpu_buffer_rsrc_t rsrc_acc = __builtin_amdgcn_make_buffer_rsrc((void*)p.acc_init, 0, (int)p.acc_bytes, 0x00020000);
      int o_acc[MR][4];
      load_perm_rows<MR>(p, row0 + wm * MR * 16, lane >> 4, o_acc);
#pragma unroll
      for (int s = 0; s < MR; ++s)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const auto v = buffer_load_floats<NT>(
              rsrc_acc, o_acc[s][reg] >= 0 ? (uint32_t)o_acc[s][reg] * (uint32_t)(p.acc_ld * 4) + (uint32_t)col0 * 4u : BUF_ABSENT, 0u);
#pragma unroll
          for (int n = 0; n < NT; ++n) acc[s][n][reg] = v[n];
        }
    } else {
#pragma unroll
      for (int s = 0; s < MR; ++s)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int64_t r = row0 + wm * MR * 16 + s * 16 + (lane >> 4) * 4 + reg;
          const int64_t o = p.perm ? (int64_t)p.perm[r] : (r < p.V_out ? r : -1);
#pragma unroll
          for (int n = 0; n < NT; ++n) acc[s][n][reg] = (o >= 0 && col0 + n < Cout) ? p.acc_init[o * p.acc_ld + col0 + n] : 0.0f;
        }
    }
  }
  // ---- stage the tile's neighbour table (or the identity for dense rows) in LDS
  uint32_t dense_mask = (1u << SUBS) - 1u;
  if (p.submask == nullptr) {
    const int64_t rem = p.V_out - row0;
    const int nsub = rem >= TM_ ? SUBS : (int)((rem + 15) / 16);
    dense_mask = (1u << nsub) - 1u;
  }
  if constexpr (FAST) {
    // all of the thread's table entries are requested before the first is used (a rolled loop waits for each load in
    // turn); the table holds each row's BYTE offset in `in` (absent: beyond the buffer's extent -> zeros)
    constexpr int STAGE_IT = (32 * TM_ + 255) / 256;  // K <= 32
    int n_st[STAGE_IT];
#pragma unroll
    for (int it = 0; it < STAGE_IT; ++it) {
      const int e = tid + 256 * it;
      const int k = e / TM_, r = e % TM_;
      n_st[it] = -1;
      if (e < K * TM_) {
        if (p.nbr_s)
          n_st[it] = p.nbr_s[(int64_t)k * p.Vpad + row0 + r];
        else
          n_st[it] = (row0 + r < p.V_out) ? (int)(row0 + r) : -1;
      }
    }
#pragma unroll
    for (int it = 0; it < STAGE_IT; ++it) {
      const int e = tid + 256 * it;
      if (e < K * TM_) idx_s[e] = (int)(n_st[it] >= 0 ? (uint32_t)n_st[it] * (uint32_t)(p.in_ld * 4) : BUF_ABSENT);
    }
  } else {
    for (int e = tid; e < K * TM_; e += 256) {
      const int k = e / TM_, r = e - k * TM_;
      int n;
      if (p.nbr_s)
        n = p.nbr_s[(int64_t)k * p.Vpad + row0 + r];
      else
        n = (row0 + r < p.V_out) ? (int)(row0 + r) : -1;
      idx_s[e] = n;
    }
  }
  const __amdgpu_buffer_rsrc_t rsrc_in = __builtin_amdgcn_make_buffer_rsrc((void*)p.in, 0, (int)p.in_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, (int)p.w_bytes, 0x00020000);

  // ---- step iterator over (active offset, chunk).  The plan's submask words cover 128 rows = 8 sub-tiles; lane k of
  //      every wave keeps the tile's word for offset k in a register and a ballot gives the active-offset set, so
  //      stepping to the next active offset is a bit scan + v_readlane (no memory access between steps).
  const int64_t sm_word = row0 / PLAN_TILE;
  const int sm_shift = (int)((row0 % PLAN_TILE) / 16);
  uint32_t my_sm = 0;
  if (lane < K) my_sm = p.submask ? ((p.submask[sm_word * K + lane] >> sm_shift) & ((1u << SUBS) - 1u)) : dense_mask;
  const uint32_t amask = (uint32_t)__ballot(my_sm != 0);
  // fused-offset steps: a step starts at offset k0 = multiple of GK, its sub-tile mask is the union over its offsets
  auto fused_mask = [&](int k0) -> uint32_t {
    uint32_t m = 0;
#pragma unroll
    for (int g = 0; g < GK; ++g) m |= (uint32_t)__builtin_amdgcn_readlane((int)my_sm, min(k0 + g, 31));
    return m;  // lanes >= K hold 0
  };
  int k_n, c_n = 0;
  uint32_t sm_n = 0;
  bool have_n;
  if (CPO) {
    k_n = 0;
    while (k_n < K && (sm_n = fused_mask(k_n)) == 0) k_n += GK;
    have_n = k_n < K;
  } else {
    k_n = amask ? __builtin_ctz(amask) : K;
    sm_n = amask ? (uint32_t)__builtin_amdgcn_readlane((int)my_sm, k_n) : 0u;
    have_n = amask != 0;
  }
  auto advance = [&]() {
    if (CPO) {
      k_n += GK;
      while (k_n < K && (sm_n = fused_mask(k_n)) == 0) k_n += GK;
      have_n = k_n < K;
      return;
    }
    c_n += KC;
    if (c_n >= Cin) {
      c_n = 0;
      const uint32_t rest = amask & ~((2u << k_n) - 1u);
      have_n = rest != 0;
      k_n = have_n ? __builtin_ctz(rest) : K;
      sm_n = (uint32_t)__builtin_amdgcn_readlane((int)my_sm, have_n ? k_n : 0);
    }
  };

  // gathered rows in flight: the rows of step s + 1 are requested at the start of step s and written to LDS at its end.
  // (One step of look-ahead is enough: gather latency is not what a step waits for - two steps ahead cost the wide
  // layers a wave per SIMD)  The WIDE step moves them in two halves through ra[0] alone.
  float4 ra[A_F4];
  const int a_cc = (tid % Cfg::F4_PER_ROW) * 4;
  const int a_r = tid / Cfg::F4_PER_ROW;

  // FAST: this thread's column inside a chunk in bytes; in a partial last chunk, threads past Cin use minus the chunk's
  // start instead (voffset + soffset = the row's first columns)
  const uint32_t col_bytes = (uint32_t)a_cc * 4u;
  const int cin_rem = Cin % KC;
  const uint32_t col_last = (cin_rem == 0 || a_cc < cin_rem) ? col_bytes : 0u - (uint32_t)(Cin - cin_rem) * 4u;
  // gather_row: this thread's j-th float4 of step (k, c0)
  auto gather_row = [&](int k, int c0, uint32_t sm, int j) -> float4 {
    const int r = a_r + ROWS_PER_PASS * j;
    if (FAST) {
      // one ds_read (the row's byte offset), one add (this thread's column) and a buffer_load whose SGPR offset is the
      // step's channel chunk: rows past the tile (clamped), sub-tiles without a neighbour at this offset (all their
      // rows are absent) and absent neighbours need no test - the descriptor's range check returns zeros for them
      const int rr = (A_F4 * ROWS_PER_PASS > TM_) ? min(r, TM_ - 1) : r;
      if (CPO) {
        // fused offsets: column a_cc of the step belongs to offset k + a_cc / CPO, channel a_cc % CPO
        const int kk = k + a_cc / (CPO ? CPO : 1);
        uint32_t off = (uint32_t)idx_s[min(kk, K - 1) * TM_ + rr];
        if (kk >= K) off = BUF_ABSENT;
        const f32x4 v = buffer_load_floats<4>(rsrc_in, off + (uint32_t)(a_cc % (CPO ? CPO : 1)) * 4u, 0u);
        return make_float4(v[0], v[1], v[2], v[3]);
      } else {
        const uint32_t off = (uint32_t)idx_s[k * TM_ + rr];
        // the last chunk of a layer whose Cin is not a multiple of KC: columns past Cin are never multiplied; their
        // lanes re-read the row's first columns (col_last) so that no load reaches past a row
        const uint32_t cb = (!FULL && c0 + KC > Cin) ? col_last : col_bytes;
        const f32x4 v = buffer_load_floats<4>(rsrc_in, off + cb, (uint32_t)c0 * 4u);
        return make_float4(v[0], v[1], v[2], v[3]);
      }
      (void)sm;
    } else if (CPO) {
      float e[4] = {0.f, 0.f, 0.f, 0.f};
      if (r < TM_ && ((sm >> (r >> 4)) & 1u)) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = a_cc + q, kk = k + i / (CPO ? CPO : 1), c = i % (CPO ? CPO : 1);
          if (i < GK * CPO && kk < K) {
            const int n = idx_s[kk * TM_ + r];
            if (n >= 0) e[q] = p.in[(int64_t)n * p.in_ld + c];
          }
        }
      }
      return make_float4(e[0], e[1], e[2], e[3]);
    } else {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < TM_ && ((sm >> (r >> 4)) & 1u)) {
        const int n = idx_s[k * TM_ + r];
        const int c = c0 + a_cc;
        if (n >= 0) {
          const float* src = p.in + (int64_t)n * p.in_ld + c;
          if (p.vec_a) {
            if (c < Cin) v = *(const float4*)src;
          } else {
            if (c + 0 < Cin) v.x = src[0];
            if (c + 1 < Cin) v.y = src[1];
            if (c + 2 < Cin) v.z = src[2];
            if (c + 3 < Cin) v.w = src[3];
          }
        }
      }
      return v;
    }
  };
  auto load_a = [&](int k, int c0, uint32_t sm) {
#pragma unroll
    for (int j = 0; j < A_F4; ++j) ra[j] = gather_row(k, c0, sm, j);
  };
  auto scatter_row = [&](float* dstbuf, uint32_t sm, int j, const float4& v) {
    const int r = a_r + ROWS_PER_PASS * j;
    // FAST: rows of sub-tiles that are inactive at this offset arrive as zeros and are stored like the others (their
    // matrix ops are skipped anyway) - no per-row mask arithmetic in the loop (skipping their gathers and stores
    // measured -2 %)
    if (r < TM_ && (FAST || ((sm >> (r >> 4)) & 1u))) {
      float2* dst = (float2*)(dstbuf + r * SA + a_cc);
      dst[0] = make_float2(v.x, v.y);
      dst[1] = make_float2(v.z, v.w);
    }
  };
  auto store_a = [&](float* dstbuf, uint32_t sm) {
#pragma unroll
    for (int j = 0; j < A_F4; ++j) scatter_row(dstbuf, sm, j, ra[j]);
  };

  // B operands of one k-step: rows c0 + 4 ks + lq of W[k], NT consecutive output channels starting at col0.  Each
  // k-step's NT values are ONE register tuple (the destination of one global_load_dwordxNT): kept as a vector value the
  // loop carries it as a tuple, and the reload lands in the registers the next step's matrix ops read (as NT separate
  // floats the tuple was copied element by element at the loop back-edge, behind an s_waitcnt vmcnt(0))
  typedef float bvec_t __attribute__((ext_vector_type(NT)));
  typedef float bvec_load_t __attribute__((ext_vector_type(NT), aligned(4)));
  // WIDE: a ring of BR = 4 tuples - the reload after k-step ks fetches k-step ks + BR (of this step, or of the next one
  // once ks + BR passes the chunk), the same prefetch distance in matrix ops with half the registers of a whole chunk
  constexpr int KS = KC / 4;
  constexpr int BR = WIDE ? 4 : KS;
  bvec_t b[BR];
  // FAST: wstep = first weight row of the step (wave-uniform -> scalar registers), b_off = this lane's constant offset;
  // per k-step only a scalar add remains.  K-steps past the channel tail re-read row 0 of the step (never multiplied).
  const int b_off = lq * Cout + col0;
  const uint32_t b_off_bytes = (uint32_t)b_off * 4u;
  auto step_weights = [&](int k, int c0) -> const float* { return p.W + ((int64_t)k * Cin + c0) * Cout; };
  // valid A columns of the step starting at (k, c0): the rest of the chunk is zero padding
  auto cols_of = [&](int k, int c0) { return CPO ? min(GK, K - k) * CPO : min(KC, Cin - c0); };
  auto ksteps_of = [&](int k, int c0) { return (cols_of(k, c0) + 3) >> 2; };
  auto load_b = [&](const float* wstep, int k, int c0, int ksteps_valid, int ks, bvec_t& dst) {
    if (FAST) {
      // SGPR offset = the k-step's first weight row, VGPR offset = this lane's constant (row lq, column col0)
      const uint32_t row = (uint32_t)(k * Cin + c0 + (ks < ksteps_valid ? 4 * ks : 0));
      dst = buffer_load_floats<NT>(rsrc_w, b_off_bytes, row * (uint32_t)Cout * 4u);
      (void)wstep;
    } else {
      // W row of A column i of the step: (k * Cin + c0 + i) - fused offsets are consecutive row blocks of W
      const int i = 4 * ks + lq;
      const float* src = p.W + ((int64_t)k * Cin + c0 + i) * Cout + col0;
      const bool row_ok = i < cols_of(k, c0);
#pragma unroll
      for (int n = 0; n < NT; ++n) dst[n] = (row_ok && col0 + n < Cout) ? src[n] : 0.0f;
    }
  };

  __syncthreads();  // idx_s visible
  if (have_n) {
    // ---- prologue: operands of step 0 (c = the current step).  x = the step after c: a copy of the iterator (n) after
    //      every advance(), kept as loop state of its own - with the iterator read directly hipcc lays out the loop
    //      entry of every instance differently
    int k_c = k_n, c_c = c_n;
    uint32_t sm_c = sm_n;
    load_a(k_c, c_c, sm_c);
#pragma unroll
    for (int ks = 0; ks < BR; ++ks) load_b(step_weights(k_c, c_c), k_c, c_c, ksteps_of(k_c, c_c), ks, b[ks]);
    store_a(As, sm_c);
    advance();
    int k_x = k_n, c_x = c_n;
    uint32_t sm_x = sm_n;
    bool have_x = have_n;
    __syncthreads();
    int buf = 0;
    if (p.trace) trace_t_loop = wall_clock64();

    // one pipeline step
    auto step = [&]() -> bool {
      // ---- gathers of step x go out first: they land during matrix work and are written to the other LDS buffer
      //      at the end of this step.  (Issued here rather than after the barrier so that a conservative wait on the
      //      loop back-edge never waits for a gather that was just issued.)
      if (FAST || have_x) load_a(have_x ? k_x : 0, have_x ? c_x : 0, have_x ? sm_x : 0u);
      // ---- MFMA over the current step; A operand reads run one k-step ahead of the matrix ops; each k-step's B
      //      registers are refilled for step x as soon as the matrix ops that read them are issued
      const float* a_base = As + buf * (TM_ * SA) + (wm * MR * 16 + li) * SA + lq;
      const uint32_t smw = (sm_c >> (wm * MR)) & ((1u << MR) - 1u);
      const int ksteps = ksteps_of(k_c, c_c);
      const int kb = have_x ? k_x : 0;
      const int cb = have_x ? c_x : 0;
      const float* wnext = step_weights(kb, cb);
      const int ksteps_next = ksteps_of(kb, cb);
      // A operands run PFD k-steps ahead of the matrix ops (register ring when PFD > 1): one k-step of a small tile is
      // only MR * NT * 32 cycles of matrix work, less than an LDS round trip, and on the small pyramid levels a wave
      // has no co-resident wave to hide that latency behind.
      // FULL (every step uses all KC columns: Cin % KC == 0, chosen at launch): compile-time trip count and plain
      // weight-row addressing, i.e. no per-k-step compare / select / branch in the hot loop.
      {
        auto reload_b = [&](int ks) {
          if (FULL) {
            b[ks] = buffer_load_floats<NT>(rsrc_w, b_off_bytes, (uint32_t)(kb * Cin + cb + 4 * ks) * (uint32_t)Cout * 4u);
          } else if (FAST || have_x) {
            load_b(wnext, kb, cb, ksteps_next, ks, b[ks]);
          }
        };
        auto mfma_row = [&](int ks, const float (&a)[MR]) {
#pragma unroll
          for (int s = 0; s < MR; ++s) {
            // a tile with ONE sub-tile per wave row group is only visited for offsets where that sub-tile is active
            // (steps with an empty submask are skipped), so the test is compile-time true there
            if ((MR == 1 && Cfg::WAVES_M == 1) || ((smw >> s) & 1u)) {
#pragma unroll
              for (int n = 0; n < NT; ++n)
                acc[s][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[ks][n], acc[s][n], 0, 0, 0);
            }
          }
        };
        if constexpr (PFD == 1) {
          float a_cur[MR];
#pragma unroll
          for (int s = 0; s < MR; ++s) a_cur[s] = a_base[s * 16 * SA];
#pragma unroll
          for (int ks = 0; ks < KC / 4; ++ks) {
            if (FULL || ks < ksteps) {
              float a_nx[MR];
              if (ks + 1 < KC / 4) {
#pragma unroll
                for (int s = 0; s < MR; ++s) a_nx[s] = a_base[s * 16 * SA + (ks + 1) * 4];
                if (FULL) __builtin_amdgcn_sched_barrier(0);  // operand reads go out first
              }
              mfma_row(ks, a_cur);
              if (ks + 1 < KC / 4) {
#pragma unroll
                for (int s = 0; s < MR; ++s) a_cur[s] = a_nx[s];
              }
            }
            reload_b(ks);
            // straight-line code (FULL): keep the written interleaving of operand reads, matrix ops and weight reloads -
            // left alone, the scheduler batches the reloads behind all matrix ops and their latency is exposed
            if (FULL) __builtin_amdgcn_sched_barrier(0);
          }
        } else {
          float a_ring[PFD + 1][MR];
#pragma unroll
          for (int d = 0; d < PFD; ++d)
#pragma unroll
            for (int s = 0; s < MR; ++s) a_ring[d][s] = a_base[s * 16 * SA + d * 4];
#pragma unroll
          for (int ks = 0; ks < KC / 4; ++ks) {
            if (FULL || ks < ksteps) {
              if (ks + PFD < KC / 4) {
#pragma unroll
                for (int s = 0; s < MR; ++s)
                  a_ring[(ks + PFD) % (PFD + 1)][s] = a_base[s * 16 * SA + (ks + PFD) * 4];
                if (FULL) __builtin_amdgcn_sched_barrier(0);
              }
              mfma_row(ks, a_ring[ks % (PFD + 1)]);
            }
            reload_b(ks);
            if (FULL) __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
      ++trace_steps;
      if (!have_x) return false;
      // ---- hand over to step x
      store_a(As + (buf ^ 1) * (TM_ * SA), sm_x);
      k_c = k_x;
      c_c = c_x;
      sm_c = sm_x;
      advance();
      k_x = k_n;
      c_x = c_n;
      sm_x = sm_n;
      have_x = have_n;
      __syncthreads();
      buf ^= 1;
      return true;
    };
    // WIDE form of a step.  Same operands, same order of matrix ops; what differs is how long operands sit in registers:
    //   * weights: tuple ks % BR is refilled with k-step ks + BR right after the matrix ops of k-step ks;
    //   * gathers of step x in two halves through ONE float4: half 0 is requested at the start and written to the other
    //     LDS buffer after the first half of the k-steps, half 1 then takes its place and is written at the end.  Nobody
    //     reads the other buffer during a step (the barrier at its end hands it over), so the early write needs no
    //     synchronisation; in the last step of a tile it writes rows nobody will read.
    auto step_wide = [&]() -> bool {
      const int kb = have_x ? k_x : 0;
      const int cb = have_x ? c_x : 0;
      float* const a_next = As + (buf ^ 1) * (TM_ * SA);
      ra[0] = gather_row(kb, cb, 0u, 0);
      const float* a_base = As + buf * (TM_ * SA) + (wm * MR * 16 + li) * SA + lq;
      const uint32_t smw = (sm_c >> (wm * MR)) & ((1u << MR) - 1u);
      const int ksteps = ksteps_of(k_c, c_c);
      const int ksteps_next = ksteps_of(kb, cb);
      // first weight row of this step and of step x (k-steps past a channel tail re-read row 0 of their step)
      const uint32_t wrow_c = (uint32_t)(k_c * Cin + c_c);
      const uint32_t wrow_x = (uint32_t)(kb * Cin + cb);
      float a_cur[MR];
#pragma unroll
      for (int s = 0; s < MR; ++s) a_cur[s] = a_base[s * 16 * SA];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        if (ks < ksteps) {
          float a_nx[MR];
          if (ks + 1 < KS) {
#pragma unroll
            for (int s = 0; s < MR; ++s) a_nx[s] = a_base[s * 16 * SA + (ks + 1) * 4];
          }
#pragma unroll
          for (int s = 0; s < MR; ++s) {
            if ((smw >> s) & 1u) {
#pragma unroll
              for (int n = 0; n < NT; ++n)
                acc[s][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[s], b[ks % BR][n], acc[s][n], 0, 0, 0);
            }
          }
          if (ks + 1 < KS) {
#pragma unroll
            for (int s = 0; s < MR; ++s) a_cur[s] = a_nx[s];
          }
        }
        const int kn = ks + BR < KS ? ks + BR : ks + BR - KS;  // the k-step the ring slot holds next
        const uint32_t wrow = ks + BR < KS ? wrow_c + (uint32_t)(kn < ksteps ? 4 * kn : 0)
                                           : wrow_x + (uint32_t)(kn < ksteps_next ? 4 * kn : 0);
        b[ks % BR] = buffer_load_floats<NT>(rsrc_w, b_off_bytes, wrow * (uint32_t)Cout * 4u);
        if (ks == KS / 2 - 1) {
          scatter_row(a_next, 0u, 0, ra[0]);
          ra[0] = gather_row(kb, cb, 0u, 1);
        }
      }
      ++trace_steps;
      if (!have_x) return false;
      scatter_row(a_next, 0u, 1, ra[0]);
      k_c = k_x;
      c_c = c_x;
      sm_c = sm_x;
      advance();
      k_x = k_n;
      c_x = c_n;
      sm_x = sm_n;
      have_x = have_n;
      __syncthreads();
      buf ^= 1;
      return true;
    };
    if constexpr (WIDE) {
      while (step_wide()) {
      }
    } else {
      while (step()) {
      }
    }
  }

  if (p.trace) trace_t_epi = wall_clock64();
  // ---- epilogue: BN(eval)/bias -> residual -> activation -> store.  C/D map: MFMA col = lane&15, row = (lane>>4)*4+reg
  float sc[NT], sh[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const bool ok = col0 + n < Cout;
    sc[n] = (p.scale && ok) ? p.scale[col0 + n] : 1.0f;
    sh[n] = (p.shift && ok) ? p.shift[col0 + n] : 0.0f;
  }
  if constexpr (FAST) {
    epilogue_buffered<MR, NT>(p, acc, row0 + wm * MR * 16, lq, col0);
  } else
#pragma unroll
  for (int s = 0; s < MR; ++s) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t r = row0 + wm * MR * 16 + s * 16 + lq * 4 + reg;
      int64_t o;
      if (p.perm)
        o = p.perm[r];
      else
        o = (r < p.V_out) ? r : -1;
      if (o < 0) continue;
      float y[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        float v = acc[s][n][reg];
        if (p.scale)
          v = __builtin_fmaf(v, sc[n], sh[n]);
        else if (p.shift)
          v = v + sh[n];
        y[n] = v;
      }
      if (p.residual) {
        const float* res = p.residual + o * p.res_ld + col0;
#pragma unroll
        for (int n = 0; n < NT; ++n)
          if (col0 + n < Cout) y[n] = y[n] + res[n];
      }
      float* dst = p.out + o * p.out_ld + col0;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        float v = y[n];
        if (p.act == SV_ACT_RELU)
          v = v < 0.f ? 0.f : v;  // NaN stays NaN, as torch.relu
        else if (p.act == SV_ACT_LEAKY_RELU)
          v = v > 0.f ? v : v * p.slope;
        if (col0 + n < Cout) dst[n] = v;
      }
    }
  }
  if (p.trace && tid == 0) {  // 100 MHz wall clock; HW_REG_HW_ID (CU / SE) and HW_REG_XCC_ID place the workgroup
    unsigned long long* t = p.trace + (size_t)blockIdx.x * 4;
    t[0] = trace_t0;
    t[1] = wall_clock64();
    t[2] = ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) |
           (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);
    // steps | prologue (start -> first step) and epilogue-start offsets in 100 MHz ticks / 16 (experiments)
    const unsigned long long pro = trace_t_loop ? ((trace_t_loop - trace_t0) >> 4) & 0xffffull : 0ull;
    const unsigned long long epi = ((t[1] - trace_t_epi) >> 4) & 0xffffull;
    t[3] = (unsigned long long)(unsigned)trace_steps | (pro << 32) | (epi << 48);
  }
}

// resident waves per SIMD an instance is compiled for: five for the 64-row WIDE tile (alone or as the main body of the
// dual launch), no target of their own for the others
constexpr unsigned wide_waves(int tm, int waves_n, int nt, bool fast, int cpo, bool ring, bool full) {
  return (tm == 64 && waves_n == 4 && nt == 3 && fast && cpo == 0 && !ring && !full) ? 5u : 1u;
}

template <int TM_, int WAVES_N, int NT, bool FAST, int CPO = 0, bool RING = false, bool FULL = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(wide_waves(TM_, WAVES_N, NT, FAST, CPO, RING, FULL))))
void conv_fwd_kernel(ConvParams p) {
  conv_tile_body<TM_, WAVES_N, NT, FAST, CPO, RING, FULL>(p, (int)blockIdx.x, 0);
}

// Dual-body launch for chip-filling layers: the hardware hands out workgroups in blockIdx order, so the grid is the plan
// tiles in longest-first order as TM_-row tiles followed by the CHEAPEST plan tiles as TAIL_TM-row tiles.  A launch ends
// with every CU's residency decaying from 4 workgroups to 0 over about the duration of its last (cheapest) tiles; with
// half-height tiles at the end that decay is half as long (tools/wg_trace.py: ~22 % of a level-0 launch, i.e. ~11 % of
// its slot-time idle).  Everything else about a tile - offsets visited, the (k, c) order of every output element's fma
// chain, hence every result bit - is independent of the tile height.
template <int TM_, int TAIL_TM, int WAVES_N, int NT, bool FAST>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(wide_waves(TM_, WAVES_N, NT, FAST, 0, false, false))))
void conv_fwd_dual_kernel(ConvParams p) {
  if ((int)blockIdx.x < p.main_blocks)
    conv_tile_body<TM_, WAVES_N, NT, FAST>(p, (int)blockIdx.x, 0);
  else
    conv_tile_body<TAIL_TM, WAVES_N, NT, FAST>(p, (int)blockIdx.x - p.main_blocks, p.main_tiles128);
}

// Runs `launch()` (the kernel launch of a tile shape <tm, wn, nt> over `grid` workgroups with parameters q) and checks it.
// SV_CONV_TRACE=<file> (experiments only): trace the launch per workgroup, synchronise, append to <file>
// (tools/wg_trace.py reads it: residency over time, per-CU tail, time per step)
template <class Launch>
static int launch_traced(ConvParams& q, unsigned grid, int tm, int wn, int nt, hipStream_t stream, Launch&& launch) {
  static const char* trace_path = getenv("SV_CONV_TRACE");
  q.trace = nullptr;
  if (trace_path) SV_HIP(hipMalloc((void**)&q.trace, (size_t)grid * 4 * sizeof(unsigned long long)));
  launch();
  SV_LAUNCH_CHECK();
  if (q.trace) {
    std::vector<unsigned long long> host((size_t)grid * 4);
    SV_HIP(hipStreamSynchronize(stream));
    SV_HIP(hipMemcpy(host.data(), q.trace, host.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    SV_HIP(hipFree(q.trace));
    if (FILE* f = fopen(trace_path, "ab")) {
      const long long hdr[8] = {0x5356545243ll, (long long)grid, tm, wn, nt, q.ny, q.K, q.Cin};
      fwrite(hdr, sizeof(hdr), 1, f);
      fwrite(host.data(), sizeof(unsigned long long), host.size(), f);
      fclose(f);
    }
  }
  return SV_OK;
}

// launches tile <TM_, WAVES_N, NT, CPO> in the form the choice names (conv_tile_form)
template <int TM_, int WAVES_N, int NT, int CPO>
static int launch_conv(const ConvParams& p, hipStream_t stream, const ConvChoice& c) {
  using Cfg = ConvCfg<TM_, WAVES_N, NT, CPO>;
  ConvParams q = p;
  q.ntiles = (int)(p.Vpad / TM_);
  q.ny = (p.Cout + Cfg::TN - 1) / Cfg::TN;
  dim3 grid((unsigned)(q.ntiles * q.ny));
  constexpr bool F = (CPO % 4 == 0);  // odd channel counts (Cin = 3) only exist in the guarded form
  const size_t lds = Cfg::lds_bytes(p.K);
  return launch_traced(q, grid.x, TM_, WAVES_N, NT, stream, [&] {
    if (c.full) {
      if (c.ring)
        hipLaunchKernelGGL((conv_fwd_kernel<TM_, WAVES_N, NT, F, CPO, (Cfg::PFD > 1), (F && Cfg::USE_FULL)>), grid, dim3(256), lds, stream, q);
      else
        hipLaunchKernelGGL((conv_fwd_kernel<TM_, WAVES_N, NT, F, CPO, false, (F && Cfg::USE_FULL)>), grid, dim3(256), lds, stream, q);
    } else if (c.fast) {
      if (c.ring)
        hipLaunchKernelGGL((conv_fwd_kernel<TM_, WAVES_N, NT, F, CPO, (Cfg::PFD > 1)>), grid, dim3(256), lds, stream, q);
      else
        hipLaunchKernelGGL((conv_fwd_kernel<TM_, WAVES_N, NT, F, CPO, false>), grid, dim3(256), lds, stream, q);
    } else {
      if (c.ring)
        hipLaunchKernelGGL((conv_fwd_kernel<TM_, WAVES_N, NT, false, CPO, (Cfg::PFD > 1)>), grid, dim3(256), lds, stream, q);
      else
        hipLaunchKernelGGL((conv_fwd_kernel<TM_, WAVES_N, NT, false, CPO, false>), grid, dim3(256), lds, stream, q);
    }
  });
}

// dual-body launch (conv_fwd_dual_kernel): TM_-row tiles for the expensive plan tiles, TAIL_TM-row tiles for the cheapest
// c.tail128 of them (conv_select says when a layer qualifies)
template <int TM_, int TAIL_TM, int WAVES_N, int NT>
static int launch_conv_dual(const ConvParams& p, hipStream_t stream, const ConvChoice& c) {
  using Main = ConvCfg<TM_, WAVES_N, NT, 0>;
  using Tail = ConvCfg<TAIL_TM, WAVES_N, NT, 0>;
  ConvParams q = p;
  q.ny = p.Cout / Main::TN;
  q.main_tiles128 = (int)(p.Vpad / PLAN_TILE) - c.tail128;
  q.main_blocks = q.main_tiles128 * (PLAN_TILE / TM_) * q.ny;
  q.ntiles = (int)(p.Vpad / TM_);
  const unsigned grid = (unsigned)(q.main_blocks + c.tail128 * (PLAN_TILE / TAIL_TM) * q.ny);
  const size_t lds = Main::lds_bytes(p.K) > Tail::lds_bytes(p.K) ? Main::lds_bytes(p.K) : Tail::lds_bytes(p.K);
  return launch_traced(q, grid, TM_, WAVES_N, NT, stream, [&] {
    hipLaunchKernelGGL((conv_fwd_dual_kernel<TM_, TAIL_TM, WAVES_N, NT, true>), dim3(grid), dim3(256), lds, stream, q);
  });
}

// one launcher per row of CONV_TILES (sv_conv_select.h): the table IS the list of instantiations
typedef int (*ConvLauncher)(const ConvParams&, hipStream_t, const ConvChoice&);
template <size_t... I>
static constexpr std::array<ConvLauncher, sizeof...(I)> conv_launchers(std::index_sequence<I...>) {
  return {{&launch_conv<CONV_TILES[I].tm, CONV_TILES[I].wn, CONV_TILES[I].nt, CONV_TILES[I].cpo>...}};
}
static constexpr auto CONV_LAUNCHERS = conv_launchers(std::make_index_sequence<N_CONV_TILES>{});

// SV_CONV_FORCE* (experiments only) override WHICH tile a layer that reaches the lists runs on; its form stays
// conv_tile_form's.  True when a switch applies to the shape: `tile` is then the row of CONV_TILES, or -1 (error set) when
// the tile it names is not instantiated.
static bool forced_tile(const ConvShape& s, int& tile) {
  int tm = 0, wn = 0, nt = 0, cpo = 0, cout = 0;
  long long vmin = 0, vmax = 0;
  const char* f;
  bool hit = false;
  if ((f = getenv("SV_CONV_FORCE_RANGE")))  // "vmin:vmax:cout:tm,wn,nt": one level's layers only
    hit = sscanf(f, "%lld:%lld:%d:%d,%d,%d", &vmin, &vmax, &cout, &tm, &wn, &nt) == 6 && s.Vpad >= vmin && s.Vpad <= vmax &&
          s.Cout == cout && s.K > 1;
  if (!hit && (f = getenv("SV_CONV_FORCE_DENSE")))  // "vmin:cout:tm,wn,nt": dense (K = 1) layers of one width
    hit = sscanf(f, "%lld:%d:%d,%d,%d", &vmin, &cout, &tm, &wn, &nt) == 5 && s.Vpad >= vmin && s.Cout == cout && s.K == 1;
  if (!hit && (f = getenv("SV_CONV_FORCE")))  // "tm,wn,nt[,cpo]"
    hit = sscanf(f, "%d,%d,%d,%d", &tm, &wn, &nt, &cpo) >= 3;
  if (!hit) return false;
  tile = find_conv_tile(tm, wn, nt, cpo);
  if (tile < 0) set_error("sv_conv_fwd: no kernel instance <%d,%d,%d> cpo %d", tm, wn, nt, cpo);
  return true;
}

// the dispatch knobs a call on this thread uses now: sv_conv_set_dispatch's override, else the environment, else the default
static void effective_dispatch(double& want_scale, double& tail_fraction) {
  static const double env_want_scale =
      getenv("SV_CONV_WANT_SCALE") ? atof(getenv("SV_CONV_WANT_SCALE")) : SV_CONV_WANT_SCALE_DEFAULT;
  static const double env_tail = getenv("SV_CONV_TAIL") ? atof(getenv("SV_CONV_TAIL")) : SV_CONV_TAIL_DEFAULT;
  want_scale = g_want_scale_override >= 0.0 ? g_want_scale_override : env_want_scale;
  tail_fraction = g_tail_override >= 0.0 ? g_tail_override : env_tail;
}

static int launch_choice(const ConvChoice& c, const ConvParams& p, hipStream_t stream) {
  switch (c.kind) {
    case CONV_FIRST_MFMA: return launch_conv_first_mfma(p, stream);
    case CONV_FIRST_LAYER: return launch_conv_first_layer(p, stream);
    case CONV_THIN: return launch_conv_thin(p, stream);
    case CONV_THIN_LDS: return launch_conv_thin_lds(p, stream);
    case CONV_NARROW: return launch_linear_narrow(p, stream);
    case CONV_DUAL: return launch_conv_dual<64, 32, 4, 3>(p, stream, c);
    default: return CONV_LAUNCHERS[find_conv_tile(c.tm, c.wn, c.nt, c.cpo)](p, stream, c);
  }
}

}  // namespace sv

using namespace sv;

extern "C" const char* sv_conv_last_instance(void) { return sv::g_last_instance; }

extern "C" int sv_conv_set_dispatch(double want_scale, double tail_fraction) {
  SV_CHECK_ARG(tail_fraction < 1.0, "tail_fraction must be below 1");
  sv::g_want_scale_override = want_scale;
  sv::g_tail_override = tail_fraction;
  return SV_OK;
}

extern "C" int sv_conv_fwd(const float* in, int64_t V_in, int64_t in_ld, int Cin, const float* W, int K, int Cout,
                           const int32_t* perm, const int32_t* nbr_s, const uint32_t* submask,
                           const int32_t* tile_order, int64_t V_out, int64_t Vpad, const float* scale, const float* shift, const float* residual, int64_t res_ld,
                           int act, float slope, float* out, int64_t out_ld, sv_stream_t stream_) {
  return sv_conv_fwd_acc(in, V_in, in_ld, Cin, W, K, Cout, perm, nbr_s, submask, tile_order, V_out, Vpad, nullptr, 0, scale, shift,
                         residual, res_ld, act, slope, out, out_ld, stream_);
}

extern "C" int sv_conv_fwd_acc(const float* in, int64_t V_in, int64_t in_ld, int Cin, const float* W, int K, int Cout,
                               const int32_t* perm, const int32_t* nbr_s, const uint32_t* submask, const int32_t* tile_order,
                               int64_t V_out, int64_t Vpad, const float* acc_init, int64_t acc_ld, const float* scale,
                               const float* shift, const float* residual, int64_t res_ld, int act, float slope, float* out,
                               int64_t out_ld, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(!acc_init || acc_ld >= Cout, "acc_init stride too small");
  SV_CHECK_ARG(Cin > 0 && Cout > 0 && K >= 1 && K <= 32, "bad channel / kernel volume");
  SV_CHECK_ARG(V_out >= 0 && Vpad >= V_out && Vpad % PLAN_TILE == 0, "Vpad must be a multiple of 128 >= V_out");
  SV_CHECK_ARG(in_ld >= Cin && out_ld >= Cout, "row strides too small");
  SV_CHECK_ARG(act >= SV_ACT_NONE && act <= SV_ACT_LEAKY_RELU, "bad activation");
  if (V_out == 0) return SV_OK;
  SV_CHECK_ARG(in && W && out, "null pointer");
  SV_CHECK_ARG(V_in >= 1, "V_in = rows of `in` (every index of the plan is below it)");
  const bool has_plan = perm || nbr_s || submask;
  SV_CHECK_ARG(!has_plan || (perm && nbr_s && submask), "perm, nbr_s and submask must be given together");
  SV_CHECK_ARG(has_plan || K == 1, "K > 1 needs a plan");
  SV_CHECK_ARG(!residual || res_ld >= Cout, "residual stride too small");
  ConvParams p;
  p.in = in; p.in_ld = in_ld; p.Cin = Cin; p.W = W; p.K = K; p.Cout = Cout;
  p.perm = perm; p.nbr_s = nbr_s; p.submask = submask; p.tile_order = tile_order; p.V_out = V_out; p.Vpad = Vpad;
  p.scale = scale; p.shift = shift; p.residual = residual; p.res_ld = res_ld;
  p.acc_init = acc_init; p.acc_ld = acc_ld;
  p.act = act; p.slope = slope; p.out = out; p.out_ld = out_ld;
  p.vec_a = (in_ld % 4 == 0) && (Cin % 4 == 0) && (((uintptr_t)in & 15) == 0);
  // extents for the buffer descriptors of the FAST instances: `in` through the last channel of its last row
  const uint64_t in_bytes = ((uint64_t)(V_in - 1) * (uint64_t)in_ld + (uint64_t)Cin) * 4u;
  const uint64_t w_bytes = (uint64_t)K * (uint64_t)Cin * (uint64_t)Cout * 4u;
  const uint64_t out_bytes = ((uint64_t)(V_out - 1) * (uint64_t)out_ld + (uint64_t)Cout) * 4u;
  const uint64_t res_bytes = residual ? ((uint64_t)(V_out - 1) * (uint64_t)res_ld + (uint64_t)Cout) * 4u : 0u;
  const uint64_t acc_bytes = acc_init ? ((uint64_t)(V_out - 1) * (uint64_t)acc_ld + (uint64_t)Cout) * 4u : 0u;
  // (the buffer-addressed epilogue reads `perm` four entries at a time: a plan carved from a workspace at an odd offset
  //  takes the guarded form)
  p.buf_ok = in_bytes < BUF_LIMIT && w_bytes < BUF_LIMIT && out_bytes < BUF_LIMIT && res_bytes < BUF_LIMIT &&
             acc_bytes < BUF_LIMIT && (((uintptr_t)perm & 15) == 0);
  p.acc_bytes = p.buf_ok ? (uint32_t)acc_bytes : 0u;
  if (!p.buf_ok && !has_plan && K == 1 && w_bytes < BUF_LIMIT) {
    // dense rows (Linear / 1x1 conv) of a tensor beyond the 2 GB extent: every row range is a layer of its own, so the
    // launch is split into ranges that fit the buffer-addressed instances (64 Cfg-2 frames x 1024 channels = 23 GB)
    int64_t ld_max = in_ld > out_ld ? in_ld : out_ld;
    if (residual && res_ld > ld_max) ld_max = res_ld;
    const int64_t rows = (int64_t)((BUF_LIMIT - 4096u) / ((uint64_t)ld_max * 4u)) / PLAN_TILE * PLAN_TILE;
    if (rows >= PLAN_TILE && rows < V_out) {
      for (int64_t r0 = 0; r0 < V_out; r0 += rows) {
        const int64_t n = V_out - r0 < rows ? V_out - r0 : rows;
        const int rc = sv_conv_fwd_acc(in + r0 * in_ld, n, in_ld, Cin, W, K, Cout, nullptr, nullptr, nullptr, nullptr, n,
                                       (n + PLAN_TILE - 1) / PLAN_TILE * PLAN_TILE, acc_init ? acc_init + r0 * acc_ld : nullptr,
                                       acc_ld, scale, shift, residual ? residual + r0 * res_ld : nullptr, res_ld, act, slope,
                                       out + r0 * out_ld, out_ld, stream_);
        if (rc != SV_OK) return rc;
      }
      return SV_OK;
    }
  }
  p.in_bytes = p.buf_ok ? (uint32_t)in_bytes : 0u;
  p.w_bytes = p.buf_ok ? (uint32_t)w_bytes : 0u;
  p.out_bytes = p.buf_ok ? (uint32_t)out_bytes : 0u;
  p.res_bytes = p.buf_ok ? (uint32_t)res_bytes : 0u;
  p.ntiles = 0;
  p.ny = 0;
  p.trace = nullptr;
  p.main_blocks = 0;
  p.main_tiles128 = 0;
  const ConvShape shape = {K, Cin, Cout, Vpad, has_plan, tile_order != nullptr, p.vec_a != 0, p.buf_ok != 0, acc_init != nullptr,
                           ((uintptr_t)W & 15) == 0, g_want_scale_override >= 1.0};
  double want_scale, tail_fraction;
  effective_dispatch(want_scale, tail_fraction);
  ConvChoice c = conv_select(shape, want_scale, tail_fraction);
  int forced;
  if ((c.kind == CONV_TILE || c.kind == CONV_DUAL) && forced_tile(shape, forced)) {
    if (forced < 0) return SV_ERR_INVALID;
    c = conv_tile_form(CONV_TILES[forced], shape);
  }
  const int rc = launch_choice(c, p, stream);
  if (rc == SV_OK) conv_choice_name(c, g_last_instance, sizeof(g_last_instance));
  return rc;
}

extern "C" int sv_conv_select(int64_t n, const int64_t* shapes_host, double want_scale, double tail_fraction, char* names_host,
                              size_t name_bytes) {
  SV_CHECK_ARG(n >= 0 && (n == 0 || (shapes_host && names_host)) && name_bytes > 0, "null pointer");
  SV_CHECK_ARG(tail_fraction < 1.0, "tail_fraction must be below 1");
  double ws, tf;
  effective_dispatch(ws, tf);
  const bool alone = want_scale >= 0.0 ? want_scale >= 1.0 : g_want_scale_override >= 1.0;
  if (want_scale >= 0.0) ws = want_scale;
  if (tail_fraction >= 0.0) tf = tail_fraction;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t* s = shapes_host + 5 * i;
    const int64_t K = s[0], Cin = s[1], Cout = s[2], Vpad = s[3], flags = s[4];
    SV_CHECK_ARG(Cin > 0 && Cin <= INT32_MAX && Cout > 0 && Cout <= INT32_MAX && K >= 1 && K <= 32, "bad channel / kernel volume");
    SV_CHECK_ARG(Vpad > 0 && Vpad % PLAN_TILE == 0, "Vpad must be a positive multiple of 128");
    SV_CHECK_ARG((flags & SV_CONV_SEL_PLAN) || K == 1, "K > 1 needs a plan");
    SV_CHECK_ARG(!(flags & SV_CONV_SEL_VEC_A) || Cin % 4 == 0, "float4 gathers need Cin % 4 == 0");
    const ConvShape shape = {(int)K, (int)Cin, (int)Cout, Vpad, (flags & SV_CONV_SEL_PLAN) != 0, (flags & SV_CONV_SEL_TILE_ORDER) != 0,
                             (flags & SV_CONV_SEL_VEC_A) != 0, (flags & SV_CONV_SEL_BUF_OK) != 0, (flags & SV_CONV_SEL_ACC_INIT) != 0,
                             (flags & SV_CONV_SEL_W_ALIGNED) != 0, alone};
    conv_choice_name(conv_select(shape, ws, tf), names_host + (size_t)i * name_bytes, name_bytes);
  }
  return SV_OK;
}

extern "C" int sv_conv_tile_info(int index, int* out_host) {
  SV_CHECK_ARG(index >= 0 && index < N_CONV_TILES, "no such row of the tile table");
  SV_CHECK_ARG(out_host, "null pointer");
  const ConvTile& t = CONV_TILES[index];
  const int row[10] = {t.tm, t.wn, t.nt, t.cpo, t.mr, t.tn, t.gk, t.kc, t.pfd, (int)t.use_full};
  for (int i = 0; i < 10; ++i) out_host[i] = row[i];
  return SV_OK;
}
