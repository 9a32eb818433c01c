// Special-shape kernels of sv_conv_fwd and their launchers: the narrow-output linear layer, the thin 32 -> 32 layers (one
// wave per sub-tile, weights through L1 or resident in LDS) and the first layer (3 -> 32) on the matrix pipe and on the VALU.
// Same accumulation order (k ascending, c ascending) and epilogue as the tiled kernel of sv_conv.hip, hence the same bits.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

#include "sv_conv_params.h"

namespace sv {

// ---- narrow-output dense layer (K = 1, identity rows, Cout <= 4: the last Linear of the classification heads,
//      model/robotnet_segmentation.py:43-48).  1.5 flop per byte: an HBM stream, not a matrix problem - on the MFMA
//      tiles 13 of 16 output columns would be padding and the step chain (gather -> LDS -> barrier) is latency-bound.
//      Here a workgroup streams ROWS (64) rows: [ROWS x 32 channels] stages are read coalesced (8 lanes per 128-byte row
//      segment), double-buffered through LDS (row stride 33 words: conflict-free), and thread r walks row r with the
//      same ascending-channel fmaf chain as everywhere else (weights are wave-uniform -> scalar loads).
constexpr int NARROW_ROWS = 64;  // 256 / 128 / 64 / 32 rows: 3.2 / 3.6 / 3.9 / 2.8 TB/s on 88k x 1024 -> 3
template <int C>
__global__ __launch_bounds__(256) void linear_narrow_kernel(ConvParams p) {
  constexpr int ROWS = NARROW_ROWS, COLS = 32, SW = COLS + 1, LPT = ROWS / 32;  // LPT float4 loads per thread and stage
  __shared__ float tile[2][ROWS * SW];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * ROWS;
  const int Cin = p.Cin;
  const int lr = tid >> 3, lc = (tid & 7) * 4;  // load mapping: row lr + 32 i, channels lc .. lc + 3
  float4 ra[LPT];
  auto load = [&](int c0) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int64_t r = row0 + lr + 32 * i;
      const int c = c0 + lc;
      const bool ok = r < p.V_out && c < Cin;
      const float4 v = *(const float4*)(p.in + (ok ? r * p.in_ld + c : 0));
      ra[i] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto store = [&](float* dst) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      float* d = dst + (lr + 32 * i) * SW + lc;
      d[0] = ra[i].x;
      d[1] = ra[i].y;
      d[2] = ra[i].z;
      d[3] = ra[i].w;
    }
  };
  float acc[C];
#pragma unroll
  for (int j = 0; j < C; ++j) acc[j] = 0.0f;
  load(0);
  store(tile[0]);
  __syncthreads();
  int buf = 0;
  for (int c0 = 0; c0 < Cin; c0 += COLS) {
    const bool more = c0 + COLS < Cin;
    if (more) load(c0 + COLS);
    if (tid < ROWS) {
      const float* x = tile[buf] + tid * SW;
      const float* w = p.W + (int64_t)c0 * p.Cout;
      const int nc = min(COLS, Cin - c0);  // channels beyond Cin hold zeros, but their weights would be out of bounds
#pragma unroll 8
      for (int c = 0; c < nc; ++c) {
        const float xv = x[c];
#pragma unroll
        for (int j = 0; j < C; ++j) acc[j] = __builtin_fmaf(xv, w[c * p.Cout + j], acc[j]);
      }
    }
    if (more) store(tile[buf ^ 1]);
    __syncthreads();
    buf ^= 1;
  }
  const int64_t r = row0 + tid;
  if (tid >= ROWS || r >= p.V_out) return;
#pragma unroll
  for (int j = 0; j < C; ++j) {
    float v = acc[j];
    if (p.scale)
      v = __builtin_fmaf(v, p.scale[j], p.shift ? p.shift[j] : 0.0f);
    else if (p.shift)
      v = v + p.shift[j];
    if (p.residual) v = v + p.residual[r * p.res_ld + j];
    if (p.act == SV_ACT_RELU)
      v = v < 0.f ? 0.f : v;  // NaN stays NaN, as torch.relu
    else if (p.act == SV_ACT_LEAKY_RELU)
      v = v > 0.f ? v : v * p.slope;
    p.out[r * p.out_ld + j] = v;
  }
}

// ---- thin gather-bound layers (Cin = 32 -> Cout = 32: block1's four convs, conv1p1s2, conv2p2s2;
//      model/backbone/minkunet.py:59-71).  14 flop per gathered byte: the layer is its gather, and a tile's life in the
//      LDS-staged kernel above is a chain of dependent round trips (neighbour table -> barrier -> gather -> LDS -> barrier,
//      then one gather per step).  Here ONE WAVE owns a 16-row sub-tile and never synchronises with anybody:
//        * the sub-tile's active offsets are compacted into a list (ballot over the plan's submask words);
//        * per active offset every lane gathers the CIN channels of ITS row straight into registers - lane (row li,
//          group lq) loads float4s at channels 16 j + 4 lq .. + 3 - with D offsets in flight (register ring);
//        * the matrix op wants lane group lq to hold channel 4 m + lq for op m: a 4 x 4 transpose between the four lane
//          groups and four registers, done with two v_permlane32_swap + two v_permlane16_swap per float4 (gfx950), so
//          the accumulation chain keeps its (offset ascending, channel ascending) order and every bit of the result;
//        * weights (wave-uniform per offset, 4 KB) come from L1/L2 one offset ahead.
//      No LDS traffic for the features, no barrier, D gathers in flight per wave from its first microsecond on.
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void transpose4x4_lanegroups(float& r0, float& r1, float& r2, float& r3) {
  // in: lane group g (16 lanes) holds X[g][i] in r_i; out: lane group g holds X[i][g] in r_i
  u32x2_t a = __builtin_amdgcn_permlane32_swap(__float_as_uint(r0), __float_as_uint(r2), false, false);
  u32x2_t b = __builtin_amdgcn_permlane32_swap(__float_as_uint(r1), __float_as_uint(r3), false, false);
  u32x2_t c = __builtin_amdgcn_permlane16_swap(a.x, b.x, false, false);
  u32x2_t d = __builtin_amdgcn_permlane16_swap(a.y, b.y, false, false);
  r0 = __uint_as_float(c.x);
  r1 = __uint_as_float(c.y);
  r2 = __uint_as_float(d.x);
  r3 = __uint_as_float(d.y);
}

template <int CIN, int COUT, int MR, int D, int CSPLIT = 1>
__global__ __launch_bounds__(256) void conv_thin_kernel(ConvParams p) {
  // CSPLIT > 1: blockIdx.y selects a slice of COUT / CSPLIT output channels (the gathers are repeated per slice - they hit
  // the L2 - but a wave's matrix work and weight registers shrink by CSPLIT and the launch has CSPLIT times the waves: on
  // the small pyramid levels a launch is a few waves per SIMD, bound by one wave's chain of offsets)
  constexpr int NT = COUT / 16 / CSPLIT;  // MFMA column tiles per wave; interleaved: column li of tile n = channel NT * li + n
  const int cbase = (int)blockIdx.y * (COUT / CSPLIT);
  constexpr int KS = CIN / 4;    // k-steps per offset
  constexpr int G4 = CIN / 16;   // float4 gathers per lane, row and offset
  // MR: 16-row sub-tiles per wave (they share every weight register: half the weight traffic per row at MR = 2);
  // D: offsets in flight per wave (gather ring)
  static_assert(CIN % 16 == 0 && COUT % 16 == 0 && NT >= 1 && NT <= 4 && (MR == 1 || MR == 2), "shape");
  typedef float bvec_t __attribute__((ext_vector_type(NT)));
  __shared__ int idx_s[4][32 * 16 * MR];
  __shared__ int klist_s[4][32];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, lq = lane >> 4;
  const int K = p.K;
  constexpr int ROWS = 16 * MR;
  // (giving every XCD a contiguous eighth of the plan, for L2 locality of the gathers, measured no different: 24 vs 25 us
  //  at level 1, 53 vs 49 us at level 0)
  const int64_t row0 = ((int64_t)blockIdx.x * 4 + wid) * ROWS;  // Vpad is a multiple of 128: every wave has its rows
  const int64_t t128 = row0 / PLAN_TILE;
  const int sub = (int)((row0 % PLAN_TILE) / 16);
  // ---- active offsets of this wave's sub-tile(s), compacted; neighbour rows of its rows for every offset
  int o_pre[MR][4];
  load_perm_rows<MR>(p, row0, lq, o_pre);
  const bool active = lane < K && ((p.submask[t128 * K + lane] >> sub) & ((1u << MR) - 1u));
  const unsigned long long amask = __ballot(active);
  const int nact = __popcll(amask);
  if (active) klist_s[wid][__popcll(amask & ((1ull << lane) - 1ull))] = lane;
  // the wave's neighbour table: all entries requested before the first is stored (a rolled loop is a chain of K / 4
  // dependent round trips - a third of this kernel's life at level 1), kept as BYTE offsets of the rows in `in`
  // (absent: beyond the extent, the gather then returns zeros)
  {
    constexpr int ST = 32 * ROWS / 64;  // K <= 32
    int n_st[ST];
#pragma unroll
    for (int it = 0; it < ST; ++it) {
      const int e = lane + 64 * it;
      n_st[it] = e < K * ROWS ? p.nbr_s[(int64_t)(e / ROWS) * p.Vpad + row0 + (e % ROWS)] : -1;
    }
#pragma unroll
    for (int it = 0; it < ST; ++it) {
      const int e = lane + 64 * it;
      if (e < K * ROWS) idx_s[wid][e] = (int)(n_st[it] >= 0 ? (uint32_t)n_st[it] * (uint32_t)(p.in_ld * 4) : BUF_ABSENT);
    }
  }
  __builtin_amdgcn_wave_barrier();  // same-wave LDS traffic is ordered; keep the compiler from moving reads above
  const __amdgpu_buffer_rsrc_t rsrc_in = __builtin_amdgcn_make_buffer_rsrc((void*)p.in, 0, (int)p.in_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, (int)p.w_bytes, 0x00020000);

  f32x4 acc[MR][NT];
#pragma unroll
  for (int s = 0; s < MR; ++s)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[s][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float4 g[D][MR][G4];
  bvec_t b[2][KS];
  // Every load below is unconditional (slots past the end of the list re-read the last offset's weights and read zeros
  // through the range check, their matrix ops then add fma(0, w, acc) = acc): straight-line code, so hipcc can count its
  // s_waitcnt vmcnt instead of draining the ring at every control-flow merge.
  const int last = nact > 0 ? nact - 1 : 0;
  auto offset_of = [&](int j) { return __builtin_amdgcn_readfirstlane(klist_s[wid][min(j, last)]); };
  auto issue = [&](int j, float4 (&dst)[MR][G4]) {
    const int k = offset_of(j);
#pragma unroll
    for (int s = 0; s < MR; ++s) {
      // an absent neighbour (and a ring slot past the end of the list) reads beyond the buffer's extent: zeros from the
      // range check, no select behind the load (with `ok ? value : 0` hipcc sinks the load under the condition)
      const uint32_t off = j < nact ? (uint32_t)idx_s[wid][k * ROWS + s * 16 + li] : BUF_ABSENT;
#pragma unroll
      for (int jj = 0; jj < G4; ++jj) {
        const f32x4 v = buffer_load_floats<4>(rsrc_in, off + 16u * (uint32_t)lq, 64u * (uint32_t)jj);
        dst[s][jj] = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  };
  auto load_w = [&](int j, bvec_t (&dst)[KS]) {
    const uint32_t wk = (uint32_t)offset_of(j) * (uint32_t)(CIN * COUT * 4);  // wave-uniform: the SGPR offset
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      dst[ks] = buffer_load_floats<NT>(rsrc_w, (uint32_t)(lq * COUT + cbase + NT * li) * 4u, wk + (uint32_t)(4 * ks * COUT * 4));
  };
  auto compute = [&](float4 (&a)[MR][G4], bvec_t (&w)[KS]) {
#pragma unroll
    for (int jj = 0; jj < G4; ++jj) {
      float am[MR][4];
#pragma unroll
      for (int s = 0; s < MR; ++s) {
        am[s][0] = a[s][jj].x; am[s][1] = a[s][jj].y; am[s][2] = a[s][jj].z; am[s][3] = a[s][jj].w;
        transpose4x4_lanegroups(am[s][0], am[s][1], am[s][2], am[s][3]);  // [m]: channel 16 jj + 4 m + lq of row li
      }
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int s = 0; s < MR; ++s)
#pragma unroll
          for (int n = 0; n < NT; ++n)
            acc[s][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(am[s][m], w[4 * jj + m][n], acc[s][n], 0, 0, 0);
    }
  };
  if (nact > 0) {
#pragma unroll
    for (int d = 0; d < D; ++d) issue(d, g[d]);
    load_w(0, b[0]);
    constexpr int U = (D % 2 == 0) ? D : 2 * D;  // unroll so that ring slot and weight buffer indices are static
    for (int j0 = 0; j0 < nact; j0 += U) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = j0 + u;
        load_w(j + 1, b[(u + 1) & 1]);
        compute(g[u % D], b[u & 1]);
        issue(j + D, g[u % D]);
      }
    }
  }
  // ---- epilogue (shared with conv_tile_body): C/D map: MFMA col = lane & 15, row = (lane >> 4) * 4 + reg
  epilogue_buffered<MR, NT, true>(p, acc, row0, lq, cbase + NT * li, o_pre);
}

// ---- first layer on the matrix pipe (conv0: 3 -> 32, every voxel of the frame; model/backbone/minkunet.py:55-57).
//      The 27 x 3 = 81 (offset, channel) products of an output element are ONE ascending chain, so the layer is a
//      [V x 81] x [81 x 32] product whose A rows are gathered: 21 k-steps of 4 (the last three columns read zeros).  One
//      wave owns a 16-row sub-tile and never synchronises with anybody: lane (row li, group lq) fetches element
//      e = 4 ks + lq of its row - channel e % 3 of the neighbour at offset e / 3 - for all 21 k-steps at once (21 dword
//      gathers in flight per lane behind ONE round trip for the wave's neighbour table), the 81 x 32 weights arrive in the
//      matrix-op layout straight from L2 meanwhile (requested before the table), then 42 matrix ops.  Against the
//      thread-per-voxel VALU kernel: 5.4 instead of 1.3 waves per SIMD and 1 344 instead of 2 592 issue cycles per 16 rows.
//      Same chain order (k ascending, c ascending), absent neighbours contribute fma(0, w, acc) = acc.
template <int COUT>
__global__ __launch_bounds__(256) void conv_first_mfma_kernel(ConvParams p) {
  constexpr int CIN = 3, KMAX = 27, E = KMAX * CIN, KS = (E + 3) / 4, NT = COUT / 16;
  constexpr int SX = 85;  // LDS row stride of the gathered [16 rows][81] block: 85 = 21 mod 32 spreads the rows over the banks
  constexpr int PAIRS = KMAX * 16, IT = (PAIRS + 63) / 64;
  typedef float bvec_t __attribute__((ext_vector_type(NT)));
  __shared__ float xs[4][16 * SX];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, lq = lane >> 4;
  const int K = p.K;
  const __amdgpu_buffer_rsrc_t rsrc_in = __builtin_amdgcn_make_buffer_rsrc((void*)p.in, 0, (int)p.in_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, (int)p.w_bytes, 0x00020000);
  // weights first: they depend on nothing.  Row e of the flat [K * 3][COUT] weight block; rows past the extent (e >= 3 K)
  // read zeros through the range check
  bvec_t b[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
    b[ks] = buffer_load_floats<NT>(rsrc_w, (uint32_t)(lq * COUT + NT * li) * 4u, (uint32_t)(4 * ks * COUT * 4));
  // A workgroup of this kernel lives ~1.7 us, and the chip starts only ~126 of them per microsecond (PMC: 0.8 waves per SIMD
  // on average at 5 542 workgroups): a launch of one workgroup per 64 rows is bound by the dispatcher, not by its memory
  // chain.  So the grid is capped and every wave walks several sub-tiles (64-row groups blockIdx.x, + gridDim.x, ...) with
  // its weights loaded once; the LDS block is the wave's own and same-wave LDS traffic is ordered.
  const int ngroups = (int)(p.Vpad / 64);
  for (int grp = (int)blockIdx.x; grp < ngroups; grp += (int)gridDim.x) {
  const int64_t row0 = ((int64_t)grp * 4 + wid) * 16;  // Vpad is a multiple of 128: every wave has its rows
  int o_pre[1][4];
  load_perm_rows<1>(p, row0, lq, o_pre);
  // the wave's 27 x 16 (offset, row) pairs, one per lane and pass: consecutive lanes = consecutive rows of one offset, so
  // the index reads are coalesced, and each pair is ONE 12-byte gather (a third of the requests of per-element gathers:
  // at four frames per tensor the per-element form was bound by the texture addresser, 0.32 of the HBM peak)
  int n_st[IT];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int pr = lane + 64 * it;
    n_st[it] = (pr < K * 16) ? p.nbr_s[(int64_t)(pr >> 4) * p.Vpad + row0 + (pr & 15)] : -1;
  }
  typedef float f32x3 __attribute__((ext_vector_type(3)));
  f32x3 g[IT];
#pragma unroll
  for (int it = 0; it < IT; ++it)
    g[it] = buffer_load_floats<3>(rsrc_in, n_st[it] >= 0 ? (uint32_t)n_st[it] * (uint32_t)(p.in_ld * 4) : BUF_ABSENT, 0u);
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int pr = lane + 64 * it;
    if (pr < PAIRS) {
      float* d = &xs[wid][(pr & 15) * SX + 3 * (pr >> 4)];
      d[0] = g[it][0];
      d[1] = g[it][1];
      d[2] = g[it][2];
    }
  }
  __builtin_amdgcn_wave_barrier();  // same-wave LDS traffic is ordered; keep the compiler from moving reads above
  float a[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int e = 4 * ks + lq;
    a[ks] = e < E ? xs[wid][li * SX + e] : 0.0f;
  }
  f32x4 acc[1][NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[0][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[0][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ks], b[ks][n], acc[0][n], 0, 0, 0);
  epilogue_buffered<1, NT, true>(p, acc, row0, lq, NT * li, o_pre);
  }
}

// ---- the thin layers with the layer's WHOLE weight tensor resident in LDS (round 4; conv_thin_kernel above stays the
//      choice inside the frame pipeline, see launch_conv_thin).  What the counters said about conv_thin_kernel at 88k voxels (profiles/r04_pmc_thin_*.txt):
//      matrix pipe 29 % busy, waves 66 % of their life stalled at issue, and the CU's vector-memory pipe (TCP) handling
//      17.4 M cache accesses per launch = 68 k cycles per CU of a 110 k-cycle launch - two thirds of them WEIGHT loads: every
//      wave fetched the 4 KB weight block of every offset it visited through L1 (251 MB per launch for a 110 KB tensor),
//      and a wave alone on its SIMD waited an L2 round trip per offset for them (one offset of look-ahead is shorter).
//      27 x 32 x 32 floats are 110 KB: they fit the CU's 160 KB LDS beside the waves' neighbour tables.  So: ONE workgroup
//      of 16 waves per CU stages the weights once (coalesced float4, ~1 us), then every wave walks 16-row sub-tiles
//      (longest plan tiles first, wave w of workgroup b takes sub-tiles b + G w, b + G (w + 16), ...) exactly as
//      conv_thin_kernel does - compacted offset list, D gathers in flight, lane-group transposes, the (k, c) chain order
//      and therefore every result bit - with its B operands read from LDS (one conflict-free ds_read_b64 per k-step) and
//      only the row gathers left on the vector-memory path.
template <int CIN, int COUT, int D, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void conv_thin_lds_kernel(ConvParams p, int n_sub) {
  constexpr int NT = COUT / 16, KS = CIN / 4, G4 = CIN / 16;
  constexpr int ST = 32 * 16 / 64;  // table entries per lane (K <= 32)
  static_assert(CIN % 16 == 0 && COUT % 16 == 0 && NT >= 1 && NT <= 4, "shape");
  typedef float bvec_t __attribute__((ext_vector_type(NT)));
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ int q_head;  // the workgroup's tile queue: next unassigned position of its tile list
  const int K = p.K;
  float* w_s = lds;                                     // [K][CIN][COUT]
  int* idx_all = (int*)(lds + (size_t)K * CIN * COUT);  // [WAVES][32 * 16] neighbour rows of a wave's sub-tile (byte offsets)
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lq = lane >> 4;
  // SV_THIN_TRACE experiments: per-wave cycle stamps {start, weights staged, first tile: table staged / loop done / stored,
  // end, tiles, offsets of the first tile}
  unsigned long long tr[6] = {0, 0, 0, 0, 0, 0}, tr_it[3] = {0, 0, 0};
  int tr_tiles = 0, tr_nact = 0;
  if (p.trace) tr[0] = __builtin_amdgcn_s_memtime();
  if (tid == 0) q_head = WAVES;  // positions 0 .. WAVES-1 are the waves' first tiles
  // The workgroup's tile list: position i = sub-tile blockIdx.x + gridDim.x * i in LONGEST-FIRST order (plan tile
  // tile_order[t / 8], its sub-tile t % 8): every workgroup gets the same mix of long and short tiles; inside the workgroup
  // the waves PULL positions from q_head (an LDS atomic: no global counter to reset), so a CU's sixteen waves finish within
  // one tile of each other.
  struct Tile {
    int t128, sub;   // wave-uniform (scalar registers)
    int perm[1][4];
    uint32_t sm;     // lane k: the tile's submask word of offset k
    int n_st[ST];    // neighbour rows (lane + 64 it: offset e / 16, row e % 16)
  };
  auto fetch = [&](int pos, Tile& T) -> bool {  // requests a tile's table; nothing waits here
    const int t = (int)blockIdx.x + (int)gridDim.x * pos;
    if (t >= n_sub) return false;
    T.t128 = __builtin_amdgcn_readfirstlane(p.tile_order ? p.tile_order[t >> 3] : (t >> 3));
    T.sub = t & 7;
    const int64_t row0 = (int64_t)T.t128 * PLAN_TILE + T.sub * 16;
    load_perm_rows<1>(p, row0, lq, T.perm);
    T.sm = lane < K ? p.submask[(int64_t)T.t128 * K + lane] : 0u;
#pragma unroll
    for (int it = 0; it < ST; ++it) {
      const int e = lane + 64 * it;
      T.n_st[it] = e < K * 16 ? p.nbr_s[(int64_t)(e >> 4) * p.Vpad + row0 + (e & 15)] : -1;
    }
    return true;
  };
  // ---- the layer's weights, once per workgroup
  {
    const float4* src = (const float4*)p.W;
    float4* dst = (float4*)w_s;
    const int n4 = K * CIN * COUT / 4;
    for (int i = tid; i < n4; i += WAVES * 64) dst[i] = src[i];
  }
  __syncthreads();
  if (p.trace) tr[1] = __builtin_amdgcn_s_memtime();
  Tile cur;
  bool have = fetch(wid, cur);
  int* idx_s = idx_all + wid * (32 * 16);
  const __amdgpu_buffer_rsrc_t rsrc_in = __builtin_amdgcn_make_buffer_rsrc((void*)p.in, 0, (int)p.in_bytes, 0x00020000);
  const float* w_lane = w_s + lq * COUT + NT * li;
  while (have) {
    // ---- this tile's table into LDS as byte offsets (absent: beyond the extent -> the gather returns zeros)
#pragma unroll
    for (int it = 0; it < ST; ++it) {
      const int e = lane + 64 * it;
      if (e < K * 16) idx_s[e] = (int)(cur.n_st[it] >= 0 ? (uint32_t)cur.n_st[it] * (uint32_t)(p.in_ld * 4) : BUF_ABSENT);
    }
    // active offsets of the sub-tile: a scalar bit mask walked with bit scans (no list in memory; two cursors: the gathers
    // run D offsets ahead of the matrix ops, the weight reads one)
    const uint32_t amask = (uint32_t)__ballot((cur.sm >> cur.sub) & 1u);
    const int nact = __builtin_popcount(amask);
    const int64_t row0 = (int64_t)cur.t128 * PLAN_TILE + cur.sub * 16;
    int o_pre[1][4] = {{cur.perm[0][0], cur.perm[0][1], cur.perm[0][2], cur.perm[0][3]}};
    __builtin_amdgcn_wave_barrier();
    if (p.trace && tr_tiles == 0) {
      tr[2] = __builtin_amdgcn_s_memtime();
      tr_nact = nact;
    }
    f32x4 acc[1][NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[0][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float4 g[D][G4];
    bvec_t b[2][KS];
    uint32_t g_rest = amask, w_rest = amask;
    const int k_last = amask ? 31 - __builtin_clz(amask) : 0;
    auto issue = [&](float4 (&dst)[G4]) {  // gathers of the next offset of the gather cursor (past the end: zeros, no access)
      const bool any = g_rest != 0u;
      const int k = any ? __builtin_ctz(g_rest) : k_last;
      g_rest &= g_rest - 1u;
      const uint32_t off = any ? (uint32_t)idx_s[k * 16 + li] : BUF_ABSENT;
#pragma unroll
      for (int jj = 0; jj < G4; ++jj) {
        const f32x4 v = buffer_load_floats<4>(rsrc_in, off + 16u * (uint32_t)lq, 64u * (uint32_t)jj);
        dst[jj] = make_float4(v[0], v[1], v[2], v[3]);
      }
    };
    auto load_w = [&](bvec_t (&dst)[KS]) {  // B operands of the weight cursor's next offset, from LDS
      const int k = w_rest ? __builtin_ctz(w_rest) : k_last;
      w_rest &= w_rest - 1u;
      const float* wk = w_lane + k * (CIN * COUT);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) dst[ks] = *(const bvec_t*)(wk + 4 * ks * COUT);
    };
    auto compute = [&](float4 (&a)[G4], bvec_t (&w)[KS]) {
#pragma unroll
      for (int jj = 0; jj < G4; ++jj) {
        float am[4] = {a[jj].x, a[jj].y, a[jj].z, a[jj].w};
        transpose4x4_lanegroups(am[0], am[1], am[2], am[3]);  // [m]: channel 16 jj + 4 m + lq of row li
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int n = 0; n < NT; ++n)
            acc[0][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(am[m], w[4 * jj + m][n], acc[0][n], 0, 0, 0);
      }
    };
#pragma unroll
    for (int d = 0; d < D; ++d) issue(g[d]);
    load_w(b[0]);
    if (nact > 0) {
      constexpr int U = (D % 2 == 0) ? D : 2 * D;
      for (int j0 = 0; j0 < nact; j0 += U) {
        if (p.trace && tr_tiles == 0 && j0 < 3 * U) tr_it[j0 / U] = __builtin_amdgcn_s_memtime() + (unsigned long long)(acc[0][0][0] == 12345.678f);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          load_w(b[(u + 1) & 1]);
          __builtin_amdgcn_sched_barrier(0);  // the weight reads of the NEXT offset go out before this offset's matrix ops
          compute(g[u % D], b[u & 1]);
          issue(g[u % D]);
        }
      }
    }
    if (p.trace && tr_tiles == 0) {
      // the accumulators are the loop's last results: reading one orders the stamp behind the matrix ops
      tr[3] = __builtin_amdgcn_s_memtime() + (unsigned long long)(acc[0][0][0] == 12345.678f);
    }
    epilogue_buffered<1, NT, true>(p, acc, row0, lq, NT * li, o_pre);
    __builtin_amdgcn_wave_barrier();  // the next sub-tile's table overwrites this one's
    if (p.trace && tr_tiles == 0) tr[4] = __builtin_amdgcn_s_memtime();
    ++tr_tiles;
    // ---- pull the next tile (requesting its table during the current tile measured no better: launch_conv_thin_lds)
    Tile nxt;
    int pos = 0;
    if (lane == 0) pos = __hip_atomic_fetch_add(&q_head, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    pos = __builtin_amdgcn_readfirstlane(pos);
    have = fetch(pos, nxt);
    if (have) cur = nxt;
  }
  if (p.trace && lane == 0) {
    tr[5] = __builtin_amdgcn_s_memtime();
    unsigned long long* o = p.trace + ((size_t)blockIdx.x * WAVES + wid) * 12;
    for (int i = 0; i < 6; ++i) o[i] = tr[i];
    o[6] = (unsigned long long)tr_tiles;
    o[7] = (unsigned long long)tr_nact;
    for (int i = 0; i < 3; ++i) o[8 + i] = tr_it[i];
  }
}

int launch_conv_thin_lds(const ConvParams& p, hipStream_t stream) {
  // <gathers in flight, waves per workgroup, next tile's table requested during the current tile>: measured at 88k / 26k voxels
  // (tools/hbm_layers_microbench.py, profiles/r04_thin_variants.txt): <2,16,no> 33.9 / 19.3 us (126 VGPRs, no spills),
  // <2,16,yes> 36.9 / 18.7, <4,16,no> 38.5 / 20.2 (14 registers spilled at the 128-VGPR limit of a 16-wave workgroup),
  // <4,8,no> 39.4 / 21.2, <4,12,yes> 39.9 / 19.5, <1,16,no> 36.8 / 21.9, <6,16,no> 43.3 / 23.1
  constexpr int D = 2, WAVES = 16;
  static int n_cu = 0;
  const size_t lds = ((size_t)p.K * 32 * 32 + (size_t)WAVES * (32 * 16)) * sizeof(float);
  static bool attr_set = false;
  if (!attr_set) {
    int dev = 0;
    hipDeviceProp_t prop;
    SV_HIP(hipGetDevice(&dev));
    SV_HIP(hipGetDeviceProperties(&prop, dev));
    n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    SV_HIP(hipFuncSetAttribute((const void*)conv_thin_lds_kernel<32, 32, D, WAVES>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(((size_t)27 * 32 * 32 + (size_t)WAVES * (32 * 16)) * sizeof(float))));
    attr_set = true;
  }
  const int n_sub = (int)(p.Vpad / 16);
  const int grid = n_sub < n_cu ? n_sub : n_cu;
  static const bool trace = getenv("SV_THIN_TRACE") != nullptr;  // experiments only: phase stamps of one launch to stderr
  ConvParams q = p;
  q.trace = nullptr;
  if (trace) {
    SV_HIP(hipMalloc((void**)&q.trace, (size_t)grid * WAVES * 12 * sizeof(unsigned long long)));
    SV_HIP(hipMemsetAsync(q.trace, 0, (size_t)grid * WAVES * 12 * sizeof(unsigned long long), stream));
  }
  hipLaunchKernelGGL((conv_thin_lds_kernel<32, 32, D, WAVES>), dim3((unsigned)grid), dim3(WAVES * 64), lds, stream, q, n_sub);
  SV_LAUNCH_CHECK();
  if (trace) {
    std::vector<unsigned long long> h((size_t)grid * WAVES * 12);
    SV_HIP(hipStreamSynchronize(stream));
    SV_HIP(hipMemcpy(h.data(), q.trace, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    SV_HIP(hipFree(q.trace));
    std::vector<double> stage, table, loop, store, life, per_off, it01, it12, pre;
    for (size_t w = 0; w < (size_t)grid * WAVES; ++w) {
      const unsigned long long* o = &h[w * 12];
      if (!o[0]) continue;
      if (o[8] && o[9] && o[10]) {
        pre.push_back((double)(o[8] - o[2]));
        it01.push_back((double)(o[9] - o[8]));
        it12.push_back((double)(o[10] - o[9]));
      }
      stage.push_back((double)(o[1] - o[0]));
      life.push_back((double)(o[5] - o[0]));
      if (o[6]) {
        table.push_back((double)(o[2] - o[1]));
        loop.push_back((double)(o[3] - o[2]));
        store.push_back((double)(o[4] - o[3]));
        if (o[7]) per_off.push_back((double)(o[3] - o[2]) / (double)o[7]);
      }
    }
    auto med = [](std::vector<double>& v) {
      if (v.empty()) return 0.0;
      std::sort(v.begin(), v.end());
      return v[v.size() / 2];
    };
    fprintf(stderr, "[thin trace] K=%d n_sub=%d grid=%d | median cycles: weights staged %.0f, first tile: table %.0f, loop %.0f "
            "(%.0f per offset; table staged -> loop %.0f, first 4 offsets %.0f, next 4 %.0f), store %.0f, wave life %.0f\n", p.K, n_sub,
            grid, med(stage), med(table), med(loop), med(per_off), med(pre), med(it01), med(it12), med(store), med(life));
  }
  return SV_OK;
}

int launch_conv_thin(const ConvParams& p, hipStream_t stream) {
  // one 16-row sub-tile per wave, four offsets in flight: 24 us for block1's 32->32 at level 1 (26.5k voxels) against 35 us
  // on the LDS-staged fused-offset tile, 49 against 84 us at 88k voxels (2.65 TB/s on algorithmic gather-bytes).  Two
  // sub-tiles per wave (shared weight registers) 27-28 / 48 us, three or six offsets in flight 26 / 51-54 us.
  // Round 4: the layer's weights resident in LDS, one 16-wave workgroup per CU (conv_thin_lds_kernel) - for a GPU that holds
  // ONE frame (the caller said so: sv_conv_set_dispatch(want_scale >= 1), the per-frame InferenceEngine.predict path and
  // every measurement of a layer alone; the rule itself is conv_select's).  Its workgroup needs a whole CU - 145 KB of LDS, sixteen wave slots at 126 VGPRs -
  // and beside the convolutions of other frames a CU only drains completely when a launch ends: inside the three-stream
  // pipeline its launches wait 0.2-3.6 ms for CUs (profiles/r04_bench_kernel_by_grid.txt, r04_cfg5_kernel_by_grid.txt) and
  // predict_stream loses 4 % (profiles/r04_ab_thin_in_pipeline.txt); there the four-wave workgroups of conv_thin_kernel,
  // which fit the slot any finishing convolution workgroup frees, stay the choice.  Same bits either way.
  hipLaunchKernelGGL((conv_thin_kernel<32, 32, 1, 4>), dim3((unsigned)(p.Vpad / 64)), dim3(256), 0, stream, p);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ---- first layer of the networks (conv0: Cin = 3 colour channels -> 32, 3x3x3, every voxel of the frame;
//      model/backbone/minkunet.py:55-57).  5.8 flop per byte of gather traffic: the layer is its gather.  One THREAD
//      per output voxel (in the plan's mask-sorted order, so a wavefront's rows share most neighbour offsets and an
//      offset nobody has is skipped for the whole wave): neighbour indices are read coalesced from the plan, the
//      3-float input rows come from the (cache-resident, 1 MB) feature table, the 27 x 3 x 32 weights are wave-uniform
//      scalar loads (SGPR operands of the fma), and the 32 accumulators per voxel are plain VALU fmaf chains in the same
//      (offset ascending, channel ascending) order as the matrix path.
template <int CIN, int COUT, int SPLIT>
__global__ __launch_bounds__(256) void conv_first_layer_kernel(ConvParams p) {
  constexpr int CT = COUT / SPLIT;  // output channels per thread; blockIdx.y selects the slice
  constexpr int KMAX = 27;
  const int tid = threadIdx.x;
  const int K = p.K;
  const int j0 = (int)blockIdx.y * CT;
  const float* __restrict__ w_s = p.W + j0;  // wave-uniform indices below -> scalar loads, weights as SGPR operands
  const int64_t r = (int64_t)blockIdx.x * 256 + tid;  // plan position
  const bool in_range = r < p.Vpad;
  const int64_t o = in_range ? (int64_t)p.perm[r] : -1;
  float acc[CT];
#pragma unroll
  for (int j = 0; j < CT; ++j) acc[j] = 0.0f;
  int n[KMAX];  // all neighbour indices of the voxel are requested up front (coalesced across the wavefront)
#pragma unroll
  for (int k = 0; k < KMAX; ++k) n[k] = (o >= 0 && k < K) ? p.nbr_s[(int64_t)k * p.Vpad + r] : -1;
  constexpr int G = 9;  // input rows in flight per thread
#pragma unroll
  for (int k0 = 0; k0 < KMAX; k0 += G) {
    float x[G][CIN];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float* src = p.in + (n[k0 + g] >= 0 ? (int64_t)n[k0 + g] * p.in_ld : 0);
#pragma unroll
      for (int c = 0; c < CIN; ++c) x[g][c] = src[c];
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const bool has = n[k0 + g] >= 0;
      if (__ballot(has) == 0ull) continue;  // no voxel of this wavefront has a neighbour at this offset
      const float* w = w_s + (k0 + g) * CIN * COUT;
      if (has) {
#pragma unroll
        for (int c = 0; c < CIN; ++c) {
#pragma unroll
          for (int j = 0; j < CT; ++j) acc[j] = __builtin_fmaf(x[g][c], w[c * COUT + j], acc[j]);
        }
      }
    }
  }
  if (o < 0) return;
  float* dst = p.out + o * p.out_ld + j0;
#pragma unroll
  for (int j = 0; j < CT; ++j) {
    float v = acc[j];
    if (p.scale)
      v = __builtin_fmaf(v, p.scale[j0 + j], p.shift ? p.shift[j0 + j] : 0.0f);
    else if (p.shift)
      v = v + p.shift[j0 + j];
    if (p.residual) v = v + p.residual[o * p.res_ld + j0 + j];
    if (p.act == SV_ACT_RELU)
      v = v < 0.f ? 0.f : v;  // NaN stays NaN, as torch.relu
    else if (p.act == SV_ACT_LEAKY_RELU)
      v = v > 0.f ? v : v * p.slope;
    acc[j] = v;
  }
  if ((p.out_ld & 3) == 0 && (((uintptr_t)p.out) & 15) == 0) {
#pragma unroll
    for (int j = 0; j < CT; j += 4) *(float4*)(dst + j) = make_float4(acc[j], acc[j + 1], acc[j + 2], acc[j + 3]);
  } else {
#pragma unroll
    for (int j = 0; j < CT; ++j) dst[j] = acc[j];
  }
}

int launch_conv_first_mfma(const ConvParams& p, hipStream_t stream) {
  const unsigned cap = 768;  // workgroups (see the kernel)
  const unsigned groups = (unsigned)(p.Vpad / 64);
  hipLaunchKernelGGL((conv_first_mfma_kernel<32>), dim3(groups > cap ? cap : groups), dim3(256), 0, stream, p);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

int launch_conv_first_layer(const ConvParams& p, hipStream_t stream) {
  // SPLIT = 1: one thread computes all 32 channels of its voxel (two / four threads per voxel measured 18 / 26 us
  // against 16 us: the gathers are repeated per slice)
  dim3 grid((unsigned)((p.Vpad + 255) / 256), 1);
  hipLaunchKernelGGL((conv_first_layer_kernel<3, 32, 1>), grid, dim3(256), 0, stream, p);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

int launch_linear_narrow(const ConvParams& p, hipStream_t stream) {
  dim3 grid((unsigned)((p.V_out + NARROW_ROWS - 1) / NARROW_ROWS));
  switch (p.Cout) {
    case 1: hipLaunchKernelGGL((linear_narrow_kernel<1>), grid, dim3(256), 0, stream, p); break;
    case 2: hipLaunchKernelGGL((linear_narrow_kernel<2>), grid, dim3(256), 0, stream, p); break;
    case 3: hipLaunchKernelGGL((linear_narrow_kernel<3>), grid, dim3(256), 0, stream, p); break;
    default: hipLaunchKernelGGL((linear_narrow_kernel<4>), grid, dim3(256), 0, stream, p); break;
  }
  SV_LAUNCH_CHECK();
  return SV_OK;
}

}  // namespace sv
