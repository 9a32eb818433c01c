// Shared by the sparse convolution kernels of sv_conv.hip (tiled wide kernel, instance selection) and sv_conv_special.hip
// (thin, thin-LDS, conv0 and narrow-linear kernels): the launch parameters, buffer addressing and the fused epilogue.
#pragma once
#include <type_traits>

#include "sv_common.h"
#include "sv_conv_select.h"

namespace sv {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct ConvParams {
  const float* in;
  int64_t in_ld;
  int Cin;
  const float* W;
  int K;
  int Cout;
  const int32_t* perm;
  const int32_t* nbr_s;
  const uint32_t* submask;
  const int32_t* tile_order;  // plan tiles (128 rows), longest first; NULL = reverse plan order
  int64_t V_out;
  int64_t Vpad;
  const float* scale;
  const float* shift;
  const float* residual;
  int64_t res_ld;
  // accumulator hand-over between the passes of a layer whose kernel offsets are split into ascending ranges (each range
  // with its own plan / row order): acc_init[o][n] = the raw fma chain over the EARLIER offsets of output element (o, n); it
  // is the matrix op's C operand at the start of this launch's chain, so the chain over all offsets is the one chain it
  // always was.  NULL = the chain starts at 0.
  const float* acc_init;
  int64_t acc_ld;
  uint32_t acc_bytes;
  int act;
  float slope;
  float* out;
  int64_t out_ld;
  int vec_a;  // in_ld % 4 == 0 && Cin % 4 == 0 && base aligned -> float4 gathers
  // FAST instances address `in` and `W` through buffer descriptors with 32-bit byte offsets (see conv_tile_body):
  uint32_t in_bytes, w_bytes, out_bytes, res_bytes;  // extents of in, W, out, residual
  int buf_ok;  // all of them below BUF_LIMIT (else the guarded generic form with 64-bit addresses runs)
  int ntiles;
  int ny;
  unsigned long long* trace;  // SV_CONV_TRACE experiments: per-workgroup {start, end, hw id, steps}; null otherwise
  int main_blocks;            // dual-body launches: workgroups [0, main_blocks) run the main tile shape over the plan tiles
  int main_tiles128;          //   tile_order[0, main_tiles128), the rest the tail shape over tile_order[main_tiles128, ..)
};

// launchers of the special-shape kernels (sv_conv_special.hip), one per ConvKind that conv_select() names
int launch_conv_first_mfma(const ConvParams& p, hipStream_t stream);
int launch_conv_first_layer(const ConvParams& p, hipStream_t stream);
int launch_conv_thin(const ConvParams& p, hipStream_t stream);
int launch_conv_thin_lds(const ConvParams& p, hipStream_t stream);
int launch_linear_narrow(const ConvParams& p, hipStream_t stream);

// Buffer addressing of the FAST instances.  Measured with tools/mfma_probe.py on gfx950: a `global_load` with a 64-bit
// VGPR address costs the SIMD's matrix pipe ~45 cycles of issue per instruction (one per 12 matrix ops: 0.98 -> 0.86 of
// the peak issue rate), and every VALU instruction in the loop (address arithmetic, selects) its own execution time;
// `buffer_load` with a 32-bit VGPR offset and an SGPR offset costs nothing measurable (0.97).  Out-of-range offsets
// return 0 without a memory access, which is how absent neighbours read as zero rows: no select, no branch.
constexpr uint32_t BUF_ABSENT = 0x80000000u;  // byte offset of an absent neighbour's row: beyond every extent
constexpr uint32_t BUF_LIMIT = 0x7fff0000u;   // extents stay below BUF_ABSENT minus the largest column offset
typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x3_t __attribute__((ext_vector_type(3)));
typedef int i32x2_t __attribute__((ext_vector_type(2)));
template <int N>
__device__ __forceinline__ auto buffer_load_floats(__amdgpu_buffer_rsrc_t rsrc, uint32_t voffset, uint32_t soffset) {
  typedef float vec_t __attribute__((ext_vector_type(N)));
  if constexpr (N == 1) {
    vec_t r;
    r[0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voffset, soffset, 0));
    return r;
  } else if constexpr (N == 2) {
    return __builtin_bit_cast(vec_t, __builtin_amdgcn_raw_buffer_load_b64(rsrc, voffset, soffset, 0));
  } else if constexpr (N == 3) {
    return __builtin_bit_cast(vec_t, __builtin_amdgcn_raw_buffer_load_b96(rsrc, voffset, soffset, 0));
  } else {
    static_assert(N == 4, "1..4 floats per load");
    return __builtin_bit_cast(vec_t, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voffset, soffset, 0));
  }
}

// ---- epilogue of the buffer-addressed kernels: BN(eval) / bias -> residual -> activation -> store by `perm`.
//      acc[s][n][reg]: C/D map of the matrix op, column = lane & 15 of column tile n (output channel col0 + n), row =
//      rows0 + 16 s + 4 lq + reg of the plan.
// the 4 consecutive plan rows a lane stores per sub-tile (one int4 of `perm`); the single-wave kernels request them at
// their very start so that the epilogue does not begin with a dependent round trip
template <int MR>
__device__ __forceinline__ void load_perm_rows(const ConvParams& p, const int64_t rows0, const int lq, int (&o)[MR][4]) {
#pragma unroll
  for (int s = 0; s < MR; ++s) {
    const int64_t r = rows0 + s * 16 + lq * 4;
    if (p.perm) {
      const int4 o4 = *(const int4*)(p.perm + r);
      o[s][0] = o4.x;
      o[s][1] = o4.y;
      o[s][2] = o4.z;
      o[s][3] = o4.w;
    } else {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) o[s][reg] = (r + reg < p.V_out) ? (int)(r + reg) : -1;
    }
  }
}

template <int MR, int NT, bool PRELOADED = false>
__device__ __forceinline__ void epilogue_buffered(const ConvParams& p, const f32x4 (&acc)[MR][NT], const int64_t rows0,
                                                  const int lq, const int col0, const int (*o_pre)[4] = nullptr) {
  // branch-free: the 4 consecutive output rows a lane holds per sub-tile come from ONE int4 load of `perm`, all MR of
  // them requested up front; a sub-tile's residual rows are requested together; rows past V_out (perm < 0) get a
  // byte offset beyond the extents, so their residual loads return zeros and their stores are dropped by the
  // descriptor's range check.  (With a branch per row and per column the epilogue was a chain of dependent round
  // trips - 31 us of a 770 us workgroup on the 64-row tile; this form: dense layers +4-5 %, the level-0 launch and
  // the frame rate +1.2 %.)
  typedef float yvec_t __attribute__((ext_vector_type(NT)));
  const __amdgpu_buffer_rsrc_t rsrc_out = __builtin_amdgcn_make_buffer_rsrc((void*)p.out, 0, (int)p.out_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_res =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.residual, 0, p.residual ? (int)p.res_bytes : 0, 0x00020000);
  int o[MR][4];
  if constexpr (PRELOADED) {
#pragma unroll
    for (int s = 0; s < MR; ++s)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) o[s][reg] = o_pre[s][reg];
  } else {
    load_perm_rows<MR>(p, rows0, lq, o);
  }
  // The arithmetic is unconditional: absent BN / bias / residual become operands that change no bit of any value
  // (fmaf(x, 1, -0) == x and x + (-0) == x for every x, signed zeros and NaN included; bias alone: fmaf(x, 1, b) is
  // the one rounding of x + b), and the activation is chosen ONCE, outside the unrolled element loops.  (With the
  // three run-time switches tested per element the 48 elements of a lane were ~150 scalar branches: 22 us from the
  // end of the loop to the last store of a 64-row workgroup, 7 us of a 16-row one - per-phase stamps of a trace build.)
  float scf[NT], shf[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    scf[n] = p.scale ? p.scale[col0 + n] : 1.0f;
    shf[n] = p.shift ? p.shift[col0 + n] : (p.scale ? 0.0f : -0.0f);
  }
  const float slope = p.slope;
  auto finish = [&](auto act_tag) {
    constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
    for (int s = 0; s < MR; ++s) {
      yvec_t res[4];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
#pragma unroll
        for (int n = 0; n < NT; ++n) res[reg][n] = -0.0f;
      if (p.residual) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          res[reg] = buffer_load_floats<NT>(
              rsrc_res, o[s][reg] >= 0 ? (uint32_t)o[s][reg] * (uint32_t)(p.res_ld * 4) + (uint32_t)col0 * 4u : BUF_ABSENT,
              0u);
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        yvec_t y;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          float v = __builtin_fmaf(acc[s][n][reg], scf[n], shf[n]) + res[reg][n];
          if constexpr (ACT == SV_ACT_RELU)
            v = v < 0.f ? 0.f : v;  // NaN stays NaN, as torch.relu
          else if constexpr (ACT == SV_ACT_LEAKY_RELU)
            v = v > 0.f ? v : v * slope;
          y[n] = v;
        }
        const uint32_t off =
            o[s][reg] >= 0 ? (uint32_t)o[s][reg] * (uint32_t)(p.out_ld * 4) + (uint32_t)col0 * 4u : BUF_ABSENT;
        if constexpr (NT == 1)
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, y[0]), rsrc_out, off, 0, 0);
        else if constexpr (NT == 2)
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(i32x2_t, y), rsrc_out, off, 0, 0);
        else if constexpr (NT == 3)
          __builtin_amdgcn_raw_buffer_store_b96(__builtin_bit_cast(i32x3_t, y), rsrc_out, off, 0, 0);
        else
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4_t, y), rsrc_out, off, 0, 0);
      }
    }
  };
  if (p.act == SV_ACT_RELU)
    finish(std::integral_constant<int, SV_ACT_RELU>{});
  else if (p.act == SV_ACT_LEAKY_RELU)
    finish(std::integral_constant<int, SV_ACT_LEAKY_RELU>{});
  else
    finish(std::integral_constant<int, SV_ACT_NONE>{});
}

}  // namespace sv
