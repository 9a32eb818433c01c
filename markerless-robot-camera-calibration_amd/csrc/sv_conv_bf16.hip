// Opt-in bf16 matrix-core path of the wide sparse convolution layers (sv_conv_fwd_bf16, sv_pack_weights_bf16).
//
// Replaces the same ME.MinkowskiConvolution / ConvolutionTranspose / Linear (+ BN(eval) / bias + residual + activation)
// calls as sv_conv.hip (model/backbone/minkunet.py:125-187, model/robotnet_segmentation.py:55-64) for layers with
// Cin % 32 == 0, Cin >= 64, Cout % 16 == 0, Cout >= 64, at reduced precision: weights rounded once to bf16 (packed), each
// gathered fp32 input row rounded to bf16 in registers, products summed in fp32 by v_mfma_f32_16x16x32_bf16, the epilogue
// in fp32 exactly as sv_conv_fwd's.
//
// Work decomposition
//   * a workgroup (8 waves) owns one plan tile (128 output rows in the plan's mask-sorted order) x TN = 16 NT output
//     channels; wave w owns the tile's 16-row sub-tile w, so the plan's sub-tile skipping (submask bit w) is a
//     wave-uniform branch;
//   * it walks steps = (active kernel offset k ascending, 32-channel chunk ascending), one MFMA per step and column tile;
//   * A (the wave's 16 gathered rows x 32 channels): lane l reads row l & 15, channels 8 (l >> 4) .. +7 (32 B, two float4)
//     of its own gathered row straight into registers one step ahead and converts them to one bf16 fragment
//     (v_cvt_pk_bf16_f32, round to nearest even, NaN stays NaN);
//   * B (the step's packed weights, 32 x TN bf16 = 64 TN bytes): global -> registers one step ahead -> LDS (double
//     buffered, one barrier per step), shared by the eight waves; every lane reads its 16-byte fragment per column tile.
// Numerics: every output element is ONE accumulator chain over (k ascending, chunk ascending) with the raw accumulator of
// an earlier offset-range pass as its C operand, so the result does not depend on the tile, the launch, the dispatch
// scale, the pass split or the frames grouped into the tensor.  An absent neighbour's row reads as zeros.
#include <stdio.h>

#include "sv_common.h"

namespace sv {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4_b __attribute__((ext_vector_type(4)));

constexpr int BF_TM = SV_TILE_ROWS;  // output rows per workgroup = one plan tile
constexpr int BF_WAVES = BF_TM / 16;  // one 16-row sub-tile per wave
constexpr int BF_THREADS = BF_WAVES * 64;
constexpr int BF_KC = 32;            // input channels per step (the MFMA's k)
constexpr int BF_MAX_K = 27;

struct Bf16Params {
  const float* in;
  int64_t in_ld;
  int Cin;
  const bf16x8* Wp;
  int K;
  int Cout;
  const int32_t* perm;
  const int32_t* nbr_s;
  const uint32_t* submask;
  const int32_t* tile_order;
  int64_t V_out;
  int64_t Vpad;
  const float* acc_init;
  int64_t acc_ld;
  const float* scale;
  const float* shift;
  const float* residual;
  int64_t res_ld;
  int act;
  float slope;
  float* out;
  int64_t out_ld;
  int ny;  // column blocks of TN channels
};

template <int NT>
__global__ __launch_bounds__(BF_THREADS) void conv_bf16_kernel(Bf16Params p) {
  constexpr int TN = NT * 16;
  constexpr int B_FRAGS = NT * 64;  // 16-byte fragments of one step's weights
  constexpr int B_PER_THREAD = (B_FRAGS + BF_THREADS - 1) / BF_THREADS;
  __shared__ bf16x8 Bs[2][B_FRAGS];
  __shared__ int idx_s[BF_MAX_K * BF_TM];  // gathered input row of every (offset, tile row), -1 = absent

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = p.K;
  const int ncb = p.Cin / BF_KC;
  const int t_lin = blockIdx.x / p.ny;
  const int n0 = (blockIdx.x % p.ny) * TN;
  const int ntiles = (int)(p.Vpad / BF_TM);
  const int p128 = p.tile_order ? p.tile_order[t_lin] : ntiles - 1 - t_lin;
  const int64_t row0 = (int64_t)p128 * BF_TM;

  // ---- neighbour table of the tile (identity for dense rows)
  for (int e = tid; e < K * BF_TM; e += BF_THREADS) {
    const int k = e / BF_TM, r = e % BF_TM;
    int n;
    if (p.nbr_s)
      n = p.nbr_s[(int64_t)k * p.Vpad + row0 + r];
    else
      n = (row0 + r < p.V_out) ? (int)(row0 + r) : -1;
    idx_s[e] = n;
  }
  // ---- active offsets: lane k holds the tile's sub-tile mask for offset k; the workgroup steps through the union
  uint32_t dense_mask = 0xffu;
  if (p.submask == nullptr) {
    const int64_t rem = p.V_out - row0;
    const int nsub = rem >= BF_TM ? BF_WAVES : (int)((rem + 15) / 16);
    dense_mask = (1u << nsub) - 1u;
  }
  uint32_t my_sm = 0;
  if (lane < K) my_sm = p.submask ? p.submask[(int64_t)p128 * K + lane] & 0xffu : dense_mask;
  const uint32_t amask = (uint32_t)__ballot(my_sm != 0);
  auto wave_active = [&](int k) -> bool {
    return ((uint32_t)__builtin_amdgcn_readlane((int)my_sm, k) >> w) & 1u;
  };

  // ---- accumulators: C/D map col = lane & 15 (channel n0 + 16 n + col), row = 4 (lane >> 4) + reg of sub-tile w
  const int li = lane & 15, lq = lane >> 4;
  int o_rows[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int64_t r = row0 + 16 * w + 4 * lq + reg;
    o_rows[reg] = p.perm ? p.perm[r] : (r < p.V_out ? (int)r : -1);
  }
  f32x4_b acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
      acc[n][reg] = (p.acc_init && o_rows[reg] >= 0) ? p.acc_init[(int64_t)o_rows[reg] * p.acc_ld + n0 + 16 * n + li] : 0.0f;
  }

  const float* in = p.in;
  const int64_t in_ld = p.in_ld;
  auto load_a = [&](int k, int cb, float4 (&ra)[2]) {
    const int n = idx_s[k * BF_TM + 16 * w + li];
    if (n >= 0) {
      const float4* src = (const float4*)(in + (int64_t)n * in_ld + cb * BF_KC + 8 * lq);
      ra[0] = src[0];
      ra[1] = src[1];
    } else {
      ra[0] = make_float4(0.f, 0.f, 0.f, 0.f);
      ra[1] = ra[0];
    }
  };
  const int tiles16 = p.Cout / 16;
  auto load_b = [&](int k, int cb, bf16x8 (&rb)[B_PER_THREAD]) {
    const bf16x8* src = p.Wp + ((int64_t)(k * ncb + cb) * tiles16 + n0 / 16) * 64;
#pragma unroll
    for (int i = 0; i < B_PER_THREAD; ++i) {
      const int f = tid + BF_THREADS * i;
      if (B_FRAGS % BF_THREADS == 0 || f < B_FRAGS) rb[i] = src[f];
    }
  };
  auto store_b = [&](int buf, const bf16x8 (&rb)[B_PER_THREAD]) {
#pragma unroll
    for (int i = 0; i < B_PER_THREAD; ++i) {
      const int f = tid + BF_THREADS * i;
      if (B_FRAGS % BF_THREADS == 0 || f < B_FRAGS) Bs[buf][f] = rb[i];
    }
  };

  if (amask != 0) {
    int k = __builtin_ctz(amask), cb = 0;
    bool act = wave_active(k);
    float4 ra[2];
    bf16x8 rb[B_PER_THREAD];
    __syncthreads();  // idx_s
    load_b(k, cb, rb);
    if (act) load_a(k, cb, ra);
    store_b(0, rb);
    __syncthreads();
    int buf = 0;
    for (;;) {
      // next step: (k, cb + 1) or the next active offset's first chunk
      int k2 = k, cb2 = cb + 1;
      bool have_next = true;
      if (cb2 == ncb) {
        cb2 = 0;
        const uint32_t rest = amask & ~((2u << k) - 1u);
        have_next = rest != 0;
        k2 = have_next ? __builtin_ctz(rest) : 0;
      }
      const bool act2 = have_next && wave_active(k2);
      float4 ra2[2];
      if (have_next) {
        load_b(k2, cb2, rb);
        if (act2) load_a(k2, cb2, ra2);
      }
      if (act) {
        const f32x8 v = {ra[0].x, ra[0].y, ra[0].z, ra[0].w, ra[1].x, ra[1].y, ra[1].z, ra[1].w};
        const bf16x8 a = __builtin_convertvector(v, bf16x8);
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, Bs[buf][n * 64 + lane], acc[n], 0, 0, 0);
      }
      if (!have_next) break;
      store_b(buf ^ 1, rb);
      __syncthreads();
      buf ^= 1;
      k = k2;
      cb = cb2;
      act = act2;
      if (act) {
        ra[0] = ra2[0];
        ra[1] = ra2[1];
      }
    }
  }

  // ---- epilogue (fp32, sv_conv_fwd's arithmetic): y = fmaf(acc, scale, shift) + residual -> activation -> out[perm]
  const float slope = p.slope;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int col = n0 + 16 * n + li;
    const float sc = p.scale ? p.scale[col] : 1.0f;
    const float sh = p.shift ? p.shift[col] : (p.scale ? 0.0f : -0.0f);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int o = o_rows[reg];
      if (o < 0) continue;
      const float res = p.residual ? p.residual[(int64_t)o * p.res_ld + col] : -0.0f;
      float v = __builtin_fmaf(acc[n][reg], sc, sh) + res;
      if (p.act == SV_ACT_RELU)
        v = v < 0.f ? 0.f : v;  // NaN stays NaN, as torch.relu
      else if (p.act == SV_ACT_LEAKY_RELU)
        v = v > 0.f ? v : v * slope;
      p.out[(int64_t)o * p.out_ld + col] = v;
    }
  }
}

// Wp[((k * Cin/32 + cb) * Cout/16 + t) * 512 + 8 l + j] = bf16(W[k][32 cb + 8 (l >> 4) + j][16 t + (l & 15)]): the B
// fragment of lane l for chunk cb and column tile t, 16 consecutive bytes.
__global__ __launch_bounds__(256) void pack_weights_bf16_kernel(const float* __restrict__ W, int K, int Cin, int Cout,
                                                                bf16x8* __restrict__ Wp) {
  const int64_t nfrag = (int64_t)K * Cin * Cout / 8;
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nfrag) return;
  const int l = (int)(f & 63);
  const int64_t blk = f >> 6;  // (k, cb, t)
  const int tiles16 = Cout / 16, ncb = Cin / BF_KC;
  const int t = (int)(blk % tiles16);
  const int64_t kcb = blk / tiles16;
  const int cb = (int)(kcb % ncb);
  const int k = (int)(kcb / ncb);
  const int col = 16 * t + (l & 15);
  const int c0 = BF_KC * cb + 8 * (l >> 4);
  f32x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = W[((int64_t)k * Cin + c0 + j) * Cout + col];
  Wp[f] = __builtin_convertvector(v, bf16x8);
}

template <int NT>
int launch_bf16(const Bf16Params& p0, hipStream_t stream) {
  Bf16Params p = p0;
  p.ny = p.Cout / (16 * NT);
  const int64_t grid = (p.Vpad / BF_TM) * p.ny;
  if (grid > 0x7fffffff) {
    set_error("sv_conv_fwd_bf16: %lld workgroups", (long long)grid);
    return SV_ERR_INVALID;
  }
  hipLaunchKernelGGL(conv_bf16_kernel<NT>, dim3((unsigned)grid), dim3(BF_THREADS), 0, stream, p);
  SV_LAUNCH_CHECK();
  // the thread's instance record is the buffer sv_conv_last_instance() returns (128 bytes, this thread's own)
  snprintf(const_cast<char*>(sv_conv_last_instance()), 128, "conv_bf16_kernel<%d, %d>|fast=0,ring=0,full=0", BF_TM, 16 * NT);
  return SV_OK;
}

// unsupported shapes: a message and SV_ERR_UNSUPPORTED, no pointer looked at
int bf16_shape_unsupported(const char* fn, int Cin, int Cout, int K, bool conv) {
  if (Cin % BF_KC != 0 || Cout % 16 != 0) {
    set_error("%s: needs Cin %% 32 == 0 and Cout %% 16 == 0 (got Cin %d, Cout %d)", fn, Cin, Cout);
    return SV_ERR_UNSUPPORTED;
  }
  if (conv && (Cin < 64 || Cout < 64)) {
    set_error("%s: needs Cin >= 64 and Cout >= 64 (got Cin %d, Cout %d): the thin layers stay on sv_conv_fwd", fn, Cin, Cout);
    return SV_ERR_UNSUPPORTED;
  }
  if (K > BF_MAX_K) {
    set_error("%s: kernel volume %d above 27", fn, K);
    return SV_ERR_UNSUPPORTED;
  }
  return SV_OK;
}

}  // namespace
}  // namespace sv

using namespace sv;

extern "C" int sv_pack_weights_bf16(const float* W, int K, int Cin, int Cout, uint16_t* Wp, sv_stream_t stream_) {
  SV_CHECK_ARG(Cin > 0 && Cout > 0 && K >= 1, "bad channel / kernel volume");
  if (int rc = bf16_shape_unsupported(__func__, Cin, Cout, K, false)) return rc;
  SV_CHECK_ARG(W && Wp, "null pointer");
  SV_CHECK_ARG(((uintptr_t)Wp & 15) == 0, "Wp must be 16-byte aligned");
  const int64_t nfrag = (int64_t)K * Cin * Cout / 8;
  hipLaunchKernelGGL(pack_weights_bf16_kernel, dim3((unsigned)((nfrag + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, W, K,
                     Cin, Cout, (bf16x8*)Wp);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_conv_fwd_bf16(const float* in, int64_t V_in, int64_t in_ld, int Cin, const uint16_t* Wp, int K, int Cout,
                                const int32_t* perm, const int32_t* nbr_s, const uint32_t* submask, const int32_t* tile_order,
                                int64_t V_out, int64_t Vpad, const float* acc_init, int64_t acc_ld, const float* scale,
                                const float* shift, const float* residual, int64_t res_ld, int act, float slope, float* out,
                                int64_t out_ld, sv_stream_t stream_) {
  SV_CHECK_ARG(Cin > 0 && Cout > 0 && K >= 1, "bad channel / kernel volume");
  if (int rc = bf16_shape_unsupported(__func__, Cin, Cout, K, true)) return rc;
  SV_CHECK_ARG(!acc_init || acc_ld >= Cout, "acc_init stride too small");
  SV_CHECK_ARG(V_out >= 0 && Vpad >= V_out && Vpad % BF_TM == 0, "Vpad must be a multiple of 128 >= V_out");
  SV_CHECK_ARG(in_ld >= Cin && out_ld >= Cout, "row strides too small");
  SV_CHECK_ARG(act >= SV_ACT_NONE && act <= SV_ACT_LEAKY_RELU, "bad activation");
  if (V_out == 0) return SV_OK;
  SV_CHECK_ARG(in && Wp && out, "null pointer");
  SV_CHECK_ARG(V_in >= 1, "V_in = rows of `in` (every index of the plan is below it)");
  const bool has_plan = perm || nbr_s || submask;
  SV_CHECK_ARG(!has_plan || (perm && nbr_s && submask), "perm, nbr_s and submask must be given together");
  SV_CHECK_ARG(has_plan || K == 1, "K > 1 needs a plan");
  SV_CHECK_ARG(!residual || res_ld >= Cout, "residual stride too small");
  SV_CHECK_ARG(in_ld % 4 == 0 && ((uintptr_t)in & 15) == 0, "in must be 16-byte aligned with in_ld % 4 == 0");
  SV_CHECK_ARG(((uintptr_t)Wp & 15) == 0, "Wp must be 16-byte aligned");
  Bf16Params p;
  p.in = in; p.in_ld = in_ld; p.Cin = Cin; p.Wp = (const bf16x8*)Wp; p.K = K; p.Cout = Cout;
  p.perm = perm; p.nbr_s = nbr_s; p.submask = submask; p.tile_order = tile_order; p.V_out = V_out; p.Vpad = Vpad;
  p.acc_init = acc_init; p.acc_ld = acc_ld;
  p.scale = scale; p.shift = shift; p.residual = residual; p.res_ld = res_ld;
  p.act = act; p.slope = slope; p.out = out; p.out_ld = out_ld;
  p.ny = 0;
  hipStream_t stream = (hipStream_t)stream_;
  // widest column block that divides Cout (384: the whole row; 1024: four blocks of 256)
  const int t16 = Cout / 16;
  if (t16 % 24 == 0) return launch_bf16<24>(p, stream);
  if (t16 % 16 == 0) return launch_bf16<16>(p, stream);
  if (t16 % 12 == 0) return launch_bf16<12>(p, stream);
  if (t16 % 8 == 0) return launch_bf16<8>(p, stream);
  if (t16 % 6 == 0) return launch_bf16<6>(p, stream);
  if (t16 % 4 == 0) return launch_bf16<4>(p, stream);
  if (t16 % 2 == 0) return launch_bf16<2>(p, stream);
  return launch_bf16<1>(p, stream);
}
