// Local pooling over a kernel map (ME.MinkowskiMaxPooling / AvgPooling / SumPooling; model/backbone/resnet.py:57 is the
// kernel_size 2 stride 2 max pooling of the ResNet stem).  Memory-bound: the forward is one wavefront per output row with the
// lanes along the channels (coalesced rows, float4 where the alignment allows), the backward one thread per (input row,
// channel) over the TRANSPOSED table - a gather, no float atomics, so repeated calls give the same bits.
#include "sv_common.h"

namespace sv {

constexpr int POOL_WAVES = 4;  // output rows per 256-thread workgroup

struct PoolAcc {
  float v;
  int arg;
  bool any;
};

__device__ __forceinline__ void pool_step(PoolAcc& a, float x, int row, int mode) {
  if (mode == SV_POOL_MAX) {
    // torch's max(dim) rule (sv_group_max): the first NaN wins and stays, a tie goes to the lowest k
    if (!a.any || (x > a.v) || (x != x && a.v == a.v)) {
      a.v = x;
      a.arg = row;
    }
  } else {
    a.v = a.v + x;
  }
  a.any = true;
}

__device__ __forceinline__ float pool_finish(const PoolAcc& a, int count, int mode) {
  if (!a.any) return 0.0f;
  return mode == SV_POOL_AVG ? a.v / (float)count : a.v;
}

template <int VW>
__global__ __launch_bounds__(64 * POOL_WAVES) void pool_local_kernel(const float* __restrict__ in, int64_t in_ld, int C,
                                                                     const int32_t* __restrict__ nbr, int64_t ld, int K,
                                                                     int64_t V_out, int mode, float* __restrict__ out,
                                                                     int64_t out_ld, int32_t* __restrict__ arg) {
  const int64_t o = (int64_t)blockIdx.x * POOL_WAVES + (threadIdx.x >> 6);
  if (o >= V_out) return;
  const int lane = threadIdx.x & 63;
  int count = 0;
  for (int k = 0; k < K; ++k) count += nbr[(int64_t)k * ld + o] >= 0;
  for (int c0 = lane * VW; c0 < C; c0 += 64 * VW) {
    PoolAcc a[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) a[j] = {0.0f, -1, false};
    for (int k = 0; k < K; ++k) {
      const int i = nbr[(int64_t)k * ld + o];  // wave-uniform
      if (i < 0) continue;
      const float* p = in + (int64_t)i * in_ld + c0;
      if constexpr (VW == 4) {
        const float4 x = *(const float4*)p;
        pool_step(a[0], x.x, i, mode);
        pool_step(a[1], x.y, i, mode);
        pool_step(a[2], x.z, i, mode);
        pool_step(a[3], x.w, i, mode);
      } else {
        pool_step(a[0], p[0], i, mode);
      }
    }
    if constexpr (VW == 4) {
      *(float4*)(out + o * out_ld + c0) = make_float4(pool_finish(a[0], count, mode), pool_finish(a[1], count, mode),
                                                      pool_finish(a[2], count, mode), pool_finish(a[3], count, mode));
      if (arg) *(int4*)(arg + o * (int64_t)C + c0) = make_int4(a[0].arg, a[1].arg, a[2].arg, a[3].arg);
    } else {
      out[o * out_ld + c0] = pool_finish(a[0], count, mode);
      if (arg) arg[o * (int64_t)C + c0] = a[0].arg;
    }
  }
}

__global__ __launch_bounds__(256) void pool_local_backward_kernel(const float* __restrict__ dy, int64_t dy_ld, int C,
                                                                   const int32_t* __restrict__ nbr_t, int64_t ld_t, int K,
                                                                   int64_t V_in, int mode, const int32_t* __restrict__ arg,
                                                                   const uint32_t* __restrict__ mask_fwd,
                                                                   float* __restrict__ dx, int64_t dx_ld) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= V_in * C) return;
  const int64_t i = t / C;
  const int c = (int)(t - i * C);
  float acc = 0.0f;
  for (int k = 0; k < K; ++k) {
    const int o = nbr_t[(int64_t)k * ld_t + i];
    if (o < 0) continue;
    const float g = dy[(int64_t)o * dy_ld + c];
    if (mode == SV_POOL_MAX) {
      if (arg[(int64_t)o * C + c] == (int32_t)i) acc += g;
    } else if (mode == SV_POOL_AVG) {
      acc += g / (float)__popc(mask_fwd[o]);
    } else {
      acc += g;
    }
  }
  dx[i * dx_ld + c] = acc;
}

}  // namespace sv

using namespace sv;

extern "C" {

int sv_pool_local(const float* in, int64_t V_in, int64_t in_ld, int C, const int32_t* nbr, int64_t ld, int K, int64_t V_out,
                  int mode, float* out, int64_t out_ld, int32_t* arg, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(C >= 1 && in_ld >= C && out_ld >= C && V_in >= 0 && V_out >= 0, "bad shape");
  SV_CHECK_ARG(K >= 1 && K <= 32, "K must be in 1..32");
  SV_CHECK_ARG(ld >= V_out, "bad shape (ld < V_out)");
  SV_CHECK_ARG(mode == SV_POOL_MAX || mode == SV_POOL_AVG || mode == SV_POOL_SUM, "bad mode");
  SV_CHECK_ARG(V_out < (1ll << 31) - 1024 && V_in < (1ll << 31), "row count out of range");
  if (V_out == 0) return SV_OK;
  SV_CHECK_ARG(nbr && out && (in || V_in == 0), "null pointer");
  SV_CHECK_ARG(mode != SV_POOL_MAX || arg, "null pointer (max pooling writes arg)");
  const bool vec = C % 4 == 0 && in_ld % 4 == 0 && out_ld % 4 == 0 && ((uintptr_t)in % 16) == 0 && ((uintptr_t)out % 16) == 0 &&
                   ((uintptr_t)arg % 16) == 0;
  const unsigned nb = (unsigned)((V_out + POOL_WAVES - 1) / POOL_WAVES);
  int32_t* a = mode == SV_POOL_MAX ? arg : nullptr;
  if (vec)
    hipLaunchKernelGGL(pool_local_kernel<4>, dim3(nb), dim3(64 * POOL_WAVES), 0, stream, in, in_ld, C, nbr, ld, K, V_out, mode,
                       out, out_ld, a);
  else
    hipLaunchKernelGGL(pool_local_kernel<1>, dim3(nb), dim3(64 * POOL_WAVES), 0, stream, in, in_ld, C, nbr, ld, K, V_out, mode,
                       out, out_ld, a);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

int sv_pool_local_backward(const float* dy, int64_t V_out, int64_t dy_ld, int C, const int32_t* nbr_t, int64_t ld_t, int K,
                           int64_t V_in, int mode, const int32_t* arg, const uint32_t* mask_fwd, float* dx, int64_t dx_ld,
                           sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(C >= 1 && dy_ld >= C && dx_ld >= C && V_in >= 0 && V_out >= 0, "bad shape");
  SV_CHECK_ARG(K >= 1 && K <= 32, "K must be in 1..32");
  SV_CHECK_ARG(ld_t >= V_in, "bad shape (ld_t < V_in)");
  SV_CHECK_ARG(mode == SV_POOL_MAX || mode == SV_POOL_AVG || mode == SV_POOL_SUM, "bad mode");
  SV_CHECK_ARG(V_out < (1ll << 31) && V_in < (1ll << 31) - 1024, "row count out of range");
  if (V_in == 0) return SV_OK;
  SV_CHECK_ARG(nbr_t && dx && (dy || V_out == 0), "null pointer");
  SV_CHECK_ARG(mode != SV_POOL_MAX || arg || V_out == 0, "null pointer (max pooling needs arg)");
  SV_CHECK_ARG(mode != SV_POOL_AVG || mask_fwd || V_out == 0, "null pointer (average pooling needs the forward mask)");
  const int64_t total = V_in * C;
  hipLaunchKernelGGL(pool_local_backward_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, dy, dy_ld, C,
                     nbr_t, ld_t, K, V_in, mode, arg, mask_fwd, dx, dx_ld);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

}  // extern "C"
