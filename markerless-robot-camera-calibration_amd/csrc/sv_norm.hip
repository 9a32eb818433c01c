// Instance normalisation of a batched sparse tensor (ME.MinkowskiInstanceNorm, model/backbone/resnet.py:55,78), with the
// activation that follows it fused (ReLU :56, GELU :79), and its backward.
//
// A frame's rows are contiguous (the batch index is the key's top bits), so the statistics are segment reductions over
// batch_start ranges (sv_batch_offsets).  Everything is float64.  Fixed summation tree per (frame, channel): a frame is cut
// into chunks of SV_NORM_CHUNK_ROWS rows; a workgroup's four waves each sum a quarter of a chunk sequentially in ascending
// row order, the quarters are added in ascending order, and a second stage adds a frame's chunks in ascending order.  No
// atomics: the same bits on every run.  Lanes run along the channels (coalesced rows).
#include "sv_common.h"

namespace sv {

constexpr int NORM_WAVES = 4;
constexpr int NORM_SUB = SV_NORM_CHUNK_ROWS / NORM_WAVES;  // rows one wave sums
static_assert(SV_NORM_CHUNK_ROWS % NORM_WAVES == 0, "chunk must split evenly over the waves");

// Partial-sum slot of chunk j of frame b that starts at row s: frames never share a slot and the slots of all frames fit into
// V / CHUNK + B + 1 (floor(s / CHUNK) + ceil(n / CHUNK) <= floor((s + n) / CHUNK) + 1).
__device__ __forceinline__ int64_t norm_slot(int s, int b, int j) { return (int64_t)(s / SV_NORM_CHUNK_ROWS) + b + j; }

__device__ __forceinline__ double norm_act(double y, int act) {
  if (act == SV_ACT_RELU) return y > 0.0 ? y : (y != y ? y : 0.0);
  if (act == SV_ACT_GELU) return 0.5 * y * (1.0 + erf(y * 0.70710678118654752440));
  return y;
}
__device__ __forceinline__ double norm_act_grad(double y, int act) {
  if (act == SV_ACT_RELU) return y > 0.0 ? 1.0 : 0.0;
  if (act == SV_ACT_GELU)
    return 0.5 * (1.0 + erf(y * 0.70710678118654752440)) + y * 0.39894228040143267794 * exp(-0.5 * y * y);
  return 1.0;
}

// WHAT 0: sum x.  1: sum (x - mean)^2.  2: sum dy' and sum dy' * xhat, dy' = dy * act'(pre-activation).
template <int WHAT>
__global__ __launch_bounds__(64 * NORM_WAVES) void norm_partial_kernel(
    const float* __restrict__ x, int64_t V, int64_t ld, int C, const int32_t* __restrict__ batch_start,
    const double* __restrict__ mean, const double* __restrict__ inv_std, const float* __restrict__ weight, const float* __restrict__ bias, int act,
    const float* __restrict__ dy, int64_t dy_ld, double* __restrict__ part0, double* __restrict__ part1) {
  __shared__ double sh[2][NORM_WAVES][64];
  const int b = blockIdx.y, j = blockIdx.x;
  const int s = batch_start[b], e = min(batch_start[b + 1], (int)V);  // never past the rows the caller owns
  const int r0 = s + j * SV_NORM_CHUNK_ROWS;
  if (r0 >= e) return;  // uniform over the workgroup
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.z * 64 + lane;
  double a0 = 0.0, a1 = 0.0;
  if (c < C) {
    const int q0 = r0 + w * NORM_SUB;
    const int q1 = min(q0 + NORM_SUB, e);
    double m = 0.0, is = 0.0, wt = 0.0, bs = 0.0;
    if (WHAT >= 1) m = mean[(int64_t)b * C + c];
    if (WHAT == 2) {
      is = inv_std[(int64_t)b * C + c];
      wt = (double)weight[c];
      bs = (double)bias[c];
    }
    for (int r = q0; r < q1; ++r) {
      const double v = (double)x[(int64_t)r * ld + c];
      if (WHAT == 0) {
        a0 += v;
      } else if (WHAT == 1) {
        const double d = v - m;
        a0 += d * d;
      } else {
        const double xh = (v - m) * is;
        const double g = (double)dy[(int64_t)r * dy_ld + c] * norm_act_grad(xh * wt + bs, act);
        a0 += g;
        a1 += g * xh;
      }
    }
  }
  sh[0][w][lane] = a0;
  if (WHAT == 2) sh[1][w][lane] = a1;
  __syncthreads();
  if (w == 0 && c < C) {
    const int64_t slot = norm_slot(s, b, j) * C + c;
    double t = sh[0][0][lane];
    for (int i = 1; i < NORM_WAVES; ++i) t += sh[0][i][lane];
    part0[slot] = t;
    if (WHAT == 2) {
      t = sh[1][0][lane];
      for (int i = 1; i < NORM_WAVES; ++i) t += sh[1][i][lane];
      part1[slot] = t;
    }
  }
}

// second stage, one thread per (frame, channel): a frame's chunks in ascending order
template <int WHAT>
__global__ __launch_bounds__(256) void norm_combine_kernel(const int32_t* __restrict__ batch_start, int64_t V, int B, int C, double eps,
                                                            const double* __restrict__ part0, const double* __restrict__ part1,
                                                            double* __restrict__ out0, double* __restrict__ out1) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= B * C) return;
  const int b = t / C, c = t - b * C;
  const int s = batch_start[b], n = max(min(batch_start[b + 1], (int)V) - s, 0);
  const int chunks = (n + SV_NORM_CHUNK_ROWS - 1) / SV_NORM_CHUNK_ROWS;
  double a0 = 0.0, a1 = 0.0;
  for (int j = 0; j < chunks; ++j) {
    a0 += part0[norm_slot(s, b, j) * C + c];
    if (WHAT == 2) a1 += part1[norm_slot(s, b, j) * C + c];
  }
  if (WHAT == 0) out0[t] = n > 0 ? a0 / (double)n : 0.0;                     // mean
  if (WHAT == 1) out0[t] = n > 0 ? 1.0 / sqrt(a0 / (double)n + eps) : 0.0;  // 1 / sqrt(biased variance + eps)
  if (WHAT == 2) {
    out0[t] = a0;
    out1[t] = a1;
  }
}

__global__ __launch_bounds__(256) void norm_apply_kernel(const float* __restrict__ x, int64_t ld, int C, int64_t V,
                                                          const int32_t* __restrict__ batch_start, int B,
                                                          const double* __restrict__ mean, const double* __restrict__ inv_std,
                                                          const float* __restrict__ weight, const float* __restrict__ bias,
                                                          int act, float* __restrict__ y, int64_t y_ld) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= V * C) return;
  const int64_t r = t / C;
  const int c = (int)(t - r * C);
  // frame of row r: the last b with batch_start[b] <= r (empty frames share their start with the next one)
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (batch_start[mid] <= r) lo = mid; else hi = mid;
  }
  if (r < batch_start[0] || r >= batch_start[B]) return;
  const int64_t bc = (int64_t)lo * C + c;
  const double v = ((double)x[r * ld + c] - mean[bc]) * inv_std[bc] * (double)weight[c] + (double)bias[c];
  y[r * y_ld + c] = (float)norm_act(v, act);
}

__global__ __launch_bounds__(256) void norm_backward_apply_kernel(
    const float* __restrict__ x, int64_t ld, int C, int64_t V, const int32_t* __restrict__ batch_start, int B,
    const double* __restrict__ mean, const double* __restrict__ inv_std, const float* __restrict__ weight,
    const float* __restrict__ bias, int act, const float* __restrict__ dy, int64_t dy_ld, const double* __restrict__ sum_g,
    const double* __restrict__ sum_gx, float* __restrict__ dx, int64_t dx_ld) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= V * C) return;
  const int64_t r = t / C;
  const int c = (int)(t - r * C);
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (batch_start[mid] <= r) lo = mid; else hi = mid;
  }
  if (r < batch_start[0] || r >= batch_start[B]) return;
  const int64_t bc = (int64_t)lo * C + c;
  const double n = (double)(batch_start[lo + 1] - batch_start[lo]);
  const double w = (double)weight[c], is = inv_std[bc];
  const double xh = ((double)x[r * ld + c] - mean[bc]) * is;
  const double g = (double)dy[r * dy_ld + c] * norm_act_grad(xh * w + (double)bias[c], act) * w;
  dx[r * dx_ld + c] = (float)(is * (g - w * sum_g[bc] / n - xh * (w * sum_gx[bc] / n)));
}

// dweight[c] = sum over frames (ascending b) of sum dy' * xhat, dbias[c] = ... of sum dy'
__global__ __launch_bounds__(256) void norm_param_grad_kernel(const double* __restrict__ sum_g, const double* __restrict__ sum_gx,
                                                               int B, int C, float* __restrict__ dweight,
                                                               float* __restrict__ dbias) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double a = 0.0, g = 0.0;
  for (int b = 0; b < B; ++b) {
    g += sum_g[(int64_t)b * C + c];
    a += sum_gx[(int64_t)b * C + c];
  }
  if (dweight) dweight[c] = (float)a;
  if (dbias) dbias[c] = (float)g;
}

static size_t norm_slots(int64_t V, int B) { return (size_t)(V / SV_NORM_CHUNK_ROWS) + (size_t)B + 2; }

}  // namespace sv

using namespace sv;

extern "C" {

size_t sv_instance_norm_workspace_bytes(int64_t V, int B, int C) {
  if (V <= 0 || B <= 0 || C <= 0) return 256;
  return 2 * align_up(norm_slots(V, B) * (size_t)C * sizeof(double), 256) + 2 * align_up((size_t)B * C * sizeof(double), 256) + 1024;
}

static int norm_check(const char* fn, int64_t V, int64_t ld, int C, int B, int act) {
  if (!(C >= 1 && ld >= C && V >= 0 && V < (1ll << 31) - 1024 && B >= 1 && B <= SV_MAX_BATCH)) {
    set_error("%s: bad shape", fn);
    return SV_ERR_INVALID;
  }
  if (!(act == SV_ACT_NONE || act == SV_ACT_RELU || act == SV_ACT_GELU)) {
    set_error("%s: activation must be SV_ACT_NONE, SV_ACT_RELU or SV_ACT_GELU", fn);
    return SV_ERR_INVALID;
  }
  return SV_OK;
}

int sv_instance_norm(const float* x, int64_t V, int64_t ld, int C, const int32_t* batch_start, int B, const float* weight,
                     const float* bias, double eps, int act, void* workspace, size_t workspace_bytes, float* y, int64_t y_ld,
                     double* mean, double* inv_std, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = norm_check(__func__, V, ld, C, B, act);
  if (rc) return rc;
  SV_CHECK_ARG(y_ld >= C && eps >= 0.0, "bad shape");
  SV_CHECK_ARG(batch_start && weight && bias && mean && inv_std && workspace && (V == 0 || (x && y)), "null pointer");
  Workspace ws(workspace, workspace_bytes);
  double* part = ws.take<double>(norm_slots(V, B) * (size_t)C);
  if (!ws.ok) {
    set_error("sv_instance_norm: workspace too small (%zu given)", workspace_bytes);
    return SV_ERR_WORKSPACE;
  }
  const dim3 pgrid((unsigned)((V + SV_NORM_CHUNK_ROWS - 1) / SV_NORM_CHUNK_ROWS), (unsigned)B, (unsigned)((C + 63) / 64));
  const unsigned cb = (unsigned)(((int64_t)B * C + 255) / 256);
  if (V > 0)
    hipLaunchKernelGGL(norm_partial_kernel<0>, pgrid, dim3(64 * NORM_WAVES), 0, stream, x, V, ld, C, batch_start, nullptr, nullptr,
                       nullptr, nullptr, act, nullptr, 0, part, nullptr);
  hipLaunchKernelGGL(norm_combine_kernel<0>, dim3(cb), dim3(256), 0, stream, batch_start, V, B, C, eps, part, nullptr, mean, nullptr);
  if (V > 0)
    hipLaunchKernelGGL(norm_partial_kernel<1>, pgrid, dim3(64 * NORM_WAVES), 0, stream, x, V, ld, C, batch_start, mean, nullptr,
                       nullptr, nullptr, act, nullptr, 0, part, nullptr);
  hipLaunchKernelGGL(norm_combine_kernel<1>, dim3(cb), dim3(256), 0, stream, batch_start, V, B, C, eps, part, nullptr, inv_std,
                     nullptr);
  if (V > 0)
    hipLaunchKernelGGL(norm_apply_kernel, dim3((unsigned)((V * C + 255) / 256)), dim3(256), 0, stream, x, ld, C, V,
                       batch_start, B, mean, inv_std, weight, bias, act, y, y_ld);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

int sv_instance_norm_backward(const float* x, int64_t V, int64_t ld, int C, const int32_t* batch_start, int B, const float* weight,
                              const float* bias, const double* mean, const double* inv_std, int act, const float* dy,
                              int64_t dy_ld, void* workspace, size_t workspace_bytes, float* dx, int64_t dx_ld, float* dweight,
                              float* dbias, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = norm_check(__func__, V, ld, C, B, act);
  if (rc) return rc;
  SV_CHECK_ARG(dy_ld >= C && dx_ld >= C, "bad shape");
  SV_CHECK_ARG(batch_start && weight && bias && mean && inv_std && workspace && (V == 0 || (x && dy && dx)), "null pointer");
  Workspace ws(workspace, workspace_bytes);
  const size_t slots = norm_slots(V, B) * (size_t)C;
  double* part0 = ws.take<double>(slots);
  double* part1 = ws.take<double>(slots);
  double* sum_g = ws.take<double>((size_t)B * C);
  double* sum_gx = ws.take<double>((size_t)B * C);
  if (!ws.ok) {
    set_error("sv_instance_norm_backward: workspace too small (%zu given)", workspace_bytes);
    return SV_ERR_WORKSPACE;
  }
  const dim3 pgrid((unsigned)((V + SV_NORM_CHUNK_ROWS - 1) / SV_NORM_CHUNK_ROWS), (unsigned)B, (unsigned)((C + 63) / 64));
  const unsigned cb = (unsigned)(((int64_t)B * C + 255) / 256);
  if (V > 0)
    hipLaunchKernelGGL(norm_partial_kernel<2>, pgrid, dim3(64 * NORM_WAVES), 0, stream, x, V, ld, C, batch_start, mean,
                       inv_std, weight, bias, act, dy, dy_ld, part0, part1);
  hipLaunchKernelGGL(norm_combine_kernel<2>, dim3(cb), dim3(256), 0, stream, batch_start, V, B, C, 0.0, part0, part1, sum_g, sum_gx);
  if (V > 0)
    hipLaunchKernelGGL(norm_backward_apply_kernel, dim3((unsigned)((V * C + 255) / 256)), dim3(256), 0, stream, x, ld, C, V,
                       batch_start, B, mean, inv_std, weight, bias, act, dy, dy_ld, sum_g, sum_gx, dx, dx_ld);
  if (dweight || dbias)
    hipLaunchKernelGGL(norm_param_grad_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, stream, sum_g, sum_gx, B, C,
                       dweight, dbias);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

}  // extern "C"
