// PointNet++ training on libsvhip (set_training_path "hip"): the gather, pooling and interpolation work around the
// shared-MLP GEMMs (which run on sv_conv_fwd / sv_conv_wgrad as dense rows) and its backward.
//
//   sv_group_rows          the grouped rows of a set abstraction      model/pointnet2_utils.py:131-137 / :245-250 / :143-160
//   sv_index_transpose     CSR inverse of a ball-query / 3-NN table   (replaces the atomic scatter of index_points' backward)
//   sv_gather_transpose    dPoints from dRows over that CSR, fixed order
//   sv_group_max(_backward) torch.max(t, 2) of the set abstraction   :203 / :258, and its gradient
//   sv_three_nn(_gather)   the 3-NN search + weights and the weighted gather of PointNetFeaturePropagation  :298-305
//
// No float atomics anywhere: every sum runs in a fixed order, so two identical steps give identical bits.  Plain
// element-per-thread kernels: these layers are thin (3 .. 1024 columns) and bound by memory traffic.
#include "sv_common.h"
#include "sv_pointnet_dev.h"

namespace sv {

constexpr int PG_THREADS = 256;
constexpr int64_t PG_MAX_ELEMS = (int64_t)1 << 31;  // flat element counts are decoded in 32-bit arithmetic

static unsigned pg_blocks(int64_t n) {
  const int64_t b = (n + PG_THREADS - 1) / PG_THREADS;
  return (unsigned)(b < 1 ? 1 : b);
}

// ---- grouped rows ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PG_THREADS) void group_rows_kernel(const float* __restrict__ xyz,
                                                                const float* __restrict__ points,
                                                                const float* __restrict__ new_xyz,
                                                                const int64_t* __restrict__ idx, int N, int D, int S,
                                                                int nsample, int order, int ld, uint32_t total,
                                                                float* __restrict__ out) {
  const uint32_t e = blockIdx.x * PG_THREADS + threadIdx.x;
  if (e >= total) return;
  const uint32_t row = e / (uint32_t)ld;
  const int col = (int)(e - row * (uint32_t)ld);
  const uint32_t g = row / (uint32_t)nsample;  // (b, s)
  out[e] = col < 3 + D ? pn_group_element(xyz, points, new_xyz, idx, g / (uint32_t)S, g, (int)(row - g * (uint32_t)nsample),
                                          nsample, N, D, order, col)
                       : 0.0f;
}

// ---- index transpose (CSR over the targets) ------------------------------------------------------------------------
template <typename IdxT>
__global__ __launch_bounds__(PG_THREADS) void transpose_keys_kernel(const IdxT* __restrict__ idx, uint32_t M, uint32_t N,
                                                                    uint32_t total, uint32_t sentinel,
                                                                    uint32_t* __restrict__ keys) {
  const uint32_t e = blockIdx.x * PG_THREADS + threadIdx.x;
  if (e >= total) return;
  const int64_t v = (int64_t)idx[e];
  keys[e] = (v >= 0 && v < (int64_t)N) ? (e / M) * N + (uint32_t)v : sentinel;
}

// offsets[t] = first sorted position whose key is >= t (lower bound), t = 0 .. T
__global__ __launch_bounds__(PG_THREADS) void transpose_offsets_kernel(const uint32_t* __restrict__ keys, uint32_t n,
                                                                       uint32_t T, int32_t* __restrict__ offsets) {
  const uint32_t t = blockIdx.x * PG_THREADS + threadIdx.x;
  if (t > T) return;
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (keys[mid] < t) lo = mid + 1;
    else hi = mid;
  }
  offsets[t] = (int32_t)lo;
}

__global__ __launch_bounds__(PG_THREADS) void gather_transpose_kernel(const int32_t* __restrict__ offsets,
                                                                      const int32_t* __restrict__ pos,
                                                                      const float* __restrict__ w,
                                                                      const float* __restrict__ rows, int64_t ld_rows,
                                                                      int col0, int C, int per_row, uint32_t total,
                                                                      float* __restrict__ out, int64_t ld_out) {
  const uint32_t e = blockIdx.x * PG_THREADS + threadIdx.x;
  if (e >= total) return;
  const uint32_t t = e / (uint32_t)C;
  const int c = (int)(e - t * (uint32_t)C);
  const int32_t p0 = offsets[t], p1 = offsets[t + 1];
  float acc = 0.0f;
  for (int32_t q = p0; q < p1; ++q) {
    const int32_t p = pos[q];
    const float v = rows[(int64_t)(p / per_row) * ld_rows + col0 + c];
    acc = __fadd_rn(acc, w ? __fmul_rn(w[p], v) : v);
  }
  out[(int64_t)t * ld_out + c] = acc;
}

// ---- max over groups ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PG_THREADS) void group_max_kernel(const float* __restrict__ rows, int64_t ld, int nsample,
                                                               int C, uint32_t total, float* __restrict__ out,
                                                               int32_t* __restrict__ arg) {
  const uint32_t e = blockIdx.x * PG_THREADS + threadIdx.x;
  if (e >= total) return;
  const uint32_t g = e / (uint32_t)C;
  const int c = (int)(e - g * (uint32_t)C);
  const float* r = rows + (int64_t)g * nsample * ld + c;
  float m = r[0];
  int a = 0;
  for (int k = 1; k < nsample; ++k) {
    const float v = r[(int64_t)k * ld];
    if (!(m != m) && (v > m || v != v)) {  // the first NaN stays; otherwise a strictly larger value or a NaN takes over
      m = v;
      a = k;
    }
  }
  out[e] = m;
  arg[e] = a;
}

__global__ __launch_bounds__(PG_THREADS) void group_max_backward_kernel(const float* __restrict__ dpooled,
                                                                        const int32_t* __restrict__ arg, int nsample,
                                                                        int C, uint32_t total, float* __restrict__ drows) {
  const uint32_t e = blockIdx.x * PG_THREADS + threadIdx.x;
  if (e >= total) return;
  const uint32_t row = e / (uint32_t)C;
  const uint32_t c = e - row * (uint32_t)C;
  const uint32_t g = row / (uint32_t)nsample;
  const int k = (int)(row - g * (uint32_t)nsample);
  const uint32_t o = g * (uint32_t)C + c;
  drows[e] = arg[o] == k ? dpooled[o] : 0.0f;
}

// ---- 3-NN search and weighted gather -------------------------------------------------------------------------------
// sv_three_nn_interpolate (sv_points.hip) in two launches, so that the neighbours and weights can be kept for the
// backward: the same three_nn_search and three_nn_mix (sv_pointnet_dev.h), here with one query per thread.
static_assert(PG_THREADS == NN_THREADS, "three_nn_search stages NN_THREADS points per step");

__global__ __launch_bounds__(PG_THREADS) void three_nn_kernel(const float* __restrict__ xyz1,
                                                              const float* __restrict__ xyz2, int N, int S,
                                                              int32_t* __restrict__ idx, float* __restrict__ w) {
  const int b = blockIdx.y;
  const int q = blockIdx.x * PG_THREADS + threadIdx.x;
  int32_t qi[3];
  float qw[3];
  three_nn_search(xyz1 + (int64_t)b * N * 3, xyz2 + (int64_t)b * S * 3, S, q, q < N, qi, qw);
  if (q >= N) return;
  const int64_t o = ((int64_t)b * N + q) * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    idx[o + k] = qi[k];
    w[o + k] = qw[k];
  }
}

__global__ __launch_bounds__(PG_THREADS) void three_nn_gather_kernel(const float* __restrict__ points2,
                                                                     const int32_t* __restrict__ idx,
                                                                     const float* __restrict__ w, int N, int S, int C,
                                                                     uint32_t total, float* __restrict__ out) {
  const uint32_t e = blockIdx.x * PG_THREADS + threadIdx.x;
  if (e >= total) return;
  const uint32_t row = e / (uint32_t)C;  // b * N + n
  const int c = (int)(e - row * (uint32_t)C);
  const float* p2 = points2 + (int64_t)(row / (uint32_t)N) * S * C;
  const int32_t* ix = idx + (int64_t)row * 3;
  if ((uint32_t)ix[0] >= (uint32_t)S || (uint32_t)ix[1] >= (uint32_t)S || (uint32_t)ix[2] >= (uint32_t)S) {
    out[e] = NAN;  // an index outside the source cloud reads nothing
    return;
  }
  out[e] = three_nn_mix(p2, C, c, ix, w + (int64_t)row * 3);
}

static int bits_for(uint64_t v) {  // bits that hold every value 0 .. v
  int n = 0;
  while (n < 64 && (v >> n) != 0) ++n;
  return n;
}

}  // namespace sv

using namespace sv;

extern "C" {

int sv_group_rows(const float* xyz, const float* points, const float* new_xyz, const int64_t* idx, int B, int N, int D,
                  int S, int nsample, int order, int ld, float* out, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(B >= 0 && N >= 1 && D >= 0 && S >= 1 && nsample >= 1, "bad shape");
  SV_CHECK_ARG(order == SV_GROUP_SSG || order == SV_GROUP_MSG, "order must be SV_GROUP_SSG or SV_GROUP_MSG");
  SV_CHECK_ARG(ld >= 3 + D, "ld must be at least 3 + D");
  SV_CHECK_ARG(idx || (S == 1 && nsample == N && order == SV_GROUP_SSG),
               "group_all (idx NULL) needs S = 1, nsample = N and the SSG order");
  SV_CHECK_ARG((int64_t)B * S * nsample * ld < PG_MAX_ELEMS, "too many elements");
  if (B == 0) return SV_OK;
  SV_CHECK_ARG(xyz && out && (D == 0 || points) && (!idx || new_xyz), "null pointer");
  const int64_t total = (int64_t)B * S * nsample * ld;
  hipLaunchKernelGGL(group_rows_kernel, dim3(pg_blocks(total)), dim3(PG_THREADS), 0, stream, xyz, points, new_xyz, idx, N,
                     D, S, nsample, order, ld, (uint32_t)total, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

size_t sv_index_transpose_workspace_bytes(int B, int64_t M, int N) {
  (void)N;
  const int64_t n = (B > 0 && M > 0) ? (int64_t)B * M : 0;
  return 2 * align_up((size_t)n * 4, 256) + radix_sort_temp_bytes(n, 4) + 512;
}

int sv_index_transpose(const void* idx, int idx_bytes, int B, int64_t M, int N, void* workspace, size_t workspace_bytes,
                       int32_t* offsets, int32_t* pos, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(idx_bytes == 4 || idx_bytes == 8, "idx_bytes must be 4 or 8");
  SV_CHECK_ARG(B >= 0 && M >= 0 && N >= 1, "bad shape");
  SV_CHECK_ARG((int64_t)B * M < PG_MAX_ELEMS && (int64_t)B * N < PG_MAX_ELEMS, "too many entries");
  SV_CHECK_ARG(offsets && (B == 0 || M == 0 || (idx && pos)), "null pointer");
  const size_t need = sv_index_transpose_workspace_bytes(B, M, N);
  if (workspace_bytes < need || (need > 0 && !workspace)) {
    set_error("sv_index_transpose: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    return SV_ERR_WORKSPACE;
  }
  const uint32_t n = (uint32_t)((int64_t)B * M);
  const uint32_t T = (uint32_t)((int64_t)B * N);
  Workspace ws(workspace, workspace_bytes);
  uint32_t* keys = ws.take<uint32_t>(n);
  uint32_t* sorted = ws.take<uint32_t>(n);
  const size_t tbytes = radix_sort_temp_bytes(n, 4);
  void* temp = ws.take<char>(tbytes);
  if (!ws.ok) {
    set_error("sv_index_transpose: workspace too small");
    return SV_ERR_WORKSPACE;
  }
  if (n > 0) {
    if (idx_bytes == 8)
      hipLaunchKernelGGL(transpose_keys_kernel<int64_t>, dim3(pg_blocks(n)), dim3(PG_THREADS), 0, stream,
                         (const int64_t*)idx, (uint32_t)M, (uint32_t)N, n, T, keys);
    else
      hipLaunchKernelGGL(transpose_keys_kernel<int32_t>, dim3(pg_blocks(n)), dim3(PG_THREADS), 0, stream,
                         (const int32_t*)idx, (uint32_t)M, (uint32_t)N, n, T, keys);
    SV_LAUNCH_CHECK();
    const int rc = radix_sort_pairs<uint32_t>(keys, nullptr, sorted, pos, n, 0, bits_for(T), temp, tbytes, stream);
    if (rc != SV_OK) return rc;
  }
  hipLaunchKernelGGL(transpose_offsets_kernel, dim3(pg_blocks((int64_t)T + 1)), dim3(PG_THREADS), 0, stream, sorted, n, T,
                     offsets);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

int sv_gather_transpose(const int32_t* offsets, const int32_t* pos, const float* w, const float* rows, int64_t ld_rows,
                        int col0, int C, int per_row, int64_t T, float* out, int64_t ld_out, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(T >= 0 && C >= 1 && col0 >= 0 && per_row >= 1, "bad shape");
  SV_CHECK_ARG(ld_rows >= col0 + C && ld_out >= C, "row strides too small");
  SV_CHECK_ARG(T * C < PG_MAX_ELEMS, "too many elements");
  if (T == 0) return SV_OK;
  SV_CHECK_ARG(offsets && pos && rows && out, "null pointer");
  const int64_t total = T * C;
  hipLaunchKernelGGL(gather_transpose_kernel, dim3(pg_blocks(total)), dim3(PG_THREADS), 0, stream, offsets, pos, w, rows,
                     ld_rows, col0, C, per_row, (uint32_t)total, out, ld_out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

int sv_group_max(const float* rows, int64_t ld, int64_t G, int nsample, int C, float* out, int32_t* arg,
                 sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(G >= 0 && nsample >= 1 && C >= 1 && ld >= C, "bad shape");
  SV_CHECK_ARG(G * C < PG_MAX_ELEMS, "too many elements");
  if (G == 0) return SV_OK;
  SV_CHECK_ARG(rows && out && arg, "null pointer");
  const int64_t total = G * C;
  hipLaunchKernelGGL(group_max_kernel, dim3(pg_blocks(total)), dim3(PG_THREADS), 0, stream, rows, ld, nsample, C,
                     (uint32_t)total, out, arg);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

int sv_group_max_backward(const float* dpooled, const int32_t* arg, int64_t G, int nsample, int C, float* drows,
                          sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(G >= 0 && nsample >= 1 && C >= 1, "bad shape");
  SV_CHECK_ARG(G * nsample * C < PG_MAX_ELEMS, "too many elements");
  if (G == 0) return SV_OK;
  SV_CHECK_ARG(dpooled && arg && drows, "null pointer");
  const int64_t total = G * nsample * C;
  hipLaunchKernelGGL(group_max_backward_kernel, dim3(pg_blocks(total)), dim3(PG_THREADS), 0, stream, dpooled, arg,
                     nsample, C, (uint32_t)total, drows);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

int sv_three_nn(const float* xyz1, const float* xyz2, int B, int N, int S, int32_t* idx, float* w, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(B >= 0 && N >= 1 && S >= 3, "bad shape (S >= 3 source points)");
  SV_CHECK_ARG(B <= 65535, "B above the grid limit");
  if (B == 0) return SV_OK;
  SV_CHECK_ARG(xyz1 && xyz2 && idx && w, "null pointer");
  hipLaunchKernelGGL(three_nn_kernel, dim3((unsigned)((N + PG_THREADS - 1) / PG_THREADS), (unsigned)B), dim3(PG_THREADS),
                     0, stream, xyz1, xyz2, N, S, idx, w);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

int sv_three_nn_gather(const float* points2, const int32_t* idx, const float* w, int B, int N, int S, int C, float* out,
                       sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(B >= 0 && N >= 1 && S >= 3 && C >= 1, "bad shape (S >= 3 source points)");
  SV_CHECK_ARG((int64_t)B * N * C < PG_MAX_ELEMS, "too many elements");
  if (B == 0) return SV_OK;
  SV_CHECK_ARG(points2 && idx && w && out, "null pointer");
  const int64_t total = (int64_t)B * N * C;
  hipLaunchKernelGGL(three_nn_gather_kernel, dim3(pg_blocks(total)), dim3(PG_THREADS), 0, stream, points2, idx, w, N, S, C,
                     (uint32_t)total, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

}  // extern "C"
