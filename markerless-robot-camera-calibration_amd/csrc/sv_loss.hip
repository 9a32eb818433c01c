// N4: the four point-matching pose losses of the reference's utils/loss.py (:166-188 pose, :190-209 shape_match,
// :211-227 pose_match, :229-249 kp_pose_match) with their gradients, for a whole batch in one launch sequence.  The
// reference loops over the batch in Python with a dozen small torch ops per instance (shape_match also builds an
// [n, 3, n] difference tensor); here every instance's rows are walked once, in float64, and loss and gradient come from
// the same pass.  The contract (residuals, terms, rounding, edge cases) is in include/sv_hip.h.
//
//   loss_plan_kernel    1 workgroup: first workgroup of every instance (prefix sum of ceil(rows / 256)), so that the
//                       grid depends on (M, B) only - ceil(M / 256) + B workgroups - and no workgroup straddles instances
//   loss_search_kernel  SHAPE_MATCH only: one thread per query row; the instance's rotated target rows pass through a
//                       1024-row float64 LDS tile (24 KB; every lane reads the same address: a broadcast, no bank
//                       conflict) and each thread keeps its running (min, index), first minimum winning
//   loss_reduce_kernel  one thread per row: 14 float64 partial sums (rows, loss, 9 of dR, 3 of dt) reduced by shuffles,
//                       then through LDS in wave order; one partial per workgroup to the workspace
//   loss_finish_kernel  one wave per instance: thread c adds component c of the instance's partials in ascending
//                       workgroup order, divides, rounds once to float32 and writes
// No atomics and no data-dependent order anywhere: two runs give the same bits, and an instance's outputs depend on
// that instance's rows alone.
#include "sv_common.h"

namespace sv {

constexpr int LOSS_BLOCK = 256;
constexpr int LOSS_TILE = 1024;
constexpr int LOSS_NSUM = 14;  // [0] unmasked rows, [1] sum of terms, [2..10] sum of g p^T (row-major), [11..13] sum of g

struct LossRange {
  int b, lo, hi, first;  // instance, its row range [lo, hi) and the first row of this workgroup
};

// rows of instance b, whatever `offsets` holds: both ends inside [0, M] and hi >= lo, so no row index leaves the arrays
__device__ __forceinline__ void loss_instance_rows(const int32_t* __restrict__ offsets, int b, int M, int& lo, int& hi) {
  lo = min(max(offsets[b], 0), M);
  hi = min(max(offsets[b + 1], lo), M);
}

__global__ __launch_bounds__(1024) void loss_plan_kernel(const int32_t* __restrict__ offsets, int M, int B,
                                                         int32_t* __restrict__ blk_start) {
  __shared__ int scan[1024];
  const int b = threadIdx.x;
  int cnt = 0;
  if (b < B) {
    int lo, hi;
    loss_instance_rows(offsets, b, M, lo, hi);
    cnt = (hi - lo + LOSS_BLOCK - 1) / LOSS_BLOCK;
  }
  scan[b] = cnt;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int v = b >= d ? scan[b - d] : 0;
    __syncthreads();
    scan[b] += v;
    __syncthreads();
  }
  if (b < B) blk_start[b + 1] = scan[b];
  if (b == 0) blk_start[0] = 0;
}

// the instance whose workgroups include workgroup g (empty instances own none); false past the last one
__device__ __forceinline__ bool loss_resolve(const int32_t* __restrict__ blk_start, const int32_t* __restrict__ offsets,
                                             int M, int B, int g, LossRange& r) {
  if (g >= blk_start[B]) return false;
  int lo = 0, hi = B;  // largest b with blk_start[b] <= g
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (blk_start[mid] <= g) lo = mid; else hi = mid;
  }
  r.b = lo;
  loss_instance_rows(offsets, lo, M, r.lo, r.hi);
  r.first = r.lo + (g - blk_start[lo]) * LOSS_BLOCK;
  return true;
}

__device__ __forceinline__ void loss_transform(const float* __restrict__ R, const float* __restrict__ t, int b, double x,
                                               double y, double z, double& ox, double& oy, double& oz) {
  const float* Rb = R + b * 9;
  ox = ((double)Rb[0] * x + (double)Rb[1] * y) + (double)Rb[2] * z;
  oy = ((double)Rb[3] * x + (double)Rb[4] * y) + (double)Rb[5] * z;
  oz = ((double)Rb[6] * x + (double)Rb[7] * y) + (double)Rb[8] * z;
  if (t) {
    ox += (double)t[b * 3];
    oy += (double)t[b * 3 + 1];
    oz += (double)t[b * 3 + 2];
  }
}

__global__ __launch_bounds__(LOSS_BLOCK) void loss_search_kernel(
    const float* __restrict__ points, const int32_t* __restrict__ offsets, int M, int B, const uint8_t* __restrict__ mask,
    const float* __restrict__ R, const float* __restrict__ t, const float* __restrict__ R_pred,
    const float* __restrict__ t_pred, const int32_t* __restrict__ blk_start, int32_t* __restrict__ kstar) {
  __shared__ double tile[LOSS_TILE * 3];
  LossRange r;
  if (!loss_resolve(blk_start, offsets, M, B, blockIdx.x, r)) return;  // uniform over the workgroup
  const int i = r.first + threadIdx.x;
  const bool live = i < r.hi && (!mask || mask[i]);
  double ax = 0, ay = 0, az = 0;
  if (live) loss_transform(R_pred, t_pred, r.b, points[i * 3], points[i * 3 + 1], points[i * 3 + 2], ax, ay, az);
  double best = INFINITY;
  int bi = -1;
  for (int base = r.lo; base < r.hi; base += LOSS_TILE) {
    const int n = min(LOSS_TILE, r.hi - base);
    __syncthreads();
    for (int e = threadIdx.x; e < n; e += LOSS_BLOCK) {
      const int k = base + e;
      double bx = NAN, by = NAN, bz = NAN;  // a masked-out row is nobody's match: its distances are NaN
      if (!mask || mask[k]) loss_transform(R, t, r.b, points[k * 3], points[k * 3 + 1], points[k * 3 + 2], bx, by, bz);
      tile[e * 3] = bx;
      tile[e * 3 + 1] = by;
      tile[e * 3 + 2] = bz;
    }
    __syncthreads();
    if (live) {
      for (int j = 0; j < n; ++j) {
        const double dx = ax - tile[j * 3], dy = ay - tile[j * 3 + 1], dz = az - tile[j * 3 + 2];
        const double d = (dx * dx + dy * dy) + dz * dz;
        if (d < best) {  // first minimum wins (ascending row); a NaN distance never matches
          best = d;
          bi = base + j;
        }
      }
    }
  }
  if (i < r.hi) kstar[i] = live && bi >= 0 ? bi - r.lo : -1;
}

template <int MODE>
__global__ __launch_bounds__(LOSS_BLOCK) void loss_reduce_kernel(
    const float* __restrict__ points, const int32_t* __restrict__ offsets, int M, int B,
    const float* __restrict__ weights, const uint8_t* __restrict__ mask, const float* __restrict__ R,
    const float* __restrict__ t, const float* __restrict__ R_pred, const float* __restrict__ t_pred,
    const int32_t* __restrict__ blk_start, const int32_t* __restrict__ kstar, double* __restrict__ partial) {
  __shared__ double red[LOSS_BLOCK / 64][LOSS_NSUM];
  LossRange r;
  if (!loss_resolve(blk_start, offsets, M, B, blockIdx.x, r)) return;  // uniform over the workgroup
  const int i = r.first + threadIdx.x;
  double s[LOSS_NSUM];
#pragma unroll
  for (int c = 0; c < LOSS_NSUM; ++c) s[c] = 0.0;
  if (i < r.hi && (!mask || mask[i])) {
    const double px = points[i * 3], py = points[i * 3 + 1], pz = points[i * 3 + 2];
    double ax, ay, az, bx, by, bz;
    loss_transform(R_pred, t_pred, r.b, px, py, pz, ax, ay, az);
    if (MODE == SV_LOSS_SHAPE_MATCH) {
      const int k = kstar[i];  // -1: every distance was NaN (non-finite inputs) -> the instance's outputs are NaN
      if (k >= 0 && k < r.hi - r.lo) {
        const int q = r.lo + k;
        loss_transform(R, t, r.b, points[q * 3], points[q * 3 + 1], points[q * 3 + 2], bx, by, bz);
      } else {
        bx = by = bz = NAN;
      }
    } else {
      loss_transform(R, t, r.b, px, py, pz, bx, by, bz);
    }
    const double rx = ax - bx, ry = ay - by, rz = az - bz;
    double gx, gy, gz, term;
    if (MODE == SV_LOSS_POSE_MATCH) {
      term = (fabs(rx) + fabs(ry)) + fabs(rz);
      // sign(r) with sign(0) = 0; a NaN residual stays NaN
      gx = rx > 0 ? 1.0 : (rx < 0 ? -1.0 : rx);
      gy = ry > 0 ? 1.0 : (ry < 0 ? -1.0 : ry);
      gz = rz > 0 ? 1.0 : (rz < 0 ? -1.0 : rz);
    } else {
      double w2 = 1.0;
      if (weights) {
        const double w = weights[i];
        w2 = w * w;
      }
      term = w2 * ((rx * rx + ry * ry) + rz * rz);
      gx = w2 * rx;
      gy = w2 * ry;
      gz = w2 * rz;
    }
    s[0] = 1.0;
    s[1] = term;
    s[2] = gx * px, s[3] = gx * py, s[4] = gx * pz;
    s[5] = gy * px, s[6] = gy * py, s[7] = gy * pz;
    s[8] = gz * px, s[9] = gz * py, s[10] = gz * pz;
    s[11] = gx, s[12] = gy, s[13] = gz;
  }
#pragma unroll
  for (int c = 0; c < LOSS_NSUM; ++c) {
    double v = s[c];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    s[c] = v;
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < LOSS_NSUM; ++c) red[threadIdx.x >> 6][c] = s[c];
  }
  __syncthreads();
  if (threadIdx.x < LOSS_NSUM) {
    double v = 0.0;
    for (int w = 0; w < LOSS_BLOCK / 64; ++w) v += red[w][threadIdx.x];  // wave order
    partial[(int64_t)blockIdx.x * LOSS_NSUM + threadIdx.x] = v;
  }
}

__global__ __launch_bounds__(64) void loss_finish_kernel(const int32_t* __restrict__ blk_start,
                                                         const double* __restrict__ partial, int nblk, int mode,
                                                         float* __restrict__ loss, float* __restrict__ grad_R,
                                                         float* __restrict__ grad_t) {
  __shared__ double tot[LOSS_NSUM];
  const int b = blockIdx.x, c = threadIdx.x;
  if (c < LOSS_NSUM) {
    const int g0 = min(blk_start[b], nblk), g1 = min(blk_start[b + 1], nblk);
    double v = 0.0;
    for (int g = g0; g < g1; ++g) v += partial[(int64_t)g * LOSS_NSUM + c];  // ascending workgroup order
    tot[c] = v;
  }
  __syncthreads();
  if (c >= LOSS_NSUM) return;
  const double n = tot[0];  // 0 rows: 0 / 0 = NaN for the loss and every gradient entry, as the reference's mean of nothing
  if (c == 0) return;
  if (c == 1) {
    loss[b] = (float)(mode == SV_LOSS_POSE_MATCH ? tot[1] / n : tot[1] / (2.0 * n));
  } else if (c < 11) {
    if (grad_R) grad_R[b * 9 + (c - 2)] = (float)(tot[c] / n);
  } else {
    if (grad_t) grad_t[b * 3 + (c - 11)] = (float)(tot[c] / n);
  }
}

static inline size_t loss_blocks(int64_t M, int B) { return (size_t)((M + LOSS_BLOCK - 1) / LOSS_BLOCK) + (size_t)B; }

}  // namespace sv

using namespace sv;

extern "C" {

size_t sv_pose_loss_workspace_bytes(int64_t M, int B) {
  if (M < 0) M = 0;
  if (B < 0) B = 0;
  return align_up((size_t)(B + 1) * 4, 256) + align_up(loss_blocks(M, B) * LOSS_NSUM * sizeof(double), 256) +
         align_up((size_t)M * 4, 256) + 256;
}

int sv_pose_match_loss(const float* points, const int32_t* offsets, int64_t M, int B, const float* weights,
                       const uint8_t* mask, const float* R, const float* t, const float* R_pred, const float* t_pred,
                       int mode, void* workspace, size_t workspace_bytes, float* loss, float* grad_R, float* grad_t,
                       int32_t* match, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(B >= 1 && B <= SV_MAX_BATCH, "need 1 to 1024 instances");
  SV_CHECK_ARG(M >= 0 && M < (1 << 24), "need 0 <= M < 2^24 rows");
  SV_CHECK_ARG(mode >= SV_LOSS_POSE && mode <= SV_LOSS_KP_POSE_MATCH, "bad mode");
  SV_CHECK_ARG((points || M == 0) && offsets && R && R_pred && loss && workspace, "null pointer");
  SV_CHECK_ARG((t == nullptr) == (t_pred == nullptr), "t and t_pred must be given together");
  SV_CHECK_ARG(t || !grad_t, "grad_t without a translation");
  SV_CHECK_ARG(!(weights && mode == SV_LOSS_POSE_MATCH), "POSE_MATCH takes no weights");
  SV_CHECK_ARG(!(match && mode != SV_LOSS_SHAPE_MATCH), "match is written by SHAPE_MATCH only");
  Workspace ws(workspace, workspace_bytes);
  const size_t nblk = loss_blocks(M, B);
  int32_t* blk_start = ws.take<int32_t>((size_t)B + 1);
  double* partial = ws.take<double>(nblk * LOSS_NSUM);
  int32_t* kstar = ws.take<int32_t>((size_t)M);
  if (!ws.ok) {
    set_error("sv_pose_match_loss: workspace too small");
    return SV_ERR_WORKSPACE;
  }
  if (match) kstar = match;
  const int Mi = (int)M;
  hipLaunchKernelGGL(loss_plan_kernel, dim3(1), dim3(1024), 0, stream, offsets, Mi, B, blk_start);
#define SV_LOSS_REDUCE(MODE)                                                                                           \
  hipLaunchKernelGGL(loss_reduce_kernel<MODE>, dim3((unsigned)nblk), dim3(LOSS_BLOCK), 0, stream, points, offsets, Mi, \
                     B, weights, mask, R, t, R_pred, t_pred, blk_start, kstar, partial)
  switch (mode) {
    case SV_LOSS_POSE:
      SV_LOSS_REDUCE(SV_LOSS_POSE);
      break;
    case SV_LOSS_SHAPE_MATCH:
      hipLaunchKernelGGL(loss_search_kernel, dim3((unsigned)nblk), dim3(LOSS_BLOCK), 0, stream, points, offsets, Mi, B,
                         mask, R, t, R_pred, t_pred, blk_start, kstar);
      SV_LOSS_REDUCE(SV_LOSS_SHAPE_MATCH);
      break;
    case SV_LOSS_POSE_MATCH:
      SV_LOSS_REDUCE(SV_LOSS_POSE_MATCH);
      break;
    default:
      SV_LOSS_REDUCE(SV_LOSS_KP_POSE_MATCH);
      break;
  }
#undef SV_LOSS_REDUCE
  hipLaunchKernelGGL(loss_finish_kernel, dim3(B), dim3(64), 0, stream, blk_start, partial, (int)nblk, mode, loss, grad_R,
                     grad_t);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

}  // extern "C"
