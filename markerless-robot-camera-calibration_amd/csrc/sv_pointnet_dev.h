// Device code shared by the PointNet++ kernels of sv_points.hip, sv_pointnet.hip and sv_pointnet_grad.hip: each rule
// below has one text, so the kernels that must agree bit for bit (fused and unfused set abstraction, eval and training
// interpolation) cannot drift apart.  Every user is compiled with -ffp-contract=off: the expressions round as written.
#pragma once

#include "sv_common.h"

namespace sv {

// One element of a grouped row (model/pointnet2_utils.py:131-137 / :245-250): column `col` < 3 + D of neighbour k of
// group g = (cloud b, centroid s) over xyz [B, N, 3] / points [B, N, D] / new_xyz [B, S, 3] / idx [B, S, nsample].
// Order SV_GROUP_SSG is [xyz[j] - new_xyz[g], points[j]], SV_GROUP_MSG [points[j], xyz[j] - new_xyz[g]] with
// j = idx[g][k].  idx NULL is group_all (:143-160): j = k and the coordinates stay as they are.  An index outside the
// cloud (an empty ball's N) reads nothing: NaN.
__device__ __forceinline__ float pn_group_element(const float* __restrict__ xyz, const float* __restrict__ points,
                                                  const float* __restrict__ new_xyz, const int64_t* __restrict__ idx,
                                                  int64_t b, int64_t g, int k, int nsample, int N, int D, int order,
                                                  int col) {
  const int64_t j = idx ? idx[g * nsample + k] : (int64_t)k;
  if (j < 0 || j >= N) return NAN;
  const int64_t src = b * N + j;
  const int xc = order == SV_GROUP_SSG ? col : col - D;  // coordinate column, or < 0 / >= 3 for a feature column
  if (xc >= 0 && xc < 3) {
    const float v = xyz[src * 3 + xc];
    return idx ? __fsub_rn(v, new_xyz[g * 3 + xc]) : v;
  }
  return points[src * D + (order == SV_GROUP_SSG ? col - 3 : col)];
}

// 3-NN search of PointNetFeaturePropagation.forward (model/pointnet2_utils.py:298-303) for a workgroup of NN_THREADS
// threads, every one of which must call it: thread `active` owns query q of x1 and walks the S points of x2 (staged
// through LDS, NN_THREADS at a time) with the reference's expanded float32 distance (-2 q.p + |q|^2) + |p|^2, keeping the
// three smallest (ascending, the first index wins a tie - the order of the reference's full sort); w = 1 / (d + 1e-8)
// normalised.  An inactive thread only helps staging; its results mean nothing.
constexpr int NN_THREADS = 256;

__device__ __forceinline__ void three_nn_search(const float* __restrict__ x1, const float* __restrict__ x2, int S, int q,
                                                bool active, int idx[3], float w[3]) {
  __shared__ float src[NN_THREADS * 3];
  float qx = 0.f, qy = 0.f, qz = 0.f, qq = 0.f;
  if (active) {
    qx = x1[q * 3 + 0];
    qy = x1[q * 3 + 1];
    qz = x1[q * 3 + 2];
    qq = (qx * qx + qy * qy) + qz * qz;
  }
  float d0 = INFINITY, d1 = INFINITY, d2 = INFINITY;
  int i0 = 0, i1 = 0, i2 = 0;
  for (int s0 = 0; s0 < S; s0 += NN_THREADS) {
    const int cnt = min(NN_THREADS, S - s0);
    __syncthreads();
    for (int e = threadIdx.x; e < cnt * 3; e += NN_THREADS) src[e] = x2[(int64_t)s0 * 3 + e];
    __syncthreads();
    if (active) {
      for (int j = 0; j < cnt; ++j) {
        const float px = src[j * 3], py = src[j * 3 + 1], pz = src[j * 3 + 2];
        const float dot = (qx * px + qy * py) + qz * pz;
        const float pp = (px * px + py * py) + pz * pz;
        const float d = (-2.0f * dot + qq) + pp;
        const int i = s0 + j;
        if (d < d2) {
          if (d < d1) {
            d2 = d1; i2 = i1;
            if (d < d0) { d1 = d0; i1 = i0; d0 = d; i0 = i; }
            else { d1 = d; i1 = i; }
          } else { d2 = d; i2 = i; }
        }
      }
    }
  }
  const float w0 = 1.0f / (d0 + 1e-8f), w1 = 1.0f / (d1 + 1e-8f), w2 = 1.0f / (d2 + 1e-8f);
  const float ws = (w0 + w1) + w2;
  idx[0] = i0; idx[1] = i1; idx[2] = i2;
  w[0] = w0 / ws; w[1] = w1 / ws; w[2] = w2 / ws;
}

// channel c of the interpolated row (:304-305): the three neighbours' rows of p2 [S, C], weighted, summed left to right
__device__ __forceinline__ float three_nn_mix(const float* __restrict__ p2, int C, int c, const int32_t* idx,
                                              const float* w) {
  return (p2[(int64_t)idx[0] * C + c] * w[0] + p2[(int64_t)idx[1] * C + c] * w[1]) + p2[(int64_t)idx[2] * C + c] * w[2];
}

}  // namespace sv
