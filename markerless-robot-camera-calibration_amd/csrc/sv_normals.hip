// N3b: surface normals for point-to-plane ICP (the reference's utils/icp.py:46-48 estimate_normals with
// KDTreeSearchParamHybrid(radius, max_nn); definitions in include/sv_hip.h).
//
// One wavefront per query point, four queries per 256-thread block.  The cloud is staged through LDS in tiles of 1024
// points shared by the block's waves (brute force as icp_nn_search: crops have thousands of points, no grid).  Lanes
// stride over the tile; in-radius candidates are compacted in ascending index order (ballot + popcount prefix, no
// atomics) into a per-wave LDS buffer of (distance bits, index).  Then, per wave and with no block-wide barrier:
//   * at most max_nn candidates: the buffer is the neighbour set;
//   * more: the max_nn-th smallest distance is found by bisection on the float32 distance bits (non-negative floats
//     order as their bit patterns) - over the buffer when everything fitted, otherwise over re-scans of the cloud in
//     global memory - and the set is every candidate below it plus the lowest-index ones equal to it.
// Either way the selected indices come out in ascending order, lane l takes neighbour l (max_nn <= 64), and mean and
// covariance are butterfly sums over the lanes in float64: the bits of the result depend on the neighbour set only,
// not on the tile size, the buffer capacity or which path selected the set.
#include "sv_common.h"
#include "sv_dense_math.h"

namespace sv {

constexpr int NRM_TILE = 1024;   // points per LDS tile
constexpr int NRM_WAVES = 4;     // queries per block
constexpr int NRM_CAP = 512;     // candidates buffered per query
constexpr int NRM_MAX_NN = 64;   // one neighbour per lane

// orders this wave's LDS writes before its later LDS reads (the waves of a block run independently after the scan)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int lanes_below(unsigned long long mask, int lane) {
  return __popcll(mask & ((1ull << lane) - 1ull));
}

__device__ __forceinline__ float sqdist(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);  // commutative adds: every lane ends with the same bits
  return v;
}

// Candidate e of a query's stream: its distance bits and cloud index.  BUFFERED reads the wave's LDS buffer (cnt entries,
// ascending index); otherwise the cloud itself is re-scanned (N entries, in-radius ones are candidates).
template <bool BUFFERED>
__device__ __forceinline__ bool candidate(int e, int n_entries, const uint32_t* cbits, const int32_t* cidx,
                                          const float* __restrict__ xyz, float qx, float qy, float qz, float r2,
                                          uint32_t& bits, int& idx) {
  if (e >= n_entries) return false;
  if (BUFFERED) {
    bits = cbits[e];
    idx = cidx[e];
    return true;
  }
  const float d = sqdist(xyz[(int64_t)e * 3], xyz[(int64_t)e * 3 + 1], xyz[(int64_t)e * 3 + 2], qx, qy, qz);
  bits = __float_as_uint(d);
  idx = e;
  return d < r2;  // false for NaN
}

// Writes the indices of the k nearest of more than k candidates to sel[0..k), ascending (ties at the k-th distance: the
// lowest indices).
template <bool BUFFERED>
__device__ __forceinline__ void select_nearest(int k, int n_entries, const uint32_t* cbits, const int32_t* cidx,
                                               const float* __restrict__ xyz, float qx, float qy, float qz, float r2,
                                               int32_t* sel, int lane) {
  auto count_le = [&](uint32_t th) {
    int c = 0;
    for (int base = 0; base < n_entries; base += 64) {
      uint32_t bits = 0;
      int idx = 0;
      const bool ok = candidate<BUFFERED>(base + lane, n_entries, cbits, cidx, xyz, qx, qy, qz, r2, bits, idx);
      c += __popcll(__ballot(ok && bits <= th));
    }
    return c;
  };
  // smallest th with count_le(th) >= k; every candidate's bits are below those of r2
  uint32_t lo = 0, hi = __float_as_uint(r2) - 1u;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (count_le(mid) >= k)
      hi = mid;
    else
      lo = mid + 1u;
  }
  const uint32_t th = lo;
  const int need = k - (th > 0u ? count_le(th - 1u) : 0);  // how many of the candidates AT th belong to the set
  int out = 0, ties = 0;
  for (int base = 0; base < n_entries; base += 64) {
    uint32_t bits = 0;
    int idx = 0;
    const bool ok = candidate<BUFFERED>(base + lane, n_entries, cbits, cidx, xyz, qx, qy, qz, r2, bits, idx);
    const unsigned long long eq = __ballot(ok && bits == th);
    const bool take = ok && (bits < th || (bits == th && ties + lanes_below(eq, lane) < need));
    const unsigned long long tk = __ballot(take);
    if (take) sel[out + lanes_below(tk, lane)] = idx;  // out + prefix < k <= 64
    out += __popcll(tk);
    ties += __popcll(eq);
  }
}

__global__ __launch_bounds__(NRM_WAVES * 64) void normals_kernel(const float* __restrict__ xyz, int N, float r2,
                                                                  int max_nn, float* __restrict__ normals,
                                                                  int32_t* __restrict__ counts) {
  __shared__ float tile[NRM_TILE * 3];
  __shared__ uint32_t cand_bits[NRM_WAVES][NRM_CAP];
  __shared__ int32_t cand_idx[NRM_WAVES][NRM_CAP];
  __shared__ int32_t selected[NRM_WAVES][NRM_MAX_NN];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * NRM_WAVES + w;  // this wave's query point
  const bool live = i < N;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (live) {
    qx = xyz[(int64_t)i * 3];
    qy = xyz[(int64_t)i * 3 + 1];
    qz = xyz[(int64_t)i * 3 + 2];
  }
  uint32_t* cbits = cand_bits[w];
  int32_t* cidx = cand_idx[w];
  int32_t* sel = selected[w];
  // ---- scan: count the in-radius points and buffer the first NRM_CAP of them
  int cnt = 0;
  for (int base = 0; base < N; base += NRM_TILE) {
    const int n = min(NRM_TILE, N - base);
    __syncthreads();
    for (int e = threadIdx.x; e < n * 3; e += NRM_WAVES * 64) tile[e] = xyz[(int64_t)base * 3 + e];
    __syncthreads();
    if (!live) continue;
    for (int j0 = 0; j0 < n; j0 += 64) {
      const int j = j0 + lane;
      bool in = false;
      float d = 0.f;
      if (j < n) {
        d = sqdist(tile[j * 3], tile[j * 3 + 1], tile[j * 3 + 2], qx, qy, qz);
        in = d < r2;  // a NaN or inf coordinate on either side gives inf or NaN: never a neighbour
      }
      const unsigned long long m = __ballot(in);
      const int pos = cnt + lanes_below(m, lane);
      if (in && pos < NRM_CAP) {
        cbits[pos] = __float_as_uint(d);
        cidx[pos] = base + j;
      }
      cnt += __popcll(m);
    }
  }
  if (!live) return;  // no block-wide barrier below
  wave_lds_sync();
  // ---- neighbour set -> sel[0..k), ascending index
  const int k = min(cnt, max_nn);
  if (cnt <= max_nn) {
    if (lane < cnt) sel[lane] = cidx[lane];
  } else if (cnt <= NRM_CAP) {
    select_nearest<true>(k, cnt, cbits, cidx, xyz, qx, qy, qz, r2, sel, lane);
  } else {
    select_nearest<false>(k, N, cbits, cidx, xyz, qx, qy, qz, r2, sel, lane);
  }
  wave_lds_sync();
  // ---- mean and covariance of the set in float64, one neighbour per lane
  double p[3] = {0.0, 0.0, 0.0};
  if (lane < k) {
    const int64_t j = min(max(sel[lane], 0), N - 1);  // always a row of the cloud
    p[0] = (double)xyz[j * 3];
    p[1] = (double)xyz[j * 3 + 1];
    p[2] = (double)xyz[j * 3 + 2];
  }
  double mean[3], C[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a) mean[a] = wave_sum(p[a]) / (double)max(k, 1);
#pragma unroll
  for (int a = 0; a < 3; ++a) p[a] = lane < k ? p[a] - mean[a] : 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = a; b < 3; ++b) C[a][b] = C[b][a] = wave_sum(p[a] * p[b]) / (double)max(k, 1);
  if (lane != 0) return;
  float nrm[3] = {0.f, 0.f, 1.f};  // fewer than 3 neighbours
  if (!(isfinite(qx) && isfinite(qy) && isfinite(qz))) {
    nrm[0] = nrm[1] = nrm[2] = __builtin_nanf("");
  } else if (k >= 3) {
    double lam[3], V[3][3];
    jacobi_eig3(C, lam, V);
    int m = 0;  // smallest eigenvalue; with collinear or coincident neighbours any of the null space's unit vectors
    if (lam[1] < lam[m]) m = 1;
    if (lam[2] < lam[m]) m = 2;
    const double len = sqrt(V[0][m] * V[0][m] + V[1][m] * V[1][m] + V[2][m] * V[2][m]);
#pragma unroll
    for (int a = 0; a < 3; ++a) nrm[a] = (float)(V[a][m] / len);
    // sign: the stored component of largest magnitude is positive, the first on ties
    int g = 0;
    if (fabsf(nrm[1]) > fabsf(nrm[g])) g = 1;
    if (fabsf(nrm[2]) > fabsf(nrm[g])) g = 2;
    if (nrm[g] < 0.f) {
#pragma unroll
      for (int a = 0; a < 3; ++a) nrm[a] = -nrm[a];
    }
  }
  normals[(int64_t)i * 3] = nrm[0];
  normals[(int64_t)i * 3 + 1] = nrm[1];
  normals[(int64_t)i * 3 + 2] = nrm[2];
  if (counts) counts[i] = k;
}

}  // namespace sv

using namespace sv;

extern "C" {

// the workspace is currently unused (the kernel keeps its candidates in LDS); a fixed 256 bytes keeps the calling
// convention of the other entry points
size_t sv_normals_workspace_bytes(int64_t N, int max_nn) {
  (void)N;
  (void)max_nn;
  return 256;
}

int sv_estimate_normals(const float* xyz, int64_t N, double radius, int max_nn, void* workspace, size_t workspace_bytes,
                        float* normals, int32_t* counts, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(N >= 1 && N <= (1 << 20), "need 1 to 2^20 points");
  SV_CHECK_ARG(radius > 0 && (float)(radius * radius) > 0.f && (float)(radius * radius) < INFINITY, "bad radius");
  SV_CHECK_ARG(max_nn >= 3 && max_nn <= NRM_MAX_NN, "max_nn must lie in [3, 64]");
  SV_CHECK_ARG(xyz && normals && workspace, "null pointer");
  if (workspace_bytes < sv_normals_workspace_bytes(N, max_nn)) {
    set_error("sv_estimate_normals: workspace too small");
    return SV_ERR_WORKSPACE;
  }
  const unsigned nb = (unsigned)((N + NRM_WAVES - 1) / NRM_WAVES);
  hipLaunchKernelGGL(normals_kernel, dim3(nb), dim3(NRM_WAVES * 64), 0, stream, xyz, (int)N, (float)(radius * radius),
                     max_nn, normals, counts);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

}  // extern "C"
