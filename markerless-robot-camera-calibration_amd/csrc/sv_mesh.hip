// N3d: the ICP model from a triangle mesh (the reference's utils/icp.py:13-40, run once by app/inference_engine.py:56-57):
// area-weighted surface samples (sample_points_uniformly) and weighted sample elimination (sample_points_poisson_disk).
// Definitions in include/sv_hip.h.  Everything is float64 with the operations rounding as written (-ffp-contract=off),
// so the results equal a numpy restatement bit for bit.  This is set-up work, run once per engine.
//
// sv_mesh_sample: triangle areas (one thread each) -> their running sums in index order (ONE thread adds, the block
// stages the values through LDS: np.cumsum's order is the contract) -> one thread per sample (binary search, barycentric
// point, geometric normal).
//
// sv_sample_eliminate: a fixed-stride neighbour table [N][max_degree] of (index, pair weight), one wavefront per point
// scanning the cloud in ascending index (ballot + popcount prefix, as the ball query), then ONE persistent workgroup
// that runs the whole deletion loop: block arg-max over the weights (largest weight, lowest index), delete, one thread
// per neighbour of the deleted point re-sums its own list.  Up to 16384 points the weights live in LDS (128 KiB: the
// reference's own size), above that in the workspace; the liveness bits are always in LDS.
#include "sv_common.h"

namespace sv {

constexpr int64_t MESH_MAX_F = 1 << 20;
constexpr int64_t MESH_MAX_N = 1 << 20;
constexpr int CDF_THREADS = 256;
constexpr int CDF_CHUNK = 2048;

constexpr int EL_TILE = 1024;        // points per LDS tile of the table kernel
constexpr int EL_WAVES = 4;          // points per block of the table kernel
constexpr int EL_THREADS = 1024;     // the loop's one workgroup
constexpr int EL_MAX_N = 65536;
constexpr int EL_LDS_N = 16384;      // weights in LDS up to this many points
constexpr int EL_MAX_DEGREE = 1024;

__device__ __forceinline__ int lanes_before(unsigned long long mask, int lane) {
  return __popcll(mask & ((1ull << lane) - 1ull));
}

// Corners, cross product and its length of triangle t; false when an index lies outside [0, Nv).
__device__ __forceinline__ bool triangle(const double* __restrict__ verts, int64_t Nv, const int32_t* __restrict__ tris,
                                         int64_t t, double v0[3], double v1[3], double v2[3], double c[3], double& len) {
  const int64_t i0 = tris[t * 3], i1 = tris[t * 3 + 1], i2 = tris[t * 3 + 2];
  if (i0 < 0 || i0 >= Nv || i1 < 0 || i1 >= Nv || i2 < 0 || i2 >= Nv) return false;
  double e1[3], e2[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    v0[a] = verts[i0 * 3 + a];
    v1[a] = verts[i1 * 3 + a];
    v2[a] = verts[i2 * 3 + a];
    e1[a] = v1[a] - v0[a];
    e2[a] = v2[a] - v0[a];
  }
  c[0] = e1[1] * e2[2] - e1[2] * e2[1];
  c[1] = e1[2] * e2[0] - e1[0] * e2[2];
  c[2] = e1[0] * e2[1] - e1[1] * e2[0];
  len = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
  return true;
}

__global__ __launch_bounds__(256) void mesh_area_kernel(const double* __restrict__ verts, int64_t Nv,
                                                         const int32_t* __restrict__ tris, int F,
                                                         double* __restrict__ a, int32_t* __restrict__ counters) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= F) return;
  double v0[3], v1[3], v2[3], c[3], len;
  if (!triangle(verts, Nv, tris, t, v0, v1, v2, c, len)) {
    a[t] = 0.0;
    atomicAdd(&counters[0], 1);  // a count: the order of the additions cannot show
    return;
  }
  a[t] = 0.5 * len;
}

// cdf[t] = a[0] + ... + a[t] in place, added in ascending t by thread 0; the block only moves the values.
__global__ __launch_bounds__(CDF_THREADS) void mesh_cdf_kernel(double* __restrict__ cdf, int F,
                                                                double* __restrict__ area) {
  __shared__ double buf[CDF_CHUNK];
  double carry = 0.0;  // thread 0's
  for (int base = 0; base < F; base += CDF_CHUNK) {
    const int n = min(CDF_CHUNK, F - base);
    for (int e = threadIdx.x; e < n; e += CDF_THREADS) buf[e] = cdf[base + e];
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int e = 0; e < n; ++e) {
        carry += buf[e];
        buf[e] = carry;
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n; e += CDF_THREADS) cdf[base + e] = buf[e];  // each thread rereads its own slots next
  }
  if (threadIdx.x == 0) area[0] = carry;
}

__global__ __launch_bounds__(256) void mesh_sample_kernel(const double* __restrict__ verts, int64_t Nv,
                                                           const int32_t* __restrict__ tris, int F,
                                                           const double* __restrict__ cdf,
                                                           const double* __restrict__ area,
                                                           const double* __restrict__ draws, int N,
                                                           double* __restrict__ points, double* __restrict__ normals,
                                                           int32_t* __restrict__ tri) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= N) return;
  const double nan = __builtin_nan("");
  double p[3] = {nan, nan, nan}, nrm[3] = {nan, nan, nan};
  int t = -1;
  const double A = area[0];
  if (A > 0.0 && isfinite(A)) {  // every area is then finite and the sums do not descend
    const double x = draws[(int64_t)s * 3] * A, r1 = draws[(int64_t)s * 3 + 1], r2 = draws[(int64_t)s * 3 + 2];
    int lo = 0, hi = F;  // number of sums <= x
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;
      if (cdf[mid] <= x)
        lo = mid + 1;
      else
        hi = mid;
    }
    t = min(lo, F - 1);
    double v0[3], v1[3], v2[3], c[3], len;
    // only the clamp can land on a triangle with a bad index (its area is 0): its sample stays NaN
    if (triangle(verts, Nv, tris, t, v0, v1, v2, c, len)) {
      const double q = sqrt(r1), w0 = 1.0 - q, w1 = q * (1.0 - r2), w2 = q * r2;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        p[a] = (w0 * v0[a] + w1 * v1[a]) + w2 * v2[a];
        nrm[a] = c[a] / len;
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    points[(int64_t)s * 3 + a] = p[a];
    normals[(int64_t)s * 3 + a] = nrm[a];
  }
  tri[s] = t;
}

// ---- sample elimination --------------------------------------------------------------------------------------------

// Row i of the table: the j != i with d2 < r_max^2 in ascending j and their pair weights; deg[i] = entries stored,
// counters[0] = the largest true degree (the loop does not run when that exceeds max_degree).
__global__ __launch_bounds__(EL_WAVES * 64) void elim_table_kernel(const double* __restrict__ pts, int N, double r_max,
                                                                    double r_min, int max_degree,
                                                                    int32_t* __restrict__ nbr, double* __restrict__ wt,
                                                                    int32_t* __restrict__ deg,
                                                                    int32_t* __restrict__ counters) {
  __shared__ double tile[EL_TILE * 3];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * EL_WAVES + w;
  const bool live = i < N;
  double qx = 0.0, qy = 0.0, qz = 0.0;
  if (live) {
    qx = pts[(int64_t)i * 3];
    qy = pts[(int64_t)i * 3 + 1];
    qz = pts[(int64_t)i * 3 + 2];
  }
  const double r2 = r_max * r_max;
  const int64_t row = (int64_t)i * max_degree;
  int cnt = 0;
  for (int base = 0; base < N; base += EL_TILE) {
    const int n = min(EL_TILE, N - base);
    __syncthreads();
    for (int e = threadIdx.x; e < n * 3; e += EL_WAVES * 64) tile[e] = pts[(int64_t)base * 3 + e];
    __syncthreads();
    if (!live) continue;
    for (int j0 = 0; j0 < n; j0 += 64) {
      const int j = j0 + lane;
      bool in = false;
      double d2 = 0.0;
      if (j < n && base + j != i) {
        const double dx = tile[j * 3] - qx, dy = tile[j * 3 + 1] - qy, dz = tile[j * 3 + 2] - qz;
        d2 = (dx * dx + dy * dy) + dz * dz;
        in = d2 < r2;  // false for NaN: a non-finite point has no neighbour and is nobody's
      }
      const unsigned long long m = __ballot(in);
      const int pos = cnt + lanes_before(m, lane);
      if (in && pos < max_degree) {
        const double d = fmax(sqrt(d2), r_min);
        const double t = 1.0 - d / r_max;
        double pw = t * t;  // alpha = 8 by three squarings
        pw = pw * pw;
        pw = pw * pw;
        nbr[row + pos] = base + j;
        wt[row + pos] = pw;
      }
      cnt += __popcll(m);
    }
  }
  if (!live || lane != 0) return;
  deg[i] = min(cnt, max_degree);
  atomicMax(&counters[0], cnt);  // a maximum: the order of the updates cannot show
}

template <bool LDS>
__global__ __launch_bounds__(EL_THREADS) void elim_loop_kernel(int N, int n_keep, int max_degree,
                                                                const int32_t* __restrict__ nbr,
                                                                const double* __restrict__ wt,
                                                                const int32_t* __restrict__ deg, double* gweight,
                                                                int32_t* __restrict__ kept, int32_t* __restrict__ order,
                                                                const int32_t* __restrict__ counters) {
  extern __shared__ __attribute__((aligned(16))) double lds_weight[];  // [N] when LDS
  __shared__ uint32_t alive[EL_MAX_N / 32];
  __shared__ double red_v[EL_THREADS / 64];
  __shared__ int red_i[EL_THREADS / 64];
  __shared__ int wave_cnt[EL_THREADS / 64];
  if (counters[0] > max_degree) return;  // truncated rows: the caller retries with a larger table
  double* weight = LDS ? lds_weight : gweight;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  auto is_alive = [&](int j) { return (alive[j >> 5] >> (j & 31)) & 1u; };
  // the sum of row q over its live entries, added in ascending neighbour index
  auto row_weight = [&](int q) {
    const int64_t row = (int64_t)q * max_degree;
    const int d = deg[q];
    double s = 0.0;
    for (int m = 0; m < d; ++m) {
      const double pw = wt[row + m];
      if (is_alive(nbr[row + m])) s += pw;
    }
    return s;
  };
  for (int i = tid; i < EL_MAX_N / 32; i += EL_THREADS) alive[i] = 0xffffffffu;
  __syncthreads();
  for (int i = tid; i < N; i += EL_THREADS) weight[i] = row_weight(i);
  __syncthreads();
  const int n_del = N - n_keep;
  for (int it = 0; it < n_del; ++it) {
    // ---- the live point of largest weight, lowest index on a tie (a deleted point's weight is -1)
    double best = -2.0;
    int bi = 0x7fffffff;
    for (int i = tid; i < N; i += EL_THREADS) {
      const double v = weight[i];
      if (v > best) {  // strictly greater: the lowest index wins within a thread (i ascending)
        best = v;
        bi = i;
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const double ov = __shfl_xor(best, d);
      const int oi = __shfl_xor(bi, d);
      if (ov > best || (ov == best && oi < bi)) {
        best = ov;
        bi = oi;
      }
    }
    if (lane == 0) {
      red_v[wid] = best;
      red_i[wid] = bi;
    }
    __syncthreads();
    double v = red_v[0];
    int p = red_i[0];
#pragma unroll
    for (int k = 1; k < EL_THREADS / 64; ++k) {
      if (red_v[k] > v || (red_v[k] == v && red_i[k] < p)) {
        v = red_v[k];
        p = red_i[k];
      }
    }
    p = min(max(p, 0), N - 1);  // always a row of the table
    if (tid == 0) {
      order[it] = p;
      weight[p] = -1.0;
      alive[p >> 5] &= ~(1u << (p & 31));
    }
    __syncthreads();
    // ---- every live neighbour of p sums its list again
    const int dp = deg[p];
    const int64_t prow = (int64_t)p * max_degree;
    for (int k = tid; k < dp; k += EL_THREADS) {
      const int q = nbr[prow + k];
      if (is_alive(q)) weight[q] = row_weight(q);
    }
    __syncthreads();
  }
  // ---- the survivors in ascending order
  int out = 0;
  for (int base = 0; base < N; base += EL_THREADS) {
    const int i = base + tid;
    const bool keep = i < N && is_alive(i);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_cnt[wid] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < EL_THREADS / 64; ++k) {
      const int c = wave_cnt[k];
      before += k < wid ? c : 0;
      total += c;
    }
    const int pos = out + before + lanes_before(m, lane);
    if (keep && pos < n_keep) kept[pos] = i;
    out += total;
    __syncthreads();
  }
}

static size_t eliminate_bytes(int64_t N, int max_degree) {
  const size_t n = (size_t)(N > 0 ? N : 0), d = (size_t)(max_degree > 0 ? max_degree : 0);
  return align_up(n * d * sizeof(int32_t), 256) + align_up(n * d * sizeof(double), 256) +
         align_up(n * sizeof(int32_t), 256) + align_up(n * sizeof(double), 256) + 256;
}

}  // namespace sv

using namespace sv;

extern "C" {

size_t sv_mesh_sample_workspace_bytes(int64_t F) { return align_up((size_t)(F > 0 ? F : 0) * sizeof(double), 256) + 256; }

int sv_mesh_sample(const double* verts, int64_t Nv, const int32_t* tris, int64_t F, const double* draws, int64_t N,
                   void* workspace, size_t workspace_bytes, double* points, double* normals, int32_t* tri, double* area,
                   int32_t* counters, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(F >= 1 && F <= MESH_MAX_F, "need 1 to 2^20 triangles");
  SV_CHECK_ARG(N >= 1 && N <= MESH_MAX_N, "need 1 to 2^20 samples");
  SV_CHECK_ARG(Nv >= 1, "need at least one vertex");
  SV_CHECK_ARG(verts && tris && draws && workspace && points && normals && tri && area && counters, "null pointer");
  if (workspace_bytes < sv_mesh_sample_workspace_bytes(F)) {
    set_error("sv_mesh_sample: workspace too small");
    return SV_ERR_WORKSPACE;
  }
  Workspace ws(workspace, workspace_bytes);
  double* cdf = ws.take<double>((size_t)F);
  if (!ws.ok) {
    set_error("sv_mesh_sample: workspace too small");
    return SV_ERR_WORKSPACE;
  }
  SV_HIP(hipMemsetAsync(counters, 0, sizeof(int32_t), stream));
  hipLaunchKernelGGL(mesh_area_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, stream, verts, Nv, tris, (int)F,
                     cdf, counters);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(mesh_cdf_kernel, dim3(1), dim3(CDF_THREADS), 0, stream, cdf, (int)F, area);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(mesh_sample_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, verts, Nv, tris, (int)F,
                     cdf, area, draws, (int)N, points, normals, tri);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

size_t sv_sample_eliminate_workspace_bytes(int64_t N, int max_degree) { return eliminate_bytes(N, max_degree); }

int sv_sample_eliminate(const double* points, int64_t N, int64_t n_keep, double r_max, double r_min, int max_degree,
                        void* workspace, size_t workspace_bytes, int32_t* kept, int32_t* order, int32_t* counters,
                        sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(N >= 1 && N <= EL_MAX_N, "need 1 to 65536 points");
  SV_CHECK_ARG(n_keep >= 1 && n_keep <= N, "n_keep must lie in [1, N]");
  SV_CHECK_ARG(max_degree >= 1 && max_degree <= EL_MAX_DEGREE, "max_degree must lie in [1, 1024]");
  SV_CHECK_ARG(r_max > 0 && r_max < INFINITY, "r_max must be finite and positive");
  SV_CHECK_ARG(r_min >= 0 && r_min <= r_max, "r_min must lie in [0, r_max]");
  SV_CHECK_ARG(points && workspace && kept && counters && (order || n_keep == N), "null pointer");
  if (workspace_bytes < sv_sample_eliminate_workspace_bytes(N, max_degree)) {
    set_error("sv_sample_eliminate: workspace too small");
    return SV_ERR_WORKSPACE;
  }
  Workspace ws(workspace, workspace_bytes);
  const size_t cells = (size_t)N * (size_t)max_degree;
  int32_t* nbr = ws.take<int32_t>(cells);
  double* wt = ws.take<double>(cells);
  int32_t* deg = ws.take<int32_t>((size_t)N);
  double* gweight = ws.take<double>((size_t)N);
  if (!ws.ok) {
    set_error("sv_sample_eliminate: workspace too small");
    return SV_ERR_WORKSPACE;
  }
  SV_HIP(hipMemsetAsync(counters, 0, sizeof(int32_t), stream));
  hipLaunchKernelGGL(elim_table_kernel, dim3((unsigned)((N + EL_WAVES - 1) / EL_WAVES)), dim3(EL_WAVES * 64), 0, stream,
                     points, (int)N, r_max, r_min, max_degree, nbr, wt, deg, counters);
  SV_LAUNCH_CHECK();
  if (N <= EL_LDS_N) {
    static bool attr_set = false;
    if (!attr_set) {
      SV_HIP(hipFuncSetAttribute((const void*)elim_loop_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 EL_LDS_N * (int)sizeof(double)));
      attr_set = true;
    }
    hipLaunchKernelGGL(elim_loop_kernel<true>, dim3(1), dim3(EL_THREADS), (size_t)N * sizeof(double), stream, (int)N,
                       (int)n_keep, max_degree, nbr, wt, deg, gweight, kept, order, counters);
  } else {
    hipLaunchKernelGGL(elim_loop_kernel<false>, dim3(1), dim3(EL_THREADS), 0, stream, (int)N, (int)n_keep, max_degree,
                       nbr, wt, deg, gweight, kept, order, counters);
  }
  SV_LAUNCH_CHECK();
  return SV_OK;
}

}  // extern "C"
