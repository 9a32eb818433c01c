// N3: point-to-point ICP (replaces utils/icp.py:13-83, i.e. open3d.pipelines.registration.registration_icp with
// TransformationEstimationPointToPoint, max_correspondence_distance = 0.1, at most 30 iterations, relative fitness /
// rmse tolerance 1e-6; call sites app/inference_engine.py:358-362).
//
// Per iteration: (1) nearest target point of every transformed source point — brute force, the target cloud staged
// through LDS in tiles, one thread per source point (S, T <= ~20k: 10^8 distance evaluations, latency-trivial on 256 CUs;
// no k-d tree); (2) one workgroup reduces the correspondences within the distance threshold to centroids + the 3x3
// cross-covariance in fp64 and solves the Kabsch problem with the same one-sided Jacobi SVD as sv_kabsch_batched.
// The iteration loop runs on the device side of the stream: a `state` record carries the current transform, the
// previous fitness / rmse and a converged flag that turns the remaining launches into no-ops (no host read-backs).
//
// sv_icp_point2plane shares the search, the state record and the loop; only step (2) differs (icp_plane_sums /
// icp_plane_step: the 6x6 normal equations of the linearised point-to-plane residual, Cholesky, T <- U T).  The target
// normals come from sv_estimate_normals (sv_normals.hip) or from the caller.
//
// N3c, sv_icp_batched: P problems (one source cloud, P target clouds) per launch - the search on a grid of
// (ceil(S / 256), P), one update workgroup per problem.  There is one host routine (icp_run) and one init, search and
// finish kernel: the single calls are the P = 1 independent case (offsets {0, T}, no pre).  Only the update of that case
// keeps kernels of its own (icp_update_kernel, icp_plane_update_kernel: thin wrappers, as the batch's, round
// icp_p2p_sums / icp_p2p_step and icp_plane_sums / icp_plane_step, measurably faster without the problem index), so a
// problem of an independent batch runs the single call's arithmetic in the single call's order.  In shared mode (one transform for all problems) the update workgroups write their totals to the
// workspace and a one-wave tail kernel adds them in ascending problem order and takes the step on the pooled sums.
#include "sv_common.h"
#include "sv_dense_math.h"

namespace sv {

struct IcpState {
  double T[16];       // current source -> target transform (row-major 4x4)
  double fitness;     // inlier fraction of the last evaluation
  double rmse;        // inlier rmse of the last evaluation
  int iterations;     // updates applied
  int converged;
};

constexpr int NN_TILE = 1024;

// source point i of a problem: the model point m, or pre . m in float64 (the row expressions of T . x, never rounded)
__device__ __forceinline__ void icp_source_point(const float* __restrict__ src, int i, const double* __restrict__ pre,
                                                 double& x, double& y, double& z) {
  x = src[i * 3], y = src[i * 3 + 1], z = src[i * 3 + 2];
  if (pre) {
    const double mx = x, my = y, mz = z;
    x = pre[0] * mx + pre[1] * my + pre[2] * mz + pre[3];
    y = pre[4] * mx + pre[5] * my + pre[6] * mz + pre[7];
    z = pre[8] * mx + pre[9] * my + pre[10] * mz + pre[11];
  }
}

// one workgroup of 256 source points against the T target points; tile: NN_TILE * 3 floats of LDS
__device__ __forceinline__ void icp_nn_search(const float* __restrict__ src, int S, const double* __restrict__ pre,
                                              const float* __restrict__ tgt, int T, const IcpState* __restrict__ st,
                                              float max_d2, int32_t* __restrict__ nn, float* __restrict__ d2out,
                                              float* tile) {
  if (st->converged) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (i < S) {
    double x, y, z;
    icp_source_point(src, i, pre, x, y, z);
    px = (float)(st->T[0] * x + st->T[1] * y + st->T[2] * z + st->T[3]);
    py = (float)(st->T[4] * x + st->T[5] * y + st->T[6] * z + st->T[7]);
    pz = (float)(st->T[8] * x + st->T[9] * y + st->T[10] * z + st->T[11]);
  }
  float best = INFINITY;
  int bi = -1;
  for (int base = 0; base < T; base += NN_TILE) {
    const int n = min(NN_TILE, T - base);
    __syncthreads();
    for (int e = threadIdx.x; e < n * 3; e += 256) tile[e] = tgt[(int64_t)base * 3 + e];
    __syncthreads();
    if (i < S) {
      for (int j = 0; j < n; ++j) {
        const float dx = tile[j * 3] - px, dy = tile[j * 3 + 1] - py, dz = tile[j * 3 + 2] - pz;
        const float d = dx * dx + dy * dy + dz * dz;
        if (d < best) {  // first minimum wins (ascending target index)
          best = d;
          bi = base + j;
        }
      }
    }
  }
  if (i < S) {
    const bool ok = bi >= 0 && best <= max_d2;
    nn[i] = ok ? bi : -1;
    d2out[i] = best;
  }
}

__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double t = 0;
  for (int k = 0; k < 16; ++k) t += red[k];  // fixed order -> reproducible
  return t;
}

constexpr int P2P_ACC = 17;  // n, sp(3), sq(3), spq(9), err

// a problem's inlier sums under Tm, by one workgroup of 1024: tot[P2P_ACC] on every thread
__device__ __forceinline__ void icp_p2p_sums(const float* __restrict__ src, int S, const double* __restrict__ pre,
                                             const float* __restrict__ tgt, const int32_t* __restrict__ nn,
                                             const float* __restrict__ d2, const double* Tm, double* tot, double* red) {
  double acc[16];  // n, sp(3), sq(3), spq(9) -> 16 values
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0;
  double err = 0.0;
  for (int i = threadIdx.x; i < S; i += 1024) {
    const int j = nn[i];
    if (j < 0) continue;
    double x, y, z;
    icp_source_point(src, i, pre, x, y, z);
    const double p[3] = {Tm[0] * x + Tm[1] * y + Tm[2] * z + Tm[3], Tm[4] * x + Tm[5] * y + Tm[6] * z + Tm[7],
                         Tm[8] * x + Tm[9] * y + Tm[10] * z + Tm[11]};
    const double q[3] = {tgt[j * 3], tgt[j * 3 + 1], tgt[j * 3 + 2]};
    acc[0] += 1.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      acc[1 + a] += p[a];
      acc[4 + a] += q[a];
#pragma unroll
      for (int b = 0; b < 3; ++b) acc[7 + a * 3 + b] += p[a] * q[b];
    }
    err += (double)d2[i];
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) tot[k] = block_sum(acc[k], red);
  tot[16] = block_sum(err, red);
}

// one thread: evaluation (fitness = inliers / points), stop rule and Kabsch update from the sums tot[P2P_ACC]
__device__ __forceinline__ void icp_p2p_step(IcpState* __restrict__ st, const double* Tm, const double* tot,
                                             double points, double rel_fitness, double rel_rmse, int last) {
  const double n = tot[0];
  const double fitness = n / points;
  const double rmse = n > 0 ? sqrt(tot[16] / n) : 0.0;
  // open3d: stop when both the fitness and the rmse moved by less than the tolerances since the previous evaluation
  const bool stop = (st->iterations > 0 || st->fitness >= 0) &&
                    fabs(st->fitness - fitness) < rel_fitness && fabs(st->rmse - rmse) < rel_rmse;
  st->fitness = fitness;
  st->rmse = rmse;
  if (stop || n < 3 || last) {
    st->converged = 1;
    return;
  }
  double cp[3], cq[3], H[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    cp[a] = tot[1 + a] / n;
    cq[a] = tot[4 + a] / n;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) H[a][b] = tot[7 + a * 3 + b] - n * cp[a] * cq[b];
  double R[3][3], t[3];
  kabsch_from_covariance(H, cp, cq, R, t);
  // T <- [R t] * T
  double Tn[16];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      Tn[r * 4 + c] = R[r][0] * Tm[0 * 4 + c] + R[r][1] * Tm[1 * 4 + c] + R[r][2] * Tm[2 * 4 + c] + (c == 3 ? t[r] : 0.0);
  Tn[12] = Tn[13] = Tn[14] = 0.0;
  Tn[15] = 1.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) st->T[k] = Tn[k];
  st->iterations += 1;
}

// the update of a single call (one problem, no pre); a batch goes through icp_batch_update_kernel
__global__ __launch_bounds__(1024) void icp_update_kernel(const float* __restrict__ src, int S,
                                                           const float* __restrict__ tgt,
                                                           const int32_t* __restrict__ nn,
                                                           const float* __restrict__ d2, IcpState* __restrict__ st,
                                                           double rel_fitness, double rel_rmse, int last) {
  __shared__ double red[16];
  if (st->converged) return;
  double Tm[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) Tm[k] = st->T[k];
  double tot[P2P_ACC];
  icp_p2p_sums(src, S, nullptr, tgt, nn, d2, Tm, tot, red);
  if (threadIdx.x != 0) return;
  icp_p2p_step(st, Tm, tot, (double)S, rel_fitness, rel_rmse, last);
}

__device__ __forceinline__ void icp_init_state(IcpState* st, const double* init_T) {
  if (threadIdx.x < 16) st->T[threadIdx.x] = init_T ? init_T[threadIdx.x] : ((threadIdx.x % 5 == 0) ? 1.0 : 0.0);
  if (threadIdx.x == 0) {
    st->fitness = -1.0;
    st->rmse = 0.0;
    st->iterations = 0;
    st->converged = 0;
  }
}

// ---- point-to-plane update (sv_icp_point2plane) -------------------------------------------------------------------
// Same evaluation as icp_p2p_step (inliers of icp_nn_search, fitness, rmse, stop rule); the update linearises the
// rotation: per inlier r = (p - q).n, J = [p x n, n], A = sum J J^T (upper triangle, 21 values), b = sum J r, solved by
// a 6x6 Cholesky in float64.  PL_ACC values per thread are summed over the wave by shuffles, then over the 8 waves in
// ascending order, one thread per sum, through LDS: a fixed order, so repeated runs give the same bits (and thread 0's
// solve reads the totals from LDS instead of holding 30 of them next to L in registers).
constexpr int PL_ACC = 30;       // inliers, contributing, err, A (21), b (6)
constexpr int PL_THREADS = 512;  // 8 waves

__device__ __forceinline__ void nan_transform(double* T) {
  const double nan = __builtin_nan("");
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = nan;
  T[12] = T[13] = T[14] = 0.0;
  T[15] = 1.0;
}

// a problem's sums under Tm, by one workgroup of PL_THREADS: tot[PL_ACC] (LDS), valid for every thread on return
__device__ __forceinline__ void icp_plane_sums(const float* __restrict__ src, int S, const double* __restrict__ pre,
                                               const float* __restrict__ tgt, const float* __restrict__ tgt_normals,
                                               const int32_t* __restrict__ nn, const float* __restrict__ d2,
                                               const double* Tm, double (*red)[PL_THREADS / 64], double* tot) {
  double acc[PL_ACC];
#pragma unroll
  for (int k = 0; k < PL_ACC; ++k) acc[k] = 0.0;
  for (int i = threadIdx.x; i < S; i += PL_THREADS) {
    const int j = nn[i];
    if (j < 0) continue;
    acc[0] += 1.0;
    acc[2] += (double)d2[i];
    const double n[3] = {tgt_normals[j * 3], tgt_normals[j * 3 + 1], tgt_normals[j * 3 + 2]};
    if (!(isfinite(n[0]) && isfinite(n[1]) && isfinite(n[2]))) continue;  // counts as an inlier, adds no equation
    double x, y, z;
    icp_source_point(src, i, pre, x, y, z);
    const double p[3] = {Tm[0] * x + Tm[1] * y + Tm[2] * z + Tm[3], Tm[4] * x + Tm[5] * y + Tm[6] * z + Tm[7],
                         Tm[8] * x + Tm[9] * y + Tm[10] * z + Tm[11]};
    const double q[3] = {tgt[j * 3], tgt[j * 3 + 1], tgt[j * 3 + 2]};
    const double r = (p[0] - q[0]) * n[0] + (p[1] - q[1]) * n[1] + (p[2] - q[2]) * n[2];
    const double J[6] = {p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0],
                         n[0], n[1], n[2]};
    acc[1] += 1.0;
    int e = 3;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = a; b < 6; ++b) acc[e++] += J[a] * J[b];
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[24 + a] += J[a] * r;
  }
#pragma unroll
  for (int k = 0; k < PL_ACC; ++k) {
    double v = acc[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < PL_ACC) {
    double t = 0;
    for (int w = 0; w < PL_THREADS / 64; ++w) t += red[threadIdx.x][w];  // fixed order -> reproducible
    tot[threadIdx.x] = t;
  }
  __syncthreads();
}

// one thread: evaluation (fitness = inliers / points), stop rule and point-to-plane update from the sums tot[PL_ACC]
__device__ __forceinline__ void icp_plane_step(IcpState* __restrict__ st, const double* Tm, const double* tot,
                                               double points, double rel_fitness, double rel_rmse, int last) {
  const double n = tot[0];
  const double fitness = n / points;
  const double rmse = n > 0 ? sqrt(tot[2] / n) : 0.0;
  const bool stop = (st->iterations > 0 || st->fitness >= 0) &&
                    fabs(st->fitness - fitness) < rel_fitness && fabs(st->rmse - rmse) < rel_rmse;
  st->fitness = fitness;
  st->rmse = rmse;
  if (stop || tot[1] < 6 || last) {
    st->converged = 1;
    return;
  }
  // A = L L^T (lower triangle of L), then L y = -b, L^T x = y.  A pivot that is not a positive finite number (parallel
  // normals, NaN sums) ends the iteration without an update.
  double L[6][6], x[6];
  {
    int e = 3;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = a; b < 6; ++b) L[b][a] = tot[e++];
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double d = L[c][c];
#pragma unroll
    for (int k = 0; k < c; ++k) d -= L[c][k] * L[c][k];
    if (!(d > 0.0) || !isfinite(d)) {
      st->converged = 1;
      return;
    }
    d = sqrt(d);
    L[c][c] = d;
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      double v = L[r][c];
#pragma unroll
      for (int k = 0; k < c; ++k) v -= L[r][k] * L[c][k];
      L[r][c] = v / d;
    }
  }
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    double v = -tot[24 + r];
#pragma unroll
    for (int k = 0; k < r; ++k) v -= L[r][k] * x[k];
    x[r] = v / L[r][r];
  }
#pragma unroll
  for (int r = 5; r >= 0; --r) {
    double v = x[r];
#pragma unroll
    for (int k = r + 1; k < 6; ++k) v -= L[k][r] * x[k];
    x[r] = v / L[r][r];
  }
  double Tn[16];
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 6; ++k) finite = finite && isfinite(x[k]);
  if (!finite) {
    nan_transform(Tn);
  } else {
    // U = [Rz(gamma) Ry(beta) Rx(alpha) | t], T <- U * T
    const double sa = sin(x[0]), ca = cos(x[0]), sb = sin(x[1]), cb = cos(x[1]), sg = sin(x[2]), cg = cos(x[2]);
    const double R[3][3] = {{cb * cg, sa * sb * cg - ca * sg, ca * sb * cg + sa * sg},
                            {cb * sg, sa * sb * sg + ca * cg, ca * sb * sg - sa * cg},
                            {-sb, sa * cb, ca * cb}};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        Tn[r * 4 + c] =
            R[r][0] * Tm[0 * 4 + c] + R[r][1] * Tm[1 * 4 + c] + R[r][2] * Tm[2 * 4 + c] + (c == 3 ? x[3 + r] : 0.0);
    Tn[12] = Tn[13] = Tn[14] = 0.0;
    Tn[15] = 1.0;
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) st->T[k] = Tn[k];
  st->iterations += 1;
}

__global__ __launch_bounds__(PL_THREADS) void icp_plane_update_kernel(
    const float* __restrict__ src, int S, const float* __restrict__ tgt, const float* __restrict__ tgt_normals,
    const int32_t* __restrict__ nn, const float* __restrict__ d2, IcpState* __restrict__ st, double rel_fitness,
    double rel_rmse, int last) {
  __shared__ double red[PL_ACC][PL_THREADS / 64];
  __shared__ double tot[PL_ACC];
  if (st->converged) return;
  double Tm[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) Tm[k] = st->T[k];
  icp_plane_sums(src, S, nullptr, tgt, tgt_normals, nn, d2, Tm, red, tot);
  if (threadIdx.x != 0) return;
  icp_plane_step(st, Tm, tot, (double)S, rel_fitness, rel_rmse, last);
}

// ---- N3c: P problems per launch (sv_icp_batched) -------------------------------------------------------------------
// Problem p = blockIdx.y (search) or blockIdx.x (update): source = src (through pre[p] when given), target rows
// off.v[p] .. off.v[p + 1] - 1 of tgt, correspondences nn / d2 [p][S], state states[p] - or states[0] in shared mode,
// where the update workgroups only write their sums to part[p][ICP_PART] and icp_joint_tail_kernel takes the step.
constexpr int ICP_MAX_PROBLEMS = 64;
constexpr int ICP_PART = 32;  // doubles per problem in part: P2P_ACC or PL_ACC sums

struct IcpOffsets {
  int32_t v[ICP_MAX_PROBLEMS + 1];  // a kernel argument: the host array needs no copy and no wait
};

__global__ __launch_bounds__(256) void icp_batch_nn_kernel(const float* __restrict__ src, int S,
                                                            const double* __restrict__ pre,
                                                            const float* __restrict__ tgt, IcpOffsets off,
                                                            const IcpState* __restrict__ states, int shared,
                                                            float max_d2, int32_t* __restrict__ nn,
                                                            float* __restrict__ d2out) {
  __shared__ float tile[NN_TILE * 3];
  const int p = blockIdx.y;
  const int o = off.v[p];
  icp_nn_search(src, S, pre ? pre + p * 16 : nullptr, tgt + (int64_t)o * 3, off.v[p + 1] - o, states + (shared ? 0 : p),
                max_d2, nn + (size_t)p * S, d2out + (size_t)p * S, tile);
}

__global__ __launch_bounds__(1024) void icp_batch_update_kernel(
    const float* __restrict__ src, int S, const double* __restrict__ pre, const float* __restrict__ tgt, IcpOffsets off,
    const int32_t* __restrict__ nn, const float* __restrict__ d2, IcpState* __restrict__ states, int shared,
    double* __restrict__ part, double rel_fitness, double rel_rmse, int last) {
  __shared__ double red[16];
  const int p = blockIdx.x;
  IcpState* st = states + (shared ? 0 : p);
  if (st->converged) return;
  double Tm[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) Tm[k] = st->T[k];
  double tot[P2P_ACC];
  icp_p2p_sums(src, S, pre ? pre + p * 16 : nullptr, tgt + (int64_t)off.v[p] * 3, nn + (size_t)p * S, d2 + (size_t)p * S,
               Tm, tot, red);
  if (threadIdx.x != 0) return;
  if (shared) {
#pragma unroll
    for (int k = 0; k < P2P_ACC; ++k) part[p * ICP_PART + k] = tot[k];
    return;
  }
  icp_p2p_step(st, Tm, tot, (double)S, rel_fitness, rel_rmse, last);
}

__global__ __launch_bounds__(PL_THREADS) void icp_batch_plane_update_kernel(
    const float* __restrict__ src, int S, const double* __restrict__ pre, const float* __restrict__ tgt,
    const float* __restrict__ tgt_normals, IcpOffsets off, const int32_t* __restrict__ nn, const float* __restrict__ d2,
    IcpState* __restrict__ states, int shared, double* __restrict__ part, double rel_fitness, double rel_rmse, int last) {
  __shared__ double red[PL_ACC][PL_THREADS / 64];
  __shared__ double tot[PL_ACC];
  const int p = blockIdx.x;
  IcpState* st = states + (shared ? 0 : p);
  if (st->converged) return;
  double Tm[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) Tm[k] = st->T[k];
  const int64_t o = (int64_t)off.v[p] * 3;
  icp_plane_sums(src, S, pre ? pre + p * 16 : nullptr, tgt + o, tgt_normals + o, nn + (size_t)p * S, d2 + (size_t)p * S,
                 Tm, red, tot);
  if (shared) {
    if (threadIdx.x < PL_ACC) part[p * ICP_PART + threadIdx.x] = tot[threadIdx.x];
    return;
  }
  if (threadIdx.x != 0) return;
  icp_plane_step(st, Tm, tot, (double)S, rel_fitness, rel_rmse, last);
}

// shared mode, one wave: pooled sums = problem 0's, then problems 1 .. P-1 added in ascending order (one thread per
// sum); per-problem fitness and rmse of this evaluation -> pstats[p][2]; the single call's step on the pooled sums with
// P * S points.
template <bool PLANE>
__global__ __launch_bounds__(64) void icp_joint_tail_kernel(IcpState* __restrict__ st, const double* __restrict__ part,
                                                            int P, int S, double* __restrict__ pstats,
                                                            double rel_fitness, double rel_rmse, int last) {
  __shared__ double tot[ICP_PART];
  if (st->converged) return;
  constexpr int NV = PLANE ? PL_ACC : P2P_ACC;
  constexpr int ERR = PLANE ? 2 : 16;
  const int t = threadIdx.x;
  if (t < NV) {
    double v = part[t];
    for (int p = 1; p < P; ++p) v += part[p * ICP_PART + t];
    tot[t] = v;
  }
  if (t < P) {
    const double n = part[t * ICP_PART];
    pstats[t * 2] = n / (double)S;
    pstats[t * 2 + 1] = n > 0 ? sqrt(part[t * ICP_PART + ERR] / n) : 0.0;
  }
  __syncthreads();
  if (t != 0) return;
  double Tm[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) Tm[k] = st->T[k];
  const double points = (double)P * (double)S;
  if (PLANE)
    icp_plane_step(st, Tm, tot, points, rel_fitness, rel_rmse, last);
  else
    icp_p2p_step(st, Tm, tot, points, rel_fitness, rel_rmse, last);
}

// block b: state b from init_T[b] (identity when null)
__global__ void icp_batch_init_kernel(IcpState* states, const double* init_T) {
  icp_init_state(states + blockIdx.x, init_T ? init_T + blockIdx.x * 16 : nullptr);
}

// independent: block p -> out_T[p], out_stats[p][3]; shared: one block -> out_T, out_stats[3 + 2 P]
__global__ void icp_batch_finish_kernel(const IcpState* states, const double* pstats, int P, int shared, double* out_T,
                                        double* out_stats) {
  const int b = blockIdx.x, t = threadIdx.x;
  const IcpState* st = states + b;
  if (t < 16) out_T[b * 16 + t] = st->T[t];
  if (!out_stats) return;
  if (t == 0) {
    out_stats[b * 3] = st->fitness;
    out_stats[b * 3 + 1] = st->rmse;
    out_stats[b * 3 + 2] = (double)st->iterations;
  }
  if (shared && t < P) {
    out_stats[3 + t * 2] = pstats[t * 2];
    out_stats[3 + t * 2 + 1] = pstats[t * 2 + 1];
  }
}

// The one launch sequence: init, (max_iterations + 1) rounds of search + update (+ the tail in shared mode), finish -
// 2 + 2 (max_iterations + 1) launches, 3 per round in shared mode, no read-back and no host wait.  Evaluation
// 0 .. max_iterations: each update is followed by a re-evaluation, the last round only evaluates.  The arguments are
// checked by the entry point `who`, whose name the errors carry.  One independent problem without pre (the single calls)
// takes its update through icp_update_kernel / icp_plane_update_kernel, which measure about 2 us per launch faster than
// the batch update kernels at P = 1 and give the same bits; init, search and finish are the batch's.
static int icp_run(const char* who, const float* src, int64_t S, const double* pre, const float* tgt,
                   const float* tgt_normals, const IcpOffsets& off, int P, const double* init_T, int shared,
                   double max_distance, int max_iterations, double rel_fitness, double rel_rmse, void* workspace,
                   size_t workspace_bytes, double* out_T, double* out_stats, hipStream_t stream) {
  Workspace ws(workspace, workspace_bytes);
  IcpState* states = ws.take<IcpState>(P);
  int32_t* nn = ws.take<int32_t>((size_t)P * S);
  float* d2 = ws.take<float>((size_t)P * S);
  double* part = ws.take<double>((size_t)P * ICP_PART);
  double* pstats = ws.take<double>((size_t)P * 2);
  if (!ws.ok) {
    set_error("%s: workspace too small", who);
    return SV_ERR_WORKSPACE;
  }
  const unsigned nstates = shared ? 1u : (unsigned)P;
  const bool single = P == 1 && !shared && !pre;
  hipLaunchKernelGGL(icp_batch_init_kernel, dim3(nstates), dim3(64), 0, stream, states, init_T);
  const float max_d2 = (float)(max_distance * max_distance);
  const dim3 grid_nn((unsigned)((S + 255) / 256), (unsigned)P);
  for (int it = 0; it <= max_iterations; ++it) {
    const int last = it == max_iterations ? 1 : 0;
    hipLaunchKernelGGL(icp_batch_nn_kernel, grid_nn, dim3(256), 0, stream, src, (int)S, pre, tgt, off, states, shared,
                       max_d2, nn, d2);
    if (single && tgt_normals)
      hipLaunchKernelGGL(icp_plane_update_kernel, dim3(1), dim3(PL_THREADS), 0, stream, src, (int)S, tgt, tgt_normals, nn,
                         d2, states, rel_fitness, rel_rmse, last);
    else if (single)
      hipLaunchKernelGGL(icp_update_kernel, dim3(1), dim3(1024), 0, stream, src, (int)S, tgt, nn, d2, states, rel_fitness,
                         rel_rmse, last);
    else if (tgt_normals)
      hipLaunchKernelGGL(icp_batch_plane_update_kernel, dim3(P), dim3(PL_THREADS), 0, stream, src, (int)S, pre, tgt,
                         tgt_normals, off, nn, d2, states, shared, part, rel_fitness, rel_rmse, last);
    else
      hipLaunchKernelGGL(icp_batch_update_kernel, dim3(P), dim3(1024), 0, stream, src, (int)S, pre, tgt, off, nn, d2,
                         states, shared, part, rel_fitness, rel_rmse, last);
    if (shared && tgt_normals)
      hipLaunchKernelGGL(icp_joint_tail_kernel<true>, dim3(1), dim3(64), 0, stream, states, part, P, (int)S, pstats,
                         rel_fitness, rel_rmse, last);
    else if (shared)
      hipLaunchKernelGGL(icp_joint_tail_kernel<false>, dim3(1), dim3(64), 0, stream, states, part, P, (int)S, pstats,
                         rel_fitness, rel_rmse, last);
  }
  hipLaunchKernelGGL(icp_batch_finish_kernel, dim3(nstates), dim3(64), 0, stream, states, pstats, P, shared, out_T,
                     out_stats);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: hipGetLastError() -> %s", who, hipGetErrorString(e));
    return SV_ERR_HIP;
  }
  return SV_OK;
}

// one problem with T target points: rows 0 .. T - 1 (the unused entries repeat the end, as sv_icp_batched's do)
static IcpOffsets icp_single_offsets(int64_t T) {
  IcpOffsets off;
  off.v[0] = 0;
  for (int p = 1; p <= ICP_MAX_PROBLEMS; ++p) off.v[p] = (int32_t)T;
  return off;
}

}  // namespace sv

using namespace sv;

extern "C" {

size_t sv_icp_workspace_bytes(int64_t S) { return align_up(sizeof(IcpState), 256) + align_up((size_t)S * 4, 256) * 2 + 1024; }

int sv_icp_point2point(const float* src, int64_t S, const float* tgt, int64_t T, const double* init_T,
                       double max_distance, int max_iterations, double rel_fitness, double rel_rmse, void* workspace,
                       size_t workspace_bytes, double* out_T, double* out_stats, sv_stream_t stream_) {
  SV_CHECK_ARG(S >= 3 && T >= 1 && S < (1 << 24) && T < (1 << 24), "need at least 3 source points and 1 target point");
  SV_CHECK_ARG(max_iterations >= 0 && max_distance > 0, "bad parameters");
  SV_CHECK_ARG(src && tgt && out_T && workspace, "null pointer");
  return icp_run(__func__, src, S, nullptr, tgt, nullptr, icp_single_offsets(T), 1, init_T, 0, max_distance,
                 max_iterations, rel_fitness, rel_rmse, workspace, workspace_bytes, out_T, out_stats,
                 (hipStream_t)stream_);
}

size_t sv_icp_point2plane_workspace_bytes(int64_t S) { return sv_icp_workspace_bytes(S); }

int sv_icp_point2plane(const float* src, int64_t S, const float* tgt, const float* tgt_normals, int64_t T,
                       const double* init_T, double max_distance, int max_iterations, double rel_fitness,
                       double rel_rmse, void* workspace, size_t workspace_bytes, double* out_T, double* out_stats,
                       sv_stream_t stream_) {
  SV_CHECK_ARG(S >= 3 && T >= 1 && S < (1 << 24) && T < (1 << 24), "need at least 3 source points and 1 target point");
  SV_CHECK_ARG(max_iterations >= 0 && max_distance > 0, "bad parameters");
  SV_CHECK_ARG(src && tgt && tgt_normals && out_T && workspace, "null pointer");
  return icp_run(__func__, src, S, nullptr, tgt, tgt_normals, icp_single_offsets(T), 1, init_T, 0, max_distance,
                 max_iterations, rel_fitness, rel_rmse, workspace, workspace_bytes, out_T, out_stats,
                 (hipStream_t)stream_);
}

size_t sv_icp_batched_workspace_bytes(int64_t S, int P) {
  if (S < 0 || P < 0) return 0;
  const size_t p = (size_t)P;
  return align_up(p * sizeof(IcpState), 256) + align_up(p * (size_t)S * 4, 256) * 2 +
         align_up(p * ICP_PART * sizeof(double), 256) + align_up(p * 2 * sizeof(double), 256) + 1024;
}

int sv_icp_batched(const float* src, int64_t S, const double* pre, const float* tgt, const float* tgt_normals,
                   const int64_t* tgt_offsets, int P, const double* init_T, int shared, double max_distance,
                   int max_iterations, double rel_fitness, double rel_rmse, void* workspace, size_t workspace_bytes,
                   double* out_T, double* out_stats, sv_stream_t stream_) {
  SV_CHECK_ARG(P >= 1 && P <= ICP_MAX_PROBLEMS, "need 1 to 64 problems");
  SV_CHECK_ARG(S >= 3 && S < (1 << 24), "need 3 to 2^24 - 1 source points");
  SV_CHECK_ARG(max_iterations >= 0 && max_distance > 0 && (shared == 0 || shared == 1), "bad parameters");
  SV_CHECK_ARG(src && tgt && tgt_offsets && out_T && workspace, "null pointer");
  SV_CHECK_ARG(tgt_offsets[0] == 0, "tgt_offsets must start at 0");
  IcpOffsets off;
  off.v[0] = 0;
  for (int p = 0; p < P; ++p) {
    const int64_t T = tgt_offsets[p + 1] - tgt_offsets[p];
    SV_CHECK_ARG(T >= 1 && T < (1 << 24), "every problem needs 1 to 2^24 - 1 target points (ascending tgt_offsets)");
    off.v[p + 1] = (int32_t)tgt_offsets[p + 1];  // <= 64 * 2^24
  }
  for (int p = P + 1; p <= ICP_MAX_PROBLEMS; ++p) off.v[p] = off.v[P];
  return icp_run(__func__, src, S, pre, tgt, tgt_normals, off, P, init_T, shared, max_distance, max_iterations,
                 rel_fitness, rel_rmse, workspace, workspace_bytes, out_T, out_stats, (hipStream_t)stream_);
}

}  // extern "C"
