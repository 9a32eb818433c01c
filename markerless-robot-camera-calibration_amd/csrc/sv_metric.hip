// N10: the metric-learning criterion of train_feature-extractor.py:65-81 (MultiSimilarityMiner -> truncation ->
// TripletMarginLoss, both of pytorch_metric_learning with their defaults) on B embeddings of E floats, B <= SV_MAX_BATCH.
// The library sorts two [B, B] matrices, reads pair counts back, builds a [P, N] boolean matrix and a triplet list; the
// arithmetic is B^2 similarities and at most B^3 hinge terms.  Here everything is a row-owned pass over [B, B] matrices:
// workgroup i owns anchor i, nothing is proportional to the number of pairs or triplets, and nothing waits for the host.
// The contract is in include/sv_hip.h.
//
//   metric_norm_kernel     row i: ||x_i|| in float64, u_i = x_i / max(||x_i||, 1e-12) into the workspace, non-finite flag
//   metric_matrix_kernel   row i of S = u_i . u_j and / or D = ||u_i - u_j||: one wave per (i, j), lanes over e, a butterfly
//                          sum (every lane ends with the same bits; (i, j) and (j, i) run the same additions: S and D are
//                          bitwise symmetric)
//   ms_rank_kernel         row i: maxneg / minpos, the hard flags, and each hard column's rank among the row's hard columns
//                          of its kind in (S, column) order - a count over the row in LDS, no sort: code[i][j] = +(rank + 1)
//                          for a hard positive, -(rank + 1) for a hard negative, 0 otherwise; the row's two counts
//   ms_write_kernel        row i: its offsets are the sums of the counts of the rows before it (every workgroup adds them
//                          itself: B <= 1024 integers); writes the kept pairs at offset + rank and / or the row's 0 / 1
//                          multiplicities CP[i][:], CN[i][:]; workgroup 0 writes counts and n_nonfinite
//   tm_zero / tm_count     a given tuple -> multiplicity matrices CP[a][j], CN[a][j] (integer atomics; a pair given twice
//                          counts twice), out-of-range indices counted in n_invalid
//   tm_row_kernel          anchor i: sum over (j, k) of CP[i][j] CN[i][k] max(D[i][j] - D[i][k] + margin, 0) with thread c
//                          owning column c as the negative, j ascending; and the integer row of d sum / d D:
//                          W[i][c] = CP[i][c] #{violating negatives} - CN[i][c] #{violating positives}
//   tm_finish_kernel       the B row sums in ascending order -> sums, n_triplets
//   tm_grad_kernel         row i: g = sum_c (W[i][c] + W[c][i]) / D[i][c] (u_i - u_c), c ascending, then through the
//                          normalisation; float64 until the one rounding to float32
// No floating-point atomics; every float sum has an order fixed by (B, E).
#include "sv_common.h"

namespace sv {

constexpr int MT_BLOCK = 256;
constexpr int MT_WAVES = MT_BLOCK / 64;
constexpr double MT_NORM_EPS = 1e-12;  // F.normalize's clamp

struct MtAdd {
  template <typename T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct MtMax {
  __device__ __forceinline__ double operator()(double a, double b) const { return a > b ? a : b; }
};
struct MtMin {
  __device__ __forceinline__ double operator()(double a, double b) const { return a < b ? a : b; }
};

// every thread gets op over the workgroup's values: lanes by a butterfly, waves in wave order.  red: MT_WAVES slots of LDS.
template <typename T, typename Op>
__device__ __forceinline__ T mt_block_reduce(T v, T* red, Op op) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  T r = red[0];
#pragma unroll
  for (int w = 1; w < MT_WAVES; ++w) r = op(r, red[w]);
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(MT_BLOCK) void metric_norm_kernel(const float* __restrict__ x, int64_t ld, int E,
                                                               double* __restrict__ U, double* __restrict__ nrm,
                                                               int32_t* __restrict__ bad) {
  __shared__ double red[MT_WAVES];
  __shared__ long long redi[MT_WAVES];
  const int i = blockIdx.x;
  const float* row = x + (int64_t)i * ld;
  double s = 0.0;
  long long nonfinite = 0;
  for (int e = threadIdx.x; e < E; e += MT_BLOCK) {
    const float v = row[e];
    nonfinite += (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
    s += (double)v * (double)v;
  }
  s = mt_block_reduce(s, red, MtAdd());
  nonfinite = mt_block_reduce(nonfinite, redi, MtAdd());
  const double n = sqrt(s);
  const double div = n > MT_NORM_EPS ? n : MT_NORM_EPS;
  for (int e = threadIdx.x; e < E; e += MT_BLOCK) U[(int64_t)i * E + e] = (double)row[e] / div;
  if (threadIdx.x == 0) {
    nrm[i] = n;
    bad[i] = nonfinite != 0;
  }
}

template <bool WANT_S, bool WANT_D>
__global__ __launch_bounds__(MT_BLOCK) void metric_matrix_kernel(const double* __restrict__ U, int B, int E,
                                                                 double* __restrict__ S, double* __restrict__ D) {
  const int i = blockIdx.x, lane = threadIdx.x & 63;
  const double* ui = U + (int64_t)i * E;
  for (int j = threadIdx.x >> 6; j < B; j += MT_WAVES) {
    const double* uj = U + (int64_t)j * E;
    double s = 0.0, d = 0.0;
    for (int e = lane; e < E; e += 64) {
      const double a = ui[e], b = uj[e];
      if (WANT_S) s += a * b;
      if (WANT_D) {
        const double t = a - b;
        d += t * t;
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      if (WANT_S) s += __shfl_xor(s, o);
      if (WANT_D) d += __shfl_xor(d, o);
    }
    if (lane == 0) {
      if (WANT_S) S[(int64_t)i * B + j] = s;
      if (WANT_D) D[(int64_t)i * B + j] = sqrt(d);
    }
  }
}

// kind of column j for anchor i: 1 positive, 2 negative, 0 neither (itself, or either row non-finite)
__global__ __launch_bounds__(MT_BLOCK) void ms_rank_kernel(const double* __restrict__ S, const int64_t* __restrict__ labels,
                                                           const int32_t* __restrict__ bad, int B, double epsilon,
                                                           int32_t* __restrict__ code, int32_t* __restrict__ rowcnt) {
  __shared__ double s[SV_MAX_BATCH];
  __shared__ unsigned char kind[SV_MAX_BATCH];
  __shared__ double red[MT_WAVES];
  __shared__ long long redi[MT_WAVES];
  const int i = blockIdx.x;
  const int64_t yi = labels[i];
  const bool bad_i = bad[i] != 0;
  double maxneg = -INFINITY, minpos = INFINITY;
  for (int j = threadIdx.x; j < B; j += MT_BLOCK) {
    const double v = S[(int64_t)i * B + j];
    int k = 0;
    if (!bad_i && j != i && !bad[j]) k = labels[j] == yi ? 1 : 2;
    s[j] = v;
    kind[j] = (unsigned char)k;
    if (k == 1 && v < minpos) minpos = v;
    if (k == 2 && v > maxneg) maxneg = v;
  }
  maxneg = mt_block_reduce(maxneg, red, MtMax());  // the syncs inside also publish s and kind
  minpos = mt_block_reduce(minpos, red, MtMin());
  for (int j = threadIdx.x; j < B; j += MT_BLOCK) {
    const int k = kind[j];
    const bool hard = k == 1 ? s[j] - epsilon < maxneg : (k == 2 ? s[j] + epsilon > minpos : false);
    kind[j] = (unsigned char)(hard ? k : 0);  // own slot only
  }
  __syncthreads();
  long long n_pos = 0, n_neg = 0;
  for (int j = threadIdx.x; j < B; j += MT_BLOCK) {
    const int k = kind[j];
    int c = 0;
    if (k) {
      const double v = s[j];
      int r = 0;
      for (int o = 0; o < B; ++o) r += kind[o] == k && (s[o] < v || (s[o] == v && o < j));
      c = k == 1 ? r + 1 : -(r + 1);
      n_pos += k == 1;
      n_neg += k == 2;
    }
    code[(int64_t)i * B + j] = c;
  }
  n_pos = mt_block_reduce(n_pos, redi, MtAdd());
  n_neg = mt_block_reduce(n_neg, redi, MtAdd());
  if (threadIdx.x == 0) {
    rowcnt[2 * i] = (int)n_pos;
    rowcnt[2 * i + 1] = (int)n_neg;
  }
}

static __host__ __device__ __forceinline__ int64_t mt_kept(int64_t total, int64_t cap, int64_t capacity) {
  int64_t k = total;
  if (cap >= 0 && cap < k) k = cap;
  if (capacity < k) k = capacity;
  return k;
}

// a1 / p / a2 / n may be NULL (capacity INT64_MAX then), and so may CP / CN
__global__ __launch_bounds__(MT_BLOCK) void ms_write_kernel(const int32_t* __restrict__ code, const int32_t* __restrict__ rowcnt,
                                                            const int32_t* __restrict__ bad, int B, int64_t max_pos,
                                                            int64_t max_neg, int64_t* __restrict__ a1, int64_t* __restrict__ p,
                                                            int64_t cap_pos, int64_t* __restrict__ a2, int64_t* __restrict__ n,
                                                            int64_t cap_neg, int32_t* __restrict__ CP, int32_t* __restrict__ CN,
                                                            int64_t* __restrict__ counts, int32_t* __restrict__ n_nonfinite) {
  __shared__ long long redi[MT_WAVES];
  const int i = blockIdx.x;
  long long before_p = 0, before_n = 0, total_p = 0, total_n = 0, n_bad = 0;
  for (int r = threadIdx.x; r < B; r += MT_BLOCK) {
    const int cp = rowcnt[2 * r], cn = rowcnt[2 * r + 1];
    total_p += cp;
    total_n += cn;
    if (r < i) {
      before_p += cp;
      before_n += cn;
    }
    n_bad += bad[r] != 0;
  }
  before_p = mt_block_reduce(before_p, redi, MtAdd());
  before_n = mt_block_reduce(before_n, redi, MtAdd());
  total_p = mt_block_reduce(total_p, redi, MtAdd());
  total_n = mt_block_reduce(total_n, redi, MtAdd());
  const int64_t kept_p = mt_kept(total_p, max_pos, cap_pos), kept_n = mt_kept(total_n, max_neg, cap_neg);
  if (i == 0) {
    n_bad = mt_block_reduce(n_bad, redi, MtAdd());
    if (threadIdx.x == 0) {
      counts[0] = kept_p;
      counts[1] = kept_n;
      counts[2] = total_p;
      counts[3] = total_n;
      n_nonfinite[0] = (int)n_bad;
    }
  }
  for (int j = threadIdx.x; j < B; j += MT_BLOCK) {
    const int c = code[(int64_t)i * B + j];
    const int64_t at = c > 0 ? before_p + c - 1 : before_n - c - 1;
    const bool keep_p = c > 0 && at < kept_p, keep_n = c < 0 && at < kept_n;
    if (keep_p && a1) {
      a1[at] = i;
      p[at] = j;
    }
    if (keep_n && a2) {
      a2[at] = i;
      n[at] = j;
    }
    if (CP) {
      CP[(int64_t)i * B + j] = keep_p;
      CN[(int64_t)i * B + j] = keep_n;
    }
  }
}

__global__ __launch_bounds__(256) void tm_zero_kernel(int32_t* __restrict__ C2, int64_t cells, int32_t* __restrict__ n_invalid) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < cells) C2[t] = 0;
  if (t == 0) n_invalid[0] = 0;
}

// threads [0, cap_pos) take the positive list, [cap_pos, cap_pos + cap_neg) the negative one; the lengths come from the device
__global__ __launch_bounds__(256) void tm_count_kernel(const int64_t* __restrict__ a1, const int64_t* __restrict__ p,
                                                        int64_t cap_pos, const int64_t* __restrict__ a2,
                                                        const int64_t* __restrict__ n, int64_t cap_neg,
                                                        const int64_t* __restrict__ counts, int B, int32_t* __restrict__ CP,
                                                        int32_t* __restrict__ CN, int32_t* __restrict__ n_invalid) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool pos = t < cap_pos;
  const int64_t s = pos ? t : t - cap_pos;
  const int64_t len = pos ? counts[0] : counts[1];
  if (s >= (pos ? cap_pos : cap_neg) || s >= len) return;  // a negative length keeps nothing
  const int64_t a = pos ? a1[s] : a2[s], j = pos ? p[s] : n[s];
  if (a < 0 || a >= B || j < 0 || j >= B) {
    atomicAdd(n_invalid, 1);
    return;
  }
  atomicAdd((pos ? CP : CN) + a * B + j, 1);
}

__global__ __launch_bounds__(MT_BLOCK) void tm_row_kernel(const double* __restrict__ D, const int32_t* __restrict__ CP,
                                                          const int32_t* __restrict__ CN, int B, double margin,
                                                          double* __restrict__ W, double* __restrict__ row_sum,
                                                          int64_t* __restrict__ row_nz, int64_t* __restrict__ row_triplets) {
  __shared__ double d[SV_MAX_BATCH];
  __shared__ int cp[SV_MAX_BATCH];
  __shared__ int cn[SV_MAX_BATCH];
  __shared__ double red[MT_WAVES];
  __shared__ long long redi[MT_WAVES];
  const int i = blockIdx.x;
  long long n_p = 0, n_n = 0;
  for (int c = threadIdx.x; c < B; c += MT_BLOCK) {
    d[c] = D[(int64_t)i * B + c];
    n_p += cp[c] = CP[(int64_t)i * B + c];
    n_n += cn[c] = CN[(int64_t)i * B + c];
  }
  n_p = mt_block_reduce(n_p, redi, MtAdd());  // the syncs inside also publish d, cp and cn
  n_n = mt_block_reduce(n_n, redi, MtAdd());
  double loss = 0.0;
  long long nz = 0;
  for (int c = threadIdx.x; c < B; c += MT_BLOCK) {
    const int cpc = cp[c], cnc = cn[c];
    const double dc = d[c];
    long long viol_n = 0, viol_p = 0;  // violating triplets with c as the negative / as the positive
    if (n_p != 0 && n_n != 0 && (cpc | cnc)) {
      for (int o = 0; o < B; ++o) {
        if (cnc && cp[o]) {
          const double l = d[o] - dc + margin;
          if (!(l <= 0.0)) {  // NaN counts as violating and makes the sum NaN
            const long long m = (long long)cp[o] * cnc;
            loss += (double)m * l;
            nz += m;
            viol_n += cp[o];
          }
        }
        if (cpc && cn[o]) {
          const double l = dc - d[o] + margin;
          if (!(l <= 0.0)) viol_p += cn[o];
        }
      }
    }
    W[(int64_t)i * B + c] = (double)(cpc * viol_p - cnc * viol_n);
  }
  loss = mt_block_reduce(loss, red, MtAdd());
  nz = mt_block_reduce(nz, redi, MtAdd());
  if (threadIdx.x == 0) {
    row_sum[i] = loss;
    row_nz[i] = nz;
    row_triplets[i] = n_p * n_n;
  }
}

__global__ __launch_bounds__(MT_BLOCK) void tm_finish_kernel(const double* __restrict__ row_sum, const int64_t* __restrict__ row_nz,
                                                             const int64_t* __restrict__ row_triplets, int B,
                                                             double* __restrict__ sums, int64_t* __restrict__ n_triplets) {
  __shared__ double red[MT_WAVES];
  __shared__ long long redi[MT_WAVES];
  double a = 0.0;
  long long nz = 0, nt = 0;
  for (int r = threadIdx.x; r < B; r += MT_BLOCK) {  // ascending rows
    a += row_sum[r];
    nz += row_nz[r];
    nt += row_triplets[r];
  }
  a = mt_block_reduce(a, red, MtAdd());
  nz = mt_block_reduce(nz, redi, MtAdd());
  nt = mt_block_reduce(nt, redi, MtAdd());
  if (threadIdx.x == 0) {
    sums[0] = a;
    sums[1] = (double)nz;
    n_triplets[0] = nt;
  }
}

__global__ __launch_bounds__(MT_BLOCK) void tm_grad_kernel(const double* __restrict__ U, const double* __restrict__ nrm,
                                                           const double* __restrict__ D, const double* __restrict__ W, int B,
                                                           int E, double* __restrict__ G, float* __restrict__ grad) {
  __shared__ double coef[SV_MAX_BATCH];
  __shared__ double red[MT_WAVES];
  __shared__ long long redi[MT_WAVES];
  const int i = blockIdx.x;
  long long live = 0;
  for (int c = threadIdx.x; c < B; c += MT_BLOCK) {
    const double w = W[(int64_t)i * B + c] + W[(int64_t)c * B + i];  // integers: exact
    const double dist = D[(int64_t)i * B + c];
    const double q = (w != 0.0 && dist != 0.0) ? w / dist : 0.0;  // d = 0: subgradient 0
    coef[c] = q;
    live += q != 0.0;
  }
  live = mt_block_reduce(live, redi, MtAdd());  // publishes coef
  float* out = grad + (int64_t)i * E;
  if (live == 0) {  // a row in no violating triplet (or a non-finite row that joined no pair): exactly 0
    for (int e = threadIdx.x; e < E; e += MT_BLOCK) out[e] = 0.0f;
    return;
  }
  const double* ui = U + (int64_t)i * E;
  double* g = G + (int64_t)i * E;
  double dot = 0.0;
  for (int e = threadIdx.x; e < E; e += MT_BLOCK) {
    const double a = ui[e];
    double acc = 0.0;
    for (int c = 0; c < B; ++c) {
      const double q = coef[c];
      if (q != 0.0) acc += q * (a - U[(int64_t)c * E + e]);
    }
    g[e] = acc;  // read back by this thread only
    dot += acc * a;
  }
  dot = mt_block_reduce(dot, red, MtAdd());
  const double n = nrm[i];
  for (int e = threadIdx.x; e < E; e += MT_BLOCK) {
    // u = x / max(|x|, eps): above the clamp d u / d x = (I - u u^T) / |x|, at or below it I / eps
    const double v = n > MT_NORM_EPS ? (g[e] - ui[e] * dot) / n : g[e] / MT_NORM_EPS;
    out[e] = (float)v;
  }
}

struct MetricWs {
  double *U, *G, *nrm, *S, *D, *W, *row_sum;
  int32_t *bad, *code, *rowcnt, *C2;
  int64_t *row_nz, *row_triplets;
  bool ok;
};

static MetricWs metric_take(void* workspace, size_t bytes, int B, int E) {
  Workspace ws(workspace, bytes);
  const size_t b = (size_t)B, bb = b * b, be = b * (size_t)E;
  MetricWs m;
  m.U = ws.take<double>(be);
  m.G = ws.take<double>(be);
  m.nrm = ws.take<double>(b);
  m.S = ws.take<double>(bb);
  m.D = ws.take<double>(bb);
  m.W = ws.take<double>(bb);
  m.row_sum = ws.take<double>(b);
  m.bad = ws.take<int32_t>(b);
  m.code = ws.take<int32_t>(bb);
  m.rowcnt = ws.take<int32_t>(2 * b);
  m.C2 = ws.take<int32_t>(2 * bb);  // CP then CN
  m.row_nz = ws.take<int64_t>(b);
  m.row_triplets = ws.take<int64_t>(b);
  m.ok = ws.ok;
  return m;
}

static size_t metric_bytes(int B, int E) {
  const size_t b = (size_t)B, bb = b * b, be = b * (size_t)E;
  size_t total = 0;
  for (size_t part : {be * 8, be * 8, b * 8, bb * 8, bb * 8, bb * 8, b * 8, b * 4, bb * 4, 2 * b * 4, 2 * bb * 4, b * 8, b * 8})
    total = align_up(total, 256) + part;
  return align_up(total, 256);
}

#define MT_CHECK_SHAPE()                                                        \
  SV_CHECK_ARG(B >= 1 && B <= SV_MAX_BATCH, "need 1 to 1024 embeddings");        \
  SV_CHECK_ARG(E >= 1, "need E >= 1");                                           \
  SV_CHECK_ARG(ld >= E, "need ld >= E")

static void metric_launch_loss(const MetricWs& m, int B, int E, double margin, double* sums, float* grad, int64_t* n_triplets,
                               hipStream_t stream) {
  int32_t* CP = m.C2;
  int32_t* CN = m.C2 + (size_t)B * B;
  hipLaunchKernelGGL(tm_row_kernel, dim3(B), dim3(MT_BLOCK), 0, stream, m.D, CP, CN, B, margin, m.W, m.row_sum, m.row_nz,
                     m.row_triplets);
  hipLaunchKernelGGL(tm_finish_kernel, dim3(1), dim3(MT_BLOCK), 0, stream, m.row_sum, m.row_nz, m.row_triplets, B, sums,
                     n_triplets);
  if (grad) hipLaunchKernelGGL(tm_grad_kernel, dim3(B), dim3(MT_BLOCK), 0, stream, m.U, m.nrm, m.D, m.W, B, E, m.G, grad);
}

}  // namespace sv

using namespace sv;

extern "C" {

size_t sv_metric_workspace_bytes(int B, int E) {
  if (B < 1) B = 1;
  if (B > SV_MAX_BATCH) B = SV_MAX_BATCH;
  if (E < 1) E = 1;
  return metric_bytes(B, E);
}

int sv_ms_mine(const float* x, int64_t ld, int B, int E, const int64_t* labels, double epsilon, int64_t max_pos, int64_t max_neg,
               void* workspace, size_t workspace_bytes, int64_t* a1, int64_t* p, int64_t cap_pos, int64_t* a2, int64_t* n,
               int64_t cap_neg, int64_t* counts, int32_t* n_nonfinite, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  MT_CHECK_SHAPE();
  SV_CHECK_ARG(cap_pos >= 0 && cap_neg >= 0, "need capacities >= 0");
  SV_CHECK_ARG(max_pos >= -1 && max_neg >= -1, "need caps >= -1");
  SV_CHECK_ARG(x && labels && workspace && counts && n_nonfinite && ((a1 && p) || cap_pos == 0) && ((a2 && n) || cap_neg == 0),
               "null pointer");
  const MetricWs m = metric_take(workspace, workspace_bytes, B, E);
  SV_CHECK_ARG(m.ok && workspace_bytes >= metric_bytes(B, E), "workspace too small");
  hipLaunchKernelGGL(metric_norm_kernel, dim3(B), dim3(MT_BLOCK), 0, stream, x, ld, E, m.U, m.nrm, m.bad);
  hipLaunchKernelGGL((metric_matrix_kernel<true, false>), dim3(B), dim3(MT_BLOCK), 0, stream, m.U, B, E, m.S, nullptr);
  hipLaunchKernelGGL(ms_rank_kernel, dim3(B), dim3(MT_BLOCK), 0, stream, m.S, labels, m.bad, B, epsilon, m.code, m.rowcnt);
  hipLaunchKernelGGL(ms_write_kernel, dim3(B), dim3(MT_BLOCK), 0, stream, m.code, m.rowcnt, m.bad, B, max_pos, max_neg,
                     cap_pos ? a1 : nullptr, p, cap_pos, cap_neg ? a2 : nullptr, n, cap_neg, nullptr, nullptr, counts,
                     n_nonfinite);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

int sv_triplet_margin(const float* x, int64_t ld, int B, int E, const int64_t* a1, const int64_t* p, int64_t cap_pos,
                      const int64_t* a2, const int64_t* n, int64_t cap_neg, const int64_t* counts, double margin,
                      void* workspace, size_t workspace_bytes, double* sums, float* grad, int64_t* n_triplets,
                      int32_t* n_invalid, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  MT_CHECK_SHAPE();
  SV_CHECK_ARG(cap_pos >= 0 && cap_neg >= 0 && cap_pos <= INT32_MAX && cap_neg <= INT32_MAX, "need 0 <= capacities < 2^31");
  SV_CHECK_ARG(x && counts && workspace && sums && n_triplets && n_invalid && ((a1 && p) || cap_pos == 0) &&
                   ((a2 && n) || cap_neg == 0),
               "null pointer");
  const MetricWs m = metric_take(workspace, workspace_bytes, B, E);
  SV_CHECK_ARG(m.ok && workspace_bytes >= metric_bytes(B, E), "workspace too small");
  const int64_t cells = 2 * (int64_t)B * B;
  hipLaunchKernelGGL(tm_zero_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, m.C2, cells, n_invalid);
  if (cap_pos + cap_neg > 0)
    hipLaunchKernelGGL(tm_count_kernel, dim3((unsigned)((cap_pos + cap_neg + 255) / 256)), dim3(256), 0, stream, a1, p, cap_pos,
                       a2, n, cap_neg, counts, B, m.C2, m.C2 + (size_t)B * B, n_invalid);
  hipLaunchKernelGGL(metric_norm_kernel, dim3(B), dim3(MT_BLOCK), 0, stream, x, ld, E, m.U, m.nrm, m.bad);
  hipLaunchKernelGGL((metric_matrix_kernel<false, true>), dim3(B), dim3(MT_BLOCK), 0, stream, m.U, B, E, nullptr, m.D);
  metric_launch_loss(m, B, E, margin, sums, grad, n_triplets, stream);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

int sv_mined_triplet_step(const float* x, int64_t ld, int B, int E, const int64_t* labels, double epsilon, double margin,
                          int64_t max_pos, int64_t max_neg, void* workspace, size_t workspace_bytes, double* sums, float* grad,
                          int64_t* counts, int64_t* n_triplets, int32_t* n_nonfinite, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  MT_CHECK_SHAPE();
  SV_CHECK_ARG(max_pos >= -1 && max_neg >= -1, "need caps >= -1");
  SV_CHECK_ARG(x && labels && workspace && sums && counts && n_triplets && n_nonfinite, "null pointer");
  const MetricWs m = metric_take(workspace, workspace_bytes, B, E);
  SV_CHECK_ARG(m.ok && workspace_bytes >= metric_bytes(B, E), "workspace too small");
  hipLaunchKernelGGL(metric_norm_kernel, dim3(B), dim3(MT_BLOCK), 0, stream, x, ld, E, m.U, m.nrm, m.bad);
  hipLaunchKernelGGL((metric_matrix_kernel<true, true>), dim3(B), dim3(MT_BLOCK), 0, stream, m.U, B, E, m.S, m.D);
  hipLaunchKernelGGL(ms_rank_kernel, dim3(B), dim3(MT_BLOCK), 0, stream, m.S, labels, m.bad, B, epsilon, m.code, m.rowcnt);
  hipLaunchKernelGGL(ms_write_kernel, dim3(B), dim3(MT_BLOCK), 0, stream, m.code, m.rowcnt, m.bad, B, max_pos, max_neg,
                     nullptr, nullptr, INT64_MAX, nullptr, nullptr, INT64_MAX, m.C2, m.C2 + (size_t)B * B, counts, n_nonfinite);
  metric_launch_loss(m, B, E, margin, sums, grad, n_triplets, stream);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

}  // extern "C"
