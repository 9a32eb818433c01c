// N5: the training-time point augmentation of the reference's utils/augmentation.py (:14-33 distort_elastic, :49-51
// add_noise, :54-61 transform_random, :64-67 flip_random, :70-75 rotate_along_gravity, :108-138 augment_segmentation) and
// the quantisation that follows it in data/alivev2.py:199-208,290-296, for a whole batch of frames per call.  The
// reference spends most of its time in scipy's RegularGridInterpolator, one Python call per field component; here a
// point is read once, walks every enabled stage in registers (float64, the reference's operation order, no fma) and is
// written once.  The contract (table layout, rounding, edge cases) is in include/sv_hip.h.
//
//   field_blur_kernel   one 3-tap box blur along one axis of every field of a launch (grid.y = field); six launches
//                       ping-pong between the workspace and `out`
//   aug_plan_kernel     1 workgroup: first workgroup of every frame (prefix sum of ceil(rows / 256)), so that the grid
//                       depends on (N, B) only and no workgroup straddles frames
//   aug_points_kernel   one point per lane; the frame's table row sits in LDS; per-workgroup min / max to the workspace
//   aug_stats_kernel    one wave per frame: thread c folds component c of the frame's partials
//   quantise_kernel     one point per lane: subtract the frame's origin, floor(p / size), one 16-byte store per row
// No atomics; min and max do not depend on the order, so two runs give the same bits.
#include "sv_common.h"

namespace sv {

constexpr int AUG_BLOCK = 256;
constexpr int FIELD_CHUNK = 32;     // fields per blur launch (their shapes travel as kernel arguments)
constexpr int FIELD_MAX_DIM = 1024;

struct FieldTable {
  long long first[FIELD_CHUNK];  // offset of the field's first float in `raw` / `out`
  int bx[FIELD_CHUNK], by[FIELD_CHUNK], bz[FIELD_CHUNK];
};

// scipy.ndimage.convolve(x, ones(3) / 3 as float32, mode='constant', cval=0) along one axis: products and sum in
// double with the float32 weight, one rounding to float32
__global__ __launch_bounds__(AUG_BLOCK) void field_blur_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                               FieldTable t, int axis) {
  const int f = blockIdx.y;
  const int bx = t.bx[f], by = t.by[f], bz = t.bz[f];
  const int cells = bx * by * bz;
  const int e = blockIdx.x * AUG_BLOCK + threadIdx.x;
  if (e >= 3 * cells) return;
  const int cell = e % cells;
  const int iz = cell % bz, iy = (cell / bz) % by, ix = cell / (bz * by);
  const int pos = axis == 0 ? ix : (axis == 1 ? iy : iz);
  const int dim = axis == 0 ? bx : (axis == 1 ? by : bz);
  const int stride = axis == 0 ? by * bz : (axis == 1 ? bz : 1);
  const float* p = in + t.first[f] + e;
  const double w = (double)(1.0f / 3.0f);
  const double a = pos > 0 ? (double)p[-stride] : 0.0;
  const double b = (double)p[0];
  const double c = pos < dim - 1 ? (double)p[stride] : 0.0;
  out[t.first[f] + e] = (float)((a * w + b * w) + c * w);
}

struct AugRange {
  int b, lo, hi, first;  // frame, its row range [lo, hi) and the first row of this workgroup
};

// rows of frame b, whatever `offsets` holds: both ends inside [0, N] and hi >= lo, so no row index leaves the arrays
__device__ __forceinline__ void aug_frame_rows(const int32_t* __restrict__ offsets, int b, int N, int& lo, int& hi) {
  lo = min(max(offsets[b], 0), N);
  hi = min(max(offsets[b + 1], lo), N);
}

__global__ __launch_bounds__(1024) void aug_plan_kernel(const int32_t* __restrict__ offsets, int N, int B,
                                                        int32_t* __restrict__ blk_start) {
  __shared__ int scan[1024];
  const int b = threadIdx.x;
  int cnt = 0;
  if (b < B) {
    int lo, hi;
    aug_frame_rows(offsets, b, N, lo, hi);
    cnt = (hi - lo + AUG_BLOCK - 1) / AUG_BLOCK;
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

// the frame whose workgroups include workgroup g (empty frames own none); false past the last one
__device__ __forceinline__ bool aug_resolve(const int32_t* __restrict__ blk_start, const int32_t* __restrict__ offsets,
                                            int N, int B, int g, AugRange& r) {
  if (g >= blk_start[B]) return false;
  int lo = 0, hi = B;  // largest b with blk_start[b] <= g
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (blk_start[mid] <= g) lo = mid; else hi = mid;
  }
  r.b = lo;
  aug_frame_rows(offsets, lo, N, r.lo, r.hi);
  r.first = r.lo + (g - blk_start[lo]) * AUG_BLOCK;
  return true;
}

// numpy's min / max: a NaN on either side wins
__device__ __forceinline__ double nan_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }

// One axis of RegularGridInterpolator on np.linspace(-(b - 1) * gran, (b - 1) * gran, b): cell k with node(k) <= v <
// node(k + 1) (the last cell includes its upper node), t = (v - node(k)) / (node(k + 1) - node(k)).  Returns false when v
// lies outside [node(0), node(b - 1)].  b >= 2.
struct AugAxis {
  double start, stop, step;
  int b;
  __device__ __forceinline__ AugAxis(int b_, double gran) : b(b_) {
    stop = (double)(b_ - 1) * gran;
    start = -stop;
    step = (stop - start) / (double)(b_ - 1);
  }
  __device__ __forceinline__ double node(int k) const { return k == b - 1 ? stop : (double)k * step + start; }
  __device__ __forceinline__ bool locate(double v, int& k, double& t) const {
    if (v < node(0) || v > stop) return false;
    // clamped in double first: the quotient of a huge coordinate does not fit an int
    k = (int)fmin(fmax(floor((v - start) / step), 0.0), (double)(b - 2));
    while (k > 0 && node(k) > v) --k;
    while (k < b - 2 && node(k + 1) <= v) ++k;
    const double n0 = node(k);
    t = (v - n0) / (node(k + 1) - n0);
    return true;
  }
};

// x += mag * trilinear(field)(x) for one elastic stage; prm points at the stage's seven table entries
__device__ __forceinline__ void aug_elastic(const double* prm, const float* __restrict__ fields, long long fields_len,
                                            double& x, double& y, double& z) {
  const long long off = (long long)prm[SV_AUG_E_OFFSET];
  const int bx = (int)prm[SV_AUG_E_BX], by = (int)prm[SV_AUG_E_BY], bz = (int)prm[SV_AUG_E_BZ];
  const double gran = prm[SV_AUG_E_GRAN], mag = prm[SV_AUG_E_MAG];
  double d[3] = {0.0, 0.0, 0.0};
  const bool dims_ok = bx >= 2 && by >= 2 && bz >= 2 && bx <= FIELD_MAX_DIM && by <= FIELD_MAX_DIM && bz <= FIELD_MAX_DIM;
  const long long cells = dims_ok ? (long long)bx * by * bz : 0;
  if (!dims_ok || off < 0 || 3 * cells > fields_len || off > fields_len - 3 * cells || x != x || y != y || z != z) {
    // a NaN coordinate gives a NaN row (scipy's f(nan) = nan); so does a table row that points outside `fields`
    d[0] = d[1] = d[2] = NAN;
  } else {
    int ix, iy, iz;
    double tx, ty, tz;
    const AugAxis ax(bx, gran), ay(by, gran), az(bz, gran);
    // all three evaluated (no short-circuit): ix, iy, iz are only used when every axis is inside
    const bool in_x = ax.locate(x, ix, tx), in_y = ay.locate(y, iy, ty), in_z = az.locate(z, iz, tz);
    if (in_x && in_y && in_z) {  // outside the grid: fill_value = 0
      const float* base = fields + off + ((long long)ix * by + iy) * bz + iz;
      const double wx[2] = {1.0 - tx, tx}, wy[2] = {1.0 - ty, ty}, wz[2] = {1.0 - tz, tz};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float* v = base + c * cells;
        double s = 0.0;  // the hypercube's corners in scipy's order (z fastest), weight ((1 * wx) * wy) * wz
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 2; ++k) s = s + (double)v[(i * by + j) * bz + k] * ((wx[i] * wy[j]) * wz[k]);
        d[c] = s;
      }
    }
  }
  x = x + d[0] * mag;
  y = y + d[1] * mag;
  z = z + d[2] * mag;
}

// row (x, y, z) times the 3x3 matrix whose column c is (m0[c], m1[c], m2[c])
#define SV_AUG_DOT(a0, a1, a2) ((x * (a0) + y * (a1)) + z * (a2))

template <typename T>
__global__ __launch_bounds__(AUG_BLOCK) void aug_points_kernel(
    const T* __restrict__ points, const int32_t* __restrict__ offsets, int N, int B, const double* __restrict__ table,
    const float* __restrict__ fields, long long fields_len, const double* __restrict__ noise,
    const int32_t* __restrict__ blk_start, double* __restrict__ out, double* __restrict__ partial) {
  __shared__ double prm[SV_AUG_STRIDE];
  __shared__ double red[AUG_BLOCK / 64][6];
  AugRange r;
  if (!aug_resolve(blk_start, offsets, N, B, blockIdx.x, r)) return;  // uniform over the workgroup
  if (threadIdx.x < SV_AUG_STRIDE) prm[threadIdx.x] = table[(size_t)r.b * SV_AUG_STRIDE + threadIdx.x];
  __syncthreads();
  const int i = r.first + threadIdx.x;
  const bool live = i < r.hi;
  double s[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  if (live) {
    double x = points[(size_t)i * 3], y = points[(size_t)i * 3 + 1], z = points[(size_t)i * 3 + 2];
    if (prm[SV_AUG_ELASTIC0 + SV_AUG_E_ON] != 0.0) aug_elastic(prm + SV_AUG_ELASTIC0, fields, fields_len, x, y, z);
    if (prm[SV_AUG_ELASTIC1 + SV_AUG_E_ON] != 0.0) aug_elastic(prm + SV_AUG_ELASTIC1, fields, fields_len, x, y, z);
    if (prm[SV_AUG_NOISE_ON] != 0.0 && noise) {  // x + clip(sigma * n, -clip, clip); a NaN draw stays NaN
      const double sigma = prm[SV_AUG_NOISE_SIGMA], clip = prm[SV_AUG_NOISE_CLIP];
      double n[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double v = sigma * noise[(size_t)i * 3 + c];
        n[c] = v < -clip ? -clip : (v > clip ? clip : v);
      }
      x = x + n[0], y = y + n[1], z = z + n[2];
    }
    if (prm[SV_AUG_TRANSFORM_ON] != 0.0) {  // (pc @ rot + t) @ rot.T, both products kept
      const double* R = prm + SV_AUG_ROT;
      const double px = SV_AUG_DOT(R[0], R[3], R[6]) + prm[SV_AUG_TRANSLATION];
      const double py = SV_AUG_DOT(R[1], R[4], R[7]) + prm[SV_AUG_TRANSLATION + 1];
      const double pz = SV_AUG_DOT(R[2], R[5], R[8]) + prm[SV_AUG_TRANSLATION + 2];
      x = px, y = py, z = pz;
      const double qx = SV_AUG_DOT(R[0], R[1], R[2]), qy = SV_AUG_DOT(R[3], R[4], R[5]), qz = SV_AUG_DOT(R[6], R[7], R[8]);
      x = qx, y = qy, z = qz;
    }
    if (prm[SV_AUG_FLIP_SIGN] != 0.0) {  // pc @ diag(sign, 1, 1) as the full product: inf * 0 is NaN there too
      const double sg = prm[SV_AUG_FLIP_SIGN];
      const double qx = SV_AUG_DOT(sg, 0.0, 0.0), qy = SV_AUG_DOT(0.0, 1.0, 0.0), qz = SV_AUG_DOT(0.0, 0.0, 1.0);
      x = qx, y = qy, z = qz;
    }
    if (prm[SV_AUG_GRAVITY_ON] != 0.0) {  // (rot @ pc.T).T, rot = [[c, 0, -s], [0, 1, 0], [s, 0, c]]
      const double cs = prm[SV_AUG_GRAVITY_COS], sn = prm[SV_AUG_GRAVITY_SIN];
      const double qx = SV_AUG_DOT(cs, 0.0, -sn), qy = SV_AUG_DOT(0.0, 1.0, 0.0), qz = SV_AUG_DOT(sn, 0.0, cs);
      x = qx, y = qy, z = qz;
    }
    out[(size_t)i * 3] = x;
    out[(size_t)i * 3 + 1] = y;
    out[(size_t)i * 3 + 2] = z;
    s[0] = s[3] = x, s[1] = s[4] = y, s[2] = s[5] = z;
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double v = s[c];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const double o = __shfl_xor(v, d);
      v = c < 3 ? nan_min(v, o) : nan_max(v, o);
    }
    s[c] = v;
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 6; ++c) red[threadIdx.x >> 6][c] = s[c];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int c = threadIdx.x;
    double v = red[0][c];
    for (int w = 1; w < AUG_BLOCK / 64; ++w) v = c < 3 ? nan_min(v, red[w][c]) : nan_max(v, red[w][c]);
    partial[(size_t)blockIdx.x * 6 + c] = v;
  }
}

__global__ __launch_bounds__(64) void aug_stats_kernel(const int32_t* __restrict__ blk_start,
                                                       const double* __restrict__ partial, int nblk,
                                                       double* __restrict__ stats) {
  const int b = blockIdx.x, c = threadIdx.x;
  if (c >= 6) return;
  const int g0 = min(blk_start[b], nblk), g1 = min(blk_start[b + 1], nblk);
  double v = c < 3 ? INFINITY : -INFINITY;  // a frame without rows: min = +inf, max = -inf
  for (int g = g0; g < g1; ++g) v = c < 3 ? nan_min(v, partial[(size_t)g * 6 + c]) : nan_max(v, partial[(size_t)g * 6 + c]);
  stats[b * 6 + c] = v;
}

__global__ __launch_bounds__(AUG_BLOCK) void quantise_kernel(const double* __restrict__ points,
                                                             const int32_t* __restrict__ offsets, int N, int B,
                                                             const double* __restrict__ stats, int origin,
                                                             double size, int32_t* __restrict__ coords,
                                                             float* __restrict__ shifted, double* __restrict__ shift_out) {
  const int i = blockIdx.x * AUG_BLOCK + threadIdx.x;
  if (shift_out && i < B * 3) {
    const int b = i / 3, c = i % 3;
    const double mn = stats[b * 6 + c], mx = stats[b * 6 + 3 + c];
    shift_out[i] = origin == SV_ORIGIN_CENTER ? (mx + mn) / 2.0 : (origin == SV_ORIGIN_BASE ? mn : 0.0);
  }
  if (i >= N) return;
  int lo = 0, hi = B;  // largest b with offsets[b] <= i: the frame that owns row i when offsets is non-decreasing
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= i) lo = mid; else hi = mid;
  }
  const int b = lo;
  int qv[3];
  float f[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double v = points[(size_t)i * 3 + c];
    if (origin == SV_ORIGIN_CENTER) v = v - (stats[b * 6 + 3 + c] + stats[b * 6 + c]) / 2.0;
    else if (origin == SV_ORIGIN_BASE) v = v - stats[b * 6 + c];
    f[c] = (float)v;
    const double fl = floor(v / size);
    // NaN, inf and anything outside int32 become INT32_MIN: outside the key range, so sv_voxelize reports the row
    qv[c] = (fl >= -2147483648.0 && fl <= 2147483647.0) ? (int)fl : INT32_MIN;
  }
  ((int4*)coords)[i] = make_int4(b, qv[0], qv[1], qv[2]);
  if (shifted) {
    shifted[(size_t)i * 3] = f[0];
    shifted[(size_t)i * 3 + 1] = f[1];
    shifted[(size_t)i * 3 + 2] = f[2];
  }
}

static inline size_t aug_blocks(int64_t N, int B) { return (size_t)((N + AUG_BLOCK - 1) / AUG_BLOCK) + (size_t)B; }

// total floats of F fields, or -1 when a shape is outside [3, FIELD_MAX_DIM]
static long long field_floats(const int32_t* dims, int F) {
  long long total = 0;
  for (int f = 0; f < F; ++f) {
    for (int a = 0; a < 3; ++a)
      if (dims[f * 3 + a] < 3 || dims[f * 3 + a] > FIELD_MAX_DIM) return -1;
    total += 3LL * dims[f * 3] * dims[f * 3 + 1] * dims[f * 3 + 2];
  }
  return total;
}

}  // namespace sv

using namespace sv;

extern "C" {

size_t sv_elastic_field_workspace_bytes(const int32_t* dims, int F) {
  if (!dims || F < 1 || F > 2 * SV_MAX_BATCH) return 0;
  const long long total = field_floats(dims, F);
  return total < 0 ? 0 : align_up((size_t)total * sizeof(float), 256) + 256;
}

int sv_elastic_field(const float* raw, const int32_t* dims, int F, void* workspace, size_t workspace_bytes, float* out,
                     sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(F >= 1 && F <= 2 * SV_MAX_BATCH, "need 1 to 2048 fields");
  SV_CHECK_ARG(raw && dims && out && workspace, "null pointer");
  const long long total = field_floats(dims, F);
  SV_CHECK_ARG(total >= 0, "every grid dimension must be in [3, 1024]");
  SV_CHECK_ARG(total < (1LL << 31), "fields too large");
  for (int f = 0; f < F; ++f)
    SV_CHECK_ARG(3LL * dims[f * 3] * dims[f * 3 + 1] * dims[f * 3 + 2] < (1LL << 30), "field too large");
  Workspace ws(workspace, workspace_bytes);
  float* tmp = ws.take<float>((size_t)total);
  if (!ws.ok) {
    set_error("sv_elastic_field: workspace too small");
    return SV_ERR_WORKSPACE;
  }
  for (int pass = 0; pass < 6; ++pass) {  // axes 0, 1, 2, 0, 1, 2: raw -> tmp -> out -> tmp -> out -> tmp -> out
    const float* src = pass == 0 ? raw : (pass % 2 ? tmp : out);
    float* dst = pass % 2 ? out : tmp;
    long long first = 0;
    for (int f0 = 0; f0 < F; f0 += FIELD_CHUNK) {
      FieldTable t;
      const int n = F - f0 < FIELD_CHUNK ? F - f0 : FIELD_CHUNK;
      long long most = 0;
      for (int k = 0; k < FIELD_CHUNK; ++k) {
        const int f = f0 + (k < n ? k : 0);  // unused entries repeat the chunk's first field; no workgroup reads them
        t.bx[k] = dims[f * 3], t.by[k] = dims[f * 3 + 1], t.bz[k] = dims[f * 3 + 2];
        t.first[k] = first;
        if (k < n) {
          const long long floats = 3LL * t.bx[k] * t.by[k] * t.bz[k];
          first += floats;
          if (floats > most) most = floats;
        }
      }
      hipLaunchKernelGGL(field_blur_kernel, dim3((unsigned)((most + AUG_BLOCK - 1) / AUG_BLOCK), (unsigned)n),
                         dim3(AUG_BLOCK), 0, stream, src, dst, t, pass % 3);
    }
  }
  SV_LAUNCH_CHECK();
  return SV_OK;
}

size_t sv_augment_points_workspace_bytes(int64_t N, int B) {
  if (N < 0) N = 0;
  if (B < 0) B = 0;
  return align_up((size_t)(B + 1) * 4, 256) + align_up(aug_blocks(N, B) * 6 * sizeof(double), 256) + 256;
}

int sv_augment_points(const void* points, int points_f64, const int32_t* offsets, int64_t N, int B, const double* table,
                      const float* fields, int64_t fields_len, const double* noise, void* workspace,
                      size_t workspace_bytes, double* out, double* stats, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(B >= 1 && B <= SV_MAX_BATCH, "need 1 to 1024 frames");
  SV_CHECK_ARG(N >= 0 && N < (1LL << 29), "need 0 <= N < 2^29 points");
  SV_CHECK_ARG((points || N == 0) && (out || N == 0) && offsets && table && stats && workspace, "null pointer");
  SV_CHECK_ARG(fields_len >= 0 && (fields || fields_len == 0), "fields_len without fields");
  Workspace ws(workspace, workspace_bytes);
  const size_t nblk = aug_blocks(N, B);
  int32_t* blk_start = ws.take<int32_t>((size_t)B + 1);
  double* partial = ws.take<double>(nblk * 6);
  if (!ws.ok) {
    set_error("sv_augment_points: workspace too small");
    return SV_ERR_WORKSPACE;
  }
  const int Ni = (int)N;
  hipLaunchKernelGGL(aug_plan_kernel, dim3(1), dim3(1024), 0, stream, offsets, Ni, B, blk_start);
  if (points_f64)
    hipLaunchKernelGGL(aug_points_kernel<double>, dim3((unsigned)nblk), dim3(AUG_BLOCK), 0, stream, (const double*)points,
                       offsets, Ni, B, table, fields, (long long)fields_len, noise, blk_start, out, partial);
  else
    hipLaunchKernelGGL(aug_points_kernel<float>, dim3((unsigned)nblk), dim3(AUG_BLOCK), 0, stream, (const float*)points,
                       offsets, Ni, B, table, fields, (long long)fields_len, noise, blk_start, out, partial);
  hipLaunchKernelGGL(aug_stats_kernel, dim3(B), dim3(64), 0, stream, blk_start, partial, (int)nblk, stats);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

int sv_quantise_points(const double* points, const int32_t* offsets, int64_t N, int B, const double* stats, int origin,
                       double quantization_size, int32_t* coords, float* shifted, double* shift_out,
                       sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(B >= 1 && B <= SV_MAX_BATCH, "need 1 to 1024 frames");
  SV_CHECK_ARG(N >= 0 && N < (1LL << 29), "need 0 <= N < 2^29 points");
  SV_CHECK_ARG(origin >= SV_ORIGIN_NONE && origin <= SV_ORIGIN_BASE, "bad origin mode");
  SV_CHECK_ARG(quantization_size > 0.0 && quantization_size < INFINITY, "quantization_size must be positive and finite");
  SV_CHECK_ARG((points || N == 0) && (coords || N == 0) && offsets, "null pointer");
  SV_CHECK_ARG(stats || (origin == SV_ORIGIN_NONE && !shift_out), "null pointer (stats)");
  const int64_t threads = N > (int64_t)B * 3 ? N : (int64_t)B * 3;
  hipLaunchKernelGGL(quantise_kernel, dim3((unsigned)((threads + AUG_BLOCK - 1) / AUG_BLOCK)), dim3(AUG_BLOCK), 0, stream,
                     points, offsets, (int)N, B, stats, origin, quantization_size, coords, shifted, shift_out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

}  // extern "C"
