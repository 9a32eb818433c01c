// Field front end of the ResFieldNets (model/backbone/resnet.py:165-193 of the reference): ME.MinkowskiSinusoidal on its
// own (sv_sinusoidal) and the eval() form of one whole field network - Sinusoidal -> BN -> ReLU -> Linear -> BN -> ReLU ->
// per-voxel mean - as ONE kernel that reads every point once and writes [V, C] (sv_field_stage).  Vector ALU only: the work
// is 100 fp32 FMAs and one fp64 sine per (point, channel), far below what the memory system delivers.
//
// Arithmetic shared by both entries, per (point p, channel n):
//   a = 0;  a = fmaf(x[p][k], kernel[k][n], a) for k ascending;  a = a + bias[n];  s = (float)sin((double)a);  y = coef[n] * s
// sv_field_stage goes on with  h = relu(fmaf(y, scale1[n], shift1[n])),
//   b = 0;  b = fmaf(h[c], W[c][n], b) for c ascending;  (b = b + lin_bias[n]);  z = relu(fmaf(b, scale2[n], shift2[n]))
// and sums z over the voxel's points in ascending original index (sv_voxel_reduce's order), one division by the count.
// relu(v) = v < 0 ? 0 : v (NaN stays NaN).  No float atomics: repeated calls give the same bits.
#include <atomic>

#include "sv_common.h"

namespace sv {

// ------------------------------------------------------------------------------------------------
// sv_sinusoidal: one thread per output element; the lanes of a wavefront run along the channels (coalesced kernel rows and
// stores), the point's row is read through the cache
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sin_once(float a) {
  // the double sine is within 1 ulp(double) of the exact one for every argument (full-range reduction): rounding it to
  // fp32 gives the correctly rounded fp32 sine except in 2^-29 of the cases, where it is the other neighbour
  return (float)sin((double)a);
}

__global__ __launch_bounds__(256) void sinusoidal_kernel(const float* __restrict__ x, int64_t ld, int Cin, int64_t N,
                                                          const float* __restrict__ kernel, const float* __restrict__ bias,
                                                          const float* __restrict__ coef, int Cout, float* __restrict__ out,
                                                          int64_t out_ld) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= N * Cout) return;
  const int64_t p = t / Cout;
  const int n = (int)(t - p * Cout);
  const float* row = x + p * ld;
  float a = 0.0f;
  for (int k = 0; k < Cin; ++k) a = fmaf(row[k], kernel[(int64_t)k * Cout + n], a);
  a = a + bias[n];
  out[p * out_ld + n] = coef[n] * sin_once(a);
}

// ------------------------------------------------------------------------------------------------
// sv_field_stage
//
// A workgroup (256 threads) owns the voxels whose first sorted position lies in [b * FS_RANGE, (b + 1) * FS_RANGE) and
// walks their positions, first to last, in tiles of FS_TILE points; a voxel that is longer than a tile (or than the range)
// is carried from tile to tile by that workgroup in LDS, so every voxel is ONE sequential sum whatever its neighbours are.
// Per tile:
//   0  p = order[j], the voxel bounds of the tile and the input rows [G[inverse[p]], F[p]] go to LDS, transposed (xT[k][pt])
//   1  a[pt][n] = sum_k xT[k][pt] K[k][n]: each thread a block of PP points x 4 channels, both operands as wide LDS reads
//   1b bias, sine, coef, BN 1, ReLU on the tile's elements in place (hT[c][pt])
//   2  b[pt][n] = sum_c hT[c][pt] W[c][n], same blocks; bias, BN 2, ReLU -> z[pt][n]
//   3  thread (group g, channel n): the voxels g, g + G, ... of the tile, each summed over its points in order
// ------------------------------------------------------------------------------------------------
constexpr int FS_TILE = 64;
constexpr int FS_RANGE = 256;
constexpr int FS_TS = FS_TILE + 4;  // row stride of the transposed tiles (16-byte rows, off the 64-bank period)
constexpr int FS_MAX_CIN = 128;

struct FieldStageParams {
  const float* F;
  int64_t f_ld;
  int Cf;
  const float* G;
  int64_t g_ld;
  int Cg;
  const int64_t* inverse;
  const float *kernel, *bias, *coef, *scale1, *shift1, *W, *lin_bias, *scale2, *shift2;
  const int32_t *order, *seg_start;
  int64_t V;
  float* out;
  int64_t out_ld;
};

__host__ __device__ constexpr int fs_cin4(int Cin) { return (Cin + 3) / 4 * 4; }
// LDS floats: K[Cin4][C], W[C][C], xT[Cin4][TS], hT[C][TS], z[TILE][C], carry[2][C], 7 parameter rows [C], then the ints
// row[TILE], grow[TILE], segs[TILE + 1] (+ 3 to keep 16 bytes)
static size_t fs_lds_bytes(int Cin, int C) {
  const size_t c4 = fs_cin4(Cin);
  return 4 * (c4 * C + (size_t)C * C + c4 * FS_TS + (size_t)C * FS_TS + (size_t)FS_TILE * C + 2 * C + 7 * C + 3 * FS_TILE + 4);
}

// first v in [0, V] with seg_start[v] >= j (seg_start ascending, seg_start[V] = N >= j)
__device__ __forceinline__ int64_t fs_lower_bound(const int32_t* __restrict__ seg_start, int64_t V, int64_t j) {
  int64_t lo = 0, hi = V;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (seg_start[mid] < j)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// acc[i][c] += sum_k xT[k][p0 + i] * Wl[k][n0 + c], k ascending; points past npts are skipped (uniform per point group)
template <int C, int PP>
__device__ __forceinline__ void fs_block(const float* __restrict__ xT, const float* __restrict__ Wl, int Kdim, int p0, int n0,
                                         float (&acc)[PP][4]) {
#pragma unroll 4
  for (int k = 0; k < Kdim; ++k) {
    const float4 w = *(const float4*)(Wl + k * C + n0);
    float xv[PP];
    if constexpr (PP == 4) {
      const float4 x = *(const float4*)(xT + k * FS_TS + p0);
      xv[0] = x.x, xv[1] = x.y, xv[2] = x.z, xv[3] = x.w;
    } else {
      const float2 x = *(const float2*)(xT + k * FS_TS + p0);
      xv[0] = x.x, xv[1] = x.y;
    }
#pragma unroll
    for (int i = 0; i < PP; ++i) {
      acc[i][0] = fmaf(xv[i], w.x, acc[i][0]);
      acc[i][1] = fmaf(xv[i], w.y, acc[i][1]);
      acc[i][2] = fmaf(xv[i], w.z, acc[i][2]);
      acc[i][3] = fmaf(xv[i], w.w, acc[i][3]);
    }
  }
}

template <int C>
__global__ __launch_bounds__(256) void field_stage_kernel(const FieldStageParams p) {
  constexpr int CG = C / 4;             // channel groups of 4
  constexpr int PG = 256 / CG;          // point groups
  constexpr int PP = FS_TILE / PG;      // points per thread: 4 (C = 64) or 2 (C = 32)
  constexpr int G = 256 / C;            // voxel groups of the segmented sum
  static_assert(PP == 4 || PP == 2, "tile shape");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int Cin = p.Cg + p.Cf, Cin4 = fs_cin4(Cin);
  float* Kl = lds;
  float* Wl = Kl + Cin4 * C;
  float* xT = Wl + C * C;
  float* hT = xT + Cin4 * FS_TS;
  float* z = hT + C * FS_TS;
  float* carry = z + FS_TILE * C;
  float* par = carry + 2 * C;  // bias, coef, scale1, shift1, lin_bias, scale2, shift2
  int32_t* row = (int32_t*)(par + 7 * C);
  int32_t* grow = row + FS_TILE;
  int32_t* segs = grow + FS_TILE;

  const int64_t r0 = (int64_t)blockIdx.x * FS_RANGE;
  const int64_t vbeg = fs_lower_bound(p.seg_start, p.V, r0);
  const int64_t vend = fs_lower_bound(p.seg_start, p.V, r0 + FS_RANGE);
  if (vbeg >= vend) return;  // uniform: every position of the range belongs to a voxel that began earlier
  const int64_t jbeg = p.seg_start[vbeg], jend = p.seg_start[vend];

  // weights and parameters, once per workgroup; rows Cin..Cin4 of K (and of xT) are zero: fmaf(0, 0, a) = a
  for (int i = tid; i < Cin4 * C; i += 256) Kl[i] = i < Cin * C ? p.kernel[i] : 0.0f;
  for (int i = tid; i < C * C; i += 256) Wl[i] = p.W[i];
  for (int i = tid; i < (Cin4 - Cin) * FS_TS; i += 256) xT[Cin * FS_TS + i] = 0.0f;
  if (tid < C) {
    par[tid] = p.bias[tid];
    par[C + tid] = p.coef[tid];
    par[2 * C + tid] = p.scale1[tid];
    par[3 * C + tid] = p.shift1[tid];
    par[4 * C + tid] = p.lin_bias ? p.lin_bias[tid] : 0.0f;
    par[5 * C + tid] = p.scale2[tid];
    par[6 * C + tid] = p.shift2[tid];
  }
  const bool has_lin_bias = p.lin_bias != nullptr;

  const int cg = tid % CG, pg = tid / CG;
  const int n0 = 4 * cg, p0 = PP * pg;
  const int sum_n = tid % C, sum_g = tid / C;
  int64_t vcur = vbeg;  // the voxel that holds position j0
  int buf = 0;
  for (int64_t j0 = jbeg; j0 < jend; j0 += FS_TILE, buf ^= 1) {
    const int npts = (int)(jend - j0 < FS_TILE ? jend - j0 : FS_TILE);
    const int64_t j1 = j0 + npts;
    __syncthreads();  // the previous tile's reads of row / segs / xT / z are over
    if (tid < FS_TILE) {
      int32_t r = 0, g = 0;
      if (tid < npts) {
        r = p.order[j0 + tid];
        if (p.Cg > 0) g = (int32_t)p.inverse[r];
      }
      row[tid] = r;
      grow[tid] = g;
    }
    if (tid <= FS_TILE) {
      const int64_t v = vcur + tid < vend ? vcur + tid : vend;
      segs[tid] = p.seg_start[v];
    }
    __syncthreads();
    // 0: gather, lanes along a row's channels
    for (int i = tid; i < FS_TILE * Cin; i += 256) {
      const int pt = i / Cin, k = i - pt * Cin;
      float v = 0.0f;
      if (pt < npts)
        v = k < p.Cg ? p.G[(int64_t)grow[pt] * p.g_ld + k] : p.F[(int64_t)row[pt] * p.f_ld + (k - p.Cg)];
      xT[k * FS_TS + pt] = v;
    }
    __syncthreads();
    // 1: the sinusoidal layer's argument
    const bool live = p0 < npts;
    {
      float acc[PP][4];
#pragma unroll
      for (int i = 0; i < PP; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.0f;
      if (live) fs_block<C, PP>(xT, Kl, Cin4, p0, n0, acc);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if constexpr (PP == 4)
          *(float4*)(hT + (n0 + c) * FS_TS + p0) = make_float4(acc[0][c], acc[1][c], acc[2][c], acc[3][c]);
        else
          *(float2*)(hT + (n0 + c) * FS_TS + p0) = make_float2(acc[0][c], acc[1][c]);
      }
    }
    __syncthreads();
    // 1b: bias, sine, coef, BN 1, ReLU in place
#pragma unroll 1
    for (int i = tid; i < C * FS_TILE; i += 256) {
      const int c = i / FS_TILE, pt = i % FS_TILE;
      if (pt >= npts) continue;
      const float a = hT[c * FS_TS + pt] + par[c];
      const float y = par[C + c] * sin_once(a);
      const float h = fmaf(y, par[2 * C + c], par[3 * C + c]);
      hT[c * FS_TS + pt] = h < 0.0f ? 0.0f : h;
    }
    __syncthreads();
    // 2: linear, BN 2, ReLU
    if (live) {
      float acc[PP][4];
#pragma unroll
      for (int i = 0; i < PP; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.0f;
      fs_block<C, PP>(hT, Wl, C, p0, n0, acc);
#pragma unroll
      for (int i = 0; i < PP; ++i) {
        float o[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float b = acc[i][c];
          if (has_lin_bias) b = b + par[4 * C + n0 + c];
          b = fmaf(b, par[5 * C + n0 + c], par[6 * C + n0 + c]);
          o[c] = b < 0.0f ? 0.0f : b;
        }
        *(float4*)(z + (p0 + i) * C + n0) = make_float4(o[0], o[1], o[2], o[3]);
      }
    }
    __syncthreads();
    // 3: the voxels of the tile, each one sequential sum; voxel vcur + i overlaps the tile iff segs[i] < j1
    for (int i = sum_g; i < FS_TILE; i += G) {
      if (vcur + i >= vend) break;
      const int64_t s = segs[i], e = segs[i + 1];
      if (s >= j1) break;
      const int a0 = (int)(s > j0 ? s - j0 : 0), a1 = (int)(e < j1 ? e - j0 : npts);
      float acc;
      int a = a0;
      if (s < j0)
        acc = carry[buf * C + sum_n];  // begun in an earlier tile
      else
        acc = z[(a++) * C + sum_n];
      for (; a < a1; ++a) acc += z[a * C + sum_n];
      if (e <= j1)
        p.out[(vcur + i) * p.out_ld + sum_n] = acc / (float)(e - s);
      else
        carry[(buf ^ 1) * C + sum_n] = acc;  // only the tile's last voxel: read back by the next tile's first
    }
    // the voxel that holds position j1: voxels are never empty, so it is among vcur .. vcur + TILE
    {
      const int lane = tid & 63;
      const bool done = vcur + lane + 1 <= vend && (int64_t)segs[lane + 1] <= j1;  // FS_TILE = 64 = the wavefront
      vcur += __popcll(__ballot(done));
    }
  }
}

}  // namespace sv

using namespace sv;

// The stage kernels take more than 64 KiB of dynamic LDS from 20 input channels on (C = 64): the limit is raised to the
// largest size a supported shape needs, once per kernel and device (hipFuncSetAttribute acts on the current device).
static int fs_allow_lds(const void* fn, int C) {
  static std::atomic<bool> done[2][16];
  int dev = 0;
  SV_HIP(hipGetDevice(&dev));
  std::atomic<bool>* flag = dev >= 0 && dev < 16 ? &done[C == 64][dev] : nullptr;
  if (flag && flag->load(std::memory_order_acquire)) return SV_OK;
  SV_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fs_lds_bytes(FS_MAX_CIN, C)));
  if (flag) flag->store(true, std::memory_order_release);
  return SV_OK;
}

extern "C" {

int sv_sinusoidal(const float* x, int64_t ld, int Cin, int64_t N, const float* kernel, const float* bias, const float* coef,
                  int Cout, float* out, int64_t out_ld, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(Cin >= 1 && Cout >= 1 && N >= 0 && ld >= Cin && out_ld >= Cout, "bad shape");
  SV_CHECK_ARG(N <= ((1ll << 31) - 1) * 256 / Cout, "too many elements for one launch");
  if (N == 0) return SV_OK;
  SV_CHECK_ARG(x && kernel && bias && coef && out, "null pointer");
  const int64_t total = N * Cout;
  hipLaunchKernelGGL(sinusoidal_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x, ld, Cin, N, kernel, bias,
                     coef, Cout, out, out_ld);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

int sv_field_stage(const float* F, int64_t f_ld, int Cf, int64_t N, const float* G, int64_t g_ld, int Cg, const int64_t* inverse,
                   const float* kernel, const float* bias, const float* coef, const float* scale1, const float* shift1,
                   const float* W, const float* lin_bias, const float* scale2, const float* shift2, int C,
                   const int32_t* order, const int32_t* seg_start, int64_t V, float* out, int64_t out_ld, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(Cf >= 1 && Cg >= 0 && C >= 1 && N >= 0 && V >= 0 && V <= N, "bad shape");
  SV_CHECK_ARG(f_ld >= Cf && out_ld >= C && (Cg == 0 || g_ld >= Cg), "bad shape (row stride below the row length)");
  SV_CHECK_ARG(N < (1ll << 31) - FS_RANGE, "row count out of range");
  if ((C != 32 && C != 64) || (int64_t)Cg + Cf > FS_MAX_CIN) {
    set_error("%s: C = %d with %d + %d inputs is outside the fused kernel (C in {32, 64}, Cg + Cf <= %d)", __func__, C, Cg, Cf,
              FS_MAX_CIN);
    return SV_ERR_UNSUPPORTED;
  }
  SV_CHECK_ARG((N == 0) == (V == 0), "bad shape (points without voxels or voxels without points)");
  if (N == 0) return SV_OK;
  SV_CHECK_ARG(F && kernel && bias && coef && scale1 && shift1 && W && scale2 && shift2 && order && seg_start && out,
               "null pointer");
  SV_CHECK_ARG(Cg == 0 || (G && inverse), "null pointer (voxel features need G and inverse)");
  FieldStageParams p{F, f_ld, Cf, G, g_ld, Cg, inverse, kernel, bias, coef, scale1, shift1, W, lin_bias, scale2, shift2,
                     order, seg_start, V, out, out_ld};
  const size_t lds = fs_lds_bytes(Cg + Cf, C);
  const void* fn = C == 64 ? (const void*)field_stage_kernel<64> : (const void*)field_stage_kernel<32>;
  if (lds > 64 * 1024) {
    const int rc = fs_allow_lds(fn, C);
    if (rc) return rc;
  }
  const unsigned nb = (unsigned)((N + FS_RANGE - 1) / FS_RANGE);
  if (C == 64)
    hipLaunchKernelGGL(field_stage_kernel<64>, dim3(nb), dim3(256), lds, stream, p);
  else
    hipLaunchKernelGGL(field_stage_kernel<32>, dim3(nb), dim3(256), lds, stream, p);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

}  // extern "C"
