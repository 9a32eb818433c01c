// N3f: a depth image and a colour image -> a registered, coloured, unorganised cloud on the device (the reference does
// this on the host, scripts/ycb_generate_point_cloud.py:127-274 filterDiscontinuities, registerDepthMap and
// registeredDepthMapToPointCloud, the last two as Python loops over every pixel).  Definitions in include/sv_hip.h; all
// arithmetic is float64 in the order written there (the library is built with -ffp-contract=off), and every output
// equals a numpy restatement bit for bit.
//
// Five launches whatever the images hold, no read-back:
//   rgbd_clear_kernel   : the z-buffer (one uint64 per colour pixel) to "nothing landed here"
//   rgbd_project_kernel : one depth pixel per thread in RG_TH x RG_TW tiles.  With the filter on, the tile and a halo of
//                         filter_size / 2 raw values go through LDS and a thread reads its own window from there: only
//                         the own pixel's verdict is needed, so filtered values never travel between threads.  Then
//                         d = value * depth_scale, back-projection, transform, projection and a 64-bit integer
//                         atomicMax / atomicMin on the bit pattern of the positive Z (positive doubles order as their
//                         bits do, so the winner does not depend on the order of arrival).  SV_RGBD_ALIGNED: a plain
//                         store of d at the own pixel.
//   rgbd_count_kernel   : one colour pixel per thread, keep flag -> ballot + popcount -> tile_count[tile]; writes the
//                         registered map when it is asked for
//   compact_scan_kernel : sv_compact.h
//   rgbd_write_kernel   : recomputes the keep flags, ordered write of points, colours and source indices
//
// N3g: lens distortion (plumb-bob and rational).  sv_lens_rays inverts the model once per camera into a table of rays, one
// thread per pixel, 64 fixed-point rounds without an early exit.  The project, count and write kernels exist twice, as
// instantiations of one body: the pinhole ones take the arguments they always took and read no table, the *_lens ones take
// a LensArgs beside them.  There is one host routine (rgbd_run); sv_rgbd_cloud is its call without a lens.
#include "sv_common.h"
#include "sv_compact.h"

namespace sv {

constexpr int RG_TW = 32, RG_TH = 8;  // the filter's tile: RG_TW * RG_TH == CP_THREADS
constexpr int RG_MAX_FILTER = 15;
constexpr int RG_LDS = (RG_TW + RG_MAX_FILTER - 1) * (RG_TH + RG_MAX_FILTER - 1);
constexpr int64_t RG_MAX_PIXELS = 1 << 24;
static_assert(RG_TW * RG_TH == CP_THREADS, "one thread per pixel of a tile");

struct RgbdArgs {
  const uint8_t* depth;
  const uint8_t* color;
  const uint8_t* mask;
  int64_t depth_row, color_row;
  int Hd, Wd, Hc, Wc, tiles_x;
  int f32, fsize, fthresh, aligned, nearest, bgr, has_box;
  double cxd, cyd, inv_fxd, inv_fyd;  // 1.0 / fx and 1.0 / fy are formed on the host: one IEEE division either way
  double fxc, fyc, cxc, cyc, inv_fxc, inv_fyc;
  double H[12], depth_scale;
  double lo[3], hi[3];
};

// the z-buffer's "nothing landed": below every positive double for the maximum, above every one for the minimum
__device__ __forceinline__ unsigned long long z_empty(const RgbdArgs& a) { return a.nearest ? ~0ull : 0ull; }

__device__ __forceinline__ uint32_t load16(const uint8_t* __restrict__ p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

// N3g.  Tables are double[H * W * 2 + 1] (sv_lens_rays); r2_max is their last element.
struct LensArgs {
  const double* depth_rays;  // stage 2 back-projection, or nullptr = pinhole
  const double* color_rays;  // stage 3 back-projection and the fold-back bound, or nullptr = pinhole
  int has_dist;              // stage 2 projects through the forward model with D
  double D[8];               // k1, k2, p1, p2, k3, k4, k5, k6
};

// the forward model F of include/sv_hip.h N3g: every operation rounded on its own, in the order written there
__device__ __forceinline__ void lens_tangential(const double* D, double a, double b, double r2, double& dx,
                                                double& dy) {
  dx = (2.0 * D[2]) * (a * b) + D[3] * (r2 + 2.0 * (a * a));
  dy = D[2] * (r2 + 2.0 * (b * b)) + (2.0 * D[3]) * (a * b);
}

__device__ __forceinline__ void lens_forward(const double* D, double a, double b, double& xd, double& yd) {
  const double r2 = a * a + b * b;
  const double num = 1.0 + ((D[4] * r2 + D[1]) * r2 + D[0]) * r2;
  const double den = 1.0 + ((D[7] * r2 + D[6]) * r2 + D[5]) * r2;
  const double c = num / den;
  double dx, dy;
  lens_tangential(D, a, b, r2, dx, dy);
  xd = a * c + dx;
  yd = b * c + dy;
}

struct LensCam {
  double fx, fy, cx, cy, inv_fx, inv_fy, D[8];
  int H, W;
};

constexpr int LENS_ROUNDS = 64;

__global__ __launch_bounds__(CP_THREADS) void lens_rays_kernel(LensCam c, double* __restrict__ rays) {
  __shared__ double wave_max[CP_WAVES];
  const int n = c.H * c.W;
  const int j = blockIdx.x * CP_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  double r2_own = 0.0;  // an invalid pixel and a thread beyond the image leave the maximum alone
  if (j < n) {
    const int v = j / c.W, u = j - v * c.W;
    const double x0 = ((double)u - c.cx) * c.inv_fx, y0 = ((double)v - c.cy) * c.inv_fy;
    double x = x0, y = y0;
    for (int k = 0; k < LENS_ROUNDS; ++k) {
      const double r2 = x * x + y * y;
      const double ic = (1.0 + ((c.D[7] * r2 + c.D[6]) * r2 + c.D[5]) * r2) / (1.0 + ((c.D[4] * r2 + c.D[1]) * r2 + c.D[0]) * r2);
      double dx, dy;
      lens_tangential(c.D, x, y, r2, dx, dy);
      x = (x0 - dx) * ic;
      y = (y0 - dy) * ic;
    }
    double xd, yd;
    lens_forward(c.D, x, y, xd, yd);
    // false for a NaN on either side
    const bool valid = fabs((c.fx * xd + c.cx) - (double)u) <= 1e-6 && fabs((c.fy * yd + c.cy) - (double)v) <= 1e-6;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    rays[2 * (int64_t)j] = valid ? x : nan;  // j < H * W: inside the table's first 2 * H * W entries
    rays[2 * (int64_t)j + 1] = valid ? y : nan;
    if (valid) r2_own = x * x + y * y;
  }
  // a maximum does not depend on the order: wave by shuffles, workgroup through LDS, then the z-buffer's idiom, a 64-bit
  // integer atomic max on the bit pattern (r2 >= +0, and non-negative doubles order as their bits do)
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double other = __shfl_xor(r2_own, d);
    r2_own = other > r2_own ? other : r2_own;
  }
  if (lane == 0) wave_max[wid] = r2_own;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = wave_max[0];
#pragma unroll
    for (int k = 1; k < CP_WAVES; ++k) m = wave_max[k] > m ? wave_max[k] : m;
    atomicMax((unsigned long long*)(rays + 2 * (int64_t)n), (unsigned long long)__double_as_longlong(m));
  }
}

__global__ __launch_bounds__(CP_THREADS) void rgbd_clear_kernel(unsigned long long* __restrict__ zbuf, int n,
                                                                 unsigned long long value) {
  const int j = blockIdx.x * CP_THREADS + threadIdx.x;
  if (j < n) zbuf[j] = value;
}

template <bool LENS>
__device__ __forceinline__ void rgbd_project(const RgbdArgs& a, const LensArgs* l, unsigned long long* __restrict__ zbuf,
                                             uint16_t* tile) {
  const int o = a.fsize >> 1;  // 0 when the filter is off
  const int tx = threadIdx.x % RG_TW, ty = threadIdx.x / RG_TW;
  const int by = blockIdx.x / a.tiles_x, bx = blockIdx.x - by * a.tiles_x;
  const int u0 = bx * RG_TW, v0 = by * RG_TH;
  const int tw = RG_TW + 2 * o;
  if (o > 0) {  // the same for every thread of the launch
    const int cells = tw * (RG_TH + 2 * o);
    for (int k = threadIdx.x; k < cells; k += CP_THREADS) {
      const int r = k / tw, c = k - r * tw;
      const int v = v0 - o + r, u = u0 - o + c;
      uint32_t raw = 0;  // outside the image: never inside the window of a pixel the filter may change
      if (v >= 0 && v < a.Hd && u >= 0 && u < a.Wd) raw = load16(a.depth + (int64_t)v * a.depth_row + 2 * (int64_t)u);
      tile[k] = (uint16_t)raw;
    }
    __syncthreads();
  }
  const int u = u0 + tx, v = v0 + ty;
  if (u >= a.Wd || v >= a.Hd) return;
  double value;
  if (a.f32) {
    const uint8_t* p = a.depth + (int64_t)v * a.depth_row + 4 * (int64_t)u;
    const uint32_t bits = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    // finite and > 0, decided on the bits: sign clear, exponent not all ones, not +0 (a denormal is valid)
    const bool valid = (bits >> 31) == 0 && (bits & 0x7f800000u) != 0x7f800000u && bits != 0;
    value = valid ? (double)__uint_as_float(bits) : 0.0;
  } else if (o > 0) {
    int mid = tile[(ty + o) * tw + tx + o];
    if (v >= o && v < a.Hd - o && u >= o && u < a.Wd - o) {
      int mn = 65535, mx = 0;
      for (int r = 0; r < a.fsize; ++r) {
        const uint16_t* row = tile + (ty + r) * tw + tx;
        for (int c = 0; c < a.fsize; ++c) {
          const int w = row[c];
          mn = w < mn ? w : mn;
          mx = w > mx ? w : mx;
        }
      }
      const int lo = mid - mn, hi = mx - mid;
      if ((lo > hi ? lo : hi) > a.fthresh) mid = 0;
    }
    value = (double)mid;
  } else {
    value = (double)load16(a.depth + (int64_t)v * a.depth_row + 2 * (int64_t)u);
  }
  const double d = value * a.depth_scale;
  if (a.aligned) {  // Hd x Wd == Hc x Wc
    zbuf[(int64_t)v * a.Wc + u] = (unsigned long long)__double_as_longlong(d);
    return;
  }
  if (d == 0.0) return;
  double x, y;
  if (LENS && l->depth_rays) {  // a NaN ray makes X, Y and Z NaN: dropped below
    const double* ray = l->depth_rays + 2 * ((int64_t)v * a.Wd + u);  // v < Hd, u < Wd: inside the depth table
    x = ray[0] * d;
    y = ray[1] * d;
  } else {
    x = (((double)u - a.cxd) * d) * a.inv_fxd;
    y = (((double)v - a.cyd) * d) * a.inv_fyd;
  }
  const double z = d;
  const double X = ((a.H[0] * x + a.H[1] * y) + a.H[2] * z) + a.H[3];
  const double Y = ((a.H[4] * x + a.H[5] * y) + a.H[6] * z) + a.H[7];
  const double Z = ((a.H[8] * x + a.H[9] * y) + a.H[10] * z) + a.H[11];
  const double iz = 1.0 / Z;
  double uu, vv;
  if (LENS && l->has_dist) {
    const double na = X * iz, nb = Y * iz;
    // a rational model is not monotonic: beyond the table's largest valid radius a point may fold back into the image.
    // The host refuses has_dist without color_rays; false for a NaN.
    if (!(na * na + nb * nb <= l->color_rays[2 * (int64_t)a.Hc * a.Wc])) return;
    double xd, yd;
    lens_forward(l->D, na, nb, xd, yd);
    uu = a.fxc * xd + a.cxc;
    vv = a.fyc * yd + a.cyc;
  } else {
    uu = (a.fxc * X) * iz + a.cxc;
    vv = (a.fyc * Y) * iz + a.cyc;
  }
  const double ut = trunc(uu + 0.5), vt = trunc(vv + 0.5);
  // every comparison is false for a NaN; an infinite ut or vt fails its upper bound
  if (!(ut >= 0.0 && ut < (double)a.Wc && vt >= 0.0 && vt < (double)a.Hc)) return;
  if (!(Z > 0.0 && Z < __longlong_as_double(0x7ff0000000000000ll))) return;
  // (int)ut < Wc and (int)vt < Hc: the slot lies inside the Hc * Wc entries of the z-buffer
  unsigned long long* slot = zbuf + ((int64_t)(int)vt * a.Wc + (int)ut);
  const unsigned long long zb = (unsigned long long)__double_as_longlong(Z);
  if (a.nearest)
    atomicMin(slot, zb);
  else
    atomicMax(slot, zb);
}

__global__ __launch_bounds__(CP_THREADS) void rgbd_project_kernel(RgbdArgs a, unsigned long long* __restrict__ zbuf) {
  __shared__ uint16_t tile[RG_LDS];
  rgbd_project<false>(a, nullptr, zbuf, tile);
}

__global__ __launch_bounds__(CP_THREADS) void rgbd_project_lens_kernel(RgbdArgs a, LensArgs l,
                                                                        unsigned long long* __restrict__ zbuf) {
  __shared__ uint16_t tile[RG_LDS];
  rgbd_project<true>(a, &l, zbuf, tile);
}

// registered depth of colour pixel j, its point as float64 and as float32 bits, and its keep flag
template <bool LENS>
__device__ __forceinline__ bool rgbd_point(const RgbdArgs& a, const LensArgs* l, const unsigned long long* __restrict__ zbuf,
                                           int j, double& r, double p[3], uint32_t q[3]) {
  const unsigned long long zb = zbuf[j];
  r = (!a.aligned && zb == z_empty(a)) ? 0.0 : __longlong_as_double((long long)zb);
  const int v = j / a.Wc, u = j - v * a.Wc;
  bool keep = r > 0.0;  // false for a NaN
  if (a.mask) keep = keep && a.mask[j] == 0;
  if (LENS && l->color_rays) {
    const double rx = l->color_rays[2 * (int64_t)j], ry = l->color_rays[2 * (int64_t)j + 1];  // j < Hc * Wc
    keep = keep && rx == rx;  // an invalid pixel holds (NaN, NaN)
    p[0] = rx * r;
    p[1] = ry * r;
  } else {
    p[0] = (((double)u - a.cxc) * r) * a.inv_fxc;
    p[1] = (((double)v - a.cyc) * r) * a.inv_fyc;
  }
  p[2] = r;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float f = (float)p[c];  // round to nearest even; beyond FLT_MAX -> inf
    q[c] = __float_as_uint(f);
    if (a.has_box) {
      const double w = (double)f;
      keep = keep && (a.lo[c] < w) && (w < a.hi[c]);  // strict; false for NaN
    }
  }
  return keep;
}

template <bool LENS>
__device__ __forceinline__ void rgbd_count(const RgbdArgs& a, const LensArgs* l, const unsigned long long* __restrict__ zbuf,
                                           double* __restrict__ registered, int32_t* __restrict__ tile_count, int* wave_cnt) {
  const int j = blockIdx.x * CP_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  bool keep = false;
  if (j < a.Hc * a.Wc) {
    double r, p[3];
    uint32_t q[3];
    keep = rgbd_point<LENS>(a, l, zbuf, j, r, p, q);
    if (registered) registered[j] = r;
  }
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wave_cnt[wid] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < CP_WAVES; ++k) s += wave_cnt[k];
    tile_count[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(CP_THREADS) void rgbd_count_kernel(RgbdArgs a, const unsigned long long* __restrict__ zbuf,
                                                                 double* __restrict__ registered,
                                                                 int32_t* __restrict__ tile_count) {
  __shared__ int wave_cnt[CP_WAVES];
  rgbd_count<false>(a, nullptr, zbuf, registered, tile_count, wave_cnt);
}

__global__ __launch_bounds__(CP_THREADS) void rgbd_count_lens_kernel(RgbdArgs a, LensArgs l,
                                                                      const unsigned long long* __restrict__ zbuf,
                                                                      double* __restrict__ registered,
                                                                      int32_t* __restrict__ tile_count) {
  __shared__ int wave_cnt[CP_WAVES];
  rgbd_count<true>(a, &l, zbuf, registered, tile_count, wave_cnt);
}

template <bool LENS>
__device__ __forceinline__ void rgbd_write(const RgbdArgs& a, const LensArgs* l, const unsigned long long* __restrict__ zbuf,
                                           const int32_t* __restrict__ tile_base, const float* __restrict__ lut,
                                           uint32_t* __restrict__ points, double* __restrict__ points64,
                                           float* __restrict__ rgb, int32_t* __restrict__ src, int* wave_cnt) {
  const int j = blockIdx.x * CP_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  bool keep = false;
  double r, p[3] = {0.0, 0.0, 0.0};
  uint32_t q[3] = {0, 0, 0};
  if (j < a.Hc * a.Wc) keep = rgbd_point<LENS>(a, l, zbuf, j, r, p, q);
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wave_cnt[wid] = __popcll(m);
  __syncthreads();
  if (!keep) return;
  int before = 0;
#pragma unroll
  for (int k = 0; k < CP_WAVES; ++k) before += k < wid ? wave_cnt[k] : 0;
  // row < the number kept <= Hc * Wc: inside the caller's [Hc * Wc][3] arrays
  const int64_t row = (int64_t)tile_base[blockIdx.x] + before + __popcll(m & ((1ull << lane) - 1ull));
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    points[row * 3 + c] = q[c];
    if (points64) points64[row * 3 + c] = p[c];
  }
  if (src) src[row] = j;
  if (a.color) {
    const int v = j / a.Wc, u = j - v * a.Wc;
    const uint8_t* px = a.color + (int64_t)v * a.color_row + 3 * (int64_t)u;
    const int c0 = px[0], g = px[1], c2 = px[2];
    const int red = a.bgr ? c2 : c0, blue = a.bgr ? c0 : c2;
    rgb[row * 3] = lut ? lut[red] : (float)red;
    rgb[row * 3 + 1] = lut ? lut[g] : (float)g;
    rgb[row * 3 + 2] = lut ? lut[blue] : (float)blue;
  }
}

__global__ __launch_bounds__(CP_THREADS) void rgbd_write_kernel(RgbdArgs a, const unsigned long long* __restrict__ zbuf,
                                                                 const int32_t* __restrict__ tile_base,
                                                                 const float* __restrict__ lut, uint32_t* __restrict__ points,
                                                                 double* __restrict__ points64, float* __restrict__ rgb,
                                                                 int32_t* __restrict__ src) {
  __shared__ int wave_cnt[CP_WAVES];
  rgbd_write<false>(a, nullptr, zbuf, tile_base, lut, points, points64, rgb, src, wave_cnt);
}

__global__ __launch_bounds__(CP_THREADS) void rgbd_write_lens_kernel(RgbdArgs a, LensArgs l,
                                                                      const unsigned long long* __restrict__ zbuf,
                                                                      const int32_t* __restrict__ tile_base,
                                                                      const float* __restrict__ lut, uint32_t* __restrict__ points,
                                                                      double* __restrict__ points64, float* __restrict__ rgb,
                                                                      int32_t* __restrict__ src) {
  __shared__ int wave_cnt[CP_WAVES];
  rgbd_write<true>(a, &l, zbuf, tile_base, lut, points, points64, rgb, src, wave_cnt);
}

static inline bool finite64(double x) { return x - x == 0.0; }

}  // namespace sv

using namespace sv;

extern "C" {

size_t sv_rgbd_cloud_workspace_bytes(int64_t Hd, int64_t Wd, int64_t Hc, int64_t Wc) {
  (void)Hd;
  (void)Wd;
  const size_t n = (Hc > 0 && Wc > 0) ? (size_t)Hc * (size_t)Wc : 0;
  return align_up(n * sizeof(uint64_t), 256) + align_up((n + CP_THREADS - 1) / CP_THREADS * sizeof(int32_t), 256) + 256;
}

}  // extern "C"

// as SV_CHECK_ARG, with the name of the entry point that was called
#define RG_CHECK(cond, msg)                  \
  do {                                       \
    if (!(cond)) {                           \
      sv::set_error("%s: %s", who, msg);     \
      return SV_ERR_INVALID;                 \
    }                                        \
  } while (0)
#define RG_LAUNCH_CHECK()                                                              \
  do {                                                                                 \
    hipError_t e__ = hipGetLastError();                                                \
    if (e__ != hipSuccess) {                                                           \
      sv::set_error("%s: hipGetLastError() -> %s", who, hipGetErrorString(e__));       \
      return SV_ERR_HIP;                                                               \
    }                                                                                  \
  } while (0)

// The one host routine of the RGB-D ingest, called by the entry point `who`, whose name the errors carry.  Without a lens
// (all three of depth_rays, color_rays and color_dist_host NULL: sv_rgbd_cloud) it launches the pinhole kernels, which
// take no LensArgs and read no table; with any of them, the *_lens instantiations.  Five launches either way.
static int rgbd_run(const char* who, const void* depth, int depth_type, int64_t Hd, int64_t Wd, int64_t depth_row_bytes,
                    const uint8_t* color, int64_t Hc, int64_t Wc, int64_t color_row_bytes, const uint8_t* mask,
                    const double* cam_host, int filter_size, int filter_thresh, int flags, const double* box_host,
                    const float* lut, void* workspace, size_t workspace_bytes, float* points, double* points64, float* rgb,
                    int32_t* src, double* registered, int64_t* count, const double* depth_rays, const double* color_rays,
                    const double* color_dist_host, hipStream_t stream) {
  RG_CHECK(Hd >= 1 && Wd >= 1 && Hc >= 1 && Wc >= 1, "image dimensions must be at least 1");
  RG_CHECK(Hd <= RG_MAX_PIXELS && Wd <= RG_MAX_PIXELS && Hd * Wd <= RG_MAX_PIXELS && Hc <= RG_MAX_PIXELS &&
                   Wc <= RG_MAX_PIXELS && Hc * Wc <= RG_MAX_PIXELS,
               "an image holds at most 2^24 pixels");
  RG_CHECK(depth_type == SV_DEPTH_U16 || depth_type == SV_DEPTH_F32, "depth_type must be SV_DEPTH_U16 or SV_DEPTH_F32");
  RG_CHECK(depth_row_bytes >= Wd * (depth_type == SV_DEPTH_F32 ? 4 : 2), "depth_row_bytes does not cover a row");
  RG_CHECK(!color || color_row_bytes >= 3 * Wc, "color_row_bytes does not cover a row");
  RG_CHECK((flags & ~(SV_RGBD_ALIGNED | SV_RGBD_NEAREST | SV_RGBD_BGR)) == 0, "unknown flags");
  RG_CHECK(filter_size == 0 || (filter_size >= 3 && filter_size <= RG_MAX_FILTER && (filter_size & 1)),
               "filter_size must be 0 or odd and in 3..15");
  RG_CHECK(filter_size == 0 || depth_type == SV_DEPTH_U16, "the filter takes SV_DEPTH_U16 depth only");
  RG_CHECK(filter_thresh >= 0, "filter_thresh must not be negative");
  RG_CHECK(cam_host != nullptr, "null pointer (cam_host)");
  for (int k = 0; k < 21; ++k) RG_CHECK(finite64(cam_host[k]), "a cam_host value is not finite");
  RG_CHECK(cam_host[0] != 0.0 && cam_host[1] != 0.0 && cam_host[4] != 0.0 && cam_host[5] != 0.0,
               "a focal length is zero");
  RG_CHECK(cam_host[20] != 0.0, "depth_scale is zero");
  RG_CHECK(!(flags & SV_RGBD_ALIGNED) || (Hd == Hc && Wd == Wc), "SV_RGBD_ALIGNED needs images of one size");
  if (box_host) {
    for (int c = 0; c < 3; ++c) {
      RG_CHECK(box_host[c] == box_host[c] && box_host[3 + c] == box_host[3 + c], "a box bound is NaN");
      RG_CHECK(box_host[c] <= box_host[3 + c], "the box needs lo <= hi");
    }
  }
  RG_CHECK(depth && workspace && points && count && (rgb || !color), "null pointer");
  const bool lens = depth_rays || color_rays || color_dist_host;
  RG_CHECK(!(flags & SV_RGBD_ALIGNED) || (!depth_rays && !color_dist_host),
           "SV_RGBD_ALIGNED takes color_rays only: depth_rays and color_dist_host must be NULL");
  RG_CHECK(!color_dist_host || color_rays, "color_dist_host needs color_rays (the fold-back bound is the table's r2_max)");
  if (color_dist_host)
    for (int k = 0; k < 8; ++k) RG_CHECK(finite64(color_dist_host[k]), "a color_dist_host value is not finite");
  if (workspace_bytes < sv_rgbd_cloud_workspace_bytes(Hd, Wd, Hc, Wc)) {
    set_error("%s: workspace too small", who);
    return SV_ERR_WORKSPACE;
  }
  const int n = (int)(Hc * Wc);
  const int tiles = (n + CP_THREADS - 1) / CP_THREADS;
  Workspace ws(workspace, workspace_bytes);
  unsigned long long* zbuf = ws.take<unsigned long long>((size_t)n);
  int32_t* tile_count = ws.take<int32_t>((size_t)tiles);
  if (!ws.ok) {
    set_error("%s: workspace too small", who);
    return SV_ERR_WORKSPACE;
  }
  RgbdArgs a;
  a.depth = (const uint8_t*)depth;
  a.color = color;
  a.mask = mask;
  a.depth_row = depth_row_bytes;
  a.color_row = color_row_bytes;
  a.Hd = (int)Hd;
  a.Wd = (int)Wd;
  a.Hc = (int)Hc;
  a.Wc = (int)Wc;
  a.tiles_x = (int)((Wd + RG_TW - 1) / RG_TW);
  a.f32 = depth_type == SV_DEPTH_F32;
  a.fsize = filter_size;
  a.fthresh = filter_thresh;
  a.aligned = (flags & SV_RGBD_ALIGNED) != 0;
  a.nearest = (flags & SV_RGBD_NEAREST) != 0;
  a.bgr = (flags & SV_RGBD_BGR) != 0;
  a.has_box = box_host != nullptr;
  // the camera and the box travel as kernel arguments: no copy, no wait
  a.cxd = cam_host[2];
  a.cyd = cam_host[3];
  a.inv_fxd = 1.0 / cam_host[0];
  a.inv_fyd = 1.0 / cam_host[1];
  a.fxc = cam_host[4];
  a.fyc = cam_host[5];
  a.cxc = cam_host[6];
  a.cyc = cam_host[7];
  a.inv_fxc = 1.0 / cam_host[4];
  a.inv_fyc = 1.0 / cam_host[5];
  for (int k = 0; k < 12; ++k) a.H[k] = cam_host[8 + k];
  a.depth_scale = cam_host[20];
  for (int c = 0; c < 3; ++c) {
    a.lo[c] = box_host ? box_host[c] : 0.0;
    a.hi[c] = box_host ? box_host[3 + c] : 0.0;
  }
  // a tile holds at least RG_TH or RG_TW pixels of the image: at most 2^21 tiles, in one grid dimension
  const int64_t ptiles = (int64_t)a.tiles_x * ((Hd + RG_TH - 1) / RG_TH);
  hipLaunchKernelGGL(rgbd_clear_kernel, dim3((unsigned)tiles), dim3(CP_THREADS), 0, stream, zbuf, n, a.nearest ? ~0ull : 0ull);
  RG_LAUNCH_CHECK();
  if (!lens) {
    hipLaunchKernelGGL(rgbd_project_kernel, dim3((unsigned)ptiles), dim3(CP_THREADS), 0, stream, a, zbuf);
    RG_LAUNCH_CHECK();
    hipLaunchKernelGGL(rgbd_count_kernel, dim3((unsigned)tiles), dim3(CP_THREADS), 0, stream, a, zbuf, registered, tile_count);
    RG_LAUNCH_CHECK();
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(CP_THREADS), 0, stream, tile_count, tiles, count);
    RG_LAUNCH_CHECK();
    hipLaunchKernelGGL(rgbd_write_kernel, dim3((unsigned)tiles), dim3(CP_THREADS), 0, stream, a, zbuf, tile_count, lut,
                       (uint32_t*)points, points64, rgb, src);
    RG_LAUNCH_CHECK();
    return SV_OK;
  }
  LensArgs l;
  l.depth_rays = depth_rays;
  l.color_rays = color_rays;
  l.has_dist = color_dist_host != nullptr;
  for (int k = 0; k < 8; ++k) l.D[k] = color_dist_host ? color_dist_host[k] : 0.0;
  hipLaunchKernelGGL(rgbd_project_lens_kernel, dim3((unsigned)ptiles), dim3(CP_THREADS), 0, stream, a, l, zbuf);
  RG_LAUNCH_CHECK();
  hipLaunchKernelGGL(rgbd_count_lens_kernel, dim3((unsigned)tiles), dim3(CP_THREADS), 0, stream, a, l, zbuf, registered,
                     tile_count);
  RG_LAUNCH_CHECK();
  hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(CP_THREADS), 0, stream, tile_count, tiles, count);
  RG_LAUNCH_CHECK();
  hipLaunchKernelGGL(rgbd_write_lens_kernel, dim3((unsigned)tiles), dim3(CP_THREADS), 0, stream, a, l, zbuf, tile_count, lut,
                     (uint32_t*)points, points64, rgb, src);
  RG_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" {

int sv_rgbd_cloud(const void* depth, int depth_type, int64_t Hd, int64_t Wd, int64_t depth_row_bytes, const uint8_t* color,
                  int64_t Hc, int64_t Wc, int64_t color_row_bytes, const uint8_t* mask, const double* cam_host,
                  int filter_size, int filter_thresh, int flags, const double* box_host, const float* lut, void* workspace,
                  size_t workspace_bytes, float* points, double* points64, float* rgb, int32_t* src, double* registered,
                  int64_t* count, sv_stream_t stream) {
  return rgbd_run(__func__, depth, depth_type, Hd, Wd, depth_row_bytes, color, Hc, Wc, color_row_bytes, mask, cam_host,
                  filter_size, filter_thresh, flags, box_host, lut, workspace, workspace_bytes, points, points64, rgb, src,
                  registered, count, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

int sv_rgbd_cloud_lens(const void* depth, int depth_type, int64_t Hd, int64_t Wd, int64_t depth_row_bytes,
                       const uint8_t* color, int64_t Hc, int64_t Wc, int64_t color_row_bytes, const uint8_t* mask,
                       const double* cam_host, int filter_size, int filter_thresh, int flags, const double* box_host,
                       const float* lut, void* workspace, size_t workspace_bytes, float* points, double* points64, float* rgb,
                       int32_t* src, double* registered, int64_t* count, const double* depth_rays, const double* color_rays,
                       const double* color_dist_host, sv_stream_t stream) {
  return rgbd_run(__func__, depth, depth_type, Hd, Wd, depth_row_bytes, color, Hc, Wc, color_row_bytes, mask, cam_host,
                  filter_size, filter_thresh, flags, box_host, lut, workspace, workspace_bytes, points, points64, rgb, src,
                  registered, count, depth_rays, color_rays, color_dist_host, (hipStream_t)stream);
}

int sv_lens_rays(const double* cam_host, const double* dist_host, int64_t H, int64_t W, double* rays, sv_stream_t stream_) {
  const char* who = __func__;
  hipStream_t stream = (hipStream_t)stream_;
  RG_CHECK(H >= 1 && W >= 1, "image dimensions must be at least 1");
  RG_CHECK(H <= RG_MAX_PIXELS && W <= RG_MAX_PIXELS && H * W <= RG_MAX_PIXELS, "an image holds at most 2^24 pixels");
  RG_CHECK(cam_host && dist_host && rays, "null pointer");
  for (int k = 0; k < 4; ++k) RG_CHECK(finite64(cam_host[k]), "a cam_host value is not finite");
  for (int k = 0; k < 8; ++k) RG_CHECK(finite64(dist_host[k]), "a dist_host value is not finite");
  RG_CHECK(cam_host[0] != 0.0 && cam_host[1] != 0.0, "a focal length is zero");
  LensCam c;
  c.fx = cam_host[0];
  c.fy = cam_host[1];
  c.cx = cam_host[2];
  c.cy = cam_host[3];
  c.inv_fx = 1.0 / cam_host[0];
  c.inv_fy = 1.0 / cam_host[1];
  for (int k = 0; k < 8; ++k) c.D[k] = dist_host[k];
  c.H = (int)H;
  c.W = (int)W;
  const int n = (int)(H * W);
  const int tiles = (n + CP_THREADS - 1) / CP_THREADS;
  // r2_max starts as +0.0 (all bits clear), the result when no pixel is valid
  hipLaunchKernelGGL(rgbd_clear_kernel, dim3(1), dim3(CP_THREADS), 0, stream, (unsigned long long*)(rays + 2 * (int64_t)n), 1,
                     0ull);
  RG_LAUNCH_CHECK();
  hipLaunchKernelGGL(lens_rays_kernel, dim3((unsigned)tiles), dim3(CP_THREADS), 0, stream, c, rays);
  RG_LAUNCH_CHECK();
  return SV_OK;
}

}  // extern "C"
