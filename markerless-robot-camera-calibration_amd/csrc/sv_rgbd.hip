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

__global__ __launch_bounds__(CP_THREADS) void rgbd_clear_kernel(unsigned long long* __restrict__ zbuf, int n,
                                                                 unsigned long long value) {
  const int j = blockIdx.x * CP_THREADS + threadIdx.x;
  if (j < n) zbuf[j] = value;
}

__global__ __launch_bounds__(CP_THREADS) void rgbd_project_kernel(RgbdArgs a, unsigned long long* __restrict__ zbuf) {
  __shared__ uint16_t tile[RG_LDS];
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
  const double x = (((double)u - a.cxd) * d) * a.inv_fxd;
  const double y = (((double)v - a.cyd) * d) * a.inv_fyd;
  const double z = d;
  const double X = ((a.H[0] * x + a.H[1] * y) + a.H[2] * z) + a.H[3];
  const double Y = ((a.H[4] * x + a.H[5] * y) + a.H[6] * z) + a.H[7];
  const double Z = ((a.H[8] * x + a.H[9] * y) + a.H[10] * z) + a.H[11];
  const double iz = 1.0 / Z;
  const double uu = (a.fxc * X) * iz + a.cxc;
  const double vv = (a.fyc * Y) * iz + a.cyc;
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

// registered depth of colour pixel j, its point as float64 and as float32 bits, and its keep flag
__device__ __forceinline__ bool rgbd_point(const RgbdArgs& a, const unsigned long long* __restrict__ zbuf, int j, double& r,
                                           double p[3], uint32_t q[3]) {
  const unsigned long long zb = zbuf[j];
  r = (!a.aligned && zb == z_empty(a)) ? 0.0 : __longlong_as_double((long long)zb);
  const int v = j / a.Wc, u = j - v * a.Wc;
  bool keep = r > 0.0;  // false for a NaN
  if (a.mask) keep = keep && a.mask[j] == 0;
  p[0] = (((double)u - a.cxc) * r) * a.inv_fxc;
  p[1] = (((double)v - a.cyc) * r) * a.inv_fyc;
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

__global__ __launch_bounds__(CP_THREADS) void rgbd_count_kernel(RgbdArgs a, const unsigned long long* __restrict__ zbuf,
                                                                 double* __restrict__ registered,
                                                                 int32_t* __restrict__ tile_count) {
  __shared__ int wave_cnt[CP_WAVES];
  const int j = blockIdx.x * CP_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  bool keep = false;
  if (j < a.Hc * a.Wc) {
    double r, p[3];
    uint32_t q[3];
    keep = rgbd_point(a, zbuf, j, r, p, q);
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

__global__ __launch_bounds__(CP_THREADS) void rgbd_write_kernel(RgbdArgs a, const unsigned long long* __restrict__ zbuf,
                                                                 const int32_t* __restrict__ tile_base,
                                                                 const float* __restrict__ lut, uint32_t* __restrict__ points,
                                                                 double* __restrict__ points64, float* __restrict__ rgb,
                                                                 int32_t* __restrict__ src) {
  __shared__ int wave_cnt[CP_WAVES];
  const int j = blockIdx.x * CP_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  bool keep = false;
  double r, p[3] = {0.0, 0.0, 0.0};
  uint32_t q[3] = {0, 0, 0};
  if (j < a.Hc * a.Wc) keep = rgbd_point(a, zbuf, j, r, p, q);
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

int sv_rgbd_cloud(const void* depth, int depth_type, int64_t Hd, int64_t Wd, int64_t depth_row_bytes, const uint8_t* color,
                  int64_t Hc, int64_t Wc, int64_t color_row_bytes, const uint8_t* mask, const double* cam_host,
                  int filter_size, int filter_thresh, int flags, const double* box_host, const float* lut, void* workspace,
                  size_t workspace_bytes, float* points, double* points64, float* rgb, int32_t* src, double* registered,
                  int64_t* count, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(Hd >= 1 && Wd >= 1 && Hc >= 1 && Wc >= 1, "image dimensions must be at least 1");
  SV_CHECK_ARG(Hd <= RG_MAX_PIXELS && Wd <= RG_MAX_PIXELS && Hd * Wd <= RG_MAX_PIXELS && Hc <= RG_MAX_PIXELS &&
                   Wc <= RG_MAX_PIXELS && Hc * Wc <= RG_MAX_PIXELS,
               "an image holds at most 2^24 pixels");
  SV_CHECK_ARG(depth_type == SV_DEPTH_U16 || depth_type == SV_DEPTH_F32, "depth_type must be SV_DEPTH_U16 or SV_DEPTH_F32");
  SV_CHECK_ARG(depth_row_bytes >= Wd * (depth_type == SV_DEPTH_F32 ? 4 : 2), "depth_row_bytes does not cover a row");
  SV_CHECK_ARG(!color || color_row_bytes >= 3 * Wc, "color_row_bytes does not cover a row");
  SV_CHECK_ARG((flags & ~(SV_RGBD_ALIGNED | SV_RGBD_NEAREST | SV_RGBD_BGR)) == 0, "unknown flags");
  SV_CHECK_ARG(filter_size == 0 || (filter_size >= 3 && filter_size <= RG_MAX_FILTER && (filter_size & 1)),
               "filter_size must be 0 or odd and in 3..15");
  SV_CHECK_ARG(filter_size == 0 || depth_type == SV_DEPTH_U16, "the filter takes SV_DEPTH_U16 depth only");
  SV_CHECK_ARG(filter_thresh >= 0, "filter_thresh must not be negative");
  SV_CHECK_ARG(cam_host != nullptr, "null pointer (cam_host)");
  for (int k = 0; k < 21; ++k) SV_CHECK_ARG(finite64(cam_host[k]), "a cam_host value is not finite");
  SV_CHECK_ARG(cam_host[0] != 0.0 && cam_host[1] != 0.0 && cam_host[4] != 0.0 && cam_host[5] != 0.0,
               "a focal length is zero");
  SV_CHECK_ARG(cam_host[20] != 0.0, "depth_scale is zero");
  SV_CHECK_ARG(!(flags & SV_RGBD_ALIGNED) || (Hd == Hc && Wd == Wc), "SV_RGBD_ALIGNED needs images of one size");
  if (box_host) {
    for (int c = 0; c < 3; ++c) {
      SV_CHECK_ARG(box_host[c] == box_host[c] && box_host[3 + c] == box_host[3 + c], "a box bound is NaN");
      SV_CHECK_ARG(box_host[c] <= box_host[3 + c], "the box needs lo <= hi");
    }
  }
  SV_CHECK_ARG(depth && workspace && points && count && (rgb || !color), "null pointer");
  if (workspace_bytes < sv_rgbd_cloud_workspace_bytes(Hd, Wd, Hc, Wc)) {
    set_error("sv_rgbd_cloud: workspace too small");
    return SV_ERR_WORKSPACE;
  }
  const int n = (int)(Hc * Wc);
  const int tiles = (n + CP_THREADS - 1) / CP_THREADS;
  Workspace ws(workspace, workspace_bytes);
  unsigned long long* zbuf = ws.take<unsigned long long>((size_t)n);
  int32_t* tile_count = ws.take<int32_t>((size_t)tiles);
  if (!ws.ok) {
    set_error("sv_rgbd_cloud: workspace too small");
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
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(rgbd_project_kernel, dim3((unsigned)ptiles), dim3(CP_THREADS), 0, stream, a, zbuf);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(rgbd_count_kernel, dim3((unsigned)tiles), dim3(CP_THREADS), 0, stream, a, zbuf, registered, tile_count);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(CP_THREADS), 0, stream, tile_count, tiles, count);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(rgbd_write_kernel, dim3((unsigned)tiles), dim3(CP_THREADS), 0, stream, a, zbuf, tile_count, lut,
                     (uint32_t*)points, points64, rgb, src);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

}  // extern "C"
