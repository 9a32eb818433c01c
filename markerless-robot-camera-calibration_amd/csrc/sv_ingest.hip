// N3e: packed sensor records -> points, colours and source indices on the device (the reference decodes a ROS
// PointCloud2 on the host, utils/ros_utils.py get_points_and_colors, and reads .pcd frames through Open3D,
// app/data_engine.py PCDDataEngine).  A PointCloud2 `data` buffer and a binary PCD body are the same thing: a strided
// array of fixed-layout records.  Definitions in include/sv_hip.h; every output equals a numpy restatement bit for bit.
//
// Three launches, no atomics, no memset, no read-back:
//   unpack_count_kernel : one record per thread, keep flag -> ballot + popcount per wave, the four wave totals of a tile
//                         through LDS -> tile_count[tile]
//   compact_scan_kernel : sv_compact.h.  ONE workgroup, exclusive scan of the tile counts in place (it loops when there
//                         are more tiles than threads), total -> count[0]
//   unpack_write_kernel : recomputes the keep flags, row = tile base + waves before + lanes before (the ordered-write
//                         idiom of elim_table_kernel and the ball query), then decodes the colour of the kept records only
//
// Fields are assembled from single bytes, so a record may sit at any byte address (point_step = 19, a uint8 field in front
// of x, row padding) on one code path.  A tile's records are NOT staged through LDS: with point_step up to 4096 and row
// padding a tile's byte span has no bound, and the 16 bytes a record contributes are read once per pass from cache lines
// that neighbouring lanes share.  There is no dword path for 4-aligned layouts: on a 640 x 480 frame of 32-byte records a
// call of either form took the 24 us the host needs to issue it (tools/ingest_timing.py), so the second path
// would only have been more to test.
#include "sv_common.h"
#include "sv_compact.h"

namespace sv {

constexpr int UP_THREADS = CP_THREADS;  // records per tile, and the threads of the scan's one workgroup
constexpr int UP_WAVES = UP_THREADS / 64;
constexpr int64_t UP_MAX_RECORDS = 1 << 24;
constexpr int64_t UP_MAX_STEP = 4096;

struct UnpackArgs {
  const uint8_t* data;
  int64_t row_step;
  int n, width, point_step;  // width is clamped to n by the host: i / width is then the same for every i < n
  int off[3], rgb_off;
  int f64, big, keep_nonfinite, has_box;
  double lo[3], hi[3];
};

__device__ __forceinline__ uint32_t load32(const uint8_t* __restrict__ p, bool big) {
  const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
  return big ? __builtin_bswap32(v) : v;
}

// float32 bits of a float64 given as bits: round to nearest even (a finite value beyond FLT_MAX becomes inf); a NaN
// keeps its sign and the top 22 payload bits and has its quiet bit set, whatever the hardware conversion would do
__device__ __forceinline__ uint32_t f64_bits_to_f32_bits(uint64_t u) {
  if ((u & 0x7fffffffffffffffull) > 0x7ff0000000000000ull)
    return (uint32_t)((u >> 32) & 0x80000000u) | 0x7fc00000u | (uint32_t)((u >> 29) & 0x003fffffu);
  return __float_as_uint((float)__longlong_as_double((long long)u));
}

// Coordinates of record i as float32 bits and its keep flag.
__device__ __forceinline__ bool decode_xyz(const UnpackArgs& a, int i, const uint8_t* __restrict__& rec, uint32_t p[3]) {
  const int row = i / a.width, col = i - row * a.width;
  rec = a.data + (int64_t)row * a.row_step + (int64_t)col * a.point_step;
  bool keep = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint8_t* f = rec + a.off[c];
    bool finite;
    if (a.f64) {
      const uint32_t w0 = load32(f, a.big), w1 = load32(f + 4, a.big);
      const uint64_t u = a.big ? ((uint64_t)w0 << 32) | w1 : ((uint64_t)w1 << 32) | w0;
      finite = (u & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;  // tested as a double, before the rounding
      p[c] = f64_bits_to_f32_bits(u);
    } else {
      p[c] = load32(f, a.big);
      finite = (p[c] & 0x7f800000u) != 0x7f800000u;
    }
    keep = keep && (finite || a.keep_nonfinite);
    if (a.has_box) {
      const double v = (double)__uint_as_float(p[c]);
      keep = keep && (a.lo[c] < v) && (v < a.hi[c]);  // strict; false for NaN
    }
  }
  return keep;
}

__global__ __launch_bounds__(UP_THREADS) void unpack_count_kernel(UnpackArgs a, int32_t* __restrict__ tile_count) {
  __shared__ int wave_cnt[UP_WAVES];
  const int i = blockIdx.x * UP_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  bool keep = false;
  if (i < a.n) {
    const uint8_t* rec;
    uint32_t p[3];
    keep = decode_xyz(a, i, rec, p);
  }
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wave_cnt[wid] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < UP_WAVES; ++k) s += wave_cnt[k];
    tile_count[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(UP_THREADS) void unpack_write_kernel(UnpackArgs a, const int32_t* __restrict__ tile_base,
                                                                   const float* __restrict__ lut,
                                                                   uint32_t* __restrict__ points, float* __restrict__ rgb,
                                                                   int32_t* __restrict__ src) {
  __shared__ int wave_cnt[UP_WAVES];
  const int i = blockIdx.x * UP_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  bool keep = false;
  const uint8_t* rec = a.data;
  uint32_t p[3] = {0, 0, 0};
  if (i < a.n) keep = decode_xyz(a, i, rec, p);
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wave_cnt[wid] = __popcll(m);
  __syncthreads();
  if (!keep) return;
  int before = 0;
#pragma unroll
  for (int k = 0; k < UP_WAVES; ++k) before += k < wid ? wave_cnt[k] : 0;
  // row < the number kept <= n: inside the caller's [n][3] arrays
  const int64_t row = (int64_t)tile_base[blockIdx.x] + before + __popcll(m & ((1ull << lane) - 1ull));
  points[row * 3] = p[0];
  points[row * 3 + 1] = p[1];
  points[row * 3 + 2] = p[2];
  if (src) src[row] = i;
  if (a.rgb_off >= 0) {
    const uint32_t v = load32(rec + a.rgb_off, a.big);
    const int r = (v >> 16) & 255, g = (v >> 8) & 255, b = v & 255;
    rgb[row * 3] = lut ? lut[r] : (float)r;
    rgb[row * 3 + 1] = lut ? lut[g] : (float)g;
    rgb[row * 3 + 2] = lut ? lut[b] : (float)b;
  }
}

static inline bool disjoint(int a, int an, int b, int bn) { return a + an <= b || b + bn <= a; }

}  // namespace sv

using namespace sv;

extern "C" {

size_t sv_unpack_points_workspace_bytes(int64_t n_records) {
  const size_t n = (size_t)(n_records > 0 ? n_records : 0);
  return align_up((n + UP_THREADS - 1) / UP_THREADS * sizeof(int32_t), 256) + 256;
}

int sv_unpack_points(const uint8_t* data, int64_t data_bytes, int64_t n_records, int64_t width, int64_t point_step,
                     int64_t row_step, int x_off, int y_off, int z_off, int xyz_type, int rgb_off, int flags,
                     const double* box_host, const float* lut, void* workspace, size_t workspace_bytes, float* points,
                     float* rgb, int32_t* src, int64_t* count, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(n_records >= 1 && n_records <= UP_MAX_RECORDS, "need 1 to 2^24 records");
  SV_CHECK_ARG(width >= 1, "width must be at least 1");
  SV_CHECK_ARG(point_step >= 1 && point_step <= UP_MAX_STEP, "point_step must lie in [1, 4096]");
  SV_CHECK_ARG(row_step >= 0 && width <= row_step / point_step, "row_step must be at least width * point_step");
  SV_CHECK_ARG(xyz_type == SV_FIELD_F32 || xyz_type == SV_FIELD_F64, "xyz_type must be SV_FIELD_F32 or SV_FIELD_F64");
  SV_CHECK_ARG((flags & ~(SV_UNPACK_BIGENDIAN | SV_UNPACK_KEEP_NONFINITE)) == 0, "unknown flags");
  const int fsize = xyz_type == SV_FIELD_F64 ? 8 : 4;
  const int off[3] = {x_off, y_off, z_off};
  for (int c = 0; c < 3; ++c)
    SV_CHECK_ARG(off[c] >= 0 && (int64_t)off[c] + fsize <= point_step, "an x, y or z field lies outside the record");
  SV_CHECK_ARG(rgb_off < 0 || (int64_t)rgb_off + 4 <= point_step, "the rgb field lies outside the record");
  SV_CHECK_ARG(disjoint(x_off, fsize, y_off, fsize) && disjoint(x_off, fsize, z_off, fsize) &&
                   disjoint(y_off, fsize, z_off, fsize),
               "the x, y and z fields overlap");
  if (rgb_off >= 0)
    for (int c = 0; c < 3; ++c) SV_CHECK_ARG(disjoint(off[c], fsize, rgb_off, 4), "the rgb field overlaps a coordinate field");
  {  // the last record ends inside the buffer (every step is >= 0, so it ends last); no product here can overflow
    const int64_t rows = (n_records - 1) / width, col = (n_records - 1) % width;
    SV_CHECK_ARG(data_bytes >= 1 && (rows == 0 || row_step <= data_bytes / rows) &&
                     rows * row_step + (col + 1) * point_step <= data_bytes,
                 "data_bytes does not cover the last record");
  }
  if (box_host) {
    for (int c = 0; c < 3; ++c) {
      SV_CHECK_ARG(box_host[c] == box_host[c] && box_host[3 + c] == box_host[3 + c], "a box bound is NaN");
      SV_CHECK_ARG(box_host[c] <= box_host[3 + c], "the box needs lo <= hi");
    }
  }
  SV_CHECK_ARG(data && workspace && points && count && (rgb || rgb_off < 0), "null pointer");
  if (workspace_bytes < sv_unpack_points_workspace_bytes(n_records)) {
    set_error("sv_unpack_points: workspace too small");
    return SV_ERR_WORKSPACE;
  }
  const int tiles = (int)((n_records + UP_THREADS - 1) / UP_THREADS);
  Workspace ws(workspace, workspace_bytes);
  int32_t* tile_count = ws.take<int32_t>((size_t)tiles);
  if (!ws.ok) {
    set_error("sv_unpack_points: workspace too small");
    return SV_ERR_WORKSPACE;
  }
  UnpackArgs a;
  a.data = data;
  a.row_step = row_step;
  a.n = (int)n_records;
  a.width = (int)(width < n_records ? width : n_records);
  a.point_step = (int)point_step;
  for (int c = 0; c < 3; ++c) {
    a.off[c] = off[c];
    a.lo[c] = box_host ? box_host[c] : 0.0;  // the six values travel as kernel arguments: no copy, no wait
    a.hi[c] = box_host ? box_host[3 + c] : 0.0;
  }
  a.rgb_off = rgb_off;
  a.f64 = xyz_type == SV_FIELD_F64;
  a.big = (flags & SV_UNPACK_BIGENDIAN) != 0;
  a.keep_nonfinite = (flags & SV_UNPACK_KEEP_NONFINITE) != 0;
  a.has_box = box_host != nullptr;
  uint32_t* pbits = (uint32_t*)points;  // coordinates move as bits
  hipLaunchKernelGGL(unpack_count_kernel, dim3((unsigned)tiles), dim3(UP_THREADS), 0, stream, a, tile_count);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(UP_THREADS), 0, stream, tile_count, tiles, count);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(unpack_write_kernel, dim3((unsigned)tiles), dim3(UP_THREADS), 0, stream, a, tile_count, lut, pbits, rgb,
                     src);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

}  // extern "C"
