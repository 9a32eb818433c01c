// The middle launch of the ordered compaction that sv_ingest.hip and sv_rgbd.hip share: per-tile counts (ballot + popcount
// in the caller's own kernel) -> exclusive scan by ONE workgroup -> ordered write (again the caller's kernel).
#pragma once
#include "sv_common.h"

namespace sv {

constexpr int CP_THREADS = 256;  // elements per tile, and the threads of the scan's one workgroup
constexpr int CP_WAVES = CP_THREADS / 64;

// tile_count[t] -> the number kept in the tiles before t, in place; count[0] = the number kept
static __global__ __launch_bounds__(CP_THREADS) void compact_scan_kernel(int32_t* __restrict__ tile_count, int tiles,
                                                                         int64_t* __restrict__ count) {
  __shared__ int wave_sum[CP_WAVES];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int carry = 0;  // at most 2^24
  for (int base = 0; base < tiles; base += CP_THREADS) {
    const int t = base + threadIdx.x;
    const int c = t < tiles ? tile_count[t] : 0;
    int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d);
      if (lane >= d) incl += o;
    }
    if (lane == 63) wave_sum[wid] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < CP_WAVES; ++k) {
      const int s = wave_sum[k];
      before += k < wid ? s : 0;
      total += s;
    }
    if (t < tiles) tile_count[t] = carry + before + incl - c;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) count[0] = carry;
}

}  // namespace sv
