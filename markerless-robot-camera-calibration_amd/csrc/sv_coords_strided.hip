// Coordinate maps of STRIDED convolutions and pooling at a tensor stride that is no power of two: what
// ME.MinkowskiConvolution(kernel_size=3, stride=3) of model/backbone/resnet.py:48-127 asks of the coordinate manager.  The
// power-of-two stride maps and every kernel map (sv_kernel_map_probe among them) are in sv_coords.hip.
//
// A general tensor stride does not keep the canonical (batch | Morton) order under coordinate flooring - clearing key bits
// does, which is all sv_stride_map does - so sv_stride_map_general re-keys every voxel, sorts (sv_sort.hip) and uniques.
#include "sv_common.h"

namespace sv {

// floor(c / s) * s on the signed coordinate (towards minus infinity), s > 0
__host__ __device__ __forceinline__ int floor_to_stride(int c, int s) {
  int q = c / s;
  if (c % s != 0 && c < 0) --q;
  return q * s;
}

__global__ __launch_bounds__(256) void stride_rekey_kernel(const uint64_t* __restrict__ keys_in, int64_t n, int s_out,
                                                            uint64_t* __restrict__ keys, int32_t* __restrict__ counters) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int b, x, y, z;
  decode_key(keys_in[i], b, x, y, z);
  x = floor_to_stride(x, s_out);
  y = floor_to_stride(y, s_out);
  z = floor_to_stride(z, s_out);
  if (!coord_in_range(b, x, y, z)) {  // below -2^17 after flooring: counted, keyed as sv_voxelize keys a bad point
    atomicAdd(&counters[1], 1);
    b = x = y = z = 0;
  }
  keys[i] = make_key(b, x, y, z);
}

__global__ __launch_bounds__(256) void stride_general_scatter_kernel(const uint64_t* __restrict__ keys_in, int s_out,
                                                                      const uint64_t* __restrict__ skeys,
                                                                      const int32_t* __restrict__ sidx,
                                                                      const int32_t* __restrict__ rank, int64_t n,
                                                                      uint64_t* __restrict__ keys_out,
                                                                      int32_t* __restrict__ vcoords_out,
                                                                      int32_t* __restrict__ parent) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int v = rank[j];
  const int i = sidx[j];
  int b, x, y, z;
  decode_key(keys_in[i], b, x, y, z);
  const bool ok = coord_in_range(b, floor_to_stride(x, s_out), floor_to_stride(y, s_out), floor_to_stride(z, s_out));
  parent[i] = ok ? v : -1;
  if (j == 0 || rank[j - 1] != v) {
    const uint64_t k = skeys[j];
    keys_out[v] = k;
    decode_key(k, b, x, y, z);
    ((int4*)vcoords_out)[v] = make_int4(b, x, y, z);
  }
}

}  // namespace sv

using namespace sv;

extern "C" {

size_t sv_stride_map_general_workspace_bytes(int64_t V_in) {
  if (V_in <= 0) return 256;
  const size_t n = (size_t)V_in;
  return align_up(n * 8, 256) * 2 + align_up(n * 4, 256) * 2 + align_up(unique_sorted_blocks(V_in) * 4 + 4, 256) +
         align_up(radix_sort_temp_bytes(V_in, sizeof(uint64_t)), 256) + 4096;
}

int sv_stride_map_general(const uint64_t* keys_in, int64_t V_in, int s_in, int s_out, void* workspace, size_t workspace_bytes,
                          uint64_t* keys_out, int32_t* vcoords_out, int32_t* parent, int32_t* counters, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(V_in >= 0 && V_in < (1ll << 31) - 1024, "V_in out of range");
  SV_CHECK_ARG(s_in >= 1 && s_out >= s_in && s_out < (1 << SV_COORD_BITS), "tensor strides out of range");
  SV_CHECK_ARG(s_out % s_in == 0, "s_out must be a multiple of s_in");
  SV_CHECK_ARG(counters != nullptr, "counters is null");
  if (V_in > 0) SV_CHECK_ARG(keys_in && keys_out && vcoords_out && parent && workspace, "null pointer");
  Workspace ws(workspace, workspace_bytes);
  uint64_t* k_in = nullptr;
  uint64_t* k_sorted = nullptr;
  int32_t *i_sorted = nullptr, *rank = nullptr, *blocks = nullptr;
  char* sort_tmp = nullptr;
  size_t sort_bytes = 0;
  if (V_in > 0) {
    k_in = ws.take<uint64_t>(V_in);
    k_sorted = ws.take<uint64_t>(V_in);
    i_sorted = ws.take<int32_t>(V_in);
    rank = ws.take<int32_t>(V_in);
    blocks = ws.take<int32_t>(unique_sorted_blocks(V_in) + 1);
    sort_bytes = radix_sort_temp_bytes(V_in, sizeof(uint64_t));
    sort_tmp = ws.take<char>(sort_bytes);
    if (!ws.ok) {
      set_error("sv_stride_map_general: workspace too small (%zu given)", workspace_bytes);
      return SV_ERR_WORKSPACE;
    }
  }
  SV_HIP(hipMemsetAsync(counters, 0, 4 * sizeof(int32_t), stream));
  if (V_in == 0) return SV_OK;
  const unsigned nb = (unsigned)((V_in + 255) / 256);
  hipLaunchKernelGGL(stride_rekey_kernel, dim3(nb), dim3(256), 0, stream, keys_in, V_in, s_out, k_in, counters);
  SV_LAUNCH_CHECK();
  int rc = radix_sort_pairs<uint64_t>(k_in, nullptr, k_sorted, i_sorted, V_in, 0, 64, sort_tmp, sort_bytes, stream);
  if (rc) return rc;
  rc = launch_unique_sorted(k_sorted, V_in, ~0ull, rank, blocks, &counters[0], stream);
  if (rc) return rc;
  hipLaunchKernelGGL(stride_general_scatter_kernel, dim3(nb), dim3(256), 0, stream, keys_in, s_out, k_sorted, i_sorted, rank,
                     V_in, keys_out, vcoords_out, parent);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

}  // extern "C"
