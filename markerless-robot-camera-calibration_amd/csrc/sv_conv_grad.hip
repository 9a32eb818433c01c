// Weight gradient of the sparse convolution (include/sv_hip.h sv_conv_wgrad):
//   dW[k][c][n] = sum over plan rows r with o = perm[r] >= 0, i = nbr_s[k][r] >= 0 of  in[i][c] * dY[o][n]
// a gather-GEMM per kernel offset whose reduction runs over that offset's (in, out) pairs.  The forward's own plan is
// reused: its 16-row sub-tiles group rows that share neighbours, so `submask` lets a workgroup skip every sub-tile with
// no pair at its offset.
//
// Tile: one workgroup = 4 waves = a 64 (Cin) x 64 (Cout) block of dW[k]; each wave owns a 32 x 32 quarter as 2 x 2
// accumulators of v_mfma_f32_16x16x4_f32 with A = in^T, B = dY (reduction dimension = pairs):
//   lane l: A[l & 15][l >> 4] = in[row l >> 4][c0 + (l & 15)],  B[l >> 4][l & 15] = dY[row l >> 4][n0 + (l & 15)]
// so both operands are plain row-major rows of the 16-row sub-tile staged in LDS, no transpose.  The next sub-tile's
// rows are gathered into registers while the matrix ops of the current one run.
// Grid: (Cin blocks x Cout blocks, K, chunks of plan tiles).  Every chunk writes its partial dW to the workspace; a
// second pass sums the partials in ascending chunk order: no float atomics, two runs give the same bits.
#include "sv_common.h"

namespace sv {
namespace {

constexpr int WG_TILE = 128;    // plan tile rows (SV_TILE_ROWS)
constexpr int SUB = 16;         // rows per sub-tile (one submask bit)
constexpr int BC = 64;          // Cin block
constexpr int BN = 64;          // Cout block
constexpr int LDS_LD = BC + 4;  // padded LDS row
constexpr int TARGET_WGS = 2048;  // enough workgroups to fill 256 CUs several times over
constexpr int MAX_CHUNKS = 128;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct WgradParams {
  const float* in;
  int64_t V_in, in_ld;
  int Cin;
  const float* dy;
  int64_t V_out, dy_ld;
  int Cout, K;
  const int32_t* perm;
  const int32_t* nbr_s;
  const uint32_t* submask;
  int64_t Vpad;
  int ntiles, chunks, tiles_per_chunk;
  bool vec_a, vec_b;  // rows 16-byte aligned with channel counts % 4 == 0: one 16-byte load per thread and operand
  float* part;  // [chunks][K][Cin][Cout]
};

// 256 threads stage one 16 x 64 block of each operand: thread t -> row t >> 4, columns 4 (t & 15) .. + 3
struct Stage {
  float a[4], b[4];
};

__device__ __forceinline__ void gather(const WgradParams& p, int k, int64_t r, int c0, int n0, Stage& s) {
  const int t = threadIdx.x;
  const int64_t row = r + (t >> 4);
  const int col = 4 * (t & 15);
  int64_t i = -1, o = -1;
  if (p.perm) {
    if (row < p.Vpad) {
      o = p.perm[row];
      i = p.nbr_s[(int64_t)k * p.Vpad + row];
    }
  } else if (row < p.V_out) {
    o = i = row;
  }
  // a pair needs both rows: an absent one zeroes BOTH operands (0 * inf in the other would otherwise give NaN)
  const bool ok = o >= 0 && o < p.V_out && i >= 0 && i < p.V_in;
  const float* ar = p.in + (ok ? i : 0) * p.in_ld;
  const float* br = p.dy + (ok ? o : 0) * p.dy_ld;
  if (p.vec_a) {
    const float4 v = (ok && c0 + col < p.Cin) ? *(const float4*)(ar + c0 + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    s.a[0] = v.x; s.a[1] = v.y; s.a[2] = v.z; s.a[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) s.a[j] = (ok && c0 + col + j < p.Cin) ? ar[c0 + col + j] : 0.f;
  }
  if (p.vec_b) {
    const float4 v = (ok && n0 + col < p.Cout) ? *(const float4*)(br + n0 + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    s.b[0] = v.x; s.b[1] = v.y; s.b[2] = v.z; s.b[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) s.b[j] = (ok && n0 + col + j < p.Cout) ? br[n0 + col + j] : 0.f;
  }
}

__global__ void __launch_bounds__(256) wgrad_kernel(WgradParams p) {
  __shared__ __attribute__((aligned(16))) float sA[SUB][LDS_LD];
  __shared__ __attribute__((aligned(16))) float sB[SUB][LDS_LD];
  const int nbn = (p.Cout + BN - 1) / BN;
  const int c0 = (blockIdx.x / nbn) * BC, n0 = (blockIdx.x % nbn) * BN;
  const int k = blockIdx.y;
  const int chunk = blockIdx.z;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wc = (wave >> 1) * 32, wn = (wave & 1) * 32;  // the wave's quarter of the block
  f32x4 acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) acc[x][y] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int t0 = chunk * p.tiles_per_chunk;
  const int t1 = min(t0 + p.tiles_per_chunk, p.ntiles);
  // walk the sub-tiles of this chunk that hold a pair at offset k (all of them for dense rows)
  int tile = t0, s = -1;
  uint32_t bits = 0;
  auto next = [&]() -> int64_t {  // plan row of the next live sub-tile, or -1 (uniform over the workgroup)
    for (;;) {
      if (bits == 0) {
        if (tile >= t1) return -1;
        bits = p.submask ? p.submask[(int64_t)tile * p.K + k] & 0xffu : 0xffu;
        s = tile++;
        continue;
      }
      const int b = __builtin_ctz(bits);
      bits &= bits - 1;
      return (int64_t)s * WG_TILE + b * SUB;
    }
  };
  int64_t r = next();
  Stage st;
  if (r >= 0) gather(p, k, r, c0, n0, st);
  while (r >= 0) {
    __syncthreads();  // the previous sub-tile's operands have been read
    const int row = t >> 4, col = 4 * (t & 15);
    *(float4*)&sA[row][col] = make_float4(st.a[0], st.a[1], st.a[2], st.a[3]);
    *(float4*)&sB[row][col] = make_float4(st.b[0], st.b[1], st.b[2], st.b[3]);
    __syncthreads();
    r = next();
    if (r >= 0) gather(p, k, r, c0, n0, st);  // in flight while the matrix ops below run
#pragma unroll
    for (int kk = 0; kk < SUB; kk += 4) {
      const int rr = kk + (lane >> 4), cc = lane & 15;
      const float a0 = sA[rr][wc + cc], a1 = sA[rr][wc + 16 + cc];
      const float b0 = sB[rr][wn + cc], b1 = sB[rr][wn + 16 + cc];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
  // D[i][j]: j = lane & 15, i = 4 (lane >> 4) + reg
  float* out = p.part + ((int64_t)chunk * p.K + k) * p.Cin * p.Cout;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      const int n = n0 + wn + 16 * y + (lane & 15);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c = c0 + wc + 16 * x + 4 * (lane >> 4) + g;
        if (c < p.Cin && n < p.Cout) out[(int64_t)c * p.Cout + n] = acc[x][y][g];
      }
    }
}

// dW = (accumulate ? dW : 0) + (partial_0 + partial_1 + ... ) summed in ascending chunk order
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float* __restrict__ part, int chunks, int64_t n,
                                                           int accumulate, float* __restrict__ dW) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  float s = part[e];
  for (int ch = 1; ch < chunks; ++ch) s += part[(int64_t)ch * n + e];
  dW[e] = accumulate ? dW[e] + s : s;
}

int wgrad_chunks(int64_t Vpad, int K, int Cin, int Cout) {
  const int64_t ntiles = Vpad / WG_TILE;
  const int64_t blocks = (int64_t)((Cin + BC - 1) / BC) * ((Cout + BN - 1) / BN) * K;
  int64_t c = (TARGET_WGS + blocks - 1) / blocks;
  if (c > MAX_CHUNKS) c = MAX_CHUNKS;
  if (c > ntiles) c = ntiles;
  return c < 1 ? 1 : (int)c;
}

}  // namespace
}  // namespace sv

extern "C" size_t sv_conv_wgrad_workspace_bytes(int64_t Vpad, int K, int Cin, int Cout) {
  if (Vpad <= 0 || K <= 0 || Cin <= 0 || Cout <= 0) return 0;
  const int64_t vp = (Vpad + sv::WG_TILE - 1) / sv::WG_TILE * sv::WG_TILE;
  return (size_t)sv::wgrad_chunks(vp, K, Cin, Cout) * (size_t)K * (size_t)Cin * (size_t)Cout * sizeof(float) + 256;
}

extern "C" int sv_conv_wgrad(const float* in, int64_t V_in, int64_t in_ld, int Cin, const float* dy, int64_t V_out,
                             int64_t dy_ld, int Cout, int K, const int32_t* perm, const int32_t* nbr_s,
                             const uint32_t* submask, int64_t Vpad, int accumulate, void* workspace,
                             size_t workspace_bytes, float* dW, sv_stream_t stream_) {
  using namespace sv;
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(Cin > 0 && Cout > 0 && K >= 1 && K <= 32, "bad channel / kernel volume");
  SV_CHECK_ARG(V_out >= 0 && V_in >= 0 && Vpad >= V_out && Vpad % WG_TILE == 0, "Vpad must be a multiple of 128 >= V_out");
  SV_CHECK_ARG(in_ld >= Cin && dy_ld >= Cout, "row strides too small");
  SV_CHECK_ARG(dW, "null pointer");
  const bool has_plan = perm || nbr_s || submask;
  SV_CHECK_ARG(!has_plan || (perm && nbr_s && submask), "perm, nbr_s and submask must be given together");
  SV_CHECK_ARG(has_plan || K == 1, "K > 1 needs a plan");
  SV_CHECK_ARG(!has_plan || ((((uintptr_t)perm | (uintptr_t)nbr_s | (uintptr_t)submask) & 3) == 0),
               "plan arrays must be 4-byte aligned");
  const int64_t n = (int64_t)K * Cin * Cout;
  if (V_out == 0 || Vpad == 0) {  // no pairs: dW = 0 (or unchanged when accumulating)
    if (!accumulate) SV_HIP(hipMemsetAsync(dW, 0, (size_t)n * sizeof(float), stream));
    return SV_OK;
  }
  SV_CHECK_ARG(in && dy, "null pointer");
  SV_CHECK_ARG(V_in >= 1, "V_in = rows of `in` (every index of the plan is below it)");
  SV_CHECK_ARG(workspace || workspace_bytes == 0, "null pointer");
  if (workspace_bytes < sv_conv_wgrad_workspace_bytes(Vpad, K, Cin, Cout)) {
    set_error("sv_conv_wgrad: workspace too small (%zu < %zu bytes)", workspace_bytes,
              sv_conv_wgrad_workspace_bytes(Vpad, K, Cin, Cout));
    return SV_ERR_WORKSPACE;
  }
  WgradParams p;
  p.in = in; p.V_in = V_in; p.in_ld = in_ld; p.Cin = Cin;
  p.dy = dy; p.V_out = V_out; p.dy_ld = dy_ld; p.Cout = Cout; p.K = K;
  p.perm = perm; p.nbr_s = nbr_s; p.submask = submask; p.Vpad = Vpad;
  p.ntiles = (int)(Vpad / WG_TILE);
  p.chunks = wgrad_chunks(Vpad, K, Cin, Cout);
  p.tiles_per_chunk = (p.ntiles + p.chunks - 1) / p.chunks;
  p.chunks = (p.ntiles + p.tiles_per_chunk - 1) / p.tiles_per_chunk;  // no empty trailing chunk
  p.vec_a = in_ld % 4 == 0 && Cin % 4 == 0 && ((uintptr_t)in & 15) == 0;
  p.vec_b = dy_ld % 4 == 0 && Cout % 4 == 0 && ((uintptr_t)dy & 15) == 0;
  p.part = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  const int nblk = ((Cin + BC - 1) / BC) * ((Cout + BN - 1) / BN);
  hipLaunchKernelGGL(wgrad_kernel, dim3(nblk, K, p.chunks), dim3(256), 0, stream, p);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p.part, p.chunks, n,
                     accumulate, dW);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
