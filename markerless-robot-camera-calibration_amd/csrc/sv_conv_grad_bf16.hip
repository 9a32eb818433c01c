// Weight gradient of the sparse convolution at reduced precision (include/sv_hip.h sv_conv_wgrad_bf16):
//   dW[k][c][n] = sum over plan rows r with o = perm[r] >= 0, i = nbr_s[k][r] >= 0 of  bf16(in[i][c]) * bf16(dY[o][n])
// sv_conv_wgrad's gather-GEMM per kernel offset on v_mfma_f32_16x16x32_bf16: the reduction dimension is the offset's
// (in, out) pairs, 32 per matrix op = two 16-row sub-tiles of the forward's plan.  The live sub-tiles of a chunk (submask)
// are taken two by two in plan order; a lone last one is paired with zeros.
//
// Tile: one workgroup = 4 waves = a 128 (Cin) x 128 (Cout) block of dW[k]; each wave owns a 64 x 64 quarter as 4 x 4
// accumulators.  Both operands need 8 consecutive pairs per lane (lane l: A[c = l & 15][pair 8 (l >> 4) + j],
// B[pair 8 (l >> 4) + j][n = l & 15]) while the gathered rows are row-major, so the register -> LDS pass transposes:
//   gather: thread t holds pairs 4 (t >> 5) .. +3 x channels 4 (t & 31) .. +3 of each operand (four 16-byte row loads);
//   store:  rounded to bf16 (RNE, NaN stays NaN) and written as [channel][32 pairs] (one 8-byte write per channel);
//   read:   each lane's fragment is 16 consecutive bytes of one channel row.
// The next step's rows are gathered into registers while the matrix ops of the current one run.
// Grid: (Cin blocks x Cout blocks, K, chunks of plan tiles).  Every chunk writes its partial dW to the workspace; a second
// pass sums the partials in ascending chunk order: no float atomics, two runs give the same bits.
#include "sv_common.h"

namespace sv {
namespace {

constexpr int WG_TILE = SV_TILE_ROWS;  // plan tile rows
constexpr int SUB = 16;                // rows per sub-tile (one submask bit)
constexpr int PAIRS = 32;              // pairs per matrix op (two sub-tiles)
constexpr int BC = 128;                // Cin block
constexpr int BN = 128;                // Cout block
constexpr int LDS_LD = PAIRS + 8;      // padded LDS row (80 bytes): a 16-lane fragment read touches 64 distinct banks
constexpr int MAX_K = 27;
constexpr int TARGET_WGS = 1536;
constexpr int MAX_CHUNKS = 128;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct WgradBf16Params {
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
  int ntiles, tiles_per_chunk;
  float* part;  // [chunks][K][Cin][Cout]
};

struct Stage {
  float a[16], b[16];  // [pair row j][channel e] at 4 j + e, 4 pair rows x 4 channels of each operand
};

// rows of the step: pairs 0..15 from the sub-tile at plan row r0, 16..31 from r1 (-1 = none: zeros)
__device__ __forceinline__ void gather(const WgradBf16Params& p, int k, int64_t r0, int64_t r1, int c0, int n0,
                                       Stage& s) {
  const int t = threadIdx.x;
  const int q = t >> 5, col = 4 * (t & 31);
  const int64_t base = (q >> 2) ? r1 : r0;
  const bool ca = c0 + col < p.Cin, cb = n0 + col < p.Cout;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int64_t i = -1, o = -1;
    if (base >= 0) {
      const int64_t row = base + 4 * (q & 3) + j;
      if (p.perm) {
        if (row < p.Vpad) {
          o = p.perm[row];
          i = p.nbr_s[(int64_t)k * p.Vpad + row];
        }
      } else if (row < p.V_out) {
        o = i = row;
      }
    }
    // a pair needs both rows: an absent one zeroes BOTH operands (0 * inf in the other would otherwise give NaN)
    const bool ok = o >= 0 && o < p.V_out && i >= 0 && i < p.V_in;
    float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
    if (ok && ca) va = *(const float4*)(p.in + i * p.in_ld + c0 + col);
    if (ok && cb) vb = *(const float4*)(p.dy + o * p.dy_ld + n0 + col);
    s.a[4 * j] = va.x; s.a[4 * j + 1] = va.y; s.a[4 * j + 2] = va.z; s.a[4 * j + 3] = va.w;
    s.b[4 * j] = vb.x; s.b[4 * j + 1] = vb.y; s.b[4 * j + 2] = vb.z; s.b[4 * j + 3] = vb.w;
  }
}

// channel e of the thread's 4 pair rows -> bf16 -> dst[col + e][4 q .. 4 q + 3] (the transpose)
__device__ __forceinline__ void store_t(__bf16 (*dst)[LDS_LD], const float (&v)[16], int q, int col) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const f32x4 x = {v[e], v[4 + e], v[8 + e], v[12 + e]};
    *(bf16x4*)&dst[col + e][4 * q] = __builtin_convertvector(x, bf16x4);
  }
}

__global__ void __launch_bounds__(256) wgrad_bf16_kernel(WgradBf16Params p) {
  __shared__ __attribute__((aligned(16))) __bf16 sA[BC][LDS_LD];
  __shared__ __attribute__((aligned(16))) __bf16 sB[BN][LDS_LD];
  const int nbn = (p.Cout + BN - 1) / BN;
  const int c0 = (blockIdx.x / nbn) * BC, n0 = (blockIdx.x % nbn) * BN;
  const int k = blockIdx.y;
  const int chunk = blockIdx.z;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wc = (wave >> 1) * 64, wn = (wave & 1) * 64;  // the wave's quarter of the block
  f32x4 acc[4][4];
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) acc[x][y] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int t0 = chunk * p.tiles_per_chunk;
  const int t1 = min(t0 + p.tiles_per_chunk, p.ntiles);
  // walk the sub-tiles of this chunk that hold a pair at offset k (all of them for dense rows), in plan order
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
  const int q = t >> 5, col = 4 * (t & 31);
  int64_t r0 = next(), r1 = r0 >= 0 ? next() : -1;
  Stage st;
  if (r0 >= 0) gather(p, k, r0, r1, c0, n0, st);
  while (r0 >= 0) {
    __syncthreads();  // the previous step's operands have been read
    store_t(sA, st.a, q, col);
    store_t(sB, st.b, q, col);
    __syncthreads();
    r0 = next();
    r1 = r0 >= 0 ? next() : -1;
    if (r0 >= 0) gather(p, k, r0, r1, c0, n0, st);  // in flight while the matrix ops below run
    const int li = lane & 15, kq = 8 * (lane >> 4);
    bf16x8 fa[4], fb[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) fa[x] = *(const bf16x8*)&sA[wc + 16 * x + li][kq];
#pragma unroll
    for (int y = 0; y < 4; ++y) fb[y] = *(const bf16x8*)&sB[wn + 16 * y + li][kq];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
      for (int y = 0; y < 4; ++y) acc[x][y] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[x], fb[y], acc[x][y], 0, 0, 0);
  }
  // D[i][j]: j = lane & 15, i = 4 (lane >> 4) + reg
  float* out = p.part + ((int64_t)chunk * p.K + k) * p.Cin * p.Cout;
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      const int n = n0 + wn + 16 * y + (lane & 15);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c = c0 + wc + 16 * x + 4 * (lane >> 4) + g;
        if (c < p.Cin && n < p.Cout) out[(int64_t)c * p.Cout + n] = acc[x][y][g];
      }
    }
}

// dW = (accumulate ? dW : 0) + (partial_0 + partial_1 + ... ) summed in ascending chunk order
__global__ void __launch_bounds__(256) wgrad_bf16_reduce_kernel(const float* __restrict__ part, int chunks, int64_t n,
                                                                int accumulate, float* __restrict__ dW) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  float s = part[e];
  for (int ch = 1; ch < chunks; ++ch) s += part[(int64_t)ch * n + e];
  dW[e] = accumulate ? dW[e] + s : s;
}

int wgrad_bf16_chunks(int64_t Vpad, int K, int Cin, int Cout) {
  const int64_t ntiles = Vpad / WG_TILE;
  const int64_t blocks = (int64_t)((Cin + BC - 1) / BC) * ((Cout + BN - 1) / BN) * K;
  int64_t c = (TARGET_WGS + blocks - 1) / blocks;
  if (c > MAX_CHUNKS) c = MAX_CHUNKS;
  if (c > ntiles) c = ntiles;
  return c < 1 ? 1 : (int)c;
}

}  // namespace
}  // namespace sv

extern "C" size_t sv_conv_wgrad_bf16_workspace_bytes(int64_t Vpad, int K, int Cin, int Cout) {
  if (Vpad <= 0 || K <= 0 || Cin <= 0 || Cout <= 0) return 0;
  const int64_t vp = (Vpad + sv::WG_TILE - 1) / sv::WG_TILE * sv::WG_TILE;
  return (size_t)sv::wgrad_bf16_chunks(vp, K, Cin, Cout) * (size_t)K * (size_t)Cin * (size_t)Cout * sizeof(float) + 256;
}

extern "C" int sv_conv_wgrad_bf16(const float* in, int64_t V_in, int64_t in_ld, int Cin, const float* dy, int64_t V_out,
                                  int64_t dy_ld, int Cout, int K, const int32_t* perm, const int32_t* nbr_s,
                                  const uint32_t* submask, int64_t Vpad, int accumulate, void* workspace,
                                  size_t workspace_bytes, float* dW, sv_stream_t stream_) {
  using namespace sv;
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(Cin > 0 && Cout > 0 && K >= 1 && K <= 32, "bad channel / kernel volume");
  if (Cin % 16 != 0 || Cout % 16 != 0 || K > MAX_K) {
    set_error("%s: needs Cin %% 16 == 0, Cout %% 16 == 0 and K <= 27 (got Cin %d, Cout %d, K %d): use sv_conv_wgrad",
              __func__, Cin, Cout, K);
    return SV_ERR_UNSUPPORTED;
  }
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
  if (in_ld % 4 != 0 || dy_ld % 4 != 0 || (((uintptr_t)in | (uintptr_t)dy) & 15) != 0) {
    set_error("%s: needs 16-byte aligned rows (in, dy 16-byte aligned, in_ld %% 4 == 0, dy_ld %% 4 == 0): use sv_conv_wgrad",
              __func__);
    return SV_ERR_UNSUPPORTED;
  }
  SV_CHECK_ARG(workspace || workspace_bytes == 0, "null pointer");
  if (workspace_bytes < sv_conv_wgrad_bf16_workspace_bytes(Vpad, K, Cin, Cout)) {
    set_error("sv_conv_wgrad_bf16: workspace too small (%zu < %zu bytes)", workspace_bytes,
              sv_conv_wgrad_bf16_workspace_bytes(Vpad, K, Cin, Cout));
    return SV_ERR_WORKSPACE;
  }
  WgradBf16Params p;
  p.in = in; p.V_in = V_in; p.in_ld = in_ld; p.Cin = Cin;
  p.dy = dy; p.V_out = V_out; p.dy_ld = dy_ld; p.Cout = Cout; p.K = K;
  p.perm = perm; p.nbr_s = nbr_s; p.submask = submask; p.Vpad = Vpad;
  p.ntiles = (int)(Vpad / WG_TILE);
  int chunks = wgrad_bf16_chunks(Vpad, K, Cin, Cout);
  p.tiles_per_chunk = (p.ntiles + chunks - 1) / chunks;
  chunks = (p.ntiles + p.tiles_per_chunk - 1) / p.tiles_per_chunk;  // no empty trailing chunk
  p.part = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  const int nblk = ((Cin + BC - 1) / BC) * ((Cout + BN - 1) / BN);
  hipLaunchKernelGGL(wgrad_bf16_kernel, dim3(nblk, K, chunks), dim3(256), 0, stream, p);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(wgrad_bf16_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p.part, chunks, n,
                     accumulate, dW);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
