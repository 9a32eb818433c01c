// A8: PointNet++ set abstraction (eval mode) as ONE launch: group gather -> shared MLP -> max over the group.
//
//  sv_pointnet_sa <- model/pointnet2_utils.py:178-204 PointNetSetAbstraction.forward: the grouped tensor of
//                    sample_and_group (:112-140, [xyz[idx] - new_xyz, points[idx]]), Conv2d 1x1 + BatchNorm2d + ReLU per
//                    layer, torch.max over the nsample neighbours.  The unfused eval path runs the same layers as dense
//                    rows through sv_conv_fwd (one launch per layer, every intermediate in HBM) plus a torch gather / cat /
//                    max; here a workgroup keeps all of it in LDS and writes only the pooled [S][C_last] rows.
//  sv_pointnet_sa_msg <- model/pointnet2_utils.py:207-264 PointNetSetAbstractionMsg.forward: the R scales of one
//                    multi-scale layer (grouping [points[idx], xyz[idx] - new_xyz], :247-250; nsample up to 128) in one
//                    launch, every scale's pooled rows written into its columns of the concatenated output (:262).
// Both entries run one kernel body, pointnet_sa_kernel<MSG>: single-scale is its one-scale, one-pass instance in the
// SV_GROUP_SSG row layout.  The grouped element itself (pn_group_element, sv_pointnet_dev.h) is sv_group_rows' too.
//
// Work decomposition
//   * a workgroup (4 waves) owns PN_ROWS = 64 rows = 64 / nsample centroids x nsample neighbours;
//   * it gathers the rows into LDS (input channels zero-padded to a multiple of 4), then runs the layers one after
//     another, ping-ponging between two LDS buffers; row strides are 4 * odd floats, so the 16 rows x 4 k of a
//     v_mfma_f32_16x16x4_f32 A operand read hit 64 distinct banks;
//   * per layer, a wave owns (16 * MR rows) x (16 * NT channels) units: A from LDS, B (weights) straight from L2 into
//     registers, MR * NT independent accumulators;
//   * the last layer never leaves the chip: ReLU, max over each 16-row sub-tile (registers + two lane shuffles) into
//     LDS, then max over the sub-tiles of a centroid, written as out[centroid][c].
// Numerics: every output element is ONE f32 fma chain over the input channels ascending, starting at 0 (the f32 MFMA is a
// k-ordered fmaf chain), then fmaf(acc, scale, shift) and ReLU: the arithmetic of sv_conv_fwd's dense rows, so the result is
// bit-identical to the unfused eval path on the same groups.  Zero-padded channels add fma(0, 0, acc) = acc.
#include <atomic>

#include "sv_common.h"
#include "sv_pointnet_dev.h"

namespace sv {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int PN_ROWS = 64;
constexpr int PN_THREADS = 256;
constexpr size_t PN_LDS_MAX = 160 * 1024;  // LDS of one CU (MI355X): one workgroup per CU at the largest shapes

// smallest row stride >= c that is 4 * odd (see the header comment)
static inline int pn_stride(int c) {
  int s = (c + 3) / 4 * 4;
  if ((s / 4) % 2 == 0) s += 4;
  return s;
}

struct PnLayer {
  int cin, kpad, cout;
  int sa_in, sa_out;  // LDS row strides of the layer's input and output
  int64_t w, scale, shift;  // offsets into the packed parameter buffer (floats)
};

// One scale: a ball (group_idx, nsample), its layers and parameters, and where its work and its output sit in the launch.
struct PnScale {
  const int64_t* idx;
  const float* params;
  int nsample, L, col;  // col: first column of the scale in the [B][S][ctot] output
  int buf1;  // float offset of the scale's second LDS buffer
  int run;   // float offset of the running maxima (two-pass balls)
  int64_t blk0;  // first workgroup of the scale
  PnLayer layer[SV_PN_MAX_LAYERS];
};

template <int MAXR>
struct PnParams {
  const float* xyz;
  const float* points;
  const float* new_xyz;
  float* out;
  int N, S, D, R, ctot;
  int64_t nq;  // B * S
  PnScale sc[MAXR];
};

template <int MR, int NT>
__device__ __forceinline__ void pn_layer(const float* __restrict__ params, const PnLayer& ly,
                                         const float* __restrict__ in_s, float* __restrict__ out_s, const bool last,
                                         const int wave, const int lane) {
  constexpr int RG = 4 / MR;  // row groups of the 64-row tile
  const int li = lane & 15, lq = lane >> 4;
  const float* __restrict__ W = params + ly.w;
  const float* __restrict__ scale = params + ly.scale;
  const float* __restrict__ shift = params + ly.shift;
  const int units = ly.cout / (16 * NT) * RG;
  for (int u = wave; u < units; u += PN_THREADS / 64) {
    const int rg = u % RG, cg = u / RG;
    const int r0 = rg * MR * 16, c0 = cg * NT * 16;
    f32x4 acc[MR][NT];
#pragma unroll
    for (int s = 0; s < MR; ++s)
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[s][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* __restrict__ wp = W + c0 + li;
    const float* __restrict__ ap = in_s + (r0 + li) * ly.sa_in + lq;
    int k0 = 0;
    // four k-steps per round: their weight loads are issued together, ahead of the matrix ops
    for (; k0 + 16 <= ly.kpad; k0 += 16) {
      float b[4][NT];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + 4 * j + lq;
#pragma unroll
        for (int n = 0; n < NT; ++n) b[j][n] = k < ly.cin ? wp[(int64_t)k * ly.cout + n * 16] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float a[MR];
#pragma unroll
        for (int s = 0; s < MR; ++s) a[s] = ap[s * 16 * ly.sa_in + k0 + 4 * j];
#pragma unroll
        for (int s = 0; s < MR; ++s)
#pragma unroll
          for (int n = 0; n < NT; ++n) acc[s][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[j][n], acc[s][n], 0, 0, 0);
      }
    }
    for (; k0 < ly.kpad; k0 += 4) {
      const int k = k0 + lq;
      float b[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) b[n] = k < ly.cin ? wp[(int64_t)k * ly.cout + n * 16] : 0.f;
#pragma unroll
      for (int s = 0; s < MR; ++s) {
        const float a = ap[s * 16 * ly.sa_in + k0];
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[s][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[n], acc[s][n], 0, 0, 0);
      }
    }
    // epilogue: C/D map of the 16x16x4 op - column = lane & 15, row = 4 * (lane >> 4) + reg
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int c = c0 + n * 16 + li;
      const float sc = scale[c], sh = shift[c];
#pragma unroll
      for (int s = 0; s < MR; ++s) {
        float v[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const float y = __builtin_fmaf(acc[s][n][reg], sc, sh);
          v[reg] = y < 0.f ? 0.f : y;  // NaN stays NaN, as torch.relu
        }
        if (!last) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) out_s[(r0 + s * 16 + lq * 4 + reg) * ly.sa_out + c] = v[reg];
        } else {
          // max over the sub-tile's 16 rows (NaN propagates, as torch.max)
          float m = v[0];
#pragma unroll
          for (int reg = 1; reg < 4; ++reg) m = (v[reg] > m || v[reg] != v[reg]) ? v[reg] : m;
#pragma unroll
          for (int d = 16; d <= 32; d <<= 1) {
            const float o = __shfl_xor(m, d);
            m = (o > m || o != o) ? o : m;
          }
          if (lq == 0) out_s[(r0 / 16 + s) * ly.cout + c] = m;  // partial maxima [4 sub-tiles][cout]
        }
      }
    }
  }
}

template <int MR, int NT>
__device__ __forceinline__ void pn_layer_nt(const float* params, const PnLayer& ly, const float* in_s, float* out_s,
                                            bool last, int wave, int lane) {
  pn_layer<MR, NT>(params, ly, in_s, out_s, last, wave, lane);
}

__device__ __forceinline__ void pn_layer_any(const float* params, const PnLayer& ly, const float* in_s, float* out_s,
                                             bool last, int wave, int lane) {
  // widest units that still give every wave work: NT = 2 column tiles when Cout % 32 == 0, MR = 4 row sub-tiles
  // when there are at least four column groups (else the rows are split between the waves)
  const int nt = ly.cout % 32 == 0 ? 2 : 1;
  const int cgroups = ly.cout / (16 * nt);
  if (nt == 2) {
    if (cgroups >= 4) pn_layer_nt<4, 2>(params, ly, in_s, out_s, last, wave, lane);
    else if (cgroups >= 2) pn_layer_nt<2, 2>(params, ly, in_s, out_s, last, wave, lane);
    else pn_layer_nt<1, 2>(params, ly, in_s, out_s, last, wave, lane);
  } else {
    if (cgroups >= 4) pn_layer_nt<4, 1>(params, ly, in_s, out_s, last, wave, lane);
    else if (cgroups >= 2) pn_layer_nt<2, 1>(params, ly, in_s, out_s, last, wave, lane);
    else pn_layer_nt<1, 1>(params, ly, in_s, out_s, last, wave, lane);
  }
}

// The set abstraction of R scales over the same centroids in ONE launch.  Workgroups blk0[r] .. blk0[r + 1] - 1 serve
// scale r, each with its own ball (group_idx_r, nsample_r), layers and parameters; LDS is sized for the largest scale.
// A ball of up to 64 neighbours is one pass of 64 / nsample centroids per workgroup; nsample 128 is one centroid in two
// 64-row passes: pass 0's per-channel maxima wait in LDS (`run`, [C_last]) and pass 1 folds its own into them with the
// same NaN-propagating rule.  Scale r writes its pooled rows into columns col_r .. col_r + C_r of the [B][S][sum C_r]
// output (no cat).
//   MSG = false (sv_pointnet_sa): one scale in the row layout SV_GROUP_SSG, one pass - the scale lookup and the pass
//   loop fold away at compile time, which keeps this instance's registers (and so its occupancy) below the other's;
//   MSG = true (sv_pointnet_sa_msg): up to SV_PN_MAX_SCALES scales in the row layout SV_GROUP_MSG, one or two passes.
template <bool MSG>
__global__ __launch_bounds__(PN_THREADS) void pointnet_sa_kernel(const PnParams<MSG ? SV_PN_MAX_SCALES : 1> p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int r = 0;
  if (MSG)
    while (r + 1 < p.R && (int64_t)blockIdx.x >= p.sc[r + 1].blk0) ++r;
  const PnScale& sc = p.sc[r];
  float* bufs[2] = {lds, lds + sc.buf1};
  float* run = lds + sc.run;
  const int ns = sc.nsample;
  const int rows_c = MSG && ns > PN_ROWS ? PN_ROWS : ns;  // rows of one centroid in one pass
  const int tc = PN_ROWS / rows_c;                         // centroids per workgroup
  const int npass = MSG ? ns / rows_c : 1;
  const int64_t q0 = ((int64_t)blockIdx.x - (MSG ? sc.blk0 : 0)) * tc;
  const int cout = sc.layer[sc.L - 1].cout;
  const int nsub = rows_c / 16;
  __builtin_assume(sc.idx != nullptr);  // the entry points check it: pn_group_element's group_all branch is not built
  for (int pass = 0; pass < npass; ++pass) {
    // ---- gather: row rr = (centroid q0 + rr / rows_c, neighbour pass * rows_c + rr % rows_c), zero-padded to kpad
    {
      const PnLayer& l0 = sc.layer[0];
      const int c_real = p.D + 3;
      for (int e = tid; e < PN_ROWS * l0.kpad; e += PN_THREADS) {
        const int rr = e / l0.kpad, c = e - rr * l0.kpad;
        const int64_t q = q0 + rr / rows_c;
        float v = 0.f;
        if (q < p.nq && c < c_real)
          v = pn_group_element(p.xyz, p.points, p.new_xyz, sc.idx, q / p.S, q, pass * rows_c + rr % rows_c, ns, p.N, p.D,
                               MSG ? SV_GROUP_MSG : SV_GROUP_SSG, c);
        bufs[0][rr * l0.sa_in + c] = v;
      }
    }
    __syncthreads();
    // ---- layers: layer l reads bufs[l & 1], writes bufs[(l + 1) & 1]
    for (int l = 0; l < sc.L; ++l) {
      pn_layer_any(sc.params, sc.layer[l], bufs[l & 1], bufs[(l + 1) & 1], l == sc.L - 1, wave, lane);
      __syncthreads();
    }
    // ---- max over the sub-tiles of each centroid (and over the passes of a two-pass ball)
    const float* part = bufs[sc.L & 1];
    for (int e = tid; e < tc * cout; e += PN_THREADS) {
      const int cl = e / cout, c = e - cl * cout;
      const int64_t q = q0 + cl;
      if (q >= p.nq) continue;
      float m = part[(cl * nsub) * cout + c];
      for (int j = 1; j < nsub; ++j) {
        const float o = part[(cl * nsub + j) * cout + c];
        m = (o > m || o != o) ? o : m;
      }
      if (pass + 1 < npass) {
        if (pass > 0) {
          const float o = run[c];
          m = (m > o || m != m) ? m : o;
        }
        run[c] = m;  // tc == 1 for a multi-pass ball
      } else {
        if (pass > 0) {
          const float o = m;
          m = run[c];
          m = (o > m || o != o) ? o : m;
        }
        p.out[q * p.ctot + sc.col + c] = m;
      }
    }
    if (pass + 1 < npass) __syncthreads();  // the next gather overwrites bufs[0]
  }
}

}  // namespace sv

using namespace sv;

// hipFuncSetAttribute acts on the current device: remembered per device ordinal, not once per process
static int pn_allow_lds(const void* fn, std::atomic<bool>* done, int ndone) {
  int dev = 0;
  SV_HIP(hipGetDevice(&dev));
  if (dev < ndone && done[dev].load(std::memory_order_acquire)) return SV_OK;
  SV_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PN_LDS_MAX));
  if (dev < ndone) done[dev].store(true, std::memory_order_release);
  return SV_OK;
}

// Layer table and LDS plan of one shared MLP on the 64-row tile.  Buffer 0 holds the gathered input and the outputs of
// layers 1, 3; buffer 1 those of layers 0, 2; the partial maxima of the last layer ([4][C_last]) go to the buffer the last
// layer does not read.  Returns SV_OK or SV_ERR_UNSUPPORTED (message set) for widths the kernel does not cover.
static int pn_plan(const char* fn, const int* widths, int L, PnLayer* layer, int64_t need[2]) {
  for (int l = 1; l <= L; ++l)
    if (widths[l] < 16 || widths[l] % 16 != 0 || widths[l] > 1024) {
      set_error("%s: %s", fn, "layer widths must be multiples of 16 in 16..1024");
      return SV_ERR_UNSUPPORTED;
    }
  need[0] = need[1] = 0;
  int64_t off = 0;
  for (int l = 0; l < L; ++l) {
    PnLayer& ly = layer[l];
    ly.cin = widths[l];
    ly.kpad = (widths[l] + 3) / 4 * 4;
    ly.cout = widths[l + 1];
    ly.sa_in = pn_stride(ly.kpad);
    ly.sa_out = l + 1 < L ? pn_stride(ly.cout) : 0;
    ly.w = off;
    off += (int64_t)ly.cin * ly.cout;
    ly.scale = off;
    off += ly.cout;
    ly.shift = off;
    off += ly.cout;
    if (l == 0) need[0] = (int64_t)PN_ROWS * ly.sa_in;
    const int64_t o = l + 1 < L ? (int64_t)PN_ROWS * ly.sa_out : 4 * (int64_t)ly.cout;
    if (o > need[(l + 1) & 1]) need[(l + 1) & 1] = o;
  }
  for (int l = 1; l < L; ++l) layer[l].sa_in = layer[l - 1].sa_out;
  return SV_OK;
}

// Validates and plans one scale (widths [L + 1], ns neighbours, over nq centroids of D features) for entry point fn, which
// takes balls of up to max_ns neighbours: fills sc but for its device pointers and appends the scale to the launch - its
// columns to ctot, its workgroups to blocks, its LDS need to lds_bytes (the maximum over the scales).
static int pn_plan_scale(const char* fn, int max_ns, const int* widths, int L, int ns, int D, int64_t nq, PnScale& sc,
                         int& ctot, int64_t& blocks, size_t& lds_bytes) {
  const bool msg = max_ns > PN_ROWS;
  if (L < 1 || L > SV_PN_MAX_LAYERS) {
    set_error("%s: %s", fn, "layer count outside 1..SV_PN_MAX_LAYERS");
    return SV_ERR_UNSUPPORTED;
  }
  if (widths[0] != 3 + D) {
    set_error("%s: %s", fn, msg ? "widths[0] of every scale must be 3 + D" : "widths[0] must be 3 + D");
    return SV_ERR_INVALID;
  }
  if ((ns != 16 && ns != 32 && ns != 64 && ns != 128) || ns > max_ns) {
    set_error("%s: %s", fn, msg ? "nsample must be 16, 32, 64 or 128" : "nsample must be 16, 32 or 64");
    return SV_ERR_UNSUPPORTED;
  }
  int64_t need[2];
  const int rc = pn_plan(fn, widths, L, sc.layer, need);
  if (rc != SV_OK) return rc;
  const int64_t cout = widths[L];
  const int64_t floats = need[0] + need[1] + (ns > PN_ROWS ? cout : 0);  // + running maxima of a two-pass ball
  const size_t bytes = (size_t)floats * sizeof(float);
  if (bytes > PN_LDS_MAX) {
    set_error("%s: %s", fn, "layer widths exceed the LDS of one CU");
    return SV_ERR_UNSUPPORTED;
  }
  if (bytes > lds_bytes) lds_bytes = bytes;
  sc.nsample = ns; sc.L = L; sc.col = ctot;
  sc.buf1 = (int)need[0];
  sc.run = (int)(need[0] + need[1]);
  ctot += (int)cout;
  const int tc = PN_ROWS / (ns < PN_ROWS ? ns : PN_ROWS);
  sc.blk0 = blocks;
  blocks += (nq + tc - 1) / tc;
  return SV_OK;
}

template <bool MSG, int MAXR>
static int pn_launch(const PnParams<MAXR>& p, int64_t blocks, size_t lds_bytes, hipStream_t stream) {
  static std::atomic<bool> attr_set[64];
  const int arc = pn_allow_lds((const void*)pointnet_sa_kernel<MSG>, attr_set, 64);
  if (arc != SV_OK) return arc;
  hipLaunchKernelGGL(pointnet_sa_kernel<MSG>, dim3((unsigned)blocks), dim3(PN_THREADS), lds_bytes, stream, p);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_pointnet_sa(const float* xyz, const float* points, const float* new_xyz, const int64_t* group_idx, int B,
                              int N, int D, int S, int nsample, const float* params, const int* widths, int L, float* out,
                              sv_stream_t stream_) {
  SV_CHECK_ARG(B >= 0 && N >= 1 && S >= 1 && D >= 0, "bad shape");
  SV_CHECK_ARG(widths, "null pointer");
  PnParams<1> p;
  p.N = N; p.S = S; p.D = D; p.R = 1; p.ctot = 0;
  p.nq = (int64_t)B * S;
  size_t lds_bytes = 0;
  int64_t blocks = 0;
  const int rc = pn_plan_scale(__func__, 64, widths, L, nsample, D, p.nq, p.sc[0], p.ctot, blocks, lds_bytes);
  if (rc != SV_OK) return rc;
  if (B == 0) return SV_OK;
  SV_CHECK_ARG(xyz && new_xyz && group_idx && params && out && (D == 0 || points), "null pointer");
  SV_CHECK_ARG(blocks < (1ll << 31), "too many centroids");
  p.xyz = xyz; p.points = points; p.new_xyz = new_xyz; p.out = out;
  p.sc[0].idx = group_idx;
  p.sc[0].params = params;
  return pn_launch<false>(p, blocks, lds_bytes, (hipStream_t)stream_);
}

extern "C" int sv_pointnet_sa_msg(const float* xyz, const float* points, const float* new_xyz, int B, int N, int D, int S,
                                  int R, const int* nsamples, const int64_t* const* group_idx,
                                  const float* const* params, const int* widths, const int* nlayers, float* out,
                                  sv_stream_t stream_) {
  SV_CHECK_ARG(B >= 0 && N >= 1 && S >= 1 && D >= 0, "bad shape");
  SV_CHECK_ARG(nsamples && group_idx && params && widths && nlayers, "null pointer");
  if (R < 1 || R > SV_PN_MAX_SCALES) {
    set_error("%s: %s", __func__, "scale count outside 1..SV_PN_MAX_SCALES");
    return SV_ERR_UNSUPPORTED;
  }
  PnParams<SV_PN_MAX_SCALES> p;
  p.N = N; p.S = S; p.D = D; p.R = R; p.ctot = 0;
  p.nq = (int64_t)B * S;
  size_t lds_bytes = 0;
  int64_t blocks = 0;
  for (int r = 0, wofs = 0; r < R; wofs += nlayers[r] + 1, ++r) {
    const int rc = pn_plan_scale(__func__, 128, widths + wofs, nlayers[r], nsamples[r], D, p.nq, p.sc[r], p.ctot, blocks,
                                 lds_bytes);
    if (rc != SV_OK) return rc;
  }
  if (B == 0) return SV_OK;
  SV_CHECK_ARG(xyz && new_xyz && out && (D == 0 || points), "null pointer");
  for (int r = 0; r < R; ++r) {
    SV_CHECK_ARG(group_idx[r] && params[r], "null pointer");
    p.sc[r].idx = group_idx[r];
    p.sc[r].params = params[r];
  }
  SV_CHECK_ARG(blocks < (1ll << 31), "too many centroids");
  p.xyz = xyz; p.points = points; p.new_xyz = new_xyz; p.out = out;
  return pn_launch<true>(p, blocks, lds_bytes, (hipStream_t)stream_);
}
