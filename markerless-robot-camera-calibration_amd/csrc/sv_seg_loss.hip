// N7: the criterion and the per-step metrics of train_segmentation.py / train_vote.py / train_key_points.py
// (nn.CrossEntropyLoss with ignore_index on out.features [N, C]; compute_accuracies; the top 8 votes per frame of
// compute_center_dists) for a whole batch.  torch runs log-softmax, NLL and their backwards as four passes over [N, C]
// and the trainers add one arg-max pass and one host wait per frame; here one pass over the logits gives the loss sum,
// the unscaled gradient and the per-frame confusion counts, with no host wait.  The contract is in include/sv_hip.h.
//
//   seg_zero_kernel       zeroes the integer outputs (confusion, n_rows_ignored, n_invalid)
//   seg_criterion_kernel  workgroup g of G = min(tiles, SEG_MAX_GROUPS) owns the contiguous tiles [g T, (g + 1) T),
//                         T = ceil(tiles / G), of SEG_TILE rows each.  A tile's logits enter LDS by a flat, coalesced
//                         copy (rows are 4 to 128 bytes: a thread-per-row global read would touch one cache line per
//                         lane and column); thread r then walks row r of the tile in float64 (LDS row stride C | 1: odd,
//                         no bank conflict), writes the row's gradient back into the tile, and the tile leaves by the
//                         same flat copy.  Confusion cells of the frame that owns the tile's first row are counted in
//                         LDS and flushed with one global atomic per non-zero cell; rows of a later frame (a frame
//                         boundary inside the tile) add to global memory directly.  Every thread adds its rows' losses
//                         in tile order; lanes by shuffles, waves through LDS in wave order: one (sum, count) per
//                         workgroup.
//   seg_finish_kernel     one workgroup adds the G partials: thread t takes t, t + 256, ... ascending, then shuffles
//                         and wave order again.
//   segtopk_select_kernel<false>  workgroup (j, b) selects the k largest keys of chunk j of frame b (topk_key of
//                         sv_common.h on the row within the frame: sv_topk_indices' order); <true>: one workgroup per
//                         frame selects the k largest of its chunks' candidates and writes the indices.
// Float sums use no atomics and an order fixed by (N, B, C); the integer counts use LDS and global integer atomics.
#include "sv_common.h"

namespace sv {

constexpr int SEG_BLOCK = 256;
constexpr int SEG_TILE = 256;         // rows per tile: one per thread
constexpr int SEG_MAX_GROUPS = 512;   // workgroups of one launch; N > SEG_TILE * SEG_MAX_GROUPS rows: several tiles each
constexpr int SEG_MAX_C = 32;
constexpr int SEGTOPK_CHUNK = 4096;   // rows per stage-1 workgroup

// frame of row i: the largest b with offsets[b] <= i, provided offsets[0] <= i < offsets[B]; -1: no frame owns the row.
// Whatever `offsets` holds the result is in [-1, B).
__device__ __forceinline__ int seg_frame_of(const int32_t* __restrict__ offsets, int B, int64_t i) {
  if (i < offsets[0] || i >= offsets[B]) return -1;
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void seg_zero_kernel(int64_t* __restrict__ confusion, int64_t n_conf,
                                                        int64_t* __restrict__ n_rows_ignored, int B,
                                                        int32_t* __restrict__ n_invalid) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (confusion && t < n_conf) confusion[t] = 0;
  if (n_rows_ignored && t < B) n_rows_ignored[t] = 0;
  if (t == 0) n_invalid[0] = 0;
}

__global__ __launch_bounds__(SEG_BLOCK) void seg_criterion_kernel(
    const float* __restrict__ logits, int64_t ld, int C, int64_t N, const int64_t* __restrict__ labels,
    int64_t ignore_index, const int32_t* __restrict__ offsets, int B, int64_t tiles, int64_t tiles_per_group,
    double* __restrict__ partial, float* __restrict__ grad, unsigned long long* __restrict__ confusion,
    unsigned long long* __restrict__ n_rows_ignored, int32_t* __restrict__ n_invalid) {
  __shared__ float tile[SEG_TILE * (SEG_MAX_C + 1)];
  __shared__ int hist[SEG_MAX_C * SEG_MAX_C + 1];  // [gt][pred] of the tile's first frame, then its ignored rows
  __shared__ int tile_frame;
  __shared__ double red[SEG_BLOCK / 64][2];
  const int Cp = C | 1;
  const int cells = C * C + 1;
  const bool counts = confusion || n_rows_ignored;
  double loss_sum = 0.0, n_counted = 0.0;
  const int64_t t0 = (int64_t)blockIdx.x * tiles_per_group;
  const int64_t t1 = t0 + tiles_per_group < tiles ? t0 + tiles_per_group : tiles;
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t row0 = t * SEG_TILE;
    const int rows = (int)(N - row0 < SEG_TILE ? N - row0 : SEG_TILE);
    for (int e = threadIdx.x; e < rows * C; e += SEG_BLOCK) {
      const int r = e / C, c = e - r * C;
      tile[r * Cp + c] = logits[(row0 + r) * ld + c];
    }
    if (counts) {
      for (int e = threadIdx.x; e < cells; e += SEG_BLOCK) hist[e] = 0;
    }
    const int r = threadIdx.x;
    const int frame = r < rows ? seg_frame_of(offsets, B, row0 + r) : -1;
    if (r == 0) tile_frame = frame;
    __syncthreads();
    if (r < rows) {
      float* x = tile + r * Cp;
      float best = x[0];
      int pred = 0;
      for (int c = 1; c < C; ++c) {
        const float v = x[c];
        if (v > best || (v != v && best == best)) {  // torch's max(1), the rule of sv_slice_argmax
          best = v;
          pred = c;
        }
      }
      const int64_t y = labels[row0 + r];
      if (y == ignore_index) {
        for (int c = 0; c < C; ++c) x[c] = 0.0f;
        if (n_rows_ignored && frame >= 0) {
          if (frame == tile_frame) atomicAdd(&hist[C * C], 1);
          else atomicAdd(&n_rows_ignored[frame], 1ull);
        }
      } else if (y < 0 || y >= C) {
        for (int c = 0; c < C; ++c) x[c] = NAN;
        atomicAdd(n_invalid, 1);
      } else {
        // lse = m + log(sum exp(x_c - m)) in float64; a NaN maximum or inf - inf makes every term NaN
        const double m = (double)best;
        double s = 0.0, others = 0.0;
        for (int c = 0; c < C; ++c) {
          const double e = exp((double)x[c] - m);
          s += e;
          if (c != (int)y) others += e;
        }
        loss_sum += (m + log(s)) - (double)x[y];
        n_counted += 1.0;
        // softmax - onehot; the label's column as -(sum of the others) / s: p - 1 would cancel when p is close to 1
        for (int c = 0; c < C; ++c) {
          const double e = exp((double)x[c] - m);
          x[c] = (float)(c == (int)y ? -(others / s) : e / s);
        }
        if (confusion && frame >= 0) {
          if (frame == tile_frame) atomicAdd(&hist[(int)y * C + pred], 1);
          else atomicAdd(&confusion[((int64_t)frame * C + y) * C + pred], 1ull);
        }
      }
    }
    __syncthreads();
    if (grad) {
      for (int e = threadIdx.x; e < rows * C; e += SEG_BLOCK) {
        const int rr = e / C, c = e - rr * C;
        grad[(row0 + rr) * C + c] = tile[rr * Cp + c];
      }
    }
    if (counts && tile_frame >= 0) {
      for (int e = threadIdx.x; e < cells; e += SEG_BLOCK) {
        const int v = hist[e];
        if (v == 0) continue;
        if (e < C * C) atomicAdd(&confusion[(int64_t)tile_frame * C * C + e], (unsigned long long)v);
        else atomicAdd(&n_rows_ignored[tile_frame], (unsigned long long)v);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    loss_sum += __shfl_xor(loss_sum, d);
    n_counted += __shfl_xor(n_counted, d);
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = loss_sum;
    red[threadIdx.x >> 6][1] = n_counted;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    double v = 0.0;
    for (int w = 0; w < SEG_BLOCK / 64; ++w) v += red[w][threadIdx.x];  // wave order
    partial[(int64_t)blockIdx.x * 2 + threadIdx.x] = v;
  }
}

__global__ __launch_bounds__(SEG_BLOCK) void seg_finish_kernel(const double* __restrict__ partial, int groups,
                                                               double* __restrict__ sums) {
  __shared__ double red[SEG_BLOCK / 64][2];
  double a = 0.0, n = 0.0;
  for (int g = threadIdx.x; g < groups; g += SEG_BLOCK) {  // ascending workgroup order
    a += partial[g * 2];
    n += partial[g * 2 + 1];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    a += __shfl_xor(a, d);
    n += __shfl_xor(n, d);
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = a;
    red[threadIdx.x >> 6][1] = n;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    double v = 0.0;
    for (int w = 0; w < SEG_BLOCK / 64; ++w) v += red[w][threadIdx.x];
    sums[threadIdx.x] = v;
  }
}

static inline int64_t seg_tiles(int64_t N) { return (N + SEG_TILE - 1) / SEG_TILE; }
static inline int64_t seg_groups(int64_t N) {
  const int64_t t = seg_tiles(N);
  return t < SEG_MAX_GROUPS ? t : SEG_MAX_GROUPS;
}

// rows of frame b clamped into [0, N] with hi >= lo, as the loss and label entries do
__device__ __forceinline__ void segtopk_frame_rows(const int32_t* __restrict__ offsets, int b, int64_t N, int64_t& lo,
                                                   int64_t& hi) {
  lo = offsets[b] < 0 ? 0 : (offsets[b] > N ? N : offsets[b]);
  hi = offsets[b + 1] < lo ? lo : (offsets[b + 1] > N ? N : offsets[b + 1]);
}

// FINAL false: grid (chunks, B); workgroup (j, b) writes the k largest keys of rows [j CHUNK, (j + 1) CHUNK) of frame b to
// cand[b][j][k] (0 = nothing left); a chunk past the frame's end writes nothing and is never read.
// FINAL true: grid (B); the k largest of the frame's ceil(len / CHUNK) * k candidates become idx[b][k].
template <bool FINAL>
__global__ __launch_bounds__(256) void segtopk_select_kernel(const float* __restrict__ x, int64_t ld, int64_t N,
                                                              const int32_t* __restrict__ offsets, int k, int64_t chunks,
                                                              unsigned long long* __restrict__ cand,
                                                              int64_t* __restrict__ idx) {
  __shared__ unsigned long long wave_best[4];
  __shared__ unsigned long long chosen;
  const int b = FINAL ? blockIdx.x : blockIdx.y;
  int64_t lo, hi;
  segtopk_frame_rows(offsets, b, N, lo, hi);
  const int64_t len = hi - lo;
  int64_t first, end;  // FINAL: candidate slots of the frame; else rows within the frame
  if (FINAL) {
    first = 0;
    end = (len + SEGTOPK_CHUNK - 1) / SEGTOPK_CHUNK * k;
  } else {
    first = (int64_t)blockIdx.x * SEGTOPK_CHUNK;
    if (first >= len) return;  // uniform over the workgroup
    end = first + SEGTOPK_CHUNK < len ? first + SEGTOPK_CHUNK : len;
  }
  const unsigned long long* keys_in = cand + (int64_t)b * chunks * k;
  unsigned long long* keys_out = cand + ((int64_t)b * chunks + (FINAL ? 0 : blockIdx.x)) * k;
  unsigned long long prev = ~0ull;
  for (int j = 0; j < k; ++j) {
    unsigned long long best = 0ull;  // key 0 = nothing left (a real key has value bits != 0)
    if (prev != 0ull) {
      for (int64_t i = first + threadIdx.x; i < end; i += 256) {
        const unsigned long long key = FINAL ? keys_in[i] : topk_key(x[(lo + i) * ld], (unsigned)i);
        if (key < prev && key > best) best = key;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const unsigned long long o = __shfl_xor(best, off, 64);
      best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0) wave_best[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long v = wave_best[0];
      for (int w = 1; w < 4; ++w) v = wave_best[w] > v ? wave_best[w] : v;
      chosen = v;
      if (FINAL) idx[(int64_t)b * k + j] = v ? (int64_t)(0xffffffffu - (unsigned)(v & 0xffffffffull)) : -1;
      else keys_out[j] = v;
    }
    __syncthreads();
    prev = chosen;  // 0 once the rows run out: the remaining slots are 0 (idx -1)
  }
}

static inline int64_t segtopk_chunks(int64_t N) { return N <= 0 ? 1 : (N + SEGTOPK_CHUNK - 1) / SEGTOPK_CHUNK; }

}  // namespace sv

using namespace sv;

extern "C" {

size_t sv_seg_criterion_workspace_bytes(int64_t N, int B, int C) {
  (void)B;
  (void)C;
  if (N < 0) N = 0;
  return align_up((size_t)(seg_groups(N) > 0 ? seg_groups(N) : 1) * 2 * sizeof(double), 256) + 256;
}

int sv_seg_criterion(const float* logits, int64_t ld, int C, int64_t N, const int64_t* labels, int64_t ignore_index,
                     const int32_t* offsets, int B, void* workspace, size_t workspace_bytes, double* sums, float* grad,
                     int64_t* confusion, int64_t* n_rows_ignored, int32_t* n_invalid, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(C >= 1 && C <= SEG_MAX_C, "need 1 <= C <= 32 classes");
  SV_CHECK_ARG(ld >= C, "need ld >= C");
  SV_CHECK_ARG(B >= 1 && B <= SV_MAX_BATCH, "need 1 to 1024 frames");
  SV_CHECK_ARG(N >= 0 && N <= INT32_MAX, "need 0 <= N < 2^31 rows");
  SV_CHECK_ARG(((logits && labels) || N == 0) && offsets && workspace && sums && n_invalid, "null pointer");
  const int64_t groups = seg_groups(N);
  Workspace ws(workspace, workspace_bytes);
  double* partial = ws.take<double>((size_t)(groups > 0 ? groups : 1) * 2);
  SV_CHECK_ARG(ws.ok, "workspace too small");
  const int64_t n_conf = confusion ? (int64_t)B * C * C : 0;
  const int64_t n_zero = n_conf > B ? n_conf : B;
  hipLaunchKernelGGL(seg_zero_kernel, dim3((unsigned)((n_zero + 255) / 256)), dim3(256), 0, stream, confusion, n_conf,
                     n_rows_ignored, B, n_invalid);
  if (groups > 0) {
    const int64_t tiles = seg_tiles(N);
    hipLaunchKernelGGL(seg_criterion_kernel, dim3((unsigned)groups), dim3(SEG_BLOCK), 0, stream, logits, ld, C, N, labels,
                       ignore_index, offsets, B, tiles, (tiles + groups - 1) / groups, partial, grad,
                       (unsigned long long*)confusion, (unsigned long long*)n_rows_ignored, n_invalid);
  }
  hipLaunchKernelGGL(seg_finish_kernel, dim3(1), dim3(SEG_BLOCK), 0, stream, partial, (int)groups, sums);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

size_t sv_segment_topk_workspace_bytes(int64_t N, int B, int k) {
  if (B < 0) B = 0;
  if (k < 0) k = 0;
  return align_up((size_t)segtopk_chunks(N) * (size_t)B * (size_t)k * sizeof(unsigned long long), 256) + 256;
}

int sv_segment_topk(const float* x, int64_t ld, int64_t N, const int32_t* offsets, int B, int k, void* workspace,
                    size_t workspace_bytes, int64_t* idx, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_CHECK_ARG(k >= 1 && k <= 64, "need 1 <= k <= 64");
  SV_CHECK_ARG(B >= 1 && B <= SV_MAX_BATCH, "need 1 to 1024 frames");
  SV_CHECK_ARG(ld >= 1 && N >= 0 && N <= INT32_MAX, "need ld >= 1 and 0 <= N < 2^31 rows");
  SV_CHECK_ARG((x || N == 0) && offsets && workspace && idx, "null pointer");
  const int64_t chunks = segtopk_chunks(N);
  Workspace ws(workspace, workspace_bytes);
  unsigned long long* cand = ws.take<unsigned long long>((size_t)chunks * B * k);
  SV_CHECK_ARG(ws.ok, "workspace too small");
  if (N > 0)
    hipLaunchKernelGGL(segtopk_select_kernel<false>, dim3((unsigned)chunks, (unsigned)B), dim3(256), 0, stream, x, ld, N,
                       offsets, k, chunks, cand, nullptr);
  hipLaunchKernelGGL(segtopk_select_kernel<true>, dim3((unsigned)B), dim3(256), 0, stream, nullptr, 0, N, offsets, k,
                     chunks, cand, idx);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

}  // extern "C"
