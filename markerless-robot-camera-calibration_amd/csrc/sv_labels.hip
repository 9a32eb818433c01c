// N6: the per-frame training labels the reference synthesises from a frame's pose in utils/data.py (:58-103 get_roi_mask /
// get_ee_idx, :106-122 get_ee_cross_section_idx with utils/transformation.py:138-160, :125-335 get_closest_point /
// get_key_points / get_6_key_points, :338-342 collect_closest_points with the label write of data/alivev2.py:212-238), for
// a whole batch of frames per call.  The contract (dtype rules, tie rules, defined edge cases) is in include/sv_hip.h.
//
//   ee_mask_kernel        one point per lane: q = R^T (p - pos), six strict compares
//   key_points_kernel     one 256-thread workgroup per frame, two passes over the frame's points (recomputed per pass):
//                         pass A = the four front arg-mins and the two masked max-z of the gripper, pass B = the four back
//                         arg-mins (targets moved by pass A) and the two gripper arg-mins, then a count and an ordered
//                         ballot scan for the index the reference records for the gripper pair; thread 0 keeps the books
//   line_dist_kernel      one point per lane: distance to the line, to the workspace
//   line_topk_kernel      one workgroup per frame: rounds of block arg-min over the candidates with dist < cutoff that
//                         come after the previous pick in (dist, index) order; stops at the first round without one
//   radius_labels_kernel  one point per lane: classes from the highest down, first anchor within the radius wins
// No atomics; every reduction is a min / max under a total order, so two runs give the same bits.
#include <limits.h>

#include "sv_common.h"

namespace sv {

constexpr int LBL_BLOCK = 256;
constexpr int LBL_WAVES = LBL_BLOCK / 64;
constexpr int LBL_MAX_K = 64;  // key points per frame sv_radius_labels accepts

// rows of frame b, whatever `offsets` holds: both ends inside [0, N] and hi >= lo, so no row index leaves the arrays
__device__ __forceinline__ void lbl_frame_rows(const int32_t* __restrict__ offsets, int b, int N, int& lo, int& hi) {
  lo = min(max(offsets[b], 0), N);
  hi = min(max(offsets[b + 1], lo), N);
}

// the frame that owns row i (largest b with offsets[b] <= i, then the clamped range must hold i); -1 when none does
__device__ __forceinline__ int lbl_frame_of(const int32_t* __restrict__ offsets, int B, int N, int i, int& lo, int& hi) {
  int l = 0, h = B;
  while (h - l > 1) {
    const int mid = (l + h) >> 1;
    if (offsets[mid] <= i) l = mid; else h = mid;
  }
  lbl_frame_rows(offsets, l, N, lo, hi);
  return (i >= lo && i < hi) ? l : -1;
}

// R^T v as numpy's (rot.T @ v): column c of R against v, (a + b) + c
__device__ __forceinline__ void lbl_rot_t(const double* R, double x, double y, double z, double& qx, double& qy, double& qz) {
  qx = (R[0] * x + R[3] * y) + R[6] * z;
  qy = (R[1] * x + R[4] * y) + R[7] * z;
  qz = (R[2] * x + R[5] * y) + R[8] * z;
}

// get_ee_idx (:92-93): the difference in float64, then the rotation
template <typename T>
__device__ __forceinline__ void lbl_q_crop(const T* __restrict__ pts, size_t i, const double* R, const double* pos, double& qx,
                                           double& qy, double& qz) {
  const double x = (double)pts[i * 3] - pos[0], y = (double)pts[i * 3 + 1] - pos[1], z = (double)pts[i * 3 + 2] - pos[2];
  lbl_rot_t(R, x, y, z, qx, qy, qz);
}

// get_ee_cross_section_idx (:107-112): the in-place subtraction rounds the difference to the points' own dtype first
template <typename T>
__device__ __forceinline__ void lbl_q_line(const T* __restrict__ pts, size_t i, const double* R, const double* pos, double& qx,
                                           double& qy, double& qz) {
  const T x = (T)((double)pts[i * 3] - pos[0]), y = (T)((double)pts[i * 3 + 1] - pos[1]), z = (T)((double)pts[i * 3 + 2] - pos[2]);
  lbl_rot_t(R, (double)x, (double)y, (double)z, qx, qy, qz);
}

// get_key_points / get_6_key_points (:144-148, :258-262): the rotated point minus the rotated position `off`
template <typename T>
__device__ __forceinline__ void lbl_q_kp(const T* __restrict__ pts, size_t i, const double* R, const double* off, double& qx,
                                         double& qy, double& qz) {
  lbl_rot_t(R, (double)pts[i * 3], (double)pts[i * 3 + 1], (double)pts[i * 3 + 2], qx, qy, qz);
  qx = qx - off[0], qy = qy - off[1], qz = qz - off[2];
}

__device__ __forceinline__ double lbl_norm3(double x, double y, double z) { return __dsqrt_rn((x * x + y * y) + z * z); }

// numpy's max: a NaN on either side wins
__device__ __forceinline__ double lbl_nan_max(double a, double b) { return (a > b || a != a) ? a : b; }

// a candidate of an arg-min; {inf, INT_MAX} is "none", which every real candidate beats
struct Cand {
  double d;
  int i;
};
// numpy argmin's order: the first NaN before everything, else the smaller distance, a tie to the lower index
__device__ __forceinline__ bool cand_before(const Cand& a, const Cand& b) {
  const bool an = a.d != a.d, bn = b.d != b.d;
  if (an || bn) return an && (!bn || a.i < b.i);
  return a.d < b.d || (a.d == b.d && a.i < b.i);
}
__device__ __forceinline__ Cand cand_wave_min(Cand c) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    Cand o;
    o.d = __shfl_xor(c.d, s);
    o.i = __shfl_xor(c.i, s);
    if (cand_before(o, c)) c = o;
  }
  return c;
}

struct EeBox {
  double v[6];  // min_x, max_x, min_y, max_y, min_z, max_z
};

template <typename T>
__global__ __launch_bounds__(LBL_BLOCK) void ee_mask_kernel(const T* __restrict__ pts, const int32_t* __restrict__ offsets, int N,
                                                            int B, const double* __restrict__ pos, const double* __restrict__ rot,
                                                            EeBox box, uint8_t* __restrict__ mask) {
  const int i = blockIdx.x * LBL_BLOCK + threadIdx.x;
  if (i >= N) return;
  int lo, hi;
  const int b = lbl_frame_of(offsets, B, N, i, lo, hi);
  bool in = false;
  if (b >= 0) {
    double qx, qy, qz;
    lbl_q_crop(pts, (size_t)i, rot + (size_t)b * 9, pos + (size_t)b * 3, qx, qy, qz);
    // get_roi_mask:66-73, the redundant first term kept: every compare is false for a NaN
    in = qx > -500.0 && qx < box.v[1] && qx > box.v[0] && qy < box.v[3] && qy > box.v[2] && qz < box.v[5] && qz > box.v[4];
  }
  mask[i] = in ? 1 : 0;
}

// ---- key points ----------------------------------------------------------------------------------------------------
enum { SEL_FRONT = 0, SEL_BACK, SEL_GRIP_L, SEL_GRIP_R, SEL_EE6, SEL_NONE };

__device__ __forceinline__ bool lbl_selected(int sel, double x, double y, double z) {
  switch (sel) {
    case SEL_FRONT: return x > 0.005;
    case SEL_BACK: return x < -0.01;
    case SEL_GRIP_L: return z > 0.08 && y > 0.0;
    case SEL_GRIP_R: return z > 0.08 && y < 0.0;
    case SEL_EE6: return x > -0.005 && z < 0.09;
    default: return false;
  }
}

constexpr int KP_SLOTS = 6;  // searches per pass

struct KpShared {
  double R[9], off[3];
  double kp[10][3];
  long long idx[10];
  double tg[KP_SLOTS][3];  // targets of the running pass
  int sel[KP_SLOTS];
  Cand res[KP_SLOTS];
  double zmax[2];
  Cand red[LBL_WAVES][KP_SLOTS];
  double redz[LBL_WAVES][2];
  int cnt[LBL_WAVES][2], rank[2], gidx[2], wtot[LBL_WAVES];
};

// One pass over the frame's rows: for every slot s the arg-min of ||q - tg[s]|| over the rows its selection holds
// (get_closest_point:133-136), and, with want_z, the max of z over the two gripper selections (:131).
template <typename T>
__device__ void kp_pass(const T* __restrict__ pts, int lo, int hi, KpShared& sh, bool want_z) {
  __syncthreads();  // thread 0's targets are visible; the previous pass's results have been read
  Cand best[KP_SLOTS];
  double tg[KP_SLOTS][3];
  int sel[KP_SLOTS];
#pragma unroll
  for (int s = 0; s < KP_SLOTS; ++s) {
    best[s].d = INFINITY, best[s].i = INT_MAX;
    tg[s][0] = sh.tg[s][0], tg[s][1] = sh.tg[s][1], tg[s][2] = sh.tg[s][2];
    sel[s] = sh.sel[s];
  }
  double zl = -INFINITY, zr = -INFINITY;
  for (int i = lo + (int)threadIdx.x; i < hi; i += LBL_BLOCK) {
    double x, y, z;
    lbl_q_kp(pts, (size_t)i, sh.R, sh.off, x, y, z);
    if (want_z) {
      if (lbl_selected(SEL_GRIP_L, x, y, z)) zl = lbl_nan_max(zl, z);
      if (lbl_selected(SEL_GRIP_R, x, y, z)) zr = lbl_nan_max(zr, z);
    }
#pragma unroll
    for (int s = 0; s < KP_SLOTS; ++s) {
      if (!lbl_selected(sel[s], x, y, z)) continue;
      Cand c;
      c.d = lbl_norm3(x - tg[s][0], y - tg[s][1], z - tg[s][2]);
      c.i = i - lo;
      if (cand_before(c, best[s])) best[s] = c;  // rows ascend per thread, so an equal distance keeps the earlier row
    }
  }
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < KP_SLOTS; ++s) {
    const Cand c = cand_wave_min(best[s]);
    if ((threadIdx.x & 63) == 0) sh.red[w][s] = c;
  }
  if (want_z) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      zl = lbl_nan_max(zl, __shfl_xor(zl, s));
      zr = lbl_nan_max(zr, __shfl_xor(zr, s));
    }
    if ((threadIdx.x & 63) == 0) sh.redz[w][0] = zl, sh.redz[w][1] = zr;
  }
  __syncthreads();
  if (threadIdx.x < KP_SLOTS) {
    Cand c = sh.red[0][threadIdx.x];
    for (int k = 1; k < LBL_WAVES; ++k)
      if (cand_before(sh.red[k][threadIdx.x], c)) c = sh.red[k][threadIdx.x];
    sh.res[threadIdx.x] = c;
  }
  if (want_z && threadIdx.x >= 64 && threadIdx.x < 66) {
    const int k = threadIdx.x - 64;
    double v = sh.redz[0][k];
    for (int q = 1; q < LBL_WAVES; ++q) v = lbl_nan_max(v, sh.redz[q][k]);
    sh.zmax[k] = v;
  }
  __syncthreads();
}

__device__ __forceinline__ void kp_set_target(KpShared& sh, int s, int sel, double x, double y, double z) {
  sh.sel[s] = sel;
  sh.tg[s][0] = x, sh.tg[s][1] = y, sh.tg[s][2] = z;
}

// The index the reference records for a gripper key point (:227, :239): the winner's position within its side's subset
// (z > 0.08 and y > 0, or y < 0), looked up in the list of ALL rows with z > 0.08.  sh.gidx[g] = the rank-th such row, rank =
// the number of the side's rows before the winner sh.res[4 + g].  Called by the whole workgroup.
template <typename T>
__device__ void kp_gripper_index(const T* __restrict__ pts, int lo, int hi, KpShared& sh) {
  const int win[2] = {sh.res[4].i, sh.res[5].i};
  int c[2] = {0, 0};
  for (int i = lo + (int)threadIdx.x; i < hi; i += LBL_BLOCK) {
    double x, y, z;
    lbl_q_kp(pts, (size_t)i, sh.R, sh.off, x, y, z);
    if (lbl_selected(SEL_GRIP_L, x, y, z) && i - lo < win[0]) ++c[0];
    if (lbl_selected(SEL_GRIP_R, x, y, z) && i - lo < win[1]) ++c[1];
  }
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int g = 0; g < 2; ++g) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) c[g] += __shfl_xor(c[g], s);
    if (lane == 0) sh.cnt[w][g] = c[g];
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    int v = 0;
    for (int k = 0; k < LBL_WAVES; ++k) v += sh.cnt[k][threadIdx.x];
    sh.rank[threadIdx.x] = v;
    sh.gidx[threadIdx.x] = 0;
  }
  __syncthreads();
  const int rank[2] = {sh.rank[0], sh.rank[1]};
  int run = 0;  // rows with z > 0.08 before this chunk
  for (int base = lo; base < hi; base += LBL_BLOCK) {  // uniform trip count
    const int i = base + (int)threadIdx.x;
    bool flag = false;
    if (i < hi) {
      double x, y, z;
      lbl_q_kp(pts, (size_t)i, sh.R, sh.off, x, y, z);
      flag = z > 0.08;
    }
    const unsigned long long bal = __ballot(flag);
    if (lane == 0) sh.wtot[w] = __popcll(bal);
    __syncthreads();
    int before = run + __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
    for (int k = 0; k < LBL_WAVES; ++k) {
      if (k < w) before += sh.wtot[k];
      total += sh.wtot[k];
    }
    if (flag) {
      if (win[0] != INT_MAX && before == rank[0]) sh.gidx[0] = i - lo;
      if (win[1] != INT_MAX && before == rank[1]) sh.gidx[1] = i - lo;
    }
    run += total;
    __syncthreads();  // wtot is rewritten by the next chunk
  }
  __syncthreads();
}

// the gripper pair (:214-247 / :297-330), slots 4 and 5 of the finished pass, then the mirror and equal-z fix-ups
template <typename T>
__device__ void kp_gripper(const T* __restrict__ pts, int lo, KpShared& sh) {
  bool found[2];
  for (int g = 0; g < 2; ++g) {
    const Cand c = sh.res[4 + g];
    found[g] = c.i != INT_MAX;
    if (found[g]) {
      lbl_q_kp(pts, (size_t)(lo + c.i), sh.R, sh.off, sh.kp[4 + g][0], sh.kp[4 + g][1], sh.kp[4 + g][2]);
      sh.idx[4 + g] = sh.gidx[g];
    }
  }
  if (!found[0] && found[1]) {
    sh.kp[4][0] = sh.kp[5][0] * 1.0, sh.kp[4][1] = sh.kp[5][1] * -1.0, sh.kp[4][2] = sh.kp[5][2] * 1.0;
  } else if (found[0] && !found[1]) {
    sh.kp[5][0] = sh.kp[4][0] * 1.0, sh.kp[5][1] = sh.kp[4][1] * -1.0, sh.kp[5][2] = sh.kp[4][2] * 1.0;
  }
  if (sh.kp[5][2] > sh.kp[4][2]) sh.kp[4][2] = sh.kp[5][2];  // python's max(a, b)
  sh.kp[5][2] = sh.kp[4][2];
}

template <typename T>
__global__ __launch_bounds__(LBL_BLOCK) void key_points_kernel(const T* __restrict__ pts, const int32_t* __restrict__ offsets,
                                                               int N, const double* __restrict__ pos,
                                                               const double* __restrict__ rot, int mode, double thr,
                                                               long long ignore_label, double* __restrict__ key_points,
                                                               long long* __restrict__ kp_idx,
                                                               int32_t* __restrict__ selection_empty) {
  __shared__ KpShared sh;
  const int b = blockIdx.x;
  const int K = mode == 10 ? 10 : 6;
  int lo, hi;
  lbl_frame_rows(offsets, b, N, lo, hi);
  if (threadIdx.x == 0) {
    for (int k = 0; k < 9; ++k) sh.R[k] = rot[(size_t)b * 9 + k];
    // the position goes through the same product as the points; center_at_origin of one row: (max + min) / 2
    double ox, oy, oz;
    lbl_rot_t(sh.R, pos[(size_t)b * 3], pos[(size_t)b * 3 + 1], pos[(size_t)b * 3 + 2], ox, oy, oz);
    sh.off[0] = (ox + ox) / 2.0, sh.off[1] = (oy + oy) / 2.0, sh.off[2] = (oz + oz) / 2.0;
    const double t10[10][3] = {{0.02, 0.09, 0},     {0.02, -0.09, 0},     {0.014, 0.095, 0.07}, {0.014, -0.095, 0.07},
                               {0, 0.048, 0.12},    {0, -0.048, 0.12},    {-0.022, 0.09, 0},    {-0.022, -0.09, 0},
                               {-0.014, 0.095, 0.07}, {-0.014, -0.095, 0.07}};
    for (int k = 0; k < 10; ++k) {
      sh.kp[k][0] = t10[k][0], sh.kp[k][1] = t10[k][1], sh.kp[k][2] = t10[k][2];
      sh.idx[k] = ignore_label;
    }
    if (mode == 6) sh.kp[1][0] = 0.01, sh.kp[1][1] = -0.1;  // P2 of get_6_key_points:266
    if (mode == 10) {
      for (int s = 0; s < 4; ++s) kp_set_target(sh, s, SEL_FRONT, sh.kp[s][0], sh.kp[s][1], sh.kp[s][2]);
    } else {  // ee_bbox:279-284
      kp_set_target(sh, 0, SEL_EE6, 0.24, 0.32, -0.2);
      kp_set_target(sh, 1, SEL_EE6, 0.24, -0.32, -0.2);
      kp_set_target(sh, 2, SEL_EE6, 0.24, 0.32, 0.2);
      kp_set_target(sh, 3, SEL_EE6, 0.24, -0.32, 0.2);
    }
    kp_set_target(sh, 4, SEL_NONE, 0, 0, 0);
    kp_set_target(sh, 5, SEL_NONE, 0, 0, 0);
  }
  kp_pass(pts, lo, hi, sh, true);
  bool skip_rest = false;  // get_6_key_points with an empty selection: the template as it is
  if (mode == 6) skip_rest = sh.res[0].i == INT_MAX;
  if (selection_empty && threadIdx.x == 0) selection_empty[b] = skip_rest ? 1 : 0;
  if (threadIdx.x == 0 && !skip_rest) {
    if (mode == 10) {
      const double dx[4] = {-0.04, -0.04, -0.03, -0.03};
      for (int s = 0; s < 4; ++s) {  // P1 .. P4: found moves the key point and its mirror on the back side
        const Cand c = sh.res[s];
        if (c.i != INT_MAX && c.d < thr) {
          double x, y, z;
          lbl_q_kp(pts, (size_t)(lo + c.i), sh.R, sh.off, x, y, z);
          sh.kp[s][0] = x, sh.kp[s][1] = y, sh.kp[s][2] = z;
          sh.idx[s] = c.i;
          sh.kp[6 + s][0] = x + dx[s], sh.kp[6 + s][1] = y + 0.0, sh.kp[6 + s][2] = z + 0.0;
        }
      }
      for (int s = 0; s < 4; ++s) kp_set_target(sh, s, SEL_BACK, sh.kp[6 + s][0], sh.kp[6 + s][1], sh.kp[6 + s][2]);
    } else {
      for (int s = 0; s < 4; ++s) {  // the point nearest the box corner, kept when it lies within thr of the template
        const Cand c = sh.res[s];
        double x, y, z;
        lbl_q_kp(pts, (size_t)(lo + c.i), sh.R, sh.off, x, y, z);
        sh.tg[s][0] = x, sh.tg[s][1] = y, sh.tg[s][2] = z;
      }
      for (int s = 0; s < 4; ++s) {  // all four distances against the untouched template, then the writes (:293-295)
        const double d = lbl_norm3(sh.kp[s][0] - sh.tg[s][0], sh.kp[s][1] - sh.tg[s][1], sh.kp[s][2] - sh.tg[s][2]);
        sh.sel[s] = d < thr ? 1 : 0;
      }
      for (int s = 0; s < 4; ++s) {
        if (sh.sel[s]) {
          sh.kp[s][0] = sh.tg[s][0], sh.kp[s][1] = sh.tg[s][1], sh.kp[s][2] = sh.tg[s][2];
          sh.idx[s] = sh.res[s].i;
        }
        sh.sel[s] = SEL_NONE;
      }
    }
    kp_set_target(sh, 4, SEL_GRIP_L, 0.0, 0.01, sh.zmax[0]);
    kp_set_target(sh, 5, SEL_GRIP_R, 0.0, -0.01, sh.zmax[1]);
  }
  if (!skip_rest) {  // uniform over the workgroup: sh.res was written before kp_pass's last barrier
    kp_pass(pts, lo, hi, sh, false);
    if (threadIdx.x == 0 && mode == 10) {
      for (int s = 0; s < 4; ++s) {  // P7 .. P10
        const Cand c = sh.res[s];
        if (c.i != INT_MAX && c.d < thr) {
          lbl_q_kp(pts, (size_t)(lo + c.i), sh.R, sh.off, sh.kp[6 + s][0], sh.kp[6 + s][1], sh.kp[6 + s][2]);
          sh.idx[6 + s] = c.i;
        }
      }
    }
    kp_gripper_index(pts, lo, hi, sh);
    if (threadIdx.x == 0) kp_gripper(pts, lo, sh);
  }
  __syncthreads();
  if (threadIdx.x < K) {  // key_points += ee_pose_offset, then rot @ key_points
    const int k = threadIdx.x;
    const double x = sh.kp[k][0] + sh.off[0], y = sh.kp[k][1] + sh.off[1], z = sh.kp[k][2] + sh.off[2];
    double* o = key_points + ((size_t)b * K + k) * 3;
    o[0] = (sh.R[0] * x + sh.R[1] * y) + sh.R[2] * z;
    o[1] = (sh.R[3] * x + sh.R[4] * y) + sh.R[5] * z;
    o[2] = (sh.R[6] * x + sh.R[7] * y) + sh.R[8] * z;
    kp_idx[(size_t)b * K + k] = sh.idx[k];
  }
}

// ---- cross-section -------------------------------------------------------------------------------------------------
struct Line {
  double p1[3], d[3];  // compute_dists_to_line's lp1 and (lp1 - lp2) / ||lp1 - lp2||
};

template <typename T>
__global__ __launch_bounds__(LBL_BLOCK) void line_dist_kernel(const T* __restrict__ pts, const int32_t* __restrict__ offsets, int N,
                                                              int B, const double* __restrict__ pos,
                                                              const double* __restrict__ rot, Line ln, double* __restrict__ dist) {
  const int i = blockIdx.x * LBL_BLOCK + threadIdx.x;
  if (i >= N) return;
  int lo, hi;
  const int b = lbl_frame_of(offsets, B, N, i, lo, hi);
  double r = NAN;
  if (b >= 0) {
    double x, y, z;
    lbl_q_line(pts, (size_t)i, rot + (size_t)b * 9, pos + (size_t)b * 3, x, y, z);
    const double vx = x - ln.p1[0], vy = y - ln.p1[1], vz = z - ln.p1[2];
    const double t = (vx * ln.d[0] + vy * ln.d[1]) + vz * ln.d[2];
    const double ex = (ln.p1[0] + t * ln.d[0]) - x, ey = (ln.p1[1] + t * ln.d[1]) - y, ez = (ln.p1[2] + t * ln.d[2]) - z;
    r = lbl_norm3(ex, ey, ez);
  }
  dist[i] = r;
}

__global__ __launch_bounds__(LBL_BLOCK) void line_topk_kernel(const double* __restrict__ dist, const int32_t* __restrict__ offsets,
                                                              int N, int count, double cutoff, long long* __restrict__ idx,
                                                              double* __restrict__ out_dist, int32_t* __restrict__ n_sel) {
  __shared__ Cand red[LBL_WAVES];
  __shared__ Cand pick;
  const int b = blockIdx.x;
  int lo, hi;
  lbl_frame_rows(offsets, b, N, lo, hi);
  Cand prev;
  prev.d = -INFINITY, prev.i = -1;
  int found = 0;
  for (; found < count; ++found) {
    Cand best;
    best.d = INFINITY, best.i = INT_MAX;
    for (int i = lo + (int)threadIdx.x; i < hi; i += LBL_BLOCK) {
      Cand c;
      c.d = dist[i], c.i = i - lo;
      // argsort's first `count` entries that pass `dist < cutoff` (transformation.py:154-158): a NaN sorts last and fails
      if (!(c.d < cutoff)) continue;
      if (!(c.d > prev.d || (c.d == prev.d && c.i > prev.i))) continue;  // already picked
      if (cand_before(c, best)) best = c;
    }
    best = cand_wave_min(best);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
      Cand c = red[0];
      for (int k = 1; k < LBL_WAVES; ++k)
        if (cand_before(red[k], c)) c = red[k];
      pick = c;
    }
    __syncthreads();
    prev = pick;
    __syncthreads();  // pick is rewritten in the next round
    if (prev.i == INT_MAX) break;  // uniform
    if (threadIdx.x == 0) {
      idx[(size_t)b * count + found] = prev.i;
      out_dist[(size_t)b * count + found] = prev.d;
    }
  }
  for (int k = found + (int)threadIdx.x; k < count; k += LBL_BLOCK) {
    idx[(size_t)b * count + k] = -1;
    out_dist[(size_t)b * count + k] = INFINITY;
  }
  if (threadIdx.x == 0) n_sel[b] = found;
}

// ---- radius labels -------------------------------------------------------------------------------------------------
__device__ __forceinline__ float lbl_sqrt(float v) { return __fsqrt_rn(v); }
__device__ __forceinline__ double lbl_sqrt(double v) { return __dsqrt_rn(v); }

template <typename T>
__global__ __launch_bounds__(LBL_BLOCK) void radius_labels_kernel(const T* __restrict__ pts, const int32_t* __restrict__ offsets,
                                                                  int N, int B, const long long* __restrict__ kp_idx, int K,
                                                                  T thr, long long ignore_label, long long* __restrict__ labels) {
  const int i = blockIdx.x * LBL_BLOCK + threadIdx.x;
  if (i >= N) return;
  int lo, hi;
  const int b = lbl_frame_of(offsets, B, N, i, lo, hi);
  long long lab = ignore_label;
  if (b >= 0) {
    const T x = pts[(size_t)i * 3], y = pts[(size_t)i * 3 + 1], z = pts[(size_t)i * 3 + 2];
    for (int k = K - 1; k >= 0; --k) {  // the last write of labels[p_idx] = classes wins: the highest class
      const long long a = kp_idx[(size_t)b * K + k];
      if (a < 0 || a >= (long long)(hi - lo)) continue;
      const size_t r = (size_t)lo + (size_t)a;
      // collect_closest_points:339-340 in the points' own dtype: points[idx] - points, squares, (a + b) + c, sqrt
      const T dx = pts[r * 3] - x, dy = pts[r * 3 + 1] - y, dz = pts[r * 3 + 2] - z;
      if (lbl_sqrt((dx * dx + dy * dy) + dz * dz) < thr) {
        lab = k;
        break;
      }
    }
  }
  labels[i] = lab;
}

static inline unsigned lbl_grid(int64_t n) { return (unsigned)((n + LBL_BLOCK - 1) / LBL_BLOCK); }

}  // namespace sv

using namespace sv;

#define SV_LBL_COMMON_CHECKS()                                                        \
  SV_CHECK_ARG(B >= 1 && B <= SV_MAX_BATCH, "need 1 to 1024 frames");                 \
  SV_CHECK_ARG(N >= 0 && N < (1LL << 29), "need 0 <= N < 2^29 points")

extern "C" {

int sv_ee_mask(const void* points, int points_f64, const int32_t* offsets, int64_t N, int B, const double* pos,
               const double* rot, const double* box, uint8_t* mask, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_LBL_COMMON_CHECKS();
  SV_CHECK_ARG((points || N == 0) && (mask || N == 0) && offsets && pos && rot, "null pointer");
  if (N == 0) return SV_OK;
  EeBox bx = {{-0.05, 0.05, -0.11, 0.11, -0.006, 0.12}};  // ee_dim_init, utils/data.py:79-86
  if (box)
    for (int k = 0; k < 6; ++k) bx.v[k] = box[k];
  if (points_f64)
    hipLaunchKernelGGL(ee_mask_kernel<double>, dim3(lbl_grid(N)), dim3(LBL_BLOCK), 0, stream, (const double*)points, offsets,
                       (int)N, B, pos, rot, bx, mask);
  else
    hipLaunchKernelGGL(ee_mask_kernel<float>, dim3(lbl_grid(N)), dim3(LBL_BLOCK), 0, stream, (const float*)points, offsets,
                       (int)N, B, pos, rot, bx, mask);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

int sv_key_points(const void* points, int points_f64, const int32_t* offsets, int64_t N, int B, const double* pos,
                  const double* rot, int mode, double euclidean_threshold, int64_t ignore_label, double* key_points,
                  int64_t* kp_idx, int32_t* selection_empty, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_LBL_COMMON_CHECKS();
  SV_CHECK_ARG(mode == 10 || mode == 6, "mode must be 10 or 6");
  SV_CHECK_ARG(ignore_label < 0, "ignore_label must be negative");
  SV_CHECK_ARG((points || N == 0) && offsets && pos && rot && key_points && kp_idx, "null pointer");
  if (points_f64)
    hipLaunchKernelGGL(key_points_kernel<double>, dim3(B), dim3(LBL_BLOCK), 0, stream, (const double*)points, offsets, (int)N,
                       pos, rot, mode, euclidean_threshold, (long long)ignore_label, key_points, (long long*)kp_idx,
                       selection_empty);
  else
    hipLaunchKernelGGL(key_points_kernel<float>, dim3(B), dim3(LBL_BLOCK), 0, stream, (const float*)points, offsets, (int)N,
                       pos, rot, mode, euclidean_threshold, (long long)ignore_label, key_points, (long long*)kp_idx,
                       selection_empty);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

size_t sv_line_topk_workspace_bytes(int64_t N) {
  if (N < 0) N = 0;
  return align_up((size_t)N * sizeof(double), 256) + 256;
}

int sv_line_topk(const void* points, int points_f64, const int32_t* offsets, int64_t N, int B, const double* pos,
                 const double* rot, const double* lp1, const double* lp2, int count, double cutoff, void* workspace,
                 size_t workspace_bytes, int64_t* idx, double* dist, int32_t* n_sel, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_LBL_COMMON_CHECKS();
  SV_CHECK_ARG(count >= 1 && count <= 1024, "count must be in [1, 1024]");
  SV_CHECK_ARG((points || N == 0) && offsets && pos && rot && lp1 && lp2 && workspace && idx && dist && n_sel, "null pointer");
  Line ln;
  const double ax = lp1[0] - lp2[0], ay = lp1[1] - lp2[1], az = lp1[2] - lp2[2];
  const double len = sqrt((ax * ax + ay * ay) + az * az);
  SV_CHECK_ARG(len > 0.0 && len < INFINITY, "lp1 and lp2 must be two distinct finite points");
  ln.d[0] = ax / len, ln.d[1] = ay / len, ln.d[2] = az / len;
  for (int k = 0; k < 3; ++k) ln.p1[k] = lp1[k];
  Workspace ws(workspace, workspace_bytes);
  double* d_all = ws.take<double>((size_t)N);
  if (!ws.ok) {
    set_error("sv_line_topk: workspace too small");
    return SV_ERR_WORKSPACE;
  }
  if (N > 0) {
    if (points_f64)
      hipLaunchKernelGGL(line_dist_kernel<double>, dim3(lbl_grid(N)), dim3(LBL_BLOCK), 0, stream, (const double*)points, offsets,
                         (int)N, B, pos, rot, ln, d_all);
    else
      hipLaunchKernelGGL(line_dist_kernel<float>, dim3(lbl_grid(N)), dim3(LBL_BLOCK), 0, stream, (const float*)points, offsets,
                         (int)N, B, pos, rot, ln, d_all);
  }
  hipLaunchKernelGGL(line_topk_kernel, dim3(B), dim3(LBL_BLOCK), 0, stream, d_all, offsets, (int)N, count, cutoff,
                     (long long*)idx, dist, n_sel);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

int sv_radius_labels(const void* points, int points_f64, const int32_t* offsets, int64_t N, int B, const int64_t* kp_idx,
                     int K, double euclidean_threshold, int64_t ignore_label, int64_t* labels, sv_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SV_LBL_COMMON_CHECKS();
  SV_CHECK_ARG(K >= 1 && K <= LBL_MAX_K, "K must be in [1, 64]");
  SV_CHECK_ARG(ignore_label < 0, "ignore_label must be negative");
  SV_CHECK_ARG((points || N == 0) && (labels || N == 0) && offsets && kp_idx, "null pointer");
  if (N == 0) return SV_OK;
  if (points_f64)
    hipLaunchKernelGGL(radius_labels_kernel<double>, dim3(lbl_grid(N)), dim3(LBL_BLOCK), 0, stream, (const double*)points,
                       offsets, (int)N, B, (const long long*)kp_idx, K, euclidean_threshold, (long long)ignore_label,
                       (long long*)labels);
  else
    hipLaunchKernelGGL(radius_labels_kernel<float>, dim3(lbl_grid(N)), dim3(LBL_BLOCK), 0, stream, (const float*)points,
                       offsets, (int)N, B, (const long long*)kp_idx, K, (float)euclidean_threshold, (long long)ignore_label,
                       (long long*)labels);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

}  // extern "C"
