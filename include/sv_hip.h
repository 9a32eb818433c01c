/*
 * sv_hip.h — C-ABI of libsvhip.so, the MI355X (gfx950) sparse-voxel inference library.
 *
 * This is the drop-in boundary for the hot path of bcsefercik/markerless-robot-camera-calibration
 * (SURVEY.md §8b): everything the reference gets from MinkowskiEngine 0.5.4 / numpy LAPACK on the
 * path  voxelise -> sparse U-Net -> slice/argmax -> Kabsch  is exported here as plain C functions.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (memory owned by the caller, normally a PyTorch-ROCm tensor)
 *    unless the name ends in _host;
 *  - `stream` is a hipStream_t passed as void*; NULL = the default stream;
 *  - the library allocates nothing persistent: temporaries come from a caller-supplied workspace whose
 *    size is returned by the matching *_workspace_bytes();
 *  - return value: 0 = OK, <0 = error (SV_ERR_*); sv_last_error() gives the message (thread-local);
 *  - dynamic sizes (number of voxels ...) are written to a small device `counters` array the caller
 *    reads back (one D2H copy), never returned through host pointers, so calls stay asynchronous.
 *
 * Row order of every coordinate map is CANONICAL: ascending 64-bit key
 *    key = batch << 54 | morton3(x + 2^17, y + 2^17, z + 2^17)       (x in bit 3j, y in 3j+1, z in 3j+2)
 * so a stride-2 parent key is the child key with 3 low Morton bits cleared and children of one parent are
 * contiguous rows.  (MinkowskiEngine leaves row order unspecified — SURVEY.md Appendix B.2.)
 *
 * Kernel-offset numbering (index into W[K][Cin][Cout]):
 *    kernel_size 3:  k = (dx+1) + 3*(dy+1) + 9*(dz+1),  dx,dy,dz in {-1,0,1}   (x fastest)
 *    kernel_size 2:  k = dx + 2*dy + 4*dz,              dx,dy,dz in {0,1}
 *    transposed kernel_size 2 stride 2: the fine voxel c with parent p uses k of (c - p) / tensor_stride.
 */
#ifndef SV_HIP_H
#define SV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SV_OK 0
#define SV_ERR_INVALID (-1)   /* bad shape / null pointer / unsupported parameter */
#define SV_ERR_WORKSPACE (-2) /* workspace too small */
#define SV_ERR_HIP (-3)       /* HIP runtime error, see sv_last_error() */
#define SV_ERR_RANGE (-4)     /* coordinate or batch index outside the key range (reported in counters) */
#define SV_ERR_UNSUPPORTED (-5) /* valid arguments outside what a fused kernel covers: the caller takes its unfused path */

#define SV_ACT_NONE 0
#define SV_ACT_RELU 1
#define SV_ACT_LEAKY_RELU 2

#define SV_POOL_MAX 0
#define SV_POOL_AVG 1

#define SV_REDUCE_MEAN 0  /* ME.SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE */
#define SV_REDUCE_FIRST 1 /* ME.utils.sparse_quantize: lowest original index represents the voxel */
#define SV_REDUCE_SUM 2   /* ME.SparseTensorQuantizationMode.UNWEIGHTED_SUM; the backward of slicing */

#define SV_TILE_ROWS 128 /* output rows per conv tile; plans are padded to a multiple of this */
#define SV_COORD_BIAS 131072 /* 2^17 */
#define SV_COORD_BITS 18
#define SV_MAX_BATCH 1024

typedef void* sv_stream_t;

const char* sv_last_error(void);
/* 2: sv_conv_fwd takes V_in (rows of `in`); sv_single_linkage_roots / sv_select_equal added
 * 3: sv_plan_build takes nbr_base (plans of a batch range of a kernel map); sv_key_point_predictions,
 *    sv_conv_last_instance and sv_conv_fwd_acc (offset-range passes of one layer) added
 * 4: sv_conv_set_dispatch (per-thread dispatch thresholds: one frame alone vs frames overlapped), the frame composites
 *    sv_frame_maps / sv_frame_plans (a frame's coordinate work as two host calls), sv_topk_indices (get_pred_center),
 *    sv_key_point_predictions_batched; later additions that leave every earlier signature as it was: sv_conv_wgrad,
 *    sv_conv_wgrad_bf16, the PointNet++ training entries of A9, the pose losses of N4, the augmentation entries of N5, the label
 *    entries of N6, the segmentation criterion and step metrics of N7, the packed-record ingest of N3e, the RGB-D ingest of N3f
 *    and its lens models of N3g, the field front end of N9 (sv_sinusoidal, sv_field_stage, SV_REDUCE_SUM) */
#define SV_ABI_VERSION 4
int sv_abi_version(void);

/* ---------------------------------------------------------------------------------------------
 * A1/A2  voxelisation   (replaces ME.TensorField(...).sparse(), ME.SparseTensor(coordinates=...),
 *        ME.utils.sparse_quantize; reference call sites app/inference_engine.py:405-415,446-454,540-549,
 *        test_segmentation.py:62-70, data/alivev2.py:290-296, train_segmentation.py:78)
 *
 * coords4: float32[N,4] rows (batch, x, y, z) already multiplied by `scale` by the caller, exactly what
 *          ME.utils.batched_coordinates hands to TensorField.  voxel = floor(coord) per axis.
 *          With coords_are_int != 0 the buffer is int32[N,4] (already quantised coordinates).
 *          Key range: a voxel coordinate lies in [-2^17, 2^17 - 1] per axis and the batch index in [0, 1023] (the 18 + 18 +
 *          18 + 10 bits of the key); a float row is in range iff -2^17 <= coord < 2^17 and 0 <= batch < 1024 (the batch is
 *          truncated), so NaN, +-inf and a negative batch fraction are out of range, as is every int32 outside those intervals.
 * keys:    uint64[N]    first V entries = canonical sorted unique keys
 * vcoords: int32[N,4]   first V rows   = (batch,x,y,z) of each voxel
 * inverse: int64[N]     voxel row of every input point  (TensorField -> SparseTensor inverse map)
 * order:   int32[N]     point indices sorted by (key, original index)  (stable)
 * seg_start:int32[N+1]  first V+1 entries: voxel v owns order[seg_start[v] .. seg_start[v+1])
 * counters:int32[4]     [0] = V, [1] = number of out-of-range points (must be 0), [2..3] reserved
 * ------------------------------------------------------------------------------------------- */
size_t sv_voxelize_workspace_bytes(int64_t N);
int sv_voxelize(const void* coords4, int coords_are_int, int64_t N, void* workspace, size_t workspace_bytes,
                uint64_t* keys, int32_t* vcoords, int64_t* inverse, int32_t* order, int32_t* seg_start,
                int32_t* counters, sv_stream_t stream);

/* per-voxel feature reduction: out[v][c] = mean (or first, or sum) of feats[order[j]][c], j in the voxel's segment,
 * summed sequentially in ascending original point index (deterministic); SV_REDUCE_SUM is that sum without the division.
 * IEEE sums: a NaN feature makes its voxel's mean NaN, +inf and -inf together give NaN.  Segments are never empty
 * (sv_voxelize's seg_start). */
int sv_voxel_reduce(const float* feats, int C, const int32_t* order, const int32_t* seg_start, int64_t V, int mode,
                    float* out, sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Coordinate manager pieces (replace ME's coordinate_map_gpu / kernel_map; implicit in every
 * ME.MinkowskiConvolution call of model/backbone/minkunet.py:55-121)
 * ------------------------------------------------------------------------------------------- */
/* open-addressing hash  key -> row ;  capacity must be a power of two >= 2*V.  An empty slot holds the key ~0, which is
 * also the key of the voxel (1023, 2^17-1, 2^17-1, 2^17-1): that key is not stored; sv_kernel_map_k3 and
 * sv_kernel_map_probe find the voxel as the last row of the table map's (canonical) vcoords instead. */
int sv_hash_build(const uint64_t* keys, int64_t V, uint64_t* table_keys, int32_t* table_vals, int64_t capacity,
                  sv_stream_t stream);

/* stride-2 coordinate map of a map at tensor stride 2^level:  out coord = floor(c / 2^(level+1)) * 2^(level+1).
 * parent: int32[V_in] row of each input voxel in the output map.  child_start: int32[V_in+1] (first V_out+1 used).
 * counters[0] = V_out. */
size_t sv_stride_map_workspace_bytes(int64_t V_in);
int sv_stride_map(const uint64_t* keys_in, int64_t V_in, int level, void* workspace, size_t workspace_bytes,
                  uint64_t* keys_out, int32_t* vcoords_out, int32_t* parent, int32_t* child_start, int32_t* counters,
                  sv_stream_t stream);

/* 27-offset neighbour table of a map with itself (kernel_size 3, stride 1):
 * nbr[k*ld + o] = row of voxel at coords[o] + offset_k * tensor_stride * dilation, or -1.   mask[o] bit k = present. */
int sv_kernel_map_k3(const int32_t* vcoords, int64_t V, int tensor_stride, int dilation, const uint64_t* table_keys,
                     const int32_t* table_vals, int64_t capacity, int32_t* nbr, int64_t ld, uint32_t* mask,
                     sv_stream_t stream);
/* kernel_size 2 stride 2 (down): out rows = coarse voxels; nbr[k*ld + p] = fine row of child k of p, or -1. */
int sv_kernel_map_down(const uint64_t* keys_fine, const int32_t* parent, int64_t V_fine, int level, int64_t V_coarse,
                       int32_t* nbr, int64_t ld, uint32_t* mask, sv_stream_t stream);
/* transposed kernel_size 2 stride 2 (up): out rows = fine voxels; nbr[k*ld + i] = parent[i] iff k == child id of i. */
int sv_kernel_map_up(const uint64_t* keys_fine, const int32_t* parent, int64_t V_fine, int level, int32_t* nbr,
                     int64_t ld, uint32_t* mask, sv_stream_t stream);

/* Conv execution plan: rows sorted by neighbour mask so that 16-row MFMA sub-tiles share offsets.
 * perm:    int32[Vpad]        output row handled at sorted position r (-1 = padding)
 * nbr_s:   int32[K][Vpad]     nbr[k][perm[r]]
 * submask: uint32[Vpad/128][K] bit s set = sub-tile s (rows 16s..16s+15 of the tile) has a neighbour at offset k
 * tile_order: int32[Vpad/128] plan tiles sorted by work (number of active (offset, sub-tile) slots) descending: the
 *          conv kernel dispatches its workgroups in this order (longest first) so the launch has a short tail
 * Vpad = round_up(V, 128).
 * Plans of a ROW RANGE of a kernel map (batched tensors whose feature tables exceed the 2 GB extent of the buffer-addressed
 * conv instances: the frames of a batch never share neighbours, data/alivev2.py:358-383): pass nbr + o0 / mask + o0 / V = o1 - o0
 * for output rows [o0, o1) and nbr_base = first input row of the range; every stored index is then relative to that row, and
 * sv_conv_fwd runs on `in + nbr_base * in_ld`, `out + o0 * out_ld`.  nbr_base = 0 for a whole map.
 * `perm` (and every plan array) must be 16-byte aligned: the conv epilogue reads it four entries at a time. */
size_t sv_plan_workspace_bytes(int64_t V);
int sv_plan_build(const int32_t* nbr, int64_t ld, const uint32_t* mask, int K, int64_t V, int64_t nbr_base, void* workspace,
                  size_t workspace_bytes, int32_t* perm, int32_t* nbr_s, uint32_t* submask, int32_t* tile_order,
                  int64_t Vpad, sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Frame composites: the coordinate work of ONE frame as two host calls (the reference reaches all of it implicitly through
 * ME.TensorField(...).sparse(), app/inference_engine.py:405-415, and the ME.MinkowskiConvolution calls of
 * model/backbone/minkunet.py:125-183; its consumer calls InferenceEngine.predict once per frame, app/main.py:432-456, so the
 * host time of ~200 launches behind ~120 calls is frame latency).  Same kernels, same array contents as the piecewise entry
 * points above.
 *
 * sv_frame_maps: voxelise (as sv_voxelize) + `levels` stride-2 maps (as sv_stride_map).  The level sizes are read back
 *   inside the call through `counters_host` (PINNED host memory, 4 * (levels + 2) int32): the only host synchronisations of
 *   a frame's coordinate work, each waiting for this call's own kernels on `stream`.  Outputs are carved from `arena`
 *   (sv_frame_maps_arena_bytes: worst case V_l <= N); `scratch` (sv_frame_maps_scratch_bytes) is free again on return.
 *   layout (host int64[8 + 6 * (levels + 1)]): [0] arena bytes used, [1] N, [2] levels, [3] offset of inverse int64[N],
 *   [4] order int32[N], [5] seg_start int32[V_0 + 1], [6] points outside the key range (then SV_ERR_RANGE), then per level l
 *   six entries: V_l, offset of keys uint64[V_l], vcoords int32[V_l][4], parent int32[V_l] (row of each voxel in level
 *   l + 1; -1 at the last level), child_start int32[V_{l+1} + 1] (-1 at the last level), 0.
 * sv_frame_plans: hash tables, kernel maps and conv plans of levels 0..levels; no synchronisation.  flags select what is
 *   built: SV_FRAME_K3 (27-offset map + plan per level), SV_FRAME_DOWN / SV_FRAME_UP (the kernel_size 2 stride 2 maps
 *   between levels l and l + 1 and their plans), SV_FRAME_SPLIT (offset-range plans: split_cuts[l][SV_FRAME_MAX_CUTS] holds
 *   level l's ascending split points, 0-terminated; they need the level's 27-offset map - built by SV_FRAME_K3 in the same
 *   call or passed in k3_nbr[l] / k3_mask[l], so that a caller can build them in a second call while the encoder runs).
 *   keys / coords / parent: per-level device pointers (parent[l] as in sv_frame_maps).  layout (host int64[16 * (1 +
 *   max_records)]): [0] arena bytes used, [1] number of records; record r at 16 * (1 + r): kind (SV_FRAME_REC_*), level, k0,
 *   k1, offset of the raw map int32[K][ld] (hash: of the table values; -1: rows k0..k1 of the caller's k3_nbr), of its mask
 *   (split: the range's mask), of perm, nbr_s, submask, tile_order, V_out, Vpad, K, ld, offset of the hash keys, capacity.
 * ------------------------------------------------------------------------------------------- */
#define SV_FRAME_MAX_LEVELS 8
#define SV_FRAME_MAX_CUTS 4
#define SV_FRAME_K3 1
#define SV_FRAME_DOWN 2
#define SV_FRAME_UP 4
#define SV_FRAME_SPLIT 8
#define SV_FRAME_RECORD 16
#define SV_FRAME_REC_HASH 1
#define SV_FRAME_REC_K3 2
#define SV_FRAME_REC_DOWN 3
#define SV_FRAME_REC_UP 4
#define SV_FRAME_REC_SPLIT 5
size_t sv_frame_maps_arena_bytes(int64_t N, int levels);
size_t sv_frame_maps_scratch_bytes(int64_t N);
int sv_frame_maps(const void* coords4, int coords_are_int, int64_t N, int levels, void* arena, size_t arena_bytes, void* scratch,
                  size_t scratch_bytes, int32_t* counters_host, int64_t* layout, sv_stream_t stream);
size_t sv_frame_plans_arena_bytes(const int64_t* V, int levels, int flags, const int32_t* split_cuts);
size_t sv_frame_plans_scratch_bytes(const int64_t* V, int levels);
int sv_frame_plans(const void* const* keys, const void* const* coords, const void* const* parent, const int64_t* V, int levels,
                   int flags, const int32_t* split_cuts, const void* const* k3_nbr, const void* const* k3_mask, void* arena,
                   size_t arena_bytes, void* scratch, size_t scratch_bytes, int64_t* layout, int max_records, sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * A3/A5  sparse convolution, output stationary, fp32 MFMA, fused epilogue
 *   (replaces ME.MinkowskiConvolution / ConvolutionTranspose / Linear + MinkowskiBatchNorm(eval) +
 *    residual add + ReLU/LeakyReLU: model/backbone/minkunet.py:125-187, resnet.py:95-127,
 *    model/robotnet_segmentation.py:55-64)
 *
 *   acc[o][n] = sum over k ascending, c ascending of  in[nbr[k][o]][c] * W[k][c][n]     (one fmaf chain)
 *   y = acc * scale[n] + shift[n]  (fmaf; scale NULL = 1, shift NULL = 0)   BN(eval) folded / bias
 *   y += residual[o][n]            (residual NULL = none)
 *   out[o][n] = act(y)
 * perm/nbr_s/submask NULL = dense rows (kernel_size 1 / Linear): nbr = identity.  tile_order may be NULL.
 * V_in = rows of `in` (every index in nbr_s is below it; = V_out for dense rows): with it the wide-layer kernels
 * address `in` through a bounds-checked buffer descriptor (32-bit offsets, absent neighbours read as zero rows);
 * inputs of 2 GB and more take the guarded form with 64-bit addresses - except dense rows (no plan, K = 1), which this
 * entry point splits into row ranges below the extent, and batched tensors, whose callers launch one batch range at a
 * time with plans built for that range (sv_plan_build: nbr_base).
 * One entry point, several kernels behind it (all with the chain order above, so results do not depend on the
 * choice): fp32-MFMA tiles for the wide layers, their fused-offset form for 32/64-channel inputs, a thread-per-voxel
 * VALU kernel for the 3-channel first layer and a row-streaming VALU kernel for dense layers with <= 4 outputs.
 * ------------------------------------------------------------------------------------------- */
int sv_conv_fwd(const float* in, int64_t V_in, int64_t in_ld, int Cin, const float* W, int K, int Cout, const int32_t* perm,
                const int32_t* nbr_s, const uint32_t* submask, const int32_t* tile_order, int64_t V_out, int64_t Vpad,
                const float* scale,
                const float* shift, const float* residual, int64_t res_ld, int act, float slope, float* out,
                int64_t out_ld, sv_stream_t stream);
/* The same layer with its chains CONTINUED from an earlier launch: acc_init[o][n] (row stride acc_ld, NULL = start at 0) is
 * the raw accumulator of output element (o, n) over the kernel offsets that precede this launch's - the caller splits the K
 * offsets of a layer into ascending ranges, runs every range with its own plan (its own row order: rows that share their
 * neighbours among 13-14 offsets group far better into 16-row matrix-op sub-tiles than rows that must share all 27:
 * 0.87 -> 0.96 useful row slots on the 2 cm room level) and weight block W + k0 * Cin * Cout, the first ranges with no
 * epilogue at all (scale = shift = residual = NULL, act = none: `out` then IS the raw accumulator), the last one with
 * acc_init = that buffer and the layer's epilogue.  The matrix op takes acc_init as its C operand, so every output
 * element is still ONE fma chain over (k ascending, c ascending): the result has the bits of the single launch. */
int sv_conv_fwd_acc(const float* in, int64_t V_in, int64_t in_ld, int Cin, const float* W, int K, int Cout, const int32_t* perm,
                    const int32_t* nbr_s, const uint32_t* submask, const int32_t* tile_order, int64_t V_out, int64_t Vpad,
                    const float* acc_init, int64_t acc_ld, const float* scale, const float* shift, const float* residual,
                    int64_t res_ld, int act, float slope, float* out, int64_t out_ld, sv_stream_t stream);
/* Kernel instance the calling thread's last sv_conv_fwd launched: "name|fast=F,ring=R,full=U" (fast = buffer-addressed
 * form; a tensor beyond its 2 GB extent, a misaligned plan or an odd channel count takes the guarded form).  Tests and the
 * bench's per-kernel table read it back instead of re-deriving the dispatch. */
const char* sv_conv_last_instance(void);
/* Dispatch thresholds of the calling thread's later sv_conv_fwd calls.  The instance lists were measured one launch at a
 * time; inside a multi-stream frame pipeline taller tiles win earlier (their launch tails are filled by the neighbour
 * frames' kernels), so the library default scales every "chosen from N workgroups" threshold by 0.3.  A caller that runs
 * ONE frame at a time (the reference's consumer: InferenceEngine.predict per frame, app/main.py:432-456) sets
 * want_scale = 1 - which also selects, for the thin 32 -> 32 layers, the kernel that keeps the layer's weights in LDS (one
 * 16-wave workgroup per CU: it needs whole CUs, which only a GPU that holds one frame has free).
 * tail_fraction = share of the plan tiles that chip-filling launches run as half-height tiles.
 * A negative value restores the library default (environment SV_CONV_WANT_SCALE / SV_CONV_TAIL).  Results never depend on
 * the instance (one fma chain per output element in every one of them). */
int sv_conv_set_dispatch(double want_scale, double tail_fraction);
/* Which instance an sv_conv_fwd_acc call of a shape would run on, asked without running it (host only: no stream, no
 * device pointer, works on a machine without a GPU).  This is the function the launch itself consults, so the answer is
 * the "name|fast=F,ring=R,full=U" string sv_conv_last_instance would report after that call.  n shapes per call (a sweep
 * of every padded row count is millions of questions): shapes_host[n][5] = K, Cin, Cout, Vpad, flags; the answer to shape
 * i is the NUL-terminated string at names_host + i * name_bytes.
 * flags: what the rules otherwise read from the call's pointers - */
#define SV_CONV_SEL_PLAN 1        /* perm / nbr_s / submask given */
#define SV_CONV_SEL_TILE_ORDER 2  /* tile_order given */
#define SV_CONV_SEL_VEC_A 4       /* `in` 16-byte aligned, in_ld % 4 == 0 (and Cin % 4 == 0): float4 gathers */
#define SV_CONV_SEL_BUF_OK 8      /* every operand below the 2 GB buffer extent and `perm` 16-byte aligned */
#define SV_CONV_SEL_ACC_INIT 16   /* acc_init given */
#define SV_CONV_SEL_W_ALIGNED 32  /* W 16-byte aligned */
/* want_scale / tail_fraction as in sv_conv_set_dispatch; a negative value means what a call on this thread would use now
 * (its sv_conv_set_dispatch setting, else the environment, else the library default).  The SV_CONV_FORCE* experiment
 * switches are ignored.  Shapes sv_conv_fwd_acc refuses (K outside 1..32, Vpad not a multiple of 128, K > 1 without a
 * plan) return SV_ERR_INVALID. */
int sv_conv_select(int64_t n, const int64_t* shapes_host, double want_scale, double tail_fraction, char* names_host,
                   size_t name_bytes);
/* Row `index` of the table of tile instances behind sv_conv_fwd: out_host[10] = TM, WAVES_N, NT, CPO (channels per fused
 * offset, 0 = one offset per step), MR, TN, GK, KC, PFD, USE_FULL.  SV_ERR_INVALID past the end of the table. */
int sv_conv_tile_info(int index, int* out_host);

/* ---------------------------------------------------------------------------------------------
 * A3/A5 at reduced precision: the opt-in bf16 matrix-core path of the wide layers (the same ME.MinkowskiConvolution /
 *   ConvolutionTranspose / Linear + BN(eval) + residual + ReLU/LeakyReLU calls as sv_conv_fwd: model/backbone/minkunet.py:125-187,
 *   model/robotnet_segmentation.py:55-64; 41 of the 51 conv / linear layers of RobotNetSegmentation(MinkUNet18D))
 *
 *   Wp = bf16(W) (round to nearest even, NaN stays NaN), packed once per weight by sv_pack_weights_bf16;
 *   acc[o][n] = acc_init[o][n] + sum over k ascending, 32-channel chunks c ascending of  bf16(in[nbr[k][o]][c..c+31]) . Wp[k][c..c+31][n]
 *     (activations stay fp32 in memory and are rounded to bf16 in registers; products summed in fp32 by the matrix op,
 *      one v_mfma_f32_16x16x32_bf16 per (offset, chunk): ONE accumulator chain per output element, so the result does not
 *      depend on the tile, the launch, sv_conv_set_dispatch, offset-range passes or the frames grouped into a tensor)
 *   epilogue in fp32, sv_conv_fwd's:  out[o][n] = act(fmaf(acc, scale[n], shift[n]) + residual[o][n])
 * sv_pack_weights_bf16: W float32[K][Cin][Cout] -> Wp uint16 (bf16 bits)[K * Cin * Cout] in B-fragment order:
 *     Wp[((k * Cin/32 + cb) * Cout/16 + t) * 512 + 8 l + j] = bf16(W[k][32 cb + 8 (l >> 4) + j][16 t + (l & 15)]),
 *   l = 0..63, j = 0..7; offsets stay outermost, so the block of offsets k0.. is Wp + k0 * Cin * Cout.  Needs Cin % 32 == 0
 *   and Cout % 16 == 0 (else SV_ERR_UNSUPPORTED); Wp 16-byte aligned.
 * sv_conv_fwd_bf16: sv_conv_fwd_acc's arguments with Wp in place of W (acc_init NULL = start at 0), same plans (perm / nbr_s /
 *   submask / tile_order, NULL = dense rows).  Returns SV_ERR_UNSUPPORTED, before looking at any pointer, unless
 *   Cin % 32 == 0, Cin >= 64, Cout % 16 == 0, Cout >= 64 and K <= 27; `in` must be 16-byte aligned with in_ld % 4 == 0.
 *   sv_conv_last_instance() then reports "conv_bf16_kernel<128, TN>".
 * ------------------------------------------------------------------------------------------- */
int sv_pack_weights_bf16(const float* W, int K, int Cin, int Cout, uint16_t* Wp, sv_stream_t stream);
int sv_conv_fwd_bf16(const float* in, int64_t V_in, int64_t in_ld, int Cin, const uint16_t* Wp, int K, int Cout,
                     const int32_t* perm, const int32_t* nbr_s, const uint32_t* submask, const int32_t* tile_order, int64_t V_out,
                     int64_t Vpad, const float* acc_init, int64_t acc_ld, const float* scale, const float* shift,
                     const float* residual, int64_t res_ld, int act, float slope, float* out, int64_t out_ld, sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * A3/A5 backward: the weight gradient of sv_conv_fwd's layers (training: the reference's train_segmentation.py,
 *   train_vote.py, train.py and train_key_points.py call loss.backward() through ME.MinkowskiConvolution /
 *   ConvolutionTranspose / Linear)
 *
 *   dW[k][c][n] (+)= sum over plan rows r with o = perm[r] >= 0 and i = nbr_s[k][r] >= 0 of  in[i][c] * dY[o][n]
 * for the K offsets of the plan (the FORWARD's plan: perm / nbr_s / submask / Vpad exactly as sv_conv_fwd takes them; NULL
 * = dense rows, i = o = r < V_out, K = 1).  `in` rows have stride in_ld, dY rows dy_ld (column slices of a cat buffer).
 * submask lets a workgroup skip the 16-row sub-tiles without a pair at its offset.  The input gradient needs no entry of
 * its own: it is sv_conv_fwd on dY with mirrored weights (offset 26 - k, transposed) on the same 3x3x3 plan, with W[k]^T
 * on the up plan (down conv) or the down plan (transposed conv).
 * Matrix op: v_mfma_f32_16x16x4_f32 (A = in^T, B = dY, reduction over pairs).  Every (chunk of plan tiles) writes its
 * partial dW into the workspace (sv_conv_wgrad_workspace_bytes, monotone in Vpad); a second pass sums the partials in
 * ascending chunk order and writes dW (accumulate = 0) or dW + that sum (accumulate != 0: the batch ranges of
 * ConvPlan.chunks and the offset ranges of a split layer): no float atomics, the same bits on every run.
 * V_out = 0 gives dW = 0 (unchanged when accumulating).  Plan arrays 4-byte aligned.
 * ------------------------------------------------------------------------------------------- */
size_t sv_conv_wgrad_workspace_bytes(int64_t Vpad, int K, int Cin, int Cout);
int sv_conv_wgrad(const float* in, int64_t V_in, int64_t in_ld, int Cin, const float* dy, int64_t V_out, int64_t dy_ld,
                  int Cout, int K, const int32_t* perm, const int32_t* nbr_s, const uint32_t* submask, int64_t Vpad,
                  int accumulate, void* workspace, size_t workspace_bytes, float* dW, sv_stream_t stream);

/* sv_conv_wgrad at reduced precision (the opt-in bf16 training mode: nn.set_training_precision):
 *   dW[k][c][n] (+)= sum over plan rows r with o = perm[r] >= 0 and i = nbr_s[k][r] >= 0 of  bf16(in[i][c]) * bf16(dY[o][n])
 * operands rounded to bf16 (round to nearest even, NaN stays NaN) when they are staged, products summed in fp32 by
 * v_mfma_f32_16x16x32_bf16 (32 pairs = two 16-row sub-tiles of the plan per matrix op; the live sub-tiles are paired in plan
 * order, a lone last one with zeros).  Same arguments, plans, accumulate, V_out = 0 and determinism as sv_conv_wgrad (per-chunk
 * partials summed in ascending chunk order, no float atomics; an absent pair zeroes both operands), with a workspace of its
 * own (sv_conv_wgrad_bf16_workspace_bytes, monotone in Vpad).  Returns SV_ERR_UNSUPPORTED, before looking at any pointer,
 * unless Cin % 16 == 0, Cout % 16 == 0 and K <= 27, and (after the argument checks) unless in and dy are 16-byte aligned
 * with in_ld % 4 == 0 and dy_ld % 4 == 0: the caller then uses sv_conv_wgrad. */
size_t sv_conv_wgrad_bf16_workspace_bytes(int64_t Vpad, int K, int Cin, int Cout);
int sv_conv_wgrad_bf16(const float* in, int64_t V_in, int64_t in_ld, int Cin, const float* dy, int64_t V_out, int64_t dy_ld,
                       int Cout, int K, const int32_t* perm, const int32_t* nbr_s, const uint32_t* submask, int64_t Vpad,
                       int accumulate, void* workspace, size_t workspace_bytes, float* dW, sv_stream_t stream);

/* Stand-alone BN(eval)/bias + residual + activation on feature rows, same arithmetic as the conv epilogue:
 *   out[v][c] = act( fmaf(in[v][c], scale[c], shift[c]) + residual[v][c] )
 * (ME.MinkowskiBatchNorm / MinkowskiReLU / MinkowskiLeakyReLU when not fused behind a conv, e.g.
 *  model/robotnet.py:47-50 output_layer, model/robotnet_segmentation.py:60) */
int sv_affine_act(const float* in, int64_t in_ld, int C, int64_t V, const float* scale, const float* shift,
                  const float* residual, int64_t res_ld, int act, float slope, float* out, int64_t out_ld,
                  sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * A11  pre-voxelisation transforms on device rows
 *   (replace utils/preprocess.py:8-11 center_at_origin, :14-17 base_at_origin, :20-37 normalize_colors,
 *    :40-56 normalize_points; callers app/inference_engine.py:396-404,440-444,470-488)
 * ------------------------------------------------------------------------------------------- */
/* Column statistics of x[N][C], C <= 4: col_min[C], col_max[C] (exact), col_sum[C] (float64, deterministic order) and,
 * when max_row_norm is given (it needs sub), max over rows of the float32 norm of (row - sub) over all C columns,
 * 1 <= C <= 4, in numpy's order sqrt((((x0-s0)^2 + (x1-s1)^2) + (x2-s2)^2) + (x3-s3)^2), float32 without contraction.
 * workspace: sv_col_stats_workspace_bytes(N). */
size_t sv_col_stats_workspace_bytes(int64_t N);
int sv_col_stats(const float* x, int64_t ld, int64_t N, int C, const float* sub, void* workspace, size_t workspace_bytes,
                 float* col_min, float* col_max, double* col_sum, float* max_row_norm, sv_stream_t stream);
/* out[r][c] = (x[r][c] - sub[c]) / div[c] + add[c]; a null sub / div / add skips that operation (IEEE float32 operations
 * in this order: `points - offset` and `rgb / 255` round exactly as the reference's numpy expressions). */
int sv_center_scale(const float* x, int64_t ld, int64_t N, int C, const float* sub, const float* div, const float* add,
                    float* out, int64_t out_ld, sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * A6/A7  pooling, slice, argmax
 *   (replace ME.MinkowskiGlobalMaxPooling/AvgPooling model/robotnet.py:43, robotnet_encode.py:41;
 *    SparseTensor.slice app/inference_engine.py:417,551; utils/output.py:67-73)
 * ------------------------------------------------------------------------------------------- */
/* batch_start[b] = first row with batch index >= b, b = 0..B  (rows are sorted by batch first; an empty batch b has
 * batch_start[b] == batch_start[b + 1], V = 0 gives all zeros). */
int sv_batch_offsets(const uint64_t* keys, int64_t V, int B, int32_t* batch_start, sv_stream_t stream);
/* out[b][c] over rows batch_start[b] .. batch_start[b + 1] of F (row stride ld >= C; out is [B][C] dense).
 * SV_POOL_MAX: torch.amax - a NaN in the column gives NaN, otherwise the exact maximum (+-inf included).
 * SV_POOL_AVG: float32 sum / row count (+inf with -inf gives NaN, as torch.mean); the summation order is the kernel's
 * (4 strided partial sums), so the last bits are not a sequential sum's.
 * An empty batch gives 0 in both modes (torch would raise for the max and give NaN for the mean). */
int sv_global_pool(const float* F, int64_t ld, int C, const int32_t* batch_start, int B, int mode, float* out,
                   sv_stream_t stream);
/* out[i][0..C) = F[inverse[i]][0..C) (a bit-exact gather; out is [N][C] dense). */
int sv_slice_rows(const float* F, int64_t ld, int C, const int64_t* inverse, int64_t N, float* out,
                  sv_stream_t stream);
/* label[i] = first index of the row maximum of F[inverse[i]][0..C), conf[i] = sigmoid(max) (conf may be NULL): torch's
 * max(1) - among equal maxima the first column, and the first NaN of a row is its maximum (conf NaN). */
int sv_slice_argmax(const float* F, int64_t ld, int C, const int64_t* inverse, int64_t N, int64_t* label,
                    float* conf, sv_stream_t stream);
/* Key-point selection (utils/output.py:81-87 get_key_point_predictions): softmax over the C <= 32 classes of each of
 * the N rows of `logits`, then per class c: prob[c] = max over rows of softmax[:, c], idx[c] = the LOWEST row that attains
 * it (-1 and 0 when N = 0), selected[c] = prob[c] > conf_th.  workspace: 8 C bytes.  One pass over the logits, no host
 * round trip between softmax, max and threshold.  NaN as in torch's softmax(1).max(0): a row holding a NaN, a +inf or
 * only -inf logits has a NaN softmax; if any row does, every class gets prob NaN, idx = the lowest such row and
 * selected 0. */
int sv_key_point_predictions(const float* logits, int64_t ld, int C, int64_t N, float conf_th, void* workspace,
                             size_t workspace_bytes, float* prob, int64_t* idx, int32_t* selected, sv_stream_t stream);

/* The same selection for G clouds whose rows are consecutive segments of `logits` (the crops of G frames in one sparse
 * tensor): segment g = rows seg_start_host[g] .. seg_start_host[g + 1] (HOST array, G + 1 entries); outputs [G][C], idx
 * relative to the segment's first row.  workspace: 8 C G bytes.  Segment by segment the result of the single call. */
int sv_key_point_predictions_batched(const float* logits, int64_t ld, int C, const int64_t* seg_start_host, int G, float conf_th,
                                     void* workspace, size_t workspace_bytes, float* prob, int64_t* idx, int32_t* selected,
                                     sv_stream_t stream);
/* idx[j] = row of the j-th largest x[i * ld], i < N, j < k <= 64 (ties: the lower row first, -0.0 and +0.0 tie; -1 when
 * N < k; every NaN, whatever its sign and payload, orders above +inf as in torch.sort, NaNs among themselves by row) - the
 * `out[:, 1].sort(descending=True)[1][:8]` of utils/output.py:45-64 get_pred_center without sorting N votes.  workspace: sv_topk_workspace_bytes(N, k). */
size_t sv_topk_workspace_bytes(int64_t N, int k);
int sv_topk_indices(const float* x, int64_t ld, int64_t N, int k, void* workspace, size_t workspace_bytes, int64_t* idx,
                    sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * A9/A10/A12  dense solves, one wavefront per problem, float64
 *   (replace utils/transformation.py:178-222 get_rigid_transform_3D + :80-84 get_q_from_matrix,
 *    utils/calibration.py:69-95 compute_quaternions_weighted_average, utils/metrics.py:139-150 compute_ADD_np)
 * ------------------------------------------------------------------------------------------- */
/* Counts: B >= 0 (0 = nothing to do); Kmax, Mmax, Pmax >= 1; every K[b], M[b], P[b] must lie in [1, max] (NULL = max).
 * The Python wrappers reject other counts before anything reaches the device; a kernel clamps a count to [0, max], so it
 * never reads outside its problem, and a count of 0 gives NaN.  Rows past a problem's count are never read.
 * NaN rule: a NaN or inf among the values a problem reads makes all of that problem's outputs NaN (not the identity
 * rotation or quaternion the Jacobi iterations would leave); other problems of the batch are unaffected, and each
 * problem's result has the same bits whatever else is in the batch. */
/* ref,tgt: double[B][Kmax][3]; K: int32[B] points used per problem.  R: double[B][9] row-major, t: double[B][3],
 * q: double[B][4] (w,x,y,z) or NULL, sign as scipy's Rotation.from_matrix leaves it (the branch of the largest of
 * trace and diagonal, the first on ties).  R is the proper rotation minimising sum |R a + t - b|^2, t = c_B - R c_A.
 * K = 1 or 2, or collinear points, give *a* proper rotation reaching that minimum: it is not unique there. */
int sv_kabsch_batched(const double* ref, const double* tgt, const int32_t* K, int Kmax, int B, double* R, double* t,
                      double* q_wxyz, sv_stream_t stream);
/* Q: double[B][Mmax][4] (w,x,y,z), w: double[B][Mmax] or NULL (all 1), M: int32[B].  out: double[B][4] principal
 * eigenvector of sum w_i q_i q_i^T / sum w_i, normalised, sign such that the largest-magnitude component is positive.
 * A weight sum <= 0 gives NaN, as a NaN does. */
int sv_quat_avg_batched(const double* Q, const double* w, const int32_t* M, int Mmax, int B, double* out,
                        sv_stream_t stream);
/* ADD = mean_p || (R_gt p + t_gt) - (R_pr p + t_pr) ||, poses (x,y,z,qw,qx,qy,qz) with R(q) of the reference's
 * formula (q not normalised).  points double[B][Pmax][3].  Identical poses give exactly 0. */
int sv_add_metric_batched(const double* points, const int32_t* P, int Pmax, const double* gt_pose,
                          const double* pred_pose, int B, double* add_out, sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N3  point-to-point ICP refinement (replaces utils/icp.py:13-83 = open3d registration_icp with
 *      TransformationEstimationPointToPoint; call sites app/inference_engine.py:358-362)
 *   src float32[S][3] (CAD model points), tgt float32[T][3] (end-effector crop), init_T double[16] row-major 4x4
 *   source->target (NULL = identity).  Correspondence = nearest target point within max_distance; update = Kabsch on
 *   the correspondences; stops when |d fitness| < rel_fitness and |d rmse| < rel_rmse between two evaluations or after
 *   max_iterations updates.  out_T double[16]; out_stats double[3] = {fitness, inlier rmse, updates applied}.
 *   Nearest neighbour: float32 squared distances of the transformed source point (transformed in float64, rounded to
 *   float32) to every target point; ties go to the lowest target index; a NaN distance never matches, so NaN or inf
 *   target or source points have no correspondence.  Inlier: d^2 <= (float)(max_distance^2), a point at exactly
 *   max_distance included.  fitness = inliers / S, rmse over the inliers (0 with none).  With fewer than 3 inliers the
 *   iteration stops with no update (0 inliers: out_T = init_T bit for bit).  A non-finite update makes T NaN.
 *   S in [3, 2^24), T in [1, 2^24), max_distance > 0, max_iterations >= 0.
 *   The whole iteration runs on the stream without host read-backs.
 * ------------------------------------------------------------------------------------------- */
size_t sv_icp_workspace_bytes(int64_t S);
int sv_icp_point2point(const float* src, int64_t S, const float* tgt, int64_t T, const double* init_T,
                       double max_distance, int max_iterations, double rel_fitness, double rel_rmse, void* workspace,
                       size_t workspace_bytes, double* out_T, double* out_stats, sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N3b  point-to-plane ICP refinement with device-side normal estimation (the registration the reference prepares but
 *      never runs: utils/icp.py:46-48 estimates normals on the crop with KDTreeSearchParamHybrid(radius=0.02,
 *      max_nn=30), :63 then passes the point-to-point estimator, which does not read them).  Opt-in; the definitions
 *      below follow Open3D's published algorithm, parity with Open3D binaries is by construction and unverified.
 *
 *   sv_estimate_normals: xyz float32[N][3] -> normals float32[N][3], counts int32[N] (or NULL).
 *   Neighbour set of point i: the points j (i included) whose float32 squared distance (dx*dx + dy*dy) + dz*dz (no fma,
 *   as sv_fps) is strictly below (float)(radius*radius); when more than max_nn qualify, the max_nn nearest, ties going
 *   to the lower index.  counts[i] = size of the set.  A point with a NaN or inf coordinate is nobody's neighbour, has
 *   an empty set and gets a NaN normal.  Fewer than 3 neighbours: normal (0, 0, 1).  Otherwise the covariance of the
 *   neighbours about their mean in float64 and the unit eigenvector of its smallest eigenvalue (float64 cyclic Jacobi),
 *   rounded to float32; sign: the stored component of largest magnitude is positive, the first on ties (as
 *   sv_quat_avg_batched; Open3D leaves the sign to its solver and point-to-plane does not depend on it).  Collinear or
 *   coincident neighbours: a unit vector orthogonal to the largest eigenvector.  The same cloud gives the same bits
 *   whatever the kernel's tiling.  N in [1, 2^20], radius > 0, max_nn in [3, 64];
 *   workspace: sv_normals_workspace_bytes(N, max_nn) - a fixed 256 bytes that the kernel currently does not use (its
 *   candidates stay in LDS); the size is still checked.
 *
 *   sv_icp_point2plane: arguments, nearest-neighbour rule, inlier rule, fitness, rmse (over point distances), stop rule,
 *   max_iterations, out_T and out_stats exactly as sv_icp_point2point; tgt_normals float32[T][3].  Update: for each
 *   inlier with p the source point under the current T (float64), q its target point and n that point's normal,
 *   r = (p - q).n, J = [p x n, n]; A = sum J J^T, b = sum J r (fixed summation order: repeated runs give the same bits);
 *   A x = -b by Cholesky in float64, x = (alpha, beta, gamma, t); T <- [Rz(gamma) Ry(beta) Rx(alpha) | t] T.
 *   An inlier whose normal is not finite counts towards fitness and rmse but adds nothing to A and b.  Fewer than 6
 *   contributing inliers, or a Cholesky pivot that is not positive and finite (e.g. all normals parallel), stop the
 *   iteration with no update (0 inliers: out_T = init_T bit for bit).  A non-finite x makes T NaN.
 *   workspace: sv_icp_point2plane_workspace_bytes(S).
 * ------------------------------------------------------------------------------------------- */
size_t sv_normals_workspace_bytes(int64_t N, int max_nn);
int sv_estimate_normals(const float* xyz, int64_t N, double radius, int max_nn, void* workspace, size_t workspace_bytes,
                        float* normals, int32_t* counts, sv_stream_t stream);
size_t sv_icp_point2plane_workspace_bytes(int64_t S);
int sv_icp_point2plane(const float* src, int64_t S, const float* tgt, const float* tgt_normals, int64_t T,
                       const double* init_T, double max_distance, int max_iterations, double rel_fitness,
                       double rel_rmse, void* workspace, size_t workspace_bytes, double* out_T, double* out_stats,
                       sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N3c  batched ICP: P registrations of one source cloud per call, independent or with one shared transform
 *      (beyond the reference, opt-in; additive, sv_abi_version() stays 4).
 *
 *   src float32[S][3], shared by the P problems.  pre double[P][16] (device) or NULL: with pre, the source point of
 *   problem p is pre_p . m, in float64 with the row expressions of T . x, never rounded to float32; NULL skips the
 *   multiply.  tgt float32[sum T_p][3]: the P target clouds concatenated; tgt_normals the same layout or NULL.
 *   NULL tgt_normals = the point-to-point update of N3, otherwise the point-to-plane update of N3b.  tgt_offsets is a
 *   HOST array int64[P + 1], ascending from 0, every T_p = tgt_offsets[p+1] - tgt_offsets[p] in [1, 2^24); it is
 *   validated on the host and travels as a kernel argument, so the call never waits for the device.
 *   P in [1, 64]; S, max_distance, max_iterations as N3.
 *
 *   shared == 0: P independent problems.  init_T double[P][16] (device) or NULL = identities; out_T double[P][16];
 *   out_stats double[P][3] = {fitness, rmse, updates} (or NULL).  Every problem has its own state and stops on its own;
 *   problem p's out_T and out_stats are, bit for bit, those of sv_icp_point2point / sv_icp_point2plane on
 *   (src, target p, init_T[p]) - the single calls are the P = 1 independent case - whatever else is in the call and
 *   whatever its order.
 *
 *   shared == 1: one transform T for all problems, minimising the pooled objective.  init_T double[16] or NULL; out_T
 *   double[16]; out_stats double[3 + 2 P] = pooled {fitness, rmse, updates}, then {fitness_p, rmse_p} of the last
 *   evaluation of every problem.  Each problem's sums (N3: n, sum p, sum q, sum p q^T, sum d^2; N3b: inliers,
 *   contributing inliers, sum d^2, A, b) are formed exactly as the single call forms them; the pooled sums are problem
 *   0's with problems 1 .. P-1 added in ascending order (no float atomics: repeated runs give the same bits, and P = 1
 *   without pre is the single call bit for bit).  Pooled fitness = sum_p inliers_p / (P S), pooled rmse =
 *   sqrt(sum d^2 / sum inliers); the stop rule and the no-update conditions (fewer than 3 inliers; fewer than 6
 *   contributing inliers; a bad pivot) are the single calls', applied to the pooled values; the update is Kabsch /
 *   Cholesky on the pooled sums.
 *
 *   Nearest-neighbour rule, inlier rule, max_iterations == 0, zero inliers (out_T = init_T bit for bit) and NaN handling
 *   as N3 / N3b.  Launches per call: 2 + (max_iterations + 1) * 2, or * 3 in shared mode, whatever P is; no read-back.
 *   workspace: sv_icp_batched_workspace_bytes(S, P).
 * ------------------------------------------------------------------------------------------- */
size_t sv_icp_batched_workspace_bytes(int64_t S, int P);
int sv_icp_batched(const float* src, int64_t S, const double* pre, const float* tgt, const float* tgt_normals,
                   const int64_t* tgt_offsets, int P, const double* init_T, int shared, double max_distance,
                   int max_iterations, double rel_fitness, double rel_rmse, void* workspace, size_t workspace_bytes,
                   double* out_T, double* out_stats, sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N3d  the ICP model from a triangle mesh: area-weighted surface samples and weighted sample elimination (the
 *      reference builds its model at start-up, app/inference_engine.py:56-57 -> utils/icp.py:13-40:
 *      read_triangle_mesh, sample_points_uniformly(16384), sample_points_poisson_disk(8192, pcl=...), keep x > 0).
 *      Additive, the ABI version stays 4.  The definitions restate Open3D's algorithm; Open3D draws from its own generator,
 *      so parity with Open3D binaries is by construction and unverified.  Everything is float64 and every operation
 *      rounds as written (no fma): a numpy restatement gives the same bits.
 *
 *   sv_mesh_sample: verts double[Nv][3], tris int32[F][3], draws double[N][3] = (u, r1, r2) in [0, 1) ->
 *   points double[N][3], normals double[N][3], tri int32[N], area double[1], counters int32[1].
 *   Per triangle: e1 = v1 - v0, e2 = v2 - v0, c = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x),
 *   len = sqrt((cx*cx + cy*cy) + cz*cz), a = 0.5*len.  A triangle with an index outside [0, Nv) has a = 0 and is counted
 *   in counters[0].  cdf[t] = a[0] + ... + a[t], added in ascending t (np.cumsum's order); area[0] = cdf[F-1].
 *   Per sample: t = the number of cdf entries <= u*area, clamped to F-1 (searchsorted, side "right": a draw on a boundary
 *   goes to the next triangle, zero-area triangles are never chosen); q = sqrt(r1), w0 = 1 - q, w1 = q*(1 - r2),
 *   w2 = q*r2; point = (w0*v0 + w1*v1) + w2*v2 and normal = c / len per component (the geometric normal of the
 *   triangle; vertex normals are not used); tri[s] = t.  Should the clamp land on a triangle with a bad index, that
 *   sample's point and normal are NaN.  area not finite or not > 0: tri = -1 and NaN points and normals for every sample.
 *   F in [1, 2^20], N in [1, 2^20], Nv >= 1; workspace: sv_mesh_sample_workspace_bytes(F).  4 launches, no read-back.
 *
 *   sv_sample_eliminate: weighted sample elimination (Yuksel 2015) as Open3D's SamplePointsPoissonDisk runs it.
 *   points double[N][3] -> kept int32[n_keep] (the survivors, ascending), order int32[N - n_keep] (the deleted indices
 *   in deletion order; may be NULL when n_keep == N), counters int32[1].
 *   Neighbours of i: the j != i with d2 = (dx*dx + dy*dy) + dz*dz < r_max*r_max, in ascending j; a NaN distance is no
 *   neighbour, so a non-finite point has none.  Pair weight: d = max(sqrt(d2), r_min), t = 1 - d/r_max,
 *   w = ((t*t)^2)^2 (alpha = 8 by three squarings).  weight[i] = the sum of w over the LIVE neighbours of i, added in
 *   ascending j.  While more than n_keep points live: delete the live point of largest weight (the lowest index on a
 *   tie), then sum again, from nothing, the weight of each of its live neighbours - so a weight never depends on the
 *   deletions before it.  counters[0] = the largest true neighbour count; when it exceeds max_degree the table rows
 *   were cut short, the loop is not run and kept / order are NOT valid: call again with a larger max_degree.
 *   N in [1, 65536], n_keep in [1, N], max_degree in [1, 1024], r_max finite and > 0, 0 <= r_min <= r_max;
 *   workspace: sv_sample_eliminate_workspace_bytes(N, max_degree) (the table is N * max_degree * 12 bytes).
 *   3 launches whatever N - n_keep is (one workgroup runs the whole loop), no read-back; repeated calls give the
 *   same bits.
 * ------------------------------------------------------------------------------------------- */
size_t sv_mesh_sample_workspace_bytes(int64_t F);
int sv_mesh_sample(const double* verts, int64_t Nv, const int32_t* tris, int64_t F, const double* draws, int64_t N,
                   void* workspace, size_t workspace_bytes, double* points, double* normals, int32_t* tri,
                   double* area, int32_t* counters, sv_stream_t stream);
size_t sv_sample_eliminate_workspace_bytes(int64_t N, int max_degree);
int sv_sample_eliminate(const double* points, int64_t N, int64_t n_keep, double r_max, double r_min, int max_degree,
                        void* workspace, size_t workspace_bytes, int32_t* kept, int32_t* order, int32_t* counters,
                        sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N3e  packed sensor records -> points, colours and source indices (the reference decodes a ROS PointCloud2 on the host,
 *      utils/ros_utils.py get_points_and_colors called by app/freenect_data_engine.py, and reads .pcd frames through
 *      Open3D, app/data_engine.py:161-204 PCDDataEngine with get_roi_mask).  A PointCloud2 `data` buffer and a binary PCD
 *      body are the same thing, a strided array of fixed-layout records, and one entry serves both.  Additive, the ABI
 *      version stays 4.  Every output equals a numpy restatement bit for bit; parity with sensor_msgs, PCL and Open3D is
 *      by construction and unverified.
 *
 *   sv_unpack_points: data uint8[data_bytes] (device, any alignment) -> points float32[n_records][3],
 *   rgb float32[n_records][3] (not touched and may be NULL when rgb_off < 0), src int32[n_records] (may be NULL),
 *   count int64[1].  Record i (0 <= i < n_records) starts at byte (i / width) * row_step + (i % width) * point_step.
 *   Field bytes: a field is the 4 (F32, rgb) or 8 (F64) bytes at record + offset, at any alignment, least significant
 *   byte first, or most significant first when SV_UNPACK_BIGENDIAN is set.
 *   Coordinates: SV_FIELD_F32 values are copied as bits (a kept NaN keeps its payload).  SV_FIELD_F64 values are tested
 *   for finiteness as doubles and then rounded to float32, round-to-nearest-even (np.copyto(float32, float64)): a finite
 *   double beyond FLT_MAX becomes +-inf and is still kept, a result below FLT_MIN is a denormal; a float64 NaN becomes
 *   sign | 0x7fc00000 | (the top 22 bits of its payload).
 *   Keep rule: a record is kept iff x, y and z are all finite, or SV_UNPACK_KEEP_NONFINITE is set; and, when box_host is
 *   given, lo[a] < (double)p32[a] < hi[a] on all three axes (strict bounds, get_roi_mask), p32 being the float32
 *   coordinate - a NaN coordinate fails it.  box_host is a HOST double[6] = lo x, y, z, hi x, y, z (or NULL); the six
 *   values travel as kernel arguments: no copy and no wait.
 *   Order: kept records are written in ascending record index, the order a boolean mask gives.  points[k] = the
 *   coordinates of the k-th kept record, src[k] = its record index, count[0] = the number kept; rows at or beyond
 *   count[0] are unspecified.
 *   Colour: v = the uint32 at rgb_off, whatever type the field declares (PCL stores the bits in a float field);
 *   r = (v >> 16) & 255, g = (v >> 8) & 255, b = v & 255; rgb[k] = (lut[r], lut[g], lut[b]) with lut a device float[256],
 *   or the byte values as floats when lut is NULL.
 *   Checked before any HIP call: n_records in [1, 2^24], width >= 1, point_step in [1, 4096],
 *   row_step >= width * point_step, xyz_type and flags known, every field inside the record, the x, y, z and rgb fields
 *   disjoint, data_bytes covering the last record, box bounds not NaN and lo <= hi, required pointers non-null,
 *   workspace >= sv_unpack_points_workspace_bytes(n_records).
 *   3 launches whatever n_records is (per-tile counts by ballot + popcount, one workgroup's exclusive scan, ordered
 *   write), no memset, no atomics, no read-back; repeated calls give the same bits.
 * ------------------------------------------------------------------------------------------- */
#define SV_FIELD_F32 7 /* the PointField datatype codes */
#define SV_FIELD_F64 8
#define SV_UNPACK_BIGENDIAN 1
#define SV_UNPACK_KEEP_NONFINITE 2
size_t sv_unpack_points_workspace_bytes(int64_t n_records);
int sv_unpack_points(const uint8_t* data, int64_t data_bytes, int64_t n_records, int64_t width, int64_t point_step,
                     int64_t row_step, int x_off, int y_off, int z_off, int xyz_type, int rgb_off, int flags,
                     const double* box_host, const float* lut, void* workspace, size_t workspace_bytes, float* points,
                     float* rgb, int32_t* src, int64_t* count, sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N3f  a depth image and a colour image -> a registered, coloured, unorganised cloud (the reference does this on the host,
 *      scripts/ycb_generate_point_cloud.py:127-274: filterDiscontinuities, registerDepthMap and
 *      registeredDepthMapToPointCloud, the last two as Python loops over every pixel).  Additive, the ABI version stays 4.
 *      Every output equals a numpy restatement bit for bit, and the filter, the registered map and the cloud equal the
 *      reference's own three functions on tests/golden/rgbd_ycb.npz; parity with depth_image_proc, librealsense and Open3D
 *      is by construction and unverified.
 *
 *   sv_rgbd_cloud: depth (device, any alignment) = Hd rows of Wd values, row v at byte v * depth_row_bytes, little-endian
 *   uint16 (SV_DEPTH_U16) or float32 (SV_DEPTH_F32); color (device, any alignment, or NULL) = Hc rows of Wc pixels of
 *   3 bytes r, g, b (b, g, r under SV_RGBD_BGR), row v at byte v * color_row_bytes; mask uint8[Hc * Wc] or NULL.
 *   -> points float32[Hc * Wc][3], points64 double[Hc * Wc][3] (may be NULL), rgb float32[Hc * Wc][3] (may be NULL only if
 *   color is; not touched then), src int32[Hc * Wc] (may be NULL), registered double[Hc * Wc] (may be NULL), count int64[1].
 *   cam_host is a HOST double[21]: depth fx, fy, cx, cy; colour fx, fy, cx, cy; the top three rows of the colour-from-depth
 *   transform H, row-major (12 values); depth_scale.  box_host is a HOST double[6] = lo x, y, z, hi x, y, z, or NULL.  Both
 *   travel as kernel arguments: no copy and no wait.
 *   ARITHMETIC: float64 throughout, every operation rounded on its own (no fused multiply-add) and in exactly the order
 *   and bracketing written below.  This order is the contract.
 *   Stage 1, filter (U16 only; off when filter_size == 0, else filter_size odd in 3..15): with o = filter_size / 2, pixel
 *   (v, u) with o <= v < Hd - o and o <= u < Wd - o becomes 0 iff max(mid - min, max - mid) > filter_thresh, min and max
 *   over the filter_size^2 window of RAW values, zeros included, compared as integers.  Border pixels never change; an
 *   image smaller than the window is unchanged.  d = (double)value * depth_scale.  F32: a value is valid iff it is finite
 *   and > 0, an invalid value counts as 0, and filter_size must be 0.
 *   Stage 2, register (skipped under SV_RGBD_ALIGNED, where registered[v][u] = d and the colour intrinsics are the ones
 *   used): for every depth pixel with d != 0
 *     x = ((u - cxd) * d) * (1.0 / fxd), y = ((v - cyd) * d) * (1.0 / fyd), z = d
 *     X = ((H00 * x + H01 * y) + H02 * z) + H03, Y and Z likewise from rows 1 and 2
 *     iz = 1.0 / Z, uu = (fxc * X) * iz + cxc, vv = (fyc * Y) * iz + cyc
 *     ui = trunc(uu + 0.5), vi = trunc(vv + 0.5): toward zero, as Python's int(), so uu in (-1.5, -0.5) lands on pixel 0
 *   the candidate is dropped when ui or vi is not finite or lies outside [0, Wc) x [0, Hc), or when Z is not a positive
 *   finite number; registered[vi][ui] = the LARGEST candidate Z (the reference's `>` against a zero-initialised map), the
 *   smallest under SV_RGBD_NEAREST, 0 where none lands.  The z-buffer is a 64-bit integer atomic max / min on the bit
 *   pattern of the positive double: the order of arrival cannot show and repeated calls give the same bits.
 *   Stage 3, cloud: colour pixel j = v * Wc + u with r = registered[v][u] is kept iff r > 0, and mask is NULL or
 *   mask[j] == 0, and, when box_host is given, lo[a] < (double)p32[a] < hi[a] on all three axes (strict, as
 *   sv_unpack_points).  points64 = (((u - cxc) * r) * (1.0 / fxc), ((v - cyc) * r) * (1.0 / fyc), r); points = p32 = the
 *   same rounded to float32, nearest-even; rgb[k] = lut[byte] per channel in r, g, b order (lut a device float[256]), or
 *   the byte as a float when lut is NULL; src[k] = j.  Kept pixels are written in ascending j; count[0] = their number;
 *   rows at or beyond it are unspecified.
 *   Checked before any HIP call: dimensions >= 1 and Hd * Wd, Hc * Wc <= 2^24; row bytes covering a row; depth_type and
 *   flags known; the filter rules above and filter_thresh >= 0; every cam_host value finite, the four focal lengths and
 *   depth_scale non-zero; SV_RGBD_ALIGNED with Hd, Wd == Hc, Wc; box bounds not NaN and lo <= hi; required pointers
 *   non-null; workspace >= sv_rgbd_cloud_workspace_bytes(Hd, Wd, Hc, Wc).
 *   5 launches whatever the images hold (z-buffer clear; filter + project, the window staged through an LDS tile with
 *   halo; per-tile counts; one workgroup's scan; ordered write), no read-back.
 * ------------------------------------------------------------------------------------------- */
#define SV_DEPTH_U16 4 /* the PointField datatype codes */
#define SV_DEPTH_F32 7
#define SV_RGBD_ALIGNED 1
#define SV_RGBD_NEAREST 2
#define SV_RGBD_BGR 4
size_t sv_rgbd_cloud_workspace_bytes(int64_t Hd, int64_t Wd, int64_t Hc, int64_t Wc);
int sv_rgbd_cloud(const void* depth, int depth_type, int64_t Hd, int64_t Wd, int64_t depth_row_bytes,
                  const uint8_t* color, int64_t Hc, int64_t Wc, int64_t color_row_bytes,
                  const uint8_t* mask, const double* cam_host, int filter_size, int filter_thresh, int flags,
                  const double* box_host, const float* lut, void* workspace, size_t workspace_bytes,
                  float* points, double* points64, float* rgb, int32_t* src, double* registered,
                  int64_t* count, sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N3g  lens distortion for the RGB-D ingest: the plumb-bob (5 coefficients) and rational (8) models of OpenCV and of a ROS
 *      CameraInfo.  Additive, the ABI version stays 4.  Every output equals a numpy restatement bit for bit; agreement with
 *      cv2.projectPoints, cv2.undistortPoints and image_proc is by construction and unverified.
 *
 *   Coefficients D = (k1, k2, p1, p2, k3, k4, k5, k6), the OpenCV / ROS order; shorter sets are zero-padded by the caller.
 *   ARITHMETIC: float64 throughout, every operation rounded on its own (no fused multiply-add) and in exactly the order
 *   and bracketing written below.  This order is the contract.
 *   Forward model F(a, b): a normalised direction (a, b) -> the distorted normalised point (xd, yd)
 *     r2  = a*a + b*b
 *     num = 1.0 + ((k3*r2 + k2)*r2 + k1)*r2
 *     den = 1.0 + ((k6*r2 + k5)*r2 + k4)*r2
 *     c   = num / den
 *     dx  = (2.0*p1)*(a*b) + p2*(r2 + 2.0*(a*a))
 *     dy  = p1*(r2 + 2.0*(b*b)) + (2.0*p2)*(a*b)
 *     xd  = a*c + dx
 *     yd  = b*c + dy
 *   Ray table of a camera (fx, fy, cx, cy, D, H, W), the inverse model, per pixel (v, u):
 *     x0 = (u - cx)*(1.0/fx), y0 = (v - cy)*(1.0/fy), x = x0, y = y0
 *     exactly 64 rounds, no early exit, of
 *       r2 = x*x + y*y
 *       ic = (1.0 + ((k6*r2 + k5)*r2 + k4)*r2) / (1.0 + ((k3*r2 + k2)*r2 + k1)*r2)
 *       dx, dy as above, at (x, y)
 *       x = (x0 - dx)*ic, y = (y0 - dy)*ic
 *     (xd, yd) = F(x, y); the pixel is VALID iff |(fx*xd + cx) - u| <= 1e-6 and |(fy*yd + cy) - v| <= 1e-6 (a NaN fails).
 *     A valid pixel stores (x, y), an invalid one (NaN, NaN).
 *   (OpenCV's default inverse stops after 5 rounds: 1.7e-2 px off on the reference's Kinect 1 colour lens and 2 px off on
 *   an Azure-Kinect-like rational depth lens; 64 rounds end below 1e-11 px on both.)
 *   The table is double[H * W * 2 + 1], pixel j = v * W + u at [2j], [2j + 1]; the last element is r2_max, the largest
 *   x*x + y*y over the valid pixels, 0 when none is valid.
 *
 *   sv_lens_rays: cam_host = HOST double[4] fx, fy, cx, cy; dist_host = HOST double[8]; rays = DEVICE double[H*W*2 + 1].
 *   Two launches: r2_max cleared, then one thread per pixel; r2_max is reduced per wave and workgroup and then by a 64-bit
 *   integer atomic max on the bit pattern (no float atomics): repeated calls give the same bits.  Checked before any HIP
 *   call: H, W >= 1 and H * W <= 2^24, all twelve values finite, fx and fy non-zero, pointers non-null.
 *
 *   sv_rgbd_cloud_lens: sv_rgbd_cloud (N3f) with three more arguments, each of which may be NULL = "pinhole for that part,
 *   with exactly sv_rgbd_cloud's arithmetic"; with all three NULL every output has sv_rgbd_cloud's bits.  The workspace is
 *   sv_rgbd_cloud_workspace_bytes.
 *     depth_rays  DEVICE table of the depth camera [Hd x Wd].  Stage 2: x = rx*d, y = ry*d, z = d with (rx, ry) the depth
 *                 pixel's ray.  A NaN ray makes X, Y, Z NaN, which the existing rule drops.
 *     color_rays  DEVICE table of the colour camera [Hc x Wc].  Stage 3: colour pixel j is kept only if its ray is valid
 *                 (and the conditions of N3f hold); points64 = (rx*r, ry*r, r).
 *     color_dist_host  HOST double[8] of the colour camera; needs color_rays.  Stage 2: a = X*iz, b = Y*iz,
 *                 (xd, yd) = F(a, b), uu = fxc*xd + cxc, vv = fyc*yd + cyc; rounding and range rules as in N3f.  The
 *                 candidate is dropped unless a*a + b*b <= r2_max of color_rays (a failed comparison, NaN included, drops
 *                 it): a rational model is not monotonic, and a point far outside the field of view can fold back into
 *                 the image.  LIMIT: the bound is radial, so a point beyond an image edge but inside the corner radius is
 *                 not caught.
 *   SV_RGBD_ALIGNED uses color_rays only; depth_rays and color_dist_host must be NULL.  Checked before any HIP call: N3f's
 *   list, these two rules, and the color_dist_host values finite.  Five launches, no read-back; the pinhole kernels take the
 *   arguments they took before and read no table.
 * ------------------------------------------------------------------------------------------- */
int sv_lens_rays(const double* cam_host, const double* dist_host, int64_t H, int64_t W, double* rays, sv_stream_t stream);
int sv_rgbd_cloud_lens(const void* depth, int depth_type, int64_t Hd, int64_t Wd, int64_t depth_row_bytes,
                       const uint8_t* color, int64_t Hc, int64_t Wc, int64_t color_row_bytes,
                       const uint8_t* mask, const double* cam_host, int filter_size, int filter_thresh, int flags,
                       const double* box_host, const float* lut, void* workspace, size_t workspace_bytes,
                       float* points, double* points64, float* rgb, int32_t* src, double* registered,
                       int64_t* count, const double* depth_rays, const double* color_rays,
                       const double* color_dist_host, sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N4  point-matching pose losses with their gradients (replace the per-instance Python loops of utils/loss.py:166-188
 *      compute_pose_loss, :190-209 compute_shape_match_loss, :211-227 compute_pose_match_loss, :229-249
 *      compute_kp_pose_match_loss; call sites train.py:89,189 and train_kp_to_pose.py:297).  Additions of ABI 4.
 *
 *   points float32[M][3]; instance b owns rows offsets[b] .. offsets[b+1]-1 (offsets int32[B+1], as sv_batch_offsets
 *   writes it: non-decreasing, inside [0, M]; anything else is clamped into [0, M] so that no access leaves the arrays,
 *   with unspecified results).  weights float32[M] or NULL (= 1); mask uint8[M] or NULL (= all rows): a row whose mask
 *   byte is 0 contributes nothing, whatever its point and weight hold, and is nobody's match.  R, R_pred float32[B][9]
 *   row-major (target, prediction); t, t_pred float32[B][3], both given or both NULL (= no translation).
 *   With n_b the number of unmasked rows of instance b, p_j such a row, a_j = R_pred[b] p_j (+ t_pred[b]) and
 *   b_j = R[b] p_j (+ t[b]):
 *     SV_LOSS_POSE           r_j = a_j - b_j                                  loss[b] = sum_j w_j^2 |r_j|^2 / (2 n_b)
 *     SV_LOSS_SHAPE_MATCH    r_j = a_j - b_k*, k* = argmin_k |a_j - b_k|^2 over the instance's unmasked rows, ties to
 *                            the lowest k                                     loss[b] = sum_j w_j^2 |r_j|^2 / (2 n_b)
 *     SV_LOSS_POSE_MATCH     r_j = a_j - b_j                                  loss[b] = sum_j |r_j|_1 / n_b
 *     SV_LOSS_KP_POSE_MATCH  r_j = a_j - b_j                                  loss[b] = sum_j w_j^2 |r_j|^2 / (2 n_b)
 *   (the reference calls POSE and SHAPE_MATCH without a translation and without weights, POSE_MATCH and KP_POSE_MATCH
 *   with the translation, KP_POSE_MATCH with weights; POSE_MATCH with weights is refused.)
 *   grad_R float32[B][9] = d loss[b] / d R_pred[b] = sum_j g_j p_j^T / n_b and grad_t float32[B][3] =
 *   d loss[b] / d t_pred[b] = sum_j g_j / n_b, with g_j = w_j^2 r_j for the squared terms and sign(r_j), sign(0) = 0,
 *   for the L1 term; k* is a constant of the differentiation; either may be NULL, grad_t must be NULL when t is.
 *   match int32[M] or NULL, SHAPE_MATCH only: k* of every row of an instance, relative to the instance's first row
 *   (-1 for a masked-out row and for a row whose distances are all NaN).
 *   Arithmetic: the float32 inputs are promoted to float64; transforms ((R0 x + R1 y) + R2 z, then + t), distances
 *   ((dx^2 + dy^2) + dz^2, the search included), terms and sums are float64 without fma; loss, grad_R and grad_t are
 *   the float64 results rounded once to float32.  Sums run in a fixed order without atomics: the same inputs give the
 *   same bits, and identical poses (R_pred = R, t_pred = t bit for bit) give exactly 0 everywhere.
 *   n_b = 0 gives NaN for that instance's loss and gradients (the reference's 0 / 0).  A NaN or inf among an instance's
 *   unmasked inputs makes that instance's outputs non-finite and changes no bit of any other instance.
 *   B in [1, SV_MAX_BATCH], M in [0, 2^24); a bad mode, a null pointer, t without t_pred or a short workspace is refused
 *   on the host before any HIP call.  workspace: sv_pose_loss_workspace_bytes(M, B).  No host read-back.
 * ------------------------------------------------------------------------------------------- */
#define SV_LOSS_POSE 0
#define SV_LOSS_SHAPE_MATCH 1
#define SV_LOSS_POSE_MATCH 2
#define SV_LOSS_KP_POSE_MATCH 3
size_t sv_pose_loss_workspace_bytes(int64_t M, int B);
int sv_pose_match_loss(const float* points, const int32_t* offsets, int64_t M, int B, const float* weights,
                       const uint8_t* mask, const float* R, const float* t, const float* R_pred, const float* t_pred,
                       int mode, void* workspace, size_t workspace_bytes, float* loss, float* grad_R, float* grad_t,
                       int32_t* match, sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N5  training-time augmentation and batched quantisation (replace utils/augmentation.py:14-33 distort_elastic, :49-75
 *      add_noise / transform_random / flip_random / rotate_along_gravity, :108-138 augment_segmentation, called per
 *      frame at data/alivev2.py:273-279, and the centring + ME.utils.sparse_quantize + collate that follow it,
 *      data/alivev2.py:199-208,290-296,358-365).  Additions of ABI 4.  The random draws are the caller's: nothing here
 *      draws a number, so the same arguments give the same bits.
 *
 * sv_elastic_field: the blurred displacement fields of distort_elastic:15-26.  raw, out float32: F fields one after the
 *   other, field f being [3][bx][by][bz] with (bx, by, bz) = dims[3f .. 3f+2]; dims is a HOST array (int32[F][3]), every
 *   entry in [3, 1024], F in [1, 2 * SV_MAX_BATCH].  Each component goes through six 3-tap box blurs along axes 0, 1, 2,
 *   0, 1, 2 with zero padding (scipy.ndimage.convolve, mode='constant', cval=0): one pass computes
 *   (a*w + b*w) + c*w in float64 with w = (double)(float)(1/3) and rounds once to float32, as scipy does, so the second
 *   blur along an axis sees the first one's rounded, truncated result.  out must not alias raw.
 *   workspace: sv_elastic_field_workspace_bytes(dims, F) (0 for arguments the call would refuse).
 *
 * sv_augment_points: points float32[N][3] (float64[N][3] with points_f64 != 0, for a caller that chains calls: the
 *   reference's intermediate clouds are float64) of B frames, frame b owning rows offsets[b] .. offsets[b+1]-1 (int32[B+1],
 *   non-decreasing inside [0, N]; anything else is clamped so that no access leaves the arrays).  table is
 *   float64[B][SV_AUG_STRIDE] on the device, one row per frame (integers stored as float64):
 *     SV_AUG_ELASTIC0 / SV_AUG_ELASTIC1 + SV_AUG_E_ON      stage enabled (0 / 1)
 *                                       + SV_AUG_E_OFFSET  index in `fields` of the stage's field's first float
 *                                       + SV_AUG_E_BX..BZ  its shape        + SV_AUG_E_GRAN, SV_AUG_E_MAG
 *     SV_AUG_NOISE_ON, SV_AUG_NOISE_SIGMA, SV_AUG_NOISE_CLIP
 *     SV_AUG_TRANSFORM_ON, SV_AUG_ROT (9, row-major), SV_AUG_TRANSLATION (3)
 *     SV_AUG_FLIP_SIGN     0 = off, else the factor of x (+1 / -1)
 *     SV_AUG_GRAVITY_ON, SV_AUG_GRAVITY_ANGLE (informative), SV_AUG_GRAVITY_COS, SV_AUG_GRAVITY_SIN (host cos / sin)
 *   fields float32[fields_len]: the output of sv_elastic_field (may be NULL with fields_len = 0 when no stage is on);
 *   noise float64[N][3] standard normal draws or NULL (then no frame gets noise).  Every step is float64 without fma, in
 *   the reference's order:
 *     elastic stage: p += mag * g(p), g = trilinear interpolation of the three components on the axes
 *       np.linspace(-(b-1)*gran, (b-1)*gran, b) (nodes k * step + start, the last one = stop), cell k with
 *       node(k) <= v < node(k+1), the upper edge inclusive, weights ((1 * wx) * wy) * wz summed in scipy's corner order;
 *       a point outside the grid on any axis gets exactly zero displacement, a NaN coordinate makes its row NaN; the
 *       second stage is evaluated at the positions the first produced.  A table row whose field does not lie inside
 *       [0, fields_len) makes its frame's rows NaN instead of reading outside the buffer.
 *     noise: p + clip(sigma * n, -clip, clip)
 *     transform: (p @ rot + translation) @ rot^T, both products computed
 *     flip: p @ diag(sign, 1, 1);  gravity: p @ [[c, 0, -s], [0, 1, 0], [s, 0, c]]^T, as full three-term products
 *   out float64[N][3]; stats float64[B][6] = per-frame (min x, y, z, max x, y, z) of out, NaN if the column holds one
 *   (numpy's min / max), (+inf, -inf) for a frame without rows.  B in [1, SV_MAX_BATCH], N in [0, 2^29).
 *   workspace: sv_augment_points_workspace_bytes(N, B).
 *
 * sv_quantise_points: points float64[N][3] and offsets as above; stats as sv_augment_points wrote it.  origin selects what
 *   is subtracted from frame b's rows first: SV_ORIGIN_NONE nothing, SV_ORIGIN_CENTER (max + min) / 2
 *   (utils/preprocess.py:8-11), SV_ORIGIN_BASE min (:14-17) - read from stats on the device.  coords int32[N][4] =
 *   (b, floor(p / quantization_size)) with the float64 division and floor of ME.utils.sparse_quantize, 16-byte aligned;
 *   a NaN, an inf or a quotient outside int32 gives INT32_MIN, which sv_voxelize reports as out of range.
 *   shifted float32[N][3] or NULL: the shifted points rounded once; shift_out float64[B][3] or NULL: what was subtracted.
 *
 * All three validate on the host before any HIP call and never read back.
 * ------------------------------------------------------------------------------------------- */
#define SV_AUG_STRIDE 40
#define SV_AUG_ELASTIC0 0
#define SV_AUG_ELASTIC1 7
#define SV_AUG_E_ON 0
#define SV_AUG_E_OFFSET 1
#define SV_AUG_E_BX 2
#define SV_AUG_E_BY 3
#define SV_AUG_E_BZ 4
#define SV_AUG_E_GRAN 5
#define SV_AUG_E_MAG 6
#define SV_AUG_NOISE_ON 14
#define SV_AUG_NOISE_SIGMA 15
#define SV_AUG_NOISE_CLIP 16
#define SV_AUG_TRANSFORM_ON 17
#define SV_AUG_ROT 18
#define SV_AUG_TRANSLATION 27
#define SV_AUG_FLIP_SIGN 30
#define SV_AUG_GRAVITY_ON 31
#define SV_AUG_GRAVITY_ANGLE 32
#define SV_AUG_GRAVITY_COS 33
#define SV_AUG_GRAVITY_SIN 34
#define SV_ORIGIN_NONE 0
#define SV_ORIGIN_CENTER 1
#define SV_ORIGIN_BASE 2
size_t sv_elastic_field_workspace_bytes(const int32_t* dims, int F);
int sv_elastic_field(const float* raw, const int32_t* dims, int F, void* workspace, size_t workspace_bytes, float* out,
                     sv_stream_t stream);
size_t sv_augment_points_workspace_bytes(int64_t N, int B);
int sv_augment_points(const void* points, int points_f64, const int32_t* offsets, int64_t N, int B, const double* table,
                      const float* fields, int64_t fields_len, const double* noise, void* workspace,
                      size_t workspace_bytes, double* out, double* stats, sv_stream_t stream);
int sv_quantise_points(const double* points, const int32_t* offsets, int64_t N, int B, const double* stats, int origin,
                       double quantization_size, int32_t* coords, float* shifted, double* shift_out, sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N6  per-frame training labels synthesised from the frame's pose (replace utils/data.py:58-103 get_roi_mask / get_ee_idx,
 *      :106-122 get_ee_cross_section_idx with utils/transformation.py:138-160, :125-335 get_closest_point / get_key_points /
 *      get_6_key_points, :338-342 collect_closest_points and the label write of data/alivev2.py:212-238), for a batch of
 *      frames per call.  Additions of ABI 4.
 *
 * Common arguments: points float32[N][3] (float64[N][3] with points_f64 != 0) of B frames, frame b owning rows
 *   offsets[b] .. offsets[b+1]-1 (int32[B+1] on the device, non-decreasing inside [0, N]; anything else is clamped so that
 *   no access leaves the arrays; a frame without rows is legal everywhere); pos float64[B][3] and rot float64[B][9]
 *   (row-major get_quaternion_rotation_matrix of the frame's quaternion, computed on the host) on the device.
 *   B in [1, SV_MAX_BATCH], N in [0, 2^29).  Every entry validates on the host before any HIP call, launches on the stream
 *   and never waits or reads back.  No atomics: the same arguments give the same bits.
 *
 * dtype rules (numpy's promotion in the reference, float64 pose):
 *   get_ee_idx                 float64 throughout: d = (double)p - pos, q = R^T d
 *   get_key_points / get_6_..  float64 throughout: q = R^T (double)p - R^T pos (the position is rotated with the points
 *                              and subtracted afterwards, center_at_origin of one row)
 *   get_ee_cross_section_idx   the in-place `-= pose[:3]` rounds d to the points' dtype: d = (T)((double)p - pos), then
 *                              q = R^T (double)d and the line distance in float64
 *   collect_closest_points     entirely in the points' dtype T: difference, squares, (a + b) + c, sqrt, compare against (T)thr
 *   Products R^T v and R v are three-term sums (a + b) + c without fma; norms are sqrt((x^2 + y^2) + z^2).
 *
 * sv_ee_mask: mask uint8[N] = 1 where q = R^T (p - pos) satisfies q.x > -500 and the six strict inequalities of
 *   get_roi_mask against box = HOST float64[6] (min_x, max_x, min_y, max_y, min_z, max_z; NULL: the reference's ee_dim_init
 *   -0.05, 0.05, -0.11, 0.11, -0.006, 0.12).  A row with a NaN is outside; a row no frame owns gets 0.
 *
 * sv_key_points: mode 10 = get_key_points, mode 6 = get_6_key_points; K = mode.  key_points float64[B][K][3] in the
 *   camera frame, kp_idx int64[B][K] = index within the frame or ignore_label (< 0).  Every search is an arg-min over
 *   (distance, index) on the rows a mask selects: numpy argmin's rule (a NaN distance wins at its first index, a tie goes
 *   to the lower index); a thresholded search finds its key point when that distance < euclidean_threshold.
 *   mode 10: P1-P4 on q.x > 0.005 (found: the key point moves to the row and its back-side twin to row + (-0.04 | -0.03,
 *   0, 0)); P7-P10 on q.x < -0.01 against the moved twins; the gripper pair on q.z > 0.08 with q.y > 0 / < 0 against
 *   (0, +-0.01, max z of the selection), no threshold; a missing gripper side mirrors the other one, both get the larger
 *   z; then + R^T pos and R @.  mode 6: the rows nearest the four box corners on (q.x > -0.005) and (q.z < 0.09), kept
 *   when within the threshold of the template key point; the same gripper pair.
 *   kp_idx of a gripper key point is what the reference records (:227, :239), not the row the coordinates come from: the
 *   winner's position within its side's subset, looked up in the list of all rows with q.z > 0.08.
 *   Where the reference fails, defined here: an empty selection of a search means "not found" (index ignore_label, the
 *   template coordinates kept; get_key_points raises a TypeError on an empty front side); mode 6 with an empty selection
 *   gives the template key points (carried to the camera frame like any result) and ignore_label everywhere, and
 *   selection_empty[b] = 1 (int32[B], may be NULL; 0 otherwise) so that a caller can return the reference's empty arrays.
 *
 * sv_line_topk: get_ee_cross_section_idx / select_closest_points_to_line.  dist(q) = ||(lp1 + t d) - q||,
 *   t = (q - lp1) . d, d = (lp1 - lp2) / ||lp1 - lp2|| (compute_dists_to_line; lp1, lp2 HOST float64[3], distinct and
 *   finite).  Per frame the `count` (1..1024) smallest distances in ascending order, a tie to the lower index, cut at the
 *   first that is not < cutoff (a NaN distance never qualifies): idx int64[B][count] (index within the frame, padded with
 *   -1), dist float64[B][count] (padded with +inf), n_sel int32[B].  workspace: sv_line_topk_workspace_bytes(N).
 *
 * sv_radius_labels: labels int64[N]: row i of frame b gets the largest k < K (1..64) whose anchor row kp_idx[b][k]
 *   (int64[B][K], index within the frame; negative or >= the frame's length: takes no part) lies at distance
 *   < euclidean_threshold, computed in the points' dtype; no such k (or a row no frame owns): ignore_label (< 0).
 * ------------------------------------------------------------------------------------------- */
int sv_ee_mask(const void* points, int points_f64, const int32_t* offsets, int64_t N, int B, const double* pos,
               const double* rot, const double* box, uint8_t* mask, sv_stream_t stream);
int sv_key_points(const void* points, int points_f64, const int32_t* offsets, int64_t N, int B, const double* pos,
                  const double* rot, int mode, double euclidean_threshold, int64_t ignore_label, double* key_points,
                  int64_t* kp_idx, int32_t* selection_empty, sv_stream_t stream);
size_t sv_line_topk_workspace_bytes(int64_t N);
int sv_line_topk(const void* points, int points_f64, const int32_t* offsets, int64_t N, int B, const double* pos,
                 const double* rot, const double* lp1, const double* lp2, int count, double cutoff, void* workspace,
                 size_t workspace_bytes, int64_t* idx, double* dist, int32_t* n_sel, sv_stream_t stream);
int sv_radius_labels(const void* points, int points_f64, const int32_t* offsets, int64_t N, int B, const int64_t* kp_idx,
                     int K, double euclidean_threshold, int64_t ignore_label, int64_t* labels, sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N7  segmentation criterion and step metrics (replace nn.CrossEntropyLoss(ignore_index, reduction) on out.features of
 *      train_segmentation.py / train_vote.py / train_key_points.py, compute_accuracies of train_segmentation.py:34-46 and
 *      train_vote.py:35-45, and the per-frame vote sort of compute_center_dists, train_vote.py:48-65).  Additions of ABI 4.
 *
 * Common arguments: B frames, frame b owning the consecutive rows offsets[b] .. offsets[b+1]-1 (int32[B+1] on the
 *   device, non-decreasing).  B in [1, SV_MAX_BATCH], N in [0, 2^31); N = 0 is valid.  Both entries validate on the host
 *   before any HIP call (a workspace below *_workspace_bytes is one of the argument errors, SV_ERR_INVALID), launch on the
 *   stream and never wait or read back; the same arguments give the same bits.
 *
 * sv_seg_criterion: one pass over logits float32[N][ld] (columns 0 .. C-1, 1 <= C <= 32 - the limit of
 *   sv_key_point_predictions -, ld >= C) and labels int64[N].
 *   Row loss  lse(x) - x[y],  lse = m + log(sum_c exp(x_c - m)),  m = the row maximum, everything in float64 from the
 *   float32 logits.  A row with a NaN logit gives NaN, and so does a row that holds +inf (inf - inf), both as torch's
 *   log-softmax.
 *   sums float64[2] = (sum of the row losses over the counted rows, number of counted rows).  The sum is taken in float64
 *   in an order that depends on (N, B, C) only, never on scheduling; no floating-point atomics.  The reduction ("mean":
 *   sums[0] / sums[1], 0 / 0 = NaN as torch; "sum": sums[0]) is the caller's.
 *   grad float32[N][C] dense (may be NULL): the UNSCALED softmax(x) - onehot(y) of a counted row (the label's column as
 *   -(sum of the other columns' exp) / sum, which does not cancel), 0 for an ignored row; the caller's backward multiplies
 *   by the reduction's factor and the incoming gradient, so the kernel needs no second pass to learn the count.
 *   pred = torch's max(1), the rule of sv_slice_argmax: the first index among equal maxima; the first NaN of a row is its
 *   maximum.  confusion int64[B][C][C] (may be NULL): [b][gt][pred] over the counted rows of frame b.
 *   label == ignore_index: the row is not counted, its gradient row is 0, it adds one to n_rows_ignored[b] (int64[B], may
 *   be NULL) and appears in no confusion cell.
 *   Any other label outside [0, C): the row is not counted, its gradient row is NaN and n_invalid[0] (int32) goes up by
 *   one; nothing faults (torch device-asserts here).  A caller turns n_invalid != 0 into a NaN loss.
 *   Rows before offsets[0] or at or after offsets[B] count for sums and grad but belong to no frame.
 *   Integer counts use LDS and global integer atomics (integer addition is order-free).
 *   workspace: sv_seg_criterion_workspace_bytes(N, B, C).
 *
 * sv_segment_topk: the per-frame form of sv_topk_indices on x[i * ld], i < N: idx int64[B][k] = row within the frame of
 *   its j-th largest x, padded with -1 when the frame has fewer than k rows (an empty frame: all -1).  sv_topk_indices'
 *   order: ties go to the lower row, NaN sorts above +inf; frame by frame the result equals sv_topk_indices on that frame's
 *   rows alone.  1 <= k <= 64, ld >= 1; offsets outside [0, N] are clamped so that no access leaves x.
 *   workspace: sv_segment_topk_workspace_bytes(N, B, k) (k keys per frame and 4096-row chunk of x).
 * ------------------------------------------------------------------------------------------- */
size_t sv_seg_criterion_workspace_bytes(int64_t N, int B, int C);
int sv_seg_criterion(const float* logits, int64_t ld, int C, int64_t N, const int64_t* labels, int64_t ignore_index,
                     const int32_t* offsets, int B, void* workspace, size_t workspace_bytes, double* sums, float* grad,
                     int64_t* confusion, int64_t* n_rows_ignored, int32_t* n_invalid, sv_stream_t stream);
size_t sv_segment_topk_workspace_bytes(int64_t N, int B, int k);
int sv_segment_topk(const float* x, int64_t ld, int64_t N, const int32_t* offsets, int B, int k, void* workspace,
                    size_t workspace_bytes, int64_t* idx, sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * A8  PointNet++ sampling / grouping / set abstraction (replace model/pointnet2_utils.py:65-86 farthest_point_sample,
 *      :89-109 query_ball_point, :178-204 the set abstraction's shared MLP + max, utils/data.py:13-34 numpy FPS)
 * ------------------------------------------------------------------------------------------- */
/* xyz float32[B][N][3]; start int64[B] first centroid (the reference draws it at random: pass it in);
 * out int64[B][S].  Distances are float32 ((dx*dx + dy*dy) + dz*dz, no fma), argmax = first maximum. */
int sv_fps(const float* xyz, int B, int N, int S, const int64_t* start, int64_t* out, sv_stream_t stream);
/* out int64[B][S][nsample]: the first nsample indices n (ascending) with ||xyz[n]-new_xyz[s]||^2 <= r^2,
 * padded with the first hit (r^2 = (float)(radius*radius), as torch compares a float32 tensor with the python
 * scalar radius**2); the distance uses the reference's expanded form (-2ab + a^2 + b^2) in float32.  A point is a hit
 * when NOT (d > r^2), so a NaN distance is a hit.  An empty ball (no hit at all) yields the index N in all nsample
 * entries, as the reference does: an index outside the cloud, which sv_pointnet_sa[_msg] and sv_group_rows turn into a NaN
 * row (never pass it to a plain gather). */
int sv_ball_query(const float* xyz, const float* new_xyz, int B, int N, int S, double radius, int nsample,
                  int64_t* out, sv_stream_t stream);
/* The R ball queries of one PointNetSetAbstractionMsg layer (model/pointnet2_utils.py:242-244, query_ball_point per radius
 * over the same centroids) in one scan over the cloud: out[r] int64[B][S][nsamples[r]] is exactly sv_ball_query with
 * (radii[r], nsamples[r]) - the same float32 distance, r^2 = (float)(radius*radius), ascending order and first-hit
 * padding, and the index N in every entry of an empty ball.  radii, nsamples and out are HOST arrays of R entries (out:
 * device pointers); the radii need not be sorted.
 * Returns SV_ERR_UNSUPPORTED (nothing launched) when R is outside 1..SV_BQ_MAX_RADII. */
#define SV_BQ_MAX_RADII 4
int sv_ball_query_multi(const float* xyz, const float* new_xyz, int B, int N, int S, int R, const double* radii,
                        const int* nsamples, int64_t* const* out, sv_stream_t stream);
/* PointNetFeaturePropagation's interpolation (model/pointnet2_utils.py:298-305): out[b][n][:] = sum over the three
 * nearest xyz2 points of points2 rows weighted by 1 / (d + 1e-8), normalised; d in the reference's expanded float32
 * form, nearest first, ties to the lower index.  xyz1 float32[B][N][3], xyz2 [B][S][3] (S >= 3), points2 [B][S][C],
 * out [B][N][C]. */
int sv_three_nn_interpolate(const float* xyz1, const float* xyz2, const float* points2, int B, int N, int S, int C,
                            float* out, sv_stream_t stream);
/* Farthest-point sampling of G clouds of different lengths in one launch (the end-effector crops of a group of frames,
 * utils/data.py:13-34 per crop): cloud g = xyz rows offsets[g] .. offsets[g + 1], its out_offsets[g + 1] - out_offsets[g]
 * samples go to out[out_offsets[g] ..] as indices relative to the cloud's first row, start[g] = its first centroid.
 * offsets, out_offsets, start: DEVICE arrays (G + 1, G + 1, G entries); max_n (host) >= the longest cloud, at most 38400
 * (sv_fps's limit; a longer cloud is read as its first max_n points).  Arithmetic and tie rule of sv_fps: cloud by cloud
 * the result of sv_fps on that cloud alone. */
int sv_fps_segmented(const float* xyz, const int64_t* offsets, const int64_t* out_offsets, const int64_t* start, int G,
                     int max_n, int64_t* out, sv_stream_t stream);
/* PointNetSetAbstraction.forward in eval mode after sampling and ball query (model/pointnet2_utils.py:178-204, grouping of
 * :112-140) as one launch: for every centroid q = (b, s) and neighbour j the row [xyz[b][i] - new_xyz[b][s], points[b][i]]
 * with i = group_idx[b][s][j] goes through L shared-MLP layers y = relu(fmaf(x @ W_l, scale_l, shift_l)) (Conv 1x1 + bias +
 * BatchNorm folded: scale = gamma / sqrt(var + eps), shift = beta + (bias - mean) * scale), then out[b][s][c] = max over
 * the nsample rows.  xyz float32[B][N][3], points float32[B][N][D] (NULL when D = 0), new_xyz float32[B][S][3],
 * group_idx int64[B][S][nsample] (sv_ball_query's output), out float32[B][S][widths[L]].
 * params: one device buffer, per layer l in order W_l float32[widths[l]][widths[l + 1]], scale_l [widths[l + 1]],
 * shift_l [widths[l + 1]]; widths: HOST int[L + 1], widths[0] = 3 + D.
 * Every output element is one fma chain over the input channels ascending from 0 (as sv_conv_fwd's dense rows): the
 * unfused path's bits.  A group index outside [0, N) (sv_ball_query's N for an empty ball) reads nothing: its row is NaN
 * in every column, so that centroid's pooled output is NaN (as sv_group_rows + sv_group_max on the training path); the
 * other centroids are unaffected.  Returns SV_ERR_UNSUPPORTED (nothing launched) when nsample is not 16 / 32 / 64, L is
 * outside 1..SV_PN_MAX_LAYERS, a layer width is not a multiple of 16 in 16..1024, or the 64-row tile's two LDS buffers
 * exceed 160 KiB. */
#define SV_PN_MAX_LAYERS 4
int sv_pointnet_sa(const float* xyz, const float* points, const float* new_xyz, const int64_t* group_idx, int B, int N,
                   int D, int S, int nsample, const float* params, const int* widths, int L, float* out,
                   sv_stream_t stream);
/* PointNetSetAbstractionMsg.forward in eval mode after sampling and ball query (model/pointnet2_utils.py:207-264) as one
 * launch over R scales that share the centroids new_xyz.  Scale r groups the rows [points[b][i], xyz[b][i] - new_xyz[b][s]]
 * with i = group_idx[r][b][s][j] (features FIRST, :247-250), runs its nlayers[r] shared-MLP layers as sv_pointnet_sa does
 * and writes the max over its nsamples[r] rows into columns col_r .. col_r + C_r of out float32[B][S][sum C_r]
 * (col_r = C_0 + .. + C_{r-1}, C_r its last width: the reference's torch.cat, :262).
 * nsamples, group_idx (device pointers), params (device pointers, sv_pointnet_sa's packing per scale), nlayers: HOST
 * arrays of R entries; widths: HOST, the R scales' width lists concatenated (nlayers[r] + 1 entries each, first 3 + D).
 * Same arithmetic as sv_pointnet_sa: every scale's columns are bit-identical to the unfused eval path on its groups, and
 * a group index outside [0, N) gives a NaN row (that scale's columns of the centroid are NaN).
 * Returns SV_ERR_UNSUPPORTED (nothing launched) when R is outside 1..SV_PN_MAX_SCALES, a scale's nsample is not
 * 16 / 32 / 64 / 128, its layer count or widths are outside sv_pointnet_sa's limits, or its LDS (two 64-row buffers, plus
 * C_r floats of running maxima when nsample = 128) exceeds 160 KiB. */
#define SV_PN_MAX_SCALES 4
int sv_pointnet_sa_msg(const float* xyz, const float* points, const float* new_xyz, int B, int N, int D, int S, int R,
                       const int* nsamples, const int64_t* const* group_idx, const float* const* params,
                       const int* widths, const int* nlayers, float* out, sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * A9  PointNet++ training (set_training_path "hip"): the gather, pooling and interpolation around the shared-MLP GEMMs
 *     and their backward.  No float atomics: every result is bit-reproducible.
 * ------------------------------------------------------------------------------------------- */
/* The grouped rows of a set abstraction, row (b, s, k) = (b * S + s) * nsample + k of out float32[B*S*nsample][ld], with
 * i = idx[b][s][k]: order SV_GROUP_SSG [xyz[b][i] - new_xyz[b][s], points[b][i]] (model/pointnet2_utils.py:131-137),
 * SV_GROUP_MSG [points[b][i], xyz[b][i] - new_xyz[b][s]] (:245-250).  Columns 3 + D .. ld - 1 are written 0.  idx NULL is
 * sample_and_group_all (:143-160): S = 1, nsample = N, row k = [xyz[b][k], points[b][k]], no subtraction, SSG order,
 * new_xyz unused.  points NULL when D = 0.  The bits of torch's index_points and subtraction.  An index outside [0, N)
 * (sv_ball_query's N for an empty ball) reads nothing: columns 0 .. 3 + D - 1 of its row are NaN. */
#define SV_GROUP_SSG 0
#define SV_GROUP_MSG 1
int sv_group_rows(const float* xyz, const float* points, const float* new_xyz, const int64_t* idx, int B, int N, int D,
                  int S, int nsample, int order, int ld, float* out, sv_stream_t stream);
/* Inverse of an index table idx[B][M] (int32 or int64 by idx_bytes) with values in [0, N): target t = b * N + idx[b][m]
 * is referenced by the positions pos[offsets[t] .. offsets[t + 1]) (position p = b * M + m), ascending per target.
 * offsets int32[B*N + 1], pos int32[B*M]; entries outside [0, N) are dropped (they sort behind every target).  The
 * stable radix sort of sv_sort.hip on key = target, value = position.  workspace: sv_index_transpose_workspace_bytes. */
size_t sv_index_transpose_workspace_bytes(int B, int64_t M, int N);
int sv_index_transpose(const void* idx, int idx_bytes, int B, int64_t M, int N, void* workspace, size_t workspace_bytes,
                       int32_t* offsets, int32_t* pos, sv_stream_t stream);
/* out[t][c] = sum over p in pos[offsets[t] .. offsets[t + 1]) ascending of w[p] * rows[p / per_row][col0 + c] (w NULL:
 * 1), for t < T and c < C; every target is written (0 where nothing references it).  rows row stride ld_rows, out
 * [T][ld_out].  The backward of sv_group_rows over the point-feature columns (per_row 1) and of sv_three_nn_gather with
 * the 3-NN weights (per_row 3); it replaces the atomic scatter of index_points' backward. */
int sv_gather_transpose(const int32_t* offsets, const int32_t* pos, const float* w, const float* rows, int64_t ld_rows,
                        int col0, int C, int per_row, int64_t T, float* out, int64_t ld_out, sv_stream_t stream);
/* Max over every group of nsample consecutive rows (torch.max(t, 2) of the set abstraction, :203 / :258):
 * out[g][c] = max over k of rows[g * nsample + k][c], arg[g][c] = its k; torch's max(dim) rule: the first NaN wins, a tie
 * goes to the lowest k.  rows row stride ld; out float32[G][C], arg int32[G][C].  group_all is G = B, nsample = N. */
int sv_group_max(const float* rows, int64_t ld, int64_t G, int nsample, int C, float* out, int32_t* arg,
                 sv_stream_t stream);
/* drows float32[G*nsample][C] = dpooled[g][c] at k = arg[g][c], 0 elsewhere: every element written in one pass. */
int sv_group_max_backward(const float* dpooled, const int32_t* arg, int64_t G, int nsample, int C, float* drows,
                          sv_stream_t stream);
/* The search and weights of sv_three_nn_interpolate written out (:298-305): idx int32[B][N][3] nearest first, w float32
 * [B][N][3] normalised 1 / (d + 1e-8); same float32 distance, tie rule and weight arithmetic, S >= 3. */
int sv_three_nn(const float* xyz1, const float* xyz2, int B, int N, int S, int32_t* idx, float* w, sv_stream_t stream);
/* out[b][n][c] = (points2[b][i0][c] * w0 + points2[b][i1][c] * w1) + points2[b][i2][c] * w2 with sv_three_nn's idx / w:
 * the bits of sv_three_nn_interpolate.  points2 [B][S][C], out [B][N][C]. */
int sv_three_nn_gather(const float* points2, const int32_t* idx, const float* w, int B, int N, int S, int C, float* out,
                       sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N4  largest single-linkage cluster of the end-effector points
 *   (replaces utils/output.py:13-28 ClusterUtil.get_largest_cluster = sklearn AgglomerativeClustering(
 *    linkage="single", distance_threshold=0.06) + most frequent label; call site app/inference_engine.py:422-433)
 *
 * Single linkage cut at `dist` = connected components of the graph "distance < dist" (strict, as sklearn merges while
 * the linkage distance is below the threshold).  Points: rows idx[i] (idx NULL = row i) of xyz, float32 or float64
 * (elem_bytes 4 / 8), row stride ld elements; distance in float64: sqrt((dx*dx + dy*dy) + dz*dz), no fma.
 *   root[i]  = the smallest i' in i's component (i, i' positions 0..n-1): a deterministic labelling
 *   best[0]  = root of the largest component (ties: the smallest root), best[1] = its size   (best may be NULL)
 * Lock-free union-find over all n(n-1)/2 pairs, tiled through LDS.  workspace: sv_cluster_workspace_bytes(n).
 * ------------------------------------------------------------------------------------------- */
size_t sv_cluster_workspace_bytes(int64_t n);
int sv_single_linkage_roots(const void* xyz, int elem_bytes, int64_t ld, const int32_t* idx, int64_t n, double dist,
                            void* workspace, size_t workspace_bytes, int32_t* root, int32_t* best, sv_stream_t stream);
/* out = the ascending positions i with v[i] == value (v int32 / int64 by elem_bytes; value_dev non-NULL: compare with
 * the int32 it points to on the device instead of `value`), count[0] = how many.  The np.where(...)[0] of
 * utils/output.py:24 and app/inference_engine.py:420 without a host round trip. */
int sv_select_equal(const void* v, int elem_bytes, int64_t n, int64_t value, const int32_t* value_dev, int64_t* out,
                    int64_t* count, sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N8  strided kernel maps, local pooling, instance normalisation: what the classification ResNets need beyond the
 *      U-Nets (ME.MinkowskiConvolution(kernel_size=3 / 1, stride=2 / 3), ME.MinkowskiMaxPooling(kernel_size=2, stride=2),
 *      ME.MinkowskiInstanceNorm; model/backbone/resnet.py:48-84,95-127).  Additions of ABI 4.
 *
 * Semantics (MinkowskiEngine 0.5.4, restated from memory - ME is not installed; tests/test_gpu_resnet_dense.py pins the
 * definition itself against dense conv3d / max_pool3d): a convolution of stride st on a tensor of tensor stride ts writes
 * the map at tensor stride ts * st, whose voxels are floor(c / (ts st)) * ts st of the input voxels c; an ODD kernel is
 * centred on the output coordinate (inputs at o + d * ts * dilation, d in {-1,0,1}^3), an EVEN kernel starts at it.
 *
 * sv_stride_map_general: the map at tensor stride s_out of a map at s_in, s_out a positive multiple of s_in (any multiple;
 *   powers of two stay on sv_stride_map, which only clears key bits).  Output coordinate = floor(c / s_out) * s_out per axis
 *   on the SIGNED coordinate (negative coordinates floor towards minus infinity).  The interleaved key does not keep its order
 *   under that, so the voxels are re-keyed, sorted (stable radix sort) and uniqued.  keys_out / vcoords_out: canonical sorted
 *   unique keys and (batch,x,y,z) rows, first V_out entries (arrays of V_in); parent int32[V_in]: row of every input voxel in
 *   the output map; counters int32[4]: [0] = V_out, [1] = input voxels whose output coordinate leaves the key range (a
 *   coordinate below -2^17 after flooring; must be 0 - as sv_voxelize's counters[1]: such a voxel is keyed as (batch 0, 0,0,0)
 *   and gets parent -1, the map is then not the input's).
 * sv_kernel_map_probe: kernel map between TWO maps - sv_kernel_map_k3 with the query rows (vcoords_q, V_q) taken from one
 *   map and the hash table (and vcoords_t / V_t, its canonical rows: the SV_EMPTY_KEY voxel is found as their last row) from
 *   another.  kernel_size 1 (K = 1, offset 0) or 3 (K = 27, x fastest as everywhere).  step: SIGNED, input tensor stride *
 *   dilation.  nbr[k*ld + o] = row in the table's map of coords_q[o] + d_k * step, or -1 (also when that coordinate leaves
 *   the key range); mask[o] bit k = present.  Forward map of a strided conv: queries = output map, table = input map, +step;
 *   map of its input gradient (and of pooling's backward): queries = input map, table = output map, -step - the transpose:
 *   nbr[k][o] = i exactly when nbr_t[k][i] = o.  sv_kernel_map_k3(vcoords, V, tensor_stride, dilation, ...) is its
 *   same-map case - (vcoords_q, V_q) = (vcoords_t, V_t) = (vcoords, V), kernel_size 3, step = tensor_stride * dilation - on
 *   the same kernel, which then writes the centre offset's nbr[13][o] = o without a lookup; the tables are equal.
 * ------------------------------------------------------------------------------------------- */
size_t sv_stride_map_general_workspace_bytes(int64_t V_in);
int sv_stride_map_general(const uint64_t* keys_in, int64_t V_in, int s_in, int s_out, void* workspace, size_t workspace_bytes,
                          uint64_t* keys_out, int32_t* vcoords_out, int32_t* parent, int32_t* counters, sv_stream_t stream);
int sv_kernel_map_probe(const int32_t* vcoords_q, int64_t V_q, int kernel_size, int step, const int32_t* vcoords_t, int64_t V_t,
                        const uint64_t* table_keys, const int32_t* table_vals, int64_t capacity, int32_t* nbr, int64_t ld,
                        uint32_t* mask, sv_stream_t stream);

/* Local pooling over any kernel-map neighbour table nbr int32[K][ld] (the raw map, not a conv plan):
 *   SV_POOL_SUM: out[o][c] = sum over k ascending of in[nbr[k][o]][c], fp32, starting from 0;
 *   SV_POOL_AVG: that sum / number of present neighbours of o;
 *   SV_POOL_MAX: the maximum, arg[o][c] (int32[V_out][C], dense) = the input row that won; torch's max(dim) rule as
 *     sv_group_max: the first NaN (lowest k) wins and stays, a tie goes to the lowest k.
 *   A row without neighbours (no kernel map produces one) gives 0, and arg = -1.
 * One wavefront per output row, lanes along C (float4 when C % 4 == 0 and rows are 16-byte aligned).  arg may be NULL unless
 * mode is SV_POOL_MAX.
 * Backward: one thread per (input row, channel) over the TRANSPOSED table nbr_t int32[K][ld_t] (kernel_size 2 stride 2: the
 * up map; else sv_kernel_map_probe with -step):
 *   dx[i][c] = sum over k ascending with o = nbr_t[k][i] >= 0 of  dy[o][c]                       (sum)
 *                                                                 dy[o][c] / popcount(mask_fwd[o]) (avg; the forward map's mask)
 *                                                                 dy[o][c] if arg[o][c] == i       (max)
 * no float atomics: the same bits on every run.  Every dx element is written. */
#define SV_POOL_SUM 2
int sv_pool_local(const float* in, int64_t V_in, int64_t in_ld, int C, const int32_t* nbr, int64_t ld, int K, int64_t V_out,
                  int mode, float* out, int64_t out_ld, int32_t* arg, sv_stream_t stream);
int sv_pool_local_backward(const float* dy, int64_t V_out, int64_t dy_ld, int C, const int32_t* nbr_t, int64_t ld_t, int K,
                           int64_t V_in, int mode, const int32_t* arg, const uint32_t* mask_fwd, float* dx, int64_t dx_ld,
                           sv_stream_t stream);

/* Instance normalisation over the frames of a batched tensor (rows batch_start[b] .. batch_start[b+1], sv_batch_offsets;
 * V = rows of x, batch_start[B] <= V), per (frame b, channel c) over the frame's n rows, all in float64:
 *   mean = sum x / n;  var = sum (x - mean)^2 / n  (second pass, biased);  inv_std = 1 / sqrt(var + eps)
 *   y = (float) act((x - mean) * inv_std * weight[c] + bias[c])      act: SV_ACT_NONE, SV_ACT_RELU or SV_ACT_GELU
 *       (GELU in the exact erf form, evaluated in float64 before the one rounding to float32)
 * eps = 1e-8 and weight / bias of shape [1, C] are ME 0.5.4's MinkowskiInstanceNorm from memory (unverified).
 * Summation tree: chunks of SV_NORM_CHUNK_ROWS rows; a chunk's four quarters are each summed sequentially in ascending row
 * order and added in ascending order; a frame's chunks are added in ascending order.  No atomics.
 * A frame with n = 0 writes no row (its mean / inv_std entries are 0); n = 1 gives act(bias).  mean / inv_std: double[B][C],
 * written for the backward.
 * Backward (dy' = dy * act'(pre-activation), the pre-activation recomputed; g = dy' * weight):
 *   dx = inv_std * (g - mean_b(g) - xhat * mean_b(g * xhat)),  xhat = (x - mean) * inv_std
 *   dweight[c] = sum over frames ascending of sum_rows dy' * xhat;  dbias[c] = ... of sum_rows dy'   (float32[C], may be NULL)
 * the frame sums through the same tree.  One workspace size serves both calls. */
#define SV_ACT_GELU 3
#define SV_NORM_CHUNK_ROWS 256
size_t sv_instance_norm_workspace_bytes(int64_t V, int B, int C);
int sv_instance_norm(const float* x, int64_t V, int64_t ld, int C, const int32_t* batch_start, int B, const float* weight,
                     const float* bias, double eps, int act, void* workspace, size_t workspace_bytes, float* y, int64_t y_ld,
                     double* mean, double* inv_std, sv_stream_t stream);
int sv_instance_norm_backward(const float* x, int64_t V, int64_t ld, int C, const int32_t* batch_start, int B, const float* weight,
                              const float* bias, const double* mean, const double* inv_std, int act, const float* dy,
                              int64_t dy_ld, void* workspace, size_t workspace_bytes, float* dx, int64_t dx_ld, float* dweight,
                              float* dbias, sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N9  field front end of the ResFieldNets (reference model/backbone/resnet.py:165-193): layers that run on the POINTS of a
 * TensorField before voxelisation.  Semantics of ME 0.5.4 restated from memory (unverified).
 *
 * sv_sinusoidal - ME.MinkowskiSinusoidal:  out[p][n] = coef[n] * sin(sum_k x[p][k] kernel[k][n] + bias[n])
 *   x: [N] rows of Cin floats, row stride ld >= Cin; kernel [Cin][Cout]; bias, coef [Cout]; out row stride out_ld >= Cout
 *   (column views are fine on both sides).  Any Cin, Cout >= 1; N = 0 is valid.
 *   Order: a = 0; a = fmaf(x[p][k], kernel[k][n], a) for k ascending; a = a + bias[n]  (all fp32).  The sine is evaluated in
 *   float64 on that fp32 argument (full-range argument reduction) and rounded once to fp32; one more rounding for the
 *   product with coef.  NaN or +-inf in a row give NaN in that row only.  Same bits on every call.
 *
 * sv_field_stage - the eval() form of one field network in one launch:
 *     Sinusoidal -> BN -> ReLU -> Linear -> BN -> ReLU -> per-voxel mean            (the [N, C] intermediates stay on chip)
 *   input row of point p: [G[inverse[p]][0..Cg), F[p][0..Cf)]  (SparseTensor.cat_slice's order); Cg = 0 with G = inverse =
 *   NULL is a network on the field alone.  F row stride f_ld >= Cf, G row stride g_ld >= Cg, out [V] rows of C, out_ld >= C.
 *   kernel [Cg + Cf][C], bias / coef [C]: the sinusoidal layer, computed exactly as sv_sinusoidal does.
 *   scale1 / shift1, scale2 / shift2 [C]: the folded batch norms, y = fmaf(x, scale, shift).  relu(v) = v < 0 ? 0 : v.
 *   W [C][C] (W[c][n], input channel first: MinkowskiLinear.weight3()), lin_bias [C] or NULL:
 *     b = 0; b = fmaf(h[c], W[c][n], b) for c ascending; b = b + lin_bias[n].
 *   order / seg_start / V: sv_voxelize's.  out[v][n] = the sequential fp32 sum over the voxel's points in ascending
 *   original index, then ONE division by the voxel's count (sv_voxel_reduce's rule): a voxel's row does not depend on
 *   the other voxels of the call nor on the kernel's tiles (a voxel longer than a tile is carried by one workgroup, in order).
 *   A NaN point makes exactly its voxel's row NaN.  No float atomics; same bits on every call.
 *   C in {32, 64} and Cg + Cf <= 128, else SV_ERR_UNSUPPORTED before anything is launched (the caller runs the layers one by
 *   one).  N = 0 with V = 0 is valid.
 * ------------------------------------------------------------------------------------------- */
int sv_sinusoidal(const float* x, int64_t ld, int Cin, int64_t N, const float* kernel, const float* bias, const float* coef,
                  int Cout, float* out, int64_t out_ld, sv_stream_t stream);
int sv_field_stage(const float* F, int64_t f_ld, int Cf, int64_t N, const float* G, int64_t g_ld, int Cg, const int64_t* inverse,
                   const float* kernel, const float* bias, const float* coef, const float* scale1, const float* shift1,
                   const float* W, const float* lin_bias, const float* scale2, const float* shift2, int C,
                   const int32_t* order, const int32_t* seg_start, int64_t V, float* out, int64_t out_ld, sv_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N10  metric-learning criterion (replaces the criterion of train_feature-extractor.py:65-81 and
 *      train_feature-extractor-voxel.py, built by model/featurenet.py:30-34: miners.MultiSimilarityMiner() on
 *      out.features, truncation of the mined pairs to batch_size * max_pair, losses.TripletMarginLoss() on what is left;
 *      both classes are pytorch_metric_learning's, with their defaults).  Additions of ABI 4.
 *      The semantics below are that library's published algorithm restated from memory; the library is not available to
 *      this project, so parity with it is by construction and unverified.
 *
 * Common arguments: x float32[B][ld], columns 0 .. E-1 are the embedding (ld >= E >= 1; the padding is never read),
 *   B in [1, SV_MAX_BATCH].  All arithmetic is float64 on the float32 inputs:
 *     u_i = x_i / max(||x_i||_2, 1e-12)         (F.normalize)
 *     S[i][j] = u_i . u_j                        (CosineSimilarity)
 *     D[i][j] = ||u_i - u_j||_2                  (LpDistance(normalize_embeddings=True, p=2, power=1)), from the differences
 *   Every entry validates on the host before any HIP call (null pointer, B outside [1, SV_MAX_BATCH], E < 1, ld < E, a
 *   negative capacity, a cap below -1, a workspace below sv_metric_workspace_bytes(B, E): SV_ERR_INVALID), launches on the
 *   stream and never waits or reads back; the same arguments give the same bits; no floating-point atomics (integer
 *   atomics count the pairs of a given tuple).  Nothing is sized by the number of pairs or triplets: the workspace holds
 *   [B][B] matrices and two [B][E] float64 copies of the embeddings.
 *
 * sv_ms_mine - MultiSimilarityMiner(epsilon) with CosineSimilarity, labels int64[B] (any values):
 *   for anchor i the positives are j != i with labels[j] == labels[i], the negatives j with labels[j] != labels[i];
 *   maxneg_i = the largest S[i][j] over its negatives (-inf without one), minpos_i = the smallest over its positives
 *   (+inf without one).  Hard positive: S[i][j] - epsilon < maxneg_i.  Hard negative: S[i][j] + epsilon > minpos_i.
 *   A batch without any positive pair, or without any negative pair, therefore has no hard pair at all (the library's
 *   early return).
 *   Order of each list: anchor ascending; within an anchor S ascending; equal S by column ascending (the order of
 *   torch.sort followed by torch.where; the tie rule is this library's, torch leaves it open).
 *   max_pos / max_neg (-1: none): only the first max_* pairs in that order are kept - the trainer's truncation.
 *   a1, p int64[cap_pos] and a2, n int64[cap_neg]: the kept pairs; entries at and after the kept count are not written.
 *   A capacity below the kept count truncates in the same way (cap_* = 0 with NULL lists just counts).
 *   counts int64[4] = (kept positives, kept negatives, hard positives, hard negatives), on the device.
 *   A row of x with a NaN or an infinity joins no pair, as anchor or as partner, and adds one to n_nonfinite[0] (int32);
 *   the other rows mine as if it were absent.  No parity with the library is claimed there.
 *
 * sv_triplet_margin - TripletMarginLoss(margin) with the library's defaults (no swap, no smooth loss, all triplets per
 *   anchor, AvgNonZeroReducer) on a tuple of pair lists in any order:
 *   a1, p int64[cap_pos], a2, n int64[cap_neg]; the lengths are read from the device: counts[0] positives and counts[1]
 *   negatives, each clamped to [0, cap_*] (counts is int64[>= 2]: sv_ms_mine's output fits).
 *   Triplets: every (a1[s], p[s], n[t]) with a1[s] == a2[t]; a pair listed twice counts twice.
 *   Triplet loss: max(D[a][p] - D[a][n] + margin, 0).
 *   sums float64[2] = (sum over the triplets, number of triplets with loss > 0); the caller forms sums[0] / sums[1], or 0
 *   when sums[1] == 0.  The sum's order depends on (B, E) and on the multiset of pairs only, not on their order in the
 *   lists: anchors ascending, negatives by column, positives by column.
 *   grad float32[B][E] dense (may be NULL): the UNSCALED d sums[0] / d x through the distance and the normalisation, in
 *   float64 until the one rounding; the subgradient is 0 where D = 0 (torch.cdist's) and at the hinge; a row in no
 *   violating triplet is exactly 0.  The caller multiplies by 1 / sums[1] and the incoming gradient.
 *   n_triplets int64[1] = the number of triplets.  n_invalid int32[1] = pairs with an index outside [0, B): skipped.
 *   A non-finite embedding that takes part in a triplet makes sums[0] NaN.
 *
 * sv_mined_triplet_step - sv_ms_mine(max_pos, max_neg) followed by sv_triplet_margin on the kept pairs, in one entry that
 *   computes S and D together and never writes the lists: counts, n_nonfinite, sums, grad and n_triplets are bit-equal to
 *   the two calls composed (with capacities that hold the kept pairs).  The trainer's randperm after the truncation only
 *   reorders the kept pairs, which the loss does not see.
 *
 * workspace: sv_metric_workspace_bytes(B, E) for all three.
 * ------------------------------------------------------------------------------------------- */
size_t sv_metric_workspace_bytes(int B, int E);
int sv_ms_mine(const float* x, int64_t ld, int B, int E, const int64_t* labels, double epsilon, int64_t max_pos, int64_t max_neg,
               void* workspace, size_t workspace_bytes, int64_t* a1, int64_t* p, int64_t cap_pos, int64_t* a2, int64_t* n,
               int64_t cap_neg, int64_t* counts, int32_t* n_nonfinite, sv_stream_t stream);
int sv_triplet_margin(const float* x, int64_t ld, int B, int E, const int64_t* a1, const int64_t* p, int64_t cap_pos,
                      const int64_t* a2, const int64_t* n, int64_t cap_neg, const int64_t* counts, double margin,
                      void* workspace, size_t workspace_bytes, double* sums, float* grad, int64_t* n_triplets,
                      int32_t* n_invalid, sv_stream_t stream);
int sv_mined_triplet_step(const float* x, int64_t ld, int B, int E, const int64_t* labels, double epsilon, double margin,
                          int64_t max_pos, int64_t max_neg, void* workspace, size_t workspace_bytes, double* sums, float* grad,
                          int64_t* counts, int64_t* n_triplets, int32_t* n_nonfinite, sv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SV_HIP_H */
