"""ctypes binding of libsvhip.so (the C-ABI declared in include/sv_hip.h).

There is NO fallback: if the HIP library is missing or a call fails, the product path raises.  PyTorch-ROCm is used
only to own device memory and streams; every computation on the hot path is a call into the library.
"""
import ctypes
import os
import threading
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
ABI_VERSION = 4  # SV_ABI_VERSION of include/sv_hip.h
LIB_PATH = os.environ.get("SVHIP_LIB") or os.path.join(_HERE, "libsvhip.so")  # SVHIP_LIB: kernel A/B experiments

SV_ACT_NONE, SV_ACT_RELU, SV_ACT_LEAKY_RELU, SV_ACT_GELU = 0, 1, 2, 3
SV_POOL_MAX, SV_POOL_AVG, SV_POOL_SUM = 0, 1, 2
SV_NORM_CHUNK_ROWS = 256
SV_REDUCE_MEAN, SV_REDUCE_FIRST, SV_REDUCE_SUM = 0, 1, 2
SV_TILE_ROWS = 128
SV_ERR_UNSUPPORTED = -5
SV_PN_MAX_LAYERS = 4
SV_PN_MAX_SCALES = 4
SV_BQ_MAX_RADII = 4
SV_GROUP_SSG, SV_GROUP_MSG = 0, 1
SV_LOSS_POSE, SV_LOSS_SHAPE_MATCH, SV_LOSS_POSE_MATCH, SV_LOSS_KP_POSE_MATCH = 0, 1, 2, 3
SV_AUG_STRIDE, SV_AUG_ELASTIC0, SV_AUG_ELASTIC1 = 40, 0, 7
SV_AUG_E_ON, SV_AUG_E_OFFSET, SV_AUG_E_BX, SV_AUG_E_BY, SV_AUG_E_BZ, SV_AUG_E_GRAN, SV_AUG_E_MAG = range(7)
SV_AUG_NOISE_ON, SV_AUG_NOISE_SIGMA, SV_AUG_NOISE_CLIP, SV_AUG_TRANSFORM_ON, SV_AUG_ROT, SV_AUG_TRANSLATION = 14, 15, 16, 17, 18, 27
SV_AUG_FLIP_SIGN, SV_AUG_GRAVITY_ON, SV_AUG_GRAVITY_ANGLE, SV_AUG_GRAVITY_COS, SV_AUG_GRAVITY_SIN = 30, 31, 32, 33, 34
SV_ORIGIN_NONE, SV_ORIGIN_CENTER, SV_ORIGIN_BASE = 0, 1, 2
SV_COORD_BIAS = 1 << 17
SV_COORD_BITS = 18
SV_MAX_BATCH = 1024
SV_FRAME_MAX_LEVELS, SV_FRAME_MAX_CUTS, SV_FRAME_RECORD = 8, 4, 16
SV_FRAME_K3, SV_FRAME_DOWN, SV_FRAME_UP, SV_FRAME_SPLIT = 1, 2, 4, 8
SV_FIELD_F32, SV_FIELD_F64 = 7, 8
SV_UNPACK_BIGENDIAN, SV_UNPACK_KEEP_NONFINITE = 1, 2
SV_DEPTH_U16, SV_DEPTH_F32 = 4, 7
SV_RGBD_ALIGNED, SV_RGBD_NEAREST, SV_RGBD_BGR = 1, 2, 4
SV_CONV_SEL_PLAN, SV_CONV_SEL_TILE_ORDER, SV_CONV_SEL_VEC_A, SV_CONV_SEL_BUF_OK, SV_CONV_SEL_ACC_INIT, SV_CONV_SEL_W_ALIGNED = (
    1, 2, 4, 8, 16, 32)
SV_FRAME_REC_HASH, SV_FRAME_REC_K3, SV_FRAME_REC_DOWN, SV_FRAME_REC_UP, SV_FRAME_REC_SPLIT = 1, 2, 3, 4, 5


class SvHipError(RuntimeError):
    pass


# name -> (restype, argtypes); kept in one table so tests can check that every symbol of include/sv_hip.h is exported
_P = c_void_p
SIGNATURES = {
    "sv_last_error": (c_char_p, []),
    "sv_abi_version": (c_int, []),
    "sv_voxelize_workspace_bytes": (c_size_t, [c_int64]),
    "sv_voxelize": (c_int, [_P, c_int, c_int64, _P, c_size_t, _P, _P, _P, _P, _P, _P, _P]),
    "sv_voxel_reduce": (c_int, [_P, c_int, _P, _P, c_int64, c_int, _P, _P]),
    "sv_hash_build": (c_int, [_P, c_int64, _P, _P, c_int64, _P]),
    "sv_stride_map_workspace_bytes": (c_size_t, [c_int64]),
    "sv_stride_map": (c_int, [_P, c_int64, c_int, _P, c_size_t, _P, _P, _P, _P, _P, _P]),
    "sv_kernel_map_k3": (c_int, [_P, c_int64, c_int, c_int, _P, _P, c_int64, _P, c_int64, _P, _P]),
    "sv_kernel_map_down": (c_int, [_P, _P, c_int64, c_int, c_int64, _P, c_int64, _P, _P]),
    "sv_kernel_map_up": (c_int, [_P, _P, c_int64, c_int, _P, c_int64, _P, _P]),
    "sv_plan_workspace_bytes": (c_size_t, [c_int64]),
    "sv_plan_build": (c_int, [_P, c_int64, _P, c_int, c_int64, c_int64, _P, c_size_t, _P, _P, _P, _P, c_int64, _P]),
    "sv_conv_fwd": (
        c_int,
        [_P, c_int64, c_int64, c_int, _P, c_int, c_int, _P, _P, _P, _P, c_int64, c_int64, _P, _P, _P, c_int64, c_int,
         c_float, _P, c_int64, _P],
    ),
    "sv_conv_fwd_acc": (
        c_int,
        [_P, c_int64, c_int64, c_int, _P, c_int, c_int, _P, _P, _P, _P, c_int64, c_int64, _P, c_int64, _P, _P, _P, c_int64, c_int,
         c_float, _P, c_int64, _P],
    ),
    "sv_pack_weights_bf16": (c_int, [_P, c_int, c_int, c_int, _P, _P]),
    "sv_conv_fwd_bf16": (
        c_int,
        [_P, c_int64, c_int64, c_int, _P, c_int, c_int, _P, _P, _P, _P, c_int64, c_int64, _P, c_int64, _P, _P, _P, c_int64, c_int,
         c_float, _P, c_int64, _P],
    ),
    "sv_conv_wgrad_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int]),
    "sv_conv_wgrad": (
        c_int,
        [_P, c_int64, c_int64, c_int, _P, c_int64, c_int64, c_int, c_int, _P, _P, _P, c_int64, c_int, _P, c_size_t, _P, _P],
    ),
    "sv_conv_wgrad_bf16_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int]),
    "sv_conv_wgrad_bf16": (
        c_int,
        [_P, c_int64, c_int64, c_int, _P, c_int64, c_int64, c_int, c_int, _P, _P, _P, c_int64, c_int, _P, c_size_t, _P, _P],
    ),
    "sv_conv_last_instance": (c_char_p, []),
    "sv_conv_set_dispatch": (c_int, [c_double, c_double]),
    "sv_conv_select": (c_int, [c_int64, _P, c_double, c_double, _P, c_size_t]),
    "sv_conv_tile_info": (c_int, [c_int, _P]),
    "sv_frame_maps_arena_bytes": (c_size_t, [c_int64, c_int]),
    "sv_frame_maps_scratch_bytes": (c_size_t, [c_int64]),
    "sv_frame_maps": (c_int, [_P, c_int, c_int64, c_int, _P, c_size_t, _P, c_size_t, _P, _P, _P]),
    "sv_frame_plans_arena_bytes": (c_size_t, [_P, c_int, c_int, _P]),
    "sv_frame_plans_scratch_bytes": (c_size_t, [_P, c_int]),
    "sv_frame_plans": (c_int, [_P, _P, _P, _P, c_int, c_int, _P, _P, _P, _P, c_size_t, _P, c_size_t, _P, c_int, _P]),
    "sv_affine_act": (c_int, [_P, c_int64, c_int, c_int64, _P, _P, _P, c_int64, c_int, c_float, _P, c_int64, _P]),
    "sv_col_stats_workspace_bytes": (c_size_t, [c_int64]),
    "sv_col_stats": (c_int, [_P, c_int64, c_int64, c_int, _P, _P, c_size_t, _P, _P, _P, _P, _P]),
    "sv_center_scale": (c_int, [_P, c_int64, c_int64, c_int, _P, _P, _P, _P, c_int64, _P]),
    "sv_batch_offsets": (c_int, [_P, c_int64, c_int, _P, _P]),
    "sv_global_pool": (c_int, [_P, c_int64, c_int, _P, c_int, c_int, _P, _P]),
    "sv_slice_rows": (c_int, [_P, c_int64, c_int, _P, c_int64, _P, _P]),
    "sv_slice_argmax": (c_int, [_P, c_int64, c_int, _P, c_int64, _P, _P, _P]),
    "sv_key_point_predictions": (c_int, [_P, c_int64, c_int, c_int64, c_float, _P, c_size_t, _P, _P, _P, _P]),
    "sv_key_point_predictions_batched": (c_int, [_P, c_int64, c_int, _P, c_int, c_float, _P, c_size_t, _P, _P, _P, _P]),
    "sv_topk_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "sv_topk_indices": (c_int, [_P, c_int64, c_int64, c_int, _P, c_size_t, _P, _P]),
    "sv_kabsch_batched": (c_int, [_P, _P, _P, c_int, c_int, _P, _P, _P, _P]),
    "sv_quat_avg_batched": (c_int, [_P, _P, _P, c_int, c_int, _P, _P]),
    "sv_add_metric_batched": (c_int, [_P, _P, c_int, _P, _P, c_int, _P, _P]),
    "sv_icp_workspace_bytes": (c_size_t, [c_int64]),
    "sv_icp_point2point": (c_int, [_P, c_int64, _P, c_int64, _P, c_double, c_int, c_double, c_double, _P, c_size_t, _P, _P,
                                   _P]),
    "sv_normals_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "sv_estimate_normals": (c_int, [_P, c_int64, c_double, c_int, _P, c_size_t, _P, _P, _P]),
    "sv_icp_point2plane_workspace_bytes": (c_size_t, [c_int64]),
    "sv_icp_point2plane": (c_int, [_P, c_int64, _P, _P, c_int64, _P, c_double, c_int, c_double, c_double, _P, c_size_t, _P,
                                   _P, _P]),
    "sv_icp_batched_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "sv_icp_batched": (c_int, [_P, c_int64, _P, _P, _P, _P, c_int, _P, c_int, c_double, c_int, c_double, c_double, _P,
                               c_size_t, _P, _P, _P]),
    "sv_mesh_sample_workspace_bytes": (c_size_t, [c_int64]),
    "sv_mesh_sample": (c_int, [_P, c_int64, _P, c_int64, _P, c_int64, _P, c_size_t, _P, _P, _P, _P, _P, _P]),
    "sv_sample_eliminate_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "sv_sample_eliminate": (c_int, [_P, c_int64, c_int64, c_double, c_double, c_int, _P, c_size_t, _P, _P, _P, _P]),
    "sv_unpack_points_workspace_bytes": (c_size_t, [c_int64]),
    "sv_unpack_points": (c_int, [_P, c_int64, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, _P,
                                 _P, _P, c_size_t, _P, _P, _P, _P, _P]),
    "sv_rgbd_cloud_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64, c_int64]),
    "sv_rgbd_cloud": (c_int, [_P, c_int, c_int64, c_int64, c_int64, _P, c_int64, c_int64, c_int64, _P, _P, c_int, c_int, c_int,
                              _P, _P, _P, c_size_t, _P, _P, _P, _P, _P, _P, _P]),
    "sv_lens_rays": (c_int, [_P, _P, c_int64, c_int64, _P, _P]),
    "sv_rgbd_cloud_lens": (c_int, [_P, c_int, c_int64, c_int64, c_int64, _P, c_int64, c_int64, c_int64, _P, _P, c_int, c_int,
                                   c_int, _P, _P, _P, c_size_t, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "sv_pose_loss_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "sv_pose_match_loss": (c_int, [_P, _P, c_int64, c_int, _P, _P, _P, _P, _P, _P, c_int, _P, c_size_t, _P, _P, _P, _P, _P]),
    "sv_elastic_field_workspace_bytes": (c_size_t, [_P, c_int]),
    "sv_elastic_field": (c_int, [_P, _P, c_int, _P, c_size_t, _P, _P]),
    "sv_augment_points_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "sv_augment_points": (c_int, [_P, c_int, _P, c_int64, c_int, _P, _P, c_int64, _P, _P, c_size_t, _P, _P, _P]),
    "sv_quantise_points": (c_int, [_P, _P, c_int64, c_int, _P, c_int, c_double, _P, _P, _P, _P]),
    "sv_ee_mask": (c_int, [_P, c_int, _P, c_int64, c_int, _P, _P, _P, _P, _P]),
    "sv_key_points": (c_int, [_P, c_int, _P, c_int64, c_int, _P, _P, c_int, c_double, c_int64, _P, _P, _P, _P]),
    "sv_line_topk_workspace_bytes": (c_size_t, [c_int64]),
    "sv_line_topk": (c_int, [_P, c_int, _P, c_int64, c_int, _P, _P, _P, _P, c_int, c_double, _P, c_size_t, _P, _P, _P, _P]),
    "sv_radius_labels": (c_int, [_P, c_int, _P, c_int64, c_int, _P, c_int, c_double, c_int64, _P, _P]),
    "sv_seg_criterion_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "sv_seg_criterion": (c_int, [_P, c_int64, c_int, c_int64, _P, c_int64, _P, c_int, _P, c_size_t, _P, _P, _P, _P, _P, _P]),
    "sv_segment_topk_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "sv_segment_topk": (c_int, [_P, c_int64, c_int64, _P, c_int, c_int, _P, c_size_t, _P, _P]),
    "sv_fps": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P]),
    "sv_three_nn_interpolate": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P, _P]),
    "sv_cluster_workspace_bytes": (c_size_t, [c_int64]),
    "sv_single_linkage_roots": (c_int, [_P, c_int, c_int64, _P, c_int64, c_double, _P, c_size_t, _P, _P, _P]),
    "sv_select_equal": (c_int, [_P, c_int, c_int64, c_int64, _P, _P, _P, _P]),
    "sv_ball_query": (c_int, [_P, _P, c_int, c_int, c_int, c_double, c_int, _P, _P]),
    "sv_fps_segmented": (c_int, [_P, _P, _P, _P, c_int, c_int, _P, _P]),
    "sv_pointnet_sa": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P, c_int, _P, _P]),
    "sv_ball_query_multi": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P]),
    "sv_pointnet_sa_msg": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P]),
    "sv_group_rows": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "sv_index_transpose_workspace_bytes": (c_size_t, [c_int, c_int64, c_int]),
    "sv_index_transpose": (c_int, [_P, c_int, c_int, c_int64, c_int, _P, c_size_t, _P, _P, _P]),
    "sv_gather_transpose": (c_int, [_P, _P, _P, _P, c_int64, c_int, c_int, c_int, c_int64, _P, c_int64, _P]),
    "sv_group_max": (c_int, [_P, c_int64, c_int64, c_int, c_int, _P, _P, _P]),
    "sv_group_max_backward": (c_int, [_P, _P, c_int64, c_int, c_int, _P, _P]),
    "sv_three_nn": (c_int, [_P, _P, c_int, c_int, c_int, _P, _P, _P]),
    "sv_three_nn_gather": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P, _P]),
    "sv_stride_map_general_workspace_bytes": (c_size_t, [c_int64]),
    "sv_stride_map_general": (c_int, [_P, c_int64, c_int, c_int, _P, c_size_t, _P, _P, _P, _P, _P]),
    "sv_kernel_map_probe": (c_int, [_P, c_int64, c_int, c_int, _P, c_int64, _P, _P, c_int64, _P, c_int64, _P, _P]),
    "sv_pool_local": (c_int, [_P, c_int64, c_int64, c_int, _P, c_int64, c_int, c_int64, c_int, _P, c_int64, _P, _P]),
    "sv_pool_local_backward": (c_int, [_P, c_int64, c_int64, c_int, _P, c_int64, c_int, c_int64, c_int, _P, _P, _P, c_int64, _P]),
    "sv_instance_norm_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "sv_instance_norm": (c_int, [_P, c_int64, c_int64, c_int, _P, c_int, _P, _P, c_double, c_int, _P, c_size_t, _P, c_int64, _P,
                                 _P, _P]),
    "sv_instance_norm_backward": (c_int, [_P, c_int64, c_int64, c_int, _P, c_int, _P, _P, _P, _P, c_int, _P, c_int64, _P,
                                          c_size_t, _P, c_int64, _P, _P, _P]),
    "sv_sinusoidal": (c_int, [_P, c_int64, c_int, c_int64, _P, _P, _P, c_int, _P, c_int64, _P]),
    "sv_field_stage": (c_int, [_P, c_int64, c_int, c_int64, _P, c_int64, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, _P,
                               _P, c_int64, _P, c_int64, _P]),
    "sv_metric_workspace_bytes": (c_size_t, [c_int, c_int]),
    "sv_ms_mine": (c_int, [_P, c_int64, c_int, c_int, _P, c_double, c_int64, c_int64, _P, c_size_t, _P, _P, c_int64, _P, _P,
                           c_int64, _P, _P, _P]),
    "sv_triplet_margin": (c_int, [_P, c_int64, c_int, c_int, _P, _P, c_int64, _P, _P, c_int64, _P, c_double, _P, c_size_t, _P, _P,
                                  _P, _P, _P]),
    "sv_mined_triplet_step": (c_int, [_P, c_int64, c_int, c_int, _P, c_double, c_double, c_int64, c_int64, _P, c_size_t, _P, _P,
                                      _P, _P, _P, _P]),
}

_lib = None


def load():
    """Load libsvhip.so (once).  Raises SvHipError when it has not been built: there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SvHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C markerless-robot-camera-calibration_amd/csrc`). There is no CPU fallback."
        )
    lib = ctypes.CDLL(LIB_PATH)
    lib.sv_abi_version.restype = c_int
    if lib.sv_abi_version() != ABI_VERSION:  # a stale build would misread the arguments of a call whose signature moved
        raise SvHipError(f"{LIB_PATH} has C-ABI version {lib.sv_abi_version()}, this package binds version {ABI_VERSION}: "
                         "rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`)")
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _check(rc, name):
    if rc != 0:
        msg = _lib.sv_last_error().decode("utf-8", "replace")
        raise SvHipError(f"{name} failed with status {rc}: {msg}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return c_void_p(t.data_ptr())


def stream_ptr():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def call(name, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    _check(rc, name)


def _parse_instance(raw):
    name, _, flags = raw.partition("|")
    return name, {k: int(v) for k, v in (kv.split("=") for kv in flags.split(",") if kv)}


def conv_last_instance():
    """(kernel instance name, {"fast": 0/1, "ring": 0/1, "full": 0/1}) of this thread's last sv_conv_fwd launch."""
    return _parse_instance(load().sv_conv_last_instance().decode())


def conv_instance(K, Cin, Cout, Vpad, flags, want_scale=-1.0, tail_fraction=-1.0):
    """What sv_conv_last_instance would report after an sv_conv_fwd_acc call of this shape, as the raw string
    "name|fast=F,ring=R,full=U" (sv_conv_select: the library's own dispatch rules, asked on the host; flags = SV_CONV_SEL_*;
    negative scale / tail = this thread's current dispatch)"""
    name = ctypes.create_string_buffer(128)
    call("sv_conv_select", 1, (c_int64 * 5)(K, Cin, Cout, Vpad, flags), want_scale, tail_fraction, name, 128)
    return name.value.decode()


def conv_tiles():
    """The library's table of tile instances (sv_conv_tile_info): [(TM, WAVES_N, NT, CPO, MR, TN, GK, KC, PFD, USE_FULL)]"""
    rows, out = [], (c_int * 10)()
    while load().sv_conv_tile_info(len(rows), out) == 0:
        rows.append(tuple(out))
    return rows


class conv_dispatch:
    """`with conv_dispatch(want_scale):` - dispatch thresholds of this thread's sv_conv_fwd calls inside the block
    (sv_conv_set_dispatch; 1.0 = one frame alone on the GPU); afterwards the setting in force on entry is back: the
    enclosing block's pair (blocks nest; the open ones are a per-thread stack), or the library defaults at the bottom."""

    _open = threading.local()  # .stack: the (want_scale, tail_fraction) pairs of this thread's open blocks, innermost last

    def __init__(self, want_scale, tail_fraction=-1.0):
        self.args = (float(want_scale), float(tail_fraction))

    def __enter__(self):
        stack = self._open.__dict__.setdefault("stack", [])
        call("sv_conv_set_dispatch", c_double(self.args[0]), c_double(self.args[1]))
        stack.append(self.args)

    def __exit__(self, *exc):
        stack = self._open.stack
        stack.pop()
        want_scale, tail_fraction = stack[-1] if stack else (-1.0, -1.0)
        call("sv_conv_set_dispatch", c_double(want_scale), c_double(tail_fraction))


def require_cuda(t, what="tensor"):
    if not t.is_cuda:
        raise SvHipError(f"{what} must live on the GPU (got {t.device}); the HIP path has no CPU fallback")
    return t
