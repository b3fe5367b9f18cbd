"""ctypes binding of libstereonet_hip.so (include/stereonet_hip.h) — the Python face of the
drop-in boundary.  It mirrors the call sequence of the reference node:

    Init()/GetModelInputSize  -> StereoNetHIP(model_file)          stereonet_node.cpp:44-45
    Run(inputs, out, sync)    -> .infer(...) / .submit()+.wait()    stereonet_node.cpp:812,968
    CvtNV12Data2Tensors       -> .preprocess_nv12(...)              preprocess.cpp:913-1059

There is no CPU fallback: constructing StereoNetHIP without a gfx950 device raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import build as _build

SN_MEM_HOST, SN_MEM_DEVICE = 0, 1
PREC_DEFAULT, PREC_F16X3, PREC_F16, PREC_FP32, PREC_AUTO = 0, 1, 2, 3, 4      # include/stereonet_hip.h; 0 selects PREC_AUTO
PREC_NAMES = {PREC_F16X3: "f16x3", PREC_F16: "f16", PREC_FP32: "fp32", PREC_AUTO: "auto"}
ABI_VERSION = 4
SN_ERR_RANGE = -8      # include/stereonet_hip.h: the maps were written by an arithmetic that left the range of fp16
F16_MAX = 65504.0      # the largest value the fp16 modes can store between two layers
STAGES = ("features", "aggregate", "refine", "refine_conv", "total", "dominant")


class SnConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("max_batch", C.c_int), ("width", C.c_int), ("height", C.c_int),
                ("dmax", C.c_int), ("precision", C.c_int), ("task_num", C.c_int), ("refine_chunk", C.c_int),
                ("piece", C.c_int)]


class SnIoInfo(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("dmax", C.c_int), ("in_channels", C.c_int),
                ("max_batch", C.c_int), ("precision", C.c_int), ("task_num", C.c_int), ("device", C.c_int),
                ("out_scale", C.c_float), ("in_bytes", C.c_size_t), ("out_bytes", C.c_size_t),
                ("flops_per_pair", C.c_double), ("refine_chunk", C.c_int), ("piece", C.c_int),
                ("tower_streams", C.c_int), ("refine_levels", C.c_int), ("precision_selected", C.c_int)]


class SnRefineStats(C.Structure):
    """sn_refine_stats (include/stereonet_hip.h): the refinement statistic and SN_PREC_AUTO's state."""
    _fields_ = [("levels", C.c_int), ("precision", C.c_int), ("precision_selected", C.c_int), ("precision_last", C.c_int),
                ("calls", C.c_uint64), ("pairs", C.c_uint64), ("switches", C.c_uint64), ("reruns", C.c_uint64),
                ("level_px", C.c_double * 4), ("residual_px", C.c_double), ("running_px", C.c_double),
                ("envelope_px", C.c_double), ("limit_px", C.c_double), ("selfcheck_epe_px", C.c_double),
                ("selfcheck_residual_px", C.c_double), ("nonfinite_px", C.c_uint64 * 4), ("nonfinite_low_px", C.c_uint64)]


class SnAutoState(C.Structure):
    """sn_auto_state: SN_PREC_AUTO's state machine (pure functions sn_auto_*)."""
    _fields_ = [("mode", C.c_int), ("calm", C.c_int), ("envelope_px", C.c_double), ("epe_per_px", C.c_double),
                ("running_px", C.c_double), ("switches", C.c_uint64)]


class SnCamera(C.Structure):
    """sn_camera (include/stereonet_hip.h); pointcloud.Camera is the Python face of it."""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("baseline_mm", C.c_float),
                ("z_min_m", C.c_float), ("z_max_m", C.c_float), ("step", C.c_int)]


class SnLrcParams(C.Structure):
    """sn_lrc_params (include/stereonet_hip.h): tolerances of the left-right consistency check."""
    _fields_ = [("tau_px", C.c_float), ("tau_rel", C.c_float), ("right_mirrored", C.c_int)]


class SnFilterParams(C.Structure):
    """sn_filter_params (include/stereonet_hip.h): speckle removal and hole filling of the int32 map."""
    _fields_ = [("speckle_max_px", C.c_int), ("speckle_diff_px", C.c_float), ("fill_max_px", C.c_int)]


class SnConfParams(C.Structure):
    """sn_conf_params (include/stereonet_hip.h): the confidence threshold, 0..1."""
    _fields_ = [("min_conf", C.c_float)]


class SnSmoothParams(C.Structure):
    """sn_smooth_params (include/stereonet_hip.h): guided weighted-median smoothing of the int32 map."""
    _fields_ = [("radius", C.c_int), ("sigma_luma", C.c_int), ("min_valid", C.c_int)]


class SnTemporalParams(C.Structure):
    """sn_temporal_params (include/stereonet_hip.h): the temporal filter of disparity streams."""
    _fields_ = [("alpha", C.c_int), ("delta_px", C.c_float), ("persist", C.c_int), ("luma_delta", C.c_int)]


class SnEyeCalib(C.Structure):
    """sn_eye_calib (include/stereonet_hip.h); rectify.Eye is the Python face of it."""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("d", C.c_double * 5),
                ("R", C.c_double * 9)]


class SnStereoCalib(C.Structure):
    """sn_stereo_calib (include/stereonet_hip.h); rectify.Calib is the Python face of it."""
    _fields_ = [("src_w", C.c_int), ("src_h", C.c_int), ("left", SnEyeCalib), ("right", SnEyeCalib), ("pfx", C.c_double),
                ("pfy", C.c_double), ("pcx", C.c_double), ("pcy", C.c_double), ("baseline_mm", C.c_double)]


class SnJpegParams(C.Structure):
    """sn_jpeg_params (include/stereonet_hip.h)"""
    _fields_ = [("quality", C.c_int), ("rows_per_slice", C.c_int)]


class SnRenderParams(C.Structure):
    """sn_render_params (include/stereonet_hip.h); render.RenderParams is the Python face of it.  All zero: the reference's
    render node."""
    _fields_ = [("scale", C.c_double), ("focal_px", C.c_double), ("baseline_mm", C.c_double), ("alpha", C.c_double),
                ("layout", C.c_int), ("colormap", C.c_int), ("true_colours", C.c_int), ("invalid_black", C.c_int)]


def render_params(p=None) -> SnRenderParams:
    """render.RenderParams (or None: the reference's render node) -> sn_render_params"""
    if isinstance(p, SnRenderParams):
        return p
    if p is None:
        return SnRenderParams()
    return SnRenderParams(p.scale, p.focal_px, p.baseline_mm, p.alpha, p.layout, p.colormap, p.true_colours, p.invalid_black)


class SnObstacleParams(C.Structure):
    """sn_obstacle_params (include/stereonet_hip.h); obstacles.ObstacleParams is the Python face of it."""
    _fields_ = [("base_from_cam", C.c_float * 12), ("x_min_m", C.c_float), ("y_min_m", C.c_float), ("cell_m", C.c_float),
                ("gw", C.c_int), ("gh", C.c_int), ("z_floor_m", C.c_float), ("z_lo_m", C.c_float), ("z_hi_m", C.c_float),
                ("min_obstacle_hits", C.c_int), ("min_ground_hits", C.c_int), ("beams", C.c_int), ("angle_min_rad", C.c_float),
                ("angle_increment_rad", C.c_float), ("range_min_m", C.c_float), ("range_max_m", C.c_float)]


def obstacle_params(p) -> SnObstacleParams:
    """obstacles.ObstacleParams -> sn_obstacle_params"""
    if isinstance(p, SnObstacleParams):
        return p
    return SnObstacleParams((C.c_float * 12)(*p.base_from_cam), p.x_min_m, p.y_min_m, p.cell_m, p.gw, p.gh, p.z_floor_m, p.z_lo_m,
                            p.z_hi_m, p.min_obstacle_hits, p.min_ground_hits, p.beams, p.angle_min_rad, p.angle_increment_rad,
                            p.range_min_m, p.range_max_m)


class SnGroundParams(C.Structure):
    """sn_ground_params (include/stereonet_hip.h); ground.GroundParams is the Python face of it."""
    _fields_ = [("base_from_cam", C.c_float * 12), ("roi_x", C.c_int), ("roi_y", C.c_int), ("roi_w", C.c_int), ("roi_h", C.c_int),
                ("hypotheses", C.c_int), ("seed", C.c_uint32), ("min_area", C.c_int), ("min_inliers", C.c_int), ("refits", C.c_int),
                ("tol_px", C.c_float), ("max_tilt_rad", C.c_float), ("height_min_m", C.c_float), ("height_max_m", C.c_float)]


class SnGround(C.Structure):
    """sn_ground (include/stereonet_hip.h); ground.RECORD is the numpy dtype of it."""
    _fields_ = [("flags", C.c_uint32), ("usable", C.c_uint32), ("inliers", C.c_uint32), ("winner", C.c_int32), ("survivors", C.c_uint32),
                ("reserved", C.c_uint32), ("plane_q16", C.c_int64 * 3), ("plane_cam", C.c_float * 4), ("base_from_cam", C.c_float * 12)]


def ground_params(p) -> SnGroundParams:
    """ground.GroundParams -> sn_ground_params"""
    if isinstance(p, SnGroundParams):
        return p
    return SnGroundParams((C.c_float * 12)(*p.base_from_cam), p.roi_x, p.roi_y, p.roi_w, p.roi_h, p.hypotheses, p.seed, p.min_area,
                          p.min_inliers, p.refits, p.tol_px, p.max_tilt_rad, p.height_min_m, p.height_max_m)


class SnCostmapParams(C.Structure):
    """sn_costmap_params (include/stereonet_hip.h); costmap.CostmapParams is the Python face of it."""
    _fields_ = [("mw", C.c_int), ("mh", C.c_int), ("l_hit", C.c_int), ("l_miss", C.c_int), ("l_min", C.c_int), ("l_max", C.c_int),
                ("clear_margin_m", C.c_float), ("clear_min_m", C.c_float), ("clear_max_m", C.c_float)]


def costmap_params(p) -> SnCostmapParams:
    """costmap.CostmapParams -> sn_costmap_params"""
    if isinstance(p, SnCostmapParams):
        return p
    return SnCostmapParams(p.mw, p.mh, p.l_hit, p.l_miss, p.l_min, p.l_max, p.clear_margin_m, p.clear_min_m, p.clear_max_m)


class SnElevationParams(C.Structure):
    """sn_elevation_params (include/stereonet_hip.h); elevation.ElevationParams is the Python face of it."""
    _fields_ = [("mw", C.c_int), ("mh", C.c_int), ("cell_m", C.c_float), ("base_from_cam", C.c_float * 12), ("z_min_m", C.c_float),
                ("z_max_m", C.c_float), ("range_max_m", C.c_float), ("min_points", C.c_int), ("alpha", C.c_int),
                ("max_step_mm", C.c_int), ("radius", C.c_int), ("flags", C.c_int)]


def elevation_params(p) -> SnElevationParams:
    """elevation.ElevationParams -> sn_elevation_params"""
    if isinstance(p, SnElevationParams):
        return p
    return SnElevationParams(p.mw, p.mh, p.cell_m, (C.c_float * 12)(*p.base_from_cam), p.z_min_m, p.z_max_m, p.range_max_m,
                             p.min_points, p.alpha, p.max_step_mm, p.radius, p.flags)


class SnInflateParams(C.Structure):
    """sn_inflate_params (include/stereonet_hip.h); inflate.InflateParams is the Python face of it."""
    _fields_ = [("cell_m", C.c_float), ("inscribed_radius_m", C.c_float), ("inflation_radius_m", C.c_float), ("cost_scaling", C.c_float),
                ("lethal_min", C.c_int), ("flags", C.c_int)]


def inflate_params(p) -> SnInflateParams:
    """inflate.InflateParams -> sn_inflate_params"""
    if isinstance(p, SnInflateParams):
        return p
    return SnInflateParams(p.cell_m, p.inscribed_radius_m, p.inflation_radius_m, p.cost_scaling, p.lethal_min, p.flags)


class SnNavParams(C.Structure):
    """sn_nav_params (include/stereonet_hip.h); navfn.NavParams is the Python face of it."""
    _fields_ = [("neutral", C.c_int), ("lethal_cost", C.c_int), ("unknown_cost", C.c_int), ("flags", C.c_int), ("max_rounds", C.c_int),
                ("max_path", C.c_int)]


def nav_params(p) -> SnNavParams:
    """navfn.NavParams -> sn_nav_params"""
    if isinstance(p, SnNavParams):
        return p
    return SnNavParams(p.neutral, p.lethal_cost, p.unknown_cost, p.flags, p.max_rounds, p.max_path)


class SnRolloutParams(C.Structure):
    """sn_rollout_params (include/stereonet_hip.h); rollout.RolloutParams is the Python face of it."""
    _fields_ = [("cell_m", C.c_float), ("v_min", C.c_float), ("v_max", C.c_float), ("nv", C.c_int), ("w_min", C.c_float),
                ("w_max", C.c_float), ("nw", C.c_int), ("sim_time_s", C.c_float), ("steps", C.c_int), ("lethal_cost", C.c_int),
                ("centre_lethal_cost", C.c_int), ("unknown_cost", C.c_int), ("flags", C.c_int), ("w_goal", C.c_int), ("w_occ", C.c_int)]


def rollout_params(p) -> SnRolloutParams:
    """rollout.RolloutParams -> sn_rollout_params"""
    if isinstance(p, SnRolloutParams):
        return p
    return SnRolloutParams(p.cell_m, p.v_min, p.v_max, p.nv, p.w_min, p.w_max, p.nw, p.sim_time_s, p.steps, p.lethal_cost,
                           p.centre_lethal_cost, p.unknown_cost, p.flags, p.w_goal, p.w_occ)


def _footprint(params, footprint) -> np.ndarray:
    """float32 (nf, 2): `footprint`, or the one a rollout.RolloutParams carries"""
    fp = getattr(params, "footprint", ()) if footprint is None else footprint
    return np.ascontiguousarray(np.asarray(fp, np.float32).reshape(-1, 2))


class SnRectifyInfo(C.Structure):
    _fields_ = [("src_w", C.c_int), ("src_h", C.c_int), ("w", C.c_int), ("h", C.c_int), ("valid_left", C.c_uint32),
                ("valid_right", C.c_uint32)]


def stereo_calib(c) -> SnStereoCalib:
    """rectify.Calib -> sn_stereo_calib"""
    if isinstance(c, SnStereoCalib):
        return c
    eyes = [SnEyeCalib(e.fx, e.fy, e.cx, e.cy, (C.c_double * 5)(*e.d), (C.c_double * 9)(*e.R)) for e in (c.left, c.right)]
    return SnStereoCalib(int(c.src_w), int(c.src_h), eyes[0], eyes[1], c.pfx, c.pfy, c.pcx, c.pcy, c.baseline_mm)


SN_FLT_INVALID_IN, SN_FLT_SPECKLE, SN_FLT_FILLED = 1, 16, 32
SN_TMP_INVALID_IN, SN_TMP_BLENDED, SN_TMP_HELD, SN_TMP_MOVED, SN_TMP_JUMP = 1, 2, 4, 8, 16      # a mask plane of its own
SN_SMOOTH_INVALID_IN, SN_SMOOTH_CHANGED = 1, 128
SN_GUIDE_NV12, SN_GUIDE_TENSOR = 0, 1
SN_CONF_KEPT, SN_CONF_INVALID_IN, SN_CONF_LOW = 0, 1, 64
SN_LRC_KEPT, SN_LRC_INVALID_IN, SN_LRC_OUT_OF_VIEW, SN_LRC_NO_PARTNER, SN_LRC_INCONSISTENT = 0, 1, 2, 4, 8
SN_LRC_IN_TENSOR, SN_LRC_IN_SBS_NV12 = 0, 1


class StereoNetError(RuntimeError):
    def __init__(self, code: int, where: str, detail: str = ""):
        self.code = code
        super().__init__(f"{where}: {error_string(code)} (code {code}){': ' + detail if detail else ''}")


class StereoNetRangeError(StereoNetError):
    """SN_ERR_RANGE: the call ran and its maps were written, by an arithmetic in which activations left the range of fp16
    (65504) — they are not to be used; run such a model with precision=PREC_FP32.  nonfinite_px[k]: pixels of refinement level
    k whose disparity was not finite before the head's relu; nonfinite_low_px: low-resolution pixels with a non-finite
    matching cost; outputs: what the call would have returned (StereoNetHIP.infer and the calls built like it), for
    diagnosis only."""

    def __init__(self, where: str, detail: str, nonfinite_px, nonfinite_low_px):
        super().__init__(SN_ERR_RANGE, where, detail)
        self.nonfinite_px = list(nonfinite_px)
        self.nonfinite_low_px = int(nonfinite_low_px)
        self.outputs = None


_lib = None


def load_library(path: Optional[str] = None):
    """Loads (building if stale and hipcc is present) libstereonet_hip.so."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("STEREONET_HIP_LIB") or _build.LIB      # STEREONET_HIP_LIB: A/B builds of the library
    # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64/libhsa-runtime64.  If this library
    # came in first it would bind the system ROCm copies, torch would later add its own, and whichever runtime
    # opened the device second would report "no ROCm-capable device".  Importing torch first makes both share
    # torch's copy (same SONAME); without torch installed the system runtime is the only one.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(path) or (os.path.exists(_build.HIPCC) and _build.is_stale()):
        _build.build()
    lib = C.CDLL(path)
    vp, ip, i8p, i32p, fp, u8p = C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p
    lib.sn_create.argtypes = [C.c_char_p, C.POINTER(SnConfig), C.POINTER(vp)]
    lib.sn_destroy.argtypes = [vp]
    lib.sn_get_io_info.argtypes = [vp, C.POINTER(SnIoInfo)]
    lib.sn_strerror.restype = C.c_char_p
    lib.sn_strerror.argtypes = [ip]
    lib.sn_last_error.restype = C.c_char_p
    lib.sn_last_error.argtypes = [vp]
    lib.sn_infer_i8.argtypes = [vp, i8p, i32p, fp, ip, vp]
    lib.sn_infer_batch.argtypes = [vp, ip, i8p, i32p, fp, ip, vp]
    lib.sn_preprocess_nv12.argtypes = [vp, u8p, u8p, ip, ip, i8p, ip, vp]
    lib.sn_infer_sbs_nv12.argtypes = [vp, u8p, ip, ip, i32p, fp, i8p, ip, vp]
    lib.sn_preprocess_sbs_nv12_batch.argtypes = [vp, ip, u8p, ip, ip, i8p, ip, vp]
    lib.sn_submit.argtypes = [vp, i8p, i32p, fp, ip, C.POINTER(C.c_uint64)]
    lib.sn_submit_nv12.argtypes = [vp, u8p, ip, ip, i32p, fp, ip, C.POINTER(C.c_uint64)]
    lib.sn_wait.argtypes = [vp, C.c_uint64, C.POINTER(C.c_float)]
    lib.sn_synchronize.argtypes = [vp]
    lib.sn_set_profiling.argtypes = [vp, ip]
    lib.sn_get_stage_ms.argtypes = [vp, C.POINTER(C.c_float), ip]
    lib.sn_get_dominant_kernel.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(ip), C.POINTER(C.c_double),
                                           C.POINTER(C.c_double)]
    lib.sn_mgpu_shard.argtypes = [ip, ip, ip, C.POINTER(ip), C.POINTER(ip)]
    lib.sn_mgpu_create.argtypes = [C.c_char_p, C.POINTER(SnConfig), C.POINTER(ip), ip, C.POINTER(vp)]
    lib.sn_mgpu_destroy.argtypes = [vp]
    lib.sn_mgpu_get_info.argtypes = [vp, C.POINTER(ip), C.POINTER(ip), C.POINTER(ip)]
    lib.sn_mgpu_get_handle.argtypes = [vp, ip, C.POINTER(vp)]
    lib.sn_mgpu_infer_batch.argtypes = [vp, ip, i8p, i32p, fp]
    lib.sn_mgpu_infer_batch_device.argtypes = [vp, ip, C.POINTER(vp), i32p, fp]
    lib.sn_mgpu_submit_device.argtypes = [vp, ip, C.POINTER(vp), i32p, fp, C.POINTER(C.c_uint64)]
    lib.sn_mgpu_wait.argtypes = [vp, C.c_uint64]
    lib.sn_mgpu_ring_init.argtypes = [vp]
    lib.sn_mgpu_ring_submit.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(ip)]
    lib.sn_mgpu_ring_wait.argtypes = [vp, C.c_uint64, C.POINTER(ip)]
    lib.sn_mgpu_last_error.restype = C.c_char_p
    lib.sn_mgpu_last_error.argtypes = [vp]
    # the parity hooks; tests/test_cabi.py holds every list to the parameter count of its prototype in the header
    lib.sn_dbg_conv2d_n.argtypes = [vp, ip, fp, ip, ip, ip, fp, fp, ip, ip, ip, ip, ip, fp, fp]
    lib.sn_dbg_conv3d.argtypes = [vp, fp, ip, ip, ip, fp, fp, ip, ip, fp]
    lib.sn_dbg_down0_n.argtypes = [vp, ip, i8p, ip, ip, fp, fp, ip, fp]
    lib.sn_dbg_compose_down01.argtypes = [fp, fp, fp, fp, fp, fp]
    lib.sn_dbg_round_kernels_f16.argtypes = [fp, ip, fp]
    lib.sn_dbg_down01_n.argtypes = [vp, ip, i8p, ip, ip, fp, fp, fp, fp, fp]
    lib.sn_dbg_refin_n.argtypes = [vp, ip, fp, i8p, ip, ip, ip, fp, fp, ip, fp]
    lib.sn_dbg_ref_conv_f16_n.argtypes = [vp, ip, fp, ip, ip, fp, fp, ip, ip, ip, fp, fp]
    lib.sn_dbg_ref_conv_f16x3_n.argtypes = [vp, ip, fp, ip, ip, fp, fp, ip, ip, fp, fp]
    lib.sn_dbg_ref_block_f16_n.argtypes = [vp, ip, fp, ip, ip, fp, fp, fp, fp, ip, ip, fp]
    lib.sn_dbg_ref_block_f16x3_n.argtypes = [vp, ip, fp, ip, ip, fp, fp, fp, fp, ip, ip, fp]
    lib.sn_dbg_ref_tail_f16.argtypes = [vp, ip, fp, ip, ip, fp, fp, fp, fp, fp, C.c_float, fp, ip, C.c_float, ip, ip, ip, fp, i32p]
    lib.sn_dbg_read.argtypes = [vp, C.c_char_p, fp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.sn_dbg_set_grid_cus.argtypes = [vp, ip]
    lib.sn_dbg_last_launch.argtypes = [vp, C.POINTER(ip), C.POINTER(ip)]
    lib.sn_dbg_slot_graphs.argtypes = [vp, C.POINTER(ip), C.POINTER(ip), C.POINTER(ip)]
    u64p = C.POINTER(C.c_uint64)
    lib.sn_dbg_cost_volume.argtypes = [vp, fp, ip, ip, ip, ip, ip, fp]
    lib.sn_dbg_agg_first_f32.argtypes = [vp, fp, ip, ip, ip, ip, fp, fp, fp]
    lib.sn_dbg_softargmin.argtypes = [vp, ip, ip, ip, ip, ip, ip, C.c_float, fp, fp, fp, fp, fp, u64p]
    lib.sn_dbg_agg_tail.argtypes = [vp, fp, ip, ip, ip, ip, fp, fp, fp, C.c_float, ip, ip, fp, fp, fp, u64p, fp]
    lib.sn_dbg_head.argtypes = [vp, ip, fp, ip, ip, fp, C.c_float, fp, ip, C.c_float, ip, ip, ip, fp, i32p, C.POINTER(C.c_double), u64p]
    lib.sn_dbg_img_pool2.argtypes = [vp, i8p, ip, ip, ip, ip, fp]
    lib.sn_dbg_copy_limited.argtypes = [vp, vp, C.c_size_t, ip, vp]
    lib.sn_depth_from_raw.argtypes = [vp, ip, i32p, C.c_float, C.c_float, fp, fp, ip, vp]
    lib.sn_pointcloud_from_raw.argtypes = [vp, ip, i32p, u8p, ip, C.POINTER(SnCamera), ip, fp, vp, ip, vp]
    lib.sn_mirror_pair_i8.argtypes = [vp, ip, i8p, i8p, ip, vp]
    lib.sn_lr_check.argtypes = [vp, ip, i32p, i32p, C.POINTER(SnLrcParams), i32p, fp, u8p, vp, ip, vp]
    lib.sn_infer_lrc.argtypes = [vp, ip, vp, ip, ip, ip, C.POINTER(SnLrcParams), i32p, fp, i32p, u8p, vp, ip, vp]
    lib.sn_filter_raw.argtypes = [vp, ip, i32p, C.POINTER(SnFilterParams), i32p, fp, u8p, vp, ip, vp]
    lib.sn_smooth_raw.argtypes = [vp, ip, i32p, vp, ip, ip, C.POINTER(SnSmoothParams), i32p, fp, u8p, vp, ip, vp]
    lib.sn_temporal_create.argtypes = [vp, ip, C.POINTER(SnTemporalParams), C.POINTER(vp)]
    lib.sn_temporal_reset.argtypes = [vp, ip]
    lib.sn_temporal_destroy.argtypes = [vp]
    lib.sn_temporal_destroy.restype = None
    lib.sn_temporal_push.argtypes = [vp, ip, vp, i32p, vp, ip, ip, i32p, fp, u8p, vp, ip, vp]
    lib.sn_rectify_build_map.argtypes = [C.POINTER(SnStereoCalib), ip, ip, ip, i32p]
    lib.sn_rectify_create.argtypes = [vp, C.POINTER(SnStereoCalib), C.POINTER(vp)]
    lib.sn_rectify_destroy.argtypes = [vp]
    lib.sn_rectify_destroy.restype = None
    lib.sn_rectify_get_info.argtypes = [vp, C.POINTER(SnRectifyInfo)]
    lib.sn_rectify_get_camera.argtypes = [vp, C.POINTER(SnCamera)]
    lib.sn_rectify_get_map.argtypes = [vp, ip, i32p]
    lib.sn_rectify_nv12.argtypes = [vp, ip, u8p, u8p, ip, C.c_size_t, u8p, i8p, ip, vp]
    lib.sn_jpeg_bound.argtypes = [ip, ip]
    lib.sn_jpeg_bound.restype = C.c_size_t
    lib.sn_jpeg_encode_nv12.argtypes = [vp, ip, u8p, ip, ip, ip, C.c_size_t, C.POINTER(SnJpegParams), u8p, C.c_size_t, vp, ip, vp]
    lib.sn_dbg_jpeg_dct.argtypes = [vp, u8p, ip, ip, ip, fp]
    lib.sn_render_tables.argtypes = [C.POINTER(SnRenderParams), u8p, u8p]
    lib.sn_render.argtypes = [vp, ip, i32p, u8p, ip, C.POINTER(SnRenderParams), ip, u8p, ip, C.c_size_t, ip, vp]
    lib.sn_render_jpeg.argtypes = [vp, ip, i32p, u8p, ip, C.POINTER(SnRenderParams), C.POINTER(SnJpegParams), u8p, C.c_size_t, vp, ip, vp]
    lib.sn_obstacle_beam_edges.argtypes = [C.POINTER(SnObstacleParams), fp]
    lib.sn_obstacles_from_raw.argtypes = [vp, ip, i32p, C.POINTER(SnCamera), C.POINTER(SnObstacleParams), vp, vp, i32p, fp, vp, ip, vp]
    lib.sn_obstacles_from_raw_mounts.argtypes = [vp, ip, i32p, C.POINTER(SnCamera), C.POINTER(SnObstacleParams), fp, ip, vp, vp, i32p, fp, vp,
                                                 ip, vp]
    lib.sn_ground_gate.argtypes = [C.POINTER(SnCamera), C.POINTER(SnGroundParams), ip, ip, vp]
    lib.sn_ground_from_raw.argtypes = [vp, ip, i32p, C.POINTER(SnCamera), C.POINTER(SnGroundParams), vp, u8p, ip, vp]
    lib.sn_costmap_create.argtypes = [vp, ip, C.POINTER(SnObstacleParams), C.POINTER(SnCostmapParams), C.POINTER(vp)]
    lib.sn_costmap_reset.argtypes = [vp, ip]
    lib.sn_costmap_destroy.argtypes = [vp]
    lib.sn_costmap_destroy.restype = None
    lib.sn_costmap_pose_q.argtypes = [vp, vp, i32p]
    lib.sn_costmap_push.argtypes = [vp, ip, vp, vp, i8p, fp, i8p, vp, vp, i32p, ip, vp]
    lib.sn_elevation_create.argtypes = [vp, ip, C.POINTER(SnElevationParams), C.POINTER(vp)]
    lib.sn_elevation_reset.argtypes = [vp, ip]
    lib.sn_elevation_destroy.argtypes = [vp]
    lib.sn_elevation_destroy.restype = None
    lib.sn_elevation_pose_q.argtypes = [vp, vp, i32p]
    lib.sn_elevation_push.argtypes = [vp, ip, vp, vp, vp, C.POINTER(SnCamera), vp, ip, vp, vp, vp, vp, vp, i32p, ip, vp]
    lib.sn_inflate_table.argtypes = [C.POINTER(SnInflateParams), u8p, C.POINTER(C.c_int)]
    lib.sn_inflate_grid.argtypes = [vp, ip, i8p, ip, ip, C.POINTER(SnInflateParams), u8p, i8p, vp, vp, ip, vp]
    lib.sn_navfn.argtypes = [vp, ip, u8p, ip, ip, i32p, i32p, C.POINTER(SnNavParams), vp, i32p, vp, C.POINTER(C.c_int), ip, vp]
    lib.sn_rollout_tables.argtypes = [C.POINTER(SnRolloutParams), vp, ip, vp, vp]
    lib.sn_rollout_pose_q.argtypes = [C.c_float, C.c_double, C.c_double, vp, vp]
    lib.sn_rollout_velocity.argtypes = [C.POINTER(SnRolloutParams), ip, vp]
    lib.sn_rollout.argtypes = [vp, ip, vp, vp, ip, ip, vp, vp, C.POINTER(SnRolloutParams), vp, ip, vp, vp, vp, ip, vp]
    lib.sn_infer_conf.argtypes = [vp, ip, vp, ip, ip, ip, C.POINTER(SnConfParams), i32p, fp, fp, u8p, vp, ip, vp]
    lib.sn_conf_mask.argtypes = [vp, ip, i32p, fp, C.POINTER(SnConfParams), i32p, fp, u8p, vp, ip, vp]
    lib.sn_get_refine_stats.argtypes = [vp, C.POINTER(SnRefineStats)]
    lib.sn_auto_init.argtypes = [C.POINTER(SnAutoState), ip]
    lib.sn_auto_observe.argtypes = [C.POINTER(SnAutoState), C.c_double]
    lib.sn_auto_limit_px.argtypes = [C.POINTER(SnAutoState)]
    lib.sn_auto_limit_px.restype = C.c_double
    lib.sn_auto_envelope_px.argtypes = [ip]
    lib.sn_auto_envelope_px.restype = C.c_double
    for name in ("sn_create", "sn_destroy", "sn_get_io_info", "sn_infer_i8", "sn_infer_batch", "sn_preprocess_nv12",
                 "sn_infer_sbs_nv12", "sn_preprocess_sbs_nv12_batch", "sn_submit", "sn_submit_nv12", "sn_wait", "sn_synchronize", "sn_set_profiling",
                 "sn_get_stage_ms", "sn_get_dominant_kernel", "sn_mgpu_shard", "sn_mgpu_create", "sn_mgpu_destroy",
                 "sn_mgpu_get_info", "sn_mgpu_get_handle", "sn_mgpu_infer_batch", "sn_mgpu_infer_batch_device",
                 "sn_mgpu_submit_device", "sn_mgpu_wait", "sn_mgpu_ring_init", "sn_mgpu_ring_submit", "sn_mgpu_ring_wait", "sn_dbg_compose_down01", "sn_dbg_round_kernels_f16", "sn_dbg_conv3d", "sn_dbg_ref_tail_f16", "sn_dbg_set_grid_cus", "sn_dbg_last_launch", "sn_dbg_slot_graphs", "sn_dbg_conv2d_n", "sn_dbg_down0_n", "sn_dbg_down01_n", "sn_dbg_refin_n", "sn_dbg_ref_conv_f16_n", "sn_dbg_ref_conv_f16x3_n", "sn_dbg_ref_block_f16_n", "sn_dbg_ref_block_f16x3_n", "sn_dbg_cost_volume", "sn_dbg_agg_first_f32", "sn_dbg_softargmin", "sn_dbg_agg_tail", "sn_dbg_head", "sn_dbg_img_pool2", "sn_dbg_read", "sn_dbg_copy_limited", "sn_depth_from_raw", "sn_pointcloud_from_raw", "sn_mirror_pair_i8", "sn_lr_check", "sn_infer_lrc", "sn_filter_raw", "sn_smooth_raw", "sn_temporal_create", "sn_temporal_reset", "sn_temporal_push", "sn_rectify_build_map", "sn_rectify_create", "sn_rectify_get_info", "sn_rectify_get_camera", "sn_rectify_get_map", "sn_rectify_nv12", "sn_jpeg_encode_nv12", "sn_dbg_jpeg_dct", "sn_render_tables", "sn_render", "sn_render_jpeg", "sn_obstacle_beam_edges", "sn_obstacles_from_raw", "sn_obstacles_from_raw_mounts", "sn_ground_gate", "sn_ground_from_raw", "sn_costmap_create", "sn_costmap_reset", "sn_costmap_pose_q", "sn_costmap_push", "sn_elevation_create", "sn_elevation_reset", "sn_elevation_pose_q", "sn_elevation_push", "sn_inflate_table", "sn_inflate_grid", "sn_navfn", "sn_rollout_tables", "sn_rollout_pose_q", "sn_rollout_velocity", "sn_rollout", "sn_infer_conf", "sn_conf_mask", "sn_get_refine_stats", "sn_auto_init", "sn_auto_observe"):
        getattr(lib, name).restype = C.c_int
    _lib = lib
    return lib


def round_kernels_f16(w):
    """The fp16 rounding SN_PREC_F16 applies to its tower's 3x3 weights at model load (host only): w (..., 3, 3) float32 ->
    same shape, fp16-representable float32, the sum of every kernel's nine rounding errors minimised."""
    a = np.ascontiguousarray(w, np.float32)
    assert a.shape[-2:] == (3, 3)
    out = np.empty_like(a)
    rc = load_library().sn_dbg_round_kernels_f16(a.ctypes.data, a.size // 9, out.ctypes.data)
    if rc:
        raise StereoNetError(rc, "sn_dbg_round_kernels_f16")
    return out


def compose_down01(w0, b0, w1, b1):
    """Host-side fold of the first two down-convs (no device needed): -> (weff (9,32,3,13,13), beff (9,32)) float32;
    class = 3 * row class + column class, each {first, inner, last} row / column of the quarter-resolution map."""
    w0, b0, w1, b1 = (np.ascontiguousarray(a, np.float32) for a in (w0, b0, w1, b1))
    assert w0.shape == (32, 3, 5, 5) and w1.shape == (32, 32, 5, 5) and b0.shape == (32,) and b1.shape == (32,)
    weff = np.empty((9, 32, 3, 13, 13), np.float32)
    beff = np.empty((9, 32), np.float32)
    rc = load_library().sn_dbg_compose_down01(w0.ctypes.data, b0.ctypes.data, w1.ctypes.data, b1.ctypes.data,
                                              weff.ctypes.data, beff.ctypes.data)
    if rc:
        raise StereoNetError(rc, "sn_dbg_compose_down01")
    return weff, beff


def rectify_build_map(calib, eye: int, w: int, h: int) -> np.ndarray:
    """sn_rectify_build_map (host only, no device needed): Stage A of rectify.build_map by the library -> int32 (h, w, 2)."""
    c = stereo_calib(calib)
    out = np.empty((max(h, 0), max(w, 0), 2), np.int32)
    rc = load_library().sn_rectify_build_map(C.byref(c), eye, w, h, out.ctypes.data)
    if rc:
        raise StereoNetError(rc, "sn_rectify_build_map")
    return out


def jpeg_bound(w: int, h: int) -> int:
    """sn_jpeg_bound (host only): a capacity no JPEG stream of a w x h image can exceed; 0 for a size the encoder does not take"""
    return int(load_library().sn_jpeg_bound(w, h))


def render_tables(params=None):
    """sn_render_tables (host only): -> (rgb, ycc) uint8 (257, 3), the canvas bytes of every colour index and their YCbCr;
    render.render_tables is the numpy twin."""
    prm = render_params(params)
    rgb, ycc = np.empty((257, 3), np.uint8), np.empty((257, 3), np.uint8)
    rc = load_library().sn_render_tables(C.byref(prm), rgb.ctypes.data, ycc.ctypes.data)
    if rc:
        raise StereoNetError(rc, "sn_render_tables")
    return rgb, ycc


def beam_edges(params) -> np.ndarray:
    """sn_obstacle_beam_edges (host only): float32 (beams + 1,), the tangents that bound the beams of the scan;
    obstacles.beam_edges is the numpy twin (the two may differ by an ulp: two implementations of a double tan)."""
    prm = obstacle_params(params)
    edges = np.empty(max(prm.beams, 0) + 1, np.float32)
    rc = load_library().sn_obstacle_beam_edges(C.byref(prm), edges.ctypes.data)
    if rc:
        raise StereoNetError(rc, "sn_obstacle_beam_edges")
    return edges


def _sn_camera(cam, w: int, h: int) -> "SnCamera":
    c = cam.resolved(w, h)
    return SnCamera(c.fx, c.fy, c.cx, c.cy, c.baseline_mm, c.z_min_m, c.z_max_m, c.step)


def ground_gate(cam, params, w: int, h: int) -> np.ndarray:
    """sn_ground_gate (host only): int64 (6,), the Q16 bounds on the plane's a, b and c that a hypothesis must meet;
    ground.gate is the numpy twin (the two may differ by one: two implementations of a double cos and sin)."""
    c, prm = _sn_camera(cam, w, h), ground_params(params)
    gate = np.empty(6, np.int64)
    rc = load_library().sn_ground_gate(C.byref(c), C.byref(prm), w, h, gate.ctypes.data)
    if rc:
        raise StereoNetError(rc, "sn_ground_gate")
    return gate


def _pose_q_rows(fn, obj, poses):
    """poses (x, y, yaw) or (n, 3) through the sn_*_pose_q `fn` of `obj` -> (q int32 (6,) or (n, 6), 0, n), or (None, rc, k)
    at the first pose k that the library refuses"""
    ps = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
    q = np.empty((ps.shape[0], 6), np.int32)
    for k in range(ps.shape[0]):
        rc = fn(obj, ps[k].ctypes.data, q[k].ctypes.data)
        if rc:
            return None, rc, k
    return (q[0] if np.ndim(poses) == 1 else q), 0, ps.shape[0]


def _host_pose_q(sym: str, create_args, poses) -> np.ndarray:
    """sn_costmap_pose_q / sn_elevation_pose_q on an object made without an engine (`sym`_create(NULL, 1, ...))"""
    lib, o = load_library(), C.c_void_p()
    rc = getattr(lib, sym + "_create")(None, 1, *create_args, C.byref(o))
    if rc:
        raise StereoNetError(rc, sym + "_create")
    try:
        q, rc, k = _pose_q_rows(getattr(lib, sym + "_pose_q"), o, poses)
    finally:
        getattr(lib, sym + "_destroy")(o)
    if rc:
        raise StereoNetError(rc, sym + "_pose_q", f"pose {k}: {np.asarray(poses, np.float64).reshape(-1, 3)[k].tolist()}")
    return q


def costmap_pose_q(params, obstacle, poses) -> np.ndarray:
    """sn_costmap_pose_q (host only: a costmap without an engine serves it): poses (x, y, yaw) or (n, 3) -> int32 (6,) or
    (n, 6) = {tx, ty, cq, sq, ox, oy}; costmap.pose_q is the Python twin (the two may differ by one unit in cq and sq: two
    implementations of a double cos and sin)."""
    prm, op = costmap_params(params), obstacle_params(obstacle)
    return _host_pose_q("sn_costmap", (C.byref(op), C.byref(prm)), poses)


def elevation_pose_q(params, poses) -> np.ndarray:
    """sn_elevation_pose_q (host only: an elevation object without an engine serves it): poses (x, y, yaw) or (n, 3) -> int32
    (6,) or (n, 6) = {tx, ty, cq, sq, ox, oy}; elevation.pose_q is the Python twin (the two may differ by one unit in cq and sq:
    two implementations of a double cos and sin)."""
    prm = elevation_params(params)
    return _host_pose_q("sn_elevation", (C.byref(prm),), poses)


def inflate_table(params) -> np.ndarray:
    """sn_inflate_table (host only): uint8 (R*R + 1,), the cost of every squared distance in cells up to the inflation radius;
    inflate.table is the Python twin (an entry of the fall-off may differ by one: two implementations of a double exp)."""
    lib, prm, R = load_library(), inflate_params(params), C.c_int(0)
    rc = lib.sn_inflate_table(C.byref(prm), None, C.byref(R))
    if rc:
        raise StereoNetError(rc, "sn_inflate_table")
    T = np.empty(R.value * R.value + 1, np.uint8)
    rc = lib.sn_inflate_table(C.byref(prm), T.ctypes.data, None)
    if rc:
        raise StereoNetError(rc, "sn_inflate_table")
    return T


def rollout_tables(params, footprint=None):
    """sn_rollout_tables (host only) -> (centres int32 (S, T+1, 3), offsets int32 (nw, T+1, nf, 2)); footprint (nf, 2) in metres,
    or the one `params` carries; rollout.tables is the Python restatement (an entry may differ by one: two libms)."""
    lib, prm, fp = load_library(), rollout_params(params), _footprint(params, footprint)
    nf = fp.shape[0]
    if lib.sn_rollout_tables(C.byref(prm), fp.ctypes.data, nf, None, None):      # the sizes below only mean something once accepted
        raise StereoNetError(-1, "sn_rollout_tables")
    centres = np.empty((prm.nv * prm.nw, prm.steps + 1, 3), np.int32)
    offsets = np.empty((prm.nw, prm.steps + 1, nf, 2), np.int32)
    rc = lib.sn_rollout_tables(C.byref(prm), fp.ctypes.data, nf, centres.ctypes.data, offsets.ctypes.data)
    if rc:
        raise StereoNetError(rc, "sn_rollout_tables")
    return centres, offsets


def rollout_pose_q(cell_m: float, origin_x_m: float, origin_y_m: float, poses) -> np.ndarray:
    """sn_rollout_pose_q (host only): poses (x, y, yaw) or (n, 3) -> int32 (5,) or (n, 5) = {px, py, cq, sq, yaw_bam}"""
    lib = load_library()
    ps = np.ascontiguousarray(np.asarray(poses, np.float64))
    flat = ps.reshape(-1, 3)
    q = np.empty((flat.shape[0], 5), np.int32)
    for k in range(flat.shape[0]):
        rc = lib.sn_rollout_pose_q(cell_m, origin_x_m, origin_y_m, flat[k].ctypes.data, q[k].ctypes.data)
        if rc:
            raise StereoNetError(rc, "sn_rollout_pose_q")
    return q[0] if ps.ndim == 1 else q


def rollout_velocity(params, s: int):
    """sn_rollout_velocity (host only): (v, w) of sample s"""
    prm, out = rollout_params(params), (C.c_double * 2)()
    rc = load_library().sn_rollout_velocity(C.byref(prm), s, out)
    if rc:
        raise StereoNetError(rc, "sn_rollout_velocity")
    return out[0], out[1]


def error_string(code: int) -> str:
    return load_library().sn_strerror(code).decode()


def _np_ptr(a: Optional[np.ndarray]):
    return a.ctypes.data if a is not None else None


class StereoNetHIP:
    """One GPU's StereoNet engine (sn_handle)."""

    def __init__(self, model_file: str, device: int = -1, max_batch: int = 1, width: int = 0, height: int = 0,
                 dmax: int = 0, precision: int = PREC_DEFAULT, task_num: int = 4, refine_chunk: int = 0,
                 piece: int = 0):
        self._lib = load_library()
        self._h = C.c_void_p()
        cfg = SnConfig(device, max_batch, width, height, dmax, precision, task_num, refine_chunk, piece)
        rc = self._lib.sn_create(model_file.encode(), C.byref(cfg), C.byref(self._h))
        if rc != 0:
            self._h = C.c_void_p()
            detail = self._lib.sn_last_error(None)
            raise StereoNetError(rc, f"sn_create({model_file!r})", detail.decode() if detail else "")
        info = SnIoInfo()
        self._check(self._lib.sn_get_io_info(self._h, C.byref(info)), "sn_get_io_info")
        self.info = info
        self.width, self.height, self.dmax = info.width, info.height, info.dmax
        self.max_batch = info.max_batch
        self.refine_chunk, self.piece, self.tower_streams = info.refine_chunk, info.piece, info.tower_streams
        self.refine_levels = info.refine_levels
        self.precision = info.precision
        self.out_scale = float(info.out_scale)
        self.flops_per_pair = float(info.flops_per_pair)

    # -- plumbing -----------------------------------------------------------------------------
    def _check(self, rc: int, where: str, outputs=None):
        if rc != 0:
            detail = self._lib.sn_last_error(self._h).decode() if self._h else ""
            if rc == SN_ERR_RANGE:
                st = SnRefineStats()
                self._lib.sn_get_refine_stats(self._h, C.byref(st))
                err = StereoNetRangeError(where, detail, [int(v) for v in st.nonfinite_px][:max(1, st.levels)], st.nonfinite_low_px)
                err.outputs = outputs
                raise err
            raise StereoNetError(rc, where, detail)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            rc = self._lib.sn_destroy(self._h)
            if rc:                            # refused (a live TemporalFilter): the handle stays valid, close the filter first
                self._check(rc, "sn_destroy")
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- refinement statistic / SN_PREC_AUTO ----------------------------------------------------
    def refine_stats(self) -> dict:
        """sn_get_refine_stats as a dict (precisions as names): what the refinement moved the last call's maps by, and
        which arithmetic an SN_PREC_AUTO handle is in."""
        st = SnRefineStats()
        self._check(self._lib.sn_get_refine_stats(self._h, C.byref(st)), "sn_get_refine_stats")
        d = {k: getattr(st, k) for k, _ in SnRefineStats._fields_ if k not in ("level_px", "nonfinite_px")}
        d["level_px"] = [float(v) for v in st.level_px][:max(1, st.levels)]
        d["nonfinite_px"] = [int(v) for v in st.nonfinite_px][:max(1, st.levels)]
        for k in ("precision", "precision_selected", "precision_last"):
            d[k] = PREC_NAMES.get(d[k], str(d[k]))
        return d

    @property
    def precision_selected(self) -> int:
        info = SnIoInfo()
        self._check(self._lib.sn_get_io_info(self._h, C.byref(info)), "sn_get_io_info")
        return info.precision_selected

    # -- Run (host numpy buffers) ---------------------------------------------------------------
    def infer(self, in6: np.ndarray, want_disp: bool = True, want_raw: bool = True):
        """in6: int8 (6,H,W) or (n,6,H,W) -> (disp float32, raw int32) with matching leading dims."""
        x = np.ascontiguousarray(in6, dtype=np.int8)
        single = x.ndim == 3
        if single:
            x = x[None]
        n = x.shape[0]
        if x.shape[1:] != (6, self.height, self.width):
            raise StereoNetError(-1, "infer", f"input shape {x.shape} != (n,6,{self.height},{self.width})")
        disp = np.empty((n, self.height, self.width), np.float32) if want_disp else None
        raw = np.empty((n, self.height, self.width), np.int32) if want_raw else None
        out = ((disp[0] if disp is not None else None), (raw[0] if raw is not None else None)) if single else (disp, raw)
        self._check(self._lib.sn_infer_batch(self._h, n, x.ctypes.data, _np_ptr(raw), _np_ptr(disp), SN_MEM_HOST, None),
                    "sn_infer_batch", out)
        return out

    # -- Run (device pointers, e.g. torch tensors' data_ptr(); stream = hipStream_t as int) ------
    def infer_device(self, n: int, in_ptr: int, raw_ptr: int, disp_ptr: int, stream: int = 0):
        self._check(self._lib.sn_infer_batch(self._h, n, in_ptr, raw_ptr or None, disp_ptr or None, SN_MEM_DEVICE,
                                             stream or None), "sn_infer_batch")

    def preprocess_nv12(self, left: np.ndarray, right: np.ndarray, w: int, h: int) -> np.ndarray:
        left = np.ascontiguousarray(left, dtype=np.uint8)
        right = np.ascontiguousarray(right, dtype=np.uint8)
        out = np.empty((6, h, w), np.int8)
        self._check(self._lib.sn_preprocess_nv12(self._h, left.ctypes.data, right.ctypes.data, w, h, out.ctypes.data,
                                                 SN_MEM_HOST, None), "sn_preprocess_nv12")
        return out

    def preprocess_sbs_nv12_device(self, n: int, sbs_ptr: int, out_ptr: int, stream: int = 0):
        """n side-by-side NV12 frames (device, n*3*H*W bytes) -> n int8 model tensors (device), on `stream`."""
        self._check(self._lib.sn_preprocess_sbs_nv12_batch(self._h, n, sbs_ptr, 2 * self.width, self.height, out_ptr,
                                                           SN_MEM_DEVICE, stream or None), "sn_preprocess_sbs_nv12_batch")

    def preprocess_sbs_nv12(self, sbs: np.ndarray) -> np.ndarray:
        """uint8 (n, 3*H*W) side-by-side NV12 frames -> int8 (n, 6, H, W) model tensors (host buffers)."""
        x = np.ascontiguousarray(sbs, dtype=np.uint8).reshape(-1, 3 * self.width * self.height)
        out = np.empty((x.shape[0], 6, self.height, self.width), np.int8)
        self._check(self._lib.sn_preprocess_sbs_nv12_batch(self._h, x.shape[0], x.ctypes.data, 2 * self.width, self.height,
                                                           out.ctypes.data, SN_MEM_HOST, None), "sn_preprocess_sbs_nv12_batch")
        return out

    def infer_sbs_nv12(self, sbs: np.ndarray, want_tensor: bool = False):
        """sbs: uint8 side-by-side NV12 frame (H*3/2 rows of 2W bytes) -> (disp, raw[, tensor])"""
        sbs = np.ascontiguousarray(sbs, dtype=np.uint8)
        disp = np.empty((self.height, self.width), np.float32)
        raw = np.empty((self.height, self.width), np.int32)
        ten = np.empty((6, self.height, self.width), np.int8) if want_tensor else None
        self._check(self._lib.sn_infer_sbs_nv12(self._h, sbs.ctypes.data, 2 * self.width, self.height, raw.ctypes.data,
                                                disp.ctypes.data, _np_ptr(ten), SN_MEM_HOST, None), "sn_infer_sbs_nv12")
        return (disp, raw, ten) if want_tensor else (disp, raw)

    # -- async Run -------------------------------------------------------------------------------
    def submit(self, in6: np.ndarray, raw_out: Optional[np.ndarray], disp_out: Optional[np.ndarray],
               timeout_ms: int = -1) -> int:
        x = np.ascontiguousarray(in6, dtype=np.int8)
        t = C.c_uint64()
        self._check(self._lib.sn_submit(self._h, x.ctypes.data, _np_ptr(raw_out), _np_ptr(disp_out), timeout_ms,
                                        C.byref(t)), "sn_submit")
        return t.value

    def submit_nv12(self, sbs: np.ndarray, raw_out: Optional[np.ndarray], disp_out: Optional[np.ndarray],
                    timeout_ms: int = -1) -> int:
        """async Run on FeedImg's raw side-by-side NV12 frame (uint8, 3*H*W bytes): half the H2D bytes of submit()."""
        x = np.ascontiguousarray(sbs, dtype=np.uint8)
        if x.size != 3 * self.width * self.height:
            raise StereoNetError(-1, "submit_nv12", f"frame has {x.size} bytes, expected {3 * self.width * self.height}")
        t = C.c_uint64()
        self._check(self._lib.sn_submit_nv12(self._h, x.ctypes.data, 2 * self.width, self.height, _np_ptr(raw_out),
                                             _np_ptr(disp_out), timeout_ms, C.byref(t)), "sn_submit_nv12")
        return t.value

    def wait(self, ticket: int) -> float:
        ms = C.c_float()
        self._check(self._lib.sn_wait(self._h, ticket, C.byref(ms)), "sn_wait")
        return ms.value

    # -- int32 / float32 maps of the model's size: what the post-processing calls take and return ------------------------
    def _maps(self, a, where: str, dtype=np.int32) -> np.ndarray:
        r = np.ascontiguousarray(a, dtype=dtype)
        # the calls move n * H * W elements of the MODEL's size: anything else would run past these arrays
        if r.ndim not in (2, 3) or r.shape[-2:] != (self.height, self.width):
            raise StereoNetError(-1, where, f"map shape {r.shape} != ([n,] {self.height}, {self.width})")
        n = self._count(r)
        if n < 1 or n > self.max_batch:
            raise StereoNetError(-1, where, f"{n} maps, the engine was created for 1..{self.max_batch}")
        return r

    @staticmethod
    def _count(r: np.ndarray) -> int:
        return 1 if r.ndim == 2 else r.shape[0]

    @staticmethod
    def _disp_ptr(disp: Optional[np.ndarray], shape, where: str):
        """The optional float map a call rewrites IN PLACE: checked, -> its address (None without one)."""
        if disp is not None and (disp.dtype != np.float32 or disp.shape != shape or not disp.flags.c_contiguous):
            raise StereoNetError(-1, where, "disp must be a C-contiguous float32 array of the maps' shape")
        return _np_ptr(disp)

    def _mask_outputs(self, r: np.ndarray, per_map: int = 1):
        """-> (n, out, mask, counter) for the validated maps r: the map and mask of r's shape, per_map uint32 counters per map."""
        n = self._count(r)
        return n, np.empty_like(r), np.empty(r.shape, np.uint8), np.zeros(n if per_map == 1 else (n, per_map), np.uint32)

    def _guide(self, guide, guide_kind: int, guide_pitch: int, n: int, where: str):
        """The optional luma guide of n maps, checked against the model's size -> (the array to pass or None, the pitch to pass)."""
        if guide is None:
            return None, guide_pitch
        w, h = self.width, self.height
        if guide_kind == SN_GUIDE_TENSOR:
            g = np.ascontiguousarray(guide, dtype=np.int8)
            if g.shape not in ((6, h, w), (n, 6, h, w)) or g.size != n * 6 * h * w:
                raise StereoNetError(-1, where, f"guide shape {g.shape} != ([{n},] 6, {h}, {w})")
            return g, guide_pitch
        g = np.ascontiguousarray(guide, dtype=np.uint8).reshape(-1)
        guide_pitch = guide_pitch or w
        need = (n - 1) * guide_pitch * (h + (h + 1) // 2) + guide_pitch * (h - 1) + w
        if guide_pitch < w or g.size < need:      # the library cannot see how long a host buffer is
            raise StereoNetError(-1, where, f"guide of {g.size} bytes, {n} frames of pitch {guide_pitch} take {need}")
        return g, guide_pitch

    def depth_from_raw(self, raw: np.ndarray, focal_px: float = 527.1931762695312, baseline_mm: float = 119.89382172,
                       want_disp: bool = False):
        """Parse()'s dequantisation + depth (parser.cpp:84-86) on the GPU: int32 (H,W) or (n,H,W) -> depth in metres
        (float32, inf where raw == 0) [, disparity px]; bit-identical to the host Parse."""
        r = self._maps(raw, "depth_from_raw")
        n = self._count(r)
        depth = np.empty(r.shape, np.float32)
        disp = np.empty(r.shape, np.float32) if want_disp else None
        self._check(self._lib.sn_depth_from_raw(self._h, n, r.ctypes.data, focal_px, baseline_mm, depth.ctypes.data,
                                                _np_ptr(disp), SN_MEM_HOST, None), "sn_depth_from_raw")
        return (depth, disp) if want_disp else depth

    def _camera(self, cam) -> "SnCamera":
        from . import pointcloud
        c = (cam or pointcloud.Camera()).resolved(self.width, self.height)
        return SnCamera(c.fx, c.fy, c.cx, c.cy, c.baseline_mm, c.z_min_m, c.z_max_m, c.step)

    def pointcloud(self, raw: np.ndarray, cam=None, layout: int = 0, nv12: Optional[np.ndarray] = None,
                   nv12_pitch: int = 0):
        """sn_pointcloud_from_raw on host buffers: int32 (H,W) or (n,H,W) -> (points float32, counts uint32 (n,)), points
        (n, Ho, Wo, 4) for pointcloud.ORGANISED and (n, Ho*Wo, 4) for pointcloud.COMPACT (map k's first counts[k] rows are
        its points; the rest is unspecified), leading n dropped for a 2-D raw.  cam: pointcloud.Camera (default: the
        reference's intrinsics, principal point at the centre).  nv12: n frames of pointcloud.nv12_frame_bytes(nv12_pitch,
        H) bytes (W for a plain left image, 2W for the side-by-side frame) colour the points."""
        from . import pointcloud
        r = self._maps(raw, "pointcloud")
        n = self._count(r)
        c = self._camera(cam)
        f = None
        if nv12 is not None:
            f = np.ascontiguousarray(nv12, dtype=np.uint8)
            if nv12_pitch < self.width or f.size != n * pointcloud.nv12_frame_bytes(nv12_pitch, self.height):
                raise StereoNetError(-1, "pointcloud", f"nv12 of {f.size} bytes at pitch {nv12_pitch} is not {n} frames of "
                                                       f"{self.width}x{self.height}")
        ho, wo = pointcloud.Camera(step=c.step).out_shape(self.width, self.height)
        shape = (n, ho, wo, 4) if layout == pointcloud.ORGANISED else (n, ho * wo, 4)
        pts = np.empty(int(np.prod(shape)) + 4, np.float32)         # points must be 16-byte aligned
        off = (-pts.ctypes.data % 16) // 4
        pts = pts[off:off + int(np.prod(shape))].reshape(shape)
        counts = np.zeros(n, np.uint32)
        self._check(self._lib.sn_pointcloud_from_raw(self._h, n, r.ctypes.data, _np_ptr(f), nv12_pitch, C.byref(c), layout,
                                                     pts.ctypes.data, counts.ctypes.data, SN_MEM_HOST, None),
                    "sn_pointcloud_from_raw")
        return (pts[0], counts[:1]) if r.ndim == 2 else (pts, counts)

    def pointcloud_device(self, n: int, raw_ptr: int, cam, points_ptr: int, counts_ptr: int, nv12_ptr: int = 0,
                          nv12_pitch: int = 0, layout: int = 0, stream: int = 0):
        """sn_pointcloud_from_raw on device pointers (e.g. torch tensors' data_ptr()); stream = hipStream_t as int
        (0: the point cloud's own stream, and the call returns after completion)."""
        c = self._camera(cam)
        self._check(self._lib.sn_pointcloud_from_raw(self._h, n, raw_ptr, nv12_ptr or None, nv12_pitch, C.byref(c), layout,
                                                     points_ptr, counts_ptr or None, SN_MEM_DEVICE, stream or None),
                    "sn_pointcloud_from_raw")

    # -- obstacle grid and laser scan ------------------------------------------------------------------
    def obstacles(self, raw: np.ndarray, cam, params, grid: bool = True, scan: bool = True, mounts=None):
        """sn_obstacles_from_raw on host buffers: int32 (H,W) or (n,H,W) -> (occ int8 (n, gh, gw), hits uint32 (n, gh, gw, 2),
        height_mm int32 (n, gh, gw), ranges float32 (n, beams), stats uint32 (n, 4)), leading n dropped for a 2-D raw;
        obstacles.reference is the numpy twin.  cam: pointcloud.Camera (None: as pointcloud()); params:
        obstacles.ObstacleParams.  Without a grid (gw = gh = 0, or grid=False) the grid outputs are empty, without a scan
        (beams = 0, or scan=False) ranges is.  mounts: float32 (n, 12), one base_from_cam per map (sn_obstacles_from_raw_mounts:
        params.base_from_cam is then ignored), e.g. ground()'s records' base_from_cam."""
        r = self._maps(raw, "obstacles")
        n = self._count(r)
        c, prm = self._camera(cam), obstacle_params(params)
        gw, gh = (max(prm.gw, 0), max(prm.gh, 0)) if grid else (0, 0)
        beams = max(prm.beams, 0) if scan else 0
        occ, hits = np.empty((n, gh, gw), np.int8), np.empty((n, gh, gw, 2), np.uint32)
        height, ranges, stats = np.empty((n, gh, gw), np.int32), np.empty((n, beams), np.float32), np.zeros((n, 4), np.uint32)
        g = gw * gh > 0
        outs = (_np_ptr(occ if g else None), _np_ptr(hits if g else None), _np_ptr(height if g else None),
                _np_ptr(ranges if beams else None), _np_ptr(stats if g else None), SN_MEM_HOST, None)
        if mounts is None:
            self._check(self._lib.sn_obstacles_from_raw(self._h, n, r.ctypes.data, C.byref(c), C.byref(prm), *outs), "sn_obstacles_from_raw")
        else:
            m = np.ascontiguousarray(mounts, np.float32)
            if m.size != n * 12:
                raise StereoNetError(-1, "obstacles", f"mounts of shape {m.shape} for {n} maps: (n, 12) is needed")
            self._check(self._lib.sn_obstacles_from_raw_mounts(self._h, n, r.ctypes.data, C.byref(c), C.byref(prm), m.ctypes.data, 12, *outs),
                        "sn_obstacles_from_raw_mounts")
        out = (occ, hits, height, ranges, stats)
        return tuple(a[0] for a in out) if r.ndim == 2 else out

    beam_edges = staticmethod(beam_edges)      # sn_obstacle_beam_edges needs no engine; here beside the calls that use its table

    def obstacles_device(self, n: int, raw_ptr: int, cam, params, occ_ptr: int = 0, hits_ptr: int = 0, height_ptr: int = 0,
                         ranges_ptr: int = 0, stats_ptr: int = 0, stream: int = 0, mounts_ptr: int = 0, mount_stride: int = 12):
        """sn_obstacles_from_raw on device pointers (0: that output is not wanted); stream = hipStream_t as int (0: the stage's
        own stream, and the call returns after completion).  mounts_ptr: sn_obstacles_from_raw_mounts, map k's mount at
        mounts_ptr + 4 * k * mount_stride (ground_device's records: their address + 64, ground.RECORD_FLOATS)."""
        c, prm = self._camera(cam), obstacle_params(params)
        if mounts_ptr:
            self._check(self._lib.sn_obstacles_from_raw_mounts(self._h, n, raw_ptr, C.byref(c), C.byref(prm), mounts_ptr, mount_stride,
                                                               occ_ptr or None, hits_ptr or None, height_ptr or None, ranges_ptr or None,
                                                               stats_ptr or None, SN_MEM_DEVICE, stream or None),
                        "sn_obstacles_from_raw_mounts")
            return
        self._check(self._lib.sn_obstacles_from_raw(self._h, n, raw_ptr, C.byref(c), C.byref(prm), occ_ptr or None, hits_ptr or None,
                                                    height_ptr or None, ranges_ptr or None, stats_ptr or None, SN_MEM_DEVICE,
                                                    stream or None), "sn_obstacles_from_raw")

    # -- inflation by the robot's radius ------------------------------------------------------------------
    def inflate(self, occ: np.ndarray, params, want=(True, True, True, True)):
        """sn_inflate_grid on host buffers: occ int8 (gh, gw) or (n, gh, gw), as obstacles() or Costmap.push() give it ->
        (cost uint8, grid int8, dist2 uint16 (each (n, gh, gw)), stats uint32 (n, 5)), None where `want` says an output is not
        asked for, leading n dropped for a 2-D occ; inflate.reference is the numpy twin.  params: inflate.InflateParams."""
        o = np.ascontiguousarray(occ, np.int8)
        if o.ndim not in (2, 3):
            raise StereoNetError(-1, "inflate", f"occ of shape {o.shape}: (gh, gw) or (n, gh, gw) is needed")
        n, (gh, gw) = (1 if o.ndim == 2 else o.shape[0]), o.shape[-2:]
        prm = inflate_params(params)
        shapes = ((n, gh, gw), (n, gh, gw), (n, gh, gw), (n, 5))
        outs = [np.zeros(s, d) if w else None for s, d, w in zip(shapes, (np.uint8, np.int8, np.uint16, np.uint32), want)]
        self._check(self._lib.sn_inflate_grid(self._h, n, o.ctypes.data, gw, gh, C.byref(prm), *[_np_ptr(a) for a in outs], SN_MEM_HOST, None),
                    "sn_inflate_grid")
        return tuple(a if a is None or o.ndim == 3 else a[0] for a in outs)

    def inflate_device(self, n: int, occ_ptr: int, gw: int, gh: int, params, cost_ptr: int = 0, grid_ptr: int = 0, dist2_ptr: int = 0,
                       stats_ptr: int = 0, stream: int = 0):
        """sn_inflate_grid on device pointers (0: that output is not wanted); stream = hipStream_t as int (0: the stage's own
        stream, and the call returns after completion)."""
        prm = inflate_params(params)
        self._check(self._lib.sn_inflate_grid(self._h, n, occ_ptr or None, gw, gh, C.byref(prm), cost_ptr or None, grid_ptr or None,
                                              dist2_ptr or None, stats_ptr or None, SN_MEM_DEVICE, stream or None), "sn_inflate_grid")

    # -- navigation function and path ---------------------------------------------------------------------
    def navfn(self, cost: np.ndarray, goals, starts, params, want=(True, True, True)):
        """sn_navfn on host buffers: cost uint8 (gh, gw) or (n, gh, gw) as inflate() gives it, goals (n, 2) and starts (n, 2) or
        None as {x, y} in cells -> (potential uint32 (n, gh, gw), path int32 (n, max_path, 2) with -1 past the path's length,
        stats uint32 (n, 5), rounds: how many rounds did work), None where `want` says an output is not asked for, leading n
        dropped for a 2-D cost; navfn.reference is the twin.  params: navfn.NavParams."""
        c = np.ascontiguousarray(cost, np.uint8)
        if c.ndim not in (2, 3):
            raise StereoNetError(-1, "navfn", f"cost of shape {c.shape}: (gh, gw) or (n, gh, gw) is needed")
        n, (gh, gw) = (1 if c.ndim == 2 else c.shape[0]), c.shape[-2:]
        prm = nav_params(params)
        g = np.ascontiguousarray(np.asarray(goals, np.int32).reshape(n, 2))
        s = None if starts is None else np.ascontiguousarray(np.asarray(starts, np.int32).reshape(n, 2))
        outs = [np.zeros((n, gh, gw), np.uint32) if want[0] else None, np.full((n, prm.max_path, 2), -1, np.int32) if want[1] else None,
                np.zeros((n, 5), np.uint32) if want[2] else None]
        rounds = C.c_int(0)
        self._check(self._lib.sn_navfn(self._h, n, c.ctypes.data, gw, gh, g.ctypes.data, _np_ptr(s), C.byref(prm), *[_np_ptr(a) for a in outs],
                                       C.byref(rounds), SN_MEM_HOST, None), "sn_navfn")
        return tuple(a if a is None or c.ndim == 3 else a[0] for a in outs) + (rounds.value,)

    def navfn_device(self, n: int, cost_ptr: int, gw: int, gh: int, goals_ptr: int, starts_ptr: int, params, potential_ptr: int = 0,
                     path_ptr: int = 0, stats_ptr: int = 0, stream: int = 0) -> int:
        """sn_navfn on device pointers (0: that buffer is not given); stream = hipStream_t as int (0: the stage's own stream).
        -> how many rounds did work, or -1 where the call only enqueued (max_rounds > 0 on a caller stream)."""
        prm, rounds = nav_params(params), C.c_int(0)
        self._check(self._lib.sn_navfn(self._h, n, cost_ptr or None, gw, gh, goals_ptr or None, starts_ptr or None, C.byref(prm),
                                       potential_ptr or None, path_ptr or None, stats_ptr or None, C.byref(rounds), SN_MEM_DEVICE,
                                       stream or None), "sn_navfn")
        return rounds.value

    # -- trajectory rollout -------------------------------------------------------------------------------
    def rollout(self, cost: np.ndarray, potential: np.ndarray, poses_q, params, footprint=None, window=None, want=(True, True, True)):
        """sn_rollout on host buffers: cost uint8 and potential uint32, (gh, gw) or (n, gh, gw) as inflate() and navfn() give them,
        poses_q (n, 5) as rollout_pose_q gives it, window (n, 4) or None -> (samples uint32 (n, S, 2), best uint32 (n, 8), traj
        int32 (n, T+1, 3), zeros where a map has no valid sample), None where `want` says an output is not asked for, leading n
        dropped for a 2-D cost; rollout.reference is the twin.  params: rollout.RolloutParams."""
        c = np.ascontiguousarray(cost, np.uint8)
        if c.ndim not in (2, 3):
            raise StereoNetError(-1, "rollout", f"cost of shape {c.shape}: (gh, gw) or (n, gh, gw) is needed")
        n, (gh, gw) = (1 if c.ndim == 2 else c.shape[0]), c.shape[-2:]
        pot = np.ascontiguousarray(potential, np.uint32)
        if pot.shape != c.shape:
            raise StereoNetError(-1, "rollout", f"potential of shape {pot.shape} over a cost of shape {c.shape}")
        prm, fp = rollout_params(params), _footprint(params, footprint)
        q = np.ascontiguousarray(np.asarray(poses_q, np.int32).reshape(n, 5))
        win = None if window is None else np.ascontiguousarray(np.asarray(window, np.int32).reshape(n, 4))
        S, T1 = max(prm.nv * prm.nw, 0), max(prm.steps + 1, 0)
        outs = [np.zeros((n, S, 2), np.uint32) if want[0] else None, np.zeros((n, 8), np.uint32) if want[1] else None,
                np.zeros((n, T1, 3), np.int32) if want[2] else None]
        self._check(self._lib.sn_rollout(self._h, n, c.ctypes.data, pot.ctypes.data, gw, gh, q.ctypes.data, _np_ptr(win), C.byref(prm),
                                         fp.ctypes.data, fp.shape[0], *[_np_ptr(a) for a in outs], SN_MEM_HOST, None), "sn_rollout")
        return tuple(a if a is None or c.ndim == 3 else a[0] for a in outs)

    def rollout_device(self, n: int, cost_ptr: int, potential_ptr: int, gw: int, gh: int, poses_ptr: int, params, footprint=None,
                       window_ptr: int = 0, samples_ptr: int = 0, best_ptr: int = 0, traj_ptr: int = 0, stream: int = 0) -> None:
        """sn_rollout on device pointers (0: that buffer is not given; the footprint is host memory); stream = hipStream_t as int
        (0: the stage's own stream, and the call returns after completion)."""
        prm, fp = rollout_params(params), _footprint(params, footprint)
        self._check(self._lib.sn_rollout(self._h, n, cost_ptr or None, potential_ptr or None, gw, gh, poses_ptr or None, window_ptr or None,
                                         C.byref(prm), fp.ctypes.data, fp.shape[0], samples_ptr or None, best_ptr or None, traj_ptr or None,
                                         SN_MEM_DEVICE, stream or None), "sn_rollout")

    # -- ground plane -----------------------------------------------------------------------------------
    def ground(self, raw: np.ndarray, cam, params, labels: bool = True):
        """sn_ground_from_raw on host buffers: int32 (H,W) or (n,H,W) -> (records ground.RECORD (n,), labels uint8 (n, H, W) or
        None), leading n dropped for a 2-D raw; ground.reference is the numpy twin.  cam: pointcloud.Camera (None: as
        pointcloud()); params: ground.GroundParams.  ground.angles(rec["base_from_cam"]) gives pitch and roll."""
        from . import ground as gr
        r = self._maps(raw, "ground")
        n = self._count(r)
        c, prm = self._camera(cam), ground_params(params)
        rec = np.zeros(n, gr.RECORD)
        lab = np.empty((n, self.height, self.width), np.uint8) if labels else None
        self._check(self._lib.sn_ground_from_raw(self._h, n, r.ctypes.data, C.byref(c), C.byref(prm), rec.ctypes.data, _np_ptr(lab),
                                                 SN_MEM_HOST, None), "sn_ground_from_raw")
        return (rec[0], lab[0] if labels else None) if r.ndim == 2 else (rec, lab)

    def ground_gate(self, cam, params) -> np.ndarray:
        """sn_ground_gate for this engine's map size (needs no device)"""
        from . import pointcloud
        return ground_gate(cam or pointcloud.Camera(), params, self.width, self.height)

    def ground_device(self, n: int, raw_ptr: int, cam, params, ground_ptr: int = 0, labels_ptr: int = 0, stream: int = 0):
        """sn_ground_from_raw on device pointers (0: that output is not wanted); stream = hipStream_t as int (0: the stage's own
        stream, and the call returns after completion)."""
        c, prm = self._camera(cam), ground_params(params)
        self._check(self._lib.sn_ground_from_raw(self._h, n, raw_ptr, C.byref(c), C.byref(prm), ground_ptr or None, labels_ptr or None,
                                                 SN_MEM_DEVICE, stream or None), "sn_ground_from_raw")

    # -- left-right consistency check -----------------------------------------------------------------
    def mirror_pair(self, in6: np.ndarray) -> np.ndarray:
        """sn_mirror_pair_i8 on host buffers: int8 (6,H,W) or (n,6,H,W) -> the pair with the eyes swapped and every row
        reversed (lrcheck.mirror_pair is the numpy twin)."""
        x = np.ascontiguousarray(in6, dtype=np.int8)
        if x.ndim not in (3, 4) or x.shape[-3:] != (6, self.height, self.width):
            raise StereoNetError(-1, "mirror_pair", f"input shape {x.shape} != ([n,] 6, {self.height}, {self.width})")
        n = 1 if x.ndim == 3 else x.shape[0]
        out = np.empty_like(x)
        self._check(self._lib.sn_mirror_pair_i8(self._h, n, x.ctypes.data, out.ctypes.data, SN_MEM_HOST, None),
                    "sn_mirror_pair_i8")
        return out

    def mirror_pair_device(self, n: int, in_ptr: int, out_ptr: int, stream: int = 0):
        self._check(self._lib.sn_mirror_pair_i8(self._h, n, in_ptr, out_ptr, SN_MEM_DEVICE, stream or None),
                    "sn_mirror_pair_i8")

    def lr_check(self, raw_left: np.ndarray, raw_right: np.ndarray, tau_px: float = 1.0, tau_rel: float = 0.0,
                 mirrored: bool = False, disp: Optional[np.ndarray] = None):
        """sn_lr_check on host buffers: int32 (H,W) or (n,H,W) maps -> (out_raw int32, mask uint8, kept uint32 (n,)); `disp`
        (float32, same shape) gets 0.0 written IN PLACE at the rejected pixels.  mirrored: raw_right is stored
        column-reversed, as the network wrote the map of the mirrored pair.  lrcheck.reference is the numpy twin."""
        l = self._maps(raw_left, "lr_check")
        r = self._maps(raw_right, "lr_check")
        if l.shape != r.shape:
            raise StereoNetError(-1, "lr_check", f"maps of shape {l.shape} and {r.shape}")
        dp = self._disp_ptr(disp, l.shape, "lr_check")
        n, out, mask, kept = self._mask_outputs(l)
        p = SnLrcParams(tau_px, tau_rel, int(bool(mirrored)))
        self._check(self._lib.sn_lr_check(self._h, n, l.ctypes.data, r.ctypes.data, C.byref(p), out.ctypes.data,
                                          dp, mask.ctypes.data, kept.ctypes.data, SN_MEM_HOST, None), "sn_lr_check")
        return out, mask, kept

    def lr_check_device(self, n: int, left_ptr: int, right_ptr: int, tau_px: float, tau_rel: float, mirrored: bool,
                        out_raw_ptr: int = 0, disp_ptr: int = 0, mask_ptr: int = 0, kept_ptr: int = 0, stream: int = 0):
        """sn_lr_check on device pointers (out_raw_ptr may equal left_ptr); stream = hipStream_t as int."""
        p = SnLrcParams(tau_px, tau_rel, int(bool(mirrored)))
        self._check(self._lib.sn_lr_check(self._h, n, left_ptr, right_ptr, C.byref(p), out_raw_ptr or None, disp_ptr or None,
                                          mask_ptr or None, kept_ptr or None, SN_MEM_DEVICE, stream or None), "sn_lr_check")

    def _pair_input(self, x, where: str):
        """-> (contiguous array, in_kind, n, single) of an int8 model tensor or uint8 side-by-side NV12 frames (what infer_lrc and infer_conf take)"""
        a = np.asarray(x)
        frame = 3 * self.width * self.height
        if a.dtype == np.uint8:
            single = a.ndim == 1 or a.size == frame
            a = np.ascontiguousarray(a).reshape(-1)
            if a.size == 0 or a.size % frame:
                raise StereoNetError(-1, where, f"{a.size} bytes are not side-by-side NV12 frames of {frame} bytes")
            return a, SN_LRC_IN_SBS_NV12, a.size // frame, single
        a = np.ascontiguousarray(a, dtype=np.int8)
        single = a.ndim == 3
        if a.ndim not in (3, 4) or a.shape[-3:] != (6, self.height, self.width):
            raise StereoNetError(-1, where, f"input shape {a.shape} != ([n,] 6, {self.height}, {self.width})")
        return a, SN_LRC_IN_TENSOR, (1 if single else a.shape[0]), single

    def infer_lrc(self, x: np.ndarray, tau_px: float = 1.0, tau_rel: float = 0.0, want_right: bool = False):
        """sn_infer_lrc on host buffers.  x: the int8 model tensor (6,H,W) / (n,6,H,W), or uint8 side-by-side NV12 frames
        (3*H*W bytes each: flat, or (n, 3*H*W)).  -> (disp float32, raw int32, mask uint8, kept uint32 (n,)[, right_raw
        int32]): the left map with rejected pixels at 0, the reason per pixel, kept pixels per map and, with want_right, the
        right eye's own map in right-image coordinates (unmasked).  The leading n is dropped for a single tensor / frame."""
        a, kind, n, single = self._pair_input(x, "infer_lrc")
        shape = (n, self.height, self.width)
        disp, raw = np.empty(shape, np.float32), np.empty(shape, np.int32)
        mask, kept = np.empty(shape, np.uint8), np.zeros(n, np.uint32)
        right = np.empty(shape, np.int32) if want_right else None
        p = SnLrcParams(tau_px, tau_rel, 1)
        self._check(self._lib.sn_infer_lrc(self._h, n, a.ctypes.data, kind, 2 * self.width, self.height, C.byref(p),
                                           raw.ctypes.data, disp.ctypes.data, _np_ptr(right), mask.ctypes.data,
                                           kept.ctypes.data, SN_MEM_HOST, None), "sn_infer_lrc")
        out = [disp, raw, mask] if not single else [disp[0], raw[0], mask[0]]
        out.append(kept)
        if want_right:
            out.append(right[0] if single else right)
        return tuple(out)

    def infer_lrc_device(self, n: int, in_ptr: int, tau_px: float, tau_rel: float, raw_ptr: int = 0, disp_ptr: int = 0,
                         right_ptr: int = 0, mask_ptr: int = 0, kept_ptr: int = 0, in_kind: int = SN_LRC_IN_TENSOR,
                         stream: int = 0):
        """sn_infer_lrc on device pointers (e.g. torch tensors' data_ptr()); stream = hipStream_t as int (0: the engine's own
        stream, and the call returns after completion)."""
        p = SnLrcParams(tau_px, tau_rel, 1)
        self._check(self._lib.sn_infer_lrc(self._h, n, in_ptr, in_kind, 2 * self.width, self.height, C.byref(p),
                                           raw_ptr or None, disp_ptr or None, right_ptr or None, mask_ptr or None,
                                           kept_ptr or None, SN_MEM_DEVICE, stream or None), "sn_infer_lrc")

    # -- confidence of the soft-argmin distribution and the mask on it ---------------------------------------------
    def infer_conf(self, x: np.ndarray, min_conf: Optional[float] = None):
        """sn_infer_conf on host buffers: ONE forward pass.  x as for infer_lrc (int8 model tensor (6,H,W) / (n,6,H,W), or uint8
        side-by-side NV12 frames).  min_conf None: no masking -> (disp float32, raw int32, conf float32), the plain map of
        infer plus the confidence.  Otherwise -> (disp, raw, conf, mask uint8, kept uint32 (n,)): pixels with
        conf < min_conf (or raw <= 0) at 0, the reason per pixel, kept pixels per map.  The leading n is dropped for a
        single tensor / frame.  confidence.low / upsample / mask are the numpy twin."""
        a, kind, n, single = self._pair_input(x, "infer_conf")
        shape = (n, self.height, self.width)
        disp, raw, conf = np.empty(shape, np.float32), np.empty(shape, np.int32), np.empty(shape, np.float32)
        masking = min_conf is not None
        mask = np.empty(shape, np.uint8) if masking else None
        kept = np.zeros(n, np.uint32) if masking else None
        p = SnConfParams(min_conf) if masking else None
        self._check(self._lib.sn_infer_conf(self._h, n, a.ctypes.data, kind, 2 * self.width, self.height,
                                            C.byref(p) if masking else None, raw.ctypes.data, disp.ctypes.data, conf.ctypes.data,
                                            _np_ptr(mask), _np_ptr(kept), SN_MEM_HOST, None), "sn_infer_conf")
        out = [disp, raw, conf] + ([mask] if masking else [])
        if single:
            out = [o[0] for o in out]
        if masking:
            out.append(kept)
        return tuple(out)

    def infer_conf_device(self, n: int, in_ptr: int, min_conf: Optional[float] = None, raw_ptr: int = 0, disp_ptr: int = 0,
                          conf_ptr: int = 0, mask_ptr: int = 0, kept_ptr: int = 0, in_kind: int = SN_LRC_IN_TENSOR,
                          stream: int = 0):
        """sn_infer_conf on device pointers (e.g. torch tensors' data_ptr()); min_conf None: no masking (mask_ptr / kept_ptr
        must be 0); stream = hipStream_t as int (0: the engine's own stream, and the call returns after completion)."""
        p = SnConfParams(min_conf) if min_conf is not None else None
        self._check(self._lib.sn_infer_conf(self._h, n, in_ptr, in_kind, 2 * self.width, self.height,
                                            C.byref(p) if p is not None else None, raw_ptr or None, disp_ptr or None,
                                            conf_ptr or None, mask_ptr or None, kept_ptr or None, SN_MEM_DEVICE, stream or None),
                    "sn_infer_conf")

    def conf_mask(self, raw: np.ndarray, conf: np.ndarray, min_conf: float, disp: Optional[np.ndarray] = None):
        """sn_conf_mask on host buffers: int32 raw and float32 conf, (H,W) or (n,H,W) -> (out_raw int32, mask uint8, kept uint32
        (n,)); `disp` (float32, same shape) gets 0.0 written IN PLACE at the rejected pixels.  confidence.mask is the twin."""
        r = self._maps(raw, "conf_mask")
        c = self._maps(conf, "conf_mask", np.float32)
        if r.shape != c.shape:
            raise StereoNetError(-1, "conf_mask", f"maps of shape {r.shape} and {c.shape}")
        dp = self._disp_ptr(disp, r.shape, "conf_mask")
        n, out, mask, kept = self._mask_outputs(r)
        p = SnConfParams(min_conf)
        self._check(self._lib.sn_conf_mask(self._h, n, r.ctypes.data, c.ctypes.data, C.byref(p), out.ctypes.data, dp,
                                           mask.ctypes.data, kept.ctypes.data, SN_MEM_HOST, None), "sn_conf_mask")
        return out, mask, kept

    def conf_mask_device(self, n: int, raw_ptr: int, conf_ptr: int, min_conf: float, out_raw_ptr: int = 0, disp_ptr: int = 0,
                         mask_ptr: int = 0, kept_ptr: int = 0, stream: int = 0):
        """sn_conf_mask on device pointers (out_raw_ptr may equal raw_ptr); stream = hipStream_t as int."""
        p = SnConfParams(min_conf)
        self._check(self._lib.sn_conf_mask(self._h, n, raw_ptr or None, conf_ptr or None, C.byref(p), out_raw_ptr or None,
                                           disp_ptr or None, mask_ptr or None, kept_ptr or None, SN_MEM_DEVICE, stream or None),
                    "sn_conf_mask")

    # -- speckle removal and hole filling ---------------------------------------------------------------
    def filter_raw(self, raw: np.ndarray, speckle_max_px: int = 0, speckle_diff_px: float = 1.0, fill_max_px: int = 0,
                   disp: Optional[np.ndarray] = None):
        """sn_filter_raw on host buffers: int32 (H,W) or (n,H,W) -> (out int32, mask uint8, counts uint32 (n,3) = {valid,
        removed, filled} per map); `disp` (float32, same shape) is rewritten IN PLACE where the mask is not 0 (0.0 at pixels
        that end invalid, the dequantised value at filled ones).  dispfilter.reference is the numpy twin."""
        r = self._maps(raw, "filter_raw")
        dp = self._disp_ptr(disp, r.shape, "filter_raw")
        n, out, mask, counts = self._mask_outputs(r, 3)
        p = SnFilterParams(int(speckle_max_px), speckle_diff_px, int(fill_max_px))
        self._check(self._lib.sn_filter_raw(self._h, n, r.ctypes.data, C.byref(p), out.ctypes.data, dp,
                                            mask.ctypes.data, counts.ctypes.data, SN_MEM_HOST, None), "sn_filter_raw")
        return out, mask, counts

    def filter_raw_device(self, n: int, raw_ptr: int, speckle_max_px: int, speckle_diff_px: float, fill_max_px: int,
                          out_raw_ptr: int = 0, mask_ptr: int = 0, disp_ptr: int = 0, counts_ptr: int = 0, stream: int = 0):
        """sn_filter_raw on device pointers (out_raw_ptr may equal raw_ptr); stream = hipStream_t as int (0: the filter's own
        stream, and the call returns after completion)."""
        p = SnFilterParams(int(speckle_max_px), speckle_diff_px, int(fill_max_px))
        self._check(self._lib.sn_filter_raw(self._h, n, raw_ptr or None, C.byref(p), out_raw_ptr or None, disp_ptr or None,
                                            mask_ptr or None, counts_ptr or None, SN_MEM_DEVICE, stream or None),
                    "sn_filter_raw")

    # -- guided weighted-median smoothing ------------------------------------------------------------------
    def smooth_raw(self, raw: np.ndarray, guide: Optional[np.ndarray] = None, guide_kind: int = SN_GUIDE_NV12,
                   guide_pitch: int = 0, radius: int = 2, sigma_luma: int = 12, min_valid: int = 0,
                   disp: Optional[np.ndarray] = None):
        """sn_smooth_raw on host buffers: int32 (H,W) or (n,H,W) -> (out int32, mask uint8, counts uint32 (n,3) = {valid,
        smoothed measurements, filled pixels} per map).  guide: the left image's luma, either uint8 NV12 frames (guide_kind
        SN_GUIDE_NV12; guide_pitch = the luma pitch, 0 = the width, 2 * width for side-by-side frames; the luma rows alone
        are enough for one map) or the int8 model input ([n,] 6, H, W) (SN_GUIDE_TENSOR); None only with sigma_luma = 0.
        `disp` (float32, the maps' shape) is rewritten IN PLACE where the mask has SN_SMOOTH_CHANGED.  smooth.reference is the
        numpy twin."""
        r = self._maps(raw, "smooth_raw")
        dp = self._disp_ptr(disp, r.shape, "smooth_raw")
        n, out, mask, counts = self._mask_outputs(r, 3)
        g, guide_pitch = self._guide(guide, guide_kind, guide_pitch, n, "smooth_raw")
        p = SnSmoothParams(int(radius), int(sigma_luma), int(min_valid))
        self._check(self._lib.sn_smooth_raw(self._h, n, r.ctypes.data, _np_ptr(g), guide_kind, guide_pitch, C.byref(p),
                                            out.ctypes.data, dp, mask.ctypes.data, counts.ctypes.data, SN_MEM_HOST, None),
                    "sn_smooth_raw")
        return out, mask, counts

    def smooth_raw_device(self, n: int, raw_ptr: int, guide_ptr: int, guide_kind: int, guide_pitch: int, radius: int,
                          sigma_luma: int, min_valid: int, out_raw_ptr: int = 0, mask_ptr: int = 0, disp_ptr: int = 0,
                          counts_ptr: int = 0, stream: int = 0):
        """sn_smooth_raw on device pointers (out_raw_ptr may equal raw_ptr); stream = hipStream_t as int (0: the smoother's own
        stream, and the call returns after completion)."""
        p = SnSmoothParams(int(radius), int(sigma_luma), int(min_valid))
        self._check(self._lib.sn_smooth_raw(self._h, n, raw_ptr or None, guide_ptr or None, guide_kind, guide_pitch, C.byref(p),
                                            out_raw_ptr or None, disp_ptr or None, mask_ptr or None, counts_ptr or None,
                                            SN_MEM_DEVICE, stream or None), "sn_smooth_raw")

    # -- temporal filter of disparity streams ----------------------------------------------------------------
    def temporal_filter(self, streams: int = 1, alpha: int = 64, delta_px: float = 0.5, persist: int = 2,
                        luma_delta: int = 0) -> "TemporalFilter":
        """A TemporalFilter (sn_temporal) of `streams` independent states on this engine; close it before the engine."""
        return TemporalFilter(self, streams, alpha, delta_px, persist, luma_delta)

    def costmap(self, obstacle, params, streams: int = 1) -> "Costmap":
        """A Costmap (sn_costmap) of `streams` rolling log-odds maps on this engine, fed by obstacles() under `obstacle`
        (obstacles.ObstacleParams); params: costmap.CostmapParams.  Close it before the engine."""
        return Costmap(self, obstacle, params, streams)

    def elevation(self, params, streams: int = 1) -> "Elevation":
        """An Elevation (sn_elevation) of `streams` rolling elevation maps on this engine, fed by the engine's int32 maps;
        params: elevation.ElevationParams.  Close it before the engine."""
        return Elevation(self, params, streams)

    def rectifier(self, calib):
        """A Rectifier (sn_rectify) for this engine's model size from a rectify.Calib; close it before the engine."""
        return Rectifier(self, calib)

    def jpeg_encode_nv12(self, nv12: np.ndarray, w: int, h: int, pitch: int = 0, n: int = 1, frame: int = 0, quality: int = 95,
                         rows_per_slice: int = 1, out_stride: int = 0, raw: bool = False):
        """sn_jpeg_encode_nv12 on a host buffer that starts at image 0 (jpeg.encode_nv12 is the numpy twin): n NV12 images of
        w x h at luma pitch `pitch` (0: w), image k at byte k * frame (0: pitch * h * 3/2).  out_stride 0: sn_jpeg_bound(w, h).
        -> list of n bytes objects, None where a stream did not fit out_stride; raw: (uint8 (n, out_stride), uint32 (n,))."""
        src = np.ascontiguousarray(nv12, np.uint8).reshape(-1)
        pitch = pitch or w
        frame = frame or pitch * (h + h // 2)
        span = (n - 1) * frame + (h + h // 2 - 1) * pitch + w
        if n < 1 or src.size < span:
            raise StereoNetError(-1, "jpeg_encode_nv12", f"{n} images of {w}x{h} at pitch {pitch} take {span} bytes, the buffer has {src.size}")
        out_stride = out_stride or jpeg_bound(w, h)
        out = np.empty((n, out_stride), np.uint8)
        sizes = np.zeros(n, np.uint32)
        prm = SnJpegParams(quality, rows_per_slice)
        self._check(self._lib.sn_jpeg_encode_nv12(self._h, n, src.ctypes.data, w, h, pitch, frame, C.byref(prm), out.ctypes.data,
                                                  out_stride, sizes.ctypes.data, SN_MEM_HOST, None), "sn_jpeg_encode_nv12")
        if raw:
            return out, sizes
        return [out[k, :sizes[k]].tobytes() if sizes[k] else None for k in range(n)]

    def jpeg_encode_nv12_device(self, n: int, nv12_ptr: int, w: int, h: int, pitch: int, frame: int, quality: int,
                                rows_per_slice: int, out_ptr: int, out_stride: int, sizes_ptr: int, stream: int = 0):
        """sn_jpeg_encode_nv12 on device pointers; stream = hipStream_t as int (0: the encoder's own stream, and the call returns
        after completion)."""
        prm = SnJpegParams(quality, rows_per_slice)
        self._check(self._lib.sn_jpeg_encode_nv12(self._h, n, nv12_ptr or None, w, h, pitch, frame, C.byref(prm), out_ptr or None,
                                                  out_stride, sizes_ptr or None, SN_MEM_DEVICE, stream or None), "sn_jpeg_encode_nv12")

    # -- the depth view: colour-mapped depth under the left eye ------------------------------------------------
    def _render_inputs(self, raw, left_nv12, left_pitch: int, prm: "SnRenderParams", where: str):
        r = self._maps(raw, where) if np.asarray(raw).dtype != np.uint32 else self._maps(np.asarray(raw).view(np.int32), where)
        n = self._count(r)
        left = None
        if prm.layout == 0:
            left_pitch = left_pitch or self.width
            rows = self.height + (self.height + 1) // 2
            need = (n - 1) * left_pitch * rows + (rows - 1) * left_pitch + ((self.width + 1) & ~1)
            left = np.ascontiguousarray(left_nv12, np.uint8).reshape(-1) if left_nv12 is not None else None
            if left is None or left_pitch < self.width or left.size < need:
                raise StereoNetError(-1, where, f"{n} left eyes of {self.width}x{self.height} at pitch {left_pitch} take {need} bytes")
        return r, n, left, left_pitch

    def render(self, raw: np.ndarray, left_nv12: Optional[np.ndarray] = None, left_pitch: int = 0, params=None, fmt: int = 0):
        """sn_render on host buffers (render.canvas is the numpy twin): int32 (H,W) or (n,H,W) and, for the stacked layout, n
        left eyes as NV12 at luma pitch left_pitch (0: W; 2W: the side-by-side frames in place) -> uint8 (n, Hc, W, 3) for
        render.RGB8, (n, Hc * 3 / 2, W) for render.NV12; leading n dropped for a 2-D raw."""
        prm = render_params(params)
        r, n, left, left_pitch = self._render_inputs(raw, left_nv12, left_pitch, prm, "render")
        hc = self.height * (2 if prm.layout == 0 else 1)
        shape = (n, hc + hc // 2, self.width) if fmt == 1 else (n, hc, self.width, 3)
        out = np.empty(shape, np.uint8)
        pitch = self.width * (1 if fmt == 1 else 3)
        self._check(self._lib.sn_render(self._h, n, r.ctypes.data, _np_ptr(left), left_pitch, C.byref(prm), fmt, out.ctypes.data,
                                        pitch, shape[1] * pitch, SN_MEM_HOST, None), "sn_render")
        return out[0] if r.ndim == 2 else out

    def render_device(self, n: int, raw_ptr: int, left_ptr: int, left_pitch: int, params, fmt: int, out_ptr: int, out_pitch: int,
                      out_frame: int, stream: int = 0):
        """sn_render on device pointers; stream = hipStream_t as int (0: the stage's own stream, and the call returns after
        completion)."""
        prm = render_params(params)
        self._check(self._lib.sn_render(self._h, n, raw_ptr or None, left_ptr or None, left_pitch, C.byref(prm), fmt, out_ptr or None,
                                        out_pitch, out_frame, SN_MEM_DEVICE, stream or None), "sn_render")

    def render_jpeg(self, raw: np.ndarray, left_nv12: Optional[np.ndarray] = None, left_pitch: int = 0, params=None,
                    quality: int = 95, rows_per_slice: int = 1, out_stride: int = 0, raw_out: bool = False):
        """sn_render_jpeg on host buffers (render.canvas_jpeg is the numpy twin): the JPEG of every NV12 canvas -> list of n bytes
        objects, None where a stream did not fit out_stride (0: sn_jpeg_bound of the canvas); raw_out: (uint8 (n, out_stride),
        uint32 (n,))."""
        prm = render_params(params)
        r, n, left, left_pitch = self._render_inputs(raw, left_nv12, left_pitch, prm, "render_jpeg")
        out_stride = out_stride or jpeg_bound(self.width, self.height * (2 if prm.layout == 0 else 1)) or 1
        out = np.empty((n, out_stride), np.uint8)
        sizes = np.zeros(n, np.uint32)
        jp = SnJpegParams(quality, rows_per_slice)
        self._check(self._lib.sn_render_jpeg(self._h, n, r.ctypes.data, _np_ptr(left), left_pitch, C.byref(prm), C.byref(jp),
                                             out.ctypes.data, out_stride, sizes.ctypes.data, SN_MEM_HOST, None), "sn_render_jpeg")
        if raw_out:
            return out, sizes
        return [out[k, :sizes[k]].tobytes() if sizes[k] else None for k in range(n)]

    def render_jpeg_device(self, n: int, raw_ptr: int, left_ptr: int, left_pitch: int, params, quality: int, rows_per_slice: int,
                           out_ptr: int, out_stride: int, sizes_ptr: int, stream: int = 0):
        """sn_render_jpeg on device pointers; stream as in render_device."""
        prm = render_params(params)
        jp = SnJpegParams(quality, rows_per_slice)
        self._check(self._lib.sn_render_jpeg(self._h, n, raw_ptr or None, left_ptr or None, left_pitch, C.byref(prm), C.byref(jp),
                                             out_ptr or None, out_stride, sizes_ptr or None, SN_MEM_DEVICE, stream or None),
                    "sn_render_jpeg")

    def dbg_jpeg_dct(self, nv12: np.ndarray, w: int, h: int, pitch: int = 0) -> np.ndarray:
        """sn_dbg_jpeg_dct: the fp32 coefficients of the encoder's transform before quantisation -> float32 (blocks, 64)"""
        src = np.ascontiguousarray(nv12, np.uint8).reshape(-1)
        pitch = pitch or w
        out = np.empty((((w + 15) // 16) * ((h + 15) // 16) * 6, 64), np.float32)
        assert src.size >= (h + h // 2 - 1) * pitch + w
        self._check(self._lib.sn_dbg_jpeg_dct(self._h, src.ctypes.data, w, h, pitch, out.ctypes.data), "sn_dbg_jpeg_dct")
        return out

    def synchronize(self):
        self._check(self._lib.sn_synchronize(self._h), "sn_synchronize")

    # -- measurement -------------------------------------------------------------------------------
    def set_profiling(self, on: bool):
        self._check(self._lib.sn_set_profiling(self._h, int(on)), "sn_set_profiling")

    def stage_ms(self) -> dict:
        arr = (C.c_float * len(STAGES))()
        self._check(self._lib.sn_get_stage_ms(self._h, arr, len(STAGES)), "sn_get_stage_ms")
        return dict(zip(STAGES, [float(v) for v in arr]))

    def dominant_kernel(self) -> dict:
        name = C.create_string_buffer(128)
        launches = C.c_int()
        fl, by = C.c_double(), C.c_double()
        self._check(self._lib.sn_get_dominant_kernel(self._h, name, 128, C.byref(launches), C.byref(fl), C.byref(by)),
                    "sn_get_dominant_kernel")
        return {"name": name.value.decode(), "launches": launches.value, "flops_per_launch": fl.value,
                "bytes_per_launch": by.value}

    # -- parity hooks --------------------------------------------------------------------------------
    def dbg_set_grid_cus(self, cus: int = 0):
        """sn_dbg_set_grid_cus: the CU count the parity hooks (and only they) size their persistent grids with; 0 = the
        device's.  Hooks whose launcher builds its grid in bands of 8 refuse a value that is no multiple of 8."""
        self._check(self._lib.sn_dbg_set_grid_cus(self._h, int(cus)), "sn_dbg_set_grid_cus")

    def dbg_last_launch(self):
        """-> (workgroups, work units) of the last hook call's last persistent launch: tiles, half tiles for
        k_ref_conv_f32, flat rows for the streamed blocks"""
        wgs, units = C.c_int(0), C.c_int(0)
        self._check(self._lib.sn_dbg_last_launch(self._h, C.byref(wgs), C.byref(units)), "sn_dbg_last_launch")
        return wgs.value, units.value

    def dbg_slot_graphs(self):
        """sn_dbg_slot_graphs -> (enabled, instantiated, launches): whether the async slots still replay hipGraphs (0 under
        SN_NO_GRAPH, or after a capture failed and they fell back to plain launches), the graphs instantiated and the
        requests served by hipGraphLaunch over the handle's life"""
        en, inst, launches = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        self._check(self._lib.sn_dbg_slot_graphs(self._h, C.byref(en), C.byref(inst), C.byref(launches)), "sn_dbg_slot_graphs")
        return en.value, inst.value, launches.value

    @staticmethod
    def _batch(x, dtype=np.float32):
        """(c, h, w) or (n, c, h, w) -> contiguous (n, c, h, w) and whether the caller passed one image without the batch axis"""
        x = np.ascontiguousarray(x, dtype)
        return (x[None], True) if x.ndim == 3 else (x, False)

    @staticmethod
    def _f32(*arrays):
        """contiguous float32 arrays (None stays None): the weights, biases and residual of a hook"""
        return [None if a is None else np.ascontiguousarray(a, np.float32) for a in arrays]

    def _hook(self, name, out, one, *args):
        """hook `name`(handle, *args, out), arrays passed by address (None = NULL) -> out, without the batch axis if `one`"""
        a = [_np_ptr(v) if v is None or isinstance(v, np.ndarray) else v for v in args]
        self._check(getattr(self._lib, name)(self._h, *a, out.ctypes.data), name)
        return out[0] if one else out

    @staticmethod
    def _conv_form(x3, slots, dma=False, tower32=False):
        """the SN_DBG_CONV_* enumerator of the keywords; -1, which the hooks refuse, where there is none"""
        if x3 != slots or (dma and not slots):
            return -1
        return (3 if dma else 2) if slots else (1 if tower32 else 0)

    def dbg_conv2d(self, x, wt, bias, k, stride=1, dil=1, lrelu=False, residual=None, x3=False, slots=False, tower32=False, dma=False):
        """x (cin, h, w) or (n, cin, h, w): n images in one launch.  dma (with x3 and slots): the kernel of the zero-bordered
        tensors — k_down_x3s_dma (5x5 stride 2) or k_feat_x3s_dma (3x3, also with a residual); the hook also checks that the
        borders stay zero"""
        x, one = self._batch(x)
        wt, bias, res = self._f32(wt, bias, residual)
        n, cin, h, w = x.shape
        ho, wo = (h, w) if stride == 1 else (h // 2, w // 2)
        out = np.empty((n, 32, ho, wo), np.float32)
        assert res is None or res.size == out.size
        return self._hook("sn_dbg_conv2d_n", out, one, n, x, cin, h, w, wt, bias, k, stride, dil, int(bool(lrelu)),
                          self._conv_form(x3, slots, dma, tower32), res)

    def dbg_down0(self, in6, wt, bias, tc=32):
        """in6 int8 (6,h,w) -> float32 (2, 32, ho, wo): first down-conv of both eyes on the fp16 MFMA; in6 (n,6,h,w): n pairs
        in one launch -> (2n, 32, ho, wo)."""
        x, _ = self._batch(in6, np.int8)
        wt, bias = self._f32(wt, bias)
        n, _, h, w = x.shape
        out = np.empty((2 * n, 32, (h + 15) // 16 * 8, (w + 15) // 16 * 8), np.float32)
        return self._hook("sn_dbg_down0_n", out, False, n, x, h, w, wt, bias, tc)

    def dbg_down01(self, in6, w0, b0, w1, b1):
        """in6 int8 (6,h,w) -> float32 (2, 32, ho, wo), ho/wo = ceil16/4: the first two down-convs of both eyes as the
        folded 13x13 stride-4 convolution (k_down01_f16 + k_down01_border); in6 (n,6,h,w): n pairs in one launch -> (2n, ...)."""
        x, _ = self._batch(in6, np.int8)
        w0, b0, w1, b1 = self._f32(w0, b0, w1, b1)
        assert w0.shape == (32, 3, 5, 5) and w1.shape == (32, 32, 5, 5) and b0.shape == (32,) and b1.shape == (32,)
        n, _, h, w = x.shape
        out = np.empty((2 * n, 32, (h + 15) // 16 * 4, (w + 15) // 16 * 4), np.float32)
        return self._hook("sn_dbg_down01_n", out, False, n, x, h, w, w0, b0, w1, b1)

    def dbg_refin(self, disp_low, in6, dmax, wt, bias, split=False):
        """disp_low float32 (hp/16, wp/16), in6 int8 (6,h,w) -> float32 (32, hp, wp): refinement input conv; with a leading
        batch axis on both, n images in one launch."""
        x, one = self._batch(in6, np.int8)
        dl, wt, bias = self._f32(disp_low, wt, bias)
        n, _, h, w = x.shape
        hp, wp = (h + 15) // 16 * 16, (w + 15) // 16 * 16
        assert dl.shape == ((hp // 16, wp // 16) if one else (n, hp // 16, wp // 16))
        out = np.empty((n, 32, hp, wp), np.float32)
        return self._hook("sn_dbg_refin_n", out, one, n, dl, x, h, w, dmax, wt, bias, int(split))

    def dbg_conv3d(self, x, wt, bias, lrelu=False, x3=False, slots=False, dma=False):
        """dma: the aggregation kernel on zero-bordered volumes (k_agg_x3s_dma; needs x3 and slots); the hook also checks that
        the kernel left the borders untouched"""
        x, wt, bias = self._f32(x, wt, bias)
        _, d, h, w = x.shape
        return self._hook("sn_dbg_conv3d", np.empty_like(x), False, x, d, h, w, wt, bias, int(bool(lrelu)), self._conv_form(x3, slots, dma))

    def dbg_ref_conv_f16(self, x, wt, bias, dil=1, lrelu=False, residual=None, tile_w=0):
        """x (32, h, w) or (n, 32, h, w): n images in one launch.  tile_w: 0 = the width the engine would choose for this
        launch, 64 / 32 = force that variant (dilation 1, 2)"""
        x, one = self._batch(x)
        wt, bias, res = self._f32(wt, bias, residual)
        n, _, h, w = x.shape
        out = np.empty((n, 32, h, w), np.float32)
        assert res is None or res.size == out.size
        return self._hook("sn_dbg_ref_conv_f16_n", out, one, n, x, h, w, wt, bias, dil, int(bool(lrelu)),
                          tile_w if tile_w in (64, 32) else 0, res)

    def dbg_ref_conv_f16x3(self, x, wt, bias, dil=1, lrelu=False, residual=None):
        x, one = self._batch(x)
        wt, bias, res = self._f32(wt, bias, residual)
        n, _, h, w = x.shape
        out = np.empty((n, 32, h, w), np.float32)
        assert res is None or res.size == out.size
        return self._hook("sn_dbg_ref_conv_f16x3_n", out, one, n, x, h, w, wt, bias, dil, int(bool(lrelu)), res)

    def dbg_ref_block_f16(self, x, w1, b1, w2, b2, dil=1, fused=0):
        """fused: 0 = two conv launches, 2 = row-streaming fused kernel (every dilation: 1, 2, 4, 8)"""
        x, one = self._batch(x)
        n, _, h, w = x.shape
        form = {0: 0, 2: 1}.get(fused, -1)          # -1: the hook refuses it
        return self._hook("sn_dbg_ref_block_f16_n", np.empty((n, 32, h, w), np.float32), one, n, x, h, w,
                          *self._f32(w1, b1, w2, b2), dil, form)

    def dbg_ref_block_f16x3(self, x, w1, b1, w2, b2, dil=1, streamed=False):
        """the same block on split operands (SN_PREC_F16X3): two k_ref_conv_f16x3 launches, or the row-streaming fused kernel"""
        x, one = self._batch(x)
        n, _, h, w = x.shape
        return self._hook("sn_dbg_ref_block_f16x3_n", np.empty((n, 32, h, w), np.float32), one, n, x, h, w,
                          *self._f32(w1, b1, w2, b2), dil, int(streamed))

    def dbg_ref_tail_f16(self, x, w1, b1, w2, b2, head_w, head_b, low, ups, dnorm, h_out, w_out, form):
        """Last residual block + refinement head on x float32 (n, 32, hk, wk); low (n, hk/ups, wk/ups); form 0 = streamed
        block + k_head_final_f16, 1 = the tail form (one launch).  -> (disp float32, raw int32), each (n, h_out, w_out)."""
        a = [np.ascontiguousarray(v, np.float32) for v in (x, w1, b1, w2, b2, head_w, low)]
        n, _, hk, wk = a[0].shape
        assert a[6].shape == (n, hk // ups, wk // ups)
        disp = np.empty((n, h_out, w_out), np.float32)
        raw = np.empty((n, h_out, w_out), np.int32)
        self._check(self._lib.sn_dbg_ref_tail_f16(self._h, n, a[0].ctypes.data, hk, wk, a[1].ctypes.data, a[2].ctypes.data,
                                                  a[3].ctypes.data, a[4].ctypes.data, a[5].ctypes.data, float(head_b),
                                                  a[6].ctypes.data, ups, float(dnorm), h_out, w_out, form, disp.ctypes.data,
                                                  raw.ctypes.data), "sn_dbg_ref_tail_f16")
        return disp, raw

    # mid-stage hooks: every output sits between guard bands and starts as the 0xff pattern (include/stereonet_hip.h)
    def dbg_cost_volume(self, feat, dl, form):
        """feat float32 (2n, 32, hl, wl), left / right interleaved -> cost volume (n, dl, 32, hl, wl) read back from split slots;
        form 0 = k_cost_slots, 1 = k_cost_slots_pad (zero-bordered volume; the hook checks the borders)"""
        f = np.ascontiguousarray(feat, np.float32)
        n2, c, hl, wl = f.shape
        assert c == 32 and n2 % 2 == 0
        out = np.empty((n2 // 2, dl, 32, hl, wl), np.float32)
        self._check(self._lib.sn_dbg_cost_volume(self._h, f.ctypes.data, n2 // 2, dl, hl, wl, form, out.ctypes.data),
                    "sn_dbg_cost_volume")
        return out

    def dbg_agg_first_f32(self, feat, dl, wt, bias):
        """the fp32 first aggregation layer with the cost-volume loader -> (n, 32, dl, hl, wl)"""
        f, wt, bias = (np.ascontiguousarray(a, np.float32) for a in (feat, wt, bias))
        n2, c, hl, wl = f.shape
        assert c == 32 and n2 % 2 == 0 and wt.size == 32 * 32 * 27 and bias.size == 32
        out = np.empty((n2 // 2, dl, 32, hl, wl), np.float32)
        self._check(self._lib.sn_dbg_agg_first_f32(self._h, f.ctypes.data, n2 // 2, dl, hl, wl, wt.ctypes.data, bias.ctypes.data,
                                                   out.ctypes.data), "sn_dbg_agg_first_f32")
        return np.ascontiguousarray(out.transpose(0, 2, 1, 3, 4))

    def dbg_softargmin(self, v, bias, w=None, want_conf=False):
        """w given: k_head_softargmin on the volume v (n, dl, 32, hl, wl) with w (32, 27); w None: k_softargmin_p on the partial
        sums v (n, dl, 27, hl, wl).  -> dict cost (n, dl, hl, wl), disp_low, conf_low (n, hl, wl; the 0xff pattern = NaN
        without want_conf), nonfinite"""
        v = np.ascontiguousarray(v, np.float32)
        n, dl, c, hl, wl = v.shape
        assert c == (27 if w is None else 32)
        wa = None if w is None else np.ascontiguousarray(w, np.float32).reshape(32, 27)
        cost = np.empty((n, dl, hl, wl), np.float32)
        disp = np.empty((n, hl, wl), np.float32)
        conf = np.empty((n, hl, wl), np.float32)
        nf = C.c_uint64()
        self._check(self._lib.sn_dbg_softargmin(self._h, n, dl, hl, wl, 1 if w is None else 0, int(want_conf), float(bias),
                                                v.ctypes.data, _np_ptr(wa), cost.ctypes.data, disp.ctypes.data, conf.ctypes.data,
                                                C.byref(nf)), "sn_dbg_softargmin")
        return {"cost": cost, "disp_low": disp, "conf_low": conf, "nonfinite": int(nf.value)}

    def dbg_agg_tail(self, vol, wt, bias, out_w, out_b, form, want_conf=False):
        """Last aggregation layer (fp32 output) + soft-argmin on vol (n, 32, dl, hl, wl); form 0 = plain slots (k_conv_x3s +
        k_head_softargmin), 1 = zero-bordered (k_agg_x3s_dma + k_head_softargmin), 2 = partial sums P (k_agg_x3s_dma HEADP +
        k_softargmin_p).  -> dict as dbg_softargmin plus layer_vol (n, 32, dl, hl, wl) for forms 0 and 1"""
        vol, wt, bias, ow = (np.ascontiguousarray(a, np.float32) for a in (vol, wt, bias, out_w))
        n, c, dl, hl, wl = vol.shape
        assert c == 32 and wt.size == 32 * 32 * 27 and bias.size == 32 and ow.size == 32 * 27
        cost = np.empty((n, dl, hl, wl), np.float32)
        disp = np.empty((n, hl, wl), np.float32)
        conf = np.empty((n, hl, wl), np.float32)
        lv = np.empty((n, dl, 32, hl, wl), np.float32) if form != 2 else None
        nf = C.c_uint64()
        self._check(self._lib.sn_dbg_agg_tail(self._h, vol.ctypes.data, n, dl, hl, wl, wt.ctypes.data, bias.ctypes.data,
                                              ow.ctypes.data, float(out_b), form, int(want_conf), cost.ctypes.data,
                                              disp.ctypes.data, conf.ctypes.data, C.byref(nf), _np_ptr(lv)), "sn_dbg_agg_tail")
        return {"cost": cost, "disp_low": disp, "conf_low": conf, "nonfinite": int(nf.value),
                "layer_vol": None if lv is None else np.ascontiguousarray(lv.transpose(0, 2, 1, 3, 4))}

    def dbg_head(self, x, head_w, head_b, low, ups, dnorm, h_out, w_out, form):
        """The refinement head alone on x float32 (n, 32, hk, wk), low (n, hk/ups, wk/ups); form 0 = k_head_final, 1 =
        k_head_final_mfma32 (fp32 engine), 2 = k_head_final_f16<true> on the hi / lo tensor (fp16-mode engine).
        -> dict disp float32, raw int32 (n, h_out, w_out), mean_abs_dr, nonfinite"""
        x, hw, low = (np.ascontiguousarray(a, np.float32) for a in (x, head_w, low))
        n, c, hk, wk = x.shape
        assert c == 32 and hw.size == 32 * 9 and low.shape == (n, hk // ups, wk // ups)
        disp = np.empty((n, h_out, w_out), np.float32)
        raw = np.empty((n, h_out, w_out), np.int32)
        mean, nf = C.c_double(), C.c_uint64()
        self._check(self._lib.sn_dbg_head(self._h, n, x.ctypes.data, hk, wk, hw.ctypes.data, float(head_b), low.ctypes.data, ups,
                                          float(dnorm), h_out, w_out, form, disp.ctypes.data, raw.ctypes.data, C.byref(mean),
                                          C.byref(nf)), "sn_dbg_head")
        return {"disp": disp, "raw": raw, "mean_abs_dr": float(mean.value), "nonfinite": int(nf.value)}

    def dbg_img_pool2(self, in6, levels):
        """in6 int8 (n, 6, h, w) -> [level 1, ..., level levels-1], level k float32 (n, 3, hp >> k, wp >> k): the image pyramid of
        the hierarchical refinement through both k_img_pool2 instantiations, chained as the forward pass chains them"""
        a = np.ascontiguousarray(in6, np.int8)
        n, c, h, w = a.shape
        assert c == 6 and 2 <= levels <= 4
        hp, wp = (h + 15) // 16 * 16, (w + 15) // 16 * 16
        shapes = [(n, 3, hp >> k, wp >> k) for k in range(1, levels)]
        flat = np.empty(sum(int(np.prod(s)) for s in shapes), np.float32)
        self._check(self._lib.sn_dbg_img_pool2(self._h, a.ctypes.data, n, h, w, levels, flat.ctypes.data), "sn_dbg_img_pool2")
        out, at = [], 0
        for s in shapes:
            out.append(flat[at:at + int(np.prod(s))].reshape(s).copy())
            at += int(np.prod(s))
        return out

    def stream_priority_high(self) -> bool:
        """True when the engine's pipeline streams were created with the device's highest priority (SN_STREAM_PRIORITY=1,
        or sn_mgpu_create with more than one device)."""
        return bool(self.dbg_read("stream_prio")[0])

    def dbg_read(self, what: str) -> np.ndarray:
        n = C.c_size_t()
        self._check(self._lib.sn_dbg_read(self._h, what.encode(), None, 0, C.byref(n)), "sn_dbg_read")
        out = np.empty(n.value, np.float32)
        self._check(self._lib.sn_dbg_read(self._h, what.encode(), out.ctypes.data, n.value, C.byref(n)), "sn_dbg_read")
        return out


def mgpu_shard(n: int, ndev: int, k: int):
    """(first, count) of shard k when n pairs are cut over ndev devices (sn_mgpu_shard; needs no GPU)."""
    lib = load_library()
    first, count = C.c_int(), C.c_int()
    rc = lib.sn_mgpu_shard(n, ndev, k, C.byref(first), C.byref(count))
    if rc != 0:
        raise StereoNetError(rc, "sn_mgpu_shard")
    return first.value, count.value


class SnMgpuRing(C.Structure):
    _fields_ = [("next", C.c_uint64), ("slot_ticket", C.c_uint64 * 2)]


class MgpuRing:
    """The ticket / buffer-slot bookkeeping of sn_mgpu_submit_device / sn_mgpu_wait (pure; needs no GPU)."""

    def __init__(self):
        self._lib = load_library()
        self._r = SnMgpuRing()
        self._lib.sn_mgpu_ring_init(C.byref(self._r))

    def submit(self):
        t, s = C.c_uint64(), C.c_int()
        rc = self._lib.sn_mgpu_ring_submit(C.byref(self._r), C.byref(t), C.byref(s))
        if rc != 0:
            raise StereoNetError(rc, "sn_mgpu_ring_submit")
        return t.value, s.value

    def wait(self, ticket: int) -> int:
        s = C.c_int()
        rc = self._lib.sn_mgpu_ring_wait(C.byref(self._r), C.c_uint64(ticket), C.byref(s))
        if rc != 0:
            raise StereoNetError(rc, "sn_mgpu_ring_wait")
        return s.value


class StereoNetMultiGPU:
    """sn_mgpu_*: one batch sharded over the GPUs of one node inside ONE process (one host thread per GPU)."""

    def __init__(self, model_file: str, devices=None, ndev: int = 0, max_batch: int = 1, precision: int = PREC_DEFAULT,
                 refine_chunk: int = 0, piece: int = 0, width: int = 0, height: int = 0, dmax: int = 0):
        self._lib = load_library()
        self._m = C.c_void_p()
        devs = list(devices) if devices is not None else None
        if devs is None and ndev <= 0:      # neither given: every visible GPU (sn_mgpu_create itself rejects ndev <= 0)
            import torch
            ndev = torch.cuda.device_count() if torch.cuda.is_available() else 0
            if ndev <= 0:
                raise StereoNetError(-4, "StereoNetMultiGPU: no GPU visible and neither devices nor ndev given")
        n = len(devs) if devs is not None else ndev
        arr = (C.c_int * n)(*devs) if devs is not None else None
        cfg = SnConfig(-1, max_batch, width, height, dmax, precision, 4, refine_chunk, piece)
        rc = self._lib.sn_mgpu_create(model_file.encode(), C.byref(cfg), arr, n, C.byref(self._m))
        if rc != 0:
            self._m = C.c_void_p()
            raise StereoNetError(rc, f"sn_mgpu_create({model_file!r}, ndev={n})")
        nd, per, kind = C.c_int(), C.c_int(), C.c_int()
        self._lib.sn_mgpu_get_info(self._m, C.byref(nd), C.byref(per), C.byref(kind))
        self.ndev, self.per_device_batch, self.gather_kind = nd.value, per.value, kind.value
        h = C.c_void_p()
        self._lib.sn_mgpu_get_handle(self._m, 0, C.byref(h))
        info = SnIoInfo()
        self._lib.sn_get_io_info(h, C.byref(info))
        self.width, self.height, self.dmax = info.width, info.height, info.dmax
        self.max_batch = max_batch

    def _check(self, rc: int, where: str):
        if rc != 0:
            raise StereoNetError(rc, where, self._lib.sn_mgpu_last_error(self._m).decode() if self._m else "")

    def engine_stream_priority_high(self, k: int = 0) -> bool:
        """True when shard k's engine runs its pipeline on high-priority streams (sn_mgpu_create chooses that itself whenever
        more than one device takes part: its gather runs beside the engines)."""
        h = C.c_void_p()
        self._check(self._lib.sn_mgpu_get_handle(self._m, k, C.byref(h)), "sn_mgpu_get_handle")
        v, n = np.empty(1, np.float32), C.c_size_t()
        rc = self._lib.sn_dbg_read(h, b"stream_prio", v.ctypes.data, 1, C.byref(n))
        if rc != 0:
            raise StereoNetError(rc, "sn_dbg_read(stream_prio)")
        return bool(v[0])

    def infer(self, in6: np.ndarray):
        """int8 (n,6,H,W) host array -> (disp float32 (n,H,W), raw int32 (n,H,W)); the host is the gather root."""
        x = np.ascontiguousarray(in6, dtype=np.int8)
        n = x.shape[0]
        disp = np.empty((n, self.height, self.width), np.float32)
        raw = np.empty((n, self.height, self.width), np.int32)
        self._check(self._lib.sn_mgpu_infer_batch(self._m, n, x.ctypes.data, raw.ctypes.data, disp.ctypes.data),
                    "sn_mgpu_infer_batch")
        return disp, raw

    def infer_device(self, n: int, in_ptrs, raw_root_ptr: int, disp_root_ptr: int):
        """in_ptrs[k] = device pointer of shard k on device k; outputs gathered on device 0."""
        arr = (C.c_void_p * self.ndev)(*[C.c_void_p(p) for p in in_ptrs])
        self._check(self._lib.sn_mgpu_infer_batch_device(self._m, n, arr, raw_root_ptr or None, disp_root_ptr or None),
                    "sn_mgpu_infer_batch_device")

    def submit_device(self, n: int, in_ptrs, raw_root_ptr: int, disp_root_ptr: int) -> int:
        """Asynchronous infer_device: returns a ticket once every device has its shard enqueued (two may be in flight)."""
        arr = (C.c_void_p * self.ndev)(*[C.c_void_p(p) for p in in_ptrs])
        t = C.c_uint64()
        self._check(self._lib.sn_mgpu_submit_device(self._m, n, arr, raw_root_ptr or None, disp_root_ptr or None, C.byref(t)),
                    "sn_mgpu_submit_device")
        return t.value

    def wait(self, ticket: int):
        self._check(self._lib.sn_mgpu_wait(self._m, C.c_uint64(ticket)), "sn_mgpu_wait")

    def close(self):
        if getattr(self, "_m", None) and self._m.value:
            self._lib.sn_mgpu_destroy(self._m)
            self._m = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Owned:
    """The lifecycle of an object created on an engine: `_destroy` names the library's destroy function, `_handle` the
    attribute that holds the object's handle.  close() is idempotent; the object is a context manager."""
    _destroy = _handle = ""

    def close(self):
        p = getattr(self, self._handle, None)
        if p:      # a c_void_p of NULL is false
            getattr(self._lib, self._destroy)(p)
            setattr(self, self._handle, C.c_void_p())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class _Streams(_Owned):
    """An object with per-stream state on the GPU: `_sym` is the prefix of its functions in the library, `_what` its name in
    this module's own messages."""
    _sym = _what = ""

    def reset(self, stream: int = -1):
        """Stream `stream` (-1: all) starts afresh at its next push."""
        self._eng._check(getattr(self._lib, self._sym + "_reset")(getattr(self, self._handle), int(stream)), self._sym + "_reset")

    def _ids(self, stream_of, n: int):
        if stream_of is None:
            return None
        ids = np.ascontiguousarray(stream_of, dtype=np.int32).reshape(-1)
        if ids.size != n:
            raise StereoNetError(-1, f"{self._what} push", f"{ids.size} stream ids for {n} maps")
        return ids


class _TorusStreams(_Streams):
    """... and the two rolling maps, whose frames come with a pose"""

    def pose_q(self, poses) -> np.ndarray:
        """sn_costmap_pose_q / sn_elevation_pose_q: (x, y, yaw) or (n, 3) -> int32 (6,) or (n, 6)"""
        q, rc, _ = _pose_q_rows(getattr(self._lib, self._sym + "_pose_q"), getattr(self, self._handle), poses)
        self._eng._check(rc, self._sym + "_pose_q")
        return q

    def _poses(self, poses, stream_of, n: int):
        ps = np.ascontiguousarray(poses, np.float64).reshape(-1)
        if ps.size != 3 * n:
            raise StereoNetError(-1, f"{self._what} push", f"{ps.size} pose numbers for {n} maps: (n, 3) is needed")
        return ps, self._ids(stream_of, n)


class TemporalFilter(_Streams):
    """sn_temporal: the temporal filter of disparity streams, with its per-stream state on the GPU (temporal.reference is the
    numpy twin).  A context object: the engine refuses to close while one of its filters is open."""
    _destroy, _handle, _sym, _what = "sn_temporal_destroy", "_t", "sn_temporal", "temporal"

    def __init__(self, engine: StereoNetHIP, streams: int = 1, alpha: int = 64, delta_px: float = 0.5, persist: int = 2,
                 luma_delta: int = 0):
        self._eng, self._lib, self._t = engine, engine._lib, C.c_void_p()
        self.streams, self.params = int(streams), SnTemporalParams(int(alpha), delta_px, int(persist), int(luma_delta))
        engine._check(self._lib.sn_temporal_create(engine._h, self.streams, C.byref(self.params), C.byref(self._t)),
                      "sn_temporal_create")

    def push(self, raw: np.ndarray, guide: Optional[np.ndarray] = None, guide_kind: int = SN_GUIDE_NV12, guide_pitch: int = 0,
             stream_of=None, disp: Optional[np.ndarray] = None):
        """sn_temporal_push on host buffers: int32 (H,W) or (n,H,W), map k the next frame of stream stream_of[k] (None: all
        of stream 0, one clip) -> (out int32, mask uint8 (SN_TMP_*), counts uint32 (n,4) = {valid, blended, held, moved or
        jumped} per map).  guide as smooth_raw's (None only with luma_delta = 0); `disp` (float32, the maps' shape) is
        rewritten IN PLACE where the result differs from max(raw, 0)."""
        eng = self._eng
        r = eng._maps(raw, "temporal push")
        dp = eng._disp_ptr(disp, r.shape, "temporal push")
        n, out, mask, counts = eng._mask_outputs(r, 4)
        ids = self._ids(stream_of, n)
        g, guide_pitch = eng._guide(guide, guide_kind, guide_pitch, n, "temporal push")
        eng._check(self._lib.sn_temporal_push(self._t, n, _np_ptr(ids), r.ctypes.data, _np_ptr(g), guide_kind, guide_pitch,
                                              out.ctypes.data, dp, mask.ctypes.data, counts.ctypes.data, SN_MEM_HOST, None),
                   "sn_temporal_push")
        return out, mask, counts

    def push_device(self, n: int, raw_ptr: int, guide_ptr: int = 0, guide_kind: int = SN_GUIDE_NV12, guide_pitch: int = 0,
                    stream_of=None, out_raw_ptr: int = 0, mask_ptr: int = 0, disp_ptr: int = 0, counts_ptr: int = 0,
                    stream: int = 0):
        """sn_temporal_push on device pointers (out_raw_ptr may equal raw_ptr; stream_of stays a host sequence); stream =
        hipStream_t as int (0: the filter's own stream, and the call returns after completion)."""
        ids = self._ids(stream_of, n)
        self._eng._check(self._lib.sn_temporal_push(self._t, n, _np_ptr(ids), raw_ptr or None, guide_ptr or None, guide_kind,
                                                    guide_pitch, out_raw_ptr or None, disp_ptr or None, mask_ptr or None,
                                                    counts_ptr or None, SN_MEM_DEVICE, stream or None), "sn_temporal_push")


class Costmap(_TorusStreams):
    """sn_costmap: a rolling log-odds costmap with ray clearing per stream, its state on the GPU (costmap.Reference is the numpy
    twin).  A context object: the engine refuses to close while one of its costmaps is open."""
    _destroy, _handle, _sym, _what = "sn_costmap_destroy", "_c", "sn_costmap", "costmap"

    def __init__(self, engine: StereoNetHIP, obstacle, params, streams: int = 1):
        self._eng, self._lib, self._c = engine, engine._lib, C.c_void_p()
        self.streams, self.params, self.obstacle = int(streams), costmap_params(params), obstacle_params(obstacle)
        engine._check(self._lib.sn_costmap_create(engine._h, self.streams, C.byref(self.obstacle), C.byref(self.params), C.byref(self._c)),
                      "sn_costmap_create")

    def push(self, poses, occ: Optional[np.ndarray] = None, ranges: Optional[np.ndarray] = None, stream_of=None,
             want=(True, True, True)):
        """sn_costmap_push on host buffers: poses (n, 3) = x, y, yaw; occ int8 (n, gh, gw) and ranges float32 (n, beams) as
        obstacles() returns them (either may be None); map k the next frame of stream stream_of[k] (None: all of stream 0, one
        clip) -> (grid int8 (n, mh, mw), logodds int16 (n, mh, mw), stats uint32 (n, 4) = {known, occupied, hit, cleared} per
        map, q int32 (n, 6)); `want` drops grid, logodds or stats (None in their place)."""
        n = int(np.size(poses)) // 3
        ps, ids = self._poses(poses, stream_of, n)
        o = None if occ is None else np.ascontiguousarray(occ, np.int8)
        r = None if ranges is None else np.ascontiguousarray(ranges, np.float32)
        cells, beams, (mh, mw) = self.obstacle.gw * self.obstacle.gh, self.obstacle.beams, (self.params.mh, self.params.mw)
        if (o is not None and o.size != n * cells) or (r is not None and r.size != n * beams):
            raise StereoNetError(-1, "costmap push", f"occ and ranges must hold {n} x {cells} cells and {n} x {beams} beams")
        grid = np.empty((n, mh, mw), np.int8) if want[0] else None
        logodds = np.empty((n, mh, mw), np.int16) if want[1] else None
        stats = np.zeros((n, 4), np.uint32) if want[2] else None
        q = np.zeros((n, 6), np.int32)
        self._eng._check(self._lib.sn_costmap_push(self._c, n, _np_ptr(ids), ps.ctypes.data, _np_ptr(o), _np_ptr(r), _np_ptr(grid),
                                                   _np_ptr(logodds), _np_ptr(stats), q.ctypes.data, SN_MEM_HOST, None), "sn_costmap_push")
        return grid, logodds, stats, q

    def push_device(self, n: int, poses, occ_ptr: int = 0, ranges_ptr: int = 0, stream_of=None, grid_ptr: int = 0, logodds_ptr: int = 0,
                    stats_ptr: int = 0, stream: int = 0) -> np.ndarray:
        """sn_costmap_push on device pointers (0: absent / not wanted; poses and stream_of stay host sequences); stream =
        hipStream_t as int (0: the costmap's own stream, and the call returns after completion) -> q int32 (n, 6)."""
        ps, ids = self._poses(poses, stream_of, n)
        q = np.zeros((n, 6), np.int32)
        self._eng._check(self._lib.sn_costmap_push(self._c, n, _np_ptr(ids), ps.ctypes.data, occ_ptr or None, ranges_ptr or None,
                                                   grid_ptr or None, logodds_ptr or None, stats_ptr or None, q.ctypes.data, SN_MEM_DEVICE,
                                                   stream or None), "sn_costmap_push")
        return q


class Elevation(_TorusStreams):
    """sn_elevation: a rolling elevation map with a step-height traversability verdict per stream, its state on the GPU
    (elevation.Reference is the numpy twin).  A context object: the engine refuses to close while one of its maps is open."""
    _destroy, _handle, _sym, _what = "sn_elevation_destroy", "_e", "sn_elevation", "elevation"
    OUTPUTS = ("trav", "hi", "lo", "rise", "stats")

    def __init__(self, engine: StereoNetHIP, params, streams: int = 1):
        self._eng, self._lib, self._e = engine, engine._lib, C.c_void_p()
        self.streams, self.params = int(streams), elevation_params(params)
        engine._check(self._lib.sn_elevation_create(engine._h, self.streams, C.byref(self.params), C.byref(self._e)),
                      "sn_elevation_create")

    def push(self, poses, raw: np.ndarray, cam, mounts: Optional[np.ndarray] = None, stream_of=None,
             want=(True, True, True, True, True)):
        """sn_elevation_push on host buffers: poses (n, 3) = x, y, yaw; raw int32 (H, W) or (n, H, W); cam a
        pointcloud.Camera; mounts float32 (n, 12) or None (the parameters' mount); map k the next frame of stream stream_of[k]
        (None: all of stream 0, one clip) -> (trav int8, hi int16, lo int16, rise uint16, each (n, mh, mw), stats uint32 (n, 4)
        = {known, lethal, fused, points} per map, q int32 (n, 6)); `want` drops outputs (None in their place)."""
        eng = self._eng
        r = eng._maps(raw, "elevation push")
        n = eng._count(r)
        ps, ids = self._poses(poses, stream_of, n)
        c = _sn_camera(cam, eng.width, eng.height)
        m = None if mounts is None else np.ascontiguousarray(mounts, np.float32).reshape(-1)
        if m is not None and m.size != 12 * n:
            raise StereoNetError(-1, "elevation push", f"{m.size} mount numbers for {n} maps: (n, 12) is needed")
        mh, mw = self.params.mh, self.params.mw
        dts = (np.int8, np.int16, np.int16, np.uint16)
        outs = [np.empty((n, mh, mw), d) if w_ else None for d, w_ in zip(dts, want)]
        stats = np.zeros((n, 4), np.uint32) if want[4] else None
        q = np.zeros((n, 6), np.int32)
        eng._check(self._lib.sn_elevation_push(self._e, n, _np_ptr(ids), ps.ctypes.data, r.ctypes.data, C.byref(c), _np_ptr(m), 12,
                                               *[_np_ptr(o) for o in outs], _np_ptr(stats), q.ctypes.data, SN_MEM_HOST, None),
                   "sn_elevation_push")
        return (*outs, stats, q)

    def push_device(self, n: int, poses, raw_ptr: int, cam, mounts_ptr: int = 0, mount_stride: int = 12, stream_of=None,
                    trav_ptr: int = 0, hi_ptr: int = 0, lo_ptr: int = 0, rise_ptr: int = 0, stats_ptr: int = 0,
                    stream: int = 0) -> np.ndarray:
        """sn_elevation_push on device pointers (0: absent / not wanted; poses and stream_of stay host sequences); stream =
        hipStream_t as int (0: the object's own stream, and the call returns after completion) -> q int32 (n, 6)."""
        ps, ids = self._poses(poses, stream_of, n)
        c = _sn_camera(cam, self._eng.width, self._eng.height)
        q = np.zeros((n, 6), np.int32)
        self._eng._check(self._lib.sn_elevation_push(self._e, n, _np_ptr(ids), ps.ctypes.data, raw_ptr or None, C.byref(c),
                                                     mounts_ptr or None, int(mount_stride), trav_ptr or None, hi_ptr or None,
                                                     lo_ptr or None, rise_ptr or None, stats_ptr or None, q.ctypes.data,
                                                     SN_MEM_DEVICE, stream or None), "sn_elevation_push")
        return q


class Rectifier(_Owned):
    """sn_rectify: raw NV12 pairs of the calibration's source size -> rectified side-by-side NV12 frames of the model's size
    (and the int8 model tensor), on the GPU (rectify.reference is the numpy twin).  A context object: the engine refuses to
    close while one of its rectifiers is open."""
    _destroy, _handle = "sn_rectify_destroy", "_r"

    def __init__(self, engine: StereoNetHIP, calib):
        self._eng, self._lib, self._r = engine, engine._lib, C.c_void_p()
        self.calib = stereo_calib(calib)
        engine._check(self._lib.sn_rectify_create(engine._h, C.byref(self.calib), C.byref(self._r)), "sn_rectify_create")
        self.src_w, self.src_h = self.calib.src_w, self.calib.src_h

    @property
    def info(self) -> dict:
        """{src_w, src_h, w, h, valid_left, valid_right}: valid_* = map entries with a source"""
        i = SnRectifyInfo()
        self._eng._check(self._lib.sn_rectify_get_info(self._r, C.byref(i)), "sn_rectify_get_info")
        return {k: int(getattr(i, k)) for k, _ in SnRectifyInfo._fields_}

    @property
    def camera(self):
        """pointcloud.Camera of the rectified left eye (sn_rectify_get_camera)"""
        from . import pointcloud
        c = SnCamera()
        self._eng._check(self._lib.sn_rectify_get_camera(self._r, C.byref(c)), "sn_rectify_get_camera")
        return pointcloud.Camera(fx=c.fx, fy=c.fy, cx=c.cx, cy=c.cy, baseline_mm=c.baseline_mm, z_min_m=c.z_min_m,
                                 z_max_m=c.z_max_m, step=c.step)

    def map(self, eye: int) -> np.ndarray:
        """the device copy of an eye's map: int32 (H, W, 2)"""
        out = np.empty((self._eng.height, self._eng.width, 2), np.int32)
        self._eng._check(self._lib.sn_rectify_get_map(self._r, int(eye), out.ctypes.data), "sn_rectify_get_map")
        return out

    def rectify(self, left: np.ndarray, right: Optional[np.ndarray] = None, pitch: int = 0, n: int = 1, frame: int = 0,
                want_sbs: bool = True, want_tensor: bool = False):
        """sn_rectify_nv12 on host buffers.  left / right: uint8 buffers that start at pair 0's eye (right None: side-by-side
        frames, the right eye src_w bytes into the left's rows); pitch (0: src_w, or 2 src_w side by side) and frame (0: pitch *
        src_h * 3/2) are src_pitch and src_frame -> uint8 (n, H*3/2, 2W) and / or int8 (n, 6, H, W)."""
        eng, sw, sh = self._eng, self.src_w, self.src_h
        le = np.ascontiguousarray(left, dtype=np.uint8).reshape(-1)
        pitch = pitch or (2 * sw if right is None else sw)
        frame = frame or pitch * (sh + sh // 2)
        span = (n - 1) * frame + (sh + sh // 2 - 1) * pitch + sw
        re = le[sw:] if right is None else np.ascontiguousarray(right, dtype=np.uint8).reshape(-1)
        if n < 1 or pitch < sw or le.size < span or re.size < span:      # the library cannot see how long a host buffer is
            raise StereoNetError(-1, "rectify", f"{n} eyes of {sw}x{sh} at pitch {pitch} take {span} bytes, the buffers have "
                                                f"{le.size} and {re.size}")
        w, h = eng.width, eng.height
        sbs = np.empty((n, h + h // 2, 2 * w), np.uint8) if want_sbs else None
        ten = np.empty((n, 6, h, w), np.int8) if want_tensor else None
        eng._check(self._lib.sn_rectify_nv12(self._r, n, le.ctypes.data, re.ctypes.data, pitch, frame, _np_ptr(sbs), _np_ptr(ten),
                                             SN_MEM_HOST, None), "sn_rectify_nv12")
        return (sbs, ten) if want_sbs and want_tensor else sbs if want_sbs else ten

    def rectify_device(self, n: int, left_ptr: int, right_ptr: int, pitch: int, frame: int, sbs_ptr: int = 0, tensor_ptr: int = 0,
                       stream: int = 0):
        """sn_rectify_nv12 on device pointers; stream = hipStream_t as int (0: the rectifier's own stream, and the call returns
        after completion)."""
        self._eng._check(self._lib.sn_rectify_nv12(self._r, n, left_ptr or None, right_ptr or None, pitch, frame, sbs_ptr or None,
                                                   tensor_ptr or None, SN_MEM_DEVICE, stream or None), "sn_rectify_nv12")
