"""ctypes binding of libvstab.so (the C ABI in include/vstab.h) for tests, bench.py and smoke().

This is a thin test/bench driver, not the product: the product is the HIP/C++ library.  There
is NO fallback: if lib/libvstab.so is missing or fails to load, importing this module raises.
Device memory and streams come from PyTorch-ROCm (plumbing only): functions take CUDA uint8 /
float32 tensors and enqueue on torch's current stream.

Import with ``importlib.import_module("video-annotator_amd")`` (the directory name is not a
Python identifier).
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# Always the in-tree product library.  (Development tools that want another build load this module by hand and plant a
# path in its namespace first -- tools/devlib.py; no environment variable can swap the library under the tests.)
LIB_PATH = globals().get("_VSTAB_LIB_OVERRIDE") or os.path.join(_HERE, "lib", "libvstab.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `make -C {_HERE}` (or __graft_entry__.build()); "
        "there is no CPU fallback for the HIP path")

# PyTorch-ROCm bundles its own libamdhip64.so.7; it must be the one already mapped when libvstab.so
# resolves the same SONAME, or the process ends up with two HIP runtimes and no visible device.
import torch  # noqa: E402,F401  (plumbing: device memory + streams)

_L = ctypes.CDLL(LIB_PATH)

OK, EOF, ERR_INVALID, ERR_DEVICE, ERR_NOMEM, ERR_SOURCE, ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5, -6

(GOPRO_H4B_WIDE43_PUBLISHED, GOPRO_H4B_WIDE43_MEASURED, GOPRO_H4B_WIDE43_MEASURED_STABILISATION,
 GOPRO_H4B_WIDE169_PUBLISHED, GOPRO_H4B_WIDE169_MEASURED, GOPRO_H4B_WIDE169_MEASURED_STABILISATION) = range(6)

_c = ctypes
_vp, _sz, _i, _d = _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_double
_dp, _fp, _ip = _c.POINTER(_c.c_double), _c.POINTER(_c.c_float), _c.POINTER(_c.c_int)

_u8p, _i64, _u64 = _c.POINTER(_c.c_ubyte), _c.c_int64, _c.c_uint64


class Frame(_c.Structure):  # vstab_frame
    _fields_ = [("y", _vp), ("uv", _vp), ("pitch_y", _sz), ("pitch_uv", _sz), ("width", _i), ("height", _i),
                ("mem", _i), ("pts", _i64), ("delta_rotation", _dp), ("bit_depth", _i), ("hold", _i),
                ("readout_rotation", _dp), ("dmabuf_fd", _i), ("dmabuf_size", _sz), ("dmabuf_modifier", _u64)]


PULL_FN = _c.CFUNCTYPE(_i, _vp, _c.POINTER(Frame))


class Source(_c.Structure):  # vstab_source
    _fields_ = [("pull", PULL_FN), ("peek", PULL_FN), ("user", _vp)]


class Config(_c.Structure):  # vstab_config
    _fields_ = [("abi_version", _i), ("preset", _i), ("scale", _d), ("crop_borders", _i), ("zoom", _d), ("smooth_radius", _i),
                ("interpolation", _i), ("smoother", _i), ("tracking", _i), ("seed", _u64), ("stream", _vp),
                ("lens_mode", _i), ("in_projection", _i), ("out_projection", _i), ("in_dfov", _d), ("out_dfov", _d),
                ("out_width", _i), ("out_height", _i), ("out_cx", _d), ("out_cy", _d), ("debug", _i), ("pixel_depth", _i),
                ("blend", _i), ("read_ahead", _i), ("map_precision", _i), ("resample", _i)]


class FrameLog(_c.Structure):  # vstab_frame_log
    _fields_ = [("key_frame", _i), ("n_corners", _i), ("n_tracked", _i), ("n_inliers", _i), ("fallback", _i),
                ("R_frame", _d * 9), ("R_accum", _d * 9)]


class Profile(_c.Structure):  # vstab_profile
    _fields_ = [("frames_consumed", _c.c_long), ("frames_emitted", _c.c_long), ("key_frames", _c.c_long),
                ("gpu_ingest_ms", _d), ("gpu_pyramid_ms", _d), ("gpu_corners_ms", _d), ("gpu_lk_ms", _d), ("gpu_warp_ms", _d),
                ("host_corners_ms", _d), ("host_track_wait_ms", _d), ("host_estimate_ms", _d), ("host_smooth_ms", _d),
                ("warp_launches", _c.c_long), ("warp_timed", _c.c_long),
                ("dmabuf_imports", _c.c_long), ("dmabuf_evictions", _c.c_long), ("dmabuf_cached", _c.c_long),
                ("corner_selections_by_caller", _c.c_long), ("corner_selections_by_helper", _c.c_long), ("epochs_in_turn", _c.c_long)]


SMOOTHER_SG, SMOOTHER_KALMAN, SMOOTHER_NONE, SMOOTHER_FIXED = 0, 1, 2, 3
PROJ_RECT, PROJ_FISH = 0, 1
MAP_CREATEMAP_CL, MAP_FISH_TO_RECT, MAP_FISH_TO_FISH, MAP_RECT_TO_RECT, MAP_RECT_TO_FISH, MAP_CREATEMAP_CL_OPENCL = range(6)
OUT_BGR8, OUT_NV12, OUT_NV12_PLANAR = 0, 1, 2
MAP_PRECISION_IEEE, MAP_PRECISION_OPENCL = 0, 1
RESAMPLE_DEFAULT, RESAMPLE_CUBIC, RESAMPLE_LANCZOS4 = 0, 2, 4  # vstab_config.resample (2 = cv::INTER_CUBIC, 4 = cv::INTER_LANCZOS4)
# cv::remap's borderMode (cv::BorderTypes values): vstab_remap_bilinear_border, vstab_warp_nv12_border, vstab_set_border_mode; with INTER_CUBIC /
# INTER_LANCZOS4: vstab_remap_{cubic,lanczos4}_border, vstab_warp_nv12_{cubic,lanczos4}_border, vstab_set_border_mode_ex
BORDER_CONSTANT, BORDER_REPLICATE, BORDER_REFLECT, BORDER_REFLECT_101 = 0, 1, 2, 4
# the colour spec of the BGR path (include/vstab.h, "Colour matrix and range"): matrix, range
COLOUR_CVTCOLOR, COLOUR_BT601, COLOUR_BT709, COLOUR_BT2020 = range(4)
RANGE_LIMITED, RANGE_FULL = 0, 1
READOUT_REFUSE, READOUT_PER_ROW = 0, 1  # vstab_set_readout_warp
_pp = _c.POINTER(_vp)

# name -> (restype, argtypes); mirrors include/vstab.h one to one
SIGNATURES = {
    "vstab_last_error": (_c.c_char_p, []),
    "vstab_version": (_c.c_char_p, []),
    "vstab_device_count": (_i, []),
    "vstab_struct_size": (_i, [_i]),
    "vstab_abi_version": (_i, []),
    "vstab_get_preset_camera": (_i, [_i, _i, _i, _dp]),
    "vstab_get_output_camera": (_i, [_dp, _i, _i, _d, _i, _d, _dp, _ip, _ip]),
    "vstab_fisheye_undistort_points": (_i, [_dp, _i, _dp, _dp, _dp, _dp]),
    "vstab_map_params": (None, [_dp, _dp, _dp, _fp]),
    "vstab_pack_nv12": (_i, [_vp, _sz, _vp, _sz, _i, _i, _vp, _vp]),
    "vstab_pack_p010": (_i, [_vp, _sz, _vp, _sz, _i, _i, _vp, _vp]),
    "vstab_cvt_nv12_bgr": (_i, [_vp, _sz, _vp, _sz, _i, _i, _vp, _sz, _vp]),
    "vstab_create_map": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _vp]),
    "vstab_remap_bilinear": (_i, [_vp, _sz, _i, _i, _i, _vp, _sz, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "vstab_warp_nv12_bgr": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _vp, _sz, _i, _i, _vp]),
    "vstab_warp_nv12_nearest": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _vp, _sz, _i, _i, _vp]),
    "vstab_warp_nv12_nearest_ex": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _i, _vp, _sz, _i, _i, _vp]),
    "vstab_create_map_ex": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _i, _vp]),
    "vstab_warp_nv12_ex": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _i, _i, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "vstab_warp_nv12_rs": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _fp, _i, _i, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "vstab_quantised_map_bytes": (_sz, [_i, _i]),
    "vstab_quantised_map": (_i, [_vp, _i, _i, _fp, _i, _vp]),
    "vstab_warp_nv12_mapped": (_i, [_vp, _sz, _vp, _sz, _i, _i, _vp, _i, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "vstab_draw_markers": (_i, [_vp, _sz, _i, _i, _i, _vp, _i, _i, _c.c_uint, _vp]),
    "vstab_pyr_down": (_i, [_vp, _sz, _i, _i, _vp, _sz, _vp]),
    "vstab_pyr_down_x2": (_i, [_vp, _sz, _i, _i, _vp, _sz, _vp, _sz, _vp]),
    "vstab_min_eig": (_i, [_vp, _sz, _i, _i, _vp, _vp]),
    "vstab_good_features": (_i, [_vp, _sz, _i, _i, _i, _d, _d, _fp, _ip, _vp]),
    "vstab_pull_frame_bgr16": (_i, [_vp, _vp, _sz]),
    "vstab_warp_p010": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _fp, _i, _i, _vp, _sz, _i, _i, _vp]),
    "vstab_good_features_ex": (_i, [_vp, _sz, _i, _i, _i, _d, _d, _i, _fp, _ip, _ip, _vp]),
    "vstab_pyr_lk": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _i, _fp, _u8p, _vp]),
    "vstab_pyr_lk_ex": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _i, _fp, _u8p, _fp, _i, _i, _d, _d, _i, _vp]),
    "vstab_estimate_rotation": (_i, [_fp, _fp, _i, _dp, _dp, _u64, _dp, _ip]),
    "vstab_time_next_launch": (None, [_vp, _vp]),
    "vstab_sg_weights": (_i, [_i, _dp]),
    "vstab_gyro_integrate": (_i, [_vp, _i, _d, _d, _d, _d, _dp, _dp]),
    "vstab_gpmf_parse_gyro": (_i, [_vp, _sz, _d, _d, _vp, _i, _ip]),
    "vstab_preload_kernels": (_i, []),
    "vstab_rotation_filter_create": (_i, [_i, _pp]),
    "vstab_rotation_filter_add": (_i, [_vp, _dp]),
    "vstab_rotation_filter_filter": (_i, [_vp, _dp]),
    "vstab_rotation_filter_destroy": (None, [_vp]),
    "vstab_config_default": (None, [_c.POINTER(Config)]),
    "vstab_create": (_i, [_c.POINTER(Config), _c.POINTER(Source), _pp]),
    "vstab_get_output_info": (_i, [_vp, _ip, _ip, _dp, _dp]),
    "vstab_pull_frame": (_i, [_vp, _vp, _sz]),
    "vstab_warp_p010_planes": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _fp, _i, _i, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "vstab_warp_p010_planar": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _fp, _i, _i, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "vstab_cvt_bgr16_p010": (_i, [_vp, _sz, _i, _i, _vp, _sz, _vp, _sz, _vp]),
    "vstab_pull_frame_p010": (_i, [_vp, _vp, _sz, _vp, _sz]),
    "vstab_pull_frames": (_i, [_vp, _i, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _i, _i, _c.POINTER(_c.c_int)]),
    "vstab_pull_frame_nv12": (_i, [_vp, _vp, _sz, _vp, _sz]),
    "vstab_pull_frame_nv12_planar": (_i, [_vp, _vp, _sz, _vp, _sz]),
    "vstab_pull_frame_p010_planar": (_i, [_vp, _vp, _sz, _vp, _sz]),
    "vstab_pull_frame_host": (_i, [_vp, _vp, _sz]),
    "vstab_lens_camera": (_i, [_i, _d, _i, _i, _d, _d, _dp]),
    "vstab_peek_frame": (_i, [_vp, _vp, _sz]),
    "vstab_destroy": (None, [_vp]),
    "vstab_frame_log_count": (_i, [_vp]),
    "vstab_get_frame_log": (_i, [_vp, _i, _c.POINTER(FrameLog)]),
    "vstab_get_warp_rotation": (_i, [_vp, _i, _dp]),
    "vstab_enable_profiling": (_i, [_vp, _i]),
    "vstab_get_profile": (_i, [_vp, _c.POINTER(Profile)]),
    "vstab_ring_source_create": (_i, [_pp, _i, _i, _i, _sz, _c.c_long, _pp, _c.POINTER(Source)]),
    "vstab_ring_source_create_ex": (_i, [_c.POINTER(_vp), _i, _i, _i, _sz, _c.c_long, _i, _dp, _c.POINTER(_vp), _c.POINTER(Source)]),
    "vstab_ring_source_set_hold": (None, [_vp, _i]),
    "vstab_ring_source_destroy": (None, [_vp]),
    "vstab_cubic_weights": (_i, [_c.POINTER(_c.c_int16)]),
    "vstab_remap_cubic": (_i, [_vp, _sz, _i, _i, _i, _vp, _sz, _vp, _sz, _ip, _vp, _sz, _i, _i, _vp]),
    "vstab_warp_nv12_cubic": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _i, _i, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "vstab_lanczos4_weights": (_i, [_c.POINTER(_c.c_int16)]),
    "vstab_remap_lanczos4": (_i, [_vp, _sz, _i, _i, _i, _vp, _sz, _vp, _sz, _ip, _vp, _sz, _i, _i, _vp]),
    "vstab_warp_nv12_lanczos4": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _i, _i, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "vstab_remap_bilinear_border": (_i, [_vp, _sz, _i, _i, _i, _vp, _sz, _vp, _sz, _i, _vp, _sz, _i, _i, _vp]),
    "vstab_warp_nv12_border": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _fp, _i, _i, _i, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "vstab_set_border_mode": (_i, [_vp, _i]),
    "vstab_colour_coefficients": (_i, [_i, _i, _c.POINTER(_c.c_int32)]),
    "vstab_cvt_nv12_bgr_colour": (_i, [_vp, _sz, _vp, _sz, _i, _i, _vp, _sz, _i, _i, _vp]),
    "vstab_cvt_bgr_nv12_colour": (_i, [_vp, _sz, _i, _i, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "vstab_warp_nv12_colour": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _i, _i, _vp, _sz, _vp, _sz, _i, _i, _i, _i, _vp]),
    "vstab_set_colour": (_i, [_vp, _i, _i]),
    "vstab_colour_coefficients10": (_i, [_i, _i, _c.POINTER(_c.c_int32)]),
    "vstab_warp_p010_colour": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _fp, _i, _i, _vp, _sz, _i, _i, _i, _i, _vp]),
    "vstab_warp_p010_planes_colour": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _fp, _i, _i, _vp, _sz, _vp, _sz, _i, _i, _i, _i, _vp]),
    "vstab_cvt_p010_bgr16_colour": (_i, [_vp, _sz, _vp, _sz, _i, _i, _vp, _sz, _i, _i, _vp]),
    "vstab_cvt_bgr16_p010_colour": (_i, [_vp, _sz, _i, _i, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "vstab_set_colour10": (_i, [_vp, _i, _i]),
    "vstab_warp_p010_planar_ex": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _fp, _i, _i, _i, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "vstab_set_resample10": (_i, [_vp, _i, _i]),
    "vstab_warp_nv12_rs_ex": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _fp, _fp, _i, _i, _i, _i, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "vstab_set_readout_warp": (_i, [_vp, _i]),
    "vstab_remap_cubic_border": (_i, [_vp, _sz, _i, _i, _i, _vp, _sz, _vp, _sz, _i, _ip, _vp, _sz, _i, _i, _vp]),
    "vstab_remap_lanczos4_border": (_i, [_vp, _sz, _i, _i, _i, _vp, _sz, _vp, _sz, _i, _ip, _vp, _sz, _i, _i, _vp]),
    "vstab_warp_nv12_cubic_border": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _i, _i, _i, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "vstab_warp_nv12_lanczos4_border": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _i, _i, _i, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "vstab_set_border_mode_ex": (_i, [_vp, _i]),
    "vstab_set_input_calibration": (_i, [_vp, _dp, _dp]),
    "vstab_set_input_calibration_ex": (_i, [_vp, _dp, _dp]),
    "vstab_fisheye_undistort_points_d": (_i, [_dp, _i, _dp, _dp, _dp, _dp, _dp]),
    "vstab_estimate_rotation_d": (_i, [_fp, _fp, _i, _dp, _dp, _dp, _u64, _dp, _ip]),
    "vstab_create_map_dist": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _fp, _i, _vp]),
    "vstab_quantised_map_dist": (_i, [_vp, _i, _i, _fp, _fp, _i, _vp]),
    "vstab_warp_nv12_dist": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _fp, _i, _i, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "vstab_warp_nv12_dist_ex": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _fp, _i, _i, _i, _i, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "vstab_remap_bilinear_keep": (_i, [_vp, _sz, _i, _i, _i, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "vstab_warp_nv12_keep": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _fp, _i, _i, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "vstab_pull_frame_keep": (_i, [_vp, _vp, _sz, _vp, _sz]),
    "vstab_pull_frame_nv12_planar_keep": (_i, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz]),
    "vstab_set_input_pinhole": (_i, [_vp, _dp, _dp]),
    "vstab_undistort_points_pinhole": (_i, [_dp, _i, _dp, _dp, _dp, _dp, _dp]),
    "vstab_estimate_rotation_pinhole": (_i, [_fp, _fp, _i, _dp, _dp, _dp, _u64, _dp, _ip]),
    "vstab_create_map_pinhole": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _fp, _i, _vp]),
    "vstab_warp_nv12_pinhole": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _fp, _i, _i, _i, _i, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "vstab_good_features_mask": (_i, [_vp, _sz, _i, _i, _vp, _sz, _i, _d, _d, _i, _fp, _ip, _ip, _vp]),
    "vstab_set_detection_mask": (_i, [_vp, _vp, _sz, _i]),
    "vstab_corner_harris": (_i, [_vp, _sz, _i, _i, _d, _vp, _vp]),
    "vstab_good_features_harris": (_i, [_vp, _sz, _i, _i, _vp, _sz, _i, _d, _d, _d, _i, _fp, _ip, _ip, _vp]),
    "vstab_set_corner_response": (_i, [_vp, _i, _d]),
    "vstab_min_eig_block": (_i, [_vp, _sz, _i, _i, _i, _vp, _vp]),
    "vstab_corner_harris_block": (_i, [_vp, _sz, _i, _i, _i, _d, _vp, _vp]),
    "vstab_good_features_block": (_i, [_vp, _sz, _i, _i, _vp, _sz, _i, _d, _d, _i, _i, _d, _i, _fp, _ip, _ip, _vp]),
    "vstab_set_corner_block": (_i, [_vp, _i]),
    "vstab_min_eig_grad": (_i, [_vp, _sz, _i, _i, _i, _i, _vp, _vp]),
    "vstab_corner_harris_grad": (_i, [_vp, _sz, _i, _i, _i, _i, _d, _vp, _vp]),
    "vstab_good_features_grad": (_i, [_vp, _sz, _i, _i, _vp, _sz, _i, _d, _d, _i, _i, _i, _d, _i, _fp, _ip, _ip, _vp]),
    "vstab_set_corner_gradient": (_i, [_vp, _i]),
    "vstab_set_tracker_options": (_i, [_vp, _i, _i, _d, _d]),
    "vstab_pyr_lk_win": (_i, [_vp, _sz, _vp, _sz, _i, _i, _fp, _i, _fp, _u8p, _fp, _i, _i, _d, _d, _i, _i, _vp]),
    "vstab_set_tracker_window": (_i, [_vp, _i]),
}
for _name, (_res, _args) in SIGNATURES.items():
    _f = getattr(_L, _name)  # AttributeError here = header/library mismatch: fail loudly
    _f.restype, _f.argtypes = _res, _args
# test hook, not part of include/vstab.h (lk_segments below)
_L.vstabx_lk_segments.restype = _i
_L.vstabx_lk_segments.argtypes = [_pp, _c.POINTER(_sz), _i, _i, _fp, _i, _ip, _i, _pp, _c.POINTER(_sz), _pp, _i, _c.POINTER(_c.c_uint32),
                                  _c.POINTER(_c.c_uint32), _u8p, _vp]
_L.vstabx_lk_segments_win.restype = _i
_L.vstabx_lk_segments_win.argtypes = _L.vstabx_lk_segments.argtypes[:-1] + [_i, _vp]   # ... pyr_out, win, stream

_L.vstabx_warps_from_cache.restype = _c.c_long
_L.vstabx_warps_from_cache.argtypes = [_vp]
# test hooks of the corner detector (corners_fused and Stabilizer.detector_counters below)
_L.vstabx_corners_fused.restype = _i
_L.vstabx_corners_fused.argtypes = [_vp, _sz, _i, _i, _d, _c.c_uint, _c.c_uint, _c.POINTER(_u64), _c.POINTER(_c.c_uint), _c.POINTER(_c.c_uint), _vp]
_L.vstabx_corners_fused_mask.restype = _i
_L.vstabx_corners_fused_mask.argtypes = [_vp, _sz, _i, _i, _vp, _sz, _d, _c.c_uint, _c.c_uint, _c.POINTER(_u64), _c.POINTER(_c.c_uint), _c.POINTER(_c.c_uint), _vp]
_L.vstabx_corners_fused_harris.restype = _i
_L.vstabx_corners_fused_harris.argtypes = [_vp, _sz, _i, _i, _vp, _sz, _d, _d, _c.c_uint, _c.c_uint, _c.POINTER(_u64), _c.POINTER(_c.c_uint), _c.POINTER(_c.c_uint), _ip, _vp]
_L.vstabx_corners_fused_block.restype = _i
_L.vstabx_corners_fused_block.argtypes = [_vp, _sz, _i, _i, _vp, _sz, _d, _d, _i, _i, _c.c_uint, _c.c_uint, _c.POINTER(_u64), _c.POINTER(_c.c_uint), _c.POINTER(_c.c_uint), _ip, _vp]
_L.vstabx_corners_fused_grad.restype = _i
_L.vstabx_corners_fused_grad.argtypes = [_vp, _sz, _i, _i, _vp, _sz, _d, _d, _i, _i, _i, _c.c_uint, _c.c_uint, _c.POINTER(_u64), _c.POINTER(_c.c_uint), _c.POINTER(_c.c_uint), _ip, _vp]
_L.vstabx_select_corners.restype = _i
_L.vstabx_select_corners.argtypes = [_c.POINTER(_u64), _c.c_uint, _i, _i, _i, _d, _fp, _ip]
_L.vstabx_detector_counters.restype = _i
_L.vstabx_detector_counters.argtypes = [_vp, _c.POINTER(_c.c_long)]
_L.vstabx_tracker_counters.restype = _i
_L.vstabx_tracker_counters.argtypes = [_vp, _c.POINTER(_c.c_long)]
# test hooks of the pyramid (pack_pyr below; tests/test_pyr_paths_cpu.py calls vstabx_pyr_down_check through lib)
for _f in (_L.vstabx_pack_pyr, _L.vstabx_launch_pack_pyr):
    _f.restype, _f.argtypes = _i, [_vp, _sz, _vp, _sz, _i, _i, _vp, _vp, _sz, _vp]
_L.vstabx_pyr_down_check.restype = _i
_L.vstabx_pyr_down_check.argtypes = [_sz, _i, _i, _sz, _sz, _i]

lib = _L
ABI_VERSION = 0x56534206  # include/vstab.h: VSTAB_ABI_VERSION ("VSB" + layout version 6)
if _L.vstab_abi_version() != ABI_VERSION:
    raise ImportError(f"video-annotator_amd: this binding mirrors ABI version {ABI_VERSION}, libvstab.so is version {_L.vstab_abi_version()}")
for _k, _t in enumerate((Frame, Source, Config, FrameLog, Profile)):  # the ctypes mirrors must match the compiled structs
    if _L.vstab_struct_size(_k) != _c.sizeof(_t):
        raise ImportError(f"video-annotator_amd: ctypes mirror of {_t.__name__} is {_c.sizeof(_t)} bytes, libvstab.so has {_L.vstab_struct_size(_k)}")


class VstabError(RuntimeError):
    def __init__(self, status, where):
        self.status = status
        super().__init__(f"{where}: status {status}: {_L.vstab_last_error().decode()}")


def _check(st, where):
    if st != OK:
        raise VstabError(st, where)


def _stream():
    import torch
    return _vp(torch.cuda.current_stream().cuda_stream)


def _dptr(a):
    return a.ctypes.data_as(_dp)


def _fptr(a):
    return a.ctypes.data_as(_fp)


def version():
    return _L.vstab_version().decode()


def device_count():
    return _L.vstab_device_count()


# ---------------------------------------------------------------------------------------------
# cameras (host)
# ---------------------------------------------------------------------------------------------
def get_preset_camera(preset, width, height):
    K = np.zeros(9)
    _check(_L.vstab_get_preset_camera(preset, width, height, _dptr(K)), "vstab_get_preset_camera")
    return K.reshape(3, 3)


def get_output_camera(K_in, width, height, scale=1.0, crop_borders=False, zoom=1.0):
    Ki = np.ascontiguousarray(K_in, np.float64).reshape(9)
    Ko = np.zeros(9)
    ow, oh = _c.c_int(), _c.c_int()
    _check(_L.vstab_get_output_camera(_dptr(Ki), width, height, scale, int(crop_borders), zoom, _dptr(Ko),
                                      _c.byref(ow), _c.byref(oh)), "vstab_get_output_camera")
    return Ko.reshape(3, 3), (ow.value, oh.value)


def lens_camera(projection, dfov_deg, width, height, cx=-1.0, cy=-1.0):
    K = np.zeros(9)
    _check(_L.vstab_lens_camera(int(projection), float(dfov_deg), width, height, cx, cy, _dptr(K)), "vstab_lens_camera")
    return K.reshape(3, 3)


def fisheye_undistort_points(pts, K, R=None, P=None, D=None):
    """D: k1..k4 of the lens (vstab_fisheye_undistort_points_d), None = the ideal equidistant lens."""
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 2)
    Kc = np.ascontiguousarray(K, np.float64).reshape(9)
    Rc = None if R is None else np.ascontiguousarray(R, np.float64).reshape(9)
    Pc = None if P is None else np.ascontiguousarray(P, np.float64).reshape(9)
    out = np.zeros_like(p)
    if D is not None:
        Dc = np.ascontiguousarray(D, np.float64).reshape(4)
        _check(_L.vstab_fisheye_undistort_points_d(_dptr(p), p.shape[0], _dptr(Kc), _dptr(Dc), None if Rc is None else _dptr(Rc),
                                                   None if Pc is None else _dptr(Pc), _dptr(out)), "vstab_fisheye_undistort_points_d")
        return out
    _check(_L.vstab_fisheye_undistort_points(_dptr(p), p.shape[0], _dptr(Kc), None if Rc is None else _dptr(Rc),
                                             None if Pc is None else _dptr(Pc), _dptr(out)),
           "vstab_fisheye_undistort_points")
    return out


def undistort_points_pinhole(pts, K, D, R=None, P=None):
    """vstab_undistort_points_pinhole: cv::undistortPoints of a rectilinear lens with D = (k1, k2, p1, p2, k3) -> (n, 2) float64."""
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 2)
    Kc, Dc = np.ascontiguousarray(K, np.float64).reshape(9), np.ascontiguousarray(D, np.float64).reshape(5)
    Rc = None if R is None else np.ascontiguousarray(R, np.float64).reshape(9)
    Pc = None if P is None else np.ascontiguousarray(P, np.float64).reshape(9)
    out = np.zeros_like(p)
    _check(_L.vstab_undistort_points_pinhole(_dptr(p), p.shape[0], _dptr(Kc), _dptr(Dc), None if Rc is None else _dptr(Rc),
                                             None if Pc is None else _dptr(Pc), _dptr(out)), "vstab_undistort_points_pinhole")
    return out


def map_params(K_in, K_out, R):
    a = np.ascontiguousarray(K_in, np.float64).reshape(9)
    b = np.ascontiguousarray(K_out, np.float64).reshape(9)
    c = np.ascontiguousarray(R, np.float64).reshape(9)
    p = np.zeros(17, np.float32)
    _L.vstab_map_params(_dptr(a), _dptr(b), _dptr(c), _fptr(p))
    return p


# ---------------------------------------------------------------------------------------------
# stateless device operators (torch CUDA tensors in / out)
# ---------------------------------------------------------------------------------------------
def _planes(nv12):
    """(h*3/2, w) packed NV12 tensor (any row stride) -> y ptr, uv ptr, pitch, w, h."""
    rows, w = nv12.shape
    assert nv12.stride(1) == 1
    h = rows * 2 // 3
    pitch = nv12.stride(0)
    return nv12.data_ptr(), nv12.data_ptr() + h * pitch, pitch, w, h


def pack_nv12(y, uv):
    """y: (h, >=w) view with row stride = pitch; uv: (h/2, >=w) view."""
    import torch
    h, w = y.shape
    dst = torch.empty((h * 3 // 2, w), dtype=torch.uint8, device=y.device)
    _check(_L.vstab_pack_nv12(y.data_ptr(), y.stride(0), uv.data_ptr(), uv.stride(0), w, h, dst.data_ptr(),
                              _stream()), "vstab_pack_nv12")
    return dst


def pack_p010(y16, uv16):
    """y16: (h, >=w) uint16/int16 view of the luma plane, uv16: (h/2, >=w) view of the interleaved chroma plane
    (P010: significant bits at the top) -> packed 8-bit NV12 (h*3/2, w)."""
    import torch
    h, w = y16.shape
    dst = torch.empty((h * 3 // 2, w), dtype=torch.uint8, device=y16.device)
    _check(_L.vstab_pack_p010(y16.data_ptr(), y16.stride(0) * 2, uv16.data_ptr(), uv16.stride(0) * 2, w, h, dst.data_ptr(),
                              _stream()), "vstab_pack_p010")
    return dst


def cvt_nv12_bgr(nv12, out=None):
    import torch
    yp, uvp, pitch, w, h = _planes(nv12)
    if out is None:
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=nv12.device)
    _check(_L.vstab_cvt_nv12_bgr(yp, pitch, uvp, pitch, w, h, out.data_ptr(), out.stride(0), _stream()),
           "vstab_cvt_nv12_bgr")
    return out


def colour_coefficients(matrix, range_):
    """vstab_colour_coefficients: CY, CUB, CUG, CVG, CVR, yoff, CRY, CGY, CBY, CRU, CGU, CBU, CGV, CBV of a spec (host only) -> int32 array of 14."""
    out = np.zeros(14, np.int32)
    _check(_L.vstab_colour_coefficients(int(matrix), int(range_), out.ctypes.data_as(_c.POINTER(_c.c_int32))), "vstab_colour_coefficients")
    return out


def colour_coefficients10(matrix, range_):
    """vstab_colour_coefficients10: the same 14 integers of a spec's row in the 10-bit table (host only) -> int32 array of 14."""
    out = np.zeros(14, np.int32)
    _check(_L.vstab_colour_coefficients10(int(matrix), int(range_), out.ctypes.data_as(_c.POINTER(_c.c_int32))), "vstab_colour_coefficients10")
    return out


def cvt_nv12_bgr_colour(nv12, matrix, range_, out=None):
    """vstab_cvt_nv12_bgr_colour: cvt_nv12_bgr with a colour spec."""
    import torch
    yp, uvp, pitch, w, h = _planes(nv12)
    if out is None:
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=nv12.device)
    _check(_L.vstab_cvt_nv12_bgr_colour(yp, pitch, uvp, pitch, w, h, out.data_ptr(), out.stride(0), int(matrix), int(range_), _stream()),
           "vstab_cvt_nv12_bgr_colour")
    return out


def cvt_bgr_nv12_colour(bgr, matrix, range_, out=None):
    """vstab_cvt_bgr_nv12_colour: (h, w, 3) BGR, even sizes -> packed NV12 (h*3/2, w) with the spec's inverse."""
    import torch
    h, w, _ = bgr.shape
    if out is None:
        out = torch.empty((h * 3 // 2, w), dtype=torch.uint8, device=bgr.device)
    yp, uvp, pitch, _, _ = _planes(out)
    _check(_L.vstab_cvt_bgr_nv12_colour(bgr.data_ptr(), bgr.stride(0), w, h, yp, pitch, uvp, pitch, int(matrix), int(range_), _stream()),
           "vstab_cvt_bgr_nv12_colour")
    return out


def warp_nv12_colour(nv12, params, dw, dh, matrix, range_, mode=MAP_CREATEMAP_CL, out_format=OUT_BGR8, out=None):
    """vstab_warp_nv12_colour: warp_nv12 with a colour spec.  OUT_BGR8 -> (dh, dw, 3) tensor; OUT_NV12 -> (luma, chroma) tensors."""
    import torch
    yp, uvp, pitch, w, h = _planes(nv12)
    if out_format == OUT_BGR8:
        if out is None:
            out = torch.empty((dh, dw, 3), dtype=torch.uint8, device=nv12.device)
        planes = (out.data_ptr(), out.stride(0), None, 0)
    else:
        yo, co = out = tuple(out) if out is not None else nv12_out_planes(dw, dh, nv12.device)
        planes = (yo.data_ptr(), yo.stride(0), co.data_ptr(), co.stride(0))
    _check(_L.vstab_warp_nv12_colour(yp, pitch, uvp, pitch, w, h, _fptr(_f32(params)), int(mode), int(out_format), *planes, dw, dh, int(matrix), int(range_),
                                     _stream()), "vstab_warp_nv12_colour")
    return out


def create_map(params, cols, rows, device="cuda", mode=MAP_CREATEMAP_CL):
    import torch
    p = np.ascontiguousarray(params, np.float32)
    mx = torch.empty((rows, cols), dtype=torch.float32, device=device)
    my = torch.empty((rows, cols), dtype=torch.float32, device=device)
    if mode == MAP_CREATEMAP_CL:
        _check(_L.vstab_create_map(mx.data_ptr(), mx.stride(0) * 4, my.data_ptr(), my.stride(0) * 4, cols, rows,
                                   _fptr(p), _stream()), "vstab_create_map")
    else:
        _check(_L.vstab_create_map_ex(mx.data_ptr(), mx.stride(0) * 4, my.data_ptr(), my.stride(0) * 4, cols, rows,
                                      _fptr(p), int(mode), _stream()), "vstab_create_map_ex")
    return mx, my


def create_map_dist(params, dist, cols, rows, mode=MAP_FISH_TO_RECT, device="cuda"):
    """vstab_create_map_dist: the map planes of mode 1 / 2 with the input lens's k1..k4."""
    import torch
    p, d = np.ascontiguousarray(params, np.float32), np.ascontiguousarray(dist, np.float32).reshape(4)
    mx = torch.empty((rows, cols), dtype=torch.float32, device=device)
    my = torch.empty((rows, cols), dtype=torch.float32, device=device)
    _check(_L.vstab_create_map_dist(mx.data_ptr(), mx.stride(0) * 4, my.data_ptr(), my.stride(0) * 4, cols, rows, _fptr(p), _fptr(d), int(mode),
                                    _stream()), "vstab_create_map_dist")
    return mx, my


def create_map_pinhole(params, dist, cols, rows, mode=MAP_RECT_TO_RECT, device="cuda"):
    """vstab_create_map_pinhole: the map planes of mode 3 / 4 with the rectilinear input lens's (k1, k2, p1, p2, k3)."""
    import torch
    p, d = np.ascontiguousarray(params, np.float32), np.ascontiguousarray(dist, np.float32).reshape(5)
    mx = torch.empty((rows, cols), dtype=torch.float32, device=device)
    my = torch.empty((rows, cols), dtype=torch.float32, device=device)
    _check(_L.vstab_create_map_pinhole(mx.data_ptr(), mx.stride(0) * 4, my.data_ptr(), my.stride(0) * 4, cols, rows, _fptr(p), _fptr(d), int(mode),
                                       _stream()), "vstab_create_map_pinhole")
    return mx, my


def remap_bilinear(src, mapx, mapy):
    import torch
    cn = 1 if src.dim() == 2 else src.shape[2]
    sh, sw = src.shape[0], src.shape[1]
    dh, dw = mapx.shape
    shape = (dh, dw) if src.dim() == 2 else (dh, dw, cn)
    out = torch.empty(shape, dtype=torch.uint8, device=src.device)
    _check(_L.vstab_remap_bilinear(src.data_ptr(), src.stride(0), sw, sh, cn, mapx.data_ptr(), mapx.stride(0) * 4,
                                   mapy.data_ptr(), mapy.stride(0) * 4, out.data_ptr(), out.stride(0), dw, dh,
                                   _stream()), "vstab_remap_bilinear")
    return out


def cubic_weights():
    """vstab_cubic_weights: the INTER_CUBIC fixed-point table the kernels use -> (1024, 4, 4) int16, entry fy * 32 + fx."""
    w = np.zeros(1024 * 16, np.int16)
    _check(_L.vstab_cubic_weights(w.ctypes.data_as(_c.POINTER(_c.c_int16))), "vstab_cubic_weights")
    return w.reshape(1024, 4, 4)


def remap_cubic(src, mapx, mapy, border=(0, 0, 0), out=None):
    """vstab_remap_cubic: cv::remap(INTER_CUBIC, BORDER_CONSTANT border).  src: (h, w) or (h, w, cn) uint8 CUDA tensor, cn 1..3;
    mapx / mapy: (dh, dw) float32 CUDA tensors."""
    import torch
    cn = 1 if src.dim() == 2 else src.shape[2]
    sh, sw = src.shape[0], src.shape[1]
    dh, dw = mapx.shape
    if out is None:
        out = torch.empty((dh, dw) if src.dim() == 2 else (dh, dw, cn), dtype=torch.uint8, device=src.device)
    b = (_i * 3)(*(list(border) + [0, 0, 0])[:3])
    _check(_L.vstab_remap_cubic(src.data_ptr(), src.stride(0), sw, sh, cn, mapx.data_ptr(), mapx.stride(0) * 4, mapy.data_ptr(), mapy.stride(0) * 4,
                                b, out.data_ptr(), out.stride(0), dw, dh, _stream()), "vstab_remap_cubic")
    return out


def warp_nv12_cubic(nv12, params, dw, dh, mode=MAP_CREATEMAP_CL, out_format=OUT_BGR8, out=None):
    """vstab_warp_nv12_cubic: the warp with INTER_CUBIC.  OUT_BGR8 -> (dh, dw, 3) tensor; OUT_NV12_PLANAR -> (luma, chroma) tensors."""
    return _warp_nv12(_L.vstab_warp_nv12_cubic, nv12, dw, dh, out_format, out, (_f32(params), int(mode)))


def lanczos4_weights():
    """vstab_lanczos4_weights: the INTER_LANCZOS4 fixed-point table the kernels use -> (1024, 8, 8) int16, entry fy * 32 + fx."""
    w = np.zeros(1024 * 64, np.int16)
    _check(_L.vstab_lanczos4_weights(w.ctypes.data_as(_c.POINTER(_c.c_int16))), "vstab_lanczos4_weights")
    return w.reshape(1024, 8, 8)


def remap_lanczos4(src, mapx, mapy, border=(0, 0, 0), out=None):
    """vstab_remap_lanczos4: cv::remap(INTER_LANCZOS4, BORDER_CONSTANT border).  Arguments as remap_cubic."""
    import torch
    cn = 1 if src.dim() == 2 else src.shape[2]
    sh, sw = src.shape[0], src.shape[1]
    dh, dw = mapx.shape
    if out is None:
        out = torch.empty((dh, dw) if src.dim() == 2 else (dh, dw, cn), dtype=torch.uint8, device=src.device)
    b = (_i * 3)(*(list(border) + [0, 0, 0])[:3])
    _check(_L.vstab_remap_lanczos4(src.data_ptr(), src.stride(0), sw, sh, cn, mapx.data_ptr(), mapx.stride(0) * 4, mapy.data_ptr(), mapy.stride(0) * 4,
                                   b, out.data_ptr(), out.stride(0), dw, dh, _stream()), "vstab_remap_lanczos4")
    return out


def warp_nv12_lanczos4(nv12, params, dw, dh, mode=MAP_CREATEMAP_CL, out_format=OUT_BGR8, out=None):
    """vstab_warp_nv12_lanczos4: the warp with INTER_LANCZOS4.  OUT_BGR8 -> (dh, dw, 3) tensor; OUT_NV12_PLANAR -> (luma, chroma) tensors."""
    return _warp_nv12(_L.vstab_warp_nv12_lanczos4, nv12, dw, dh, out_format, out, (_f32(params), int(mode)))


def warp_nv12_bgr(nv12, params, dw, dh, out=None):
    import torch
    yp, uvp, pitch, w, h = _planes(nv12)
    p = np.ascontiguousarray(params, np.float32)
    if out is None:
        out = torch.empty((dh, dw, 3), dtype=torch.uint8, device=nv12.device)
    _check(_L.vstab_warp_nv12_bgr(yp, pitch, uvp, pitch, w, h, _fptr(p), out.data_ptr(), out.stride(0), dw, dh,
                                  _stream()), "vstab_warp_nv12_bgr")
    return out


def warp_nv12_nearest(nv12, params, dw, dh, out=None, mode=None):
    """vstab_warp_nv12_nearest(_ex): the fused warp with cv::remap's INTER_NEAREST."""
    import torch
    yp, uvp, pitch, w, h = _planes(nv12)
    p = np.ascontiguousarray(params, np.float32)
    if out is None:
        out = torch.empty((dh, dw, 3), dtype=torch.uint8, device=nv12.device)
    if mode is None:
        _check(_L.vstab_warp_nv12_nearest(yp, pitch, uvp, pitch, w, h, _fptr(p), out.data_ptr(), out.stride(0), dw, dh, _stream()), "vstab_warp_nv12_nearest")
    else:
        _check(_L.vstab_warp_nv12_nearest_ex(yp, pitch, uvp, pitch, w, h, _fptr(p), int(mode), out.data_ptr(), out.stride(0), dw, dh, _stream()),
               "vstab_warp_nv12_nearest_ex")
    return out


def nv12_out_planes(dw, dh, device="cuda"):
    """Output planes for OUT_NV12: luma (dh, dw) and interleaved chroma (ceil(dh/2), 2*ceil(dw/2))."""
    import torch
    return (torch.empty((dh, dw), dtype=torch.uint8, device=device),
            torch.empty(((dh + 1) // 2, 2 * ((dw + 1) // 2)), dtype=torch.uint8, device=device))


def _f32(a, n=None):
    """A float32 array for _fptr (n: its length), or None for None."""
    return None if a is None else np.ascontiguousarray(a, np.float32).reshape(-1 if n is None else n)


def _warp_nv12(fn, nv12, dw, dh, out_format, out, head, tail=()):
    """The body of every warp_nv12* wrapper: fn(the source planes, *head, out_format, *tail, the output planes, dw, dh, the stream).  head and
    tail: the middle of the C argument list, float32 arrays in it passed by pointer (None: a null pointer).  OUT_BGR8 -> the (dh, dw, 3) tensor;
    the other formats -> the (luma, chroma) tensors.  out: the caller's tensor / pair, default new ones."""
    import torch
    yp, uvp, pitch, w, h = _planes(nv12)
    if out_format == OUT_BGR8:
        if out is None:
            out = torch.empty((dh, dw, 3), dtype=torch.uint8, device=nv12.device)
        planes = (out.data_ptr(), out.stride(0), None, 0)
    else:
        if out is None:
            out = nv12_out_planes(dw, dh, nv12.device)
        yo, co = out
        out = yo, co
        planes = (yo.data_ptr(), yo.stride(0), co.data_ptr(), co.stride(0))
    head, tail = ([_fptr(a) if isinstance(a, np.ndarray) else a for a in part] for part in (head, tail))
    _check(fn(yp, pitch, uvp, pitch, w, h, *head, int(out_format), *tail, *planes, dw, dh, _stream()), fn.__name__)
    return out


def warp_nv12(nv12, params, dw, dh, mode=MAP_CREATEMAP_CL, out_format=OUT_BGR8, out=None):
    """vstab_warp_nv12_ex.  OUT_BGR8 -> (dh, dw, 3) tensor; OUT_NV12 -> (luma, chroma) tensors."""
    return _warp_nv12(_L.vstab_warp_nv12_ex, nv12, dw, dh, out_format, out, (_f32(params), int(mode)))


def warp_nv12_dist(nv12, params, dist, dw, dh, mode=MAP_FISH_TO_RECT, out_format=OUT_BGR8, out=None):
    """vstab_warp_nv12_dist: warp_nv12 in mode 1 / 2 with the input lens's k1..k4.  OUT_BGR8 -> (dh, dw, 3) tensor; OUT_NV12_PLANAR ->
    (luma, chroma) tensors."""
    return _warp_nv12(_L.vstab_warp_nv12_dist, nv12, dw, dh, out_format, out, (_f32(params), _f32(dist, 4), int(mode)))


def warp_nv12_dist_ex(nv12, params, dist, dw, dh, mode=MAP_FISH_TO_RECT, resample=RESAMPLE_DEFAULT, border_mode=BORDER_CONSTANT, out_format=OUT_BGR8,
                      out=None):
    """vstab_warp_nv12_dist_ex: warp_nv12_dist with a resampler (RESAMPLE_DEFAULT, _CUBIC, _LANCZOS4) and a border mode (BORDER_*).  OUT_BGR8 ->
    (dh, dw, 3) tensor; OUT_NV12_PLANAR -> (luma, chroma) tensors."""
    return _warp_nv12(_L.vstab_warp_nv12_dist_ex, nv12, dw, dh, out_format, out, (_f32(params), _f32(dist, 4), int(mode), int(resample), int(border_mode)))


def warp_nv12_pinhole(nv12, params, dist, dw, dh, mode=MAP_RECT_TO_RECT, resample=RESAMPLE_DEFAULT, border_mode=BORDER_CONSTANT, out_format=OUT_BGR8,
                      out=None):
    """vstab_warp_nv12_pinhole: the warp through a rectilinear lens with dist = (k1, k2, p1, p2, k3), map mode 3 / 4, with a resampler
    (RESAMPLE_DEFAULT, _CUBIC, _LANCZOS4) and a border mode (BORDER_*).  OUT_BGR8 -> (dh, dw, 3) tensor; OUT_NV12_PLANAR -> (luma, chroma)."""
    return _warp_nv12(_L.vstab_warp_nv12_pinhole, nv12, dw, dh, out_format, out, (_f32(params), _f32(dist, 5), int(mode), int(resample), int(border_mode)))


def warp_nv12_rs_ex(nv12, params, dw, dh, rot_bottom=None, dist=None, mode=MAP_CREATEMAP_CL, resample=RESAMPLE_DEFAULT, border_mode=BORDER_CONSTANT,
                    out_format=OUT_BGR8, out=None):
    """vstab_warp_nv12_rs_ex: the 8-bit warp with a rotation per output row (rot_bottom, 9 floats or None), a calibrated lens (dist, k1..k4 or
    None), a resampler (RESAMPLE_*) and a border mode (BORDER_*).  OUT_BGR8 -> (dh, dw, 3) tensor; OUT_NV12_PLANAR -> (luma, chroma) tensors."""
    return _warp_nv12(_L.vstab_warp_nv12_rs_ex, nv12, dw, dh, out_format, out,
                      (_f32(params), _f32(rot_bottom, 9), _f32(dist, 4), int(mode), int(resample), int(border_mode)))


def remap_bilinear_border(src, mapx, mapy, border_mode=BORDER_REFLECT_101, out=None):
    """vstab_remap_bilinear_border: cv::remap(INTER_LINEAR, border_mode; BORDER_CONSTANT with value 0).  src: (h, w) or (h, w, cn) uint8 CUDA
    tensor, cn 1..3; mapx / mapy: (dh, dw) float32 CUDA tensors."""
    import torch
    cn = 1 if src.dim() == 2 else src.shape[2]
    sh, sw = src.shape[0], src.shape[1]
    dh, dw = mapx.shape
    if out is None:
        out = torch.empty((dh, dw) if src.dim() == 2 else (dh, dw, cn), dtype=torch.uint8, device=src.device)
    _check(_L.vstab_remap_bilinear_border(src.data_ptr(), src.stride(0), sw, sh, cn, mapx.data_ptr(), mapx.stride(0) * 4, mapy.data_ptr(),
                                          mapy.stride(0) * 4, int(border_mode), out.data_ptr(), out.stride(0), dw, dh, _stream()),
           "vstab_remap_bilinear_border")
    return out


def warp_nv12_border(nv12, params, dw, dh, mode=MAP_CREATEMAP_CL, out_format=OUT_BGR8, border_mode=BORDER_REFLECT_101, rot_bottom=None, out=None):
    """vstab_warp_nv12_border: the bilinear warp with a border mode (rot_bottom: vstab_warp_nv12_rs's rotation of the last output row).
    OUT_BGR8 -> (dh, dw, 3) tensor; OUT_NV12_PLANAR -> (luma, chroma) tensors."""
    return _warp_nv12(_L.vstab_warp_nv12_border, nv12, dw, dh, out_format, out, (_f32(params), _f32(rot_bottom, 9), int(mode)), (int(border_mode),))


def remap_bilinear_keep(src, mapx, mapy, prev, out=None):
    """vstab_remap_bilinear_keep: cv::remap(INTER_LINEAR) where the 2 x 2 footprint lies inside src, prev's bytes everywhere else
    (BORDER_TRANSPARENT).  src: (h, w) or (h, w, cn) uint8 CUDA tensor, cn 1..3; mapx / mapy: (dh, dw) float32 CUDA tensors; prev: the frame to
    keep, shaped as the output.  out: a tensor of its own (default: a new one), or prev itself -- in place."""
    import torch
    cn = 1 if src.dim() == 2 else src.shape[2]
    sh, sw = src.shape[0], src.shape[1]
    dh, dw = mapx.shape
    if out is None:
        out = torch.empty((dh, dw) if src.dim() == 2 else (dh, dw, cn), dtype=torch.uint8, device=src.device)
    _check(_L.vstab_remap_bilinear_keep(src.data_ptr(), src.stride(0), sw, sh, cn, mapx.data_ptr(), mapx.stride(0) * 4, mapy.data_ptr(),
                                        mapy.stride(0) * 4, prev.data_ptr(), prev.stride(0), out.data_ptr(), out.stride(0), dw, dh, _stream()),
           "vstab_remap_bilinear_keep")
    return out


def warp_nv12_keep(nv12, params, dw, dh, prev, mode=MAP_CREATEMAP_CL, out_format=OUT_BGR8, rot_bottom=None, out=None):
    """vstab_warp_nv12_keep: the bilinear warp where its footprint lies inside the source, prev's bytes everywhere else.  OUT_BGR8: prev a
    (dh, dw, 3) tensor -> (dh, dw, 3) tensor; OUT_NV12_PLANAR: prev a (luma, chroma) pair -> (luma, chroma) tensors.  out: tensors of their
    own (default: new ones), or prev itself -- in place.  rot_bottom: vstab_warp_nv12_rs's rotation of the last output row."""
    if out_format == OUT_BGR8:
        history = (prev.data_ptr(), prev.stride(0), None, 0)
    else:
        history = (prev[0].data_ptr(), prev[0].stride(0), prev[1].data_ptr(), prev[1].stride(0))
    return _warp_nv12(_L.vstab_warp_nv12_keep, nv12, dw, dh, out_format, out, (_f32(params), _f32(rot_bottom, 9), int(mode)), history)


def _remap_resample_border(fn, name, src, mapx, mapy, border_mode, border, out):
    import torch
    cn = 1 if src.dim() == 2 else src.shape[2]
    sh, sw = src.shape[0], src.shape[1]
    dh, dw = mapx.shape
    if out is None:
        out = torch.empty((dh, dw) if src.dim() == 2 else (dh, dw, cn), dtype=torch.uint8, device=src.device)
    b = (_i * 3)(*(list(border) + [0, 0, 0])[:3])
    _check(fn(src.data_ptr(), src.stride(0), sw, sh, cn, mapx.data_ptr(), mapx.stride(0) * 4, mapy.data_ptr(), mapy.stride(0) * 4, int(border_mode), b,
              out.data_ptr(), out.stride(0), dw, dh, _stream()), name)
    return out


def remap_cubic_border(src, mapx, mapy, border_mode=BORDER_REFLECT_101, border=(0, 0, 0), out=None):
    """vstab_remap_cubic_border: cv::remap(INTER_CUBIC, border_mode; border values under BORDER_CONSTANT only).  Arguments as remap_cubic."""
    return _remap_resample_border(_L.vstab_remap_cubic_border, "vstab_remap_cubic_border", src, mapx, mapy, border_mode, border, out)


def remap_lanczos4_border(src, mapx, mapy, border_mode=BORDER_REFLECT_101, border=(0, 0, 0), out=None):
    """vstab_remap_lanczos4_border: cv::remap(INTER_LANCZOS4, border_mode; border values under BORDER_CONSTANT only).  Arguments as remap_cubic."""
    return _remap_resample_border(_L.vstab_remap_lanczos4_border, "vstab_remap_lanczos4_border", src, mapx, mapy, border_mode, border, out)


def warp_nv12_cubic_border(nv12, params, dw, dh, mode=MAP_CREATEMAP_CL, out_format=OUT_BGR8, border_mode=BORDER_REFLECT_101, out=None):
    """vstab_warp_nv12_cubic_border: the INTER_CUBIC warp with a border mode.  OUT_BGR8 -> (dh, dw, 3) tensor; OUT_NV12_PLANAR -> (luma, chroma)."""
    return _warp_nv12(_L.vstab_warp_nv12_cubic_border, nv12, dw, dh, out_format, out, (_f32(params), int(mode)), (int(border_mode),))


def warp_nv12_lanczos4_border(nv12, params, dw, dh, mode=MAP_CREATEMAP_CL, out_format=OUT_BGR8, border_mode=BORDER_REFLECT_101, out=None):
    """vstab_warp_nv12_lanczos4_border: the INTER_LANCZOS4 warp with a border mode.  Arguments and results as warp_nv12_cubic_border."""
    return _warp_nv12(_L.vstab_warp_nv12_lanczos4_border, nv12, dw, dh, out_format, out, (_f32(params), int(mode)), (int(border_mode),))


def warp_nv12_rs(nv12, params, rot_bottom, dw, dh, mode=MAP_CREATEMAP_CL, out_format=OUT_BGR8, out=None):
    """vstab_warp_nv12_rs: the warp with a rotation per output row (first row params[8:17], last row rot_bottom)."""
    return _warp_nv12(_L.vstab_warp_nv12_rs, nv12, dw, dh, out_format, out, (_f32(params), _f32(rot_bottom, 9), int(mode)))


BLEND_EXACT, BLEND_FP16 = 0, 1


def warp_p010(y, uv, params, dw, dh, rot_bottom=None, mode=MAP_CREATEMAP_CL, blend=BLEND_EXACT, out=None, colour=None):
    """vstab_warp_p010 (config 5): y (h, w) / uv (h/2, w) int16-or-uint16 CUDA tensors holding P010 samples ->
    (dh, dw, 3) int16 tensor of BGR values 0..1023.  colour=(matrix, range): vstab_warp_p010_colour."""
    import torch
    h, w = y.shape
    p = np.ascontiguousarray(params, np.float32)
    rb = None if rot_bottom is None else np.ascontiguousarray(rot_bottom, np.float32).reshape(9)
    if out is None:
        out = torch.empty((dh, dw, 3), dtype=torch.int16, device=y.device)
    args = (y.data_ptr(), y.stride(0) * 2, uv.data_ptr(), uv.stride(0) * 2, w, h, _fptr(p), None if rb is None else _fptr(rb), int(mode), int(blend), out.data_ptr(),
            out.stride(0) * 2, dw, dh)
    if colour is None:
        _check(_L.vstab_warp_p010(*args, _stream()), "vstab_warp_p010")
    else:
        _check(_L.vstab_warp_p010_colour(*args, int(colour[0]), int(colour[1]), _stream()), "vstab_warp_p010_colour")
    return out


def warp_p010_planes(y, uv, params, dw, dh, rot_bottom=None, mode=MAP_CREATEMAP_CL, blend=BLEND_EXACT, out_y=None, out_uv=None, colour=None):
    """vstab_warp_p010_planes: the 10-bit warp with P010 planes out, one kernel.  Raises VstabError (ERR_UNSUPPORTED) for planes the
    tiled kernel cannot take.  colour=(matrix, range): vstab_warp_p010_planes_colour."""
    import torch
    h, w = y.shape
    p = np.ascontiguousarray(params, np.float32)
    rb = None if rot_bottom is None else np.ascontiguousarray(rot_bottom, np.float32).reshape(9)
    if out_y is None:
        out_y = torch.empty((dh, dw), dtype=torch.int16, device=y.device)
    if out_uv is None:
        out_uv = torch.empty(((dh + 1) // 2, 2 * ((dw + 1) // 2)), dtype=torch.int16, device=y.device)
    args = (y.data_ptr(), y.stride(0) * 2, uv.data_ptr(), uv.stride(0) * 2, w, h, _fptr(p), None if rb is None else _fptr(rb), int(mode), int(blend),
            out_y.data_ptr(), out_y.stride(0) * 2, out_uv.data_ptr(), out_uv.stride(0) * 2, dw, dh)
    if colour is None:
        _check(_L.vstab_warp_p010_planes(*args, _stream()), "vstab_warp_p010_planes")
    else:
        _check(_L.vstab_warp_p010_planes_colour(*args, int(colour[0]), int(colour[1]), _stream()), "vstab_warp_p010_planes_colour")
    return out_y, out_uv


def warp_p010_planar(y, uv, params, dw, dh, rot_bottom=None, mode=MAP_CREATEMAP_CL, blend=BLEND_EXACT, out_y=None, out_uv=None):
    """vstab_warp_p010_planar: the plane-wise 10-bit warp, P010 planes in and out, no colour round trip."""
    import torch
    h, w = y.shape
    p = np.ascontiguousarray(params, np.float32)
    rb = None if rot_bottom is None else np.ascontiguousarray(rot_bottom, np.float32).reshape(9)
    if out_y is None:
        out_y = torch.empty((dh, dw), dtype=torch.int16, device=y.device)
    if out_uv is None:
        out_uv = torch.empty(((dh + 1) // 2, 2 * ((dw + 1) // 2)), dtype=torch.int16, device=y.device)
    _check(_L.vstab_warp_p010_planar(y.data_ptr(), y.stride(0) * 2, uv.data_ptr(), uv.stride(0) * 2, w, h, _fptr(p), None if rb is None else _fptr(rb),
                                     int(mode), int(blend), out_y.data_ptr(), out_y.stride(0) * 2, out_uv.data_ptr(), out_uv.stride(0) * 2, dw, dh, _stream()),
           "vstab_warp_p010_planar")
    return out_y, out_uv


def warp_p010_planar_ex(y, uv, params, dw, dh, rot_bottom=None, mode=MAP_CREATEMAP_CL, resample=RESAMPLE_CUBIC, border_mode=BORDER_CONSTANT, out_y=None,
                        out_uv=None):
    """vstab_warp_p010_planar_ex: warp_p010_planar with cv::remap's INTER_CUBIC or INTER_LANCZOS4 (RESAMPLE_*) and a border mode (BORDER_*)."""
    import torch
    h, w = y.shape
    p = np.ascontiguousarray(params, np.float32)
    rb = None if rot_bottom is None else np.ascontiguousarray(rot_bottom, np.float32).reshape(9)
    if out_y is None:
        out_y = torch.empty((dh, dw), dtype=torch.int16, device=y.device)
    if out_uv is None:
        out_uv = torch.empty(((dh + 1) // 2, 2 * ((dw + 1) // 2)), dtype=torch.int16, device=y.device)
    _check(_L.vstab_warp_p010_planar_ex(y.data_ptr(), y.stride(0) * 2, uv.data_ptr(), uv.stride(0) * 2, w, h, _fptr(p), None if rb is None else _fptr(rb),
                                        int(mode), int(resample), int(border_mode), out_y.data_ptr(), out_y.stride(0) * 2, out_uv.data_ptr(),
                                        out_uv.stride(0) * 2, dw, dh, _stream()),
           "vstab_warp_p010_planar_ex")
    return out_y, out_uv


def cvt_bgr16_p010(bgr16, out_y=None, out_uv=None, colour=None):
    """vstab_cvt_bgr16_p010: (h, w, 3) int16 CUDA tensor of BGR values 0..1023 -> P010 planes (h, w) and (ceil(h/2), 2 * ceil(w/2)), int16 bit patterns.
    colour=(matrix, range): vstab_cvt_bgr16_p010_colour."""
    import torch
    h, w = bgr16.shape[:2]
    if out_y is None:
        out_y = torch.empty((h, w), dtype=torch.int16, device=bgr16.device)
    if out_uv is None:
        out_uv = torch.empty(((h + 1) // 2, 2 * ((w + 1) // 2)), dtype=torch.int16, device=bgr16.device)
    args = (bgr16.data_ptr(), bgr16.stride(0) * 2, w, h, out_y.data_ptr(), out_y.stride(0) * 2, out_uv.data_ptr(), out_uv.stride(0) * 2)
    if colour is None:
        _check(_L.vstab_cvt_bgr16_p010(*args, _stream()), "vstab_cvt_bgr16_p010")
    else:
        _check(_L.vstab_cvt_bgr16_p010_colour(*args, int(colour[0]), int(colour[1]), _stream()), "vstab_cvt_bgr16_p010_colour")
    return out_y, out_uv


def cvt_p010_bgr16(y, uv, colour=None, out=None):
    """vstab_cvt_p010_bgr16_colour: P010 planes y (h, w) / uv (h/2, w), int16 CUDA tensors -> (h, w, 3) int16 tensor of BGR values 0..1023.
    colour=(matrix, range); None: (COLOUR_CVTCOLOR, RANGE_LIMITED), the 10-bit path's own arithmetic."""
    import torch
    h, w = y.shape
    m, r = (COLOUR_CVTCOLOR, RANGE_LIMITED) if colour is None else colour
    if out is None:
        out = torch.empty((h, w, 3), dtype=torch.int16, device=y.device)
    _check(_L.vstab_cvt_p010_bgr16_colour(y.data_ptr(), y.stride(0) * 2, uv.data_ptr(), uv.stride(0) * 2, w, h, out.data_ptr(), out.stride(0) * 2, int(m), int(r),
                                          _stream()), "vstab_cvt_p010_bgr16_colour")
    return out


def time_next_launch(start_event, stop_event):
    """The next stateless warp call stamps its kernel's own start / end into the two torch.cuda.Event(enable_timing=True):
    kernel-only time, as rocprofv3's kernel trace reports it."""
    for e in (start_event, stop_event):
        if not e.cuda_event:   # torch creates the hipEvent_t lazily, at the first record
            e.record()
    _L.vstab_time_next_launch(_c.c_void_p(start_event.cuda_event), _c.c_void_p(stop_event.cuda_event))


def quantised_map(params, dw, dh, mode=MAP_CREATEMAP_CL, device="cuda"):
    """The per-pixel quantised map for a run of frames with the same warp parameters -> opaque device tensor."""
    import torch
    p = np.ascontiguousarray(params, np.float32)
    q = torch.empty(_L.vstab_quantised_map_bytes(dw, dh), dtype=torch.uint8, device=device)
    _check(_L.vstab_quantised_map(q.data_ptr(), dw, dh, _fptr(p), int(mode), _stream()), "vstab_quantised_map")
    return q


def quantised_map_dist(params, dist, dw, dh, mode=MAP_FISH_TO_RECT, device="cuda"):
    """vstab_quantised_map_dist: quantised_map of mode 1 / 2 with the input lens's k1..k4 (for warp_nv12_mapped)."""
    import torch
    p, d = np.ascontiguousarray(params, np.float32), np.ascontiguousarray(dist, np.float32).reshape(4)
    q = torch.empty(_L.vstab_quantised_map_bytes(dw, dh), dtype=torch.uint8, device=device)
    _check(_L.vstab_quantised_map_dist(q.data_ptr(), dw, dh, _fptr(p), _fptr(d), int(mode), _stream()), "vstab_quantised_map_dist")
    return q


def warp_nv12_mapped(nv12, qmap, dw, dh, out_format=OUT_BGR8, out=None):
    return _warp_nv12(_L.vstab_warp_nv12_mapped, nv12, dw, dh, out_format, out, (qmap.data_ptr(),))


def _caller_plane(out, rows, cols, device, what):
    """A plane the caller laid out for an operator to write: 2-D uint8 of (rows, cols) on `device`, unit column stride, any row stride >= cols."""
    import torch
    if (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() != 2 or tuple(out.shape) != (rows, cols) or out.device != device
            or out.stride(1) != 1 or out.stride(0) < cols):
        raise ValueError(f"{what}: out must be a ({rows}, {cols}) uint8 tensor on {device} with stride(1) == 1 and stride(0) >= {cols}")
    return out


def pyr_down(img, out=None):
    """vstab_pyr_down -> the level, in a fresh dense tensor or in `out` (a caller's plane, _caller_plane)."""
    import torch
    h, w = img.shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    out = torch.empty((dh, dw), dtype=torch.uint8, device=img.device) if out is None else _caller_plane(out, dh, dw, img.device, "pyr_down")
    _check(_L.vstab_pyr_down(img.data_ptr(), img.stride(0), w, h, out.data_ptr(), out.stride(0), _stream()), "vstab_pyr_down")
    return out


def pyr_down_x2(img, out=None):
    """vstab_pyr_down_x2: two pyramid levels in one launch -> (mid, dst), fresh dense tensors or out = (mid, dst) (caller's planes, _caller_plane)."""
    import torch
    h, w = img.shape
    mw, mh = (w + 1) // 2, (h + 1) // 2
    dw, dh = (mw + 1) // 2, (mh + 1) // 2
    if out is None:
        mid = torch.empty((mh, mw), dtype=torch.uint8, device=img.device)
        dst = torch.empty((dh, dw), dtype=torch.uint8, device=img.device)
    else:
        mid, dst = out
        _caller_plane(mid, mh, mw, img.device, "pyr_down_x2 (mid)"), _caller_plane(dst, dh, dw, img.device, "pyr_down_x2 (dst)")
    _check(_L.vstab_pyr_down_x2(img.data_ptr(), img.stride(0), w, h, mid.data_ptr(), mid.stride(0), dst.data_ptr(), dst.stride(0), _stream()), "vstab_pyr_down_x2")
    return mid, dst


def pack_pyr(y, pitch_y, uv, pitch_uv, w, h, ring, dst, dpitch, launch_anyway=False, stream=None):
    """Test hook vstabx_pack_pyr (not part of include/vstab.h): k_pack_pyr alone on raw device addresses -- the NV12 frame (y, uv) copied into
    `ring` (w * h * 3 / 2 bytes) and pyrDown of its luma written to dst (pitch dpitch).  -> -1 where pack_pyr_ok refuses the planes (nothing is
    launched), else the status of launch_pack_pyr.  launch_anyway: vstabx_launch_pack_pyr, the launcher without the question -- its own refusal.
    Addresses are taken as given, so the refusals can be asked for without a device."""
    fn = _L.vstabx_launch_pack_pyr if launch_anyway else _L.vstabx_pack_pyr
    return fn(y, pitch_y, uv, pitch_uv, int(w), int(h), ring, dst, dpitch, _stream() if stream is None else stream)


def min_eig(gray):
    import torch
    h, w = gray.shape
    out = torch.empty((h, w), dtype=torch.float32, device=gray.device)
    _check(_L.vstab_min_eig(gray.data_ptr(), gray.stride(0), w, h, out.data_ptr(), _stream()), "vstab_min_eig")
    return out


DETECTOR_AUTO, DETECTOR_TWO_PASS, DETECTOR_FUSED = 0, 1, 2


def _good_features(name, gray, max_corners, info, head, with_used=True):
    """One call shape for the vstab_good_features* entry points: fn(gray, pitch, w, h, *head, xy, &count[, &detector_used], stream);
    head is what stands between the image and xy.  info["detector_used"] is filled where the entry point reports it."""
    h, w = gray.shape
    xy = np.zeros((max_corners, 2), np.float32)
    n, used = _c.c_int(), _c.c_int()
    out = (_fptr(xy), _c.byref(n)) + ((_c.byref(used),) if with_used else ())
    _check(getattr(_L, name)(gray.data_ptr(), gray.stride(0), w, h, *head, *out, _stream()), name)
    if with_used and info is not None:
        info["detector_used"] = used.value
    return xy[:n.value].copy()


def _mask_args(mask):
    return (None, 0) if mask is None else (mask.data_ptr(), mask.stride(0))


def good_features(gray, max_corners=200, quality=0.01, min_distance=30.0, detector=None, info=None):
    """detector: None -> vstab_good_features; DETECTOR_AUTO / DETECTOR_TWO_PASS -> vstab_good_features_ex, and
    info["detector_used"] (if a dict is given) says which kernel path produced the corners."""
    if detector is None:
        return _good_features("vstab_good_features", gray, max_corners, None, (max_corners, quality, min_distance), with_used=False)
    return _good_features("vstab_good_features_ex", gray, max_corners, info, (max_corners, quality, min_distance, detector))


def good_features_mask(gray, mask, max_corners=200, quality=0.01, min_distance=30.0, detector=DETECTOR_AUTO, info=None):
    """vstab_good_features_mask: good_features under a detection mask, an (h, w) uint8 device tensor or view (any pitch and base address;
    non-zero = "a corner may be reported here"), or None for no mask.  detector: DETECTOR_AUTO, DETECTOR_FUSED or DETECTOR_TWO_PASS;
    info["detector_used"] (if a dict is given) says which kernel path produced the corners."""
    return _good_features("vstab_good_features_mask", gray, max_corners, info, _mask_args(mask) + (max_corners, quality, min_distance, detector))


CORNER_MIN_EIGENVAL, CORNER_HARRIS = 0, 1


def corner_harris(gray, k=0.04):
    """vstab_corner_harris: cornerHarris(gray, 3, 3, k) as an (h, w) float32 device map (include/vstab.h, "Harris response")"""
    import torch
    h, w = gray.shape
    out = torch.empty((h, w), dtype=torch.float32, device=gray.device)
    _check(_L.vstab_corner_harris(gray.data_ptr(), gray.stride(0), w, h, float(k), out.data_ptr(), _stream()), "vstab_corner_harris")
    return out


def good_features_harris(gray, mask=None, max_corners=200, quality=0.01, min_distance=30.0, k=0.04, detector=DETECTOR_AUTO, info=None):
    """vstab_good_features_harris: good_features_mask with the Harris response (goodFeaturesToTrack's useHarrisDetector = true and k);
    mask None = no mask."""
    return _good_features("vstab_good_features_harris", gray, max_corners, info, _mask_args(mask) + (max_corners, quality, min_distance, float(k), detector))


def min_eig_block(gray, block_size):
    """vstab_min_eig_block: cornerMinEigenVal(gray, block_size, 3) as an (h, w) float32 device map, block_size 3, 5 or 7 (include/vstab.h,
    "Corner block size"); with 3 it is min_eig"""
    import torch
    h, w = gray.shape
    out = torch.empty((h, w), dtype=torch.float32, device=gray.device)
    _check(_L.vstab_min_eig_block(gray.data_ptr(), gray.stride(0), w, h, int(block_size), out.data_ptr(), _stream()), "vstab_min_eig_block")
    return out


def corner_harris_block(gray, block_size, k=0.04):
    """vstab_corner_harris_block: cornerHarris(gray, block_size, 3, k) as an (h, w) float32 device map; with 3 it is corner_harris"""
    import torch
    h, w = gray.shape
    out = torch.empty((h, w), dtype=torch.float32, device=gray.device)
    _check(_L.vstab_corner_harris_block(gray.data_ptr(), gray.stride(0), w, h, int(block_size), float(k), out.data_ptr(), _stream()), "vstab_corner_harris_block")
    return out


def good_features_block(gray, mask=None, max_corners=200, quality=0.01, min_distance=30.0, block_size=3, use_harris=False, k=0.04, detector=DETECTOR_AUTO,
                        info=None):
    """vstab_good_features_block: goodFeaturesToTrack's whole argument list -- mask (None = no mask), blockSize (3, 5 or 7), useHarrisDetector
    and k (looked at only with use_harris)"""
    return _good_features("vstab_good_features_block", gray, max_corners, info,
                          _mask_args(mask) + (max_corners, quality, min_distance, int(block_size), int(use_harris), float(k), detector))


def min_eig_grad(gray, block_size, gradient_size):
    """vstab_min_eig_grad: cornerMinEigenVal(gray, block_size, gradient_size) as an (h, w) float32 device map, both sizes 3, 5 or 7
    (include/vstab.h, "Corner gradient size"); with gradient_size 3 it is min_eig_block"""
    import torch
    h, w = gray.shape
    out = torch.empty((h, w), dtype=torch.float32, device=gray.device)
    _check(_L.vstab_min_eig_grad(gray.data_ptr(), gray.stride(0), w, h, int(block_size), int(gradient_size), out.data_ptr(), _stream()), "vstab_min_eig_grad")
    return out


def corner_harris_grad(gray, block_size, gradient_size, k=0.04):
    """vstab_corner_harris_grad: cornerHarris(gray, block_size, gradient_size, k) as an (h, w) float32 device map; with gradient_size 3 it
    is corner_harris_block"""
    import torch
    h, w = gray.shape
    out = torch.empty((h, w), dtype=torch.float32, device=gray.device)
    _check(_L.vstab_corner_harris_grad(gray.data_ptr(), gray.stride(0), w, h, int(block_size), int(gradient_size), float(k), out.data_ptr(), _stream()),
           "vstab_corner_harris_grad")
    return out


def good_features_grad(gray, mask=None, max_corners=200, quality=0.01, min_distance=30.0, block_size=3, gradient_size=3, use_harris=False, k=0.04,
                       detector=DETECTOR_AUTO, info=None):
    """vstab_good_features_grad: goodFeaturesToTrack's ten-argument overload -- good_features_block with gradientSize (3, 5 or 7) behind
    blockSize"""
    return _good_features("vstab_good_features_grad", gray, max_corners, info,
                          _mask_args(mask) + (max_corners, quality, min_distance, int(block_size), int(gradient_size), int(use_harris), float(k), detector))


CORNERS_FUSED_FILL = 0xA5A5A5A5A5A5A5A5  # what vstabx_corners_fused fills its key buffer with before the kernels run


def _corners_fused(name, gray, w, h, stream, cap, canary, head, tail=()):
    """One buffer set-up and call shape for the vstabx_corners_fused* hooks: fn(gray, pitch, w, h, *head, cap, canary, keys, counts,
    tiles, *tail, stream) -> (keys, keys kept, tiles that spilled, per-tile survivor counts).  w / h / stream are taken as given."""
    h = gray.shape[0] if h is None else h
    w = gray.shape[1] if w is None else w
    cap, canary = int(cap), int(canary)
    ok = 0 < cap <= 1 << 24 and 0 < canary <= 1 << 16    # (the library refuses the rest: nothing is allocated for them here)
    keys = np.zeros(cap + canary if ok else 1, np.uint64)
    counts = np.zeros(2, np.uint32)
    tx, ty = max(1, (int(w) + 63) // 64), max(1, (int(h) + 30) // 31)
    tiles = np.zeros((ty, tx) if tx * ty < 1 << 21 else (1, 1), np.uint32)   # (2^21 tiles are over 2^31 pixels: refused)
    _check(getattr(_L, name)(gray.data_ptr(), gray.stride(0), int(w), int(h), *head, cap & 0xFFFFFFFF, canary & 0xFFFFFFFF,
                             keys.ctypes.data_as(_c.POINTER(_u64)), counts.ctypes.data_as(_c.POINTER(_c.c_uint)),
                             tiles.ctypes.data_as(_c.POINTER(_c.c_uint)), *tail, _stream() if stream is None else stream), name)
    return keys, int(counts[0]), int(counts[1]), tiles


def corners_fused(gray, quality=0.01, cap=1 << 18, canary=64, w=None, h=None, stream=None):
    """Test hook vstabx_corners_fused (not part of include/vstab.h): the one-pass detector's raw output on the (h, w) uint8 device luma
    view `gray` (pitched views allowed) with a key buffer of exactly `cap` keys and `canary` more behind it.
    -> (keys (cap + canary,) uint64 as the kernels left them over the fill, keys kept, tiles that spilled, per-tile survivor counts
    (tiles_y, tiles_x) uint32).  w / h / stream are taken as given, so that a test of the refusals needs no device."""
    return _corners_fused("vstabx_corners_fused", gray, w, h, stream, cap, canary, (float(quality),))


def corners_fused_mask(gray, mask, quality=0.01, cap=1 << 18, canary=64, w=None, h=None, stream=None, mask_ptr=None, mask_pitch=None):
    """Test hook vstabx_corners_fused_mask: corners_fused under the detection mask `mask`, an (h, w) uint8 device tensor or view; the same
    outputs.  mask_ptr / mask_pitch (for a test of the refusals, which needs no device) stand in for the tensor's."""
    mp = mask.data_ptr() if mask_ptr is None else mask_ptr
    mpitch = mask.stride(0) if mask_pitch is None else mask_pitch
    return _corners_fused("vstabx_corners_fused_mask", gray, w, h, stream, cap, canary, (mp, mpitch, float(quality)))


def corners_fused_harris(gray, mask=None, k=0.04, quality=0.01, cap=1 << 18, canary=64, w=None, h=None, stream=None):
    """Test hook vstabx_corners_fused_harris: corners_fused / corners_fused_mask (mask None = no mask) with the Harris response.
    -> (keys, keys kept, tiles that spilled, per-tile survivor counts, max_bits): max_bits is the frame maximum the kernels published, the
    float's bits as int32 -- negative: no response above zero, the host reports no corner whatever the keys say."""
    mx = _c.c_int()
    out = _corners_fused("vstabx_corners_fused_harris", gray, w, h, stream, cap, canary, _mask_args(mask) + (float(quality), float(k)), (_c.byref(mx),))
    return out + (mx.value,)


def corners_fused_block(gray, mask=None, block_size=3, response=CORNER_MIN_EIGENVAL, k=0.04, quality=0.01, cap=1 << 18, canary=64, w=None, h=None, stream=None):
    """Test hook vstabx_corners_fused_block: corners_fused_harris with the block size (3, 5 or 7) and the response (CORNER_MIN_EIGENVAL: k
    is not looked at; CORNER_HARRIS) as arguments; the same five outputs."""
    mx = _c.c_int()
    out = _corners_fused("vstabx_corners_fused_block", gray, w, h, stream, cap, canary,
                         _mask_args(mask) + (float(quality), float(k), int(block_size), int(response)), (_c.byref(mx),))
    return out + (mx.value,)


def corners_fused_grad(gray, mask=None, block_size=3, gradient_size=3, response=CORNER_MIN_EIGENVAL, k=0.04, quality=0.01, cap=1 << 18, canary=64, w=None, h=None,
                       stream=None):
    """Test hook vstabx_corners_fused_grad: corners_fused_block with the gradient size (3, 5 or 7) behind the block size; the same five
    outputs."""
    mx = _c.c_int()
    out = _corners_fused("vstabx_corners_fused_grad", gray, w, h, stream, cap, canary,
                         _mask_args(mask) + (float(quality), float(k), int(block_size), int(gradient_size), int(response)), (_c.byref(mx),))
    return out + (mx.value,)


def select_corners(keys, w, h, max_corners=200, min_distance=30.0):
    """Test hook vstabx_select_corners (no device needed): the host half of goodFeaturesToTrack over candidate keys (uint64: float bits
    << 32 | raster index) of a w x h image -> (n, 2) float32 corners in the order they were accepted.  max_corners <= 0: no limit."""
    keys = np.ascontiguousarray(keys, np.uint64)
    xy = np.zeros((max(1, keys.size if max_corners <= 0 else min(keys.size, max_corners)), 2), np.float32)
    n = _c.c_int()
    _check(_L.vstabx_select_corners(keys.ctypes.data_as(_c.POINTER(_u64)), keys.size, int(w), int(h), int(max_corners), float(min_distance), _fptr(xy),
                                    _c.byref(n)), "vstabx_select_corners")
    return xy[:n.value].copy()


def pyr_lk(prev, nxt, pts):
    h, w = prev.shape
    p = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    n = p.shape[0]
    out = np.zeros((n, 2), np.float32)
    st = np.zeros(n, np.uint8)
    _check(_L.vstab_pyr_lk(prev.data_ptr(), prev.stride(0), nxt.data_ptr(), nxt.stride(0), w, h, _fptr(p), n, _fptr(out),
                           st.ctypes.data_as(_u8p), _stream()), "vstab_pyr_lk")
    return out, st


LK_USE_INITIAL_FLOW, LK_GET_MIN_EIGENVALS = 4, 8   # calcOpticalFlowPyrLK's flags (OpenCV's values)


def _pyr_lk_with_options(name, tail, prev, nxt, pts, max_level, max_iter, eps, min_eig_threshold, flags, guess, want_err):
    """the call of vstab_pyr_lk_ex and vstab_pyr_lk_win: `tail` is what stands between flags and the stream"""
    h, w = prev.shape
    p = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    n = p.shape[0]
    out = np.zeros((n, 2), np.float32)
    if guess is not None:
        out[:] = np.asarray(guess, np.float32).reshape(-1, 2)
    st = np.zeros(n, np.uint8)
    err = np.zeros(n, np.float32) if want_err else None
    _check(getattr(_L, name)(prev.data_ptr(), prev.stride(0), nxt.data_ptr(), nxt.stride(0), w, h, _fptr(p), n, _fptr(out), st.ctypes.data_as(_u8p),
                             _fptr(err) if want_err else None, int(max_level), int(max_iter), float(eps), float(min_eig_threshold), int(flags), *tail,
                             _stream()), name)
    return out, st, err


def pyr_lk_ex(prev, nxt, pts, max_level=3, max_iter=30, eps=0.01, min_eig_threshold=1e-4, flags=0, guess=None, want_err=True):
    """vstab_pyr_lk_ex (include/vstab.h, "Tracker options"): calcOpticalFlowPyrLK with maxLevel, the criteria's count and epsilon,
    minEigThreshold, flags and err; winSize is 21 x 21 (pyr_lk_win takes another).  guess: the n start positions in the next image, read
    with LK_USE_INITIAL_FLOW (any float).  -> (next points (n, 2) float32, status (n,) uint8, err (n,) float32 or None without want_err)."""
    return _pyr_lk_with_options("vstab_pyr_lk_ex", (), prev, nxt, pts, max_level, max_iter, eps, min_eig_threshold, flags, guess, want_err)


def pyr_lk_win(prev, nxt, pts, win_size, max_level=3, max_iter=30, eps=0.01, min_eig_threshold=1e-4, flags=0, guess=None, want_err=True):
    """vstab_pyr_lk_win (include/vstab.h, "Tracker window"): pyr_lk_ex with calcOpticalFlowPyrLK's winSize, win_size x win_size for 15, 21
    or 31; with 21 it is pyr_lk_ex."""
    return _pyr_lk_with_options("vstab_pyr_lk_win", (int(win_size),), prev, nxt, pts, max_level, max_iter, eps, min_eig_threshold, flags, guess, want_err)


def lk_segments(frames, pts, segs, uv=None, rings=None, bad_parent=-1, want_pyr=False, w=None, h=None, stream=None, win=21):
    """Test hook vstabx_lk_segments (not part of include/vstab.h): the K + 1 (h, w) uint8 device luma views `frames` (pitched views
    allowed), n start points, launches of segs[s] frame pairs each (sum K), the first from pts and every later one chained behind the
    one before.  uv / rings (K + 1 device tensors each): level 1 and the ring copy by k_pack_pyr.  bad_parent: the launch that gets a
    wrong parent tag.  -> (host records (K, n, 4) uint32, device records (K, n, 4) uint32, pyramid bytes (K + 1, ...) uint8 or None).
    w / h / pts / frames are taken as given, and stream (default: torch's current one), so that a test of the refusals can hand in what
    it likes without a device.  win: the tracker's window; any other than 21 goes through vstabx_lk_segments_win."""
    n_fr = len(frames)
    h = frames[0].shape[0] if h is None else h
    w = frames[0].shape[1] if w is None else w
    p = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    n = p.shape[0]
    sg = np.ascontiguousarray(segs, np.int32)
    K = int(sg.sum()) if sg.size else 0
    fptrs = (_vp * max(1, n_fr))(*[f.data_ptr() for f in frames])
    fpit = (_sz * max(1, n_fr))(*[f.stride(0) for f in frames])
    uptrs = upit = rptrs = None
    if uv is not None:
        uptrs = (_vp * len(uv))(*[u.data_ptr() for u in uv])
        upit = (_sz * len(uv))(*[u.stride(0) for u in uv])
    if rings is not None:
        rptrs = (_vp * len(rings))(*[r.data_ptr() for r in rings])
    hrec = np.zeros((max(K, 0), n, 4), np.uint32)
    drec = np.zeros((max(K, 0), n, 4), np.uint32)
    pyr = None
    if want_pyr:
        lw, lh, nb = w, h, 0
        for _ in range(3):
            lw, lh = (lw + 1) // 2, (lh + 1) // 2
            if lw <= win or lh <= win:
                break
            nb += lw * lh
        pyr = np.zeros((n_fr, max(nb, 1)), np.uint8)
    args = (fptrs, fpit, int(w), int(h), _fptr(p), n, sg.ctypes.data_as(_ip), int(sg.size), uptrs, upit, rptrs, int(bad_parent),
            hrec.ctypes.data_as(_c.POINTER(_c.c_uint32)), drec.ctypes.data_as(_c.POINTER(_c.c_uint32)), None if pyr is None else pyr.ctypes.data_as(_u8p))
    st = _stream() if stream is None else stream
    if win == 21:   # the hook as it always was
        _check(_L.vstabx_lk_segments(*args, st), "vstabx_lk_segments")
    else:           # vstabx_lk_segments_win: the tracker's window (15 or 31; anything else is refused there)
        _check(_L.vstabx_lk_segments_win(*args, int(win), st), "vstabx_lk_segments_win")
    return hrec, drec, pyr


def estimate_rotation(prev_xy, cur_xy, K_in, K_out, seed=1, D=None):
    """D: k1..k4 of the input lens (vstab_estimate_rotation_d), None = the ideal equidistant lens."""
    a = np.ascontiguousarray(prev_xy, np.float32).reshape(-1, 2)
    b = np.ascontiguousarray(cur_xy, np.float32).reshape(-1, 2)
    Ki = np.ascontiguousarray(K_in, np.float64).reshape(9)
    Ko = np.ascontiguousarray(K_out, np.float64).reshape(9)
    R = np.zeros(9)
    inl = _c.c_int()
    if D is not None:
        Dc = np.ascontiguousarray(D, np.float64).reshape(4)
        _check(_L.vstab_estimate_rotation_d(_fptr(a), _fptr(b), a.shape[0], _dptr(Ki), _dptr(Ko), _dptr(Dc), seed, _dptr(R), _c.byref(inl)),
               "vstab_estimate_rotation_d")
        return R.reshape(3, 3), inl.value
    _check(_L.vstab_estimate_rotation(_fptr(a), _fptr(b), a.shape[0], _dptr(Ki), _dptr(Ko), seed, _dptr(R), _c.byref(inl)),
           "vstab_estimate_rotation")
    return R.reshape(3, 3), inl.value


def estimate_rotation_pinhole(prev_xy, cur_xy, K_in, K_out, D, seed=1):
    """vstab_estimate_rotation_pinhole: estimate_rotation for a rectilinear input lens with D = (k1, k2, p1, p2, k3) -> (R, inliers)."""
    a = np.ascontiguousarray(prev_xy, np.float32).reshape(-1, 2)
    b = np.ascontiguousarray(cur_xy, np.float32).reshape(-1, 2)
    Ki, Ko = np.ascontiguousarray(K_in, np.float64).reshape(9), np.ascontiguousarray(K_out, np.float64).reshape(9)
    Dc = np.ascontiguousarray(D, np.float64).reshape(5)
    R = np.zeros(9)
    inl = _c.c_int()
    _check(_L.vstab_estimate_rotation_pinhole(_fptr(a), _fptr(b), a.shape[0], _dptr(Ki), _dptr(Ko), _dptr(Dc), seed, _dptr(R), _c.byref(inl)),
           "vstab_estimate_rotation_pinhole")
    return R.reshape(3, 3), inl.value


def gyro_integrate(samples, rate_scale, t_prev_first_row, t_first_row, t_last_row):
    """vstab_gyro_integrate.  samples: (n, 5) doubles {start_ts, end_ts, roll, pitch, yaw} (the reference's GyroFrame,
    gpmf.cpp:5-11) -> (R_delta, R_readout) 3x3."""
    a = np.ascontiguousarray(samples, np.float64).reshape(-1, 5)
    Rd, Rr = np.zeros(9), np.zeros(9)
    _check(_L.vstab_gyro_integrate(a.ctypes.data_as(_vp), a.shape[0], float(rate_scale), float(t_prev_first_row), float(t_first_row),
                                   float(t_last_row), Rd.ctypes.data_as(_dp), Rr.ctypes.data_as(_dp)), "vstab_gyro_integrate")
    return Rd.reshape(3, 3), Rr.reshape(3, 3)


def preload_kernels():
    """vstab_preload_kernels: load the library's GPU code objects now (vstab_create does it itself)."""
    _check(_L.vstab_preload_kernels(), "vstab_preload_kernels")


def gpmf_parse_gyro(payload, pkt_ts, pkt_dur, cap=None):
    """vstab_gpmf_parse_gyro: bytes of one GPMF packet -> (n, 5) array of {start_ts, end_ts, roll, pitch, yaw} samples."""
    buf = bytes(payload)
    n = _c.c_int(0)
    cap = (len(buf) // 2 + 1) if cap is None else int(cap)
    out = np.zeros((max(cap, 1), 5), np.float64)
    _check(_L.vstab_gpmf_parse_gyro(buf, len(buf), float(pkt_ts), float(pkt_dur), out.ctypes.data, cap, _c.byref(n)), "vstab_gpmf_parse_gyro")
    return out[: min(n.value, cap)].copy(), n.value


def sg_weights(m):
    w = np.zeros(2 * m + 1)
    _check(_L.vstab_sg_weights(m, _dptr(w)), "vstab_sg_weights")
    return w


class RotationFilter:
    def __init__(self, m):
        self._h = _vp()
        _check(_L.vstab_rotation_filter_create(m, _c.byref(self._h)), "vstab_rotation_filter_create")

    def add(self, R):
        r = np.ascontiguousarray(R, np.float64).reshape(9)
        _check(_L.vstab_rotation_filter_add(self._h, _dptr(r)), "vstab_rotation_filter_add")

    def filter(self):
        out = np.zeros(9)
        _check(_L.vstab_rotation_filter_filter(self._h, _dptr(out)), "vstab_rotation_filter_filter")
        return out.reshape(3, 3)

    def __del__(self):
        if getattr(self, "_h", None) and _L is not None:
            _L.vstab_rotation_filter_destroy(self._h)
            self._h = None


# ---------------------------------------------------------------------------------------------
# the pipeline object (FrameSourceWarp replacement)
# ---------------------------------------------------------------------------------------------
def default_config(**kw):
    cfg = Config()
    _L.vstab_config_default(_c.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


class Stabilizer:
    """vstab_handle wrapper.  `frames`: list of packed NV12 CUDA tensors (cycled by the C ring
    source for `total` pulls) or a Python iterable of such tensors (python callback source)."""

    def __init__(self, frames, total=None, use_torch_stream=True, hold=12, bit_depth=8, readouts=None, ring_hold=None, border_mode=None, calibration=None,
                 calibration_ex=None, pinhole=None, detection_mask=None, corner_response=None, harris_k=0.04, tracker_options=None, tracker_window=None, corner_block=None,
                 corner_gradient=None, **cfg_kw):
        """tracker_options: (max_level, max_iter, eps, min_eig) for set_tracker_options right after create.
        tracker_window: 15, 21 or 31 for set_tracker_window right after create.
        corner_response: set_corner_response(corner_response, harris_k) right after create (CORNER_HARRIS or CORNER_MIN_EIGENVAL).
        corner_block: 3, 5 or 7 for set_corner_block right after create.
        corner_gradient: 3, 5 or 7 for set_corner_gradient right after create.
        detection_mask: set_detection_mask right after create (a device tensor or a numpy array of the luma plane's size).
        border_mode: vstab_set_border_mode_ex right after create (BORDER_* constants; None keeps the constant border).
        calibration: (K, D) for set_input_calibration right after create, applied after border_mode (K None keeps the camera from in_dfov).
        calibration_ex: the same through set_input_calibration_ex (every resampler and border mode).
        pinhole: (K, D) for set_input_pinhole right after create: a rectilinear input lens with D = (k1, k2, p1, p2, k3) (K None as above).
        hold (iterable sources): vstab_frame.hold -- how many further pulls each tensor is kept alive and unchanged
        for; from smooth_radius + 14 on the library uses the tensors in place instead of copying them.
        bit_depth / readouts (list sources): P010 frames as int16 tensors of shape (h * 3 / 2, w); one 3x3 read-out
        rotation per ring frame (vstab_frame.readout_rotation).  ring_hold (list sources): the hold the ring source
        promises (default: forever, frames used in place; 0: every frame is copied into the library's ring)."""
        import torch
        self._keep = []
        self._src = Source()
        self._ring = None
        if isinstance(frames, (list, tuple)):
            f0 = frames[0]
            rows, w = f0.shape
            h = rows * 2 // 3
            ptrs = (_vp * len(frames))(*[f.data_ptr() for f in frames])
            self._keep += [frames, ptrs]
            self._ring = _vp()
            ro = None if readouts is None else np.ascontiguousarray(np.stack([np.asarray(r, np.float64).reshape(9) for r in readouts]))
            assert ro is None or ro.shape == (len(frames), 9)
            _check(_L.vstab_ring_source_create_ex(ptrs, len(frames), w, h, f0.stride(0) * f0.element_size(), len(frames) if total is None else total,
                                                  int(bit_depth), None if ro is None else _dptr(ro), _c.byref(self._ring), _c.byref(self._src)),
                   "vstab_ring_source_create_ex")
            if ring_hold is not None:
                _L.vstab_ring_source_set_hold(self._ring, int(ring_hold))
        else:
            it = iter(frames)
            state = {"next": None, "done": False}

            def fill(out, advance):
                if state["next"] is None and not state["done"]:
                    try:
                        state["next"] = next(it)
                    except StopIteration:
                        state["done"] = True
                if state["next"] is None:
                    return EOF
                f = state["next"]
                yp, uvp, pitch, w, h = _planes(f)
                o = out.contents
                o.y, o.uv, o.pitch_y, o.pitch_uv, o.width, o.height, o.mem, o.pts = yp, uvp, pitch, pitch, w, h, 0, 0
                o.hold = hold  # self._keep holds the last hold + 4 tensors alive
                if advance:
                    self._keep.append(f)
                    if len(self._keep) > hold + 4:
                        self._keep.pop(0)
                    state["next"] = None
                return 0
            self._pull = PULL_FN(lambda user, out: fill(out, True))
            self._peek = PULL_FN(lambda user, out: fill(out, False))
            self._src.pull, self._src.peek, self._src.user = self._pull, self._peek, None
        cfg = default_config(**cfg_kw)
        if use_torch_stream:
            cfg.stream = torch.cuda.current_stream().cuda_stream
        self._h = _vp()
        _check(_L.vstab_create(_c.byref(cfg), _c.byref(self._src), _c.byref(self._h)), "vstab_create")
        ow, oh = _c.c_int(), _c.c_int()
        Ki, Ko = np.zeros(9), np.zeros(9)
        _check(_L.vstab_get_output_info(self._h, _c.byref(ow), _c.byref(oh), _dptr(Ki), _dptr(Ko)), "vstab_get_output_info")
        self.out_size = (ow.value, oh.value)
        self.K_in, self.K_out = Ki.reshape(3, 3), Ko.reshape(3, 3)
        if border_mode is not None:
            self.set_border_mode_ex(border_mode)
        if calibration is not None:
            self.set_input_calibration(*calibration)
        if calibration_ex is not None:
            self.set_input_calibration_ex(*calibration_ex)
        if pinhole is not None:
            self.set_input_pinhole(*pinhole)
        if detection_mask is not None:
            self.set_detection_mask(detection_mask)
        if corner_response is not None:
            self.set_corner_response(corner_response, harris_k)
        if tracker_options is not None:
            self.set_tracker_options(*tracker_options)
        if tracker_window is not None:
            self.set_tracker_window(tracker_window)
        if corner_block is not None:
            self.set_corner_block(corner_block)
        if corner_gradient is not None:
            self.set_corner_gradient(corner_gradient)

    def set_tracker_window(self, win_size):
        """vstab_set_tracker_window: calcOpticalFlowPyrLK's winSize (15, 21 or 31) for every tracker launch of this handle, before the first
        pull; 21 is the handle as it always was.  Independent of set_tracker_options."""
        _check(_L.vstab_set_tracker_window(self._h, int(win_size)), "vstab_set_tracker_window")

    def set_tracker_options(self, max_level=3, max_iter=30, eps=0.01, min_eig=1e-4):
        """vstab_set_tracker_options: calcOpticalFlowPyrLK's maxLevel, criteria and minEigThreshold for every tracker launch of this handle,
        before the first pull; (3, 30, 0.01, 1e-4) is the handle as it always was."""
        _check(_L.vstab_set_tracker_options(self._h, int(max_level), int(max_iter), float(eps), float(min_eig)), "vstab_set_tracker_options")

    def set_corner_block(self, block_size):
        """vstab_set_corner_block: goodFeaturesToTrack's blockSize (3, 5 or 7) for every detection of this handle, before the first pull; in
        any order with set_corner_response and set_detection_mask"""
        _check(_L.vstab_set_corner_block(self._h, int(block_size)), "vstab_set_corner_block")

    def set_corner_gradient(self, gradient_size):
        """vstab_set_corner_gradient: goodFeaturesToTrack's gradientSize (3, 5 or 7) for every detection of this handle, before the first
        pull; in any order with set_corner_block, set_corner_response and set_detection_mask"""
        _check(_L.vstab_set_corner_gradient(self._h, int(gradient_size)), "vstab_set_corner_gradient")

    def set_corner_response(self, response, k=0.04):
        """vstab_set_corner_response: CORNER_HARRIS with k (goodFeaturesToTrack's useHarrisDetector and k) for every detection of this
        handle, or CORNER_MIN_EIGENVAL (k not looked at) to have the handle as it always was; before the first pull."""
        _check(_L.vstab_set_corner_response(self._h, int(response), float(k)), "vstab_set_corner_response")

    def set_detection_mask(self, mask):
        """vstab_set_detection_mask: goodFeaturesToTrack's mask for every detection of this handle, before the first pull.  mask: (h, w) uint8,
        non-zero = "a corner may be reported here" -- a device tensor or view (VSTAB_MEM_DEVICE), a numpy array (VSTAB_MEM_HOST; any row stride),
        or None to remove the mask.  The handle keeps a copy."""
        if mask is None:
            _check(_L.vstab_set_detection_mask(self._h, None, 0, 0), "vstab_set_detection_mask")
        elif isinstance(mask, np.ndarray):
            assert mask.dtype == np.uint8 and mask.ndim == 2 and mask.strides[1] == 1
            _check(_L.vstab_set_detection_mask(self._h, mask.ctypes.data, mask.strides[0], 1), "vstab_set_detection_mask")
        else:
            _check(_L.vstab_set_detection_mask(self._h, mask.data_ptr(), mask.stride(0), 0), "vstab_set_detection_mask")

    def _calibrate(self, fn, K, D):
        Kc = None if K is None else np.ascontiguousarray(K, np.float64).reshape(9)
        Dc = np.ascontiguousarray(np.broadcast_to(np.asarray(D, np.float64), (4,)))
        _check(getattr(_L, fn)(self._h, None if Kc is None else _dptr(Kc), _dptr(Dc)), fn)
        if Kc is not None:
            self.K_in = Kc.reshape(3, 3).copy()

    def set_input_calibration(self, K, D):
        """vstab_set_input_calibration: the calibrated input lens, camera matrix K (3x3, or None) and k1..k4 (a scalar 0 stands for four zeros),
        before the first pull."""
        self._calibrate("vstab_set_input_calibration", K, D)

    def set_input_calibration_ex(self, K, D):
        """vstab_set_input_calibration_ex: set_input_calibration for INTER_LINEAR, INTER_CUBIC and INTER_LANCZOS4 handles, with any border mode."""
        self._calibrate("vstab_set_input_calibration_ex", K, D)

    def set_input_pinhole(self, K, D):
        """vstab_set_input_pinhole: a rectilinear input lens with camera matrix K (3x3, or None) and D = (k1, k2, p1, p2, k3), before the first
        pull."""
        Kc = None if K is None else np.ascontiguousarray(K, np.float64).reshape(9)
        Dc = np.ascontiguousarray(D, np.float64).reshape(5)
        _check(_L.vstab_set_input_pinhole(self._h, None if Kc is None else _dptr(Kc), _dptr(Dc)), "vstab_set_input_pinhole")
        if Kc is not None:
            self.K_in = Kc.reshape(3, 3).copy()

    def warps_from_cache(self):
        """Test hook vstabx_warps_from_cache: warps of this handle that read the quantised map of an earlier frame with equal parameters."""
        return int(_L.vstabx_warps_from_cache(self._h))

    def detector_counters(self):
        """Test hook vstabx_detector_counters: speculative selections that found more than Detector::SPEC_CAP candidates, fused detections
        that overflowed the key buffer, the key capacity now in force."""
        out = (_c.c_long * 3)()
        _check(_L.vstabx_detector_counters(self._h, out), "vstabx_detector_counters")
        return dict(spec_over_cap=out[0], fused_overflows=out[1], key_capacity=out[2])

    def tracker_counters(self):
        """Test hook vstabx_tracker_counters: the handle's tracker launches, the frame pairs they cover and the pairs dropped with launches
        nobody read; frames that took the launch enqueued ahead of them, frames whose launch was replaced on demand, and planned key frames
        whose tracker was already running on the speculated corners."""
        out = (_c.c_long * 6)()
        _check(_L.vstabx_tracker_counters(self._h, out), "vstabx_tracker_counters")
        return dict(zip(("segs_launched", "seg_frames_launched", "seg_frames_dropped", "chained_adopted", "chained_discarded", "key_prelaunched"), out))

    def set_colour(self, matrix, range_=RANGE_LIMITED):
        """vstab_set_colour: the colour spec of the converting pulls (BGR, host, NV12 through BGR), from the next pull on."""
        _check(_L.vstab_set_colour(self._h, int(matrix), int(range_)), "vstab_set_colour")

    def set_colour10(self, matrix, range_=RANGE_LIMITED):
        """vstab_set_colour10: the colour spec of a pixel_depth 10 handle's converting pulls (16-bit BGR, P010), from the next pull on."""
        _check(_L.vstab_set_colour10(self._h, int(matrix), int(range_)), "vstab_set_colour10")

    def set_resample10(self, resample, border_mode=BORDER_CONSTANT):
        """vstab_set_resample10: the resampler (RESAMPLE_*) and border mode (BORDER_*) of a pixel_depth 10 handle's plane-wise pull, from the
        next pull on; (RESAMPLE_DEFAULT, BORDER_CONSTANT) restores the bilinear warp."""
        _check(_L.vstab_set_resample10(self._h, int(resample), int(border_mode)), "vstab_set_resample10")

    def set_border_mode(self, border_mode):
        """vstab_set_border_mode: cv::remap's borderMode for the frames pulled from now on."""
        _check(_L.vstab_set_border_mode(self._h, int(border_mode)), "vstab_set_border_mode")

    def set_readout_warp(self, mode):
        """vstab_set_readout_warp: READOUT_PER_ROW warps a frame that carries a read-out rotation row by row on cubic, Lanczos and calibrated
        handles (READOUT_REFUSE, the default, refuses and consumes it); applies from the next pull."""
        _check(_L.vstab_set_readout_warp(self._h, int(mode)), "vstab_set_readout_warp")

    def set_border_mode_ex(self, border_mode):
        """vstab_set_border_mode_ex: set_border_mode for INTER_LINEAR, INTER_CUBIC and INTER_LANCZOS4 handles."""
        _check(_L.vstab_set_border_mode_ex(self._h, int(border_mode)), "vstab_set_border_mode_ex")

    def pull_into(self, out, timing=None):
        """Returns True, or False at end of stream (the reference throws EOF)."""
        st = _L.vstab_pull_frame(self._h, out.data_ptr(), out.stride(0))
        if st == EOF:
            return False
        _check(st, "vstab_pull_frame")
        return True

    def pull_frames_into(self, outs, first, n):
        """vstab_pull_frames: n frames in one call, frame i into outs[(first + i) % len(outs)].  Returns the number emitted
        (fewer than n at end of stream)."""
        ring = getattr(self, "_out_ring", None)
        if ring is None or ring[0] is not outs:
            ptrs = (_c.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
            pitches = (_c.c_size_t * len(outs))(*[o.stride(0) for o in outs])
            ring = self._out_ring = (outs, ptrs, pitches)
        done = _c.c_int(0)
        st = _L.vstab_pull_frames(self._h, int(n), ring[1], ring[2], len(outs), int(first) % len(outs), _c.byref(done))
        if st != EOF:
            _check(st, "vstab_pull_frames")
        return done.value

    def pull(self):
        import torch
        out = torch.empty((self.out_size[1], self.out_size[0], 3), dtype=torch.uint8, device="cuda")
        return out if self.pull_into(out) else None

    def pull_bgr16_into(self, out):
        """pixel_depth = 10 handles: out is a (h, w, 3) int16 CUDA tensor; values 0..1023."""
        st = _L.vstab_pull_frame_bgr16(self._h, out.data_ptr(), out.stride(0) * 2)
        if st == EOF:
            return False
        _check(st, "vstab_pull_frame_bgr16")
        return True

    def pull_p010_into(self, out_y, out_uv):
        """pixel_depth = 10 handles: P010 planes (int16 CUDA tensors, (h, w) and (ceil(h/2), 2 * ceil(w/2)))."""
        st = _L.vstab_pull_frame_p010(self._h, out_y.data_ptr(), out_y.stride(0) * 2, out_uv.data_ptr(), out_uv.stride(0) * 2)
        if st == EOF:
            return False
        _check(st, "vstab_pull_frame_p010")
        return True

    def pull_host(self):
        """-> (h, w, 3) numpy array in host memory, or None at end of stream."""
        out = np.empty((self.out_size[1], self.out_size[0], 3), np.uint8)
        st = _L.vstab_pull_frame_host(self._h, out.ctypes.data, out.strides[0])
        if st == EOF:
            return None
        _check(st, "vstab_pull_frame_host")
        return out

    def pull_nv12_into(self, y, uv, planar=False):
        """planar=True: vstab_pull_frame_nv12_planar, the plane-wise warp (no colour round trip)."""
        fn, name = (_L.vstab_pull_frame_nv12_planar, "vstab_pull_frame_nv12_planar") if planar else (_L.vstab_pull_frame_nv12, "vstab_pull_frame_nv12")
        st = fn(self._h, y.data_ptr(), y.stride(0), uv.data_ptr(), uv.stride(0))
        if st == EOF:
            return False
        _check(st, name)
        return True

    def pull_nv12(self, planar=False):
        """-> (luma, chroma) tensors, or None at end of stream."""
        y, uv = nv12_out_planes(self.out_size[0], self.out_size[1])
        return (y, uv) if self.pull_nv12_into(y, uv, planar) else None

    def pull_keep_into(self, out, prev):
        """vstab_pull_frame_keep: the next frame into out, with prev's bytes where the warped frame does not cover the output.  prev: the
        previous output -- another tensor (a ring of two), or out itself (in place).  Returns True, or False at end of stream."""
        st = _L.vstab_pull_frame_keep(self._h, out.data_ptr(), out.stride(0), prev.data_ptr(), prev.stride(0))
        if st == EOF:
            return False
        _check(st, "vstab_pull_frame_keep")
        return True

    def pull_nv12_planar_keep_into(self, y, uv, prev_y, prev_uv):
        """vstab_pull_frame_nv12_planar_keep: pull_keep_into for the plane-wise warp; (prev_y, prev_uv) another pair of planes, or (y, uv)."""
        st = _L.vstab_pull_frame_nv12_planar_keep(self._h, y.data_ptr(), y.stride(0), uv.data_ptr(), uv.stride(0), prev_y.data_ptr(), prev_y.stride(0),
                                                  prev_uv.data_ptr(), prev_uv.stride(0))
        if st == EOF:
            return False
        _check(st, "vstab_pull_frame_nv12_planar_keep")
        return True

    def pull_p010_planar_into(self, out_y, out_uv):
        """pixel_depth = 10 handles: the frame warped plane by plane (vstab_pull_frame_p010_planar), P010 planes as pull_p010_into."""
        st = _L.vstab_pull_frame_p010_planar(self._h, out_y.data_ptr(), out_y.stride(0) * 2, out_uv.data_ptr(), out_uv.stride(0) * 2)
        if st == EOF:
            return False
        _check(st, "vstab_pull_frame_p010_planar")
        return True

    def frame_log(self):
        out = []
        for i in range(_L.vstab_frame_log_count(self._h)):
            lg = FrameLog()
            _check(_L.vstab_get_frame_log(self._h, i, _c.byref(lg)), "vstab_get_frame_log")
            out.append(dict(key=bool(lg.key_frame), n_corners=lg.n_corners, n_tracked=lg.n_tracked, inliers=lg.n_inliers,
                            fallback=bool(lg.fallback), R=np.array(lg.R_frame).reshape(3, 3),
                            R_accum=np.array(lg.R_accum).reshape(3, 3)))
        return out

    def enable_profiling(self, level=2):
        _check(_L.vstab_enable_profiling(self._h, int(level)), "vstab_enable_profiling")

    def profile(self):
        p = Profile()
        _check(_L.vstab_get_profile(self._h, _c.byref(p)), "vstab_get_profile")
        return {k: getattr(p, k) for k, _ in Profile._fields_}

    def warp_rotation(self, i):
        R = np.zeros(9)
        _check(_L.vstab_get_warp_rotation(self._h, i, _dptr(R)), "vstab_get_warp_rotation")
        return R.reshape(3, 3)

    def close(self):
        if _L is None:
            return
        if getattr(self, "_h", None):
            _L.vstab_destroy(self._h)
            self._h = None
        if getattr(self, "_ring", None):
            _L.vstab_ring_source_destroy(self._ring)
            self._ring = None

    def __del__(self):
        self.close()
