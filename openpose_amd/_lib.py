"""ctypes binding of libopk_hip.so (C-ABI: include/opk.h).

The library is REQUIRED: importing the product API without it raises -- there is no CPU or
PyTorch fallback anywhere in the product path.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libopk_hip.so")
if os.environ.get("OPK_LIB_PATH"):   # dev A/B of two builds in one process tree
    LIB_PATH = os.environ["OPK_LIB_PATH"]

_c = ctypes
_p = _c.c_void_p
_i = _c.c_int
_f = _c.c_float
_d = _c.c_double
_ip = _c.POINTER(_c.c_int)
_fp = _c.POINTER(_c.c_float)

# name: (restype, argtypes)
_SIGS = {
    "opk_last_error": (_c.c_char_p, []),
    "opk_version": (_i, []),
    "opk_dev_set": (_i, [_c.c_char_p, _i, _i]),
    "opk_ctx_create": (_i, [_i, _p, _c.POINTER(_p)]),
    "opk_ctx_create_private_stream": (_i, [_i, _c.POINTER(_p)]),
    "opk_ctx_destroy": (_i, [_p]),
    "opk_ctx_stream": (_i, [_p, _c.POINTER(_p)]),
    "opk_sync": (_i, [_p]),
    "opk_malloc": (_i, [_p, _c.POINTER(_p), _c.c_size_t]),
    "opk_free": (_i, [_p, _p]),
    "opk_memset": (_i, [_p, _p, _i, _c.c_size_t]),
    "opk_convert": (_i, [_p, _p, _i, _p, _i, _c.c_size_t]),
    "opk_memcpy_h2d": (_i, [_p, _p, _p, _c.c_size_t]),
    "opk_memcpy_d2h": (_i, [_p, _p, _p, _c.c_size_t]),
    "opk_probe_peaks": (_i, [_p, _c.POINTER(_d), _c.POINTER(_d), _c.POINTER(_d)]),
    "opk_render_pose_keypoints": (_i, [_p, _p, _i, _i, _c.c_uint, _c.c_uint, _p, _f, _i, _i, _f]),
    "opk_render_face_keypoints": (_i, [_p, _p, _c.c_uint, _c.c_uint, _p, _i, _f, _f]),
    "opk_render_hand_keypoints": (_i, [_p, _p, _c.c_uint, _c.c_uint, _p, _i, _f, _f]),
    "opk_render_pose_heat_map": (_i, [_p, _p, _c.c_uint, _c.c_uint, _p, _i, _i, _f, _c.c_uint, _f]),
    "opk_render_pose_heat_maps": (_i, [_p, _p, _i, _c.c_uint, _c.c_uint, _p, _i, _i, _f, _f]),
    "opk_render_pose_paf": (_i, [_p, _p, _i, _c.c_uint, _c.c_uint, _p, _i, _i, _f, _i, _f]),
    "opk_render_pose_pafs": (_i, [_p, _p, _i, _c.c_uint, _c.c_uint, _p, _i, _i, _f, _f]),
    "opk_render_pose_distance": (_i, [_p, _p, _c.c_uint, _c.c_uint, _p, _i, _i, _f, _c.c_uint, _f]),
    "opk_resize_and_merge": (_i, [_p, _p, _c.POINTER(_p), _i, _ip, _ip, _fp]),
    "opk_nms": (_i, [_p, _p, _p, _p, _f, _ip, _ip, _f, _f]),
    "opk_nms_semantics": (_i, [_p, _p, _p, _p, _f, _ip, _ip, _f, _f, _i]),
    "opk_pose_set_map_semantics": (_i, [_p, _i]),
    "opk_resize_and_merge_semantics": (_i, [_p, _p, _c.POINTER(_p), _i, _ip, _ip, _fp, _i]),
    "opk_paf_scores": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _f, _f, _f]),
    "opk_paf_scores_sources": (_i, [_p, _p, _i, _c.POINTER(_p), _i, _ip, _i, _i, _i, _fp, _p, _i, _i,
                                    _f, _f, _f, _c.POINTER(_c.c_size_t)]),
    "opk_connect_body_parts": (_i, [_p, _p, _p, _i, _ip, _p, _p, _i, _i, _i, _i, _i, _f, _f, _i,
                                    _f, _f, _f, _i]),
    "opk_assemble_people": (_i, [_p, _p, _i, _ip, _p, _p, _i, _i, _i, _f, _f, _i]),
    "opk_connect_body_parts_semantics": (_i, [_p, _p, _p, _i, _ip, _p, _p, _i, _i, _i, _i, _i, _f,
                                              _f, _i, _f, _f, _f, _i, _i]),
    "opk_assemble_people_semantics": (_i, [_p, _p, _i, _ip, _p, _p, _i, _i, _i, _f, _f, _i, _i]),
    "opk_pose_model_info": (_i, [_i, _ip, _ip, _ip, _ip, _p, _p]),
    "opk_pose_default_thresholds": (_i, [_i, _i, _fp, _fp]),
    "opk_net_create": (_i, [_p, _c.c_char_p, _c.c_char_p, _c.POINTER(_p)]),
    "opk_net_destroy": (_i, [_p]),
    "opk_net_num_convs": (_i, [_p]),
    "opk_net_conv_info": (_i, [_p, _i, _c.c_char_p, _ip, _ip, _ip, _ip]),
    "opk_net_set_conv": (_i, [_p, _c.c_char_p, _p, _p, _p]),
    "opk_net_forward": (_i, [_p, _p, _i, _i, _i]),
    "opk_net_flops_per_frame": (_i, [_p, _i, _i, _c.POINTER(_d)]),
    "opk_net_output": (_i, [_p, _c.POINTER(_p), _ip]),
    "opk_net_blob": (_i, [_p, _c.c_char_p, _i, _i, _p, _ip]),
    "opk_net_launch_log": (_i, [_p, _c.c_char_p, _c.c_size_t, _c.POINTER(_c.c_size_t)]),
    "opk_launch_log_begin": (_i, []),
    "opk_launch_log_end": (_i, [_c.c_char_p, _c.c_size_t, _c.POINTER(_c.c_size_t)]),
    "opk_pose_create": (_i, [_p, _p, _i, _c.POINTER(_p)]),
    "opk_pose_create_model": (_i, [_p, _p, _i, _i, _i, _c.POINTER(_p)]),
    "opk_pose_destroy": (_i, [_p]),
    "opk_pose_set_property": (_i, [_p, _i, _d]),
    "opk_pose_forward": (_i, [_p, _p, _i, _i, _i, _i, _i]),
    "opk_pose_forward_net_output": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i]),
    "opk_pose_set_upsampling_ratio": (_i, [_p, _f]),
    "opk_pose_heatmap_size": (_i, [_p, _ip]),
    "opk_pose_set_overlay": (_i, [_p, _p]),
    "opk_pose_submit": (_i, [_p, _p, _i, _i, _i, _i, _i]),
    "opk_pose_submit_net_output": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i]),
    "opk_pose_collect": (_i, [_p, _ip]),
    "opk_pose_submit_multi": (_i, [_p, _c.POINTER(_p), _ip, _i, _i, _i, _i]),
    "opk_pose_forward_multi": (_i, [_p, _c.POINTER(_p), _ip, _i, _i, _i, _i]),
    "opk_pose_pending": (_i, [_p]),
    "opk_pose_num_people": (_i, [_p, _i]),
    "opk_pose_keypoints": (_i, [_p, _i, _p, _p, _i]),
    "opk_pose_set_timing": (_i, [_p, _i]),
    "opk_pose_read_timing": (_i, [_p, _ip, _c.POINTER(_d)]),
    "opk_pose_read_collect_times": (_i, [_p, _ip, _c.POINTER(_d), _c.POINTER(_d), _ip]),
    "opk_net_set_precision": (_i, [_p, _i]),
    "opk_net_set_precision_schedule": (_i, [_p, _ip, _i]),
    "opk_net_conv_precision": (_i, [_p, _i]),
    "opk_net_blob_planes": (_i, [_p, _c.c_char_p, _i, _i, _p, _p, _ip, _ip]),
    "opk_net_set_small_batch": (_i, [_p, _i]),
    "opk_net_small_batch": (_i, [_p]),
    "opk_net_conv_plan": (_i, [_p, _i, _i, _i, _i, _i, _ip, _ip, _ip, _ip]),
    "opk_net_conv_kernels": (_i, [_p, _i, _i, _i, _i, _i, _c.c_char_p, _c.c_size_t, _c.POINTER(_c.c_size_t)]),
    "opk_pose_records":(_i, [_p, _p, _c.c_size_t, _c.POINTER(_c.c_size_t)]),
    "opk_pose_heatmaps": (_i, [_p, _c.POINTER(_p), _ip]),
    "opk_pose_peaks": (_i, [_p, _c.POINTER(_p), _ip]),
    "opk_pose_scale_net_to_output": (_f, [_p]),
    "opk_net_load_caffemodel": (_i, [_p, _c.c_char_p, _ip]),
    "opk_caffemodel_blob": (_i, [_c.c_char_p, _c.c_char_p, _i, _p, _c.c_size_t, _p, _ip]),
    "opk_net_set_timing": (_i, [_p, _i]),
    "opk_net_read_timing": (_i, [_p, _ip, _c.POINTER(_d)]),
    "opk_pose_heatmaps_copy": (_i, [_p, _i, _i, _p, _ip]),
    "opk_pose_heatmaps_copy_range": (_i, [_p, _i, _i, _i, _i, _p, _i, _ip]),
    "opk_pose_candidates": (_i, [_p, _i, _p, _ip]),
    "opk_scale_keypoints": (_i, [_p, _i, _i, _i, _d, _d, _i, _i]),
    "opk_keep_top_n_people": (_i, [_p, _i, _i, _p, _i, _p, _p, _ip]),
    "opk_people_json": (_i, [_p, _i, _p, _p, _i, _i, _p, ctypes.c_size_t, _p]),
    "opk_save_people_json": (_i, [ctypes.c_char_p, _p, _i, _p, _p, _i, _i]),
    "opk_face_detect": (_i, [_i, _p, _i, _i, _p]),
    "opk_hand_detect": (_i, [_i, _p, _i, _i, _p]),
    "opk_extractor_create": (_i, [_p, _p, _i, _i, _i, _c.POINTER(_p)]),
    "opk_extractor_destroy": (_i, [_p]),
    "opk_extractor_set_scales": (_i, [_p, _i, _f]),
    "opk_extractor_set_max_batch": (_i, [_p, _i]),
    "opk_extractor_set_heatmaps": (_i, [_p, _i]),
    "opk_extractor_heatmaps": (_i, [_p, _p, _ip]),
    "opk_extractor_parts": (_i, [_p]),
    "opk_extractor_forward": (_i, [_p, _p, _i, _i, _i, _c.c_size_t, _p, _p, _i, _p]),
    "opk_extractor_crop_count": (_i, [_p]),
    "opk_extractor_crop": (_i, [_p, _i, _p, _c.POINTER(_p)]),
    "opk_pose_attach_extractor": (_i, [_p, _p]),
    "opk_pose_detach_extractor": (_i, [_p, _i]),
    "opk_pose_part_rectangles": (_i, [_p, _i, _i, _p]),
    "opk_pose_part_keypoints": (_i, [_p, _i, _i, _p, _i]),
    "opk_pose_read_part_times": (_i, [_p, _i, _ip, _ip, _c.POINTER(_d), _c.POINTER(_d)]),
    "opk_pose_render_frames_parts": (_i, [_p, _p, _c.c_size_t, _i, _i, _p, _i, _i, _i, _c.c_size_t,
                                          _d, _f, _f, _i, _i, _i, _f, _f, _f, _f]),
    "opk_scale_and_size": (_i, [_i, _i, _i, _i, _f, _i, _d, _c.POINTER(_d), _ip]),
    "opk_cvmat_to_input": (_i, [_p, _p, _p, _i, _i, _i, _c.c_size_t, _d, _i, _i, _i]),
    "opk_pose_set_input": (_i, [_p, _i, _i, _f, _i, _d]),
    "opk_pose_submit_frames": (_i, [_p, _p, _i, _i, _i, _c.c_size_t]),
    "opk_pose_forward_frames": (_i, [_p, _p, _i, _i, _i, _c.c_size_t]),
    "opk_pose_net_input": (_i, [_p, _i, _c.POINTER(_p), _ip, _ip]),
    "opk_cvmat_to_output": (_i, [_p, _p, _p, _i, _i, _i, _c.c_size_t, _d, _i, _i]),
    "opk_output_to_cvmat": (_i, [_p, _p, _c.c_size_t, _p, _i, _i, _i, _i]),
    "opk_render_frames": (_i, [_p, _p, _c.c_size_t, _i, _i, _p, _i, _i, _i, _c.c_size_t, _d, _p, _i,
                               _i, _i]),
    "opk_pose_render_frames": (_i, [_p, _p, _c.c_size_t, _i, _i, _p, _i, _i, _i, _c.c_size_t, _d,
                                    _f, _f, _i, _i, _i]),
    "opk_render_frames_heat": (_i, [_p, _p, _c.c_size_t, _i, _i, _p, _i, _i, _i, _c.c_size_t, _d, _p,
                                    _i, _i, _i, _p]),
    "opk_render_element": (_i, [_i, _i, _ip, _ip]),
    # the same on opk_frames descriptors (FramesStruct)
    "opk_frames_to_bgr": (_i, [_p, _p, _c.c_size_t, _p]),
    "opk_cvmat_to_input_fmt": (_i, [_p, _p, _p, _d, _i, _i, _i]),
    "opk_pose_submit_frames_fmt": (_i, [_p, _p]),
    "opk_pose_forward_frames_fmt": (_i, [_p, _p]),
    "opk_extractor_forward_fmt": (_i, [_p, _p, _p, _p, _i, _p]),
    "opk_cvmat_to_output_fmt": (_i, [_p, _p, _p, _d, _i, _i]),
    "opk_render_frames_fmt": (_i, [_p, _p, _c.c_size_t, _i, _i, _p, _d, _p, _i, _i, _i]),
    "opk_render_frames_heat_fmt": (_i, [_p, _p, _c.c_size_t, _i, _i, _p, _d, _p, _i, _i, _i, _p]),
    "opk_pose_render_frames_fmt": (_i, [_p, _p, _c.c_size_t, _i, _i, _p, _d, _f, _f, _i, _i, _i]),
    "opk_pose_render_frames_parts_fmt": (_i, [_p, _p, _c.c_size_t, _i, _i, _p, _d, _f, _f, _i, _i,
                                              _i, _f, _f, _f, _f]),
    "opk_pose_render_frames_element_fmt": (_i, [_p, _p, _c.c_size_t, _i, _i, _p, _d, _i, _f, _f,
                                                _f, _i, _i, _i]),
    "opk_pose_render_frames_element": (_i, [_p, _p, _c.c_size_t, _i, _i, _p, _i, _i, _i,
                                            _c.c_size_t, _d, _i, _f, _f, _f, _i, _i, _i]),
    # frames out: an opk_frames_out destination (FramesOutStruct), BGR, NV12 or I420
    "opk_bgr_to_frames": (_i, [_p, _p, _p]),
    "opk_render_frames_to": (_i, [_p, _p, _p, _d, _p, _i, _i, _i, _p]),
    "opk_pose_render_frames_to": (_i, [_p, _p, _p, _d, _i, _f, _f, _f, _i, _i, _i, _fp]),
    # person ids across frames: pyramid, Lucas-Kanade, matching, tracker
    "opk_pyramid_layout": (_i, [_i, _i, _i, _ip, _ip, _c.POINTER(_c.c_size_t),
                                _c.POINTER(_c.c_size_t)]),
    "opk_pyramid_build": (_i, [_p, _p, _p, _i]),
    "opk_pyramid_level": (_i, [_p, _p, _p, _i, _i, _i, _i, _i]),
    "opk_lk_points": (_i, [_p, _p, _i, _p, _i, _i, _p, _i]),
    "opk_match_people": (_i, [_p, _p, _i, _p, _i, _i, _f, _f, _i, _i, _c.POINTER(_c.c_longlong),
                              _p]),
    "opk_tracker_create": (_i, [_p, _f, _f, _f, _i, _c.POINTER(_p)]),
    "opk_tracker_destroy": (_i, [_p]),
    "opk_tracker_reset": (_i, [_p]),
    "opk_tracker_update": (_i, [_p, _p, _p, _p, _i, _p]),
    "opk_tracker_set_timing": (_i, [_p, _i]),
    "opk_tracker_read_times": (_i, [_p, _ip, _c.POINTER(_d), _c.POINTER(_d), _c.POINTER(_d),
                                    _c.POINTER(_c.c_size_t)]),
    "opk_pose_attach_tracker": (_i, [_p, _p]),
    "opk_pose_detach_tracker": (_i, [_p]),
    "opk_pose_person_ids": (_i, [_p, _i, _p]),
    "opk_pose_read_track_times": (_i, [_p, _ip, _c.POINTER(_d), _c.POINTER(_d), _c.POINTER(_d)]),
    # 3-D keypoints from a camera rig (RigStruct)
    "opk_camera_matrix": (_i, [_p, _p, _p]),
    "opk_triangulate_host": (_i, [_p, _i, _i, _p, _p, _p, _p, _p, _p]),
    "opk_triangulate": (_i, [_p, _p, _i, _i, _p, _p, _p, _p, _p, _p]),
    "opk_pose_set_views": (_i, [_p, _p]),
    "opk_pose_keypoints_3d": (_i, [_p, _i, _i, _p, _ip]),
    # undistorted rig frames and the calibration files (CamerasStruct, CameraParametersStruct)
    "opk_undistort_maps_host": (_i, [_p, _i, _p, _p]),
    "opk_undistort_frames": (_i, [_p, _p, _p, _p]),
    "opk_pose_set_undistort": (_i, [_p, _p]),
    "opk_pose_undistorted_frames": (_i, [_p, _p]),
    "opk_camera_parameters_read": (_i, [_c.c_char_p, _c.POINTER(_c.c_char_p), _i, _p, _i, _ip]),
    # rotated and flipped frames
    "opk_orient_size": (_i, [_i, _i, _i, _ip, _ip]),
    "opk_orient_frames": (_i, [_p, _p, _p, _i, _i]),
    "opk_orient_keypoints": (_i, [_p, _i, _i, _i, _i, _i, _i, _i]),
    "opk_pose_set_orientation": (_i, [_p, _i, _i]),
    "opk_pose_oriented_frames": (_i, [_p, _p]),
    # frames to JPEG files
    "opk_jpeg_bound": (_c.c_size_t, [_i, _i, _i]),
    "opk_jpeg_encode_host": (_i, [_p, _c.c_size_t, _p, _p, _c.c_size_t, _c.c_size_t, _i, _i, _i, _i]),
    "opk_jpeg_encode": (_i, [_p, _p, _c.c_size_t, _p, _p, _i]),
}


class FramesStruct(ctypes.Structure):
    """opk_frames (include/opk.h)."""
    _fields_ = [("format", _i), ("n", _i), ("width", _i), ("height", _i), ("plane", _p * 3),
                ("step", _c.c_size_t * 3), ("frame_bytes", _c.c_size_t * 3)]


class RigStruct(ctypes.Structure):
    """opk_rig (include/opk.h)."""
    _fields_ = [("views", _i), ("camera_matrices", _p), ("image_sizes", _p), ("min_views", _i)]


class CamerasStruct(ctypes.Structure):
    """opk_cameras (include/opk.h)."""
    _fields_ = [("views", _i), ("intrinsics", _p), ("distortions", _p), ("ncoef", _p),
                ("image_sizes", _p)]


class CameraParametersStruct(ctypes.Structure):
    """opk_camera_parameters (include/opk.h)."""
    _fields_ = [("serial", _c.c_char * 256), ("extrinsics", _d * 12), ("intrinsics", _d * 9),
                ("distortion", _d * 14), ("ncoef", _i), ("has_initial", _i),
                ("extrinsics_initial", _d * 12), ("camera_matrix", _d * 12)]


class FramesOutStruct(ctypes.Structure):
    """opk_frames_out (include/opk.h): opk_frames with writable planes."""
    _fields_ = list(FramesStruct._fields_)


class RenderHeatStruct(ctypes.Structure):
    """opk_render_heat (include/opk.h)."""
    _fields_ = [("kind", _i), ("pose_model", _i), ("channel", _i), ("heat_dev", _p),
                ("channels", _i), ("heat_w", _i), ("heat_h", _i), ("scale_to_keep_ratio", _f),
                ("alpha", _f)]


class RenderLayerStruct(ctypes.Structure):
    """opk_render_layer (include/opk.h)."""
    _fields_ = [("kind", _i), ("pose_model", _i), ("keypoints_dev", _p), ("counts_host", _ip),
                ("render_threshold", _f), ("alpha", _f), ("googly_eyes", _i)]


_LIB = None


class OpkError(RuntimeError):
    pass


def load():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise OpkError("libopk_hip.so not built (run `python -m openpose_amd.build`); the "
                           "product has no fallback path")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name, None)
            if fn is None:       # reported by tests/test_abi.py::test_exports_every_symbol
                continue
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def exported_symbols():
    return list(_SIGS)


def check(rc):
    if rc != 0:
        raise OpkError("opk error %d: %s" % (rc, load().opk_last_error().decode()))
    return rc


def int4(v):
    return (ctypes.c_int * 4)(*[int(x) for x in v])
