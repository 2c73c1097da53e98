"""ctypes binding of libsuperslam_hip.so (the C ABI in include/sship.h).

The product path is the HIP library and nothing else: if it is missing, or no gfx950 device is
visible, every call raises - there is no CPU or PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# The ONE library this package loads.  No environment variable moves it (include/sship.h, "Environment": the product reads
# SUPERSLAM_HIP_DEVICE and SSHIP_RCCL_LIBRARY, nothing else); a developer A/B build of the same ABI is selected explicitly, in code, with
# set_library_path() before the first call (tests/test_gpu_alt_paths.py and scripts/dev/* do that through scripts/_devlib.py).
LIB_PATH = os.path.join(_HERE, "lib", "libsuperslam_hip.so")


def set_library_path(path) -> None:
    """Load `path` instead of the shipped library (developer A/B builds: build.build_variant / build_dev).  None = keep the shipped one.
    Must come before the first call into the library: one process, one library."""
    global LIB_PATH
    if not path:
        return
    path = os.path.abspath(path)
    if _lib is not None and path != LIB_PATH:
        raise SshipError(ERR_INVALID, f"set_library_path({path}): {LIB_PATH} is already loaded in this process")
    LIB_PATH = path

OK = 0
ERR_INVALID, ERR_HIP, ERR_IO, ERR_NOMEM, ERR_POOL_EXHAUSTED, ERR_NO_DEVICE = 1, 2, 3, 4, 5, 6


class SshipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"sship error {code}: {msg}")
        self.code = code


class SpConfig(C.Structure):
    _fields_ = [("weights_path", C.c_char_p), ("max_keypoints", C.c_int), ("keypoint_threshold", C.c_double),
                ("remove_borders", C.c_int), ("nms_radius", C.c_int), ("pool_slots", C.c_int),
                ("max_batch", C.c_int)]


class Features(C.Structure):
    _fields_ = [("kp_xys", C.POINTER(C.c_float)), ("n", C.c_int), ("desc_dev", C.c_void_p), ("slot", C.c_int)]


class PoseParams(C.Structure):
    _fields_ = [("sigma_px", C.c_double), ("sigma_d0", C.c_double), ("cond_depth", C.c_double), ("huber_k2", C.c_double),
                ("lambda0", C.c_double), ("lambda_max", C.c_double), ("abs_tol", C.c_double), ("rel_tol", C.c_double),
                ("inlier_px", C.c_double), ("max_iterations", C.c_int)]


class RansacParams(C.Structure):
    _fields_ = [("inlier_px", C.c_double), ("min_disparity", C.c_double), ("min_area2", C.c_double), ("seed", C.c_uint32),
                ("num_hypotheses", C.c_int)]


class BaParams(C.Structure):
    _fields_ = [("sigma_px", C.c_double), ("huber_k2", C.c_double), ("lambda0", C.c_double), ("lambda_max", C.c_double),
                ("abs_tol", C.c_double), ("rel_tol", C.c_double), ("max_iterations", C.c_int)]


class PgParams(C.Structure):
    _fields_ = [("odom_sigma_rot", C.c_double), ("odom_sigma_trans", C.c_double), ("lambda0", C.c_double), ("lambda_max", C.c_double),
                ("abs_tol", C.c_double), ("rel_tol", C.c_double), ("max_translation", C.c_double), ("max_iterations", C.c_int)]


class RgbdParams(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("dist", C.c_double * 8),
                ("bf", C.c_double), ("depth_factor", C.c_double), ("max_depth", C.c_double)]


class StereoRefineParams(C.Structure):
    _fields_ = [("half_window", C.c_int), ("search_radius", C.c_int), ("max_rms", C.c_float), ("min_disparity", C.c_float),
                ("on_reject", C.c_int)]


class StereoSearchParams(C.Structure):
    _fields_ = [("half_window", C.c_int), ("min_disparity", C.c_int), ("max_disparity", C.c_int), ("uniqueness", C.c_int),
                ("min_texture", C.c_float), ("max_rms", C.c_float), ("lr_check", C.c_int)]


class PatchTrackParams(C.Structure):
    _fields_ = [("half_window", C.c_int), ("search_radius", C.c_int), ("uniqueness", C.c_int), ("min_texture", C.c_float),
                ("max_rms", C.c_float), ("fb_check", C.c_int)]


class PyrTrackParams(C.Structure):
    _fields_ = [("fine", PatchTrackParams), ("levels", C.c_int), ("coarse_radius", C.c_int)]


class FastParams(C.Structure):
    _fields_ = [("threshold", C.c_int), ("border", C.c_int), ("min_distance", C.c_int), ("selection", C.c_int), ("bucket_px", C.c_int),
                ("max_new", C.c_int), ("target", C.c_int)]


_lib = None
vp, ip, fp, dp = C.c_void_p, C.c_int, C.c_float, C.c_double
_SIGS = {
    "sship_init": (ip, [ip]),
    "sship_version": (ip, []),
    "sship_last_error": (C.c_char_p, []),
    "sship_device_synchronize": (ip, []),
    "sship_pool_create": (ip, [ip, ip, ip, C.POINTER(vp)]),
    "sship_pool_destroy": (None, [vp]),
    "sship_pool_retain": (None, [vp]),
    "sship_pool_release_ref": (None, [vp]),
    "sship_pool_acquire": (ip, [vp]),
    "sship_pool_release": (None, [vp, ip]),
    "sship_pool_in_use": (ip, [vp]),
    "sship_pool_slot_ptr": (vp, [vp, ip]),
    "sship_gather_normalize": (ip, [vp, ip, ip, ip, vp, vp, ip, vp, vp]),
    "sship_gather_normalize_hwc": (ip, [vp, ip, ip, ip, vp, vp, ip, vp, vp]),
    "sship_sample_descriptors_bilinear": (ip, [vp, ip, ip, ip, vp, ip, vp, vp]),
    "sship_sample_descriptors_bilinear_hwc": (ip, [vp, ip, ip, ip, vp, ip, vp, vp]),
    "sship_refine_keypoints": (ip, [vp, ip, ip, vp, ip, vp, vp]),
    "sship_refine_keypoints_hwc": (ip, [vp, ip, ip, ip, vp, ip, vp, vp]),
    "sship_nms": (ip, [vp, ip, ip, ip, ip, vp, vp]),
    "sship_select_topk": (ip, [vp, ip, ip, ip, ip, C.c_double, ip, ip, ip, ip, vp, vp, vp, vp, vp, vp]),
    "sship_sp_create": (ip, [C.POINTER(SpConfig), C.POINTER(vp)]),
    "sship_sp_destroy": (None, [vp]),
    "sship_sp_pool": (vp, [vp]),
    "sship_sp_max_keypoints": (ip, [vp]),
    "sship_sp_set_descriptor_sampling": (ip, [vp, ip]),
    "sship_sp_descriptor_sampling": (ip, [vp]),
    "sship_sp_set_keypoint_refinement": (ip, [vp, ip]),
    "sship_sp_keypoint_refinement": (ip, [vp]),
    "sship_sp_set_keypoint_selection": (ip, [vp, ip, ip]),
    "sship_sp_keypoint_selection": (ip, [vp, C.POINTER(ip)]),
    "sship_select_topk_balanced": (ip, [vp, ip, ip, ip, ip, C.c_double, ip, ip, ip, ip, ip, vp, vp, vp, vp, vp, vp]),
    "sship_sp_extract": (ip, [vp, vp, ip, ip, ip, ip, C.POINTER(Features)]),
    "sship_sp_extract_stereo": (ip, [vp, vp, vp, ip, ip, ip, ip, C.POINTER(Features), C.POINTER(Features)]),
    "sship_sp_infer_host": (ip, [vp, vp, ip, ip, ip, ip, vp, vp, C.POINTER(ip)]),
    "sship_sp_ring_create": (ip, [vp, ip, ip, ip, ip]),
    "sship_sp_ring_host": (vp, [vp, ip, ip]),
    "sship_sp_ring_upload": (ip, [vp, ip]),
    "sship_sp_extract_stereo_ring": (ip, [vp, ip, C.POINTER(Features), C.POINTER(Features)]),
    "sship_sp_ring_submit": (ip, [vp, ip]),
    "sship_sp_extract_batch_device": (ip, [vp, vp, ip, ip, ip, vp, vp, vp, vp]),
    "sship_sp_dense": (ip, [vp, vp, ip, ip, ip, vp, vp, vp, vp]),
    "sship_sp_debug_activation": (ip, [vp, ip, vp, C.c_ulonglong]),
    "sship_lg_weights_load": (ip, [C.c_char_p, C.POINTER(vp)]),
    "sship_lg_weights_retain": (None, [vp]),
    "sship_lg_weights_release": (None, [vp]),
    "sship_lg_create": (ip, [vp, ip, ip, ip, ip, C.POINTER(vp)]),
    "sship_lg_destroy": (None, [vp]),
    "sship_lg_normalize_keypoints": (ip, [vp, vp, ip, ip, vp]),
    "sship_lg_match_device": (ip, [vp, vp, ip, ip, vp, vp, ip, ip, vp, vp, vp]),
    "sship_lg_match_host": (ip, [vp, vp, ip, ip, vp, vp, ip, ip, vp, vp, vp]),
    "sship_lg_match_batch_device": (ip, [vp, vp, vp, vp, ip, vp, vp, vp]),
    "sship_lg_set_depth_confidence": (ip, [vp, fp]),
    "sship_lg_layers_run": (ip, [vp, vp, ip]),
    "sship_lg_set_width_confidence": (ip, [vp, fp, ip]),
    "sship_lg_prune_counts": (ip, [vp, ip, vp, ip, vp, ip]),
    "sship_lg_debug_set_layers": (ip, [vp, ip]),
    "sship_lg_debug_read": (ip, [vp, ip, ip, ip, ip, vp]),
    "sship_lg_debug_capture": (ip, [vp, vp, ip]),
    "sship_lg_debug_stage": (ip, [vp, ip, ip, ip, vp, C.c_ulonglong]),
    "sship_lg_debug_adaptive": (ip, [vp, ip, ip, ip, vp, C.c_ulonglong]),
    "sship_filter_matches": (ip, [vp, vp, ip, vp, vp, vp]),
    "sship_nn_create": (ip, [ip, ip, C.POINTER(vp)]),
    "sship_nn_destroy": (None, [vp]),
    "sship_nn_set_params": (ip, [vp, fp, fp, ip]),
    "sship_nn_get_params": (ip, [vp, C.POINTER(fp), C.POINTER(fp), C.POINTER(ip)]),
    "sship_nn_match_device": (ip, [vp, ip, vp, ip, vp, vp, vp]),
    "sship_nn_match_host": (ip, [vp, ip, vp, ip, vp, vp, vp]),
    "sship_nn_match_batch_device": (ip, [vp, vp, vp, ip, vp, vp, vp]),
    "sship_nn_bench": (ip, [vp, ip, C.POINTER(fp)]),
    "sship_nn_set_gate": (ip, [vp, ip, fp, fp, fp, fp]),
    "sship_nn_get_gate": (ip, [vp, C.POINTER(ip), C.POINTER(fp), C.POINTER(fp), C.POINTER(fp), C.POINTER(fp)]),
    "sship_nn_match_gated_device": (ip, [vp, vp, ip, ip, vp, vp, ip, ip, vp, vp, vp]),
    "sship_nn_match_gated_host": (ip, [vp, vp, ip, ip, vp, vp, ip, ip, vp, vp, vp]),
    "sship_nn_match_gated_batch_device": (ip, [vp, vp, vp, vp, ip, vp, vp, vp]),
    "sship_stereo_associate_batch_device": (ip, [vp, vp, vp, ip, ip, fp, fp, vp, vp, vp]),
    "sship_ep_create": (ip, [C.c_char_p, ip, ip, C.POINTER(vp)]),
    "sship_ep_destroy": (None, [vp]),
    "sship_ep_descriptor_dim": (ip, [vp]),
    "sship_ep_infer": (ip, [vp, vp, vp]),
    "sship_ep_preprocess": (ip, [vp, ip, ip, ip, ip, ip, ip, vp]),
    "sship_ep_infer_u8": (ip, [vp, vp, ip, ip, ip, ip, vp]),
    "sship_ep_infer_u8_device": (ip, [vp, vp, ip, ip, ip, ip, vp, vp]),
    "sship_ep_bench": (ip, [vp, vp, ip, ip, ip, ip, ip, C.POINTER(C.c_float)]),
    "sship_ep_debug_capture": (ip, [vp, ip]),
    "sship_ep_debug_activation": (ip, [vp, ip, vp, C.c_ulonglong]),
    "sship_ep_reserve_batch": (ip, [vp, ip]),
    "sship_ep_max_batch": (ip, [vp]),
    "sship_ep_batch_workspace_bytes": (C.c_size_t, [ip, ip, ip]),
    "sship_ep_infer_u8_batch_device": (ip, [vp, vp, ip, ip, ip, ip, C.c_longlong, ip, vp, ip, vp]),
    "sship_ep_infer_u8_batch": (ip, [vp, vp, ip, ip, ip, ip, C.c_longlong, ip, vp]),
    "sship_ep_bench_batch": (ip, [vp, vp, ip, ip, ip, ip, C.c_longlong, ip, ip, C.POINTER(C.c_float)]),
    "sship_ep_debug_capture_image": (ip, [vp, ip]),
    "sship_index_create": (ip, [ip, ip, ip, ip, C.POINTER(vp)]),
    "sship_index_destroy": (None, [vp]),
    "sship_index_dim": (ip, [vp]),
    "sship_index_capacity": (ip, [vp]),
    "sship_index_size": (ip, [vp]),
    "sship_index_clear": (ip, [vp]),
    "sship_index_add_host": (ip, [vp, vp, vp, ip, ip]),
    "sship_index_add_device": (ip, [vp, vp, vp, ip, ip, vp]),
    "sship_index_read": (ip, [vp, ip, ip, vp, vp]),
    "sship_index_query_host": (ip, [vp, vp, ip, ip, fp, vp, vp, C.POINTER(ip)]),
    "sship_index_query_device": (ip, [vp, vp, ip, ip, fp, vp, vp, C.POINTER(ip)]),
    "sship_index_query_batch_device": (ip, [vp, vp, ip, ip, vp, ip, ip, fp, vp, vp, vp, vp]),
    "sship_index_bench": (ip, [vp, ip, C.POINTER(fp)]),
    "sship_pose_create": (ip, [ip, ip, C.POINTER(vp)]),
    "sship_pose_destroy": (None, [vp]),
    "sship_pose_set_camera": (ip, [vp, dp, dp, dp, dp, dp]),
    "sship_pose_get_camera": (ip, [vp, C.POINTER(dp), C.POINTER(dp), C.POINTER(dp), C.POINTER(dp), C.POINTER(dp)]),
    "sship_pose_set_params": (ip, [vp, C.POINTER(PoseParams)]),
    "sship_pose_get_params": (ip, [vp, C.POINTER(PoseParams)]),
    "sship_pose_solve_batch_device": (ip, [vp, vp, vp, vp, vp, ip, vp, vp, vp, vp, vp]),
    "sship_pose_solve_host": (ip, [vp, vp, vp, vp, ip, vp, vp, vp, vp, vp]),
    "sship_pose_obs_from_matches_batch_device": (ip, [vp, vp, vp, vp, vp, vp, vp, vp, ip, ip, vp, vp, vp, vp]),
    "sship_pose_bench": (ip, [vp, ip, C.POINTER(fp)]),
    "sship_ransac_create": (ip, [ip, ip, C.POINTER(vp)]),
    "sship_ransac_destroy": (None, [vp]),
    "sship_ransac_set_camera": (ip, [vp, dp, dp, dp, dp, dp]),
    "sship_ransac_get_camera": (ip, [vp, C.POINTER(dp), C.POINTER(dp), C.POINTER(dp), C.POINTER(dp), C.POINTER(dp)]),
    "sship_ransac_set_params": (ip, [vp, C.POINTER(RansacParams)]),
    "sship_ransac_get_params": (ip, [vp, C.POINTER(RansacParams)]),
    "sship_ransac_solve_batch_device": (ip, [vp, vp, vp, vp, ip, vp, vp, vp, vp, vp]),
    "sship_ransac_solve_host": (ip, [vp, vp, vp, vp, ip, vp, vp, vp, vp]),
    "sship_ransac_bench": (ip, [vp, ip, C.POINTER(fp)]),
    "sship_ba_create": (ip, [ip, ip, ip, ip, C.POINTER(vp)]),
    "sship_ba_destroy": (None, [vp]),
    "sship_ba_set_camera": (ip, [vp, dp, dp, dp, dp, dp]),
    "sship_ba_get_camera": (ip, [vp, C.POINTER(dp), C.POINTER(dp), C.POINTER(dp), C.POINTER(dp), C.POINTER(dp)]),
    "sship_ba_set_params": (ip, [vp, C.POINTER(BaParams)]),
    "sship_ba_get_params": (ip, [vp, C.POINTER(BaParams)]),
    "sship_ba_solve_batch_device": (ip, [vp, vp, vp, vp, vp, ip, vp, vp, vp, vp, vp]),
    "sship_ba_solve_host": (ip, [vp, vp, vp, ip, vp, vp, vp, vp, vp]),
    "sship_ba_tracks_from_matches_batch_device": (ip, [vp, vp, vp, vp, vp, ip, vp, vp]),
    "sship_ba_bench": (ip, [vp, ip, C.POINTER(fp)]),
    "sship_pg_create": (ip, [ip, ip, ip, C.POINTER(vp)]),
    "sship_pg_workspace_slice_bytes": (C.c_size_t, [ip, ip]),
    "sship_pg_destroy": (None, [vp]),
    "sship_pg_set_params": (ip, [vp, C.POINTER(PgParams)]),
    "sship_pg_get_params": (ip, [vp, C.POINTER(PgParams)]),
    "sship_pg_solve_batch_device": (ip, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ip, vp, vp, vp, vp, vp]),
    "sship_pg_solve_host": (ip, [vp, ip, vp, vp, vp, ip, vp, vp, vp, vp, vp, vp, vp, vp]),
    "sship_pg_odometry_from_poses_batch_device": (ip, [vp, vp, ip, vp, vp]),
    "sship_pg_loops_from_pose_batch_device": (ip, [vp, vp, vp, vp, vp, ip, ip, dp, vp, vp, vp, vp, vp, vp]),
    "sship_pg_bench": (ip, [vp, ip, C.POINTER(fp)]),
    "sship_rect_build_maps": (ip, [vp, vp, ip, vp, vp, ip, ip, vp, vp]),
    "sship_rect_fixed_table": (ip, [vp, vp, C.c_size_t, vp, vp, vp]),
    "sship_rect_create": (ip, [ip, ip, ip, ip, ip, C.POINTER(vp)]),
    "sship_rect_destroy": (None, [vp]),
    "sship_rect_set_maps": (ip, [vp, ip, vp, vp]),
    "sship_rect_set_camera": (ip, [vp, ip, vp, vp, ip, vp, vp]),
    "sship_rect_read_table": (ip, [vp, ip, vp, vp, vp]),
    "sship_rect_tile_paths": (ip, [vp, ip, C.POINTER(ip), C.POINTER(ip)]),
    "sship_rect_remap_batch_device": (ip, [vp, vp, ip, ip, vp, vp]),
    "sship_rect_remap_host": (ip, [vp, ip, vp, ip, vp]),
    "sship_rect_bench": (ip, [vp, ip, ip, ip, C.POINTER(fp)]),
    "sship_rgbd_associate_batch_device": (ip, [vp, vp, ip, ip, vp, ip, ip, ip, ip, C.POINTER(RgbdParams), vp, vp, vp, vp]),
    "sship_rgbd_associate_host": (ip, [vp, ip, ip, vp, ip, ip, ip, ip, C.POINTER(RgbdParams), vp, vp, vp]),
    "sship_stereo_refine_batch_device": (ip, [vp, ip, ip, ip, ip, vp, vp, vp, ip, ip, C.POINTER(StereoRefineParams), vp, vp, vp, vp, vp]),
    "sship_stereo_refine_host": (ip, [vp, ip, vp, ip, ip, ip, vp, vp, ip, C.POINTER(StereoRefineParams), vp, vp, vp, vp]),
    "sship_stereo_search_batch_device": (ip, [vp, ip, ip, ip, ip, vp, vp, ip, ip, C.POINTER(StereoSearchParams), vp, vp, vp, vp, vp]),
    "sship_stereo_search_host": (ip, [vp, ip, vp, ip, ip, ip, vp, ip, ip, C.POINTER(StereoSearchParams), vp, vp, vp, vp]),
    "sship_patch_track_batch_device": (ip, [vp, C.c_longlong, ip, vp, C.c_longlong, ip, ip, ip, ip, vp, vp, ip, vp, ip,
                                            C.POINTER(PatchTrackParams), vp, vp, vp, vp, vp, vp]),
    "sship_patch_track_host": (ip, [vp, ip, vp, ip, ip, ip, vp, ip, vp, ip, ip, C.POINTER(PatchTrackParams), vp, vp, vp, vp]),
    "sship_pyr_create": (ip, [ip, ip, ip, ip, C.POINTER(vp)]),
    "sship_pyr_destroy": (None, [vp]),
    "sship_pyr_build_batch_device": (ip, [vp, vp, C.c_longlong, ip, ip, vp]),
    "sship_pyr_level": (ip, [vp, ip, C.POINTER(vp), C.POINTER(ip), C.POINTER(ip), C.POINTER(ip), C.POINTER(C.c_longlong), C.POINTER(ip)]),
    "sship_pyr_read_level": (ip, [vp, ip, ip, ip, vp, ip]),
    "sship_pyr_down_host": (ip, [vp, ip, ip, ip, vp, ip]),
    "sship_pyr_bench": (ip, [vp, ip, C.POINTER(fp)]),
    "sship_patch_track_pyramid_batch_device": (ip, [vp, ip, ip, vp, ip, ip, ip, vp, vp, ip, vp, ip, C.POINTER(PyrTrackParams), vp, vp, vp, vp,
                                                    vp, vp, vp]),
    "sship_patch_track_pyramid_host": (ip, [vp, ip, vp, ip, ip, ip, vp, ip, vp, ip, ip, C.POINTER(PyrTrackParams), vp, vp, vp, vp, vp]),
    "sship_clahe_create": (ip, [ip, ip, ip, ip, dp, ip, C.POINTER(vp)]),
    "sship_clahe_destroy": (None, [vp]),
    "sship_clahe_set_clip_limit": (ip, [vp, dp]),
    "sship_clahe_get_params": (ip, [vp, C.POINTER(ip), C.POINTER(ip), C.POINTER(ip), C.POINTER(ip), C.POINTER(dp), C.POINTER(ip)]),
    "sship_clahe_apply_batch_device": (ip, [vp, vp, C.c_longlong, ip, vp, C.c_longlong, ip, ip, vp]),
    "sship_clahe_read_luts": (ip, [vp, ip, ip, vp]),
    "sship_clahe_apply_host": (ip, [vp, ip, ip, ip, ip, ip, dp, vp, ip]),
    "sship_clahe_bench": (ip, [vp, ip, C.POINTER(fp)]),
    "sship_clahe_bench_kernels": (ip, [vp, ip, ip, C.POINTER(fp)]),
    "sship_fast_create": (ip, [ip, ip, ip, ip, C.POINTER(vp)]),
    "sship_fast_destroy": (None, [vp]),
    "sship_fast_set_params": (ip, [vp, C.POINTER(FastParams)]),
    "sship_fast_get_params": (ip, [vp, C.POINTER(FastParams), C.POINTER(ip), C.POINTER(ip), C.POINTER(ip), C.POINTER(ip)]),
    "sship_fast_detect_batch_device": (ip, [vp, vp, C.c_longlong, ip, ip, vp, vp, ip, vp, vp, vp, vp, vp]),
    "sship_fast_detect_host": (ip, [vp, ip, ip, ip, ip, C.POINTER(FastParams), vp, ip, ip, vp, vp, vp, vp]),
    "sship_fast_score_batch_device": (ip, [vp, C.c_longlong, ip, ip, ip, ip, vp, C.c_longlong, ip, vp]),
    "sship_fast_bench": (ip, [vp, ip, C.POINTER(fp)]),
    "sship_fast_bench_kernels": (ip, [vp, ip, ip, C.POINTER(fp)]),
    "sship_brief_pattern": (ip, [ip, vp]),
    "sship_brief_describe_batch_device": (ip, [vp, C.c_longlong, ip, ip, ip, ip, vp, vp, ip, ip, ip, vp, vp, vp, vp]),
    "sship_brief_describe_host": (ip, [vp, ip, ip, ip, vp, ip, ip, ip, vp, vp, vp]),
    "sship_hm_create": (ip, [ip, ip, C.POINTER(vp)]),
    "sship_hm_destroy": (None, [vp]),
    "sship_hm_set_params": (ip, [vp, ip, ip, ip]),
    "sship_hm_get_params": (ip, [vp, C.POINTER(ip), C.POINTER(ip), C.POINTER(ip), C.POINTER(ip), C.POINTER(ip)]),
    "sship_hm_set_gate": (ip, [vp, ip, fp, fp, fp, fp]),
    "sship_hm_get_gate": (ip, [vp, C.POINTER(ip), C.POINTER(fp), C.POINTER(fp), C.POINTER(fp), C.POINTER(fp)]),
    "sship_hm_match_batch_device": (ip, [vp, vp, vp, vp, vp, ip, ip, ip, ip, ip, vp, vp, vp, vp]),
    "sship_hm_match_host": (ip, [vp, ip, vp, vp, vp, ip, ip, vp, vp, vp, ip, vp, vp, vp]),
    "sship_hm_bench": (ip, [vp, ip, C.POINTER(fp)]),
    "sship_desc_to_host": (ip, [vp, ip, ip, vp]),
    "sship_frontend_batch_device": (ip, [vp, vp, vp, ip, ip, ip, vp, vp, vp, vp, vp, vp]),
    "sship_sp_bench_layer": (ip, [vp, ip, ip, ip, ip, ip, C.POINTER(fp), C.POINTER(C.c_double)]),
    "sship_lg_bench_stage": (ip, [vp, ip, ip, C.POINTER(fp)]),
    "sship_mfma_probe": (ip, [ip, C.POINTER(fp)]),
    "sship_set_profiling": (None, [ip]),
    "sship_get_stage_timings": (ip, [C.POINTER(C.c_char_p), C.POINTER(fp), ip]),
    "sship_set_log_callback": (None, [vp]),
    "sship_comm_unique_id": (ip, [vp]),
    "sship_comm_create": (ip, [vp, ip, ip, C.POINTER(vp)]),
    "sship_comm_destroy": (None, [vp]),
    "sship_comm_rank": (ip, [vp]),
    "sship_comm_world": (ip, [vp]),
    "sship_gather_features_rccl": (ip, [vp, vp, vp, vp, ip, ip, vp, vp, vp, vp]),
}


def lib():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SshipError(ERR_IO, f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                     "(hipcc --offload-arch=gfx950); there is no fallback path")
        # ONE HIP runtime per process: torch bundles its own libamdhip64 / libhsa-runtime64, and a second
        # copy (the system one this library was linked against) cannot initialise the GPU once the first has.
        # Importing torch first makes the dynamic loader resolve our DT_NEEDED libamdhip64.so.7 to the copy
        # torch already mapped (same SONAME), exactly like a torch.utils.cpp_extension module.
        import torch  # noqa: F401  (device-memory / stream plumbing only)

        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc: int) -> None:
    if rc != OK:
        raise SshipError(rc, (lib().sship_last_error() or b"").decode(errors="replace"))


_inited = False


def init(device: int = -1) -> None:
    """Select the device (SUPERSLAM_HIP_DEVICE / LOCAL_RANK aware).  Raises SshipError without a GPU."""
    global _inited
    if device < 0 and "SUPERSLAM_HIP_DEVICE" not in os.environ and "LOCAL_RANK" in os.environ:
        device = int(os.environ["LOCAL_RANK"])
    check(lib().sship_init(device))
    _inited = True


def stage_timings() -> dict:
    labels = (C.c_char_p * 32)()
    ms = (fp * 32)()
    n = lib().sship_get_stage_timings(labels, ms, 32)
    return {labels[i].decode(): ms[i] for i in range(n)}
