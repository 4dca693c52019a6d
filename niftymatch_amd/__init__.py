"""niftymatch_amd -- MI355X (gfx950) drop-in for NiftyMatch's SIFT detect/describe + brute-force L2 match path.

The product is the HIP library niftymatch_amd/lib/libnm_hip.so (C ABI: include/nm_abi.h) and the C++ headers under
niftymatch_amd/nm/ that mirror the reference's API. This Python module is host plumbing for tests, bench.py and the
multi-GPU launcher: it binds the C ABI with ctypes and uses torch only for device memory, streams and
torch.distributed. There is NO CPU fallback: if the library is missing, every entry point raises.
"""
import collections
import ctypes as C
import math
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libnm_hip.so")
# A/B diagnostics (tools/build_variant.py builds libraries with pieces compiled out: wrong results by design). A stray
# NM_HIP_LIB alone must never redirect the product or its tests, so the override also needs NM_DIAGNOSTIC=1.
if os.environ.get("NM_HIP_LIB"):
    if os.environ.get("NM_DIAGNOSTIC") != "1":
        raise RuntimeError("NM_HIP_LIB is set without NM_DIAGNOSTIC=1: refusing to load a diagnostic library build")
    LIB_PATH = os.environ["NM_HIP_LIB"]
_lib = None

_F = C.c_float
_I = C.c_int
_P = C.c_void_p
_SZ = C.c_size_t

_SIGNATURES = {
    "DivUp": (_I, [_I, _I]), "DivDown": (_I, [_I, _I]), "AlignUp": (_I, [_I, _I]), "AlignDown": (_I, [_I, _I]),
    "nm_version": (C.c_char_p, []), "nm_device_count": (_I, [_P]), "nm_set_device": (_I, [_I]),
    "nm_error_string": (C.c_char_p, [_I]),
    "nm_fill_u32": (_I, [_P, _SZ, C.c_uint, _P]),
    "nm_profile_events": (_I, [_I, _P, _P]),
    "nm_create_kernel_for_sigma": (_I, [_F, _P]),
    "nm_convolve_f32": (_I, [_P, _P, _P, _I, _I, _P, _I, _P]),
    "nm_conv_route_of": (_I, [_I, _I, _I, _I, _I, _I, _I, C.c_uint, C.c_uint]),
    "nm_downsample2_f32": (_I, [_P, _I, _I, _P, _I, _I, _P]),
    "nm_subtract_f32": (_I, [_P, _P, _P, _I, _I, _P]),
    "nm_gradient_f32": (_I, [_P, _P, _I, _I, _P]),
    "nm_find_keypoints_f32": (_I, [_P, _P, _P, _I, _I, _F, _F, _F, _F, _I, _I, _P, _P]),
    "nm_find_keypoints_masked_f32": (_I, [_P, _P, _I, _I, _P, _P, _I, _I, _F, _F, _F, _F, _I, _I, _P, _P]),
    "nm_subtract_batch_f32": (_I, [_I, _P, _P, _P, _I, _I, _P]),
    "nm_gradient_batch_f32": (_I, [_I, _P, _P, _I, _I, _P]),
    "nm_find_keypoints3_f32": (_I, [_P, _P, _I, _I, _I, _I, _F, _F, _F, _F, _I, _P, _P]),
    "nm_find_keypoints3_reset_f32": (_I, [_P, _P, _I, _I, _I, _I, _F, _F, _F, _F, _I, _P, _P, _P]),
    "nm_find_keypoints3_compact_workspace_bytes": (_SZ, [_I, _I]),
    "nm_find_keypoints3_compact_f32": (_I, [_P, _I, _I, _F, _F, _F, _F, _I, _I, _P, _P, _P, _P]),
    "nm_compact3_workspace_bytes": (_SZ, [_I]),
    "nm_compact_keypoints3": (_I, [_P, _I, _P, _P, _P, _P]),
    "nm_detect_orientations_levels": (_I, [_I, _P, _P, _P, _I, _I, _F, _F, _P, _P]),
    "nm_compute_sift_descriptors_levels": (_I, [_I, _P, _P, _P, _P, _I, _I, _I, _F, _P, _P, _P, _P]),
    "nm_detect_orientations_levels_dev": (_I, [_P, _P, _I, _P, _I, _I, _F, _F, _P, _P, _P]),
    "nm_compute_sift_descriptors_levels_dev": (_I, [_P, _P, _P, _I, _P, _I, _I, _P, _P, _P, _I, _I, _I, _F, _P, _P, _P, _P]),
    "nm_compact_workspace_bytes": (_SZ, [_I]),
    "nm_compact_keypoints": (_I, [_P, _I, _P, _P, _P, _P]),
    "nm_detect_orientations": (_I, [_P, _P, _I, _I, _I, _F, _F, _P, _P]),
    "nm_compute_sift_descriptors": (_I, [_P, _P, _P, _I, _I, _I, _I, _F, _P, _P, _P, _P]),
    "nm_transpose_f32": (_I, [_P, _P, _I, _I, _P]),
    "nm_bf_distance_f32": (_I, [_P, _I, _P, _I, _I, _P, _P]),
    "nm_get_sift_matches_f32": (_I, [_P, _I, _I, _I, _P, _F, _P]),
    "nm_sift_match_plan": (_I, [_I, _I, _P]),
    "nm_sift_match_plan_segments": (_I, [_I, _I, _I, _P, _I]),
    "nm_sift_match_plan_on": (_I, [_I, _I, _I, _I, _P]),
    "nm_sift_match_plan_segments_on": (_I, [_I, _I, _I, _I, _I, _P, _I]),
    "nm_profile_event_pairs": (_I, [_I, _P, _I]),
    "nm_sift_match_batch_workspace_bytes": (_SZ, [_I, _P, _P]),
    "nm_sift_match_batch_f32": (_I, [_I, _P, _P, _P, _P, _P, _F, _P, _P]),
    "nm_sift_match_batch_dev_workspace_bytes": (_SZ, [_I, _I, _I]),
    "nm_sift_match_batch_dev_f32": (_I, [_I, _P, _P, _P, _P, _I, _I, _P, _F, _P, _P]),
    "nm_sift_match_batch_dev_phases_f32": (_I, [_I, _I, _P, _P, _P, _P, _I, _I, _P, _F, _P, _P]),
    "nm_sift_match_workspace_bytes": (_SZ, [_I, _I]),
    "nm_sift_match_set_screen": (_I, [_I]),
    "nm_sift_match_get_screen": (_I, []),
    "nm_sift_match_pairs_per_launch": (_I, [_I]),
    "nm_sift_match_set_distance_mode": (_I, [_I]),
    "nm_sift_set_detect_tall_min": (_I, [_I]),
    "nm_sift_set_frame_skew": (_I, [_I]),
    "nm_sift_match_get_distance_mode": (_I, []),
    "nm_sift_match_distance_listed": (_I, [_P, _I, _I, _P, _P, _P]),
    "nm_sift_match_f32": (_I, [_P, _I, _P, _I, _P, _P, _F, _P, _P]),
    "nm_sift_match_fallback_count": (_I, [_P, _I, _I, _P, _P]),
    "nm_sift_match_second_pass_count": (_I, [_P, _I, _I, _P, _P]),
    "nm_sift_match_shard_f32": (_I, [_P, _I, _P, _I, _I, _P, _P, _P, _P, _P]),
    "nm_sift_match_merge_f32": (_I, [_P, _P, _P, _I, _I, _P, _F, _P]),
    "nm_sift_match_merge_packed_f32": (_I, [_P, _I, _I, _P, _F, _P]),
    "nm_sift_match_allgather_workspace_bytes": (_SZ, [_I, _I, _I]),
    "nm_sift_match_allgather_f32": (_I, [_P, _I, _P, _I, _I, _I, _P, _F, _P, _P, _P]),
    "nm_grayscale_f32": (_I, [_P, _P, _I, _I, _P]),
    "nm_extract_channel_f32": (_I, [_P, _P, _I, _I, _I, _P]),
    "nm_put_channel_f32": (_I, [_P, _P, _I, _I, _I, _P]),
    "nm_set_alpha_to_const": (_I, [_P, _I, _I, C.c_ubyte, _P]),
    "nm_cast_f32_u8": (_I, [_P, _SZ, _SZ, _P, C.c_ubyte, _P]),
    "nm_downsample2_u8x4": (_I, [_P, _I, _I, _P, _I, _I, _P]),
    "nm_align_points": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "nm_selftest_sqrt": (_I, [_P, _P]),
    "nm_selftest_expw": (_I, [_P, _P]),
    "nm_selftest_orient": (_I, [_P, _P]),
    "nm_selftest_mfma_model": (_I, [_I, _I, _I, _P, _P]),
    "nm_sift_match_accum_budget": (_F, [_I]),
    "nm_selftest_mfma_f32": (_I, [_I, _I, _P, _P]),
    "nm_sift_match_distance_budget": (_F, []),
    "nm_undistort_map_f32": (_I, [_P, _P, _SZ, _SZ, _P, _P, _P, _P, _P]),
    "nm_resample_undistort_f32": (_I, [_P, _I, _I, _I, _P, _P, _SZ, _SZ, _P, _P]),
    "nm_resample_mask_u8": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _F, _P]),
    "nm_resample_perspective_u8x4": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _P]),
    "nm_resample_map_u8x4": (_I, [_P, _P, _I, _I, _P, _P, _I, _I, _P]),
    "nm_transform_blend": (_I, [_P, _I, _I, _P, _I, _I, _I, _I, _P, _I, _I, _P, _I, _P, _P, _I, _P]),
    "nm_ransac_f32": (_I, [_I, _P, _P, _P, _P, _I, _P, _I, _F, _P, _P, _P, _P, _P]),
    "nm_ransac_seed": (None, [C.c_uint]),
    "nm_ransac_batch_dev_workspace_bytes": (_SZ, [_I, _I, _I]),
    "nm_ransac_batch_dev_f32": (_I, [_I, _I, _P, _P, _P, _I, _P, _P, _P, _I, _F, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "nm_ransac_batch_sample": (_I, [C.c_uint, _I, _I, _I, _I]),
    "nm_ransac_refit_batch_dev_f32": (_I, [_I, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P, _F, _I, _P, _P, _P, _P, _P, _P, _P]),
    "nm_ransac_refit_host_f32": (_I, [_I, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P, _F, _I, _P, _P, _P, _P, _P, _P]),
    "nm_link_verify_workspace_bytes": (_SZ, [_I]),
    "nm_link_verify_batch_dev_f32": (_I, [_I, _P, _P, _I, _I, _P, _P, _P, _P, _I, _I, _F, _F, _F, _P, _P, _P, _P, _P]),
    "nm_link_verify_host_f32": (_I, [_I, _P, _P, _I, _I, _P, _P, _P, _P, _I, _I, _F, _F, _F, _P, _P, _P]),
    "nm_link_verify_sums_host_f32": (_I, [_I, _P, _P, _I, _I, _P, _P, _I, _P]),
    "nm_link_refine_workspace_bytes": (_SZ, [_I]),
    "nm_link_refine_batch_dev_f32": (_I, [_I, _P, _P, _I, _I, _P, _P, _P, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P]),
    "nm_link_refine_host_f32": (_I, [_I, _P, _P, _I, _I, _P, _P, _P, _I, _I, _I, _I, _F, _P, _P, _P]),
    "nm_link_refine_sums_host_f32": (_I, [_I, _P, _P, _I, _I, _P, _P, _I, _P]),
    "nm_sift_match_guided_batch_dev_f32": (_I, [_I, _P, _P, _P, _P, _I, _P, _P, _P, _P, _I, _P, _P, _F, _F, _F, _P, _P, _P, _P]),
    "nm_sift_match_guided_host_f32": (_I, [_I, _P, _P, _P, _P, _I, _P, _P, _P, _P, _I, _P, _P, _F, _F, _F, _P, _P, _P]),
    "nm_sift_match_mutual_workspace_bytes": (_SZ, [_I, _I]),
    "nm_sift_match_mutual_batch_dev_f32": (_I, [_I, _P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P]),
    "nm_sift_match_mutual_host_f32": (_I, [_I, _P, _P, _I, _P, _P, _I, _P, _P, _P, _P]),
    "nm_sift_desc_finish_batch_dev": (_I, [_I, _P, _P, _I, _P, _P, _I, _P]),
    "nm_sift_desc_finish_host": (_I, [_I, _P, _P, _I, _P, _P, _I]),
    "nm_sift_select_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "nm_sift_select_batch_dev": (_I, [_I] * 7 + [_P] * 18),
    "nm_sift_select_host": (_I, [_I] * 7 + [_P] * 16),
    "nm_sift_match_u8_workspace_bytes": (_SZ, [_I, _I, _I]),
    "nm_sift_match_u8_batch_dev": (_I, [_I, _P, _P, _I, _P, _P, _I, _P, _F, _P, _P]),
    "nm_sift_match_u8_host": (_I, [_I, _P, _P, _I, _P, _P, _I, _P, _F]),
    "nm_sift_match_knn_u8_workspace_bytes": (_SZ, [_I, _I, _I]),
    "nm_sift_match_knn_u8_batch_dev": (_I, [_I, _P, _P, _I, _P, _P, _I, _I, _P, _P, _P, _P]),
    "nm_sift_match_knn_u8_host": (_I, [_I, _P, _P, _I, _P, _P, _I, _I, _P, _P]),
    "nm_sift_match_mutual_u8_workspace_bytes": (_SZ, [_I, _I, _I]),
    "nm_sift_match_mutual_u8_batch_dev": (_I, [_I, _P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P]),
    "nm_sift_match_mutual_u8_host": (_I, [_I, _P, _P, _I, _P, _P, _I, _P, _P, _P, _P]),
    "nm_sift_match_guided_u8_batch_dev": (_I, [_I, _P, _P, _P, _P, _I, _P, _P, _P, _P, _I, _P, _P, _F, _F, _F, _P, _P, _P, _P]),
    "nm_sift_match_guided_u8_host": (_I, [_I, _P, _P, _P, _P, _I, _P, _P, _P, _P, _I, _P, _P, _F, _F, _F, _P, _P, _P]),
    "nm_mosaic_plan_f32": (_I, [_I, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "nm_mosaic_plan_host_f32": (_I, [_I, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "nm_transform_blend_batch": (_I, [_P, _I, _I, _P, _I, _P, _I, _I, _P, _I, _P, _I, _P, _P]),
    "nm_mosaic_place_f32": (_I, [_I, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "nm_mosaic_place_host_f32": (_I, [_I, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "nm_mosaic_adjust_workspace_bytes": (_SZ, [_I, _I]),
    "nm_mosaic_adjust_dev_f32": (_I, [_I, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, C.c_double,
                                      C.c_double, _P, _P, _P, _P, _P, _P]),
    "nm_mosaic_adjust_host_f32": (_I, [_I, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, C.c_double,
                                       C.c_double, _P, _P, _P, _P]),
    "nm_mosaic_adjust_sums_host_f32": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "nm_mosaic_exposure_sums_dev": (_I, [_I, _I, _P, _P, _P, _I, _I, _P, _P, _P, _I, _I, _I, _P, _P]),
    "nm_mosaic_exposure_sums_host": (_I, [_I, _I, _P, _P, _P, _I, _I, _P, _P, _P, _I, _I, _I, _P]),
    "nm_mosaic_gains_dev": (_I, [_I, _I, _P, _P, _P, _P, _I, C.c_double, C.c_double, _F, _F, _I, _P, _P, _P]),
    "nm_mosaic_gains_host": (_I, [_I, _I, _P, _P, _P, _P, _I, C.c_double, C.c_double, _F, _F, _I, _P, _P]),
    "nm_transform_blend_batch_gain": (_I, [_P, _I, _I, _P, _I, _P, _I, _I, _P, _I, _P, _I, _P, _P, _P]),
    "nm_mosaic_bands_workspace_bytes": (_SZ, [_I, C.c_longlong, _I, _I]),
    "nm_mosaic_bands_taps": (_I, [_I, C.c_double, _P]),
    "nm_mosaic_warp_tiles": (_I, [_I, _P, _I, _I, _P, _I, _P, _I, _P, _P, _P, C.c_longlong, _P, _P]),
    "nm_mosaic_bands_dev": (_I, [_I, _P, C.c_longlong, _P, _P, _I, _I, _P, _I, C.c_double, _P, _P]),
    "nm_mosaic_bands_host": (_I, [_I, _P, C.c_longlong, _P, _P, _I, _I, _P, _I, C.c_double, _P]),
    "nm_mosaic_median_dev": (_I, [_I, _P, C.c_longlong, _P, _P, _I, _I, _P, _I, _F, _F, _P, _P, _P, _P]),
    "nm_mosaic_median_host": (_I, [_I, _P, C.c_longlong, _P, _P, _I, _I, _P, _I, _F, _F, _P, _P, _P]),
    "nm_frame_weights_workspace_bytes": (_SZ, [_I, _I, _I]),
    "nm_frame_weights_batch_dev": (_I, [_I, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P]),
    "nm_frame_weights_host": (_I, [_I, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P]),
    "nm_frame_weights_set_grid_cap": (_I, [_I]),
    "nm_frame_quality_batch_dev": (_I, [_I, _P, _I, _I, _P, _I, _I, _I, _I, _I, _P, _P]),
    "nm_frame_quality_host": (_I, [_I, _P, _I, _I, _P, _I, _I, _I, _I, _I, _P]),
    "nm_frame_quality_set_grid_cap": (_I, [_I]),
    "nm_keyframe_pick_dev": (_I, [_I, _P, _I, _I, _P, _P, _I, _I, _I, C.c_longlong, C.c_longlong, C.c_double, C.c_double, _I, _F,
                                  _F, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "nm_keyframe_pick_host": (_I, [_I, _P, _I, _I, _P, _P, _I, _I, _I, C.c_longlong, C.c_longlong, C.c_double, C.c_double, _I, _F,
                                   _F, _I, _P, _P, _P, _P, _P, _P, _P]),
    "nm_slots_gather_dev": (_I, [_I, _P, _I, _P, _P, C.c_longlong, _I, _P]),
    "nm_slots_gather_host": (_I, [_I, _P, _I, _P, _P, C.c_longlong, _I]),
    "nm_gray_pyramid_floats": (_SZ, [_I, _I, _I]),
    "nm_gray_pyramid_offset": (_SZ, [_I, _I, _I]),
    "nm_gray_pyramid_batch_f32": (_I, [_I, _P, _I, _I, _I, _P, _P, _P, _P]),
    "nm_gray_pyramid_host_f32": (_I, [_I, _P, _I, _I, _I, _P, _P, _P]),
    "nm_klt_track_batch_dev_f32": (_I, [_I, _P, _P, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _I, _I, _F, _F, _F, _F, _F, _P, _P, _P,
                                        _P, _P, _P, _P, _P]),
    "nm_klt_track_host_f32": (_I, [_I, _P, _P, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _I, _I, _F, _F, _F, _F, _F, _P, _P, _P, _P,
                                   _P, _P, _P]),
    "nm_klt_sums_host": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, C.c_double, C.c_double, C.c_double, C.c_double, _P, _P]),
    "nm_klt_set_grid_cap": (_I, [_I]),
    "nm_klt_set_lanes": (_I, [_I]),
    "nm_klt_corners_workspace_bytes": (_SZ, [_I, _I, _I]),
    "nm_klt_corners_batch_dev_f32": (_I, [_I, _P, _I, _I, _P, _P, _P, _P, _I, _I, _I, _F, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "nm_klt_corners_host_f32": (_I, [_I, _P, _I, _I, _P, _P, _P, _P, _I, _I, _I, _F, _I, _P, _P, _P, _P, _P, _P]),
    "nm_klt_corners_set_grid_cap": (_I, [_I]),
    "nm_link_votes_workspace_bytes": (_SZ, [_I, _I]),
    "nm_link_votes_dev_u8": (_I, [_I, _P, _P, _I, _F, _P, _P, _P]),
    "nm_link_votes_host_u8": (_I, [_I, _P, _P, _I, _F, _P]),
    "nm_link_votes_set_split": (_I, [_I]),
    "nm_link_rank_dev": (_I, [_I, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "nm_link_rank_host": (_I, [_I, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "nm_frame_ingest_batch_f32": (_I, [_I, _P, _I, _I, _P, _P, _I, _I, _P, _P, _P]),
    "nm_sift_arena_create": (_I, [_I, _I, _I, _P]),
    "nm_sift_arena_destroy": (None, [_P]),
    "nm_sift_arena_bytes": (_SZ, [_P]),
    "nm_sift_arena_tail_trace": (_I, [_P, _P, _I, _P, _I]),
    "nm_sift_arena_tail_segments": (_I, [_P]),
    "nm_sift_arena_tail_status": (_I, [_P, _P, _P]),
    "nm_sift_arena_tail_inject_error": (_I, [_P]),
    "nm_sift_arena_launches_per_call": (_I, [_P, _I]),
    "nm_sift_tail_plan": (_I, [_I, _I, _I, _P, _I, _P]),
    "nm_sift_frame_plan": (_I, [_I, _I, _I, _I, _I, _P, _I]),
    "nm_sift_frame_resolve": (_I, [_I, _I, _I, _I, _I, _I, _P]),
    "nm_sift_frame_cross_min_frames": (_I, []),
    "nm_sift_arena_set_params": (_I, [_P, _F, _F]),
    "nm_sift_arena_get_params": (_I, [_P, _P, _P]),
    "nm_sift_arena_set_mask": (_I, [_P, _P, _I, _I]),
    "nm_sift_detect_describe": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "nm_sift_detect_describe_batch": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "nm_sift_scale_space_batch": (_I, [_P, _I, _P, _P]),
    "nm_sift_scale_space_batch_ex": (_I, [_P, _I, _P, _I, _P]),
    "nm_sift_arena_level": (_P, [_P, _I]), "nm_sift_arena_dog": (_P, [_P, _I]), "nm_sift_arena_grad": (_P, [_P]),
    "nm_sift_octave_pyramid": (_I, [_P, _I, _I, _P]),
    "nm_client_detect_describe": (_I, [_P, _I, _I, _I, _P, _P, _P]),
    "nm_client_match": (_I, [_P, _I, _P, _I, _P, _P, _F]),
    "nm_client_copy_semantics": (_I, [_P, _I, _I, _I]),
    "nm_client_lazy_counts": (_I, [_P, _I, _I, _I, _P, _I, _P]),
    "nm_client_dense_level_keypoints": (_I, [_P, _I, _I, _I, _F, _P, _P, _P, _P]),
    "nm_client_pair_loop_ex": (C.c_double, [_P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "nm_client_pair_loop": (C.c_double, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "nm_client_ransac": (_I, [_I, _P, _P, _P, _P, _I, _F, _I, C.c_uint, _P]),
}

ABI_SYMBOLS = tuple(k for k in _SIGNATURES if not k.startswith("nm_client_"))


class NmError(RuntimeError):
    pass


def lib():
    """Load libnm_hip.so (built by `python -m niftymatch_amd.build`). Fails loudly when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NmError("libnm_hip.so not found at %s: build it with `python -m niftymatch_amd.build` "
                          "(there is no CPU fallback)" % LIB_PATH)
        # torch bundles its own HIP runtime (same SONAME libamdhip64.so.7). Import it FIRST so that the dynamic loader
        # binds libnm_hip.so to that copy: two HIP runtimes in one process cannot both own the device.
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(status, what):
    if status != 0:
        raise NmError("%s failed: (%d) %s" % (what, status, lib().nm_error_string(status).decode()))


def _torch():
    import torch
    return torch


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def _dev(t, dtype=None):
    torch = _torch()
    if not t.is_cuda:
        raise NmError("expected a device tensor")
    if dtype is not None and t.dtype != dtype:
        raise NmError("expected dtype %s, got %s" % (dtype, t.dtype))
    if not t.is_contiguous():
        raise NmError("expected a contiguous tensor")
    return t.data_ptr()


PROF_MATCH_TOP2 = 0
PROF_PYRAMID_O0 = 1
PROF_DESCRIBE = 2
PROF_ORIENT = 3
PROF_DETECT_O0 = 4
PROF_DISTANCE = 5


def profile_events(site, start=None, stop=None):
    """Register (torch.cuda.Event, torch.cuda.Event) to be recorded around a kernel site; None clears."""
    _check(lib().nm_profile_events(site, start.cuda_event if start is not None else None,
                                   stop.cuda_event if stop is not None else None), "nm_profile_events")


def profile_event_pairs(site, pairs):
    """pairs: list of (start, stop) torch.cuda.Event, consumed one per launch of the site; [] clears. The returned ctypes
    array must stay alive until the hook is cleared."""
    n = len(pairs)
    arr = (C.c_void_p * (2 * n))(*[e.cuda_event for p in pairs for e in p]) if n else None
    _check(lib().nm_profile_event_pairs(site, arr, n), "nm_profile_event_pairs")
    return arr


def create_kernel_for_sigma(sigma):
    """Host taps of PyramidData::create_kernel_for_sigma -> (numpy float32 taps, radius)."""
    import numpy as np
    r = lib().nm_create_kernel_for_sigma(sigma, None)
    taps = np.zeros(2 * r + 1, np.float32)
    lib().nm_create_kernel_for_sigma(sigma, taps.ctypes.data)
    return taps, r


# ---- stage wrappers (device tensors in, device tensors out) ----------------------------------------------------
def convolve(image, taps_dev, radius, want_buffer=False):
    torch = _torch()
    h, w = image.shape
    out = torch.empty_like(image)
    buf = torch.empty_like(image)
    _check(lib().nm_convolve_f32(_dev(out), _dev(image, torch.float32), _dev(buf), w, h, _dev(taps_dev), radius,
                                 _stream()), "nm_convolve_f32")
    return (out, buf) if want_buffer else out


def downsample2(src, rw, rh):
    torch = _torch()
    sh, sw = src.shape
    out = torch.empty((rh, rw), dtype=torch.float32, device=src.device)
    _check(lib().nm_downsample2_f32(_dev(out), rw, rh, _dev(src, torch.float32), sw, sh, _stream()), "nm_downsample2_f32")
    return out


def subtract(a, b):
    torch = _torch()
    out = torch.empty_like(a)
    _check(lib().nm_subtract_f32(_dev(a, torch.float32), _dev(b, torch.float32), _dev(out), a.shape[1], a.shape[0],
                                 _stream()), "nm_subtract_f32")
    return out


def gradient(src):
    torch = _torch()
    h, w = src.shape
    out = torch.empty((h, w, 2), dtype=torch.float32, device=src.device)
    _check(lib().nm_gradient_f32(_dev(src, torch.float32), _dev(out), w, h, _stream()), "nm_gradient_f32")
    return out


def find_keypoints(cur, dn, up, peak, edge, xper, sigma0, num_dogs, level, mask=None):
    torch = _torch()
    h, w = cur.shape
    res = torch.full((h, w, 4), -1.0, dtype=torch.float32, device=cur.device)
    if mask is None:
        _check(lib().nm_find_keypoints_f32(_dev(cur), _dev(dn), _dev(up), w, h, peak, edge, xper, sigma0, num_dogs,
                                           level, _dev(res), _stream()), "nm_find_keypoints_f32")
    else:
        mh, mw = mask.shape
        _check(lib().nm_find_keypoints_masked_f32(_dev(cur), _dev(mask, torch.float32), mw, mh, _dev(dn), _dev(up), w,
                                                  h, peak, edge, xper, sigma0, num_dogs, level, _dev(res), _stream()),
               "nm_find_keypoints_masked_f32")
    return res


def compact_keypoints(dense):
    torch = _torch()
    flat = dense.reshape(-1, 4)
    n = flat.shape[0]
    out = torch.full_like(flat, -1.0)
    cnt = torch.zeros(1, dtype=torch.int32, device=dense.device)
    ws = torch.empty(lib().nm_compact_workspace_bytes(n) + 16, dtype=torch.uint8, device=dense.device)
    _check(lib().nm_compact_keypoints(_dev(flat), n, _dev(out), _dev(cnt), _dev(ws), _stream()), "nm_compact_keypoints")
    return out[: int(cnt.item())]


def detect_orientations(kpts, grad, ow, oh, gauss_factor, xper):
    torch = _torch()
    n = kpts.shape[0]
    res = torch.full((n, 2), -1.0, dtype=torch.float32, device=kpts.device)
    _check(lib().nm_detect_orientations(_dev(kpts, torch.float32), _dev(grad, torch.float32), n, ow, oh, gauss_factor,
                                        xper, _dev(res), _stream()), "nm_detect_orientations")
    return res


def compute_sift_descriptors(kpts, orients, grad, ow, oh, num_dogs, xper):
    torch = _torch()
    n = kpts.shape[0]
    desc = torch.zeros((n, 128), dtype=torch.float32, device=kpts.device)
    x = torch.zeros(n, dtype=torch.float32, device=kpts.device)
    y = torch.zeros(n, dtype=torch.float32, device=kpts.device)
    _check(lib().nm_compute_sift_descriptors(_dev(kpts), _dev(orients), _dev(grad), n, ow, oh, num_dogs, xper,
                                             _dev(desc), _dev(x), _dev(y), _stream()), "nm_compute_sift_descriptors")
    return desc, x, y


def transpose(a):
    torch = _torch()
    h, w = a.shape
    out = torch.empty((w, h), dtype=torch.float32, device=a.device)
    _check(lib().nm_transpose_f32(_dev(out), _dev(a, torch.float32), w, h, _stream()), "nm_transpose_f32")
    return out


def bf_distance(At, B):
    torch = _torch()
    dim, na = At.shape
    nb = B.shape[0]
    D = torch.empty((nb, na), dtype=torch.float32, device=At.device)
    _check(lib().nm_bf_distance_f32(_dev(At, torch.float32), na, _dev(B, torch.float32), nb, dim, _dev(D), _stream()),
           "nm_bf_distance_f32")
    return D


def get_sift_matches(distance, ambiguity=0.8, prior=None, cols=None):
    torch = _torch()
    rows, bw = distance.shape
    cols = bw if cols is None else cols
    res = torch.full((rows,), -1, dtype=torch.int32, device=distance.device) if prior is None else prior.clone()
    _check(lib().nm_get_sift_matches_f32(_dev(distance, torch.float32), rows, cols, bw, _dev(res, torch.int32),
                                         ambiguity, _stream()), "nm_get_sift_matches_f32")
    return res


class MatchWorkspace:
    """Device scratch of the fused matcher, sized for (nA, nB); reusable across calls of at most that size."""

    def __init__(self, nA, nB, device):
        torch = _torch()
        self.nA, self.nB = nA, nB
        self.buf = torch.empty(lib().nm_sift_match_workspace_bytes(nA, nB) + 256, dtype=torch.uint8, device=device)


def sift_match(A, B, ambiguity=0.8, want_distance=False, prior=None, workspace=None, nA=None, nB=None):
    """compute_sift_matches on raw descriptor tensors (n x 128). Returns (result int32[nA], distance or None)."""
    torch = _torch()
    nA = A.shape[0] if nA is None else nA
    nB = B.shape[0] if nB is None else nB
    ws = workspace or MatchWorkspace(nA, nB, A.device)
    D = torch.empty((nA, nB), dtype=torch.float32, device=A.device) if want_distance else None
    res = torch.full((nA,), -1, dtype=torch.int32, device=A.device) if prior is None else prior
    _check(lib().nm_sift_match_f32(_dev(A, torch.float32), nA, _dev(B, torch.float32), nB,
                                   _dev(D) if D is not None else None, _dev(res, torch.int32), ambiguity,
                                   _dev(ws.buf), _stream()), "nm_sift_match_f32")
    return res, D


MATCH_MAX_BATCH = 16


class MatchBatchWorkspace:
    """Device scratch for nm_sift_match_batch_f32 with at most n pairs of at most (nA, nB) rows."""

    def __init__(self, n, nA, nB, device):
        torch = _torch()
        self.n, self.nA, self.nB = n, nA, nB
        self.buf = torch.empty(n * lib().nm_sift_match_workspace_bytes(nA, nB), dtype=torch.uint8, device=device)


def sift_match_batch(As, Bs, nAs, nBs, results, ambiguity=0.8, workspace=None):
    """len(As) <= MATCH_MAX_BATCH matches in one call; results[k] (int32, >= nAs[k]) is updated in place like the
    `prior` of sift_match."""
    torch = _torch()
    n = len(As)
    if not (n == len(Bs) == len(nAs) == len(nBs) == len(results)) or not 0 < n <= MATCH_MAX_BATCH:
        raise NmError("bad batch")
    ia = (C.c_int * n)(*nAs)
    ib = (C.c_int * n)(*nBs)
    need = lib().nm_sift_match_batch_workspace_bytes(n, ia, ib)
    if workspace is None:
        workspace = MatchBatchWorkspace(n, max(nAs), max(nBs), As[0].device)
    if workspace.buf.numel() < need:
        raise NmError("batch workspace too small")
    arr = lambda vals: (C.c_void_p * n)(*vals)
    _check(lib().nm_sift_match_batch_f32(n, arr([_dev(a, torch.float32) for a in As]), ia,
                                         arr([_dev(b, torch.float32) for b in Bs]), ib,
                                         arr([_dev(r, torch.int32) for r in results]), ambiguity, _dev(workspace.buf),
                                         _stream()), "nm_sift_match_batch_f32")
    return workspace


class MatchBatchDevWorkspace:
    """Device scratch for nm_sift_match_batch_dev_f32: n pairs of at most (capA, capB) rows, sizes read on the device."""

    def __init__(self, n, capA, capB, device):
        torch = _torch()
        self.n, self.capA, self.capB = n, capA, capB
        self.pair_bytes = lib().nm_sift_match_batch_dev_workspace_bytes(1, capA, capB)
        self.buf = torch.empty(n * self.pair_bytes, dtype=torch.uint8, device=device)

    def row_counts(self, k):
        """(rows of pair k that the bf16x3 second pass screened again, rows that took the exact fallback) in the last call
        on this workspace; the first is meaningful under the two-stage screen only. Synchronises the stream."""
        class _View:                                     # the pair's slice, shaped like a single-pair workspace
            pass
        v = _View()
        v.buf = self.buf[k * self.pair_bytes:(k + 1) * self.pair_bytes]
        return match_second_pass_count(v, self.capA, self.capB), match_fallback_count(v, self.capA, self.capB)


MATCH_PHASE_PREP, MATCH_PHASE_SCREEN, MATCH_PHASE_FINISH = 1, 2, 4


def sift_match_batch_dev(As, d_nAs, Bs, d_nBs, results, ambiguity=0.8, workspace=None, capA=None, capB=None, phases=7):
    """len(As) <= MATCH_MAX_BATCH matches whose set sizes are int32 DEVICE tensors (e.g. SiftArena.num_items): no host
    read-back between detect and match. capA / capB default to the rows of the descriptor tensors."""
    torch = _torch()
    n = len(As)
    if not (n == len(Bs) == len(d_nAs) == len(d_nBs) == len(results)) or not 0 < n <= MATCH_MAX_BATCH:
        raise NmError("bad batch")
    capA = min(a.shape[0] for a in As) if capA is None else capA
    capB = min(b.shape[0] for b in Bs) if capB is None else capB
    if any(a.shape[0] < capA for a in As) or any(b.shape[0] < capB for b in Bs) or any(r.shape[0] < capA for r in results):
        raise NmError("a descriptor set or result is smaller than the capacity")
    if workspace is None:
        workspace = MatchBatchDevWorkspace(n, capA, capB, As[0].device)
    if workspace.buf.numel() < lib().nm_sift_match_batch_dev_workspace_bytes(n, capA, capB):
        raise NmError("batch workspace too small")
    arr = lambda vals: (C.c_void_p * n)(*vals)
    _check(lib().nm_sift_match_batch_dev_phases_f32(phases, n, arr([_dev(a, torch.float32) for a in As]),
                                                    arr([_dev(c, torch.int32) for c in d_nAs]),
                                                    arr([_dev(b, torch.float32) for b in Bs]),
                                                    arr([_dev(c, torch.int32) for c in d_nBs]), capA, capB,
                                                    arr([_dev(r, torch.int32) for r in results]), ambiguity,
                                                    _dev(workspace.buf), _stream()), "nm_sift_match_batch_dev_phases_f32")
    return workspace


MATCH_SCREENS = {"f32": 0, "bf16x3": 1, "f16": 2}


def set_match_screen(name):
    """Select the MFMA screen of the fused matcher ("f32", "bf16x3" or the two-stage "f16"; results are identical, see
    nm_abi.h)."""
    _check(lib().nm_sift_match_set_screen(MATCH_SCREENS[name]), "nm_sift_match_set_screen")


def get_match_screen():
    v = lib().nm_sift_match_get_screen()
    return [k for k, x in MATCH_SCREENS.items() if x == v][0]


def match_pairs_per_launch(n_pairs):
    """Pairs one launch of the screening kernel covers in a batched call of n_pairs pairs under the current screen (nm_abi.h)."""
    return int(lib().nm_sift_match_pairs_per_launch(int(n_pairs)))


def set_detect_tall_min(min_groups=-1):
    """Batched detection launches with at least `min_groups` 20-row unit groups take the tall form (default 2048; -1 restores
    it, 2**31 - 1 disables it). Returns the previous value. Results do not depend on it."""
    return lib().nm_sift_set_detect_tall_min(int(min_groups))


def set_frame_skew(mode=-1):
    """Issue order of many-frame detect/describe calls: 0 = every octave's five levels on the caller's stream, 1 = levels 4-5
    on the detection stream (the small octaves run beside the large ones), 2 = levels 4-5 on a third stream (detection stays
    beside the next octave's levels 1-3); -1 restores the default (NM_FRAME_SKEW, 0 when unset). Returns the previous value.
    Results do not depend on it."""
    return lib().nm_sift_set_frame_skew(int(mode))


DISTANCE_MODES = {"exact": 0, "mfma": 1}


def set_distance_mode(name):
    """How sift_match(..., want_distance=True) fills the matrix: "mfma" (default: fp32 matrix cores, every entry within 1e-4
    relative of the reference's chain, near-duplicates recomputed exactly) or "exact" (VALU kernel, bit-equal)."""
    _check(lib().nm_sift_match_set_distance_mode(DISTANCE_MODES[name]), "nm_sift_match_set_distance_mode")


def get_distance_mode():
    v = lib().nm_sift_match_get_distance_mode()
    return [k for k, x in DISTANCE_MODES.items() if x == v][0]


def match_distance_listed(workspace, nA, nB):
    """(32 x 32 blocks of the matrix the last MFMA distance pass on `workspace` listed for re-examination, capacity of its
    list); (-1, 0) when the pass took the exact kernel for lack of scratch."""
    n, cap = C.c_int(0), C.c_int(0)
    _check(lib().nm_sift_match_distance_listed(_dev(workspace.buf), nA, nB, C.byref(n), C.byref(cap), _stream()),
           "nm_sift_match_distance_listed")
    return n.value, cap.value


def match_fallback_count(workspace, nA, nB):
    """Rows of the last match call on `workspace` (same sizes) that needed the exact full-scan fallback."""
    n = C.c_int(0)
    _check(lib().nm_sift_match_fallback_count(_dev(workspace.buf), nA, nB, C.byref(n), _stream()),
           "nm_sift_match_fallback_count")
    return n.value


def match_second_pass_count(workspace, nA, nB):
    """Two-stage screen: rows of the last match call on `workspace` (same sizes) that the bf16x3 pass screened again."""
    n = C.c_int(0)
    _check(lib().nm_sift_match_second_pass_count(_dev(workspace.buf), nA, nB, C.byref(n), _stream()),
           "nm_sift_match_second_pass_count")
    return n.value


def sift_match_shard(A, B_shard, index_offset, workspace=None):
    """Exact (min1, idx+offset, min2) of every row of A over the local shard of B."""
    torch = _torch()
    nA, nB = A.shape[0], B_shard.shape[0]
    ws = workspace or MatchWorkspace(nA, nB, A.device)
    m1 = torch.empty(nA, dtype=torch.float32, device=A.device)
    ix = torch.empty(nA, dtype=torch.int32, device=A.device)
    m2 = torch.empty(nA, dtype=torch.float32, device=A.device)
    _check(lib().nm_sift_match_shard_f32(_dev(A, torch.float32), nA, _dev(B_shard, torch.float32), nB, index_offset,
                                         _dev(m1), _dev(ix), _dev(m2), _dev(ws.buf), _stream()),
           "nm_sift_match_shard_f32")
    return m1, ix, m2


def sift_match_merge(m1_all, ix_all, m2_all, ambiguity=0.8, prior=None):
    """Merge shard-major (n_shards, nA) triples into match indexes."""
    torch = _torch()
    n_shards, nA = m1_all.shape
    res = torch.full((nA,), -1, dtype=torch.int32, device=m1_all.device) if prior is None else prior
    _check(lib().nm_sift_match_merge_f32(_dev(m1_all, torch.float32), _dev(ix_all, torch.int32),
                                         _dev(m2_all, torch.float32), n_shards, nA, _dev(res), ambiguity, _stream()),
           "nm_sift_match_merge_f32")
    return res


# ---- element-wise stages either side of the path --------------------------------------------
def grayscale(bgra):
    """uint8 (H, W, 4) BGRA -> float32 (H, W): 0.07 B + 0.72 G + 0.21 R."""
    torch = _torch()
    h, w, _ = bgra.shape
    out = torch.empty((h, w), dtype=torch.float32, device=bgra.device)
    _check(lib().nm_grayscale_f32(_dev(bgra, torch.uint8), _dev(out), w, h, _stream()), "nm_grayscale_f32")
    return out


def extract_channel(bgra, channel):
    torch = _torch()
    h, w, _ = bgra.shape
    out = torch.full((h, w), -7.0, dtype=torch.float32, device=bgra.device)
    _check(lib().nm_extract_channel_f32(_dev(bgra, torch.uint8), _dev(out), w, h, channel, _stream()),
           "nm_extract_channel_f32")
    return out


def put_channel(bgra, plane, channel):
    torch = _torch()
    out = bgra.clone()
    h, w, _ = out.shape
    _check(lib().nm_put_channel_f32(_dev(out, torch.uint8), _dev(plane, torch.float32), w, h, channel, _stream()),
           "nm_put_channel_f32")
    return out


def set_alpha(bgra, val=255):
    torch = _torch()
    out = bgra.clone()
    h, w, _ = out.shape
    _check(lib().nm_set_alpha_to_const(_dev(out, torch.uint8), w, h, val, _stream()), "nm_set_alpha_to_const")
    return out


def cast_f32_u8(src, max_val=0):
    torch = _torch()
    h, w = src.shape
    out = torch.empty((h, w), dtype=torch.uint8, device=src.device)
    _check(lib().nm_cast_f32_u8(_dev(src, torch.float32), w, h, _dev(out), max_val, _stream()), "nm_cast_f32_u8")
    return out


def downsample2_u8x4(src, rw, rh):
    torch = _torch()
    sh, sw, _ = src.shape
    out = torch.empty((rh, rw, 4), dtype=torch.uint8, device=src.device)
    _check(lib().nm_downsample2_u8x4(_dev(out), rw, rh, _dev(src, torch.uint8), sw, sh, _stream()), "nm_downsample2_u8x4")
    return out


def align_points(sx, sy, dx, dy, matches):
    torch = _torch()
    n = matches.shape[0]
    outs = [torch.empty(n, dtype=torch.float32, device=matches.device) for _ in range(4)]
    _check(lib().nm_align_points(_dev(sx), _dev(sy), _dev(dx), _dev(dy), *[_dev(o) for o in outs],
                                 _dev(matches, torch.int32), n, _stream()), "nm_align_points")
    return outs


def selftest_sqrt():
    """Number of inputs for which the gradient's fast sqrt differs from IEEE sqrt over its whole domain (must be 0)."""
    torch = _torch()
    out = torch.zeros(1, dtype=torch.int64, device="cuda")
    _check(lib().nm_selftest_sqrt(_dev(out), _stream()), "nm_selftest_sqrt")
    return int(out.item())


def selftest_expw():
    """nm_selftest_expw: (unreported differences, inputs reporting a nearby rounding boundary, inputs tested) of the descriptor
    weight's fast form against the spec sequence over its whole domain. The first must be 0."""
    torch = _torch()
    out = torch.zeros(3, dtype=torch.int64, device="cuda")
    _check(lib().nm_selftest_expw(_dev(out), _stream()), "nm_selftest_expw")
    return tuple(int(v) for v in out.cpu())


def selftest_orient():
    """nm_selftest_orient: (differing thirds, inputs the third's guard rejects, differing window tests, differing quotients,
    quotients tested) of the orientation kernel's hoisted arithmetic against the expressions it replaces. [0], [2], [3] must be 0."""
    torch = _torch()
    out = torch.zeros(5, dtype=torch.int64, device="cuda")
    _check(lib().nm_selftest_orient(_dev(out), _stream()), "nm_selftest_orient")
    return tuple(int(v) for v in out.cpu())


MFMA_BF16, MFMA_F16 = 0, 1


def selftest_mfma_model(instruction, n_random=1 << 20, n_chains=4096):
    """nm_selftest_mfma_model: the rounding model of the matrix instruction the matcher's screens issue, measured on this
    device (layout probe, directed cases, random instructions, the screens' own accumulator chains on adversarial rows
    incl. fp16 subnormals, all against binary64). Returns a dict of the NM_SELFTEST_MFMA_OUTPUTS figures."""
    torch = _torch()
    out = torch.zeros(16, dtype=torch.float32, device="cuda")
    _check(lib().nm_selftest_mfma_model(int(instruction), int(n_random), int(n_chains), _dev(out), _stream()),
           "nm_selftest_mfma_model")
    v = [float(x) for x in out.cpu()]
    return {"layout_mismatches": v[0], "c1_plus_16_small_ulp": v[1], "c1_plus_one_small_ulp": v[2],
            "one_plus_15_small_ulp": v[3], "c2p24_plus_16": v[4], "rel_u": v[5], "model_ratio": v[6],
            "instructions": v[7], "chain_coeff": v[8], "chain_coeff_subnormal": v[9], "chain_launches": v[10],
            "same_half_truncation_ulp": v[11]}


def selftest_mfma_f32(n_random=1 << 22, n_chains=2048):
    """nm_selftest_mfma_f32: rounding of v_mfma_f32_32x32x2_f32 on this device (single instructions and the two accumulation
    forms the library issues), against binary64."""
    torch = _torch()
    out = torch.zeros(8, dtype=torch.float32, device="cuda")
    _check(lib().nm_selftest_mfma_f32(int(n_random), int(n_chains), _dev(out), _stream()), "nm_selftest_mfma_f32")
    v = [float(x) for x in out.cpu()]
    return {"rel_u": v[0], "frac_fma_chain": v[1] / max(v[5], 1.0), "frac_correctly_rounded": v[2] / max(v[5], 1.0),
            "two_chain_coeff": v[3], "one_chain_coeff": v[4], "results": v[5]}


def match_distance_budget():
    return float(lib().nm_sift_match_distance_budget())


def match_accum_budget(screen):
    return float(lib().nm_sift_match_accum_budget(int(screen)))


TEX_U8N, TEX_U8X4N, TEX_F32 = 0, 1, 2


def _tex_format(t):
    torch = _torch()
    if t.dtype == torch.float32 and t.dim() == 2:
        return TEX_F32
    if t.dtype == torch.uint8 and t.dim() == 2:
        return TEX_U8N
    raise NmError("a scalar texture must be a 2-D float32 or uint8 device tensor")


def undistort_map(x, y, camera_matrix, distortion_coeffs):
    """cuda_undistort: per-pixel source coordinates (u, v) of the radial model. camera_matrix = (fx, fy, cx, cy) and
    distortion_coeffs = (k1, k2, k3) are device tensors, as in the reference."""
    torch = _torch()
    h, w = x.shape
    u, v = torch.empty_like(x), torch.empty_like(y)
    _check(lib().nm_undistort_map_f32(_dev(x, torch.float32), _dev(y, torch.float32), w, h,
                                      _dev(camera_matrix, torch.float32), _dev(distortion_coeffs, torch.float32), _dev(u),
                                      _dev(v), _stream()), "nm_undistort_map_f32")
    return u, v


def resample_undistort(tex, x, y):
    torch = _torch()
    h, w = x.shape
    out = torch.empty((h, w), dtype=torch.float32, device=x.device)
    _check(lib().nm_resample_undistort_f32(_dev(tex), tex.shape[1], tex.shape[0], _tex_format(tex), _dev(x, torch.float32),
                                           _dev(y, torch.float32), w, h, _dev(out), _stream()), "nm_resample_undistort_f32")
    return out


def resample_mask(tex, x_pos, y_pos, threshold=0.5):
    torch = _torch()
    h, w = x_pos.shape
    out = torch.empty((h, w), dtype=torch.uint8, device=x_pos.device)
    _check(lib().nm_resample_mask_u8(_dev(out), _dev(tex), tex.shape[1], tex.shape[0], _tex_format(tex), w, h,
                                     _dev(x_pos, torch.float32), _dev(y_pos, torch.float32), threshold, _stream()),
           "nm_resample_mask_u8")
    return out


def resample_perspective(tex_bgra, cols, rows, mat3x3, inverse=True):
    """resample_perspective_transform: returns (result (rows, cols, 4) uint8, x_pos, y_pos)."""
    torch = _torch()
    out = torch.empty((rows, cols, 4), dtype=torch.uint8, device=tex_bgra.device)
    xp = torch.empty((rows, cols), dtype=torch.float32, device=tex_bgra.device)
    yp = torch.empty_like(xp)
    _check(lib().nm_resample_perspective_u8x4(_dev(out), _dev(tex_bgra, torch.uint8), tex_bgra.shape[1], tex_bgra.shape[0],
                                              cols, rows, _dev(xp), _dev(yp), _dev(mat3x3, torch.float32),
                                              1 if inverse else 0, _stream()), "nm_resample_perspective_u8x4")
    return out, xp, yp


def transform_blend(canvas, canvas_wts, frame, nw, nh, mat3x3, tx, ty, frame_mask, frame_wts):
    """transform_blend: blends the warped frame into `canvas` / `canvas_wts` IN PLACE."""
    torch = _torch()
    ch, cw, _ = canvas.shape
    fh, fw, _ = frame.shape
    _check(lib().nm_transform_blend(_dev(canvas, torch.uint8), cw, ch, _dev(frame, torch.uint8), fw, fh, nw, nh,
                                    _dev(mat3x3, torch.float32), tx, ty, _dev(frame_mask), _tex_format(frame_mask),
                                    _dev(canvas_wts, torch.float32), _dev(frame_wts), _tex_format(frame_wts), _stream()),
           "nm_transform_blend")


def ransac(model, sx, sy, dx, dy, rand_list, thr):
    """Evaluate RANSAC hypotheses on the device. model 0/1/2 = translation/similarity/homography; rand_list int32
    (iterations, samples). Returns (position, H_best[9], homographies[iterations, 9], inliers[iterations])."""
    torch = _torch()
    it = rand_list.shape[0]
    H_all = torch.zeros((it, 9), dtype=torch.float32, device=sx.device)
    inl = torch.zeros(it, dtype=torch.int32, device=sx.device)
    Hb = torch.zeros(9, dtype=torch.float32, device=sx.device)
    pos = torch.zeros(1, dtype=torch.int32, device=sx.device)
    _check(lib().nm_ransac_f32(model, _dev(sx, torch.float32), _dev(sy), _dev(dx), _dev(dy), sx.shape[0],
                               _dev(rand_list, torch.int32), it, thr, _dev(H_all), _dev(inl), _dev(Hb), _dev(pos),
                               _stream()), "nm_ransac_f32")
    return pos, Hb, H_all, inl


# ---- the pair-batch stages (batched RANSAC, inlier refit, guided and mutual matching): csrc/nm_pair_batch.hpp in Python ----
# A call takes n <= 64 pairs as equally long lists of per-pair tensors; a capacity is the number of rows the kernels may
# touch and lies in [1, 2^22); device wrappers want everything on the current device, host twins take numpy.
_PAIR_MAX_BATCH = 64
_PAIR_CAP_LIMIT = 1 << 22
RANSAC_MAX_BATCH = MATCH_GUIDED_MAX_BATCH = MATCH_MUTUAL_MAX_BATCH = _PAIR_MAX_BATCH
RANSAC_MAX_ITERATIONS = 1 << 20
RANSAC_REFIT_MAX_ROUNDS = 4


def _pair_count(*lists):
    """n of a call: its per-pair lists (None: an optional list that was not given) are equally long, 0 < n <= 64."""
    n = len(lists[0])
    if any(len(v) != n for v in lists if v is not None) or not 0 < n <= _PAIR_MAX_BATCH:
        raise NmError("pair batch: lists of one length in [1, %d] expected" % _PAIR_MAX_BATCH)
    return n


def _pair_cap(cap, tensors):
    """A capacity (default: the smallest first dimension of `tensors`), in range and no larger than any of them."""
    cap = min(t.shape[0] for t in tensors) if cap is None else cap
    if not 1 <= cap < _PAIR_CAP_LIMIT:
        raise NmError("pair batch: capacity %r outside [1, %d)" % (cap, _PAIR_CAP_LIMIT))
    if any(t.shape[0] < cap for t in tensors):
        raise NmError("pair batch: a tensor is smaller than the capacity %d" % cap)
    return cap


def _pair_model_shape(n, h_numel, status_numel):
    if h_numel != 9 * n or status_numel not in (None, n):
        raise NmError("pair batch: H must hold n x 9 floats and status n values")


def _pair_descriptors(*lists):
    if any(t.ndim != 2 or t.shape[1] != 128 for ts in lists for t in ts):
        raise NmError("descriptors must be (rows, 128)")


def _pair_device(tensors, sizes):
    """The device of a call: every tensor (None: an optional one that was not given) on the current CUDA device, no
    DEVICE size tensor empty."""
    torch = _torch()
    device = tensors[0].device
    if any(t is not None and t.device != device for t in tensors) or device.type != "cuda" or \
            torch.cuda.current_device() != device.index:
        raise NmError("pair batch: all tensors must live on the current device")
    if any(c.numel() < 1 for c in sizes):
        raise NmError("pair batch: a device size tensor is empty")
    return device


def _pair_dev_table(tensors, dtype):
    """Host table of the device pointers of contiguous `dtype` tensors (_dev's rules, checked for the table as a whole);
    None (an optional table) stays None."""
    if tensors is None:
        return None
    if not all(t.is_cuda and t.dtype == dtype and t.is_contiguous() for t in tensors):
        raise NmError("pair batch: contiguous device tensors of dtype %s expected" % dtype)
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _pair_host_table(arrays):
    return None if arrays is None else (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def _pair_host_ptr(a):
    return None if a is None else a.ctypes.data


def _pair_host_arrays(values, dtype, flat=True):
    import numpy as np
    arrays = [np.ascontiguousarray(v, dtype=dtype) for v in values]
    return [a.reshape(-1) for a in arrays] if flat else arrays


def _pair_host_sizes(ns):
    """Host sizes as the C entries take them, one pointer per pair: the one-element views of one int32 array."""
    import numpy as np
    a = np.array([int(v) for v in ns], np.int32)
    return [a[k:k + 1] for k in range(a.size)]


def _pair_host_model(n, H, status):
    import numpy as np
    H = np.ascontiguousarray(H, dtype=np.float32).reshape(-1)
    status = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(-1)
    _pair_model_shape(n, H.size, None if status is None else status.size)
    return H, status


def _pair_host_match_out(n, capA, want_distance):
    import numpy as np
    return np.zeros((n, capA), np.int32), np.zeros(n, np.int32), np.zeros((n, capA), np.float32) if want_distance else None


def _pair_dev_match_out(n, capA, results, device, want_distance):
    """results (given or new, no smaller than capA), count and the optional per-row distances of guided / mutual matching."""
    torch = _torch()
    if results is None:
        results = [torch.empty(capA, dtype=torch.int32, device=device) for _ in range(n)]
    _pair_cap(capA, results)
    count = torch.empty(n, dtype=torch.int32, device=device)
    dist = [torch.empty(capA, dtype=torch.float32, device=device) for _ in range(n)] if want_distance else None
    return results, count, dist


def _point_tables_dev(src_xs, src_ys, d_nAs, dst_xs, dst_ys, matches):
    f, i32 = _torch().float32, _torch().int32
    return [_pair_dev_table(ts, dt) for ts, dt in ((src_xs, f), (src_ys, f), (d_nAs, i32), (dst_xs, f), (dst_ys, f), (matches, i32))]


# ---- the frame-sequence stages (ingest, frame weights, link verify and refine, mosaic plan to median), DESIGN.md section 7 ----
# A call takes n <= 64 frames of one shape as a list; every frame, map and canvas extent lies in [1, _SIZE_LIMIT], which is
# NM_SIZE_LIMIT of csrc/nm_common.hpp; device wrappers want torch tensors on the current device, host twins take numpy. The
# checks below read shapes and dtypes only, so they serve both.
_SIZE_LIMIT = 32767
_FRAMES_MAX_BATCH = _PAIR_MAX_BATCH


def _opt(t, dtype=None):
    """_dev of an optional tensor"""
    return None if t is None else _dev(t, dtype)


def _on_current_device(tensors, what):
    """The device of a call: every tensor (None: an optional one that was not given) on the current CUDA device."""
    tensors = [t for t in tensors if t is not None]
    device = tensors[0].device
    if any(t.device != device for t in tensors) or device.type != "cuda" or _torch().cuda.current_device() != device.index:
        raise NmError("%s: all tensors must live on the current device" % what)
    return device


def _is_dtype(a, name):
    return str(a.dtype).split(".")[-1] == name              # torch.uint8 and numpy's uint8 alike


def _size_check(what, name, w, h):
    if not (1 <= w <= _SIZE_LIMIT and 1 <= h <= _SIZE_LIMIT):
        raise NmError("%s: %s %r x %r outside [1, %d]" % (what, name, w, h, _SIZE_LIMIT))


def _frames_check(what, frames):
    """(n, fw, fh) of a list of n in [1, 64] BGRA frames, uint8 and of one (fh, fw, 4) shape."""
    n = len(frames)
    if not 0 < n <= _FRAMES_MAX_BATCH:
        raise NmError("%s: %d frames (1 .. %d)" % (what, n, _FRAMES_MAX_BATCH))
    if any(len(f.shape) != 3 or f.shape[2] != 4 or not _is_dtype(f, "uint8") for f in frames):
        raise NmError("%s: frames must be (fh, fw, 4) uint8" % what)
    fh, fw = frames[0].shape[:2]
    if any(tuple(f.shape) != (fh, fw, 4) for f in frames):
        raise NmError("%s: all frames must have one shape" % what)
    _size_check(what, "frame", fw, fh)
    return n, fw, fh


def _planes_check(what, planes, mask):
    """(fw, fh) of gray planes and an optional mask, all of one (fh, fw) shape."""
    shape = tuple(planes[0].shape)
    if len(shape) != 2 or any(tuple(p.shape) != shape for p in planes + ([mask] if mask is not None else [])):
        raise NmError("%s: planes of one (height, width) shape expected" % what)
    return shape[1], shape[0]


def _lattice_check(what, fw, fh, stride):
    """A frame and the stride of the lattice the link and exposure stages walk over it (csrc/nm_lattice.hpp)."""
    _size_check(what, "frame", fw, fh)
    if int(stride) != stride or not 1 <= stride <= 64 or (fw // stride) * (fh // stride) > 1 << 28:
        raise NmError("%s: stride %r outside [1, 64] or a lattice beyond 2^28 pixels" % (what, stride))


def _scalar_planes(what, n, fw, fh, masks, wts):
    """masks and wts as two lists of n (fh, fw) planes (one plane stands for every frame) and their formats, one per call."""
    masks, wts = (list(v) if isinstance(v, (list, tuple)) else [v] * n for v in (masks, wts))
    if len(masks) != n or len(wts) != n:
        raise NmError("%s: %d frames, %d masks, %d weight planes" % (what, n, len(masks), len(wts)))
    if any(tuple(t.shape) != (fh, fw) for t in masks + wts):
        raise NmError("%s: masks and weights must be (fh, fw) planes" % what)
    mfmt, wfmt = _tex_format(masks[0]), _tex_format(wts[0])
    if any(_tex_format(t) != mfmt for t in masks) or any(_tex_format(t) != wfmt for t in wts):
        raise NmError("%s: one mask format and one weight format per call" % what)
    return masks, wts, mfmt, wfmt


def _records_check(what, records, n):
    if tuple(records.shape) != (n, 16) or not _is_dtype(records, "int32"):
        raise NmError("%s: records must be int32 (n, 16)" % what)


def _canvas_check(what, canvas, canvas_wts, wts_optional=False):
    """(cw, ch) of a (ch, cw, 4) canvas and its (ch, cw) weights, which may be None where the stage says so."""
    shape = tuple(canvas.shape)
    if len(shape) != 3 or shape[2] != 4 or (canvas_wts is None and not wts_optional) or \
            (canvas_wts is not None and tuple(canvas_wts.shape) != shape[:2]):
        raise NmError("%s: canvas must be (ch, cw, 4) uint8 with (ch, cw) float32 weights%s"
                      % (what, " or None" if wts_optional else ""))
    _size_check(what, "canvas", shape[1], shape[0])
    return shape[1], shape[0]


def _composite_head(what, canvas, canvas_wts, tiles, records):
    """What mosaic_bands and mosaic_median look at first: tiles (n, tile_cap, 4), records (n, 16), the canvas. Returns
    (n, tile_cap, cw, ch)."""
    if len(tiles.shape) != 3 or tiles.shape[2] != 4:
        raise NmError("%s: tiles must be float32 (n, tile_cap, 4)" % what)
    n, tile_cap = tiles.shape[:2]
    _records_check(what, records, n)
    return (n, tile_cap) + _canvas_check(what, canvas, canvas_wts, wts_optional=True)


def _composite_head_host(what, canvas, canvas_wts, tiles, records, outputs=()):
    """_composite_head of the host twins: tiles and records converted, every in-place output ((array, dtype) pairs) contiguous,
    writeable and of its type, the tiles copied to 16-byte aligned memory. Returns (n, tile_cap, cw, ch, tiles, records)."""
    import numpy as np
    tiles, records = np.ascontiguousarray(tiles, dtype=np.float32), np.ascontiguousarray(records, dtype=np.int32)
    for a, dt in ((canvas, np.uint8), (canvas_wts, np.float32)) + tuple(outputs):
        if a is not None and (a.dtype != dt or not a.flags.c_contiguous or not a.flags.writeable):
            raise NmError("%s: outputs must be contiguous, writeable and of their documented types" % what)
    head = _composite_head(what, canvas, canvas_wts, tiles, records)
    aligned = _aligned_host(tiles.nbytes, np)
    aligned[:] = tiles.reshape(-1).view(np.uint8)
    return head + (aligned, records)


def _aligned_host(nbytes, np, align=16):
    raw = np.empty(nbytes + align, np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + nbytes]


class _PairWorkspace:
    """Device scratch of a pair-batch stage: `buf` holds what the stage's *_workspace_bytes asks for the shape, which is
    kept as attributes. A subclass names the C function, the stage (for messages) and how it words a refused shape."""
    _bytes_fn = _what = _shape_text = None

    def _alloc(self, device, **shape):
        need = getattr(lib(), self._bytes_fn)(*shape.values())
        if need == 0:
            raise NmError("%s: %s out of range" % (self._what, self._shape_text % tuple(shape.values())))
        self.__dict__.update(shape)
        self.buf = _torch().empty(need, dtype=_torch().uint8, device=device if device is not None else "cuda")


def _pair_workspace(cls, workspace, device, *shape):
    """The workspace of a call: the given one, or a new `cls`; never smaller than the stage asks for this shape."""
    if workspace is None:
        workspace = cls(*shape, device)
    need = getattr(lib(), cls._bytes_fn)(*shape)
    if need == 0 or workspace.buf.numel() < need:
        raise NmError(cls._what + " too small")
    return workspace


class RansacBatchWorkspace(_PairWorkspace):
    """Device scratch for nm_ransac_batch_dev_f32: n pairs of at most capA rows and `iterations` hypotheses."""
    _bytes_fn, _what, _shape_text = "nm_ransac_batch_dev_workspace_bytes", "RANSAC batch workspace", "n=%d capA=%d iterations=%d"

    def __init__(self, n, capA, iterations, device):
        self._alloc(device, n=n, capA=capA, iterations=iterations)


def ransac_batch_sample(seed, hypothesis, sample, samples, m):
    """The batched RANSAC's sampler (host): index j in [0, m) into the pair's valid rows, or -1 for bad arguments."""
    return lib().nm_ransac_batch_sample(seed & 0xFFFFFFFF, hypothesis, sample, samples, m)


def ransac_batch_dev(model, src_xs, src_ys, d_nAs, dst_xs, dst_ys, matches, iterations=4096, threshold=4.0, seeds=None,
                     capA=None, workspace=None, want_all=False):
    """len(src_xs) <= RANSAC_MAX_BATCH frame pairs in one call (nm_ransac_batch_dev_f32), sampled on the device: no host
    read, no allocation inside the C call. d_nAs are int32 DEVICE tensors (e.g. SiftArena.num_items); matches[k] is the
    pair's matcher result. model 0/1/2 = translation/similarity/homography; threshold bounds the squared reprojection
    error. seeds (host ints) default to range(n); capA to the rows of the source tensors. Returns (H_best[n, 9],
    best_inliers[n], position[n], status[n]) and, with want_all, also (homographies[n, iterations, 9], inliers[n, iterations])."""
    torch = _torch()
    n = _pair_count(src_xs, src_ys, d_nAs, dst_xs, dst_ys, matches)
    if model not in (0, 1, 2) or not 0 < iterations <= RANSAC_MAX_ITERATIONS:
        raise NmError("model %r / iterations %r out of range" % (model, iterations))
    seeds = list(range(n)) if seeds is None else [int(s) for s in seeds]
    if len(seeds) != n or any(not 0 <= s <= 0xFFFFFFFF for s in seeds):
        raise NmError("seeds: %d unsigned 32-bit values expected" % n)
    capA = _pair_cap(capA, list(src_xs) + list(src_ys) + list(matches))
    device = _pair_device(list(src_xs) + list(src_ys) + list(d_nAs) + list(dst_xs) + list(dst_ys) + list(matches) +
                          [workspace.buf if workspace is not None else None], d_nAs)
    workspace = _pair_workspace(RansacBatchWorkspace, workspace, device, n, capA, iterations)
    H_best = torch.empty((n, 9), dtype=torch.float32, device=device)
    best, pos, status = (torch.empty(n, dtype=torch.int32, device=device) for _ in range(3))
    H_all = torch.empty((n, iterations, 9), dtype=torch.float32, device=device) if want_all else None
    inl = torch.empty((n, iterations), dtype=torch.int32, device=device) if want_all else None
    tables = _point_tables_dev(src_xs, src_ys, d_nAs, dst_xs, dst_ys, matches)
    _check(lib().nm_ransac_batch_dev_f32(model, n, *tables[:3], capA, *tables[3:], iterations, threshold,
                                         (C.c_uint * n)(*seeds), _dev(H_best), _dev(best), _dev(pos), _dev(status),
                                         _dev(H_all) if want_all else None, _dev(inl) if want_all else None,
                                         _dev(workspace.buf), _stream()), "nm_ransac_batch_dev_f32")
    if want_all:
        return H_best, best, pos, status, H_all, inl
    return H_best, best, pos, status


def _refit_check(model, rounds, threshold):
    if model not in (0, 1, 2) or not 0 <= int(rounds) <= RANSAC_REFIT_MAX_ROUNDS or int(rounds) != rounds:
        raise NmError("model %r / rounds %r out of range" % (model, rounds))
    if not math.isfinite(threshold):
        raise NmError("threshold must be finite")


def ransac_refit_batch_dev(model, src_xs, src_ys, d_nAs, dst_xs, dst_ys, matches, H, status=None, rounds=2, threshold=4.0,
                           capA=None, want_mask=False, want_rms=False):
    """Least-squares refit of n = len(src_xs) <= RANSAC_MAX_BATCH maps over their inliers (nm_ransac_refit_batch_dev_f32):
    one launch on the current stream, no host read. The per-pair tensors are those of ransac_batch_dev; H is float32
    device (n, 9) or (n, 3, 3), e.g. its H_best; status int32 device (n,) or None (all usable). rounds in [0, 4]: 0 gives
    the inlier count (and mask) of H itself. Returns (H_out[n, 9], count[n], status[n], rounds_done[n]) and then, when
    asked for, mask uint8 (n, capA) and rms float32 (n,)."""
    torch = _torch()
    n = _pair_count(src_xs, src_ys, d_nAs, dst_xs, dst_ys, matches)
    _refit_check(model, rounds, threshold)
    capA = _pair_cap(capA, list(src_xs) + list(src_ys) + list(matches))
    _pair_model_shape(n, H.numel(), None if status is None else status.numel())
    device = _pair_device(list(src_xs) + list(src_ys) + list(d_nAs) + list(dst_xs) + list(dst_ys) + list(matches) + [H, status],
                          d_nAs)
    H_out = torch.empty((n, 9), dtype=torch.float32, device=device)
    count, st, done = (torch.empty(n, dtype=torch.int32, device=device) for _ in range(3))
    mask = torch.empty((n, capA), dtype=torch.uint8, device=device) if want_mask else None
    rms = torch.empty(n, dtype=torch.float32, device=device) if want_rms else None
    tables = _point_tables_dev(src_xs, src_ys, d_nAs, dst_xs, dst_ys, matches)
    _check(lib().nm_ransac_refit_batch_dev_f32(model, n, *tables[:3], capA, *tables[3:], _dev(H, torch.float32),
                                               _dev(status, torch.int32) if status is not None else None, threshold,
                                               int(rounds), _dev(H_out), _dev(count), _dev(st), _dev(done),
                                               _dev(mask) if want_mask else None, _dev(rms) if want_rms else None,
                                               _stream()), "nm_ransac_refit_batch_dev_f32")
    return (H_out, count, st, done) + ((mask,) if want_mask else ()) + ((rms,) if want_rms else ())


def ransac_refit_host(model, src_xs, src_ys, nAs, dst_xs, dst_ys, matches, H, status=None, rounds=2, threshold=4.0,
                      capA=None, want_mask=False, want_rms=False):
    """ransac_refit_batch_dev on the host (nm_ransac_refit_host_f32, the same functions): numpy in and out, bit-identical
    results. nAs are host ints."""
    import numpy as np
    n = _pair_count(src_xs, src_ys, nAs, dst_xs, dst_ys, matches)
    _refit_check(model, rounds, threshold)
    src_xs, src_ys, dst_xs, dst_ys = (_pair_host_arrays(vs, np.float32) for vs in (src_xs, src_ys, dst_xs, dst_ys))
    matches = _pair_host_arrays(matches, np.int32)
    capA = _pair_cap(capA, src_xs + src_ys + matches)
    for m, x, y in zip(matches, dst_xs, dst_ys):
        if m.size and int(m.max()) >= min(x.size, y.size):
            raise NmError("a match points beyond the destination coordinates")
    H, status = _pair_host_model(n, H, status)
    nA = _pair_host_sizes(nAs)
    H_out = np.zeros((n, 9), np.float32)
    count, st, done = (np.zeros(n, np.int32) for _ in range(3))
    mask = np.zeros((n, capA), np.uint8) if want_mask else None
    rms = np.zeros(n, np.float32) if want_rms else None
    arr, ptr = _pair_host_table, _pair_host_ptr
    _check(lib().nm_ransac_refit_host_f32(model, n, arr(src_xs), arr(src_ys), arr(nA), capA, arr(dst_xs), arr(dst_ys),
                                          arr(matches), ptr(H), ptr(status), threshold, int(rounds), ptr(H_out), ptr(count),
                                          ptr(st), ptr(done), ptr(mask), ptr(rms)), "nm_ransac_refit_host_f32")
    return (H_out, count, st, done) + ((mask,) if want_mask else ()) + ((rms,) if want_rms else ())


LINK_UNUSABLE, LINK_FEW_INLIERS, LINK_BAD_GEOMETRY, LINK_LOW_OVERLAP, LINK_LOW_NCC = 1, 2, 4, 8, 16
LINK_STATS = ("N", "L", "overlap", "ncc", "gain", "bias", "mean_a", "mean_b")
# The photometric thresholds' defaults: midway between the true links and the wrong maps of the synthetic mosaic views
# under the unquantised float64 model ("Link verification"; tests/test_link_verify_host.py).
LINK_MIN_NCC = 0.52            # true links 0.9989 .. 0.9994, wrong maps -0.019 .. 0.038
LINK_MIN_OVERLAP = 0.60        # true links 0.817 .. 0.860, the true map shifted by half a frame 0.352 .. 0.385


class LinkVerifyWorkspace(_PairWorkspace):
    """Device scratch for nm_link_verify_batch_dev_f32: n pairs."""
    _bytes_fn, _what, _shape_text = "nm_link_verify_workspace_bytes", "link verification workspace", "n=%d"

    def __init__(self, n, device):
        self._alloc(device, n=n)


def _link_check(grayAs, grayBs, mask, stride, min_inliers, max_area_ratio, min_overlap, min_ncc):
    fw, fh = _planes_check("link verification", list(grayAs) + list(grayBs), mask)
    _lattice_check("link verification", fw, fh, stride)
    if int(min_inliers) != min_inliers or min_inliers < 0:
        raise NmError("link verification: min_inliers %r must be an integer >= 0" % (min_inliers,))
    if not all(math.isfinite(v) for v in (max_area_ratio, min_overlap, min_ncc)) or max_area_ratio < 1:
        raise NmError("link verification: thresholds must be finite and max_area_ratio >= 1")
    return fw, fh


def link_verify_batch_dev(grayAs, grayBs, H, status=None, inliers=None, mask=None, stride=4, min_inliers=16,
                          max_area_ratio=4.0, min_overlap=LINK_MIN_OVERLAP, min_ncc=LINK_MIN_NCC, workspace=None):
    """May the maps of n = len(grayAs) <= 64 frame pairs be chained (nm_link_verify_batch_dev_f32)? Two launches on the
    current stream, no host read. grayAs[k], grayBs[k]: float32 device planes (fh, fw), all of one shape, e.g. those of
    ingest_batch (tensors may repeat); H float32 device (n, 9) or (n, 3, 3) maps A pixels to B pixels, e.g. the refit's
    H_out; status and inliers int32 device (n,) or None, e.g. the refit's status and count; mask float32 device (fh, fw)
    or None. Returns (status_out[n], reason[n], stats[n, 8]): reason is a sum of LINK_* bits, stats float64 in the order of
    LINK_STATS. status_out goes to mosaic_plan, ransac_refit_batch_dev and the guided matchers as it is."""
    torch = _torch()
    n = _pair_count(grayAs, grayBs)
    fw, fh = _link_check(grayAs, grayBs, mask, stride, min_inliers, max_area_ratio, min_overlap, min_ncc)
    _pair_model_shape(n, H.numel(), None if status is None else status.numel())
    if inliers is not None and inliers.numel() != n:
        raise NmError("link verification: inliers must hold n values")
    device = _pair_device(list(grayAs) + list(grayBs) + [H, status, inliers, mask,
                                                         workspace.buf if workspace is not None else None], [])
    workspace = _pair_workspace(LinkVerifyWorkspace, workspace, device, n)
    st, why = (torch.empty(n, dtype=torch.int32, device=device) for _ in range(2))
    stats = torch.empty((n, 8), dtype=torch.float64, device=device)
    _check(lib().nm_link_verify_batch_dev_f32(n, _pair_dev_table(grayAs, torch.float32), _pair_dev_table(grayBs, torch.float32),
                                              fw, fh, _opt(mask, torch.float32), _dev(H, torch.float32),
                                              _opt(status, torch.int32), _opt(inliers, torch.int32), int(stride),
                                              int(min_inliers), max_area_ratio, min_overlap, min_ncc, _dev(st), _dev(why),
                                              _dev(stats), _dev(workspace.buf), _stream()), "nm_link_verify_batch_dev_f32")
    return st, why, stats


def link_verify_host(grayAs, grayBs, H, status=None, inliers=None, mask=None, stride=4, min_inliers=16, max_area_ratio=4.0,
                     min_overlap=LINK_MIN_OVERLAP, min_ncc=LINK_MIN_NCC, want_sums=False):
    """link_verify_batch_dev on the host (nm_link_verify_host_f32, the same functions): numpy in and out, bit-identical
    results. With want_sums also the seven integer sums, uint64 (n, 7) (nm_link_verify_sums_host_f32)."""
    import numpy as np
    n = _pair_count(grayAs, grayBs)
    grayAs, grayBs = (_pair_host_arrays(vs, np.float32, flat=False) for vs in (grayAs, grayBs))
    mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.float32)
    fw, fh = _link_check(grayAs, grayBs, mask, stride, min_inliers, max_area_ratio, min_overlap, min_ncc)
    H, status = _pair_host_model(n, H, status)
    inliers = None if inliers is None else np.ascontiguousarray(inliers, dtype=np.int32).reshape(-1)
    if inliers is not None and inliers.size != n:
        raise NmError("link verification: inliers must hold n values")
    st, why = np.zeros(n, np.int32), np.zeros(n, np.int32)
    stats = np.zeros((n, 8), np.float64)
    arr, ptr = _pair_host_table, _pair_host_ptr
    _check(lib().nm_link_verify_host_f32(n, arr(grayAs), arr(grayBs), fw, fh, ptr(mask), ptr(H), ptr(status), ptr(inliers),
                                         int(stride), int(min_inliers), max_area_ratio, min_overlap, min_ncc, ptr(st),
                                         ptr(why), ptr(stats)), "nm_link_verify_host_f32")
    if not want_sums:
        return st, why, stats
    sums = np.zeros((n, 7), np.uint64)
    _check(lib().nm_link_verify_sums_host_f32(n, arr(grayAs), arr(grayBs), fw, fh, ptr(mask), ptr(H), int(stride), ptr(sums)),
           "nm_link_verify_sums_host_f32")
    return st, why, stats, sums


LINK_REFINE_MAX_BATCH, LINK_REFINE_MAX_ITERATIONS = 64, 8
LINK_REFINE_TRANSLATION, LINK_REFINE_AFFINE, LINK_REFINE_HOMOGRAPHY = 0, 1, 2
LINK_REFINE_GAIN_SCALE, LINK_REFINE_BIAS_SCALE, LINK_REFINE_CONVERGED_STEP = 4.0, 8192.0, 2.0 ** -7
(LINK_REFINE_END_ITERATIONS, LINK_REFINE_END_CONVERGED, LINK_REFINE_END_UNUSABLE, LINK_REFINE_END_FEW_PIXELS,
 LINK_REFINE_END_SINGULAR, LINK_REFINE_END_STEP) = range(6)
LINK_REFINE_STATS = ("N", "L", "rms_first", "rms_last", "gain", "bias", "iterations", "last_step", "end")
LINK_REFINE_SUMS = 67


class LinkRefineWorkspace(_PairWorkspace):
    """Device scratch for nm_link_refine_batch_dev_f32: n pairs."""
    _bytes_fn, _what, _shape_text = "nm_link_refine_workspace_bytes", "link refinement workspace", "n=%d"

    def __init__(self, n, device):
        self._alloc(device, n=n)


def _link_refine_check(grayAs, grayBs, mask, model, stride, iterations, min_pixels, max_step):
    fw, fh = _planes_check("link refinement", list(grayAs) + list(grayBs), mask)
    _lattice_check("link refinement", fw, fh, stride)
    if model not in (LINK_REFINE_TRANSLATION, LINK_REFINE_AFFINE, LINK_REFINE_HOMOGRAPHY):
        raise NmError("link refinement: model %r is none of LINK_REFINE_TRANSLATION, _AFFINE, _HOMOGRAPHY" % (model,))
    if int(iterations) != iterations or not 1 <= iterations <= LINK_REFINE_MAX_ITERATIONS:
        raise NmError("link refinement: iterations %r outside [1, %d]" % (iterations, LINK_REFINE_MAX_ITERATIONS))
    if int(min_pixels) != min_pixels or min_pixels < 1:
        raise NmError("link refinement: min_pixels %r must be an integer >= 1" % (min_pixels,))
    if not math.isfinite(max_step) or not max_step > 0:
        raise NmError("link refinement: max_step %r must be finite and > 0" % (max_step,))
    return fw, fh


def link_refine_batch_dev(grayAs, grayBs, H, status=None, mask=None, model=LINK_REFINE_HOMOGRAPHY, stride=4, iterations=4,
                          min_pixels=64, max_step=16.0, workspace=None):
    """Direct (photometric) refinement of the maps of n = len(grayAs) <= 64 frame pairs (nm_link_refine_batch_dev_f32): up to
    `iterations` Gauss-Newton steps on the gray planes with gain and bias, two launches per iteration on the current
    stream, no host read. The tensors are those of link_verify_batch_dev; H is e.g. the refit's H_out. Returns
    (H_out[n, 9], status_out[n], stats[n, 9]): stats float64 in the order of LINK_REFINE_STATS, its last entry one of
    LINK_REFINE_END_*. A pair without an applied step keeps its H and gets status 0. H_out and status_out go to
    link_verify_batch_dev, mosaic_plan and the guided matchers as they are."""
    torch = _torch()
    n = _pair_count(grayAs, grayBs)
    fw, fh = _link_refine_check(grayAs, grayBs, mask, model, stride, iterations, min_pixels, max_step)
    _pair_model_shape(n, H.numel(), None if status is None else status.numel())
    device = _pair_device(list(grayAs) + list(grayBs) + [H, status, mask, workspace.buf if workspace is not None else None], [])
    workspace = _pair_workspace(LinkRefineWorkspace, workspace, device, n)
    H_out = torch.empty((n, 9), dtype=torch.float32, device=device)
    st = torch.empty(n, dtype=torch.int32, device=device)
    stats = torch.empty((n, len(LINK_REFINE_STATS)), dtype=torch.float64, device=device)
    _check(lib().nm_link_refine_batch_dev_f32(n, _pair_dev_table(grayAs, torch.float32), _pair_dev_table(grayBs, torch.float32),
                                              fw, fh, _opt(mask, torch.float32), _dev(H, torch.float32),
                                              _opt(status, torch.int32), int(model), int(stride), int(iterations),
                                              int(min_pixels), max_step, _dev(H_out), _dev(st), _dev(stats),
                                              _dev(workspace.buf), _stream()), "nm_link_refine_batch_dev_f32")
    return H_out, st, stats


def link_refine_host(grayAs, grayBs, H, status=None, mask=None, model=LINK_REFINE_HOMOGRAPHY, stride=4, iterations=4,
                     min_pixels=64, max_step=16.0, want_sums=False):
    """link_refine_batch_dev on the host (nm_link_refine_host_f32, the same functions in the same summation order): numpy
    in and out, bit-identical results. With want_sums also the 67 sums of one walk under H, float64 (n, 67)
    (nm_link_refine_sums_host_f32)."""
    import numpy as np
    n = _pair_count(grayAs, grayBs)
    grayAs, grayBs = (_pair_host_arrays(vs, np.float32, flat=False) for vs in (grayAs, grayBs))
    mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.float32)
    fw, fh = _link_refine_check(grayAs, grayBs, mask, model, stride, iterations, min_pixels, max_step)
    H, status = _pair_host_model(n, H, status)
    H_out = np.zeros((n, 9), np.float32)
    st = np.zeros(n, np.int32)
    stats = np.zeros((n, len(LINK_REFINE_STATS)), np.float64)
    arr, ptr = _pair_host_table, _pair_host_ptr
    _check(lib().nm_link_refine_host_f32(n, arr(grayAs), arr(grayBs), fw, fh, ptr(mask), ptr(H), ptr(status), int(model),
                                         int(stride), int(iterations), int(min_pixels), max_step, ptr(H_out), ptr(st),
                                         ptr(stats)), "nm_link_refine_host_f32")
    if not want_sums:
        return H_out, st, stats
    sums = np.zeros((n, LINK_REFINE_SUMS), np.float64)
    _check(lib().nm_link_refine_sums_host_f32(n, arr(grayAs), arr(grayBs), fw, fh, ptr(mask), ptr(H), int(stride), ptr(sums)),
           "nm_link_refine_sums_host_f32")
    return H_out, st, stats, sums


def _guided_check(radius2, ambiguity, max_distance):
    if not (math.isfinite(radius2) and math.isfinite(ambiguity)):
        raise NmError("radius2 and ambiguity must be finite")
    if max_distance != max_distance:
        raise NmError("max_distance must not be NaN")


def sift_match_guided_batch_dev(As, axs, ays, d_nAs, Bs, bxs, bys, d_nBs, H, status=None, radius2=9.0, ambiguity=0.8,
                                max_distance=float("inf"), capA=None, capB=None, results=None, want_distance=False):
    """Homography-guided matching of n = len(As) <= MATCH_GUIDED_MAX_BATCH pairs (nm_sift_match_guided_batch_dev_f32): three
    launches on the current stream, no host read. As / Bs are float32 device descriptors (rows, 128), axs .. bys the rows'
    coordinates, d_nAs / d_nBs int32 DEVICE sizes (e.g. SiftArena.desc, .x, .y, .num_items); H float32 device (n, 9) or
    (n, 3, 3) mapping A pixels to B pixels (e.g. the refit's H_out), status int32 device (n,) or None. Row i of A is matched
    by the reference's scan against the rows of B within sqrt(radius2) pixels of H(ax, ay); max_distance bounds the best
    descriptor distance (inf = no bound). results: n int32 device tensors of >= capA rows to write into (default: new).
    Returns (results, count[n]) and, with want_distance, the list of float32 (capA,) best distances. results[k] plugs into
    ransac_refit_batch_dev(matches=...)."""
    return _guided_dev(_torch().float32, "nm_sift_match_guided_batch_dev_f32", As, axs, ays, d_nAs, Bs, bxs, bys, d_nBs, H,
                       status, radius2, ambiguity, max_distance, capA, capB, results, want_distance)


def sift_match_guided_host(As, axs, ays, nAs, Bs, bxs, bys, nBs, H, status=None, radius2=9.0, ambiguity=0.8,
                           max_distance=float("inf"), capA=None, capB=None, want_distance=False):
    """sift_match_guided_batch_dev on the host (nm_sift_match_guided_host_f32, the same functions): numpy in and out,
    bit-identical results. nAs / nBs are host ints. Returns (results (n, capA) int32, count (n,)) and, with want_distance,
    best distances (n, capA) float32."""
    return _guided_host("float32", "nm_sift_match_guided_host_f32", As, axs, ays, nAs, Bs, bxs, bys, nBs, H, status, radius2,
                        ambiguity, max_distance, capA, capB, want_distance)


def _guided_dev(dtype, entry, As, axs, ays, d_nAs, Bs, bxs, bys, d_nBs, H, status, radius2, ambiguity, max_distance, capA,
                capB, results, want_distance):
    """The device call of both guided matchers: descriptors of `dtype`, the C entry `entry`."""
    torch = _torch()
    n = _pair_count(As, axs, ays, d_nAs, Bs, bxs, bys, d_nBs, results)
    capA = _pair_cap(capA, list(As) + list(axs) + list(ays))
    capB = _pair_cap(capB, list(Bs) + list(bxs) + list(bys))
    _pair_descriptors(As, Bs)
    _guided_check(radius2, ambiguity, max_distance)
    _pair_model_shape(n, H.numel(), None if status is None else status.numel())
    device = _pair_device(list(As) + list(axs) + list(ays) + list(d_nAs) + list(Bs) + list(bxs) + list(bys) + list(d_nBs) +
                          list(results or ()) + [H, status], list(d_nAs) + list(d_nBs))
    results, count, best = _pair_dev_match_out(n, capA, results, device, want_distance)
    arr, f, i32 = _pair_dev_table, torch.float32, torch.int32
    _check(getattr(lib(), entry)(n, arr(As, dtype), arr(axs, f), arr(ays, f), arr(d_nAs, i32), capA, arr(Bs, dtype),
                                 arr(bxs, f), arr(bys, f), arr(d_nBs, i32), capB, _dev(H, f),
                                 _dev(status, i32) if status is not None else None, radius2, ambiguity, max_distance,
                                 arr(results, i32), _dev(count), arr(best, f), _stream()), entry)
    return (results, count) + ((best,) if want_distance else ())


def _guided_host(np_dtype, entry, As, axs, ays, nAs, Bs, bxs, bys, nBs, H, status, radius2, ambiguity, max_distance, capA,
                 capB, want_distance):
    """The host twin of both guided matchers: descriptors of `np_dtype`, the C entry `entry`."""
    import numpy as np
    n = _pair_count(As, axs, ays, nAs, Bs, bxs, bys, nBs)
    As, Bs = (_pair_host_arrays(vs, np_dtype, flat=False) for vs in (As, Bs))
    axs, ays, bxs, bys = (_pair_host_arrays(vs, np.float32) for vs in (axs, ays, bxs, bys))
    capA = _pair_cap(capA, As + axs + ays)
    capB = _pair_cap(capB, Bs + bxs + bys)
    _pair_descriptors(As, Bs)
    _guided_check(radius2, ambiguity, max_distance)
    H, status = _pair_host_model(n, H, status)
    nA, nB = _pair_host_sizes(nAs), _pair_host_sizes(nBs)
    result, count, best = _pair_host_match_out(n, capA, want_distance)
    arr, ptr = _pair_host_table, _pair_host_ptr
    _check(getattr(lib(), entry)(n, arr(As), arr(axs), arr(ays), arr(nA), capA, arr(Bs), arr(bxs), arr(bys), arr(nB), capB,
                                 ptr(H), ptr(status), radius2, ambiguity, max_distance, arr(list(result)), ptr(count),
                                 arr(list(best)) if want_distance else None), entry)
    return (result, count) + ((best,) if want_distance else ())


def _mutual_caps(As, Bs, matches, capA, capB):
    _pair_descriptors(As, Bs)
    if any(t.ndim != 1 for t in matches):
        raise NmError("a match list must be one-dimensional")
    return _pair_cap(capA, list(As) + list(matches)), _pair_cap(capB, list(Bs))


class MatchMutualWorkspace(_PairWorkspace):
    """Device scratch of sift_match_mutual_batch_dev for up to n pairs of capA rows (the compacted claims)."""
    _bytes_fn, _what, _shape_text = "nm_sift_match_mutual_workspace_bytes", "mutual-match workspace", "n %r / capA %r"

    def __init__(self, n, capA, device=None):
        self._alloc(device, n=n, capA=capA)


def _mutual_dev(dtype, entry, ws_cls, ws_shape, As, d_nAs, Bs, d_nBs, matches, capA, capB, results, workspace, want_distance):
    """The device call of both mutual filters: descriptors of `dtype`, the C entry `entry`, a workspace of class `ws_cls`
    whose shape is ws_shape(n, capA, capB)."""
    torch = _torch()
    n = _pair_count(As, d_nAs, Bs, d_nBs, matches, results)
    capA, capB = _mutual_caps(As, Bs, matches, capA, capB)
    device = _pair_device(list(As) + list(d_nAs) + list(Bs) + list(d_nBs) + list(matches) + list(results or ()) +
                          [workspace.buf if workspace is not None else None], list(d_nAs) + list(d_nBs))
    results, count, fwd = _pair_dev_match_out(n, capA, results, device, want_distance)
    if {r.data_ptr() for r in results} & {m.data_ptr() for m in matches}:
        raise NmError("a result tensor is also a match list")
    workspace = _pair_workspace(ws_cls, workspace, device, *ws_shape(n, capA, capB))
    arr, f, i32 = _pair_dev_table, torch.float32, torch.int32
    _check(getattr(lib(), entry)(n, arr(As, dtype), arr(d_nAs, i32), capA, arr(Bs, dtype), arr(d_nBs, i32), capB,
                                 arr(matches, i32), arr(results, i32), _dev(count), arr(fwd, f), _dev(workspace.buf),
                                 _stream()), entry)
    return (results, count) + ((fwd,) if want_distance else ())


def _mutual_host(np_dtype, entry, As, nAs, Bs, nBs, matches, capA, capB, want_distance):
    """The host twin of both mutual filters: descriptors of `np_dtype`, the C entry `entry`."""
    import numpy as np
    n = _pair_count(As, nAs, Bs, nBs, matches)
    As, Bs = (_pair_host_arrays(vs, np_dtype, flat=False) for vs in (As, Bs))
    matches = _pair_host_arrays(matches, np.int32, flat=False)
    capA, capB = _mutual_caps(As, Bs, matches, capA, capB)
    nA, nB = _pair_host_sizes(nAs), _pair_host_sizes(nBs)
    result, count, fwd = _pair_host_match_out(n, capA, want_distance)
    arr = _pair_host_table
    _check(getattr(lib(), entry)(n, arr(As), arr(nA), capA, arr(Bs), arr(nB), capB, arr(matches), arr(list(result)),
                                 _pair_host_ptr(count), arr(list(fwd)) if want_distance else None), entry)
    return (result, count) + ((fwd,) if want_distance else ())


def sift_match_mutual_batch_dev(As, d_nAs, Bs, d_nBs, matches, capA=None, capB=None, results=None, workspace=None,
                                want_distance=False):
    """Mutual-nearest-neighbour filter of n = len(As) <= MATCH_MUTUAL_MAX_BATCH match lists
    (nm_sift_match_mutual_batch_dev_f32): three launches on the current stream, no host read. As / Bs are float32 device
    descriptors (rows, 128), d_nAs / d_nBs int32 DEVICE sizes (e.g. SiftArena.desc, .num_items), matches[k] the int32 device
    list to filter (e.g. what sift_match_batch_dev wrote). Row i keeps its match j only when no row of A is nearer to column
    j and no earlier row is as near. results: n int32 device tensors of >= capA rows to write into (default: new; none may
    be a match list). workspace: a MatchMutualWorkspace (default: new). Returns (results, count[n]) and, with
    want_distance, the list of float32 (capA,) forward distances (+inf for a row without a claim). results[k] plugs into
    ransac_batch_dev, ransac_refit_batch_dev and align_points as matches."""
    return _mutual_dev(_torch().float32, "nm_sift_match_mutual_batch_dev_f32", MatchMutualWorkspace,
                       lambda n, capA, capB: (n, capA), As, d_nAs, Bs, d_nBs, matches, capA, capB, results, workspace,
                       want_distance)


def sift_match_mutual_host(As, nAs, Bs, nBs, matches, capA=None, capB=None, want_distance=False):
    """sift_match_mutual_batch_dev on the host (nm_sift_match_mutual_host_f32, the same functions): numpy in and out,
    bit-identical results. nAs / nBs are host ints. Returns (results (n, capA) int32, count (n,)) and, with want_distance,
    forward distances (n, capA) float32."""
    return _mutual_host("float32", "nm_sift_match_mutual_host_f32", As, nAs, Bs, nBs, matches, capA, capB, want_distance)


# ---- descriptor finish and the u8 matcher ----
DESC_L2, DESC_ROOT = 0, 1
DESC_FINISH_MAX_BATCH = MATCH_U8_MAX_BATCH = MATCH_MUTUAL_U8_MAX_BATCH = _PAIR_MAX_BATCH


def _finish_mode(mode):
    modes = {"l2": DESC_L2, "root": DESC_ROOT, DESC_L2: DESC_L2, DESC_ROOT: DESC_ROOT}
    if isinstance(mode, bool) or mode not in modes:
        raise NmError("descriptor finish: mode must be DESC_L2 / 'l2' or DESC_ROOT / 'root', got %r" % (mode,))
    return modes[mode]


def desc_finish_batch_dev(descs, d_counts, mode=DESC_L2, out_f32=None, out_u8=None, capacity=None):
    """The standard SIFT form of the raw descriptors of n = len(descs) <= DESC_FINISH_MAX_BATCH frames
    (nm_sift_desc_finish_batch_dev): L2-normalise, clip at 0.2, renormalise, with DESC_ROOT also RootSIFT; one launch on the
    current stream, no host read. descs: float32 device tensors (rows, 128) (SiftArena.desc), d_counts: int32 DEVICE row
    counts (SiftArena.num_items). out_f32 / out_u8: None (not wanted), True (new tensors) or a list of n device tensors
    (capacity, 128) float32 / uint8 to write into; out_f32 may be descs itself (in place). At least one is needed. Rows at
    and beyond a frame's count are not written (new tensors are zero-filled). u8 = min(255, rint(512 v)). Returns
    (out_f32, out_u8), None for the one not asked for."""
    torch = _torch()
    mode = _finish_mode(mode)
    f32_given, u8_given = isinstance(out_f32, (list, tuple)), isinstance(out_u8, (list, tuple))
    n = _pair_count(descs, d_counts, out_f32 if f32_given else None, out_u8 if u8_given else None)
    _pair_descriptors(descs, out_f32 if f32_given else (), out_u8 if u8_given else ())
    if (out_f32 is None or out_f32 is False) and (out_u8 is None or out_u8 is False):
        raise NmError("descriptor finish: ask for out_f32, out_u8 or both")
    capacity = _pair_cap(capacity, list(descs) + (list(out_f32) if f32_given else []) + (list(out_u8) if u8_given else []))
    device = _pair_device(list(descs) + list(d_counts) + (list(out_f32) if f32_given else []) +
                          (list(out_u8) if u8_given else []), list(d_counts))
    if out_f32 is True:
        out_f32 = [torch.zeros((capacity, 128), dtype=torch.float32, device=device) for _ in range(n)]
    if out_u8 is True:
        out_u8 = [torch.zeros((capacity, 128), dtype=torch.uint8, device=device) for _ in range(n)]
    out_f32, out_u8 = out_f32 or None, out_u8 or None
    arr = _pair_dev_table
    _check(lib().nm_sift_desc_finish_batch_dev(n, arr(descs, torch.float32), arr(d_counts, torch.int32), capacity,
                                               arr(out_f32, torch.float32), arr(out_u8, torch.uint8), mode, _stream()),
           "nm_sift_desc_finish_batch_dev")
    return out_f32, out_u8


def desc_finish_host(descs, counts, mode=DESC_L2, want_f32=True, want_u8=True, capacity=None, in_place=False):
    """desc_finish_batch_dev on the host (nm_sift_desc_finish_host, the same functions): numpy in and out, bit-identical
    results. counts are host ints. Returns (out_f32 (n, capacity, 128) float32 or None, out_u8 (n, capacity, 128) uint8 or
    None); rows at and beyond a count stay zero. in_place: the fp32 result is written over a copy of the input itself (the
    aliased call), rows at and beyond the count then keep the input's values."""
    import numpy as np
    mode = _finish_mode(mode)
    n = _pair_count(descs, counts)
    descs = _pair_host_arrays(descs, np.float32, flat=False)
    _pair_descriptors(descs)
    if not (want_f32 or want_u8):
        raise NmError("descriptor finish: ask for out_f32, out_u8 or both")
    capacity = _pair_cap(capacity, descs)
    if in_place:
        descs = [d[:capacity].copy() for d in descs]
    cnt = _pair_host_sizes(counts)
    f32 = (np.stack(descs) if in_place else np.zeros((n, capacity, 128), np.float32)) if want_f32 else None
    u8 = np.zeros((n, capacity, 128), np.uint8) if want_u8 else None
    src = list(f32) if in_place and want_f32 else descs
    arr = _pair_host_table
    _check(lib().nm_sift_desc_finish_host(n, arr(src), arr(cnt), capacity, arr(list(f32)) if want_f32 else None,
                                          arr(list(u8)) if want_u8 else None, mode), "nm_sift_desc_finish_host")
    return f32, u8


SELECT_MAX_BATCH = _PAIR_MAX_BATCH
SELECT_MAX_CAPACITY = 65536
SELECT_MAX_GRID = 64
# the payload of a selection: name -> (dtype name, trailing shape); x and y are required, the rest optional
_SELECT_PAYLOAD = (("x", "float32", ()), ("y", "float32", ()), ("desc", "float32", (128,)), ("desc_u8", "uint8", (128,)),
                   ("kpts", "float32", (4,)), ("orients", "float32", (2,)))


class SelectWorkspace(_PairWorkspace):
    """Device scratch of sift_select_batch_dev for up to n frames of `capacity` rows on a gx x gy grid (keys, cell
    segments, flags and each frame's parked payload pointers)."""
    _bytes_fn, _what, _shape_text = "nm_sift_select_workspace_bytes", "select workspace", "n %r / capacity %r / grid %r x %r"

    def __init__(self, n, capacity, gx, gy, device=None):
        self._alloc(device, n=n, capacity=capacity, gx=gx, gy=gy)


def _select_shape(n, capacity, given, gx, gy, keep):
    """The checks the C entries make on sizes, worded for Python; returns (capacity, keep)."""
    for name, _, tail in _SELECT_PAYLOAD:
        if any(tuple(t.shape[1:]) != tail for t in given.get(name) or ()):
            raise NmError("select: %s must be (rows,%s)" % (name, " %d" % tail[0] if tail else ""))
    capacity = _pair_cap(capacity, [t for ts in given.values() if ts is not None for t in ts])
    if capacity > SELECT_MAX_CAPACITY or not (1 <= gx <= SELECT_MAX_GRID and 1 <= gy <= SELECT_MAX_GRID):
        raise NmError("select: capacity %r above %d or grid %r x %r outside [1, %d]" % (capacity, SELECT_MAX_CAPACITY, gx, gy,
                                                                                       SELECT_MAX_GRID))
    if not 1 <= keep <= capacity:
        raise NmError("select: keep %r outside [1, capacity %d]" % (keep, capacity))
    return capacity


def sift_select_batch_dev(d_counts, xs, ys, width, height, scores=None, descs=None, descs_u8=None, kpts=None, orients=None,
                          gx=16, gy=9, keep=2048, capacity=None, out=None, want_index=True, workspace=None):
    """The strongest `keep` keypoints of n = len(xs) <= SELECT_MAX_BATCH frames, spread over a gx x gy grid
    (nm_sift_select_batch_dev): every cell's best row first, then every cell's second best, ..., written in ascending source
    order; four launches on the current stream, no host read. d_counts: int32 DEVICE row counts (SiftArena.num_items), xs /
    ys: float32 device coordinates in a width x height frame. scores: optional float32 device scores; without them descs
    (raw (rows, 128) float32 descriptors) is required and a row's score is its squared norm. descs, descs_u8 (rows, 128),
    kpts (rows, 4) and orients (rows, 2) are the optional payload: what is given is gathered. keep may not exceed the
    capacity (default: the smallest first dimension). out: the dict a former call returned, to write into the same tensors
    (what a graph capture needs, with a workspace); default: new tensors, zero-filled. Rows at and beyond a frame's output
    count are not written. Returns a dict: "x", "y" and a key per given payload list (lists of n tensors of `capacity`
    rows), "index" (the source row of every output row; None with want_index=False) and "count", an (n,) int32 DEVICE
    tensor of min(keep, rows)."""
    torch = _torch()
    given = dict(x=xs, y=ys, desc=descs, desc_u8=descs_u8, kpts=kpts, orients=orients)
    lists = [v for v in given.values() if v is not None]
    n = _pair_count(xs, d_counts, ys, scores, descs, descs_u8, kpts, orients)
    if scores is None and descs is None:
        raise NmError("select: give scores or descs")
    outs = [t for name in given if out is not None and out.get(name) is not None for t in out[name]]
    everything = [t for ts in lists for t in ts] + list(scores or ()) + outs
    capacity = _select_shape(n, capacity, dict(given, scores=scores, outs=outs or None), gx, gy, keep)
    device = _pair_device(everything + list(d_counts) + [workspace.buf if workspace is not None else None], list(d_counts))
    if out is None:
        out = {name: None if given[name] is None else
               [torch.zeros((capacity,) + tail, dtype=getattr(torch, dt), device=device) for _ in range(n)]
               for name, dt, tail in _SELECT_PAYLOAD}
        out["index"] = [torch.zeros(capacity, dtype=torch.int32, device=device) for _ in range(n)] if want_index else None
        out["count"] = torch.zeros(n, dtype=torch.int32, device=device)
    if any((out.get(name) is None) != (given[name] is None) for name in given) or out["count"].numel() != n or \
            any(out[name] is not None and len(out[name]) != n for name in list(given) + ["index"]):
        raise NmError("select: `out` does not fit this call's payload")
    workspace = _pair_workspace(SelectWorkspace, workspace, device, n, capacity, gx, gy)
    arr, i32 = _pair_dev_table, torch.int32
    tab = lambda src: [arr(src[name], getattr(torch, dt)) for name, dt, _ in _SELECT_PAYLOAD]
    ti, to = tab(given), tab(out)
    counts = [out["count"][k:k + 1] for k in range(n)]
    _check(lib().nm_sift_select_batch_dev(n, capacity, width, height, gx, gy, keep, arr(d_counts, i32), ti[0], ti[1],
                                          arr(scores, torch.float32), *ti[2:], *to, arr(out["index"], i32), arr(counts, i32),
                                          _dev(workspace.buf), _stream()), "nm_sift_select_batch_dev")
    return out


def sift_select_host(counts, xs, ys, width, height, scores=None, descs=None, descs_u8=None, kpts=None, orients=None,
                     gx=16, gy=9, keep=2048, capacity=None, fill=0):
    """sift_select_batch_dev on the host (nm_sift_select_host, the same score, cell and key functions): numpy in and out,
    bit-identical results. counts are host ints. Returns the same dict with (n, capacity, ...) arrays, "index" always and
    "count" an (n,) int32 array; rows at and beyond a count hold `fill`."""
    import numpy as np
    given = dict(x=xs, y=ys, desc=descs, desc_u8=descs_u8, kpts=kpts, orients=orients)
    n = _pair_count(xs, counts, ys, scores, descs, descs_u8, kpts, orients)
    if scores is None and descs is None:
        raise NmError("select: give scores or descs")
    for name, dt, _ in _SELECT_PAYLOAD:
        if given[name] is not None:
            given[name] = _pair_host_arrays(given[name], getattr(np, dt), flat=False)
    scores = None if scores is None else _pair_host_arrays(scores, np.float32)
    capacity = _select_shape(n, capacity, dict(given, scores=scores), gx, gy, keep)
    out = {name: None if given[name] is None else np.full((n, capacity) + tail, fill, getattr(np, dt))
           for name, dt, tail in _SELECT_PAYLOAD}
    out["index"] = np.full((n, capacity), fill, np.int32)
    out["count"] = np.full(n, fill, np.int32)
    arr = _pair_host_table
    ti = [arr(given[name]) for name, _, _ in _SELECT_PAYLOAD]
    to = [None if out[name] is None else arr(list(out[name])) for name, _, _ in _SELECT_PAYLOAD]
    cnt_in = _pair_host_sizes(counts)
    cnt_out = [out["count"][k:k + 1] for k in range(n)]
    _check(lib().nm_sift_select_host(n, capacity, width, height, gx, gy, keep, arr(cnt_in), ti[0], ti[1], arr(scores),
                                     *ti[2:], *to, arr(list(out["index"])), arr(cnt_out)), "nm_sift_select_host")
    return out


def _u8_caps(As, Bs, results, capA, capB):
    _pair_descriptors(As, Bs)
    return _pair_cap(capA, list(As) + list(results or ())), _pair_cap(capB, list(Bs))


class MatchU8Workspace(_PairWorkspace):
    """Device scratch of sift_match_u8_batch_dev for up to n pairs of capA x capB rows (the integer row norms)."""
    _bytes_fn, _what, _shape_text = "nm_sift_match_u8_workspace_bytes", "u8-match workspace", "n %r / capA %r / capB %r"

    def __init__(self, n, capA, capB, device=None):
        self._alloc(device, n=n, capA=capA, capB=capB)


def sift_match_u8_batch_dev(As, d_nAs, Bs, d_nBs, results=None, ambiguity=0.8, workspace=None, capA=None, capB=None):
    """Brute-force ratio-test matching of n = len(As) <= MATCH_U8_MAX_BATCH pairs of uint8 descriptors on the i8 matrix cores
    (nm_sift_match_u8_batch_dev): two launches on the current stream, no host read. As / Bs are uint8 device tensors
    (rows, 128) (out_u8 of desc_finish_batch_dev), d_nAs / d_nBs int32 DEVICE sizes. results: n int32 device tensors of
    >= capA rows to write into (default: new, filled with -1); a row whose second-best distance is 0 keeps its entry, rows
    at and beyond nA too. The result equals sift_match_batch_dev on float copies of the same bytes. workspace: a
    MatchU8Workspace (default: new). Returns results."""
    torch = _torch()
    n = _pair_count(As, d_nAs, Bs, d_nBs, results)
    capA, capB = _u8_caps(As, Bs, results, capA, capB)
    device = _pair_device(list(As) + list(d_nAs) + list(Bs) + list(d_nBs) + list(results or ()) +
                          [workspace.buf if workspace is not None else None], list(d_nAs) + list(d_nBs))
    if results is None:
        results = [torch.full((capA,), -1, dtype=torch.int32, device=device) for _ in range(n)]
    workspace = _pair_workspace(MatchU8Workspace, workspace, device, n, capA, capB)
    arr, u8, i32 = _pair_dev_table, torch.uint8, torch.int32
    _check(lib().nm_sift_match_u8_batch_dev(n, arr(As, u8), arr(d_nAs, i32), capA, arr(Bs, u8), arr(d_nBs, i32), capB,
                                            arr(results, i32), float(ambiguity), _dev(workspace.buf), _stream()),
           "nm_sift_match_u8_batch_dev")
    return results


def sift_match_u8_host(As, nAs, Bs, nBs, ambiguity=0.8, capA=None, capB=None, prior=-1):
    """sift_match_u8_batch_dev on the host (nm_sift_match_u8_host): numpy in and out, identical results. nAs / nBs are host
    ints. prior: what the result rows are pre-filled with (a value, or an (n, capA) array). Returns (n, capA) int32."""
    import numpy as np
    n = _pair_count(As, nAs, Bs, nBs)
    As, Bs = (_pair_host_arrays(vs, np.uint8, flat=False) for vs in (As, Bs))
    capA, capB = _u8_caps(As, Bs, None, capA, capB)
    result = np.empty((n, capA), np.int32)
    result[...] = prior
    nA, nB = _pair_host_sizes(nAs), _pair_host_sizes(nBs)
    arr = _pair_host_table
    _check(lib().nm_sift_match_u8_host(n, arr(As), arr(nA), capA, arr(Bs), arr(nB), capB, arr(list(result)),
                                       float(ambiguity)), "nm_sift_match_u8_host")
    return result


MATCH_KNN_U8_MAX_BATCH = _PAIR_MAX_BATCH
MATCH_KNN_U8_MAX_K = 8
KNN_U8_NONE = (-1, 0x7fffffff)                 # index and distance of a slot without a candidate


class MatchKnnU8Workspace(_PairWorkspace):
    """Device scratch of sift_match_knn_u8_batch_dev for up to n pairs of capA x capB rows (the integer row norms)."""
    _bytes_fn, _what, _shape_text = "nm_sift_match_knn_u8_workspace_bytes", "u8 k-NN workspace", "n %r / capA %r / capB %r"

    def __init__(self, n, capA, capB, device=None):
        self._alloc(device, n=n, capA=capA, capB=capB)


def _knn_k(k, *lists):
    """k of a k-NN call, in range; the given output tensors are (rows, k)."""
    if not isinstance(k, int) or not 1 <= k <= MATCH_KNN_U8_MAX_K:
        raise NmError("k-NN: k %r outside [1, %d]" % (k, MATCH_KNN_U8_MAX_K))
    if any(t.ndim != 2 or t.shape[1] != k for ts in lists for t in ts or ()):
        raise NmError("k-NN: index and distance tensors must be (rows, %d)" % k)
    return k


def sift_match_knn_u8_batch_dev(As, d_nAs, Bs, d_nBs, k, indices=None, distances=None, want_distance=True, workspace=None,
                                capA=None, capB=None):
    """The k nearest rows of Bs[p] for every row of As[p], n = len(As) <= MATCH_KNN_U8_MAX_BATCH pairs of uint8 descriptors
    on the i8 matrix cores (nm_sift_match_knn_u8_batch_dev): two launches on the current stream, no host read. As / Bs are
    uint8 device tensors (rows, 128) (out_u8 of desc_finish_batch_dev), d_nAs / d_nBs int32 DEVICE sizes, k in
    [1, MATCH_KNN_U8_MAX_K]. Row i of indices[p] lists the candidates by (distance, index) ascending, distances[p] their exact
    integer squared distances; slots at and beyond min(k, nB) hold -1 / 0x7fffffff. indices / distances: n int32 device
    tensors (>= capA, k) to write into (default: new, filled with -1 / 0x7fffffff); rows at and beyond nA keep their
    contents. want_distance=False (and no distances given) asks for indices only. workspace: a MatchKnnU8Workspace
    (default: new). Returns (indices, distances), distances None when not wanted."""
    torch = _torch()
    want_distance = want_distance or distances is not None
    n = _pair_count(As, d_nAs, Bs, d_nBs, indices, distances)
    k = _knn_k(k, indices, distances)
    capA, capB = _u8_caps(As, Bs, list(indices or ()) + list(distances or ()), capA, capB)
    device = _pair_device(list(As) + list(d_nAs) + list(Bs) + list(d_nBs) + list(indices or ()) + list(distances or ()) +
                          [workspace.buf if workspace is not None else None], list(d_nAs) + list(d_nBs))
    new = lambda fill: [torch.full((capA, k), fill, dtype=torch.int32, device=device) for _ in range(n)]
    indices = new(KNN_U8_NONE[0]) if indices is None else indices
    distances = (new(KNN_U8_NONE[1]) if distances is None else distances) if want_distance else None
    workspace = _pair_workspace(MatchKnnU8Workspace, workspace, device, n, capA, capB)
    arr, u8, i32 = _pair_dev_table, torch.uint8, torch.int32
    _check(lib().nm_sift_match_knn_u8_batch_dev(n, arr(As, u8), arr(d_nAs, i32), capA, arr(Bs, u8), arr(d_nBs, i32), capB, k,
                                                arr(indices, i32), arr(distances, i32), _dev(workspace.buf), _stream()),
           "nm_sift_match_knn_u8_batch_dev")
    return indices, distances


def sift_match_knn_u8_host(As, nAs, Bs, nBs, k, capA=None, capB=None, want_distance=True, prior=KNN_U8_NONE):
    """sift_match_knn_u8_batch_dev on the host (nm_sift_match_knn_u8_host): numpy in and out, identical results. nAs / nBs
    are host ints. prior: what the index and the distance rows are pre-filled with (a pair of values or of (n, capA, k)
    arrays). Returns (indices, distances), (n, capA, k) int32 each, distances None when not wanted."""
    import numpy as np
    n = _pair_count(As, nAs, Bs, nBs)
    k = _knn_k(k)
    As, Bs = (_pair_host_arrays(vs, np.uint8, flat=False) for vs in (As, Bs))
    capA, capB = _u8_caps(As, Bs, None, capA, capB)
    index = np.empty((n, capA, k), np.int32)
    index[...] = prior[0]
    dist = None
    if want_distance:
        dist = np.empty((n, capA, k), np.int32)
        dist[...] = prior[1]
    nA, nB = _pair_host_sizes(nAs), _pair_host_sizes(nBs)
    arr = _pair_host_table
    _check(lib().nm_sift_match_knn_u8_host(n, arr(As), arr(nA), capA, arr(Bs), arr(nB), capB, k, arr(list(index)),
                                           arr(list(dist)) if want_distance else None), "nm_sift_match_knn_u8_host")
    return index, dist


class MatchMutualU8Workspace(_PairWorkspace):
    """Device scratch of sift_match_mutual_u8_batch_dev for up to n pairs of capA x capB rows (the integer norms of A's
    rows and the compacted claims)."""
    _bytes_fn, _what, _shape_text = "nm_sift_match_mutual_u8_workspace_bytes", "mutual-u8 workspace", "n %r / capA %r / capB %r"

    def __init__(self, n, capA, capB, device=None):
        self._alloc(device, n=n, capA=capA, capB=capB)


def sift_match_mutual_u8_batch_dev(As, d_nAs, Bs, d_nBs, matches, capA=None, capB=None, results=None, workspace=None,
                                   want_distance=False):
    """Mutual-nearest-neighbour filter of n = len(As) <= MATCH_MUTUAL_U8_MAX_BATCH match lists over uint8 descriptors on the
    i8 matrix cores (nm_sift_match_mutual_u8_batch_dev): three launches on the current stream, no host read. As / Bs are
    uint8 device descriptors (rows, 128) (out_u8 of desc_finish_batch_dev), d_nAs / d_nBs int32 DEVICE sizes, matches[k] the
    int32 device list to filter (e.g. what sift_match_u8_batch_dev wrote). Row i keeps its match j only when no row of A is
    nearer to column j and no earlier row is as near; distances are exact integers. results: n int32 device tensors of
    >= capA rows to write into (default: new; none may be a match list). workspace: a MatchMutualU8Workspace (default: new).
    Returns (results, count[n]) and, with want_distance, the list of float32 (capA,) forward distances (+inf for a row
    without a claim). The outputs equal sift_match_mutual_batch_dev's on float copies of the same bytes bit for bit.
    results[k] plugs into ransac_batch_dev, ransac_refit_batch_dev and align_points as matches."""
    return _mutual_dev(_torch().uint8, "nm_sift_match_mutual_u8_batch_dev", MatchMutualU8Workspace,
                       lambda n, capA, capB: (n, capA, capB), As, d_nAs, Bs, d_nBs, matches, capA, capB, results, workspace,
                       want_distance)


def sift_match_mutual_u8_host(As, nAs, Bs, nBs, matches, capA=None, capB=None, want_distance=False):
    """sift_match_mutual_u8_batch_dev on the host (nm_sift_match_mutual_u8_host): numpy in and out, identical results.
    nAs / nBs are host ints. Returns (results (n, capA) int32, count (n,)) and, with want_distance, forward distances
    (n, capA) float32."""
    return _mutual_host("uint8", "nm_sift_match_mutual_u8_host", As, nAs, Bs, nBs, matches, capA, capB, want_distance)


MATCH_GUIDED_U8_MAX_BATCH = _PAIR_MAX_BATCH


def sift_match_guided_u8_batch_dev(As, axs, ays, d_nAs, Bs, bxs, bys, d_nBs, H, status=None, radius2=9.0, ambiguity=0.8,
                                   max_distance=float("inf"), capA=None, capB=None, results=None, want_distance=False):
    """Homography-guided matching of n = len(As) <= MATCH_GUIDED_U8_MAX_BATCH pairs of uint8 descriptors
    (nm_sift_match_guided_u8_batch_dev): three launches on the current stream, no host read, no workspace. As / Bs are uint8
    device descriptors (rows, 128) (out_u8 of desc_finish_batch_dev, 16-byte aligned); every other argument and the return
    value are those of sift_match_guided_batch_dev. Distances are exact integers: results, count and best distances equal
    sift_match_guided_batch_dev's on float copies of the same bytes bit for bit."""
    return _guided_dev(_torch().uint8, "nm_sift_match_guided_u8_batch_dev", As, axs, ays, d_nAs, Bs, bxs, bys, d_nBs, H,
                       status, radius2, ambiguity, max_distance, capA, capB, results, want_distance)


def sift_match_guided_u8_host(As, axs, ays, nAs, Bs, bxs, bys, nBs, H, status=None, radius2=9.0, ambiguity=0.8,
                              max_distance=float("inf"), capA=None, capB=None, want_distance=False):
    """sift_match_guided_u8_batch_dev on the host (nm_sift_match_guided_u8_host, the same functions): numpy uint8
    descriptors in (no other dtype is converted), identical results out. nAs / nBs are host ints. Returns (results (n, capA)
    int32, count (n,)) and, with want_distance, best distances (n, capA) float32."""
    import numpy as np
    if any(np.asarray(v).dtype != np.uint8 for vs in (As, Bs) for v in vs):
        raise NmError("guided u8 matching: descriptors must be uint8")
    return _guided_host("uint8", "nm_sift_match_guided_u8_host", As, axs, ays, nAs, Bs, bxs, bys, nBs, H, status, radius2,
                        ambiguity, max_distance, capA, capB, want_distance)


MOSAIC_MAX_BATCH = _FRAMES_MAX_BATCH
_MOSAIC_OFFSET_LIMIT = 1 << 20


def _mosaic_check_geometry(n, fw, fh, cw, ch, ox, oy):
    if not 0 < n <= MOSAIC_MAX_BATCH:
        raise NmError("mosaic: %d frames (1 .. %d)" % (n, MOSAIC_MAX_BATCH))
    _size_check("mosaic", "frame", int(fw), int(fh))
    _size_check("mosaic", "canvas", int(cw), int(ch))
    if any(abs(int(v)) >= _MOSAIC_OFFSET_LIMIT for v in (ox, oy)):
        raise NmError("mosaic: |ox|, |oy| must be below 2^20")


def mosaic_plan(H, status, fw, fh, cw, ch, ox, oy, M_first=None):
    """Placement records of n = H.shape[0] + 1 frames from the pairwise homographies (nm_mosaic_plan_f32), one launch on
    the current stream, no host read. H: float32 device (n-1, 9) or (n-1, 3, 3), pair k mapping frame k to frame k+1 (e.g.
    ransac_batch_dev's H_best); status: int32 device (n-1,) or None (every link valid); frame-0 pixel (0, 0) lands on
    canvas pixel (ox, oy); M_first: float32 device (9,) or (3, 3) map from the reference coordinates to frame 0, None =
    identity. Returns (records int32 (n, 16): m = records[:, :9].view(float32), then tx, ty, nw, nh, placed, 0, 0;
    chain float32 (n, 9); extent float32 (4,))."""
    torch = _torch()
    n = H.shape[0] + 1
    _mosaic_check_geometry(n, fw, fh, cw, ch, ox, oy)
    if H.numel() != 9 * (n - 1):
        raise NmError("mosaic_plan: H must hold (n-1) x 9 floats")
    device = _on_current_device([H, status, M_first], "mosaic_plan")
    if status is not None and status.numel() != n - 1:
        raise NmError("mosaic_plan: status must hold n-1 values")
    if M_first is not None and M_first.numel() != 9:
        raise NmError("mosaic_plan: M_first must hold 9 floats")
    records = torch.empty((n, 16), dtype=torch.int32, device=device)
    chain = torch.empty((n, 9), dtype=torch.float32, device=device)
    extent = torch.empty(4, dtype=torch.float32, device=device)
    _check(lib().nm_mosaic_plan_f32(n, _dev(H, torch.float32) if n > 1 else None, _opt(status, torch.int32), fw, fh, cw, ch,
                                    ox, oy, _opt(M_first, torch.float32), _dev(records), _dev(chain), _dev(extent), _stream()),
           "nm_mosaic_plan_f32")
    return records, chain, extent


def mosaic_plan_host(H, status, fw, fh, cw, ch, ox, oy, M_first=None):
    """mosaic_plan on the host (nm_mosaic_plan_host_f32, the same functions): numpy in and out, bit-identical results."""
    import numpy as np
    H = np.ascontiguousarray(H, dtype=np.float32).reshape(-1, 9)
    n = H.shape[0] + 1
    _mosaic_check_geometry(n, fw, fh, cw, ch, ox, oy)
    if status is not None:
        status = np.ascontiguousarray(status, dtype=np.int32).reshape(-1)
        if status.size != n - 1:
            raise NmError("mosaic_plan_host: status must hold n-1 values")
    if M_first is not None:
        M_first = np.ascontiguousarray(M_first, dtype=np.float32).reshape(-1)
        if M_first.size != 9:
            raise NmError("mosaic_plan_host: M_first must hold 9 floats")
    records = np.zeros((n, 16), np.int32)
    chain = np.zeros((n, 9), np.float32)
    extent = np.zeros(4, np.float32)
    ptr = _pair_host_ptr
    _check(lib().nm_mosaic_plan_host_f32(n, ptr(H) if n > 1 else None, ptr(status), fw, fh, cw, ch, ox, oy, ptr(M_first),
                                         ptr(records), ptr(chain), ptr(extent)), "nm_mosaic_plan_host_f32")
    return records, chain, extent


def transform_blend_batch(canvas, canvas_wts, frames, masks, wts, records):
    """n = len(frames) <= MOSAIC_MAX_BATCH frames into the canvas IN PLACE, one launch (nm_transform_blend_batch): the same
    bits as transform_blend(canvas, canvas_wts, frames[k], nw_k, nh_k, m_k, tx_k, ty_k, masks[k], wts[k]) for k in order,
    with the fields of records[k] (int32 device (n, 16), e.g. from mosaic_plan). masks / wts: one scalar plane for every
    frame, or a list of n planes of one format."""
    _blend_batch("nm_transform_blend_batch", canvas, canvas_wts, frames, masks, wts, records, ())


def transform_blend_batch_gain(canvas, canvas_wts, frames, masks, wts, records, gains=None):
    """transform_blend_batch with frame k's B, G, R multiplied by gains[k] (float32 device (n, 3), e.g. mosaic_gains') between
    the sample and the blend (nm_transform_blend_batch_gain), one launch. canvas_wts is the ungained call's; with gains None
    or all 1 so is the canvas, bit for bit."""
    torch = _torch()
    if gains is not None and (tuple(gains.shape) != (len(frames), 3) or gains.device != canvas.device):
        raise NmError("transform_blend_batch_gain: gains must be float32 (n, 3) on the canvas' device")
    _blend_batch("nm_transform_blend_batch_gain", canvas, canvas_wts, frames, masks, wts, records, (_opt(gains, torch.float32),))


def _blend_batch(entry, canvas, canvas_wts, frames, masks, wts, records, extra):
    torch, what = _torch(), "transform_blend_batch"
    n, fw, fh = _frames_check(what, frames)
    masks, wts, mfmt, wfmt = _scalar_planes(what, n, fw, fh, masks, wts)
    cw, ch = _canvas_check(what, canvas, canvas_wts)
    _records_check(what, records, n)
    _on_current_device([canvas, canvas_wts, records] + list(frames) + masks + wts, what)
    _check(getattr(lib(), entry)(_dev(canvas, torch.uint8), cw, ch, _dev(canvas_wts, torch.float32), n,
                                 _pair_dev_table(frames, torch.uint8), fw, fh, _pair_dev_table(masks, masks[0].dtype), mfmt,
                                 _pair_dev_table(wts, wts[0].dtype), wfmt, _dev(records, torch.int32), *extra, _stream()), entry)


def mosaic_place(chain, fw, fh, cw, ch, ox, oy, frame_status=None):
    """Placement records of the n = chain.shape[0] frames of a GIVEN chain (nm_mosaic_place_f32), e.g. mosaic_adjust's
    chain_out: the placement half of mosaic_plan, one launch, no host read. chain float32 device (n, 9) or (n, 3, 3);
    frame_status int32 device (n,) or None. Returns (records int32 (n, 16), extent float32 (4,)) as mosaic_plan does; on
    mosaic_plan's own chain they equal its records and extent bit for bit."""
    torch = _torch()
    n = chain.shape[0]
    _mosaic_check_geometry(n, fw, fh, cw, ch, ox, oy)
    if chain.numel() != 9 * n or (frame_status is not None and frame_status.numel() != n):
        raise NmError("mosaic_place: chain must hold n x 9 floats and frame_status n values")
    device = _on_current_device([chain, frame_status], "mosaic_place")
    records = torch.empty((n, 16), dtype=torch.int32, device=device)
    extent = torch.empty(4, dtype=torch.float32, device=device)
    _check(lib().nm_mosaic_place_f32(n, _dev(chain, torch.float32), _opt(frame_status, torch.int32), fw, fh, cw, ch, ox, oy,
                                     _dev(records), _dev(extent), _stream()), "nm_mosaic_place_f32")
    return records, extent


def mosaic_place_host(chain, fw, fh, cw, ch, ox, oy, frame_status=None):
    """mosaic_place on the host (nm_mosaic_place_host_f32, the same functions): numpy in and out, bit-identical results."""
    import numpy as np
    chain = np.ascontiguousarray(chain, dtype=np.float32).reshape(-1, 9)
    n = chain.shape[0]
    _mosaic_check_geometry(n, fw, fh, cw, ch, ox, oy)
    if frame_status is not None:
        frame_status = np.ascontiguousarray(frame_status, dtype=np.int32).reshape(-1)
        if frame_status.size != n:
            raise NmError("mosaic_place_host: frame_status must hold n values")
    records = np.zeros((n, 16), np.int32)
    extent = np.zeros(4, np.float32)
    _check(lib().nm_mosaic_place_host_f32(n, chain.ctypes.data, _pair_host_ptr(frame_status), fw, fh, cw, ch, ox, oy,
                                          records.ctypes.data, extent.ctypes.data), "nm_mosaic_place_host_f32")
    return records, extent


MOSAIC_ADJUST_MAX_LINKS, MOSAIC_ADJUST_MAX_ITERATIONS, MOSAIC_ADJUST_SUMS = 256, 16, 153
MOSAIC_ADJUST_CONVERGED_STEP = 2.0 ** -7
MOSAIC_ADJUST_STATS = ("cost_first", "cost_last", "rows", "links", "unknown_frames", "steps", "last_step", "end")
(MOSAIC_ADJUST_END_ITERATIONS, MOSAIC_ADJUST_END_CONVERGED, MOSAIC_ADJUST_END_UNUSABLE, MOSAIC_ADJUST_END_NO_LINK,
 MOSAIC_ADJUST_END_SINGULAR, MOSAIC_ADJUST_END_STEP, MOSAIC_ADJUST_END_COST_ROSE) = range(7)


class MosaicAdjustWorkspace(_PairWorkspace):
    """Device scratch for nm_mosaic_adjust_dev_f32: n frames, L links."""
    _bytes_fn, _what, _shape_text = "nm_mosaic_adjust_workspace_bytes", "mosaic adjustment workspace", "n=%d L=%d"

    def __init__(self, n, L, device):
        self._alloc(device, n=n, L=L)


def _mosaic_adjust_check(n, lists, link_a, link_b, anchor, fw, fh, iterations, min_rows, damping, max_step):
    L = len(link_a)
    if not 2 <= n <= MOSAIC_MAX_BATCH or not 1 <= L <= MOSAIC_ADJUST_MAX_LINKS or len(link_b) != L or \
            any(len(v) != L for v in lists):
        raise NmError("mosaic adjustment: n in [2, %d] frames and lists of one length in [1, %d] expected"
                      % (MOSAIC_MAX_BATCH, MOSAIC_ADJUST_MAX_LINKS))
    if any(not (0 <= int(a) < n and 0 <= int(b) < n and int(a) != int(b)) for a, b in zip(link_a, link_b)):
        raise NmError("mosaic adjustment: a link joins two different frames in [0, n)")
    if not 0 <= int(anchor) < n:
        raise NmError("mosaic adjustment: anchor %r outside [0, n)" % (anchor,))
    _size_check("mosaic adjustment", "frame", fw, fh)
    if int(iterations) != iterations or not 1 <= iterations <= MOSAIC_ADJUST_MAX_ITERATIONS:
        raise NmError("mosaic adjustment: iterations %r outside [1, %d]" % (iterations, MOSAIC_ADJUST_MAX_ITERATIONS))
    if int(min_rows) != min_rows or min_rows < 4:
        raise NmError("mosaic adjustment: min_rows %r must be an integer >= 4" % (min_rows,))
    if not (math.isfinite(damping) and damping >= 0 and math.isfinite(max_step) and max_step > 0):
        raise NmError("mosaic adjustment: damping must be finite and >= 0, max_step finite and > 0")
    return L, (C.c_int * L)(*[int(a) for a in link_a]), (C.c_int * L)(*[int(b) for b in link_b])


def mosaic_adjust(link_a, link_b, src_xs, src_ys, d_nAs, dst_xs, dst_ys, matches, chain, fw, fh, anchor=0, mask=None,
                  link_status=None, iterations=5, min_rows=8, damping=1e-6, max_step=64.0, capA=None, workspace=None):
    """Joint least-squares adjustment of the n = chain.shape[0] <= 64 frame maps of a mosaic over L = len(link_a) <= 256
    links, loop closures included (nm_mosaic_adjust_dev_f32): (iterations + 1) x (ceil(L / 64) + 1) launches on the current
    stream, no host read. link_a, link_b: host ints, link l matches frame link_a[l] (src) to frame link_b[l] (dst); the
    per-link tensors are those of ransac_refit_batch_dev; chain float32 device (n, 9), e.g. mosaic_plan's; mask uint8 device
    (L, capA) or None, e.g. the refit's; link_status int32 device (L,) or None, e.g. link_verify_batch_dev's. Returns
    (chain_out[n, 9], frame_status[n], link_rms[L, 2], stats[8]): stats float64 in the order of MOSAIC_ADJUST_STATS, its last
    entry one of MOSAIC_ADJUST_END_*. chain_out and frame_status go to mosaic_place as they are."""
    torch = _torch()
    n = chain.shape[0]
    lists = (src_xs, src_ys, d_nAs, dst_xs, dst_ys, matches)
    L, la, lb = _mosaic_adjust_check(n, lists, link_a, link_b, anchor, fw, fh, iterations, min_rows, damping, max_step)
    capA = _pair_cap(capA, list(src_xs) + list(src_ys) + list(matches))
    if chain.numel() != 9 * n or (link_status is not None and link_status.numel() != L) or \
            (mask is not None and tuple(mask.shape) != (L, capA)):
        raise NmError("mosaic adjustment: chain n x 9, link_status L values and mask (L, capA) expected")
    device = _pair_device([t for ts in lists for t in ts] + [chain, mask, link_status,
                                                              workspace.buf if workspace is not None else None], d_nAs)
    workspace = _pair_workspace(MosaicAdjustWorkspace, workspace, device, n, L)
    chain_out = torch.empty((n, 9), dtype=torch.float32, device=device)
    fstat = torch.empty(n, dtype=torch.int32, device=device)
    rms = torch.empty((L, 2), dtype=torch.float64, device=device)
    stats = torch.empty(len(MOSAIC_ADJUST_STATS), dtype=torch.float64, device=device)
    tables = _point_tables_dev(*lists)
    _check(lib().nm_mosaic_adjust_dev_f32(n, L, la, lb, *tables[:3], capA, *tables[3:], _opt(mask, torch.uint8),
                                          _opt(link_status, torch.int32), _dev(chain, torch.float32), int(anchor), fw, fh,
                                          int(iterations), int(min_rows), damping, max_step, _dev(chain_out), _dev(fstat),
                                          _dev(rms), _dev(stats), _dev(workspace.buf), _stream()), "nm_mosaic_adjust_dev_f32")
    return chain_out, fstat, rms, stats


def _mosaic_adjust_host_rows(src_xs, src_ys, dst_xs, dst_ys, matches, capA):
    import numpy as np
    src_xs, src_ys, dst_xs, dst_ys = (_pair_host_arrays(vs, np.float32) for vs in (src_xs, src_ys, dst_xs, dst_ys))
    matches = _pair_host_arrays(matches, np.int32)
    capA = _pair_cap(capA, src_xs + src_ys + matches)
    for m, x, y in zip(matches, dst_xs, dst_ys):
        if m.size and int(m.max()) >= min(x.size, y.size):
            raise NmError("a match points beyond the destination coordinates")
    return src_xs, src_ys, dst_xs, dst_ys, matches, capA


def mosaic_adjust_host(link_a, link_b, src_xs, src_ys, nAs, dst_xs, dst_ys, matches, chain, fw, fh, anchor=0, mask=None,
                       link_status=None, iterations=5, min_rows=8, damping=1e-6, max_step=64.0, capA=None):
    """mosaic_adjust on the host (nm_mosaic_adjust_host_f32, the same functions in the same summation order): numpy in and
    out, bit-identical results. nAs are host ints."""
    import numpy as np
    chain = np.ascontiguousarray(chain, dtype=np.float32).reshape(-1, 9)
    n = chain.shape[0]
    lists = (src_xs, src_ys, nAs, dst_xs, dst_ys, matches)
    L, la, lb = _mosaic_adjust_check(n, lists, link_a, link_b, anchor, fw, fh, iterations, min_rows, damping, max_step)
    src_xs, src_ys, dst_xs, dst_ys, matches, capA = _mosaic_adjust_host_rows(src_xs, src_ys, dst_xs, dst_ys, matches, capA)
    mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    link_status = None if link_status is None else np.ascontiguousarray(link_status, dtype=np.int32).reshape(-1)
    if (link_status is not None and link_status.size != L) or (mask is not None and mask.shape != (L, capA)):
        raise NmError("mosaic adjustment: link_status L values and mask (L, capA) expected")
    nA = _pair_host_sizes(nAs)
    chain_out = np.zeros((n, 9), np.float32)
    fstat = np.zeros(n, np.int32)
    rms = np.zeros((L, 2), np.float64)
    stats = np.zeros(len(MOSAIC_ADJUST_STATS), np.float64)
    arr, ptr = _pair_host_table, _pair_host_ptr
    _check(lib().nm_mosaic_adjust_host_f32(n, L, la, lb, arr(src_xs), arr(src_ys), arr(nA), capA, arr(dst_xs), arr(dst_ys),
                                           arr(matches), ptr(mask), ptr(link_status), ptr(chain), int(anchor), fw, fh,
                                           int(iterations), int(min_rows), damping, max_step, ptr(chain_out), ptr(fstat),
                                           ptr(rms), ptr(stats)), "nm_mosaic_adjust_host_f32")
    return chain_out, fstat, rms, stats


def mosaic_adjust_sums_host(src_x, src_y, nA, dst_x, dst_y, matches, fw, fh, Ga, Gb, mask=None, capA=None):
    """One link's 153 sums and its contributing rows under the normalised maps Ga, Gb (float64, 9 values each, element 8
    = 1) in the adjustment's summation order (nm_mosaic_adjust_sums_host_f32), for tests: (sums float64 (153,), count)."""
    import numpy as np
    (sx,), (sy,), (dx,), (dy,), (mt,), capA = _mosaic_adjust_host_rows([src_x], [src_y], [dst_x], [dst_y], [matches], capA)
    mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
    if mask is not None and mask.size < capA:
        raise NmError("mosaic adjustment: the mask is smaller than the capacity")
    Ga, Gb = (np.ascontiguousarray(G, dtype=np.float64).reshape(-1) for G in (Ga, Gb))
    if Ga.size != 9 or Gb.size != 9:
        raise NmError("mosaic adjustment: Ga and Gb hold 9 values each")
    sums = np.zeros(MOSAIC_ADJUST_SUMS, np.float64)
    count = C.c_int(0)
    ptr = _pair_host_ptr
    _check(lib().nm_mosaic_adjust_sums_host_f32(ptr(sx), ptr(sy), int(nA), capA, ptr(dx), ptr(dy), ptr(mt), ptr(mask), fw, fh,
                                                ptr(Ga), ptr(Gb), ptr(sums), C.byref(count)), "nm_mosaic_adjust_sums_host_f32")
    return sums, count.value


EXPOSURE_MAX_LINKS, EXPOSURE_SUMS = MOSAIC_ADJUST_MAX_LINKS, 7
EXPOSURE_PER_CHANNEL, EXPOSURE_COMMON = 0, 1
EXPOSURE_STATS = ("cost_unit_b", "cost_unit_g", "cost_unit_r", "cost_b", "cost_g", "cost_r", "links", "frames", "end")
EXPOSURE_END_OK, EXPOSURE_END_NO_LINK, EXPOSURE_END_SINGULAR = range(3)
EXPOSURE_SIGMA_MIN, EXPOSURE_SIGMA_MAX = 1e-6, 1e6


def _exposure_links(n, link_a, link_b):
    L = len(link_a)
    if not 1 <= n <= MOSAIC_MAX_BATCH or not 1 <= L <= EXPOSURE_MAX_LINKS or len(link_b) != L:
        raise NmError("mosaic exposure: n in [1, %d] frames and two link lists of one length in [1, %d] expected"
                      % (MOSAIC_MAX_BATCH, EXPOSURE_MAX_LINKS))
    if any(not (0 <= int(a) < n and 0 <= int(b) < n and int(a) != int(b)) for a, b in zip(link_a, link_b)):
        raise NmError("mosaic exposure: a link joins two different frames in [0, n)")
    return L, (C.c_int * L)(*[int(a) for a in link_a]), (C.c_int * L)(*[int(b) for b in link_b])


def _exposure_sums_check(frames, link_a, link_b, stride, lo, hi):
    n, fw, fh = _frames_check("mosaic exposure", frames)
    L, la, lb = _exposure_links(n, link_a, link_b)
    _lattice_check("mosaic exposure", fw, fh, stride)
    if any(int(v) != v for v in (lo, hi)) or not 0 <= lo <= hi <= 255:
        raise NmError("mosaic exposure: bytes 0 <= lo <= hi <= 255 expected")
    return n, fw, fh, L, la, lb


def _exposure_gains_check(n, link_a, link_b, min_pixels, sigma_n, sigma_g, g_min, g_max, mode):
    L, la, lb = _exposure_links(n, link_a, link_b)
    if int(min_pixels) != min_pixels or min_pixels < 1:
        raise NmError("mosaic exposure: min_pixels %r must be an integer >= 1" % (min_pixels,))
    if not all(EXPOSURE_SIGMA_MIN <= s <= EXPOSURE_SIGMA_MAX for s in (sigma_n, sigma_g)):
        raise NmError("mosaic exposure: sigma_n and sigma_g lie in [%g, %g]" % (EXPOSURE_SIGMA_MIN, EXPOSURE_SIGMA_MAX))
    if not (math.isfinite(g_min) and math.isfinite(g_max) and 0 < g_min <= 1 <= g_max):
        raise NmError("mosaic exposure: 0 < g_min <= 1 <= g_max, both finite, expected")
    if mode not in (EXPOSURE_PER_CHANNEL, EXPOSURE_COMMON):
        raise NmError("mosaic exposure: unknown mode %r" % (mode,))
    return L, la, lb


def mosaic_exposure_sums(frames, link_a, link_b, H, link_status=None, mask=None, stride=4, lo=5, hi=250, sums=None):
    """Per-link, per-channel overlap sums of n = len(frames) <= 64 BGRA frames over L = len(link_a) <= 256 links
    (nm_mosaic_exposure_sums_dev): two launches on the current stream (the first zeroes the sums), no host read. frames:
    uint8 device (fh, fw, 4), tensors may repeat; link_a, link_b: host ints; H float32 device (L, 9) or (L, 3, 3), H_l mapping frame
    link_a[l] to frame link_b[l]; link_status int32 device (L,) or None; mask float32 device (fh, fw) or None; a pixel counts
    when its three bytes and the twelve tap bytes lie in [lo, hi]. sums: an int64 device tensor of L x 7 to write into
    (default: new). Returns it as (L, 7): N, Sa_B, Sa_G, Sa_R, Sb_B, Sb_G, Sb_R (unsigned 64-bit values below 2^63)."""
    torch = _torch()
    n, fw, fh, L, la, lb = _exposure_sums_check(frames, link_a, link_b, stride, lo, hi)
    if H.numel() != 9 * L or (link_status is not None and link_status.numel() != L) or \
            (mask is not None and tuple(mask.shape) != (fh, fw)):
        raise NmError("mosaic exposure: H L x 9, link_status L values and mask (fh, fw) expected")
    if sums is None:
        sums = torch.empty((L, EXPOSURE_SUMS), dtype=torch.int64, device=frames[0].device)
    if sums.numel() != L * EXPOSURE_SUMS:
        raise NmError("mosaic exposure: sums must hold L x 7 values")
    _on_current_device(list(frames) + [H, sums, link_status, mask], "mosaic_exposure_sums")
    _check(lib().nm_mosaic_exposure_sums_dev(n, L, _pair_dev_table(frames, torch.uint8), la, lb, fw, fh,
                                             _opt(mask, torch.float32), _dev(H, torch.float32), _opt(link_status, torch.int32),
                                             int(stride), int(lo), int(hi), _dev(sums, torch.int64), _stream()),
           "nm_mosaic_exposure_sums_dev")
    return sums.view(L, EXPOSURE_SUMS)


def mosaic_exposure_sums_host(frames, link_a, link_b, H, link_status=None, mask=None, stride=4, lo=5, hi=250):
    """mosaic_exposure_sums on the host (nm_mosaic_exposure_sums_host, the same functions): numpy in and out, identical
    results. Returns uint64 (L, 7)."""
    import numpy as np
    frames = _pair_host_arrays(frames, np.uint8, flat=False)
    n, fw, fh, L, la, lb = _exposure_sums_check(frames, link_a, link_b, stride, lo, hi)
    H = np.ascontiguousarray(H, dtype=np.float32).reshape(-1)
    link_status = None if link_status is None else np.ascontiguousarray(link_status, dtype=np.int32).reshape(-1)
    mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.float32)
    if H.size != 9 * L or (link_status is not None and link_status.size != L) or (mask is not None and mask.shape != (fh, fw)):
        raise NmError("mosaic exposure: H L x 9, link_status L values and mask (fh, fw) expected")
    sums = np.zeros((L, EXPOSURE_SUMS), np.uint64)
    ptr = _pair_host_ptr
    _check(lib().nm_mosaic_exposure_sums_host(n, L, _pair_host_table(frames), la, lb, fw, fh, ptr(mask), ptr(H),
                                              ptr(link_status), int(stride), int(lo), int(hi), ptr(sums)),
           "nm_mosaic_exposure_sums_host")
    return sums


def mosaic_gains(n, link_a, link_b, sums, link_status=None, min_pixels=64, sigma_n=10.0, sigma_g=0.1, g_min=0.25, g_max=4.0,
                 mode=EXPOSURE_PER_CHANNEL, gains=None, stats=None):
    """Per-frame, per-channel gains of n frames from the links' overlap sums (nm_mosaic_gains_dev): one launch of one
    workgroup on the current stream, no host read. sums: int64 device (L, 7) of mosaic_exposure_sums; link_status int32 device
    (L,) or None; sigma_n in byte levels. gains / stats: float32 (n, 3) / float64 (9,) device tensors to write into (default:
    new). Returns (gains[n, 3] in B, G, R order, stats[9] in the order of EXPOSURE_STATS, its last entry one of
    EXPOSURE_END_*). gains goes to transform_blend_batch_gain as it is."""
    torch = _torch()
    L, la, lb = _exposure_gains_check(n, link_a, link_b, min_pixels, sigma_n, sigma_g, g_min, g_max, mode)
    if sums.numel() != L * EXPOSURE_SUMS or (link_status is not None and link_status.numel() != L):
        raise NmError("mosaic exposure: sums L x 7 and link_status L values expected")
    if gains is None:
        gains = torch.empty((n, 3), dtype=torch.float32, device=sums.device)
    if stats is None:
        stats = torch.empty(len(EXPOSURE_STATS), dtype=torch.float64, device=sums.device)
    if gains.numel() != 3 * n or stats.numel() != len(EXPOSURE_STATS):
        raise NmError("mosaic exposure: gains must hold n x 3 values and stats %d" % len(EXPOSURE_STATS))
    _on_current_device([sums, gains, stats, link_status], "mosaic_gains")
    _check(lib().nm_mosaic_gains_dev(n, L, la, lb, _dev(sums, torch.int64), _opt(link_status, torch.int32), int(min_pixels),
                                     float(sigma_n), float(sigma_g), float(g_min), float(g_max), int(mode),
                                     _dev(gains, torch.float32), _dev(stats, torch.float64), _stream()), "nm_mosaic_gains_dev")
    return gains.view(n, 3), stats


def mosaic_gains_host(n, link_a, link_b, sums, link_status=None, min_pixels=64, sigma_n=10.0, sigma_g=0.1, g_min=0.25,
                      g_max=4.0, mode=EXPOSURE_PER_CHANNEL):
    """mosaic_gains on the host (nm_mosaic_gains_host, the same functions in the same order): numpy in and out, bit-identical
    results."""
    import numpy as np
    L, la, lb = _exposure_gains_check(n, link_a, link_b, min_pixels, sigma_n, sigma_g, g_min, g_max, mode)
    sums = np.ascontiguousarray(sums).astype(np.uint64, copy=False).reshape(-1)
    link_status = None if link_status is None else np.ascontiguousarray(link_status, dtype=np.int32).reshape(-1)
    if sums.size != L * EXPOSURE_SUMS or (link_status is not None and link_status.size != L):
        raise NmError("mosaic exposure: sums L x 7 and link_status L values expected")
    gains = np.zeros((n, 3), np.float32)
    stats = np.zeros(len(EXPOSURE_STATS), np.float64)
    ptr = _pair_host_ptr
    _check(lib().nm_mosaic_gains_host(n, L, la, lb, ptr(sums), ptr(link_status), int(min_pixels), float(sigma_n),
                                      float(sigma_g), float(g_min), float(g_max), int(mode), ptr(gains), ptr(stats)),
           "nm_mosaic_gains_host")
    return gains, stats


def mosaic_exposure(frames, link_a, link_b, H, link_status=None, mask=None, stride=4, lo=5, hi=250, min_pixels=64,
                    sigma_n=10.0, sigma_g=0.1, g_min=0.25, g_max=4.0, mode=EXPOSURE_PER_CHANNEL, sums=None, gains=None,
                    stats=None):
    """Exposure gains of a mosaic's frames: mosaic_exposure_sums, then mosaic_gains, three launches on the current stream
    and no host read. Returns (gains, stats, sums), all device tensors."""
    _exposure_gains_check(len(frames), link_a, link_b, min_pixels, sigma_n, sigma_g, g_min, g_max, mode)
    sums = mosaic_exposure_sums(frames, link_a, link_b, H, link_status=link_status, mask=mask, stride=stride, lo=lo, hi=hi,
                                sums=sums)
    gains, stats = mosaic_gains(len(frames), link_a, link_b, sums, link_status=link_status, min_pixels=min_pixels,
                                sigma_n=sigma_n, sigma_g=sigma_g, g_min=g_min, g_max=g_max, mode=mode, gains=gains, stats=stats)
    return gains, stats, sums


BANDS_MAX_RADIUS, BANDS_STATS = 32, ("used", "skipped")
_BANDS_MAX_TILE_CAP = 1 << 30


class MosaicBandsWorkspace(_PairWorkspace):
    """Device scratch for nm_mosaic_bands_dev: n frames of tile_cap pixels into a cw x ch canvas."""
    _bytes_fn, _what, _shape_text = "nm_mosaic_bands_workspace_bytes", "mosaic bands workspace", "n=%d tile_cap=%d cw=%d ch=%d"

    def __init__(self, n, tile_cap, cw, ch, device):
        self._alloc(device, n=n, tile_cap=tile_cap, cw=cw, ch=ch)


def _bands_check(n, tile_cap, R=0, sigma=1.0):
    if not 0 < n <= MOSAIC_MAX_BATCH:
        raise NmError("mosaic bands: %d frames (1 .. %d)" % (n, MOSAIC_MAX_BATCH))
    if int(tile_cap) != tile_cap or not 1 <= tile_cap <= _BANDS_MAX_TILE_CAP:
        raise NmError("mosaic bands: tile_cap %r outside [1, 2^30]" % (tile_cap,))
    if int(R) != R or not 0 <= R <= BANDS_MAX_RADIUS:
        raise NmError("mosaic bands: radius %r outside [0, %d]" % (R, BANDS_MAX_RADIUS))
    if R > 0 and not (math.isfinite(sigma) and sigma > 0):
        raise NmError("mosaic bands: sigma %r must be finite and positive" % (sigma,))


def mosaic_bands_taps(R, sigma):
    """The low band's taps g[0..R] (float32 numpy) as nm_mosaic_bands_dev / _host compute them on the host."""
    import numpy as np
    _bands_check(1, 1, R, sigma)
    g = np.zeros(int(R) + 1, np.float32)
    _check(lib().nm_mosaic_bands_taps(int(R), float(sigma), g.ctypes.data), "nm_mosaic_bands_taps")
    return g


def mosaic_warp_tiles(frames, masks, wts, records, gains=None, tile_cap=None, tiles=None, stats=None):
    """Every placed frame's gained colour and weight on its own rectangle (nm_mosaic_warp_tiles): one launch on the current
    stream, no host read. frames, masks, wts, records, gains as transform_blend_batch_gain takes them. tile_cap: pixels per
    slot (default fh * fw * 2); a frame whose nw * nh exceeds it is skipped. tiles / stats: float32 (n, tile_cap, 4) / int32
    (2,) device tensors to write into (default: new, tiles uninitialised). Returns (tiles, stats): frame k's pixel (x, y) is
    tiles[k, y * nw_k + x] = (C_B, C_G, C_R, w); stats in the order of BANDS_STATS."""
    torch, what = _torch(), "mosaic_warp_tiles"
    n, fw, fh = _frames_check(what, frames)
    masks, wts, mfmt, wfmt = _scalar_planes(what, n, fw, fh, masks, wts)
    _records_check(what, records, n)
    if tile_cap is None:
        tile_cap = 2 * fh * fw
    _bands_check(n, tile_cap)
    if gains is not None and tuple(gains.shape) != (n, 3):
        raise NmError("mosaic_warp_tiles: gains must be float32 (n, 3)")
    device = frames[0].device
    if tiles is None:
        tiles = torch.empty((n, int(tile_cap), 4), dtype=torch.float32, device=device)
    if stats is None:
        stats = torch.empty(len(BANDS_STATS), dtype=torch.int32, device=device)
    if tiles.numel() != n * int(tile_cap) * 4 or stats.numel() != len(BANDS_STATS):
        raise NmError("mosaic_warp_tiles: tiles must hold n x tile_cap x 4 floats and stats %d ints" % len(BANDS_STATS))
    _on_current_device(list(frames) + masks + wts + [records, tiles, stats, gains], what)
    _check(lib().nm_mosaic_warp_tiles(n, _pair_dev_table(frames, torch.uint8), fw, fh, _pair_dev_table(masks, masks[0].dtype),
                                      mfmt, _pair_dev_table(wts, wts[0].dtype), wfmt, _dev(records, torch.int32),
                                      _opt(gains, torch.float32), _dev(tiles, torch.float32), int(tile_cap),
                                      _dev(stats, torch.int32), _stream()), what)
    return tiles.view(n, int(tile_cap), 4), stats


def mosaic_bands(canvas, canvas_wts, tiles, records, R=16, sigma=None, workspace=None):
    """Two-band composite of the tiles of mosaic_warp_tiles into the canvas IN PLACE (nm_mosaic_bands_dev): label, two blur
    passes and compose, four launches on the current stream whatever n is, no host read. canvas uint8 device (ch, cw, 4);
    canvas_wts float32 (ch, cw) or None; tiles float32 (n, tile_cap, 4); records int32 (n, 16); R in [0, 32], sigma default
    R / 2. A labelled pixel is overwritten, every other keeps its bytes and weight. Returns the workspace used."""
    torch = _torch()
    n, tile_cap, cw, ch = _composite_head("mosaic_bands", canvas, canvas_wts, tiles, records)
    sigma = (max(R, 1) / 2.0) if sigma is None else sigma
    _bands_check(n, tile_cap, R, sigma)
    device = _on_current_device([canvas, tiles, records, canvas_wts, workspace.buf if workspace is not None else None],
                                "mosaic_bands")
    workspace = _pair_workspace(MosaicBandsWorkspace, workspace, device, n, tile_cap, cw, ch)
    _check(lib().nm_mosaic_bands_dev(n, _dev(tiles, torch.float32), tile_cap, _dev(records, torch.int32),
                                     _dev(canvas, torch.uint8), cw, ch, _opt(canvas_wts, torch.float32), int(R), float(sigma),
                                     _dev(workspace.buf), _stream()), "nm_mosaic_bands_dev")
    return workspace


def mosaic_bands_host(canvas, canvas_wts, tiles, records, R=16, sigma=None):
    """mosaic_bands on the host (nm_mosaic_bands_host, the same functions): numpy arrays, canvas (ch, cw, 4) uint8 and
    canvas_wts (ch, cw) float32 or None written IN PLACE, bit-identical to the device."""
    import numpy as np
    n, tile_cap, cw, ch, tiles, records = _composite_head_host("mosaic_bands_host", canvas, canvas_wts, tiles, records)
    sigma = (max(R, 1) / 2.0) if sigma is None else sigma
    _bands_check(n, tile_cap, R, sigma)
    ws = _aligned_host(lib().nm_mosaic_bands_workspace_bytes(n, tile_cap, cw, ch), np)
    ptr = _pair_host_ptr
    _check(lib().nm_mosaic_bands_host(n, ptr(tiles), tile_cap, ptr(records), ptr(canvas), cw, ch, ptr(canvas_wts), int(R),
                                      float(sigma), ptr(ws)), "nm_mosaic_bands_host")


def mosaic_blend_bands(canvas, canvas_wts, frames, masks, wts, records, gains=None, R=16, sigma=None, tile_cap=None,
                       tiles=None, stats=None, workspace=None):
    """mosaic_warp_tiles, then mosaic_bands: five launches on the current stream, no host read. Returns (tiles, stats,
    workspace) for reuse in the next call."""
    tiles, stats = mosaic_warp_tiles(frames, masks, wts, records, gains=gains, tile_cap=tile_cap, tiles=tiles, stats=stats)
    workspace = mosaic_bands(canvas, canvas_wts, tiles, records, R=R, sigma=sigma, workspace=workspace)
    return tiles, stats, workspace


MEDIAN_SELECT, MEDIAN_MEAN = 0, 1
# The default inlier half-width, in units of the key (a luminance in [0, 1]). A parameter, not a result: chosen on the
# synthetic loop-closure views of tests/median_ref.py ("Median composite"), not on real footage.
MEDIAN_TAU = 0.05


def _median_check(n, tile_cap, mode, w_min, tau):
    _bands_check(n, tile_cap)
    if mode not in (MEDIAN_SELECT, MEDIAN_MEAN):
        raise NmError("mosaic median: unknown mode %r" % (mode,))
    if not (math.isfinite(w_min) and w_min >= 0):
        raise NmError("mosaic median: w_min %r must be finite and not negative" % (w_min,))
    if not tau >= 0:
        raise NmError("mosaic median: tau %r must not be negative or NaN" % (tau,))


def mosaic_median(canvas, canvas_wts, tiles, records, mode=MEDIAN_SELECT, w_min=0.0, tau=MEDIAN_TAU, support=None, label=None,
                  counts=None):
    """Median composite of the tiles of mosaic_warp_tiles into the canvas IN PLACE (nm_mosaic_median_dev): per canvas pixel
    the frame of lower-median key among the valid frames (w > w_min), either its own sample (MEDIAN_SELECT) or the weighted
    mean of the frames whose key lies within tau of its key (MEDIAN_MEAN). One launch on the current stream, plus one tiny
    zeroing launch when counts is given; no workspace, no host read. canvas uint8 device (ch, cw, 4); canvas_wts float32 (ch, cw) or
    None; tiles float32 (n, tile_cap, 4); records int32 (n, 16). Optional outputs: support / label uint8 (ch, cw) (the
    number of inliers / the median frame), counts int64 (n, 2) (pixels at which frame k is valid / valid but no inlier). A
    pixel with a valid frame is overwritten, every other keeps its contents. The default tau was chosen on synthetic views
    (MEDIAN_TAU); tune it on real footage. Returns counts."""
    torch = _torch()
    n, tile_cap, cw, ch = _composite_head("mosaic_median", canvas, canvas_wts, tiles, records)
    _median_check(n, tile_cap, mode, w_min, tau)
    if any(p is not None and tuple(p.shape) != (ch, cw) for p in (support, label)) or \
            (counts is not None and counts.numel() != 2 * n):
        raise NmError("mosaic_median: support and label must be uint8 (ch, cw) and counts int64 (n, 2)")
    _on_current_device([canvas, tiles, records, canvas_wts, support, label, counts], "mosaic_median")
    _check(lib().nm_mosaic_median_dev(n, _dev(tiles, torch.float32), tile_cap, _dev(records, torch.int32),
                                      _dev(canvas, torch.uint8), cw, ch, _opt(canvas_wts, torch.float32), int(mode),
                                      float(w_min), float(tau), _opt(support, torch.uint8), _opt(label, torch.uint8),
                                      _opt(counts, torch.int64), _stream()), "nm_mosaic_median_dev")
    return counts


def mosaic_median_host(canvas, canvas_wts, tiles, records, mode=MEDIAN_SELECT, w_min=0.0, tau=MEDIAN_TAU, support=None,
                       label=None, counts=None):
    """mosaic_median on the host (nm_mosaic_median_host, the same functions): numpy arrays written IN PLACE, canvas
    (ch, cw, 4) uint8, canvas_wts (ch, cw) float32 or None, support / label (ch, cw) uint8 or None, counts (n, 2) uint64 or
    None; bit-identical to the device."""
    import numpy as np
    n, tile_cap, cw, ch, tiles, records = _composite_head_host(
        "mosaic_median_host", canvas, canvas_wts, tiles, records, ((support, np.uint8), (label, np.uint8), (counts, np.uint64)))
    _median_check(n, tile_cap, mode, w_min, tau)
    if any(p is not None and p.shape != (ch, cw) for p in (support, label)) or (counts is not None and counts.size != 2 * n):
        raise NmError("mosaic_median_host: support and label must be (ch, cw) and counts (n, 2)")
    ptr = _pair_host_ptr
    _check(lib().nm_mosaic_median_host(n, ptr(tiles), tile_cap, ptr(records), ptr(canvas), cw, ch, ptr(canvas_wts), int(mode),
                                       float(w_min), float(tau), ptr(support), ptr(label), ptr(counts)), "nm_mosaic_median_host")


def mosaic_blend_median(canvas, canvas_wts, frames, masks, wts, records, gains=None, mode=MEDIAN_SELECT, w_min=0.0,
                        tau=MEDIAN_TAU, tile_cap=None, tiles=None, stats=None, support=None, label=None, counts=None):
    """mosaic_warp_tiles, then mosaic_median: two launches on the current stream (and one tiny zeroing launch when counts is given),
    no host read. Returns (tiles, stats) for reuse in the next call."""
    tiles, stats = mosaic_warp_tiles(frames, masks, wts, records, gains=gains, tile_cap=tile_cap, tiles=tiles, stats=stats)
    mosaic_median(canvas, canvas_wts, tiles, records, mode=mode, w_min=w_min, tau=tau, support=support, label=label,
                  counts=counts)
    return tiles, stats


LINK_PROPOSE_MAX_FRAMES = _PAIR_MAX_BATCH
LINK_PROPOSE_MAX_LINKS = MOSAIC_ADJUST_MAX_LINKS


class LinkVotesWorkspace(_PairWorkspace):
    """Device scratch of link_votes_dev for up to n frames of cap rows (one integer norm per row and frame)."""
    _bytes_fn, _what, _shape_text = "nm_link_votes_workspace_bytes", "link-votes workspace", "n %r / cap %r"

    def __init__(self, n, cap, device=None):
        self._alloc(device, n=n, cap=cap)


def link_votes_set_split(z=0):
    """Tuning: the number of parts the vote scan divides a wave's candidate frames into (nm_link_votes_set_split); 0 restores
    the default. Results do not depend on it. Returns the previous setting."""
    return lib().nm_link_votes_set_split(int(z))


def link_votes_dev(descs_u8, d_counts, ambiguity=0.8, votes=None, workspace=None, cap=None):
    """The u8 matcher's ratio test for all ordered pairs of n = len(descs_u8) <= LINK_PROPOSE_MAX_FRAMES frames, each pair
    reduced to a count (nm_link_votes_dev_u8): two launches on the current stream whatever n is, no host read. descs_u8 are
    uint8 device tensors (rows, 128) (out_u8 of desc_finish_batch_dev, out_desc_u8 of the selection), d_counts int32 DEVICE
    sizes. votes: an int32 device tensor of n x n entries to write into (default: new); every entry is written:
    votes[a, b] = rows of frame a that sift_match_u8_batch_dev would match into frame b, 0 on the diagonal. workspace: a
    LinkVotesWorkspace (default: new). Returns votes as (n, n)."""
    torch = _torch()
    n = _pair_count(descs_u8, d_counts)
    _pair_descriptors(descs_u8)
    cap = _pair_cap(cap, list(descs_u8))
    device = _pair_device(list(descs_u8) + list(d_counts) + [votes, workspace.buf if workspace is not None else None],
                          list(d_counts))
    if votes is None:
        votes = torch.empty((n, n), dtype=torch.int32, device=device)
    if votes.numel() != n * n:
        raise NmError("link votes: votes must hold n x n values")
    workspace = _pair_workspace(LinkVotesWorkspace, workspace, device, n, cap)
    arr = _pair_dev_table
    _check(lib().nm_link_votes_dev_u8(n, arr(descs_u8, torch.uint8), arr(d_counts, torch.int32), cap, float(ambiguity),
                                      _dev(votes, torch.int32), _dev(workspace.buf), _stream()), "nm_link_votes_dev_u8")
    return votes.view(n, n)


def link_votes_host(descs_u8, counts, ambiguity=0.8, cap=None):
    """link_votes_dev on the host (nm_link_votes_host_u8): numpy in and out, identical results. counts are host ints.
    Returns (n, n) int32."""
    import numpy as np
    n = _pair_count(descs_u8, counts)
    descs_u8 = _pair_host_arrays(descs_u8, np.uint8, flat=False)
    _pair_descriptors(descs_u8)
    cap = _pair_cap(cap, descs_u8)
    votes = np.empty((n, n), np.int32)
    arr = _pair_host_table
    _check(lib().nm_link_votes_host_u8(n, arr(descs_u8), arr(_pair_host_sizes(counts)), cap, float(ambiguity),
                                       _pair_host_ptr(votes)), "nm_link_votes_host_u8")
    return votes


def _link_rank_check(votes_shape, min_votes, min_gap, per_frame, max_links):
    n = votes_shape[0]
    if len(votes_shape) != 2 or votes_shape[1] != n or not 1 <= n <= LINK_PROPOSE_MAX_FRAMES:
        raise NmError("link ranking: votes must be (n, n) with n in [1, %d]" % LINK_PROPOSE_MAX_FRAMES)
    if any(int(v) != v for v in (min_votes, min_gap, per_frame, max_links)) or min_votes < 1 or min_gap < 1 or per_frame < 0 or \
            not 1 <= max_links <= LINK_PROPOSE_MAX_LINKS:
        raise NmError("link ranking: min_votes >= 1, min_gap >= 1, per_frame >= 0 and max_links in [1, %d] expected"
                      % LINK_PROPOSE_MAX_LINKS)
    return n


def link_rank_dev(votes, min_votes=16, min_gap=2, per_frame=0, max_links=LINK_PROPOSE_MAX_LINKS, links=None):
    """The vote matrix of link_votes_dev -> a ranked link list (nm_link_rank_dev): one launch on the current stream, no host
    read. score(a, b) = min(votes[a, b], votes[b, a]) for a < b; candidates have b - a >= min_gap and score >= min_votes, go
    by (score descending, a, b) and are accepted while fewer than max_links are and, for per_frame > 0, both frames have fewer
    than per_frame links. links: (link_a, link_b, link_score, d_links) int32 device tensors to write into (default: new).
    Returns them: the accepted links in acceptance order, -1 / -1 / 0 behind them, and the count in d_links[0]."""
    torch = _torch()
    n = _link_rank_check(tuple(votes.shape), min_votes, min_gap, per_frame, max_links)
    if links is None:
        links = tuple(torch.empty(max_links, dtype=torch.int32, device=votes.device) for _ in range(3)) + \
            (torch.empty(1, dtype=torch.int32, device=votes.device),)
    la, lb, ls, cnt = links
    if any(t.numel() < max_links for t in (la, lb, ls)) or cnt.numel() < 1:
        raise NmError("link ranking: the link lists hold max_links values and d_links one")
    _pair_device([votes, la, lb, ls, cnt], [])
    i32 = torch.int32
    _check(lib().nm_link_rank_dev(n, _dev(votes, i32), int(min_votes), int(min_gap), int(per_frame), int(max_links), _dev(la, i32),
                                  _dev(lb, i32), _dev(ls, i32), _dev(cnt, i32), _stream()), "nm_link_rank_dev")
    return la, lb, ls, cnt


def link_rank_host(votes, min_votes=16, min_gap=2, per_frame=0, max_links=LINK_PROPOSE_MAX_LINKS):
    """link_rank_dev on the host (nm_link_rank_host): numpy in and out, identical results. Returns (link_a, link_b,
    link_score, count) with count a Python int."""
    import numpy as np
    votes = np.ascontiguousarray(votes, dtype=np.int32)
    n = _link_rank_check(votes.shape, min_votes, min_gap, per_frame, max_links)
    la, lb, ls = (np.full(max_links, -9, np.int32) for _ in range(3))
    cnt = np.full(1, -9, np.int32)
    ptr = _pair_host_ptr
    _check(lib().nm_link_rank_host(n, ptr(votes), int(min_votes), int(min_gap), int(per_frame), int(max_links), ptr(la), ptr(lb),
                                   ptr(ls), ptr(cnt)), "nm_link_rank_host")
    return la, lb, ls, int(cnt[0])


def link_propose(descs_u8, d_counts, ambiguity=0.8, min_votes=16, min_gap=2, per_frame=0, max_links=LINK_PROPOSE_MAX_LINKS,
                 cap=None, votes=None, links=None, workspace=None):
    """Which frame pairs of a sequence to link: link_votes_dev, then link_rank_dev, three launches on the current stream and
    no host read. Returns (link_a, link_b, link_score, d_links, votes), all device tensors. The pair tables of the stages
    that follow are host tables, so the caller reads d_links and the lists once."""
    votes = link_votes_dev(descs_u8, d_counts, ambiguity=ambiguity, votes=votes, workspace=workspace, cap=cap)
    la, lb, ls, cnt = link_rank_dev(votes, min_votes=min_votes, min_gap=min_gap, per_frame=per_frame, max_links=max_links,
                                    links=links)
    return la, lb, ls, cnt, votes


INGEST_MAX_BATCH = _FRAMES_MAX_BATCH


def _ingest_map(u, v, what):
    torch = _torch()
    if u.dim() != 2 or tuple(v.shape) != tuple(u.shape) or u.dtype != torch.float32 or v.dtype != torch.float32:
        raise NmError("%s: the map must be two float32 (rows, cols) planes of one shape" % what)
    rows, cols = u.shape
    _size_check(what, "map", cols, rows)
    return cols, rows


def resample_map_u8x4(tex, x, y):
    """resample_2D<uchar4> on a caller's map (nm_resample_map_u8x4): tex uint8 (fh, fw, 4) BGRA sampled at (x + 0.5,
    y + 0.5) of the float32 (rows, cols) planes x, y. Returns uint8 (rows, cols, 4)."""
    torch = _torch()
    _, fw, fh = _frames_check("resample_map_u8x4", [tex])
    cols, rows = _ingest_map(x, y, "resample_map_u8x4")
    device = _on_current_device([tex, x, y], "resample_map_u8x4")
    out = torch.empty((rows, cols, 4), dtype=torch.uint8, device=device)
    _check(lib().nm_resample_map_u8x4(_dev(out), _dev(tex, torch.uint8), fw, fh, _dev(x, torch.float32),
                                      _dev(y, torch.float32), cols, rows, _stream()), "nm_resample_map_u8x4")
    return out


def ingest_batch(frames, u=None, v=None, undistorted=False):
    """n = len(frames) <= INGEST_MAX_BATCH BGRA frames (uint8 (fh, fw, 4), one camera) in ONE launch
    (nm_frame_ingest_batch_f32). With a map (u, v: float32 (rows, cols), e.g. from undistort_map) each frame is resampled
    as resample_map_u8x4(frame, u, v) and its gray plane is grayscale() of that uchar4 result; without one (identity mode)
    gray[k] = grayscale(frames[k]). Returns the list of float32 gray planes, and with undistorted=True (a map is needed)
    also the list of uint8 (rows, cols, 4) undistorted frames."""
    torch = _torch()
    frames = list(frames)
    n, fw, fh = _frames_check("ingest_batch", frames)
    if (u is None) != (v is None):
        raise NmError("ingest_batch: give both map planes or neither")
    if u is None:
        if undistorted:
            raise NmError("ingest_batch: undistorted frames need a map")
    cols, rows = (fw, fh) if u is None else _ingest_map(u, v, "ingest_batch")
    device = _on_current_device(frames + [u, v], "ingest_batch")
    gray = [torch.empty((rows, cols), dtype=torch.float32, device=device) for _ in range(n)]
    und = [torch.empty((rows, cols, 4), dtype=torch.uint8, device=device) for _ in range(n)] if undistorted else None
    _check(lib().nm_frame_ingest_batch_f32(n, _pair_dev_table(frames, torch.uint8), fw, fh, _opt(u, torch.float32),
                                           _opt(v, torch.float32), cols, rows, _pair_dev_table(gray, torch.float32),
                                           _pair_dev_table(und, torch.uint8), _stream()), "nm_frame_ingest_batch_f32")
    return (gray, und) if undistorted else gray


FRAME_WEIGHTS_MAX_BATCH, FRAME_WEIGHTS_MAX_RADIUS = 64, 64
FRAME_WEIGHTS_KINDS = ("mask", "wts", "dist2")


class FrameWeightsWorkspace(_PairWorkspace):
    """Device scratch for nm_frame_weights_batch_dev: n frames of fw x fh (one byte per pixel, rows padded to 64)."""
    _bytes_fn, _what, _shape_text = "nm_frame_weights_workspace_bytes", "frame-weights workspace", "n=%d fw=%d fh=%d"

    def __init__(self, n, fw, fh, device):
        self._alloc(device, n=n, fw=fw, fh=fh)


def _frame_weights_check(lo, hi, R, margin, min_count, mask_format, want, counts):
    if any(int(v) != v for v in (lo, hi, R, margin, min_count)):
        raise NmError("frame weights: lo, hi, R, margin and min_count are integers")
    if not (0 <= lo <= 255 and 0 <= hi <= 255):
        raise NmError("frame weights: lo %r and hi %r must lie in [0, 255]" % (lo, hi))
    if not 1 <= min_count <= 9:
        raise NmError("frame weights: min_count %r outside [1, 9]" % (min_count,))
    if not 1 <= R <= FRAME_WEIGHTS_MAX_RADIUS:
        raise NmError("frame weights: radius %r outside [1, %d]" % (R, FRAME_WEIGHTS_MAX_RADIUS))
    if not 0 <= margin < R:
        raise NmError("frame weights: margin %r outside [0, R)" % (margin,))
    if mask_format not in (TEX_U8N, TEX_F32):
        raise NmError("frame weights: mask_format must be TEX_U8N or TEX_F32")
    want = tuple(want)
    if any(w not in FRAME_WEIGHTS_KINDS for w in want) or len(set(want)) != len(want):
        raise NmError("frame weights: want holds each of %r at most once" % (FRAME_WEIGHTS_KINDS,))
    if not want and not counts:
        raise NmError("frame weights: no output requested")
    return want


def frame_weights_batch(frames, lo=0, hi=255, R=32, margin=0, min_count=1, border=True, base=None, mask_format=TEX_U8N,
                        want=("mask", "wts"), counts=False, workspace=None):
    """Per-frame validity masks and feather weights of n = len(frames) <= FRAME_WEIGHTS_MAX_BATCH BGRA frames (uint8 device
    (fh, fw, 4)) on the device (nm_frame_weights_batch_dev): two launches on the current stream whatever n is, plus one tiny
    zeroing launch with counts=True; no host read. A pixel is a seed when base (optional uint8 (fh, fw) plane shared by all
    frames) is 0 there, or when max(B, G, R) < lo or > hi there and in at least min_count pixels of its 3 x 3 window; D is
    the squared distance to the nearest seed (with border: or lattice point outside the frame), clipped to R * R; a pixel
    is valid when D > margin^2; mask = 255 / 1.0 where valid (mask_format TEX_U8N / TEX_F32), wts = (sqrt(D) - margin) /
    (R - margin) where valid, else 0. want: which of "mask", "wts", "dist2" to compute. Returns the requested tensors in the
    order of want, each ONE (n, fh, fw) allocation (mask uint8 or float32, wts float32, dist2 int16: the values are at most
    4096, so the signed view holds them as they are), followed by the int64 (n, 2) counts (seeds, valid pixels) when
    counts=True; a single result comes back bare. out[k] of a returned tensor goes straight into transform_blend_batch,
    mosaic_warp_tiles and mosaic_blend_median. workspace: a FrameWeightsWorkspace (default: new)."""
    torch = _torch()
    frames = list(frames)
    n, fw, fh = _frames_check("frame_weights_batch", frames)
    want = _frame_weights_check(lo, hi, R, margin, min_count, mask_format, want, counts)
    if base is not None and (tuple(base.shape) != (fh, fw) or base.dtype != torch.uint8):
        raise NmError("frame_weights_batch: base must be uint8 (fh, fw)")
    device = _on_current_device(frames + [base, workspace.buf if workspace is not None else None], "frame_weights_batch")
    workspace = _pair_workspace(FrameWeightsWorkspace, workspace, device, n, fw, fh)
    dtypes = {"mask": torch.uint8 if mask_format == TEX_U8N else torch.float32, "wts": torch.float32, "dist2": torch.int16}
    out = {w: torch.empty((n, fh, fw), dtype=dtypes[w], device=device) for w in want}
    cnt = torch.empty((n, 2), dtype=torch.int64, device=device) if counts else None
    table = lambda w: _pair_dev_table(list(out[w]), dtypes[w]) if w in out else None
    _check(lib().nm_frame_weights_batch_dev(n, _pair_dev_table(frames, torch.uint8), fw, fh, _opt(base, torch.uint8), int(lo),
                                            int(hi), int(min_count), 1 if border else 0, int(R), int(margin), table("mask"),
                                            int(mask_format), table("wts"), table("dist2"), _opt(cnt, torch.int64),
                                            _dev(workspace.buf), _stream()), "nm_frame_weights_batch_dev")
    res = tuple(out[w] for w in want) + ((cnt,) if counts else ())
    return res[0] if len(res) == 1 else res


def frame_weights_host(frames, lo=0, hi=255, R=32, margin=0, min_count=1, border=True, base=None, mask_format=TEX_U8N,
                       want=("mask", "wts"), counts=False):
    """frame_weights_batch on the host (nm_frame_weights_host, the same functions): frames are numpy uint8 (fh, fw, 4) arrays,
    base a uint8 (fh, fw) array or None. Returns numpy arrays in the same order: mask uint8 or float32, wts float32, dist2
    uint16, each (n, fh, fw), and counts uint64 (n, 2); bit-identical to the device."""
    import numpy as np
    frames = _pair_host_arrays(frames, np.uint8, flat=False)
    n, fw, fh = _frames_check("frame_weights_host", frames)
    want = _frame_weights_check(lo, hi, R, margin, min_count, mask_format, want, counts)
    if base is not None:
        base = np.ascontiguousarray(base, dtype=np.uint8)
        if base.shape != (fh, fw):
            raise NmError("frame_weights_host: base must be uint8 (fh, fw)")
    dtypes = {"mask": np.uint8 if mask_format == TEX_U8N else np.float32, "wts": np.float32, "dist2": np.uint16}
    out = {w: np.empty((n, fh, fw), dtypes[w]) for w in want}
    cnt = np.empty((n, 2), np.uint64) if counts else None
    table = lambda w: _pair_host_table(list(out[w])) if w in out else None
    _check(lib().nm_frame_weights_host(n, _pair_host_table(frames), fw, fh, _pair_host_ptr(base), int(lo), int(hi),
                                       int(min_count), 1 if border else 0, int(R), int(margin), table("mask"),
                                       int(mask_format), table("wts"), table("dist2"), _pair_host_ptr(cnt)),
           "nm_frame_weights_host")
    res = tuple(out[w] for w in want) + ((cnt,) if counts else ())
    return res[0] if len(res) == 1 else res


def frame_weights_set_grid_cap(cap=0):
    """Tuning and tests: the most workgroups either pass of frame_weights_batch launches (nm_frame_weights_set_grid_cap); 0
    restores the default. Results do not depend on it. Returns the previous setting."""
    return lib().nm_frame_weights_set_grid_cap(int(cap))


FRAME_QUALITY_MAX_BATCH, FRAME_QUALITY_MAX_GRID = 64, 8
KEYFRAME_STATUS, KEYFRAME_FEW, KEYFRAME_BAD, KEYFRAME_BLURRED, KEYFRAME_KEY, KEYFRAME_JUMP = 1, 2, 4, 8, 16, 32
KeyframePick = collections.namedtuple("KeyframePick", "keys key_count key_status flags scores H_keys H_status")


def _frame_quality_check(what, n, fw, fh, masks, lo, hi, grid, stats):
    """masks as a list of n planes (or None) with their format, and (gx, gy); shapes and dtypes only, torch or numpy."""
    if any(int(v) != v for v in (lo, hi)) or not (0 <= lo <= 255 and 0 <= hi <= 255):
        raise NmError("%s: lo %r and hi %r must be integers in [0, 255]" % (what, lo, hi))
    gx, gy = grid
    if int(gx) != gx or int(gy) != gy or not (1 <= gx <= min(FRAME_QUALITY_MAX_GRID, fw) and 1 <= gy <= min(FRAME_QUALITY_MAX_GRID, fh)):
        raise NmError("%s: grid %r outside [1, min(%d, fw)] x [1, min(%d, fh)]" % (what, grid, FRAME_QUALITY_MAX_GRID,
                                                                                  FRAME_QUALITY_MAX_GRID))
    mfmt = TEX_U8N
    if masks is not None:
        masks = list(masks) if isinstance(masks, (list, tuple)) else [masks] * n
        if len(masks) != n or any(tuple(m.shape) != (fh, fw) for m in masks):
            raise NmError("%s: masks must be %d (fh, fw) planes" % (what, n))
        kinds = {("uint8" if _is_dtype(m, "uint8") else "float32" if _is_dtype(m, "float32") else None) for m in masks}
        if len(kinds) != 1 or None in kinds:
            raise NmError("%s: masks must all be uint8 or all float32" % what)
        mfmt = TEX_U8N if "uint8" in kinds else TEX_F32
    if stats is not None and (tuple(stats.shape) != (n, int(gy), int(gx), 8) or
                              not (_is_dtype(stats, "int64") or _is_dtype(stats, "uint64"))):
        raise NmError("%s: stats must be 64-bit integers of shape (n, gy, gx, 8)" % what)
    return masks, mfmt, int(gx), int(gy)


def frame_quality_batch(frames, masks=None, lo=0, hi=255, grid=(4, 4), stats=None):
    """Exact quality statistics of n = len(frames) <= FRAME_QUALITY_MAX_BATCH BGRA frames (uint8 device (fh, fw, 4)) per cell
    of a grid = (gx, gy) <= (8, 8) (nm_frame_quality_batch_dev): two launches on the current stream whatever n is, no host
    read. masks: None, one (fh, fw) plane for all frames or a list of n, uint8 (valid: >= 128) or float32 (> 0.5). A pixel
    is dark when max(B, G, R) < lo and bright when > hi (the defaults 0 and 255 turn both off); it is measured when it and
    its four edge neighbours are eligible and neither. Returns stats, int64 (n, gy, gx, 8) (given or new; zeroed by the
    call): measured pixels, sum of Y, of Y^2, of the squared Laplacian, of the squared gradient, dark, bright and eligible
    pixels, with Y = (7 B + 72 G + 21 R + 50) // 100. stats goes straight into keyframe_pick."""
    torch = _torch()
    frames = list(frames)
    n, fw, fh = _frames_check("frame_quality_batch", frames)
    masks, mfmt, gx, gy = _frame_quality_check("frame_quality_batch", n, fw, fh, masks, lo, hi, grid, stats)
    if masks is not None:
        masks, _, mfmt, _ = _scalar_planes("frame_quality_batch", n, fw, fh, masks, masks)
    device = _on_current_device(frames + (masks or []) + [stats], "frame_quality_batch")
    if stats is None:
        stats = torch.empty((n, gy, gx, 8), dtype=torch.int64, device=device)
    _check(lib().nm_frame_quality_batch_dev(n, _pair_dev_table(frames, torch.uint8), fw, fh,
                                            _pair_dev_table(masks, masks[0].dtype if masks else None), mfmt, int(lo), int(hi),
                                            gx, gy, _dev(stats, torch.int64), _stream()), "nm_frame_quality_batch_dev")
    return stats


def frame_quality_host(frames, masks=None, lo=0, hi=255, grid=(4, 4), stats=None):
    """frame_quality_batch on the host (nm_frame_quality_host, the same functions): numpy frames and masks; returns (or
    fills) uint64 (n, gy, gx, 8), identical to the device's."""
    import numpy as np
    frames = _pair_host_arrays(frames, np.uint8, flat=False)
    n, fw, fh = _frames_check("frame_quality_host", frames)
    if masks is not None:
        masks = [np.asarray(m) for m in (masks if isinstance(masks, (list, tuple)) else [masks] * n)]
    masks, mfmt, gx, gy = _frame_quality_check("frame_quality_host", n, fw, fh, masks, lo, hi, grid, stats)
    if masks is not None:
        masks = [np.ascontiguousarray(m) for m in masks]
    if stats is None:
        stats = np.empty((n, gy, gx, 8), np.uint64)
    if not stats.flags["C_CONTIGUOUS"]:
        raise NmError("frame_quality_host: stats must be contiguous")
    _check(lib().nm_frame_quality_host(n, _pair_host_table(frames), fw, fh, _pair_host_table(masks), mfmt, int(lo), int(hi),
                                       gx, gy, _pair_host_ptr(stats)), "nm_frame_quality_host")
    return stats


def frame_quality_set_grid_cap(cap=0):
    """Tuning and tests: the most workgroups frame_quality_batch's walk launches (nm_frame_quality_set_grid_cap); 0 restores
    the default. Results do not depend on it. Returns the previous setting."""
    return lib().nm_frame_quality_set_grid_cap(int(cap))


def _keyframe_check(what, stats, chain, fw, fh, keep, frame_status, cell_min, min_pixels, max_bad, rel, w, d_min, d_max):
    import math
    if len(stats.shape) != 4 or stats.shape[3] != 8 or not (_is_dtype(stats, "int64") or _is_dtype(stats, "uint64")):
        raise NmError("%s: stats must be 64-bit integers of shape (n, gy, gx, 8)" % what)
    n, gy, gx = (int(v) for v in stats.shape[:3])
    if not (1 <= n <= FRAME_QUALITY_MAX_BATCH and 1 <= gx <= FRAME_QUALITY_MAX_GRID and 1 <= gy <= FRAME_QUALITY_MAX_GRID):
        raise NmError("%s: %d frames on a %d x %d grid (1 .. %d frames, 1 .. %d cells a side)"
                      % (what, n, gx, gy, FRAME_QUALITY_MAX_BATCH, FRAME_QUALITY_MAX_GRID))
    _size_check(what, "frame", fw, fh)
    if any(int(v) != v for v in (keep, w, cell_min, min_pixels)) or not (1 <= keep <= FRAME_QUALITY_MAX_BATCH and 0 <= w <= 8):
        raise NmError("%s: keep %r outside [1, %d] or w %r outside [0, 8]" % (what, keep, FRAME_QUALITY_MAX_BATCH, w))
    if not (1 <= cell_min < 1 << 62 and 0 <= min_pixels < 1 << 62):
        raise NmError("%s: cell_min %r must be >= 1 and min_pixels %r >= 0" % (what, cell_min, min_pixels))
    if not (0.0 <= max_bad <= 1.0 and 0.0 <= rel <= 1.0):
        raise NmError("%s: max_bad %r and rel %r must lie in [0, 1]" % (what, max_bad, rel))
    if not (math.isfinite(d_min) and math.isfinite(d_max) and 0.0 <= d_min <= d_max and d_max <= 3.0e38):
        raise NmError("%s: 0 <= d_min %r <= d_max %r, both finite" % (what, d_min, d_max))
    if _numel(chain) != 9 * n or not _is_dtype(chain, "float32"):
        raise NmError("%s: chain must hold n x 9 float32" % what)
    if frame_status is not None and (_numel(frame_status) != n or not _is_dtype(frame_status, "int32")):
        raise NmError("%s: frame_status must hold n int32" % what)
    return n, gx, gy


def _numel(a):
    v = 1
    for d in a.shape:
        v *= int(d)
    return v


def keyframe_pick(stats, chain, fw, fh, keep, frame_status=None, cell_min=64, min_pixels=1024, max_bad=0.25, rel=0.6, w=2,
                  d_min=32.0, d_max=128.0, carry=False):
    """Which of the n frames behind stats (frame_quality_batch's, int64 device (n, gy, gx, 8)) to keep, on the device
    (nm_keyframe_pick_dev): one launch of one workgroup on the current stream, no host read. chain: float32 device (n, 9)
    or (n, 3, 3), row k mapping mosaic coordinates to frame-k pixels (mosaic_plan's or mosaic_adjust's chain);
    frame_status: int32 device (n,) or None. A cell qualifies with >= cell_min measured pixels; a frame's score is the lower
    median of its qualifying cells' mean squared Laplacian; it is usable with status 1, a finite non-zero chain row, a
    qualifying cell, >= min_pixels measured pixels and (dark + bright) <= max_bad * eligible, and unless its score is below
    rel times the best usable score within w frames (blurred). The walk keeps the sharpest usable frame each time the
    view's corners have moved between d_min and d_max pixels since the last keyframe, at most keep of them; carry=True makes
    frame 0 the first keyframe whatever its flags (the last keyframe of the previous chunk of a long video). Returns
    KeyframePick(keys int32 (keep,) ascending with -1 beyond the count, key_count int32 (2,) = count and truncated,
    key_status int32 (keep,), flags int32 (n,) of KEYFRAME_* bits, scores float64 (n, 4) = score, mean Y, bad fraction and
    ref, H_keys float32 (keep - 1, 9) and H_status int32 (keep - 1,): keyframe i -> keyframe i + 1, for mosaic_plan and the
    link stages on the frames that slots_gather compacts by keys)."""
    torch = _torch()
    n, gx, gy = _keyframe_check("keyframe_pick", stats, chain, fw, fh, keep, frame_status, cell_min, min_pixels, max_bad, rel, w,
                                d_min, d_max)
    device = _on_current_device([stats, chain, frame_status], "keyframe_pick")
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=device)
    out = KeyframePick(i32(keep), i32(2), i32(keep), i32(n), torch.empty((n, 4), dtype=torch.float64, device=device),
                       torch.empty((keep - 1, 9), dtype=torch.float32, device=device), i32(keep - 1))
    _check(lib().nm_keyframe_pick_dev(n, _dev(stats, torch.int64), gx, gy, _dev(chain, torch.float32),
                                      _opt(frame_status, torch.int32), fw, fh, int(keep), int(cell_min), int(min_pixels),
                                      float(max_bad), float(rel), int(w), float(d_min), float(d_max), 1 if carry else 0,
                                      *[_dev(t) for t in out], _stream()), "nm_keyframe_pick_dev")
    return out


def keyframe_pick_host(stats, chain, fw, fh, keep, frame_status=None, cell_min=64, min_pixels=1024, max_bad=0.25, rel=0.6, w=2,
                       d_min=32.0, d_max=128.0, carry=False):
    """keyframe_pick on the host (nm_keyframe_pick_host, the same functions): numpy in and out, identical results."""
    import numpy as np
    stats, chain = np.asarray(stats), np.ascontiguousarray(chain, dtype=np.float32)
    if frame_status is not None:
        frame_status = np.ascontiguousarray(frame_status, dtype=np.int32)
    n, gx, gy = _keyframe_check("keyframe_pick_host", stats, chain, fw, fh, keep, frame_status, cell_min, min_pixels, max_bad, rel,
                                w, d_min, d_max)
    stats = np.ascontiguousarray(stats)
    i32 = lambda *shape: np.empty(shape, np.int32)
    out = KeyframePick(i32(keep), i32(2), i32(keep), i32(n), np.empty((n, 4), np.float64), np.empty((keep - 1, 9), np.float32),
                       i32(keep - 1))
    ptr = _pair_host_ptr
    _check(lib().nm_keyframe_pick_host(n, ptr(stats), gx, gy, ptr(chain), ptr(frame_status), fw, fh, int(keep), int(cell_min),
                                       int(min_pixels), float(max_bad), float(rel), int(w), float(d_min), float(d_max),
                                       1 if carry else 0, *[ptr(a) for a in out]), "nm_keyframe_pick_host")
    return out


def _slots_gather_check(what, keys, src, dst, fill):
    """(n, keep, bytes per slot) of a gather: src and dst are lists of equally shaped, equally typed arrays."""
    src = list(src)
    n, keep = len(src), _numel(keys)
    if not (1 <= n <= FRAME_QUALITY_MAX_BATCH and 1 <= keep <= FRAME_QUALITY_MAX_BATCH) or not _is_dtype(keys, "int32"):
        raise NmError("%s: %d sources and %d int32 keys (1 .. %d each)" % (what, n, keep, FRAME_QUALITY_MAX_BATCH))
    if int(fill) != fill or not 0 <= fill <= 255:
        raise NmError("%s: fill %r is a byte" % (what, fill))
    shape, dtype = tuple(src[0].shape), src[0].dtype
    if any(tuple(t.shape) != shape or t.dtype != dtype for t in src):
        raise NmError("%s: sources of one shape and dtype expected" % what)
    if dst is not None:
        dst = list(dst)
        if len(dst) != keep or any(tuple(t.shape) != shape or t.dtype != dtype for t in dst):
            raise NmError("%s: dst must be %d arrays shaped and typed like the sources" % (what, keep))
    size = _numel(src[0]) * (src[0].element_size() if hasattr(src[0], "element_size") else src[0].itemsize)
    if not 1 <= size < 1 << 31:
        raise NmError("%s: %d bytes per slot outside [1, 2^31)" % (what, size))
    return src, dst, n, keep, size


def slots_gather(keys, src, dst=None, fill=0):
    """Compact any per-frame table by the device's choice (nm_slots_gather_dev), one launch on the current stream, no host
    read: dst[i] = src[keys[i]] where keys[i] (int32 device (keep,), keyframe_pick's) lies in [0, len(src)), else every byte
    of dst[i] is `fill`. src: a list of n <= 64 contiguous device tensors of one shape and dtype (BGRA frames, gray planes,
    masks, weights, descriptor or coordinate tables, single count words); entries may repeat. dst: keep such tensors that
    overlap nothing (default: the slices of one new (keep, ...) allocation). Returns dst as a list."""
    torch = _torch()
    src, dst, n, keep, size = _slots_gather_check("slots_gather", keys, src, dst, fill)
    device = _on_current_device([keys] + src + (dst or []), "slots_gather")
    if dst is None:
        dst = list(torch.empty((keep,) + tuple(src[0].shape), dtype=src[0].dtype, device=device))
    _check(lib().nm_slots_gather_dev(n, _pair_dev_table(src, src[0].dtype), keep, _pair_dev_table(dst, src[0].dtype),
                                     _dev(keys, torch.int32), size, int(fill), _stream()), "nm_slots_gather_dev")
    return dst


def slots_gather_host(keys, src, dst=None, fill=0):
    """slots_gather on the host (nm_slots_gather_host): numpy arrays; dst entries must be contiguous."""
    import numpy as np
    keys = np.ascontiguousarray(keys, dtype=np.int32)
    src = [np.ascontiguousarray(a) for a in src]
    src, dst, n, keep, size = _slots_gather_check("slots_gather_host", keys, src, dst, fill)
    if dst is None:
        dst = list(np.empty((keep,) + src[0].shape, src[0].dtype))
    if any(not a.flags["C_CONTIGUOUS"] for a in dst):
        raise NmError("slots_gather_host: dst entries must be contiguous")
    _check(lib().nm_slots_gather_host(n, _pair_host_table(src), keep, _pair_host_table(dst), _pair_host_ptr(keys), size,
                                      int(fill)), "nm_slots_gather_host")
    return dst


# ---- gray pyramid and pyramidal KLT point tracking (include/nm_abi.h, "Gray pyramid and point tracking") ----
KLT_MAX_BATCH, KLT_MAX_LEVELS, KLT_MAX_RADIUS, KLT_MAX_ITERATIONS = _PAIR_MAX_BATCH, 6, 7, 16
KLT_OK, KLT_ABSENT, KLT_START, KLT_BORDER, KLT_FLAT, KLT_STEP, KLT_RESIDUAL, KLT_FB = range(8)
KltTrack = collections.namedtuple("KltTrack", "dst_xs dst_ys matches count reason residual fb_error")


def gray_pyramid_floats(fw, fh, levels):
    """Floats of one frame's pyramid block (nm_gray_pyramid_floats); 0 for a shape the pyramid refuses."""
    return int(lib().nm_gray_pyramid_floats(int(fw), int(fh), int(levels)))


def gray_pyramid_offset(fw, fh, level):
    """Floats (bytes of the mask block) from a block's start to its level `level` (nm_gray_pyramid_offset)."""
    return int(lib().nm_gray_pyramid_offset(int(fw), int(fh), int(level)))


def gray_pyramid_level(block, fw, fh, level):
    """Level `level` of a pyramid or mask block as an (h_l, w_l) view; torch and numpy alike."""
    w, h = fw, fh
    for _ in range(level):
        w, h = (w + 1) >> 1, (h + 1) >> 1
    off = gray_pyramid_offset(fw, fh, level)
    return block.reshape(-1)[off:off + w * h].reshape(h, w)


def _pyramid_check(what, grays, levels, mask):
    n = len(grays)
    if not 0 < n <= KLT_MAX_BATCH:
        raise NmError("%s: %d frames (1 .. %d)" % (what, n, KLT_MAX_BATCH))
    fw, fh = _planes_check(what, list(grays), mask)
    _size_check(what, "frame", fw, fh)
    if any(not _is_dtype(g, "float32") for g in list(grays) + ([mask] if mask is not None else [])):
        raise NmError("%s: float32 planes expected" % what)
    if int(levels) != levels or not 1 <= levels <= KLT_MAX_LEVELS or gray_pyramid_floats(fw, fh, levels) == 0:
        raise NmError("%s: levels %r outside [1, %d] or too many for a %d x %d frame" % (what, levels, KLT_MAX_LEVELS, fw, fh))
    return n, fw, fh, gray_pyramid_floats(fw, fh, levels)


def gray_pyramid_batch(grays, levels=4, mask=None, pyrs=None, mask_pyr=None):
    """Gray pyramids of n = len(grays) <= KLT_MAX_BATCH float32 device planes of one (fh, fw) shape
    (nm_gray_pyramid_batch_f32): max(levels - 1, 1) launches on the current stream whatever n is, no host read. A frame's
    pyramid is one float32 tensor of gray_pyramid_floats(fw, fh, levels) values, level l at gray_pyramid_offset(fw, fh, l):
    level 0 is the plane itself, level l + 1 the (1 4 6 4 1) / 16 binomial filter of level l at its even pixels. mask: the
    link stages' float32 (fh, fw) plane (seen where > 0.5); its pyramid of bytes (1: every pixel below is seen) costs one
    more launch and serves every frame. Returns (pyrs, mask_pyr or None); both may be given to be filled."""
    torch = _torch()
    grays = list(grays)
    n, fw, fh, floats = _pyramid_check("gray_pyramid_batch", grays, levels, mask)
    device = _on_current_device(grays + [mask, mask_pyr] + list(pyrs or []), "gray_pyramid_batch")
    if pyrs is None:
        pyrs = [torch.empty(floats, dtype=torch.float32, device=device) for _ in range(n)]
    if len(pyrs) != n or any(p.numel() < floats for p in pyrs):
        raise NmError("gray_pyramid_batch: %d blocks of at least %d floats expected" % (n, floats))
    if mask is not None and mask_pyr is None:
        mask_pyr = torch.empty(floats, dtype=torch.uint8, device=device)
    if (mask is None) != (mask_pyr is None) or (mask_pyr is not None and mask_pyr.numel() < floats):
        raise NmError("gray_pyramid_batch: mask_pyr needs a mask and %d bytes" % floats)
    _check(lib().nm_gray_pyramid_batch_f32(n, _pair_dev_table(grays, torch.float32), fw, fh, int(levels),
                                           _pair_dev_table(list(pyrs), torch.float32), _opt(mask, torch.float32),
                                           _opt(mask_pyr, torch.uint8), _stream()), "nm_gray_pyramid_batch_f32")
    return list(pyrs), mask_pyr


def gray_pyramid_host(grays, levels=4, mask=None):
    """gray_pyramid_batch on the host (nm_gray_pyramid_host_f32, the same functions): numpy planes in, (list of float32
    blocks, uint8 mask block or None) out, identical bits."""
    import numpy as np
    grays = _pair_host_arrays(grays, np.float32, flat=False)
    mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.float32)
    n, fw, fh, floats = _pyramid_check("gray_pyramid_host", grays, levels, mask)
    pyrs = [np.zeros(floats, np.float32) for _ in range(n)]
    mask_pyr = None if mask is None else np.zeros(floats, np.uint8)
    _check(lib().nm_gray_pyramid_host_f32(n, _pair_host_table(grays), fw, fh, int(levels), _pair_host_table(pyrs),
                                          _pair_host_ptr(mask), _pair_host_ptr(mask_pyr)), "nm_gray_pyramid_host_f32")
    return pyrs, mask_pyr


def _klt_check(what, n, fw, fh, levels, floats_of, H, status, radius, iterations, eps, max_step, min_eig, max_residual, fb_max):
    """The tracker's host values; floats_of: the sizes of the pyramid blocks and, last, of the mask block or None."""
    _size_check(what, "frame", fw, fh)
    if int(levels) != levels or not 1 <= levels <= KLT_MAX_LEVELS or gray_pyramid_floats(fw, fh, levels) == 0:
        raise NmError("%s: levels %r outside [1, %d] or too many for a %d x %d frame" % (what, levels, KLT_MAX_LEVELS, fw, fh))
    if any(v is not None and v < gray_pyramid_floats(fw, fh, levels) for v in floats_of):
        raise NmError("%s: a pyramid or mask block is smaller than %d" % (what, gray_pyramid_floats(fw, fh, levels)))
    if int(radius) != radius or not 1 <= radius <= KLT_MAX_RADIUS or int(iterations) != iterations or \
            not 1 <= iterations <= KLT_MAX_ITERATIONS:
        raise NmError("%s: radius %r outside [1, %d] or iterations %r outside [1, %d]"
                      % (what, radius, KLT_MAX_RADIUS, iterations, KLT_MAX_ITERATIONS))
    if not all(math.isfinite(v) for v in (eps, max_step, min_eig, max_residual, fb_max)) or eps <= 0 or max_step <= 0 or \
            min_eig < 0 or max_residual < 0 or fb_max < 0:
        raise NmError("%s: eps and max_step must be > 0, min_eig, max_residual and fb_max >= 0, all finite" % what)
    if H is None and status is not None:
        raise NmError("%s: status needs H" % what)
    if H is not None:
        _pair_model_shape(n, _numel(H), None if status is None else _numel(status))


def klt_track_batch_dev(pyrAs, pyrBs, fw, fh, src_xs, src_ys, d_nAs, levels=4, radius=7, iterations=10, eps=2.0 ** -6,
                        max_step=16.0, min_eig=0.0, max_residual=0.0, fb_max=0.0, mask_pyr=None, H=None, status=None,
                        capA=None, want_reason=False, want_residual=False, want_fb_error=False, out=None):
    """Pyramidal Lucas-Kanade tracking of the points (src_xs[k], src_ys[k]) of n = len(pyrAs) <= KLT_MAX_BATCH frame pairs
    from pyramid block pyrAs[k] into pyrBs[k] (gray_pyramid_batch; nm_klt_track_batch_dev_f32): the zeroing launch and one
    launch per 32 pairs on the current stream, no host read. d_nAs are int32 DEVICE tensors; rows at and beyond
    min(*d_nA, capA), rows with src_x < 0 and rows that are lost get -1. H (n, 9) float32 with status (n,) int32: predicted
    maps A -> B as the start. min_eig: the smaller eigenvalue of the window's gradient matrix per tap, gray^2;
    max_residual: mean absolute difference in gray values, 0 turns it off; fb_max: forward-backward distance in pixels, 0
    turns the check off. Returns KltTrack(dst_xs, dst_ys, matches, count, reason, residual, fb_error): lists of n tensors of
    capA float32 / float32 / int32 that go into ransac_batch_dev as they stand, count int64 (n,), and the optional per-row
    uint8 KLT_* codes, residuals and forward-backward errors (None when not asked for). out: a KltTrack from an earlier
    call of the same shape to be filled again."""
    torch = _torch()
    n = _pair_count(pyrAs, pyrBs, src_xs, src_ys, d_nAs)
    _klt_check("klt_track_batch_dev", n, fw, fh, levels, [p.numel() for p in list(pyrAs) + list(pyrBs)] +
               [None if mask_pyr is None else mask_pyr.numel()], H, status, radius, iterations, eps, max_step, min_eig,
               max_residual, fb_max)
    capA = _pair_cap(capA, list(src_xs) + list(src_ys))
    device = _pair_device(list(pyrAs) + list(pyrBs) + list(src_xs) + list(src_ys) + list(d_nAs) + [mask_pyr, H, status], d_nAs)
    if out is None:
        new = lambda dt: [torch.empty(capA, dtype=dt, device=device) for _ in range(n)]
        out = KltTrack(new(torch.float32), new(torch.float32), new(torch.int32), torch.empty(n, dtype=torch.int64, device=device),
                       new(torch.uint8) if want_reason else None, new(torch.float32) if want_residual else None,
                       new(torch.float32) if want_fb_error else None)
    _pair_cap(capA, [t for ts in out[:3] + out[4:] if ts is not None for t in ts])
    if len(out.dst_xs) != n or out.count.numel() != n:
        raise NmError("klt_track_batch_dev: out is of another shape")
    f, i32, tab = torch.float32, torch.int32, _pair_dev_table
    _check(lib().nm_klt_track_batch_dev_f32(n, tab(list(pyrAs), f), tab(list(pyrBs), f), fw, fh, int(levels),
                                            _opt(mask_pyr, torch.uint8), tab(list(src_xs), f), tab(list(src_ys), f),
                                            tab(list(d_nAs), i32), capA, _opt(H, f), _opt(status, i32), int(radius),
                                            int(iterations), eps, max_step, min_eig, max_residual, fb_max, tab(out.dst_xs, f),
                                            tab(out.dst_ys, f), tab(out.matches, i32), _dev(out.count, torch.int64),
                                            tab(out.reason, torch.uint8), tab(out.residual, f), tab(out.fb_error, f),
                                            _stream()), "nm_klt_track_batch_dev_f32")
    return out


def klt_track_host(pyrAs, pyrBs, fw, fh, src_xs, src_ys, nAs, levels=4, radius=7, iterations=10, eps=2.0 ** -6, max_step=16.0,
                   min_eig=0.0, max_residual=0.0, fb_max=0.0, mask_pyr=None, H=None, status=None, capA=None):
    """klt_track_batch_dev on the host (nm_klt_track_host_f32, the same functions): numpy in and out, identical results;
    nAs are host ints. Returns a KltTrack of (n, capA) arrays with count uint64 and every optional output."""
    import numpy as np
    n = _pair_count(pyrAs, pyrBs, src_xs, src_ys, nAs)
    pyrAs, pyrBs, src_xs, src_ys = (_pair_host_arrays(vs, np.float32) for vs in (pyrAs, pyrBs, src_xs, src_ys))
    mask_pyr = None if mask_pyr is None else np.ascontiguousarray(mask_pyr, dtype=np.uint8).reshape(-1)
    if H is not None:
        H = np.ascontiguousarray(H, dtype=np.float32).reshape(-1)
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(-1)
    _klt_check("klt_track_host", n, fw, fh, levels, [p.size for p in pyrAs + pyrBs] + [None if mask_pyr is None else mask_pyr.size],
               H, status, radius, iterations, eps, max_step, min_eig, max_residual, fb_max)
    capA = _pair_cap(capA, src_xs + src_ys)
    nA = _pair_host_sizes(nAs)
    dst_x, dst_y, residual, fb = (np.zeros((n, capA), np.float32) for _ in range(4))
    matches, reason, count = np.zeros((n, capA), np.int32), np.zeros((n, capA), np.uint8), np.zeros(n, np.uint64)
    arr, ptr = _pair_host_table, _pair_host_ptr
    _check(lib().nm_klt_track_host_f32(n, arr(pyrAs), arr(pyrBs), fw, fh, int(levels), ptr(mask_pyr), arr(src_xs), arr(src_ys),
                                       arr(nA), capA, ptr(H), ptr(status), int(radius), int(iterations), eps, max_step, min_eig,
                                       max_residual, fb_max, arr(list(dst_x)), arr(list(dst_y)), arr(list(matches)), ptr(count),
                                       arr(list(reason)), arr(list(residual)), arr(list(fb))), "nm_klt_track_host_f32")
    return KltTrack(dst_x, dst_y, matches, count, reason, residual, fb)


def klt_sums_host(pyrA, pyrB, fw, fh, levels, level, radius, px, py, dx, dy, mask_pyr=None):
    """The integer sums of one evaluation of the tracker (nm_klt_sums_host, for tests): (Gxx, Gxy, Gyy, bx, by, sum |e|) as
    Python ints and the flags (1: template invalid, 2: the other window invalid)."""
    import numpy as np
    pyrA, pyrB = (np.ascontiguousarray(p, dtype=np.float32).reshape(-1) for p in (pyrA, pyrB))
    mask_pyr = None if mask_pyr is None else np.ascontiguousarray(mask_pyr, dtype=np.uint8).reshape(-1)
    sums, flags = np.zeros(6, np.int64), np.zeros(1, np.int32)
    _check(lib().nm_klt_sums_host(_pair_host_ptr(pyrA), _pair_host_ptr(pyrB), _pair_host_ptr(mask_pyr), fw, fh, int(levels),
                                  int(level), int(radius), float(px), float(py), float(dx), float(dy), _pair_host_ptr(sums),
                                  _pair_host_ptr(flags)), "nm_klt_sums_host")
    return tuple(int(v) for v in sums), int(flags[0])


def klt_set_grid_cap(cap=0):
    """Tuning and tests: the most workgroups a pyramid or tracker launch uses (nm_klt_set_grid_cap); 0 restores the default.
    Results do not depend on it. Returns the previous setting."""
    return lib().nm_klt_set_grid_cap(int(cap))


def klt_set_lanes(lanes=0):
    """Tuning and tests: the lanes of a wave that share a point in the tracker's kernel (nm_klt_set_lanes): 8, 16 or 32; 0
    restores the default (16). Results do not depend on it. Returns the previous setting."""
    return lib().nm_klt_set_lanes(int(lanes))


def klt_grid_points(fw, fh, step, mask=None):
    """A regular lattice as a point table, for frames without keypoints: the points (step // 2 + i step, step // 2 + j step)
    inside the frame, row by row, as two float32 numpy arrays (x, y). mask: an (fh, fw) array; points where it is <= 0.5
    are left out. Hand them to the device with torch.from_numpy(...).cuda()."""
    import numpy as np
    if int(step) != step or step < 1:
        raise NmError("klt_grid_points: step %r must be a whole number >= 1" % (step,))
    _size_check("klt_grid_points", "frame", fw, fh)
    ys, xs = np.meshgrid(np.arange(step // 2, fh, step), np.arange(step // 2, fw, step), indexing="ij")
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    if mask is not None:
        if tuple(mask.shape) != (fh, fw):
            raise NmError("klt_grid_points: mask must be (fh, fw)")
        keep = np.asarray(mask)[ys, xs] > 0.5
        xs, ys = xs[keep], ys[keep]
    return xs.astype(np.float32), ys.astype(np.float32)


KLT_CORNERS_MAX_NMS = 16


class KltCornersWorkspace(_PairWorkspace):
    """Device scratch for nm_klt_corners_batch_dev_f32: n frames of fw x fh (a score plane, the corner flag words and the
    held-point marks of every frame)."""
    _bytes_fn, _what, _shape_text = "nm_klt_corners_workspace_bytes", "KLT corners workspace", "n=%d fw=%d fh=%d"

    def __init__(self, n, fw, fh, device):
        self._alloc(device, n=n, fw=fw, fh=fh)


def klt_corners_workspace_bytes(n, fw, fh):
    """Bytes of the workspace of klt_corners_batch (nm_klt_corners_workspace_bytes); 0 for arguments out of range."""
    return int(lib().nm_klt_corners_workspace_bytes(int(n), int(fw), int(fh)))


def klt_corners_set_grid_cap(cap=0):
    """Tuning and tests: the most workgroups a launch of klt_corners_batch uses (nm_klt_corners_set_grid_cap); 0 restores the
    default. Results do not depend on it. Returns the previous setting."""
    return lib().nm_klt_corners_set_grid_cap(int(cap))


def _klt_corners_check(what, grays, radius, nms, min_eig, cap, mask, held):
    """(n, fw, fh, cap_held) of a corners call; shapes, dtypes and host values only, torch or numpy."""
    grays = list(grays)
    n = len(grays)
    if not 0 < n <= KLT_MAX_BATCH:
        raise NmError("%s: %d frames (1 .. %d)" % (what, n, KLT_MAX_BATCH))
    fw, fh = _planes_check(what, grays, mask)
    _size_check(what, "frame", fw, fh)
    if any(not _is_dtype(g, "float32") for g in grays) or (mask is not None and not _is_dtype(mask, "uint8")):
        raise NmError("%s: float32 planes and a uint8 mask expected" % what)
    if int(radius) != radius or not 1 <= radius <= KLT_MAX_RADIUS or int(nms) != nms or not 1 <= nms <= KLT_CORNERS_MAX_NMS:
        raise NmError("%s: radius %r outside [1, %d] or nms %r outside [1, %d]" % (what, radius, KLT_MAX_RADIUS, nms,
                                                                                   KLT_CORNERS_MAX_NMS))
    if not math.isfinite(min_eig) or min_eig < 0:
        raise NmError("%s: min_eig %r must be finite and >= 0" % (what, min_eig))
    if int(cap) != cap or not 1 <= cap < _PAIR_CAP_LIMIT:
        raise NmError("%s: cap %r outside [1, %d)" % (what, cap, _PAIR_CAP_LIMIT))
    cap_held = 0
    if held is not None:
        if len(held) != 3 or any(len(v) != n for v in held):
            raise NmError("%s: held is (xs, ys, counts), each a list of n" % what)
        cap_held = _pair_cap(None, list(held[0]) + list(held[1]))
    return n, fw, fh, cap_held


def klt_corners_batch(grays, radius=7, nms=8, min_eig=1.0, cap=4096, mask=None, held=None, want_score_plane=False, out=None,
                      workspace=None):
    """Shi-Tomasi corners of n = len(grays) <= KLT_MAX_BATCH float32 device planes of one (fh, fw) shape
    (nm_klt_corners_batch_dev_f32): three launches on the current stream whatever n is, four with held points, no host
    read. The score of a pixel is the tracker's own level-0 texture gate at that pixel (the smaller eigenvalue of the
    window's gradient matrix per tap, gray^2, for the same radius), so with the same radius, min_eig and mask
    klt_track_batch_dev calls no corner FLAT or BORDER at level 0. A corner is a scored pixel (score >= min_eig) that is the
    strongest within Chebyshev distance nms, the first in raster order among equals. mask: a uint8 (fh, fw) plane, 1 =
    seen (level 0 of a mask_pyr block: gray_pyramid_level(mask_pyr, fw, fh, 0)). held: (xs, ys, d_counts), lists of n float32
    / float32 / int32 DEVICE tensors, the points a caller already tracks in each frame (survivors of the last frame): no
    corner appears within nms of one. Returns a dict: "x", "y", "score" (lists of n float32 tensors of `cap` rows, the corners
    in raster order, rows at and beyond the count not written), "count" and "total" (int32 (n,) device: min(total, cap) and
    the total), "score_plane" (a list of n (fh, fw) planes, -1 where a pixel is not scored; None unless asked for). out: the
    dict a former call returned, to write into the same tensors (what a graph capture needs, with a workspace). The chain:
        c = klt_corners_batch(grays)
        s = sift_select_batch_dev([c["count"][k:k + 1] for k in range(n)], c["x"], c["y"], fw, fh, scores=c["score"], keep=512)
        t = klt_track_batch_dev(pyrAs, pyrBs, fw, fh, s["x"], s["y"], [s["count"][k:k + 1] for k in range(n)])
    workspace: a KltCornersWorkspace (default: new)."""
    torch = _torch()
    grays = list(grays)
    n, fw, fh, cap_held = _klt_corners_check("klt_corners_batch", grays, radius, nms, min_eig, cap, mask, held)
    held_all = [t for ts in held for t in ts] if held is not None else []
    device = _on_current_device(grays + held_all + [mask, workspace.buf if workspace is not None else None], "klt_corners_batch")
    workspace = _pair_workspace(KltCornersWorkspace, workspace, device, n, fw, fh)
    if out is None:
        new = lambda: [torch.zeros(cap, dtype=torch.float32, device=device) for _ in range(n)]
        out = dict(x=new(), y=new(), score=new(), count=torch.zeros(n, dtype=torch.int32, device=device),
                   total=torch.zeros(n, dtype=torch.int32, device=device),
                   score_plane=[torch.empty((fh, fw), dtype=torch.float32, device=device) for _ in range(n)]
                   if want_score_plane else None)
    if any(len(out[name]) != n for name in ("x", "y", "score")) or out["count"].numel() != n or out["total"].numel() != n or \
            (out["score_plane"] is not None and
             (len(out["score_plane"]) != n or any(tuple(p.shape) != (fh, fw) for p in out["score_plane"]))):
        raise NmError("klt_corners_batch: `out` does not fit this call")
    _pair_cap(cap, out["x"] + out["y"] + out["score"])
    f, i32, tab = torch.float32, torch.int32, _pair_dev_table
    hx, hy, hn = (tab(list(held[0]), f), tab(list(held[1]), f), tab(list(held[2]), i32)) if held is not None else (None,) * 3
    _check(lib().nm_klt_corners_batch_dev_f32(n, tab(grays, f), fw, fh, _opt(mask, torch.uint8), hx, hy, hn, cap_held,
                                              int(radius), int(nms), min_eig, int(cap), tab(out["x"], f), tab(out["y"], f),
                                              tab(out["score"], f), _dev(out["count"], i32), _dev(out["total"], i32),
                                              tab(out["score_plane"], f), _dev(workspace.buf), _stream()),
           "nm_klt_corners_batch_dev_f32")
    return out


def klt_corners_host(grays, radius=7, nms=8, min_eig=1.0, cap=4096, mask=None, held=None, want_score_plane=False, fill=0):
    """klt_corners_batch on the host (nm_klt_corners_host_f32, the same functions): numpy planes in, identical results.
    held: (xs, ys, counts) with host ints as counts. Returns the same dict with (n, cap) float32 arrays "x", "y", "score"
    (rows at and beyond a count hold `fill`), int32 (n,) "count" and "total", and "score_plane" (n, fh, fw) or None. The
    chain: klt_corners_host -> sift_select_host(scores=...) -> klt_track_host."""
    import numpy as np
    grays = _pair_host_arrays(grays, np.float32, flat=False)
    mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    if held is not None and len(held) == 3:
        held = (_pair_host_arrays(held[0], np.float32), _pair_host_arrays(held[1], np.float32), list(held[2]))
    n, fw, fh, cap_held = _klt_corners_check("klt_corners_host", grays, radius, nms, min_eig, cap, mask, held)
    x, y, score = (np.full((n, cap), fill, np.float32) for _ in range(3))
    count, total = np.zeros(n, np.int32), np.zeros(n, np.int32)
    plane = np.zeros((n, fh, fw), np.float32) if want_score_plane else None
    arr, ptr = _pair_host_table, _pair_host_ptr
    sizes = _pair_host_sizes(held[2]) if held is not None else None           # alive until the call returns
    hx, hy, hn = (arr(held[0]), arr(held[1]), arr(sizes)) if held is not None else (None,) * 3
    _check(lib().nm_klt_corners_host_f32(n, arr(grays), fw, fh, ptr(mask), hx, hy, hn, cap_held, int(radius), int(nms), min_eig,
                                         int(cap), arr(list(x)), arr(list(y)), arr(list(score)), ptr(count), ptr(total),
                                         None if plane is None else arr(list(plane))), "nm_klt_corners_host_f32")
    return dict(x=x, y=y, score=score, count=count, total=total, score_plane=plane)


SIFT_MAX_BATCH = 64


def detect_describe_batch(arenas, grays):
    """Enqueue len(arenas) <= SIFT_MAX_BATCH equally sized frames as ONE launch sequence on the current stream
    (nm_sift_detect_describe_batch); outputs land in each arena's own tensors, exactly as detect_describe would."""
    torch = _torch()
    n = len(arenas)
    if n != len(grays) or not 0 < n <= SIFT_MAX_BATCH:
        raise NmError("batch of %d arenas / %d frames (max %d)" % (n, len(grays), SIFT_MAX_BATCH))
    for a, g in zip(arenas, grays):
        if tuple(g.shape) != (a.height, a.width):
            raise NmError("frame shape %s does not match the arena (%d,%d)" % (tuple(g.shape), a.height, a.width))
        if g.device != a.device or torch.cuda.current_device() != a.device.index:
            raise NmError("arena lives on %s: frame on %s, current device %d" % (a.device, g.device,
                                                                                torch.cuda.current_device()))

    def arr(vals):
        return (C.c_void_p * n)(*vals)
    _check(lib().nm_sift_detect_describe_batch(
        arr([a._h.value for a in arenas]), n, arr([_dev(g, torch.float32) for g in grays]),
        arr([_dev(a.desc) for a in arenas]), arr([_dev(a.x) for a in arenas]), arr([_dev(a.y) for a in arenas]),
        arr([_dev(a.kpts) for a in arenas]), arr([_dev(a.orients) for a in arenas]),
        arr([_dev(a.num_items) for a in arenas]), _stream()), "nm_sift_detect_describe_batch")


def scale_space_batch(arenas, grays, write_dog=True, write_grad=True):
    """Only the scale-space launches (nm_sift_scale_space_batch_ex), on the current stream. write_dog=True: levels + DoG +
    gradient planes; False: what detect_describe_batch runs (no DoG planes). write_grad=False leaves the fused gradient
    planes out: with write_dog=True that is exactly the reference's convolve + compute_dog work (108 B per octave-pixel)."""
    torch = _torch()
    n = len(arenas)
    if n != len(grays) or not 0 < n <= SIFT_MAX_BATCH:
        raise NmError("batch of %d arenas / %d frames (max %d)" % (n, len(grays), SIFT_MAX_BATCH))
    _check(lib().nm_sift_scale_space_batch_ex((C.c_void_p * n)(*[a._h.value for a in arenas]), n,
                                              (C.c_void_p * n)(*[_dev(g, torch.float32) for g in grays]),
                                              (1 if write_dog else 0) | (0 if write_grad else 2), _stream()),
           "nm_sift_scale_space_batch_ex")


class SiftArena:
    """Per-stream frame arena + outputs of nm_sift_detect_describe (replaces PyramidData + SiftData)."""

    def __init__(self, width, height, capacity=16384, device="cuda", num_items=None):
        """num_items: optional 1-element int32 device tensor (e.g. a view into a table of all arenas' counts) that
        receives the descriptor count instead of a tensor of the arena's own."""
        torch = _torch()
        self.width, self.height, self.capacity = width, height, capacity
        self._h = C.c_void_p()
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        # the native arena (buffers, side stream, events) is created on the CURRENT HIP device: make that `device`,
        # where the output tensors live; the launchers refuse an arena of another device (hipErrorInvalidDevice)
        with torch.cuda.device(self.device):
            _check(lib().nm_sift_arena_create(width, height, capacity, C.byref(self._h)), "nm_sift_arena_create")
        device = self.device
        self.desc = torch.zeros((capacity, 128), dtype=torch.float32, device=device)
        self.x = torch.zeros(capacity, dtype=torch.float32, device=device)
        self.y = torch.zeros(capacity, dtype=torch.float32, device=device)
        self.kpts = torch.zeros((capacity, 4), dtype=torch.float32, device=device)
        self.orients = torch.zeros((capacity, 2), dtype=torch.float32, device=device)
        if num_items is not None and (num_items.dtype != torch.int32 or num_items.numel() != 1 or num_items.device != device):
            raise NmError("num_items must be a 1-element int32 tensor on %s" % device)
        self.num_items = torch.zeros(1, dtype=torch.int32, device=device) if num_items is None else num_items

    @property
    def bytes(self):
        return lib().nm_sift_arena_bytes(self._h)

    def detect_describe(self, gray):
        """Enqueue one frame (device fp32 (H,W)) on the current stream; no host synchronisation."""
        torch = _torch()
        if tuple(gray.shape) != (self.height, self.width):
            raise NmError("frame shape %s does not match the arena (%d,%d)" % (tuple(gray.shape), self.height, self.width))
        if gray.device != self.device or torch.cuda.current_device() != self.device.index:
            raise NmError("arena lives on %s: frame on %s, current device %d" % (self.device, gray.device,
                                                                                torch.cuda.current_device()))
        _check(lib().nm_sift_detect_describe(self._h, _dev(gray, torch.float32), _dev(self.desc), _dev(self.x),
                                             _dev(self.y), _dev(self.kpts), _dev(self.orients), _dev(self.num_items),
                                             _stream()), "nm_sift_detect_describe")

    def set_params(self, peak_threshold=0.0, edge_threshold=10.0):
        """SiftParams::_peak_threshold / _edge_threshold for the calls enqueued from now on."""
        _check(lib().nm_sift_arena_set_params(self._h, peak_threshold, edge_threshold), "nm_sift_arena_set_params")

    def set_mask(self, mask=None):
        """Full-resolution float32 device mask (height, width) as in compute_keypoints_with_mask, or None. The arena
        keeps a reference to the tensor."""
        torch = _torch()
        if mask is not None and (tuple(mask.shape) != (self.height, self.width) or mask.device != self.device):
            raise NmError("mask must be a (%d, %d) tensor on %s" % (self.height, self.width, self.device))
        self._mask = mask
        _check(lib().nm_sift_arena_set_mask(self._h, _dev(mask, torch.float32) if mask is not None else None,
                                            self.width, self.height), "nm_sift_arena_set_mask")

    def tail_status(self):
        """0 / 1: whether the last octave-tail launch on this arena's state words timed out (synchronises the stream)."""
        v = C.c_int(0)
        _check(lib().nm_sift_arena_tail_status(self._h, C.byref(v), _stream()), "nm_sift_arena_tail_status")
        return v.value

    def tail_inject_error(self):
        _check(lib().nm_sift_arena_tail_inject_error(self._h), "nm_sift_arena_tail_inject_error")

    def octave_pyramid(self, ow, oh):
        _check(lib().nm_sift_octave_pyramid(self._h, ow, oh, _stream()), "nm_sift_octave_pyramid")

    def level_ptr(self, l):
        return lib().nm_sift_arena_level(self._h, l)

    def dog_ptr(self, d):
        return lib().nm_sift_arena_dog(self._h, d)

    def grad_ptr(self):
        return lib().nm_sift_arena_grad(self._h)

    def close(self):
        if self._h:
            lib().nm_sift_arena_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
