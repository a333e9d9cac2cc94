"""Loader of the in-tree C-ABI library (toyslam_amd/libndt_mi355.so).

There is no fallback of any kind: if the HIP library is missing this raises, and
if no gfx950 device is usable every compute call raises NdtError(NO_DEVICE).
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libndt_mi355.so")
CSRC = os.path.join(_HERE, "csrc")

NDT_OK, NDT_ERR_INVALID, NDT_ERR_NO_DEVICE, NDT_ERR_HIP, NDT_ERR_GRID_OVERFLOW, NDT_ERR_NO_INPUT, NDT_ERR_COMM = range(7)
KDTREE, DIRECT26, DIRECT7, DIRECT1 = 0, 1, 2, 3
BOX_ROUTES = ("none", "host_scalar", "host_avx2", "repack", "rec16_copy", "rec16_polled", "filter_rows", "multi_words", "staged", "select",
              "deskew")
EVAL_STRIDE = 32
COMM_ID_BYTES = 128

SELECT_FINITE, SELECT_BOX, SELECT_BOX_NEGATE, SELECT_RANGE, SELECT_RANGE_NEGATE, SELECT_KEY, SELECT_KEY_NEGATE = 1, 2, 4, 8, 16, 32, 64
OUTLIER_RADIUS, OUTLIER_STATISTICAL = 1, 2
NORMAL_KNN, NORMAL_RADIUS = 1, 2
NORMAL_KEEP_CURVATURE, NORMAL_KEEP_ANGLE, NORMAL_KEEP_NEGATE = 1, 2, 4
COV_LAPLACE, COV_SANDWICH = 0, 1
COV_INDEFINITE = 1
GICP_VOXEL_COV_PLANE, GICP_VOXEL_COV_RAW = 0, 1


class PoseInformation(C.Structure):
    """ndt_pose_information (include/ndt_mi355.h)"""
    _fields_ = [("A", C.c_double * 36), ("B", C.c_double * 36), ("g", C.c_double * 6), ("n_found", C.c_size_t),
                ("eig_min", C.c_double), ("eig_max", C.c_double), ("flags", C.c_int)]


class SelectSpec(C.Structure):
    """ndt_select_spec (include/ndt_mi355.h)"""
    _fields_ = [("flags", C.c_uint), ("box_min", C.c_float * 3), ("box_max", C.c_float * 3), ("centre", C.c_float * 3),
                ("r_min", C.c_float), ("r_max", C.c_float), ("key_lo", C.c_double), ("key_hi", C.c_double)]


class DeskewMotion(C.Structure):
    """ndt_deskew_motion (include/ndt_mi355.h)"""
    _fields_ = [("t_begin", C.c_double), ("t_end", C.c_double), ("t_ref", C.c_double), ("axis", C.c_double * 3), ("angle", C.c_double),
                ("tau_ref", C.c_double * 3)]


class RaySpec(C.Structure):
    """ndt_ray_spec (include/ndt_mi355.h)"""
    _fields_ = [("min_range", C.c_float), ("max_range", C.c_float), ("margin", C.c_float), ("min_rays", C.c_int)]


class OutlierSpec(C.Structure):
    """ndt_outlier_spec (include/ndt_mi355.h)"""
    _fields_ = [("method", C.c_int), ("negate", C.c_int), ("radius", C.c_float), ("min_neighbors", C.c_int), ("mean_k", C.c_int),
                ("stddev_mul", C.c_double)]


class OutlierStats(C.Structure):
    """ndt_outlier_stats (include/ndt_mi355.h)"""
    _fields_ = [("n_finite", C.c_size_t), ("n_valid", C.c_size_t), ("mean", C.c_double), ("stddev", C.c_double),
                ("threshold", C.c_double)]


class PlaneSpec(C.Structure):
    """ndt_plane_spec (include/ndt_mi355.h)"""
    _fields_ = [("distance_threshold", C.c_float), ("n_hypotheses", C.c_int), ("seed", C.c_uint64), ("use_axis", C.c_int),
                ("axis", C.c_float * 3), ("eps_angle", C.c_float), ("refine", C.c_int)]


class PlaneResult(C.Structure):
    """ndt_plane_result (include/ndt_mi355.h)"""
    _fields_ = [("found", C.c_int), ("refined", C.c_int), ("coeff", C.c_double * 4), ("best", C.c_int), ("best_count", C.c_size_t),
                ("n_inliers", C.c_size_t), ("n_finite", C.c_size_t), ("n_degenerate", C.c_size_t), ("n_rejected", C.c_size_t)]


class ClusterSpec(C.Structure):
    """ndt_cluster_spec (include/ndt_mi355.h)"""
    _fields_ = [("tolerance", C.c_float), ("min_size", C.c_int), ("max_size", C.c_int)]


class NormalSpec(C.Structure):
    """ndt_normal_spec (include/ndt_mi355.h)"""
    _fields_ = [("method", C.c_int), ("k", C.c_int), ("radius", C.c_float), ("min_neighbors", C.c_int), ("viewpoint", C.c_double * 3)]


class NormalStats(C.Structure):
    """ndt_normal_stats (include/ndt_mi355.h)"""
    _fields_ = [("n_finite", C.c_size_t), ("n_valid", C.c_size_t), ("n_collinear", C.c_size_t), ("max_neighbors", C.c_size_t)]


class NormalFilter(C.Structure):
    """ndt_normal_filter (include/ndt_mi355.h)"""
    _fields_ = [("flags", C.c_uint), ("curvature_lo", C.c_float), ("curvature_hi", C.c_float), ("axis", C.c_double * 3),
                ("cos_lo", C.c_double), ("cos_hi", C.c_double)]


class ClusterInfo(C.Structure):
    """ndt_cluster_info (include/ndt_mi355.h)"""
    _fields_ = [("root", C.c_int32), ("size", C.c_int32), ("first", C.c_uint32), ("box_min", C.c_float * 3), ("box_max", C.c_float * 3),
                ("centroid", C.c_double * 3)]


class ClusterSummary(C.Structure):
    """ndt_cluster_summary (include/ndt_mi355.h)"""
    _fields_ = [("n_finite", C.c_size_t), ("n_components", C.c_size_t), ("n_clusters", C.c_size_t), ("n_clustered", C.c_size_t),
                ("largest", C.c_size_t)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)
EVAL_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_double),
                      C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))


class NdtError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("ndt_mi355 status %d: %s" % (status, msg))
        self.status = status


def build(force=False):
    """Compile the HIP extension for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None

# name -> (restype, argtypes); also the list the symbol-export test walks
vp, fp, dp, ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)
szp = C.POINTER(C.c_size_t)
SIGNATURES = {
    "ndt_last_error": (C.c_char_p, []),
    "ndt_device_count": (C.c_int, []),
    "ndt_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
    "ndt_clone": (C.c_int, [vp, C.POINTER(vp)]),
    "ndt_destroy": (None, [vp]),
    "ndt_set_resolution": (C.c_int, [vp, C.c_float]),
    "ndt_set_step_size": (C.c_int, [vp, C.c_double]),
    "ndt_set_outlier_ratio": (C.c_int, [vp, C.c_double]),
    "ndt_set_transformation_epsilon": (C.c_int, [vp, C.c_double]),
    "ndt_set_maximum_iterations": (C.c_int, [vp, C.c_int]),
    "ndt_set_neighborhood_search_method": (C.c_int, [vp, C.c_int]),
    "ndt_set_num_threads": (C.c_int, [vp, C.c_int]),
    "ndt_set_min_points_per_voxel": (C.c_int, [vp, C.c_int]),
    "ndt_set_cov_eig_value_inflation_ratio": (C.c_int, [vp, C.c_double]),
    "ndt_get_resolution": (C.c_float, [vp]),
    "ndt_get_step_size": (C.c_double, [vp]),
    "ndt_get_outlier_ratio": (C.c_double, [vp]),
    "ndt_set_input_target": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.c_int]),
    "ndt_set_input_source": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t]),
    "ndt_set_input_target_device": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.c_int]),
    "ndt_set_input_source_device": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t]),
    "ndt_share_input_target": (C.c_int, [vp, vp]),
    "ndt_set_cu_partition": (C.c_int, [vp, C.c_int]),
    "ndt_get_cu_partition": (C.c_int, [vp, ip, ip]),
    "ndt_set_input_target_device_ref": (C.c_int, [vp, vp, C.c_size_t, C.c_int]),
    "ndt_set_input_source_device_ref": (C.c_int, [vp, vp, C.c_size_t]),
    "ndt_share_input_source": (C.c_int, [vp, vp]),
    "ndt_set_voxel_index": (C.c_int, [vp, C.c_int]),
    "ndt_align": (C.c_int, [vp, fp, fp, ip, ip, dp, vp, C.c_size_t]),
    "ndt_get_result": (C.c_int, [vp, fp, ip, ip, dp]),
    "ndt_get_output_device": (C.c_int, [vp, C.POINTER(vp), szp]),
    "ndt_get_stats": (C.c_int, [vp, ip, ip, dp]),
    "ndt_calculate_score": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t, dp]),
    "ndt_voxel_grid_filter": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.c_int, C.c_float, vp, C.c_size_t, szp]),
    "ndt_voxel_grid_filter_device": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.c_int, C.c_float, vp, szp]),
    "ndt_get_fitness_score": (C.c_int, [vp, C.c_double, dp]),
    "ndt_map_clear": (C.c_int, [vp]),
    "ndt_map_update": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.c_int, fp, C.c_float, ip]),
    "ndt_map_update_device": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.c_int, fp, C.c_float, ip]),
    "ndt_map_size": (C.c_int, [vp, szp]),
    "ndt_map_get": (C.c_int, [vp, vp, C.c_size_t]),
    "ndt_map_get_device": (C.c_int, [vp, C.POINTER(C.c_void_p), szp]),
    "ndt_cloud_voxel_filter": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.c_int, C.c_float, C.c_int, C.POINTER(vp), ip]),
    "ndt_warm_up": (C.c_int, [vp, C.c_size_t]),
    "ndt_cloud_upload": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(vp)]),
    "ndt_cloud_size": (C.c_int, [vp, szp]),
    "ndt_cloud_data": (C.c_int, [vp, C.POINTER(C.c_void_p), szp]),
    "ndt_cloud_download": (C.c_int, [vp, vp, vp, C.c_size_t]),
    "ndt_cloud_release": (None, [vp]),
    "ndt_cloud_bounds": (C.c_int, [vp, fp, ip]),
    "ndt_diag_input_bounds": (C.c_int, [vp, C.c_int, fp, ip]),
    "ndt_host_repack_bbox": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_int, vp, fp]),
    "ndt_set_input_source_cloud": (C.c_int, [vp, vp]),
    "ndt_set_input_target_cloud": (C.c_int, [vp, vp, C.c_int]),
    "ndt_map_update_cloud": (C.c_int, [vp, vp, C.c_int, fp, C.c_float, ip]),
    "ndt_map_update_clouds": (C.c_int, [vp, C.POINTER(vp), C.c_size_t, ip, fp, C.c_float, ip]),
    "ndt_map_update_batch": (C.c_int, [vp, vp, szp, C.c_size_t, C.c_size_t, ip, fp, C.c_float, C.c_int, ip]),
    "ndt_diag_map_batch": (C.c_int, [vp, szp, szp, szp]),
    "ndt_promote_source_to_target": (C.c_int, [vp, C.c_int]),
    "ndt_target_accumulate": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.c_int, fp]),
    "ndt_target_accumulate_device": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.c_int, fp]),
    "ndt_target_accumulate_cloud": (C.c_int, [vp, vp, C.c_int, fp]),
    "ndt_target_accumulate_clouds": (C.c_int, [vp, C.POINTER(vp), C.c_size_t, C.c_int, fp]),
    "ndt_target_accumulate_reset": (C.c_int, [vp]),
    "ndt_target_accumulated": (C.c_int, [vp, szp, szp, szp]),
    "ndt_diag_target_accumulate": (C.c_int, [vp, szp, szp, ip, ip, szp]),
    "ndt_target_accumulate_crop": (C.c_int, [vp, fp, fp]),
    "ndt_diag_target_crop": (C.c_int, [vp, szp, szp, szp, ip, szp]),
    "ndt_target_accumulate_clear_rays": (C.c_int, [vp, vp, fp, fp, C.POINTER(RaySpec)]),
    "ndt_target_accumulate_clear_rays_clouds": (C.c_int, [vp, C.POINTER(vp), C.c_size_t, fp, fp, C.POINTER(RaySpec)]),
    "ndt_target_accumulate_ray_counts": (C.c_int, [vp, C.POINTER(vp), C.c_size_t, fp, fp, C.POINTER(RaySpec), ip, C.POINTER(C.c_uint),
                                                   C.POINTER(C.c_ubyte), C.c_size_t, szp]),
    "ndt_diag_target_clear_rays": (C.c_int, [vp, szp, szp, C.POINTER(C.c_uint64), szp, szp, szp, szp, ip, szp]),
    "ndt_host_ray_spec_check": (C.c_int, [C.POINTER(RaySpec), C.c_float]),
    "ndt_host_ray_cells": (C.c_int, [fp, fp, C.c_float, C.c_float, ip, C.c_size_t, szp]),
    "ndt_host_ray_plan": (C.c_int, [C.c_size_t, ip, ip]),
    "ndt_target_accumulate_export": (C.c_int, [vp, fp, fp, vp, C.c_size_t, szp]),
    "ndt_target_accumulate_import": (C.c_int, [vp, vp, C.c_size_t]),
    "ndt_target_accumulate_save": (C.c_int, [vp, fp, fp, C.c_char_p]),
    "ndt_target_accumulate_load": (C.c_int, [vp, C.c_char_p]),
    "ndt_diag_target_export": (C.c_int, [vp, szp, szp, szp]),
    "ndt_host_acc_blob_info": (C.c_int, [vp, C.c_size_t, fp, szp, ip, ip]),
    "ndt_host_acc_blob_checksum": (C.c_int, [vp, C.c_size_t, C.POINTER(C.c_uint64)]),
    "ndt_host_acc_pack_cell": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]),
    "ndt_host_acc_unpack_cell": (None, [C.c_uint64, ip, ip, ip]),
    "ndt_host_chain_pose": (None, [fp, fp, fp]),
    "ndt_host_lattice": (C.c_int, [C.c_float, fp, fp, ip, ip, ip, C.POINTER(C.c_longlong), C.c_int, C.c_longlong, ip]),
    "ndt_pcd_read_header": (C.c_int, [C.c_char_p, szp, ip, ip]),
    "ndt_pcd_read_xyz": (C.c_int, [C.c_char_p, vp, C.c_size_t, C.c_size_t, szp, ip]),
    "ndt_pcd_write_xyz": (C.c_int, [C.c_char_p, vp, C.c_size_t, C.c_size_t, C.c_int]),
    "ndt_align_batch": (C.c_int, [vp, vp, szp, C.c_size_t, C.c_size_t, fp, fp, ip, ip, dp]),
    "ndt_align_batch_device": (C.c_int, [vp, vp, szp, C.c_size_t, C.c_size_t, fp, fp, ip, ip, dp]),
    "ndt_set_allreduce": (C.c_int, [vp, ALLREDUCE_FN, vp, C.c_int]),
    "ndt_set_batch_groups": (C.c_int, [vp, C.c_int]),
    "ndt_align_pairs": (C.c_int, [vp, vp, szp, C.c_size_t, C.c_size_t, C.c_int, ip, C.c_size_t, fp, fp, ip, ip, dp]),
    "ndt_align_pairs_clouds": (C.c_int, [vp, C.POINTER(vp), C.c_size_t, C.c_int, ip, C.c_size_t, fp, fp, ip, ip, dp]),
    "ndt_pairs_grid_size": (C.c_int, [vp, C.c_size_t, szp, szp]),
    "ndt_pairs_grid_info": (C.c_int, [vp, C.c_size_t, ip, ip, ip]),
    "ndt_pairs_grid_dump": (C.c_int, [vp, C.c_size_t, C.POINTER(C.c_int64), ip, dp, dp, dp, dp]),
    "ndt_pairs_fitness_scores": (C.c_int, [vp, fp, C.c_double, dp]),
    "ndt_pairs_count": (C.c_int, [vp, szp]),
    "ndt_diag_fitness_launches": (C.c_int, [vp, szp, szp]),
    "ndt_batch_fitness_scores": (C.c_int, [vp, vp, szp, C.c_size_t, C.c_size_t, fp, C.c_double, dp]),
    "ndt_batch_fitness_scores_device": (C.c_int, [vp, vp, szp, C.c_size_t, C.c_size_t, fp, C.c_double, dp]),
    "ndt_grid_centroids": (C.c_int, [vp, fp, C.POINTER(C.c_int64), C.c_size_t, szp]),
    "ndt_grid_centroids_cloud": (C.c_int, [vp, C.POINTER(vp)]),
    "ndt_get_centroid_fitness_score": (C.c_int, [vp, C.c_double, dp]),
    "ndt_batch_centroid_fitness_scores": (C.c_int, [vp, vp, szp, C.c_size_t, C.c_size_t, fp, C.c_double, dp]),
    "ndt_batch_centroid_fitness_scores_device": (C.c_int, [vp, vp, szp, C.c_size_t, C.c_size_t, fp, C.c_double, dp]),
    "ndt_diag_centroid_fitness": (C.c_int, [vp, szp, szp, fp, szp]),
    "ndt_score_poses": (C.c_int, [vp, fp, C.c_size_t, dp]),
    "ndt_diag_score_poses": (C.c_int, [vp, szp, szp]),
    "ndt_calculate_nvtl": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t, dp, szp]),
    "ndt_get_nvtl": (C.c_int, [vp, dp, szp]),
    "ndt_nvtl_poses": (C.c_int, [vp, fp, C.c_size_t, dp, szp]),
    "ndt_source_point_count": (C.c_int, [vp, szp]),
    "ndt_source_point_nvtl": (C.c_int, [vp, fp, dp, C.POINTER(C.c_void_p), dp, szp]),
    "ndt_diag_nvtl": (C.c_int, [vp, szp, szp]),
    "ndt_cloud_select": (C.c_int, [vp, vp, C.POINTER(SelectSpec), vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_int32), szp]),
    "ndt_cloud_select_clouds": (C.c_int, [vp, C.POINTER(vp), C.c_size_t, C.POINTER(SelectSpec), C.POINTER(vp), szp]),
    "ndt_source_select_by_nvtl": (C.c_int, [vp, fp, C.c_double, C.c_int, C.POINTER(vp), szp, szp]),
    "ndt_diag_select": (C.c_int, [vp, szp, szp, szp]),
    "ndt_host_select_point": (C.c_int, [C.POINTER(SelectSpec), fp, C.c_double, ip]),
    "ndt_host_select_plan": (C.c_int, [C.c_size_t, ip, ip]),
    "ndt_cloud_deskew": (C.c_int, [vp, vp, C.POINTER(DeskewMotion), vp, C.c_int, C.POINTER(vp), szp]),
    "ndt_cloud_deskew_clouds": (C.c_int, [vp, C.POINTER(vp), C.c_size_t, C.POINTER(DeskewMotion), vp, C.c_int, C.POINTER(vp), szp]),
    "ndt_diag_deskew": (C.c_int, [vp, szp, szp, szp]),
    "ndt_host_deskew_motion": (C.c_int, [fp, C.c_double, C.c_double, C.c_double, C.POINTER(DeskewMotion)]),
    "ndt_host_deskew_point": (C.c_int, [C.POINTER(DeskewMotion), fp, C.c_double, fp, ip]),
    "ndt_host_deskew_plan": (C.c_int, [C.c_size_t, ip, ip]),
    "ndt_host_extract_field": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, dp]),
    "ndt_pcd_read_field": (C.c_int, [C.c_char_p, C.c_char_p, dp, C.c_size_t, szp]),
    "ndt_cloud_neighbor_values": (C.c_int, [vp, vp, C.POINTER(OutlierSpec), vp, C.c_int, C.POINTER(OutlierStats)]),
    "ndt_cloud_remove_outliers": (C.c_int, [vp, vp, C.POINTER(OutlierSpec), C.POINTER(vp), C.POINTER(C.c_int32), szp,
                                            C.POINTER(OutlierStats)]),
    "ndt_cloud_remove_outliers_clouds": (C.c_int, [vp, C.POINTER(vp), C.c_size_t, C.POINTER(OutlierSpec), C.POINTER(vp), szp,
                                                   C.POINTER(OutlierStats)]),
    "ndt_diag_outliers": (C.c_int, [vp, szp, szp, szp, szp]),
    "ndt_host_outlier_spec_check": (C.c_int, [C.POINTER(OutlierSpec)]),
    "ndt_host_outlier_plan": (C.c_int, [C.c_size_t, ip, ip]),
    "ndt_cloud_plane_counts": (C.c_int, [vp, vp, C.POINTER(PlaneSpec), C.POINTER(C.c_int32), dp, C.POINTER(C.c_int32),
                                         C.POINTER(C.c_uint32)]),
    "ndt_cloud_segment_plane": (C.c_int, [vp, vp, C.POINTER(PlaneSpec), C.POINTER(C.c_int32), C.POINTER(PlaneResult), C.POINTER(vp),
                                          C.POINTER(vp)]),
    "ndt_cloud_segment_plane_clouds": (C.c_int, [vp, C.POINTER(vp), C.c_size_t, C.POINTER(PlaneSpec), C.POINTER(PlaneResult),
                                                 C.POINTER(vp), C.POINTER(vp)]),
    "ndt_cloud_plane_distances": (C.c_int, [vp, vp, dp, vp, C.c_int]),
    "ndt_diag_plane": (C.c_int, [vp, szp, szp, szp, szp]),
    "ndt_host_plane_spec_check": (C.c_int, [C.POINTER(PlaneSpec)]),
    "ndt_host_plane_sample": (C.c_int, [C.c_uint64, C.c_int, C.c_size_t, C.POINTER(C.c_int32)]),
    "ndt_host_plane_model": (C.c_int, [C.POINTER(PlaneSpec), fp, fp, fp, C.c_int, dp, ip]),
    "ndt_host_plane_distance": (C.c_int, [dp, fp, dp]),
    "ndt_host_plane_fit": (C.c_int, [C.POINTER(PlaneSpec), C.c_double, dp, dp, dp, dp, dp, ip]),
    "ndt_host_plane_plan": (C.c_int, [C.c_size_t, C.c_int, ip, ip, ip, ip, ip]),
    "ndt_cloud_cluster": (C.c_int, [vp, vp, C.POINTER(ClusterSpec), vp, C.c_int, vp, C.POINTER(ClusterInfo), C.c_size_t, C.POINTER(C.c_int32),
                                    C.POINTER(ClusterSummary)]),
    "ndt_cloud_extract_clusters": (C.c_int, [vp, vp, C.POINTER(ClusterSpec), C.c_int, C.POINTER(vp), C.POINTER(C.c_int32), szp,
                                             C.POINTER(ClusterSummary)]),
    "ndt_cloud_extract_clusters_clouds": (C.c_int, [vp, C.POINTER(vp), C.c_size_t, C.POINTER(ClusterSpec), C.c_int, C.POINTER(vp), szp,
                                                    C.POINTER(ClusterSummary)]),
    "ndt_diag_clusters": (C.c_int, [vp, szp, szp, szp, szp, szp]),
    "ndt_host_cluster_spec_check": (C.c_int, [C.POINTER(ClusterSpec)]),
    "ndt_host_cluster_plan": (C.c_int, [C.c_size_t, ip, ip]),
    "ndt_cloud_estimate_normals": (C.c_int, [vp, vp, C.POINTER(NormalSpec), vp, vp, C.c_int, C.POINTER(NormalStats)]),
    "ndt_cloud_estimate_normals_clouds": (C.c_int, [vp, C.POINTER(vp), C.c_size_t, C.POINTER(NormalSpec), vp, vp, C.c_int,
                                                    C.POINTER(NormalStats)]),
    "ndt_cloud_select_by_normals": (C.c_int, [vp, vp, C.POINTER(NormalSpec), C.POINTER(NormalFilter), C.POINTER(vp), C.POINTER(C.c_int32), szp,
                                              C.POINTER(NormalStats)]),
    "ndt_cloud_select_by_normals_clouds": (C.c_int, [vp, C.POINTER(vp), C.c_size_t, C.POINTER(NormalSpec), C.POINTER(NormalFilter),
                                                     C.POINTER(vp), szp, C.POINTER(NormalStats)]),
    "ndt_diag_normals": (C.c_int, [vp, szp, szp, szp, szp]),
    "ndt_host_normal_spec_check": (C.c_int, [C.POINTER(NormalSpec)]),
    "ndt_host_normal_filter_check": (C.c_int, [C.POINTER(NormalFilter)]),
    "ndt_host_normal_plan": (C.c_int, [C.c_size_t, ip, ip]),
    "ndt_host_normal_from_sums": (C.c_int, [C.POINTER(NormalSpec), fp, C.c_int, dp, dp, fp, ip]),
    "ndt_host_normal_keep": (C.c_int, [C.POINTER(NormalFilter), fp, ip]),
    "ndt_pose_covariance": (C.c_int, [vp, fp, C.c_int, C.c_double, dp, vp]),
    "ndt_pairs_pose_covariances": (C.c_int, [vp, fp, C.c_int, C.c_double, dp, vp]),
    "ndt_host_pose_covariance": (C.c_int, [dp, dp, dp, C.c_size_t, C.c_int, C.c_double, dp, dp, dp, ip]),
    "ndt_diag_pose_covariance": (C.c_int, [vp, szp, szp]),
    "ndt_align_guesses": (C.c_int, [vp, fp, C.c_size_t, fp, ip, ip, dp, ip]),
    "ndt_host_pick_top": (None, [dp, C.c_size_t, C.c_size_t, ip, szp]),
    "ndt_align_multistart": (C.c_int, [vp, fp, C.c_size_t, C.c_size_t, ip, szp, fp, ip, ip, dp, ip]),
    "ndt_align_batch_sharded": (C.c_int, [vp, vp, szp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, fp, fp, ip, ip, dp]),
    "ndt_align_batch_sharded_device": (C.c_int, [vp, vp, szp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, fp, fp, ip, ip, dp]),
    "ndt_comm_get_unique_id": (C.c_int, [vp]),
    "ndt_comm_init_rank": (C.c_int, [vp, vp, C.c_int, C.c_int]),
    "ndt_comm_destroy": (C.c_int, [vp]),
    "ndt_comm_stats": (C.c_int, [vp, ip, ip, C.POINTER(C.c_longlong), ip]),
    "ndt_eval": (C.c_int, [vp, dp, dp, dp, dp, dp]),
    "ndt_eval_with_matrix": (C.c_int, [vp, fp, dp, dp, dp, dp, dp]),
    "ndt_eval_hessian_f64": (C.c_int, [vp, dp, dp]),
    "ndt_grid_size": (C.c_int, [vp, szp, szp]),
    "ndt_grid_info": (C.c_int, [vp, ip, ip, ip]),
    "ndt_grid_dump": (C.c_int, [vp, C.POINTER(C.c_int64), ip, dp, dp, dp, dp]),
    "ndt_diag_stamps": (C.c_int, [vp, dp, C.POINTER(C.c_ulonglong), szp]),
    "ndt_diag_eval_plan": (C.c_int, [vp, C.c_size_t, ip, ip, ip, ip, ip]),
    "ndt_host_grid_plan": (C.c_int, [C.c_longlong, C.c_longlong, ip, ip, ip, ip, ip, ip, ip, ip, ip, C.POINTER(C.c_longlong), ip,
                                     C.POINTER(C.c_longlong), ip, ip, ip]),
    "ndt_diag_grid_build": (C.c_int, [vp, ip, szp, C.POINTER(C.c_longlong), ip, ip, ip, ip, ip, ip, C.POINTER(C.c_longlong), ip,
                                      C.POINTER(C.c_longlong), ip, ip]),
    "ndt_diag_server_roundtrip": (C.c_int, [vp, dp, C.c_int, dp]),
    "ndt_diag_selfdrive": (C.c_int, [vp, dp, C.c_int, dp]),
    "ndt_selftest_reduce": (C.c_int, [vp, C.c_int, dp]),
    "ndt_selftest_server_idle": (C.c_int, [vp, dp, C.c_int, ip, dp]),
    "ndt_profile_enable": (C.c_int, [vp, C.c_int]),
    "ndt_set_evaluation_path": (C.c_int, [vp, C.c_int]),
    "ndt_profile_read": (C.c_int, [vp, C.c_int, C.POINTER(C.c_longlong), dp, C.c_int]),
    "ndt_host_solve6": (None, [dp, dp, dp]),
    "ndt_host_pose_to_matrix": (None, [dp, fp]),
    "ndt_host_matrix_to_pose": (None, [fp, dp]),
    "ndt_host_angle_derivatives": (None, [dp, fp, fp, dp, dp]),
    "ndt_host_gauss": (None, [C.c_float, C.c_double, dp]),
    "ndt_host_thread_budget": (None, [ip, dp, ip]),
    "ndt_host_thread_plan": (None, [C.c_int, C.c_double, C.c_int, ip, ip]),
    "ndt_host_run_driver": (C.c_int, [EVAL_CB, vp, C.c_size_t, fp, C.c_float, C.c_double, C.c_double, C.c_double,
                                      C.c_int, fp, ip, ip, dp, ip, ip]),
    "ndt_host_run_driver_reuse": (C.c_int, [EVAL_CB, vp, C.c_size_t, fp, C.c_float, C.c_double, C.c_double, C.c_double,
                                            C.c_int, fp, ip, ip, dp, ip, ip, ip]),
    "ndt_set_evaluation_reuse": (C.c_int, [vp, C.c_int]),
    "ndt_diag_eval_reuse": (C.c_int, [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "ndt_diag_eval_server": (C.c_int, [vp, dp, C.c_int, C.c_int, dp]),
    "ndt_pcd_sequence_open": (C.c_int, [C.c_char_p, C.POINTER(vp)]),
    "ndt_pcd_sequence_poll": (C.c_int, [vp, C.c_size_t, szp]),
    "ndt_pcd_sequence_next": (C.c_int, [vp, C.POINTER(vp), szp, ip, ip]),
    "ndt_pcd_sequence_close": (None, [vp]),
    "ndt_pcd_sequence_stage": (C.c_int, [vp, C.c_int]),
    "ndt_pcd_sequence_next_cloud": (C.c_int, [vp, C.POINTER(vp), C.POINTER(C.c_void_p), szp, ip, ip]),
    "ndt_cloud_voxel_filter_begin": (C.c_int, [vp, vp, C.c_int, C.c_float]),
    "ndt_cloud_voxel_filter_end": (C.c_int, [vp, C.POINTER(vp), ip]),
    "ndt_cloud_voxel_filter_batch": (C.c_int, [vp, vp, szp, C.c_size_t, C.c_size_t, ip, C.c_float, C.c_int, C.POINTER(vp), ip]),
    "ndt_cloud_voxel_filter_clouds": (C.c_int, [vp, C.POINTER(vp), C.c_size_t, ip, C.c_float, C.POINTER(vp), ip]),
    "ndt_diag_filter_batch": (C.c_int, [vp, szp, szp, szp]),
    "ndt_pcd_sequence_next_device": (C.c_int, [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), szp, ip, ip]),
    "ndt_host_extract_file_number": (C.c_int, [C.c_char_p]),
    "ndt_host_repack_fields": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, vp, ip]),
    # GICP row (include/gicp_mi355.h)
    "gicp_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
    "gicp_destroy": (None, [vp]),
    "gicp_set_correspondence_randomness": (C.c_int, [vp, C.c_int]),
    "gicp_set_rotation_epsilon": (C.c_int, [vp, C.c_double]),
    "gicp_set_maximum_optimizer_iterations": (C.c_int, [vp, C.c_int]),
    "gicp_set_transformation_epsilon": (C.c_int, [vp, C.c_double]),
    "gicp_set_maximum_iterations": (C.c_int, [vp, C.c_int]),
    "gicp_set_max_correspondence_distance": (C.c_int, [vp, C.c_double]),
    "gicp_set_input_target": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t]),
    "gicp_set_input_source": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t]),
    "gicp_set_source_covariances": (C.c_int, [vp, dp, C.c_size_t]),
    "gicp_set_target_covariances": (C.c_int, [vp, dp, C.c_size_t]),
    "gicp_set_input_target_cloud": (C.c_int, [vp, vp]),
    "gicp_set_input_source_cloud": (C.c_int, [vp, vp]),
    "gicp_set_input_target_grid": (C.c_int, [vp, vp, C.c_int]),
    "gicp_target_grid_voxels": (C.c_int, [vp, fp, dp, C.POINTER(C.c_int64), C.c_size_t, szp]),
    "gicp_diag_target_grid": (C.c_int, [vp, szp, szp, fp, szp]),
    "gicp_align_pairs_clouds": (C.c_int, [vp, C.POINTER(vp), C.c_size_t, ip, C.c_size_t, fp, C.c_double, fp, ip, ip, ip, dp]),
    "gicp_align_pairs_lockstep": (C.c_int, [vp, C.POINTER(vp), C.c_size_t, ip, C.c_size_t, fp, C.c_double, fp, ip, ip, ip, dp]),
    "gicp_align_guesses": (C.c_int, [vp, fp, C.c_size_t, C.c_double, fp, ip, ip, ip, dp]),
    "gicp_diag_lockstep": (C.c_int, [vp, szp, szp, szp, szp]),
    "gicp_pairs_covariances": (C.c_int, [vp, C.c_size_t, dp]),
    "gicp_diag_pairs": (C.c_int, [vp, szp, szp, szp]),
    "gicp_diag_pairs_time": (C.c_int, [vp, dp, dp]),
    "gicp_align": (C.c_int, [vp, fp, fp, ip, ip, vp]),
    "gicp_get_result": (C.c_int, [vp, fp, ip, ip]),
    "gicp_get_fitness_score": (C.c_int, [vp, C.c_double, dp]),
    "gicp_get_stats": (C.c_int, [vp, ip, ip, ip, ip]),
    "gicp_covariances": (C.c_int, [vp, C.c_int, dp, ip, fp]),
    "gicp_step_correspond": (C.c_int, [vp, fp, fp, ip, fp, ip]),
    "gicp_step_functor": (C.c_int, [vp, C.c_int, dp, dp, dp]),
    "gicp_diag_plan": (C.c_int, [vp, C.c_size_t, ip]),
    "gicp_host_apply_state": (None, [dp, fp]),
}


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(status):
    if status != NDT_OK:
        raise NdtError(status, lib().ndt_last_error().decode("utf-8", "replace"))
