"""ctypes binding of the C ABI in include/ks_hip.h (libks_hip.so).

Plumbing for tests and bench.py; the product boundary is the C ABI itself and the C++
adapter in kimera_semantics_amd/host/.  There is NO CPU fallback: if the HIP library is
missing or no GPU is present, constructing an integrator raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KS_HIP_LIB") or os.path.join(_HERE, "libks_hip.so")   # KS_HIP_LIB: a diagnostics build
NUM_LABELS = 21

KS_METHOD_FAST, KS_METHOD_MERGED = 0, 1
KS_COLOR_MODE_COLOR, KS_COLOR_MODE_SEMANTIC, KS_COLOR_MODE_SEMANTIC_PROBABILITY = 0, 1, 2
KS_ORDER_MIXED, KS_ORDER_SORTED, KS_ORDER_MIXED_1024_GROUPS = 0, 1, 2   # include/ks_hip.h
KS_BUNDLE_ORDER_REFERENCE, KS_BUNDLE_ORDER_CANONICAL = 0, 1
KS_EARLY_OUT_EXACT = 1   # value of KsConfig.early_out_phase_growth: the reference's serial early-out result
KS_ERR_LABEL_RANGE, KS_ERR_PROBABILITY, KS_ERR_POOL_FULL, KS_ERR_NO_DEVICE, KS_ERR_UNSUPPORTED = -2, -3, -5, -7, -8
KS_ERR_INVALID_ARG, KS_ERR_PEER_FAILED = -1, -9
KS_ERR_HIP, KS_ERR_INDEX_RANGE = -4, -6

STAGES = ["points", "sort_points", "rays", "march", "emit", "sort_pairs", "apply", "apply_long"]

TSDF_DTYPE = np.dtype([("distance", "<f4"), ("weight", "<f4"), ("color", "u1", (4,))])
SEM_DTYPE = np.dtype([("label", "u1"), ("pad", "u1", (3,)), ("priors", "<f4", (NUM_LABELS,)),
                      ("color", "u1", (4,))])

# Every symbol include/ks_hip.h declares (checked by tests/test_abi.py).
ABI_SYMBOLS = [
    "ks_default_config", "ks_create", "ks_destroy", "ks_last_error", "ks_set_color_to_label",
    "ks_integrate_points", "ks_integrate_points_device", "ks_integrate_depth", "ks_integrate_depth_device", "ks_num_blocks", "ks_get_block_indices",
    "ks_get_updated_block_indices", "ks_count_updated_voxels", "ks_download_updated_voxels", "ks_download_blocks", "ks_upload_blocks", "ks_host_alloc", "ks_host_free", "ks_get_tile_keys", "ks_export_tiles_device", "ks_merge_tiles_device", "ks_clear", "ks_clear_voxels", "ks_reset_tiles", "ks_tile_owner", "ks_reduce",
    "ks_debug_radix_sort", "ks_debug_radix_sort_range", "ks_debug_radix_sort_batch", "ks_synchronize", "ks_flush", "ks_stream",
    "ks_profile_enable", "ks_profile_get", "ks_early_out_iterations", "ks_early_out_stats", "ks_pipeline_shape", "ks_stream_plan", "ks_tail_batch_stats", "ks_tail_batch_rule", "ks_seed_launch_shape", "ks_update_stats", "ks_integrate_round_exact",
    "ks_mesh_default_config", "ks_mesh_update", "ks_mesh_size", "ks_mesh_download", "ks_mesh_changed_blocks",
    "ks_esdf_default_config", "ks_esdf_update", "ks_esdf_download_blocks", "ks_esdf_query",
    "ks_esdf_refresh", "ks_esdf_changed_blocks",
    "ks_esdf_sample", "ks_esdf_sample_device", "ks_esdf_slice", "ks_esdf_slice_device",
    "ks_esdf_sweep_default_config", "ks_esdf_sweep", "ks_esdf_sweep_device",
    "ks_render_default_config", "ks_render_view", "ks_render_view_device",
    "ks_align_default_config", "ks_align_points", "ks_align_points_device",
    "ks_objects_default_config", "ks_objects_update", "ks_objects_size", "ks_objects_download", "ks_objects_download_blocks", "ks_objects_query",
    "ks_remove_blocks", "ks_remove_distant_blocks", "ks_removed_blocks",
    "ks_fuse_default_config", "ks_fuse_map",
    "ks_mesh_index", "ks_mesh_index_size", "ks_mesh_index_download",
    "ks_nav_default_config", "ks_nav_update", "ks_nav_query", "ks_nav_query_device", "ks_nav_download_blocks", "ks_nav_paths", "ks_nav_paths_device",
    "ks_frontiers_default_config", "ks_frontiers_update", "ks_frontiers_size", "ks_frontiers_download", "ks_frontiers_download_blocks", "ks_frontiers_query",
    "ks_rooms_default_config", "ks_rooms_update", "ks_rooms_size", "ks_rooms_download", "ks_rooms_links_download", "ks_rooms_objects",
    "ks_rooms_download_blocks", "ks_rooms_query",
    "ks_view_gain_default_config", "ks_view_gain", "ks_view_gain_device",
    "ks_path_shorten_default_config", "ks_path_shorten", "ks_path_shorten_device",
]


class KsConfig(C.Structure):
    _fields_ = [
        ("voxel_size", C.c_float), ("voxels_per_side", C.c_int32),
        ("truncation_distance", C.c_float), ("max_weight", C.c_float),
        ("min_ray_length_m", C.c_float), ("max_ray_length_m", C.c_float),
        ("voxel_carving_enabled", C.c_int32), ("use_const_weight", C.c_int32),
        ("allow_clear", C.c_int32), ("use_weight_dropoff", C.c_int32),
        ("use_sparsity_compensation_factor", C.c_int32), ("sparsity_compensation_factor", C.c_float),
        ("enable_anti_grazing", C.c_int32), ("start_voxel_subsampling_factor", C.c_float),
        ("max_consecutive_ray_collisions", C.c_int32), ("clear_checks_every_n_frames", C.c_int32),
        ("integration_order_mode", C.c_int32), ("integrator_threads", C.c_int32),
        ("method", C.c_int32), ("bundle_order", C.c_int32),
        ("semantic_measurement_probability", C.c_float), ("color_mode", C.c_int32),
        ("n_dynamic_labels", C.c_int32), ("dynamic_labels", C.c_uint8 * 32),
        ("label_rgba", (C.c_uint8 * 4) * 256),
        ("early_out_phase_growth", C.c_int32),
        ("device_id", C.c_int32), ("max_tiles", C.c_uint32), ("max_points", C.c_uint32), ("pipeline_frames", C.c_int32),
    ]


class KsRoundStats(C.Structure):
    _fields_ = [("updates_marched", C.c_uint64), ("updates_applied", C.c_uint64), ("bytes_sent", C.c_uint64),
                ("origin_voxel_touched", C.c_uint64), ("rays_cast", C.c_uint64)]


class KsFrameStats(C.Structure):
    _fields_ = [("n_points", C.c_uint64), ("n_valid_points", C.c_uint64), ("n_rays_cast", C.c_uint64),
                ("n_voxel_updates", C.c_uint64), ("n_blocks_allocated", C.c_uint64)]


class KsReduceStats(C.Structure):
    _fields_ = [("tiles_sent", C.c_uint64), ("tiles_received", C.c_uint64), ("tiles_local", C.c_uint64),
                ("bytes_sent", C.c_uint64)]


class KsMeshConfig(C.Structure):
    _fields_ = [("min_weight", C.c_float), ("only_stale", C.c_int32)]


class KsMeshStats(C.Structure):
    _fields_ = [("blocks_meshed", C.c_uint64), ("blocks_total", C.c_uint64), ("triangles_total", C.c_uint64),
                ("triangles_changed", C.c_uint64), ("degenerate_dropped", C.c_uint64)]


MESH_BLOCK_DTYPE = np.dtype([("block", "<i4", (3,)), ("first_vertex", "<u4"), ("n_vertices", "<u4")])


class KsEsdfConfig(C.Structure):
    _fields_ = [("min_weight", C.c_float), ("min_distance_m", C.c_float), ("max_distance_m", C.c_float), ("use_region", C.c_int32),
                ("region_min", C.c_int32 * 3), ("region_max", C.c_int32 * 3), ("max_workspace_bytes", C.c_uint64)]


class KsEsdfStats(C.Structure):
    _fields_ = [("voxels_observed", C.c_uint64), ("voxels_fixed", C.c_uint64), ("voxels_clamped", C.c_uint64),
                ("box_voxels", C.c_uint64 * 3), ("workspace_bytes", C.c_uint64)]


class KsEsdfRefreshStats(C.Structure):
    _fields_ = [("tiles_stale", C.c_uint64), ("tiles_recomputed", C.c_uint64), ("tiles_total", C.c_uint64),
                ("voxels_observed", C.c_uint64), ("voxels_fixed", C.c_uint64), ("voxels_clamped", C.c_uint64),
                ("workspace_bytes", C.c_uint64)]


# KS_ESDF_RECORD_BYTES = 8; flags = observed | fixed << 1; label 255 = no site within reach (or a default record)
ESDF_DTYPE = np.dtype([("distance", "<f4"), ("flags", "u1"), ("label", "u1"), ("pad", "u1", (2,))])


class KsEsdfSampleStats(C.Structure):
    _fields_ = [("points_interpolated", C.c_uint64), ("points_nearest", C.c_uint64), ("points_unknown", C.c_uint64)]


class KsEsdfSweepConfig(C.Structure):
    _fields_ = [("radius_m", C.c_float), ("min_step_m", C.c_float), ("unknown_is_free", C.c_int32), ("max_samples", C.c_int32)]


class KsEsdfSweepStats(C.Structure):
    _fields_ = [("segments_free", C.c_uint64), ("segments_collision", C.c_uint64), ("segments_unknown", C.c_uint64),
                ("segments_invalid", C.c_uint64), ("samples", C.c_uint64)]


KS_ESDF_UNKNOWN, KS_ESDF_NEAREST, KS_ESDF_INTERPOLATED = 0, 1, 2
KS_SWEEP_FREE, KS_SWEEP_COLLISION, KS_SWEEP_UNKNOWN, KS_SWEEP_INVALID = 0, 1, 2, 3


class KsNavConfig(C.Structure):
    _fields_ = [("radius_m", C.c_float), ("max_cost", C.c_uint32), ("max_rounds", C.c_uint32), ("pad", C.c_uint32)]


class KsNavStats(C.Structure):
    _fields_ = [("voxels_traversable", C.c_uint64), ("voxels_reached", C.c_uint64), ("goals_used", C.c_uint64), ("goals_blocked", C.c_uint64),
                ("largest_cost", C.c_uint64), ("rounds", C.c_uint64), ("tile_relaxations", C.c_uint64), ("workspace_bytes", C.c_uint64)]


class KsNavPathStats(C.Structure):
    _fields_ = [("paths_reached", C.c_uint64), ("paths_unreachable", C.c_uint64), ("paths_blocked", C.c_uint64),
                ("paths_truncated", C.c_uint64), ("waypoints", C.c_uint64)]


KS_NAV_BLOCKED, KS_NAV_UNREACHED, KS_NAV_MAX_COST = 0xffffffff, 0xfffffffe, 0xffffff00
KS_NAV_COST_FACE, KS_NAV_COST_EDGE, KS_NAV_COST_CORNER = 10, 14, 17
KS_NAV_PATH_REACHED, KS_NAV_PATH_UNREACHABLE, KS_NAV_PATH_BLOCKED, KS_NAV_PATH_TRUNCATED, KS_NAV_PATH_INVALID = 0, 1, 2, 3, 4


class KsPathShortenConfig(C.Structure):
    _fields_ = [("radius_m", C.c_float), ("min_step_m", C.c_float), ("unknown_is_free", C.c_int32), ("max_samples", C.c_int32),
                ("lookahead", C.c_uint32), ("pad", C.c_uint32 * 3)]


class KsPathShortenStats(C.Structure):
    _fields_ = [("paths_ok", C.c_uint64), ("paths_unverified", C.c_uint64), ("paths_invalid", C.c_uint64), ("waypoints_in", C.c_uint64),
                ("waypoints_out", C.c_uint64), ("segments_unverified", C.c_uint64), ("sweeps", C.c_uint64), ("samples", C.c_uint64)]


KS_SHORTEN_OK, KS_SHORTEN_UNVERIFIED, KS_SHORTEN_INVALID = 0, 1, 2


class KsRenderConfig(C.Structure):
    _fields_ = [("min_weight", C.c_float), ("min_range_m", C.c_float), ("max_range_m", C.c_float)]


class KsRenderStats(C.Structure):
    _fields_ = [("pixels_hit", C.c_uint64), ("pixels_missed", C.c_uint64), ("samples", C.c_uint64)]


class KsAlignConfig(C.Structure):
    _fields_ = [("min_weight", C.c_float), ("max_residual_m", C.c_float), ("damping", C.c_float), ("eps_rotation_rad", C.c_float),
                ("eps_translation_m", C.c_float), ("max_iterations", C.c_int32), ("point_stride", C.c_int32), ("min_inliers", C.c_int32),
                ("dof_mask", C.c_uint32)]


class KsAlignStats(C.Structure):
    _fields_ = [("status", C.c_uint32), ("iterations", C.c_uint32), ("points_used", C.c_uint64), ("inliers_first", C.c_uint64),
                ("inliers_last", C.c_uint64), ("rmse_first", C.c_double), ("rmse_last", C.c_double)]


class KsObjectsConfig(C.Structure):
    _fields_ = [("min_weight", C.c_float), ("surface_distance_m", C.c_float), ("label_mask", C.c_uint32), ("min_voxels", C.c_uint32)]


class KsObjectsStats(C.Structure):
    _fields_ = [("voxels_surface", C.c_uint64), ("components", C.c_uint64), ("objects", C.c_uint64), ("voxels_in_objects", C.c_uint64),
                ("largest_object_voxels", C.c_uint64), ("workspace_bytes", C.c_uint64)]


class KsRemoveStats(C.Structure):
    _fields_ = [("blocks_removed", C.c_uint64), ("tiles_removed", C.c_uint64), ("tiles_moved", C.c_uint64), ("tiles_resident", C.c_uint64),
                ("pool_capacity_tiles", C.c_uint64)]


class KsFuseConfig(C.Structure):
    _fields_ = [("min_weight", C.c_float), ("pad", C.c_uint32), ("max_workspace_bytes", C.c_uint64)]


class KsFuseStats(C.Structure):
    _fields_ = [("tiles_source", C.c_uint64), ("tiles_candidate", C.c_uint64), ("tiles_touched", C.c_uint64), ("tiles_allocated", C.c_uint64),
                ("voxels_fused", C.c_uint64), ("chunks", C.c_uint64), ("workspace_bytes", C.c_uint64)]


class KsMeshIndexStats(C.Structure):
    _fields_ = [("corners", C.c_uint64), ("vertices", C.c_uint64), ("max_corners_per_vertex", C.c_uint64), ("workspace_bytes", C.c_uint64)]


# ks_object: 72 bytes; centroid_k = (sum_k / n_voxels + 0.5) * voxel_size (object_centroids)
OBJECT_DTYPE = np.dtype([("first_voxel", "<i4", (3,)), ("n_voxels", "<u4"), ("bb_min", "<i4", (3,)), ("bb_max", "<i4", (3,)),
                         ("sum", "<i8", (3,)), ("label", "<u4"), ("pad", "<u4")])
KS_OBJECT_NONE = 0xffffffff


def object_centroids(records, voxel_size) -> np.ndarray:
    """Centroids in metres, (n, 3) f64, of ks_object records: the host's one division."""
    r = np.asarray(records)
    return (r["sum"].astype(np.float64) / np.maximum(r["n_voxels"], 1)[:, None].astype(np.float64) + 0.5) * float(voxel_size)


class KsFrontierConfig(C.Structure):
    _fields_ = [("radius_m", C.c_float), ("min_voxels", C.c_uint32), ("use_bounds", C.c_int32), ("bounds_min", C.c_int32 * 3),
                ("bounds_max", C.c_int32 * 3), ("pad", C.c_uint32)]


class KsFrontierStats(C.Structure):
    _fields_ = [("voxels_traversable", C.c_uint64), ("voxels_frontier", C.c_uint64), ("components", C.c_uint64), ("frontiers", C.c_uint64),
                ("voxels_in_frontiers", C.c_uint64), ("largest_frontier_voxels", C.c_uint64), ("unknown_faces", C.c_uint64),
                ("nav_field_used", C.c_uint64), ("workspace_bytes", C.c_uint64)]


# ks_frontier: 88 bytes; centroid as for ks_object (frontier_centroids), the start of a path to it: frontier_targets
FRONTIER_DTYPE = np.dtype([("first_voxel", "<i4", (3,)), ("n_voxels", "<u4"), ("bb_min", "<i4", (3,)), ("bb_max", "<i4", (3,)),
                           ("sum", "<i8", (3,)), ("unknown_faces", "<u4"), ("nav_cost", "<u4"), ("nav_voxel", "<i4", (3,)), ("pad", "<u4")])
KS_FRONTIER_NONE = 0xffffffff


def frontier_centroids(records, voxel_size) -> np.ndarray:
    """Centroids in metres, (n, 3) f64, of ks_frontier records: the host's one division."""
    return object_centroids(records, voxel_size)


def frontier_targets(records, voxel_size) -> np.ndarray:
    """(n, 3) f32: the centres of the records' nav_voxel, ((float)v + 0.5f) * voxel_size — valid starts for nav_paths."""
    v = np.asarray(records)["nav_voxel"].astype(np.float32)
    return (v + np.float32(0.5)) * np.float32(voxel_size)


def frontier_bounds(box_min_m, box_max_m, voxel_size):
    """(bounds_min, bounds_max) int32 (3,): the voxels that contain the two corners of a metric box, by ks_esdf_query's
    point-to-voxel rule floor(p * (1 / voxel_size) + 1e-6) in f32."""
    inv = np.float32(1.0 / np.float64(np.float32(voxel_size)))
    lo, hi = (np.floor(np.asarray(p, np.float32).reshape(3) * inv + np.float32(1e-6)).astype(np.int32) for p in (box_min_m, box_max_m))
    return lo, hi


class KsRoomsConfig(C.Structure):
    _fields_ = [("free_distance_m", C.c_float), ("core_distance_m", C.c_float), ("min_core_voxels", C.c_uint32), ("max_cost", C.c_uint32),
                ("max_rounds", C.c_uint32), ("use_bounds", C.c_int32), ("bounds_min", C.c_int32 * 3), ("bounds_max", C.c_int32 * 3)]


class KsRoomsStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("voxels_free", "voxels_core", "components", "rooms", "voxels_assigned", "voxels_unassigned",
                                          "largest_room_voxels", "largest_cost", "links", "contacts", "objects_seen", "objects_joined",
                                          "rounds", "tile_relaxations", "workspace_bytes")]


# ks_room: 96 bytes; centroid as for ks_object (room_centroids), a goal inside the room: room_centres.  ks_room_link: 32 bytes.
ROOM_DTYPE = np.dtype([("first_voxel", "<i4", (3,)), ("n_core_voxels", "<u4"), ("bb_min", "<i4", (3,)), ("bb_max", "<i4", (3,)),
                       ("sum", "<i8", (3,)), ("n_voxels", "<u4"), ("largest_cost", "<u4"), ("clearance_bits", "<u4"),
                       ("centre_voxel", "<i4", (3,)), ("n_links", "<u4"), ("n_objects", "<u4")])
ROOM_LINK_DTYPE = np.dtype([("room_a", "<u4"), ("room_b", "<u4"), ("n_contacts", "<u4"), ("clearance_bits", "<u4"),
                            ("door_voxel", "<i4", (3,)), ("door_room", "<u4")])
KS_ROOM_NONE = 0xffffffff


def room_centroids(records, voxel_size) -> np.ndarray:
    """Centroids in metres, (n, 3) f64, of ks_room records over their assigned voxels: the host's one division.  The centroid of an
    L-shaped room can lie inside a wall; room_centres never does."""
    return object_centroids(records, voxel_size)


def room_centres(records, voxel_size) -> np.ndarray:
    """(n, 3) f32: the centres of the records' centre_voxel, ((float)v + 0.5f) * voxel_size — free, and valid goals for nav_update."""
    v = np.asarray(records)["centre_voxel"].astype(np.float32)
    return (v + np.float32(0.5)) * np.float32(voxel_size)


class KsViewGainConfig(C.Structure):
    _fields_ = [("min_range_m", C.c_float), ("max_range_m", C.c_float), ("step_m", C.c_float), ("stop_distance_m", C.c_float),
                ("width", C.c_uint32), ("height", C.c_uint32), ("K", C.c_float * 4), ("label", C.c_uint32), ("pad", C.c_uint32),
                ("max_workspace_bytes", C.c_uint64)]


class KsViewGainStats(C.Structure):
    _fields_ = [("views_valid", C.c_uint64), ("views_invalid", C.c_uint64), ("unknown_voxels", C.c_uint64), ("free_voxels", C.c_uint64),
                ("surface_voxels", C.c_uint64), ("label_voxels", C.c_uint64), ("rays_hit", C.c_uint64), ("rays_open", C.c_uint64),
                ("samples", C.c_uint64), ("workspace_bytes", C.c_uint64), ("views_in_lds", C.c_uint64)]


# ks_view_gain_record: 32 bytes, one per candidate pose
VIEW_GAIN_DTYPE = np.dtype([(k, "<u4") for k in ("unknown_voxels", "free_voxels", "surface_voxels", "label_voxels", "rays_hit", "rays_open",
                                                  "samples", "flags")])
KS_VIEW_GAIN_VALID = 1


def view_gain_yaw_poses(xyz, n_yaws=8) -> np.ndarray:
    """(n * n_yaws, 7) f32 candidate poses T_G_C for view_gain: at every position of xyz (n, 3) a level camera (optical axis
    horizontal, image y pointing down the world's -z) turned about the world's z axis in n_yaws equal steps from +x."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    half = np.pi * np.arange(n_yaws) / n_yaws
    cz, sz = np.cos(half), np.sin(half)
    w0, x0, y0, z0 = 0.5, -0.5, 0.5, -0.5                       # camera z -> world x, camera x -> world -y, camera y -> world -z
    q = np.stack([cz * w0 - sz * z0, cz * x0 - sz * y0, cz * y0 + sz * x0, cz * z0 + sz * w0], axis=1)   # (cz, 0, 0, sz) * q0
    out = np.zeros((len(xyz), n_yaws, 7), np.float32)
    out[:, :, :4] = q[None, :, :]
    out[:, :, 4:] = xyz[:, None, :]
    return out.reshape(-1, 7)


KS_ALIGN_CONVERGED, KS_ALIGN_ITERATION_LIMIT, KS_ALIGN_TOO_FEW_INLIERS, KS_ALIGN_DEGENERATE = 0, 1, 2, 3


class KsProfile(C.Structure):
    _fields_ = [("ms", C.c_double * 8), ("launches", C.c_uint64 * 8), ("frames", C.c_uint64),
                ("updates", C.c_uint64), ("points", C.c_uint64), ("apply_kernel_ms", C.c_double),
                ("apply_kernel_launches", C.c_uint64), ("apply_kernel_updates", C.c_uint64),
                ("host_ms", C.c_double), ("host_wait_ms", C.c_double)]


def build(force: bool = False) -> str:
    """Compile libks_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    src_dir = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(src_dir, f) for f in ("ks_hip.hip", "ks_types.h", "ks_k_rays.h", "ks_k_bundle_order.h", "ks_k_march.h", "ks_k_exact.h", "ks_k_apply.h",
                                                "ks_k_apply_xl.h", "ks_k_shard.h", "ks_k_shard_merged.h", "ks_k_io.h", "ks_k_mesh.h", "ks_k_mesh_index.h", "ks_k_esdf.h", "ks_k_esdf_read.h", "ks_k_render.h", "ks_k_align.h", "ks_k_objects.h", "ks_k_nav.h", "ks_k_frontier.h", "ks_k_rooms.h", "ks_k_view_gain.h", "ks_k_path.h", "ks_k_remove.h", "ks_k_fuse.h", "ks_mc_tri_table.inc", "ks_device_math.h", "ks_radix_sort.h", "ks_owned.h")]
    srcs.append(os.path.join(_HERE, "..", "include", "ks_hip.h"))
    stale = (not os.path.exists(LIB_PATH)) or any(
        os.path.exists(s) and os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", src_dir])
    return LIB_PATH


_lib = None


def lib():
    """Loads libks_hip.so.  Raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(the HIP path has no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.ks_default_config.argtypes = [C.POINTER(KsConfig)]
        L.ks_create.argtypes = [C.POINTER(KsConfig), C.POINTER(vp)]
        L.ks_destroy.argtypes = [vp]
        L.ks_destroy.restype = None
        L.ks_last_error.argtypes = [vp]
        L.ks_last_error.restype = C.c_char_p
        L.ks_set_color_to_label.argtypes = [vp, vp, vp, C.c_size_t]
        L.ks_integrate_points.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, C.c_int, C.POINTER(KsFrameStats)]
        L.ks_integrate_points_device.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, C.c_int, C.POINTER(KsFrameStats)]
        L.ks_integrate_depth.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.POINTER(KsFrameStats)]
        L.ks_integrate_depth_device.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.POINTER(KsFrameStats)]
        L.ks_num_blocks.argtypes = [vp, C.POINTER(C.c_size_t)]
        L.ks_get_block_indices.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ks_get_updated_block_indices.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.c_int]
        L.ks_download_blocks.argtypes = [vp, vp, C.c_size_t, vp, vp]
        L.ks_count_updated_voxels.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.ks_download_updated_voxels.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ks_upload_blocks.argtypes = [vp, vp, C.c_size_t, vp, vp]
        L.ks_host_alloc.argtypes = [C.c_size_t]
        L.ks_host_alloc.restype = C.c_void_p
        L.ks_host_free.argtypes = [vp]
        L.ks_host_free.restype = None
        L.ks_get_tile_keys.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ks_export_tiles_device.argtypes = [vp, vp, C.c_size_t, vp]
        L.ks_merge_tiles_device.argtypes = [vp, vp, C.c_size_t, vp]
        L.ks_clear.argtypes = [vp]
        L.ks_clear_voxels.argtypes = [vp]
        L.ks_reset_tiles.argtypes = [vp, vp, C.c_size_t]
        L.ks_tile_owner.argtypes = [C.c_uint64, C.c_int]
        L.ks_reduce.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(KsReduceStats)]
        L.ks_debug_radix_sort.argtypes = [vp, vp, vp, C.c_size_t, C.c_int, C.c_uint]
        L.ks_debug_radix_sort_range.argtypes = [vp, vp, vp, C.c_size_t, C.c_int, C.c_uint, C.c_uint]
        L.ks_debug_radix_sort_batch.argtypes = [vp, vp, vp, vp, C.c_int, C.c_size_t, C.c_uint, C.c_uint]
        L.ks_synchronize.argtypes = [vp]
        L.ks_flush.argtypes = [vp, C.POINTER(KsFrameStats)]
        L.ks_stream.argtypes = [vp]
        L.ks_stream.restype = vp
        L.ks_profile_enable.argtypes = [vp, C.c_int]
        L.ks_profile_get.argtypes = [vp, C.POINTER(KsProfile), C.c_int]
        L.ks_early_out_iterations.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.ks_early_out_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.ks_pipeline_shape.argtypes = [vp, C.POINTER(C.c_int32)]
        L.ks_stream_plan.argtypes = [vp, C.POINTER(C.c_int32)]
        L.ks_tail_batch_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.ks_tail_batch_rule.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_int32, C.c_int32, C.c_int32, C.c_uint64]
        L.ks_seed_launch_shape.argtypes = [C.c_int32, C.c_int32, C.c_uint64, C.POINTER(C.c_uint32), C.c_int32]
        L.ks_update_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.ks_integrate_round_exact.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_uint64, vp, vp, vp, vp, C.c_size_t, C.c_int, C.POINTER(KsRoundStats)]
        L.ks_mesh_default_config.argtypes = [C.POINTER(KsMeshConfig)]
        L.ks_mesh_update.argtypes = [vp, C.POINTER(KsMeshConfig), C.POINTER(KsMeshStats)]
        L.ks_mesh_size.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.ks_mesh_download.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, vp, C.c_size_t]
        L.ks_mesh_changed_blocks.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ks_esdf_default_config.argtypes = [C.POINTER(KsEsdfConfig)]
        L.ks_esdf_update.argtypes = [vp, C.POINTER(KsEsdfConfig), C.POINTER(KsEsdfStats)]
        L.ks_esdf_download_blocks.argtypes = [vp, vp, C.c_size_t, vp]
        L.ks_esdf_query.argtypes = [vp, vp, C.c_size_t, vp, vp, vp]
        L.ks_esdf_refresh.argtypes = [vp, C.c_uint64, C.POINTER(KsEsdfRefreshStats)]
        L.ks_esdf_changed_blocks.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        for name in ("ks_esdf_sample", "ks_esdf_sample_device"):
            getattr(L, name).argtypes = [vp, vp, C.c_size_t, vp, vp, vp, vp, vp, C.POINTER(KsEsdfSampleStats)]
        for name in ("ks_esdf_slice", "ks_esdf_slice_device"):
            getattr(L, name).argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.POINTER(KsEsdfSampleStats)]
        L.ks_esdf_sweep_default_config.argtypes = [C.POINTER(KsEsdfSweepConfig)]
        for name in ("ks_esdf_sweep", "ks_esdf_sweep_device"):
            getattr(L, name).argtypes = [vp, vp, C.c_size_t, C.POINTER(KsEsdfSweepConfig), vp, vp, vp, vp, C.POINTER(KsEsdfSweepStats)]
        L.ks_render_default_config.argtypes = [C.POINTER(KsRenderConfig)]
        L.ks_render_view.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.POINTER(KsRenderConfig), vp, vp, vp, vp, C.POINTER(KsRenderStats)]
        L.ks_render_view_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.POINTER(KsRenderConfig), vp, vp, vp, vp, C.POINTER(KsRenderStats)]
        L.ks_align_default_config.argtypes = [C.POINTER(KsAlignConfig)]
        L.ks_align_points.argtypes = [vp, vp, vp, C.c_size_t, C.POINTER(KsAlignConfig), vp, C.POINTER(KsAlignStats)]
        L.ks_align_points_device.argtypes = [vp, vp, vp, C.c_size_t, C.POINTER(KsAlignConfig), vp, C.POINTER(KsAlignStats)]
        L.ks_objects_default_config.argtypes = [C.POINTER(KsObjectsConfig)]
        L.ks_objects_update.argtypes = [vp, C.POINTER(KsObjectsConfig), C.POINTER(KsObjectsStats)]
        L.ks_objects_size.argtypes = [vp, C.POINTER(C.c_size_t)]
        L.ks_objects_download.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ks_objects_download_blocks.argtypes = [vp, vp, C.c_size_t, vp]
        L.ks_objects_query.argtypes = [vp, vp, C.c_size_t, vp]
        L.ks_remove_blocks.argtypes = [vp, vp, C.c_size_t, C.POINTER(KsRemoveStats)]
        L.ks_remove_distant_blocks.argtypes = [vp, vp, C.c_float, C.POINTER(KsRemoveStats)]
        L.ks_removed_blocks.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ks_fuse_default_config.argtypes = [C.POINTER(KsFuseConfig)]
        L.ks_fuse_map.argtypes = [vp, vp, vp, C.POINTER(KsFuseConfig), C.POINTER(KsFuseStats)]
        L.ks_mesh_index.argtypes = [vp, C.POINTER(KsMeshIndexStats)]
        L.ks_mesh_index_size.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.ks_mesh_index_download.argtypes = [vp, vp, vp, vp, vp, vp, C.c_size_t, vp, C.c_size_t]
        L.ks_frontiers_default_config.argtypes = [C.POINTER(KsFrontierConfig)]
        L.ks_frontiers_update.argtypes = [vp, C.POINTER(KsFrontierConfig), C.POINTER(KsFrontierStats)]
        L.ks_frontiers_size.argtypes = [vp, C.POINTER(C.c_size_t)]
        L.ks_frontiers_download.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ks_frontiers_download_blocks.argtypes = [vp, vp, C.c_size_t, vp]
        L.ks_frontiers_query.argtypes = [vp, vp, C.c_size_t, vp]
        L.ks_rooms_default_config.argtypes = [C.POINTER(KsRoomsConfig)]
        L.ks_rooms_update.argtypes = [vp, C.POINTER(KsRoomsConfig), C.POINTER(KsRoomsStats)]
        L.ks_rooms_size.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.ks_rooms_download.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ks_rooms_links_download.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ks_rooms_objects.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ks_rooms_download_blocks.argtypes = [vp, vp, C.c_size_t, vp, vp]
        L.ks_rooms_query.argtypes = [vp, vp, C.c_size_t, vp]
        L.ks_view_gain_default_config.argtypes = [C.POINTER(KsViewGainConfig)]
        for name in ("ks_view_gain", "ks_view_gain_device"):
            getattr(L, name).argtypes = [vp, vp, C.c_size_t, C.POINTER(KsViewGainConfig), vp, C.POINTER(KsViewGainStats)]
        L.ks_path_shorten_default_config.argtypes = [C.POINTER(KsPathShortenConfig)]
        for name in ("ks_path_shorten", "ks_path_shorten_device"):
            getattr(L, name).argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, C.POINTER(KsPathShortenConfig), vp, vp, vp, vp, vp, C.POINTER(KsPathShortenStats)]
        L.ks_nav_default_config.argtypes = [C.POINTER(KsNavConfig)]
        L.ks_nav_update.argtypes = [vp, vp, C.c_size_t, C.POINTER(KsNavConfig), C.POINTER(KsNavStats)]
        for name in ("ks_nav_query", "ks_nav_query_device", "ks_nav_download_blocks"):
            getattr(L, name).argtypes = [vp, vp, C.c_size_t, vp]
        for name in ("ks_nav_paths", "ks_nav_paths_device"):
            getattr(L, name).argtypes = [vp, vp, C.c_size_t, C.c_uint32, vp, vp, vp, vp, C.POINTER(KsNavPathStats)]
        _lib = L
    return _lib


def default_config(**overrides) -> KsConfig:
    cfg = KsConfig()
    lib().ks_default_config(C.byref(cfg))
    apply_overrides(cfg, **overrides)
    return cfg


def apply_overrides(cfg, **overrides):
    for k, v in overrides.items():
        if k == "dynamic_labels":
            cfg.n_dynamic_labels = len(v)
            for i, lab in enumerate(v):
                cfg.dynamic_labels[i] = int(lab)
        elif k == "label_rgba":
            arr = np.ascontiguousarray(np.asarray(v, dtype=np.uint8).reshape(256, 4))
            C.memmove(cfg.label_rgba, arr.ctypes.data, 1024)
        else:
            if not hasattr(cfg, k):
                raise AttributeError(k)
            setattr(cfg, k, v)
    return cfg


class KsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"ks error {code}: {msg}")
        self.code = code


def _ptr(a):
    return None if a is None else a.ctypes.data


class HipIntegrator:
    """Thin RAII wrapper of ks_ctx."""

    def __init__(self, cfg: KsConfig):
        self.cfg = cfg
        self.vps = cfg.voxels_per_side
        self._h = C.c_void_p()
        rc = lib().ks_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            raise KsError(rc, lib().ks_last_error(None).decode())

    def _chk(self, rc):
        if rc != 0:
            raise KsError(rc, lib().ks_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            lib().ks_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_color_to_label(self, rgba_keys, labels):
        k = np.ascontiguousarray(rgba_keys, dtype=np.uint8).reshape(-1, 4)
        l = np.ascontiguousarray(labels, dtype=np.uint8)
        self._chk(lib().ks_set_color_to_label(self._h, _ptr(k), _ptr(l), len(l)))

    def integrate(self, T_G_C, xyz, rgba, labels, freespace=False) -> KsFrameStats:
        T = np.ascontiguousarray(T_G_C, dtype=np.float32)
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        labels = None if labels is None else np.ascontiguousarray(labels, dtype=np.uint8)
        rgba = None if rgba is None else np.ascontiguousarray(rgba, dtype=np.uint8)
        st = KsFrameStats()
        self._chk(lib().ks_integrate_points(self._h, _ptr(T), _ptr(xyz), _ptr(rgba), _ptr(labels), xyz.shape[0],
                                            int(freespace), C.byref(st)))
        return st

    def integrate_depth(self, T_G_C, depth, K, label_img=None, rgba_img=None, freespace=False) -> KsFrameStats:
        """depth: [H,W] float32 metres or uint16 millimetres; K = (fx, fy, cx, cy)."""
        T = np.ascontiguousarray(T_G_C, dtype=np.float32)
        depth = np.ascontiguousarray(depth)
        fmt = 0 if depth.dtype == np.float32 else 1
        assert depth.dtype in (np.float32, np.uint16)
        Kc = np.ascontiguousarray(K, dtype=np.float32)
        lab = None if label_img is None else np.ascontiguousarray(label_img, dtype=np.uint8)
        col = None if rgba_img is None else np.ascontiguousarray(rgba_img, dtype=np.uint8)
        st = KsFrameStats()
        self._chk(lib().ks_integrate_depth(self._h, _ptr(T), _ptr(depth), fmt, _ptr(lab), _ptr(col), depth.shape[1],
                                           depth.shape[0], _ptr(Kc), int(freespace), C.byref(st)))
        return st

    def integrate_depth_device(self, T_G_C, d_depth: int, fmt: int, d_label_img: int, d_rgba_img: int, width: int,
                               height: int, K, freespace=False) -> KsFrameStats:
        """Raw device addresses (e.g. torch.Tensor.data_ptr()); fmt 0 = f32 metres, 1 = u16 mm."""
        T = np.ascontiguousarray(T_G_C, dtype=np.float32)
        Kc = np.ascontiguousarray(K, dtype=np.float32)
        st = KsFrameStats()
        self._chk(lib().ks_integrate_depth_device(self._h, _ptr(T), d_depth or None, fmt, d_label_img or None,
                                                  d_rgba_img or None, width, height, _ptr(Kc), int(freespace), C.byref(st)))
        return st

    def integrate_device(self, T_G_C, d_xyz: int, d_rgba: int, d_labels: int, n: int, freespace=False) -> KsFrameStats:
        """d_* are raw device addresses (e.g. torch.Tensor.data_ptr()); 0/None = NULL."""
        T = np.ascontiguousarray(T_G_C, dtype=np.float32)
        st = KsFrameStats()
        self._chk(lib().ks_integrate_points_device(self._h, _ptr(T), d_xyz or None, d_rgba or None, d_labels or None, n,
                                                   int(freespace), C.byref(st)))
        return st

    def block_indices(self) -> np.ndarray:
        n = C.c_size_t()
        self._chk(lib().ks_get_block_indices(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 3), dtype=np.int32)
        if n.value:
            self._chk(lib().ks_get_block_indices(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def updated_block_indices(self, reset=True) -> np.ndarray:
        n = C.c_size_t()
        self._chk(lib().ks_get_updated_block_indices(self._h, None, 0, C.byref(n), 0))
        out = np.zeros((n.value, 3), dtype=np.int32)
        self._chk(lib().ks_get_updated_block_indices(self._h, _ptr(out), n.value, C.byref(n), int(reset)))
        return out

    def download(self, indices=None):
        if indices is None:
            indices = self.block_indices()
        indices = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1, 3)
        nv = self.vps ** 3
        t = np.zeros((len(indices), nv), dtype=TSDF_DTYPE)
        s = np.zeros((len(indices), nv), dtype=SEM_DTYPE)
        if len(indices):
            self._chk(lib().ks_download_blocks(self._h, _ptr(indices), len(indices), _ptr(t), _ptr(s)))
        return indices, t, s

    def upload(self, indices, tsdf=None, sem=None):
        """Seed / overwrite host-layout blocks in the GPU map (inverse of download)."""
        indices = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1, 3)
        nv = self.vps ** 3
        tp = sp = None
        if tsdf is not None:
            tsdf = np.ascontiguousarray(tsdf, dtype=TSDF_DTYPE).reshape(len(indices), nv)
            tp = _ptr(tsdf)
        if sem is not None:
            sem = np.ascontiguousarray(sem, dtype=SEM_DTYPE).reshape(len(indices), nv)
            sp = _ptr(sem)
        self._chk(lib().ks_upload_blocks(self._h, _ptr(indices), len(indices), tp, sp))

    def mesh(self, only_stale=False, min_weight=1e-4):
        """Extracts (or, only_stale, refreshes) the semantic mesh on the device and fetches it: kimera_semantics_amd.mesh.Mesh
        with blocks (MESH_BLOCK_DTYPE, ascending), xyz / normals (N, 3) f32, rgba (N, 4) u8, labels (N,) u8, stats (dict).
        Three vertices per triangle; the order is part of the ABI (ks_mesh_update in include/ks_hip.h)."""
        from .mesh import Mesh
        mc, st = KsMeshConfig(float(min_weight), int(bool(only_stale))), KsMeshStats()
        self._chk(lib().ks_mesh_update(self._h, C.byref(mc), C.byref(st)))
        nb, nv = C.c_size_t(), C.c_size_t()
        self._chk(lib().ks_mesh_size(self._h, C.byref(nb), C.byref(nv)))
        blocks = np.zeros(nb.value, dtype=MESH_BLOCK_DTYPE)
        xyz, normals = np.zeros((nv.value, 3), np.float32), np.zeros((nv.value, 3), np.float32)
        rgba, labels = np.zeros((nv.value, 4), np.uint8), np.zeros(nv.value, np.uint8)
        self._chk(lib().ks_mesh_download(self._h, _ptr(blocks), nb.value, _ptr(xyz), _ptr(normals), _ptr(rgba), _ptr(labels), nv.value))
        return Mesh(blocks, xyz, normals, rgba, labels, {k: int(getattr(st, k)) for k, _ in KsMeshStats._fields_})

    def mesh_index(self, build=True):
        """Builds the indexed view of the STORED mesh on the device (ks_mesh_index: shared vertices, a smooth normal and the object
        id per vertex) and fetches it: kimera_semantics_amd.mesh.IndexedMesh.  mesh() must have run; the index is a snapshot that
        the next mesh() or clear() drops.  `blocks` is the directory of the stored mesh: first_vertex / n_vertices address `indices`.
        build=False fetches the index that is stored (stats all zero)."""
        from .mesh import IndexedMesh
        st = KsMeshIndexStats()
        if build:
            self._chk(lib().ks_mesh_index(self._h, C.byref(st)))
        nv, ni, nb, nc = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._chk(lib().ks_mesh_index_size(self._h, C.byref(nv), C.byref(ni)))
        self._chk(lib().ks_mesh_size(self._h, C.byref(nb), C.byref(nc)))
        blocks = np.zeros(nb.value, dtype=MESH_BLOCK_DTYPE)
        self._chk(lib().ks_mesh_download(self._h, _ptr(blocks), nb.value, None, None, None, None, 0))
        xyz, normals = np.zeros((nv.value, 3), np.float32), np.zeros((nv.value, 3), np.float32)
        rgba, labels = np.zeros((nv.value, 4), np.uint8), np.zeros(nv.value, np.uint8)
        object_ids, indices = np.zeros(nv.value, np.uint32), np.zeros(ni.value, np.uint32)
        self._chk(lib().ks_mesh_index_download(self._h, _ptr(xyz), _ptr(normals), _ptr(rgba), _ptr(labels), _ptr(object_ids), nv.value,
                                               _ptr(indices), ni.value))
        return IndexedMesh(blocks, xyz, normals, rgba, labels, object_ids, indices, {k: int(getattr(st, k)) for k, _ in KsMeshIndexStats._fields_})

    def mesh_changed_blocks(self) -> np.ndarray:
        """Blocks whose segment the last mesh() replaced (including ones that are empty now), ascending."""
        n = C.c_size_t()
        self._chk(lib().ks_mesh_changed_blocks(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 3), dtype=np.int32)
        if n.value:
            self._chk(lib().ks_mesh_changed_blocks(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def esdf_update(self, region=None, **cfg) -> dict:
        """ks_esdf_update: computes the batch ESDF of the map as it is now and stores it on the device.  cfg: min_weight,
        min_distance_m, max_distance_m, max_workspace_bytes; region = (block_min[3], block_max[3]), inclusive.  Returns the
        stats; a KsError raised here carries them too (stats: the work space a refused call would have needed)."""
        ec, st = KsEsdfConfig(), KsEsdfStats()
        lib().ks_esdf_default_config(C.byref(ec))
        for k, v in cfg.items():
            if k not in ("min_weight", "min_distance_m", "max_distance_m", "max_workspace_bytes"):
                raise AttributeError(k)
            setattr(ec, k, v)
        if region is not None:
            ec.use_region = 1
            for a in range(3):
                ec.region_min[a], ec.region_max[a] = int(region[0][a]), int(region[1][a])
        rc = lib().ks_esdf_update(self._h, C.byref(ec), C.byref(st))
        stats = {k: ([int(v) for v in getattr(st, k)] if k == "box_voxels" else int(getattr(st, k))) for k, _ in KsEsdfStats._fields_}
        if rc != 0:
            err = KsError(rc, lib().ks_last_error(self._h).decode())
            err.stats = stats
            raise err
        return stats

    def esdf(self, region=None, **cfg):
        """Batch ESDF with nearest-surface labels of the whole map: (block_indices (N, 3) i32 ascending, records (N, vps^3)
        ESDF_DTYPE in host block layout, stats).  The contract is DESIGN.md, section "ESDF"."""
        stats = self.esdf_update(region=region, **cfg)
        idx = self.block_indices()
        return idx, self.esdf_blocks(idx), stats

    def esdf_refresh(self, max_workspace_bytes=0) -> dict:
        """ks_esdf_refresh: brings the stored ESDF up to date with the map, recomputing only the tiles that the tiles written
        since the last update or refresh can reach; it uses the configuration of the update that made the store.
        max_workspace_bytes 0: that update's.  Returns the stats; a KsError raised here carries them too."""
        st = KsEsdfRefreshStats()
        rc = lib().ks_esdf_refresh(self._h, int(max_workspace_bytes), C.byref(st))
        stats = {k: int(getattr(st, k)) for k, _ in KsEsdfRefreshStats._fields_}
        if rc != 0:
            err = KsError(rc, lib().ks_last_error(self._h).decode())
            err.stats = stats
            raise err
        return stats

    def esdf_changed_blocks(self) -> np.ndarray:
        """Blocks that hold a tile the last esdf_refresh() recomputed, ascending; empty after an esdf_update()."""
        n = C.c_size_t()
        self._chk(lib().ks_esdf_changed_blocks(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 3), dtype=np.int32)
        if n.value:
            self._chk(lib().ks_esdf_changed_blocks(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def esdf_blocks(self, indices) -> np.ndarray:
        """Records of the stored ESDF (as of the last esdf() / esdf_update() / esdf_refresh()) for host-layout blocks."""
        indices = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1, 3)
        out = np.zeros((len(indices), self.vps ** 3), dtype=ESDF_DTYPE)
        self._chk(lib().ks_esdf_download_blocks(self._h, _ptr(indices), len(indices), _ptr(out)))
        return out

    def esdf_query(self, xyz) -> np.ndarray:
        """The stored record of the voxel that contains each world point (nearest voxel, no interpolation): (n,) ESDF_DTYPE."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        n = len(xyz)
        d, f, l = np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        self._chk(lib().ks_esdf_query(self._h, _ptr(xyz), n, _ptr(d), _ptr(f), _ptr(l)))
        out = np.zeros(n, dtype=ESDF_DTYPE)
        out["distance"], out["flags"], out["label"] = d, f, l
        return out

    @staticmethod
    def _stats_dict(st) -> dict:
        return {k: int(getattr(st, k)) for k, _ in st._fields_}

    def esdf_sample(self, xyz, outputs=("distance", "gradient", "status", "label", "flags"), stats=True) -> dict:
        """ks_esdf_sample: the trilinear sample E(p) of the STORED ESDF at world points xyz (n, 3).  Returns a dict of the asked
        outputs — distance (n,) f32 (NaN where unknown), gradient (n, 3) f32, status / label / flags (n,) u8 — plus "stats".
        The contract is DESIGN.md, section "ESDF reads"."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        out = self._esdf_sample_arrays((len(xyz),), outputs)
        st = KsEsdfSampleStats()
        self._chk(lib().ks_esdf_sample(self._h, _ptr(xyz), len(xyz), *[_ptr(out.get(k)) for k in self._ESDF_SAMPLE_OUTPUTS],
                                       C.byref(st) if stats else None))
        out["stats"] = self._stats_dict(st) if stats else None
        return out

    _ESDF_SAMPLE_OUTPUTS = ("distance", "gradient", "status", "label", "flags")

    @classmethod
    def _esdf_sample_arrays(cls, shape, outputs) -> dict:
        for k in outputs:
            if k not in cls._ESDF_SAMPLE_OUTPUTS:
                raise AttributeError(k)
        # (filled with a pattern no result has, so that an element the library did not write shows)
        make = {"distance": lambda: np.full(shape, -7.0, np.float32), "gradient": lambda: np.full(shape + (3,), -7.0, np.float32)}
        return {k: make.get(k, lambda: np.full(shape, 0xee, np.uint8))() for k in outputs}

    def esdf_sample_device(self, d_xyz: int, n: int, d_distance: int = 0, d_gradient: int = 0, d_status: int = 0, d_label: int = 0,
                           d_flags: int = 0, stats=True):
        """ks_esdf_sample_device: raw device addresses (e.g. torch.Tensor.data_ptr()); 0 / None = not wanted.  The kernel is
        enqueued on self.stream; with stats=False the host does not wait for it and None is returned."""
        st = KsEsdfSampleStats()
        self._chk(lib().ks_esdf_sample_device(self._h, d_xyz or None, int(n), d_distance or None, d_gradient or None, d_status or None,
                                              d_label or None, d_flags or None, C.byref(st) if stats else None))
        return self._stats_dict(st) if stats else None

    def esdf_slice(self, origin, du, dv, width, height, outputs=("distance", "gradient", "status", "label", "flags"), stats=True) -> dict:
        """ks_esdf_slice: E at (origin + i du) + j dv for the pixels (i, j) of a width x height image: a dict of (H, W[, 3]) arrays
        as esdf_sample returns them, plus "stats"."""
        o, u, v = (np.ascontiguousarray(a, dtype=np.float32).reshape(3) for a in (origin, du, dv))
        w, h = int(width), int(height)
        out = self._esdf_sample_arrays((max(h, 0), max(w, 0)), outputs)
        st = KsEsdfSampleStats()
        self._chk(lib().ks_esdf_slice(self._h, _ptr(o), _ptr(u), _ptr(v), w, h, *[_ptr(out.get(k)) for k in self._ESDF_SAMPLE_OUTPUTS],
                                      C.byref(st) if stats else None))
        out["stats"] = self._stats_dict(st) if stats else None
        return out

    def esdf_slice_device(self, origin, du, dv, width, height, d_distance: int = 0, d_gradient: int = 0, d_status: int = 0,
                          d_label: int = 0, d_flags: int = 0, stats=True):
        """ks_esdf_slice_device: as esdf_sample_device."""
        o, u, v = (np.ascontiguousarray(a, dtype=np.float32).reshape(3) for a in (origin, du, dv))
        st = KsEsdfSampleStats()
        self._chk(lib().ks_esdf_slice_device(self._h, _ptr(o), _ptr(u), _ptr(v), int(width), int(height), d_distance or None, d_gradient or None,
                                             d_status or None, d_label or None, d_flags or None, C.byref(st) if stats else None))
        return self._stats_dict(st) if stats else None

    def esdf_sweep_config(self, **cfg) -> KsEsdfSweepConfig:
        sc = KsEsdfSweepConfig()
        lib().ks_esdf_sweep_default_config(C.byref(sc))
        for k, v in cfg.items():
            if k not in [f for f, _ in KsEsdfSweepConfig._fields_]:
                raise AttributeError(k)
            if v is not None:
                setattr(sc, k, v)
        return sc

    _ESDF_SWEEP_OUTPUTS = ("status", "t_stop", "min_clearance", "t_min")

    def esdf_sweep(self, segments, outputs=("status", "t_stop", "min_clearance", "t_min"), stats=True, **cfg) -> dict:
        """ks_esdf_sweep: segments (n, 6) {a, b} against a sphere of radius_m over the STORED ESDF.  Returns a dict of status (n,)
        u8 (KS_SWEEP_*), t_stop / min_clearance / t_min (n,) f32, plus "stats"; cfg are the fields of KsEsdfSweepConfig."""
        seg = np.ascontiguousarray(segments, dtype=np.float32).reshape(-1, 6)
        for k in outputs:
            if k not in self._ESDF_SWEEP_OUTPUTS:
                raise AttributeError(k)
        out = {k: (np.full(len(seg), 0xee, np.uint8) if k == "status" else np.full(len(seg), -7.0, np.float32)) for k in outputs}
        sc, st = self.esdf_sweep_config(**cfg), KsEsdfSweepStats()
        self._chk(lib().ks_esdf_sweep(self._h, _ptr(seg), len(seg), C.byref(sc), *[_ptr(out.get(k)) for k in self._ESDF_SWEEP_OUTPUTS],
                                      C.byref(st) if stats else None))
        out["stats"] = self._stats_dict(st) if stats else None
        return out

    def esdf_sweep_device(self, d_segments: int, n: int, d_status: int = 0, d_t_stop: int = 0, d_min_clearance: int = 0, d_t_min: int = 0,
                          stats=True, **cfg):
        """ks_esdf_sweep_device: as esdf_sample_device."""
        sc, st = self.esdf_sweep_config(**cfg), KsEsdfSweepStats()
        self._chk(lib().ks_esdf_sweep_device(self._h, d_segments or None, int(n), C.byref(sc), d_status or None, d_t_stop or None,
                                             d_min_clearance or None, d_t_min or None, C.byref(st) if stats else None))
        return self._stats_dict(st) if stats else None

    def render_config(self, **cfg) -> KsRenderConfig:
        rc = KsRenderConfig()
        lib().ks_render_default_config(C.byref(rc))
        for k, v in cfg.items():
            if k not in ("min_weight", "min_range_m", "max_range_m"):
                raise AttributeError(k)
            if v is not None:
                setattr(rc, k, v)
        return rc

    def render(self, T_G_C, K, width, height, min_weight=None, min_range_m=None, max_range_m=None, normals=True):
        """ks_render_view: the map seen from the camera pose T_G_C with intrinsics K = (fx, fy, cx, cy).  Returns
        (depth (H, W) f32 z-depth, NaN at a miss; labels (H, W) u8, 255 at a miss; rgba (H, W, 4) u8; normals (H, W, 3) f32 in
        the world frame, or None with normals=False; stats dict).  The contract is DESIGN.md, section "View rendering"."""
        T = np.ascontiguousarray(T_G_C, dtype=np.float32)
        Kc = np.ascontiguousarray(K, dtype=np.float32)
        rc, st = self.render_config(min_weight=min_weight, min_range_m=min_range_m, max_range_m=max_range_m), KsRenderStats()
        w, h = int(width), int(height)
        shape = (max(h, 0), max(w, 0))
        depth, labels, rgba = np.zeros(shape, np.float32), np.zeros(shape, np.uint8), np.zeros(shape + (4,), np.uint8)
        nrm = np.zeros(shape + (3,), np.float32) if normals else None
        self._chk(lib().ks_render_view(self._h, _ptr(T), _ptr(Kc), w, h, C.byref(rc), _ptr(depth), _ptr(labels), _ptr(rgba), _ptr(nrm), C.byref(st)))
        return depth, labels, rgba, nrm, {k: int(getattr(st, k)) for k, _ in KsRenderStats._fields_}

    def render_device(self, T_G_C, K, width, height, d_depth: int, d_labels: int, d_rgba: int, d_normals: int, stats=True, **cfg):
        """ks_render_view_device: raw device addresses (e.g. torch.Tensor.data_ptr()); 0 / None = not wanted.  The kernel is
        enqueued on self.stream; with stats=False the host does not wait for it and None is returned."""
        T = np.ascontiguousarray(T_G_C, dtype=np.float32)
        Kc = np.ascontiguousarray(K, dtype=np.float32)
        rc, st = self.render_config(**cfg), KsRenderStats()
        self._chk(lib().ks_render_view_device(self._h, _ptr(T), _ptr(Kc), int(width), int(height), C.byref(rc), d_depth or None, d_labels or None,
                                              d_rgba or None, d_normals or None, C.byref(st) if stats else None))
        return {k: int(getattr(st, k)) for k, _ in KsRenderStats._fields_} if stats else None

    def align_config(self, **cfg) -> KsAlignConfig:
        ac = KsAlignConfig()
        lib().ks_align_default_config(C.byref(ac))
        for k, v in cfg.items():
            if k not in [f for f, _ in KsAlignConfig._fields_]:
                raise AttributeError(k)
            if v is not None:
                setattr(ac, k, v)
        return ac

    @staticmethod
    def _align_stats(st) -> dict:
        return {k: (float if k.startswith("rmse") else int)(getattr(st, k)) for k, _ in KsAlignStats._fields_}

    def align(self, T_G_C, xyz, **cfg):
        """ks_align_points: refines the pose T_G_C of the cloud xyz (n, 3; camera frame) against the TSDF of the map.  Returns
        (T_out (7,) f32, stats dict); a status other than KS_ALIGN_CONVERGED is no error.  The contract is DESIGN.md, section
        "Scan alignment"; cfg are the fields of KsAlignConfig."""
        T = np.ascontiguousarray(T_G_C, dtype=np.float32)
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        ac, st, out = self.align_config(**cfg), KsAlignStats(), np.zeros(7, np.float32)
        self._chk(lib().ks_align_points(self._h, _ptr(T), _ptr(xyz), len(xyz), C.byref(ac), _ptr(out), C.byref(st)))
        return out, self._align_stats(st)

    def align_device(self, T_G_C, d_xyz: int, n: int, **cfg):
        """ks_align_points_device: the cloud at the raw device address d_xyz (e.g. torch.Tensor.data_ptr()), read on self.stream."""
        T = np.ascontiguousarray(T_G_C, dtype=np.float32)
        ac, st, out = self.align_config(**cfg), KsAlignStats(), np.zeros(7, np.float32)
        self._chk(lib().ks_align_points_device(self._h, _ptr(T), d_xyz or None, int(n), C.byref(ac), _ptr(out), C.byref(st)))
        return out, self._align_stats(st)

    def objects_config(self, **cfg) -> KsObjectsConfig:
        oc = KsObjectsConfig()
        lib().ks_objects_default_config(C.byref(oc))
        for k, v in cfg.items():
            if k not in [f for f, _ in KsObjectsConfig._fields_]:
                raise AttributeError(k)
            if v is not None:
                setattr(oc, k, v)
        return oc

    def objects(self, **cfg):
        """ks_objects_update + ks_objects_download: clusters the surface voxels of every label into 26-connected components and
        returns (records (n,) OBJECT_DTYPE ascending by first_voxel, stats dict).  cfg are the fields of KsObjectsConfig.  The
        contract is DESIGN.md, section "Object instances"; object_ids() / object_query() read the per-voxel ids it stores."""
        oc, st = self.objects_config(**cfg), KsObjectsStats()
        self._chk(lib().ks_objects_update(self._h, C.byref(oc), C.byref(st)))
        return self.object_records(), {k: int(getattr(st, k)) for k, _ in KsObjectsStats._fields_}

    def object_records(self) -> np.ndarray:
        """The records of the last objects() call."""
        n = C.c_size_t()
        self._chk(lib().ks_objects_size(self._h, C.byref(n)))
        out = np.zeros(n.value, dtype=OBJECT_DTYPE)
        self._chk(lib().ks_objects_download(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def object_ids(self, block_idx) -> np.ndarray:
        """(N, vps^3) u32 in host block layout: the index of each voxel's object in the records of the last objects() call, or
        KS_OBJECT_NONE."""
        indices = np.ascontiguousarray(block_idx, dtype=np.int32).reshape(-1, 3)
        out = np.zeros((len(indices), self.vps ** 3), dtype=np.uint32)
        self._chk(lib().ks_objects_download_blocks(self._h, _ptr(indices), len(indices), _ptr(out)))
        return out

    def object_query(self, xyz) -> np.ndarray:
        """(n,) u32: the object id of the voxel that contains each world point, or KS_OBJECT_NONE."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(len(xyz), dtype=np.uint32)
        self._chk(lib().ks_objects_query(self._h, _ptr(xyz), len(xyz), _ptr(out)))
        return out

    # ---- exploration frontiers over the stored ESDF (DESIGN.md, section "Exploration frontiers") ----
    def frontier_config(self, **cfg) -> KsFrontierConfig:
        fc = KsFrontierConfig()
        lib().ks_frontiers_default_config(C.byref(fc))
        for k, v in cfg.items():
            if k not in ("radius_m", "min_voxels", "use_bounds", "bounds_min", "bounds_max"):
                raise AttributeError(k)
            if v is None:
                continue
            if k in ("bounds_min", "bounds_max"):
                v = (C.c_int32 * 3)(*[int(a) for a in v])
            setattr(fc, k, v)
        return fc

    def frontiers(self, **cfg):
        """ks_frontiers_update + ks_frontiers_download: the traversable voxels of the STORED ESDF with an unobserved face neighbour,
        clustered into 26-connected components and joined with the stored navigation field, if there is one.  Returns (records (n,)
        FRONTIER_DTYPE ascending by first_voxel, stats dict).  cfg are the fields of KsFrontierConfig.  The contract is DESIGN.md,
        section "Exploration frontiers"; frontier_ids() / frontier_query() read the per-voxel ids it stores."""
        fc, st = self.frontier_config(**cfg), KsFrontierStats()
        self._chk(lib().ks_frontiers_update(self._h, C.byref(fc), C.byref(st)))
        return self.frontier_records(), {k: int(getattr(st, k)) for k, _ in KsFrontierStats._fields_}

    def frontier_records(self) -> np.ndarray:
        """The records of the last frontiers() call."""
        n = C.c_size_t()
        self._chk(lib().ks_frontiers_size(self._h, C.byref(n)))
        out = np.zeros(n.value, dtype=FRONTIER_DTYPE)
        self._chk(lib().ks_frontiers_download(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def frontier_ids(self, block_idx) -> np.ndarray:
        """(N, vps^3) u32 in host block layout: the index of each voxel's frontier in the records of the last frontiers() call, or
        KS_FRONTIER_NONE."""
        indices = np.ascontiguousarray(block_idx, dtype=np.int32).reshape(-1, 3)
        out = np.zeros((len(indices), self.vps ** 3), dtype=np.uint32)
        self._chk(lib().ks_frontiers_download_blocks(self._h, _ptr(indices), len(indices), _ptr(out)))
        return out

    def frontier_query(self, xyz) -> np.ndarray:
        """(n,) u32: the frontier id of the voxel that contains each world point, or KS_FRONTIER_NONE."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(len(xyz), dtype=np.uint32)
        self._chk(lib().ks_frontiers_query(self._h, _ptr(xyz), len(xyz), _ptr(out)))
        return out

    # ---- rooms over the stored ESDF (DESIGN.md, section "Rooms") ----
    def rooms_config(self, **cfg) -> KsRoomsConfig:
        rc = KsRoomsConfig()
        lib().ks_rooms_default_config(C.byref(rc))
        for k, v in cfg.items():
            if k not in [f for f, _ in KsRoomsConfig._fields_]:
                raise AttributeError(k)
            if v is None:
                continue
            if k in ("bounds_min", "bounds_max"):
                v = (C.c_int32 * 3)(*[int(a) for a in v])
            setattr(rc, k, v)
        return rc

    def rooms(self, **cfg):
        """ks_rooms_update + the two downloads: the free voxels of the STORED ESDF whose distance reaches core_distance_m clustered
        into rooms, every other free voxel handed to the room nearest through free space, the contacts between rooms as links, the
        stored objects joined.  Returns (records (n,) ROOM_DTYPE ascending by first_voxel, links (m,) ROOM_LINK_DTYPE ascending by
        (room_a, room_b), stats dict).  cfg are the fields of KsRoomsConfig.  The contract is DESIGN.md, section "Rooms";
        room_ids() / room_costs() / room_query() / room_objects() read what it stores."""
        rc, st = self.rooms_config(**cfg), KsRoomsStats()
        self._chk(lib().ks_rooms_update(self._h, C.byref(rc), C.byref(st)))
        return self.room_records(), self.room_links(), {k: int(getattr(st, k)) for k, _ in KsRoomsStats._fields_}

    def room_records(self) -> np.ndarray:
        """The records of the last rooms() call."""
        n = C.c_size_t()
        self._chk(lib().ks_rooms_size(self._h, C.byref(n), None))
        out = np.zeros(n.value, dtype=ROOM_DTYPE)
        self._chk(lib().ks_rooms_download(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def room_links(self) -> np.ndarray:
        """The links of the last rooms() call."""
        n = C.c_size_t()
        self._chk(lib().ks_rooms_size(self._h, None, C.byref(n)))
        out = np.zeros(n.value, dtype=ROOM_LINK_DTYPE)
        self._chk(lib().ks_rooms_links_download(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def room_objects(self) -> np.ndarray:
        """(n_objects,) u32: the room every object of the objects() result stored at the last rooms() call was joined to, or
        KS_ROOM_NONE; empty if no objects were stored then."""
        n = C.c_size_t()
        lib().ks_rooms_objects(self._h, None, 0, C.byref(n))          # (the count alone: refused as too small unless it is 0)
        out = np.zeros(n.value, dtype=np.uint32)
        self._chk(lib().ks_rooms_objects(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def _room_plane(self, block_idx, plane) -> np.ndarray:
        indices = np.ascontiguousarray(block_idx, dtype=np.int32).reshape(-1, 3)
        out = np.zeros((len(indices), self.vps ** 3), dtype=np.uint32)
        self._chk(lib().ks_rooms_download_blocks(self._h, _ptr(indices), len(indices), *((_ptr(out), None) if plane == 0 else (None, _ptr(out)))))
        return out

    def room_ids(self, block_idx) -> np.ndarray:
        """(N, vps^3) u32 in host block layout: the index of each voxel's room in the records of the last rooms() call, or KS_ROOM_NONE."""
        return self._room_plane(block_idx, 0)

    def room_costs(self, block_idx) -> np.ndarray:
        """(N, vps^3) u32 in host block layout: each voxel's cost to the nearest core of a room, KS_NAV_BLOCKED where the voxel is not
        free, KS_NAV_UNREACHED where it is unassigned."""
        return self._room_plane(block_idx, 1)

    def room_query(self, xyz) -> np.ndarray:
        """(n,) u32: the room of the voxel that contains each world point, or KS_ROOM_NONE."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(len(xyz), dtype=np.uint32)
        self._chk(lib().ks_rooms_query(self._h, _ptr(xyz), len(xyz), _ptr(out)))
        return out

    # ---- view information gain over the stored ESDF (DESIGN.md, section "View information gain") ----
    def view_gain_config(self, K, width=None, height=None, **cfg) -> KsViewGainConfig:
        vc = KsViewGainConfig()
        lib().ks_view_gain_default_config(C.byref(vc))
        vc.K = (C.c_float * 4)(*[float(a) for a in K])
        for k, v in dict(cfg, width=width, height=height).items():
            if k not in ("min_range_m", "max_range_m", "step_m", "stop_distance_m", "width", "height", "label", "max_workspace_bytes"):
                raise AttributeError(k)
            if v is not None:
                setattr(vc, k, v)
        return vc

    def view_gain(self, poses, K, width=None, height=None, **cfg):
        """ks_view_gain: for each candidate camera pose T_G_C (n, 7) the distinct unknown, free and surface voxels of the STORED ESDF
        that the rays of a width x height pinhole image with K = (fx, fy, cx, cy) visit before a surface stops them.  Returns
        (records (n,) VIEW_GAIN_DTYPE, stats dict).  cfg are the fields of KsViewGainConfig.  The contract is DESIGN.md, section
        "View information gain"."""
        T = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 7)
        vc, st = self.view_gain_config(K, width, height, **cfg), KsViewGainStats()
        out = np.zeros(len(T), dtype=VIEW_GAIN_DTYPE)
        self._chk(lib().ks_view_gain(self._h, _ptr(T), len(T), C.byref(vc), _ptr(out), C.byref(st)))
        return out, {k: int(getattr(st, k)) for k, _ in KsViewGainStats._fields_}

    def view_gain_device(self, d_poses: int, n: int, K, width=None, height=None, d_out: int = 0, stats=True, **cfg):
        """ks_view_gain_device: raw device addresses (e.g. torch.Tensor.data_ptr()) of n x 7 floats and n 32-byte records.  The
        kernels are enqueued on self.stream; with stats=False the host does not wait for them and None is returned."""
        vc, st = self.view_gain_config(K, width, height, **cfg), KsViewGainStats()
        self._chk(lib().ks_view_gain_device(self._h, d_poses or None, int(n), C.byref(vc), d_out or None, C.byref(st) if stats else None))
        return {k: int(getattr(st, k)) for k, _ in KsViewGainStats._fields_} if stats else None

    # ---- navigation field over the stored ESDF (DESIGN.md, section "Navigation field") ----
    def nav_config(self, **cfg) -> KsNavConfig:
        nc = KsNavConfig()
        lib().ks_nav_default_config(C.byref(nc))
        for k, v in cfg.items():
            if k not in ("radius_m", "max_cost", "max_rounds"):
                raise AttributeError(k)
            if v is not None:
                setattr(nc, k, v)
        return nc

    def nav_update(self, goals, radius_m=None, max_cost=None, max_rounds=None) -> dict:
        """ks_nav_update: the cost-to-go field of the STORED ESDF to the nearest of the world points goals (n, 3), through the voxels
        a sphere of radius_m may occupy.  Returns the statistics; the field stays on the device for nav_query / nav_blocks /
        nav_paths until the ESDF store or the map changes."""
        goals = np.ascontiguousarray(goals, dtype=np.float32).reshape(-1, 3)
        nc, st = self.nav_config(radius_m=radius_m, max_cost=max_cost, max_rounds=max_rounds), KsNavStats()
        self._chk(lib().ks_nav_update(self._h, _ptr(goals), len(goals), C.byref(nc), C.byref(st)))
        return self._stats_dict(st)

    def nav_query(self, xyz) -> np.ndarray:
        """(n,) u32: the cost of the voxel that contains each world point; KS_NAV_BLOCKED / KS_NAV_UNREACHED as in the field."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        out = np.full(len(xyz), 0xeeeeeeee, dtype=np.uint32)
        self._chk(lib().ks_nav_query(self._h, _ptr(xyz), len(xyz), _ptr(out)))
        return out

    def nav_query_device(self, d_xyz: int, n: int, d_cost: int) -> None:
        """ks_nav_query_device: raw device addresses (e.g. torch.Tensor.data_ptr()); enqueued on self.stream, the host does not wait."""
        self._chk(lib().ks_nav_query_device(self._h, d_xyz or None, int(n), d_cost or None))

    def nav_blocks(self, block_idx) -> np.ndarray:
        """(n, vps^3) u32: the field of host-layout blocks; KS_NAV_BLOCKED where a block or tile is not in the field."""
        indices = np.ascontiguousarray(block_idx, dtype=np.int32).reshape(-1, 3)
        out = np.full((len(indices), self.vps ** 3), 0xeeeeeeee, dtype=np.uint32)
        self._chk(lib().ks_nav_download_blocks(self._h, _ptr(indices), len(indices), _ptr(out)))
        return out

    _NAV_PATH_OUTPUTS = ("status", "cost", "n_waypoints", "waypoints")
    NAV_WAYPOINT_FILL = -7.0   # rows of `waypoints` from n_waypoints on keep this pattern: the library does not write them

    def nav_paths(self, starts, max_waypoints, outputs=("status", "cost", "n_waypoints", "waypoints"), stats=True) -> dict:
        """ks_nav_paths: a path per world point of starts (n, 3) by steepest descent of the stored field.  Returns a dict of status
        (n,) u8 (KS_NAV_PATH_*), cost (n,) u32, n_waypoints (n,) u32, waypoints (n, max_waypoints, 3) f32, plus "stats"."""
        starts = np.ascontiguousarray(starts, dtype=np.float32).reshape(-1, 3)
        n, mw = len(starts), max(int(max_waypoints), 0)
        for k in outputs:
            if k not in self._NAV_PATH_OUTPUTS:
                raise AttributeError(k)
        make = {"status": lambda: np.full(n, 0xee, np.uint8), "cost": lambda: np.full(n, 0xeeeeeeee, np.uint32),
                "n_waypoints": lambda: np.full(n, 0xeeeeeeee, np.uint32),
                "waypoints": lambda: np.full((n, min(mw, 65536), 3), self.NAV_WAYPOINT_FILL, np.float32)}
        out = {k: make[k]() for k in outputs}
        st = KsNavPathStats()
        self._chk(lib().ks_nav_paths(self._h, _ptr(starts), n, int(max_waypoints) & 0xffffffff, *[_ptr(out.get(k)) for k in self._NAV_PATH_OUTPUTS],
                                     C.byref(st) if stats else None))
        out["stats"] = self._stats_dict(st) if stats else None
        return out

    def nav_paths_device(self, d_starts: int, n: int, max_waypoints: int, d_status: int = 0, d_cost: int = 0, d_n_waypoints: int = 0,
                         d_waypoints: int = 0, stats=True):
        """ks_nav_paths_device: as esdf_sample_device."""
        st = KsNavPathStats()
        self._chk(lib().ks_nav_paths_device(self._h, d_starts or None, int(n), int(max_waypoints) & 0xffffffff, d_status or None, d_cost or None,
                                            d_n_waypoints or None, d_waypoints or None, C.byref(st) if stats else None))
        return self._stats_dict(st) if stats else None

    def path_shorten_config(self, **cfg) -> KsPathShortenConfig:
        pc = KsPathShortenConfig()
        lib().ks_path_shorten_default_config(C.byref(pc))
        for k, v in cfg.items():
            if k not in ("radius_m", "min_step_m", "unknown_is_free", "max_samples", "lookahead"):
                raise AttributeError(k)
            if v is not None:
                setattr(pc, k, v)
        return pc

    _SHORTEN_OUTPUTS = ("status", "n_waypoints", "waypoints", "length", "min_clearance")

    def shorten_paths(self, waypoints, n_waypoints, outputs=("status", "n_waypoints", "waypoints", "length", "min_clearance"), stats=True,
                      in_place=False, **cfg) -> dict:
        """ks_path_shorten: each path of waypoints (n, max_waypoints, 3) f32 / n_waypoints (n,) u32 (the layout nav_paths returns)
        pulled taut by line of sight over the STORED ESDF.  Returns a dict of status (n,) u8 (KS_SHORTEN_*), n_waypoints (n,) u32,
        waypoints (n, max_waypoints, 3) f32 whose rows from n_waypoints on keep NAV_WAYPOINT_FILL, length / min_clearance (n,) f32,
        plus "stats"; cfg are the fields of KsPathShortenConfig.  in_place: the library gets one array as input and output (a copy
        of `waypoints`, returned as "waypoints": rows from n_waypoints on then keep the input)."""
        wp = np.ascontiguousarray(waypoints, dtype=np.float32)
        assert wp.ndim == 3 and wp.shape[2] == 3, wp.shape
        nw = np.ascontiguousarray(n_waypoints, dtype=np.uint32).reshape(-1)
        n, mw = len(nw), wp.shape[1]
        assert wp.shape[0] == n
        for k in outputs:
            if k not in self._SHORTEN_OUTPUTS:
                raise AttributeError(k)
        if in_place:
            assert "waypoints" in outputs
            wp = wp.copy()
        make = {"status": lambda: np.full(n, 0xee, np.uint8), "n_waypoints": lambda: np.full(n, 0xeeeeeeee, np.uint32),
                "waypoints": lambda: wp if in_place else np.full((n, mw, 3), self.NAV_WAYPOINT_FILL, np.float32),
                "length": lambda: np.full(n, -7.0, np.float32), "min_clearance": lambda: np.full(n, -7.0, np.float32)}
        out = {k: make[k]() for k in outputs}
        pc, st = self.path_shorten_config(**cfg), KsPathShortenStats()
        self._chk(lib().ks_path_shorten(self._h, _ptr(wp), _ptr(nw), n, mw & 0xffffffff, C.byref(pc), *[_ptr(out.get(k)) for k in self._SHORTEN_OUTPUTS],
                                        C.byref(st) if stats else None))
        out["stats"] = self._stats_dict(st) if stats else None
        return out

    def shorten_paths_device(self, d_waypoints: int, d_n_waypoints: int, n: int, max_waypoints: int, d_status: int = 0, d_n_waypoints_out: int = 0,
                             d_waypoints_out: int = 0, d_length: int = 0, d_min_clearance: int = 0, stats=True, **cfg):
        """ks_path_shorten_device: raw device addresses (e.g. torch.Tensor.data_ptr()) on ks_stream; d_waypoints_out may equal
        d_waypoints.  With stats the call has waited for the kernel; without, it returns None and waits for nothing."""
        pc, st = self.path_shorten_config(**cfg), KsPathShortenStats()
        self._chk(lib().ks_path_shorten_device(self._h, d_waypoints or None, d_n_waypoints or None, int(n), int(max_waypoints) & 0xffffffff, C.byref(pc),
                                               d_status or None, d_n_waypoints_out or None, d_waypoints_out or None, d_length or None,
                                               d_min_clearance or None, C.byref(st) if stats else None))
        return self._stats_dict(st) if stats else None

    # ---- multi-GPU exchange primitives (used by kimera_semantics_amd.parallel) ----
    TILE_BYTES = 65536

    def tile_keys(self) -> np.ndarray:
        n = C.c_size_t()
        self._chk(lib().ks_get_tile_keys(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint64)
        if n.value:
            self._chk(lib().ks_get_tile_keys(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def export_tiles(self, slots: np.ndarray, d_payload: int):
        """Gathers the tiles at `slots` into the device buffer at address d_payload (len(slots) x 64 KiB)."""
        s = np.ascontiguousarray(slots, dtype=np.uint32)
        self._chk(lib().ks_export_tiles_device(self._h, _ptr(s), len(s), d_payload or None))

    def merge_tiles(self, keys: np.ndarray, d_payload: int):
        k = np.ascontiguousarray(keys, dtype=np.uint64)
        self._chk(lib().ks_merge_tiles_device(self._h, _ptr(k), len(k), d_payload or None))

    def download_updated_voxels(self):
        """Voxels written since the previous call: structured array (block [3] i32, linear u32, tsdf, sem)."""
        n, nr = C.c_size_t(), C.c_size_t()
        self._chk(lib().ks_count_updated_voxels(self._h, C.byref(n), C.byref(nr)))
        dt = np.dtype([("block", "<i4", (3,)), ("linear", "<u4"), ("tsdf", TSDF_DTYPE), ("sem", SEM_DTYPE)])
        rdt = np.dtype([("block", "<i4", (3,)), ("first", "<u4"), ("count", "<u4")])
        assert dt.itemsize == 120 and rdt.itemsize == 20
        out = np.zeros(n.value, dtype=dt)
        runs = np.zeros(nr.value, dtype=rdt)
        if n.value:
            m, mr = C.c_size_t(), C.c_size_t()
            self._chk(lib().ks_download_updated_voxels(self._h, _ptr(out), n.value, C.byref(m), _ptr(runs), nr.value, C.byref(mr)))
            assert m.value == n.value and mr.value == nr.value
            # every record belongs to exactly one run, and carries its run's block index
            assert int(runs["count"].sum()) == n.value
            for r in runs[:: max(1, len(runs) // 16)]:
                if r["count"]:
                    assert (out["block"][r["first"]:r["first"] + r["count"]] == r["block"]).all()
        return out

    def clear(self):
        self._chk(lib().ks_clear(self._h))

    def clear_voxels(self):
        """The map goes, the integrator's sets and counters stay (ks_clear_voxels)."""
        self._chk(lib().ks_clear_voxels(self._h))

    def remove_blocks(self, indices) -> dict:
        """ks_remove_blocks: takes the host-layout blocks `indices` (n, 3) out of the map (absent and repeated ones are ignored).
        Returns the stats; removed_blocks() lists what left.  The contract is DESIGN.md, section 16."""
        indices = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1, 3)
        st = KsRemoveStats()
        self._chk(lib().ks_remove_blocks(self._h, _ptr(indices) if len(indices) else None, len(indices), C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in KsRemoveStats._fields_}

    def remove_distant(self, center, max_distance_m) -> dict:
        """ks_remove_distant_blocks: removes every block whose ORIGIN is further than max_distance_m from `center` (the rule of
        Voxblox's Layer::removeDistantBlocks, evaluated on the device in f32).  Returns the stats."""
        ctr = np.ascontiguousarray(center, dtype=np.float32).reshape(3)
        st = KsRemoveStats()
        self._chk(lib().ks_remove_distant_blocks(self._h, _ptr(ctr), float(max_distance_m), C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in KsRemoveStats._fields_}

    def removed_blocks(self) -> np.ndarray:
        """The blocks the last remove_blocks() / remove_distant() took out, (n, 3) i32 ascending by (x, y, z)."""
        n = C.c_size_t()
        self._chk(lib().ks_removed_blocks(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 3), dtype=np.int32)
        if n.value:
            self._chk(lib().ks_removed_blocks(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def fuse(self, src: "HipIntegrator", T_D_S, min_weight=None, max_workspace_bytes=None) -> dict:
        """ks_fuse_map: resamples the map of `src` under T_D_S (qw qx qy qz tx ty tz: source frame -> this map's frame) into this
        map's grid and folds it in by the merge rule.  `src` is only read.  Returns the stats — also when the call is refused for
        its work space (KsError.stats).  The contract is DESIGN.md, section 17."""
        cfg = KsFuseConfig()
        self._chk(lib().ks_fuse_default_config(C.byref(cfg)))
        if min_weight is not None:
            cfg.min_weight = min_weight
        if max_workspace_bytes is not None:
            cfg.max_workspace_bytes = int(max_workspace_bytes)
        T = np.ascontiguousarray(T_D_S, dtype=np.float32).reshape(7)
        st = KsFuseStats()
        rc = lib().ks_fuse_map(self._h, src._h, _ptr(T), C.byref(cfg), C.byref(st))
        stats = {k: int(getattr(st, k)) for k, _ in KsFuseStats._fields_}
        try:
            self._chk(rc)
        except KsError as e:
            e.stats = stats
            raise
        return stats

    def reset_tiles(self, slots: np.ndarray):
        s = np.ascontiguousarray(slots, dtype=np.uint32)
        self._chk(lib().ks_reset_tiles(self._h, _ptr(s), len(s)))

    def reduce(self, rccl_comm, rank: int, world: int) -> dict:
        """ks_reduce: rccl_comm is an ncclComm_t (int / c_void_p) created with the same librccl."""
        st = KsReduceStats()
        self._chk(lib().ks_reduce(self._h, C.c_void_p(rccl_comm) if rccl_comm else None, rank, world, C.byref(st)))
        return {"tiles_sent": st.tiles_sent, "tiles_received": st.tiles_received, "tiles_local": st.tiles_local,
                "bytes_sent": st.bytes_sent}

    def debug_radix_sort(self, keys: np.ndarray, vals=None, end_bit=None):
        keys = np.ascontiguousarray(keys).copy()
        bits = keys.dtype.itemsize * 8
        vals = None if vals is None else np.ascontiguousarray(vals, dtype=np.uint32).copy()
        self._chk(lib().ks_debug_radix_sort(self._h, _ptr(keys), _ptr(vals), keys.shape[0], bits,
                                            bits if end_bit is None else end_bit))
        return keys, vals

    def debug_radix_sort_range(self, keys: np.ndarray, vals=None, begin_bit=0, end_bit=None):
        """ks_debug_radix_sort_range: (keys, vals) stably sorted by the bits [begin_bit, end_bit) of the keys (copies)."""
        keys = np.ascontiguousarray(keys).copy()
        bits = keys.dtype.itemsize * 8
        vals = None if vals is None else np.ascontiguousarray(vals, dtype=np.uint32).copy()
        self._chk(lib().ks_debug_radix_sort_range(self._h, _ptr(keys), _ptr(vals), keys.shape[0], bits, begin_bit,
                                                  bits if end_bit is None else end_bit))
        return keys, vals

    def debug_radix_sort_batch(self, keys: np.ndarray, vals: np.ndarray, counts, begin_bit, end_bit):
        """ks_debug_radix_sort_batch: keys u64 [nb, cap], vals u32 [nb, cap], counts [nb] -> the whole result buffers (copies)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64).copy()
        vals = np.ascontiguousarray(vals, dtype=np.uint32).copy()
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        nb, cap = keys.shape
        assert vals.shape == (nb, cap) and counts.shape == (nb,)
        self._chk(lib().ks_debug_radix_sort_batch(self._h, _ptr(keys), _ptr(vals), _ptr(counts), nb, cap, begin_bit, end_bit))
        return keys, vals

    def synchronize(self):
        self._chk(lib().ks_synchronize(self._h))

    @property
    def stream(self) -> int:
        return lib().ks_stream(self._h) or 0

    def profile_enable(self, level=1):
        """0 off, 1 all stages, 2 sampled k_apply dispatches only (see ks_hip.h)."""
        self._chk(lib().ks_profile_enable(self._h, int(level)))

    def early_out_stats(self):
        """Exact early-out: dict(frames, rounds, fallbacks, event_driven, pipelined)."""
        out = (C.c_uint64 * 5)()
        self._chk(lib().ks_early_out_stats(self._h, out))
        return dict(frames=int(out[0]), rounds=int(out[1]), fallbacks=int(out[2]), event_driven=bool(out[3]), pipelined=bool(out[4]))

    def integrate_round_exact(self, marcher: "HipIntegrator", rccl_comm, rank: int, world: int, first_frame: int, T_G_C, xyz, rgba, labels,
                              freespace=False) -> dict:
        """self = the OWNER context of this rank; `marcher` casts this rank's frame of the round (ks_integrate_round_exact).
        Both contexts `fast` or both `merged` (colours from the labels, pipeline_frames = 0).  COLLECTIVE: a rank whose frame fails
        (a label >= 21, a cloud of 2^24 points or more, rounds out of order) tells its peers in the count exchange; it raises its own
        error, the others KS_ERR_PEER_FAILED naming it, and no rank applies anything of that round."""
        T = np.ascontiguousarray(T_G_C, dtype=np.float32)
        n = 0 if xyz is None else len(xyz)
        x = None if xyz is None else np.ascontiguousarray(xyz, dtype=np.float32)
        c = None if rgba is None else np.ascontiguousarray(rgba, dtype=np.uint8)
        l = None if labels is None else np.ascontiguousarray(labels, dtype=np.uint8)
        st = KsRoundStats()
        self._chk(lib().ks_integrate_round_exact(marcher._h, self._h, rccl_comm, int(rank), int(world), int(first_frame), _ptr(T),
                                                 _ptr(x) if x is not None else None, _ptr(c) if c is not None else None,
                                                 _ptr(l) if l is not None else None, n, int(bool(freespace)), C.byref(st)))
        return dict(updates_marched=int(st.updates_marched), updates_applied=int(st.updates_applied), bytes_sent=int(st.bytes_sent),
                    origin_voxel_touched=bool(st.origin_voxel_touched), rays_cast=int(st.rays_cast))

    def update_stats(self):
        """Runs of more than 1024 updates: dict(walked, serial, chunks, replayed) — ks_update_stats."""
        out = (C.c_uint64 * 4)()
        self._chk(lib().ks_update_stats(self._h, out))
        return dict(walked=int(out[0]), serial=int(out[1]), chunks=int(out[2]), replayed=int(out[3]))

    def pipeline_shape(self):
        """dict(lag, slots, batch, march_streams): what ks_create made of ks_config.pipeline_frames."""
        out = (C.c_int32 * 4)()
        self._chk(lib().ks_pipeline_shape(self._h, out))
        return dict(lag=int(out[0]), slots=int(out[1]), batch=int(out[2]), march_streams=int(out[3]))

    def stream_plan(self):
        """dict(budget, streams, march_streams, long, xlong, march, tail): which chain runs on which stream (ks_stream_plan).
        long / xlong: "own" (a stream beside k_apply), "tail" (on the stage-T stream, behind it) or, xlong only, "none"."""
        out = (C.c_int32 * 8)()
        self._chk(lib().ks_stream_plan(self._h, out))
        side = {1: "own", 0: "tail", -1: "none"}
        return dict(budget=int(out[0]), streams=int(out[1]), march_streams=int(out[2]), long=side[int(out[3])], xlong=side[int(out[4])],
                    march="own" if out[5] else "A", tail="own" if out[6] else "A", streams_held=int(out[7]))

    def tail_batch_stats(self):
        """dict(batches, frames, per_frame_batches, pairs): batches of frames whose tail ran as one pass, the frames in them, batches
        whose frames' tails ran one by one, updates applied by the passes (ks_tail_batch_stats)."""
        out = (C.c_uint64 * 4)()
        self._chk(lib().ks_tail_batch_stats(self._h, out))
        return dict(batches=int(out[0]), frames=int(out[1]), per_frame_batches=int(out[2]), pairs=int(out[3]))

    def early_out_iterations(self):
        """(frames, fix-point iterations) of a KS_EARLY_OUT_EXACT context."""
        f, it = C.c_uint64(), C.c_uint64()
        self._chk(lib().ks_early_out_iterations(self._h, C.byref(f), C.byref(it)))
        return f.value, it.value

    def flush(self) -> KsFrameStats:
        """Finish the frames a pipelined context still holds; returns their statistics (summed)."""
        st = KsFrameStats()
        self._chk(lib().ks_flush(self._h, C.byref(st)))
        return st

    def profile(self, reset=False) -> dict:
        p = KsProfile()
        self._chk(lib().ks_profile_get(self._h, C.byref(p), int(reset)))
        return {"ms": {STAGES[i]: p.ms[i] for i in range(8)}, "launches": {STAGES[i]: p.launches[i] for i in range(8)},
                "frames": p.frames, "updates": p.updates, "points": p.points,
                "apply_kernel_ms": p.apply_kernel_ms, "apply_kernel_launches": p.apply_kernel_launches,
                "apply_kernel_updates": p.apply_kernel_updates, "host_ms": p.host_ms, "host_wait_ms": p.host_wait_ms}
