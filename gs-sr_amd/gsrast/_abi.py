"""The ctypes side of the C ABI, in one place: a Structure mirror of every `typedef struct` of include/gsrast.h and include/gsdecode.h (STRUCTS) and
one row (name, restype, argtypes) per entry point of both headers (FUNCTIONS).  gsrast.lib() applies the table once, at load.  This module imports
nothing from the package.  A new entry point is one row here and, for a new struct, one mirror; tests/test_abi_headers_cpu.py parses the two headers
and fails until names, argument counts, scalar types, pointees, field order, offsets and sizes agree with them."""
import ctypes as C

vp, sz, cint = C.c_void_p, C.c_size_t, C.c_int
i32, u32, i64, u64, f32, f64 = C.c_int32, C.c_uint32, C.c_int64, C.c_uint64, C.c_float, C.c_double
P = C.POINTER


def _of(ctype, *names):
    return [(n, ctype) for n in names]


# ---- include/gsrast.h
class gsr_cfg(C.Structure):
    _fields_ = _of(i32, "variant", "P", "D", "M", "W", "H") + _of(f32, "tanfovx", "tanfovy", "scale_modifier") + \
        _of(i32, "prefiltered", "debug", "render_geo") + _of(vp, "bg", "viewmatrix", "projmatrix", "campos")


class gsr_inputs(C.Structure):
    _fields_ = _of(vp, "means3D", "shs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp", "all_map")


class gsr_outputs(C.Structure):
    _fields_ = _of(vp, "out_color", "out_others", "out_observe", "out_all_map", "out_plane_depth")


class gsr_out_grads(C.Structure):
    _fields_ = _of(vp, "dL_dcolor", "dL_dothers", "dL_dout_all_map", "dL_dplane_depth", "all_map_pixels")


class gsr_in_grads(C.Structure):
    _fields_ = _of(vp, "dL_dmeans3D", "dL_dmeans2D", "dL_dmeans2D_abs", "dL_dcolors", "dL_dopacity", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations",
                   "dL_dall_map")


class gsr_tsdf_sparse(C.Structure):
    MAX_CHUNKS = 24                                       # GSR_TSDF_MAX_CHUNKS
    _fields_ = _of(vp, "keys", "slot", "coord", "stamp", "list", "counters", "mask") + [("chunk", vp * MAX_CHUNKS)] + \
        _of(u32, "chunk0_log2", "n_chunks", "cap_hash_log2", "cap_blocks") + _of(f32, "voxel_length", "sdf_trunc")


class gsr_adam_tensor(C.Structure):
    _fields_ = _of(vp, "param", "grad", "exp_avg", "exp_avg_sq", "lr_scale") + [("n", i64), ("beta1", f64), ("beta2", f64)] + \
        _of(f32, "step_size", "bias_correction2_sqrt", "eps", "pad_") + [("grad2", vp)]


class gsr_lod_cfg(C.Structure):
    _fields_ = _of(f32, "voxel_size", "fork", "standard_dist", "resolution_scale") + _of(i32, "coarse_index", "mode")


class gsr_mv_cfg(C.Structure):
    _fields_ = _of(i32, "W", "H", "Wn", "Hn", "Wg", "Hg") + _of(f32, "fx", "fy", "cx", "cy", "nfx", "nfy", "ncx", "ncy") + \
        [("v2n", f32 * 12), ("n2v", f32 * 12), ("ncc_scale", f32), ("noise_th", f32), ("patch", i32)]


class gsr_anchor_level(C.Structure):
    _fields_ = _of(i32, "Na", "N0", "k", "F", "scaling_stride") + _of(f32, "thr_lo", "thr_hi", "rand_thr", "cell") + [("origin", f32 * 3)] + \
        _of(vp, "anchor", "mask", "offset", "scaling", "anchor_feat", "grads", "offset_mask", "rand")


class gsr_octree_weed(C.Structure):
    _fields_ = [("cam_infos", vp)] + _of(i32, "C", "levels", "mode", "lv") + _of(f32, "standard_dist", "fork", "visible_threshold")


class gsr_rows_tensor(C.Structure):
    _fields_ = _of(vp, "src", "dst", "tail") + _of(i64, "row_bytes", "n_tail")


class gsr_densify_args(C.Structure):
    _fields_ = _of(i32, "P", "scaling_cols", "N", "flags") + \
        _of(f32, "clone_thr", "split_thr", "abs_thr", "dense_thr", "min_opacity", "world_thr", "abs_radii_thr", "child_div", "clone_cap", "split_cap", "abs_cap") + \
        _of(vp, "accum", "denom", "accum_abs", "denom_abs", "scaling", "opacity", "max_radii2D", "masked_out")


class gsr_densify_tensor(C.Structure):
    _fields_ = _of(vp, "src", "dst") + [("row_bytes", i64), ("zero_new", i32), ("pad_", i32)]


class gsr_densify_compute(C.Structure):
    _fields_ = _of(vp, "xyz", "rotation", "xyz_dst", "scaling_dst", "noise_split", "noise_clone")


class gsr_mesh_filter(C.Structure):
    _fields_ = _of(vp, "triangles", "remove_mask") + _of(i64, "n_triangles", "n_vertices") + _of(i32, "cluster_to_keep", "floor", "flags", "pad_")


# ---- include/gsdecode.h
class gsd_cfg(C.Structure):
    _fields_ = _of(i32, "Na", "Nv", "k", "A", "dist_o", "dist_c", "dist_k", "level")


class gsd_inputs(C.Structure):
    _fields_ = _of(vp, "anchor", "feat", "offset", "scaling", "level", "opacity_scale", "vis_idx", "campos")


class gsd_params(C.Structure):
    _fields_ = _of(vp, "W1o", "b1o", "W2o", "b2o", "W1c", "b1c", "W2c", "b2c", "W1k", "b1k", "W2k", "b2k", "app")


class gsd_outputs(C.Structure):
    _fields_ = _of(vp, "xyz", "color", "opacity", "scaling", "rot")


class gsd_out_grads(C.Structure):
    _fields_ = _of(vp, "xyz", "color", "opacity", "scaling", "rot")


class gsd_in_grads(C.Structure):
    _fields_ = _of(vp, "anchor", "feat", "offset", "scaling") + [("params", gsd_params)]


STRUCTS = {s.__name__: s for s in (
    gsr_cfg, gsr_inputs, gsr_outputs, gsr_out_grads, gsr_in_grads, gsr_tsdf_sparse, gsr_adam_tensor, gsr_lod_cfg, gsr_mv_cfg, gsr_anchor_level, gsr_octree_weed,
    gsr_rows_tensor, gsr_densify_args, gsr_densify_tensor, gsr_densify_compute, gsr_mesh_filter,
    gsd_cfg, gsd_inputs, gsd_params, gsd_outputs, gsd_out_grads, gsd_in_grads)}

_cfg, _in, _out, _vol, _lv, _weed, _den = P(gsr_cfg), P(gsr_inputs), P(gsr_outputs), P(gsr_tsdf_sparse), P(gsr_anchor_level), P(gsr_octree_weed), P(gsr_densify_args)
_dec = [P(gsd_cfg), P(gsd_inputs), P(gsd_params)]
_arenas = [vp, sz, vp, sz, vp, sz]                        # geom, binning, img: pointer and bytes each

# (name, restype, argtypes), in the order of the headers.  Array and buffer pointers are void*; a pointer the host wrapper fills in with byref() or a
# ctypes array is typed.
FUNCTIONS = [
    ("gsr_geom_bytes", sz, [i32, i32]),
    ("gsr_img_bytes", sz, [i32, i32, i32]),
    ("gsr_binning_bytes", sz, [i32, u32, i32, i32]),
    ("gsr_backward_scratch_bytes", sz, [i32, i32]),
    ("gsr_forward_stage1", cint, [_cfg, _in, vp, sz, vp, P(u32), vp]),
    ("gsr_forward_stage2", cint, [_cfg, _in] + _arenas + [u32, _out, vp]),
    ("gsr_forward_stage1_ex", cint, [_cfg, _in, vp, sz, vp, P(u32), P(u32), vp]),
    ("gsr_forward_stage2_ex", cint, [_cfg, _in] + _arenas + [u32, u32, _out, vp]),
    ("gsr_binning_capacity", u32, [i32, sz, i32, i32]),
    ("gsr_forward", cint, [_cfg, _in] + _arenas + [vp, _out, P(u32), P(i32), vp]),
    ("gsr_backward", cint, [_cfg, _in, vp] + _arenas + [u32, vp, sz, P(gsr_out_grads), P(gsr_in_grads), vp]),
    ("gsr_backward_ex", cint, [_cfg, _in, vp] + _arenas + [u32, vp, sz, P(gsr_out_grads), P(gsr_in_grads), u32, vp]),
    ("gsr_forward_async", cint, [_cfg, _in] + _arenas + [vp, _out, vp, vp]),
    ("gsr_mark_visible", cint, [i32, vp, vp, vp, vp, vp]),
    ("gsr_visible_filter", cint, [_cfg, vp, vp, vp, vp, vp, vp]),
    ("gsr_tsdf_integrate", cint, [i64, vp, vp, i32, i32, vp, vp, f32, vp, vp, vp, vp, vp, vp]),
    ("gsr_tsdf_integrate_dense", cint, [i32, i32, i32, P(f32), f32, f32, f32, i32, i32, vp, vp, f32, f32, f32, f32, P(f32), vp, vp, vp, vp]),
    ("gsr_tsdf_sparse_integrate2", cint, [_vol, i32, i32, vp, vp, i32, f32, f32, f32, f32, P(f32), P(f32), f32, i32, u32, vp, vp, u32, vp]),
    ("gsr_tsdf_sparse_status", cint, [_vol, vp, vp]),
    ("gsr_tsdf_sparse_rehash", cint, [_vol, i32, vp]),
    ("gsr_tsdf_sparse_merge", cint, [_vol, i32, vp, vp, vp, vp, vp]),
    ("gsr_tsdf_sparse_merge_volume", cint, [_vol, _vol, i32, vp]),
    ("gsr_tsdf_sparse_materialize", cint, [_vol, i32, vp]),
    ("gsr_tsdf_sparse_mesh_scratch_bytes", sz, [i32]),
    ("gsr_tsdf_sparse_mesh_count", cint, [_vol, i32, vp, f32, vp, sz, P(u64), vp]),
    ("gsr_tsdf_sparse_mesh_emit", cint, [_vol, i32, vp, f32, vp, sz, vp, vp, vp, vp]),
    ("gsr_loss_l1_linear", cint, [i64, vp, vp, vp, i64, vp, vp, vp, vp]),
    ("gsr_adam_step", cint, [i64, vp, vp, vp, vp, f32, f64, f64, f32, f32, vp, vp]),
    ("gsr_adam_step_multi", cint, [i32, vp, vp]),
    ("gsr_adam_step_multi_dev", cint, [i32, vp, vp, vp]),
    ("gsr_octree_visible", cint, [_cfg, P(gsr_lod_cfg), vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
    ("gsr_loss_l1_ssim_scratch_bytes", sz, [i32, i32, i32]),
    ("gsr_loss_l1_ssim", cint, [i32, i32, i32, vp, vp, f32, vp, vp, vp, sz, vp]),
    ("gsr_loss_surfel_geo_scratch_bytes", sz, [i32, i32]),
    ("gsr_loss_surfel_geo", cint, [i32, i32, vp, vp, vp, f32, f32, f32, vp, vp, vp, vp, vp, vp, sz, vp]),
    ("gsr_loss_plane_geo", cint, [i32, i32, vp, vp, vp, vp, vp, f32, vp, vp, vp, vp, vp, sz, vp]),
    ("gsr_loss_scaling_prod", cint, [i64, i32, i32, vp, vp, f32, vp, vp, vp]),
    ("gsr_densify_stats", cint, [i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]),
    ("gsr_gauss_activations", cint, [i32, i32] + [vp] * 7),
    ("gsr_gauss_activations_backward", cint, [i32, i32] + [vp] * 11),
    ("gsr_plane_allmap", cint, [i32, vp, vp, vp, i32, vp, vp, vp, vp]),
    ("gsr_plane_allmap_backward", cint, [i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
    ("gsr_sample_mask_scratch_bytes", sz, [i64]),
    ("gsr_sample_mask", cint, [i64, vp, i32, u64, vp, vp, sz, vp]),
    ("gsr_loss_plane_mv_scratch_bytes", sz, [i32, i32, i32]),
    ("gsr_loss_plane_mv_geo", cint, [P(gsr_mv_cfg)] + [vp] * 9 + [sz, vp]),
    ("gsr_loss_plane_mv_ncc", cint, [P(gsr_mv_cfg), i32] + [vp] * 12 + [sz, vp]),
    ("gsr_loss_plane_mv_values", cint, [vp, f32, f32, vp, vp]),
    ("gsr_loss_plane_mv_scale", cint, [sz, sz, sz, vp, vp, vp, vp, f32, f32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]),
    ("gsr_anchor_level_scratch_bytes", sz, [i32, i32, i32]),
    ("gsr_anchor_level_find", cint, [_lv, vp, sz, vp, vp]),
    ("gsr_anchor_level_emit", cint, [_lv, vp, sz, u32, vp, vp, vp]),
    ("gsr_anchor_level_find_weed", cint, [_lv, vp, _weed, vp, sz, vp, vp]),
    ("gsr_octree_weed_out", cint, [vp, vp, i64, _weed, vp, vp, vp]),
    ("gsr_rows_compact_scratch_bytes", sz, [i64]),
    ("gsr_rows_compact_multi", cint, [i64, vp, i32, P(gsr_rows_tensor), vp, sz, vp]),
    ("gsr_densify_plan_scratch_bytes", sz, [i32, i32]),
    ("gsr_densify_plan", cint, [_den, vp, sz, vp, vp]),
    ("gsr_densify_emit", cint, [_den, vp, sz, P(u32), i32, P(gsr_densify_tensor), P(gsr_densify_compute), vp]),
    ("gsr_mesh_post_scratch_bytes", sz, [i64, i64]),
    ("gsr_mesh_cluster_triangles", cint, [vp, i64, i64, vp, vp, vp, vp, vp, sz, vp, vp]),
    ("gsr_mesh_filter_count", cint, [P(gsr_mesh_filter), vp, sz, vp, vp]),
    ("gsr_mesh_filter_emit", cint, [P(gsr_mesh_filter), vp, sz, P(u32), i32, P(gsr_rows_tensor), vp, vp]),
    ("gsr_mesh_simplify_scratch_bytes", sz, [i64, i64, i32]),
    ("gsr_mesh_simplify_count", cint, [vp, i64, vp, i64, f64, i32, vp, sz, vp, vp]),
    ("gsr_mesh_simplify_emit", cint, [vp, vp, i64, i64, f64, i32, vp, sz, P(u32), vp, vp, vp, vp, vp]),
    ("gsr_mesh_adjacency_scratch_bytes", sz, [i64, i64]),
    ("gsr_mesh_adjacency_count", cint, [vp, i64, i64, vp, sz, vp, vp]),
    ("gsr_mesh_adjacency_emit", cint, [i64, i64, vp, sz, P(u32), vp, vp, vp]),
    ("gsr_mesh_normals_scratch_bytes", sz, [i64, i64]),
    ("gsr_mesh_normals", cint, [vp, i64, vp, i64, i32, vp, vp, vp, sz, vp, vp]),
    ("gsr_mesh_smooth_scratch_bytes", sz, [i64, i64, i32]),
    ("gsr_mesh_smooth", cint, [vp, vp, i64, vp, i64, i32, i32, f64, f64, i32, vp, vp, vp, sz, vp, vp]),
    ("gsr_mesh_raster_scratch_bytes", sz, [i64, i64, i32, i32, i32]),
    ("gsr_mesh_rasterize", cint, [vp, i64, vp, i64, vp, i32, i32, i32, f64, i32, f64, i32, vp, vp, vp, vp, vp, vp, sz, vp, vp]),
    ("gsr_unbounded_lattice_points", cint, [i32, i32, i32, vp, vp, vp, P(f32), f32, f32, vp, vp, vp]),
    ("gsr_unbounded_lattice_tsdf", cint, [i32, i32, i32, vp, vp, vp, P(f32), f32, f32, i32, vp, i32, i32, vp, vp, vp, vp]),
    ("gsr_unbounded_mc_scratch_bytes", sz, [i32, i32, i32]),
    ("gsr_unbounded_mc_count", cint, [i32, i32, i32, i32, vp, vp, sz, i64, i64, P(u64), vp]),
    ("gsr_unbounded_mc_emit", cint, [i32, i32, i32, i32, vp, vp, vp, vp, vp, sz, i64, i64, i64, vp, vp, vp]),
    ("gsr_unbounded_finish", cint, [i64, P(f32), f32, f32, vp, vp]),
    ("gsr_unbounded_texture", cint, [i64, vp, f32, i32, vp, i32, i32, vp, vp, vp, vp]),
    ("gsr_dist2_scratch_bytes", sz, [i32]),
    ("gsr_dist2", cint, [i32, vp, vp, vp, sz, vp]),
    ("gsr_cam_dist_quantiles_scratch_bytes", sz, [i64, i32]),
    ("gsr_cam_dist_quantiles", cint, [vp, i64, vp, i32, P(i64), P(i64), P(f32), vp, vp, sz, vp, vp]),
    ("gsr_select_lerp_scratch_bytes", sz, [i64]),
    ("gsr_select_lerp", cint, [vp, i64, vp, i32, P(i64), P(i64), P(f32), vp, vp, sz, vp, vp]),
    ("gsr_voxel_unique_scratch_bytes", sz, [i64, i32]),
    ("gsr_voxel_unique_count", cint, [vp, i64, i32, P(f64), P(f64), i32, vp, sz, vp, vp]),
    ("gsr_voxel_unique_emit", cint, [vp, i64, i32, P(f64), P(f64), i32, vp, sz, P(u32), vp, vp, vp]),
    ("gsr_view_select_scratch_bytes", sz, [i64, i32]),
    ("gsr_view_select", cint, [vp, i32, vp, vp, i64, vp, vp, i64, f64, f64, f64, i32, i32, vp, vp, vp, vp, sz, vp, vp]),
    ("gsr_partition_boxes", cint, [vp, i64, i32, vp, i32, vp, vp, vp, vp]),
    ("gsr_partition_zrange_scratch_bytes", sz, [i64, i64]),
    ("gsr_partition_zrange", cint, [vp, i64, vp, i32, i32, i64, i64, vp, vp, vp, sz, vp, vp]),
    ("gsr_partition_visibility", cint, [vp, vp, i32, vp, vp, vp, i32, vp, f64, vp, vp, vp, vp, vp, vp]),
    ("gsr_partition_coverage_mask", cint, [vp, vp, i64, vp, i32, vp, i64, i32, vp, vp, vp, vp]),
    ("gsr_partition_coverage_rows_scratch_bytes", sz, [i64]),
    ("gsr_partition_coverage_rows", cint, [vp, i64, i32, P(i64), vp, vp, sz, vp]),
    ("gsr_nearest_points_scratch_bytes", sz, [i64, i64]),
    ("gsr_nearest_points", cint, [vp, i64, vp, i64, f32, vp, vp, vp, sz, vp]),
    ("gsr_sample_surface_scratch_bytes", sz, [i64]),
    ("gsr_sample_surface_count", cint, [vp, i64, vp, i64, f64, vp, sz, vp, vp]),
    ("gsr_sample_surface_emit", cint, [vp, i64, vp, i64, f64, vp, sz, i64, vp, vp]),
    ("gsr_voxel_downsample_scratch_bytes", sz, [i64]),
    ("gsr_voxel_downsample_count", cint, [vp, i64, f64, vp, sz, vp, vp]),
    ("gsr_voxel_downsample_emit", cint, [vp, i64, vp, sz, i64, vp, vp, vp]),
    ("gsr_distance_stats_scratch_bytes", sz, [i64]),
    ("gsr_distance_stats", cint, [vp, i64, f64, P(f64), i32, vp, vp, sz, vp]),
    ("gsr_nearest_grid_scratch_bytes", sz, [i64]),
    ("gsr_nearest_grid_build", cint, [vp, i64, f32, vp, sz, vp]),
    ("gsr_nearest_grid_query", cint, [vp, i64, i64, f32, vp, sz, vp, vp, vp, vp]),
    ("gsr_transform_points", cint, [vp, i64, P(f64), vp, vp]),
    ("gsr_correspondence_sums_scratch_bytes", sz, [i64]),
    ("gsr_correspondence_sums", cint, [vp, i64, vp, i64, vp, vp, vp, sz, vp]),
    ("gsr_solve_transform", cint, [vp, i32, vp]),
    ("gsr_icp_scratch_bytes", sz, [i64, i64]),
    ("gsr_icp", cint, [vp, i64, vp, i64, f32, P(f64), i32, f64, f64, i32, vp, vp, sz, vp]),
    ("gsr_crop_polygon_scratch_bytes", sz, []),
    ("gsr_crop_polygon_volume", cint, [vp, i64, P(f64), i32, i32, f64, f64, vp, vp, sz, vp]),
    ("gsr_image_resample_scratch_bytes", sz, [i32, i32, i32, i32, i32]),
    ("gsr_image_resample", cint, [vp, i32, i32, i32, i64, i32, i32, vp, vp, i32, vp, vp, vp, sz, vp]),
    ("gsr_debug_read", cint, [_cfg, i32, vp, vp, sz, vp, u32, vp, vp]),
    ("gsr_profile_enable", cint, [i32]),
    ("gsr_profile_read", cint, [P(f64), P(u64)]),
    ("gsr_last_error", C.c_char_p, []),
    ("gsr_abi_version", i32, []),
    ("gsd_compact_scratch_bytes", sz, [i32]),
    ("gsd_compact_visible", cint, [vp, i32, vp, P(u32), vp, sz, vp]),
    ("gsd_compact_visible_padded", cint, [vp, i32, vp, vp, vp, sz, vp]),
    ("gsd_forward_scratch_bytes", sz, [i32]),
    ("gsd_forward_stage1", cint, _dec + [vp, vp, vp, P(u32), vp, sz, vp]),
    ("gsd_forward_stage2", cint, _dec + [vp, vp, u32, P(gsd_outputs), vp, sz, vp]),
    ("gsd_forward", cint, _dec + [vp, vp, vp, P(gsd_outputs), P(u32), vp, sz, vp]),
    ("gsd_forward_static", cint, _dec + [vp, vp, vp, P(gsd_outputs), vp, vp, sz, vp]),
    ("gsd_forward_deferred", cint, _dec + [vp, vp, vp, P(gsd_outputs), vp, vp, vp, sz, vp]),
    ("gsd_backward_scratch_bytes", sz, [P(gsd_cfg)]),
    ("gsd_backward", cint, _dec + [vp, vp, u32, P(gsd_out_grads), P(gsd_in_grads), vp, vp, sz, vp]),
    ("gsd_training_stats_scratch_bytes", sz, [i32]),
    ("gsd_training_stats", cint, [i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, sz, vp]),
]


def bind(L, path):
    """Gives every entry point of the table its signature on the loaded library L; one that the library lacks is named."""
    for name, restype, argtypes in FUNCTIONS:
        f = getattr(L, name, None)
        if f is None:
            raise RuntimeError(f"gsrast: {path} does not export {name}, which include/ declares: rebuild the library (`make -C gs-sr_amd/csrc`)")
        f.restype, f.argtypes = restype, argtypes
