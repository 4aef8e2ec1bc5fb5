"""ctypes mirror of include/rtx.h, include/rtx_scene.h and include/rtx_kat.h.

Test / bench plumbing only: the product boundary is the C-ABI in include/.
"""
import ctypes as C

RTX_OK = 0
RTX_ERR_ARG, RTX_ERR_HIP, RTX_ERR_NOMEM, RTX_ERR_SCENE, RTX_ERR_NODEV, RTX_ERR_STATE, RTX_ERR_IO = (
    -1, -2, -3, -4, -5, -6, -7)

RTX_SPHERE, RTX_TRIANGLE, RTX_PLANE = 0, 1, 2
RTX_TEX_UNIFORM, RTX_TEX_CHECKERBOARD, RTX_TEX_BRICK, RTX_TEX_NOISY_PERIODIC = 0, 1, 2, 3
RTX_PHONG, RTX_BLINN = 0, 1
RTX_GI_AMBIENT, RTX_GI_PATH = 0, 1
RTX_ATT_NONE, RTX_ATT_LIN, RTX_ATT_SQR = 0, 1, 2
RTX_RNG_COUNTER, RTX_RNG_CONST, RTX_RNG_STRAT = 0, 1, 2
RTX_U32_SAT, RTX_U32_WRAP = 0, 1

F3 = C.c_float * 3


class Material(C.Structure):
    _fields_ = [("id", C.c_int32), ("ks", F3), ("ka", F3), ("kr", F3), ("kt", F3), ("ke", F3),
                ("shininess", C.c_float), ("refractive_index", C.c_float), ("texture", C.c_int32),
                ("periodic", C.c_int32), ("color", F3 * 2), ("scale", C.c_float), ("mortar_width", C.c_float),
                ("noise_feature_scale", C.c_float), ("noise_scale", C.c_float), ("frequency_scale", C.c_float),
                ("emittant", C.c_int32), ("reflective", C.c_int32), ("transparent", C.c_int32)]


class Object(C.Structure):
    _fields_ = [("type", C.c_int32), ("material", C.c_int32), ("num_lights", C.c_uint32), ("epsilon", C.c_float),
                ("p0", F3), ("p1", F3), ("p2", F3), ("e1", F3), ("e2", F3), ("n", F3), ("radius", C.c_float),
                ("d", C.c_float)]


class Camera(C.Structure):
    _fields_ = [("position", F3), ("vectors", F3 * 3), ("fov", C.c_float), ("focal_length", C.c_float)]


class SceneDesc(C.Structure):
    _fields_ = [("num_materials", C.c_uint32), ("materials", C.POINTER(Material)), ("num_objects", C.c_uint32),
                ("objects", C.POINTER(Object)), ("num_emitters", C.c_uint32), ("emitters", C.POINTER(C.c_uint32)),
                ("ambient", F3), ("camera", Camera)]


class Frame(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("corner", F3), ("step_x", F3), ("step_y", F3),
                ("origin", F3)]


class Params(C.Structure):
    _fields_ = [("max_bounces", C.c_uint32), ("min_intensity_sqr", C.c_float), ("reflection", C.c_int32),
                ("gi", C.c_int32), ("samples", C.c_uint32), ("attenuation", C.c_int32),
                ("attenuation_offset", C.c_float), ("rng", C.c_int32), ("seed", C.c_uint64),
                ("u32conv", C.c_int32), ("tile_offset", C.c_uint32), ("tile_stride", C.c_uint32),
                ("count_traversal", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("closest_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("node_visits", C.c_uint64),
                ("tri_tests", C.c_uint64), ("sphere_tests", C.c_uint64), ("plane_tests", C.c_uint64),
                ("shadow_node_visits", C.c_uint64), ("shadow_tri_tests", C.c_uint64),
                ("shadow_sphere_tests", C.c_uint64), ("shadow_plane_tests", C.c_uint64),
                ("shade_points", C.c_uint64), ("kernel_ms", C.c_double), ("trace_ms", C.c_double),
                ("shadow_ms", C.c_double), ("accum_ms", C.c_double), ("sort_ms", C.c_double), ("build_ms", C.c_double),
                ("bvh_nodes", C.c_uint32),
                ("bvh_depth", C.c_uint32), ("bvh_prims", C.c_uint32), ("waves", C.c_uint32),
                ("chunks", C.c_uint32), ("builder", C.c_uint32),
                ("shadow_box_tests", C.c_uint64), ("shadow_global_box_tests", C.c_uint64),
                ("shadow_wave_steps", C.c_uint64), ("shadow_wave_walks", C.c_uint64),
                ("wide_nodes", C.c_uint32), ("wide_depth", C.c_uint32), ("shadow_leaf_rounds", C.c_uint64),
                ("gather_ms", C.c_double), ("devices", C.c_uint32), ("pad_", C.c_uint32),
                ("shadow_uniform_steps", C.c_uint64), ("shadow_walk", C.c_uint32), ("wide_entries", C.c_uint32),
                ("trace_walk", C.c_uint32), ("pad2_", C.c_uint32), ("tree_rotated", C.c_uint32),
                ("pad3_", C.c_uint32), ("frame_cost", C.c_double), ("frame_ms", C.c_double),
                ("upload_copy_ms", C.c_double), ("transport", C.c_uint32), ("peer_access", C.c_uint32),
                ("far_closest_rays", C.c_uint64), ("far_shadow_rays", C.c_uint64),
                ("shadow_stack_spills", C.c_uint64), ("shadow_cone_clear", C.c_uint64)]


class PointStats(C.Structure):
    """rtx_point_stats: rtx_stats' continuation (rtxpy's stats() set its fields on the Stats they return)"""
    _fields_ = [("shadow_plane_skipped", C.c_uint64), ("shadow_lin_skipped", C.c_uint64),
                ("shadow_point_clear", C.c_uint64)]


class DarkStats(C.Structure):
    """rtx_dark_stats: the counters of RTX_OPT_SHADOW_DARK (rtxpy's stats() set them on the Stats they return)"""
    _fields_ = [("shadow_dark_rays", C.c_uint64), ("shadow_dark_packet_rays", C.c_uint64)]


class OrderStats(C.Structure):
    """rtx_order_stats: the counters of RTX_OPT_SHADOW_ORDER (rtxpy's stats() set them on the Stats they return)"""
    _fields_ = [("shadow_ordered_points", C.c_uint64), ("shadow_ordered_rays", C.c_uint64)]


class PremaskStats(C.Structure):
    """rtx_premask_stats: whether RTX_OPT_SHADOW_PREMASK took effect (rtxpy's stats() set it on the Stats they return)"""
    _fields_ = [("premask_points", C.c_uint64)]


class ClearlaneStats(C.Structure):
    """rtx_clearlane_stats: what RTX_OPT_SHADOW_CLEARLANE took (rtxpy's stats() set them on the Stats they return)"""
    _fields_ = [("clear_points", C.c_uint64), ("clear_rays", C.c_uint64)]


RTX_TRANSPORT_NONE, RTX_TRANSPORT_RCCL, RTX_TRANSPORT_LOOPBACK, RTX_TRANSPORT_RCCL_SELF = 0, 1, 2, 3


class GroupMember(C.Structure):
    _fields_ = [("device", C.c_int32), ("comm_count", C.c_int32), ("comm_rank", C.c_int32), ("comm_device", C.c_int32),
                ("can_access_peer0", C.c_uint32), ("peer0_can_access", C.c_uint32), ("peer_enabled", C.c_uint32),
                ("transport", C.c_uint32), ("pci_bus_id", C.c_char * 32)]


RTX_BUILD_SAH_HOST, RTX_BUILD_LBVH_GPU, RTX_BUILD_PLOC_GPU, RTX_BUILD_SAH_GPU = 0, 1, 2, 3
RTX_WALK_AUTO, RTX_WALK_BVH2, RTX_WALK_W8, RTX_WALK_LINEAR = -1, 0, 2, 3
WALK_NAMES = {RTX_WALK_BVH2: "bvh2", RTX_WALK_W8: "w8", RTX_WALK_LINEAR: "linear"}
RTX_SHADOW_LINEAR_MAX = 8
RTX_FRAME_AUTO, RTX_FRAME_WORLD = 0, 1
RTX_OPT_SHADOW_WALK, RTX_OPT_BVH_LEAF, RTX_OPT_SPSORT, RTX_OPT_SHADOW_SLOT, RTX_OPT_SHADOW_GRAB, \
    RTX_OPT_SHADOW_LDS_STACK, RTX_OPT_TRACE_WALK, RTX_OPT_TREE_FRAME, RTX_OPT_CHUNK_TILES, \
    RTX_OPT_SP_PER_TILE, RTX_OPT_SHADOW_CULL, RTX_OPT_RAYS_GRAB, RTX_OPT_RAYS_QUEUES, \
    RTX_OPT_SHADOW_POINT, RTX_OPT_SHADOW_DARK, RTX_OPT_SHADOW_PREMASK, RTX_OPT_SHADOW_ORDER, \
    RTX_OPT_SHADOW_SPEC, RTX_OPT_TRACE_PACK, RTX_OPT_SHADOW_CLEARLANE = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20
RTX_DOF_NONE, RTX_DOF_SCALE_BIAS, RTX_DOF_CAMERA = 0, 1, 2
RTX_FALLOFF_QUAD, RTX_FALLOFF_LIN, RTX_FALLOFF_INV_QUAD = 0, 1, 2


class Post(C.Structure):
    _fields_ = [("brighten", C.c_int32), ("brighten_factor", C.c_float), ("dof", C.c_int32),
                ("dof_scale", C.c_float), ("dof_bias", C.c_float), ("aperture", C.c_float),
                ("focal_length", C.c_float), ("plane_in_focus", C.c_float), ("mist", C.c_int32),
                ("mist_start", C.c_float), ("mist_depth", C.c_float), ("mist_falloff", C.c_int32),
                ("mist_color", F3)]


# ray queries (rtx_trace_rays*)
RTX_RAYS_ANY_HIT, RTX_RAYS_REORDER, RTX_RAYS_COUNT = 1, 2, 4
RTX_RAYS_MAX = 0x7FFFFFFF


class Ray(C.Structure):
    _fields_ = [("origin", F3), ("tmax", C.c_float), ("dir", F3), ("pad_", C.c_uint32)]


class Hit(C.Structure):
    _fields_ = [("t", C.c_float), ("object", C.c_int32), ("material", C.c_int32), ("outside", C.c_uint32),
                ("n", F3), ("pad_", C.c_uint32)]


class RayStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("hits", C.c_uint64), ("node_visits", C.c_uint64), ("tri_tests", C.c_uint64),
                ("sphere_tests", C.c_uint64), ("plane_tests", C.c_uint64), ("far_rays", C.c_uint64),
                ("kernel_ms", C.c_double), ("sort_ms", C.c_double)]


# numpy views of rtx_ray / rtx_hit arrays (the same 32-byte layouts)
RAY_DTYPE = [("origin", "<f4", 3), ("tmax", "<f4"), ("dir", "<f4", 3), ("pad_", "<u4")]
HIT_DTYPE = [("t", "<f4"), ("object", "<i4"), ("material", "<i4"), ("outside", "<u4"), ("n", "<f4", 3), ("pad_", "<u4")]

# shadow queries (rtx_trace_shadow_rays)
RTX_SHADOW_RAYS_SLOTS, RTX_SHADOW_RAYS_COUNT = 1, 2


class ShadowRay(C.Structure):
    _fields_ = [("origin", F3), ("dist", C.c_float), ("dir", F3), ("light_object", C.c_int32)]


class ShadowResult(C.Structure):
    _fields_ = [("transmittance", F3), ("blocked", C.c_uint32)]


class ShadowRayStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("blocked", C.c_uint64), ("far_rays", C.c_uint64), ("box_tests", C.c_uint64),
                ("tri_tests", C.c_uint64), ("sphere_tests", C.c_uint64), ("wave_steps", C.c_uint64),
                ("uniform_steps", C.c_uint64), ("leaf_rounds", C.c_uint64), ("stack_spills", C.c_uint64),
                ("kernel_ms", C.c_double)]


# closest-point queries (rtx_closest_points*)
RTX_CLOSEST_BOUNDED_ONLY, RTX_CLOSEST_REORDER, RTX_CLOSEST_COUNT = 1, 2, 4
RTX_NONE = 0xFFFFFFFF


class PointQuery(C.Structure):
    _fields_ = [("p", F3), ("max_dist", C.c_float)]


class Closest(C.Structure):
    _fields_ = [("point", F3), ("dist", C.c_float), ("object", C.c_uint32), ("material", C.c_uint32),
                ("pad", C.c_uint32 * 2)]


class ClosestStats(C.Structure):
    _fields_ = [("points", C.c_uint64), ("found", C.c_uint64), ("node_visits", C.c_uint64), ("tri_tests", C.c_uint64),
                ("sphere_tests", C.c_uint64), ("plane_tests", C.c_uint64), ("far_points", C.c_uint64),
                ("kernel_ms", C.c_double), ("sort_ms", C.c_double)]


POINT_QUERY_DTYPE = [("p", "<f4", 3), ("max_dist", "<f4")]
CLOSEST_DTYPE = [("point", "<f4", 3), ("dist", "<f4"), ("object", "<u4"), ("material", "<u4"), ("pad", "<u4", 2)]

SHADOW_RAY_DTYPE = [("origin", "<f4", 3), ("dist", "<f4"), ("dir", "<f4", 3), ("light_object", "<i4")]
SHADOW_RESULT_DTYPE = [("transmittance", "<f4", 3), ("blocked", "<u4")]

# denoiser (rtx_frame_features*, rtx_denoise*)
class Feature(C.Structure):
    _fields_ = [("position", F3), ("z", C.c_float), ("normal", F3), ("material", C.c_int32), ("albedo", F3),
                ("object", C.c_int32)]


class DenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_albedo", C.c_float), ("sigma_plane", C.c_float)]


class DenoiseStats(C.Structure):
    _fields_ = [("features_ms", C.c_double), ("filter_ms", C.c_double), ("pixels", C.c_uint64),
                ("hit_pixels", C.c_uint64), ("iterations", C.c_uint32), ("pad_", C.c_uint32)]


# numpy view of rtx_feature arrays (the same 48-byte layout)
FEATURE_DTYPE = [("position", "<f4", 3), ("z", "<f4"), ("normal", "<f4", 3), ("material", "<i4"), ("albedo", "<f4", 3),
                 ("object", "<i4")]
# rtx_denoise_params_default
DENOISE_DEFAULTS = {"iterations": 1, "sigma_color": 0.004, "sigma_normal": 0.05, "sigma_albedo": 0.1, "sigma_plane": 0.02}


class DenoiseVarianceParams(C.Structure):
    """rtx_denoise_variance_params: sigma_color in standard deviations of a colour difference"""
    _fields_ = [("iterations", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_albedo", C.c_float), ("sigma_plane", C.c_float)]


# rtx_denoise_variance_params_default
DENOISE_VARIANCE_DEFAULTS = {"iterations": 1, "sigma_color": 3.0, "sigma_normal": 0.05, "sigma_albedo": 0.1,
                             "sigma_plane": 0.02}

# multi-pass rendering (rtx_pass_frame, rtx_render_passes*)
RTX_PASS_JITTER = 1
RTX_PASSES_MAX = 65536


class PassParams(C.Structure):
    _fields_ = [("passes", C.c_uint32), ("flags", C.c_uint32), ("aperture", C.c_float), ("focus", C.c_float),
                ("target_error", C.c_float), ("min_passes", C.c_uint32)]


class PassStats(C.Structure):
    _fields_ = [("passes_run", C.c_uint32), ("pad_", C.c_uint32), ("error", C.c_double), ("render_ms", C.c_double),
                ("accum_ms", C.c_double), ("closest_rays", C.c_uint64), ("shadow_rays", C.c_uint64)]


class AdaptiveStats(C.Structure):
    _fields_ = [("passes_run", C.c_uint32), ("tiles", C.c_uint32), ("tile_passes", C.c_uint64), ("error", C.c_double),
                ("render_ms", C.c_double), ("fold_ms", C.c_double), ("closest_rays", C.c_uint64), ("shadow_rays", C.c_uint64)]


class GroupExchangeStats(C.Structure):
    """rtx_group_exchange_stats: what the last rtx_group_render_passes / rtx_group_render_adaptive moved between members"""
    _fields_ = [("exchanges", C.c_uint32), ("pad_", C.c_uint32), ("bytes", C.c_uint64), ("exchange_ms", C.c_double),
                ("gather_ms", C.c_double)]


# pixel reconstruction filters (rtx_pass_filter_weights, rtx_render_passes_filtered*)
RTX_FILTER_BOX, RTX_FILTER_TENT, RTX_FILTER_GAUSSIAN, RTX_FILTER_MITCHELL = range(4)
RTX_FILTER_TAPS = 5
FILTER_KINDS = {"box": RTX_FILTER_BOX, "tent": RTX_FILTER_TENT, "gaussian": RTX_FILTER_GAUSSIAN,
                "mitchell": RTX_FILTER_MITCHELL}
# each kind's radius range in pixels
FILTER_RADIUS = {RTX_FILTER_BOX: (0.5, 2.5), RTX_FILTER_TENT: (1.0, 2.5), RTX_FILTER_GAUSSIAN: (1.0, 2.5),
                 RTX_FILTER_MITCHELL: (1.0, 2.5)}


class FilterParams(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("radius", C.c_float), ("alpha", C.c_float), ("pad_", C.c_uint32)]


# rtx_filter_params_default
FILTER_DEFAULTS = {"kind": RTX_FILTER_GAUSSIAN, "radius": 1.5, "alpha": 2.0, "pad_": 0}

# feature-guided upsampling (rtx_frame_scaled, rtx_upsample*, rtx_upsample_tiles*, rtx_render_upsampled*)
RTX_UPSAMPLE_SCALE_MAX = 8
RTX_UPSAMPLE_E_MAX = 32.0


class UpsampleParams(C.Structure):
    _fields_ = [("scale", C.c_uint32), ("match_material", C.c_int32), ("demodulate", C.c_int32),
                ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float), ("sigma_plane", C.c_float),
                ("albedo_min", C.c_float), ("refine_threshold", C.c_float)]


class UpsampleStats(C.Structure):
    _fields_ = [("low_width", C.c_uint32), ("low_height", C.c_uint32), ("tiles", C.c_uint32), ("refined_tiles", C.c_uint32),
                ("low_conf_pixels", C.c_uint64), ("low_ms", C.c_double), ("features_ms", C.c_double),
                ("upsample_ms", C.c_double), ("refine_ms", C.c_double), ("closest_rays", C.c_uint64),
                ("shadow_rays", C.c_uint64)]


# rtx_upsample_params_default
UPSAMPLE_DEFAULTS = {"scale": 2, "match_material": 1, "demodulate": 0, "sigma_normal": 0.05, "sigma_albedo": 0.1,
                     "sigma_plane": 0.02, "albedo_min": 1.0 / 64.0, "refine_threshold": 0.5}

# temporal accumulation (rtx_frame_project, rtx_temporal*, rtx_render_temporal*)
RTX_TEMPORAL_HISTORY_MAX = 65536
RTX_TEMPORAL_E_MAX = 32.0


class TemporalParams(C.Structure):
    _fields_ = [("max_history", C.c_uint32), ("match_material", C.c_int32), ("sigma_normal", C.c_float),
                ("sigma_albedo", C.c_float), ("sigma_plane", C.c_float), ("pad_", C.c_uint32)]


class TemporalStats(C.Structure):
    _fields_ = [("frames", C.c_uint32), ("pad_", C.c_uint32), ("render_ms", C.c_double), ("features_ms", C.c_double),
                ("temporal_ms", C.c_double), ("pixels", C.c_uint64), ("live_pixels", C.c_uint64),
                ("history_pixels", C.c_uint64), ("reset_pixels", C.c_uint64), ("closest_rays", C.c_uint64),
                ("shadow_rays", C.c_uint64)]


# rtx_temporal_params_default
TEMPORAL_DEFAULTS = {"max_history": 32, "match_material": 1, "sigma_normal": 0.05, "sigma_albedo": 0.1,
                     "sigma_plane": 0.02, "pad_": 0}

# renders of a caller's rays and the camera models (rtx_render_rays*, rtx_ray_features*, rtx_projection*)
RTX_PROJ_PANORAMA, RTX_PROJ_FISHEYE, RTX_PROJ_ORTHO = 0, 1, 2
PROJ_KINDS = {"panorama": RTX_PROJ_PANORAMA, "fisheye": RTX_PROJ_FISHEYE, "ortho": RTX_PROJ_ORTHO}


class Projection(C.Structure):
    _fields_ = [("kind", C.c_int32), ("fov", C.c_float), ("extent", C.c_float), ("offset_x", C.c_float),
                ("offset_y", C.c_float)]


# rtx_projection_default (fov: 2 pi rounded to float)
PROJECTION_DEFAULTS = {"kind": RTX_PROJ_PANORAMA, "fov": 6.2831854820251465, "extent": 0.0, "offset_x": 0.0, "offset_y": 0.0}

# rtx_pass_params_default
PASS_DEFAULTS = {"passes": 1, "flags": 0, "aperture": 0.0, "focus": 1.0, "target_error": 0.0, "min_passes": 2}

# include/rtx_kat.h
KAT_MOLLER, KAT_SPHERE, KAT_PLANE, KAT_SLAB, KAT_NOISE, KAT_TEXTURE, KAT_SPH_LIGHT, KAT_TRI_LIGHT, \
    KAT_MORTON, KAT_U32, KAT_GI_DIR, KAT_REFRACT, KAT_ANY_TRI, KAT_SPH_LIGHT_SH, KAT_BOX_Q, KAT_SPEC_POW, \
    KAT_BOX_Q8, KAT_PLANE_CLEAR, KAT_LIN_CLEAR, KAT_DARK, KAT_ORDER, KAT_SPEC0 = range(22)
KAT_IN = [16, 11, 11, 13, 3, 16, 9, 11, 3, 1, 6, 7, 17, 9, 19, 2, 25, 21, 28, 26, 37, 26]
KAT_OUT = [2, 5, 5, 3, 1, 3, 3, 3, 1, 2, 3, 3, 1, 3, 2, 1, 2, 6, 6, 7, 7332, 7]
KAT_NAMES = ["moller", "sphere", "plane", "slab", "noise", "texture", "sph_light", "tri_light", "morton", "u32",
             "gi_dir", "refract", "any_tri", "sph_light_sh", "box_q", "spec_pow", "box_q8", "plane_clear", "lin_clear", "dark", "order", "spec0"]

# symbols include/rtx.h declares (checked by tests/test_abi.py)
RTX_SYMBOLS = ["rtx_params_default", "rtx_device_count", "rtx_open", "rtx_upload_scene", "rtx_render",
               "rtx_render_device", "rtx_get_stats", "rtx_get_point_stats", "rtx_get_dark_stats", "rtx_get_order_stats", "rtx_get_premask_stats", "rtx_get_clearlane_stats", "rtx_close", "rtx_last_error", "rtx_kat", "rtx_postprocess",
               "rtx_postprocess_device", "rtx_set_builder", "rtx_set_option", "rtx_group_open", "rtx_group_open_loopback", "rtx_group_open_rccl_self", "rtx_group_size", "rtx_read_wide_tree", "rtx_read_bvh2",
               "rtx_group_set_builder", "rtx_group_set_option", "rtx_group_upload_scene", "rtx_group_render", "rtx_group_get_stats", "rtx_group_device_stats",
               "rtx_group_get_point_stats", "rtx_group_device_point_stats",
               "rtx_group_get_dark_stats", "rtx_group_device_dark_stats",
               "rtx_group_get_order_stats", "rtx_group_device_order_stats",
               "rtx_group_get_premask_stats", "rtx_group_device_premask_stats", "rtx_group_get_clearlane_stats", "rtx_group_device_clearlane_stats",
               "rtx_group_member_info", "rtx_group_close", "rtx_tile_pack_count", "rtx_tile_pack_host", "rtx_tile_unpack_host",
               "rtx_tile_pack_device", "rtx_tile_unpack_device", "rtx_tree_frame",
               "rtx_trace_rays", "rtx_trace_rays_device", "rtx_frame_rays_device", "rtx_get_ray_stats",
               "rtx_trace_shadow_rays", "rtx_get_shadow_ray_stats",
               "rtx_closest_point_object", "rtx_closest_points", "rtx_closest_points_device", "rtx_get_closest_stats",
               "rtx_closest_kat", "rtx_closest_kat_grid",
               "rtx_frame_features_device", "rtx_frame_features", "rtx_denoise_params_default", "rtx_denoise_device",
               "rtx_denoise", "rtx_get_denoise_stats",
               "rtx_denoise_variance_params_default", "rtx_denoise_variance_device", "rtx_denoise_variance",
               "rtx_pass_params_default", "rtx_pass_frame", "rtx_render_passes", "rtx_render_passes_device",
               "rtx_get_pass_stats",
               "rtx_filter_params_default", "rtx_pass_filter_weights", "rtx_render_passes_filtered",
               "rtx_render_passes_filtered_device",
               "rtx_render_tiles", "rtx_render_tiles_device",
               "rtx_render_adaptive", "rtx_render_adaptive_device", "rtx_get_adaptive_stats",
               "rtx_group_render_passes", "rtx_group_get_pass_stats", "rtx_group_render_adaptive",
               "rtx_group_get_adaptive_stats", "rtx_group_get_exchange_stats",
               "rtx_pass_pack_host", "rtx_pass_unpack_host", "rtx_pass_pack_device", "rtx_pass_unpack_device",
               "rtx_upsample_params_default", "rtx_frame_scaled", "rtx_upsample", "rtx_upsample_device",
               "rtx_upsample_tiles", "rtx_upsample_tiles_device", "rtx_render_upsampled", "rtx_render_upsampled_device",
               "rtx_get_upsample_stats",
               "rtx_temporal_params_default", "rtx_frame_project", "rtx_temporal", "rtx_temporal_device",
               "rtx_render_temporal", "rtx_render_temporal_device", "rtx_temporal_reset", "rtx_get_temporal_stats",
               "rtx_render_rays", "rtx_render_rays_device", "rtx_ray_features", "rtx_ray_features_device",
               "rtx_projection_default", "rtx_projection_ray", "rtx_projection_rays_device", "rtx_render_projection",
               "rtx_render_projection_device"]
RTX_SCENE_SYMBOLS = ["rtx_scene_load", "rtx_scene_parse", "rtx_scene_desc_of", "rtx_scene_num_json_objects",
                     "rtx_scene_free", "rtx_scene_last_error", "rtx_frame_setup", "rtx_tiff_write", "rtx_hash_djb",
                     "rtx_params_from_argv", "rtx_stl_write", "rtx_tiff_read_raw", "rtx_buffer_free",
                     "rtx_post_from_argv"]


def declare_scene(lib):
    lib.rtx_scene_load.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]
    lib.rtx_scene_load.restype = C.c_int
    lib.rtx_scene_parse.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_char_p, C.c_char_p,
                                    C.POINTER(C.c_void_p)]
    lib.rtx_scene_parse.restype = C.c_int
    lib.rtx_scene_desc_of.argtypes = [C.c_void_p]
    lib.rtx_scene_desc_of.restype = C.POINTER(SceneDesc)
    lib.rtx_scene_num_json_objects.argtypes = [C.c_void_p]
    lib.rtx_scene_num_json_objects.restype = C.c_uint32
    lib.rtx_scene_free.argtypes = [C.c_void_p]
    lib.rtx_scene_free.restype = None
    lib.rtx_scene_last_error.argtypes = []
    lib.rtx_scene_last_error.restype = C.c_char_p
    lib.rtx_frame_setup.argtypes = [C.POINTER(Camera), C.c_uint32, C.c_uint32, C.POINTER(Frame)]
    lib.rtx_frame_setup.restype = C.c_int
    lib.rtx_tiff_write.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int]
    lib.rtx_tiff_write.restype = C.c_int
    lib.rtx_hash_djb.argtypes = [C.c_char_p]
    lib.rtx_hash_djb.restype = C.c_uint32
    lib.rtx_params_from_argv.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(Params)]
    lib.rtx_params_from_argv.restype = None
    lib.rtx_stl_write.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p]
    lib.rtx_stl_write.restype = C.c_int
    lib.rtx_tiff_read_raw.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    lib.rtx_tiff_read_raw.restype = C.c_int
    lib.rtx_buffer_free.argtypes = [C.c_void_p]
    lib.rtx_buffer_free.restype = None
    lib.rtx_post_from_argv.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(Post)]
    lib.rtx_post_from_argv.restype = C.c_int


def declare_rtx(lib):
    lib.rtx_params_default.argtypes = [C.POINTER(Params)]
    lib.rtx_params_default.restype = None
    lib.rtx_device_count.argtypes = [C.POINTER(C.c_int)]
    lib.rtx_device_count.restype = C.c_int
    lib.rtx_open.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.rtx_open.restype = C.c_int
    lib.rtx_upload_scene.argtypes = [C.c_void_p, C.POINTER(SceneDesc)]
    lib.rtx_upload_scene.restype = C.c_int
    lib.rtx_render.argtypes = [C.c_void_p, C.POINTER(Frame), C.POINTER(Params), C.c_void_p, C.c_void_p]
    lib.rtx_render.restype = C.c_int
    lib.rtx_render_device.argtypes = [C.c_void_p, C.POINTER(Frame), C.POINTER(Params), C.c_void_p, C.c_void_p,
                                      C.c_void_p]
    lib.rtx_render_device.restype = C.c_int
    lib.rtx_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
    lib.rtx_get_stats.restype = C.c_int
    lib.rtx_get_point_stats.argtypes = [C.c_void_p, C.POINTER(PointStats)]
    lib.rtx_get_point_stats.restype = C.c_int
    lib.rtx_get_dark_stats.argtypes = [C.c_void_p, C.POINTER(DarkStats)]
    lib.rtx_get_dark_stats.restype = C.c_int
    lib.rtx_get_order_stats.argtypes = [C.c_void_p, C.POINTER(OrderStats)]
    lib.rtx_get_order_stats.restype = C.c_int
    lib.rtx_get_premask_stats.argtypes = [C.c_void_p, C.POINTER(PremaskStats)]
    lib.rtx_get_premask_stats.restype = C.c_int
    lib.rtx_get_clearlane_stats.argtypes = [C.c_void_p, C.POINTER(ClearlaneStats)]
    lib.rtx_get_clearlane_stats.restype = C.c_int
    lib.rtx_close.argtypes = [C.c_void_p]
    lib.rtx_close.restype = None
    lib.rtx_last_error.argtypes = []
    lib.rtx_last_error.restype = C.c_char_p
    lib.rtx_kat.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Params)]
    lib.rtx_kat.restype = C.c_int
    lib.rtx_set_builder.argtypes = [C.c_void_p, C.c_int]
    lib.rtx_set_builder.restype = C.c_int
    lib.rtx_set_option.argtypes = [C.c_void_p, C.c_int, C.c_int64]
    lib.rtx_set_option.restype = C.c_int
    lib.rtx_group_set_option.argtypes = [C.c_void_p, C.c_int, C.c_int64]
    lib.rtx_group_set_option.restype = C.c_int
    lib.rtx_postprocess.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(Post), C.c_void_p, C.c_void_p]
    lib.rtx_postprocess.restype = C.c_int
    lib.rtx_postprocess_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(Post), C.c_void_p,
                                           C.c_void_p, C.c_void_p]
    lib.rtx_postprocess_device.restype = C.c_int
    lib.rtx_group_open.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.rtx_group_open.restype = C.c_int
    lib.rtx_read_wide_tree.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p]
    lib.rtx_read_wide_tree.restype = C.c_int
    lib.rtx_read_bvh2.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                  C.POINTER(C.c_uint32), C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p]
    lib.rtx_read_bvh2.restype = C.c_int
    lib.rtx_group_open_loopback.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.rtx_group_open_loopback.restype = C.c_int
    lib.rtx_group_open_rccl_self.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.rtx_group_open_rccl_self.restype = C.c_int
    lib.rtx_group_size.argtypes = [C.c_void_p]
    lib.rtx_group_size.restype = C.c_int
    lib.rtx_group_set_builder.argtypes = [C.c_void_p, C.c_int]
    lib.rtx_group_set_builder.restype = C.c_int
    lib.rtx_group_upload_scene.argtypes = [C.c_void_p, C.POINTER(SceneDesc)]
    lib.rtx_group_upload_scene.restype = C.c_int
    lib.rtx_group_render.argtypes = [C.c_void_p, C.POINTER(Frame), C.POINTER(Params), C.c_void_p, C.c_void_p]
    lib.rtx_group_render.restype = C.c_int
    lib.rtx_group_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
    lib.rtx_group_get_stats.restype = C.c_int
    lib.rtx_group_device_stats.argtypes = [C.c_void_p, C.c_int, C.POINTER(Stats)]
    lib.rtx_group_device_stats.restype = C.c_int
    lib.rtx_group_get_point_stats.argtypes = [C.c_void_p, C.POINTER(PointStats)]
    lib.rtx_group_get_point_stats.restype = C.c_int
    lib.rtx_group_device_point_stats.argtypes = [C.c_void_p, C.c_int, C.POINTER(PointStats)]
    lib.rtx_group_device_point_stats.restype = C.c_int
    lib.rtx_group_get_dark_stats.argtypes = [C.c_void_p, C.POINTER(DarkStats)]
    lib.rtx_group_get_dark_stats.restype = C.c_int
    lib.rtx_group_device_dark_stats.argtypes = [C.c_void_p, C.c_int, C.POINTER(DarkStats)]
    lib.rtx_group_device_dark_stats.restype = C.c_int
    lib.rtx_group_get_order_stats.argtypes = [C.c_void_p, C.POINTER(OrderStats)]
    lib.rtx_group_get_order_stats.restype = C.c_int
    lib.rtx_group_device_order_stats.argtypes = [C.c_void_p, C.c_int, C.POINTER(OrderStats)]
    lib.rtx_group_device_order_stats.restype = C.c_int
    lib.rtx_group_get_premask_stats.argtypes = [C.c_void_p, C.POINTER(PremaskStats)]
    lib.rtx_group_get_premask_stats.restype = C.c_int
    lib.rtx_group_device_premask_stats.argtypes = [C.c_void_p, C.c_int, C.POINTER(PremaskStats)]
    lib.rtx_group_device_premask_stats.restype = C.c_int
    lib.rtx_group_get_clearlane_stats.argtypes = [C.c_void_p, C.POINTER(ClearlaneStats)]
    lib.rtx_group_get_clearlane_stats.restype = C.c_int
    lib.rtx_group_device_clearlane_stats.argtypes = [C.c_void_p, C.c_int, C.POINTER(ClearlaneStats)]
    lib.rtx_group_device_clearlane_stats.restype = C.c_int
    lib.rtx_group_member_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(GroupMember)]
    lib.rtx_group_member_info.restype = C.c_int
    lib.rtx_group_close.argtypes = [C.c_void_p]
    lib.rtx_group_close.restype = None
    lib.rtx_tile_pack_count.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.rtx_tile_pack_count.restype = C.c_size_t
    lib.rtx_tile_pack_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.c_void_p]
    lib.rtx_tile_pack_host.restype = C.c_int
    lib.rtx_tile_unpack_host.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                         C.c_void_p]
    lib.rtx_tile_unpack_host.restype = C.c_int
    lib.rtx_tile_pack_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.c_uint32, C.c_void_p, C.c_void_p]
    lib.rtx_tile_pack_device.restype = C.c_int
    lib.rtx_tile_unpack_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                           C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rtx_tile_unpack_device.restype = C.c_int
    lib.rtx_tree_frame.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_int), C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_double)]
    lib.rtx_tree_frame.restype = C.c_int
    lib.rtx_trace_rays.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.rtx_trace_rays.restype = C.c_int
    lib.rtx_trace_rays_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.rtx_trace_rays_device.restype = C.c_int
    lib.rtx_frame_rays_device.argtypes = [C.c_void_p, C.POINTER(Frame), C.c_void_p, C.c_void_p]
    lib.rtx_frame_rays_device.restype = C.c_int
    lib.rtx_get_ray_stats.argtypes = [C.c_void_p, C.POINTER(RayStats)]
    lib.rtx_get_ray_stats.restype = C.c_int
    lib.rtx_trace_shadow_rays.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.rtx_trace_shadow_rays.restype = C.c_int
    lib.rtx_get_shadow_ray_stats.argtypes = [C.c_void_p, C.POINTER(ShadowRayStats)]
    lib.rtx_get_shadow_ray_stats.restype = C.c_int
    lib.rtx_closest_point_object.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rtx_closest_point_object.restype = C.c_int
    lib.rtx_closest_points.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.rtx_closest_points.restype = C.c_int
    lib.rtx_closest_points_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.rtx_closest_points_device.restype = C.c_int
    lib.rtx_get_closest_stats.argtypes = [C.c_void_p, C.POINTER(ClosestStats)]
    lib.rtx_get_closest_stats.restype = C.c_int
    lib.rtx_closest_kat.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rtx_closest_kat.restype = C.c_int
    lib.rtx_closest_kat_grid.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.rtx_closest_kat_grid.restype = C.c_int
    lib.rtx_frame_features_device.argtypes = [C.c_void_p, C.POINTER(Frame), C.c_int32, C.c_void_p, C.c_void_p]
    lib.rtx_frame_features_device.restype = C.c_int
    lib.rtx_frame_features.argtypes = [C.c_void_p, C.POINTER(Frame), C.c_int32, C.c_void_p]
    lib.rtx_frame_features.restype = C.c_int
    lib.rtx_render_rays.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p]
    lib.rtx_render_rays.restype = C.c_int
    lib.rtx_render_rays_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(Params), C.c_void_p,
                                           C.c_void_p, C.c_void_p]
    lib.rtx_render_rays_device.restype = C.c_int
    lib.rtx_ray_features.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p]
    lib.rtx_ray_features.restype = C.c_int
    lib.rtx_ray_features_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.rtx_ray_features_device.restype = C.c_int
    lib.rtx_projection_default.argtypes = [C.POINTER(Projection)]
    lib.rtx_projection_default.restype = None
    lib.rtx_projection_ray.argtypes = [C.POINTER(Frame), C.POINTER(Projection), C.c_uint32, C.c_uint32, C.c_void_p]
    lib.rtx_projection_ray.restype = C.c_int
    lib.rtx_projection_rays_device.argtypes = [C.c_void_p, C.POINTER(Frame), C.POINTER(Projection), C.c_void_p, C.c_void_p]
    lib.rtx_projection_rays_device.restype = C.c_int
    lib.rtx_render_projection.argtypes = [C.c_void_p, C.POINTER(Frame), C.POINTER(Projection), C.POINTER(Params), C.c_void_p,
                                          C.c_void_p]
    lib.rtx_render_projection.restype = C.c_int
    lib.rtx_render_projection_device.argtypes = [C.c_void_p, C.POINTER(Frame), C.POINTER(Projection), C.POINTER(Params),
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rtx_render_projection_device.restype = C.c_int
    lib.rtx_denoise_params_default.argtypes = [C.POINTER(DenoiseParams)]
    lib.rtx_denoise_params_default.restype = None
    lib.rtx_denoise_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(DenoiseParams), C.c_void_p, C.c_void_p,
                                       C.c_void_p]
    lib.rtx_denoise_device.restype = C.c_int
    lib.rtx_denoise.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(DenoiseParams), C.c_void_p, C.c_void_p]
    lib.rtx_denoise.restype = C.c_int
    lib.rtx_get_denoise_stats.argtypes = [C.c_void_p, C.POINTER(DenoiseStats)]
    lib.rtx_get_denoise_stats.restype = C.c_int
    lib.rtx_denoise_variance_params_default.argtypes = [C.POINTER(DenoiseVarianceParams)]
    lib.rtx_denoise_variance_params_default.restype = None
    lib.rtx_denoise_variance_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(DenoiseVarianceParams), C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rtx_denoise_variance_device.restype = C.c_int
    lib.rtx_denoise_variance.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(DenoiseVarianceParams), C.c_void_p,
                                         C.c_void_p, C.c_void_p]
    lib.rtx_denoise_variance.restype = C.c_int
    lib.rtx_pass_params_default.argtypes = [C.POINTER(PassParams)]
    lib.rtx_pass_params_default.restype = None
    lib.rtx_pass_frame.argtypes = [C.POINTER(Frame), C.POINTER(PassParams), C.c_uint32, C.POINTER(Frame)]
    lib.rtx_pass_frame.restype = C.c_int
    lib.rtx_render_passes.argtypes = [C.c_void_p, C.POINTER(Frame), C.POINTER(Params), C.POINTER(PassParams), C.c_void_p,
                                      C.c_void_p, C.c_void_p]
    lib.rtx_render_passes.restype = C.c_int
    lib.rtx_render_passes_device.argtypes = [C.c_void_p, C.POINTER(Frame), C.POINTER(Params), C.POINTER(PassParams),
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rtx_render_passes_device.restype = C.c_int
    lib.rtx_get_pass_stats.argtypes = [C.c_void_p, C.POINTER(PassStats)]
    lib.rtx_get_pass_stats.restype = C.c_int
    lib.rtx_filter_params_default.argtypes = [C.POINTER(FilterParams)]
    lib.rtx_filter_params_default.restype = None
    lib.rtx_pass_filter_weights.argtypes = [C.POINTER(PassParams), C.POINTER(FilterParams), C.c_uint32, C.c_void_p, C.c_void_p]
    lib.rtx_pass_filter_weights.restype = C.c_int
    lib.rtx_render_passes_filtered.argtypes = [C.c_void_p, C.POINTER(Frame), C.POINTER(Params), C.POINTER(PassParams),
                                               C.POINTER(FilterParams), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rtx_render_passes_filtered.restype = C.c_int
    lib.rtx_render_passes_filtered_device.argtypes = [C.c_void_p, C.POINTER(Frame), C.POINTER(Params), C.POINTER(PassParams),
                                                      C.POINTER(FilterParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rtx_render_passes_filtered_device.restype = C.c_int
    lib.rtx_render_tiles.argtypes = [C.c_void_p, C.POINTER(Frame), C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_void_p,
                                     C.c_void_p]
    lib.rtx_render_tiles.restype = C.c_int
    lib.rtx_render_tiles_device.argtypes = [C.c_void_p, C.POINTER(Frame), C.POINTER(Params), C.c_void_p, C.c_uint32,
                                            C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rtx_render_tiles_device.restype = C.c_int
    lib.rtx_render_adaptive.argtypes = [C.c_void_p, C.POINTER(Frame), C.POINTER(Params), C.POINTER(PassParams), C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rtx_render_adaptive.restype = C.c_int
    lib.rtx_render_adaptive_device.argtypes = [C.c_void_p, C.POINTER(Frame), C.POINTER(Params), C.POINTER(PassParams),
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rtx_render_adaptive_device.restype = C.c_int
    lib.rtx_get_adaptive_stats.argtypes = [C.c_void_p, C.POINTER(AdaptiveStats)]
    lib.rtx_get_adaptive_stats.restype = C.c_int
    lib.rtx_group_render_passes.argtypes = [C.c_void_p, C.POINTER(Frame), C.POINTER(Params), C.POINTER(PassParams), C.c_void_p,
                                            C.c_void_p, C.c_void_p]
    lib.rtx_group_render_passes.restype = C.c_int
    lib.rtx_group_get_pass_stats.argtypes = [C.c_void_p, C.POINTER(PassStats)]
    lib.rtx_group_get_pass_stats.restype = C.c_int
    lib.rtx_group_render_adaptive.argtypes = [C.c_void_p, C.POINTER(Frame), C.POINTER(Params), C.POINTER(PassParams), C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rtx_group_render_adaptive.restype = C.c_int
    lib.rtx_group_get_adaptive_stats.argtypes = [C.c_void_p, C.POINTER(AdaptiveStats)]
    lib.rtx_group_get_adaptive_stats.restype = C.c_int
    lib.rtx_group_get_exchange_stats.argtypes = [C.c_void_p, C.POINTER(GroupExchangeStats)]
    lib.rtx_group_get_exchange_stats.restype = C.c_int
    lib.rtx_pass_pack_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.c_void_p]
    lib.rtx_pass_pack_host.restype = C.c_int
    lib.rtx_pass_unpack_host.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
    lib.rtx_pass_unpack_host.restype = C.c_int
    lib.rtx_pass_pack_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.c_uint32, C.c_void_p, C.c_void_p]
    lib.rtx_pass_pack_device.restype = C.c_int
    lib.rtx_pass_unpack_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rtx_pass_unpack_device.restype = C.c_int
    lib.rtx_upsample_params_default.argtypes = [C.POINTER(UpsampleParams)]
    lib.rtx_upsample_params_default.restype = None
    lib.rtx_frame_scaled.argtypes = [C.POINTER(Frame), C.c_uint32, C.POINTER(Frame)]
    lib.rtx_frame_scaled.restype = C.c_int
    lib.rtx_upsample.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(UpsampleParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]
    lib.rtx_upsample.restype = C.c_int
    lib.rtx_upsample_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(UpsampleParams), C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rtx_upsample_device.restype = C.c_int
    lib.rtx_upsample_tiles.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_float, C.c_void_p,
                                       C.POINTER(C.c_uint32)]
    lib.rtx_upsample_tiles.restype = C.c_int
    lib.rtx_upsample_tiles_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_float, C.c_void_p,
                                              C.POINTER(C.c_uint32), C.c_void_p]
    lib.rtx_upsample_tiles_device.restype = C.c_int
    lib.rtx_render_upsampled.argtypes = [C.c_void_p, C.POINTER(Frame), C.POINTER(Params), C.POINTER(UpsampleParams), C.c_void_p,
                                         C.c_void_p]
    lib.rtx_render_upsampled.restype = C.c_int
    lib.rtx_render_upsampled_device.argtypes = [C.c_void_p, C.POINTER(Frame), C.POINTER(Params), C.POINTER(UpsampleParams),
                                                C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rtx_render_upsampled_device.restype = C.c_int
    lib.rtx_get_upsample_stats.argtypes = [C.c_void_p, C.POINTER(UpsampleStats)]
    lib.rtx_get_upsample_stats.restype = C.c_int
    lib.rtx_temporal_params_default.argtypes = [C.POINTER(TemporalParams)]
    lib.rtx_temporal_params_default.restype = None
    lib.rtx_frame_project.argtypes = [C.POINTER(Frame), C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(C.c_int)]
    lib.rtx_frame_project.restype = C.c_int
    lib.rtx_temporal.argtypes = [C.c_void_p, C.POINTER(TemporalParams), C.POINTER(Frame), C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.POINTER(Frame)] + [C.c_void_p] * 8
    lib.rtx_temporal.restype = C.c_int
    lib.rtx_temporal_device.argtypes = lib.rtx_temporal.argtypes + [C.c_void_p]
    lib.rtx_temporal_device.restype = C.c_int
    lib.rtx_render_temporal.argtypes = [C.c_void_p, C.POINTER(Frame), C.POINTER(Params), C.POINTER(PassParams),
                                        C.POINTER(TemporalParams)] + [C.c_void_p] * 4
    lib.rtx_render_temporal.restype = C.c_int
    lib.rtx_render_temporal_device.argtypes = lib.rtx_render_temporal.argtypes + [C.c_void_p]
    lib.rtx_render_temporal_device.restype = C.c_int
    lib.rtx_temporal_reset.argtypes = [C.c_void_p]
    lib.rtx_temporal_reset.restype = C.c_int
    lib.rtx_get_temporal_stats.argtypes = [C.c_void_p, C.POINTER(TemporalStats)]
    lib.rtx_get_temporal_stats.restype = C.c_int


def declare_oracle(lib):
    lib.rtx_oracle_params_default.argtypes = [C.POINTER(Params)]
    lib.rtx_oracle_params_default.restype = None
    lib.rtx_oracle_render.argtypes = [C.POINTER(SceneDesc), C.POINTER(Frame), C.POINTER(Params), C.c_void_p,
                                      C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
    lib.rtx_oracle_render.restype = C.c_int
    lib.rtx_oracle_kat.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Params)]
    lib.rtx_oracle_kat.restype = C.c_int
    lib.rtx_oracle_primary.argtypes = [C.POINTER(SceneDesc), C.POINTER(Frame), C.c_void_p, C.c_void_p, C.c_int]
    lib.rtx_oracle_primary.restype = C.c_int
