"""ctypes mirror of include/beifong_hip.h and loader for libbeifong_hip.so.

This is plumbing: the product is the HIP library behind the C ABI.  Loading
fails loudly when the extension is missing — there is no CPU fallback.
"""
import ctypes as C
import math
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libbeifong_hip.so")

BF_OK, BF_ERR_INVALID, BF_ERR_DEVICE, BF_ERR_NOMEM, BF_ERR_UNSUPPORTED = range(5)
BF_BSDF_DIFFUSE, BF_BSDF_ROUGHCONDUCTOR, BF_BSDF_NULL = range(3)
BF_MF_BECKMANN, BF_MF_GGX = range(2)
BF_SHAPE_RECTANGLE, BF_SHAPE_MESH = range(2)
BF_EMITTER_SPOT, BF_EMITTER_AREA, BF_TRANSMITTER_AREA, BF_TRANSMITTER_WIGNER, BF_TRANSMITTER_PHASED, BF_EMITTER_POINT = range(6)
BF_SIGNAL_CW, BF_SIGNAL_PULSE, BF_SIGNAL_LINFMCW = range(3)
BF_SENSOR_FLUXMETER, BF_SENSOR_PERSPECTIVE, BF_RECEIVER_OMNI, BF_RECEIVER_WIGNER, BF_RECEIVER_PHASED, BF_SENSOR_IRRADIANCEMETER, BF_SENSOR_RADIANCEMETER = range(7)
BF_ABI_VERSION = 5          # include/beifong_hip.h: BF_ABI_VERSION
BF_VELEM_FLOATS = 32
BF_SI_FLOATS = 27
BF_MODE_PATH, BF_MODE_RANGE, BF_MODE_TIME, BF_MODE_RECEIVE_RAW, BF_MODE_RECEIVE_IQ = range(5)
BF_COLOR_RGB, BF_COLOR_MONO = range(2)
BF_FLAG_STATS, BF_FLAG_GLOBAL_ATOMICS, BF_FLAG_MEGAKERNEL, BF_FLAG_DOPPLER, BF_FLAG_MIX_RESAMPLE = 1, 2, 4, 8, 16
BF_FLAG_ROLLING, BF_FLAG_TIMING, BF_FLAG_COUNT, BF_FLAG_FAST, BF_FLAG_MOMENT = 32, 64, 128, 256, 512
BF_FLAG_CLASSES = 1024
BF_MAX_CLASSES = 256
BF_FLAG_AOV = 2048
BF_MAX_AOVS = 16
BF_FLAG_EXACT_SUM = 4096
BF_NORMALS_GIVEN, BF_NORMALS_RECOMPUTE = range(2)
BF_SKIN_LINEAR, BF_SKIN_DUAL_QUATERNION = range(2)
BF_VELOCITY_TWIST, BF_VELOCITY_VERTEX, BF_VELOCITY_DIFFERENCE = range(3)
(BF_AOV_DEPTH, BF_AOV_POSITION, BF_AOV_UV, BF_AOV_GEO_NORMAL, BF_AOV_SH_NORMAL, BF_AOV_DP_DU, BF_AOV_DP_DV, BF_AOV_DUV_DX,
 BF_AOV_DUV_DY, BF_AOV_TYPES) = range(10)
# the reference's type names (aov.cpp:96-127) in BF_AOV_* order, and the floats of each
AOV_TYPE_NAMES = ("depth", "position", "uv", "geo_normal", "sh_normal", "dp_du", "dp_dv", "duv_dx", "duv_dy")
AOV_TYPE_FLOATS = (1, 3, 2, 3, 3, 3, 3, 2, 2)

M16 = C.c_float * 16


class bf_material(C.Structure):
    _fields_ = [("type", C.c_uint32), ("twosided", C.c_uint32), ("reflectance", C.c_float),
                ("alpha_u", C.c_float), ("alpha_v", C.c_float), ("distribution", C.c_uint32),
                ("sample_visible", C.c_uint32), ("eta", C.c_float), ("k", C.c_float),
                ("has_specular_reflectance", C.c_uint32), ("back_material", C.c_uint32)]


class bf_shape(C.Structure):
    _fields_ = [("type", C.c_uint32), ("material", C.c_uint32), ("emitter", C.c_int32),
                ("is_sensor", C.c_uint32), ("to_world", M16), ("to_object", M16),
                ("positions", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)),
                ("texcoords", C.POINTER(C.c_float)), ("indices", C.POINTER(C.c_uint32)), ("n_vertices", C.c_uint32), ("n_faces", C.c_uint32),
                ("velocity", M16)]


class bf_phased_array(C.Structure):
    _fields_ = [("velems", C.POINTER(C.c_float)), ("n_velems", C.c_uint32), ("elem_dims", C.c_float * 3)]


class bf_emitter(C.Structure):
    _fields_ = [("type", C.c_uint32), ("shape", C.c_int32), ("to_world", M16), ("to_object", M16),
                ("radiance", C.c_float), ("cutoff_angle_deg", C.c_float), ("beam_width_deg", C.c_float),
                ("signal_type", C.c_uint32), ("amplitude", C.c_float), ("freq_centre", C.c_float),
                ("freq_ext", C.c_float), ("pulse_len", C.c_float), ("prf", C.c_float), ("gain", C.c_float),
                ("resample_freq", C.c_uint32), ("array", bf_phased_array)]


BF_FILTER_RESOLUTION = 31
BF_VARIANT_LEAN, BF_VARIANT_WIDE, BF_VARIANT_FAST, BF_VARIANT_MOMENT, BF_VARIANT_CLASS = 1, 2, 4, 8, 16
BF_VARIANT_AOV = 32
BF_VARIANT_EXACT_SUM = 64


class bf_rfilter(C.Structure):
    _fields_ = [("radius", C.c_float), ("scale", C.c_float), ("border", C.c_uint32), ("block_size", C.c_uint32),
                ("values", C.c_float * (BF_FILTER_RESOLUTION + 1))]


class bf_sensor(C.Structure):
    _fields_ = [("type", C.c_uint32), ("shape", C.c_int32), ("to_world", M16), ("sample_to_camera", M16),
                ("fov_x_deg", C.c_float), ("near_clip", C.c_float), ("far_clip", C.c_float),
                ("film_width", C.c_uint32), ("film_height", C.c_uint32),
                ("shutter_open", C.c_float), ("shutter_open_time", C.c_float),
                ("adc_sampling_start", C.c_float), ("adc_sampling_time", C.c_float),
                ("t_bins", C.c_uint32), ("f_bins", C.c_uint32),
                ("t_bandwidth", C.c_float), ("f_bandwidth", C.c_float),
                ("freq_centre", C.c_float), ("freq_ext", C.c_float), ("gain", C.c_float), ("rx_sig_is_delta", C.c_uint32),
                ("array", bf_phased_array), ("rfilter", bf_rfilter),
                ("window_offset_t", C.c_uint32), ("window_offset_f", C.c_uint32), ("window_t_bins", C.c_uint32), ("window_f_bins", C.c_uint32),
                ("crop_offset_x", C.c_uint32), ("crop_offset_y", C.c_uint32),
                ("rx_signal_type", C.c_uint32), ("rx_pulse_len", C.c_float), ("rx_prf", C.c_float), ("rx_amplitude", C.c_float)]


class bf_physics(C.Structure):
    _fields_ = [("c", C.c_float), ("lambda_min_nm", C.c_float), ("lambda_max_nm", C.c_float)]


class bf_scene_desc(C.Structure):
    _fields_ = [("shapes", C.POINTER(bf_shape)), ("n_shapes", C.c_uint32),
                ("materials", C.POINTER(bf_material)), ("n_materials", C.c_uint32),
                ("emitters", C.POINTER(bf_emitter)), ("n_emitters", C.c_uint32),
                ("sensor", bf_sensor), ("physics", bf_physics)]


class bf_launch(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("color_mode", C.c_uint32), ("n_paths", C.c_uint64),
                ("path_offset", C.c_uint64), ("seed", C.c_uint64), ("max_depth", C.c_int32),
                ("rr_depth", C.c_int32), ("bins", C.c_uint32), ("bins_y", C.c_uint32), ("bin_width", C.c_float),
                ("time_c", C.c_float), ("flags", C.c_uint32), ("phase_bins", C.c_uint32),
                ("film_width", C.c_uint32), ("film_height", C.c_uint32), ("spp", C.c_uint32)]


class bf_path_record(C.Structure):
    _fields_ = [("L", C.c_float), ("aux", C.c_float), ("valid", C.c_uint32), ("n_rays", C.c_uint32)]


PATH_RECORD_DTYPE = np.dtype([("L", "<f4"), ("aux", "<f4"), ("valid", "<u4"), ("n_rays", "<u4")])
# the device trees as bf_scene_read_bvh returns them (bf_bvh.h: Node4, Node16)
NODE4_DTYPE = np.dtype([("lox", "<f4", (4,)), ("loy", "<f4", (4,)), ("loz", "<f4", (4,)), ("hix", "<f4", (4,)), ("hiy", "<f4", (4,)),
                        ("hiz", "<f4", (4,)), ("child", "<i4", (4,)), ("pad", "<i4", (4,))])
NODE16_CHILD_DTYPE = np.dtype([("lo", "<f4", (3,)), ("hi", "<f4", (3,)), ("child", "<i4"), ("pad", "<u4")])      # one child record
NODE16_DTYPE = np.dtype([("c", NODE16_CHILD_DTYPE, (16,))])
EMPTY_CHILD = -(1 << 31)


class bf_stats(C.Structure):
    _fields_ = [("n_paths", C.c_uint64), ("n_rays_closest", C.c_uint64), ("n_rays_shadow", C.c_uint64),
                ("n_nodes_visited", C.c_uint64), ("n_tris_tested", C.c_uint64), ("n_invalid", C.c_uint64),
                ("n_bounces", C.c_uint64), ("kernel_ms", C.c_float), ("trace_ms", C.c_float),
                ("shade_ms", C.c_float), ("tail_ms", C.c_float), ("n_launches_trace", C.c_uint32),
                ("n_bounce_iters", C.c_uint32), ("n_rays_tail", C.c_uint64), ("n_rays_traced", C.c_uint64),
                ("n_nodes_lds", C.c_uint64), ("n_nodes_tail", C.c_uint64), ("n_wnodes_tail", C.c_uint64),
                ("n_tris_tail", C.c_uint64), ("n_bounces_tail", C.c_uint64), ("n_shade_loads", C.c_uint64),
                ("n_shade_stores", C.c_uint64), ("n_shade_shadow", C.c_uint64), ("n_shade_rays", C.c_uint64),
                ("n_guard", C.c_uint64), ("n_launches_tail", C.c_uint32), ("n_launches_shade", C.c_uint32),
                ("kernel_variant", C.c_uint32), ("reserved_", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class bf_scene_info(C.Structure):
    _fields_ = [("n_shapes", C.c_uint32), ("n_rects", C.c_uint32), ("n_triangles", C.c_uint32),
                ("n_bvh_nodes", C.c_uint32), ("node_bytes", C.c_uint32), ("tri_bytes", C.c_uint32),
                ("device_bytes", C.c_uint64), ("bbox_min", C.c_float * 3), ("bbox_max", C.c_float * 3),
                ("bvh_depth", C.c_uint32), ("bvh_stack_need", C.c_uint32), ("trace_node_bytes", C.c_uint32), ("device", C.c_int32)]


class bf_batch(C.Structure):
    _fields_ = [("n_renders", C.c_uint32), ("seeds", C.POINTER(C.c_uint64)), ("mesh_offsets", C.POINTER(C.c_float))]


class bf_arrival_bins(C.Structure):
    _fields_ = [("axis_u", C.c_float * 3), ("axis_v", C.c_float * 3), ("u0", C.c_float), ("u1", C.c_float), ("v0", C.c_float),
                ("v1", C.c_float), ("n_u", C.c_uint32), ("n_v", C.c_uint32)]


class bf_twist(C.Structure):
    _fields_ = [("lin", C.c_float * 3), ("ang", C.c_float * 3), ("pivot", C.c_float * 3)]


class bf_range_rate_bins(C.Structure):
    _fields_ = [("sensor_lin", C.c_float * 3), ("r0", C.c_float), ("r1", C.c_float), ("n_bins", C.c_uint32)]


# include/beifong_hip.h: BF_ABI_MATERIAL .. BF_ABI_BATCH, in that order
ABI_STRUCTS = [bf_material, bf_shape, bf_emitter, bf_sensor, bf_scene_desc, bf_launch, bf_path_record, bf_stats, bf_scene_info, bf_batch]

# every symbol include/beifong_hip.h declares
EXPORTED_SYMBOLS = [
    "bf_abi_sizeof", "bf_abi_fingerprint", "bf_version", "bf_last_error", "bf_device_count", "bf_set_device", "bf_scene_create",
    "bf_scene_destroy", "bf_scene_update_endpoints", "bf_scene_translate_meshes", "bf_scene_transform_meshes", "bf_scene_get_info", "bf_scene_clone", "bf_launch_channels", "bf_render_device", "bf_render",
    "bf_scene_flush", "bf_scene_sync", "bf_shard_range", "bf_render_sharded_device", "bf_render_sharded", "bf_allreduce_device",
    "bf_render_batch_device", "bf_render_batch", "bf_render_motion_batch_device", "bf_render_motion_batch",
    "bf_scene_update_vertices", "bf_scene_update_vertices_device", "bf_render_deform_batch_device", "bf_render_deform_batch",
    "bf_scene_set_skin", "bf_scene_pose_skin", "bf_render_skin_batch_device", "bf_render_skin_batch",
    "bf_scene_set_skin_mode", "bf_scene_get_skin_mode", "bf_bone_dual_quaternions",
    "bf_scene_set_morph", "bf_scene_pose_morph", "bf_render_morph_batch_device", "bf_render_morph_batch",
    "bf_vertex_normals", "bf_scene_set_normal_mode", "bf_scene_get_normal_mode",
    "bf_scene_rebuild_bvh", "bf_scene_read_bvh",
    "bf_trace_closest", "bf_trace_any", "bf_ray_intersect", "bf_eval_elementary",
    "bf_bsdf_eval_pdf", "bf_bsdf_eval_pdf_device", "bf_bsdf_sample", "bf_bsdf_sample_device",
    "bf_emitter_sample_direction", "bf_emitter_sample_direction_device", "bf_sensor_sample_ray", "bf_sensor_sample_ray_device",
    "bf_ray_intersect_device", "bf_trace_any_device", "bf_eval_microfacet",
    "bf_render_converge_device", "bf_render_converge", "bf_converge_statistic_device",
    "bf_scene_set_velocity_mode", "bf_scene_get_velocity_mode", "bf_scene_set_vertex_velocities", "bf_scene_set_vertex_velocities_device",
    "bf_scene_set_classes", "bf_scene_set_arrival_classes", "bf_scene_set_range_rate_classes", "bf_scene_launch_channels", "bf_aov_floats", "bf_scene_set_aovs",
    "bf_exact_sum_host", "bf_exact_sum",
]

_lib = None


class BeifongError(RuntimeError):
    pass


def load_library(path=None):
    """dlopen libbeifong_hip.so; raise if it has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("BF_HIP_LIB") or LIB_PATH      # BF_HIP_LIB: developer A/B builds
    if not os.path.exists(p):
        raise BeifongError(
            f"{p} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()'). "
            "There is no CPU fallback.")
    lib = C.CDLL(p)
    vp = C.c_void_p
    lib.bf_version.restype = C.c_int
    if lib.bf_version() != BF_ABI_VERSION:
        raise BeifongError(f"{p}: ABI version {lib.bf_version()}, this binding is for {BF_ABI_VERSION} (include/beifong_hip.h) — rebuild")
    # struct sizes as the library was compiled against this binding's ctypes mirrors (include/beifong_hip.h: bf_abi_sizeof)
    lib.bf_abi_sizeof.argtypes = [C.c_uint32]
    lib.bf_abi_sizeof.restype = C.c_uint32
    for k, t in enumerate(ABI_STRUCTS):
        if lib.bf_abi_sizeof(k) != C.sizeof(t):
            raise BeifongError(f"{p}: sizeof({t.__name__}) is {lib.bf_abi_sizeof(k)} in the library, {C.sizeof(t)} in this binding — "
                               "rebuild (python -c 'import __graft_entry__ as g; g.build()')")
    lib.bf_last_error.restype = C.c_char_p
    lib.bf_device_count.restype = C.c_int
    lib.bf_set_device.argtypes = [C.c_int]
    lib.bf_scene_create.argtypes = [C.POINTER(bf_scene_desc), C.POINTER(vp)]
    lib.bf_scene_destroy.argtypes = [vp]
    lib.bf_scene_get_info.argtypes = [vp, C.POINTER(bf_scene_info)]
    lib.bf_scene_clone.argtypes = [vp, C.POINTER(vp)]
    lib.bf_scene_update_endpoints.argtypes = [vp, C.POINTER(bf_scene_desc), vp]
    lib.bf_scene_translate_meshes.argtypes = [vp, C.POINTER(C.c_float * 3), vp]
    lib.bf_scene_transform_meshes.argtypes = [vp, C.c_uint32, vp, vp]
    lib.bf_launch_channels.argtypes = [C.POINTER(bf_launch)]
    lib.bf_launch_channels.restype = C.c_uint32
    lib.bf_scene_set_classes.argtypes = [vp, C.c_uint32, vp, C.c_uint32, vp]
    lib.bf_scene_set_arrival_classes.argtypes = [vp, C.POINTER(bf_arrival_bins), vp]
    lib.bf_scene_set_range_rate_classes.argtypes = [vp, C.POINTER(bf_range_rate_bins), vp, vp]
    lib.bf_scene_set_velocity_mode.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_float]
    lib.bf_scene_get_velocity_mode.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
    lib.bf_scene_set_vertex_velocities.argtypes = [vp, C.c_uint32, vp, vp]
    lib.bf_scene_set_vertex_velocities_device.argtypes = [vp, C.c_uint32, vp, vp]
    lib.bf_scene_launch_channels.argtypes = [vp, C.POINTER(bf_launch)]
    lib.bf_scene_launch_channels.restype = C.c_uint32
    lib.bf_aov_floats.argtypes = [C.c_uint32, vp]
    lib.bf_aov_floats.restype = C.c_uint32
    lib.bf_scene_set_aovs.argtypes = [vp, C.c_uint32, vp, vp]
    lib.bf_render_device.argtypes = [vp, C.POINTER(bf_launch), vp, vp, vp, C.POINTER(bf_stats)]
    lib.bf_render.argtypes = [vp, C.POINTER(bf_launch), vp, vp, C.POINTER(bf_stats)]
    lib.bf_scene_flush.argtypes = [vp, vp, C.POINTER(bf_stats)]
    lib.bf_scene_sync.argtypes = [vp]
    lib.bf_shard_range.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.bf_shard_range.restype = None
    lib.bf_render_sharded_device.argtypes = [C.POINTER(vp), C.c_uint32, C.POINTER(bf_launch), C.POINTER(vp), C.POINTER(vp), C.POINTER(bf_stats)]
    lib.bf_render_sharded.argtypes = [C.POINTER(vp), C.c_uint32, C.POINTER(bf_launch), vp, C.POINTER(bf_stats)]
    lib.bf_allreduce_device.argtypes = [C.POINTER(C.c_int), C.c_uint32, C.POINTER(vp), C.c_uint64, C.POINTER(vp)]
    lib.bf_render_batch_device.argtypes = [vp, C.POINTER(bf_launch), C.POINTER(bf_batch), vp, vp, vp, C.POINTER(bf_stats)]
    lib.bf_render_batch.argtypes = [vp, C.POINTER(bf_launch), C.POINTER(bf_batch), vp, vp, C.POINTER(bf_stats)]
    lib.bf_render_motion_batch_device.argtypes = [vp, C.POINTER(bf_launch), C.c_uint32, vp, C.c_uint32, vp, vp, vp, vp, C.POINTER(bf_stats)]
    lib.bf_render_motion_batch.argtypes = [vp, C.POINTER(bf_launch), C.c_uint32, vp, C.c_uint32, vp, vp, vp, C.POINTER(bf_stats)]
    lib.bf_scene_update_vertices.argtypes = [vp, C.c_uint32, vp, vp, vp]
    lib.bf_scene_rebuild_bvh.argtypes = [vp, vp]
    lib.bf_scene_read_bvh.argtypes = [vp, C.c_uint32, vp, C.c_uint64, vp, C.POINTER(C.c_int32)]
    lib.bf_scene_update_vertices_device.argtypes = [vp, C.c_uint32, vp, vp, C.c_float, vp]
    lib.bf_render_deform_batch_device.argtypes = [vp, C.POINTER(bf_launch), C.c_uint32, vp, C.c_uint32, vp, vp, vp, C.c_float, C.c_uint32,
                                                  vp, vp, vp, vp, C.POINTER(bf_stats)]
    lib.bf_render_deform_batch.argtypes = [vp, C.POINTER(bf_launch), C.c_uint32, vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp, vp,
                                           C.POINTER(bf_stats)]
    lib.bf_scene_set_skin.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    lib.bf_scene_pose_skin.argtypes = [vp, C.c_uint32, vp, vp]
    lib.bf_render_skin_batch_device.argtypes = [vp, C.POINTER(bf_launch), C.c_uint32, vp, C.c_uint32, vp, vp, C.c_uint32, vp, vp, vp, vp,
                                                C.POINTER(bf_stats)]
    lib.bf_render_skin_batch.argtypes = [vp, C.POINTER(bf_launch), C.c_uint32, vp, C.c_uint32, vp, vp, C.c_uint32, vp, vp, vp, C.POINTER(bf_stats)]
    lib.bf_vertex_normals.argtypes = [C.c_uint32, vp, C.c_uint32, vp, vp]
    lib.bf_scene_set_skin_mode.argtypes = [vp, C.c_uint32, C.c_uint32]
    lib.bf_scene_get_skin_mode.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.bf_bone_dual_quaternions.argtypes = [C.c_uint32, vp, vp]
    lib.bf_scene_set_normal_mode.argtypes = [vp, C.c_uint32, C.c_uint32]
    lib.bf_scene_get_normal_mode.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.bf_scene_set_morph.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    lib.bf_scene_pose_morph.argtypes = [vp, C.c_uint32, vp, vp, vp]
    lib.bf_render_morph_batch_device.argtypes = [vp, C.POINTER(bf_launch), C.c_uint32, vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp, vp, vp,
                                                 C.POINTER(bf_stats)]
    lib.bf_render_morph_batch.argtypes = [vp, C.POINTER(bf_launch), C.c_uint32, vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp, vp,
                                          C.POINTER(bf_stats)]
    lib.bf_trace_closest.argtypes = [vp, C.c_uint64, vp, vp, vp, vp, vp]
    lib.bf_trace_any.argtypes = [vp, C.c_uint64, vp, vp]
    lib.bf_ray_intersect.argtypes = [vp, C.c_uint64, vp, vp, vp, vp]
    lib.bf_eval_elementary.argtypes = [C.c_int, C.c_uint64, vp, vp]
    lib.bf_exact_sum_host.argtypes = [C.c_uint64, vp, vp, C.c_uint32, vp]
    lib.bf_exact_sum.argtypes = [C.c_uint64, vp, vp, C.c_uint32, C.c_uint32, vp]
    for f in ("bf_bsdf_eval_pdf", "bf_bsdf_sample"):
        getattr(lib, f).argtypes = [vp, C.c_uint64, vp, vp, vp]
        getattr(lib, f + "_device").argtypes = [vp, C.c_uint64, vp, vp, vp, vp]
    lib.bf_emitter_sample_direction.argtypes = [vp, C.c_uint32, C.c_uint64, vp, vp]
    lib.bf_emitter_sample_direction_device.argtypes = [vp, C.c_uint32, C.c_uint64, vp, vp, vp]
    lib.bf_sensor_sample_ray.argtypes = [vp, C.c_uint64, vp, vp]
    lib.bf_sensor_sample_ray_device.argtypes = [vp, C.c_uint64, vp, vp, vp]
    lib.bf_ray_intersect_device.argtypes = [vp, C.c_uint64, vp, vp, vp, vp, vp]
    lib.bf_trace_any_device.argtypes = [vp, C.c_uint64, vp, vp, vp]
    lib.bf_eval_microfacet.argtypes = [C.c_int, C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_uint64, vp, vp]
    lib.bf_render_converge_device.argtypes = [vp, C.POINTER(bf_launch), C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp,
                                              C.POINTER(C.c_uint32), vp, C.POINTER(C.c_uint64), C.POINTER(bf_stats)]
    lib.bf_render_converge.argtypes = [vp, C.POINTER(bf_launch), C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, vp,
                                       C.POINTER(C.c_uint32), vp, C.POINTER(C.c_uint64), C.POINTER(bf_stats)]
    lib.bf_converge_statistic_device.argtypes = [C.POINTER(bf_launch), vp, C.c_float, C.POINTER(C.c_double), C.POINTER(C.c_uint64), vp]
    # test hooks (not in include/beifong_hip.h, not part of the ABI)
    if hasattr(lib, "bfdbg_scene_read_tree"):
        lib.bfdbg_scene_origin_scale.argtypes = [vp, C.POINTER(C.c_float)]
        lib.bfdbg_scene_read_tree.argtypes = [vp, C.c_uint32, C.c_int32, vp, C.c_uint64, vp, vp]
    if hasattr(lib, "bfdbg_scene_generation_waves"):
        lib.bfdbg_scene_generation_waves.argtypes = [vp, C.POINTER(C.c_int)]
    if path is None:
        _lib = lib
    return lib


def check(lib, status, what):
    if status != BF_OK:
        msg = lib.bf_last_error()
        raise BeifongError(f"{what} failed (status {status}): {msg.decode() if msg else ''}")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _rows(a, width, dtype, what):
    """A query's input rows: an array of `dtype` whose last axis is `width` (any leading shape, flattened to [n, width]);
    a wrong dtype or shape is a ValueError before any library call."""
    a = np.asarray(a)
    if a.dtype != dtype:
        raise ValueError(f"{what}: dtype {a.dtype}, expected {np.dtype(dtype)}")
    if a.ndim == 0 or a.shape[-1] != width:
        raise ValueError(f"{what}: shape {a.shape}, expected [..., {width}]")
    return np.ascontiguousarray(a.reshape(-1, width))


def _indices(a, n, what):
    a = np.asarray(a)
    if a.dtype != np.uint32:
        raise ValueError(f"{what}: dtype {a.dtype}, expected uint32")
    a = np.ascontiguousarray(a.reshape(-1))
    if a.size != n:
        raise ValueError(f"{what}: {a.size} indices for {n} queries")
    return a


def _stream(stream):
    return C.c_void_p(stream) if stream else None


def _dev(ptr, what):
    if not isinstance(ptr, int) or isinstance(ptr, bool):
        raise ValueError(f"{what}: a device pointer (int, e.g. tensor.data_ptr()) is expected, got {type(ptr).__name__}")
    return C.c_void_p(ptr) if ptr else None


def vertex_normals(positions, faces, lib=None):
    """bf_vertex_normals: the fp32 statement of recomputed vertex normals (include/beifong_hip.h) on the host, bit for bit what the
    device computes under BF_NORMALS_RECOMPUTE.  positions float32[nv, 3], faces uint32[nf, 3] -> float32[nv, 3].  No device."""
    p = vertex_array(positions, "positions")
    f = np.asarray(faces)
    if f.dtype != np.uint32:
        raise TypeError(f"faces must be uint32, got {f.dtype}")
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"faces must be [nf, 3], got {f.shape}")
    f = np.ascontiguousarray(f)
    out = np.empty_like(p)
    lib = lib or load_library()
    check(lib, lib.bf_vertex_normals(p.shape[0], _ptr(p), f.shape[0], _ptr(f), _ptr(out)), "bf_vertex_normals")
    return out


def bone_dual_quaternions(bones, lib=None):
    """bf_bone_dual_quaternions: the conversion the library applies to a bone table of a shape in BF_SKIN_DUAL_QUATERNION, on the
    host (include/beifong_hip.h; motion.bone_dual_quaternions is its numpy restatement, bit for bit).  bones float32[n_bones, 3, 4],
    every one rigid -> float32[n_bones, 8]: (w, x, y, z) of the rotation, then of the dual part.  No device."""
    b = np.ascontiguousarray(bones, dtype=np.float32)
    if b.ndim != 3 or b.shape[1:] != (3, 4):
        raise ValueError(f"bones must be [n_bones, 3, 4], got {b.shape}")
    out = np.empty((b.shape[0], 8), np.float32)
    lib = lib or load_library()
    check(lib, lib.bf_bone_dual_quaternions(b.shape[0], _ptr(b), _ptr(out)), "bf_bone_dual_quaternions")
    return out


MF_EVAL, MF_PDF, MF_SMITH_G1, MF_SAMPLE = range(4)


def eval_microfacet(op, distribution, alpha_u, alpha_v, sample_visible, rows, lib=None):
    """bf_eval_microfacet: MicrofacetDistribution on the device.  rows float32[..., 8] = wi.xyz, m.xyz, s.xy ->
    float32[n, 4] (op MF_SAMPLE: m.xyz, pdf; otherwise the value in column 0)."""
    rows = _rows(rows, 8, np.float32, "eval_microfacet rows")
    lib = lib or load_library()
    out = np.zeros((rows.shape[0], 4), np.float32)
    check(lib, lib.bf_eval_microfacet(int(op), int(distribution), float(alpha_u), float(alpha_v), int(bool(sample_visible)),
                                      rows.shape[0], _ptr(rows), _ptr(out)), "bf_eval_microfacet")
    return out


def make_launch(mode, n_paths, seed=0, path_offset=0, bins=0, bin_width=0.0, color_mode=BF_COLOR_RGB,
                max_depth=-1, rr_depth=5, time_c=3.0e8, flags=0, bins_y=0, phase_bins=0, film=None, spp=0):
    """film=(width, height), spp: multi-pixel film of the render modes; n_paths is then this call's share of the
    width * height * spp paths of the whole film (path g samples pixel g // spp)."""
    lp = bf_launch()
    if film is not None:
        lp.film_width, lp.film_height, lp.spp = int(film[0]), int(film[1]), int(spp)
    lp.mode, lp.color_mode, lp.n_paths, lp.path_offset, lp.seed = mode, color_mode, n_paths, path_offset, seed
    lp.max_depth, lp.rr_depth, lp.bins, lp.bin_width, lp.time_c, lp.flags = max_depth, rr_depth, bins, bin_width, time_c, flags
    lp.bins_y = bins_y
    lp.phase_bins = phase_bins
    return lp


def _moment_shape(lp):
    """(cells, channels per cell, first-moment offsets, m2_ offsets, offset of W) of a BF_FLAG_MOMENT launch
    (include/beifong_hip.h: the layout at the flag)."""
    if not lp.flags & BF_FLAG_MOMENT:
        raise ValueError("the launch does not carry BF_FLAG_MOMENT")
    if lp.mode == BF_MODE_RECEIVE_RAW:
        return lp.bins * lp.bins_y, 4 + lp.phase_bins, np.array([0]), np.array([3 + lp.phase_bins]), 2
    if lp.mode == BF_MODE_RECEIVE_IQ:
        return lp.bins * lp.bins_y, 5, np.array([0, 1]), np.array([3, 4]), 2
    a = {BF_MODE_PATH: 0, BF_MODE_RANGE: lp.bins, BF_MODE_TIME: 3 * lp.bins}[lp.mode]
    pixels = lp.film_width * lp.film_height if (lp.spp and lp.film_width and lp.film_height) else 1
    first = np.arange(5, 8 + a)                # nested AOVs, nested.X .Y .Z
    return pixels, 11 + 2 * a, first, first + a + 3, 4


def moment_layout(lp):
    """(first, second): flat histogram indices pairing every first-moment channel of a BF_FLAG_MOMENT launch with its m2_
    channel, shape [pixels or ADC cells, pairs].  Render modes pair the nested AOVs and nested.X/.Y/.Z (moment.cpp:39-52),
    receive modes Y (RAW) or I and Q."""
    cells, c, first, second, _ = _moment_shape(lp)
    base = (np.arange(cells, dtype=np.int64) * c)[:, None]
    return base + first[None, :].astype(np.int64), base + second[None, :].astype(np.int64)


def moment_estimate(hist, lp):
    """(mean, var_of_mean, rel_stderr) of every paired channel of a BF_FLAG_MOMENT histogram, in float64, shape as
    moment_layout's.  n = the pixel's or ADC cell's W, or the launch's n_paths for a 1 x 1 film; mean = m1 / n,
    var_of_mean = max(m2 / n - mean^2, 0) / (n - 1), rel_stderr = sqrt(var_of_mean) / |mean| (inf where mean = 0;
    everything nan where n < 2)."""
    cells, c, _, _, w_off = _moment_shape(lp)
    h = np.asarray(hist, np.float64).reshape(-1)
    if h.size != cells * c:
        raise ValueError(f"histogram of {h.size} floats, the launch has {cells * c}")
    first, second = moment_layout(lp)
    receive = lp.mode in (BF_MODE_RECEIVE_RAW, BF_MODE_RECEIVE_IQ)
    n = h[np.arange(cells) * c + w_off][:, None] if (receive or cells > 1) else np.full((1, 1), float(lp.n_paths))
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = h[first] / n
        var = np.maximum(h[second] / n - mean * mean, 0.0) / (n - 1.0)
        rel = np.where(mean != 0.0, np.sqrt(var) / np.abs(mean), np.inf)
    bad = np.broadcast_to(n < 2.0, mean.shape)
    mean, var, rel = (np.where(bad, np.nan, x) for x in (mean, var, rel))
    return mean, var, rel


def converge_layout(lp):
    """(first, second, w): the WATCHED pairs of a BF_FLAG_MOMENT launch, flat histogram indices of shape [cells, pairs], and the
    index of every cell's W, shape [cells, 1].  The pairs of moment_layout restricted by mode: range / time the A nested AOVs
    (not nested.X .Y .Z), path nested.Y, receive RAW Y, receive IQ I and Q."""
    lp = bf_launch.from_buffer_copy(lp)
    lp.flags |= BF_FLAG_MOMENT                 # (the converge entries force the flag on)
    cells, c, _, _, w_off = _moment_shape(lp)
    first, second = moment_layout(lp)
    if lp.mode == BF_MODE_PATH:
        first, second = first[:, 1:2], second[:, 1:2]
    elif lp.mode in (BF_MODE_RANGE, BF_MODE_TIME):
        first, second = first[:, :-3], second[:, :-3]
    return first, second, (np.arange(cells, dtype=np.int64) * c + w_off)[:, None]


def converge_seeds(lp, n_renders):
    """uint64[n_renders]: the seeds of the renders of a converge call on `lp`, render k = round * round_renders + j of the call
    with lp.seed + k * lp.n_paths (mod 2^64).  Path p of a render draws from the stream seed + path_offset + p, so seeds
    n_paths apart give disjoint sample sets where consecutive seeds would share all but one path (include/beifong_hip.h)."""
    return np.array([(lp.seed + k * lp.n_paths) % (1 << 64) for k in range(n_renders)], dtype=np.uint64)


def converge_statistic(hist, lp, floor=0.01):
    """(stat, n_significant) of an accumulated BF_FLAG_MOMENT histogram: the float64 statement of what
    bf_converge_statistic_device computes, and the specification its kernels are held to (include/beifong_hip.h).

    Per watched pair (converge_layout) moment_estimate's definitions with n = the pixel's or cell's W (on a 1 x 1 film the paths
    accumulated so far; moment_estimate itself takes the launch's n_paths there, which is one render's): mean = m1 / n,
    var_of_mean = max(m2 / n - mean^2, 0) / (n - 1), rel = sqrt(var_of_mean) / |mean|.  A pair is significant when
    |m1| >= floor * max |m1| (the maximum over all watched pairs; floor in [0, 1], rounded to fp32 as the C ABI carries it);
    stat = max rel over the significant pairs, n_significant their number.  stat is +inf, never NaN, when no pair is
    significant (max |m1| == 0), when a significant pair has n < 2 (or mean 0, which floor = 0 admits), or when any cell of
    the histogram is not finite (n_significant is then 0)."""
    if not 0.0 <= floor <= 1.0:
        raise ValueError(f"floor {floor} is outside [0, 1]")
    first, second, w = converge_layout(lp)
    cells, c = first.shape[0], {BF_MODE_RECEIVE_RAW: 4 + lp.phase_bins, BF_MODE_RECEIVE_IQ: 5, BF_MODE_PATH: 11, BF_MODE_RANGE: 11 + 2 * lp.bins,
                                BF_MODE_TIME: 11 + 6 * lp.bins}[lp.mode]
    h = np.asarray(hist, np.float32).astype(np.float64).reshape(-1)
    if h.size != cells * c:
        raise ValueError(f"histogram of {h.size} floats, the launch has {cells * c}")
    if not np.all(np.isfinite(h)):
        return np.inf, 0
    m1, m2, n = h[first], h[second], h[w]
    top = np.abs(m1).max()
    sig = (np.abs(m1) >= float(np.float32(floor)) * top) & (top > 0.0)
    n_sig = int(np.count_nonzero(sig))
    if n_sig == 0:
        return np.inf, 0
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = m1 / n
        var = np.maximum(m2 / n - mean * mean, 0.0) / (n - 1.0)
        rel = np.where(mean != 0.0, np.sqrt(var) / np.abs(mean), np.inf)
    rel = np.where(np.broadcast_to(n < 2.0, rel.shape), np.inf, rel)
    return float(rel[sig].max()), n_sig


def split_classes(hist, launch, n_classes, lib=None):
    """A BF_FLAG_CLASSES histogram ([classes * channels], or [..., classes * channels] of a batch) as a view of shape
    [..., n_classes, channels]: block k is the plain layout of `launch` (bf_launch_channels) for the paths of class k."""
    lib = lib or load_library()
    n = lib.bf_launch_channels(C.byref(launch))
    hist = np.asarray(hist)
    n_classes = int(n_classes)
    if n_classes < 1 or hist.shape[-1] != n_classes * n:
        raise ValueError(f"a histogram of {hist.shape[-1]} floats per render is not {n_classes} classes x {n} channels")
    return hist.reshape(hist.shape[:-1] + (n_classes, n))


def arrival_bins(axis_u, axis_v, n_u, n_v, window):
    """bf_arrival_bins: the arrival table of Scene.set_arrival_classes.  axis_u, axis_v: world-space axes, used as given;
    window = (u0, u1, v0, v1): the bins cut [u0, u1) x [v0, v1) into n_u x n_v; n_u * n_v + 1 classes, the last one for the
    directions outside the window."""
    b = bf_arrival_bins()
    au, av = (np.asarray(a, np.float32).reshape(3) for a in (axis_u, axis_v))
    b.axis_u, b.axis_v = (C.c_float * 3)(*au.tolist()), (C.c_float * 3)(*av.tolist())
    b.u0, b.u1, b.v0, b.v1 = (float(np.float32(x)) for x in window)
    b.n_u, b.n_v = int(n_u), int(n_v)
    return b


def arrival_n_classes(bins):
    return int(bins.n_u) * int(bins.n_v) + 1


def arrival_classes(d, bins):
    """The class of a path whose primary ray has direction d (float32[n, 3], world space) under the arrival table `bins`
    (arrival_bins): THE SPECIFICATION of bf_scene_set_arrival_classes, in numpy float32 — every product and sum rounded on its
    own, no FMA:
        u  = (d.x a.x + d.y a.y) + d.z a.z            a = axis_u; v likewise with axis_v
        su = float32(n_u) / (u1 - u0)                 sv likewise
        tu = (u - u0) * su, tv = (v - v0) * sv
        inside = 0 <= tu < n_u and 0 <= tv < n_v      (a NaN is outside)
        class  = uint32(tv) * n_u + uint32(tu) if inside else n_u * n_v
    Returns int64[n]."""
    f = np.float32
    d = np.asarray(d, f).reshape(-1, 3)
    n_u, n_v = int(bins.n_u), int(bins.n_v)
    with np.errstate(all="ignore"):
        def coordinate(axis, lo, hi, n):
            a = [f(x) for x in axis]
            u = (d[:, 0] * a[0] + d[:, 1] * a[1]) + d[:, 2] * a[2]
            s = f(n) / (f(hi) - f(lo))
            return (u - f(lo)) * s
        tu = coordinate(bins.axis_u, bins.u0, bins.u1, n_u)
        tv = coordinate(bins.axis_v, bins.v0, bins.v1, n_v)
        assert tu.dtype == f and tv.dtype == f
        inside = (tu >= f(0)) & (tu < f(n_u)) & (tv >= f(0)) & (tv < f(n_v))
    iu = np.where(inside, tu, f(0)).astype(np.int64)      # (truncation: the values are in [0, n))
    iv = np.where(inside, tv, f(0)).astype(np.int64)
    return np.where(inside, iv * n_u + iu, n_u * n_v)


def arrival_bins_for(sd, n_u, n_v, window):
    """The arrival table whose axes are the sensor's own tangents: the normalised first two columns of the to_world of its
    rectangle (flux meters, receivers) or of the camera itself, computed in float64 and rounded once.  u and v are then the
    direction cosines of the arriving ray against the sensor's x and y axes: 0, 0 is the boresight.  `sd`: a SceneDesc."""
    s = sd.sensor
    m = np.asarray(list(sd.shapes[int(s.shape)].to_world if int(s.shape) >= 0 else s.to_world), np.float64).reshape(4, 4)
    cols = [m[:3, k] / np.linalg.norm(m[:3, k]) for k in (0, 1)]
    return arrival_bins(cols[0].astype(np.float32), cols[1].astype(np.float32), n_u, n_v, window)


def range_rate_bins(window, n_bins, sensor_lin=(0, 0, 0)):
    """bf_range_rate_bins: the range-rate table of Scene.set_range_rate_classes.  window = (r0, r1) in m/s: the bins cut [r0, r1)
    into n_bins; sensor_lin: the radar's own velocity, world space, m/s.  n_bins + 2 classes: the bins, one class for the rates
    outside the window and one for the paths whose first ray leaves the scene."""
    b = bf_range_rate_bins()
    b.sensor_lin = (C.c_float * 3)(*np.asarray(sensor_lin, np.float32).reshape(3).tolist())
    b.r0, b.r1 = (float(np.float32(x)) for x in window)
    b.n_bins = int(n_bins)
    return b


def range_rate_n_classes(bins):
    return int(bins.n_bins) + 2


def range_rate_twists(twists, n_shapes=None):
    """float32[n_shapes, 9]: a list of motion.twist (or an array of them) as one contiguous table [lin | ang | pivot] per shape"""
    t = np.ascontiguousarray(np.asarray(twists, np.float32).reshape(-1, 9))
    if n_shapes is not None and len(t) != int(n_shapes):
        raise ValueError(f"{len(t)} twists for a scene of {int(n_shapes)} shapes")
    return t


def corner_velocities(p_prev, p_next, dt):
    """float32, the shape of p_prev: the corner velocities of BF_VELOCITY_DIFFERENCE from two sets of rendered positions, THE
    SPECIFICATION of the difference in numpy float32: (p_next - p_prev) / dt per component, the difference and the IEEE quotient
    each rounded on its own.  dt: a positive finite float32 (a scalar, or anything that broadcasts)."""
    f = np.float32
    a, b, t = np.asarray(p_prev, f), np.asarray(p_next, f), np.asarray(dt, f)
    with np.errstate(all="ignore"):
        diff = b - a
        v = diff / t
    assert diff.dtype == f and v.dtype == f
    return v


def interpolate_velocity(uv, v0, v1, v2):
    """float32[n, 3]: the velocity at a hit with barycentrics uv (float32[n, 2], bf_ray_intersect's prim_uv) of a triangle whose
    corners, in face order, move with v0, v1, v2 (float32[n, 3] each), THE SPECIFICATION of the interpolation in numpy float32,
    every product, sum and difference rounded on its own, no FMA:
        b0 = (1 - u) - v
        U  = (b0 v0 + u v1) + v v2                        per component"""
    f = np.float32
    uv = np.asarray(uv, f).reshape(-1, 2)
    v0, v1, v2 = (np.asarray(x, f).reshape(-1, 3) for x in (v0, v1, v2))
    u, v = uv[:, 0:1], uv[:, 1:2]
    with np.errstate(all="ignore"):
        b0 = (f(1) - u) - v
        out = (b0 * v0 + u * v1) + v * v2
    assert b0.dtype == f and out.dtype == f
    return out


def range_rates(d, p, shape, bins, twists, vertex_velocity=None, has_velocity=None):
    """float32[n]: rr of range_rate_classes, the range rate of every path's first intersection along its primary ray (whatever
    the row of shape 0 gives where shape < 0: range_rate_classes never looks at it).  vertex_velocity (float32[n, 3],
    interpolate_velocity) and has_velocity (bool[n]): the paths whose first intersection lies on a shape in BF_VELOCITY_VERTEX or
    BF_VELOCITY_DIFFERENCE, and the velocity U interpolated there; for those w = ((lin + c) + U) - sensor_lin."""
    f = np.float32
    d = np.asarray(d, f).reshape(-1, 3)
    p = np.asarray(p, f).reshape(-1, 3)
    shape = np.asarray(shape, np.int64).reshape(-1)
    tw = range_rate_twists(twists)
    hit = shape >= 0
    row = tw[np.where(hit, shape, 0)] if len(tw) else np.zeros((len(shape), 9), f)
    lin, ang, pivot = row[:, 0:3], row[:, 3:6], row[:, 6:9]
    sl = [f(x) for x in bins.sensor_lin]
    with np.errstate(all="ignore"):
        q = np.where(hit[:, None], p, f(0)) - pivot
        c = [ang[:, 1] * q[:, 2] - ang[:, 2] * q[:, 1], ang[:, 2] * q[:, 0] - ang[:, 0] * q[:, 2], ang[:, 0] * q[:, 1] - ang[:, 1] * q[:, 0]]
        w = [(lin[:, k] + c[k]) - sl[k] for k in range(3)]
        if vertex_velocity is not None:
            U = np.asarray(vertex_velocity, f).reshape(-1, 3)
            has = np.ones(len(shape), bool) if has_velocity is None else np.asarray(has_velocity, bool).reshape(-1)
            w = [np.where(has, ((lin[:, k] + c[k]) + U[:, k]) - sl[k], w[k]) for k in range(3)]
        rr = (d[:, 0] * w[0] + d[:, 1] * w[1]) + d[:, 2] * w[2]
    assert rr.dtype == f and q.dtype == f and all(x.dtype == f for x in c + w)
    return rr


def range_rate_classes(d, p, shape, bins, twists, vertex_velocity=None, has_velocity=None):
    """The class of a path whose primary ray has direction d (float32[n, 3]) and first meets shape `shape` (int[n]; < 0: the ray
    leaves the scene) at p (float32[n, 3], world space) under the range-rate table `bins` (range_rate_bins) and `twists`
    (float32[n_shapes, 9], motion.twist): THE SPECIFICATION of bf_scene_set_range_rate_classes, in numpy float32 — every product,
    sum and difference rounded on its own, no FMA:
        q   = p - pivot
        c   = (ang.y q.z - ang.z q.y, ang.z q.x - ang.x q.z, ang.x q.y - ang.y q.x)
        w   = (lin + c) - sensor_lin
        rr  = (d.x w.x + d.y w.y) + d.z w.z               positive: an opening range (range_rates)
        sr  = float32(n_bins) / (r1 - r0)
        t   = (rr - r0) * sr
        class = uint32(t) if 0 <= t < n_bins else n_bins  (a NaN is outside); n_bins + 1 for a miss
    With vertex_velocity (float32[n, 3]: U of interpolate_velocity) the paths of has_velocity (bool[n]; absent: all), those whose
    first intersection lies on a mesh in BF_VELOCITY_VERTEX or BF_VELOCITY_DIFFERENCE (Scene.set_velocity_mode), take
        w   = ((lin + c) + U) - sensor_lin
    Returns int64[n]."""
    f = np.float32
    hit = np.asarray(shape, np.int64).reshape(-1) >= 0
    n_bins = int(bins.n_bins)
    rr = range_rates(d, p, shape, bins, twists, vertex_velocity, has_velocity)
    with np.errstate(all="ignore"):
        sr = f(n_bins) / (f(bins.r1) - f(bins.r0))
        t = (rr - f(bins.r0)) * sr
        assert t.dtype == f
        inside = (t >= f(0)) & (t < f(n_bins))
    k = np.where(inside, t, f(0)).astype(np.int64)      # (truncation: the values are in [0, n_bins))
    return np.where(hit, np.where(inside, k, n_bins), n_bins + 1)


def range_rate_centres(bins):
    """float64[n_bins]: the centre of every bin of the table, in m/s (the monostatic Doppler shift of a centre rr is -2 rr / lambda)"""
    n = int(bins.n_bins)
    return float(bins.r0) + (np.arange(n, dtype=np.float64) + 0.5) * ((float(bins.r1) - float(bins.r0)) / n)


def aov_types(types):
    """A list of BF_AOV_* numbers or of the reference's type names ("depth", "sh_normal", ...) as a uint32 array."""
    out = []
    for t in types:
        if isinstance(t, str):
            if t not in AOV_TYPE_NAMES:
                raise ValueError(f"unknown AOV type {t!r} (one of {', '.join(AOV_TYPE_NAMES)})")
            t = AOV_TYPE_NAMES.index(t)
        out.append(int(t))
    return np.asarray(out, dtype=np.uint32)


def aov_floats(types, lib=None):
    """bf_aov_floats: K, the floats the list occupies in a pixel; 0 for an invalid list."""
    lib = lib or load_library()
    t = np.ascontiguousarray(types, dtype=np.uint32)
    return int(lib.bf_aov_floats(len(t), _ptr(t) if len(t) else None))


def aov_layout(launch, types, lib=None):
    """The pixel of a BF_FLAG_AOV render of `launch` with the AOV table `types` (beifong_hip.h, at the flag):
    {"aovs": [slice per table entry, in table order], "names": {type name: slice of its first entry}, "K": K,
     "nested": slice of the nested integrator's own AOVs (range / time bins), "nested_rgba": slice of nested.R G B A,
     "chan_px": channels per pixel}."""
    lib = lib or load_library()
    t = aov_types(types)
    K = aov_floats(t, lib)
    if K == 0:
        raise ValueError("invalid AOV list")
    px = 1
    if launch.spp and launch.film_width and launch.film_height:
        px = launch.film_width * launch.film_height
    plain = bf_launch(**{f: getattr(launch, f) for f, _ in bf_launch._fields_})
    plain.flags &= ~BF_FLAG_AOV
    n_nested = lib.bf_launch_channels(C.byref(plain)) // px - 5
    slices, names, at = [], {}, 5
    for ty in t:
        sl = slice(at, at + AOV_TYPE_FLOATS[ty])
        slices.append(sl)
        names.setdefault(AOV_TYPE_NAMES[ty], sl)
        at = sl.stop
    return {"aovs": slices, "names": names, "K": K, "nested": slice(5 + K, 5 + K + n_nested),
            "nested_rgba": slice(5 + K + n_nested, 9 + K + n_nested), "chan_px": 9 + K + n_nested}


def _exact_sum_args(cell, value, n_cells):
    c = np.asarray(cell)
    v = np.asarray(value)
    if c.dtype != np.uint32:
        raise ValueError(f"cell: dtype {c.dtype}, expected uint32")
    if v.dtype != np.float32:
        raise ValueError(f"value: dtype {v.dtype}, expected float32")
    c = np.ascontiguousarray(c.reshape(-1))
    v = np.ascontiguousarray(v.reshape(-1))
    if c.size != v.size:
        raise ValueError(f"{c.size} cell indices for {v.size} values")
    return c, v, int(n_cells)


def exact_sum(cell, value, n_cells):
    """The specification of BF_FLAG_EXACT_SUM and of bf_exact_sum(_host): out[c] = fl(sum of value[i] over cell[i] == c), the EXACT sum
    rounded once to fp32, nearest-even, +0.0 for a cell without addends.  Integer arithmetic throughout: every finite fp32 is an integer
    multiple of 2^-149, K[c] = sum of int(value * 2^149) is summed as Python integers (grouped by exponent first: (-1)^s M << shift,
    the same integer), K is rounded to 24 significant bits by shifts and comparisons, and math.ldexp scales the result; a magnitude at
    or above 2^128 - 2^103 is +-inf.  No floating-point addition anywhere.  cell uint32[n], value float32[n] (finite) -> float32[n_cells]."""
    c, v, n_cells = _exact_sum_args(cell, value, n_cells)
    if c.size and int(c.max()) >= n_cells:
        raise ValueError(f"cell index {int(c.max())} is not below n_cells {n_cells}")
    bits = v.view(np.uint32)
    e = (bits >> np.uint32(23)) & np.uint32(0xff)
    if np.any(e == 0xff):
        raise ValueError("value: a non-finite addend")
    f = (bits & np.uint32(0x7fffff)).astype(np.int64)
    M = np.where(e != 0, f | np.int64(0x800000), f)
    M = np.where(bits >> np.uint32(31) != 0, -M, M)
    shift = np.maximum(e, 1).astype(np.int64) - 1      # value = M * 2^(shift - 149) exactly
    # integer sums of the mantissas per (cell, shift): below 2^24 * n, exact in int64 for n < 2^39
    key, inv = np.unique(c.astype(np.int64) * 254 + shift, return_inverse=True)
    part = np.zeros(key.size, np.int64)
    np.add.at(part, inv.reshape(-1), M)
    K = [0] * n_cells
    for k, s in zip(key.tolist(), part.tolist()):
        K[k // 254] += s << (k % 254)
    out = np.zeros(n_cells, np.float32)
    for i, k in enumerate(K):
        a = abs(k)
        if a == 0:
            continue
        sh = max(a.bit_length() - 24, 0)
        m = a >> sh
        if sh:
            rem, half = a & ((1 << sh) - 1), 1 << (sh - 1)
            if rem > half or (rem == half and (m & 1)):
                m += 1
        x = math.ldexp(m, sh - 149)      # exact: m <= 2^24
        if x >= math.ldexp(1.0, 128):
            x = math.inf
        out[i] = np.float32(-x if k < 0 else x)
    return out


def exact_sum_host(cell, value, n_cells, lib=None):
    """bf_exact_sum_host: exact_sum through the engine's accumulator (csrc/bf_sum.h) on the CPU.  No device."""
    c, v, n_cells = _exact_sum_args(cell, value, n_cells)
    out = np.empty(n_cells, np.float32)
    lib = lib or load_library()
    check(lib, lib.bf_exact_sum_host(c.size, _ptr(c), _ptr(v), n_cells, _ptr(out)), "bf_exact_sum_host")
    return out


def exact_sum_device(cell, value, n_cells, in_lds=False, lib=None):
    """bf_exact_sum: exact_sum on the device, through the device functions the BF_FLAG_EXACT_SUM kernels add with and their resolve
    kernel.  in_lds: the workgroups privatise the cells in LDS and flush limbs (where n_cells cells fit), else global limbs."""
    c, v, n_cells = _exact_sum_args(cell, value, n_cells)
    out = np.empty(n_cells, np.float32)
    lib = lib or load_library()
    check(lib, lib.bf_exact_sum(c.size, _ptr(c), _ptr(v), n_cells, 1 if in_lds else 0, _ptr(out)), "bf_exact_sum")
    return out


def shard_range(n_paths, shard, n_shards, lib=None):
    """bf_shard_range: (offset, count) of shard `shard` of `n_shards` — the partition every multi-GPU driver uses
    (beifong_amd.dist.shard_range is the same arithmetic in Python)."""
    lib = lib or load_library()
    off, cnt = C.c_uint64(), C.c_uint64()
    lib.bf_shard_range(n_paths, shard, n_shards, C.byref(off), C.byref(cnt))
    return off.value, cnt.value


def render_sharded(scenes, launch, lib=None):
    """bf_render_sharded: ONE render split over the GPUs of `scenes` (one handle per GPU), host histogram + summed stats."""
    lib = lib or load_library()
    n = scenes[0].channels(launch)
    hist = np.zeros(n, dtype=np.float32)
    st = bf_stats()
    handles = (C.c_void_p * len(scenes))(*[s.handle for s in scenes])
    check(lib, lib.bf_render_sharded(handles, len(scenes), C.byref(launch), _ptr(hist), C.byref(st)), "bf_render_sharded")
    return hist, st


def render_sharded_device(scenes, launch, hist_ptrs, streams=None, lib=None):
    """bf_render_sharded_device: hist_ptrs[g] is a device pointer on scenes[g]'s GPU; all-reduced on completion."""
    lib = lib or load_library()
    handles = (C.c_void_p * len(scenes))(*[s.handle for s in scenes])
    hp = (C.c_void_p * len(scenes))(*[C.c_void_p(int(p)) for p in hist_ptrs])
    sp = (C.c_void_p * len(scenes))(*[C.c_void_p(int(x)) if x else None for x in streams]) if streams is not None else None
    check(lib, lib.bf_render_sharded_device(handles, len(scenes), C.byref(launch), hp, sp, None), "bf_render_sharded_device")


def rigid_table(transforms, n_shapes):
    """The float32[n_shapes, 3, 4] table bf_scene_transform_meshes reads, from a {shape_index: 3x4 or 4x4} dict (shapes
    left out: the identity) or an [n_shapes, 3, 4] array.  Checks shapes and indices only; the library checks rigidity."""
    n_shapes = int(n_shapes)
    if isinstance(transforms, dict):
        xf = np.zeros((n_shapes, 3, 4), np.float32)
        xf[:, :, :3] = np.eye(3, dtype=np.float32)
        for k, m in transforms.items():
            k = int(k)
            if not 0 <= k < n_shapes:
                raise ValueError(f"shape index {k} out of range for a scene of {n_shapes} shapes")
            m = np.asarray(m)
            if m.shape not in ((3, 4), (4, 4)):
                raise ValueError(f"shape {k}: a transform is 3x4 or 4x4, got {m.shape}")
            if m.shape == (4, 4) and not np.array_equal(m[3], [0, 0, 0, 1]):
                raise ValueError(f"shape {k}: the last row of a 4x4 transform must be (0, 0, 0, 1)")
            xf[k] = m[:3].astype(np.float32)
        return xf
    xf = np.asarray(transforms)
    if xf.ndim != 3 or xf.shape[1:] != (3, 4):
        raise ValueError(f"transforms must be [n_shapes, 3, 4], got {xf.shape}")
    if xf.shape[0] != n_shapes:
        raise ValueError(f"{xf.shape[0]} transforms for a scene of {n_shapes} shapes")
    if not np.issubdtype(xf.dtype, np.floating):
        raise TypeError(f"transforms must be floating point, got {xf.dtype}")
    return np.ascontiguousarray(xf, dtype=np.float32)


def motion_tables(transforms, n_shapes, seeds=None):
    """The float32[n_renders, n_shapes, 3, 4] table and uint64[n_renders] seeds (or None) bf_render_motion_batch reads, from an
    [n_renders, n_shapes, 3, 4] array (every render's table checked by rigid_table).  Shapes only; the library checks rigidity."""
    xf = np.asarray(transforms)
    if xf.ndim != 4 or xf.shape[2:] != (3, 4):
        raise ValueError(f"transforms must be [n_renders, n_shapes, 3, 4], got {xf.shape}")
    if xf.shape[0] == 0:
        raise ValueError("transforms: no renders")
    xf = np.stack([rigid_table(xf[k], n_shapes) for k in range(xf.shape[0])])
    sa = None
    if seeds is not None:
        sa = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(-1)
        if sa.size != xf.shape[0]:
            raise ValueError(f"{sa.size} seeds for {xf.shape[0]} renders")
    return np.ascontiguousarray(xf), sa


def vertex_array(a, name, n_vertices=None, n_renders=None):
    """A float32 vertex array for a vertex update, checked: [nv, 3] (or flat [3 nv]) for one update, [K, nv, 3] for a batch.
    float32 only (the rows hold the floats given: nothing is converted behind the caller's back)."""
    a = np.asarray(a)
    if a.dtype != np.float32:
        raise TypeError(f"{name} must be float32, got {a.dtype}")
    if n_renders is None:
        if a.ndim == 1 and a.size % 3 == 0:
            a = a.reshape(-1, 3)
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f"{name} must be [n_vertices, 3], got {a.shape}")
    else:
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"{name} must be [n_renders, n_vertices, 3], got {a.shape}")
        if a.shape[0] != n_renders:
            raise ValueError(f"{name}: {a.shape[0]} slices for {n_renders} renders")
    if n_vertices is not None and a.shape[-2] != n_vertices:
        raise ValueError(f"{name}: {a.shape[-2]} vertices for a mesh of {n_vertices}")
    return np.ascontiguousarray(a)


def _keyed_tables(items, noun, kind, layout, rank_ok, check_one):
    """The check deform_tables, skin_tables and morph_tables share: `items` ({shape: array[K, ...]} or a list of (shape, array) pairs)
    -> (n_renders, uint32 shapes, [check_one(array, name, shape, n_renders)]).  noun ("positions"), kind ("deforming") and layout
    ("[n_renders, n_vertices, 3]") word the refusals; rank_ok(ndim) says whether the first array can be a batch at all."""
    items = list(items.items()) if isinstance(items, dict) else [(k, v) for k, v in items]
    if not items:
        raise ValueError(f"{noun}: no {kind} shape")
    shapes = [int(k) for k, _ in items]
    if len(set(shapes)) != len(shapes):
        raise ValueError(f"a shape is listed twice: {shapes}")
    if any(k < 0 for k in shapes):
        raise ValueError(f"negative shape index in {shapes}")
    first = np.asarray(items[0][1])
    if not rank_ok(first.ndim):
        raise ValueError(f"{noun} of shape {shapes[0]} must be {layout}, got {first.shape}")
    n_renders = first.shape[0]
    if n_renders == 0:
        raise ValueError(f"{noun}: no renders")
    tabs = [check_one(v, f"{noun} of shape {k}", k, n_renders) for k, (_, v) in zip(shapes, items)]
    return n_renders, np.asarray(shapes, np.uint32), tabs


def deform_tables(positions, normals=None, n_vertices=None):
    """What bf_render_deform_batch reads, from {shape: positions[K, nv, 3]} (and {shape: normals[K, nv, 3]} for some or all
    of them): (n_renders, uint32 shapes, [positions arrays], [normals arrays or None] or None).  `positions` may also be a
    list of (shape, array) pairs; a shape listed twice is refused here.  n_vertices: {shape: count} to check against."""
    nv = n_vertices or {}
    n_renders, shape_arr, pos = _keyed_tables(positions, "positions", "deforming", "[n_renders, n_vertices, 3]", lambda d: d == 3,
                                              lambda v, name, k, n: vertex_array(v, name, nv.get(k), n))
    shapes = shape_arr.tolist()
    nrm = None
    if normals is not None:
        for k in normals:
            if int(k) not in shapes:
                raise ValueError(f"normals for shape {k}, which has no positions in this call")
        nrm = [vertex_array(normals[k], f"normals of shape {k}", p.shape[1], n_renders) if k in normals else None for k, p in zip(shapes, pos)]
    return n_renders, shape_arr, pos, nrm


def bone_array(a, name, n_bones=None, n_renders=None):
    """A float32 bone table for a skin pose, checked: [n_bones, 3, 4] for one pose, [K, n_bones, 3, 4] for a batch (a trailing
    12 instead of 3, 4 is taken too).  float32 only, as vertex_array."""
    a = np.asarray(a)
    if a.dtype != np.float32:
        raise TypeError(f"{name} must be float32, got {a.dtype}")
    if a.ndim >= 1 and a.shape[-1] == 12:
        a = a.reshape(a.shape[:-1] + (3, 4))
    want = 3 if n_renders is None else 4
    if a.ndim != want or a.shape[-2:] != (3, 4):
        raise ValueError(f"{name} must be [{'' if n_renders is None else 'n_renders, '}n_bones, 3, 4], got {a.shape}")
    if n_renders is not None and a.shape[0] != n_renders:
        raise ValueError(f"{name}: {a.shape[0]} slices for {n_renders} renders")
    if n_bones is not None and a.shape[-3] != n_bones:
        raise ValueError(f"{name}: {a.shape[-3]} bones for a skin of {n_bones}")
    return np.ascontiguousarray(a)


def skin_tables(bones, n_bones=None):
    """What bf_render_skin_batch reads, from {shape: bones[K, n_bones, 3, 4]} or a list of (shape, array) pairs:
    (n_renders, uint32 shapes, [bone arrays]).  A shape listed twice is refused here.  n_bones: {shape: count} to check against."""
    nb = n_bones or {}
    return _keyed_tables(bones, "bones", "skinned", "[n_renders, n_bones, 3, 4]", lambda d: d >= 3,
                         lambda v, name, k, n: bone_array(v, name, nb.get(k), n))


def weight_array(a, name, n_targets=None, n_renders=None):
    """A float32 weight table for a morph pose, checked: [n_targets] for one pose, [K, n_targets] for a batch.  float32 only, as
    vertex_array."""
    a = np.asarray(a)
    if a.dtype != np.float32:
        raise TypeError(f"{name} must be float32, got {a.dtype}")
    want = 1 if n_renders is None else 2
    if a.ndim != want:
        raise ValueError(f"{name} must be [{'' if n_renders is None else 'n_renders, '}n_targets], got {a.shape}")
    if n_renders is not None and a.shape[0] != n_renders:
        raise ValueError(f"{name}: {a.shape[0]} slices for {n_renders} renders")
    if n_targets is not None and a.shape[-1] != n_targets:
        raise ValueError(f"{name}: {a.shape[-1]} weights for a morph of {n_targets} targets")
    return np.ascontiguousarray(a)


def morph_tables(weights, n_targets=None):
    """What bf_render_morph_batch reads, from {shape: weights[K, n_targets]} or a list of (shape, array) pairs:
    (n_renders, uint32 shapes, [weight arrays]).  A shape listed twice is refused here.  n_targets: {shape: count} to check against."""
    nt = n_targets or {}
    return _keyed_tables(weights, "weights", "morphed", "[n_renders, n_targets]", lambda d: d == 2,
                         lambda v, name, k, n: weight_array(v, name, nt.get(k), n))


class Scene:
    """Device-resident immutable scene (bf_scene)."""

    def __init__(self, desc_holder, lib=None):
        self.lib = lib or load_library()
        self.holder = desc_holder          # keeps numpy arrays alive
        h = C.c_void_p()
        check(self.lib, self.lib.bf_scene_create(C.byref(desc_holder.desc), C.byref(h)), "bf_scene_create")
        self.handle = h

    @classmethod
    def borrow(cls, handle, owner=None, lib=None):
        """A Scene on a bf_scene handle another layer owns (the host layer's Scene): every query and render works on it,
        close() leaves it alone; `owner` is kept alive."""
        s = cls.__new__(cls)
        s.lib = lib or load_library()
        s.holder = owner
        s.handle = C.c_void_p(handle)
        s._borrowed = True
        return s

    def close(self):
        if self.handle and not getattr(self, "_borrowed", False):
            self.lib.bf_scene_destroy(self.handle)
        self.handle = None

    def clone(self):
        """bf_scene_clone: another handle on the same geometry (own endpoint tables, path pool, counters) for another stream."""
        other = Scene.__new__(Scene)
        other.lib = self.lib
        other.holder = self.holder
        h = C.c_void_p()
        check(self.lib, self.lib.bf_scene_clone(self.handle, C.byref(h)), "bf_scene_clone")
        other.handle = h
        other._skin_bones = dict(getattr(self, "_skin_bones", {}))      # skins are shared with clones taken afterwards
        other._morph_targets = dict(getattr(self, "_morph_targets", {}))    # and so are morphs
        return other

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update_endpoints(self, desc_holder, stream=0):
        """bf_scene_update_endpoints: same geometry, new rectangle / emitter / sensor records (no BVH rebuild)."""
        check(self.lib, self.lib.bf_scene_update_endpoints(self.handle, C.byref(desc_holder.desc),
                                                           C.c_void_p(stream) if stream else None),
              "bf_scene_update_endpoints")
        self.holder = desc_holder

    def translate_meshes(self, offset, stream=0):
        """bf_scene_translate_meshes: all triangles to fl(p0 + offset), BVH re-fitted in place."""
        off = (C.c_float * 3)(*[float(x) for x in offset])
        check(self.lib, self.lib.bf_scene_translate_meshes(self.handle, C.byref(off), C.c_void_p(stream) if stream else None),
              "bf_scene_translate_meshes")

    def transform_meshes(self, transforms, stream=0):
        """bf_scene_transform_meshes: mesh shape k rigidly to transforms[k] (absolute from the vertices as created), BVHs
        re-fitted on the device.  `transforms`: {shape_index: 3x4 or 4x4} (shapes left out stay as created) or an
        [n_shapes, 3, 4] array."""
        xf = rigid_table(transforms, self.info().n_shapes)
        check(self.lib, self.lib.bf_scene_transform_meshes(self.handle, xf.shape[0], _ptr(xf), C.c_void_p(stream) if stream else None),
              "bf_scene_transform_meshes")

    def rebuild_bvh(self, stream=None):
        """bf_scene_rebuild_bvh: both trees rebuilt on the device, in place, over the geometry the handle renders now (base
        vertices as last updated, pose on top).  Host-synchronous; results stay bit-identical, traversal gets the tree a new
        Scene of the same vertices would have."""
        check(self.lib, self.lib.bf_scene_rebuild_bvh(self.handle, _stream(stream)), "bf_scene_rebuild_bvh")

    def read_bvh(self, width=4):
        """bf_scene_read_bvh: (nodes, rows, root_child) of the four- or sixteen-wide tree.  nodes: NODE4_DTYPE / NODE16_DTYPE
        array; rows: float32[n_triangles, 3, 4] in leaf order (x, y, z and the primitive / shape / tag word, viewable as
        uint32); root_child: the root's child reference."""
        width = int(width)
        if width not in (4, 16):
            raise ValueError(f"read_bvh: width {width} (4 or 16)")
        dt = NODE4_DTYPE if width == 4 else NODE16_DTYPE
        root = C.c_int32(0)
        n = self.info().n_bvh_nodes
        if width == 16:
            # the sixteen-wide node count is not in bf_scene_info: a call with no buffer is refused with BF_ERR_INVALID and the
            # text "needs <n> bytes", which the header documents as the way to learn the size
            st = self.lib.bf_scene_read_bvh(self.handle, 16, None, 0, None, C.byref(root))
            n = 0
            if st != BF_OK:
                msg = self.lib.bf_last_error().decode()
                m = re.search(r"needs (\d+) bytes", msg)
                if st != BF_ERR_INVALID or not m:
                    check(self.lib, st, "bf_scene_read_bvh")
                n = int(m.group(1)) // dt.itemsize
        nodes = np.zeros(n, dtype=dt)
        rows = np.zeros((self.info().n_triangles, 3, 4), dtype=np.float32)
        check(self.lib, self.lib.bf_scene_read_bvh(self.handle, width, _ptr(nodes) if n else None, nodes.nbytes,
                                                   _ptr(rows) if rows.size else None, C.byref(root)), "bf_scene_read_bvh")
        return nodes, rows, int(root.value)

    def debug_origin_scale(self):
        """test hook bfdbg_scene_origin_scale: the ray-origin bound the handle's boxes are padded for, as a numpy float32"""
        out = C.c_float(0.0)
        check(self.lib, self.lib.bfdbg_scene_origin_scale(self.handle, C.byref(out)), "bfdbg_scene_origin_scale")
        return np.float32(out.value)

    def debug_generation_waves(self):
        """test hook bfdbg_scene_generation_waves: waves per SIMD of the build the handle's latest generation launch of wf_shade ran"""
        out = C.c_int(0)
        check(self.lib, self.lib.bfdbg_scene_generation_waves(self.handle, C.byref(out)), "bfdbg_scene_generation_waves")
        return int(out.value)

    def debug_read_tree(self, which, version=-1):
        """test hook bfdbg_scene_read_tree: (nodes, rows, normals) as the device holds them.  which = 4 / 16: NODE4_DTYPE /
        NODE16_DTYPE nodes, 64: the quantised nodes as uint32[n, 16]; version = -1: the handle's own arrays, k >= 0: geometry
        version k of its last motion / deform batch.  rows, normals: float32[n_triangles, 3, 4] (normals: None if the scene
        has none)."""
        which, version = int(which), int(version)
        if which not in (4, 16, 64):
            raise ValueError(f"debug_read_tree: which {which} (4, 16 or 64)")
        item = {4: NODE4_DTYPE.itemsize, 16: NODE16_DTYPE.itemsize, 64: 64}[which]
        n = 0
        st = self.lib.bfdbg_scene_read_tree(self.handle, which, version, None, 1, None, None)      # learns the size, as read_bvh
        if st != BF_OK:
            m = re.search(r"needs (\d+) bytes", self.lib.bf_last_error().decode())
            if st != BF_ERR_INVALID or not m:
                check(self.lib, st, "bfdbg_scene_read_tree")
            n = int(m.group(1)) // item
        nodes = np.zeros(n, dtype=NODE4_DTYPE if which == 4 else NODE16_DTYPE) if which != 64 else np.zeros((n, 16), np.uint32)
        nt = self.info().n_triangles
        rows = np.zeros((nt, 3, 4), np.float32)
        normals = np.full((nt, 3, 4), np.nan, np.float32)
        check(self.lib, self.lib.bfdbg_scene_read_tree(self.handle, which, version, _ptr(nodes) if n else None, nodes.nbytes,
                                                       _ptr(rows) if nt else None, _ptr(normals) if nt else None), "bfdbg_scene_read_tree")
        if nt == 0 or np.isnan(normals[0, 0, 0]):      # (left alone: the scene has no vertex normals; the library refuses NaN normals)
            normals = None
        return nodes, rows, normals

    def info(self):
        i = bf_scene_info()
        check(self.lib, self.lib.bf_scene_get_info(self.handle, C.byref(i)), "bf_scene_get_info")
        return i

    def channels(self, launch):
        """bf_scene_launch_channels: floats one render of `launch` writes on this handle (bf_launch_channels, times the handle's
        number of classes under BF_FLAG_CLASSES; the AOV layout under BF_FLAG_AOV)."""
        return self.lib.bf_scene_launch_channels(self.handle, C.byref(launch))

    def set_classes(self, shape_class, n_classes=None, miss_class=0, stream=0):
        """bf_scene_set_classes: shape_class[s] is the class of the paths whose first intersection is shape s (rectangles
        included), miss_class the class of the paths whose first ray leaves the scene; n_classes=None: the largest class
        named + 1.  Stream-ordered; BF_FLAG_CLASSES renders then write [n_classes, channels] (split_classes)."""
        sc = np.ascontiguousarray(shape_class, dtype=np.uint32).reshape(-1)
        n_shapes = self.info().n_shapes
        if sc.size != n_shapes:
            raise ValueError(f"shape_class has {sc.size} entries, the scene {n_shapes} shapes")
        if n_classes is None:
            n_classes = max(int(sc.max()) if sc.size else 0, int(miss_class)) + 1
        check(self.lib, self.lib.bf_scene_set_classes(self.handle, int(n_classes), _ptr(sc), int(miss_class), _stream(stream)),
              "bf_scene_set_classes")

    def set_arrival_classes(self, axis_u, axis_v=None, n_u=None, n_v=None, window=None, stream=0):
        """bf_scene_set_arrival_classes: the class of a path is the bin of its primary ray's direction d in the window
        (u0, u1, v0, v1) of (d . axis_u, d . axis_v), cut into n_u x n_v bins; the last of the n_u * n_v + 1 classes takes the
        directions outside (arrival_classes is the rule).  World-space axes: they do not follow update_endpoints.  The first
        argument may be a bf_arrival_bins (arrival_bins, arrival_bins_for) instead.  Replaces a set_classes table and is
        replaced by one; clear_classes clears either.  Returns the number of classes."""
        b = axis_u if isinstance(axis_u, bf_arrival_bins) else arrival_bins(axis_u, axis_v, n_u, n_v, window)
        check(self.lib, self.lib.bf_scene_set_arrival_classes(self.handle, C.byref(b), _stream(stream)), "bf_scene_set_arrival_classes")
        return arrival_n_classes(b)

    def set_range_rate_classes(self, bins, twists, stream=0):
        """bf_scene_set_range_rate_classes: the class of a path is the bin of the range rate of its first intersection along its
        primary ray (range_rate_classes is the rule).  bins: range_rate_bins; twists: one motion.twist per shape, in
        scene-description order (world space: they do not follow transform_meshes or a motion batch).  Classes [bins..., outside,
        miss].  Replaces a set_classes or set_arrival_classes table and is replaced by one; clear_classes clears any.  Returns the
        number of classes."""
        tw = range_rate_twists(twists, self.info().n_shapes)
        check(self.lib, self.lib.bf_scene_set_range_rate_classes(self.handle, C.byref(bins), _ptr(tw), _stream(stream)),
              "bf_scene_set_range_rate_classes")
        return range_rate_n_classes(bins)

    def set_aovs(self, types, stream=0):
        """bf_scene_set_aovs: the AOVs every pixel of a BF_FLAG_AOV render carries behind X Y Z A W, in this order (BF_AOV_*
        numbers or names such as "depth", "sh_normal"; aov_layout names the channels).  An empty list clears the table."""
        t = aov_types(types)
        check(self.lib, self.lib.bf_scene_set_aovs(self.handle, len(t), _ptr(t) if len(t) else None, _stream(stream)), "bf_scene_set_aovs")

    def clear_classes(self, stream=0):
        """bf_scene_set_classes with n_classes = 0: the handle has no class table again."""
        check(self.lib, self.lib.bf_scene_set_classes(self.handle, 0, None, 0, _stream(stream)), "bf_scene_set_classes")

    def render(self, launch, records=False):
        """bf_render: host histogram float32[channels] (+ per-path records, stats)."""
        n = self.channels(launch)
        hist = np.zeros(n, dtype=np.float32)
        rec = np.zeros(launch.n_paths, dtype=PATH_RECORD_DTYPE) if records else None
        st = bf_stats()
        check(self.lib, self.lib.bf_render(self.handle, C.byref(launch), _ptr(hist), _ptr(rec), C.byref(st)), "bf_render")
        return hist, rec, st

    def render_device(self, launch, hist_ptr, stream=0, records_ptr=None, want_stats=False):
        """bf_render_device: accumulate into a device buffer (e.g. a torch tensor's data_ptr)."""
        st = bf_stats() if want_stats else None
        check(self.lib, self.lib.bf_render_device(self.handle, C.byref(launch), C.c_void_p(hist_ptr),
                                                  C.c_void_p(records_ptr) if records_ptr else None,
                                                  C.c_void_p(stream) if stream else None,
                                                  C.byref(st) if st is not None else None), "bf_render_device")
        return st

    def render_converge(self, launch, target, floor=0.01, round_renders=4, min_rounds=1, max_rounds=64, want_stats=True):
        """bf_render_converge: rounds of round_renders moment renders of `launch` (seeds converge_seeds(launch, ...): disjoint paths),
        accumulated on the device until the statistic (converge_statistic) of a round is at or below `target`, plus the one
        round that was in flight by then -> (hist float32[channels with BF_FLAG_MOMENT], rounds, stat_history float64[rounds],
        n_significant, stats).  want_stats=False: stats is None and no round waits for its own statistics."""
        lm = bf_launch.from_buffer_copy(launch)
        lm.flags |= BF_FLAG_MOMENT
        hist = np.zeros(self.channels(lm), dtype=np.float32)
        out = self._converge(self.lib.bf_render_converge, "bf_render_converge", launch, target, floor, round_renders, min_rounds, max_rounds,
                             want_stats, _ptr(hist))
        return (hist,) + out

    def render_converge_device(self, launch, hist_ptr, target, floor=0.01, round_renders=4, min_rounds=1, max_rounds=64, stream=0,
                               want_stats=False):
        """bf_render_converge_device: the same into device memory hist_ptr[channels with BF_FLAG_MOMENT] (zeroed by the call),
        stream-ordered; returns (rounds, stat_history, n_significant, stats) once the last round's statistic has been read."""
        return self._converge(self.lib.bf_render_converge_device, "bf_render_converge_device", launch, target, floor, round_renders, min_rounds,
                              max_rounds, want_stats, _dev(hist_ptr, "hist_ptr"), _stream(stream))

    def _converge(self, fn, what, launch, target, floor, round_renders, min_rounds, max_rounds, want_stats, *buffers):
        rounds, n_sig = C.c_uint32(0), C.c_uint64(0)
        history = np.full(max(int(max_rounds), 1), np.nan)
        st = bf_stats() if want_stats else None
        check(self.lib, fn(self.handle, C.byref(launch), float(target), float(floor), int(round_renders), int(min_rounds), int(max_rounds),
                           *buffers, C.byref(rounds), _ptr(history), C.byref(n_sig), C.byref(st) if st is not None else None), what)
        return rounds.value, history[:rounds.value].copy(), n_sig.value, st

    def converge_statistic_device(self, launch, hist_ptr, floor=0.01, stream=0):
        """bf_converge_statistic_device: the statistic kernels alone on a device histogram in the moment layout of `launch`
        -> (stat, n_significant); waits for the result."""
        stat, n_sig = C.c_double(0.0), C.c_uint64(0)
        check(self.lib, self.lib.bf_converge_statistic_device(C.byref(launch), _dev(hist_ptr, "hist_ptr"), float(floor), C.byref(stat),
                                                              C.byref(n_sig), _stream(stream)), "bf_converge_statistic_device")
        return stat.value, n_sig.value

    def flush(self, stream=0, want_stats=False):
        """bf_scene_flush: finish the paths the handle's rolling renders (BF_FLAG_ROLLING) left alive; with want_stats the
        call waits and returns the whole sequence's bf_stats."""
        st = bf_stats() if want_stats else None
        check(self.lib, self.lib.bf_scene_flush(self.handle, C.c_void_p(stream) if stream else None,
                                                C.byref(st) if st is not None else None), "bf_scene_flush")
        return st

    def sync(self):
        """bf_scene_sync: flush, wait for the handle's work and raise if any render since the last check dropped rays."""
        check(self.lib, self.lib.bf_scene_sync(self.handle), "bf_scene_sync")

    @staticmethod
    def _batch(n_renders, seeds, offsets):
        """bf_batch + the arrays it points to (keep the tuple alive for the duration of the call)."""
        b = bf_batch()
        b.n_renders = int(n_renders)
        sa = oa = None
        if seeds is not None:
            sa = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(-1)
            assert sa.size == b.n_renders, "one seed per render"
            b.seeds = sa.ctypes.data_as(C.POINTER(C.c_uint64))
        if offsets is not None:
            oa = np.ascontiguousarray(offsets, dtype=np.float32).reshape(-1, 3)
            assert oa.shape[0] == b.n_renders, "one mesh offset per render"
            b.mesh_offsets = oa.ctypes.data_as(C.POINTER(C.c_float))
        return b, sa, oa

    def render_batch(self, launch, n_renders, seeds=None, offsets=None, records=False):
        """bf_render_batch: n_renders renders of `launch` in one launch sequence -> float32[n_renders, channels]
        (+ records [n_renders, n_paths], stats)."""
        n = self.channels(launch)
        hist = np.zeros((n_renders, n), dtype=np.float32)
        rec = np.zeros((n_renders, launch.n_paths), dtype=PATH_RECORD_DTYPE) if records else None
        st = bf_stats()
        b, sa, oa = self._batch(n_renders, seeds, offsets)
        check(self.lib, self.lib.bf_render_batch(self.handle, C.byref(launch), C.byref(b), _ptr(hist), _ptr(rec), C.byref(st)),
              "bf_render_batch")
        return hist, rec, st

    def render_batch_device(self, launch, n_renders, hist_ptr, seeds=None, offsets=None, stream=0, records_ptr=None,
                            want_stats=False):
        """bf_render_batch_device: accumulate n_renders renders into hist_ptr[n_renders * channels] (device memory)."""
        st = bf_stats() if want_stats else None
        b, sa, oa = self._batch(n_renders, seeds, offsets)
        check(self.lib, self.lib.bf_render_batch_device(self.handle, C.byref(launch), C.byref(b), C.c_void_p(hist_ptr),
                                                        C.c_void_p(records_ptr) if records_ptr else None,
                                                        C.c_void_p(stream) if stream else None,
                                                        C.byref(st) if st is not None else None), "bf_render_batch_device")
        return st

    # The batches with a geometry version per render (motion, deform, skin, morph) end alike: the host form returns hist / rec / stats
    # of its own, the device form takes the caller's buffers; either way the library's arguments are (handle, launch, n_renders,
    # seeds, the call's own tables, n_shapes, transforms, the outputs).
    def _host_outputs(self, launch, n_renders, records):
        """(hist, rec, bf_stats) of a host-form batch, and the outputs of its call."""
        hist = np.zeros((n_renders, self.channels(launch)), dtype=np.float32)
        rec = np.zeros((n_renders, launch.n_paths), dtype=PATH_RECORD_DTYPE) if records else None
        st = bf_stats()
        return (hist, rec, st), (_ptr(hist), _ptr(rec), C.byref(st))

    @staticmethod
    def _device_outputs(hist_ptr, records_ptr, stream, want_stats):
        """bf_stats (or None) of a device-form batch, and the outputs of its call."""
        st = bf_stats() if want_stats else None
        return st, (C.c_void_p(hist_ptr), C.c_void_p(records_ptr) if records_ptr else None, _stream(stream), C.byref(st) if st is not None else None)

    def _version_batch(self, name, launch, n_renders, sa, tables, xf, outputs):
        check(self.lib, getattr(self.lib, name)(self.handle, C.byref(launch), n_renders, _ptr(sa), *tables, xf.shape[1] if xf is not None else 0,
                                                _ptr(xf), *outputs), name)

    def render_motion_batch(self, launch, transforms, seeds=None, records=False):
        """bf_render_motion_batch: render k moves every mesh shape s to transforms[k, s] (absolute from the geometry as
        created; the handle's own pose is untouched) -> float32[n_renders, channels] (+ records [n_renders, n_paths], stats).
        `transforms`: [n_renders, n_shapes, 3, 4]; `seeds`: one per render, or None for launch.seed everywhere."""
        xf, sa = motion_tables(transforms, self.info().n_shapes, seeds)
        ret, out = self._host_outputs(launch, xf.shape[0], records)
        self._version_batch("bf_render_motion_batch", launch, xf.shape[0], sa, (), xf, out)
        return ret

    def render_motion_batch_device(self, launch, transforms, hist_ptr, seeds=None, stream=0, records_ptr=None, want_stats=False):
        """bf_render_motion_batch_device: accumulate render k of the motion batch into hist_ptr[k * channels ..] (device)."""
        xf, sa = motion_tables(transforms, self.info().n_shapes, seeds)
        st, out = self._device_outputs(hist_ptr, records_ptr, stream, want_stats)
        self._version_batch("bf_render_motion_batch_device", launch, xf.shape[0], sa, (), xf, out)
        return st

    def mesh_vertex_count(self, shape):
        """Vertices of mesh shape `shape` in the description this Scene was created from (None if unknown)."""
        shapes = getattr(self.holder, "shapes", None)
        if shapes is None or not 0 <= int(shape) < len(shapes):
            return None
        return int(shapes[int(shape)].n_vertices)

    def update_vertices(self, shape, positions, normals=None, stream=0):
        """bf_scene_update_vertices: replace the base vertices [nv, 3] float32 (and vertex normals) of mesh shape `shape`;
        the handle's pose is applied on top, the BVHs are re-fitted on the device."""
        shape = int(shape)
        if shape < 0:
            raise ValueError(f"shape index {shape}")
        p = vertex_array(positions, "positions", self.mesh_vertex_count(shape))
        n = vertex_array(normals, "normals", p.shape[0]) if normals is not None else None
        check(self.lib, self.lib.bf_scene_update_vertices(self.handle, shape, _ptr(p), _ptr(n), C.c_void_p(stream) if stream else None),
              "bf_scene_update_vertices")

    def update_vertices_device(self, shape, positions_ptr, normals_ptr, bound, stream=0):
        """bf_scene_update_vertices_device: the same from device arrays (float32 [nv, 3], e.g. a torch tensor's data_ptr(),
        valid until `stream` has run the call); bound >= max |coordinate| is the caller's promise, checked on the device."""
        check(self.lib, self.lib.bf_scene_update_vertices_device(self.handle, int(shape), C.c_void_p(int(positions_ptr)),
                                                                 C.c_void_p(int(normals_ptr)) if normals_ptr else None, float(bound),
                                                                 C.c_void_p(stream) if stream else None), "bf_scene_update_vertices_device")

    def set_normal_mode(self, shape, mode):
        """bf_scene_set_normal_mode: BF_NORMALS_RECOMPUTE makes every later position update of mesh shape `shape` that carries no
        normals recompute them on the device (vertex_normals' arithmetic); BF_NORMALS_GIVEN (the default) keeps or replaces them."""
        shape, mode = int(shape), int(mode)
        if shape < 0 or mode < 0:
            raise ValueError(f"shape index {shape}, mode {mode}")
        check(self.lib, self.lib.bf_scene_set_normal_mode(self.handle, shape, mode), "bf_scene_set_normal_mode")

    def normal_mode(self, shape):
        """bf_scene_get_normal_mode: BF_NORMALS_GIVEN or BF_NORMALS_RECOMPUTE of mesh shape `shape` on this handle."""
        shape = int(shape)
        if shape < 0:
            raise ValueError(f"shape index {shape}")
        mode = C.c_uint32(0)
        check(self.lib, self.lib.bf_scene_get_normal_mode(self.handle, shape, C.byref(mode)), "bf_scene_get_normal_mode")
        return int(mode.value)

    def set_velocity_mode(self, shape, mode, dt=0.0):
        """bf_scene_set_velocity_mode: how mesh shape `shape` moves under a range-rate table (range_rate_classes with
        vertex_velocity= is the rule).  BF_VELOCITY_TWIST (the default): with its twist alone; BF_VELOCITY_VERTEX: plus the
        per-vertex field of set_vertex_velocities; BF_VELOCITY_DIFFERENCE: plus the differences of its rendered positions over
        `dt` seconds (corner_velocities), backward between the moves of a handle, forward between the renders of a batch.  Every
        call with a mode other than BF_VELOCITY_TWIST zeroes the shape's field, a call that repeats the mode (to change dt) included;
        the call waits for the handle's work in flight."""
        shape, mode = int(shape), int(mode)
        if shape < 0 or mode < 0:
            raise ValueError(f"shape index {shape}, mode {mode}")
        check(self.lib, self.lib.bf_scene_set_velocity_mode(self.handle, shape, mode, float(dt)), "bf_scene_set_velocity_mode")

    def get_velocity_mode(self, shape):
        """bf_scene_get_velocity_mode: (BF_VELOCITY_* mode, dt) of mesh shape `shape` on this handle."""
        shape = int(shape)
        if shape < 0:
            raise ValueError(f"shape index {shape}")
        mode, dt = C.c_uint32(0), C.c_float(0)
        check(self.lib, self.lib.bf_scene_get_velocity_mode(self.handle, shape, C.byref(mode), C.byref(dt)), "bf_scene_get_velocity_mode")
        return int(mode.value), float(dt.value)

    def set_vertex_velocities(self, shape, velocities, stream=0, device=False):
        """bf_scene_set_vertex_velocities: the world-space velocity [nv, 3] float32 of every vertex of mesh shape `shape`, which must
        be in BF_VELOCITY_VERTEX (None: zeros).  device=True: `velocities` is the address of a device array (a torch tensor's
        data_ptr(), valid until `stream` has run the call)."""
        shape = int(shape)
        if shape < 0:
            raise ValueError(f"shape index {shape}")
        st = C.c_void_p(stream) if stream else None
        if device:
            check(self.lib, self.lib.bf_scene_set_vertex_velocities_device(self.handle, shape, C.c_void_p(int(velocities)) if velocities else None, st),
                  "bf_scene_set_vertex_velocities_device")
            return
        v = vertex_array(velocities, "velocities", self.mesh_vertex_count(shape)) if velocities is not None else None
        check(self.lib, self.lib.bf_scene_set_vertex_velocities(self.handle, shape, _ptr(v), st), "bf_scene_set_vertex_velocities")

    def set_skin_mode(self, shape, mode):
        """bf_scene_set_skin_mode: BF_SKIN_DUAL_QUATERNION makes every later call that takes bones for mesh shape `shape` blend them
        as unit dual quaternions (motion.apply_skin_dq's arithmetic; the bones must then be rigid); BF_SKIN_LINEAR (the default) is
        motion.apply_skin.  Nothing moves until the next pose."""
        shape, mode = int(shape), int(mode)
        if shape < 0 or mode < 0:
            raise ValueError(f"shape index {shape}, mode {mode}")
        check(self.lib, self.lib.bf_scene_set_skin_mode(self.handle, shape, mode), "bf_scene_set_skin_mode")

    def skin_mode(self, shape):
        """bf_scene_get_skin_mode: BF_SKIN_LINEAR or BF_SKIN_DUAL_QUATERNION of mesh shape `shape` on this handle."""
        shape = int(shape)
        if shape < 0:
            raise ValueError(f"shape index {shape}")
        mode = C.c_uint32(0)
        check(self.lib, self.lib.bf_scene_get_skin_mode(self.handle, shape, C.byref(mode)), "bf_scene_get_skin_mode")
        return int(mode.value)

    def _version_args(self, n_renders, transforms, seeds):
        """The optional transforms and seeds of a deform, skin or morph batch of n_renders, checked against that count."""
        xf = sa = None
        if transforms is not None:
            xf, sa = motion_tables(transforms, self.info().n_shapes, seeds)
            if xf.shape[0] != n_renders:
                raise ValueError(f"{xf.shape[0]} transform tables for {n_renders} renders")
        elif seeds is not None:
            sa = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(-1)
            if sa.size != n_renders:
                raise ValueError(f"{sa.size} seeds for {n_renders} renders")
        return xf, sa

    def render_deform_batch(self, launch, positions, normals=None, transforms=None, seeds=None, records=False):
        """bf_render_deform_batch: render k sees shape s at positions[s][k] ([K, nv, 3] float32 each; normals likewise for
        some or all of them), then every mesh at transforms[k] (None: none) -> float32[K, channels] (+ records, stats)."""
        nv = {int(k): self.mesh_vertex_count(k) for k in (positions.keys() if isinstance(positions, dict) else [k for k, _ in positions])}
        n_renders, shapes, pos, nrm = deform_tables(positions, normals, {k: v for k, v in nv.items() if v is not None})
        xf, sa = self._version_args(n_renders, transforms, seeds)
        pp = (C.c_void_p * len(pos))(*[p.ctypes.data for p in pos])
        np_ = (C.c_void_p * len(pos))(*[(q.ctypes.data if q is not None else None) for q in nrm]) if nrm is not None else None
        ret, out = self._host_outputs(launch, n_renders, records)
        self._version_batch("bf_render_deform_batch", launch, n_renders, sa, (len(pos), _ptr(shapes), pp, np_), xf, out)
        return ret

    def render_deform_batch_device(self, launch, n_renders, positions_ptrs, hist_ptr, bound, normals_ptrs=None, transforms=None, seeds=None,
                                   stream=0, records_ptr=None, want_stats=False):
        """bf_render_deform_batch_device: positions_ptrs = {shape: device pointer to float32 [K, nv, 3]} (normals_ptrs likewise
        for some of them); render k accumulates into hist_ptr[k * channels ..] (device)."""
        shapes = [int(k) for k in positions_ptrs]
        if len(set(shapes)) != len(shapes):
            raise ValueError(f"a shape is listed twice: {shapes}")
        n_renders = int(n_renders)
        xf, sa = self._version_args(n_renders, transforms, seeds)
        sh = np.asarray(shapes, np.uint32)
        pp = (C.c_void_p * len(shapes))(*[int(positions_ptrs[k]) for k in positions_ptrs])
        np_ = None
        if normals_ptrs:
            np_ = (C.c_void_p * len(shapes))(*[(int(normals_ptrs[k]) if normals_ptrs.get(k) else None) for k in positions_ptrs])
        st, out = self._device_outputs(hist_ptr, records_ptr, stream, want_stats)
        self._version_batch("bf_render_deform_batch_device", launch, n_renders, sa, (len(shapes), _ptr(sh), pp, np_, float(bound)), xf, out)
        return st

    def set_skin(self, shape, n_bones, rest_positions=None, index=None, weight=None, rest_normals=None):
        """bf_scene_set_skin: attach a skin to mesh shape `shape`: rest positions float32[nv, 3] (and rest normals, for a mesh with
        vertex normals), bone indices uint32[nv, 4] and weights float32[nv, 4]; deep-copied.  n_bones = 0 removes the skin."""
        shape, n_bones = int(shape), int(n_bones)
        if shape < 0 or n_bones < 0:
            raise ValueError(f"shape index {shape}, {n_bones} bones")
        p = n = ix = w = None
        if n_bones:
            p = vertex_array(rest_positions, "rest_positions", self.mesh_vertex_count(shape))
            n = vertex_array(rest_normals, "rest_normals", p.shape[0]) if rest_normals is not None else None
            ix, w = np.asarray(index), np.asarray(weight)
            if ix.dtype != np.uint32:
                raise TypeError(f"index must be uint32, got {ix.dtype}")
            if w.dtype != np.float32:
                raise TypeError(f"weight must be float32, got {w.dtype}")
            if ix.shape != (p.shape[0], 4) or w.shape != (p.shape[0], 4):
                raise ValueError(f"index and weight must be [{p.shape[0]}, 4], got {ix.shape} and {w.shape}")
            ix, w = np.ascontiguousarray(ix), np.ascontiguousarray(w)
        check(self.lib, self.lib.bf_scene_set_skin(self.handle, shape, n_bones, _ptr(p), _ptr(n), _ptr(ix), _ptr(w)), "bf_scene_set_skin")
        counts = self.__dict__.setdefault("_skin_bones", {})
        counts[shape] = n_bones

    def _skin_bone_count(self, shape):
        return getattr(self, "_skin_bones", {}).get(int(shape)) or None

    def pose_skin(self, shape, bones, stream=0):
        """bf_scene_pose_skin: the base of skinned mesh shape `shape` becomes its rest pose under `bones` (float32[n_bones, 3, 4],
        motion.apply_skin's arithmetic); the handle's pose is applied on top, the BVHs are re-fitted on the device."""
        shape = int(shape)
        if shape < 0:
            raise ValueError(f"shape index {shape}")
        b = bone_array(bones, "bones", self._skin_bone_count(shape))
        check(self.lib, self.lib.bf_scene_pose_skin(self.handle, shape, _ptr(b), _stream(stream)), "bf_scene_pose_skin")

    def _skin_args(self, bones):
        keys = bones.keys() if isinstance(bones, dict) else [k for k, _ in bones]
        nb = {int(k): self._skin_bone_count(k) for k in keys}
        n_renders, shapes, tabs = skin_tables(bones, {k: v for k, v in nb.items() if v is not None})
        return n_renders, shapes, tabs, (C.c_void_p * len(tabs))(*[t.ctypes.data for t in tabs])

    def render_skin_batch(self, launch, bones, transforms=None, seeds=None, records=False):
        """bf_render_skin_batch: render k sees skinned shape s posed by bones[s][k] ([K, n_bones, 3, 4] float32 each), then every
        mesh at transforms[k] (None: none) -> float32[K, channels] (+ records, stats).  The handle itself does not change."""
        n_renders, shapes, tabs, bp = self._skin_args(bones)
        xf, sa = self._version_args(n_renders, transforms, seeds)
        ret, out = self._host_outputs(launch, n_renders, records)
        self._version_batch("bf_render_skin_batch", launch, n_renders, sa, (len(tabs), _ptr(shapes), bp), xf, out)
        return ret

    def render_skin_batch_device(self, launch, bones, hist_ptr, transforms=None, seeds=None, stream=0, records_ptr=None, want_stats=False):
        """bf_render_skin_batch_device: the same (the bone tables stay host arrays) with render k accumulated into
        hist_ptr[k * channels ..] (device)."""
        n_renders, shapes, tabs, bp = self._skin_args(bones)
        xf, sa = self._version_args(n_renders, transforms, seeds)
        st, out = self._device_outputs(hist_ptr, records_ptr, stream, want_stats)
        self._version_batch("bf_render_skin_batch_device", launch, n_renders, sa, (len(tabs), _ptr(shapes), bp), xf, out)
        return st

    def set_morph(self, shape, n_targets, rest_positions=None, delta_positions=None, rest_normals=None, delta_normals=None):
        """bf_scene_set_morph: attach morph targets to mesh shape `shape`: rest positions float32[nv, 3] (and rest normals, for a mesh
        with vertex normals), position deltas float32[n_targets, nv, 3] and optionally normal deltas of the same shape; deep-copied.
        n_targets = 0 removes the morph."""
        shape, n_targets = int(shape), int(n_targets)
        if shape < 0 or n_targets < 0:
            raise ValueError(f"shape index {shape}, {n_targets} targets")
        p = n = dp = dn = None
        if n_targets:
            p = vertex_array(rest_positions, "rest_positions", self.mesh_vertex_count(shape))
            n = vertex_array(rest_normals, "rest_normals", p.shape[0]) if rest_normals is not None else None
            dp = vertex_array(delta_positions, "delta_positions", p.shape[0], n_targets)
            dn = vertex_array(delta_normals, "delta_normals", p.shape[0], n_targets) if delta_normals is not None else None
        check(self.lib, self.lib.bf_scene_set_morph(self.handle, shape, n_targets, _ptr(p), _ptr(n), _ptr(dp), _ptr(dn)), "bf_scene_set_morph")
        counts = self.__dict__.setdefault("_morph_targets", {})
        counts[shape] = n_targets

    def _morph_target_count(self, shape):
        return getattr(self, "_morph_targets", {}).get(int(shape)) or None

    def pose_morph(self, shape, weights, bones=None, stream=0):
        """bf_scene_pose_morph: the base of morphed mesh shape `shape` becomes its rest shape plus the targets weighted by `weights`
        (float32[n_targets], motion.apply_morph's arithmetic), skinned by `bones` (float32[n_bones, 3, 4]) behind that if given;
        the handle's pose is applied on top, the BVHs are re-fitted on the device."""
        shape = int(shape)
        if shape < 0:
            raise ValueError(f"shape index {shape}")
        w = weight_array(weights, "weights", self._morph_target_count(shape))
        b = bone_array(bones, "bones", self._skin_bone_count(shape)) if bones is not None else None
        check(self.lib, self.lib.bf_scene_pose_morph(self.handle, shape, _ptr(w), _ptr(b), _stream(stream)), "bf_scene_pose_morph")

    def _morph_args(self, weights, bones):
        keys = [int(k) for k in (weights.keys() if isinstance(weights, dict) else [k for k, _ in weights])]
        nt = {k: self._morph_target_count(k) for k in keys}
        n_renders, shapes, tabs = morph_tables(weights, {k: v for k, v in nt.items() if v is not None})
        wp = (C.c_void_p * len(tabs))(*[t.ctypes.data for t in tabs])
        btabs, bp = [], None
        if bones:
            bones = {int(k): v for k, v in (bones.items() if isinstance(bones, dict) else bones)}
            if not set(bones) <= set(keys):
                raise ValueError(f"bones for shapes {sorted(bones)}, weights for shapes {sorted(keys)}")
            btabs = [bone_array(bones[k], f"bones of shape {k}", self._skin_bone_count(k), n_renders) if bones.get(k) is not None else None
                     for k in keys]
            bp = (C.c_void_p * len(btabs))(*[t.ctypes.data if t is not None else None for t in btabs])
        return n_renders, shapes, (tabs, btabs), wp, bp

    def render_morph_batch(self, launch, weights, bones=None, transforms=None, seeds=None, records=False):
        """bf_render_morph_batch: render k sees morphed shape s posed by weights[s][k] ([K, n_targets] float32 each) and, for the shapes
        `bones` lists ({shape: [K, n_bones, 3, 4]}), skinned behind that; then every mesh at transforms[k] (None: none)
        -> float32[K, channels] (+ records, stats).  The handle itself does not change."""
        n_renders, shapes, keep, wp, bp = self._morph_args(weights, bones)
        xf, sa = self._version_args(n_renders, transforms, seeds)
        ret, out = self._host_outputs(launch, n_renders, records)
        self._version_batch("bf_render_morph_batch", launch, n_renders, sa, (len(shapes), _ptr(shapes), wp, bp), xf, out)
        return ret

    def render_morph_batch_device(self, launch, weights, hist_ptr, bones=None, transforms=None, seeds=None, stream=0, records_ptr=None,
                                  want_stats=False):
        """bf_render_morph_batch_device: the same (weights and bone tables stay host arrays) with render k accumulated into
        hist_ptr[k * channels ..] (device)."""
        n_renders, shapes, keep, wp, bp = self._morph_args(weights, bones)
        xf, sa = self._version_args(n_renders, transforms, seeds)
        st, out = self._device_outputs(hist_ptr, records_ptr, stream, want_stats)
        self._version_batch("bf_render_morph_batch_device", launch, n_renders, sa, (len(shapes), _ptr(shapes), wp, bp), xf, out)
        return st

    def trace_closest(self, rays):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = rays.shape[0]
        t = np.empty(n, np.float32)
        prim = np.empty(n, np.uint32)
        shape = np.empty(n, np.uint32)
        uv = np.empty((n, 2), np.float32)
        check(self.lib, self.lib.bf_trace_closest(self.handle, n, _ptr(rays), _ptr(t), _ptr(prim), _ptr(shape), _ptr(uv)),
              "bf_trace_closest")
        return t, prim, shape, uv

    def ray_intersect(self, rays):
        """Scene::ray_intersect -> dict of SurfaceInteraction fields (arrays over rays), prim, shape."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = rays.shape[0]
        si = np.empty((n, BF_SI_FLOATS), np.float32)
        prim = np.empty(n, np.uint32)
        shape = np.empty(n, np.uint32)
        check(self.lib, self.lib.bf_ray_intersect(self.handle, n, _ptr(rays), _ptr(si), _ptr(prim), _ptr(shape)),
              "bf_ray_intersect")
        return dict(t=si[:, 0], p=si[:, 1:4], n=si[:, 4:7], sh_n=si[:, 7:10], sh_s=si[:, 10:13], sh_t=si[:, 13:16],
                    wi=si[:, 16:19], prim_uv=si[:, 19:21], dp_du=si[:, 21:24], dp_dv=si[:, 24:27], prim=prim, shape=shape,
                    raw=si)

    def trace_any(self, rays):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = rays.shape[0]
        hit = np.empty(n, np.uint8)
        check(self.lib, self.lib.bf_trace_any(self.handle, n, _ptr(rays), _ptr(hit)), "bf_trace_any")
        return hit

    # ---- plugin-level queries on the device (include/beifong_hip.h: bf_bsdf_eval_pdf ...) --------------------------------
    # Host forms take and return numpy arrays; the _device forms take data_ptr() integers of device buffers the caller
    # allocated (rows as in the header) and a stream, as render_device does, and return nothing (asynchronous).

    def bsdf_eval_pdf(self, materials, wi_wo):
        """BSDF::eval / pdf: materials uint32[n], wi_wo float32[n, 6] (local wi, wo) -> float32[n, 2] = eval, pdf."""
        wi_wo = _rows(wi_wo, 6, np.float32, "bsdf_eval_pdf wi_wo")
        mats = _indices(materials, wi_wo.shape[0], "bsdf_eval_pdf materials")
        out = np.zeros((wi_wo.shape[0], 2), np.float32)
        check(self.lib, self.lib.bf_bsdf_eval_pdf(self.handle, wi_wo.shape[0], _ptr(mats), _ptr(wi_wo), _ptr(out)), "bf_bsdf_eval_pdf")
        return out

    def bsdf_sample(self, materials, wi_u):
        """BSDF::sample: materials uint32[n], wi_u float32[n, 6] = wi.xyz, sample1, sample2.xy -> float32[n, 5] = wo.xyz,
        pdf, weight."""
        wi_u = _rows(wi_u, 6, np.float32, "bsdf_sample wi_u")
        mats = _indices(materials, wi_u.shape[0], "bsdf_sample materials")
        out = np.zeros((wi_u.shape[0], 5), np.float32)
        check(self.lib, self.lib.bf_bsdf_sample(self.handle, wi_u.shape[0], _ptr(mats), _ptr(wi_u), _ptr(out)), "bf_bsdf_sample")
        return out

    def emitter_sample_direction(self, emitter, rows):
        """Emitter::sample_direction of emitter `emitter`: rows float32[n, 5] = ref_p.xyz, sample.xy -> float32[n, 8] = d.xyz,
        dist, pdf, delta, spectrum, pdf_direction."""
        rows = _rows(rows, 5, np.float32, "emitter_sample_direction rows")
        out = np.zeros((rows.shape[0], 8), np.float32)
        check(self.lib, self.lib.bf_emitter_sample_direction(self.handle, int(emitter), rows.shape[0], _ptr(rows), _ptr(out)),
              "bf_emitter_sample_direction")
        return out

    def sensor_sample_ray(self, rows):
        """Sensor::sample_ray: rows float32[n, 4] = film position.xy, aperture.xy -> float32[n, 9] = o.xyz, mint, d.xyz,
        weight, maxt."""
        rows = _rows(rows, 4, np.float32, "sensor_sample_ray rows")
        out = np.zeros((rows.shape[0], 9), np.float32)
        check(self.lib, self.lib.bf_sensor_sample_ray(self.handle, rows.shape[0], _ptr(rows), _ptr(out)), "bf_sensor_sample_ray")
        return out

    def bsdf_eval_pdf_device(self, n, materials_ptr, wi_wo_ptr, out_ptr, stream=0):
        check(self.lib, self.lib.bf_bsdf_eval_pdf_device(self.handle, int(n), _dev(materials_ptr, "materials"), _dev(wi_wo_ptr, "wi_wo"),
                                                         _dev(out_ptr, "out"), _stream(stream)), "bf_bsdf_eval_pdf_device")

    def bsdf_sample_device(self, n, materials_ptr, wi_u_ptr, out_ptr, stream=0):
        check(self.lib, self.lib.bf_bsdf_sample_device(self.handle, int(n), _dev(materials_ptr, "materials"), _dev(wi_u_ptr, "wi_u"),
                                                       _dev(out_ptr, "out"), _stream(stream)), "bf_bsdf_sample_device")

    def emitter_sample_direction_device(self, emitter, n, in_ptr, out_ptr, stream=0):
        check(self.lib, self.lib.bf_emitter_sample_direction_device(self.handle, int(emitter), int(n), _dev(in_ptr, "in"),
                                                                    _dev(out_ptr, "out"), _stream(stream)),
              "bf_emitter_sample_direction_device")

    def sensor_sample_ray_device(self, n, in_ptr, out_ptr, stream=0):
        check(self.lib, self.lib.bf_sensor_sample_ray_device(self.handle, int(n), _dev(in_ptr, "in"), _dev(out_ptr, "out"),
                                                             _stream(stream)), "bf_sensor_sample_ray_device")

    def ray_intersect_device(self, n, rays_ptr, si_ptr, prim_ptr=None, shape_ptr=None, stream=0):
        """bf_ray_intersect_device: rays float32[n, 8] -> si float32[n, BF_SI_FLOATS] (+ prim / shape uint32[n]) on the device."""
        check(self.lib, self.lib.bf_ray_intersect_device(self.handle, int(n), _dev(rays_ptr, "rays"), _dev(si_ptr, "si"),
                                                         _dev(prim_ptr or 0, "prim"), _dev(shape_ptr or 0, "shape"), _stream(stream)),
              "bf_ray_intersect_device")

    def trace_any_device(self, n, rays_ptr, hit_ptr, stream=0):
        """bf_trace_any_device: rays float32[n, 8] -> hit uint8[n] on the device."""
        check(self.lib, self.lib.bf_trace_any_device(self.handle, int(n), _dev(rays_ptr, "rays"), _dev(hit_ptr, "hit"), _stream(stream)),
              "bf_trace_any_device")
