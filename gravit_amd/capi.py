"""ctypes binding of libgvt_hip.so (include/gvt_hip.h) -- the only way the Python host side reaches
the device.  There is NO CPU fallback: a missing library or a failing call raises.
"""
import ctypes as C
import os

import numpy as np

from .layouts import HIT_DTYPE, LIGHT_DTYPE, MATERIAL_DTYPE, RAY_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GVT_HIP_LIB") or os.path.join(HERE, "libgvt_hip.so")  # GVT_HIP_LIB: an alternative build (A/B measurements)

# every symbol include/gvt_hip.h declares
ABI_VERSION = 6  # GVT_HIP_ABI_VERSION of include/gvt_hip.h this file mirrors (tests/test_host_cpu.py compares the two)

SYMBOLS = [
    "gvt_hip_init", "gvt_hip_set_stream", "gvt_hip_synchronize", "gvt_hip_last_error",
    "gvt_hip_mesh_create", "gvt_hip_mesh_destroy", "gvt_hip_trace_ex", "gvt_hip_mesh_get_info", "gvt_hip_mesh_get_normals", "gvt_hip_mesh_update_vertices",
    "gvt_hip_trace", "gvt_hip_intersect", "gvt_hip_occluded",
    "gvt_hip_queue_create", "gvt_hip_queue_destroy", "gvt_hip_queue_reserve", "gvt_hip_queue_clear", "gvt_hip_queue_size",
    "gvt_hip_queue_append", "gvt_hip_queue_append_flags", "gvt_hip_abi_version", "gvt_hip_queue_export", "gvt_hip_trace_queue", "gvt_hip_trace_queue_sink",
    "gvt_hip_camera_generate",
    "gvt_hip_camera_generate_tiled",
    "gvt_hip_camera_filter",
    "gvt_hip_top_create", "gvt_hip_top_destroy", "gvt_hip_top_order", "gvt_hip_top_update", "gvt_hip_shuffle", "gvt_hip_queue_sizes",
    "gvt_hip_fb_create", "gvt_hip_fb_destroy", "gvt_hip_fb_clear", "gvt_hip_fb_download", "gvt_hip_fb_device_ptr",
    "gvt_hip_fb_write_ppm_bytes",
    "gvt_hip_profile", "gvt_hip_stats_read", "gvt_hip_stats_reset", "gvt_hip_set_option", "gvt_hip_is_experiments_build", "gvt_hip_counters_peek", "gvt_hip_visit_stats", "gvt_hip_wide_visit_stats", "gvt_hip_mesh_download_nodes", "gvt_hip_mesh_download_wide", "gvt_hip_mesh_download_clusters", "gvt_hip_mesh_upload_nodes", "gvt_hip_marked_visit_stats", "gvt_hip_image_frame",
    "gvt_hip_math_probe", "gvt_hip_ctx_create", "gvt_hip_ctx_make_current", "gvt_hip_ctx_destroy",
    "gvt_hip_comm_unique_id", "gvt_hip_comm_create", "gvt_hip_hub_create", "gvt_hip_hub_abort", "gvt_hip_hub_destroy", "gvt_hip_comm_create_local",
    "gvt_hip_comm_destroy", "gvt_hip_comm_rank", "gvt_hip_comm_world", "gvt_hip_comm_count", "gvt_hip_comm_reserved_cus", "gvt_hip_comm_set_deadline_ms", "gvt_hip_comm_selftest",
    "gvt_hip_tracer_create", "gvt_hip_tracer_destroy", "gvt_hip_tracer_set_camera", "gvt_hip_tracer_set_transforms", "gvt_hip_tracer_set_domains", "gvt_hip_tracer_frame",
    "gvt_hip_volume_create", "gvt_hip_volume_destroy", "gvt_hip_volume_get_info", "gvt_hip_volume_set_transfer", "gvt_hip_volume_trace",
    "gvt_hip_shuffle_volume", "gvt_hip_volume_frame",
    "gvt_hip_volume_set_surfaces", "gvt_hip_volume_set_lights", "gvt_hip_volume_get_crossings",
    "gvt_hip_volume_set_shading", "gvt_hip_volume_get_shading", "gvt_hip_volume_get_shaded",
    "gvt_hip_volume_update_samples",
    "gvt_hip_volume_create_typed", "gvt_hip_volume_update_samples_typed", "gvt_hip_volume_get_voxel_type",
    "gvt_hip_depth_create", "gvt_hip_depth_destroy", "gvt_hip_depth_clear", "gvt_hip_depth_upload", "gvt_hip_depth_download", "gvt_hip_depth_render",
    "gvt_hip_volume_frame_clipped", "gvt_hip_fb_composite_over",
    "gvt_hip_volume_set_subgrids", "gvt_hip_volume_get_amr_info", "gvt_hip_volume_update_amr",
    "gvt_hip_volume_march_queue", "gvt_hip_volume_camera_filter", "gvt_hip_queues_export_wire", "gvt_hip_queues_append_wire",
    "gvt_hip_volume_set_ghosts", "gvt_hip_volume_set_gradient", "gvt_hip_volume_get_gradient",
    "gvt_hip_volume_frame_fused", "gvt_hip_volume_frame_fused_shaded", "gvt_hip_volume_frame_fused_amr",
    "gvt_hip_volume_frame_shadowed",
    "gvt_hip_volume_light_grid_bake", "gvt_hip_volume_light_grid_download", "gvt_hip_volume_light_grid_info", "gvt_hip_volume_light_grid_release",
    "gvt_hip_volume_frame_fog_shadowed",
    "gvt_hip_volume_occluder_grid_bake", "gvt_hip_volume_occluder_grid_download", "gvt_hip_volume_occluder_grid_info", "gvt_hip_volume_occluder_grid_release",
    "gvt_hip_volume_frame_mesh_shadowed",
    "gvt_hip_volume_ao_grid_bake", "gvt_hip_volume_ao_grid_download", "gvt_hip_volume_ao_grid_info", "gvt_hip_volume_ao_grid_release",
    "gvt_hip_volume_frame_ao",
]


class GvtHipError(RuntimeError):
    pass


class MeshInfo(C.Structure):
    _fields_ = [("n_tris", C.c_uint64), ("n_verts", C.c_uint64), ("n_nodes", C.c_uint64), ("n_leaves", C.c_uint64),
                ("bbox_lo", C.c_float * 3), ("bbox_hi", C.c_float * 3), ("build_ms", C.c_float), ("max_leaf", C.c_uint32),
                ("packet", C.c_uint32), ("bytes_nodes", C.c_uint64), ("bytes_tris", C.c_uint64), ("sah_inner", C.c_float), ("pad", C.c_float)]


class CameraPod(C.Structure):
    _fields_ = [("eye", C.c_float * 3), ("focus", C.c_float * 3), ("up", C.c_float * 3), ("fov", C.c_float), ("width", C.c_int32),
                ("height", C.c_int32), ("samples", C.c_int32), ("depth", C.c_int32), ("jitter_window_size", C.c_float)]


class FrameStats(C.Structure):
    _fields_ = [("rounds", C.c_uint64), ("chains", C.c_uint64), ("host_syncs", C.c_uint64), ("rays_sent", C.c_uint64),
                ("rays_closest", C.c_uint64), ("rays_any", C.c_uint64), ("packets_bailed", C.c_uint64), ("bytes_sent", C.c_uint64),
                ("ms_chain", C.c_double), ("ms_announce", C.c_double), ("ms_payload", C.c_double), ("ms_composite", C.c_double), ("ms_host_wait", C.c_double),
                ("exchanges", C.c_uint64), ("rays_inline", C.c_uint64), ("early_deposit_launches", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class VolumeInfo(C.Structure):
    _fields_ = [("box_lo", C.c_float * 3), ("box_hi", C.c_float * 3), ("dt", C.c_float), ("value_min", C.c_float), ("value_max", C.c_float),
                ("blocks", C.c_int32 * 3), ("pad", C.c_float), ("n_blocks", C.c_uint64), ("n_blocks_empty", C.c_uint64),
                ("samples_marched", C.c_uint64), ("samples_gathered", C.c_uint64)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k in ("box_lo", "box_hi", "blocks") else getattr(self, k)) for k, _ in self._fields_ if k != "pad"}


class SubgridPod(C.Structure):
    """gvt_hip_subgrid: one refined subgrid of an AMR volume."""
    _fields_ = [("parent", C.c_int32), ("ratio", C.c_int32), ("lo", C.c_int32 * 3), ("cells", C.c_int32 * 3)]


class VolumeAmrInfo(C.Structure):
    _fields_ = [("n_subgrids", C.c_int32), ("n_levels", C.c_int32), ("subgrid_bytes", C.c_uint64), ("samples_refined", C.c_uint64),
                ("amr_marches", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class VolumeFusedStats(C.Structure):
    """gvt_hip_volume_fused_stats: what gvt_hip_volume_frame_fused reports of one frame."""
    _fields_ = [("fused", C.c_uint32), ("pad", C.c_uint32), ("samples_marched", C.c_uint64), ("samples_gathered", C.c_uint64),
                ("brick_visits", C.c_uint64), ("rays_deposited", C.c_uint64), ("adapter_calls", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class VolumeFusedShadedStats(C.Structure):
    """gvt_hip_volume_fused_shaded_stats: what gvt_hip_volume_frame_fused_shaded reports of one frame."""
    _fields_ = [("fused", C.c_uint32), ("features", C.c_uint32), ("samples_marched", C.c_uint64), ("samples_gathered", C.c_uint64),
                ("brick_visits", C.c_uint64), ("rays_deposited", C.c_uint64), ("adapter_calls", C.c_uint64), ("crossings_rendered", C.c_uint64),
                ("samples_shaded", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class VolumeFusedAmrStats(C.Structure):
    """gvt_hip_volume_fused_amr_stats: gvt_hip_volume_fused_shaded_stats' fields, then the refined samples and the AMR bricks of the frame."""
    _fields_ = VolumeFusedShadedStats._fields_ + [("samples_refined", C.c_uint64), ("amr_bricks", C.c_uint32), ("pad", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class VolumeShadowParams(C.Structure):
    """gvt_hip_volume_shadow_params: flags is 0, or VOLUME_ALLOW_CENTRAL and VOLUME_ALLOW_AMR ORed; bias = the first shadow sample's lattice index, 1 .. 64."""
    _fields_ = [("flags", C.c_uint32), ("bias", C.c_int32)]


class VolumeShadowStats(C.Structure):
    """gvt_hip_volume_shadow_stats: gvt_hip_volume_fused_shaded_stats' fields (the camera rays), then the shadow rays' counters."""
    _fields_ = VolumeFusedShadedStats._fields_ + [("shadowed", C.c_uint32), ("pad", C.c_uint32), ("shadow_rays", C.c_uint64), ("shadow_brick_visits", C.c_uint64),
                                                  ("shadow_crossings", C.c_uint64), ("shadow_samples_marched", C.c_uint64), ("shadow_samples_gathered", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class VolumeLightGridParams(C.Structure):
    """gvt_hip_volume_light_grid_params: flags is 0, or VOLUME_ALLOW_CENTRAL and VOLUME_ALLOW_AMR ORed; bias = the first sample of a vertex's shadow ray, 1 .. 64."""
    _fields_ = [("flags", C.c_uint32), ("bias", C.c_int32)]


class VolumeLightGridStats(C.Structure):
    """gvt_hip_volume_light_grid_stats: what gvt_hip_volume_light_grid_bake reports of one bake."""
    _fields_ = [("rays", C.c_uint64), ("samples_marched", C.c_uint64), ("samples_gathered", C.c_uint64), ("crossings", C.c_uint64), ("bytes", C.c_uint64),
                ("ms", C.c_float), ("pad", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class VolumeLightGridState(C.Structure):
    """gvt_hip_volume_light_grid_state: what gvt_hip_volume_light_grid_info reports of one volume."""
    _fields_ = [("present", C.c_uint32), ("current", C.c_uint32), ("n_planes", C.c_int32), ("bias", C.c_int32), ("bytes", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class VolumeFogShadowStats(C.Structure):
    """gvt_hip_volume_fog_shadow_stats: the shadowed frame's counters, then the lit fog samples that read the light grids."""
    _fields_ = VolumeShadowStats._fields_ + [("fog_samples_shadowed", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class VolumeOccluderParams(C.Structure):
    """gvt_hip_volume_occluder_params: flags is 0, or VOLUME_ALLOW_CENTRAL and VOLUME_ALLOW_AMR ORed."""
    _fields_ = [("flags", C.c_uint32), ("pad", C.c_uint32)]


class VolumeOccluderStats(C.Structure):
    """gvt_hip_volume_occluder_stats: what gvt_hip_volume_occluder_grid_bake reports of one bake."""
    _fields_ = [("rays", C.c_uint64), ("rays_blocked", C.c_uint64), ("any_hit_launches", C.c_uint64), ("bytes", C.c_uint64), ("ms", C.c_float), ("pad", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class VolumeOccluderState(C.Structure):
    """gvt_hip_volume_occluder_state: what gvt_hip_volume_occluder_grid_info reports of one volume."""
    _fields_ = [("present", C.c_uint32), ("current", C.c_uint32), ("n_planes", C.c_int32), ("pad", C.c_int32), ("bytes", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class VolumeMeshShadowStats(C.Structure):
    """gvt_hip_volume_mesh_shadow_stats: the fog-shadowed frame's counters, then whether the mesh-shadowed kernel ran."""
    _fields_ = [("fog", VolumeFogShadowStats), ("mesh_shadowed", C.c_uint32), ("pad", C.c_uint32)]

    def as_dict(self):
        out = self.fog.as_dict()
        out["mesh_shadowed"] = self.mesh_shadowed
        return out


VOLUME_AO_MAX_DIRS = 32  # directions of one AO bake
VOLUME_AO_MESH = 8  # flags of VolumeAoFrameParams only: the base frame is the mesh-shadowed frame


class VolumeAoParams(C.Structure):
    """gvt_hip_volume_ao_params: flags is 0 or VOLUME_ALLOW_CENTRAL; bias 1 .. 64; n_dirs 1 .. VOLUME_AO_MAX_DIRS world-space directions; radius > 0 (inf: no clip)."""
    _fields_ = [("flags", C.c_uint32), ("bias", C.c_int32), ("n_dirs", C.c_int32), ("radius", C.c_float), ("dirs", (C.c_float * 3) * VOLUME_AO_MAX_DIRS)]


class VolumeAoStats(C.Structure):
    """gvt_hip_volume_ao_stats: what gvt_hip_volume_ao_grid_bake reports of one bake (rays = vertices x n_dirs)."""
    _fields_ = [("rays", C.c_uint64), ("samples_marched", C.c_uint64), ("samples_gathered", C.c_uint64), ("crossings", C.c_uint64), ("bytes", C.c_uint64),
                ("ms", C.c_float), ("pad", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class VolumeAoState(C.Structure):
    """gvt_hip_volume_ao_state: what gvt_hip_volume_ao_grid_info reports of one volume."""
    _fields_ = [("present", C.c_uint32), ("current", C.c_uint32), ("n_dirs", C.c_int32), ("bias", C.c_int32), ("radius", C.c_float), ("pad", C.c_uint32),
                ("bytes", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class VolumeAoFrameParams(C.Structure):
    """gvt_hip_volume_ao_frame_params: flags is 0, VOLUME_ALLOW_CENTRAL, VOLUME_AO_MESH or both; bias = the crossings' shadow rays', 1 .. 64."""
    _fields_ = [("flags", C.c_uint32), ("bias", C.c_int32)]


class VolumeAoFrameStats(C.Structure):
    """gvt_hip_volume_ao_frame_stats: the base frame's counters, then whether the AO kernel ran."""
    _fields_ = [("base", VolumeMeshShadowStats), ("ao", C.c_uint32), ("pad", C.c_uint32)]

    def as_dict(self):
        out = self.base.as_dict()
        out["ao"] = self.ao
        return out


FUSED_SURFACES, FUSED_LIT = 1, 2  # gvt_hip_volume_frame_fused_shaded's allow bits: frames with surfaces / with lit fog may be fused
FUSED_AMR = 16  # gvt_hip_volume_frame_fused_amr's further allow bit: frames in which some or all bricks have AMR subgrids may be fused
FUSED_CENTRAL = 8  # ... and such frames whose bricks all shade with VOLUME_GRADIENT_CENTRAL (the kernel's CENTRAL instantiation; its bit in features)
VOLUME_ALLOW_CENTRAL = 2  # flags of VolumeShadowParams, VolumeLightGridParams and VolumeOccluderParams: accept frames whose bricks are all CENTRAL
VOLUME_ALLOW_AMR = 4  # ... the next bit of the same word: accept frames in which some or all bricks have AMR subgrids (the kernels' AMR instantiations)

# volume ray flags (Ray::depth, actor/ORays.h) and gvt_hip_volume_create flags
RAY_OPAQUE, RAY_BOUNDARY, RAY_EXTERNAL_BOUNDARY = 0x2, 0x4, 0x10
RAY_SIDES = 0x20  # the ray's t field holds the surface sides of the sample in t_min
RAY_CLIP = 0x40  # the march takes only the samples with k * dt < the ray's t_max
MARCH_MAY_CLIP = 1  # gvt_hip_volume_march_queue: the queue may hold rays that carry RAY_CLIP
WIRE_MAX_QUEUES = 256  # queues of one gvt_hip_queues_export_wire / _append_wire call
VOLUME_MAX_SURFACES, VOLUME_MAX_LIGHTS = 16, 8
VOLUME_OPAQUE_A = 0.99
VOLUME_DEVICE, VOLUME_NO_SKIP = 1, 2
VOLUME_MAX_SUBGRIDS, VOLUME_MAX_LEVELS = 4096, 4  # AMR volumes (gvt_hip_volume_set_subgrids)
VOLUME_AMR_SHADED = 8  # gvt_hip_volume_set_subgrids flag: this set of subgrids takes surfaces and gradient shading
VOLUME_SHADE_NONE, VOLUME_SHADE_GRADIENT = 0, 1  # gvt_hip_volume_set_shading: the fog's samples lit by the interpolant's gradient
VOLUME_GRADIENT_CELL, VOLUME_GRADIENT_CENTRAL = 0, 1  # gvt_hip_volume_set_gradient: which gradient shades (CENTRAL needs set_ghosts)
VOXEL_F32, VOXEL_U8, VOXEL_I16, VOXEL_U16 = 0, 1, 2, 3  # a volume's voxel type: the samples stay on the device at that width
VOXEL_TYPES = {"float32": VOXEL_F32, "uint8": VOXEL_U8, "int16": VOXEL_I16, "uint16": VOXEL_U16}  # by numpy / torch dtype name

FRAME_BSP, FRAME_NO_COMPOSITE, FRAME_FULL_REDUCE, FRAME_IMAGE = 1, 2, 4, 8


class Stats(C.Structure):
    _fields_ = [("rays_closest", C.c_uint64), ("rays_any", C.c_uint64), ("rays_shaded", C.c_uint64),
                ("rays_forwarded", C.c_uint64), ("trace_calls", C.c_uint64),
                ("ms_closest", C.c_double), ("ms_any", C.c_double), ("ms_shade", C.c_double), ("ms_convert", C.c_double),
                ("ms_shuffle", C.c_double), ("ms_camera", C.c_double), ("ms_build", C.c_double),
                ("launches_closest", C.c_uint64), ("launches_any", C.c_uint64), ("ms_sort", C.c_double), ("ms_long", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib = None


def load():
    """Load the library (no device call).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GvtHipError("%s is missing: build it with `python -m gravit_amd._build` (hipcc, gfx950). "
                              "There is no CPU fallback for the adapter." % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for s in SYMBOLS:
            getattr(lib, s)  # AttributeError if the ABI is incomplete
        lib.gvt_hip_last_error.restype = C.c_char_p
        lib.gvt_hip_volume_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int]
        lib.gvt_hip_volume_set_transfer.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float]
        lib.gvt_hip_volume_set_surfaces.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float]
        lib.gvt_hip_volume_set_lights.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float]
        lib.gvt_hip_volume_set_shading.argtypes = [C.c_void_p, C.c_int]
        lib.gvt_hip_volume_get_shading.argtypes = [C.c_void_p, C.c_void_p]
        lib.gvt_hip_volume_get_shaded.argtypes = [C.c_void_p, C.c_void_p]
        lib.gvt_hip_volume_update_samples.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
        lib.gvt_hip_volume_create_typed.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int]
        lib.gvt_hip_volume_update_samples_typed.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_uint32, C.c_void_p]
        lib.gvt_hip_volume_get_voxel_type.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.gvt_hip_volume_set_subgrids.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        lib.gvt_hip_volume_get_amr_info.argtypes = [C.c_void_p, C.c_void_p]
        lib.gvt_hip_volume_update_amr.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]
        lib.gvt_hip_volume_set_ghosts.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32]
        lib.gvt_hip_volume_set_gradient.argtypes = [C.c_void_p, C.c_int]
        lib.gvt_hip_volume_get_gradient.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.gvt_hip_volume_march_queue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        lib.gvt_hip_volume_camera_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.gvt_hip_queues_export_wire.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.gvt_hip_queues_append_wire.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.gvt_hip_depth_create.argtypes = [C.c_int, C.c_int]
        lib.gvt_hip_depth_clear.argtypes = [C.c_void_p]
        lib.gvt_hip_depth_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        lib.gvt_hip_depth_download.argtypes = [C.c_void_p, C.c_void_p]
        lib.gvt_hip_depth_render.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.gvt_hip_volume_frame_clipped.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.gvt_hip_volume_frame_fused.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.gvt_hip_volume_frame_fused_shaded.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                                          C.c_void_p]
        lib.gvt_hip_volume_frame_fused_amr.argtypes = lib.gvt_hip_volume_frame_fused_shaded.argtypes
        lib.gvt_hip_volume_frame_shadowed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p]
        lib.gvt_hip_volume_frame_fog_shadowed.argtypes = lib.gvt_hip_volume_frame_shadowed.argtypes
        lib.gvt_hip_volume_light_grid_bake.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.gvt_hip_volume_light_grid_download.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.gvt_hip_volume_light_grid_info.argtypes = [C.c_void_p, C.c_void_p]
        lib.gvt_hip_volume_light_grid_release.argtypes = [C.c_void_p]
        lib.gvt_hip_volume_frame_mesh_shadowed.argtypes = lib.gvt_hip_volume_frame_shadowed.argtypes
        lib.gvt_hip_volume_occluder_grid_bake.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.gvt_hip_volume_occluder_grid_download.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.gvt_hip_volume_occluder_grid_info.argtypes = [C.c_void_p, C.c_void_p]
        lib.gvt_hip_volume_occluder_grid_release.argtypes = [C.c_void_p]
        lib.gvt_hip_volume_ao_grid_bake.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.gvt_hip_volume_ao_grid_download.argtypes = [C.c_void_p, C.c_void_p]
        lib.gvt_hip_volume_ao_grid_info.argtypes = [C.c_void_p, C.c_void_p]
        lib.gvt_hip_volume_ao_grid_release.argtypes = [C.c_void_p]
        lib.gvt_hip_volume_frame_ao.argtypes = lib.gvt_hip_volume_frame_shadowed.argtypes
        lib.gvt_hip_fb_composite_over.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        if lib.gvt_hip_abi_version() != ABI_VERSION:  # the out-structs below (MeshInfo, Stats, FrameStats) mirror ONE revision of include/gvt_hip.h
            raise GvtHipError("%s is ABI revision %d, this binding was written against %d: rebuild the library (python -m gravit_amd._build)" % (LIB_PATH, lib.gvt_hip_abi_version(), ABI_VERSION))
        for f in ("gvt_hip_mesh_create", "gvt_hip_queue_create", "gvt_hip_top_create", "gvt_hip_fb_create", "gvt_hip_fb_device_ptr", "gvt_hip_ctx_create",
                  "gvt_hip_comm_create", "gvt_hip_hub_create", "gvt_hip_comm_create_local", "gvt_hip_tracer_create", "gvt_hip_volume_create", "gvt_hip_volume_create_typed",
                  "gvt_hip_depth_create"):
            getattr(lib, f).restype = C.c_void_p
        for f in ("gvt_hip_mesh_destroy", "gvt_hip_queue_destroy", "gvt_hip_top_destroy", "gvt_hip_fb_destroy", "gvt_hip_ctx_destroy", "gvt_hip_hub_abort",
                  "gvt_hip_hub_destroy", "gvt_hip_comm_destroy", "gvt_hip_tracer_destroy", "gvt_hip_volume_destroy", "gvt_hip_depth_destroy"):
            getattr(lib, f).restype = None
            getattr(lib, f).argtypes = [C.c_void_p]
        _lib = lib
    return _lib


def last_error():
    return load().gvt_hip_last_error().decode(errors="replace")


def check(rc, what):
    if rc != 0:
        raise GvtHipError("%s failed (%d): %s" % (what, rc, last_error()))


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a if shape is None else a.reshape(shape)


def counters_peek():
    """Diagnostic: the 32 counter words of the calling thread's context after a stream synchronisation ([3] rays the last closest-hit
    launch parked for k_long_closest, [8] overflow flags)."""
    out = (C.c_uint32 * 32)()
    check(load().gvt_hip_counters_peek(out), "gvt_hip_counters_peek")
    return list(out)


def init(device=0):
    check(load().gvt_hip_init(C.c_int(device)), "gvt_hip_init")


def set_stream(stream_handle):
    check(load().gvt_hip_set_stream(C.c_void_p(stream_handle)), "gvt_hip_set_stream")


def synchronize():
    check(load().gvt_hip_synchronize(), "gvt_hip_synchronize")


def profile(enable):
    check(load().gvt_hip_profile(C.c_int(int(enable))), "gvt_hip_profile")


def stats(reset=False):
    s = Stats()
    check(load().gvt_hip_stats_read(C.byref(s)), "gvt_hip_stats_read")
    if reset:
        check(load().gvt_hip_stats_reset(), "gvt_hip_stats_reset")
    return s.as_dict()


def set_option(name, value):
    check(load().gvt_hip_set_option(name.encode(), C.c_int(int(value))), "gvt_hip_set_option")


def math_probe(kind, x):
    """include/gvt_math.h evaluated on the device (diagnostic): kind 0 gvt_sinf, 1 gvt_cosf, 2 (float)gvt_acos(sqrt(1 - x))."""
    x = f32(x, -1)
    out = np.zeros_like(x)
    check(load().gvt_hip_math_probe(C.c_int(kind), ptr(x), C.c_size_t(len(x)), ptr(out)), "gvt_hip_math_probe")
    return out


def stats_reset():
    check(load().gvt_hip_stats_reset(), "gvt_hip_stats_reset")


__all__ = ["load", "init", "check", "ptr", "f32", "GvtHipError", "MeshInfo", "VolumeInfo", "VolumeAmrInfo", "VolumeFusedStats", "VolumeFusedAmrStats", "VolumeShadowParams", "VolumeShadowStats", "VolumeLightGridParams", "VolumeLightGridStats", "VolumeLightGridState", "VolumeFogShadowStats", "VolumeAoParams", "VolumeAoStats", "VolumeAoState", "VolumeAoFrameParams", "VolumeAoFrameStats", "SubgridPod", "Stats", "SYMBOLS", "RAY_DTYPE", "HIT_DTYPE",
           "LIGHT_DTYPE", "MATERIAL_DTYPE"]
