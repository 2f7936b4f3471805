"""ctypes bindings for the C ABI in include/rt_amd.h and include/rt_host.h.

This is plumbing: struct mirrors, library loading and error translation.  The
render path itself is librt_amd.so (hand-written HIP for gfx950); there is no
Python or CPU fallback — if the library or a device is missing, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
REPO_ROOT = PKG_DIR.parent

RT_OK = 0
RT_MAX_DEPTH = 32


class RtError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"rt_amd error {code}: {message}")
        self.code = code


class Vertex(C.Structure):  # geometric.rs:42-47
    _fields_ = [("position", C.c_float * 3), ("normal", C.c_float * 3), ("uv", C.c_float * 2)]


class Triangle(C.Structure):  # primitives.rs:26-29
    _fields_ = [("object_index", C.c_uint32), ("vertices", Vertex * 3)]


class Sphere(C.Structure):  # primitives.rs:15-24
    _fields_ = [("object_index", C.c_uint32), ("center", C.c_float * 3), ("radius", C.c_float)]


class Material(C.Structure):  # materials.rs:21-31 + enumerated closures
    _fields_ = [
        ("diffuse_fn", C.c_uint32),
        ("normal_fn", C.c_uint32),
        ("normal", C.c_float * 3),
        ("diffuse_color", C.c_float * 3),
        ("shiness", C.c_float),
        ("specular_color", C.c_float * 3),
        ("smoothness", C.c_float),
        ("transparency", C.c_float),
        ("refraction_index", C.c_float),
        ("opaque_decay", C.c_float),
        ("tex_color_a", C.c_float * 3),
        ("tex_color_b", C.c_float * 3),
        ("tex_frequency", C.c_float),
        ("normal_frequency", C.c_float),
    ]


class Light(C.Structure):  # lights.rs:6-30
    _fields_ = [
        ("kind", C.c_uint32),
        ("has_origin", C.c_uint32),
        ("origin", C.c_float * 3),
        ("direction", C.c_float * 3),
        ("angle", C.c_float),
        ("softness", C.c_float),
        ("color", C.c_float * 3),
    ]


class SceneDesc(C.Structure):  # main.rs:130-137
    _fields_ = [
        ("triangles", C.POINTER(Triangle)),
        ("n_triangles", C.c_uint32),
        ("spheres", C.POINTER(Sphere)),
        ("n_spheres", C.c_uint32),
        ("materials", C.POINTER(Material)),
        ("n_materials", C.c_uint32),
        ("lights", C.POINTER(Light)),
        ("n_lights", C.c_uint32),
    ]


class Camera(C.Structure):  # main.rs:43-49
    _fields_ = [
        ("fovy", C.c_float),
        ("center", C.c_float * 3),
        ("toward", C.c_float * 3),
        ("up", C.c_float * 3),
        ("near", C.c_float),
    ]


class Frame(C.Structure):
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("max_depth", C.c_int32),
        ("x0", C.c_uint32),
        ("y0", C.c_uint32),
        ("x1", C.c_uint32),
        ("y1", C.c_uint32),
        ("y_step", C.c_uint32),
    ]

    @classmethod
    def full(cls, width: int, height: int, max_depth: int) -> "Frame":
        return cls(width, height, max_depth, 0, 0, width, height, 1)

    @classmethod
    def rows_of_rank(cls, width: int, height: int, max_depth: int, rank: int, world: int) -> "Frame":
        """Interleaved row bands: rank r renders rows r, r+world, ...."""
        return cls(width, height, max_depth, 0, rank, width, height, world)

    @property
    def cols(self) -> int:
        return self.x1 - self.x0

    @property
    def rows(self) -> int:
        return (self.y1 - self.y0 + self.y_step - 1) // self.y_step


class Ray(C.Structure):  # main.rs:69-81 Ray + Option<Exclusion>, flattened (rt_ray)
    _fields_ = [
        ("origin", C.c_float * 3), ("direction", C.c_float * 3), ("face_direction", C.c_uint32),
        ("has_exclude", C.c_uint32), ("exclude_kind", C.c_uint32), ("exclude_index", C.c_uint32),
        ("exclude_face", C.c_uint32),
    ]


class Hit(C.Structure):  # main.rs:139-147 Hit, flattened (rt_hit)
    _fields_ = [
        ("kind", C.c_uint32), ("index", C.c_uint32), ("object_index", C.c_uint32), ("position", C.c_float * 3),
        ("normal", C.c_float * 3), ("uv", C.c_float * 2), ("face_direction", C.c_uint32), ("distance", C.c_float),
    ]


class Surface(C.Structure):  # materials.rs:21-31 ColorMaterial as approx returns it, and adjust_normal's result (rt_surface)
    _fields_ = [
        ("normal", C.c_float * 3), ("diffuse_color", C.c_float * 3), ("shiness", C.c_float), ("specular_color", C.c_float * 3),
        ("smoothness", C.c_float), ("transparency", C.c_float), ("refraction_index", C.c_float), ("opaque_decay", C.c_float),
        ("shading_normal", C.c_float * 3), ("valid", C.c_uint32),
    ]


RT_HIT_NONE = 0xFFFFFFFF
RAY_WORDS = C.sizeof(Ray) // 4  # 11
HIT_WORDS = C.sizeof(Hit) // 4  # 13
SURFACE_WORDS = C.sizeof(Surface) // 4  # 18


# every symbol include/rt_amd.h declares (checked by tests/test_capi_symbols.py)
DEFAULT_VARIANT = 18  # RT_VARIANT_PWF | RT_VARIANT_STATIC (csrc/rt_kernels.h)

def sources_sha256() -> str:
    """One hash over the sources librt_amd.so is built from (csrc/*.hip, *.h, *.inc, the Makefile), in name order.  The committed
    counter profiles (profiles/traffic*.json, tools/make_traffic.py) carry the hash of the sources they were taken with; bench.py
    reports counter-based figures only while it equals this one — a kernel change without a fresh profile reads as `null`, not as a
    stale number."""
    import hashlib

    h = hashlib.sha256()
    src = PKG_DIR / "csrc"
    for f in sorted(list(src.glob("*.hip")) + list(src.glob("*.h")) + list(src.glob("*.inc")) + [src / "Makefile"]):
        h.update(f.name.encode() + b"\0")
        h.update(f.read_bytes())
    return h.hexdigest()


class DenoiseGuides(C.Structure):
    """rt_denoise_guides: a base pointer and a record stride in 4-byte words per guide plane; a null pointer leaves the plane out"""
    _fields_ = [("normal", C.c_void_p), ("position", C.c_void_p), ("albedo", C.c_void_p), ("valid", C.c_void_p),
                ("normal_stride", C.c_uint32), ("position_stride", C.c_uint32), ("albedo_stride", C.c_uint32), ("valid_stride", C.c_uint32)]


class DenoiseParams(C.Structure):
    """rt_denoise_params"""
    _fields_ = [("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_position", C.c_float),
                ("first_level", C.c_uint32), ("n_levels", C.c_uint32), ("flags", C.c_uint32)]


class TemporalPixel(C.Structure):
    """rt_temporal_pixel: one 32-byte history record"""
    _fields_ = [("color", C.c_float * 3), ("moment1", C.c_float), ("moment2", C.c_float), ("length", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class TemporalGuides(C.Structure):
    """rt_temporal_guides: a base pointer and a record stride in 4-byte words per guide plane; a null pointer leaves the plane out"""
    _fields_ = [("normal", C.c_void_p), ("position", C.c_void_p), ("object", C.c_void_p), ("valid", C.c_void_p),
                ("normal_stride", C.c_uint32), ("position_stride", C.c_uint32), ("object_stride", C.c_uint32), ("valid_stride", C.c_uint32)]


class TemporalParams(C.Structure):
    """rt_temporal_params"""
    _fields_ = [("normal_min", C.c_float), ("position_max", C.c_float), ("alpha_min", C.c_float), ("max_length", C.c_uint32), ("flags", C.c_uint32)]


class TemporalBox(C.Structure):
    """rt_temporal_box: the colour box of one pixel, channels 0..2 colour and 3 luminance"""
    _fields_ = [("lo", C.c_float * 4), ("hi", C.c_float * 4)]


class BoundsParams(C.Structure):
    """rt_bounds_params"""
    _fields_ = [("gamma", C.c_float), ("radius", C.c_uint32), ("flags", C.c_uint32)]


class SvgfVarianceParams(C.Structure):
    """rt_svgf_variance_params"""
    _fields_ = [("sigma_normal", C.c_float), ("sigma_position", C.c_float), ("min_length", C.c_uint32), ("flags", C.c_uint32)]


class SvgfAtrousParams(C.Structure):
    """rt_svgf_atrous_params"""
    _fields_ = [("sigma_luminance", C.c_float), ("sigma_normal", C.c_float), ("sigma_position", C.c_float),
                ("first_level", C.c_uint32), ("n_levels", C.c_uint32), ("flags", C.c_uint32)]


class SampleBudgetParams(C.Structure):
    """rt_sample_budget_params"""
    _fields_ = [("gain", C.c_float), ("epsilon", C.c_float), ("min_count", C.c_uint32), ("max_count", C.c_uint32), ("flags", C.c_uint32)]


class UpsampleParams(C.Structure):
    """rt_upsample_params"""
    _fields_ = [("sigma_normal", C.c_float), ("sigma_position", C.c_float), ("scale", C.c_uint32), ("radius", C.c_uint32), ("flags", C.c_uint32)]


class BloomParams(C.Structure):
    """rt_bloom_params"""
    _fields_ = [("threshold", C.c_float), ("knee", C.c_float), ("intensity", C.c_float), ("n_levels", C.c_uint32)]


class EnvironmentDesc(C.Structure):
    """rt_environment"""
    _fields_ = [("d_texels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("rotation", C.c_float), ("scale", C.c_float),
                ("filter", C.c_uint32)]


class TextureDesc(C.Structure):
    """rt_texture"""
    _fields_ = [("d_texels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("n_levels", C.c_uint32), ("filter", C.c_uint32),
                ("wrap_u", C.c_uint32), ("wrap_v", C.c_uint32), ("scale", C.c_float * 2), ("offset", C.c_float * 2)]


AMD_SYMBOLS = [
    "rt_abi_version", "rt_last_error", "rt_device_count", "rt_set_device", "rt_frame_rows", "rt_frame_pixels",
    "rt_scene_create", "rt_scene_destroy", "rt_render_whitted", "rt_render_whitted_host", "rt_set_option", "rt_set_variant",
    "rt_get_variant", "rt_set_wavefront_budget", "rt_set_distributed_split", "rt_profile_enable", "rt_profile_read", "rt_profile_read_distributed", "rt_math_eval_host", "rt_math_eval_device", "rt_math_eval64_host", "rt_math_eval64_device", "rt_scene_describe_nodes", "rt_scene_describe_filters", "rt_rng_state_words", "rt_rng_create",
    "rt_rng_destroy", "rt_rng_download", "rt_render_distributed", "rt_render_distributed_host", "rt_multi_create", "rt_multi_destroy", "rt_multi_render_whitted_host", "rt_multi_render_distributed_host", "rt_multi_render_whitted", "rt_multi_render_distributed", "rt_post_process_device", "rt_post_keys_device", "rt_post_hist_device", "rt_post_pick_device", "rt_post_scale_device", "rt_post_release", "rt_encode_srgb8_device", "rt_accumulate_device", "rt_accumulator_resolve_device",
    "rt_cast_rays", "rt_cast_rays_host", "rt_camera_rays", "rt_trace_rays", "rt_trace_rays_host",
    "rt_rng_create_seeded", "rt_rng_upload", "rt_trace_rays_distributed", "rt_trace_rays_distributed_host", "rt_focus_rays",
    "rt_shade_hits", "rt_reflect_rays", "rt_refract_rays", "rt_shade_hits_host", "rt_refract_rays_host",
    "rt_scatter_hits", "rt_scatter_factors", "rt_scatter_hits_host", "rt_scatter_factors_host",
    "rt_select_records", "rt_cast_rays_indexed", "rt_level_split", "rt_level_join", "rt_level_close", "rt_level_fold", "rt_level_finish",
    "rt_tree_gate", "rt_tree_split", "rt_tree_spawn", "rt_tree_gather", "rt_tree_fold",
    "rt_light_rays", "rt_light_terms", "rt_light_fold",
    "rt_area_light_rays", "rt_area_light_terms", "rt_area_light_fold",
    "rt_hemisphere_rays", "rt_hemisphere_fold",
    "rt_environment_lookup", "rt_environment_table_bytes", "rt_environment_table", "rt_environment_rays", "rt_environment_fold",
    "rt_material_hits", "rt_material_hits_host", "rt_probe_surfaces", "rt_probe_surfaces_host",
    "rt_lobe_rays", "rt_lobe_pdf", "rt_environment_pdf", "rt_mis_weigh",
    "rt_path_begin", "rt_path_advance", "rt_path_resolve",
    "rt_path_branch", "rt_path_transmit",
    "rt_path_connect", "rt_path_settle", "rt_path_weigh_escape",
    "rt_path_connect_lights", "rt_path_settle_lights",
    "rt_texture_levels", "rt_texture_pyramid_floats", "rt_texture_pyramid", "rt_texture_footprint", "rt_texture_sample", "rt_texture_surfaces",
    "rt_light_terms_surfaces",
    "rt_film_offsets", "rt_camera_rays_offset", "rt_camera_rays_offset_host", "rt_film_splat",
    "rt_sample_budget", "rt_sample_list_temp_bytes", "rt_sample_list", "rt_film_offsets_listed", "rt_camera_rays_listed", "rt_film_splat_listed",
    "rt_denoise_temp_bytes", "rt_denoise_atrous", "rt_denoise_atrous_host",
    "rt_temporal_motion", "rt_temporal_accumulate", "rt_temporal_motion_host", "rt_temporal_accumulate_host",
    "rt_temporal_bounds", "rt_temporal_accumulate_bounded", "rt_temporal_feedback",
    "rt_temporal_bounds_host", "rt_temporal_accumulate_bounded_host", "rt_temporal_feedback_host",
    "rt_svgf_variance", "rt_svgf_temp_bytes", "rt_svgf_atrous", "rt_svgf_variance_host", "rt_svgf_atrous_host",
    "rt_upsample_guided", "rt_upsample_guided_host",
    "rt_bloom_temp_bytes", "rt_bloom", "rt_bloom_host",
    "rt_refract_enter", "rt_refract_step",
    "rt_scene_update_vertices", "rt_scene_update_spheres", "rt_scene_update_lights", "rt_scene_update_materials",
    "rt_scene_keep_positions", "rt_scene_positions_kept", "rt_previous_positions", "rt_previous_positions_host",
    "rt_ray_keys", "rt_sort_temp_bytes", "rt_sort_records", "rt_gather_records", "rt_scatter_records",
    "rt_triangle_keys", "rt_order_triangles_temp_bytes", "rt_order_triangles", "rt_order_triangles_host",
    "rt_diag_scene_nodes", "rt_diag_pwf_plan", "rt_diag_pwf_plan_rays", "rt_diag_pwf_outcome",
]
HOST_SYMBOLS = [
    "rt_world_new", "rt_world_free", "rt_world_push_object", "rt_world_push_triangle", "rt_world_push_sphere",
    "rt_world_push_light", "rt_world_push_flat_triangle", "rt_world_push_square", "rt_world_load_obj",
    "rt_world_build_reference_scene", "rt_world_save_scene", "rt_world_load_scene", "rt_reference_camera", "rt_world_desc", "rt_frame_full", "rt_post_process", "rt_luma_row",
    "rt_encode_srgb8", "rt_accumulate", "rt_accumulator_resolve", "rt_write_png", "rt_host_last_error",
    "rt_film_offsets_host", "rt_film_splat_host", "rt_denoise_atrous_cpu",
    "rt_temporal_motion_cpu", "rt_temporal_accumulate_cpu", "rt_svgf_variance_cpu", "rt_svgf_atrous_cpu",
    "rt_previous_positions_cpu",
    "rt_temporal_bounds_cpu", "rt_temporal_accumulate_bounded_cpu", "rt_temporal_feedback_cpu",
    "rt_sample_budget_cpu", "rt_sample_list_cpu", "rt_film_offsets_listed_cpu", "rt_camera_rays_listed_cpu", "rt_film_splat_listed_cpu",
    "rt_upsample_guided_cpu",
    "rt_bloom_cpu",
    "rt_area_light_samples_cpu",
    "rt_hemisphere_dirs_cpu", "rt_hemisphere_fold_cpu",
]
# librt_host.so's CPU forms of the environment queries, declared in include/rt_environment_host.h (which says why they have a header and
# a list of their own: they are no image-side rt_X / rt_X_cpu pairs)
ENVIRONMENT_HOST_SYMBOLS = ["rt_environment_lookup_cpu", "rt_environment_table_cpu", "rt_environment_samples_cpu", "rt_environment_fold_cpu"]
# ... and of the lobe queries, declared in include/rt_lobe_host.h for the same reason
LOBE_HOST_SYMBOLS = ["rt_lobe_samples_cpu", "rt_lobe_pdf_cpu", "rt_environment_pdf_cpu", "rt_mis_weigh_cpu"]
# ... and of the path queries, declared in include/rt_path_host.h
PATH_HOST_SYMBOLS = ["rt_path_begin_cpu", "rt_path_advance_cpu", "rt_path_resolve_cpu"]
# ... and of the transmission queries, declared in include/rt_transmit_host.h
TRANSMIT_HOST_SYMBOLS = ["rt_path_branch_cpu", "rt_path_transmit_cpu"]
# ... and of the connection queries, declared in include/rt_connect_host.h
CONNECT_HOST_SYMBOLS = ["rt_path_connect_cpu", "rt_path_settle_cpu", "rt_path_weigh_escape_cpu"]
# ... and of the light-connection queries, declared in include/rt_light_connect_host.h
LIGHT_CONNECT_HOST_SYMBOLS = ["rt_path_connect_lights_cpu", "rt_path_settle_lights_cpu"]
# ... and of the texture queries, declared in include/rt_texture_host.h
TEXTURE_HOST_SYMBOLS = ["rt_texture_pyramid_cpu", "rt_texture_footprint_cpu", "rt_texture_sample_cpu", "rt_texture_surfaces_cpu"]

_amd = None
_host = None


def _load(name: str) -> C.CDLL:
    path = PKG_DIR / name
    if not path.exists():
        raise RtError(-2, f"{path} is not built; run __graft_entry__.build() (make -C {PKG_DIR / 'csrc'})")
    return C.CDLL(str(path), mode=getattr(os, "RTLD_NOW", 2))


def host_lib() -> C.CDLL:
    global _host
    if _host is None:
        lib = _load("librt_host.so")
        lib.rt_world_new.restype = C.c_void_p
        lib.rt_world_free.argtypes = [C.c_void_p]
        lib.rt_world_free.restype = None
        lib.rt_world_push_object.argtypes = [C.c_void_p, C.POINTER(Material)]
        lib.rt_world_push_triangle.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(Vertex)]
        lib.rt_world_push_sphere.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_float), C.c_float]
        lib.rt_world_push_light.argtypes = [C.c_void_p, C.POINTER(Light)]
        lib.rt_world_push_flat_triangle.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        lib.rt_world_push_square.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        lib.rt_world_load_obj.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_float, C.POINTER(C.c_float)]
        lib.rt_world_build_reference_scene.argtypes = [C.c_void_p, C.c_char_p]
        lib.rt_world_save_scene.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_char_p]
        lib.rt_world_load_scene.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(Camera), C.POINTER(C.c_int)]
        lib.rt_reference_camera.argtypes = [C.POINTER(Camera)]
        lib.rt_reference_camera.restype = None
        lib.rt_world_desc.argtypes = [C.c_void_p, C.POINTER(SceneDesc)]
        lib.rt_world_desc.restype = None
        lib.rt_frame_full.argtypes = [C.c_uint32, C.c_uint32, C.c_int32, C.POINTER(Frame)]
        lib.rt_frame_full.restype = None
        lib.rt_post_process.argtypes = [C.c_void_p, C.c_size_t]
        lib.rt_post_process.restype = C.c_float
        lib.rt_encode_srgb8.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        lib.rt_encode_srgb8.restype = None
        lib.rt_accumulate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.rt_accumulate.restype = None
        lib.rt_accumulator_resolve.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.rt_accumulator_resolve.restype = None
        lib.rt_film_offsets_host.argtypes = [C.POINTER(Frame), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.rt_film_splat_host.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p,
                                           C.c_void_p]
        lib.rt_denoise_atrous_cpu.argtypes = [C.c_void_p, C.POINTER(DenoiseGuides), C.POINTER(DenoiseParams), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.rt_temporal_motion_cpu.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(Camera), C.POINTER(Frame), C.c_void_p]
        lib.rt_temporal_accumulate_cpu.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(TemporalGuides), C.POINTER(TemporalGuides), C.POINTER(TemporalParams),
                                                   C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_temporal_bounds_cpu.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(BoundsParams), C.c_uint32, C.c_uint32,
                                               C.c_void_p]
        lib.rt_temporal_accumulate_bounded_cpu.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(TemporalGuides), C.POINTER(TemporalGuides), C.POINTER(TemporalParams),
                                                           C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.rt_temporal_feedback_cpu.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.rt_svgf_variance_cpu.argtypes = [C.c_void_p, C.POINTER(DenoiseGuides), C.POINTER(SvgfVarianceParams), C.c_uint32, C.c_uint32, C.c_void_p]
        lib.rt_svgf_atrous_cpu.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(DenoiseGuides), C.POINTER(SvgfAtrousParams), C.c_uint32, C.c_uint32,
                                           C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_previous_positions_cpu.argtypes = [C.POINTER(SceneDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32]
        lib.rt_write_png.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32]
        lib.rt_sample_budget_cpu.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                             C.POINTER(SampleBudgetParams), C.c_size_t, C.c_void_p]
        lib.rt_sample_list_cpu.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_film_offsets_listed_cpu.argtypes = [C.POINTER(Frame), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.rt_camera_rays_listed_cpu.argtypes = [C.POINTER(Camera), C.POINTER(Frame), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.rt_film_splat_listed_cpu.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32,
                                                 C.c_float, C.c_void_p, C.c_void_p]
        lib.rt_upsample_guided_cpu.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(DenoiseGuides), C.c_void_p, C.c_uint32, C.POINTER(DenoiseGuides), C.c_void_p,
                                               C.c_uint32, C.POINTER(UpsampleParams), C.c_uint32, C.c_uint32, C.c_void_p]
        lib.rt_bloom_cpu.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(BloomParams), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.rt_area_light_samples_cpu.argtypes = [C.POINTER(Light), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32,
                                                  C.c_uint32, C.c_void_p]
        lib.rt_hemisphere_dirs_cpu.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.rt_hemisphere_fold_cpu.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_float,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_environment_lookup_cpu.argtypes = [C.POINTER(EnvironmentDesc), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.rt_environment_table_cpu.argtypes = [C.POINTER(EnvironmentDesc), C.c_void_p]
        lib.rt_environment_samples_cpu.argtypes = [C.POINTER(EnvironmentDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_environment_fold_cpu.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p]
        lib.rt_lobe_samples_cpu.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_lobe_pdf_cpu.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.rt_environment_pdf_cpu.argtypes = [C.POINTER(EnvironmentDesc), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.rt_mis_weigh_cpu.argtypes = [C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
        lib.rt_path_begin_cpu.argtypes = [C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_path_advance_cpu.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                            C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_path_resolve_cpu.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.rt_path_branch_cpu.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_path_transmit_cpu.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                             C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_path_connect_cpu.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EnvironmentDesc), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                            C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_path_settle_cpu.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_path_weigh_escape_cpu.argtypes = [C.POINTER(EnvironmentDesc), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_uint32, C.c_void_p]
        lib.rt_path_connect_lights_cpu.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                   C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p]
        lib.rt_path_settle_lights_cpu.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p]
        lib.rt_texture_pyramid_cpu.argtypes = [C.POINTER(TextureDesc)]
        lib.rt_texture_footprint_cpu.argtypes = [C.POINTER(SceneDesc), C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p]
        lib.rt_texture_sample_cpu.argtypes = [C.POINTER(TextureDesc), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        lib.rt_texture_surfaces_cpu.argtypes = [C.POINTER(TextureDesc), C.POINTER(TextureDesc), C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32,
                                                C.c_uint32, C.c_void_p]
        lib.rt_host_last_error.restype = C.c_char_p
        _host = lib
    return _host


def amd_lib() -> C.CDLL:
    """The HIP library.  Loading needs libamdhip64 but no GPU; calls need a GPU."""
    global _amd
    if _amd is None:
        # One HIP runtime per process: PyTorch ships its own libamdhip64.so (soname libamdhip64.so.7) and a
        # process that initialises two copies of the runtime loses the device in the second one ("no
        # ROCm-capable device is detected").  Import torch FIRST so that librt_amd.so's DT_NEEDED
        # libamdhip64.so.7 binds to the copy torch already loaded; without torch it binds to /opt/rocm's.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = _load("librt_amd.so")
        lib.rt_last_error.restype = C.c_char_p
        lib.rt_frame_rows.argtypes = [C.POINTER(Frame)]
        lib.rt_frame_rows.restype = C.c_uint32
        lib.rt_frame_pixels.argtypes = [C.POINTER(Frame)]
        lib.rt_frame_pixels.restype = C.c_uint64
        lib.rt_scene_create.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_void_p)]
        lib.rt_scene_destroy.argtypes = [C.c_void_p]
        lib.rt_render_whitted.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Frame), C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_render_whitted_host.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Frame), C.c_void_p, C.POINTER(C.c_ulonglong)]
        lib.rt_set_variant.argtypes = [C.c_int]
        lib.rt_set_option.argtypes = [C.c_char_p, C.c_char_p]
        lib.rt_multi_create.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]
        lib.rt_multi_destroy.argtypes = [C.c_void_p]
        lib.rt_multi_render_whitted_host.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Frame), C.c_void_p, C.POINTER(C.c_ulonglong)]
        lib.rt_multi_render_distributed_host.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Frame), C.c_float, C.c_float, C.c_uint32,
                                                         C.c_void_p, C.POINTER(C.c_ulonglong)]
        lib.rt_multi_render_whitted.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Frame), C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_multi_render_distributed.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Frame), C.c_float, C.c_float, C.c_uint32,
                                                    C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_post_process_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.rt_post_keys_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_post_hist_device.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
        lib.rt_post_pick_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        lib.rt_post_scale_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_encode_srgb8_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.rt_accumulate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_accumulator_resolve_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.rt_rng_create.argtypes = [C.POINTER(Frame), C.POINTER(C.c_void_p)]
        lib.rt_rng_destroy.argtypes = [C.c_void_p]
        lib.rt_rng_download.argtypes = [C.c_void_p, C.c_void_p]
        lib.rt_render_distributed.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Frame), C.c_float, C.c_float, C.c_void_p,
                                              C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_render_distributed_host.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Frame), C.c_float, C.c_float, C.c_void_p,
                                                   C.c_uint32, C.c_void_p, C.POINTER(C.c_ulonglong)]
        lib.rt_set_wavefront_budget.argtypes = [C.c_uint]
        lib.rt_set_distributed_split.argtypes = [C.c_int]
        lib.rt_profile_enable.argtypes = [C.c_int]
        lib.rt_profile_read.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_uint)]
        lib.rt_math_eval_host.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.rt_math_eval_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.rt_math_eval64_host.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.rt_math_eval64_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.rt_cast_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.rt_cast_rays_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.rt_camera_rays.argtypes = [C.POINTER(Camera), C.POINTER(Frame), C.c_void_p, C.c_void_p]
        lib.rt_trace_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_trace_rays_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_float, C.c_void_p, C.POINTER(C.c_ulonglong)]
        lib.rt_rng_create_seeded.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        lib.rt_rng_upload.argtypes = [C.c_void_p, C.c_void_p]
        lib.rt_trace_rays_distributed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_trace_rays_distributed_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p,
                                                       C.POINTER(C.c_ulonglong)]
        lib.rt_focus_rays.argtypes = [C.POINTER(Camera), C.POINTER(Frame), C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_shade_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_reflect_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.rt_refract_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]
        lib.rt_shade_hits_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_ulonglong)]
        lib.rt_refract_rays_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.POINTER(C.c_ulonglong)]
        lib.rt_scatter_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]
        lib.rt_scatter_factors.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.rt_scatter_hits_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_scatter_factors_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.rt_select_records.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_cast_rays_indexed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_level_split.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_level_join.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]
        lib.rt_level_close.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.rt_level_fold.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.rt_level_finish.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_tree_gate.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_tree_split.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]
        lib.rt_tree_spawn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_tree_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_tree_fold.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.rt_light_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]
        lib.rt_light_terms.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_light_fold.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_area_light_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                           C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_area_light_terms.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_area_light_fold.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]
        lib.rt_hemisphere_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_hemisphere_fold.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_environment_lookup.argtypes = [C.POINTER(EnvironmentDesc), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                              C.c_void_p]
        lib.rt_environment_table_bytes.argtypes = [C.c_uint32, C.c_uint32]
        lib.rt_environment_table_bytes.restype = C.c_size_t
        lib.rt_environment_table.argtypes = [C.POINTER(EnvironmentDesc), C.c_void_p, C.c_void_p]
        lib.rt_environment_rays.argtypes = [C.c_void_p, C.POINTER(EnvironmentDesc), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint32,
                                            C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_environment_fold.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_lobe_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_lobe_pdf.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.rt_environment_pdf.argtypes = [C.POINTER(EnvironmentDesc), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_mis_weigh.argtypes = [C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_path_begin.argtypes = [C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_path_advance.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                        C.c_uint32, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_path_resolve.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_path_branch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_path_transmit.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                         C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_path_connect.argtypes = [C.c_void_p, C.POINTER(EnvironmentDesc), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_path_settle.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_path_weigh_escape.argtypes = [C.POINTER(EnvironmentDesc), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_uint32, C.c_void_p, C.c_void_p]
        lib.rt_path_connect_lights.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                               C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_path_settle_lights.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]
        lib.rt_texture_levels.argtypes = [C.c_uint32, C.c_uint32]
        lib.rt_texture_levels.restype = C.c_uint32
        lib.rt_texture_pyramid_floats.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        lib.rt_texture_pyramid_floats.restype = C.c_size_t
        lib.rt_texture_pyramid.argtypes = [C.POINTER(TextureDesc), C.c_void_p]
        lib.rt_texture_footprint.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_texture_sample.argtypes = [C.POINTER(TextureDesc), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.rt_texture_surfaces.argtypes = [C.POINTER(TextureDesc), C.POINTER(TextureDesc), C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32,
                                            C.c_void_p, C.c_void_p]
        lib.rt_light_terms_surfaces.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_material_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.rt_material_hits_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.rt_probe_surfaces.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_probe_surfaces_host.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.rt_film_offsets.argtypes = [C.POINTER(Frame), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.rt_camera_rays_offset.argtypes = [C.POINTER(Camera), C.POINTER(Frame), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.rt_camera_rays_offset_host.argtypes = [C.POINTER(Camera), C.POINTER(Frame), C.c_void_p, C.c_uint32, C.c_void_p]
        lib.rt_film_splat.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p,
                                      C.c_void_p]
        lib.rt_denoise_temp_bytes.argtypes = [C.c_uint32, C.c_uint32]
        lib.rt_denoise_temp_bytes.restype = C.c_size_t
        lib.rt_denoise_atrous.argtypes = [C.c_void_p, C.POINTER(DenoiseGuides), C.POINTER(DenoiseParams), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.c_void_p]
        lib.rt_denoise_atrous_host.argtypes = [C.c_void_p, C.POINTER(DenoiseGuides), C.POINTER(DenoiseParams), C.c_uint32, C.c_uint32, C.c_void_p]
        lib.rt_temporal_motion.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(Camera), C.POINTER(Frame), C.c_void_p, C.c_void_p]
        lib.rt_temporal_motion_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(Camera), C.POINTER(Frame), C.c_void_p]
        lib.rt_temporal_accumulate.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(TemporalGuides), C.POINTER(TemporalGuides), C.POINTER(TemporalParams),
                                               C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_temporal_accumulate_host.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(TemporalGuides), C.POINTER(TemporalGuides), C.POINTER(TemporalParams),
                                                    C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_temporal_bounds.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(BoundsParams), C.c_uint32, C.c_uint32,
                                           C.c_void_p, C.c_void_p]
        lib.rt_temporal_bounds_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(BoundsParams), C.c_uint32,
                                                C.c_uint32, C.c_void_p]
        lib.rt_temporal_accumulate_bounded.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(TemporalGuides), C.POINTER(TemporalGuides), C.POINTER(TemporalParams),
                                                       C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.rt_temporal_accumulate_bounded_host.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(TemporalGuides), C.POINTER(TemporalGuides),
                                                            C.POINTER(TemporalParams), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                            C.c_uint32, C.c_void_p]
        lib.rt_temporal_feedback.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.rt_temporal_feedback_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.rt_svgf_variance.argtypes = [C.c_void_p, C.POINTER(DenoiseGuides), C.POINTER(SvgfVarianceParams), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.rt_svgf_variance_host.argtypes = [C.c_void_p, C.POINTER(DenoiseGuides), C.POINTER(SvgfVarianceParams), C.c_uint32, C.c_uint32, C.c_void_p]
        lib.rt_svgf_temp_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        lib.rt_svgf_temp_bytes.restype = C.c_size_t
        lib.rt_svgf_atrous.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(DenoiseGuides), C.POINTER(SvgfAtrousParams), C.c_uint32, C.c_uint32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_svgf_atrous_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(DenoiseGuides), C.POINTER(SvgfAtrousParams), C.c_uint32, C.c_uint32,
                                            C.c_void_p, C.c_void_p]
        lib.rt_upsample_guided.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(DenoiseGuides), C.c_void_p, C.c_uint32, C.POINTER(DenoiseGuides), C.c_void_p,
                                           C.c_uint32, C.POINTER(UpsampleParams), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.rt_upsample_guided_host.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(DenoiseGuides), C.c_void_p, C.c_uint32, C.POINTER(DenoiseGuides), C.c_void_p,
                                                C.c_uint32, C.POINTER(UpsampleParams), C.c_uint32, C.c_uint32, C.c_void_p]
        lib.rt_bloom_temp_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        lib.rt_bloom_temp_bytes.restype = C.c_size_t
        lib.rt_bloom.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(BloomParams), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_bloom_host.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(BloomParams), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.rt_refract_enter.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
        lib.rt_refract_step.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_scene_update_vertices.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.rt_scene_update_spheres.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.rt_scene_update_lights.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(Light), C.c_void_p]
        lib.rt_scene_update_materials.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(Material), C.c_void_p]
        lib.rt_scene_keep_positions.argtypes = [C.c_void_p, C.c_void_p]
        lib.rt_scene_positions_kept.argtypes = [C.c_void_p]
        lib.rt_previous_positions.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.rt_previous_positions_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32]
        lib.rt_ray_keys.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, C.c_void_p, C.c_void_p]
        lib.rt_sample_budget.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                         C.POINTER(SampleBudgetParams), C.c_size_t, C.c_void_p, C.c_void_p]
        lib.rt_sample_list_temp_bytes.argtypes = [C.c_size_t]
        lib.rt_sample_list_temp_bytes.restype = C.c_size_t
        lib.rt_sample_list.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                       C.c_void_p]
        lib.rt_film_offsets_listed.argtypes = [C.POINTER(Frame), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.rt_camera_rays_listed.argtypes = [C.POINTER(Camera), C.POINTER(Frame), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.rt_film_splat_listed.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32,
                                             C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_sort_temp_bytes.argtypes = [C.c_size_t]
        lib.rt_sort_temp_bytes.restype = C.c_size_t
        lib.rt_sort_records.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_void_p]
        lib.rt_gather_records.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.rt_scatter_records.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.rt_triangle_keys.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rt_order_triangles_temp_bytes.argtypes = [C.c_size_t]
        lib.rt_order_triangles_temp_bytes.restype = C.c_size_t
        lib.rt_order_triangles.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_size_t, C.c_void_p]
        lib.rt_order_triangles_host.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, C.c_void_p, C.c_void_p]
        lib.rt_scene_describe_nodes.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]
        lib.rt_scene_describe_filters.argtypes = [C.POINTER(SceneDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        lib.rt_diag_scene_nodes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        lib.rt_diag_pwf_plan.argtypes = [C.c_void_p, C.POINTER(Frame), C.c_void_p, C.c_void_p]
        lib.rt_diag_pwf_plan_rays.argtypes = [C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p]
        lib.rt_diag_pwf_outcome.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _amd = lib
    return _amd


def check(rc: int) -> int:
    if rc < 0:
        raise RtError(rc, amd_lib().rt_last_error().decode("utf-8", "replace"))
    return rc


def check_host(rc: int) -> int:
    if rc < 0:
        raise RtError(rc, host_lib().rt_host_last_error().decode("utf-8", "replace"))
    return rc
