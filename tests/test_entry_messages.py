"""Every argument check an entry point of include/rt_amd.h can fail without a GPU: its status and the FULL text of rt_last_error().
The *_abi.py tests look for substrings; this table pins the messages byte for byte, so that the shared checkers of
csrc/rt_api_internal.h cannot drift from what each entry point has always said.  The scene is a fake pointer and the generators are
an empty rt_rng (as in tests/test_scatter_query_abi.py): every case is refused on its arguments, or has nothing to do, before
anything is read through either."""
import ctypes as C

import pytest

from homework_18_graphics_raytracer_amd import _capi

OK, INVALID, UNSUPPORTED = 0, -1, -5
BIG = 1 << 32

BUF = (C.c_uint64 * 512)()  # stands for every record array: never read, every case ends in a check
P = C.cast(BUF, C.c_void_p)
SCENE = C.c_void_p(16)  # never dereferenced
RNG = "the empty rt_rng"  # replaced by the fixture's handle
CAMERA = _capi.Camera()
FRAME = _capi.Frame.full(8, 6, 3)
BAD_FRAME = _capi.Frame(8, 6, 3, 4, 0, 4, 6, 1)  # x0 == x1
HUGE_FRAME = _capi.Frame.full(65536, 65536, 3)  # 2^32 pixels
DEEP_FRAME = _capi.Frame.full(8, 6, _capi.RT_MAX_DEPTH + 1)
BOX = (C.c_float * 3)(0.0, 0.0, 0.0)
OUT = C.pointer(C.c_void_p())  # where a create call puts its handle

# the arguments of each entry point, in order, with a value that passes every check
SIGNATURES = {
    "rt_set_option": [("name", b"RT_AMD_SCATTER_PREPARE"), ("value", b"0")],
    "rt_set_variant": [("variant", 18)],
    "rt_set_wavefront_budget": [("budget", 6)],
    "rt_profile_read": [("ms", C.pointer(C.c_double())), ("launches", C.pointer(C.c_uint()))],
    "rt_profile_read_distributed": [("ms", P), ("launches", P)],
    "rt_scene_create": [("desc", C.pointer(_capi.SceneDesc())), ("out", OUT)],
    "rt_scene_describe_filters": [("desc", C.pointer(_capi.SceneDesc())), ("tri4", P), ("sphere1", P), ("light2", P), ("origin2", C.pointer(C.c_float()))],
    "rt_diag_scene_nodes": [("scene", SCENE), ("which", 0), ("words", P), ("cap", 4), ("n_words", C.pointer(C.c_size_t()))],
    "rt_diag_pwf_plan": [("scene", SCENE), ("frame", FRAME), ("stream", None), ("words", P)],
    "rt_diag_pwf_plan_rays": [("scene", SCENE), ("n", 2), ("depth", 3), ("stream", None), ("words", P)],
    "rt_diag_pwf_outcome": [("scene", SCENE), ("stream", None), ("words", P)],
    "rt_render_whitted": [("scene", SCENE), ("camera", CAMERA), ("frame", FRAME), ("rgb", P), ("count", P), ("stream", None)],
    "rt_render_whitted_host": [("scene", SCENE), ("camera", CAMERA), ("frame", FRAME), ("rgb", P), ("count", None)],
    "rt_trace_rays": [("scene", SCENE), ("rays", P), ("n", 2), ("depth", 3), ("contribution", 1.0), ("rgb", P), ("count", P), ("stream", None)],
    "rt_trace_rays_host": [("scene", SCENE), ("rays", P), ("n", 2), ("depth", 3), ("contribution", 1.0), ("rgb", P), ("count", None)],
    "rt_cast_rays": [("scene", SCENE), ("rays", P), ("n", 2), ("hits", P), ("stream", None)],
    "rt_cast_rays_host": [("scene", SCENE), ("rays", P), ("n", 2), ("hits", P)],
    "rt_camera_rays": [("camera", CAMERA), ("frame", FRAME), ("rays", P), ("stream", None)],
    "rt_shade_hits": [("scene", SCENE), ("hits", P), ("incoming", P), ("n", 2), ("rgb", P), ("count", P), ("stream", None)],
    "rt_shade_hits_host": [("scene", SCENE), ("hits", P), ("incoming", P), ("n", 2), ("rgb", P), ("count", None)],
    "rt_reflect_rays": [("hits", P), ("incoming", P), ("n", 2), ("out", P), ("stream", None)],
    "rt_refract_rays": [("scene", SCENE), ("hits", P), ("incoming", P), ("n", 2), ("max_distance", 1.0), ("kind", P), ("travel", P), ("escape", P),
                        ("count", P), ("stream", None)],
    "rt_refract_rays_host": [("scene", SCENE), ("hits", P), ("incoming", P), ("n", 2), ("max_distance", 1.0), ("kind", P), ("travel", P),
                             ("escape", P), ("count", None)],
    "rt_scatter_hits": [("scene", SCENE), ("hits", P), ("incoming", P), ("n", 2), ("rng", RNG), ("index", P), ("type", P), ("scattered", P),
                        ("cosine", P), ("stream", None)],
    "rt_scatter_hits_host": [("scene", SCENE), ("hits", P), ("incoming", P), ("n", 2), ("rng", RNG), ("index", P), ("type", P), ("scattered", P),
                             ("cosine", P)],
    "rt_scatter_factors": [("scene", SCENE), ("hits", P), ("incoming", P), ("type", P), ("next", P), ("travel", P), ("n", 2), ("rgb", P),
                           ("stream", None)],
    "rt_scatter_factors_host": [("scene", SCENE), ("hits", P), ("incoming", P), ("type", P), ("next", P), ("travel", P), ("n", 2), ("rgb", P)],
    "rt_select_records": [("flags", P), ("n", 2), ("index", P), ("count", P), ("stream", None)],
    "rt_cast_rays_indexed": [("scene", SCENE), ("rays", P), ("n", 2), ("index", P), ("count", P), ("max_count", 2), ("hits", P), ("ray_count", P),
                             ("stream", None)],
    "rt_level_split": [("hits", P), ("type", P), ("cosine", P), ("n", 2), ("reflect", P), ("refract", P), ("stream", None)],
    "rt_level_join": [("type", P), ("cosine", P), ("reflected", P), ("refr_kind", P), ("escape", P), ("n", 2), ("next", P), ("next_hits", P),
                      ("flags", P), ("stream", None)],
    "rt_level_close": [("hits", P), ("type", P), ("cosine", P), ("next_hits", P), ("n", 2), ("missed", P), ("stream", None)],
    "rt_level_fold": [("type", P), ("cosine", P), ("next_hits", P), ("factor", P), ("shade_next", P), ("shade_missed", P), ("n", 2), ("value", P),
                      ("stream", None)],
    "rt_level_finish": [("value", P), ("n", 2), ("accum", P), ("valid", P), ("stream", None)],
    "rt_tree_gate": [("contribution", P), ("n", 2), ("count", P), ("flags", P), ("hits", P), ("stream", None)],
    "rt_tree_split": [("scene", SCENE), ("hits", P), ("contribution", P), ("n", 2), ("count", P), ("depth_left", 3), ("shade", P), ("reflect", P),
                      ("refract", P), ("weights", P), ("stream", None)],
    "rt_tree_spawn": [("reflect", P), ("refr_kind", P), ("n", 2), ("flags", P), ("child_values", P), ("stream", None)],
    "rt_tree_gather": [("index", P), ("count", P), ("max_count", 4), ("reflected", P), ("escape", P), ("contribution", P), ("weights", P), ("n", 2),
                       ("child_rays", P), ("child_contribution", P), ("child_parent", P), ("child_count", P), ("overflow", P), ("stream", None)],
    "rt_tree_fold": [("hits", P), ("count", P), ("n", 2), ("depth_left", 3), ("shade", P), ("weights", P), ("refr_kind", P), ("travel", P),
                     ("child_values", P), ("parent", P), ("out", P), ("n_out", 2), ("stream", None)],
    "rt_light_rays": [("scene", SCENE), ("hits", P), ("incoming", P), ("n", 2), ("first", 0), ("lights", 1), ("shadow_rays", P), ("asks", P),
                      ("distance", P), ("stream", None)],
    "rt_light_terms": [("scene", SCENE), ("hits", P), ("incoming", P), ("n", 2), ("first", 0), ("lights", 1), ("asks", P), ("shadow_hits", P),
                       ("lit", P), ("diffuse", P), ("specular", P), ("stream", None)],
    "rt_light_fold": [("scene", SCENE), ("hits", P), ("n", 2), ("lights", 1), ("lit", P), ("diffuse", P), ("specular", P), ("rgb", P),
                      ("stream", None)],
    "rt_refract_enter": [("scene", SCENE), ("hits", P), ("incoming", P), ("n", 2), ("rays", P), ("kind", P), ("travel", P), ("casts", P),
                         ("flags", P), ("stream", None)],
    "rt_refract_step": [("scene", SCENE), ("hits", P), ("n", 2), ("max_distance", 1.0), ("inside", P), ("rays", P), ("kind", P), ("travel", P),
                        ("casts", P), ("flags", P), ("escape", P), ("stream", None)],
    "rt_scene_update_vertices": [("scene", SCENE), ("first", 0), ("count", 1), ("data", P), ("stream", None)],
    "rt_scene_update_spheres": [("scene", SCENE), ("first", 0), ("count", 1), ("data", P), ("stream", None)],
    "rt_scene_update_lights": [("scene", SCENE), ("first", 0), ("count", 1), ("data", None), ("stream", None)],
    "rt_scene_update_materials": [("scene", SCENE), ("first", 0), ("count", 1), ("data", None), ("stream", None)],
    "rt_ray_keys": [("rays", P), ("n", 2), ("lo", BOX), ("hi", BOX), ("flags", 0), ("keys", P), ("stream", None)],
    "rt_sort_records": [("keys", P), ("n", 2), ("first_bit", 0), ("key_bits", 8), ("index_in", P), ("count_in", P), ("index_out", P), ("temp", P),
                        ("temp_bytes", 1 << 20), ("stream", None)],
    "rt_gather_records": [("src", P), ("record_bytes", 8), ("n", 2), ("index", P), ("count", P), ("max_count", 2), ("dst", P), ("stream", None)],
    "rt_scatter_records": [("src", P), ("record_bytes", 8), ("n", 2), ("index", P), ("count", P), ("max_count", 2), ("dst", P), ("stream", None)],
    "rt_triangle_keys": [("triangles", P), ("n", 2), ("lo", BOX), ("hi", BOX), ("keys", P), ("objects", P), ("stream", None)],
    "rt_order_triangles": [("triangles", P), ("n", 2), ("lo", BOX), ("hi", BOX), ("objects", 1), ("perm", P), ("ordered", P), ("temp", P),
                           ("temp_bytes", 1 << 20), ("stream", None)],
    "rt_order_triangles_host": [("triangles", P), ("n", 2), ("lo", BOX), ("hi", BOX), ("objects", 1), ("perm", P), ("ordered", P)],
    "rt_rng_create": [("frame", FRAME), ("out", OUT)],
    "rt_rng_create_seeded": [("seeds", P), ("n", 2), ("out", OUT)],
    "rt_rng_download": [("rng", RNG), ("states", P)],
    "rt_rng_upload": [("rng", RNG), ("states", P)],
    "rt_render_distributed": [("scene", SCENE), ("camera", CAMERA), ("frame", FRAME), ("focus", 1.0), ("blur", 0.1), ("rng", RNG), ("epochs", 1),
                              ("accum", P), ("samples", P), ("valid", P), ("count", P), ("stream", None)],
    "rt_render_distributed_host": [("scene", SCENE), ("camera", CAMERA), ("frame", FRAME), ("focus", 1.0), ("blur", 0.1), ("rng", RNG),
                                   ("epochs", 1), ("accum", P), ("count", None)],
    "rt_trace_rays_distributed": [("scene", SCENE), ("rays", P), ("n", 0), ("depth", 3), ("rng", RNG), ("epochs", 1), ("accum", P), ("samples", P),
                                  ("valid", P), ("count", P), ("stream", None)],
    "rt_trace_rays_distributed_host": [("scene", SCENE), ("rays", P), ("n", 0), ("depth", 3), ("rng", RNG), ("epochs", 1), ("accum", P),
                                       ("count", None)],
    "rt_focus_rays": [("camera", CAMERA), ("frame", FRAME), ("focus", 1.0), ("blur", 0.1), ("rng", RNG), ("rays", P), ("stream", None)],
    "rt_post_process_device": [("rgb", P), ("n", 2), ("divisor", P), ("stream", None)],
    "rt_post_keys_device": [("rgb", P), ("n", 2), ("keys", P), ("state", P), ("stream", None)],
    "rt_post_hist_device": [("keys", P), ("n", 2), ("pass_", 0), ("state", P), ("stream", None)],
    "rt_post_pick_device": [("pass_", 0), ("state", P), ("stream", None)],
    "rt_post_scale_device": [("rgb", P), ("n", 2), ("state", P), ("divisor", P), ("stream", None)],
    "rt_accumulate_device": [("samples", P), ("valid", P), ("epochs", 1), ("n", 2), ("sum", P), ("weight", P), ("stream", None)],
    "rt_accumulator_resolve_device": [("sum", P), ("weight", P), ("n", 2), ("rgb", P), ("stream", None)],
    "rt_encode_srgb8_device": [("rgb", P), ("n", 6), ("out", P), ("stream", None)],
    "rt_math_eval_host": [("op", 0), ("x", P), ("y", P), ("out", P), ("n", 2)],
    "rt_math_eval_device": [("op", 0), ("x", P), ("y", P), ("out", P), ("n", 2)],
    "rt_math_eval64_host": [("op", 0), ("a", P), ("b", P), ("out", P), ("n", 2)],
    "rt_math_eval64_device": [("op", 0), ("a", P), ("b", P), ("out", P), ("n", 2)],
}

def _null(*names):
    return dict.fromkeys(names)


# ---- the image-side queries: a device form (the arguments, then the stream), a _host form (the arguments) and a _cpu form of
# librt_host.so (the arguments), all three on one argument check.  The two A-Trous filters take a temp plane in the device and the
# _cpu form; the adaptive queries have no _host form.
_BASE = (C.addressof(BUF) + 15) & ~15
A, B, D = C.c_void_p(_BASE), C.c_void_p(_BASE + 1024), C.c_void_p(_BASE + 2048)  # three distinct arrays, 16-byte aligned
ODD = C.c_void_p(_BASE + 4)  # not 16-byte aligned
GUIDES = _capi.DenoiseGuides()  # every plane left out
TGUIDES = _capi.TemporalGuides()
DENOISE = _capi.DenoiseParams(1.0, 1.0, 1.0, 0, 1, 0)
DENOISE_2 = _capi.DenoiseParams(1.0, 1.0, 1.0, 0, 2, 0)  # two levels: needs a temp plane
TEMPORAL = _capi.TemporalParams(0.9, 1.0, 0.1, 8, 0)
BOUNDS = _capi.BoundsParams(1.0, 1, 0)
SVGF_VARIANCE = _capi.SvgfVarianceParams(1.0, 1.0, 4, 0)
SVGF_ATROUS = _capi.SvgfAtrousParams(1.0, 1.0, 1.0, 0, 1, 0)
SVGF_ATROUS_2 = _capi.SvgfAtrousParams(1.0, 1.0, 1.0, 0, 2, 0)
UPSAMPLE = _capi.UpsampleParams(1.0, 1.0, 2, 1, 0)
BUDGET = _capi.SampleBudgetParams(1.0, 1e-3, 1, 4, 0)
EMPTY_FRAME = _capi.Frame.full(0, 6, 3)
SIDE = 1 << 16  # SIDE x SIDE is 2^32 pixels

_ACCUMULATE = [("color", A), ("motion", A), ("current", TGUIDES), ("previous", TGUIDES), ("params", TEMPORAL), ("rows", 4), ("cols", 4),
               ("history_in", A), ("history_out", B), ("variance", None)]
IMAGE_QUERIES = {
    "rt_denoise_atrous": [("color", A), ("guides", GUIDES), ("params", DENOISE), ("rows", 4), ("cols", 4), ("out", B)],
    "rt_temporal_motion": [("position", A), ("position_stride", 3), ("valid", None), ("valid_stride", 1), ("camera", CAMERA), ("frame", FRAME),
                           ("motion", B)],
    "rt_temporal_accumulate": _ACCUMULATE,
    "rt_svgf_variance": [("history", A), ("guides", GUIDES), ("params", SVGF_VARIANCE), ("rows", 4), ("cols", 4), ("variance_out", B)],
    "rt_svgf_atrous": [("color", A), ("color_stride", 3), ("variance", B), ("guides", GUIDES), ("params", SVGF_ATROUS), ("rows", 4), ("cols", 4),
                       ("out", D), ("variance_out", None)],
    "rt_temporal_bounds": [("color", A), ("color_stride", 3), ("object", None), ("object_stride", 1), ("valid", None), ("valid_stride", 1),
                           ("params", BOUNDS), ("rows", 4), ("cols", 4), ("box", B)],
    "rt_temporal_accumulate_bounded": _ACCUMULATE + [("box", D), ("clamped_length", 0), ("clamped", None)],
    "rt_temporal_feedback": [("color", A), ("color_stride", 3), ("valid", None), ("valid_stride", 1), ("rows", 4), ("cols", 4), ("history", B)],
    "rt_upsample_guided": [("color", A), ("color_stride", 3), ("low", GUIDES), ("object_lo", None), ("object_lo_stride", 1), ("full", GUIDES),
                           ("object_full", None), ("object_full_stride", 1), ("params", UPSAMPLE), ("rows", 4), ("cols", 4), ("out", B)],
    "rt_sample_budget": [("mean", A), ("mean_stride", 1), ("variance", B), ("variance_stride", 1), ("count", None), ("count_stride", 1),
                         ("valid", None), ("valid_stride", 1), ("params", BUDGET), ("n", 4), ("budget", D)],
    "rt_film_offsets_listed": [("frame", FRAME), ("pattern", 1), ("seed", 1), ("pixel", A), ("sample", B), ("total", D),
                               ("capacity", 4), ("offsets", A)],
}
WITH_TEMP = ("rt_denoise_atrous", "rt_svgf_atrous")
WITHOUT_HOST = ("rt_sample_budget", "rt_film_offsets_listed")
DEVICE, HOST, CPU = "", "_host", "_cpu"
for _name, _args in IMAGE_QUERIES.items():
    _temp = [("temp", None)] if _name in WITH_TEMP else []
    SIGNATURES[_name + DEVICE] = _args + _temp + [("stream", None)]
    SIGNATURES[_name + CPU] = _args + _temp
    if _name not in WITHOUT_HOST:
        SIGNATURES[_name + HOST] = _args

PIXELS = "rows * cols: 2^32 pixels or more"
# (query, its forms the row holds for — None: all it has, the arguments that differ, status, the text after "<entry point>: ")
IMAGE_CASES = [
    ("rt_denoise_atrous", None, _null("guides"), INVALID, "null guides"),
    ("rt_denoise_atrous", None, {"rows": 0, "color": None, "out": None}, OK, None),
    ("rt_denoise_atrous", None, {"rows": SIDE, "cols": SIDE}, INVALID, PIXELS),
    ("rt_denoise_atrous", (DEVICE, CPU), {"params": DENOISE_2}, INVALID, "null temp pointer with n_levels >= 2"),
    ("rt_denoise_atrous", (DEVICE, CPU), {"params": DENOISE_2, "temp": B}, INVALID, "temp must not be out"),
    ("rt_temporal_motion", None, _null("camera"), INVALID, "null prev_camera"),
    ("rt_temporal_motion", None, {"frame": EMPTY_FRAME, "position": None, "motion": None}, OK, None),
    ("rt_temporal_motion", None, {"frame": HUGE_FRAME}, UNSUPPORTED, PIXELS),
    ("rt_temporal_motion", None, _null("motion"), INVALID, "null motion pointer"),
    ("rt_temporal_accumulate", None, {"rows": SIDE, "cols": SIDE}, UNSUPPORTED, PIXELS),
    ("rt_temporal_accumulate", None, {"cols": 0, "current": None, "previous": None, "params": None, "color": None, "history_out": None}, OK, None),
    ("rt_temporal_accumulate", None, _null("current"), INVALID, "null current guides"),
    ("rt_temporal_accumulate", (DEVICE,), {"history_in": ODD}, INVALID, "history_in and history_out must be 16-byte aligned"),
    ("rt_svgf_variance", None, _null("guides"), INVALID, "null guides"),
    ("rt_svgf_variance", None, {"cols": 0, "history": None, "variance_out": None}, OK, None),
    ("rt_svgf_variance", None, _null("history"), INVALID, "null history pointer"),
    ("rt_svgf_variance", (DEVICE,), {"history": ODD}, INVALID, "history must be 16-byte aligned"),
    ("rt_svgf_atrous", None, _null("guides"), INVALID, "null guides"),
    ("rt_svgf_atrous", None, {"rows": 0, "color": None, "variance": None, "out": None}, OK, None),
    ("rt_svgf_atrous", None, {"color_stride": 2}, INVALID, "color_stride must be at least 3 words"),
    ("rt_svgf_atrous", (DEVICE, CPU), {"params": SVGF_ATROUS_2}, INVALID, "null temp pointer with n_levels >= 2"),
    ("rt_svgf_atrous", (DEVICE, CPU), {"params": SVGF_ATROUS_2, "temp": D}, INVALID, "temp must not be color, variance, out or variance_out"),
    ("rt_temporal_bounds", None, {"rows": SIDE, "cols": SIDE}, UNSUPPORTED, PIXELS),
    ("rt_temporal_bounds", None, {"rows": 0, "params": None, "color": None, "box": None}, OK, None),
    ("rt_temporal_bounds", None, _null("params"), INVALID, "null params"),
    ("rt_temporal_bounds", (DEVICE,), {"box": ODD}, INVALID, "box must be 16-byte aligned"),
    ("rt_temporal_accumulate_bounded", None, {"rows": SIDE, "cols": SIDE}, UNSUPPORTED, PIXELS),
    ("rt_temporal_accumulate_bounded", None, {"rows": 0, "current": None, "params": None, "history_in": None, "box": None}, OK, None),
    ("rt_temporal_accumulate_bounded", None, _null("box"), INVALID, "null box pointer"),
    ("rt_temporal_accumulate_bounded", None, {"clamped_length": 9}, INVALID, "clamped_length must not exceed max_length (0: the length is not cut)"),
    ("rt_temporal_accumulate_bounded", (DEVICE,), {"history_out": ODD}, INVALID, "history_in and history_out must be 16-byte aligned"),
    ("rt_temporal_accumulate_bounded", (DEVICE,), {"box": ODD}, INVALID, "box must be 16-byte aligned"),
    ("rt_temporal_feedback", None, {"rows": SIDE, "cols": SIDE}, UNSUPPORTED, PIXELS),
    ("rt_temporal_feedback", None, {"cols": 0, "color": None, "history": None}, OK, None),
    ("rt_temporal_feedback", None, _null("color"), INVALID, "null color pointer"),
    ("rt_temporal_feedback", (DEVICE,), {"history": ODD}, INVALID, "history must be 16-byte aligned"),
    ("rt_upsample_guided", None, _null("params"), INVALID, "null params"),
    ("rt_upsample_guided", None, {"rows": 0, "color": None, "out": None}, OK, None),
    ("rt_upsample_guided", None, {"object_full": A, "object_full_stride": 0}, INVALID, "object_full_stride must be at least 1 word"),
    ("rt_upsample_guided", None, _null("out"), INVALID, "null out pointer"),
    ("rt_sample_budget", None, {"n": BIG}, UNSUPPORTED, "2^32 pixels or more"),
    ("rt_sample_budget", None, {"n": 0, "params": None, "mean": None, "budget": None}, OK, None),
    ("rt_sample_budget", None, _null("params"), INVALID, "null params"),
    ("rt_film_offsets_listed", None, _null("frame"), INVALID, "null frame"),
    ("rt_film_offsets_listed", None, {"capacity": 0, "pixel": None, "sample": None, "total": None, "offsets": None}, OK, None),
    ("rt_film_offsets_listed", None, {"capacity": BIG}, UNSUPPORTED, "2^32 pixels or records or more"),
]

RECORDS = "2^32 records or more (checked first; query them in several calls)"
LEVEL = "2^32 records or more (checked first; split the level)"
FRAME_NEEDS = "bad frame (need 0 <= x0 < x1 <= width, 0 <= y0 < y1 <= height, y_step >= 1)"

# (entry point, the arguments that differ from SIGNATURES, status, rt_last_error() — None where the status is RT_OK)
CASES = [
    ("rt_set_option", _null("name"), INVALID, "rt_set_option: null name"),
    ("rt_set_option", {"name": b"RT_AMD_NO_SUCH_SWITCH"}, INVALID, "rt_set_option: unknown option RT_AMD_NO_SUCH_SWITCH"),
    ("rt_set_option", {"value": b"1x"}, INVALID, "rt_set_option: the value is not an integer"),
    ("rt_set_variant", {"variant": 5}, INVALID, "rt_set_variant: 2, 3, 18 or 19 (include/rt_amd.h)"),
    ("rt_set_wavefront_budget", {"budget": 0}, INVALID, "rt_set_wavefront_budget: 1..4096 nodes per pixel"),
    ("rt_set_wavefront_budget", {"budget": 4097}, INVALID, "rt_set_wavefront_budget: 1..4096 nodes per pixel"),
    ("rt_profile_read", _null("ms"), INVALID, "rt_profile_read: null argument"),
    ("rt_profile_read", _null("launches"), INVALID, "rt_profile_read: null argument"),
    ("rt_profile_read_distributed", _null("ms"), INVALID, "rt_profile_read_distributed: null argument"),
    ("rt_scene_create", _null("desc"), INVALID, "rt_scene_create: null argument"),
    ("rt_scene_create", _null("out"), INVALID, "rt_scene_create: null argument"),
    ("rt_scene_describe_filters", _null("desc"), INVALID, "rt_scene_describe_filters: null argument"),
    ("rt_diag_scene_nodes", _null("scene"), INVALID, "rt_diag_scene_nodes: null argument"),
    ("rt_diag_pwf_plan", _null("scene"), INVALID, "rt_diag_pwf_plan: null argument"),
    ("rt_diag_pwf_plan", _null("words"), INVALID, "rt_diag_pwf_plan: null argument"),
    ("rt_diag_pwf_plan", _null("frame"), INVALID, "render: " + FRAME_NEEDS),
    ("rt_diag_pwf_plan", {"frame": BAD_FRAME}, INVALID, "render: " + FRAME_NEEDS),
    ("rt_diag_pwf_plan", {"frame": HUGE_FRAME}, UNSUPPORTED, "render: tile of 2^32 pixels or more (render it as several tiles)"),
    ("rt_diag_pwf_plan", {"frame": DEEP_FRAME}, UNSUPPORTED, "render: max_depth above RT_MAX_DEPTH"),
    ("rt_diag_pwf_plan_rays", {"n": BIG}, UNSUPPORTED, "rt_diag_pwf_plan_rays: 2^32 rays or more (checked first; trace them in several calls)"),
    ("rt_diag_pwf_plan_rays", _null("scene"), INVALID, "rt_diag_pwf_plan_rays: null argument"),
    ("rt_diag_pwf_plan_rays", _null("words"), INVALID, "rt_diag_pwf_plan_rays: null argument"),
    ("rt_diag_pwf_plan_rays", {"n": 0}, INVALID, "rt_diag_pwf_plan_rays: an empty batch launches nothing"),
    ("rt_diag_pwf_plan_rays", {"depth": 33}, UNSUPPORTED, "rt_diag_pwf_plan_rays: max_depth above RT_MAX_DEPTH"),
    ("rt_diag_pwf_outcome", _null("scene"), INVALID, "rt_diag_pwf_outcome: null argument"),
    ("rt_diag_pwf_outcome", _null("words"), INVALID, "rt_diag_pwf_outcome: null argument"),
    # the Whitted frame and the ray batch
    ("rt_render_whitted", _null("scene"), INVALID, "rt_render_whitted: null argument"),
    ("rt_render_whitted", _null("rgb"), INVALID, "rt_render_whitted: null argument"),
    ("rt_render_whitted", _null("camera"), INVALID, "render: null camera"),
    ("rt_render_whitted", _null("frame"), INVALID, "render: " + FRAME_NEEDS),
    ("rt_render_whitted", {"frame": BAD_FRAME}, INVALID, "render: " + FRAME_NEEDS),
    ("rt_render_whitted", {"frame": HUGE_FRAME}, UNSUPPORTED, "render: tile of 2^32 pixels or more (render it as several tiles)"),
    ("rt_render_whitted", {"frame": DEEP_FRAME}, UNSUPPORTED, "render: max_depth above RT_MAX_DEPTH"),
    ("rt_render_whitted_host", _null("scene"), INVALID, "rt_render_whitted_host: null argument"),
    ("rt_render_whitted_host", _null("rgb"), INVALID, "rt_render_whitted_host: null argument"),
    ("rt_render_whitted_host", {"frame": BAD_FRAME}, INVALID, "rt_render_whitted_host: bad frame"),
    ("rt_trace_rays", {"n": BIG}, UNSUPPORTED, "rt_trace_rays: 2^32 rays or more (checked first; trace them in several calls)"),
    ("rt_trace_rays", {"n": BIG, "scene": None, "rays": None}, UNSUPPORTED, "rt_trace_rays: 2^32 rays or more (checked first; trace them in several calls)"),
    ("rt_trace_rays", _null("scene"), INVALID, "rt_trace_rays: null scene"),
    ("rt_trace_rays", {"n": 0, "scene": None}, INVALID, "rt_trace_rays: null scene"),
    ("rt_trace_rays", {"n": 0, "rays": None, "rgb": None}, OK, None),
    ("rt_trace_rays", _null("rays"), INVALID, "rt_trace_rays: null ray or rgb pointer"),
    ("rt_trace_rays", _null("rgb"), INVALID, "rt_trace_rays: null ray or rgb pointer"),
    ("rt_trace_rays", {"depth": 33}, UNSUPPORTED, "rt_trace_rays: max_depth above RT_MAX_DEPTH"),
    ("rt_trace_rays_host", {"n": BIG}, UNSUPPORTED, "rt_trace_rays_host: 2^32 rays or more (checked first; trace them in several calls)"),
    ("rt_trace_rays_host", _null("scene"), INVALID, "rt_trace_rays_host: null scene"),
    ("rt_trace_rays_host", {"n": 0, "scene": None}, INVALID, "rt_trace_rays_host: null scene"),
    ("rt_trace_rays_host", {"n": 0, "rays": None, "rgb": None}, OK, None),
    ("rt_trace_rays_host", _null("rays"), INVALID, "rt_trace_rays_host: null ray or rgb pointer"),
    ("rt_trace_rays_host", _null("rgb"), INVALID, "rt_trace_rays_host: null ray or rgb pointer"),
    ("rt_trace_rays_host", {"depth": 33}, UNSUPPORTED, "rt_trace_rays_host: max_depth above RT_MAX_DEPTH"),
    # ray queries
    ("rt_cast_rays", {"n": BIG}, UNSUPPORTED, "rt_cast_rays: 2^32 rays or more (checked first; cast them in several calls)"),
    ("rt_cast_rays", _null("scene"), INVALID, "rt_cast_rays: null scene"),
    ("rt_cast_rays", {"n": 0, "scene": None}, INVALID, "rt_cast_rays: null scene"),
    ("rt_cast_rays", {"n": 0, "rays": None, "hits": None}, OK, None),
    ("rt_cast_rays", _null("rays"), INVALID, "rt_cast_rays: null ray or hit pointer"),
    ("rt_cast_rays", _null("hits"), INVALID, "rt_cast_rays: null ray or hit pointer"),
    ("rt_cast_rays_host", {"n": BIG}, UNSUPPORTED, "rt_cast_rays_host: 2^32 rays or more (checked first; cast them in several calls)"),
    ("rt_cast_rays_host", _null("scene"), INVALID, "rt_cast_rays_host: null scene"),
    ("rt_cast_rays_host", {"n": 0, "rays": None, "hits": None}, OK, None),
    ("rt_cast_rays_host", _null("rays"), INVALID, "rt_cast_rays_host: null ray or hit pointer"),
    ("rt_cast_rays_host", _null("hits"), INVALID, "rt_cast_rays_host: null ray or hit pointer"),
    ("rt_camera_rays", _null("camera"), INVALID, "rt_camera_rays: null argument"),
    ("rt_camera_rays", _null("frame"), INVALID, "rt_camera_rays: null argument"),
    ("rt_camera_rays", {"frame": BAD_FRAME}, INVALID, "rt_camera_rays: " + FRAME_NEEDS),
    ("rt_camera_rays", _null("rays"), INVALID, "rt_camera_rays: null ray pointer"),
    ("rt_camera_rays", {"frame": HUGE_FRAME}, UNSUPPORTED, "render: tile of 2^32 pixels or more (render it as several tiles)"),
    # hit queries
    ("rt_shade_hits", {"n": BIG}, UNSUPPORTED, "rt_shade_hits: " + RECORDS),
    ("rt_shade_hits", _null("scene"), INVALID, "rt_shade_hits: null scene"),
    ("rt_shade_hits", {"n": 0, "scene": None}, INVALID, "rt_shade_hits: null scene"),
    ("rt_shade_hits", {"n": 0, "hits": None, "incoming": None, "rgb": None}, OK, None),
    ("rt_shade_hits", _null("hits"), INVALID, "rt_shade_hits: null hit, incoming-ray or rgb pointer"),
    ("rt_shade_hits", _null("incoming"), INVALID, "rt_shade_hits: null hit, incoming-ray or rgb pointer"),
    ("rt_shade_hits", _null("rgb"), INVALID, "rt_shade_hits: null hit, incoming-ray or rgb pointer"),
    ("rt_shade_hits_host", {"n": BIG}, UNSUPPORTED, "rt_shade_hits_host: " + RECORDS),
    ("rt_shade_hits_host", _null("scene"), INVALID, "rt_shade_hits_host: null scene"),
    ("rt_shade_hits_host", {"n": 0, "hits": None}, OK, None),
    ("rt_shade_hits_host", _null("rgb"), INVALID, "rt_shade_hits_host: null hit, incoming-ray or rgb pointer"),
    ("rt_reflect_rays", {"n": BIG}, UNSUPPORTED, "rt_reflect_rays: " + RECORDS),
    ("rt_reflect_rays", {"n": 0, "hits": None, "incoming": None, "out": None}, OK, None),
    ("rt_reflect_rays", _null("hits"), INVALID, "rt_reflect_rays: null hit, incoming-ray or output pointer"),
    ("rt_reflect_rays", _null("out"), INVALID, "rt_reflect_rays: null hit, incoming-ray or output pointer"),
    ("rt_refract_rays", {"n": BIG}, UNSUPPORTED, "rt_refract_rays: " + RECORDS),
    ("rt_refract_rays", _null("scene"), INVALID, "rt_refract_rays: null scene"),
    ("rt_refract_rays", {"n": 0, "hits": None, "kind": None}, OK, None),
    ("rt_refract_rays", _null("kind"), INVALID, "rt_refract_rays: null hit, incoming-ray, kind or escape-ray pointer"),
    ("rt_refract_rays", _null("escape"), INVALID, "rt_refract_rays: null hit, incoming-ray, kind or escape-ray pointer"),
    ("rt_refract_rays_host", {"n": BIG}, UNSUPPORTED, "rt_refract_rays_host: " + RECORDS),
    ("rt_refract_rays_host", _null("scene"), INVALID, "rt_refract_rays_host: null scene"),
    ("rt_refract_rays_host", {"n": 0, "hits": None}, OK, None),
    ("rt_refract_rays_host", _null("incoming"), INVALID, "rt_refract_rays_host: null hit, incoming-ray, kind or escape-ray pointer"),
    # scatter queries
    ("rt_scatter_hits", {"n": BIG}, UNSUPPORTED, "rt_scatter_hits: " + RECORDS),
    ("rt_scatter_hits", _null("scene"), INVALID, "rt_scatter_hits: null scene"),
    ("rt_scatter_hits", _null("scene", "rng"), INVALID, "rt_scatter_hits: null scene"),
    ("rt_scatter_hits", _null("rng"), INVALID, "rt_scatter_hits: null rng"),
    ("rt_scatter_hits", {"n": 0, "rng": None}, INVALID, "rt_scatter_hits: null rng"),
    ("rt_scatter_hits", _null("index"), INVALID,
     "rt_scatter_hits: without an index array the RNG must hold as many generators as there are records"),
    ("rt_scatter_hits", {"n": 0, "index": None, "hits": None}, OK, None),
    ("rt_scatter_hits", _null("type"), INVALID, "rt_scatter_hits: null hit, incoming-ray, type or scattered-ray pointer"),
    ("rt_scatter_hits_host", {"n": BIG}, UNSUPPORTED, "rt_scatter_hits_host: " + RECORDS),
    ("rt_scatter_hits_host", _null("scene"), INVALID, "rt_scatter_hits_host: null scene"),
    ("rt_scatter_hits_host", _null("rng"), INVALID, "rt_scatter_hits_host: null rng"),
    ("rt_scatter_hits_host", _null("index"), INVALID,
     "rt_scatter_hits_host: without an index array the RNG must hold as many generators as there are records"),
    ("rt_scatter_hits_host", {"n": 0}, OK, None),
    ("rt_scatter_hits_host", _null("scattered"), INVALID, "rt_scatter_hits_host: null hit, incoming-ray, type or scattered-ray pointer"),
    ("rt_scatter_factors", {"n": BIG}, UNSUPPORTED, "rt_scatter_factors: " + RECORDS),
    ("rt_scatter_factors", _null("scene"), INVALID, "rt_scatter_factors: null scene"),
    ("rt_scatter_factors", {"n": 0, "hits": None, "rgb": None}, OK, None),
    ("rt_scatter_factors", _null("travel"), INVALID, "rt_scatter_factors: null hit, incoming-ray, type, next-ray, travel or rgb pointer"),
    ("rt_scatter_factors_host", {"n": BIG}, UNSUPPORTED, "rt_scatter_factors_host: " + RECORDS),
    ("rt_scatter_factors_host", _null("scene"), INVALID, "rt_scatter_factors_host: null scene"),
    ("rt_scatter_factors_host", {"n": 0, "hits": None}, OK, None),
    ("rt_scatter_factors_host", _null("next"), INVALID, "rt_scatter_factors_host: null hit, incoming-ray, type, next-ray, travel or rgb pointer"),
    # the level loop
    ("rt_select_records", {"n": BIG}, UNSUPPORTED, "rt_select_records: " + RECORDS),
    ("rt_select_records", {"n": 0, "flags": None, "index": None, "count": None}, OK, None),
    ("rt_select_records", _null("count"), INVALID, "rt_select_records: null flag, index or count pointer"),
    ("rt_cast_rays_indexed", {"n": BIG}, UNSUPPORTED,
     "rt_cast_rays_indexed: 2^32 rays or index entries or more (checked first; cast them in several calls)"),
    ("rt_cast_rays_indexed", {"max_count": BIG}, UNSUPPORTED,
     "rt_cast_rays_indexed: 2^32 rays or index entries or more (checked first; cast them in several calls)"),
    ("rt_cast_rays_indexed", _null("scene"), INVALID, "rt_cast_rays_indexed: null scene"),
    ("rt_cast_rays_indexed", {"n": 0, "scene": None}, INVALID, "rt_cast_rays_indexed: null scene"),
    ("rt_cast_rays_indexed", {"n": 0, "rays": None}, OK, None),
    ("rt_cast_rays_indexed", {"max_count": 0, "index": None}, OK, None),
    ("rt_cast_rays_indexed", _null("index"), INVALID, "rt_cast_rays_indexed: null ray, index, count or hit pointer"),
    ("rt_cast_rays_indexed", _null("hits"), INVALID, "rt_cast_rays_indexed: null ray, index, count or hit pointer"),
    ("rt_level_split", {"n": BIG}, UNSUPPORTED, "rt_level_split: " + RECORDS),
    ("rt_level_split", {"n": 0, "hits": None}, OK, None),
    ("rt_level_split", _null("refract"), INVALID, "rt_level_split: null hit, type, cosine or output pointer"),
    ("rt_level_join", {"n": BIG}, UNSUPPORTED, "rt_level_join: " + RECORDS),
    ("rt_level_join", {"n": 0, "type": None}, OK, None),
    ("rt_level_join", _null("flags"), INVALID, "rt_level_join: null type, cosine, reflected-ray, refraction-kind, escape-ray or output pointer"),
    ("rt_level_close", {"n": BIG}, UNSUPPORTED, "rt_level_close: " + RECORDS),
    ("rt_level_close", {"n": 0, "hits": None}, OK, None),
    ("rt_level_close", _null("missed"), INVALID, "rt_level_close: null hit, type, cosine, next-hit or output pointer"),
    ("rt_level_fold", {"n": BIG}, UNSUPPORTED, "rt_level_fold: " + RECORDS),
    ("rt_level_fold", {"n": 0, "value": None}, OK, None),
    ("rt_level_fold", _null("factor"), INVALID, "rt_level_fold: null type, cosine, next-hit, factor, shade or value pointer"),
    ("rt_level_finish", {"n": BIG}, UNSUPPORTED, "rt_level_finish: " + RECORDS),
    ("rt_level_finish", {"n": 0, "value": None, "accum": None, "valid": None}, OK, None),
    ("rt_level_finish", _null("value"), INVALID, "rt_level_finish: null value pointer"),
    ("rt_level_finish", _null("accum", "valid"), INVALID, "rt_level_finish: neither d_accum nor d_valid"),
    # the tree loop
    ("rt_tree_gate", {"n": BIG}, UNSUPPORTED, "rt_tree_gate: " + LEVEL),
    ("rt_tree_gate", {"n": 0, "contribution": None}, OK, None),
    ("rt_tree_gate", _null("flags"), INVALID, "rt_tree_gate: null contribution, flag or hit pointer"),
    ("rt_tree_split", {"n": BIG}, UNSUPPORTED, "rt_tree_split: " + LEVEL),
    ("rt_tree_split", _null("scene"), INVALID, "rt_tree_split: null scene"),
    ("rt_tree_split", {"n": 0, "scene": None}, INVALID, "rt_tree_split: null scene"),
    ("rt_tree_split", {"n": 0, "hits": None}, OK, None),
    ("rt_tree_split", _null("weights"), INVALID, "rt_tree_split: null hit, contribution, output-hit or weight pointer"),
    ("rt_tree_spawn", {"n": 1 << 31}, UNSUPPORTED, "rt_tree_spawn: 2^31 records or more (checked first; split the level)"),
    ("rt_tree_spawn", {"n": 0, "reflect": None}, OK, None),
    ("rt_tree_spawn", _null("child_values"), INVALID, "rt_tree_spawn: null reflect-hit, refraction-kind, flag or child-value pointer"),
    ("rt_tree_gather", {"max_count": BIG}, UNSUPPORTED, "rt_tree_gather: a capacity of 2^32 records or more (checked first; split the level)"),
    ("rt_tree_gather", {"max_count": BIG, "n": 1 << 31}, UNSUPPORTED,
     "rt_tree_gather: a capacity of 2^32 records or more (checked first; split the level)"),
    ("rt_tree_gather", {"n": 1 << 31}, UNSUPPORTED, "rt_tree_gather: 2^31 records or more (checked first; split the level)"),
    ("rt_tree_gather", {"n": 0, "index": None}, OK, None),
    ("rt_tree_gather", _null("overflow"), INVALID, "rt_tree_gather: null index, count, ray, contribution, weight, child or overflow pointer"),
    ("rt_tree_gather", _null("child_rays"), INVALID, "rt_tree_gather: null index, count, ray, contribution, weight, child or overflow pointer"),
    ("rt_tree_fold", {"n": BIG}, UNSUPPORTED, "rt_tree_fold: " + LEVEL),
    ("rt_tree_fold", {"n": 0, "hits": None}, OK, None),
    ("rt_tree_fold", _null("shade"), INVALID, "rt_tree_fold: null hit, shade, weight, refraction, child-value or output pointer"),
    ("rt_tree_fold", _null("travel"), INVALID, "rt_tree_fold: null hit, shade, weight, refraction, child-value or output pointer"),
    # light queries
    ("rt_light_rays", {"n": BIG}, UNSUPPORTED, "rt_light_rays: " + RECORDS),
    ("rt_light_rays", {"n": 1 << 20, "lights": 1 << 12}, UNSUPPORTED,
     "rt_light_rays: 2^32 (record, light) pairs or more (checked first; pass the lights in several ranges)"),
    ("rt_light_rays", _null("scene"), INVALID, "rt_light_rays: null scene"),
    ("rt_light_rays", {"n": 0, "scene": None}, INVALID, "rt_light_rays: null scene"),
    ("rt_light_rays", {"n": 0, "hits": None}, OK, None),
    ("rt_light_rays", {"lights": 0, "hits": None}, OK, None),
    ("rt_light_rays", _null("asks"), INVALID, "rt_light_rays: null hit, incoming-ray, shadow-ray or flag pointer"),
    ("rt_light_terms", {"n": BIG}, UNSUPPORTED, "rt_light_terms: " + RECORDS),
    ("rt_light_terms", {"n": 1 << 31, "lights": 2}, UNSUPPORTED,
     "rt_light_terms: 2^32 (record, light) pairs or more (checked first; pass the lights in several ranges)"),
    ("rt_light_terms", _null("scene"), INVALID, "rt_light_terms: null scene"),
    ("rt_light_terms", {"n": 0, "hits": None}, OK, None),
    ("rt_light_terms", _null("lit"), INVALID, "rt_light_terms: null hit, incoming-ray, flag, shadow-hit, lit, diffuse or specular pointer"),
    ("rt_light_fold", {"n": BIG}, UNSUPPORTED, "rt_light_fold: " + RECORDS),
    ("rt_light_fold", {"n": 1 << 31, "lights": 2}, UNSUPPORTED,
     "rt_light_fold: 2^32 (record, light) pairs or more (checked first; pass the lights in several ranges)"),
    ("rt_light_fold", _null("scene"), INVALID, "rt_light_fold: null scene"),
    ("rt_light_fold", {"lights": 0, "hits": None}, OK, None),
    ("rt_light_fold", _null("rgb"), INVALID, "rt_light_fold: null hit, lit, diffuse, specular or rgb pointer"),
    # refraction queries
    ("rt_refract_enter", {"n": BIG}, UNSUPPORTED, "rt_refract_enter: " + RECORDS),
    ("rt_refract_enter", _null("scene"), INVALID, "rt_refract_enter: null scene"),
    ("rt_refract_enter", {"n": 0, "scene": None}, INVALID, "rt_refract_enter: null scene"),
    ("rt_refract_enter", {"n": 0, "hits": None}, OK, None),
    ("rt_refract_enter", _null("casts"), INVALID, "rt_refract_enter: null hit, incoming-ray, ray, kind, travel, cast-count or flag pointer"),
    ("rt_refract_step", {"n": BIG}, UNSUPPORTED, "rt_refract_step: " + RECORDS),
    ("rt_refract_step", _null("scene"), INVALID, "rt_refract_step: null scene"),
    ("rt_refract_step", {"n": 0, "hits": None}, OK, None),
    ("rt_refract_step", _null("escape"), INVALID,
     "rt_refract_step: null hit, inside-hit, ray, kind, travel, cast-count, flag or escape-ray pointer"),
    # scene updates (everything after the scene is read from it)
    ("rt_scene_update_vertices", _null("scene"), INVALID, "rt_scene_update_vertices: null scene"),
    ("rt_scene_update_spheres", _null("scene"), INVALID, "rt_scene_update_spheres: null scene"),
    ("rt_scene_update_lights", _null("scene"), INVALID, "rt_scene_update_lights: null scene"),
    ("rt_scene_update_materials", _null("scene"), INVALID, "rt_scene_update_materials: null scene"),
    # record ordering
    ("rt_ray_keys", {"n": BIG}, UNSUPPORTED, "rt_ray_keys: 2^32 rays or more (checked first; key them in several calls)"),
    ("rt_ray_keys", {"n": 0, "rays": None, "keys": None}, OK, None),
    ("rt_ray_keys", _null("lo"), INVALID, "rt_ray_keys: null ray, box or key pointer"),
    ("rt_ray_keys", _null("keys"), INVALID, "rt_ray_keys: null ray, box or key pointer"),
    ("rt_ray_keys", {"flags": 2}, INVALID, "rt_ray_keys: unknown flag bit (RT_ORDER_DIRECTION_MAJOR is the only one)"),
    ("rt_sort_records", {"n": BIG}, UNSUPPORTED, "rt_sort_records: 2^32 records or more (checked first; sort them in several calls)"),
    ("rt_sort_records", {"n": 0, "keys": None, "temp": None}, OK, None),
    ("rt_sort_records", _null("temp"), INVALID, "rt_sort_records: null key, output or workspace pointer"),
    ("rt_sort_records", {"key_bits": 0}, INVALID, "rt_sort_records: need key_bits >= 1 and first_bit + key_bits <= 32"),
    ("rt_sort_records", {"first_bit": 30, "key_bits": 3}, INVALID, "rt_sort_records: need key_bits >= 1 and first_bit + key_bits <= 32"),
    ("rt_sort_records", {"temp_bytes": 16}, INVALID, "rt_sort_records: the workspace is smaller than rt_sort_temp_bytes(n)"),
    ("rt_sort_records", _null("index_in"), INVALID, "rt_sort_records: a count without an index list (the identity list has n entries)"),
    ("rt_gather_records", {"n": BIG}, UNSUPPORTED,
     "rt_gather_records: 2^32 records or index entries or more (checked first; move them in several calls)"),
    ("rt_gather_records", {"max_count": BIG}, UNSUPPORTED,
     "rt_gather_records: 2^32 records or index entries or more (checked first; move them in several calls)"),
    ("rt_gather_records", {"n": 0, "src": None}, OK, None),
    ("rt_gather_records", {"max_count": 0, "src": None}, OK, None),
    ("rt_gather_records", _null("index"), INVALID, "rt_gather_records: null source, index or destination pointer"),
    ("rt_gather_records", {"record_bytes": 6}, INVALID, "rt_gather_records: record_bytes must be a multiple of 4 from 4 to 256"),
    ("rt_gather_records", {"record_bytes": 260}, INVALID, "rt_gather_records: record_bytes must be a multiple of 4 from 4 to 256"),
    ("rt_scatter_records", {"n": BIG}, UNSUPPORTED,
     "rt_scatter_records: 2^32 records or index entries or more (checked first; move them in several calls)"),
    ("rt_scatter_records", {"n": 0, "src": None}, OK, None),
    ("rt_scatter_records", _null("dst"), INVALID, "rt_scatter_records: null source, index or destination pointer"),
    ("rt_scatter_records", {"record_bytes": 0}, INVALID, "rt_scatter_records: record_bytes must be a multiple of 4 from 4 to 256"),
    # mesh ordering
    ("rt_triangle_keys", {"n": BIG}, UNSUPPORTED, "rt_triangle_keys: 2^32 triangles or more (checked first)"),
    ("rt_triangle_keys", {"n": 0, "triangles": None}, OK, None),
    ("rt_triangle_keys", _null("hi"), INVALID, "rt_triangle_keys: null triangle, box or key pointer"),
    ("rt_order_triangles", {"n": BIG}, UNSUPPORTED, "rt_order_triangles: 2^32 triangles or more (checked first)"),
    ("rt_order_triangles", {"n": 0, "triangles": None}, OK, None),
    ("rt_order_triangles", _null("perm"), INVALID, "rt_order_triangles: null triangle, box, permutation or workspace pointer"),
    ("rt_order_triangles", {"temp_bytes": 16}, INVALID, "rt_order_triangles: the workspace is smaller than rt_order_triangles_temp_bytes(n)"),
    ("rt_order_triangles_host", {"n": BIG}, UNSUPPORTED, "rt_order_triangles_host: 2^32 triangles or more (checked first)"),
    ("rt_order_triangles_host", {"n": 0, "triangles": None}, OK, None),
    ("rt_order_triangles_host", _null("lo"), INVALID, "rt_order_triangles_host: null triangle, box or permutation pointer"),
    # the generators and the depth-of-field pass
    ("rt_rng_create", _null("out"), INVALID, "rt_rng_create: null argument"),
    ("rt_rng_create", {"frame": BAD_FRAME}, INVALID, "rt_rng_create: bad frame"),
    ("rt_rng_create", {"frame": HUGE_FRAME}, UNSUPPORTED, "rt_rng_create: tile of 2^32 pixels or more"),
    ("rt_rng_create_seeded", {"n": BIG}, UNSUPPORTED, "rt_rng_create_seeded: 2^32 generators or more (checked first)"),
    ("rt_rng_create_seeded", _null("out"), INVALID, "rt_rng_create_seeded: null argument"),
    ("rt_rng_create_seeded", _null("seeds"), INVALID, "rt_rng_create_seeded: null seed pointer"),
    ("rt_rng_download", _null("rng"), INVALID, "rt_rng_download: null argument"),
    ("rt_rng_download", _null("states"), INVALID, "rt_rng_download: null argument"),
    ("rt_rng_download", {}, OK, None),  # no generators: nothing to copy
    ("rt_rng_upload", _null("rng"), INVALID, "rt_rng_upload: null argument"),
    ("rt_rng_upload", {}, OK, None),
    ("rt_render_distributed", _null("scene"), INVALID, "rt_render_distributed: null argument"),
    ("rt_render_distributed", _null("rng"), INVALID, "rt_render_distributed: null argument"),
    ("rt_render_distributed", _null("accum", "samples"), INVALID, "rt_render_distributed: need d_accum or d_samples"),
    ("rt_render_distributed", _null("camera"), INVALID, "render: null camera"),
    ("rt_render_distributed", {"frame": BAD_FRAME}, INVALID, "render: " + FRAME_NEEDS),
    ("rt_render_distributed", {}, INVALID, "rt_render_distributed: the RNG was created for a different tile"),
    ("rt_render_distributed_host", _null("accum"), INVALID, "rt_render_distributed_host: null argument"),
    ("rt_render_distributed_host", {"frame": BAD_FRAME}, INVALID, "rt_render_distributed_host: bad frame"),
    ("rt_trace_rays_distributed", {"n": BIG}, UNSUPPORTED,
     "rt_trace_rays_distributed: 2^32 rays or more (checked first; trace them in several calls)"),
    ("rt_trace_rays_distributed", _null("scene"), INVALID, "rt_trace_rays_distributed: null scene"),
    ("rt_trace_rays_distributed", _null("rng"), INVALID, "rt_trace_rays_distributed: null rng"),
    ("rt_trace_rays_distributed", {"n": 2}, INVALID,
     "rt_trace_rays_distributed: the RNG holds a different number of generators than there are rays"),
    ("rt_trace_rays_distributed", {"rays": None, "accum": None, "samples": None}, OK, None),
    ("rt_trace_rays_distributed_host", {"n": BIG}, UNSUPPORTED,
     "rt_trace_rays_distributed_host: 2^32 rays or more (checked first; trace them in several calls)"),
    ("rt_trace_rays_distributed_host", _null("scene"), INVALID, "rt_trace_rays_distributed_host: null scene"),
    ("rt_trace_rays_distributed_host", _null("rng"), INVALID, "rt_trace_rays_distributed_host: null rng"),
    ("rt_trace_rays_distributed_host", {"n": 2}, INVALID,
     "rt_trace_rays_distributed_host: the RNG holds a different number of generators than there are rays"),
    ("rt_trace_rays_distributed_host", {"rays": None, "accum": None}, OK, None),
    ("rt_focus_rays", _null("camera"), INVALID, "rt_focus_rays: null argument"),
    ("rt_focus_rays", _null("rng"), INVALID, "rt_focus_rays: null argument"),
    ("rt_focus_rays", {"frame": BAD_FRAME}, INVALID, "rt_focus_rays: " + FRAME_NEEDS),
    ("rt_focus_rays", _null("rays"), INVALID, "rt_focus_rays: null ray pointer"),
    ("rt_focus_rays", {}, INVALID,
     "rt_focus_rays: the RNG was created for a different tile (or, seeded, holds a different number of generators)"),
    # after the render
    ("rt_post_process_device", _null("rgb"), INVALID, "rt_post_process_device: null argument"),
    ("rt_post_process_device", {"n": 0}, OK, None),
    ("rt_post_keys_device", _null("state"), INVALID, "rt_post_keys_device: null argument"),
    ("rt_post_keys_device", _null("keys"), INVALID, "rt_post_keys_device: null argument"),
    ("rt_post_hist_device", _null("state"), INVALID, "rt_post_hist_device: null argument"),
    ("rt_post_hist_device", {"pass_": 4}, INVALID, "rt_post_hist_device: pass 0..3"),
    ("rt_post_pick_device", _null("state"), INVALID, "rt_post_pick_device: null argument"),
    ("rt_post_pick_device", {"pass_": -1}, INVALID, "rt_post_pick_device: pass 0..3"),
    ("rt_post_scale_device", _null("state"), INVALID, "rt_post_scale_device: null argument"),
    ("rt_post_scale_device", _null("rgb"), INVALID, "rt_post_scale_device: null argument"),
    ("rt_accumulate_device", _null("weight"), INVALID, "rt_accumulate_device: null argument"),
    ("rt_accumulator_resolve_device", _null("sum"), INVALID, "rt_accumulator_resolve_device: null argument"),
    ("rt_encode_srgb8_device", _null("out"), INVALID, "rt_encode_srgb8_device: null argument"),
    ("rt_math_eval_host", _null("x"), INVALID, "rt_math_eval_host: null argument"),
    ("rt_math_eval_device", _null("out"), INVALID, "rt_math_eval_device: null argument"),
    ("rt_math_eval_device", {"n": 0}, OK, None),
    ("rt_math_eval64_host", _null("a"), INVALID, "rt_math_eval64_host: null argument"),
    ("rt_math_eval64_host", _null("out"), INVALID, "rt_math_eval64_host: null argument"),
    ("rt_math_eval64_device", _null("a"), INVALID, "rt_math_eval64_device: null argument"),
    ("rt_math_eval64_device", _null("out"), INVALID, "rt_math_eval64_device: null argument"),
    ("rt_math_eval64_device", {"n": 0}, OK, None),
]
# the image-side queries: every row in every form it holds for, under that entry point's name
CASES += [(name + form, changed, status, None if text is None else f"{name + form}: {text}")
          for name, forms, changed, status, text in IMAGE_CASES
          for form in (forms or (DEVICE, HOST, CPU)) if name + form in SIGNATURES]


def case_id(case):
    name, changed = case[0], case[1]
    return name + "(" + ",".join(k if v is None else f"{k}={'BIG' if v == BIG else v if isinstance(v, int) else '*'}" for k, v in changed.items()) + ")"


def call(rng, case):
    """-> (status, the library's last error as text) of one case; the message is cleared of what an earlier case left by a call that
    fails with a text of its own.  A _cpu form is librt_host.so's and leaves its text in rt_host_last_error()."""
    name, changed = case[0], case[1]
    names = [k for k, _ in SIGNATURES[name]]
    assert set(changed) <= set(names), (name, changed)
    args = dict(SIGNATURES[name])
    args.update(changed)
    values = [rng if args[k] is RNG else args[k] for k in names]
    values = [C.byref(v) if isinstance(v, C.Structure) else v for v in values]
    if name.endswith(CPU):
        lib = _capi.host_lib()
        assert lib.rt_world_push_object(None, None) == INVALID  # leaves its own text behind: a case that sets none is seen
        return getattr(lib, name)(*values), lib.rt_host_last_error().decode()
    lib = _capi.amd_lib()
    assert lib.rt_set_variant(-1) == INVALID  # as above
    return getattr(lib, name)(*values), lib.rt_last_error().decode()


@pytest.fixture(scope="module")
def empty_rng():
    lib = _capi.amd_lib()
    h = C.c_void_p()
    assert lib.rt_rng_create_seeded(None, 0, C.byref(h)) == 0 and h.value
    yield h
    assert lib.rt_rng_destroy(h) == 0


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_status_and_message(case, empty_rng):
    status, text = call(empty_rng, case)
    assert status == case[2]
    if case[3] is not None:
        assert text == case[3]


def test_every_entry_point_of_the_table_has_a_case_and_is_exported():
    assert {c[0] for c in CASES} == set(SIGNATURES)
    assert {name for name in SIGNATURES if not name.endswith(CPU)} <= set(_capi.AMD_SYMBOLS)
    assert {name for name in SIGNATURES if name.endswith(CPU)} <= set(_capi.HOST_SYMBOLS)


def test_every_form_of_an_image_side_query_has_its_first_refusal_and_its_empty_image():
    for name in IMAGE_QUERIES:
        for form in (DEVICE, HOST, CPU):
            if name + form in SIGNATURES:
                statuses = [c[2] for c in CASES if c[0] == name + form]
                assert OK in statuses and any(s != OK for s in statuses), name + form
