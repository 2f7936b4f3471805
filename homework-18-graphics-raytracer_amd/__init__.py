"""MI355X-native render path for the homework-18 raytracer — Python host mirror.

The product is the C-ABI library ``librt_amd.so`` (hand-written HIP for gfx950,
``csrc/rt_kernels.hip``) plus ``librt_host.so`` (scene build / OBJ import /
post_process / PNG, ``csrc/host/rt_host.cpp``).  This package only mirrors the
reference's host-side names on top of them:

    World / ObjectProxy            src/main.rs:130-178, 700-728
    Camera                         src/main.rs:43-49
    render (the Whitted par_iter)  src/main.rs:1087-1104
    cast_rays (World::cast)        src/main.rs:180-326, on caller-supplied rays
    trace_rays (World::ray_trace)  src/main.rs:466-519, on caller-supplied rays
    trace_rays_distributed         src/main.rs:521-614 (distributed_ray_trace), on caller-supplied rays
    shade_hits / reflect_rays / refract_rays   src/main.rs:407-464, 328-341, 343-405 (get_shade, get_reflect, get_refract), on caller-supplied hits
    trace_rays_distributed_levels  src/main.rs:521-614 again, one level at a time from the queries and the level-loop calls
    trace_rays_levels              src/main.rs:466-519 again, one level of the tree at a time from the queries and the tree-loop calls
    light_rays / light_terms / light_fold      src/main.rs:407-464 (get_shade) opened into the calls between its shadow casts
    shade_hits_by_light            src/main.rs:407-464 again, light by light from those calls, select_records and cast_rays_indexed
    refract_enter / refract_step   src/main.rs:343-405 (get_refract) opened into the calls between its casts
    refract_rays_by_bounce         src/main.rs:343-405 again, bounce by bounce from those calls, select_records and cast_rays_indexed
    ray_keys / sort_records / gather_records / scatter_records   the order of a batch: include/rt_amd.h "record ordering"
    cast_rays_ordered / trace_rays_ordered     cast_rays and trace_rays again, on rays the device put into a coherent order first
    triangle_keys / order_triangles / World.ordered   the order of a mesh: include/rt_amd.h "mesh ordering"
    unorder_hits / order_rays      triangle indices between an ordered world and the one it was made from
    materials (a submodule)        src/main.rs:408-410 and materials.rs:46-66: approx, adjust_normal and the Phong terms on caller-supplied hits
    film (a submodule)             src/photon.rs:30-33 (accumulate_weight) behind a reconstruction filter, and Camera::shoot through sub-pixel positions
    denoise (a submodule)          no counterpart in the reference: an edge-avoiding A-Trous filter guided by the planes of materials.primary_surfaces
    temporal (a submodule)         no counterpart in the reference: the previous frame's history reprojected, tested against the guides and blended, with luminance moments
    svgf (a submodule)             no counterpart in the reference: a variance for every history length and the variance-guided A-Trous filter that consume the temporal records
    moving (a submodule)           no counterpart in the reference: the positions a scene keeps before an update, and where each hit's point was on them — the plane temporal wants for moving geometry
    rectify (a submodule)          no counterpart in the reference: the colour box of a pixel's neighbourhood, the accumulate that clamps the history into it, and the feedback of the filtered colour into the records
    adaptive (a submodule)         no counterpart in the reference: a sample budget per pixel from a variance estimate, the ragged pixel-major list of those samples, and the film queries on such a list
    arealights (a submodule)       no counterpart in the reference: get_shade's light loop on lights that have a radius — sampled points on the light, the light queries on the displaced light, and a fold that averages the samples: soft shadows
    upsample (a submodule)         no counterpart in the reference: a low-resolution radiance carried onto full-resolution guide planes by a joint bilateral upsample
    hemisphere (a submodule)       no counterpart in the reference: cosine-distributed directions over a hit, their shadow rays, and a fold of the answers into ambient occlusion and one bounce of diffuse light
    environment (a submodule)      no counterpart in the reference (a ray that leaves the scene is black, src/main.rs:475): a lat-long sky looked up along the rays that found nothing, its sampling table built on the device, directions drawn from it over a hit with their shadow rays, and a fold of the answers: sky light
    lobes (a submodule)            no counterpart in the reference: directions drawn from a hit's own Phong lobes (the diffuse lobe about the normal, the specular lobe about the mirrored view), the density of a direction under that mixture and under an environment's table, and the weights of multiple importance sampling
    paths (a submodule)            no counterpart in the reference: the inner step of a path tracer on caller hits — a record that carries the throughput from bounce to bounce, one kernel per bounce that draws from the hit's lobes, weighs, deposits and plays Russian roulette, the mean of a pixel's paths, and the multi-bounce loop written from them
    textures (a submodule)         materials.rs:70-103, GenerativeMaterial's closures of uv read from images: mip-mapped textures and normal maps on rt_surface records, the cone footprint that chooses the level, and get_shade's light terms on such records
    bloom (a submodule)           src/main.rs:761, post_process's "TODO: highlight bloom effect": the highlights above a luma threshold spread down and up a pyramid and added back, between post_process and the encode
    post_process / write_to_file   src/main.rs:748-776

PyTorch is used only for device memory, streams and torch.distributed.
"""
from . import _capi, adaptive, arealights, bloom, denoise, diagnostics, environment, film, hemisphere, lobes, materials, moving, paths, rectify, svgf, temporal, textures, upsample
from ._capi import Camera, Frame, Light, Material, RtError, SceneDesc, Sphere, Triangle, Vertex
from ._world import DEFAULT_OBJ, ObjectProxy, Scene, World, reference_camera, reference_world
from ._render import (Rng, focus_rays, options, render_distributed, render_distributed_numpy, render_whitted, render_whitted_numpy,
                      set_option)
from ._queries import (BACK, BOTH, DIFFUSE, ESCAPED, FRONT, HIT_DTYPE, HIT_NONE, INFINITE, RAY_DTYPE, REFLECTION, REFRACTION, SPHERE,
                       TRAPPED, TRIANGLE, Hits, Refractions, Scatters, camera_rays, cast_rays, cast_rays_indexed, cast_rays_numpy,
                       make_rays, reflect_rays, refract_rays, refract_rays_numpy, scatter_factors, scatter_factors_numpy, scatter_hits,
                       scatter_hits_numpy, select_records, shade_hits, shade_hits_numpy, trace_rays, trace_rays_distributed,
                       trace_rays_distributed_numpy, trace_rays_numpy)
from ._opened import (WALKING, LightWorkspace, RefractWorkspace, light_fold, light_rays, light_terms, light_workspace,
                      refract_enter, refract_rays_by_bounce, refract_step, refract_workspace, shade_hits_by_light)
from ._loops import (LEVEL_CAPACITY_FACTOR, default_level_capacity, level_close, level_finish, level_fold, level_join, level_split,
                     trace_rays_distributed_levels, trace_rays_levels, tree_fold, tree_gate, tree_gather, tree_split, tree_spawn)
from ._ordering import (ORDER_DIRECTION_MAJOR, TRIANGLE_WORDS, OrderWorkspace, cast_rays_ordered, gather_records, order_rays,
                        order_triangles, order_triangles_temp_bytes, order_workspace, ray_keys, scatter_records, sort_records,
                        sort_temp_bytes, trace_rays_ordered, triangle_keys, unorder_hits)
from ._post import (PhotonAccumulator, encode_srgb8, encode_srgb8_device, luma_row, post_process, post_process_device,
                    write_to_file)

__all__ = [
    "World", "ObjectProxy", "Scene", "Camera", "Frame", "Material", "Light", "RtError", "reference_world",
    "reference_camera", "render_whitted", "render_whitted_numpy", "make_rays", "cast_rays", "Hits", "camera_rays", "cast_rays_numpy", "trace_rays", "trace_rays_numpy", "shade_hits", "reflect_rays", "refract_rays", "Refractions", "ESCAPED", "INFINITE", "TRAPPED", "HIT_NONE", "shade_hits_numpy", "refract_rays_numpy", "scatter_hits", "scatter_factors", "Scatters", "DIFFUSE", "REFLECTION", "REFRACTION", "scatter_hits_numpy", "scatter_factors_numpy", "select_records", "cast_rays_indexed", "level_split", "level_join", "level_close", "level_fold", "level_finish", "trace_rays_distributed_levels", "tree_gate", "tree_split", "tree_spawn", "tree_gather", "tree_fold", "trace_rays_levels", "default_level_capacity", "light_rays", "light_terms", "light_fold", "shade_hits_by_light", "light_workspace", "LightWorkspace", "WALKING", "refract_enter", "refract_step", "refract_rays_by_bounce", "refract_workspace", "RefractWorkspace", "ORDER_DIRECTION_MAJOR", "ray_keys", "sort_temp_bytes", "sort_records", "gather_records", "scatter_records", "order_workspace", "OrderWorkspace", "cast_rays_ordered", "trace_rays_ordered", "triangle_keys", "order_triangles_temp_bytes", "order_triangles", "unorder_hits", "order_rays", "Rng", "focus_rays", "trace_rays_distributed", "trace_rays_distributed_numpy", "render_distributed", "render_distributed_numpy", "set_option", "options", "post_process_device", "encode_srgb8_device", "post_process", "encode_srgb8", "write_to_file",
    "DEFAULT_OBJ",
]
