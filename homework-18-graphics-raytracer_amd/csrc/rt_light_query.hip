/*
 * rt_light_query.hip — get_shade (main.rs:407-464) opened into the calls between its casts (include/rt_amd.h "light queries"): which
 * lights ask for a shadow cast and with which ray, the occlusion rule and the Phong terms once those rays have been cast, and the
 * weighted sum — so that the shadow rays are records like every other ray (rt_select_records + rt_cast_rays_indexed cast them, on a
 * scene walked breadth-first with that walk), and a caller can change the light loop: per-light output, a subset of lights, a shadow
 * rule of its own, a re-weighting of diffuse against specular.
 *
 *   rt::light_rays_kernel    main.rs:408-433 per (record, light): the flag "this light asks", the shadow ray, the distance to the light
 *   rt::light_terms_kernel   main.rs:435-459 per (record, light): lit or occluded, and the locals `diffuse` and `specular`
 *   rt::light_fold_kernel    main.rs:461 per record, over the lights in order, in place
 *
 * Nothing here is new arithmetic: hit_from_abi, ray_from_abi, material_approx, adjust_normal, light_asks, approximate_into_directional,
 * get_diffuse and get_specular are called as rt::shade_hits_kernel (rt_hit_query.hip) calls them, with the same operands in the same
 * order, and the unit is compiled with -ffp-contract=off like every other — so every bit is rt_shade_hits'.  One record per lane, the
 * record number counted in 64 bits; the material and the bump normal once per record, not once per pair; the light loop is wave-uniform
 * (the light record comes through uniform_ref: scalar loads); per-(light, record) arrays are light-major, entry (l - light_first) * n + i,
 * so that the stores of one light's plane are coalesced.  Records move as dwords.  No LDS, no cast.  The C entry points of the block are
 * at the end of the file.
 */
#include "rt_api_internal.h"
#include "rt_light_record.h" /* light_record: what get_shade computes once per hit */

namespace rt {

/* main.rs:408-433 */
__global__ __launch_bounds__(RT_LIGHT_THREADS) void light_rays_kernel(const KernelScene sc, const rt_hit *__restrict__ hits, const uint64_t n,
                                                                      const uint32_t light_first, const uint32_t light_count,
                                                                      rt_ray *__restrict__ shadow_rays, unsigned char *__restrict__ asks,
                                                                      float *__restrict__ light_distance) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_LIGHT_THREADS + threadIdx.x;
    if (i >= n) return;
    const LightRecord r = light_record(sc, hits, i);
    const V3 pos = r.h.g.pos;
    for (uint32_t l = 0; l < light_count; ++l) { /* wave-uniform */
        const auto &L = uniform_ref(sc.lights + (light_first + l));
        const uint64_t k = (uint64_t)l * n + i;
        V3 l_direction = v3(0.0f, 0.0f, 0.0f);
        const bool need = light_asks(L, uniform_ref(sc.light_aux + (light_first + l)), pos, r.adj_n, &l_direction) && r.valid;
        asks[k] = need ? 1 : 0;
        if (need) /* shadow_ray, main.rs:426-433: bit for bit the ray shade_hits_kernel casts */
            store_ray(shadow_rays + k, pos, -l_direction, FACE_BACK, 1u, r.h.kind, r.h.index, FACE_BACK);
        else
            store_ray(shadow_rays + k, v3(0.0f, 0.0f, 0.0f), v3(0.0f, 0.0f, 0.0f), 0u, 0u, 0u, 0u, 0u);
        if (light_distance != nullptr) { /* what main.rs:439 compares against */
            const bool has_origin = (L.kind != RT_LIGHT_DIRECTIONAL) || (L.has_origin != 0u);
            const float d = has_origin ? distance(pos, v3(L.origin[0], L.origin[1], L.origin[2])) : __builtin_inff();
            light_distance[k] = need ? d : 0.0f;
        }
    }
}

/* main.rs:435-459 */
__global__ __launch_bounds__(RT_LIGHT_THREADS) void light_terms_kernel(const KernelScene sc, const rt_hit *__restrict__ hits,
                                                                       const rt_ray *__restrict__ incoming, const uint64_t n,
                                                                       const uint32_t light_first, const uint32_t light_count,
                                                                       const unsigned char *__restrict__ asks, const rt_hit *__restrict__ shadow_hits,
                                                                       unsigned char *__restrict__ lit_out, float *__restrict__ diffuse_out,
                                                                       float *__restrict__ specular_out) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_LIGHT_THREADS + threadIdx.x;
    if (i >= n) return;
    const LightRecord r = light_record(sc, hits, i);
    const V3 pos = r.h.g.pos;
    V3 view = v3(0.0f, 0.0f, 1.0f);
    if (r.valid) view = ray_from_abi(incoming + i, sc.n_triangles, sc.n_spheres).d; /* hit.ray.direction */
    for (uint32_t l = 0; l < light_count; ++l) { /* wave-uniform */
        const uint64_t k = (uint64_t)l * n + i;
        const bool asked = r.valid && asks[k] != 0;
        bool lit = false;
        V3 diffuse = v3(0.0f, 0.0f, 0.0f), specular = v3(0.0f, 0.0f, 0.0f);
        if (__builtin_amdgcn_ballot_w64(asked) != 0ull) { /* a wave nobody asks in skips the light: its acosf and powf are binary64 */
            const auto &L = uniform_ref(sc.lights + (light_first + l));
            if (asked) {
                lit = true;
                const uint32_t *const occluder = reinterpret_cast<const uint32_t *>(shadow_hits + k);
                if (occluder[0] <= 1u) { /* main.rs:435-448: Some(occlusion) */
                    const bool has_origin = (L.kind != RT_LIGHT_DIRECTIONAL) || (L.has_origin != 0u);
                    if (has_origin) {
                        const V3 occ = v3(__uint_as_float(occluder[RT_LIGHT_HIT_POSITION]), __uint_as_float(occluder[RT_LIGHT_HIT_POSITION + 1u]),
                                          __uint_as_float(occluder[RT_LIGHT_HIT_POSITION + 2u])); /* occlusion.at.position */
                        if (distance(pos, occ) < distance(pos, v3(L.origin[0], L.origin[1], L.origin[2]))) lit = false;
                    } else {
                        lit = false;
                    }
                }
                if (lit) {
                    DirLight dl;
                    dl.direction = dl.color = v3(0.0f, 0.0f, 0.0f);
                    lit = approximate_into_directional(L, pos, &dl); /* None only where the caller set a flag the light did not */
                    if (lit) {
                        const V3 light_direction = -dl.direction; /* the light's own, not the shadow record's: a caller may have replaced that ray */
                        diffuse = get_diffuse(r.m, r.adj_n, light_direction) * dl.color;
                        specular = get_specular(r.m, r.adj_n, -view, light_direction) * dl.color;
                    }
                }
            }
        }
        lit_out[k] = lit ? 1 : 0;
        diffuse_out[k * 3u] = diffuse.x;
        diffuse_out[k * 3u + 1u] = diffuse.y;
        diffuse_out[k * 3u + 2u] = diffuse.z;
        specular_out[k * 3u] = specular.x;
        specular_out[k * 3u + 1u] = specular.y;
        specular_out[k * 3u + 2u] = specular.z;
    }
}

/* main.rs:461 in shade_hits_kernel's association: (sum + diffuse * (1 - shiness)) + specular * shiness */
__global__ __launch_bounds__(RT_LIGHT_THREADS) void light_fold_kernel(const KernelScene sc, const rt_hit *__restrict__ hits, const uint64_t n,
                                                                      const uint32_t light_count, const unsigned char *__restrict__ lit,
                                                                      const float *__restrict__ diffuse, const float *__restrict__ specular,
                                                                      float *__restrict__ rgb) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_LIGHT_THREADS + threadIdx.x;
    if (i >= n) return;
    const AbiHit h = hit_from_abi(hits + i, sc.n_triangles, sc.n_spheres, sc.n_materials, true);
    if (!h.valid) return; /* "no hit": not written */
    const float shiness = material_approx(sc.materials[h.g.obj], h.g.u, h.g.v).shiness;
    V3 sum = v3(rgb[i * 3u], rgb[i * 3u + 1u], rgb[i * 3u + 2u]);
    for (uint32_t l = 0; l < light_count; ++l) {
        const uint64_t k = (uint64_t)l * n + i;
        if (lit[k] == 0) continue;
        const V3 d = v3(diffuse[k * 3u], diffuse[k * 3u + 1u], diffuse[k * 3u + 2u]);
        const V3 s = v3(specular[k * 3u], specular[k * 3u + 1u], specular[k * 3u + 2u]);
        sum = sum + d * (1.0f - shiness) + s * shiness;
    }
    rgb[i * 3u] = sum.x;
    rgb[i * 3u + 1u] = sum.y;
    rgb[i * 3u + 2u] = sum.z;
}

} /* namespace rt */

/* ---- the C entry points (include/rt_amd.h "light queries") ---- */

/* the block's checks before any device work, in the documented order; *done: nothing to launch.  light_first < 0: the call takes no
 * range of lights (rt_light_fold reads the material only) */
static int light_args(const char *who, const rt_scene *scene, size_t n, int64_t light_first, uint32_t light_count, bool pointers_ok,
                      const char *pointers, bool *done) {
    *done = true;
    int rc = check_count(who, n, RECORDS_2_32);
    if (rc == RT_OK) rc = check_count(who, (uint64_t)n * (uint64_t)light_count, {32u, "(record, light) pairs", "pass the lights in several ranges"});
    if (rc == RT_OK) rc = check_scene(who, scene);
    if (rc != RT_OK || n == 0 || light_count == 0) return rc;
    rc = check_pointers(who, pointers_ok, pointers);
    if (rc != RT_OK) return rc;
    if (light_first >= 0 && (uint64_t)light_first + (uint64_t)light_count > (uint64_t)scene->ks.n_lights)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": lights " + std::to_string(light_first) + " .. " +
                                                 std::to_string((uint64_t)light_first + light_count) + " of a scene with " + std::to_string(scene->ks.n_lights));
    *done = false;
    return RT_OK;
}

extern "C" {

int rt_light_rays(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, uint32_t light_first, uint32_t light_count,
                  rt_ray *d_shadow_rays, unsigned char *d_asks, float *d_light_distance, void *hip_stream) {
    bool done;
    const int rc = light_args("rt_light_rays", scene, n, light_first, light_count, d_hits && d_incoming && d_shadow_rays && d_asks,
                              "hit, incoming-ray, shadow-ray or flag", &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::light_rays_kernel, grid_of(n, RT_LIGHT_THREADS), dim3(RT_LIGHT_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks, d_hits,
                       (uint64_t)n, light_first, light_count, d_shadow_rays, d_asks, d_light_distance);
    return launched("rt_light_rays");
}

int rt_light_terms(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, uint32_t light_first, uint32_t light_count,
                   const unsigned char *d_asks, const rt_hit *d_shadow_hits, unsigned char *d_lit, float *d_diffuse, float *d_specular,
                   void *hip_stream) {
    bool done;
    const int rc = light_args("rt_light_terms", scene, n, light_first, light_count,
                              d_hits && d_incoming && d_asks && d_shadow_hits && d_lit && d_diffuse && d_specular,
                              "hit, incoming-ray, flag, shadow-hit, lit, diffuse or specular", &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::light_terms_kernel, grid_of(n, RT_LIGHT_THREADS), dim3(RT_LIGHT_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks, d_hits,
                       d_incoming, (uint64_t)n, light_first, light_count, d_asks, d_shadow_hits, d_lit, d_diffuse, d_specular);
    return launched("rt_light_terms");
}

int rt_light_fold(const rt_scene *scene, const rt_hit *d_hits, size_t n, uint32_t light_count, const unsigned char *d_lit, const float *d_diffuse,
                  const float *d_specular, float *d_rgb, void *hip_stream) {
    bool done;
    const int rc = light_args("rt_light_fold", scene, n, -1, light_count, d_hits && d_lit && d_diffuse && d_specular && d_rgb,
                              "hit, lit, diffuse, specular or rgb", &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::light_fold_kernel, grid_of(n, RT_LIGHT_THREADS), dim3(RT_LIGHT_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks, d_hits,
                       (uint64_t)n, light_count, d_lit, d_diffuse, d_specular, d_rgb);
    return launched("rt_light_fold");
}

} /* extern "C" */
