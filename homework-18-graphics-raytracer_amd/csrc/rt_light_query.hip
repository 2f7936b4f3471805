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
 * order, and the unit is compiled with -ffp-contract=off like every other — so every bit is rt_shade_hits'.  What is done per record
 * and per entry (light_record, store_shadow_ray, light_terms, fold_shiness) is rt_light_record.h's, where the area-light, hemisphere,
 * environment, lobe and texture queries take it from too; the kernels here are the loops around it.  One record per lane, the
 * record number counted in 64 bits; the material and the bump normal once per record, not once per pair; the light loop is wave-uniform
 * (the light record comes through uniform_ref: scalar loads); per-(light, record) arrays are light-major, entry (l - light_first) * n + i,
 * so that the stores of one light's plane are coalesced.  Records move as dwords.  No LDS, no cast.  The C entry points of the block are
 * at the end of the file.
 */
#include "rt_api_internal.h"
#include "rt_light_record.h"

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
        store_shadow_ray(shadow_rays + k, r, -l_direction, need);
        if (light_distance != nullptr) { /* what main.rs:439 compares against */
            const float d = area_light_has_origin(L) ? distance(pos, v3(L.origin[0], L.origin[1], L.origin[2])) : __builtin_inff();
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
        LightTerms t; /* not lit, +0 */
        if (__builtin_amdgcn_ballot_w64(asked) != 0ull) { /* a wave nobody asks in skips the light: its acosf and powf are binary64 */
            const auto &L = uniform_ref(sc.lights + (light_first + l));
            t = light_terms(L, area_light_has_origin(L), v3(L.origin[0], L.origin[1], L.origin[2]), pos, r.m, r.adj_n, view, asked, shadow_hits + k);
        }
        store_light_terms(lit_out, diffuse_out, specular_out, k, t);
    }
}

/* main.rs:461 in shade_hits_kernel's association: (sum + diffuse * (1 - shiness)) + specular * shiness */
__global__ __launch_bounds__(RT_LIGHT_THREADS) void light_fold_kernel(const KernelScene sc, const rt_hit *__restrict__ hits, const uint64_t n,
                                                                      const uint32_t light_count, const unsigned char *__restrict__ lit,
                                                                      const float *__restrict__ diffuse, const float *__restrict__ specular,
                                                                      float *__restrict__ rgb) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_LIGHT_THREADS + threadIdx.x;
    if (i >= n) return;
    bool valid;
    const float shiness = fold_shiness(sc, hits, i, &valid);
    if (!valid) return; /* "no hit": not written */
    V3 sum = load_v3(rgb, i);
    for (uint32_t l = 0; l < light_count; ++l) {
        const uint64_t k = (uint64_t)l * n + i;
        if (lit[k] == 0) continue;
        sum = sum + load_v3(diffuse, k) * (1.0f - shiness) + load_v3(specular, k) * shiness;
    }
    store_v3(rgb, i, sum);
}

} /* namespace rt */

/* ---- the C entry points (include/rt_amd.h "light queries") ---- */

/* the checks before any device work are hit_sample_args' (rt_api_internal.h); rt_light_fold takes no range of lights: it reads the
 * material only */
extern "C" {

int rt_light_rays(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, uint32_t light_first, uint32_t light_count,
                  rt_ray *d_shadow_rays, unsigned char *d_asks, float *d_light_distance, void *hip_stream) {
    bool done;
    const int rc = hit_sample_args("rt_light_rays", scene,
                                   HitSampleArgs(n, d_hits && d_incoming && d_shadow_rays && d_asks, "hit, incoming-ray, shadow-ray or flag")
                                       .lights(light_count, light_first), &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::light_rays_kernel, grid_of(n, RT_LIGHT_THREADS), dim3(RT_LIGHT_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks, d_hits,
                       (uint64_t)n, light_first, light_count, d_shadow_rays, d_asks, d_light_distance);
    return launched("rt_light_rays");
}

int rt_light_terms(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, uint32_t light_first, uint32_t light_count,
                   const unsigned char *d_asks, const rt_hit *d_shadow_hits, unsigned char *d_lit, float *d_diffuse, float *d_specular,
                   void *hip_stream) {
    bool done;
    const int rc = hit_sample_args("rt_light_terms", scene,
                                   HitSampleArgs(n, d_hits && d_incoming && d_asks && d_shadow_hits && d_lit && d_diffuse && d_specular,
                                                 "hit, incoming-ray, flag, shadow-hit, lit, diffuse or specular")
                                       .lights(light_count, light_first), &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::light_terms_kernel, grid_of(n, RT_LIGHT_THREADS), dim3(RT_LIGHT_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks, d_hits,
                       d_incoming, (uint64_t)n, light_first, light_count, d_asks, d_shadow_hits, d_lit, d_diffuse, d_specular);
    return launched("rt_light_terms");
}

int rt_light_fold(const rt_scene *scene, const rt_hit *d_hits, size_t n, uint32_t light_count, const unsigned char *d_lit, const float *d_diffuse,
                  const float *d_specular, float *d_rgb, void *hip_stream) {
    bool done;
    const int rc = hit_sample_args("rt_light_fold", scene,
                                   HitSampleArgs(n, d_hits && d_lit && d_diffuse && d_specular && d_rgb, "hit, lit, diffuse, specular or rgb").lights(light_count),
                                   &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::light_fold_kernel, grid_of(n, RT_LIGHT_THREADS), dim3(RT_LIGHT_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks, d_hits,
                       (uint64_t)n, light_count, d_lit, d_diffuse, d_specular, d_rgb);
    return launched("rt_light_fold");
}

} /* extern "C" */
