/*
 * rt_refract_query.hip — get_refract (main.rs:343-405) opened into the calls between its casts (include/rt_amd.h "refraction queries"):
 * the ray that enters the glass, and what one answered cast of the walk leads to — the next total-reflection bounce, the escape ray, or
 * the end — so that the 1 to 11 casts of a refraction are records like every other ray (rt_select_records + rt_cast_rays_indexed cast
 * them, on a scene walked breadth-first with that walk), and a caller can change the walk: a bounce limit of its own, an absorption rule
 * per segment, a stop at the first interior hit.
 *
 *   rt::refract_enter_kernel  main.rs:354-368 per record: Trapped at entry, or ray_inside and the state of a walk that has cast nothing
 *   rt::refract_step_kernel   main.rs:371-402 per walking record, for ONE answered cast: Infinite, the bounce ray, the escape ray or Trapped
 *
 * Nothing here is new arithmetic: hit_from_abi, ray_from_abi, material_approx, refract_dir, reflect_dir, normalize and distance are called
 * as rt::refract_rays_kernel (rt_hit_query.hip) calls them (the entry through rt_refract_entry.h, which rt_path_branch shares), with the same operands in the same order, and the unit is compiled with
 * -ffp-contract=off like every other — so every bit is rt_refract_rays'.  One record per lane, the record number counted in 64 bits.
 * The walk's state lives in the caller's arrays (kind, travel, casts, the ray in flight) and is validated, never trusted: nothing is
 * indexed with a state word.  Records move as dwords.  No LDS, no cast.  The C entry points of the block are at the end of the file.
 */
#include "rt_api_internal.h"
#include "rt_cast.h"
#include "rt_hit_abi.h"
#include "rt_refract_entry.h"

namespace rt {

#define RT_REFR_THREADS 256u
#define RT_REFR_MAX_RETRY 10u /* main.rs:378 */

__device__ __forceinline__ void store_no_ray(rt_ray *__restrict__ out) {
    store_ray(out, v3(0.0f, 0.0f, 0.0f), v3(0.0f, 0.0f, 0.0f), 0u, 0u, 0u, 0u, 0u);
}

/* main.rs:354-368 */
__global__ __launch_bounds__(RT_REFR_THREADS) void refract_enter_kernel(const KernelScene sc, const rt_hit *__restrict__ hits,
                                                                        const rt_ray *__restrict__ incoming, const uint64_t n,
                                                                        rt_ray *__restrict__ rays, uint32_t *__restrict__ kind,
                                                                        float *__restrict__ travel, uint32_t *__restrict__ casts,
                                                                        unsigned char *__restrict__ flags) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_REFR_THREADS + threadIdx.x;
    if (i >= n) return;
    const AbiHit h = hit_from_abi(hits + i, sc.n_triangles, sc.n_spheres, sc.n_materials, true);
    V3 in_dir = v3(0.0f, 0.0f, 0.0f);
    float k = 1.0f;
    if (h.valid) {
        in_dir = ray_from_abi(incoming + i, sc.n_triangles, sc.n_spheres).d; /* hit.ray.direction */
        k = material_approx(sc.materials[h.g.obj], h.g.u, h.g.v).refraction_index; /* main.rs:354 */
    }
    rt_ray inside; /* Trapped at entry (main.rs:356-358), or ray_inside (main.rs:360-368): rt_refract_entry.h */
    const uint32_t result = refract_enter_record(h.valid, h.g.pos, h.g.normal, in_dir, k, h.kind, h.index, &inside);
    store_ray_record(rays + i, inside);
    kind[i] = result;
    travel[i] = 0.0f;
    casts[i] = 0u;
    flags[i] = result == RT_REFR_WALKING ? 1 : 0;
}

/* main.rs:371-402 for one answered cast */
__global__ __launch_bounds__(RT_REFR_THREADS) void refract_step_kernel(const KernelScene sc, const rt_hit *__restrict__ hits, const uint64_t n,
                                                                       const float max_distance, const rt_hit *__restrict__ inside_hits,
                                                                       rt_ray *__restrict__ rays, uint32_t *__restrict__ kind,
                                                                       float *__restrict__ travel, uint32_t *__restrict__ casts,
                                                                       unsigned char *__restrict__ flags, rt_ray *__restrict__ escape) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_REFR_THREADS + threadIdx.x;
    if (i >= n) return;
    if (kind[i] != RT_REFR_WALKING) { /* finished, whatever the word says: nothing was cast for it */
        flags[i] = 0;
        return;
    }
    const uint32_t j = casts[i]; /* the casts answered before this one: `retry` of main.rs:377 */
    casts[i] = j + 1u;
    const AbiHit ih = hit_from_abi(inside_hits + i, sc.n_triangles, sc.n_spheres, 0u, false); /* hit_inside */
    uint32_t result = 2u; /* Trapped */
    if (!ih.valid) {
        result = 1u; /* Infinite, main.rs:373, 383: rays[i] stays — it is the ray of Refraction::Infinite */
    } else {
        const AbiHit h = hit_from_abi(hits + i, sc.n_triangles, sc.n_spheres, sc.n_materials, true);
        float k = 1.0f;
        if (h.valid) k = material_approx(sc.materials[h.g.obj], h.g.u, h.g.v).refraction_index; /* main.rs:354 */
        const Ray req = ray_from_abi(rays + i, sc.n_triangles, sc.n_spheres); /* hit_inside.ray */
        float t;
        if (j == 0u) t = distance(ih.g.pos, h.g.pos); /* main.rs:375 */
        else t = travel[i] + distance(req.o, ih.g.pos); /* main.rs:385: previous_hit_position is the bounce ray's origin */
        travel[i] = t;
        V3 out_dir;
        const bool have_out = refract_dir(ih.g.normal, req.d, 1.0f / k, &out_dir);
        if (!have_out && t <= max_distance && j < RT_REFR_MAX_RETRY) { /* main.rs:378, in its order; get_reflect(&hit_inside) */
            store_ray(rays + i, ih.g.pos, reflect_dir(ih.g.normal, req.d), FACE_BACK, 1u, ih.kind, ih.index, ih.g.bf ? FACE_FRONT : FACE_BACK);
            flags[i] = 1;
            return; /* still walking */
        }
        if (have_out) { /* main.rs:392-402 */
            result = 0u;
            store_ray(escape + i, ih.g.pos, normalize(out_dir), FACE_FRONT, 1u, ih.kind, ih.index, FACE_BACK);
        }
    }
    if (result != 0u) store_no_ray(escape + i);
    kind[i] = result;
    flags[i] = 0;
}

} /* namespace rt */

/* ---- the C entry points (include/rt_amd.h "refraction queries") ---- */

extern "C" {

int rt_refract_enter(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, rt_ray *d_rays, uint32_t *d_kind,
                     float *d_travel, uint32_t *d_casts, unsigned char *d_flags, void *hip_stream) {
    bool done;
    const int rc = query_args("rt_refract_enter", n, RECORDS_2_32, true, scene, d_hits && d_incoming && d_rays && d_kind && d_travel && d_casts && d_flags,
                                "hit, incoming-ray, ray, kind, travel, cast-count or flag", &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::refract_enter_kernel, grid_of(n, RT_REFR_THREADS), dim3(RT_REFR_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks,
                       d_hits, d_incoming, (uint64_t)n, d_rays, d_kind, d_travel, d_casts, d_flags);
    return launched("rt_refract_enter");
}

int rt_refract_step(const rt_scene *scene, const rt_hit *d_hits, size_t n, float max_distance, const rt_hit *d_inside_hits, rt_ray *d_rays,
                    uint32_t *d_kind, float *d_travel, uint32_t *d_casts, unsigned char *d_flags, rt_ray *d_escape, void *hip_stream) {
    bool done;
    const int rc = query_args("rt_refract_step", n, RECORDS_2_32, true, scene, d_hits && d_inside_hits && d_rays && d_kind && d_travel && d_casts && d_flags && d_escape,
                                "hit, inside-hit, ray, kind, travel, cast-count, flag or escape-ray", &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::refract_step_kernel, grid_of(n, RT_REFR_THREADS), dim3(RT_REFR_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks,
                       d_hits, (uint64_t)n, max_distance, d_inside_hits, d_rays, d_kind, d_travel, d_casts, d_flags, d_escape);
    return launched("rt_refract_step");
}

} /* extern "C" */
