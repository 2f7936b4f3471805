/*
 * rt_transmit_query.hip — paths that pass through glass (include/rt_amd.h "transmission queries"): the two steps a path tracer written
 * from the public calls could not supply around the refraction queries' walk.
 *
 *   rt::path_branch_kernel    per listed path: the choice between the vertex's lobes and the glass from the counter hash, and for a
 *                             path that transmits rt_refract_enter's state of a walk that has cast nothing
 *   rt::path_transmit_kernel  per listed path: a finished walk folded into the record — decay, roulette, the escape ray as the next
 *                             ray — or the path's end
 *
 * The arithmetic is rt_transmit.h's, shared with librt_host.so: the entry is rt_refract_entry.h's body, which refract_enter_kernel
 * calls too, the tail rt_path.h's path_step_tail, which path_advance_record calls too.  The launch shape, the listed slot, the record's
 * codec and the "no hit" preset are rt_path_kernel.h's: one listed path per lane, the path record as 16-byte accesses (the branch reads
 * and writes its second half alone: it needs no throughput), hits, rays and state as dwords.  The walk's state words are the
 * caller's: they are compared, never indexed with.  No LDS, no cast, no workspace, no atomics.  The C entry points of the block are at
 * the end of the file.
 */
#include "rt_api_internal.h"
#include "rt_path_kernel.h"
#include "rt_transmit.h"

namespace rt {

#define RT_TRANSMIT_RAY_WORDS 11u
static_assert(sizeof(rt_ray) == RT_TRANSMIT_RAY_WORDS * sizeof(uint32_t), "rt_ray is 11 dwords");

/* hits is read and, for a path `last` ends, written: not restrict, not const */
__global__ __launch_bounds__(RT_PATH_THREADS) void path_branch_kernel(const KernelScene sc, rt_path *__restrict__ paths, const uint32_t m,
                                                                          const uint32_t *__restrict__ index, const uint32_t *__restrict__ count, rt_hit *hits,
                                                                          const rt_ray *__restrict__ incoming, const uint32_t seed, const bool last,
                                                                          unsigned char *__restrict__ lobe, unsigned char *__restrict__ transmit,
                                                                          rt_ray *__restrict__ walk_rays, uint32_t *__restrict__ kind, float *__restrict__ travel,
                                                                          uint32_t *__restrict__ casts, unsigned char *__restrict__ walk_flags) {
    const uint32_t j = path_slot(index, count, m);
    if (j >= m) return;
    PathTail t = load_path_tail(paths, j);
    bool transmits = false, lobes = false; /* a slot that is not alive: neither */
    uint32_t result = RT_HIT_NONE; /* a slot that does not walk: the state of a finished walk */
    rt_ray inside = no_ray_record();
    if ((t.flags & RT_PATH_ALIVE) != 0u) {
        const AbiHit h = hit_from_abi(hits + j, sc.n_triangles, sc.n_spheres, sc.n_materials, true);
        float transparency = 0.0f, k = 1.0f;
        if (h.valid) {
            const Mat mat = material_approx(sc.materials[h.g.obj], h.g.u, h.g.v);
            transparency = mat.transparency;
            k = mat.refraction_index; /* main.rs:354 */
        }
        transmits = path_transmits(t.id, t.bounce, seed, h.valid, transparency);
        if (transmits && last) { /* the path ends here: flags 0, nothing walked, the vertex "no hit" */
            t.flags = 0u;
            store_path_tail(paths, j, t);
            store_no_hit(hits + j);
            transmits = false;
        } else if (transmits) {
            const V3 in_dir = ray_from_abi(incoming + j, sc.n_triangles, sc.n_spheres).d; /* hit.ray.direction */
            result = refract_enter_record(true, h.g.pos, h.g.normal, in_dir, k, h.kind, h.index, &inside);
        } else {
            lobes = true;
        }
    }
    lobe[j] = lobes ? 1 : 0;
    transmit[j] = transmits ? 1 : 0;
    store_ray_record(walk_rays + j, inside);
    kind[j] = result;
    travel[j] = 0.0f;
    casts[j] = 0u;
    walk_flags[j] = result == RT_REFR_WALKING ? 1 : 0;
}

/* hits is read (the vertex's material) and, for a path that ends, written: not restrict, not const */
__global__ __launch_bounds__(RT_PATH_THREADS) void path_transmit_kernel(const KernelScene sc, rt_path *__restrict__ paths, const uint32_t m,
                                                                            const uint32_t *__restrict__ index, const uint32_t *__restrict__ count, rt_hit *hits,
                                                                            uint32_t *__restrict__ kind, const float *__restrict__ travel,
                                                                            const rt_ray *__restrict__ escape, const PathStep step,
                                                                            rt_ray *__restrict__ next_rays, unsigned char *__restrict__ alive,
                                                                            unsigned char *__restrict__ walk_flags) {
    const uint32_t j = path_slot(index, count, m);
    if (j >= m) return;
    const uint32_t walk = kind[j];
    kind[j] = RT_HIT_NONE; /* stale walk state never walks in a later bounce */
    walk_flags[j] = 0;
    rt_path p = load_path(paths, j);
    if ((p.flags & RT_PATH_ALIVE) == 0u) return;

    const AbiHit h = hit_from_abi(hits + j, sc.n_triangles, sc.n_spheres, sc.n_materials, true);
    float opaque_decay = 0.0f;
    if (h.valid) opaque_decay = material_approx(sc.materials[h.g.obj], h.g.u, h.g.v).opaque_decay;
    const bool lives = path_transmit_record(p, walk, h.valid, opaque_decay, travel[j], step);

    store_path(paths, j, p);
    alive[j] = lives ? 1 : 0;
    const uint32_t *const from = reinterpret_cast<const uint32_t *>(escape + j);
    uint32_t *const to = reinterpret_cast<uint32_t *>(next_rays + j);
#pragma unroll
    for (uint32_t k = 0; k < RT_TRANSMIT_RAY_WORDS; ++k) to[k] = lives ? from[k] : 0u;
    if (!lives) store_no_hit(hits + j);
}

} /* namespace rt */

/* ---- the C entry points (include/rt_amd.h "transmission queries") ---- */

extern "C" {

/* rt_path_advance's checks (listed_path_args, rt_api_internal.h) on the m slots, the record's alignment last */
int rt_path_branch(const rt_scene *scene, rt_path *d_paths, size_t m, const uint32_t *d_index, const uint32_t *d_count, rt_hit *d_hits,
                   const rt_ray *d_incoming, uint32_t seed, int last, unsigned char *d_lobe, unsigned char *d_transmit, rt_ray *d_walk_rays, uint32_t *d_kind,
                   float *d_travel, uint32_t *d_casts, unsigned char *d_walk_flags, void *hip_stream) {
    const char *const who = "rt_path_branch";
    bool done;
    const int rc = listed_path_args(who, scene, d_paths, d_index, d_count,
                                    HitSampleArgs(m, d_hits && d_incoming && d_lobe && d_transmit && d_walk_rays && d_kind && d_travel && d_casts && d_walk_flags,
                                                  "path, count (with an index), hit, incoming-ray, lobe, transmit, walk-ray, kind, travel, cast-count or walk-flag"),
                                    &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::path_branch_kernel, grid_of(m, RT_PATH_THREADS), dim3(RT_PATH_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks,
                       d_paths, (uint32_t)m, d_index, d_count, d_hits, d_incoming, seed, last != 0, d_lobe, d_transmit, d_walk_rays, d_kind, d_travel, d_casts,
                       d_walk_flags);
    return launched(who);
}

/* the same, then rr_floor (rt::path_limits), then the record's alignment */
int rt_path_transmit(const rt_scene *scene, rt_path *d_paths, size_t m, const uint32_t *d_index, const uint32_t *d_count, rt_hit *d_hits, uint32_t *d_kind,
                     const float *d_travel, const rt_ray *d_escape, uint32_t seed, uint32_t rr_start, float rr_floor, rt_ray *d_next_rays,
                     unsigned char *d_alive, unsigned char *d_walk_flags, void *hip_stream) {
    const char *const who = "rt_path_transmit";
    bool done;
    const int rc = listed_path_args(who, scene, d_paths, d_index, d_count,
                                    HitSampleArgs(m, d_hits && d_kind && d_travel && d_escape && d_next_rays && d_alive && d_walk_flags,
                                                  "path, count (with an index), hit, kind, travel, escape-ray, ray, flag or walk-flag")
                                        .limits(rt::path_limits(RT_HEMISPHERE_SHADING, rr_floor)), &done);
    if (rc != RT_OK || done) return rc;
    const rt::PathStep step = {seed, rr_start, rr_floor, false};
    hipLaunchKernelGGL(rt::path_transmit_kernel, grid_of(m, RT_PATH_THREADS), dim3(RT_PATH_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks,
                       d_paths, (uint32_t)m, d_index, d_count, d_hits, d_kind, d_travel, d_escape, step, d_next_rays, d_alive, d_walk_flags);
    return launched(who);
}

} /* extern "C" */
