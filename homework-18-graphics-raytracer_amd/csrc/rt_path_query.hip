/*
 * rt_path_query.hip — the inner step of a path tracer on caller-supplied hits (include/rt_amd.h "path queries"): a record per path
 * that carries the throughput from bounce to bounce, one kernel that does between two casts what rt_material_hits, rt_lobe_rays,
 * rt_probe_surfaces, rt_mis_weigh and rt_environment_fold do in five, ends paths by Russian roulette on the device, and the mean of a
 * pixel's paths at the end.
 *
 *   rt::path_begin_kernel     per (sample, root): the record of a fresh path, and its radiance zeroed
 *   rt::path_advance_kernel   per listed path: deposit, escape, sample, terms, throughput, roulette; the next ray or the end
 *   rt::path_resolve_kernel   per root: the samples' radiance in ascending order, their mean added to the root's slot
 *
 * The arithmetic is rt_path.h's, shared with librt_host.so, and that header calls rt_lobe.h's sampler and rt_shade.h's terms as
 * lobe_rays_kernel and probe_surfaces_kernel call them: the record and the sampling normal are rt_light_record.h's.  The ray a survivor
 * goes on along is no shadow ray: it looks for the path's next vertex, the nearest surface whichever way it faces, so it is cast with
 * face Both and the vertex's own primitive excluded for both faces (store_continuation_ray); Back is an occlusion query's face.
 * The launch shape, the listed slot, the record's codec, the view direction and the "no hit" preset are rt_path_kernel.h's, shared with
 * the three other units of the path loop: one listed path (or root) per lane, the path record as two 16-byte accesses, the hit and the
 * rays as dwords.  No LDS, no cast, no workspace, no atomics.  The C entry points of the block are at the end of the file.
 */
#include "rt_api_internal.h"
#include "rt_path_kernel.h"

namespace rt {

__global__ __launch_bounds__(RT_PATH_THREADS) void path_begin_kernel(const uint64_t n, const uint32_t spp, const uint32_t *__restrict__ ids,
                                                                     rt_path *__restrict__ paths, float *__restrict__ radiance) {
    const uint64_t k = (uint64_t)blockIdx.x * RT_PATH_THREADS + threadIdx.x;
    if (k >= n * spp) return;
    const uint64_t i = k % n;
    store_path(paths, k, path_begin_record((uint32_t)i, record_id(ids, i), (uint32_t)(k / n)));
    store_v3(radiance, k, v3(0.0f, 0.0f, 0.0f));
}

/* the ray a path goes on along: rt_light_record.h's shadow ray — from the hit along `dir`, the hit's own primitive excluded — with its
 * two face words Both in the place of Back, or all-zero words for a path that ended */
__device__ __forceinline__ void store_continuation_ray(rt_ray *__restrict__ ray, const LightRecord &r, const V3 dir, const bool lives) {
    if (lives)
        store_ray(ray, r.h.g.pos, dir, FACE_BOTH, 1u, r.h.kind, r.h.index, FACE_BOTH);
    else
        store_ray(ray, v3(0.0f, 0.0f, 0.0f), v3(0.0f, 0.0f, 0.0f), 0u, 0u, 0u, 0u, 0u);
}

/* hits is read (the record's own slot) and, for a path that ends, written: not restrict, not const */
__global__ __launch_bounds__(RT_PATH_THREADS) void path_advance_kernel(const KernelScene sc, rt_path *__restrict__ paths, const uint32_t m,
                                                                       const uint32_t *__restrict__ index, const uint32_t *__restrict__ count, rt_hit *hits,
                                                                       const rt_ray *__restrict__ incoming, const float *__restrict__ emitted,
                                                                       const PathStep step, const uint32_t normal_kind, float *__restrict__ radiance,
                                                                       rt_ray *__restrict__ next_rays, unsigned char *__restrict__ alive) {
    const uint32_t j = path_slot(index, count, m);
    if (j >= m) return;
    rt_path p = load_path(paths, j);
    if ((p.flags & RT_PATH_ALIVE) == 0u) return;

    if (emitted != nullptr) {
        const V3 e = load_v3(emitted, j), l = load_v3(radiance, j);
        store_v3(radiance, j, v3(path_deposit(l.x, p.beta[0], e.x), path_deposit(l.y, p.beta[1], e.y), path_deposit(l.z, p.beta[2], e.z)));
    }

    const LightRecord r = light_record(sc, hits, j);
    V3 dir;
    const bool lives = path_advance_record(p, r.valid, r.m, r.adj_n, sampling_normal(r, normal_kind), view_of(r.valid, incoming, j), step, &dir);

    store_path(paths, j, p);
    alive[j] = lives ? 1 : 0;
    store_continuation_ray(next_rays + j, r, dir, lives);
    if (!lives) store_no_hit(hits + j);
}

__global__ __launch_bounds__(RT_PATH_THREADS) void path_resolve_kernel(const float *__restrict__ radiance, const uint64_t n, const uint32_t spp,
                                                                       const uint32_t *__restrict__ root, float *__restrict__ rgb) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_PATH_THREADS + threadIdx.x;
    if (i >= n) return;
    path_resolve_root(radiance, n, spp, i, root, rgb);
}

} /* namespace rt */

/* ---- the C entry points (include/rt_amd.h "path queries") ---- */

extern "C" {

int rt_path_begin(size_t n, uint32_t spp, const uint32_t *d_ids, rt_path *d_paths, float *d_radiance, void *hip_stream) {
    const char *const who = "rt_path_begin";
    bool done;
    const int rc = hit_sample_args(who, nullptr,
                                   HitSampleArgs(n, d_paths && d_radiance, "path or radiance").no_scene().samples(spp).limits(rt::hemisphere_limits(spp, false, 0u, 0u)),
                                   &done);
    if (rc != RT_OK || done) return rc;
    if (!aligned_16(d_paths)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": d_paths is not 16-byte aligned");
    hipLaunchKernelGGL(rt::path_begin_kernel, grid_of((uint64_t)n * spp, RT_PATH_THREADS), dim3(RT_PATH_THREADS), 0, static_cast<hipStream_t>(hip_stream),
                       (uint64_t)n, spp, d_ids, d_paths, d_radiance);
    return launched(who);
}

/* rt_lobe_rays' checks on the m slots, then rr_floor, then the record's alignment (listed_path_args, rt_api_internal.h) */
int rt_path_advance(const rt_scene *scene, rt_path *d_paths, size_t m, const uint32_t *d_index, const uint32_t *d_count, rt_hit *d_hits,
                    const rt_ray *d_incoming, const float *d_emitted, uint32_t seed, uint32_t normal_kind, uint32_t rr_start, float rr_floor, int last,
                    float *d_radiance, rt_ray *d_next_rays, unsigned char *d_alive, void *hip_stream) {
    const char *const who = "rt_path_advance";
    bool done;
    const int rc = listed_path_args(who, scene, d_paths, d_index, d_count,
                                    HitSampleArgs(m, d_hits && d_incoming && d_radiance && d_next_rays && d_alive,
                                                  "path, count (with an index), hit, incoming-ray, radiance, ray or flag")
                                        .limits(rt::path_limits(normal_kind, rr_floor)), &done);
    if (rc != RT_OK || done) return rc;
    const rt::PathStep step = {seed, rr_start, rr_floor, last != 0};
    hipLaunchKernelGGL(rt::path_advance_kernel, grid_of(m, RT_PATH_THREADS), dim3(RT_PATH_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks, d_paths,
                       (uint32_t)m, d_index, d_count, d_hits, d_incoming, d_emitted, step, normal_kind, d_radiance, d_next_rays, d_alive);
    return launched(who);
}

int rt_path_resolve(const float *d_radiance, size_t n, uint32_t spp, const uint32_t *d_root, float *d_rgb, void *hip_stream) {
    const char *const who = "rt_path_resolve";
    bool done;
    const int rc = hit_sample_args(who, nullptr,
                                   HitSampleArgs(n, d_radiance && d_rgb, "radiance or rgb").no_scene().samples(spp).limits(rt::hemisphere_limits(spp, false, 0u, 0u)),
                                   &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::path_resolve_kernel, grid_of(n, RT_PATH_THREADS), dim3(RT_PATH_THREADS), 0, static_cast<hipStream_t>(hip_stream), d_radiance, (uint64_t)n,
                       spp, d_root, d_rgb);
    return launched(who);
}

} /* extern "C" */
