/*
 * rt_light_connect_query.hip — next-event estimation of the scene's own lights inside the path loop (include/rt_amd.h "light-connection
 * queries"): one sampled light per path vertex in the place of rt_shade_hits' every light as a point.
 *
 *   rt::light_connect_kernel   per listed path: one light chosen and one point on its sphere drawn from the path's own hash streams,
 *                              the light's Phong terms times the throughput over the chance of the choice — what the path gains if
 *                              the shadow ray written beside it is not occluded — and how far that ray may go
 *   rt::light_settle_kernel    per listed slot: the shadow cast's answer by get_shade's rule — radiance += pending unless something
 *                              nearer than the light was hit — and the flag cleared
 *
 * The arithmetic is rt_light_connect.h's, shared with librt_host.so, and that header calls rt_area_light.h's sampler and rt_shade.h's
 * light_asks, approximate_into_directional, get_diffuse and get_specular as area_rays_kernel and light_terms call them; the record and
 * the shadow ray are rt_light_record.h's.  The launch shape, the listed slot, the record's codec and the view direction are
 * rt_path_kernel.h's: one listed path per lane; the path record is read as two 16-byte accesses and never written, the hit, the rays
 * and the planes move as dwords.  The light differs from lane to lane, so the light, its aux and its radius are read with vector
 * loads, not through uniform_ref; the weights are read in a loop every lane walks alike.  A spot light's acosf and powf and
 * get_specular's power stay behind branches a wave without such a lane skips.  No LDS, no cast, no workspace, no atomics.  The C entry
 * points of the block are at the end.
 */
#include "rt_api_internal.h"
#include "rt_light_connect.h"
#include "rt_path_kernel.h"

namespace rt {

__global__ __launch_bounds__(RT_PATH_THREADS) void light_connect_kernel(const KernelScene sc, const rt_path *__restrict__ paths, const uint32_t m,
                                                                                 const uint32_t *__restrict__ index, const uint32_t *__restrict__ count,
                                                                                 const rt_hit *__restrict__ hits, const rt_ray *__restrict__ incoming,
                                                                                 const LightConnect step, rt_ray *__restrict__ shadow_rays,
                                                                                 unsigned char *__restrict__ asks, float *__restrict__ pending,
                                                                                 float *__restrict__ reach, uint32_t *__restrict__ chosen) {
    const uint32_t j = path_slot(index, count, m);
    if (j >= m) return;
    const rt_path p = load_path(paths, j);
    if ((p.flags & RT_PATH_ALIVE) == 0u) return;

    const LightRecord r = light_record(sc, hits, j);
    const LightConnection c = light_connect_record(p, r.valid, r.m, r.adj_n, r.h.g.pos, view_of(r.valid, incoming, j), sc.lights, sc.light_aux, step);

    asks[j] = c.ask ? 1 : 0;
    store_shadow_ray(shadow_rays + j, r, c.dir, c.ask);
    if (chosen != nullptr) chosen[j] = c.chosen;
    if (c.ask) {
        store_v3(pending, j, c.pending);
        reach[j] = c.reach;
    }
}

__global__ __launch_bounds__(RT_PATH_THREADS) void light_settle_kernel(const uint32_t m, const uint32_t *__restrict__ index,
                                                                                const uint32_t *__restrict__ count, unsigned char *__restrict__ asks,
                                                                                const rt_ray *__restrict__ shadow_rays, const rt_hit *__restrict__ shadow_hits,
                                                                                const float *__restrict__ reach, const float *__restrict__ pending,
                                                                                float *__restrict__ radiance) {
    const uint32_t j = path_slot(index, count, m);
    if (j >= m) return;
    light_settle_record(j, asks, reinterpret_cast<const uint32_t *>(shadow_rays), reinterpret_cast<const uint32_t *>(shadow_hits), reach, pending, radiance);
}

} /* namespace rt */

/* ---- the C entry points (include/rt_amd.h "light-connection queries") ---- */

extern "C" {

/* rt_path_connect's checks (listed_path_args, rt_api_internal.h) on the m slots — no lights is an empty batch, as no slots is —, then
 * the alignment of the record, then the range of lights in rt_area_light_rays' words */
int rt_path_connect_lights(const rt_scene *scene, const rt_path *d_paths, size_t m, const uint32_t *d_index, const uint32_t *d_count, const rt_hit *d_hits,
                           const rt_ray *d_incoming, uint32_t light_first, uint32_t light_count, const float *d_radii, const float *d_weights, uint32_t seed,
                           rt_ray *d_shadow_rays, unsigned char *d_asks, float *d_pending, float *d_reach, uint32_t *d_chosen, void *hip_stream) {
    const char *const who = "rt_path_connect_lights";
    bool done;
    HitSampleArgs args(m, d_hits && d_incoming && d_shadow_rays && d_asks && d_pending && d_reach,
                       "path, count (with an index), hit, incoming-ray, ray, flag, pending or reach");
    args.per_record = light_count == 0u ? 0u : 1u; /* one light per record is drawn; none: nothing to do */
    const int rc = listed_path_args(who, scene, d_paths, d_index, d_count, args, &done);
    if (rc != RT_OK || done) return rc;
    if ((uint64_t)light_first + (uint64_t)light_count > (uint64_t)scene->ks.n_lights)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": lights " + std::to_string(light_first) + " .. " +
                                                 std::to_string((uint64_t)light_first + light_count) + " of a scene with " + std::to_string(scene->ks.n_lights));
    const rt::LightConnect step = {seed, light_first, light_count, d_radii, d_weights};
    hipLaunchKernelGGL(rt::light_connect_kernel, grid_of(m, RT_PATH_THREADS), dim3(RT_PATH_THREADS), 0, static_cast<hipStream_t>(hip_stream),
                       scene->ks, d_paths, (uint32_t)m, d_index, d_count, d_hits, d_incoming, step, d_shadow_rays, d_asks, d_pending, d_reach, d_chosen);
    return launched(who);
}

/* rt_path_settle's checks with the two operands more (d_shadow_hits may be NULL: nothing occludes); no scene */
int rt_path_settle_lights(const rt_path *d_paths, size_t m, const uint32_t *d_index, const uint32_t *d_count, unsigned char *d_asks,
                          const rt_ray *d_shadow_rays, const rt_hit *d_shadow_hits, const float *d_reach, const float *d_pending, float *d_radiance,
                          void *hip_stream) {
    const char *const who = "rt_path_settle_lights";
    bool done;
    const int rc = listed_path_args(who, nullptr, d_paths, d_index, d_count,
                                    HitSampleArgs(m, d_asks && d_shadow_rays && d_reach && d_pending && d_radiance,
                                                  "path, count (with an index), flag, ray, reach, pending or radiance").no_scene(), &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::light_settle_kernel, grid_of(m, RT_PATH_THREADS), dim3(RT_PATH_THREADS), 0, static_cast<hipStream_t>(hip_stream),
                       (uint32_t)m, d_index, d_count, d_asks, d_shadow_rays, d_shadow_hits, d_reach, d_pending, d_radiance);
    return launched(who);
}

} /* extern "C" */
