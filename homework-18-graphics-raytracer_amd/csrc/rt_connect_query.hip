/*
 * rt_connect_query.hip — next-event estimation of the sky inside the path loop (include/rt_amd.h "connection queries"): the three steps
 * a path tracer written from the public calls could not supply around rt_path_advance.
 *
 *   rt::path_connect_kernel        per listed path: one direction from the environment's table drawn from the path's own hash streams,
 *                                  its weight against the vertex's lobes, the throughput and the Phong terms multiplied in — what the
 *                                  path gains if the shadow ray written beside it finds nothing
 *   rt::path_settle_kernel         per listed slot: the shadow cast's answer — radiance += pending where it is open — and the flag cleared
 *   rt::path_weigh_escape_kernel   per listed path that left the scene along a lobe-sampled ray: the sky it found times the weight of
 *                                  the lobe's density, kept in the record, against the table's
 *
 * The arithmetic is rt_connect.h's, shared with librt_host.so, and that header calls rt_environment.h's sampler, rt_lobe.h's densities
 * and weight and rt_shade.h's terms as environment_rays_kernel, lobe_pdf_kernel, environment_pdf_kernel, mis_weigh_kernel and
 * probe_surfaces_kernel call them: the record, the sampling normal and the shadow ray are rt_light_record.h's.  The launch shape,
 * the listed slot, the record's codec and the view direction are rt_path_kernel.h's: one listed path per lane; the path record is
 * read as two 16-byte accesses and never written, the hit, the rays and the planes move as dwords.  The table is read by binary
 * search inside the bounds the descriptor's size gives, whatever it holds.  No LDS, no cast, no workspace, no atomics.  The C entry
 * points of the block are at the end of the file.
 */
#include "rt_api_internal.h"
#include "rt_connect.h"
#include "rt_path_kernel.h"

namespace rt {

__global__ __launch_bounds__(RT_PATH_THREADS) void path_connect_kernel(const KernelScene sc, const rt_environment e, const void *__restrict__ table,
                                                                          const rt_path *__restrict__ paths, const uint32_t m,
                                                                          const uint32_t *__restrict__ index, const uint32_t *__restrict__ count,
                                                                          const rt_hit *__restrict__ hits, const rt_ray *__restrict__ incoming,
                                                                          const PathConnect step, const uint32_t normal_kind,
                                                                          rt_ray *__restrict__ shadow_rays, unsigned char *__restrict__ asks,
                                                                          float *__restrict__ pending) {
    const uint32_t j = path_slot(index, count, m);
    if (j >= m) return;
    const rt_path p = load_path(paths, j);
    if ((p.flags & RT_PATH_ALIVE) == 0u) return;

    const LightRecord r = light_record(sc, hits, j);
    const Connection c = path_connect_record(p, r.valid, r.m, r.adj_n, sampling_normal(r, normal_kind), view_of(r.valid, incoming, j), e,
                                             env_table_view(e, table), step);

    asks[j] = c.ask ? 1 : 0;
    store_shadow_ray(shadow_rays + j, r, c.dir, c.ask);
    if (c.ask) store_v3(pending, j, c.pending);
}

__global__ __launch_bounds__(RT_PATH_THREADS) void path_settle_kernel(const uint32_t m, const uint32_t *__restrict__ index, const uint32_t *__restrict__ count,
                                                                         unsigned char *__restrict__ asks, const rt_hit *__restrict__ shadow_hits,
                                                                         const float *__restrict__ pending, float *__restrict__ radiance) {
    const uint32_t j = path_slot(index, count, m);
    if (j >= m) return;
    path_settle_record(j, asks, reinterpret_cast<const uint32_t *>(shadow_hits), pending, radiance);
}

__global__ __launch_bounds__(RT_PATH_THREADS) void path_weigh_escape_kernel(const rt_environment e, const void *__restrict__ table,
                                                                               const rt_path *__restrict__ paths, const uint32_t m,
                                                                               const uint32_t *__restrict__ index, const uint32_t *__restrict__ count,
                                                                               const rt_hit *__restrict__ hits, const rt_ray *__restrict__ incoming,
                                                                               const uint32_t heuristic, float *__restrict__ emitted) {
    const uint32_t j = path_slot(index, count, m);
    if (j >= m) return;
    const rt_path p = load_path(paths, j);
    const EnvTable t = env_table_view(e, table);
    if (!path_escape_weighed(p.flags, reinterpret_cast<const uint32_t *>(hits + j)[0], p.pdf, t)) return;
    const float w = path_escape_weight(e, t, heuristic, p.pdf, ray_direction(incoming, j));
    store_v3(emitted, j, load_v3(emitted, j) * w);
}

} /* namespace rt */

/* ---- the C entry points (include/rt_amd.h "connection queries") ---- */

/* the descriptor's checks under the entry point's name */
static int environment_ok(const char *who, const rt_environment *env) { return check_descriptor(who, env, rt::environment_limits); }

/* what follows listed_path_args in the two calls that read the table */
static int table_ok(const char *who, const void *d_table) {
    if (!aligned_8(d_table)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": the table is not 8-byte aligned");
    return RT_OK;
}

extern "C" {

/* rt_path_advance's checks (listed_path_args, rt_api_internal.h) on the m slots, with the descriptor after the scene as in
 * rt_environment_rays; then the normal_kind, then the heuristic, then the alignment of the record and of the table */
int rt_path_connect(const rt_scene *scene, const rt_environment *env, const void *d_table, const rt_path *d_paths, size_t m, const uint32_t *d_index,
                    const uint32_t *d_count, const rt_hit *d_hits, const rt_ray *d_incoming, uint32_t seed, uint32_t normal_kind, uint32_t heuristic, int last,
                    rt_ray *d_shadow_rays, unsigned char *d_asks, float *d_pending, void *hip_stream) {
    const char *const who = "rt_path_connect";
    bool done;
    const int rc = listed_path_args(who, scene, d_paths, d_index, d_count,
                                    HitSampleArgs(m, d_table && d_hits && d_incoming && d_shadow_rays && d_asks && d_pending,
                                                  "table, path, count (with an index), hit, incoming-ray, ray, flag or pending")
                                        .described([env, who] { return environment_ok(who, env); }).limits(rt::connect_limits(normal_kind, heuristic)), &done);
    if (rc != RT_OK || done) return rc;
    if (const int bad = table_ok(who, d_table)) return bad;
    const rt::PathConnect step = {seed, heuristic, last != 0};
    hipLaunchKernelGGL(rt::path_connect_kernel, grid_of(m, RT_PATH_THREADS), dim3(RT_PATH_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks, *env,
                       d_table, d_paths, (uint32_t)m, d_index, d_count, d_hits, d_incoming, step, normal_kind, d_shadow_rays, d_asks, d_pending);
    return launched(who);
}

/* the count, the empty batch, the pointers (d_shadow_hits may be NULL: nothing occludes), the record's alignment; no scene, no descriptor */
int rt_path_settle(const rt_path *d_paths, size_t m, const uint32_t *d_index, const uint32_t *d_count, unsigned char *d_asks, const rt_hit *d_shadow_hits,
                   const float *d_pending, float *d_radiance, void *hip_stream) {
    const char *const who = "rt_path_settle";
    bool done;
    const int rc = listed_path_args(who, nullptr, d_paths, d_index, d_count,
                                    HitSampleArgs(m, d_asks && d_pending && d_radiance, "path, count (with an index), flag, pending or radiance").no_scene(), &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::path_settle_kernel, grid_of(m, RT_PATH_THREADS), dim3(RT_PATH_THREADS), 0, static_cast<hipStream_t>(hip_stream), (uint32_t)m,
                       d_index, d_count, d_asks, d_shadow_hits, d_pending, d_radiance);
    return launched(who);
}

/* the count, the descriptor, the empty batch, the pointers, the heuristic, the alignment of the record and of the table; no scene */
int rt_path_weigh_escape(const rt_environment *env, const void *d_table, const rt_path *d_paths, size_t m, const uint32_t *d_index, const uint32_t *d_count,
                         const rt_hit *d_hits, const rt_ray *d_incoming, uint32_t heuristic, float *d_emitted, void *hip_stream) {
    const char *const who = "rt_path_weigh_escape";
    bool done;
    const int rc = listed_path_args(who, nullptr, d_paths, d_index, d_count,
                                    HitSampleArgs(m, d_table && d_hits && d_incoming && d_emitted, "table, path, count (with an index), hit, incoming-ray or emitted")
                                        .no_scene().described([env, who] { return environment_ok(who, env); }).limits(rt::mis_limits(heuristic)), &done);
    if (rc != RT_OK || done) return rc;
    if (const int bad = table_ok(who, d_table)) return bad;
    hipLaunchKernelGGL(rt::path_weigh_escape_kernel, grid_of(m, RT_PATH_THREADS), dim3(RT_PATH_THREADS), 0, static_cast<hipStream_t>(hip_stream), *env,
                       d_table, d_paths, (uint32_t)m, d_index, d_count, d_hits, d_incoming, heuristic, d_emitted);
    return launched(who);
}

} /* extern "C" */
