/*
 * rt_lobe_query.hip — a surface's own Phong lobes, sampled (include/rt_amd.h "lobe queries"): per (sample, record) a direction drawn
 * from the mixture of the diffuse and the specular lobe with its density and its shadow ray, the density of directions of the caller's
 * own under that mixture and under an environment's table, and the weight that combines two sampling strategies.
 *
 *   rt::lobe_rays_kernel         per (sample, record): the direction, the lobe it came from, the mixture density, the flag, the shadow ray
 *   rt::lobe_pdf_kernel          per (probe, record): the mixture density of a given direction on an rt_surface record
 *   rt::environment_pdf_kernel   per direction: the texel the lookup names and the table's density there
 *   rt::mis_weigh_kernel         per entry: the balance or power weight, and rgb times it (over the entry's own density)
 *
 * The arithmetic is rt_lobe.h's, shared with librt_host.so: the record, the sampling normal and the shadow ray are the hemisphere and
 * environment queries' own (rt_light_record.h), and hemisphere_dir and env_texel_point are called as those queries call them, so a
 * surface of shiness 0 gets rt_hemisphere_rays' words.  One record
 * (or entry) per lane, the number counted in 64 bits; the material, N, R and e once per record; the sample and probe loops are
 * wave-uniform; arrays are sample-major, entry s * n + i.  Records move as dwords.  No LDS, no cast, no workspace.  The C entry points
 * of the block are at the end of the file.
 */
#include "rt_api_internal.h"
#include "rt_light_record.h"
#include "rt_lobe.h"

namespace rt {

#define RT_LOBE_THREADS 256u
#define RT_LOBE_RAY_DIRECTION 3u /* word of rt_ray.direction */

__global__ __launch_bounds__(RT_LOBE_THREADS) void lobe_rays_kernel(const KernelScene sc, const rt_hit *__restrict__ hits, const rt_ray *__restrict__ incoming,
                                                                    const uint64_t n, const uint32_t *__restrict__ ids, const uint32_t spp,
                                                                    const uint32_t pattern, const uint32_t strata, const uint32_t seed,
                                                                    const uint32_t normal_kind, rt_ray *__restrict__ shadow_rays,
                                                                    unsigned char *__restrict__ asks, float *__restrict__ dirs, float *__restrict__ pdf,
                                                                    unsigned char *__restrict__ lobe) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_LOBE_THREADS + threadIdx.x;
    if (i >= n) return;
    const LightRecord r = light_record(sc, hits, i);
    const V3 normal = sampling_normal(r, normal_kind);
    V3 view = v3(0.0f, 0.0f, 1.0f);
    if (r.valid) {
        const float *const d = reinterpret_cast<const float *>(incoming + i) + RT_LOBE_RAY_DIRECTION;
        view = -v3(d[0], d[1], d[2]); /* what get_shade passes as view_direction */
    }
    const LobeSurface surface = lobe_surface(normal, view, r.m.shiness, r.m.smoothness);
    const uint32_t id = record_id(ids, i);
    const uint32_t seed_h = hemisphere_seed(seed);
    for (uint32_t s = 0; s < spp; ++s) { /* wave-uniform */
        const uint64_t k = (uint64_t)s * n + i;
        const LobeSample p = lobe_sample(surface, pattern, strata, id, seed_h, s, r.valid);
        store_v3(dirs, k, p.dir);
        pdf[k] = r.valid ? p.pdf : 0.0f;
        lobe[k] = p.specular ? 1 : 0;
        asks[k] = p.ok ? 1 : 0;
        store_shadow_ray(shadow_rays + k, r, p.dir, p.ok);
    }
}

__global__ __launch_bounds__(RT_LOBE_THREADS) void lobe_pdf_kernel(const rt_surface *__restrict__ surfaces, const uint64_t n, const float *__restrict__ view,
                                                                   const float *__restrict__ dirs, const uint32_t n_probes, float *__restrict__ pdf) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_LOBE_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t *const p = reinterpret_cast<const uint32_t *>(surfaces + i); /* six words of the record, not surface_record's eighteen */
    const bool valid = p[17] != 0u;
    const V3 normal = v3(__uint_as_float(p[14]), __uint_as_float(p[15]), __uint_as_float(p[16])); /* shading_normal */
    const LobeSurface surface = lobe_surface(normal, load_v3(view, i), __uint_as_float(p[6]), __uint_as_float(p[10]));
    for (uint32_t q = 0; q < n_probes; ++q) { /* wave-uniform */
        const uint64_t k = (uint64_t)q * n + i;
        const V3 dir = valid ? load_v3(dirs, k) : v3(0.0f, 0.0f, 0.0f);
        const float density = lobe_pdf(surface, dir, valid);
        pdf[k] = valid ? density : 0.0f;
    }
}

__global__ __launch_bounds__(RT_LOBE_THREADS) void environment_pdf_kernel(const rt_environment e, const void *__restrict__ table, const float *__restrict__ dirs,
                                                                          const uint64_t count, float *__restrict__ pdf, uint32_t *__restrict__ texel) {
    const uint64_t k = (uint64_t)blockIdx.x * RT_LOBE_THREADS + threadIdx.x;
    if (k >= count) return;
    const EnvTable t = env_table_view(e, table);
    uint32_t at;
    pdf[k] = env_pdf(e, t, v3p(dirs + k * 3u), &at);
    if (texel != nullptr) texel[k] = at;
}

__global__ __launch_bounds__(RT_LOBE_THREADS) void mis_weigh_kernel(const MisWeigh m) {
    const uint64_t k = (uint64_t)blockIdx.x * RT_LOBE_THREADS + threadIdx.x;
    if (k >= m.count) return;
    mis_weigh_entry(m, k);
}

} /* namespace rt */

/* ---- the C entry points (include/rt_amd.h "lobe queries") ---- */

extern "C" {

/* rt_hemisphere_rays' checks (hit_sample_args, rt_api_internal.h), with the incoming rays among the pointers */
int rt_lobe_rays(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, const uint32_t *d_ids, uint32_t spp, uint32_t pattern,
                 uint32_t seed, uint32_t normal_kind, rt_ray *d_rays, unsigned char *d_asks, float *d_dirs, float *d_pdf, unsigned char *d_lobe,
                 void *hip_stream) {
    const char *const who = "rt_lobe_rays";
    bool done;
    const int rc = hit_sample_args(who, scene,
                                   HitSampleArgs(n, d_hits && d_incoming && d_rays && d_asks && d_dirs && d_pdf && d_lobe,
                                                 "hit, incoming-ray, ray, flag, direction, pdf or lobe")
                                       .samples(spp).limits(rt::hemisphere_limits(spp, true, pattern, normal_kind)), &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::lobe_rays_kernel, grid_of(n, RT_LOBE_THREADS), dim3(RT_LOBE_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks, d_hits,
                       d_incoming, (uint64_t)n, d_ids, spp, pattern, rt::film_strata(spp), seed, normal_kind, d_rays, d_asks, d_dirs, d_pdf, d_lobe);
    return launched(who);
}

/* rt_probe_surfaces' checks, then the normal_kind */
int rt_lobe_pdf(const rt_surface *d_surfaces, size_t n, const float *d_view, const float *d_dirs, uint32_t n_probes, uint32_t normal_kind, float *d_pdf,
                void *hip_stream) {
    const char *const who = "rt_lobe_pdf";
    bool done;
    const int rc = hit_sample_args(who, nullptr,
                                   HitSampleArgs(n, d_surfaces && d_view && d_dirs && d_pdf, "surface, view, direction or pdf")
                                       .no_scene().probes(n_probes).limits(rt::lobe_pdf_limits(normal_kind)), &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::lobe_pdf_kernel, grid_of(n, RT_LOBE_THREADS), dim3(RT_LOBE_THREADS), 0, static_cast<hipStream_t>(hip_stream), d_surfaces, (uint64_t)n,
                       d_view, d_dirs, n_probes, d_pdf);
    return launched(who);
}

/* the environment queries' checks: the count, the descriptor, the empty batch, the pointers */
int rt_environment_pdf(const rt_environment *env, const void *d_table, const float *d_dirs, size_t count, float *d_pdf, uint32_t *d_texel, void *hip_stream) {
    const char *const who = "rt_environment_pdf";
    int rc = check_count(who, count, {32u, "directions", "query them in several calls"});
    if (rc != RT_OK) return rc;
    bool unsupported;
    if (const char *bad = rt::environment_limits(env, &unsupported))
        return fail(unsupported ? RT_ERR_UNSUPPORTED : RT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + bad);
    if (count == 0) return RT_OK;
    rc = check_pointers(who, d_table && d_dirs && d_pdf, "table, direction or pdf");
    if (rc != RT_OK) return rc;
    hipLaunchKernelGGL(rt::environment_pdf_kernel, grid_of(count, RT_LOBE_THREADS), dim3(RT_LOBE_THREADS), 0, static_cast<hipStream_t>(hip_stream), *env, d_table,
                       d_dirs, (uint64_t)count, d_pdf, d_texel);
    return launched(who);
}

int rt_mis_weigh(size_t count, const float *d_pdf_own, uint32_t n_own, const float *d_pdf_other, uint32_t n_other, uint32_t heuristic, int divide_by_own,
                 float *d_weight, float *d_rgb, void *hip_stream) {
    const char *const who = "rt_mis_weigh";
    int rc = check_count(who, count, {32u, "entries", "weigh them in several calls"});
    if (rc != RT_OK || count == 0) return rc;
    rc = check_pointers(who, d_pdf_own && (d_weight || d_rgb), "own-pdf, or weight and rgb (one of the two is given)");
    if (rc != RT_OK) return rc;
    if (const char *bad = rt::mis_limits(heuristic)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + bad);
    const rt::MisWeigh m = rt::mis_weigh_call((uint64_t)count, d_pdf_own, n_own, d_pdf_other, n_other, heuristic, divide_by_own != 0, d_weight, d_rgb);
    hipLaunchKernelGGL(rt::mis_weigh_kernel, grid_of(count, RT_LOBE_THREADS), dim3(RT_LOBE_THREADS), 0, static_cast<hipStream_t>(hip_stream), m);
    return launched(who);
}

} /* extern "C" */
