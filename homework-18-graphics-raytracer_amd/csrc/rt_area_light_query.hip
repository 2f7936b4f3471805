/*
 * rt_area_light_query.hip — the light queries (rt_light_query.hip) on lights that have a size (include/rt_amd.h "area-light
 * queries"): per (sample, light, record) a point on the light's sphere, the shadow ray and the Phong terms of the light displaced to
 * that point, and the fold that averages a light's samples before it weights and sums the lights.
 *
 *   rt::area_rays_kernel    light_rays_kernel's body on the displaced light, and the sample it was displaced to
 *   rt::area_terms_kernel   light_terms_kernel's body on the light displaced to the caller's sample
 *   rt::area_fold_kernel    per record and light the mean over the samples, then light_fold_kernel's sum
 *
 * Nothing here is new arithmetic but the sampler (rt_area_light.h, shared with librt_host.so) and the mean: the record, the shadow
 * ray and the light-term body are the light queries' own (rt_light_record.h: light_record, store_shadow_ray, light_terms), and
 * light_asks is called as light_rays_kernel calls it — all on a register copy of the light whose origin (or direction) is the sample.
 * With radius 0 that copy holds the stored words, so every bit is rt_light_rays' / rt_light_terms', and with one sample the mean
 * divides by 1.  One record per lane, the record
 * number counted in 64 bits; the material and the bump normal once per record; the sample and light loops are wave-uniform (the light
 * and its radius come through uniform_ref: scalar loads); arrays are sample-major, then light-major, entry
 * (s * light_count + (l - light_first)) * n + i, so that the stores of one (sample, light) plane are coalesced.  Records move as
 * dwords.  No LDS, no cast.  The C entry points of the block are at the end of the file.
 */
#include "rt_api_internal.h"
#include "rt_area_light.h"
#include "rt_light_record.h"

namespace rt {

__global__ __launch_bounds__(RT_LIGHT_THREADS) void area_rays_kernel(const KernelScene sc, const rt_hit *__restrict__ hits, const uint64_t n,
                                                                     const uint32_t light_first, const uint32_t light_count,
                                                                     const float *__restrict__ radii, const uint32_t *__restrict__ ids,
                                                                     const uint32_t spp, const uint32_t pattern, const uint32_t strata,
                                                                     const uint32_t seed, rt_ray *__restrict__ shadow_rays,
                                                                     unsigned char *__restrict__ asks, float *__restrict__ sample_out) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_LIGHT_THREADS + threadIdx.x;
    if (i >= n) return;
    const LightRecord r = light_record(sc, hits, i);
    const V3 pos = r.h.g.pos;
    const uint32_t id = record_id(ids, i);
    for (uint32_t s = 0; s < spp; ++s)                 /* wave-uniform */
        for (uint32_t l = 0; l < light_count; ++l) {   /* wave-uniform */
            const auto &L = uniform_ref(sc.lights + (light_first + l));
            const float rad = uniform_ref(radii + l);
            const uint64_t k = ((uint64_t)s * light_count + l) * n + i;
            const V3 sample = area_light_sample(L, light_first + l, rad, pattern, strata, id, seed, s);
            store_v3(sample_out, k, sample);
            const rt_light D = area_light_displaced(L, sample);
            V3 l_direction = v3(0.0f, 0.0f, 0.0f);
            const bool need = light_asks(D, uniform_ref(sc.light_aux + (light_first + l)), pos, r.adj_n, &l_direction) && r.valid;
            asks[k] = need ? 1 : 0;
            store_shadow_ray(shadow_rays + k, r, -l_direction, need); /* towards the sample */
        }
}

__global__ __launch_bounds__(RT_LIGHT_THREADS) void area_terms_kernel(const KernelScene sc, const rt_hit *__restrict__ hits,
                                                                      const rt_ray *__restrict__ incoming, const uint64_t n,
                                                                      const uint32_t light_first, const uint32_t light_count, const uint32_t spp,
                                                                      const unsigned char *__restrict__ asks, const float *__restrict__ sample_in,
                                                                      const rt_hit *__restrict__ shadow_hits, unsigned char *__restrict__ lit_out,
                                                                      float *__restrict__ diffuse_out, float *__restrict__ specular_out) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_LIGHT_THREADS + threadIdx.x;
    if (i >= n) return;
    const LightRecord r = light_record(sc, hits, i);
    const V3 pos = r.h.g.pos;
    V3 view = v3(0.0f, 0.0f, 1.0f);
    if (r.valid) view = ray_from_abi(incoming + i, sc.n_triangles, sc.n_spheres).d; /* hit.ray.direction */
    for (uint32_t s = 0; s < spp; ++s)                 /* wave-uniform */
        for (uint32_t l = 0; l < light_count; ++l) {   /* wave-uniform */
            const uint64_t k = ((uint64_t)s * light_count + l) * n + i;
            const bool asked = r.valid && asks[k] != 0;
            LightTerms t; /* not lit, +0 */
            if (__builtin_amdgcn_ballot_w64(asked) != 0ull) { /* a wave nobody asks in skips the pair: its acosf and powf are binary64 */
                const auto &L = uniform_ref(sc.lights + (light_first + l));
                if (asked) { /* the sample is read where asked alone; the occluder's distance is measured to the displaced origin */
                    const rt_light D = area_light_displaced(L, load_v3(sample_in, k));
                    t = light_terms(D, area_light_has_origin(L), v3(D.origin[0], D.origin[1], D.origin[2]), pos, r.m, r.adj_n, view, true, shadow_hits + k);
                }
            }
            store_light_terms(lit_out, diffuse_out, specular_out, k, t);
        }
}

/* per light: acc = the first lit sample's term, each later lit term added in ascending s; D = acc_d / spp, S = acc_s / spp; then
 * light_fold_kernel's association, (sum + D * (1 - shiness)) + S * shiness */
__global__ __launch_bounds__(RT_LIGHT_THREADS) void area_fold_kernel(const KernelScene sc, const rt_hit *__restrict__ hits, const uint64_t n,
                                                                     const uint32_t light_count, const uint32_t spp,
                                                                     const unsigned char *__restrict__ lit, const float *__restrict__ diffuse,
                                                                     const float *__restrict__ specular, float *__restrict__ rgb,
                                                                     float *__restrict__ visibility) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_LIGHT_THREADS + threadIdx.x;
    if (i >= n) return;
    bool valid;
    const float shiness = fold_shiness(sc, hits, i, &valid);
    if (!valid) { /* "no hit": rgb not written, visibility 0 */
        if (visibility != nullptr)
            for (uint32_t l = 0; l < light_count; ++l) visibility[(uint64_t)l * n + i] = 0.0f;
        return;
    }
    const float samples = (float)spp;
    V3 sum = load_v3(rgb, i);
    for (uint32_t l = 0; l < light_count; ++l) {
        V3 acc_d = v3(0.0f, 0.0f, 0.0f), acc_s = v3(0.0f, 0.0f, 0.0f);
        uint32_t lit_count = 0u;
        for (uint32_t s = 0; s < spp; ++s) {
            const uint64_t k = ((uint64_t)s * light_count + l) * n + i;
            if (lit[k] == 0) continue;
            const V3 d = load_v3(diffuse, k), sp = load_v3(specular, k);
            acc_d = lit_count == 0u ? d : acc_d + d;
            acc_s = lit_count == 0u ? sp : acc_s + sp;
            ++lit_count;
        }
        if (visibility != nullptr) visibility[(uint64_t)l * n + i] = (float)lit_count / samples;
        if (lit_count == 0u) continue;
        sum = sum + (acc_d / samples) * (1.0f - shiness) + (acc_s / samples) * shiness;
    }
    store_v3(rgb, i, sum);
}

} /* namespace rt */

/* ---- the C entry points (include/rt_amd.h "area-light queries") ---- */

/* the checks before any device work are hit_sample_args' (rt_api_internal.h): the light queries' with the sample count.  Only
 * rt_area_light_rays takes a pattern, and rt_area_light_fold no range of lights */
extern "C" {

int rt_area_light_rays(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, uint32_t light_first, uint32_t light_count,
                       const float *d_radii, const uint32_t *d_ids, uint32_t spp, uint32_t pattern, uint32_t seed, rt_ray *d_shadow_rays,
                       unsigned char *d_asks, float *d_sample, void *hip_stream) {
    bool done;
    const int rc = hit_sample_args("rt_area_light_rays", scene,
                                   HitSampleArgs(n, d_hits && d_incoming && d_radii && d_shadow_rays && d_asks && d_sample,
                                                 "hit, incoming-ray, radius, shadow-ray, flag or sample")
                                       .lights(light_count, light_first).samples(spp).limits(rt::area_light_limits(spp, true, pattern)), &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::area_rays_kernel, grid_of(n, RT_LIGHT_THREADS), dim3(RT_LIGHT_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks, d_hits,
                       (uint64_t)n, light_first, light_count, d_radii, d_ids, spp, pattern, rt::film_strata(spp), seed, d_shadow_rays, d_asks, d_sample);
    return launched("rt_area_light_rays");
}

int rt_area_light_terms(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, uint32_t light_first, uint32_t light_count,
                        uint32_t spp, const unsigned char *d_asks, const float *d_sample, const rt_hit *d_shadow_hits, unsigned char *d_lit,
                        float *d_diffuse, float *d_specular, void *hip_stream) {
    bool done;
    const int rc = hit_sample_args("rt_area_light_terms", scene,
                                   HitSampleArgs(n, d_hits && d_incoming && d_asks && d_sample && d_shadow_hits && d_lit && d_diffuse && d_specular,
                                                 "hit, incoming-ray, flag, sample, shadow-hit, lit, diffuse or specular")
                                       .lights(light_count, light_first).samples(spp).limits(rt::area_light_limits(spp, false, 0u)), &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::area_terms_kernel, grid_of(n, RT_LIGHT_THREADS), dim3(RT_LIGHT_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks, d_hits,
                       d_incoming, (uint64_t)n, light_first, light_count, spp, d_asks, d_sample, d_shadow_hits, d_lit, d_diffuse, d_specular);
    return launched("rt_area_light_terms");
}

int rt_area_light_fold(const rt_scene *scene, const rt_hit *d_hits, size_t n, uint32_t light_count, uint32_t spp, const unsigned char *d_lit,
                       const float *d_diffuse, const float *d_specular, float *d_rgb, float *d_visibility, void *hip_stream) {
    bool done;
    const int rc = hit_sample_args("rt_area_light_fold", scene,
                                   HitSampleArgs(n, d_hits && d_lit && d_diffuse && d_specular && d_rgb, "hit, lit, diffuse, specular or rgb")
                                       .lights(light_count).samples(spp).limits(rt::area_light_limits(spp, false, 0u)), &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::area_fold_kernel, grid_of(n, RT_LIGHT_THREADS), dim3(RT_LIGHT_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks, d_hits,
                       (uint64_t)n, light_count, spp, d_lit, d_diffuse, d_specular, d_rgb, d_visibility);
    return launched("rt_area_light_fold");
}

} /* extern "C" */
