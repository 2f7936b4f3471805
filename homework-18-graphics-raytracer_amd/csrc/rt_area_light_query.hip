/*
 * rt_area_light_query.hip — the light queries (rt_light_query.hip) on lights that have a size (include/rt_amd.h "area-light
 * queries"): per (sample, light, record) a point on the light's sphere, the shadow ray and the Phong terms of the light displaced to
 * that point, and the fold that averages a light's samples before it weights and sums the lights.
 *
 *   rt::area_rays_kernel    light_rays_kernel's body on the displaced light, and the sample it was displaced to
 *   rt::area_terms_kernel   light_terms_kernel's body on the light displaced to the caller's sample
 *   rt::area_fold_kernel    per record and light the mean over the samples, then light_fold_kernel's sum
 *
 * Nothing here is new arithmetic but the sampler (rt_area_light.h, shared with librt_host.so) and the mean: light_record, light_asks,
 * approximate_into_directional, get_diffuse and get_specular are called as the light queries call them, with the same operands in the
 * same order, on a register copy of the light whose origin (or direction) is the sample — with radius 0 that copy holds the stored
 * words, so every bit is rt_light_rays' / rt_light_terms', and with one sample the mean divides by 1.  One record per lane, the record
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
    const uint32_t id = ids != nullptr ? ids[i] : (uint32_t)i;
    for (uint32_t s = 0; s < spp; ++s)                 /* wave-uniform */
        for (uint32_t l = 0; l < light_count; ++l) {   /* wave-uniform */
            const auto &L = uniform_ref(sc.lights + (light_first + l));
            const float rad = uniform_ref(radii + l);
            const uint64_t k = ((uint64_t)s * light_count + l) * n + i;
            const V3 sample = area_light_sample(L, light_first + l, rad, pattern, strata, id, seed, s);
            sample_out[k * 3u] = sample.x;
            sample_out[k * 3u + 1u] = sample.y;
            sample_out[k * 3u + 2u] = sample.z;
            const rt_light D = area_light_displaced(L, sample);
            V3 l_direction = v3(0.0f, 0.0f, 0.0f);
            const bool need = light_asks(D, uniform_ref(sc.light_aux + (light_first + l)), pos, r.adj_n, &l_direction) && r.valid;
            asks[k] = need ? 1 : 0;
            if (need) /* light_rays_kernel's shadow ray, towards the sample */
                store_ray(shadow_rays + k, pos, -l_direction, FACE_BACK, 1u, r.h.kind, r.h.index, FACE_BACK);
            else
                store_ray(shadow_rays + k, v3(0.0f, 0.0f, 0.0f), v3(0.0f, 0.0f, 0.0f), 0u, 0u, 0u, 0u, 0u);
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
            bool lit = false;
            V3 diffuse = v3(0.0f, 0.0f, 0.0f), specular = v3(0.0f, 0.0f, 0.0f);
            if (__builtin_amdgcn_ballot_w64(asked) != 0ull) { /* a wave nobody asks in skips the pair: its acosf and powf are binary64 */
                const auto &L = uniform_ref(sc.lights + (light_first + l));
                if (asked) {
                    const rt_light D = area_light_displaced(L, v3(sample_in[k * 3u], sample_in[k * 3u + 1u], sample_in[k * 3u + 2u]));
                    lit = true;
                    const uint32_t *const occluder = reinterpret_cast<const uint32_t *>(shadow_hits + k);
                    if (occluder[0] <= 1u) { /* main.rs:435-448: Some(occlusion), the distance measured to the displaced origin */
                        if (area_light_has_origin(L)) {
                            const V3 occ = v3(__uint_as_float(occluder[RT_LIGHT_HIT_POSITION]), __uint_as_float(occluder[RT_LIGHT_HIT_POSITION + 1u]),
                                              __uint_as_float(occluder[RT_LIGHT_HIT_POSITION + 2u])); /* occlusion.at.position */
                            if (distance(pos, occ) < distance(pos, v3(D.origin[0], D.origin[1], D.origin[2]))) lit = false;
                        } else {
                            lit = false;
                        }
                    }
                    if (lit) {
                        DirLight dl;
                        dl.direction = dl.color = v3(0.0f, 0.0f, 0.0f);
                        lit = approximate_into_directional(D, pos, &dl);
                        if (lit) {
                            const V3 light_direction = -dl.direction;
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

/* per light: acc = the first lit sample's term, each later lit term added in ascending s; D = acc_d / spp, S = acc_s / spp; then
 * light_fold_kernel's association, (sum + D * (1 - shiness)) + S * shiness */
__global__ __launch_bounds__(RT_LIGHT_THREADS) void area_fold_kernel(const KernelScene sc, const rt_hit *__restrict__ hits, const uint64_t n,
                                                                     const uint32_t light_count, const uint32_t spp,
                                                                     const unsigned char *__restrict__ lit, const float *__restrict__ diffuse,
                                                                     const float *__restrict__ specular, float *__restrict__ rgb,
                                                                     float *__restrict__ visibility) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_LIGHT_THREADS + threadIdx.x;
    if (i >= n) return;
    const AbiHit h = hit_from_abi(hits + i, sc.n_triangles, sc.n_spheres, sc.n_materials, true);
    if (!h.valid) { /* "no hit": rgb not written, visibility 0 */
        if (visibility != nullptr)
            for (uint32_t l = 0; l < light_count; ++l) visibility[(uint64_t)l * n + i] = 0.0f;
        return;
    }
    const float shiness = material_approx(sc.materials[h.g.obj], h.g.u, h.g.v).shiness;
    const float samples = (float)spp;
    V3 sum = v3(rgb[i * 3u], rgb[i * 3u + 1u], rgb[i * 3u + 2u]);
    for (uint32_t l = 0; l < light_count; ++l) {
        V3 acc_d = v3(0.0f, 0.0f, 0.0f), acc_s = v3(0.0f, 0.0f, 0.0f);
        uint32_t lit_count = 0u;
        for (uint32_t s = 0; s < spp; ++s) {
            const uint64_t k = ((uint64_t)s * light_count + l) * n + i;
            if (lit[k] == 0) continue;
            const V3 d = v3(diffuse[k * 3u], diffuse[k * 3u + 1u], diffuse[k * 3u + 2u]);
            const V3 sp = v3(specular[k * 3u], specular[k * 3u + 1u], specular[k * 3u + 2u]);
            acc_d = lit_count == 0u ? d : acc_d + d;
            acc_s = lit_count == 0u ? sp : acc_s + sp;
            ++lit_count;
        }
        if (visibility != nullptr) visibility[(uint64_t)l * n + i] = (float)lit_count / samples;
        if (lit_count == 0u) continue;
        sum = sum + (acc_d / samples) * (1.0f - shiness) + (acc_s / samples) * shiness;
    }
    rgb[i * 3u] = sum.x;
    rgb[i * 3u + 1u] = sum.y;
    rgb[i * 3u + 2u] = sum.z;
}

} /* namespace rt */

/* ---- the C entry points (include/rt_amd.h "area-light queries") ---- */

/* the block's checks before any device work, in the documented order — those of the light queries' light_args, extended by the sample
 * count; *done: nothing to launch.  light_first < 0: the call takes no range of lights; check_pattern: the call takes a pattern */
static int area_args(const char *who, const rt_scene *scene, size_t n, int64_t light_first, uint32_t light_count, uint32_t spp, bool check_pattern,
                     uint32_t pattern, bool pointers_ok, const char *pointers, bool *done) {
    *done = true;
    const uint64_t pairs = (uint64_t)n * (uint64_t)light_count; /* below 2^64: both factors are below 2^32 where it is used */
    int rc = check_count(who, n, RECORDS_2_32);
    if (rc == RT_OK) rc = check_count(who, pairs, {32u, "(record, light) pairs", "pass the lights in several ranges"});
    if (rc == RT_OK) rc = check_count(who, pairs * (uint64_t)spp, {32u, "(sample, light, record) entries", "pass the lights in several ranges, or fewer samples"});
    if (rc == RT_OK) rc = check_scene(who, scene);
    if (rc != RT_OK || n == 0 || light_count == 0) return rc;
    rc = check_pointers(who, pointers_ok, pointers);
    if (rc != RT_OK) return rc;
    if (const char *bad = rt::area_light_limits(spp, check_pattern, pattern)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + bad);
    if (light_first >= 0 && (uint64_t)light_first + (uint64_t)light_count > (uint64_t)scene->ks.n_lights)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": lights " + std::to_string(light_first) + " .. " +
                                                 std::to_string((uint64_t)light_first + light_count) + " of a scene with " + std::to_string(scene->ks.n_lights));
    *done = false;
    return RT_OK;
}

extern "C" {

int rt_area_light_rays(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, uint32_t light_first, uint32_t light_count,
                       const float *d_radii, const uint32_t *d_ids, uint32_t spp, uint32_t pattern, uint32_t seed, rt_ray *d_shadow_rays,
                       unsigned char *d_asks, float *d_sample, void *hip_stream) {
    bool done;
    const int rc = area_args("rt_area_light_rays", scene, n, light_first, light_count, spp, true, pattern,
                             d_hits && d_incoming && d_radii && d_shadow_rays && d_asks && d_sample,
                             "hit, incoming-ray, radius, shadow-ray, flag or sample", &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::area_rays_kernel, grid_of(n, RT_LIGHT_THREADS), dim3(RT_LIGHT_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks, d_hits,
                       (uint64_t)n, light_first, light_count, d_radii, d_ids, spp, pattern, rt::film_strata(spp), seed, d_shadow_rays, d_asks, d_sample);
    return launched("rt_area_light_rays");
}

int rt_area_light_terms(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, uint32_t light_first, uint32_t light_count,
                        uint32_t spp, const unsigned char *d_asks, const float *d_sample, const rt_hit *d_shadow_hits, unsigned char *d_lit,
                        float *d_diffuse, float *d_specular, void *hip_stream) {
    bool done;
    const int rc = area_args("rt_area_light_terms", scene, n, light_first, light_count, spp, false, 0u,
                             d_hits && d_incoming && d_asks && d_sample && d_shadow_hits && d_lit && d_diffuse && d_specular,
                             "hit, incoming-ray, flag, sample, shadow-hit, lit, diffuse or specular", &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::area_terms_kernel, grid_of(n, RT_LIGHT_THREADS), dim3(RT_LIGHT_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks, d_hits,
                       d_incoming, (uint64_t)n, light_first, light_count, spp, d_asks, d_sample, d_shadow_hits, d_lit, d_diffuse, d_specular);
    return launched("rt_area_light_terms");
}

int rt_area_light_fold(const rt_scene *scene, const rt_hit *d_hits, size_t n, uint32_t light_count, uint32_t spp, const unsigned char *d_lit,
                       const float *d_diffuse, const float *d_specular, float *d_rgb, float *d_visibility, void *hip_stream) {
    bool done;
    const int rc = area_args("rt_area_light_fold", scene, n, -1, light_count, spp, false, 0u, d_hits && d_lit && d_diffuse && d_specular && d_rgb,
                             "hit, lit, diffuse, specular or rgb", &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::area_fold_kernel, grid_of(n, RT_LIGHT_THREADS), dim3(RT_LIGHT_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks, d_hits,
                       (uint64_t)n, light_count, spp, d_lit, d_diffuse, d_specular, d_rgb, d_visibility);
    return launched("rt_area_light_fold");
}

} /* extern "C" */
