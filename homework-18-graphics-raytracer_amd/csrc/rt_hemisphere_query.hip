/*
 * rt_hemisphere_query.hip — the hemisphere over a hit, sampled (include/rt_amd.h "hemisphere queries"): per (sample, record) a
 * cosine-distributed direction about the hit's normal and the shadow ray along it, and the fold that turns the answers of the casts
 * into ambient occlusion and the radiance along those rays into one bounce of diffuse light.
 *
 *   rt::hemisphere_rays_kernel   per (sample, record): the direction, the flag "it leaves the surface", the shadow ray
 *   rt::hemisphere_fold_kernel   per record, over the samples in order: open flags, their share, and the weighted mean radiance
 *
 * Nothing here is new arithmetic but the sampler and the fold (rt_hemisphere.h, shared with librt_host.so): the record is the light
 * queries' own (rt_light_record.h light_record), store_ray is called as that header's store_shadow_ray calls it, and the ray is the
 * one light_rays_kernel writes for a directional light without origin whose direction is -dir — the negation commutes with every rounding of light_asks, so the flag and the eleven words
 * are rt_light_rays'.  One record per lane, the record number counted in 64 bits; the material and the normal once per record; the
 * sample loop is wave-uniform; arrays are sample-major, entry s * n + i, so that the stores of one sample's plane are coalesced.
 * Records move as dwords.  No LDS, no cast.  The C entry points of the block are at the end of the file.
 */
#include "rt_api_internal.h"
#include "rt_hemisphere.h"
#include "rt_light_record.h"

namespace rt {

__global__ __launch_bounds__(RT_LIGHT_THREADS) void hemisphere_rays_kernel(const KernelScene sc, const rt_hit *__restrict__ hits, const uint64_t n,
                                                                           const uint32_t *__restrict__ ids, const uint32_t spp,
                                                                           const uint32_t pattern, const uint32_t strata, const uint32_t seed,
                                                                           const uint32_t normal_kind, rt_ray *__restrict__ shadow_rays,
                                                                           unsigned char *__restrict__ asks, float *__restrict__ dirs) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_LIGHT_THREADS + threadIdx.x;
    if (i >= n) return;
    const LightRecord r = light_record(sc, hits, i);
    const V3 normal = sampling_normal(r, normal_kind);
    const uint32_t id = record_id(ids, i);
    const uint32_t seed_h = hemisphere_seed(seed);
    for (uint32_t s = 0; s < spp; ++s) { /* wave-uniform */
        const uint64_t k = (uint64_t)s * n + i;
        V3 dir = v3(0.0f, 0.0f, 0.0f);
        bool need = false;
        if (r.valid) {
            dir = hemisphere_dir(pattern, strata, id, seed_h, s, normal);
            need = hemisphere_asks(dir, normal);
        }
        /* The tail is written out — store_v3's and store_shadow_ray's lines (rt_light_record.h) — because only in this form does the
         * compiler copy it into both sides of `if (r.valid)` above; through the helpers it emits one shared tail, and that kernel
         * measured 3 - 5 % slower at 4 and 16 samples. */
        dirs[k * 3u] = dir.x;
        dirs[k * 3u + 1u] = dir.y;
        dirs[k * 3u + 2u] = dir.z;
        asks[k] = need ? 1 : 0;
        if (need) /* light_rays_kernel's shadow ray (main.rs:425-433) with -light.direction = dir */
            store_ray(shadow_rays + k, r.h.g.pos, dir, FACE_BACK, 1u, r.h.kind, r.h.index, FACE_BACK);
        else
            store_ray(shadow_rays + k, v3(0.0f, 0.0f, 0.0f), v3(0.0f, 0.0f, 0.0f), 0u, 0u, 0u, 0u, 0u);
    }
}

__global__ __launch_bounds__(RT_LIGHT_THREADS) void hemisphere_fold_kernel(const KernelScene sc, const rt_hit *__restrict__ hits, const HemisphereFold f) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_LIGHT_THREADS + threadIdx.x;
    if (i >= f.n) return;
    const AbiHit h = hit_from_abi(hits + i, sc.n_triangles, sc.n_spheres, sc.n_materials, true);
    V3 diffuse = v3(0.0f, 0.0f, 0.0f);
    float shiness = 0.0f;
    if (h.valid && f.rgb != nullptr) { /* the material is the bounce's alone */
        const Mat m = material_approx(sc.materials[h.g.obj], h.g.u, h.g.v);
        diffuse = m.diffuse;
        shiness = m.shiness;
    }
    hemisphere_fold_record(f, i, h.valid, h.g.pos, diffuse, shiness);
}

} /* namespace rt */

/* ---- the C entry points (include/rt_amd.h "hemisphere queries") ---- */

/* the checks before any device work are hit_sample_args' (rt_api_internal.h): the area-light queries' without the lights.  Only
 * rt_hemisphere_rays takes a pattern and a normal_kind */
extern "C" {

int rt_hemisphere_rays(const rt_scene *scene, const rt_hit *d_hits, size_t n, const uint32_t *d_ids, uint32_t spp, uint32_t pattern, uint32_t seed,
                       uint32_t normal_kind, rt_ray *d_rays, unsigned char *d_asks, float *d_dirs, void *hip_stream) {
    bool done;
    const int rc = hit_sample_args("rt_hemisphere_rays", scene,
                                   HitSampleArgs(n, d_hits && d_rays && d_asks && d_dirs, "hit, ray, flag or direction")
                                       .samples(spp).limits(rt::hemisphere_limits(spp, true, pattern, normal_kind)), &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::hemisphere_rays_kernel, grid_of(n, RT_LIGHT_THREADS), dim3(RT_LIGHT_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks, d_hits,
                       (uint64_t)n, d_ids, spp, pattern, rt::film_strata(spp), seed, normal_kind, d_rays, d_asks, d_dirs);
    return launched("rt_hemisphere_rays");
}

int rt_hemisphere_fold(const rt_scene *scene, const rt_hit *d_hits, size_t n, uint32_t spp, const unsigned char *d_asks, const rt_hit *d_shadow_hits,
                       float max_distance, const float *d_radiance, unsigned char *d_open, float *d_ambient, float *d_rgb, void *hip_stream) {
    bool done;
    const bool paired = (d_radiance != nullptr) == (d_rgb != nullptr);
    const int rc = hit_sample_args("rt_hemisphere_fold", scene,
                                   HitSampleArgs(n, d_hits && d_asks && paired, paired ? "hit or flag" : "radiance or rgb (they are given together or not at all)")
                                       .samples(spp).limits(rt::hemisphere_limits(spp, false, 0u, 0u)), &done);
    if (rc != RT_OK || done) return rc;
    const rt::HemisphereFold f = {(uint64_t)n, spp, d_asks, reinterpret_cast<const uint32_t *>(d_shadow_hits), max_distance, d_radiance, d_open, d_ambient, d_rgb};
    hipLaunchKernelGGL(rt::hemisphere_fold_kernel, grid_of(n, RT_LIGHT_THREADS), dim3(RT_LIGHT_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks, d_hits, f);
    return launched("rt_hemisphere_fold");
}

} /* extern "C" */
