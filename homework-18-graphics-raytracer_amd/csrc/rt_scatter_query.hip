/*
 * rt_scatter_query.hip — scatter queries: the three generator draws distributed_ray_trace (main.rs:521-614) makes per level, on
 * caller-supplied rt_hit records, and the level's factor once the next ray is known.
 *
 *   rt::scatter_hits_kernel     one work-item per record: weighted_select (main.rs:652-666, one draw) and scatter_hit (main.rs:539-554,
 *                               two draws) on the record's generator, which is opened, advanced by exactly three words and parked
 *   rt::scatter_factors_kernel  one work-item per record: get_diffuse / get_specular on the geometric normal, or opaque_decay^travel
 *                               (main.rs:566-570, 585-589, 605); pure
 *
 * Nothing here is new arithmetic.  The level is rt_dist_advance.inc:70-99 with the same helper calls on the same values (rtdm::powf,
 * rtdm::acosf, the fused rtdm::sincosf, adjust_normal(v, normalize(lobe))), the factor is rt_dist_advance.inc:30-37, and the generator
 * is the stochastic pass's, rt_rng.h (rng_open, next_u32x3, range_f32_of, rng_park) — so rt_distributed.hip's exactness argument carries
 * over unchanged.  Records are validated as the hit queries validate them (rt_hit_abi.h); a record that is "no hit" never opens its
 * generator.
 *
 * Of the stochastic pass this unit includes the generator alone; the materials (material_approx, get_diffuse, adjust_normal) are
 * rt_shade.h's, which rt_hit_abi.h brings with rt_cast.h.
 */
#include "rt_rng.h"
#include "rt_hit_abi.h"
#include "rt_api_internal.h"

namespace rt {

/* Record i draws from generator g = rng_index ? rng_index[i] : first_generator + i.  A dry generator without a prepared bank runs
 * IsaacCore::generate here, in HBM (rng.lds = nullptr, as focus_rays_kernel); with the look-ahead pass ahead of the launch
 * (launch_rng_prepare) it only switches banks. */
__global__ __launch_bounds__(256) void scatter_hits_kernel(const KernelScene sc, const rt_hit *__restrict__ hits, const rt_ray *__restrict__ incoming,
                                                           uint32_t *states, const uint32_t n_generators, const uint32_t *__restrict__ rng_index,
                                                           const uint32_t first_generator, uint32_t *__restrict__ out_type,
                                                           rt_ray *__restrict__ out_scattered, float *__restrict__ out_cosine, const uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = rng_index != nullptr ? rng_index[i] : first_generator + i;
    const AbiHit h = hit_from_abi(hits + i, sc.n_triangles, sc.n_spheres, sc.n_materials, true);
    if (!h.valid || g >= n_generators) { /* "no hit": nothing is drawn */
        out_type[i] = RT_HIT_NONE;
        store_ray(out_scattered + i, v3(0.0f, 0.0f, 0.0f), v3(0.0f, 0.0f, 0.0f), 0u, 0u, 0u, 0u, 0u);
        if (out_cosine != nullptr) out_cosine[i] = 0.0f;
        return;
    }
    const rt_ray *const in_rec = incoming + i;
    const Ray in = ray_from_abi(in_rec, sc.n_triangles, sc.n_spheres);
    const V3 h_in_dir = in.d; /* hit.ray.direction */
    const rt_material &rm = sc.materials[h.g.obj];
    /* weighted_select (main.rs:652-666) */
    const float w0 = (1.0f - rm.shiness) * (1.0f - rm.transparency);
    const float w1 = rm.shiness * (1.0f - rm.transparency);
    const float w2 = rm.transparency;
    float wsum = 0.0f;
    wsum = wsum + w0;
    wsum = wsum + w1;
    wsum = wsum + w2;
    Rng rng;
    rng.lds = nullptr;
    rng_open(rng, states + (size_t)g * RNG_WORDS);
    uint32_t word_sel, word_phi, word_theta; /* the level's three draws, in stream order */
    next_u32x3(rng, &word_sel, &word_phi, &word_theta);
    rng_park(rng);
    const float rsel = range_f32_of(word_sel, 0.0f, wsum);
    float acc = 0.0f;
    acc += w0;
    uint32_t kind = 2u;
    if (rsel < acc) kind = 0u;
    else {
        acc += w1;
        if (rsel < acc) kind = 1u;
    }
    /* scatter_hit (main.rs:539-554) */
    const float exponent = kind == 0u ? 1.0f : rm.smoothness;
    const V3 lobe = kind == 0u ? -h.g.normal : h_in_dir;
    const float phi = rtdm::acosf(rtdm::powf(1.0f - range_f32_of(word_phi, 0.0f, 1.0f), exponent));
    const float theta = range_f32_of(word_theta, -RT_F_PI, RT_F_PI);
    float sphi, cphi, stheta, ctheta;
    rtdm::sincosf(phi, &sphi, &cphi);
    rtdm::sincosf(theta, &stheta, &ctheta);
    const V3 sdir = adjust_normal(v3(sphi * ctheta, sphi * stheta, cphi), normalize(lobe));
    const float cosine = -dot(h.g.normal, sdir);
    out_type[i] = kind;
    /* scattered_hit.ray: hit.ray with the new direction — the face mode as it was read, the exclusion's words as they came */
    store_ray(out_scattered + i, in.o, sdir, in.mode, in_rec->has_exclude, in_rec->exclude_kind, in_rec->exclude_index, in_rec->exclude_face);
    if (out_cosine != nullptr) out_cosine[i] = cosine;
}

/* the level's factor, rt_dist_advance.inc:30-37, in all three channels for a refraction */
__global__ __launch_bounds__(256) void scatter_factors_kernel(const KernelScene sc, const rt_hit *__restrict__ hits, const rt_ray *__restrict__ incoming,
                                                              const uint32_t *__restrict__ types, const rt_ray *__restrict__ next,
                                                              const float *__restrict__ travel, float *__restrict__ rgb, const uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    V3 factor = v3(0.0f, 0.0f, 0.0f);
    const uint32_t kind = types[i];
    const AbiHit h = hit_from_abi(hits + i, sc.n_triangles, sc.n_spheres, sc.n_materials, true);
    if (h.valid && kind <= 2u) {
        if (kind == 2u) {
            const float decay = rtdm::powf(sc.materials[h.g.obj].opaque_decay, travel[i]);
            factor = v3(decay, decay, decay);
        } else {
            const Mat m = material_approx(sc.materials[h.g.obj], h.g.u, h.g.v);
            const V3 h_in_dir = ray_from_abi(incoming + i, sc.n_triangles, sc.n_spheres).d;
            const V3 light = ray_from_abi(next + i, sc.n_triangles, sc.n_spheres).d;
            const V3 view = -h_in_dir;
            factor = kind == 0u ? get_diffuse(m, h.g.normal, light) : get_specular(m, h.g.normal, view, light);
        }
    }
    rgb[(size_t)i * 3u] = factor.x;
    rgb[(size_t)i * 3u + 1u] = factor.y;
    rgb[(size_t)i * 3u + 2u] = factor.z;
}

/* Bands of at most band_records records per launch (rt_api_internal.h for_each_band, as rt_hit_query.hip).  Without an index array a
 * band's first generator is the band's first record. */

hipError_t launch_scatter_hits(const KernelScene &sc, const rt_hit *hits, const rt_ray *incoming, uint32_t n, uint32_t *states, uint32_t n_generators,
                               const uint32_t *rng_index, uint32_t *type, rt_ray *scattered, float *cosine, uint32_t band_records, hipStream_t stream) {
    return for_each_band(n, band_records, [&](uint64_t off, uint32_t band) {
        hipLaunchKernelGGL(scatter_hits_kernel, grid_of(band, 256u), dim3(256), 0, stream, sc, hits + off, incoming + off, states, n_generators,
                           rng_index != nullptr ? rng_index + off : nullptr, (uint32_t)off, type + off, scattered + off,
                           cosine != nullptr ? cosine + off : nullptr, band);
    });
}

hipError_t launch_scatter_factors(const KernelScene &sc, const rt_hit *hits, const rt_ray *incoming, const uint32_t *types, const rt_ray *next,
                                  const float *travel, uint32_t n, float *rgb, uint32_t band_records, hipStream_t stream) {
    return for_each_band(n, band_records, [&](uint64_t off, uint32_t band) {
        hipLaunchKernelGGL(scatter_factors_kernel, grid_of(band, 256u), dim3(256), 0, stream, sc, hits + off, incoming + off, types + off,
                           next + off, travel + off, rgb + (size_t)off * 3u, band);
    });
}

} /* namespace rt */
