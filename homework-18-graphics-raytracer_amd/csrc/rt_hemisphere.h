/*
 * rt_hemisphere.h — the arithmetic of the hemisphere queries (include/rt_amd.h "hemisphere queries"), written once for the host
 * (librt_host.so: rt_hemisphere_dirs_cpu / rt_hemisphere_fold_cpu) and the device (rt_hemisphere_query.hip).  Sample s of record `id`
 * is a direction, cosine-distributed about a normal N: a point of the unit disc chosen by rt_film.h's counter hash, lifted onto the
 * hemisphere about +z (Malley) and rotated onto N by rt_shade.h's adjust_normal, the reference's own Quaternion::from_arc.  The fold
 * turns what the casts and the radiance query answered along those directions into an ambient-occlusion value and one bounce of
 * diffuse light per record.  Every function is a sequence of single f32 or u32 operations in the order the header comment of the
 * block gives; both libraries are built with -ffp-contract=off and sqrt and the divide are correctly rounded on either side, so the
 * host and the device forms agree bit for bit.
 */
#ifndef RT_HEMISPHERE_H
#define RT_HEMISPHERE_H

#include <math.h>
#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_area_light.h" /* area_light_limits: the limits of spp and pattern, and their texts */
#include "rt_film.h"
#include "rt_shade.h"
#include "rt_vec.h"

namespace rt {

#define RT_HEMISPHERE_HIT_WORDS 13u   /* an rt_hit in words */
#define RT_HEMISPHERE_HIT_POSITION 3u /* word of rt_hit.position */

/* the hemispheres draw from a stream of their own, apart from the area lights' (area_light_seed) and the film's */
RT_FILM_HD uint32_t hemisphere_seed(uint32_t seed) { return film_mix(seed ^ 0x85ebca6bu); }

/* sample s of record `id` about +z; k: film_strata(spp) (used by RT_FILM_STRATIFIED only).  r = sqrt(u_0) and phi uniform are a
 * uniform point of the disc, and z = sqrt(1 - u_0) lifts it to a cosine-distributed direction.  A u_0 that rounds to 1 gives z = 0: a
 * direction in the tangent plane, which hemisphere_asks refuses. */
RT_FILM_HD V3 hemisphere_local(uint32_t pattern, uint32_t k, uint32_t id, uint32_t seed_h, uint32_t s) {
    const float u0 = film_offset(pattern, k, id, seed_h, s, 0u) + 0.5f;
    const float u1 = film_offset(pattern, k, id, seed_h, s, 1u) + 0.5f;
    const float r = rtdm::f_sqrt(u0);
    const float z = rtdm::f_sqrt(fmaxf(1.0f - u0, 0.0f));
    const float phi = 6.2831855f * u1;
    float sine, cosine;
    rtdm::sincosf(phi, &sine, &cosine);
    return v3(r * cosine, r * sine, z);
}

/* ... and about the normal n */
RT_FILM_HD V3 hemisphere_dir(uint32_t pattern, uint32_t k, uint32_t id, uint32_t seed_h, uint32_t s, V3 n) {
    return adjust_normal(hemisphere_local(pattern, k, id, seed_h, s), n);
}

/* light_asks' test (rt_shade.h) for a directional light whose direction is -dir: -dot(-dir, n) is dot(dir, n) bit for bit */
RT_FILM_HD bool hemisphere_asks(V3 dir, V3 n) { return !(dot(dir, n) <= 0.0f); }

/* one fold call: sample-major arrays of spp * n entries, entry s * n + i */
struct HemisphereFold {
    uint64_t n;
    uint32_t spp;
    const unsigned char *asks;
    const uint32_t *shadow_hits; /* rt_hit records as words; null: nothing occludes */
    float max_distance;
    const float *radiance;       /* null together with rgb */
    unsigned char *open;         /* may be null */
    float *ambient;              /* may be null */
    float *rgb;                  /* may be null */
};

/* Record i of a fold; valid: the record is a hit, pos its position, diffuse and shiness its material's.  Samples in ascending order:
 * a sample is open where it was asked and no answered cast lies nearer than max_distance (a NaN distance compares false: open);
 * ambient = open samples / spp; E = (the asked samples' radiance, the first as it is and each later one added) / spp, and
 * rgb = rgb + (diffuse * E) * (1 - shiness).  A record that is no hit: every flag 0, ambient 0, rgb not written. */
RT_FILM_HD void hemisphere_fold_record(const HemisphereFold &f, uint64_t i, bool valid, V3 pos, V3 diffuse, float shiness) {
    V3 acc = v3(0.0f, 0.0f, 0.0f);
    uint32_t asked_count = 0u, open_count = 0u;
    for (uint32_t s = 0; s < f.spp; ++s) {
        const uint64_t k = (uint64_t)s * f.n + i;
        const bool asked = valid && f.asks[k] != 0;
        bool open = asked;
        if (asked && f.shadow_hits != nullptr) {
            const uint32_t *const occluder = f.shadow_hits + k * RT_HEMISPHERE_HIT_WORDS;
            if (occluder[0] <= 1u) { /* Some(occlusion) */
                const V3 occ = v3(rtdm::f32_from_bits(occluder[RT_HEMISPHERE_HIT_POSITION]), rtdm::f32_from_bits(occluder[RT_HEMISPHERE_HIT_POSITION + 1u]),
                                  rtdm::f32_from_bits(occluder[RT_HEMISPHERE_HIT_POSITION + 2u])); /* occlusion.at.position */
                if (distance(pos, occ) < f.max_distance) open = false;
            }
        }
        if (f.open != nullptr) f.open[k] = open ? 1 : 0;
        if (open) ++open_count;
        if (asked && f.rgb != nullptr) {
            const V3 l = v3(f.radiance[k * 3u], f.radiance[k * 3u + 1u], f.radiance[k * 3u + 2u]);
            acc = asked_count == 0u ? l : acc + l;
            ++asked_count;
        }
    }
    const float samples = (float)f.spp;
    if (f.ambient != nullptr) f.ambient[i] = (float)open_count / samples; /* 0 for a record that is no hit */
    if (f.rgb == nullptr || asked_count == 0u) return;
    const V3 sum = v3(f.rgb[i * 3u], f.rgb[i * 3u + 1u], f.rgb[i * 3u + 2u]) + (diffuse * (acc / samples)) * (1.0f - shiness);
    f.rgb[i * 3u] = sum.x;
    f.rgb[i * 3u + 1u] = sum.y;
    f.rgb[i * 3u + 2u] = sum.z;
}

/* the limits of spp, pattern and normal_kind, for the device calls and the CPU forms; null: all in range.  spp and pattern are the
 * area lights', with their texts.  check_sampler: the call takes a pattern and a normal_kind */
inline const char *hemisphere_limits(uint32_t spp, bool check_sampler, uint32_t pattern, uint32_t normal_kind) {
    if (const char *bad = area_light_limits(spp, check_sampler, pattern)) return bad;
    if (check_sampler && normal_kind != RT_HEMISPHERE_SHADING && normal_kind != RT_HEMISPHERE_GEOMETRIC)
        return "unknown normal_kind (RT_HEMISPHERE_SHADING or RT_HEMISPHERE_GEOMETRIC)";
    return nullptr;
}

} /* namespace rt */

#endif /* RT_HEMISPHERE_H */
