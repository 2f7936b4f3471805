/*
 * rt_area_light.h — the sampler of the area-light queries (include/rt_amd.h "area-light queries"), written once for the host
 * (librt_host.so: rt_area_light_samples_cpu) and the device (rt_area_light_query.hip).  A light with a radius is a sphere around its
 * origin (around the tip of its direction, for a directional light without origin); sample s of record `id` for light l is a point
 * chosen uniformly on that sphere by rt_film.h's counter hash, and the displaced light is the stored one with that point in the place
 * of its origin (or direction).  Every function is a sequence of single f32 or u32 operations in the order the header comment of the
 * block gives; both libraries are built with -ffp-contract=off and sqrt is correctly rounded on either side, so the host and the
 * device forms agree bit for bit.
 */
#ifndef RT_AREA_LIGHT_H
#define RT_AREA_LIGHT_H

#include <math.h>
#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_film.h"
#include "rt_vec.h"

namespace rt {

#define RT_AREA_LIGHT_MAX_SPP 64u

/* the seed of light l (its absolute index in the scene): lights draw from streams of their own */
RT_FILM_HD uint32_t area_light_seed(uint32_t seed, uint32_t l) { return film_mix(seed ^ (0x9e3779b9u * (l + 1u))); }

/* the offset on the unit sphere of sample s of record `id`; k: film_strata(spp) (used by RT_FILM_STRATIFIED only).  z uniform in
 * (-1, 1] and phi uniform in [0, 2 pi) are a uniform point (Archimedes); rtdm::sincosf gives rtdm::sinf's and rtdm::cosf's bits. */
RT_FILM_HD V3 area_light_offset(uint32_t pattern, uint32_t k, uint32_t id, uint32_t seed_l, uint32_t s) {
    const float u0 = film_offset(pattern, k, id, seed_l, s, 0u) + 0.5f;
    const float u1 = film_offset(pattern, k, id, seed_l, s, 1u) + 0.5f;
    const float z = 1.0f - 2.0f * u0;
    const float r = rtdm::f_sqrt(fmaxf(1.0f - z * z, 0.0f));
    const float phi = 6.2831855f * u1;
    float sine, cosine;
    rtdm::sincosf(phi, &sine, &cosine);
    return v3(r * cosine, r * sine, z);
}

template <class Light>
RT_FILM_HD bool area_light_has_origin(const Light &l) { return (l.kind != RT_LIGHT_DIRECTIONAL) || (l.has_origin != 0u); }

/* what a light is displaced at: its origin, or its direction where it has none */
template <class Light>
RT_FILM_HD V3 area_light_anchor(const Light &l) {
    return area_light_has_origin(l) ? v3(l.origin[0], l.origin[1], l.origin[2]) : v3(l.direction[0], l.direction[1], l.direction[2]);
}

/* the anchor moved by offset * rad, rad > 0: per component the product, then the add; a direction is normalised again */
template <class Light>
RT_FILM_HD V3 area_light_moved(const Light &l, float rad, V3 offset) {
    const V3 moved = area_light_anchor(l) + offset * rad;
    return area_light_has_origin(l) ? moved : normalize(moved);
}

/* The sample of (light l of the scene, record id, sample s): !(rad > 0) — zero, negative, NaN — is the stored anchor, no word of it
 * touched and nothing hashed. */
template <class Light>
RT_FILM_HD V3 area_light_sample(const Light &l, uint32_t light_index, float rad, uint32_t pattern, uint32_t k, uint32_t id, uint32_t seed, uint32_t s) {
    if (!(rad > 0.0f)) return area_light_anchor(l);
    return area_light_moved(l, rad, area_light_offset(pattern, k, id, area_light_seed(seed, light_index), s));
}

/* the light with `sample` in the place of its anchor, every other field as stored: a copy in registers */
template <class Light>
RT_FILM_HD rt_light area_light_displaced(const Light &l, V3 sample) {
    rt_light d;
    d.kind = l.kind;
    d.has_origin = l.has_origin;
    const bool at_origin = area_light_has_origin(l);
    d.origin[0] = at_origin ? sample.x : l.origin[0];
    d.origin[1] = at_origin ? sample.y : l.origin[1];
    d.origin[2] = at_origin ? sample.z : l.origin[2];
    d.direction[0] = at_origin ? l.direction[0] : sample.x;
    d.direction[1] = at_origin ? l.direction[1] : sample.y;
    d.direction[2] = at_origin ? l.direction[2] : sample.z;
    d.angle = l.angle;
    d.softness = l.softness;
    d.color[0] = l.color[0];
    d.color[1] = l.color[1];
    d.color[2] = l.color[2];
    return d;
}

/* the limits of spp and pattern, for the device calls and the CPU form; null: all in range.  check_pattern: the call takes one */
inline const char *area_light_limits(uint32_t spp, bool check_pattern, uint32_t pattern) {
    if (spp < 1u || spp > RT_AREA_LIGHT_MAX_SPP) return "spp must be in 1 .. 64";
    if (!check_pattern) return nullptr;
    if (pattern == RT_FILM_CENTER) return "RT_FILM_CENTER is no pattern of an area light (RT_FILM_UNIFORM or RT_FILM_STRATIFIED)";
    if (pattern != RT_FILM_UNIFORM && pattern != RT_FILM_STRATIFIED) return "unknown pattern (RT_FILM_UNIFORM or RT_FILM_STRATIFIED)";
    if (pattern == RT_FILM_STRATIFIED && film_strata(spp) == 0u) return "a stratified pattern needs spp = k * k with 1 <= k <= 8";
    return nullptr;
}

} /* namespace rt */

#endif /* RT_AREA_LIGHT_H */
