/*
 * rt_path.h — the arithmetic of the path queries (include/rt_amd.h "path queries"), written once for the host (librt_host.so:
 * rt_path_begin_cpu / rt_path_advance_cpu / rt_path_resolve_cpu) and the device (rt_path_query.hip).  One step of a path is what five
 * calls of the other blocks compute between two casts, on one record: rt_lobe.h's sampler and density for the direction, rt_shade.h's
 * get_diffuse and get_specular for the terms, rt_lobe.h's weighing "over its own density" for the throughput and rt_environment.h's
 * fold association for the mixture of the two terms — called here, none of them written again — and then what no call had: the
 * throughput carried in the record, Russian roulette from a stream of the counter hash (path_step_tail, which rt_transmit.h's fold of a
 * walk through glass calls too), and the mean of a pixel's paths.  Every
 * function is a sequence of single f32 or u32 operations in the order the header comment of the block gives; both libraries are built
 * with -ffp-contract=off and the divides are correctly rounded on either side, so the host and the device forms agree bit for bit.
 */
#ifndef RT_PATH_H
#define RT_PATH_H

#include <math.h>
#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_film.h"
#include "rt_hemisphere.h"
#include "rt_lobe.h"
#include "rt_shade.h"
#include "rt_vec.h"

namespace rt {

#define RT_PATH_WORDS 8u
static_assert(sizeof(rt_path) == RT_PATH_WORDS * sizeof(uint32_t), "rt_path is 8 dwords");

#define RT_PATH_ROULETTE_STREAM 0x165667b1u /* u_3's stream: film_mix(seed_h ^ RT_PATH_ROULETTE_STREAM), apart from u_0's, u_1's and u_2's */
#define RT_PATH_BOUNCE_STEP 0x9e3779b9u     /* the seed of bounce b: seed + RT_PATH_BOUNCE_STEP * b, a u32 wrap */
#define RT_PATH_SAMPLE_SHIFT 24u            /* rt_path.bounce: the sample index s above, the bounces taken below */
#define RT_PATH_BOUNCE_MASK 0x00ffffffu

RT_FILM_HD uint32_t path_bounce_word(uint32_t s, uint32_t bounces) { return (s << RT_PATH_SAMPLE_SHIFT) | (bounces & RT_PATH_BOUNCE_MASK); }

/* rt_path_begin's record of sample s of root i */
RT_FILM_HD rt_path path_begin_record(uint32_t root, uint32_t id, uint32_t s) {
    rt_path p;
    p.beta[0] = p.beta[1] = p.beta[2] = 1.0f;
    p.pdf = 0.0f;
    p.root = root;
    p.id = id;
    p.bounce = path_bounce_word(s, 0u);
    p.flags = RT_PATH_ALIVE;
    return p;
}

/* the call's own arguments */
struct PathStep {
    uint32_t seed, rr_start;
    float rr_floor;
    bool last;
};

/* the limits of rr_floor and normal_kind; null: all in range */
inline const char *path_limits(uint32_t normal_kind, float rr_floor) {
    if (const char *bad = hemisphere_limits(1u, true, RT_FILM_UNIFORM, normal_kind)) return bad;
    if (!(rr_floor > 0.0f && rr_floor <= 1.0f)) return "rr_floor must lie in (0, 1]";
    return nullptr;
}

/* the deposit of one channel: the product rounded, then the sum */
RT_FILM_HD float path_deposit(float radiance, float beta, float emitted) { return radiance + beta * emitted; }

/* The end of a step, on the new throughput *next — shared by path_advance_record and rt_transmit.h's path_transmit_record: the dark test
 * (`ok` is the direction's flag), then roulette from the bounce's own stream where bounces + 1 >= rr_start, with `seed_h` the bounce's
 * hemisphere_seed.  Returns the flag the path ends with, or 0: it survives, and *next is divided by its chance. */
RT_FILM_HD uint32_t path_step_tail(V3 *next_io, bool ok, uint32_t id, uint32_t s, uint32_t bounces, uint32_t seed_h, const PathStep &q) {
    V3 next = *next_io;
    if (!ok || !(next.x > 0.0f || next.y > 0.0f || next.z > 0.0f)) return RT_PATH_DARK;

    /* roulette: q = the largest channel (a NaN channel is passed over), raised to rr_floor, cut at 1 */
    if (bounces + 1u >= q.rr_start) {
        float chance = 0.0f;
        chance = next.x > chance ? next.x : chance;
        chance = next.y > chance ? next.y : chance;
        chance = next.z > chance ? next.z : chance;
        chance = chance < q.rr_floor ? q.rr_floor : chance;
        chance = chance > 1.0f ? 1.0f : chance;
        const float u3 = film_u(id, film_mix(seed_h ^ RT_PATH_ROULETTE_STREAM), s, 0u);
        if (!(u3 < chance)) return RT_PATH_ROULETTE;
        next = next / chance;
    }
    *next_io = next;
    return 0u;
}

/* One ALIVE path at a vertex, after the deposit.  `hit`: the record is a hit by the hit queries' rules, `m` its material, `shading_n`
 * adjust_normal of its normal — the N of the terms — and `sampling_n` the N the direction is drawn about (normal_kind), `view` minus
 * the incoming direction.  The record `p` is advanced in place; *dir: the direction drawn, zeros for a path that ended.  Returns
 * whether the path lives on.  A lane whose path ends before the sample still walks through lobe_sample and get_specular with
 * live = false, so that their wave-level branches see every lane of the wave. */
RT_FILM_HD bool path_advance_record(rt_path &p, bool hit, const Mat &m, V3 shading_n, V3 sampling_n, V3 view, const PathStep &q, V3 *dir) {
    const uint32_t s = p.bounce >> RT_PATH_SAMPLE_SHIFT, bounces = p.bounce & RT_PATH_BOUNCE_MASK;
    const bool draws = hit && !q.last;
    uint32_t ended = hit ? 0u : RT_PATH_ESCAPED; /* `last`: no flag at all */
    *dir = v3(0.0f, 0.0f, 0.0f);

    /* the sample: rt_lobe_rays' for spp = 1, RT_FILM_UNIFORM, id and sample s, with the bounce's seed */
    const uint32_t seed_h = hemisphere_seed(q.seed + RT_PATH_BOUNCE_STEP * bounces);
    const LobeSurface surface = lobe_surface(sampling_n, view, m.shiness, m.smoothness);
    const LobeSample d = lobe_sample(surface, RT_FILM_UNIFORM, 1u, p.id, seed_h, s, draws);

    /* the terms: rt_probe_surfaces' for that direction */
    V3 diffuse = v3(0.0f, 0.0f, 0.0f), specular = v3(0.0f, 0.0f, 0.0f);
    if (draws) {
        diffuse = get_diffuse(m, shading_n, d.dir);
        specular = get_specular(m, shading_n, view, d.dir);
    }
    if (!draws) {
        p.flags = ended;
        return false;
    }

    /* the throughput: mis_weigh_entry with divide_by_own and no other strategy (w is 1 here: d.ok says the density is finite and > 0),
     * then env_fold_record's association for one sample into a zeroed rgb */
    const V3 beta = v3(p.beta[0], p.beta[1], p.beta[2]);
    const float f = d.ok ? 1.0f / d.pdf : 0.0f;
    const V3 t = beta * f;
    V3 next = v3(0.0f, 0.0f, 0.0f) + (diffuse * t) * (1.0f - m.shiness) + (specular * t) * m.shiness;
    if (const uint32_t ended = path_step_tail(&next, d.ok, p.id, s, bounces, seed_h, q)) {
        p.flags = ended;
        return false;
    }

    p.beta[0] = next.x;
    p.beta[1] = next.y;
    p.beta[2] = next.z;
    p.pdf = d.pdf;
    p.bounce = path_bounce_word(s, bounces + 1u);
    p.flags = RT_PATH_ALIVE | (d.specular ? RT_PATH_SPECULAR : 0u);
    *dir = d.dir;
    return true;
}

/* the live length of a list: all m slots without an index, else min(*count, m) */
RT_FILM_HD uint32_t path_listed(const uint32_t *index, const uint32_t *count, uint32_t m) {
    if (index == nullptr) return m;
    const uint32_t c = *count;
    return c < m ? c : m;
}

/* root i of a resolve: the samples in ascending order, the first as it is and each later one added, / (float)spp, ADDED to rgb's slot */
RT_FILM_HD void path_resolve_root(const float *radiance, uint64_t n, uint32_t spp, uint64_t i, const uint32_t *root, float *rgb) {
    V3 acc = v3(0.0f, 0.0f, 0.0f);
    for (uint32_t s = 0; s < spp; ++s) {
        const V3 l = v3p(radiance + ((uint64_t)s * n + i) * 3u);
        acc = s == 0u ? l : acc + l;
    }
    const V3 mean = acc / (float)spp;
    const uint64_t slot = root != nullptr ? root[i] : i;
    rgb[slot * 3u] = rgb[slot * 3u] + mean.x;
    rgb[slot * 3u + 1u] = rgb[slot * 3u + 1u] + mean.y;
    rgb[slot * 3u + 2u] = rgb[slot * 3u + 2u] + mean.z;
}

} /* namespace rt */

#endif /* RT_PATH_H */
