/*
 * rt_light_connect.h — the arithmetic of the light-connection queries (include/rt_amd.h "light-connection queries"), written once for
 * the host (librt_host.so: rt_path_connect_lights_cpu / rt_path_settle_lights_cpu) and the device (rt_light_connect_query.hip).
 * Next-event estimation of the scene's own lights inside the path loop is two steps on the 32-byte record of rt_path.h, neither of
 * which writes it: one light chosen at the path's vertex and one point on its sphere, its Phong terms multiplied by the throughput over
 * the chance of the choice before its shadow cast is answered (light_connect_record); and the answer added to the path's radiance by
 * get_shade's own occlusion rule (light_settle_record).  Nothing here is a sampler, a density or a Phong term of its own:
 * rt_area_light.h's area_light_sample / area_light_displaced, rt_shade.h's light_asks, approximate_into_directional, get_diffuse and
 * get_specular and rt_path.h's helpers are called as rt_area_light_rays, rt_light_terms and rt_path_advance call them.  Every function
 * is a sequence of single f32 or u32 operations in the order the header comment of the block gives; both libraries are built with
 * -ffp-contract=off and the divides and square roots are correctly rounded on either side, so the host and the device forms agree bit
 * for bit.
 *
 * The streams.  With seed_b = seed + RT_PATH_BOUNCE_STEP * b and seed_h = hemisphere_seed(seed_b), the light is chosen by
 * u_5 = film_u(id, film_mix(seed_h ^ RT_LIGHT_CONNECT_CHOICE_STREAM), s, 0) — made as the roulette's u_3 is, with 0x2545f491 in the
 * place of 0x165667b1 — and the point on the light by rt_area_light_rays' two uniforms for the seed light_connect_seed(seed_b) =
 * film_mix(seed_b ^ RT_LIGHT_CONNECT_POINT_STREAM), 0x68e31da4.  Neither constant is one of 0xc2b2ae35 (the sky connection),
 * 0x85ebca6b (the lobe, and the transmission's u_4 inside it), 0x165667b1 (the roulette) and 0x27d4eb2f (the lobe's choice).
 *
 * No multiple importance sampling: the scene's lights are not geometry, so no lobe-sampled ray ever finds one — the connection is the
 * only strategy that reaches them, and its weight is 1.
 */
#ifndef RT_LIGHT_CONNECT_H
#define RT_LIGHT_CONNECT_H

#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_area_light.h"
#include "rt_film.h"
#include "rt_hemisphere.h"
#include "rt_path.h"
#include "rt_shade.h"
#include "rt_vec.h"

namespace rt {

#define RT_LIGHT_CONNECT_CHOICE_STREAM 0x2545f491u /* u_5's stream: film_mix(seed_h ^ RT_LIGHT_CONNECT_CHOICE_STREAM), apart from u_0 .. u_4's */
#define RT_LIGHT_CONNECT_POINT_STREAM 0x68e31da4u  /* the point's seed: film_mix(seed_b ^ RT_LIGHT_CONNECT_POINT_STREAM), handed to area_light_sample */
#define RT_LIGHT_CONNECT_NONE 0xffffffffu          /* d_chosen of a path that drew no light */
#define RT_LIGHT_CONNECT_RAY_WORDS 11u
#define RT_LIGHT_CONNECT_HIT_WORDS 13u
#define RT_LIGHT_CONNECT_HIT_POSITION 3u /* word of rt_hit.position */
static_assert(sizeof(rt_ray) == RT_LIGHT_CONNECT_RAY_WORDS * sizeof(uint32_t), "rt_ray is 11 dwords");
static_assert(sizeof(rt_hit) == RT_LIGHT_CONNECT_HIT_WORDS * sizeof(uint32_t), "rt_hit is 13 dwords");

/* the seed rt_area_light_rays takes to draw the points this block draws at the bounce whose seed is seed_b */
RT_FILM_HD uint32_t light_connect_seed(uint32_t seed_b) { return film_mix(seed_b ^ RT_LIGHT_CONNECT_POINT_STREAM); }

/* u_5 in [0, 1): the uniform the light is chosen by */
RT_FILM_HD float light_connect_u(uint32_t seed_b, uint32_t id, uint32_t s) {
    return film_u(id, film_mix(hemisphere_seed(seed_b) ^ RT_LIGHT_CONNECT_CHOICE_STREAM), s, 0u);
}

/* the call's own arguments; radii and weights hold light_count floats each, or are null */
struct LightConnect {
    uint32_t seed, light_first, light_count;
    const float *radii, *weights;
};

/* the light chosen, relative to light_first, and one over the chance it was chosen with; !ok: nothing can be chosen */
struct LightChoice {
    uint32_t l;
    float inv_p;
    bool ok;
};

/* a weight as the choice counts it: one that is not > 0 — zero, negative, NaN — is 0 */
RT_FILM_HD float light_connect_weight(float w) { return w > 0.0f ? w : 0.0f; }

/* weights null: uniform, l = min((uint32_t)(u * count), count - 1), inv_p = (float)count.  Else the running sum in ascending order in
 * f32; the light chosen is the first whose running sum exceeds u * total, so a light of weight 0 is never chosen; should rounding leave
 * no such light (u * total is below total for every u the hash gives, so it does not), the last light of positive weight; inv_p =
 * total / w_l.  A total that is not > 0 (no positive weight, or an infinite weight's NaN) chooses nothing. */
RT_FILM_HD LightChoice light_connect_choose(float u, uint32_t count, const float *weights) {
    LightChoice c;
    c.l = 0u;
    c.inv_p = 0.0f;
    c.ok = false;
    if (count == 0u) return c;
    if (weights == nullptr) {
        const uint32_t l = (uint32_t)(u * (float)count);
        c.l = l < count - 1u ? l : count - 1u;
        c.inv_p = (float)count;
        c.ok = true;
        return c;
    }
    float total = 0.0f;
    for (uint32_t i = 0; i < count; ++i) total = total + light_connect_weight(weights[i]);
    if (!(total > 0.0f)) return c;
    const float x = u * total;
    float running = 0.0f, chosen_w = 0.0f;
    bool found = false;
    for (uint32_t i = 0; i < count; ++i) {
        const float w = light_connect_weight(weights[i]);
        running = running + w;
        if (!found && w > 0.0f) {
            c.l = i; /* the last positive weight so far: what is left if no running sum exceeds x */
            chosen_w = w;
            c.ok = true;
            found = running > x;
        }
    }
    c.inv_p = total / chosen_w;
    return c;
}

/* what one vertex asks */
struct LightConnection {
    V3 dir;          /* the shadow ray's direction, towards the point drawn; zeros where the path does not ask */
    V3 pending;      /* what the path's radiance gains if the light is not occluded; read only where `ask` */
    float reach;     /* the distance to the point drawn, or -1: a directional light without origin; read only where `ask` */
    uint32_t chosen; /* the absolute index of the light drawn, or RT_LIGHT_CONNECT_NONE */
    bool ask;
};

/* One ALIVE path at a vertex, before rt_path_advance has moved it.  `hit`, the material `m`, `adj_n` and `pos` are light_record's,
 * `view` minus the incoming direction (what get_shade passes as view_direction: light_terms' -view).  `lights` and `aux` are the
 * scene's arrays, indexed by the absolute light index — a different one in every lane, so the device reads them with vector loads.  The
 * record is read, never written.  In this order:
 *   light      light_connect_choose by u_5
 *   point      area_light_sample for RT_FILM_UNIFORM, k = 1, id, light_connect_seed(seed_b) and s: rt_area_light_rays' d_sample
 *   ask        light_asks and approximate_into_directional on the displaced copy must both hold; `last` is no argument
 *   terms      d = get_diffuse * color, sp = get_specular * color: light_terms' operands;
 *              e = (+0 + d * (1 - shiness)) + sp * shiness: rt_light_fold's association for one light into a zeroed rgb
 *   pending    beta * (e * inv_p) per channel, each product rounded once: path_deposit's product
 *   reach      distance(pos, the point) where the light has an origin, -1 where it has none */
template <class Aux>
RT_FILM_HD LightConnection light_connect_record(const rt_path &p, bool hit, const Mat &m, V3 adj_n, V3 pos, V3 view, const rt_light *lights,
                                                const Aux *aux, const LightConnect &q) {
    const uint32_t s = p.bounce >> RT_PATH_SAMPLE_SHIFT, bounces = p.bounce & RT_PATH_BOUNCE_MASK;
    LightConnection c;
    c.dir = c.pending = v3(0.0f, 0.0f, 0.0f);
    c.reach = 0.0f;
    c.chosen = RT_LIGHT_CONNECT_NONE;
    c.ask = false;
    if (!hit) return c;

    const uint32_t seed_b = q.seed + RT_PATH_BOUNCE_STEP * bounces;
    const LightChoice choice = light_connect_choose(light_connect_u(seed_b, p.id, s), q.light_count, q.weights);
    if (!choice.ok) return c;
    const uint32_t li = q.light_first + choice.l;
    c.chosen = li;

    const rt_light L = lights[li];
    const float rad = q.radii != nullptr ? q.radii[choice.l] : 0.0f;
    const V3 sample = area_light_sample(L, li, rad, RT_FILM_UNIFORM, 1u, p.id, light_connect_seed(seed_b), s);
    const rt_light D = area_light_displaced(L, sample);

    V3 l_direction = v3(0.0f, 0.0f, 0.0f);
    if (!light_asks(D, aux[li], pos, adj_n, &l_direction)) return c;
    DirLight dl;
    dl.direction = dl.color = v3(0.0f, 0.0f, 0.0f);
    if (!approximate_into_directional(D, pos, &dl)) return c;

    const V3 light_direction = -dl.direction;
    const V3 d = get_diffuse(m, adj_n, light_direction) * dl.color;
    const V3 sp = get_specular(m, adj_n, view, light_direction) * dl.color;
    const V3 e = v3(0.0f, 0.0f, 0.0f) + d * (1.0f - m.shiness) + sp * m.shiness;
    c.pending = v3(p.beta[0], p.beta[1], p.beta[2]) * (e * choice.inv_p);
    c.reach = area_light_has_origin(L) ? distance(pos, v3(D.origin[0], D.origin[1], D.origin[2])) : -1.0f;
    c.dir = -l_direction; /* towards the point */
    c.ask = true;
    return c;
}

/* a record's word as the float it holds */
RT_FILM_HD float light_connect_f32(uint32_t w) {
    float f;
    __builtin_memcpy(&f, &w, 4);
    return f;
}

/* light_terms' rule for one slot (main.rs:435-448): it is open where it asked, unless its cast found something (kind word <= 1) and
 * the light has no origin (reach negative) or the occluder is nearer than the light.  `shadow_ray`: the slot's own shadow ray as words
 * — its origin is the vertex, which d_hits may no longer hold —; `shadow_hit`: the cast's record as words, or null: nothing occludes.
 * A NaN makes either compare false: lit, as in light_terms. */
RT_FILM_HD bool light_settle_open(unsigned char ask, const uint32_t *shadow_ray, const uint32_t *shadow_hit, float reach) {
    if (ask == 0) return false;
    if (shadow_hit == nullptr || !(shadow_hit[0] <= 1u)) return true;
    if (reach < 0.0f) return false;
    const V3 from = v3(light_connect_f32(shadow_ray[0]), light_connect_f32(shadow_ray[1]), light_connect_f32(shadow_ray[2]));
    const V3 occ = v3(light_connect_f32(shadow_hit[RT_LIGHT_CONNECT_HIT_POSITION]), light_connect_f32(shadow_hit[RT_LIGHT_CONNECT_HIT_POSITION + 1u]),
                      light_connect_f32(shadow_hit[RT_LIGHT_CONNECT_HIT_POSITION + 2u]));
    return !(distance(from, occ) < reach);
}

/* One listed slot: radiance += pending per channel (path_settle's sum) where the slot asked and is open, and the ask byte cleared either
 * way.  Whether the path is still alive is not asked: rt_path_advance may have ended it after it connected. */
RT_FILM_HD void light_settle_record(uint32_t j, unsigned char *asks, const uint32_t *shadow_rays, const uint32_t *shadow_hits, const float *reach,
                                    const float *pending, float *radiance) {
    const unsigned char ask = asks[j];
    asks[j] = 0;
    if (ask == 0) return;
    const bool open = light_settle_open(ask, shadow_rays + (uint64_t)j * RT_LIGHT_CONNECT_RAY_WORDS,
                                        shadow_hits != nullptr ? shadow_hits + (uint64_t)j * RT_LIGHT_CONNECT_HIT_WORDS : nullptr, reach[j]);
    if (!open) return;
    for (uint32_t c = 0; c < 3u; ++c) radiance[3u * (uint64_t)j + c] = radiance[3u * (uint64_t)j + c] + pending[3u * (uint64_t)j + c];
}

} /* namespace rt */

#endif /* RT_LIGHT_CONNECT_H */
