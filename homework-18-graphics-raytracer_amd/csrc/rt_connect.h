/*
 * rt_connect.h — the arithmetic of the connection queries (include/rt_amd.h "connection queries"), written once for the host
 * (librt_host.so: rt_path_connect_cpu / rt_path_settle_cpu / rt_path_weigh_escape_cpu) and the device (rt_connect_query.hip).  Next-event
 * estimation of the sky inside the path loop is three steps on the 32-byte record of rt_path.h, none of which writes it: one direction
 * drawn from the environment's table at the path's vertex, weighed against the vertex's own lobes and multiplied by the throughput
 * before its shadow cast is answered (path_connect_record); the answer added to the path's radiance (path_settle_record); and the sky a
 * lobe-sampled ray found by leaving the scene weighed against the table with the density the record kept (path_escape_weight).
 * Nothing here is a sampler, a density or a Phong term of its own: rt_environment.h's env_sample_of / env_sample_radiance, rt_lobe.h's
 * lobe_surface / lobe_pdf / env_pdf / mis_weight and rt_shade.h's get_diffuse / get_specular are called as rt_environment_rays,
 * rt_lobe_pdf, rt_environment_pdf, rt_mis_weigh and rt_probe_surfaces call them.  Every function is a sequence of single f32 or u32
 * operations in the order the header comment of the block gives; both libraries are built with -ffp-contract=off and the divides are
 * correctly rounded on either side, so the host and the device forms agree bit for bit.
 *
 * The streams.  The connection's two uniforms are film_offset(RT_FILM_UNIFORM, 1, id, environment_seed(seed_b), s, axis) + 0.5 with
 * seed_b = seed + RT_PATH_BOUNCE_STEP * b: environment_seed XORs 0xc2b2ae35 into the seed before the mix and hemisphere_seed, which the
 * lobe's u_0 and u_1 (and through it u_2, u_3 and u_4) come from, XORs 0x85ebca6b — so at one vertex the connection's direction and
 * the lobe's are drawn from two streams of the counter hash, not from one pair of numbers.
 *
 * The escape.  rt_shade_hits writes +0, +0, +0 for a record that is "no hit" (rt_hit_query.hip, shade_hits_kernel: `sum` starts as zeros,
 * only a valid hit's lights add to it, and every record in range is stored), and rt_environment_lookup writes the sky over exactly the
 * records whose kind word is > 1.  So after the two calls the emitted light of such a record is the sky alone, and weighing all of it is
 * weighing the sky.  path_escape_weight takes that rule — the kind word, which needs no scene — not rt_path_advance's: a record with
 * kind <= 1 that names no material ends its path as "no hit" there, but no sky was written for it and its emitted light is zeros.
 */
#ifndef RT_CONNECT_H
#define RT_CONNECT_H

#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_environment.h"
#include "rt_film.h"
#include "rt_hemisphere.h"
#include "rt_lobe.h"
#include "rt_path.h"
#include "rt_shade.h"
#include "rt_vec.h"

namespace rt {

/* the call's own arguments */
struct PathConnect {
    uint32_t seed, heuristic;
    bool last;
};

/* what one vertex asks */
struct Connection {
    V3 dir;     /* the direction drawn; zeros where nothing was drawn */
    V3 pending; /* what the path's radiance gains if the shadow cast finds nothing; read only where `ask` */
    bool ask;
};

/* the limits of normal_kind and heuristic, in that order; null: all in range */
inline const char *connect_limits(uint32_t normal_kind, uint32_t heuristic) {
    if (const char *bad = hemisphere_limits(1u, true, RT_FILM_UNIFORM, normal_kind)) return bad;
    return mis_limits(heuristic);
}

/* One ALIVE path at a vertex, before rt_path_advance has moved it.  The operands are path_advance_record's: `hit`, the material `m`,
 * `shading_n` — the N of the terms —, `sampling_n` — the N of the lobes' density and of "leaves the surface" — and `view`.  The record
 * is read, never written.  In this order:
 *   sample     rt_environment_rays' for spp = 1, RT_FILM_UNIFORM, the path's id and sample s and the bounce's seed; r = texel * scale / pdf
 *   densities  p_env = env_pdf(dir), p_lobe = lobe_pdf(dir) on path_advance_record's surface
 *   weight     w = mis_weight(heuristic, 1, p_env, 1, p_lobe); r = r * w per channel, as mis_weigh_entry multiplies an rgb
 *   throughput t = beta * r per channel
 *   terms      pending = (+0 + (diffuse * t) * (1 - shiness)) + (specular * t) * shiness: env_fold_record's association for one sample
 *              into a zeroed rgb, as path_advance_record restates it
 * It asks where rt_environment_rays asks (a hit, a table with light, a finite density > 0, a direction that leaves the surface) and w is
 * finite; `last`, a record that is no hit and a table without light ask nothing and draw nothing.  A lane that does not ask still walks
 * through lobe_pdf with live = false, so that its wave-level branch sees every lane that got here. */
RT_FILM_HD Connection path_connect_record(const rt_path &p, bool hit, const Mat &m, V3 shading_n, V3 sampling_n, V3 view, const rt_environment &e,
                                          const EnvTable &t, const PathConnect &q) {
    const uint32_t s = p.bounce >> RT_PATH_SAMPLE_SHIFT, bounces = p.bounce & RT_PATH_BOUNCE_MASK;
    Connection c;
    c.dir = c.pending = v3(0.0f, 0.0f, 0.0f);
    c.ask = false;
    const bool draws = hit && !q.last && t.total > 0u;

    V3 r = v3(0.0f, 0.0f, 0.0f);
    float p_env = 0.0f;
    bool need = false;
    if (draws) {
        const EnvSample d = env_sample_of(e, t, RT_FILM_UNIFORM, 1u, p.id, environment_seed(q.seed + RT_PATH_BOUNCE_STEP * bounces), s);
        c.dir = d.dir;
        need = d.ok && hemisphere_asks(d.dir, sampling_n);
        if (need) {
            uint32_t at;
            r = env_sample_radiance(e, d);
            p_env = env_pdf(e, t, d.dir, &at);
        }
    }
    const LobeSurface surface = lobe_surface(sampling_n, view, m.shiness, m.smoothness);
    const float p_lobe = lobe_pdf(surface, c.dir, need);
    if (!need) return c;

    const float w = mis_weight(q.heuristic, 1.0f, p_env, false, 1.0f, p_lobe);
    if (!env_finite(w)) return c;
    r = r * w;
    const V3 tt = v3(p.beta[0], p.beta[1], p.beta[2]) * r;
    const V3 diffuse = get_diffuse(m, shading_n, c.dir);
    const V3 specular = get_specular(m, shading_n, view, c.dir);
    c.pending = v3(0.0f, 0.0f, 0.0f) + (diffuse * tt) * (1.0f - m.shiness) + (specular * tt) * m.shiness;
    c.ask = true;
    return c;
}

/* env_fold_record's rule for one sample: it is open where it asked and its cast found nothing at all — the sky is infinitely far, so
 * whatever was hit occludes; `shadow_hit`: the cast's rt_hit record as words, read only where it asked, or null: nothing occludes */
RT_FILM_HD bool path_settle_open(unsigned char ask, const uint32_t *shadow_hit) {
    bool open = ask != 0;
    if (open && shadow_hit != nullptr && shadow_hit[0] <= 1u) open = false; /* Some(occlusion) */
    return open;
}

/* one channel of the settlement: the sum alone — the product with the throughput was rounded when the connection was made */
RT_FILM_HD float path_settle(float radiance, float pending) { return radiance + pending; }

/* One listed slot: radiance += pending per channel where the slot asked and its cast is open, and the ask byte cleared either way — so
 * that the flags are all 0 again for the next bounce's rt_path_connect, which writes the listed live slots alone.  Whether the path is
 * still alive is not asked: rt_path_advance may have ended it after it connected, and the connection counts all the same. */
RT_FILM_HD void path_settle_record(uint32_t j, unsigned char *asks, const uint32_t *shadow_hits, const float *pending, float *radiance) {
    const bool open = path_settle_open(asks[j], shadow_hits != nullptr ? shadow_hits + (uint64_t)j * RT_ENV_HIT_WORDS : nullptr);
    asks[j] = 0;
    if (!open) return;
    for (uint32_t c = 0; c < 3u; ++c) radiance[3u * (uint64_t)j + c] = path_settle(radiance[3u * (uint64_t)j + c], pending[3u * (uint64_t)j + c]);
}

/* Does the escape of a path get a weight?  An ALIVE path whose vertex is "no hit" by rt_environment_lookup's rule (kind word > 1: the
 * records that call wrote the sky for), whose last direction was drawn from a density — pdf finite and > 0; +0 is a camera ray or a ray
 * that left glass, delta events no connection could have made — under a table that has light (none: no connection was made either). */
RT_FILM_HD bool path_escape_weighed(uint32_t flags, uint32_t kind, float pdf, const EnvTable &t) {
    return (flags & RT_PATH_ALIVE) != 0u && kind > 1u && env_finite(pdf) && pdf > 0.0f && t.total > 0u;
}

/* ... and the weight: the lobe's sample against the one connection that could have found the same direction */
RT_FILM_HD float path_escape_weight(const rt_environment &e, const EnvTable &t, uint32_t heuristic, float pdf, V3 incoming_dir) {
    uint32_t at;
    return mis_weight(heuristic, 1.0f, pdf, false, 1.0f, env_pdf(e, t, incoming_dir, &at));
}

} /* namespace rt */

#endif /* RT_CONNECT_H */
