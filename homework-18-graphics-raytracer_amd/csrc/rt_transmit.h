/*
 * rt_transmit.h — the arithmetic of the transmission queries (include/rt_amd.h "transmission queries"), written once for the host
 * (librt_host.so: rt_path_branch_cpu / rt_path_transmit_cpu) and the device (rt_transmit_query.hip).  A path at a vertex of a
 * transparent material either goes off the vertex's lobes (rt_path_advance, unchanged) or through the glass: the choice is one uniform
 * of the counter hash against the material's transparency, the walk through the glass is the refraction queries' (its entry is
 * rt_refract_entry.h's, shared with rt_refract_enter), and the fold of a finished walk into the 32-byte record is the decay
 * opaque_decay.powf(travel_distance) (main.rs:508) on the throughput and then rt_path.h's own tail, path_step_tail, not restated.
 * Every function is a sequence of single f32 or u32 operations in the order the header comment of the block gives; both libraries are
 * built with -ffp-contract=off, so the host and the device forms agree bit for bit.
 */
#ifndef RT_TRANSMIT_H
#define RT_TRANSMIT_H

#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_detmath.h"
#include "rt_path.h"
#include "rt_refract_entry.h"

namespace rt {

#define RT_PATH_TRANSMIT_STREAM 0x85ebca6bu /* u_4's stream: film_mix(seed_h ^ RT_PATH_TRANSMIT_STREAM), apart from u_0 .. u_3's */

/* the choice: u_4 < transparency, so 0 never transmits, 1 and above always, a NaN never; a record that is no hit takes the lobes */
RT_FILM_HD bool path_transmits(uint32_t id, uint32_t bounce_word, uint32_t seed, bool hit, float transparency) {
    const uint32_t s = bounce_word >> RT_PATH_SAMPLE_SHIFT, bounces = bounce_word & RT_PATH_BOUNCE_MASK;
    const uint32_t seed_h = hemisphere_seed(seed + RT_PATH_BOUNCE_STEP * bounces);
    const float u4 = film_u(id, film_mix(seed_h ^ RT_PATH_TRANSMIT_STREAM), s, 0u);
    return hit && u4 < transparency;
}

/* opaque_decay.powf(travel_distance), main.rs:508, where the walk escaped, +0 elsewhere.  rtdm::powf works in binary64: on the device a
 * wave none of whose lanes escaped skips it, as lobe_pdf skips its power. */
RT_FILM_HD float transmit_decay(bool escaped, float opaque_decay, float travel) {
    float w = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
    if (__builtin_amdgcn_ballot_w64(escaped) != 0ull) w = escaped ? rtdm::powf(opaque_decay, travel) : 0.0f;
#else
    if (escaped) w = rtdm::powf(opaque_decay, travel);
#endif
    return w;
}

/* One ALIVE path whose walk is over: `kind` is the walk's d_kind word — validated, never indexed with — `hit` whether the vertex is a
 * hit by the hit queries' rules, `opaque_decay` its material's, `travel` the walk's d_travel.  The record `p` is advanced in place.
 * Returns whether the path lives on: only an Escaped walk (kind 0) of a hit does; everything else — Infinite, Trapped, no hit, a walk
 * still RT_REFR_WALKING, any other word — ends it with RT_PATH_TRAPPED.  `q.last` is not read: rt_path_branch ends those paths. */
RT_FILM_HD bool path_transmit_record(rt_path &p, uint32_t kind, bool hit, float opaque_decay, float travel, const PathStep &q) {
    const uint32_t s = p.bounce >> RT_PATH_SAMPLE_SHIFT, bounces = p.bounce & RT_PATH_BOUNCE_MASK;
    const bool escaped = hit && kind == 0u;
    const float w = transmit_decay(escaped, opaque_decay, travel);
    if (!escaped) {
        p.flags = RT_PATH_TRAPPED;
        return false;
    }
    V3 next = v3(p.beta[0] * w, p.beta[1] * w, p.beta[2] * w);
    const uint32_t seed_h = hemisphere_seed(q.seed + RT_PATH_BOUNCE_STEP * bounces);
    if (const uint32_t ended = path_step_tail(&next, true, p.id, s, bounces, seed_h, q)) {
        p.flags = ended;
        return false;
    }
    p.beta[0] = next.x;
    p.beta[1] = next.y;
    p.beta[2] = next.z;
    p.pdf = 0.0f; /* a delta event no other strategy could have drawn, as before the first bounce */
    p.bounce = path_bounce_word(s, bounces + 1u);
    p.flags = RT_PATH_ALIVE | RT_PATH_TRANSMITTED;
    return true;
}

} /* namespace rt */

#endif /* RT_TRANSMIT_H */
