/*
 * rt_lobe.h — the arithmetic of the lobe queries (include/rt_amd.h "lobe queries"), written once for the host (librt_host.so:
 * rt_lobe_samples_cpu / rt_lobe_pdf_cpu / rt_environment_pdf_cpu / rt_mis_weigh_cpu) and the device (rt_lobe_query.hip).  A surface's
 * Phong mixture is a diffuse lobe about its normal N, rt_hemisphere.h's cosine sampler, and a specular lobe about R, the mirror of the
 * view: get_specular's `reflected` with the view in the place of the light, so that specular(dir) / pdf(dir) is constant over the
 * lobe.  `shiness`, clamped to [0, 1], chooses between the two.  The density of a direction is one function, lobe_pdf, which the sampler
 * evaluates at the direction it produced; the density under an environment's table runs env_texel_point, the lookup's own map, and reads
 * the texel's quantum; the weight of multiple importance sampling is two products, a sum and a quotient.  Every function is a sequence
 * of single f32, u32 or f64 operations in the order the header comment of the block gives; both libraries are built with
 * -ffp-contract=off and sqrt and the divides are correctly rounded on either side, so the host and the device forms agree bit for bit.
 */
#ifndef RT_LOBE_H
#define RT_LOBE_H

#include <math.h>
#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_detmath.h"
#include "rt_environment.h"
#include "rt_film.h"
#include "rt_hemisphere.h"
#include "rt_shade.h"
#include "rt_vec.h"

namespace rt {

#define RT_LOBE_SELECT 0x27d4eb2fu /* u_2's stream: film_mix(seed_h ^ RT_LOBE_SELECT), apart from u_0's and u_1's */

/* what a record's samples share */
struct LobeSurface {
    V3 n, r;       /* the normal, and R = 2 * dot(V, N) * N - V */
    float e, p_s;  /* get_specular's exponent 1 / (smoothness + RT_F_EPSILON); shiness clamped to [0, 1], NaN read as 0 */
};

RT_FILM_HD LobeSurface lobe_surface(V3 n, V3 view, float shiness, float smoothness) {
    LobeSurface l;
    l.n = n;
    l.r = 2.0f * dot(view, n) * n - view; /* get_specular's `reflected` (materials.rs:59) with V in the place of light_direction */
    l.e = 1.0f / (smoothness + RT_F_EPSILON);
    l.p_s = shiness > 0.0f ? (shiness < 1.0f ? shiness : 1.0f) : 0.0f;
    return l;
}

/* max(x, 0) as get_specular writes it: NaN -> 0 */
RT_FILM_HD float lobe_positive(float x) { return x > 0.0f ? x : 0.0f; }

/* the mixture density of `dir`, per solid angle:
 *     d   = ((1 - p_s) * max(dot(dir, N), 0)) * 0.31830987f                          1 / pi
 *     s   = ((p_s * (e + 1)) * 0.15915494f) * powf(max(dot(dir, R), 0), e)           1 / (2 pi)
 *     pdf = d + s
 * The power is get_specular's: +0 where pow_underflows_to_zero says so, and on the device a wave none of whose lanes needs the binary64
 * evaluation branches around it.  `live`: the lane has a direction (the others only keep the wave's branch uniform). */
RT_FILM_HD float lobe_pdf(const LobeSurface &l, V3 dir, bool live) {
    const float cos_n = lobe_positive(dot(dir, l.n));
    const float cos_r = lobe_positive(dot(dir, l.r));
    float power = 0.0f;
    const bool zero = !live || pow_underflows_to_zero(cos_r, l.e);
#if defined(__HIP_DEVICE_COMPILE__)
    if (__builtin_amdgcn_ballot_w64(!zero) != 0ull) power = zero ? 0.0f : rtdm::powf(cos_r, l.e);
#else
    if (!zero) power = rtdm::powf(cos_r, l.e);
#endif
    const float d = ((1.0f - l.p_s) * cos_n) * 0.31830987f;
    const float s = ((l.p_s * (l.e + 1.0f)) * 0.15915494f) * power;
    return d + s;
}

struct LobeSample {
    V3 dir;
    float pdf;
    bool specular; /* drawn from lobe 1 */
    bool ok;       /* pdf finite and > 0, and the direction leaves the surface */
};

/* sample s of record `id`; k: film_strata(spp) (used by RT_FILM_STRATIFIED only); seed_h: hemisphere_seed(seed) — u_0 and u_1 are
 * rt_hemisphere_rays' own, so a surface of shiness 0 draws that call's directions.  u_2 = film_u(id, film_mix(seed_h ^
 * RT_LOBE_SELECT), s, 0), never stratified, chooses the lobe: specular where u_2 < p_s.  Lobe 0 is hemisphere_dir about N.  Lobe 1:
 *     c = powf(u_0, 1 / (e + 1));  r = sqrt(max(1 - c * c, 0));  phi = 6.2831855f * u_1
 *     dir = adjust_normal((r * cos phi, r * sin phi, c), R)
 * — a density proportional to cos^e about R.  The pdf is lobe_pdf of the produced direction, not a function of c. */
RT_FILM_HD LobeSample lobe_sample(const LobeSurface &l, uint32_t pattern, uint32_t k, uint32_t id, uint32_t seed_h, uint32_t s, bool live) {
    LobeSample p;
    p.dir = v3(0.0f, 0.0f, 0.0f);
    p.specular = false;
    if (live) {
        const float u2 = film_u(id, film_mix(seed_h ^ RT_LOBE_SELECT), s, 0u);
        p.specular = u2 < l.p_s;
        if (p.specular) {
            const float u0 = film_offset(pattern, k, id, seed_h, s, 0u) + 0.5f;
            const float u1 = film_offset(pattern, k, id, seed_h, s, 1u) + 0.5f;
            const float c = rtdm::powf(u0, 1.0f / (l.e + 1.0f));
            const float r = rtdm::f_sqrt(fmaxf(1.0f - c * c, 0.0f));
            const float phi = 6.2831855f * u1;
            float sine, cosine;
            rtdm::sincosf(phi, &sine, &cosine);
            p.dir = adjust_normal(v3(r * cosine, r * sine, c), l.r);
        } else {
            p.dir = hemisphere_dir(pattern, k, id, seed_h, s, l.n);
        }
    }
    p.pdf = lobe_pdf(l, p.dir, live);
    p.ok = live && env_finite(p.pdf) && p.pdf > 0.0f && hemisphere_asks(p.dir, l.n);
    return p;
}

/* ---- the density under an environment's table ---- */

/* dir -> the texel the lookup's own map names (x = min((uint32)x_f, W - 1), y likewise) and
 *     pdf = (float)((double)q / (double)total) * (float)(W * H) / (19.739209f * sinf(theta))      q = C[y][x] - C[y][x - 1]
 * with the theta of that map, acosf of the normalised direction's y.  +0 for a zero or non-finite direction, a table that is not this
 * environment's or is empty (total == 0), and a pdf that is not finite.  The two loads are addressed by x and y
 * alone, which the image's size bounds: whatever the table holds, they stay inside it.  *at: y * W + x, 0 where no texel is named. */
RT_FILM_HD float env_pdf(const rt_environment &e, const EnvTable &t, V3 dir, uint32_t *at) {
    *at = 0u;
    float x_f, y_f, theta;
    if (t.total == 0u || !env_texel_point(e, dir, &x_f, &y_f, &theta)) return 0.0f;
    const uint32_t xi = (uint32_t)x_f, yi = (uint32_t)y_f;
    const uint32_t x = xi < e.width - 1u ? xi : e.width - 1u, y = yi < e.height - 1u ? yi : e.height - 1u;
    *at = y * e.width + x;
    const uint32_t *const row = t.rows + (uint64_t)y * e.width;
    const uint32_t q = row[x] - (x > 0u ? row[x - 1u] : 0u);
    const float pdf = (float)((double)q / (double)t.total) * (float)(e.width * e.height) / (19.739209f * rtdm::sinf(theta));
    return env_finite(pdf) ? pdf : 0.0f;
}

/* ---- multiple importance sampling ---- */

/* the weight of a sample drawn by its own strategy (n_own samples of density pdf_own) against another (n_other of pdf_other):
 *     a = (float)n_own * pdf_own;  b = (float)n_other * pdf_other
 *     RT_MIS_BALANCE  w = a / (a + b)            RT_MIS_POWER  w = (a * a) / (a * a + b * b)
 * a not finite or <= 0 gives +0.  `alone` (no other strategy: a null pdf_other or n_other == 0): w = 1 without any arithmetic. */
RT_FILM_HD float mis_weight(uint32_t heuristic, float n_own, float pdf_own, bool alone, float n_other, float pdf_other) {
    const float a = n_own * pdf_own;
    if (!env_finite(a) || !(a > 0.0f)) return 0.0f;
    if (alone) return 1.0f;
    const float b = n_other * pdf_other;
    if (heuristic == RT_MIS_POWER) {
        const float aa = a * a;
        return aa / (aa + b * b);
    }
    return a / (a + b);
}

/* one weighing call */
struct MisWeigh {
    uint64_t count;
    const float *pdf_own, *pdf_other; /* pdf_other null: no other strategy */
    float n_own, n_other;
    uint32_t heuristic;
    bool alone, divide_by_own;
    float *weight, *rgb;              /* either may be null */
};

/* entry k: weight[k] = w; rgb[3k ..] *= w, or with divide_by_own *= (w / pdf_own) — a w of 0 multiplies by +0 either way, so a density
 * of 0 divides nothing.  Alone and not dividing, an entry whose w is 1 keeps rgb's bits: no multiply at all. */
RT_FILM_HD void mis_weigh_entry(const MisWeigh &m, uint64_t k) {
    const float own = m.pdf_own[k];
    const float w = mis_weight(m.heuristic, m.n_own, own, m.alone, m.n_other, m.alone ? 0.0f : m.pdf_other[k]);
    if (m.weight != nullptr) m.weight[k] = w;
    if (m.rgb == nullptr) return;
    if (m.alone && !m.divide_by_own && w == 1.0f) return;
    const float f = m.divide_by_own && w != 0.0f ? w / own : w;
    m.rgb[k * 3u] = m.rgb[k * 3u] * f;
    m.rgb[k * 3u + 1u] = m.rgb[k * 3u + 1u] * f;
    m.rgb[k * 3u + 2u] = m.rgb[k * 3u + 2u] * f;
}

inline MisWeigh mis_weigh_call(uint64_t count, const float *pdf_own, uint32_t n_own, const float *pdf_other, uint32_t n_other, uint32_t heuristic,
                               bool divide_by_own, float *weight, float *rgb) {
    const bool alone = pdf_other == nullptr || n_other == 0u;
    return {count, pdf_own, pdf_other, (float)n_own, (float)n_other, heuristic, alone, divide_by_own, weight, rgb};
}

/* the limits of the weighing call's own arguments; null: all in range */
inline const char *mis_limits(uint32_t heuristic) {
    if (heuristic != RT_MIS_BALANCE && heuristic != RT_MIS_POWER) return "unknown heuristic (RT_MIS_BALANCE or RT_MIS_POWER)";
    return nullptr;
}

/* rt_lobe_pdf's normal_kind: a surface record carries the shading normal alone */
inline const char *lobe_pdf_limits(uint32_t normal_kind) {
    if (normal_kind == RT_HEMISPHERE_GEOMETRIC) return "RT_HEMISPHERE_GEOMETRIC is no normal_kind of a surface record (it carries no geometric normal)";
    return hemisphere_limits(1u, true, RT_FILM_UNIFORM, normal_kind);
}

} /* namespace rt */

#endif /* RT_LOBE_H */
