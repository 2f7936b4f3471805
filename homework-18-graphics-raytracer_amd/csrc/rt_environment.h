/*
 * rt_environment.h — the arithmetic of the environment queries (include/rt_amd.h "environment queries"), written once for the host
 * (librt_host.so: rt_environment_lookup_cpu / _table_cpu / _samples_cpu / _fold_cpu) and the device (rt_environment_query.hip).  The
 * environment is a lat-long image, row 0 at the zenith, y up: texel-space point (x_f, y_f) lies in the direction
 *     theta = 3.1415927f * y_f / (float)H      phi = 6.2831855f * x_f / (float)W + rotation      dir = (sin theta cos phi, cos theta, sin theta sin phi)
 * The lookup runs that map backwards with rtdm::acosf / rtdm::atan2f on the normalised direction; the sampling table is integer — a
 * quantised luma * sin(theta) per texel, summed along each row and down the rows — so any scan order gives its bits; a sample is a row
 * and a column by inverse CDF in u64 / f64 and a point inside that texel.  Every function is a sequence of single f32, u32, u64 or f64
 * operations in the order the header comment of the block gives; both libraries are built with -ffp-contract=off and sqrt and the
 * divides are correctly rounded on either side, so the host and the device forms agree bit for bit.
 */
#ifndef RT_ENVIRONMENT_H
#define RT_ENVIRONMENT_H

#include <math.h>
#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_detmath.h"
#include "rt_film.h"
#include "rt_hemisphere.h" /* hemisphere_limits, hemisphere_asks: the limits of spp, pattern and normal_kind with their texts, and the test "leaves the surface" */
#include "rt_vec.h"

namespace rt {

#define RT_ENV_HIT_WORDS 13u    /* an rt_hit in words */
#define RT_ENV_RAY_WORDS 11u    /* an rt_ray in words */
#define RT_ENV_RAY_DIRECTION 3u /* word of rt_ray.direction */
#define RT_ENV_NO_PARENT 0xffffffffu

/* the table: a header, the inclusive marginal M[y] (u64) and the inclusive rows C[y][x] (u32) */
#define RT_ENV_TABLE_HEADER_BYTES 24u
#define RT_ENV_TABLE_WIDTH 0u  /* header words: width, height, */
#define RT_ENV_TABLE_HEIGHT 1u
#define RT_ENV_TABLE_TOTAL 2u  /* total (u64, words 2 and 3), */
#define RT_ENV_TABLE_W_MAX 4u  /* the bits of w_max, and a word that is 0 */
#define RT_ENV_Q_STEPS 65534.0f

/* the environment's sampling stream, apart from the hemispheres' (hemisphere_seed) and the area lights' (area_light_seed) */
RT_FILM_HD uint32_t environment_seed(uint32_t seed) { return film_mix(seed ^ 0xc2b2ae35u); }

RT_FILM_HD bool env_finite(float x) { return (rtdm::f32_bits(x) & 0x7f800000u) != 0x7f800000u; }

RT_FILM_HD V3 env_texel(const rt_environment &e, uint32_t x, uint32_t y) { return v3p(e.d_texels + ((uint64_t)y * e.width + x) * 3u); }

/* ---- the lookup ---- */

/* dir -> (x_f, y_f) in [0, W] x [0, H]; false: a zero or non-finite direction.  d = dir / |dir|, theta = acosf(clamp(d.y)),
 * phi = atan2f(d.z, d.x) - rotation, x_f = phi * W / 6.2831855f wrapped into one turn by x_f - floorf(x_f / W) * W, y_f = theta * H /
 * 3.1415927f; both are then clamped to their range (a NaN, from a rotation that is not finite, becomes 0) */
RT_FILM_HD bool env_texel_point(const rt_environment &e, V3 dir, float *x_f, float *y_f, float *theta_out) {
    const float len = magnitude(dir);
    if (!(len > 0.0f) || !env_finite(len)) return false;
    const V3 d = dir / len;
    const float w = (float)e.width, h = (float)e.height;
    const float theta = rtdm::acosf(fminf(fmaxf(d.y, -1.0f), 1.0f));
    const float phi = rtdm::atan2f(d.z, d.x) - e.rotation;
    float x = phi * w / 6.2831855f;
    x = x - floorf(x / w) * w;
    *x_f = fminf(fmaxf(x, 0.0f), w);
    *y_f = fminf(fmaxf(theta * h / 3.1415927f, 0.0f), h);
    *theta_out = theta;
    return true;
}
RT_FILM_HD bool env_texel_point(const rt_environment &e, V3 dir, float *x_f, float *y_f) {
    float theta; /* the lobe queries' density reads it (rt_lobe.h) */
    return env_texel_point(e, dir, x_f, y_f, &theta);
}

/* a * (1 - t) + b * t, per channel */
RT_FILM_HD V3 env_mix(V3 a, V3 b, float t) { return a * (1.0f - t) + b * t; }

/* texel(dir) * scale.  Nearest: x = min((uint32)x_f, W - 1), likewise y.  Bilinear: texel centres at + 0.5, so xs = x_f - 0.5f,
 * x0 = floorf(xs), fx = xs - x0, columns x0 and x0 + 1 wrapped; ys, y0 and fy likewise, rows y0 and y0 + 1 clamped; the two rows are
 * mixed along x first, then the results along y.  NaN and Inf texels pass through the arithmetic. */
RT_FILM_HD V3 env_lookup(const rt_environment &e, V3 dir) {
    float x_f, y_f;
    if (!env_texel_point(e, dir, &x_f, &y_f)) return v3(0.0f, 0.0f, 0.0f);
    const uint32_t w = e.width, h = e.height;
    if (e.filter != RT_ENV_BILINEAR) {
        const uint32_t x = (uint32_t)x_f, y = (uint32_t)y_f;
        return env_texel(e, x < w - 1u ? x : w - 1u, y < h - 1u ? y : h - 1u) * e.scale;
    }
    const float xs = x_f - 0.5f, ys = y_f - 0.5f;
    const float x0f = floorf(xs), y0f = floorf(ys);
    const float fx = xs - x0f, fy = ys - y0f;
    const int32_t xi = (int32_t)x0f, yi = (int32_t)y0f; /* -1 .. W, -1 .. H */
    const uint32_t x0 = xi < 0 ? w - 1u : ((uint32_t)xi >= w ? (uint32_t)xi - w : (uint32_t)xi);
    const uint32_t x1 = x0 + 1u >= w ? 0u : x0 + 1u;
    const uint32_t y0 = yi < 0 ? 0u : ((uint32_t)yi > h - 1u ? h - 1u : (uint32_t)yi);
    const uint32_t y1 = yi + 1 < 0 ? 0u : ((uint32_t)(yi + 1) > h - 1u ? h - 1u : (uint32_t)(yi + 1));
    const V3 top = env_mix(env_texel(e, x0, y0), env_texel(e, x1, y0), fx);
    const V3 bottom = env_mix(env_texel(e, x0, y1), env_texel(e, x1, y1), fx);
    return env_mix(top, bottom, fy) * e.scale;
}

/* one lookup call */
struct EnvLookup {
    rt_environment env;
    const uint32_t *rays;   /* rt_ray records as words */
    uint64_t n;
    const uint32_t *count;  /* null: n */
    const uint32_t *hits;   /* rt_hit records as words; null: every record is written */
    const uint32_t *parent; /* null: record j writes slot j */
    float *out;
    uint64_t n_out;
};

/* record j of a lookup, j below the live count: a record that is a hit (kind <= 1) is left alone; the value goes to slot parent[j], or
 * j, when that lies below n_out — rt_tree_fold's addressing */
RT_FILM_HD void env_lookup_record(const EnvLookup &a, uint64_t j) {
    if (a.hits != nullptr && a.hits[j * RT_ENV_HIT_WORDS] <= 1u) return;
    const uint64_t slot = a.parent != nullptr ? (uint64_t)a.parent[j] : j;
    if (slot >= a.n_out) return;
    const uint32_t *const r = a.rays + j * RT_ENV_RAY_WORDS + RT_ENV_RAY_DIRECTION;
    const V3 value = env_lookup(a.env, v3(rtdm::f32_from_bits(r[0]), rtdm::f32_from_bits(r[1]), rtdm::f32_from_bits(r[2])));
    a.out[slot * 3u] = value.x;
    a.out[slot * 3u + 1u] = value.y;
    a.out[slot * 3u + 2u] = value.z;
}

/* ---- the table ---- */

inline uint64_t env_table_bytes(uint32_t width, uint32_t height) {
    return (uint64_t)RT_ENV_TABLE_HEADER_BYTES + 8u * (uint64_t)height + 4u * (uint64_t)width * height;
}
RT_FILM_HD uint64_t *env_table_marginal(void *table) { return reinterpret_cast<uint64_t *>(static_cast<unsigned char *>(table) + RT_ENV_TABLE_HEADER_BYTES); }
RT_FILM_HD uint32_t *env_table_rows(void *table, uint32_t height) { return reinterpret_cast<uint32_t *>(env_table_marginal(table) + height); }

RT_FILM_HD float env_sin_row(uint32_t y, uint32_t height) { return rtdm::sinf(3.1415927f * ((float)y + 0.5f) / (float)height); }

/* w = luma(rgb) * sin_row, the luma (r * l0 + g * l1) + b * l2 with rt_luma.h's weights; *usable: the three channels and w are finite
 * and w > 0 */
RT_FILM_HD float env_weight(const rt_environment &e, uint32_t x, uint32_t y, float sin_row, float l0, float l1, float l2, bool *usable) {
    const V3 t = env_texel(e, x, y);
    const float w = ((t.x * l0 + t.y * l1) + t.z * l2) * sin_row;
    *usable = env_finite(t.x) && env_finite(t.y) && env_finite(t.z) && env_finite(w) && w > 0.0f;
    return w;
}

/* 1 .. 65535 for a usable texel — whatever carries light can be sampled — and 0 for every other */
RT_FILM_HD uint32_t env_quantum(float w, bool usable, float w_max) { return usable ? 1u + (uint32_t)(w / w_max * RT_ENV_Q_STEPS) : 0u; }

/* the limits of an environment and the messages, for the device calls and the CPU forms; null: all in range.  *unsupported: the
 * refusal is RT_ERR_UNSUPPORTED (an image beyond what row sums in u32 allow) */
inline const char *environment_limits(const rt_environment *env, bool *unsupported) {
    *unsupported = false;
    if (env == nullptr) return "null environment";
    if (env->d_texels == nullptr) return "null environment texels";
    if (env->width == 0u || env->height == 0u) return "an environment of width or height 0";
    if (env->width > RT_ENV_MAX_WIDTH || env->height > RT_ENV_MAX_HEIGHT || (uint64_t)env->width * env->height >= (1ull << 27)) {
        *unsupported = true;
        return "an environment wider than 16384, higher than 8192 or of 2^27 texels or more";
    }
    if (env->filter != RT_ENV_NEAREST && env->filter != RT_ENV_BILINEAR) return "unknown filter (RT_ENV_NEAREST or RT_ENV_BILINEAR)";
    return nullptr;
}

/* ---- the sampler ---- */

/* a table as the sampler reads it: the total is 0 — nothing asks — unless the header names this environment's size */
struct EnvTable {
    const uint64_t *marginal;
    const uint32_t *rows;
    uint64_t total;
};
RT_FILM_HD EnvTable env_table_view(const rt_environment &e, const void *table) {
    const uint32_t *const header = static_cast<const uint32_t *>(table);
    EnvTable t;
    t.marginal = reinterpret_cast<const uint64_t *>(static_cast<const unsigned char *>(table) + RT_ENV_TABLE_HEADER_BYTES);
    t.rows = reinterpret_cast<const uint32_t *>(t.marginal + e.height);
    t.total = header[RT_ENV_TABLE_WIDTH] == e.width && header[RT_ENV_TABLE_HEIGHT] == e.height
                  ? ((uint64_t)header[RT_ENV_TABLE_TOTAL + 1u] << 32) | header[RT_ENV_TABLE_TOTAL]
                  : 0u;
    return t;
}

struct EnvSample {
    V3 dir;
    float pdf;     /* per solid angle */
    uint32_t x, y; /* the texel */
    bool ok;       /* total > 0, and pdf finite and > 0 */
};

/* (u0, u1) -> a texel and a point in it.  Row: a = (double)u0 * (double)total, t = min((uint64)a, total - 1), y the first row with
 * M[y] > t, fy = (float)((a - M[y - 1]) / rowsum) kept below 1.  Column, on the row's own sums: b = (double)u1 * (double)rowsum,
 * tx = min((uint64)b, rowsum - 1), x the first with C[y][x] > tx, fx = (float)((b - C[y][x - 1]) / q) kept below 1.  Then
 * (x_f, y_f) = ((float)x + fx, (float)y + fy), the direction of that point, and
 *     pdf = (float)((double)q / (double)total) * (float)(W * H) / (19.739209f * sin theta)
 * Both searches stay inside their arrays whatever the table holds; a row or a texel of weight 0 (a table that is not this
 * environment's) gives ok = false. */
RT_FILM_HD EnvSample env_sample(const rt_environment &e, const EnvTable &t, float u0, float u1) {
    EnvSample s;
    s.dir = v3(0.0f, 0.0f, 0.0f);
    s.pdf = 0.0f;
    s.x = s.y = 0u;
    s.ok = false;
    if (t.total == 0u) return s;
    const double a = (double)u0 * (double)t.total;
    const uint64_t at = (uint64_t)a;
    const uint64_t ty = at < t.total - 1u ? at : t.total - 1u;
    uint32_t lo = 0u, hi = e.height - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (t.marginal[mid] > ty) hi = mid; else lo = mid + 1u;
    }
    const uint32_t y = lo;
    const uint64_t above = y > 0u ? t.marginal[y - 1u] : 0u;
    const uint64_t rowsum = t.marginal[y] - above;
    s.y = y;
    if (rowsum == 0u || t.marginal[y] < above) return s;
    const float fy = fminf((float)((a - (double)above) / (double)rowsum), 0.99999994f);
    const uint32_t *const row = t.rows + (uint64_t)y * e.width;
    const double b = (double)u1 * (double)rowsum;
    const uint64_t bt = (uint64_t)b;
    const uint64_t tx = bt < rowsum - 1u ? bt : rowsum - 1u;
    lo = 0u;
    hi = e.width - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint64_t)row[mid] > tx) hi = mid; else lo = mid + 1u;
    }
    const uint32_t x = lo;
    const uint32_t left = x > 0u ? row[x - 1u] : 0u;
    const uint32_t q = row[x] - left;
    s.x = x;
    if (q == 0u || row[x] < left) return s;
    const float fx = fminf((float)((b - (double)left) / (double)q), 0.99999994f);
    const float x_f = (float)x + fx, y_f = (float)y + fy;
    const float theta = 3.1415927f * y_f / (float)e.height;
    const float phi = 6.2831855f * x_f / (float)e.width + e.rotation;
    float sin_t, cos_t, sin_p, cos_p;
    rtdm::sincosf(theta, &sin_t, &cos_t);
    rtdm::sincosf(phi, &sin_p, &cos_p);
    s.dir = v3(sin_t * cos_p, cos_t, sin_t * sin_p);
    s.pdf = (float)((double)q / (double)t.total) * (float)(e.width * e.height) / (19.739209f * sin_t);
    s.ok = env_finite(s.pdf) && s.pdf > 0.0f;
    return s;
}

/* sample s of record `id`; k: film_strata(spp) (used by RT_FILM_STRATIFIED only) */
RT_FILM_HD EnvSample env_sample_of(const rt_environment &e, const EnvTable &t, uint32_t pattern, uint32_t k, uint32_t id, uint32_t seed_e, uint32_t s) {
    const float u0 = film_offset(pattern, k, id, seed_e, s, 0u) + 0.5f;
    const float u1 = film_offset(pattern, k, id, seed_e, s, 1u) + 0.5f;
    return env_sample(e, t, u0, u1);
}

/* texel(x, y) * scale / pdf: the sampled texel itself, whatever the filter */
RT_FILM_HD V3 env_sample_radiance(const rt_environment &e, const EnvSample &s) { return env_texel(e, s.x, s.y) * e.scale / s.pdf; }

/* ---- the fold ---- */

/* one fold call: sample-major arrays of spp * n entries, entry s * n + i */
struct EnvFold {
    uint64_t n;
    uint32_t spp;
    const unsigned char *asks;
    const uint32_t *shadow_hits; /* rt_hit records as words; null: nothing occludes */
    const float *radiance, *diffuse, *specular;
    unsigned char *open;         /* may be null */
    float *rgb;
};

/* Record i of a fold; valid: the record is a hit, shiness its material's.  Samples in ascending order: a sample is open where it asked
 * and its cast found nothing (the light is infinitely far: whatever was hit occludes); acc_d = diffuse * radiance and acc_s = specular
 * * radiance per channel, the first open sample's as they are and each later one's added; D = acc_d / spp, S = acc_s / spp and
 * rgb = (rgb + D * (1 - shiness)) + S * shiness — rt_area_light_fold's association.  A record that is no hit: every flag 0, rgb not
 * written; one without an open sample adds nothing. */
RT_FILM_HD void env_fold_record(const EnvFold &f, uint64_t i, bool valid, float shiness) {
    V3 acc_d = v3(0.0f, 0.0f, 0.0f), acc_s = v3(0.0f, 0.0f, 0.0f);
    uint32_t open_count = 0u;
    for (uint32_t s = 0; s < f.spp; ++s) {
        const uint64_t k = (uint64_t)s * f.n + i;
        bool open = valid && f.asks[k] != 0;
        if (open && f.shadow_hits != nullptr && f.shadow_hits[k * RT_ENV_HIT_WORDS] <= 1u) open = false; /* Some(occlusion) */
        if (f.open != nullptr) f.open[k] = open ? 1 : 0;
        if (!open) continue;
        const V3 l = v3p(f.radiance + k * 3u);
        const V3 d = v3p(f.diffuse + k * 3u) * l, sp = v3p(f.specular + k * 3u) * l;
        acc_d = open_count == 0u ? d : acc_d + d;
        acc_s = open_count == 0u ? sp : acc_s + sp;
        ++open_count;
    }
    if (open_count == 0u) return;
    const float samples = (float)f.spp;
    const V3 sum = v3p(f.rgb + i * 3u) + (acc_d / samples) * (1.0f - shiness) + (acc_s / samples) * shiness;
    f.rgb[i * 3u] = sum.x;
    f.rgb[i * 3u + 1u] = sum.y;
    f.rgb[i * 3u + 2u] = sum.z;
}

} /* namespace rt */

#endif /* RT_ENVIRONMENT_H */
