/*
 * rt_denoise.h — the arithmetic of the denoise queries (include/rt_amd.h "denoise queries"), written once for the host (librt_host.so:
 * rt_denoise_atrous_cpu) and the device (rt_denoise_query.hip, both kernel forms).  Every function is a sequence of single f32
 * operations in the order the header comment of the block gives — the exponential alone is rt_detmath.h's binary64 exp_mid, + - * / only,
 * rounded once; both libraries are built with -ffp-contract=off and the divides are correctly rounded on either side, so host and device
 * agree bit for bit.  The three loops (CPU, simple kernel, tiled kernel) differ only in where a DenoisePix comes from.
 */
#ifndef RT_DENOISE_H
#define RT_DENOISE_H

#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_detmath.h"

#if defined(__HIPCC__)
#define RT_DN_HD __host__ __device__ __forceinline__
#else
#define RT_DN_HD inline
#endif

namespace rt {

/* one level of a call, as the loops see it */
struct DenoiseLevel {
    const float *in;
    float *out;
    const float *normal, *position, *albedo; /* any may be null */
    const uint32_t *valid;                    /* may be null */
    uint32_t normal_stride, position_stride, albedo_stride, valid_stride;
    uint32_t rows, cols;
    int32_t step;            /* 1 << l */
    float sc2, sn2, sp2;     /* the squared sigmas of this level */
    uint32_t demod_in, demod_out;
};

/* what the filter knows of a pixel: the colour it sees (step 1 of the definition), shading normal, position */
struct DenoisePix {
    float c0, c1, c2, n0, n1, n2, p0, p1, p2;
};

struct DenoiseAcc {
    float s0, s1, s2, w;
};

#define RT_DENOISE_ALBEDO_EPS 1e-3f

RT_DN_HD bool denoise_valid(const DenoiseLevel &L, uint64_t i) { return L.valid == nullptr || L.valid[i * L.valid_stride] != 0u; }

/* step 1; a plane that is null leaves its fields +0 (they are not looked at) */
RT_DN_HD DenoisePix denoise_load(const DenoiseLevel &L, uint64_t i) {
    DenoisePix q = {L.in[3u * i], L.in[3u * i + 1u], L.in[3u * i + 2u], 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (L.demod_in) {
        const float *a = L.albedo + i * L.albedo_stride;
        q.c0 = q.c0 / (a[0] + RT_DENOISE_ALBEDO_EPS);
        q.c1 = q.c1 / (a[1] + RT_DENOISE_ALBEDO_EPS);
        q.c2 = q.c2 / (a[2] + RT_DENOISE_ALBEDO_EPS);
    }
    if (L.normal) {
        const float *n = L.normal + i * L.normal_stride;
        q.n0 = n[0], q.n1 = n[1], q.n2 = n[2];
    }
    if (L.position) {
        const float *p = L.position + i * L.position_stride;
        q.p0 = p[0], q.p1 = p[1], q.p2 = p[2];
    }
    return q;
}

RT_DN_HD float denoise_dist2(float a0, float a1, float a2, float b0, float b1, float b2) {
    const float d0 = a0 - b0, d1 = a1 - b1, d2 = a2 - b2;
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

/* the B3 spline {1/16, 1/4, 3/8, 1/4, 1/16} by tap index 0..4 (no table: the loops are unrolled and this folds to a literal) */
RT_DN_HD float denoise_h(int k) { return k == 2 ? 0.375f : (k == 1 || k == 3) ? 0.25f : 0.0625f; }

/* step 3 for one source q that is inside the image and valid */
RT_DN_HD void denoise_tap(const DenoiseLevel &L, DenoiseAcc &a, const DenoisePix &p, const DenoisePix &q, int dr, int dc) {
    float x = denoise_dist2(p.c0, p.c1, p.c2, q.c0, q.c1, q.c2) / L.sc2;
    if (L.normal) x = x + denoise_dist2(p.n0, p.n1, p.n2, q.n0, q.n1, q.n2) / L.sn2;
    if (L.position) x = x + denoise_dist2(p.p0, p.p1, p.p2, q.p0, q.p1, q.p2) / L.sp2;
    if (!(x >= 0.0f)) return;
    const float e = x > 100.0f ? 0.0f : (float)rtdm::exp_mid(-(double)x);
    const float w = denoise_h(dr + 2) * denoise_h(dc + 2) * e;
    a.s0 = a.s0 + q.c0 * w;
    a.s1 = a.s1 + q.c1 * w;
    a.s2 = a.s2 + q.c2 * w;
    a.w = a.w + w;
}

/* steps 2 and 4: `filtered` is false for an invalid p, whose accumulator is not looked at */
RT_DN_HD void denoise_store(const DenoiseLevel &L, uint64_t i, bool filtered, const DenoiseAcc &a) {
    if (filtered && a.w > 0.0f) {
        float o0 = a.s0 / a.w, o1 = a.s1 / a.w, o2 = a.s2 / a.w;
        if (L.demod_out) {
            const float *al = L.albedo + i * L.albedo_stride;
            o0 = o0 * (al[0] + RT_DENOISE_ALBEDO_EPS);
            o1 = o1 * (al[1] + RT_DENOISE_ALBEDO_EPS);
            o2 = o2 * (al[2] + RT_DENOISE_ALBEDO_EPS);
        }
        L.out[3u * i] = o0;
        L.out[3u * i + 1u] = o1;
        L.out[3u * i + 2u] = o2;
    } else { /* the raw words: a NaN keeps its payload */
        const uint32_t *src = reinterpret_cast<const uint32_t *>(L.in);
        uint32_t *dst = reinterpret_cast<uint32_t *>(L.out);
        dst[3u * i] = src[3u * i];
        dst[3u * i + 1u] = src[3u * i + 1u];
        dst[3u * i + 2u] = src[3u * i + 2u];
    }
}

/* Level j (0-based) of a call: which planes it reads and writes — alternating so that the last level writes `out` — its sigmas and
 * whether it demodulates.  sigma_color * 2^-j is an exact multiply by a power of two. */
inline DenoiseLevel denoise_level(const float *color, const rt_denoise_guides &g, const rt_denoise_params &p, uint32_t rows, uint32_t cols, float *out,
                                  float *temp, uint32_t j) {
    const uint32_t after = p.n_levels - 1u - j; /* levels still to come */
    DenoiseLevel L;
    L.in = j == 0u ? color : (after % 2u == 0u ? temp : out);
    L.out = after % 2u == 0u ? out : temp;
    L.normal = g.normal, L.position = g.position, L.albedo = g.albedo, L.valid = g.valid;
    L.normal_stride = g.normal_stride, L.position_stride = g.position_stride, L.albedo_stride = g.albedo_stride, L.valid_stride = g.valid_stride;
    L.rows = rows, L.cols = cols;
    L.step = (int32_t)(1u << (p.first_level + j));
    const float sc = p.sigma_color * (1.0f / (float)(1u << j));
    L.sc2 = sc * sc;
    L.sn2 = p.sigma_normal * p.sigma_normal;
    L.sp2 = p.sigma_position * p.sigma_position;
    L.demod_in = (j == 0u && (p.flags & RT_DENOISE_DEMODULATE_IN)) ? 1u : 0u;
    L.demod_out = (after == 0u && (p.flags & RT_DENOISE_DEMODULATE_OUT)) ? 1u : 0u;
    return L;
}

/* THE argument check of rt_denoise_atrous, rt_denoise_atrous_host and rt_denoise_atrous_cpu, in the order include/rt_amd.h states;
 * null: all in range.  needs_temp: the caller passes a temp plane (the _host round trip makes its own). */
inline const char *denoise_limits(const float *color, const rt_denoise_guides *g, const rt_denoise_params *p, uint64_t rows, uint64_t cols, const float *out,
                                  const float *temp, bool needs_temp) {
    if (!g) return "null guides";
    if (!p) return "null params";
    if (rows >= (1ull << 32) || cols >= (1ull << 32) || rows * cols >= (1ull << 32)) return "rows * cols: 2^32 pixels or more";
    if (p->n_levels < 1u) return "n_levels must be at least 1";
    if (p->first_level >= RT_DENOISE_MAX_LEVELS || p->n_levels > RT_DENOISE_MAX_LEVELS || p->first_level + p->n_levels > RT_DENOISE_MAX_LEVELS)
        return "first_level + n_levels must be at most 6";
    if (!(p->sigma_color > 0.0f)) return "sigma_color must be > 0 (+inf: the term is off)";
    if (!(p->sigma_normal > 0.0f)) return "sigma_normal must be > 0 (+inf: the term is off)";
    if (!(p->sigma_position > 0.0f)) return "sigma_position must be > 0 (+inf: the term is off)";
    if (p->flags & ~RT_DENOISE_DEMODULATE) return "flags: unknown bits (RT_DENOISE_DEMODULATE_IN, RT_DENOISE_DEMODULATE_OUT)";
    if ((p->flags & RT_DENOISE_DEMODULATE) && !g->albedo) return "flags: demodulation needs an albedo plane";
    if (g->normal && g->normal_stride < 3u) return "normal_stride must be at least 3 words";
    if (g->position && g->position_stride < 3u) return "position_stride must be at least 3 words";
    if (g->albedo && g->albedo_stride < 3u) return "albedo_stride must be at least 3 words";
    if (g->valid && g->valid_stride < 1u) return "valid_stride must be at least 1 word";
    if (rows == 0u || cols == 0u) return nullptr;
    if (!color) return "null color pointer";
    if (!out) return "null out pointer";
    if (out == color) return "out must not be color";
    if (needs_temp) {
        if (!temp && p->n_levels >= 2u) return "null temp pointer with n_levels >= 2";
        if (temp && temp == color) return "temp must not be color";
        if (temp && temp == out) return "temp must not be out";
    }
    return nullptr;
}

} /* namespace rt */

#endif /* RT_DENOISE_H */
