/*
 * rt_svgf.h — the arithmetic of the variance-guided filter queries (include/rt_amd.h "variance-guided filter queries"), written once for
 * the host (librt_host.so: rt_svgf_variance_cpu / rt_svgf_atrous_cpu) and the device (rt_svgf_query.hip, every kernel form).  Every
 * function is a sequence of single f32 operations in the order the header comment of the block gives; the exponential is rt_detmath.h's
 * binary64 exp_mid rounded once, the square root rtdm::f_sqrt (correctly rounded on either side); both libraries are built with
 * -ffp-contract=off, so host and device agree bit for bit.  Where the operation is the denoise or the temporal block's it IS theirs:
 * denoise_dist2, denoise_h, temporal_luminance.  The loops (CPU, simple kernel, tiled kernels) differ only in where a pixel comes from.
 */
#ifndef RT_SVGF_H
#define RT_SVGF_H

#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_denoise.h"
#include "rt_detmath.h"
#include "rt_temporal.h"

#if defined(__HIPCC__)
#define RT_SV_HD __host__ __device__ __forceinline__
#else
#define RT_SV_HD inline
#endif

namespace rt {

/* e(x) of the definition, for an x >= 0 */
RT_SV_HD float svgf_e(float x) { return x > 100.0f ? 0.0f : (float)rtdm::exp_mid(-(double)x); }

/* THE rule wherever a variance is read: negative or NaN reads as +0 */
RT_SV_HD float svgf_vpos(float v) { return v >= 0.0f ? v : 0.0f; }

RT_SV_HD float svgf_abs(float x) { return temporal_float(temporal_bits(x) & 0x7fffffffu); }

/* ---- rt_svgf_variance ---- */

struct SvgfVariance {
    const rt_temporal_pixel *history;
    const float *normal, *position; /* either may be null */
    const uint32_t *valid;          /* may be null */
    uint32_t normal_stride, position_stride, valid_stride;
    uint32_t rows, cols;
    float sn2, sp2;
    uint32_t min_length;
    float min_length_f;
    float *out;
};

inline SvgfVariance svgf_variance_call(const rt_temporal_pixel *history, const rt_denoise_guides &g, const rt_svgf_variance_params &p, uint32_t rows,
                                       uint32_t cols, float *out) {
    SvgfVariance v;
    v.history = history, v.normal = g.normal, v.position = g.position, v.valid = g.valid;
    v.normal_stride = g.normal_stride, v.position_stride = g.position_stride, v.valid_stride = g.valid_stride;
    v.rows = rows, v.cols = cols;
    v.sn2 = p.sigma_normal * p.sigma_normal, v.sp2 = p.sigma_position * p.sigma_position;
    v.min_length = p.min_length, v.min_length_f = (float)p.min_length;
    v.out = out;
    return v;
}

/* what the estimate knows of a pixel: nine words.  length == 0 says "no source": no history there, or its valid word is cleared (or, in
 * a staged tile, it lies outside the image). */
struct SvgfMoments {
    float m1, m2;
    uint32_t length;
    float n0, n1, n2, p0, p1, p2;
};

struct SvgfMomentSums {
    float s1, s2, w;
};

/* pixel i, inside the image; a guide plane that is null leaves its fields +0 (they are not looked at) */
RT_SV_HD SvgfMoments svgf_moments_load(const SvgfVariance &v, uint64_t i) {
    SvgfMoments q = {0.0f, 0.0f, 0u, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (v.valid != nullptr && v.valid[i * v.valid_stride] == 0u) return q;
    const rt_temporal_pixel &h = v.history[i];
    q.m1 = h.moment1, q.m2 = h.moment2, q.length = h.length;
    if (q.length == 0u) return q;
    if (v.normal) {
        const float *n = v.normal + i * v.normal_stride;
        q.n0 = n[0], q.n1 = n[1], q.n2 = n[2];
    }
    if (v.position) {
        const float *s = v.position + i * v.position_stride;
        q.p0 = s[0], q.p1 = s[1], q.p2 = s[2];
    }
    return q;
}

/* does p take step 3, the 7 x 7 estimate */
RT_SV_HD bool svgf_moments_short(const SvgfVariance &v, const SvgfMoments &p) { return p.length != 0u && p.length < v.min_length; }

/* steps 1 and 2, for a p that is not short */
RT_SV_HD float svgf_variance_temporal(const SvgfMoments &p) {
    if (p.length == 0u) return 0.0f;
    const float t = p.m2 - p.m1 * p.m1;
    return t > 0.0f ? t : 0.0f;
}

/* step 3 for one source q inside the image */
RT_SV_HD void svgf_variance_tap(const SvgfVariance &v, SvgfMomentSums &a, const SvgfMoments &p, const SvgfMoments &q) {
    if (q.length == 0u) return;
    float x = 0.0f;
    if (v.normal) x = x + denoise_dist2(p.n0, p.n1, p.n2, q.n0, q.n1, q.n2) / v.sn2;
    if (v.position) x = x + denoise_dist2(p.p0, p.p1, p.p2, q.p0, q.p1, q.p2) / v.sp2;
    if (!(x >= 0.0f)) return;
    const float w = svgf_e(x);
    a.s1 = a.s1 + q.m1 * w;
    a.s2 = a.s2 + q.m2 * w;
    a.w = a.w + w;
}

/* after the loop */
RT_SV_HD float svgf_variance_spatial(const SvgfVariance &v, const SvgfMoments &p, const SvgfMomentSums &a) {
    if (!(a.w > 0.0f)) return 0.0f;
    const float a1 = a.s1 / a.w, a2 = a.s2 / a.w;
    float t = a2 - a1 * a1;
    t = t > 0.0f ? t : 0.0f;
    return t * (v.min_length_f / (float)p.length);
}

#define RT_SVGF_VARIANCE_REACH 3

/* steps 1 to 3 for pixel (r, c), every source read from global memory: the CPU form, and a short pixel whose tile was not staged never
 * comes here on the device */
RT_SV_HD float svgf_variance_pixel(const SvgfVariance &v, uint32_t r, uint32_t c) {
    const SvgfMoments p = svgf_moments_load(v, (uint64_t)r * v.cols + c);
    if (!svgf_moments_short(v, p)) return svgf_variance_temporal(p);
    SvgfMomentSums a = {0.0f, 0.0f, 0.0f};
    for (int dr = -RT_SVGF_VARIANCE_REACH; dr <= RT_SVGF_VARIANCE_REACH; ++dr) {
        const int64_t qr = (int64_t)r + dr;
        if (qr < 0 || qr >= (int64_t)v.rows) continue;
        for (int dc = -RT_SVGF_VARIANCE_REACH; dc <= RT_SVGF_VARIANCE_REACH; ++dc) {
            const int64_t qc = (int64_t)c + dc;
            if (qc < 0 || qc >= (int64_t)v.cols) continue;
            svgf_variance_tap(v, a, p, svgf_moments_load(v, (uint64_t)qr * v.cols + (uint64_t)qc));
        }
    }
    return svgf_variance_spatial(v, p, a);
}

/* ---- rt_svgf_atrous ---- */

/* one level of a call, as the loops see it: colour and variance each a base pointer and a stride in words, so the caller's planes, the
 * outputs and the interleaved scratch entries are read and written through the same code */
struct SvgfLevel {
    const float *in, *vin;
    float *out, *vout; /* vout may be null: the last level of a call without d_variance_out */
    uint32_t in_stride, vin_stride, out_stride, vout_stride;
    const float *normal, *position, *albedo; /* any may be null */
    const uint32_t *valid;                    /* may be null */
    uint32_t normal_stride, position_stride, albedo_stride, valid_stride;
    uint32_t rows, cols;
    int32_t step; /* 1 << l */
    float sigma_l, sn2, sp2;
    uint32_t demod_in, demod_out;
};

/* what the filter knows of a pixel: the colour it sees, its luminance, its variance through vpos, shading normal, position — 11 words */
struct SvgfPix {
    float c0, c1, c2, lum, var, n0, n1, n2, p0, p1, p2;
};

struct SvgfAcc {
    float s0, s1, s2, v, w;
};

RT_SV_HD bool svgf_valid(const SvgfLevel &L, uint64_t i) { return L.valid == nullptr || L.valid[i * L.valid_stride] != 0u; }

/* step 1 */
RT_SV_HD SvgfPix svgf_load(const SvgfLevel &L, uint64_t i) {
    const float *c = L.in + i * L.in_stride;
    SvgfPix q = {c[0], c[1], c[2], 0.0f, svgf_vpos(L.vin[i * L.vin_stride]), 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (L.demod_in) {
        const float *a = L.albedo + i * L.albedo_stride;
        q.c0 = q.c0 / (a[0] + RT_DENOISE_ALBEDO_EPS);
        q.c1 = q.c1 / (a[1] + RT_DENOISE_ALBEDO_EPS);
        q.c2 = q.c2 / (a[2] + RT_DENOISE_ALBEDO_EPS);
    }
    q.lum = temporal_luminance(q.c0, q.c1, q.c2);
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

/* {1/4, 1/2, 1/4} by tap index 0..2 */
RT_SV_HD float svgf_hk(int k) { return k == 1 ? 0.5f : 0.25f; }

/* step 3: the 3 x 3 prefilter of the variance around the valid pixel (r, c), always at step 1 and always from global memory, and the
 * luminance sigma it gives */
RT_SV_HD float svgf_sigma_luminance(const SvgfLevel &L, uint32_t r, uint32_t c) {
    float gs = 0.0f, ks = 0.0f;
    for (int dr = -1; dr <= 1; ++dr) {
        const int64_t qr = (int64_t)r + dr;
        if (qr < 0 || qr >= (int64_t)L.rows) continue;
        for (int dc = -1; dc <= 1; ++dc) {
            const int64_t qc = (int64_t)c + dc;
            if (qc < 0 || qc >= (int64_t)L.cols) continue;
            const uint64_t qi = (uint64_t)qr * L.cols + (uint64_t)qc;
            if (!svgf_valid(L, qi)) continue;
            const float k = svgf_hk(dr + 1) * svgf_hk(dc + 1);
            gs = gs + k * svgf_vpos(L.vin[qi * L.vin_stride]);
            ks = ks + k;
        }
    }
    const float g = ks > 0.0f ? gs / ks : 0.0f;
    return L.sigma_l * (rtdm::f_sqrt(g) + 1e-6f);
}

/* step 4 for one source q that is inside the image and valid */
RT_SV_HD void svgf_tap(const SvgfLevel &L, SvgfAcc &a, const SvgfPix &p, const SvgfPix &q, float sl, int dr, int dc) {
    float x = svgf_abs(p.lum - q.lum) / sl;
    if (L.normal) x = x + denoise_dist2(p.n0, p.n1, p.n2, q.n0, q.n1, q.n2) / L.sn2;
    if (L.position) x = x + denoise_dist2(p.p0, p.p1, p.p2, q.p0, q.p1, q.p2) / L.sp2;
    if (!(x >= 0.0f)) return;
    const float w = denoise_h(dr + 2) * denoise_h(dc + 2) * svgf_e(x);
    a.s0 = a.s0 + q.c0 * w;
    a.s1 = a.s1 + q.c1 * w;
    a.s2 = a.s2 + q.c2 * w;
    a.v = a.v + q.var * (w * w);
    a.w = a.w + w;
}

/* steps 2 and 5: `filtered` is false for an invalid p, whose accumulator is not looked at */
RT_SV_HD void svgf_store(const SvgfLevel &L, uint64_t i, bool filtered, const SvgfAcc &a) {
    float *o = L.out + i * L.out_stride;
    if (filtered && a.w > 0.0f) {
        float o0 = a.s0 / a.w, o1 = a.s1 / a.w, o2 = a.s2 / a.w;
        if (L.demod_out) {
            const float *al = L.albedo + i * L.albedo_stride;
            o0 = o0 * (al[0] + RT_DENOISE_ALBEDO_EPS);
            o1 = o1 * (al[1] + RT_DENOISE_ALBEDO_EPS);
            o2 = o2 * (al[2] + RT_DENOISE_ALBEDO_EPS);
        }
        o[0] = o0, o[1] = o1, o[2] = o2;
        if (L.vout) L.vout[i * L.vout_stride] = a.v / (a.w * a.w);
    } else { /* the raw words: a NaN keeps its payload */
        const uint32_t *src = reinterpret_cast<const uint32_t *>(L.in + i * L.in_stride);
        uint32_t *dst = reinterpret_cast<uint32_t *>(o);
        dst[0] = src[0], dst[1] = src[1], dst[2] = src[2];
        if (L.vout) reinterpret_cast<uint32_t *>(L.vout)[i * L.vout_stride] = reinterpret_cast<const uint32_t *>(L.vin)[i * L.vin_stride];
    }
}

/* steps 1 to 5 for pixel (r, c), every source read from global memory: the CPU form and the simple kernel */
RT_SV_HD void svgf_pixel(const SvgfLevel &L, uint32_t r, uint32_t c) {
    const uint64_t i = (uint64_t)r * L.cols + c;
    const bool filtered = svgf_valid(L, i);
    SvgfAcc a = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (filtered) {
        const SvgfPix p = svgf_load(L, i);
        const float sl = svgf_sigma_luminance(L, r, c);
        for (int dr = -2; dr <= 2; ++dr) {
            const int64_t qr = (int64_t)r + (int64_t)dr * L.step;
            if (qr < 0 || qr >= (int64_t)L.rows) continue;
            for (int dc = -2; dc <= 2; ++dc) {
                const int64_t qc = (int64_t)c + (int64_t)dc * L.step;
                if (qc < 0 || qc >= (int64_t)L.cols) continue;
                const uint64_t qi = (uint64_t)qr * L.cols + (uint64_t)qc;
                if (!svgf_valid(L, qi)) continue;
                svgf_tap(L, a, p, svgf_load(L, qi), sl, dr, dc);
            }
        }
    }
    svgf_store(L, i, filtered, a);
}

/* The scratch of a call, in f32 words per pixel: between levels colour and variance travel as one 16-byte entry {c0, c1, c2, variance};
 * a call of three or more levels also passes through the outputs on its way, and keeps a compact variance plane behind the entries for
 * the case that the caller gave no d_variance_out. */
#define RT_SVGF_ENTRY_WORDS 4u
inline uint32_t svgf_temp_words(uint32_t n_levels) { return n_levels < 2u ? 0u : n_levels == 2u ? RT_SVGF_ENTRY_WORDS : RT_SVGF_ENTRY_WORDS + 1u; }

/* Level j (0-based) of a call: which planes it reads and writes — alternating so that the last level writes the outputs — and whether it
 * demodulates.  sigma_luminance is the same at every level. */
inline SvgfLevel svgf_level(const float *color, uint32_t color_stride, const float *variance, const rt_denoise_guides &g, const rt_svgf_atrous_params &p,
                            uint32_t rows, uint32_t cols, float *out, float *variance_out, float *temp, uint32_t j) {
    const uint32_t after = p.n_levels - 1u - j; /* levels still to come */
    const uint64_t n = (uint64_t)rows * cols;
    /* where a level that writes "the outputs" puts its variance: the caller's plane, else (unless it is the last level) the spare plane */
    float *const spare = temp ? temp + n * RT_SVGF_ENTRY_WORDS : nullptr;
    float *const out_variance = variance_out ? variance_out : spare;
    const bool to_out = after % 2u == 0u;
    SvgfLevel L;
    if (j == 0u) {
        L.in = color, L.in_stride = color_stride, L.vin = variance, L.vin_stride = 1u;
    } else if (to_out) { /* the level before wrote the entries */
        L.in = temp, L.in_stride = RT_SVGF_ENTRY_WORDS, L.vin = temp + 3, L.vin_stride = RT_SVGF_ENTRY_WORDS;
    } else {
        L.in = out, L.in_stride = 3u, L.vin = out_variance, L.vin_stride = 1u;
    }
    if (to_out) {
        L.out = out, L.out_stride = 3u, L.vout = after == 0u ? variance_out : out_variance, L.vout_stride = 1u;
    } else {
        L.out = temp, L.out_stride = RT_SVGF_ENTRY_WORDS, L.vout = temp + 3, L.vout_stride = RT_SVGF_ENTRY_WORDS;
    }
    L.normal = g.normal, L.position = g.position, L.albedo = g.albedo, L.valid = g.valid;
    L.normal_stride = g.normal_stride, L.position_stride = g.position_stride, L.albedo_stride = g.albedo_stride, L.valid_stride = g.valid_stride;
    L.rows = rows, L.cols = cols;
    L.step = (int32_t)(1u << (p.first_level + j));
    L.sigma_l = p.sigma_luminance;
    L.sn2 = p.sigma_normal * p.sigma_normal;
    L.sp2 = p.sigma_position * p.sigma_position;
    L.demod_in = (j == 0u && (p.flags & RT_DENOISE_DEMODULATE_IN)) ? 1u : 0u;
    L.demod_out = (after == 0u && (p.flags & RT_DENOISE_DEMODULATE_OUT)) ? 1u : 0u;
    return L;
}

/* ---- THE argument checks, in the order include/rt_amd.h states; null: all in range ---- */

inline const char *svgf_guide_strides(const rt_denoise_guides *g) {
    if (g->normal && g->normal_stride < 3u) return "normal_stride must be at least 3 words";
    if (g->position && g->position_stride < 3u) return "position_stride must be at least 3 words";
    if (g->albedo && g->albedo_stride < 3u) return "albedo_stride must be at least 3 words";
    if (g->valid && g->valid_stride < 1u) return "valid_stride must be at least 1 word";
    return nullptr;
}

/* rt_svgf_variance, rt_svgf_variance_host and rt_svgf_variance_cpu.  aligned: the device form takes the records rt_temporal_accumulate
 * wrote, which are 16-byte aligned there. */
inline const char *svgf_variance_limits(const rt_temporal_pixel *history, const rt_denoise_guides *g, const rt_svgf_variance_params *p, uint64_t rows,
                                        uint64_t cols, const float *out, bool aligned) {
    if (!g) return "null guides";
    if (!p) return "null params";
    if (rows >= (1ull << 32) || cols >= (1ull << 32) || rows * cols >= (1ull << 32)) return "rows * cols: 2^32 pixels or more";
    if (!(p->sigma_normal > 0.0f)) return "sigma_normal must be > 0 (+inf: the term is off)";
    if (!(p->sigma_position > 0.0f)) return "sigma_position must be > 0 (+inf: the term is off)";
    if (p->min_length < 1u) return "min_length must be at least 1";
    if (p->flags != 0u) return "flags: unknown bits (none is defined)";
    if (const char *bad = svgf_guide_strides(g)) return bad;
    if (rows == 0u || cols == 0u) return nullptr;
    if (!history) return "null history pointer";
    if (!out) return "null variance_out pointer";
    if ((const void *)out == (const void *)history) return "variance_out must not be history";
    if (aligned && ((uintptr_t)history & 15u)) return "history must be 16-byte aligned";
    return nullptr;
}

/* rt_svgf_atrous, rt_svgf_atrous_host and rt_svgf_atrous_cpu.  needs_temp: the caller passes the scratch (the _host round trip makes its own). */
inline const char *svgf_atrous_limits(const float *color, uint32_t color_stride, const float *variance, const rt_denoise_guides *g,
                                      const rt_svgf_atrous_params *p, uint64_t rows, uint64_t cols, const float *out, const float *variance_out,
                                      const float *temp, bool needs_temp) {
    if (!g) return "null guides";
    if (!p) return "null params";
    if (rows >= (1ull << 32) || cols >= (1ull << 32) || rows * cols >= (1ull << 32)) return "rows * cols: 2^32 pixels or more";
    if (p->n_levels < 1u) return "n_levels must be at least 1";
    if (p->first_level >= RT_DENOISE_MAX_LEVELS || p->n_levels > RT_DENOISE_MAX_LEVELS || p->first_level + p->n_levels > RT_DENOISE_MAX_LEVELS)
        return "first_level + n_levels must be at most 6";
    if (!(p->sigma_luminance > 0.0f)) return "sigma_luminance must be > 0 (+inf: the term is off)";
    if (!(p->sigma_normal > 0.0f)) return "sigma_normal must be > 0 (+inf: the term is off)";
    if (!(p->sigma_position > 0.0f)) return "sigma_position must be > 0 (+inf: the term is off)";
    if (p->flags & ~RT_DENOISE_DEMODULATE) return "flags: unknown bits (RT_DENOISE_DEMODULATE_IN, RT_DENOISE_DEMODULATE_OUT)";
    if ((p->flags & RT_DENOISE_DEMODULATE) && !g->albedo) return "flags: demodulation needs an albedo plane";
    if (color_stride < 3u) return "color_stride must be at least 3 words";
    if (const char *bad = svgf_guide_strides(g)) return bad;
    if (rows == 0u || cols == 0u) return nullptr;
    if (!color) return "null color pointer";
    if (!variance) return "null variance pointer";
    if (!out) return "null out pointer";
    if (out == color || out == variance) return "out must not be color or variance";
    if (variance_out && (variance_out == color || variance_out == variance || variance_out == out)) return "variance_out must not be color, variance or out";
    if (needs_temp) {
        if (!temp && p->n_levels >= 2u) return "null temp pointer with n_levels >= 2";
        if (temp && (temp == color || temp == variance || temp == out || temp == variance_out)) return "temp must not be color, variance, out or variance_out";
    }
    return nullptr;
}

} /* namespace rt */

#endif /* RT_SVGF_H */
