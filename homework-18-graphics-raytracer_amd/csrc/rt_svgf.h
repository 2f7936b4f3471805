/*
 * rt_svgf.h — the arithmetic of the variance-guided filter queries (include/rt_amd.h "variance-guided filter queries"), written once for
 * the host (librt_host.so: rt_svgf_variance_cpu / rt_svgf_atrous_cpu) and the device (rt_svgf_query.hip, every kernel form).  Every
 * function is a sequence of single f32 operations in the order the header comment of the block gives; the exponential is rt_detmath.h's
 * binary64 exp_mid rounded once, the square root rtdm::f_sqrt (correctly rounded on either side); both libraries are built with
 * -ffp-contract=off, so host and device agree bit for bit.  Where the operation is the denoise or the temporal block's it IS theirs:
 * the guide readers, guide_terms, atrous_e and denoise_h of rt_atrous.h, temporal_luminance.  The A-Trous filter is SvgfFilter, a filter of
 * rt_atrous.h beside DenoiseFilter: the walks are that header's and rt_atrous_kernel.h's, and the CPU form, the simple kernel and the
 * tiled kernel differ only in where a pixel comes from.  The variance estimate keeps its own 7 x 7 walk.
 */
#ifndef RT_SVGF_H
#define RT_SVGF_H

#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_atrous.h"
#include "rt_detmath.h"
#include "rt_temporal.h"

namespace rt {

/* THE rule wherever a variance is read: negative or NaN reads as +0 */
RT_AT_HD float svgf_vpos(float v) { return v >= 0.0f ? v : 0.0f; }

RT_AT_HD float svgf_abs(float x) { return temporal_float(temporal_bits(x) & 0x7fffffffu); }

/* ---- rt_svgf_variance ---- */

struct SvgfVariance : GuidePlanes { /* the albedo plane is not looked at */
    const rt_temporal_pixel *history;
    float sn2, sp2;
    uint32_t min_length;
    float min_length_f;
    float *out;
};

/* what the estimate knows of a pixel: nine words.  length == 0 says "no source": no history there, or its valid word is cleared (or, in
 * a staged tile, it lies outside the image). */
struct SvgfMoments {
    float m1, m2;
    uint32_t length;
    GuidePoint g;
};

struct SvgfMomentSums {
    float s1, s2, w;
};

/* pixel i, inside the image; a guide plane that is null leaves its fields +0 (they are not looked at) */
RT_AT_HD SvgfMoments svgf_moments_load(const SvgfVariance &v, uint64_t i) {
    SvgfMoments q = {0.0f, 0.0f, 0u, {}};
    if (!guide_valid(v, i)) return q;
    const rt_temporal_pixel &h = v.history[i];
    q.m1 = h.moment1, q.m2 = h.moment2, q.length = h.length;
    if (q.length != 0u) q.g = guide_point(v, i);
    return q;
}

/* does p take step 3, the 7 x 7 estimate */
RT_AT_HD bool svgf_moments_short(const SvgfVariance &v, const SvgfMoments &p) { return p.length != 0u && p.length < v.min_length; }

/* steps 1 and 2, for a p that is not short */
RT_AT_HD float svgf_variance_temporal(const SvgfMoments &p) {
    if (p.length == 0u) return 0.0f;
    const float t = p.m2 - p.m1 * p.m1;
    return t > 0.0f ? t : 0.0f;
}

/* step 3 for one source q inside the image */
RT_AT_HD void svgf_variance_tap(const SvgfVariance &v, SvgfMomentSums &a, const SvgfMoments &p, const SvgfMoments &q) {
    if (q.length == 0u) return;
    const float x = guide_terms(v, v.sn2, v.sp2, 0.0f, p.g, q.g);
    if (!(x >= 0.0f)) return;
    const float w = atrous_e(x);
    a.s1 = a.s1 + q.m1 * w;
    a.s2 = a.s2 + q.m2 * w;
    a.w = a.w + w;
}

/* after the loop */
RT_AT_HD float svgf_variance_spatial(const SvgfVariance &v, const SvgfMoments &p, const SvgfMomentSums &a) {
    if (!(a.w > 0.0f)) return 0.0f;
    const float a1 = a.s1 / a.w, a2 = a.s2 / a.w;
    float t = a2 - a1 * a1;
    t = t > 0.0f ? t : 0.0f;
    return t * (v.min_length_f / (float)p.length);
}

#define RT_SVGF_VARIANCE_REACH 3

/* steps 1 to 3 for pixel (r, c), every source read from global memory: the CPU form, and a short pixel whose tile was not staged never
 * comes here on the device */
RT_AT_HD float svgf_variance_pixel(const SvgfVariance &v, uint32_t r, uint32_t c) {
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
struct SvgfLevel : AtrousLevel {
    const float *in, *vin;
    float *out, *vout; /* vout may be null: the last level of a call without d_variance_out */
    uint32_t in_stride, vin_stride, out_stride, vout_stride;
    float sigma_l;
};

/* what the filter knows of a pixel: the colour it sees, its luminance, its variance through vpos, shading normal, position — 11 words */
struct SvgfPix {
    float c0, c1, c2, lum, var;
    GuidePoint g;
};

struct SvgfAcc {
    float s0, s1, s2, v, w;
};

/* {1/4, 1/2, 1/4} by tap index 0..2 */
RT_AT_HD float svgf_hk(int k) { return k == 1 ? 0.5f : 0.25f; }

/* step 3: the 3 x 3 prefilter of the variance around the valid pixel (r, c), always at step 1 and always from global memory, and the
 * luminance sigma it gives */
RT_AT_HD float svgf_sigma_luminance(const SvgfLevel &L, uint32_t r, uint32_t c) {
    float gs = 0.0f, ks = 0.0f;
    for (int dr = -1; dr <= 1; ++dr) {
        const int64_t qr = (int64_t)r + dr;
        if (qr < 0 || qr >= (int64_t)L.rows) continue;
        for (int dc = -1; dc <= 1; ++dc) {
            const int64_t qc = (int64_t)c + dc;
            if (qc < 0 || qc >= (int64_t)L.cols) continue;
            const uint64_t qi = (uint64_t)qr * L.cols + (uint64_t)qc;
            if (!guide_valid(L, qi)) continue;
            const float k = svgf_hk(dr + 1) * svgf_hk(dc + 1);
            gs = gs + k * svgf_vpos(L.vin[qi * L.vin_stride]);
            ks = ks + k;
        }
    }
    const float g = ks > 0.0f ? gs / ks : 0.0f;
    return L.sigma_l * (rtdm::f_sqrt(g) + 1e-6f);
}

/* DenoiseFilter with another first weight term, and the variance carried along */
struct SvgfFilter {
    typedef SvgfLevel Level;
    typedef SvgfPix Pix;
    typedef SvgfAcc Acc;
    typedef float Context; /* the luminance sigma of the centre */

    /* step 1 */
    static RT_AT_HD SvgfPix load(const SvgfLevel &L, uint64_t i) {
        const float *c = L.in + i * L.in_stride;
        SvgfPix q = {c[0], c[1], c[2], 0.0f, svgf_vpos(L.vin[i * L.vin_stride]), {}};
        if (L.demod_in) guide_demodulate(L, i, q.c0, q.c1, q.c2);
        q.lum = temporal_luminance(q.c0, q.c1, q.c2);
        q.g = guide_point(L, i);
        return q;
    }

    static RT_AT_HD float context(const SvgfLevel &L, uint32_t r, uint32_t c) { return svgf_sigma_luminance(L, r, c); }

    /* step 4 for one source q that is inside the image and valid */
    static RT_AT_HD void tap(const SvgfLevel &L, SvgfAcc &a, const SvgfPix &p, const SvgfPix &q, float sl, int dr, int dc) {
        const float x = guide_terms(L, L.sn2, L.sp2, svgf_abs(p.lum - q.lum) / sl, p.g, q.g);
        if (!(x >= 0.0f)) return;
        const float w = denoise_h(dr + 2) * denoise_h(dc + 2) * atrous_e(x);
        a.s0 = a.s0 + q.c0 * w;
        a.s1 = a.s1 + q.c1 * w;
        a.s2 = a.s2 + q.c2 * w;
        a.v = a.v + q.var * (w * w);
        a.w = a.w + w;
    }

    /* steps 2 and 5 */
    static RT_AT_HD void store(const SvgfLevel &L, uint64_t i, bool filtered, const SvgfAcc &a) {
        float *o = L.out + i * L.out_stride;
        if (filtered && a.w > 0.0f) {
            float o0 = a.s0 / a.w, o1 = a.s1 / a.w, o2 = a.s2 / a.w;
            if (L.demod_out) guide_modulate(L, i, o0, o1, o2);
            o[0] = o0, o[1] = o1, o[2] = o2;
            if (L.vout) L.vout[i * L.vout_stride] = a.v / (a.w * a.w);
        } else { /* the raw words: a NaN keeps its payload */
            const uint32_t *src = reinterpret_cast<const uint32_t *>(L.in + i * L.in_stride);
            uint32_t *dst = reinterpret_cast<uint32_t *>(o);
            dst[0] = src[0], dst[1] = src[1], dst[2] = src[2];
            if (L.vout) reinterpret_cast<uint32_t *>(L.vout)[i * L.vout_stride] = reinterpret_cast<const uint32_t *>(L.vin)[i * L.vin_stride];
        }
    }

    /* a NaN colour and luminance: its exponent is NaN and tap skips it, as it skips a caller's own NaN colour */
    static RT_AT_HD SvgfPix dead() { return {__builtin_nanf(""), 0.0f, 0.0f, __builtin_nanf(""), 0.0f, {}}; }
    /* a NaN luminance — marked, or the caller's own — takes no tap: it needs no sigma, which saves the staged centre the 3 x 3 reads */
    static RT_AT_HD bool takes_taps(const SvgfPix &p) { return p.lum == p.lum; }
};

/* The scratch of a call, in f32 words per pixel: between levels colour and variance travel as one 16-byte entry {c0, c1, c2, variance};
 * a call of three or more levels also passes through the outputs on its way, and keeps a compact variance plane behind the entries for
 * the case that the caller gave no d_variance_out. */
#define RT_SVGF_ENTRY_WORDS 4u
inline uint32_t svgf_temp_words(uint32_t n_levels) { return n_levels < 2u ? 0u : n_levels == 2u ? RT_SVGF_ENTRY_WORDS : RT_SVGF_ENTRY_WORDS + 1u; }

/* ---- the arguments of the entry points (rt_query_args.h): the checks in the order include/rt_amd.h states ---- */

/* rt_svgf_variance, rt_svgf_variance_host and rt_svgf_variance_cpu.  The device form takes the records rt_temporal_accumulate wrote,
 * which are 16-byte aligned there. */
struct SvgfVarianceArgs {
    const rt_temporal_pixel *history;
    const rt_denoise_guides *guides;
    const rt_svgf_variance_params *params;
    uint32_t rows, cols;
    float *variance_out;

    const char *limits(QueryForm form, int *status) const {
        *status = RT_ERR_INVALID_ARGUMENT;
        if (!guides) return "null guides";
        if (!params) return "null params";
        const char *bad = limits_image(rows, cols);
        if (!bad) bad = RT_LIMITS_SIGMA(params, sigma_normal);
        if (!bad) bad = RT_LIMITS_SIGMA(params, sigma_position);
        if (!bad && params->min_length < 1u) bad = "min_length must be at least 1";
        if (!bad && params->flags != 0u) bad = "flags: unknown bits (none is defined)";
        if (!bad) bad = limits_guide_strides(guides);
        if (bad) return bad;
        if (empty()) return nullptr;
        if (!history) return "null history pointer";
        if (!variance_out) return "null variance_out pointer";
        if ((const void *)variance_out == (const void *)history) return "variance_out must not be history";
        if (query_misaligned(form, history)) return "history must be 16-byte aligned";
        return nullptr;
    }

    bool empty() const { return rows == 0u || cols == 0u; }

    template <class Stage>
    void arrays(Stage &s) {
        const size_t n = (size_t)rows * cols;
        history = s.in(history, n * sizeof(rt_temporal_pixel));
        guides = s.guides(guides, n, false); /* the estimate reads no albedo */
        variance_out = s.out(variance_out, n * sizeof(float));
    }

    SvgfVariance call() const {
        SvgfVariance v;
        guide_planes(v, *guides, rows, cols);
        v.history = history;
        v.sn2 = params->sigma_normal * params->sigma_normal, v.sp2 = params->sigma_position * params->sigma_position;
        v.min_length = params->min_length, v.min_length_f = (float)params->min_length;
        v.out = variance_out;
        return v;
    }
};

/* rt_svgf_atrous, rt_svgf_atrous_host and rt_svgf_atrous_cpu.  temp is the caller's scratch; the _host form passes null and its round
 * trip makes its own. */
struct SvgfAtrousArgs {
    const float *color; uint32_t color_stride; const float *variance;
    const rt_denoise_guides *guides; const rt_svgf_atrous_params *params;
    uint32_t rows, cols; float *out, *variance_out, *temp;

    const char *limits(QueryForm form, int *status) const {
        *status = RT_ERR_INVALID_ARGUMENT;
        if (!guides) return "null guides";
        if (!params) return "null params";
        const char *bad = limits_image(rows, cols);
        if (!bad) bad = limits_levels(params->first_level, params->n_levels);
        if (!bad) bad = RT_LIMITS_SIGMA(params, sigma_luminance);
        if (!bad) bad = RT_LIMITS_SIGMA(params, sigma_normal);
        if (!bad) bad = RT_LIMITS_SIGMA(params, sigma_position);
        if (!bad) bad = limits_demodulation(params->flags, guides);
        if (!bad && color_stride < 3u) bad = "color_stride must be at least 3 words";
        if (!bad) bad = limits_guide_strides(guides);
        if (bad) return bad;
        if (empty()) return nullptr;
        if (!color) return "null color pointer";
        if (!variance) return "null variance pointer";
        if (!out) return "null out pointer";
        if (out == color || out == variance) return "out must not be color or variance";
        if (variance_out && (variance_out == color || variance_out == variance || variance_out == out)) return "variance_out must not be color, variance or out";
        if (query_takes_temp(form)) {
            if (!temp && params->n_levels >= 2u) return "null temp pointer with n_levels >= 2";
            if (temp && (temp == color || temp == variance || temp == out || temp == variance_out)) return "temp must not be color, variance, out or variance_out";
        }
        return nullptr;
    }

    bool empty() const { return rows == 0u || cols == 0u; }

    template <class Stage>
    void arrays(Stage &s) {
        const size_t n = (size_t)rows * cols, temp_bytes = n * svgf_temp_words(params->n_levels) * sizeof(float);
        color = s.plane(color, n, color_stride, 3u);
        variance = s.in(variance, n * sizeof(float));
        guides = s.guides(guides, n);
        out = s.out(out, n * 3u * sizeof(float));
        variance_out = s.out(variance_out, n * sizeof(float));
        temp = temp_bytes ? static_cast<float *>(s.scratch(temp_bytes)) : nullptr;
    }

    /* Level j (0-based) of the call: which planes it reads and writes.  sigma_luminance is the same at every level. */
    SvgfLevel level(uint32_t j) const {
        SvgfLevel L;
        const AtrousTurn t = atrous_schedule(L, *guides, *params, rows, cols, j);
        const uint64_t n = (uint64_t)rows * cols;
        /* where a level that writes "the outputs" puts its variance: the caller's plane, else (unless it is the last level) the spare plane */
        float *const spare = temp ? temp + n * RT_SVGF_ENTRY_WORDS : nullptr;
        float *const out_variance = variance_out ? variance_out : spare;
        if (j == 0u) {
            L.in = color, L.in_stride = color_stride, L.vin = variance, L.vin_stride = 1u;
        } else if (t.to_out) { /* the level before wrote the entries */
            L.in = temp, L.in_stride = RT_SVGF_ENTRY_WORDS, L.vin = temp + 3, L.vin_stride = RT_SVGF_ENTRY_WORDS;
        } else {
            L.in = out, L.in_stride = 3u, L.vin = out_variance, L.vin_stride = 1u;
        }
        if (t.to_out) {
            L.out = out, L.out_stride = 3u, L.vout = t.after == 0u ? variance_out : out_variance, L.vout_stride = 1u;
        } else {
            L.out = temp, L.out_stride = RT_SVGF_ENTRY_WORDS, L.vout = temp + 3, L.vout_stride = RT_SVGF_ENTRY_WORDS;
        }
        L.sigma_l = params->sigma_luminance;
        return L;
    }
};

} /* namespace rt */

#endif /* RT_SVGF_H */

