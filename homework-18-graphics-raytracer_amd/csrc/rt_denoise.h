/*
 * rt_denoise.h — the arithmetic of the denoise queries (include/rt_amd.h "denoise queries"), written once for the host (librt_host.so:
 * rt_denoise_atrous_cpu) and the device (rt_denoise_query.hip, both kernel forms) as DenoiseFilter, a filter of rt_atrous.h.  Every function is a sequence of single f32
 * operations in the order the header comment of the block gives — the exponential alone is rt_detmath.h's binary64 exp_mid, + - * / only,
 * rounded once; both libraries are built with -ffp-contract=off and the divides are correctly rounded on either side, so host and device
 * agree bit for bit.  The walks are rt_atrous.h's and rt_atrous_kernel.h's: the CPU form, the simple kernel and the tiled kernel differ
 * only in where a DenoisePix comes from.
 */
#ifndef RT_DENOISE_H
#define RT_DENOISE_H

#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_atrous.h"

namespace rt {

/* one level of a call, as the loops see it */
struct DenoiseLevel : AtrousLevel {
    const float *in;
    float *out;
    float sc2; /* the squared colour sigma of this level */
};

/* what the filter knows of a pixel: the colour it sees (step 1 of the definition), shading normal, position */
struct DenoisePix {
    float c0, c1, c2;
    GuidePoint g;
};

struct DenoiseAcc {
    float s0, s1, s2, w;
};

struct DenoiseFilter {
    typedef DenoiseLevel Level;
    typedef DenoisePix Pix;
    typedef DenoiseAcc Acc;
    struct Context {}; /* a walk needs nothing of its centre beyond p */

    /* step 1 */
    static RT_AT_HD DenoisePix load(const DenoiseLevel &L, uint64_t i) {
        DenoisePix q = {L.in[3u * i], L.in[3u * i + 1u], L.in[3u * i + 2u], {}};
        if (L.demod_in) guide_demodulate(L, i, q.c0, q.c1, q.c2);
        q.g = guide_point(L, i);
        return q;
    }

    static RT_AT_HD Context context(const DenoiseLevel &, uint32_t, uint32_t) { return {}; }

    /* step 3 for one source q that is inside the image and valid */
    static RT_AT_HD void tap(const DenoiseLevel &L, DenoiseAcc &a, const DenoisePix &p, const DenoisePix &q, Context, int dr, int dc) {
        const float x = guide_terms(L, L.sn2, L.sp2, denoise_dist2(p.c0, p.c1, p.c2, q.c0, q.c1, q.c2) / L.sc2, p.g, q.g);
        if (!(x >= 0.0f)) return;
        const float w = denoise_h(dr + 2) * denoise_h(dc + 2) * atrous_e(x);
        a.s0 = a.s0 + q.c0 * w;
        a.s1 = a.s1 + q.c1 * w;
        a.s2 = a.s2 + q.c2 * w;
        a.w = a.w + w;
    }

    /* steps 2 and 4 */
    static RT_AT_HD void store(const DenoiseLevel &L, uint64_t i, bool filtered, const DenoiseAcc &a) {
        if (filtered && a.w > 0.0f) {
            float o0 = a.s0 / a.w, o1 = a.s1 / a.w, o2 = a.s2 / a.w;
            if (L.demod_out) guide_modulate(L, i, o0, o1, o2);
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

    /* a NaN colour: its exponent is NaN and tap skips it, as it skips a caller's own NaN colour */
    static RT_AT_HD DenoisePix dead() { return {__builtin_nanf(""), 0.0f, 0.0f, {}}; }
    static RT_AT_HD bool takes_taps(const DenoisePix &) { return true; }
};

/* The arguments of rt_denoise_atrous, rt_denoise_atrous_host and rt_denoise_atrous_cpu (rt_query_args.h).  temp is the caller's plane; the
 * _host form passes null and its round trip makes its own. */
struct DenoiseArgs {
    const float *color;
    const rt_denoise_guides *guides;
    const rt_denoise_params *params;
    uint32_t rows, cols;
    float *out, *temp;

    const char *limits(QueryForm form, int *status) const {
        *status = RT_ERR_INVALID_ARGUMENT;
        if (!guides) return "null guides";
        if (!params) return "null params";
        const char *bad = limits_image(rows, cols);
        if (!bad) bad = limits_levels(params->first_level, params->n_levels);
        if (!bad) bad = RT_LIMITS_SIGMA(params, sigma_color);
        if (!bad) bad = RT_LIMITS_SIGMA(params, sigma_normal);
        if (!bad) bad = RT_LIMITS_SIGMA(params, sigma_position);
        if (!bad) bad = limits_demodulation(params->flags, guides);
        if (!bad) bad = limits_guide_strides(guides);
        if (bad) return bad;
        if (empty()) return nullptr;
        if (!color) return "null color pointer";
        if (!out) return "null out pointer";
        if (out == color) return "out must not be color";
        if (query_takes_temp(form)) {
            if (!temp && params->n_levels >= 2u) return "null temp pointer with n_levels >= 2";
            if (temp && temp == color) return "temp must not be color";
            if (temp && temp == out) return "temp must not be out";
        }
        return nullptr;
    }

    bool empty() const { return rows == 0u || cols == 0u; }

    template <class Stage>
    void arrays(Stage &s) {
        const size_t n = (size_t)rows * cols, plane = n * 3u * sizeof(float);
        color = s.in(color, plane);
        guides = s.guides(guides, n);
        out = s.out(out, plane);
        temp = params->n_levels >= 2u ? static_cast<float *>(s.scratch(plane)) : nullptr;
    }

    /* Level j (0-based) of the call: which planes it reads and writes and its colour sigma.  sigma_color * 2^-j is an exact multiply by
     * a power of two. */
    DenoiseLevel level(uint32_t j) const {
        DenoiseLevel L;
        const AtrousTurn t = atrous_schedule(L, *guides, *params, rows, cols, j);
        L.in = j == 0u ? color : (t.to_out ? temp : out);
        L.out = t.to_out ? out : temp;
        const float sc = params->sigma_color * (1.0f / (float)(1u << j));
        L.sc2 = sc * sc;
        return L;
    }
};

} /* namespace rt */

#endif /* RT_DENOISE_H */
