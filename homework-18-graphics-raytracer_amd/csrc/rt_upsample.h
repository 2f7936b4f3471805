/*
 * rt_upsample.h — the arithmetic of the guided upsampling queries (include/rt_amd.h "guided upsampling queries"), written once for the
 * host (librt_host.so: rt_upsample_guided_cpu) and the device (rt_upsample_query.hip, both kernel forms).  Every function is a sequence
 * of single f32 operations in the order the header comment of the block gives — the exponential alone is rt_detmath.h's binary64
 * exp_mid; both libraries are built with -ffp-contract=off and the divides are correctly rounded on either side, so host and device agree
 * bit for bit.  The guide planes, their readers, the weight terms and e(x) ARE rt_atrous.h's.
 *
 * A pixel's walk is upsample_pixel's: the CPU form and the plain kernel hand it sources it reads from global memory (upsample_source_at),
 * the tiled kernel the entries of its staged window.  A source that does not exist (outside the low image, valid word cleared) is
 * UpsampleSource::dead(), a colour whose first word is a NaN: the walk skips a colour that is not finite anyway, so a dead entry needs
 * no test of its own.
 */
#ifndef RT_UPSAMPLE_H
#define RT_UPSAMPLE_H

#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_atrous.h"

namespace rt {

#define RT_UPSAMPLE_MIN_SCALE 2u
#define RT_UPSAMPLE_MAX_SCALE 4u
#define RT_UPSAMPLE_MAX_RADIUS 2

/* one call, as the loops see it.  lo: the low-resolution guides and the size derived from the output's; hi: the full-resolution guides
 * and the output's size.  A guide term is on where BOTH sets carry its plane, the object test where both object planes are given:
 * UpsampleArgs::call clears the other side's pointer otherwise, so the readers of rt_atrous.h see the planes the definition uses. */
struct UpsampleCall {
    const float *color;
    GuidePlanes lo, hi;
    const uint32_t *object_lo, *object_hi;
    uint32_t color_stride, object_lo_stride, object_hi_stride;
    uint32_t scale;
    int radius;
    float sn2, sp2; /* the squared sigmas of the guide terms */
    uint32_t demod_in, demod_out;
    float *out;
    RT_AT_HD uint64_t count() const { return (uint64_t)hi.rows * hi.cols; }
    RT_AT_HD void operator()(uint64_t i) const; /* upsample_pixel_global */
};

inline uint32_t upsample_low_size(uint32_t full, uint32_t scale) { return (uint32_t)(((uint64_t)full + scale - 1u) / scale); }

/* what the walk knows of a low-resolution pixel, and an entry of the staged window: the colour it sees (demodulated where the call
 * says so), shading normal and position, the object (+0 without object planes) */
struct UpsampleSource {
    float c0, c1, c2;
    GuidePoint g;
    uint32_t object;

    static RT_AT_HD UpsampleSource dead() { return {__builtin_nanf(""), 0.0f, 0.0f, {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, 0u}; }
};

/* low-resolution pixel qi, inside the low image */
RT_AT_HD UpsampleSource upsample_source(const UpsampleCall &u, uint64_t qi) {
    if (!guide_valid(u.lo, qi)) return UpsampleSource::dead();
    const float *c = u.color + qi * u.color_stride;
    UpsampleSource q = {c[0], c[1], c[2], {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, 0u};
    if (u.demod_in) guide_demodulate(u.lo, qi, q.c0, q.c1, q.c2);
    q.g = guide_point(u.lo, qi);
    if (u.object_lo) q.object = u.object_lo[qi * u.object_lo_stride];
    return q;
}

/* ... and the low-resolution pixel (qr, qc), wherever it lies */
RT_AT_HD UpsampleSource upsample_source_at(const UpsampleCall &u, int64_t qr, int64_t qc) {
    if (qr < 0 || qr >= (int64_t)u.lo.rows || qc < 0 || qc >= (int64_t)u.lo.cols) return UpsampleSource::dead();
    return upsample_source(u, (uint64_t)qr * u.lo.cols + (uint64_t)qc);
}

/* step 2 along one axis, for output coordinate r: b = floor((2 r + 1 - s) / 2 s), in integers */
RT_AT_HD int64_t upsample_base(uint32_t r, uint32_t s) {
    const int64_t a = 2 * (int64_t)r + 1 - (int64_t)s, d = 2 * (int64_t)s;
    return a >= 0 ? a / d : -((d - 1 - a) / d);
}

/* ... its fraction, and the tents of step 3: t[k] belongs to the offset k - (R - 1), k = 0 .. 2 R - 1 */
template <int R>
struct UpsampleAxis {
    int64_t b;
    float t[2 * R];
};

template <int R>
RT_AT_HD UpsampleAxis<R> upsample_axis(uint32_t r, uint32_t s) {
    UpsampleAxis<R> x;
    x.b = upsample_base(r, s);
    const int64_t d = 2 * (int64_t)s, n = (2 * (int64_t)r + 1 - (int64_t)s) - d * x.b; /* 0 .. 2 s - 1 */
    const float f = (float)n / (float)d;
    for (int k = 0; k < 2 * R; ++k) x.t[k] = 1.0f - __builtin_fabsf((float)(k - (R - 1)) - f) / (float)R;
    return x;
}

/* steps 1 and 4's "otherwise": the raw words of the nearest low-resolution colour; a NaN keeps its payload */
RT_AT_HD void upsample_nearest(const UpsampleCall &u, uint64_t i, uint32_t r, uint32_t c) {
    const uint64_t ni = (uint64_t)(r / u.scale) * u.lo.cols + (uint64_t)(c / u.scale);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(u.color) + ni * u.color_stride;
    uint32_t *dst = reinterpret_cast<uint32_t *>(u.out) + 3u * i;
    dst[0] = src[0], dst[1] = src[1], dst[2] = src[2];
}

RT_AT_HD bool upsample_finite(float c) { return c - c == 0.0f; }

/* Output pixel (r, c): source(kr, kc) is the source of tap dr = kr - (R - 1), dc = kc - (R - 1), dead() where there is none.  R is a
 * constant so that the (2 R)^2 taps unroll. */
template <int R, class SourceAt>
RT_AT_HD void upsample_pixel(const UpsampleCall &u, uint32_t r, uint32_t c, const UpsampleAxis<R> &y, const UpsampleAxis<R> &x, SourceAt source) {
    const uint64_t i = (uint64_t)r * u.hi.cols + c;
    if (!guide_valid(u.hi, i)) return upsample_nearest(u, i, r, c);
    const GuidePoint p = guide_point(u.hi, i);
    const uint32_t object = u.object_hi ? u.object_hi[i * u.object_hi_stride] : 0u;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, wsum = 0.0f;
    for (int kr = 0; kr < 2 * R; ++kr) {
        if (y.t[kr] <= 0.0f) continue;
        for (int kc = 0; kc < 2 * R; ++kc) {
            if (x.t[kc] <= 0.0f) continue;
            const UpsampleSource q = source(kr, kc);
            if (!(upsample_finite(q.c0) && upsample_finite(q.c1) && upsample_finite(q.c2))) continue; /* a dead entry too */
            if (q.object != object) continue;
            const float e = guide_terms(u.hi, u.sn2, u.sp2, 0.0f, p, q.g);
            if (!(e >= 0.0f)) continue;
            const float w = (y.t[kr] * x.t[kc]) * atrous_e(e);
            s0 = s0 + q.c0 * w;
            s1 = s1 + q.c1 * w;
            s2 = s2 + q.c2 * w;
            wsum = wsum + w;
        }
    }
    if (!(wsum > 0.0f)) return upsample_nearest(u, i, r, c);
    float o0 = s0 / wsum, o1 = s1 / wsum, o2 = s2 / wsum;
    if (u.demod_out) guide_modulate(u.hi, i, o0, o1, o2);
    u.out[3u * i] = o0;
    u.out[3u * i + 1u] = o1;
    u.out[3u * i + 2u] = o2;
}

/* pixel i, every source read from global memory: the CPU form and the plain kernel */
template <int R>
RT_AT_HD void upsample_pixel_global(const UpsampleCall &u, uint64_t i) {
    const uint32_t r = (uint32_t)(i / u.hi.cols), c = (uint32_t)(i - (uint64_t)r * u.hi.cols);
    const UpsampleAxis<R> y = upsample_axis<R>(r, u.scale), x = upsample_axis<R>(c, u.scale);
    upsample_pixel<R>(u, r, c, y, x, [&](int kr, int kc) { return upsample_source_at(u, y.b + (kr - (R - 1)), x.b + (kc - (R - 1))); });
}
RT_AT_HD void UpsampleCall::operator()(uint64_t i) const {
    if (radius == 1) {
        upsample_pixel_global<1>(*this, i);
    } else {
        upsample_pixel_global<2>(*this, i);
    }
}

/* The arguments of rt_upsample_guided, rt_upsample_guided_host and rt_upsample_guided_cpu (rt_query_args.h); the checks in the order
 * include/rt_amd.h states */
struct UpsampleArgs {
    const float *color; uint32_t color_stride;
    const rt_denoise_guides *low; const uint32_t *object_lo; uint32_t object_lo_stride;
    const rt_denoise_guides *full; const uint32_t *object_hi; uint32_t object_hi_stride;
    const rt_upsample_params *params; uint32_t rows, cols; float *out;

    const char *limits(QueryForm, int *status) const {
        *status = RT_ERR_INVALID_ARGUMENT;
        if (!params) return "null params";
        if (!low) return "null low guides";
        if (!full) return "null full guides";
        if (const char *bad = limits_image(rows, cols)) return bad;
        if (params->scale < RT_UPSAMPLE_MIN_SCALE || params->scale > RT_UPSAMPLE_MAX_SCALE) return "scale must be 2, 3 or 4";
        if (params->radius < 1u || params->radius > (uint32_t)RT_UPSAMPLE_MAX_RADIUS) return "radius must be 1 or 2";
        if (const char *bad = RT_LIMITS_SIGMA(params, sigma_normal)) return bad;
        if (const char *bad = RT_LIMITS_SIGMA(params, sigma_position)) return bad;
        if (params->flags & ~RT_DENOISE_DEMODULATE) return "flags: unknown bits (RT_DENOISE_DEMODULATE_IN, RT_DENOISE_DEMODULATE_OUT)";
        if ((params->flags & RT_DENOISE_DEMODULATE_IN) && !low->albedo) return "flags: RT_DENOISE_DEMODULATE_IN needs the low albedo plane";
        if ((params->flags & RT_DENOISE_DEMODULATE_OUT) && !full->albedo) return "flags: RT_DENOISE_DEMODULATE_OUT needs the full albedo plane";
        if (const char *bad = limits_guide_strides(low)) return bad;
        if (const char *bad = limits_guide_strides(full)) return bad;
        if (color_stride < 3u) return "color_stride must be at least 3 words";
        if (object_lo && object_lo_stride < 1u) return "object_lo_stride must be at least 1 word";
        if (object_hi && object_hi_stride < 1u) return "object_full_stride must be at least 1 word";
        if (empty()) return nullptr;
        if (!color) return "null color pointer";
        if (!out) return "null out pointer";
        if (out == color) return "out must not be color";
        return nullptr;
    }

    bool empty() const { return rows == 0u || cols == 0u; }
    uint32_t low_rows() const { return upsample_low_size(rows, params->scale); }
    uint32_t low_cols() const { return upsample_low_size(cols, params->scale); }

    template <class Stage>
    void arrays(Stage &s) {
        const size_t n = (size_t)rows * cols, n_lo = (size_t)low_rows() * low_cols();
        color = s.plane(color, n_lo, color_stride, 3u);
        low = s.guides(low, n_lo, (params->flags & RT_DENOISE_DEMODULATE_IN) != 0u);
        full = s.guides(full, n, (params->flags & RT_DENOISE_DEMODULATE_OUT) != 0u);
        object_lo = s.plane(object_lo, n_lo, object_lo_stride, 1u);
        object_hi = s.plane(object_hi, n, object_hi_stride, 1u);
        out = s.out(out, n * 3u * sizeof(float));
    }

    UpsampleCall call() const {
        UpsampleCall u;
        u.color = color, u.color_stride = color_stride;
        guide_planes(u.lo, *low, low_rows(), low_cols());
        guide_planes(u.hi, *full, rows, cols);
        if (!u.lo.normal || !u.hi.normal) u.lo.normal = u.hi.normal = nullptr;
        if (!u.lo.position || !u.hi.position) u.lo.position = u.hi.position = nullptr;
        const bool objects = object_lo && object_hi;
        u.object_lo = objects ? object_lo : nullptr, u.object_hi = objects ? object_hi : nullptr;
        u.object_lo_stride = object_lo_stride, u.object_hi_stride = object_hi_stride;
        u.scale = params->scale, u.radius = (int)params->radius;
        u.sn2 = params->sigma_normal * params->sigma_normal;
        u.sp2 = params->sigma_position * params->sigma_position;
        u.demod_in = (params->flags & RT_DENOISE_DEMODULATE_IN) ? 1u : 0u;
        u.demod_out = (params->flags & RT_DENOISE_DEMODULATE_OUT) ? 1u : 0u;
        u.out = out;
        return u;
    }
};

} /* namespace rt */

#endif /* RT_UPSAMPLE_H */
