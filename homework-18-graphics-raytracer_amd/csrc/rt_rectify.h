/*
 * rt_rectify.h — the arithmetic of the history rectification queries (include/rt_amd.h "history rectification queries"), written once for
 * the host (librt_host.so: rt_temporal_bounds_cpu / rt_temporal_accumulate_bounded_cpu / rt_temporal_feedback_cpu) and the device
 * (rt_rectify_query.hip).  Every function is a sequence of single f32 operations in the order the header comment of the block gives; the
 * divides and rtdm::f_sqrt are correctly rounded on either side and both libraries are built with -ffp-contract=off, so host and device
 * agree bit for bit.  Where the operation is another block's it IS theirs: temporal_luminance, svgf_vpos, and — for the bounded
 * accumulate — temporal_load / temporal_gather / temporal_blend / temporal_reset of rt_temporal.h, so the gather is stated once.
 *
 * The box of a pixel is two passes over its window, and both passes are rectify_window's: the CPU form hands it sources it reads from
 * global memory, the kernel the entries of its staged tile.  A source that does not exist (outside the image, valid word cleared)
 * is an entry with the mark RectifySource::none(), which no pixel can carry: a colour of three +0 words has the luminance +0.
 */
#ifndef RT_RECTIFY_H
#define RT_RECTIFY_H

#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_detmath.h"
#include "rt_svgf.h"
#include "rt_temporal.h"

namespace rt {

#define RT_RECTIFY_MAX_RADIUS 3

/* The rows of a window are walked one after the other and only a row's taps side by side: unrolled whole, the 49 taps of radius 3 keep
 * 245 words of sources in flight and leave the kernel two waves per SIMD. */
#if defined(__HIPCC__)
#define RT_RECTIFY_ROW_BY_ROW _Pragma("unroll 1")
#else
#define RT_RECTIFY_ROW_BY_ROW
#endif

/* ---- rt_temporal_bounds ---- */

struct RectifyBounds {
    const float *color;
    const uint32_t *object, *valid; /* each may be null */
    uint32_t color_stride, object_stride, valid_stride;
    uint32_t rows, cols;
    int radius;
    float gamma;
    rt_temporal_box *box;
};

/* what the box knows of a pixel: five words, x[3] the luminance.  An odd number, so a tile row spreads over the LDS banks. */
struct RectifySource {
    float x[4];
    uint32_t object; /* +0 without an object plane */

    /* "no source": three +0 colour words under a luminance that is not +0 — lum(+0, +0, +0) is +0, so no pixel reads like this */
    static RT_TP_HD RectifySource none() { return {{0.0f, 0.0f, 0.0f, 1.0f}, 0u}; }
    RT_TP_HD bool is_none() const { return (temporal_bits(x[0]) | temporal_bits(x[1]) | temporal_bits(x[2])) == 0u && temporal_bits(x[3]) != 0u; }
};

/* pixel i, inside the image */
RT_TP_HD RectifySource rectify_source(const RectifyBounds &b, uint64_t i) {
    if (b.valid != nullptr && b.valid[i * b.valid_stride] == 0u) return RectifySource::none();
    const float *c = b.color + i * b.color_stride;
    RectifySource q = {{c[0], c[1], c[2], 0.0f}, 0u};
    q.x[3] = temporal_luminance(q.x[0], q.x[1], q.x[2]);
    if (b.object) q.object = b.object[i * b.object_stride];
    return q;
}

/* does source q count for the centre p (which is not none) */
RT_TP_HD bool rectify_counts(const RectifySource &p, const RectifySource &q) { return !q.is_none() && q.object == p.object; }

struct RectifySums {
    float s[4];
    uint32_t k;
};

/* pass 1, step 1, for a source that counts */
RT_TP_HD void rectify_sum(RectifySums &a, const RectifySource &q) {
    for (int j = 0; j < 4; ++j) a.s[j] = a.s[j] + q.x[j];
    a.k += 1u;
}

/* pass 2, step 3, for the same source */
RT_TP_HD void rectify_deviation(float (&v)[4], const float (&mean)[4], const RectifySource &q) {
    for (int j = 0; j < 4; ++j) {
        const float d = q.x[j] - mean[j];
        v[j] = v[j] + d * d;
    }
}

/* The two passes over the (2 R + 1)^2 window of a centre p that counts itself: source(dr, dc) is the window's source, none() where there
 * is none.  Which sources count is decided once, in pass 1, and remembered as a bit per tap.  R is a constant so that a row's taps unroll. */
template <int R, class SourceAt>
RT_TP_HD void rectify_window(const RectifySource &p, float gamma, SourceAt source, float (&lo)[4], float (&hi)[4]) {
    RectifySums a = {{0.0f, 0.0f, 0.0f, 0.0f}, 0u};
    uint64_t counted = 0u;
    int tap = 0;
    RT_RECTIFY_ROW_BY_ROW
    for (int dr = -R; dr <= R; ++dr)
        for (int dc = -R; dc <= R; ++dc, ++tap) {
            const RectifySource q = source(dr, dc);
            if (!rectify_counts(p, q)) continue;
            counted |= 1ull << tap;
            rectify_sum(a, q);
        }
    const float kf = (float)a.k;
    float mean[4], v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = 0; j < 4; ++j) mean[j] = a.s[j] / kf;
    tap = 0;
    RT_RECTIFY_ROW_BY_ROW
    for (int dr = -R; dr <= R; ++dr)
        for (int dc = -R; dc <= R; ++dc, ++tap)
            if (counted >> tap & 1u) rectify_deviation(v, mean, source(dr, dc));
    for (int j = 0; j < 4; ++j) {
        const float var = svgf_vpos(v[j] / kf);
        const float sd = rtdm::f_sqrt(var);
        const float half = gamma * sd;
        lo[j] = mean[j] - half;
        hi[j] = mean[j] + half;
    }
}

/* the window of the call's radius (1 .. 3, checked by the entry point) */
template <class SourceAt>
RT_TP_HD void rectify_box(const RectifyBounds &b, const RectifySource &p, SourceAt source, float (&lo)[4], float (&hi)[4]) {
    if (p.is_none()) { /* its history resets anyway */
        for (int j = 0; j < 4; ++j) lo[j] = -__builtin_inff(), hi[j] = __builtin_inff();
    } else if (b.radius == 1) {
        rectify_window<1>(p, b.gamma, source, lo, hi);
    } else if (b.radius == 2) {
        rectify_window<2>(p, b.gamma, source, lo, hi);
    } else {
        rectify_window<3>(p, b.gamma, source, lo, hi);
    }
}

/* pixel (r, c), every source read from global memory: the CPU form */
inline void rectify_bounds_pixel(const RectifyBounds &b, uint32_t r, uint32_t c) {
    const uint64_t i = (uint64_t)r * b.cols + c;
    rt_temporal_box &out = b.box[i];
    rectify_box(b, rectify_source(b, i), [&](int dr, int dc) {
        const int64_t qr = (int64_t)r + dr, qc = (int64_t)c + dc;
        if (qr < 0 || qr >= (int64_t)b.rows || qc < 0 || qc >= (int64_t)b.cols) return RectifySource::none();
        return rectify_source(b, (uint64_t)qr * b.cols + (uint64_t)qc);
    }, out.lo, out.hi);
}

/* ---- rt_temporal_accumulate_bounded ---- */

struct RectifyAccumulate {
    TemporalCall t;
    const rt_temporal_box *box;
    uint32_t clamped_length;
    uint32_t *clamped; /* may be null */
    RT_TP_HD uint64_t count() const { return t.count(); }
    RT_TP_HD void operator()(uint64_t i) const; /* rectify_pixel */
};

/* operation 1 and the first half of 2: x into [lo, hi]; a NaN x, or a NaN bound, compares false and passes */
RT_TP_HD float rectify_clamp(float x, float lo, float hi, uint32_t &changed) {
    if (x < lo) {
        changed += 1u;
        return lo;
    }
    if (x > hi) {
        changed += 1u;
        return hi;
    }
    return x;
}

/* the three operations between H = sum / bsum and the blend; returns the number of channels the clamp changed */
RT_TP_HD uint32_t rectify_history(TemporalHist &h, const float (&lo)[4], const float (&hi)[4], uint32_t clamped_length) {
    uint32_t changed = 0u;
    h.c0 = rectify_clamp(h.c0, lo[0], hi[0], changed);
    h.c1 = rectify_clamp(h.c1, lo[1], hi[1], changed);
    h.c2 = rectify_clamp(h.c2, lo[2], hi[2], changed);
    const uint32_t before = changed;
    const float m1 = rectify_clamp(h.m1, lo[3], hi[3], changed);
    if (changed != before) { /* the variance is kept while the mean is shifted */
        h.m2 = h.m2 + (m1 * m1 - h.m1 * h.m1);
        h.m1 = m1;
    }
    if (changed != 0u && clamped_length != 0u && h.n > clamped_length) h.n = clamped_length;
    return changed;
}

/* output pixel i: rt_temporal_accumulate's pixel with the box between its gather and its blend */
RT_TP_HD void rectify_pixel(const RectifyAccumulate &a, uint64_t i) {
    const TemporalPix p = temporal_load(a.t, i);
    float lo[4], hi[4];
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 *b = reinterpret_cast<const uint4 *>(a.box + i); /* 32 bytes, 16-byte aligned: two 128-bit loads, issued before the gather */
    const uint4 l = b[0], u = b[1];
    lo[0] = temporal_float(l.x), lo[1] = temporal_float(l.y), lo[2] = temporal_float(l.z), lo[3] = temporal_float(l.w);
    hi[0] = temporal_float(u.x), hi[1] = temporal_float(u.y), hi[2] = temporal_float(u.z), hi[3] = temporal_float(u.w);
#else
    for (int j = 0; j < 4; ++j) lo[j] = a.box[i].lo[j], hi[j] = a.box[i].hi[j];
#endif
    TemporalHist h;
    uint32_t changed = 0u;
    if (temporal_gather(a.t, i, p, h)) {
        changed = rectify_history(h, lo, hi, a.clamped_length);
        temporal_blend(a.t, i, p, h);
    } else {
        temporal_reset(a.t, i, p);
    }
    if (a.clamped) a.clamped[i] = changed;
}
RT_TP_HD void RectifyAccumulate::operator()(uint64_t i) const { rectify_pixel(*this, i); }

/* ---- rt_temporal_feedback ---- */

struct RectifyFeedback {
    const float *color;
    const uint32_t *valid; /* may be null */
    uint32_t color_stride, valid_stride;
    uint64_t n;
    rt_temporal_pixel *history;
    RT_TP_HD uint64_t count() const { return n; }
    RT_TP_HD void operator()(uint64_t i) const; /* rectify_feedback_pixel */
};

/* record i: the colour's raw words over the record's three colour words; the moments, the length and the reserved words keep their bits */
RT_TP_HD void rectify_feedback_pixel(const RectifyFeedback &f, uint64_t i) {
    if (f.valid != nullptr && f.valid[i * f.valid_stride] == 0u) return;
    if (f.history[i].length == 0u) return;
    const uint32_t *c = reinterpret_cast<const uint32_t *>(f.color) + i * f.color_stride;
#if defined(__HIP_DEVICE_COMPILE__)
    uint4 *h = reinterpret_cast<uint4 *>(f.history + i); /* the record's first 16 bytes: one 128-bit load, one 128-bit store */
    const uint4 w = h[0];
    h[0] = make_uint4(c[0], c[1], c[2], w.w);
#else
    uint32_t *h = reinterpret_cast<uint32_t *>(f.history + i);
    h[0] = c[0], h[1] = c[1], h[2] = c[2];
#endif
}
RT_TP_HD void RectifyFeedback::operator()(uint64_t i) const { rectify_feedback_pixel(*this, i); }

/* ---- the arguments of the entry points (rt_query_args.h): the checks in the order include/rt_amd.h states.  The device forms read and
 * write a box, and a record's first 16 bytes, as 128-bit words. ---- */

/* rt_temporal_bounds, rt_temporal_bounds_host and rt_temporal_bounds_cpu */
struct RectifyBoundsArgs {
    const float *color; uint32_t color_stride;
    const uint32_t *object; uint32_t object_stride;
    const uint32_t *valid; uint32_t valid_stride;
    const rt_bounds_params *params; uint32_t rows, cols; rt_temporal_box *box;

    const char *limits(QueryForm form, int *status) const {
        *status = RT_ERR_INVALID_ARGUMENT;
        if (const char *bad = limits_image(rows, cols)) {
            *status = RT_ERR_UNSUPPORTED;
            return bad;
        }
        if (empty()) return nullptr;
        if (!params) return "null params";
        if (!color) return "null color pointer";
        if (!box) return "null box pointer";
        if (color_stride < 3u) return "color_stride must be at least 3 words";
        if (object && object_stride < 1u) return "object_stride must be at least 1 word";
        if (valid && valid_stride < 1u) return "valid_stride must be at least 1 word";
        if (params->radius < 1u || params->radius > (uint32_t)RT_RECTIFY_MAX_RADIUS) return "radius must be 1, 2 or 3";
        if (!(params->gamma >= 0.0f && params->gamma < __builtin_inff())) return "gamma must be >= 0 and finite";
        if (params->flags != 0u) return "flags: unknown bits (none is defined)";
        if (query_misaligned(form, box)) return "box must be 16-byte aligned";
        return nullptr;
    }

    bool empty() const { return rows == 0u || cols == 0u; }

    template <class Stage>
    void arrays(Stage &s) {
        const size_t n = (size_t)rows * cols;
        color = s.plane(color, n, color_stride, 3u);
        object = s.plane(object, n, object_stride, 1u);
        valid = s.plane(valid, n, valid_stride, 1u);
        box = s.out(box, n * sizeof(rt_temporal_box));
    }

    RectifyBounds call() const {
        RectifyBounds b;
        b.color = color, b.object = object, b.valid = valid;
        b.color_stride = color_stride, b.object_stride = object_stride, b.valid_stride = valid_stride;
        b.rows = rows, b.cols = cols, b.radius = (int)params->radius, b.gamma = params->gamma, b.box = box;
        return b;
    }
};

/* rt_temporal_accumulate_bounded, its _host and its _cpu form: rt_temporal_accumulate's arguments and checks, then the box's */
struct RectifyAccumulateArgs : TemporalAccumulateArgs {
    const rt_temporal_box *box;
    uint32_t clamped_length;
    uint32_t *clamped;

    const char *limits(QueryForm form, int *status) const {
        if (const char *bad = TemporalAccumulateArgs::limits(form, status)) return bad;
        if (empty()) return nullptr;
        if (!box) return "null box pointer";
        if (query_misaligned(form, box)) return "box must be 16-byte aligned";
        if (clamped_length > params->max_length) return "clamped_length must not exceed max_length (0: the length is not cut)";
        return nullptr;
    }

    template <class Stage>
    void arrays(Stage &s) {
        const size_t n = (size_t)rows * cols;
        TemporalAccumulateArgs::arrays(s);
        box = s.in(box, n * sizeof(rt_temporal_box));
        clamped = s.out(clamped, n * sizeof(uint32_t));
    }

    RectifyAccumulate call() const { return {TemporalAccumulateArgs::call(), box, clamped_length, clamped}; }
};

/* rt_temporal_feedback, rt_temporal_feedback_host and rt_temporal_feedback_cpu */
struct RectifyFeedbackArgs {
    const float *color; uint32_t color_stride;
    const uint32_t *valid; uint32_t valid_stride;
    uint32_t rows, cols; rt_temporal_pixel *history;

    const char *limits(QueryForm form, int *status) const {
        *status = RT_ERR_INVALID_ARGUMENT;
        if (const char *bad = limits_image(rows, cols)) {
            *status = RT_ERR_UNSUPPORTED;
            return bad;
        }
        if (empty()) return nullptr;
        if (!color) return "null color pointer";
        if (!history) return "null history pointer";
        if (color_stride < 3u) return "color_stride must be at least 3 words";
        if (valid && valid_stride < 1u) return "valid_stride must be at least 1 word";
        if (query_misaligned(form, history)) return "history must be 16-byte aligned";
        return nullptr;
    }

    bool empty() const { return rows == 0u || cols == 0u; }

    template <class Stage>
    void arrays(Stage &s) {
        const size_t n = (size_t)rows * cols;
        color = s.plane(color, n, color_stride, 3u);
        valid = s.plane(valid, n, valid_stride, 1u);
        history = s.inout(history, n * sizeof(rt_temporal_pixel));
    }

    RectifyFeedback call() const { return {color, valid, color_stride, valid_stride, (uint64_t)rows * cols, history}; }
};

} /* namespace rt */

#endif /* RT_RECTIFY_H */

