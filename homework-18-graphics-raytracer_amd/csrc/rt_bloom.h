/*
 * rt_bloom.h — the arithmetic of the bloom queries (include/rt_amd.h "bloom queries"), written once for the host (librt_host.so:
 * rt_bloom_cpu) and the device (rt_bloom_query.hip, both kernel forms).  Every function is a sequence of single f32 operations in the
 * order the header comment of the block gives; both libraries are built with -ffp-contract=off and the divide is correctly rounded on
 * either side, so host and device agree bit for bit.
 *
 * A call is 2 L steps (bloom_steps): L down steps (BloomDown; the first sees the colour through the bright pass), L - 1 up-and-add
 * steps (BloomUp) and the composite (BloomComposite).  Each is an Op of rt_image_kernel.h — count() and operator()(i), one output pixel
 * per element, every tap read from global memory — which librt_host.so runs in a plain loop and the plain kernel form one thread per
 * element.  The down step's pixel is bloom_down_pixel, handed its 4 x 4 sources by whoever calls it: the Op reads them from global
 * memory (bloom_source, which clamps), the tiled kernel from its staged window.
 */
#ifndef RT_BLOOM_H
#define RT_BLOOM_H

#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_atrous.h"
#include "rt_luma.h"

namespace rt {

struct BloomRgb {
    float c0, c1, c2;
};

/* clamp(i, n) of the definition: an index into 0 .. n - 1 */
RT_AT_HD uint32_t bloom_clamp(int64_t i, uint32_t n) { return i < 0 ? 0u : (i >= (int64_t)n ? n - 1u : (uint32_t)i); }

/* the next level's size along one axis */
inline uint32_t bloom_half(uint32_t n) { return n / 2u + (n & 1u); }

/* ---- step 1: the bright pass ---- */

struct BloomBright {
    float w0, w1, w2; /* rt_luma.h's row, computed on the host */
    float threshold, knee;
};

RT_AT_HD bool bloom_finite(float c) { return c - c == 0.0f; }

RT_AT_HD BloomRgb bloom_bright(const BloomBright &b, float c0, float c1, float c2) {
    const BloomRgb black = {0.0f, 0.0f, 0.0f};
    const float l = (b.w0 * c0 + b.w1 * c1) + b.w2 * c2;
    if (!(bloom_finite(c0) && bloom_finite(c1) && bloom_finite(c2)) || !(l > 0.0f)) return black;
    const float s = l - b.threshold;
    float m = s;
    if (b.knee > 0.0f) {
        const float t = __builtin_fminf(__builtin_fmaxf(s + b.knee, 0.0f), 2.0f * b.knee);
        const float q = (t * t) / (4.0f * b.knee);
        m = __builtin_fmaxf(s, q);
    }
    if (!(m > 0.0f)) return black;
    const float g = m / l;
    return {c0 * g, c1 * g, c2 * g};
}

/* ---- step 2: down ---- */

/* D_j from S: S is the colour seen through the bright pass (bright != 0; src_stride the caller's) or D_{j-1} (compact) */
struct BloomDown {
    const float *src;
    float *dst;
    uint32_t src_stride, src_rows, src_cols;
    uint32_t rows, cols; /* of dst */
    uint32_t bright;
    BloomBright b;
    RT_AT_HD uint64_t count() const { return (uint64_t)rows * cols; }
    RT_AT_HD void operator()(uint64_t i) const;
};

/* source pixel (r, c) of a down step, wherever it lies: the replicated edge */
RT_AT_HD BloomRgb bloom_source(const BloomDown &d, int64_t r, int64_t c) {
    const uint64_t qi = (uint64_t)bloom_clamp(r, d.src_rows) * d.src_cols + (uint64_t)bloom_clamp(c, d.src_cols);
    const float *s = d.src + qi * d.src_stride;
    if (d.bright) return bloom_bright(d.b, s[0], s[1], s[2]);
    return {s[0], s[1], s[2]};
}

/* [1 3 3 1], mirror-symmetric: the taps swapped end for end give the same bits */
RT_AT_HD float bloom_tent4(float s0, float s1, float s2, float s3) { return (s0 + 3.0f * s1) + (3.0f * s2 + s3); }

/* Output pixel (r, c) of a down step: source(kr, kc) is the source at row clamp(2 r - 1 + kr), column clamp(2 c - 1 + kc) */
template <class SourceAt>
RT_AT_HD void bloom_down_pixel(const BloomDown &d, uint32_t r, uint32_t c, SourceAt source) {
    float h0[4], h1[4], h2[4];
    for (int kr = 0; kr < 4; ++kr) {
        const BloomRgb s0 = source(kr, 0), s1 = source(kr, 1), s2 = source(kr, 2), s3 = source(kr, 3);
        h0[kr] = bloom_tent4(s0.c0, s1.c0, s2.c0, s3.c0);
        h1[kr] = bloom_tent4(s0.c1, s1.c1, s2.c1, s3.c1);
        h2[kr] = bloom_tent4(s0.c2, s1.c2, s2.c2, s3.c2);
    }
    float *o = d.dst + 3u * ((uint64_t)r * d.cols + c);
    o[0] = bloom_tent4(h0[0], h0[1], h0[2], h0[3]) * 0.015625f;
    o[1] = bloom_tent4(h1[0], h1[1], h1[2], h1[3]) * 0.015625f;
    o[2] = bloom_tent4(h2[0], h2[1], h2[2], h2[3]) * 0.015625f;
}

RT_AT_HD void BloomDown::operator()(uint64_t i) const {
    const uint32_t r = (uint32_t)(i / cols), c = (uint32_t)(i - (uint64_t)r * cols);
    const BloomDown &d = *this;
    bloom_down_pixel(d, r, c, [&](int kr, int kc) { return bloom_source(d, 2 * (int64_t)r - 1 + kr, 2 * (int64_t)c - 1 + kc); });
}

/* ---- steps 3 and 4: up ---- */

/* a compact plane of the pyramid */
struct BloomPlane {
    float *p;
    uint32_t rows, cols;
};

/* up(X)(r, c) */
RT_AT_HD BloomRgb bloom_up(const BloomPlane &x, uint32_t r, uint32_t c) {
    const uint32_t near_r = r >> 1, near_c = c >> 1;
    const uint32_t far_r = bloom_clamp((int64_t)near_r + ((r & 1u) ? 1 : -1), x.rows), far_c = bloom_clamp((int64_t)near_c + ((c & 1u) ? 1 : -1), x.cols);
    const float *nn = x.p + 3u * ((uint64_t)near_r * x.cols + near_c), *nf = x.p + 3u * ((uint64_t)near_r * x.cols + far_c);
    const float *fn = x.p + 3u * ((uint64_t)far_r * x.cols + near_c), *ff = x.p + 3u * ((uint64_t)far_r * x.cols + far_c);
    float u[3];
    for (int k = 0; k < 3; ++k) {
        const float h_near = 3.0f * nn[k] + nf[k], h_far = 3.0f * fn[k] + ff[k];
        u[k] = (3.0f * h_near + h_far) * 0.0625f;
    }
    return {u[0], u[1], u[2]};
}

/* U_j = D_j + up(U_{j+1}), over D_j in place: a pixel reads and writes its own words of `fine` only */
struct BloomUp {
    BloomPlane coarse, fine;
    RT_AT_HD uint64_t count() const { return (uint64_t)fine.rows * fine.cols; }
    RT_AT_HD void operator()(uint64_t i) const {
        const uint32_t r = (uint32_t)(i / fine.cols), c = (uint32_t)(i - (uint64_t)r * fine.cols);
        const BloomRgb u = bloom_up(coarse, r, c);
        float *o = fine.p + 3u * i;
        o[0] = o[0] + u.c0;
        o[1] = o[1] + u.c1;
        o[2] = o[2] + u.c2;
    }
};

/* out = c + g up(U_1); out may be the colour itself (color_stride 3): a pixel reads its own colour only */
struct BloomComposite {
    const float *color;
    float *out;
    BloomPlane coarse;
    uint32_t color_stride, rows, cols;
    float g; /* intensity / (float)L */
    RT_AT_HD uint64_t count() const { return (uint64_t)rows * cols; }
    RT_AT_HD void operator()(uint64_t i) const {
        const uint32_t r = (uint32_t)(i / cols), c = (uint32_t)(i - (uint64_t)r * cols);
        const BloomRgb u = bloom_up(coarse, r, c);
        const float *s = color + i * color_stride;
        const float c0 = s[0], c1 = s[1], c2 = s[2];
        float *o = out + 3u * i;
        o[0] = c0 + g * u.c0;
        o[1] = c1 + g * u.c1;
        o[2] = c2 + g * u.c2;
    }
};

/* ---- the call ---- */

inline bool bloom_levels_ok(uint32_t n_levels) { return n_levels >= 1u && n_levels <= RT_BLOOM_MAX_LEVELS; }

/* step 5: D_1 .. D_L compact, one after the other */
inline size_t bloom_temp_bytes(uint32_t rows, uint32_t cols, uint32_t n_levels) {
    if (!bloom_levels_ok(n_levels)) return 0;
    size_t words = 0;
    for (uint32_t j = 1; j <= n_levels; ++j) {
        rows = bloom_half(rows), cols = bloom_half(cols);
        words += (size_t)rows * cols * 3u;
    }
    return words * sizeof(float);
}

/* The arguments of rt_bloom, rt_bloom_host and rt_bloom_cpu (rt_query_args.h); the checks in the order include/rt_amd.h states.  temp is
 * the caller's scratch; the _host form passes null and its round trip makes its own. */
struct BloomArgs {
    const float *color; uint32_t color_stride;
    const rt_bloom_params *params; uint32_t rows, cols;
    float *temp, *out;

    const char *limits(QueryForm form, int *status) const {
        *status = RT_ERR_INVALID_ARGUMENT;
        if (!params) return "null params";
        if (!bloom_levels_ok(params->n_levels)) return "n_levels must be 1 .. 8";
        if (!(params->threshold >= 0.0f)) return "threshold must be >= 0 (+inf: nothing glows)";
        if (!(params->knee >= 0.0f) || !bloom_finite(params->knee)) return "knee must be finite and >= 0";
        if (!(params->intensity >= 0.0f) || !bloom_finite(params->intensity)) return "intensity must be finite and >= 0";
        if (color_stride < 3u) return "color_stride must be at least 3 words";
        if (const char *bad = limits_image(rows, cols)) return bad;
        if (empty()) return nullptr;
        if (!color) return "null color pointer";
        if (!out) return "null out pointer";
        if (query_takes_temp(form) && !temp) return "null temp pointer";
        if (out == color && color_stride != 3u) return "out may be color only with color_stride 3";
        return nullptr;
    }

    bool empty() const { return rows == 0u || cols == 0u; }

    template <class Stage>
    void arrays(Stage &s) {
        const size_t n = (size_t)rows * cols;
        color = s.plane(color, n, color_stride, 3u);
        temp = static_cast<float *>(s.scratch(bloom_temp_bytes(rows, cols, params->n_levels)));
        out = s.out(out, n * 3u * sizeof(float));
    }

    /* level j of the pyramid: 0 is the image itself (no plane of temp), 1 .. L are D_j / U_j in temp */
    BloomPlane level(uint32_t j) const {
        BloomPlane p = {nullptr, rows, cols};
        float *at = temp;
        for (uint32_t k = 1; k <= j; ++k) {
            p.rows = bloom_half(p.rows), p.cols = bloom_half(p.cols);
            p.p = at;
            at += (size_t)p.rows * p.cols * 3u;
        }
        return p;
    }

    /* the down step that makes D_j, j = 1 .. L */
    BloomDown down(uint32_t j) const {
        const BloomPlane from = level(j - 1u), to = level(j);
        BloomDown d;
        d.src = j == 1u ? color : from.p, d.src_stride = j == 1u ? color_stride : 3u;
        d.src_rows = from.rows, d.src_cols = from.cols;
        d.dst = to.p, d.rows = to.rows, d.cols = to.cols;
        d.bright = j == 1u ? 1u : 0u;
        float row[3];
        luma_row(row);
        d.b = {row[0], row[1], row[2], params->threshold, params->knee};
        return d;
    }

    /* the up-and-add step that makes U_j, j = L - 1 .. 1 */
    BloomUp up(uint32_t j) const { return {level(j + 1u), level(j)}; }

    BloomComposite composite() const {
        return {color, out, level(1u), color_stride, rows, cols, params->intensity / (float)params->n_levels};
    }
};

/* The 2 L steps of a call in their order: down(D) for the L down steps, each(Op) for the up-and-add steps and the composite; either
 * returns false to stop the call there. */
template <class Down, class Each>
inline bool bloom_steps(const BloomArgs &a, Down down, Each each) {
    const uint32_t L = a.params->n_levels;
    for (uint32_t j = 1; j <= L; ++j)
        if (!down(a.down(j))) return false;
    for (uint32_t j = L - 1u; j >= 1u; --j)
        if (!each(a.up(j))) return false;
    return each(a.composite());
}

} /* namespace rt */

#endif /* RT_BLOOM_H */
