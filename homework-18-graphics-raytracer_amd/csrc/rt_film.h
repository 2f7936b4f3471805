/*
 * rt_film.h — the arithmetic of the film queries (include/rt_amd.h "film queries"), written once for the host (librt_host.so:
 * rt_film_offsets_host / rt_film_splat_host) and the device (rt_film_query.hip).  Every function is a sequence of single f32 or u32
 * operations in the order the header comment of the block gives; both libraries are built with -ffp-contract=off, the divides are
 * correctly rounded on either side, and constant expressions (16.0f / 3.0f, ...) are folded in IEEE f32 by either compiler — so the
 * host and the device forms agree bit for bit.
 */
#ifndef RT_FILM_H
#define RT_FILM_H

#include <math.h>
#include <stdint.h>

#include "../../include/rt_amd.h"

#if defined(__HIPCC__)
#define RT_FILM_HD __host__ __device__ __forceinline__
#else
#define RT_FILM_HD inline
#endif

namespace rt {

RT_FILM_HD uint32_t film_mix(uint32_t v) {
    v ^= v >> 16;
    v *= 0x7feb352du;
    v ^= v >> 15;
    v *= 0x846ca68bu;
    v ^= v >> 16;
    return v;
}

/* u in [0, 1) of (global pixel, seed, sample, axis): 24 bits of the counter hash */
RT_FILM_HD float film_u(uint32_t pixel, uint32_t seed, uint32_t s, uint32_t axis) {
    const uint32_t h = film_mix(film_mix(pixel + seed) ^ (2u * s + axis));
    return (float)(h >> 8) * 5.9604644775390625e-8f; /* 2^-24 */
}

/* the side k of a stratified pattern of spp = k * k samples, 1 <= k <= 8; 0: spp is no such square */
inline uint32_t film_strata(uint32_t spp) {
    for (uint32_t k = 1u; k <= 8u; ++k)
        if (k * k == spp) return k;
    return 0u;
}

/* one coordinate of sample s of a pixel; k: film_strata(spp) (used by RT_FILM_STRATIFIED only) */
RT_FILM_HD float film_offset(uint32_t pattern, uint32_t k, uint32_t pixel, uint32_t seed, uint32_t s, uint32_t axis) {
    if (pattern == RT_FILM_CENTER) return 0.0f;
    const float u = film_u(pixel, seed, s, axis);
    if (pattern == RT_FILM_UNIFORM) return u - 0.5f;
    const uint32_t cell = axis == 0u ? s % k : s / k;
    return ((float)cell + u) / (float)k - 0.5f;
}

RT_FILM_HD int film_reach(float radius) { return (int)ceilf(radius + 0.5f); }

/* the reconstruction filter along one axis, for -radius <= d < radius */
RT_FILM_HD float film_filter(uint32_t filter, float d, float radius) {
    if (filter == RT_FILM_BOX) return 1.0f;
    if (filter == RT_FILM_TENT) return 1.0f - fabsf(d) / radius;
    const float x = 2.0f * fabsf(d) / radius; /* Mitchell-Netravali, B = C = 1/3 */
    if (x < 1.0f) return ((7.0f * x - 12.0f) * x * x + 16.0f / 3.0f) / 6.0f;
    return (((-7.0f / 3.0f * x + 12.0f) * x - 20.0f) * x + 32.0f / 3.0f) / 6.0f;
}

/* the running (sum, weight) of one output pixel: PhotonAccumulator::accumulate_weight (photon.rs:30-33) */
struct FilmAcc {
    float s0, s1, s2, w;
};

/* One source sample seen from an output pixel (dr, dc) away: dx, dy its sub-pixel offset, p0..p2 its radiance.  Steps 6-8 of the
 * definition: the half-open support test, then w = f(ddx) * f(ddy), sum_c = sum_c + photon_c * w (the product rounded before the
 * add), weight = weight + w. */
RT_FILM_HD bool film_covers(int dr, int dc, float dx, float dy, float radius, float *ddx, float *ddy) {
    *ddx = (float)dc + dx;
    *ddy = (float)dr + dy;
    return -radius <= *ddx && *ddx < radius && -radius <= *ddy && *ddy < radius;
}
RT_FILM_HD void film_apply(FilmAcc &a, uint32_t filter, float radius, float ddx, float ddy, float p0, float p1, float p2) {
    const float w = film_filter(filter, ddx, radius) * film_filter(filter, ddy, radius);
    a.s0 = a.s0 + p0 * w;
    a.s1 = a.s1 + p1 * w;
    a.s2 = a.s2 + p2 * w;
    a.w = a.w + w;
}

/* ---- the splat: one walk over two layouts ----
 * A layout says where sample s of source pixel q lives and how many samples q has; everything else of the gather is written once.
 *   ragged                 a constant: counts differ from pixel to pixel (the tiled kernel then stages the ranges and skips an s nobody has)
 *   s_end()                no pixel has a sample s at or beyond it
 *   range(q, &lo)          the samples of q; lo: what record() needs of q, below 2^32 (the tiled kernel keeps it in one LDS word)
 *   record(lo, s)          the index of sample s < range(q, &lo) in samples / valid / offsets
 * UniformLayout is rt_film_splat's sample-major record s * n + q; rt_adaptive.h's ListedLayout is the pixel-major list's lo_q + s. */
struct UniformLayout {
    static constexpr bool ragged = false;
    const float *samples;
    const unsigned char *valid; /* may be null */
    const float *offsets;
    uint64_t n; /* rows * cols < 2^32 */
    uint32_t spp;
    RT_FILM_HD uint32_t s_end() const { return spp; }
    RT_FILM_HD uint32_t range(uint64_t q, uint64_t *lo) const {
        *lo = q;
        return spp;
    }
    RT_FILM_HD uint64_t record(uint64_t lo, uint32_t s) const { return (uint64_t)s * n + lo; }
};

/* one splat call (0 < radius <= 4 and rows * cols < 2^32, checked by the entry points) */
template <class Layout>
struct FilmSplat {
    Layout layout;
    float *sum, *weight;
    uint32_t rows, cols, filter;
    float radius;
};

/* a dx that fails the support test of film_covers for every output pixel */
#define RT_FILM_NAN 0x7fc00000u

/* Output pixel i = r * cols + c: the walk of the definition straight from the arrays — s outermost, then dr, then dc, ascending.  The CPU
 * forms and the plain kernel; apply(a, ddx, ddy, p0, p1, p2) is film_apply with the caller's filter (a constant in a kernel). */
template <class Layout, class Apply>
RT_FILM_HD void film_splat_pixel(const FilmSplat<Layout> &p, uint64_t i, Apply apply) {
    const Layout &L = p.layout;
    const uint32_t r = (uint32_t)(i / p.cols), c = (uint32_t)(i - (uint64_t)r * p.cols);
    const int reach = film_reach(p.radius);
    FilmAcc a = {p.sum[3u * i], p.sum[3u * i + 1u], p.sum[3u * i + 2u], p.weight[i]};
    for (uint32_t s = 0; s < L.s_end(); ++s)
        for (int dr = -reach; dr <= reach; ++dr) {
            const int64_t qr = (int64_t)r + dr;
            if (qr < 0 || qr >= (int64_t)p.rows) continue;
            for (int dc = -reach; dc <= reach; ++dc) {
                const int64_t qc = (int64_t)c + dc;
                if (qc < 0 || qc >= (int64_t)p.cols) continue;
                uint64_t lo;
                if (s >= L.range((uint64_t)qr * p.cols + (uint64_t)qc, &lo)) continue;
                const uint64_t rec = L.record(lo, s);
                if (L.valid != nullptr && L.valid[rec] == 0u) continue;
                float ddx, ddy;
                if (!film_covers(dr, dc, L.offsets[2u * rec], L.offsets[2u * rec + 1u], p.radius, &ddx, &ddy)) continue;
                apply(a, ddx, ddy, L.samples[3u * rec], L.samples[3u * rec + 1u], L.samples[3u * rec + 2u]);
            }
        }
    p.sum[3u * i] = a.s0;
    p.sum[3u * i + 1u] = a.s1;
    p.sum[3u * i + 2u] = a.s2;
    p.weight[i] = a.w;
}

/* a splat as an element loop over its output pixels, the filter a constant (the plain kernel) */
template <uint32_t FILTER, class Layout>
struct FilmSplatEach {
    FilmSplat<Layout> p;
    RT_FILM_HD uint64_t count() const { return (uint64_t)p.rows * p.cols; }
    RT_FILM_HD void operator()(uint64_t i) const {
        film_splat_pixel(p, i, [&](FilmAcc &a, float ddx, float ddy, float p0, float p1, float p2) { film_apply(a, FILTER, p.radius, ddx, ddy, p0, p1, p2); });
    }
};

/* the CPU form of a splat: every output pixel in turn */
template <class Layout>
inline void film_splat_cpu(const FilmSplat<Layout> &p) {
    for (uint64_t i = 0; i < (uint64_t)p.rows * p.cols; ++i)
        film_splat_pixel(p, i, [&](FilmAcc &a, float ddx, float ddy, float p0, float p1, float p2) { film_apply(a, p.filter, p.radius, ddx, ddy, p0, p1, p2); });
}

/* the pixels of a frame's tile, or 0 for a frame that is none (include/rt_amd.h rt_frame) */
inline uint64_t film_frame_pixels(const rt_frame *f) {
    if (!(f && f->width > 0 && f->height > 0 && f->y_step >= 1 && f->x0 < f->x1 && f->y0 < f->y1 && f->x1 <= f->width && f->y1 <= f->height)) return 0u;
    return (((uint64_t)f->y1 - f->y0 + f->y_step - 1u) / f->y_step) * (uint64_t)(f->x1 - f->x0);
}

/* what a sample position needs of a frame or tile (one that film_frame_pixels accepts): the compact pixel row * cols + col has the
 * GLOBAL index y * width + x, so the tiles of one frame agree with the full frame */
struct FilmTile {
    uint32_t cols, rows, x0, y0, y_step, width;
};
inline FilmTile film_tile(const rt_frame *f) {
    const uint32_t cols = f->x1 - f->x0;
    return {cols, (uint32_t)(film_frame_pixels(f) / cols), f->x0, f->y0, f->y_step, f->width};
}
RT_FILM_HD uint32_t film_global_pixel(const FilmTile &t, uint32_t row, uint32_t col) { return (t.y0 + row * t.y_step) * t.width + (t.x0 + col); }

/* the argument limits of rt_film_offsets and rt_film_offsets_host; null: all in range.  *unsupported: the refusal is about size */
inline const char *film_offsets_limits(const rt_frame *frame, uint32_t spp, uint32_t pattern, bool *unsupported) {
    *unsupported = false;
    if (!frame) return "null frame";
    const uint64_t pixels = film_frame_pixels(frame);
    if (pixels == 0u) return "bad frame (need 0 <= x0 < x1 <= width, 0 <= y0 < y1 <= height, y_step >= 1)";
    if (spp < 1u) return "spp must be at least 1";
    if (pattern != RT_FILM_CENTER && pattern != RT_FILM_UNIFORM && pattern != RT_FILM_STRATIFIED)
        return "unknown pattern (RT_FILM_CENTER, RT_FILM_UNIFORM or RT_FILM_STRATIFIED)";
    if (pattern == RT_FILM_STRATIFIED && film_strata(spp) == 0u) return "a stratified pattern needs spp = k * k with 1 <= k <= 8";
    if (pixels >= (1ull << 32) || pixels * spp >= (1ull << 32)) {
        *unsupported = true;
        return "2^32 samples or more (make them in several calls)";
    }
    return nullptr;
}

/* the argument limits of rt_film_splat and rt_film_splat_host; null: all in range */
inline const char *film_splat_limits(uint64_t rows, uint64_t cols, uint32_t spp, uint32_t filter, float radius) {
    if (filter != RT_FILM_BOX && filter != RT_FILM_TENT && filter != RT_FILM_MITCHELL) return "unknown filter (RT_FILM_BOX, RT_FILM_TENT or RT_FILM_MITCHELL)";
    if (!(radius > 0.0f && radius <= 4.0f)) return "radius must be in (0, 4] pixels";
    if (spp < 1u) return "spp must be at least 1";
    if (rows >= (1ull << 32) || cols >= (1ull << 32) || rows * cols >= (1ull << 32)) return "2^32 pixels or more";
    return nullptr;
}

} /* namespace rt */

#endif /* RT_FILM_H */
