/*
 * rt_atrous.h — what the two A-Trous filters (rt_denoise.h, rt_svgf.h) and the variance estimate share, written once for the host
 * (librt_host.so) and the device (rt_atrous_kernel.h): the guide planes and their four readers, the normal and position weight terms
 * and e(x), the schedule of a call's levels, the pieces of the argument checks, and atrous_pixel — THE 5 x 5 source walk with holes
 * over global memory.  A filter is a policy type (DenoiseFilter, SvgfFilter) that supplies
 *     Level, Pix, Acc, Context      one level of a call (an AtrousLevel and its own planes); what the filter knows of a pixel, which is
 *                                   also an entry of the staged tile; the sums of a walk; what a walk needs of its centre beyond p
 *     load(L, i)                    the Pix of pixel i, inside the image and valid
 *     context(L, r, c)              the Context of the centre (r, c)
 *     tap(L, a, p, q, k, dr, dc)    one source q into a
 *     store(L, i, filtered, a)      the outputs of pixel i; `filtered` is false for an invalid centre, whose sums are not looked at
 *     dead()                        the entry of a staged source that does not exist: tap skips it
 *     takes_taps(p)                 can a staged centre collect weight at all (the tiled kernel asks before it computes the Context)
 * and keeps the pixel arithmetic and its order of operations to itself.  Nothing here needs HIP.
 */
#ifndef RT_ATROUS_H
#define RT_ATROUS_H

#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_detmath.h"
#include "rt_query_args.h"

#if defined(__HIPCC__)
#define RT_AT_HD __host__ __device__ __forceinline__
#else
#define RT_AT_HD inline
#endif

namespace rt {

/* ---- the guide planes of a call: rt_denoise_guides as the caller gave them (any plane may be null) and the image they cover ---- */

struct GuidePlanes : rt_denoise_guides {
    uint32_t rows, cols;
};

inline void guide_planes(GuidePlanes &G, const rt_denoise_guides &g, uint32_t rows, uint32_t cols) {
    static_cast<rt_denoise_guides &>(G) = g;
    G.rows = rows, G.cols = cols;
}

/* shading normal and position of a pixel, six consecutive words of every pixel type */
struct GuidePoint {
    float n0, n1, n2, p0, p1, p2;
};

#define RT_DENOISE_ALBEDO_EPS 1e-3f

RT_AT_HD bool guide_valid(const GuidePlanes &G, uint64_t i) { return G.valid == nullptr || G.valid[i * G.valid_stride] != 0u; }

/* a plane that is null leaves its fields +0 (they are not looked at) */
RT_AT_HD GuidePoint guide_point(const GuidePlanes &G, uint64_t i) {
    GuidePoint q = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (G.normal) {
        const float *n = G.normal + i * G.normal_stride;
        q.n0 = n[0], q.n1 = n[1], q.n2 = n[2];
    }
    if (G.position) {
        const float *p = G.position + i * G.position_stride;
        q.p0 = p[0], q.p1 = p[1], q.p2 = p[2];
    }
    return q;
}

/* the albedo demodulation: the divide going in, the multiply coming out */
RT_AT_HD void guide_demodulate(const GuidePlanes &G, uint64_t i, float &c0, float &c1, float &c2) {
    const float *a = G.albedo + i * G.albedo_stride;
    c0 = c0 / (a[0] + RT_DENOISE_ALBEDO_EPS);
    c1 = c1 / (a[1] + RT_DENOISE_ALBEDO_EPS);
    c2 = c2 / (a[2] + RT_DENOISE_ALBEDO_EPS);
}
RT_AT_HD void guide_modulate(const GuidePlanes &G, uint64_t i, float &c0, float &c1, float &c2) {
    const float *a = G.albedo + i * G.albedo_stride;
    c0 = c0 * (a[0] + RT_DENOISE_ALBEDO_EPS);
    c1 = c1 * (a[1] + RT_DENOISE_ALBEDO_EPS);
    c2 = c2 * (a[2] + RT_DENOISE_ALBEDO_EPS);
}

/* ---- the weight terms ---- */

RT_AT_HD float denoise_dist2(float a0, float a1, float a2, float b0, float b1, float b2) {
    const float d0 = a0 - b0, d1 = a1 - b1, d2 = a2 - b2;
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

/* x, then the normal term, then the position term, each only where its plane is there */
RT_AT_HD float guide_terms(const GuidePlanes &G, float sn2, float sp2, float x, const GuidePoint &p, const GuidePoint &q) {
    if (G.normal) x = x + denoise_dist2(p.n0, p.n1, p.n2, q.n0, q.n1, q.n2) / sn2;
    if (G.position) x = x + denoise_dist2(p.p0, p.p1, p.p2, q.p0, q.p1, q.p2) / sp2;
    return x;
}

/* e(x) of the definitions, for an x >= 0; a tap whose x is not (NaN: a marked entry, or the caller's own) is skipped before it */
RT_AT_HD float atrous_e(float x) { return x > 100.0f ? 0.0f : (float)rtdm::exp_mid(-(double)x); }

/* the B3 spline {1/16, 1/4, 3/8, 1/4, 1/16} by tap index 0..4 (no table: the loops are unrolled and this folds to a literal) */
RT_AT_HD float denoise_h(int k) { return k == 2 ? 0.375f : (k == 1 || k == 3) ? 0.25f : 0.0625f; }

/* ---- the schedule of a call's levels ---- */

/* what a level of either filter has beyond its own colour planes */
struct AtrousLevel : GuidePlanes {
    int32_t step;   /* 1 << l */
    float sn2, sp2; /* the squared sigmas of the guide terms */
    uint32_t demod_in, demod_out;
};

/* levels still to come, and whether this one writes the outputs: they alternate so that the last level does */
struct AtrousTurn {
    uint32_t after;
    bool to_out;
};

/* level j (0-based) of a call with Params p (rt_denoise_params, rt_svgf_atrous_params): the first level demodulates in, the last one out */
template <class Params>
inline AtrousTurn atrous_schedule(AtrousLevel &L, const rt_denoise_guides &g, const Params &p, uint32_t rows, uint32_t cols, uint32_t j) {
    const uint32_t after = p.n_levels - 1u - j;
    guide_planes(L, g, rows, cols);
    L.step = (int32_t)(1u << (p.first_level + j));
    L.sn2 = p.sigma_normal * p.sigma_normal;
    L.sp2 = p.sigma_position * p.sigma_position;
    L.demod_in = (j == 0u && (p.flags & RT_DENOISE_DEMODULATE_IN)) ? 1u : 0u;
    L.demod_out = (after == 0u && (p.flags & RT_DENOISE_DEMODULATE_OUT)) ? 1u : 0u;
    return {after, after % 2u == 0u};
}

/* ---- THE gather of a level from global memory: the CPU forms and the simple kernels ---- */

template <class F>
RT_AT_HD void atrous_pixel(const typename F::Level &L, uint32_t r, uint32_t c) {
    const uint64_t i = (uint64_t)r * L.cols + c;
    const bool filtered = guide_valid(L, i);
    typename F::Acc a = {};
    if (filtered) {
        const typename F::Pix p = F::load(L, i);
        const typename F::Context k = F::context(L, r, c);
        for (int dr = -2; dr <= 2; ++dr) {
            const int64_t qr = (int64_t)r + (int64_t)dr * L.step;
            if (qr < 0 || qr >= (int64_t)L.rows) continue;
            for (int dc = -2; dc <= 2; ++dc) {
                const int64_t qc = (int64_t)c + (int64_t)dc * L.step;
                if (qc < 0 || qc >= (int64_t)L.cols) continue;
                const uint64_t qi = (uint64_t)qr * L.cols + (uint64_t)qc;
                if (!guide_valid(L, qi)) continue;
                F::tap(L, a, p, F::load(L, qi), k, dr, dc);
            }
        }
    }
    F::store(L, i, filtered, a);
}

/* one level as an element loop: output pixel i = r * cols + c */
template <class F>
struct AtrousEach {
    typename F::Level L;
    RT_AT_HD uint64_t count() const { return (uint64_t)L.rows * L.cols; }
    RT_AT_HD void operator()(uint64_t i) const {
        const uint32_t r = (uint32_t)(i / L.cols), c = (uint32_t)(i - (uint64_t)r * L.cols);
        atrous_pixel<F>(L, r, c);
    }
};

/* every level of a call on the host: a.level(j) is the filter's Level */
template <class F, class Args>
inline void atrous_cpu(const Args &a) {
    for (uint32_t j = 0; j < a.params->n_levels; ++j) {
        const AtrousEach<F> level = {a.level(j)};
        for (uint64_t i = 0; i < level.count(); ++i) level(i);
    }
}

/* ---- the pieces of the argument checks: each returns its text, or null; a query's limits() puts them in the order
 * include/rt_amd.h states ---- */

inline const char *limits_image(uint64_t rows, uint64_t cols) {
    return rows >= (1ull << 32) || cols >= (1ull << 32) || rows * cols >= (1ull << 32) ? "rows * cols: 2^32 pixels or more" : nullptr;
}

inline const char *limits_levels(uint32_t first_level, uint32_t n_levels) {
    if (n_levels < 1u) return "n_levels must be at least 1";
    if (first_level >= RT_DENOISE_MAX_LEVELS || n_levels > RT_DENOISE_MAX_LEVELS || first_level + n_levels > RT_DENOISE_MAX_LEVELS)
        return "first_level + n_levels must be at most 6";
    return nullptr;
}

/* field `name` of *p, a sigma */
#define RT_LIMITS_SIGMA(p, name) (!((p)->name > 0.0f) ? #name " must be > 0 (+inf: the term is off)" : nullptr)

inline const char *limits_demodulation(uint32_t flags, const rt_denoise_guides *g) {
    if (flags & ~RT_DENOISE_DEMODULATE) return "flags: unknown bits (RT_DENOISE_DEMODULATE_IN, RT_DENOISE_DEMODULATE_OUT)";
    if ((flags & RT_DENOISE_DEMODULATE) && !g->albedo) return "flags: demodulation needs an albedo plane";
    return nullptr;
}

inline const char *limits_guide_strides(const rt_denoise_guides *g) {
    if (g->normal && g->normal_stride < 3u) return "normal_stride must be at least 3 words";
    if (g->position && g->position_stride < 3u) return "position_stride must be at least 3 words";
    if (g->albedo && g->albedo_stride < 3u) return "albedo_stride must be at least 3 words";
    if (g->valid && g->valid_stride < 1u) return "valid_stride must be at least 1 word";
    return nullptr;
}

} /* namespace rt */

#endif /* RT_ATROUS_H */
