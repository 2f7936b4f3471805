/*
 * rt_texture.h — the arithmetic of the texture queries (include/rt_amd.h "texture queries"), written once for the host (librt_host.so:
 * rt_texture_pyramid_cpu / _footprint_cpu / _sample_cpu / _surfaces_cpu) and the device (rt_texture_query.hip).  A texture is a pyramid
 * of row-major RGB f32 levels, level 0 first, level l of extent max(1, W >> l) by max(1, H >> l).  A level is the exact box filter of the
 * one before it: two taps along an even extent, three integer-weighted taps along an odd one, x before y.  A lookup maps uv through the
 * texture's scale and offset to texel space, wraps or clamps it per axis and reads the nearest texel or mixes four as env_lookup does
 * (rt_environment.h); a trilinear lookup takes its level from the exponent of the footprint in texels and mixes two levels by the
 * mantissa.  The footprint of a ray cone at a hit is its width over the cosine, carried into uv space by the primitive's own ratio of
 * uv area to surface area.  Every function is a sequence of single f32 or u32 operations in the order the header comment of the block
 * gives; both libraries are built with -ffp-contract=off and sqrt and the divides are correctly rounded on either side, so the host and
 * the device forms agree bit for bit.
 */
#ifndef RT_TEXTURE_H
#define RT_TEXTURE_H

#include <math.h>
#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_detmath.h"
#include "rt_environment.h" /* env_finite, env_mix */
#include "rt_film.h"
#include "rt_shade.h"       /* adjust_normal */
#include "rt_vec.h"

namespace rt {

#define RT_TEX_MAX_LEVELS 15u   /* 1 + log2(RT_TEX_MAX_SIDE) */
#define RT_TEX_SMALL 32u        /* a source level of at most this extent each way: the rest of the pyramid is one workgroup's */
#define RT_TEX_HIT_WORDS 13u    /* an rt_hit in words */
#define RT_TEX_HIT_OBJECT 2u    /* word of rt_hit.object_index */
#define RT_TEX_HIT_POSITION 3u
#define RT_TEX_HIT_NORMAL 6u
#define RT_TEX_HIT_UV 9u
#define RT_TEX_RAY_WORDS 11u    /* an rt_ray in words */
#define RT_TEX_SURFACE_WORDS 18u
#define RT_TEX_MIN_COSINE 0.015625f /* 2^-6 */

/* ---- sizes ---- */

RT_FILM_HD uint32_t tex_extent(uint32_t side, uint32_t level) {
    const uint32_t e = level < 32u ? side >> level : 0u;
    return e != 0u ? e : 1u;
}

/* 1 + floor(log2(max(w, h))); 0 for a side of 0 */
inline uint32_t tex_levels(uint32_t w, uint32_t h) {
    if (w == 0u || h == 0u) return 0u;
    uint32_t m = w > h ? w : h, levels = 1u;
    while (m > 1u) {
        m >>= 1;
        ++levels;
    }
    return levels;
}

/* the floats of levels 0 .. n_levels - 1; 0 when a side is 0 or above RT_TEX_MAX_SIDE, or n_levels is 0 or above tex_levels */
inline uint64_t tex_pyramid_floats(uint32_t w, uint32_t h, uint32_t n_levels) {
    if (w == 0u || h == 0u || w > RT_TEX_MAX_SIDE || h > RT_TEX_MAX_SIDE || n_levels == 0u || n_levels > tex_levels(w, h)) return 0u;
    uint64_t texels = 0u;
    for (uint32_t l = 0; l < n_levels; ++l) texels += (uint64_t)tex_extent(w, l) * tex_extent(h, l);
    return texels * 3u;
}

/* the limits of a texture and the messages, for the device calls and the CPU forms; null: all in range.  *unsupported: the refusal is
 * RT_ERR_UNSUPPORTED (a side above RT_TEX_MAX_SIDE) */
inline const char *texture_limits(const rt_texture *tex, bool *unsupported) {
    *unsupported = false;
    if (tex == nullptr) return "null texture";
    if (tex->d_texels == nullptr) return "null texture texels";
    if (tex->width == 0u || tex->height == 0u) return "a texture of width or height 0";
    if (tex->width > RT_TEX_MAX_SIDE || tex->height > RT_TEX_MAX_SIDE) {
        *unsupported = true;
        return "a texture wider or higher than 16384";
    }
    if (tex->n_levels == 0u || tex->n_levels > tex_levels(tex->width, tex->height)) return "n_levels of 0 or above rt_texture_levels(width, height)";
    if (tex->filter != RT_TEX_NEAREST && tex->filter != RT_TEX_BILINEAR && tex->filter != RT_TEX_TRILINEAR)
        return "unknown filter (RT_TEX_NEAREST, RT_TEX_BILINEAR or RT_TEX_TRILINEAR)";
    if ((tex->wrap_u != RT_TEX_REPEAT && tex->wrap_u != RT_TEX_CLAMP) || (tex->wrap_v != RT_TEX_REPEAT && tex->wrap_v != RT_TEX_CLAMP))
        return "unknown wrap (RT_TEX_REPEAT or RT_TEX_CLAMP)";
    return nullptr;
}

/* a texture as the kernels take it: the descriptor and where each level starts, in texels */
struct TexView {
    const float *texels;
    uint32_t width, height, n_levels, filter, wrap_u, wrap_v;
    float scale_u, scale_v, offset_u, offset_v;
    uint32_t start[RT_TEX_MAX_LEVELS];
};

/* of a texture texture_limits has passed */
inline TexView tex_view(const rt_texture &t) {
    TexView v;
    v.texels = t.d_texels;
    v.width = t.width, v.height = t.height, v.n_levels = t.n_levels;
    v.filter = t.filter, v.wrap_u = t.wrap_u, v.wrap_v = t.wrap_v;
    v.scale_u = t.scale[0], v.scale_v = t.scale[1], v.offset_u = t.offset[0], v.offset_v = t.offset[1];
    uint32_t at = 0u; /* below 2^29: 16384^2 * 4 / 3 */
    for (uint32_t l = 0; l < RT_TEX_MAX_LEVELS; ++l) {
        v.start[l] = at;
        if (l < t.n_levels) at += tex_extent(t.width, l) * tex_extent(t.height, l);
    }
    return v;
}

/* ---- the pyramid ---- */

/* one axis of the box filter: destination texel x of a source of `extent` texels, whose texels p(k) come from `tap`.
 *     extent 1         p(0)
 *     extent 2m        (p(2x) + p(2x + 1)) * 0.5f
 *     extent 2m + 1    (((float)(m - x) * p(2x) + (float)m * p(2x + 1)) + (float)(1 + x) * p(2x + 2)) / (float)(2m + 1)
 * — the three weights are what of each source texel lies under the destination texel, in units of 1 / m */
template <class Tap>
RT_FILM_HD V3 tex_box(const Tap &tap, uint32_t extent, uint32_t x) {
    if (extent == 1u) return tap(0u);
    if ((extent & 1u) == 0u) return (tap(2u * x) + tap(2u * x + 1u)) * 0.5f;
    const uint32_t m = extent >> 1;
    return ((float)(m - x) * tap(2u * x) + (float)m * tap(2u * x + 1u) + (float)(1u + x) * tap(2u * x + 2u)) / (float)extent;
}

/* a source level behind a pointer, global or LDS */
struct TexLevel {
    const float *texels;
    uint32_t width, height;
};

struct TexRowTap {
    const float *row;
    RT_FILM_HD V3 operator()(uint32_t k) const { return v3p(row + 3u * (uint64_t)k); }
};

/* rows reduced along x first ... */
struct TexColumnTap {
    TexLevel src;
    uint32_t x;
    RT_FILM_HD V3 operator()(uint32_t r) const {
        const TexRowTap row = {src.texels + 3u * (uint64_t)r * src.width};
        return tex_box(row, src.width, x);
    }
};

/* ... then the up to three partial rows along y: texel (x, y) of the level after `src` */
RT_FILM_HD V3 tex_reduce(const TexLevel &src, uint32_t x, uint32_t y) {
    const TexColumnTap column = {src, x};
    return tex_box(column, src.height, y);
}

/* ---- the footprint ---- */

/* sqrt(|du1 * dv2 - du2 * dv1| / |e1 x e2|) with e1 = p1 - p0, e2 = p2 - p0 and the uv differences likewise: uv length per unit of
 * surface length.  *ok: the surface area is finite and > 0 */
RT_FILM_HD float tex_triangle_ratio(V3 p0, V3 p1, V3 p2, float u0, float v0, float u1, float v1, float u2, float v2, bool *ok) {
    const V3 e1 = p1 - p0, e2 = p2 - p0;
    const float du1 = u1 - u0, dv1 = v1 - v0, du2 = u2 - u0, dv2 = v2 - v0;
    const float area_uv = rtdm::f_abs(du1 * dv2 - du2 * dv1);
    const float area = magnitude(cross(e1, e2));
    *ok = area > 0.0f && env_finite(area);
    return rtdm::f_sqrt(area_uv / area);
}

/* a sphere's uv square covers 4 pi r^2: sqrt(1 / (4 pi)) / r */
RT_FILM_HD float tex_sphere_ratio(float radius, bool *ok) {
    *ok = radius > 0.0f && env_finite(radius);
    return 0.28209479f / radius;
}

/* w = width0 + spread * |position - origin|;  c = max(|dot(D / |D|, normal)|, 2^-6);  footprint = w * ratio / c;  +0 when not finite */
RT_FILM_HD float tex_footprint(float width0, float spread, V3 position, V3 origin, V3 direction, V3 normal, float ratio) {
    const float w = width0 + spread * magnitude(position - origin);
    const float cosine = rtdm::f_abs(dot(direction / magnitude(direction), normal));
    const float c = cosine > RT_TEX_MIN_COSINE ? cosine : RT_TEX_MIN_COSINE; /* NaN: the floor */
    const float f = w * ratio / c;
    return env_finite(f) ? f : 0.0f;
}

/* record i of a footprint call, its hit and ray as words; `ratio` and `ok` of the primitive the hit names (ok false: "no hit", an
 * index outside its array, a degenerate primitive) */
RT_FILM_HD float tex_footprint_record(const uint32_t *hit, const uint32_t *ray, float width0, float spread, float ratio, bool ok) {
    if (!ok) return 0.0f;
    const V3 position = v3(rtdm::f32_from_bits(hit[RT_TEX_HIT_POSITION]), rtdm::f32_from_bits(hit[RT_TEX_HIT_POSITION + 1u]),
                           rtdm::f32_from_bits(hit[RT_TEX_HIT_POSITION + 2u]));
    const V3 normal = v3(rtdm::f32_from_bits(hit[RT_TEX_HIT_NORMAL]), rtdm::f32_from_bits(hit[RT_TEX_HIT_NORMAL + 1u]),
                         rtdm::f32_from_bits(hit[RT_TEX_HIT_NORMAL + 2u]));
    const V3 origin = v3(rtdm::f32_from_bits(ray[0]), rtdm::f32_from_bits(ray[1]), rtdm::f32_from_bits(ray[2]));
    const V3 direction = v3(rtdm::f32_from_bits(ray[3]), rtdm::f32_from_bits(ray[4]), rtdm::f32_from_bits(ray[5]));
    return tex_footprint(width0, spread, position, origin, direction, normal, ratio);
}

/* ---- the lookup ---- */

RT_FILM_HD V3 tex_texel(const TexView &t, uint32_t level, uint32_t width, uint32_t x, uint32_t y) {
    return v3p(t.texels + ((uint64_t)t.start[level] + (uint64_t)y * width + x) * 3u);
}

/* a texel-space coordinate s along an axis of `extent` texels, into [0, extent]: wrapped by s - floorf(s / extent) * extent or clamped;
 * a NaN becomes 0 */
RT_FILM_HD float tex_coordinate(float s, uint32_t extent, uint32_t wrap) {
    const float e = (float)extent;
    const float x = wrap == RT_TEX_REPEAT ? s - floorf(s / e) * e : s;
    return fminf(fmaxf(x, 0.0f), e);
}

/* the two texels about x_f - 0.5 and the weight of the second, as env_lookup takes its columns (wrapped) and its rows (clamped) */
RT_FILM_HD void tex_pair(float x_f, uint32_t extent, uint32_t wrap, uint32_t *x0, uint32_t *x1, float *fx) {
    const float xs = x_f - 0.5f;
    const float x0f = floorf(xs);
    *fx = xs - x0f;
    const int32_t xi = (int32_t)x0f; /* -1 .. extent */
    if (wrap == RT_TEX_REPEAT) {
        *x0 = xi < 0 ? extent - 1u : ((uint32_t)xi >= extent ? (uint32_t)xi - extent : (uint32_t)xi);
        *x1 = *x0 + 1u >= extent ? 0u : *x0 + 1u;
    } else {
        *x0 = xi < 0 ? 0u : ((uint32_t)xi > extent - 1u ? extent - 1u : (uint32_t)xi);
        *x1 = xi + 1 < 0 ? 0u : ((uint32_t)(xi + 1) > extent - 1u ? extent - 1u : (uint32_t)(xi + 1));
    }
}

/* level `level` at the point (pu, pv) = uv * scale + offset: s = p * (float)extent per axis */
RT_FILM_HD V3 tex_level_lookup(const TexView &t, uint32_t level, float pu, float pv, bool nearest) {
    const uint32_t w = tex_extent(t.width, level), h = tex_extent(t.height, level);
    const float x_f = tex_coordinate(pu * (float)w, w, t.wrap_u), y_f = tex_coordinate(pv * (float)h, h, t.wrap_v);
    if (nearest) {
        const uint32_t x = (uint32_t)x_f, y = (uint32_t)y_f;
        return tex_texel(t, level, w, x < w - 1u ? x : w - 1u, y < h - 1u ? y : h - 1u);
    }
    uint32_t x0, x1, y0, y1;
    float fx, fy;
    tex_pair(x_f, w, t.wrap_u, &x0, &x1, &fx);
    tex_pair(y_f, h, t.wrap_v, &y0, &y1, &fy);
    const V3 top = env_mix(tex_texel(t, level, w, x0, y0), tex_texel(t, level, w, x1, y0), fx);
    const V3 bottom = env_mix(tex_texel(t, level, w, x0, y1), tex_texel(t, level, w, x1, y1), fx);
    return env_mix(top, bottom, fy);
}

/* The filtered lookup at (u, v) with a footprint in uv units.  Trilinear: t = footprint * max(|scale_u| * W, |scale_v| * H) texels;
 * !(t > 1) is level 0; else l = the unbiased exponent of t and f = t * 2^-l - 1, the mantissa, both read from t's bits; the bilinear
 * samples of levels l and l + 1 are mixed by f, and at or above the top level that level is used alone.  *ok false — u or v not finite
 * — returns zeros. */
RT_FILM_HD V3 tex_sample(const TexView &t, float u, float v, float footprint, bool *ok) {
    *ok = env_finite(u) && env_finite(v);
    if (!*ok) return v3(0.0f, 0.0f, 0.0f);
    const float pu = u * t.scale_u + t.offset_u, pv = v * t.scale_v + t.offset_v;
    if (t.filter != RT_TEX_TRILINEAR) return tex_level_lookup(t, 0u, pu, pv, t.filter == RT_TEX_NEAREST);
    const float su = rtdm::f_abs(t.scale_u) * (float)t.width, sv = rtdm::f_abs(t.scale_v) * (float)t.height;
    const float texels = footprint * (su > sv ? su : sv);
    if (!(texels > 1.0f)) return tex_level_lookup(t, 0u, pu, pv, false);
    const uint32_t bits = rtdm::f32_bits(texels);
    const uint32_t level = (bits >> 23) - 127u; /* texels > 1: positive, exponent field 127 .. 255 */
    const uint32_t top = t.n_levels - 1u;
    if (level >= top) return tex_level_lookup(t, top, pu, pv, false);
    const float f = rtdm::f32_from_bits((bits & 0x007fffffu) | 0x3f800000u) - 1.0f;
    return env_mix(tex_level_lookup(t, level, pu, pv, false), tex_level_lookup(t, level + 1u, pu, pv, false), f);
}

/* one sampling call: uv and the output live inside records of the caller's */
struct TexSample {
    TexView tex;
    const float *uv;
    uint64_t uv_stride;
    const float *footprint; /* null: 0 */
    uint64_t n;
    float *out;
    uint64_t out_stride;
};

RT_FILM_HD void tex_sample_record(const TexSample &a, uint64_t i) {
    const float *const uv = a.uv + i * a.uv_stride;
    bool ok;
    const V3 value = tex_sample(a.tex, uv[0], uv[1], a.footprint != nullptr ? a.footprint[i] : 0.0f, &ok);
    float *const out = a.out + i * a.out_stride;
    out[0] = value.x;
    out[1] = value.y;
    out[2] = value.z;
}

/* ---- surfaces ---- */

/* one call that edits rt_surface records */
struct TexSurfaces {
    TexView diffuse, normal;
    bool has_diffuse, has_normal;
    const uint32_t *hits;   /* rt_hit records as words */
    const float *footprint; /* null: 0 */
    uint64_t n;
    uint32_t object_index, flags;
    uint32_t *surfaces;     /* rt_surface records as words */
};

/* Record i: edited only where valid != 0, the hit's object_index is the one asked for (RT_TEX_ALL_OBJECTS: any) and its uv is finite.
 * diffuse_color = the sample, or with RT_TEX_MODULATE the old colour times it.  normal = the sample, or with RT_TEX_NORMALIZE v / |v|
 * — a length that is 0 or not finite leaves normal and shading_normal alone; shading_normal = adjust_normal(normal, hit.normal).  No
 * other word is read or written. */
RT_FILM_HD void tex_surface_record(const TexSurfaces &a, uint64_t i) {
    uint32_t *const p = a.surfaces + i * RT_TEX_SURFACE_WORDS;
    const uint32_t *const hit = a.hits + i * RT_TEX_HIT_WORDS;
    if (p[17] == 0u) return;
    if (a.object_index != RT_TEX_ALL_OBJECTS && hit[RT_TEX_HIT_OBJECT] != a.object_index) return;
    const float u = rtdm::f32_from_bits(hit[RT_TEX_HIT_UV]), v = rtdm::f32_from_bits(hit[RT_TEX_HIT_UV + 1u]);
    if (!env_finite(u) || !env_finite(v)) return;
    const float footprint = a.footprint != nullptr ? a.footprint[i] : 0.0f;
    bool ok;
    if (a.has_diffuse) {
        V3 c = tex_sample(a.diffuse, u, v, footprint, &ok);
        if ((a.flags & RT_TEX_MODULATE) != 0u)
            c = v3(rtdm::f32_from_bits(p[3]), rtdm::f32_from_bits(p[4]), rtdm::f32_from_bits(p[5])) * c;
        p[3] = rtdm::f32_bits(c.x);
        p[4] = rtdm::f32_bits(c.y);
        p[5] = rtdm::f32_bits(c.z);
    }
    if (a.has_normal) {
        V3 m = tex_sample(a.normal, u, v, footprint, &ok);
        if ((a.flags & RT_TEX_NORMALIZE) != 0u) {
            const float len = magnitude(m);
            if (!(len > 0.0f) || !env_finite(len)) return;
            m = m / len;
        }
        const V3 geometric = v3(rtdm::f32_from_bits(hit[RT_TEX_HIT_NORMAL]), rtdm::f32_from_bits(hit[RT_TEX_HIT_NORMAL + 1u]),
                                rtdm::f32_from_bits(hit[RT_TEX_HIT_NORMAL + 2u]));
        const V3 shading = adjust_normal(m, geometric); /* main.rs:410, as material_hits_kernel calls it */
        p[0] = rtdm::f32_bits(m.x);
        p[1] = rtdm::f32_bits(m.y);
        p[2] = rtdm::f32_bits(m.z);
        p[14] = rtdm::f32_bits(shading.x);
        p[15] = rtdm::f32_bits(shading.y);
        p[16] = rtdm::f32_bits(shading.z);
    }
}

inline const char *tex_surface_limits(uint32_t flags) {
    if ((flags & ~(RT_TEX_MODULATE | RT_TEX_NORMALIZE)) != 0u) return "unknown flags (RT_TEX_MODULATE and RT_TEX_NORMALIZE)";
    return nullptr;
}

inline const char *tex_stride_limits(uint64_t uv_stride, uint64_t out_stride) {
    if (uv_stride < 2u || out_stride < 3u) return "uv_stride_words below 2 or out_stride_words below 3";
    return nullptr;
}

} /* namespace rt */

#endif /* RT_TEXTURE_H */
