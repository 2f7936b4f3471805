/*
 * rt_light_record.h — what a hit-sample kernel does per record and per entry, written once for the units that open get_shade
 * (main.rs:407-464) on caller hits: the light, area-light, hemisphere, environment, lobe and texture queries, and the material queries
 * for the surface record.  Device code only; every helper is inlined, none uses LDS.
 *
 *   per record   light_record     hit, material and shading normal (main.rs:408-410), from the scene
 *                surface_record   material and shading normal from an rt_surface record
 *                fold_shiness     what a fold reads of a record: is it a hit, and its shiness
 *                record_id, sampling_normal
 *   per entry    light_terms      main.rs:435-459: lit or occluded, `diffuse` and `specular` — and store_light_terms for the triple
 *                store_shadow_ray the Back ray get_shade casts towards a light (main.rs:426-433), or eleven zero words
 *                store_v3, load_v3 on a plane of three floats per entry
 *
 * The kernels keep their own loops, their own entry index and what they draw; the arithmetic is rt_shade.h's, called here with
 * rt::shade_hits_kernel's operands in its order.
 */
#ifndef RT_LIGHT_RECORD_H
#define RT_LIGHT_RECORD_H

#include "rt_area_light.h" /* area_light_has_origin */
#include "rt_cast.h"
#include "rt_hit_abi.h"

namespace rt {

#define RT_LIGHT_THREADS 256u
#define RT_LIGHT_HIT_POSITION 3u /* word of rt_hit.position */
#define RT_SURFACE_WORDS 18u
static_assert(sizeof(rt_surface) == RT_SURFACE_WORDS * sizeof(uint32_t), "rt_surface is 18 dwords");

__device__ __forceinline__ void store_v3(float *__restrict__ plane, const uint64_t k, const V3 v) {
    plane[k * 3u] = v.x;
    plane[k * 3u + 1u] = v.y;
    plane[k * 3u + 2u] = v.z;
}
__device__ __forceinline__ V3 load_v3(const float *__restrict__ plane, const uint64_t k) { return v3(plane[k * 3u], plane[k * 3u + 1u], plane[k * 3u + 2u]); }

/* the material of a record that is no hit */
__device__ __forceinline__ Mat no_material() {
    Mat m;
    m.normal = v3(0.0f, 0.0f, 1.0f);
    m.diffuse = m.specular = v3(0.0f, 0.0f, 0.0f);
    m.shiness = m.smoothness = m.transparency = m.refraction_index = m.opaque_decay = 0.0f;
    return m;
}

/* what get_shade computes once per hit (main.rs:408-410) */
struct LightRecord {
    bool valid;
    AbiHit h;
    Mat m;
    V3 adj_n;
};
__device__ __forceinline__ LightRecord light_record(const KernelScene &sc, const rt_hit *__restrict__ hits, const uint64_t i) {
    LightRecord r;
    r.valid = false;
    r.h.g.pos = v3(0.0f, 0.0f, 0.0f);
    r.h.g.normal = v3(0.0f, 0.0f, 1.0f);
    r.h.g.prim = RT_HIT_NO_PRIM;
    r.h.kind = r.h.index = 0u;
    r.m = no_material();
    const AbiHit h = hit_from_abi(hits + i, sc.n_triangles, sc.n_spheres, sc.n_materials, true);
    if (h.valid) {
        r.valid = true;
        r.h = h;
        r.m = material_approx(sc.materials[h.g.obj], h.g.u, h.g.v);
    }
    r.adj_n = adjust_normal(r.m.normal, r.h.g.normal); /* main.rs:410 */
    return r;
}

/* the same two of an rt_surface record, as rt_material_hits wrote them or a caller edited them: surface_record reads it whole, 17
 * floats and the flag; surface_flag the flag alone, for a kernel that reads the rest only where it is set.  A SurfaceRecord that was
 * not read is "no hit" */
struct SurfaceRecord {
    bool valid = false;
    Mat m = no_material();
    V3 adj_n = v3(0.0f, 0.0f, 1.0f);
};
__device__ __forceinline__ bool surface_flag(const rt_surface *__restrict__ surfaces, const uint64_t i) {
    return reinterpret_cast<const uint32_t *>(surfaces + i)[RT_SURFACE_WORDS - 1u] != 0u;
}
__device__ __forceinline__ SurfaceRecord surface_record(const rt_surface *__restrict__ surfaces, const uint64_t i) {
    const uint32_t *const p = reinterpret_cast<const uint32_t *>(surfaces + i);
    float f[RT_SURFACE_WORDS - 1u];
#pragma unroll
    for (uint32_t k = 0; k < RT_SURFACE_WORDS - 1u; ++k) f[k] = __uint_as_float(p[k]);
    SurfaceRecord s;
    s.valid = p[RT_SURFACE_WORDS - 1u] != 0u;
    s.m.normal = v3(f[0], f[1], f[2]);
    s.m.diffuse = v3(f[3], f[4], f[5]);
    s.m.shiness = f[6];
    s.m.specular = v3(f[7], f[8], f[9]);
    s.m.smoothness = f[10];
    s.m.transparency = f[11];
    s.m.refraction_index = f[12];
    s.m.opaque_decay = f[13];
    s.adj_n = v3(f[14], f[15], f[16]);
    return s;
}

/* a fold's prologue: *valid: the record is a hit; its material's shiness, 0 for a record that is none */
__device__ __forceinline__ float fold_shiness(const KernelScene &sc, const rt_hit *__restrict__ hits, const uint64_t i, bool *valid) {
    const AbiHit h = hit_from_abi(hits + i, sc.n_triangles, sc.n_spheres, sc.n_materials, true);
    *valid = h.valid;
    return h.valid ? material_approx(sc.materials[h.g.obj], h.g.u, h.g.v).shiness : 0.0f;
}

/* the id a sampler hashes: the caller's, or the record's number */
__device__ __forceinline__ uint32_t record_id(const uint32_t *__restrict__ ids, const uint64_t i) { return ids != nullptr ? ids[i] : (uint32_t)i; }

/* the normal a sampler draws about: a wave-uniform choice */
__device__ __forceinline__ V3 sampling_normal(const LightRecord &r, const uint32_t normal_kind) {
    return normal_kind == RT_HEMISPHERE_GEOMETRIC ? r.h.g.normal : r.adj_n;
}

/* shadow_ray, main.rs:426-433, along `dir`: bit for bit the ray shade_hits_kernel casts — from the hit, face Back, the hit's own
 * primitive excluded — or all-zero words for an entry that does not ask */
__device__ __forceinline__ void store_shadow_ray(rt_ray *__restrict__ ray, const LightRecord &r, const V3 dir, const bool need) {
    if (need)
        store_ray(ray, r.h.g.pos, dir, FACE_BACK, 1u, r.h.kind, r.h.index, FACE_BACK);
    else
        store_ray(ray, v3(0.0f, 0.0f, 0.0f), v3(0.0f, 0.0f, 0.0f), 0u, 0u, 0u, 0u, 0u);
}

/* main.rs:435-459 for one (record, light) entry: `L` is the light the terms see — the stored record (Light: the reference uniform_ref
 * gives, as rt_shade.h takes its lights), or a register copy displaced to a sample; `has_origin` is rt_area_light.h's
 * area_light_has_origin of the stored light, and `origin` what the occluder's distance is measured against where it has one.  `occluder`: the shadow cast's
 * answer, read only where `asked`.  Not asked: not lit, +0 terms.  The callers skip the call for a wave nobody asks in (its acosf
 * and powf are binary64). */
struct LightTerms {
    bool lit = false;
    V3 diffuse = v3(0.0f, 0.0f, 0.0f), specular = v3(0.0f, 0.0f, 0.0f);
};
template <class Light>
__device__ __forceinline__ LightTerms light_terms(const Light &L, const bool has_origin, const V3 origin, const V3 pos, const Mat &m, const V3 adj_n,
                                                  const V3 view, const bool asked, const rt_hit *__restrict__ occluder_hit) {
    LightTerms t;
    if (!asked) return t;
    t.lit = true;
    const uint32_t *const occluder = reinterpret_cast<const uint32_t *>(occluder_hit);
    if (occluder[0] <= 1u) { /* main.rs:435-448: Some(occlusion) */
        if (has_origin) {
            const V3 occ = v3(__uint_as_float(occluder[RT_LIGHT_HIT_POSITION]), __uint_as_float(occluder[RT_LIGHT_HIT_POSITION + 1u]),
                              __uint_as_float(occluder[RT_LIGHT_HIT_POSITION + 2u])); /* occlusion.at.position */
            if (distance(pos, occ) < distance(pos, origin)) t.lit = false;
        } else {
            t.lit = false;
        }
    }
    if (t.lit) {
        DirLight dl;
        dl.direction = dl.color = v3(0.0f, 0.0f, 0.0f);
        t.lit = approximate_into_directional(L, pos, &dl); /* None only where the caller set a flag the light did not */
        if (t.lit) {
            const V3 light_direction = -dl.direction; /* the light's own, not the shadow record's: a caller may have replaced that ray */
            t.diffuse = get_diffuse(m, adj_n, light_direction) * dl.color;
            t.specular = get_specular(m, adj_n, -view, light_direction) * dl.color;
        }
    }
    return t;
}

/* the three outputs of entry k */
__device__ __forceinline__ void store_light_terms(unsigned char *__restrict__ lit_out, float *__restrict__ diffuse_out, float *__restrict__ specular_out,
                                                  const uint64_t k, const LightTerms &t) {
    lit_out[k] = t.lit ? 1 : 0;
    store_v3(diffuse_out, k, t.diffuse);
    store_v3(specular_out, k, t.specular);
}

} /* namespace rt */

#endif /* RT_LIGHT_RECORD_H */
