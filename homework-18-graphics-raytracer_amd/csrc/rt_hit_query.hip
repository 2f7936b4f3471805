/*
 * rt_hit_query.hip — hit queries: what the reference does with a Hit it holds, on caller-supplied rt_hit records (each with the
 * rt_ray that produced it, Hit.ray): get_shade (main.rs:407-464), get_reflect (main.rs:328-341) and get_refract (main.rs:343-405).
 * Nothing here is new arithmetic: the material, the bump normal, the lights and Phong are rt_shade.h's helpers, the casts are
 * rt_cast.h's cast_pairs / cast_asm and finish_hit exactly as the render kernels call them, and get_refract's loop is the one
 * rt_dist_advance.inc unrolls into one cast per step — so their exactness arguments carry over unchanged.  What is new is reading
 * hits from ABI records that a caller may have written: a record is validated before anything is indexed with it.
 *
 *   rt::shade_hits_kernel     one wave per 64 hits, all 64 lanes executing; the light loop is wave-uniform with the ballot skip of
 *                             dist_shade_kernel; one shadow cast per light that asks, pair-wise or (RT_AMD_QUERY_WAVE_UNIFORM) wave-uniform
 *   rt::refract_rays_kernel   one wave per 64 hits; a per-lane state machine (enter, the inside cast, up to 10 total-reflection
 *                             bounces, exit) around ONE cast per iteration for the whole wave, lanes that have finished helping
 *   rt::reflect_rays_kernel   one work-item per hit; pure
 */
#include "rt_cast.h"
#include "rt_hit_abi.h"
#include "rt_api_internal.h"

namespace rt {

/* one cast for the whole wave: every lane calls, `want` says whose ray it is */
template <bool WAVE_UNIFORM, class Scene>
__device__ __forceinline__ CastResult query_cast(const Scene &sc, const Ray &req, const bool want, PairLdsSlim *pl) {
    CastResult cr;
    cr.prim = -1;
    cr.t = 0.0f;
    cr.bf = 0u;
    cr.a0 = cr.a1 = cr.a2 = 0.0f;
    if constexpr (WAVE_UNIFORM) {
        if (want) cr = cast_asm(sc, req);
    } else {
        cr = cast_pairs(sc, req, want, pl); /* all 64 lanes: those without a ray help */
    }
    return cr;
}

/* Launch bounds, LDS and register budget as cast_rays_kernel's (rt_query.hip): 256 threads, 6 waves per SIMD (80 VGPRs), one
 * PairLdsSlim per wave.  What the compiler makes of them is recorded in profiles/README.md. */
#ifndef RT_HITQ_THREADS
#define RT_HITQ_THREADS 256
#endif
#ifndef RT_HITQ_MIN_WAVES
#define RT_HITQ_MIN_WAVES 6
#endif

/* get_shade(&hit) (main.rs:407-464) */
template <bool WAVE_UNIFORM>
__global__ __launch_bounds__(RT_HITQ_THREADS, RT_HITQ_MIN_WAVES) void shade_hits_kernel(const KernelScene sc, const rt_hit *__restrict__ hits,
                                                                                        const rt_ray *__restrict__ incoming, float *__restrict__ rgb,
                                                                                        unsigned long long *ray_count, const uint32_t n) {
    PairLdsSlim *pl = nullptr;
    if constexpr (!WAVE_UNIFORM) {
        __shared__ PairLdsSlim pair_lds_all[RT_HITQ_THREADS / 64];
        pl = &pair_lds_all[threadIdx.x >> 6];
    }
    const uint32_t first = blockIdx.x * RT_HITQ_THREADS + (threadIdx.x & ~63u); /* the wave's first record */
    if (first >= n) return;                                                      /* whole waves only */
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = first + lane;
    const bool in_range = i < n;
    bool active = false;
    V3 pos = v3(0.0f, 0.0f, 0.0f), normal = v3(0.0f, 0.0f, 1.0f), view = v3(0.0f, 0.0f, 1.0f);
    uint32_t prim = RT_HIT_NO_PRIM;
    Mat m;
    m.normal = v3(0.0f, 0.0f, 1.0f);
    m.diffuse = m.specular = v3(0.0f, 0.0f, 0.0f);
    m.shiness = m.smoothness = m.transparency = m.refraction_index = m.opaque_decay = 0.0f;
    if (in_range) {
        const AbiHit h = hit_from_abi(hits + i, sc.n_triangles, sc.n_spheres, sc.n_materials, true);
        if (h.valid) {
            active = true;
            pos = h.g.pos;
            normal = h.g.normal;
            prim = h.g.prim;
            view = ray_from_abi(incoming + i, sc.n_triangles, sc.n_spheres).d; /* hit.ray.direction */
            m = material_approx(sc.materials[h.g.obj], h.g.u, h.g.v);
        }
    }
    const V3 adj_n = adjust_normal(m.normal, normal); /* main.rs:410 */
    V3 sum = v3(0.0f, 0.0f, 0.0f);
    uint32_t casts = 0u;
    for (uint32_t light_i = 0; light_i < sc.n_lights; ++light_i) { /* wave-uniform */
        const auto &L = uniform_ref(sc.lights + light_i);
        /* does the light ask for a shadow cast (main.rs:413-433)?  light_asks answers without a spot light's acos wherever the angle
         * is clear of the cone's edge (rt_shade.h); the light's colour waits for the lit lanes */
        V3 l_direction = v3(0.0f, 0.0f, 0.0f);
        const bool need = light_asks(L, uniform_ref(sc.light_aux + light_i), pos, adj_n, &l_direction) && active;
        if (__builtin_amdgcn_ballot_w64(need) == 0ull) continue;
        Ray req;
        req.o = pos;
        req.d = -l_direction;
        req.mode = FACE_BACK;
        req.excl = excl_of(prim, FACE_BACK);
        const CastResult cr = query_cast<WAVE_UNIFORM>(sc, req, need, pl);
        if (need) {
            casts += 1u;
            bool lit = true;
            if (cr.prim >= 0) { /* main.rs:435-448 */
                const bool has_origin = (L.kind != RT_LIGHT_DIRECTIONAL) || (L.has_origin != 0u);
                if (has_origin) {
                    const V3 occ = req.o + req.d * cr.t; /* occlusion.at.position (finish_hit) */
                    if (distance(pos, occ) < distance(pos, v3(L.origin[0], L.origin[1], L.origin[2]))) lit = false;
                } else {
                    lit = false;
                }
            }
            if (lit) {
                DirLight dl;
                dl.direction = dl.color = v3(0.0f, 0.0f, 0.0f);
                (void)approximate_into_directional(L, pos, &dl); /* the light asked: Some */
                const V3 light_direction = req.d;
                const V3 diffuse = get_diffuse(m, adj_n, light_direction) * dl.color;
                const V3 specular = get_specular(m, adj_n, -view, light_direction) * dl.color;
                sum = sum + diffuse * (1.0f - m.shiness) + specular * m.shiness;
            }
        }
    }
    if (in_range) { /* "no hit": black (sum was never touched) */
        rgb[(size_t)i * 3u] = sum.x;
        rgb[(size_t)i * 3u + 1u] = sum.y;
        rgb[(size_t)i * 3u + 2u] = sum.z;
    }
    if (ray_count != nullptr) {
        for (int off = 32; off > 0; off >>= 1) casts += __shfl_down(casts, off, 64);
        if (lane == 0u && casts != 0u) atomicAdd(ray_count, (unsigned long long)casts);
    }
}

/* get_refract(&hit, max_distance) (main.rs:343-405), one cast per loop iteration as rt_dist_advance.inc unrolls it */
enum : uint32_t { RQ_DONE = 0u, RQ_INSIDE = 1u, RQ_BOUNCE = 2u };
enum : uint32_t { REFR_ESCAPED = 0u, REFR_INFINITE = 1u, REFR_TRAPPED = 2u }; /* main.rs:149-158 */
template <bool WAVE_UNIFORM>
__global__ __launch_bounds__(RT_HITQ_THREADS, RT_HITQ_MIN_WAVES) void refract_rays_kernel(const KernelScene sc, const rt_hit *__restrict__ hits,
                                                                                          const rt_ray *__restrict__ incoming, const float max_distance,
                                                                                          uint32_t *__restrict__ out_kind, float *__restrict__ out_travel,
                                                                                          rt_ray *__restrict__ out_escape, unsigned long long *ray_count,
                                                                                          const uint32_t n) {
    PairLdsSlim *pl = nullptr;
    if constexpr (!WAVE_UNIFORM) {
        __shared__ PairLdsSlim pair_lds_all[RT_HITQ_THREADS / 64];
        pl = &pair_lds_all[threadIdx.x >> 6];
    }
    const uint32_t first = blockIdx.x * RT_HITQ_THREADS + (threadIdx.x & ~63u);
    if (first >= n) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = first + lane;
    const bool in_range = i < n;
    uint32_t phase = RQ_DONE, result = RT_HIT_NONE, retry = 0u, casts = 0u;
    float travel = 0.0f, k = 1.0f;
    V3 entry_pos = v3(0.0f, 0.0f, 0.0f);
    Ray req;
    req.o = v3(0.0f, 0.0f, 0.0f);
    req.d = v3(0.0f, 0.0f, 1.0f);
    req.mode = FACE_FRONT;
    req.excl = 0u;
    if (in_range) {
        const AbiHit h = hit_from_abi(hits + i, sc.n_triangles, sc.n_spheres, sc.n_materials, true);
        if (h.valid) {
            const V3 in_dir = ray_from_abi(incoming + i, sc.n_triangles, sc.n_spheres).d; /* hit.ray.direction */
            k = material_approx(sc.materials[h.g.obj], h.g.u, h.g.v).refraction_index;   /* main.rs:354 */
            entry_pos = h.g.pos;
            V3 refract_in;
            if (refract_dir(h.g.normal, in_dir, k, &refract_in)) {
                req.o = h.g.pos;
                req.d = normalize(refract_in); /* normalised a second time, main.rs:362 */
                req.mode = FACE_BACK;
                req.excl = excl_of(h.g.prim, FACE_FRONT);
                phase = RQ_INSIDE;
            } else {
                result = REFR_TRAPPED; /* main.rs:356-358 */
            }
        }
    }
    V3 esc_o = v3(0.0f, 0.0f, 0.0f), esc_d = v3(0.0f, 0.0f, 0.0f);
    uint32_t esc_prim = 0u;
    while (__builtin_amdgcn_ballot_w64(phase != RQ_DONE) != 0ull) { /* wave-uniform: one cast per iteration, at most 11 */
        const bool want = phase != RQ_DONE;
        const CastResult cr = query_cast<WAVE_UNIFORM>(sc, req, want, pl);
        if (want) casts += 1u;
        if (want && cr.prim < 0) { /* main.rs:373, 383 */
            result = REFR_INFINITE;
            phase = RQ_DONE;
        } else if (want) {
            const HitGeom ih = finish_hit(sc, req, cr, false); /* hit_inside */
            if (phase == RQ_INSIDE) {
                travel = distance(ih.pos, entry_pos); /* main.rs:375 */
                retry = 0u;
            } else {
                travel += distance(req.o, ih.pos); /* main.rs:385: previous_hit_position is the bounce ray's origin */
                retry += 1u;
            }
            V3 out_dir;
            const bool have_out = refract_dir(ih.normal, req.d, 1.0f / k, &out_dir);
            if (!have_out && travel <= max_distance && retry < 10u) { /* main.rs:378, in its order; get_reflect(&hit_inside) */
                const V3 in_dir = req.d;
                req.o = ih.pos;
                req.d = reflect_dir(ih.normal, in_dir);
                req.excl = pack_excl(ih.prim, ih.bf ? FACE_FRONT : FACE_BACK); /* the face mode stays hit_inside.ray's: Back */
                phase = RQ_BOUNCE;
            } else if (have_out) { /* main.rs:392-402 */
                esc_o = ih.pos;
                esc_d = normalize(out_dir);
                esc_prim = ih.prim;
                result = REFR_ESCAPED;
                phase = RQ_DONE;
            } else {
                result = REFR_TRAPPED;
                phase = RQ_DONE;
            }
        }
    }
    if (in_range) {
        const bool escaped = result == REFR_ESCAPED;
        out_kind[i] = result;
        if (out_travel != nullptr) out_travel[i] = escaped ? travel : 0.0f;
        if (escaped) {
            const bool tri = esc_prim < sc.n_triangles;
            store_ray(out_escape + i, esc_o, esc_d, FACE_FRONT, 1u, tri ? 1u : 0u, tri ? esc_prim : esc_prim - sc.n_triangles, FACE_BACK);
        } else {
            store_ray(out_escape + i, v3(0.0f, 0.0f, 0.0f), v3(0.0f, 0.0f, 0.0f), 0u, 0u, 0u, 0u, 0u);
        }
    }
    if (ray_count != nullptr) {
        for (int off = 32; off > 0; off >>= 1) casts += __shfl_down(casts, off, 64);
        if (lane == 0u && casts != 0u) atomicAdd(ray_count, (unsigned long long)casts);
    }
}

/* get_reflect(&hit) (main.rs:328-341); records written as camera_rays_kernel writes its own */
__global__ __launch_bounds__(256) void reflect_rays_kernel(const rt_hit *__restrict__ hits, const rt_ray *__restrict__ incoming, rt_ray *__restrict__ out,
                                                           const uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const AbiHit h = hit_from_abi(hits + i, 0u, 0u, 0u, false);
    if (!h.valid) {
        store_ray(out + i, v3(0.0f, 0.0f, 0.0f), v3(0.0f, 0.0f, 0.0f), 0u, 0u, 0u, 0u, 0u);
        return;
    }
    const Ray in = ray_from_abi(incoming + i, 0u, 0u); /* origin, direction and face mode: the exclusion of hit.ray is not read */
    store_ray(out + i, h.g.pos, reflect_dir(h.g.normal, in.d), in.mode, 1u, h.kind, h.index, h.g.bf ? FACE_FRONT : FACE_BACK);
}

/* No launch takes more than band_records records (rt_api_internal.h for_each_band; RT_HITQ_BAND, or fewer under the test hook
 * RT_AMD_DIAG_HIT_BAND_RECORDS) — as RT_TRACE_BAND_RAYS of rt_trace_rays. */

hipError_t launch_shade_hits(const KernelScene &sc, const rt_hit *hits, const rt_ray *incoming, uint32_t n, float *rgb,
                             unsigned long long *ray_count, bool wave_uniform, uint32_t band_records, hipStream_t stream) {
    return for_each_band(n, band_records, [&](uint64_t off, uint32_t band) {
        if (wave_uniform)
            hipLaunchKernelGGL(shade_hits_kernel<true>, grid_of(band, RT_HITQ_THREADS), dim3(RT_HITQ_THREADS), 0, stream, sc, hits + off, incoming + off,
                               rgb + (size_t)off * 3u, ray_count, band);
        else
            hipLaunchKernelGGL(shade_hits_kernel<false>, grid_of(band, RT_HITQ_THREADS), dim3(RT_HITQ_THREADS), 0, stream, sc, hits + off, incoming + off,
                               rgb + (size_t)off * 3u, ray_count, band);
    });
}

hipError_t launch_refract_rays(const KernelScene &sc, const rt_hit *hits, const rt_ray *incoming, uint32_t n, float max_distance, uint32_t *kind,
                               float *travel, rt_ray *escape, unsigned long long *ray_count, bool wave_uniform, uint32_t band_records, hipStream_t stream) {
    return for_each_band(n, band_records, [&](uint64_t off, uint32_t band) {
        float *const band_travel = travel != nullptr ? travel + off : nullptr;
        if (wave_uniform)
            hipLaunchKernelGGL(refract_rays_kernel<true>, grid_of(band, RT_HITQ_THREADS), dim3(RT_HITQ_THREADS), 0, stream, sc, hits + off, incoming + off,
                               max_distance, kind + off, band_travel, escape + off, ray_count, band);
        else
            hipLaunchKernelGGL(refract_rays_kernel<false>, grid_of(band, RT_HITQ_THREADS), dim3(RT_HITQ_THREADS), 0, stream, sc, hits + off, incoming + off,
                               max_distance, kind + off, band_travel, escape + off, ray_count, band);
    });
}

hipError_t launch_reflect_rays(const rt_hit *hits, const rt_ray *incoming, uint32_t n, rt_ray *out, uint32_t band_records, hipStream_t stream) {
    return for_each_band(n, band_records, [&](uint64_t off, uint32_t band) {
        hipLaunchKernelGGL(reflect_rays_kernel, grid_of(band, 256u), dim3(256), 0, stream, hits + off, incoming + off, out + off, band);
    });
}

} /* namespace rt */
