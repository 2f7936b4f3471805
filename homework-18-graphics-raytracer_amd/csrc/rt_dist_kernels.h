/*
 * rt_dist_kernels.h — the two organisations of the stochastic pass as kernel templates, with their launchers:
 *
 *   distributed_kernel<MAXD, BFS, RAYS>, launch_distributed_of<RAYS>   the fused kernel: a lane keeps its pixel through a whole sample
 *   dist_chain_kernel<ORDER, RAYS>, launch_dist_chain_of<RAYS>         the split pass's chain kernel ("the split pass" below)
 *
 * rt_distributed.hip instantiates them for camera frames (RAYS = false) and holds the plain kernels of the pass; rt_distributed_rays.hip
 * instantiates them for ray batches (RAYS = true).  Nothing here is emitted unless a unit instantiates it.  The file-scope device
 * globals of diagnostic builds (rt_cast.h's pair-time / need counters) are per-unit copies: see rt_distributed_rays.hip.
 */
#ifndef RT_DIST_KERNELS_H
#define RT_DIST_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_cast.h"
#include "rt_pwf_common.h"
#include "rt_rng.h"

namespace rt {

/* ---- the kernel ------------------------------------------------------------------------------- */

enum : uint32_t {
    DP_DONE = 0u,
    DP_PRIMARY = 1u,     /* cast of the shoot_focus ray                        (main.rs:1150) */
    DP_NEXT = 2u,        /* cast of the reflected / escape ray of a level      (main.rs:564, 583, 603) */
    DP_SHADOW = 3u,      /* a shadow ray of get_shade                          (main.rs:435) */
    DP_REFR_INSIDE = 4u, /* get_refract's first inside cast                    (main.rs:371) */
    DP_REFR_BOUNCE = 5u, /* a total-internal-reflection bounce                 (main.rs:381) */
    DP_START = 6u        /* chain kernel: the next epoch's shoot_focus is due */
};

struct DFrame {
    V3 shade;        /* get_shade(&next_hit) */
    V3 factor;       /* brdf (kinds 0, 1) or (decay, -, -) (kind 2) */
    uint32_t kind;   /* 0 Diffuse, 1 Reflection, 2 Refraction */
};

#ifndef RT_DIST_MIN_WAVES
#define RT_DIST_MIN_WAVES 3 /* waves per SIMD the register allocation aims for (profiles/README.md) */
#endif
/* BFS: the casts as a breadth-first walk of the node tree (rt_cast_bfs.h cast_bfs), for scenes beyond the caches (KernelScene::bfs_walk):
 * 256 VGPRs, two waves per SIMD, 5 KB of LDS and a set of record lists per wave */
#define RT_DIST_BFS_WAVES 2
/* RAYS: the roots are a ray batch's (rt_trace_rays_distributed; rt_kernels.h frame_is_rays): slot i of the one-row frame is ray i,
 * start_epoch reads its rt_ray record instead of shooting through the lens — no draws, no clip coordinates — and samples / flags
 * are indexed with the call's ray count (frame_sample_stride), which a band of a larger batch does not have as its own.
 * Instantiated in rt_distributed_rays.hip. */
template <int MAXD, bool BFS = false, bool RAYS = false>
__global__ __launch_bounds__(64, BFS ? RT_DIST_BFS_WAVES : RT_DIST_MIN_WAVES) void distributed_kernel(const KernelScene sc, const KernelFrame fr, const DistParams dp) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    BfsLds *bfs_lds = nullptr;
    BfsScratch bfs_ws = {nullptr, nullptr, nullptr, 0u, 0u};
    if constexpr (BFS) {
        __shared__ BfsLds bfs_lds_one;
        bfs_lds = &bfs_lds_one;
        uint2 *const mine = reinterpret_cast<uint2 *>(dp.bfs_scratch) + (size_t)wave * (2u * (size_t)dp.bfs_items_cap + dp.bfs_jobs_cap);
        bfs_ws.items_a = mine;
        bfs_ws.items_b = mine + dp.bfs_items_cap;
        bfs_ws.jobs = mine + 2u * (size_t)dp.bfs_items_cap;
        bfs_ws.items_cap = dp.bfs_items_cap;
        bfs_ws.jobs_cap = dp.bfs_jobs_cap;
    }
    const uint32_t total_slots = fr.cols * fr.rows;
    const uint32_t band_slots = fr.cols << 3;
    /* Persistent lanes: a lane takes a pixel, runs ALL of this call's epochs for it (the pixel's random stream
     * is sequential), then takes the next pixel.  The scattered rays are incoherent whatever the assignment, so
     * nothing is lost by mixing pixels in a wave, and every lane stays busy until the tile runs dry.  Pixels are
     * handed out as in the Whitted kernel: 64-slot chunks from a global counter (one atomic per chunk per wave),
     * slots inside a chunk by ballot + prefix count.  dp.work_queue == nullptr selects the static assignment
     * (wave w = chunk w); no host path selects it any more (rt_api_dist.hip always passes the chunk counter). */
    const bool persistent = dp.work_queue != nullptr;
    uint32_t q_next = 0u, q_end = 0u;
    bool exhausted = false;
    if (!persistent) {
        q_next = wave * 64u < total_slots ? wave * 64u : total_slots;
        q_end = q_next + 64u < total_slots ? q_next + 64u : total_slots;
        exhausted = true;
    }
    uint32_t out_index = 0u;
    float clip_x = 0.0f, clip_y = 0.0f;
    const V3 cam_x = v3(fr.cam_x[0], fr.cam_x[1], fr.cam_x[2]);
    const V3 cam_y = v3(fr.cam_y[0], fr.cam_y[1], fr.cam_y[2]);
    const V3 cam_t = v3(fr.cam_toward[0], fr.cam_toward[1], fr.cam_toward[2]);
    const V3 cam_o = v3(fr.cam_origin_focus[0], fr.cam_origin_focus[1], fr.cam_origin_focus[2]);
    const size_t n_pixels = RAYS ? (size_t)frame_sample_stride(fr) : (size_t)total_slots;

    Rng rng;
    rng.rec = rng.st = dp.rng_states;
    rng.index = 256u;
    rng.flags = 0u;
    rng.lds = nullptr;

    uint32_t phase = DP_DONE;
    uint32_t epoch = 0u;
    Ray req;
    req.o = v3(0.0f, 0.0f, 0.0f);
    req.d = v3(0.0f, 0.0f, 1.0f);
    req.mode = FACE_FRONT;
    req.excl = 0u;
    uint32_t casts = 0u;

    HitGeom h; /* the hit of the current level */
    h.pos = h.normal = v3(0.0f, 0.0f, 0.0f);
    h.u = h.v = 0.0f;
    h.prim = h.bf = h.obj = 0u;
    V3 h_in_dir = v3(0.0f, 0.0f, 0.0f); /* hit.ray.direction */
    uint32_t h_in_mode = FACE_FRONT;     /* hit.ray.face_direction */
    V3 sdir = v3(0.0f, 0.0f, 0.0f);     /* scattered_hit.ray.direction */
    uint32_t kind = 0u;                  /* RayType selected at this level */
    V3 view_dir_in = v3(0.0f, 0.0f, 0.0f); /* ray direction used as `hit.ray` by the get_shade in progress */
    uint32_t shade_then = 0u;            /* 0: result is the level's value (return), 1: result is get_shade(next_hit) (descend) */
    int32_t sp = 0;
    V3 sum = v3(0.0f, 0.0f, 0.0f), adj_n = v3(0.0f, 0.0f, 0.0f), l_color = v3(0.0f, 0.0f, 0.0f);
    uint32_t light_i = 0u;
    float travel = 0.0f;
    int32_t retry = 0;
    V3 accum = v3(0.0f, 0.0f, 0.0f);
    DFrame stack[MAXD];

    /* Camera::shoot_focus for the next epoch of this pixel (main.rs:101-127) */
    auto start_epoch = [&]() {
        if constexpr (RAYS) { /* the caller's ray, the same in every epoch */
            req = ray_from_abi(frame_rays(fr) + out_index, sc.n_triangles, sc.n_spheres);
            sp = 0;
            phase = DP_PRIMARY;
            return;
        }
        const V3 direction = normalize(clip_x * cam_x + clip_y * cam_y + cam_t);
        const float xoffset = (float)(0.0 + (double)dp.blur * standard_normal(rng)); /* Normal::new(0.0, blur as f64) */
        const float yoffset = (float)(0.0 + (double)dp.blur * standard_normal(rng));
        req.d = normalize(direction * dp.focus + cam_x * xoffset + cam_y * yoffset);
        /* center + toward.normalize() * near - (x*xo + y*yo); the first two terms are per-frame (rt_api.hip) */
        req.o = cam_o - (cam_x * xoffset + cam_y * yoffset);
        req.mode = FACE_FRONT;
        req.excl = 0u;
        sp = 0;
        phase = DP_PRIMARY;
    };

    for (;;) {
        /* ---- idle lanes take the next pixels ---- */
        unsigned long long need = __builtin_amdgcn_ballot_w64(phase == DP_DONE);
        if (dp.n_epochs == 0u) need = 0ull;
        while (need != 0ull) {
            if (q_next == q_end) { /* wave-uniform */
                if (exhausted) break;
                uint32_t c = 0u;
                if (lane == 0u) c = atomicAdd(dp.work_queue, 1u);
                c = (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
                if (c * 64u >= total_slots) { exhausted = true; break; }
                q_next = c * 64u;
                q_end = q_next + 64u < total_slots ? q_next + 64u : total_slots;
            }
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
            const uint32_t avail = q_end - q_next;
            if (phase == DP_DONE && rank < avail) {
                /* same slot -> pixel mapping as the Whitted kernel: 8-row bands, column-major inside a band */
                const uint32_t slot = q_next + rank;
                if constexpr (RAYS) {
                    out_index = slot;
                } else {
                const uint32_t band = slot / band_slots;
                const uint32_t r = slot - band * band_slots;
                const uint32_t rows_left = fr.rows - (band << 3);
                const uint32_t band_rows = rows_left < 8u ? rows_left : 8u;
                const uint32_t col = r / band_rows;
                const uint32_t row = (band << 3) + (r - col * band_rows);
                out_index = row * fr.cols + col;
                const uint32_t x = fr.x0 + col, y = fr.y0 + row * fr.y_step;
                clip_y = (fr.half_height - (float)y) / fr.height_f; /* main.rs:1134-1135 */
                clip_x = ((float)x - fr.half_width) / fr.height_f;
                }
                rng_open(rng, dp.rng_states + (size_t)out_index * RNG_WORDS);
                accum = v3(0.0f, 0.0f, 0.0f);
                if (dp.accum != nullptr) accum = v3(dp.accum[(size_t)out_index * 3u], dp.accum[(size_t)out_index * 3u + 1u], dp.accum[(size_t)out_index * 3u + 2u]);
                epoch = 0u;
                start_epoch();
            }
            const uint32_t n_need = (uint32_t)__builtin_popcountll(need);
            q_next += n_need < avail ? n_need : avail;
            need = __builtin_amdgcn_ballot_w64(phase == DP_DONE);
        }
        if (__builtin_amdgcn_ballot_w64(phase != DP_DONE) == 0ull) break;

        CastResult cr;
        cr.prim = -1;
        cr.t = 0.0f;
        cr.bf = 0u;
        cr.a0 = cr.a1 = cr.a2 = 0.0f;
        if constexpr (BFS) {
            cr = cast_bfs(sc, req, phase != DP_DONE, bfs_lds, bfs_ws); /* all lanes: those without a ray help */
            if (phase != DP_DONE) casts += 1u;
        } else if (phase != DP_DONE) {
            cr = cast_asm(sc, req);
            casts += 1u;
        }
        if (phase == DP_DONE) continue;

        enum { GO_LEVEL, GO_START_SHADE, GO_NEXT_LIGHT, GO_SHADE_DONE, GO_TRY_EXIT, GO_RETURN } go = GO_RETURN;
        V3 value = v3(0.0f, 0.0f, 0.0f);
        HitGeom ih = h; /* inside hit of get_refract, live within this step only */
        V3 i_in_dir = req.d;
        uint32_t i_in_mode = req.mode;

        if (phase == DP_PRIMARY) {
            if (cr.prim < 0) {
                value = v3(0.0f, 0.0f, 0.0f); /* main.rs:1154 */
                go = GO_RETURN;
            } else {
                h = finish_hit(sc, req, cr, false);
                h_in_dir = req.d;
                h_in_mode = req.mode;
                go = GO_LEVEL;
            }
        } else if (phase == DP_NEXT) {
            if (cr.prim < 0) {
                if (kind == 2u) { /* main.rs:606-608 */
                    value = v3(0.0f, 0.0f, 0.0f);
                    go = GO_RETURN;
                } else { /* get_shade(&scattered_hit): the same hit, seen along the scattered direction (main.rs:573, 592) */
                    view_dir_in = sdir;
                    shade_then = 0u;
                    go = GO_START_SHADE;
                }
            } else {
                /* brdf of the CURRENT level, before `h` moves on to the next hit (main.rs:566-570, 585-589) */
                DFrame f;
                f.kind = kind;
                f.shade = v3(0.0f, 0.0f, 0.0f);
                if (kind == 2u) {
                    f.factor = v3(rtdm::powf(sc.materials[h.obj].opaque_decay, travel), 0.0f, 0.0f); /* main.rs:605 */
                } else {
                    const Mat m = material_approx(sc.materials[h.obj], h.u, h.v);
                    const V3 view = -h_in_dir;
                    f.factor = kind == 0u ? get_diffuse(m, h.normal, req.d) : get_specular(m, h.normal, view, req.d);
                }
                stack[sp] = f;
                h = finish_hit(sc, req, cr, false);
                h_in_dir = req.d;
                h_in_mode = req.mode;
                view_dir_in = req.d;
                shade_then = 1u;
                go = GO_START_SHADE;
            }
        } else if (phase == DP_SHADOW) {
            const rt_light &L = sc.lights[light_i];
            bool lit = true;
            if (cr.prim >= 0) {
                const bool has_origin = (L.kind != RT_LIGHT_DIRECTIONAL) || (L.has_origin != 0u);
                if (has_origin) {
                    const V3 occ = req.o + req.d * cr.t;
                    if (distance(h.pos, occ) < distance(h.pos, v3(L.origin[0], L.origin[1], L.origin[2]))) lit = false;
                } else {
                    lit = false;
                }
            }
            if (lit) {
                const Mat m = material_approx(sc.materials[h.obj], h.u, h.v);
                const V3 light_direction = req.d;
                const V3 diffuse = get_diffuse(m, adj_n, light_direction) * l_color;
                const V3 specular = get_specular(m, adj_n, -view_dir_in, light_direction) * l_color;
                sum = sum + diffuse * (1.0f - m.shiness) + specular * m.shiness;
            }
            light_i += 1u;
            go = GO_NEXT_LIGHT;
        } else { /* DP_REFR_INSIDE / DP_REFR_BOUNCE */
            if (cr.prim < 0) {
                value = v3(0.0f, 0.0f, 0.0f); /* Refraction::Infinite -> black (main.rs:610) */
                go = GO_RETURN;
            } else {
                ih = finish_hit(sc, req, cr, false);
                i_in_dir = req.d;
                i_in_mode = req.mode;
                if (phase == DP_REFR_INSIDE) {
                    travel = distance(ih.pos, h.pos);
                    retry = 0;
                } else {
                    travel += distance(req.o, ih.pos);
                    retry += 1;
                }
                go = GO_TRY_EXIT;
            }
        }

        for (;;) {
            if (go == GO_LEVEL) {
                /* distributed_ray_trace(state, &h), depth = max_depth - sp */
                const int32_t depth = fr.max_depth - sp;
                if (depth <= 0) { /* main.rs:524-527 */
                    view_dir_in = h_in_dir;
                    shade_then = 0u;
                    go = GO_START_SHADE;
                    continue;
                }
                const rt_material &rm = sc.materials[h.obj];
                /* weighted_select (main.rs:652-666) */
                const float w0 = (1.0f - rm.shiness) * (1.0f - rm.transparency);
                const float w1 = rm.shiness * (1.0f - rm.transparency);
                const float w2 = rm.transparency;
                float wsum = 0.0f;
                wsum = wsum + w0;
                wsum = wsum + w1;
                wsum = wsum + w2;
                const float rsel = gen_range_f32(rng, 0.0f, wsum);
                float acc = 0.0f;
                acc += w0;
                kind = 2u;
                if (rsel < acc) kind = 0u;
                else {
                    acc += w1;
                    if (rsel < acc) kind = 1u;
                }
                /* scatter_hit (main.rs:539-554) */
                const float exponent = kind == 0u ? 1.0f : rm.smoothness;
                const V3 lobe = kind == 0u ? -h.normal : h_in_dir;
                const float phi = rtdm::acosf(rtdm::powf(1.0f - gen_range_f32(rng, 0.0f, 1.0f), exponent));
                const float theta = gen_range_f32(rng, -RT_F_PI, RT_F_PI);
                float sphi, cphi, stheta, ctheta;
                rtdm::sincosf(phi, &sphi, &cphi);
                rtdm::sincosf(theta, &stheta, &ctheta);
                sdir = adjust_normal(v3(sphi * ctheta, sphi * stheta, cphi), normalize(lobe));
                const float cosine = -dot(h.normal, sdir);
                if (cosine <= 0.0f) { /* main.rs:560, 579, 598 */
                    value = v3(0.0f, 0.0f, 0.0f);
                    go = GO_RETURN;
                    continue;
                }
                if (kind != 2u) {
                    /* get_reflect(&scattered_hit) (main.rs:328-341) */
                    req.o = h.pos;
                    req.d = reflect_dir(h.normal, sdir);
                    req.mode = h_in_mode;
                    req.excl = pack_excl(h.prim, h.bf ? FACE_FRONT : FACE_BACK);
                    phase = DP_NEXT;
                    break;
                }
                /* get_refract(&scattered_hit, 100.0) (main.rs:343-405) */
                V3 refract_in;
                if (refract_dir(h.normal, sdir, rm.refraction_index, &refract_in)) {
                    req.o = h.pos;
                    req.d = normalize(refract_in);
                    req.mode = FACE_BACK;
                    req.excl = pack_excl(h.prim, FACE_FRONT);
                    phase = DP_REFR_INSIDE;
                    break;
                }
                value = v3(0.0f, 0.0f, 0.0f); /* Trapped */
                go = GO_RETURN;
            } else if (go == GO_TRY_EXIT) {
                const rt_material &rm = sc.materials[h.obj];
                V3 out_dir;
                const bool have_out = refract_dir(ih.normal, i_in_dir, 1.0f / rm.refraction_index, &out_dir);
                if (!have_out && travel <= 100.0f && retry < 10) {
                    req.o = ih.pos;
                    req.d = reflect_dir(ih.normal, i_in_dir);
                    req.mode = i_in_mode;
                    req.excl = pack_excl(ih.prim, ih.bf ? FACE_FRONT : FACE_BACK);
                    phase = DP_REFR_BOUNCE;
                    break;
                }
                if (!have_out) { /* Trapped */
                    value = v3(0.0f, 0.0f, 0.0f);
                    go = GO_RETURN;
                    continue;
                }
                req.o = ih.pos; /* escape ray, main.rs:393-401 */
                req.d = normalize(out_dir);
                req.mode = FACE_FRONT;
                req.excl = pack_excl(ih.prim, FACE_BACK);
                phase = DP_NEXT;
                break;
            } else if (go == GO_START_SHADE) {
                /* get_shade(&h') where h' = h with ray.direction = view_dir_in (main.rs:407-412) */
                const Mat m = material_approx(sc.materials[h.obj], h.u, h.v);
                adj_n = adjust_normal(m.normal, h.normal);
                sum = v3(0.0f, 0.0f, 0.0f);
                light_i = 0u;
                go = GO_NEXT_LIGHT;
            } else if (go == GO_NEXT_LIGHT) {
                bool issued = false;
                while (light_i < sc.n_lights) {
                    DirLight dl;
                    if (approximate_into_directional(sc.lights[light_i], h.pos, &dl)) {
                        const float cosine = -dot(dl.direction, adj_n);
                        if (!(cosine <= 0.0f)) {
                            req.o = h.pos;
                            req.d = -dl.direction;
                            req.mode = FACE_BACK;
                            req.excl = pack_excl(h.prim, FACE_BACK);
                            l_color = dl.color;
                            phase = DP_SHADOW;
                            issued = true;
                            break;
                        }
                    }
                    light_i += 1u;
                }
                if (issued) break;
                go = GO_SHADE_DONE;
            } else if (go == GO_SHADE_DONE) {
                if (shade_then == 1u) { /* that was get_shade(&next_hit): keep it and descend (main.rs:565, 584, 604) */
                    stack[sp].shade = sum;
                    sp += 1;
                    go = GO_LEVEL;
                } else {
                    value = sum;
                    go = GO_RETURN;
                }
            } else { /* GO_RETURN */
                if (sp > 0) {
                    const DFrame f = stack[sp - 1];
                    if (f.kind == 2u) {
                        value = (value + f.shade) * f.factor.x; /* main.rs:605 */
                    } else {
                        const V3 s = value * f.factor;           /* main.rs:566, 585 */
                        value = f.shade + (s - f.shade) * 0.5f;  /* palette Mix::mix(&s, 0.5), main.rs:571, 590 */
                    }
                    sp -= 1;
                    continue;
                }
                /* the sample of this (pixel, epoch): filter (main.rs:1157-1160) and accumulate (main.rs:1165) */
                const bool ok = rtdm::is_normal(value.x) && rtdm::is_normal(value.y) && rtdm::is_normal(value.z);
                if (dp.samples != nullptr) {
                    float *o = dp.samples + ((size_t)epoch * n_pixels + out_index) * 3u;
                    o[0] = value.x; o[1] = value.y; o[2] = value.z;
                }
                if (dp.valid != nullptr) dp.valid[(size_t)epoch * n_pixels + out_index] = ok ? 1 : 0;
                if (ok) accum = accum + value;
                epoch += 1u;
                if (epoch < dp.n_epochs) {
                    start_epoch();
                } else { /* this pixel is finished for this call: park its stream position and its sum */
                    rng_park(rng);
                    if (dp.accum != nullptr) {
                        float *o = dp.accum + (size_t)out_index * 3u;
                        o[0] = accum.x; o[1] = accum.y; o[2] = accum.z;
                    }
                    phase = DP_DONE;
                }
                break;
            }
        }
    }

    if (dp.ray_count != nullptr) {
        uint32_t c = casts;
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
        if (lane == 0u && c != 0u) atomicAdd(dp.ray_count, (unsigned long long)c);
    }
}

template <bool RAYS>
static hipError_t launch_distributed_of(const KernelScene &sc, const KernelFrame &fr, const DistParams &dp, uint32_t resident_waves, hipStream_t stream) {
    const uint32_t total = fr.cols * fr.rows;
    uint32_t waves = (total + 63u) / 64u;
    if (waves == 0u) return hipSuccess;
    if (dp.work_queue != nullptr && waves > resident_waves) waves = resident_waves; /* persistent lanes: fill the chip once */
    if (sc.bfs_walk != 0u && dp.bfs_scratch != nullptr && dp.work_queue != nullptr) { /* (the caller sized resident_waves by dist_bfs_waves) */
        if (fr.max_depth <= 8) hipLaunchKernelGGL((distributed_kernel<9, true, RAYS>), dim3(waves), dim3(64), 0, stream, sc, fr, dp);
        else hipLaunchKernelGGL((distributed_kernel<RT_MAX_DEPTH + 1, true, RAYS>), dim3(waves), dim3(64), 0, stream, sc, fr, dp);
        return hipGetLastError();
    }
    if (fr.max_depth <= 8) {
        hipLaunchKernelGGL((distributed_kernel<9, false, RAYS>), dim3(waves), dim3(64), 0, stream, sc, fr, dp);
    } else {
        hipLaunchKernelGGL((distributed_kernel<RT_MAX_DEPTH + 1, false, RAYS>), dim3(waves), dim3(64), 0, stream, sc, fr, dp);
    }
    return hipGetLastError();
}

/* ---- the split pass ----------------------------------------------------------------------------------------------
 * distributed_kernel above keeps a lane on one pixel through everything a sample needs: the scatter chain, every
 * get_shade along it (three shadow casts each) and the unwind — 168 VGPRs with 76 of them spilled, three waves per
 * SIMD, lanes in six different phases.  But get_shade draws no random numbers and the chain does not wait for it:
 * get_shade(&next_hit) is only needed when the level returns (main.rs:565-571, 584-590, 604-605).  So the pass is cut
 * in three:
 *
 *   dist_chain_kernel   the chain alone — shoot_focus, the casts of the scattered/refracted rays, weighted_select,
 *                       scatter_hit, the per-level factor (brdf or decay) — all the random draws, in the reference's
 *                       order; per sample it records the get_shade REQUESTS (hit + view direction) and the frames;
 *   dist_shade_kernel   every request of the batch: get_shade (main.rs:407-464) with a wave-uniform light index — the
 *                       organisation of the Whitted path's SHADE items;
 *   dist_unwind_kernel  per pixel, the batch's epochs in order: the unwind of main.rs:571/590/605 over the recorded
 *                       frames, the sample filter (main.rs:1157-1160) and `img += photon` (main.rs:1165).
 *
 * Same operations on the same values as the fused kernel, so samples, flags, RNG states and cast counts are
 * bit-identical to it and to the oracle (tests/test_gpu_distributed_parity.py runs both). */

/* The shade kernel keeps the wave-uniform cast: pair-wise it was slower, 5.97 against 5.15 ms per 8-epoch batch — its shadow rays
 * need the clusters less sparsely (half of the leaf visits have 8 lanes or more, a quarter 34 or more, against 7 and 25 in the chain
 * kernel) and the 19 KB of PairLds per workgroup cost it two of its six waves per SIMD (profiles/r03p7_*). */
#ifndef RT_DIST_CHAIN_MIN_WAVES
#define RT_DIST_CHAIN_MIN_WAVES 5 /* 96 VGPRs, no more scratch than at 4 (112); 3 / 4 / 5: 709 / 853 / 868 Msamples/s */
#endif

__device__ __forceinline__ uint32_t dfu(float x) { return __float_as_uint(x); }
__device__ __forceinline__ float duf(uint32_t x) { return __uint_as_float(x); }

/* RAYS: as in distributed_kernel — the batch's rays are the roots (instantiated in rt_distributed_rays.hip) */
template <int DUMMY, bool RAYS = false>
__global__ __launch_bounds__(64, RT_DIST_CHAIN_MIN_WAVES) void dist_chain_kernel(const KernelScene sc, const KernelFrame fr, const DistParams dp) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t total_slots = fr.cols * fr.rows;
    const uint32_t band_slots = fr.cols << 3;
    const size_t n_pixels = total_slots;
    const size_t n_samples = n_pixels * dp.n_epochs; /* of this batch */
    /* dp.own_first_chunk: a wave's first chunk is its own — chunk w for wave w: the grid never has more waves than there are chunks */
    uint32_t q_next = dp.own_first_chunk != 0u ? blockIdx.x * 64u : 0u;
    uint32_t q_end = dp.own_first_chunk != 0u ? (q_next + 64u < total_slots ? q_next + 64u : total_slots) : 0u;
    bool exhausted = false;
    uint32_t out_index = 0u;
    float clip_x = 0.0f, clip_y = 0.0f;
    const V3 cam_x = v3(fr.cam_x[0], fr.cam_x[1], fr.cam_x[2]);
    const V3 cam_y = v3(fr.cam_y[0], fr.cam_y[1], fr.cam_y[2]);
    const V3 cam_t = v3(fr.cam_toward[0], fr.cam_toward[1], fr.cam_toward[2]);
    const V3 cam_o = v3(fr.cam_origin_focus[0], fr.cam_origin_focus[1], fr.cam_origin_focus[2]);

    /* one wave per workgroup.  The pair-wise cast's scratch SHARES the refill's staging area — one union, so that the compiler sees the
     * two views alias — because a generator is refilled between casts, never during one: every refill (rng_open /
     * refill in start_epoch and rt_dist_advance.inc) completes, LDS traffic included, before the step's cast_pairs call, and the
     * cast has returned before the next one.  With 8 KB per wave the kernel sits exactly at five waves per SIMD; anything on top
     * would cost the fifth. */
    union ChainLds {
        uint32_t stage[RNG_LDS_SLOTS * 256u];
        PairLds pairs;
    };
    __shared__ __attribute__((aligned(16))) ChainLds chain_lds;
    static_assert(sizeof(PairLds) <= sizeof(chain_lds.stage), "PairLds must fit the staging area");
    PairLds *const pair_lds = &chain_lds.pairs;
    Rng rng;
    rng.rec = rng.st = dp.rng_states;
    rng.index = 256u;
    rng.flags = 0u;
    rng.lds = chain_lds.stage;
    uint32_t phase = DP_DONE;
    uint32_t epoch = 0u;
    Ray req;
    req.o = v3(0.0f, 0.0f, 0.0f);
    req.d = v3(0.0f, 0.0f, 1.0f);
    req.mode = FACE_FRONT;
    req.excl = 0u;
    uint32_t casts = 0u;
    HitGeom h;
    h.pos = h.normal = v3(0.0f, 0.0f, 0.0f);
    h.u = h.v = 0.0f;
    h.prim = h.bf = h.obj = 0u;
    V3 h_in_dir = v3(0.0f, 0.0f, 0.0f);
    uint32_t h_in_mode = FACE_FRONT;
    V3 sdir = v3(0.0f, 0.0f, 0.0f);
    uint32_t kind = 0u;
    int32_t sp = 0; /* frames recorded so far = the level */
    float travel = 0.0f;
    int32_t retry = 0;

    auto start_epoch = [&]() { /* Camera::shoot_focus (main.rs:101-127) */
        if constexpr (RAYS) { /* the caller's ray, the same in every epoch */
            req = ray_from_abi(frame_rays(fr) + out_index, sc.n_triangles, sc.n_spheres);
            sp = 0;
            phase = DP_PRIMARY;
            return;
        }
        const V3 direction = normalize(clip_x * cam_x + clip_y * cam_y + cam_t);
        double nx, ny;
        standard_normal_x2(rng, &nx, &ny);
        const float xoffset = (float)(0.0 + (double)dp.blur * nx);
        const float yoffset = (float)(0.0 + (double)dp.blur * ny);
        req.d = normalize(direction * dp.focus + cam_x * xoffset + cam_y * yoffset);
        req.o = cam_o - (cam_x * xoffset + cam_y * yoffset);
        req.mode = FACE_FRONT;
        req.excl = 0u;
        sp = 0;
        phase = DP_PRIMARY;
    };
    /* get_shade(&h') with h' = h seen along `view` is due: leave it to dist_shade_kernel, in request slot sp */
    auto emit_request = [&](V3 view) {
        const size_t s = (size_t)epoch * n_pixels + out_index;
        uint4 *r = dp.sp_req + ((size_t)sp * n_samples + s) * 4u;
        r[0] = make_uint4(dfu(h.pos.x), dfu(h.pos.y), dfu(h.pos.z), dfu(h.u));
        r[1] = make_uint4(dfu(h.normal.x), dfu(h.normal.y), dfu(h.normal.z), dfu(h.v));
        r[2] = make_uint4(dfu(view.x), dfu(view.y), dfu(view.z), h.obj);
        r[3] = make_uint4(h.prim, 0u, 0u, 0u);
    };

#ifdef RT_DIAG_PAIR_TIME /* per wave: [0] steps, [1..7] rt_cast.h, [8] the kernel, [9] fetching work + shoot_focus, [10] after the cast: the hit and the
                          * level's factor, [11] the level's draws and scatter_hit, [12] get_refract's exit, [13] the rest of the step */
    unsigned long long diag_dt[16] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull}; /* [14] lanes at work, summed over the steps; [15] steps after the work queue ran dry */
    const unsigned long long diag_t0 = __builtin_readcyclecounter();
    unsigned long long diag_tick = diag_t0;
#define RT_STEP_TICK(k) { const unsigned long long now_ = __builtin_readcyclecounter(); diag_dt[k] += now_ - diag_tick; diag_tick = now_; }
#else
#define RT_STEP_TICK(k)
#endif
    for (;;) {
        unsigned long long need = __builtin_amdgcn_ballot_w64(phase == DP_DONE);
        if (dp.n_epochs == 0u) need = 0ull;
        while (need != 0ull) {
            if (q_next == q_end) {
                if (exhausted) break;
                uint32_t c = 0u;
                if (lane == 0u) c = atomicAdd(dp.work_queue, 1u);
                c = (uint32_t)__builtin_amdgcn_readfirstlane((int)c) + (dp.own_first_chunk != 0u ? gridDim.x : 0u); /* with own first chunks, 0 .. G - 1 are taken */
                if (c * 64u >= total_slots) { exhausted = true; break; }
                q_next = c * 64u;
                q_end = q_next + 64u < total_slots ? q_next + 64u : total_slots;
            }
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
            const uint32_t avail = q_end - q_next;
            if (phase == DP_DONE && rank < avail) {
                const uint32_t slot = q_next + rank;
                uint32_t row = 0u, col = 0u;
                if constexpr (RAYS) { /* one row: slot i is ray i */
                    out_index = DUMMY != 0 ? dp.pixel_order[slot] : slot;
                } else if (DUMMY != 0) { /* instantiation 1: the pixels grouped by cost (rt_kernels.h); its own, so that instantiation 0 does not carry it */
                    out_index = dp.pixel_order[slot];
                    row = out_index / fr.cols;
                    col = out_index - row * fr.cols;
                } else { /* the image in 8-row bands, column by column: a chunk is an 8 x 8 tile */
                    const uint32_t band = slot / band_slots;
                    const uint32_t r = slot - band * band_slots;
                    const uint32_t rows_left = fr.rows - (band << 3);
                    const uint32_t band_rows = rows_left < 8u ? rows_left : 8u;
                    col = r / band_rows;
                    row = (band << 3) + (r - col * band_rows);
                    out_index = row * fr.cols + col;
                }
                if constexpr (!RAYS) {
                    const uint32_t x = fr.x0 + col, y = fr.y0 + row * fr.y_step;
                    clip_y = (fr.half_height - (float)y) / fr.height_f;
                    clip_x = ((float)x - fr.half_width) / fr.height_f;
                }
                rng_open(rng, dp.rng_states + (size_t)out_index * RNG_WORDS);
                epoch = 0u;
                phase = DP_START;
            }
            const uint32_t n_need = (uint32_t)__builtin_popcountll(need);
            q_next += n_need < avail ? n_need : avail;
            need = __builtin_amdgcn_ballot_w64(phase == DP_DONE);
        }
        if (__builtin_amdgcn_ballot_w64(phase != DP_DONE) == 0ull) break;
        /* one copy of each expensive piece per iteration — the lanes of a wave are in all phases at once, so whatever
         * appears in several branches is executed several times over */
        if (phase == DP_START) start_epoch();

        CastResult cr;
#ifdef RT_DIAG_PAIR_TIME
        RT_STEP_TICK(9)
        cr = cast_pairs(sc, req, phase != DP_DONE, pair_lds, diag_dt);
        diag_dt[0] += 1ull;
        diag_dt[14] += (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(phase != DP_DONE));
        if (exhausted) diag_dt[15] += 1ull;
        diag_tick = __builtin_readcyclecounter();
#else
        cr = cast_pairs(sc, req, phase != DP_DONE, pair_lds); /* all lanes: the idle ones help with the others' pairs */
#endif
        if (phase == DP_DONE) continue;
        casts += 1u;

#include "rt_dist_advance.inc"
        if (!casting) { /* the chain of this (pixel, epoch) is over */
            dp.sp_hdr[(size_t)epoch * n_pixels + out_index] = (uint32_t)sp | (terminal ? 0x100u : 0u);
            epoch += 1u;
            if (epoch < dp.n_epochs) {
                phase = DP_START;
            } else {
                rng_park(rng); /* the stream position */
                phase = DP_DONE;
            }
        }
        RT_STEP_TICK(13)
    }

#ifdef RT_DIAG_PAIR_TIME
    diag_dt[8] = __builtin_readcyclecounter() - diag_t0;
    if (lane == 0u) {
        for (int q = 0; q < 16; ++q) atomicAdd(&g_pair_time[q], diag_dt[q]);
        atomicMax(&g_chain_critical[0], diag_dt[0]); /* the wave that made the most steps, the wave that ran longest: what a launch cannot be shorter than */
        atomicMax(&g_chain_critical[1], diag_dt[8]);
        atomicAdd(&g_chain_critical[2], 1ull);
    }
#endif
    if (dp.ray_count != nullptr) {
        uint32_t c = casts;
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
        if (lane == 0u && c != 0u) atomicAdd(dp.ray_count, (unsigned long long)c);
    }
}

/* (Round 2 also had the chain as a kernel of workgroup-local queues — every cast a work item, START / NEXT / REFR queues, phase-
 * coherent chunks, the organisation of the Whitted path.  It lost to the persistent lanes above twice: 2.35 against 2.28 ms per epoch
 * in round 2, 1 015 against 1 136 Msamples/s in round 3 with the pair-wise cast in both (profiles/README.md), and is gone.) */

template <bool RAYS>
static hipError_t launch_dist_chain_of(const KernelScene &sc, const KernelFrame &fr, const DistParams &dp, uint32_t resident_waves, hipStream_t stream) {
    const uint32_t total = fr.cols * fr.rows;
    if (total == 0u || dp.n_epochs == 0u) return hipSuccess;
    uint32_t waves = (total + 63u) / 64u;
    const uint32_t chain_waves = dist_chain_waves(resident_waves);
    if (waves > chain_waves) waves = chain_waves;
    if (dp.pixel_order != nullptr) hipLaunchKernelGGL((dist_chain_kernel<1, RAYS>), dim3(waves), dim3(64), 0, stream, sc, fr, dp);
    else hipLaunchKernelGGL((dist_chain_kernel<0, RAYS>), dim3(waves), dim3(64), 0, stream, sc, fr, dp);
    return hipGetLastError();
}

} /* namespace rt */

#endif /* RT_DIST_KERNELS_H */
