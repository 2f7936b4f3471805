/*
 * rt_path_query.hip — the inner step of a path tracer on caller-supplied hits (include/rt_amd.h "path queries"): a record per path
 * that carries the throughput from bounce to bounce, one kernel that does between two casts what rt_material_hits, rt_lobe_rays,
 * rt_probe_surfaces, rt_mis_weigh and rt_environment_fold do in five, ends paths by Russian roulette on the device, and the mean of a
 * pixel's paths at the end.
 *
 *   rt::path_begin_kernel     per (sample, root): the record of a fresh path, and its radiance zeroed
 *   rt::path_advance_kernel   per listed path: deposit, escape, sample, terms, throughput, roulette; the next ray or the end
 *   rt::path_resolve_kernel   per root: the samples' radiance in ascending order, their mean added to the root's slot
 *
 * The arithmetic is rt_path.h's, shared with librt_host.so, and that header calls rt_lobe.h's sampler and rt_shade.h's terms as
 * lobe_rays_kernel and probe_surfaces_kernel call them: the record and the sampling normal are rt_light_record.h's.  The ray a survivor
 * goes on along is no shadow ray: it looks for the path's next vertex, the nearest surface whichever way it faces, so it is cast with
 * face Both and the vertex's own primitive excluded for both faces (store_continuation_ray); Back is an occlusion query's face.
 * One listed path (or root) per lane, 256 lanes per workgroup; the path record moves as two 16-byte accesses, the hit and the rays as
 * dwords.  No LDS, no cast, no workspace, no atomics.  The C entry points of the block are at the end of the file.
 */
#include "rt_api_internal.h"
#include "rt_light_record.h"
#include "rt_path.h"

namespace rt {

#define RT_PATH_THREADS 256u
#define RT_PATH_RAY_DIRECTION 3u /* word of rt_ray.direction */
#define RT_PATH_HIT_WORDS 13u
static_assert(sizeof(rt_hit) == RT_PATH_HIT_WORDS * sizeof(uint32_t), "rt_hit is 13 dwords");

__global__ __launch_bounds__(RT_PATH_THREADS) void path_begin_kernel(const uint64_t n, const uint32_t spp, const uint32_t *__restrict__ ids,
                                                                     rt_path *__restrict__ paths, float *__restrict__ radiance) {
    const uint64_t k = (uint64_t)blockIdx.x * RT_PATH_THREADS + threadIdx.x;
    if (k >= n * spp) return;
    const uint64_t i = k % n;
    const rt_path p = path_begin_record((uint32_t)i, record_id(ids, i), (uint32_t)(k / n));
    uint4 *const out = reinterpret_cast<uint4 *>(paths + k);
    out[0] = make_uint4(__float_as_uint(p.beta[0]), __float_as_uint(p.beta[1]), __float_as_uint(p.beta[2]), __float_as_uint(p.pdf));
    out[1] = make_uint4(p.root, p.id, p.bounce, p.flags);
    store_v3(radiance, k, v3(0.0f, 0.0f, 0.0f));
}

/* the ray a path goes on along: rt_light_record.h's shadow ray — from the hit along `dir`, the hit's own primitive excluded — with its
 * two face words Both in the place of Back, or all-zero words for a path that ended */
__device__ __forceinline__ void store_continuation_ray(rt_ray *__restrict__ ray, const LightRecord &r, const V3 dir, const bool lives) {
    if (lives)
        store_ray(ray, r.h.g.pos, dir, FACE_BOTH, 1u, r.h.kind, r.h.index, FACE_BOTH);
    else
        store_ray(ray, v3(0.0f, 0.0f, 0.0f), v3(0.0f, 0.0f, 0.0f), 0u, 0u, 0u, 0u, 0u);
}

/* hits is read (the record's own slot) and, for a path that ends, written: not restrict, not const */
__global__ __launch_bounds__(RT_PATH_THREADS) void path_advance_kernel(const KernelScene sc, rt_path *__restrict__ paths, const uint32_t m,
                                                                       const uint32_t *__restrict__ index, const uint32_t *__restrict__ count, rt_hit *hits,
                                                                       const rt_ray *__restrict__ incoming, const float *__restrict__ emitted,
                                                                       const PathStep step, const uint32_t normal_kind, float *__restrict__ radiance,
                                                                       rt_ray *__restrict__ next_rays, unsigned char *__restrict__ alive) {
    const uint64_t lane = (uint64_t)blockIdx.x * RT_PATH_THREADS + threadIdx.x;
    if (lane >= path_listed(index, count, m)) return;
    const uint32_t j = index != nullptr ? index[lane] : (uint32_t)lane;
    if (j >= m) return; /* an index beyond the slots names nothing, as in rt_cast_rays_indexed */
    uint4 *const record = reinterpret_cast<uint4 *>(paths + j);
    const uint4 lo = record[0], hi = record[1];
    if ((hi.w & RT_PATH_ALIVE) == 0u) return;
    rt_path p;
    p.beta[0] = __uint_as_float(lo.x);
    p.beta[1] = __uint_as_float(lo.y);
    p.beta[2] = __uint_as_float(lo.z);
    p.pdf = __uint_as_float(lo.w);
    p.root = hi.x;
    p.id = hi.y;
    p.bounce = hi.z;
    p.flags = hi.w;

    if (emitted != nullptr) {
        const V3 e = load_v3(emitted, j), l = load_v3(radiance, j);
        store_v3(radiance, j, v3(path_deposit(l.x, p.beta[0], e.x), path_deposit(l.y, p.beta[1], e.y), path_deposit(l.z, p.beta[2], e.z)));
    }

    const LightRecord r = light_record(sc, hits, j);
    V3 view = v3(0.0f, 0.0f, 1.0f);
    if (r.valid) {
        const float *const d = reinterpret_cast<const float *>(incoming + j) + RT_PATH_RAY_DIRECTION;
        view = -v3(d[0], d[1], d[2]); /* what get_shade passes as view_direction */
    }
    V3 dir;
    const bool lives = path_advance_record(p, r.valid, r.m, r.adj_n, sampling_normal(r, normal_kind), view, step, &dir);

    record[0] = make_uint4(__float_as_uint(p.beta[0]), __float_as_uint(p.beta[1]), __float_as_uint(p.beta[2]), __float_as_uint(p.pdf));
    record[1] = make_uint4(p.root, p.id, p.bounce, p.flags);
    alive[j] = lives ? 1 : 0;
    store_continuation_ray(next_rays + j, r, dir, lives);
    if (!lives) { /* "no hit", as the tree loop presets it: a later rt_shade_hits spends nothing here, a later advance escapes at once */
        uint32_t *const preset = reinterpret_cast<uint32_t *>(hits + j);
#pragma unroll
        for (uint32_t k = 0; k < RT_PATH_HIT_WORDS; ++k) preset[k] = k == 0u ? RT_HIT_NONE : 0u;
    }
}

__global__ __launch_bounds__(RT_PATH_THREADS) void path_resolve_kernel(const float *__restrict__ radiance, const uint64_t n, const uint32_t spp,
                                                                       const uint32_t *__restrict__ root, float *__restrict__ rgb) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_PATH_THREADS + threadIdx.x;
    if (i >= n) return;
    path_resolve_root(radiance, n, spp, i, root, rgb);
}

} /* namespace rt */

/* ---- the C entry points (include/rt_amd.h "path queries") ---- */

static bool aligned_16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0u; }

extern "C" {

int rt_path_begin(size_t n, uint32_t spp, const uint32_t *d_ids, rt_path *d_paths, float *d_radiance, void *hip_stream) {
    const char *const who = "rt_path_begin";
    bool done;
    const int rc = hit_sample_args(who, nullptr,
                                   HitSampleArgs(n, d_paths && d_radiance, "path or radiance").no_scene().samples(spp).limits(rt::hemisphere_limits(spp, false, 0u, 0u)),
                                   &done);
    if (rc != RT_OK || done) return rc;
    if (!aligned_16(d_paths)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": d_paths is not 16-byte aligned");
    hipLaunchKernelGGL(rt::path_begin_kernel, grid_of((uint64_t)n * spp, RT_PATH_THREADS), dim3(RT_PATH_THREADS), 0, static_cast<hipStream_t>(hip_stream),
                       (uint64_t)n, spp, d_ids, d_paths, d_radiance);
    return launched(who);
}

/* rt_lobe_rays' checks (hit_sample_args, rt_api_internal.h) on the m slots, then rr_floor, then the record's alignment */
int rt_path_advance(const rt_scene *scene, rt_path *d_paths, size_t m, const uint32_t *d_index, const uint32_t *d_count, rt_hit *d_hits,
                    const rt_ray *d_incoming, const float *d_emitted, uint32_t seed, uint32_t normal_kind, uint32_t rr_start, float rr_floor, int last,
                    float *d_radiance, rt_ray *d_next_rays, unsigned char *d_alive, void *hip_stream) {
    const char *const who = "rt_path_advance";
    bool done;
    const int rc = hit_sample_args(who, scene,
                                   HitSampleArgs(m, d_paths && (d_index == nullptr || d_count != nullptr) && d_hits && d_incoming && d_radiance && d_next_rays && d_alive,
                                                 "path, count (with an index), hit, incoming-ray, radiance, ray or flag")
                                       .limits(rt::path_limits(normal_kind, rr_floor)), &done);
    if (rc != RT_OK || done) return rc;
    if (!aligned_16(d_paths)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": d_paths is not 16-byte aligned");
    const rt::PathStep step = {seed, rr_start, rr_floor, last != 0};
    hipLaunchKernelGGL(rt::path_advance_kernel, grid_of(m, RT_PATH_THREADS), dim3(RT_PATH_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks, d_paths,
                       (uint32_t)m, d_index, d_count, d_hits, d_incoming, d_emitted, step, normal_kind, d_radiance, d_next_rays, d_alive);
    return launched(who);
}

int rt_path_resolve(const float *d_radiance, size_t n, uint32_t spp, const uint32_t *d_root, float *d_rgb, void *hip_stream) {
    const char *const who = "rt_path_resolve";
    bool done;
    const int rc = hit_sample_args(who, nullptr,
                                   HitSampleArgs(n, d_radiance && d_rgb, "radiance or rgb").no_scene().samples(spp).limits(rt::hemisphere_limits(spp, false, 0u, 0u)),
                                   &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::path_resolve_kernel, grid_of(n, RT_PATH_THREADS), dim3(RT_PATH_THREADS), 0, static_cast<hipStream_t>(hip_stream), d_radiance, (uint64_t)n,
                       spp, d_root, d_rgb);
    return launched(who);
}

} /* extern "C" */
