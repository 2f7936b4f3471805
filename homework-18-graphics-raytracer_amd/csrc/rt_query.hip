/*
 * rt_query.hip — ray queries: World::cast (main.rs:180-326) on caller-supplied rays, and the primary rays of a frame
 * (Camera::shoot, main.rs:83-99).  Nothing here is new arithmetic: the casts are rt_cast.h's cast_pairs / cast_asm /
 * cast_bfs and finish_hit exactly as the render kernels call them, so their exactness arguments carry over unchanged; what
 * is new is reading rays from and writing hits to the ABI records of include/rt_amd.h.
 *
 *   rt::cast_rays_kernel       one wave per 64 rays, all 64 lanes executing (the tail wave passes active = false for lanes
 *                              past the end): cast_pairs — the rays of a batch are unrelated by contract, the case it was
 *                              built for (rt_cast.h) — or, with RT_AMD_QUERY_WAVE_UNIFORM, cast_asm for every wave
 *   rt::cast_rays_bfs_kernel   scenes with KernelScene::bfs_walk: cast_bfs over 64-ray chunks, a grid of resident waves
 *                              taking chunks grid-stride (no atomic counter: nothing to reset, capturable)
 *   rt::cast_rays_indexed_kernel, rt::cast_rays_indexed_bfs_kernel   the same two with the ray number taken from an index list and
 *                              the bound from a device-side count (rt_cast_rays_indexed)
 *   rt::camera_rays_kernel     one work-item per pixel of a tile, in its compact row order
 */
#include "rt_cast.h"
#include "rt_primary_ray.h"

namespace rt {

/* the Hit of main.rs:139-147 as the ABI record; a miss is RT_HIT_NONE with every other field 0 */
template <class Scene>
__device__ __forceinline__ void store_hit(const Scene &sc, const Ray &ray, const CastResult &cr, rt_hit *__restrict__ out) {
    uint32_t w[13] = {RT_HIT_NONE, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (cr.prim >= 0) {
        const HitGeom h = finish_hit(sc, ray, cr, true); /* a sphere hit always carries its uv (main.rs:310-313) */
        const bool tri = h.prim < sc.n_triangles;
        w[0] = tri ? 1u : 0u;
        w[1] = tri ? h.prim : h.prim - sc.n_triangles;
        w[2] = h.obj;
        w[3] = __float_as_uint(h.pos.x); w[4] = __float_as_uint(h.pos.y); w[5] = __float_as_uint(h.pos.z);
        w[6] = __float_as_uint(h.normal.x); w[7] = __float_as_uint(h.normal.y); w[8] = __float_as_uint(h.normal.z);
        w[9] = __float_as_uint(h.u); w[10] = __float_as_uint(h.v);
        w[11] = h.bf;
        w[12] = __float_as_uint(cr.t);
    }
    uint32_t *const o = reinterpret_cast<uint32_t *>(out);
#pragma unroll
    for (int k = 0; k < 13; ++k) o[k] = w[k];
}

/* Launch bounds, LDS and register budget as dist_shade_kernel's (rt_distributed.hip), the other kernel whose waves run cast_pairs
 * on unrelated rays: 256 threads, 6 waves per SIMD (80 VGPRs), one PairLdsSlim per wave (2.8 KB; the hand-scheduled loop owns
 * s34..s99, the Makefile's -disable-machine-licm keeps loop-invariant scalars from being parked around it). */
#ifndef RT_QUERY_THREADS
#define RT_QUERY_THREADS 256
#endif
#ifndef RT_QUERY_MIN_WAVES
#define RT_QUERY_MIN_WAVES 6
#endif
template <bool WAVE_UNIFORM>
__global__ __launch_bounds__(RT_QUERY_THREADS, RT_QUERY_MIN_WAVES) void cast_rays_kernel(const KernelScene sc, const rt_ray *__restrict__ rays,
                                                                                        rt_hit *__restrict__ hits, const uint32_t n_rays) {
    const uint32_t first = blockIdx.x * RT_QUERY_THREADS + (threadIdx.x & ~63u); /* the wave's first ray */
    if (first >= n_rays) return;                                                  /* whole waves only */
    const uint32_t i = first + (threadIdx.x & 63u);
    const bool active = i < n_rays;
    Ray ray;
    if (active) ray = ray_from_abi(rays + i, sc.n_triangles, sc.n_spheres);
    else {
        ray.o = v3(0.0f, 0.0f, 0.0f);
        ray.d = v3(0.0f, 0.0f, 1.0f);
        ray.mode = FACE_FRONT;
        ray.excl = 0u;
    }
    CastResult cr;
    cr.prim = -1;
    cr.t = 0.0f;
    cr.bf = 0u;
    cr.a0 = cr.a1 = cr.a2 = 0.0f;
    if constexpr (WAVE_UNIFORM) {
        if (active) cr = cast_asm(sc, ray);
    } else {
        __shared__ PairLdsSlim pair_lds_all[RT_QUERY_THREADS / 64];
        cr = cast_pairs(sc, ray, active, &pair_lds_all[threadIdx.x >> 6]); /* all 64 lanes: those past the end help */
    }
    if (active) store_hit(sc, ray, cr, hits + i);
}

/* The breadth-first walk (rt_cast_bfs.h) as pwf_kernel<.., BFS> runs it: 256 VGPRs, RT_QUERY_BFS_WAVES waves per workgroup and one
 * workgroup per CU, one BfsLds per wave (5 KB) and one set of record lists per wave of the grid. */
__global__ __launch_bounds__(RT_QUERY_BFS_WAVES * 64u, 2) void cast_rays_bfs_kernel(const KernelScene sc, const rt_ray *__restrict__ rays,
                                                                                   rt_hit *__restrict__ hits, const uint32_t n_rays,
                                                                                   uint32_t *bfs_scratch, const uint32_t items_cap,
                                                                                   const uint32_t jobs_cap) {
    __shared__ BfsLds bfs_lds_all[RT_QUERY_BFS_WAVES];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * RT_QUERY_BFS_WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * RT_QUERY_BFS_WAVES;
    BfsLds *const bl = &bfs_lds_all[threadIdx.x >> 6];
    BfsScratch ws;
    uint2 *const mine = reinterpret_cast<uint2 *>(bfs_scratch) + (size_t)wave * (2u * (size_t)items_cap + jobs_cap);
    ws.items_a = mine;
    ws.items_b = mine + items_cap;
    ws.jobs = mine + 2u * (size_t)items_cap;
    ws.items_cap = items_cap;
    ws.jobs_cap = jobs_cap;
    const uint32_t n_chunks = (n_rays + 63u) / 64u;
    for (uint32_t chunk = wave; chunk < n_chunks; chunk += n_waves) { /* wave-uniform */
        const uint32_t i = chunk * 64u + lane;
        const bool active = i < n_rays;
        Ray ray;
        if (active) ray = ray_from_abi(rays + i, sc.n_triangles, sc.n_spheres);
        else {
            ray.o = v3(0.0f, 0.0f, 0.0f);
            ray.d = v3(0.0f, 0.0f, 1.0f);
            ray.mode = FACE_FRONT;
            ray.excl = 0u;
        }
        const CastResult cr = cast_bfs(sc, ray, active, bl, ws); /* all lanes: those past the end help */
        if (active) store_hit(sc, ray, cr, hits + i);
    }
}

/* ---- the same casts through an index list (rt_cast_rays_indexed): entry j of the list names the ray, the device-side count bounds j ----
 * A wave takes 64 consecutive ENTRIES; the hit goes to the record of the ray it names, so records that are not named are not written.
 * An entry at or beyond n_rays is skipped: its lane only helps, as a lane beyond the count does. */

/* the ray of a lane that has none of its own: it misses everything and only helps */
__device__ __forceinline__ Ray idle_ray() {
    Ray ray;
    ray.o = v3(0.0f, 0.0f, 0.0f);
    ray.d = v3(0.0f, 0.0f, 1.0f);
    ray.mode = FACE_FRONT;
    ray.excl = 0u;
    return ray;
}

__device__ __forceinline__ uint32_t indexed_count(const uint32_t *__restrict__ count, uint32_t max_count) {
    const uint32_t c = *count;
    return c < max_count ? c : max_count;
}

template <bool WAVE_UNIFORM>
__global__ __launch_bounds__(RT_QUERY_THREADS, RT_QUERY_MIN_WAVES) void cast_rays_indexed_kernel(const KernelScene sc, const rt_ray *__restrict__ rays,
                                                                                                rt_hit *__restrict__ hits, const uint32_t n_rays,
                                                                                                const uint32_t *__restrict__ index,
                                                                                                const uint32_t *__restrict__ count, const uint32_t max_count,
                                                                                                unsigned long long *ray_count) {
    const uint32_t n_entries = indexed_count(count, max_count);
    const uint32_t first = blockIdx.x * RT_QUERY_THREADS + (threadIdx.x & ~63u); /* the wave's first entry */
    if (first >= n_entries) return;                                              /* whole waves only, before LDS is touched */
    const uint32_t j = first + (threadIdx.x & 63u);
    const uint32_t i = j < n_entries ? index[j] : 0xffffffffu;
    const bool active = j < n_entries && i < n_rays;
    const Ray ray = active ? ray_from_abi(rays + i, sc.n_triangles, sc.n_spheres) : idle_ray();
    CastResult cr;
    cr.prim = -1;
    cr.t = 0.0f;
    cr.bf = 0u;
    cr.a0 = cr.a1 = cr.a2 = 0.0f;
    if constexpr (WAVE_UNIFORM) {
        if (active) cr = cast_asm(sc, ray);
    } else {
        __shared__ PairLdsSlim pair_lds_all[RT_QUERY_THREADS / 64];
        cr = cast_pairs(sc, ray, active, &pair_lds_all[threadIdx.x >> 6]); /* all 64 lanes: those without a ray help */
    }
    if (active) store_hit(sc, ray, cr, hits + i);
    if (ray_count != nullptr) {
        const unsigned long long cast = __ballot(active);
        if ((threadIdx.x & 63u) == 0u && cast != 0ull) atomicAdd(ray_count, (unsigned long long)__popcll(cast));
    }
}

__global__ __launch_bounds__(RT_QUERY_BFS_WAVES * 64u, 2) void cast_rays_indexed_bfs_kernel(const KernelScene sc, const rt_ray *__restrict__ rays,
                                                                                           rt_hit *__restrict__ hits, const uint32_t n_rays,
                                                                                           const uint32_t *__restrict__ index,
                                                                                           const uint32_t *__restrict__ count, const uint32_t max_count,
                                                                                           unsigned long long *ray_count, uint32_t *bfs_scratch,
                                                                                           const uint32_t items_cap, const uint32_t jobs_cap) {
    __shared__ BfsLds bfs_lds_all[RT_QUERY_BFS_WAVES];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * RT_QUERY_BFS_WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * RT_QUERY_BFS_WAVES;
    BfsLds *const bl = &bfs_lds_all[threadIdx.x >> 6];
    BfsScratch ws;
    uint2 *const mine = reinterpret_cast<uint2 *>(bfs_scratch) + (size_t)wave * (2u * (size_t)items_cap + jobs_cap);
    ws.items_a = mine;
    ws.items_b = mine + items_cap;
    ws.jobs = mine + 2u * (size_t)items_cap;
    ws.items_cap = items_cap;
    ws.jobs_cap = jobs_cap;
    const uint32_t n_entries = indexed_count(count, max_count);
    const uint32_t n_chunks = (n_entries >> 6) + ((n_entries & 63u) != 0u ? 1u : 0u);
    uint32_t casts = 0u;
    for (uint32_t chunk = wave; chunk < n_chunks; chunk += n_waves) { /* wave-uniform */
        const uint32_t j = chunk * 64u + lane;
        const uint32_t i = j < n_entries ? index[j] : 0xffffffffu;
        const bool active = j < n_entries && i < n_rays;
        const Ray ray = active ? ray_from_abi(rays + i, sc.n_triangles, sc.n_spheres) : idle_ray();
        const CastResult cr = cast_bfs(sc, ray, active, bl, ws); /* all lanes: those without a ray help */
        if (active) store_hit(sc, ray, cr, hits + i);
        casts += (uint32_t)__popcll(__ballot(active));
    }
    if (ray_count != nullptr && lane == 0u && casts != 0u) atomicAdd(ray_count, (unsigned long long)casts);
}

/* Camera::shoot(clip(x, y)): primary_ray and the record it is written as are rt_primary_ray.h's, shared with rt_film_query.hip */
__global__ __launch_bounds__(256) void camera_rays_kernel(const KernelFrame fr, rt_ray *__restrict__ rays) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= fr.cols * fr.rows) return;
    const uint32_t row = i / fr.cols, col = i - row * fr.cols;
    store_primary_ray(primary_ray(fr, col, row), rays + i);
}

hipError_t launch_cast_rays(const KernelScene &sc, const rt_ray *rays, rt_hit *hits, uint32_t n_rays, bool wave_uniform, hipStream_t stream) {
    if (n_rays == 0u) return hipSuccess;
    const uint32_t groups = (uint32_t)(((uint64_t)n_rays + RT_QUERY_THREADS - 1u) / RT_QUERY_THREADS);
    if (wave_uniform) hipLaunchKernelGGL(cast_rays_kernel<true>, dim3(groups), dim3(RT_QUERY_THREADS), 0, stream, sc, rays, hits, n_rays);
    else hipLaunchKernelGGL(cast_rays_kernel<false>, dim3(groups), dim3(RT_QUERY_THREADS), 0, stream, sc, rays, hits, n_rays);
    return hipGetLastError();
}

hipError_t launch_cast_rays_bfs(const KernelScene &sc, const rt_ray *rays, rt_hit *hits, uint32_t n_rays, uint32_t *bfs_scratch,
                                uint32_t items_cap, uint32_t jobs_cap, uint32_t bfs_groups, hipStream_t stream) {
    if (n_rays == 0u || bfs_groups == 0u) return hipSuccess;
    hipLaunchKernelGGL(cast_rays_bfs_kernel, dim3(bfs_groups), dim3(RT_QUERY_BFS_WAVES * 64u), 0, stream, sc, rays, hits, n_rays, bfs_scratch,
                       items_cap, jobs_cap);
    return hipGetLastError();
}

hipError_t launch_cast_rays_indexed(const KernelScene &sc, const rt_ray *rays, rt_hit *hits, uint32_t n_rays, const uint32_t *index,
                                    const uint32_t *count, uint32_t max_count, unsigned long long *ray_count, bool wave_uniform, hipStream_t stream) {
    if (n_rays == 0u || max_count == 0u) return hipSuccess;
    const uint32_t groups = (uint32_t)(((uint64_t)max_count + RT_QUERY_THREADS - 1u) / RT_QUERY_THREADS);
    if (wave_uniform)
        hipLaunchKernelGGL(cast_rays_indexed_kernel<true>, dim3(groups), dim3(RT_QUERY_THREADS), 0, stream, sc, rays, hits, n_rays, index, count,
                           max_count, ray_count);
    else
        hipLaunchKernelGGL(cast_rays_indexed_kernel<false>, dim3(groups), dim3(RT_QUERY_THREADS), 0, stream, sc, rays, hits, n_rays, index, count,
                           max_count, ray_count);
    return hipGetLastError();
}

hipError_t launch_cast_rays_indexed_bfs(const KernelScene &sc, const rt_ray *rays, rt_hit *hits, uint32_t n_rays, const uint32_t *index,
                                        const uint32_t *count, uint32_t max_count, unsigned long long *ray_count, uint32_t *bfs_scratch,
                                        uint32_t items_cap, uint32_t jobs_cap, uint32_t bfs_groups, hipStream_t stream) {
    if (n_rays == 0u || max_count == 0u || bfs_groups == 0u) return hipSuccess;
    hipLaunchKernelGGL(cast_rays_indexed_bfs_kernel, dim3(bfs_groups), dim3(RT_QUERY_BFS_WAVES * 64u), 0, stream, sc, rays, hits, n_rays, index, count,
                       max_count, ray_count, bfs_scratch, items_cap, jobs_cap);
    return hipGetLastError();
}

hipError_t launch_camera_rays(const KernelFrame &fr, rt_ray *rays, hipStream_t stream) {
    const uint64_t n = (uint64_t)fr.cols * fr.rows;
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(camera_rays_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, stream, fr, rays);
    return hipGetLastError();
}

} /* namespace rt */
