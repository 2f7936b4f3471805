/*
 * rt_path_kernel.h — what the kernels of the path loop do per lane around their own arithmetic, written once for the four units that
 * work on listed rt_path records: rt_path_query.hip, rt_transmit_query.hip, rt_connect_query.hip and rt_light_connect_query.hip.
 * Device code only; every helper is inlined, none uses LDS.
 *
 *   the launch   RT_PATH_THREADS: one listed path (or root) per lane, 256 lanes per workgroup
 *   the list     path_slot        the listed slot of a lane, or m
 *   the record   load_path, store_path            the 32 bytes as two 16-byte accesses
 *                load_path_tail, store_path_tail  the second 16 bytes alone (root, id, bounce, flags)
 *   the vertex   ray_direction, view_of           a ray's direction; the view direction of a vertex
 *                store_no_hit                     the vertex of a path that ended
 *
 * The record and the step are rt_path.h's, the per-hit record, the shadow ray and the planes rt_light_record.h's.
 */
#ifndef RT_PATH_KERNEL_H
#define RT_PATH_KERNEL_H

#include <stddef.h>

#include "rt_light_record.h"
#include "rt_path.h"

namespace rt {

#define RT_PATH_THREADS 256u
#define RT_PATH_HIT_WORDS 13u
#define RT_RAY_DIRECTION_WORD 3u /* word of rt_ray.direction */
static_assert(sizeof(rt_hit) == RT_PATH_HIT_WORDS * sizeof(uint32_t), "rt_hit is 13 dwords");
static_assert(offsetof(rt_ray, direction) == RT_RAY_DIRECTION_WORD * sizeof(uint32_t), "rt_ray.direction is word 3");

/* the listed slot of a lane, or m: the lane has nothing to do */
__device__ __forceinline__ uint32_t path_slot(const uint32_t *__restrict__ index, const uint32_t *__restrict__ count, const uint32_t m) {
    const uint64_t lane = (uint64_t)blockIdx.x * RT_PATH_THREADS + threadIdx.x;
    if (lane >= path_listed(index, count, m)) return m;
    const uint32_t j = index != nullptr ? index[lane] : (uint32_t)lane;
    return j < m ? j : m; /* an index beyond the slots names nothing, as in rt_cast_rays_indexed */
}

__device__ __forceinline__ rt_path load_path(const rt_path *__restrict__ paths, const uint64_t j) {
    const uint4 *const record = reinterpret_cast<const uint4 *>(paths + j);
    const uint4 lo = record[0], hi = record[1];
    rt_path p;
    p.beta[0] = __uint_as_float(lo.x);
    p.beta[1] = __uint_as_float(lo.y);
    p.beta[2] = __uint_as_float(lo.z);
    p.pdf = __uint_as_float(lo.w);
    p.root = hi.x;
    p.id = hi.y;
    p.bounce = hi.z;
    p.flags = hi.w;
    return p;
}

__device__ __forceinline__ void store_path(rt_path *__restrict__ paths, const uint64_t j, const rt_path &p) {
    uint4 *const record = reinterpret_cast<uint4 *>(paths + j);
    record[0] = make_uint4(__float_as_uint(p.beta[0]), __float_as_uint(p.beta[1]), __float_as_uint(p.beta[2]), __float_as_uint(p.pdf));
    record[1] = make_uint4(p.root, p.id, p.bounce, p.flags);
}

/* the record's second half, for a kernel that needs no throughput: 16 bytes read, 16 written */
struct PathTail {
    uint32_t root, id, bounce, flags;
};
__device__ __forceinline__ PathTail load_path_tail(const rt_path *__restrict__ paths, const uint64_t j) {
    const uint4 hi = reinterpret_cast<const uint4 *>(paths + j)[1];
    return {hi.x, hi.y, hi.z, hi.w};
}
__device__ __forceinline__ void store_path_tail(rt_path *__restrict__ paths, const uint64_t j, const PathTail &t) {
    reinterpret_cast<uint4 *>(paths + j)[1] = make_uint4(t.root, t.id, t.bounce, t.flags);
}

__device__ __forceinline__ V3 ray_direction(const rt_ray *__restrict__ rays, const uint64_t j) {
    const float *const d = reinterpret_cast<const float *>(rays + j) + RT_RAY_DIRECTION_WORD;
    return v3(d[0], d[1], d[2]);
}

/* what get_shade passes as view_direction: minus the incoming direction; +z for a vertex that is no hit, whose ray is not read */
__device__ __forceinline__ V3 view_of(const bool valid, const rt_ray *__restrict__ incoming, const uint64_t j) {
    V3 view = v3(0.0f, 0.0f, 1.0f);
    if (valid) view = -ray_direction(incoming, j);
    return view;
}

/* "no hit", as the tree loop presets it: the vertex of a path that ended — a later rt_shade_hits spends nothing here, a later advance
 * escapes at once */
__device__ __forceinline__ void store_no_hit(rt_hit *hit) {
    uint32_t *const preset = reinterpret_cast<uint32_t *>(hit);
#pragma unroll
    for (uint32_t k = 0; k < RT_PATH_HIT_WORDS; ++k) preset[k] = k == 0u ? RT_HIT_NONE : 0u;
}

} /* namespace rt */

#endif /* RT_PATH_KERNEL_H */
