/*
 * rt_level_query.hip — what lies between two queries of a level loop (include/rt_amd.h "level loop"): a stable selection with a
 * device-side count, and the element-wise glue and fold of one level of distributed_ray_trace (main.rs:521-614) on the records the
 * scatter and hit queries read and write.
 *
 *   rt::select_count_kernel    one workgroup per tile of flags: how many are set (block total)
 *   rt::select_scatter_kernel  the same tiles again: a workgroup's base is the sum of the totals before it, a wave's the counts of the
 *                              waves before it (LDS), a lane's the ballots' bits below it — ascending indices, no ordering by atomics
 *   rt::level_split_kernel     the level's hits as the operands of get_reflect and get_refract, the others "no hit"
 *   rt::level_join_kernel      the level's next ray, its flag, and the next hits preset to "no hit"
 *   rt::level_close_kernel     the operand of get_shade(&scattered_hit): diffuse / reflection records whose next cast missed
 *   rt::level_fold_kernel      one step of the unwind, dist_unwind_kernel's operations on the caller's arrays
 *   rt::level_finish_kernel    the sample filter (main.rs:1157-1160) and the accumulation (main.rs:1165)
 *
 * Nothing here is new arithmetic: the fold is rt_distributed.hip's dist_unwind_kernel line by line (the same V3 operators, compiled
 * with -ffp-contract=off like every unit: each operation rounds to f32 and nothing is fused), the filter is rtdm::is_normal.  Records
 * are flat words (rt_ray 11, rt_hit 13), moved as dwords, one record per lane, the record number counted in 64 bits.
 */
#include "rt_detmath.h"
#include "rt_vec.h"
#include "rt_kernels.h"

namespace rt {

/* ---- selection ---- */

#define RT_SELECT_THREADS 256u
#define RT_SELECT_STEP (RT_SELECT_THREADS * 4u) /* flags a workgroup takes per step: a dword of four per lane */
#define RT_SELECT_MIN_TILE (4u * RT_SELECT_STEP)

/* flags i .. i+3 as one word, byte k = flag i + k (0 at and beyond n); i is a multiple of 4, so the word is aligned when the array is */
__device__ __forceinline__ uint32_t load_flags4(const unsigned char *__restrict__ flags, uint64_t i, uint64_t n, bool aligned) {
    if (aligned && i + 4u <= n) return *reinterpret_cast<const uint32_t *>(flags + i);
    uint32_t w = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k)
        if (i + k < n) w |= (uint32_t)flags[i + k] << (8u * k);
    return w;
}

__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

/* the sum of one value per thread over a workgroup of RT_SELECT_THREADS, in every thread (integers: the order does not matter) */
__device__ __forceinline__ uint32_t group_sum(uint32_t v, uint32_t *lds) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63u) == 0u) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t sum = 0u;
#pragma unroll
    for (uint32_t w = 0; w < RT_SELECT_THREADS / 64u; ++w) sum += lds[w];
    __syncthreads();
    return sum;
}

__global__ __launch_bounds__(RT_SELECT_THREADS) void select_count_kernel(const unsigned char *__restrict__ flags, const uint64_t n, const uint64_t tile,
                                                                         uint32_t *__restrict__ totals) {
    __shared__ uint32_t lds[RT_SELECT_THREADS / 64u];
    const bool aligned = (reinterpret_cast<uintptr_t>(flags) & 3u) == 0u;
    const uint64_t start = (uint64_t)blockIdx.x * tile, end = start + tile < n ? start + tile : n;
    uint32_t c = 0u;
    for (uint64_t i = start + threadIdx.x * 4u; i < end; i += RT_SELECT_STEP) {
        const uint32_t w = load_flags4(flags, i, n, aligned);
        c += ((w & 0xffu) != 0u) + ((w & 0xff00u) != 0u) + ((w & 0xff0000u) != 0u) + ((w & 0xff000000u) != 0u);
    }
    const uint32_t sum = group_sum(c, lds);
    if (threadIdx.x == 0u) totals[blockIdx.x] = sum;
}

__global__ __launch_bounds__(RT_SELECT_THREADS) void select_scatter_kernel(const unsigned char *__restrict__ flags, const uint64_t n, const uint64_t tile,
                                                                           const uint32_t *__restrict__ totals, uint32_t *__restrict__ index,
                                                                           uint32_t *__restrict__ count) {
    __shared__ uint32_t lds[RT_SELECT_THREADS / 64u];
    __shared__ uint32_t wave_count[2][RT_SELECT_THREADS / 64u];
    const bool aligned = (reinterpret_cast<uintptr_t>(flags) & 3u) == 0u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t start = (uint64_t)blockIdx.x * tile, end = start + tile < n ? start + tile : n;
    uint32_t before = 0u; /* the totals of the workgroups before this one */
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += RT_SELECT_THREADS) before += totals[b];
    uint32_t base = group_sum(before, lds);
    uint32_t parity = 0u;
    for (uint64_t s = start; s < end; s += RT_SELECT_STEP, parity ^= 1u) { /* workgroup-uniform */
        const uint64_t i = s + threadIdx.x * 4u;
        const uint32_t w = i < end ? load_flags4(flags, i, n, aligned) : 0u;
        uint32_t below = 0u, in_wave = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const unsigned long long set = __ballot(((w >> (8u * k)) & 0xffu) != 0u);
            below += lanes_below(set);
            in_wave += (uint32_t)__popcll(set);
        }
        if ((threadIdx.x & 63u) == 0u) wave_count[parity][wave] = in_wave;
        __syncthreads(); /* one barrier per step: the other half of wave_count is not written before every wave has passed this one */
        uint32_t at = base + below;
#pragma unroll
        for (uint32_t v = 0; v < RT_SELECT_THREADS / 64u; ++v) {
            const uint32_t c = wave_count[parity][v];
            if (v < wave) at += c;
            base += c;
        }
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k)
            if (((w >> (8u * k)) & 0xffu) != 0u) index[at++] = (uint32_t)(i + k);
    }
    if (blockIdx.x == gridDim.x - 1u && threadIdx.x == 0u) *count = base;
}

hipError_t launch_select_records(const unsigned char *flags, uint32_t n, uint32_t *index, uint32_t *count, uint32_t *totals, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    /* at most RT_SELECT_MAX_GROUPS tiles of whole steps, so that `totals` has a fixed size and a workgroup sums it in one go */
    uint64_t tile = ((uint64_t)n + RT_SELECT_MAX_GROUPS - 1u) / RT_SELECT_MAX_GROUPS;
    tile = (tile + RT_SELECT_STEP - 1u) / RT_SELECT_STEP * RT_SELECT_STEP;
    if (tile < RT_SELECT_MIN_TILE) tile = RT_SELECT_MIN_TILE;
    const uint32_t groups = (uint32_t)(((uint64_t)n + tile - 1u) / tile);
    hipLaunchKernelGGL(select_count_kernel, dim3(groups), dim3(RT_SELECT_THREADS), 0, stream, flags, (uint64_t)n, tile, totals);
    hipLaunchKernelGGL(select_scatter_kernel, dim3(groups), dim3(RT_SELECT_THREADS), 0, stream, flags, (uint64_t)n, tile, totals, index, count);
    return hipGetLastError();
}

/* ---- the glue of one level ---- */

#define RT_LEVEL_THREADS 256u
#define RT_HIT_WORDS 13u
#define RT_RAY_WORDS 11u

/* alive: the level goes on — spelt as the negation of the reference's `cosine <= 0`, so that NaN goes on as it does there */
__device__ __forceinline__ bool level_alive(uint32_t type, float cosine) { return type != RT_HIT_NONE && !(cosine <= 0.0f); }
__device__ __forceinline__ bool level_dr(uint32_t type, float cosine) { return level_alive(type, cosine) && type <= 1u; }
__device__ __forceinline__ bool level_fr(uint32_t type, float cosine) { return level_alive(type, cosine) && type == 2u; }

/* a record copied word by word, or "no hit" / all-zero words in its place */
__device__ __forceinline__ void copy_hit_or_none(uint32_t *__restrict__ out, const uint32_t *__restrict__ in, bool keep) {
#pragma unroll
    for (uint32_t k = 0; k < RT_HIT_WORDS; ++k) out[k] = keep ? in[k] : (k == 0u ? RT_HIT_NONE : 0u);
}

__global__ __launch_bounds__(RT_LEVEL_THREADS) void level_split_kernel(const rt_hit *__restrict__ hits, const uint32_t *__restrict__ type,
                                                                       const float *__restrict__ cosine, const uint64_t n,
                                                                       rt_hit *__restrict__ hits_reflect, rt_hit *__restrict__ hits_refract) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_LEVEL_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = type[i];
    const float c = cosine[i];
    const bool dr = level_dr(t, c), fr = level_fr(t, c);
    uint32_t w[RT_HIT_WORDS];
    const uint32_t *const in = reinterpret_cast<const uint32_t *>(hits + i);
#pragma unroll
    for (uint32_t k = 0; k < RT_HIT_WORDS; ++k) w[k] = (dr || fr) ? in[k] : 0u;
    copy_hit_or_none(reinterpret_cast<uint32_t *>(hits_reflect + i), w, dr);
    copy_hit_or_none(reinterpret_cast<uint32_t *>(hits_refract + i), w, fr);
}

__global__ __launch_bounds__(RT_LEVEL_THREADS) void level_join_kernel(const uint32_t *__restrict__ type, const float *__restrict__ cosine,
                                                                      const rt_ray *__restrict__ reflected, const uint32_t *__restrict__ refr_kind,
                                                                      const rt_ray *__restrict__ escape, const uint64_t n, rt_ray *__restrict__ next,
                                                                      rt_hit *__restrict__ next_hits, unsigned char *__restrict__ flags) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_LEVEL_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = type[i];
    const float c = cosine[i];
    const bool dr = level_dr(t, c);
    const bool escaped = level_fr(t, c) && refr_kind[i] == 0u; /* Refraction::Escaped */
    const uint32_t *const in = reinterpret_cast<const uint32_t *>(dr ? reflected + i : escape + i);
    uint32_t *const out = reinterpret_cast<uint32_t *>(next + i);
#pragma unroll
    for (uint32_t k = 0; k < RT_RAY_WORDS; ++k) out[k] = (dr || escaped) ? in[k] : 0u;
    uint32_t *const preset = reinterpret_cast<uint32_t *>(next_hits + i); /* "no hit": the indexed cast overwrites the records it names */
#pragma unroll
    for (uint32_t k = 0; k < RT_HIT_WORDS; ++k) preset[k] = k == 0u ? RT_HIT_NONE : 0u;
    flags[i] = (dr || escaped) ? 1 : 0;
}

__global__ __launch_bounds__(RT_LEVEL_THREADS) void level_close_kernel(const rt_hit *__restrict__ hits, const uint32_t *__restrict__ type,
                                                                       const float *__restrict__ cosine, const rt_hit *__restrict__ next_hits,
                                                                       const uint64_t n, rt_hit *__restrict__ hits_missed) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_LEVEL_THREADS + threadIdx.x;
    if (i >= n) return;
    const bool missed = level_dr(type[i], cosine[i]) && next_hits[i].kind > 1u;
    uint32_t w[RT_HIT_WORDS];
    const uint32_t *const in = reinterpret_cast<const uint32_t *>(hits + i);
#pragma unroll
    for (uint32_t k = 0; k < RT_HIT_WORDS; ++k) w[k] = missed ? in[k] : 0u;
    copy_hit_or_none(reinterpret_cast<uint32_t *>(hits_missed + i), w, missed);
}

/* one step of the unwind: dist_unwind_kernel's two expressions (main.rs:566-571, 585-590, 605) and the values of the branches that
 * record no frame there (main.rs:560, 573, 579, 592, 598, 607-611) */
__global__ __launch_bounds__(RT_LEVEL_THREADS) void level_fold_kernel(const uint32_t *__restrict__ type, const float *__restrict__ cosine,
                                                                      const rt_hit *__restrict__ next_hits, const float *__restrict__ factor,
                                                                      const float *__restrict__ shade_next, const float *__restrict__ shade_missed,
                                                                      const uint64_t n, float *__restrict__ value_io) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_LEVEL_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = type[i];
    V3 out = v3(0.0f, 0.0f, 0.0f);
    if (level_alive(t, cosine[i]) && t <= 2u) {
        const bool found = next_hits[i].kind <= 1u;
        if (found) {
            const V3 value = v3(value_io[i * 3u], value_io[i * 3u + 1u], value_io[i * 3u + 2u]);
            const V3 shade = v3(shade_next[i * 3u], shade_next[i * 3u + 1u], shade_next[i * 3u + 2u]);
            const V3 f = v3(factor[i * 3u], factor[i * 3u + 1u], factor[i * 3u + 2u]);
            if (t == 2u) {
                out = (value + shade) * f.x; /* main.rs:605 */
            } else {
                const V3 sc_ = value * f;           /* main.rs:566, 585 */
                out = shade + (sc_ - shade) * 0.5f; /* palette Mix::mix(&s, 0.5), main.rs:571, 590 */
            }
        } else if (t <= 1u) {
            out = v3(shade_missed[i * 3u], shade_missed[i * 3u + 1u], shade_missed[i * 3u + 2u]); /* get_shade(&scattered_hit), main.rs:573, 592 */
        }
    }
    value_io[i * 3u] = out.x;
    value_io[i * 3u + 1u] = out.y;
    value_io[i * 3u + 2u] = out.z;
}

__global__ __launch_bounds__(RT_LEVEL_THREADS) void level_finish_kernel(const float *__restrict__ value, const uint64_t n, float *__restrict__ accum,
                                                                        unsigned char *__restrict__ valid) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_LEVEL_THREADS + threadIdx.x;
    if (i >= n) return;
    const V3 v = v3(value[i * 3u], value[i * 3u + 1u], value[i * 3u + 2u]);
    const bool ok = rtdm::is_normal(v.x) && rtdm::is_normal(v.y) && rtdm::is_normal(v.z);
    if (valid != nullptr) valid[i] = ok ? 1 : 0;
    if (accum != nullptr && ok) {
        const V3 a = v3(accum[i * 3u], accum[i * 3u + 1u], accum[i * 3u + 2u]) + v;
        accum[i * 3u] = a.x;
        accum[i * 3u + 1u] = a.y;
        accum[i * 3u + 2u] = a.z;
    }
}

static inline dim3 level_grid(uint32_t n) { return dim3((unsigned)(((uint64_t)n + RT_LEVEL_THREADS - 1u) / RT_LEVEL_THREADS)); }

hipError_t launch_level_split(const rt_hit *hits, const uint32_t *type, const float *cosine, uint32_t n, rt_hit *hits_reflect, rt_hit *hits_refract,
                              hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(level_split_kernel, level_grid(n), dim3(RT_LEVEL_THREADS), 0, stream, hits, type, cosine, (uint64_t)n, hits_reflect, hits_refract);
    return hipGetLastError();
}

hipError_t launch_level_join(const uint32_t *type, const float *cosine, const rt_ray *reflected, const uint32_t *refr_kind, const rt_ray *escape,
                             uint32_t n, rt_ray *next, rt_hit *next_hits, unsigned char *flags, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(level_join_kernel, level_grid(n), dim3(RT_LEVEL_THREADS), 0, stream, type, cosine, reflected, refr_kind, escape, (uint64_t)n, next,
                       next_hits, flags);
    return hipGetLastError();
}

hipError_t launch_level_close(const rt_hit *hits, const uint32_t *type, const float *cosine, const rt_hit *next_hits, uint32_t n, rt_hit *hits_missed,
                              hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(level_close_kernel, level_grid(n), dim3(RT_LEVEL_THREADS), 0, stream, hits, type, cosine, next_hits, (uint64_t)n, hits_missed);
    return hipGetLastError();
}

hipError_t launch_level_fold(const uint32_t *type, const float *cosine, const rt_hit *next_hits, const float *factor, const float *shade_next,
                             const float *shade_missed, uint32_t n, float *value, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(level_fold_kernel, level_grid(n), dim3(RT_LEVEL_THREADS), 0, stream, type, cosine, next_hits, factor, shade_next, shade_missed,
                       (uint64_t)n, value);
    return hipGetLastError();
}

hipError_t launch_level_finish(const float *value, uint32_t n, float *accum, unsigned char *valid, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(level_finish_kernel, level_grid(n), dim3(RT_LEVEL_THREADS), 0, stream, value, (uint64_t)n, accum, valid);
    return hipGetLastError();
}

} /* namespace rt */
