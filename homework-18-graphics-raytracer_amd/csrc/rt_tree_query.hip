/*
 * rt_tree_query.hip — what lies between two queries when ray_trace (main.rs:466-519) runs one level at a time (include/rt_amd.h "tree
 * loop"): the recursion is a tree with up to two children per node, so next to the hit queries and the level loop's selection and
 * indexed cast it needs the weights and threshold gates of main.rs:480-504 as a query, the compaction of 2n child candidates into the
 * next level with a link to the parent's slot, and a fold that hands each child's value to that slot.
 *
 *   rt::tree_gate_kernel    the entry check of main.rs:469 on the roots; their hits preset to "no hit"
 *   rt::tree_split_kernel   a level's hits as the operands of get_shade, get_reflect and get_refract, gated by contribution * weight
 *                           against the threshold; the weights (sc, rc, fc) and opaque_decay per record
 *   rt::tree_spawn_kernel   two candidate flags per record (reflection child, refraction child) and the record's child values zeroed
 *   rt::tree_gather_kernel  the selected candidates as the next level: ray, contribution (one f32 multiply, TraceState::nested) and
 *                           parent slot; the next level's count; what did not fit counted into the overflow word
 *   rt::tree_fold_kernel    main.rs:516-518 on one level, written into the parent's child-value slot (one writer per slot, no atomics)
 *
 * Nothing here is new arithmetic: the weights are the three products rt_kernels.hip and rt_pwf.hip form, the fold is rt_pwf.hip's
 * fold_node with the same V3 operators in the same association, the decay is rtdm::powf.  The unit is compiled with -ffp-contract=off
 * like every other: each operation rounds to f32 and nothing is fused.  Records are flat words (rt_ray 11, rt_hit 13) moved as dwords,
 * one record per lane, the record number counted in 64 bits.  The C entry points of the block are at the end of the file.
 */
#include "rt_api_internal.h"
#include "rt_detmath.h"

namespace rt {

#define RT_TREE_THREADS 256u
#define RT_TREE_HIT_WORDS 13u
#define RT_TREE_RAY_WORDS 11u
#define RT_TREE_THRESHOLD 0.001f /* main.rs:467 */
#define RT_TREE_NO_PARENT 0xffffffffu

/* the number of live records: *count clipped to the capacity, or the capacity */
__device__ __forceinline__ uint64_t tree_live_count(const uint32_t *__restrict__ count, uint64_t n) {
    if (count == nullptr) return n;
    const uint64_t c = *count;
    return c < n ? c : n;
}

__device__ __forceinline__ void tree_store_hit(uint32_t *__restrict__ out, const uint32_t *w, bool keep) {
#pragma unroll
    for (uint32_t k = 0; k < RT_TREE_HIT_WORDS; ++k) out[k] = keep ? w[k] : (k == 0u ? RT_HIT_NONE : 0u);
}

/* main.rs:469: `contribution < THRESHOLD` returns black — spelt as its negation, so that a NaN contribution goes on as it does there */
__global__ __launch_bounds__(RT_TREE_THREADS) void tree_gate_kernel(const float *__restrict__ contribution, const uint64_t n,
                                                                    const uint32_t *__restrict__ count, unsigned char *__restrict__ flags,
                                                                    rt_hit *__restrict__ hits) {
    const uint64_t j = (uint64_t)blockIdx.x * RT_TREE_THREADS + threadIdx.x;
    if (j >= n) return;
    const bool pass = j < tree_live_count(count, n) && !(contribution[j] < RT_TREE_THRESHOLD);
    flags[j] = pass ? 1 : 0;
    uint32_t *const preset = reinterpret_cast<uint32_t *>(hits + j); /* "no hit": the indexed cast overwrites the records it names */
#pragma unroll
    for (uint32_t k = 0; k < RT_TREE_HIT_WORDS; ++k) preset[k] = k == 0u ? RT_HIT_NONE : 0u;
}

/* main.rs:478-504 up to the three calls: material.approx(hit.at) copies shiness, transparency and opaque_decay from the material as
 * they are (materials.rs:21-31; only the diffuse colour and the normal depend on uv), so they are read there */
__global__ __launch_bounds__(RT_TREE_THREADS) void tree_split_kernel(const rt_material *__restrict__ materials, const uint32_t n_materials,
                                                                     const rt_hit *__restrict__ hits, const float *__restrict__ contribution,
                                                                     const uint64_t n, const uint32_t *__restrict__ count, const int32_t depth_left,
                                                                     rt_hit *__restrict__ hits_shade, rt_hit *__restrict__ hits_reflect,
                                                                     rt_hit *__restrict__ hits_refract, float *__restrict__ weights) {
    const uint64_t j = (uint64_t)blockIdx.x * RT_TREE_THREADS + threadIdx.x;
    if (j >= n) return;
    const uint32_t *const in = reinterpret_cast<const uint32_t *>(hits + j);
    const uint32_t kind = in[0], obj = in[2];
    const bool live = j < tree_live_count(count, n) && kind <= 1u && obj < n_materials;
    uint32_t w[RT_TREE_HIT_WORDS];
#pragma unroll
    for (uint32_t k = 0; k < RT_TREE_HIT_WORDS; ++k) w[k] = live ? in[k] : 0u;
    float sc = 0.0f, rc = 0.0f, fc = 0.0f, decay = 0.0f;
    bool want_shade = false, want_reflect = false, want_refract = false;
    if (live) {
        const rt_material &rm = materials[obj];
        const float c = contribution[j];
        sc = (1.0f - rm.shiness) * (1.0f - rm.transparency); /* main.rs:480 */
        rc = rm.shiness * (1.0f - rm.transparency);          /* main.rs:493 */
        fc = rm.transparency;                                /* main.rs:502 */
        decay = rm.opaque_decay;
        want_shade = c * sc >= RT_TREE_THRESHOLD;                      /* main.rs:481-482 */
        want_reflect = depth_left > 0 && c * rc >= RT_TREE_THRESHOLD;  /* main.rs:488, 494-495 */
        want_refract = depth_left > 0 && c * fc > RT_TREE_THRESHOLD;   /* main.rs:503-504: strict */
    }
    tree_store_hit(reinterpret_cast<uint32_t *>(hits_shade + j), w, want_shade);
    tree_store_hit(reinterpret_cast<uint32_t *>(hits_reflect + j), w, want_reflect);
    tree_store_hit(reinterpret_cast<uint32_t *>(hits_refract + j), w, want_refract);
    weights[j * 4u] = sc;
    weights[j * 4u + 1u] = rc;
    weights[j * 4u + 2u] = fc;
    weights[j * 4u + 3u] = decay;
}

__global__ __launch_bounds__(RT_TREE_THREADS) void tree_spawn_kernel(const rt_hit *__restrict__ hits_reflect, const uint32_t *__restrict__ refr_kind,
                                                                     const uint64_t n, unsigned char *__restrict__ flags,
                                                                     float *__restrict__ child_values) {
    const uint64_t j = (uint64_t)blockIdx.x * RT_TREE_THREADS + threadIdx.x;
    if (j >= n) return;
    flags[2u * j] = hits_reflect[j].kind <= 1u ? 1 : 0; /* the reflection child: ray_trace(&reflection_state, &reflected_ray), main.rs:497 */
    flags[2u * j + 1u] = refr_kind[j] == 0u ? 1 : 0;    /* the refraction child: Refraction::Escaped, main.rs:506-507 */
#pragma unroll
    for (uint32_t k = 0; k < 6u; ++k) child_values[j * 6u + k] = 0.0f; /* black until the child's fold writes its slot */
}

__global__ __launch_bounds__(RT_TREE_THREADS) void tree_gather_kernel(const uint32_t *__restrict__ index, const uint32_t *__restrict__ count,
                                                                      const uint64_t max_count, const rt_ray *__restrict__ reflected,
                                                                      const rt_ray *__restrict__ escape, const float *__restrict__ contribution,
                                                                      const float *__restrict__ weights, const uint64_t n,
                                                                      rt_ray *__restrict__ child_rays, float *__restrict__ child_contribution,
                                                                      uint32_t *__restrict__ child_parent, uint32_t *__restrict__ child_count,
                                                                      uint32_t *__restrict__ overflow) {
    const uint64_t j = (uint64_t)blockIdx.x * RT_TREE_THREADS + threadIdx.x;
    uint64_t found = *count; /* candidates selected: never more than there are */
    if (found > 2u * n) found = 2u * n;
    const uint64_t kept = found < max_count ? found : max_count;
    if (j == 0u) {
        *child_count = (uint32_t)kept;
        if (found > kept) atomicAdd(overflow, (uint32_t)(found - kept)); /* their parents see a black child */
    }
    if (j >= kept) return;
    const uint32_t c = index[j];
    uint32_t *const out = reinterpret_cast<uint32_t *>(child_rays + j);
    if ((uint64_t)c >= 2u * n) { /* not a candidate of this level: a record that casts nothing useful and folds into no slot */
#pragma unroll
        for (uint32_t k = 0; k < RT_TREE_RAY_WORDS; ++k) out[k] = 0u;
        child_contribution[j] = 0.0f;
        child_parent[j] = RT_TREE_NO_PARENT;
        return;
    }
    const uint64_t p = c >> 1;
    const bool refraction = (c & 1u) != 0u;
    const uint32_t *const in = reinterpret_cast<const uint32_t *>(refraction ? escape + p : reflected + p);
#pragma unroll
    for (uint32_t k = 0; k < RT_TREE_RAY_WORDS; ++k) out[k] = in[k];
    child_contribution[j] = contribution[p] * weights[p * 4u + (refraction ? 2u : 1u)]; /* TraceState::nested, main.rs:677 */
    child_parent[j] = c;
}

/* main.rs:516-518 in rt_pwf.hip's association (fold_node): (shade * sc + reflection * rc) + refraction * fc */
__global__ __launch_bounds__(RT_TREE_THREADS) void tree_fold_kernel(const rt_hit *__restrict__ hits, const uint32_t *__restrict__ count, const uint64_t n,
                                                                    const int32_t depth_left, const float *__restrict__ shade,
                                                                    const float *__restrict__ weights, const uint32_t *__restrict__ refr_kind,
                                                                    const float *__restrict__ travel, const float *__restrict__ child_values,
                                                                    const uint32_t *__restrict__ parent, float *__restrict__ out, const uint64_t n_out) {
    const uint64_t j = (uint64_t)blockIdx.x * RT_TREE_THREADS + threadIdx.x;
    if (j >= tree_live_count(count, n)) return; /* dead records write nothing */
    const uint64_t slot = parent != nullptr ? (uint64_t)parent[j] : j;
    if (slot >= n_out) return;
    V3 value = v3(0.0f, 0.0f, 0.0f); /* a miss or a gated root: main.rs:470, 475 */
    if (hits[j].kind <= 1u) {
        const V3 sh = v3(shade[j * 3u], shade[j * 3u + 1u], shade[j * 3u + 2u]);
        if (depth_left <= 0) {
            value = sh; /* main.rs:488-490: the shade, not weighted */
        } else {
            const float sc = weights[j * 4u], rc = weights[j * 4u + 1u], fc = weights[j * 4u + 2u];
            const V3 reflection = v3(child_values[j * 6u], child_values[j * 6u + 1u], child_values[j * 6u + 2u]);
            V3 refraction = v3(0.0f, 0.0f, 0.0f);
            if (refr_kind[j] == 0u) { /* Escaped, main.rs:506-509 */
                const float decay = rtdm::powf(weights[j * 4u + 3u], travel[j]);
                refraction = v3(child_values[j * 6u + 3u], child_values[j * 6u + 4u], child_values[j * 6u + 5u]) * decay;
            }
            value = (sh * sc + reflection * rc) + refraction * fc;
        }
    }
    out[slot * 3u] = value.x;
    out[slot * 3u + 1u] = value.y;
    out[slot * 3u + 2u] = value.z;
}

} /* namespace rt */

/* ---- the C entry points (include/rt_amd.h "tree loop") ---- */

/* a level of 2^32 (2^31 where a record has two children) records or more is refused: the caller splits it */
static const CountLimit TREE_2_32 = {32u, "records", "split the level"}, TREE_2_31 = {31u, "records", "split the level"};

extern "C" {

int rt_tree_gate(const float *d_contribution, size_t n, const uint32_t *d_count, unsigned char *d_flags, rt_hit *d_hits, void *hip_stream) {
    bool done;
    const int rc = query_args("rt_tree_gate", n, TREE_2_32, false, nullptr, d_contribution && d_flags && d_hits, "contribution, flag or hit", &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::tree_gate_kernel, grid_of(n, RT_TREE_THREADS), dim3(RT_TREE_THREADS), 0, static_cast<hipStream_t>(hip_stream), d_contribution, (uint64_t)n,
                       d_count, d_flags, d_hits);
    return launched("rt_tree_gate");
}

int rt_tree_split(const rt_scene *scene, const rt_hit *d_hits, const float *d_contribution, size_t n, const uint32_t *d_count, int32_t depth_left,
                  rt_hit *d_hits_shade, rt_hit *d_hits_reflect, rt_hit *d_hits_refract, float *d_weights, void *hip_stream) {
    bool done;
    const int rc = query_args("rt_tree_split", n, TREE_2_32, true, scene, d_hits && d_contribution && d_hits_shade && d_hits_reflect && d_hits_refract && d_weights,
                             "hit, contribution, output-hit or weight", &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::tree_split_kernel, grid_of(n, RT_TREE_THREADS), dim3(RT_TREE_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks.materials,
                       scene->ks.n_materials, d_hits, d_contribution, (uint64_t)n, d_count, depth_left, d_hits_shade, d_hits_reflect, d_hits_refract,
                       d_weights);
    return launched("rt_tree_split");
}

int rt_tree_spawn(const rt_hit *d_hits_reflect, const uint32_t *d_refr_kind, size_t n, unsigned char *d_flags, float *d_child_values, void *hip_stream) {
    bool done;
    const int rc = query_args("rt_tree_spawn", n, TREE_2_31, false, nullptr, d_hits_reflect && d_refr_kind && d_flags && d_child_values,
                             "reflect-hit, refraction-kind, flag or child-value", &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::tree_spawn_kernel, grid_of(n, RT_TREE_THREADS), dim3(RT_TREE_THREADS), 0, static_cast<hipStream_t>(hip_stream), d_hits_reflect, d_refr_kind,
                       (uint64_t)n, d_flags, d_child_values);
    return launched("rt_tree_spawn");
}

int rt_tree_gather(const uint32_t *d_index, const uint32_t *d_count, size_t max_count, const rt_ray *d_reflected, const rt_ray *d_escape,
                   const float *d_contribution, const float *d_weights, size_t n, rt_ray *d_child_rays, float *d_child_contribution,
                   uint32_t *d_child_parent, uint32_t *d_child_count, uint32_t *d_overflow, void *hip_stream) {
    if ((uint64_t)max_count >= (1ull << 32))
        return fail(RT_ERR_UNSUPPORTED, "rt_tree_gather: a capacity of 2^32 records or more (checked first; split the level)");
    bool done;
    const int rc = query_args("rt_tree_gather", n, TREE_2_31, false, nullptr,
                             d_index && d_count && d_reflected && d_escape && d_contribution && d_weights && d_child_count && d_overflow &&
                                 (max_count == 0 || (d_child_rays && d_child_contribution && d_child_parent)),
                             "index, count, ray, contribution, weight, child or overflow", &done);
    if (rc != RT_OK || done) return rc;
    /* the grid covers what can be kept; with no room at all one workgroup still writes the count and the overflow */
    const uint64_t most = (uint64_t)max_count < 2u * (uint64_t)n ? (uint64_t)max_count : 2u * (uint64_t)n;
    hipLaunchKernelGGL(rt::tree_gather_kernel, grid_of(most > 0u ? most : 1u, RT_TREE_THREADS), dim3(RT_TREE_THREADS), 0, static_cast<hipStream_t>(hip_stream), d_index,
                       d_count, (uint64_t)max_count, d_reflected, d_escape, d_contribution, d_weights, (uint64_t)n, d_child_rays, d_child_contribution,
                       d_child_parent, d_child_count, d_overflow);
    return launched("rt_tree_gather");
}

int rt_tree_fold(const rt_hit *d_hits, const uint32_t *d_count, size_t n, int32_t depth_left, const float *d_shade, const float *d_weights,
                 const uint32_t *d_refr_kind, const float *d_travel, const float *d_child_values, const uint32_t *d_parent, float *d_out, size_t n_out,
                 void *hip_stream) {
    bool done;
    const bool below = depth_left <= 0 || (d_weights && d_refr_kind && d_travel && d_child_values);
    const int rc = query_args("rt_tree_fold", n, TREE_2_32, false, nullptr, d_hits && d_shade && d_out && below, "hit, shade, weight, refraction, child-value or output",
                             &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::tree_fold_kernel, grid_of(n, RT_TREE_THREADS), dim3(RT_TREE_THREADS), 0, static_cast<hipStream_t>(hip_stream), d_hits, d_count, (uint64_t)n,
                       depth_left, d_shade, d_weights, d_refr_kind, d_travel, d_child_values, d_parent, d_out, (uint64_t)n_out);
    return launched("rt_tree_fold");
}

} /* extern "C" */
