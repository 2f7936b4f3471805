/*
 * rt_environment_query.hip — a lat-long sky (include/rt_amd.h "environment queries"): the radiance along rays that found nothing, the
 * sampling table of an image built on the device, per (sample, record) a direction drawn from that table with its shadow ray and its
 * radiance over density, and the fold of what the casts and the material probes answered.
 *
 *   rt::environment_lookup_kernel   per record: the texel (or four) its ray's direction names, into the record's or its parent's slot
 *   rt::environment_max_kernel      the table, step 1: one workgroup per row, the largest usable weight into the header (a wave
 *                                   reduction by __shfl_down, the wave maxima through LDS, one atomicMax on the f32's bits per row:
 *                                   usable weights are positive, so their bits order as they do)
 *   rt::environment_rows_kernel     step 2: one workgroup per row, the inclusive scan of the row's quanta in tiles of RT_ENV_ROW_TILE
 *                                   columns — a wave scan by __shfl_up, the wave sums through LDS, a running carry from tile to tile
 *                                   — and the row's sum into M[y]
 *   rt::environment_marginal_kernel step 3: one workgroup, the same scan in u64 over the H row sums, in place; it writes the header's
 *                                   size and total last, so a table reads as "no table" until it is whole
 *   rt::environment_rays_kernel     per (sample, record): the sampled direction, its texel, the flag, radiance / pdf, the shadow ray
 *   rt::environment_fold_kernel     per record, over the samples in order: open flags and the weighted mean added to rgb
 *
 * The arithmetic is rt_environment.h's, shared with librt_host.so; the table is integer sums and one maximum, so the scans' shape does
 * not show in its bits.  One record per lane in the record kernels, the record number counted in 64 bits, arrays sample-major so that
 * one sample's plane is stored coalesced; records move as dwords.  The C entry points of the block are at the end of the file.
 */
#include "rt_api_internal.h"
#include "rt_environment.h"
#include "rt_light_record.h"

namespace rt {

#define RT_ENV_THREADS 256u
#define RT_ENV_ROW_TILE RT_ENV_THREADS /* columns a workgroup scans at a time: one per lane */
#define RT_ENV_WAVES (RT_ENV_THREADS / 64u)

__global__ __launch_bounds__(RT_ENV_THREADS) void environment_lookup_kernel(const EnvLookup a) {
    const uint64_t j = (uint64_t)blockIdx.x * RT_ENV_THREADS + threadIdx.x;
    uint64_t live = a.n;
    if (a.count != nullptr) {
        const uint64_t c = *a.count;
        live = c < a.n ? c : a.n;
    }
    if (j >= live) return; /* dead records write nothing */
    env_lookup_record(a, j);
}

/* an inclusive scan over the 64 lanes of a wave */
template <class T>
__device__ __forceinline__ T env_wave_scan(T v, uint32_t lane) {
#pragma unroll
    for (uint32_t off = 1u; off < 64u; off <<= 1) {
        const T up = __shfl_up(v, off, 64);
        if (lane >= off) v += up;
    }
    return v;
}

/* the inclusive scan of one value per lane over the workgroup; *total: the sum over all lanes.  lds: RT_ENV_WAVES words, free again
 * after the call (it ends on a barrier) */
template <class T>
__device__ __forceinline__ T env_group_scan(T v, T *lds, T *total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const T incl = env_wave_scan(v, lane);
    if (lane == 63u) lds[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (uint32_t k = 0; k < RT_ENV_WAVES; ++k) {
        const T s = lds[k];
        if (k < wave) before += s;
        all += s;
    }
    __syncthreads();
    *total = all;
    return before + incl;
}

__global__ __launch_bounds__(RT_ENV_THREADS) void environment_max_kernel(const rt_environment e, const float l0, const float l1, const float l2,
                                                                         uint32_t *__restrict__ header) {
    __shared__ float lds[RT_ENV_WAVES];
    const uint32_t y = blockIdx.x;
    const float sin_row = env_sin_row(y, e.height);
    float m = 0.0f;
    for (uint32_t x = threadIdx.x; x < e.width; x += RT_ENV_THREADS) {
        bool usable;
        const float w = env_weight(e, x, y, sin_row, l0, l1, l2, &usable);
        if (usable) m = fmaxf(m, w);
    }
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_down(m, off, 64));
    if ((threadIdx.x & 63u) == 0u) lds[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (uint32_t k = 1u; k < RT_ENV_WAVES; ++k) m = fmaxf(m, lds[k]);
        if (m > 0.0f) atomicMax(header + RT_ENV_TABLE_W_MAX, rtdm::f32_bits(m));
    }
}

__global__ __launch_bounds__(RT_ENV_THREADS) void environment_rows_kernel(const rt_environment e, const float l0, const float l1, const float l2,
                                                                          const uint32_t *__restrict__ header, uint64_t *__restrict__ marginal,
                                                                          uint32_t *__restrict__ rows) {
    __shared__ uint32_t lds[RT_ENV_WAVES];
    const uint32_t y = blockIdx.x;
    const float sin_row = env_sin_row(y, e.height);
    const float w_max = rtdm::f32_from_bits(header[RT_ENV_TABLE_W_MAX]);
    uint32_t *const row = rows + (uint64_t)y * e.width;
    uint32_t carry = 0u; /* the sum of the tiles before this one: the same in every lane */
    for (uint32_t base = 0u; base < e.width; base += RT_ENV_ROW_TILE) { /* workgroup-uniform: every lane reaches the barriers */
        const uint32_t x = base + threadIdx.x;
        uint32_t q = 0u;
        if (x < e.width) {
            bool usable;
            const float w = env_weight(e, x, y, sin_row, l0, l1, l2, &usable);
            q = env_quantum(w, usable, w_max);
        }
        uint32_t tile;
        const uint32_t incl = env_group_scan(q, lds, &tile);
        if (x < e.width) row[x] = carry + incl;
        carry += tile;
    }
    if (threadIdx.x == 0u) marginal[y] = carry;
}

__global__ __launch_bounds__(RT_ENV_THREADS) void environment_marginal_kernel(const uint32_t width, const uint32_t height, uint32_t *__restrict__ header,
                                                                              uint64_t *__restrict__ marginal) {
    __shared__ unsigned long long lds[RT_ENV_WAVES];
    unsigned long long carry = 0u;
    for (uint32_t base = 0u; base < height; base += RT_ENV_THREADS) {
        const uint32_t y = base + threadIdx.x;
        const unsigned long long v = y < height ? marginal[y] : 0u;
        unsigned long long tile;
        const unsigned long long incl = env_group_scan(v, lds, &tile);
        if (y < height) marginal[y] = carry + incl;
        carry += tile;
    }
    if (threadIdx.x == 0u) {
        header[RT_ENV_TABLE_TOTAL] = (uint32_t)carry;
        header[RT_ENV_TABLE_TOTAL + 1u] = (uint32_t)(carry >> 32);
        header[RT_ENV_TABLE_WIDTH] = width;
        header[RT_ENV_TABLE_HEIGHT] = height;
    }
}

__global__ __launch_bounds__(RT_LIGHT_THREADS) void environment_rays_kernel(const KernelScene sc, const rt_environment e, const void *__restrict__ table,
                                                                            const rt_hit *__restrict__ hits, const uint64_t n,
                                                                            const uint32_t *__restrict__ ids, const uint32_t spp, const uint32_t pattern,
                                                                            const uint32_t strata, const uint32_t seed, const uint32_t normal_kind,
                                                                            rt_ray *__restrict__ shadow_rays, unsigned char *__restrict__ asks,
                                                                            float *__restrict__ dirs, float *__restrict__ radiance,
                                                                            uint32_t *__restrict__ texel) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_LIGHT_THREADS + threadIdx.x;
    if (i >= n) return;
    const LightRecord r = light_record(sc, hits, i);
    const V3 normal = sampling_normal(r, normal_kind);
    const uint32_t id = record_id(ids, i);
    const uint32_t seed_e = environment_seed(seed);
    const EnvTable t = env_table_view(e, table);
    const bool drawn = r.valid && t.total > 0u;
    for (uint32_t s = 0; s < spp; ++s) { /* wave-uniform */
        const uint64_t k = (uint64_t)s * n + i;
        V3 dir = v3(0.0f, 0.0f, 0.0f), l = v3(0.0f, 0.0f, 0.0f);
        uint32_t at = 0u;
        bool need = false;
        if (drawn) {
            const EnvSample p = env_sample_of(e, t, pattern, strata, id, seed_e, s);
            dir = p.dir;
            at = p.y * e.width + p.x;
            need = p.ok && hemisphere_asks(dir, normal);
            if (need) l = env_sample_radiance(e, p);
        }
        store_v3(dirs, k, dir);
        store_v3(radiance, k, l);
        if (texel != nullptr) texel[k] = at;
        asks[k] = need ? 1 : 0;
        store_shadow_ray(shadow_rays + k, r, dir, need);
    }
}

__global__ __launch_bounds__(RT_LIGHT_THREADS) void environment_fold_kernel(const KernelScene sc, const rt_hit *__restrict__ hits, const EnvFold f) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_LIGHT_THREADS + threadIdx.x;
    if (i >= f.n) return;
    bool valid;
    const float shiness = fold_shiness(sc, hits, i, &valid);
    env_fold_record(f, i, valid, shiness);
}

} /* namespace rt */

/* ---- the C entry points (include/rt_amd.h "environment queries") ---- */

/* the descriptor's checks under the entry point's name */
static int environment_ok(const char *who, const rt_environment *env) { return check_descriptor(who, env, rt::environment_limits); }

/* the checks before any device work are hit_sample_args' (rt_api_internal.h): the hemisphere queries' with the descriptor after the
 * scene.  rt_environment_lookup takes no scene and no samples, rt_environment_fold no descriptor */
extern "C" {

int rt_environment_lookup(const rt_environment *env, const rt_ray *d_rays, size_t n, const uint32_t *d_count, const rt_hit *d_hits,
                          const uint32_t *d_parent, float *d_out, size_t n_out, void *hip_stream) {
    bool done;
    const int rc = hit_sample_args("rt_environment_lookup", nullptr,
                                   HitSampleArgs(n, d_rays && d_out, "ray or output").no_scene().described([env] { return environment_ok("rt_environment_lookup", env); }),
                                   &done);
    if (rc != RT_OK || done) return rc;
    const rt::EnvLookup a = {*env, reinterpret_cast<const uint32_t *>(d_rays), (uint64_t)n, d_count, reinterpret_cast<const uint32_t *>(d_hits), d_parent,
                             d_out, (uint64_t)n_out};
    hipLaunchKernelGGL(rt::environment_lookup_kernel, grid_of(n, RT_ENV_THREADS), dim3(RT_ENV_THREADS), 0, static_cast<hipStream_t>(hip_stream), a);
    return launched("rt_environment_lookup");
}

size_t rt_environment_table_bytes(uint32_t width, uint32_t height) {
    static const float no_texels = 0.0f; /* the limits want a pointer; nothing reads it */
    const rt_environment probe = {&no_texels, width, height, 0.0f, 1.0f, RT_ENV_NEAREST};
    bool unsupported;
    return rt::environment_limits(&probe, &unsupported) != nullptr ? 0u : (size_t)rt::env_table_bytes(width, height);
}

int rt_environment_table(const rt_environment *env, void *d_table, void *hip_stream) {
    const char *const who = "rt_environment_table";
    int rc = environment_ok(who, env);
    if (rc == RT_OK) rc = check_pointers(who, d_table != nullptr, "table");
    if (rc == RT_OK && (reinterpret_cast<uintptr_t>(d_table) & 7u) != 0u) rc = fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": the table is not 8-byte aligned");
    if (rc != RT_OK) return rc;
    float luma[3];
    rt::luma_row(luma);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    uint32_t *const header = static_cast<uint32_t *>(d_table);
    uint64_t *const marginal = rt::env_table_marginal(d_table);
    uint32_t *const rows = rt::env_table_rows(d_table, env->height);
    RT_HIP(hipMemsetAsync(d_table, 0, RT_ENV_TABLE_HEADER_BYTES, stream)); /* "no table", and the 0 the maximum starts from */
    hipLaunchKernelGGL(rt::environment_max_kernel, dim3(env->height), dim3(RT_ENV_THREADS), 0, stream, *env, luma[0], luma[1], luma[2], header);
    hipLaunchKernelGGL(rt::environment_rows_kernel, dim3(env->height), dim3(RT_ENV_THREADS), 0, stream, *env, luma[0], luma[1], luma[2], header, marginal, rows);
    hipLaunchKernelGGL(rt::environment_marginal_kernel, dim3(1), dim3(RT_ENV_THREADS), 0, stream, env->width, env->height, header, marginal);
    return launched(who);
}

int rt_environment_rays(const rt_scene *scene, const rt_environment *env, const void *d_table, const rt_hit *d_hits, size_t n, const uint32_t *d_ids,
                        uint32_t spp, uint32_t pattern, uint32_t seed, uint32_t normal_kind, rt_ray *d_rays, unsigned char *d_asks, float *d_dirs,
                        float *d_radiance, uint32_t *d_texel, void *hip_stream) {
    bool done;
    const int rc = hit_sample_args("rt_environment_rays", scene,
                                   HitSampleArgs(n, d_table && d_hits && d_rays && d_asks && d_dirs && d_radiance, "table, hit, ray, flag, direction or radiance")
                                       .described([env] { return environment_ok("rt_environment_rays", env); }).samples(spp)
                                       .limits(rt::hemisphere_limits(spp, true, pattern, normal_kind)), &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::environment_rays_kernel, grid_of(n, RT_LIGHT_THREADS), dim3(RT_LIGHT_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks, *env,
                       d_table, d_hits, (uint64_t)n, d_ids, spp, pattern, rt::film_strata(spp), seed, normal_kind, d_rays, d_asks, d_dirs, d_radiance, d_texel);
    return launched("rt_environment_rays");
}

int rt_environment_fold(const rt_scene *scene, const rt_hit *d_hits, size_t n, uint32_t spp, const unsigned char *d_asks, const rt_hit *d_shadow_hits,
                        const float *d_radiance, const float *d_diffuse, const float *d_specular, unsigned char *d_open, float *d_rgb, void *hip_stream) {
    bool done;
    const int rc = hit_sample_args("rt_environment_fold", scene,
                                   HitSampleArgs(n, d_hits && d_asks && d_radiance && d_diffuse && d_specular && d_rgb, "hit, flag, radiance, diffuse, specular or rgb")
                                       .samples(spp).limits(rt::hemisphere_limits(spp, false, 0u, 0u)), &done);
    if (rc != RT_OK || done) return rc;
    const rt::EnvFold f = {(uint64_t)n, spp, d_asks, reinterpret_cast<const uint32_t *>(d_shadow_hits), d_radiance, d_diffuse, d_specular, d_open, d_rgb};
    hipLaunchKernelGGL(rt::environment_fold_kernel, grid_of(n, RT_LIGHT_THREADS), dim3(RT_LIGHT_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks, d_hits, f);
    return launched("rt_environment_fold");
}

} /* extern "C" */
