/*
 * rt_adaptive_query.hip — the adaptive sampling queries (include/rt_amd.h "adaptive sampling queries"): a sample budget per pixel from a
 * mean and a variance plane, the ragged pixel-major list of the samples that budget asks for, and the film queries on such a list:
 * sample positions, camera rays and the filtered splat; kernels and entry points in one unit.
 *
 *   rt::each_kernel<SampleBudget>   one thread per pixel: rt_adaptive.h's sample_budget_pixel (rt_image_kernel.h has the element loop)
 *   rt::sample_totals_kernel        rt_sample_list, 1 of 3: a workgroup takes 256-pixel steps grid-stride and writes the sum of each step's
 *                                   clamped counts (a wave reduction by __shfl_down, four wave sums through LDS) to totals[step]
 *   rt::sample_scan_kernel          2 of 3: ONE workgroup turns totals[0 .. steps) into their exclusive sums in place, 256 entries at a time
 *                                   with a carried base (coalesced), and writes totals[steps] = S_n, start_n and d_total
 *   rt::sample_expand_kernel        3 of 3: the same steps again.  A workgroup scans its 256 counts (an inclusive scan per wave by
 *                                   __shfl_up, the wave sums through LDS) into 257 LDS prefix values, writes start_i and first_i, and its
 *                                   threads then walk the step's OUTPUT range [base, base + block_total) with stride 256: record base + k
 *                                   belongs to the pixel p with prefix[p] <= k < prefix[p + 1], found by a binary search of eight LDS
 *                                   reads.  So the stores to d_pixel and d_sample are coalesced whatever the counts are, and a pixel with
 *                                   64 samples costs its neighbours' lanes nothing.  block_total <= 256 * 64 = 16 384.
 *   rt::offsets_listed_kernel       one thread per record of [0, capacity), grid-stride: rt_adaptive.h's listed_offsets_record
 *   rt::camera_rays_listed_kernel   one thread per record: rt_primary_ray.h's primary_ray_offset, or the all-zero ray
 *   the splat                       rt_film_splat_kernel.h's two forms, the kernels of rt_film_splat, instantiated for rt_adaptive.h's
 *                                   ListedLayout (record lo_q + s for s < count_q); that header says what a ragged layout adds to them
 *
 * Everything the list kernels compute is u32 arithmetic on sums below 2^32 (n * RT_SAMPLE_MAX < 2^32 is checked by the entry point), so
 * the result cannot depend on the launch geometry: there is no atomic and no order to decide.  A record index is clamped into
 * [0, capacity) before anything is read through it (listed_range).  Every loop that holds a barrier is workgroup-uniform.
 */
#include "rt_image_kernel.h"
#include "rt_adaptive.h"
#include "rt_film_splat_kernel.h"
#include "rt_primary_ray.h"

namespace rt {

#define RT_ADAPTIVE_WAVES (RT_IMAGE_THREADS / 64u)
static_assert(RT_IMAGE_THREADS == RT_SAMPLE_LIST_STEP, "a workgroup takes one step of the list per pass");

/* ---- the list ---- */

/* the sum of one value per thread over the workgroup, in every thread; lds: RT_ADAPTIVE_WAVES words */
__device__ __forceinline__ uint32_t adaptive_group_sum(uint32_t v, uint32_t *lds) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads(); /* the previous use of lds is over */
    if ((threadIdx.x & 63u) == 0u) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t sum = 0u;
#pragma unroll
    for (uint32_t w = 0; w < RT_ADAPTIVE_WAVES; ++w) sum += lds[w];
    return sum;
}

/* the inclusive sum of one value per thread over the workgroup, in thread order; *total: the sum of all; lds: RT_ADAPTIVE_WAVES words */
__device__ __forceinline__ uint32_t adaptive_group_scan(uint32_t v, uint32_t *lds, uint32_t *total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(v, off, 64);
        if (lane >= (uint32_t)off) v += up;
    }
    __syncthreads(); /* the previous use of lds is over */
    if (lane == 63u) lds[wave] = v;
    __syncthreads();
    uint32_t before = 0u, all = 0u;
#pragma unroll
    for (uint32_t w = 0; w < RT_ADAPTIVE_WAVES; ++w) {
        const uint32_t c = lds[w];
        if (w < wave) before += c;
        all += c;
    }
    *total = all;
    return v + before;
}

__global__ __launch_bounds__(RT_IMAGE_THREADS) void sample_totals_kernel(const uint32_t *__restrict__ counts, const uint64_t n, const uint64_t steps,
                                                                            uint32_t *__restrict__ totals) {
    __shared__ uint32_t lds[RT_ADAPTIVE_WAVES];
    for (uint64_t step = blockIdx.x; step < steps; step += gridDim.x) { /* workgroup-uniform */
        const uint64_t i = step * RT_IMAGE_THREADS + threadIdx.x;
        const uint32_t sum = adaptive_group_sum(i < n ? sample_count_clamped(counts[i]) : 0u, lds);
        if (threadIdx.x == 0u) totals[step] = sum;
    }
}

__global__ __launch_bounds__(RT_IMAGE_THREADS) void sample_scan_kernel(uint32_t *__restrict__ totals, const uint64_t steps, const uint64_t n,
                                                                          const uint64_t capacity, uint32_t *__restrict__ start, uint32_t *__restrict__ total) {
    __shared__ uint32_t lds[RT_ADAPTIVE_WAVES];
    uint32_t base = 0u; /* the sum of the entries before this round's: below 2^32, as S_n is */
    for (uint64_t first = 0u; first < steps; first += RT_IMAGE_THREADS) { /* workgroup-uniform */
        const uint64_t k = first + threadIdx.x;
        const uint32_t v = k < steps ? totals[k] : 0u;
        uint32_t all;
        const uint32_t inclusive = adaptive_group_scan(v, lds, &all);
        if (k < steps) totals[k] = base + (inclusive - v);
        base += all;
    }
    if (threadIdx.x == 0u) {
        const uint32_t listed = (uint64_t)base < capacity ? base : (uint32_t)capacity;
        totals[steps] = base;
        start[n] = listed;
        total[0] = listed;
        total[1] = base;
    }
}

__global__ __launch_bounds__(RT_IMAGE_THREADS) void sample_expand_kernel(const uint32_t *__restrict__ counts, const uint64_t n, const uint64_t steps,
                                                                            const uint32_t *__restrict__ totals, const uint64_t capacity,
                                                                            uint32_t *__restrict__ first, uint32_t *__restrict__ start,
                                                                            uint32_t *__restrict__ pixel, uint32_t *__restrict__ sample) {
    __shared__ uint32_t lds[RT_ADAPTIVE_WAVES];
    __shared__ uint32_t l_prefix[RT_IMAGE_THREADS + 1u];
    __shared__ uint32_t l_first[RT_IMAGE_THREADS];
    for (uint64_t step = blockIdx.x; step < steps; step += gridDim.x) { /* workgroup-uniform */
        const uint64_t i = step * RT_IMAGE_THREADS + threadIdx.x;
        const uint32_t c = i < n ? sample_count_clamped(counts[i]) : 0u;
        uint32_t block_total;
        const uint32_t inclusive = adaptive_group_scan(c, lds, &block_total); /* its first barrier: the previous step's LDS reads are done */
        const uint64_t base = totals[step];
        const uint32_t f = (first != nullptr && i < n) ? first[i] : 0u;
        l_prefix[threadIdx.x + 1u] = inclusive;
        if (threadIdx.x == 0u) l_prefix[0] = 0u;
        l_first[threadIdx.x] = f;
        if (i < n) {
            const uint64_t s0 = base + (inclusive - c), s1 = base + inclusive;
            const uint32_t lo = (uint32_t)(s0 < capacity ? s0 : capacity), hi = (uint32_t)(s1 < capacity ? s1 : capacity);
            start[i] = lo;
            if (first != nullptr) first[i] = f + (hi - lo);
        }
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < block_total; k += RT_IMAGE_THREADS) { /* no barrier inside */
            const uint64_t j = base + k;
            if (j >= capacity) break; /* j grows with k: nothing of this thread's lies below capacity any more */
            uint32_t lo = 0u, hi = RT_IMAGE_THREADS; /* l_prefix[lo] <= k < l_prefix[hi] throughout */
            while (hi - lo > 1u) {
                const uint32_t mid = (lo + hi) >> 1;
                if (l_prefix[mid] <= k) lo = mid;
                else hi = mid;
            }
            pixel[j] = (uint32_t)(step * RT_IMAGE_THREADS) + lo;
            sample[j] = l_first[lo] + (k - l_prefix[lo]);
        }
    }
}

/* n == 0: start_0 and both totals, nothing else */
__global__ void sample_list_empty_kernel(uint32_t *__restrict__ start, uint32_t *__restrict__ total) {
    if (threadIdx.x == 0u && blockIdx.x == 0u) start[0] = 0u, total[0] = 0u, total[1] = 0u;
}

/* ---- positions and rays of a list ---- */

/* These two keep their own grid-stride loops: the list's length is read once per thread, ahead of the loop.  As Ops of each_kernel it
 * is read per element, and the pass that runs both (adaptive.render_pass) then measured above the parent's range. */
__global__ __launch_bounds__(RT_IMAGE_THREADS) void offsets_listed_kernel(const ListedOffsets o) {
    const uint64_t listed = listed_count(o.total, o.capacity), stride = (uint64_t)gridDim.x * RT_IMAGE_THREADS;
    for (uint64_t j = (uint64_t)blockIdx.x * RT_IMAGE_THREADS + threadIdx.x; j < o.capacity; j += stride) listed_offsets_record(o, j, listed);
}

__global__ __launch_bounds__(RT_IMAGE_THREADS) void camera_rays_listed_kernel(const KernelFrame fr, const float *__restrict__ offsets,
                                                                              const uint32_t *__restrict__ pixel, const uint32_t *__restrict__ total,
                                                                              const uint64_t capacity, rt_ray *__restrict__ rays) {
    const uint64_t listed = listed_count(total, capacity), stride = (uint64_t)gridDim.x * RT_IMAGE_THREADS;
    const uint64_t n_pixels = (uint64_t)fr.rows * fr.cols;
    for (uint64_t j = (uint64_t)blockIdx.x * RT_IMAGE_THREADS + threadIdx.x; j < capacity; j += stride) {
        const uint32_t pix = j < listed ? pixel[j] : 0xffffffffu;
        if ((uint64_t)pix >= n_pixels) { /* beyond the list, or a pixel the frame does not have: the record of an absent candidate */
            uint32_t *const o = reinterpret_cast<uint32_t *>(rays + j);
#pragma unroll
            for (int k = 0; k < 11; ++k) o[k] = 0u;
            continue;
        }
        store_primary_ray(primary_ray_offset(fr, pix, offsets[2u * j], offsets[2u * j + 1u]), rays + j);
    }
}

/* ---- launchers ---- */

static hipError_t launch_offsets_listed(const ListedOffsetsArgs &a, hipStream_t stream) {
    return launch_groups(offsets_listed_kernel, (a.capacity + RT_IMAGE_THREADS - 1u) / RT_IMAGE_THREADS, OPT_DIAG_ADAPTIVE_MAX_GROUPS, stream, a.call());
}

static hipError_t launch_sample_list(const uint32_t *counts, uint64_t n, uint64_t capacity, uint32_t *first, uint32_t *start, uint32_t *pixel, uint32_t *sample,
                                     uint32_t *total, uint32_t *totals, hipStream_t stream) {
    const uint64_t steps = sample_list_steps(n);
    const hipError_t e = launch_groups(sample_totals_kernel, steps, OPT_DIAG_ADAPTIVE_MAX_GROUPS, stream, counts, n, steps, totals);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sample_scan_kernel, dim3(1), dim3(RT_IMAGE_THREADS), 0, stream, totals, steps, n, capacity, start, total);
    return launch_groups(sample_expand_kernel, steps, OPT_DIAG_ADAPTIVE_MAX_GROUPS, stream, counts, n, steps, totals, capacity, first, start, pixel, sample);
}

} /* namespace rt */

/* which form rt_film_splat_listed launches unless RT_AMD_FILM_SPLAT_FORM says otherwise: 0 plain, 1 tiled, as rt_film_splat (DESIGN.md 3.26
 * has the figures of both) */
#define RT_LISTED_SPLAT_FORM_DEFAULT 1

extern "C" {

int rt_sample_budget(const float *d_mean, uint32_t mean_stride, const float *d_variance, uint32_t variance_stride, const uint32_t *d_count,
                     uint32_t count_stride, const uint32_t *d_valid, uint32_t valid_stride, const rt_sample_budget_params *params, size_t n,
                     uint32_t *d_budget, void *hip_stream) {
    return device_query("rt_sample_budget",
                        rt::SampleBudgetArgs{d_mean, mean_stride, d_variance, variance_stride, d_count, count_stride, d_valid, valid_stride, params, n, d_budget},
                        rt::LaunchEach<rt::OPT_DIAG_ADAPTIVE_MAX_GROUPS>(), hip_stream);
}

size_t rt_sample_list_temp_bytes(size_t n) { return (size_t)rt::sample_list_temp_bytes(n); }

int rt_sample_list(const uint32_t *d_counts, size_t n, size_t capacity, uint32_t *d_first, uint32_t *d_start, uint32_t *d_pixel, uint32_t *d_sample,
                   uint32_t *d_total, void *d_temp, size_t temp_bytes, void *hip_stream) {
    int status;
    const char *bad = rt::sample_list_limits(d_counts, n, capacity, d_start, d_pixel, d_sample, d_total, &status);
    if (bad) return fail(status, std::string("rt_sample_list: ") + bad);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (n == 0u) {
        hipLaunchKernelGGL(rt::sample_list_empty_kernel, dim3(1), dim3(64), 0, stream, d_start, d_total);
        return launched("rt_sample_list");
    }
    if (!d_temp || temp_bytes < rt::sample_list_temp_bytes(n))
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_sample_list: temp is null or smaller than rt_sample_list_temp_bytes(n)");
    if ((reinterpret_cast<uintptr_t>(d_temp) & 3u) != 0u) return fail(RT_ERR_INVALID_ARGUMENT, "rt_sample_list: temp is not 4-byte aligned");
    return launched("rt_sample_list",
                    rt::launch_sample_list(d_counts, n, capacity, d_first, d_start, d_pixel, d_sample, d_total, static_cast<uint32_t *>(d_temp), stream));
}

int rt_film_offsets_listed(const rt_frame *frame, uint32_t pattern, uint32_t seed, const uint32_t *d_pixel, const uint32_t *d_sample, const uint32_t *d_total,
                           size_t capacity, float *d_offsets, void *hip_stream) {
    return device_query("rt_film_offsets_listed", rt::ListedOffsetsArgs{frame, pattern, seed, d_pixel, d_sample, d_total, capacity, d_offsets},
                        rt::launch_offsets_listed, hip_stream);
}

int rt_camera_rays_listed(const rt_camera *camera, const rt_frame *frame, const float *d_offsets, const uint32_t *d_pixel, const uint32_t *d_total,
                          size_t capacity, rt_ray *d_rays, void *hip_stream) {
    int status;
    const char *bad = rt::listed_rays_limits(camera, frame, d_offsets, d_pixel, d_total, capacity, d_rays, &status);
    if (bad) return fail(status, std::string("rt_camera_rays_listed: ") + bad);
    if (capacity == 0u) return RT_OK;
    rt_frame f = *frame;
    f.max_depth = 0; /* not used here */
    rt::KernelFrame kf;
    const int rc = make_kernel_frame(camera, &f, &kf);
    if (rc != RT_OK) return rc;
    return launched("rt_camera_rays_listed",
                    rt::launch_groups(rt::camera_rays_listed_kernel, (capacity + RT_IMAGE_THREADS - 1u) / RT_IMAGE_THREADS, rt::OPT_DIAG_ADAPTIVE_MAX_GROUPS,
                                      static_cast<hipStream_t>(hip_stream), kf, d_offsets, d_pixel, d_total, (uint64_t)capacity, d_rays));
}

int rt_film_splat_listed(uint32_t rows, uint32_t cols, const float *d_samples, const unsigned char *d_valid, const float *d_offsets, const uint32_t *d_start,
                         size_t capacity, uint32_t max_count, uint32_t filter, float radius, float *d_sum, float *d_weight, void *hip_stream) {
    int status;
    const char *bad = rt::listed_splat_limits(rows, cols, d_samples, d_offsets, d_start, capacity, max_count, filter, radius, d_sum, d_weight, &status);
    if (bad) return fail(status, std::string("rt_film_splat_listed: ") + bad);
    if (rows == 0u || cols == 0u) return RT_OK;
    const rt::FilmSplat<rt::ListedLayout> p = {{d_samples, d_valid, d_offsets, d_start, capacity, max_count}, d_sum, d_weight, rows, cols, filter, radius};
    const bool tiled = rt::option(rt::OPT_FILM_SPLAT_FORM, RT_LISTED_SPLAT_FORM_DEFAULT) == 1;
    return launched("rt_film_splat_listed",
                    rt::launch_film_splat_forms(p, tiled, rt::OPT_DIAG_ADAPTIVE_MAX_GROUPS, static_cast<hipStream_t>(hip_stream)));
}

} /* extern "C" */
