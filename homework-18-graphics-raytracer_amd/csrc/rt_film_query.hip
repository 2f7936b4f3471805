/*
 * rt_film_query.hip — the image side handed to the caller (include/rt_amd.h "film queries"): sub-pixel sample positions, the camera
 * rays through them, and PhotonAccumulator::accumulate_weight (photon.rs:30-33) behind a reconstruction filter.
 *
 *   rt::film_offsets_kernel          one work-item per sample: the counter hash of rt_film.h, keyed by the GLOBAL pixel index
 *   rt::camera_rays_offset_kernel    one work-item per sample: rt_primary_ray.h's primary_ray_offset, the record of camera_rays_kernel
 *   the splat                        rt_film_splat_kernel.h's two forms, instantiated for rt_film.h's UniformLayout (sample-major records,
 *                                    spp samples per pixel); that header says what they do and why they agree bit for bit
 *
 * The arithmetic is rt_film.h's, shared with librt_host.so.
 */
#include "rt_film_splat_kernel.h"
#include "rt_primary_ray.h"

namespace rt {

__global__ __launch_bounds__(RT_IMAGE_THREADS) void film_offsets_kernel(const FilmTile t, const uint32_t spp, const uint32_t pattern, const uint32_t k,
                                                                       const uint32_t seed, float *__restrict__ offsets) {
    const uint64_t n_pixels = (uint64_t)t.rows * t.cols;
    const uint64_t i = (uint64_t)blockIdx.x * RT_IMAGE_THREADS + threadIdx.x;
    if (i >= n_pixels * spp) return;
    const uint32_t s = (uint32_t)(i / n_pixels), pix = (uint32_t)(i - (uint64_t)s * n_pixels);
    const uint32_t row = pix / t.cols, col = pix - row * t.cols;
    const uint32_t pixel = film_global_pixel(t, row, col);
    offsets[2u * i] = film_offset(pattern, k, pixel, seed, s, 0u);
    offsets[2u * i + 1u] = film_offset(pattern, k, pixel, seed, s, 1u);
}

__global__ __launch_bounds__(RT_IMAGE_THREADS) void camera_rays_offset_kernel(const KernelFrame fr, const float *__restrict__ offsets, const uint32_t spp,
                                                                             rt_ray *__restrict__ rays) {
    const uint64_t n_pixels = (uint64_t)fr.rows * fr.cols;
    const uint64_t i = (uint64_t)blockIdx.x * RT_IMAGE_THREADS + threadIdx.x;
    if (i >= n_pixels * spp) return;
    store_primary_ray(primary_ray_offset(fr, (uint32_t)(i % n_pixels), offsets[2u * i], offsets[2u * i + 1u]), rays + i);
}

hipError_t launch_film_offsets(const FilmTile &t, uint32_t spp, uint32_t pattern, uint32_t seed, float *offsets, hipStream_t stream) {
    const uint64_t n = (uint64_t)t.rows * t.cols * spp;
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(film_offsets_kernel, grid_of(n, RT_IMAGE_THREADS), dim3(RT_IMAGE_THREADS), 0, stream, t, spp, pattern, film_strata(spp), seed, offsets);
    return hipGetLastError();
}

hipError_t launch_camera_rays_offset(const KernelFrame &fr, const float *offsets, uint32_t spp, rt_ray *rays, hipStream_t stream) {
    const uint64_t n = (uint64_t)fr.rows * fr.cols * spp;
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(camera_rays_offset_kernel, grid_of(n, RT_IMAGE_THREADS), dim3(RT_IMAGE_THREADS), 0, stream, fr, offsets, spp, rays);
    return hipGetLastError();
}

hipError_t launch_film_splat(const FilmSplat<UniformLayout> &p, bool tiled, hipStream_t stream) {
    return launch_film_splat_forms(p, tiled, OPT_DIAG_FILM_MAX_GROUPS, stream);
}

} /* namespace rt */
