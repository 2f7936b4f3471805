/*
 * rt_film_query.hip — the image side handed to the caller (include/rt_amd.h "film queries"): sub-pixel sample positions, the camera
 * rays through them, and PhotonAccumulator::accumulate_weight (photon.rs:30-33) behind a reconstruction filter.
 *
 *   rt::film_offsets_kernel          one work-item per sample: the counter hash of rt_film.h, keyed by the GLOBAL pixel index
 *   rt::camera_rays_offset_kernel    one work-item per sample: rt_primary_ray.h's primary_ray_through, the record of camera_rays_kernel
 *   rt::film_splat_kernel<FILTER>    the splat as a gather, one thread per output pixel, straight from global memory
 *   rt::film_splat_tiled_kernel<FILTER>  the same gather from LDS: a workgroup owns a 16 x 16 tile of output pixels and stages, for one
 *                                    sample index at a time, the (16 + 2 reach)^2 halo of offsets and samples
 *
 * The arithmetic is rt_film.h's, shared with librt_host.so.  Both splat kernels walk a pixel's sources in the order of the definition
 * — s outermost, then dr, then dc, ascending — and call film_covers / film_apply on the same operands, so they give the same bits as
 * each other and as rt_film_splat_host by construction, whatever the launch geometry.  An output pixel is written by one thread: no
 * atomics.  The tiled form marks a halo entry that lies outside the image or whose flag is cleared ONCE, while staging, by giving it a
 * NaN dx: the half-open support test of film_covers is false for it, as it is for a caller's own NaN offset in either form.
 * Everything is counted in 64 bits up to the record index; rows * cols < 2^32 is checked by the entry point.
 */
#include "rt_api_internal.h"
#include "rt_film.h"
#include "rt_primary_ray.h"

namespace rt {

#define RT_FILM_THREADS 256u

__global__ __launch_bounds__(RT_FILM_THREADS) void film_offsets_kernel(const FilmTile t, const uint32_t spp, const uint32_t pattern, const uint32_t k,
                                                                       const uint32_t seed, float *__restrict__ offsets) {
    const uint64_t n_pixels = (uint64_t)t.rows * t.cols;
    const uint64_t i = (uint64_t)blockIdx.x * RT_FILM_THREADS + threadIdx.x;
    if (i >= n_pixels * spp) return;
    const uint32_t s = (uint32_t)(i / n_pixels), pix = (uint32_t)(i - (uint64_t)s * n_pixels);
    const uint32_t row = pix / t.cols, col = pix - row * t.cols;
    const uint32_t pixel = (t.y0 + row * t.y_step) * t.width + (t.x0 + col); /* the global index: tiles of one frame agree */
    offsets[2u * i] = film_offset(pattern, k, pixel, seed, s, 0u);
    offsets[2u * i + 1u] = film_offset(pattern, k, pixel, seed, s, 1u);
}

__global__ __launch_bounds__(RT_FILM_THREADS) void camera_rays_offset_kernel(const KernelFrame fr, const float *__restrict__ offsets, const uint32_t spp,
                                                                             rt_ray *__restrict__ rays) {
    const uint64_t n_pixels = (uint64_t)fr.rows * fr.cols;
    const uint64_t i = (uint64_t)blockIdx.x * RT_FILM_THREADS + threadIdx.x;
    if (i >= n_pixels * spp) return;
    const uint32_t pix = (uint32_t)(i % n_pixels);
    const uint32_t row = pix / fr.cols, col = pix - row * fr.cols;
    const uint32_t x = fr.x0 + col, y = fr.y0 + row * fr.y_step;
    store_primary_ray(primary_ray_through(fr, (float)x + offsets[2u * i], (float)y + offsets[2u * i + 1u]), rays + i);
}

/* ---- the splat, simple form: every source record read from global memory by every output pixel it may reach ---- */
template <uint32_t FILTER>
__global__ __launch_bounds__(RT_FILM_THREADS) void film_splat_kernel(const FilmSplat p) {
    const uint64_t n = (uint64_t)p.rows * p.cols, stride = (uint64_t)gridDim.x * RT_FILM_THREADS;
    const int reach = film_reach(p.radius);
    for (uint64_t i = (uint64_t)blockIdx.x * RT_FILM_THREADS + threadIdx.x; i < n; i += stride) {
        const uint32_t r = (uint32_t)(i / p.cols), c = (uint32_t)(i - (uint64_t)r * p.cols);
        FilmAcc a = {p.sum[3u * i], p.sum[3u * i + 1u], p.sum[3u * i + 2u], p.weight[i]};
        for (uint32_t s = 0; s < p.spp; ++s) {
            const uint64_t base = (uint64_t)s * n;
            for (int dr = -reach; dr <= reach; ++dr) {
                const int64_t qr = (int64_t)r + dr;
                if (qr < 0 || qr >= (int64_t)p.rows) continue;
                for (int dc = -reach; dc <= reach; ++dc) {
                    const int64_t qc = (int64_t)c + dc;
                    if (qc < 0 || qc >= (int64_t)p.cols) continue;
                    const uint64_t rec = base + (uint64_t)qr * p.cols + (uint64_t)qc;
                    if (p.valid != nullptr && p.valid[rec] == 0u) continue;
                    float ddx, ddy;
                    if (!film_covers(dr, dc, p.offsets[2u * rec], p.offsets[2u * rec + 1u], p.radius, &ddx, &ddy)) continue;
                    film_apply(a, FILTER, p.radius, ddx, ddy, p.samples[3u * rec], p.samples[3u * rec + 1u], p.samples[3u * rec + 2u]);
                }
            }
        }
        p.sum[3u * i] = a.s0;
        p.sum[3u * i + 1u] = a.s1;
        p.sum[3u * i + 2u] = a.s2;
        p.weight[i] = a.w;
    }
}

/* ---- the splat, tiled form ----
 * 256 threads = a 16 x 16 tile; the halo is (16 + 2 reach) entries wide, reach <= 5 (radius <= 4): at most 26 x 26 = 676 entries of
 * 5 dwords, 13.5 KB of LDS.  Staging: entry e of the halo by thread e, e + 256, ...: consecutive threads read consecutive records of an
 * image row.  Workgroups take tiles grid-stride, so every thread of a workgroup meets the same barriers. */
#define RT_FILM_TILE 16u
#define RT_FILM_HALO_MAX (RT_FILM_TILE + 2u * 5u)
template <uint32_t FILTER>
__global__ __launch_bounds__(RT_FILM_THREADS) void film_splat_tiled_kernel(const FilmSplat p, const uint32_t tiles_x, const uint64_t n_tiles) {
    __shared__ float2 l_off[RT_FILM_HALO_MAX * RT_FILM_HALO_MAX];
    __shared__ float l_smp[RT_FILM_HALO_MAX * RT_FILM_HALO_MAX * 3u];
    const uint64_t n = (uint64_t)p.rows * p.cols;
    const int reach = film_reach(p.radius);
    const uint32_t halo = RT_FILM_TILE + 2u * (uint32_t)reach; /* <= RT_FILM_HALO_MAX: the entry point bounds the radius */
    const uint32_t ty = threadIdx.x / RT_FILM_TILE, tx = threadIdx.x % RT_FILM_TILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) { /* workgroup-uniform */
        const uint32_t tile_r = (uint32_t)(tile / tiles_x), tile_c = (uint32_t)(tile - (uint64_t)tile_r * tiles_x);
        const int64_t r0 = (int64_t)tile_r * RT_FILM_TILE, c0 = (int64_t)tile_c * RT_FILM_TILE;
        const int64_t r = r0 + ty, c = c0 + tx;
        const bool inside = r < (int64_t)p.rows && c < (int64_t)p.cols;
        const uint64_t i = inside ? (uint64_t)r * p.cols + (uint64_t)c : 0u;
        FilmAcc a = {0.0f, 0.0f, 0.0f, 0.0f};
        if (inside) a = {p.sum[3u * i], p.sum[3u * i + 1u], p.sum[3u * i + 2u], p.weight[i]};
        for (uint32_t s = 0; s < p.spp; ++s) {
            const uint64_t base = (uint64_t)s * n;
            __syncthreads(); /* the previous sample's (or tile's) reads are done */
            for (uint32_t e = threadIdx.x; e < halo * halo; e += RT_FILM_THREADS) {
                const uint32_t hr = e / halo, hc = e - hr * halo;
                const int64_t qr = r0 - reach + hr, qc = c0 - reach + hc;
                float2 off = make_float2(__uint_as_float(0x7fc00000u), 0.0f); /* NaN dx: contributes to nobody */
                float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
                if (qr >= 0 && qr < (int64_t)p.rows && qc >= 0 && qc < (int64_t)p.cols) {
                    const uint64_t rec = base + (uint64_t)qr * p.cols + (uint64_t)qc;
                    if (p.valid == nullptr || p.valid[rec] != 0u) {
                        off = make_float2(p.offsets[2u * rec], p.offsets[2u * rec + 1u]);
                        s0 = p.samples[3u * rec];
                        s1 = p.samples[3u * rec + 1u];
                        s2 = p.samples[3u * rec + 2u];
                    }
                }
                l_off[e] = off;
                l_smp[3u * e] = s0;
                l_smp[3u * e + 1u] = s1;
                l_smp[3u * e + 2u] = s2;
            }
            __syncthreads();
            if (inside) {
                for (int dr = -reach; dr <= reach; ++dr) {
                    const uint32_t row_e = (uint32_t)((int)ty + reach + dr) * halo + (uint32_t)((int)tx + reach);
                    for (int dc = -reach; dc <= reach; ++dc) {
                        const uint32_t e = (uint32_t)((int)row_e + dc);
                        const float2 off = l_off[e];
                        float ddx, ddy;
                        if (!film_covers(dr, dc, off.x, off.y, p.radius, &ddx, &ddy)) continue;
                        film_apply(a, FILTER, p.radius, ddx, ddy, l_smp[3u * e], l_smp[3u * e + 1u], l_smp[3u * e + 2u]);
                    }
                }
            }
        }
        if (inside) {
            p.sum[3u * i] = a.s0;
            p.sum[3u * i + 1u] = a.s1;
            p.sum[3u * i + 2u] = a.s2;
            p.weight[i] = a.w;
        }
    }
}

hipError_t launch_film_offsets(const FilmTile &t, uint32_t spp, uint32_t pattern, uint32_t seed, float *offsets, hipStream_t stream) {
    const uint64_t n = (uint64_t)t.rows * t.cols * spp;
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(film_offsets_kernel, grid_of(n, RT_FILM_THREADS), dim3(RT_FILM_THREADS), 0, stream, t, spp, pattern, film_strata(spp), seed, offsets);
    return hipGetLastError();
}

hipError_t launch_camera_rays_offset(const KernelFrame &fr, const float *offsets, uint32_t spp, rt_ray *rays, hipStream_t stream) {
    const uint64_t n = (uint64_t)fr.rows * fr.cols * spp;
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(camera_rays_offset_kernel, grid_of(n, RT_FILM_THREADS), dim3(RT_FILM_THREADS), 0, stream, fr, offsets, spp, rays);
    return hipGetLastError();
}

template <uint32_t FILTER>
static void launch_film_splat_of(const FilmSplat &p, bool tiled, uint32_t max_groups, hipStream_t stream) {
    if (tiled) {
        const uint32_t tiles_x = (p.cols + RT_FILM_TILE - 1u) / RT_FILM_TILE, tiles_y = (p.rows + RT_FILM_TILE - 1u) / RT_FILM_TILE;
        const uint64_t n_tiles = (uint64_t)tiles_x * tiles_y;
        const uint32_t groups = (uint32_t)std::min<uint64_t>(n_tiles, max_groups);
        hipLaunchKernelGGL(film_splat_tiled_kernel<FILTER>, dim3(groups), dim3(RT_FILM_THREADS), 0, stream, p, tiles_x, n_tiles);
    } else {
        const uint64_t groups = ((uint64_t)p.rows * p.cols + RT_FILM_THREADS - 1u) / RT_FILM_THREADS;
        hipLaunchKernelGGL(film_splat_kernel<FILTER>, dim3((uint32_t)std::min<uint64_t>(groups, max_groups)), dim3(RT_FILM_THREADS), 0, stream, p);
    }
}

hipError_t launch_film_splat(const FilmSplat &p, bool tiled, uint32_t max_groups, hipStream_t stream) {
    if (p.rows == 0u || p.cols == 0u || p.spp == 0u) return hipSuccess;
    if (max_groups < 1u || max_groups > RT_FILM_MAX_GROUPS) return hipErrorInvalidValue;
    if (!(p.radius > 0.0f) || film_reach(p.radius) > 5) return hipErrorInvalidValue; /* the tiled form's LDS holds a halo of reach 5 */
    if (p.filter == RT_FILM_BOX) launch_film_splat_of<RT_FILM_BOX>(p, tiled, max_groups, stream);
    else if (p.filter == RT_FILM_TENT) launch_film_splat_of<RT_FILM_TENT>(p, tiled, max_groups, stream);
    else launch_film_splat_of<RT_FILM_MITCHELL>(p, tiled, max_groups, stream);
    return hipGetLastError();
}

} /* namespace rt */
