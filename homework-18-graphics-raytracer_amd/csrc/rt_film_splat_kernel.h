/*
 * rt_film_splat_kernel.h — the two forms of the film splat, templates over the filter and a layout of rt_film.h; rt_film_query.hip
 * instantiates them with UniformLayout (rt_film_splat), rt_adaptive_query.hip with rt_adaptive.h's ListedLayout (rt_film_splat_listed).
 *
 *   rt::each_kernel<FilmSplatEach<FILTER, Layout>>  the plain gather: one thread per output pixel (rt_image_kernel.h), straight from global
 *                                                memory (film_splat_pixel, which is also the CPU form)
 *   rt::film_splat_tiled_kernel<FILTER, Layout>  the same gather from LDS: a 256-thread workgroup owns a 16 x 16 tile of output pixels and
 *                                                stages, for one sample index at a time, the (16 + 2 reach)^2 halo of offsets and samples:
 *                                                at most 26 x 26 = 676 entries of 5 words, 13.5 KB.  Entry e is staged by thread e,
 *                                                e + 256, ...: consecutive threads read consecutive source pixels of an image row.
 *
 * Both walk a pixel's sources in the order of the definition — s outermost, then dr, then dc, ascending — and call film_covers /
 * film_apply on the same operands, so they give the same bits as each other and as the CPU forms by construction, whatever the launch
 * geometry.  An output pixel is written by one thread: no atomics.  The tiled form marks a halo entry that has no sample s — outside the
 * image, beyond its pixel's count, or with a cleared flag — ONCE, while staging, by giving it a NaN dx: the half-open support test of
 * film_covers is false for it, as it is for a caller's own NaN offset in either form.
 *
 * A ragged layout (Layout::ragged) costs the tiled form three things the uniform one does not pay for — they are compiled out of it, with
 * their LDS: the halo's record ranges (lo, count) are staged once per tile, 2 more words per entry (18.5 KB in all); the largest count of
 * the halo is reduced over the workgroup; and the s loop ends there, so an s that no pixel of the halo has is skipped and a tile whose
 * halo has no sample stages nothing.  Workgroups take tiles grid-stride and every loop that holds a barrier has workgroup-uniform bounds.
 * Everything is counted in 64 bits up to the record index; rows * cols < 2^32 is checked by the entry points.
 */
#ifndef RT_FILM_SPLAT_KERNEL_H
#define RT_FILM_SPLAT_KERNEL_H

#include "rt_image_kernel.h"
#include "rt_film.h"

namespace rt {

#define RT_FILM_HALO_MAX (RT_IMAGE_TILE + 2u * 5u) /* reach <= 5: radius <= 4 */
#define RT_FILM_HALO_ENTRIES (RT_FILM_HALO_MAX * RT_FILM_HALO_MAX)

template <uint32_t FILTER, class Layout>
__global__ __launch_bounds__(RT_IMAGE_THREADS) void film_splat_tiled_kernel(const FilmSplat<Layout> p, const uint32_t tiles_x, const uint64_t n_tiles) {
    constexpr uint32_t RANGES = Layout::ragged ? RT_FILM_HALO_ENTRIES : 1u;
    __shared__ float2 l_off[RT_FILM_HALO_ENTRIES];
    __shared__ float l_smp[RT_FILM_HALO_ENTRIES * 3u];
    __shared__ uint32_t l_lo[RANGES], l_cnt[RANGES], l_max[Layout::ragged ? RT_IMAGE_THREADS / 64u : 1u];
    const Layout &L = p.layout;
    const int reach = film_reach(p.radius);
    const uint32_t halo = RT_IMAGE_TILE + 2u * (uint32_t)reach; /* <= RT_FILM_HALO_MAX: the launcher bounds the reach */
    const auto [ty, tx] = tile_thread();
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) { /* workgroup-uniform */
        const TileOrigin origin = tile_origin(tile, tiles_x);
        const int64_t r0 = origin.r0, c0 = origin.c0; /* by name: the lambda below captures them */
        const int64_t r = r0 + ty, c = c0 + tx;
        const bool inside = r < (int64_t)p.rows && c < (int64_t)p.cols;
        const uint64_t i = inside ? (uint64_t)r * p.cols + (uint64_t)c : 0u;
        FilmAcc a = {0.0f, 0.0f, 0.0f, 0.0f};
        if (inside) a = {p.sum[3u * i], p.sum[3u * i + 1u], p.sum[3u * i + 2u], p.weight[i]};
        /* the samples of halo entry e, none outside the image */
        const auto entry_range = [&](uint32_t e, uint64_t *lo) -> uint32_t {
            const uint32_t hr = e / halo, hc = e - hr * halo;
            const int64_t qr = r0 - reach + hr, qc = c0 - reach + hc;
            *lo = 0u;
            if (qr < 0 || qr >= (int64_t)p.rows || qc < 0 || qc >= (int64_t)p.cols) return 0u;
            return L.range((uint64_t)qr * p.cols + (uint64_t)qc, lo);
        };
        uint32_t s_end = L.s_end();
        if constexpr (Layout::ragged) {
            __syncthreads(); /* the previous tile's reads are done */
            uint32_t most = 0u;
            for (uint32_t e = threadIdx.x; e < halo * halo; e += RT_IMAGE_THREADS) { /* the halo's record ranges, once per tile */
                uint64_t lo;
                const uint32_t cnt = entry_range(e, &lo);
                l_lo[e] = (uint32_t)lo; /* below 2^32 in every layout */
                l_cnt[e] = cnt;
                most = cnt > most ? cnt : most;
            }
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t other = __shfl_down(most, off, 64);
                most = other > most ? other : most;
            }
            if ((threadIdx.x & 63u) == 0u) l_max[threadIdx.x >> 6] = most;
            __syncthreads();
            most = 0u;
#pragma unroll
            for (uint32_t w = 0; w < RT_IMAGE_THREADS / 64u; ++w) most = l_max[w] > most ? l_max[w] : most;
            s_end = most < s_end ? most : s_end; /* workgroup-uniform: an s at or beyond it has no source in the halo */
        }
        for (uint32_t s = 0; s < s_end; ++s) {
            __syncthreads(); /* the previous sample's (or tile's) reads are done */
            for (uint32_t e = threadIdx.x; e < halo * halo; e += RT_IMAGE_THREADS) {
                uint64_t lo;
                uint32_t cnt;
                if constexpr (Layout::ragged) lo = l_lo[e], cnt = l_cnt[e];
                else cnt = entry_range(e, &lo);
                float2 off = make_float2(__uint_as_float(RT_FILM_NAN), 0.0f); /* contributes to nobody */
                float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
                if (s < cnt) {
                    const uint64_t rec = L.record(lo, s);
                    if (L.valid == nullptr || L.valid[rec] != 0u) {
                        off = make_float2(L.offsets[2u * rec], L.offsets[2u * rec + 1u]);
                        s0 = L.samples[3u * rec];
                        s1 = L.samples[3u * rec + 1u];
                        s2 = L.samples[3u * rec + 2u];
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

template <uint32_t FILTER, class Layout>
static hipError_t launch_film_splat_of(const FilmSplat<Layout> &p, bool tiled, Option hook, hipStream_t stream) {
    if (tiled) return launch_tiles(film_splat_tiled_kernel<FILTER, Layout>, p.rows, p.cols, hook, stream, p);
    return launch_each(FilmSplatEach<FILTER, Layout>{p}, hook, stream);
}

/* tiled: the LDS form instead of the plain one (same bits).  hook: the unit's cap on the workgroups of either form */
template <class Layout>
static hipError_t launch_film_splat_forms(const FilmSplat<Layout> &p, bool tiled, Option hook, hipStream_t stream) {
    if (p.rows == 0u || p.cols == 0u || p.layout.s_end() == 0u) return hipSuccess;
    if (!(p.radius > 0.0f) || film_reach(p.radius) > 5) return hipErrorInvalidValue; /* the tiled form's LDS holds a halo of reach 5 */
    if (p.filter == RT_FILM_BOX) return launch_film_splat_of<RT_FILM_BOX>(p, tiled, hook, stream);
    if (p.filter == RT_FILM_TENT) return launch_film_splat_of<RT_FILM_TENT>(p, tiled, hook, stream);
    return launch_film_splat_of<RT_FILM_MITCHELL>(p, tiled, hook, stream);
}

} /* namespace rt */

#endif /* RT_FILM_SPLAT_KERNEL_H */
