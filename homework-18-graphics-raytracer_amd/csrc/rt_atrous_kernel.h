/*
 * rt_atrous_kernel.h — the kernels of one A-Trous level, templates over a filter of rt_atrous.h; rt_denoise_query.hip instantiates them
 * with DenoiseFilter, rt_svgf_query.hip with SvgfFilter.
 *
 *   rt::each_kernel<AtrousEach<F>>  the simple form: one thread per output pixel (rt_image_kernel.h); the 25 sources read from global memory
 *                               (atrous_pixel, which is also the CPU form)
 *   rt::atrous_tiled_kernel<F>  the tiled form: a 256-thread workgroup owns 16 x 16 output pixels SPACED step APART — one residue class
 *                               (row mod step, column mod step) of a block of 16 step x 16 step pixels — and stages the 20 x 20 entries,
 *                               also step apart, that those outputs read: 400 entries of F::Pix (9 words, 14.4 KB of LDS, for the
 *                               denoise filter; 11 words, 17.6 KB, for the variance-guided one) at EVERY level (a contiguous tile's
 *                               halo is (16 + 4 step)^2 entries and stops fitting at step 16).  At step 1 it is the contiguous tile.
 *                               The thread split, the stager and the launch tail are rt_image_kernel.h's; the residue-class
 *                               decomposition of `tile` is this kernel's own.  Entries have an odd number of words, so a tile row
 *                               spreads over the LDS banks.
 *
 * Both walk a pixel's sources in the order of the definition — dr, then dc, ascending — and call F::load / F::tap / F::store on the same
 * operands, so they give the same bits as each other and as the CPU form by construction, whatever the launch geometry.  An output
 * pixel is written by one thread: no atomics.  The tiled form marks an entry that lies outside the image or whose valid word is cleared
 * ONCE, while staging, with F::dead(), which F::tap skips; an output pixel whose own entry is so marked collects no weight and passes
 * through, which is what the definitions say of an invalid pixel.  Guides are read through their record strides where they lie: no
 * pre-pass packs them.  Every index into a plane is 64-bit; every read is behind an inside-the-image test; rows * cols < 2^32 is checked
 * by the entry points.
 */
#ifndef RT_ATROUS_KERNEL_H
#define RT_ATROUS_KERNEL_H

#include "rt_image_kernel.h"
#include "rt_atrous.h"

namespace rt {

#define RT_ATROUS_HALO (RT_IMAGE_TILE + 4u) /* two taps either side */

/* blocks_x: blocks of 16 step x 16 step pixels across the image; n_tiles = blocks * step * step, block-major, then the residue's row, then
 * its column.  Workgroups take tiles grid-stride, so every thread of a workgroup meets the same barriers. */
template <class F>
__global__ __launch_bounds__(RT_IMAGE_THREADS) void atrous_tiled_kernel(const typename F::Level L, const uint32_t blocks_x, const uint64_t n_tiles) {
    __shared__ typename F::Pix l_pix[RT_ATROUS_HALO * RT_ATROUS_HALO];
    const int64_t step = L.step;
    const uint32_t per_block = (uint32_t)(L.step * L.step);
    const auto [ty, tx] = tile_thread();
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) { /* workgroup-uniform */
        const uint64_t block = tile / per_block;
        const uint32_t res = (uint32_t)(tile - block * per_block);
        const uint32_t block_r = (uint32_t)(block / blocks_x), block_c = (uint32_t)(block - (uint64_t)block_r * blocks_x);
        const int64_t r0 = (int64_t)block_r * RT_IMAGE_TILE * step + res / (uint32_t)L.step;
        const int64_t c0 = (int64_t)block_c * RT_IMAGE_TILE * step + res % (uint32_t)L.step;
        if (r0 >= (int64_t)L.rows || c0 >= (int64_t)L.cols) continue; /* a residue class the image's last block does not reach: uniform */
        __syncthreads(); /* the previous tile's reads are done */
        stage_halo<2u>(l_pix, r0, c0, L.rows, L.cols, step, 0u, F::dead(), [&](uint64_t qi) {
            typename F::Pix q = F::dead(); /* a cleared valid word: nobody's source either */
            if (guide_valid(L, qi)) q = F::load(L, qi);
            return q;
        });
        __syncthreads();
        const int64_t r = r0 + (int64_t)ty * step, c = c0 + (int64_t)tx * step;
        if (r < (int64_t)L.rows && c < (int64_t)L.cols) {
            const typename F::Pix p = l_pix[(ty + 2u) * RT_ATROUS_HALO + (tx + 2u)];
            typename F::Acc a = {};
            if (F::takes_taps(p)) {
                const typename F::Context k = F::context(L, (uint32_t)r, (uint32_t)c);
                for (int dr = -2; dr <= 2; ++dr)
                    for (int dc = -2; dc <= 2; ++dc) F::tap(L, a, p, l_pix[(uint32_t)((int)ty + 2 + dr) * RT_ATROUS_HALO + (uint32_t)((int)tx + 2 + dc)], k, dr, dc);
            }
            F::store(L, (uint64_t)r * L.cols + (uint64_t)c, true, a);
        }
    }
}

/* hook: the unit's cap on the workgroups of either form */
template <class F>
static hipError_t launch_atrous_level(const typename F::Level &L, bool tiled, Option hook, hipStream_t stream) {
    if (!tiled) return launch_each(AtrousEach<F>{L}, hook, stream);
    const uint64_t side = (uint64_t)RT_IMAGE_TILE * (uint64_t)L.step;
    const uint32_t blocks_x = (uint32_t)((L.cols + side - 1u) / side), blocks_y = (uint32_t)((L.rows + side - 1u) / side);
    const uint64_t n_tiles = (uint64_t)blocks_x * blocks_y * (uint64_t)L.step * (uint64_t)L.step;
    return launch_groups(atrous_tiled_kernel<F>, n_tiles, hook, stream, L, blocks_x, n_tiles);
}

/* one launch per level of a call: a.level(j) is the filter's Level */
template <class F, class Args>
static hipError_t launch_atrous(const Args &a, bool tiled, Option hook, hipStream_t stream) {
    for (uint32_t j = 0; j < a.params->n_levels; ++j) {
        const hipError_t e = launch_atrous_level<F>(a.level(j), tiled, hook, stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} /* namespace rt */

#endif /* RT_ATROUS_KERNEL_H */
