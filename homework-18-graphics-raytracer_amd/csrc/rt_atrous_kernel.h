/*
 * rt_atrous_kernel.h — the kernels of one A-Trous level, templates over a filter of rt_atrous.h; rt_denoise_query.hip instantiates them
 * with DenoiseFilter, rt_svgf_query.hip with SvgfFilter.
 *
 *   rt::atrous_kernel<F>        the simple form: one thread per output pixel, grid-stride; the 25 sources read from global memory
 *                               (atrous_pixel, which is also the CPU form)
 *   rt::atrous_tiled_kernel<F>  the tiled form: a 256-thread workgroup owns 16 x 16 output pixels SPACED step APART — one residue class
 *                               (row mod step, column mod step) of a block of 16 step x 16 step pixels — and stages the 20 x 20 entries,
 *                               also step apart, that those outputs read: 400 entries of F::Pix (9 words, 14.4 KB of LDS, for the
 *                               denoise filter; 11 words, 17.6 KB, for the variance-guided one) at EVERY level (a contiguous tile's
 *                               halo is (16 + 4 step)^2 entries and stops fitting at step 16).  At step 1 it is the contiguous tile.
 *                               Entry e is staged by thread e mod 256.  Entries have an odd number of words, so a tile row spreads
 *                               over the LDS banks.
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

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "rt_atrous.h"

namespace rt {

#define RT_ATROUS_THREADS 256u
#define RT_ATROUS_TILE 16u
#define RT_ATROUS_HALO (RT_ATROUS_TILE + 4u) /* two taps either side */
#define RT_ATROUS_MAX_GROUPS (1u << 16)

template <class F>
__global__ __launch_bounds__(RT_ATROUS_THREADS) void atrous_kernel(const typename F::Level L) {
    const uint64_t n = (uint64_t)L.rows * L.cols, stride = (uint64_t)gridDim.x * RT_ATROUS_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * RT_ATROUS_THREADS + threadIdx.x; i < n; i += stride) {
        const uint32_t r = (uint32_t)(i / L.cols), c = (uint32_t)(i - (uint64_t)r * L.cols);
        atrous_pixel<F>(L, r, c);
    }
}

/* blocks_x: blocks of 16 step x 16 step pixels across the image; n_tiles = blocks * step * step, block-major, then the residue's row, then
 * its column.  Workgroups take tiles grid-stride, so every thread of a workgroup meets the same barriers. */
template <class F>
__global__ __launch_bounds__(RT_ATROUS_THREADS) void atrous_tiled_kernel(const typename F::Level L, const uint32_t blocks_x, const uint64_t n_tiles) {
    __shared__ typename F::Pix l_pix[RT_ATROUS_HALO * RT_ATROUS_HALO];
    const int64_t step = L.step;
    const uint32_t per_block = (uint32_t)(L.step * L.step);
    const uint32_t ty = threadIdx.x / RT_ATROUS_TILE, tx = threadIdx.x % RT_ATROUS_TILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) { /* workgroup-uniform */
        const uint64_t block = tile / per_block;
        const uint32_t res = (uint32_t)(tile - block * per_block);
        const uint32_t block_r = (uint32_t)(block / blocks_x), block_c = (uint32_t)(block - (uint64_t)block_r * blocks_x);
        const int64_t r0 = (int64_t)block_r * RT_ATROUS_TILE * step + res / (uint32_t)L.step;
        const int64_t c0 = (int64_t)block_c * RT_ATROUS_TILE * step + res % (uint32_t)L.step;
        if (r0 >= (int64_t)L.rows || c0 >= (int64_t)L.cols) continue; /* a residue class the image's last block does not reach: uniform */
        __syncthreads(); /* the previous tile's reads are done */
        for (uint32_t e = threadIdx.x; e < RT_ATROUS_HALO * RT_ATROUS_HALO; e += RT_ATROUS_THREADS) {
            const uint32_t hr = e / RT_ATROUS_HALO, hc = e - hr * RT_ATROUS_HALO;
            const int64_t qr = r0 + ((int64_t)hr - 2) * step, qc = c0 + ((int64_t)hc - 2) * step;
            typename F::Pix q = F::dead(); /* a source of nobody */
            if (qr >= 0 && qr < (int64_t)L.rows && qc >= 0 && qc < (int64_t)L.cols) {
                const uint64_t qi = (uint64_t)qr * L.cols + (uint64_t)qc;
                if (guide_valid(L, qi)) q = F::load(L, qi);
            }
            l_pix[e] = q;
        }
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

/* max_groups: both forms take their pixels or tiles grid-stride beyond this many workgroups, 1 .. RT_ATROUS_MAX_GROUPS */
template <class F>
static hipError_t launch_atrous_level(const typename F::Level &L, bool tiled, uint32_t max_groups, hipStream_t stream) {
    if (tiled) {
        const uint64_t side = (uint64_t)RT_ATROUS_TILE * (uint64_t)L.step;
        const uint32_t blocks_x = (uint32_t)((L.cols + side - 1u) / side), blocks_y = (uint32_t)((L.rows + side - 1u) / side);
        const uint64_t n_tiles = (uint64_t)blocks_x * blocks_y * (uint64_t)L.step * (uint64_t)L.step;
        hipLaunchKernelGGL(atrous_tiled_kernel<F>, dim3((uint32_t)std::min<uint64_t>(n_tiles, max_groups)), dim3(RT_ATROUS_THREADS), 0, stream, L, blocks_x, n_tiles);
    } else {
        const uint64_t groups = ((uint64_t)L.rows * L.cols + RT_ATROUS_THREADS - 1u) / RT_ATROUS_THREADS;
        hipLaunchKernelGGL(atrous_kernel<F>, dim3((uint32_t)std::min<uint64_t>(groups, max_groups)), dim3(RT_ATROUS_THREADS), 0, stream, L);
    }
    return hipGetLastError();
}

/* one launch per level of a call: level_of(j) is the filter's Level */
template <class F, class LevelOf>
static hipError_t launch_atrous(uint32_t n_levels, bool tiled, uint32_t max_groups, hipStream_t stream, LevelOf level_of) {
    for (uint32_t j = 0; j < n_levels; ++j) {
        const hipError_t e = launch_atrous_level<F>(level_of(j), tiled, max_groups, stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} /* namespace rt */

#endif /* RT_ATROUS_KERNEL_H */
