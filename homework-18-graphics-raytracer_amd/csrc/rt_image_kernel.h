/*
 * rt_image_kernel.h — the launch shape of the image-side kernels (film, denoise, temporal, SVGF, motion, rectify, adaptive), written once.
 * No arithmetic lives here: a unit brings what happens to an element or to a staged tile, this header how the elements and tiles are
 * handed to workgroups of RT_IMAGE_THREADS threads, at most RT_IMAGE_MAX_GROUPS of them (2^16 x 256 threads stay far below the 2^32
 * threads a launch may have) or what the unit's RT_AMD_DIAG_*_MAX_GROUPS hook asks for; a smaller cap changes no bit.
 *
 *   each_kernel<Op> / launch_each   one thread per element, grid-stride.  Op is a small trivially copyable struct with count() and a host-
 *                                   and-device operator()(i); librt_host.so runs the same Op in a plain loop, so a query's loop body is
 *                                   written once for both libraries.
 *   tile_thread / tile_origin /     a workgroup owns RT_IMAGE_TILE x RT_IMAGE_TILE output pixels, thread t the pixel (t / 16, t % 16) of
 *   launch_tiles                    them, and takes its tiles grid-stride: the tile loop of every such kernel is workgroup-uniform.
 *   stage_halo<REACH>               the (16 + 2 REACH)^2 entries a tile's outputs read, `step` pixels apart, into LDS: entry e by thread
 *                                   e mod 256.  An entry outside the image is the caller's "nobody"; load(qi) is called for an index
 *                                   inside the image only, so every global read is behind the inside-the-image test.
 *
 * The two invariants these kernels rely on are therefore here: a barrier stands only in a workgroup-uniform loop (the stager holds none;
 * each kernel keeps its barriers where its uniformity argument is made), and nothing outside the image is read.  film_splat_tiled_kernel
 * (rt_film_splat_kernel.h) keeps its own staging: its halo width is a runtime value, it fills two LDS arrays and it restages per sample.
 */
#ifndef RT_IMAGE_KERNEL_H
#define RT_IMAGE_KERNEL_H

#include <type_traits>

#include "rt_api_internal.h"

namespace rt {

#define RT_IMAGE_THREADS 256u
#define RT_IMAGE_TILE 16u
#define RT_IMAGE_MAX_GROUPS (1u << 16)

/* `wanted` workgroups of RT_IMAGE_THREADS under the cap: kernel(args...) takes what is beyond the grid grid-stride */
template <class Kernel, class... Args>
static hipError_t launch_groups(Kernel kernel, uint64_t wanted, Option hook, hipStream_t stream, const Args &...args) {
    const uint32_t groups = (uint32_t)std::min<uint64_t>(wanted, max_groups(hook, RT_IMAGE_MAX_GROUPS));
    hipLaunchKernelGGL(kernel, dim3(groups), dim3(RT_IMAGE_THREADS), 0, stream, args...);
    return hipGetLastError();
}

/* ---- one thread per element ---- */

template <class Op>
__global__ __launch_bounds__(RT_IMAGE_THREADS) void each_kernel(const Op op) {
    const uint64_t n = op.count(), stride = (uint64_t)gridDim.x * RT_IMAGE_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * RT_IMAGE_THREADS + threadIdx.x; i < n; i += stride) op(i);
}

template <class Op>
static hipError_t launch_each(const Op &op, Option hook, hipStream_t stream) {
    static_assert(std::is_trivially_copyable<Op>::value, "an Op travels as a kernel argument");
    return launch_groups(each_kernel<Op>, (op.count() + RT_IMAGE_THREADS - 1u) / RT_IMAGE_THREADS, hook, stream, op);
}

/* the launcher of a query (rt_query_args.h) whose call() is such an Op, under the unit's hook */
template <Option HOOK>
struct LaunchEach {
    template <class Args>
    hipError_t operator()(const Args &a, hipStream_t stream) const { return launch_each(a.call(), HOOK, stream); }
};

/* ---- one workgroup per 16 x 16 tile ---- */

struct TilePixel { uint32_t ty, tx; };
__device__ __forceinline__ TilePixel tile_thread() { return {threadIdx.x / RT_IMAGE_TILE, threadIdx.x % RT_IMAGE_TILE}; }

/* the first pixel of contiguous tile `tile`, row-major over tiles_x tiles across the image */
struct TileOrigin { int64_t r0, c0; };
__device__ __forceinline__ TileOrigin tile_origin(uint64_t tile, uint32_t tiles_x) {
    const uint32_t tile_r = (uint32_t)(tile / tiles_x), tile_c = (uint32_t)(tile - (uint64_t)tile_r * tiles_x);
    return {(int64_t)tile_r * RT_IMAGE_TILE, (int64_t)tile_c * RT_IMAGE_TILE};
}

/* kernel(args..., tiles_x, n_tiles) over the contiguous tiles of a rows x cols image */
template <class Kernel, class... Args>
static hipError_t launch_tiles(Kernel kernel, uint32_t rows, uint32_t cols, Option hook, hipStream_t stream, const Args &...args) {
    const uint32_t tiles_x = (cols + RT_IMAGE_TILE - 1u) / RT_IMAGE_TILE, tiles_y = (rows + RT_IMAGE_TILE - 1u) / RT_IMAGE_TILE;
    const uint64_t n_tiles = (uint64_t)tiles_x * tiles_y;
    return launch_groups(kernel, n_tiles, hook, stream, args..., tiles_x, n_tiles);
}

/* The halo of the tile at (r0, c0) into lds[(16 + 2 REACH)^2]: entry (hr, hc) is the pixel (r0 + (hr - REACH) step, c0 + (hc - REACH) step).
 * ring: that many outermost rows and columns of entries are never looked at and are left as they are.  No barrier: the caller puts one
 * before (the previous tile's reads) and one after. */
template <uint32_t REACH, class Entry, class Load>
__device__ __forceinline__ void stage_halo(Entry *lds, int64_t r0, int64_t c0, uint32_t rows, uint32_t cols, int64_t step, uint32_t ring, const Entry &nobody,
                                           Load load) {
    constexpr uint32_t HALO = RT_IMAGE_TILE + 2u * REACH;
    for (uint32_t e = threadIdx.x; e < HALO * HALO; e += RT_IMAGE_THREADS) {
        const uint32_t hr = e / HALO, hc = e - hr * HALO;
        if (ring != 0u && (hr < ring || hr >= HALO - ring || hc < ring || hc >= HALO - ring)) continue; /* ring 0 folds the test away */
        const int64_t qr = r0 + ((int64_t)hr - (int64_t)REACH) * step, qc = c0 + ((int64_t)hc - (int64_t)REACH) * step;
        Entry q = nobody; /* a source of nobody */
        if (qr >= 0 && qr < (int64_t)rows && qc >= 0 && qc < (int64_t)cols) q = load((uint64_t)qr * cols + (uint64_t)qc);
        lds[e] = q;
    }
}

} /* namespace rt */

#endif /* RT_IMAGE_KERNEL_H */
