/*
 * rt_upsample_query.hip — the guided upsampling queries (include/rt_amd.h "guided upsampling queries"): a low-resolution colour carried
 * onto full-resolution guide planes by a joint bilateral upsample; kernels and entry points in one unit.
 *
 *   rt::each_kernel<UpsampleCall>   the plain form: one thread per output pixel, grid-stride, every source read from global memory — the
 *                                   Op librt_host.so runs in a loop (rt_image_kernel.h has the element loop)
 *   rt::upsample_tiled_kernel<R>    the tiled form: a 256-thread workgroup owns 16 x 16 output pixels and stages the low-resolution
 *                                   window they can touch once — rows b(r0) - (R - 1) .. b(r0 + 15) + R and the same for columns, at most
 *                                   12 x 12 sources (scale 2, radius 2) — as ten planes of 13 x 13 words, 6.8 KB of LDS: the colour as
 *                                   the walk sees it (demodulated while staging), normal, position, object.  Each thread then walks its
 *                                   (2 R)^2 taps in LDS; its own full-resolution guides it reads once, from global memory.
 *
 * The arithmetic is rt_upsample.h's, shared with librt_host.so: both forms call upsample_pixel on the same operands in the same order, so
 * they give the same bits by construction, whatever the launch geometry.  The tile walk is rt_image_kernel.h's; the stager is this
 * unit's own, because its window is of ANOTHER resolution than the tile (stage_halo maps a halo of the tile's own).  A source that does
 * not exist — outside the low image, valid word cleared — is marked ONCE, while staging, with UpsampleSource::dead().  The window is
 * a structure of arrays: the threads of a tile row read entries that lie side by side (several threads the same one, a broadcast), so
 * every plane is read at consecutive words, and a window row is 13 words, an odd number, so the four tile rows of a wave spread over the
 * banks.  Workgroups take tiles grid-stride and every barrier stands in the workgroup-uniform tile loop.  An output word is written by
 * one thread: no atomics.  Every index into a plane is 64-bit; every global read is behind an inside-the-image test; rows * cols < 2^32
 * is checked by the entry points.
 */
#include "rt_image_kernel.h"
#include "rt_upsample.h"

namespace rt {

/* A tile's window along one axis: 16 output pixels from r0 span b(r0 + 15) - b(r0) + 1 <= 30 / (2 s) + 2 <= 9 bases (s >= 2), and the
 * taps add R - 1 before and R after: at most 8 + 2 R = 12 sources at scale 2, radius 2.  13 keeps a window row an odd number of words. */
#define RT_UPSAMPLE_WINDOW 13u
#define RT_UPSAMPLE_PLANES 9u /* colour 3, normal 3, position 3; the object plane is a tenth, of its own type */

/* tiles_x: tiles of 16 x 16 output pixels across the image */
template <int R>
__global__ __launch_bounds__(RT_IMAGE_THREADS) void upsample_tiled_kernel(const UpsampleCall u, const uint32_t tiles_x, const uint64_t n_tiles) {
    constexpr uint32_t W = RT_UPSAMPLE_WINDOW;
    __shared__ float l_f[RT_UPSAMPLE_PLANES][W * W];
    __shared__ uint32_t l_object[W * W];
    const auto [ty, tx] = tile_thread();
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) { /* workgroup-uniform */
        const auto [r0, c0] = tile_origin(tile, tiles_x);
        /* the window: low-resolution rows wy0 .. wy0 + ny - 1, columns wx0 .. wx0 + nx - 1; the tile's last pixel inside the image bounds it */
        const int64_t r_end = r0 + (int64_t)(RT_IMAGE_TILE - 1u), c_end = c0 + (int64_t)(RT_IMAGE_TILE - 1u);
        const uint32_t r1 = (uint32_t)(r_end < (int64_t)u.hi.rows ? r_end : (int64_t)u.hi.rows - 1);
        const uint32_t c1 = (uint32_t)(c_end < (int64_t)u.hi.cols ? c_end : (int64_t)u.hi.cols - 1);
        const int64_t wy0 = upsample_base((uint32_t)r0, u.scale) - (R - 1), wx0 = upsample_base((uint32_t)c0, u.scale) - (R - 1);
        const uint32_t ny = (uint32_t)(upsample_base(r1, u.scale) + R - wy0 + 1), nx = (uint32_t)(upsample_base(c1, u.scale) + R - wx0 + 1);
        __syncthreads(); /* the previous tile's reads are done */
        for (uint32_t e = threadIdx.x; e < W * W; e += RT_IMAGE_THREADS) {
            const uint32_t wr = e / W, wc = e - wr * W;
            if (wr >= ny || wc >= nx) continue; /* no pixel of this tile looks there */
            const UpsampleSource q = upsample_source_at(u, wy0 + wr, wx0 + wc);
            l_f[0][e] = q.c0, l_f[1][e] = q.c1, l_f[2][e] = q.c2;
            l_f[3][e] = q.g.n0, l_f[4][e] = q.g.n1, l_f[5][e] = q.g.n2;
            l_f[6][e] = q.g.p0, l_f[7][e] = q.g.p1, l_f[8][e] = q.g.p2;
            l_object[e] = q.object;
        }
        __syncthreads();
        const int64_t r = r0 + ty, c = c0 + tx;
        if (r >= (int64_t)u.hi.rows || c >= (int64_t)u.hi.cols) continue; /* no barrier below */
        const UpsampleAxis<R> y = upsample_axis<R>((uint32_t)r, u.scale), x = upsample_axis<R>((uint32_t)c, u.scale);
        /* b(r0) <= y.b <= b(r1): tap (kr, kc) is window entry (y.b - (R - 1) - wy0 + kr, x.b - (R - 1) - wx0 + kc), inside [0, ny) x [0, nx) */
        const uint32_t first = (uint32_t)(y.b - (R - 1) - wy0) * W + (uint32_t)(x.b - (R - 1) - wx0);
        upsample_pixel<R>(u, (uint32_t)r, (uint32_t)c, y, x, [&](int kr, int kc) {
            const uint32_t e = first + (uint32_t)kr * W + (uint32_t)kc;
            return UpsampleSource{l_f[0][e], l_f[1][e], l_f[2][e], {l_f[3][e], l_f[4][e], l_f[5][e], l_f[6][e], l_f[7][e], l_f[8][e]}, l_object[e]};
        });
    }
}

/* which form rt_upsample_guided launches unless RT_AMD_UPSAMPLE_FORM says otherwise: 0 plain, 1 tiled (same bits; DESIGN.md 3.28 has the A/B) */
#define RT_UPSAMPLE_FORM_DEFAULT 1

static hipError_t launch_upsample(const UpsampleArgs &a, hipStream_t stream) {
    const UpsampleCall u = a.call();
    if (option(OPT_UPSAMPLE_FORM, RT_UPSAMPLE_FORM_DEFAULT) != 1) return launch_each(u, OPT_DIAG_UPSAMPLE_MAX_GROUPS, stream);
    if (u.radius == 1) return launch_tiles(upsample_tiled_kernel<1>, u.hi.rows, u.hi.cols, OPT_DIAG_UPSAMPLE_MAX_GROUPS, stream, u);
    return launch_tiles(upsample_tiled_kernel<2>, u.hi.rows, u.hi.cols, OPT_DIAG_UPSAMPLE_MAX_GROUPS, stream, u);
}

} /* namespace rt */

extern "C" {

int rt_upsample_guided(const float *d_color_lo, uint32_t color_stride, const rt_denoise_guides *low, const uint32_t *d_object_lo, uint32_t object_lo_stride,
                       const rt_denoise_guides *full, const uint32_t *d_object_full, uint32_t object_full_stride, const rt_upsample_params *params,
                       uint32_t rows, uint32_t cols, float *d_out, void *hip_stream) {
    return device_query("rt_upsample_guided",
                        rt::UpsampleArgs{d_color_lo, color_stride, low, d_object_lo, object_lo_stride, full, d_object_full, object_full_stride, params, rows, cols, d_out},
                        rt::launch_upsample, hip_stream);
}

int rt_upsample_guided_host(const float *h_color_lo, uint32_t color_stride, const rt_denoise_guides *low, const uint32_t *h_object_lo, uint32_t object_lo_stride,
                            const rt_denoise_guides *full, const uint32_t *h_object_full, uint32_t object_full_stride, const rt_upsample_params *params,
                            uint32_t rows, uint32_t cols, float *h_out) {
    return host_query("rt_upsample_guided_host",
                      rt::UpsampleArgs{h_color_lo, color_stride, low, h_object_lo, object_lo_stride, full, h_object_full, object_full_stride, params, rows, cols, h_out},
                      rt::launch_upsample);
}

} /* extern "C" */

