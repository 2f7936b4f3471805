/*
 * rt_bloom_query.hip — the bloom queries (include/rt_amd.h "bloom queries"): the highlights above a threshold spread down and up a
 * pyramid and added back, between rt_post_process_device and rt_encode_srgb8_device; kernels and entry points in one unit.  A call is
 * 2 L stream-ordered launches and nothing else (rt_bloom.h bloom_steps): L down launches, the first fused with the bright pass, L - 1
 * up-and-add launches and the composite.
 *
 *   rt::each_kernel<BloomDown / BloomUp / BloomComposite>
 *                                   the plain form: one thread per output pixel, grid-stride, every tap read from global memory (level 1
 *                                   evaluates the bright pass per tap, 16 times per output) — the Ops librt_host.so runs in a loop
 *                                   (rt_image_kernel.h has the element loop)
 *   rt::bloom_down_tiled_kernel     the tiled form of the down step: a 256-thread workgroup owns 16 x 16 output pixels and stages the
 *                                   34 x 34 sources they read — rows 2 r0 - 1 .. 2 r0 + 32 and the same for columns — once, for level 1
 *                                   AFTER the bright pass, so the luma, the knee and the divide run once per source pixel.  Each
 *                                   thread then takes its 4 x 4 taps from LDS.
 * The up-and-add step and the composite have the plain form only: they read about 2.25 sources per output, which the cache serves
 * (DESIGN.md 3.30 has the measurement that left it there).
 *
 * The arithmetic is rt_bloom.h's, shared with librt_host.so: both forms call bloom_down_pixel on the same operands in the same order, so
 * they give the same bits by construction, whatever the launch geometry.  The tile walk is rt_image_kernel.h's; the stager is this
 * unit's own, because its window is of ANOTHER resolution than the tile (stage_halo maps a halo of the tile's own).  Indices are
 * clamped ONCE, while staging (bloom_source): a window entry beyond the source's edge holds the edge pixel, which is what the
 * definition's clamp reads, and the clamped index is the inside-the-image test every global read stands behind.
 *
 * The window in LDS: three planes (one per channel) of 34 rows at a pitch of 40 words, 16.3 KB, and within a row the even window columns
 * first, then the odd ones (bloom_window_at).  Why: thread (ty, tx) reads window row 2 ty + kr, column 2 tx + kc, one word at a time,
 * and one-word LDS reads are served per 32-lane half of a wave over 32 banks.  A half is two tile rows of 16 threads.  With the columns
 * as they come, the 16 threads of a tile row would read words two apart — 16 banks of ONE parity — and the other tile row of the half,
 * a whole number of rows further, 16 banks of the same parity: a two-way conflict at every pitch.  With the columns split by parity the
 * 16 threads read 16 consecutive words, and the second tile row lies 2 x 40 = 80 words further, 16 banks on (80 mod 32): the half
 * covers all 32 banks once.  Any pitch that is 8 mod 16 does that; 40 is the smallest that holds 34 columns.
 *
 * Workgroups take tiles grid-stride and every barrier stands in the workgroup-uniform tile loop.  An output word is written by one
 * thread: no atomics.  Every index into a plane is 64-bit; rows * cols < 2^32 is checked by the entry points.
 */
#include "rt_image_kernel.h"
#include "rt_bloom.h"

namespace rt {

#define RT_BLOOM_WINDOW (2u * RT_IMAGE_TILE + 2u) /* 34: two sources per output and one more either side */
#define RT_BLOOM_HALF_ROW (RT_BLOOM_WINDOW / 2u)  /* the even columns of a window row, then the odd ones */
#define RT_BLOOM_PITCH 40u

__device__ __forceinline__ uint32_t bloom_window_at(uint32_t wr, uint32_t wc) { return wr * RT_BLOOM_PITCH + (wc & 1u) * RT_BLOOM_HALF_ROW + (wc >> 1); }

/* tiles_x: tiles of 16 x 16 output pixels across the level */
__global__ __launch_bounds__(RT_IMAGE_THREADS) void bloom_down_tiled_kernel(const BloomDown d, const uint32_t tiles_x, const uint64_t n_tiles) {
    constexpr uint32_t W = RT_BLOOM_WINDOW;
    __shared__ float l_s[3][W * RT_BLOOM_PITCH];
    const auto [ty, tx] = tile_thread();
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) { /* workgroup-uniform */
        const auto [r0, c0] = tile_origin(tile, tiles_x);
        /* the window: source rows 2 r0 - 1 .. 2 r1 + 2 for the tile's last row r1 inside the level, and the same for columns */
        const int64_t r_end = r0 + (int64_t)(RT_IMAGE_TILE - 1u), c_end = c0 + (int64_t)(RT_IMAGE_TILE - 1u);
        const int64_t r1 = r_end < (int64_t)d.rows ? r_end : (int64_t)d.rows - 1, c1 = c_end < (int64_t)d.cols ? c_end : (int64_t)d.cols - 1;
        const uint32_t ny = (uint32_t)(2 * (r1 - r0) + 4), nx = (uint32_t)(2 * (c1 - c0) + 4);
        __syncthreads(); /* the previous tile's reads are done */
        for (uint32_t e = threadIdx.x; e < W * W; e += RT_IMAGE_THREADS) {
            const uint32_t wr = e / W, wc = e - wr * W;
            if (wr >= ny || wc >= nx) continue; /* no pixel of this tile looks there */
            const BloomRgb q = bloom_source(d, 2 * r0 - 1 + (int64_t)wr, 2 * c0 - 1 + (int64_t)wc);
            const uint32_t at = bloom_window_at(wr, wc);
            l_s[0][at] = q.c0, l_s[1][at] = q.c1, l_s[2][at] = q.c2;
        }
        __syncthreads();
        const int64_t r = r0 + ty, c = c0 + tx;
        if (r >= (int64_t)d.rows || c >= (int64_t)d.cols) continue; /* no barrier below */
        /* tap (kr, kc) is window entry (2 ty + kr, 2 tx + kc), inside [0, ny) x [0, nx) */
        bloom_down_pixel(d, (uint32_t)r, (uint32_t)c, [&](int kr, int kc) {
            const uint32_t at = bloom_window_at(2u * ty + (uint32_t)kr, 2u * tx + (uint32_t)kc);
            return BloomRgb{l_s[0][at], l_s[1][at], l_s[2][at]};
        });
    }
}

/* which form rt_bloom launches unless RT_AMD_BLOOM_FORM says otherwise: 0 plain, 1 tiled (same bits; DESIGN.md 3.30 has the A/B) */
#define RT_BLOOM_FORM_DEFAULT 1

static hipError_t launch_bloom(const BloomArgs &a, hipStream_t stream) {
    const bool tiled = option(OPT_BLOOM_FORM, RT_BLOOM_FORM_DEFAULT) == 1;
    hipError_t e = hipSuccess;
    bloom_steps(
        a,
        [&](const BloomDown &d) {
            e = tiled ? launch_tiles(bloom_down_tiled_kernel, d.rows, d.cols, OPT_DIAG_BLOOM_MAX_GROUPS, stream, d) : launch_each(d, OPT_DIAG_BLOOM_MAX_GROUPS, stream);
            return e == hipSuccess;
        },
        [&](const auto &op) {
            e = launch_each(op, OPT_DIAG_BLOOM_MAX_GROUPS, stream);
            return e == hipSuccess;
        });
    return e;
}

} /* namespace rt */

extern "C" {

size_t rt_bloom_temp_bytes(uint32_t rows, uint32_t cols, uint32_t n_levels) { return rt::bloom_temp_bytes(rows, cols, n_levels); }

int rt_bloom(const float *d_color, uint32_t color_stride, const rt_bloom_params *params, uint32_t rows, uint32_t cols, float *d_temp, float *d_out,
             void *hip_stream) {
    return device_query("rt_bloom", rt::BloomArgs{d_color, color_stride, params, rows, cols, d_temp, d_out}, rt::launch_bloom, hip_stream);
}

/* h_temp is not looked at: the round trip makes the scratch on the device */
int rt_bloom_host(const float *h_color, uint32_t color_stride, const rt_bloom_params *params, uint32_t rows, uint32_t cols, float *, float *h_out) {
    return host_query("rt_bloom_host", rt::BloomArgs{h_color, color_stride, params, rows, cols, nullptr, h_out}, rt::launch_bloom);
}

} /* extern "C" */
