/*
 * rt_svgf_query.hip — the variance-guided filter queries (include/rt_amd.h "variance-guided filter queries"): the variance estimate
 * for every history length and the variance-guided A-Trous filter, one launch per level; kernels and entry points in one unit.
 *
 *   rt::svgf_variance_kernel  a 256-thread workgroup owns a contiguous tile of 16 x 16 pixels.  Each thread reads its own record first;
 *                             whether ANY pixel of the tile has a history shorter than min_length is decided for the whole workgroup
 *                             (__syncthreads_or).  A tile without one — after a few frames most of the image — writes steps 1 and 2
 *                             and stages nothing.  Otherwise the tile and its halo of 3, 22 x 22 entries of 9 words (17.4 KB of LDS),
 *                             are staged once and the short pixels walk their 49 taps there.
 *   rt::each_kernel<AtrousEach<SvgfFilter>>  the A-Trous level, simple form
 *   rt::atrous_tiled_kernel<SvgfFilter>  the A-Trous level, tiled form: 400 staged entries of 11 words (the colour as seen, its
 *                             luminance, the variance through vpos, normal, position), 17.6 KB of LDS at every level.  The 3 x 3
 *                             prefilter of the variance concerns the output pixel alone and its neighbours lie at step 1, not in the
 *                             residue class: each thread reads it from global memory.
 *
 * The A-Trous kernels are rt_atrous_kernel.h's, which says what they do and why they agree bit for bit.  The variance kernel is this unit's
 * own from its early leave on; its tile walk, halo stager and launch are rt_image_kernel.h's.  The arithmetic is rt_svgf.h's, shared with
 * librt_host.so.  Every kernel walks a pixel's sources in the order of the definition — dr, then dc, ascending — and calls the same
 * functions on the same operands, so the forms give the same bits as each other and as the CPU forms by construction, whatever the launch
 * geometry.  An output word is written by one thread: no atomics.  A staged entry of the variance tile that lies outside the image or whose
 * valid word is cleared is marked ONCE, while staging, by length 0, which the definition skips anyway.  Entries have an odd number of
 * words, so a tile row spreads over the LDS banks.  Guides are read through their record strides where they lie.  Every index into a plane
 * is 64-bit; every read is behind an inside-the-image test; rows * cols < 2^32 is checked by the entry point.
 */
#include "rt_api_internal.h"
#include "rt_atrous_kernel.h"
#include "rt_svgf.h"

/* which form rt_svgf_atrous launches unless RT_AMD_SVGF_FORM says otherwise: 0 simple, 1 tiled (DESIGN.md 3.23 has the reasons) */
#define RT_SVGF_FORM_DEFAULT 1

namespace rt {

#define RT_SVGF_VARIANCE_HALO (RT_IMAGE_TILE + 2u * RT_SVGF_VARIANCE_REACH)

/* tiles_x: tiles of 16 x 16 pixels across the image.  Workgroups take tiles grid-stride; `any_short` is the same in every thread of the
 * workgroup, so every thread meets the same barriers.  The __syncthreads_or at the top of a tile is also what separates the previous
 * tile's reads of l_pix from this tile's writes. */
__global__ __launch_bounds__(RT_IMAGE_THREADS) void svgf_variance_kernel(const SvgfVariance v, const uint32_t tiles_x, const uint64_t n_tiles) {
    __shared__ SvgfMoments l_pix[RT_SVGF_VARIANCE_HALO * RT_SVGF_VARIANCE_HALO];
    const auto [ty, tx] = tile_thread();
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) { /* workgroup-uniform */
        const auto [r0, c0] = tile_origin(tile, tiles_x);
        const int64_t r = r0 + ty, c = c0 + tx;
        const bool inside = r < (int64_t)v.rows && c < (int64_t)v.cols;
        const uint64_t i = inside ? (uint64_t)r * v.cols + (uint64_t)c : 0u;
        SvgfMoments p = {0.0f, 0.0f, 0u, {}};
        if (inside) p = svgf_moments_load(v, i);
        const bool is_short = inside && svgf_moments_short(v, p);
        const int any_short = __syncthreads_or(is_short ? 1 : 0);
        if (!any_short) {
            if (inside) v.out[i] = svgf_variance_temporal(p);
            continue;
        }
        stage_halo<RT_SVGF_VARIANCE_REACH>(l_pix, r0, c0, v.rows, v.cols, 1, 0u, SvgfMoments{0.0f, 0.0f, 0u, {}} /* length 0 */,
                                           [&](uint64_t qi) { return svgf_moments_load(v, qi); });
        __syncthreads();
        if (!inside) continue; /* no barrier below */
        float out = svgf_variance_temporal(p);
        if (is_short) {
            SvgfMomentSums a = {0.0f, 0.0f, 0.0f};
            for (int dr = -RT_SVGF_VARIANCE_REACH; dr <= RT_SVGF_VARIANCE_REACH; ++dr)
                for (int dc = -RT_SVGF_VARIANCE_REACH; dc <= RT_SVGF_VARIANCE_REACH; ++dc)
                    svgf_variance_tap(v, a, p, l_pix[(uint32_t)((int)ty + RT_SVGF_VARIANCE_REACH + dr) * RT_SVGF_VARIANCE_HALO + (uint32_t)((int)tx + RT_SVGF_VARIANCE_REACH + dc)]);
            out = svgf_variance_spatial(v, p, a);
        }
        v.out[i] = out;
    }
}

static hipError_t launch_svgf_variance(const SvgfVarianceArgs &a, hipStream_t stream) {
    return launch_tiles(svgf_variance_kernel, a.rows, a.cols, OPT_DIAG_SVGF_MAX_GROUPS, stream, a.call());
}

static hipError_t launch_svgf(const SvgfAtrousArgs &a, hipStream_t stream) {
    return launch_atrous<SvgfFilter>(a, option(OPT_SVGF_FORM, RT_SVGF_FORM_DEFAULT) == 1, OPT_DIAG_SVGF_MAX_GROUPS, stream);
}

} /* namespace rt */

extern "C" {

size_t rt_svgf_temp_bytes(uint32_t rows, uint32_t cols, uint32_t n_levels) { return (size_t)rows * cols * rt::svgf_temp_words(n_levels) * sizeof(float); }

int rt_svgf_variance(const rt_temporal_pixel *d_history, const rt_denoise_guides *guides, const rt_svgf_variance_params *params, uint32_t rows,
                     uint32_t cols, float *d_variance_out, void *hip_stream) {
    return device_query("rt_svgf_variance", rt::SvgfVarianceArgs{d_history, guides, params, rows, cols, d_variance_out}, rt::launch_svgf_variance, hip_stream);
}

int rt_svgf_atrous(const float *d_color, uint32_t color_stride, const float *d_variance, const rt_denoise_guides *guides,
                   const rt_svgf_atrous_params *params, uint32_t rows, uint32_t cols, float *d_out, float *d_variance_out, void *d_temp,
                   void *hip_stream) {
    return device_query("rt_svgf_atrous",
                        rt::SvgfAtrousArgs{d_color, color_stride, d_variance, guides, params, rows, cols, d_out, d_variance_out, static_cast<float *>(d_temp)},
                        rt::launch_svgf, hip_stream);
}

int rt_svgf_variance_host(const rt_temporal_pixel *h_history, const rt_denoise_guides *guides, const rt_svgf_variance_params *params, uint32_t rows,
                          uint32_t cols, float *h_variance_out) {
    return host_query("rt_svgf_variance_host", rt::SvgfVarianceArgs{h_history, guides, params, rows, cols, h_variance_out}, rt::launch_svgf_variance);
}

int rt_svgf_atrous_host(const float *h_color, uint32_t color_stride, const float *h_variance, const rt_denoise_guides *guides,
                        const rt_svgf_atrous_params *params, uint32_t rows, uint32_t cols, float *h_out, float *h_variance_out) {
    return host_query("rt_svgf_atrous_host", rt::SvgfAtrousArgs{h_color, color_stride, h_variance, guides, params, rows, cols, h_out, h_variance_out, nullptr},
                      rt::launch_svgf);
}

} /* extern "C" */

