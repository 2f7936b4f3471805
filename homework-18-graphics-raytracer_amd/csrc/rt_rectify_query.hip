/*
 * rt_rectify_query.hip — the history rectification queries (include/rt_amd.h "history rectification queries"): the colour box of every
 * pixel's neighbourhood, the temporal accumulate that clamps the reprojected history into it, and the feedback of a filtered colour
 * into the history records; kernels and entry points in one unit.
 *
 *   rt::bounds_kernel              a 256-thread workgroup owns a contiguous tile of 16 x 16 pixels and stages it with a halo of 3 once:
 *                                  22 x 22 entries of 5 words (colour, the luminance computed while staging, object), 9.7 KB of LDS.
 *                                  Of the halo only the ring the call's radius reaches is read from global memory; the entries beyond
 *                                  it are never looked at.  Each thread then walks its window twice in LDS — sums, then squared
 *                                  deviations from the mean — and writes its box as two 128-bit stores.
 *   rt::each_kernel<RectifyAccumulate>  rt_temporal_accumulate's loop with the box, two 128-bit loads more per pixel, between its
 *                                  gather and its blend: one thread per output pixel
 *   rt::each_kernel<RectifyFeedback>  one thread per record: a 128-bit load and a 128-bit store of the record's first 16 bytes
 *
 * The arithmetic is rt_rectify.h's, shared with librt_host.so; the gather of the accumulate is rt_temporal.h's.  bounds_kernel walks
 * pixel's sources in the order of the definition — dr, then dc, ascending — and calls the same functions on the same operands as the CPU
 * form, so the forms give the same bits by construction, whatever the launch geometry.  The element loop, the tile walk and the halo stager
 * are rt_image_kernel.h's.  An entry that lies outside the image or whose valid word is cleared is marked ONCE, while staging, with
 * RectifySource::none().  Entries have an odd number of words, so a tile row spreads over the LDS banks (rt_atrous_kernel.h).  Workgroups
 * take tiles grid-stride and every barrier is workgroup-uniform.  An output word is written by one thread: no atomics.  Every index into a
 * plane is 64-bit; every global read is behind an inside-the-image test; rows * cols < 2^32 is checked by the entry points.
 */
#include "rt_image_kernel.h"
#include "rt_rectify.h"

namespace rt {

#define RT_RECTIFY_HALO (RT_IMAGE_TILE + 2u * RT_RECTIFY_MAX_RADIUS)

/* tiles_x: tiles of 16 x 16 pixels across the image */
__global__ __launch_bounds__(RT_IMAGE_THREADS) void bounds_kernel(const RectifyBounds b, const uint32_t tiles_x, const uint64_t n_tiles) {
    __shared__ RectifySource l_src[RT_RECTIFY_HALO * RT_RECTIFY_HALO];
    const auto [ty, tx] = tile_thread();
    const uint32_t ring = (uint32_t)(RT_RECTIFY_MAX_RADIUS - b.radius); /* outer entries no window of this radius can reach */
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) { /* workgroup-uniform */
        const auto [r0, c0] = tile_origin(tile, tiles_x);
        __syncthreads(); /* the previous tile's reads are done */
        stage_halo<RT_RECTIFY_MAX_RADIUS>(l_src, r0, c0, b.rows, b.cols, 1, ring, RectifySource::none(), [&](uint64_t qi) { return rectify_source(b, qi); });
        __syncthreads();
        const int64_t r = r0 + ty, c = c0 + tx;
        if (r >= (int64_t)b.rows || c >= (int64_t)b.cols) continue; /* no barrier below */
        const RectifySource *centre = l_src + (ty + RT_RECTIFY_MAX_RADIUS) * RT_RECTIFY_HALO + (tx + RT_RECTIFY_MAX_RADIUS);
        float lo[4], hi[4];
        rectify_box(b, *centre, [&](int dr, int dc) { return centre[dr * (int)RT_RECTIFY_HALO + dc]; }, lo, hi);
        float4 *out = reinterpret_cast<float4 *>(b.box + ((uint64_t)r * b.cols + (uint64_t)c)); /* 32 bytes, 16-byte aligned */
        out[0] = make_float4(lo[0], lo[1], lo[2], lo[3]);
        out[1] = make_float4(hi[0], hi[1], hi[2], hi[3]);
    }
}

static hipError_t launch_box(const RectifyBoundsArgs &a, hipStream_t stream) {
    return launch_tiles(bounds_kernel, a.rows, a.cols, OPT_DIAG_RECTIFY_MAX_GROUPS, stream, a.call());
}

} /* namespace rt */

static const rt::LaunchEach<rt::OPT_DIAG_RECTIFY_MAX_GROUPS> launch_rectify;

extern "C" {

int rt_temporal_bounds(const float *d_color, uint32_t color_stride, const uint32_t *d_object, uint32_t object_stride, const uint32_t *d_valid,
                       uint32_t valid_stride, const rt_bounds_params *params, uint32_t rows, uint32_t cols, rt_temporal_box *d_box, void *hip_stream) {
    return device_query("rt_temporal_bounds", rt::RectifyBoundsArgs{d_color, color_stride, d_object, object_stride, d_valid, valid_stride, params, rows, cols, d_box},
                        rt::launch_box, hip_stream);
}

int rt_temporal_accumulate_bounded(const float *d_color, const float *d_motion, const rt_temporal_guides *current, const rt_temporal_guides *previous,
                                   const rt_temporal_params *params, uint32_t rows, uint32_t cols, const rt_temporal_pixel *d_history_in,
                                   rt_temporal_pixel *d_history_out, float *d_variance, const rt_temporal_box *d_box, uint32_t clamped_length,
                                   uint32_t *d_clamped, void *hip_stream) {
    return device_query("rt_temporal_accumulate_bounded",
                        rt::RectifyAccumulateArgs{{d_color, d_motion, current, previous, params, rows, cols, d_history_in, d_history_out, d_variance},
                                                  d_box, clamped_length, d_clamped},
                        launch_rectify, hip_stream);
}

int rt_temporal_feedback(const float *d_color, uint32_t color_stride, const uint32_t *d_valid, uint32_t valid_stride, uint32_t rows, uint32_t cols,
                         rt_temporal_pixel *d_history, void *hip_stream) {
    return device_query("rt_temporal_feedback", rt::RectifyFeedbackArgs{d_color, color_stride, d_valid, valid_stride, rows, cols, d_history}, launch_rectify,
                        hip_stream);
}

int rt_temporal_bounds_host(const float *h_color, uint32_t color_stride, const uint32_t *h_object, uint32_t object_stride, const uint32_t *h_valid,
                            uint32_t valid_stride, const rt_bounds_params *params, uint32_t rows, uint32_t cols, rt_temporal_box *h_box) {
    return host_query("rt_temporal_bounds_host", rt::RectifyBoundsArgs{h_color, color_stride, h_object, object_stride, h_valid, valid_stride, params, rows, cols, h_box},
                      rt::launch_box);
}

int rt_temporal_accumulate_bounded_host(const float *h_color, const float *h_motion, const rt_temporal_guides *current, const rt_temporal_guides *previous,
                                        const rt_temporal_params *params, uint32_t rows, uint32_t cols, const rt_temporal_pixel *h_history_in,
                                        rt_temporal_pixel *h_history_out, float *h_variance, const rt_temporal_box *h_box, uint32_t clamped_length,
                                        uint32_t *h_clamped) {
    return host_query("rt_temporal_accumulate_bounded_host",
                      rt::RectifyAccumulateArgs{{h_color, h_motion, current, previous, params, rows, cols, h_history_in, h_history_out, h_variance},
                                                h_box, clamped_length, h_clamped},
                      launch_rectify);
}

int rt_temporal_feedback_host(const float *h_color, uint32_t color_stride, const uint32_t *h_valid, uint32_t valid_stride, uint32_t rows, uint32_t cols,
                              rt_temporal_pixel *h_history) {
    return host_query("rt_temporal_feedback_host", rt::RectifyFeedbackArgs{h_color, color_stride, h_valid, valid_stride, rows, cols, h_history}, launch_rectify);
}

} /* extern "C" */

