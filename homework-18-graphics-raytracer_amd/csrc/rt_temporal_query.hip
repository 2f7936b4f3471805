/*
 * rt_temporal_query.hip — the temporal queries (include/rt_amd.h "temporal queries"): where each pixel's surface point was in the previous
 * frame, and the previous frame's history gathered from there and blended with the current frame; kernels and entry points in one unit.
 *
 *   rt::each_kernel<TemporalMotion>  one thread per pixel: the seven steps of the projection
 *   rt::each_kernel<TemporalCall>    one thread per output pixel: a data-dependent 2 x 2 gather over the previous frame
 * (rt_image_kernel.h has the element loop and its launch)
 *
 * The arithmetic is rt_temporal.h's, shared with librt_host.so: the kernels call temporal_project / temporal_pixel on the same operands
 * as rt_temporal_motion_cpu / rt_temporal_accumulate_cpu, so they give the same bits by construction, whatever the launch geometry.
 * The gather is bound by memory latency: temporal_pixel reads all four taps — each history record as two 128-bit loads, then the
 * guide words — before the first test that depends on one, so up to four records and their guides are in flight per thread.  An
 * output pixel is written by one thread (two 128-bit stores): no atomics, no LDS.  Every index into a plane is 64-bit; every read of
 * the previous frame is behind its inside-the-image test; rows * cols < 2^32 is checked by the entry point.
 */
#include "rt_image_kernel.h"
#include "rt_temporal.h"

static const rt::LaunchEach<rt::OPT_DIAG_TEMPORAL_MAX_GROUPS> launch_temporal;

extern "C" {

int rt_temporal_motion(const float *d_position, uint32_t position_stride, const uint32_t *d_valid, uint32_t valid_stride, const rt_camera *prev_camera,
                       const rt_frame *prev_frame, float *d_motion, void *hip_stream) {
    return device_query("rt_temporal_motion", rt::TemporalMotionArgs{d_position, position_stride, d_valid, valid_stride, prev_camera, prev_frame, d_motion},
                        launch_temporal, hip_stream);
}

int rt_temporal_accumulate(const float *d_color, const float *d_motion, const rt_temporal_guides *current, const rt_temporal_guides *previous,
                           const rt_temporal_params *params, uint32_t rows, uint32_t cols, const rt_temporal_pixel *d_history_in,
                           rt_temporal_pixel *d_history_out, float *d_variance, void *hip_stream) {
    return device_query("rt_temporal_accumulate",
                        rt::TemporalAccumulateArgs{d_color, d_motion, current, previous, params, rows, cols, d_history_in, d_history_out, d_variance},
                        launch_temporal, hip_stream);
}

int rt_temporal_motion_host(const float *h_position, uint32_t position_stride, const uint32_t *h_valid, uint32_t valid_stride, const rt_camera *prev_camera,
                            const rt_frame *prev_frame, float *h_motion) {
    return host_query("rt_temporal_motion_host", rt::TemporalMotionArgs{h_position, position_stride, h_valid, valid_stride, prev_camera, prev_frame, h_motion},
                      launch_temporal);
}

int rt_temporal_accumulate_host(const float *h_color, const float *h_motion, const rt_temporal_guides *current, const rt_temporal_guides *previous,
                                const rt_temporal_params *params, uint32_t rows, uint32_t cols, const rt_temporal_pixel *h_history_in,
                                rt_temporal_pixel *h_history_out, float *h_variance) {
    return host_query("rt_temporal_accumulate_host",
                      rt::TemporalAccumulateArgs{h_color, h_motion, current, previous, params, rows, cols, h_history_in, h_history_out, h_variance},
                      launch_temporal);
}

} /* extern "C" */

