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

namespace rt {

static hipError_t launch_motion(const float *position, uint32_t position_stride, const uint32_t *valid, uint32_t valid_stride, const rt_camera *camera,
                                const rt_frame *frame, float *motion, hipStream_t stream) {
    TemporalMotion m;
    m.cam = temporal_camera(camera, frame);
    m.position = position, m.valid = valid, m.position_stride = position_stride, m.valid_stride = valid_stride, m.motion = motion;
    m.n = (uint64_t)frame->width * frame->height;
    return launch_each(m, OPT_DIAG_TEMPORAL_MAX_GROUPS, stream);
}

static hipError_t launch_accumulate(const TemporalCall &t, hipStream_t stream) { return launch_each(t, OPT_DIAG_TEMPORAL_MAX_GROUPS, stream); }

} /* namespace rt */

extern "C" {

int rt_temporal_motion(const float *d_position, uint32_t position_stride, const uint32_t *d_valid, uint32_t valid_stride, const rt_camera *prev_camera,
                       const rt_frame *prev_frame, float *d_motion, void *hip_stream) {
    int status;
    const char *bad = rt::temporal_motion_limits(d_position, position_stride, d_valid, valid_stride, prev_camera, prev_frame, d_motion, &status);
    if (bad) return fail(status, std::string("rt_temporal_motion: ") + bad);
    if (prev_frame->width == 0u || prev_frame->height == 0u) return RT_OK;
    return launched("rt_temporal_motion", rt::launch_motion(d_position, position_stride, d_valid, valid_stride, prev_camera, prev_frame, d_motion,
                                                            static_cast<hipStream_t>(hip_stream)));
}

int rt_temporal_accumulate(const float *d_color, const float *d_motion, const rt_temporal_guides *current, const rt_temporal_guides *previous,
                           const rt_temporal_params *params, uint32_t rows, uint32_t cols, const rt_temporal_pixel *d_history_in,
                           rt_temporal_pixel *d_history_out, float *d_variance, void *hip_stream) {
    int status;
    const char *bad = rt::temporal_limits(d_color, d_motion, current, previous, params, rows, cols, d_history_in, d_history_out, true, &status);
    if (bad) return fail(status, std::string("rt_temporal_accumulate: ") + bad);
    if (rows == 0u || cols == 0u) return RT_OK;
    return launched("rt_temporal_accumulate",
                    rt::launch_accumulate(rt::temporal_call(d_color, d_motion, *current, *previous, *params, rows, cols, d_history_in, d_history_out, d_variance),
                                          static_cast<hipStream_t>(hip_stream)));
}

int rt_temporal_motion_host(const float *h_position, uint32_t position_stride, const uint32_t *h_valid, uint32_t valid_stride, const rt_camera *prev_camera,
                            const rt_frame *prev_frame, float *h_motion) {
    int status;
    const char *bad = rt::temporal_motion_limits(h_position, position_stride, h_valid, valid_stride, prev_camera, prev_frame, h_motion, &status);
    if (bad) return fail(status, std::string("rt_temporal_motion_host: ") + bad);
    if (prev_frame->width == 0u || prev_frame->height == 0u) return RT_OK;
    const size_t n = (size_t)prev_frame->width * prev_frame->height;
    HostRoundTrip t("rt_temporal_motion_host");
    const float *d_position = t.plane(h_position, n, position_stride, 3u);
    const uint32_t *d_valid = t.plane(h_valid, n, valid_stride, 1u);
    float *d_motion = t.out(h_motion, n * 2u * sizeof(float));
    if (!t.ok()) return t.failed();
    const hipError_t e = rt::launch_motion(d_position, position_stride, d_valid, valid_stride, prev_camera, prev_frame, d_motion, nullptr);
    if (e != hipSuccess) return launched("rt_temporal_motion_host", e);
    return t.finish();
}

int rt_temporal_accumulate_host(const float *h_color, const float *h_motion, const rt_temporal_guides *current, const rt_temporal_guides *previous,
                                const rt_temporal_params *params, uint32_t rows, uint32_t cols, const rt_temporal_pixel *h_history_in,
                                rt_temporal_pixel *h_history_out, float *h_variance) {
    int status;
    /* the device copies are hipMalloc's and aligned whatever the host arrays are */
    const char *bad = rt::temporal_limits(h_color, h_motion, current, previous, params, rows, cols, h_history_in, h_history_out, false, &status);
    if (bad) return fail(status, std::string("rt_temporal_accumulate_host: ") + bad);
    if (rows == 0u || cols == 0u) return RT_OK;
    const size_t n = (size_t)rows * cols;
    HostRoundTrip t("rt_temporal_accumulate_host");
    const float *d_color = t.in(h_color, n * 3u * sizeof(float));
    const float *d_motion = t.in(h_motion, n * 2u * sizeof(float));
    const rt_temporal_guides cur = t.temporal_guides(*current, n), prev = t.temporal_guides(*previous, n);
    const rt_temporal_pixel *d_in = t.in(h_history_in, n * sizeof(rt_temporal_pixel));
    rt_temporal_pixel *d_out = t.out(h_history_out, n * sizeof(rt_temporal_pixel));
    float *d_variance = t.out(h_variance, n * sizeof(float));
    if (!t.ok()) return t.failed();
    const hipError_t e = rt::launch_accumulate(rt::temporal_call(d_color, d_motion, cur, prev, *params, rows, cols, d_in, d_out, d_variance), nullptr);
    if (e != hipSuccess) return launched("rt_temporal_accumulate_host", e);
    return t.finish();
}

} /* extern "C" */
