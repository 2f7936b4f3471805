/*
 * rt_denoise_query.hip — the denoise queries (include/rt_amd.h "denoise queries"): the edge-avoiding A-Trous filter, one launch per level,
 * kernels and entry points in one unit.
 *
 *   rt::each_kernel<AtrousEach<DenoiseFilter>>  the simple form
 *   rt::atrous_tiled_kernel<DenoiseFilter>      the tiled form: 400 staged entries of 9 words, 14.4 KB of LDS
 *
 * The kernels are rt_atrous_kernel.h's, which says what they do and why they agree bit for bit; the arithmetic is rt_denoise.h's
 * DenoiseFilter, shared with librt_host.so.  The temp plane is one colour plane.
 */
#include "rt_api_internal.h"
#include "rt_atrous_kernel.h"
#include "rt_denoise.h"

/* which form rt_denoise_atrous launches unless RT_AMD_DENOISE_FORM says otherwise: 0 simple, 1 tiled — the tiled one, which the
 * measurement at 1920 x 1080 chose: far ahead on guides read through record strides, level on compact ones (DESIGN.md 3.21 has the
 * figures and the bar) */
#define RT_DENOISE_FORM_DEFAULT 1

namespace rt {

static hipError_t launch_denoise(const DenoiseArgs &a, hipStream_t stream) {
    return launch_atrous<DenoiseFilter>(a, option(OPT_DENOISE_FORM, RT_DENOISE_FORM_DEFAULT) == 1, OPT_DIAG_DENOISE_MAX_GROUPS, stream);
}

} /* namespace rt */

extern "C" {

size_t rt_denoise_temp_bytes(uint32_t rows, uint32_t cols) { return (size_t)rows * cols * 3u * sizeof(float); }

int rt_denoise_atrous(const float *d_color, const rt_denoise_guides *guides, const rt_denoise_params *params, uint32_t rows, uint32_t cols,
                      float *d_out, float *d_temp, void *hip_stream) {
    return device_query("rt_denoise_atrous", rt::DenoiseArgs{d_color, guides, params, rows, cols, d_out, d_temp}, rt::launch_denoise, hip_stream);
}

int rt_denoise_atrous_host(const float *h_color, const rt_denoise_guides *guides, const rt_denoise_params *params, uint32_t rows, uint32_t cols,
                           float *h_out) {
    return host_query("rt_denoise_atrous_host", rt::DenoiseArgs{h_color, guides, params, rows, cols, h_out, nullptr}, rt::launch_denoise);
}

} /* extern "C" */
