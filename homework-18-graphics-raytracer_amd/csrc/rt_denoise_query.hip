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

static hipError_t launch_denoise(const float *color, const rt_denoise_guides &g, const rt_denoise_params &p, uint32_t rows, uint32_t cols, float *out, float *temp,
                                 hipStream_t stream) {
    return launch_atrous<DenoiseFilter>(p.n_levels, option(OPT_DENOISE_FORM, RT_DENOISE_FORM_DEFAULT) == 1, OPT_DIAG_DENOISE_MAX_GROUPS, stream,
                                        [&](uint32_t j) { return denoise_level(color, g, p, rows, cols, out, temp, j); });
}

} /* namespace rt */

extern "C" {

size_t rt_denoise_temp_bytes(uint32_t rows, uint32_t cols) { return (size_t)rows * cols * 3u * sizeof(float); }

int rt_denoise_atrous(const float *d_color, const rt_denoise_guides *guides, const rt_denoise_params *params, uint32_t rows, uint32_t cols,
                      float *d_out, float *d_temp, void *hip_stream) {
    const char *bad = rt::denoise_limits(d_color, guides, params, rows, cols, d_out, d_temp, true);
    if (bad) return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_denoise_atrous: ") + bad);
    if (rows == 0u || cols == 0u) return RT_OK;
    return launched("rt_denoise_atrous", rt::launch_denoise(d_color, *guides, *params, rows, cols, d_out, d_temp, static_cast<hipStream_t>(hip_stream)));
}

int rt_denoise_atrous_host(const float *h_color, const rt_denoise_guides *guides, const rt_denoise_params *params, uint32_t rows, uint32_t cols,
                           float *h_out) {
    const char *bad = rt::denoise_limits(h_color, guides, params, rows, cols, h_out, nullptr, false);
    if (bad) return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_denoise_atrous_host: ") + bad);
    if (rows == 0u || cols == 0u) return RT_OK;
    const size_t n = (size_t)rows * cols, plane = n * 3u * sizeof(float);
    HostRoundTrip t("rt_denoise_atrous_host");
    const float *d_color = t.in(h_color, plane);
    const rt_denoise_guides g = t.guides(*guides, n);
    float *d_out = t.out(h_out, plane);
    float *d_temp = params->n_levels >= 2u ? static_cast<float *>(t.scratch(plane)) : nullptr;
    if (!t.ok()) return t.failed();
    const hipError_t e = rt::launch_denoise(d_color, g, *params, rows, cols, d_out, d_temp, nullptr);
    if (e != hipSuccess) return launched("rt_denoise_atrous_host", e);
    return t.finish();
}

} /* extern "C" */
