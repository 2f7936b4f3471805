/*
 * rt_svgf_query.hip — the variance-guided filter queries (include/rt_amd.h "variance-guided filter queries"): the variance estimate
 * for every history length and the variance-guided A-Trous filter, one launch per level; kernels and entry points in one unit.
 *
 *   rt::svgf_variance_kernel  a 256-thread workgroup owns a contiguous tile of 16 x 16 pixels.  Each thread reads its own record first;
 *                             whether ANY pixel of the tile has a history shorter than min_length is decided for the whole workgroup
 *                             (__syncthreads_or).  A tile without one — after a few frames most of the image — writes steps 1 and 2
 *                             and stages nothing.  Otherwise the tile and its halo of 3, 22 x 22 entries of 9 words (17.4 KB of LDS),
 *                             are staged once and the short pixels walk their 49 taps there.
 *   rt::svgf_kernel           the A-Trous level, simple form: one thread per output pixel, grid-stride; the 25 sources from global memory
 *   rt::svgf_tiled_kernel     the A-Trous level, tiled form: denoise_tiled_kernel's residue-class tile — 16 x 16 outputs SPACED step
 *                             APART, 20 x 20 staged entries also step apart — with entries of 11 words (the colour as seen, its
 *                             luminance, the variance through vpos, normal, position): 17.6 KB of LDS at every level.  The 3 x 3
 *                             prefilter of the variance concerns the output pixel alone and its neighbours lie at step 1, not in the
 *                             residue class: each thread reads it from global memory.
 *
 * The arithmetic is rt_svgf.h's, shared with librt_host.so.  Every kernel walks a pixel's sources in the order of the definition — dr,
 * then dc, ascending — and calls the same functions on the same operands, so the forms give the same bits as each other and as the
 * CPU forms by construction, whatever the launch geometry.  An output word is written by one thread: no atomics.  A staged entry that
 * lies outside the image or whose valid word is cleared is marked ONCE, while staging: in the A-Trous tile by a NaN colour and
 * luminance (its exponent is NaN and svgf_tap skips it, as it skips a caller's own NaN colour; an output pixel whose own entry is so
 * marked collects no weight and passes through), in the variance tile by length 0, which the definition skips anyway.  Entries have an
 * odd number of words, so a tile row spreads over the LDS banks.  Guides are read through their record strides where they lie.  Every
 * index into a plane is 64-bit; every read is behind an inside-the-image test; rows * cols < 2^32 is checked by the entry point.
 */
#include "rt_api_internal.h"
#include "rt_svgf.h"

/* which form rt_svgf_atrous launches unless RT_AMD_SVGF_FORM says otherwise: 0 simple, 1 tiled (DESIGN.md 3.23 has the reasons) */
#define RT_SVGF_FORM_DEFAULT 1

namespace rt {

#define RT_SVGF_THREADS 256u
#define RT_SVGF_TILE 16u
#define RT_SVGF_HALO (RT_SVGF_TILE + 4u)                                    /* the A-Trous tile: two taps either side */
#define RT_SVGF_VARIANCE_HALO (RT_SVGF_TILE + 2u * RT_SVGF_VARIANCE_REACH) /* the variance tile: three pixels either side */
#define RT_SVGF_MAX_GROUPS (1u << 16)

/* tiles_x: tiles of 16 x 16 pixels across the image.  Workgroups take tiles grid-stride; `any_short` is the same in every thread of the
 * workgroup, so every thread meets the same barriers.  The __syncthreads_or at the top of a tile is also what separates the previous
 * tile's reads of l_pix from this tile's writes. */
__global__ __launch_bounds__(RT_SVGF_THREADS) void svgf_variance_kernel(const SvgfVariance v, const uint32_t tiles_x, const uint64_t n_tiles) {
    __shared__ SvgfMoments l_pix[RT_SVGF_VARIANCE_HALO * RT_SVGF_VARIANCE_HALO];
    const uint32_t ty = threadIdx.x / RT_SVGF_TILE, tx = threadIdx.x % RT_SVGF_TILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) { /* workgroup-uniform */
        const uint32_t tile_r = (uint32_t)(tile / tiles_x), tile_c = (uint32_t)(tile - (uint64_t)tile_r * tiles_x);
        const int64_t r0 = (int64_t)tile_r * RT_SVGF_TILE, c0 = (int64_t)tile_c * RT_SVGF_TILE;
        const int64_t r = r0 + ty, c = c0 + tx;
        const bool inside = r < (int64_t)v.rows && c < (int64_t)v.cols;
        const uint64_t i = inside ? (uint64_t)r * v.cols + (uint64_t)c : 0u;
        SvgfMoments p = {0.0f, 0.0f, 0u, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (inside) p = svgf_moments_load(v, i);
        const bool is_short = inside && svgf_moments_short(v, p);
        const int any_short = __syncthreads_or(is_short ? 1 : 0);
        if (!any_short) {
            if (inside) v.out[i] = svgf_variance_temporal(p);
            continue;
        }
        for (uint32_t e = threadIdx.x; e < RT_SVGF_VARIANCE_HALO * RT_SVGF_VARIANCE_HALO; e += RT_SVGF_THREADS) {
            const uint32_t hr = e / RT_SVGF_VARIANCE_HALO, hc = e - hr * RT_SVGF_VARIANCE_HALO;
            const int64_t qr = r0 + (int64_t)hr - RT_SVGF_VARIANCE_REACH, qc = c0 + (int64_t)hc - RT_SVGF_VARIANCE_REACH;
            SvgfMoments q = {0.0f, 0.0f, 0u, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}; /* length 0: a source of nobody */
            if (qr >= 0 && qr < (int64_t)v.rows && qc >= 0 && qc < (int64_t)v.cols) q = svgf_moments_load(v, (uint64_t)qr * v.cols + (uint64_t)qc);
            l_pix[e] = q;
        }
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

__global__ __launch_bounds__(RT_SVGF_THREADS) void svgf_kernel(const SvgfLevel L) {
    const uint64_t n = (uint64_t)L.rows * L.cols, stride = (uint64_t)gridDim.x * RT_SVGF_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * RT_SVGF_THREADS + threadIdx.x; i < n; i += stride) {
        const uint32_t r = (uint32_t)(i / L.cols), c = (uint32_t)(i - (uint64_t)r * L.cols);
        svgf_pixel(L, r, c);
    }
}

/* blocks_x: blocks of 16 step x 16 step pixels across the image; n_tiles = blocks * step * step, block-major, then the residue's row, then
 * its column.  Workgroups take tiles grid-stride, so every thread of a workgroup meets the same barriers. */
__global__ __launch_bounds__(RT_SVGF_THREADS) void svgf_tiled_kernel(const SvgfLevel L, const uint32_t blocks_x, const uint64_t n_tiles) {
    __shared__ SvgfPix l_pix[RT_SVGF_HALO * RT_SVGF_HALO];
    const int64_t step = L.step;
    const uint32_t per_block = (uint32_t)(L.step * L.step);
    const uint32_t ty = threadIdx.x / RT_SVGF_TILE, tx = threadIdx.x % RT_SVGF_TILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) { /* workgroup-uniform */
        const uint64_t block = tile / per_block;
        const uint32_t res = (uint32_t)(tile - block * per_block);
        const uint32_t block_r = (uint32_t)(block / blocks_x), block_c = (uint32_t)(block - (uint64_t)block_r * blocks_x);
        const int64_t r0 = (int64_t)block_r * RT_SVGF_TILE * step + res / (uint32_t)L.step;
        const int64_t c0 = (int64_t)block_c * RT_SVGF_TILE * step + res % (uint32_t)L.step;
        if (r0 >= (int64_t)L.rows || c0 >= (int64_t)L.cols) continue; /* a residue class the image's last block does not reach: uniform */
        __syncthreads(); /* the previous tile's reads are done */
        for (uint32_t e = threadIdx.x; e < RT_SVGF_HALO * RT_SVGF_HALO; e += RT_SVGF_THREADS) {
            const uint32_t hr = e / RT_SVGF_HALO, hc = e - hr * RT_SVGF_HALO;
            const int64_t qr = r0 + ((int64_t)hr - 2) * step, qc = c0 + ((int64_t)hc - 2) * step;
            const float nan = __uint_as_float(0x7fc00000u);
            SvgfPix q = {nan, 0.0f, 0.0f, nan, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}; /* NaN colour and luminance: a source of nobody */
            if (qr >= 0 && qr < (int64_t)L.rows && qc >= 0 && qc < (int64_t)L.cols) {
                const uint64_t qi = (uint64_t)qr * L.cols + (uint64_t)qc;
                if (svgf_valid(L, qi)) q = svgf_load(L, qi);
            }
            l_pix[e] = q;
        }
        __syncthreads();
        const int64_t r = r0 + (int64_t)ty * step, c = c0 + (int64_t)tx * step;
        if (r < (int64_t)L.rows && c < (int64_t)L.cols) {
            const SvgfPix p = l_pix[(ty + 2u) * RT_SVGF_HALO + (tx + 2u)];
            SvgfAcc a = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if (p.lum == p.lum) { /* a NaN luminance — marked, or the caller's own — takes no tap: it needs no sigma */
                const float sl = svgf_sigma_luminance(L, (uint32_t)r, (uint32_t)c);
                for (int dr = -2; dr <= 2; ++dr)
                    for (int dc = -2; dc <= 2; ++dc) svgf_tap(L, a, p, l_pix[(uint32_t)((int)ty + 2 + dr) * RT_SVGF_HALO + (uint32_t)((int)tx + 2 + dc)], sl, dr, dc);
            }
            svgf_store(L, (uint64_t)r * L.cols + (uint64_t)c, true, a);
        }
    }
}

static uint32_t svgf_max_groups() {
    const long long cap = option(OPT_DIAG_SVGF_MAX_GROUPS, RT_SVGF_MAX_GROUPS); /* test hook: fewer workgroups, so a small image is taken grid-stride */
    return cap >= 1 && cap < (long long)RT_SVGF_MAX_GROUPS ? (uint32_t)cap : RT_SVGF_MAX_GROUPS;
}

static hipError_t launch_svgf_variance(const SvgfVariance &v, hipStream_t stream) {
    const uint32_t tiles_x = (v.cols + RT_SVGF_TILE - 1u) / RT_SVGF_TILE, tiles_y = (v.rows + RT_SVGF_TILE - 1u) / RT_SVGF_TILE;
    const uint64_t n_tiles = (uint64_t)tiles_x * tiles_y;
    hipLaunchKernelGGL(svgf_variance_kernel, dim3((uint32_t)std::min<uint64_t>(n_tiles, svgf_max_groups())), dim3(RT_SVGF_THREADS), 0, stream, v, tiles_x, n_tiles);
    return hipGetLastError();
}

static hipError_t launch_svgf_level(const SvgfLevel &L, bool tiled, uint32_t max_groups, hipStream_t stream) {
    if (tiled) {
        const uint64_t side = (uint64_t)RT_SVGF_TILE * (uint64_t)L.step;
        const uint32_t blocks_x = (uint32_t)((L.cols + side - 1u) / side), blocks_y = (uint32_t)((L.rows + side - 1u) / side);
        const uint64_t n_tiles = (uint64_t)blocks_x * blocks_y * (uint64_t)L.step * (uint64_t)L.step;
        hipLaunchKernelGGL(svgf_tiled_kernel, dim3((uint32_t)std::min<uint64_t>(n_tiles, max_groups)), dim3(RT_SVGF_THREADS), 0, stream, L, blocks_x, n_tiles);
    } else {
        const uint64_t groups = ((uint64_t)L.rows * L.cols + RT_SVGF_THREADS - 1u) / RT_SVGF_THREADS;
        hipLaunchKernelGGL(svgf_kernel, dim3((uint32_t)std::min<uint64_t>(groups, max_groups)), dim3(RT_SVGF_THREADS), 0, stream, L);
    }
    return hipGetLastError();
}

static hipError_t launch_svgf(const float *color, uint32_t color_stride, const float *variance, const rt_denoise_guides &g, const rt_svgf_atrous_params &p,
                              uint32_t rows, uint32_t cols, float *out, float *variance_out, float *temp, hipStream_t stream) {
    const bool tiled = option(OPT_SVGF_FORM, RT_SVGF_FORM_DEFAULT) == 1;
    const uint32_t max_groups = svgf_max_groups();
    for (uint32_t j = 0; j < p.n_levels; ++j) {
        const hipError_t e = launch_svgf_level(svgf_level(color, color_stride, variance, g, p, rows, cols, out, variance_out, temp, j), tiled, max_groups, stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} /* namespace rt */

extern "C" {

size_t rt_svgf_temp_bytes(uint32_t rows, uint32_t cols, uint32_t n_levels) { return (size_t)rows * cols * rt::svgf_temp_words(n_levels) * sizeof(float); }

int rt_svgf_variance(const rt_temporal_pixel *d_history, const rt_denoise_guides *guides, const rt_svgf_variance_params *params, uint32_t rows,
                     uint32_t cols, float *d_variance_out, void *hip_stream) {
    const char *bad = rt::svgf_variance_limits(d_history, guides, params, rows, cols, d_variance_out, true);
    if (bad) return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_svgf_variance: ") + bad);
    if (rows == 0u || cols == 0u) return RT_OK;
    return launched("rt_svgf_variance",
                    rt::launch_svgf_variance(rt::svgf_variance_call(d_history, *guides, *params, rows, cols, d_variance_out), static_cast<hipStream_t>(hip_stream)));
}

int rt_svgf_atrous(const float *d_color, uint32_t color_stride, const float *d_variance, const rt_denoise_guides *guides,
                   const rt_svgf_atrous_params *params, uint32_t rows, uint32_t cols, float *d_out, float *d_variance_out, void *d_temp,
                   void *hip_stream) {
    const char *bad = rt::svgf_atrous_limits(d_color, color_stride, d_variance, guides, params, rows, cols, d_out, d_variance_out, static_cast<float *>(d_temp), true);
    if (bad) return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_svgf_atrous: ") + bad);
    if (rows == 0u || cols == 0u) return RT_OK;
    return launched("rt_svgf_atrous", rt::launch_svgf(d_color, color_stride, d_variance, *guides, *params, rows, cols, d_out, d_variance_out,
                                                      static_cast<float *>(d_temp), static_cast<hipStream_t>(hip_stream)));
}

int rt_svgf_variance_host(const rt_temporal_pixel *h_history, const rt_denoise_guides *guides, const rt_svgf_variance_params *params, uint32_t rows,
                          uint32_t cols, float *h_variance_out) {
    /* the device copy is hipMalloc's and aligned whatever the host array is */
    const char *bad = rt::svgf_variance_limits(h_history, guides, params, rows, cols, h_variance_out, false);
    if (bad) return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_svgf_variance_host: ") + bad);
    if (rows == 0u || cols == 0u) return RT_OK;
    const size_t n = (size_t)rows * cols;
    /* a strided plane travels as the span from its first word to its last: (n - 1) strides and one width */
    const auto span = [n](uint32_t stride, uint32_t width) { return ((n - 1u) * stride + width) * sizeof(uint32_t); };
    HostRoundTrip t("rt_svgf_variance_host");
    rt_denoise_guides g = *guides;
    const rt_temporal_pixel *d_history = t.in(h_history, n * sizeof(rt_temporal_pixel));
    g.normal = t.in(guides->normal, span(guides->normal_stride, 3u));
    g.position = t.in(guides->position, span(guides->position_stride, 3u));
    g.albedo = nullptr;
    g.valid = t.in(guides->valid, span(guides->valid_stride, 1u));
    float *d_out = t.out(h_variance_out, n * sizeof(float));
    if (!t.ok()) return t.failed();
    const hipError_t e = rt::launch_svgf_variance(rt::svgf_variance_call(d_history, g, *params, rows, cols, d_out), nullptr);
    if (e != hipSuccess) return launched("rt_svgf_variance_host", e);
    return t.finish();
}

int rt_svgf_atrous_host(const float *h_color, uint32_t color_stride, const float *h_variance, const rt_denoise_guides *guides,
                        const rt_svgf_atrous_params *params, uint32_t rows, uint32_t cols, float *h_out, float *h_variance_out) {
    const char *bad = rt::svgf_atrous_limits(h_color, color_stride, h_variance, guides, params, rows, cols, h_out, h_variance_out, nullptr, false);
    if (bad) return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_svgf_atrous_host: ") + bad);
    if (rows == 0u || cols == 0u) return RT_OK;
    const size_t n = (size_t)rows * cols;
    const auto span = [n](uint32_t stride, uint32_t width) { return ((n - 1u) * stride + width) * sizeof(uint32_t); };
    HostRoundTrip t("rt_svgf_atrous_host");
    rt_denoise_guides g = *guides;
    const float *d_color = t.in(h_color, span(color_stride, 3u));
    const float *d_variance = t.in(h_variance, n * sizeof(float));
    g.normal = t.in(guides->normal, span(guides->normal_stride, 3u));
    g.position = t.in(guides->position, span(guides->position_stride, 3u));
    g.albedo = t.in(guides->albedo, span(guides->albedo_stride, 3u));
    g.valid = t.in(guides->valid, span(guides->valid_stride, 1u));
    float *d_out = t.out(h_out, n * 3u * sizeof(float));
    float *d_variance_out = t.out(h_variance_out, n * sizeof(float));
    const size_t temp_bytes = rt_svgf_temp_bytes(rows, cols, params->n_levels);
    float *d_temp = temp_bytes ? static_cast<float *>(t.scratch(temp_bytes)) : nullptr;
    if (!t.ok()) return t.failed();
    const hipError_t e = rt::launch_svgf(d_color, color_stride, d_variance, g, *params, rows, cols, d_out, d_variance_out, d_temp, nullptr);
    if (e != hipSuccess) return launched("rt_svgf_atrous_host", e);
    return t.finish();
}

} /* extern "C" */
