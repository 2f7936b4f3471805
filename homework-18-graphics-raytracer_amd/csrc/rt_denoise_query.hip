/*
 * rt_denoise_query.hip — the denoise queries (include/rt_amd.h "denoise queries"): the edge-avoiding A-Trous filter, one launch per level,
 * kernels and entry points in one unit.
 *
 *   rt::denoise_kernel        the simple form: one thread per output pixel, grid-stride; the 25 sources read from global memory
 *   rt::denoise_tiled_kernel  the tiled form: a 256-thread workgroup owns 16 x 16 output pixels SPACED step APART — one residue class
 *                             (row mod step, column mod step) of a block of 16 step x 16 step pixels — and stages the 20 x 20 entries,
 *                             also step apart, that those outputs read: 400 entries of 9 words, 14.4 KB of LDS, at EVERY level (a
 *                             contiguous tile's halo is (16 + 4 step)^2 entries and stops fitting at step 16).  At step 1 it is the
 *                             contiguous tile.  Entry e is staged by thread e mod 256.
 *
 * The arithmetic is rt_denoise.h's, shared with librt_host.so.  Both kernels walk a pixel's sources in the order of the definition — dr,
 * then dc, ascending — and call denoise_load / denoise_tap / denoise_store on the same operands, so they give the same bits as each
 * other and as rt_denoise_atrous_cpu by construction, whatever the launch geometry.  An output pixel is written by one thread: no
 * atomics.  The tiled form marks an entry that lies outside the image or whose valid word is cleared ONCE, while staging, by giving it
 * a NaN colour: its exponent is NaN and denoise_tap skips it, as it skips a caller's own NaN colour in either form; an output pixel
 * whose own entry is so marked collects no weight and passes through, which is what the definition says of an invalid pixel.
 * Guides are read through their record strides where they lie: no pre-pass packs them, and the temp plane is one colour plane.
 * Every index into a plane is 64-bit; every read is behind an inside-the-image test; rows * cols < 2^32 is checked by the entry point.
 */
#include "rt_api_internal.h"
#include "rt_denoise.h"

/* which form rt_denoise_atrous launches unless RT_AMD_DENOISE_FORM says otherwise: 0 simple, 1 tiled — the tiled one, which the
 * measurement at 1920 x 1080 chose: far ahead on guides read through record strides, level on compact ones (DESIGN.md 3.21 has the
 * figures and the bar) */
#define RT_DENOISE_FORM_DEFAULT 1

namespace rt {

#define RT_DENOISE_THREADS 256u
#define RT_DENOISE_TILE 16u
#define RT_DENOISE_HALO (RT_DENOISE_TILE + 4u)
#define RT_DENOISE_MAX_GROUPS (1u << 16)

__global__ __launch_bounds__(RT_DENOISE_THREADS) void denoise_kernel(const DenoiseLevel L) {
    const uint64_t n = (uint64_t)L.rows * L.cols, stride = (uint64_t)gridDim.x * RT_DENOISE_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * RT_DENOISE_THREADS + threadIdx.x; i < n; i += stride) {
        const uint32_t r = (uint32_t)(i / L.cols), c = (uint32_t)(i - (uint64_t)r * L.cols);
        const bool filtered = denoise_valid(L, i);
        DenoiseAcc a = {0.0f, 0.0f, 0.0f, 0.0f};
        if (filtered) {
            const DenoisePix p = denoise_load(L, i);
            for (int dr = -2; dr <= 2; ++dr) {
                const int64_t qr = (int64_t)r + (int64_t)dr * L.step;
                if (qr < 0 || qr >= (int64_t)L.rows) continue;
                for (int dc = -2; dc <= 2; ++dc) {
                    const int64_t qc = (int64_t)c + (int64_t)dc * L.step;
                    if (qc < 0 || qc >= (int64_t)L.cols) continue;
                    const uint64_t qi = (uint64_t)qr * L.cols + (uint64_t)qc;
                    if (!denoise_valid(L, qi)) continue;
                    denoise_tap(L, a, p, denoise_load(L, qi), dr, dc);
                }
            }
        }
        denoise_store(L, i, filtered, a);
    }
}

/* blocks_x: blocks of 16 step x 16 step pixels across the image; n_tiles = blocks * step * step, block-major, then the residue's row, then
 * its column.  Workgroups take tiles grid-stride, so every thread of a workgroup meets the same barriers. */
__global__ __launch_bounds__(RT_DENOISE_THREADS) void denoise_tiled_kernel(const DenoiseLevel L, const uint32_t blocks_x, const uint64_t n_tiles) {
    __shared__ DenoisePix l_pix[RT_DENOISE_HALO * RT_DENOISE_HALO];
    const int64_t step = L.step;
    const uint32_t per_block = (uint32_t)(L.step * L.step);
    const uint32_t ty = threadIdx.x / RT_DENOISE_TILE, tx = threadIdx.x % RT_DENOISE_TILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) { /* workgroup-uniform */
        const uint64_t block = tile / per_block;
        const uint32_t res = (uint32_t)(tile - block * per_block);
        const uint32_t block_r = (uint32_t)(block / blocks_x), block_c = (uint32_t)(block - (uint64_t)block_r * blocks_x);
        const int64_t r0 = (int64_t)block_r * RT_DENOISE_TILE * step + res / (uint32_t)L.step;
        const int64_t c0 = (int64_t)block_c * RT_DENOISE_TILE * step + res % (uint32_t)L.step;
        if (r0 >= (int64_t)L.rows || c0 >= (int64_t)L.cols) continue; /* a residue class the image's last block does not reach: uniform */
        __syncthreads(); /* the previous tile's reads are done */
        for (uint32_t e = threadIdx.x; e < RT_DENOISE_HALO * RT_DENOISE_HALO; e += RT_DENOISE_THREADS) {
            const uint32_t hr = e / RT_DENOISE_HALO, hc = e - hr * RT_DENOISE_HALO;
            const int64_t qr = r0 + ((int64_t)hr - 2) * step, qc = c0 + ((int64_t)hc - 2) * step;
            DenoisePix q = {__uint_as_float(0x7fc00000u), 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}; /* NaN colour: a source of nobody */
            if (qr >= 0 && qr < (int64_t)L.rows && qc >= 0 && qc < (int64_t)L.cols) {
                const uint64_t qi = (uint64_t)qr * L.cols + (uint64_t)qc;
                if (denoise_valid(L, qi)) q = denoise_load(L, qi);
            }
            l_pix[e] = q;
        }
        __syncthreads();
        const int64_t r = r0 + (int64_t)ty * step, c = c0 + (int64_t)tx * step;
        if (r < (int64_t)L.rows && c < (int64_t)L.cols) {
            const DenoisePix p = l_pix[(ty + 2u) * RT_DENOISE_HALO + (tx + 2u)];
            DenoiseAcc a = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int dr = -2; dr <= 2; ++dr)
                for (int dc = -2; dc <= 2; ++dc) denoise_tap(L, a, p, l_pix[(uint32_t)((int)ty + 2 + dr) * RT_DENOISE_HALO + (uint32_t)((int)tx + 2 + dc)], dr, dc);
            denoise_store(L, (uint64_t)r * L.cols + (uint64_t)c, true, a);
        }
    }
}

static hipError_t launch_denoise_level(const DenoiseLevel &L, bool tiled, uint32_t max_groups, hipStream_t stream) {
    if (tiled) {
        const uint64_t side = (uint64_t)RT_DENOISE_TILE * (uint64_t)L.step;
        const uint32_t blocks_x = (uint32_t)((L.cols + side - 1u) / side), blocks_y = (uint32_t)((L.rows + side - 1u) / side);
        const uint64_t n_tiles = (uint64_t)blocks_x * blocks_y * (uint64_t)L.step * (uint64_t)L.step;
        hipLaunchKernelGGL(denoise_tiled_kernel, dim3((uint32_t)std::min<uint64_t>(n_tiles, max_groups)), dim3(RT_DENOISE_THREADS), 0, stream, L, blocks_x, n_tiles);
    } else {
        const uint64_t groups = ((uint64_t)L.rows * L.cols + RT_DENOISE_THREADS - 1u) / RT_DENOISE_THREADS;
        hipLaunchKernelGGL(denoise_kernel, dim3((uint32_t)std::min<uint64_t>(groups, max_groups)), dim3(RT_DENOISE_THREADS), 0, stream, L);
    }
    return hipGetLastError();
}

static hipError_t launch_denoise(const float *color, const rt_denoise_guides &g, const rt_denoise_params &p, uint32_t rows, uint32_t cols, float *out, float *temp,
                                 hipStream_t stream) {
    const bool tiled = option(OPT_DENOISE_FORM, RT_DENOISE_FORM_DEFAULT) == 1;
    const long long cap = option(OPT_DIAG_DENOISE_MAX_GROUPS, RT_DENOISE_MAX_GROUPS); /* test hook: fewer workgroups, so a small image is taken grid-stride */
    const uint32_t max_groups = cap >= 1 && cap < (long long)RT_DENOISE_MAX_GROUPS ? (uint32_t)cap : RT_DENOISE_MAX_GROUPS;
    for (uint32_t j = 0; j < p.n_levels; ++j) {
        const hipError_t e = launch_denoise_level(denoise_level(color, g, p, rows, cols, out, temp, j), tiled, max_groups, stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
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
    /* a strided plane travels as the span from its first word to its last: (n - 1) strides and one width */
    const auto span = [n](uint32_t stride, uint32_t width) { return ((n - 1u) * stride + width) * sizeof(uint32_t); };
    HostRoundTrip t("rt_denoise_atrous_host");
    rt_denoise_guides g = *guides;
    const float *d_color = t.in(h_color, plane);
    g.normal = t.in(guides->normal, span(guides->normal_stride, 3u));
    g.position = t.in(guides->position, span(guides->position_stride, 3u));
    g.albedo = t.in(guides->albedo, span(guides->albedo_stride, 3u));
    g.valid = t.in(guides->valid, span(guides->valid_stride, 1u));
    float *d_out = t.out(h_out, plane);
    float *d_temp = params->n_levels >= 2u ? static_cast<float *>(t.scratch(plane)) : nullptr;
    if (!t.ok()) return t.failed();
    const hipError_t e = rt::launch_denoise(d_color, g, *params, rows, cols, d_out, d_temp, nullptr);
    if (e != hipSuccess) return launched("rt_denoise_atrous_host", e);
    return t.finish();
}

} /* extern "C" */
