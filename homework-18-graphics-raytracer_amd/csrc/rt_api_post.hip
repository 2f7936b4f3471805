/*
 * rt_api_post.hip — what follows the render path on the device (main.rs:748-762, image.rs:55-66, photon.rs): post_process, the
 * sRGB / u8 encode, the accumulator, and the rt_math_eval diagnostics.  Kernels: rt_post.hip.  And the film queries' rt_film_offsets /
 * rt_film_splat (include/rt_amd.h "film queries"): the accumulator behind a reconstruction filter.  Kernels: rt_film_query.hip.
 */
#include "rt_api_internal.h"
#include "rt_film.h"

/* which form of the splat rt_film_splat launches unless RT_AMD_FILM_SPLAT_FORM says otherwise: 0 simple, 1 tiled — the tiled one, which
 * the measurement at 1920 x 1080 chose (DESIGN.md 3.20 has the figures and how they were taken) */
#define RT_FILM_SPLAT_FORM_DEFAULT 1

namespace rt {
void math_eval_host(int op, const float *x, const float *y, float *out, size_t n);
void math_eval_host(int op, const double *a, const double *b, double *out, size_t n);
}

/* rt_math_eval_device and rt_math_eval64_device: the operands to the device, one launch, the results back */
template <typename T>
static int math_eval_round_trip(const char *who, int op, const T *h_x, const T *h_y, T *h_out, size_t n) {
    if (!h_x || !h_out) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": null argument");
    if (n == 0) return RT_OK;
    T *d_x = nullptr, *d_y = nullptr, *d_o = nullptr;
    const size_t bytes = n * sizeof(T);
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_x), bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_y), bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_o), bytes);
    if (e == hipSuccess) e = hipMemcpy(d_x, h_x, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = h_y ? hipMemcpy(d_y, h_y, bytes, hipMemcpyHostToDevice) : hipMemset(d_y, 0, bytes);
    if (e == hipSuccess) e = rt::launch_math_eval(op, d_x, d_y, d_o, n, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(h_out, d_o, bytes, hipMemcpyDeviceToHost);
    if (d_x) (void)hipFree(d_x);
    if (d_y) (void)hipFree(d_y);
    if (d_o) (void)hipFree(d_o);
    if (e != hipSuccess) return fail_hip(who, e);
    return RT_OK;
}

extern "C" {

/* ---- post_process / encode on the device ----------------------------------------- */

struct PostWs {
    DeviceBuffer d_keys;  /* one word per pixel of the largest frame so far */
    DeviceBuffer d_state; /* 260 words */
};
/* keyed by (device, stream): the default stream is nullptr on every device, and a buffer allocated on one device must
 * not serve a launch on another.  Grow-only; rt_post_release() frees the buffers of the current device. */
static std::mutex g_post_mutex;
static std::map<std::pair<int, hipStream_t>, PostWs> g_post_ws;

int rt_post_release(void) {
    int device = 0;
    RT_HIP(hipGetDevice(&device));
    RT_HIP(hipDeviceSynchronize());
    select_release(device); /* rt_select_records' block totals */
    std::lock_guard<std::mutex> lock(g_post_mutex);
    for (auto it = g_post_ws.begin(); it != g_post_ws.end();) {
        if (it->first.first == device) {
            (void)it->second.d_keys.release();
            (void)it->second.d_state.release();
            it = g_post_ws.erase(it);
        } else {
            ++it;
        }
    }
    return RT_OK;
}

int rt_post_process_device(float *d_rgb, size_t n_pixels, float *d_divisor, void *hip_stream) {
    if (n_pixels && !d_rgb) return fail(RT_ERR_INVALID_ARGUMENT, "rt_post_process_device: null argument"); /* no pixels: nothing is read */
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (n_pixels == 0) {
        /* an empty image is "left untouched": divisor 0 (all bits zero), written in stream order as a memset node — nothing written from
         * the host, and capturable.  Only memory the runtime knows a device can reach takes a stream-ordered write; for any other
         * pointer (and without a device) there is nothing to enqueue, as before. */
        if (!d_divisor) return RT_OK;
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, d_divisor) != hipSuccess) {
            (void)hipGetLastError();
            return RT_OK;
        }
        if (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged && attr.type != hipMemoryTypeHost) return RT_OK;
        return launched("rt_post_process_device", hipMemsetAsync(d_divisor, 0, sizeof(float), stream));
    }
    uint32_t *keys = nullptr, *state = nullptr;
    int device = 0;
    RT_HIP(hipGetDevice(&device));
    {
        std::lock_guard<std::mutex> lock(g_post_mutex);
        PostWs &ws = g_post_ws[std::make_pair(device, stream)];
        hipError_t e = ws.d_state.reserve(260 * sizeof(uint32_t));
        if (e != hipSuccess) return fail_hip("hipMalloc(reinterpret_cast<void **>(&ws.d_state), 260 * sizeof(uint32_t))", e);
        e = ws.d_keys.reserve(n_pixels * sizeof(uint32_t));
        if (e != hipSuccess) return fail_hip("hipMalloc(reinterpret_cast<void **>(&ws.d_keys), n_pixels * sizeof(uint32_t))", e);
        keys = ws.d_keys.get<uint32_t>();
        state = ws.d_state.get<uint32_t>();
    }
    float row[3];
    rt::luma_row(row);
    return launched("rt_post_process_device", rt::launch_post_process(d_rgb, n_pixels, row, keys, state, d_divisor, stream));
}

/* the passes of rt_post_process_device one by one, on the caller's device memory (include/rt_amd.h) */
int rt_post_keys_device(const float *d_rgb, size_t n_pixels, uint32_t *d_keys, uint32_t *d_state, void *hip_stream) {
    if (!d_state || (n_pixels && (!d_rgb || !d_keys))) return fail(RT_ERR_INVALID_ARGUMENT, "rt_post_keys_device: null argument");
    float row[3];
    rt::luma_row(row);
    return launched("rt_post_keys_device", rt::launch_post_keys(d_rgb, n_pixels, row, d_keys, d_state, static_cast<hipStream_t>(hip_stream)));
}

int rt_post_hist_device(const uint32_t *d_keys, size_t n_pixels, int pass, uint32_t *d_state, void *hip_stream) {
    if (!d_state || (n_pixels && !d_keys)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_post_hist_device: null argument");
    if (pass < 0 || pass > 3) return fail(RT_ERR_INVALID_ARGUMENT, "rt_post_hist_device: pass 0..3");
    return launched("rt_post_hist_device", rt::launch_post_hist(d_keys, n_pixels, pass, d_state, static_cast<hipStream_t>(hip_stream)));
}

int rt_post_pick_device(int pass, uint32_t *d_state, void *hip_stream) {
    if (!d_state) return fail(RT_ERR_INVALID_ARGUMENT, "rt_post_pick_device: null argument");
    if (pass < 0 || pass > 3) return fail(RT_ERR_INVALID_ARGUMENT, "rt_post_pick_device: pass 0..3");
    return launched("rt_post_pick_device", rt::launch_post_pick(pass, d_state, static_cast<hipStream_t>(hip_stream)));
}

int rt_post_scale_device(float *d_rgb, size_t n_pixels, const uint32_t *d_state, float *d_divisor, void *hip_stream) {
    if (!d_state || (n_pixels && !d_rgb)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_post_scale_device: null argument");
    return launched("rt_post_scale_device", rt::launch_post_scale(d_rgb, n_pixels, d_state, d_divisor, static_cast<hipStream_t>(hip_stream)));
}

int rt_accumulate_device(const float *d_samples, const unsigned char *d_valid, uint32_t n_epochs, size_t n_pixels, float *d_sum,
                         float *d_weight, void *hip_stream) {
    /* what an empty call never reads may be NULL (an empty tensor's pointer is): no epochs -> no samples, no pixels -> nothing at all */
    if (n_pixels && (!d_sum || !d_weight || (n_epochs && (!d_samples || !d_valid))))
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_accumulate_device: null argument");
    return launched("rt_accumulate_device", rt::launch_accumulate(d_samples, d_valid, n_epochs, n_pixels, d_sum, d_weight, static_cast<hipStream_t>(hip_stream)));
}

int rt_accumulator_resolve_device(const float *d_sum, const float *d_weight, size_t n_pixels, float *d_rgb, void *hip_stream) {
    if (!d_sum || !d_weight || !d_rgb) return fail(RT_ERR_INVALID_ARGUMENT, "rt_accumulator_resolve_device: null argument");
    return launched("rt_accumulator_resolve_device", rt::launch_accumulator_resolve(d_sum, d_weight, n_pixels, d_rgb, static_cast<hipStream_t>(hip_stream)));
}

/* ---- film queries (rt_film_query.hip; rt_camera_rays_offset is rt_api_query.hip's) ---- */

int rt_film_offsets(const rt_frame *frame, uint32_t spp, uint32_t pattern, uint32_t seed, float *d_offsets, void *hip_stream) {
    bool unsupported;
    const char *bad = rt::film_offsets_limits(frame, spp, pattern, &unsupported);
    if (bad) return fail(unsupported ? RT_ERR_UNSUPPORTED : RT_ERR_INVALID_ARGUMENT, std::string("rt_film_offsets: ") + bad);
    const int rc = check_pointers("rt_film_offsets", d_offsets != nullptr, "offset");
    if (rc != RT_OK) return rc;
    return launched("rt_film_offsets", rt::launch_film_offsets(rt::film_tile(frame), spp, pattern, seed, d_offsets, static_cast<hipStream_t>(hip_stream)));
}

int rt_film_splat(uint32_t rows, uint32_t cols, const float *d_samples, const unsigned char *d_valid, const float *d_offsets, uint32_t spp,
                  uint32_t filter, float radius, float *d_sum, float *d_weight, void *hip_stream) {
    const char *bad = rt::film_splat_limits(rows, cols, spp, filter, radius);
    if (bad) return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_film_splat: ") + bad);
    if (rows == 0u || cols == 0u) return RT_OK;
    const int rc = check_pointers("rt_film_splat", d_samples && d_offsets && d_sum && d_weight, "sample, offset, sum or weight");
    if (rc != RT_OK) return rc;
    const rt::FilmSplat<rt::UniformLayout> p = {{d_samples, d_valid, d_offsets, (uint64_t)rows * cols, spp}, d_sum, d_weight, rows, cols, filter, radius};
    const bool tiled = rt::option(rt::OPT_FILM_SPLAT_FORM, RT_FILM_SPLAT_FORM_DEFAULT) == 1;
    return launched("rt_film_splat", rt::launch_film_splat(p, tiled, static_cast<hipStream_t>(hip_stream)));
}

int rt_encode_srgb8_device(const float *d_rgb, size_t n_values, unsigned char *d_out, void *hip_stream) {
    if (!d_rgb || !d_out) return fail(RT_ERR_INVALID_ARGUMENT, "rt_encode_srgb8_device: null argument");
    return launched("rt_encode_srgb8_device", rt::launch_encode_srgb8(d_rgb, n_values, d_out, static_cast<hipStream_t>(hip_stream)));
}

int rt_math_eval_host(int op, const float *x, const float *y, float *out, size_t n) {
    if (!x || !out) return fail(RT_ERR_INVALID_ARGUMENT, "rt_math_eval_host: null argument");
    rt::math_eval_host(op, x, y, out, n);
    return RT_OK;
}

int rt_math_eval_device(int op, const float *h_x, const float *h_y, float *h_out, size_t n) {
    return math_eval_round_trip("rt_math_eval_device", op, h_x, h_y, h_out, n);
}

int rt_math_eval64_host(int op, const double *a, const double *b, double *out, size_t n) {
    if (!a || !out) return fail(RT_ERR_INVALID_ARGUMENT, "rt_math_eval64_host: null argument");
    rt::math_eval_host(op, a, b, out, n);
    return RT_OK;
}

int rt_math_eval64_device(int op, const double *h_a, const double *h_b, double *h_out, size_t n) {
    return math_eval_round_trip("rt_math_eval64_device", op, h_a, h_b, h_out, n);
}

} /* extern "C" */
