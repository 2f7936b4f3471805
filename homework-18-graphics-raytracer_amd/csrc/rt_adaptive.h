/*
 * rt_adaptive.h — the arithmetic of the adaptive sampling queries (include/rt_amd.h "adaptive sampling queries"), written once for the
 * host (librt_host.so: rt_sample_budget_cpu / rt_sample_list_cpu / rt_film_offsets_listed_cpu / rt_camera_rays_listed_cpu /
 * rt_film_splat_listed_cpu) and the device (rt_adaptive_query.hip).  Every function is a sequence of single f32 or u32 operations in
 * the order the header comment of the block gives; both libraries are built with -ffp-contract=off, divide and square root are
 * correctly rounded on either side, so host and device agree bit for bit.  The sample positions, the tile, the filter and the whole
 * splat walk are rt_film.h's: film_u / film_offset, FilmTile, film_splat_pixel.  The listed splat adds one thing, ListedLayout: where
 * the samples of a source pixel lie in a pixel-major list.
 *
 * listed_ray_words restates rt_primary_ray.h's primary_ray_through for the CPU form (that header is device code on rt_cast.h); the
 * device kernel calls primary_ray_through itself, and the tests hold the two against each other.
 */
#ifndef RT_ADAPTIVE_H
#define RT_ADAPTIVE_H

#include "rt_film.h"
#include "rt_temporal.h"

namespace rt {

/* ---- rt_sample_budget ---- */

struct SampleBudget {
    const float *mean, *variance;
    const uint32_t *taken, *valid; /* the count plane and the valid plane: each may be null */
    uint32_t mean_stride, variance_stride, count_stride, valid_stride;
    float gain, epsilon;
    uint32_t min_count, max_count;
    uint32_t *budget;
    uint64_t n;
    RT_FILM_HD uint64_t count() const { return n; }
    RT_FILM_HD void operator()(uint64_t i) const; /* budget[i] = sample_budget_pixel */
};

/* the six steps of the definition for pixel i */
RT_FILM_HD uint32_t sample_budget_pixel(const SampleBudget &b, uint64_t i) {
    if (b.valid != nullptr && b.valid[i * b.valid_stride] == 0u) return 0u;
    const uint32_t count = b.taken != nullptr ? b.taken[i * b.count_stride] : 1u;
    if (count == 0u) return b.max_count;
    const float e = rtdm::f_sqrt(b.variance[i * b.variance_stride] / (float)count) / (fabsf(b.mean[i * b.mean_stride]) + b.epsilon);
    const float t = e * b.gain;
    const uint32_t range = b.max_count - b.min_count;
    return b.min_count + (t < (float)range ? (uint32_t)t : range); /* the test first: a NaN or a huge t is never converted */
}
RT_FILM_HD void SampleBudget::operator()(uint64_t i) const { budget[i] = sample_budget_pixel(*this, i); }

/* the arguments of rt_sample_budget and its CPU form (rt_query_args.h; there is no _host form, so no arrays()) */
struct SampleBudgetArgs {
    const float *mean; uint32_t mean_stride;
    const float *variance; uint32_t variance_stride;
    const uint32_t *count; uint32_t count_stride;
    const uint32_t *valid; uint32_t valid_stride;
    const rt_sample_budget_params *params; uint64_t n; uint32_t *budget;

    const char *limits(QueryForm, int *status) const {
        *status = RT_ERR_UNSUPPORTED;
        if (n >= (1ull << 32)) return "2^32 pixels or more";
        *status = RT_ERR_INVALID_ARGUMENT;
        if (empty()) return nullptr;
        if (!params) return "null params";
        if (!mean || !variance || !budget) return "null mean, variance or budget pointer";
        if (mean_stride < 1u || variance_stride < 1u || (count && count_stride < 1u) || (valid && valid_stride < 1u)) return "a stride smaller than its plane's width (1 word)";
        if (!(params->gain >= 0.0f)) return "gain must be >= 0";
        if (!(params->epsilon > 0.0f)) return "epsilon must be > 0";
        if (!(params->min_count <= params->max_count && params->max_count <= RT_SAMPLE_MAX)) return "need min_count <= max_count <= RT_SAMPLE_MAX";
        if (params->flags != 0u) return "flags must be 0";
        return nullptr;
    }

    bool empty() const { return n == 0u; }

    SampleBudget call() const {
        return {mean, variance, count, valid, mean_stride, variance_stride, count_stride, valid_stride, params->gain, params->epsilon, params->min_count,
                params->max_count, budget, n};
    }
};

/* ---- rt_sample_list ---- */

RT_FILM_HD uint32_t sample_count_clamped(uint32_t c) { return c < RT_SAMPLE_MAX ? c : RT_SAMPLE_MAX; }

/* the 256-pixel steps of n pixels, and the scratch of rt_sample_list: one u32 per step and one for the sum of all */
#define RT_SAMPLE_LIST_STEP 256u
inline uint64_t sample_list_steps(uint64_t n) { return (n + RT_SAMPLE_LIST_STEP - 1u) / RT_SAMPLE_LIST_STEP; }
inline uint64_t sample_list_temp_bytes(uint64_t n) {
    if (n == 0u || n * RT_SAMPLE_MAX >= (1ull << 32)) return 0u;
    return (sample_list_steps(n) + 1u) * sizeof(uint32_t);
}

/* the limits and pointers of rt_sample_list and its CPU form; *empty: n == 0 (only start_0 and the totals are written) */
inline const char *sample_list_limits(const uint32_t *counts, uint64_t n, uint64_t capacity, const uint32_t *start, const uint32_t *pixel, const uint32_t *sample,
                                      const uint32_t *total, int *status) {
    *status = RT_ERR_UNSUPPORTED;
    if (n >= (1ull << 32) || n * RT_SAMPLE_MAX >= (1ull << 32)) return "n * RT_SAMPLE_MAX is 2^32 or more (list the frame in several calls)";
    if (capacity >= (1ull << 32)) return "a capacity of 2^32 records or more";
    *status = RT_ERR_INVALID_ARGUMENT;
    if (!start || !total) return "null start or total pointer";
    if (n == 0u) return nullptr;
    if (!counts) return "null counts pointer";
    if (capacity != 0u && (!pixel || !sample)) return "null pixel or sample pointer";
    return nullptr;
}

/* ---- rt_film_offsets_listed / rt_camera_rays_listed ---- */

struct ListedOffsets {
    FilmTile t;
    uint32_t pattern, seed;
    const uint32_t *pixel, *sample, *total;
    uint64_t capacity;
    float *offsets;
};

RT_FILM_HD uint64_t listed_count(const uint32_t *total, uint64_t capacity) { return (uint64_t)total[0] < capacity ? (uint64_t)total[0] : capacity; }

/* record j of the offsets; listed: listed_count(total, capacity) */
RT_FILM_HD void listed_offsets_record(const ListedOffsets &o, uint64_t j, uint64_t listed) {
    uint32_t *out = reinterpret_cast<uint32_t *>(o.offsets) + 2u * j;
    out[0] = RT_FILM_NAN, out[1] = RT_FILM_NAN;
    if (j >= listed) return;
    const uint32_t pix = o.pixel[j];
    if ((uint64_t)pix >= (uint64_t)o.t.rows * o.t.cols) return;
    const uint32_t row = pix / o.t.cols, col = pix - row * o.t.cols;
    const uint32_t global = film_global_pixel(o.t, row, col);
    const uint32_t s = o.sample[j];
    o.offsets[2u * j] = film_offset(o.pattern, 0u, global, o.seed, s, 0u);
    o.offsets[2u * j + 1u] = film_offset(o.pattern, 0u, global, o.seed, s, 1u);
}

/* the arguments of rt_film_offsets_listed and its CPU form (rt_query_args.h; no _host form) */
struct ListedOffsetsArgs {
    const rt_frame *frame;
    uint32_t pattern, seed;
    const uint32_t *pixel, *sample, *total;
    uint64_t capacity;
    float *offsets;

    const char *limits(QueryForm, int *status) const {
        *status = RT_ERR_INVALID_ARGUMENT;
        if (!frame) return "null frame";
        const uint64_t pixels = film_frame_pixels(frame);
        if (pixels == 0u) return "bad frame (need 0 <= x0 < x1 <= width, 0 <= y0 < y1 <= height, y_step >= 1)";
        if (pattern == RT_FILM_STRATIFIED) return "RT_FILM_STRATIFIED has no k x k in a ragged pass (RT_FILM_CENTER or RT_FILM_UNIFORM)";
        if (pattern != RT_FILM_CENTER && pattern != RT_FILM_UNIFORM) return "unknown pattern (RT_FILM_CENTER or RT_FILM_UNIFORM)";
        if (pixels >= (1ull << 32) || capacity >= (1ull << 32)) {
            *status = RT_ERR_UNSUPPORTED;
            return "2^32 pixels or records or more";
        }
        if (empty()) return nullptr;
        if (!pixel || !sample || !total || !offsets) return "null pixel, sample, total or offset pointer";
        return nullptr;
    }

    bool empty() const { return capacity == 0u; }

    ListedOffsets call() const { return {film_tile(frame), pattern, seed, pixel, sample, total, capacity, offsets}; }
};

/* the camera of a listed ray: make_kernel_frame's fields (rt_temporal.h temporal_camera) and the tile */
struct ListedCamera {
    TemporalCamera cam;
    FilmTile t;
};

/* primary_ray_through (rt_primary_ray.h) and store_primary_ray as the eleven words of an rt_ray, for the CPU form */
inline void listed_ray_words(const ListedCamera &c, float xf, float yf, uint32_t w[11]) {
    const float clip_y = (c.cam.half_height - yf) / c.cam.height_f;
    const float clip_x = (xf - c.cam.half_width) / c.cam.height_f;
    const V3 d = normalize(clip_x * v3p(c.cam.cam_x) + clip_y * v3p(c.cam.cam_y) + v3p(c.cam.toward));
    w[0] = temporal_bits(c.cam.origin[0]), w[1] = temporal_bits(c.cam.origin[1]), w[2] = temporal_bits(c.cam.origin[2]);
    w[3] = temporal_bits(d.x), w[4] = temporal_bits(d.y), w[5] = temporal_bits(d.z);
    w[6] = 0u /* Front */, w[7] = 0u, w[8] = 0u, w[9] = 0u, w[10] = 0u;
}

inline const char *listed_rays_limits(const rt_camera *camera, const rt_frame *frame, const float *offsets, const uint32_t *pixel, const uint32_t *total,
                                      uint64_t capacity, const rt_ray *rays, int *status) {
    *status = RT_ERR_INVALID_ARGUMENT;
    if (!camera || !frame) return "null camera or frame";
    const uint64_t pixels = film_frame_pixels(frame);
    if (pixels == 0u) return "bad frame (need 0 <= x0 < x1 <= width, 0 <= y0 < y1 <= height, y_step >= 1)";
    if (pixels >= (1ull << 32) || capacity >= (1ull << 32)) {
        *status = RT_ERR_UNSUPPORTED;
        return "2^32 pixels or rays or more";
    }
    if (capacity == 0u) return nullptr;
    if (!offsets || !pixel || !total || !rays) return "null offset, pixel, total or ray pointer";
    return nullptr;
}

/* ---- rt_film_splat_listed ---- */

/* the records of source pixel q of a list: [*lo, *lo + the return value), always inside [0, capacity) whatever `start` holds */
RT_FILM_HD uint32_t listed_range(const uint32_t *start, uint64_t capacity, uint64_t q, uint64_t *lo) {
    const uint64_t a = (uint64_t)start[q] < capacity ? (uint64_t)start[q] : capacity;
    const uint64_t b = (uint64_t)start[q + 1u] < capacity ? (uint64_t)start[q + 1u] : capacity;
    *lo = a;
    return b > a ? (uint32_t)(b - a) : 0u;
}

/* the pixel-major list as a layout of rt_film.h's walk (film_splat_pixel) and of rt_film_splat_kernel.h's tiled kernel */
struct ListedLayout {
    static constexpr bool ragged = true;
    const float *samples;
    const unsigned char *valid; /* may be null */
    const float *offsets;
    const uint32_t *start;
    uint64_t capacity;
    uint32_t max_count;
    RT_FILM_HD uint32_t s_end() const { return max_count; }
    RT_FILM_HD uint32_t range(uint64_t q, uint64_t *lo) const { return listed_range(start, capacity, q, lo); }
    RT_FILM_HD uint64_t record(uint64_t lo, uint32_t s) const { return lo + s; }
};

inline const char *listed_splat_limits(uint64_t rows, uint64_t cols, const float *samples, const float *offsets, const uint32_t *start, uint64_t capacity,
                                       uint32_t max_count, uint32_t filter, float radius, const float *sum, const float *weight, int *status) {
    *status = RT_ERR_INVALID_ARGUMENT;
    if (filter != RT_FILM_BOX && filter != RT_FILM_TENT && filter != RT_FILM_MITCHELL) return "unknown filter (RT_FILM_BOX, RT_FILM_TENT or RT_FILM_MITCHELL)";
    if (!(radius > 0.0f && radius <= 4.0f)) return "radius must be in (0, 4] pixels";
    if (max_count < 1u || max_count > RT_SAMPLE_MAX) return "max_count must be in 1 .. RT_SAMPLE_MAX";
    if (rows >= (1ull << 32) || cols >= (1ull << 32) || rows * cols >= (1ull << 32) || capacity >= (1ull << 32)) {
        *status = RT_ERR_UNSUPPORTED;
        return "2^32 pixels or records or more";
    }
    if (rows == 0u || cols == 0u) return nullptr;
    if (!start || !sum || !weight) return "null start, sum or weight pointer";
    if (capacity != 0u && (!samples || !offsets)) return "null sample or offset pointer";
    return nullptr;
}

} /* namespace rt */

#endif /* RT_ADAPTIVE_H */
