/*
 * rt_api_query.hip — rt_cast_rays / rt_cast_rays_host / rt_camera_rays (include/rt_amd.h "ray queries"): validation, the
 * per-(scene, stream) workspace of a scene walked breadth-first, the launches of rt_query.hip; and rt_shade_hits / rt_reflect_rays /
 * rt_refract_rays with their _host forms ("hit queries"): validation and the launches of rt_hit_query.hip, no workspace; and
 * rt_scatter_hits / rt_scatter_factors with theirs ("scatter queries", rt_scatter_query.hip).  No CPU path: without a device every
 * call fails with a status.
 */
#include "rt_api_internal.h"

static_assert(sizeof(rt_ray) == 44 && sizeof(rt_hit) == 52, "the ABI records are flat u32 / f32 words");

/* The breadth-first walk's record lists for a cast of n rays (or index entries) on `stream`: per wave of the grid, in the workspace
 * rt_render_whitted keeps them in (sized and grown as there: workgroups x 8 waves x pwf_bfs_scratch_words_per_wave), one workgroup per
 * CU at most.  false: no room for the lists, or a capture before the first call on this stream (allocation cannot be captured). */
namespace {
struct BfsLists {
    uint32_t *lists = nullptr;
    uint32_t items_cap = RT_BFS_ITEMS_CAP, jobs_cap = RT_BFS_JOBS_CAP, groups = 0;
};
} /* namespace */
static bool bfs_lists(const rt_scene *scene, hipStream_t stream, uint32_t n, BfsLists *out) {
    const uint64_t cus = scene->resident_waves / (4u * (uint32_t)RT_MIN_WAVES);
    uint64_t groups = ((uint64_t)n + 64u * RT_QUERY_BFS_WAVES - 1u) / (64u * RT_QUERY_BFS_WAVES);
    if (groups > cus) groups = cus;
    if (groups < 1) groups = 1;
    static_assert(RT_QUERY_BFS_WAVES == 8u, "the lists are sized per wave of an 8-wave workgroup, as rt_render_whitted sizes them");
    const size_t words = (size_t)groups * RT_QUERY_BFS_WAVES * rt::pwf_bfs_scratch_words_per_wave();
    out->groups = (uint32_t)groups;
    rt_scene *mut = const_cast<rt_scene *>(scene); /* workspaces are the only mutable part of a scene */
    std::lock_guard<std::mutex> lock(mut->ws_mutex);
    Workspace &ws = mut->workspaces[stream];
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &capturing) != hipSuccess) (void)hipGetLastError();
    if (ws.bfs_words < words && capturing == hipStreamCaptureStatusNone) { /* allocation cannot be captured */
        if (ws.d_bfs) (void)hipFree(ws.d_bfs);
        ws.d_bfs = nullptr;
        ws.bfs_words = 0;
        if (hipMalloc(reinterpret_cast<void **>(&ws.d_bfs), words * sizeof(uint32_t)) != hipSuccess) { (void)hipGetLastError(); ws.d_bfs = nullptr; }
        else ws.bfs_words = words;
    }
    if (ws.d_bfs != nullptr && ws.bfs_words >= words) out->lists = ws.d_bfs;
    const long long cap = rt::option(rt::OPT_DIAG_BFS_CAP, 0); /* test hook: shorter lists (the memory is the same) */
    if (cap > 0) {
        out->items_cap = (uint32_t)std::min<long long>(cap, RT_BFS_ITEMS_CAP);
        out->jobs_cap = (uint32_t)std::min<long long>(cap, RT_BFS_JOBS_CAP);
    }
    return out->lists != nullptr;
}

extern "C" {

int rt_cast_rays(const rt_scene *scene, const rt_ray *d_rays, size_t n_rays, rt_hit *d_hits, void *hip_stream) {
    if ((uint64_t)n_rays >= (1ull << 32)) return fail(RT_ERR_UNSUPPORTED, "rt_cast_rays: 2^32 rays or more (checked first; cast them in several calls)");
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "rt_cast_rays: null scene");
    if (n_rays == 0) return RT_OK;
    if (!d_rays || !d_hits) return fail(RT_ERR_INVALID_ARGUMENT, "rt_cast_rays: null ray or hit pointer");
    const uint32_t n = (uint32_t)n_rays;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const bool wave_uniform = rt::option(rt::OPT_QUERY_WAVE_UNIFORM, 0) == 1;
    hipError_t e = hipSuccess;
    if (scene->ks.bfs_walk != 0u && !wave_uniform) {
        BfsLists bl;
        if (bfs_lists(scene, stream, n, &bl)) {
            e = rt::launch_cast_rays_bfs(scene->ks, d_rays, d_hits, n, bl.lists, bl.items_cap, bl.jobs_cap, bl.groups, stream);
            if (e != hipSuccess) return fail_hip("rt_cast_rays: launch", e);
            return RT_OK;
        }
        /* no room for the lists (or a capture before the first call on this stream): the pair-wise kernel, exact as well */
    }
    e = rt::launch_cast_rays(scene->ks, d_rays, d_hits, n, wave_uniform, stream);
    if (e != hipSuccess) return fail_hip("rt_cast_rays: launch", e);
    return RT_OK;
}

int rt_cast_rays_host(const rt_scene *scene, const rt_ray *h_rays, size_t n_rays, rt_hit *h_hits) {
    if ((uint64_t)n_rays >= (1ull << 32)) return fail(RT_ERR_UNSUPPORTED, "rt_cast_rays_host: 2^32 rays or more (checked first; cast them in several calls)");
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "rt_cast_rays_host: null scene");
    if (n_rays == 0) return RT_OK;
    if (!h_rays || !h_hits) return fail(RT_ERR_INVALID_ARGUMENT, "rt_cast_rays_host: null ray or hit pointer");
    rt_ray *d_rays = nullptr;
    rt_hit *d_hits = nullptr;
    RT_HIP(hipMalloc(reinterpret_cast<void **>(&d_rays), n_rays * sizeof(rt_ray)));
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_hits), n_rays * sizeof(rt_hit));
    if (e == hipSuccess) e = hipMemcpy(d_rays, h_rays, n_rays * sizeof(rt_ray), hipMemcpyHostToDevice);
    int rc = RT_OK;
    if (e == hipSuccess) {
        rc = rt_cast_rays(scene, d_rays, n_rays, d_hits, nullptr);
        if (rc == RT_OK) {
            e = hipDeviceSynchronize();
            if (e == hipSuccess) e = hipMemcpy(h_hits, d_hits, n_rays * sizeof(rt_hit), hipMemcpyDeviceToHost);
        }
    }
    (void)hipFree(d_rays);
    if (d_hits) (void)hipFree(d_hits);
    if (rc != RT_OK) return rc;
    if (e != hipSuccess) return fail_hip("rt_cast_rays_host", e);
    return RT_OK;
}

int rt_camera_rays(const rt_camera *camera, const rt_frame *frame, rt_ray *d_rays, void *hip_stream) {
    if (!camera || !frame) return fail(RT_ERR_INVALID_ARGUMENT, "rt_camera_rays: null argument");
    if (!frame_ok(frame)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_camera_rays: bad frame (need 0 <= x0 < x1 <= width, 0 <= y0 < y1 <= height, y_step >= 1)");
    if (!d_rays) return fail(RT_ERR_INVALID_ARGUMENT, "rt_camera_rays: null ray pointer");
    rt_frame f = *frame;
    f.max_depth = 0; /* not used here */
    rt::KernelFrame kf;
    const int rc = make_kernel_frame(camera, &f, &kf); /* refuses a tile of 2^32 pixels or more */
    if (rc != RT_OK) return rc;
    const hipError_t e = rt::launch_camera_rays(kf, d_rays, static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail_hip("rt_camera_rays: launch", e);
    return RT_OK;
}

/* ---- hit queries (rt_hit_query.hip) ---- */

/* the checks every hit query makes before any device work, in the documented order; *done: nothing to launch */
static int hit_query_args(const char *who, bool needs_scene, const void *scene, size_t n, bool pointers_ok, const char *pointers, bool *done) {
    *done = true;
    if ((uint64_t)n >= (1ull << 32)) return fail(RT_ERR_UNSUPPORTED, std::string(who) + ": 2^32 records or more (checked first; query them in several calls)");
    if (needs_scene && !scene) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": null scene");
    if (n == 0) return RT_OK;
    if (!pointers_ok) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": null " + pointers + " pointer");
    *done = false;
    return RT_OK;
}

/* records per launch: RT_HITQ_BAND, or what the test hook asks for, in whole 64-record chunks */
static uint32_t hit_query_band() {
    const long long hook = rt::option(rt::OPT_DIAG_HIT_BAND_RECORDS, 0);
    if (hook > 0 && hook < (long long)RT_HITQ_BAND) return (uint32_t)((hook + 63) & ~63ll);
    return RT_HITQ_BAND;
}

int rt_shade_hits(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, float *d_rgb, unsigned long long *d_ray_count,
                  void *hip_stream) {
    bool done;
    const int rc = hit_query_args("rt_shade_hits", true, scene, n, d_hits && d_incoming && d_rgb, "hit, incoming-ray or rgb", &done);
    if (rc != RT_OK || done) return rc;
    const bool wave_uniform = rt::option(rt::OPT_QUERY_WAVE_UNIFORM, 0) == 1;
    const hipError_t e = rt::launch_shade_hits(scene->ks, d_hits, d_incoming, (uint32_t)n, d_rgb, d_ray_count, wave_uniform, hit_query_band(),
                                               static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail_hip("rt_shade_hits: launch", e);
    return RT_OK;
}

int rt_reflect_rays(const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, rt_ray *d_out, void *hip_stream) {
    bool done;
    const int rc = hit_query_args("rt_reflect_rays", false, nullptr, n, d_hits && d_incoming && d_out, "hit, incoming-ray or output", &done);
    if (rc != RT_OK || done) return rc;
    const hipError_t e = rt::launch_reflect_rays(d_hits, d_incoming, (uint32_t)n, d_out, hit_query_band(), static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail_hip("rt_reflect_rays: launch", e);
    return RT_OK;
}

int rt_refract_rays(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, float max_distance, uint32_t *d_kind,
                    float *d_travel, rt_ray *d_escape, unsigned long long *d_ray_count, void *hip_stream) {
    bool done;
    const int rc = hit_query_args("rt_refract_rays", true, scene, n, d_hits && d_incoming && d_kind && d_escape, "hit, incoming-ray, kind or escape-ray", &done);
    if (rc != RT_OK || done) return rc;
    const bool wave_uniform = rt::option(rt::OPT_QUERY_WAVE_UNIFORM, 0) == 1;
    const hipError_t e = rt::launch_refract_rays(scene->ks, d_hits, d_incoming, (uint32_t)n, max_distance, d_kind, d_travel, d_escape, d_ray_count,
                                                 wave_uniform, hit_query_band(), static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail_hip("rt_refract_rays: launch", e);
    return RT_OK;
}

/* device copies of the two inputs and a zeroed counter, shared by the _host forms; everything is freed by the destructor */
namespace {
struct HitQueryBuffers {
    rt_hit *d_hits = nullptr;
    rt_ray *d_incoming = nullptr;
    unsigned long long *d_cnt = nullptr;
    std::vector<void *> outs;
    ~HitQueryBuffers() {
        if (d_hits) (void)hipFree(d_hits);
        if (d_incoming) (void)hipFree(d_incoming);
        if (d_cnt) (void)hipFree(d_cnt);
        for (void *p : outs) if (p) (void)hipFree(p);
    }
    hipError_t upload(const rt_hit *h_hits, const rt_ray *h_incoming, size_t n) {
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_hits), n * sizeof(rt_hit));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_incoming), n * sizeof(rt_ray));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_cnt), sizeof(unsigned long long));
        if (e == hipSuccess) e = hipMemset(d_cnt, 0, sizeof(unsigned long long));
        if (e == hipSuccess) e = hipMemcpy(d_hits, h_hits, n * sizeof(rt_hit), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_incoming, h_incoming, n * sizeof(rt_ray), hipMemcpyHostToDevice);
        return e;
    }
    hipError_t out(void **p, size_t bytes) {
        const hipError_t e = hipMalloc(p, bytes);
        if (e == hipSuccess) outs.push_back(*p);
        return e;
    }
};
} /* namespace */

int rt_shade_hits_host(const rt_scene *scene, const rt_hit *h_hits, const rt_ray *h_incoming, size_t n, float *h_rgb, unsigned long long *h_ray_count) {
    bool done;
    int rc = hit_query_args("rt_shade_hits_host", true, scene, n, h_hits && h_incoming && h_rgb, "hit, incoming-ray or rgb", &done);
    if (rc == RT_OK && done && h_ray_count) *h_ray_count = 0;
    if (rc != RT_OK || done) return rc;
    HitQueryBuffers b;
    float *d_rgb = nullptr;
    hipError_t e = b.upload(h_hits, h_incoming, n);
    if (e == hipSuccess) e = b.out(reinterpret_cast<void **>(&d_rgb), n * 3 * sizeof(float));
    if (e != hipSuccess) return fail_hip("rt_shade_hits_host", e);
    rc = rt_shade_hits(scene, b.d_hits, b.d_incoming, n, d_rgb, b.d_cnt, nullptr);
    if (rc != RT_OK) return rc;
    unsigned long long cnt = 0;
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(&cnt, b.d_cnt, sizeof cnt, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h_rgb, d_rgb, n * 3 * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail_hip("rt_shade_hits_host", e);
    if (h_ray_count) *h_ray_count = cnt;
    return RT_OK;
}

int rt_refract_rays_host(const rt_scene *scene, const rt_hit *h_hits, const rt_ray *h_incoming, size_t n, float max_distance, uint32_t *h_kind,
                         float *h_travel, rt_ray *h_escape, unsigned long long *h_ray_count) {
    bool done;
    int rc = hit_query_args("rt_refract_rays_host", true, scene, n, h_hits && h_incoming && h_kind && h_escape, "hit, incoming-ray, kind or escape-ray", &done);
    if (rc == RT_OK && done && h_ray_count) *h_ray_count = 0;
    if (rc != RT_OK || done) return rc;
    HitQueryBuffers b;
    uint32_t *d_kind = nullptr;
    float *d_travel = nullptr;
    rt_ray *d_escape = nullptr;
    hipError_t e = b.upload(h_hits, h_incoming, n);
    if (e == hipSuccess) e = b.out(reinterpret_cast<void **>(&d_kind), n * sizeof(uint32_t));
    if (e == hipSuccess && h_travel) e = b.out(reinterpret_cast<void **>(&d_travel), n * sizeof(float));
    if (e == hipSuccess) e = b.out(reinterpret_cast<void **>(&d_escape), n * sizeof(rt_ray));
    if (e != hipSuccess) return fail_hip("rt_refract_rays_host", e);
    rc = rt_refract_rays(scene, b.d_hits, b.d_incoming, n, max_distance, d_kind, d_travel, d_escape, b.d_cnt, nullptr);
    if (rc != RT_OK) return rc;
    unsigned long long cnt = 0;
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(&cnt, b.d_cnt, sizeof cnt, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h_kind, d_kind, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && h_travel) e = hipMemcpy(h_travel, d_travel, n * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h_escape, d_escape, n * sizeof(rt_ray), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail_hip("rt_refract_rays_host", e);
    if (h_ray_count) *h_ray_count = cnt;
    return RT_OK;
}

/* ---- scatter queries (rt_scatter_query.hip) ---- */

#ifndef RT_SCATTER_PREPARE_DEFAULT
#define RT_SCATTER_PREPARE_DEFAULT 0
#endif

/* the checks of rt_scatter_hits before any device work, in the documented order; *done: nothing to launch */
static int scatter_hits_args(const char *who, const rt_scene *scene, const rt_rng *rng, size_t n, bool has_index, bool pointers_ok, bool *done) {
    const std::string w(who);
    *done = true;
    if ((uint64_t)n >= (1ull << 32)) return fail(RT_ERR_UNSUPPORTED, w + ": 2^32 records or more (checked first; query them in several calls)");
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, w + ": null scene");
    if (!rng) return fail(RT_ERR_INVALID_ARGUMENT, w + ": null rng");
    if (!has_index && n != rng_generator_count(rng))
        return fail(RT_ERR_INVALID_ARGUMENT, w + ": without an index array the RNG must hold as many generators as there are records");
    if (n == 0) return RT_OK;
    if (!pointers_ok) return fail(RT_ERR_INVALID_ARGUMENT, w + ": null hit, incoming-ray, type or scattered-ray pointer");
    *done = false;
    return RT_OK;
}

int rt_scatter_hits(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, rt_rng *rng, const uint32_t *d_rng_index,
                    uint32_t *d_type, rt_ray *d_scattered, float *d_cosine, void *hip_stream) {
    bool done;
    const int rc = scatter_hits_args("rt_scatter_hits", scene, rng, n, d_rng_index != nullptr, d_hits && d_incoming && d_type && d_scattered, &done);
    if (rc != RT_OK || done) return rc;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const bool prepare = rt::option(rt::OPT_SCATTER_PREPARE, RT_SCATTER_PREPARE_DEFAULT) != 0;
    uint32_t *d_states = nullptr;
    hipError_t e = rng_begin_draws(rng, prepare, stream, &d_states);
    if (e == hipSuccess)
        e = rt::launch_scatter_hits(scene->ks, d_hits, d_incoming, (uint32_t)n, d_states, (uint32_t)rng_generator_count(rng), d_rng_index, d_type,
                                    d_scattered, d_cosine, hit_query_band(), stream);
    if (e != hipSuccess) return fail_hip("rt_scatter_hits: launch", e);
    return RT_OK;
}

int rt_scatter_factors(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, const uint32_t *d_type, const rt_ray *d_next,
                       const float *d_travel, size_t n, float *d_rgb, void *hip_stream) {
    bool done;
    const int rc = hit_query_args("rt_scatter_factors", true, scene, n, d_hits && d_incoming && d_type && d_next && d_travel && d_rgb,
                                  "hit, incoming-ray, type, next-ray, travel or rgb", &done);
    if (rc != RT_OK || done) return rc;
    const hipError_t e = rt::launch_scatter_factors(scene->ks, d_hits, d_incoming, d_type, d_next, d_travel, (uint32_t)n, d_rgb, hit_query_band(),
                                                    static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail_hip("rt_scatter_factors: launch", e);
    return RT_OK;
}

int rt_scatter_hits_host(const rt_scene *scene, const rt_hit *h_hits, const rt_ray *h_incoming, size_t n, rt_rng *rng, const uint32_t *h_rng_index,
                         uint32_t *h_type, rt_ray *h_scattered, float *h_cosine) {
    bool done;
    int rc = scatter_hits_args("rt_scatter_hits_host", scene, rng, n, h_rng_index != nullptr, h_hits && h_incoming && h_type && h_scattered, &done);
    if (rc != RT_OK || done) return rc;
    HitQueryBuffers b;
    uint32_t *d_index = nullptr, *d_type = nullptr;
    rt_ray *d_scattered = nullptr;
    float *d_cosine = nullptr;
    hipError_t e = b.upload(h_hits, h_incoming, n);
    if (e == hipSuccess && h_rng_index) e = b.out(reinterpret_cast<void **>(&d_index), n * sizeof(uint32_t));
    if (e == hipSuccess && h_rng_index) e = hipMemcpy(d_index, h_rng_index, n * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = b.out(reinterpret_cast<void **>(&d_type), n * sizeof(uint32_t));
    if (e == hipSuccess) e = b.out(reinterpret_cast<void **>(&d_scattered), n * sizeof(rt_ray));
    if (e == hipSuccess && h_cosine) e = b.out(reinterpret_cast<void **>(&d_cosine), n * sizeof(float));
    if (e != hipSuccess) return fail_hip("rt_scatter_hits_host", e);
    rc = rt_scatter_hits(scene, b.d_hits, b.d_incoming, n, rng, d_index, d_type, d_scattered, d_cosine, nullptr);
    if (rc != RT_OK) return rc;
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(h_type, d_type, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h_scattered, d_scattered, n * sizeof(rt_ray), hipMemcpyDeviceToHost);
    if (e == hipSuccess && h_cosine) e = hipMemcpy(h_cosine, d_cosine, n * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail_hip("rt_scatter_hits_host", e);
    return RT_OK;
}

int rt_scatter_factors_host(const rt_scene *scene, const rt_hit *h_hits, const rt_ray *h_incoming, const uint32_t *h_type, const rt_ray *h_next,
                            const float *h_travel, size_t n, float *h_rgb) {
    bool done;
    int rc = hit_query_args("rt_scatter_factors_host", true, scene, n, h_hits && h_incoming && h_type && h_next && h_travel && h_rgb,
                            "hit, incoming-ray, type, next-ray, travel or rgb", &done);
    if (rc != RT_OK || done) return rc;
    HitQueryBuffers b;
    uint32_t *d_type = nullptr;
    rt_ray *d_next = nullptr;
    float *d_travel = nullptr, *d_rgb = nullptr;
    hipError_t e = b.upload(h_hits, h_incoming, n);
    if (e == hipSuccess) e = b.out(reinterpret_cast<void **>(&d_type), n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(d_type, h_type, n * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = b.out(reinterpret_cast<void **>(&d_next), n * sizeof(rt_ray));
    if (e == hipSuccess) e = hipMemcpy(d_next, h_next, n * sizeof(rt_ray), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = b.out(reinterpret_cast<void **>(&d_travel), n * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(d_travel, h_travel, n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = b.out(reinterpret_cast<void **>(&d_rgb), n * 3 * sizeof(float));
    if (e != hipSuccess) return fail_hip("rt_scatter_factors_host", e);
    rc = rt_scatter_factors(scene, b.d_hits, b.d_incoming, d_type, d_next, d_travel, n, d_rgb, nullptr);
    if (rc != RT_OK) return rc;
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(h_rgb, d_rgb, n * 3 * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail_hip("rt_scatter_factors_host", e);
    return RT_OK;
}

/* ---- the level loop (rt_level_query.hip; the indexed casts: rt_query.hip) ---- */

} /* extern "C" */

/* rt_select_records' block totals: RT_SELECT_MAX_GROUPS words per (device, stream), as rt_post_process_device keeps its scratch */
static std::mutex g_select_mutex;
static std::map<std::pair<int, hipStream_t>, uint32_t *> g_select_totals;

void select_release(int device) {
    std::lock_guard<std::mutex> lock(g_select_mutex);
    for (auto it = g_select_totals.begin(); it != g_select_totals.end();) {
        if (it->first.first == device) {
            if (it->second) (void)hipFree(it->second);
            it = g_select_totals.erase(it);
        } else {
            ++it;
        }
    }
}

extern "C" {

int rt_select_records(const unsigned char *d_flags, size_t n, uint32_t *d_index, uint32_t *d_count, void *hip_stream) {
    bool done;
    const int rc = hit_query_args("rt_select_records", false, nullptr, n, d_flags && d_index && d_count, "flag, index or count", &done);
    if (rc != RT_OK || done) return rc;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    int device = 0;
    RT_HIP(hipGetDevice(&device));
    uint32_t *totals = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_select_mutex);
        uint32_t *&slot = g_select_totals[std::make_pair(device, stream)];
        if (!slot) {
            hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(stream, &capturing) != hipSuccess) (void)hipGetLastError();
            if (capturing != hipStreamCaptureStatusNone)
                return fail(RT_ERR_UNSUPPORTED, "rt_select_records: the first call on a stream allocates its scratch and cannot be captured; call once uncaptured");
            RT_HIP(hipMalloc(reinterpret_cast<void **>(&slot), RT_SELECT_MAX_GROUPS * sizeof(uint32_t)));
        }
        totals = slot;
    }
    const hipError_t e = rt::launch_select_records(d_flags, (uint32_t)n, d_index, d_count, totals, stream);
    if (e != hipSuccess) return fail_hip("rt_select_records: launch", e);
    return RT_OK;
}

int rt_cast_rays_indexed(const rt_scene *scene, const rt_ray *d_rays, size_t n, const uint32_t *d_index, const uint32_t *d_count, size_t max_count,
                         rt_hit *d_hits, unsigned long long *d_ray_count, void *hip_stream) {
    if ((uint64_t)n >= (1ull << 32) || (uint64_t)max_count >= (1ull << 32))
        return fail(RT_ERR_UNSUPPORTED, "rt_cast_rays_indexed: 2^32 rays or index entries or more (checked first; cast them in several calls)");
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "rt_cast_rays_indexed: null scene");
    if (n == 0 || max_count == 0) return RT_OK;
    if (!d_rays || !d_index || !d_count || !d_hits) return fail(RT_ERR_INVALID_ARGUMENT, "rt_cast_rays_indexed: null ray, index, count or hit pointer");
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const bool wave_uniform = rt::option(rt::OPT_QUERY_WAVE_UNIFORM, 0) == 1;
    hipError_t e = hipSuccess;
    if (scene->ks.bfs_walk != 0u && !wave_uniform) {
        BfsLists bl;
        if (bfs_lists(scene, stream, (uint32_t)max_count, &bl)) {
            e = rt::launch_cast_rays_indexed_bfs(scene->ks, d_rays, d_hits, (uint32_t)n, d_index, d_count, (uint32_t)max_count, d_ray_count, bl.lists,
                                                 bl.items_cap, bl.jobs_cap, bl.groups, stream);
            if (e != hipSuccess) return fail_hip("rt_cast_rays_indexed: launch", e);
            return RT_OK;
        }
        /* no room for the lists (or a capture before the first call on this stream): the pair-wise kernel, exact as well */
    }
    e = rt::launch_cast_rays_indexed(scene->ks, d_rays, d_hits, (uint32_t)n, d_index, d_count, (uint32_t)max_count, d_ray_count, wave_uniform, stream);
    if (e != hipSuccess) return fail_hip("rt_cast_rays_indexed: launch", e);
    return RT_OK;
}

int rt_level_split(const rt_hit *d_hits, const uint32_t *d_type, const float *d_cosine, size_t n, rt_hit *d_hits_reflect, rt_hit *d_hits_refract,
                   void *hip_stream) {
    bool done;
    const int rc = hit_query_args("rt_level_split", false, nullptr, n, d_hits && d_type && d_cosine && d_hits_reflect && d_hits_refract,
                                  "hit, type, cosine or output", &done);
    if (rc != RT_OK || done) return rc;
    const hipError_t e = rt::launch_level_split(d_hits, d_type, d_cosine, (uint32_t)n, d_hits_reflect, d_hits_refract, static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail_hip("rt_level_split: launch", e);
    return RT_OK;
}

int rt_level_join(const uint32_t *d_type, const float *d_cosine, const rt_ray *d_reflected, const uint32_t *d_refr_kind, const rt_ray *d_escape, size_t n,
                  rt_ray *d_next, rt_hit *d_next_hits, unsigned char *d_flags, void *hip_stream) {
    bool done;
    const int rc = hit_query_args("rt_level_join", false, nullptr, n, d_type && d_cosine && d_reflected && d_refr_kind && d_escape && d_next && d_next_hits && d_flags,
                                  "type, cosine, reflected-ray, refraction-kind, escape-ray or output", &done);
    if (rc != RT_OK || done) return rc;
    const hipError_t e = rt::launch_level_join(d_type, d_cosine, d_reflected, d_refr_kind, d_escape, (uint32_t)n, d_next, d_next_hits, d_flags,
                                               static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail_hip("rt_level_join: launch", e);
    return RT_OK;
}

int rt_level_close(const rt_hit *d_hits, const uint32_t *d_type, const float *d_cosine, const rt_hit *d_next_hits, size_t n, rt_hit *d_hits_missed,
                   void *hip_stream) {
    bool done;
    const int rc = hit_query_args("rt_level_close", false, nullptr, n, d_hits && d_type && d_cosine && d_next_hits && d_hits_missed,
                                  "hit, type, cosine, next-hit or output", &done);
    if (rc != RT_OK || done) return rc;
    const hipError_t e = rt::launch_level_close(d_hits, d_type, d_cosine, d_next_hits, (uint32_t)n, d_hits_missed, static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail_hip("rt_level_close: launch", e);
    return RT_OK;
}

int rt_level_fold(const uint32_t *d_type, const float *d_cosine, const rt_hit *d_next_hits, const float *d_factor, const float *d_shade_next,
                  const float *d_shade_missed, size_t n, float *d_value, void *hip_stream) {
    bool done;
    const int rc = hit_query_args("rt_level_fold", false, nullptr, n, d_type && d_cosine && d_next_hits && d_factor && d_shade_next && d_shade_missed && d_value,
                                  "type, cosine, next-hit, factor, shade or value", &done);
    if (rc != RT_OK || done) return rc;
    const hipError_t e = rt::launch_level_fold(d_type, d_cosine, d_next_hits, d_factor, d_shade_next, d_shade_missed, (uint32_t)n, d_value,
                                               static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail_hip("rt_level_fold: launch", e);
    return RT_OK;
}

int rt_level_finish(const float *d_value, size_t n, float *d_accum, unsigned char *d_valid, void *hip_stream) {
    bool done;
    const int rc = hit_query_args("rt_level_finish", false, nullptr, n, d_value != nullptr, "value", &done);
    if (rc != RT_OK || done) return rc;
    if (!d_accum && !d_valid) return fail(RT_ERR_INVALID_ARGUMENT, "rt_level_finish: neither d_accum nor d_valid");
    const hipError_t e = rt::launch_level_finish(d_value, (uint32_t)n, d_accum, d_valid, static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail_hip("rt_level_finish: launch", e);
    return RT_OK;
}

} /* extern "C" */
