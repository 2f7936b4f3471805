/*
 * rt_api_query.hip — rt_cast_rays / rt_cast_rays_host / rt_camera_rays (include/rt_amd.h "ray queries"): validation, the
 * per-(scene, stream) workspace of a scene walked breadth-first, the launches of rt_query.hip; and rt_shade_hits / rt_reflect_rays /
 * rt_refract_rays with their _host forms ("hit queries"): validation and the launches of rt_hit_query.hip, no workspace; and
 * rt_scatter_hits / rt_scatter_factors with theirs ("scatter queries", rt_scatter_query.hip); and rt_camera_rays_offset with its _host
 * form ("film queries", rt_film_query.hip).  No CPU path: without a device every
 * call fails with a status.
 */
#include "rt_api_internal.h"

static_assert(sizeof(rt_ray) == 44 && sizeof(rt_hit) == 52, "the ABI records are flat u32 / f32 words");

/* The breadth-first walk's record lists for a cast of n rays (or index entries) on `stream` (rt_api_internal.h bfs_lists), for *groups
 * workgroups: one per CU at most.  lists == nullptr: no room for them, or a capture before the first call on this stream
 * (allocation cannot be captured). */
static BfsLists query_bfs_lists(const rt_scene *scene, hipStream_t stream, uint32_t n, uint32_t *groups_out) {
    const uint64_t cus = scene->resident_waves / (4u * (uint32_t)RT_MIN_WAVES);
    uint64_t groups = ((uint64_t)n + 64u * RT_QUERY_BFS_WAVES - 1u) / (64u * RT_QUERY_BFS_WAVES);
    if (groups > cus) groups = cus;
    if (groups < 1) groups = 1;
    static_assert(RT_QUERY_BFS_WAVES == 8u, "the lists are sized per wave of an 8-wave workgroup, as rt_render_whitted sizes them");
    const uint32_t waves = (uint32_t)groups * RT_QUERY_BFS_WAVES;
    *groups_out = (uint32_t)groups;
    rt_scene *mut = const_cast<rt_scene *>(scene); /* workspaces are the only mutable part of a scene */
    std::lock_guard<std::mutex> lock(mut->ws_mutex);
    Workspace &ws = mut->workspaces[stream];
    BfsLists bl = bfs_lists(ws, waves, false);
    if (bl.lists == nullptr && !stream_capturing(stream)) bl = bfs_lists(ws, waves, true); /* what is held is too small */
    return bl;
}

static const CountLimit CAST_RAYS_LIMIT = {32u, "rays", "cast them in several calls"};

extern "C" {

int rt_cast_rays(const rt_scene *scene, const rt_ray *d_rays, size_t n_rays, rt_hit *d_hits, void *hip_stream) {
    bool done;
    const int rc = query_args("rt_cast_rays", n_rays, CAST_RAYS_LIMIT, true, scene, d_rays && d_hits, "ray or hit", &done);
    if (rc != RT_OK || done) return rc;
    const uint32_t n = (uint32_t)n_rays;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const bool wave_uniform = rt::option(rt::OPT_QUERY_WAVE_UNIFORM, 0) == 1;
    if (scene->ks.bfs_walk != 0u && !wave_uniform) {
        uint32_t groups;
        const BfsLists bl = query_bfs_lists(scene, stream, n, &groups);
        if (bl.lists != nullptr)
            return launched("rt_cast_rays", rt::launch_cast_rays_bfs(scene->ks, d_rays, d_hits, n, bl.lists, bl.items_cap, bl.jobs_cap, groups, stream));
        /* no room for the lists (or a capture before the first call on this stream): the pair-wise kernel, exact as well */
    }
    return launched("rt_cast_rays", rt::launch_cast_rays(scene->ks, d_rays, d_hits, n, wave_uniform, stream));
}

int rt_cast_rays_host(const rt_scene *scene, const rt_ray *h_rays, size_t n_rays, rt_hit *h_hits) {
    bool done;
    int rc = query_args("rt_cast_rays_host", n_rays, CAST_RAYS_LIMIT, true, scene, h_rays && h_hits, "ray or hit", &done);
    if (rc != RT_OK || done) return rc;
    HostRoundTrip t("rt_cast_rays_host");
    const rt_ray *d_rays = t.in(h_rays, n_rays * sizeof(rt_ray));
    rt_hit *d_hits = t.out(h_hits, n_rays * sizeof(rt_hit));
    if (!t.ok()) return t.failed();
    rc = rt_cast_rays(scene, d_rays, n_rays, d_hits, nullptr);
    return rc != RT_OK ? rc : t.finish();
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
    return launched("rt_camera_rays", rt::launch_camera_rays(kf, d_rays, static_cast<hipStream_t>(hip_stream)));
}

/* Camera::shoot through a sub-pixel position (include/rt_amd.h "film queries"; kernel: rt_film_query.hip) */
static int camera_rays_offset_args(const char *who, const rt_camera *camera, const rt_frame *frame, const void *offsets, uint32_t spp, const void *rays,
                                   rt::KernelFrame *kf) {
    if (!camera || !frame) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": null argument");
    if (!frame_ok(frame)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": bad frame (need 0 <= x0 < x1 <= width, 0 <= y0 < y1 <= height, y_step >= 1)");
    if (spp < 1u) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": spp must be at least 1");
    rt_frame f = *frame;
    f.max_depth = 0; /* not used here */
    int rc = make_kernel_frame(camera, &f, kf); /* refuses a tile of 2^32 pixels or more */
    if (rc == RT_OK) rc = check_count(who, rt_frame_pixels(frame) * (uint64_t)spp, {32u, "rays", "make them in several calls"});
    if (rc == RT_OK) rc = check_pointers(who, offsets && rays, "offset or ray");
    return rc;
}

int rt_camera_rays_offset(const rt_camera *camera, const rt_frame *frame, const float *d_offsets, uint32_t spp, rt_ray *d_rays, void *hip_stream) {
    rt::KernelFrame kf;
    const int rc = camera_rays_offset_args("rt_camera_rays_offset", camera, frame, d_offsets, spp, d_rays, &kf);
    if (rc != RT_OK) return rc;
    return launched("rt_camera_rays_offset", rt::launch_camera_rays_offset(kf, d_offsets, spp, d_rays, static_cast<hipStream_t>(hip_stream)));
}

int rt_camera_rays_offset_host(const rt_camera *camera, const rt_frame *frame, const float *h_offsets, uint32_t spp, rt_ray *h_rays) {
    rt::KernelFrame kf;
    int rc = camera_rays_offset_args("rt_camera_rays_offset_host", camera, frame, h_offsets, spp, h_rays, &kf);
    if (rc != RT_OK) return rc;
    const size_t n = (size_t)rt_frame_pixels(frame) * spp;
    HostRoundTrip t("rt_camera_rays_offset_host");
    const float *d_offsets = t.in(h_offsets, n * 2u * sizeof(float));
    rt_ray *d_rays = t.out(h_rays, n * sizeof(rt_ray));
    if (!t.ok()) return t.failed();
    rc = rt_camera_rays_offset(camera, frame, d_offsets, spp, d_rays, nullptr);
    return rc != RT_OK ? rc : t.finish();
}

/* ---- hit queries (rt_hit_query.hip) ---- */

/* records per launch: RT_HITQ_BAND, or what the test hook asks for */
static uint32_t hit_query_band() { return band_limit(rt::OPT_DIAG_HIT_BAND_RECORDS, RT_HITQ_BAND); }

int rt_shade_hits(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, float *d_rgb, unsigned long long *d_ray_count,
                  void *hip_stream) {
    bool done;
    const int rc = query_args("rt_shade_hits", n, RECORDS_2_32, true, scene, d_hits && d_incoming && d_rgb, "hit, incoming-ray or rgb", &done);
    if (rc != RT_OK || done) return rc;
    const bool wave_uniform = rt::option(rt::OPT_QUERY_WAVE_UNIFORM, 0) == 1;
    return launched("rt_shade_hits", rt::launch_shade_hits(scene->ks, d_hits, d_incoming, (uint32_t)n, d_rgb, d_ray_count, wave_uniform, hit_query_band(),
                                               static_cast<hipStream_t>(hip_stream)));
}

int rt_reflect_rays(const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, rt_ray *d_out, void *hip_stream) {
    bool done;
    const int rc = query_args("rt_reflect_rays", n, RECORDS_2_32, false, nullptr, d_hits && d_incoming && d_out, "hit, incoming-ray or output", &done);
    if (rc != RT_OK || done) return rc;
    return launched("rt_reflect_rays", rt::launch_reflect_rays(d_hits, d_incoming, (uint32_t)n, d_out, hit_query_band(), static_cast<hipStream_t>(hip_stream)));
}

int rt_refract_rays(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, float max_distance, uint32_t *d_kind,
                    float *d_travel, rt_ray *d_escape, unsigned long long *d_ray_count, void *hip_stream) {
    bool done;
    const int rc = query_args("rt_refract_rays", n, RECORDS_2_32, true, scene, d_hits && d_incoming && d_kind && d_escape, "hit, incoming-ray, kind or escape-ray", &done);
    if (rc != RT_OK || done) return rc;
    const bool wave_uniform = rt::option(rt::OPT_QUERY_WAVE_UNIFORM, 0) == 1;
    return launched("rt_refract_rays", rt::launch_refract_rays(scene->ks, d_hits, d_incoming, (uint32_t)n, max_distance, d_kind, d_travel, d_escape, d_ray_count,
                                                 wave_uniform, hit_query_band(), static_cast<hipStream_t>(hip_stream)));
}

int rt_shade_hits_host(const rt_scene *scene, const rt_hit *h_hits, const rt_ray *h_incoming, size_t n, float *h_rgb, unsigned long long *h_ray_count) {
    bool done;
    int rc = query_args("rt_shade_hits_host", n, RECORDS_2_32, true, scene, h_hits && h_incoming && h_rgb, "hit, incoming-ray or rgb", &done);
    if (rc == RT_OK && done && h_ray_count) *h_ray_count = 0;
    if (rc != RT_OK || done) return rc;
    HostRoundTrip t("rt_shade_hits_host");
    const rt_hit *d_hits = t.in(h_hits, n * sizeof(rt_hit));
    const rt_ray *d_incoming = t.in(h_incoming, n * sizeof(rt_ray));
    float *d_rgb = t.out(h_rgb, n * 3 * sizeof(float));
    unsigned long long *d_cnt = t.counter();
    if (!t.ok()) return t.failed();
    rc = rt_shade_hits(scene, d_hits, d_incoming, n, d_rgb, d_cnt, nullptr);
    return rc != RT_OK ? rc : t.finish(h_ray_count);
}

int rt_refract_rays_host(const rt_scene *scene, const rt_hit *h_hits, const rt_ray *h_incoming, size_t n, float max_distance, uint32_t *h_kind,
                         float *h_travel, rt_ray *h_escape, unsigned long long *h_ray_count) {
    bool done;
    int rc = query_args("rt_refract_rays_host", n, RECORDS_2_32, true, scene, h_hits && h_incoming && h_kind && h_escape,
                        "hit, incoming-ray, kind or escape-ray", &done);
    if (rc == RT_OK && done && h_ray_count) *h_ray_count = 0;
    if (rc != RT_OK || done) return rc;
    HostRoundTrip t("rt_refract_rays_host");
    const rt_hit *d_hits = t.in(h_hits, n * sizeof(rt_hit));
    const rt_ray *d_incoming = t.in(h_incoming, n * sizeof(rt_ray));
    uint32_t *d_kind = t.out(h_kind, n * sizeof(uint32_t));
    float *d_travel = t.out(h_travel, n * sizeof(float)); /* optional */
    rt_ray *d_escape = t.out(h_escape, n * sizeof(rt_ray));
    unsigned long long *d_cnt = t.counter();
    if (!t.ok()) return t.failed();
    rc = rt_refract_rays(scene, d_hits, d_incoming, n, max_distance, d_kind, d_travel, d_escape, d_cnt, nullptr);
    return rc != RT_OK ? rc : t.finish(h_ray_count);
}

/* ---- scatter queries (rt_scatter_query.hip) ---- */

#ifndef RT_SCATTER_PREPARE_DEFAULT
#define RT_SCATTER_PREPARE_DEFAULT 0
#endif

/* the checks of rt_scatter_hits before any device work, in the documented order; *done: nothing to launch */
static int scatter_hits_args(const char *who, const rt_scene *scene, const rt_rng *rng, size_t n, bool has_index, bool pointers_ok, bool *done) {
    *done = true;
    int rc = check_count(who, n, RECORDS_2_32);
    if (rc == RT_OK) rc = check_scene(who, scene);
    if (rc != RT_OK) return rc;
    if (!rng) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": null rng");
    if (!has_index && n != rng_generator_count(rng))
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": without an index array the RNG must hold as many generators as there are records");
    if (n == 0) return RT_OK;
    rc = check_pointers(who, pointers_ok, "hit, incoming-ray, type or scattered-ray");
    *done = rc != RT_OK;
    return rc;
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
    return launched("rt_scatter_hits", e);
}

int rt_scatter_factors(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, const uint32_t *d_type, const rt_ray *d_next,
                       const float *d_travel, size_t n, float *d_rgb, void *hip_stream) {
    bool done;
    const int rc = query_args("rt_scatter_factors", n, RECORDS_2_32, true, scene, d_hits && d_incoming && d_type && d_next && d_travel && d_rgb,
                                  "hit, incoming-ray, type, next-ray, travel or rgb", &done);
    if (rc != RT_OK || done) return rc;
    return launched("rt_scatter_factors", rt::launch_scatter_factors(scene->ks, d_hits, d_incoming, d_type, d_next, d_travel, (uint32_t)n, d_rgb, hit_query_band(),
                                                    static_cast<hipStream_t>(hip_stream)));
}

int rt_scatter_hits_host(const rt_scene *scene, const rt_hit *h_hits, const rt_ray *h_incoming, size_t n, rt_rng *rng, const uint32_t *h_rng_index,
                         uint32_t *h_type, rt_ray *h_scattered, float *h_cosine) {
    bool done;
    int rc = scatter_hits_args("rt_scatter_hits_host", scene, rng, n, h_rng_index != nullptr, h_hits && h_incoming && h_type && h_scattered, &done);
    if (rc != RT_OK || done) return rc;
    HostRoundTrip t("rt_scatter_hits_host");
    const rt_hit *d_hits = t.in(h_hits, n * sizeof(rt_hit));
    const rt_ray *d_incoming = t.in(h_incoming, n * sizeof(rt_ray));
    const uint32_t *d_index = t.in(h_rng_index, n * sizeof(uint32_t)); /* optional */
    uint32_t *d_type = t.out(h_type, n * sizeof(uint32_t));
    rt_ray *d_scattered = t.out(h_scattered, n * sizeof(rt_ray));
    float *d_cosine = t.out(h_cosine, n * sizeof(float)); /* optional */
    if (!t.ok()) return t.failed();
    rc = rt_scatter_hits(scene, d_hits, d_incoming, n, rng, d_index, d_type, d_scattered, d_cosine, nullptr);
    return rc != RT_OK ? rc : t.finish();
}

int rt_scatter_factors_host(const rt_scene *scene, const rt_hit *h_hits, const rt_ray *h_incoming, const uint32_t *h_type, const rt_ray *h_next,
                            const float *h_travel, size_t n, float *h_rgb) {
    bool done;
    int rc = query_args("rt_scatter_factors_host", n, RECORDS_2_32, true, scene, h_hits && h_incoming && h_type && h_next && h_travel && h_rgb,
                        "hit, incoming-ray, type, next-ray, travel or rgb", &done);
    if (rc != RT_OK || done) return rc;
    HostRoundTrip t("rt_scatter_factors_host");
    const rt_hit *d_hits = t.in(h_hits, n * sizeof(rt_hit));
    const rt_ray *d_incoming = t.in(h_incoming, n * sizeof(rt_ray));
    const uint32_t *d_type = t.in(h_type, n * sizeof(uint32_t));
    const rt_ray *d_next = t.in(h_next, n * sizeof(rt_ray));
    const float *d_travel = t.in(h_travel, n * sizeof(float));
    float *d_rgb = t.out(h_rgb, n * 3 * sizeof(float));
    if (!t.ok()) return t.failed();
    rc = rt_scatter_factors(scene, d_hits, d_incoming, d_type, d_next, d_travel, n, d_rgb, nullptr);
    return rc != RT_OK ? rc : t.finish();
}

/* ---- the level loop (rt_level_query.hip; the indexed casts: rt_query.hip) ---- */

} /* extern "C" */

/* rt_select_records' block totals: RT_SELECT_MAX_GROUPS words per (device, stream), as rt_post_process_device keeps its scratch */
static std::mutex g_select_mutex;
static std::map<std::pair<int, hipStream_t>, DeviceBuffer> g_select_totals;

void select_release(int device) {
    std::lock_guard<std::mutex> lock(g_select_mutex);
    for (auto it = g_select_totals.begin(); it != g_select_totals.end();) {
        if (it->first.first == device) {
            (void)it->second.release();
            it = g_select_totals.erase(it);
        } else {
            ++it;
        }
    }
}

extern "C" {

int rt_select_records(const unsigned char *d_flags, size_t n, uint32_t *d_index, uint32_t *d_count, void *hip_stream) {
    bool done;
    const int rc = query_args("rt_select_records", n, RECORDS_2_32, false, nullptr, d_flags && d_index && d_count, "flag, index or count", &done);
    if (rc != RT_OK || done) return rc;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    int device = 0;
    RT_HIP(hipGetDevice(&device));
    uint32_t *totals = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_select_mutex);
        DeviceBuffer &slot = g_select_totals[std::make_pair(device, stream)];
        if (slot.bytes() == 0) {
            if (stream_capturing(stream))
                return fail(RT_ERR_UNSUPPORTED, "rt_select_records: the first call on a stream allocates its scratch and cannot be captured; call once uncaptured");
            const hipError_t e = slot.reserve(RT_SELECT_MAX_GROUPS * sizeof(uint32_t));
            if (e != hipSuccess) return fail_hip("hipMalloc(reinterpret_cast<void **>(&slot), RT_SELECT_MAX_GROUPS * sizeof(uint32_t))", e);
        }
        totals = slot.get<uint32_t>();
    }
    return launched("rt_select_records", rt::launch_select_records(d_flags, (uint32_t)n, d_index, d_count, totals, stream));
}

int rt_cast_rays_indexed(const rt_scene *scene, const rt_ray *d_rays, size_t n, const uint32_t *d_index, const uint32_t *d_count, size_t max_count,
                         rt_hit *d_hits, unsigned long long *d_ray_count, void *hip_stream) {
    int rc = check_count("rt_cast_rays_indexed", std::max<uint64_t>(n, max_count), {32u, "rays or index entries", "cast them in several calls"});
    if (rc == RT_OK) rc = check_scene("rt_cast_rays_indexed", scene);
    if (rc != RT_OK || n == 0 || max_count == 0) return rc;
    rc = check_pointers("rt_cast_rays_indexed", d_rays && d_index && d_count && d_hits, "ray, index, count or hit");
    if (rc != RT_OK) return rc;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const bool wave_uniform = rt::option(rt::OPT_QUERY_WAVE_UNIFORM, 0) == 1;
    if (scene->ks.bfs_walk != 0u && !wave_uniform) {
        uint32_t groups;
        const BfsLists bl = query_bfs_lists(scene, stream, (uint32_t)max_count, &groups);
        if (bl.lists != nullptr)
            return launched("rt_cast_rays_indexed", rt::launch_cast_rays_indexed_bfs(scene->ks, d_rays, d_hits, (uint32_t)n, d_index, d_count, (uint32_t)max_count,
                                                                                     d_ray_count, bl.lists, bl.items_cap, bl.jobs_cap, groups, stream));
        /* no room for the lists (or a capture before the first call on this stream): the pair-wise kernel, exact as well */
    }
    return launched("rt_cast_rays_indexed", rt::launch_cast_rays_indexed(scene->ks, d_rays, d_hits, (uint32_t)n, d_index, d_count, (uint32_t)max_count, d_ray_count,
                                                                         wave_uniform, stream));
}

int rt_level_split(const rt_hit *d_hits, const uint32_t *d_type, const float *d_cosine, size_t n, rt_hit *d_hits_reflect, rt_hit *d_hits_refract,
                   void *hip_stream) {
    bool done;
    const int rc = query_args("rt_level_split", n, RECORDS_2_32, false, nullptr, d_hits && d_type && d_cosine && d_hits_reflect && d_hits_refract,
                                  "hit, type, cosine or output", &done);
    if (rc != RT_OK || done) return rc;
    return launched("rt_level_split", rt::launch_level_split(d_hits, d_type, d_cosine, (uint32_t)n, d_hits_reflect, d_hits_refract, static_cast<hipStream_t>(hip_stream)));
}

int rt_level_join(const uint32_t *d_type, const float *d_cosine, const rt_ray *d_reflected, const uint32_t *d_refr_kind, const rt_ray *d_escape, size_t n,
                  rt_ray *d_next, rt_hit *d_next_hits, unsigned char *d_flags, void *hip_stream) {
    bool done;
    const int rc = query_args("rt_level_join", n, RECORDS_2_32, false, nullptr, d_type && d_cosine && d_reflected && d_refr_kind && d_escape && d_next && d_next_hits && d_flags,
                                  "type, cosine, reflected-ray, refraction-kind, escape-ray or output", &done);
    if (rc != RT_OK || done) return rc;
    return launched("rt_level_join", rt::launch_level_join(d_type, d_cosine, d_reflected, d_refr_kind, d_escape, (uint32_t)n, d_next, d_next_hits, d_flags,
                                               static_cast<hipStream_t>(hip_stream)));
}

int rt_level_close(const rt_hit *d_hits, const uint32_t *d_type, const float *d_cosine, const rt_hit *d_next_hits, size_t n, rt_hit *d_hits_missed,
                   void *hip_stream) {
    bool done;
    const int rc = query_args("rt_level_close", n, RECORDS_2_32, false, nullptr, d_hits && d_type && d_cosine && d_next_hits && d_hits_missed,
                                  "hit, type, cosine, next-hit or output", &done);
    if (rc != RT_OK || done) return rc;
    return launched("rt_level_close", rt::launch_level_close(d_hits, d_type, d_cosine, d_next_hits, (uint32_t)n, d_hits_missed, static_cast<hipStream_t>(hip_stream)));
}

int rt_level_fold(const uint32_t *d_type, const float *d_cosine, const rt_hit *d_next_hits, const float *d_factor, const float *d_shade_next,
                  const float *d_shade_missed, size_t n, float *d_value, void *hip_stream) {
    bool done;
    const int rc = query_args("rt_level_fold", n, RECORDS_2_32, false, nullptr, d_type && d_cosine && d_next_hits && d_factor && d_shade_next && d_shade_missed && d_value,
                                  "type, cosine, next-hit, factor, shade or value", &done);
    if (rc != RT_OK || done) return rc;
    return launched("rt_level_fold", rt::launch_level_fold(d_type, d_cosine, d_next_hits, d_factor, d_shade_next, d_shade_missed, (uint32_t)n, d_value,
                                               static_cast<hipStream_t>(hip_stream)));
}

int rt_level_finish(const float *d_value, size_t n, float *d_accum, unsigned char *d_valid, void *hip_stream) {
    bool done;
    const int rc = query_args("rt_level_finish", n, RECORDS_2_32, false, nullptr, d_value != nullptr, "value", &done);
    if (rc != RT_OK || done) return rc;
    if (!d_accum && !d_valid) return fail(RT_ERR_INVALID_ARGUMENT, "rt_level_finish: neither d_accum nor d_valid");
    return launched("rt_level_finish", rt::launch_level_finish(d_value, (uint32_t)n, d_accum, d_valid, static_cast<hipStream_t>(hip_stream)));
}

} /* extern "C" */
