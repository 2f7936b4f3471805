/*
 * rt_api_query.hip — rt_cast_rays / rt_cast_rays_host / rt_camera_rays (include/rt_amd.h "ray queries"): validation, the
 * per-(scene, stream) workspace of a scene walked breadth-first, the launches of rt_query.hip.  No CPU path: without a device
 * every call fails with a status.
 */
#include "rt_api_internal.h"

static_assert(sizeof(rt_ray) == 44 && sizeof(rt_hit) == 52, "the ABI records are flat u32 / f32 words");

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
        /* the breadth-first walk's record lists: per wave of the grid, in the workspace rt_render_whitted keeps them in (sized and grown
         * as there: workgroups x 8 waves x pwf_bfs_scratch_words_per_wave), one workgroup per CU at most */
        const uint64_t cus = scene->resident_waves / (4u * (uint32_t)RT_MIN_WAVES);
        uint64_t groups = ((uint64_t)n + 64u * RT_QUERY_BFS_WAVES - 1u) / (64u * RT_QUERY_BFS_WAVES);
        if (groups > cus) groups = cus;
        if (groups < 1) groups = 1;
        static_assert(RT_QUERY_BFS_WAVES == 8u, "the lists are sized per wave of an 8-wave workgroup, as rt_render_whitted sizes them");
        const size_t words = (size_t)groups * RT_QUERY_BFS_WAVES * rt::pwf_bfs_scratch_words_per_wave();
        uint32_t *lists = nullptr;
        uint32_t items_cap = RT_BFS_ITEMS_CAP, jobs_cap = RT_BFS_JOBS_CAP;
        {
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
            if (ws.d_bfs != nullptr && ws.bfs_words >= words) lists = ws.d_bfs;
            const long long cap = rt::option(rt::OPT_DIAG_BFS_CAP, 0); /* test hook: shorter lists (the memory is the same) */
            if (cap > 0) {
                items_cap = (uint32_t)std::min<long long>(cap, RT_BFS_ITEMS_CAP);
                jobs_cap = (uint32_t)std::min<long long>(cap, RT_BFS_JOBS_CAP);
            }
        }
        if (lists != nullptr) {
            e = rt::launch_cast_rays_bfs(scene->ks, d_rays, d_hits, n, lists, items_cap, jobs_cap, (uint32_t)groups, stream);
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

} /* extern "C" */
