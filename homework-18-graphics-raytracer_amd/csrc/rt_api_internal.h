/*
 * rt_api_internal.h — what the translation units behind include/rt_amd.h share: the scene handle with its per-stream
 * workspaces, the status/error helpers, the frame checks, and the host plumbing every entry point is made of (argument checks, the
 * launch tail, the band loop, the round trip of a _host form).  Internal (hidden visibility): the library's exports are the
 * extern "C" entry points of include/rt_amd.h and nothing else.
 *
 *   rt_api.hip         errors and the shared host plumbing declared below, settings, profiling, rt_scene_create/destroy,
 *                      rt_render_whitted (the per-stream arenas), rt_trace_rays, and the diagnostics that report their plan and
 *                      outcome (rt_diag_pwf_plan / _plan_rays / _outcome)
 *   rt_api_layout.hip  the device records and the node tree built from the ABI arrays — host only, no HIP call
 *   rt_api_dist.hip    rt_rng_*, rt_render_distributed and rt_trace_rays_distributed: batches, the two workspaces, the streams of a
 *                      pipelined call
 *   rt_api_multi.hip   rt_multi_*: a device list from one process
 *   rt_api_post.hip    post_process / sRGB / accumulator / rt_math_eval entry points
 *   rt_api_query.hip   rt_cast_rays / rt_camera_rays, the hit queries rt_shade_hits / rt_reflect_rays / rt_refract_rays, the scatter
 *                      queries rt_scatter_hits / rt_scatter_factors and the level loop's rt_select_records / rt_cast_rays_indexed /
 *                      rt_level_*
 *   rt_tree_query.hip  the tree loop's rt_tree_*: kernels and entry points in one unit
 *   rt_light_query.hip the light queries' rt_light_*: kernels and entry points in one unit
 *   rt_area_light_query.hip the area-light queries' rt_area_light_*: kernels and entry points in one unit (the sampler is rt_area_light.h's, shared
 *                      with librt_host.so; the per-hit record, the shadow ray and the light-term body rt_light_record.h's, shared with
 *                      rt_light_query.hip and the other hit-sample units; their entry points' checks are hit_sample_args below)
 *   rt_hemisphere_query.hip the hemisphere queries' rt_hemisphere_rays / rt_hemisphere_fold: kernels and entry points in one unit (the sampler and the
 *                      fold are rt_hemisphere.h's, shared with librt_host.so)
 *   rt_environment_query.hip the environment queries' rt_environment_lookup / _table / _rays / _fold: kernels and entry points in one unit (the arithmetic
 *                      is rt_environment.h's, shared with librt_host.so)
 *   rt_path_query.hip  the path queries' rt_path_begin / rt_path_advance / rt_path_resolve: kernels and entry points in one unit (the record, the step
 *                      and the resolve are rt_path.h's, shared with librt_host.so; the step calls rt_lobe.h's sampler and rt_shade.h's terms)
 *   rt_refract_query.hip the refraction queries' rt_refract_enter / rt_refract_step: kernels and entry points in one unit
 *   rt_scene_update.hip the scene updates' rt_scene_update_*: kernels and entry points in one unit
 *   rt_motion_query.hip the motion queries' rt_scene_keep_positions / rt_scene_positions_kept / rt_previous_positions and its _host form: kernels and entry points in one unit
 *   rt_order_query.hip the record ordering's rt_ray_keys / rt_sort_records / rt_gather_records / rt_scatter_records: kernels and entry points in one unit
 *   rt_mesh_order.hip  the mesh ordering's rt_triangle_keys / rt_order_triangles: the key kernel and entry points that call rt_order_query.hip's
 *   rt_material_query.hip the material queries' rt_material_hits / rt_probe_surfaces: kernels and entry points in one unit
 *   rt_denoise_query.hip the denoise queries' rt_denoise_atrous / rt_denoise_atrous_host / rt_denoise_temp_bytes: kernels and entry points in one unit
 *   rt_temporal_query.hip the temporal queries' rt_temporal_motion / rt_temporal_accumulate and their _host forms: kernels and entry points in one unit
 *   rt_rectify_query.hip the history rectification queries' rt_temporal_bounds / rt_temporal_accumulate_bounded / rt_temporal_feedback and their _host forms: kernels and entry points in one unit
 *   rt_adaptive_query.hip the adaptive sampling queries' rt_sample_budget / rt_sample_list / rt_film_offsets_listed / rt_camera_rays_listed / rt_film_splat_listed: kernels and entry points in one unit
 *   rt_upsample_query.hip the guided upsampling queries' rt_upsample_guided and its _host form: kernels and entry points in one unit
 *   rt_bloom_query.hip   the bloom queries' rt_bloom / rt_bloom_host / rt_bloom_temp_bytes: kernels and entry points in one unit
 *   rt_svgf_query.hip    the variance-guided filter queries' rt_svgf_variance / rt_svgf_atrous, their _host forms and rt_svgf_temp_bytes: kernels and entry points in one unit
 * The image-side units from rt_denoise_query.hip on state each query's arguments once, as the struct of rt_query_args.h in the query's
 * shared header; their device and _host entry points are device_query / host_query below, one statement each (rt_sample_list,
 * rt_camera_rays_listed and the splats keep bodies of their own).
 * The film queries' kernels are rt_film_query.hip; their entry points are rt_api_query.hip's (rt_camera_rays_offset, beside rt_camera_rays) and
 * rt_api_post.hip's (rt_film_offsets / rt_film_splat, beside the accumulator).  The two splats, rt_film_query.hip's and
 * rt_adaptive_query.hip's, instantiate the kernel templates of rt_film_splat_kernel.h, each with its layout (rt_film.h, rt_adaptive.h).
 * The two A-Trous filters, rt_denoise_query.hip and rt_svgf_query.hip, instantiate the kernel templates of rt_atrous_kernel.h, each with
 * its filter (rt_denoise.h, rt_svgf.h) on the shared walk, guide readers and argument checks of rt_atrous.h.
 * The kernel units rt_hit_query.hip and rt_scatter_query.hip include this header for the band loop of their launchers.
 *
 * No unit includes another unit's source.  What two kernel units share is a header: the render kernels that are instantiated once for
 * camera frames and once for ray batches are templates in rt_whitted_kernel.h (rt_kernels.hip, rt_kernels_rays.hip), rt_pwf_kernel.h
 * (rt_pwf.hip, rt_pwf_rays.hip) and rt_dist_kernels.h (rt_distributed.hip, rt_distributed_rays.hip), and the stochastic pass's
 * generator is rt_rng.h (those two and rt_scatter_query.hip).  Every *.hip of this directory is one object of the Makefile.
 */
#ifndef RT_API_INTERNAL_H
#define RT_API_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <deque>
#include <functional>
#include <cmath>
#include <limits>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/rt_amd.h"
#include "rt_device_scene.h"
#include "rt_kernels.h"
#include "rt_vec.h"
#include "rt_luma.h"
#include "rt_film.h"
#include "rt_query_args.h"

#define RT_API_HIDDEN __attribute__((visibility("hidden")))

/* A device (or pinned host) allocation and the size it really has: every persistent buffer of the library is one of these.
 * reserve() grows only: a request beyond what is held frees, then allocates; when that fails the buffer holds nothing, the sticky HIP
 * error is cleared and the error is returned — what a failure means is each caller's business.  Move-only, and no HIP call in the
 * destructor (statics outlive the runtime, and a buffer is freed with its own device current): release() is called by whoever owns
 * the buffer, where the comments below say.  Definitions: rt_api.hip. */
class RT_API_HIDDEN DeviceBuffer {
public:
    enum Kind { DEVICE, PINNED_HOST };
    explicit DeviceBuffer(Kind kind = DEVICE) : kind_(kind) {}
    DeviceBuffer(DeviceBuffer &&o) noexcept : p_(o.p_), bytes_(o.bytes_), kind_(o.kind_) { o.p_ = nullptr; o.bytes_ = 0; }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept { std::swap(p_, o.p_); std::swap(bytes_, o.bytes_); std::swap(kind_, o.kind_); return *this; }
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    hipError_t reserve(size_t bytes);
    hipError_t release(); /* the status of the free; holds nothing afterwards either way, and may be called again */
    template <class T> T *get() const { return static_cast<T *>(p_); }
    size_t bytes() const { return bytes_; }

private:
    void *p_ = nullptr;
    size_t bytes_ = 0;
    Kind kind_;
};

/* Per-(scene, stream) scratch.  Launches on one stream are ordered, so they can share it; other streams get their own.  Grow-only;
 * allocated on the first call that needs it.  The scene owns its workspaces: they are made and changed under rt_scene::ws_mutex only,
 * by rt_render_whitted / rt_trace_rays (arenas, lists), rt_render_distributed / rt_trace_rays_distributed (split, lists, counters) and
 * rt_cast_rays / rt_cast_rays_indexed (lists), and rt_scene_destroy frees them all. */
#define RT_WS_COUNTER_BYTES 256u
struct Workspace {
    uint32_t *d_counters = nullptr; /* RT_WS_COUNTER_BYTES, zeroed once: [0] the stochastic pass's chunk counter */
    DeviceBuffer d_pwf; /* persistent-wavefront path: two blocks of global words, the frame description, one arena per workgroup */
    /* Launches on this workspace alternate between the two blocks of global words: a launch's last workgroup zeroes the
     * other block, so the next launch needs no preparation of its own unless its frame description differs from what is in
     * device memory (or nothing has run here yet). */
    uint32_t pw_parity = 0;
    bool pw_ready = false;
    bool pw_always_prepare = false; /* a call on this stream was captured into a graph: replays come unannounced, so from then on
                                     * every launch prepares its own block and frame description, as a captured one does */
    rt::KernelFrame pw_frame;
    int pw_last_block = -1; /* the block the last call's launch(es) of the persistent kernel took; -1: that call launched none.  The
                             * block stays as the kernel left it until the next launch here (rt_diag_pwf_outcome reads it) */
    DeviceBuffer d_bfs;   /* a scene walked breadth-first: item and job lists per wave (rt_kernels.h PwParams), through bfs_lists() below */
    DeviceBuffer d_split; /* split distributed pass: requests, shades and frames of one batch of epochs */
    void drop_arenas() { (void)d_pwf.release(); pw_ready = false; pw_last_block = -1; } /* whatever the blocks held went with them */
};

/* The breadth-first walk's record lists for a grid of `waves` waves, in the stream's workspace (the Whitted frame, the one-kernel
 * stochastic pass and the ray queries of one stream share them): grown to that many waves when may_allocate, and `lists` is null when
 * what is held is too small.  The caps: RT_BFS_ITEMS_CAP / RT_BFS_JOBS_CAP, or what the test hook RT_AMD_DIAG_BFS_CAP shortens them
 * to (the memory is the same).  Call under the scene's ws_mutex.  Definition: rt_api.hip. */
struct BfsLists {
    uint32_t *lists;
    uint32_t items_cap, jobs_cap;
};
RT_API_HIDDEN BfsLists bfs_lists(Workspace &ws, uint32_t waves, bool may_allocate);

inline hipError_t ensure_counters(Workspace &ws) {
    if (ws.d_counters) return hipSuccess;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&ws.d_counters), RT_WS_COUNTER_BYTES);
    if (e == hipSuccess) e = hipMemset(ws.d_counters, 0, RT_WS_COUNTER_BYTES);
    return e;
}

/* What the scene updates (rt_scene_update.hip) need beyond KernelScene.  A node that rt_scene_create built with a bounding sphere — every
 * inner node, every clustered leaf — is refitted over its unchanged triangle range [lo, hi); leaves that were plain at creation stay
 * plain and are not listed. */
struct RefitNode {
    uint32_t lo, hi;  /* the triangles below the node */
    uint32_t seg;     /* its index in KernelScene::segments (pre-order) ... */
    uint32_t bfs_pos; /* ... and in bfs_nodes / bfs_soa (level order) */
};
#define RT_REFIT_WAVE_MAX 1024u /* a node of up to this many triangles is refitted by one wave, a larger one by a workgroup */
struct SceneUpdate { /* the buffers and the event: freed by rt_scene_destroy */
    double extent = 0.0;          /* the scene's box at creation: fixed (KernelScene::filter_origin2 travels by value) */
    std::vector<RefitNode> nodes; /* kept on the host by rt_scene_create, uploaded with the first rt_scene_update_vertices */
    std::mutex mutex;
    bool uploaded = false;
    DeviceBuffer d_nodes;         /* RefitNode: n_small nodes for a wave each, then n_large for a workgroup each */
    uint32_t n_small = 0, n_large = 0;
    DeviceBuffer h_stage{DeviceBuffer::PINNED_HOST}; /* the light and material records of one call on their way to the device */
    hipEvent_t stage_event = nullptr; /* recorded after that call's copies */
};

/* What the motion queries (rt_motion_query.hip) keep of a scene: the positions as they stood at the last rt_scene_keep_positions, in the
 * pieces of rt_motion.h.  Allocated by the first keep under the mutex, the size fixed from then on (the counts of a scene never change);
 * freed by rt_scene_destroy. */
struct KeptPositions {
    std::mutex mutex;
    std::atomic<bool> kept{false}; /* rt_scene_keep_positions has been called (true also for a scene with nothing to keep) */
    DeviceBuffer d_pieces;
};

using rt::light_aux_of; /* rt_shade.h: a spot light's cone edge as a cosine, with margins */

struct rt_scene {
    int device;
    void *d_blob; /* one allocation holding every array */
    rt::KernelScene ks;
    uint32_t resident_waves; /* CUs * 4 SIMDs * RT_MIN_WAVES: the persistent grid */
    uint32_t pwf_workgroups;  /* CUs * resident workgroups of the persistent-wavefront kernel */
    std::mutex ws_mutex;
    std::map<hipStream_t, Workspace> workspaces;
    SceneUpdate upd;
    KeptPositions kept;
};

/* rt_last_error() of the calling thread.  (Thread-local state is reached through functions of the translation unit that defines
 * it: an `extern thread_local` of hidden visibility makes the other units call its weak, undefined initialisation function through
 * a PC-relative address that is not null — a jump to the library's first byte.) */
RT_API_HIDDEN std::string &last_error();
RT_API_HIDDEN int fail(int code, const std::string &msg);
RT_API_HIDDEN int fail_hip(const char *what, hipError_t e);
#define RT_HIP(call)                                          \
    do {                                                      \
        hipError_t e_ = (call);                               \
        if (e_ != hipSuccess) return fail_hip(#call, e_);     \
    } while (0)

/* ---- the host plumbing of an entry point (definitions: rt_api.hip, next to fail / fail_hip) ---- */

/* The argument checks, in the house order: the count limit first, then a null scene (reported even for an empty batch), then "nothing
 * to do", then the pointers.  Each returns RT_OK or what fail() returned; the text is put together only when a check fails.
 * A limit reads "<who>: 2^<log2> <noun> or more (checked first; <advice>)"; advice may be null. */
struct CountLimit {
    unsigned log2;
    const char *noun, *advice;
};
constexpr CountLimit RECORDS_2_32 = {32u, "records", "query them in several calls"};
RT_API_HIDDEN int check_count(const char *who, uint64_t n, const CountLimit &limit);
RT_API_HIDDEN int check_scene(const char *who, const void *scene);
RT_API_HIDDEN int check_pointers(const char *who, bool ok, const char *names); /* "<who>: null <names> pointer" */
/* ... and the four of them composed; *done: nothing to launch (a failed check or an empty batch).  An entry point with a check of its
 * own in between composes the three above itself. */
RT_API_HIDDEN int query_args(const char *who, size_t n, const CountLimit &limit, bool needs_scene, const void *scene, bool pointers_ok,
                             const char *names, bool *done);

/* The checks of a hit-sample query — the light, area-light, hemisphere, environment, lobe, texture and material blocks' calls on n
 * records times lights, probes or samples — in the documented order: 1 the counts (records, then records x lights or probes, then
 * those x samples), 2 the scene, 3 the descriptor, 4 the empty batch (no records, no lights, no probes: RT_OK, *done), 5 the pointers,
 * 6 the block's limits, 7 the light range.  A call states what it takes and leaves the rest out. */
constexpr CountLimit LIGHT_PAIRS_2_32 = {32u, "(record, light) pairs", "pass the lights in several ranges"};
constexpr CountLimit PROBE_PAIRS_2_32 = {32u, "(record, probe) pairs", "pass the probes in several calls"};
constexpr CountLimit SAMPLE_ENTRIES_2_32 = {32u, "(sample, record) entries", "query the records in several calls, or fewer samples"};
constexpr CountLimit SAMPLE_LIGHT_ENTRIES_2_32 = {32u, "(sample, light, record) entries", "pass the lights in several ranges, or fewer samples"};
struct HitSampleArgs {
    HitSampleArgs(size_t n, bool pointers_ok, const char *pointers) : n(n), pointers_ok(pointers_ok), pointers(pointers) {}
    size_t n; /* records */
    bool pointers_ok;
    const char *pointers;                /* the names of "<who>: null <names> pointer" */
    bool takes_scene = true;
    std::function<int()> descriptor;     /* the check of the call's descriptor, run in its place in the order; empty: the call has none */
    const CountLimit *pairs = nullptr;   /* the call takes `per_record` lights or probes per record: their limit */
    uint32_t per_record = 1u;
    bool of_lights = false;              /* ... and they are lights: the samples' limit names them */
    int64_t light_first = -1;            /* < 0: no range of the scene's lights */
    bool takes_samples = false;
    uint32_t spp = 0u;
    const char *bad = nullptr;           /* what the block's limits (the *_limits of its header) say, or null */
    HitSampleArgs &no_scene() { takes_scene = false; return *this; }
    HitSampleArgs &described(std::function<int()> check) { descriptor = std::move(check); return *this; }
    HitSampleArgs &lights(uint32_t count, int64_t first = -1) { pairs = &LIGHT_PAIRS_2_32, per_record = count, of_lights = true, light_first = first; return *this; }
    HitSampleArgs &probes(uint32_t count) { pairs = &PROBE_PAIRS_2_32, per_record = count; return *this; }
    HitSampleArgs &samples(uint32_t count) { takes_samples = true, spp = count; return *this; }
    HitSampleArgs &limits(const char *text) { bad = text; return *this; }
};
RT_API_HIDDEN int hit_sample_args(const char *who, const rt_scene *scene, const HitSampleArgs &a, bool *done);

static inline bool aligned_16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0u; }
static inline bool aligned_8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0u; }

/* The checks of a path-loop call on listed rt_path records (the path, transmission, connection and light-connection blocks):
 * hit_sample_args with the record pointer and the list pair — an index comes with its count — among the pointers, `a` stating the
 * call's own operands and every name of the text, and after everything else the record's alignment. */
static inline int listed_path_args(const char *who, const rt_scene *scene, const rt_path *d_paths, const uint32_t *d_index, const uint32_t *d_count,
                                   HitSampleArgs a, bool *done) {
    a.pointers_ok = a.pointers_ok && d_paths && (d_index == nullptr || d_count != nullptr);
    const int rc = hit_sample_args(who, scene, a, done);
    if (rc != RT_OK || *done) return rc;
    if (!aligned_16(d_paths)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": d_paths is not 16-byte aligned");
    return RT_OK;
}

/* a descriptor's limits (rt::environment_limits, rt::texture_limits) under the entry point's name */
template <class Desc>
static inline int check_descriptor(const char *who, const Desc *d, const char *(*limits)(const Desc *, bool *)) {
    bool unsupported;
    if (const char *bad = limits(d, &unsupported)) return fail(unsupported ? RT_ERR_UNSUPPORTED : RT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + bad);
    return RT_OK;
}

/* the end of an entry point that launched: RT_OK, or "<who>: launch: <the HIP error>" with its status */
RT_API_HIDDEN int launched(const char *who, hipError_t e);
static inline int launched(const char *who) { return launched(who, hipGetLastError()); }

static inline dim3 grid_of(uint64_t n, uint32_t threads) { return dim3((unsigned)((n + threads - 1u) / threads)); }

/* is `stream` being captured into a graph (then nothing may be allocated, and host memory is not read later) */
RT_API_HIDDEN bool stream_capturing(hipStream_t stream);

/* Bands: no launch takes more than `band` records, a multiple of 64 so that bands are whole 64-record chunks.  band_limit: `limit`, or
 * what the test hook `hook` asks for, in whole chunks.  for_each_band: launch(off, len) for every band of n records; the start of a
 * band is counted in 64 bits (n may be anything below 2^32, and the start of the band after the last one need not fit 32 bits). */
static inline uint64_t round_up_64(uint64_t x) { return (x + 63u) & ~(uint64_t)63u; }
static inline uint32_t band_limit(rt::Option hook, uint32_t limit) {
    const long long h = rt::option(hook, 0);
    return h > 0 && h < (long long)limit ? (uint32_t)round_up_64((uint64_t)h) : limit;
}
/* Workgroups: a grid-stride kernel is launched with at most `limit` of them, or with what the test hook `hook` asks for, 1 .. limit, so
 * that a small image or batch is taken grid-stride; a smaller cap changes no bit.  The image-side kernels' launchers are
 * rt_image_kernel.h's, which take the hook. */
static inline uint32_t max_groups(rt::Option hook, uint32_t limit) {
    const long long cap = rt::option(hook, limit);
    return cap >= 1 && cap < (long long)limit ? (uint32_t)cap : limit;
}
template <class Launch>
static inline hipError_t for_each_band(uint32_t n, uint32_t band, Launch launch) {
    for (uint64_t off = 0u; off < n; off += band) {
        launch(off, (uint32_t)(n - off < band ? n - off : band));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

/* The round trip of a _host form: device copies of the caller's arrays, the device form on the null stream, the results back.  A null
 * host pointer is an optional array the caller left out: nothing is allocated and the device pointer is null.  The first HIP error
 * sticks: every later step is skipped, ok() is false and failed() reports it under the entry point's name.  finish(): one
 * hipDeviceSynchronize, the downloads in declaration order, then the counter (*h_count is written last, and only if all went well).
 * A strided plane — n pixels, `stride` words apart, `width` words each — travels as the span from its first word to its last: (n - 1)
 * strides and one width.  The destructor frees everything, whichever way the call ends. */
class RT_API_HIDDEN HostRoundTrip {
public:
    explicit HostRoundTrip(const char *who) : who_(who) {}
    ~HostRoundTrip();
    HostRoundTrip(const HostRoundTrip &) = delete;
    HostRoundTrip &operator=(const HostRoundTrip &) = delete;
    template <class T> T *in(const T *h, size_t bytes) { return static_cast<T *>(add(const_cast<T *>(h), bytes, h != nullptr, true, false)); }
    template <class T> T *plane(const T *h, size_t n, uint32_t stride, uint32_t width) { return in(h, ((n - 1u) * stride + width) * sizeof(uint32_t)); }
    /* the four planes of n pixels of a guides struct (albedo only where the call reads it): a copy of *h, held here until the
     * destructor, that points at the device planes */
    const rt_denoise_guides *guides(const rt_denoise_guides *h, size_t n, bool albedo = true);
    const rt_temporal_guides *guides(const rt_temporal_guides *h, size_t n);
    template <class T> T *out(T *h, size_t bytes) { return static_cast<T *>(add(h, bytes, h != nullptr, false, true)); }
    template <class T> T *inout(T *h, size_t bytes) { return static_cast<T *>(add(h, bytes, h != nullptr, true, true)); } /* continues from the caller's values */
    void *scratch(size_t bytes) { return add(nullptr, bytes, true, false, false); }
    unsigned long long *counter(); /* zeroed */
    bool ok() const { return e_ == hipSuccess; }
    int failed() const { return fail_hip(who_, e_); }
    int finish(unsigned long long *h_count = nullptr);

private:
    struct Buffer {
        void *d, *h; /* h: where finish() downloads to, or null */
        size_t bytes;
    };
    void *add(void *h, size_t bytes, bool wanted, bool upload, bool download);
    const char *who_;
    hipError_t e_ = hipSuccess;
    std::vector<Buffer> buffers_;
    std::deque<rt_denoise_guides> guides_; /* deques: an element stays where it is */
    std::deque<rt_temporal_guides> temporal_guides_;
    unsigned long long *d_count_ = nullptr;
};

/* ---- the device form and the _host form of an image-side query, each written once.  `a` is the query's argument struct
 * (rt_query_args.h); launch(a, stream) puts its kernels on the stream and returns the launch's status. ---- */

/* the limits under the entry point's name, then "nothing to do"; *done: nothing to launch */
template <class Args>
static inline int query_checked(const char *who, const Args &a, rt::QueryForm form, bool *done) {
    int status = RT_ERR_INVALID_ARGUMENT;
    const char *bad = a.limits(form, &status);
    *done = bad || a.empty();
    return bad ? fail(status, std::string(who) + ": " + bad) : RT_OK;
}

template <class Args, class Launch>
static inline int device_query(const char *who, const Args &a, Launch launch, void *hip_stream) {
    bool done;
    const int rc = query_checked(who, a, rt::QUERY_DEVICE, &done);
    if (done) return rc;
    return launched(who, launch(a, static_cast<hipStream_t>(hip_stream)));
}

/* the round trip: a.arrays() swaps every host pointer of the copy for its device array */
template <class Args, class Launch>
static inline int host_query(const char *who, Args a, Launch launch) {
    bool done;
    const int rc = query_checked(who, a, rt::QUERY_HOST_COPY, &done);
    if (done) return rc;
    HostRoundTrip t(who);
    a.arrays(t);
    if (!t.ok()) return t.failed();
    const hipError_t e = launch(a, nullptr);
    if (e != hipSuccess) return launched(who, e);
    return t.finish();
}

RT_API_HIDDEN bool frame_ok(const rt_frame *f);
RT_API_HIDDEN bool frame_fits(const rt_frame *f);
RT_API_HIDDEN int make_kernel_frame(const rt_camera *camera, const rt_frame *frame, rt::KernelFrame *kf);

/* the profiling events live on the device that was current when they were made: calls that hop between devices (rt_multi_*) are
 * not profiled (the thread-local switch is theirs) */
RT_API_HIDDEN bool &profiling_off_flag(); /* of the calling thread */
struct ProfilingOff {
    bool prev;
    ProfilingOff() : prev(profiling_off_flag()) { profiling_off_flag() = true; }
    ~ProfilingOff() { profiling_off_flag() = prev; }
};

/* rt_profile_enable also times the depth-of-field pass's kernels (rt_api_dist.hip): is it on for this thread's calls, and the hooks
 * rt_profile_enable / rt_profile_read_distributed are made of */
RT_API_HIDDEN bool profiling_on();
RT_API_HIDDEN void dist_profile_reset();

/* Everything rt_scene_create derives from the ABI arrays, on the host (no HIP call in there): the device records of
 * rt_device_scene.h.  Also behind rt_scene_describe_nodes, which lets a test look at the node array without a GPU. */
struct SceneLayout {
    std::vector<rt::DevTri> tris;
    std::vector<rt::DevTriAttr> attrs;
    std::vector<rt::DevSegment> segments;
    std::vector<rt::DevTriHead> heads;
    std::vector<rt::DevSphere> spheres;
    double scene_extent = 0.0;
};
RT_API_HIDDEN int layout_scene(const rt_scene_desc *desc, SceneLayout &layout);
/* KernelScene::filter_origin2 of a scene of that extent: origins up to 4 x extent from the centre of coordinates use the rejections */
inline float filter_origin2_of(double scene_extent) { return (float)(16.0 * scene_extent * scene_extent); }

/* The hit queries' kernels (rt_hit_query.hip): get_shade / get_refract / get_reflect on n ABI records, in bands of at most
 * band_records per launch (a multiple of 64, RT_HITQ_BAND at most).  wave_uniform: the casts go through cast_asm instead of cast_pairs
 * (same bits). */
#define RT_HITQ_BAND (1u << 26)
namespace rt {
hipError_t launch_shade_hits(const KernelScene &sc, const rt_hit *hits, const rt_ray *incoming, uint32_t n, float *rgb,
                             unsigned long long *ray_count, bool wave_uniform, uint32_t band_records, hipStream_t stream);
hipError_t launch_refract_rays(const KernelScene &sc, const rt_hit *hits, const rt_ray *incoming, uint32_t n, float max_distance, uint32_t *kind,
                               float *travel, rt_ray *escape, unsigned long long *ray_count, bool wave_uniform, uint32_t band_records, hipStream_t stream);
hipError_t launch_reflect_rays(const rt_hit *hits, const rt_ray *incoming, uint32_t n, rt_ray *out, uint32_t band_records, hipStream_t stream);
/* The scatter queries' kernels (rt_scatter_query.hip), banded the same way.  states: the n_generators device records of an rt_rng;
 * record i draws from generator rng_index[i], or i when rng_index is null; a generator index >= n_generators is "no hit". */
hipError_t launch_scatter_hits(const KernelScene &sc, const rt_hit *hits, const rt_ray *incoming, uint32_t n, uint32_t *states, uint32_t n_generators,
                               const uint32_t *rng_index, uint32_t *type, rt_ray *scattered, float *cosine, uint32_t band_records, hipStream_t stream);
hipError_t launch_scatter_factors(const KernelScene &sc, const rt_hit *hits, const rt_ray *incoming, const uint32_t *types, const rt_ray *next,
                                  const float *travel, uint32_t n, float *rgb, uint32_t band_records, hipStream_t stream);
/* The level loop's kernels (rt_level_query.hip): the stable selection (totals: RT_SELECT_MAX_GROUPS words of scratch) and the
 * element-wise glue, fold and filter of one level; none is banded, the record number is counted in 64 bits. */
hipError_t launch_select_records(const unsigned char *flags, uint32_t n, uint32_t *index, uint32_t *count, uint32_t *totals, hipStream_t stream);
hipError_t launch_level_split(const rt_hit *hits, const uint32_t *type, const float *cosine, uint32_t n, rt_hit *hits_reflect, rt_hit *hits_refract,
                              hipStream_t stream);
hipError_t launch_level_join(const uint32_t *type, const float *cosine, const rt_ray *reflected, const uint32_t *refr_kind, const rt_ray *escape,
                             uint32_t n, rt_ray *next, rt_hit *next_hits, unsigned char *flags, hipStream_t stream);
hipError_t launch_level_close(const rt_hit *hits, const uint32_t *type, const float *cosine, const rt_hit *next_hits, uint32_t n, rt_hit *hits_missed,
                              hipStream_t stream);
hipError_t launch_level_fold(const uint32_t *type, const float *cosine, const rt_hit *next_hits, const float *factor, const float *shade_next,
                             const float *shade_missed, uint32_t n, float *value, hipStream_t stream);
hipError_t launch_level_finish(const float *value, uint32_t n, float *accum, unsigned char *valid, hipStream_t stream);
/* The film queries' kernels (rt_film_query.hip); FilmTile, FilmSplat and UniformLayout are rt_film.h's, shared with the host.  The splat's
 * two forms and their launcher are rt_film_splat_kernel.h's, instantiated there for rt_film_splat and in rt_adaptive_query.hip for
 * rt_film_splat_listed.  tiled: the LDS form of the splat instead of the simple one (same bits). */
hipError_t launch_film_offsets(const FilmTile &t, uint32_t spp, uint32_t pattern, uint32_t seed, float *offsets, hipStream_t stream);
hipError_t launch_camera_rays_offset(const KernelFrame &fr, const float *offsets, uint32_t spp, rt_ray *rays, hipStream_t stream);
hipError_t launch_film_splat(const FilmSplat<UniformLayout> &p, bool tiled, hipStream_t stream);
} /* namespace rt */

/* rt_select_records (rt_api_query.hip) keeps its block totals per (device, stream); rt_post_release (rt_api_post.hip) frees those of a
 * device, which it has synchronised */
RT_API_HIDDEN void select_release(int device);

/* What rt_scatter_hits (rt_api_query.hip) needs of an rt_rng (rt_api_dist.hip): how many generators it holds; and, for a call about to
 * be put on `stream`, its device records — after the look-ahead pass when `prepare` is set and the generators are not known to have
 * their next block already.  Either way the generators may move on to that block in the call, so the object's look-ahead bookkeeping
 * is reset: the next call on it looks for itself. */
RT_API_HIDDEN size_t rng_generator_count(const rt_rng *rng);
RT_API_HIDDEN hipError_t rng_begin_draws(rt_rng *rng, bool prepare, hipStream_t stream, uint32_t **d_states);

#endif /* RT_API_INTERNAL_H */
