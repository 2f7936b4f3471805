/*
 * rt_api.hip — implementation of the C ABI in include/rt_amd.h.
 *
 * Host-side plumbing only: argument validation, the one-time scene upload
 * (with the per-primitive precompute described in rt_device_scene.h), the
 * per-frame camera basis (Camera::shoot's ray-independent part, main.rs:85-92)
 * and stream-ordered kernel launches.  There is NO CPU rendering fallback: if
 * the HIP runtime or a device is missing every render entry point fails with
 * RT_ERR_NO_DEVICE / RT_ERR_HIP.
 */
#include "rt_api_internal.h"
#include "rt_temporal.h"
#include "rt_pwf_common.h" /* pa_ready_packed, the rule launch_pwf and pwf_kernel share: rt_diag_pwf_plan reports it */

/* Process-wide settings (rt_set_*): read by render calls on any thread, so they are atomics.  A value < 0 means "not set
 * yet": the first reader resolves it from the environment (two threads doing that at once compute the same value). */
static std::atomic<int> g_wf_nodes_per_pixel{-1};
static std::atomic<const uint32_t *> g_diag_tile_order{nullptr};
extern "C" void rt_diag_set_tile_order(const void *device_ptr) { g_diag_tile_order.store(static_cast<const uint32_t *>(device_ptr)); }
static std::atomic<uint32_t *> g_diag_tile_cost{nullptr};
extern "C" void rt_diag_set_tile_cost(void *device_ptr) { g_diag_tile_cost.store(static_cast<uint32_t *>(device_ptr)); }
#ifdef RT_DIAG_TIMELINE
static unsigned long long *g_diag_timeline = nullptr;
extern "C" void rt_diag_set_timeline(void *device_ptr) { g_diag_timeline = static_cast<unsigned long long *>(device_ptr); }
#endif

#ifndef RT_BFS_WALK_TRIANGLES_DEFAULT
#define RT_BFS_WALK_TRIANGLES_DEFAULT 8192 /* measured (profiles/r04_scene_sweep_*_bfs.jsonl against *_wave_uniform.jsonl): the breadth-first walk is 1.3-1.7x
                                              * ahead at 9 244 triangles, 2.1-2.3x at 36 892, 8-17x at 147 484; at 2 332 it loses (1.2x on flat meshes, 2x
                                              * on spherized ones) */
#endif
/* the switches of rt_kernels.h RT_OPTIONS: name (also the environment variable that seeds it), whether it has a value, the value */
#define RT_OPTION_NAME(id, name) name,
static const char *const OPT_NAMES[rt::OPT_COUNT] = {RT_OPTIONS(RT_OPTION_NAME)};
#undef RT_OPTION_NAME
static std::atomic<int> g_opt_set[rt::OPT_COUNT];
static std::atomic<long long> g_opt_val[rt::OPT_COUNT];
static std::once_flag g_opt_once;
static void options_from_environment() {
    std::call_once(g_opt_once, [] {
        for (int i = 0; i < rt::OPT_COUNT; ++i) {
            const char *v = getenv(OPT_NAMES[i]);
            if (v && *v) {
                g_opt_val[i].store(strtoll(v, nullptr, 10));
                g_opt_set[i].store(1);
            }
        }
    });
}
namespace rt {
long long option(Option id, long long unset) {
    options_from_environment();
    return g_opt_set[id].load(std::memory_order_acquire) ? g_opt_val[id].load(std::memory_order_relaxed) : unset;
}
} /* namespace rt */

static thread_local std::string g_error;
static thread_local bool t_prof_off = false; /* rt_api_internal.h ProfilingOff */
std::string &last_error() { return g_error; }
bool &profiling_off_flag() { return t_prof_off; }
static std::atomic<int> g_variant{-1};

int fail(int code, const std::string &msg) {
    g_error = msg;
    return code;
}
int fail_hip(const char *what, hipError_t e) {
    g_error = std::string(what) + ": " + hipGetErrorString(e);
    return (e == hipErrorNoDevice || e == hipErrorInvalidDevice) ? RT_ERR_NO_DEVICE
           : (e == hipErrorOutOfMemory)                           ? RT_ERR_OUT_OF_MEMORY
                                                                  : RT_ERR_HIP;
}

int check_count(const char *who, uint64_t n, const CountLimit &limit) {
    if (n < (1ull << limit.log2)) return RT_OK;
    std::string msg = std::string(who) + ": 2^" + std::to_string(limit.log2) + " " + limit.noun + " or more (checked first";
    if (limit.advice) msg = msg + "; " + limit.advice;
    return fail(RT_ERR_UNSUPPORTED, msg + ")");
}
int check_scene(const char *who, const void *scene) {
    if (scene) return RT_OK;
    return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": null scene");
}
int check_pointers(const char *who, bool ok, const char *names) {
    if (ok) return RT_OK;
    return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": null " + names + " pointer");
}
int query_args(const char *who, size_t n, const CountLimit &limit, bool needs_scene, const void *scene, bool pointers_ok, const char *names,
               bool *done) {
    *done = true;
    int rc = check_count(who, n, limit);
    if (rc == RT_OK && needs_scene) rc = check_scene(who, scene);
    if (rc != RT_OK || n == 0) return rc;
    rc = check_pointers(who, pointers_ok, names);
    *done = rc != RT_OK;
    return rc;
}
int hit_sample_args(const char *who, const rt_scene *scene, const HitSampleArgs &a, bool *done) {
    *done = true;
    const uint64_t pairs = (uint64_t)a.n * (uint64_t)a.per_record; /* below 2^64: both factors are below 2^32 where it is used */
    int rc = check_count(who, a.n, RECORDS_2_32);
    if (rc == RT_OK && a.pairs) rc = check_count(who, pairs, *a.pairs);
    if (rc == RT_OK && a.takes_samples)
        rc = check_count(who, pairs * (uint64_t)a.spp, a.of_lights ? SAMPLE_LIGHT_ENTRIES_2_32 : SAMPLE_ENTRIES_2_32);
    if (rc == RT_OK && a.takes_scene) rc = check_scene(who, scene);
    if (rc == RT_OK && a.descriptor) rc = a.descriptor();
    if (rc != RT_OK || pairs == 0) return rc;
    rc = check_pointers(who, a.pointers_ok, a.pointers);
    if (rc != RT_OK) return rc;
    if (a.bad) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + a.bad);
    if (a.light_first >= 0 && (uint64_t)a.light_first + (uint64_t)a.per_record > (uint64_t)scene->ks.n_lights)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": lights " + std::to_string(a.light_first) + " .. " +
                                                 std::to_string((uint64_t)a.light_first + a.per_record) + " of a scene with " + std::to_string(scene->ks.n_lights));
    *done = false;
    return RT_OK;
}

int launched(const char *who, hipError_t e) {
    if (e == hipSuccess) return RT_OK;
    return fail_hip((std::string(who) + ": launch").c_str(), e);
}

bool stream_capturing(hipStream_t stream) {
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &status) != hipSuccess) (void)hipGetLastError();
    return status != hipStreamCaptureStatusNone;
}

HostRoundTrip::~HostRoundTrip() {
    for (const Buffer &b : buffers_) (void)hipFree(b.d);
    if (d_count_) (void)hipFree(d_count_);
}
void *HostRoundTrip::add(void *h, size_t bytes, bool wanted, bool upload, bool download) {
    if (!wanted || e_ != hipSuccess) return nullptr;
    void *d = nullptr;
    e_ = hipMalloc(&d, bytes);
    if (e_ != hipSuccess) return nullptr;
    buffers_.push_back({d, download ? h : nullptr, bytes});
    if (upload) e_ = hipMemcpy(d, h, bytes, hipMemcpyHostToDevice);
    return d;
}
const rt_denoise_guides *HostRoundTrip::guides(const rt_denoise_guides *h, size_t n, bool albedo) {
    rt_denoise_guides g = *h;
    g.normal = plane(h->normal, n, h->normal_stride, 3u);
    g.position = plane(h->position, n, h->position_stride, 3u);
    g.albedo = albedo ? plane(h->albedo, n, h->albedo_stride, 3u) : nullptr;
    g.valid = plane(h->valid, n, h->valid_stride, 1u);
    guides_.push_back(g);
    return &guides_.back();
}
const rt_temporal_guides *HostRoundTrip::guides(const rt_temporal_guides *h, size_t n) {
    rt_temporal_guides g = *h;
    g.normal = plane(h->normal, n, h->normal_stride, 3u);
    g.position = plane(h->position, n, h->position_stride, 3u);
    g.object = plane(h->object, n, h->object_stride, 1u);
    g.valid = plane(h->valid, n, h->valid_stride, 1u);
    temporal_guides_.push_back(g);
    return &temporal_guides_.back();
}
unsigned long long *HostRoundTrip::counter() {
    if (e_ != hipSuccess) return nullptr;
    e_ = hipMalloc(reinterpret_cast<void **>(&d_count_), sizeof *d_count_);
    if (e_ == hipSuccess) e_ = hipMemset(d_count_, 0, sizeof *d_count_);
    return d_count_;
}
int HostRoundTrip::finish(unsigned long long *h_count) {
    if (e_ == hipSuccess) e_ = hipDeviceSynchronize();
    for (const Buffer &b : buffers_)
        if (e_ == hipSuccess && b.h) e_ = hipMemcpy(b.h, b.d, b.bytes, hipMemcpyDeviceToHost);
    unsigned long long count = 0;
    if (e_ == hipSuccess && d_count_) e_ = hipMemcpy(&count, d_count_, sizeof count, hipMemcpyDeviceToHost);
    if (e_ != hipSuccess) return failed();
    if (h_count) *h_count = count;
    return RT_OK;
}

hipError_t DeviceBuffer::reserve(size_t bytes) {
    if (bytes <= bytes_) return hipSuccess;
    (void)release();
    const hipError_t e = kind_ == PINNED_HOST ? hipHostMalloc(&p_, bytes, hipHostMallocDefault) : hipMalloc(&p_, bytes);
    if (e == hipSuccess) bytes_ = bytes;
    else { (void)hipGetLastError(); p_ = nullptr; }
    return e;
}
hipError_t DeviceBuffer::release() {
    const hipError_t e = !p_ ? hipSuccess : kind_ == PINNED_HOST ? hipHostFree(p_) : hipFree(p_);
    p_ = nullptr;
    bytes_ = 0;
    return e;
}

BfsLists bfs_lists(Workspace &ws, uint32_t waves, bool may_allocate) {
    const size_t bytes = (size_t)waves * rt::pwf_bfs_scratch_words_per_wave() * sizeof(uint32_t);
    if (may_allocate) (void)ws.d_bfs.reserve(bytes);
    BfsLists out = {ws.d_bfs.bytes() >= bytes ? ws.d_bfs.get<uint32_t>() : nullptr, RT_BFS_ITEMS_CAP, RT_BFS_JOBS_CAP};
    const long long cap = rt::option(rt::OPT_DIAG_BFS_CAP, 0);
    if (cap > 0) {
        out.items_cap = (uint32_t)std::min<long long>(cap, RT_BFS_ITEMS_CAP);
        out.jobs_cap = (uint32_t)std::min<long long>(cap, RT_BFS_JOBS_CAP);
    }
    return out;
}

/* 2 / 3: the per-pixel kernel with scalar / LDS triangle fetches; 18 / 19: the persistent wavefront kernel (with that as its fallback) */
static bool variant_ok(int v) { return v == 2 || v == 3 || v == 18 || v == 19; }
static int current_variant() {
    int v = g_variant.load(std::memory_order_relaxed);
    if (v < 0) {
        const char *e = getenv("RT_AMD_VARIANT");
        v = (e && *e) ? atoi(e) : RT_VARIANT_DEFAULT;
        if (!variant_ok(v)) v = RT_VARIANT_DEFAULT;
        g_variant.store(v, std::memory_order_relaxed);
    }
    return v;
}
static int current_wf_budget() {
    int v = g_wf_nodes_per_pixel.load(std::memory_order_relaxed);
    if (v < 0) {
        const char *e = getenv("RT_AMD_WF_NODES_PER_PIXEL");
        v = (e && *e) ? atoi(e) : 6; /* the reference scene needs 3.4 at depth 8 */
        if (v < 1 || v > 4096) v = 6;
        g_wf_nodes_per_pixel.store(v, std::memory_order_relaxed);
    }
    return v;
}

bool frame_ok(const rt_frame *f) {
    return f && f->width > 0 && f->height > 0 && f->y_step >= 1 && f->x0 < f->x1 && f->y0 < f->y1 && f->x1 <= f->width &&
           f->y1 <= f->height;
}
/* the kernels and launchers index a tile's pixels with 32-bit arithmetic: a tile of 2^32 pixels or more is refused
 * rather than wrapped (65536 x 65536 would wrap to 0 and "render" nothing) */
bool frame_fits(const rt_frame *f) {
    const uint64_t rows = ((uint64_t)f->y1 - f->y0 + f->y_step - 1) / f->y_step;
    return rows * (uint64_t)(f->x1 - f->x0) < (1ull << 32) - 64u;
}

static std::atomic<bool> g_prof_on{false}; /* rt_profile_enable */
bool profiling_on() { return g_prof_on.load() && !t_prof_off; }

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }

const char *rt_last_error(void) { return g_error.c_str(); }

int rt_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail_hip("hipGetDeviceCount", e);
    return n;
}

int rt_set_device(int device) {
    RT_HIP(hipSetDevice(device));
    return RT_OK;
}

int rt_set_option(const char *name, const char *value) {
    if (!name) return fail(RT_ERR_INVALID_ARGUMENT, "rt_set_option: null name");
    options_from_environment(); /* first, so that a later first use does not overwrite what is set here */
    for (int i = 0; i < rt::OPT_COUNT; ++i) {
        if (strcmp(name, OPT_NAMES[i]) != 0) continue;
        if (value && *value) {
            char *end = nullptr;
            const long long v = strtoll(value, &end, 10);
            if (end == value || *end != '\0') return fail(RT_ERR_INVALID_ARGUMENT, "rt_set_option: the value is not an integer");
            g_opt_val[i].store(v, std::memory_order_relaxed);
            g_opt_set[i].store(1, std::memory_order_release);
        } else {
            g_opt_set[i].store(0, std::memory_order_release);
        }
        return RT_OK;
    }
    return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_set_option: unknown option ") + name);
}

int rt_set_variant(int variant) {
    if (!variant_ok(variant)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_set_variant: 2, 3, 18 or 19 (include/rt_amd.h)");
    g_variant.store(variant);
    return RT_OK;
}
int rt_get_variant(void) { return current_variant(); }

int rt_set_wavefront_budget(unsigned nodes_per_pixel) {
    if (nodes_per_pixel < 1u || nodes_per_pixel > 4096u) return fail(RT_ERR_INVALID_ARGUMENT, "rt_set_wavefront_budget: 1..4096 nodes per pixel");
    g_wf_nodes_per_pixel.store((int)nodes_per_pixel);
    return RT_OK;
}

/* ---- profiling of the dominant kernel ----
 * bench.py's roofline needs the duration of the render kernel alone (a call may also launch the small probe
 * kernel).  When enabled, every rt_render_whitted call records a HIP event pair on the launch stream right
 * around that kernel; rt_profile_read() synchronises and sums the elapsed times.
 * Thread safety: the event list is under a mutex; the pair a call is recording into travels in thread-local state of the
 * calling thread (rt_kernels.hip), so render calls on several host threads do not see each other's events. */
static std::mutex g_prof_mutex;
static std::vector<std::pair<hipEvent_t, hipEvent_t>> g_prof_events;
static size_t g_prof_used = 0;

int rt_profile_enable(int on) {
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    g_prof_on.store(on != 0);
    g_prof_used = 0;
    dist_profile_reset();
    rt::set_main_kernel_events(nullptr, nullptr);
    return RT_OK;
}

int rt_profile_read(double *kernel_ms_sum, unsigned *n_launches) {
    if (!kernel_ms_sum || !n_launches) return fail(RT_ERR_INVALID_ARGUMENT, "rt_profile_read: null argument");
    RT_HIP(hipDeviceSynchronize());
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    double sum = 0.0;
    for (size_t i = 0; i < g_prof_used; ++i) {
        float ms = 0.0f;
        RT_HIP(hipEventElapsedTime(&ms, g_prof_events[i].first, g_prof_events[i].second));
        sum += ms;
    }
    *kernel_ms_sum = sum;
    *n_launches = (unsigned)g_prof_used;
    g_prof_used = 0;
    return RT_OK;
}

uint32_t rt_frame_rows(const rt_frame *f) {
    if (!frame_ok(f)) return 0;
    return (f->y1 - f->y0 + f->y_step - 1) / f->y_step;
}
uint64_t rt_frame_pixels(const rt_frame *f) {
    if (!frame_ok(f)) return 0;
    return (uint64_t)rt_frame_rows(f) * (uint64_t)(f->x1 - f->x0);
}

int rt_scene_create(const rt_scene_desc *desc, rt_scene **out_scene) {
    if (!desc || !out_scene) return fail(RT_ERR_INVALID_ARGUMENT, "rt_scene_create: null argument");
    *out_scene = nullptr;
    SceneLayout layout;
    {
        const int rc = layout_scene(desc, layout);
        if (rc != RT_OK) return rc;
    }
    const std::vector<rt::DevTri> &tris = layout.tris;
    const std::vector<rt::DevTriAttr> &attrs = layout.attrs;
    const std::vector<rt::DevSegment> &segments = layout.segments;
    const std::vector<rt::DevTriHead> &heads = layout.heads;
    const std::vector<rt::DevSphere> &spheres = layout.spheres;
    const double scene_extent = layout.scene_extent;

    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t off_tris = 0;
    const size_t off_attrs = off_tris + up(tris.size() * sizeof(rt::DevTri));
    const size_t off_spheres = off_attrs + up(attrs.size() * sizeof(rt::DevTriAttr));
    const size_t off_mats = off_spheres + up(spheres.size() * sizeof(rt::DevSphere));
    const size_t off_lights = off_mats + up(desc->n_materials * sizeof(rt_material));
    const size_t off_segments = off_lights + up(desc->n_lights * sizeof(rt_light));
    const size_t off_heads = off_segments + up(segments.size() * sizeof(rt::DevSegment));
    const size_t off_light_aux = off_heads + up(heads.size() * sizeof(rt::DevTriHead));
    /* the node tree once more in LEVEL ORDER (rt_kernels.h KernelScene::bfs_nodes): the top-level nodes first, then every inner node's
     * children one after the other — an inner node's record then names its children as a range [first, first + skip_to) of the same
     * array and a breadth-first walk needs no child list beside it.  From the pre-order array: the children of inner node k are
     * k + 1, then each one's skip_to, up to k's own skip_to; the top-level nodes likewise from 0. */
    std::vector<rt::DevSegment> bfs_nodes;
    uint32_t bfs_top = 0u;
    std::vector<uint32_t> order; /* pre-order index of the node at each level-order position */
    {
        order.reserve(segments.size());
        for (uint32_t k = 0; k < (uint32_t)segments.size(); k = segments[k].skip_to) { order.push_back(k); bfs_top += 1u; }
        bfs_nodes.reserve(segments.size());
        for (size_t at = 0; at < order.size(); ++at) {
            const uint32_t k = order[at];
            rt::DevSegment g = segments[k];
            if (g.count == 0u) { /* inner: first = its first child's position, skip_to = how many */
                g.first = (uint32_t)order.size();
                g.skip_to = 0u;
                for (uint32_t j = k + 1u; j < segments[k].skip_to && j < (uint32_t)segments.size(); j = segments[j].skip_to) { order.push_back(j); g.skip_to += 1u; }
            }
            bfs_nodes.push_back(g);
        }
    }
    /* ... and what the walk reads of every node and every triangle as arrays of 16-byte pieces (KernelScene::bfs_soa): the lanes of a
     * pass hold consecutive nodes or triangles, so each of its loads is one contiguous kilobyte */
    std::vector<float> bfs_soa((3u * bfs_nodes.size() + 2u * heads.size()) * 4u, 0.0f);
    for (size_t k = 0; k < bfs_nodes.size(); ++k) {
        memcpy(&bfs_soa[4u * k], &bfs_nodes[k], 16);                                /* first, count, n_normals, r2_hi */
        memcpy(&bfs_soa[4u * (bfs_nodes.size() + k)], &bfs_nodes[k].c[0], 16);       /* centre, child count */
        memcpy(&bfs_soa[4u * (2u * bfs_nodes.size() + k)], &bfs_nodes[k].normals[0][0], 16); /* the first plane direction, or the cone */
    }
    for (size_t t = 0; t < heads.size(); ++t) {
        memcpy(&bfs_soa[4u * (3u * bfs_nodes.size() + t)], &heads[t].n[0], 16);                  /* plane */
        memcpy(&bfs_soa[4u * (3u * bfs_nodes.size() + heads.size() + t)], &heads[t].bc[0], 16);  /* bounding sphere */
    }
    const size_t off_bfs_nodes = off_light_aux + up(desc->n_lights * sizeof(rt::LightAux));
    const size_t off_bfs_soa = off_bfs_nodes + up(bfs_nodes.size() * sizeof(rt::DevSegment));
    const size_t total = off_bfs_soa + up(bfs_soa.size() * sizeof(float)) + 256;
    std::vector<rt::LightAux> light_aux(desc->n_lights);
    for (uint32_t i = 0; i < desc->n_lights; ++i) light_aux[i] = light_aux_of(desc->lights[i]);

    std::vector<unsigned char> blob(total, 0);
    if (!tris.empty()) memcpy(&blob[off_tris], tris.data(), tris.size() * sizeof(rt::DevTri));
    if (!attrs.empty()) memcpy(&blob[off_attrs], attrs.data(), attrs.size() * sizeof(rt::DevTriAttr));
    if (!spheres.empty()) memcpy(&blob[off_spheres], spheres.data(), spheres.size() * sizeof(rt::DevSphere));
    if (desc->n_materials) memcpy(&blob[off_mats], desc->materials, desc->n_materials * sizeof(rt_material));
    if (desc->n_lights) memcpy(&blob[off_lights], desc->lights, desc->n_lights * sizeof(rt_light));
    if (!segments.empty()) memcpy(&blob[off_segments], segments.data(), segments.size() * sizeof(rt::DevSegment));
    if (!heads.empty()) memcpy(&blob[off_heads], heads.data(), heads.size() * sizeof(rt::DevTriHead));
    if (!light_aux.empty()) memcpy(&blob[off_light_aux], light_aux.data(), light_aux.size() * sizeof(rt::LightAux));
    if (!bfs_nodes.empty()) memcpy(&blob[off_bfs_nodes], bfs_nodes.data(), bfs_nodes.size() * sizeof(rt::DevSegment));
    if (!bfs_soa.empty()) memcpy(&blob[off_bfs_soa], bfs_soa.data(), bfs_soa.size() * sizeof(float));

    rt_scene *sc = new (std::nothrow) rt_scene();
    if (!sc) return fail(RT_ERR_OUT_OF_MEMORY, "rt_scene_create: host allocation failed");
    /* for the scene updates (rt_scene_update.hip): the box, and the triangle range of every node that has a bounding sphere — an inner
     * node's reaches to the end of the last leaf below it */
    sc->upd.extent = scene_extent;
    for (size_t at = 0; at < order.size(); ++at) {
        const uint32_t k = order[at];
        const rt::DevSegment &g = segments[k];
        if (g.n_normals == 0u) continue; /* a plain leaf stays plain */
        RefitNode n;
        n.lo = g.first;
        n.hi = g.first + g.count;
        for (uint32_t j = k + 1u; g.count == 0u && j < g.skip_to && j < (uint32_t)segments.size(); ++j) n.hi = std::max(n.hi, segments[j].first + segments[j].count);
        n.seg = k;
        n.bfs_pos = (uint32_t)at;
        if (n.hi > n.lo) sc->upd.nodes.push_back(n);
    }
    sc->d_blob = nullptr;
    hipError_t e = hipGetDevice(&sc->device);
    if (e == hipSuccess) e = hipMalloc(&sc->d_blob, total);
    if (e == hipSuccess) e = hipMemcpy(sc->d_blob, blob.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (sc->d_blob) (void)hipFree(sc->d_blob);
        delete sc;
        return fail_hip("rt_scene_create: device upload", e);
    }
    unsigned char *base = static_cast<unsigned char *>(sc->d_blob);
    sc->ks.tris = reinterpret_cast<const rt::DevTri *>(base + off_tris);
    sc->ks.attrs = reinterpret_cast<const rt::DevTriAttr *>(base + off_attrs);
    sc->ks.spheres = reinterpret_cast<const rt::DevSphere *>(base + off_spheres);
    sc->ks.materials = reinterpret_cast<const rt_material *>(base + off_mats);
    sc->ks.lights = reinterpret_cast<const rt_light *>(base + off_lights);
    sc->ks.n_triangles = desc->n_triangles;
    sc->ks.n_spheres = desc->n_spheres;
    sc->ks.n_materials = desc->n_materials;
    sc->ks.n_lights = desc->n_lights;
    sc->ks.segments = reinterpret_cast<const rt::DevSegment *>(base + off_segments);
    sc->ks.n_segments = (uint32_t)segments.size();
    sc->ks.heads = reinterpret_cast<const rt::DevTriHead *>(base + off_heads);
    sc->ks.light_aux = reinterpret_cast<const rt::LightAux *>(base + off_light_aux);
    sc->ks.filter_origin2 = filter_origin2_of(scene_extent); /* |origin| <= 4 x extent */
    sc->ks.bfs_nodes = reinterpret_cast<const rt::DevSegment *>(base + off_bfs_nodes);
    sc->ks.bfs_soa = reinterpret_cast<const float4 *>(base + off_bfs_soa);
    sc->ks.bfs_top = bfs_top;
    {   /* a scene this large is walked breadth-first by the wavefront kernel (rt_cast_bfs.h cast_bfs): node ids must fit 26 bits */
        const long long at = rt::option(rt::OPT_BFS_WALK_TRIANGLES, RT_BFS_WALK_TRIANGLES_DEFAULT);
        sc->ks.bfs_walk = at > 0 && (long long)desc->n_triangles >= at && segments.size() < (1u << 26) ? 1u : 0u;
    }
    int cus = 0;
    e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, sc->device);
    if (e != hipSuccess || cus <= 0) cus = 256;
    sc->resident_waves = (uint32_t)cus * 4u * (uint32_t)RT_MIN_WAVES;
    sc->pwf_workgroups = (uint32_t)cus * (uint32_t)rt::pwf_workgroups_per_cu(7168u, 8192u, sc->ks.bfs_walk != 0u);
    *out_scene = sc;
    return RT_OK;
}

int rt_scene_destroy(rt_scene *scene) {
    if (!scene) return RT_OK;
    hipError_t e = hipSuccess;
    for (auto &kv : scene->workspaces) {
        if (kv.second.d_counters) (void)hipFree(kv.second.d_counters);
        (void)kv.second.d_pwf.release();
        (void)kv.second.d_bfs.release();
        (void)kv.second.d_split.release();
    }
    (void)scene->upd.d_nodes.release();
    (void)scene->upd.h_stage.release();
    if (scene->upd.stage_event) (void)hipEventDestroy(scene->upd.stage_event);
    (void)scene->kept.d_pieces.release();
    if (scene->d_blob) e = hipFree(scene->d_blob);
    delete scene;
    if (e != hipSuccess) return fail_hip("rt_scene_destroy: hipFree", e);
    return RT_OK;
}

} /* extern "C" */
/* the frame's own part of make_kernel_frame, without the camera: the checks, and the tile with its depth (all that pw_plan reads) */
static int check_render_frame(const rt_frame *frame) {
    if (!frame_ok(frame)) return fail(RT_ERR_INVALID_ARGUMENT, "render: bad frame (need 0 <= x0 < x1 <= width, 0 <= y0 < y1 <= height, y_step >= 1)");
    if (!frame_fits(frame)) return fail(RT_ERR_UNSUPPORTED, "render: tile of 2^32 pixels or more (render it as several tiles)");
    if (frame->max_depth > RT_MAX_DEPTH) return fail(RT_ERR_UNSUPPORTED, "render: max_depth above RT_MAX_DEPTH");
    /* max_depth < 0 is valid and renders as 0: TraceState.depth is an i32 tested with `depth <= 0` (main.rs:488, 669) */
    return RT_OK;
}
static void set_frame_tile(const rt_frame *frame, rt::KernelFrame *kf) {
    kf->cols = frame->x1 - frame->x0;
    kf->rows = rt_frame_rows(frame);
    kf->x0 = frame->x0;
    kf->y0 = frame->y0;
    kf->y_step = frame->y_step;
    kf->max_depth = frame->max_depth;
}
int make_kernel_frame(const rt_camera *camera, const rt_frame *frame, rt::KernelFrame *kf) {
    if (!camera) return fail(RT_ERR_INVALID_ARGUMENT, "render: null camera");
    const int rc = check_render_frame(frame);
    if (rc != RT_OK) return rc;
    using rt::V3;
    /* Camera::shoot, main.rs:85-92: the ray-independent part (rt_temporal.h camera_basis, shared with librt_host.so) */
    const rt::CameraBasis basis = rt::camera_basis(camera);
    const V3 toward = basis.toward, x = basis.x, y = basis.y, origin = basis.origin;
    set_frame_tile(frame, kf);
    kf->half_height = (float)frame->height / 2.0f;
    kf->half_width = (float)frame->width / 2.0f;
    kf->height_f = (float)frame->height;
    kf->cam_origin[0] = origin.x; kf->cam_origin[1] = origin.y; kf->cam_origin[2] = origin.z;
    kf->cam_x[0] = x.x; kf->cam_x[1] = x.y; kf->cam_x[2] = x.z;
    kf->cam_y[0] = y.x; kf->cam_y[1] = y.y; kf->cam_y[2] = y.z;
    kf->cam_toward[0] = toward.x; kf->cam_toward[1] = toward.y; kf->cam_toward[2] = toward.z;
    const V3 origin_focus = rt::v3p(camera->center) + rt::normalize(toward) * camera->near; /* main.rs:118-119 */
    kf->cam_origin_focus[0] = origin_focus.x; kf->cam_origin_focus[1] = origin_focus.y; kf->cam_origin_focus[2] = origin_focus.z;
    return RT_OK;
}

/* A ray batch is rendered in bands of at most this many rays per launch, whichever path it takes: slot indices stay far from what
 * 32 bits hold (pw_slot_to_pixel's cols << 3 wraps at 2^29). */
#define RT_TRACE_BAND_RAYS (1u << 26)

/* What a call on the persistent-wavefront path asks of its workspace, from the frame, the scene and the settings alone (no HIP call,
 * no lock): the grid and the arenas come from these numbers and from nowhere else, and the allocation is checked against `bytes`. */
struct PwPlan {
    uint32_t groups = 0;     /* the grid: one arena per workgroup */
    uint32_t band_units = 0; /* rows (a camera frame) or rays (a batch) per launch */
    uint32_t ring_cap = 0, node_cap = 0, tile_reserve = 0;
    size_t arena_stride = 0, bytes = 0; /* ..., the 512-byte header and the arenas */
};
static PwPlan pw_plan(const rt_scene *scene, const rt::KernelFrame &kf, int wf_budget) {
    const bool rays = rt::frame_is_rays(kf);
    const uint32_t units = rays ? kf.cols : kf.rows;
    PwPlan plan;
    /* The kernel keeps one LDS word per 64 ring slots and per 64 nodes, so an arena holds 64 K ring slots at most.
     * A tile too large for that at the budget asked for (beyond ~8 Mpixel at 6 nodes per pixel) is rendered as
     * several bands of rows, one launch each, through the same workspace. */
    const uint64_t ring_max = 1ull << 16;
    const uint64_t pixels = (uint64_t)kf.cols * kf.rows;
    uint64_t groups = (pixels + 63u) / 64u; /* a workgroup fetches one to eight tiles at a time */
    if (groups > scene->pwf_workgroups) groups = scene->pwf_workgroups;
    {   /* frames in flight on several streams: each launch takes a part of the device, so that they run side by side */
        const long long share = rt::option(rt::OPT_WF_SHARE, 1);
        const uint64_t cap = share > 1 ? ((uint64_t)scene->pwf_workgroups + (uint64_t)share - 1u) / (uint64_t)share : (uint64_t)scene->pwf_workgroups;
        if (groups > cap) groups = cap;
    }
    if (groups < 1) groups = 1;
    uint64_t max_pixels = (ring_max - 1024u) * groups / (uint64_t)wf_budget;
    if (rays && max_pixels > RT_TRACE_BAND_RAYS) max_pixels = RT_TRACE_BAND_RAYS;
    plan.band_units = units;
    if (pixels > max_pixels) {
        const uint64_t n_bands = (pixels + max_pixels - 1) / max_pixels;
        const uint64_t grain = rays ? 64u : 8u; /* whole tiles: 64-ray runs, 8-row tile bands */
        uint64_t len = (units + n_bands - 1) / n_bands;
        len = (len + grain - 1u) & ~(grain - 1u);
        plan.band_units = (uint32_t)(len < units ? len : units);
    }
    const uint64_t band_pixels = rays ? (uint64_t)plan.band_units : (uint64_t)kf.cols * plan.band_units;
    const uint64_t want = (band_pixels * (uint64_t)wf_budget + groups - 1) / groups; /* nodes per arena */
    /* tiles are handed out dynamically, so a workgroup may end up with several times the average: arenas have a
     * floor of 8192 ring slots (1.5 MB) however small the frame (budgets below 4 waive it: tests of the fallback) */
    uint64_t ring = wf_budget >= 4 ? 8192 : 2048;
    while (ring < want + 1024u && ring < ring_max) ring <<= 1;
    plan.ring_cap = (uint32_t)ring;
    /* (the budget sizes the rings; an arena may use all of its ring's worth of nodes: tiles are handed out
     * dynamically, and a workgroup that met expensive ones needs more than the average) */
    plan.node_cap = (uint32_t)(ring - 1024u);
    plan.tile_reserve = 10;
    plan.arena_stride = (rt::pwf_arena_bytes(plan.node_cap, plan.ring_cap, (uint32_t)(kf.max_depth > 0 ? kf.max_depth : 0)) + 255u) & ~(size_t)255u;
    plan.groups = (uint32_t)groups;
    plan.bytes = 512 + (size_t)groups * plan.arena_stride;
    return plan;
}

/* The variant a call on this scene takes: the setting, without the persistent-wavefront path where the scene does not fit its items */
static int scene_variant(const rt_scene *scene) {
    int variant = current_variant();
    /* the persistent-wavefront path packs the ray's face mode and the depth left next to a 21-bit primitive id */
    if ((variant & RT_VARIANT_PWF) && (uint64_t)scene->ks.n_triangles + scene->ks.n_spheres >= (1ull << 21)) variant &= ~RT_VARIANT_PWF;
    if ((variant & RT_VARIANT_PWF) && (scene->ks.n_lights >= (1u << 14) || scene->ks.n_materials >= (1u << 16))) variant &= ~RT_VARIANT_PWF; /* a SHADE item's word: 16 + 14 bits */
    return variant;
}
/* The breadth-first walk's lists for the plan's grid, one set per wave (PA_WAVES = 8 per workgroup): `lists` is null for a scene that
 * is not walked breadth-first, and where the workspace holds too little (and may not grow).  launch_pwf picks pwf_kernel's BFS
 * instantiations when it is handed lists.  Under the scene's ws_mutex. */
static BfsLists pw_bfs_lists(const rt_scene *scene, Workspace &ws, const PwPlan &plan, bool may_allocate) {
    if (scene->ks.bfs_walk == 0u) return BfsLists{nullptr, 0u, 0u};
    return bfs_lists(ws, plan.groups * 8u, may_allocate);
}

/* Which block of global words the call's launch(es) take and whether they prepare it themselves: the state a workspace carries from
 * call to call (rt_api_internal.h Workspace), moved on by this call.  Under the scene's ws_mutex, the arenas held. */
struct PwTurn {
    uint32_t parity = 0;
    bool init = true; /* several bands, or a stream that was captured: every launch prepares its own block */
};
static PwTurn pw_take_turn(Workspace &ws, const PwPlan &plan, const rt::KernelFrame &kf, bool capturing) {
    PwTurn turn;
    if (capturing) ws.pw_always_prepare = true;
    const uint32_t units = rt::frame_is_rays(kf) ? kf.cols : kf.rows;
    if (plan.band_units >= units && !ws.pw_always_prepare) { /* one launch: does it find its block zeroed and its frame description in place? */
        rt::KernelFrame want_frame = kf;
        want_frame.n_chunks = (kf.cols * kf.rows + 63u) / 64u; /* as launch_pwf fills it in */
        turn.init = !ws.pw_ready || memcmp(&ws.pw_frame, &want_frame, sizeof want_frame) != 0;
        turn.parity = ws.pw_parity;
        ws.pw_parity ^= 1u;
        ws.pw_frame = want_frame;
        ws.pw_ready = true;
    } else ws.pw_ready = false; /* several bands, each with its own frame description */
    return turn;
}

/* a stride near the golden section of the tile count scatters consecutive tile fetches over the image */
static uint32_t golden_tile_stride(uint64_t tiles) {
    auto gcd = [](uint64_t a, uint64_t b) { while (b) { const uint64_t t = a % b; a = b; b = t; } return a; };
    uint64_t stride = (uint64_t)((double)tiles * 0.6180339887498949);
    if (stride < 1) stride = 1;
    while (gcd(stride, tiles) != 1) stride += 1;
    return (uint32_t)stride;
}

/* The Whitted render behind rt_render_whitted and rt_trace_rays: kf is a camera frame (make_kernel_frame) or a ray batch (one row of
 * rays whose first record is d_rays; rt_kernels.h frame_set_rays).  The per-(scene, stream) arenas, the bands, the profiling events
 * and the launches; `who` names the entry point in error messages. */
static int render_whitted_frame(const rt_scene *scene, const rt::KernelFrame &kf, const rt_ray *d_rays, float *d_rgb,
                                unsigned long long *d_ray_count, hipStream_t stream, const char *who) {
    const bool rays = rt::frame_is_rays(kf);
    /* Bands: runs of whole 8-row tile bands of a camera frame, runs of whole 64-ray tiles of a ray batch (its one row).  Band k of
     * band_units: its frame description and where its output starts. */
    const uint32_t units = rays ? kf.cols : kf.rows;
    /* The band loops below count in 64 bits: a batch may hold up to 2^32 - 1 rays, and the start of the band after the last one
     * (a multiple of the band length, up to units + band length - 1) need not fit 32 bits.  Each band itself is at most
     * RT_TRACE_BAND_RAYS rays (a batch) or a frame of fewer than 2^32 pixels (frame_fits), so everything inside a launch is 32-bit. */
    auto band_of = [&](uint64_t first, uint32_t band_units, rt::KernelFrame *band, float **band_rgb) {
        const uint32_t u0 = (uint32_t)first; /* < units */
        *band = kf;
        const uint32_t len = units - u0 < band_units ? units - u0 : band_units;
        if (rays) {
            band->cols = len;
            rt::frame_set_rays(band, d_rays + u0, rt::frame_root_contribution(kf));
            *band_rgb = d_rgb + (size_t)u0 * 3u;
        } else {
            band->y0 = kf.y0 + u0 * kf.y_step;
            band->rows = len;
            *band_rgb = d_rgb + (size_t)u0 * kf.cols * 3u;
        }
    };
    int variant = scene_variant(scene);
    const PwPlan plan = (variant & RT_VARIANT_PWF) ? pw_plan(scene, kf, current_wf_budget()) : PwPlan();
    rt::PwParams pw;
    memset(&pw, 0, sizeof pw);
    PwTurn turn;
    rt::KernelQueues qs;
    memset(&qs, 0, sizeof qs);
    {
        rt_scene *mut = const_cast<rt_scene *>(scene); /* workspaces are the only mutable part of a scene */
        std::lock_guard<std::mutex> lock(mut->ws_mutex);
        Workspace &ws = mut->workspaces[stream];
        RT_HIP(ensure_counters(ws));
        ws.pw_last_block = -1;
        if (variant & RT_VARIANT_PWF) {
            if (plan.bytes > ws.d_pwf.bytes()) {
                ws.drop_arenas();
                /* OPT_DIAG_WS_REFUSE: test hook, pretend the allocation fails */
                if (rt::option(rt::OPT_DIAG_WS_REFUSE, 0) <= 0) (void)ws.d_pwf.reserve(plan.bytes);
            }
            /* the grid (groups) and the arenas (groups x arena_stride) come from the one plan; should it ever disagree with the
             * allocation the launch must not happen (round 1's memory fault was a kernel writing one page past a workspace) */
            if (ws.d_pwf.bytes() != 0 && plan.bytes > ws.d_pwf.bytes()) ws.drop_arenas();
            if (ws.d_pwf.bytes() != 0 && scene->ks.bfs_walk != 0u) { /* the breadth-first walk's item and job lists: per wave of the grid */
                const BfsLists bl = pw_bfs_lists(scene, ws, plan, true);
                if (bl.lists == nullptr) ws.drop_arenas(); /* no room: the per-pixel kernel */
                pw.bfs_scratch = bl.lists;
                pw.bfs_items_cap = bl.items_cap; pw.bfs_jobs_cap = bl.jobs_cap;
            }
            if (ws.d_pwf.bytes() == 0) variant = RT_VARIANT_SGPR | RT_VARIANT_STATIC; /* no room for the arenas: the per-pixel kernel renders the frame */
            pw.ring_cap = plan.ring_cap;
            pw.node_cap = plan.node_cap;
            pw.tile_reserve = plan.tile_reserve;
            pw.arena_stride = plan.arena_stride;
            pw.tile_order = g_diag_tile_order.load();
            pw.tile_cost = g_diag_tile_cost.load();
            static_assert(PW_G_BLOCK_WORDS * sizeof(uint32_t) == 128, "two blocks of global words and the frame description share the 512-byte header");
            static_assert(sizeof(rt::KernelFrame) <= 128, "the frame description must fit its slot of the workspace header");
            pw.frame = reinterpret_cast<const rt::KernelFrame *>(ws.d_pwf.get<unsigned char>() + 256);
            pw.arena = ws.d_pwf.get<unsigned char>() + 512;
            pw.ray_count = d_ray_count;
            if (ws.d_pwf.bytes() != 0) {
                turn = pw_take_turn(ws, plan, kf, stream_capturing(stream));
                ws.pw_last_block = (int)turn.parity;
            }
        }
#ifdef RT_DIAG_TIMELINE
        qs.timeline = g_diag_timeline;
#endif
    }
    if (g_prof_on.load() && !t_prof_off) {
        std::lock_guard<std::mutex> lock(g_prof_mutex);
        if (g_prof_used == g_prof_events.size()) {
            hipEvent_t a = nullptr, b = nullptr;
            RT_HIP(hipEventCreate(&a));
            RT_HIP(hipEventCreate(&b));
            g_prof_events.emplace_back(a, b);
        }
        rt::set_main_kernel_events(g_prof_events[g_prof_used].first, g_prof_events[g_prof_used].second);
        g_prof_used += 1;
    } else {
        rt::set_main_kernel_events(nullptr, nullptr);
    }
    hipError_t e = hipSuccess;
    if (variant & RT_VARIANT_PWF) {
        /* a band that does not fit the arenas is rendered by the per-pixel kernel instead (a no-op otherwise) */
        uint32_t *const blocks = reinterpret_cast<uint32_t *>(const_cast<unsigned char *>(pw.arena) - 512);
        pw.global = blocks + turn.parity * PW_G_BLOCK_WORDS;
        pw.global_next = blocks + (turn.parity ^ 1u) * PW_G_BLOCK_WORDS;
        qs.run_if = pw.global + PW_G_OVERFLOW;
        for (uint64_t u0 = 0; e == hipSuccess && u0 < units; u0 += plan.band_units) {
            rt::KernelFrame band;
            float *band_rgb;
            band_of(u0, plan.band_units, &band, &band_rgb);
            pw.tile_stride = golden_tile_stride(((uint64_t)band.cols * band.rows + 63u) / 64u);
            const bool first = u0 == 0, last = u0 + plan.band_units >= units;
            e = rt::launch_pwf(scene->ks, band, band_rgb, pw, plan.groups, stream, turn.init, first, last);
            if (e == hipSuccess) {
                rt::mute_main_kernel_events(true); /* the event pair brackets the persistent kernel(s), not the fallback */
                e = rt::launch_whitted(scene->ks, band, band_rgb, d_ray_count, qs, stream, (variant & RT_VARIANT_LDS) | RT_VARIANT_STATIC);
                rt::mute_main_kernel_events(false);
            }
        }
        if (e != hipSuccess) {
            rt_scene *mut = const_cast<rt_scene *>(scene);
            std::lock_guard<std::mutex> lock(mut->ws_mutex);
            mut->workspaces[stream].pw_ready = false; /* whatever state the blocks are in: the next launch prepares its own */
        }
        return launched(who, e);
    }
    /* the per-pixel kernel: a camera frame in one launch, a ray batch in bands of RT_TRACE_BAND_RAYS (one event pair around them all) */
    const uint32_t band_units = rays && units > RT_TRACE_BAND_RAYS ? RT_TRACE_BAND_RAYS : units;
    const bool several = band_units < units;
    if (several) {
        rt::record_main_kernel_event(0, stream);
        rt::mute_main_kernel_events(true);
    }
    for (uint64_t u0 = 0; e == hipSuccess && u0 < units; u0 += band_units) {
        rt::KernelFrame band;
        float *band_rgb;
        band_of(u0, band_units, &band, &band_rgb);
        e = rt::launch_whitted(scene->ks, band, band_rgb, d_ray_count, qs, stream, variant);
    }
    if (several) {
        rt::mute_main_kernel_events(false);
        if (e == hipSuccess) rt::record_main_kernel_event(1, stream);
    }
    return launched(who, e);
}

extern "C" {
int rt_render_whitted(const rt_scene *scene, const rt_camera *camera, const rt_frame *frame, float *d_rgb,
                      unsigned long long *d_ray_count, void *hip_stream) {
    if (!scene || !d_rgb) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_whitted: null argument");
    rt::KernelFrame kf;
    int rc = make_kernel_frame(camera, frame, &kf);
    if (rc != RT_OK) return rc;
    return render_whitted_frame(scene, kf, nullptr, d_rgb, d_ray_count, static_cast<hipStream_t>(hip_stream), "rt_render_whitted");
}

static const CountLimit TRACE_RAYS_LIMIT = {32u, "rays", "trace them in several calls"};

/* a ray batch as a frame: one row of n_rays roots (rt_kernels.h frame_set_rays) */
static rt::KernelFrame rays_kernel_frame(const rt_ray *d_rays, size_t n_rays, int32_t max_depth, float contribution) {
    rt::KernelFrame kf;
    memset(&kf, 0, sizeof kf);
    kf.cols = (uint32_t)n_rays;
    kf.rows = 1u;
    kf.max_depth = max_depth;
    rt::frame_set_rays(&kf, d_rays, contribution);
    return kf;
}

int rt_trace_rays(const rt_scene *scene, const rt_ray *d_rays, size_t n_rays, int32_t max_depth, float contribution, float *d_rgb,
                  unsigned long long *d_ray_count, void *hip_stream) {
    bool done;
    const int rc = query_args("rt_trace_rays", n_rays, TRACE_RAYS_LIMIT, true, scene, d_rays && d_rgb, "ray or rgb", &done);
    if (rc != RT_OK || done) return rc;
    if (max_depth > RT_MAX_DEPTH) return fail(RT_ERR_UNSUPPORTED, "rt_trace_rays: max_depth above RT_MAX_DEPTH");
    /* max_depth < 0 renders as 0, as in rt_render_whitted (TraceState.depth is tested with `depth <= 0`, main.rs:488) */
    const rt::KernelFrame kf = rays_kernel_frame(d_rays, n_rays, max_depth, contribution);
    return render_whitted_frame(scene, kf, d_rays, d_rgb, d_ray_count, static_cast<hipStream_t>(hip_stream), "rt_trace_rays");
}

/* ---- diagnostics (include/rt_amd.h): which instantiation of pwf_kernel a call reaches, and how the last call's frame ended ---- */

/* What render_whitted_frame would make of kf on this scene and stream, the workspace as it stands (nothing is allocated or changed):
 * pw_plan's numbers under the current budget and RT_AMD_WF_SHARE, and the three template arguments launch_pwf derives from them. */
static int diag_pwf_plan(const rt_scene *scene, const rt::KernelFrame &kf, hipStream_t stream, uint32_t *out_words) {
    const PwPlan plan = pw_plan(scene, kf, current_wf_budget());
    bool arenas = false, lists = false;
    {
        rt_scene *mut = const_cast<rt_scene *>(scene);
        std::lock_guard<std::mutex> lock(mut->ws_mutex);
        const auto it = mut->workspaces.find(stream);
        if (it != mut->workspaces.end()) {
            arenas = it->second.d_pwf.bytes() != 0 && plan.bytes <= it->second.d_pwf.bytes();
            lists = pw_bfs_lists(scene, it->second, plan, false).lists != nullptr;
        }
    }
    const bool persistent = (scene_variant(scene) & RT_VARIANT_PWF) != 0 && arenas && (scene->ks.bfs_walk == 0u || lists);
    out_words[RT_DIAG_PWF_PERSISTENT] = persistent ? 1u : 0u;
    out_words[RT_DIAG_PWF_GROUPS] = plan.groups;
    out_words[RT_DIAG_PWF_UNITS] = rt::frame_is_rays(kf) ? kf.cols : kf.rows;
    out_words[RT_DIAG_PWF_BAND_UNITS] = plan.band_units;
    out_words[RT_DIAG_PWF_RING_CAP] = plan.ring_cap;
    out_words[RT_DIAG_PWF_NODE_CAP] = plan.node_cap;
    out_words[RT_DIAG_PWF_PACKED] = rt::pa_ready_packed(plan.node_cap, plan.ring_cap) ? 1u : 0u;
    out_words[RT_DIAG_PWF_BFS] = scene->ks.bfs_walk != 0u && lists ? 1u : 0u; /* launch_pwf: sc.bfs_walk != 0u && pp.bfs_scratch != nullptr */
    out_words[RT_DIAG_PWF_RAYS] = rt::frame_is_rays(kf) ? 1u : 0u;
    out_words[RT_DIAG_PWF_BUDGET] = (uint32_t)current_wf_budget();
    return RT_OK;
}

int rt_diag_pwf_plan(const rt_scene *scene, const rt_frame *frame, void *hip_stream, uint32_t *out_words) {
    if (!scene || !out_words) return fail(RT_ERR_INVALID_ARGUMENT, "rt_diag_pwf_plan: null argument");
    const int rc = check_render_frame(frame);
    if (rc != RT_OK) return rc;
    rt::KernelFrame kf;
    memset(&kf, 0, sizeof kf);
    set_frame_tile(frame, &kf);
    return diag_pwf_plan(scene, kf, static_cast<hipStream_t>(hip_stream), out_words);
}

int rt_diag_pwf_plan_rays(const rt_scene *scene, size_t n_rays, int32_t max_depth, void *hip_stream, uint32_t *out_words) {
    int rc = check_count("rt_diag_pwf_plan_rays", n_rays, TRACE_RAYS_LIMIT);
    if (rc != RT_OK) return rc;
    if (!scene || !out_words) return fail(RT_ERR_INVALID_ARGUMENT, "rt_diag_pwf_plan_rays: null argument");
    if (n_rays == 0) return fail(RT_ERR_INVALID_ARGUMENT, "rt_diag_pwf_plan_rays: an empty batch launches nothing");
    if (max_depth > RT_MAX_DEPTH) return fail(RT_ERR_UNSUPPORTED, "rt_diag_pwf_plan_rays: max_depth above RT_MAX_DEPTH");
    return diag_pwf_plan(scene, rays_kernel_frame(nullptr, n_rays, max_depth, 1.0f), static_cast<hipStream_t>(hip_stream), out_words);
}

int rt_diag_pwf_outcome(const rt_scene *scene, void *hip_stream, uint32_t *out_words) {
    if (!scene || !out_words) return fail(RT_ERR_INVALID_ARGUMENT, "rt_diag_pwf_outcome: null argument");
    const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    for (int i = 0; i < RT_DIAG_PWF_OUTCOME_WORDS; ++i) out_words[i] = 0u;
    rt_scene *mut = const_cast<rt_scene *>(scene);
    std::lock_guard<std::mutex> lock(mut->ws_mutex); /* held over the copy: no call may drop the arenas under it */
    const auto it = mut->workspaces.find(stream);
    if (it == mut->workspaces.end() || it->second.pw_last_block < 0 || it->second.d_pwf.bytes() == 0) return RT_OK; /* no persistent launch to speak of */
    uint32_t block[PW_G_WORDS];
    hipError_t e = hipMemcpyAsync(block, it->second.d_pwf.get<uint32_t>() + (size_t)it->second.pw_last_block * PW_G_BLOCK_WORDS, sizeof block,
                                  hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail_hip("rt_diag_pwf_outcome: copy", e);
    out_words[RT_DIAG_PWF_LAUNCHED] = 1u;
    out_words[RT_DIAG_PWF_OVERFLOW] = block[PW_G_OVERFLOW];
    out_words[RT_DIAG_PWF_TILES_DONE] = block[PW_G_TILES_DONE];
    out_words[RT_DIAG_PWF_GROUPS_DONE] = block[PW_G_GROUPS_DONE];
    out_words[RT_DIAG_PWF_CASTS_LO] = block[PW_G_CASTS];
    out_words[RT_DIAG_PWF_CASTS_HI] = block[PW_G_CASTS + 1u];
    return RT_OK;
}

int rt_trace_rays_host(const rt_scene *scene, const rt_ray *h_rays, size_t n_rays, int32_t max_depth, float contribution, float *h_rgb,
                       unsigned long long *h_ray_count) {
    bool done;
    int rc = query_args("rt_trace_rays_host", n_rays, TRACE_RAYS_LIMIT, true, scene, h_rays && h_rgb, "ray or rgb", &done);
    if (rc == RT_OK && done && h_ray_count) *h_ray_count = 0;
    if (rc != RT_OK || done) return rc;
    if (max_depth > RT_MAX_DEPTH) return fail(RT_ERR_UNSUPPORTED, "rt_trace_rays_host: max_depth above RT_MAX_DEPTH");
    HostRoundTrip t("rt_trace_rays_host");
    const rt_ray *d_rays = t.in(h_rays, n_rays * sizeof(rt_ray));
    float *d_rgb = t.out(h_rgb, n_rays * 3 * sizeof(float));
    unsigned long long *d_cnt = t.counter();
    if (!t.ok()) return t.failed();
    rc = rt_trace_rays(scene, d_rays, n_rays, max_depth, contribution, d_rgb, d_cnt, nullptr);
    return rc != RT_OK ? rc : t.finish(h_ray_count);
}

int rt_render_whitted_host(const rt_scene *scene, const rt_camera *camera, const rt_frame *frame, float *h_rgb,
                           unsigned long long *h_ray_count) {
    if (!scene || !h_rgb) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_whitted_host: null argument");
    if (!frame_ok(frame)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_whitted_host: bad frame");
    HostRoundTrip t("rt_render_whitted_host");
    float *d_rgb = t.out(h_rgb, (size_t)rt_frame_pixels(frame) * 3 * sizeof(float));
    unsigned long long *d_cnt = t.counter();
    if (!t.ok()) return t.failed();
    const int rc = rt_render_whitted(scene, camera, frame, d_rgb, d_cnt, nullptr);
    return rc != RT_OK ? rc : t.finish(h_ray_count);
}

} /* extern "C" */
