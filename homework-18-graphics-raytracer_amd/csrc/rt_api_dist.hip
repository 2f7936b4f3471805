/*
 * rt_api_dist.hip — the depth-of-field pass behind the C ABI (main.rs:1117-1167): the per-pixel generators (rt_rng_*) and
 * rt_render_distributed — how many epochs make a batch, the workspace(s) a call runs through, and which stream each of a batch's
 * kernels (look-ahead, chain, shade, unwind; rt_distributed.hip) is put on.  The same pass on caller-supplied rays
 * (rt_trace_rays_distributed: one body, render_distributed_frame, serves both), generators that belong to no frame
 * (rt_rng_create_seeded, rt_rng_upload) and the lens as a ray source (rt_focus_rays).
 */
#include "rt_api_internal.h"

#ifndef RT_DIST_SPLIT_DEFAULT
#define RT_DIST_SPLIT_DEFAULT 1
#endif
static std::atomic<int> g_dist_split{-1}; /* -1: RT_AMD_DIST_SPLIT or the default */
extern "C" int rt_set_distributed_split(int on) { g_dist_split.store(on < 0 ? -1 : (on > 1 ? 1 : on)); return 0; } /* 2 (round 2's queued chain) is 1 now */

/* ---- timing of the pass's kernels (rt_profile_enable / rt_profile_read_distributed): while profiling is on, every launch is
 * bracketed by an event pair on the stream it is put on — kernels of a pipelined call overlap, so the per-kernel sums add up to
 * more than the call takes; what they give is each kernel's own duration under that overlap (what rocprofv3 --kernel-trace shows) */
enum { DK_PREPARE = 0, DK_CHAIN, DK_SHADE, DK_UNWIND, DK_KINDS };
struct DistProfile {
    std::mutex mutex;
    std::vector<hipEvent_t> events; /* pairs */
    std::vector<int> kind;          /* per pair */
    size_t used = 0;                /* pairs */
};
static DistProfile g_dprof;
void dist_profile_reset() {
    std::lock_guard<std::mutex> lock(g_dprof.mutex);
    g_dprof.used = 0;
}
/* n pairs of consecutive kinds starting at `kind`; false (and no events) when profiling is off or events cannot be made */
static bool dist_profile_pairs(int kind, int n, hipEvent_t *out) {
    if (!profiling_on()) return false;
    std::lock_guard<std::mutex> lock(g_dprof.mutex);
    while (g_dprof.events.size() < 2u * (g_dprof.used + (size_t)n)) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); return false; }
        g_dprof.events.push_back(e);
    }
    g_dprof.kind.resize(g_dprof.events.size() / 2u);
    for (int i = 0; i < n; ++i) {
        out[2 * i] = g_dprof.events[2u * (g_dprof.used + (size_t)i)];
        out[2 * i + 1] = g_dprof.events[2u * (g_dprof.used + (size_t)i) + 1u];
        g_dprof.kind[g_dprof.used + (size_t)i] = kind + i;
    }
    g_dprof.used += (size_t)n;
    return true;
}

extern "C" {

int rt_profile_read_distributed(double ms_sum[4], unsigned n_launches[4]) {
    if (!ms_sum || !n_launches) return fail(RT_ERR_INVALID_ARGUMENT, "rt_profile_read_distributed: null argument");
    RT_HIP(hipDeviceSynchronize());
    std::lock_guard<std::mutex> lock(g_dprof.mutex);
    for (int k = 0; k < DK_KINDS; ++k) { ms_sum[k] = 0.0; n_launches[k] = 0u; }
    for (size_t i = 0; i < g_dprof.used; ++i) {
        float ms = 0.0f;
        RT_HIP(hipEventElapsedTime(&ms, g_dprof.events[2u * i], g_dprof.events[2u * i + 1u]));
        ms_sum[g_dprof.kind[i]] += ms;
        n_launches[g_dprof.kind[i]] += 1u;
    }
    g_dprof.used = 0;
    return RT_OK;
}

/* ---- distributed pass ------------------------------------------------------- */

struct rt_rng {
    int device = -1;
    DeviceBuffer d_states; /* RT_RNG_DEVICE_WORDS per pixel */
    DeviceBuffer d_list;   /* scratch of the look-ahead pass: 1 + pixels words */
    uint32_t compute_units = 256;
    /* The look-ahead for the NEXT batch runs on a stream of its own next to this batch's shade kernel (nothing after
     * the chain kernel touches the records).  ahead = every pixel has its next block, as of the work enqueued so far. */
    hipStream_t aux = nullptr;
    hipEvent_t ev_chain = nullptr, ev_prepared = nullptr;
    bool ahead = false;
    /* The shade and unwind kernels of a batch run on a third stream, beside the NEXT batch's chain kernel (two workspaces, used
     * in turn): they fill what its tail leaves idle.  ev_tail[b]: the unwind that read workspace b has finished. */
    hipStream_t tail = nullptr;
    hipEvent_t ev_tail[2] = {nullptr, nullptr};
    /* the chain kernel's pixels grouped by what their samples cost (rt_kernels.h DistParams::pixel_order): per pixel its cost in the
     * last batch unwound | two orders, one per workspace of a pipelined call | 512 words of scratch */
    DeviceBuffer d_pix;
    bool order_valid[2] = {false, false};
    hipStream_t main_stream = nullptr; /* of the call in progress (for the after-chain hook) */
    uint32_t *la_states = nullptr;     /* ... and the records that call (or band of a ray batch) works on */
    uint32_t la_count = 0;
    /* the tile the generators were seeded for (rt_rng_create); seeded ones (rt_rng_create_seeded) belong to no frame: one row of
     * `cols` records with y_step 0, which no frame has (frame_ok) */
    uint32_t cols = 0, rows = 0, x0 = 0, y0 = 0, y_step = 0;
    uint32_t *states() const { return d_states.get<uint32_t>(); }
    uint32_t *list() const { return d_list.get<uint32_t>(); }
    uint32_t *pix() const { return d_pix.get<uint32_t>(); }
};

static size_t rng_count(const rt_rng *r) { return (size_t)r->cols * r->rows; }

static rt_rng *rng_new(uint32_t cols, uint32_t rows, uint32_t x0, uint32_t y0, uint32_t y_step) {
    rt_rng *r = new (std::nothrow) rt_rng();
    if (!r) return nullptr;
    r->cols = cols; r->rows = rows; r->x0 = x0; r->y0 = y0; r->y_step = y_step;
    return r;
}

/* the records (unseeded), the scratch arrays, the streams and the events */
static hipError_t rng_device_init(rt_rng *r) {
    const size_t n = rng_count(r);
    const size_t bytes = n * RT_RNG_DEVICE_WORDS * sizeof(uint32_t);
    hipError_t e = hipGetDevice(&r->device);
    if (e == hipSuccess) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, r->device) == hipSuccess && cus > 0) r->compute_units = (uint32_t)cus;
    }
    if (e == hipSuccess) e = r->d_states.reserve(bytes);
    if (e == hipSuccess) e = r->d_list.reserve((n + 1u) * sizeof(uint32_t));
    if (e == hipSuccess) e = r->d_pix.reserve((n * 3u + 512u) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(r->pix(), 0, r->d_pix.bytes());
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&r->aux, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->ev_chain, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->ev_prepared, hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&r->tail, hipStreamNonBlocking); /* (at the lowest stream priority: no different, 1 226 against 1 229 Msamples/s) */
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->ev_tail[0], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->ev_tail[1], hipEventDisableTiming);
    return e;
}

/* everything rng_device_init made (or as much of it as there is) and the object; the status of freeing the records */
static hipError_t rng_free(rt_rng *r) {
    const hipError_t e = r->d_states.release();
    (void)r->d_list.release();
    (void)r->d_pix.release();
    if (r->ev_chain) (void)hipEventDestroy(r->ev_chain);
    if (r->ev_prepared) (void)hipEventDestroy(r->ev_prepared);
    if (r->aux) (void)hipStreamDestroy(r->aux);
    for (int b = 0; b < 2; ++b) if (r->ev_tail[b]) (void)hipEventDestroy(r->ev_tail[b]);
    if (r->tail) (void)hipStreamDestroy(r->tail);
    delete r;
    return e;
}

int rt_rng_state_words(void) { return (int)RT_RNG_STATE_WORDS; }

int rt_rng_create(const rt_frame *frame, rt_rng **out_rng) {
    if (!out_rng) return fail(RT_ERR_INVALID_ARGUMENT, "rt_rng_create: null argument");
    *out_rng = nullptr;
    if (!frame_ok(frame)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_rng_create: bad frame");
    if (!frame_fits(frame)) return fail(RT_ERR_UNSUPPORTED, "rt_rng_create: tile of 2^32 pixels or more");
    rt_rng *r = rng_new(frame->x1 - frame->x0, rt_frame_rows(frame), frame->x0, frame->y0, frame->y_step);
    if (!r) return fail(RT_ERR_OUT_OF_MEMORY, "rt_rng_create: host allocation failed");
    hipError_t e = rng_device_init(r);
    if (e == hipSuccess) {
        rt::KernelFrame kf;
        memset(&kf, 0, sizeof kf);
        kf.cols = r->cols; kf.rows = r->rows; kf.x0 = r->x0; kf.y0 = r->y0; kf.y_step = r->y_step;
        e = rt::launch_rng_seed(r->states(), kf, nullptr);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        (void)rng_free(r);
        return fail_hip("rt_rng_create", e);
    }
    *out_rng = r;
    return RT_OK;
}

int rt_rng_create_seeded(const uint64_t *h_seeds, size_t n, rt_rng **out_rng) {
    const int rc = check_count("rt_rng_create_seeded", n, {32u, "generators", nullptr});
    if (rc != RT_OK) return rc;
    if (!out_rng) return fail(RT_ERR_INVALID_ARGUMENT, "rt_rng_create_seeded: null argument");
    *out_rng = nullptr;
    if (n != 0 && !h_seeds) return fail(RT_ERR_INVALID_ARGUMENT, "rt_rng_create_seeded: null seed pointer");
    rt_rng *r = rng_new((uint32_t)n, 1u, 0u, 0u, 0u);
    if (!r) return fail(RT_ERR_OUT_OF_MEMORY, "rt_rng_create_seeded: host allocation failed");
    if (n == 0) { /* a valid empty object: nothing on the device, nothing ever launched for it */
        *out_rng = r;
        return RT_OK;
    }
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the seed kernel reads 64-bit words");
    unsigned long long *d_seeds = nullptr;
    hipError_t e = rng_device_init(r);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_seeds), n * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMemcpy(d_seeds, h_seeds, n * sizeof(uint64_t), hipMemcpyHostToDevice); /* the one upload */
    if (e == hipSuccess) e = rt::launch_rng_seed_from(r->states(), d_seeds, (uint32_t)n, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (d_seeds) (void)hipFree(d_seeds);
    if (e != hipSuccess) {
        (void)rng_free(r);
        return fail_hip("rt_rng_create_seeded", e);
    }
    *out_rng = r;
    return RT_OK;
}

int rt_rng_destroy(rt_rng *rng) {
    if (!rng) return RT_OK;
    if (rng->aux) (void)hipStreamSynchronize(rng->aux); /* a look-ahead pass may still be writing the records */
    if (rng->tail) (void)hipStreamSynchronize(rng->tail);
    const hipError_t e = rng_free(rng);
    if (e != hipSuccess) return fail_hip("rt_rng_destroy: hipFree", e);
    return RT_OK;
}

int rt_rng_download(const rt_rng *rng, uint32_t *h_states) {
    if (!rng || !h_states) return fail(RT_ERR_INVALID_ARGUMENT, "rt_rng_download: null argument");
    /* the device keeps two banks per pixel (the block in use and the next one, generated ahead); what leaves is the
     * reference's record: the bank in use + the position */
    const size_t bytes = (size_t)rng->cols * rng->rows * RT_RNG_STATE_WORDS * sizeof(uint32_t);
    if (bytes == 0) return RT_OK;
    RT_HIP(hipDeviceSynchronize());
    uint32_t *d_tmp = nullptr;
    RT_HIP(hipMalloc(reinterpret_cast<void **>(&d_tmp), bytes));
    hipError_t e = rt::launch_rng_export(rng->states(), rng->cols * rng->rows, d_tmp, nullptr);
    if (e == hipSuccess) e = hipMemcpy(h_states, d_tmp, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d_tmp);
    if (e != hipSuccess) return fail_hip("rt_rng_download", e);
    return RT_OK;
}

int rt_rng_upload(rt_rng *rng, const uint32_t *h_states) {
    if (!rng || !h_states) return fail(RT_ERR_INVALID_ARGUMENT, "rt_rng_upload: null argument");
    const size_t bytes = rng_count(rng) * RT_RNG_STATE_WORDS * sizeof(uint32_t);
    if (bytes == 0) return RT_OK;
    RT_HIP(hipDeviceSynchronize()); /* whatever still reads or writes the records (a look-ahead on the aux stream) has finished */
    uint32_t *d_tmp = nullptr;
    RT_HIP(hipMalloc(reinterpret_cast<void **>(&d_tmp), bytes));
    hipError_t e = hipMemcpy(d_tmp, h_states, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = rt::launch_rng_import(rng->states(), (uint32_t)rng_count(rng), d_tmp, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    (void)hipFree(d_tmp);
    if (e != hipSuccess) return fail_hip("rt_rng_upload", e);
    /* every record now has its block in bank 0 and none prepared: the next call's look-ahead finds that out by itself once it is
     * not told otherwise; and what the pixels cost under the old streams says nothing about the new ones */
    rng->ahead = false;
    rng->order_valid[0] = rng->order_valid[1] = false;
    return RT_OK;
}

/* after the chain kernel of a batch: look-ahead for the next batch on the aux stream */
static hipError_t lookahead_after_chain(void *ctx) {
    rt_rng *rng = static_cast<rt_rng *>(ctx);
    hipError_t e = hipEventRecord(rng->ev_chain, rng->main_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(rng->aux, rng->ev_chain, 0);
    hipEvent_t pe[2];
    const bool prof = dist_profile_pairs(DK_PREPARE, 1, pe);
    if (e == hipSuccess && prof) e = hipEventRecord(pe[0], rng->aux);
    if (e == hipSuccess) e = rt::launch_rng_prepare(rng->la_states, rng->la_count, rng->list(), rng->compute_units, rng->aux);
    if (e == hipSuccess && prof) e = hipEventRecord(pe[1], rng->aux);
    if (e == hipSuccess) e = hipEventRecord(rng->ev_prepared, rng->aux);
    if (e == hipSuccess) rng->ahead = true;
    return e;
}

} /* extern "C" */

size_t rng_generator_count(const rt_rng *rng) { return rng_count(rng); }

hipError_t rng_begin_draws(rt_rng *rng, bool prepare, hipStream_t stream, uint32_t **d_states) {
    *d_states = rng->states();
    hipError_t e = hipSuccess;
    if (prepare && !rng->ahead && rng_count(rng) != 0)
        e = rt::launch_rng_prepare(rng->states(), (uint32_t)rng_count(rng), rng->list(), rng->compute_units, stream);
    rng->ahead = false; /* a generator may move on to its prepared block */
    return e;
}

/* One call of the pass (or one band of a ray batch) as its two organisations see it: what the caller passed and the switches
 * (rt_kernels.h RT_OPTIONS; rt_set_option or, once per process, the environment). */
struct DistCall {
    const rt_scene *scene;
    const rt::KernelFrame &kf;
    rt_rng *rng;
    hipStream_t stream;
    const char *who;
    size_t n_pixels;
    uint32_t n_epochs, dist_waves; /* ..., the persistent grid */
    bool lookahead;  /* RT_AMD_RNG_LOOKAHEAD=0 leaves every IsaacCore::generate to the render kernels */
    /* ... and those of the split pass.  pipeline: two workspaces, used in turn, when the call has more than one batch: batch k's shade and
     * unwind kernels then run on a stream of their own beside batch k+1's chain kernel (A/B: RT_AMD_DIST_PIPELINE=0: one workspace,
     * everything in line).  by_cost: the chain kernel's pixels grouped by cost when a lane gets two of them at most (rt_kernels.h
     * DistParams::pixel_order); A/B: RT_AMD_DIST_BY_COST=0 never, =1 always.  prep_first = 0: shade kernel and look-ahead start together.
     * cap: RT_AMD_DIST_WS_MB, default 32 GiB for the two workspaces of a call of several batches. */
    bool pipeline, by_cost, prep_first;
    size_t cap;
};

/* The four arrays of one split workspace, [slot][sample of a batch]; set(epochs) places them and returns the bytes of ONE workspace */
struct SplitLayout {
    size_t n_pixels;
    uint32_t slots;
    size_t o_hdr = 0, o_req = 0, o_shade = 0, o_frame = 0;
    size_t set(uint32_t epochs) {
        auto carve = [](size_t &off, size_t bytes) { const size_t at = off; off = (off + bytes + 255u) & ~(size_t)255u; return at; };
        const size_t n_samples = n_pixels * epochs;
        size_t off = 0;
        o_hdr = carve(off, n_samples * sizeof(uint32_t));
        o_req = carve(off, n_samples * slots * 4u * sizeof(uint4));
        o_shade = carve(off, n_samples * slots * sizeof(float4));
        o_frame = carve(off, n_samples * (slots - 1u) * sizeof(float4));
        return off;
    }
};

/* How many epochs make a batch and how many workspaces the call uses, settled against what `buf` holds or can be made to hold: as
 * many epochs as fit the cap (one at least) and never more than 16 — a visit of a pixel should not need more random words than the
 * block in use plus the one prepared ahead.  batch == 0: no room for one epoch (buf holds nothing). */
static int split_negotiate(DeviceBuffer &buf, hipStream_t stream, size_t cap, size_t per_epoch, uint32_t n_epochs, bool pipeline, SplitLayout &lay,
                           uint32_t &batch, uint32_t &n_buf) {
    batch = (uint32_t)std::min<size_t>(std::min<size_t>(n_epochs, 16), std::max<size_t>(1, cap / per_epoch));
    if (pipeline && batch < n_epochs) /* more than one batch: each workspace gets half the cap */
        batch = (uint32_t)std::min<size_t>(batch, std::max<size_t>(1, cap / 2u / per_epoch));
    if (batch < n_epochs) batch = (n_epochs + (n_epochs + batch - 1u) / batch - 1u) / ((n_epochs + batch - 1u) / batch); /* as many batches, of equal size */
    n_buf = pipeline && batch < n_epochs ? 2u : 1u;
    size_t need = lay.set(batch) * n_buf;
    if (buf.bytes() != 0 && buf.bytes() < need) {
        /* A workspace that holds at least half the batch wanted is used as it is: giving back and obtaining
         * gigabytes costs far more than the shorter batches do (measured: 0.65 s to replace a 14 GB workspace
         * by a 16 GB one, against 0.15 s for the 64 epochs the call was made for; profiles/README.md) */
        uint32_t fit = batch;
        while (fit > 1u && lay.set(fit) * n_buf > buf.bytes()) fit -= 1u;
        if (lay.set(fit) * n_buf <= buf.bytes() && fit * 2u >= batch) batch = fit;
        need = lay.set(batch) * n_buf;
    }
    if (buf.bytes() < need) {
        if (buf.bytes() != 0) {
            RT_HIP(hipStreamSynchronize(stream));
            const hipError_t e = buf.release();
            if (e != hipSuccess) return fail_hip("hipFree(ws.d_split)", e);
        }
        /* no room for the batch the cap allows: halve it; no room for one epoch: the one-kernel organisation */
        int refuse = (int)rt::option(rt::OPT_DIAG_WS_REFUSE, 0); /* test hook: pretend the first n allocations fail (tests/test_gpu_distributed_parity.py) */
        while (refuse-- > 0 || buf.reserve(need) != hipSuccess) {
            if (batch == 1u && n_buf == 1u) { batch = 0u; break; }
            if (batch == 1u) n_buf = 1u;
            else batch = (batch + 1u) / 2u;
            need = lay.set(batch) * n_buf;
        }
    }
    return RT_OK;
}

/* The split pass: chain / shade / unwind kernels over batches of epochs (rt_distributed.hip "the split pass"), the two workspaces in
 * turn, the look-ahead on the aux stream, the profiling events.  *no_room: nothing was launched, the one-kernel pass renders the call. */
static int dist_split_pass(const DistCall &c, rt::DistParams dp, bool *no_room) {
    rt_rng *const rng = c.rng;
    hipStream_t stream = c.stream;
    const size_t n_pixels = c.n_pixels;
    const uint32_t n_epochs = c.n_epochs;
    SplitLayout lay = {n_pixels, (uint32_t)(c.kf.max_depth > 0 ? c.kf.max_depth : 0) + 1u};
    const size_t per_epoch = rt::distributed_split_bytes_per_sample(c.kf.max_depth) * n_pixels + 4096;
    uint32_t batch = 0, n_buf = 0;
    char *base = nullptr;
    {
        rt_scene *mut = const_cast<rt_scene *>(c.scene);
        std::lock_guard<std::mutex> lock(mut->ws_mutex);
        Workspace &ws = mut->workspaces[stream];
        RT_HIP(ensure_counters(ws));
        const int rc = split_negotiate(ws.d_split, stream, c.cap, per_epoch, n_epochs, c.pipeline, lay, batch, n_buf);
        if (rc != RT_OK) return rc;
        dp.work_queue = ws.d_counters;
        base = ws.d_split.get<char>();
    }
    *no_room = batch == 0u;
    if (*no_room) return RT_OK;
    const size_t buf_stride = lay.set(batch); /* places the arrays for the batch size settled on */
    if (batch >= n_epochs) n_buf = 1u;
    dp.sp_slots = lay.slots;
    uint32_t k = 0;
    bool tail_used[2] = {false, false};
    hipError_t e = hipSuccess;
    for (uint32_t e0 = 0; e0 < n_epochs && e == hipSuccess; e0 += batch, ++k) {
        /* the layout is [slot][sample of THIS batch]: a short last batch just uses a prefix of every array */
        const uint32_t b = n_buf == 2u ? (k & 1u) : 0u;
        char *const ws_base = base + (size_t)b * buf_stride;
        dp.sp_hdr = reinterpret_cast<uint32_t *>(ws_base + lay.o_hdr);
        dp.sp_req = reinterpret_cast<uint4 *>(ws_base + lay.o_req);
        dp.sp_shade = reinterpret_cast<float4 *>(ws_base + lay.o_shade);
        dp.sp_frame = reinterpret_cast<float4 *>(ws_base + lay.o_frame);
        dp.epoch0 = e0;
        dp.n_epochs = std::min(batch, n_epochs - e0);
        e = hipMemsetAsync(dp.work_queue, 0, sizeof(uint32_t), stream);
        if (e == hipSuccess && tail_used[b]) e = hipStreamWaitEvent(stream, rng->ev_tail[b], 0); /* the unwind two batches ago has read this workspace */
        hipEvent_t pe[8]; /* profiling: prepare | chain | shade, unwind */
        if (e == hipSuccess && c.lookahead && !rng->ahead) {
            const bool prof = dist_profile_pairs(DK_PREPARE, 1, pe);
            if (prof) e = hipEventRecord(pe[0], stream);
            if (e == hipSuccess) e = rt::launch_rng_prepare(dp.rng_states, (uint32_t)n_pixels, rng->list(), rng->compute_units, stream);
            if (e == hipSuccess && prof) e = hipEventRecord(pe[1], stream);
        }
        rng->ahead = false; /* the chain kernel uses blocks up */
        const bool prof_chain = dist_profile_pairs(DK_CHAIN, 1, pe + 2);
        const bool prof_tail = dist_profile_pairs(DK_SHADE, 2, pe + 4);
        const hipEvent_t *const tail_ev = prof_tail ? pe + 4 : nullptr;
        rng->main_stream = stream;
        /* the pixels in the order of what they cost in the batch that used this workspace last (two batches ago in a pipelined
         * call, the last one else): rt_kernels.h DistParams::pixel_order */
        uint32_t *const pix_cost = rng->pix(), *const pix_order = rng->pix() + (size_t)(1u + b) * n_pixels, *const pix_scratch = rng->pix() + 3u * n_pixels; /* (by_cost: the whole rng, so n_pixels is its count) */
        dp.pixel_cost = c.by_cost ? pix_cost : nullptr;
        dp.pixel_order = c.by_cost && rng->order_valid[b] ? pix_order : nullptr;
        if (e == hipSuccess && prof_chain) e = hipEventRecord(pe[2], stream);
        if (e == hipSuccess) e = rt::launch_dist_chain(c.scene->ks, c.kf, dp, c.dist_waves, stream);
        if (e == hipSuccess && prof_chain) e = hipEventRecord(pe[3], stream);
        /* from here on this batch does not touch the RNG records: the look-ahead for the next one, on its own stream */
        if (e == hipSuccess && c.lookahead) e = lookahead_after_chain(rng);
        if (n_buf == 2u) {
            if (e == hipSuccess) e = hipEventRecord(rng->ev_tail[b], stream); /* first: the chain kernel has written workspace b ... */
            if (e == hipSuccess) e = hipStreamWaitEvent(rng->tail, rng->ev_tail[b], 0);
            /* the next chain kernel waits for the look-ahead, and the look-ahead's workgroups need 64 KB of LDS each: the shade
             * kernel starts after it instead of taking that LDS first (between two chain kernels of a 1/8 share of the 1080p
             * frame 1.1 -> 0.3 ms: 0.38 -> 0.365 ms per epoch, a 1/4 share 0.553 -> 0.517, the whole frame 1.685 -> 1.669) */
            if (e == hipSuccess && c.prep_first && rng->ahead) e = hipStreamWaitEvent(rng->tail, rng->ev_prepared, 0);
            if (e == hipSuccess) e = rt::launch_dist_shade_unwind(c.scene->ks, c.kf, dp, rng->tail, tail_ev);
            if (e == hipSuccess && c.by_cost) {
                e = rt::launch_dist_pixel_order(pix_cost, pix_order, (uint32_t)n_pixels, pix_scratch, rng->tail);
                rng->order_valid[b] = e == hipSuccess;
            }
            if (e == hipSuccess) e = hipEventRecord(rng->ev_tail[b], rng->tail); /* ... then: and the unwind has read it */
            tail_used[b] = e == hipSuccess;
        } else if (e == hipSuccess) {
            e = rt::launch_dist_shade_unwind(c.scene->ks, c.kf, dp, stream, tail_ev);
            if (e == hipSuccess && c.by_cost) {
                e = rt::launch_dist_pixel_order(pix_cost, pix_order, (uint32_t)n_pixels, pix_scratch, stream);
                rng->order_valid[b] = e == hipSuccess;
            }
        }
        /* the next chain kernel — of this call or, on whatever stream is ordered after this one, of the next — needs the prepared blocks */
        if (e == hipSuccess && rng->ahead) e = hipStreamWaitEvent(stream, rng->ev_prepared, 0);
    }
    /* everything the call started is behind the caller's stream again */
    for (uint32_t b = 0; b < 2u; ++b)
        if (tail_used[b]) { const hipError_t e2 = hipStreamWaitEvent(stream, rng->ev_tail[b], 0); if (e == hipSuccess) e = e2; }
    return launched(c.who, e);
}

/* The one-kernel organisation: persistent lanes, the grid's waves take 64-pixel chunks off the stream's chunk counter */
static int dist_one_kernel_pass(const DistCall &c, rt::DistParams dp) {
    uint32_t dist_waves = c.dist_waves;
    dp.n_epochs = c.n_epochs;
    dp.epoch0 = 0;
    dp.sp_hdr = nullptr; dp.sp_req = nullptr; dp.sp_shade = nullptr; dp.sp_frame = nullptr; dp.sp_slots = 0;
    {
        rt_scene *mut = const_cast<rt_scene *>(c.scene);
        std::lock_guard<std::mutex> lock(mut->ws_mutex);
        Workspace &ws = mut->workspaces[c.stream];
        RT_HIP(ensure_counters(ws));
        dp.work_queue = ws.d_counters;
        if (c.scene->ks.bfs_walk != 0u) { /* the breadth-first walk's lists, one set per wave of the grid (shared with the Whitted path of this stream) */
            const uint32_t waves = rt::dist_bfs_waves(c.rng->compute_units);
            const BfsLists bl = bfs_lists(ws, waves, true);
            if (bl.lists != nullptr) { /* (no room: the wave-uniform walk renders the same samples) */
                dp.bfs_scratch = bl.lists;
                dp.bfs_items_cap = bl.items_cap; dp.bfs_jobs_cap = bl.jobs_cap;
                if (dist_waves > waves) dist_waves = waves;
            }
        }
    }
    hipError_t e = hipMemsetAsync(dp.work_queue, 0, sizeof(uint32_t), c.stream);
    if (e == hipSuccess && c.lookahead && !c.rng->ahead) e = rt::launch_rng_prepare(dp.rng_states, (uint32_t)c.n_pixels, c.rng->list(), c.rng->compute_units, c.stream);
    c.rng->ahead = false;
    if (e == hipSuccess) e = rt::launch_distributed(c.scene->ks, c.kf, dp, dist_waves, c.stream);
    return launched(c.who, e);
}

/* The pass behind rt_render_distributed and rt_trace_rays_distributed: kf is a camera frame (make_kernel_frame) or a band of a ray
 * batch (one row of rays, rt_kernels.h frame_set_rays / frame_set_sample_stride); dp comes with what differs between the two — the
 * band's generator records, n_epochs, focus and blur, the outputs — and `first` is the band's first generator within rng (0 for a
 * frame).  Every RT_AMD_DIST_* switch is read here; the split pass is tried first and the one-kernel organisation renders what it
 * has no room for; `who` names the entry point in error messages. */
static int render_distributed_frame(const rt_scene *scene, const rt::KernelFrame &kf, rt_rng *rng, size_t first, rt::DistParams dp,
                                    hipStream_t stream, const char *who) {
    dp.work_queue = nullptr;
    dp.pixel_order = nullptr;
    dp.pixel_cost = nullptr;
    dp.own_first_chunk = 0u;
    dp.bfs_scratch = nullptr;
    dp.bfs_items_cap = dp.bfs_jobs_cap = 0u;
    dp.epoch0 = 0u;
    int split = g_dist_split.load();
    if (split < 0) split = rt::option(rt::OPT_DIST_SPLIT, RT_DIST_SPLIT_DEFAULT) != 0 ? 1 : 0;
    if (scene->ks.bfs_walk != 0u) split = 0; /* a scene beyond the caches: the one-kernel organisation has the breadth-first walk */
    DistCall c = {scene, kf, rng, stream, who, (size_t)kf.cols * kf.rows, dp.n_epochs, scene->resident_waves};
    if (c.n_pixels == 0 || c.n_epochs == 0) return RT_OK;
    const bool whole = first == 0 && c.n_pixels == rng_count(rng); /* not a band of a larger batch: the cost order covers what is launched */
    rng->la_states = dp.rng_states;
    rng->la_count = (uint32_t)c.n_pixels;
    c.lookahead = rt::option(rt::OPT_RNG_LOOKAHEAD, 1) != 0;
    if (split && kf.max_depth <= 254) {
        c.pipeline = rt::option(rt::OPT_DIST_PIPELINE, 1) != 0;
        const bool small_share = (c.n_pixels + 63u) / 64u <= 2u * (size_t)rt::dist_chain_waves(c.dist_waves);
        c.by_cost = whole && rt::option(rt::OPT_DIST_BY_COST, small_share ? 1 : 0) != 0;
        dp.own_first_chunk = rt::option(rt::OPT_DIST_OWN_FIRST, small_share ? 1 : 0) != 0 ? 1u : 0u; /* rt_kernels.h */
        c.prep_first = rt::option(rt::OPT_DIST_PREP_FIRST, 1) != 0;
        c.cap = (size_t)std::max<long long>(0, rt::option(rt::OPT_DIST_WS_MB, c.pipeline ? 32768 : 16384)) << 20;
        bool no_room = false;
        const int rc = dist_split_pass(c, dp, &no_room);
        if (rc != RT_OK || !no_room) return rc;
    }
    return dist_one_kernel_pass(c, dp);
}

/* A ray batch runs in bands of at most this many rays per launch set, whole 64-ray chunks (as RT_TRACE_BAND_RAYS of rt_trace_rays):
 * slot and sample indices inside a launch stay far from what 32 bits hold.  A band works on its own stretch of the generator
 * records, the accumulator and the [epoch][ray] outputs. */
#define RT_DIST_BAND_RAYS (1u << 26)

static int trace_rays_distributed_checks(const char *who, const rt_scene *scene, const void *rays, size_t n_rays, int32_t max_depth,
                                         const rt_rng *rng, uint32_t n_epochs, const void *accum, const void *samples, bool host, bool *nothing) {
    *nothing = false;
    int rc = check_count(who, n_rays, {32u, "rays", "trace them in several calls"});
    if (rc == RT_OK) rc = check_scene(who, scene);
    if (rc != RT_OK) return rc;
    if (!rng) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": null rng");
    if (n_rays != rng_count(rng)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": the RNG holds a different number of generators than there are rays");
    if (n_rays == 0 || n_epochs == 0) { *nothing = true; return RT_OK; }
    rc = check_pointers(who, rays != nullptr, "ray");
    if (rc == RT_OK && host) rc = check_pointers(who, accum != nullptr, "accum");
    if (rc != RT_OK) return rc;
    if (!host && !accum && !samples) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": need d_accum or d_samples");
    if (max_depth > RT_MAX_DEPTH) return fail(RT_ERR_UNSUPPORTED, std::string(who) + ": max_depth above RT_MAX_DEPTH");
    return RT_OK;
}

extern "C" {

int rt_render_distributed(const rt_scene *scene, const rt_camera *camera, const rt_frame *frame, float focus, float blur,
                          rt_rng *rng, uint32_t n_epochs, float *d_accum, float *d_samples, unsigned char *d_valid,
                          unsigned long long *d_ray_count, void *hip_stream) {
    if (!scene || !rng) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_distributed: null argument");
    if (!d_accum && !d_samples) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_distributed: need d_accum or d_samples");
    rt::KernelFrame kf;
    int rc = make_kernel_frame(camera, frame, &kf);
    if (rc != RT_OK) return rc;
    if (kf.cols != rng->cols || kf.rows != rng->rows || kf.x0 != rng->x0 || kf.y0 != rng->y0 || kf.y_step != rng->y_step)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_distributed: the RNG was created for a different tile");
    rt::DistParams dp;
    memset(&dp, 0, sizeof dp);
    dp.rng_states = rng->states();
    dp.n_epochs = n_epochs;
    dp.focus = focus;
    dp.blur = blur;
    dp.accum = d_accum;
    dp.samples = d_samples;
    dp.valid = d_valid;
    dp.ray_count = d_ray_count;
    return render_distributed_frame(scene, kf, rng, 0, dp, static_cast<hipStream_t>(hip_stream), "rt_render_distributed");
}

int rt_trace_rays_distributed(const rt_scene *scene, const rt_ray *d_rays, size_t n_rays, int32_t max_depth, rt_rng *rng, uint32_t n_epochs,
                              float *d_accum, float *d_samples, unsigned char *d_valid, unsigned long long *d_ray_count, void *hip_stream) {
    bool nothing = false;
    const int rc0 = trace_rays_distributed_checks("rt_trace_rays_distributed", scene, d_rays, n_rays, max_depth, rng, n_epochs, d_accum, d_samples, false, &nothing);
    if (rc0 != RT_OK || nothing) return rc0;
    /* max_depth < 0 renders as 0, as in rt_render_distributed (distributed_ray_trace tests `depth <= 0`, main.rs:524) */
    const uint32_t n = (uint32_t)n_rays;
    const uint64_t band = band_limit(rt::OPT_DIAG_DIST_BAND_RAYS, RT_DIST_BAND_RAYS); /* the option: a test hook, shorter bands */
    const bool ahead0 = rng->ahead; /* the records of the bands still to come are as the call found them */
    for (uint64_t u0 = 0; u0 < n; u0 += band) {
        const uint32_t len = (uint32_t)std::min<uint64_t>(band, n - u0);
        rt::KernelFrame kf;
        memset(&kf, 0, sizeof kf);
        kf.cols = len;
        kf.rows = 1u;
        kf.max_depth = max_depth;
        rt::frame_set_rays(&kf, d_rays + u0, 0.0f);
        rt::frame_set_sample_stride(&kf, n);
        rt::DistParams dp;
        memset(&dp, 0, sizeof dp);
        dp.rng_states = rng->states() + (size_t)u0 * RT_RNG_DEVICE_WORDS;
        dp.n_epochs = n_epochs;
        dp.accum = d_accum ? d_accum + (size_t)u0 * 3u : nullptr;
        dp.samples = d_samples ? d_samples + (size_t)u0 * 3u : nullptr;
        dp.valid = d_valid ? d_valid + (size_t)u0 : nullptr;
        dp.ray_count = d_ray_count;
        rng->ahead = ahead0;
        const int rc = render_distributed_frame(scene, kf, rng, (size_t)u0, dp, static_cast<hipStream_t>(hip_stream), "rt_trace_rays_distributed");
        if (rc != RT_OK) { rng->ahead = false; return rc; }
    }
    return RT_OK;
}

int rt_trace_rays_distributed_host(const rt_scene *scene, const rt_ray *h_rays, size_t n_rays, int32_t max_depth, rt_rng *rng, uint32_t n_epochs,
                                   float *h_accum, unsigned long long *h_ray_count) {
    bool nothing = false;
    const int rc0 = trace_rays_distributed_checks("rt_trace_rays_distributed_host", scene, h_rays, n_rays, max_depth, rng, n_epochs, h_accum, nullptr, true, &nothing);
    if (rc0 != RT_OK) return rc0;
    if (nothing) {
        if (h_ray_count) *h_ray_count = 0;
        return RT_OK;
    }
    HostRoundTrip t("rt_trace_rays_distributed_host");
    const rt_ray *d_rays = t.in(h_rays, n_rays * sizeof(rt_ray));
    float *d_accum = t.inout(h_accum, n_rays * 3 * sizeof(float));
    unsigned long long *d_cnt = t.counter();
    if (!t.ok()) return t.failed();
    const int rc = rt_trace_rays_distributed(scene, d_rays, n_rays, max_depth, rng, n_epochs, d_accum, nullptr, nullptr, d_cnt, nullptr);
    return rc != RT_OK ? rc : t.finish(h_ray_count);
}

int rt_focus_rays(const rt_camera *camera, const rt_frame *frame, float focus, float blur, rt_rng *rng, rt_ray *d_rays, void *hip_stream) {
    if (!camera || !frame || !rng) return fail(RT_ERR_INVALID_ARGUMENT, "rt_focus_rays: null argument");
    if (!frame_ok(frame)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_focus_rays: bad frame (need 0 <= x0 < x1 <= width, 0 <= y0 < y1 <= height, y_step >= 1)");
    if (!d_rays) return fail(RT_ERR_INVALID_ARGUMENT, "rt_focus_rays: null ray pointer");
    rt_frame f = *frame;
    f.max_depth = 0; /* not used here */
    rt::KernelFrame kf;
    const int rc = make_kernel_frame(camera, &f, &kf); /* refuses a tile of 2^32 pixels or more */
    if (rc != RT_OK) return rc;
    const bool same_tile = kf.cols == rng->cols && kf.rows == rng->rows && kf.x0 == rng->x0 && kf.y0 == rng->y0 && kf.y_step == rng->y_step;
    const bool seeded_same_count = rng->y_step == 0u && (size_t)kf.cols * kf.rows == rng_count(rng);
    if (!same_tile && !seeded_same_count)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_focus_rays: the RNG was created for a different tile (or, seeded, holds a different number of generators)");
    const hipError_t e = rt::launch_focus_rays(kf, focus, blur, rng->states(), d_rays, static_cast<hipStream_t>(hip_stream));
    if (e == hipSuccess) rng->ahead = false; /* a generator may have moved on to its prepared block: the next call looks */
    return launched("rt_focus_rays", e);
}

int rt_render_distributed_host(const rt_scene *scene, const rt_camera *camera, const rt_frame *frame, float focus, float blur,
                               rt_rng *rng, uint32_t n_epochs, float *h_accum, unsigned long long *h_ray_count) {
    if (!scene || !rng || !h_accum) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_distributed_host: null argument");
    if (!frame_ok(frame)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_distributed_host: bad frame");
    HostRoundTrip t("rt_render_distributed_host");
    float *d_accum = t.inout(h_accum, (size_t)rt_frame_pixels(frame) * 3 * sizeof(float)); /* img continues from the caller's sums */
    unsigned long long *d_cnt = t.counter();
    if (!t.ok()) return t.failed();
    const int rc = rt_render_distributed(scene, camera, frame, focus, blur, rng, n_epochs, d_accum, nullptr, nullptr, d_cnt, nullptr);
    return rc != RT_OK ? rc : t.finish(h_ray_count);
}

} /* extern "C" */
