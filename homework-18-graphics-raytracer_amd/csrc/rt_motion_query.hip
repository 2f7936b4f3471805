/*
 * rt_motion_query.hip — the motion queries (include/rt_amd.h "motion queries"): the positions a scene keeps before it is updated, and
 * where each hit's point was on them; kernels and entry points in one unit.
 *
 *   rt::each_kernel<KeepPositions>  one primitive per lane, triangles and spheres in one launch: three 16-byte loads and stores per
 *                                  triangle, one per sphere
 *   rt::each_kernel<MotionRecords>  one hit per lane: the hit's kind, index and position as dwords, then the primitive's record and its
 *                                  kept pieces as 16-byte loads
 * (rt_image_kernel.h has the element loop and its launch)
 *
 * The arithmetic is rt_motion.h's, shared with librt_host.so: the kernel calls motion_record on the same operands as
 * rt_previous_positions_cpu, so it gives the same bits by construction, whatever the launch geometry.  The kind branch is left
 * divergent (mixed waves are the normal case at silhouettes).  The gathers are data-dependent, but hits of primary rays are coherent —
 * neighbouring lanes name the same primitive — and are served by the caches: nothing is staged in LDS.  Every index is checked against
 * its array before anything is read with it; the record number and the output index are 64-bit.  No atomics, no workspace.
 */
#include "rt_image_kernel.h"
#include "rt_motion.h"

namespace rt {

/* primitive i of rt_scene_keep_positions, the triangles first */
struct KeepPositions {
    const DevTri *tris;
    const DevSphere *spheres;
    uint32_t n_triangles, n_spheres;
    MotionPiece *kept;
    __host__ __device__ uint64_t count() const { return (uint64_t)n_triangles + n_spheres; }
    __device__ void operator()(uint64_t i) const {
        if (i < n_triangles) {
            const unsigned char *T = reinterpret_cast<const unsigned char *>(tris + i);
            MotionPiece v0 = motion_load(T + 16), v1 = motion_load(T + 32), v2 = motion_load(T + 48); /* v0 obj | v1 area | v2 bq */
            v0.w = v1.w = v2.w = 0.0f;
            MotionPiece *k = kept + RT_MOTION_TRI_PIECES * i;
            k[0] = v0, k[1] = v1, k[2] = v2;
        } else {
            kept[(uint64_t)RT_MOTION_TRI_PIECES * n_triangles + (i - n_triangles)] = motion_load(spheres + (i - n_triangles)); /* c radius */
        }
    }
};

} /* namespace rt */

extern "C" {

int rt_scene_keep_positions(rt_scene *scene, void *hip_stream) {
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "rt_scene_keep_positions: null scene");
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    KeptPositions &k = scene->kept;
    const uint32_t n_triangles = scene->ks.n_triangles, n_spheres = scene->ks.n_spheres;
    const size_t bytes = rt::motion_kept_pieces(n_triangles, n_spheres) * sizeof(rt::MotionPiece);
    {
        std::lock_guard<std::mutex> lock(k.mutex);
        if (k.d_pieces.bytes() < bytes) { /* the first keep of a scene: the counts never change afterwards */
            if (stream_capturing(stream)) return fail(RT_ERR_UNSUPPORTED, "rt_scene_keep_positions: the first keep of a scene allocates and cannot be captured");
            const hipError_t e = k.d_pieces.reserve(bytes);
            if (e != hipSuccess) return fail_hip("rt_scene_keep_positions: hipMalloc of the kept positions", e);
        }
    }
    if (bytes != 0u) {
        const rt::KeepPositions keep = {scene->ks.tris, scene->ks.spheres, n_triangles, n_spheres, k.d_pieces.get<rt::MotionPiece>()};
        const int rc = launched("rt_scene_keep_positions", rt::launch_each(keep, rt::OPT_DIAG_MOTION_MAX_GROUPS, stream));
        if (rc != RT_OK) return rc;
    }
    k.kept.store(true);
    return RT_OK;
}

int rt_scene_positions_kept(const rt_scene *scene) {
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "rt_scene_positions_kept: null scene");
    return scene->kept.kept.load() ? 1 : 0;
}

int rt_previous_positions(const rt_scene *scene, const rt_hit *d_hits, size_t n, float *d_was, uint32_t was_stride, void *hip_stream) {
    int status;
    bool done;
    const char *bad = rt::motion_limits(n, scene, scene && scene->kept.kept.load(), RT_MOTION_NOT_KEPT, d_hits, d_was, was_stride, &status, &done);
    if (bad) return fail(status, std::string("rt_previous_positions: ") + bad);
    if (done) return RT_OK;
    const rt::MotionRecords m = {{scene->ks.tris, scene->ks.spheres, scene->kept.d_pieces.get<rt::MotionPiece>(), scene->ks.n_triangles, scene->ks.n_spheres},
                                 d_hits, (uint64_t)n, d_was, was_stride};
    return launched("rt_previous_positions", rt::launch_each(m, rt::OPT_DIAG_MOTION_MAX_GROUPS, static_cast<hipStream_t>(hip_stream)));
}

int rt_previous_positions_host(const rt_scene *scene, const rt_hit *h_hits, size_t n, float *h_was, uint32_t was_stride) {
    int status;
    bool done;
    const char *bad = rt::motion_limits(n, scene, scene && scene->kept.kept.load(), RT_MOTION_NOT_KEPT, h_hits, h_was, was_stride, &status, &done);
    if (bad) return fail(status, std::string("rt_previous_positions_host: ") + bad);
    if (done) return RT_OK;
    /* a strided plane travels as the span from its first word to its last, and goes up as well as down: the words between the
     * records come back as they were */
    if ((n - 1u) > (std::numeric_limits<size_t>::max() / sizeof(float) - 3u) / was_stride)
        return fail(RT_ERR_UNSUPPORTED, "rt_previous_positions_host: n * was_stride words do not fit a size_t");
    const size_t span = ((n - 1u) * was_stride + 3u) * sizeof(float);
    HostRoundTrip t("rt_previous_positions_host");
    const rt_hit *d_hits = t.in(h_hits, n * sizeof(rt_hit));
    float *d_was = was_stride == 3u ? t.out(h_was, span) : t.inout(h_was, span);
    if (!t.ok()) return t.failed();
    const int rc = rt_previous_positions(scene, d_hits, n, d_was, was_stride, nullptr);
    return rc != RT_OK ? rc : t.finish();
}

} /* extern "C" */
