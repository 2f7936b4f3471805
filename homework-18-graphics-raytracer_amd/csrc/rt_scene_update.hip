/*
 * rt_scene_update.hip — rt_scene_update_vertices / _spheres / _lights / _materials (include/rt_amd.h "scene updates"): kernels and
 * entry points in one unit.
 *
 * Everything rt_scene_create derives (rt_api_layout.hip) is one of two kinds.  EXACT values — n, d, v*, e*, area, r2, the
 * attributes — are pure functions of one primitive in the reference's operation order: the kernels below evaluate them with the
 * same rt_vec.h helpers under the same flags, so they are bit for bit what a fresh rt_scene_create writes.  CONSERVATIVE data —
 * bq / bc, the node spheres, the normals or the cone, q_miss, the plane-sharing bits — never decide an accept; they have to be
 * VALID under the rules of rt_device_scene.h, and they are rebuilt here by those rules over the node array as it stands: its
 * topology, the counts and every object index are fixed at creation.  A cast on an updated scene is then the cast of a fresh
 * scene of the same description.
 *
 * The scene's box is the one it was created with (rt_scene::upd.extent): KernelScene::filter_origin2 travels by value and is baked
 * into captured graphs.  A triangle with a coordinate outside it loses its own rejection (bq = +inf), and with it every node above.
 *
 * A node that no longer qualifies is written as n_normals = 0 with r2_hi = +inf: each of the three walkers — cast_asm and
 * cast_pairs (rt_cast.h) and cast_bfs (rt_cast_bfs.h) — tests a node's sphere only when n_normals != 0, and with n_normals == 0
 * visits a leaf's triangles and descends into an inner node; r2_hi = +inf says the same once more (no line misses that sphere).
 */
#include "rt_api_internal.h"

namespace {

struct UpdScene {
    rt::DevTri *tris;
    rt::DevTriAttr *attrs;
    rt::DevTriHead *heads;
    rt::DevSegment *segments, *bfs_nodes;
    float4 *soa; /* KernelScene::bfs_soa */
    uint32_t n_triangles, n_segments;
    double extent; /* of the scene at creation */
};

/* bq / bc by the rules of rt_api_layout.hip (the bounding spheres): binary64, the finite / angle / size tests, and a sphere that
 * contains the three vertices whatever the rounding did.  +inf: the rejection is off for this triangle. */
__device__ float tri_bound(const double (&P)[3][3], double extent, float bc[3]) {
    const float inf = __builtin_inff();
    bc[0] = bc[1] = bc[2] = 0.0f;
    bool finite = true;
    for (int v = 0; v < 3; ++v)
        for (int k = 0; k < 3; ++k) finite = finite && isfinite(P[v][k]) && fabs(P[v][k]) <= extent; /* inside the creation box */
    if (!finite || !(extent <= 1e10)) return inf;
    double ab[3], ac[3], bc3[3];
    for (int k = 0; k < 3; ++k) { ab[k] = P[1][k] - P[0][k]; ac[k] = P[2][k] - P[0][k]; bc3[k] = P[2][k] - P[1][k]; }
    auto dotd = [](const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    const double la = dotd(bc3, bc3), lb = dotd(ac, ac), lc = dotd(ab, ab);
    if (!(la > 0.0 && lb > 0.0 && lc > 0.0)) return inf;
    const double cr[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
    const double twice_area = sqrt(dotd(cr, cr));
    const double angA = atan2(twice_area, dotd(ab, ac));
    const double angB = atan2(twice_area, -dotd(ab, bc3));
    const double angC = atan2(twice_area, dotd(ac, bc3));
    const double ang_min = angA < angB ? (angA < angC ? angA : angC) : (angB < angC ? angB : angC);
    if (!(ang_min >= 0.0201)) return inf;
    double c[3], r2;
    if (la >= lb + lc) { for (int k = 0; k < 3; ++k) c[k] = 0.5 * (P[1][k] + P[2][k]); r2 = 0.25 * la; }
    else if (lb >= la + lc) { for (int k = 0; k < 3; ++k) c[k] = 0.5 * (P[0][k] + P[2][k]); r2 = 0.25 * lb; }
    else if (lc >= la + lb) { for (int k = 0; k < 3; ++k) c[k] = 0.5 * (P[0][k] + P[1][k]); r2 = 0.25 * lc; }
    else {
        const double wa = la * (lb + lc - la), wb = lb * (lc + la - lb), wc = lc * (la + lb - lc);
        const double w = wa + wb + wc;
        for (int k = 0; k < 3; ++k) c[k] = (wa * P[0][k] + wb * P[1][k] + wc * P[2][k]) / w;
        const double d0[3] = {P[0][0] - c[0], P[0][1] - c[1], P[0][2] - c[2]};
        r2 = dotd(d0, d0);
    }
    for (int v = 0; v < 3; ++v) {
        const double dv[3] = {P[v][0] - c[0], P[v][1] - c[1], P[v][2] - c[2]};
        const double q = dotd(dv, dv);
        if (q > r2) r2 = q;
    }
    const double radius = sqrt(r2);
    if (!(radius <= 0.5 * extent)) return inf;
    if (!(radius >= 1e-3 * extent) || !isfinite(radius)) return inf;
    bc[0] = (float)c[0]; bc[1] = (float)c[1]; bc[2] = (float)c[2];
    return nextafterf((float)(1.05 * r2 * 1.0001), inf);
}

/* One triangle per lane: DevTri (but for obj), DevTriAttr, DevTriHead and the two 16-byte pieces of the breadth-first walk, from
 * the new vertices — rt_api_layout.hip's per-triangle loop, operation for operation. */
__global__ void __launch_bounds__(256) update_triangles(UpdScene sc, const rt_vertex *vertices, uint32_t first, uint32_t count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint32_t at = first + i; /* < n_triangles: checked by the entry point */
    using rt::V3;
    const rt_vertex s0 = vertices[3u * (size_t)i], s1 = vertices[3u * (size_t)i + 1u], s2 = vertices[3u * (size_t)i + 2u];
    const V3 v0 = rt::v3p(s0.position), v1 = rt::v3p(s1.position), v2 = rt::v3p(s2.position);
    const V3 n = rt::normalize(rt::cross(v1 - v0, v2 - v1)); /* Triangle::face_normal, primitives.rs:36-42 */
    const float d = rt::dot(n, v0);                          /* main.rs:203 */
    const V3 e0 = v2 - v1, e1 = v0 - v2, e2 = v1 - v0;       /* main.rs:219-221 */
    const float area = rt::dot(rt::cross(v1 - v0, v2 - v0), n); /* main.rs:235 */
    const double P[3][3] = {{(double)v0.x, (double)v0.y, (double)v0.z}, {(double)v1.x, (double)v1.y, (double)v1.z}, {(double)v2.x, (double)v2.y, (double)v2.z}};
    float bc[3];
    const float bq = tri_bound(P, sc.extent, bc);
    rt::DevTri &t = sc.tris[at];
    t.n[0] = n.x; t.n[1] = n.y; t.n[2] = n.z; t.d = d;
    t.v0[0] = v0.x; t.v0[1] = v0.y; t.v0[2] = v0.z; /* obj stays: its index is fixed, its flags are update_plane_sharing's */
    t.v1[0] = v1.x; t.v1[1] = v1.y; t.v1[2] = v1.z; t.area = area;
    t.v2[0] = v2.x; t.v2[1] = v2.y; t.v2[2] = v2.z; t.bq = bq;
    t.e0[0] = e0.x; t.e0[1] = e0.y; t.e0[2] = e0.z; t.bcx = bc[0];
    t.e1[0] = e1.x; t.e1[1] = e1.y; t.e1[2] = e1.z; t.bcy = bc[1];
    t.e2[0] = e2.x; t.e2[1] = e2.y; t.e2[2] = e2.z; t.bcz = bc[2];
    rt::DevTriAttr &a = sc.attrs[at];
    for (int k = 0; k < 3; ++k) { a.n0[k] = s0.normal[k]; a.n1[k] = s1.normal[k]; a.n2[k] = s2.normal[k]; }
    a.uv0x = s0.uv[0]; a.uv0y = s0.uv[1];
    a.uv1x = s1.uv[0]; a.uv1y = s1.uv[1];
    a.uv2x = s2.uv[0]; a.uv2y = s2.uv[1];
    const float4 plane = make_float4(n.x, n.y, n.z, d), bound = make_float4(bc[0], bc[1], bc[2], bq);
    float4 *h = reinterpret_cast<float4 *>(sc.heads + at);
    h[0] = plane;
    h[1] = bound;
    float4 *planes = sc.soa + 3u * (size_t)sc.n_segments;
    planes[at] = plane;
    planes[(size_t)sc.n_triangles + at] = bound;
}

/* RT_TRI_FOLLOWS / _WEAK of triangles [from, to), each against its predecessor (rt_api_layout.hip, "triangles on their
 * predecessor's plane"); runs after update_triangles. */
__global__ void __launch_bounds__(256) update_plane_sharing(UpdScene sc, uint32_t from, uint32_t to) {
    const uint32_t i = from + blockIdx.x * 256u + threadIdx.x; /* from >= 1 */
    if (i >= to) return;
    const uint32_t obj = sc.tris[i].obj & RT_TRI_OBJ_MASK;
    uint32_t flags = 0u;
    if ((sc.tris[i - 1u].obj & RT_TRI_OBJ_MASK) == obj) {
        const float a[4] = {sc.tris[i - 1u].n[0], sc.tris[i - 1u].n[1], sc.tris[i - 1u].n[2], sc.tris[i - 1u].d};
        const float b[4] = {sc.tris[i].n[0], sc.tris[i].n[1], sc.tris[i].n[2], sc.tris[i].d};
        bool exact = true, weak = true;
        for (int k = 0; k < 4; ++k) {
            const bool same_bits = __float_as_uint(a[k]) == __float_as_uint(b[k]);
            exact = exact && same_bits;
            weak = weak && (same_bits || (a[k] == 0.0f && b[k] == 0.0f));
        }
        flags = exact ? RT_TRI_FOLLOWS : (weak ? (RT_TRI_FOLLOWS | RT_TRI_FOLLOWS_WEAK) : 0u);
    }
    sc.tris[i].obj = obj | flags;
}

/* v of every thread of the workgroup combined, in a fixed order, the same value in every thread */
template <int T, class Op>
__device__ double group_reduce(double v, Op op, double *lds) {
    for (int o = 32; o != 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    if (T > 64) {
        __syncthreads();
        if ((threadIdx.x & 63u) == 0u) lds[threadIdx.x >> 6] = v;
        __syncthreads();
        v = lds[0];
        for (int w = 1; w < T / 64; ++w) v = op(v, lds[w]);
    }
    return v;
}

__device__ void canonical_normal(const rt::DevTri &t, float n[3]) {
    n[0] = t.n[0]; n[1] = t.n[1]; n[2] = t.n[2];
    const int lead = fabsf(n[0]) > 1e-3f ? 0 : (fabsf(n[1]) > 1e-3f ? 1 : 2);
    if (n[lead] < 0.0f) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
}

/* node_stats of rt_api_layout.hip for one node per workgroup of T threads, over the node's unchanged triangle range: the box
 * centre, the reach, r2_hi, up to 8 representative normals or the cone with the same slack constants — from scratch, so a node
 * re-qualifies by itself when the geometry comes back.  The sequential "first unknown normal becomes a representative" loop is
 * the same set taken in rounds: the unknown triangle of the lowest index donates its normal, every triangle within 1e-4 per
 * component of a representative is known, eight rounds at most. */
template <int T>
__global__ void __launch_bounds__(T) refit_nodes(UpdScene sc, const RefitNode *list, uint32_t n_list) {
    __shared__ double lds[T / 64 > 1 ? T / 64 : 1];
    __shared__ float reps[RT_SEGMENT_NORMALS][3];
    if (blockIdx.x >= n_list) return;
    const RefitNode node = list[blockIdx.x];
    const uint32_t lo_t = node.lo, hi_t = node.hi, tid = threadIdx.x;
    const float inf = __builtin_inff();
    auto fmin2 = [](double a, double b) { return b < a ? b : a; };
    auto fmax2 = [](double a, double b) { return b > a ? b : a; };
    auto add2 = [](double a, double b) { return a + b; };

    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (uint32_t k = lo_t + tid; k < hi_t; k += T) {
        const rt::DevTri &t = sc.tris[k];
        const float *vs[3] = {t.v0, t.v1, t.v2};
        for (int v = 0; v < 3; ++v)
            for (int a = 0; a < 3; ++a) {
                const double x = (double)vs[v][a];
                if (x < lo[a]) lo[a] = x;
                if (x > hi[a]) hi[a] = x;
            }
    }
    float c[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = group_reduce<T>(lo[a], fmin2, lds);
        hi[a] = group_reduce<T>(hi[a], fmax2, lds);
        c[a] = (float)(0.5 * (lo[a] + hi[a]));
    }
    /* the sphere must contain every triangle's own bounding sphere; the cone's axis: the mean of the normals, each flipped into the
     * first one's half-space */
    const float first_n[3] = {sc.tris[lo_t].n[0], sc.tris[lo_t].n[1], sc.tris[lo_t].n[2]};
    double r2 = 0.0, bad = 0.0, mean[3] = {0.0, 0.0, 0.0};
    for (uint32_t k = lo_t + tid; k < hi_t; k += T) {
        const rt::DevTri &t = sc.tris[k];
        const double dx = (double)t.bcx - c[0], dy = (double)t.bcy - c[1], dz = (double)t.bcz - c[2];
        const double reach = sqrt(dx * dx + dy * dy + dz * dz) + sqrt((double)t.bq);
        if (reach * reach > r2) r2 = reach * reach;
        if (!(reach == reach) || !(isfinite(t.n[0]) && isfinite(t.n[1]) && isfinite(t.n[2]))) bad = 1.0;
        const double s = ((double)t.n[0] * first_n[0] + (double)t.n[1] * first_n[1] + (double)t.n[2] * first_n[2]) < 0.0 ? -1.0 : 1.0;
        for (int a = 0; a < 3; ++a) mean[a] += s * (double)t.n[a];
    }
    r2 = group_reduce<T>(r2, fmax2, lds);
    bad = group_reduce<T>(bad, fmax2, lds);
    for (int a = 0; a < 3; ++a) mean[a] = group_reduce<T>(mean[a], add2, lds);
    const double radius = sqrt(r2);
    bool ok = bad == 0.0 && isfinite(radius) && radius <= 0.5 * sc.extent && radius >= 1e-3 * sc.extent;

    uint32_t n_normals = 0u, n_reps = 0u;
    float cone[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (ok) { /* (wave-uniform, and the same in every wave of the workgroup) */
        bool explicit_ok = true;
        uint32_t k = lo_t + tid;
        for (;;) {
            for (; k < hi_t; k += T) { /* known triangles stay known: each thread only ever moves forward */
                float n[3];
                canonical_normal(sc.tris[k], n);
                bool known = false;
                for (uint32_t q = 0; q < n_normals && !known; ++q)
                    known = fabsf(reps[q][0] - n[0]) <= 1e-4f && fabsf(reps[q][1] - n[1]) <= 1e-4f && fabsf(reps[q][2] - n[2]) <= 1e-4f;
                if (!known) break;
            }
            const double donor = group_reduce<T>(k < hi_t ? (double)k : 4.0e9, fmin2, lds);
            if (donor >= 4.0e9) break;
            if (n_normals == RT_SEGMENT_NORMALS) { explicit_ok = false; break; }
            __syncthreads(); /* everybody is done comparing with the representatives so far */
            if (k < hi_t && (double)k == donor) {
                float n[3];
                canonical_normal(sc.tris[k], n);
                reps[n_normals][0] = n[0]; reps[n_normals][1] = n[1]; reps[n_normals][2] = n[2];
            }
            __syncthreads();
            n_normals += 1u;
        }
        if (!(explicit_ok && n_normals != 0u)) { /* more than 8 plane directions: a cone (rt_api_layout.hip for the derivation of K) */
            n_reps = n_normals; /* node_stats leaves the representatives it found behind the cone: so does the record here */
            n_normals = 0u;
            const double ml = sqrt(mean[0] * mean[0] + mean[1] * mean[1] + mean[2] * mean[2]);
            ok = ml > 1e-6;
            float ax[3] = {0.0f, 0.0f, 0.0f};
            if (ok)
                for (int a = 0; a < 3; ++a) ax[a] = (float)(mean[a] / ml);
            const double al = sqrt((double)ax[0] * ax[0] + (double)ax[1] * ax[1] + (double)ax[2] * ax[2]); /* of the ROUNDED axis */
            double cos_min = 1.0, fails = 0.0;
            for (uint32_t j = lo_t + tid; ok && j < hi_t; j += T) {
                const rt::DevTri &t = sc.tris[j];
                const double nl = sqrt((double)t.n[0] * t.n[0] + (double)t.n[1] * t.n[1] + (double)t.n[2] * t.n[2]);
                const double cs = fabs(((double)t.n[0] * ax[0] + (double)t.n[1] * ax[1] + (double)t.n[2] * ax[2]) / (nl * al));
                if (!(cs <= 1.0)) { if (cs > 1.0 && cs < 1.0 + 1e-9) continue; fails = 1.0; continue; }
                if (cs < cos_min) cos_min = cs;
            }
            cos_min = group_reduce<T>(cos_min, fmin2, lds);
            fails = group_reduce<T>(fails, fmax2, lds);
            ok = ok && fails == 0.0;
            const double theta = acos(cos_min) + 1e-5; /* slack for everything rounded on the way */
            ok = ok && theta < 1.0471975511965976;     /* 60 degrees */
            const double K = (1.01e-3 + sin(theta)) / cos(theta) * 1.0001;
            ok = ok && K < 1.0;
            if (ok) {
                n_normals = RT_SEGMENT_CONE;
                cone[0] = ax[0]; cone[1] = ax[1]; cone[2] = ax[2];
                cone[3] = nextafterf((float)(K * K * al * al * 1.0001), inf);
            }
        }
    }
    if (tid != 0u) return;
    /* the record in its three places; first, count, skip_to and the dealing words (they depend on counts only) stay */
    rt::DevSegment *recs[2] = {sc.segments + node.seg, sc.bfs_nodes + node.bfs_pos};
    const float r2_hi = ok ? nextafterf((float)(r2 * 1.0001), inf) : inf;
    if (!ok) { n_normals = 0u; c[0] = c[1] = c[2] = 0.0f; }
    for (int r = 0; r < 2; ++r) {
        rt::DevSegment &g = *recs[r];
        g.n_normals = n_normals;
        g.r2_hi = r2_hi;
        g.c[0] = c[0]; g.c[1] = c[1]; g.c[2] = c[2];
        for (uint32_t q = 0; q < RT_SEGMENT_NORMALS; ++q) {
            const bool have = n_normals != RT_SEGMENT_CONE ? q < n_normals : (q != 0u && q < n_reps);
            g.normals[q][0] = have ? reps[q][0] : (q == 0u ? cone[0] : 0.0f);
            g.normals[q][1] = have ? reps[q][1] : (q == 0u ? cone[1] : 0.0f);
            g.normals[q][2] = have ? reps[q][2] : (q == 0u ? cone[2] : 0.0f);
        }
        g.normals[0][3] = cone[3];
    }
    float *piece0 = reinterpret_cast<float *>(sc.soa + node.bfs_pos); /* first, count, n_normals, r2_hi */
    piece0[2] = __uint_as_float(n_normals);
    piece0[3] = r2_hi;
    float *piece1 = reinterpret_cast<float *>(sc.soa + (size_t)sc.n_segments + node.bfs_pos); /* centre, child count */
    piece1[0] = c[0]; piece1[1] = c[1]; piece1[2] = c[2];
    const rt::DevSegment &g = *recs[0];
    sc.soa[2u * (size_t)sc.n_segments + node.bfs_pos] = make_float4(g.normals[0][0], g.normals[0][1], g.normals[0][2], g.normals[0][3]);
}

/* DevSphere from rt_sphere (rt_api_layout.hip, the spheres): obj is kept */
__global__ void __launch_bounds__(256) update_spheres(rt::DevSphere *spheres, const rt_sphere *in, uint32_t first, uint32_t count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const rt_sphere s = in[i];
    rt::DevSphere &d = spheres[first + i];
    d.c[0] = s.center[0]; d.c[1] = s.center[1]; d.c[2] = s.center[2];
    d.radius = s.radius;
    d.r2 = s.radius * s.radius; /* radius.powi(2), main.rs:272 */
    float q_miss = __builtin_inff();
    if (isfinite(s.radius) && s.radius > 0.0f) {
        const double up = (double)s.radius * (1.0 + 0x1p-22);
        const float q = nextafterf((float)(up * up), __builtin_inff());
        if (isfinite(q)) q_miss = q;
    }
    d.q_miss = q_miss;
}

UpdScene upd_scene(const rt_scene *scene) {
    UpdScene u;
    u.tris = const_cast<rt::DevTri *>(scene->ks.tris);
    u.attrs = const_cast<rt::DevTriAttr *>(scene->ks.attrs);
    u.heads = const_cast<rt::DevTriHead *>(scene->ks.heads);
    u.segments = const_cast<rt::DevSegment *>(scene->ks.segments);
    u.bfs_nodes = const_cast<rt::DevSegment *>(scene->ks.bfs_nodes);
    u.soa = const_cast<float4 *>(scene->ks.bfs_soa);
    u.n_triangles = scene->ks.n_triangles;
    u.n_segments = scene->ks.n_segments;
    u.extent = scene->upd.extent;
    return u;
}

/* the house order of the argument checks, before any device work; 1: nothing to do */
int check_range(const char *who, uint32_t first, uint32_t count, uint32_t have, const void *data) {
    if ((uint64_t)first + (uint64_t)count > (uint64_t)have) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": first + count is beyond the scene's array");
    if (count == 0u) return 1;
    if (!data) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": null data pointer");
    return RT_OK;
}

/* Host records staged in the scene's pinned buffer and copied from there on the stream.  The buffer is one: a call waits for the
 * copies of the call before it. */
int stage_and_copy(rt_scene *scene, const char *who, hipStream_t stream, void *d_a, const void *h_a, size_t bytes_a, void *d_b, const void *h_b,
                   size_t bytes_b) {
    if (stream_capturing(stream)) return fail(RT_ERR_UNSUPPORTED, std::string(who) + ": the stream is being captured (the records are read from host memory at the call)");
    SceneUpdate &u = scene->upd;
    std::lock_guard<std::mutex> lock(u.mutex);
    const size_t need = bytes_a + bytes_b;
    if (u.h_stage.bytes() < need) {
        if (u.stage_event) RT_HIP(hipEventSynchronize(u.stage_event));
        const hipError_t e = u.h_stage.reserve(need);
        if (e != hipSuccess) return fail_hip("hipHostMalloc(&u.h_stage, need, hipHostMallocDefault)", e);
    }
    if (!u.stage_event) RT_HIP(hipEventCreateWithFlags(&u.stage_event, hipEventDisableTiming));
    else RT_HIP(hipEventSynchronize(u.stage_event));
    unsigned char *stage = u.h_stage.get<unsigned char>();
    memcpy(stage, h_a, bytes_a);
    if (bytes_b) memcpy(stage + bytes_a, h_b, bytes_b);
    RT_HIP(hipMemcpyAsync(d_a, stage, bytes_a, hipMemcpyHostToDevice, stream));
    if (bytes_b) RT_HIP(hipMemcpyAsync(d_b, stage + bytes_a, bytes_b, hipMemcpyHostToDevice, stream));
    RT_HIP(hipEventRecord(u.stage_event, stream));
    return RT_OK;
}

} /* namespace */

extern "C" {

int rt_scene_update_vertices(rt_scene *scene, uint32_t first, uint32_t count, const rt_vertex *d_vertices, void *hip_stream) {
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "rt_scene_update_vertices: null scene");
    const int rc = check_range("rt_scene_update_vertices", first, count, scene->ks.n_triangles, d_vertices);
    if (rc != RT_OK) return rc < 0 ? rc : RT_OK;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    SceneUpdate &u = scene->upd;
    {   /* the node ranges: kept on the host by rt_scene_create, uploaded with the first update (an allocation: not inside a capture) */
        std::lock_guard<std::mutex> lock(u.mutex);
        if (!u.uploaded) {
            if (stream_capturing(stream)) return fail(RT_ERR_UNSUPPORTED, "rt_scene_update_vertices: the first update of a scene allocates and cannot be captured");
            std::vector<RefitNode> small, large;
            for (const RefitNode &n : u.nodes) (n.hi - n.lo > RT_REFIT_WAVE_MAX ? large : small).push_back(n);
            const size_t total = small.size() + large.size();
            if (total != 0u) {
                hipError_t e = u.d_nodes.reserve(total * sizeof(RefitNode));
                if (e != hipSuccess) return fail_hip("hipMalloc(reinterpret_cast<void **>(&u.d_nodes), total * sizeof(RefitNode))", e);
                RefitNode *const d_nodes = u.d_nodes.get<RefitNode>();
                if (!small.empty()) e = hipMemcpy(d_nodes, small.data(), small.size() * sizeof(RefitNode), hipMemcpyHostToDevice);
                if (e == hipSuccess && !large.empty()) e = hipMemcpy(d_nodes + small.size(), large.data(), large.size() * sizeof(RefitNode), hipMemcpyHostToDevice);
                if (e != hipSuccess) {
                    (void)u.d_nodes.release();
                    return fail_hip("rt_scene_update_vertices: node ranges", e);
                }
            }
            u.n_small = (uint32_t)small.size();
            u.n_large = (uint32_t)large.size();
            u.uploaded = true;
        }
    }
    const UpdScene sc = upd_scene(scene);
    update_triangles<<<(count + 255u) / 256u, 256, 0, stream>>>(sc, d_vertices, first, count);
    if (scene->ks.n_materials <= RT_TRI_OBJ_MASK) { /* one past the range: triangle first + count compares with first + count - 1 */
        const uint32_t from = first > 1u ? first : 1u;
        const uint32_t to = (uint32_t)std::min<uint64_t>((uint64_t)first + count + 1u, scene->ks.n_triangles);
        if (to > from) update_plane_sharing<<<(to - from + 255u) / 256u, 256, 0, stream>>>(sc, from, to);
    }
    /* the whole scene: whether a node qualifies depends on every triangle below it */
    if (u.n_small) refit_nodes<64><<<u.n_small, 64, 0, stream>>>(sc, u.d_nodes.get<RefitNode>(), u.n_small);
    if (u.n_large) refit_nodes<256><<<u.n_large, 256, 0, stream>>>(sc, u.d_nodes.get<RefitNode>() + u.n_small, u.n_large);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int rt_scene_update_spheres(rt_scene *scene, uint32_t first, uint32_t count, const rt_sphere *d_spheres, void *hip_stream) {
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "rt_scene_update_spheres: null scene");
    const int rc = check_range("rt_scene_update_spheres", first, count, scene->ks.n_spheres, d_spheres);
    if (rc != RT_OK) return rc < 0 ? rc : RT_OK;
    update_spheres<<<(count + 255u) / 256u, 256, 0, static_cast<hipStream_t>(hip_stream)>>>(const_cast<rt::DevSphere *>(scene->ks.spheres), d_spheres, first, count);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int rt_scene_update_lights(rt_scene *scene, uint32_t first, uint32_t count, const rt_light *h_lights, void *hip_stream) {
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "rt_scene_update_lights: null scene");
    const int rc = check_range("rt_scene_update_lights", first, count, scene->ks.n_lights, h_lights);
    if (rc != RT_OK) return rc < 0 ? rc : RT_OK;
    for (uint32_t i = 0; i < count; ++i)
        if (h_lights[i].kind > RT_LIGHT_POINT) return fail(RT_ERR_INVALID_ARGUMENT, "rt_scene_update_lights: unknown light kind");
    std::vector<rt::LightAux> aux(count);
    for (uint32_t i = 0; i < count; ++i) aux[i] = light_aux_of(h_lights[i]);
    return stage_and_copy(scene, "rt_scene_update_lights", static_cast<hipStream_t>(hip_stream), const_cast<rt_light *>(scene->ks.lights) + first, h_lights,
                          count * sizeof(rt_light), const_cast<rt::LightAux *>(scene->ks.light_aux) + first, aux.data(), count * sizeof(rt::LightAux));
}

int rt_scene_update_materials(rt_scene *scene, uint32_t first, uint32_t count, const rt_material *h_materials, void *hip_stream) {
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "rt_scene_update_materials: null scene");
    const int rc = check_range("rt_scene_update_materials", first, count, scene->ks.n_materials, h_materials);
    if (rc != RT_OK) return rc < 0 ? rc : RT_OK;
    for (uint32_t i = 0; i < count; ++i)
        if (h_materials[i].diffuse_fn > RT_DIFFUSE_STRIPE_SUM || h_materials[i].normal_fn > RT_NORMAL_WAVE_U)
            return fail(RT_ERR_INVALID_ARGUMENT, "rt_scene_update_materials: unknown material function");
    return stage_and_copy(scene, "rt_scene_update_materials", static_cast<hipStream_t>(hip_stream), const_cast<rt_material *>(scene->ks.materials) + first,
                          h_materials, count * sizeof(rt_material), nullptr, nullptr, 0);
}

/* Diagnostics: the node records as they stand on the device, for tests of the refit (include/rt_amd.h). */
int rt_diag_scene_nodes(const rt_scene *scene, int which, uint32_t *h_words, size_t cap_words, size_t *n_words) {
    if (!scene || !n_words || (cap_words && !h_words)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_diag_scene_nodes: null argument");
    const size_t n_nodes = scene->ks.n_segments;
    const void *src;
    size_t bytes;
    switch (which) {
    case 0: src = scene->ks.segments; bytes = n_nodes * sizeof(rt::DevSegment); break;
    case 1: src = scene->ks.bfs_nodes; bytes = n_nodes * sizeof(rt::DevSegment); break;
    case 2: src = scene->ks.bfs_soa; bytes = (3u * n_nodes + 2u * (size_t)scene->ks.n_triangles) * sizeof(float4); break;
    default: return fail(RT_ERR_INVALID_ARGUMENT, "rt_diag_scene_nodes: which must be 0 (segments), 1 (bfs_nodes) or 2 (bfs_soa)");
    }
    *n_words = bytes / sizeof(uint32_t);
    if (cap_words < *n_words || bytes == 0u) return RT_OK; /* the size alone */
    const hipError_t e = hipMemcpy(h_words, src, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail_hip("rt_diag_scene_nodes: copy", e);
    return RT_OK;
}

} /* extern "C" */
