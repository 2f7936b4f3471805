/*
 * rt_mesh_order.hip — the order of a mesh (include/rt_amd.h "mesh ordering"): a Z-order key per triangle from its centroid's cell in a
 * 1024^3 grid over the caller's box, and the permutation that groups the triangles by object and, inside an object, by that key.
 * rt_scene_create cuts each run of one object's triangles into leaves of 16 consecutive triangles: after this permutation a leaf is a
 * patch of the surface instead of a sample of the whole object, so its bounding sphere and its plane directions can reject rays.
 *
 *   rt::triangle_keys_kernel   one triangle per lane: ten dwords of the 25-dword record are read (the object word and the three
 *                              positions; a record is 100 bytes and only 4-byte aligned), the key and — if wanted — the object word
 *                              are written
 *
 * The permutation itself is two stable sorts of rt_order_query.hip (rt_sort_records: by the 30 key bits, then by the object word) and
 * its gather (rt_gather_records), called through their entry points: nothing of the sort is repeated here.  The key's arithmetic is
 * single f32 operations in the documented order (-ffp-contract=off, hipcc's correctly rounded f32 divide); every store is a vector store.
 */
#include "rt_api_internal.h"

namespace rt {

#define RT_MESH_THREADS 256u
#define RT_MESH_TRIANGLE_WORDS 25u /* sizeof(rt_triangle) / 4: the object word, then three vertices of eight floats, the position first */
#define RT_MESH_VERTEX_WORDS 8u

struct MeshBox {
    float lo[3], scale[3];
};

/* the cell of a scaled coordinate: NaN and negatives 0, 1023 and beyond 1023, truncation between */
__device__ __forceinline__ uint32_t mesh_cell(float t) {
    if (!(t >= 0.0f)) return 0u;
    if (t >= 1023.0f) return 1023u;
    return (uint32_t)t;
}

/* bit k of a 10-bit value to bit 3k */
__device__ __forceinline__ uint32_t mesh_spread3(uint32_t v) {
    uint32_t r = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 10u; ++k) r |= ((v >> k) & 1u) << (3u * k);
    return r;
}

__global__ __launch_bounds__(RT_MESH_THREADS) void triangle_keys_kernel(const rt_triangle *__restrict__ triangles, const uint64_t n, const MeshBox box,
                                                                        uint32_t *__restrict__ keys, uint32_t *__restrict__ objects) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_MESH_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t *const w = reinterpret_cast<const uint32_t *>(triangles) + i * RT_MESH_TRIANGLE_WORDS;
    const float *const p0 = reinterpret_cast<const float *>(w + 1u), *const p1 = p0 + RT_MESH_VERTEX_WORDS, *const p2 = p1 + RT_MESH_VERTEX_WORDS;
    uint32_t c[3];
#pragma unroll
    for (uint32_t a = 0; a < 3u; ++a) {
        const float centroid = ((p0[a] + p1[a]) + p2[a]) / 3.0f;
        c[a] = mesh_cell((centroid - box.lo[a]) * box.scale[a]);
    }
    keys[i] = mesh_spread3(c[0]) | (mesh_spread3(c[1]) << 1) | (mesh_spread3(c[2]) << 2);
    if (objects != nullptr) objects[i] = w[0];
}

} /* namespace rt */

/* ---- the C entry points (include/rt_amd.h "mesh ordering") ---- */

static const CountLimit TRIANGLES_2_32 = {32u, "triangles", nullptr};

/* the bits of the second sort: those of the largest object index, one at least */
static inline uint32_t mesh_object_bits(uint32_t n_objects) {
    uint32_t bits = 1u;
    while (bits < 32u && ((uint64_t)1 << bits) < (uint64_t)n_objects) ++bits;
    return bits;
}

extern "C" {

int rt_triangle_keys(const rt_triangle *d_triangles, size_t n, const float box_lo[3], const float box_hi[3], uint32_t *d_keys, uint32_t *d_objects,
                     void *hip_stream) {
    bool done;
    const int rc = query_args("rt_triangle_keys", n, TRIANGLES_2_32, false, nullptr, d_triangles && box_lo && box_hi && d_keys, "triangle, box or key", &done);
    if (rc != RT_OK || done) return rc;
    rt::MeshBox box;
    for (int a = 0; a < 3; ++a) {
        box.lo[a] = box_lo[a];
        box.scale[a] = box_hi[a] > box_lo[a] ? 1024.0f / (box_hi[a] - box_lo[a]) : 0.0f; /* a NaN bound compares false: 0 */
    }
    hipLaunchKernelGGL(rt::triangle_keys_kernel, grid_of(n, RT_MESH_THREADS), dim3(RT_MESH_THREADS), 0, static_cast<hipStream_t>(hip_stream), d_triangles, (uint64_t)n, box,
                       d_keys, d_objects);
    return launched("rt_triangle_keys");
}

size_t rt_order_triangles_temp_bytes(size_t n) {
    if (n == 0 || (uint64_t)n >= (1ull << 32)) return 0;
    return 2u * n * sizeof(uint32_t) + rt_sort_temp_bytes(n); /* keys, objects, the sort's workspace */
}

int rt_order_triangles(const rt_triangle *d_triangles, size_t n, const float box_lo[3], const float box_hi[3], uint32_t n_objects, uint32_t *d_perm,
                       rt_triangle *d_ordered_or_null, void *d_temp, size_t temp_bytes, void *hip_stream) {
    bool done;
    int rc = query_args("rt_order_triangles", n, TRIANGLES_2_32, false, nullptr, d_triangles && box_lo && box_hi && d_perm && d_temp,
                        "triangle, box, permutation or workspace", &done);
    if (rc != RT_OK || done) return rc;
    if (temp_bytes < rt_order_triangles_temp_bytes(n))
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_order_triangles: the workspace is smaller than rt_order_triangles_temp_bytes(n)");
    uint32_t *const keys = static_cast<uint32_t *>(d_temp), *const objects = keys + n;
    void *const sort_temp = objects + n;
    const size_t sort_bytes = rt_sort_temp_bytes(n);
    rc = rt_triangle_keys(d_triangles, n, box_lo, box_hi, keys, objects, hip_stream);
    /* Z-order first, then — stable — the object: equal (object, key) pairs keep their input order.  The second sort's list is the
     * first one's output, in place (rt_sort_records reads its list before it writes one) */
    if (rc == RT_OK) rc = rt_sort_records(keys, n, 0u, 30u, nullptr, nullptr, d_perm, sort_temp, sort_bytes, hip_stream);
    if (rc == RT_OK) rc = rt_sort_records(objects, n, 0u, mesh_object_bits(n_objects), d_perm, nullptr, d_perm, sort_temp, sort_bytes, hip_stream);
    if (rc == RT_OK && d_ordered_or_null)
        rc = rt_gather_records(d_triangles, sizeof(rt_triangle), n, d_perm, nullptr, n, d_ordered_or_null, hip_stream);
    return rc;
}

int rt_order_triangles_host(const rt_triangle *h_triangles, size_t n, const float lo[3], const float hi[3], uint32_t n_objects, uint32_t *h_perm,
                            rt_triangle *h_ordered_or_null) {
    bool done;
    int rc = query_args("rt_order_triangles_host", n, TRIANGLES_2_32, false, nullptr, h_triangles && lo && hi && h_perm, "triangle, box or permutation", &done);
    if (rc != RT_OK || done) return rc;
    const size_t tri_bytes = n * sizeof(rt_triangle), temp_bytes = rt_order_triangles_temp_bytes(n);
    HostRoundTrip t("rt_order_triangles_host"); /* no device: the status, nothing written */
    const rt_triangle *d_triangles = t.in(h_triangles, tri_bytes);
    uint32_t *d_perm = t.out(h_perm, n * sizeof(uint32_t));
    void *d_temp = t.scratch(temp_bytes);
    rt_triangle *d_ordered = t.out(h_ordered_or_null, tri_bytes); /* optional */
    if (!t.ok()) return t.failed();
    rc = rt_order_triangles(d_triangles, n, lo, hi, n_objects, d_perm, d_ordered, d_temp, temp_bytes, nullptr);
    return rc != RT_OK ? rc : t.finish();
}

} /* extern "C" */
