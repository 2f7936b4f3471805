/*
 * rt_motion.h — the arithmetic of the motion queries (include/rt_amd.h "motion queries"), written once for the host (librt_host.so:
 * rt_previous_positions_cpu) and the device (rt_motion_query.hip).  A record is carried from the scene as it stands now back onto the
 * positions the scene kept: a sequence of single f32 operations in the order the header comment of the block gives, on rt_vec.h's dot
 * and cross; both libraries are built with -ffp-contract=off and the divides are correctly rounded on either side, so host and device
 * agree bit for bit.  The loops (CPU, kernel) differ only in how they walk the records.
 *
 * The signed areas and the three divides are the sequence the cast forms (rt_cast.h: the areas where a triangle is accepted, `v3(a0,
 * a1, a2) / T.area` in finish_hit).  There the two halves lie in different functions with the areas kept in between, and the render
 * path is not touched by this block, so the sequence is written out here rather than shared.
 *
 * Every record of the scene and of the kept positions is read in 16-byte pieces; a piece is four words whatever it holds.
 */
#ifndef RT_MOTION_H
#define RT_MOTION_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_device_scene.h"
#include "rt_vec.h"

#if defined(__HIPCC__)
#define RT_MO_HD __host__ __device__ __forceinline__
#else
#define RT_MO_HD inline
#endif

namespace rt {

#define RT_MOTION_NAN 0x7fc00000u

/* The kept positions, internal: triangle t's vertex k is piece 3 t + k as (x, y, z, 0); sphere s follows the triangles, piece
 * 3 n_triangles + s as (cx, cy, cz, radius). */
struct alignas(16) MotionPiece {
    float x, y, z, w;
};
static_assert(sizeof(MotionPiece) == 16, "a piece is 16 bytes");
#define RT_MOTION_TRI_PIECES 3u

inline size_t motion_kept_pieces(uint32_t n_triangles, uint32_t n_spheres) { return (size_t)RT_MOTION_TRI_PIECES * n_triangles + n_spheres; }

struct MotionScene {
    const DevTri *tris;       /* as they stand now */
    const DevSphere *spheres;
    const MotionPiece *kept;  /* as they stood at the keep */
    uint32_t n_triangles, n_spheres;
};

RT_MO_HD MotionPiece motion_load(const void *p) { /* one 16-byte load */
    MotionPiece r;
    __builtin_memcpy(&r, __builtin_assume_aligned(p, 16), sizeof r);
    return r;
}
RT_MO_HD V3 motion_xyz(const MotionPiece &p) { return v3(p.x, p.y, p.z); }
RT_MO_HD bool motion_zero(V3 m) { return m.x == 0.0f && m.y == 0.0f && m.z == 0.0f; }

/* a triangle hit at P (raw words): steps 1 to 4 of the header */
RT_MO_HD void motion_triangle(const MotionScene &s, uint32_t index, const uint32_t P[3], uint32_t was[3]) {
    const unsigned char *T = reinterpret_cast<const unsigned char *>(s.tris + index);
    const MotionPiece *K = s.kept + (size_t)RT_MOTION_TRI_PIECES * index;
    /* DevTri in pieces: n d | v0 obj | v1 area | v2 bq | e0 . | e1 . | e2 . */
    const MotionPiece tn = motion_load(T), t0 = motion_load(T + 16), t1 = motion_load(T + 32), t2 = motion_load(T + 48);
    const MotionPiece te0 = motion_load(T + 64), te1 = motion_load(T + 80), te2 = motion_load(T + 96);
    const MotionPiece k0 = motion_load(K), k1 = motion_load(K + 1), k2 = motion_load(K + 2);
    const V3 v0 = motion_xyz(t0), v1 = motion_xyz(t1), v2 = motion_xyz(t2);
    const V3 m0 = motion_xyz(k0) - v0, m1 = motion_xyz(k1) - v1, m2 = motion_xyz(k2) - v2;
    was[0] = P[0], was[1] = P[1], was[2] = P[2];
    if (motion_zero(m0) && motion_zero(m1) && motion_zero(m2)) return; /* unmoved: the hit position bit for bit */
    const V3 p = v3(rtdm::f32_from_bits(P[0]), rtdm::f32_from_bits(P[1]), rtdm::f32_from_bits(P[2]));
    const V3 n = motion_xyz(tn);
    const float area = t1.w;
    const float a0 = dot(cross(motion_xyz(te0), p - v1), n); /* main.rs:219-221 */
    const float a1 = dot(cross(motion_xyz(te1), p - v2), n);
    const float a2 = dot(cross(motion_xyz(te2), p - v0), n);
    const float b0 = a0 / area, b1 = a1 / area, b2 = a2 / area; /* main.rs:236 */
    was[0] = rtdm::f32_bits(p.x + ((m0.x * b0 + m1.x * b1) + m2.x * b2));
    was[1] = rtdm::f32_bits(p.y + ((m0.y * b0 + m1.y * b1) + m2.y * b2));
    was[2] = rtdm::f32_bits(p.z + ((m0.z * b0 + m1.z * b1) + m2.z * b2));
}

/* a sphere hit at P: the point keeps its direction from the centre (rt_sphere has no orientation), scaled by the radii */
RT_MO_HD void motion_sphere(const MotionScene &s, uint32_t index, const uint32_t P[3], uint32_t was[3]) {
    const MotionPiece now = motion_load(s.spheres + index); /* c radius | r2 obj q_miss . */
    const MotionPiece kept = motion_load(s.kept + (size_t)RT_MOTION_TRI_PIECES * s.n_triangles + index);
    was[0] = P[0], was[1] = P[1], was[2] = P[2];
    if (kept.x == now.x && kept.y == now.y && kept.z == now.z && kept.w == now.w) return;
    const V3 p = v3(rtdm::f32_from_bits(P[0]), rtdm::f32_from_bits(P[1]), rtdm::f32_from_bits(P[2]));
    const float scale = kept.w / now.w;
    const V3 w = motion_xyz(kept) + (p - motion_xyz(now)) * scale;
    was[0] = rtdm::f32_bits(w.x), was[1] = rtdm::f32_bits(w.y), was[2] = rtdm::f32_bits(w.z);
}

/* record i: only kind, index and position of the hit are read, as dwords; three words are written */
RT_MO_HD void motion_record(const MotionScene &s, const rt_hit *hits, float *was, uint32_t was_stride, uint64_t i) {
    const uint32_t *h = reinterpret_cast<const uint32_t *>(hits + i);
    const uint32_t kind = h[0], index = h[1];
    uint32_t out[3] = {RT_MOTION_NAN, RT_MOTION_NAN, RT_MOTION_NAN};
    if (kind == 1u && index < s.n_triangles) {
        const uint32_t P[3] = {h[3], h[4], h[5]};
        motion_triangle(s, index, P, out);
    } else if (kind == 0u && index < s.n_spheres) {
        const uint32_t P[3] = {h[3], h[4], h[5]};
        motion_sphere(s, index, P, out);
    }
    uint32_t *o = reinterpret_cast<uint32_t *>(was) + i * was_stride;
    o[0] = out[0], o[1] = out[1], o[2] = out[2];
}

/* rt_previous_positions as an element loop over the n records */
struct MotionRecords {
    MotionScene s;
    const rt_hit *hits;
    uint64_t n;
    float *was;
    uint32_t was_stride;
    RT_MO_HD uint64_t count() const { return n; }
    RT_MO_HD void operator()(uint64_t i) const { motion_record(s, hits, was, was_stride, i); }
};

/* ---- THE argument checks of rt_previous_positions, in the order include/rt_amd.h states; null: go on (*done: nothing to launch),
 * *status says how a refusal is reported.  kept: the scene holds kept positions (the CPU form: the arrays of them it needs). ---- */
inline const char *motion_limits(uint64_t n, const void *scene, bool kept, const char *not_kept, const void *hits, const void *was, uint32_t was_stride,
                                 int *status, bool *done) {
    *status = RT_ERR_INVALID_ARGUMENT;
    *done = true;
    if (n >= (1ull << 32)) {
        *status = RT_ERR_UNSUPPORTED;
        return "2^32 records or more (checked first; query them in several calls)";
    }
    if (!scene) return "null scene";
    if (!kept) return not_kept;
    if (n == 0u) return nullptr;
    if (!hits || !was) return "null hit or was pointer";
    if (was_stride < 3u) return "was_stride must be at least 3 words";
    *done = false;
    return nullptr;
}
#define RT_MOTION_NOT_KEPT "the scene holds no kept positions: call rt_scene_keep_positions first"

} /* namespace rt */

#endif /* RT_MOTION_H */
