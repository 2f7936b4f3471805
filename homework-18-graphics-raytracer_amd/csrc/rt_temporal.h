/*
 * rt_temporal.h — the arithmetic of the temporal queries (include/rt_amd.h "temporal queries"), written once for the host (librt_host.so:
 * rt_temporal_motion_cpu / rt_temporal_accumulate_cpu) and the device (rt_temporal_query.hip).  Every function is a sequence of single
 * f32 operations in the order the header comment of the block gives; both libraries are built with -ffp-contract=off, the divides are
 * correctly rounded on either side, nothing comes from libm and nothing from a device intrinsic (the floor is two conversions and a
 * compare), so host and device agree bit for bit.  A call struct is the Op of its element loop — count() and operator()(i) — which the
 * device runs through rt_image_kernel.h's each_kernel and the host in a plain loop.
 * temporal_pixel is temporal_gather, then temporal_blend or temporal_reset: rt_rectify.h puts its clamp between the first two, so the
 * gather of rt_temporal_accumulate_bounded is this header's and is stated once.
 *
 * camera_basis is Camera::shoot's ray-independent part (main.rs:85-92), moved here from make_kernel_frame (rt_api.hip), which calls it:
 * the CPU form needs the same basis without HIP.  Its operation order is the contract of every primary ray and is not to change.
 */
#ifndef RT_TEMPORAL_H
#define RT_TEMPORAL_H

#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_query_args.h"
#include "rt_vec.h"

#if defined(__HIPCC__)
#define RT_TP_HD __host__ __device__ __forceinline__
#else
#define RT_TP_HD inline
#endif

namespace rt {

/* ---- the camera basis ---- */

struct CameraBasis {
    V3 origin; /* center + toward * near */
    V3 x, y;   /* tan(fovy / 2) * right, tan(fovy / 2) * up' */
    V3 toward; /* normalize(toward) */
};

inline CameraBasis camera_basis(const rt_camera *camera) {
    CameraBasis b;
    const V3 toward = normalize(v3p(camera->toward));
    const V3 right = normalize(cross(toward, v3p(camera->up)));
    const V3 up = normalize(cross(right, toward));
    const float th = rtdm::tanf(camera->fovy / 2.0f);
    b.x = th * right;
    b.y = th * up;
    b.origin = v3p(camera->center) + toward * camera->near;
    b.toward = toward;
    return b;
}

/* ---- rt_temporal_motion ---- */

/* what a projection into the previous frame needs: make_kernel_frame's fields of the previous camera over the full frame */
struct TemporalCamera {
    float origin[3], cam_x[3], cam_y[3], toward[3];
    float half_width, half_height, height_f;
};

inline TemporalCamera temporal_camera(const rt_camera *camera, const rt_frame *frame) {
    const CameraBasis b = camera_basis(camera);
    TemporalCamera c;
    c.origin[0] = b.origin.x, c.origin[1] = b.origin.y, c.origin[2] = b.origin.z;
    c.cam_x[0] = b.x.x, c.cam_x[1] = b.x.y, c.cam_x[2] = b.x.z;
    c.cam_y[0] = b.y.x, c.cam_y[1] = b.y.y, c.cam_y[2] = b.y.z;
    c.toward[0] = b.toward.x, c.toward[1] = b.toward.y, c.toward[2] = b.toward.z;
    c.half_height = (float)frame->height / 2.0f;
    c.half_width = (float)frame->width / 2.0f;
    c.height_f = (float)frame->height;
    return c;
}

struct TemporalMotion {
    TemporalCamera cam;
    const float *position;
    const uint32_t *valid; /* may be null */
    uint32_t position_stride, valid_stride;
    float *motion;
    uint64_t n;
    RT_TP_HD uint64_t count() const { return n; }
    RT_TP_HD void operator()(uint64_t i) const; /* temporal_project */
};

RT_TP_HD float temporal_dot(float a0, float a1, float a2, float b0, float b1, float b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

RT_TP_HD uint32_t temporal_bits(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, sizeof u);
    return u;
}

RT_TP_HD float temporal_float(uint32_t u) {
    float x;
    __builtin_memcpy(&x, &u, sizeof x);
    return x;
}

#define RT_TEMPORAL_NAN 0x7fc00000u

/* the seven steps of the projection for pixel i; the raw words of (px, py) */
RT_TP_HD void temporal_project(const TemporalMotion &m, uint64_t i) {
    uint32_t *out = reinterpret_cast<uint32_t *>(m.motion) + 2u * i;
    out[0] = RT_TEMPORAL_NAN, out[1] = RT_TEMPORAL_NAN;
    if (m.valid != nullptr && m.valid[i * m.valid_stride] == 0u) return;
    const float *p = m.position + i * m.position_stride;
    const TemporalCamera &c = m.cam;
    const float v0 = p[0] - c.origin[0], v1 = p[1] - c.origin[1], v2 = p[2] - c.origin[2];
    const float z = temporal_dot(v0, v1, v2, c.toward[0], c.toward[1], c.toward[2]);
    if (!(z > 0.0f)) return;
    const float tt = temporal_dot(c.cam_x[0], c.cam_x[1], c.cam_x[2], c.cam_x[0], c.cam_x[1], c.cam_x[2]);
    const float zt = z * tt;
    const float clip_x = temporal_dot(v0, v1, v2, c.cam_x[0], c.cam_x[1], c.cam_x[2]) / zt;
    const float clip_y = temporal_dot(v0, v1, v2, c.cam_y[0], c.cam_y[1], c.cam_y[2]) / zt;
    m.motion[2u * i] = clip_x * c.height_f + c.half_width;
    m.motion[2u * i + 1u] = c.half_height - clip_y * c.height_f;
}
RT_TP_HD void TemporalMotion::operator()(uint64_t i) const { temporal_project(*this, i); }

/* ---- rt_temporal_accumulate ---- */

struct TemporalCall {
    const float *color, *motion;
    rt_temporal_guides cur, prev;
    const rt_temporal_pixel *in;
    rt_temporal_pixel *out;
    float *variance; /* may be null */
    uint32_t rows, cols;
    float rows_f, cols_f;
    float normal_min, position_max2, alpha_min;
    uint32_t max_length;
    RT_TP_HD uint64_t count() const { return (uint64_t)rows * cols; }
    RT_TP_HD void operator()(uint64_t i) const; /* temporal_pixel */
};

/* the current pixel as the taps see it; a plane that is null leaves its fields +0 (they are not looked at) */
struct TemporalPix {
    float c0, c1, c2, lum;
    float n0, n1, n2, p0, p1, p2;
    uint32_t object;
};

/* one tap of the previous frame: its history record and guides, read behind its inside-the-image test */
struct TemporalTap {
    float b;
    float c0, c1, c2, m1, m2;
    uint32_t length, valid, object;
    float n0, n1, n2, p0, p1, p2;
};

struct TemporalAcc {
    float s0, s1, s2, m1, m2, bsum;
    uint32_t min_length;
};

RT_TP_HD float temporal_luminance(float c0, float c1, float c2) { return (0.2126f * c0 + 0.7152f * c1) + 0.0722f * c2; }

/* floorf for |x| < 2^63 without libm: the truncation, less one where it lies above x (floor(-0) is +0 here; only its value is used) */
RT_TP_HD float temporal_floor(float x) {
    const float t = (float)(long long)x;
    return t > x ? t - 1.0f : t;
}

/* step 1's float tests: may (px, py) be gathered at all */
RT_TP_HD bool temporal_inside(const TemporalCall &t, float px, float py) {
    return px >= -1.0f && px < t.cols_f && py >= -1.0f && py < t.rows_f; /* false for a NaN */
}

RT_TP_HD TemporalPix temporal_load(const TemporalCall &t, uint64_t i) {
    TemporalPix p = {t.color[3u * i], t.color[3u * i + 1u], t.color[3u * i + 2u], 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0u};
    p.lum = temporal_luminance(p.c0, p.c1, p.c2);
    if (t.cur.normal) {
        const float *n = t.cur.normal + i * t.cur.normal_stride;
        p.n0 = n[0], p.n1 = n[1], p.n2 = n[2];
    }
    if (t.cur.position) {
        const float *q = t.cur.position + i * t.cur.position_stride;
        p.p0 = q[0], p.p1 = q[1], p.p2 = q[2];
    }
    if (t.cur.object) p.object = t.cur.object[i * t.cur.object_stride];
    return p;
}

/* Tap (j, i) of the four around (px, py) = (fx + wx, fy + wy): its weight, and — where the weight is > 0 and the tap lies inside the
 * previous image — everything the tests and the sums need of it.  Returns whether the tap was read. */
RT_TP_HD bool temporal_read_tap(const TemporalCall &t, int64_t x, int64_t y, float b, TemporalTap &q) {
    q.b = b;
    if (!(b > 0.0f) || x < 0 || x >= (int64_t)t.cols || y < 0 || y >= (int64_t)t.rows) return false;
    const uint64_t qi = (uint64_t)y * t.cols + (uint64_t)x;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 *h = reinterpret_cast<const uint4 *>(t.in + qi); /* the record is 32 bytes and 16-byte aligned: two 128-bit loads */
    const uint4 lo = h[0], hi = h[1];
    q.c0 = temporal_float(lo.x), q.c1 = temporal_float(lo.y), q.c2 = temporal_float(lo.z), q.m1 = temporal_float(lo.w);
    q.m2 = temporal_float(hi.x), q.length = hi.y;
#else
    const rt_temporal_pixel &h = t.in[qi];
    q.c0 = h.color[0], q.c1 = h.color[1], q.c2 = h.color[2], q.m1 = h.moment1, q.m2 = h.moment2, q.length = h.length;
#endif
    q.valid = t.prev.valid ? t.prev.valid[qi * t.prev.valid_stride] : 1u;
    q.object = t.prev.object ? t.prev.object[qi * t.prev.object_stride] : 0u;
    q.n0 = q.n1 = q.n2 = q.p0 = q.p1 = q.p2 = 0.0f;
    if (t.prev.normal) {
        const float *n = t.prev.normal + qi * t.prev.normal_stride;
        q.n0 = n[0], q.n1 = n[1], q.n2 = n[2];
    }
    if (t.prev.position) {
        const float *s = t.prev.position + qi * t.prev.position_stride;
        q.p0 = s[0], q.p1 = s[1], q.p2 = s[2];
    }
    return true;
}

/* step 2 for a tap that was read: the consistency tests, then the sums (each product rounded before its add) */
RT_TP_HD void temporal_tap(const TemporalCall &t, TemporalAcc &a, const TemporalPix &p, const TemporalTap &q) {
    if (q.valid == 0u || q.length == 0u) return;
    if (t.prev.object && q.object != p.object) return;
    if (t.prev.normal && !(temporal_dot(p.n0, p.n1, p.n2, q.n0, q.n1, q.n2) >= t.normal_min)) return;
    if (t.prev.position) {
        const float d0 = p.p0 - q.p0, d1 = p.p1 - q.p1, d2 = p.p2 - q.p2;
        if (!(temporal_dot(d0, d1, d2, d0, d1, d2) <= t.position_max2)) return;
    }
    a.s0 = a.s0 + q.b * q.c0;
    a.s1 = a.s1 + q.b * q.c1;
    a.s2 = a.s2 + q.b * q.c2;
    a.m1 = a.m1 + q.b * q.m1;
    a.m2 = a.m2 + q.b * q.m2;
    a.bsum = a.bsum + q.b;
    a.min_length = q.length < a.min_length ? q.length : a.min_length;
}

/* a record is written as eight words (on the device two 128-bit stores), the variance beside it */
RT_TP_HD void temporal_write(const TemporalCall &t, uint64_t i, uint32_t w0, uint32_t w1, uint32_t w2, float m1, float m2, uint32_t length, float variance) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint4 *o = reinterpret_cast<uint4 *>(t.out + i);
    o[0] = make_uint4(w0, w1, w2, temporal_bits(m1));
    o[1] = make_uint4(temporal_bits(m2), length, 0u, 0u);
#else
    uint32_t *o = reinterpret_cast<uint32_t *>(t.out + i);
    o[0] = w0, o[1] = w1, o[2] = w2, o[3] = temporal_bits(m1), o[4] = temporal_bits(m2), o[5] = length, o[6] = 0u, o[7] = 0u;
#endif
    if (t.variance) t.variance[i] = variance;
}

/* what steps 1 to 3 leave of the previous frame: H = sum / bsum (five divides) and n = min(minimum length + 1, max_length) */
struct TemporalHist {
    float c0, c1, c2, m1, m2;
    uint32_t n;
};

/* THE gather, steps 1 to 3 and step 4's H and n, for output pixel i whose current values are p; false: the pixel resets */
RT_TP_HD bool temporal_gather(const TemporalCall &t, uint64_t i, const TemporalPix &p, TemporalHist &h) {
    const float px = t.motion[2u * i], py = t.motion[2u * i + 1u];
    TemporalAcc a = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0xffffffffu};
    const bool valid = t.cur.valid == nullptr || t.cur.valid[i * t.cur.valid_stride] != 0u;
    if (valid && temporal_inside(t, px, py)) {
        const float fx = temporal_floor(px), fy = temporal_floor(py);
        const float wx = px - fx, wy = py - fy;
        const float ux = 1.0f - wx, uy = 1.0f - wy;
        const int64_t x0 = (int64_t)fx, y0 = (int64_t)fy;
        TemporalTap q[4];
        bool read[4];
        /* every tap's loads are issued before the first test that depends on one */
        read[0] = temporal_read_tap(t, x0, y0, ux * uy, q[0]);
        read[1] = temporal_read_tap(t, x0 + 1, y0, wx * uy, q[1]);
        read[2] = temporal_read_tap(t, x0, y0 + 1, ux * wy, q[2]);
        read[3] = temporal_read_tap(t, x0 + 1, y0 + 1, wx * wy, q[3]);
        for (int k = 0; k < 4; ++k)
            if (read[k]) temporal_tap(t, a, p, q[k]);
    }
    if (!(a.bsum > 0.0f)) return false;
    h.n = a.min_length >= t.max_length ? t.max_length : a.min_length + 1u; /* min(min length + 1, max_length), no wrap */
    h.c0 = a.s0 / a.bsum, h.c1 = a.s1 / a.bsum, h.c2 = a.s2 / a.bsum, h.m1 = a.m1 / a.bsum, h.m2 = a.m2 / a.bsum;
    return true;
}

/* the rest of step 4 and step 5: the history h of length h.n blended with the current pixel and written */
RT_TP_HD void temporal_blend(const TemporalCall &t, uint64_t i, const TemporalPix &p, const TemporalHist &h) {
    const float inv = 1.0f / (float)h.n;
    const float alpha = inv > t.alpha_min ? inv : t.alpha_min;
    const float keep = 1.0f - alpha;
    const float lum2 = p.lum * p.lum;
    const float o0 = h.c0 * keep + p.c0 * alpha;
    const float o1 = h.c1 * keep + p.c1 * alpha;
    const float o2 = h.c2 * keep + p.c2 * alpha;
    const float m1 = h.m1 * keep + p.lum * alpha;
    const float m2 = h.m2 * keep + lum2 * alpha;
    const float v = m2 - m1 * m1;
    temporal_write(t, i, temporal_bits(o0), temporal_bits(o1), temporal_bits(o2), m1, m2, h.n, v > 0.0f ? v : 0.0f);
}

/* a reset: the colour's raw words, so a NaN keeps its payload */
RT_TP_HD void temporal_reset(const TemporalCall &t, uint64_t i, const TemporalPix &p) {
    const uint32_t *c = reinterpret_cast<const uint32_t *>(t.color) + 3u * i;
    temporal_write(t, i, c[0], c[1], c[2], p.lum, p.lum * p.lum, 1u, 0.0f);
}

/* steps 1 to 5 for output pixel i */
RT_TP_HD void temporal_pixel(const TemporalCall &t, uint64_t i) {
    const TemporalPix p = temporal_load(t, i);
    TemporalHist h;
    if (temporal_gather(t, i, p, h))
        temporal_blend(t, i, p, h);
    else
        temporal_reset(t, i, p);
}
RT_TP_HD void TemporalCall::operator()(uint64_t i) const { temporal_pixel(*this, i); }

/* ---- the arguments of the entry points (rt_query_args.h): the checks in the order include/rt_amd.h states ---- */

/* rt_temporal_motion, rt_temporal_motion_host and rt_temporal_motion_cpu */
struct TemporalMotionArgs {
    const float *position; uint32_t position_stride;
    const uint32_t *valid; uint32_t valid_stride;
    const rt_camera *camera; const rt_frame *frame; float *motion;

    const char *limits(QueryForm, int *status) const {
        *status = RT_ERR_INVALID_ARGUMENT;
        if (!camera) return "null prev_camera";
        if (!frame) return "null prev_frame";
        if (frame->x0 != 0u || frame->y0 != 0u || frame->x1 != frame->width || frame->y1 != frame->height || frame->y_step != 1u)
            return "prev_frame must be the full frame (x0 = y0 = 0, x1 = width, y1 = height, y_step = 1)";
        if ((uint64_t)frame->width * frame->height >= (1ull << 32)) {
            *status = RT_ERR_UNSUPPORTED;
            return "rows * cols: 2^32 pixels or more";
        }
        if (empty()) return nullptr;
        if (!position) return "null position pointer";
        if (!motion) return "null motion pointer";
        if (position_stride < 3u) return "position_stride must be at least 3 words";
        if (valid && valid_stride < 1u) return "valid_stride must be at least 1 word";
        return nullptr;
    }

    bool empty() const { return frame->width == 0u || frame->height == 0u; }
    size_t pixels() const { return (size_t)frame->width * frame->height; }

    template <class Stage>
    void arrays(Stage &s) {
        position = s.plane(position, pixels(), position_stride, 3u);
        valid = s.plane(valid, pixels(), valid_stride, 1u);
        motion = s.out(motion, pixels() * 2u * sizeof(float));
    }

    TemporalMotion call() const {
        TemporalMotion m;
        m.cam = temporal_camera(camera, frame);
        m.position = position, m.valid = valid, m.position_stride = position_stride, m.valid_stride = valid_stride, m.motion = motion;
        m.n = pixels();
        return m;
    }
};

inline const char *temporal_guide_strides(const rt_temporal_guides *g, bool current) {
    if (g->normal && g->normal_stride < 3u) return current ? "current: normal_stride must be at least 3 words" : "previous: normal_stride must be at least 3 words";
    if (g->position && g->position_stride < 3u)
        return current ? "current: position_stride must be at least 3 words" : "previous: position_stride must be at least 3 words";
    if (g->object && g->object_stride < 1u) return current ? "current: object_stride must be at least 1 word" : "previous: object_stride must be at least 1 word";
    if (g->valid && g->valid_stride < 1u) return current ? "current: valid_stride must be at least 1 word" : "previous: valid_stride must be at least 1 word";
    return nullptr;
}

/* rt_temporal_accumulate, rt_temporal_accumulate_host and rt_temporal_accumulate_cpu; rt_rectify.h's bounded accumulate begins with them */
struct TemporalAccumulateArgs {
    const float *color, *motion;
    const rt_temporal_guides *current, *previous;
    const rt_temporal_params *params;
    uint32_t rows, cols;
    const rt_temporal_pixel *history_in;
    rt_temporal_pixel *history_out;
    float *variance;

    const char *limits(QueryForm form, int *status) const {
        *status = RT_ERR_INVALID_ARGUMENT;
        if ((uint64_t)rows * cols >= (1ull << 32)) {
            *status = RT_ERR_UNSUPPORTED;
            return "rows * cols: 2^32 pixels or more";
        }
        if (empty()) return nullptr;
        if (!current) return "null current guides";
        if (!previous) return "null previous guides";
        if (!params) return "null params";
        if (!color) return "null color pointer";
        if (!motion) return "null motion pointer";
        if (!history_in) return "null history_in pointer";
        if (!history_out) return "null history_out pointer";
        if (const char *bad = temporal_guide_strides(current, true)) return bad;
        if (const char *bad = temporal_guide_strides(previous, false)) return bad;
        if (history_out == history_in) return "history_out must not be history_in";
        if (query_misaligned(form, history_in, history_out)) return "history_in and history_out must be 16-byte aligned";
        if (params->max_length < 1u) return "max_length must be at least 1";
        if (!(params->alpha_min >= 0.0f && params->alpha_min <= 1.0f)) return "alpha_min must lie in [0, 1]";
        if (!(params->position_max >= 0.0f)) return "position_max must be >= 0 (+inf: every distance passes)";
        if (params->flags != 0u) return "flags: unknown bits (none is defined)";
        if ((current->normal == nullptr) != (previous->normal == nullptr)) return "normal: a plane in one guide set and null in the other";
        if ((current->position == nullptr) != (previous->position == nullptr)) return "position: a plane in one guide set and null in the other";
        if ((current->object == nullptr) != (previous->object == nullptr)) return "object: a plane in one guide set and null in the other";
        return nullptr;
    }

    bool empty() const { return rows == 0u || cols == 0u; }

    template <class Stage>
    void arrays(Stage &s) {
        const size_t n = (size_t)rows * cols;
        color = s.in(color, n * 3u * sizeof(float));
        motion = s.in(motion, n * 2u * sizeof(float));
        current = s.guides(current, n), previous = s.guides(previous, n);
        history_in = s.in(history_in, n * sizeof(rt_temporal_pixel));
        history_out = s.out(history_out, n * sizeof(rt_temporal_pixel));
        variance = s.out(variance, n * sizeof(float));
    }

    TemporalCall call() const {
        TemporalCall t;
        t.color = color, t.motion = motion, t.cur = *current, t.prev = *previous, t.in = history_in, t.out = history_out, t.variance = variance;
        t.rows = rows, t.cols = cols, t.rows_f = (float)rows, t.cols_f = (float)cols;
        t.normal_min = params->normal_min, t.position_max2 = params->position_max * params->position_max, t.alpha_min = params->alpha_min;
        t.max_length = params->max_length;
        return t;
    }
};

} /* namespace rt */

#endif /* RT_TEMPORAL_H */
