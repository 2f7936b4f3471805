/*
 * rt_host.cpp — host side of the render path (see include/rt_host.h).
 *
 * Scene construction, OBJ import, tone normalisation, sRGB encode and PNG
 * output stay on the CPU, as they do in the reference (src/main.rs:748-1083).
 * All f32 arithmetic follows the reference's operation order (rt_vec.h).
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../../include/rt_host.h"
#include "../rt_vec.h"
#include "../rt_luma.h"
#include "../rt_film.h"
#include "../rt_denoise.h"
#include "../rt_temporal.h"
#include "../rt_svgf.h"
#include "../rt_rectify.h"
#include "../rt_motion.h"
#include "../rt_adaptive.h"
#include "../rt_upsample.h"
#include "../rt_bloom.h"
#include "../rt_area_light.h"
#include "../rt_hemisphere.h"
#include "../rt_environment.h"
#include "../rt_lobe.h"
#include "../rt_path.h"
#include "../rt_transmit.h"
#include "../rt_connect.h"
#include "../rt_light_connect.h"
#include "../rt_texture.h"

using rt::V3;

struct rt_world {
    std::vector<rt_material> objects; /* Object { material } — primitives.rs:8-10 */
    std::vector<rt_triangle> triangles;
    std::vector<rt_sphere> spheres;
    std::vector<rt_light> lights;
};

static thread_local std::string g_host_error;
static int fail(int code, const std::string &msg) {
    g_host_error = msg;
    return code;
}

/* The CPU form of an element loop: the Op of a query's shared header (count() and operator()(i), the loop body written once for both
 * libraries), every element in turn; the device runs the same Op through rt_image_kernel.h's each_kernel. */
template <class Op>
static void each(const Op &op) {
    for (uint64_t i = 0; i < op.count(); ++i) op(i);
}

/* The _cpu form of an image-side query, written once: `a` is the query's argument struct (rt_query_args.h) — its limits under the entry
 * point's name, nothing to do for an empty image, then run(a), the query's loop. */
template <class Args, class Run>
static int cpu_query(const char *who, const Args &a, Run run) {
    int status = RT_ERR_INVALID_ARGUMENT;
    if (const char *bad = a.limits(rt::QUERY_CPU, &status)) return fail(status, std::string(who) + ": " + bad);
    if (!a.empty()) run(a);
    return RT_OK;
}
/* the loop of a query whose call() is an Op */
static const auto each_call = [](const auto &a) { each(a.call()); };

/* The walk of a listed form of the path loop (the path, transmission, connection and light-connection queries): body(j) for every slot
 * the list names, in the list's order; an index beyond the slots names nothing, as in rt_cast_rays_indexed. */
template <class Body>
static void each_listed(const uint32_t *index, const uint32_t *count, size_t m, Body body) {
    const uint32_t listed = rt::path_listed(index, count, (uint32_t)m);
    for (uint32_t e = 0; e < listed; ++e) {
        const uint32_t j = index ? index[e] : e;
        if (j < m) body(j);
    }
}

extern "C" {

const char *rt_host_last_error(void) { return g_host_error.c_str(); }

rt_world *rt_world_new(void) { return new (std::nothrow) rt_world(); }
void rt_world_free(rt_world *world) { delete world; }

int rt_world_push_object(rt_world *world, const rt_material *material) {
    if (!world || !material) return fail(RT_ERR_INVALID_ARGUMENT, "rt_world_push_object: null argument");
    world->objects.push_back(*material);
    return (int)world->objects.size() - 1;
}

int rt_world_push_triangle(rt_world *world, uint32_t object_index, const rt_vertex vertices[3]) {
    if (!world || !vertices) return fail(RT_ERR_INVALID_ARGUMENT, "rt_world_push_triangle: null argument");
    if (object_index >= world->objects.size()) return fail(RT_ERR_INVALID_ARGUMENT, "rt_world_push_triangle: object index out of range");
    rt_triangle t;
    t.object_index = object_index;
    memcpy(t.vertices, vertices, sizeof t.vertices);
    world->triangles.push_back(t);
    return RT_OK;
}

int rt_world_push_sphere(rt_world *world, uint32_t object_index, const float center[3], float radius) {
    if (!world || !center) return fail(RT_ERR_INVALID_ARGUMENT, "rt_world_push_sphere: null argument");
    if (object_index >= world->objects.size()) return fail(RT_ERR_INVALID_ARGUMENT, "rt_world_push_sphere: object index out of range");
    rt_sphere s;
    s.object_index = object_index;
    memcpy(s.center, center, sizeof s.center);
    s.radius = radius;
    world->spheres.push_back(s);
    return RT_OK;
}

int rt_world_push_light(rt_world *world, const rt_light *light) {
    if (!world || !light) return fail(RT_ERR_INVALID_ARGUMENT, "rt_world_push_light: null argument");
    if (light->kind > RT_LIGHT_POINT) return fail(RT_ERR_INVALID_ARGUMENT, "rt_world_push_light: unknown light kind");
    world->lights.push_back(*light);
    return RT_OK;
}

/* triangle(): src/main.rs:730-739 */
int rt_world_push_flat_triangle(rt_world *world, uint32_t object_index, const float positions[9], const float uvs[6]) {
    if (!world || !positions || !uvs) return fail(RT_ERR_INVALID_ARGUMENT, "rt_world_push_flat_triangle: null argument");
    V3 p0 = rt::v3p(positions), p1 = rt::v3p(positions + 3), p2 = rt::v3p(positions + 6);
    V3 a = p1 - p0;
    V3 b = p2 - p1;
    V3 n = rt::normalize(rt::cross(a, b));
    rt_vertex v[3];
    for (int i = 0; i < 3; ++i) {
        memcpy(v[i].position, positions + 3 * i, 3 * sizeof(float));
        v[i].normal[0] = n.x; v[i].normal[1] = n.y; v[i].normal[2] = n.z;
        v[i].uv[0] = uvs[2 * i]; v[i].uv[1] = uvs[2 * i + 1];
    }
    return rt_world_push_triangle(world, object_index, v);
}

/* square(): src/main.rs:741-746 */
int rt_world_push_square(rt_world *world, uint32_t object_index, const float positions[12], const float uvs[8]) {
    if (!world || !positions || !uvs) return fail(RT_ERR_INVALID_ARGUMENT, "rt_world_push_square: null argument");
    static const int corner[2][3] = {{0, 1, 2}, {0, 2, 3}};
    for (int t = 0; t < 2; ++t) {
        float p[9], uv[6];
        for (int i = 0; i < 3; ++i) {
            memcpy(p + 3 * i, positions + 3 * corner[t][i], 3 * sizeof(float));
            memcpy(uv + 2 * i, uvs + 2 * corner[t][i], 2 * sizeof(float));
        }
        int rc = rt_world_push_flat_triangle(world, object_index, p, uv);
        if (rc != RT_OK) return rc;
    }
    return RT_OK;
}

/* load_obj: src/main.rs:778-807 (tobj: first model, positions + triangle indices only) */
int rt_world_load_obj(rt_world *world, uint32_t object_index, const char *path, float divisor, const float offset[3]) {
    if (!world || !path || !offset) return fail(RT_ERR_INVALID_ARGUMENT, "rt_world_load_obj: null argument");
    FILE *f = fopen(path, "r");
    if (!f) return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_world_load_obj: cannot open ") + path + ": " + strerror(errno));
    std::vector<float> positions;
    std::vector<uint32_t> faces;
    char line[512];
    int models_seen = 0;
    bool bad = false;
    while (fgets(line, sizeof line, f)) {
        char *s = line;
        while (*s == ' ' || *s == '\t') ++s;
        if ((s[0] == 'o' || s[0] == 'g') && (s[1] == ' ' || s[1] == '\t')) {
            /* tobj starts a new model at each o/g record once faces exist; only models[0] is used */
            if (!faces.empty()) { models_seen = 2; break; }
            models_seen = 1;
        } else if (s[0] == 'v' && (s[1] == ' ' || s[1] == '\t')) {
            char *e = s + 1;
            for (int i = 0; i < 3; ++i) {
                char *next = nullptr;
                float v = strtof(e, &next); /* correctly rounded, like Rust's str::parse::<f32> */
                if (next == e) { bad = true; break; }
                positions.push_back(v);
                e = next;
            }
        } else if (s[0] == 'f' && (s[1] == ' ' || s[1] == '\t')) {
            char *e = s + 1;
            uint32_t idx[3];
            int n = 0;
            while (n < 3) {
                char *next = nullptr;
                long v = strtol(e, &next, 10);
                if (next == e) break;
                /* skip /vt/vn suffixes if present */
                while (*next && *next != ' ' && *next != '\t' && *next != '\n' && *next != '\r') ++next;
                long count = (long)(positions.size() / 3);
                long zero_based = v > 0 ? v - 1 : count + v; /* OBJ allows negative (relative) indices */
                if (zero_based < 0 || zero_based >= count) { bad = true; break; }
                idx[n++] = (uint32_t)zero_based;
                e = next;
            }
            if (n != 3) bad = true;
            if (bad) break;
            faces.insert(faces.end(), idx, idx + 3);
        }
        if (bad) break;
    }
    fclose(f);
    (void)models_seen;
    if (bad) return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_world_load_obj: malformed record in ") + path);
    int pushed = 0;
    V3 off = rt::v3p(offset);
    for (size_t t = 0; t + 2 < faces.size(); t += 3) {
        float p[9];
        static const float uv[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int i = 0; i < 3; ++i) {
            V3 v = rt::v3p(&positions[3 * faces[t + i]]);
            V3 q = v / divisor + off; /* p.position / 3.0 + Vector3::new(0.7, 1.0, -0.5) */
            p[3 * i] = q.x; p[3 * i + 1] = q.y; p[3 * i + 2] = q.z;
        }
        int rc = rt_world_push_flat_triangle(world, object_index, p, uv);
        if (rc != RT_OK) return rc;
        ++pushed;
    }
    return pushed;
}

/* ---- the literal scene of main(): src/main.rs:810-1075 ------------------- */

static rt_material color_material(float dr, float dg, float db, float shiness, float sr, float sg, float sb,
                                  float smoothness, float refraction_index, float opaque_decay, float transparency) {
    rt_material m;
    memset(&m, 0, sizeof m);
    m.diffuse_fn = RT_DIFFUSE_CONST;
    m.normal_fn = RT_NORMAL_CONST;
    m.normal[0] = 0.0f; m.normal[1] = 0.0f; m.normal[2] = 1.0f;
    m.diffuse_color[0] = dr; m.diffuse_color[1] = dg; m.diffuse_color[2] = db;
    m.shiness = shiness;
    m.specular_color[0] = sr; m.specular_color[1] = sg; m.specular_color[2] = sb;
    m.smoothness = smoothness;
    m.transparency = transparency;
    m.refraction_index = refraction_index;
    m.opaque_decay = opaque_decay;
    return m;
}

/* an axis-aligned box of 6 squares given as (corner order, uv order) rows; the
 * two glass slabs of main.rs:892-927 and 942-977 share this vertex pattern */
struct SquareRow {
    float p[12];
    float uv[8];
};

static int push_rows(rt_world *w, uint32_t obj, const SquareRow *rows, int n) {
    for (int i = 0; i < n; ++i) {
        int rc = rt_world_push_square(w, obj, rows[i].p, rows[i].uv);
        if (rc != RT_OK) return rc;
    }
    return RT_OK;
}

/* slab spanning x in [-hx, hx], y in [1.0, 1.5], z in [z0, z1] (z0 < z1), in
 * the face and vertex order of the reference */
static int push_glass_slab(rt_world *w, uint32_t obj, float hx, float z0, float z1) {
    const float ylo = 1.0f, yhi = 1.5f;
    const SquareRow rows[6] = {
        /* +z face */
        {{hx, yhi, z1, -hx, yhi, z1, -hx, ylo, z1, hx, ylo, z1}, {0, 0, 0, 1, 1, 0, 0, 1}},
        /* -z face */
        {{hx, ylo, z0, -hx, ylo, z0, -hx, yhi, z0, hx, yhi, z0}, {0, 1, 1, 0, 0, 1, 0, 0}},
        /* +y face */
        {{hx, yhi, z0, -hx, yhi, z0, -hx, yhi, z1, hx, yhi, z1}, {0, 1, 1, 0, 0, 1, 0, 0}},
        /* fourth and fifth faces differ between the two slabs; filled in by the caller */
        {{0}, {0}},
        {{0}, {0}},
        /* +x face */
        {{hx, ylo, z0, hx, yhi, z0, hx, yhi, z1, hx, ylo, z1}, {0, 1, 1, 0, 0, 1, 0, 0}},
    };
    SquareRow r[6];
    memcpy(r, rows, sizeof r);
    const SquareRow bottom = {{hx, ylo, z1, -hx, ylo, z1, -hx, ylo, z0, hx, ylo, z0}, {0, 1, 1, 0, 0, 1, 0, 0}};
    const SquareRow minus_x = {{-hx, yhi, z0, -hx, ylo, z0, -hx, ylo, z1, -hx, yhi, z1}, {0, 1, 1, 0, 0, 1, 0, 0}};
    if (hx == 0.5f) { /* first slab: ..., -y face (main.rs:910-915), -x face (916-921), +x */
        r[3] = bottom;
        r[4] = minus_x;
    } else {          /* second slab: ..., -x face (main.rs:960-965), -y face (966-971), +x */
        r[3] = minus_x;
        r[4] = bottom;
    }
    return push_rows(w, obj, r, 6);
}

int rt_world_build_reference_scene(rt_world *world, const char *obj_path) {
    if (!world || !obj_path) return fail(RT_ERR_INVALID_ARGUMENT, "rt_world_build_reference_scene: null argument");
    int rc;
    /* object 0: the imported dodecahedron (main.rs:812-825) */
    rt_material m0 = color_material(1.0f, 1.0f, 1.0f, 0.1f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 0.0f, 0.0f);
    int o0 = rt_world_push_object(world, &m0);
    const float obj_offset[3] = {0.7f, 1.0f, -0.5f};
    rc = rt_world_load_obj(world, (uint32_t)o0, obj_path, 3.0f, obj_offset);
    if (rc < 0) return rc;

    /* object 1: the floor (main.rs:826-844) */
    rt_material m1 = color_material(1.0f, 0.8f, 0.6f, 0.5f, 1.0f, 1.0f, 1.0f, 0.01f, 1.0f, 0.0f, 0.0f);
    int o1 = rt_world_push_object(world, &m1);
    const SquareRow floor_sq = {{-2, 0, -2, -2, 0, 2, 2, 0, 2, 2, 0, -2}, {0, 0, 0, 1, 1, 0, 0, 1}};
    if ((rc = push_rows(world, (uint32_t)o1, &floor_sq, 1)) != RT_OK) return rc;

    /* object 2: the striped, wavy wall — GenerativeMaterial (main.rs:845-877) */
    rt_material m2 = color_material(0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 1.0f, 0.00001f, 1.0f, 0.0f, 0.0f);
    m2.diffuse_fn = RT_DIFFUSE_STRIPE_V;
    m2.normal_fn = RT_NORMAL_WAVE_U;
    m2.tex_color_a[0] = 1.0f; m2.tex_color_a[1] = 1.0f; m2.tex_color_a[2] = 1.0f;
    m2.tex_color_b[0] = 0.5f; m2.tex_color_b[1] = 0.5f; m2.tex_color_b[2] = 1.0f;
    m2.tex_frequency = 20.0f;
    m2.normal_frequency = 10.0f;
    int o2 = rt_world_push_object(world, &m2);
    const SquareRow wall_sq = {{-2, 2, -2, -2, 2, 2, -2, -2, 2, -2, -2, -2}, {0, 0, 0, 1, 1, 0, 1, 1}};
    if ((rc = push_rows(world, (uint32_t)o2, &wall_sq, 1)) != RT_OK) return rc;

    /* objects 3 and 4: two glass slabs (main.rs:879-977) */
    rt_material glass = color_material(1.0f, 0.8f, 0.6f, 1.0f, 1.0f, 1.0f, 1.0f, 0.00001f, 1.6f, 0.1f, 1.0f);
    int o3 = rt_world_push_object(world, &glass);
    if ((rc = push_glass_slab(world, (uint32_t)o3, 0.5f, 0.6f, 0.7f)) != RT_OK) return rc;
    int o4 = rt_world_push_object(world, &glass);
    if ((rc = push_glass_slab(world, (uint32_t)o4, 0.3f, 0.71f, 0.81f)) != RT_OK) return rc;

    /* object 5: red sphere (main.rs:979-996); yellow = (1,1,0) consts.rs:17 */
    rt_material m5 = color_material(1.0f, 0.2f, 0.2f, 0.2f, 1.0f, 1.0f, 0.0f, 0.2f, 1.0f, 0.0f, 0.0f);
    int o5 = rt_world_push_object(world, &m5);
    const float c5[3] = {-0.5f, 0.5f, 0.5f / rtdm::f_sqrt(3.0f)};
    if ((rc = rt_world_push_sphere(world, (uint32_t)o5, c5, 0.5f)) != RT_OK) return rc;

    /* object 6: clear sphere (main.rs:998-1014) */
    rt_material m6 = color_material(1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 0.001f, 1.12f, 0.3f, 0.96f);
    int o6 = rt_world_push_object(world, &m6);
    const float c6[3] = {0.5f, 0.5f, 0.5f / rtdm::f_sqrt(3.0f)};
    if ((rc = rt_world_push_sphere(world, (uint32_t)o6, c6, 0.5f)) != RT_OK) return rc;

    /* object 7: checkered sphere — GenerativeMaterial (main.rs:1016-1038); blue = (0,0,1) consts.rs:15 */
    rt_material m7 = color_material(0.0f, 0.0f, 0.0f, 0.3f, 0.0f, 0.0f, 1.0f, 0.7f, 1.0f, 0.0f, 0.0f);
    m7.diffuse_fn = RT_DIFFUSE_STRIPE_SUM;
    m7.normal_fn = RT_NORMAL_CONST;
    m7.tex_color_a[0] = 1.0f; m7.tex_color_a[1] = 0.1f; m7.tex_color_a[2] = 0.1f;
    m7.tex_color_b[0] = 0.1f; m7.tex_color_b[1] = 0.1f; m7.tex_color_b[2] = 1.0f;
    m7.tex_frequency = 10.0f;
    int o7 = rt_world_push_object(world, &m7);
    const float c7[3] = {0.0f, 0.5f, -1.0f / rtdm::f_sqrt(3.0f)};
    if ((rc = rt_world_push_sphere(world, (uint32_t)o7, c7, 0.5f)) != RT_OK) return rc;

    /* object 8: green sphere on top (main.rs:1040-1056) */
    rt_material m8 = color_material(0.5f, 1.0f, 0.2f, 0.5f, 1.0f, 1.0f, 1.0f, 0.01f, 1.0f, 0.0f, 0.0f);
    int o8 = rt_world_push_object(world, &m8);
    const float c8[3] = {0.0f, 0.5f + rtdm::f_sqrt(2.0f / 3.0f), 0.0f};
    if ((rc = rt_world_push_sphere(world, (uint32_t)o8, c8, 0.5f)) != RT_OK) return rc;

    /* lights (main.rs:1058-1075) */
    rt_light l;
    memset(&l, 0, sizeof l);
    l.kind = RT_LIGHT_DIRECTIONAL;
    l.has_origin = 0;
    V3 d0 = rt::normalize(rt::v3(-1.0f, -1.0f, 0.0f));
    l.direction[0] = d0.x; l.direction[1] = d0.y; l.direction[2] = d0.z;
    l.color[0] = 1.0f; l.color[1] = 0.98f; l.color[2] = 0.95f;
    if ((rc = rt_world_push_light(world, &l)) != RT_OK) return rc;

    memset(&l, 0, sizeof l);
    l.kind = RT_LIGHT_SPOT;
    l.has_origin = 1;
    l.origin[0] = 0.0f; l.origin[1] = 10.0f; l.origin[2] = 0.0f;
    V3 d1 = rt::normalize(rt::v3(0.0f, -1.0f, -0.0f));
    l.direction[0] = d1.x; l.direction[1] = d1.y; l.direction[2] = d1.z;
    l.angle = 60.0f * (float)(3.14159265358979323846 / 180.0); /* cgmath Deg -> Rad */
    l.softness = 1.0f;
    l.color[0] = 1.0f * 1.0f; l.color[1] = 0.5f * 1.0f; l.color[2] = 0.9f * 1.0f;
    if ((rc = rt_world_push_light(world, &l)) != RT_OK) return rc;

    memset(&l, 0, sizeof l);
    l.kind = RT_LIGHT_POINT;
    l.has_origin = 1;
    l.origin[0] = 0.0f; l.origin[1] = 0.1f; l.origin[2] = 0.0f;
    l.color[0] = 0.8f; l.color[1] = 0.8f; l.color[2] = 1.0f;
    if ((rc = rt_world_push_light(world, &l)) != RT_OK) return rc;
    return RT_OK;
}

/* main.rs:1077-1083 */
void rt_reference_camera(rt_camera *out) {
    if (!out) return;
    out->fovy = 60.0f * (float)(3.14159265358979323846 / 180.0);
    out->center[0] = 2.0f; out->center[1] = 2.5f; out->center[2] = 2.0f;
    V3 t = rt::normalize(rt::v3(-1.0f, -1.0f, -1.0f));
    out->toward[0] = t.x; out->toward[1] = t.y; out->toward[2] = t.z;
    V3 u = rt::normalize(rt::v3(0.0f, 1.0f, 0.0f));
    out->up[0] = u.x; out->up[1] = u.y; out->up[2] = u.z;
    out->near = -0.1f;
}

void rt_world_desc(const rt_world *world, rt_scene_desc *out) {
    if (!world || !out) return;
    out->triangles = world->triangles.data(); out->n_triangles = (uint32_t)world->triangles.size();
    out->spheres = world->spheres.data();     out->n_spheres = (uint32_t)world->spheres.size();
    out->materials = world->objects.data();   out->n_materials = (uint32_t)world->objects.size();
    out->lights = world->lights.data();       out->n_lights = (uint32_t)world->lights.size();
}

/* ---- the scene as a data format -----------------------------------
 * One flat little-endian file: a 128-byte header, then the four arrays of rt_scene_desc exactly as they sit in memory
 * (rt_material[], rt_triangle[], rt_sphere[], rt_light[]: include/rt_amd.h).  Array order is kept (ties and the light
 * sum depend on it).  The header records each record's size so that a reader built against another ABI revision
 * refuses the file instead of misreading it. */
struct SceneFileHeader {
    char magic[8];          /* "RTSCENE\0" */
    uint32_t version;       /* 1 */
    uint32_t endian;        /* 0x01020304 as written by the producer */
    uint32_t n_materials, n_triangles, n_spheres, n_lights;
    uint32_t sizeof_material, sizeof_triangle, sizeof_sphere, sizeof_light;
    uint32_t has_camera;
    rt_camera camera;       /* 11 f32 */
    uint32_t reserved[8];
};
static_assert(sizeof(SceneFileHeader) == 128, "scene file header");
static const char SCENE_MAGIC[8] = {'R', 'T', 'S', 'C', 'E', 'N', 'E', 0};

int rt_world_save_scene(const rt_world *world, const rt_camera *camera, const char *path) {
    if (!world || !path) return fail(RT_ERR_INVALID_ARGUMENT, "rt_world_save_scene: null argument");
    SceneFileHeader h;
    memset(&h, 0, sizeof h);
    memcpy(h.magic, SCENE_MAGIC, 8);
    h.version = 1u;
    h.endian = 0x01020304u;
    h.n_materials = (uint32_t)world->objects.size();
    h.n_triangles = (uint32_t)world->triangles.size();
    h.n_spheres = (uint32_t)world->spheres.size();
    h.n_lights = (uint32_t)world->lights.size();
    h.sizeof_material = (uint32_t)sizeof(rt_material);
    h.sizeof_triangle = (uint32_t)sizeof(rt_triangle);
    h.sizeof_sphere = (uint32_t)sizeof(rt_sphere);
    h.sizeof_light = (uint32_t)sizeof(rt_light);
    if (camera) { h.has_camera = 1u; h.camera = *camera; }
    const std::string tmp = std::string(path) + ".tmp"; /* written beside the target, then renamed over it (as write_to_file) */
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_world_save_scene: cannot open ") + tmp + ": " + strerror(errno));
    bool ok = fwrite(&h, sizeof h, 1, f) == 1;
    auto put = [&](const void *data, size_t size, size_t n) { if (ok && n) ok = fwrite(data, size, n, f) == n; };
    put(world->objects.data(), sizeof(rt_material), world->objects.size());
    put(world->triangles.data(), sizeof(rt_triangle), world->triangles.size());
    put(world->spheres.data(), sizeof(rt_sphere), world->spheres.size());
    put(world->lights.data(), sizeof(rt_light), world->lights.size());
    ok = (fclose(f) == 0) && ok;
    if (!ok || rename(tmp.c_str(), path) != 0) {
        remove(tmp.c_str());
        return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_world_save_scene: write failed for ") + path);
    }
    return RT_OK;
}

int rt_world_load_scene(rt_world *world, const char *path, rt_camera *out_camera, int *out_has_camera) {
    if (!world || !path) return fail(RT_ERR_INVALID_ARGUMENT, "rt_world_load_scene: null argument");
    if (out_has_camera) *out_has_camera = 0;
    FILE *f = fopen(path, "rb");
    if (!f) return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_world_load_scene: cannot open ") + path + ": " + strerror(errno));
    SceneFileHeader h;
    auto bail = [&](const char *why) { fclose(f); return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_world_load_scene: ") + why + " in " + path); };
    if (fread(&h, sizeof h, 1, f) != 1) return bail("short header");
    if (memcmp(h.magic, SCENE_MAGIC, 8) != 0) return bail("not a scene file (bad magic)");
    if (h.endian != 0x01020304u) return bail("written on a machine of the other byte order");
    if (h.version != 1u) { fclose(f); return fail(RT_ERR_UNSUPPORTED, std::string("rt_world_load_scene: unknown version in ") + path); }
    if (h.sizeof_material != sizeof(rt_material) || h.sizeof_triangle != sizeof(rt_triangle) || h.sizeof_sphere != sizeof(rt_sphere) ||
        h.sizeof_light != sizeof(rt_light)) {
        fclose(f);
        return fail(RT_ERR_UNSUPPORTED, std::string("rt_world_load_scene: record sizes of another ABI revision in ") + path);
    }
    const uint64_t body = (uint64_t)h.n_materials * sizeof(rt_material) + (uint64_t)h.n_triangles * sizeof(rt_triangle) +
                          (uint64_t)h.n_spheres * sizeof(rt_sphere) + (uint64_t)h.n_lights * sizeof(rt_light);
    if (fseek(f, 0, SEEK_END) != 0) return bail("cannot seek");
    const long end = ftell(f);
    if (end < 0 || (uint64_t)end != sizeof h + body) return bail("file size does not match the counts in its header");
    if (fseek(f, (long)sizeof h, SEEK_SET) != 0) return bail("cannot seek");
    rt_world fresh; /* the world is replaced only when the whole file is good */
    bool ok = true;
    try {
        fresh.objects.resize(h.n_materials);
        fresh.triangles.resize(h.n_triangles);
        fresh.spheres.resize(h.n_spheres);
        fresh.lights.resize(h.n_lights);
    } catch (...) {
        fclose(f);
        return fail(RT_ERR_OUT_OF_MEMORY, "rt_world_load_scene: out of memory");
    }
    auto get = [&](void *data, size_t size, size_t n) { if (ok && n) ok = fread(data, size, n, f) == n; };
    get(fresh.objects.data(), sizeof(rt_material), fresh.objects.size());
    get(fresh.triangles.data(), sizeof(rt_triangle), fresh.triangles.size());
    get(fresh.spheres.data(), sizeof(rt_sphere), fresh.spheres.size());
    get(fresh.lights.data(), sizeof(rt_light), fresh.lights.size());
    if (!ok) return bail("short read");
    fclose(f);
    for (const rt_material &m : fresh.objects)
        if (m.diffuse_fn > RT_DIFFUSE_STRIPE_SUM || m.normal_fn > RT_NORMAL_WAVE_U) return fail(RT_ERR_INVALID_ARGUMENT, "rt_world_load_scene: unknown material function");
    for (const rt_triangle &t : fresh.triangles)
        if (t.object_index >= h.n_materials) return fail(RT_ERR_INVALID_ARGUMENT, "rt_world_load_scene: triangle object index out of range");
    for (const rt_sphere &sp : fresh.spheres)
        if (sp.object_index >= h.n_materials) return fail(RT_ERR_INVALID_ARGUMENT, "rt_world_load_scene: sphere object index out of range");
    for (const rt_light &l : fresh.lights)
        if (l.kind > RT_LIGHT_POINT) return fail(RT_ERR_INVALID_ARGUMENT, "rt_world_load_scene: unknown light kind");
    world->objects.swap(fresh.objects);
    world->triangles.swap(fresh.triangles);
    world->spheres.swap(fresh.spheres);
    world->lights.swap(fresh.lights);
    if (h.has_camera && out_camera) *out_camera = h.camera;
    if (out_has_camera) *out_has_camera = h.has_camera ? 1 : 0;
    return RT_OK;
}

void rt_frame_full(uint32_t width, uint32_t height, int32_t max_depth, rt_frame *out) {
    if (!out) return;
    out->width = width; out->height = height; out->max_depth = max_depth;
    out->x0 = 0; out->y0 = 0; out->x1 = width; out->y1 = height; out->y_step = 1;
}

/* ---- post_process / encode / PNG ------------------------------------------ */

/* the luma weights post_process uses (palette's LinSrgb::into_luma: the Y row of its rgb -> xyz matrix): for callers that take the
 * percentile themselves (dist.post_process_sharded: the p99 of a frame whose rows live on several ranks) */
void rt_luma_row(float *row3) {
    if (row3) rt::luma_row(row3);
}

/* main.rs:748-762 */
float rt_post_process(float *rgb, size_t n_pixels) {
    if (!rgb || n_pixels == 0) return 0.0f;
    float row[3];
    rt::luma_row(row);
    std::vector<float> lum;
    lum.reserve(n_pixels);
    for (size_t i = 0; i < n_pixels; ++i) {
        const float l = (row[0] * rgb[3 * i]) + (row[1] * rgb[3 * i + 1]) + (row[2] * rgb[3 * i + 2]);
        if (rtdm::is_normal(l)) lum.push_back(l);
    }
    if (lum.empty()) return 0.0f;
    size_t idx = (size_t)((float)lum.size() * 0.99f);
    if (idx >= lum.size()) idx = lum.size() - 1;
    /* the k-th smallest of a sorted copy == nth_element; order-independent, so bit-exact */
    std::nth_element(lum.begin(), lum.begin() + (ptrdiff_t)idx, lum.end());
    const float p98 = lum[idx];
    if (p98 > RT_F_EPSILON) {
        for (size_t i = 0; i < n_pixels * 3; ++i) rgb[i] = rgb[i] / p98;
        return p98;
    }
    return 0.0f;
}

/* image.rs:55-66: Linear -> sRGB transfer, then f32 -> u8 (x*255, clamp, truncate) */
/* photon.rs:25-28, once per surviving sample, epoch by epoch */
void rt_accumulate(const float *samples, const uint8_t *valid, uint32_t n_epochs, size_t n_pixels, float *sum, float *weight) {
    for (uint32_t e = 0; e < n_epochs; ++e) {
        const float *s = samples + (size_t)e * n_pixels * 3;
        const uint8_t *v = valid + (size_t)e * n_pixels;
        for (size_t i = 0; i < n_pixels; ++i) {
            if (!v[i]) continue;
            sum[3 * i] = sum[3 * i] + s[3 * i];
            sum[3 * i + 1] = sum[3 * i + 1] + s[3 * i + 1];
            sum[3 * i + 2] = sum[3 * i + 2] + s[3 * i + 2];
            weight[i] += 1.0f;
        }
    }
}

/* photon.rs:15-23 */
void rt_accumulator_resolve(const float *sum, const float *weight, size_t n_pixels, float *rgb) {
    for (size_t i = 0; i < n_pixels; ++i) {
        const bool empty = weight[i] < 1.1920928955078125e-7f; /* std::f32::EPSILON */
        rgb[3 * i] = empty ? 0.0f : sum[3 * i] / weight[i];
        rgb[3 * i + 1] = empty ? 0.0f : sum[3 * i + 1] / weight[i];
        rgb[3 * i + 2] = empty ? 0.0f : sum[3 * i + 2] / weight[i];
    }
}

/* ---- film queries: the CPU definition (include/rt_amd.h "film queries"; the arithmetic is rt_film.h's, shared with the device) ---- */

int rt_film_offsets_host(const rt_frame *frame, uint32_t spp, uint32_t pattern, uint32_t seed, float *offsets) {
    bool unsupported;
    const char *bad = rt::film_offsets_limits(frame, spp, pattern, &unsupported);
    if (bad) return fail(unsupported ? RT_ERR_UNSUPPORTED : RT_ERR_INVALID_ARGUMENT, std::string("rt_film_offsets_host: ") + bad);
    if (!offsets) return fail(RT_ERR_INVALID_ARGUMENT, "rt_film_offsets_host: null offset pointer");
    const rt::FilmTile t = rt::film_tile(frame);
    const uint32_t k = rt::film_strata(spp);
    const size_t n_pixels = (size_t)t.rows * t.cols;
    for (uint32_t s = 0; s < spp; ++s)
        for (uint32_t row = 0; row < t.rows; ++row)
            for (uint32_t col = 0; col < t.cols; ++col) {
                const uint32_t pixel = rt::film_global_pixel(t, row, col);
                float *o = offsets + 2u * ((size_t)s * n_pixels + (size_t)row * t.cols + col);
                o[0] = rt::film_offset(pattern, k, pixel, seed, s, 0u);
                o[1] = rt::film_offset(pattern, k, pixel, seed, s, 1u);
            }
    return RT_OK;
}

int rt_film_splat_host(uint32_t rows, uint32_t cols, const float *samples, const uint8_t *valid, const float *offsets, uint32_t spp,
                       uint32_t filter, float radius, float *sum, float *weight) {
    const char *bad = rt::film_splat_limits(rows, cols, spp, filter, radius);
    if (bad) return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_film_splat_host: ") + bad);
    if (rows == 0u || cols == 0u) return RT_OK;
    if (!samples || !offsets || !sum || !weight) return fail(RT_ERR_INVALID_ARGUMENT, "rt_film_splat_host: null sample, offset, sum or weight pointer");
    rt::film_splat_cpu<rt::UniformLayout>({{samples, valid, offsets, (uint64_t)rows * cols, spp}, sum, weight, rows, cols, filter, radius});
    return RT_OK;
}

/* ---- area-light queries: the sampler on the CPU (include/rt_amd.h "area-light queries"; the arithmetic is rt_area_light.h's, shared with the device) ---- */

int rt_area_light_samples_cpu(const rt_light *lights, uint32_t light_first, uint32_t light_count, const float *radii, const uint32_t *ids, size_t n,
                              uint32_t spp, uint32_t pattern, uint32_t seed, float *sample) {
    const char *const who = "rt_area_light_samples_cpu: ";
    const uint64_t pairs = (uint64_t)n * light_count;
    if ((uint64_t)n >= (1ull << 32) || pairs >= (1ull << 32) || pairs * spp >= (1ull << 32))
        return fail(RT_ERR_UNSUPPORTED, std::string(who) + "2^32 (sample, light, record) entries or more (pass the lights in several ranges, or fewer samples)");
    if (n == 0 || light_count == 0) return RT_OK;
    if (!lights || !radii || !sample) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null light, radius or sample pointer");
    if (const char *bad = rt::area_light_limits(spp, true, pattern)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + bad);
    const uint32_t k = rt::film_strata(spp);
    for (uint32_t s = 0; s < spp; ++s)
        for (uint32_t l = 0; l < light_count; ++l) {
            const rt_light &L = lights[(size_t)light_first + l];
            float *const plane = sample + 3u * ((size_t)s * light_count + l) * n;
            for (size_t i = 0; i < n; ++i) {
                const V3 p = rt::area_light_sample(L, light_first + l, radii[l], pattern, k, ids ? ids[i] : (uint32_t)i, seed, s);
                plane[3u * i] = p.x;
                plane[3u * i + 1u] = p.y;
                plane[3u * i + 2u] = p.z;
            }
        }
    return RT_OK;
}

/* ---- hemisphere queries: the sampler and the fold on the CPU (include/rt_amd.h "hemisphere queries"; the arithmetic is rt_hemisphere.h's, shared with the device) ---- */

static int hemisphere_counts(const char *who, size_t n, uint32_t spp) {
    if ((uint64_t)n >= (1ull << 32) || (uint64_t)n * spp >= (1ull << 32))
        return fail(RT_ERR_UNSUPPORTED, std::string(who) + "2^32 (sample, record) entries or more (query the records in several calls, or fewer samples)");
    return RT_OK;
}

int rt_hemisphere_dirs_cpu(const float *normals, const uint32_t *ids, size_t n, uint32_t spp, uint32_t pattern, uint32_t seed, float *dirs) {
    const char *const who = "rt_hemisphere_dirs_cpu: ";
    if (const int rc = hemisphere_counts(who, n, spp)) return rc;
    if (n == 0) return RT_OK;
    if (!normals || !dirs) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null normal or direction pointer");
    if (const char *bad = rt::hemisphere_limits(spp, true, pattern, RT_HEMISPHERE_GEOMETRIC)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + bad);
    const uint32_t k = rt::film_strata(spp), seed_h = rt::hemisphere_seed(seed);
    for (uint32_t s = 0; s < spp; ++s) {
        float *const plane = dirs + 3u * (size_t)s * n;
        for (size_t i = 0; i < n; ++i) {
            const V3 d = rt::hemisphere_dir(pattern, k, ids ? ids[i] : (uint32_t)i, seed_h, s, rt::v3p(normals + 3u * i));
            plane[3u * i] = d.x;
            plane[3u * i + 1u] = d.y;
            plane[3u * i + 2u] = d.z;
        }
    }
    return RT_OK;
}

int rt_hemisphere_fold_cpu(const rt_hit *hits, const unsigned char *valid, const float *diffuse_color, const float *shiness, size_t n, uint32_t spp,
                           const unsigned char *asks, const rt_hit *shadow_hits, float max_distance, const float *radiance, unsigned char *open,
                           float *ambient, float *rgb) {
    const char *const who = "rt_hemisphere_fold_cpu: ";
    if (const int rc = hemisphere_counts(who, n, spp)) return rc;
    if (n == 0) return RT_OK;
    if ((radiance != nullptr) != (rgb != nullptr))
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null radiance or rgb (they are given together or not at all) pointer");
    if (!hits || !valid || !asks || (rgb && (!diffuse_color || !shiness)))
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null hit, valid, flag, diffuse-colour or shiness pointer");
    if (const char *bad = rt::hemisphere_limits(spp, false, 0u, 0u)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + bad);
    const rt::HemisphereFold f = {(uint64_t)n, spp, asks, reinterpret_cast<const uint32_t *>(shadow_hits), max_distance, radiance, open, ambient, rgb};
    for (size_t i = 0; i < n; ++i)
        rt::hemisphere_fold_record(f, i, valid[i] != 0, rt::v3p(hits[i].position), rgb ? rt::v3p(diffuse_color + 3u * i) : rt::v3(0.0f, 0.0f, 0.0f),
                                   rgb ? shiness[i] : 0.0f);
    return RT_OK;
}

/* ---- environment queries: the lookup, the table, the sampler and the fold on the CPU (include/rt_amd.h "environment queries"; the arithmetic is rt_environment.h's, shared with the device) ---- */

static int environment_counts(const char *who, size_t n, uint32_t spp) {
    if ((uint64_t)n >= (1ull << 32) || (uint64_t)n * spp >= (1ull << 32))
        return fail(RT_ERR_UNSUPPORTED, std::string(who) + "2^32 (sample, record) entries or more (query the records in several calls, or fewer samples)");
    return RT_OK;
}

static int environment_ok(const char *who, const rt_environment *env) {
    bool unsupported;
    if (const char *bad = rt::environment_limits(env, &unsupported)) return fail(unsupported ? RT_ERR_UNSUPPORTED : RT_ERR_INVALID_ARGUMENT, std::string(who) + bad);
    return RT_OK;
}

int rt_environment_lookup_cpu(const rt_environment *env, const rt_ray *rays, size_t n, const uint32_t *count, const rt_hit *hits, const uint32_t *parent,
                              float *out, size_t n_out) {
    const char *const who = "rt_environment_lookup_cpu: ";
    if (const int rc = environment_counts(who, n, 1u)) return rc;
    if (const int rc = environment_ok(who, env)) return rc;
    if (n == 0) return RT_OK;
    if (!rays || !out) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null ray or output pointer");
    const rt::EnvLookup a = {*env, reinterpret_cast<const uint32_t *>(rays), (uint64_t)n, count, reinterpret_cast<const uint32_t *>(hits), parent, out, (uint64_t)n_out};
    const uint64_t live = count != nullptr && *count < n ? *count : n;
    for (uint64_t j = 0; j < live; ++j) rt::env_lookup_record(a, j);
    return RT_OK;
}

int rt_environment_table_cpu(const rt_environment *env, void *table) {
    const char *const who = "rt_environment_table_cpu: ";
    if (const int rc = environment_ok(who, env)) return rc;
    if (!table) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null table pointer");
    if ((reinterpret_cast<uintptr_t>(table) & 7u) != 0u) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "the table is not 8-byte aligned");
    float luma[3];
    rt::luma_row(luma);
    const uint32_t w = env->width, h = env->height;
    uint32_t *const header = static_cast<uint32_t *>(table);
    uint64_t *const marginal = rt::env_table_marginal(table);
    uint32_t *const rows = rt::env_table_rows(table, h);
    float w_max = 0.0f;
    for (uint32_t y = 0; y < h; ++y) {
        const float sin_row = rt::env_sin_row(y, h);
        for (uint32_t x = 0; x < w; ++x) {
            bool usable;
            const float v = rt::env_weight(*env, x, y, sin_row, luma[0], luma[1], luma[2], &usable);
            if (usable && v > w_max) w_max = v;
        }
    }
    uint64_t total = 0u;
    for (uint32_t y = 0; y < h; ++y) {
        const float sin_row = rt::env_sin_row(y, h);
        uint32_t sum = 0u;
        for (uint32_t x = 0; x < w; ++x) {
            bool usable;
            const float v = rt::env_weight(*env, x, y, sin_row, luma[0], luma[1], luma[2], &usable);
            sum += rt::env_quantum(v, usable, w_max);
            rows[(size_t)y * w + x] = sum;
        }
        total += sum;
        marginal[y] = total;
    }
    header[RT_ENV_TABLE_WIDTH] = w;
    header[RT_ENV_TABLE_HEIGHT] = h;
    header[RT_ENV_TABLE_TOTAL] = (uint32_t)total;
    header[RT_ENV_TABLE_TOTAL + 1u] = (uint32_t)(total >> 32);
    header[RT_ENV_TABLE_W_MAX] = rtdm::f32_bits(w_max);
    header[RT_ENV_TABLE_W_MAX + 1u] = 0u;
    return RT_OK;
}

int rt_environment_samples_cpu(const rt_environment *env, const void *table, const float *normals, const uint32_t *ids, size_t n, uint32_t spp,
                               uint32_t pattern, uint32_t seed, float *dirs, float *radiance, uint32_t *texel, unsigned char *asks) {
    const char *const who = "rt_environment_samples_cpu: ";
    if (const int rc = environment_counts(who, n, spp)) return rc;
    if (const int rc = environment_ok(who, env)) return rc;
    if (n == 0) return RT_OK;
    if (!table || !normals || !dirs || !radiance) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null table, normal, direction or radiance pointer");
    if (const char *bad = rt::hemisphere_limits(spp, true, pattern, RT_HEMISPHERE_GEOMETRIC)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + bad);
    const uint32_t k = rt::film_strata(spp), seed_e = rt::environment_seed(seed);
    const rt::EnvTable t = rt::env_table_view(*env, table);
    for (uint32_t s = 0; s < spp; ++s)
        for (size_t i = 0; i < n; ++i) {
            const size_t e = (size_t)s * n + i;
            V3 dir = rt::v3(0.0f, 0.0f, 0.0f), l = rt::v3(0.0f, 0.0f, 0.0f);
            uint32_t at = 0u;
            bool need = false;
            if (t.total > 0u) {
                const rt::EnvSample p = rt::env_sample_of(*env, t, pattern, k, ids ? ids[i] : (uint32_t)i, seed_e, s);
                dir = p.dir;
                at = p.y * env->width + p.x;
                need = p.ok && rt::hemisphere_asks(dir, rt::v3p(normals + 3u * i));
                if (need) l = rt::env_sample_radiance(*env, p);
            }
            dirs[3u * e] = dir.x;
            dirs[3u * e + 1u] = dir.y;
            dirs[3u * e + 2u] = dir.z;
            radiance[3u * e] = l.x;
            radiance[3u * e + 1u] = l.y;
            radiance[3u * e + 2u] = l.z;
            if (texel) texel[e] = at;
            if (asks) asks[e] = need ? 1 : 0;
        }
    return RT_OK;
}

int rt_environment_fold_cpu(const unsigned char *valid, const float *shiness, size_t n, uint32_t spp, const unsigned char *asks, const rt_hit *shadow_hits,
                            const float *radiance, const float *diffuse, const float *specular, unsigned char *open, float *rgb) {
    const char *const who = "rt_environment_fold_cpu: ";
    if (const int rc = environment_counts(who, n, spp)) return rc;
    if (n == 0) return RT_OK;
    if (!valid || !shiness || !asks || !radiance || !diffuse || !specular || !rgb)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null valid, shiness, flag, radiance, diffuse, specular or rgb pointer");
    if (const char *bad = rt::hemisphere_limits(spp, false, 0u, 0u)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + bad);
    const rt::EnvFold f = {(uint64_t)n, spp, asks, reinterpret_cast<const uint32_t *>(shadow_hits), radiance, diffuse, specular, open, rgb};
    for (size_t i = 0; i < n; ++i) rt::env_fold_record(f, i, valid[i] != 0, shiness[i]);
    return RT_OK;
}

/* ---- lobe queries: the sampler, the two densities and the weights on the CPU (include/rt_amd.h "lobe queries"; the arithmetic is rt_lobe.h's, shared with the device) ---- */

static rt::LobeSurface lobe_surface_of(const rt_surface &s, const float *normal, const float *view) {
    return rt::lobe_surface(rt::v3p(normal ? normal : s.shading_normal), rt::v3p(view), s.shiness, s.smoothness);
}

int rt_lobe_samples_cpu(const rt_surface *surfaces, const float *normals, const float *view, const uint32_t *ids, size_t n, uint32_t spp,
                        uint32_t pattern, uint32_t seed, float *dirs, float *pdf, unsigned char *lobe, unsigned char *asks) {
    const char *const who = "rt_lobe_samples_cpu: ";
    if (const int rc = hemisphere_counts(who, n, spp)) return rc;
    if (n == 0) return RT_OK;
    if (!surfaces || !view || !dirs || !pdf) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null surface, view, direction or pdf pointer");
    if (const char *bad = rt::hemisphere_limits(spp, true, pattern, RT_HEMISPHERE_SHADING)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + bad);
    const uint32_t k = rt::film_strata(spp), seed_h = rt::hemisphere_seed(seed);
    for (size_t i = 0; i < n; ++i) {
        const bool valid = surfaces[i].valid != 0u;
        const rt::LobeSurface l = lobe_surface_of(surfaces[i], normals ? normals + 3u * i : nullptr, view + 3u * i);
        for (uint32_t s = 0; s < spp; ++s) {
            const size_t e = (size_t)s * n + i;
            const rt::LobeSample p = rt::lobe_sample(l, pattern, k, ids ? ids[i] : (uint32_t)i, seed_h, s, valid);
            dirs[3u * e] = p.dir.x;
            dirs[3u * e + 1u] = p.dir.y;
            dirs[3u * e + 2u] = p.dir.z;
            pdf[e] = valid ? p.pdf : 0.0f;
            if (lobe) lobe[e] = p.specular ? 1 : 0;
            if (asks) asks[e] = p.ok ? 1 : 0;
        }
    }
    return RT_OK;
}

int rt_lobe_pdf_cpu(const rt_surface *surfaces, size_t n, const float *view, const float *dirs, uint32_t n_probes, uint32_t normal_kind, float *pdf) {
    const char *const who = "rt_lobe_pdf_cpu: ";
    if ((uint64_t)n >= (1ull << 32) || (uint64_t)n * n_probes >= (1ull << 32))
        return fail(RT_ERR_UNSUPPORTED, std::string(who) + "2^32 (record, probe) pairs or more (pass the probes in several calls)");
    if (n == 0 || n_probes == 0) return RT_OK;
    if (!surfaces || !view || !dirs || !pdf) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null surface, view, direction or pdf pointer");
    if (const char *bad = rt::lobe_pdf_limits(normal_kind)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + bad);
    for (size_t i = 0; i < n; ++i) {
        const bool valid = surfaces[i].valid != 0u;
        const rt::LobeSurface l = lobe_surface_of(surfaces[i], nullptr, view + 3u * i);
        for (uint32_t q = 0; q < n_probes; ++q) {
            const size_t e = (size_t)q * n + i;
            pdf[e] = valid ? rt::lobe_pdf(l, rt::v3p(dirs + 3u * e), true) : 0.0f;
        }
    }
    return RT_OK;
}

int rt_environment_pdf_cpu(const rt_environment *env, const void *table, const float *dirs, size_t count, float *pdf, uint32_t *texel) {
    const char *const who = "rt_environment_pdf_cpu: ";
    if ((uint64_t)count >= (1ull << 32)) return fail(RT_ERR_UNSUPPORTED, std::string(who) + "2^32 directions or more (query them in several calls)");
    if (const int rc = environment_ok(who, env)) return rc;
    if (count == 0) return RT_OK;
    if (!table || !dirs || !pdf) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null table, direction or pdf pointer");
    const rt::EnvTable t = rt::env_table_view(*env, table);
    for (size_t e = 0; e < count; ++e) {
        uint32_t at;
        pdf[e] = rt::env_pdf(*env, t, rt::v3p(dirs + 3u * e), &at);
        if (texel) texel[e] = at;
    }
    return RT_OK;
}

int rt_mis_weigh_cpu(size_t count, const float *pdf_own, uint32_t n_own, const float *pdf_other, uint32_t n_other, uint32_t heuristic, int divide_by_own,
                     float *weight, float *rgb) {
    const char *const who = "rt_mis_weigh_cpu: ";
    if ((uint64_t)count >= (1ull << 32)) return fail(RT_ERR_UNSUPPORTED, std::string(who) + "2^32 entries or more (weigh them in several calls)");
    if (count == 0) return RT_OK;
    if (!pdf_own || (!weight && !rgb)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null own-pdf, or weight and rgb (one of the two is given) pointer");
    if (const char *bad = rt::mis_limits(heuristic)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + bad);
    const rt::MisWeigh m = rt::mis_weigh_call((uint64_t)count, pdf_own, n_own, pdf_other, n_other, heuristic, divide_by_own != 0, weight, rgb);
    for (uint64_t e = 0; e < count; ++e) rt::mis_weigh_entry(m, e);
    return RT_OK;
}

/* ---- path queries: the record, the step and the resolve on the CPU (include/rt_amd.h "path queries"; the arithmetic is rt_path.h's, shared with the device) ---- */

/* What the listed forms of the path loop share — the path, transmission, connection and light-connection queries below: the count's
 * limit, the material of a surface record and the store into a plane of three floats; the walk is each_listed, above the C region. */
static int listed_count(const char *who, size_t m) {
    if ((uint64_t)m >= (1ull << 32)) return fail(RT_ERR_UNSUPPORTED, std::string(who) + "2^32 records or more (checked first; query them in several calls)");
    return RT_OK;
}

static rt::Mat mat_of(const rt_surface &s) {
    rt::Mat mat;
    mat.normal = rt::v3p(s.normal);
    mat.diffuse = rt::v3p(s.diffuse_color);
    mat.specular = rt::v3p(s.specular_color);
    mat.shiness = s.shiness;
    mat.smoothness = s.smoothness;
    mat.transparency = s.transparency;
    mat.refraction_index = s.refraction_index;
    mat.opaque_decay = s.opaque_decay;
    return mat;
}

static void put_v3(float *plane, size_t j, V3 v) {
    plane[3u * j] = v.x;
    plane[3u * j + 1u] = v.y;
    plane[3u * j + 2u] = v.z;
}

int rt_path_begin_cpu(size_t n, uint32_t spp, const uint32_t *ids, rt_path *paths, float *radiance) {
    const char *const who = "rt_path_begin_cpu: ";
    if (const int rc = hemisphere_counts(who, n, spp)) return rc;
    if (n == 0) return RT_OK;
    if (!paths || !radiance) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null path or radiance pointer");
    if (const char *bad = rt::hemisphere_limits(spp, false, 0u, 0u)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + bad);
    for (uint32_t s = 0; s < spp; ++s)
        for (size_t i = 0; i < n; ++i) {
            const size_t k = (size_t)s * n + i;
            paths[k] = rt::path_begin_record((uint32_t)i, ids ? ids[i] : (uint32_t)i, s);
            radiance[3u * k] = radiance[3u * k + 1u] = radiance[3u * k + 2u] = 0.0f;
        }
    return RT_OK;
}

int rt_path_advance_cpu(const rt_surface *surfaces, const float *normals, const float *view, rt_path *paths, size_t m, const uint32_t *index,
                        const uint32_t *count, const float *emitted, uint32_t seed, uint32_t rr_start, float rr_floor, int last, float *radiance, float *dirs,
                        unsigned char *alive) {
    const char *const who = "rt_path_advance_cpu: ";
    if (const int rc = listed_count(who, m)) return rc;
    if (m == 0) return RT_OK;
    if (!surfaces || !view || !paths || (index && !count) || !radiance || !dirs || !alive)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null surface, view, path, count (with an index), radiance, direction or flag pointer");
    if (const char *bad = rt::path_limits(RT_HEMISPHERE_SHADING, rr_floor)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + bad);
    const rt::PathStep step = {seed, rr_start, rr_floor, last != 0};
    each_listed(index, count, m, [&](uint32_t j) {
        rt_path &p = paths[j];
        if ((p.flags & RT_PATH_ALIVE) == 0u) return;
        if (emitted)
            for (uint32_t c = 0; c < 3u; ++c) radiance[3u * j + c] = rt::path_deposit(radiance[3u * j + c], p.beta[c], emitted[3u * j + c]);
        const rt_surface &s = surfaces[j];
        const V3 shading_n = rt::v3p(s.shading_normal);
        V3 dir;
        const bool lives = rt::path_advance_record(p, s.valid != 0u, mat_of(s), shading_n, normals ? rt::v3p(normals + 3u * j) : shading_n, rt::v3p(view + 3u * j),
                                                   step, &dir);
        put_v3(dirs, j, dir);
        alive[j] = lives ? 1 : 0;
    });
    return RT_OK;
}

int rt_path_resolve_cpu(const float *radiance, size_t n, uint32_t spp, const uint32_t *root, float *rgb) {
    const char *const who = "rt_path_resolve_cpu: ";
    if (const int rc = hemisphere_counts(who, n, spp)) return rc;
    if (n == 0) return RT_OK;
    if (!radiance || !rgb) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null radiance or rgb pointer");
    if (const char *bad = rt::hemisphere_limits(spp, false, 0u, 0u)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + bad);
    for (size_t i = 0; i < n; ++i) rt::path_resolve_root(radiance, (uint64_t)n, spp, i, root, rgb);
    return RT_OK;
}

/* ---- transmission queries: the choice and the fold on the CPU (include/rt_amd.h "transmission queries"; the arithmetic is rt_transmit.h's, shared with the device) ---- */

int rt_path_branch_cpu(const rt_surface *surfaces, const rt_hit *hits, const rt_ray *incoming, rt_path *paths, size_t m, const uint32_t *index,
                       const uint32_t *count, uint32_t seed, int last, unsigned char *lobe, unsigned char *transmit, rt_ray *walk_rays, uint32_t *kind,
                       float *travel, uint32_t *casts, unsigned char *walk_flags) {
    const char *const who = "rt_path_branch_cpu: ";
    if (const int rc = listed_count(who, m)) return rc;
    if (m == 0) return RT_OK;
    if (!surfaces || !hits || !incoming || !paths || (index && !count) || !lobe || !transmit || !walk_rays || !kind || !travel || !casts || !walk_flags)
        return fail(RT_ERR_INVALID_ARGUMENT,
                    std::string(who) + "null surface, hit, incoming-ray, path, count (with an index), lobe, transmit, walk-ray, kind, travel, cast-count or walk-flag pointer");
    each_listed(index, count, m, [&](uint32_t j) {
        rt_path &p = paths[j];
        bool transmits = false, lobes = false;
        uint32_t result = RT_HIT_NONE;
        rt_ray inside = rt::no_ray_record();
        if ((p.flags & RT_PATH_ALIVE) != 0u) {
            const rt_surface &s = surfaces[j];
            const bool valid = s.valid != 0u;
            transmits = rt::path_transmits(p.id, p.bounce, seed, valid, valid ? s.transparency : 0.0f);
            if (transmits && last) {
                p.flags = 0u;
                transmits = false;
            } else if (transmits) {
                result = rt::refract_enter_record(true, rt::v3p(hits[j].position), rt::v3p(hits[j].normal), rt::v3p(incoming[j].direction), s.refraction_index,
                                                  hits[j].kind, hits[j].index, &inside);
            } else {
                lobes = true;
            }
        }
        lobe[j] = lobes ? 1 : 0;
        transmit[j] = transmits ? 1 : 0;
        walk_rays[j] = inside;
        kind[j] = result;
        travel[j] = 0.0f;
        casts[j] = 0u;
        walk_flags[j] = result == RT_REFR_WALKING ? 1 : 0;
    });
    return RT_OK;
}

int rt_path_transmit_cpu(const rt_surface *surfaces, rt_path *paths, size_t m, const uint32_t *index, const uint32_t *count, uint32_t *kind, const float *travel,
                         const rt_ray *escape, uint32_t seed, uint32_t rr_start, float rr_floor, rt_ray *next_rays, unsigned char *alive,
                         unsigned char *walk_flags) {
    const char *const who = "rt_path_transmit_cpu: ";
    if (const int rc = listed_count(who, m)) return rc;
    if (m == 0) return RT_OK;
    if (!surfaces || !paths || (index && !count) || !kind || !travel || !escape || !next_rays || !alive || !walk_flags)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null surface, path, count (with an index), kind, travel, escape-ray, ray, flag or walk-flag pointer");
    if (const char *bad = rt::path_limits(RT_HEMISPHERE_SHADING, rr_floor)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + bad);
    const rt::PathStep step = {seed, rr_start, rr_floor, false};
    each_listed(index, count, m, [&](uint32_t j) {
        const uint32_t walk = kind[j];
        kind[j] = RT_HIT_NONE;
        walk_flags[j] = 0;
        rt_path &p = paths[j];
        if ((p.flags & RT_PATH_ALIVE) == 0u) return;
        const bool valid = surfaces[j].valid != 0u;
        const bool lives = rt::path_transmit_record(p, walk, valid, valid ? surfaces[j].opaque_decay : 0.0f, travel[j], step);
        alive[j] = lives ? 1 : 0;
        next_rays[j] = lives ? escape[j] : rt::no_ray_record();
    });
    return RT_OK;
}

/* ---- connection queries: the connection, the settlement and the escape weight on the CPU (include/rt_amd.h "connection queries"; the arithmetic is rt_connect.h's, shared with the device) ---- */

int rt_path_connect_cpu(const rt_surface *surfaces, const float *normals, const float *view, const rt_environment *env, const void *table,
                        const rt_path *paths, size_t m, const uint32_t *index, const uint32_t *count, uint32_t seed, uint32_t heuristic, int last,
                        float *dirs, unsigned char *asks, float *pending) {
    const char *const who = "rt_path_connect_cpu: ";
    if (const int rc = listed_count(who, m)) return rc;
    if (const int rc = environment_ok(who, env)) return rc;
    if (m == 0) return RT_OK;
    if (!surfaces || !view || !table || !paths || (index && !count) || !dirs || !asks || !pending)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null surface, view, table, path, count (with an index), direction, flag or pending pointer");
    if (const char *bad = rt::connect_limits(RT_HEMISPHERE_SHADING, heuristic)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + bad);
    const rt::PathConnect step = {seed, heuristic, last != 0};
    const rt::EnvTable t = rt::env_table_view(*env, table);
    each_listed(index, count, m, [&](uint32_t j) {
        const rt_path &p = paths[j];
        if ((p.flags & RT_PATH_ALIVE) == 0u) return;
        const rt_surface &s = surfaces[j];
        const V3 shading_n = rt::v3p(s.shading_normal);
        const rt::Connection c = rt::path_connect_record(p, s.valid != 0u, mat_of(s), shading_n, normals ? rt::v3p(normals + 3u * j) : shading_n,
                                                         rt::v3p(view + 3u * j), *env, t, step);
        put_v3(dirs, j, c.dir);
        asks[j] = c.ask ? 1 : 0;
        if (c.ask) put_v3(pending, j, c.pending);
    });
    return RT_OK;
}

int rt_path_settle_cpu(const rt_path *paths, size_t m, const uint32_t *index, const uint32_t *count, unsigned char *asks, const rt_hit *shadow_hits,
                       const float *pending, float *radiance) {
    const char *const who = "rt_path_settle_cpu: ";
    if (const int rc = listed_count(who, m)) return rc;
    if (m == 0) return RT_OK;
    if (!paths || (index && !count) || !asks || !pending || !radiance)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null path, count (with an index), flag, pending or radiance pointer");
    each_listed(index, count, m, [&](uint32_t j) { rt::path_settle_record(j, asks, reinterpret_cast<const uint32_t *>(shadow_hits), pending, radiance); });
    return RT_OK;
}

int rt_path_weigh_escape_cpu(const rt_environment *env, const void *table, const rt_path *paths, size_t m, const uint32_t *index, const uint32_t *count,
                             const rt_hit *hits, const rt_ray *incoming, uint32_t heuristic, float *emitted) {
    const char *const who = "rt_path_weigh_escape_cpu: ";
    if (const int rc = listed_count(who, m)) return rc;
    if (const int rc = environment_ok(who, env)) return rc;
    if (m == 0) return RT_OK;
    if (!table || !paths || (index && !count) || !hits || !incoming || !emitted)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null table, path, count (with an index), hit, incoming-ray or emitted pointer");
    if (const char *bad = rt::mis_limits(heuristic)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + bad);
    const rt::EnvTable t = rt::env_table_view(*env, table);
    each_listed(index, count, m, [&](uint32_t j) {
        const rt_path &p = paths[j];
        if (!rt::path_escape_weighed(p.flags, hits[j].kind, p.pdf, t)) return;
        const float w = rt::path_escape_weight(*env, t, heuristic, p.pdf, rt::v3p(incoming[j].direction));
        for (uint32_t c = 0; c < 3u; ++c) emitted[3u * j + c] = emitted[3u * j + c] * w;
    });
    return RT_OK;
}

/* ---- light-connection queries: the connection and the settlement on the CPU (include/rt_amd.h "light-connection queries"; the arithmetic is rt_light_connect.h's, shared with the device) ---- */

int rt_path_connect_lights_cpu(const rt_surface *surfaces, const float *positions, const float *view, const rt_light *lights, const float *aux,
                               const rt_path *paths, size_t m, const uint32_t *index, const uint32_t *count, uint32_t light_first, uint32_t light_count,
                               const float *radii, const float *weights, uint32_t seed, float *dirs, unsigned char *asks, float *pending, float *reach,
                               uint32_t *chosen) {
    const char *const who = "rt_path_connect_lights_cpu: ";
    if (const int rc = listed_count(who, m)) return rc;
    if (m == 0 || light_count == 0) return RT_OK;
    if (!surfaces || !positions || !view || !lights || !paths || (index && !count) || !dirs || !asks || !pending || !reach)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null surface, position, view, light, path, count (with an index), direction, flag, pending or reach pointer");
    const size_t n_lights = (size_t)light_first + light_count;
    std::vector<rt::LightAux> light_aux(n_lights);
    for (size_t i = 0; i < n_lights; ++i) {
        light_aux[i] = rt::light_aux_of(lights[i]);
        if (aux) light_aux[i].cos_in = aux[2u * i], light_aux[i].cos_out = aux[2u * i + 1u];
    }
    const rt::LightConnect step = {seed, light_first, light_count, radii, weights};
    each_listed(index, count, m, [&](uint32_t j) {
        const rt_path &p = paths[j];
        if ((p.flags & RT_PATH_ALIVE) == 0u) return;
        const rt_surface &s = surfaces[j];
        const rt::LightConnection c = rt::light_connect_record(p, s.valid != 0u, mat_of(s), rt::v3p(s.shading_normal), rt::v3p(positions + 3u * (size_t)j),
                                                               rt::v3p(view + 3u * (size_t)j), lights, light_aux.data(), step);
        put_v3(dirs, j, c.dir);
        asks[j] = c.ask ? 1 : 0;
        if (chosen) chosen[j] = c.chosen;
        if (c.ask) {
            put_v3(pending, j, c.pending);
            reach[j] = c.reach;
        }
    });
    return RT_OK;
}

int rt_path_settle_lights_cpu(const rt_path *paths, size_t m, const uint32_t *index, const uint32_t *count, unsigned char *asks, const rt_ray *shadow_rays,
                              const rt_hit *shadow_hits, const float *reach, const float *pending, float *radiance) {
    const char *const who = "rt_path_settle_lights_cpu: ";
    if (const int rc = listed_count(who, m)) return rc;
    if (m == 0) return RT_OK;
    if (!paths || (index && !count) || !asks || !shadow_rays || !reach || !pending || !radiance)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null path, count (with an index), flag, ray, reach, pending or radiance pointer");
    each_listed(index, count, m, [&](uint32_t j) {
        rt::light_settle_record(j, asks, reinterpret_cast<const uint32_t *>(shadow_rays), reinterpret_cast<const uint32_t *>(shadow_hits), reach, pending, radiance);
    });
    return RT_OK;
}

/* ---- texture queries: the pyramid, the footprint, the lookup and the surface edit on the CPU (include/rt_amd.h "texture queries"; the arithmetic is rt_texture.h's, shared with the device) ---- */

static int texture_ok(const char *who, const rt_texture *tex) {
    bool unsupported;
    if (const char *bad = rt::texture_limits(tex, &unsupported)) return fail(unsupported ? RT_ERR_UNSUPPORTED : RT_ERR_INVALID_ARGUMENT, std::string(who) + bad);
    return RT_OK;
}

static int texture_count(const char *who, size_t n) {
    if ((uint64_t)n >= (1ull << 32)) return fail(RT_ERR_UNSUPPORTED, std::string(who) + "2^32 records or more (checked first; query them in several calls)");
    return RT_OK;
}

int rt_texture_pyramid_cpu(const rt_texture *tex) {
    if (const int rc = texture_ok("rt_texture_pyramid_cpu: ", tex)) return rc;
    const rt::TexView t = rt::tex_view(*tex);
    float *const texels = const_cast<float *>(tex->d_texels);
    for (uint32_t level = 1u; level < t.n_levels; ++level) {
        const uint32_t w = rt::tex_extent(t.width, level), h = rt::tex_extent(t.height, level);
        const rt::TexLevel src = {t.texels + 3u * (uint64_t)t.start[level - 1u], rt::tex_extent(t.width, level - 1u), rt::tex_extent(t.height, level - 1u)};
        float *const out = texels + 3u * (uint64_t)t.start[level];
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) {
                const V3 value = rt::tex_reduce(src, x, y);
                float *const o = out + 3u * ((uint64_t)y * w + x);
                o[0] = value.x, o[1] = value.y, o[2] = value.z;
            }
    }
    return RT_OK;
}

int rt_texture_footprint_cpu(const rt_scene_desc *scene, const rt_hit *hits, const rt_ray *incoming, size_t n, float spread, const float *width0,
                             float *footprint) {
    const char *const who = "rt_texture_footprint_cpu: ";
    if (const int rc = texture_count(who, n)) return rc;
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null scene");
    if (n == 0) return RT_OK;
    if (!hits || !incoming || !footprint) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null hit, incoming-ray or footprint pointer");
    if ((scene->n_triangles && !scene->triangles) || (scene->n_spheres && !scene->spheres))
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null triangle or sphere array in the scene description");
    for (size_t i = 0; i < n; ++i) {
        const uint32_t *const hit = reinterpret_cast<const uint32_t *>(hits + i);
        const uint32_t kind = hit[0], index = hit[1];
        const bool valid = kind <= 1u && hit[RT_TEX_HIT_OBJECT] < scene->n_materials;
        float ratio = 0.0f;
        bool ok = false;
        if (valid && kind == 1u && index < scene->n_triangles) {
            const rt_vertex *const v = scene->triangles[index].vertices;
            ratio = rt::tex_triangle_ratio(rt::v3p(v[0].position), rt::v3p(v[1].position), rt::v3p(v[2].position), v[0].uv[0], v[0].uv[1], v[1].uv[0],
                                           v[1].uv[1], v[2].uv[0], v[2].uv[1], &ok);
        } else if (valid && kind == 0u && index < scene->n_spheres) {
            ratio = rt::tex_sphere_ratio(scene->spheres[index].radius, &ok);
        }
        footprint[i] = rt::tex_footprint_record(hit, reinterpret_cast<const uint32_t *>(incoming + i), width0 ? width0[i] : 0.0f, spread, ratio, ok);
    }
    return RT_OK;
}

int rt_texture_sample_cpu(const rt_texture *tex, const float *uv, size_t uv_stride_words, const float *footprint, size_t n, float *out,
                          size_t out_stride_words) {
    const char *const who = "rt_texture_sample_cpu: ";
    if (const int rc = texture_count(who, n)) return rc;
    if (const int rc = texture_ok(who, tex)) return rc;
    if (n == 0) return RT_OK;
    if (!uv || !out) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null uv or output pointer");
    if (const char *bad = rt::tex_stride_limits(uv_stride_words, out_stride_words)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + bad);
    const rt::TexSample a = {rt::tex_view(*tex), uv, (uint64_t)uv_stride_words, footprint, (uint64_t)n, out, (uint64_t)out_stride_words};
    for (uint64_t i = 0; i < a.n; ++i) rt::tex_sample_record(a, i);
    return RT_OK;
}

int rt_texture_surfaces_cpu(const rt_texture *diffuse_tex, const rt_texture *normal_tex, const rt_hit *hits, const float *footprint, size_t n,
                            uint32_t object_index, uint32_t flags, rt_surface *surfaces) {
    const char *const who = "rt_texture_surfaces_cpu: ";
    if (const int rc = texture_count(who, n)) return rc;
    if (diffuse_tex)
        if (const int rc = texture_ok(who, diffuse_tex)) return rc;
    if (normal_tex)
        if (const int rc = texture_ok(who, normal_tex)) return rc;
    if (n == 0) return RT_OK;
    if (!hits || !surfaces) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + "null hit or surface pointer");
    if (const char *bad = rt::tex_surface_limits(flags)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + bad);
    if (!diffuse_tex && !normal_tex) return RT_OK;
    rt::TexSurfaces a = {};
    if (diffuse_tex) a.diffuse = rt::tex_view(*diffuse_tex);
    if (normal_tex) a.normal = rt::tex_view(*normal_tex);
    a.has_diffuse = diffuse_tex != nullptr, a.has_normal = normal_tex != nullptr;
    a.hits = reinterpret_cast<const uint32_t *>(hits);
    a.footprint = footprint;
    a.n = (uint64_t)n;
    a.object_index = object_index, a.flags = flags;
    a.surfaces = reinterpret_cast<uint32_t *>(surfaces);
    for (uint64_t i = 0; i < a.n; ++i) rt::tex_surface_record(a, i);
    return RT_OK;
}

/* ---- adaptive sampling queries: the CPU definition (include/rt_amd.h "adaptive sampling queries";the arithmetic is rt_adaptive.h's, shared with the device) ---- */

int rt_sample_budget_cpu(const float *mean, uint32_t mean_stride, const float *variance, uint32_t variance_stride, const uint32_t *count,
                         uint32_t count_stride, const uint32_t *valid, uint32_t valid_stride, const rt_sample_budget_params *params, size_t n,
                         uint32_t *budget) {
    return cpu_query("rt_sample_budget_cpu",
                     rt::SampleBudgetArgs{mean, mean_stride, variance, variance_stride, count, count_stride, valid, valid_stride, params, n, budget}, each_call);
}

int rt_sample_list_cpu(const uint32_t *counts, size_t n, size_t capacity, uint32_t *first, uint32_t *start, uint32_t *pixel, uint32_t *sample,
                       uint32_t *total) {
    int status;
    const char *bad = rt::sample_list_limits(counts, n, capacity, start, pixel, sample, total, &status);
    if (bad) return fail(status, std::string("rt_sample_list_cpu: ") + bad);
    uint64_t sum = 0u; /* S_i: below 2^32 */
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t lo = sum < capacity ? sum : capacity;
        sum += rt::sample_count_clamped(counts[i]);
        const uint64_t hi = sum < capacity ? sum : capacity;
        const uint32_t f = first ? first[i] : 0u;
        start[i] = (uint32_t)lo;
        for (uint64_t j = lo; j < hi; ++j) pixel[j] = (uint32_t)i, sample[j] = f + (uint32_t)(j - lo);
        if (first) first[i] = f + (uint32_t)(hi - lo);
    }
    start[n] = (uint32_t)(sum < capacity ? sum : capacity);
    total[0] = start[n];
    total[1] = (uint32_t)sum;
    return RT_OK;
}

int rt_film_offsets_listed_cpu(const rt_frame *frame, uint32_t pattern, uint32_t seed, const uint32_t *pixel, const uint32_t *sample,
                               const uint32_t *total, size_t capacity, float *offsets) {
    return cpu_query("rt_film_offsets_listed_cpu", rt::ListedOffsetsArgs{frame, pattern, seed, pixel, sample, total, capacity, offsets},
                     [](const rt::ListedOffsetsArgs &a) {
                         const rt::ListedOffsets o = a.call();
                         const uint64_t listed = rt::listed_count(o.total, o.capacity);
                         for (uint64_t j = 0; j < o.capacity; ++j) rt::listed_offsets_record(o, j, listed);
                     });
}

int rt_camera_rays_listed_cpu(const rt_camera *camera, const rt_frame *frame, const float *offsets, const uint32_t *pixel, const uint32_t *total,
                              size_t capacity, rt_ray *rays) {
    int status;
    const char *bad = rt::listed_rays_limits(camera, frame, offsets, pixel, total, capacity, rays, &status);
    if (bad) return fail(status, std::string("rt_camera_rays_listed_cpu: ") + bad);
    if (capacity == 0u) return RT_OK;
    const rt::ListedCamera c = {rt::temporal_camera(camera, frame), rt::film_tile(frame)};
    const uint64_t listed = rt::listed_count(total, capacity), n_pixels = (uint64_t)c.t.rows * c.t.cols;
    for (uint64_t j = 0; j < capacity; ++j) {
        uint32_t w[11] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        const uint32_t pix = j < listed ? pixel[j] : 0xffffffffu;
        if ((uint64_t)pix < n_pixels) {
            const uint32_t row = pix / c.t.cols, col = pix - row * c.t.cols;
            const uint32_t x = c.t.x0 + col, y = c.t.y0 + row * c.t.y_step;
            rt::listed_ray_words(c, (float)x + offsets[2u * j], (float)y + offsets[2u * j + 1u], w);
        }
        memcpy(rays + j, w, sizeof w);
    }
    return RT_OK;
}

int rt_film_splat_listed_cpu(uint32_t rows, uint32_t cols, const float *samples, const uint8_t *valid, const float *offsets, const uint32_t *start,
                             size_t capacity, uint32_t max_count, uint32_t filter, float radius, float *sum, float *weight) {
    int status;
    const char *bad = rt::listed_splat_limits(rows, cols, samples, offsets, start, capacity, max_count, filter, radius, sum, weight, &status);
    if (bad) return fail(status, std::string("rt_film_splat_listed_cpu: ") + bad);
    if (rows == 0u || cols == 0u) return RT_OK;
    rt::film_splat_cpu<rt::ListedLayout>({{samples, valid, offsets, start, capacity, max_count}, sum, weight, rows, cols, filter, radius});
    return RT_OK;
}

/* ---- denoise queries: the CPU definition (include/rt_amd.h "denoise queries"; the arithmetic is rt_denoise.h's, shared with the device) ---- */

int rt_denoise_atrous_cpu(const float *color, const rt_denoise_guides *guides, const rt_denoise_params *params, uint32_t rows, uint32_t cols,
                          float *out, float *temp) {
    return cpu_query("rt_denoise_atrous_cpu", rt::DenoiseArgs{color, guides, params, rows, cols, out, temp}, rt::atrous_cpu<rt::DenoiseFilter, rt::DenoiseArgs>);
}

/* ---- temporal queries: the CPU definition (include/rt_amd.h "temporal queries"; the arithmetic is rt_temporal.h's, shared with the device) ---- */

int rt_temporal_motion_cpu(const float *position, uint32_t position_stride, const uint32_t *valid, uint32_t valid_stride, const rt_camera *prev_camera,
                           const rt_frame *prev_frame, float *motion) {
    return cpu_query("rt_temporal_motion_cpu", rt::TemporalMotionArgs{position, position_stride, valid, valid_stride, prev_camera, prev_frame, motion}, each_call);
}

int rt_temporal_accumulate_cpu(const float *color, const float *motion, const rt_temporal_guides *current, const rt_temporal_guides *previous,
                               const rt_temporal_params *params, uint32_t rows, uint32_t cols, const rt_temporal_pixel *history_in,
                               rt_temporal_pixel *history_out, float *variance) {
    return cpu_query("rt_temporal_accumulate_cpu",
                     rt::TemporalAccumulateArgs{color, motion, current, previous, params, rows, cols, history_in, history_out, variance}, each_call);
}

/* ---- history rectification queries: the CPU definition (include/rt_amd.h "history rectification queries"; the arithmetic is rt_rectify.h's, shared with the device) ---- */

int rt_temporal_bounds_cpu(const float *color, uint32_t color_stride, const uint32_t *object, uint32_t object_stride, const uint32_t *valid,
                           uint32_t valid_stride, const rt_bounds_params *params, uint32_t rows, uint32_t cols, rt_temporal_box *box) {
    return cpu_query("rt_temporal_bounds_cpu", rt::RectifyBoundsArgs{color, color_stride, object, object_stride, valid, valid_stride, params, rows, cols, box},
                     [](const rt::RectifyBoundsArgs &a) {
                         const rt::RectifyBounds b = a.call();
                         for (uint32_t r = 0; r < b.rows; ++r)
                             for (uint32_t c = 0; c < b.cols; ++c) rt::rectify_bounds_pixel(b, r, c);
                     });
}

int rt_temporal_accumulate_bounded_cpu(const float *color, const float *motion, const rt_temporal_guides *current, const rt_temporal_guides *previous,
                                       const rt_temporal_params *params, uint32_t rows, uint32_t cols, const rt_temporal_pixel *history_in,
                                       rt_temporal_pixel *history_out, float *variance, const rt_temporal_box *box, uint32_t clamped_length,
                                       uint32_t *clamped) {
    return cpu_query("rt_temporal_accumulate_bounded_cpu",
                     rt::RectifyAccumulateArgs{{color, motion, current, previous, params, rows, cols, history_in, history_out, variance}, box, clamped_length, clamped},
                     each_call);
}

int rt_temporal_feedback_cpu(const float *color, uint32_t color_stride, const uint32_t *valid, uint32_t valid_stride, uint32_t rows, uint32_t cols,
                             rt_temporal_pixel *history) {
    return cpu_query("rt_temporal_feedback_cpu", rt::RectifyFeedbackArgs{color, color_stride, valid, valid_stride, rows, cols, history}, each_call);
}

/* ---- guided upsampling queries: the CPU definition (include/rt_amd.h "guided upsampling queries"; the arithmetic is rt_upsample.h's, shared with the device) ---- */

int rt_upsample_guided_cpu(const float *color_lo, uint32_t color_stride, const rt_denoise_guides *low, const uint32_t *object_lo, uint32_t object_lo_stride,
                           const rt_denoise_guides *full, const uint32_t *object_full, uint32_t object_full_stride, const rt_upsample_params *params,
                           uint32_t rows, uint32_t cols, float *out) {
    return cpu_query("rt_upsample_guided_cpu",
                     rt::UpsampleArgs{color_lo, color_stride, low, object_lo, object_lo_stride, full, object_full, object_full_stride, params, rows, cols, out},
                     each_call);
}

/* ---- bloom queries: the CPU definition (include/rt_amd.h "bloom queries"; the arithmetic and the order of a call's steps are rt_bloom.h's, shared with the device) ---- */

int rt_bloom_cpu(const float *color, uint32_t color_stride, const rt_bloom_params *params, uint32_t rows, uint32_t cols, float *temp, float *out) {
    return cpu_query("rt_bloom_cpu", rt::BloomArgs{color, color_stride, params, rows, cols, temp, out}, [](const rt::BloomArgs &a) {
        const auto step = [](const auto &op) { return each(op), true; };
        rt::bloom_steps(a, step, step);
    });
}

/* ---- variance-guided filter queries: the CPU definition (include/rt_amd.h "variance-guided filter queries"; the arithmetic is rt_svgf.h's, shared with the device) ---- */

int rt_svgf_variance_cpu(const rt_temporal_pixel *history, const rt_denoise_guides *guides, const rt_svgf_variance_params *params, uint32_t rows,
                         uint32_t cols, float *variance_out) {
    return cpu_query("rt_svgf_variance_cpu", rt::SvgfVarianceArgs{history, guides, params, rows, cols, variance_out}, [](const rt::SvgfVarianceArgs &a) {
        const rt::SvgfVariance v = a.call();
        for (uint32_t r = 0; r < v.rows; ++r)
            for (uint32_t c = 0; c < v.cols; ++c) v.out[(uint64_t)r * v.cols + c] = rt::svgf_variance_pixel(v, r, c);
    });
}

int rt_svgf_atrous_cpu(const float *color, uint32_t color_stride, const float *variance, const rt_denoise_guides *guides,
                       const rt_svgf_atrous_params *params, uint32_t rows, uint32_t cols, float *out, float *variance_out, void *temp) {
    return cpu_query("rt_svgf_atrous_cpu",
                     rt::SvgfAtrousArgs{color, color_stride, variance, guides, params, rows, cols, out, variance_out, static_cast<float *>(temp)},
                     rt::atrous_cpu<rt::SvgfFilter, rt::SvgfAtrousArgs>);
}

/* ---- motion queries: the CPU definition (include/rt_amd.h "motion queries"; the arithmetic is rt_motion.h's, shared with the device) ---- */

int rt_previous_positions_cpu(const rt_scene_desc *now, const float *was_triangles, const float *was_spheres, const rt_hit *hits, size_t n, float *was,
                              uint32_t was_stride) {
    int status;
    bool done;
    const bool kept = now && (was_triangles || now->n_triangles == 0u) && (was_spheres || now->n_spheres == 0u);
    const char *bad = rt::motion_limits(n, now, kept, "null was_triangles with n_triangles > 0, or null was_spheres with n_spheres > 0", hits, was,
                                        was_stride, &status, &done);
    if (bad) return fail(status, std::string("rt_previous_positions_cpu: ") + bad);
    if (done) return RT_OK;
    if ((now->n_triangles && !now->triangles) || (now->n_spheres && !now->spheres))
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_previous_positions_cpu: null triangle or sphere array in the scene description");
    /* what rt_scene_create and rt_scene_update_vertices derive of a triangle, operation for operation (rt_api_layout.hip, rt_scene_update.hip) */
    std::vector<rt::DevTri> tris(now->n_triangles);
    std::vector<rt::DevSphere> spheres(now->n_spheres);
    std::vector<rt::MotionPiece> pieces(rt::motion_kept_pieces(now->n_triangles, now->n_spheres));
    for (uint32_t i = 0; i < now->n_triangles; ++i) {
        const rt_triangle &s = now->triangles[i];
        rt::DevTri &t = tris[i];
        memset(&t, 0, sizeof t);
        const V3 v0 = rt::v3p(s.vertices[0].position), v1 = rt::v3p(s.vertices[1].position), v2 = rt::v3p(s.vertices[2].position);
        const V3 nn = rt::normalize(rt::cross(v1 - v0, v2 - v1)); /* Triangle::face_normal, primitives.rs:36-42 */
        const V3 e0 = v2 - v1, e1 = v0 - v2, e2 = v1 - v0;        /* main.rs:219-221 */
        t.n[0] = nn.x; t.n[1] = nn.y; t.n[2] = nn.z;
        t.v0[0] = v0.x; t.v0[1] = v0.y; t.v0[2] = v0.z;
        t.v1[0] = v1.x; t.v1[1] = v1.y; t.v1[2] = v1.z;
        t.v2[0] = v2.x; t.v2[1] = v2.y; t.v2[2] = v2.z;
        t.e0[0] = e0.x; t.e0[1] = e0.y; t.e0[2] = e0.z;
        t.e1[0] = e1.x; t.e1[1] = e1.y; t.e1[2] = e1.z;
        t.e2[0] = e2.x; t.e2[1] = e2.y; t.e2[2] = e2.z;
        t.area = rt::dot(rt::cross(v1 - v0, v2 - v0), nn); /* main.rs:235 */
        for (uint32_t k = 0; k < RT_MOTION_TRI_PIECES; ++k) {
            const float *q = was_triangles + 9u * (size_t)i + 3u * k;
            pieces[(size_t)RT_MOTION_TRI_PIECES * i + k] = rt::MotionPiece{q[0], q[1], q[2], 0.0f};
        }
    }
    for (uint32_t i = 0; i < now->n_spheres; ++i) {
        const rt_sphere &s = now->spheres[i];
        rt::DevSphere &d = spheres[i];
        memset(&d, 0, sizeof d);
        d.c[0] = s.center[0]; d.c[1] = s.center[1]; d.c[2] = s.center[2];
        d.radius = s.radius;
        const float *q = was_spheres + 4u * (size_t)i;
        pieces[(size_t)RT_MOTION_TRI_PIECES * now->n_triangles + i] = rt::MotionPiece{q[0], q[1], q[2], q[3]};
    }
    each(rt::MotionRecords{{tris.data(), spheres.data(), pieces.data(), now->n_triangles, now->n_spheres}, hits, (uint64_t)n, was, was_stride});
    return RT_OK;
}

void rt_encode_srgb8(const float *rgb, size_t n_values, uint8_t *out) {
    if (!rgb || !out) return;
    for (size_t i = 0; i < n_values; ++i) {
        const float x = rgb[i];
        const float e = (x <= 0.0031308f) ? 12.92f * x : 1.055f * rtdm::powf(x, 1.0f / 2.4f) - 0.055f;
        /* palette 0.4 f32 -> u8: scale, clamp, truncating `as u8` (not rounding; the reference's
         * own output image pins this, see tests/test_oracle_reference_png.py) */
        float r = e * 255.0f;
        if (!(r > 0.0f)) r = 0.0f; /* also NaN -> 0 (saturating `as u8`) */
        if (r > 255.0f) r = 255.0f;
        out[i] = (uint8_t)r;
    }
}

static void put_be32(std::vector<uint8_t> &v, uint32_t x) {
    v.push_back((uint8_t)(x >> 24)); v.push_back((uint8_t)(x >> 16)); v.push_back((uint8_t)(x >> 8)); v.push_back((uint8_t)x);
}
static void put_chunk(std::vector<uint8_t> &png, const char type[4], const uint8_t *data, size_t n) {
    put_be32(png, (uint32_t)n);
    size_t start = png.size();
    png.insert(png.end(), type, type + 4);
    if (n) png.insert(png.end(), data, data + n);
    uint32_t crc = (uint32_t)crc32(0L, png.data() + start, (uInt)(png.size() - start));
    put_be32(png, crc);
}

/* main.rs:764-776: encode RGB8 PNG to a temporary file, then rename over the target */
int rt_write_png(const char *path, const uint8_t *rgb8, uint32_t width, uint32_t height) {
    if (!path || !rgb8 || width == 0 || height == 0) return fail(RT_ERR_INVALID_ARGUMENT, "rt_write_png: bad argument");
    std::vector<uint8_t> raw;
    raw.reserve((size_t)height * ((size_t)width * 3 + 1));
    for (uint32_t y = 0; y < height; ++y) {
        raw.push_back(0); /* filter type None */
        const uint8_t *row = rgb8 + (size_t)y * width * 3;
        raw.insert(raw.end(), row, row + (size_t)width * 3);
    }
    uLongf zn = compressBound((uLong)raw.size());
    std::vector<uint8_t> z(zn);
    if (compress2(z.data(), &zn, raw.data(), (uLong)raw.size(), 6) != Z_OK) return fail(RT_ERR_INVALID_ARGUMENT, "rt_write_png: deflate failed");
    std::vector<uint8_t> png;
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    png.insert(png.end(), sig, sig + 8);
    std::vector<uint8_t> ihdr;
    put_be32(ihdr, width);
    put_be32(ihdr, height);
    ihdr.push_back(8); /* bit depth */
    ihdr.push_back(2); /* colour type RGB */
    ihdr.push_back(0); ihdr.push_back(0); ihdr.push_back(0);
    put_chunk(png, "IHDR", ihdr.data(), ihdr.size());
    put_chunk(png, "IDAT", z.data(), zn);
    put_chunk(png, "IEND", nullptr, 0);
    std::string tmp = std::string(path) + ".tmp";
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) return fail(RT_ERR_INVALID_ARGUMENT, "rt_write_png: cannot create " + tmp + ": " + strerror(errno));
    size_t wr = fwrite(png.data(), 1, png.size(), f);
    if (fclose(f) != 0 || wr != png.size()) return fail(RT_ERR_INVALID_ARGUMENT, "rt_write_png: short write to " + tmp);
    if (rename(tmp.c_str(), path) != 0) return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_write_png: rename failed: ") + strerror(errno));
    return RT_OK;
}

} /* extern "C" */
