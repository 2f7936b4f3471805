/*
 * rt_material_query.hip — the material at a hit, handed to the caller (include/rt_amd.h "material queries"): what every render and
 * query kernel evaluates between two casts and none returned — Material::approx(hit.at), ColorMaterial::adjust_normal(hit.at.normal)
 * and get_diffuse / get_specular on a MaterialProbe (materials.rs:33-66, 85-103) — so that a caller's own integrator gets albedo and
 * shading-normal planes, reads transparency or refraction_index where they depend on uv, and lights a hit from a direction that is no
 * rt_light of the scene, with the bits of get_shade.
 *
 *   rt::material_hits_kernel    main.rs:408-410 per record: approx and adjust_normal, as an rt_surface
 *   rt::probe_surfaces_kernel   materials.rs:46-66 per (probe, record): get_diffuse and get_specular, no light colour applied
 *
 * Nothing here is new arithmetic: hit_from_abi, material_approx, adjust_normal, get_diffuse and get_specular are called as
 * light_record() and light_terms() (rt_light_record.h) call them, with the same operands in the same order, and the unit is
 * compiled with -ffp-contract=off like every other — so every bit is rt_shade_hits'.  A surface is read back by that header's
 * surface_record, the one rt_light_terms_surfaces reads it with.  One record per lane, the record number counted in
 * 64 bits; a surface is read once per record, not once per pair; the probe loop is wave-uniform; per-(probe, record) arrays are
 * probe-major, entry p * n + i, as the light queries' are light-major.  Records move as dwords.  No LDS, no cast, no workspace.  The C
 * entry points of the block are at the end of the file.
 */
#include "rt_api_internal.h"
#include "rt_light_record.h" /* surface_record and RT_SURFACE_WORDS: the record as the other hit-sample units read it */

namespace rt {

#define RT_MATERIAL_THREADS 256u

/* main.rs:408-410: material = approx(hit.at), normal = adjust_normal(hit.at.normal) */
__global__ __launch_bounds__(RT_MATERIAL_THREADS) void material_hits_kernel(const KernelScene sc, const rt_hit *__restrict__ hits, const uint64_t n,
                                                                            rt_surface *__restrict__ surfaces) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_MATERIAL_THREADS + threadIdx.x;
    if (i >= n) return;
    uint32_t w[RT_SURFACE_WORDS];
#pragma unroll
    for (uint32_t k = 0; k < RT_SURFACE_WORDS; ++k) w[k] = 0u; /* "no hit": 18 zero words */
    const AbiHit h = hit_from_abi(hits + i, sc.n_triangles, sc.n_spheres, sc.n_materials, true);
    if (h.valid) {
        const Mat m = material_approx(sc.materials[h.g.obj], h.g.u, h.g.v);
        const V3 adj_n = adjust_normal(m.normal, h.g.normal); /* main.rs:410 */
        const float f[17] = {m.normal.x, m.normal.y, m.normal.z, m.diffuse.x, m.diffuse.y, m.diffuse.z, m.shiness, m.specular.x, m.specular.y, m.specular.z,
                             m.smoothness, m.transparency, m.refraction_index, m.opaque_decay, adj_n.x, adj_n.y, adj_n.z};
#pragma unroll
        for (uint32_t k = 0; k < 17u; ++k) w[k] = __float_as_uint(f[k]);
        w[17] = 1u;
    }
    uint32_t *const p = reinterpret_cast<uint32_t *>(surfaces + i);
#pragma unroll
    for (uint32_t k = 0; k < RT_SURFACE_WORDS; ++k) p[k] = w[k];
}

/* materials.rs:46-66 with probe = { normal: shading_normal, view_direction: view[i], light_direction: light_dirs[p * n + i] } */
__global__ __launch_bounds__(RT_MATERIAL_THREADS) void probe_surfaces_kernel(const rt_surface *__restrict__ surfaces, const uint64_t n,
                                                                             const float *__restrict__ view, const float *__restrict__ light_dirs,
                                                                             const uint32_t n_probes, float *__restrict__ diffuse_out,
                                                                             float *__restrict__ specular_out) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_MATERIAL_THREADS + threadIdx.x;
    if (i >= n) return;
    const SurfaceRecord s = surface_record(surfaces, i);
    const V3 view_direction = load_v3(view, i);
    for (uint32_t q = 0; q < n_probes; ++q) { /* wave-uniform */
        const uint64_t k = (uint64_t)q * n + i;
        V3 diffuse = v3(0.0f, 0.0f, 0.0f), specular = v3(0.0f, 0.0f, 0.0f);
        if (s.valid) { /* a record that is no hit stays out of get_specular's wave-level branch */
            const V3 light_direction = load_v3(light_dirs, k);
            diffuse = get_diffuse(s.m, s.adj_n, light_direction);
            specular = get_specular(s.m, s.adj_n, view_direction, light_direction);
        }
        store_v3(diffuse_out, k, diffuse);
        store_v3(specular_out, k, specular);
    }
}

} /* namespace rt */

/* ---- the C entry points (include/rt_amd.h "material queries") ---- */

/* rt_probe_surfaces' checks before any device work, in the documented order (no scene: the surface carries what the probe needs);
 * *done: nothing to launch */
static int probe_args(const char *who, size_t n, uint32_t n_probes, bool pointers_ok, bool *done) {
    return hit_sample_args(who, nullptr, HitSampleArgs(n, pointers_ok, "surface, view, light-direction, diffuse or specular").no_scene().probes(n_probes), done);
}

extern "C" {

int rt_material_hits(const rt_scene *scene, const rt_hit *d_hits, size_t n, rt_surface *d_surfaces, void *hip_stream) {
    bool done;
    const int rc = query_args("rt_material_hits", n, RECORDS_2_32, true, scene, d_hits && d_surfaces, "hit or surface", &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::material_hits_kernel, grid_of(n, RT_MATERIAL_THREADS), dim3(RT_MATERIAL_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks,
                       d_hits, (uint64_t)n, d_surfaces);
    return launched("rt_material_hits");
}

int rt_material_hits_host(const rt_scene *scene, const rt_hit *h_hits, size_t n, rt_surface *h_surfaces) {
    bool done;
    int rc = query_args("rt_material_hits_host", n, RECORDS_2_32, true, scene, h_hits && h_surfaces, "hit or surface", &done);
    if (rc != RT_OK || done) return rc;
    HostRoundTrip t("rt_material_hits_host");
    const rt_hit *d_hits = t.in(h_hits, n * sizeof(rt_hit));
    rt_surface *d_surfaces = t.out(h_surfaces, n * sizeof(rt_surface));
    if (!t.ok()) return t.failed();
    rc = rt_material_hits(scene, d_hits, n, d_surfaces, nullptr);
    return rc != RT_OK ? rc : t.finish();
}

int rt_probe_surfaces(const rt_surface *d_surfaces, size_t n, const float *d_view, const float *d_light_dirs, uint32_t n_probes, float *d_diffuse,
                      float *d_specular, void *hip_stream) {
    bool done;
    const int rc = probe_args("rt_probe_surfaces", n, n_probes, d_surfaces && d_view && d_light_dirs && d_diffuse && d_specular, &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::probe_surfaces_kernel, grid_of(n, RT_MATERIAL_THREADS), dim3(RT_MATERIAL_THREADS), 0, static_cast<hipStream_t>(hip_stream), d_surfaces,
                       (uint64_t)n, d_view, d_light_dirs, n_probes, d_diffuse, d_specular);
    return launched("rt_probe_surfaces");
}

int rt_probe_surfaces_host(const rt_surface *h_surfaces, size_t n, const float *h_view, const float *h_light_dirs, uint32_t n_probes, float *h_diffuse,
                           float *h_specular) {
    bool done;
    int rc = probe_args("rt_probe_surfaces_host", n, n_probes, h_surfaces && h_view && h_light_dirs && h_diffuse && h_specular, &done);
    if (rc != RT_OK || done) return rc;
    const size_t pair_bytes = n * (size_t)n_probes * 3u * sizeof(float);
    HostRoundTrip t("rt_probe_surfaces_host");
    const rt_surface *d_surfaces = t.in(h_surfaces, n * sizeof(rt_surface));
    const float *d_view = t.in(h_view, n * 3u * sizeof(float));
    const float *d_light_dirs = t.in(h_light_dirs, pair_bytes);
    float *d_diffuse = t.out(h_diffuse, pair_bytes);
    float *d_specular = t.out(h_specular, pair_bytes);
    if (!t.ok()) return t.failed();
    rc = rt_probe_surfaces(d_surfaces, n, d_view, d_light_dirs, n_probes, d_diffuse, d_specular, nullptr);
    return rc != RT_OK ? rc : t.finish();
}

} /* extern "C" */
