/*
 * rt_texture_query.hip — image textures on caller hits (include/rt_amd.h "texture queries"): the pyramid of a texture, the footprint
 * of a ray cone in uv space, the filtered lookup, the edit of rt_surface records, and get_shade's light terms on such records.
 *
 *   rt::texture_level_kernel           one destination texel of one level per lane, the source level read from global memory
 *   rt::texture_tail_kernel            one workgroup: every level from the first whose source is at most 32 x 32, level after level
 *                                      through two LDS buffers
 *   rt::texture_footprint_kernel       per record: the primitive's uv ratio from the scene's live vertices, and the cone's width
 *   rt::texture_sample_kernel          per record: the lookup, uv and output inside records of the caller's
 *   rt::texture_surfaces_kernel        per record: diffuse_color, normal and shading_normal of an rt_surface, in place
 *   rt::light_terms_surfaces_kernel    main.rs:435-459 per (record, light), the material and the bump normal read from an rt_surface
 *
 * The arithmetic of the first five is rt_texture.h's, shared with librt_host.so; the last is light_terms_kernel's loop
 * (rt_light_query.hip) around the same body (rt_light_record.h light_terms), on surface_record's material and normal.  One element
 * per lane, counted in 64 bits; records move as dwords; every index that addresses the scene is checked against its array first.  No atomics, no workspace.  The C entry points of the block
 * are at the end of the file.
 */
#include "rt_api_internal.h"
#include "rt_light_record.h"
#include "rt_texture.h"

namespace rt {

#define RT_TEX_THREADS 256u
static_assert(sizeof(rt_surface) == RT_TEX_SURFACE_WORDS * sizeof(uint32_t), "rt_surface is 18 dwords");
static_assert(sizeof(rt_hit) == RT_TEX_HIT_WORDS * sizeof(uint32_t), "rt_hit is 13 dwords");
static_assert(sizeof(rt_ray) == RT_TEX_RAY_WORDS * sizeof(uint32_t), "rt_ray is 11 dwords");

/* level `level` from level - 1, both in global memory */
__global__ __launch_bounds__(RT_TEX_THREADS) void texture_level_kernel(const TexView t, float *__restrict__ texels, const uint32_t level) {
    const uint32_t w = tex_extent(t.width, level), h = tex_extent(t.height, level);
    const uint64_t k = (uint64_t)blockIdx.x * RT_TEX_THREADS + threadIdx.x;
    if (k >= (uint64_t)w * h) return;
    const uint32_t y = (uint32_t)(k / w), x = (uint32_t)(k - (uint64_t)y * w);
    const TexLevel src = {t.texels + 3u * (uint64_t)t.start[level - 1u], tex_extent(t.width, level - 1u), tex_extent(t.height, level - 1u)};
    const V3 value = tex_reduce(src, x, y);
    float *const out = texels + 3u * ((uint64_t)t.start[level] + k);
    out[0] = value.x;
    out[1] = value.y;
    out[2] = value.z;
}

/* levels first .. n_levels - 1; the source of `first` is at most RT_TEX_SMALL each way.  Level l is computed from the f32 values of
 * level l - 1 held in LDS — the values the level kernel would read back from memory */
__global__ __launch_bounds__(RT_TEX_THREADS) void texture_tail_kernel(const TexView t, float *__restrict__ texels, const uint32_t first) {
    __shared__ float held[2][RT_TEX_SMALL * RT_TEX_SMALL * 3u];
    uint32_t sw = tex_extent(t.width, first - 1u), sh = tex_extent(t.height, first - 1u);
    const float *const from = t.texels + 3u * (uint64_t)t.start[first - 1u];
    for (uint32_t k = threadIdx.x; k < sw * sh * 3u; k += RT_TEX_THREADS) held[0][k] = from[k];
    __syncthreads();
    uint32_t cur = 0u;
    for (uint32_t level = first; level < t.n_levels; ++level) { /* workgroup-uniform */
        const uint32_t w = tex_extent(t.width, level), h = tex_extent(t.height, level);
        const TexLevel src = {held[cur], sw, sh};
        float *const out = texels + 3u * (uint64_t)t.start[level];
        for (uint32_t k = threadIdx.x; k < w * h; k += RT_TEX_THREADS) {
            const uint32_t y = k / w, x = k - y * w;
            const V3 value = tex_reduce(src, x, y);
            held[cur ^ 1u][3u * k] = out[3u * k] = value.x;
            held[cur ^ 1u][3u * k + 1u] = out[3u * k + 1u] = value.y;
            held[cur ^ 1u][3u * k + 2u] = out[3u * k + 2u] = value.z;
        }
        __syncthreads();
        cur ^= 1u;
        sw = w, sh = h;
    }
}

__global__ __launch_bounds__(RT_TEX_THREADS) void texture_footprint_kernel(const KernelScene sc, const rt_hit *__restrict__ hits,
                                                                           const rt_ray *__restrict__ incoming, const uint64_t n, const float spread,
                                                                           const float *__restrict__ width0, float *__restrict__ footprint) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_TEX_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t *const hit = reinterpret_cast<const uint32_t *>(hits + i);
    const uint32_t kind = hit[0], index = hit[1];
    const bool valid = kind <= 1u && hit[RT_TEX_HIT_OBJECT] < sc.n_materials; /* the hit queries' "no hit" */
    float ratio = 0.0f;
    bool ok = false;
    if (valid && kind == 1u && index < sc.n_triangles) {
        const DevTri &T = sc.tris[index];
        const DevTriAttr &A = sc.attrs[index];
        ratio = tex_triangle_ratio(v3p(T.v0), v3p(T.v1), v3p(T.v2), A.uv0x, A.uv0y, A.uv1x, A.uv1y, A.uv2x, A.uv2y, &ok);
    } else if (valid && kind == 0u && index < sc.n_spheres) {
        ratio = tex_sphere_ratio(sc.spheres[index].radius, &ok);
    }
    footprint[i] = tex_footprint_record(hit, reinterpret_cast<const uint32_t *>(incoming + i), width0 != nullptr ? width0[i] : 0.0f, spread, ratio, ok);
}

__global__ __launch_bounds__(RT_TEX_THREADS) void texture_sample_kernel(const TexSample a) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_TEX_THREADS + threadIdx.x;
    if (i >= a.n) return;
    tex_sample_record(a, i);
}

__global__ __launch_bounds__(RT_TEX_THREADS) void texture_surfaces_kernel(const TexSurfaces a) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_TEX_THREADS + threadIdx.x;
    if (i >= a.n) return;
    tex_surface_record(a, i);
}

/* light_terms_kernel (rt_light_query.hip) with the material and the normal of the surface record, which probe_surfaces_kernel reads
 * with the same surface_record */
__global__ __launch_bounds__(RT_LIGHT_THREADS) void light_terms_surfaces_kernel(const KernelScene sc, const rt_surface *__restrict__ surfaces,
                                                                                const rt_hit *__restrict__ hits, const rt_ray *__restrict__ incoming,
                                                                                const uint64_t n, const uint32_t light_first, const uint32_t light_count,
                                                                                const unsigned char *__restrict__ asks,
                                                                                const rt_hit *__restrict__ shadow_hits, unsigned char *__restrict__ lit_out,
                                                                                float *__restrict__ diffuse_out, float *__restrict__ specular_out) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_LIGHT_THREADS + threadIdx.x;
    if (i >= n) return;
    const AbiHit h = hit_from_abi(hits + i, sc.n_triangles, sc.n_spheres, sc.n_materials, true);
    const bool valid = h.valid && surface_flag(surfaces, i);
    SurfaceRecord s; /* "no hit": the flag word alone is read of such a record */
    V3 pos = v3(0.0f, 0.0f, 0.0f), view = v3(0.0f, 0.0f, 1.0f);
    if (valid) {
        s = surface_record(surfaces, i);
        pos = h.g.pos;
        view = ray_from_abi(incoming + i, sc.n_triangles, sc.n_spheres).d; /* hit.ray.direction */
    }
    for (uint32_t l = 0; l < light_count; ++l) { /* wave-uniform */
        const uint64_t k = (uint64_t)l * n + i;
        const bool asked = valid && asks[k] != 0;
        LightTerms t; /* not lit, +0 */
        if (__builtin_amdgcn_ballot_w64(asked) != 0ull) { /* a wave nobody asks in skips the light: its acosf and powf are binary64 */
            const auto &L = uniform_ref(sc.lights + (light_first + l));
            t = light_terms(L, area_light_has_origin(L), v3(L.origin[0], L.origin[1], L.origin[2]), pos, s.m, s.adj_n, view, asked, shadow_hits + k);
        }
        store_light_terms(lit_out, diffuse_out, specular_out, k, t);
    }
}

} /* namespace rt */

/* ---- the C entry points (include/rt_amd.h "texture queries") ---- */

static int check_texture(const char *who, const rt_texture *tex) { return check_descriptor(who, tex, rt::texture_limits); }

extern "C" {

uint32_t rt_texture_levels(uint32_t width, uint32_t height) { return rt::tex_levels(width, height); }

size_t rt_texture_pyramid_floats(uint32_t width, uint32_t height, uint32_t n_levels) { return (size_t)rt::tex_pyramid_floats(width, height, n_levels); }

int rt_texture_pyramid(const rt_texture *tex, void *hip_stream) {
    const char *const who = "rt_texture_pyramid";
    int rc = check_texture(who, tex);
    if (rc != RT_OK) return rc;
    const rt::TexView t = rt::tex_view(*tex);
    float *const texels = const_cast<float *>(tex->d_texels);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    for (uint32_t level = 1u; level < t.n_levels; ++level) {
        if (rt::tex_extent(t.width, level - 1u) <= RT_TEX_SMALL && rt::tex_extent(t.height, level - 1u) <= RT_TEX_SMALL) {
            hipLaunchKernelGGL(rt::texture_tail_kernel, dim3(1), dim3(RT_TEX_THREADS), 0, stream, t, texels, level);
            return launched(who);
        }
        const uint64_t count = (uint64_t)rt::tex_extent(t.width, level) * rt::tex_extent(t.height, level);
        hipLaunchKernelGGL(rt::texture_level_kernel, grid_of(count, RT_TEX_THREADS), dim3(RT_TEX_THREADS), 0, stream, t, texels, level);
        rc = launched(who);
        if (rc != RT_OK) return rc;
    }
    return RT_OK;
}

int rt_texture_footprint(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, float spread, const float *d_width0,
                         float *d_footprint, void *hip_stream) {
    const char *const who = "rt_texture_footprint";
    bool done;
    const int rc = query_args(who, n, RECORDS_2_32, true, scene, d_hits && d_incoming && d_footprint, "hit, incoming-ray or footprint", &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::texture_footprint_kernel, grid_of(n, RT_TEX_THREADS), dim3(RT_TEX_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks,
                       d_hits, d_incoming, (uint64_t)n, spread, d_width0, d_footprint);
    return launched(who);
}

int rt_texture_sample(const rt_texture *tex, const float *d_uv, size_t uv_stride_words, const float *d_footprint, size_t n, float *d_out,
                      size_t out_stride_words, void *hip_stream) {
    const char *const who = "rt_texture_sample";
    int rc = check_count(who, n, RECORDS_2_32);
    if (rc == RT_OK) rc = check_texture(who, tex);
    if (rc != RT_OK || n == 0) return rc;
    rc = check_pointers(who, d_uv && d_out, "uv or output");
    if (rc != RT_OK) return rc;
    if (const char *bad = rt::tex_stride_limits(uv_stride_words, out_stride_words)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + bad);
    const rt::TexSample a = {rt::tex_view(*tex), d_uv, (uint64_t)uv_stride_words, d_footprint, (uint64_t)n, d_out, (uint64_t)out_stride_words};
    hipLaunchKernelGGL(rt::texture_sample_kernel, grid_of(n, RT_TEX_THREADS), dim3(RT_TEX_THREADS), 0, static_cast<hipStream_t>(hip_stream), a);
    return launched(who);
}

int rt_texture_surfaces(const rt_texture *diffuse_tex, const rt_texture *normal_tex, const rt_hit *d_hits, const float *d_footprint, size_t n,
                        uint32_t object_index, uint32_t flags, rt_surface *d_surfaces, void *hip_stream) {
    const char *const who = "rt_texture_surfaces";
    int rc = check_count(who, n, RECORDS_2_32);
    if (rc == RT_OK && diffuse_tex) rc = check_texture(who, diffuse_tex);
    if (rc == RT_OK && normal_tex) rc = check_texture(who, normal_tex);
    if (rc != RT_OK || n == 0) return rc;
    rc = check_pointers(who, d_hits && d_surfaces, "hit or surface");
    if (rc != RT_OK) return rc;
    if (const char *bad = rt::tex_surface_limits(flags)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + bad);
    if (!diffuse_tex && !normal_tex) return RT_OK;
    rt::TexSurfaces a = {};
    if (diffuse_tex) a.diffuse = rt::tex_view(*diffuse_tex);
    if (normal_tex) a.normal = rt::tex_view(*normal_tex);
    a.has_diffuse = diffuse_tex != nullptr, a.has_normal = normal_tex != nullptr;
    a.hits = reinterpret_cast<const uint32_t *>(d_hits);
    a.footprint = d_footprint;
    a.n = (uint64_t)n;
    a.object_index = object_index, a.flags = flags;
    a.surfaces = reinterpret_cast<uint32_t *>(d_surfaces);
    hipLaunchKernelGGL(rt::texture_surfaces_kernel, grid_of(n, RT_TEX_THREADS), dim3(RT_TEX_THREADS), 0, static_cast<hipStream_t>(hip_stream), a);
    return launched(who);
}

/* rt_light_terms' checks (hit_sample_args, rt_api_internal.h), with the surfaces among the pointers */
int rt_light_terms_surfaces(const rt_scene *scene, const rt_surface *d_surfaces, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n,
                            uint32_t light_first, uint32_t light_count, const unsigned char *d_asks, const rt_hit *d_shadow_hits,
                            unsigned char *d_lit, float *d_diffuse, float *d_specular, void *hip_stream) {
    const char *const who = "rt_light_terms_surfaces";
    bool done;
    const int rc = hit_sample_args(who, scene,
                                   HitSampleArgs(n, d_surfaces && d_hits && d_incoming && d_asks && d_shadow_hits && d_lit && d_diffuse && d_specular,
                                                 "surface, hit, incoming-ray, flag, shadow-hit, lit, diffuse or specular")
                                       .lights(light_count, light_first), &done);
    if (rc != RT_OK || done) return rc;
    hipLaunchKernelGGL(rt::light_terms_surfaces_kernel, grid_of(n, RT_LIGHT_THREADS), dim3(RT_LIGHT_THREADS), 0, static_cast<hipStream_t>(hip_stream), scene->ks,
                       d_surfaces, d_hits, d_incoming, (uint64_t)n, light_first, light_count, d_asks, d_shadow_hits, d_lit, d_diffuse, d_specular);
    return launched(who);
}

} /* extern "C" */
