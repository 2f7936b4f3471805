/*
 * rt_host.h — host side of the render path: what stays on the CPU on either
 * side of the C-ABI render call.
 *
 * The reference is a single Rust binary; there is no Rust toolchain in the
 * build image, so the host side is C++ behind these C entry points, mirroring
 * the reference's builder API by name:
 *
 *   World::new / push_object / push_light        src/main.rs:160-178
 *   ObjectProxy::push_triangle(s) / push_sphere  src/main.rs:700-728
 *   triangle() / square() flat-normal helpers    src/main.rs:730-746
 *   load_obj                                     src/main.rs:778-807
 *   the literal scene and camera of main()       src/main.rs:810-1083
 *   (the same scene as a file: rt_world_save_scene / rt_world_load_scene)
 *   post_process                                 src/main.rs:748-762
 *   Image::<Srgb<u8>>::convert_from              src/image.rs:55-66
 *   write_to_file (tmp file + rename)            src/main.rs:764-776
 *
 * Library: librt_host.so (no HIP dependency).
 */
#ifndef RT_HOST_H
#define RT_HOST_H

#include <stddef.h>
#include <stdint.h>
#include "rt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_world rt_world; /* host-side World under construction */

rt_world *rt_world_new(void);
void rt_world_free(rt_world *world);

/* World::push_object: returns the new ObjectIndex (>= 0) or a negative rt_status. */
int rt_world_push_object(rt_world *world, const rt_material *material);
/* ObjectProxy::push_triangle / push_sphere */
int rt_world_push_triangle(rt_world *world, uint32_t object_index, const rt_vertex vertices[3]);
int rt_world_push_sphere(rt_world *world, uint32_t object_index, const float center[3], float radius);
/* World::push_light */
int rt_world_push_light(rt_world *world, const rt_light *light);

/* triangle(): positions[9] = 3 x xyz, uvs[6] = 3 x uv; the vertex normal of all
 * three vertices is normalize((v1-v0) x (v2-v1)). */
int rt_world_push_flat_triangle(rt_world *world, uint32_t object_index, const float positions[9], const float uvs[6]);
/* square(): 4 corners -> triangles (0,1,2) and (0,2,3). */
int rt_world_push_square(rt_world *world, uint32_t object_index, const float positions[12], const float uvs[8]);

/* load_obj: first model only, `v` and triangular `f` records, no vn/vt; every
 * position becomes p / divisor + offset (the reference uses 3.0 and
 * (0.7, 1.0, -0.5)); uv = (0,0); flat normals via triangle().  Returns the
 * number of triangles pushed or a negative rt_status. */
int rt_world_load_obj(rt_world *world, uint32_t object_index, const char *path, float divisor, const float offset[3]);

/* The whole literal scene of main(): 9 objects, 64 triangles, 4 spheres,
 * 3 lights.  obj_path is the dodecahedron.obj to import. */
int rt_world_build_reference_scene(rt_world *world, const char *obj_path);
/* Camera literal of main.rs:1077-1083. */
void rt_reference_camera(rt_camera *out);

/* View of the world's arrays (valid until the next push / free). */
void rt_world_desc(const rt_world *world, rt_scene_desc *out);

/* The scene as a data format: one flat little-endian file — a 128-byte header ("RTSCENE", version,
 * counts, record sizes, optionally the camera) followed by the arrays of rt_scene_desc exactly as declared in rt_amd.h,
 * in the order materials, triangles, spheres, lights; array order is preserved (it is semantically significant).
 * rt_world_save_scene writes "<path>.tmp" and renames it over path.  rt_world_load_scene REPLACES the world's contents
 * (only if the whole file is valid: magic, version, byte order, record sizes, file length, index and enum ranges);
 * *out_camera is filled and *out_has_camera set when the file carries a camera (both may be NULL). */
int rt_world_save_scene(const rt_world *world, const rt_camera *camera_or_null, const char *path);
int rt_world_load_scene(rt_world *world, const char *path, rt_camera *out_camera, int *out_has_camera);

/* Full-frame rt_frame helper: tile = whole image. */
void rt_frame_full(uint32_t width, uint32_t height, int32_t max_depth, rt_frame *out);

/* post_process: divide the image by the 99th-percentile luma (in place).
 * Returns the divisor used, 0 when the image has no normal luma (the reference
 * panics there, main.rs:754; this returns instead) or the percentile is
 * <= f32::EPSILON (image left untouched, main.rs:755). */
float rt_post_process(float *rgb, size_t n_pixels);
/* its luma weights: luma = (row3[0] * r + row3[1] * g) + row3[2] * b (palette 0.4, LinSrgb::into_luma via main.rs:750) */
void rt_luma_row(float *row3);

/* Linear f32 -> sRGB-encoded u8 (n_values = 3 * pixels). */
void rt_encode_srgb8(const float *rgb, size_t n_values, uint8_t *out);

/* PhotonAccumulator (src/photon.rs:9-34; defined but never used by the reference's main(): SURVEY §8f-4) — a true
 * running average as the alternative to main()'s sum-and-renormalise.  `sum` (3 f32 per pixel) and `weight` (1 f32 per
 * pixel) start at zero.  rt_accumulate applies accumulate() — sum = sum + photon, weight_sum += 1.0 — for every sample
 * whose filter flag is set (`samples`, `valid`: the n_epochs x n_pixels outputs of rt_render_distributed), in epoch
 * order; rt_accumulator_resolve is into_rgb_internal: black while weight < f32::EPSILON, else sum / weight. */
void rt_accumulate(const float *samples, const uint8_t *valid, uint32_t n_epochs, size_t n_pixels, float *sum, float *weight);
void rt_accumulator_resolve(const float *sum, const float *weight, size_t n_pixels, float *rgb);

/* The film queries' CPU definition (include/rt_amd.h "film queries": patterns, the hash, the filters and the order are stated there):
 * plain loops over host arrays, bit-identical to rt_film_offsets / rt_film_splat of librt_amd.so.  Same arguments without the stream,
 * same checks; a failure returns a negative rt_status and sets rt_host_last_error(). */
int rt_film_offsets_host(const rt_frame *frame, uint32_t spp, uint32_t pattern, uint32_t seed, float *offsets);
int rt_film_splat_host(uint32_t rows, uint32_t cols, const float *samples, const uint8_t *valid, const float *offsets, uint32_t spp,
                       uint32_t filter, float radius, float *sum, float *weight);

/* The denoise queries' CPU definition (include/rt_amd.h "denoise queries" states every operation and the order): the plain nested loops
 * over host arrays, no device needed, bit-identical to rt_denoise_atrous of librt_amd.so.  Same arguments without the stream, same
 * checks with the same messages; a failure returns a negative rt_status and sets rt_host_last_error().  It is called _cpu, not _host as
 * the film's CPU forms are, because librt_amd.so already exports rt_denoise_atrous_host: that one is the round trip through the
 * KERNELS on host buffers, this one the definition they are tested against. */
int rt_denoise_atrous_cpu(const float *color, const rt_denoise_guides *guides, const rt_denoise_params *params, uint32_t rows, uint32_t cols,
                          float *out, float *temp);

/* The temporal queries' CPU definition (include/rt_amd.h "temporal queries" states every operation and the order): plain loops over
 * host arrays, no device needed, bit-identical to rt_temporal_motion / rt_temporal_accumulate of librt_amd.so.  Same arguments without
 * the stream, same checks with the same messages (the history arrays need no alignment here); a failure returns a negative rt_status
 * and sets rt_host_last_error().  Called _cpu for the reason rt_denoise_atrous_cpu is: the _host names are librt_amd.so's round trips
 * through the kernels. */
int rt_temporal_motion_cpu(const float *position, uint32_t position_stride, const uint32_t *valid, uint32_t valid_stride,
                           const rt_camera *prev_camera, const rt_frame *prev_frame, float *motion);
int rt_temporal_accumulate_cpu(const float *color, const float *motion, const rt_temporal_guides *current, const rt_temporal_guides *previous,
                               const rt_temporal_params *params, uint32_t rows, uint32_t cols, const rt_temporal_pixel *history_in,
                               rt_temporal_pixel *history_out, float *variance);

/* The history rectification queries' CPU definition (include/rt_amd.h "history rectification queries" states every operation and the
 * order): plain loops over host arrays, no device needed, bit-identical to rt_temporal_bounds / rt_temporal_accumulate_bounded /
 * rt_temporal_feedback of librt_amd.so.  Same arguments without the stream, same checks with the same messages (no array needs an
 * alignment here); a failure returns a negative rt_status and sets rt_host_last_error().  Called _cpu for the reason
 * rt_denoise_atrous_cpu is. */
int rt_temporal_bounds_cpu(const float *color, uint32_t color_stride, const uint32_t *object, uint32_t object_stride, const uint32_t *valid,
                           uint32_t valid_stride, const rt_bounds_params *params, uint32_t rows, uint32_t cols, rt_temporal_box *box);
int rt_temporal_accumulate_bounded_cpu(const float *color, const float *motion, const rt_temporal_guides *current, const rt_temporal_guides *previous,
                                       const rt_temporal_params *params, uint32_t rows, uint32_t cols, const rt_temporal_pixel *history_in,
                                       rt_temporal_pixel *history_out, float *variance, const rt_temporal_box *box, uint32_t clamped_length,
                                       uint32_t *clamped);
int rt_temporal_feedback_cpu(const float *color, uint32_t color_stride, const uint32_t *valid, uint32_t valid_stride, uint32_t rows,
                             uint32_t cols, rt_temporal_pixel *history);

/* The guided upsampling queries' CPU definition (include/rt_amd.h "guided upsampling queries" states every operation and the order): a
 * plain loop over host arrays, no device needed, bit-identical to rt_upsample_guided of librt_amd.so.  Same arguments without the
 * stream, same checks with the same messages; a failure returns a negative rt_status and sets rt_host_last_error().  Called _cpu for
 * the reason rt_denoise_atrous_cpu is. */
int rt_upsample_guided_cpu(const float *color_lo, uint32_t color_stride, const rt_denoise_guides *low, const uint32_t *object_lo,
                           uint32_t object_lo_stride, const rt_denoise_guides *full, const uint32_t *object_full, uint32_t object_full_stride,
                           const rt_upsample_params *params, uint32_t rows, uint32_t cols, float *out);

/* The bloom queries' CPU definition (include/rt_amd.h "bloom queries" states every operation and the order): plain loops over host
 * arrays, no device needed, bit-identical to rt_bloom of librt_amd.so.  Same arguments without the stream — temp is the caller's scratch
 * of rt_bloom_temp_bytes bytes —, same checks with the same messages; a failure returns a negative rt_status and sets
 * rt_host_last_error().  Called _cpu for the reason rt_denoise_atrous_cpu is. */
int rt_bloom_cpu(const float *color, uint32_t color_stride, const rt_bloom_params *params, uint32_t rows, uint32_t cols, float *temp, float *out);

/* The adaptive sampling queries' CPU definition (include/rt_amd.h "adaptive sampling queries" states every operation and the order): plain
 * loops over host arrays, no device needed, bit-identical to rt_sample_budget / rt_sample_list / rt_film_offsets_listed /
 * rt_camera_rays_listed / rt_film_splat_listed of librt_amd.so.  Same arguments without the stream (and, for the list, without the
 * scratch), same checks with the same messages; a failure returns a negative rt_status and sets rt_host_last_error().  Called _cpu for
 * the reason rt_denoise_atrous_cpu is. */
int rt_sample_budget_cpu(const float *mean, uint32_t mean_stride, const float *variance, uint32_t variance_stride, const uint32_t *count,
                         uint32_t count_stride, const uint32_t *valid, uint32_t valid_stride, const rt_sample_budget_params *params, size_t n,
                         uint32_t *budget);
int rt_sample_list_cpu(const uint32_t *counts, size_t n, size_t capacity, uint32_t *first, uint32_t *start, uint32_t *pixel, uint32_t *sample,
                       uint32_t *total);
int rt_film_offsets_listed_cpu(const rt_frame *frame, uint32_t pattern, uint32_t seed, const uint32_t *pixel, const uint32_t *sample,
                               const uint32_t *total, size_t capacity, float *offsets);
int rt_camera_rays_listed_cpu(const rt_camera *camera, const rt_frame *frame, const float *offsets, const uint32_t *pixel, const uint32_t *total,
                              size_t capacity, rt_ray *rays);
int rt_film_splat_listed_cpu(uint32_t rows, uint32_t cols, const float *samples, const uint8_t *valid, const float *offsets, const uint32_t *start,
                             size_t capacity, uint32_t max_count, uint32_t filter, float radius, float *sum, float *weight);

/* The motion queries' CPU definition (include/rt_amd.h "motion queries" states every operation and the order): a plain loop over host
 * arrays, no device needed, bit-identical to rt_previous_positions of librt_amd.so.  `now` is the description of the scene as it stands
 * (what the hits were cast on); was_triangles holds 9 f32 per triangle — the kept x y z of vertices 0, 1, 2 — and was_spheres 4 per
 * sphere, cx cy cz r: what rt_scene_keep_positions would have kept, i.e. the description before the update.  n, e0..e2 and area are
 * derived from now's vertices operation for operation as rt_scene_create and rt_scene_update_vertices derive them.  Same checks in the
 * same order with the same texts; in the place of "never kept", a null was_triangles with n_triangles > 0 or a null was_spheres with
 * n_spheres > 0 is RT_ERR_INVALID_ARGUMENT.  A failure returns a negative rt_status and sets rt_host_last_error(). */
int rt_previous_positions_cpu(const rt_scene_desc *now, const float *was_triangles, const float *was_spheres, const rt_hit *hits, size_t n,
                              float *was, uint32_t was_stride);

/* The variance-guided filter queries' CPU definition (include/rt_amd.h "variance-guided filter queries" states every operation and the
 * order): plain loops over host arrays, no device needed, bit-identical to rt_svgf_variance / rt_svgf_atrous of librt_amd.so.  Same
 * arguments without the stream (the history needs no alignment here; temp: rt_svgf_temp_bytes bytes, or NULL for one level), same
 * checks; a refusal returns RT_ERR_INVALID_ARGUMENT and sets rt_host_last_error().  Called _cpu for the reason rt_denoise_atrous_cpu is. */
int rt_svgf_variance_cpu(const rt_temporal_pixel *history, const rt_denoise_guides *guides, const rt_svgf_variance_params *params, uint32_t rows,
                         uint32_t cols, float *variance_out);
int rt_svgf_atrous_cpu(const float *color, uint32_t color_stride, const float *variance, const rt_denoise_guides *guides,
                       const rt_svgf_atrous_params *params, uint32_t rows, uint32_t cols, float *out, float *variance_out, void *temp);

/* The area-light queries' sampler on the CPU (include/rt_amd.h "area-light queries" states every operation and the order; the
 * arithmetic is csrc/rt_area_light.h's, shared with the device): sample[3k ..] of rt_area_light_rays, bit for bit, for host arrays and
 * no device.  lights: the scene's lights (light_first + light_count of them are read); radii: light_count floats; ids: n u32 or NULL for
 * id = i; sample: spp * light_count * n * 3 floats, entry k = (s * light_count + (l - light_first)) * n + i.  The casts and the Phong
 * terms have no CPU form: their oracle is the light queries on a scene whose lights were moved to these samples.  The limits are
 * rt_area_light_rays' with the same texts: the three counts (RT_ERR_UNSUPPORTED), n == 0 or light_count == 0 is RT_OK, a null lights,
 * radii or sample pointer, then spp and pattern.  A failure returns a negative rt_status and sets rt_host_last_error(). */
int rt_area_light_samples_cpu(const rt_light *lights, uint32_t light_first, uint32_t light_count, const float *radii, const uint32_t *ids, size_t n,
                              uint32_t spp, uint32_t pattern, uint32_t seed, float *sample);

/* The hemisphere queries on the CPU (include/rt_amd.h "hemisphere queries" states every operation and the order; the arithmetic is
 * csrc/rt_hemisphere.h's, shared with the device), for host arrays and no device.
 * rt_hemisphere_dirs_cpu: dirs[3k ..] of rt_hemisphere_rays, bit for bit, k = s * n + i, for the normals it is given — n * 3 floats,
 * the N of each record; it evaluates no material and knows no "no hit".  ids: n u32 or NULL for id = i.
 * rt_hemisphere_fold_cpu: rt_hemisphere_fold, bit for bit, with what the device reads from the scene as plain arrays: valid (n bytes:
 * the record is a hit), diffuse_color (n * 3 floats) and shiness (n floats), read only where rgb is given; hits: the records, of which
 * the position is read; shadow_hits, radiance, open, ambient and rgb as the device call's, NULL where it allows NULL.
 * The limits are the device calls' with the same texts: the counts (RT_ERR_UNSUPPORTED), n == 0 is RT_OK, a null required pointer, then
 * spp (and pattern).  A failure returns a negative rt_status and sets rt_host_last_error(). */
int rt_hemisphere_dirs_cpu(const float *normals, const uint32_t *ids, size_t n, uint32_t spp, uint32_t pattern, uint32_t seed, float *dirs);
int rt_hemisphere_fold_cpu(const rt_hit *hits, const unsigned char *valid, const float *diffuse_color, const float *shiness, size_t n, uint32_t spp,
                           const unsigned char *asks, const rt_hit *shadow_hits, float max_distance, const float *radiance, unsigned char *open,
                           float *ambient, float *rgb);

/* The environment queries on the CPU — rt_environment_lookup_cpu, rt_environment_table_cpu, rt_environment_samples_cpu and
 * rt_environment_fold_cpu, exported by librt_host.so like everything above — are declared in a header of their own, included at the end
 * of this one.  That header says why. */

/* RGB8 PNG, written to "<path>.tmp" then renamed over path. */
int rt_write_png(const char *path, const uint8_t *rgb8, uint32_t width, uint32_t height);

const char *rt_host_last_error(void);

#ifdef __cplusplus
}
#endif
#include "rt_environment_host.h"
#include "rt_lobe_host.h"
#include "rt_path_host.h"
#include "rt_connect_host.h"
#include "rt_light_connect_host.h"
#include "rt_texture_host.h"
#endif /* RT_HOST_H */
