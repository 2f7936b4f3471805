/*
 * rt_texture_host.h — the texture queries on the CPU (include/rt_amd.h "texture queries" states every operation and the order; the
 * arithmetic is csrc/rt_texture.h's, shared with the device), for host arrays and no device.  Library: librt_host.so.
 * include/rt_host.h includes this header, so a program that includes that one has these too.  A header of its own for
 * include/rt_environment_host.h's reason: these take records and a pyramid, no image planes; Python lists them as
 * _capi.TEXTURE_HOST_SYMBOLS.
 *
 * The limits are the device calls' with the same texts and in the same order.  In a descriptor d_texels is a HOST pointer here.  A
 * failure returns a negative rt_status and sets rt_host_last_error().
 */
#ifndef RT_TEXTURE_HOST_H
#define RT_TEXTURE_HOST_H

#include <stddef.h>
#include <stdint.h>
#include "rt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rt_texture_pyramid, bit for bit: levels 1 .. n_levels - 1 of tex->d_texels from level 0, in place. */
int rt_texture_pyramid_cpu(const rt_texture *tex);
/* rt_texture_footprint, bit for bit, with the scene as its description (as rt_previous_positions_cpu takes it): the triangles'
 * vertices and uv and the spheres' radii are read from `scene`; width0: n floats or NULL for 0. */
int rt_texture_footprint_cpu(const rt_scene_desc *scene, const rt_hit *hits, const rt_ray *incoming, size_t n, float spread, const float *width0,
                             float *footprint);
/* rt_texture_sample, bit for bit, on host arrays. */
int rt_texture_sample_cpu(const rt_texture *tex, const float *uv, size_t uv_stride_words, const float *footprint, size_t n, float *out,
                          size_t out_stride_words);
/* rt_texture_surfaces, bit for bit: `surfaces` is edited in place. */
int rt_texture_surfaces_cpu(const rt_texture *diffuse_tex, const rt_texture *normal_tex, const rt_hit *hits, const float *footprint, size_t n,
                            uint32_t object_index, uint32_t flags, rt_surface *surfaces);

#ifdef __cplusplus
}
#endif
#endif /* RT_TEXTURE_HOST_H */
