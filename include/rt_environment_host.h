/*
 * rt_environment_host.h — the environment queries on the CPU (include/rt_amd.h "environment queries" states every operation and the
 * order; the arithmetic is csrc/rt_environment.h's, shared with the device), for host arrays and no device.  Library: librt_host.so.
 * include/rt_host.h includes this header, so a program that includes that one has these too.
 *
 * Why a header of its own: an rt_X_cpu declared in rt_host.h is, by the convention of the image-side queries, the CPU definition of a
 * device entry point rt_X on image planes, and the suite holds every such pair to one guard-band table of image operands.  These four
 * take records, a table and hit-side arrays; rt_environment_samples_cpu has no device call of its name (it is rt_environment_rays
 * without the scene), and the block's guard-band checks live in its own suite (tests/test_gpu_environment.py).  Python lists them as
 * _capi.ENVIRONMENT_HOST_SYMBOLS.
 *
 * The limits are the device calls' with the same texts: the counts (RT_ERR_UNSUPPORTED), the descriptor, n == 0 is RT_OK, a null
 * required pointer, then spp (and pattern).  A failure returns a negative rt_status and sets rt_host_last_error().
 */
#ifndef RT_ENVIRONMENT_HOST_H
#define RT_ENVIRONMENT_HOST_H

#include <stddef.h>
#include <stdint.h>
#include "rt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rt_environment_lookup, bit for bit, on host arrays: env->d_texels is a host pointer here, count a host u32 or NULL. */
int rt_environment_lookup_cpu(const rt_environment *env, const rt_ray *rays, size_t n, const uint32_t *count, const rt_hit *hits, const uint32_t *parent,
                              float *out, size_t n_out);
/* rt_environment_table, every word: table holds rt_environment_table_bytes(width, height) bytes, 8-byte aligned. */
int rt_environment_table_cpu(const rt_environment *env, void *table);
/* What rt_environment_rays writes into d_dirs, d_radiance, d_texel and d_asks for hits whose normal N is normals[3i ..], bit for bit,
 * k = s * n + i.  It evaluates no material and knows no "no hit", as rt_hemisphere_dirs_cpu: for RT_HEMISPHERE_SHADING pass
 * rt_material_hits' shading_normal.  ids: n u32 or NULL for id = i; texel and asks may be NULL. */
int rt_environment_samples_cpu(const rt_environment *env, const void *table, const float *normals, const uint32_t *ids, size_t n, uint32_t spp,
                               uint32_t pattern, uint32_t seed, float *dirs, float *radiance, uint32_t *texel, unsigned char *asks);
/* rt_environment_fold, bit for bit, with what the device reads from the scene as plain arrays: valid (n bytes: the record is a hit)
 * and shiness (n floats); the other arrays as the device call's, NULL where it allows NULL. */
int rt_environment_fold_cpu(const unsigned char *valid, const float *shiness, size_t n, uint32_t spp, const unsigned char *asks, const rt_hit *shadow_hits,
                            const float *radiance, const float *diffuse, const float *specular, unsigned char *open, float *rgb);

#ifdef __cplusplus
}
#endif
#endif /* RT_ENVIRONMENT_HOST_H */
