/*
 * rt_path_host.h — the path queries on the CPU (include/rt_amd.h "path queries" states every operation and the order; the arithmetic
 * is csrc/rt_path.h's, shared with the device), for host arrays and no device.  Library: librt_host.so.  include/rt_host.h includes this
 * header, so a program that includes that one has these too.  A header of its own for include/rt_lobe_host.h's reason: these take
 * records and per-path arrays, no image planes; Python lists them as _capi.PATH_HOST_SYMBOLS.
 *
 * The limits are the device calls' with the same texts: the counts (RT_ERR_UNSUPPORTED), an empty batch is RT_OK, a null required
 * pointer, then spp or rr_floor.  A failure returns a negative rt_status and sets rt_host_last_error().
 */
#ifndef RT_PATH_HOST_H
#define RT_PATH_HOST_H

#include <stddef.h>
#include <stdint.h>
#include "rt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rt_path_begin, bit for bit, on host arrays. */
int rt_path_begin_cpu(size_t n, uint32_t spp, const uint32_t *ids, rt_path *paths, float *radiance);
/* What rt_path_advance writes into d_paths, d_radiance and d_alive, bit for bit, with what the device reads from the scene and d_hits
 * as rt_surface records (rt_material_hits'; valid == 0 is "no hit"), as rt_lobe_samples_cpu takes them.  normals: NULL — the direction
 * is drawn about the record's shading_normal, RT_HEMISPHERE_SHADING — or m * 3 floats, the N to draw about (hit.normal for
 * RT_HEMISPHERE_GEOMETRIC).  view: m * 3 floats, -d_incoming[j].direction.  index, count (one u32 on the host), emitted: as the device
 * call's.  dirs: m * 3 floats — the direction of d_next_rays[j] in place of the ray, zeros for a path that ended.  No hit record is
 * rewritten here: surfaces is read only. */
int rt_path_advance_cpu(const rt_surface *surfaces, const float *normals, const float *view, rt_path *paths, size_t m, const uint32_t *index,
                        const uint32_t *count, const float *emitted, uint32_t seed, uint32_t rr_start, float rr_floor, int last, float *radiance, float *dirs,
                        unsigned char *alive);
/* rt_path_resolve, bit for bit, on host arrays. */
int rt_path_resolve_cpu(const float *radiance, size_t n, uint32_t spp, const uint32_t *root, float *rgb);

#ifdef __cplusplus
}
#endif

#include "rt_transmit_host.h" /* the transmission queries' CPU forms: the same paths, through glass */

#endif /* RT_PATH_HOST_H */
