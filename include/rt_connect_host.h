/*
 * rt_connect_host.h — the connection queries on the CPU (include/rt_amd.h "connection queries" states every operation and the order;
 * the arithmetic is csrc/rt_connect.h's, shared with the device), for host arrays and no device.  Library: librt_host.so.
 * include/rt_host.h includes this header, so a program that includes that one has these too.  A header of its own so that each block's
 * header declares its own calls alone (include/rt_path_host.h stays at its three); Python lists them as _capi.CONNECT_HOST_SYMBOLS.
 *
 * What the device reads from the scene comes as rt_surface records (rt_material_hits'; valid == 0 is "no hit"), views and normals, as
 * rt_path_advance_cpu takes them.  env->d_texels and table are host pointers here (rt_environment_table_cpu's table).  index, count (one
 * u32 on the host): as the device calls'.  No record is written by any of the three.
 * The limits are the device calls' with the same texts: m >= 2^32 (RT_ERR_UNSUPPORTED), the descriptor, an empty batch is RT_OK, a null
 * required pointer, then the heuristic.  A failure returns a negative rt_status and sets rt_host_last_error().
 */
#ifndef RT_CONNECT_HOST_H
#define RT_CONNECT_HOST_H

#include <stddef.h>
#include <stdint.h>
#include "rt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What rt_path_connect writes into d_asks and d_pending, bit for bit, and into dirs (m * 3 floats) the direction of d_shadow_rays[j] in
 * place of the ray: the direction drawn, also where it does not ask, zeros where nothing was drawn.  normals: NULL — the record's
 * shading_normal, RT_HEMISPHERE_SHADING — or m * 3 floats, the N of the lobes' density and of "leaves the surface" (hit.normal for
 * RT_HEMISPHERE_GEOMETRIC).  view: m * 3 floats, -d_incoming[j].direction. */
int rt_path_connect_cpu(const rt_surface *surfaces, const float *normals, const float *view, const rt_environment *env, const void *table,
                        const rt_path *paths, size_t m, const uint32_t *index, const uint32_t *count, uint32_t seed, uint32_t heuristic, int last,
                        float *dirs, unsigned char *asks, float *pending);
/* rt_path_settle, bit for bit, on host arrays.  shadow_hits may be NULL: nothing occludes. */
int rt_path_settle_cpu(const rt_path *paths, size_t m, const uint32_t *index, const uint32_t *count, unsigned char *asks, const rt_hit *shadow_hits,
                       const float *pending, float *radiance);
/* rt_path_weigh_escape, bit for bit, on host arrays: it takes no scene on the device either. */
int rt_path_weigh_escape_cpu(const rt_environment *env, const void *table, const rt_path *paths, size_t m, const uint32_t *index, const uint32_t *count,
                             const rt_hit *hits, const rt_ray *incoming, uint32_t heuristic, float *emitted);

#ifdef __cplusplus
}
#endif
#endif /* RT_CONNECT_HOST_H */
