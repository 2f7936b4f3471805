/*
 * rt_light_connect_host.h — the light-connection queries on the CPU (include/rt_amd.h "light-connection queries" states every operation
 * and the order; the arithmetic is csrc/rt_light_connect.h's, shared with the device), for host arrays and no device.  Library:
 * librt_host.so.  include/rt_host.h includes this header, so a program that includes that one has these too.  A header of its own so
 * that each block's header declares its own calls alone (include/rt_connect_host.h and include/rt_path_host.h stay at their three);
 * Python lists them as _capi.LIGHT_CONNECT_HOST_SYMBOLS.
 *
 * What the device reads from the scene comes as rt_surface records (rt_material_hits'; valid == 0 is "no hit"), the hits' positions,
 * views, the scene's rt_light records and their aux values, as rt_path_connect_cpu takes its inputs.  index, count (one u32 on the host):
 * as the device calls'.  No record is written by either.
 * The limits are the device calls' with the same texts: m >= 2^32 (RT_ERR_UNSUPPORTED), an empty batch (no slots, no lights) is RT_OK, a
 * null required pointer.  There is no scene to hold the range of lights against: lights holds light_first + light_count records.  A
 * failure returns a negative rt_status and sets rt_host_last_error().
 */
#ifndef RT_LIGHT_CONNECT_HOST_H
#define RT_LIGHT_CONNECT_HOST_H

#include <stddef.h>
#include <stdint.h>
#include "rt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What rt_path_connect_lights writes into d_asks, d_pending, d_reach and d_chosen (chosen may be NULL), bit for bit, and into dirs
 * (m * 3 floats) the direction of d_shadow_rays[j] in place of the ray: towards the point drawn where it asks, zeros where it does not.
 * positions: m * 3 floats, hit.position; view: m * 3 floats, -d_incoming[j].direction.  lights: the scene's lights, indexed from 0;
 * aux: two floats per light of `lights` (cos_in, cos_out: rt_scene_describe_filters' light2), or NULL: computed from each light by the
 * function rt_scene_create uses.  radii, weights: light_count floats each, or NULL. */
int rt_path_connect_lights_cpu(const rt_surface *surfaces, const float *positions, const float *view, const rt_light *lights, const float *aux,
                               const rt_path *paths, size_t m, const uint32_t *index, const uint32_t *count, uint32_t light_first, uint32_t light_count,
                               const float *radii, const float *weights, uint32_t seed, float *dirs, unsigned char *asks, float *pending, float *reach,
                               uint32_t *chosen);
/* rt_path_settle_lights, bit for bit, on host arrays.  shadow_hits may be NULL: nothing occludes. */
int rt_path_settle_lights_cpu(const rt_path *paths, size_t m, const uint32_t *index, const uint32_t *count, unsigned char *asks, const rt_ray *shadow_rays,
                              const rt_hit *shadow_hits, const float *reach, const float *pending, float *radiance);

#ifdef __cplusplus
}
#endif
#endif /* RT_LIGHT_CONNECT_HOST_H */
