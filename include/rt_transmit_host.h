/*
 * rt_transmit_host.h — the transmission queries on the CPU (include/rt_amd.h "transmission queries" states every operation and the
 * order; the arithmetic is csrc/rt_transmit.h's, shared with the device), for host arrays and no device.  Library: librt_host.so.
 * include/rt_path_host.h includes this header — they are the path queries' CPU forms for glass — and include/rt_host.h includes that
 * one, so a program that includes either has these too.  A header of its own so that each block's header declares its own calls alone;
 * Python lists them as _capi.TRANSMIT_HOST_SYMBOLS.
 *
 * What the device reads from the scene comes as rt_surface records (rt_material_hits'; valid == 0 is "no hit"), as
 * rt_path_advance_cpu takes them: transparency, refraction_index and opaque_decay are read from there.  No hit record is rewritten
 * here: surfaces and hits are read only.  index, count (one u32 on the host): as the device calls'.
 * The limits are the device calls' with the same texts: m >= 2^32 (RT_ERR_UNSUPPORTED), an empty batch is RT_OK, a null required
 * pointer, then rr_floor.  A failure returns a negative rt_status and sets rt_host_last_error().
 */
#ifndef RT_TRANSMIT_HOST_H
#define RT_TRANSMIT_HOST_H

#include <stddef.h>
#include <stdint.h>
#include "rt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What rt_path_branch writes into d_paths, d_lobe, d_transmit and the five walk-state arrays, bit for bit.  hits: the vertices (position,
 * normal, kind and index are read; whether a record is a hit is surfaces[j].valid); incoming: the rays that found them (the direction is
 * read). */
int rt_path_branch_cpu(const rt_surface *surfaces, const rt_hit *hits, const rt_ray *incoming, rt_path *paths, size_t m, const uint32_t *index,
                       const uint32_t *count, uint32_t seed, int last, unsigned char *lobe, unsigned char *transmit, rt_ray *walk_rays, uint32_t *kind,
                       float *travel, uint32_t *casts, unsigned char *walk_flags);
/* What rt_path_transmit writes into d_paths, d_kind, d_next_rays, d_alive and d_walk_flags, bit for bit. */
int rt_path_transmit_cpu(const rt_surface *surfaces, rt_path *paths, size_t m, const uint32_t *index, const uint32_t *count, uint32_t *kind,
                         const float *travel, const rt_ray *escape, uint32_t seed, uint32_t rr_start, float rr_floor, rt_ray *next_rays,
                         unsigned char *alive, unsigned char *walk_flags);

#ifdef __cplusplus
}
#endif
#endif /* RT_TRANSMIT_HOST_H */
