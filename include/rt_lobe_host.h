/*
 * rt_lobe_host.h — the lobe queries on the CPU (include/rt_amd.h "lobe queries" states every operation and the order; the arithmetic
 * is csrc/rt_lobe.h's, shared with the device), for host arrays and no device.  Library: librt_host.so.  include/rt_host.h includes this
 * header, so a program that includes that one has these too.  A header of its own for include/rt_environment_host.h's reason: these take
 * records, a table and per-sample arrays, no image planes; Python lists them as _capi.LOBE_HOST_SYMBOLS.
 *
 * The limits are the device calls' with the same texts: the counts (RT_ERR_UNSUPPORTED), the descriptor, an empty batch is RT_OK, a null
 * required pointer, then spp, pattern, normal_kind or heuristic.  A failure returns a negative rt_status and sets rt_host_last_error().
 */
#ifndef RT_LOBE_HOST_H
#define RT_LOBE_HOST_H

#include <stddef.h>
#include <stdint.h>
#include "rt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What rt_lobe_rays writes into d_dirs, d_pdf, d_lobe and d_asks, bit for bit, k = s * n + i, with what the device reads from the scene
 * as rt_surface records (rt_material_hits'; valid == 0 is "no hit": zero words everywhere).  normals: NULL — N is the record's
 * shading_normal, RT_HEMISPHERE_SHADING — or n * 3 floats, the N to use (hit.normal for RT_HEMISPHERE_GEOMETRIC).  view: n * 3 floats,
 * -d_incoming[i].direction.  ids: n u32 or NULL for id = i; lobe and asks may be NULL. */
int rt_lobe_samples_cpu(const rt_surface *surfaces, const float *normals, const float *view, const uint32_t *ids, size_t n, uint32_t spp,
                        uint32_t pattern, uint32_t seed, float *dirs, float *pdf, unsigned char *lobe, unsigned char *asks);
/* rt_lobe_pdf, bit for bit, on host arrays. */
int rt_lobe_pdf_cpu(const rt_surface *surfaces, size_t n, const float *view, const float *dirs, uint32_t n_probes, uint32_t normal_kind, float *pdf);
/* rt_environment_pdf, bit for bit: env->d_texels is a host pointer here (it is not read), table what rt_environment_table_cpu wrote. */
int rt_environment_pdf_cpu(const rt_environment *env, const void *table, const float *dirs, size_t count, float *pdf, uint32_t *texel);
/* rt_mis_weigh, bit for bit, on host arrays; rgb is weighed in place. */
int rt_mis_weigh_cpu(size_t count, const float *pdf_own, uint32_t n_own, const float *pdf_other, uint32_t n_other, uint32_t heuristic, int divide_by_own,
                     float *weight, float *rgb);

#ifdef __cplusplus
}
#endif
#endif /* RT_LOBE_HOST_H */
