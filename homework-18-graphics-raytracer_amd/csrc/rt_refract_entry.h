/*
 * rt_refract_entry.h — the entry of get_refract's walk (main.rs:354-368) on one record, written once for rt_refract_enter
 * (rt_refract_query.hip), rt_path_branch (rt_transmit_query.hip) and rt_path_branch_cpu (librt_host.so): Trapped at entry, or ray_inside
 * and the state of a walk that has cast nothing.  Nothing here is new arithmetic: refract_dir and normalize are rt_shade.h's and
 * rt_vec.h's, called with rt::refract_rays_kernel's operands in its order.  The ray is an rt_ray by value: a device caller stores its
 * eleven words as dwords (store_ray_record below, on rt_hit_abi.h's store_ray), a host caller assigns it.
 */
#ifndef RT_REFRACT_ENTRY_H
#define RT_REFRACT_ENTRY_H

#include <stdint.h>

#include "../../include/rt_amd.h"
#include "rt_shade.h"
#include "rt_vec.h"

namespace rt {

#define RT_REFR_TRAPPED 2u    /* main.rs:356-358 */
#define RT_REFR_FACE_FRONT 0u /* main.rs:52-57, as rt_cast.h's FACE_FRONT and FACE_BACK */
#define RT_REFR_FACE_BACK 1u

/* eleven zero words: the ray of a record that casts nothing */
RT_HD rt_ray no_ray_record() {
    rt_ray r;
    r.origin[0] = r.origin[1] = r.origin[2] = 0.0f;
    r.direction[0] = r.direction[1] = r.direction[2] = 0.0f;
    r.face_direction = r.has_exclude = r.exclude_kind = r.exclude_index = r.exclude_face = 0u;
    return r;
}

/* The d_kind word rt_refract_enter writes for one record, and in *ray its d_rays entry.  `valid`: the record is a hit by the hit
 * queries' rules; then `pos`, `normal`, `hit_kind` and `hit_index` are the hit's, `in_dir` hit.ray.direction and `k` the refraction
 * index of approx(hit.at).  d_flags is kind == RT_REFR_WALKING; d_travel +0 and d_casts 0 are the caller's to write. */
RT_HD uint32_t refract_enter_record(bool valid, V3 pos, V3 normal, V3 in_dir, float k, uint32_t hit_kind, uint32_t hit_index, rt_ray *ray) {
    *ray = no_ray_record();
    if (!valid) return RT_HIT_NONE;
    V3 refract_in;
    if (!refract_dir(normal, in_dir, k, &refract_in)) return RT_REFR_TRAPPED;
    /* ray_inside, main.rs:360-368: the direction normalised a second time; bit for bit the ray refract_rays_kernel casts first */
    const V3 d = normalize(refract_in);
    ray->origin[0] = pos.x;
    ray->origin[1] = pos.y;
    ray->origin[2] = pos.z;
    ray->direction[0] = d.x;
    ray->direction[1] = d.y;
    ray->direction[2] = d.z;
    ray->face_direction = RT_REFR_FACE_BACK;
    ray->has_exclude = 1u;
    ray->exclude_kind = hit_kind;
    ray->exclude_index = hit_index;
    ray->exclude_face = RT_REFR_FACE_FRONT;
    return RT_REFR_WALKING;
}

} /* namespace rt */

#if defined(__HIPCC__)
#include "rt_hit_abi.h"

namespace rt {

/* the device's store of such a ray: its eleven dwords, as every kernel writes a ray */
__device__ __forceinline__ void store_ray_record(rt_ray *__restrict__ out, const rt_ray &r) {
    store_ray(out, v3(r.origin[0], r.origin[1], r.origin[2]), v3(r.direction[0], r.direction[1], r.direction[2]), r.face_direction, r.has_exclude,
              r.exclude_kind, r.exclude_index, r.exclude_face);
}

} /* namespace rt */
#endif

#endif /* RT_REFRACT_ENTRY_H */
