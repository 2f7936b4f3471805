/*
 * rt_hit_abi.h — the ABI records a caller may have written, as the kernels read and write them: an rt_hit validated before anything
 * is indexed with it (hit_from_abi) and an rt_ray written word by word (store_ray).  Shared by the hit queries (rt_hit_query.hip) and
 * the scatter queries (rt_scatter_query.hip).
 */
#ifndef RT_HIT_ABI_H
#define RT_HIT_ABI_H

#include "rt_cast.h"

namespace rt {

/* A caller's rt_hit as the kernels' HitGeom.  `valid`: kind is Sphere or Triangle and (with a scene) object_index names a material;
 * anything else is "no hit" and nothing is indexed with it.  An index outside its primitive array is used as given — it only ever
 * serves as an exclusion, and as one it excludes nothing (no PrimitiveIndex of the scene equals it): g.prim is then RT_HIT_NO_PRIM. */
#define RT_HIT_NO_PRIM 0xffffffffu
struct AbiHit {
    HitGeom g;
    uint32_t kind, index;
    bool valid;
};
__device__ __forceinline__ AbiHit hit_from_abi(const rt_hit *__restrict__ r, uint32_t n_triangles, uint32_t n_spheres, uint32_t n_materials,
                                               bool check_object) {
    AbiHit h;
    h.kind = r->kind;
    h.index = r->index;
    h.g.obj = r->object_index;
    h.g.pos = v3(r->position[0], r->position[1], r->position[2]);
    h.g.normal = v3(r->normal[0], r->normal[1], r->normal[2]);
    h.g.u = r->uv[0];
    h.g.v = r->uv[1];
    h.g.bf = r->face_direction != 0u ? 1u : 0u; /* a value above 1 is read as Back */
    h.valid = h.kind <= 1u && (!check_object || h.g.obj < n_materials);
    h.g.prim = RT_HIT_NO_PRIM;
    if (h.kind == 1u && h.index < n_triangles) h.g.prim = h.index;
    else if (h.kind == 0u && h.index < n_spheres) h.g.prim = n_triangles + h.index;
    return h;
}
__device__ __forceinline__ uint32_t excl_of(uint32_t prim, uint32_t face) { return prim == RT_HIT_NO_PRIM ? 0u : pack_excl(prim, face); }

__device__ __forceinline__ void store_ray(rt_ray *__restrict__ out, V3 o, V3 d, uint32_t mode, uint32_t has, uint32_t kind, uint32_t index,
                                          uint32_t face) {
    const uint32_t w[11] = {__float_as_uint(o.x), __float_as_uint(o.y), __float_as_uint(o.z), __float_as_uint(d.x),
                            __float_as_uint(d.y), __float_as_uint(d.z), mode, has, kind, index, face};
    uint32_t *const p = reinterpret_cast<uint32_t *>(out);
#pragma unroll
    for (int k = 0; k < 11; ++k) p[k] = w[k];
}

} /* namespace rt */

#endif /* RT_HIT_ABI_H */
