/*
 * rt_light_record.h — what get_shade computes once per hit (main.rs:408-410), shared by the two units that open its light loop:
 * the light queries (rt_light_query.hip) and the area-light queries (rt_area_light_query.hip).  Device code only.
 */
#ifndef RT_LIGHT_RECORD_H
#define RT_LIGHT_RECORD_H

#include "rt_cast.h"
#include "rt_hit_abi.h"

namespace rt {

#define RT_LIGHT_THREADS 256u
#define RT_LIGHT_HIT_POSITION 3u /* word of rt_hit.position */

/* what get_shade computes once per hit (main.rs:408-410) */
struct LightRecord {
    bool valid;
    AbiHit h;
    Mat m;
    V3 adj_n;
};
__device__ __forceinline__ LightRecord light_record(const KernelScene &sc, const rt_hit *__restrict__ hits, const uint64_t i) {
    LightRecord r;
    r.valid = false;
    r.h.g.pos = v3(0.0f, 0.0f, 0.0f);
    r.h.g.normal = v3(0.0f, 0.0f, 1.0f);
    r.h.g.prim = RT_HIT_NO_PRIM;
    r.h.kind = r.h.index = 0u;
    r.m.normal = v3(0.0f, 0.0f, 1.0f);
    r.m.diffuse = r.m.specular = v3(0.0f, 0.0f, 0.0f);
    r.m.shiness = r.m.smoothness = r.m.transparency = r.m.refraction_index = r.m.opaque_decay = 0.0f;
    const AbiHit h = hit_from_abi(hits + i, sc.n_triangles, sc.n_spheres, sc.n_materials, true);
    if (h.valid) {
        r.valid = true;
        r.h = h;
        r.m = material_approx(sc.materials[h.g.obj], h.g.u, h.g.v);
    }
    r.adj_n = adjust_normal(r.m.normal, r.h.g.normal); /* main.rs:410 */
    return r;
}

} /* namespace rt */

#endif /* RT_LIGHT_RECORD_H */
