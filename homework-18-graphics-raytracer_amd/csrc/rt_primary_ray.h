/*
 * rt_primary_ray.h — Camera::shoot(clip(x, y)) (main.rs:83-99, 1093-1096) with the per-frame basis of make_kernel_frame: the operations
 * of the Whitted kernels' primary ray (rt_kernels.hip), written once for the units that hand primary rays to the caller:
 * rt_query.hip (rt_camera_rays: through the pixel's integer coordinate), rt_film_query.hip and rt_adaptive_query.hip
 * (rt_camera_rays_offset / rt_camera_rays_listed: through a sub-pixel position).
 */
#ifndef RT_PRIMARY_RAY_H
#define RT_PRIMARY_RAY_H

#include "rt_cast.h"

namespace rt {

/* the ray through the image position (xf, yf), in pixels */
__device__ __forceinline__ Ray primary_ray_through(const KernelFrame &fr, float xf, float yf) {
    const float clip_y = (fr.half_height - yf) / fr.height_f;
    const float clip_x = (xf - fr.half_width) / fr.height_f;
    const V3 cx = v3(fr.cam_x[0], fr.cam_x[1], fr.cam_x[2]);
    const V3 cy = v3(fr.cam_y[0], fr.cam_y[1], fr.cam_y[2]);
    const V3 ct = v3(fr.cam_toward[0], fr.cam_toward[1], fr.cam_toward[2]);
    Ray r;
    r.o = v3(fr.cam_origin[0], fr.cam_origin[1], fr.cam_origin[2]);
    r.d = normalize(clip_x * cx + clip_y * cy + ct);
    r.mode = FACE_FRONT;
    r.excl = 0u;
    return r;
}

/* the ray of compact pixel (col, row) of a tile, through its integer coordinate */
__device__ __forceinline__ Ray primary_ray(const KernelFrame &fr, uint32_t col, uint32_t row) {
    const uint32_t x = fr.x0 + col, y = fr.y0 + row * fr.y_step;
    return primary_ray_through(fr, (float)x, (float)y);
}

/* the ray of compact pixel pix = row * cols + col of a tile, through the sub-pixel position (dx, dy) of it */
__device__ __forceinline__ Ray primary_ray_offset(const KernelFrame &fr, uint32_t pix, float dx, float dy) {
    const uint32_t row = pix / fr.cols, col = pix - row * fr.cols;
    const uint32_t x = fr.x0 + col, y = fr.y0 + row * fr.y_step;
    return primary_ray_through(fr, (float)x + dx, (float)y + dy);
}

/* the rt_ray record of a primary ray: face Front, no exclusion */
__device__ __forceinline__ void store_primary_ray(const Ray &r, rt_ray *__restrict__ out) {
    const uint32_t w[11] = {__float_as_uint(r.o.x), __float_as_uint(r.o.y), __float_as_uint(r.o.z), __float_as_uint(r.d.x),
                            __float_as_uint(r.d.y), __float_as_uint(r.d.z), FACE_FRONT, 0u, 0u, 0u, 0u};
    uint32_t *const o = reinterpret_cast<uint32_t *>(out);
#pragma unroll
    for (int k = 0; k < 11; ++k) o[k] = w[k];
}

} /* namespace rt */

#endif /* RT_PRIMARY_RAY_H */
