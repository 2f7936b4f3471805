/*
 * rt_distributed_rays.hip — the stochastic pass on caller-supplied rays (rt_trace_rays_distributed, rt_focus_rays, rt_rng_create_seeded,
 * rt_rng_upload), in a translation unit of its own: rt_distributed.hip's code object holds the camera instantiations and the plain
 * kernels alone, instruction for instruction as before ray batches existed.
 *
 *   distributed_kernel<MAXD, BFS, RAYS = true>, dist_chain_kernel<ORDER, RAYS = true>   the two organisations with a ray batch's roots
 *   rng_seed_from_kernel    IsaacRng::new_from_u64(seeds[i]) for generators that belong to no frame
 *   rng_import_kernel       the inverse of rng_export_kernel
 *   focus_rays_kernel       Camera::shoot_focus (main.rs:101-127) as a ray source: start_epoch's arithmetic, written out as rt_ray
 *
 * The two kernel templates and their helpers are rt_dist_kernels.h and the generator is rt_rng.h, which this unit includes as
 * rt_distributed.hip does.  Release builds have no mutable device globals there (the ziggurat tables are constants).  A
 * -DRT_DIAG_PAIR_TIME / -DRT_DIAG_NEED build has rt_cast.h's per-unit counters: this unit includes the header and gets its own
 * copies, and no reader for them (the readers are rt_distributed.hip's), so those counts cover camera frames only.
 */
#include <algorithm>

#include "rt_dist_kernels.h"

namespace rt {

__global__ __launch_bounds__(256) void rng_seed_from_kernel(uint32_t *states, const unsigned long long *seeds, uint32_t n) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    isaac_seed(states + (size_t)p * RNG_WORDS, seeds[p]);
}

hipError_t launch_rng_seed_from(uint32_t *states, const unsigned long long *seeds, uint32_t n, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(rng_seed_from_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, states, seeds, n);
    return hipGetLastError();
}

/* the reference's record of every generator (mem[256], a, b, c, results[256], index) -> bank 0 of the device record, current, with
 * nothing prepared: bank 1 is stale from here on and never read before a generate writes it (rng_refill, rng_prepare_kernel) */
__global__ __launch_bounds__(256) void rng_import_kernel(uint32_t *states, uint32_t n, const uint32_t *in) {
    const size_t n_words = (size_t)n * RNG_BANK_WORDS;
    for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (size_t)gridDim.x * blockDim.x) {
        const size_t p = w / RNG_BANK_WORDS;
        const uint32_t i = (uint32_t)(w - p * RNG_BANK_WORDS);
        uint32_t *rec = states + p * RNG_WORDS;
        rec[i] = in[w]; /* i == RNG_SPARE: the position, which is where bank 0's spare word keeps it (RNG_INDEX) */
        if (i == RNG_SPARE) rec[RNG_FLAGS] = 0u;
    }
}

hipError_t launch_rng_import(uint32_t *states, uint32_t n, const uint32_t *in, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    const size_t n_words = (size_t)n * RNG_BANK_WORDS;
    const size_t groups = std::min<size_t>(4096u, (n_words + 255u) / 256u);
    hipLaunchKernelGGL(rng_import_kernel, dim3((unsigned)groups), dim3(256), 0, stream, states, n, in);
    return hipGetLastError();
}

/* Camera::shoot_focus (main.rs:101-127) of pixel p of the tile, compact row order, with the two Normal(0, blur) draws from the pixel's
 * generator: the operations of start_epoch (dist_chain_kernel / distributed_kernel) on the same values, so the record written is bit
 * for bit the ray rt_render_distributed casts first in that epoch, and the generator is left where that epoch's chain starts. */
__global__ __launch_bounds__(256) void focus_rays_kernel(const KernelFrame fr, float focus, float blur, uint32_t *states, rt_ray *rays) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= fr.cols * fr.rows) return;
    const uint32_t row = p / fr.cols, col = p - row * fr.cols;
    const uint32_t x = fr.x0 + col, y = fr.y0 + row * fr.y_step;
    const float clip_y = (fr.half_height - (float)y) / fr.height_f; /* main.rs:1134-1135 */
    const float clip_x = ((float)x - fr.half_width) / fr.height_f;
    const V3 cam_x = v3(fr.cam_x[0], fr.cam_x[1], fr.cam_x[2]);
    const V3 cam_y = v3(fr.cam_y[0], fr.cam_y[1], fr.cam_y[2]);
    const V3 cam_t = v3(fr.cam_toward[0], fr.cam_toward[1], fr.cam_toward[2]);
    const V3 cam_o = v3(fr.cam_origin_focus[0], fr.cam_origin_focus[1], fr.cam_origin_focus[2]);
    Rng rng;
    rng.lds = nullptr;
    rng_open(rng, states + (size_t)p * RNG_WORDS);
    const V3 direction = normalize(clip_x * cam_x + clip_y * cam_y + cam_t);
    double nx, ny;
    standard_normal_x2(rng, &nx, &ny);
    const float xoffset = (float)(0.0 + (double)blur * nx);
    const float yoffset = (float)(0.0 + (double)blur * ny);
    const V3 d = normalize(direction * focus + cam_x * xoffset + cam_y * yoffset);
    const V3 o = cam_o - (cam_x * xoffset + cam_y * yoffset);
    rng_park(rng);
    rt_ray *r = rays + p;
    r->origin[0] = o.x; r->origin[1] = o.y; r->origin[2] = o.z;
    r->direction[0] = d.x; r->direction[1] = d.y; r->direction[2] = d.z;
    r->face_direction = FACE_FRONT;
    r->has_exclude = 0u;
    r->exclude_kind = 0u;
    r->exclude_index = 0u;
    r->exclude_face = 0u;
}

hipError_t launch_focus_rays(const KernelFrame &fr, float focus, float blur, uint32_t *states, rt_ray *rays, hipStream_t stream) {
    const uint32_t n = fr.cols * fr.rows;
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(focus_rays_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, fr, focus, blur, states, rays);
    return hipGetLastError();
}

hipError_t launch_distributed_rays(const KernelScene &sc, const KernelFrame &fr, const DistParams &dp, uint32_t resident_waves, hipStream_t stream) {
    return launch_distributed_of<true>(sc, fr, dp, resident_waves, stream);
}

hipError_t launch_dist_chain_rays(const KernelScene &sc, const KernelFrame &fr, const DistParams &dp, uint32_t resident_waves, hipStream_t stream) {
    return launch_dist_chain_of<true>(sc, fr, dp, resident_waves, stream);
}

} /* namespace rt */
