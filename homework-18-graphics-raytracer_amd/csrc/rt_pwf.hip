/*
 * rt_pwf.hip — the Whitted render path as ONE persistent kernel of workgroup-local wavefronts (RT_VARIANT_PWF, the default): the camera
 * instantiations of pwf_kernel, its launcher and occupancy helpers, pwf_init_kernel and the diagnostics readers.
 *
 * The kernel itself, with the description of its design (items, queues, scheduling, the fold), is the template in rt_pwf_kernel.h;
 * rt_pwf_rays.hip instantiates it for ray batches.
 */
#include "rt_pwf_kernel.h"

namespace rt {

static size_t pwf_dynamic_lds(uint32_t node_cap, uint32_t ring_cap) {
    const bool packed = pa_ready_packed(node_cap, ring_cap);
    return (size_t)(PA_READY_WORDS((node_cap + 63u) / 64u, packed) + 2u * PA_READY_WORDS(ring_cap / 64u, packed)) * sizeof(uint32_t);
}

int pwf_workgroups_per_cu(uint32_t node_cap, uint32_t ring_cap, bool bfs_walk) {
    int n = 0;
    const size_t lds = pwf_dynamic_lds(node_cap, ring_cap);
    const bool packed = pa_ready_packed(node_cap, ring_cap);
    const hipError_t e = bfs_walk ? (packed ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, pwf_kernel<true, true>, (int)PA_THREADS, lds)
                                            : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, pwf_kernel<false, true>, (int)PA_THREADS, lds))
                                  : (packed ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, pwf_kernel<true, false>, (int)PA_THREADS, lds)
                                            : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, pwf_kernel<false, false>, (int)PA_THREADS, lds));
    if (e != hipSuccess || n < 1) n = 1;
    return n;
}

__global__ void pwf_init_kernel(uint32_t *global, KernelFrame *frame, const KernelFrame fr) {
    if (threadIdx.x < PW_G_BLOCK_WORDS) global[threadIdx.x] = 0u;
    if (threadIdx.x == 0u) *frame = fr;
}

size_t pwf_arena_bytes(uint32_t node_cap, uint32_t ring_cap, uint32_t max_depth) {
    /* node inputs + records, the two rings, the tile list, one "complete as it stands" byte per node (read for roots), the fold's lists */
    return ((size_t)node_cap * 4u + (size_t)ring_cap * (3u + PA_SHADE_U4)) * sizeof(uint4) + (size_t)(node_cap / 64u) * 2u * sizeof(uint32_t) +
           (((size_t)node_cap + 15u) & ~(size_t)15u) + (size_t)pwf_fold_list_regions(max_depth) * node_cap * sizeof(uint32_t) + 256u;
}

#ifdef PA_STATS
static uint32_t *g_pw_last_global = nullptr;
extern "C" int rt_diag_read_pwf(uint32_t *out32) {
    if (!g_pw_last_global) return -1;
    return hipMemcpy(out32, g_pw_last_global, 32 * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
/* wave time by phase; reset != 0 clears the counters after reading */
extern "C" int rt_diag_read_pwf_phases(unsigned long long *out32, int reset) {
    if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(pa_phase_stats), 32 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long zero[32] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(pa_phase_stats), zero, sizeof zero) != hipSuccess) return -1;
    }
    return 0;
}
#endif

hipError_t launch_pwf(const KernelScene &sc, KernelFrame fr, float *out, const PwParams &pp, uint32_t workgroups, hipStream_t stream,
                      bool init, bool first_band, bool last_band) {
    const uint32_t total = fr.cols * fr.rows;
    fr.n_chunks = (total + 63u) / 64u;
    if (total == 0u) return hipSuccess;
#ifdef PA_STATS
    g_pw_last_global = pp.global;
#endif
    if (init) hipLaunchKernelGGL(pwf_init_kernel, dim3(1), dim3(64), 0, stream, pp.global, const_cast<KernelFrame *>(pp.frame), fr);
    if (first_band) record_main_kernel_event(0, stream); /* the pair brackets all bands of a call (one, up to ~8 Mpixel) */
    const size_t lds = pwf_dynamic_lds(pp.node_cap, pp.ring_cap);
    const bool packed = pa_ready_packed(pp.node_cap, pp.ring_cap);
    if (frame_is_rays(fr)) launch_pwf_rays(sc, pp, out, workgroups, lds, stream, packed, sc.bfs_walk != 0u && pp.bfs_scratch != nullptr);
    else launch_pwf_kernel<false>(sc, pp, out, workgroups, lds, stream, packed, sc.bfs_walk != 0u && pp.bfs_scratch != nullptr);
    if (last_band) record_main_kernel_event(1, stream);
    return hipGetLastError();
}

} /* namespace rt */

#ifdef RT_DIAG_STAGES
RT_DIAG_STAGE_READER(rt_diag_read_stages_pwf)
#endif
#ifdef RT_DIAG_NEED
RT_DIAG_NEED_READER(rt_diag_read_need_pwf)
#endif
#ifdef RT_DIAG_BFS
RT_DIAG_BFS_READER(rt_diag_read_bfs)
#endif
