/*
 * rt_kernels_rays.hip — the per-pixel kernel's ray-batch instantiations, whitted_kernel<MAXD, USE_LDS, RAYS = true> (rt_trace_rays;
 * rt_kernels.h frame_is_rays), in a translation unit of their own: rt_kernels.hip's code object holds the camera instantiations
 * alone, instruction for instruction as before ray batches existed.
 *
 * The kernel template and its helpers are rt_whitted_kernel.h, which this unit includes as rt_kernels.hip does.  Release builds have
 * no device globals there.  A -DRT_DIAG_STAGES build has one: rt_cast.h's per-unit g_stage_totals.  This unit includes the header
 * and gets its own copy, and no reader for it (the readers are rt_kernels.hip's), so those stage counts cover camera frames only.
 */
#include "rt_whitted_kernel.h"

namespace rt {

hipError_t launch_tiles_rays(int maxd, const KernelScene &sc, const KernelFrame &fr, float *out, unsigned long long *ray_count,
                             const KernelQueues &qs, uint32_t waves, hipStream_t stream, bool use_lds) {
    if (maxd <= 8) return launch_tiles_of<8, true>(sc, fr, out, ray_count, qs, waves, stream, use_lds);
    return launch_tiles_of<RT_MAX_DEPTH, true>(sc, fr, out, ray_count, qs, waves, stream, use_lds);
}

} /* namespace rt */
