/*
 * rt_pwf_rays.hip — the persistent wavefront kernel's ray-batch instantiations, pwf_kernel<PACKED, BFS, RAYS = true> (rt_trace_rays;
 * rt_kernels.h frame_is_rays), in a translation unit of their own: rt_pwf.hip's code object holds the camera instantiations alone,
 * instruction for instruction as before ray batches existed.
 *
 * The kernel template and its helpers are rt_pwf_kernel.h, which this unit includes as rt_pwf.hip does, and with them the file-scope
 * device globals of diagnostic builds: this unit includes the header and gets its own copy.  So in a -DPA_STATS build, the ray
 * kernels add their phase times into this unit's own copy of pa_phase_stats, which rt_diag_read_pwf_phases (rt_pwf.hip) does not
 * read; likewise rt_cast.h's g_stage_totals in a -DRT_DIAG_STAGES build.  Those counters cover camera frames only.  Release builds
 * have no such globals.
 */
#include "rt_pwf_kernel.h"

namespace rt {

void launch_pwf_rays(const KernelScene &sc, const PwParams &pp, float *out, uint32_t workgroups, size_t lds, hipStream_t stream, bool packed,
                     bool bfs) {
    launch_pwf_kernel<true>(sc, pp, out, workgroups, lds, stream, packed, bfs);
}

} /* namespace rt */
