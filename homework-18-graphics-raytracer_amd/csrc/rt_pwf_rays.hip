/*
 * rt_pwf_rays.hip — the persistent wavefront kernel's ray-batch instantiations, pwf_kernel<PACKED, BFS, RAYS = true> (rt_trace_rays;
 * rt_kernels.h frame_is_rays), in a translation unit of their own: rt_pwf.hip's code object holds the camera instantiations alone,
 * instruction for instruction as before ray batches existed.
 *
 * Including rt_pwf.hip compiles everything above its RT_PWF_RAYS_TU guard once more, into this unit: the kernel template and its
 * helpers, and also file-scope device globals of diagnostic builds.  So in a -DPA_STATS build, the ray kernels add their phase
 * times into this unit's own copy of pa_phase_stats, which rt_diag_read_pwf_phases (rt_pwf.hip) does not read; likewise rt_cast.h's
 * g_stage_totals in a -DRT_DIAG_STAGES build.  Those counters cover camera frames only.  Release builds have no such globals.
 */
#define RT_PWF_RAYS_TU
#include "rt_pwf.hip"

namespace rt {

void launch_pwf_rays(const KernelScene &sc, const PwParams &pp, float *out, uint32_t workgroups, size_t lds, hipStream_t stream, bool packed,
                     bool bfs) {
    launch_pwf_kernel<true>(sc, pp, out, workgroups, lds, stream, packed, bfs);
}

} /* namespace rt */
