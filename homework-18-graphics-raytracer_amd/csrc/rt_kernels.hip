/*
 * rt_kernels.hip — the per-pixel Whitted render path (one work-item per primary ray): the camera instantiations of whitted_kernel,
 * its launchers, the events around a call's main kernel, and the rt_detmath diagnostics kernel.
 *
 * The kernel itself, with the description of its design, is the template in rt_whitted_kernel.h; rt_kernels_rays.hip instantiates it
 * for ray batches.
 */
#include "rt_whitted_kernel.h"

namespace rt {

template <int MAXD>
static hipError_t launch_tiles(const KernelScene &sc, const KernelFrame &fr, float *out, unsigned long long *ray_count,
                               const KernelQueues &qs, uint32_t waves, hipStream_t stream, bool use_lds) {
    if (frame_is_rays(fr)) return launch_tiles_rays(MAXD, sc, fr, out, ray_count, qs, waves, stream, use_lds);
    return launch_tiles_of<MAXD, false>(sc, fr, out, ray_count, qs, waves, stream, use_lds);
}

/* optional HIP events recorded on the launch stream right around the dominant (render) kernel of a call */
/* thread-local: set by a render call on its own host thread and read by the launchers it calls on that thread */
static thread_local hipEvent_t g_ev_start = nullptr, g_ev_stop = nullptr;
static thread_local bool g_ev_muted = false; /* set around launches that are not "the" render kernel (the wavefront path's fallback) */
void set_main_kernel_events(hipEvent_t start, hipEvent_t stop) { g_ev_start = start; g_ev_stop = stop; }
void mute_main_kernel_events(bool muted) { g_ev_muted = muted; }
void record_main_kernel_event(int which, hipStream_t stream) {
    hipEvent_t ev = which == 0 ? g_ev_start : g_ev_stop;
    if (ev && !g_ev_muted) (void)hipEventRecord(ev, stream);
}

template <int MAXD>
static hipError_t launch_maxd(const KernelScene &sc, KernelFrame fr, float *out, unsigned long long *ray_count, const KernelQueues &qs,
                              hipStream_t stream, int variant) {
    const bool use_lds = (variant & RT_VARIANT_LDS) != 0 && (size_t)sc.n_triangles * sizeof(DevTri) <= RT_LDS_SCENE_LIMIT;
    const uint32_t total = fr.cols * fr.rows;
    fr.n_chunks = (total + 63u) / 64u;
    record_main_kernel_event(0, stream);
    uint32_t waves = fr.n_chunks;
    if (qs.run_if != nullptr && waves > RT_FALLBACK_WAVES) waves = RT_FALLBACK_WAVES;
    const hipError_t e = launch_tiles<MAXD>(sc, fr, out, ray_count, qs, waves, stream, use_lds);
    record_main_kernel_event(1, stream);
    return e;
}

hipError_t launch_whitted(const KernelScene &sc, const KernelFrame &fr, float *out, unsigned long long *ray_count,
                          const KernelQueues &qs, hipStream_t stream, int variant) {
    if (fr.max_depth <= 8) return launch_maxd<8>(sc, fr, out, ray_count, qs, stream, variant);
    return launch_maxd<RT_MAX_DEPTH>(sc, fr, out, ray_count, qs, stream, variant);
}

} /* namespace rt */

/* ---- diagnostics: rt_detmath on the device ----------------------------------------- */

namespace rt {

/* host + device so rt_math_eval_host runs the very same source */
__host__ __device__ float math_eval_one(int op, float x, float y) {
    switch (op) {
        case RT_MATH_SIN: return rtdm::sinf(x);
        case RT_MATH_COS: return rtdm::cosf(x);
        case RT_MATH_TAN: return rtdm::tanf(x);
        case RT_MATH_ACOS: return rtdm::acosf(x);
        case RT_MATH_ATAN2: return rtdm::atan2f(x, y);
        case RT_MATH_POW: return rtdm::powf(x, y);
        case RT_MATH_F32_DIV: return x / y;
        case RT_MATH_F32_SQRT: return rtdm::f_sqrt(x);
        case RT_MATH_F64_SQRT_HI: return rtdm::f32_from_bits((uint32_t)(rtdm::f64_bits(rtdm::d_sqrt((double)x * (double)y)) >> 32));
        case RT_MATH_F64_SQRT_LO: return rtdm::f32_from_bits((uint32_t)(rtdm::f64_bits(rtdm::d_sqrt((double)x * (double)y))));
        case RT_MATH_F64_DIV_HI: return rtdm::f32_from_bits((uint32_t)(rtdm::f64_bits((double)x / (double)y) >> 32));
        case RT_MATH_F64_DIV_LO: return rtdm::f32_from_bits((uint32_t)(rtdm::f64_bits((double)x / (double)y)));
        case RT_MATH_ROUND: return rtdm::f_round(x);
        case RT_MATH_SINCOS_SIN:
        case RT_MATH_SINCOS_COS: {
            float s, c;
            rtdm::sincosf(x, &s, &c);
            return op == RT_MATH_SINCOS_SIN ? s : c;
        }
        case RT_MATH_F32_AS_I32: return rtdm::f32_from_bits((uint32_t)rtdm::f32_as_i32(x));
        case RT_MATH_IS_NORMAL: return rtdm::is_normal(x) ? 1.0f : 0.0f;
        case RT_MATH_INT_CLASS: return (float)rtdm::f32_int_class(x);
        default: return 0.0f;
    }
}

/* the binary64 primitives and intermediates under the f32 results above, returned whole (op codes = rt_math64_op) */
__host__ __device__ double math_eval64_one(int op, double a, double b) {
    switch (op) {
        case RT_MATH64_DIV: return a / b;
        case RT_MATH64_SQRT: return rtdm::d_sqrt(a);
        case RT_MATH64_NARROW: return (double)(float)a;
        case RT_MATH64_ROUND_I32: return (double)rtdm::d_round_to_i32(a);
        case RT_MATH64_FROM_I64: return (double)(int64_t)rtdm::f64_bits(a);
        case RT_MATH64_EXP_MID: return rtdm::exp_mid(a);
        case RT_MATH64_LOG_POS: return rtdm::log_pos(a);
        case RT_MATH64_ATAN2_UPPER: return rtdm::atan2_upper(a, b);
        default: return 0.0;
    }
}

__global__ void math_eval_kernel(int op, const float *__restrict__ x, const float *__restrict__ y, float *__restrict__ out, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = math_eval_one(op, x[i], y[i]);
}

__global__ void math_eval64_kernel(int op, const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ out, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = math_eval64_one(op, a[i], b[i]);
}

static unsigned math_eval_blocks(size_t n) {
    const size_t blocks = (n + 255) / 256;
    return blocks > 4096 ? 4096u : (unsigned)blocks;
}

hipError_t launch_math_eval(int op, const float *d_x, const float *d_y, float *d_out, size_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(math_eval_kernel, dim3(math_eval_blocks(n)), dim3(256), 0, stream, op, d_x, d_y, d_out, n);
    return hipGetLastError();
}

hipError_t launch_math_eval(int op, const double *d_a, const double *d_b, double *d_out, size_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(math_eval64_kernel, dim3(math_eval_blocks(n)), dim3(256), 0, stream, op, d_a, d_b, d_out, n);
    return hipGetLastError();
}

void math_eval_host(int op, const float *x, const float *y, float *out, size_t n) {
    for (size_t i = 0; i < n; ++i) out[i] = math_eval_one(op, x[i], y ? y[i] : 0.0f);
}

void math_eval_host(int op, const double *a, const double *b, double *out, size_t n) {
    for (size_t i = 0; i < n; ++i) out[i] = math_eval64_one(op, a[i], b ? b[i] : 0.0);
}

} /* namespace rt */

#ifdef RT_DIAG_STAGES
RT_DIAG_STAGE_READER(rt_diag_read_stages_kernels)
#endif
