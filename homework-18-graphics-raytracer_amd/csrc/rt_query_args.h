/*
 * rt_query_args.h — how an image-side query states its arguments ONCE for its three entry points: the device form (rt_X), the _host form
 * (a round trip through the device) and the _cpu form (librt_host.so).  Beside its arithmetic, in the header both libraries share
 * (rt_denoise.h, rt_temporal.h, rt_svgf.h, rt_rectify.h, rt_upsample.h, rt_adaptive.h, rt_bloom.h), a query has a plain aggregate of the entry
 * point's arguments in interface order, without the stream, with these members:
 *     limits(form, &status)   THE argument check, in the order include/rt_amd.h states: the text of the first refusal and how it is
 *                             reported, or null.  What depends on the form is written as a question to it (below).
 *     empty()                 nothing to do; asked after the limits passed
 *     arrays(stage)           THE list of every array the call touches, each named as what it is: stage.in (a whole input), stage.plane
 *                             (n pixels, stride, width), stage.out, stage.inout, stage.scratch, stage.guides (a guides struct and its
 *                             planes).  The stage hands back the pointer the call is to use instead; HostRoundTrip (rt_api_internal.h) is
 *                             the stage of a _host form.  Queries without a _host form have none.
 *     call() / level(j)       the Op or Level struct that travels to the kernels and through the CPU loops
 * The three bodies are written once each: device_query and host_query (rt_api_internal.h), cpu_query (host/rt_host.cpp).  An entry
 * point is one statement: the aggregate, the launcher or the CPU loop, the shared body.  Nothing here needs HIP.
 */
#ifndef RT_QUERY_ARGS_H
#define RT_QUERY_ARGS_H

#include <stddef.h>
#include <stdint.h>

namespace rt {

enum QueryForm { QUERY_DEVICE, QUERY_HOST_COPY, QUERY_CPU };

/* the kernels read and write 16-byte records as 128-bit words: only the device form sees the caller's own device pointers (the copies
 * of a _host form are hipMalloc's and aligned whatever the host arrays are, the CPU loops go word by word) */
inline bool query_misaligned(QueryForm form, const void *a, const void *b = nullptr) {
    return form == QUERY_DEVICE && (((uintptr_t)a | (uintptr_t)b) & 15u) != 0u;
}

/* the scratch of a multi-level filter is the caller's, except in the _host form, whose round trip makes its own */
inline bool query_takes_temp(QueryForm form) { return form != QUERY_HOST_COPY; }

} /* namespace rt */

#endif /* RT_QUERY_ARGS_H */
