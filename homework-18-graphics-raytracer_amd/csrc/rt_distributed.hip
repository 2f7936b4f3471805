/*
 * rt_distributed.hip — the stochastic ("distributed") pass as a HIP kernel for gfx950.
 *
 * Replaces the par_iter_mut closure at src/main.rs:1131-1156: per pixel and epoch,
 *   shoot_focus (2 Gaussian draws, main.rs:101-127) -> cast -> distributed_ray_trace (main.rs:521-614),
 * with the per-pixel IsaacRng (seeded y*2^33 + x, main.rs:1117-1127) resident in HBM and its stream
 * continuing across epochs.  The sample filter of main.rs:1157-1160 (drop unless all three channels
 * are is_normal) and `img[at] += photon` (main.rs:1165) are fused into the kernel.
 *
 * distributed_ray_trace is a chain, not a tree (one scattered ray per level), so the per-lane state
 * machine is: cast -> [select + scatter] -> cast next -> shade next (3 shadow casts) -> descend ...,
 * then unwind `get_shade(next).mix(x * brdf, 0.5)` / `(x + get_shade(next)) * decay` through a small
 * frame stack.  Every cast of every lane goes through the same wave-convergent intersection loop as the
 * Whitted kernel (rt_cast.h).  get_shade(&hit) at main.rs:524 is pure and only used at depth <= 0; it is
 * evaluated there only (the oracle follows the same plan, so cast counts agree).
 *
 * rand 0.5 (ISAAC-32, Uniform<f32>, ziggurat Normal) is restated from the crate's published algorithms (the
 * crate is not in the build image).  Pinned: bit-for-bit against oracle/rt_oracle.cpp on every sample, flag and RNG
 * record, and — through main()'s whole progressive loop at 7 epochs — per pixel against the reference's own
 * report/out.png (blur 0.04) and report/out_small_blur.png (blur 0.02): tests/test_gpu_reference_pins.py.
 *
 * Layout: the generator is rt_rng.h; the two organisations of the pass, distributed_kernel and dist_chain_kernel, are templates in
 * rt_dist_kernels.h, instantiated here for camera frames and in rt_distributed_rays.hip for ray batches.  This unit holds the rest:
 * the RNG kernels (seed, look-ahead, export), the split pass's shade, unwind and pixel-order kernels, the launchers and the
 * diagnostics readers.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>

#include "rt_rng.h"

namespace rt {

__global__ __launch_bounds__(256) void rng_seed_kernel(uint32_t *states, uint32_t cols, uint32_t rows, uint32_t x0, uint32_t y0, uint32_t y_step) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= cols * rows) return;
    const uint32_t row = p / cols, col = p - row * cols;
    const unsigned long long y = y0 + (unsigned long long)row * y_step, x = x0 + col;
    isaac_seed(states + (size_t)p * RNG_WORDS, y * (2ull << 32) + x); /* main.rs:1119 */
}

hipError_t launch_rng_seed(uint32_t *states, const KernelFrame &fr, hipStream_t stream) {
    const uint32_t n = fr.cols * fr.rows;
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(rng_seed_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, states, fr.cols, fr.rows, fr.x0, fr.y0, fr.y_step);
    return hipGetLastError();
}

/* ---- the look-ahead pass: every pixel gets its next block before a render kernel may need it ---- */

/* list[1 + k] = the pixels without a prepared bank; list[0] = how many (zeroed by the launcher) */
__global__ __launch_bounds__(256) void rng_scan_kernel(const uint32_t *states, uint32_t n_pixels, uint32_t *list) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    const bool want = p < n_pixels && (states[(size_t)p * RNG_WORDS + RNG_FLAGS] & 2u) == 0u;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(want);
    if (m == 0ull) return;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t base = 0u;
    if (lane == (uint32_t)__builtin_ctzll(m)) base = atomicAdd(list, (uint32_t)__builtin_popcountll(m));
    base = (uint32_t)__builtin_amdgcn_readlane((int)base, (int)__builtin_ctzll(m));
    if (want) list[1u + base + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = p;
}

/* Every lane generates the next block of ONE record, its mem[] in a column of LDS of its own: word i of the lane's record
 * at stage[i * SLOTS + lane], SLOTS a multiple of 32, so a lane stays in its bank whatever i it asks for — the two
 * data-dependent reads of a step never conflict.  Nothing is shared between lanes: no barriers.  mem[i] and mem[i + 128] of
 * the next four steps are read ahead of the chain (step j only ever writes mem[j], so they cannot be stale), which leaves ONE
 * LDS latency per step on it (b needs mem[(y >> 10) & 255], the next y needs b), and the four results of a group leave as
 * one 16-byte store.  Two one-wave workgroups of 64 records (64 KB) per CU.  Measured alone over 2^20 records
 * (tools/diag_prepare.py, profiles/r03_lookahead_kernel.txt): 1.37 ms against 2.04 ms for round 2's form (8 records per wave
 * staged by all its lanes, the steps on 8 of the 64, twenty waves per CU: the LDS pipe served 64-lane instructions for 8
 * lanes' worth of work) — 0.78 ms of steps (~230 clocks each) and 0.92 ms of copies (2.2 TB/s in 16-byte pieces), partly
 * overlapped.  What the pass gains is more than that: the look-ahead runs beside the shade kernel, and two waves per CU
 * take far less from it than twenty did (shade kernel 5.97 -> 4.50 ms per batch, the pass 1 073 -> 1 155 Msamples/s).  One
 * workgroup of 160 lanes with all 160 KB of a CU is as fast alone (1.39 ms) but cannot share a CU with the shade kernel's
 * workgroups: 1 118 Msamples/s. */
struct __attribute__((packed, aligned(4))) RngU4 { uint32_t x, y, z, w; }; /* 16 bytes at a word boundary: results[] starts at word 259 */

template <uint32_t SLOTS>
__global__ __launch_bounds__(64) void rng_prepare_kernel(uint32_t *states, const uint32_t *list) {
    extern __shared__ uint32_t rng_prep_stage[]; /* SLOTS x 256 words */
    const uint32_t lane = threadIdx.x;
    const uint32_t count = list[0];
    uint32_t *m = rng_prep_stage + lane;
    for (uint32_t first = blockIdx.x * SLOTS; first < count; first += gridDim.x * SLOTS) {
        if (lane >= SLOTS || first + lane >= count) continue;
        uint32_t *rec = states + (size_t)list[1u + first + lane] * RNG_WORDS;
        const uint32_t cur = rec[RNG_FLAGS] & 1u;
        const uint32_t *src = rec + cur * RNG_BANK_WORDS;
        uint32_t *dst = rec + (cur ^ 1u) * RNG_BANK_WORDS;
        for (uint32_t i = 0; i < 256u; i += 32u) { /* eight loads in flight */
            uint4 v[8];
#pragma unroll
            for (uint32_t j = 0; j < 8u; ++j) v[j] = *reinterpret_cast<const uint4 *>(src + RNG_MEM + i + 4u * j);
#pragma unroll
            for (uint32_t j = 0; j < 8u; ++j) {
                m[(i + 4u * j + 0u) * SLOTS] = v[j].x;
                m[(i + 4u * j + 1u) * SLOTS] = v[j].y;
                m[(i + 4u * j + 2u) * SLOTS] = v[j].z;
                m[(i + 4u * j + 3u) * SLOTS] = v[j].w;
            }
        }
        const uint32_t cc = src[RNG_C] + 1u;
        uint32_t a = src[RNG_A], b = src[RNG_B] + cc;
        for (uint32_t i = 0; i < 256u; i += 4u) {
            const uint32_t x0 = m[(i + 0u) * SLOTS], x1 = m[(i + 1u) * SLOTS], x2 = m[(i + 2u) * SLOTS], x3 = m[(i + 3u) * SLOTS];
            const uint32_t h0 = m[((i + 128u) & 255u) * SLOTS], h1 = m[((i + 129u) & 255u) * SLOTS], h2 = m[((i + 130u) & 255u) * SLOTS],
                           h3 = m[((i + 131u) & 255u) * SLOTS];
            RngU4 r;
#define RT_ISAAC_WIDE_STEP(K, X, H, MIX, OUT)                         \
            {                                                         \
                a = (a ^ (MIX)) + (H);                                \
                const uint32_t y = a + b + m[(((X) >> 2) & 255u) * SLOTS]; \
                m[(i + (K)) * SLOTS] = y;                             \
                b = (X) + m[((y >> 10) & 255u) * SLOTS];              \
                OUT = b;                                              \
            }
            RT_ISAAC_WIDE_STEP(0u, x0, h0, a << 13, r.w)
            RT_ISAAC_WIDE_STEP(1u, x1, h1, a >> 6, r.z)
            RT_ISAAC_WIDE_STEP(2u, x2, h2, a << 2, r.y)
            RT_ISAAC_WIDE_STEP(3u, x3, h3, a >> 16, r.x)
#undef RT_ISAAC_WIDE_STEP
            *reinterpret_cast<RngU4 *>(dst + RNG_RESULTS + 252u - i) = r; /* results[255 - i] = step i's word: read forwards */
        }
        for (uint32_t i = 0; i < 256u; i += 32u) {
#pragma unroll
            for (uint32_t j = 0; j < 8u; ++j) {
                uint4 v;
                v.x = m[(i + 4u * j + 0u) * SLOTS];
                v.y = m[(i + 4u * j + 1u) * SLOTS];
                v.z = m[(i + 4u * j + 2u) * SLOTS];
                v.w = m[(i + 4u * j + 3u) * SLOTS];
                *reinterpret_cast<uint4 *>(dst + RNG_MEM + i + 4u * j) = v;
            }
        }
        dst[RNG_A] = a;
        dst[RNG_B] = b;
        dst[RNG_C] = cc;
        rec[RNG_FLAGS] = cur | 2u;
    }
}

#ifndef RNG_PREP_SLOTS
#define RNG_PREP_SLOTS 64u /* records (and KB of LDS) of a one-wave workgroup; a multiple of 32, at most 64 */
#endif

hipError_t launch_rng_prepare(uint32_t *states, uint32_t n_pixels, uint32_t *list, uint32_t compute_units, hipStream_t stream) {
    if (n_pixels == 0u) return hipSuccess;
    hipError_t e = hipMemsetAsync(list, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rng_scan_kernel, dim3((n_pixels + 255u) / 256u), dim3(256), 0, stream, states, n_pixels, list);
    const uint32_t groups = std::min((n_pixels + RNG_PREP_SLOTS - 1u) / RNG_PREP_SLOTS, compute_units * (160u / RNG_PREP_SLOTS));
    hipLaunchKernelGGL((rng_prepare_kernel<RNG_PREP_SLOTS>), dim3(groups), dim3(64), RNG_PREP_SLOTS * 1024u, stream, states, list);
    return hipGetLastError();
}

/* the oracle's record of every pixel: bank `cur` + the position (rt_rng_download) */
__global__ __launch_bounds__(256) void rng_export_kernel(const uint32_t *states, uint32_t n_pixels, uint32_t *out) {
    const size_t n_words = (size_t)n_pixels * RNG_BANK_WORDS;
    for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (size_t)gridDim.x * blockDim.x) {
        const size_t p = w / RNG_BANK_WORDS;
        const uint32_t i = (uint32_t)(w - p * RNG_BANK_WORDS);
        const uint32_t *rec = states + p * RNG_WORDS;
        out[w] = i == RNG_SPARE ? rec[RNG_INDEX] : rec[(rec[RNG_FLAGS] & 1u) * RNG_BANK_WORDS + i];
    }
}

hipError_t launch_rng_export(const uint32_t *states, uint32_t n_pixels, uint32_t *out, hipStream_t stream) {
    if (n_pixels == 0u) return hipSuccess;
    hipLaunchKernelGGL(rng_export_kernel, dim3(4096), dim3(256), 0, stream, states, n_pixels, out);
    return hipGetLastError();
}

} /* namespace rt */

#include "rt_dist_kernels.h"

namespace rt {

hipError_t launch_distributed(const KernelScene &sc, const KernelFrame &fr, const DistParams &dp, uint32_t resident_waves, hipStream_t stream) {
    if (frame_is_rays(fr)) return launch_distributed_rays(sc, fr, dp, resident_waves, stream); /* rt_distributed_rays.hip */
    return launch_distributed_of<false>(sc, fr, dp, resident_waves, stream);
}
uint32_t dist_bfs_waves(uint32_t compute_units) { return compute_units * 4u * (uint32_t)RT_DIST_BFS_WAVES; }

/* get_shade (main.rs:407-464) for every request of the batch.  The request arrays are sparse — slot k of a sample is in
 * use only if its chain got that far (90 % at slot 0, a few per cent at slot 8) — so a workgroup first lists the live
 * (slot, sample) pairs of its `tile` samples in LDS and its waves then work through the list 64 at a time with
 * every lane busy.  No global atomics; the order within the list does not matter (each result has its own address) —
 * which is used a second time: a light behind the surface needs no shadow cast (main.rs:431), on average one of the
 * scene's three, and a wave skips a light only when none of its lanes needs it.  So the list is bucket-sorted by which of
 * the first three lights face the GEOMETRIC normal (a guess at the reference's test, which uses the material's adjusted
 * normal: it only orders the work), and most waves then hold requests that need the same lights. */
#define DIST_SHADE_BUCKETS 8u /* 3 bits: which of the first three lights face the surface */
#define DIST_SHADE_HDR (1u + 2u * DIST_SHADE_BUCKETS) /* words before the lists: [0] requests, bucket sizes -> starts, bucket cursors */
#ifndef RT_DIST_SHADE_MIN_WAVES
#define RT_DIST_SHADE_MIN_WAVES 6 /* 80 VGPRs; 4 / 5 / 8 measured in profiles/README.md */
#endif
#ifndef RT_DIST_SHADE_THREADS
#define RT_DIST_SHADE_THREADS 256
#endif
#ifdef RT_DIAG_PAIR_TIME
static __device__ unsigned long long g_shade_time[8]; /* wave ticks: [0] list building + sort, [1] request load + material, [2] lights -> directional + facing, [3] the cast, [4] diffuse / specular, [5] the kernel, [6] wave-casts */
extern "C" int rt_diag_read_shade_time(unsigned long long *out8, int reset) {
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(rt::g_shade_time), 8 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) { unsigned long long z[8] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(rt::g_shade_time), z, sizeof z) != hipSuccess) return -1; }
    return 0;
}
#define RT_SHADE_TICK(k) { const unsigned long long now_ = __builtin_readcyclecounter(); sdt[k] += now_ - stick; stick = now_; }
#else
#define RT_SHADE_TICK(k)
#endif
__global__ __launch_bounds__(RT_DIST_SHADE_THREADS, RT_DIST_SHADE_MIN_WAVES) void dist_shade_kernel(const KernelScene sc, const DistParams dp, const size_t n_samples, const uint32_t tile, const uint32_t list_cap, const uint32_t sort) {
    extern __shared__ uint32_t shade_lds[];
    uint32_t *const bucket_start = shade_lds + 1u, *const bucket_cursor = bucket_start + DIST_SHADE_BUCKETS;
    uint32_t *const unsorted = shade_lds + DIST_SHADE_HDR;       /* slot << 24 | bucket << 16 | sample - tile0 */
    uint32_t *const shade_list = unsorted + list_cap;            /* the same, bucket by bucket */
    const uint32_t lane = threadIdx.x & 63u;
    const size_t tile0 = (size_t)blockIdx.x * tile;
#ifdef RT_DIAG_PAIR_TIME
    unsigned long long sdt[7] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    unsigned long long stick = __builtin_readcyclecounter();
    const unsigned long long stick0 = stick;
#endif
    for (uint32_t k = threadIdx.x; k < DIST_SHADE_HDR; k += blockDim.x) shade_lds[k] = 0u;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < tile; i += blockDim.x) {
        if (tile0 + i < n_samples) {
            const uint32_t hdr = dp.sp_hdr[tile0 + i];
            const uint32_t cnt = (hdr & 0xffu) + ((hdr >> 8) & 1u);
            if (cnt != 0u) {
                const uint32_t base = atomicAdd(&shade_lds[0], cnt);
                for (uint32_t k = 0; k < cnt; ++k) unsorted[base + k] = (k << 24) | i;
            }
        }
    }
    __syncthreads();
    const uint32_t total = shade_lds[0];
    const uint32_t key_lights = sc.n_lights < 3u ? sc.n_lights : 3u;
    for (uint32_t e = threadIdx.x; e < total; e += blockDim.x) {
        const uint32_t entry = unsorted[e];
        uint32_t key = 0u;
        if (sort) {
            const uint4 *r = dp.sp_req + ((size_t)(entry >> 24) * n_samples + tile0 + (entry & 0xffffu)) * 4u;
            const uint4 a = r[0], b = r[1];
            const V3 pos = v3(duf(a.x), duf(a.y), duf(a.z)), normal = v3(duf(b.x), duf(b.y), duf(b.z));
            for (uint32_t l = 0; l < key_lights; ++l) {
                const auto &L = uniform_ref(sc.lights + l);
                const V3 toward = L.kind == RT_LIGHT_DIRECTIONAL ? v3(L.direction[0], L.direction[1], L.direction[2])
                                                                 : pos - v3(L.origin[0], L.origin[1], L.origin[2]);
                if (dot(toward, normal) < 0.0f) key |= 1u << l;
            }
        }
        unsorted[e] = entry | (key << 16);
        atomicAdd(&bucket_start[key], 1u);
    }
    __syncthreads();
    if (threadIdx.x < DIST_SHADE_BUCKETS) { /* sizes -> starts */
        uint32_t before = 0u;
        for (uint32_t k = 0; k < threadIdx.x; ++k) before += bucket_start[k];
        bucket_cursor[threadIdx.x] = before;
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < total; e += blockDim.x) {
        const uint32_t entry = unsorted[e];
        shade_list[atomicAdd(&bucket_cursor[(entry >> 16) & (DIST_SHADE_BUCKETS - 1u)], 1u)] = entry;
    }
    __syncthreads();
    uint32_t casts = 0u;
    RT_SHADE_TICK(0)
    for (uint32_t first = (threadIdx.x >> 6) * 64u; first < total; first += blockDim.x) {
        const bool active = first + lane < total;
        V3 pos = v3(0.0f, 0.0f, 0.0f), normal = v3(0.0f, 0.0f, 1.0f), view = v3(0.0f, 0.0f, 1.0f);
        float u = 0.0f, v = 0.0f;
        uint32_t obj = 0u, prim = 0u;
        size_t at = 0;
        if (active) {
            const uint32_t e = shade_list[first + lane];
            at = (size_t)(e >> 24) * n_samples + tile0 + (e & 0xffffu);
            const uint4 *r = dp.sp_req + at * 4u;
            const uint4 a = r[0], b = r[1], c = r[2], d = r[3];
            pos = v3(duf(a.x), duf(a.y), duf(a.z)); u = duf(a.w);
            normal = v3(duf(b.x), duf(b.y), duf(b.z)); v = duf(b.w);
            view = v3(duf(c.x), duf(c.y), duf(c.z)); obj = c.w;
            prim = d.x;
        }
        const Mat m = material_approx(sc.materials[obj], u, v);
        const V3 adj_n = adjust_normal(m.normal, normal); /* main.rs:410 */
        V3 sum = v3(0.0f, 0.0f, 0.0f);
        RT_SHADE_TICK(1)
        for (uint32_t light_i = 0; light_i < sc.n_lights; ++light_i) { /* wave-uniform */
            const auto &L = uniform_ref(sc.lights + light_i);
            /* does the light ask for a shadow cast (main.rs:413-433)?  light_asks answers without a spot light's acos wherever the
             * angle is clear of the cone's edge (rt_shade.h); the light's colour — a spot light's powf — waits for the lit lanes */
            V3 l_direction = v3(0.0f, 0.0f, 0.0f);
            const bool need = light_asks(L, uniform_ref(sc.light_aux + light_i), pos, adj_n, &l_direction) && active;
            RT_SHADE_TICK(2)
            if (__builtin_amdgcn_ballot_w64(need) == 0ull) continue;
            Ray req;
            req.o = pos;
            req.d = -l_direction;
            req.mode = FACE_BACK;
            req.excl = pack_excl(prim, FACE_BACK);
            CastResult cr;
            cr.prim = -1;
            cr.t = 0.0f;
            cr.bf = 0u;
            cr.a0 = cr.a1 = cr.a2 = 0.0f;
            if (need) cr = cast_asm(sc, req);
#ifdef RT_DIAG_PAIR_TIME
            RT_SHADE_TICK(3)
            sdt[6] += 1ull;
#endif
            if (need) {
                casts += 1u;
                bool lit = true;
                if (cr.prim >= 0) {
                    const bool has_origin = (L.kind != RT_LIGHT_DIRECTIONAL) || (L.has_origin != 0u);
                    if (has_origin) {
                        const V3 occ = req.o + req.d * cr.t;
                        if (distance(pos, occ) < distance(pos, v3(L.origin[0], L.origin[1], L.origin[2]))) lit = false;
                    } else {
                        lit = false;
                    }
                }
                if (lit) {
                    DirLight dl;
                    dl.direction = dl.color = v3(0.0f, 0.0f, 0.0f);
                    (void)approximate_into_directional(L, pos, &dl); /* the light asked: Some */
                    const V3 light_direction = req.d;
                    const V3 diffuse = get_diffuse(m, adj_n, light_direction) * dl.color;
                    const V3 specular = get_specular(m, adj_n, -view, light_direction) * dl.color;
                    sum = sum + diffuse * (1.0f - m.shiness) + specular * m.shiness;
                }
            }
            RT_SHADE_TICK(4)
        }
        if (active) dp.sp_shade[at] = make_float4(sum.x, sum.y, sum.z, 0.0f);
    }
#ifdef RT_DIAG_PAIR_TIME
    sdt[5] = __builtin_readcyclecounter() - stick0;
    if (lane == 0u) for (int q = 0; q < 7; ++q) atomicAdd(&g_shade_time[q], sdt[q]);
#endif
    if (dp.ray_count != nullptr) {
        for (int off = 32; off > 0; off >>= 1) casts += __shfl_down(casts, off, 64);
        if (lane == 0u && casts != 0u) atomicAdd(dp.ray_count, (unsigned long long)casts);
    }
}

/* the unwind (main.rs:571, 590, 605), the sample filter (main.rs:1157-1160) and the accumulation (main.rs:1165) */
__global__ __launch_bounds__(256) void dist_unwind_kernel(const DistParams dp, const size_t n_pixels, const size_t call_pixels_stride) {
    const size_t n_samples = n_pixels * dp.n_epochs;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pixels; p += (size_t)gridDim.x * blockDim.x) {
        V3 accum = v3(0.0f, 0.0f, 0.0f);
        uint32_t cost = 0u; /* of the pixel's samples of this batch: a cast per level and the primary one */
        if (dp.accum != nullptr) accum = v3(dp.accum[p * 3u], dp.accum[p * 3u + 1u], dp.accum[p * 3u + 2u]);
        for (uint32_t e = 0; e < dp.n_epochs; ++e) {
            const size_t s = (size_t)e * n_pixels + p;
            const uint32_t hdr = dp.sp_hdr[s];
            const uint32_t frames = hdr & 0xffu;
            cost += frames + 1u;
            V3 value = v3(0.0f, 0.0f, 0.0f);
            if ((hdr >> 8) & 1u) {
                const float4 t = dp.sp_shade[(size_t)frames * n_samples + s];
                value = v3(t.x, t.y, t.z);
            }
            for (uint32_t k = frames; k-- > 0u;) {
                const float4 f = dp.sp_frame[(size_t)k * n_samples + s];
                const float4 sh4 = dp.sp_shade[(size_t)k * n_samples + s];
                const V3 shade = v3(sh4.x, sh4.y, sh4.z);
                if (dfu(f.w) == 2u) {
                    value = (value + shade) * f.x; /* main.rs:605 */
                } else {
                    const V3 sc_ = value * v3(f.x, f.y, f.z);  /* main.rs:566, 585 */
                    value = shade + (sc_ - shade) * 0.5f;       /* palette Mix::mix(&s, 0.5), main.rs:571, 590 */
                }
            }
            const bool ok = rtdm::is_normal(value.x) && rtdm::is_normal(value.y) && rtdm::is_normal(value.z);
            const size_t o = ((size_t)(dp.epoch0 + e)) * call_pixels_stride + p;
            if (dp.samples != nullptr) {
                dp.samples[o * 3u] = value.x;
                dp.samples[o * 3u + 1u] = value.y;
                dp.samples[o * 3u + 2u] = value.z;
            }
            if (dp.valid != nullptr) dp.valid[o] = ok ? 1 : 0;
            if (ok) accum = accum + value;
        }
        if (dp.accum != nullptr) {
            dp.accum[p * 3u] = accum.x;
            dp.accum[p * 3u + 1u] = accum.y;
            dp.accum[p * 3u + 2u] = accum.z;
        }
        if (dp.pixel_cost != nullptr) dp.pixel_cost[p] = (cost * 8u + dp.n_epochs - 1u) / dp.n_epochs; /* eighths of a cast per sample */
    }
}

/* ---- the chain kernel's pixels grouped by cost (rt_kernels.h DistParams::pixel_order): a counting sort in three launches ----
 * scratch[0..255] the histogram, scratch[256..511] the buckets' cursors; dearest first; the order within a bucket is whatever the
 * atomics make it (it only orders work) */
#define DIST_ORDER_CHUNK 4096u
__global__ __launch_bounds__(256) void dist_order_hist_kernel(const uint32_t *cost, uint32_t n, uint32_t *scratch) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t first = blockIdx.x * DIST_ORDER_CHUNK;
    for (uint32_t i = first + threadIdx.x; i < first + DIST_ORDER_CHUNK && i < n; i += 256u) atomicAdd(&h[cost[i] < 255u ? cost[i] : 255u], 1u);
    __syncthreads();
    if (h[threadIdx.x] != 0u) atomicAdd(&scratch[threadIdx.x], h[threadIdx.x]);
}
__global__ __launch_bounds__(256) void dist_order_scan_kernel(uint32_t *scratch) {
    if (threadIdx.x == 0u) {
        uint32_t sum = 0u;
        for (int b = 255; b >= 0; --b) { scratch[256 + b] = sum; sum += scratch[b]; }
    }
}
__global__ __launch_bounds__(256) void dist_order_scatter_kernel(const uint32_t *cost, uint32_t n, uint32_t *scratch, uint32_t *order) {
    __shared__ uint32_t h[256], base[256];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t first = blockIdx.x * DIST_ORDER_CHUNK;
    for (uint32_t i = first + threadIdx.x; i < first + DIST_ORDER_CHUNK && i < n; i += 256u) atomicAdd(&h[cost[i] < 255u ? cost[i] : 255u], 1u);
    __syncthreads();
    base[threadIdx.x] = h[threadIdx.x] != 0u ? atomicAdd(&scratch[256u + threadIdx.x], h[threadIdx.x]) : 0u; /* this workgroup's stretch of the bucket */
    __syncthreads();
    for (uint32_t i = first + threadIdx.x; i < first + DIST_ORDER_CHUNK && i < n; i += 256u) {
        const uint32_t b = cost[i] < 255u ? cost[i] : 255u;
        order[atomicAdd(&base[b], 1u)] = i;
    }
}

hipError_t launch_dist_pixel_order(const uint32_t *cost, uint32_t *order, uint32_t n_pixels, uint32_t *scratch, hipStream_t stream) {
    if (n_pixels == 0u) return hipSuccess;
    hipError_t e = hipMemsetAsync(scratch, 0, 256u * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const uint32_t groups = (n_pixels + DIST_ORDER_CHUNK - 1u) / DIST_ORDER_CHUNK;
    hipLaunchKernelGGL(dist_order_hist_kernel, dim3(groups), dim3(256), 0, stream, cost, n_pixels, scratch);
    hipLaunchKernelGGL(dist_order_scan_kernel, dim3(1), dim3(256), 0, stream, scratch);
    hipLaunchKernelGGL(dist_order_scatter_kernel, dim3(groups), dim3(256), 0, stream, cost, n_pixels, scratch, order);
    return hipGetLastError();
}

size_t distributed_split_bytes_per_sample(int32_t max_depth) {
    const size_t d = (size_t)(max_depth > 0 ? max_depth : 0);
    return sizeof(uint32_t) + (d + 1u) * (4u * sizeof(uint4) + sizeof(float4)) + d * sizeof(float4);
}

/* one batch of dp.n_epochs epochs (dp.epoch0 = its first epoch within the call) in two halves, so that a caller may put them on
 * different streams: the chain kernel (dp.work_queue zeroed) ... */
/* the waves the chain kernel's grid has at most: as many as are resident together */
uint32_t dist_chain_waves(uint32_t resident_waves) {
    return resident_waves / 3u * (uint32_t)RT_DIST_CHAIN_MIN_WAVES; /* resident_waves is sized for 3 per SIMD */
}

hipError_t launch_dist_chain(const KernelScene &sc, const KernelFrame &fr, const DistParams &dp, uint32_t resident_waves, hipStream_t stream) {
    if (frame_is_rays(fr)) return launch_dist_chain_rays(sc, fr, dp, resident_waves, stream); /* rt_distributed_rays.hip */
    return launch_dist_chain_of<false>(sc, fr, dp, resident_waves, stream);
}

/* ... and what only reads its records: the shade kernel and the unwind */
hipError_t launch_dist_shade_unwind(const KernelScene &sc, const KernelFrame &fr, const DistParams &dp, hipStream_t stream, const hipEvent_t *ev) {
    const uint32_t total = fr.cols * fr.rows;
    if (total == 0u || dp.n_epochs == 0u) return hipSuccess;
    const size_t n_samples = (size_t)total * dp.n_epochs;
    const uint32_t slots = (uint32_t)(fr.max_depth > 0 ? fr.max_depth : 0) + 1u;
    if (ev != nullptr) (void)hipEventRecord(ev[0], stream); /* profiling: [0, 1] around the shade kernel, [2, 3] around the unwind */
    {
        uint32_t tile = 256u; /* samples per workgroup (18 KB of LDS at depth 8: six workgroups per CU); the two lists must fit 48 KB */
        const uint32_t sort = 1u; /* the bucket sort by facing lights (profiles/README.md) */
        while (tile > 32u && (DIST_SHADE_HDR + 2u * (size_t)tile * slots) * sizeof(uint32_t) > 49152u) tile >>= 1;
        const size_t shade_tiles = (n_samples + tile - 1u) / tile;
        const uint32_t list_cap = tile * slots;
        const size_t shade_lds = (DIST_SHADE_HDR + 2u * (size_t)list_cap) * sizeof(uint32_t);
        hipLaunchKernelGGL(dist_shade_kernel, dim3((unsigned)shade_tiles), dim3(RT_DIST_SHADE_THREADS), shade_lds, stream, sc, dp, n_samples, tile, list_cap, sort);
    }
    if (ev != nullptr) { (void)hipEventRecord(ev[1], stream); (void)hipEventRecord(ev[2], stream); }
    size_t blocks = ((size_t)total + 255u) / 256u;
    if (blocks > 4096u) blocks = 4096u;
    /* samples and flags are indexed with the CALL's count: a band of a ray batch is a part of it (frame_sample_stride) */
    hipLaunchKernelGGL(dist_unwind_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, dp, (size_t)total,
                       frame_is_rays(fr) ? (size_t)frame_sample_stride(fr) : (size_t)total);
    if (ev != nullptr) (void)hipEventRecord(ev[3], stream);
    return hipGetLastError();
}

} /* namespace rt */
#ifdef RT_DIAG_NEED
RT_DIAG_NEED_READER(rt_diag_read_need_dist)
#endif
#ifdef RT_DIAG_PAIR_TIME
RT_DIAG_PAIR_TIME_READER(rt_diag_read_pair_time)
#endif
#ifdef RT_DIAG_PREPARE
/* diagnostic build (tools/diag_prepare.py): the look-ahead pass alone over n freshly seeded records, `reps` times (the
 * prepared flags cleared in between); ms_out[0] = average ms of scan + prepare, ms_out[1] = of the scan alone */
namespace rt {
__global__ void rng_diag_unprepare_kernel(uint32_t *states, uint32_t n) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) states[(size_t)p * RNG_WORDS + RNG_FLAGS] &= 1u;
}
}
extern "C" int rt_diag_prepare_time(uint32_t n_records, uint32_t reps, uint32_t compute_units, float *ms_out) {
    uint32_t *states = nullptr, *list = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&states), (size_t)n_records * rt::RNG_WORDS * sizeof(uint32_t)) != hipSuccess) return -1;
    if (hipMalloc(reinterpret_cast<void **>(&list), ((size_t)n_records + 1u) * sizeof(uint32_t)) != hipSuccess) return -1;
    rt::KernelFrame fr = {};
    fr.cols = n_records; fr.rows = 1u; fr.y_step = 1u;
    if (rt::launch_rng_seed(states, fr, nullptr) != hipSuccess) return -2;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    float total = 0.0f, scan = 0.0f;
    for (uint32_t r = 0; r < reps + 1u; ++r) { /* the first is a warm-up */
        hipLaunchKernelGGL(rt::rng_diag_unprepare_kernel, dim3((n_records + 255u) / 256u), dim3(256), 0, nullptr, states, n_records);
        hipEventRecord(e0, nullptr);
        if (rt::launch_rng_prepare(states, n_records, list, compute_units, nullptr) != hipSuccess) return -3;
        hipEventRecord(e1, nullptr);
        hipEventSynchronize(e1);
        float ms = 0.0f;
        hipEventElapsedTime(&ms, e0, e1);
        if (r > 0u) total += ms;
        hipEventRecord(e0, nullptr);
        if (rt::launch_rng_prepare(states, n_records, list, compute_units, nullptr) != hipSuccess) return -3; /* nothing left to prepare */
        hipEventRecord(e1, nullptr);
        hipEventSynchronize(e1);
        hipEventElapsedTime(&ms, e0, e1);
        if (r > 0u) scan += ms;
    }
    ms_out[0] = total / (float)reps;
    ms_out[1] = scan / (float)reps;
    hipEventDestroy(e0); hipEventDestroy(e1);
    (void)hipFree(states); (void)hipFree(list);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}
#endif
