/*
 * rt_rng.h — the generator of the stochastic pass: rand 0.5's IsaacRng (ISAAC-32) over a per-pixel record in HBM, Uniform<f32> and the
 * ziggurat StandardNormal, restated from the crate's published algorithms (rt_distributed.hip says how they are pinned).  Device code only.
 *
 * Included by every unit that draws: rt_distributed.hip (its RNG kernels, and through rt_dist_kernels.h), rt_distributed_rays.hip and
 * rt_scatter_query.hip.  isaac_seed, isaac_generate, isaac_generate_staged and standard_normal are not inline and ZIG_X / ZIG_F are
 * device constants: each including unit's code object gets its own copy of them (the units are not linked on the device).
 */
#ifndef RT_RNG_H
#define RT_RNG_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_kernels.h"
#include "rt_detmath.h"
#include "rt_ziggurat_tables.h"

namespace rt {

/* ---- per-pixel RNG record in HBM ----------------------------------------------------------------------------------
 * Two BANKS of the oracle's layout (mem[256], a, b, c, results[256], one spare word).  Bank `cur` is the generator's
 * state as the reference has it (IsaacRng: the block in use + the position in it); the other bank, when `prepared`, holds
 * the state after the NEXT IsaacCore::generate, computed ahead of time by rng_prepare_kernel.  A lane that runs dry then
 * just switches banks.  Why: generate is 256 steps with two address-dependent loads each — tens of microseconds for one
 * lane with the 63 others of its wave waiting, and after a few dozen epochs the pixels' streams are out of step, so in
 * the render kernels it is always ONE lane (measured: a third of the chain kernel's wave time).  In the prepare pass all
 * the lanes of a wave generate together.  rt_rng_download exports bank `cur` + the position: the oracle's record. */
enum : uint32_t {
    RNG_MEM = 0u, RNG_A = 256u, RNG_B = 257u, RNG_C = 258u, RNG_RESULTS = 259u, RNG_SPARE = 515u, RNG_BANK_WORDS = 516u,
    RNG_INDEX = RNG_SPARE,                      /* bank 0's spare word: position in the current block (256 = used up) */
    RNG_FLAGS = RNG_BANK_WORDS + RNG_SPARE,     /* bank 1's spare word: bit 0 = cur, bit 1 = prepared */
    RNG_WORDS = 2u * RNG_BANK_WORDS
};
static_assert(RNG_WORDS == RT_RNG_DEVICE_WORDS && RNG_BANK_WORDS == RT_RNG_STATE_WORDS, "rt_kernels.h");

__device__ const double ZIG_X[257] = RT_ZIG_NORM_X;
__device__ const double ZIG_F[257] = RT_ZIG_NORM_F;

/* IsaacCore::init(key, rounds = 1) as called by IsaacRng::new_from_u64(seed) */
__device__ void isaac_seed(uint32_t *st, unsigned long long seed) {
    for (uint32_t i = 0; i < 256u; ++i) st[RNG_MEM + i] = 0u;
    st[RNG_MEM + 0] = (uint32_t)seed;
    st[RNG_MEM + 1] = (uint32_t)(seed >> 32);
    uint32_t a = 0x1367df5au, b = 0x95d90059u, c = 0xc3163e4bu, d = 0x0f421ad8u;
    uint32_t e = 0xd92a4a78u, f = 0xa51a3c49u, g = 0xc4efea1bu, h = 0x30609119u;
    for (uint32_t i = 0; i < 256u; i += 8u) {
        a += st[i]; b += st[i + 1]; c += st[i + 2]; d += st[i + 3];
        e += st[i + 4]; f += st[i + 5]; g += st[i + 6]; h += st[i + 7];
        a ^= b << 11; d += a; b += c;
        b ^= c >> 2;  e += b; c += d;
        c ^= d << 8;  f += c; d += e;
        d ^= e >> 16; g += d; e += f;
        e ^= f << 10; h += e; f += g;
        f ^= g >> 4;  a += f; g += h;
        g ^= h << 8;  b += g; h += a;
        h ^= a >> 9;  c += h; a += b;
        st[i] = a; st[i + 1] = b; st[i + 2] = c; st[i + 3] = d;
        st[i + 4] = e; st[i + 5] = f; st[i + 6] = g; st[i + 7] = h;
    }
    st[RNG_A] = 0u;
    st[RNG_B] = 0u;
    st[RNG_C] = 0u;
    for (uint32_t i = 0; i < 256u; ++i) st[RNG_RESULTS + i] = 0u;
    st[RNG_INDEX] = 256u;
    st[RNG_FLAGS] = 0u; /* bank 0 is current, nothing prepared */
}

/* IsaacCore::generate from bank `src` into bank `dst` (results stored backwards: read forwards = the reference
 * implementation's order) */
__device__ void isaac_generate(const uint32_t *src, uint32_t *dst) {
    for (uint32_t i = 0; i < 256u; i += 4u) *reinterpret_cast<uint4 *>(dst + RNG_MEM + i) = *reinterpret_cast<const uint4 *>(src + RNG_MEM + i);
    const uint32_t cc = src[RNG_C] + 1u;
    dst[RNG_C] = cc;
    uint32_t a = src[RNG_A], b = src[RNG_B] + cc;
    for (uint32_t i = 0; i < 256u; ++i) {
        const uint32_t x = dst[RNG_MEM + i];
        const uint32_t sel = i & 3u;
        const uint32_t mixv = sel == 0u ? (a ^ (a << 13)) : sel == 1u ? (a ^ (a >> 6)) : sel == 2u ? (a ^ (a << 2)) : (a ^ (a >> 16));
        a = mixv + dst[RNG_MEM + ((i + 128u) & 255u)];
        const uint32_t y = a + b + dst[RNG_MEM + ((x >> 2) & 255u)];
        dst[RNG_MEM + i] = y;
        b = x + dst[RNG_MEM + ((y >> 10) & 255u)];
        dst[RNG_RESULTS + 255u - i] = b;
    }
    dst[RNG_A] = a;
    dst[RNG_B] = b;
}

/* The steps of generate on a mem[] staged in LDS, slot-interleaved (word i of slot k at i * SLOTS + k: the lanes'
 * accesses to the same i fall in different banks); results go straight to `dst`. */
#define RNG_LDS_SLOTS 8u
__device__ __forceinline__ void isaac_steps_lds(uint32_t *m, const uint32_t *src, uint32_t *dst) {
    const uint32_t cc = src[RNG_C] + 1u;
    dst[RNG_C] = cc;
    uint32_t a = src[RNG_A], b = src[RNG_B] + cc;
#define RT_ISAAC_STEP(I, MIX)                                                     \
    {                                                                             \
        const uint32_t x = m[(I) * RNG_LDS_SLOTS];                                \
        a = (a ^ (MIX)) + m[(((I) + 128u) & 255u) * RNG_LDS_SLOTS];               \
        const uint32_t y = a + b + m[((x >> 2) & 255u) * RNG_LDS_SLOTS];          \
        m[(I) * RNG_LDS_SLOTS] = y;                                               \
        b = x + m[((y >> 10) & 255u) * RNG_LDS_SLOTS];                            \
        dst[RNG_RESULTS + 255u - (I)] = b;                                        \
    }
    for (uint32_t i = 0; i < 256u; i += 4u) {
        RT_ISAAC_STEP(i, a << 13)
        RT_ISAAC_STEP(i + 1u, a >> 6)
        RT_ISAAC_STEP(i + 2u, a << 2)
        RT_ISAAC_STEP(i + 3u, a >> 16)
    }
#undef RT_ISAAC_STEP
    dst[RNG_A] = a;
    dst[RNG_B] = b;
}

/* generate for the lanes of a render wave that run dry WITHOUT a prepared bank (a pixel that used more than a whole
 * block within one visit — rare): a divergent branch, usually one lane.  mem[] goes through LDS, up to RNG_LDS_SLOTS
 * lanes at a time; more than 2 * SLOTS lanes at once take the HBM version, all in parallel. */
__device__ void isaac_generate_staged(const uint32_t *src, uint32_t *dst, uint32_t *lds) {
    const unsigned long long all = __builtin_amdgcn_ballot_w64(true);
    if (lds == nullptr || (uint32_t)__builtin_popcountll(all) > 2u * RNG_LDS_SLOTS) {
        isaac_generate(src, dst);
        return;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t rank = (uint32_t)__builtin_popcountll(all & ((1ull << lane) - 1ull));
    for (uint32_t first = 0u; first < 2u * RNG_LDS_SLOTS; first += RNG_LDS_SLOTS) {
        if (rank < first || rank >= first + RNG_LDS_SLOTS) continue;
        uint32_t *m = lds + (rank - first);
        for (uint32_t i = 0; i < 256u; i += 4u) {
            const uint4 v = *reinterpret_cast<const uint4 *>(src + RNG_MEM + i);
            m[(i + 0u) * RNG_LDS_SLOTS] = v.x;
            m[(i + 1u) * RNG_LDS_SLOTS] = v.y;
            m[(i + 2u) * RNG_LDS_SLOTS] = v.z;
            m[(i + 3u) * RNG_LDS_SLOTS] = v.w;
        }
        isaac_steps_lds(m, src, dst);
        for (uint32_t i = 0; i < 256u; i += 4u) {
            uint4 v;
            v.x = m[(i + 0u) * RNG_LDS_SLOTS];
            v.y = m[(i + 1u) * RNG_LDS_SLOTS];
            v.z = m[(i + 2u) * RNG_LDS_SLOTS];
            v.w = m[(i + 3u) * RNG_LDS_SLOTS];
            *reinterpret_cast<uint4 *>(dst + RNG_MEM + i) = v;
        }
    }
}

/* BlockRng over the record; position and flags live in registers while a lane works on the pixel */
struct Rng {
    uint32_t *rec;  /* the pixel's record */
    uint32_t *st;   /* its current bank */
    uint32_t index;
    uint32_t flags; /* bit 0 = cur, bit 1 = prepared */
    uint32_t *lds;  /* the wave's RNG_LDS_SLOTS x 256 words of staging, or nullptr */
};
__device__ __forceinline__ void rng_open(Rng &r, uint32_t *rec) {
    r.rec = rec;
    r.index = rec[RNG_INDEX];
    r.flags = rec[RNG_FLAGS];
    r.st = rec + (r.flags & 1u) * RNG_BANK_WORDS;
}
__device__ __forceinline__ void rng_park(Rng &r) {
    r.rec[RNG_INDEX] = r.index;
    r.rec[RNG_FLAGS] = r.flags;
}
/* the current block is used up: move on to the next one (IsaacCore::generate, BlockRng::generate_and_set) */
__device__ __forceinline__ void rng_refill(Rng &r) {
    uint32_t *other = r.rec + ((r.flags & 1u) ^ 1u) * RNG_BANK_WORDS;
    if ((r.flags & 2u) == 0u) isaac_generate_staged(r.st, other, r.lds);
    r.st = other;
    r.flags = (r.flags & 1u) ^ 1u;
}
__device__ __forceinline__ uint32_t next_u32(Rng &r) {
    if (r.index >= 256u) { rng_refill(r); r.index = 0u; }
    return r.st[RNG_RESULTS + r.index++];
}
__device__ __forceinline__ unsigned long long next_u64(Rng &r) {
    if (r.index < 255u) {
        const unsigned long long x = r.st[RNG_RESULTS + r.index], y = r.st[RNG_RESULTS + r.index + 1u];
        r.index += 2u;
        return (y << 32) | x;
    } else if (r.index >= 256u) {
        rng_refill(r);
        r.index = 2u;
        return ((unsigned long long)r.st[RNG_RESULTS + 1] << 32) | r.st[RNG_RESULTS + 0];
    } else {
        const unsigned long long x = r.st[RNG_RESULTS + 255];
        rng_refill(r);
        r.index = 1u;
        return ((unsigned long long)r.st[RNG_RESULTS + 0] << 32) | x;
    }
}
/* rand 0.5 UniformFloat<f32>::sample_single: 23 random bits -> [1,2), then * scale + offset */
__device__ __forceinline__ float gen_range_f32(Rng &r, float low, float high) {
    const float scale = high - low;
    const float offset = low - scale;
    const float value1_2 = rtdm::f32_from_bits((next_u32(r) >> 9) | 0x3f800000u);
    return value1_2 * scale + offset;
}
/* the same from a word already drawn */
__device__ __forceinline__ float range_f32_of(uint32_t word, float low, float high) {
    const float scale = high - low;
    const float offset = low - scale;
    const float value1_2 = rtdm::f32_from_bits((word >> 9) | 0x3f800000u);
    return value1_2 * scale + offset;
}
/* the next three words of the stream: when they are in the current block, three loads in flight together instead of three
 * load latencies one after the other (a pixel's block is out of the caches again between two visits) */
__device__ __forceinline__ void next_u32x3(Rng &r, uint32_t *w0, uint32_t *w1, uint32_t *w2) {
    if (r.index <= 253u) {
        const uint32_t *p = r.st + RNG_RESULTS + r.index;
        *w0 = p[0];
        *w1 = p[1];
        *w2 = p[2];
        r.index += 3u;
    } else {
        *w0 = next_u32(r);
        *w1 = next_u32(r);
        *w2 = next_u32(r);
    }
}
__device__ __forceinline__ double open01_f64(Rng &r) {
    const unsigned long long fraction = next_u64(r) >> 12;
    return rtdm::f64_from_bits(fraction | 0x3ff0000000000000ull) - (1.0 - 2.220446049250313e-16 / 2.0);
}
__device__ __forceinline__ double standard_f64(Rng &r) { return (1.0 / 9007199254740992.0) * (double)(next_u64(r) >> 11); }

/* StandardNormal: ziggurat(symmetric), rand 0.5 distributions/mod.rs */
__device__ double standard_normal(Rng &r) {
    for (;;) {
        const unsigned long long bits = next_u64(r);
        const uint32_t i = (uint32_t)(bits & 0xffull);
        const double u = rtdm::f64_from_bits((bits >> 12) | 0x4000000000000000ull) - 3.0;
        const double x = u * ZIG_X[i];
        const double test_x = x < 0.0 ? -x : x;
        if (test_x < ZIG_X[i + 1u]) return x;
        if (i == 0u) {
            double xx = 1.0, yy = 0.0;
            while (-2.0 * yy < xx * xx) {
                const double x_ = open01_f64(r);
                const double y_ = open01_f64(r);
                xx = rtdm::log_pos(x_) / RT_ZIG_NORM_R;
                yy = rtdm::log_pos(y_);
            }
            return u < 0.0 ? xx - RT_ZIG_NORM_R : RT_ZIG_NORM_R - xx;
        }
        const double z = -x * x / 2.0;
        const double pdf = z < -700.0 ? 0.0 : rtdm::exp_mid(z);
        if (ZIG_F[i + 1u] + (ZIG_F[i] - ZIG_F[i + 1u]) * standard_f64(r) < pdf) return x;
    }
}

/* the ziggurat's immediate accept (98.8 % of the draws) on 64 bits already drawn; false: the caller takes standard_normal */
__device__ __forceinline__ bool standard_normal_fast(unsigned long long bits, double *out) {
    const uint32_t i = (uint32_t)(bits & 0xffull);
    const double u = rtdm::f64_from_bits((bits >> 12) | 0x4000000000000000ull) - 3.0;
    const double x = u * ZIG_X[i];
    const double test_x = x < 0.0 ? -x : x;
    *out = x;
    return test_x < ZIG_X[i + 1u];
}

/* two StandardNormal draws in stream order.  Usually both accept at once and their four words are in the current block:
 * then the four loads travel together; otherwise redo both the ordinary way from the same position (same draws). */
__device__ __forceinline__ void standard_normal_x2(Rng &r, double *n0, double *n1) {
    if (r.index <= 252u) {
        const uint32_t *p = r.st + RNG_RESULTS + r.index;
        const unsigned long long a0 = p[0], a1 = p[1], a2 = p[2], a3 = p[3];
        double x0, x1;
        const bool f0 = standard_normal_fast((a1 << 32) | a0, &x0), f1 = standard_normal_fast((a3 << 32) | a2, &x1);
        if (f0 && f1) {
            *n0 = x0;
            *n1 = x1;
            r.index += 4u;
            return;
        }
    }
    *n0 = standard_normal(r);
    *n1 = standard_normal(r);
}

} /* namespace rt */

#endif /* RT_RNG_H */
