/*
 * rt_order_query.hip — the order of a batch of records (include/rt_amd.h "record ordering"): a coherence key per ray, a stable radix sort
 * of an index list by caller keys, and a gather and a scatter of fixed-size records through such a list.  Every query block says that a
 * wave takes 64 consecutive records and that rays which travel together should be neighbours; this unit builds the list that makes them so,
 * on the device, stream-ordered, without a workspace of its own.
 *
 *   rt::ray_keys_kernel       one ray per lane: the origin's cell in a 64^3 grid over the caller's box (18 bits, Z-order) and the
 *                             direction's cell in a 64^2 grid over the octahedral map (12 bits, Z-order)
 *   rt::sort_count_kernel     one workgroup per tile: how many entries of the tile fall into each of the 257 buckets of this pass's digit
 *                             (256 digit values, and one bucket behind them for entries that name no record); the first pass reads the
 *                             caller's list and keys and leaves (key field, index) pairs in the workspace
 *   rt::sort_scan_kernel      one workgroup: the exclusive sum over (bucket, tile), bucket-major — a bucket's entries of tile t start there
 *   rt::sort_scatter_kernel   the same tiles again: a wave owns 64 consecutive entries per step; its base per bucket is the scan's plus
 *                             the counts of the waves before it (LDS), a lane's rank the number of lanes below it with the same digit
 *                             (nine ballots) — equal digits keep their order, and nothing is ordered by an atomic
 *   rt::gather_records_kernel / rt::scatter_records_kernel   one dword per lane: dst[j] = src[index[j]], dst[index[j]] = src[j]
 *
 * The counts are sums of integers (LDS atomics: any order gives the same sum); every position is count-derived, so the same inputs give
 * the same output.  The key's arithmetic is single f32 operations in the documented order (the unit is compiled with -ffp-contract=off
 * like every other, and hipcc's f32 divide is correctly rounded); records move as dwords; every store is a vector store.  The C entry
 * points of the block are at the end of the file.
 */
#include "rt_api_internal.h"

namespace rt {

/* ---- coherence keys ---- */

#define RT_ORDER_THREADS 256u
#define RT_ORDER_RAY_WORDS 11u

struct OrderBox {
    float lo[3], scale[3];
};

/* the cell of a scaled coordinate: NaN and negatives 0, 63 and beyond 63, truncation between */
__device__ __forceinline__ uint32_t order_cell(float t) {
    if (!(t >= 0.0f)) return 0u;
    if (t >= 63.0f) return 63u;
    return (uint32_t)t;
}

/* bit k of a 6-bit value to bit 3k (spread3) or 2k (spread2) */
__device__ __forceinline__ uint32_t order_spread3(uint32_t v) {
    uint32_t r = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 6u; ++k) r |= ((v >> k) & 1u) << (3u * k);
    return r;
}
__device__ __forceinline__ uint32_t order_spread2(uint32_t v) {
    uint32_t r = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 6u; ++k) r |= ((v >> k) & 1u) << (2u * k);
    return r;
}

__device__ __forceinline__ float order_sg(float x) { return x >= 0.0f ? 1.0f : -1.0f; }

__global__ __launch_bounds__(RT_ORDER_THREADS) void ray_keys_kernel(const rt_ray *__restrict__ rays, const uint64_t n, const OrderBox box,
                                                                    const uint32_t direction_major, uint32_t *__restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_ORDER_THREADS + threadIdx.x;
    if (i >= n) return;
    const float *const r = reinterpret_cast<const float *>(rays) + i * RT_ORDER_RAY_WORDS; /* origin 0..2, direction 3..5; nothing else is read */
    uint32_t c[3];
#pragma unroll
    for (uint32_t a = 0; a < 3u; ++a) c[a] = order_cell((r[a] - box.lo[a]) * box.scale[a]);
    const float dx = r[3], dy = r[4], dz = r[5];
    const float s = (fabsf(dx) + fabsf(dy)) + fabsf(dz);
    float px = dx / s, py = dy / s;
    if (dz < 0.0f) { /* strict: -0.0 and NaN do not fold */
        const float fx = (1.0f - fabsf(py)) * order_sg(px);
        const float fy = (1.0f - fabsf(px)) * order_sg(py);
        px = fx;
        py = fy;
    }
    const uint32_t u = order_cell((px * 0.5f + 0.5f) * 64.0f), v = order_cell((py * 0.5f + 0.5f) * 64.0f);
    const uint32_t ocode = order_spread3(c[0]) | (order_spread3(c[1]) << 1) | (order_spread3(c[2]) << 2);
    const uint32_t dcode = order_spread2(u) | (order_spread2(v) << 1);
    keys[i] = direction_major != 0u ? (dcode << 18) | ocode : (ocode << 12) | dcode;
}

/* ---- the stable sort ---- */

#define RT_SORT_THREADS 256u
#define RT_SORT_WAVES (RT_SORT_THREADS / 64u)
#define RT_SORT_ITEMS 8u                                   /* entries per lane and step of a tile */
#define RT_SORT_STEP (RT_SORT_THREADS * RT_SORT_ITEMS)     /* entries a workgroup places between two barriers: 2048 */
#define RT_SORT_WAVE_SPAN (64u * RT_SORT_ITEMS)            /* ... of which a wave owns 512 consecutive ones */
#define RT_SORT_MAX_TILES 1024u                            /* so that the bucket table has a bounded size */
#define RT_SORT_BUCKETS 257u                               /* 256 digit values, then the entries that name no record */
#define RT_SORT_BUCKETS_PAD 260u
#define RT_SORT_SCAN_THREADS 1024u

/* entries per tile for a list of capacity n: whole steps, at most RT_SORT_MAX_TILES tiles */
static inline uint64_t sort_tile(uint64_t n) {
    uint64_t tile = (n + RT_SORT_MAX_TILES - 1u) / RT_SORT_MAX_TILES;
    tile = (tile + RT_SORT_STEP - 1u) / RT_SORT_STEP * RT_SORT_STEP;
    return tile < RT_SORT_STEP ? RT_SORT_STEP : tile;
}

/* the words of the bucket table reserved for capacity n: never fewer than the tiles sort_tile gives, and monotone in n */
static inline uint64_t sort_table_words(uint64_t n) {
    uint64_t tiles = (n + RT_SORT_STEP - 1u) / RT_SORT_STEP;
    if (tiles > RT_SORT_MAX_TILES) tiles = RT_SORT_MAX_TILES;
    return tiles * RT_SORT_BUCKETS;
}

__device__ __forceinline__ uint64_t sort_live_count(const uint32_t *__restrict__ count, uint64_t n) {
    if (count == nullptr) return n;
    const uint64_t c = *count;
    return c < n ? c : n;
}

__device__ __forceinline__ uint32_t sort_lanes_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

/* the bucket of an entry in the pass that looks at bits [shift, shift + 8) of its key field */
__device__ __forceinline__ uint32_t sort_bucket(uint32_t field, uint32_t index, uint64_t n, uint32_t shift) {
    return index < n ? (field >> shift) & 0xffu : 256u;
}

/* FIRST: entry j is the caller's (index_in[j] or j, the key read through it and cut to its field), written to the workspace as a pair;
 * otherwise it is the pair the pass before left there */
template <bool FIRST>
__global__ __launch_bounds__(RT_SORT_THREADS) void sort_count_kernel(const uint32_t *__restrict__ keys_in, const uint32_t *index_in, const uint64_t n,
                                                                     const uint32_t *__restrict__ count, const uint64_t tile, const uint32_t tiles,
                                                                     const uint32_t first_bit, const uint32_t field_mask, const uint32_t shift,
                                                                     uint32_t *__restrict__ pair_keys, uint32_t *__restrict__ pair_index,
                                                                     uint32_t *__restrict__ table) {
    __shared__ uint32_t hist[RT_SORT_BUCKETS_PAD];
    const uint64_t m = sort_live_count(count, n);
    const uint64_t start = (uint64_t)blockIdx.x * tile;
    if (start >= m) return; /* the scan reads a tile beyond the count as empty */
    const uint64_t end = start + tile < m ? start + tile : m;
    for (uint32_t b = threadIdx.x; b < RT_SORT_BUCKETS; b += RT_SORT_THREADS) hist[b] = 0u;
    __syncthreads();
    for (uint64_t j = start + threadIdx.x; j < end; j += RT_SORT_THREADS) {
        uint32_t field, index;
        if (FIRST) {
            index = index_in != nullptr ? index_in[j] : (uint32_t)j;
            field = index < n ? (keys_in[index] >> first_bit) & field_mask : 0u; /* an entry >= n reads no key */
            pair_keys[j] = field;
            pair_index[j] = index;
        } else {
            field = keys_in[j];
            index = index_in[j];
        }
        atomicAdd(&hist[sort_bucket(field, index, n, shift)], 1u); /* counting only */
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < RT_SORT_BUCKETS; b += RT_SORT_THREADS) table[(uint64_t)b * tiles + blockIdx.x] = hist[b];
}

/* table[b * tiles + t] becomes the number of entries in buckets below b, plus those of bucket b in tiles below t */
__global__ __launch_bounds__(RT_SORT_SCAN_THREADS) void sort_scan_kernel(uint32_t *__restrict__ table, const uint64_t n, const uint32_t *__restrict__ count,
                                                                         const uint64_t tile, const uint32_t tiles) {
    __shared__ uint32_t wave_sum[RT_SORT_SCAN_THREADS / 64u];
    const uint64_t m = sort_live_count(count, n);
    const uint32_t live = (uint32_t)((m + tile - 1u) / tile); /* tiles that counted */
    const uint32_t entries = RT_SORT_BUCKETS * tiles;
    const uint32_t chunk = (entries + RT_SORT_SCAN_THREADS - 1u) / RT_SORT_SCAN_THREADS;
    const uint32_t lo = threadIdx.x * chunk < entries ? threadIdx.x * chunk : entries;
    const uint32_t hi = lo + chunk < entries ? lo + chunk : entries;
    uint32_t sum = 0u;
    for (uint32_t e = lo; e < hi; ++e) sum += (e % tiles) < live ? table[e] : 0u;
    /* exclusive sum of one value per thread over the workgroup */
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = sum;
    for (uint32_t off = 1u; off < 64u; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    if (lane == 63u) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t before = 0u;
    for (uint32_t w = 0; w < wave; ++w) before += wave_sum[w];
    uint32_t run = before + incl - sum;
    for (uint32_t e = lo; e < hi; ++e) {
        const uint32_t c = (e % tiles) < live ? table[e] : 0u;
        table[e] = run;
        run += c;
    }
}

/* index_out alone on the last pass (keys_out null) */
__global__ __launch_bounds__(RT_SORT_THREADS) void sort_scatter_kernel(const uint32_t *__restrict__ keys_in, const uint32_t *__restrict__ index_in,
                                                                       const uint64_t n, const uint32_t *__restrict__ count, const uint64_t tile,
                                                                       const uint32_t tiles, const uint32_t shift, const uint32_t *__restrict__ table,
                                                                       uint32_t *__restrict__ keys_out, uint32_t *__restrict__ index_out) {
    __shared__ uint32_t base[RT_SORT_BUCKETS_PAD];                   /* where the tile's next entry of a bucket goes */
    __shared__ uint32_t wave_at[RT_SORT_WAVES][RT_SORT_BUCKETS_PAD]; /* a wave's counts per step, then its running positions */
    const uint64_t m = sort_live_count(count, n);
    const uint64_t start = (uint64_t)blockIdx.x * tile;
    if (start >= m) return;
    const uint64_t end = start + tile < m ? start + tile : m;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t b = threadIdx.x; b < RT_SORT_BUCKETS; b += RT_SORT_THREADS) base[b] = table[(uint64_t)b * tiles + blockIdx.x];
    volatile uint32_t *const mine = wave_at[wave]; /* read and written by this wave alone between the barriers, in program order */
    for (uint64_t s = start; s < end; s += RT_SORT_STEP) { /* workgroup-uniform */
        for (uint32_t b = threadIdx.x; b < RT_SORT_WAVES * RT_SORT_BUCKETS_PAD; b += RT_SORT_THREADS) (&wave_at[0][0])[b] = 0u;
        __syncthreads();
        uint32_t field[RT_SORT_ITEMS], index[RT_SORT_ITEMS], bucket[RT_SORT_ITEMS];
#pragma unroll
        for (uint32_t k = 0; k < RT_SORT_ITEMS; ++k) {
            const uint64_t j = s + wave * RT_SORT_WAVE_SPAN + k * 64u + lane;
            field[k] = 0u;
            index[k] = 0u;
            bucket[k] = 0xffffffffu; /* no entry */
            if (j < end) {
                field[k] = keys_in[j];
                index[k] = index_in[j];
                bucket[k] = sort_bucket(field[k], index[k], n, shift);
                atomicAdd(&wave_at[wave][bucket[k]], 1u); /* counting only */
            }
        }
        __syncthreads();
        for (uint32_t b = threadIdx.x; b < RT_SORT_BUCKETS; b += RT_SORT_THREADS) {
            uint32_t at = base[b];
#pragma unroll
            for (uint32_t w = 0; w < RT_SORT_WAVES; ++w) {
                const uint32_t c = wave_at[w][b];
                wave_at[w][b] = at;
                at += c;
            }
            base[b] = at;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < RT_SORT_ITEMS; ++k) { /* wave-uniform: every lane takes part in the ballots */
            const bool has = bucket[k] != 0xffffffffu;
            unsigned long long peers = __ballot(has);
#pragma unroll
            for (uint32_t bit = 0; bit < 9u; ++bit) {
                const unsigned long long set = __ballot(has && ((bucket[k] >> bit) & 1u) != 0u);
                peers &= ((bucket[k] >> bit) & 1u) != 0u ? set : ~set;
            }
            if (has) {
                const uint32_t rank = sort_lanes_below(peers);
                const uint32_t at = mine[bucket[k]];
                const uint64_t to = (uint64_t)at + rank;
                if (to < m) { /* always, when the pairs are what was counted */
                    if (keys_out != nullptr) keys_out[to] = field[k];
                    index_out[to] = index[k];
                }
                if (rank == 0u) mine[bucket[k]] = at + (uint32_t)__popcll(peers); /* after every peer's read: one wave, program order */
            }
        }
        __syncthreads();
    }
}

/* ---- gather and scatter ---- */

__global__ __launch_bounds__(RT_ORDER_THREADS) void gather_records_kernel(const uint32_t *__restrict__ src, const uint32_t words, const uint64_t n,
                                                                          const uint32_t *__restrict__ index, const uint32_t *__restrict__ count,
                                                                          const uint64_t max_count, uint32_t *__restrict__ dst) {
    const uint64_t g = (uint64_t)blockIdx.x * RT_ORDER_THREADS + threadIdx.x; /* the dword of dst */
    const uint64_t j = g / words;
    if (j >= sort_live_count(count, max_count)) return;
    const uint32_t k = (uint32_t)(g - j * words);
    const uint64_t from = index[j];
    dst[g] = from < n ? src[from * words + k] : 0u;
}

__global__ __launch_bounds__(RT_ORDER_THREADS) void scatter_records_kernel(const uint32_t *__restrict__ src, const uint32_t words, const uint64_t n,
                                                                           const uint32_t *__restrict__ index, const uint32_t *__restrict__ count,
                                                                           const uint64_t max_count, uint32_t *__restrict__ dst) {
    const uint64_t g = (uint64_t)blockIdx.x * RT_ORDER_THREADS + threadIdx.x; /* the dword of src */
    const uint64_t j = g / words;
    if (j >= sort_live_count(count, max_count)) return;
    const uint32_t k = (uint32_t)(g - j * words);
    const uint64_t to = index[j];
    if (to < n) dst[to * words + k] = src[g];
}

} /* namespace rt */

/* ---- the C entry points (include/rt_amd.h "record ordering") ---- */

/* the workspace of rt_sort_records for capacity n: two (key field, index) pair buffers and the bucket table */
static inline uint64_t sort_temp_bytes(uint64_t n) { return (4u * n + rt::sort_table_words(n)) * sizeof(uint32_t); }

extern "C" {

int rt_ray_keys(const rt_ray *d_rays, size_t n, const float box_lo[3], const float box_hi[3], uint32_t flags, uint32_t *d_keys, void *hip_stream) {
    bool done;
    const int rc = query_args("rt_ray_keys", n, {32u, "rays", "key them in several calls"}, false, nullptr, d_rays && box_lo && box_hi && d_keys,
                              "ray, box or key", &done);
    if (rc != RT_OK || done) return rc;
    if ((flags & ~(uint32_t)RT_ORDER_DIRECTION_MAJOR) != 0u) return fail(RT_ERR_INVALID_ARGUMENT, "rt_ray_keys: unknown flag bit (RT_ORDER_DIRECTION_MAJOR is the only one)");
    rt::OrderBox box;
    for (int a = 0; a < 3; ++a) {
        box.lo[a] = box_lo[a];
        box.scale[a] = box_hi[a] > box_lo[a] ? 64.0f / (box_hi[a] - box_lo[a]) : 0.0f; /* a NaN bound compares false: 0 */
    }
    hipLaunchKernelGGL(rt::ray_keys_kernel, grid_of(n, RT_ORDER_THREADS), dim3(RT_ORDER_THREADS), 0, static_cast<hipStream_t>(hip_stream), d_rays, (uint64_t)n, box,
                       flags & (uint32_t)RT_ORDER_DIRECTION_MAJOR, d_keys);
    return launched("rt_ray_keys");
}

size_t rt_sort_temp_bytes(size_t n) {
    if (n == 0 || (uint64_t)n >= (1ull << 32)) return 0;
    return (size_t)sort_temp_bytes((uint64_t)n);
}

int rt_sort_records(const uint32_t *d_keys, size_t n, uint32_t first_bit, uint32_t key_bits, const uint32_t *d_index_in, const uint32_t *d_count_in,
                    uint32_t *d_index_out, void *d_temp, size_t temp_bytes, void *hip_stream) {
    bool done;
    const int rc = query_args("rt_sort_records", n, {32u, "records", "sort them in several calls"}, false, nullptr, d_keys && d_index_out && d_temp,
                              "key, output or workspace", &done);
    if (rc != RT_OK || done) return rc;
    if (key_bits == 0u || (uint64_t)first_bit + key_bits > 32u)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_sort_records: need key_bits >= 1 and first_bit + key_bits <= 32");
    if ((uint64_t)temp_bytes < sort_temp_bytes((uint64_t)n))
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_sort_records: the workspace is smaller than rt_sort_temp_bytes(n)");
    if (d_count_in && !d_index_in) return fail(RT_ERR_INVALID_ARGUMENT, "rt_sort_records: a count without an index list (the identity list has n entries)");
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const uint64_t tile = rt::sort_tile((uint64_t)n);
    const uint32_t tiles = (uint32_t)(((uint64_t)n + tile - 1u) / tile);
    uint32_t *const words = static_cast<uint32_t *>(d_temp);
    uint32_t *const pair_keys[2] = {words, words + 2u * (uint64_t)n};
    uint32_t *const pair_index[2] = {words + (uint64_t)n, words + 3u * (uint64_t)n};
    uint32_t *const table = words + 4u * (uint64_t)n;
    const uint32_t field_mask = key_bits == 32u ? 0xffffffffu : (1u << key_bits) - 1u;
    const uint32_t passes = (key_bits + 7u) / 8u;
    for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t cur = p & 1u, shift = 8u * p;
        const bool last = p + 1u == passes;
        if (p == 0u)
            hipLaunchKernelGGL(rt::sort_count_kernel<true>, dim3(tiles), dim3(RT_SORT_THREADS), 0, stream, d_keys, d_index_in, (uint64_t)n, d_count_in, tile,
                               tiles, first_bit, field_mask, shift, pair_keys[0], pair_index[0], table);
        else
            hipLaunchKernelGGL(rt::sort_count_kernel<false>, dim3(tiles), dim3(RT_SORT_THREADS), 0, stream, (const uint32_t *)pair_keys[cur],
                               (const uint32_t *)pair_index[cur], (uint64_t)n, d_count_in, tile, tiles, first_bit, field_mask, shift, (uint32_t *)nullptr,
                               (uint32_t *)nullptr, table);
        hipLaunchKernelGGL(rt::sort_scan_kernel, dim3(1), dim3(RT_SORT_SCAN_THREADS), 0, stream, table, (uint64_t)n, d_count_in, tile, tiles);
        hipLaunchKernelGGL(rt::sort_scatter_kernel, dim3(tiles), dim3(RT_SORT_THREADS), 0, stream, (const uint32_t *)pair_keys[cur],
                           (const uint32_t *)pair_index[cur], (uint64_t)n, d_count_in, tile, tiles, shift, (const uint32_t *)table,
                           last ? (uint32_t *)nullptr : pair_keys[cur ^ 1u], last ? d_index_out : pair_index[cur ^ 1u]);
    }
    return launched("rt_sort_records");
}

/* the checks the two record movers share, in the documented order; *done: nothing to launch */
static int move_records_args(const char *who, const void *d_src, size_t record_bytes, size_t n, const uint32_t *d_index, size_t max_count,
                             const void *d_dst, bool *done) {
    *done = true;
    int rc = check_count(who, std::max<uint64_t>(n, max_count), {32u, "records or index entries", "move them in several calls"});
    if (rc != RT_OK || n == 0 || max_count == 0) return rc;
    rc = check_pointers(who, d_src && d_index && d_dst, "source, index or destination");
    if (rc != RT_OK) return rc;
    if (record_bytes < 4 || record_bytes > 256 || (record_bytes & 3u) != 0)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": record_bytes must be a multiple of 4 from 4 to 256");
    *done = false;
    return RT_OK;
}

int rt_gather_records(const void *d_src, size_t record_bytes, size_t n, const uint32_t *d_index, const uint32_t *d_count, size_t max_count, void *d_dst,
                      void *hip_stream) {
    bool done;
    const int rc = move_records_args("rt_gather_records", d_src, record_bytes, n, d_index, max_count, d_dst, &done);
    if (rc != RT_OK || done) return rc;
    const uint32_t words = (uint32_t)(record_bytes / 4);
    hipLaunchKernelGGL(rt::gather_records_kernel, grid_of((uint64_t)max_count * words, RT_ORDER_THREADS) /* below 2^30 */, dim3(RT_ORDER_THREADS), 0, static_cast<hipStream_t>(hip_stream),
                       static_cast<const uint32_t *>(d_src), words, (uint64_t)n, d_index, d_count, (uint64_t)max_count, static_cast<uint32_t *>(d_dst));
    return launched("rt_gather_records");
}

int rt_scatter_records(const void *d_src, size_t record_bytes, size_t n, const uint32_t *d_index, const uint32_t *d_count, size_t max_count, void *d_dst,
                       void *hip_stream) {
    bool done;
    const int rc = move_records_args("rt_scatter_records", d_src, record_bytes, n, d_index, max_count, d_dst, &done);
    if (rc != RT_OK || done) return rc;
    const uint32_t words = (uint32_t)(record_bytes / 4);
    hipLaunchKernelGGL(rt::scatter_records_kernel, grid_of((uint64_t)max_count * words, RT_ORDER_THREADS), dim3(RT_ORDER_THREADS), 0, static_cast<hipStream_t>(hip_stream),
                       static_cast<const uint32_t *>(d_src), words, (uint64_t)n, d_index, d_count, (uint64_t)max_count, static_cast<uint32_t *>(d_dst));
    return launched("rt_scatter_records");
}

} /* extern "C" */
