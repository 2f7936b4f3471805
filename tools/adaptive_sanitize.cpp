/*
 * adaptive_sanitize.cpp — the five CPU forms of the adaptive sampling queries (include/rt_host.h) on their edge inputs, and
 * rt_film_splat_host, which shares the listed splat's walk, as a stand-alone program for AddressSanitizer and UndefinedBehaviorSanitizer.  Every array is a heap allocation of exactly the size the interface
 * states, so a read or write one element outside it is reported.  Build and run, from the repository root (no device, no Python):
 *
 *   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -fno-fast-math \
 *       -o /tmp/adaptive_sanitize tools/adaptive_sanitize.cpp homework-18-graphics-raytracer_amd/csrc/host/rt_host.cpp -lz \
 *     && /tmp/adaptive_sanitize
 *
 * It prints "adaptive_sanitize: ok" and returns 0 when every call returned what it should and the sanitizers saw nothing.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/rt_host.h"

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

/* exact-size heap arrays: std::vector<T>(n).data() of n elements; n == 0 gives a pointer nobody may touch */
template <class T> static T *exact(std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }

static void budget_edges() {
    const float nan = nanf(""), inf = INFINITY;
    /* planes inside 8-word records, exactly (n - 1) * 8 + 1 words long: the last record is read at its first word only */
    const size_t n = 9;
    std::vector<float> mean((n - 1) * 8 + 1, 1.0f), variance = {0.0f, -1.0f, nan, inf, 1.0f, 4.0f, 1e30f, 0.25f, 1.0f};
    std::vector<uint32_t> count((n - 1) * 8 + 1, 1u), valid(n, 1u), out(n, 99u);
    count[4 * 8] = 0u;
    valid[8] = 0u;
    const rt_sample_budget_params p = {4.0f, 1.0f, 2u, 10u, 0u};
    EXPECT(rt_sample_budget_cpu(mean.data(), 8, variance.data(), 1, count.data(), 8, valid.data(), 1, &p, n, out.data()) == RT_OK);
    const uint32_t want[9] = {2u, 10u, 10u, 10u, 10u, 6u, 10u, 3u, 0u};
    for (size_t i = 0; i < n; ++i) EXPECT(out[i] == want[i]);
    const rt_sample_budget_params same = {0.0f, 1.0f, 7u, 7u, 0u};
    EXPECT(rt_sample_budget_cpu(mean.data(), 8, variance.data(), 1, nullptr, 0, nullptr, 0, &same, n, out.data()) == RT_OK);
    EXPECT(out[0] == 7u && out[3] == 7u);
    EXPECT(rt_sample_budget_cpu(nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr) == RT_OK);
}

static void list_edges() {
    const std::vector<uint32_t> counts = {0u, 3u, 0xffffffffu, 0u, 64u, 1u, 0u};
    const size_t n = counts.size(), asked = 3 + 64 + 64 + 1;
    const size_t capacities[] = {asked, asked - 1, 40, 0, asked + 10};
    for (size_t capacity : capacities) {
        std::vector<uint32_t> first(n, 5u), start(n + 1, 99u), pixel(capacity, 99u), sample(capacity, 99u), total(2, 99u);
        EXPECT(rt_sample_list_cpu(counts.data(), n, capacity, first.data(), start.data(), exact(pixel), exact(sample), total.data()) == RT_OK);
        const size_t listed = asked < capacity ? asked : capacity;
        EXPECT(total[0] == listed && total[1] == asked && start[n] == listed && start[0] == 0u);
        for (size_t j = 0; j < listed; ++j) EXPECT(pixel[j] < n && start[pixel[j]] <= j && j < start[pixel[j] + 1] && sample[j] == 5u + (j - start[pixel[j]]));
        /* a second call continues where the first stopped */
        std::vector<uint32_t> again(n, 1u), pixel2(n, 0u), sample2(n, 0u);
        EXPECT(rt_sample_list_cpu(again.data(), n, n, first.data(), start.data(), pixel2.data(), sample2.data(), total.data()) == RT_OK);
        for (size_t i = 0; i < n; ++i) EXPECT(sample2[i] + 1u == first[i]);
    }
    std::vector<uint32_t> start(1, 9u), total(2, 9u);
    EXPECT(rt_sample_list_cpu(nullptr, 0, 7, nullptr, start.data(), nullptr, nullptr, total.data()) == RT_OK && start[0] == 0u && total[0] == 0u && total[1] == 0u);
    EXPECT(rt_sample_list_cpu(nullptr, (size_t)1 << 26, 7, nullptr, start.data(), nullptr, nullptr, total.data()) == RT_ERR_UNSUPPORTED);
}

static void listed_edges() {
    const rt_frame frame = {6u, 5u, 3, 1u, 1u, 5u, 5u, 2u}; /* a tile of 4 x 2 pixels with a row step */
    rt_camera camera;
    rt_reference_camera(&camera);
    const size_t n = 8, capacity = 20;
    std::vector<uint32_t> counts(n, 2u), start(n + 1), pixel(capacity), sample(capacity), total(2);
    EXPECT(rt_sample_list_cpu(counts.data(), n, capacity, nullptr, start.data(), pixel.data(), sample.data(), total.data()) == RT_OK && total[0] == 16u);
    pixel[2] = 8u;          /* a pixel the tile does not have */
    pixel[3] = 0xffffffffu; /* ... and one nobody has */
    std::vector<float> offsets(2 * capacity, 7.0f);
    std::vector<rt_ray> rays(capacity);
    memset(rays.data(), 0xff, capacity * sizeof(rt_ray));
    for (uint32_t pattern = 0; pattern < 2; ++pattern) {
        EXPECT(rt_film_offsets_listed_cpu(&frame, pattern, 3u, pixel.data(), sample.data(), total.data(), capacity, offsets.data()) == RT_OK);
        EXPECT(rt_camera_rays_listed_cpu(&camera, &frame, offsets.data(), pixel.data(), total.data(), capacity, rays.data()) == RT_OK);
        for (size_t j = 0; j < capacity; ++j) {
            const bool absent = j >= 16 || j == 2 || j == 3;
            EXPECT(absent == (offsets[2 * j] != offsets[2 * j]));
            EXPECT(absent == (rays[j].direction[0] == 0.0f && rays[j].direction[1] == 0.0f && rays[j].direction[2] == 0.0f));
        }
    }
    /* a total beyond the capacity is read as the capacity */
    total[0] = 0xffffffffu;
    pixel[2] = pixel[3] = 0u;
    for (size_t j = 16; j < capacity; ++j) pixel[j] = 1u, sample[j] = 0u;
    EXPECT(rt_film_offsets_listed_cpu(&frame, RT_FILM_UNIFORM, 3u, pixel.data(), sample.data(), total.data(), capacity, offsets.data()) == RT_OK);
    EXPECT(offsets[2 * (capacity - 1)] == offsets[2 * (capacity - 1)]);
    EXPECT(rt_film_offsets_listed_cpu(&frame, RT_FILM_STRATIFIED, 3u, pixel.data(), sample.data(), total.data(), capacity, offsets.data()) == RT_ERR_INVALID_ARGUMENT);
    EXPECT(rt_film_offsets_listed_cpu(&frame, RT_FILM_UNIFORM, 3u, nullptr, nullptr, nullptr, 0, nullptr) == RT_OK);
}

static void splat_edges() {
    const uint32_t rows = 5, cols = 4, n = rows * cols;
    const size_t capacity = 23;
    std::vector<float> samples(3 * capacity, 1.0f), offsets(2 * capacity, 0.25f), sum(3 * n, 0.0f), weight(n, 0.0f);
    std::vector<uint8_t> valid(capacity, 1u);
    valid[4] = 0u;
    offsets[10] = nanf("");
    /* starts that are no prefix sum: decreasing, far beyond the capacity, the largest word */
    std::vector<uint32_t> start(n + 1);
    for (uint32_t i = 0; i <= n; ++i) start[i] = i;
    start[3] = 0xffffffffu, start[7] = 0u, start[11] = (uint32_t)capacity + 40u, start[n] = 1000u;
    const float radii[] = {0.5f, 1.0f, 4.0f};
    for (uint32_t filter = 0; filter < 3; ++filter)
        for (float radius : radii) {
            EXPECT(rt_film_splat_listed_cpu(rows, cols, samples.data(), valid.data(), offsets.data(), start.data(), capacity, 64u, filter, radius, sum.data(),
                                            weight.data()) == RT_OK);
            EXPECT(rt_film_splat_listed_cpu(rows, cols, samples.data(), nullptr, offsets.data(), start.data(), capacity, 1u, filter, radius, sum.data(),
                                            weight.data()) == RT_OK);
        }
    for (float w : weight) EXPECT(w == w);
    /* no records at all: the sample arrays may be missing */
    EXPECT(rt_film_splat_listed_cpu(rows, cols, nullptr, nullptr, nullptr, start.data(), 0, 64u, RT_FILM_TENT, 1.0f, sum.data(), weight.data()) == RT_OK);
    /* a 1 x 1 image whose one pixel has every record */
    std::vector<uint32_t> one = {0u, (uint32_t)capacity};
    std::vector<float> s1(3, 0.0f), w1(1, 0.0f);
    EXPECT(rt_film_splat_listed_cpu(1, 1, samples.data(), valid.data(), offsets.data(), one.data(), capacity, 64u, RT_FILM_BOX, 0.5f, s1.data(), w1.data()) == RT_OK);
    EXPECT(w1[0] == (float)(capacity - 2)); /* one cleared flag, one NaN offset */
    EXPECT(rt_film_splat_listed_cpu(rows, cols, samples.data(), nullptr, offsets.data(), start.data(), capacity, 65u, RT_FILM_BOX, 0.5f, sum.data(), weight.data()) ==
           RT_ERR_INVALID_ARGUMENT);
}

/* rt_film_splat_host walks the same loop with the uniform layout: record s * n + q */
static void uniform_splat_edges() {
    const uint32_t shapes[2][2] = {{1u, 1u}, {17u, 13u}}, spp = 3;
    for (const auto &shape : shapes) {
        const uint32_t rows = shape[0], cols = shape[1], n = rows * cols;
        std::vector<float> samples(3 * spp * n, 1.0f), offsets(2 * spp * n, -0.5f), sum(3 * n, 0.0f), weight(n, 0.0f);
        std::vector<uint8_t> valid(spp * n, 1u);
        valid[spp * n - 1] = 0u;
        offsets[0] = nanf("");
        for (uint32_t filter = 0; filter < 3; ++filter) {
            EXPECT(rt_film_splat_host(rows, cols, samples.data(), valid.data(), offsets.data(), spp, filter, 4.0f, sum.data(), weight.data()) == RT_OK);
            EXPECT(rt_film_splat_host(rows, cols, samples.data(), nullptr, offsets.data(), spp, filter, 0.5f, sum.data(), weight.data()) == RT_OK);
        }
        for (float w : weight) EXPECT(w == w);
        std::vector<float> s1(3 * n, 0.0f), w1(n, 0.0f);
        EXPECT(rt_film_splat_host(rows, cols, samples.data(), valid.data(), offsets.data(), spp, RT_FILM_BOX, 0.5f, s1.data(), w1.data()) == RT_OK);
        EXPECT(n == 1u ? w1[0] == (float)(spp - 2) : w1[0] == (float)(spp - 1) && w1[n - 1] == (float)(spp - 1)); /* a NaN offset, a cleared flag */
    }
    EXPECT(rt_film_splat_host(0, 5, nullptr, nullptr, nullptr, spp, RT_FILM_BOX, 0.5f, nullptr, nullptr) == RT_OK);
    EXPECT(rt_film_splat_host(1, 1, nullptr, nullptr, nullptr, spp, RT_FILM_BOX, 4.5f, nullptr, nullptr) == RT_ERR_INVALID_ARGUMENT);
}

int main() {
    budget_edges();
    list_edges();
    listed_edges();
    splat_edges();
    uniform_splat_edges();
    if (failures) {
        fprintf(stderr, "adaptive_sanitize: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("adaptive_sanitize: ok\n");
    return 0;
}
