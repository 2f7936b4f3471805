/*
 * adaptive_sanitize.cpp — the five CPU forms of the adaptive sampling queries (include/rt_host.h) on their edge inputs, rt_film_splat_host,
 * which shares the listed splat's walk, and the other CPU forms that go through the one element loop, as a stand-alone program for
 * AddressSanitizer and UndefinedBehaviorSanitizer.  Every array is a heap allocation of exactly the size the interface states, so a read or
 * write one element outside it is reported.  Build and run, from the repository root (no device, no Python):
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

/* The CPU forms that run an Op of a shared header through rt_host.cpp's one element loop, beside the budget and the listed offsets above:
 * the temporal, rectification and denoise queries on a 3 x 5 image, 15 = count() elements, every plane of exactly the stated size */
static void element_loops() {
    const uint32_t rows = 3, cols = 5, n = rows * cols;
    const rt_camera camera = {1.0f, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, -1.0f}, {0.0f, 1.0f, 0.0f}, 0.1f};
    const rt_frame frame = {cols, rows, 1, 0u, 0u, cols, rows, 1u};
    std::vector<float> position((n - 1) * 4 + 3, -2.0f), normal(3 * n, 0.0f), color(3 * n, 0.5f), motion(2 * n, 0.0f), variance(n, 9.0f), out(3 * n, 9.0f);
    std::vector<uint32_t> valid(n, 1u), object(n, 7u), clamped(n, 99u);
    for (uint32_t i = 0; i < n; ++i) normal[3 * i + 2] = 1.0f;
    valid[n - 1] = 0u;
    EXPECT(rt_temporal_motion_cpu(position.data(), 4, valid.data(), 1, &camera, &frame, motion.data()) == RT_OK);
    EXPECT(motion[0] == motion[0] && motion[2 * n - 1] != motion[2 * n - 1]); /* projected; a cleared pixel is NaN */
    for (uint32_t i = 0; i < n; ++i) motion[2 * i] = (float)(i % cols) + 0.5f, motion[2 * i + 1] = (float)(i / cols) + 0.5f;
    position.assign(3 * n, -2.0f);
    const rt_temporal_guides g = {normal.data(), position.data(), object.data(), valid.data(), 3u, 3u, 1u, 1u};
    const rt_temporal_params p = {0.9f, 0.1f, 0.05f, 8u, 0u};
    std::vector<rt_temporal_pixel> in(n, rt_temporal_pixel{{0.25f, 0.25f, 0.25f}, 0.25f, 0.0625f, 3u, {0u, 0u}}), hist(n), hist2(n);
    EXPECT(rt_temporal_accumulate_cpu(color.data(), motion.data(), &g, &g, &p, rows, cols, in.data(), hist.data(), variance.data()) == RT_OK);
    EXPECT(hist[0].length == 4u && hist[n - 1].length == 1u);
    std::vector<rt_temporal_box> box(n);
    const rt_bounds_params bp = {1.0f, 3u, 0u};
    EXPECT(rt_temporal_bounds_cpu(color.data(), 3, object.data(), 1, valid.data(), 1, &bp, rows, cols, box.data()) == RT_OK);
    EXPECT(rt_temporal_accumulate_bounded_cpu(color.data(), motion.data(), &g, &g, &p, rows, cols, in.data(), hist2.data(), nullptr, box.data(), 2u, clamped.data()) ==
           RT_OK);
    EXPECT(clamped[0] == 4u && hist2[0].length == 2u && clamped[n - 1] == 0u); /* 0.25 lies outside the box of a constant 0.5 */
    EXPECT(rt_temporal_feedback_cpu(out.data(), 3, valid.data(), 1, rows, cols, hist2.data()) == RT_OK);
    EXPECT(hist2[0].color[0] == 9.0f && hist2[0].length == 2u && hist2[n - 1].color[0] == 0.5f);
    const rt_denoise_guides dg = {normal.data(), position.data(), nullptr, valid.data(), 3u, 3u, 0u, 1u};
    const rt_denoise_params dp = {1.0f, 1.0f, 1.0f, 0u, 3u, 0u};
    std::vector<float> temp(3 * n, 0.0f);
    EXPECT(rt_denoise_atrous_cpu(color.data(), &dg, &dp, rows, cols, out.data(), temp.data()) == RT_OK);
    EXPECT(out[0] == 0.5f && out[3 * n - 1] == 0.5f);
    /* three levels: 16 + 4 bytes of scratch per pixel */
    const rt_svgf_atrous_params sp = {1.0f, 1.0f, 1.0f, 0u, 3u, 0u};
    std::vector<float> svgf_temp(5 * n, 0.0f), variance_out(n, 9.0f);
    variance.assign(n, 0.25f);
    EXPECT(rt_svgf_atrous_cpu(color.data(), 3, variance.data(), &dg, &sp, rows, cols, out.data(), variance_out.data(), svgf_temp.data()) == RT_OK);
    EXPECT(out[0] == 0.5f && variance_out[0] >= 0.0f && variance_out[0] <= 0.25f);
    /* one triangle that moved by (1, 0, 0) and one sphere that did not; a triangle hit, a sphere hit, a miss and an index out of range */
    rt_triangle tri = {};
    const float corners[3][3] = {{0.0f, 0.0f, 0.0f}, {1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}};
    for (int k = 0; k < 3; ++k) memcpy(tri.vertices[k].position, corners[k], sizeof corners[k]);
    const rt_sphere sphere = {0u, {0.0f, 0.0f, 5.0f}, 1.0f};
    rt_scene_desc now = {};
    now.triangles = &tri, now.n_triangles = 1u, now.spheres = &sphere, now.n_spheres = 1u;
    const std::vector<float> was_triangles = {1.0f, 0.0f, 0.0f, 2.0f, 0.0f, 0.0f, 1.0f, 1.0f, 0.0f}, was_spheres = {0.0f, 0.0f, 5.0f, 1.0f};
    std::vector<rt_hit> hits(4);
    memset(hits.data(), 0, hits.size() * sizeof(rt_hit));
    hits[0].kind = 1u, hits[0].position[0] = 0.25f, hits[0].position[1] = 0.25f;
    hits[1].kind = 0u, hits[1].position[2] = 4.0f;
    hits[2].kind = 0xffffffffu;
    hits[3].kind = 1u, hits[3].index = 1u;
    std::vector<float> was((hits.size() - 1) * 4 + 3, 9.0f);
    EXPECT(rt_previous_positions_cpu(&now, was_triangles.data(), was_spheres.data(), hits.data(), hits.size(), was.data(), 4) == RT_OK);
    EXPECT(was[0] == 1.25f && was[1] == 0.25f && was[3] == 9.0f && was[4 + 2] == 4.0f && was[8] != was[8] && was[12] != was[12]);
}

int main() {
    element_loops();
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
