/*
 * upsample_sanitize.cpp — rt_upsample_guided_cpu (include/rt_host.h) on its edge inputs as a stand-alone program for AddressSanitizer
 * and UndefinedBehaviorSanitizer.  Every array is a heap allocation of exactly the size the interface states — a strided plane ends with
 * its last pixel's last word — so a read or write one element outside it is reported.  Build and run, from the repository root (no
 * device, no Python):
 *
 *   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -fno-fast-math \
 *       -o /tmp/upsample_sanitize tools/upsample_sanitize.cpp homework-18-graphics-raytracer_amd/csrc/host/rt_host.cpp -lz \
 *     && /tmp/upsample_sanitize
 *
 * It prints "upsample_sanitize: ok" and returns 0 when every call returned what it should and the sanitizers saw nothing.
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

/* a plane of n pixels, `width` words each, `stride` words apart, exactly as long as that: (n - 1) * stride + width words */
template <class T> static std::vector<T> plane(size_t n, uint32_t stride, uint32_t width, T fill) {
    return std::vector<T>(n ? (n - 1) * stride + width : 0, fill);
}

static uint32_t low(uint32_t full, uint32_t s) { return (full + s - 1u) / s; }

struct Planes {
    std::vector<float> normal, position, albedo;
    std::vector<uint32_t> valid, object;
    rt_denoise_guides g;
    /* strides as inside rt_hit (13 words) and rt_surface (18 words) records */
    Planes(size_t n) : normal(plane(n, 18, 3, 0.0f)), position(plane(n, 13, 3, 0.5f)), albedo(plane(n, 18, 3, 0.5f)), valid(plane(n, 18, 1, 1u)),
                       object(plane(n, 13, 1, 0u)) {
        for (size_t i = 0; i < n; ++i) normal[i * 18 + 2] = 1.0f, position[i * 13] = 0.01f * (float)i;
        g = {normal.data(), position.data(), albedo.data(), valid.data(), 18u, 13u, 18u, 18u};
    }
};

/* every size of the tests at every scale and radius: windows that stick out of the low image on all four sides, a last low row and
 * column that cover one output pixel only, 1 x 1 */
static void sizes() {
    const uint32_t shapes[][2] = {{1u, 1u}, {2u, 2u}, {7u, 5u}, {17u, 13u}, {31u, 18u}, {1u, 33u}, {33u, 1u}};
    for (const auto &shape : shapes)
        for (uint32_t s = 2; s <= 4; ++s)
            for (uint32_t radius = 1; radius <= 2; ++radius) {
                const uint32_t rows = shape[0], cols = shape[1];
                const size_t n = (size_t)rows * cols, n_lo = (size_t)low(rows, s) * low(cols, s);
                Planes lo(n_lo), hi(n);
                std::vector<float> color = plane(n_lo, 8, 3, 0.25f), out(3 * n, 9.0f); /* the colour inside 8-word history records */
                const rt_upsample_params p = {0.5f, 2.0f, s, radius, RT_DENOISE_DEMODULATE};
                EXPECT(rt_upsample_guided_cpu(color.data(), 8, &lo.g, lo.object.data(), 13, &hi.g, hi.object.data(), 13, &p, rows, cols, out.data()) == RT_OK);
                for (float v : out) EXPECT(fabsf(v - 0.25f) < 1e-6f); /* a constant under equal albedos returns itself, up to the two roundings */
                /* no planes at all */
                const rt_denoise_guides none = {nullptr, nullptr, nullptr, nullptr, 0u, 0u, 0u, 0u};
                const rt_upsample_params q = {INFINITY, INFINITY, s, radius, 0u};
                EXPECT(rt_upsample_guided_cpu(color.data(), 8, &none, nullptr, 0, &none, nullptr, 0, &q, rows, cols, out.data()) == RT_OK);
                for (float v : out) EXPECT(v == 0.25f);
            }
}

/* the edges of the tests: an invalid output pixel, an invalid and a non-finite source, an object nobody below has, everything invalid */
static void edges() {
    const uint32_t rows = 7, cols = 5, s = 2, cl = low(cols, s);
    const size_t n = (size_t)rows * cols, n_lo = (size_t)low(rows, s) * cl;
    for (uint32_t radius = 1; radius <= 2; ++radius) {
        Planes lo(n_lo), hi(n);
        std::vector<float> color(3 * n_lo, 1.0f), out(3 * n, 9.0f);
        const uint32_t payload = 0x7fc12345u;
        memcpy(&color[3 * (2 * cl + 1)], &payload, sizeof payload); /* low (2, 1): a NaN with a payload */
        color[3 * (0 * cl + 0) + 1] = INFINITY;
        lo.valid[(1 * cl + 2) * 18] = 0u;
        hi.valid[(4 * cols + 3) * 18] = 0u; /* nearest: low (2, 1) */
        hi.object[(6 * cols + 4) * 13] = 5u;
        const rt_upsample_params p = {0.5f, 2.0f, s, radius, RT_DENOISE_DEMODULATE};
        EXPECT(rt_upsample_guided_cpu(color.data(), 3, &lo.g, lo.object.data(), 13, &hi.g, hi.object.data(), 13, &p, rows, cols, out.data()) == RT_OK);
        uint32_t word;
        memcpy(&word, &out[3 * (4 * cols + 3)], sizeof word);
        EXPECT(word == payload);
        EXPECT(out[3 * (6 * cols + 4)] == 1.0f); /* no source of object 5: the nearest, raw */
        for (size_t i = 0; i < n; ++i)
            if (i != 4 * cols + 3) EXPECT(out[3 * i] - out[3 * i] == 0.0f); /* the NaN went nowhere else */
        /* at radius 1 pixel (0, 0) has no other source than the inf one and takes it raw; everybody else skips it */
        EXPECT((out[1] == INFINITY) == (radius == 1u) && fabsf(out[3 * (2 * cols + 2) + 1] - 1.0f) < 1e-6f);
        for (size_t i = 0; i < n_lo; ++i) lo.valid[i * 18] = 0u; /* nobody is a source: every pixel takes its nearest */
        EXPECT(rt_upsample_guided_cpu(color.data(), 3, &lo.g, nullptr, 0, &hi.g, nullptr, 0, &p, rows, cols, out.data()) == RT_OK);
        EXPECT(out[0] == 1.0f && out[1] == INFINITY);
    }
}

static void refusals() {
    Planes lo(4), hi(16);
    std::vector<float> color(12, 1.0f), out(48, 0.0f);
    rt_upsample_params p = {1.0f, 1.0f, 2u, 1u, 0u};
    EXPECT(rt_upsample_guided_cpu(nullptr, 3, &lo.g, nullptr, 0, &hi.g, nullptr, 0, &p, 0, 4, nullptr) == RT_OK);
    EXPECT(rt_upsample_guided_cpu(color.data(), 3, &lo.g, nullptr, 0, &hi.g, nullptr, 0, nullptr, 4, 4, out.data()) == RT_ERR_INVALID_ARGUMENT);
    EXPECT(rt_upsample_guided_cpu(color.data(), 3, nullptr, nullptr, 0, &hi.g, nullptr, 0, &p, 4, 4, out.data()) == RT_ERR_INVALID_ARGUMENT);
    EXPECT(rt_upsample_guided_cpu(color.data(), 3, &lo.g, nullptr, 0, &hi.g, nullptr, 0, &p, 1u << 16, 1u << 16, out.data()) == RT_ERR_INVALID_ARGUMENT);
    p.scale = 5u;
    EXPECT(rt_upsample_guided_cpu(color.data(), 3, &lo.g, nullptr, 0, &hi.g, nullptr, 0, &p, 4, 4, out.data()) == RT_ERR_INVALID_ARGUMENT);
    p.scale = 2u, p.radius = 3u;
    EXPECT(rt_upsample_guided_cpu(color.data(), 3, &lo.g, nullptr, 0, &hi.g, nullptr, 0, &p, 4, 4, out.data()) == RT_ERR_INVALID_ARGUMENT);
    p.radius = 1u;
    EXPECT(rt_upsample_guided_cpu(color.data(), 3, &lo.g, nullptr, 0, &hi.g, nullptr, 0, &p, 4, 4, color.data()) == RT_ERR_INVALID_ARGUMENT);
    EXPECT(strstr(rt_host_last_error(), "out must not be color") != nullptr);
    EXPECT(rt_upsample_guided_cpu(color.data(), 3, &lo.g, nullptr, 0, &hi.g, nullptr, 0, &p, 4, 4, out.data()) == RT_OK);
}

int main() {
    sizes();
    edges();
    refusals();
    if (failures) {
        fprintf(stderr, "upsample_sanitize: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("upsample_sanitize: ok\n");
    return 0;
}
