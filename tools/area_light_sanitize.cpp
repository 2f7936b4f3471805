/*
 * area_light_sanitize.cpp — rt_area_light_samples_cpu (include/rt_host.h) on its edge inputs as a stand-alone program for
 * AddressSanitizer and UndefinedBehaviorSanitizer.  Every array is a heap allocation of exactly the size the interface states, so a
 * read or write one element outside it is reported.  Build and run, from the repository root (no device, no Python):
 *
 *   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -fno-fast-math \
 *       -o /tmp/area_light_sanitize tools/area_light_sanitize.cpp homework-18-graphics-raytracer_amd/csrc/host/rt_host.cpp -lz \
 *     && /tmp/area_light_sanitize
 *
 * It prints "area_light_sanitize: ok" and returns 0 when every call returned what it should and the sanitizers saw nothing.
 */
#include <math.h>
#include <stdio.h>
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

static rt_light light(uint32_t kind, uint32_t has_origin) {
    rt_light l;
    memset(&l, 0, sizeof l);
    l.kind = kind;
    l.has_origin = has_origin;
    l.origin[0] = 0.25f, l.origin[1] = 3.0f, l.origin[2] = -0.5f;
    l.direction[0] = 0.6f, l.direction[1] = -0.8f, l.direction[2] = 0.0f;
    l.angle = 0.9f, l.softness = 1.0f;
    l.color[0] = l.color[1] = l.color[2] = 1.0f;
    return l;
}

int main() {
    const std::vector<rt_light> lights = {light(RT_LIGHT_DIRECTIONAL, 0), light(RT_LIGHT_DIRECTIONAL, 1), light(RT_LIGHT_SPOT, 1), light(RT_LIGHT_POINT, 1)};
    const uint32_t patterns[2] = {RT_FILM_UNIFORM, RT_FILM_STRATIFIED};
    const uint32_t spps[4] = {1u, 4u, 16u, 64u};
    const size_t ns[3] = {1u, 63u, 257u};
    for (uint32_t pattern : patterns)
        for (uint32_t spp : spps)
            for (size_t n : ns)
                for (uint32_t first = 0; first < 4u; ++first)
                    for (uint32_t count = 1; first + count <= 4u; ++count) {
                        const std::vector<rt_light> range(lights.begin(), lights.begin() + first + count); /* ends with the last light read */
                        std::vector<float> radii(count);
                        for (uint32_t j = 0; j < count; ++j) radii[j] = j % 3u == 0u ? 0.5f : j % 3u == 1u ? 0.0f : NAN;
                        std::vector<uint32_t> ids(n);
                        for (size_t i = 0; i < n; ++i) ids[i] = 0xfffffff0u + (uint32_t)i * 7u; /* wraps */
                        std::vector<float> sample((size_t)spp * count * n * 3u, -1.0f);
                        EXPECT(rt_area_light_samples_cpu(range.data(), first, count, radii.data(), ids.data(), n, spp, pattern, 0xffffffffu, sample.data()) == RT_OK);
                        EXPECT(rt_area_light_samples_cpu(range.data(), first, count, radii.data(), nullptr, n, spp, pattern, 0u, sample.data()) == RT_OK);
                        for (float v : sample) EXPECT(isfinite(v));
                    }
    /* the refusals read and write nothing */
    float one = 0.5f, out[3];
    EXPECT(rt_area_light_samples_cpu(lights.data(), 0, 1, &one, nullptr, (size_t)1 << 32, 1, RT_FILM_UNIFORM, 0, out) == RT_ERR_UNSUPPORTED);
    EXPECT(rt_area_light_samples_cpu(nullptr, 0, 0, nullptr, nullptr, 5, 1, RT_FILM_UNIFORM, 0, nullptr) == RT_OK);
    EXPECT(rt_area_light_samples_cpu(nullptr, 0, 1, &one, nullptr, 1, 1, RT_FILM_UNIFORM, 0, out) == RT_ERR_INVALID_ARGUMENT);
    EXPECT(rt_area_light_samples_cpu(lights.data(), 0, 1, &one, nullptr, 1, 0, RT_FILM_UNIFORM, 0, out) == RT_ERR_INVALID_ARGUMENT);
    EXPECT(rt_area_light_samples_cpu(lights.data(), 0, 1, &one, nullptr, 1, 65, RT_FILM_UNIFORM, 0, out) == RT_ERR_INVALID_ARGUMENT);
    EXPECT(rt_area_light_samples_cpu(lights.data(), 0, 1, &one, nullptr, 1, 4, RT_FILM_CENTER, 0, out) == RT_ERR_INVALID_ARGUMENT);
    EXPECT(rt_area_light_samples_cpu(lights.data(), 0, 1, &one, nullptr, 1, 5, RT_FILM_STRATIFIED, 0, out) == RT_ERR_INVALID_ARGUMENT);
    if (failures == 0) printf("area_light_sanitize: ok\n");
    return failures == 0 ? 0 : 1;
}
