// Stand-alone driver of csrc/nrc_volume_keys.hpp (device-free), built with -fsanitize=address,undefined and run by
// tests/test_volume_keys_host.py: prints key_of_time's answer for fixed cases and a sweep of t -- one line "key <bits of t> <n_keys> <i> <W>",
// i = W = -1 for a rejected time -- which the test compares with scene.key_of_time, and checks the in-between voxel (scalar and the packed
// four-voxel form the kernel uses) over every (a, b, W) against plain 64-bit integer arithmetic.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "nrc_volume_keys.hpp"

static long g_checks = 0, g_failed = 0;
#define CHECK(c) do { g_checks++; if (!(c)) { g_failed++; std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static void emit(float t, uint32_t n_keys)
{
    uint32_t bits;
    std::memcpy(&bits, &t, 4);
    nrc::KeyTime kt;
    kt.i = 12345u; kt.w = 54321u;
    if (nrc::key_of_time(t, n_keys, &kt)) {
        CHECK(kt.i < n_keys && kt.w <= 256u);
        CHECK(kt.w == 0u || kt.i + 1u < n_keys);      // key i + 1 is read only where it exists
        std::printf("key %08" PRIx32 " %u %u %u\n", bits, n_keys, kt.i, kt.w);
    } else {
        CHECK(kt.i == 12345u && kt.w == 54321u);      // a rejected time writes nothing
        std::printf("key %08" PRIx32 " %u -1 -1\n", bits, n_keys);
    }
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (uint32_t n : {0u, 1u, 2u, 3u, 8u, 24u, 1000u}) {
        const float last = n ? (float)(n - 1) : 0.0f;
        const std::vector<float> cases = {0.0f, -0.0f, 0.5f, 129.0f / 256.0f, 127.0f / 512.0f, 255.0f / 512.0f, 511.0f / 512.0f, 1023.0f / 1024.0f,
            last, std::nextafter(last, -1.0f), std::nextafter(last, inf), last + 1.0f / 1048576.0f, last + 1.0f, 1.0f, 1.5f, 1.25f, 2.0f,
            std::nextafter(1.0f, 0.0f), std::nextafter(1.0f, 2.0f), -1e-30f, -1.0f, -inf, inf, nan, -nan, 1e-45f, 1e30f, 4294967296.0f, 3.4e38f};
        for (float t : cases) emit(t, n);
    }
    for (uint32_t n : {1u, 2u, 3u, 8u})      // a sweep across every key, finer than the weight's 1/256 steps, with a start off the grid
        for (int k = -300; k <= (int)(n - 1) * 1024 + 300; k++) {
            emit((float)k / 1024.0f, n);
            emit((float)k / 1024.0f + 1.0f / 3072.0f, n);
        }

    // the in-between voxel: ends, bounds and the packed form, every (a, b, W)
    for (uint32_t W = 0; W <= 256u; W++)
        for (uint32_t a = 0; a < 256u; a++)
            for (uint32_t b = 0; b < 256u; b++) {
                const uint32_t q = nrc::lerp_voxel(a, b, W);
                const uint64_t want = ((uint64_t)a * (256u - W) + (uint64_t)b * W + 128u) >> 8;
                const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
                // (b in byte 0, a in byte 1, ... : every byte position sees every pair)
                const uint32_t x = a | (b << 8) | ((255u - a) << 16) | (b << 24), y = b | (a << 8) | (b << 16) | ((255u - a) << 24);
                const uint32_t p = nrc::lerp_voxels4(x, y, W);
                const bool ok = q == want && q >= lo && q <= hi && (W != 0u || q == a) && (W != 256u || q == b) && (p & 255u) == q &&
                                ((p >> 8) & 255u) == nrc::lerp_voxel(b, a, W) && ((p >> 16) & 255u) == nrc::lerp_voxel(255u - a, b, W) &&
                                (p >> 24) == nrc::lerp_voxel(b, 255u - a, W);
                g_checks++;
                if (!ok) { g_failed++; std::printf("FAILED lerp a %u b %u W %u: %u (want %" PRIu64 "), packed %08" PRIx32 "\n", a, b, W, q, want, p); }
            }
    for (uint32_t W = 0; W <= 256u; W++) {      // a voxel of 1 fading to 0 is 1 up to W = 128, 0 from 129 (and the other way round)
        CHECK(nrc::lerp_voxel(1u, 0u, W) == (W <= 128u ? 1u : 0u));
        CHECK(nrc::lerp_voxel(0u, 1u, W) == (W >= 128u ? 1u : 0u));
    }
    std::printf("volume_keys: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
