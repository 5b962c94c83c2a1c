// view_aov_main -- csrc/nrc_view_aov.hpp and nrc_math.h's nrc_expm1_negf on the CPU, device-free, built with ASan + UBSan and run directly
// (tests/test_view_aov_cpu.py).
//   view_aov_main aov <scene file> <out file>
//     scene file: uint32 {nx, ny, nz, w, h, x_offset, x_stride, x_block_log2}, float {size[3], density_factor, inv_gw, inv_gh,
//     inv_proj_view[16], pos[3]}, nx * ny * nz density bytes.  out file: [h][w][4] floats of the plain voxel walk.  Every pixel is walked
//     a second time with the occupancy jumps (the bits of nrc_occupancy.hpp, as the kernel finds them in LDS): a pixel whose two results
//     differ in any bit is reported and the program fails.
//   view_aov_main expm1 <out file>
//     pairs {x, nrc_expm1_negf(x)}: every 128th float of [2^-60, 32) -- 65 * 2^16 > 2^22 arguments -- and the 129 floats around every branch
//     point of the function (0, (n + 1/2) ln 2 for n = 0 .. 25, NRC_EXPM1_ONE).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "nrc_hot_tiles.hpp"
#include "nrc_occupancy.hpp"
#include "nrc_view_aov.hpp"

static bool read_all(const char* path, std::vector<unsigned char>* out)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out->resize((size_t)n);
    const bool ok = n == 0 || std::fread(out->data(), 1, (size_t)n, f) == (size_t)n;
    std::fclose(f);
    return ok;
}
static bool write_all(const char* path, const void* p, size_t bytes)
{
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = std::fwrite(p, 1, bytes, f) == bytes;
    return std::fclose(f) == 0 && ok;
}

static int run_aov(const char* in_path, const char* out_path)
{
    std::vector<unsigned char> file;
    if (!read_all(in_path, &file)) { std::printf("FAILED: cannot read %s\n", in_path); return 1; }
    uint32_t u[8];
    float f[25];
    const size_t head = sizeof(u) + sizeof(f);
    if (file.size() < head) { std::printf("FAILED: short scene file\n"); return 1; }
    std::memcpy(u, file.data(), sizeof(u));
    std::memcpy(f, file.data() + sizeof(u), sizeof(f));
    const uint32_t nx = u[0], ny = u[1], nz = u[2], w = u[3], h = u[4];
    if (file.size() != head + (size_t)nx * ny * nz) { std::printf("FAILED: scene file size\n"); return 1; }
    const uint8_t* vol = file.data() + head;
    const nrc::OccupancyBits occ = nrc::build_occupancy_bits(vol, nx, ny, nz, 2048);
    const nrc::AovGrid g{nx, ny, nz, {f[0], f[1], f[2]}, f[3], occ.shift, occ.gx, occ.gy};
    const nrc::AovVolumeBytes density{vol, nx, ny};
    const nrc::AovOccupancyBits occupied{occ.bits.data()};
    std::vector<float> out((size_t)w * h * 4);
    size_t differ = 0;
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t lx = 0; lx < w; lx++) {
            const uint32_t gx = nrc::global_x(u[5], u[6], u[7], lx);
            const nrc::AovRay ray = nrc::view_aov_camera_ray(f + 6, f + 22, (float)gx * f[4], (float)y * f[5]);
            const nrc::ViewAov a = nrc::view_aov_walk(g, ray, density, nrc::NoOccupancy{});
            const nrc::ViewAov b = nrc::view_aov_walk(g, ray, density, occupied);
            if (std::memcmp(&a, &b, sizeof(a)) != 0) {
                if (differ++ < 8)
                    std::printf("FAILED: pixel (%u, %u): plain {%a, %a, %a, %a}, with jumps {%a, %a, %a, %a}\n", lx, y, a.alpha, a.tau, a.z_front,
                                a.z_half, b.alpha, b.tau, b.z_front, b.z_half);
            }
            std::memcpy(&out[((size_t)y * w + lx) * 4], &a, sizeof(a));
        }
    if (!write_all(out_path, out.data(), out.size() * 4)) { std::printf("FAILED: cannot write %s\n", out_path); return 1; }
    std::printf("view_aov: %u x %u pixels, %zu differ between the plain walk and the walk with jumps\n", w, h, differ);
    return differ == 0 ? 0 : 1;
}

static int run_expm1(const char* out_path)
{
    std::vector<float> out;
    auto add = [&](float x) { out.push_back(x); out.push_back(nrc_expm1_negf(x)); };
    const uint32_t lo = nrc_f2u(0x1p-60f), hi = nrc_f2u(32.0f);
    for (uint32_t b = lo; b < hi; b += 128u) add(nrc_u2f(b));
    std::vector<float> points = {0.0f, NRC_EXPM1_ONE};
    for (int n = 0; n <= 25; n++) points.push_back((float)(((double)n + 0.5) * 0.6931471805599453));
    for (float p : points) {
        const uint32_t c = nrc_f2u(p);
        for (uint32_t b = c > 64u ? c - 64u : 0u; b <= c + 64u; b++) add(nrc_u2f(b));
    }
    for (float x : {-0.0f, -1.0f, 1e30f, __builtin_huge_valf(), __builtin_nanf("")}) add(x);
    if (!write_all(out_path, out.data(), out.size() * 4)) { std::printf("FAILED: cannot write %s\n", out_path); return 1; }
    std::printf("expm1: %zu arguments\n", out.size() / 2);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && std::string(argv[1]) == "aov") return run_aov(argv[2], argv[3]);
    if (argc == 3 && std::string(argv[1]) == "expm1") return run_expm1(argv[2]);
    std::printf("FAILED: usage: view_aov_main aov <scene> <out> | view_aov_main expm1 <out>\n");
    return 2;
}
