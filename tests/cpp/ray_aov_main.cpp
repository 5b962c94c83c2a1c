// ray_aov_main -- csrc/nrc_view_aov.hpp's range walk (view_aov_walk_range) on the CPU, device-free, built with ASan + UBSan and run directly
// (tests/test_ray_aov_cpu.py).
//   ray_aov_main rays <scene file> <rays file> <out file>
//     scene file: uint32 {nx, ny, nz, n}, float {size[3], density_factor}, nx * ny * nz density bytes.  rays file: n records of 8 floats
//     {ox, oy, oz, t_min, dx, dy, dz, t_max}.  out file: [n][4] floats of the plain voxel walk.  Every ray is walked a second time with the
//     occupancy jumps (the bits of nrc_occupancy.hpp, as the kernel finds them in LDS), and every whole-range ray (t_min <= 0, t_max = +inf)
//     also by view_aov_walk, plain and with jumps: a ray whose results differ in any bit is reported and the program fails.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

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
static void report(const char* what, size_t i, const nrc::ViewAov& a, const nrc::ViewAov& b)
{
    std::printf("FAILED: ray %zu, %s: {%a, %a, %a, %a} against {%a, %a, %a, %a}\n", i, what, a.alpha, a.tau, a.z_front, a.z_half, b.alpha, b.tau,
                b.z_front, b.z_half);
}

static int run_rays(const char* scene_path, const char* rays_path, const char* out_path)
{
    std::vector<unsigned char> file, rays_file;
    if (!read_all(scene_path, &file)) { std::printf("FAILED: cannot read %s\n", scene_path); return 1; }
    if (!read_all(rays_path, &rays_file)) { std::printf("FAILED: cannot read %s\n", rays_path); return 1; }
    uint32_t u[4];
    float f[4];
    const size_t head = sizeof(u) + sizeof(f);
    if (file.size() < head) { std::printf("FAILED: short scene file\n"); return 1; }
    std::memcpy(u, file.data(), sizeof(u));
    std::memcpy(f, file.data() + sizeof(u), sizeof(f));
    const uint32_t nx = u[0], ny = u[1], nz = u[2];
    const size_t n = u[3];
    if (file.size() != head + (size_t)nx * ny * nz) { std::printf("FAILED: scene file size\n"); return 1; }
    if (rays_file.size() != n * 32) { std::printf("FAILED: rays file size\n"); return 1; }
    std::vector<float> rays(n * 8);
    if (n) std::memcpy(rays.data(), rays_file.data(), n * 32);
    const uint8_t* vol = file.data() + head;
    const nrc::OccupancyBits occ = nrc::build_occupancy_bits(vol, nx, ny, nz, 2048);
    const nrc::AovGrid g{nx, ny, nz, {f[0], f[1], f[2]}, f[3], occ.shift, occ.gx, occ.gy};
    const nrc::AovVolumeBytes density{vol, nx, ny};
    const nrc::AovOccupancyBits occupied{occ.bits.data()};
    std::vector<float> out(n * 4);
    size_t differ = 0, whole = 0, whole_differ = 0;
    for (size_t i = 0; i < n; i++) {
        const float* q = &rays[i * 8];
        const nrc::AovRay ray{{q[0], q[1], q[2]}, {q[4], q[5], q[6]}};
        const nrc::ViewAov a = nrc::view_aov_walk_range(g, ray, q[3], q[7], density, nrc::NoOccupancy{});
        const nrc::ViewAov b = nrc::view_aov_walk_range(g, ray, q[3], q[7], density, occupied);
        if (std::memcmp(&a, &b, sizeof(a)) != 0 && differ++ < 8) report("plain range walk against the one with jumps", i, a, b);
        const bool finite = std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(q[2]) && std::isfinite(q[4]) && std::isfinite(q[5]) &&
                            std::isfinite(q[6]);
        if (finite && q[3] <= 0.0f && q[7] == __builtin_huge_valf()) {      // (view_aov_walk makes no promise for a non-finite ray)
            whole++;
            const nrc::ViewAov c = nrc::view_aov_walk(g, ray, density, nrc::NoOccupancy{});
            const nrc::ViewAov d = nrc::view_aov_walk(g, ray, density, occupied);
            if ((std::memcmp(&a, &c, sizeof(a)) != 0 || std::memcmp(&a, &d, sizeof(a)) != 0) && whole_differ++ < 8)
                report("range walk against view_aov_walk", i, a, std::memcmp(&a, &c, sizeof(a)) != 0 ? c : d);
        }
        std::memcpy(&out[i * 4], &a, sizeof(a));
    }
    if (!write_all(out_path, out.data(), out.size() * 4)) { std::printf("FAILED: cannot write %s\n", out_path); return 1; }
    std::printf("ray_aov: %zu rays, %zu differ between the plain walk and the walk with jumps; %zu whole rays, %zu differ from view_aov_walk\n", n,
                differ, whole, whole_differ);
    return differ == 0 && whole_differ == 0 ? 0 : 1;
}

int main(int argc, char** argv)
{
    if (argc == 5 && std::string(argv[1]) == "rays") return run_rays(argv[2], argv[3], argv[4]);
    std::printf("FAILED: usage: ray_aov_main rays <scene> <rays> <out>\n");
    return 2;
}
