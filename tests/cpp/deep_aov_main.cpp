// deep_aov_main -- csrc/nrc_view_aov.hpp's deep range walk (deep_aov_walk_range) on the CPU, device-free, built with ASan + UBSan and run
// directly (tests/test_deep_aov_cpu.py).
//   deep_aov_main rays <scene file> <rays file> <levels file> <out file>
//     scene file: uint32 {nx, ny, nz, n}, float {size[3], density_factor}, nx * ny * nz density bytes.  rays file: n records of 8 floats
//     {ox, oy, oz, t_min, dx, dy, dz, t_max}.  levels file: K floats.  out file: [K][n] floats, the planes, then [n][4] floats, the flat
//     results, of the plain voxel walk.  Every plane is filled with NaN first, and the sink counts its calls: a level that is not emitted
//     exactly once is reported.  Every ray is walked a second time with the occupancy jumps (the bits of nrc_occupancy.hpp, as the kernel
//     finds them in LDS) and a third time by the flat range walk: a ray whose planes or flat results differ in any bit is reported and the
//     program fails.
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
static bool write_all(FILE* f, const void* p, size_t bytes) { return bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes; }

// the host sink of the header, with a count per level
struct CountingSink {
    float* z;
    size_t stride;
    uint32_t* calls;
    void emit(uint32_t k, float v)
    {
        z[(size_t)k * stride] = v;
        calls[k]++;
    }
};

static int run_rays(const char* scene_path, const char* rays_path, const char* levels_path, const char* out_path)
{
    std::vector<unsigned char> file, rays_file, levels_file;
    if (!read_all(scene_path, &file)) { std::printf("FAILED: cannot read %s\n", scene_path); return 1; }
    if (!read_all(rays_path, &rays_file)) { std::printf("FAILED: cannot read %s\n", rays_path); return 1; }
    if (!read_all(levels_path, &levels_file)) { std::printf("FAILED: cannot read %s\n", levels_path); return 1; }
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
    const uint32_t K = (uint32_t)(levels_file.size() / 4);
    std::vector<float> levels(K);
    if (K) std::memcpy(levels.data(), levels_file.data(), (size_t)K * 4);
    const char* bad = nrc::deep_aov_levels_error(K, levels.data());
    if (bad || levels_file.size() != (size_t)K * 4) { std::printf("FAILED: levels: %s\n", bad ? bad : "file size"); return 1; }
    std::vector<float> rays(n * 8);
    if (n) std::memcpy(rays.data(), rays_file.data(), n * 32);
    const uint8_t* vol = file.data() + head;
    const nrc::OccupancyBits occ = nrc::build_occupancy_bits(vol, nx, ny, nz, 2048);
    const nrc::AovGrid g{nx, ny, nz, {f[0], f[1], f[2]}, f[3], occ.shift, occ.gx, occ.gy};
    const nrc::AovVolumeBytes density{vol, nx, ny};
    const nrc::AovOccupancyBits occupied{occ.bits.data()};
    const float nan = std::nanf("");
    std::vector<float> za((size_t)K * n, nan), zb((size_t)K * n, nan), flat(n * 4);
    std::vector<uint32_t> calls(K);
    size_t differ = 0, flat_differ = 0, emitted_wrong = 0;
    for (size_t i = 0; i < n; i++) {
        const float* q = &rays[i * 8];
        const nrc::AovRay ray{{q[0], q[1], q[2]}, {q[4], q[5], q[6]}};
        std::fill(calls.begin(), calls.end(), 0u);
        CountingSink sa{&za[i], n, calls.data()};
        const nrc::ViewAov a = nrc::deep_aov_walk_range(g, ray, q[3], q[7], density, nrc::NoOccupancy{}, levels.data(), K, &sa);
        for (uint32_t k = 0; k < K; k++)
            if (calls[k] != 1u && emitted_wrong++ < 8) std::printf("FAILED: ray %zu, level %u emitted %u times by the plain walk\n", i, k, calls[k]);
        std::fill(calls.begin(), calls.end(), 0u);
        CountingSink sb{&zb[i], n, calls.data()};
        const nrc::ViewAov b = nrc::deep_aov_walk_range(g, ray, q[3], q[7], density, occupied, levels.data(), K, &sb);
        for (uint32_t k = 0; k < K; k++)
            if (calls[k] != 1u && emitted_wrong++ < 8) std::printf("FAILED: ray %zu, level %u emitted %u times by the walk with jumps\n", i, k, calls[k]);
        bool same = std::memcmp(&a, &b, sizeof(a)) == 0;
        for (uint32_t k = 0; k < K; k++) same = same && std::memcmp(&za[(size_t)k * n + i], &zb[(size_t)k * n + i], 4) == 0;
        if (!same && differ++ < 8) std::printf("FAILED: ray %zu: the plain deep walk and the one with jumps differ\n", i);
        const nrc::ViewAov c = nrc::view_aov_walk_range(g, ray, q[3], q[7], density, nrc::NoOccupancy{});
        if (std::memcmp(&a, &c, sizeof(a)) != 0 && flat_differ++ < 8)
            std::printf("FAILED: ray %zu: flat {%a, %a, %a, %a} against the range walk's {%a, %a, %a, %a}\n", i, a.alpha, a.tau, a.z_front, a.z_half,
                        c.alpha, c.tau, c.z_front, c.z_half);
        std::memcpy(&flat[i * 4], &a, sizeof(a));
    }
    FILE* out = std::fopen(out_path, "wb");
    if (!out) { std::printf("FAILED: cannot write %s\n", out_path); return 1; }
    const bool ok = write_all(out, za.data(), za.size() * 4) && write_all(out, flat.data(), flat.size() * 4);
    if (std::fclose(out) != 0 || !ok) { std::printf("FAILED: cannot write %s\n", out_path); return 1; }
    std::printf("deep_aov: %zu rays, %u levels, %zu differ between the plain walk and the walk with jumps; %zu flat results differ from the range "
                "walk; %zu levels not emitted exactly once\n", n, K, differ, flat_differ, emitted_wrong);
    return differ == 0 && flat_differ == 0 && emitted_wrong == 0 ? 0 : 1;
}

int main(int argc, char** argv)
{
    if (argc == 6 && std::string(argv[1]) == "rays") return run_rays(argv[2], argv[3], argv[4], argv[5]);
    std::printf("FAILED: usage: deep_aov_main rays <scene> <rays> <levels> <out>\n");
    return 2;
}
