// denoise_main -- csrc/nrc_denoise.hpp on the CPU, device-free, built with ASan + UBSan and run directly (tests/test_denoise_cpu.py).
//   denoise_main <in file> <out file>
//     in file: uint32 {w, h, passes}, float {sigma_alpha, sigma_depth, sigma_color, color_decay}, then rgba [h][w][4] and aov [h][w][4]
//     floats.  out file: the filtered image [h][w][4].  Parameters the header refuses are reported and the program fails.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "nrc_denoise.hpp"

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

int main(int argc, char** argv)
{
    if (argc != 3) { std::printf("FAILED: usage: denoise_main <in file> <out file>\n"); return 2; }
    std::vector<unsigned char> file;
    if (!read_all(argv[1], &file)) { std::printf("FAILED: cannot read %s\n", argv[1]); return 1; }
    uint32_t u[3];
    float f[4];
    const size_t head = sizeof(u) + sizeof(f);
    if (file.size() < head) { std::printf("FAILED: short input file\n"); return 1; }
    std::memcpy(u, file.data(), sizeof(u));
    std::memcpy(f, file.data() + sizeof(u), sizeof(f));
    const uint32_t w = u[0], h = u[1];
    const nrc::DenoiseParams p{u[2], f[0], f[1], f[2], f[3]};
    if (const char* what = nrc::denoise_params_error(p)) { std::printf("FAILED: %s\n", what); return 1; }
    if (w == 0 || h == 0 || w > nrc::kDenoiseMaxSide || h > nrc::kDenoiseMaxSide) { std::printf("FAILED: image size\n"); return 1; }
    const size_t n = (size_t)w * h * 4;
    if (file.size() != head + 2 * n * sizeof(float)) { std::printf("FAILED: input file size\n"); return 1; }
    std::vector<float> rgba(n), aov(n), out(n);
    std::memcpy(rgba.data(), file.data() + head, n * sizeof(float));
    std::memcpy(aov.data(), file.data() + head + n * sizeof(float), n * sizeof(float));
    nrc::denoise_host(rgba.data(), aov.data(), w, h, p, out.data());
    if (!write_all(argv[2], out.data(), n * sizeof(float))) { std::printf("FAILED: cannot write %s\n", argv[2]); return 1; }
    std::printf("%u x %u, %u passes\n", w, h, p.passes);
    return 0;
}
