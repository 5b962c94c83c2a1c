// reproject_main -- csrc/nrc_reproject.hpp on the CPU, device-free, built with ASan + UBSan and run directly (tests/test_reproject_cpu.py).
//   reproject_main <in file> <out file>
//     in file: uint32 {w, h, has_history}, float {max_history, sigma_alpha, sigma_depth, frames}, the current camera {inv_proj_view[16], pos[3]},
//     the history camera likewise (ignored without history), then rgba [h][w][4] and aov [h][w][4] floats and, with history, hist_rgba
//     [h][w][4], hist_count [h][w], hist_aov [h][w][4].  out file: out [h][w][4], then the counts [h][w].  Arguments the header refuses are
//     reported and the program fails.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "nrc_reproject.hpp"

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
    if (argc != 3) { std::printf("FAILED: usage: reproject_main <in file> <out file>\n"); return 2; }
    std::vector<unsigned char> file;
    if (!read_all(argv[1], &file)) { std::printf("FAILED: cannot read %s\n", argv[1]); return 1; }
    uint32_t u[3];
    float f[4 + 19 + 19];
    const size_t head = sizeof(u) + sizeof(f);
    if (file.size() < head) { std::printf("FAILED: short input file\n"); return 1; }
    std::memcpy(u, file.data(), sizeof(u));
    std::memcpy(f, file.data() + sizeof(u), sizeof(f));
    const uint32_t w = u[0], h = u[1];
    const bool hist = u[2] != 0u;
    const nrc::ReprojectParams p{f[0], f[1], f[2]};
    if (const char* what = nrc::reproject_params_error(p)) { std::printf("FAILED: %s\n", what); return 1; }
    const float *cam = f + 4, *hcam = f + 4 + 19;
    nrc::ReprojectView v;
    if (const char* what = nrc::reproject_setup(hist ? hcam : nullptr, hist ? hcam + 16 : nullptr, cam, cam + 16, w, h, f[3], p, &v)) {
        std::printf("FAILED: %s\n", what);
        return 1;
    }
    const size_t px = (size_t)w * h, n = px * 4;
    if (file.size() != head + (2 * n + (hist ? 2 * n + px : 0)) * sizeof(float)) { std::printf("FAILED: input file size\n"); return 1; }
    std::vector<float> rgba(n), aov(n), hist_rgba(hist ? n : 0), hist_n(hist ? px : 0), hist_aov(hist ? n : 0), out(n), out_n(px);
    const unsigned char* at = file.data() + head;
    auto take = [&](std::vector<float>* dst) {
        if (!dst->empty()) std::memcpy(dst->data(), at, dst->size() * sizeof(float));
        at += dst->size() * sizeof(float);
    };
    take(&rgba); take(&aov); take(&hist_rgba); take(&hist_n); take(&hist_aov);
    nrc::reproject_host(hist ? hist_rgba.data() : nullptr, hist ? hist_n.data() : nullptr, hist ? hist_aov.data() : nullptr, rgba.data(), aov.data(), w, h, v,
                        out.data(), out_n.data());
    out.insert(out.end(), out_n.begin(), out_n.end());
    if (!write_all(argv[2], out.data(), out.size() * sizeof(float))) { std::printf("FAILED: cannot write %s\n", argv[2]); return 1; }
    std::printf("%u x %u, %s\n", w, h, hist ? "history" : "no history");
    return 0;
}
