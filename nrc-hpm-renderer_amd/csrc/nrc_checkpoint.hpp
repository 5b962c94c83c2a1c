// nrc_checkpoint.hpp -- the checkpoint file of nrc_cache_save_checkpoint / _load_checkpoint: a 64-byte header that names the model, then
// the four parameter vectors (weights, two Adam moments, EMA weights) in tiny-cuda-nn layout, fp32.  Device-free: the C ABI functions
// copy from / to the device and convert the layout; this file reads, writes and judges (tests/cpp/host_logic_main.cpp runs it under
// the sanitizers).  The step number travels in the header; the non-finite guard's counter of skipped steps (nrc_cache_get_skipped_steps)
// does not: it is a statistic of the process, not state of the model.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/nrc_hpm.h"

namespace nrc {

struct CkptHeader {
    char magic[8];
    uint32_t pos_id, dir_id, width, depth, hash_log2, n_tcnn, step;
    uint32_t zero[7];
};
static_assert(sizeof(CkptHeader) == 64, "checkpoint header is 64 bytes");

inline CkptHeader ckpt_header_of(const nrc_config& cfg, uint32_t n_tcnn, uint32_t step)
{
    CkptHeader h{};
    std::memcpy(h.magic, "NRCCKPT1", 8);
    h.pos_id = cfg.pos_id; h.dir_id = cfg.dir_id; h.width = cfg.nn_width; h.depth = cfg.nn_depth;
    h.hash_log2 = cfg.pos_id == 0 ? (cfg.hashgrid_log2_size ? cfg.hashgrid_log2_size : 19u) : 0u;
    h.n_tcnn = n_tcnn;
    h.step = step;
    return h;
}

// writes the header, then the four vectors as fill(which, t) hands them over (t holds h.n_tcnn floats), one after the other
template <class Fill>
inline void ckpt_write(const char* path, const CkptHeader& h, Fill&& fill)
{
    std::vector<float> t(h.n_tcnn);
    FILE* f = std::fopen(path, "wb");
    if (!f) throw std::runtime_error(std::string("SkyRenderer ERROR: cannot write checkpoint ") + path);
    struct Close { FILE*& f; ~Close() { if (f) std::fclose(f); } } close_on_throw{f};
    bool ok = std::fwrite(&h, sizeof h, 1, f) == 1;
    for (int which = 0; which < 4 && ok; which++) {
        fill(which, t);
        ok = std::fwrite(t.data(), 4, t.size(), f) == t.size();
    }
    ok = (std::fclose(f) == 0) && ok;
    f = nullptr;
    if (!ok) throw std::runtime_error(std::string("SkyRenderer ERROR: short write to checkpoint ") + path);
}

// the four vectors of a file that is exactly a checkpoint of the model `want` describes (want.step is not compared); *step: the file's
inline std::vector<std::vector<float>> ckpt_read(const char* path, const CkptHeader& want, uint32_t* step)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("SkyRenderer ERROR: cannot read checkpoint ") + path);
    CkptHeader h{};
    std::vector<std::vector<float>> t(4, std::vector<float>(want.n_tcnn));
    bool ok = std::fread(&h, sizeof h, 1, f) == 1;
    const bool same = ok && std::memcmp(h.magic, want.magic, 8) == 0 && h.pos_id == want.pos_id && h.dir_id == want.dir_id &&
                      h.width == want.width && h.depth == want.depth && h.hash_log2 == want.hash_log2 && h.n_tcnn == want.n_tcnn;
    for (int which = 0; which < 4 && same; which++) ok = ok && std::fread(t[which].data(), 4, want.n_tcnn, f) == want.n_tcnn;
    const bool at_end = ok && same && std::fgetc(f) == EOF;
    std::fclose(f);
    if (!ok) throw std::runtime_error(std::string("SkyRenderer ERROR: checkpoint is truncated: ") + path);
    if (!same) throw std::runtime_error(std::string("SkyRenderer ERROR: checkpoint is not of this model (encoding / width / depth / table size): ") + path);
    if (!at_end) throw std::runtime_error(std::string("SkyRenderer ERROR: checkpoint has trailing bytes: ") + path);
    *step = h.step;
    return t;
}

}  // namespace nrc
