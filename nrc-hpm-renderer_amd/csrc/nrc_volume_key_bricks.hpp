// nrc_volume_key_bricks.hpp -- the device-free part of nrc_renderer_set_volume_key_bricks (include/nrc_hpm.h): a key sequence held as
// lists of 8^3 bricks.  Where every key's bricks start in the concatenated array, what the sequence costs in device bytes, and the checks
// a call has to pass before anything is allocated (counts and sizes that do not fit, host origins).  Standard library only
// (tests/cpp/volume_key_bricks_main.cpp runs it on the CPU under the sanitizers).
#pragma once
#include <cstddef>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "nrc_fail.hpp"

namespace nrc {

constexpr size_t kBrickVoxels = 512;      // 8 x 8 x 8

// the 8^3 cells of a volume (dims that are no multiples of 8: the last cell of an axis is cut)
inline size_t volume_cell_count(uint32_t nx, uint32_t ny, uint32_t nz)
{
    return (((size_t)nx + 7u) / 8u) * (((size_t)ny + 7u) / 8u) * (((size_t)nz + 7u) / 8u);
}

// a * b, or fail(who + ...) when the product does not fit a size_t
inline size_t checked_mul(size_t a, size_t b, const std::string& who, const char* what)
{
    if (a != 0 && b > std::numeric_limits<size_t>::max() / a) fail(who + ": " + what + " does not fit the address space (" + std::to_string(a) + " x " + std::to_string(b) + ")");
    return a * b;
}
inline size_t checked_add(size_t a, size_t b, const std::string& who, const char* what)
{
    if (b > std::numeric_limits<size_t>::max() - a) fail(who + ": " + what + " does not fit the address space (" + std::to_string(a) + " + " + std::to_string(b) + ")");
    return a + b;
}

// what a dense key sequence holds on the device: n_keys R8 volumes
inline size_t dense_key_bytes(uint32_t n_keys, uint32_t nx, uint32_t ny, uint32_t nz) { return (size_t)n_keys * nx * ny * nz; }

// Where the keys' lists lie in the concatenated arrays, and what the sequence holds on the device.
struct KeyBrickLayout {
    std::vector<uint32_t> first;      // n_keys + 1 entries: key k's bricks are first[k] .. first[k + 1] - 1 of the concatenated array
    uint32_t n_keys = 0;
    uint32_t total = 0;               // first[n_keys]: all bricks
    size_t cells = 0;                 // 8^3 cells of the volume = words of one key's cell_brick index
    size_t brick_bytes = 0;           // 512 * total: the R8 bricks
    size_t index_bytes = 0;           // 4 * n_keys * cells: the keys' cell_brick indices
    size_t held_bytes() const { return brick_bytes + index_bytes; }      // nrc_renderer_volume_key_bytes
    uint32_t count(uint32_t k) const { return first[k + 1] - first[k]; }
};

// Throws (fail) unless the sequence can be laid out: key_counts not NULL, the bricks numbered 1 + index in 32 bits (cell_brick's words;
// 0 is "no brick"), and every size -- the source of `element_bytes` per voxel included -- inside a size_t.  n_keys == 0: the empty layout.
inline KeyBrickLayout key_brick_layout(const std::string& who, const uint32_t* key_counts, uint32_t n_keys, uint32_t nx, uint32_t ny, uint32_t nz,
                                       size_t element_bytes = 1)
{
    KeyBrickLayout l;
    l.first.assign(1, 0u);
    if (n_keys == 0) return l;
    if (!key_counts) fail(who + ": key_counts is NULL (" + std::to_string(n_keys) + " keys)");
    l.n_keys = n_keys;
    l.first.reserve((size_t)n_keys + 1);
    uint64_t total = 0;
    for (uint32_t k = 0; k < n_keys; k++) {
        total += key_counts[k];
        if (total >= 0xffffffffull)
            fail(who + ": the keys up to key " + std::to_string(k) + " hold " + std::to_string(total) + " bricks, more than a 32-bit brick number can name");
        l.first.push_back((uint32_t)total);
    }
    l.total = (uint32_t)total;
    l.cells = checked_mul(checked_mul(volume_cell_count(nx, 1, 1), volume_cell_count(1, ny, 1), who, "the volume's cells"), volume_cell_count(1, 1, nz), who,
                          "the volume's cells");
    l.brick_bytes = checked_mul((size_t)l.total, kBrickVoxels, who, "the bricks' size");
    (void)checked_mul(l.brick_bytes, element_bytes, who, "the source bricks' size");
    (void)checked_mul((size_t)l.total, 12, who, "the origins' size");
    l.index_bytes = checked_mul(checked_mul(l.cells, 4, who, "a key's cell index"), (size_t)n_keys, who, "the keys' cell indices");
    (void)checked_add(l.brick_bytes, l.index_bytes, who, "the sequence's size");
    return l;
}

// the rule of nrc_renderer_set_volume_bricks: every component a multiple of 8 inside the volume
inline bool brick_origin_valid(const int32_t* o, uint32_t nx, uint32_t ny, uint32_t nz)
{
    const uint32_t dims[3] = {nx, ny, nz};
    for (int a = 0; a < 3; a++)
        if (o[a] < 0 || o[a] % 8 != 0 || (uint32_t)o[a] >= dims[a]) return false;
    return true;
}

// a host list: throws at the first invalid origin, naming the key and the brick inside that key's list
inline void check_key_brick_origins(const std::string& who, const KeyBrickLayout& l, const int32_t* origins, uint32_t nx, uint32_t ny, uint32_t nz)
{
    for (uint32_t k = 0; k < l.n_keys; k++)
        for (uint32_t i = l.first[k]; i < l.first[k + 1]; i++) {
            const int32_t* o = origins + 3 * (size_t)i;
            if (!brick_origin_valid(o, nx, ny, nz))
                fail(who + ": key " + std::to_string(k) + ", brick " + std::to_string(i - l.first[k]) + " has origin (" + std::to_string(o[0]) + ", " +
                     std::to_string(o[1]) + ", " + std::to_string(o[2]) + "): every component must be a multiple of 8 inside the renderer's " +
                     std::to_string(nx) + "x" + std::to_string(ny) + "x" + std::to_string(nz) + " volume");
        }
}

// Bricks of one piece when a source of `total` bricks goes through a staging buffer that should hold about `budget_bytes` (at least one)
inline uint32_t key_brick_piece(uint32_t total, size_t budget_bytes, size_t element_bytes)
{
    const size_t per = kBrickVoxels * element_bytes;
    size_t n = budget_bytes / per;
    if (n < 1) n = 1;
    return n < total ? (uint32_t)n : total;
}

}  // namespace nrc
