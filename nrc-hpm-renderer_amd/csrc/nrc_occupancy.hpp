// nrc_occupancy.hpp -- what the scene upload works out on the host before anything goes to the device: the volume's size checks and its
// two occupancy structures.  Device-free: standard library only (tests/cpp/host_logic_main.cpp runs it under the sanitizers).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "nrc_fail.hpp"

namespace nrc {

inline void check_volume_size(uint32_t nx, uint32_t ny, uint32_t nz)
{
    // the kernels index voxels with 24-bit multiply-adds and read them through a raw buffer whose out-of-range offset is 2^31
    if (nx >= (1u << 24) || (size_t)ny * nz >= ((size_t)1 << 24) || (size_t)nx * ny * nz >= ((size_t)1 << 31))
        fail("density volume too large (needs nx < 2^24, ny*nz < 2^24 and fewer than 2^31 voxels)");
}

struct OccupancyBits {
    std::vector<uint32_t> bits;      // bit (cz * gy + cy) * gx + cx; bits.size() is the word count
    uint32_t shift = 0, gx = 0, gy = 0, gz = 0;
};

// exact occupancy for the kernels' LDS copy: the smallest cubic cell (>= 8 voxels) whose bit grid fits max_words words
inline OccupancyBits build_occupancy_bits(const uint8_t* density, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t max_words)
{
    uint32_t sh = 3;
    auto cells = [&](uint32_t n) { return (n + (1u << sh) - 1u) >> sh; };
    while ((uint64_t)cells(nx) * cells(ny) * cells(nz) > (uint64_t)max_words * 32u) sh++;
    const uint32_t gx = cells(nx), gy = cells(ny), gz = cells(nz);
    // (a multiple of four words: k_gen_rays copies the table in 16-byte pieces)
    std::vector<uint32_t> bits((((size_t)gx * gy * gz + 31) / 32 + 3) & ~(size_t)3, 0u);
    for (uint32_t z = 0; z < nz; z++)
        for (uint32_t y = 0; y < ny; y++) {
            const uint8_t* row = density + ((size_t)z * ny + y) * nx;
            const size_t base = ((size_t)(z >> sh) * gy + (y >> sh)) * gx;
            for (uint32_t x = 0; x < nx; x++)
                if (row[x]) {
                    const size_t cidx = base + (x >> sh);
                    bits[cidx >> 5] |= 1u << (cidx & 31);
                }
        }
    return OccupancyBits{std::move(bits), sh, gx, gy, gz};
}

// Occupancy of the volume in cells of 8^3 voxels: a cell counts as occupied when a non-zero voxel lies in it or within one
// voxel of it (the margin that makes the tile mask conservative against every rounding in the ray / sample arithmetic: a
// sample position is computed to ~1e-5 of a voxel).  Runs of occupied cells along x become world-space boxes {lo xyz, hi xyz}.
inline std::vector<float> build_occupancy_boxes(const uint8_t* density, uint32_t nx, uint32_t ny, uint32_t nz, const float size[3])
{
    const uint32_t gx = (nx + 7) / 8, gy = (ny + 7) / 8, gz = (nz + 7) / 8;
    std::vector<uint8_t> occ((size_t)gx * gy * gz, 0);
    for (uint32_t z = 0; z < nz; z++)
        for (uint32_t y = 0; y < ny; y++) {
            const uint8_t* row = density + ((size_t)z * ny + y) * nx;
            const uint32_t cz0 = (z ? z - 1 : 0) >> 3, cz1 = std::min(z + 1, nz - 1) >> 3;
            const uint32_t cy0 = (y ? y - 1 : 0) >> 3, cy1 = std::min(y + 1, ny - 1) >> 3;
            for (uint32_t x = 0; x < nx; x++) {
                if (row[x] == 0) continue;
                const uint32_t cx0 = (x ? x - 1 : 0) >> 3, cx1 = std::min(x + 1, nx - 1) >> 3;
                for (uint32_t cz = cz0; cz <= cz1; cz++)
                    for (uint32_t cy = cy0; cy <= cy1; cy++)
                        for (uint32_t cx = cx0; cx <= cx1; cx++) occ[((size_t)cz * gy + cy) * gx + cx] = 1;
            }
        }
    std::vector<float> boxes;
    const double vs[3] = {(double)size[0] / nx, (double)size[1] / ny, (double)size[2] / nz};
    auto world = [&](int axis, uint32_t voxel) { return (float)(-0.5 * (double)size[axis] + vs[axis] * (double)voxel); };
    for (uint32_t cz = 0; cz < gz; cz++)
        for (uint32_t cy = 0; cy < gy; cy++) {
            const uint8_t* row = &occ[((size_t)cz * gy + cy) * gx];
            for (uint32_t cx = 0; cx < gx;) {
                if (!row[cx]) { cx++; continue; }
                uint32_t e = cx;
                while (e + 1 < gx && row[e + 1]) e++;
                const float lo[3] = {world(0, 8 * cx), world(1, 8 * cy), world(2, 8 * cz)};
                const float hi[3] = {world(0, std::min(8 * (e + 1), nx)), world(1, std::min(8 * (cy + 1), ny)), world(2, std::min(8 * (cz + 1), nz))};
                boxes.insert(boxes.end(), {lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]});
                cx = e + 1;
            }
        }
    return boxes;
}

}  // namespace nrc
