// nrc_volume_keys.hpp -- the arithmetic of volume keyframes (include/nrc_hpm.h, nrc_renderer_set_volume_keys): a time's key pair and
// integer weight, and the in-between voxel.  Device-free: standard library only, shared by the host layer and k_vol_ingest's VolLerp source
// (tests/cpp/volume_keys_main.cpp runs it on the CPU under the sanitizers).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define NRC_KEYS_HD __host__ __device__ __forceinline__
#else
#define NRC_KEYS_HD inline
#endif

namespace nrc {

struct KeyTime {
    uint32_t i = 0;      // the pair is keys i and i + 1 (key i alone when w == 0)
    uint32_t w = 0;      // 0 .. 256: the weight of key i + 1 in 1/256
};

// key i sits at time i.  false unless t is finite and inside [0, n_keys - 1] (no keys: every time is outside).
// i = min((uint32)t, n_keys - 1), w = t - i in fp32, W = (uint32)(w * 256 + 0.5): at the last key W = 0, so key i + 1 is read only where
// it exists.  (w * 256 is exact, so the sum rounds once whether or not the compiler contracts it.)
inline bool key_of_time(float t, uint32_t n_keys, KeyTime* out)
{
    if (n_keys == 0 || !std::isfinite(t) || t < 0.0f || t > (float)(n_keys - 1)) return false;
    uint32_t i = (uint32_t)t;
    if (i > n_keys - 1) i = n_keys - 1;
    const float w = t - (float)i;
    out->i = i;
    out->w = (uint32_t)(w * 256.0f + 0.5f);
    return true;
}

// the in-between R8 voxel, in integers (bit-exact everywhere): W = 0 gives a, W = 256 gives b, and the result lies between the two
NRC_KEYS_HD uint32_t lerp_voxel(uint32_t a, uint32_t b, uint32_t W)
{
    return (a * (256u - W) + b * W + 128u) >> 8;
}

// four voxels at once, one per byte of x and y: two pairs of 16-bit fields, each at most 255 * 256 + 128 < 65536, so no carry crosses
// a field
NRC_KEYS_HD uint32_t lerp_voxels4(uint32_t x, uint32_t y, uint32_t W)
{
    const uint32_t even = (x & 0x00ff00ffu) * (256u - W) + (y & 0x00ff00ffu) * W + 0x00800080u;
    const uint32_t odd = ((x >> 8) & 0x00ff00ffu) * (256u - W) + ((y >> 8) & 0x00ff00ffu) * W + 0x00800080u;
    return ((even >> 8) & 0x00ff00ffu) | (odd & 0xff00ff00u);
}

}  // namespace nrc
