// nrc_hot_tiles.hpp -- which pixels of a frame start in a capped RNG state (DevFrame::flight_list), found on the host by inverting the
// hash instead of scanning the frame.  Device-free: standard library only (tests/cpp/hot_tiles_main.cpp runs it under the sanitizers).
// The hash, the pixel's half of the seed and the column mapping are stated ONCE, here, for the kernels and for the host: NRC_HOT_HD is
// the one place of this file that knows about the device compiler (host + device functions there, plain inline functions elsewhere).
//
// init_random of pixel p with the frame's random numbers r is float_construct(hash1(a ^ h)):
//   a = bits(random2(u, v))           the pixel's half, a function of the frame's geometry alone
//   h = hash1(bits(random4(r)))       one word per frame
// hash1 is a bijection of 32 bits, so the pixel is in the capped state with mantissa c exactly when a ^ h is one of the 512 preimages
// Z_c = { unhash1(c | k << 23) : k < 512 }.  About one of the 512 candidates a = z ^ h is the bit pattern of a multiple of 2^-23 in
// [0, 1) at all -- what random2 returns -- and a per-geometry index from that multiple (the seed's 23-bit mantissa) to the pixels that
// have it says whether a pixel of this frame does.  A frame's list costs about a microsecond; nothing runs on the device.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define NRC_HOT_HD __host__ __device__ __forceinline__
#else
#define NRC_HOT_HD inline
#endif

namespace nrc {

constexpr uint32_t kFlightListMax = 8;      // most capped states handed over as a list (DevFrame::flight_list)
constexpr uint32_t kHotTilesMax = 8;        // = the waves of the two workgroups the launch gains in front

// ---- include/random.glsl:24-70
NRC_HOT_HD uint32_t hash1(uint32_t x)
{
    x += (x << 10);
    x ^= (x >> 6);
    x += (x << 3);
    x ^= (x >> 11);
    x += (x << 15);
    return x;
}
// the inverse of hash1, step by step from the last: x += x << k is a multiplication by the odd 1 + 2^k, x ^= x >> k is undone by
// repeating the shift until it runs out of bits
NRC_HOT_HD uint32_t unhash1(uint32_t x)
{
    x *= 0x3fff8001u;      // (1 + 2^15)^-1 mod 2^32
    x ^= (x >> 11) ^ (x >> 22);
    x *= 0x38e38e39u;      // 9^-1
    x ^= (x >> 6) ^ (x >> 12) ^ (x >> 18) ^ (x >> 24) ^ (x >> 30);
    x *= 0xc00ffc01u;      // 1025^-1
    return x;
}
NRC_HOT_HD uint32_t hot_f2u(float f) { return __builtin_bit_cast(uint32_t, f); }
NRC_HOT_HD float hot_u2f(uint32_t u) { return __builtin_bit_cast(float, u); }
NRC_HOT_HD float float_construct(uint32_t m) { return hot_u2f((m & 0x007fffffu) | 0x3f800000u) - 1.0f; }

// global column of local column lx (nrc_tile: strips of 2^x_block_log2 columns, every x_stride-th strip)
NRC_HOT_HD uint32_t global_x(uint32_t x_offset, uint32_t x_stride, uint32_t x_block_log2, uint32_t lx)
{
    const uint32_t b = x_block_log2;
    return ((x_offset + (lx >> b) * x_stride) << b) + (lx & ((1u << b) - 1u));
}
// The pixel's half of init_random's seed, random2(u, v) with uv = pixel * (1 / size): one rounded product per coordinate and nothing
// added to it, so no compiler can contract anything here.  seed_row: the row's term, shared by the pixels of the row.
NRC_HOT_HD uint32_t seed_row(uint32_t y, float inv_gh) { return hash1(hot_f2u((float)y * inv_gh)); }
NRC_HOT_HD uint32_t seed_mantissa(uint32_t gx, float inv_gw, uint32_t row) { return hash1(hot_f2u((float)gx * inv_gw) ^ row) & 0x007fffffu; }

struct HotGeometry {
    uint32_t w = 0, h = 0;                                    // local frame
    uint32_t x_offset = 0, x_stride = 1, x_block_log2 = 0;    // its columns in the global frame (global_x)
    float inv_gw = 0.0f, inv_gh = 0.0f;                       // the floats the kernels multiply by
    bool operator==(const HotGeometry& o) const
    {
        return w == o.w && h == o.h && x_offset == o.x_offset && x_stride == o.x_stride && x_block_log2 == o.x_block_log2 &&
               hot_f2u(inv_gw) == hot_f2u(o.inv_gw) && hot_f2u(inv_gh) == hot_f2u(o.inv_gh);
    }
};

// one entry (ty << 16 | tx) per capped pixel of the frame, in ascending pixel order (y * w + lx), a tile with two such pixels twice;
// count is their total, entries holds the first kHotTilesMax
struct HotList {
    uint32_t entries[kHotTilesMax] = {};
    uint32_t count = 0;
};

class HotTileFinder {
public:
    // the capped states (mantissas); the preimage tables are rebuilt only when the list changes
    void set_states(const uint32_t* list, uint32_t n)
    {
        n = std::min(n, kFlightListMax);
        if (n == (uint32_t)states_.size() && std::equal(states_.begin(), states_.end(), list)) return;
        states_.assign(list, list + n);
        z_.resize((size_t)n * 512u);
        for (uint32_t k = 0; k < n; k++)
            for (uint32_t hi = 0; hi < 512u; hi++) z_[(size_t)k * 512u + hi] = unhash1((states_[k] & 0x007fffffu) | (hi << 23));
    }
    // the frame's geometry; the index is rebuilt at the next hot_list when it changed
    void set_geometry(const HotGeometry& g)
    {
        if (indexed_ && g == geo_) return;
        geo_ = g;
        indexed_ = false;
    }
    bool indexed() const { return indexed_; }
    // builds the index now instead of at the next hot_list (milliseconds per megapixel: a renderer does it when it is created, so that
    // its first frame does not leave the device idle behind whatever ran before it)
    void prepare()
    {
        if (!indexed_ && geo_.w != 0 && geo_.h != 0) build_index();
    }
    // what the index keeps between frames
    size_t index_bytes() const { return (bitmap_.size() + offsets_.size() + pixels_.size()) * sizeof(uint32_t); }

    HotList hot_list(const float frame_random[4])
    {
        HotList out;
        if (states_.empty() || geo_.w == 0 || geo_.h == 0) return out;
        if (!indexed_) build_index();
        const uint32_t q = hot_f2u(float_construct(hash1(hot_f2u(frame_random[0]) ^ hash1(hot_f2u(frame_random[1])) ^ hash1(hot_f2u(frame_random[2])) ^
                                                         hash1(hot_f2u(frame_random[3])))));      // random4
        const uint32_t h = hash1(q);
        hits_.clear();
        for (const uint32_t z : z_) {
            // is a = z ^ h the bit pattern of s * 2^-23, s < 2^23?  (in integers: whatever the host does with denormals cannot matter)
            const uint32_t a = z ^ h;
            uint32_t s = 0;
            if (a != 0u) {
                const uint32_t e = a >> 23;      // sign and biased exponent: 2^-23 <= value < 1
                if (e < 104u || e > 126u) continue;
                const uint32_t down = 127u - e, m = (a & 0x007fffffu) | 0x00800000u;
                if ((m & ((1u << down) - 1u)) != 0u) continue;
                s = m >> down;
            }
            if (((bitmap_[s >> 5] >> (s & 31u)) & 1u) == 0u) continue;
            const uint32_t b = s >> bucket_shift_;
            for (uint32_t i = offsets_[b]; i < offsets_[b + 1u]; i++) {
                const uint32_t p = pixels_[i], y = p / geo_.w, lx = p - y * geo_.w;
                if (mantissa_of(lx, seed_row(y, geo_.inv_gh)) == s) hits_.push_back(p);
            }
        }
        // (a state listed twice finds its pixels twice: a pixel counts once whatever the list holds)
        std::sort(hits_.begin(), hits_.end());
        hits_.erase(std::unique(hits_.begin(), hits_.end()), hits_.end());
        out.count = (uint32_t)hits_.size();
        for (uint32_t k = 0; k < std::min(out.count, kHotTilesMax); k++) {
            const uint32_t y = hits_[k] / geo_.w, lx = hits_[k] - y * geo_.w;
            out.entries[k] = ((y >> 3) << 16) | (lx >> 3);
        }
        return out;
    }

private:
    uint32_t mantissa_of(uint32_t lx, uint32_t row) const
    {
        return seed_mantissa(global_x(geo_.x_offset, geo_.x_stride, geo_.x_block_log2, lx), geo_.inv_gw, row);
    }
    // Seed mantissa -> pixels: one presence bit per mantissa (2^23 bits; a frame fills a quarter of them at 1080p, so three of four
    // candidates end there) and the pixel indices bucketed by the mantissa's high bits, about four to a bucket, in ascending order
    // inside a bucket.  4 bytes per pixel + the bitmap + the bucket offsets are kept; the mantissas themselves are not (a probe
    // recomputes those of its bucket), they exist for the duration of the build only: one hash per row and one per pixel.
    void build_index()
    {
        const size_t n = (size_t)geo_.w * geo_.h;
        uint32_t bucket_bits = 0;
        while (bucket_bits < 23u && ((size_t)4 << bucket_bits) < n) bucket_bits++;
        bucket_shift_ = 23u - bucket_bits;
        bitmap_.assign((size_t)1 << 18, 0u);
        offsets_.assign(((size_t)1 << bucket_bits) + 1u, 0u);
        pixels_.assign(n, 0u);
        std::vector<uint32_t> mant(n);
        size_t p = 0;
        for (uint32_t y = 0; y < geo_.h; y++) {
            const uint32_t row = seed_row(y, geo_.inv_gh);
            for (uint32_t lx = 0; lx < geo_.w; lx++, p++) {
                const uint32_t s = mantissa_of(lx, row);
                mant[p] = s;
                bitmap_[s >> 5] |= 1u << (s & 31u);
                offsets_[(s >> bucket_shift_) + 1u]++;
            }
        }
        for (size_t b = 1; b < offsets_.size(); b++) offsets_[b] += offsets_[b - 1];
        // (offsets_[b] serves as bucket b's fill position and ends up as its end = bucket b + 1's begin: shifted back below)
        for (p = 0; p < n; p++) pixels_[offsets_[mant[p] >> bucket_shift_]++] = (uint32_t)p;
        for (size_t b = offsets_.size() - 1; b > 0; b--) offsets_[b] = offsets_[b - 1];
        offsets_[0] = 0;
        indexed_ = true;
    }

    std::vector<uint32_t> states_, z_;
    HotGeometry geo_;
    bool indexed_ = false;
    uint32_t bucket_shift_ = 23;
    std::vector<uint32_t> bitmap_, offsets_, pixels_, hits_;
};

}  // namespace nrc
