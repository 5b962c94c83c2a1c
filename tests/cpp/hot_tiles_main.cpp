// hot_tiles_main.cpp -- the host's hot-tile search (csrc/nrc_hot_tiles.hpp) driven on the CPU; tests/test_hot_tiles_host.py builds this
// with AddressSanitizer + UndefinedBehaviorSanitizer and runs it.
// The search inverts the RNG's hash; the reference here does what the device pre-pass did: it visits EVERY pixel of the frame, computes
// its initial RNG state from the pixel's coordinates (init_random, random.glsl:61-64) and compares the mantissa with the capped states.
// Every CHECK compares a value; the last line printed is "hot_tiles: <n> cases, <m> checks" (exit status 1 if any check failed).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../nrc-hpm-renderer_amd/csrc/nrc_hot_tiles.hpp"

using namespace nrc;

static int g_cases = 0, g_checks = 0, g_failed = 0;
static const char* g_case = "";
#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        g_checks++;                                                                                          \
        if (!(cond)) { g_failed++; std::printf("FAILED %s:%d [%s] %s\n", __FILE__, __LINE__, g_case, #cond); } \
    } while (0)
static void begin_case(const char* name) { g_case = name; g_cases++; }

// ---- the reference: random.glsl restated with nothing shared but hash1 (whose values the first case pins)
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float construct(uint32_t m) { const uint32_t u = (m & 0x007fffffu) | 0x3f800000u; float f; std::memcpy(&f, &u, 4); return f - 1.0f; }
static float ref_random2(float x, float y) { return construct(hash1(bits(x) ^ hash1(bits(y)))); }
static float ref_random4(const float* v) { return construct(hash1(bits(v[0]) ^ hash1(bits(v[1])) ^ hash1(bits(v[2])) ^ hash1(bits(v[3])))); }

// a local frame: columns x_offset, x_offset + x_stride, ... in strips of 2^block_log2 of a gw x gh global frame
struct Frame {
    uint32_t w, h, gw, gh, x_offset, x_stride, block_log2;
    HotGeometry geometry() const { return HotGeometry{w, h, x_offset, x_stride, block_log2, 1.0f / (float)gw, 1.0f / (float)gh}; }
    uint32_t gx(uint32_t lx) const { return ((x_offset + (lx >> block_log2) * x_stride) << block_log2) + (lx & ((1u << block_log2) - 1u)); }
};
static Frame whole(uint32_t w, uint32_t h) { return Frame{w, h, w, h, 0, 1, 0}; }
// rank `rank` of `world` ranks' column strips of 8 (nrc_tile: x_block 8) of a gw x gh frame
static Frame shard(uint32_t gw, uint32_t gh, uint32_t world, uint32_t rank)
{
    const uint32_t strips = gw / 8u, mine = (strips - rank + world - 1u) / world;
    return Frame{mine * 8u, gh, gw, gh, rank, world, 3};
}
// bits(seed_uv) of every pixel: the pixel's half of init_random's seed, from the pixel's coordinates
static std::vector<uint32_t> pixel_seeds(const Frame& f)
{
    std::vector<uint32_t> a((size_t)f.w * f.h);
    const float inv_gw = 1.0f / (float)f.gw, inv_gh = 1.0f / (float)f.gh;
    for (uint32_t y = 0; y < f.h; y++)
        for (uint32_t lx = 0; lx < f.w; lx++) a[(size_t)y * f.w + lx] = bits(ref_random2((float)f.gx(lx) * inv_gw, (float)y * inv_gh));
    return a;
}
// the scan: every pixel's initial state against the capped states -> the capped pixels {pixel index, mantissa} in pixel order.  (A pixel's
// mantissa is first looked up in a 4096-bit summary of the states' low twelve bits, which no state's mantissa misses, then compared with the states.)
struct Capped { uint32_t pixel, mantissa; };
static std::vector<Capped> scan(const std::vector<uint32_t>& seeds, const float* frame_random, const uint32_t* states, uint32_t n_states)
{
    std::vector<Capped> out;
    const uint32_t h = hash1(bits(ref_random4(frame_random)));
    uint64_t summary[64] = {};
    for (uint32_t k = 0; k < n_states; k++) summary[(states[k] >> 6) & 63u] |= 1ull << (states[k] & 63u);
    const uint32_t* a = seeds.data();
    const size_t n = seeds.size();
    for (size_t p = 0; p < n; p++) {
        const uint32_t m = hash1(a[p] ^ h) & 0x007fffffu;      // mantissa of random2(seed_uv, random4(frame random))
        if (((summary[(m >> 6) & 63u] >> (m & 63u)) & 1ull) == 0ull) continue;
        bool capped = false;
        for (uint32_t k = 0; k < n_states; k++) capped |= m == states[k];
        if (capped) out.push_back(Capped{(uint32_t)p, m});
    }
    return out;
}
// the list of the capped pixels whose state is among `states` (the scan's own, or some of them)
static HotList list_of(const Frame& f, const std::vector<Capped>& capped, const uint32_t* states, uint32_t n_states)
{
    HotList out;
    for (const Capped& c : capped) {
        if (std::find(states, states + n_states, c.mantissa) == states + n_states) continue;
        const uint32_t y = c.pixel / f.w, lx = c.pixel - y * f.w;
        if (out.count < kHotTilesMax) out.entries[out.count] = ((y >> 3) << 16) | (lx >> 3);
        out.count++;
    }
    return out;
}
static HotList brute(const Frame& f, const std::vector<uint32_t>& seeds, const float* frame_random, const uint32_t* states, uint32_t n_states)
{
    return list_of(f, scan(seeds, frame_random, states, n_states), states, n_states);
}
static bool same(const HotList& a, const HotList& b)
{
    if (a.count != b.count) return false;
    for (uint32_t k = 0; k < kHotTilesMax; k++)
        if (a.entries[k] != b.entries[k]) return false;      // (the entries past the count are zero on both sides)
    return true;
}
static void draw(std::mt19937& rng, float* r4)
{
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    for (int k = 0; k < 4; k++) r4[k] = u(rng);
}

// tests/test_gpu_integrator.py: pixel (2, 3) of a 256x144 frame starts in state 0 / pixels (1080, 90) and (1083, 90) of a 1920x1080 frame do
static const float kState0Random[4] = {0.7795426845550537f, 0.04615384712815285f, 0.75f, 0.125f};
static const float kPairRandom[4] = {0.6137924194335938f, 0.015384615398943424f, 0.75f, 0.125f};
static const uint32_t kState0[1] = {0u};
// eight capped states: the RNG's fixed point and seven arbitrary mantissas
static const uint32_t kEight[8] = {0u, 1u, 0x7fffffu, 0x400000u, 0x123456u, 0x2aaaaau, 0x555555u, 0x0f0f0fu};

static void hash_cases()
{
    begin_case("unhash1 inverts hash1");
    {
        CHECK(hash1(0u) == 0u);      // the chain's fixed point
        // values of numpy's restatement (tests/rng_search.py)
        CHECK(hash1(1u) == 0x124ea49du && hash1(0x3f800000u) == 0xf2496dc0u && unhash1(1u) == 0x4a60aae5u);
        uint32_t bad = 0;
        std::mt19937 rng(7);
        for (uint32_t i = 0; i < (1u << 20); i++) {
            const uint32_t x = rng();
            bad += unhash1(hash1(x)) != x;
            bad += hash1(unhash1(x)) != x;
            bad += unhash1(hash1(i)) != i;      // the small values too
        }
        CHECK(bad == 0u);
        const uint32_t edges[] = {0u, 1u, 2u, 0x7fffffu, 0x800000u, 0x3f800000u, 0x3f7fffffu, 0x7fffffffu, 0x80000000u, 0x80000001u, 0xfffffffeu, 0xffffffffu};
        for (const uint32_t x : edges) { CHECK(unhash1(hash1(x)) == x); CHECK(hash1(unhash1(x)) == x); }
        for (uint32_t b = 0; b < 32; b++) { CHECK(unhash1(hash1(1u << b)) == (1u << b)); CHECK(unhash1(hash1(~(1u << b))) == ~(1u << b)); }
        CHECK(float_construct(0u) == 0.0f && float_construct(0x7fffffu) == 1.0f - 1.1920928955078125e-7f && float_construct(0xff800000u) == 0.0f);
        CHECK(global_x(0, 1, 0, 17) == 17u && global_x(1, 2, 3, 0) == 8u && global_x(1, 2, 3, 9) == 25u && global_x(5, 8, 3, 239) == ((5u + 29u * 8u) << 3) + 7u);
    }
}

// 1000 seeded frame randoms: the finder with the one state of the bench scene and with eight states against ONE scan per frame
// (the capped pixels of the first state alone are those of the eight whose mantissa is that state).  Returns the hits of the eight.
static uint32_t sweep(const Frame& f, uint32_t seed, uint32_t frames = 1000)
{
    const std::vector<uint32_t> seeds = pixel_seeds(f);
    HotTileFinder one, eight;
    one.set_states(kState0, 1);
    one.set_geometry(f.geometry());
    eight.set_states(kEight, 8);
    eight.set_geometry(f.geometry());
    std::mt19937 rng(seed);
    uint32_t bad = 0, hits = 0;
    for (uint32_t i = 0; i < frames; i++) {
        float r[4];
        draw(rng, r);
        const std::vector<Capped> capped = scan(seeds, r, kEight, 8);
        bad += !same(eight.hot_list(r), list_of(f, capped, kEight, 8));
        bad += !same(one.hot_list(r), list_of(f, capped, kState0, 1));
        hits += (uint32_t)capped.size();
    }
    CHECK(bad == 0u);
    // 4 B per pixel + the 1 MB bitmap + the bucket offsets (at most one per pixel, + 1)
    CHECK(one.index_bytes() <= (size_t)f.w * f.h * 4u + (1u << 20) + ((size_t)f.w * f.h + 2u) * 4u);
    return hits;
}

static void sweep_cases()
{
    begin_case("8x8: whole, and as a strip of a 16- and a 64-wide frame");
    sweep(whole(8, 8), 1);
    sweep(Frame{8, 8, 16, 8, 1, 2, 3}, 2);
    sweep(Frame{8, 8, 64, 8, 5, 8, 3}, 3);
    begin_case("64x40 (edge tiles): whole, world 2, world 8");
    sweep(whole(64, 40), 4);
    sweep(shard(64, 40, 2, 1), 5);
    sweep(shard(64, 40, 8, 5), 6);
    begin_case("256x144: whole, world 2, world 8");
    sweep(whole(256, 144), 7);
    sweep(shard(256, 144, 2, 1), 8);
    sweep(shard(256, 144, 8, 5), 9);
    begin_case("1920x1080: whole, world 2, world 8");
    const uint32_t hits = sweep(whole(1920, 1080), 10);
    std::printf("1920x1080, 1000 frames, 8 states: %u capped pixels\n", hits);
    CHECK(hits >= 1u);
    sweep(shard(1920, 1080, 2, 1), 11);
    sweep(shard(1920, 1080, 8, 5), 12);
}

static void pinned_cases()
{
    begin_case("the state-0 frame of 256x144: pixel (2, 3)");
    {
        const Frame f = whole(256, 144);
        HotTileFinder hf;
        hf.set_states(kState0, 1);
        hf.set_geometry(f.geometry());
        const HotList l = hf.hot_list(kState0Random);
        CHECK(l.count == 1u && l.entries[0] == 0u);
        CHECK(same(l, brute(f, pixel_seeds(f), kState0Random, kState0, 1)));
        CHECK(ref_random2(ref_random2(2.0f * (1.0f / 256.0f), 3.0f * (1.0f / 144.0f)), ref_random4(kState0Random)) == 0.0f);
        // the rank that owns column 2 of the world-2 frame finds it too, the other does not
        for (uint32_t rank = 0; rank < 2; rank++) {
            const Frame s = shard(256, 144, 2, rank);
            hf.set_geometry(s.geometry());
            const HotList ls = hf.hot_list(kState0Random);
            CHECK(ls.count == (rank == 0 ? 1u : 0u));
            CHECK(same(ls, brute(s, pixel_seeds(s), kState0Random, kState0, 1)));
        }
    }
    begin_case("the pair frame of 1920x1080: tile (135, 11) twice");
    {
        const Frame f = whole(1920, 1080);
        HotTileFinder hf;
        hf.set_states(kState0, 1);
        hf.set_geometry(f.geometry());
        const HotList l = hf.hot_list(kPairRandom);
        CHECK(l.count == 2u && l.entries[0] == ((11u << 16) | 135u) && l.entries[1] == ((11u << 16) | 135u) && l.entries[2] == 0u);
        CHECK(same(l, brute(f, pixel_seeds(f), kPairRandom, kState0, 1)));
    }
}

static void truncation_case()
{
    begin_case("more than eight capped pixels: the first eight in pixel order, the total counted");
    // eight states chosen as the initial states of pixels that share their seed with another pixel of the frame (36 864 pixels on 2^23
    // seeds: some eighty such pairs): every state is then reached by two pixels at least
    const Frame f = whole(256, 144);
    const std::vector<uint32_t> seeds = pixel_seeds(f);
    std::vector<uint32_t> sorted = seeds;
    std::sort(sorted.begin(), sorted.end());
    std::vector<uint32_t> twins;
    for (size_t i = 1; i < sorted.size(); i++)
        if (sorted[i] == sorted[i - 1] && (twins.empty() || twins.back() != sorted[i])) twins.push_back(sorted[i]);
    CHECK(twins.size() >= 8u);
    if (twins.size() < 8u) return;
    std::mt19937 rng(21);
    float r[4];
    draw(rng, r);
    const uint32_t h = hash1(bits(ref_random4(r)));
    uint32_t states[8];
    for (uint32_t k = 0; k < 8; k++) states[k] = hash1(twins[twins.size() - 1u - k * (uint32_t)(twins.size() / 8u)] ^ h) & 0x007fffffu;
    HotTileFinder hf;
    hf.set_states(states, 8);
    hf.set_geometry(f.geometry());
    const HotList got = hf.hot_list(r), want = brute(f, seeds, r, states, 8);
    CHECK(want.count >= 16u);
    CHECK(same(got, want));
    std::printf("truncation: %u capped pixels, eight entries kept\n", got.count);
    // fewer states again: the preimage tables follow the list
    hf.set_states(states, 3);
    CHECK(same(hf.hot_list(r), brute(f, seeds, r, states, 3)));
    hf.set_states(states + 4, 2);
    CHECK(same(hf.hot_list(r), brute(f, seeds, r, states + 4, 2)));
    hf.set_states(nullptr, 0);
    CHECK(hf.hot_list(r).count == 0u);
}

static void rebuild_case()
{
    begin_case("the index follows the geometry");
    const Frame a = whole(256, 144), b = shard(256, 144, 2, 1), c = whole(64, 40);
    const std::vector<uint32_t> sa = pixel_seeds(a), sb = pixel_seeds(b), sc = pixel_seeds(c);
    HotTileFinder hf;
    hf.set_states(kEight, 8);
    CHECK(!hf.indexed());
    std::mt19937 rng(33);
    uint32_t bad = 0, hits = 0;
    const Frame* order[] = {&a, &b, &a, &c, &b, &c, &a};
    const std::vector<uint32_t>* seeds[] = {&sa, &sb, &sa, &sc, &sb, &sc, &sa};
    for (int round = 0; round < 7; round++) {
        hf.set_geometry(order[round]->geometry());
        CHECK(!hf.indexed());      // another geometry than the one before: built again at the next list
        for (int i = 0; i < 300; i++) {
            float r[4];
            draw(rng, r);
            const HotList want = brute(*order[round], *seeds[round], r, kEight, 8);
            bad += !same(hf.hot_list(r), want);
            hits += want.count;
        }
        CHECK(hf.indexed());
        hf.set_geometry(order[round]->geometry());
        CHECK(hf.indexed());       // the same geometry: kept
    }
    CHECK(bad == 0u);
    CHECK(hits >= 1u);
    // the state-0 frame after the changes
    hf.set_states(kState0, 1);
    hf.set_geometry(a.geometry());
    const HotList l = hf.hot_list(kState0Random);
    CHECK(l.count == 1u && l.entries[0] == 0u);
}

int main()
{
    hash_cases();
    sweep_cases();
    pinned_cases();
    truncation_case();
    rebuild_case();
    std::printf("hot_tiles: %d cases, %d checks\n", g_cases, g_checks);
    return g_failed ? 1 : 0;
}
