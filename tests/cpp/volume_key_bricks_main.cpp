// Stand-alone driver of csrc/nrc_volume_key_bricks.hpp (device-free), built with -fsanitize=address,undefined and run by
// tests/test_volume_key_bricks_host.py: the layout of a key sequence held as brick lists (per-key offsets, totals, the bytes held), the
// checks in front of an upload (NULL counts, brick numbers and sizes that do not fit, host origins: the message names key and brick) and
// the staging pieces.  Every list lives in a heap array of exactly its size, so a read past an end is the sanitizer's to report.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "nrc_volume_key_bricks.hpp"

static long g_checks = 0, g_failed = 0;
#define CHECK(c) do { g_checks++; if (!(c)) { g_failed++; std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

// the message of the failure f() ends in, "" when it returns
template <class F>
static std::string error_of(F f)
{
    try { f(); } catch (const std::runtime_error& e) { return e.what(); }
    return "";
}
static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

int main()
{
    using namespace nrc;
    const std::string who = "set_volume_key_bricks";

    // cells and the two byte formulas
    CHECK(volume_cell_count(8, 8, 8) == 1 && volume_cell_count(9, 8, 8) == 2 && volume_cell_count(61, 45, 70) == 8u * 6u * 9u);
    CHECK(volume_cell_count(1, 1, 1) == 1 && volume_cell_count(512, 512, 512) == 64u * 64u * 64u);
    CHECK(dense_key_bytes(0, 61, 45, 70) == 0 && dense_key_bytes(5, 61, 45, 70) == 5u * 61u * 45u * 70u);
    CHECK(dense_key_bytes(300, 2048, 2048, 2048) == (size_t)300 * 2048 * 2048 * 2048);      // (past 2^32: computed in size_t)

    // no keys: the empty layout, whatever the pointer
    {
        const KeyBrickLayout l = key_brick_layout(who, nullptr, 0, 61, 45, 70);
        CHECK(l.n_keys == 0 && l.total == 0 && l.first.size() == 1 && l.first[0] == 0 && l.held_bytes() == 0);
    }
    // offsets, counts and bytes; keys of no bricks in front, in the middle and at the end
    {
        const std::vector<uint32_t> counts = {0, 3, 0, 1233, 7, 0};
        const KeyBrickLayout l = key_brick_layout(who, counts.data(), (uint32_t)counts.size(), 61, 45, 70, 4);
        const std::vector<uint32_t> want = {0, 0, 3, 3, 1236, 1243, 1243};
        CHECK(l.n_keys == 6 && l.first == want && l.total == 1243 && l.cells == 432);
        for (uint32_t k = 0; k < l.n_keys; k++) CHECK(l.count(k) == counts[k]);
        CHECK(l.brick_bytes == 512u * 1243u && l.index_bytes == 4u * 6u * 432u && l.held_bytes() == 512u * 1243u + 4u * 6u * 432u);
    }
    {      // all keys empty: only the indices are held
        const std::vector<uint32_t> counts = {0, 0};
        const KeyBrickLayout l = key_brick_layout(who, counts.data(), 2, 16, 16, 16);
        CHECK(l.total == 0 && l.brick_bytes == 0 && l.held_bytes() == 4u * 2u * 8u);
    }
    // NULL counts with keys
    CHECK(has(error_of([&] { key_brick_layout(who, nullptr, 3, 8, 8, 8); }), "SkyRenderer ERROR: set_volume_key_bricks: key_counts is NULL (3 keys)"));
    // brick numbers: 1 + index has to fit 32 bits -- 2^32 - 2 bricks are the most, and the message names the key that crosses
    {
        const std::vector<uint32_t> most = {0x7fffffffu, 0x7fffffffu}, over = {0x7fffffffu, 0x7fffffffu, 1u}, one = {0xffffffffu};
        if (sizeof(size_t) >= 8) {
            const KeyBrickLayout l = key_brick_layout(who, most.data(), 2, 8, 8, 8, 4);
            CHECK(l.total == 0xfffffffeu && l.brick_bytes == (size_t)0xfffffffeu * 512u);
        }
        const std::string e = error_of([&] { key_brick_layout(who, over.data(), 3, 8, 8, 8); });
        CHECK(has(e, "the keys up to key 2 hold 4294967295 bricks"));
        CHECK(has(error_of([&] { key_brick_layout(who, one.data(), 1, 8, 8, 8); }), "the keys up to key 0"));
        const std::vector<uint32_t> wrap(5, 0xf0000000u);      // a 32-bit sum would wrap to a small number
        CHECK(has(error_of([&] { key_brick_layout(who, wrap.data(), 5, 8, 8, 8); }), "the keys up to key 1"));
    }
    // sizes past the address space
    {
        const size_t big = std::numeric_limits<size_t>::max();
        CHECK(checked_mul(0, big, who, "x") == 0 && checked_mul(big, 1, who, "x") == big && checked_mul(big / 2, 2, who, "x") == big - 1);
        CHECK(has(error_of([&] { checked_mul(big / 2 + 1, 2, who, "a size"); }), "set_volume_key_bricks: a size does not fit the address space"));
        CHECK(checked_add(big - 5, 5, who, "x") == big);
        CHECK(has(error_of([&] { checked_add(big - 5, 6, who, "a sum"); }), "a sum does not fit the address space"));
        const std::vector<uint32_t> counts = {0xfffffffeu};
        // an element size that pushes the source past a size_t
        CHECK(has(error_of([&] { key_brick_layout(who, counts.data(), 1, 8, 8, 8, big / 1024); }), "the source bricks' size does not fit"));
        // the keys' indices: 2^21 cells an axis, 2^63 cells, 4 bytes each
        const std::vector<uint32_t> none = {0, 0, 0, 0};
        CHECK(has(error_of([&] { key_brick_layout(who, none.data(), 4, 0xfffffff8u, 0xfffffff8u, 0xfffffff8u); }), "does not fit the address space"));
    }

    // host origins: every key's slice, the message names the key and the brick inside it
    {
        const uint32_t nx = 61, ny = 45, nz = 70;
        const std::vector<uint32_t> counts = {2, 0, 3};
        const KeyBrickLayout l = key_brick_layout(who, counts.data(), 3, nx, ny, nz);
        const std::vector<int32_t> good = {0, 0, 0, 56, 40, 64, 8, 8, 8, 8, 8, 8, 56, 0, 0};      // (a repeated origin is legal)
        {
            std::vector<int32_t> o(good);
            CHECK(error_of([&] { check_key_brick_origins(who, l, o.data(), nx, ny, nz); }).empty());
        }
        struct Bad { int at; int32_t v; const char* names; };
        const Bad bad[] = {{0, -8, "key 0, brick 0 has origin (-8, 0, 0)"}, {4, 48, "key 0, brick 1 has origin (56, 48, 64)"},
                           {5, 72, "key 0, brick 1 has origin (56, 40, 72)"}, {6, 4, "key 2, brick 0 has origin (4, 8, 8)"},
                           {12, 64, "key 2, brick 2 has origin (64, 0, 0)"}, {14, std::numeric_limits<int32_t>::min(), "key 2, brick 2"},
                           {10, std::numeric_limits<int32_t>::max(), "key 2, brick 1"}, {9, 1, "key 2, brick 1 has origin (1, 8, 8)"}};
        for (const Bad& b : bad) {
            std::vector<int32_t> o(good);
            o[b.at] = b.v;
            const std::string e = error_of([&] { check_key_brick_origins(who, l, o.data(), nx, ny, nz); });
            CHECK(has(e, b.names) && has(e, "multiple of 8 inside the renderer's 61x45x70 volume") && has(e, "SkyRenderer ERROR: set_volume_key_bricks"));
            if (!has(e, b.names)) std::printf("  got: %s\n", e.c_str());
        }
        {      // the first bad one is named
            std::vector<int32_t> o(good);
            o[3] = 3; o[13] = -1;
            CHECK(has(error_of([&] { check_key_brick_origins(who, l, o.data(), nx, ny, nz); }), "key 0, brick 1 has origin (3, 40, 64)"));
        }
        const int32_t edge[3] = {56, 40, 64}, past[3] = {64, 40, 64}, neg[3] = {0, -8, 0}, odd[3] = {0, 0, 12};
        CHECK(brick_origin_valid(edge, nx, ny, nz) && !brick_origin_valid(past, nx, ny, nz) && !brick_origin_valid(neg, nx, ny, nz) &&
              !brick_origin_valid(odd, nx, ny, nz));
        // no bricks at all: the origins are not looked at
        const std::vector<uint32_t> zeros = {0, 0};
        const KeyBrickLayout lz = key_brick_layout(who, zeros.data(), 2, nx, ny, nz);
        CHECK(error_of([&] { check_key_brick_origins(who, lz, nullptr, nx, ny, nz); }).empty());
    }

    // staging pieces: at least one brick, never more than there are, and they cover the list
    CHECK(key_brick_piece(1233, 64 * 64 * 64 * 4, 4) == 512 && key_brick_piece(100, 64 * 64 * 64 * 4, 4) == 100 && key_brick_piece(7, 1, 4) == 1);
    CHECK(key_brick_piece(0, 4096, 4) == 0);
    for (uint32_t total : {1u, 5u, 512u, 513u, 1233u})
        for (size_t budget : {(size_t)1, (size_t)2048, (size_t)5000, (size_t)1 << 20}) {
            const uint32_t piece = key_brick_piece(total, budget, 4);
            uint32_t covered = 0;
            for (uint32_t i = 0; i < total; i += piece) covered += (piece < total - i ? piece : total - i);
            CHECK(piece >= 1 && piece <= total && covered == total && ((size_t)piece * 2048 <= budget || piece == 1));
        }

    std::printf("volume_key_bricks: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
