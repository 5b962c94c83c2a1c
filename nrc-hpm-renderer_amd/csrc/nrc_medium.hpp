// nrc_medium.hpp -- the host layer of a renderer's medium: the scene as it is uploaded at creation (SceneDev) and everything that changes
// the density volume of a live renderer afterwards (Medium: the slots volumes are rebuilt into, the staging buffer of host sources, the key
// sequences and what a slot holds of them).  HIP host code, included by nrc_api.hip only; the kernels are nrc_integrator.hip's
// (launch_volume_*), the device-free arithmetic is nrc_occupancy.hpp's, nrc_volume_keys.hpp's and nrc_volume_key_bricks.hpp's.
// Both renderers hold one Medium and drive it through the same entry points (MediumHost, nrc_api.hip).  A renderer decides WHEN a slot may be
// written -- its streams, events and waits -- and this file decides WHICH slot, and does the write on the stream it is handed.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "nrc_integrator.hpp"
#include "nrc_occupancy.hpp"
#include "nrc_volume_key_bricks.hpp"
#include "nrc_volume_keys.hpp"

namespace nrc {

// ---------------------------------------------------------------------------------------------------- scene upload
// the world size of a scene's box: the caller's, or for an all-zero size the reference's default
inline void scene_world_size(const nrc_scene& s, float size[3])
{
    for (int k = 0; k < 3; k++) size[k] = s.size[k];
    if (size[0] == 0.0f && size[1] == 0.0f && size[2] == 0.0f) {
        // volumeSizeF = normalize(extent) * 107.5 (src/NrcHpmRenderer.cu:910-912)
        const float fnx = (float)s.nx, fny = (float)s.ny, fnz = (float)s.nz;
        const float l = sqrtf((fnx * fnx + fny * fny) + fnz * fnz);
        size[0] = fnx / l * 107.5f; size[1] = fny / l * 107.5f; size[2] = fnz / l * 107.5f;
    }
}
struct SceneDev {
    DevScene d{};
    DevBuf<uint8_t> d_density;
    DevBuf<float> d_env;
    DevBuf<float> d_boxes;        // occupancy boxes for the empty-space tile mask (launch_tile_mask)
    uint32_t n_boxes = 0;
    DevBuf<uint32_t> d_occ_bits;  // exact occupancy bits (DevScene::occ_bits)

    // (the host-side builders are nrc_occupancy.hpp's; what they return is uploaded here)
    void build_occupancy_bits(const nrc_scene& s)
    {
        d.occ_bits = nullptr;
        d.occ_shift = d.occ_gx = d.occ_gy = d.occ_words = 0;
        const OccupancyBits o = nrc::build_occupancy_bits(s.density, s.nx, s.ny, s.nz, kOccMaxWords);
        d_occ_bits.alloc(o.bits.size() * 4, "d_occ_bits");
        NRC_HIP(hipMemcpy(d_occ_bits, o.bits.data(), o.bits.size() * 4, hipMemcpyHostToDevice));
        d.occ_bits = d_occ_bits;
        d.occ_shift = o.shift; d.occ_gx = o.gx; d.occ_gy = o.gy; d.occ_words = (uint32_t)o.bits.size();
        occ_gz = o.gz;
    }
    uint32_t occ_gz = 0;

    void build_occupancy(const nrc_scene& s)
    {
        const std::vector<float> boxes = build_occupancy_boxes(s.density, s.nx, s.ny, s.nz, d.size);
        n_boxes = (uint32_t)(boxes.size() / 6);
        if (n_boxes) {
            d_boxes.alloc(boxes.size() * 4, "d_boxes");
            NRC_HIP(hipMemcpy(d_boxes, boxes.data(), boxes.size() * 4, hipMemcpyHostToDevice));
        }
    }

    void upload(const nrc_scene& s)
    {
        if (!s.density || s.nx == 0 || s.ny == 0 || s.nz == 0) fail("scene has no density volume");
        if (!(s.density_factor > 0.0f)) fail("scene density factor must be positive");
        check_volume_size(s.nx, s.ny, s.nz);
        const size_t nvox = (size_t)s.nx * s.ny * s.nz;
        d_density.alloc(nvox, "d_density");
        NRC_HIP(hipMemcpy(d_density, s.density, nvox, hipMemcpyHostToDevice));
        d.density = d_density;
        d.nx = s.nx; d.ny = s.ny; d.nz = s.nz;
        d.fnx = (float)s.nx; d.fny = (float)s.ny; d.fnz = (float)s.nz;
        float size[3];
        scene_world_size(s, size);
        for (int k = 0; k < 3; k++) {
            d.size[k] = size[k];
            d.half_size[k] = size[k] * 0.5f;
            d.inv_size[k] = 1.0f / size[k];
        }
        const float tx = 2.0f * size[0], ty = 2.0f * size[1], tz = 2.0f * size[2];
        // length(2 * skySize) with the math spec's dot product (a chain of single-rounding FMAs, nrc_math.h) -- what the oracle and
        // the device code compute; a plain (x*x + y*y) + z*z can differ in the last bit and with it every exit point
        d.len2size = sqrtf(fmaf(tz, tz, fmaf(ty, ty, tx * tx)));
        build_occupancy(s);
        build_occupancy_bits(s);
        set_params(s);
        d.env = nullptr; d.env_w = d.env_h = 0;
        if (s.env && s.env_w && s.env_h) {
            const size_t eb = (size_t)s.env_w * s.env_h * 16;
            d_env.alloc(eb, "d_env");
            NRC_HIP(hipMemcpy(d_env, s.env, eb, hipMemcpyHostToDevice));
            d.env = d_env; d.env_w = s.env_w; d.env_h = s.env_h;
        }
    }
    // the uniform-buffer part of the scene (DirLight / PointLight / VolumeData / HdrEnvMap UBOs: src/DirLight.cpp:31-49,
    // src/HpmScene.cpp:56-76): kernels take DevScene by value, so the next launch sees the new values
    void set_params(const nrc_scene& s)
    {
        if (!(s.density_factor > 0.0f)) fail("scene density factor must be positive");
        d.density_factor = s.density_factor;
        d.inv_max_density = 1.0f / s.density_factor;
        d.g = s.g;
        for (int k = 0; k < 3; k++) {
            d.dir_light_dir[k] = s.dir_light_dir[k];
            d.point_light_pos[k] = s.point_light_pos[k];
            d.point_light_color[k] = s.point_light_color[k];
        }
        d.dir_light_strength = s.dir_light_strength;
        d.point_light_strength = s.point_light_strength;
        d.env_strength = s.env_strength;
    }
};

// ---------------------------------------------------------------------------------------------------- the live medium
// what every entry point that takes a `format` checks; who: the entry point's name in the error text
inline void check_format(const std::string& who, int format)
{
    if (format != NRC_VOLUME_U8 && format != NRC_VOLUME_F32) fail(who + ": format must be NRC_VOLUME_U8 or NRC_VOLUME_F32");
}
inline size_t format_bytes(int format) { return format == NRC_VOLUME_F32 ? 4 : 1; }
// what every entry point that takes a non-empty brick list checks; n: the bricks of the whole list
inline void check_brick_pointers(const std::string& who, const int32_t* origins, const void* bricks, uint32_t n)
{
    if (!origins) fail(who + ": origins is NULL (" + std::to_string(n) + " bricks)");
    if (!bricks) fail(who + ": bricks is NULL (" + std::to_string(n) + " bricks)");
}

struct Medium : SceneDev {
    // ---- nrc_renderer_set_volume: volumes rebuilt on the device (launch_volume_rebuild) go into slots allocated on first use (a renderer
    // that never swaps keeps the memory it had); active < 0: the creation-time buffers of SceneDev.  The caller orders the writes (Renderer:
    // two slots, the one frames do not read is written; McRenderer: one, in stream order).
    struct Slot { DevBuf<uint8_t> density; DevBuf<uint32_t> occ_bits; DevBuf<float> boxes; DevBuf<uint32_t> n_boxes; };
    Slot slot[2];
    int active = -1;
    DevBuf<void> d_vol_scratch;         // launch_volume_rebuild's per-cell scratch
    DevBuf<char> d_stage;               // a host source's copy
    size_t stage_bytes = 0;

    size_t voxels() const { return (size_t)d.nx * d.ny * d.nz; }

    // what set_volume and set_volume_keys check alike; subject: "the volume is" / "the keys are" (the error texts differ there)
    void check_dims_format(const std::string& who, uint32_t nx, uint32_t ny, uint32_t nz, int format, const char* subject) const
    {
        check_format(who, format);
        if (nx != d.nx || ny != d.ny || nz != d.nz)
            fail(who + ": " + subject + " " + std::to_string(nx) + "x" + std::to_string(ny) + "x" +
                 std::to_string(nz) + ", the renderer's " + std::to_string(d.nx) + "x" + std::to_string(d.ny) + "x" + std::to_string(d.nz) +
                 " (dims are fixed at creation)");
    }
    // throws (renderer unchanged) unless the call can be carried out
    void check_volume(const void* src, uint32_t nx, uint32_t ny, uint32_t nz, int format) const
    {
        if (!src) fail("set_volume: density is NULL");
        check_dims_format("set_volume", nx, ny, nz, format, "the volume is");
    }
    // The slot the next volume is built into, for a renderer that keeps n_slots (2 or 1) of them: of two the one frames do not read, of
    // one that one.  The first call allocates the slots and the rebuild scratch.  The renderer then waits for the slot's last readers (its
    // business: two slots need events, one slot is ordered by its stream), has the slot written, and calls activate().
    int begin_write(int n_slots)
    {
        for (int k = 0; k < n_slots; k++) {
            Slot& sl = slot[k];
            if (sl.density) continue;
            sl.density.alloc(voxels(), "volume slot density");
            sl.occ_bits.alloc((size_t)d.occ_words * 4, "volume slot occupancy bits");
            sl.boxes.alloc((size_t)volume_box_capacity(d.nx, d.ny, d.nz) * 24 + 4, "volume slot boxes");
            sl.n_boxes.alloc(4, "volume slot box count");
        }
        if (!d_vol_scratch) d_vol_scratch.alloc(volume_scratch_bytes(d.nx, d.ny, d.nz), "volume rebuild scratch");
        return n_slots == 2 && active == 0 ? 1 : 0;
    }
    // rebuilds slot k from src on stream s (a host source is copied first: blocks until the copy is done)
    void write_slot(int k, const void* src, int format, bool on_device, hipStream_t s)
    {
        const size_t bytes = voxels() * format_bytes(format);
        if (!on_device) {
            reserve_stage(bytes, s);
            src = stage_host(src, bytes, 0, s);
            NRC_HIP(hipStreamSynchronize(s));      // (the host buffer is the caller's again when the call returns)
        }
        launch_volume_rebuild(src, format, rebuild_of(k), d_vol_scratch, s);
        key_state_known = false;
    }
    // the staging buffer holds at least `bytes` (it only grows; the rebuild reading the old one on s is waited for before it is freed)
    void reserve_stage(size_t bytes, hipStream_t s)
    {
        if (stage_bytes >= bytes) return;
        if (d_stage) NRC_HIP(hipStreamSynchronize(s));
        stage_bytes = 0;
        d_stage.alloc(bytes, "volume staging");
        stage_bytes = bytes;
    }
    // src -> the staging buffer at `offset`, enqueued on s (reserve_stage has made the room; the caller waits); returns where it went
    const void* stage_host(const void* src, size_t bytes, size_t offset, hipStream_t s)
    {
        NRC_HIP(hipMemcpyAsync(d_stage + offset, src, bytes, hipMemcpyHostToDevice, s));
        return d_stage + offset;
    }
    VolumeRebuild rebuild_of(int k) const
    {
        const Slot& sl = slot[k];
        VolumeRebuild v{};
        v.density = sl.density; v.occ_bits = sl.occ_bits; v.boxes = sl.boxes; v.n_boxes = sl.n_boxes;
        v.nx = d.nx; v.ny = d.ny; v.nz = d.nz;
        v.occ_shift = d.occ_shift; v.occ_gx = d.occ_gx; v.occ_gy = d.occ_gy; v.occ_gz = occ_gz; v.occ_words = d.occ_words;
        const uint32_t n[3] = {d.nx, d.ny, d.nz};
        for (int a = 0; a < 3; a++) {      // build_occupancy's world(): -0.5 * size + (size / n) * voxel in fp64
            v.lo[a] = -0.5 * (double)d.size[a];
            v.vs[a] = (double)d.size[a] / n[a];
        }
        return v;
    }

    // ---- nrc_renderer_set_volume_bricks: the same slots, rebuilt from a list of 8^3 bricks (launch_volume_rebuild_bricks)
    DevBuf<uint32_t> d_brick_index;     // one word per 8^3 cell, allocated by the first brick call

    // throws (renderer unchanged) unless the call can be carried out; a device list's origins are the kernel's to check
    void check_bricks(const int32_t* origins, const void* bricks, uint32_t n, int format, bool on_device) const
    {
        const std::string who = "set_volume_bricks";
        check_format(who, format);
        if (n == 0) return;
        check_brick_pointers(who, origins, bricks, n);
        if (on_device) return;
        for (uint32_t i = 0; i < n; i++) {
            const int32_t* o = origins + 3 * (size_t)i;
            if (!brick_origin_valid(o, d.nx, d.ny, d.nz))
                fail(who + ": brick " + std::to_string(i) + " has origin (" + std::to_string(o[0]) + ", " + std::to_string(o[1]) + ", " +
                     std::to_string(o[2]) + "): every component must be a multiple of 8 inside the renderer's " + std::to_string(d.nx) + "x" +
                     std::to_string(d.ny) + "x" + std::to_string(d.nz) + " volume");
        }
    }
    // rebuilds slot k from the list on stream s (a host list is copied first, bricks then origins: blocks until the copy is done)
    void write_slot_bricks(int k, const int32_t* origins, const void* bricks, uint32_t n, int format, bool on_device, hipStream_t s)
    {
        if (!d_brick_index) d_brick_index.alloc(volume_brick_index_bytes(d.nx, d.ny, d.nz), "volume brick index");
        if (!on_device && n) {
            const size_t brick_bytes = (size_t)n * kBrickVoxels * format_bytes(format), origin_bytes = (size_t)n * 12;
            reserve_stage(brick_bytes + origin_bytes, s);
            bricks = stage_host(bricks, brick_bytes, 0, s);
            origins = (const int32_t*)stage_host(origins, origin_bytes, brick_bytes, s);
            NRC_HIP(hipStreamSynchronize(s));      // (the host buffers are the caller's again when the call returns)
        }
        launch_volume_rebuild_bricks(origins, bricks, n, format, rebuild_of(k), d_vol_scratch, d_brick_index, s);
        key_state_known = false;
    }

    // ---- key sequences.  One sequence, dense or bricks: setting either kind replaces whatever was there.  Both kinds are library-owned R8
    // (an F32 source is quantised once, by to_r8), and the slots are rebuilt from two keys and a weight.  key_state: the (key, weight) the
    // sequence last put into a slot, unknown after any other slot write.
    uint32_t n_keys = 0;
    bool key_state_known = false;
    KeyTime key_state{};
    // nrc_renderer_set_volume_keys: n_keys volumes of the creation dims in one [n_keys][nz][ny][nx] allocation (launch_volume_rebuild_lerp)
    DevBuf<uint8_t> d_keys;
    // nrc_renderer_set_volume_key_bricks: one array of every key's 8^3 bricks in key order and, per key, a resident cell_brick index into it
    // (one word per 8^3 cell: 1 + the brick's number in that array, 0 = none) -- the origins are not kept.  The device-free part is
    // nrc_volume_key_bricks.hpp.
    DevBuf<uint8_t> d_key_bricks;       // (absent when no key has a brick)
    DevBuf<uint32_t> d_key_cells;       // [n_keys][cells]; present: the sequence is of this kind
    KeyBrickLayout key_layout;
    bool keys_are_bricks() const { return (bool)d_key_cells; }
    // nrc_renderer_volume_key_bytes
    size_t key_bytes() const { return keys_are_bricks() ? key_layout.held_bytes() : dense_key_bytes(n_keys, d.nx, d.ny, d.nz); }

    // `count` source elements at src -> R8 at dst, enqueued on s: U8 is copied, F32 quantised on the device.  A host F32 source goes
    // through the staging buffer `piece` elements at a time (the buffer holds about one F32 volume, as for set_volume).  The caller waits
    // for s before a host source's call returns.
    void to_r8(uint8_t* dst, const void* src, size_t count, size_t piece, int format, bool on_device, hipStream_t s)
    {
        if (format == NRC_VOLUME_U8)
            NRC_HIP(hipMemcpyAsync(dst, src, count, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        else if (on_device)
            launch_volume_quantize((const float*)src, dst, count, s);
        else {
            reserve_stage(piece * 4, s);
            for (size_t i = 0; i < count; i += piece) {
                const size_t n = std::min(piece, count - i);
                const void* staged = stage_host((const float*)src + i, n * 4, 0, s);
                launch_volume_quantize((const float*)staged, dst + i, n, s);
            }
        }
    }
    // throws (renderer and keys unchanged) unless the call can be carried out
    void check_keys(const void* src, uint32_t n, uint32_t nx, uint32_t ny, uint32_t nz, int format) const
    {
        if (n == 0) return;      // (drops the sequence: nothing else is looked at)
        if (!src) fail("set_volume_keys: volumes is NULL (" + std::to_string(n) + " keys)");
        check_dims_format("set_volume_keys", nx, ny, nz, format, "the keys are");
    }
    // replaces the sequence; the copies and the quantisation run on s (a host source: blocks until they are done).  The caller has waited
    // for every stream that may still read the old keys.  The new keys are complete before the old ones go: a failure leaves those.
    void set_keys(const void* src, uint32_t n, int format, bool on_device, hipStream_t s)
    {
        DevBuf<uint8_t> fresh;
        if (n) {
            fresh.alloc((size_t)n * voxels(), "volume keys");
            to_r8(fresh, src, (size_t)n * voxels(), voxels(), format, on_device, s);      // (a host F32 source: key by key)
            if (!on_device) NRC_HIP(hipStreamSynchronize(s));      // (the host buffer is the caller's again when the call returns)
        }
        d_keys = std::move(fresh);
        d_key_bricks.reset();
        d_key_cells.reset();
        key_layout = KeyBrickLayout{};
        n_keys = n;
        key_state_known = false;
    }
    // throws (renderer and keys unchanged) unless the call can be carried out; a device list's origins are the kernel's to check
    KeyBrickLayout check_key_bricks(const uint32_t* counts, const int32_t* origins, const void* bricks, uint32_t n, int format, bool on_device) const
    {
        const std::string who = "set_volume_key_bricks";
        if (n == 0) return key_brick_layout(who, nullptr, 0, d.nx, d.ny, d.nz);      // (drops the sequence: nothing else is looked at)
        check_format(who, format);
        KeyBrickLayout l = key_brick_layout(who, counts, n, d.nx, d.ny, d.nz, format_bytes(format));
        if (l.total == 0) return l;
        check_brick_pointers(who, origins, bricks, l.total);
        if (!on_device) check_key_brick_origins(who, l, origins, d.nx, d.ny, d.nz);
        return l;
    }
    // replaces the sequence, as set_keys does: copies, quantisation and the keys' indices run on s (a host source: blocks until they are
    // done), the caller has waited for every stream that may still read the old keys, and the new ones are complete before the old ones go
    void set_key_bricks(const KeyBrickLayout& l, const int32_t* origins, const void* bricks, int format, bool on_device, hipStream_t s)
    {
        DevBuf<uint8_t> fresh;
        DevBuf<uint32_t> fresh_cells;
        DevBuf<int32_t> host_origins;      // a host list's origins on the device, until the indices are built
        if (l.n_keys) {
            fresh_cells.alloc(l.index_bytes, "volume key brick indices");
            if (l.total) {
                fresh.alloc(l.brick_bytes, "volume key bricks");
                to_r8(fresh, bricks, l.brick_bytes, (size_t)key_brick_piece(l.total, voxels() * 4, 4) * kBrickVoxels, format, on_device, s);
                if (!on_device) {
                    host_origins.alloc((size_t)l.total * 12, "volume key brick origins");
                    NRC_HIP(hipMemcpyAsync(host_origins, origins, (size_t)l.total * 12, hipMemcpyHostToDevice, s));
                    origins = host_origins;
                }
            }
            for (uint32_t k = 0; k < l.n_keys; k++)
                launch_volume_brick_index(l.count(k) ? origins + 3 * (size_t)l.first[k] : nullptr, l.count(k), l.first[k], fresh_cells + (size_t)k * l.cells,
                                          d.nx, d.ny, d.nz, s);
            if (!on_device) NRC_HIP(hipStreamSynchronize(s));      // (the host buffers are the caller's again when the call returns)
        }
        d_key_bricks = std::move(fresh);
        d_key_cells = std::move(fresh_cells);
        d_keys.reset();
        key_layout = l;
        n_keys = l.n_keys;
        key_state_known = false;
    }
    // the key pair and weight of time t (nrc_volume_keys.hpp), with the end of an interval named as the next key itself: (i, 256) and
    // (i + 1, 0) are the same volume.  Throws unless t is finite and inside [0, n_keys - 1].
    KeyTime key_time(float t, const char* who) const
    {
        if (n_keys == 0) fail(std::string(who) + ": the renderer holds no volume keys (set_volume_keys / set_volume_key_bricks)");
        KeyTime kt;
        if (!key_of_time(t, n_keys, &kt))
            fail(std::string(who) + ": time " + std::to_string(t) + " is not inside [0, " + std::to_string(n_keys - 1) + "] (" + std::to_string(n_keys) + " keys)");
        if (kt.w == 256u) { kt.i++; kt.w = 0u; }
        return kt;
    }
    bool holds_key(const KeyTime& kt) const { return key_state_known && key_state.i == kt.i && key_state.w == kt.w; }
    // rebuilds slot k as the in-between volume of kt on stream s (nrc_renderer_set_volume_time: never materialised outside the slot)
    void write_slot_lerp(int k, const KeyTime& kt, hipStream_t s)
    {
        if (keys_are_bricks()) {
            const uint32_t* a = d_key_cells + (size_t)kt.i * key_layout.cells;
            launch_volume_rebuild_lerp_bricks(d_key_bricks, a, kt.w ? a + key_layout.cells : nullptr, kt.w, rebuild_of(k), d_vol_scratch, s);
        } else {
            const uint8_t* a = d_keys + (size_t)kt.i * voxels();
            launch_volume_rebuild_lerp(a, kt.w ? a + voxels() : nullptr, kt.w, rebuild_of(k), d_vol_scratch, s);
        }
        key_state = kt;
        key_state_known = true;
    }
    // slot k is the volume the frames enqueued from now on read (kernels take DevScene by value)
    void activate(int k)
    {
        active = k;
        d.density = slot[k].density;
        d.occ_bits = slot[k].occ_bits;
    }

    // ---- the active volume's boxes: creation's (count on the host), or a rebuilt slot's (count in device memory, the launches cover the capacity)
    BoxList box_list() const
    {
        if (active < 0) return {d_boxes, n_boxes, nullptr, n_boxes};
        return {slot[active].boxes, 0u, slot[active].n_boxes, volume_box_capacity(d.nx, d.ny, d.nz)};
    }
    // the empty-space tile mask from them
    void launch_mask(const DevProjView& pv, const DevFrame& fr, uint32_t* mask, float* far, hipStream_t s) const { launch_tile_mask(box_list(), pv, fr, mask, far, s); }
    // the same words from the tile-parallel build (launch_tile_mask_tiles; render_path's views)
    DevBuf<void> d_rects;         // its scratch: a packed rectangle per box, allocated by the first camera path
    void ensure_rects()
    {
        if (d_rects) return;
        const size_t n = std::max<size_t>(std::max(n_boxes, volume_box_capacity(d.nx, d.ny, d.nz)), 1);
        d_rects.alloc(n * 8, "tile mask rectangles");
    }
    void launch_mask_tiles(const DevProjView& pv, const DevFrame& fr, uint32_t* mask, float* far, hipStream_t s) const
    {
        launch_tile_mask_tiles(box_list(), pv, fr, d_rects, mask, far, s);
    }
    // nrc_renderer_volume_buffer (the caller has synchronised): 0 density, 1 occupancy bits, 2 boxes
    const void* buffer(int which, size_t* bytes) const
    {
        size_t b = 0;
        const void* p = nullptr;
        if (which == 0) { p = d.density; b = voxels(); }
        else if (which == 1) { p = d.occ_bits; b = (size_t)d.occ_words * 4; }
        else if (which == 2) {
            uint32_t n = n_boxes;
            if (active >= 0) NRC_HIP(hipMemcpy(&n, slot[active].n_boxes, 4, hipMemcpyDeviceToHost));
            p = n ? (active < 0 ? d_boxes : slot[active].boxes) : nullptr;
            b = (size_t)n * 24;
        } else fail("volume_buffer: which must be 0 (density), 1 (occupancy bits) or 2 (boxes)");
        if (bytes) *bytes = b;
        return p;
    }
};

}  // namespace nrc
