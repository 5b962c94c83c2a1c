// nrc_integrator.hpp -- volumetric path integrator kernels (host launch interface).
// HIP restatement of data/shader/nrc/{clear,gen_rays,prep_infer_rays,prep_train_rays,render}.comp,
// data/shader/mc/render.comp and data/shader/include/{random,volume,dir_gen,path_trace}.glsl.
#pragma once
#include "nrc_common.hpp"
#include "nrc_denoise.hpp"
#include "nrc_hot_tiles.hpp"
#include "nrc_reproject.hpp"
#include "nrc_view_aov.hpp"

namespace nrc {

// device-resident scene constants (specialization constants + UBOs of the reference: nrc-constants.glsl:18-26,
// nrc-descriptors.glsl:13-38)
struct DevScene {
    const uint8_t* density;       // R8, index i + nx*(j + ny*k)
    uint32_t nx, ny, nz;
    float fnx, fny, fnz;
    float size[3], half_size[3], inv_size[3];
    float len2size;               // length(2*skySize)
    float density_factor, inv_max_density, g;
    float dir_light_dir[3], dir_light_strength;
    float point_light_pos[3], point_light_strength, point_light_color[3];
    const float* env;             // RGBA32F
    uint32_t env_w, env_h;
    float env_strength;
    // exact occupancy of the volume, one bit per cell of (1 << occ_shift)^3 voxels (set: the cell holds a non-zero voxel), cell index
    // (cz * occ_gy + cy) * occ_gx + cx; at most kOccMaxWords words, copied into LDS by every kernel that samples the volume.
    // nullptr: no occupancy information (every look-up goes to memory)
    const uint32_t* occ_bits;
    uint32_t occ_shift, occ_gx, occ_gy, occ_words;
};
constexpr uint32_t kOccMaxWords = 2048;      // 65 536 cells = 8 KB of LDS

struct DevCamera {
    float m[16];                  // invProjView, column-major
    float pos[3];
};

struct DevFrame {
    float random[4];              // UniformData.random
    uint32_t w, h;                // local image: w columns x h rows
    uint32_t x_offset, x_stride;  // global x = ((x_offset + (lx >> x_block_log2) * x_stride) << x_block_log2) + (lx & block - 1)
    uint32_t x_block_log2;        // log2 of the strip width (nrc_tile::x_block)
    float inv_gw, inv_gh;         // 1/global width, 1/global height (ONE_OVER_RENDER_WIDTH/HEIGHT)
    // one bit per 8x8 pixel tile (index ty * ceil(w/8) + tx), set when a camera ray of the tile can meet a non-empty voxel; the
    // word behind the last tile word is non-zero when the mask must be ignored.  nullptr: no mask (every tile is traced).
    const uint32_t* tile_mask;
    // the far cut, built with the mask: one float per tile, an upper bound of the distance from the camera position
    // to the farthest point of any mask box whose rectangle touches the tile (0: none does).  Behind it a camera ray of the tile is in
    // empty space for good.  nullptr: no cut.
    const float* tile_far;
    // the mask may only be applied to a pixel whose delta walk through empty space provably leaves the volume before DeltaTrack's
    // cap of 128 collisions -- a property of the pixel's RNG state (2^23 of them) and of the scene's largest optical depth.  The
    // states that can reach the cap ("capped") are handed over as a list when there are at most kFlightListMax of them (one state,
    // the chain's fixed point 0, for the bench scene), otherwise as a bit per state (flight_bits, 1 MB, bit set = capped).
    // flight_mode: 0 the mask is not applied, 1 list, 2 bits.
    uint32_t flight_mode, flight_n;
    uint32_t flight_list[8];
    const uint32_t* flight_bits;
    // launch order of the camera kernels' 8x8 tiles: launch slot (workgroup * 4 + wave) -> default slot (the centre-out order of
    // pixel_of_wave_tile), costliest first (k_tile_order); nullptr: default order.  tile_cost: cycles each default slot's wave
    // took in this launch (written by k_gen_rays when non-null)
    const uint32_t* tile_order;
    uint32_t* tile_cost;
    // 0: tile_cost[slot] = this launch's cycles; k > 0: max(this launch's cycles, old - (old >> k)) -- a decaying maximum over the
    // sampled launches: the costliest-first order is hurt by tiles it under-estimates (a long tile started late ends the launch),
    // not by tiles it over-estimates
    uint32_t tile_cost_keep;
    // Tiles the camera kernels start FIRST, whatever the order says: hot_front != 0 gives the launch kHotTilesMax waves in front of the
    // ordered ones, and wave k < hot_n of them traces tile hot[k] (ty << 16 | tx).  A pixel in a capped RNG state (see flight_mode) in a
    // tile the mask rejects is one lane that walks for ~120 us; its wave would otherwise start among the empty tiles at the end of the
    // launch and end it that much later (one frame in four on the bench view).  The host finds those pixels when it enqueues the frame
    // (HotTileFinder, nrc_hot_tiles.hpp) and the list travels here by value.  Scheduling only: every tile is traced exactly once with
    // or without the list.
    uint32_t hot_front, hot_n;
    uint32_t hot[8];
    // the frame's LIVE queries (pixels that scattered: 22 % on the bench view): k_gen_rays appends their query indices to live_list
    // and counts them in *live_count (zeroed by the caller in front of the launch); nullptr: no list.  The order of the
    // list is whatever the waves' atomics made it; its only reader (the HashGrid encoder, Mlp::launch_features) writes by query index.
    uint32_t* live_list;
    uint32_t* live_count;
    // nrc_common.hpp's run-time priority switch as a kernel argument of the camera kernels (set by their launchers): their 32 400 waves
    // would each pay two dependent scalar loads for the device-side copy (0.7 % of a launch)
    uint32_t raise_priority;
    // set by the renderer, read by the launchers only: 1 = this renderer's camera kernels stay at the default wave priority although the
    // library raises (they then yield issue slots to the inference / training kernels beside them; Renderer::camera_priority_low_)
    uint32_t camera_priority_low;
    // the queries of pixels that did not scatter are not written (nobody reads them: the inference walks live_list and encodes inside its
    // kernel or from the list).  0: every slot of the query buffer is written, dead pixels with zeros (the reference's zero-filled buffer)
    uint32_t skip_dead_queries;
};
constexpr uint32_t kOrderSlotMask = 0x00ffffffu;      // (most tiles a launch order can address)

// forward camera transform for the tile mask: clip = m * (x, y, z, 1), column-major like DevCamera::m
// eye: the camera position the far cut's distances are measured from; far_margin: what a box's farthest-corner distance is grown by
// (tile_far_bound)
struct DevProjView {
    float m[16];
    float eye[3];
    float far_margin;
    float far_piece;              // the length along x of the pieces a box is cut into for its far bounds (a cell's; > 0)
};

struct TrainGrid {
    uint32_t tw, th, x_dist, y_dist, spp, ray_length, ring_size;
};

// origin / dir (the NRC vertex images) are written at the train grid's pixels only unless full_vertex_images
void launch_gen_rays(const DevScene& sc, const DevCamera& cam, const DevFrame& fr, uint32_t primary_ray_length,
                     float primary_ray_prob, float* primary, float* info, float* origin, float* dir, float* infer_in,
                     unsigned long long* fetch_counter, const TrainGrid& tg, bool full_vertex_images, hipStream_t s);

// tile-major query order of the renderer's inference buffers (see query_index in nrc_integrator.hip) -> x * H + y
void launch_query_layout(const DevFrame& fr, uint32_t floats_per_query, const float* tiled, float* linear, hipStream_t s,
                         const float* info = nullptr);
uint32_t query_count(uint32_t w, uint32_t h);      // queries in tile-major order: whole 8x8 tiles
// marks the 8x8-pixel tiles whose camera rays can meet a non-empty voxel: `boxes` = n axis-aligned world-space boxes
// {lo.xyz, hi.xyz} that together cover every non-empty voxel with a margin of one voxel.  mask: ceil(tiles/32) + 1 words, zeroed here.
// The boxes of the active volume: n_host of them, or *n_dev (<= grid, the capacity) when the count lives in device memory, as
// launch_volume_rebuild leaves it (n_dev not null); grid: the boxes a launch has to cover, 0: none
// far: DevFrame::tile_far of the same boxes (one float per tile, zeroed here), by both builds
struct BoxList {
    const float* boxes;
    uint32_t n_host;
    const uint32_t* n_dev;
    uint32_t grid;
};
void launch_tile_mask(const BoxList& b, const DevProjView& pv, const DevFrame& fr, uint32_t* mask, float* far, hipStream_t s);
uint32_t tile_mask_words(uint32_t w, uint32_t h);
// the same words (the trailing "off" word included) from a build that runs in parallel over the mask instead of over the boxes, without
// atomics and without a clear of `mask` (nrc_renderer_render_path: one mask per view).  rects: 8 bytes per box (b.grid), scratch between
// the two launches.
void launch_tile_mask_tiles(const BoxList& b, const DevProjView& pv, const DevFrame& fr, void* rects, uint32_t* mask, float* far, hipStream_t s);

// ---- device-side volume rebuild (nrc_renderer_set_volume): from a density volume in device memory (NRC_VOLUME_U8 / NRC_VOLUME_F32,
// index i + nx*(j + ny*k)) the R8 density, the exact occupancy bits (DevScene::occ_bits) and the dilated 8^3-cell boxes of the tile mask,
// bit-identical to what renderer creation builds on the host.  The box count stays in device memory (BoxList::n_dev).
struct VolumeRebuild {
    uint8_t* density;             // nx*ny*nz bytes
    uint32_t* occ_bits;           // occ_words words
    float* boxes;                 // 6 * volume_box_capacity floats
    uint32_t* n_boxes;            // one word
    uint32_t nx, ny, nz;
    uint32_t occ_shift, occ_gx, occ_gy, occ_gz, occ_words;   // the table's geometry (a function of the dims: SceneDev::build_occupancy_bits)
    double lo[3], vs[3];          // -0.5 * size, size / n (build_occupancy's fp64 world coordinates)
};
uint32_t volume_box_capacity(uint32_t nx, uint32_t ny, uint32_t nz);
size_t volume_scratch_bytes(uint32_t nx, uint32_t ny, uint32_t nz);
// scratch: volume_scratch_bytes; src must stay unchanged until the launches on s have run.  Three launches.
void launch_volume_rebuild(const void* src, int format, const VolumeRebuild& v, void* scratch, hipStream_t s);
// the same from n_bricks 8^3 bricks in device memory (nrc_renderer_set_volume_bricks: origins int32[3 * n], bricks n * 512 elements of
// `format`): voxels no brick covers become 0, the highest index wins a cell named twice, an invalid origin is ignored.  brick_index:
// volume_brick_index_bytes (one word per 8^3 cell), scratch as above.  A clear and four launches (three when n_bricks == 0); the result is
// what launch_volume_rebuild makes of the densified list, bit for bit.
size_t volume_brick_index_bytes(uint32_t nx, uint32_t ny, uint32_t nz);
void launch_volume_rebuild_bricks(const int32_t* origins, const void* bricks, uint32_t n_bricks, int format, const VolumeRebuild& v, void* scratch,
                                  uint32_t* brick_index, hipStream_t s);
// the first half of that call alone: cell_brick (volume_brick_index_bytes) cleared, then cell_brick[cell] = 1 + first + the highest index of the
// n_bricks bricks at `origins` that name the cell (nrc_renderer_set_volume_key_bricks: a key's slice of the concatenated list, first = where it
// starts).  A clear and one launch (none when n_bricks == 0).
void launch_volume_brick_index(const int32_t* origins, uint32_t n_bricks, uint32_t first, uint32_t* cell_brick, uint32_t nx, uint32_t ny, uint32_t nz,
                               hipStream_t s);
// the second half from a ready index: R8 bricks aligned to 4 bytes, cell_brick as launch_volume_brick_index leaves it (neither is written).
// Three launches.
void launch_volume_rebuild_indexed(const uint8_t* bricks, const uint32_t* cell_brick, const VolumeRebuild& v, void* scratch, hipStream_t s);
// two keys of one such array blended (nrc_renderer_set_volume_time on brick keys): voxel = lerp_voxel(a, b, W) with 0 where a key has no brick
// in the cell, 0 <= W <= 256 -- what launch_volume_rebuild_lerp makes of the two densified keys, bit for bit.  W == 0 reads cell_a's key alone
// through launch_volume_rebuild_indexed (cell_b may be null), W == 256 cell_b's.  Three launches.
void launch_volume_rebuild_lerp_bricks(const uint8_t* bricks, const uint32_t* cell_a, const uint32_t* cell_b, uint32_t W, const VolumeRebuild& v,
                                       void* scratch, hipStream_t s);
// n NRC_VOLUME_F32 voxels -> R8, the quantisation of launch_volume_rebuild (key volumes are kept as R8: nrc_renderer_set_volume_keys)
void launch_volume_quantize(const float* src, uint8_t* dst, size_t n, hipStream_t s);
// the same from two R8 key volumes in device memory (nrc_renderer_set_volume_time): every voxel lerp_voxel(a, b, W) of nrc_volume_keys.hpp,
// 0 <= W <= 256 -- the result is what launch_volume_rebuild makes of that in-between volume, bit for bit.  W == 0 reads key_a alone (key_b
// may be null), W == 256 key_b alone.  Three launches; both keys must stay unchanged until they have run.
void launch_volume_rebuild_lerp(const uint8_t* key_a, const uint8_t* key_b, uint32_t W, const VolumeRebuild& v, void* scratch, hipStream_t s);
// table[m] = optical distance covered by the 128 free flights a delta walk draws from RNG state m when it rejects every collision
constexpr uint32_t kFlightStates = 1u << 23;
void launch_flight_table(float* table, hipStream_t s);
// the states whose table entry does not exceed lambda: count_and_list[0] = their number, [1..8] the first eight (any order);
// bits (kFlightStates / 32 words): bit m set for every such state
void launch_flight_select(const float* table, float lambda, uint32_t* count_and_list, uint32_t* bits, hipStream_t s);
// launch slots of the camera kernels (rows padded to an odd number of workgroups) and the costliest-first order over them
uint32_t camera_slots(uint32_t w, uint32_t h);
void launch_tile_order(const uint32_t* cost, uint32_t n_slots, uint32_t* order, uint32_t w, hipStream_t s, uint32_t xcd_window = 0, uint32_t workgroups_in_front = 0);

void launch_mc_render(const DevScene& sc, const DevCamera& cam, const DevFrame& fr, uint32_t path_length,
                      float blend_factor, float* out_rgba, float* info, unsigned long long* fetch_counter, hipStream_t s);

// the view AOV (nrc_view_aov.hpp): out [h][w][4] = {alpha, tau, z_front, z_half} of every pixel's camera ray through the scene's active
// volume; fr carries the view's geometry and, when it has one, the empty-space tile mask of the SAME camera and medium.  One launch.
void launch_view_aov(const DevScene& sc, const DevCamera& cam, const DevFrame& fr, float* out, hipStream_t s);
// the ray AOV (nrc_view_aov.hpp, view_aov_walk_range): the same four numbers of caller-supplied ray segments, one launch of k_ray_aov each.
// fr is the renderer's frame.  rays [n][8] = {ox, oy, oz, t_min, dx, dy, dz, t_max} -> out [n][4]; the frame's camera rays up to depth [h][w]
// (fr's geometry and tile mask, as for launch_view_aov; depth null: whole rays) -> out [h][w][4]; an orthographic view of w x h pixels ->
// out [h][w][4].  rays and out 16-byte aligned.
// deep: null, or the deep AOV (nrc_view_aov.hpp, deep_aov_walk_range) in the same launch -- the depths at which the rays reach the n_levels
// optical depths `levels` (host floats, already checked: deep_aov_levels_error) go to z [n_levels][rays] (planar), and out may then be null.
struct AovPlanes { uint32_t n_levels; const float* levels; float* z; };
void launch_ray_aov_list(const DevScene& sc, const DevFrame& fr, size_t n, const float* rays, float* out, const AovPlanes* deep, hipStream_t s);
void launch_ray_aov_view_depth(const DevScene& sc, const DevCamera& cam, const DevFrame& fr, const float* depth, float* out, const AovPlanes* deep, hipStream_t s);
void launch_ray_aov_ortho(const DevScene& sc, const DevFrame& fr, const AovOrthoView& view, uint32_t w, uint32_t h, float* out, const AovPlanes* deep, hipStream_t s);

// the denoise filter (nrc_denoise.hpp): rgba [h][w][4] filtered with the guide aov [h][w][4] -> out [h][w][4], all device memory, 16-byte aligned.
// One launch that packs the guide and one per pass, ping-ponging between the scratch's images (denoise_scratch_bytes); the last pass writes
// out.  Refused before anything is enqueued: bad parameters, out overlapping an input or the scratch.
size_t denoise_scratch_bytes(uint32_t w, uint32_t h, uint32_t passes);
void launch_denoise(const float* rgba, const float* aov, uint32_t w, uint32_t h, const DenoiseParams& p, float* out, void* scratch, hipStream_t s);

// reprojection (nrc_reproject.hpp): the history {hist_rgba [h][w][4], hist_n [h][w], hist_aov [h][w][4]} -- all three or, with a view made
// without history, none -- carried into the current view {rgba, aov} -> out [h][w][4], out_n [h][w]; all device memory, the images 16-byte
// aligned.  One launch.  Refused before anything is enqueued: an output that overlaps an input or the other output, a half-given history.
void launch_reproject(const float* hist_rgba, const float* hist_n, const float* hist_aov, const float* rgba, const float* aov, uint32_t w, uint32_t h,
                      const ReprojectView& view, float* out, float* out_n, hipStream_t s);

// ring: {uint head, uint tail, RayInfo[ring_size]}; scratch: uint32[2*T + 4]
// start == nullptr: the whole of prep_train_rays.comp (scan, pop / trace / write, ring push).  start != nullptr (long train paths, the split
// frame graph): scan, the rays' start vertices -> start ([T][6] floats) + the training inputs, ring push; launch_train_trace does the rest
// tail_query / tail_rec (self-training, include/nrc_hpm.h): also write every sample's tail record -- [T*spp][5] queries, [T*spp][4]
// {light.rgb, factor} -- (one-launch path and the trace; nullptr: none, the kernels of the reference's targets)
void launch_prep_train(const DevScene& sc, const DevFrame& fr, const TrainGrid& tg, const float* info,
                       const float* origin, const float* dir, uint32_t* ring, uint32_t* scratch, float* train_in,
                       float* train_target, hipStream_t s, float* start = nullptr, float* tail_query = nullptr, float* tail_rec = nullptr);
void launch_train_trace(const DevScene& sc, const DevFrame& fr, const TrainGrid& tg, const float* start, float* train_target, hipStream_t s,
                        float* tail_query = nullptr, float* tail_rec = nullptr);
// self-training's targets from the tail records and the cache's outputs at the tails (tail_y [T*spp][3]) -> train_target [T][3]
void launch_self_train_combine(uint32_t T, uint32_t spp, const float* tail_rec, const float* tail_y, float* train_target, hipStream_t s);
bool train_paths_are_long(const TrainGrid& tg);      // train ray length x spp >= 4 (quirk Q2 fixed, or a reference build with longer paths)

void integrator_set_wave_priority_raise(int on);      // nrc_common.hpp: NRC_RAISE_WAVE_PRIORITY's run-time switch, this file's kernels
void launch_composite(const DevFrame& fr, uint32_t show_nrc, float blend_factor, const float* primary,
                      const float* info, const float* infer_out, float* out_rgba, hipStream_t s, uint32_t* live_count_reset = nullptr);

// Reference::Result; d_scratch: double[8 + 2048]
void launch_compare(const float* ref_rgba, const float* own_rgba, uint32_t n_pixels, double* d_scratch, float* d_result5,
                    hipStream_t s);

// the metrics of a frame sharded over ranks: _1 leaves this rank's raw sums in d_scratch[0..3] (all-reduce them), _2 this rank's raw
// variance sum around the global mean in d_scratch[4] (all-reduce it), _3 writes the Result
void launch_compare_sharded_1(const float* ref_rgba, const float* own_rgba, uint32_t n_pixels, double* d_scratch, hipStream_t s);
void launch_compare_sharded_2(const float* ref_rgba, const float* own_rgba, uint32_t n_pixels, double* d_scratch, hipStream_t s);
void launch_compare_sharded_3(double* d_scratch, float* d_result5, hipStream_t s);
// a sharded frame's column strips: local [h][lw] -> [h][max_lw]; gathered [world][h][max_lw] -> [h][gw]
void launch_pad_columns(const float* local, uint32_t lw, uint32_t h, uint32_t max_lw, float* padded, hipStream_t s);
void launch_assemble_columns(const float* gathered, uint32_t world, uint32_t block_log2, uint32_t gw, uint32_t h, uint32_t max_lw, float* out,
                             hipStream_t s);
void launch_test_math(int fn, const float* a, const float* b, uint32_t n, float* out, float* out2, hipStream_t s);
void launch_test_rng(float u, float v, const float* frame_random4, uint32_t n, float* out, hipStream_t s);

}  // namespace nrc
