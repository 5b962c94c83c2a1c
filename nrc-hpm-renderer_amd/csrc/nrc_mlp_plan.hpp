// nrc_mlp_plan.hpp -- what Mlp (nrc_mlp.hpp) computes without a device: the model's shapes and offsets, tiny-cuda-nn's parameter
// initialisation and layout, the fragment-image gather tables and their inversion, the weight-gradient tile and task lists, the split-K
// chunking that sizes the slabs, the bin plan of the table gradient and the LDS sizes of the generic training kernels.  Device-free:
// the standard library, nrc_fail.hpp and the boundary header (tests/cpp/mlp_plan_main.cpp runs it under the sanitizers against a
// transcription of the code it came from).  The PODs below are kernel arguments and device tables: nrc_mlp.hip's kernels read them, so
// their layouts are fixed.  NRC_PLAN_HD is the one place of this file that knows about the device compiler.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/nrc_hpm.h"
#include "nrc_fail.hpp"

#if defined(__HIPCC__)
#define NRC_PLAN_HD __host__ __device__ inline
#else
#define NRC_PLAN_HD inline
#endif

namespace nrc {

// ------------------------------------------------------------------------------------------------ the model
inline uint32_t pos_enc_dims(uint32_t id) { return id == 0 ? 32u : id == 1 ? 3u : id == 2 ? 36u : id == 3 ? 72u : 0u; }
inline uint32_t dir_enc_dims(uint32_t id) { return id == 0 ? 8u : id == 1 ? 2u : id == 2 ? 8u : ~0u; }

struct MlpLayer {
    uint32_t out, in;
    uint32_t off;   // offset into the canonical fp32 parameter vector ([out][in] row-major)
};

constexpr uint32_t HG_LEVELS = 16;
struct HashLevels {
    uint32_t off[HG_LEVELS + 1];      // per-level entry offsets
};

struct MlpPlan {
    uint32_t width = 0, depth = 0;
    uint32_t kw = 0;                 // width the kernels run at: max(width, 32)
    uint32_t enc_dims = 0, loss_id = 0;
    bool sgd = false;                // nested optimizer: Adam (default) or SGD
    bool fused = false;              // north-star model (Frequency+OneBlob, 6x64): fully fused kernels; otherwise the generic path
    bool hash = false;               // posID 0: the hash-grid table [entry][2] follows the matrices in every vector
    bool enc80_generic = false;      // generic model whose EMA inference encodes Frequency(12)+OneBlob(4) inside k_infer_gen
    std::vector<MlpLayer> layers;
    uint32_t n_mlp = 0;              // matrix parameters
    uint32_t hg_off[HG_LEVELS + 1] = {};
    uint32_t n_grid_entries = 0, n_params = 0;
};

inline MlpPlan make_mlp_plan(const nrc_config& cfg)
{
    MlpPlan p;
    p.width = cfg.nn_width;
    p.depth = cfg.nn_depth;
    if (pos_enc_dims(cfg.pos_id) == 0 || dir_enc_dims(cfg.dir_id) == ~0u) fail("NNEncodingConfig posID/dirID is invalid");
    if (p.width != 16 && p.width != 32 && p.width != 64 && p.width != 128)
        fail("nnWidth must be 16, 32, 64 or 128 -- tiny-cuda-nn's FullyFusedMLP widths (got " + std::to_string(p.width) + ")");
    // a 16-wide network runs on the 32-row MFMA tiles of the 32-wide kernels: neurons 16..31 of every hidden layer have all-zero
    // fragment entries, so they stay exactly 0 through ReLU and contribute exactly 0 downstream; the parameter vector, gradients
    // and optimizer see the true 16-wide shapes (half of the MFMA work is padding: the model is 10x cheaper than 6x64 anyway)
    p.kw = p.width < 32 ? 32 : p.width;
    if (p.depth < 1 || p.depth > 16) fail("nnDepth must be in 1..16 (got " + std::to_string(p.depth) + ")");
    if (std::strcmp(cfg.optimizer, "Adam") == 0) p.sgd = false;
    else if (std::strcmp(cfg.optimizer, "SGD") == 0) p.sgd = true;
    else fail(std::string("unsupported optimizer ") + cfg.optimizer + " (Adam and SGD are built; both run inside the EMA wrapper)");
    static const char* const losses[] = {"RelativeL2Luminance", "L2", "RelativeL2", "L1", "Mape", "Smape", "LogL1"};
    for (p.loss_id = 0; p.loss_id < 7u && std::strcmp(cfg.loss_fn, losses[p.loss_id]) != 0;) p.loss_id++;
    if (p.loss_id == 7u)
        fail(std::string("unsupported loss ") + cfg.loss_fn +
             " (built: RelativeL2Luminance, L2, RelativeL2, L1, Mape, Smape, LogL1; tiny-cuda-nn's CrossEntropy and Variance need a "
             "sample pdf the NRC path does not have)");
    // encoded width, padded to a multiple of 16 with 1.0 (tiny-cuda-nn); the fused kernels cover the north-star model
    p.enc_dims = (pos_enc_dims(cfg.pos_id) + dir_enc_dims(cfg.dir_id) + 15u) / 16u * 16u;
    p.fused = cfg.pos_id == 3 && cfg.dir_id == 0 && p.width == 64 && p.depth == 6;
    for (uint32_t l = 0; l <= p.depth; l++) {
        const MlpLayer L{l == p.depth ? 3u : p.width, l == 0 ? p.enc_dims : p.width, p.n_mlp};
        p.n_mlp += L.in * L.out;
        p.layers.push_back(L);
    }
    p.hash = cfg.pos_id == 0;
    if (p.hash) {      // per-level tables: dense while res^3 (rounded up to 8) fits, else 2^log2_hashmap_size entries
        const uint32_t log2_size = cfg.hashgrid_log2_size ? cfg.hashgrid_log2_size : 19u;
        if (log2_size < 4 || log2_size > 24) fail("hashgrid_log2_size must be in 4..24");
        for (uint32_t l = 0; l < HG_LEVELS; l++) {
            const double dense = std::pow((double)(16u << l), 3.0);
            uint32_t cnt = dense > 2147483647.0 ? 2147483647u : (uint32_t)dense;
            cnt = (cnt + 7u) / 8u * 8u;
            if (cnt > (1u << log2_size)) cnt = 1u << log2_size;
            p.hg_off[l + 1] = p.hg_off[l] + cnt;
        }
        p.n_grid_entries = p.hg_off[HG_LEVELS];
    }
    p.n_params = p.n_mlp + p.n_grid_entries * 2u;
    // k_grid_opt2 updates four parameters (two entries) per 16-byte access.  Neither can fail: every matrix has a multiple of 16 rows or
    // columns (widths 16..128, enc_dims padded to 16), every level a multiple of 8 or 2^k >= 16 entries.
    if (p.n_mlp % 4u != 0u || p.n_grid_entries % 2u != 0u) fail("the table optimizer needs n_mlp % 4 == 0 and an even number of table entries");
    // Generic models with the Frequency(12) + OneBlob(4) input (configs[4]'s 8x128): EMA inference encodes inside k_infer_gen as
    // k_infer does, so its image takes layer 0's inputs in that encoder's order (fmap80); training keeps k_encode's natural order
    p.enc80_generic = !p.fused && !p.hash && cfg.pos_id == 3 && cfg.dir_id == 0;
    return p;
}

// ------------------------------------------------------------------------------------------------ initial parameters, tiny-cuda-nn's layout
// O'Neill's pcg32 (XSH-RR) as tiny-cuda-nn vendors it (pcg32.h): its Trainer seeds pcg32{1337}, i.e. stream initseq = 1
struct Pcg32 {
    uint64_t state = 0, inc = 1;
    void seed(uint64_t init_state, uint64_t init_seq = 1u)
    {
        state = 0; inc = (init_seq << 1) | 1u; next(); state += init_state; next();
    }
    uint32_t next()
    {
        uint64_t old = state;
        state = old * 6364136223846793005ULL + inc;
        uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u);
        uint32_t rot = (uint32_t)(old >> 59u);
        return (xs >> rot) | (xs << ((32u - rot) & 31u));
    }
    // pcg32::next_float: a float in [1, 2) from the top 23 bits (the MTGP trick), minus 1
    float nextf()
    {
        const uint32_t u = (next() >> 9) | 0x3f800000u;
        float f;
        std::memcpy(&f, &u, 4);
        return f - 1.0f;
    }
};

// tiny-cuda-nn's own parameter layout (params_full_precision of its Trainer): the same matrices in the same order with the output
// matrix stored 16 x width (rows 3..15 feed the padded outputs nobody reads), then the table: n_params + 13 * width values
inline uint32_t tcnn_dead_count(const MlpPlan& p) { return 13u * p.width; }
inline uint32_t tcnn_param_count(const MlpPlan& p) { return p.n_params + tcnn_dead_count(p); }

struct MlpInit {
    std::vector<float> w;              // [n_params]
    std::vector<float> dead_rows;      // rows 3..15 of tiny-cuda-nn's 16 x width output matrix
};
// tiny-cuda-nn v1.6's initialisation (src/NeuralRadianceCache.cu:39 -> tcnn::create_from_config -> Trainer::initialize_params;
// recalled from upstream, the submodule is absent -- DESIGN.md section 2): pcg32{seed} on stream 1; the network's matrices first
// -- each Xavier-uniform under the bound sqrt(6 / (rows + columns)) of its STORED shape, element = next_float() * 2 * scale - scale
// in that order of operations, the output matrix stored with 16 rows (rows 3..15: drawn, kept for the tcnn-layout dump, never part
// of this model) --, then the table: generate_random_uniform's GPU order (thread i of ceil(n / 4) rounded up to 128 writes draw
// 4 i + j to element i + n_threads * j), value = fma(u, 2e-4, -1e-4).
inline MlpInit mlp_initial_params(const MlpPlan& p, uint32_t seed)
{
    MlpInit init{std::vector<float>(p.n_params), std::vector<float>(tcnn_dead_count(p), 0.0f)};
    Pcg32 rng;
    rng.seed(seed, 1);
    for (uint32_t l = 0; l <= p.depth; l++) {
        const MlpLayer& L = p.layers[l];
        const uint32_t rows = l == p.depth ? 16u : L.out;
        const float scale = 1.0f * sqrtf(6.0f / (float)(L.in + rows));
        for (uint32_t i = 0; i < L.in * rows; i++) {
            const float x = rng.nextf() * 2.0f * scale - scale;
            if (i < L.in * L.out) init.w[L.off + i] = x;
            else init.dead_rows[i - L.in * L.out] = x;
        }
    }
    const size_t n_grid = (size_t)p.n_grid_entries * 2;
    if (n_grid > 0) {
        const size_t n_threads = ((n_grid + 3) / 4 + 127) / 128 * 128;
        const float lower = -1e-4f, upper = 1e-4f;
        for (size_t k = 0; k < 4 * n_threads; k++) {
            const float u = rng.nextf();
            const size_t idx = k / 4 + n_threads * (k % 4);
            if (idx < n_grid) init.w[p.n_mlp + idx] = fmaf(u, upper - lower, lower);
        }
    }
    return init;
}

// own [n_params] -> tcnn [tcnn_param_count]; dead_rows: the buffer's 13 x width rows, or null (the gradient's: zero)
inline void to_tcnn_layout(const MlpPlan& p, const float* dead_rows, const float* own, float* tcnn)
{
    const size_t dead = tcnn_dead_count(p);
    std::memcpy(tcnn, own, (size_t)p.n_mlp * sizeof(float));
    if (dead_rows != nullptr) std::memcpy(tcnn + p.n_mlp, dead_rows, dead * sizeof(float));
    else std::memset(tcnn + p.n_mlp, 0, dead * sizeof(float));
    std::memcpy(tcnn + p.n_mlp + dead, own + p.n_mlp, (size_t)(p.n_params - p.n_mlp) * sizeof(float));
}
// the inverse; dead_rows (may be null) takes the rows the model does not have
inline void from_tcnn_layout(const MlpPlan& p, float* dead_rows, const float* tcnn, float* own)
{
    const size_t dead = tcnn_dead_count(p);
    std::memcpy(own, tcnn, (size_t)p.n_mlp * sizeof(float));
    if (dead_rows != nullptr) std::memcpy(dead_rows, tcnn + p.n_mlp, dead * sizeof(float));
    std::memcpy(own + p.n_mlp, tcnn + p.n_mlp + dead, (size_t)(p.n_params - p.n_mlp) * sizeof(float));
}

// ------------------------------------------------------------------------------------------------ fragment-image gather tables
// canonical feature index held by (k-step s, lane half h, element j) of the layer-0 B operand.
// s<4: natural order 16s+8h+j = four (sin,cos) pairs of one (dim, frequency quad);
// s=4: both lane halves get two (sin,cos) pairs of dim 2 and the four OneBlob bins of ONE direction dim,
//      so the two halves of a wave execute the same instruction stream.
NRC_PLAN_HD int fmap80(int s, int h, int j)
{
    if (s < 4) return 16 * s + 8 * h + j;
    if (j < 4) return 64 + 4 * h + j;
    return 72 + 4 * h + (j - 4);
}
// neuron index held by (k-step s, lane half h, element j) when a 32x32 accumulator pair is re-used as B operand
NRC_PLAN_HD int kperm(int s, int h, int j) { return 16 * s + 8 * (j >> 2) + 4 * h + (j & 3); }

// packed slot -> canonical parameter index (-1 = zero) of the fp16 MFMA A-operand images, [frag][lane][8]:
// forward image: layer 0 [mt][s], hidden layer l [mt][s], output [s];
// backward image: hidden layer l (W^T) [mt over inputs][s over outputs], output layer [mt] (one k-step, 3 live rows), and for a model
// with a trainable table W0^T [s] (rows = encoded dims 0..31) for dL/d(input)
struct FragMaps {
    uint32_t n_frag_fwd = 0, n_frag_bwd = 0;
    std::vector<int32_t> fwd, bwd;
    std::vector<int32_t> inf_own;      // the EMA inference image's map where it is not the forward map (enc80_generic)
    const std::vector<int32_t>& inf() const { return inf_own.empty() ? fwd : inf_own; }
};
inline size_t frag_slot(int frag, int lane, int j) { return ((size_t)frag * 64 + lane) * 8 + j; }
// layer 0's slots of a forward-shaped map, its inputs in k_encode's natural order or in the in-kernel encoder's (fmap80)
inline void set_layer0_slots(const MlpPlan& p, bool fmap80_order, std::vector<int32_t>& map)
{
    const int mt_n = (int)p.kw / 32, ks0 = (int)p.enc_dims / 16, W = (int)p.width, E = (int)p.enc_dims;
    for (int lane = 0; lane < 64; lane++) {
        const int r = lane & 31, h = lane >> 5;
        for (int j = 0; j < 8; j++)
            for (int mt = 0; mt < mt_n; mt++)
                for (int s = 0; s < ks0 && 32 * mt + r < W; s++)      // rows beyond the true width stay -1 = zero (width 16)
                    map[frag_slot(mt * ks0 + s, lane, j)] =
                        (int32_t)(p.layers[0].off + (32 * mt + r) * E + (fmap80_order ? fmap80(s, h, j) : 16 * s + 8 * h + j));
    }
}
inline FragMaps make_frag_maps(const MlpPlan& p)
{
    const int D = (int)p.depth, mt_n = (int)p.kw / 32, ksh = (int)p.kw / 16, ks0 = (int)p.enc_dims / 16, W = (int)p.width, E = (int)p.enc_dims;
    const int hid_base = mt_n * ks0, out_base = hid_base + (D - 1) * mt_n * ksh;
    const int din_base = (D - 1) * mt_n * ksh + mt_n;
    FragMaps m;
    m.n_frag_fwd = (uint32_t)(out_base + ksh);
    m.n_frag_bwd = (uint32_t)(din_base + (p.hash ? ksh : 0));
    m.fwd.assign((size_t)m.n_frag_fwd * 512, -1);
    m.bwd.assign((size_t)m.n_frag_bwd * 512, -1);
    const std::vector<MlpLayer>& Ls = p.layers;
    set_layer0_slots(p, p.fused, m.fwd);
    for (int lane = 0; lane < 64; lane++) {
        const int r = lane & 31, h = lane >> 5;
        for (int j = 0; j < 8; j++) {
            for (int mt = 0; mt < mt_n; mt++) {
                if (32 * mt + r >= W) continue;               // rows / columns beyond the true width stay -1 = zero (width 16)
                for (int l = 1; l < D; l++)
                    for (int s = 0; s < ksh; s++) {
                        if (kperm(s, h, j) >= W) continue;
                        m.fwd[frag_slot(hid_base + (l - 1) * mt_n * ksh + mt * ksh + s, lane, j)] = (int32_t)(Ls[l].off + (32 * mt + r) * W + kperm(s, h, j));
                        m.bwd[frag_slot((l - 1) * mt_n * ksh + mt * ksh + s, lane, j)] = (int32_t)(Ls[l].off + kperm(s, h, j) * W + (32 * mt + r));
                    }
                const int k = 8 * h + j;
                if (k < 3) m.bwd[frag_slot((D - 1) * mt_n * ksh + mt, lane, j)] = (int32_t)(Ls[D].off + k * W + (32 * mt + r));
            }
            for (int s = 0; s < ksh; s++) {
                if (kperm(s, h, j) >= W) continue;
                if (r < 3) m.fwd[frag_slot(out_base + s, lane, j)] = (int32_t)(Ls[D].off + r * W + kperm(s, h, j));
                if (p.hash) m.bwd[frag_slot(din_base + s, lane, j)] = (int32_t)(Ls[0].off + kperm(s, h, j) * E + r);
            }
        }
    }
    if (p.enc80_generic) {
        m.inf_own = m.fwd;
        set_layer0_slots(p, true, m.inf_own);
    }
    return m;
}

// inverse maps for the one-launch optimizer step (k_opt_pack): dst[3][n_mlp], parameter -> its slot in the forward / EMA inference /
// backward image (-1: in none).  Empty when an image is not one-to-one, or when the caller does not want the fused step (no_fused_opt)
inline std::vector<int32_t> invert_frag_maps(const std::vector<int32_t>& fwd, const std::vector<int32_t>& inf, const std::vector<int32_t>& bwd,
                                             uint32_t n_mlp, bool no_fused_opt)
{
    if (no_fused_opt) return {};
    std::vector<int32_t> dst((size_t)3 * n_mlp, -1);
    const std::vector<int32_t>* src[3] = {&fwd, &inf, &bwd};
    for (int k = 0; k < 3; k++) {
        int32_t* out = dst.data() + (size_t)k * n_mlp;
        for (size_t j = 0; j < src[k]->size(); j++) {
            const int32_t i = (*src[k])[j];
            if (i < 0) continue;
            if ((uint32_t)i >= n_mlp || out[i] >= 0) return {};
            out[i] = (int32_t)j;
        }
    }
    return dst;
}

// ------------------------------------------------------------------------------------------------ weight-gradient lists, split-K chunking
// k_wgrad's output tiles: one 32-column block of a layer's input against one 32-row block of its delta
struct WgradTile {
    uint32_t a_row0, b_row0, m_valid, n_valid, param_off, in_dim;
};
// k_wgrad2's row-block tasks: one 32-row block of a layer's delta against a group of up to WGRAD2_NTL 32-column blocks of its input
struct WgradTask {
    uint32_t a_row0, b_row0, m_valid, n_tiles, n_valid_last, param_off, in_dim, pad;
};
#ifndef NRC_WGRAD2_NTL
#define NRC_WGRAD2_NTL 4            // 32-column blocks (accumulators) per task, at most 4
#endif
constexpr uint32_t WGRAD_CHUNK = 128;
constexpr int WGRAD2_WAVES = 4;
constexpr int WGRAD2_NTL = NRC_WGRAD2_NTL;

struct WgradLists {
    std::vector<WgradTile> tiles;
    std::vector<WgradTask> tasks;
};
// one enumeration of the (layer, 32-row block, 32-column block) rectangles: a task is WGRAD2_NTL consecutive tiles of one row block
inline WgradLists make_wgrad_lists(const MlpPlan& p)
{
    WgradLists out;
    const uint32_t D = p.depth;
    for (uint32_t l = 0; l <= D; l++) {
        const MlpLayer& L = p.layers[l];
        const uint32_t a_rows = l == D ? D * p.kw : l * p.kw;                       // delta_l rows (kernel width: 32 for width 16)
        const uint32_t b_rows = l == 0 ? 0 : p.enc_dims + (l - 1) * p.kw;           // a_{l-1} rows (enc for l = 0)
        for (uint32_t mt = 0; mt * 32 < L.out; mt++)
            for (uint32_t nt = 0; nt * 32 < L.in; nt++) {
                const uint32_t m_valid = std::min(L.out - 32 * mt, 32u), n_valid = std::min(L.in - 32 * nt, 32u);
                out.tiles.push_back(WgradTile{a_rows + 32 * mt, b_rows + 32 * nt, m_valid, n_valid, L.off + 32 * mt * L.in + 32 * nt, L.in});
                if (nt % (uint32_t)WGRAD2_NTL == 0u)
                    out.tasks.push_back(WgradTask{a_rows + 32 * mt, b_rows + 32 * nt, m_valid, 0u, 0u, L.off + 32 * mt * L.in + 32 * nt, L.in, 0u});
                out.tasks.back().n_tiles++;
                out.tasks.back().n_valid_last = n_valid;
            }
    }
    return out;
}

namespace plan_detail {
constexpr uint32_t cdiv(uint32_t a, uint32_t b) { return (a + b - 1) / b; }
}
// K-chunks a k_wgrad2 launch aims at: ~2 workgroups per CU
inline uint32_t wgrad_target_chunks(uint32_t n_tasks, uint32_t num_cus)
{
    return std::max(1u, 2u * num_cus / std::max(1u, plan_detail::cdiv(n_tasks, (uint32_t)WGRAD2_WAVES)));
}
// samples per K-chunk of the weight-gradient launch: k_wgrad's fixed chunk, or what gives the target count -- a multiple of 32, at least 64
inline uint32_t wgrad_chunk(uint32_t n, uint32_t n_tasks, uint32_t num_cus, bool wgrad_old)
{
    if (wgrad_old) return WGRAD_CHUNK;
    return std::max(plan_detail::cdiv(plan_detail::cdiv(n, wgrad_target_chunks(n_tasks, num_cus)), 32u) * 32u, 64u);
}
// the slabs a workspace for batches up to n needs (k_wgrad2: a smaller batch has a smaller chunk, never more chunks than the target)
inline uint32_t wgrad_max_chunks(uint32_t n, uint32_t n_tasks, uint32_t num_cus, bool wgrad_old)
{
    const uint32_t chunks = plan_detail::cdiv(n, wgrad_chunk(n, n_tasks, num_cus, wgrad_old));
    return wgrad_old ? chunks : std::max(chunks, wgrad_target_chunks(n_tasks, num_cus));
}

// ------------------------------------------------------------------------------------------------ bin plan of the table gradient
#ifndef NRC_GB_BIN_LOG2
#define NRC_GB_BIN_LOG2 11
#endif
constexpr uint32_t GB_BIN_LOG2 = NRC_GB_BIN_LOG2, GB_BIN = 1u << GB_BIN_LOG2, GB_MAX_BINS = 1u << (20 - NRC_GB_BIN_LOG2), GB_MIN_BINS = 8;
struct GridBins {
    uint32_t first[HG_LEVELS], count[HG_LEVELS];      // per level: index of its first bin, number of bins (0: no lists, the level adds into the shadow)
    uint32_t cap[HG_LEVELS], list0[HG_LEVELS];        // pairs a bin's list holds; pair offset of the level's first list
};
// the levels WITHOUT bins: {first entry, count} of n ranges (k_grid_gather walks them GB_BIN entries per workgroup)
struct LooseRanges {
    uint32_t first[HG_LEVELS], count[HG_LEVELS], n;
};
struct GridBinPlan {
    GridBins bins = {};
    LooseRanges loose = {};
    uint32_t loose_chunks = 0, bins_total = 0;
    std::vector<uint32_t> info;      // uint4 per bin: {first entry, pair offset of the list, capacity, 0}
    size_t pairs = 0;                // what the lists hold together
};
// bin lists of the table gradient (k_grid_scatter) for batches up to n: levels of GB_MIN_BINS..GB_MAX_BINS bins of GB_BIN entries; a level's
// lists hold twice what the level sends a bin on average (n * 8 / bins pairs); the rest goes into the fixed-point shadow (no_bins: everything)
inline GridBinPlan make_grid_bin_plan(const uint32_t (&hg_off)[HG_LEVELS + 1], uint32_t n, bool no_bins)
{
    GridBinPlan g;
    for (uint32_t l = 0; l < HG_LEVELS; l++) {
        const uint32_t cnt = hg_off[l + 1] - hg_off[l];
        const uint32_t bins = (cnt % GB_BIN == 0u) ? cnt / GB_BIN : 0u;
        const uint32_t count = (bins >= GB_MIN_BINS && bins <= GB_MAX_BINS && !no_bins) ? bins : 0u;
        const uint32_t cap = count ? std::max(1024u, (uint32_t)std::min<uint64_t>(2ull * n * 8ull / count, 1u << 24)) : 0u;
        g.bins.first[l] = g.bins_total;
        g.bins.count[l] = count;
        g.bins.cap[l] = cap;
        g.bins.list0[l] = (uint32_t)g.pairs;
        for (uint32_t b = 0; b < count; b++) g.info.insert(g.info.end(), {hg_off[l] + b * GB_BIN, (uint32_t)(g.pairs + (size_t)b * cap), cap, 0u});
        g.pairs += (size_t)count * cap;
        g.bins_total += count;
        if (count == 0u) {
            g.loose.first[g.loose.n] = hg_off[l];
            g.loose.count[g.loose.n] = cnt;
            g.loose_chunks += plan_detail::cdiv(cnt, GB_BIN);
            g.loose.n++;
        }
    }
    if (g.pairs > 0xffffffffull) fail("train batch too large for the table gradient's bin lists");
    return g;
}

// ------------------------------------------------------------------------------------------------ LDS of the generic training kernels
// the k-group transposition scratch of a wave (store_kgroups, nrc_mlp.hip): 16 rows padded to 40 halves
constexpr int KG_ROW = 40;                          // halves per scratch row
constexpr int KG_SCRATCH = 16 * KG_ROW * 2;         // bytes per wave
constexpr size_t TRAIN_GEN_LDS_CAP = 160 * 1024;
// k_train_gen<kw, waves>: two weight stages + per wave: the k-group transposition scratch and one 64-bit ReLU mask per lane and layer
inline size_t train_gen_lds(uint32_t kw, uint32_t depth, uint32_t waves)
{
    const size_t mtg = kw / 32, ksg = kw / 16;
    const size_t lds = 2 * mtg * (ksg > 5 ? ksg : 5) * 1024 + waves * (KG_SCRATCH + (size_t)depth * 512);
    if (lds > TRAIN_GEN_LDS_CAP) fail("network too deep for the training kernel's LDS budget");
    return lds;
}
// k_train_gen2<kw, nt>: sgn sample groups of nt tiles per workgroup of four waves
inline size_t train_gen2_lds(uint32_t kw, uint32_t depth, uint32_t sgn, int nt)
{
    const size_t ksg = kw / 16;
    const size_t lds = (size_t)2 * sgn * nt * ksg * 1024 + 4 * KG_SCRATCH + (size_t)4 * depth * nt * 256;
    if (lds > TRAIN_GEN_LDS_CAP) fail("network too deep for the training kernel's LDS budget");
    return lds;
}

}  // namespace nrc
