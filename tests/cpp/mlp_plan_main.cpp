// mlp_plan_main.cpp -- Mlp's device-free half (csrc/nrc_mlp_plan.hpp) driven on the CPU; tests/test_mlp_plan_host.py builds this with
// AddressSanitizer + UndefinedBehaviorSanitizer and runs it.
// The reference (namespace ref) is the host code the header came from -- Mlp's constructor, build_wgrad_tasks, the tile loop, wgrad_chunk,
// the max_chunks expression, the bin-plan loops and the two LDS expressions -- transcribed with the members as fields and the constants as
// literals; it shares nothing with the header but nrc_config and fail().  The property cases restate nothing: they check what the kernels rely on.
// With a directory as argument the program also writes the initial parameters of a few models there (own and tiny-cuda-nn layout) for the
// Python test to compare with the oracle.  Every CHECK compares a value; the last line printed is "mlp_plan: <n> cases, <m> checks"
// (exit status 1 if any check failed).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../nrc-hpm-renderer_amd/csrc/nrc_mlp_plan.hpp"

using namespace nrc;

static int g_cases = 0, g_checks = 0, g_failed = 0;
static const char* g_case = "";
static std::string g_what;
#define CHECK(cond)                                                                                                                       \
    do {                                                                                                                                  \
        g_checks++;                                                                                                                       \
        if (!(cond)) { if (g_failed++ < 40) std::printf("FAILED %s:%d [%s %s] %s\n", __FILE__, __LINE__, g_case, g_what.c_str(), #cond); } \
    } while (0)
static void begin_case(const char* name) { g_case = name; g_what.clear(); g_cases++; }

static nrc_config make_cfg(uint32_t pos, uint32_t dir, uint32_t width, uint32_t depth, uint32_t log2 = 0, const char* loss = "RelativeL2Luminance",
                           const char* opt = "Adam", uint32_t seed = 1337)
{
    nrc_config c;
    std::memset(&c, 0, sizeof c);
    std::snprintf(c.loss_fn, sizeof c.loss_fn, "%s", loss);
    std::snprintf(c.optimizer, sizeof c.optimizer, "%s", opt);
    c.pos_id = pos; c.dir_id = dir; c.nn_width = width; c.nn_depth = depth; c.hashgrid_log2_size = log2; c.seed = seed;
    return c;
}
static std::string describe(const nrc_config& c)
{
    return "pos " + std::to_string(c.pos_id) + " dir " + std::to_string(c.dir_id) + " " + std::to_string(c.nn_depth) + "x" + std::to_string(c.nn_width) +
           " log2 " + std::to_string(c.hashgrid_log2_size);
}
template <class F>
static std::string failure_of(F&& f)
{
    try { f(); } catch (const std::exception& e) { return e.what(); }
    return "";
}

// ================================================================================================ the reference: the parent's host code
namespace ref {

static uint32_t ceil_div(uint32_t a, uint32_t b) { return (a + b - 1) / b; }
static uint32_t pos_enc_dims(uint32_t id) { return id == 0 ? 32u : id == 1 ? 3u : id == 2 ? 36u : id == 3 ? 72u : 0u; }
static uint32_t dir_enc_dims(uint32_t id) { return id == 0 ? 8u : id == 1 ? 2u : id == 2 ? 8u : ~0u; }
static int fmap80(int s, int h, int j)
{
    if (s < 4) return 16 * s + 8 * h + j;
    if (j < 4) return 64 + 4 * h + j;
    return 72 + 4 * h + (j - 4);
}
static int kperm(int s, int h, int j) { return 16 * s + 8 * (j >> 2) + 4 * h + (j & 3); }
struct Pcg {
    uint64_t state = 0, inc = 1;
    void seed(uint64_t init_state, uint64_t init_seq) { state = 0; inc = (init_seq << 1) | 1u; next(); state += init_state; next(); }
    uint32_t next()
    {
        uint64_t old = state;
        state = old * 6364136223846793005ULL + inc;
        uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u);
        uint32_t rot = (uint32_t)(old >> 59u);
        return (xs >> rot) | (xs << ((32u - rot) & 31u));
    }
    float nextf()
    {
        const uint32_t u = (next() >> 9) | 0x3f800000u;
        float f;
        std::memcpy(&f, &u, 4);
        return f - 1.0f;
    }
};
struct Layer { uint32_t out, in, off; };
struct Tile { uint32_t a_row0, b_row0, m_valid, n_valid, param_off, in_dim; };
struct Task { uint32_t a_row0, b_row0, m_valid, n_tiles, n_valid_last, param_off, in_dim, pad; };

struct Model {
    uint32_t width_ = 0, depth_ = 0, enc_dims_ = 0, n_params_ = 0, kw_ = 0, loss_id_ = 0, n_mlp_ = 0, n_grid_entries_ = 0;
    bool sgd_ = false, fused_ = false, hash_ = false, enc80_generic_ = false, fused_opt_ = false;
    std::vector<Layer> layers_;
    uint32_t hg_off_[17] = {0};
    uint32_t n_frag_fwd_ = 0, n_frag_bwd_ = 0;
    std::vector<int32_t> sf, sb, si, dst;      // si: empty unless enc80_generic_
    std::vector<float> w, dead;
    std::vector<Task> tasks;
    std::vector<Tile> tiles;

    // Mlp::Mlp; with_init: the parameters too (a 2^24 table is too large to draw under the sanitizers)
    Model(const nrc_config& cfg, bool with_init, bool no_fused_opt)
    {
        width_ = cfg.nn_width;
        depth_ = cfg.nn_depth;
        if (pos_enc_dims(cfg.pos_id) == 0 || dir_enc_dims(cfg.dir_id) == ~0u) fail("NNEncodingConfig posID/dirID is invalid");
        if (width_ != 16 && width_ != 32 && width_ != 64 && width_ != 128)
            fail("nnWidth must be 16, 32, 64 or 128 -- tiny-cuda-nn's FullyFusedMLP widths (got " + std::to_string(width_) + ")");
        kw_ = width_ < 32 ? 32 : width_;
        if (depth_ < 1 || depth_ > 16) fail("nnDepth must be in 1..16 (got " + std::to_string(depth_) + ")");
        if (std::strcmp(cfg.optimizer, "Adam") == 0) sgd_ = false;
        else if (std::strcmp(cfg.optimizer, "SGD") == 0) sgd_ = true;
        else fail(std::string("unsupported optimizer ") + cfg.optimizer + " (Adam and SGD are built; both run inside the EMA wrapper)");
        if (std::strcmp(cfg.loss_fn, "RelativeL2Luminance") == 0) loss_id_ = 0;
        else if (std::strcmp(cfg.loss_fn, "L2") == 0) loss_id_ = 1;
        else if (std::strcmp(cfg.loss_fn, "RelativeL2") == 0) loss_id_ = 2;
        else if (std::strcmp(cfg.loss_fn, "L1") == 0) loss_id_ = 3;
        else if (std::strcmp(cfg.loss_fn, "Mape") == 0) loss_id_ = 4;
        else if (std::strcmp(cfg.loss_fn, "Smape") == 0) loss_id_ = 5;
        else if (std::strcmp(cfg.loss_fn, "LogL1") == 0) loss_id_ = 6;
        else
            fail(std::string("unsupported loss ") + cfg.loss_fn +
                 " (built: RelativeL2Luminance, L2, RelativeL2, L1, Mape, Smape, LogL1; tiny-cuda-nn's CrossEntropy and Variance need a "
                 "sample pdf the NRC path does not have)");
        enc_dims_ = (pos_enc_dims(cfg.pos_id) + dir_enc_dims(cfg.dir_id) + 15u) / 16u * 16u;
        fused_ = cfg.pos_id == 3 && cfg.dir_id == 0 && width_ == 64 && depth_ == 6;

        uint32_t off = 0;
        for (uint32_t l = 0; l <= depth_; l++) {
            Layer L;
            L.in = l == 0 ? enc_dims_ : width_;
            L.out = l == depth_ ? 3u : width_;
            L.off = off;
            off += L.in * L.out;
            layers_.push_back(L);
        }
        n_mlp_ = off;
        hash_ = cfg.pos_id == 0;
        uint32_t n_grid = 0;
        if (hash_) {
            const uint32_t log2_size = cfg.hashgrid_log2_size ? cfg.hashgrid_log2_size : 19u;
            if (log2_size < 4 || log2_size > 24) fail("hashgrid_log2_size must be in 4..24");
            uint32_t o = 0;
            for (uint32_t l = 0; l < 16; l++) {
                const double dense = std::pow((double)(16u << l), 3.0);
                uint32_t cnt = dense > 2147483647.0 ? 2147483647u : (uint32_t)dense;
                cnt = (cnt + 7u) / 8u * 8u;
                if (cnt > (1u << log2_size)) cnt = 1u << log2_size;
                hg_off_[l] = o;
                o += cnt;
            }
            hg_off_[16] = o;
            n_grid_entries_ = o;
            n_grid = o * 2u;
        }
        n_params_ = n_mlp_ + n_grid;
        if (n_mlp_ % 4u != 0u || n_grid_entries_ % 2u != 0u) fail("the table optimizer needs n_mlp % 4 == 0 and an even number of table entries");

        if (with_init) {
            w.assign(n_params_, 0.0f);
            Pcg rng;
            rng.seed(cfg.seed, 1);
            dead.assign((size_t)13 * width_, 0.0f);
            for (uint32_t l = 0; l <= depth_; l++) {
                const Layer& L = layers_[l];
                const uint32_t rows = l == depth_ ? 16u : L.out;
                const float scale = 1.0f * sqrtf(6.0f / (float)(L.in + rows));
                for (uint32_t i = 0; i < L.in * rows; i++) {
                    const float x = rng.nextf() * 2.0f * scale - scale;
                    if (i < L.in * L.out) w[L.off + i] = x;
                    else dead[i - L.in * L.out] = x;
                }
            }
            if (n_grid > 0) {
                const size_t n_threads = (((size_t)n_grid + 3) / 4 + 127) / 128 * 128;
                const float lower = -1e-4f, upper = 1e-4f;
                for (size_t k = 0; k < 4 * n_threads; k++) {
                    const float u = rng.nextf();
                    const size_t idx = k / 4 + n_threads * (k % 4);
                    if (idx < n_grid) w[n_mlp_ + idx] = fmaf(u, upper - lower, lower);
                }
            }
        }

        const int D = (int)depth_, mt_n = (int)kw_ / 32, ksh = (int)kw_ / 16, ks0 = (int)enc_dims_ / 16, W = (int)width_;
        const int E = (int)enc_dims_;
        const int hid_base = mt_n * ks0, out_base = hid_base + (D - 1) * mt_n * ksh;
        n_frag_fwd_ = (uint32_t)(out_base + ksh);
        const int din_base = (D - 1) * mt_n * ksh + mt_n;
        n_frag_bwd_ = (uint32_t)(din_base + (hash_ ? ksh : 0));
        sf.assign((size_t)n_frag_fwd_ * 512, -1);
        sb.assign((size_t)n_frag_bwd_ * 512, -1);
        auto slot = [](int frag, int lane, int j) { return ((size_t)frag * 64 + lane) * 8 + j; };
        for (int lane = 0; lane < 64; lane++) {
            const int r = lane & 31, h = lane >> 5;
            for (int j = 0; j < 8; j++) {
                for (int mt = 0; mt < mt_n; mt++) {
                    const bool row_ok = 32 * mt + r < W;
                    for (int s = 0; s < ks0; s++) {
                        const int k = fused_ ? fmap80(s, h, j) : 16 * s + 8 * h + j;
                        if (row_ok) sf[slot(mt * ks0 + s, lane, j)] = (int32_t)(layers_[0].off + (32 * mt + r) * E + k);
                    }
                    for (int l = 1; l < D; l++)
                        for (int s = 0; s < ksh; s++) {
                            if (!row_ok || kperm(s, h, j) >= W) continue;
                            sf[slot(hid_base + (l - 1) * mt_n * ksh + mt * ksh + s, lane, j)] =
                                (int32_t)(layers_[l].off + (32 * mt + r) * W + kperm(s, h, j));
                            sb[slot((l - 1) * mt_n * ksh + mt * ksh + s, lane, j)] =
                                (int32_t)(layers_[l].off + kperm(s, h, j) * W + (32 * mt + r));
                        }
                    const int k = 8 * h + j;
                    if (k < 3 && row_ok) sb[slot((D - 1) * mt_n * ksh + mt, lane, j)] = (int32_t)(layers_[D].off + k * W + (32 * mt + r));
                }
                for (int s = 0; s < ksh; s++) {
                    if (kperm(s, h, j) >= W) continue;
                    if (r < 3) sf[slot(out_base + s, lane, j)] = (int32_t)(layers_[D].off + r * W + kperm(s, h, j));
                    if (hash_) sb[slot(din_base + s, lane, j)] = (int32_t)(layers_[0].off + kperm(s, h, j) * E + r);
                }
            }
        }
        enc80_generic_ = !fused_ && !hash_ && cfg.pos_id == 3 && cfg.dir_id == 0;
        if (enc80_generic_) {
            si = sf;
            for (int lane = 0; lane < 64; lane++)
                for (int j = 0; j < 8; j++)
                    for (int mt = 0; mt < mt_n; mt++)
                        for (int s = 0; s < ks0; s++)
                            if (32 * mt + (lane & 31) < W)
                                si[slot(mt * ks0 + s, lane, j)] = (int32_t)(layers_[0].off + (32 * mt + (lane & 31)) * E + fmap80(s, lane >> 5, j));
        }
        fused_opt_ = !no_fused_opt;
        if (fused_opt_) {
            dst.assign((size_t)3 * n_mlp_, -1);
            auto invert = [&](const int32_t* src, size_t n_slots, int32_t* out) {
                for (size_t j = 0; j < n_slots; j++) {
                    if (src[j] < 0) continue;
                    if ((uint32_t)src[j] >= n_mlp_ || out[src[j]] >= 0) { fused_opt_ = false; return; }
                    out[src[j]] = (int32_t)j;
                }
            };
            const std::vector<int32_t>& si_host = enc80_generic_ ? si : sf;      // (what the parent read back from the device)
            invert(sf.data(), sf.size(), dst.data());
            if (fused_opt_) invert(si_host.data(), si_host.size(), dst.data() + n_mlp_);
            if (fused_opt_) invert(sb.data(), sb.size(), dst.data() + 2 * (size_t)n_mlp_);
            if (!fused_opt_) dst.clear();
        }

        // Mlp::build_wgrad_tasks
        {
            const uint32_t Dd = depth_;
            for (uint32_t l = 0; l <= Dd; l++) {
                const Layer& L = layers_[l];
                const uint32_t a_rows = l == Dd ? Dd * kw_ : l * kw_;
                const uint32_t b_rows = l == 0 ? 0 : enc_dims_ + (l - 1) * kw_;
                for (uint32_t mt = 0; mt * 32 < L.out; mt++)
                    for (uint32_t n0 = 0; n0 * 32 < L.in; n0 += 4) {
                        Task T;
                        const uint32_t tiles_left = (L.in - 32 * n0 + 31) / 32;
                        T.n_tiles = tiles_left < 4u ? tiles_left : 4u;
                        T.a_row0 = a_rows + 32 * mt;
                        T.b_row0 = b_rows + 32 * n0;
                        T.m_valid = L.out - 32 * mt < 32 ? L.out - 32 * mt : 32;
                        const uint32_t last0 = 32 * (n0 + T.n_tiles - 1);
                        T.n_valid_last = L.in - last0 < 32 ? L.in - last0 : 32;
                        T.param_off = L.off + 32 * mt * L.in + 32 * n0;
                        T.in_dim = L.in;
                        T.pad = 0;
                        tasks.push_back(T);
                    }
            }
        }
        // the tile loop of Mlp::ensure_train_workspace
        {
            const uint32_t Dd = depth_;
            for (uint32_t l = 0; l <= Dd; l++) {
                const Layer& L = layers_[l];
                const uint32_t a_rows = l == Dd ? Dd * kw_ : l * kw_;
                const uint32_t b_rows = l == 0 ? 0 : enc_dims_ + (l - 1) * kw_;
                for (uint32_t mt = 0; mt * 32 < L.out; mt++)
                    for (uint32_t nt = 0; nt * 32 < L.in; nt++) {
                        Tile T;
                        T.a_row0 = a_rows + 32 * mt;
                        T.b_row0 = b_rows + 32 * nt;
                        T.m_valid = L.out - 32 * mt < 32 ? L.out - 32 * mt : 32;
                        T.n_valid = L.in - 32 * nt < 32 ? L.in - 32 * nt : 32;
                        T.param_off = L.off + 32 * mt * L.in + 32 * nt;
                        T.in_dim = L.in;
                        tiles.push_back(T);
                    }
            }
        }
    }
};

// Mlp::wgrad_chunk
static uint32_t wgrad_chunk(uint32_t n, int n_wgrad_tasks_, int num_cus, bool wgrad_old_)
{
    if (wgrad_old_) return 128u;
    const uint32_t wg_per_chunk = ceil_div((uint32_t)n_wgrad_tasks_, 4u);
    uint32_t chunks = std::max(1u, 2u * (uint32_t)num_cus / std::max(1u, wg_per_chunk));
    uint32_t c = ceil_div(ceil_div(n, chunks), 32u) * 32u;
    return std::max(c, 64u);
}
// the max_chunks line of Mlp::ensure_train_workspace
static uint32_t max_chunks(uint32_t n, int n_wgrad_tasks_, int num_cus, bool wgrad_old_)
{
    return wgrad_old_ ? ceil_div(n, 128u)
                      : std::max(ceil_div(n, wgrad_chunk(n, n_wgrad_tasks_, num_cus, wgrad_old_)), std::max(1u, 2u * (uint32_t)num_cus / std::max(1u, ceil_div((uint32_t)n_wgrad_tasks_, 4u))));
}

// the bin-plan loop of Mlp::ensure_train_workspace and the assembly loop of Mlp::backward
struct Bins {
    uint32_t grid_bin_first_[16] = {}, grid_bin_count_[16] = {}, grid_bin_cap_[16] = {}, grid_list0_[16] = {}, grid_bins_total_ = 0;
    std::vector<uint32_t> info;
    size_t pairs = 0;
    uint32_t loose_first[16], loose_count[16], loose_n = 0, loose_chunks = 0;
    Bins(const uint32_t* hg_off_, uint32_t n, bool no_bins)
    {
        const uint32_t GB_BIN = 2048, GB_MIN_BINS = 8, GB_MAX_BINS = 512;
        for (uint32_t l = 0; l < 16; l++) {
            const uint32_t cnt = hg_off_[l + 1] - hg_off_[l];
            const uint32_t bins = (cnt % GB_BIN == 0u) ? cnt / GB_BIN : 0u;
            grid_bin_first_[l] = grid_bins_total_;
            grid_bin_count_[l] = (bins >= GB_MIN_BINS && bins <= GB_MAX_BINS && !no_bins) ? bins : 0u;
            grid_bin_cap_[l] = grid_bin_count_[l] ? std::max(1024u, (uint32_t)std::min<uint64_t>(2ull * n * 8ull / grid_bin_count_[l], 1u << 24)) : 0u;
            grid_list0_[l] = (uint32_t)pairs;
            for (uint32_t b = 0; b < grid_bin_count_[l]; b++) {
                info.insert(info.end(), {hg_off_[l] + b * GB_BIN, (uint32_t)(pairs + (size_t)b * grid_bin_cap_[l]), grid_bin_cap_[l], 0u});
            }
            pairs += (size_t)grid_bin_count_[l] * grid_bin_cap_[l];
            grid_bins_total_ += grid_bin_count_[l];
        }
        if (pairs > 0xffffffffull) fail("train batch too large for the table gradient's bin lists");
        for (uint32_t l = 0; l < 16; l++) {
            if (grid_bin_count_[l] == 0u) {
                loose_first[loose_n] = hg_off_[l];
                loose_count[loose_n] = hg_off_[l + 1] - hg_off_[l];
                loose_chunks += ceil_div(loose_count[loose_n], GB_BIN);
                loose_n++;
            }
        }
        for (uint32_t r = loose_n; r < 16; r++) loose_first[r] = loose_count[r] = 0u;
    }
};

// lds of k_train_gen and lds2 of k_train_gen2 in Mlp::backward (KG_SCRATCH = 16 * 40 * 2)
static size_t lds(uint32_t kw_, uint32_t depth_, uint32_t waves)
{
    const int mtg = (int)kw_ / 32, ksg = (int)kw_ / 16;
    const size_t v = (size_t)2 * mtg * (ksg > 5 ? ksg : 5) * 1024 + waves * (1280 + (size_t)depth_ * 512);
    if (v > 160 * 1024) fail("network too deep for the training kernel's LDS budget");
    return v;
}
static size_t lds2(uint32_t kw_, uint32_t depth_, uint32_t sgn, int nt)
{
    const int ksg = (int)kw_ / 16;
    const size_t v = (size_t)2 * sgn * nt * ksg * 1024 + 4 * 1280 + (size_t)4 * depth_ * nt * 256;
    if (v > 160 * 1024) fail("network too deep for the training kernel's LDS budget");
    return v;
}

}  // namespace ref

// ================================================================================================ the plan against the reference
template <class A, class B>
static bool same_bytes(const std::vector<A>& a, const std::vector<B>& b)
{
    static_assert(sizeof(A) == sizeof(B), "layouts");
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(A)) == 0);
}

static void compare_model(const nrc_config& cfg, bool with_init)
{
    g_what = describe(cfg);
    const ref::Model R(cfg, with_init, false);
    const MlpPlan p = make_mlp_plan(cfg);
    CHECK(p.width == R.width_ && p.kw == R.kw_ && p.depth == R.depth_ && p.enc_dims == R.enc_dims_ && p.loss_id == R.loss_id_);
    CHECK(p.sgd == R.sgd_ && p.fused == R.fused_ && p.hash == R.hash_ && p.enc80_generic == R.enc80_generic_);
    CHECK(p.n_mlp == R.n_mlp_ && p.n_grid_entries == R.n_grid_entries_ && p.n_params == R.n_params_);
    CHECK(std::memcmp(p.hg_off, R.hg_off_, sizeof p.hg_off) == 0);
    CHECK(same_bytes(p.layers, R.layers_));
    CHECK(tcnn_param_count(p) == R.n_params_ + 13u * R.width_);

    const FragMaps m = make_frag_maps(p);
    CHECK(m.n_frag_fwd == R.n_frag_fwd_ && m.n_frag_bwd == R.n_frag_bwd_);
    CHECK(m.fwd == R.sf);
    CHECK(m.bwd == R.sb);
    CHECK(m.inf_own == R.si);
    CHECK(R.enc80_generic_ ? &m.inf() == &m.inf_own : &m.inf() == &m.fwd);
    CHECK(invert_frag_maps(m.fwd, m.inf(), m.bwd, p.n_mlp, false) == R.dst);
    CHECK(R.fused_opt_ && R.dst.size() == (size_t)3 * p.n_mlp);
    CHECK(invert_frag_maps(m.fwd, m.inf(), m.bwd, p.n_mlp, true).empty());

    const WgradLists lists = make_wgrad_lists(p);
    CHECK(same_bytes(lists.tiles, R.tiles));
    CHECK(same_bytes(lists.tasks, R.tasks));
    const uint32_t n_tasks = (uint32_t)R.tasks.size();
    for (uint32_t cus : {1u, 8u, 256u, 304u})
        for (int old = 0; old < 2; old++)
            for (uint32_t n : {32u, 64u, 96u, 1024u, 2048u, 4096u, 16384u, 40992u, 1u << 20}) {
                CHECK(wgrad_chunk(n, n_tasks, cus, old != 0) == ref::wgrad_chunk(n, (int)n_tasks, (int)cus, old != 0));
                CHECK(wgrad_max_chunks(n, n_tasks, cus, old != 0) == ref::max_chunks(n, (int)n_tasks, (int)cus, old != 0));
            }
    for (uint32_t waves : {4u, 8u}) {
        size_t a = 0, b = 0;
        const std::string fa = failure_of([&] { a = train_gen_lds(p.kw, p.depth, waves); }), fb = failure_of([&] { b = ref::lds(R.kw_, R.depth_, waves); });
        CHECK(fa == fb && a == b);
    }
    for (int nt = 1; nt <= 2; nt++) {
        const uint32_t sgn = 4u / (p.kw / 32u);
        size_t a = 0, b = 0;
        const std::string fa = failure_of([&] { a = train_gen2_lds(p.kw, p.depth, sgn, nt); }), fb = failure_of([&] { b = ref::lds2(R.kw_, R.depth_, sgn, nt); });
        CHECK(fa == fb && a == b);
    }
    if (with_init) {
        const MlpInit init = mlp_initial_params(p, cfg.seed);
        CHECK(same_bytes(init.w, R.w));
        CHECK(same_bytes(init.dead_rows, R.dead));
    }
}

static void compare_bins(const MlpPlan& p, uint32_t n, bool no_bins)
{
    const ref::Bins R(p.hg_off, n, no_bins);
    const GridBinPlan g = make_grid_bin_plan(p.hg_off, n, no_bins);
    CHECK(std::memcmp(g.bins.first, R.grid_bin_first_, 64) == 0 && std::memcmp(g.bins.count, R.grid_bin_count_, 64) == 0);
    CHECK(std::memcmp(g.bins.cap, R.grid_bin_cap_, 64) == 0 && std::memcmp(g.bins.list0, R.grid_list0_, 64) == 0);
    CHECK(g.bins_total == R.grid_bins_total_ && g.pairs == R.pairs && g.info == R.info);
    CHECK(g.loose.n == R.loose_n && g.loose_chunks == R.loose_chunks);
    CHECK(std::memcmp(g.loose.first, R.loose_first, 64) == 0 && std::memcmp(g.loose.count, R.loose_count, 64) == 0);
}

// ================================================================================================ properties
// every parameter of `expect` (a count per parameter) occurs that often in the map; nothing else does
static void check_map_counts(const std::vector<int32_t>& map, const std::vector<int>& expect)
{
    std::vector<int> seen(expect.size(), 0);
    bool in_range = true;
    for (int32_t s : map) {
        if (s < 0) continue;
        if ((size_t)s >= expect.size()) { in_range = false; continue; }
        seen[(size_t)s]++;
    }
    CHECK(in_range);
    CHECK(seen == expect);
}

static void map_properties(const nrc_config& cfg)
{
    g_what = describe(cfg);
    const MlpPlan p = make_mlp_plan(cfg);
    const FragMaps m = make_frag_maps(p);
    CHECK(m.fwd.size() == (size_t)m.n_frag_fwd * 512 && m.bwd.size() == (size_t)m.n_frag_bwd * 512);
    // every element (row < out, col < in) of every layer: once in the forward map, once in the inference map; in the backward map every layer
    // but the first, and of the first the encoded dims 0..31 (the table's features) of a model with a table
    std::vector<int> once(p.n_mlp, 1), back(p.n_mlp, 1);
    const MlpLayer& L0 = p.layers[0];
    for (uint32_t row = 0; row < L0.out; row++)
        for (uint32_t col = 0; col < L0.in; col++) back[L0.off + row * L0.in + col] = p.hash && col < 32u ? 1 : 0;
    uint32_t total = 0;
    for (const MlpLayer& L : p.layers) { CHECK(L.off == total); total += L.out * L.in; }
    CHECK(total == p.n_mlp);
    check_map_counts(m.fwd, once);
    check_map_counts(m.inf(), once);
    check_map_counts(m.bwd, back);
    // the inference image: layer 0's column of slot (s, h, j) is the in-kernel encoder's, everything else is the forward image
    if (p.enc80_generic || p.fused) {
        const std::vector<int32_t>& inf = m.inf();
        const int ks0 = (int)p.enc_dims / 16, mt_n = (int)p.kw / 32;
        bool ok = true;
        for (size_t i = 0; i < inf.size(); i++) {
            const int frag = (int)(i / 512), lane = (int)(i / 8 % 64), j = (int)(i % 8);
            if (frag >= mt_n * ks0) { ok = ok && inf[i] == m.fwd[i]; continue; }
            const int s = frag % ks0, h = lane >> 5, row = 32 * (frag / ks0) + (lane & 31);
            const int col = s < 4 ? 16 * s + 8 * h + j : (j < 4 ? 64 + 4 * h + j : 72 + 4 * h + j - 4);
            ok = ok && inf[i] == (row < (int)p.width ? row * (int)p.enc_dims + col : -1);      // (rows beyond a 16-wide model: zero)
        }
        CHECK(ok);
    }
    // the inversion: dst[k][src_k[j]] == j, and -1 where the image does not hold the parameter
    const std::vector<int32_t> dst = invert_frag_maps(m.fwd, m.inf(), m.bwd, p.n_mlp, false);
    CHECK(dst.size() == (size_t)3 * p.n_mlp);
    if (dst.size() == (size_t)3 * p.n_mlp) {
        const std::vector<int32_t>* src[3] = {&m.fwd, &m.inf(), &m.bwd};
        for (int k = 0; k < 3; k++) {
            bool ok = true;
            size_t held = 0;
            for (size_t j = 0; j < src[k]->size(); j++)
                if ((*src[k])[j] >= 0) { ok = ok && dst[(size_t)k * p.n_mlp + (size_t)(*src[k])[j]] == (int32_t)j; held++; }
            size_t placed = 0;
            for (uint32_t i = 0; i < p.n_mlp; i++) placed += dst[(size_t)k * p.n_mlp + i] >= 0;
            CHECK(ok && placed == held);
        }
    }
    // not one-to-one: a parameter twice, a parameter out of range -- in any of the three images
    for (int k = 0; k < 3; k++) {
        std::vector<int32_t> maps[3] = {m.fwd, m.inf(), m.bwd};
        size_t a = 0, b = 0;
        while (maps[k][a] < 0) a++;
        for (b = a + 1; maps[k][b] < 0;) b++;
        const int32_t keep = maps[k][b];
        maps[k][b] = maps[k][a];
        CHECK(invert_frag_maps(maps[0], maps[1], maps[2], p.n_mlp, false).empty());
        maps[k][b] = (int32_t)p.n_mlp;
        CHECK(invert_frag_maps(maps[0], maps[1], maps[2], p.n_mlp, false).empty());
        maps[k][b] = keep;
        CHECK(!invert_frag_maps(maps[0], maps[1], maps[2], p.n_mlp, false).empty());
    }
}

struct Seen { bool m16 = false, m3 = false, n16 = false, last16 = false; };
static void list_properties(const nrc_config& cfg, Seen& seen)
{
    g_what = describe(cfg);
    const MlpPlan p = make_mlp_plan(cfg);
    const WgradLists lists = make_wgrad_lists(p);
    const uint32_t rows_d = p.depth * p.kw + 8, rows_a = p.enc_dims + p.depth * p.kw;      // what k_wgrad / k_wgrad2 are launched with
    // a rectangle {param_off, rows, first column block .., columns} covers its cells of the layer that holds param_off
    std::vector<int> by_tiles(p.n_mlp, 0), by_tasks(p.n_mlp, 0);
    auto cover = [&](std::vector<int>& cells, uint32_t param_off, uint32_t in_dim, uint32_t rows, uint32_t cols) {
        const MlpLayer* L = nullptr;
        for (const MlpLayer& c : p.layers)
            if (param_off >= c.off && param_off < c.off + c.out * c.in) L = &c;
        CHECK(L != nullptr && L->in == in_dim);
        if (L == nullptr) return;
        const uint32_t row0 = (param_off - L->off) / L->in, col0 = (param_off - L->off) % L->in;
        CHECK(row0 % 32 == 0 && col0 % 32 == 0 && row0 + rows <= L->out && col0 + cols <= L->in);
        if (row0 + rows > L->out || col0 + cols > L->in) return;
        for (uint32_t r = 0; r < rows; r++)
            for (uint32_t c = 0; c < cols; c++) cells[L->off + (row0 + r) * L->in + col0 + c]++;
    };
    for (const WgradTile& T : lists.tiles) {
        CHECK(T.m_valid >= 1 && T.m_valid <= 32 && T.n_valid >= 1 && T.n_valid <= 32);
        CHECK(T.a_row0 + T.m_valid <= rows_d && T.b_row0 + T.n_valid <= rows_a);      // (the delta buffer has 8 rows behind the last hidden layer: the output's)
        cover(by_tiles, T.param_off, T.in_dim, T.m_valid, T.n_valid);
        seen.m16 |= T.m_valid == 16; seen.m3 |= T.m_valid == 3; seen.n16 |= T.n_valid == 16;
    }
    for (const WgradTask& T : lists.tasks) {
        CHECK(T.n_tiles >= 1 && T.n_tiles <= (uint32_t)WGRAD2_NTL && T.n_valid_last >= 1 && T.n_valid_last <= 32 && T.pad == 0);
        CHECK(T.a_row0 + T.m_valid <= rows_d && T.b_row0 + 32 * (T.n_tiles - 1) + T.n_valid_last <= rows_a);
        cover(by_tasks, T.param_off, T.in_dim, T.m_valid, 32 * (T.n_tiles - 1) + T.n_valid_last);
        seen.last16 |= T.n_valid_last == 16;
    }
    CHECK(by_tiles == std::vector<int>(p.n_mlp, 1));
    CHECK(by_tasks == std::vector<int>(p.n_mlp, 1));
}

// the bound d_slabs_ rests on: a workspace sized for n holds the slabs of every batch up to n
static void slab_property(uint32_t n_tasks, uint32_t cus, bool old, uint32_t n, uint32_t step)
{
    const uint32_t cap = wgrad_max_chunks(n, n_tasks, cus, old);
    bool fits = true, shaped = true;
    for (uint32_t m = 32; m <= n; m += step) {
        const uint32_t chunk = wgrad_chunk(m, n_tasks, cus, old);
        fits = fits && (m + chunk - 1) / chunk <= cap;
        shaped = shaped && chunk % 32 == 0 && chunk >= 64;
    }
    g_what = "tasks " + std::to_string(n_tasks) + " cus " + std::to_string(cus) + " old " + std::to_string(old) + " n " + std::to_string(n);
    CHECK(fits);
    CHECK(shaped);
}

static void bin_properties(uint32_t log2, uint32_t n)
{
    g_what = "log2 " + std::to_string(log2) + " n " + std::to_string(n);
    const MlpPlan p = make_mlp_plan(make_cfg(0, 0, 64, 2, log2));
    const GridBinPlan g = make_grid_bin_plan(p.hg_off, n, false);
    // bins in level order, lists back to back without overlap, their total the pair count; every level either binned or loose
    size_t next_pair = 0;
    uint32_t bin = 0, loose = 0, chunks = 0;
    bool ok = g.info.size() == (size_t)g.bins_total * 4;
    for (uint32_t l = 0; l < HG_LEVELS && ok; l++) {
        const uint32_t first = p.hg_off[l], cnt = p.hg_off[l + 1] - p.hg_off[l];
        if (g.bins.count[l] == 0) {
            ok = ok && loose < g.loose.n && g.loose.first[loose] == first && g.loose.count[loose] == cnt && g.bins.cap[l] == 0;
            chunks += (cnt + GB_BIN - 1) / GB_BIN;
            loose++;
            continue;
        }
        ok = ok && g.bins.count[l] * GB_BIN == cnt && g.bins.first[l] == bin && g.bins.list0[l] == next_pair && g.bins.cap[l] >= 1024u;
        for (uint32_t b = 0; b < g.bins.count[l] && ok; b++, bin++) {
            const uint32_t* info = &g.info[(size_t)bin * 4];
            ok = ok && info[0] == first + b * GB_BIN && info[1] == next_pair && info[2] == g.bins.cap[l] && info[3] == 0;
            next_pair += info[2];
        }
    }
    CHECK(ok);
    CHECK(bin == g.bins_total && loose == g.loose.n && chunks == g.loose_chunks && next_pair == g.pairs && g.pairs <= 0xffffffffull);
    const GridBinPlan none = make_grid_bin_plan(p.hg_off, n, true);
    CHECK(none.bins_total == 0 && none.pairs == 0 && none.info.empty() && none.loose.n == HG_LEVELS);
    bool all_loose = true;
    for (uint32_t l = 0; l < HG_LEVELS; l++)
        all_loose = all_loose && none.bins.count[l] == 0 && none.loose.first[l] == p.hg_off[l] && none.loose.count[l] == p.hg_off[l + 1] - p.hg_off[l];
    CHECK(all_loose);
}

static void write_floats(const std::string& path, const std::vector<float>& v)
{
    std::FILE* f = std::fopen(path.c_str(), "wb");
    CHECK(f != nullptr);
    if (f == nullptr) return;
    CHECK(std::fwrite(v.data(), sizeof(float), v.size(), f) == v.size());
    std::fclose(f);
}

int main(int argc, char** argv)
{
    const uint32_t widths[] = {16, 32, 64, 128}, depths[] = {1, 2, 6, 8, 16};

    begin_case("every model shape against the parent's host code");
    for (uint32_t w : widths)
        for (uint32_t d : depths)
            for (uint32_t pos = 0; pos < 4; pos++)
                for (uint32_t dir = 0; dir < 3; dir++) compare_model(make_cfg(pos, dir, w, d, pos == 0 ? (w == 64 ? 12 : 4) : 0, d == 2 ? "L2" : "LogL1", d == 1 ? "SGD" : "Adam", 7 + d), true);
    compare_model(make_cfg(3, 0, 64, 6), true);       // fused
    compare_model(make_cfg(3, 0, 128, 8), true);      // enc80_generic
    compare_model(make_cfg(1, 1, 64, 6), true);       // enc_dims 16
    {
        const MlpPlan fused = make_mlp_plan(make_cfg(3, 0, 64, 6)), c5 = make_mlp_plan(make_cfg(3, 0, 128, 8)), e16 = make_mlp_plan(make_cfg(1, 1, 64, 6));
        CHECK(fused.fused && !fused.enc80_generic && fused.enc_dims == 80 && fused.n_params == 25792);
        CHECK(!c5.fused && c5.enc80_generic && c5.enc_dims == 80);
        CHECK(e16.enc_dims == 16 && !e16.fused && !e16.enc80_generic && !e16.hash);
        const char* names[] = {"RelativeL2Luminance", "L2", "RelativeL2", "L1", "Mape", "Smape", "LogL1"};
        for (uint32_t i = 0; i < 7; i++) CHECK(make_mlp_plan(make_cfg(3, 0, 64, 6, 0, names[i])).loss_id == i);
    }

    begin_case("table offsets and bin plans against the parent's loops");
    for (uint32_t log2 : {4u, 12u, 14u, 15u, 19u, 24u, 0u}) {
        const nrc_config cfg = make_cfg(0, 0, 64, 2, log2);
        compare_model(cfg, log2 == 4 || log2 == 12);
        const MlpPlan p = make_mlp_plan(cfg);
        for (uint32_t n : {32u, 256u, 2048u, 4096u, 16384u, 1u << 20})
            for (int no_bins = 0; no_bins < 2; no_bins++) {
                g_what = describe(cfg) + " n " + std::to_string(n);
                compare_bins(p, n, no_bins != 0);
            }
    }

    begin_case("invalid configurations fail with the parent's texts");
    {
        nrc_config bad[] = {make_cfg(3, 0, 48, 6), make_cfg(3, 0, 64, 0), make_cfg(3, 0, 64, 17), make_cfg(3, 0, 64, 6, 0, "RelativeL2Luminance", "Lion"),
                            make_cfg(3, 0, 64, 6, 0, "CrossEntropy"), make_cfg(4, 0, 64, 6), make_cfg(3, 3, 64, 6), make_cfg(7, 9, 48, 0), make_cfg(0, 0, 64, 6, 3),
                            make_cfg(0, 0, 64, 6, 25), make_cfg(3, 0, 48, 17, 0, "Nope", "Nope"), make_cfg(0, 0, 64, 0, 25, "Nope")};
        const char* starts[] = {"nnWidth must be 16, 32, 64 or 128", "nnDepth must be in 1..16 (got 0)", "nnDepth must be in 1..16 (got 17)", "unsupported optimizer Lion",
                                "unsupported loss CrossEntropy", "NNEncodingConfig posID/dirID is invalid", "NNEncodingConfig posID/dirID is invalid",
                                "NNEncodingConfig posID/dirID is invalid", "hashgrid_log2_size must be in 4..24", "hashgrid_log2_size must be in 4..24",
                                "nnWidth must be", "nnDepth must be"};
        for (size_t i = 0; i < sizeof bad / sizeof bad[0]; i++) {
            g_what = describe(bad[i]);
            const std::string a = failure_of([&] { make_mlp_plan(bad[i]); }), b = failure_of([&] { ref::Model(bad[i], false, false); });
            CHECK(!a.empty() && a == b);
            CHECK(a.find(std::string("SkyRenderer ERROR: ") + starts[i]) == 0);
        }
        // the LDS budget: no depth of 1..16 exceeds it (the guard is for a wider range of depths); 32 and 64 layers of 128 would
        g_what = "LDS budget";
        const std::string too_deep = "SkyRenderer ERROR: network too deep for the training kernel's LDS budget";
        CHECK(failure_of([&] { train_gen_lds(128, 32, 8); }) == too_deep && failure_of([&] { ref::lds(128, 32, 8); }) == too_deep);
        CHECK(failure_of([&] { train_gen2_lds(128, 64, 1, 2); }) == too_deep && failure_of([&] { ref::lds2(128, 64, 1, 2); }) == too_deep);
        CHECK(failure_of([&] { train_gen_lds(128, 16, 8); }).empty() && failure_of([&] { train_gen2_lds(128, 16, 1, 2); }).empty());
    }

    begin_case("maps: every matrix element once, inversion exactly when one-to-one");
    for (uint32_t w : widths)
        for (uint32_t d : {1u, 2u, 6u, 16u})
            for (uint32_t pos = 0; pos < 4; pos++) map_properties(make_cfg(pos, pos % 3, w, d, pos == 0 ? 4 : 0));
    map_properties(make_cfg(3, 0, 64, 6));
    map_properties(make_cfg(3, 0, 128, 8));
    map_properties(make_cfg(1, 1, 64, 6));
    for (int s = 0; s < 5; s++)
        for (int h = 0; h < 2; h++)
            for (int j = 0; j < 8; j++) {
                CHECK(fmap80(s, h, j) == ref::fmap80(s, h, j));
                CHECK(kperm(s, h, j) == 16 * s + ((j >> 2) << 3) + (h << 2) + (j & 3));
            }

    begin_case("tiles and tasks partition every layer's matrix");
    {
        Seen seen;
        for (uint32_t w : widths)
            for (uint32_t d : depths)
                for (uint32_t pos = 0; pos < 4; pos++) list_properties(make_cfg(pos, pos % 3, w, d, pos == 0 ? 4 : 0), seen);
        list_properties(make_cfg(3, 0, 64, 6), seen);
        list_properties(make_cfg(3, 0, 128, 8), seen);
        list_properties(make_cfg(1, 1, 64, 6), seen);
        g_what = "edge shapes seen";
        CHECK(seen.m16 && seen.m3 && seen.n16 && seen.last16);
    }

    begin_case("slabs: a workspace sized for n holds every smaller batch");
    for (uint32_t n_tasks : {(uint32_t)make_wgrad_lists(make_mlp_plan(make_cfg(3, 0, 64, 6))).tasks.size(), (uint32_t)make_wgrad_lists(make_mlp_plan(make_cfg(3, 0, 128, 8))).tasks.size(),
                             (uint32_t)make_wgrad_lists(make_mlp_plan(make_cfg(1, 1, 16, 1))).tasks.size(), (uint32_t)make_wgrad_lists(make_mlp_plan(make_cfg(3, 0, 128, 16))).tasks.size()})
        for (uint32_t cus : {1u, 8u, 256u, 304u})
            for (int old = 0; old < 2; old++) {
                for (uint32_t n = 32; n <= 4096; n += 32) slab_property(n_tasks, cus, old != 0, n, 32);
                slab_property(n_tasks, cus, old != 0, 16384, 32);
                slab_property(n_tasks, cus, old != 0, 1u << 20, 32);
            }

    begin_case("bin plan: disjoint lists, every level binned or loose, the pair-count limit");
    for (uint32_t log2 : {4u, 12u, 14u, 15u, 19u, 24u})
        for (uint32_t n : {32u, 256u, 1024u, 4096u, 16384u, 1u << 20}) bin_properties(log2, n);
    {
        g_what = "log2 14";
        const MlpPlan p = make_mlp_plan(make_cfg(0, 0, 64, 2, 14));
        const GridBinPlan g = make_grid_bin_plan(p.hg_off, 256, false), grown = make_grid_bin_plan(p.hg_off, 4096, false);
        bool ok = g.bins.count[0] == 0 && g.loose.n == 1 && g.loose.first[0] == 0 && g.loose.count[0] == 4096 && g.loose_chunks == 2;
        for (uint32_t l = 1; l < HG_LEVELS; l++) ok = ok && g.bins.count[l] == 8 && g.bins.cap[l] == 1024 && grown.bins.cap[l] == 8192;
        CHECK(ok && g.bins_total == 120 && g.pairs == (size_t)120 * 1024);
        // the limit: the lists hold sum over the binned levels of count * clamp(16 n / count, 1024, 2^24) pairs, at most 2^32 - 1
        const MlpPlan q = make_mlp_plan(make_cfg(0, 0, 64, 2, 19));
        auto pairs_of = [&](uint64_t n) {
            uint64_t pairs = 0;
            for (uint32_t l = 0; l < HG_LEVELS; l++) {
                const uint64_t cnt = q.hg_off[l + 1] - q.hg_off[l], bins = cnt / 2048;
                if (cnt % 2048 == 0 && bins >= 8 && bins <= 512) pairs += bins * std::min<uint64_t>(std::max<uint64_t>(16 * n / bins, 1024), 1u << 24);
            }
            return pairs;
        };
        uint64_t lo = 32, hi = 0xffffffe0ull;      // pairs_of is monotone: the smallest multiple of 32 beyond the limit
        CHECK(pairs_of(lo) <= 0xffffffffull && pairs_of(hi) > 0xffffffffull);
        while (hi - lo > 32) {
            const uint64_t mid = (lo + hi) / 64 * 32;
            (pairs_of(mid) > 0xffffffffull ? hi : lo) = mid;
        }
        g_what = "limit at n " + std::to_string(hi);
        CHECK(hi > (1u << 24) && hi < (1u << 25));      // 15 binned levels of about 16 n pairs each
        CHECK(failure_of([&] { make_grid_bin_plan(q.hg_off, (uint32_t)lo, false); }).empty());
        CHECK(failure_of([&] { make_grid_bin_plan(q.hg_off, (uint32_t)hi, false); }) == "SkyRenderer ERROR: train batch too large for the table gradient's bin lists");
        CHECK(failure_of([&] { ref::Bins(q.hg_off, (uint32_t)hi, false); }) == failure_of([&] { make_grid_bin_plan(q.hg_off, (uint32_t)hi, false); }));
        CHECK(failure_of([&] { make_grid_bin_plan(q.hg_off, (uint32_t)hi, true); }).empty());
    }

    begin_case("tiny-cuda-nn layout: round trip with the dead rows, dumps for the oracle comparison");
    {
        struct Dump { const char* name; nrc_config cfg; };
        const Dump dumps[] = {{"6x64", make_cfg(3, 0, 64, 6)}, {"8x128", make_cfg(3, 0, 128, 8)}, {"1x16", make_cfg(3, 0, 16, 1)}, {"hashgrid12", make_cfg(0, 0, 64, 3, 12)}};
        for (const Dump& d : dumps)
            for (uint32_t seed : {1337u, 7u}) {
                g_what = std::string(d.name) + " seed " + std::to_string(seed);
                const MlpPlan p = make_mlp_plan(d.cfg);
                const MlpInit init = mlp_initial_params(p, seed);
                CHECK(init.w.size() == p.n_params && init.dead_rows.size() == 13u * p.width);
                std::vector<float> tcnn(tcnn_param_count(p), -1.0f), own(p.n_params, -2.0f), dead(init.dead_rows.size(), -3.0f);
                to_tcnn_layout(p, init.dead_rows.data(), init.w.data(), tcnn.data());
                from_tcnn_layout(p, dead.data(), tcnn.data(), own.data());
                CHECK(same_bytes(own, init.w) && same_bytes(dead, init.dead_rows));
                CHECK(std::memcmp(tcnn.data() + p.n_mlp, init.dead_rows.data(), dead.size() * 4) == 0);
                CHECK(p.n_params == p.n_mlp || std::memcmp(tcnn.data() + p.n_mlp + dead.size(), init.w.data() + p.n_mlp, (size_t)(p.n_params - p.n_mlp) * 4) == 0);
                // the gradient's dead rows: zero on the way out, dropped on the way in
                std::vector<float> grad(tcnn.size(), 5.0f), back(p.n_params, 0.0f);
                to_tcnn_layout(p, nullptr, init.w.data(), grad.data());
                CHECK(std::count(grad.begin() + p.n_mlp, grad.begin() + p.n_mlp + (long)dead.size(), 0.0f) == (long)dead.size());
                from_tcnn_layout(p, nullptr, grad.data(), back.data());
                CHECK(same_bytes(back, init.w));
                if (argc > 1) {
                    const std::string base = std::string(argv[1]) + "/" + d.name + "_" + std::to_string(seed);
                    write_floats(base + "_w.f32", init.w);
                    write_floats(base + "_tcnn.f32", tcnn);
                }
            }
    }

    std::printf("mlp_plan: %d cases, %d checks\n", g_cases, g_checks);
    if (g_failed) std::printf("FAILED: %d checks\n", g_failed);
    return g_failed ? 1 : 0;
}
