// nrc_mlp.hpp -- the neural radiance cache arithmetic on gfx950: fused input encoding + fully fused MLP
// (inference), forward+loss+backward, split-K weight gradients, EMA{Adam}.  Replaces what the reference gets
// from tiny-cuda-nn v1.6 through tcnn::create_from_config / network->inference / trainer->training_step
// (src/NeuralRadianceCache.cu:16-39,142,153-154).
#pragma once
#include <vector>

#include "nrc_common.hpp"
#include "nrc_mlp_plan.hpp"      // the device-free half: MlpPlan and everything computed from it (tests/test_mlp_plan_host.py)

namespace nrc {

// The non-finite guard (include/nrc_hpm.h, nrc_cache_set_nonfinite_policy).  A pass that reads the final gradient stores `stamp` into
// words[0] when a word of it, or the loss, is not finite; the optimizer kernels of the same step compare words[0] with `stamp` and turn
// their update into the identity on a match.  Every scan gets a stamp of its own, so the word is never cleared: a verdict that is not
// this step's does not match.  All writers of one scan store the same value (plain vector stores, no atomics).
struct GuardArgs {
    uint32_t* words = nullptr;                   // device: [0] stamp of the last bad scan, [1] skipped steps, [2] number of the last skipped step
    unsigned long long* host_cell = nullptr;     // host-mapped copy of {[1], [2]}, one 8-byte store per skipped step
    uint32_t stamp = 0, step = 0;
};
#if defined(__HIPCC__)
__device__ __forceinline__ bool guard_nonfinite(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) == 0x7f800000u; }
// every lane of the (one-dimensional) block calls it; the first lane that found something stores for its wave
__device__ __forceinline__ void guard_flag(bool bad, const GuardArgs& ga)
{
    const unsigned long long found = __ballot(bad);
    if (found != 0ull && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)found) - 1)) ga.words[0] = ga.stamp;
}
__device__ __forceinline__ bool guard_bad(const GuardArgs& ga) { return ga.words[0] == ga.stamp; }
// one thread of a bad step's first optimizer launch
__device__ __forceinline__ void guard_count(const GuardArgs& ga)
{
    const uint32_t skipped = ga.words[1] + 1u;
    ga.words[1] = skipped;
    ga.words[2] = ga.step;
    __hip_atomic_store(ga.host_cell, (unsigned long long)skipped | ((unsigned long long)ga.step << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
#endif

void mlp_set_wave_priority_raise(int on);      // nrc_common.hpp: NRC_RAISE_WAVE_PRIORITY's run-time switch, nrc_mlp.hip's kernels

class Mlp {
public:
    explicit Mlp(const nrc_config& cfg);
    Mlp(const Mlp&) = delete;
    Mlp& operator=(const Mlp&) = delete;

    // network->inference: y = MLP_ema(encode(x)); in [n][5], out [n][3] (device, fp32)
    // skip_zero_queries (renderer only): 32-sample tiles whose queries are all exactly zero store 0 without running the network
    // live_list / live_count (renderer only, with skip_zero_queries): the indices of the queries that are not all zero, in any order
    // (k_gen_rays writes them); a model whose encoder gathers from a table walks the list instead of testing every query
    // feat_slot: the generic models' feature buffer -- kInferSlot, or kSideSlot for a second inference caller that runs concurrently with
    // the first on another stream (the renderer's self-training tails on the training stream beside its render inference)
    static constexpr int kInferSlot = 0, kSideSlot = 4;
    void infer(const float* d_in, float* d_out, uint32_t n, bool use_ema, hipStream_t s, bool skip_zero_queries = false,
               const uint32_t* live_list = nullptr, const uint32_t* live_count = nullptr, int feat_slot = kInferSlot);
    // sizes kSideSlot's feature buffer for n EMA queries now (a buffer that grows later synchronises the device)
    void reserve_side_slot(uint32_t n) { if (!encodes_in_kernel()) ensure_features(n, kSideSlot); }
    // EMA inference encodes the raw queries inside the MLP kernel (no feature buffer sized by the launch)
    bool encodes_in_kernel() const { return plan_.fused || plan_.enc80_generic; }
    // forward (training weights) + loss + backward -> gradient vector (x loss_scale) and loss cell
    // widen_grid_grad (models with a trainable table): also write the table gradient into the fp32 gradient vector -- needed only
    // by readers of the vector (dense exchange, gradient hook, debug read-back); the optimizer reads the packed fp16 table itself
    // features_ready (generic models): the batch's fp16 features, encoded earlier by pre_encode -- backward() then launches no encoder
    void backward(const float* d_in, const float* d_target, uint32_t n, uint32_t n_norm, hipStream_t s, bool widen_grid_grad = true,
                  const void* features_ready = nullptr);
    // Encodings without trainable state (everything but HashGrid) do not depend on the weights: a caller that has the training inputs
    // before the training stream is free may encode them elsewhere (the renderer: on the train-ray stream, behind the rays).  Two
    // buffers of their own, by the caller's parity (not the one backward() encodes into: a step that encodes for itself may still be
    // reading that one); returns the features of the n samples at d_in.
    bool can_pre_encode() const { return !plan_.fused && !plan_.hash; }
    const void* pre_encode(const float* d_in, uint32_t n, int parity, hipStream_t s);
    // the gradient vector was written from outside (exchange result, hook, nrc_cache_set_params): it is what the optimizer reads
    void grad_vector_is_source() { grid16_valid_ = false; }
    // EMA{Adam} step + re-pack of the fp16 MFMA fragment images.  loss_cell (host-mapped, may be null): where the step's
    // {loss, loss_seq} pair is published; returns true when the step's own launch did that (k_opt_pack), false when the caller
    // still has to (models with a trainable encoding, NRC_DEBUG=no_fused_opt)
    bool optimizer_step(hipStream_t s, uint32_t loss_seq = 0, unsigned long long* loss_cell = nullptr);
    void repack(hipStream_t s);

    uint32_t n_params() const { return plan_.n_params; }
    uint32_t enc_dims() const { return plan_.enc_dims; }
    float* grad_ptr() { return d_grad_; }
    float* loss_ptr() { return d_loss_; }
    float* buffer(int which);    // 0 w, 1 ema, 2 m, 3 v, 4 grad
    // tiny-cuda-nn's own parameter layout (nrc_mlp_plan.hpp).  to / from convert a host vector of buffer `which` (0..3; the dead rows of
    // 4, the gradient, are zero); the dead rows are kept on the host as they were initialised / last set, so that a dump read back is the dump
    uint32_t tcnn_param_count() const { return nrc::tcnn_param_count(plan_); }
    void to_tcnn_layout(int which, const float* own, float* tcnn) const { nrc::to_tcnn_layout(plan_, dead_rows(which), own, tcnn); }
    void from_tcnn_layout(int which, const float* tcnn, float* own) { nrc::from_tcnn_layout(plan_, dead_rows(which), tcnn, own); }
    // sparse exchange of the HashGrid table gradient (nrc_mlp.hip, k_grid_pack): the gradient vector is
    // [n_mlp_params() matrix gradients][2 per table entry][2-word loss cell]
    bool has_grid() const { return plan_.hash; }
    uint32_t n_mlp_params() const { return plan_.n_mlp; }
    uint32_t grid_entries() const { return plan_.n_grid_entries; }
    uint32_t grid_list_capacity(uint32_t n_batch) const;
    static size_t grid_list_words(uint32_t cap) { return 2 + 2 * (size_t)cap; }
    void grid_grad_pack(uint32_t* d_list, uint32_t cap, hipStream_t s);
    void grid_grad_apply(const uint32_t* d_lists, uint32_t n_lists, uint32_t cap, hipStream_t s);
    uint32_t step = 0;
    static constexpr float kLossScale = 128.0f;

    // ---- non-finite guard (GuardArgs above).  Off (the default) nothing below is allocated, launched or read.
    void set_guard(bool on);
    bool guard_on() const { return guard_on_; }
    // the gradient vector or the loss cell was rewritten behind backward()'s own scan (exchange, hook, a caller that holds the pointer):
    // optimizer_step() scans again (k_guard_scan, one launch) unless a pass of the caller's does it first with guard_scan_args()
    void guard_stale() { guard_scanned_ = false; }
    // both: what a writer of the gradient vector that runs behind backward() calls
    void grad_written_from_outside() { grad_vector_is_source(); guard_stale(); }
    // for a pass that scans the final gradient + loss itself: a fresh stamp; the next optimizer_step() reads that verdict
    GuardArgs guard_scan_args();
    // {skipped steps, number of the last skipped step} as of the last optimizer launch that has completed (a plain host read)
    void guard_stats(uint32_t* skipped, uint32_t* last_step) const;

private:
    bool guard_on_ = false, guard_scanned_ = false;
    uint32_t guard_stamp_ = 0;
    DevBuf<uint32_t> d_guard_;                      // GuardArgs::words
    PinnedCell h_guard_;                            // GuardArgs::host_cell (pinned, host-mapped)
    unsigned long long* d_guard_cell_ = nullptr;    // its device address
    int num_cus();
    int num_cus_ = 0;
    bool attr_infer_set_ = false, attr_infer4_set_ = false, attr_train_set_ = false, attr_train2_set_ = false;     // hipFuncSetAttribute done on this instance's device
    void ensure_train_workspace(uint32_t n);
    void ensure_features(uint32_t n, int slot);
    void launch_features(const float* d_in, uint32_t n, bool use_ema, int slot, hipStream_t s, bool skip_zero, const uint32_t* live_list = nullptr,
                         const uint32_t* live_count = nullptr);

    nrc_config cfg_;
    const MlpPlan plan_;         // shapes, offsets and kernel family of the model (validated: make_mlp_plan)
    DevBuf<void> d_feat_[5];     // generic path: fp16 features [n][enc_dims]; [0] inference, [1] training (encoded by backward), [2] [3] training (pre_encode, by parity), [4] side inference (kSideSlot)
    uint32_t feat_n_[5] = {0, 0, 0, 0, 0};
    int infer_set_ = 0;          // which of the double-buffered inference (EMA) image / table sets is current
    bool xcd8_ = true;           // the device has eight XCDs: the level-per-XCD launch mappings of the HashGrid kernels apply
    HashLevels levels_ = {};     // plan_.hg_off as the HashGrid kernels take it
    DevBuf<uint32_t> d_t16_train_, d_t16_ema_[2];   // half2-per-entry gather copies of the table
    DevBuf<_Float16> d_denc_;    // fp16 [n][32] dL/d(grid features)
    DevBuf<uint32_t> d_grad16_;  // half2 per table entry: target of the packed gradient atomics
    // bin lists of the table gradient (k_grid_scatter / k_grid_gather): (entry, value) pairs per bin of GB_BIN = 2 048 entries, pair counters, per-bin
    // {first entry, list offset, capacity}; d_grid_fix_: the table's fixed-point shadow (two int64 per entry) for what bypasses the lists
    DevBuf<uint2> d_grid_lists_;
    DevBuf<uint32_t> d_grid_counters_;
    DevBuf<uint4> d_grid_bin_entry0_;
    DevBuf<long long> d_grid_fix_;
    GridBinPlan bins_;           // of the current workspace (rebuilt when it grows)
    bool attr_gather_set_ = false;

    DevBuf<float> d_w_, d_ema_, d_m_, d_v_, d_grad_;
    float* d_loss_ = nullptr;            // inside d_grad_, behind the parameters
    std::vector<float> tcnn_dead_rows_[4];      // rows 3..15 of tiny-cuda-nn's 16 x width output matrix, per buffer 0..3
    float* dead_rows(int which) const
    {
        if (which < 0 || which > 4) fail("bad parameter buffer id");
        return which < 4 ? const_cast<float*>(tcnn_dead_rows_[which].data()) : nullptr;
    }
    // fp16 MFMA A-operand fragment images ([frag][lane][8 halfs]): inference (EMA), training forward, training dgrad (W^T)
    DevBuf<void> d_pk_infer_[2], d_pk_fwd_, d_pk_bwd_;
    DevBuf<int32_t> d_src_fwd_, d_src_bwd_;   // packed slot -> canonical index (-1 = zero)
    DevBuf<int32_t> d_dst_;              // [3][n_mlp] parameter -> slot in the forward / EMA inference / backward image (k_opt_pack)
    bool fused_opt_ = false;
    bool grad16_clean_ = false;          // d_grad16_ is all zero (the optimizer cleared what the last backward() touched)
    bool grid16_valid_ = false;          // the packed fp16 table gradient of the last backward() is what the optimizer should read
    int32_t* d_src_inf_ = nullptr;       // the same for the EMA inference image (= d_src_fwd_ unless enc80_generic)
    DevBuf<int32_t> d_src_inf_own_;      // what d_src_inf_ points at when it is not d_src_fwd_
    uint32_t n_frag_fwd_ = 0, n_frag_bwd_ = 0;

    // training workspace
    uint32_t ws_n_ = 0;
    DevBuf<void> d_acts_;        // fp16 [enc + depth*width][n]   (transposed: neuron-major)
    DevBuf<void> d_deltas_;      // fp16 [depth*width + 32][n]
    DevBuf<float> d_slabs_;      // fp32 [n_chunks][n_params]
    DevBuf<float> d_loss_part_;
    DevBuf<void> d_tiles_;       // WgradTile[] (output tiles of the weight-gradient GEMMs)
    int n_wgrad_tiles_ = 0;
    DevBuf<void> d_tasks_;       // WgradTask[] (row-block tasks of k_wgrad2)
    int n_wgrad_tasks_ = 0;
    bool wgrad_old_ = false;     // round 3's k_wgrad (up to 64 neurons; NRC_DEBUG=wgrad_old=0|1)
    uint32_t wgrad_cus() { return wgrad_old_ ? 0u : (uint32_t)num_cus(); }      // (k_wgrad's chunk does not depend on the device)
};

}  // namespace nrc
