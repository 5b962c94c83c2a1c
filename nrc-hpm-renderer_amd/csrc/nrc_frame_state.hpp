// nrc_frame_state.hpp -- the frame bookkeeping of the renderers that touches no device: which random numbers a frame uses, and when a sorted
// tile order becomes the one in force.  Plain C++17 that nrc_api.hip includes; tests/cpp/host_logic_main.cpp drives both types on the CPU
// against the conditions they replaced, written out frame by frame.
#pragma once
#include <cstdint>
#include <cstring>
#include <random>
#include <utility>

namespace nrc {

// The four random numbers of each frame.  A frame takes, in this order of preference: the caller's pinned numbers (set_frame_random: used
// once); the numbers drawn one frame ahead; a fresh draw.  A frame that promotes hot tiles announces what the NEXT frame will use -- the
// caller's hint (render_frames knows its frames' numbers) or numbers drawn now instead of then -- so that the frame after it can say whether
// its numbers were known in time.  Scheduling does not depend on the announcement (the hot-tile list is computed for whatever numbers a
// frame uses): the draw-ahead keeps the sequence of unpinned numbers what it is without it, and the announced numbers only feed the 1 / 0
// that nrc_renderer_hot_tiles returns.  A renderer that never announces (McRenderer) pins and takes.
class FrameRandoms {
public:
    explicit FrameRandoms(uint32_t seed) : rng_(seed) {}
    void pin(const float* r4) { std::memcpy(pinned_, r4, 16); have_pinned_ = true; }
    // the numbers of the frame after the next one to be rendered: they are that frame's numbers instead of numbers drawn ahead
    void hint(const float* r4) { std::memcpy(hint_, r4, 16); have_hint_ = true; }
    void take(float* frame_random)
    {
        if (std::exchange(have_pinned_, false)) std::memcpy(frame_random, pinned_, 16);
        else if (std::exchange(have_ahead_, false)) std::memcpy(frame_random, ahead_, 16);
        else draw(frame_random);
    }
    // were these, the current frame's numbers, announced by the frame before it?
    bool was_predicted(const float* frame_random) const { return next_known_ && std::memcmp(known_, frame_random, 16) == 0; }
    // the end of a frame's planning.  promote: the frame promotes hot tiles and announces; otherwise nothing is known about the next
    // frame.  A hint lasts one frame either way.
    void announce_next(bool promote)
    {
        if (promote) {
            if (!have_hint_ && !have_ahead_) { draw(ahead_); have_ahead_ = true; }
            std::memcpy(known_, have_hint_ ? hint_ : ahead_, 16);
        }
        have_hint_ = false;
        next_known_ = promote;
    }
    const std::mt19937& generator() const { return rng_; }      // (tests: its state counts the draws)

private:
    void draw(float* r4)
    {
        std::uniform_real_distribution<float> u(0.0f, 1.0f);
        for (int k = 0; k < 4; k++) r4[k] = u(rng_);
    }
    std::mt19937 rng_;
    float pinned_[4] = {0, 0, 0, 0}, ahead_[4] = {0, 0, 0, 0}, hint_[4] = {0, 0, 0, 0}, known_[4] = {0, 0, 0, 0};
    bool have_pinned_ = false, have_ahead_ = false, have_hint_ = false, next_known_ = false;
};

// When gen_rays samples its tiles' costs and when the order sorted from them takes effect.  Two order buffers: frames launch in buffer
// current(); a frame that samples has the sort write other() (sort_enqueued), and the first frame at least `lag` frames later flips the two
// (take_effect; the schedule's cost_order_lag).  A cost sample every kEvery-th frame (the side streams live in gen_rays' tail: a sort per
// frame costs them more than a fresher order gains), never while a sort is waiting to take effect, and with the next free frame after the
// medium or the view changed (the costs belong to the old one).
struct TileOrderClock {
    static constexpr uint64_t kEvery = 4;
    bool on = true;      // cost order in use (set_cost_order)
    int current() const { return cur_; }
    int other() const { return cur_ ^ 1; }
    bool sort_pending() const { return pending_; }
    // a finished sort is due at `frame`: the buffer the next frame launches in is other()
    bool due(uint64_t frame, int lag) const { return pending_ && frame >= pending_frame_ + (uint64_t)lag; }
    // the head of frame `frame`: true when a due sort took effect -- the buffers have flipped, and the caller orders its camera launch
    // behind the sort
    bool take_effect(uint64_t frame, int lag)
    {
        if (!on || !due(frame, lag)) return false;
        cur_ ^= 1;
        pending_ = false;
        return true;
    }
    // does frame `frame` sample costs?  (asked once per frame, behind take_effect: a yes uses up the medium's request)
    bool samples(uint64_t frame)
    {
        const bool yes = on && !pending_ && (frame % kEvery == 0 || resample_);
        if (yes) resample_ = false;
        return yes;
    }
    void sort_enqueued(uint64_t frame) { pending_ = true; pending_frame_ = frame; }
    void medium_changed() { resample_ = true; }

private:
    bool pending_ = false, resample_ = false;
    int cur_ = 0;
    uint64_t pending_frame_ = 0;
};

}  // namespace nrc
