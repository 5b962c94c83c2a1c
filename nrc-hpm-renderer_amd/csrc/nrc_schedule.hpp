// nrc_schedule.hpp -- the renderer's schedule (include/nrc_hpm.h, nrc_schedule) and who chooses it: the process-wide table of schedules
// and its text file, the key a renderer is filed under, the bookkeeping of the per-frame timing-event sets, and the tuner that tries the
// knobs on live frames.  Device-free: the tuner sees the device's events only through the three questions of its Host parameter (the
// renderer answers them from its event pool; tests/cpp/host_logic_main.cpp answers them from a scripted clock, under the sanitizers).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/nrc_hpm.h"
#include "nrc_fail.hpp"

namespace nrc {

// ---- schedules the tuner has settled on, remembered per (device, model, volume, frame) -- nrc_schedule_cache_load / _save ---------------
// The tuner needs ~400 frames (128 of warm-up, then its trials) before a renderer runs on the schedule that suits its model and scene; a
// short run -- the driver's 25-frame bench of configs[4] or of the HashGrid model -- ends before that.  What it settles on is therefore
// kept in a process-wide table under a key that names what the choice depends on, a host can save the table to a text file and load it
// in the next process, and a renderer whose key is in the table starts on that schedule (source "cache") and skips the trials.  No value
// of any knob changes a pixel (tests/test_gpu_frame_graph.py), so a stale or foreign entry costs speed at worst.
struct ScheduleEntry { int pri, lag, window; };
struct ScheduleCache {
    std::mutex m;
    std::map<std::string, ScheduleEntry> table;
    static ScheduleCache& get() { static ScheduleCache c; return c; }
    bool find(const std::string& key, ScheduleEntry* out)
    {
        std::lock_guard<std::mutex> g(m);
        auto it = table.find(key);
        if (it == table.end()) return false;
        *out = it->second;
        return true;
    }
    void put(const std::string& key, ScheduleEntry e) { std::lock_guard<std::mutex> g(m); table[key] = e; }
    // text, one entry per line: <key> <camera_priority_low> <cost_order_lag> <xcd_window>; '#' starts a comment; keys hold no blanks
    int load(const char* path)
    {
        FILE* f = std::fopen(path, "r");
        if (!f) throw std::runtime_error(std::string("SkyRenderer ERROR: cannot read schedule cache ") + path);
        char line[1024];
        int n = 0;
        std::lock_guard<std::mutex> g(m);
        while (line[sizeof line - 2] = '\0', std::fgets(line, sizeof line, f)) {
            // a line that filled the buffer without ending: its head is read below, the rest of it is not a line of its own
            if (line[sizeof line - 2] != '\0' && line[sizeof line - 2] != '\n')
                for (int c; (c = std::fgetc(f)) != EOF && c != '\n';) {}
            char key[768];
            int pri = 0, lag = 0, win = 0;
            if (line[0] == '#' || std::sscanf(line, "%767s %d %d %d", key, &pri, &lag, &win) != 4) continue;
            if (lag < 1 || lag > 64 || win < 0 || win > 32) continue;      // (nrc_schedule's ranges: a damaged line is skipped, not applied)
            table[key] = ScheduleEntry{pri != 0, lag, win};
            n++;
        }
        std::fclose(f);
        return n;
    }
    int save(const char* path)
    {
        FILE* f = std::fopen(path, "w");
        if (!f) throw std::runtime_error(std::string("SkyRenderer ERROR: cannot write schedule cache ") + path);
        std::lock_guard<std::mutex> g(m);
        std::fprintf(f, "# nrc_schedule_cache_save: <device|model|volume|frame|train rays> camera_priority_low cost_order_lag xcd_window\n");
        for (const auto& kv : table) std::fprintf(f, "%s %d %d %d\n", kv.first.c_str(), kv.second.pri, kv.second.lag, kv.second.window);
        const bool ok = std::fclose(f) == 0;
        if (!ok) throw std::runtime_error(std::string("SkyRenderer ERROR: short write to schedule cache ") + path);
        return (int)table.size();
    }
};

// what the best schedule depends on (measured): the chip, the model's kernels, how large the volume is
// against the L2s, the frame and its share of the whole, the training batch
inline std::string schedule_key(const std::string& arch, int cus, int xcds, const nrc_config& cfg, unsigned long long voxels, uint32_t w, uint32_t h,
                                uint32_t global_w, uint32_t global_h, uint32_t train_batch_size, uint32_t train_ray_length)
{
    int vlog = 0;
    while ((1ull << (vlog + 1)) <= voxels) vlog++;
    char key[512];
    std::snprintf(key, sizeof key, "%s:%dcu:%dxcd|pos%u.dir%u.w%u.d%u.hg%u|vol2^%d|%ux%u.of%ux%u|train%ux%u.len%u", arch.c_str(),
                  cus, xcds, cfg.pos_id, cfg.dir_id, cfg.nn_width, cfg.nn_depth,
                  cfg.pos_id == 0 ? (cfg.hashgrid_log2_size ? cfg.hashgrid_log2_size : 19u) : 0u, vlog, w, h, global_w, global_h,
                  cfg.train_batch_count, train_batch_size, train_ray_length);
    std::string k = key;
    if (cfg.self_train != 0u) k += ".st";      // (only then: the keys of every other configuration stay as they were)
    return k;
}

// ---- which timing-event set a frame uses.  One set per frame since the last statistics reset (the reference has 8 Vulkan timestamp
// queries, :495-515); the pool grows until it holds kMaxSets, then wraps: statistics then cover the most recent frames only.  The events
// themselves are the renderer's; this is the arithmetic.
struct EventPoolIndex {
    static constexpr size_t kMaxSets = 4096;
    static constexpr size_t kNone = ~(size_t)0;
    size_t used = 0;            // sets taken since the last reset
    size_t last = kNone;        // the set of the newest frame enqueued (it outlives a reset: the frame is still in flight)
    uint64_t epoch = 0;         // bumped whenever the pool starts over (its indices then mean other frames)
    bool timed = false;         // a frame has been enqueued since the last reset
    // top of a frame, pool_size sets exist: true = the caller creates set `used` first (a full pool of kMaxSets wraps instead)
    bool must_grow(size_t pool_size)
    {
        if (used != pool_size) return false;
        if (pool_size >= kMaxSets) { used = 0; epoch++; return false; }
        return true;
    }
    size_t take() { last = used; return used++; }
    void reset() { used = 0; epoch++; timed = false; }
};

struct Schedule {
    int pri, lag, window, defer;      // nrc_schedule: camera_priority_low, cost_order_lag, xcd_window, composite_defer
};

// the plain numbers of a tuner step, taken at the top of a frame (after EventPoolIndex::must_grow, before take)
struct TunerStep {
    uint64_t frame_index;
    size_t ev_used, pool_size, last_set;      // EventPoolIndex::used, sets that exist, EventPoolIndex::last
    uint64_t pool_epoch;
    bool stage_events, multi_stream;          // (no frame timeline / the single-stream diagnostic order: nothing is tuned)
};

// ---- the schedule and who chooses it: the values in use, the caller's pins, the tuner ------------------------------------------------
//   camera_priority_low  the camera kernels at the default wave priority under the library's other kernels at 3: where the inference ->
//                        training chain sets the frame rate its kernels get issue slots sooner (configs[4] + 1.5 %); the default preset,
//                        bound by gen_rays itself, loses 5.5 % with it and the HashGrid model 2 %
//   cost_order_lag       frames between a cost sample and the first launch ordered by it: the sort sits at the end of stream D's work for
//                        the sampled frame; where the side chain is long the second-next gen_rays would wait for it (configs[4] + 1.2 % at 3)
//   xcd_window           k_tile_order_xcd: the tiles of a window of 32 M ranks are handed to the XCDs by screen row, so that each L2 sees a
//                        band of the volume (default preset: M = 1 ... 8 + 0.6-0.9 %, M = 32 - 2.5 %; the 512^3 smoke + 5.2 % at 16)
// Rounds 3-4 keyed these to the bench presets (128-wide model, more than 32 M voxels).  Now the renderer starts from neutral values and
// CHOOSES: from its own frame timeline, trying the alternatives on live frames once the pipeline runs; a caller's
// nrc_renderer_set_schedule pins what it sets.
//
// The Tuner.  No knob of the schedule changes a result, so the alternatives can be tried on the caller's own frames: once the pipeline
// has run for kWarm frames (a short run -- the driver's 100-frame benchmark -- is never touched) the knobs the caller has not pinned are
// taken one after the other (priority, lag, window: a later knob is tried on top of what the earlier ones settled on -- the window
// that pays under low-priority camera kernels is not the one that pays without).  A knob's trials are played back to back -- base,
// alternative(s), base: the current value before and after the others (the GPU's clock drifts for the first hundred frames of
// load) -- each value held for kSettle + kMeasure frames and timed by the frames' own start events (interval
// between the gen_rays launches of the first and the last measured frame).  Left alone the host runs far ahead of the GPU (it enqueues a
// frame in a third of the time the GPU needs: hundreds of frames by the end of a long call) and the tuner would learn its results long
// after the run's best part; so while it tunes, Render keeps the host at most kAhead frames ahead (it waits for the gen_rays of frame
// N - kAhead -- the reference's Render waits for the previous frame's fence every time).  When a knob's last trial has completed it
// is decided against the mean of its two base trials; an alternative is adopted only if it is more than 1.5 % faster.  A trial
// during which the host let the pipeline drain (the previous frame's gen_rays was already complete when the next frame was enqueued)
// says nothing about the schedule: the sequence is then played again, three times at most.
//
// step() asks its Host, by event-set index (always below TunerStep::pool_size):
//   bool gen_rays_done(size_t set)                          is the set's "gen_rays done" event complete
//   bool start_interval_ms(size_t a, size_t b, float* ms)   time between the start events of sets a and b; false: it cannot be told
//   bool wait_gen_rays(size_t set)                          wait (bounded by the communicator's deadline) for the set's "gen_rays done"
//                                                           event; false: the communicator has failed
class ScheduleTuner {
public:
    static constexpr uint64_t kWarm = 128, kSettle = 8, kMeasure = 16, kAhead = 8;

    ScheduleTuner() = default;
    // a renderer whose key is in the table starts on that schedule and skips the trials
    ScheduleTuner(bool xcd_ok, std::string key) : sched_{0, 2, xcd_ok ? 2 : 0, 0}, key_(std::move(key)), xcd_ok_(xcd_ok)      // (k_tile_order_xcd deals to eight XCDs)
    {
        ScheduleEntry e;
        if (ScheduleCache::get().find(key_, &e)) {
            sched_.pri = e.pri; sched_.lag = e.lag; sched_.window = e.window;
            tune_.state = Tuner::Done;
            source_ = "cache";
        }
    }
    const Schedule& now() const { return sched_; }
    bool xcd_ok() const { return xcd_ok_; }
    const char* source() const { return source_; }      // default | cache | tuner | pinned | pinned in part
    const char* key() const { return key_.c_str(); }    // ScheduleCache key of this renderer

    // nrc_renderer_set_schedule: a field >= 0 pins the knob (the tuner leaves it alone), -1 hands it back to the library
    void set(const nrc_schedule& in, uint64_t frame_index)
    {
        if (in.cost_order_lag == 0 || in.cost_order_lag > 64 || in.xcd_window > 32) fail("nrc_schedule: cost_order_lag must be 1..64, xcd_window 0..32");
        auto take = [](int32_t v, int& knob, bool& pin) { pin = v >= 0; if (pin) knob = (int)v; };
        take(in.camera_priority_low < 0 ? -1 : (in.camera_priority_low != 0), sched_.pri, pin_pri_);
        take(in.cost_order_lag, sched_.lag, pin_lag_);
        take(in.xcd_window, sched_.window, pin_win_);
        if (in.composite_defer >= 0) sched_.defer = in.composite_defer != 0;
        if (tune_.state != Tuner::Warm && tune_.state != Tuner::Done) {      // in mid-trial sched_ holds a TRIAL value: back to the base first
            const Schedule asked = sched_;
            sched_ = tune_.base;
            if (pin_pri_) sched_.pri = asked.pri;
            if (pin_lag_) sched_.lag = asked.lag;
            if (pin_win_) sched_.window = asked.window;
            sched_.defer = asked.defer;
        }
        tune_ = Tuner{};      // (what is left to choose is chosen afresh, kWarm frames from now)
        tune_start_ = frame_index;
        source_ = all_pinned() ? "pinned" : (pin_pri_ || pin_lag_ || pin_win_) ? "pinned in part" : "default";
    }
    void get(nrc_schedule* out, int* tuning_done) const
    {
        out->camera_priority_low = sched_.pri;
        out->cost_order_lag = sched_.lag;
        out->xcd_window = xcd_ok_ ? sched_.window : 0;
        out->composite_defer = sched_.defer;
        if (tuning_done) *tuning_done = (tune_.state == Tuner::Done || all_pinned()) ? 1 : 0;
    }

    // nrc_renderer_render_path, at every view: a trial window that contains a camera change is discarded.  The schedule goes back to the
    // trial sequence's base, the knob's sequence starts again kWarm frames from now (so no trial runs inside a view shorter than that, and
    // none is timed across two views), and nothing measured across a view change reaches the ScheduleCache.
    void view_changed(uint64_t frame_index)
    {
        Tuner& t = tune_;
        if (t.state == Tuner::Done) return;
        if (t.state != Tuner::Warm) {
            apply(t.trials[0]);
            t.state = Tuner::Warm;
            t.rounds = 0;
            t.attempts = 0;
        }
        tune_start_ = frame_index;
    }

    // once per frame, before the frame is enqueued (may change now(): the renderer chooses its scheduling knobs from its own frame timeline)
    template <class Host>
    void step(const TunerStep& s, Host& host)
    {
        Tuner& t = tune_;
        if (t.state == Tuner::Done) return;
        if (!s.stage_events || !s.multi_stream) return;
        if (t.state == Tuner::Warm) {
            if (s.frame_index >= tune_start_ + kWarm) begin_sequence(s);
            return;
        }
        // (bounded run-ahead while tuning, see above; a pool that started over has lost the frame)
        if (t.epoch == s.pool_epoch && s.ev_used >= kAhead + 1 && s.ev_used - 1 - kAhead < s.pool_size) {
            // (bounded by the communicator's deadline: the render stream waits, transitively, for the training stream's collective -- a
            // peer that has died must not hang this rank inside the tuner.  A failed exchange ends the trials; Render reports it.)
            if (!host.wait_gen_rays(s.ev_used - 1 - kAhead)) { apply(t.trials[0]); t.state = Tuner::Done; return; }
        }
        if (t.state == Tuner::Settle) {
            if (s.frame_index >= t.t0 + kSettle) { t.trials[t.cur].ev_first = s.ev_used; t.state = Tuner::Measure; }
            return;
        }
        if (t.state == Tuner::Measure) {
            // a host that lets the pipeline drain between two measured frames is not measuring the schedule
            if (s.last_set != EventPoolIndex::kNone && host.gen_rays_done(s.last_set)) t.trials[t.cur].stalls++;
            if (s.frame_index < t.t0 + kSettle + kMeasure) return;
            t.trials[t.cur].ev_last = s.ev_used;
            if (++t.cur < t.trials.size()) {
                apply(t.trials[t.cur]);
                t.t0 = s.frame_index;
                t.state = Tuner::Settle;
                return;
            }
            apply(t.trials[0]);      // the base schedule while the GPU catches up
            t.state = Tuner::Wait;
            return;
        }
        // Wait: have the last trial's frames run?  (the frame's "gen_rays done" event is the one to ask: a launch's START event carries a
        // time stamp but is not something to query)
        bool valid = t.epoch == s.pool_epoch;
        if (valid) {
            const size_t last = t.trials.back().ev_last;
            if (last >= s.ev_used || last >= s.pool_size) return;
            if (!host.gen_rays_done(last)) return;      // not yet: look again with the next frame
            for (Tuner::Trial& tr : t.trials) {
                float ms = 0.0f;
                if (tr.stalls > 1 || tr.ev_last <= tr.ev_first || !host.start_interval_ms(tr.ev_first, tr.ev_last, &ms) || !(ms > 0.0f)) { valid = false; break; }
                tr.ms = (double)ms / (double)(tr.ev_last - tr.ev_first);
            }
        }
        if (!valid) {      // play the sequence again; a host that never keeps the pipeline full leaves the schedule as it is
            apply(t.trials[0]);
            if (++t.attempts >= 3) { t.state = Tuner::Done; return; }
            begin_sequence(s);
            return;
        }
        // decide the knob against the mean of the base trials on either side of its alternatives.  Effects of 1-3 % are the size of a
        // 16-frame interval's noise: a result in that band is played again (three rounds at most) and decided on the averages.
        t.rounds++;
        for (Tuner::Trial& tr : t.trials) tr.sum += tr.ms;
        Schedule chosen = t.base;
        chosen.defer = sched_.defer;
        {
            const double base = 0.5 * (t.trials.front().sum + t.trials.back().sum);
            double best_alt = 1e300;
            for (size_t q = 1; q + 1 < t.trials.size(); q++) best_alt = std::min(best_alt, t.trials[q].sum);
            const double rel = best_alt / base;
            if (t.rounds < 3 && rel > 0.96 && rel < 1.005) {      // ambiguous: once more
                for (Tuner::Trial& tr : t.trials) { tr.stalls = 0; tr.ev_first = tr.ev_last = 0; }
                t.cur = 0;
                t.epoch = s.pool_epoch;
                apply(t.trials[0]);
                t.t0 = s.frame_index;
                t.state = Tuner::Settle;
                return;
            }
            double best = base * 0.985;
            for (size_t q = 1; q + 1 < t.trials.size(); q++)
                if (t.trials[q].sum < best) { best = t.trials[q].sum; (t.knob == 0 ? chosen.pri : t.knob == 1 ? chosen.lag : chosen.window) = t.trials[q].value; }
        }
        sched_ = chosen;
        t.knob++;
        t.rounds = 0;
        t.attempts = 0;
        begin_sequence(s);      // the next knob, on top of this choice (or Done)
    }

private:
    struct Tuner {
        enum State { Warm, Settle, Measure, Wait, Done } state = Warm;
        struct Trial {
            int knob, value;                // knob -1: the base schedule
            size_t ev_first = 0, ev_last = 0;
            int stalls = 0;
            double ms = 0.0, sum = 0.0;     // this round's interval; the sum over the knob's rounds
        };
        std::vector<Trial> trials;
        int knob = 0;                       // the knob whose trials are being played (0 priority, 1 lag, 2 window)
        int rounds = 0;                     // completed rounds of the knob's sequence (an ambiguous result is played again and averaged)
        size_t cur = 0;
        uint64_t t0 = 0;                    // frame at which the current trial's value took effect
        uint64_t epoch = 0;
        int attempts = 0;
        Schedule base{};
    };
    Schedule sched_{0, 2, 2, 0};
    std::string key_;
    const char* source_ = "default";
    bool pin_pri_ = false, pin_lag_ = false, pin_win_ = false;      // set by the caller (nrc_renderer_set_schedule): not tuned
    bool xcd_ok_ = true;
    Tuner tune_;
    uint64_t tune_start_ = 0;

    int& knob_ref(int k) { return k == 0 ? sched_.pri : k == 1 ? sched_.lag : sched_.window; }
    bool knob_pinned(int k) const { return k == 0 ? pin_pri_ : k == 1 ? pin_lag_ : (pin_win_ || !xcd_ok_); }
    bool all_pinned() const { return pin_pri_ && pin_lag_ && (pin_win_ || !xcd_ok_); }
    void apply(const Tuner::Trial& tr)
    {
        const int defer = sched_.defer;
        sched_ = tune_.base;
        sched_.defer = defer;
        if (tr.knob >= 0) knob_ref(tr.knob) = tr.value;
    }
    void begin_sequence(const TunerStep& s)
    {
        Tuner& t = tune_;
        while (t.knob < 3 && knob_pinned(t.knob)) t.knob++;
        if (t.knob >= 3) {      // every knob decided (or pinned): remember the result for the next renderer of this kind
            t.state = Tuner::Done;
            if (!all_pinned()) {
                ScheduleCache::get().put(key_, ScheduleEntry{sched_.pri, sched_.lag, sched_.window});
                source_ = "tuner";
            }
            return;
        }
        t.base = sched_;
        t.rounds = 0;
        t.trials.clear();
        t.trials.push_back({-1, 0});
        const int k = t.knob, cur = knob_ref(k);
        if (k == 0) t.trials.push_back({0, cur ? 0 : 1});
        else if (k == 1) t.trials.push_back({1, cur == 2 ? 3 : 2});
        else for (int w : {0, 2, 16}) if (w != cur) t.trials.push_back({2, w});
        t.trials.push_back({-1, 0});
        t.cur = 0;
        t.epoch = s.pool_epoch;
        apply(t.trials[0]);
        t.t0 = s.frame_index;
        t.state = Tuner::Settle;
    }
};

}  // namespace nrc
