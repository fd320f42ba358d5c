// vstab_track_host.cpp -- class Tracker (vstab_track_host.hpp): the pyramid sets and the LK segment launches whose records the host polls.
// Host C++; the kernels are those of vstab_pyramid.hip and vstab_lk.hip.  (The corner detector is vstab_detect_host.cpp.)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <string>

#include "vstab_hostlogic.hpp"
#include "vstab_track_host.hpp"

namespace vstab {

Tracker::~Tracker() {
    for (hipEvent_t e : {ev_a_, ev_b_})
        if (e) (void)hipEventDestroy(e);
}

vstab_status check_lk_options(const char *fn, int max_level, int max_iter, double eps, double min_eig_threshold, LkOptions &out) {
    const std::string n = std::string(fn) + ": ";
    if (max_level < 0 || max_level > LK_MAX_LEVELS - 1) return fail(VSTAB_ERR_INVALID, n + "max_level lies in 0 .. 3");
    if (max_iter < 1 || max_iter > 100) return fail(VSTAB_ERR_INVALID, n + "max_iter lies in 1 .. 100");
    if (!(eps >= 0.0 && eps <= 10.0)) return fail(VSTAB_ERR_INVALID, n + "eps is finite and lies in [0, 10]");
    if (!(min_eig_threshold >= 0.0) || !std::isfinite(min_eig_threshold)) return fail(VSTAB_ERR_INVALID, n + "min_eig_threshold is finite and not negative");
    out.max_level = max_level, out.max_iter = max_iter, out.eps = eps, out.min_eig = min_eig_threshold;
    return VSTAB_OK;
}

vstab_status Tracker::init(int w, int h, const LkOptions &opt) {
    w_ = w, h_ = h;
    opt_.win = opt.win;
    set_options(opt);
    VSTAB_TRY(ensure_levels(levels_));
    // record and point buffers for the pipeline's 200 features (FrameSourceWarp.cpp:230), so that nothing is
    // reallocated while a launch that uses them is queued
    for (int b = 0; b < REC_BUFS; b++) {
        VSTAB_TRY(hrec_[b].ensure(256 * 16));
        VSTAB_TRY(drec_[b].ensure(256 * 16));
        VSTAB_HIP_TRY(hipMemset(drec_[b].p, 0, 256 * 16));  // tag 0 is never a sequence number: a chained slot never mistakes stale bytes for its predecessor
    }
    for (int b = 0; b < PTS_BUFS; b++) VSTAB_TRY(hpts_[b].ensure(256 * sizeof(float2)));
    return VSTAB_OK;
}

// level sizes 0 .. n - 1 and the buffers of levels 1 .. n - 1 in every pyramid set (a buffer that is large enough stays)
vstab_status Tracker::ensure_levels(int n) {
    int lw = w_, lh = h_;
    lvl_w_[0] = lw, lvl_h_[0] = lh;
    for (int l = 1; l < n; l++) {
        lw = (lw + 1) / 2, lh = (lh + 1) / 2;
        lvl_w_[l] = lw, lvl_h_[l] = lh;
        for (int s = 0; s < PYR_SETS + PYR_DEV_EXTRA; s++) VSTAB_TRY(pyr_[s][l].ensure((size_t)lw * lh));
    }
    return VSTAB_OK;
}

vstab_status Tracker::set_window(int win) {
    // every level this window can ask for, whatever max_level says now: set_options may raise it afterwards
    VSTAB_TRY(ensure_levels(lk_levels(w_, h_, win)));
    opt_.win = win;
    set_options(opt_);
    return VSTAB_OK;
}

vstab_status Tracker::build_pyramid(int s, const uint8_t *gray, size_t pitch, hipStream_t st, hipEvent_t done, bool *done_bound, bool have_level1) {
#ifdef VSTAB_DEV
    static const bool twice = getenv("VSTAB_DEV_PYR_TWICE") != nullptr;
    if (twice && s != PYR_SETS) VSTAB_TRY(build_pyramid(PYR_SETS, gray, pitch, st));
#endif
    const uint8_t *src = gray;
    size_t sp = pitch;
    if (done_bound) *done_bound = false;
    for (int l = 1; l < levels_; l++) {
        // levels 2 and 3 in ONE launch (k_pyr_down_x2): as kernels of their own the small levels are launch- and latency-bound
        if (l == 2 && levels_ == 4 && pyr_down_x2_ok(lvl_w_[1], lvl_h_[1]) && !single_level_pyramid_) {
            VSTAB_TRY(launch_pyr_down_x2(src, sp, lvl_w_[1], lvl_h_[1], pyr_[s][2].as<uint8_t>(), (size_t)lvl_w_[2], pyr_[s][3].as<uint8_t>(), (size_t)lvl_w_[3], st, done));
            if (done_bound) *done_bound = done != nullptr;
            break;
        }
        const bool last = l == levels_ - 1;
        if (l == 1 && have_level1) {  // (written by k_pack_pyr together with the copy; if it is the only level the caller records the event)
            src = pyr_[s][l].as<uint8_t>(), sp = (size_t)lvl_w_[l];
            continue;
        }
        VSTAB_TRY(launch_pyr_down(src, sp, lvl_w_[l - 1], lvl_h_[l - 1], pyr_[s][l].as<uint8_t>(), (size_t)lvl_w_[l], st, last ? done : nullptr));
        if (last && done_bound) *done_bound = done != nullptr;
        src = pyr_[s][l].as<uint8_t>(), sp = (size_t)lvl_w_[l];
    }
    return VSTAB_OK;
}

vstab_status Tracker::track_wait(const Launch &L, int idx, size_t expect_n, std::vector<float> &next_xy, std::vector<uint8_t> &status, hipStream_t st, double *gpu_ms) {
    next_xy.clear(), status.clear();
    next_xy.reserve(2 * expect_n), status.reserve(expect_n);
    const int n = L.n_slots;
    if (n == 0) return expect_n == 0 ? VSTAB_OK : fail(VSTAB_ERR_DEVICE, "tracker bookkeeping mismatch");
    if (idx < 0 || idx >= L.n_frames) return fail(VSTAB_ERR_DEVICE, "tracker bookkeeping mismatch (frame pair outside its launch)");
    const uint32_t seq = L.seq[idx];
    const volatile uint32_t *rec = hrec_[L.buf[idx]].as<uint32_t>();
    const auto t0 = std::chrono::steady_clock::now();
    unsigned long spins = 0;
    int next = 0;
    for (;;) {  // (vstab_hostlogic.hpp: records are decoded as they arrive; a record is valid once both of its tags are)
        const LkParse r = lk_parse_records(rec, next, n, seq, expect_n, next_xy, status, &next);
        if (r == LK_PARSE_OK) break;
        if (r == LK_PARSE_BAD_CHAIN) return fail(VSTAB_ERR_DEVICE, "LK chain: a slot's predecessor record does not carry its parent's tag");
        if (r == LK_PARSE_COUNT_MISMATCH) return fail(VSTAB_ERR_DEVICE, "tracker bookkeeping mismatch");
        while (!lk_record_ready(rec, next, seq)) {
            __builtin_ia32_pause();
            if ((++spins & 0xffff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) {
                VSTAB_HIP_TRY(hipStreamSynchronize(st));  // surfaces a launch / execution error if there is one
                if (!lk_record_ready(rec, next, seq)) return fail(VSTAB_ERR_DEVICE, "LK kernel did not complete");
            }
        }
    }
    if (L.timed && gpu_ms) {
        float ms = 0;
        if (hipEventSynchronize(ev_b_) == hipSuccess && hipEventElapsedTime(&ms, ev_a_, ev_b_) == hipSuccess) *gpu_ms += ms;
    }
    return VSTAB_OK;
}

vstab_status Tracker::track_ex(const LkPyramid &I, const LkPyramid &J, const std::vector<float> &prev_xy, const float *guess_xy, int flags, float *err,
                               std::vector<float> &next_xy, std::vector<uint8_t> &status, hipStream_t st) {
    const size_t n = prev_xy.size() / 2;
    next_xy.clear(), status.clear();
    if (n == 0) return VSTAB_OK;
    const float2 *guess = nullptr;
    if (flags & VSTAB_LK_USE_INITIAL_FLOW) {
        VSTAB_TRY(guess_.ensure(n * sizeof(float2)));
        VSTAB_HIP_TRY(hipMemcpy(guess_.p, guess_xy, n * sizeof(float2), hipMemcpyHostToDevice));  // complete before the launch below is enqueued
        guess = guess_.as<float2>();
    }
    if (err) VSTAB_TRY(err_.ensure(n * sizeof(float)));
    Launch L;
    const LkPyramid pyr[2] = {I, J};
    ex_flags_ = flags, ex_guess_ = guess, ex_err_ = err ? err_.as<float>() : nullptr;
    const vstab_status launched = track_launch(pyr, 1, prev_xy, st, false, L);
    ex_flags_ = 0, ex_guess_ = nullptr, ex_err_ = nullptr;
    VSTAB_TRY(launched);
    VSTAB_TRY(track_wait(L, 0, n, next_xy, status, st, nullptr));
    if (err) {
        // err leaves the kernel by plain stores behind the records: complete once the stream is
        VSTAB_HIP_TRY(hipStreamSynchronize(st));
        VSTAB_HIP_TRY(hipMemcpy(err, err_.p, n * sizeof(float), hipMemcpyDeviceToHost));
    }
    return VSTAB_OK;
}

void *Tracker::clock_slot() {
    static const bool on = getenv("VSTAB_LK_CLOCK") != nullptr;
    if (!on) return nullptr;
    if (!clk_.p) {
        if (clk_.ensure(sizeof(unsigned long long) * 2 * CLK_N) != VSTAB_OK) return nullptr;
        std::vector<unsigned long long> init(2 * CLK_N, 0);
        for (int i = 0; i < CLK_N; i++) init[2 * i] = ~0ull;
        if (hipMemcpy(clk_.p, init.data(), sizeof(unsigned long long) * init.size(), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    }
    if (clk_used_ >= CLK_N) return nullptr;
    return clk_.as<unsigned long long>() + 2 * (clk_used_++);
}

void Tracker::report_clock() {
    if (!clk_.p || clk_used_ < 200) return;
    std::vector<unsigned long long> host(2 * CLK_N);
    if (hipMemcpy(host.data(), clk_.p, sizeof(unsigned long long) * host.size(), hipMemcpyDeviceToHost) != hipSuccess) return;
    const unsigned long long *c = host.data();
    double dur = 0, gap = 0, idle = 0;
    int n = 0;
    for (int i = clk_used_ - 400 > 0 ? clk_used_ - 400 : 1; i < clk_used_; i++) {
        if (c[2 * i + 1] == 0 || c[2 * i - 1] == 0) continue;
        dur += (c[2 * i + 1] - c[2 * i]) * 0.01, gap += ((double)c[2 * i] - (double)c[2 * i - 2]) * 0.01, idle += ((double)c[2 * i] - (double)c[2 * i - 1]) * 0.01;
        n++;
    }
    if (n) std::fprintf(stderr, "LK launches (last %d): duration %.1f us, start-to-start %.1f us, idle before start %.1f us\n", n, dur / n, gap / n, idle / n);
    std::vector<double> idles, durs;
    for (int i = clk_used_ - 400 > 0 ? clk_used_ - 400 : 1; i < clk_used_; i++)
        if (c[2 * i + 1] && c[2 * i - 1]) idles.push_back(((double)c[2 * i] - (double)c[2 * i - 1]) * 0.01), durs.push_back((c[2 * i + 1] - c[2 * i]) * 0.01);
    std::sort(idles.begin(), idles.end()), std::sort(durs.begin(), durs.end());
    if (idles.size() > 10) {
        const size_t m = idles.size();
        std::fprintf(stderr, "  idle percentiles 10/50/90/99: %.1f %.1f %.1f %.1f   duration 10/50/90/99: %.1f %.1f %.1f %.1f\n", idles[m / 10], idles[m / 2],
                     idles[m * 9 / 10], idles[m * 99 / 100], durs[m / 10], durs[m / 2], durs[m * 9 / 10], durs[m * 99 / 100]);
    }
}

vstab_status Tracker::launch_segment(const LkPyramid *pyr, int n_frames, const float2 *prev_pts, const void *chain_in, uint32_t parent_seq, hipStream_t st, Launch &L) {
    if (n_frames < 1 || n_frames > LK_SEG_MAX) return fail(VSTAB_ERR_INVALID, "tracker: a launch covers 1 .. LK_SEG_MAX frame pairs");
    LkSegArgs a;
    std::memset(&a, 0, sizeof(a));
    L.n_frames = n_frames;
    for (int i = 0; i <= n_frames; i++) a.pyr[i] = pyr[i];
    for (int i = 0; i < n_frames; i++) {
        L.buf[i] = (int)(rec_next_++ % REC_BUFS);
        if (++seq_ == 0) ++seq_;  // tag 0 means "never written"
        L.seq[i] = seq_;
        VSTAB_TRY(hrec_[L.buf[i]].ensure((size_t)L.n_slots * 16));
        VSTAB_TRY(drec_[L.buf[i]].ensure((size_t)L.n_slots * 16));
        if (!hrec_[L.buf[i]].dev()) return fail(VSTAB_ERR_DEVICE, "hipHostGetDevicePointer failed");
        a.host_rec[i] = static_cast<uint4 *>(hrec_[L.buf[i]].dev()), a.dev_rec[i] = drec_[L.buf[i]].as<uint4>(), a.seq[i] = L.seq[i];
    }
    a.n_frames = n_frames, a.n = L.n_slots;
    a.prev_pts = prev_pts, a.chain_in = static_cast<const uint4 *>(chain_in), a.parent_seq = parent_seq;
    lk_set_options(a, opt_);
    a.flags = ex_flags_, a.init_pts = ex_guess_, a.err = ex_err_;  // (track_ex only; launch_lk refuses them on a segment or a chained launch)
    a.clk = static_cast<unsigned long long *>(clock_slot());
    if (L.timed && !ev_a_) (void)hipEventCreate(&ev_a_), (void)hipEventCreate(&ev_b_);
    if (L.timed) (void)hipEventRecord(ev_a_, st);
    VSTAB_TRY(launch_lk(a, st));
    if (L.timed) (void)hipEventRecord(ev_b_, st);
    return VSTAB_OK;
}

}  // namespace vstab
