// vstab_track_host.cpp -- class Tracker (vstab_track_host.hpp): the pyramid sets, the host half of goodFeaturesToTrack, the speculative
// detection with its helper thread, and the LK segment launches whose records the host polls.  Host C++; the kernels are those of vstab_pyramid.hip, vstab_corners.hip and vstab_lk.hip.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>

#include "vstab_hostlogic.hpp"
#include "vstab_track_host.hpp"

namespace vstab {

Tracker::~Tracker() {
    // the helper thread polls spec_ev_ while a selection is running: stop and join it BEFORE the events go
    if (spec_thread_started_) {
        {
            std::lock_guard<std::mutex> lk(spec_m_);
            spec_quit_ = true;
        }
        spec_cv_.notify_one();
        spec_thread_.join();
    }
    for (hipEvent_t e : {spec_ev_, ev_a_, ev_b_})
        if (e) (void)hipEventDestroy(e);
}

vstab_status Tracker::init(int w, int h) {
    w_ = w, h_ = h, levels_ = lk_levels(w, h);
    int lw = w, lh = h;
    for (int l = 1; l < levels_; l++) {
        lw = (lw + 1) / 2, lh = (lh + 1) / 2;
        lvl_w_[l] = lw, lvl_h_[l] = lh;
        for (int s = 0; s < PYR_SETS + PYR_DEV_EXTRA; s++) VSTAB_TRY(pyr_[s][l].ensure((size_t)lw * lh));
    }
    lvl_w_[0] = w, lvl_h_[0] = h;
    VSTAB_TRY(small_.ensure(256));
    VSTAB_TRY(hsmall_.ensure(256));
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

vstab_status Tracker::copy_mask(const void *mask, size_t pitch, bool host) {
    if (!mask) {
        set_mask(nullptr, 0);
        return VSTAB_OK;
    }
    const size_t own_pitch = ((size_t)w_ + 3) & ~(size_t)3;
    VSTAB_TRY(mask_buf_.ensure(own_pitch * (size_t)h_));
    VSTAB_HIP_TRY(hipMemset(mask_buf_.p, 0, own_pitch * (size_t)h_));  // the padding bytes are never read; zero all the same
    VSTAB_HIP_TRY(hipMemcpy2D(mask_buf_.p, own_pitch, mask, pitch, (size_t)w_, (size_t)h_, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice));
    VSTAB_HIP_TRY(hipDeviceSynchronize());  // (a device-to-device copy may return before it is done: the caller may free the mask after this call)
    set_mask(mask_buf_.as<uint8_t>(), own_pitch);
    return VSTAB_OK;
}

void Tracker::select_corners(unsigned long long *k, unsigned int n, int max_corners, double min_distance, std::vector<float> &xy) {
    xy.clear();
    const int cell = (int)std::nearbyint(min_distance);
    const int gw = cell >= 1 ? (w_ + cell - 1) / cell : 0, gh = cell >= 1 ? (h_ + cell - 1) / cell : 0;
    const double md2 = min_distance * min_distance;
    static thread_local std::vector<int> grid_head_, grid_next_;  // min-distance grid: per-cell lists of accepted corners
    if (cell >= 1) grid_head_.assign((size_t)gw * gh, -1), grid_next_.clear();
    // The greedy pass consumes candidates in sorted order and usually stops after a few hundred, so the
    // keys are sorted lazily in chunks: nth_element splits off the next `chunk` largest keys (O(n)),
    // only that chunk is sorted.  The visiting order is exactly the fully sorted order.
    unsigned int done = 0;
    const auto greater = [](unsigned long long a, unsigned long long b) { return a > b; };
    while (done < n) {
        const unsigned int chunk = std::min(n - done, 1024u);
        if (done + chunk < n) std::nth_element(k + done, k + done + chunk, k + n, greater);
        std::sort(k + done, k + done + chunk, greater);
        for (unsigned int i = done; i < done + chunk; i++) {
            const unsigned int idx = (unsigned int)(k[i] & 0xffffffffu);
            const int x = (int)(idx % w_), y = (int)(idx / w_);
            if (cell < 1) {
                xy.push_back((float)x), xy.push_back((float)y);
            } else {
                const int xc = x / cell, yc = y / cell;
                const int x1 = std::max(0, xc - 1), y1 = std::max(0, yc - 1), x2 = std::min(gw - 1, xc + 1), y2 = std::min(gh - 1, yc + 1);
                bool good = true;
                for (int yy = y1; yy <= y2 && good; yy++)
                    for (int xx = x1; xx <= x2 && good; xx++)
                        for (int j = grid_head_[(size_t)yy * gw + xx]; j >= 0; j = grid_next_[j]) {
                            const float dx = (float)x - xy[2 * j], dy = (float)y - xy[2 * j + 1];
                            if ((double)(dx * dx + dy * dy) < md2) {
                                good = false;
                                break;
                            }
                        }
                if (!good) continue;
                grid_next_.push_back(grid_head_[(size_t)yc * gw + xc]);
                grid_head_[(size_t)yc * gw + xc] = (int)(xy.size() / 2);
                xy.push_back((float)x), xy.push_back((float)y);
            }
            if (max_corners > 0 && (int)(xy.size() / 2) == max_corners) return;
        }
        done += chunk;
    }
}

vstab_status Tracker::select_from_keys(unsigned int n, int max_corners, double min_distance, std::vector<float> &xy, hipStream_t st) {
    if (n == 0) return VSTAB_OK;
    VSTAB_TRY(hkeys_.ensure(sizeof(unsigned long long) * n));
    VSTAB_HIP_TRY(hipMemcpyAsync(hkeys_.p, keys_.p, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, st));
    VSTAB_HIP_TRY(hipStreamSynchronize(st));
    select_corners(hkeys_.as<unsigned long long>(), n, max_corners, min_distance, xy);
    return VSTAB_OK;
}

vstab_status Tracker::good_features(const uint8_t *gray, size_t pitch, int max_corners, double quality, double min_distance, std::vector<float> &xy, hipStream_t st, float *eig_out) {
    xy.clear();
    float *eig = eig_out;
    int *max_bits = small_.as<int>();
    unsigned int *count = small_.as<unsigned int>() + 4;
    if (cap_ == 0) {
        cap_ = 1u << 18;
        VSTAB_TRY(keys_.ensure(sizeof(unsigned long long) * cap_));
    }
    if (!eig_out && !two_pass_detector_) {
        // one pass: eigenvalue, threshold and 3x3 maximum test fused, the eigenvalue map never stored
        VSTAB_TRY(raw_keys_.ensure(corners_fused_scratch_bytes(w_, h_)));
#ifdef VSTAB_DEV
        if (getenv("VSTAB_DEV_DET_TWICE")) VSTAB_TRY(launch_corners_fused(gray, pitch, w_, h_, quality, raw_keys_.p, keys_.as<unsigned long long>(), cap_, small_.as<unsigned int>(), st, mask_, mask_pitch_, harris_, harris_kf_));
#endif
        VSTAB_TRY(launch_corners_fused(gray, pitch, w_, h_, quality, raw_keys_.p, keys_.as<unsigned long long>(), cap_, small_.as<unsigned int>(), st, mask_, mask_pitch_,
                                       harris_, harris_kf_));
        VSTAB_HIP_TRY(hipMemcpyAsync(hsmall_.p, count, 2 * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
        if (harris_) VSTAB_HIP_TRY(hipMemcpyAsync(hsmall_.as<unsigned int>() + 2, small_.p, sizeof(unsigned int), hipMemcpyDeviceToHost, st));  // the biased maximum
        VSTAB_HIP_TRY(hipStreamSynchronize(st));
        // Harris: a maximum with the sign bit set (biased: below 2^31; 0 = no tile published one) means no response above zero, and no corner
        if (harris_ && hsmall_.as<unsigned int>()[2] < 0x80000000u) return VSTAB_OK;
        const unsigned int kept = hsmall_.as<unsigned int>()[0];
        if (kept <= cap_) return select_from_keys(kept, max_corners, min_distance, xy, st);
        fused_overflows_++;  // more corners above the threshold than the key buffer holds: the two-pass detector below grows it
    }
    VSTAB_TRY(eig_.ensure(sizeof(float) * (size_t)w_ * h_));
    if (!eig) eig = eig_.as<float>();
    if (harris_) VSTAB_TRY(launch_corner_harris(gray, pitch, w_, h_, harris_kf_, eig, max_bits, st));
    else VSTAB_TRY(launch_min_eig(gray, pitch, w_, h_, eig, max_bits, st));
    if (mask_) {  // the threshold of a masked detection comes from the maximum over the masked-in pixels: small_[1], beside the frame's
        VSTAB_TRY(launch_masked_max(eig, w_, h_, mask_, mask_pitch_, max_bits + 1, st));
        max_bits += 1;
    }
    if (harris_) {  // as above: the sign of the (masked) maximum, before a key buffer grows for candidates above a negative threshold
        VSTAB_HIP_TRY(hipMemcpyAsync(hsmall_.p, max_bits, sizeof(int), hipMemcpyDeviceToHost, st));
        VSTAB_HIP_TRY(hipStreamSynchronize(st));
        if (*hsmall_.as<int>() < 0) return VSTAB_OK;
    }
    unsigned int n = 0;
    for (int attempt = 0; attempt < 2; attempt++) {
        VSTAB_TRY(launch_corner_candidates(eig, w_, h_, max_bits, quality, keys_.as<unsigned long long>(), count, cap_, st, mask_, mask_pitch_));
        VSTAB_HIP_TRY(hipMemcpyAsync(hsmall_.p, count, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
        VSTAB_HIP_TRY(hipStreamSynchronize(st));
        n = *hsmall_.as<unsigned int>();
        if (n <= cap_) break;
        cap_ = n;  // more local maxima than the buffer holds: grow and re-run the compaction
        VSTAB_TRY(keys_.ensure(sizeof(unsigned long long) * cap_));
    }
    return select_from_keys(n, max_corners, min_distance, xy, st);
}

vstab_status Tracker::spec_launch(const uint8_t *gray, size_t pitch, double quality, hipStream_t st, long tag) {
    spec_join();  // (a previous asynchronous selection still reading the pinned buffer: never in practice)
    VSTAB_TRY(spec_raw_.ensure(corners_fused_scratch_bytes(w_, h_)));
    VSTAB_TRY(spec_keys_.ensure(sizeof(unsigned long long) * SPEC_CAP));
    VSTAB_TRY(spec_small_.ensure(256));
    VSTAB_TRY(spec_host_.ensure(64 + sizeof(unsigned long long) * SPEC_CAP));
    if (!spec_ev_) VSTAB_HIP_TRY(hipEventCreateWithFlags(&spec_ev_, hipEventDisableTiming));
    unsigned int *count = spec_small_.as<unsigned int>() + 4;
#ifdef VSTAB_DEV
    static const bool det_twice = getenv("VSTAB_DEV_DET_TWICE") != nullptr;  // sensitivity of the frame rate to the detector: everything twice, same result
    if (det_twice) VSTAB_TRY(launch_corners_fused(gray, pitch, w_, h_, quality, spec_raw_.p, spec_keys_.as<unsigned long long>(), SPEC_CAP, spec_small_.as<unsigned int>(), st, mask_, mask_pitch_, harris_, harris_kf_));
#endif
    VSTAB_TRY(launch_corners_fused(gray, pitch, w_, h_, quality, spec_raw_.p, spec_keys_.as<unsigned long long>(), SPEC_CAP, spec_small_.as<unsigned int>(), st, mask_, mask_pitch_,
                                   harris_, harris_kf_));
    VSTAB_HIP_TRY(hipMemcpyAsync(spec_host_.p, count, 2 * sizeof(unsigned int), hipMemcpyDeviceToHost, st));  // {keys kept, tiles that spilled}
    if (harris_) VSTAB_HIP_TRY(hipMemcpyAsync(spec_host_.as<unsigned int>() + 2, spec_small_.p, sizeof(unsigned int), hipMemcpyDeviceToHost, st));  // the biased maximum
    VSTAB_HIP_TRY(hipMemcpyAsync(spec_host_.as<uint8_t>() + 64, spec_keys_.p, sizeof(unsigned long long) * SPEC_CAP, hipMemcpyDeviceToHost, st));
    VSTAB_HIP_TRY(hipEventRecord(spec_ev_, st));
    spec_tag_ = tag;
    return VSTAB_OK;
}

int Tracker::spec_select(int max_corners, double min_distance, std::vector<float> &xy, unsigned int *n_seen) {
    unsigned int n = spec_host_.as<unsigned int>()[0];
    if (harris_ && spec_host_.as<unsigned int>()[2] < 0x80000000u) n = 0;  // no response above zero: no corner (good_features has the same test)
    if (n_seen) *n_seen = n;
    if (n > SPEC_CAP) {
        spec_over_cap_.fetch_add(1, std::memory_order_relaxed);
        return 3;
    }
    select_corners(reinterpret_cast<unsigned long long *>(spec_host_.as<uint8_t>() + 64), n, max_corners, min_distance, xy);
    return 2;
}

void Tracker::spec_select_async(int max_corners, double min_distance) {
    spec_join();
    spec_owner_.store(0, std::memory_order_release);  // nobody has taken this selection yet (the helper thread, or the caller: spec_poll_inline)
    spec_state_.store(1, std::memory_order_release);
    if (!spec_thread_started_) {
        spec_thread_started_ = true;
        int dev = 0;
        (void)hipGetDevice(&dev);
        spec_thread_ = std::thread([this, dev] {
            (void)hipSetDevice(dev);  // the handle's device, not the new thread's default
            std::unique_lock<std::mutex> lk(spec_m_);
            for (;;) {
                spec_cv_.wait(lk, [this] { return spec_job_ || spec_quit_; });
                if (spec_quit_) return;
                spec_job_ = false;
                {
                    // (development: VSTAB_SPEC_HELPER_DELAY_US=n makes this thread wake up late, so that a test reaches spec_poll_inline;
                    //  read ONCE, when the Tracker is constructed -- getenv beside a setenv of the host process is undefined behaviour)
                    const long late_us = spec_late_us_;
                    if (late_us > 0) {
                        lk.unlock();
                        std::this_thread::sleep_for(std::chrono::microseconds(late_us));
                        lk.lock();
                        if (spec_quit_) return;
                    }
                    int unclaimed = 0;  // the caller may have done this selection itself while this thread was waking up
                    if (!spec_owner_.compare_exchange_strong(unclaimed, 1, std::memory_order_acq_rel)) continue;
                    selections_by_helper_.fetch_add(1, std::memory_order_relaxed);
                }
                lk.unlock();
                int result = 3;
                const auto t0 = std::chrono::steady_clock::now();
                // poll instead of a blocking wait: the wake-up latency of hipEventSynchronize (hundreds of microseconds
                // on this runtime) would eat the lead the detection was given
                hipError_t q = hipErrorNotReady;
                if (spec_ev_) {
                    for (long spins = 0; (q = hipEventQuery(spec_ev_)) == hipErrorNotReady && spins < 4000000; spins++) __builtin_ia32_pause();
                    if (q == hipErrorNotReady) q = hipEventSynchronize(spec_ev_);
                }
                if (q == hipSuccess) {
                    const auto t1 = std::chrono::steady_clock::now();
                    unsigned int n = 0;
                    result = spec_select(spec_max_, spec_dist_, spec_xy_, &n);
                    if (debug_spec())
                        std::fprintf(stderr, "async selection: waited %.0f us for the detection, selected %zu of %u candidates in %.0f us\n",
                                     std::chrono::duration<double, std::micro>(t1 - t0).count(), spec_xy_.size() / 2, n,
                                     std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t1).count());
                }
                spec_state_.store(result, std::memory_order_release);
                lk.lock();
            }
        });
    }
    {
        std::lock_guard<std::mutex> lk(spec_m_);
        spec_max_ = max_corners, spec_dist_ = min_distance, spec_job_ = true;
    }
    spec_cv_.notify_one();
}

void Tracker::spec_poll_inline() {
    if (spec_state_.load(std::memory_order_acquire) != 1 || !spec_ev_ || hipEventQuery(spec_ev_) != hipSuccess) {
        (void)hipGetLastError();  // "not ready" is an answer, not an error the next launch check should find
        return;
    }
    int unclaimed = 0;
    if (!spec_owner_.compare_exchange_strong(unclaimed, 2, std::memory_order_acq_rel)) return;  // the helper thread has it
    selections_by_caller_++;
    unsigned int n = 0;
    const int result = spec_select(spec_max_, spec_dist_, spec_xy_, &n);
    if (debug_spec()) std::fprintf(stderr, "selection done by the caller (the helper thread had not woken up): %zu of %u candidates\n", spec_xy_.size() / 2, n);
    spec_state_.store(result, std::memory_order_release);
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
    a.clk = static_cast<unsigned long long *>(clock_slot());
    if (L.timed && !ev_a_) (void)hipEventCreate(&ev_a_), (void)hipEventCreate(&ev_b_);
    if (L.timed) (void)hipEventRecord(ev_a_, st);
    VSTAB_TRY(launch_lk(a, st));
    if (L.timed) (void)hipEventRecord(ev_b_, st);
    return VSTAB_OK;
}

}  // namespace vstab
