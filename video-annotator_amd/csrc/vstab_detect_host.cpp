// vstab_detect_host.cpp -- class Detector (vstab_detect_host.hpp): the one-pass and the two-pass detector with the fall-back between them,
// the detection mask and the response in force, and the speculative detection with its helper thread.  Host C++; the kernels are those of
// vstab_corners_fused.hip and vstab_corners.hip, the sort and the minimum-distance pass are select_corners (vstab_hostlogic.hpp).
#include <chrono>

#include "vstab_detect_host.hpp"
#include "vstab_hostlogic.hpp"

namespace vstab {

Detector::~Detector() {
    // the helper thread polls spec_ev_ while a selection is running: stop and join it BEFORE the event goes
    if (spec_thread_started_) {
        {
            std::lock_guard<std::mutex> lk(spec_m_);
            spec_quit_ = true;
        }
        spec_cv_.notify_one();
        spec_thread_.join();
    }
    if (spec_ev_) (void)hipEventDestroy(spec_ev_);
}

vstab_status Detector::init(int w, int h) {
    w_ = w, h_ = h;
    VSTAB_TRY(small_.ensure(256));
    VSTAB_TRY(hsmall_.ensure(256));
    return VSTAB_OK;
}

vstab_status Detector::copy_mask(const void *mask, size_t pitch, bool host) {
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

vstab_status Detector::launch_fused(const uint8_t *gray, size_t pitch, double quality, void *scratch, unsigned long long *keys, unsigned int cap, DetectorWords *words,
                                    hipStream_t st) {
#ifdef VSTAB_DEV
    static const bool det_twice = getenv("VSTAB_DEV_DET_TWICE") != nullptr;
    if (det_twice) VSTAB_TRY(launch_corners_fused(gray, pitch, w_, h_, quality, scratch, keys, cap, words, st, spec_));
#endif
    return launch_corners_fused(gray, pitch, w_, h_, quality, scratch, keys, cap, words, st, spec_);
}

vstab_status Detector::read_words(hipStream_t st) {
    VSTAB_HIP_TRY(hipMemcpyAsync(hsmall_.p, small_.p, sizeof(DetectorWords), hipMemcpyDeviceToHost, st));
    VSTAB_HIP_TRY(hipStreamSynchronize(st));
    return VSTAB_OK;
}

vstab_status Detector::select_from_keys(unsigned int n, int max_corners, double min_distance, std::vector<float> &xy, hipStream_t st) {
    if (n == 0) return VSTAB_OK;
    VSTAB_TRY(hkeys_.ensure(sizeof(unsigned long long) * n));
    VSTAB_HIP_TRY(hipMemcpyAsync(hkeys_.p, keys_.p, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, st));
    VSTAB_HIP_TRY(hipStreamSynchronize(st));
    select_corners(hkeys_.as<unsigned long long>(), n, w_, h_, max_corners, min_distance, xy);
    return VSTAB_OK;
}

vstab_status Detector::good_features(const uint8_t *gray, size_t pitch, int max_corners, double quality, double min_distance, std::vector<float> &xy, hipStream_t st, float *eig_out) {
    xy.clear();
    DetectorWords *words = small_.as<DetectorWords>();
    const DetectorWords &seen = *hsmall_.as<DetectorWords>();  // what read_words brought back
    if (cap_ == 0) {
        cap_ = 1u << 18;
        VSTAB_TRY(keys_.ensure(sizeof(unsigned long long) * cap_));
    }
    if (!eig_out && !two_pass_detector_) {
        // one pass: response, threshold and 3x3 maximum test fused, the response map never stored
        VSTAB_TRY(raw_keys_.ensure(corners_fused_scratch_bytes(w_, h_)));
        VSTAB_TRY(launch_fused(gray, pitch, quality, raw_keys_.p, keys_.as<unsigned long long>(), cap_, words, st));
        VSTAB_TRY(read_words(st));
        if (spec_.harris && no_positive_response(seen.max, true)) return VSTAB_OK;
        if (seen.kept <= cap_) return select_from_keys(seen.kept, max_corners, min_distance, xy, st);
        fused_overflows_++;  // more corners above the threshold than the key buffer holds: the two-pass detector below grows it
    }
    VSTAB_TRY(eig_.ensure(sizeof(float) * (size_t)w_ * h_));
    float *eig = eig_out ? eig_out : eig_.as<float>();
    // the threshold of a masked detection comes from the maximum over the masked-in pixels, a word beside the frame's
    unsigned int DetectorWords::*const max_word = spec_.mask ? &DetectorWords::masked_max : &DetectorWords::max;
    VSTAB_TRY(launch_corner_response(gray, pitch, w_, h_, spec_.harris, spec_.kf, eig, reinterpret_cast<int *>(&words->max), st, spec_.block, spec_.gradient));
    if (spec_.mask) VSTAB_TRY(launch_masked_max(eig, w_, h_, spec_.mask, spec_.mask_pitch, reinterpret_cast<int *>(&words->masked_max), st));
    if (spec_.harris) {  // as above: the sign of the (masked) maximum, before a key buffer grows for candidates above a negative threshold
        VSTAB_TRY(read_words(st));
        if (no_positive_response(seen.*max_word, false)) return VSTAB_OK;
    }
    for (int attempt = 0; attempt < 2; attempt++) {
        VSTAB_TRY(launch_corner_candidates(eig, w_, h_, reinterpret_cast<const int *>(&(words->*max_word)), quality, keys_.as<unsigned long long>(), &words->kept, cap_, st, spec_));
        VSTAB_TRY(read_words(st));
        if (seen.kept <= cap_) break;
        cap_ = seen.kept;  // more local maxima than the buffer holds: grow and re-run the compaction
        VSTAB_TRY(keys_.ensure(sizeof(unsigned long long) * cap_));
    }
    return select_from_keys(seen.kept, max_corners, min_distance, xy, st);
}

vstab_status Detector::spec_launch(const uint8_t *gray, size_t pitch, double quality, hipStream_t st, long tag) {
    spec_join();  // (a previous asynchronous selection still reading the pinned buffer: never in practice)
    VSTAB_TRY(spec_raw_.ensure(corners_fused_scratch_bytes(w_, h_)));
    VSTAB_TRY(spec_keys_.ensure(sizeof(unsigned long long) * SPEC_CAP));
    VSTAB_TRY(spec_small_.ensure(256));
    VSTAB_TRY(spec_host_.ensure(SPEC_KEYS_OFF + sizeof(unsigned long long) * SPEC_CAP));
    if (!spec_ev_) VSTAB_HIP_TRY(hipEventCreateWithFlags(&spec_ev_, hipEventDisableTiming));
    VSTAB_TRY(launch_fused(gray, pitch, quality, spec_raw_.p, spec_keys_.as<unsigned long long>(), SPEC_CAP, spec_small_.as<DetectorWords>(), st));
    VSTAB_HIP_TRY(hipMemcpyAsync(spec_host_.p, spec_small_.p, sizeof(DetectorWords), hipMemcpyDeviceToHost, st));
    VSTAB_HIP_TRY(hipMemcpyAsync(spec_host_.as<uint8_t>() + SPEC_KEYS_OFF, spec_keys_.p, sizeof(unsigned long long) * SPEC_CAP, hipMemcpyDeviceToHost, st));
    VSTAB_HIP_TRY(hipEventRecord(spec_ev_, st));
    spec_tag_ = tag;
    return VSTAB_OK;
}

int Detector::spec_select(int max_corners, double min_distance, std::vector<float> &xy, unsigned int *n_seen) {
    const DetectorWords &seen = *spec_host_.as<DetectorWords>();
    const unsigned int n = spec_.harris && no_positive_response(seen.max, true) ? 0 : seen.kept;  // (good_features has the same test)
    if (n_seen) *n_seen = n;
    if (n > SPEC_CAP) {
        spec_over_cap_.fetch_add(1, std::memory_order_relaxed);
        return 3;
    }
    select_corners(reinterpret_cast<unsigned long long *>(spec_host_.as<uint8_t>() + SPEC_KEYS_OFF), n, w_, h_, max_corners, min_distance, xy);
    return 2;
}

void Detector::spec_select_async(int max_corners, double min_distance) {
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
                    //  read ONCE, when the Detector is constructed -- getenv beside a setenv of the host process is undefined behaviour)
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

void Detector::spec_poll_inline() {
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

}  // namespace vstab
