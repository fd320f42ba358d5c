// vstab_detect_host.hpp -- class Detector, the host side of goodFeaturesToTrack (defined in vstab_detect_host.cpp): used by the pipeline
// object beside its Tracker and by the stateless vstab_good_features*.  It knows nothing of pyramids or LK launches.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <mutex>
#include <thread>
#include <vector>

#include "vstab_internal.hpp"
#include "vstab_track.hpp"

namespace vstab {

inline bool debug_spec() {  // VSTAB_DEBUG_SPEC=1: the key-frame speculation narrated on stderr (development aid)
    static const bool on = getenv("VSTAB_DEBUG_SPEC") != nullptr;
    return on;
}

// "<fn>: block_size is 3, 5 or 7" for a block no kernel exists for
inline vstab_status check_corner_block(const std::string &fn, int block) {
    return corner_block_offered(block) ? VSTAB_OK : fail(VSTAB_ERR_INVALID, fn + ": block_size is 3, 5 or 7");
}

// "<fn>: gradient_size is 3, 5 or 7" for a gradient size no kernel exists for
inline vstab_status check_corner_gradient(const std::string &fn, int gradient) {
    return corner_gradient_offered(gradient) ? VSTAB_OK : fail(VSTAB_ERR_INVALID, fn + ": gradient_size is 3, 5 or 7");
}

// The DetectSpec of an entry point's arguments (mask NULL: none; harris false: k is not looked at), or its refusal under the name fn:
// the block, the gradient, the mask's pitch, then its size, then k -- on the double, before it is narrowed.
inline vstab_status check_detect_spec(const std::string &fn, const void *mask, size_t pitch_mask, bool harris, double k, int w, int h, DetectSpec &out, int block = 3,
                                      int gradient = 3) {
    VSTAB_TRY(check_corner_block(fn, block));
    VSTAB_TRY(check_corner_gradient(fn, gradient));
    if (mask && pitch_mask < (size_t)w) return fail(VSTAB_ERR_INVALID, fn + ": the mask's pitch is smaller than the image's width");
    if (mask && (uint64_t)pitch_mask * (uint64_t)h >= (1ull << 32)) return fail(VSTAB_ERR_INVALID, fn + ": mask planes of 4 GiB or more are not supported");
    if (harris && !harris_k_ok(k)) return fail(VSTAB_ERR_INVALID, fn + ": k lies in [0, 0.25)");
    out = DetectSpec(static_cast<const uint8_t *>(mask), pitch_mask, harris, (float)k, block, gradient);
    return VSTAB_OK;
}

class Detector {
  public:
    ~Detector();
    // the words and their host copy; every other buffer is allocated by the detection that first needs it
    vstab_status init(int w, int h);

    // goodFeaturesToTrack(gray, max_corners, quality, min_distance) under spec(); synchronises the stream.  eig_out (optional): the dense
    // response map, which only the two-pass detector has.  The host half is select_corners (vstab_hostlogic.hpp).
    vstab_status good_features(const uint8_t *gray, size_t pitch, int max_corners, double quality, double min_distance, std::vector<float> &xy, hipStream_t st, float *eig_out = nullptr);
    void set_two_pass_detector(bool on) { two_pass_detector_ = on; }

    // What every detection from now on reads beside the image -- good_features (fused, two-pass, the fall-back between them, and the map
    // it hands out through eig_out) and spec_launch.  Only while nothing is in flight.
    //   set_mask borrows the caller's plane; copy_mask keeps a copy in device memory of the Detector's own (base and pitch 4-byte aligned:
    //   the kernels' dword path) and returns when the copy is complete.
    //   set_response: under the Harris response a frame whose (masked) maximum is not positive has no corner, decided on the host from the
    //   sign of the maximum the kernels publish (no_positive_response).
    //   set_block: the window of the covariance sums; everything behind the response is the same for every size.
    //   set_gradient: the Sobel aperture of the derivatives; everything behind the products is the same for every size.
    const DetectSpec &spec() const { return spec_; }
    void set_mask(const uint8_t *mask, size_t pitch) { spec_ = DetectSpec(mask, pitch, spec_.harris, spec_.kf, spec_.block, spec_.gradient); }
    vstab_status copy_mask(const void *mask, size_t pitch, bool host);
    void set_response(bool harris, float kf) { spec_ = DetectSpec(spec_.mask, spec_.mask_pitch, harris, kf, spec_.block, spec_.gradient); }
    void set_block(int block) { spec_.block = block; }  // 3, 5 or 7 (check_corner_block)
    void set_gradient(int gradient) { spec_.gradient = gradient; }  // 3, 5 or 7 (check_corner_gradient)

    // Speculative detection: the same two kernels enqueued on another stream ahead of time (the counter
    // half of the key-frame rule is predictable), with the words and the first SPEC_CAP keys copied to
    // pinned memory behind them.  spec_finish() only has to wait for the event and run the host half.
    static constexpr unsigned int SPEC_CAP = 1u << 15;
    vstab_status spec_launch(const uint8_t *gray, size_t pitch, double quality, hipStream_t st, long tag);
    long spec_tag() const { return spec_tag_; }
    // Host half of the speculative detection on a helper thread: waits for the kernels' results and runs the
    // sort + minimum-distance pass, so that by the time the key frame comes its corners are simply there.
    void spec_select_async(int max_corners, double min_distance);
    // The helper thread sleeps on a condition variable between two detections (720 us apart at 4K); on a busy host its wake-up can take
    // longer than the detection itself.  Whoever looks for the corners first while the job is still unclaimed and the detection's event
    // has completed does the selection on the spot (45 us of host time instead of a wait for another thread's wake-up).
    void spec_poll_inline();
    // 0 = no asynchronous selection, 1 = running, 2 = corners ready, 3 = failed (candidate overflow / device error)
    int spec_state() const { return spec_state_.load(std::memory_order_acquire); }
    void spec_join() {
        while (spec_state_.load(std::memory_order_acquire) == 1) std::this_thread::yield();
    }
    // take the asynchronously selected corners (state must be 2)
    void spec_take(std::vector<float> &xy) {
        xy = spec_xy_;
        spec_state_.store(0, std::memory_order_release), spec_tag_ = -1;
    }
    // returns true and fills xy if the speculative result is usable (candidate count within SPEC_CAP)
    bool spec_finish(int max_corners, double min_distance, std::vector<float> &xy) {
        if (spec_state() != 0) {  // the helper thread has (or is about to have) the answer -- or nobody yet: then this thread, if the kernels are through
            spec_poll_inline();
            spec_join();
            const bool ok = spec_state() == 2;
            if (ok) xy = spec_xy_;
            spec_state_.store(0, std::memory_order_release), spec_tag_ = -1;
            return ok;
        }
        spec_tag_ = -1;
        if (!spec_ev_ || hipEventSynchronize(spec_ev_) != hipSuccess) return false;
        return spec_select(max_corners, min_distance, xy) == 2;
    }

    long selections_by_caller() const { return selections_by_caller_; }
    long selections_by_helper() const { return selections_by_helper_.load(std::memory_order_relaxed); }
    long fused_overflows() const { return fused_overflows_; }
    // (vstabx_detector_counters) speculative selections that found more than SPEC_CAP candidates; the key capacity of good_features now
    long spec_over_cap() const { return spec_over_cap_.load(std::memory_order_relaxed); }
    unsigned int key_capacity() const { return cap_; }

  private:
    // launch_corners_fused under spec_ (a development build with VSTAB_DEV_DET_TWICE set: twice, same result -- the sensitivity of the
    // frame rate to the detector)
    vstab_status launch_fused(const uint8_t *gray, size_t pitch, double quality, void *scratch, unsigned long long *keys, unsigned int cap, DetectorWords *words, hipStream_t st);
    // the words to hsmall_ (synchronises the stream)
    vstab_status read_words(hipStream_t st);
    // host half of a finished speculative detection: the corners into xy and spec_state's 2, or 3 for more candidates than SPEC_CAP; *n_seen = their count
    int spec_select(int max_corners, double min_distance, std::vector<float> &xy, unsigned int *n_seen = nullptr);
    // the tail of good_features: the first n keys of keys_ to the host (synchronises the stream), then select_corners
    vstab_status select_from_keys(unsigned int n, int max_corners, double min_distance, std::vector<float> &xy, hipStream_t st);

    static constexpr size_t SPEC_KEYS_OFF = 64;  // spec_host_: the words, then (at this offset) SPEC_CAP keys
    int w_ = 0, h_ = 0;
    DetectSpec spec_;    // the mask in force (mask_buf_'s, or a caller's) and the response
    DevBuf mask_buf_;
    bool two_pass_detector_ = false;
    DevBuf eig_, keys_, small_, raw_keys_;  // small_: DetectorWords
    PinnedBuf hsmall_, hkeys_;
    unsigned int cap_ = 0;
    long fused_overflows_ = 0;
    DevBuf spec_raw_, spec_keys_, spec_small_;
    PinnedBuf spec_host_;
    hipEvent_t spec_ev_ = nullptr;
    long spec_tag_ = -1;
    std::thread spec_thread_;
    bool spec_thread_started_ = false, spec_job_ = false, spec_quit_ = false;
    std::mutex spec_m_;
    std::condition_variable spec_cv_;
    std::atomic<int> spec_state_{0};
    std::atomic<int> spec_owner_{0};  // who runs the posted selection: 0 nobody yet, 1 the helper thread, 2 the caller (spec_poll_inline)
    const long spec_late_us_ = getenv("VSTAB_SPEC_HELPER_DELAY_US") ? atol(getenv("VSTAB_SPEC_HELPER_DELAY_US")) : 0;  // development: the helper wakes up late
    long selections_by_caller_ = 0;                 // speculative detections whose corners the caller selected itself / the helper thread selected
    std::atomic<long> selections_by_helper_{0};
    std::atomic<long> spec_over_cap_{0};            // selections (by either thread) that ended in state 3 for their count
    int spec_max_ = 200;
    double spec_dist_ = 30.0;
    std::vector<float> spec_xy_;
};

}  // namespace vstab
