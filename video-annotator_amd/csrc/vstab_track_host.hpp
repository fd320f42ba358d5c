// vstab_track_host.hpp -- class Tracker, the host side of the tracker (defined in vstab_track_host.cpp): used by the pipeline object, the
// stateless vstab_good_features* / vstab_pyr_lk and the vstabx_lk_segments hook.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
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

// ---------------------------------------------------------------------------------------------
// Tracker: device workspace for goodFeaturesToTrack + calcOpticalFlowPyrLK
// ---------------------------------------------------------------------------------------------
constexpr int PREFETCH_MAX = 16;             // upper bound of the read-ahead (the ring and the pyramid sets are sized for it)
constexpr int PYR_SETS = PREFETCH_MAX + 2;  // previous + current (in flight) + the prefetched frames
#ifdef VSTAB_DEV
constexpr int PYR_DEV_EXTRA = 1;  // a set nobody reads: VSTAB_DEV_PYR_TWICE=1 builds every pyramid a second time into it (sensitivity of the frame rate to the pyramid kernels)
#else
constexpr int PYR_DEV_EXTRA = 0;
#endif

class Tracker {
  public:
    // One record buffer per tracked frame pair, in rotation: a launch covers up to LK_SEG_MAX pairs and launches run up to
    // PREFETCH_DEPTH frames ahead of the frame the host reads, so a buffer comes round again long after its reader is done
    // (and after any launch whose results were dropped has finished: it precedes its replacement on the tracker stream).
    static constexpr int REC_BUFS = 32, PTS_BUFS = 8;
    ~Tracker();
    vstab_status init(int w, int h);
    // levels 1.. of the pyramid of `gray` into slot s (level 0 is the frame itself)
    // `done` (optional) completes with the LAST kernel of the pyramid, bound to that launch (launch_pyr_down); *done_bound says whether a kernel
    // took it (an image too small for a second level has no pyramid kernel: the caller records the event itself)
    // level 1 of set s, for a caller that fills it itself (launch_pack_pyr: the copy into the ring and the first level in one launch)
    uint8_t *level1(int s) { return levels_ >= 2 ? pyr_[s][1].as<uint8_t>() : nullptr; }
    size_t level1_pitch() const { return (size_t)lvl_w_[1]; }
    vstab_status build_pyramid(int s, const uint8_t *gray, size_t pitch, hipStream_t st, hipEvent_t done = nullptr, bool *done_bound = nullptr, bool have_level1 = false);

    LkPyramid pyramid(int s, const uint8_t *gray, size_t pitch) const {
        LkPyramid p;
        p.levels = levels_;
        for (int l = 0; l < LK_MAX_LEVELS; l++) p.img[l] = nullptr, p.pitch[l] = 0, p.w[l] = p.h[l] = 0;
        p.img[0] = gray, p.pitch[0] = pitch, p.w[0] = w_, p.h[0] = h_;
        for (int l = 1; l < levels_; l++) p.img[l] = pyr_[s][l].as<uint8_t>(), p.pitch[l] = (size_t)lvl_w_[l], p.w[l] = lvl_w_[l], p.h[l] = lvl_h_[l];
        return p;
    }

    // host half of goodFeaturesToTrack: sort the candidate keys (value descending, ties -> later raster
    // position first: greaterThanPtr in OpenCV) and run the minimum-distance grid
    void select_corners(unsigned long long *k, unsigned int n, int max_corners, double min_distance, std::vector<float> &xy);
    // goodFeaturesToTrack(gray, max_corners, quality, min_distance); synchronises the stream
    vstab_status good_features(const uint8_t *gray, size_t pitch, int max_corners, double quality, double min_distance, std::vector<float> &xy, hipStream_t st, float *eig_out = nullptr);

    // Speculative detection: the same two kernels enqueued on another stream ahead of time (the counter
    // half of the key-frame rule is predictable), with the count and the first SPEC_CAP keys copied to
    // pinned memory behind them.  spec_finish() only has to wait for the event and run the host half.
    static constexpr unsigned int SPEC_CAP = 1u << 15;
    vstab_status spec_launch(const uint8_t *gray, size_t pitch, double quality, hipStream_t st, long tag);
    long spec_tag() const { return spec_tag_; }
    long selections_by_caller() const { return selections_by_caller_; }
    long selections_by_helper() const { return selections_by_helper_.load(std::memory_order_relaxed); }
    void set_two_pass_detector(bool on) { two_pass_detector_ = on; }
    // The detection mask (vstab.h, "Detection mask"): a device plane of w x h bytes, non-zero = "a corner may be reported here", read by
    // every detection from now on -- good_features (fused, two-pass and the fall-back between them) and spec_launch.  NULL: no mask, the
    // launches of the unmasked detector.  set_mask borrows the caller's plane; copy_mask keeps a copy in device memory of the Tracker's
    // own (base and pitch 4-byte aligned: the kernels' dword path) and returns when the copy is complete.  Only while nothing is in flight.
    void set_mask(const uint8_t *mask, size_t pitch) { mask_ = mask, mask_pitch_ = mask ? pitch : 0; }
    vstab_status copy_mask(const void *mask, size_t pitch, bool host);
    const uint8_t *mask() const { return mask_; }
    size_t mask_pitch() const { return mask_pitch_; }
    // The corner response (vstab.h, "Harris response"): harris = false is cornerMinEigenVal(3, 3), the Tracker as it always was (kf is
    // not looked at); harris = true is cornerHarris(3, 3, k) with kf = (float)k, read by every detection from now on -- good_features (its
    // three paths, and the map it hands out through eig_out) and spec_launch.  Under it a frame whose (masked) maximum is not positive has
    // no corner: decided on the host from the sign of the maximum the kernels publish.  Only while nothing is in flight.
    void set_response(bool harris, float kf) { harris_ = harris, harris_kf_ = harris ? kf : 0.0f; }
    long fused_overflows() const { return fused_overflows_; }
    // (vstabx_detector_counters) speculative selections that found more than SPEC_CAP candidates; the key capacity of good_features now
    long spec_over_cap() const { return spec_over_cap_.load(std::memory_order_relaxed); }
    unsigned int key_capacity() const { return cap_; }
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

    // calcOpticalFlowPyrLK(prev, next, pts), split in two so the caller can enqueue more work behind the
    // kernel before blocking.  Points travel through mapped host memory: the kernel reads prev_pts and
    // writes one self-validating record per feature over the link directly (a few KB), and the host polls
    // the records' sequence tags instead of paying a copy launch + stream-sync round trip.
    //
    // A launch is a SEGMENT of consecutive frame pairs (k_lk_track): pair i tracks from pyramid i into pyramid i + 1, every
    // slot starts pair i + 1 from the point it reached in pair i (FrameSourceWarp.cpp:427) and lost slots stay lost.
    // Chained launches: a segment that continues where another ended reads its start points from the device copy of the
    // parent's last records, so it can be enqueued without waiting for the host.
    struct Launch {
        int n_slots = 0, n_frames = 0;
        int buf[LK_SEG_MAX] = {0};        // record buffer of every frame pair
        uint32_t seq[LK_SEG_MAX] = {0};   // and its sequence tag
        bool chained = false, timed = false;
    };

    // pyr: n_frames + 1 pyramids (the frame before the segment's first, then the segment's frames)
    vstab_status track_launch(const LkPyramid *pyr, int n_frames, const std::vector<float> &prev_xy, hipStream_t st, bool timed, Launch &L) {
        L = Launch();
        L.n_slots = (int)(prev_xy.size() / 2), L.timed = timed;
        if (L.n_slots == 0) return VSTAB_OK;
        PinnedBuf &pts = hpts_[pts_launches_++ % PTS_BUFS];  // one per launch: a launch still queued keeps its points
        VSTAB_TRY(pts.ensure((size_t)L.n_slots * sizeof(float2)));
        if (!pts.dev()) return fail(VSTAB_ERR_DEVICE, "hipHostGetDevicePointer failed");
        std::memcpy(pts.p, prev_xy.data(), sizeof(float) * prev_xy.size());
        return launch_segment(pyr, n_frames, static_cast<const float2 *>(pts.dev()), nullptr, 0, st, L);
    }
    // the launch for the frames FOLLOWING `parent`'s last one, chained behind it on the same stream (same slots; see above)
    vstab_status track_launch_chained(const LkPyramid *pyr, int n_frames, const Launch &parent, hipStream_t st, Launch &L) {
        L = Launch();
        if (parent.n_slots == 0 || parent.n_frames == 0) return VSTAB_OK;
        L.n_slots = parent.n_slots, L.chained = true;
        const int last = parent.n_frames - 1;
        return launch_segment(pyr, n_frames, nullptr, drec_[parent.buf[last]].p, parent.seq[last], st, L);
    }

    // results of frame pair `idx` of launch L in the order of the (compacted) point list it tracked: expect_n entries
    vstab_status track_wait(const Launch &L, int idx, size_t expect_n, std::vector<float> &next_xy, std::vector<uint8_t> &status, hipStream_t st, double *gpu_ms);
    vstab_status track(const LkPyramid &I, const LkPyramid &J, const std::vector<float> &prev_xy, std::vector<float> &next_xy, std::vector<uint8_t> &status, hipStream_t st,
                       double *gpu_ms = nullptr) {
        Launch L;
        const LkPyramid pyr[2] = {I, J};
        VSTAB_TRY(track_launch(pyr, 1, prev_xy, st, gpu_ms != nullptr, L));
        return track_wait(L, 0, prev_xy.size() / 2, next_xy, status, st, gpu_ms);
    }

    int levels() const { return levels_; }
    int level_w(int l) const { return lvl_w_[l]; }
    int level_h(int l) const { return lvl_h_[l]; }

    // record and point buffers for n slots, device records zeroed as init() zeroes them for 256 (vstabx_lk_segments: more slots than the pipeline's)
    vstab_status reserve_slots(int n) {
        for (int b = 0; b < REC_BUFS; b++) {
            VSTAB_TRY(hrec_[b].ensure((size_t)n * 16));
            VSTAB_TRY(drec_[b].ensure((size_t)n * 16));
            VSTAB_HIP_TRY(hipMemset(drec_[b].p, 0, drec_[b].n));
        }
        for (int b = 0; b < PTS_BUFS; b++) VSTAB_TRY(hpts_[b].ensure((size_t)n * sizeof(float2)));
        return VSTAB_OK;
    }
    // the host (mapped) and device records of frame pair idx of launch L
    const void *host_records(const Launch &L, int idx) const { return hrec_[L.buf[idx]].p; }
    const void *dev_records(const Launch &L, int idx) const { return drec_[L.buf[idx]].p; }

    // VSTAB_LK_CLOCK=1 (development aid): every LK launch stamps its first-workgroup start and last-workgroup end
    // (100 MHz wall clock) into a slot of a mapped ring; report_clock() prints durations and start-to-start gaps
    void *clock_slot();
    void report_clock();

  private:
    vstab_status launch_segment(const LkPyramid *pyr, int n_frames, const float2 *prev_pts, const void *chain_in, uint32_t parent_seq, hipStream_t st, Launch &L);
    // host half of a finished speculative detection: the corners into xy and spec_state's 2, or 3 for more candidates than SPEC_CAP; *n_seen = their count
    int spec_select(int max_corners, double min_distance, std::vector<float> &xy, unsigned int *n_seen = nullptr);
    // the tail of good_features: the first n keys of keys_ to the host (synchronises the stream), then select_corners
    vstab_status select_from_keys(unsigned int n, int max_corners, double min_distance, std::vector<float> &xy, hipStream_t st);

    int w_ = 0, h_ = 0, levels_ = 1;
    int lvl_w_[LK_MAX_LEVELS] = {0}, lvl_h_[LK_MAX_LEVELS] = {0};
    DevBuf pyr_[PYR_SETS + PYR_DEV_EXTRA][LK_MAX_LEVELS], eig_, keys_, small_;  // pyramid sets: previous, current, prefetched x2
    DevBuf spec_raw_, spec_keys_, spec_small_, raw_keys_;
    bool two_pass_detector_ = false;
    const uint8_t *mask_ = nullptr;  // the detection mask in force (mask_buf_'s, or a caller's), NULL for none
    size_t mask_pitch_ = 0;
    DevBuf mask_buf_;
    bool harris_ = false;  // the response in force: cornerHarris(3, 3, k) with harris_kf_ = (float)k, or cornerMinEigenVal(3, 3)
    float harris_kf_ = 0.0f;
    const bool single_level_pyramid_ = getenv("VSTAB_PYR_SINGLE") != nullptr;  // development: one launch per pyramid level
    long fused_overflows_ = 0;
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
    static constexpr int CLK_N = 4096;
    DevBuf clk_;
    int clk_used_ = 0;
    PinnedBuf hsmall_, hkeys_, hpts_[PTS_BUFS], hrec_[REC_BUFS];
    DevBuf drec_[REC_BUFS];
    unsigned int cap_ = 0;
    hipEvent_t ev_a_ = nullptr, ev_b_ = nullptr;
    unsigned long rec_next_ = 0, pts_launches_ = 0;
    uint32_t seq_ = 0;
};

}  // namespace vstab
