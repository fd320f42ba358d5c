// vstab_track_host.hpp -- class Tracker, the host side of the LK tracker (defined in vstab_track_host.cpp): used by the pipeline object, the
// stateless vstab_pyr_lk and the vstabx_lk_segments hook.  The corner detector beside it is class Detector (vstab_detect_host.hpp).
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vstab_internal.hpp"
#include "vstab_track.hpp"

namespace vstab {

// ---------------------------------------------------------------------------------------------
// Tracker: device workspace for calcOpticalFlowPyrLK
// ---------------------------------------------------------------------------------------------
constexpr int PREFETCH_MAX = 16;             // upper bound of the read-ahead (the ring and the pyramid sets are sized for it)
constexpr int PYR_SETS = PREFETCH_MAX + 2;  // previous + current (in flight) + the prefetched frames
#ifdef VSTAB_DEV
constexpr int PYR_DEV_EXTRA = 1;  // a set nobody reads: VSTAB_DEV_PYR_TWICE=1 builds every pyramid a second time into it (sensitivity of the frame rate to the pyramid kernels)
#else
constexpr int PYR_DEV_EXTRA = 0;
#endif

// The tracker's options as vstab_pyr_lk_ex and vstab_set_tracker_options take them (vstab.h, "Tracker options"): refused with
// "<fn>: max_level lies in 0 .. 3", "<fn>: max_iter lies in 1 .. 100", "<fn>: eps is finite and lies in [0, 10]" and
// "<fn>: min_eig_threshold is finite and not negative", in this order (a NaN fails every comparison).
vstab_status check_lk_options(const char *fn, int max_level, int max_iter, double eps, double min_eig_threshold, LkOptions &out);

class Tracker {
  public:
    // One record buffer per tracked frame pair, in rotation: a launch covers up to LK_SEG_MAX pairs and launches run up to
    // PREFETCH_DEPTH frames ahead of the frame the host reads, so a buffer comes round again long after its reader is done
    // (and after any launch whose results were dropped has finished: it precedes its replacement on the tracker stream).
    static constexpr int REC_BUFS = 32, PTS_BUFS = 8;
    ~Tracker();
    vstab_status init(int w, int h, const LkOptions &opt = LkOptions());
    // the options of every launch from here on; the pyramids get min(lk_levels(w, h, window), max_level + 1) levels, so fewer levels are
    // fewer pyramid launches.  Only while nothing is in flight (before the first launch).  The window is set_window's: opt.win is not read.
    void set_options(const LkOptions &opt) {
        const int win = opt_.win;
        opt_ = opt, opt_.win = win;
        levels_ = std::min(lk_levels(w_, h_, win), opt.max_level + 1);
    }
    // the window of every launch from here on (vstab.h, "Tracker window"; the caller checked lk_window_offered), independent of
    // set_options and in either order with it.  A smaller window can mean a deeper pyramid than init() allocated: the level buffers of
    // every set are brought up to lk_levels(w, h, win).  Only while nothing is in flight.  A failed allocation leaves the tracker as it was.
    vstab_status set_window(int win);
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

    // One pair from host points with the stateless-only arguments (vstab.h, "Tracker options", rules 2, 5 and 6): guess_xy, n host pairs
    // read iff flags has VSTAB_LK_USE_INITIAL_FLOW; err, n host floats or NULL, filled behind a synchronisation of the stream.
    vstab_status track_ex(const LkPyramid &I, const LkPyramid &J, const std::vector<float> &prev_xy, const float *guess_xy, int flags, float *err,
                          std::vector<float> &next_xy, std::vector<uint8_t> &status, hipStream_t st);

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
    vstab_status ensure_levels(int n);
    vstab_status launch_segment(const LkPyramid *pyr, int n_frames, const float2 *prev_pts, const void *chain_in, uint32_t parent_seq, hipStream_t st, Launch &L);
    int w_ = 0, h_ = 0, levels_ = 1;
    LkOptions opt_;
    DevBuf guess_, err_;  // track_ex: the guesses and the error measures of its one launch ...
    int ex_flags_ = 0;    // ... and what launch_segment hands to that launch (zero for every other launch)
    const float2 *ex_guess_ = nullptr;
    float *ex_err_ = nullptr;
    int lvl_w_[LK_MAX_LEVELS] = {0}, lvl_h_[LK_MAX_LEVELS] = {0};
    DevBuf pyr_[PYR_SETS + PYR_DEV_EXTRA][LK_MAX_LEVELS];  // pyramid sets: previous, current, prefetched x2
    const bool single_level_pyramid_ = getenv("VSTAB_PYR_SINGLE") != nullptr;  // development: one launch per pyramid level
    static constexpr int CLK_N = 4096;
    DevBuf clk_;
    int clk_used_ = 0;
    PinnedBuf hpts_[PTS_BUFS], hrec_[REC_BUFS];
    DevBuf drec_[REC_BUFS];
    hipEvent_t ev_a_ = nullptr, ev_b_ = nullptr;
    unsigned long rec_next_ = 0, pts_launches_ = 0;
    uint32_t seq_ = 0;
};

}  // namespace vstab
