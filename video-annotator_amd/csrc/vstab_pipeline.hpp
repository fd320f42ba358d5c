// vstab_pipeline.hpp -- what vstab_pipeline.cpp and vstab_pull.cpp share (internal): the handle with its worker thread, the profiler's
// and the host timers' scopes, and the steps of consume_frame.
#pragma once
#include <chrono>
#include <cstdlib>
#include <deque>
#include <memory>

#include "vstab_detect_host.hpp"
#include "vstab_hostlogic.hpp"
#include "vstab_motion.hpp"
#include "vstab_track_host.hpp"

namespace vstab {

// frames pulled from upstream ahead of the one being tracked: deep enough that the speculative corner detection of a
// key frame (137 us of kernels beside everything else + the host selection) is finished before its turn comes
// default read-ahead; VSTAB_PREFETCH=n (1 .. PREFETCH_MAX) for experiments.  Twelve since the end of round 4 (eight before): the rates are the
// same, but the speculative corner detection launched when the frame before a planned key frame is read ahead then has ~430 us at 4K for
// its ~150 + 45 us beside the saturating warp instead of ~290 -- the margin that keeps a slow box from waiting for corners at key frames
constexpr int PREFETCH_DEPTH = 12;

inline const char *resample_name(int resample) { return resample == VSTAB_RESAMPLE_CUBIC ? "VSTAB_RESAMPLE_CUBIC" : "VSTAB_RESAMPLE_LANCZOS4"; }  // (for messages; vstab_create admits no third resampler)

// ---------------------------------------------------------------------------------------------
// EstimateWorker: one helper thread per handle that runs guess_camera_rotation's arithmetic
// (estimate_rotation: undistortion, RANSAC, LM refit -- pure host code on <= 200 points) while the
// calling thread issues the next frame's HIP launches.  One job at a time, posted and joined by the
// calling thread inside the same vstab_pull_frame call, so results are applied in frame order.  The
// worker spins briefly for the next job (the pipeline posts one every ~60 us) and then sleeps.
// ---------------------------------------------------------------------------------------------
class EstimateWorker {
  public:
    ~EstimateWorker() {
        if (th_.joinable()) {
            {
                std::lock_guard<std::mutex> lk(m_);
                state_.store(QUIT, std::memory_order_release);
            }
            cv_.notify_one();
            th_.join();
        }
    }
    void post(const float *prev, const float *cur, int n, const Mat3 *Kin, const Mat3 *Kout, Pcg32 *rng, bool in_fish, const double *D) {
        if (!th_.joinable()) th_ = std::thread([this] { run(); });
        prev_ = prev, cur_ = cur, n_ = n, Kin_ = Kin, Kout_ = Kout, rng_ = rng, in_fish_ = in_fish, D_ = D;
        {
            std::lock_guard<std::mutex> lk(m_);
            state_.store(POSTED, std::memory_order_release);
        }
        cv_.notify_one();
    }
    int join(Mat3 &R) {  // blocks until the posted job is done
        for (long spins = 0; state_.load(std::memory_order_acquire) != DONE; spins++) {
            if (spins < 200000) __builtin_ia32_pause();
            else std::this_thread::yield();
        }
        state_.store(IDLE, std::memory_order_relaxed);
        R = R_;
        return inliers_;
    }

  private:
    enum { IDLE = 0, POSTED = 1, DONE = 2, QUIT = 3 };
    void run() {
        for (;;) {
            int st = state_.load(std::memory_order_acquire);
            for (int spins = 0; st != POSTED && st != QUIT && spins < 20000; spins++) {
                __builtin_ia32_pause();
                st = state_.load(std::memory_order_acquire);
            }
            if (st != POSTED && st != QUIT) {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [this] { const int s = state_.load(std::memory_order_acquire); return s == POSTED || s == QUIT; });
                st = state_.load(std::memory_order_acquire);
            }
            if (st == QUIT) return;
            inliers_ = estimate_rotation(prev_, cur_, n_, *Kin_, *Kout_, *rng_, R_, in_fish_, D_);
            int posted = POSTED;  // a destructor that stored QUIT meanwhile must not be answered with DONE
            if (!state_.compare_exchange_strong(posted, DONE, std::memory_order_acq_rel)) return;
        }
    }
    std::thread th_;
    std::mutex m_;
    std::condition_variable cv_;
    std::atomic<int> state_{IDLE};
    const float *prev_ = nullptr, *cur_ = nullptr;
    int n_ = 0;
    const Mat3 *Kin_ = nullptr, *Kout_ = nullptr;
    Pcg32 *rng_ = nullptr;
    bool in_fish_ = true;
    const double *D_ = nullptr;
    Mat3 R_;
    int inliers_ = 0;
};

}  // namespace vstab

using namespace vstab;

// ---------------------------------------------------------------------------------------------
// the pipeline handle
// ---------------------------------------------------------------------------------------------
struct vstab_handle {
    // every way out of vstab_create after the streams and events exist, and vstab_destroy, ends here
    ~vstab_handle() {
        for (hipStream_t s : {tstream, pstream, dstream})
            if (s) (void)hipStreamSynchronize(s);
        for (auto &pe : pending) (void)hipEventDestroy(pe.a), (void)hipEventDestroy(pe.b);
        for (hipEvent_t e : event_pool) (void)hipEventDestroy(e);
        for (auto &s : slots)
            if (s.ingested) (void)hipEventDestroy(s.ingested);
        for (auto &s : slots)
            if (s.copied) (void)hipEventDestroy(s.copied);
        for (hipEvent_t e : warp_events)
            if (e) (void)hipEventDestroy(e);
        if (epoch_tail) (void)hipEventDestroy(epoch_tail);
        for (hipStream_t s : {dstream, pstream, tstream})
            if (s) (void)hipStreamDestroy(s);
        dmabufs.clear([](hipExternalMemory_t &e) { (void)hipDestroyExternalMemory(e); });
    }
    vstab_config cfg;
    vstab_source src;
    hipStream_t stream = nullptr;   // caller-visible stream: the warp runs here, dst is complete when it drains
    hipStream_t tstream = nullptr;  // internal stream: corner detection + LK (the per-frame critical path)
    hipStream_t pstream = nullptr;  // internal stream: ingest + pyramid of the NEXT frame (prefetch, overlaps LK)
    int w = 0, h = 0, ow = 0, oh = 0;
    Mat3 Kin, Kout;
    int map_mode = VSTAB_MAP_CREATEMAP_CL;  // createMap.cl for the preset path, a projection pair in lens mode
    bool in_fish = true;
    // vstab_set_input_calibration: the input lens's k1..k4 (fp64 for the rotation estimate and the markers, fp32 for the map); Kin is then the
    // calibrated camera matrix where one was given
    bool calibrated = false, pulled = false;  // pulled: a pull has started to consume frames
    bool calibrated_borders = false;          // calibrated through vstab_set_input_calibration_ex: vstab_set_border_mode / _ex as without a calibration
    double dist[4] = {0, 0, 0, 0};
    float dist32[4] = {0, 0, 0, 0};
    // vstab_set_input_pinhole: a rectilinear input lens's (k1, k2, p1, p2, k3); the handle then warps through vstab_warp_nv12_pinhole
    bool pinhole = false;
    double pdist[5] = {0, 0, 0, 0, 0};
    float pdist32[5] = {0, 0, 0, 0, 0};
    // the coefficients the rotation estimate undistorts with: k1..k4 where in_fish, the five of a rectilinear lens otherwise
    const double *distortion() const { return calibrated ? dist : pinhole ? pdist : nullptr; }
    Tracker tracker;
    Detector detector;  // (both initialised only where cfg.tracking)

    struct Slot {
        DevBuf buf;  // packed NV12, pitch = w (allocated on the first copy into the slot)
        // where the frame's planes are: in buf, or still in upstream's memory when upstream promised (vstab_frame.hold)
        // that they outlive the frame's whole stay in the pipeline -- then nothing is copied at all
        const uint8_t *y = nullptr, *uv = nullptr;
        size_t pitch_y = 0, pitch_uv = 0;
        bool borrowed = false;
        std::vector<float> feats;  // vstab_config.debug: the features tracked into this frame (input pixels)
        bool have_delta = false;  // upstream supplied this frame's rotation since the previous frame (vstab_frame.delta_rotation)
        Mat3 delta;
        DevBuf buf16;  // pixel_depth 10: the frame's P010 planes (luma rows of 2w bytes, then chroma), copied on ingest ...
        const uint8_t *y16 = nullptr, *uv16 = nullptr;  // ... or left where they are when upstream keeps them for good (hold >= 1 << 29)
        size_t pitch_y16 = 0, pitch_uv16 = 0;
        bool have_readout = false;  // ... and the rotation during the frame's read-out (vstab_frame.readout_rotation): rolling-shutter warp
        Mat3 readout;
        bool queued = false, last = false;
        long freed_at = 0;               // FIFO reuse: the slot idle the longest is taken first
        hipEvent_t ingested = nullptr;   // recorded on pstream after the copy into the slot (and its pyramid, when tracking)
        hipEvent_t copied = nullptr;     // completes with the copy kernel alone (8-bit frames copied by vstab_pack_nv12 while tracking): what
        bool copied_valid = false;       //   upstream's surface has to wait for -- the pyramid behind the copy reads the ring, not the surface
        int warped = -1;                 // index into warp_events of the event recorded behind the warp that read the slot
        bool warp_pending = false;       // a warp has read the slot since it was last filled
        unsigned long ingest_serial = 0;  // which copy `ingested` was last recorded for
    };
    struct PendingCopy {
        int slot;
        unsigned long serial;
        int hold;
    };
    // A frame used in place whose vstab_frame.hold is finite: upstream counts pull callbacks, the warp that reads the
    // planes runs on the caller's stream, so the callback at which the promise runs out first waits for that warp.
    struct PendingBorrow {
        unsigned long serial;
        int hold;
        bool warp_enqueued;
        int warped;  // index into warp_events, -1 until an event is recorded behind the warp
    };
    static constexpr int HOLD_FOREVER = 1 << 29;  // promises at least this long are not tracked
    // Event operations are the expensive HIP calls here (measured on this runtime: hipEventRecord 4.4 us,
    // hipStreamWaitEvent 3.4 us, a kernel launch 2.4 us, hipEventQuery 0.08 us), so the frame loop records as
    // few as it can: one event per ingested frame (behind copy + pyramid), one event per WARP_EVENT_STRIDE
    // warps (slots freed in between share the next one), and a stream only waits on an event that a host-side
    // query says is still pending.
    static constexpr int WARP_EVENT_STRIDE = 4, WARP_EVENT_POOL = 16;
    hipEvent_t warp_events[WARP_EVENT_POOL] = {};
    int warp_event_next = 0;
    std::vector<int> uncovered;  // slots whose warp is enqueued but not yet followed by a recorded event
    vstab_status cover_warps() {  // record one event behind every warp enqueued so far
        if (uncovered.empty() && !uncovered_borrows) return VSTAB_OK;
        const int e = warp_event_next++ % WARP_EVENT_POOL;
        VSTAB_HIP_TRY(hipEventRecord(warp_events[e], stream));
        for (int sl : uncovered) slots[sl].warped = e;
        uncovered.clear();
        if (uncovered_borrows)
            for (PendingBorrow &b : borrows)
                if (b.warp_enqueued && b.warped < 0) b.warped = e;
        uncovered_borrows = 0;
        return VSTAB_OK;
    }
    // host-side wait for an event: a short query spin (0.08 us a query), then a blocking wait
    static vstab_status host_wait(hipEvent_t ev) {
        int spins = 0;
        hipError_t q;
        while ((q = hipEventQuery(ev)) == hipErrorNotReady && ++spins < 20000) __builtin_ia32_pause();
        if (q == hipErrorNotReady) q = hipEventSynchronize(ev);
        VSTAB_HIP_TRY(q);
        return VSTAB_OK;
    }
    // make stream `waiter` wait for `ev` unless the host can already see that it has completed
    static vstab_status wait_if_pending(hipStream_t waiter, hipEvent_t ev) {
        const hipError_t q = hipEventQuery(ev);
        if (q == hipSuccess) return VSTAB_OK;
        if (q != hipErrorNotReady) VSTAB_HIP_TRY(q);
        VSTAB_HIP_TRY(hipStreamWaitEvent(waiter, ev, 0));
        return VSTAB_OK;
    }
    // (the first frame of a stream is tracked from but never warped: its reads were over, host-visibly, when the
    // second frame's LK results came back)
    void forget_borrow(unsigned long serial) {
        for (auto it = borrows.begin(); it != borrows.end(); ++it)
            if (it->serial == serial) {
                borrows.erase(it);
                return;
            }
    }
    std::vector<PendingCopy> copies;  // device-frame copies upstream has not been promised to outlive yet
    std::vector<PendingBorrow> borrows;  // frames used in place whose promise is finite (oldest first)
    int uncovered_borrows = 0;           // of those, warps enqueued but not yet followed by a recorded event
    int src_error = 0;                   // upstream's error code once it has failed (surfaces when the frames read ahead are used up)
    unsigned long ingest_serial = 0;
    long free_counter = 0;
    std::vector<Slot> slots;
    int last_slot = -1;  // m_last_input_frame
    int last_ingest_slot = -1;
    EstimateWorker worker;            // runs estimate_rotation beside the launch calls of the next frame
    bool estimate_posted = false;
    bool threaded_estimate = true;    // VSTAB_THREADED_ESTIMATE=0: estimate on the calling thread
    bool speculate = true;            // VSTAB_SPECULATE=0 disables speculative corner detection
    int cur_pyr = 0;     // pyramid set holding the last tracked frame's pyramid (frame index mod 3)

    long frame_index = 0, last_key = -1;       // m_frame_index, m_last_key_frame_index
    std::vector<float> corners;                // m_last_input_frame_corners
    Mat3 measured = Mat3::identity();          // m_measured_rotation
    bool have_last_rot = false;
    Mat3 last_rot = Mat3::identity();          // m_last_frame_rotation
    std::unique_ptr<RotationFilterSG> sg;      // m_rotation_filter
    RotationFilterKalman kalman;
    std::deque<std::pair<int, Mat3>> queue;    // m_buffered_frames + m_buffered_rotations
    Pcg32 rng;
    std::deque<vstab_frame_log> log;
    std::deque<Mat3> warp_log;
    // the introspection logs keep the most recent LOG_KEEP entries (indices stay absolute)
    static constexpr size_t LOG_KEEP = 1 << 16;
    long log_base = 0, warp_log_base = 0;

    // profiler
    int profiling = 0;  // 0 off, 1 warp launches only (cheap), 2 every GPU stage
    vstab_profile prof{};
    enum Stage { ST_INGEST, ST_PYRAMID, ST_CORNERS, ST_LK, ST_WARP, ST_COUNT };
    struct Pending {
        hipEvent_t a, b;
        int stage;
    };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> event_pool;
    hipEvent_t get_event() {
        if (!event_pool.empty()) {
            hipEvent_t e = event_pool.back();
            event_pool.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
    void fold_pending() {
        if (dstream) (void)hipStreamSynchronize(dstream);
        (void)hipStreamSynchronize(pstream);
        (void)hipStreamSynchronize(tstream);
        (void)hipStreamSynchronize(stream);
        double *sums[ST_COUNT] = {&prof.gpu_ingest_ms, &prof.gpu_pyramid_ms, &prof.gpu_corners_ms, &prof.gpu_lk_ms, &prof.gpu_warp_ms};
        for (auto &p : pending) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) *sums[p.stage] += ms;
            event_pool.push_back(p.a), event_pool.push_back(p.b);
        }
        pending.clear();
    }

    // a frame whose tracking has been launched (inflight) / whose LK results have been read (ready)
    struct Tracked {
        int slot = -1;
        vstab_frame_log lg{};
        std::vector<float> prev, pp, cp;
    };
    Tracked inflight, ready, estimating;  // ... and whose rotation estimate is running (or waiting to be computed)
    bool have_inflight = false, have_ready = false, have_estimating = false, src_eof = false;
    // LK launches: the one whose results the host waits for next, and the one chained behind it for the
    // following frame (speculative: valid unless that frame turns out to be a key frame, :415)
    // Tracker launches.  One launch covers a SEGMENT of consecutive frames (k_lk_track: every feature slot runs down its own
    // chain through the segment's frames); segments are enqueued ahead of the frame the host is at, as far as the frames read
    // ahead reach, each chained on the device behind the one before it -- or started from freshly detected corners where the
    // counter half of the key-frame rule (:415) says a key frame will be.  Everything enqueued ahead is speculative: it is
    // dropped when the count half of the rule (< 150 survivors) makes a frame a key frame nobody planned for.
    struct Segment {
        long first = 0;            // frame index (frame_index numbering) of its first frame
        int n = 0;                 // frames covered
        bool key = false;          // starts from fresh corners detected on frame first - 1 (a planned key frame); else chained
        long last_key_after = -1;  // what last_key will be once the host has passed this segment
        int stream = 0;            // epoch stream it was enqueued on (vstab_handle::estream)
        std::vector<float> corners;  // key segments: the corners it was launched with
        Tracker::Launch launch;
    };
    std::deque<Segment> segs;        // launched, not yet used up; consecutive, in frame order; front covers the host's frame
    Tracker::Launch inflight_launch; // the launch, and the frame pair of it, whose results the host waits for next
    int inflight_idx = 0;
    long segs_launched = 0, seg_frames_launched = 0, seg_frames_dropped = 0;
    DevBuf host_out;                // staging buffer of vstab_pull_frame_host
    DevBuf bgr16_out;               // 16-bit BGR frame of vstab_pull_frame_p010 (converted to P010 planes behind the warp)
    // Quantised-map cache: when two consecutive frames are warped with the same 17 parameters (tracking off, or any
    // run of identical rotations) the map is written once (vstab_quantised_map) and the following warps read it
    // instead of evaluating it -- the reference recomputes an identical map per frame (FrameSourceWarp.cpp:283-304).
    DevBuf qmap;
    float qmap_params[17] = {0}, last_params[17] = {0};
    bool qmap_valid = false, have_last_params = false, map_cache = true;  // VSTAB_MAP_CACHE=0 disables
    int border_mode = VSTAB_BORDER_CONSTANT;  // vstab_set_border_mode: applies from the next pull
    // vstab_set_colour: the colour spec of the converting pulls (BGR, NV12 through BGR), from the next pull on
    int colour_matrix = VSTAB_COLOUR_CVTCOLOR, colour_range = VSTAB_RANGE_LIMITED;
    bool colour() const { return colour_matrix != VSTAB_COLOUR_CVTCOLOR || colour_range != VSTAB_RANGE_LIMITED; }
    // vstab_set_colour10: the colour spec of a pixel_depth 10 handle's converting pulls (16-bit BGR, P010 through BGR), from the next pull on
    int colour10_matrix = VSTAB_COLOUR_CVTCOLOR, colour10_range = VSTAB_RANGE_LIMITED;
    // vstab_set_resample10: the resampler and border mode of a pixel_depth 10 handle's plane-wise pull, from the next pull on
    int resample10 = VSTAB_RESAMPLE_DEFAULT, border10 = VSTAB_BORDER_CONSTANT;
    int readout_warp = VSTAB_READOUT_REFUSE;  // vstab_set_readout_warp: applies from the next pull
    long warps_from_cache = 0;
    PinnedBuf marker_pts;           // vstab_config.debug: rotating sets of marker centres, read by the kernel in place
    unsigned marker_set = 0;
    hipStream_t dstream = nullptr;  // speculative corner detection (137 us of kernels every 21st frame) beside everything else
    // EPOCHS IN TURN (when dstream exists): what follows a planned key frame -- its speculative detection, the tracker segment launched from
    // those corners and the segments chained behind it -- depends on nothing tracked before it, so it runs on the OTHER of the two streams
    // {tstream, dstream} than the epoch still being tracked: two dependent chains side by side for as long as the read-ahead reaches into
    // the next epoch.  The tracker's chain sets the frame period at 1080p (profiles/r05_epochs_in_turn.txt).  VSTAB_EPOCH_OVERLAP=0 (read
    // once, in vstab_create) keeps everything on tstream.
    bool epoch_overlap = false;
    int epoch_stream = 0;            // stream (0 = tstream, 1 = dstream) of the most recently launched epoch
    int spec_stream = 1;             // stream the pending speculative detection was enqueued on
    int inflight_stream = 0;         // stream of the launch whose results the host waits for next
    long epochs_on_second_stream = 0;
    hipEvent_t epoch_tail = nullptr; // a fresh start waits for what is still queued on the other epoch stream (dropped launches precede their replacement)
    hipStream_t estream(int i) const { return i && dstream ? dstream : tstream; }
    // DMA-BUF objects imported so far (vstab_frame.mem == VSTAB_MEM_DMABUF), keyed by the inode of the object
    DmaBufCache<hipExternalMemory_t> dmabufs;  // vstab_hostlogic.hpp; VSTAB_DMABUF_CACHE=n (tests) shrinks its 256 entries
    bool chain_lk = true;        // VSTAB_CHAIN_LK=0: no launches ahead of the host's frame (one frame per launch, on demand)
    int seg_max = LK_SEG_MAX;    // VSTAB_LK_SEGMENT=n: frames per tracker launch at most (1 = a launch per frame, chained one frame ahead)
    int prefetch_depth = PREFETCH_DEPTH;  // frames pulled from upstream ahead of the one being tracked
    int seg_target = 4;          // a chained segment is enqueued once this many frames are waiting (fewer only at a key frame or when the tracker would idle)
    long chained_adopted = 0, chained_discarded = 0, key_prelaunched = 0;
    // a frame that has been pulled from upstream, copied into the ring and whose pyramid is being built
    std::deque<std::pair<int, int>> prefetched;  // (ring slot, pyramid set), oldest first
    long prefetch_count = 0;

    int acquire_slot() {
        int best = -1;
        for (size_t i = 0; i < slots.size(); i++)
            if (!slots[i].queued && !slots[i].last && (best < 0 || slots[i].freed_at < slots[best].freed_at)) best = (int)i;
        return best;
    }
    const uint8_t *gray(int s) const { return slots[s].y; }
    size_t gpitch(int s) const { return slots[s].pitch_y; }
    int borrow_hold = 0;  // vstab_frame.hold from which a device frame is used in place (set in vstab_create)
    long frames_borrowed = 0, frames_copied = 0;
};

struct GpuStage {  // records an event pair around a stage when profiling is on
    vstab_handle *H;
    hipEvent_t a = nullptr, b = nullptr;
    int stage;
    hipStream_t s;
    GpuStage(vstab_handle *h, int st)
        : H(h), stage(st), s(st == vstab_handle::ST_WARP ? h->stream : (st == vstab_handle::ST_INGEST || st == vstab_handle::ST_PYRAMID) ? h->pstream : h->tstream) {
        // level 1 times every 8th warp launch: two event records cost more host time than the launch itself
        if (H->profiling >= 2 || (H->profiling == 1 && st == vstab_handle::ST_WARP && (H->prof.warp_launches & 7) == 0)) {
            a = H->get_event();
            if (st == vstab_handle::ST_WARP) {
                // the warp launcher stamps the kernel's own start and end into the pair (hipExtLaunchKernelGGL): kernel
                // time as rocprofv3 reports it, without the dispatch wait behind the other streams' kernels
                H->prof.warp_timed++;
                b = H->get_event();
                set_launch_events(a, b);
            } else {
                (void)hipEventRecord(a, s);
            }
        }
    }
    ~GpuStage() {
        if (!a) return;
        if (b && launch_events_pending()) {  // a warp path that does not take the pair (10-bit, direct gather): stream positions
            (void)take_launch_events();
            (void)hipEventRecord(a, s);  // (late: such a launch is then timed as ~0; only the fused kernel is the metric's)
            (void)hipEventRecord(b, s);
        } else if (!b) {
            b = H->get_event();
            (void)hipEventRecord(b, s);
        }
        H->pending.push_back({a, b, stage});
        if (H->pending.size() > 4096) H->fold_pending();
    }
};
// VSTAB_HOST_TIMING=1: wall time of the host-side steps of the pull loop, printed by vstab_destroy (development aid)
struct HostTimers {
    enum { PULL_CB, INGEST_SYNC, INGEST, PYRAMID, SPEC_DETECT, LK_LAUNCH, LK_CHAIN, WARP, TOTAL, N };
    double ms[N] = {0};
    long calls[N] = {0};
    bool on = getenv("VSTAB_HOST_TIMING") != nullptr;
    static const char *name(int i) {
        static const char *n[N] = {"pull_cb", "ingest_sync", "ingest", "pyramid", "spec_detect", "lk_launch", "lk_chain", "warp", "pull_frame_total"};
        return n[i];
    }
};
inline HostTimers g_ht;
struct HT {
    int i;
    std::chrono::steady_clock::time_point t0;
    explicit HT(int idx) : i(idx) {
        if (g_ht.on) t0 = std::chrono::steady_clock::now();
    }
    ~HT() {
        if (g_ht.on) g_ht.ms[i] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), g_ht.calls[i]++;
    }
};

struct HostStage {
    double *sum;
    std::chrono::steady_clock::time_point t0;
    explicit HostStage(double *s) : sum(s), t0(std::chrono::steady_clock::now()) {}
    ~HostStage() { *sum += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// the steps of consume_frame (vstab_pipeline.cpp), run by the pull loop (vstab_pull.cpp) in frame order
vstab_status prefetch_next(vstab_handle *H);
vstab_status launch_tracking(vstab_handle *H);
vstab_status finish_wait(vstab_handle *H);
void post_estimate(vstab_handle *H), finish_estimate(vstab_handle *H);
