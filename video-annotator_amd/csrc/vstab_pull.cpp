// vstab_pull.cpp -- FrameSourceWarp::pull_frame (:452-476) behind the pull entry points of the C ABI, as its seven steps, and
// vstab_set_border_mode / _ex and vstab_set_readout_warp, whose modes those steps read.
#include <cmath>

#include "vstab_colour.hpp"
#include "vstab_pipeline.hpp"
#include "vstab_warp_request.hpp"

constexpr int OUT_BGR16 = 16;        // internal: the 10-bit path's output (vstab_pull_frame_bgr16)
constexpr int OUT_P010 = 17;         // internal: the 10-bit path's frame as P010 planes (vstab_pull_frame_p010)
constexpr int OUT_P010_PLANAR = 18;  // internal: the 10-bit frame warped plane by plane (vstab_pull_frame_p010_planar)
static inline bool out_is_10bit(int f) { return f == OUT_BGR16 || f == OUT_P010 || f == OUT_P010_PLANAR; }
static inline bool out_has_chroma_plane(int f) { return f == VSTAB_OUT_NV12 || f == VSTAB_OUT_NV12_PLANAR || f == OUT_P010 || f == OUT_P010_PLANAR; }

struct KeepPrev {  // a keep pull (vstab_pull_frame_keep / _nv12_planar_keep): its entry point's name, the caller's previous output
    const char *fn;
    const void *prev, *prev_uv;
    size_t pitch_prev, pitch_prev_uv;
};

struct Pull {  // one pull on its way through the steps: what the caller asked for and the border mode in force, then what the steps add
    const int out_format;
    void *const dst, *const dst_uv;
    const size_t pitch_dst, pitch_dst_uv;
    const int border_mode;
    const int colour_matrix, colour_range;  // the colour spec in force (vstab_set_colour)
    const KeepPrev *const keep = nullptr;  // a keep pull
    bool colour() const { return colour_matrix != VSTAB_COLOUR_CVTCOLOR || colour_range != VSTAB_RANGE_LIMITED; }
    int slot = -1;
    Mat3 warp_R;
    float p[17], p_bottom[17];
    const float *rot_bottom = nullptr;  // the last row's rotation (in p_bottom) when the frame carries a read-out rotation
    bool cached = false;
};

// 1. the formats this handle does not emit
static vstab_status refuse_formats(const vstab_handle *H, const Pull &P) {
    if ((H->cfg.pixel_depth == 10) != out_is_10bit(P.out_format))
        return fail(VSTAB_ERR_INVALID, "vstab_pull_frame: a pixel_depth 10 handle emits through vstab_pull_frame_bgr16, an 8-bit handle through the others");
    // (a 10-bit handle with a resampler set warps plane by plane alone; refused before any frame is dequeued: the frame stays pullable plane-wise)
    if (H->resample10 != VSTAB_RESAMPLE_DEFAULT && (P.out_format == OUT_BGR16 || P.out_format == OUT_P010))
        return fail(VSTAB_ERR_INVALID, std::string("vstab_pull_frame: ") + resample_name(H->resample10) +
                                           " on a pixel_depth 10 handle (vstab_set_resample10) emits plane-wise P010 frames (vstab_pull_frame_p010_planar), not 16-bit BGR or P010 through BGR");
    if (P.out_format == VSTAB_OUT_BGR8 || P.out_format == VSTAB_OUT_NV12_PLANAR) return VSTAB_OK;
    static const char served[] = " emits 8-bit BGR or plane-wise NV12 frames (vstab_pull_frame / _frames / _host / vstab_peek_frame / vstab_pull_frame_nv12_planar), not NV12 through BGR";
    // (refused before any frame is dequeued: the caller can pull the same frame in a format the cubic warp serves)
    if (H->cfg.resample != VSTAB_RESAMPLE_DEFAULT) return fail(VSTAB_ERR_INVALID, std::string("vstab_pull_frame: ") + resample_name(H->cfg.resample) + served);
    // (the mode in force for this pull: a border warp serves the same two formats as the cubic one, refused before any frame is dequeued)
    if (P.border_mode != VSTAB_BORDER_CONSTANT) return fail(VSTAB_ERR_INVALID, std::string("vstab_pull_frame: a border mode other than VSTAB_BORDER_CONSTANT") + served);
    // (nor does the distorted-lens warp of a calibrated handle)
    if (H->calibrated) return fail(VSTAB_ERR_INVALID, std::string("vstab_pull_frame: a calibrated handle (vstab_set_input_calibration)") + served);
    if (H->pinhole) return fail(VSTAB_ERR_INVALID, std::string("vstab_pull_frame: a calibrated handle (vstab_set_input_pinhole)") + served);
    return VSTAB_OK;
}

// 1b. a keep pull: the handles whose warp has no keep-edge form, then the caller's history (all before a frame is dequeued)
static vstab_status refuse_keep(const vstab_handle *H, const Pull &P) {
    const KeepPrev &k = *P.keep;
    const std::string n = k.fn;
    if (H->cfg.resample != VSTAB_RESAMPLE_DEFAULT) return fail(VSTAB_ERR_UNSUPPORTED, n + ": " + resample_name(H->cfg.resample) + " has no keep-edge warp");
    if (H->cfg.interpolation == 0) return fail(VSTAB_ERR_UNSUPPORTED, n + ": INTER_NEAREST has no keep-edge warp");
    if (P.border_mode != VSTAB_BORDER_CONSTANT)
        return fail(VSTAB_ERR_UNSUPPORTED, n + ": a border mode other than VSTAB_BORDER_CONSTANT is in force (vstab_set_border_mode)");
    if (H->calibrated) return fail(VSTAB_ERR_UNSUPPORTED, n + ": a calibrated handle (vstab_set_input_calibration) has no keep-edge warp");
    if (H->pinhole) return fail(VSTAB_ERR_UNSUPPORTED, n + ": a calibrated handle (vstab_set_input_pinhole) has no keep-edge warp");
    if (P.colour()) return fail(VSTAB_ERR_UNSUPPORTED, n + ": a colour spec is set (vstab_set_colour), and the keep-edge warp converts with cvtColor's arithmetic");
    const bool planar = P.out_format == VSTAB_OUT_NV12_PLANAR;
    const KeepPlane planes[2] = {{k.prev, k.pitch_prev, P.dst, P.pitch_dst, (size_t)H->ow * (planar ? 1 : 3), H->oh},
                                 {k.prev_uv, k.pitch_prev_uv, P.dst_uv, P.pitch_dst_uv, (size_t)((H->ow + 1) / 2) * 2, (H->oh + 1) / 2}};
    bool in_place;
    return check_keep_prev(k.fn, planes, planar ? 2 : 1, in_place);
}

// 2. consume frames until the look-ahead window of the next one to emit is complete, or upstream has ended
static vstab_status advance_until_due(vstab_handle *H) {
    while (H->queue.size() <= (size_t)H->cfg.smooth_radius) {  // :453
        if (!H->have_inflight && !H->have_ready && !H->have_estimating && H->prefetched.empty() && H->src_eof) {  // every frame read has been queued
            if (H->src_error) return fail(VSTAB_ERR_SOURCE, "upstream pull failed with " + std::to_string(H->src_error));
            // :456-461 pretend the camera kept its last orientation (once per call while draining)
            if (H->sg) H->sg->add(H->measured);
            break;
        }
        // 1. LK results of the frame in flight -> surviving corners
        if (H->have_inflight) VSTAB_TRY(finish_wait(H));
        // 2. the rotation estimate that was started a frame ago (it ran beside everything since) -> queue its frame; then
        //    the frame just read starts its estimate on the worker thread
        finish_estimate(H);
        post_estimate(H);
        // 3. key-frame rule + LK launch for the oldest prefetched frame, and the launches that can be enqueued ahead of it
        if (H->prefetched.empty() && !H->src_eof) {
            const vstab_status st = prefetch_next(H);
            if (st != VSTAB_OK && st != VSTAB_EOF) return st;
        }
        if (!H->prefetched.empty() && !H->have_inflight) {
            const size_t queued = H->queue.size();
            VSTAB_TRY(launch_tracking(H));
            if (H->queue.size() != queued) continue;  // (tracking off: the frame is queued at once) re-check :453 before :456
        }
        // 4. read ahead: pull + copy + pyramid of the following frames (prefetch stream)
        while ((int)H->prefetched.size() < H->prefetch_depth && !H->src_eof) {
            const vstab_status st = prefetch_next(H);
            if (st != VSTAB_OK && st != VSTAB_EOF) return st;
        }
    }
    return VSTAB_OK;
}

// 3. the frame at the head of the queue: its stabilising rotation and the parameter sets of its warp
static void smooth(vstab_handle *H, Pull &P) {
    P.slot = H->queue.front().first;
    const Mat3 measured = H->queue.front().second;
    H->queue.pop_front();
    Mat3 corrected;
    {
        HostStage hs(&H->prof.host_smooth_ms);
        if (H->cfg.smoother == VSTAB_SMOOTHER_SG)
            corrected = H->sg->filter();  // :471
        else if (H->cfg.smoother == VSTAB_SMOOTHER_KALMAN)
            corrected = H->kalman.update(measured);
        else if (H->cfg.smoother == VSTAB_SMOOTHER_FIXED)
            corrected = Mat3::identity();  // hold the orientation of the first frame
        else
            corrected = measured;
        const Mat3 correction = corrected * measured.inv();  // :472
        P.warp_R = correction.inv();                         // :475
    }
    H->warp_log.push_back(P.warp_R);
    if (H->warp_log.size() > vstab_handle::LOG_KEEP) H->warp_log.pop_front(), H->warp_log_base++;
    H->prof.frames_emitted++, H->prof.warp_launches++;
    map_params(H->Kin, H->Kout, P.warp_R, P.p);
    const vstab_handle::Slot &S = H->slots[P.slot];
    // rolling shutter: the camera kept turning while the rows were read out; the last row is warped with the stabilising
    // rotation of the orientation it was exposed at (measured' = readout * measured  =>  W' = readout * W)
    if (S.have_readout) map_params(H->Kin, H->Kout, S.readout * P.warp_R, P.p_bottom), P.rot_bottom = P.p_bottom + 8;
}

// 4. whether the quantised map of an earlier frame serves this one (written down now if this is the second frame in a row with its parameters)
static vstab_status choose_cached_map(vstab_handle *H, Pull &P) {
    // (the quantised map holds no chroma positions: the plane-wise warp always evaluates its map)
    // (nor do the cubic, Lanczos and border warps read it, with or without a border mode: they evaluate the map of every frame; the cached
    //  map's kernel has the constant border built in)
    // (a keep pull neither reads nor updates this state: plain pulls around it see the parameters of the plain pull before)
    // (nor does the pinhole-lens warp: vstab_set_input_pinhole)
    // (nor does a converting pull with a colour spec: the cached map's kernel has cvtColor's constants.  It steps aside as for a keep pull.)
    if (P.keep || H->pinhole || (P.colour() && P.out_format != VSTAB_OUT_NV12_PLANAR)) return VSTAB_OK;
    if (!H->map_cache || H->cfg.resample != VSTAB_RESAMPLE_DEFAULT || P.border_mode != VSTAB_BORDER_CONSTANT || P.rot_bottom || out_is_10bit(P.out_format) ||
        P.out_format == VSTAB_OUT_NV12_PLANAR)
        return VSTAB_OK;
    if (H->qmap_valid && std::memcmp(P.p, H->qmap_params, sizeof(P.p)) == 0) {
        P.cached = true;
    } else if (H->have_last_params && std::memcmp(P.p, H->last_params, sizeof(P.p)) == 0) {
        // second frame in a row with these parameters: write the map down now (same stream, ahead of the warp)
        VSTAB_TRY(H->qmap.ensure(vstab_quantised_map_bytes(H->ow, H->oh)));
        if (H->calibrated) VSTAB_TRY(vstab_quantised_map_dist(H->qmap.p, H->ow, H->oh, P.p, H->dist32, H->map_mode, H->stream));
        else VSTAB_TRY(vstab_quantised_map(H->qmap.p, H->ow, H->oh, P.p, H->map_mode, H->stream));
        std::memcpy(H->qmap_params, P.p, sizeof(P.p));
        H->qmap_valid = P.cached = true;
    }
    std::memcpy(H->last_params, P.p, sizeof(P.p));
    H->have_last_params = true;
    H->warps_from_cache += P.cached;
    return VSTAB_OK;
}

// (every warp launcher takes the profiler's event pair; a request refused by launch_warp itself launches nothing, so the pair armed by
//  GpuStage is taken back here instead of staying pending for somebody else's launch)
static vstab_status refuse_launch(const std::string &msg) {
    (void)take_launch_events();
    return fail(VSTAB_ERR_INVALID, msg);
}

// 5. the warp kernel for this (out_format, resample, border, interpolation, readout, cached)
static vstab_status launch_warp(vstab_handle *H, const Pull &P) {
    const vstab_handle::Slot &S = H->slots[P.slot];
    const int out_format = P.out_format, w = H->w, h = H->h, ow = H->ow, oh = H->oh, mode = H->map_mode;
    const bool border = P.border_mode != VSTAB_BORDER_CONSTANT;
    const bool resampled = H->cfg.resample != VSTAB_RESAMPLE_DEFAULT, lanczos4 = H->cfg.resample == VSTAB_RESAMPLE_LANCZOS4;  // (else CUBIC: vstab_create)
    // the profiling events bracket the launch call and nothing else, so the interval is the kernel
    // (plus its dispatch), not host work between two API calls
    GpuStage gs(H, vstab_handle::ST_WARP);
#ifdef VSTAB_DEV
    // development builds: VSTAB_DEV_SKIP_WARP=1 launches no warp at all, so that tools/lk_timeline.py sees the tracker chain with
    // nothing but the pyramid kernels beside it (how much of an iteration is the chain, how much is contention with the warp)
    static const bool skip_warp = getenv("VSTAB_DEV_SKIP_WARP") != nullptr;
    if (skip_warp) {
        (void)take_launch_events();
        return VSTAB_OK;
    }
#endif
    // The converting 10-bit pulls with a colour spec (vstab_set_colour10) go through the _colour twins; without one they call what they always called,
    // messages included.
    const int m10 = H->colour10_matrix, r10 = H->colour10_range;
    const bool c10 = !colour_spec_default(m10, r10);
    const auto warp_bgr16 = [&](void *dst, size_t pitch_dst) {
        return c10 ? vstab_warp_p010_colour(S.y16, S.pitch_y16, S.uv16, S.pitch_uv16, w, h, P.p, P.rot_bottom, mode, H->cfg.blend, dst, pitch_dst, ow, oh, m10, r10, H->stream)
                   : vstab_warp_p010(S.y16, S.pitch_y16, S.uv16, S.pitch_uv16, w, h, P.p, P.rot_bottom, mode, H->cfg.blend, dst, pitch_dst, ow, oh, H->stream);
    };
    if (out_format == OUT_BGR16) return warp_bgr16(P.dst, P.pitch_dst);
    if (out_format == OUT_P010_PLANAR && H->resample10 != VSTAB_RESAMPLE_DEFAULT)  // vstab_set_resample10
        return vstab_warp_p010_planar_ex(S.y16, S.pitch_y16, S.uv16, S.pitch_uv16, w, h, P.p, P.rot_bottom, mode, H->resample10, H->border10, P.dst, P.pitch_dst,
                                         P.dst_uv, P.pitch_dst_uv, ow, oh, H->stream);
    if (out_format == OUT_P010_PLANAR)
        return vstab_warp_p010_planar(S.y16, S.pitch_y16, S.uv16, S.pitch_uv16, w, h, P.p, P.rot_bottom, mode, H->cfg.blend, P.dst, P.pitch_dst, P.dst_uv,
                                      P.pitch_dst_uv, ow, oh, H->stream);
    if (out_format == OUT_P010) {
        vstab_status st = c10 ? vstab_warp_p010_planes_colour(S.y16, S.pitch_y16, S.uv16, S.pitch_uv16, w, h, P.p, P.rot_bottom, mode, H->cfg.blend, P.dst, P.pitch_dst,
                                                              P.dst_uv, P.pitch_dst_uv, ow, oh, m10, r10, H->stream)
                              : vstab_warp_p010_planes(S.y16, S.pitch_y16, S.uv16, S.pitch_uv16, w, h, P.p, P.rot_bottom, mode, H->cfg.blend, P.dst, P.pitch_dst, P.dst_uv,
                                                       P.pitch_dst_uv, ow, oh, H->stream);
        if (st == VSTAB_ERR_UNSUPPORTED) {
            const size_t bpitch = ((size_t)ow * 6 + 255) & ~(size_t)255;
            st = H->bgr16_out.ensure(bpitch * oh);
            if (st == VSTAB_OK) st = warp_bgr16(H->bgr16_out.p, bpitch);
            if (st == VSTAB_OK)
                st = c10 ? vstab_cvt_bgr16_p010_colour(H->bgr16_out.p, bpitch, ow, oh, P.dst, P.pitch_dst, P.dst_uv, P.pitch_dst_uv, m10, r10, H->stream)
                         : vstab_cvt_bgr16_p010(H->bgr16_out.p, bpitch, ow, oh, P.dst, P.pitch_dst, P.dst_uv, P.pitch_dst_uv, H->stream);
        }
        return st;
    }
    // The 8-bit warps: one request from the handle and the pull, the pipeline's own refusals, then the stateless warps' one path
    // (warp_nv12: vstab_warp_request.hpp), under the name of the stateless entry point that stands for this handle.
    const bool per_row = P.rot_bottom && H->readout_warp == VSTAB_READOUT_PER_ROW;  // vstab_set_readout_warp(VSTAB_READOUT_PER_ROW)
    // a frame that carries a read-out rotation where the handle's warp has no rotation per row: it is consumed, as INTER_NEAREST consumes it
    // below.  (A rectilinear input refuses such a frame where it takes it from upstream, prefetch_next; a keep pull warps it per row.)
    if (P.rot_bottom && !P.keep) {
        if (H->pinhole) return refuse_launch("a calibrated handle (vstab_set_input_pinhole) warps frames without a read-out rotation");
        if (H->calibrated && !per_row) return refuse_launch("a calibrated handle (vstab_set_input_calibration) warps frames without a read-out rotation");
        if (resampled && !per_row) return refuse_launch(std::string(resample_name(H->cfg.resample)) + " warps frames without a read-out rotation (vstab_frame.readout_rotation)");
    }
    if (H->cfg.interpolation == 0) {  // (vstab_create, vstab_set_*: such a handle has no resampler, lens, border mode or keep pull)
        if (out_format != VSTAB_OUT_BGR8 || P.rot_bottom) return refuse_launch("INTER_NEAREST emits 8-bit BGR frames without a read-out rotation");
        return vstab_warp_nv12_nearest_ex(S.y, S.pitch_y, S.uv, S.pitch_uv, w, h, P.p, mode, P.dst, P.pitch_dst, ow, oh, H->stream);
    }
    static const float no_params[17] = {0};
    WarpRequest q = {.e = ENTRY_EX, .y = S.y, .pitch_y = S.pitch_y, .uv = S.uv, .pitch_uv = S.pitch_uv, .sw = w, .sh = h, .params = P.p, .rot_bottom = P.rot_bottom,
                     .map_mode = mode, .out_format = out_format, .dst = P.dst, .pitch_dst = P.pitch_dst, .dst_uv = P.dst_uv, .pitch_dst_uv = P.pitch_dst_uv,
                     .dw = ow, .dh = oh, .stream = H->stream};
    // a colour spec (vstab_set_colour: INTER_LINEAR, constant border, ideal lens, no keep pull): the converting pulls; the plane-wise pull converts nothing
    if (P.colour() && out_format != VSTAB_OUT_NV12_PLANAR) {
        if (P.rot_bottom) return refuse_launch("a handle with a colour spec (vstab_set_colour) warps frames without a read-out rotation");
        q.e = ENTRY_COLOUR, q.colour_matrix = P.colour_matrix, q.colour_range = P.colour_range;
        return warp_nv12(q);
    }
    if (P.keep) {  // (refuse_keep: INTER_LINEAR, constant border, ideal lens)
        q.e = ENTRY_KEEP, q.keep = true;
        q.prev = P.keep->prev, q.pitch_prev = P.keep->pitch_prev, q.prev_uv = P.keep->prev_uv, q.pitch_prev_uv = P.keep->pitch_prev_uv;
        return warp_nv12(q);
    }
    q.resample = H->cfg.resample, q.border_mode = P.border_mode;
    if (H->pinhole) q.e = ENTRY_PINHOLE, q.pinhole = H->pdist32;
    else if (P.rot_bottom && (H->calibrated || resampled)) q.e = ENTRY_RS_EX, q.dist = H->calibrated ? H->dist32 : nullptr;
    else if (P.cached) q.e = ENTRY_MAPPED, q.params = no_params, q.qmap = H->qmap.p, q.qpitch = (ow + 3) & ~3, q.map_mode = VSTAB_MAP_CREATEMAP_CL;  // (the map is written down, the lens with it)
    else if (H->calibrated) q.e = ENTRY_DIST_EX, q.dist = H->dist32;
    else if (resampled) q.e = lanczos4 ? (border ? ENTRY_LANCZOS4_BORDER : ENTRY_LANCZOS4) : (border ? ENTRY_CUBIC_BORDER : ENTRY_CUBIC);
    else if (border) q.e = ENTRY_BORDER;
    else if (P.rot_bottom) q.e = ENTRY_RS;
    return warp_nv12(q);
}

// 6. vstab_config.debug: a marker on every feature tracked into the frame (marker_pts holds MARKER_SETS rotating sets of MARKER_CAP centres)
constexpr int MARKER_SETS = 16, MARKER_CAP = 256;
static vstab_status draw_markers(vstab_handle *H, const Pull &P) {
    vstab_handle::Slot &S = H->slots[P.slot];
    const Mat3 &warp_R = P.warp_R;
    // where the warp sends each tracked feature: input pixel -> ray -> R^T -> output projection (the inverse of the map)
    int *host = H->marker_pts.as<int>() + 2 * MARKER_CAP * (H->marker_set % MARKER_SETS);
    int *dev = static_cast<int *>(H->marker_pts.dev()) + 2 * MARKER_CAP * (H->marker_set % MARKER_SETS);
    H->marker_set++;
    const bool out_fish = H->map_mode == VSTAB_MAP_FISH_TO_FISH || H->map_mode == VSTAB_MAP_RECT_TO_FISH;
    int n = 0;
    for (size_t i = 0; i + 1 < S.feats.size() && n < MARKER_CAP; i += 2) {
        const double a = (S.feats[i] - H->Kin(0, 2)) / H->Kin(0, 0), b = (S.feats[i + 1] - H->Kin(1, 2)) / H->Kin(1, 1);
        double rx = a, ry = b, rz = 1;
        if (H->in_fish) {
            const double thd = std::hypot(a, b);  // theta_d of a calibrated lens: back to theta first
            double th = thd;
            if (H->calibrated && !fisheye_theta(thd, H->dist, th)) continue;
            const double sc = thd > 0 ? std::sin(th) / thd : 1.0;
            rx = a * sc, ry = b * sc, rz = std::cos(th);
        } else if (H->pinhole) {
            pinhole_undistort_normalised(a, b, H->pdist, rx, ry);  // the distorted pinhole lens: back to the ideal one first
        }
        const double ox = warp_R(0, 0) * rx + warp_R(1, 0) * ry + warp_R(2, 0) * rz, oy = warp_R(0, 1) * rx + warp_R(1, 1) * ry + warp_R(2, 1) * rz,
                     oz = warp_R(0, 2) * rx + warp_R(1, 2) * ry + warp_R(2, 2) * rz;
        if (!(oz > 0)) continue;
        double u = ox / oz, v = oy / oz;
        if (out_fish) {
            const double r = std::hypot(ox, oy), th = std::atan2(r, oz), sc = r > 0 ? th / r : 1.0;
            u = ox * sc, v = oy * sc;
        }
        host[2 * n] = (int)std::nearbyint(H->Kout(0, 2) + u * H->Kout(0, 0)), host[2 * n + 1] = (int)std::nearbyint(H->Kout(1, 2) + v * H->Kout(1, 1));
        n++;
    }
    S.feats.clear();
    if (P.out_format == VSTAB_OUT_NV12 || P.out_format == VSTAB_OUT_NV12_PLANAR)
        return vstab_draw_markers(P.dst, P.pitch_dst, H->ow, H->oh, 1, dev, n, 3, 235u, H->stream);
    return vstab_draw_markers(P.dst, P.pitch_dst, H->ow, H->oh, 3, dev, n, 3, 0x0000FF00u, H->stream);
}

// 7. the slot goes back to the ring, behind the warp that read it
static vstab_status release_slot(vstab_handle *H, int slot) {
    vstab_handle::Slot &S = H->slots[slot];
    S.queued = false, S.freed_at = ++H->free_counter;
    if (!S.borrowed) {
        S.warp_pending = true, S.warped = -1;
        H->uncovered.push_back(slot);  // the next copy into this slot waits for an event recorded behind this warp
        if ((int)H->uncovered.size() >= vstab_handle::WARP_EVENT_STRIDE) VSTAB_TRY(H->cover_warps());
    } else if (!H->borrows.empty()) {
        for (vstab_handle::PendingBorrow &b : H->borrows)
            if (b.serial == S.ingest_serial) {
                b.warp_enqueued = true;
                if (++H->uncovered_borrows >= vstab_handle::WARP_EVENT_STRIDE) VSTAB_TRY(H->cover_warps());
                break;
            }
    }
    return VSTAB_OK;
}

// FrameSourceWarp::pull_frame, :452-476
static vstab_status pull_frame_impl(vstab_handle *H, int out_format, void *dst, size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv,
                                    const KeepPrev *keep = nullptr) {
    if (keep && (!H || !dst || !keep->prev || (out_has_chroma_plane(out_format) && (!dst_uv || !keep->prev_uv))))
        return fail(VSTAB_ERR_INVALID, std::string(keep->fn) + ": null argument");
    if (!H || !dst || (out_has_chroma_plane(out_format) && !dst_uv)) return fail(VSTAB_ERR_INVALID, "vstab_pull_frame: null argument");
    Pull P{out_format, dst, dst_uv, pitch_dst, pitch_dst_uv, H->border_mode, H->colour_matrix, H->colour_range, keep};
    VSTAB_TRY(refuse_formats(H, P));
    if (keep) VSTAB_TRY(refuse_keep(H, P));
    H->pulled = true;
    HT t_total(HostTimers::TOTAL);
    VSTAB_TRY(advance_until_due(H));
    if (H->queue.empty()) return VSTAB_EOF;  // :465-467
    smooth(H, P);
    VSTAB_TRY(choose_cached_map(H, P));
    HT t_warp(HostTimers::WARP);
    VSTAB_TRY(vstab_handle::wait_if_pending(H->stream, H->slots[P.slot].ingested));  // the slot was filled on the prefetch stream (long ago, as a rule)
    vstab_status st = launch_warp(H, P);
    if (st == VSTAB_OK && H->cfg.debug && !H->slots[P.slot].feats.empty() && !out_is_10bit(out_format)) {  // (markers are drawn into 8-bit outputs)
        VSTAB_TRY(H->marker_pts.ensure(sizeof(int) * 2 * MARKER_CAP * MARKER_SETS));
        st = draw_markers(H, P);
    }
    VSTAB_TRY(release_slot(H, P.slot));
    return st;
}

// vstab_set_border_mode / _ex: `resamplers`: whether a CUBIC or LANCZOS4 handle is served; `served`: how the refusal names what is
static vstab_status set_border_mode(vstab_handle *h, int border_mode, const char *fn, bool resamplers, const char *served) {
    if (!h) return fail(VSTAB_ERR_INVALID, std::string(fn) + ": null handle");
    if (!border_mode_valid(border_mode))
        return fail(VSTAB_ERR_INVALID, std::string(fn) + ": border_mode must be VSTAB_BORDER_CONSTANT (0), _REPLICATE (1), _REFLECT (2) or _REFLECT_101 (4)");
    if (border_mode != VSTAB_BORDER_CONSTANT && (h->cfg.pixel_depth == 10 || h->cfg.interpolation == 0 || (!resamplers && h->cfg.resample != VSTAB_RESAMPLE_DEFAULT)))
        return fail(VSTAB_ERR_UNSUPPORTED, std::string(fn) + ": border modes other than VSTAB_BORDER_CONSTANT are served for 8-bit pixels with " + served);
    if (border_mode != VSTAB_BORDER_CONSTANT && h->colour())
        return fail(VSTAB_ERR_UNSUPPORTED, std::string(fn) + ": a colour spec is set (vstab_set_colour), and the border warps convert with cvtColor's arithmetic");
    if (border_mode != VSTAB_BORDER_CONSTANT && h->calibrated && !h->calibrated_borders)
        return fail(VSTAB_ERR_INVALID, std::string(fn) + ": a calibrated handle (vstab_set_input_calibration) warps with VSTAB_BORDER_CONSTANT");
    h->border_mode = border_mode;
    return VSTAB_OK;
}

extern "C" {

vstab_status vstab_set_readout_warp(vstab_handle *h, int mode) {
    if (!h) return fail(VSTAB_ERR_INVALID, "vstab_set_readout_warp: null handle");
    if (mode != VSTAB_READOUT_REFUSE && mode != VSTAB_READOUT_PER_ROW)
        return fail(VSTAB_ERR_INVALID, "vstab_set_readout_warp: mode must be VSTAB_READOUT_REFUSE (0) or VSTAB_READOUT_PER_ROW (1)");
    if (h->cfg.pixel_depth == 10 || h->cfg.interpolation == 0)
        return fail(VSTAB_ERR_UNSUPPORTED, "vstab_set_readout_warp: served for 8-bit pixels with INTER_LINEAR, INTER_CUBIC or INTER_LANCZOS4");
    h->readout_warp = mode;
    return VSTAB_OK;
}

// The colour spec of the converting pulls.  The handles that are served are those whose warp is the bilinear fused kernel with one rotation
// per frame: every other kernel has cvtColor's constants.
vstab_status vstab_set_colour(vstab_handle *h, int matrix, int range) {
    const std::string n = "vstab_set_colour: ";
    if (!h) return fail(VSTAB_ERR_INVALID, n + "null handle");
    VSTAB_TRY(check_colour_spec("vstab_set_colour", matrix, range));
    if (!colour_spec_default(matrix, range)) {
        const char *why = h->cfg.pixel_depth == 10 ? "a pixel_depth 10 handle" : h->cfg.interpolation == 0 ? "INTER_NEAREST" :
                          h->cfg.resample != VSTAB_RESAMPLE_DEFAULT ? resample_name(h->cfg.resample) : h->calibrated ? "a calibrated handle (vstab_set_input_calibration)" :
                          h->pinhole ? "a calibrated handle (vstab_set_input_pinhole)" : h->border_mode != VSTAB_BORDER_CONSTANT ? "a border mode other than VSTAB_BORDER_CONSTANT (vstab_set_border_mode)" : nullptr;
        if (why) return fail(VSTAB_ERR_UNSUPPORTED, n + "a colour spec other than (VSTAB_COLOUR_CVTCOLOR, VSTAB_RANGE_LIMITED) is served for 8-bit pixels with INTER_LINEAR, the constant border and an ideal lens; this handle has " + why);
    }
    h->colour_matrix = matrix, h->colour_range = range;
    return VSTAB_OK;
}

// The colour spec of a pixel_depth 10 handle's converting pulls: every 10-bit warp kernel has its COLOUR form, so nothing about the handle refuses.
vstab_status vstab_set_colour10(vstab_handle *h, int matrix, int range) {
    if (!h) return fail(VSTAB_ERR_INVALID, "vstab_set_colour10: null handle");
    VSTAB_TRY(check_colour_spec("vstab_set_colour10", matrix, range));
    if (h->cfg.pixel_depth != 10)
        return fail(VSTAB_ERR_UNSUPPORTED, "vstab_set_colour10: served for pixel_depth 10 handles; the colour spec of an 8-bit handle is set with vstab_set_colour");
    h->colour10_matrix = matrix, h->colour10_range = range;
    return VSTAB_OK;
}

// The resampler and border mode of a pixel_depth 10 handle's plane-wise pull.  The values are checked before the handle is read; the handle
// is unchanged on every refusal.
vstab_status vstab_set_resample10(vstab_handle *h, int resample, int border_mode) {
    const std::string n = "vstab_set_resample10: ";
    if (!h) return fail(VSTAB_ERR_INVALID, n + "null handle");
    if (resample != VSTAB_RESAMPLE_DEFAULT && resample != VSTAB_RESAMPLE_CUBIC && resample != VSTAB_RESAMPLE_LANCZOS4)
        return fail(VSTAB_ERR_INVALID, n + "resample must be VSTAB_RESAMPLE_DEFAULT (0), _CUBIC (2) or _LANCZOS4 (4)");
    if (!border_mode_valid(border_mode))
        return fail(VSTAB_ERR_INVALID, n + "border_mode must be VSTAB_BORDER_CONSTANT (0), _REPLICATE (1), _REFLECT (2) or _REFLECT_101 (4)");
    if (resample == VSTAB_RESAMPLE_DEFAULT && border_mode != VSTAB_BORDER_CONSTANT)
        return fail(VSTAB_ERR_UNSUPPORTED, n + "VSTAB_RESAMPLE_DEFAULT (the bilinear warp) has the constant border at 10 bits; border modes are served with _CUBIC and _LANCZOS4");
    if (h->cfg.pixel_depth != 10)
        return fail(VSTAB_ERR_UNSUPPORTED, n + "served for pixel_depth 10 handles; an 8-bit handle takes its resampler from vstab_config.resample and its border mode from vstab_set_border_mode_ex");
    h->resample10 = resample, h->border10 = border_mode;
    return VSTAB_OK;
}

vstab_status vstab_pull_frame(vstab_handle *h, void *dst, size_t pitch_dst) { return pull_frame_impl(h, VSTAB_OUT_BGR8, dst, pitch_dst, nullptr, 0); }

vstab_status vstab_pull_frames(vstab_handle *h, int n, void *const *dst, const size_t *pitch_dst, int n_dst, int first, int *n_done) {
    if (n_done) *n_done = 0;
    if (!h || !dst || !pitch_dst || n < 0 || n_dst <= 0 || first < 0) return fail(VSTAB_ERR_INVALID, "vstab_pull_frames: bad argument");
    for (int i = 0; i < n; i++) {
        const int k = (int)(((long)first + i) % n_dst);
        const vstab_status st = pull_frame_impl(h, VSTAB_OUT_BGR8, dst[k], pitch_dst[k], nullptr, 0);
        if (st != VSTAB_OK) return st;
        if (n_done) *n_done = i + 1;
    }
    return VSTAB_OK;
}

vstab_status vstab_pull_frame_host(vstab_handle *h, void *dst, size_t pitch_dst) {
    if (!h || !dst || pitch_dst < (size_t)h->ow * 3) return fail(VSTAB_ERR_INVALID, "vstab_pull_frame_host: bad argument");
    const size_t dpitch = ((size_t)h->ow * 3 + 255) & ~(size_t)255;
    VSTAB_TRY(h->host_out.ensure(dpitch * h->oh));
    const vstab_status st = pull_frame_impl(h, VSTAB_OUT_BGR8, h->host_out.p, dpitch, nullptr, 0);
    if (st != VSTAB_OK) return st;
    VSTAB_HIP_TRY(hipMemcpy2DAsync(dst, pitch_dst, h->host_out.p, dpitch, (size_t)h->ow * 3, h->oh, hipMemcpyDeviceToHost, h->stream));
    VSTAB_HIP_TRY(hipStreamSynchronize(h->stream));
    return VSTAB_OK;
}

vstab_status vstab_pull_frame_bgr16(vstab_handle *h, void *dst, size_t pitch_dst) { return pull_frame_impl(h, OUT_BGR16, dst, pitch_dst, nullptr, 0); }

vstab_status vstab_pull_frame_p010(vstab_handle *h, void *dst_y, size_t pitch_y, void *dst_uv, size_t pitch_uv) {
    if (!h || !dst_y || !dst_uv) return fail(VSTAB_ERR_INVALID, "vstab_pull_frame_p010: null argument");
    // the warp writes the planes itself (OUT_P010) where the frame's planes allow the tiled kernel; pull_frame_impl falls back
    // to a 16-bit BGR buffer of the handle + vstab_cvt_bgr16_p010 otherwise
    return pull_frame_impl(h, OUT_P010, dst_y, pitch_y, dst_uv, pitch_uv);
}

vstab_status vstab_pull_frame_nv12(vstab_handle *h, void *dst_y, size_t pitch_y, void *dst_uv, size_t pitch_uv) { return pull_frame_impl(h, VSTAB_OUT_NV12, dst_y, pitch_y, dst_uv, pitch_uv); }

vstab_status vstab_pull_frame_nv12_planar(vstab_handle *h, void *dst_y, size_t pitch_y, void *dst_uv, size_t pitch_uv) { return pull_frame_impl(h, VSTAB_OUT_NV12_PLANAR, dst_y, pitch_y, dst_uv, pitch_uv); }

vstab_status vstab_pull_frame_p010_planar(vstab_handle *h, void *dst_y, size_t pitch_y, void *dst_uv, size_t pitch_uv) { return pull_frame_impl(h, OUT_P010_PLANAR, dst_y, pitch_y, dst_uv, pitch_uv); }

vstab_status vstab_pull_frame_keep(vstab_handle *h, void *dst, size_t pitch_dst, const void *prev, size_t pitch_prev) {
    const KeepPrev keep = {"vstab_pull_frame_keep", prev, nullptr, pitch_prev, 0};
    return pull_frame_impl(h, VSTAB_OUT_BGR8, dst, pitch_dst, nullptr, 0, &keep);
}

vstab_status vstab_pull_frame_nv12_planar_keep(vstab_handle *h, void *dst_y, size_t pitch_y, void *dst_uv, size_t pitch_uv, const void *prev_y, size_t pitch_prev_y,
                                               const void *prev_uv, size_t pitch_prev_uv) {
    const KeepPrev keep = {"vstab_pull_frame_nv12_planar_keep", prev_y, prev_uv, pitch_prev_y, pitch_prev_uv};
    return pull_frame_impl(h, VSTAB_OUT_NV12_PLANAR, dst_y, pitch_y, dst_uv, pitch_uv, &keep);
}

vstab_status vstab_peek_frame(vstab_handle *h, void *dst, size_t pitch_dst) { return vstab_pull_frame(h, dst, pitch_dst); }  // :478-480

vstab_status vstab_set_border_mode(vstab_handle *h, int border_mode) { return set_border_mode(h, border_mode, "vstab_set_border_mode", false, "INTER_LINEAR (interpolation 1) and resample VSTAB_RESAMPLE_DEFAULT"); }

vstab_status vstab_set_border_mode_ex(vstab_handle *h, int border_mode) { return set_border_mode(h, border_mode, "vstab_set_border_mode_ex", true, "INTER_LINEAR, INTER_CUBIC or INTER_LANCZOS4"); }

}  // extern "C"
