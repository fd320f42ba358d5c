// vstab_pipeline.cpp -- the FrameSourceWarp replacement behind the C ABI: tracking workspace, look-ahead ring in HBM, the steps of
// consume_frame (FrameSourceWarp.cpp:397-450), create / destroy and the getters.  Host C++; every pixel touches a HIP kernel.
#include <sys/stat.h>

#include <algorithm>

#include "vstab_pipeline.hpp"

// mem == VSTAB_MEM_DMABUF: the planes are offsets into a DMA-BUF object (an exported decoder surface).  Import the object
// once (objects are recognised by the inode of their fd: decoders hand the same pool of surfaces round and round, under
// fds that may be closed and reused) and rewrite the frame as ordinary device memory.  This is the zero-copy stand-in for
// AvFrameSourceMapOpenCl.cpp:17-66, which moves every frame VAAPI -> host -> OpenCL.
static vstab_status resolve_dmabuf(vstab_handle *H, vstab_frame &f) {
    if (f.mem != VSTAB_MEM_DMABUF) return VSTAB_OK;
    const size_t off_y = reinterpret_cast<uintptr_t>(f.y), off_uv = reinterpret_cast<uintptr_t>(f.uv);
    const size_t bps = f.bit_depth > 8 ? 2 : 1;
    if (f.dmabuf_fd < 0 || f.dmabuf_size == 0 || f.height <= 0 || off_y + f.pitch_y * (size_t)f.height > f.dmabuf_size ||
        off_uv + f.pitch_uv * (size_t)(f.height / 2) > f.dmabuf_size || f.pitch_y < (size_t)f.width * bps || f.pitch_uv < (size_t)f.width * bps)
        return fail(VSTAB_ERR_INVALID, "vstab_frame: DMA-BUF planes do not fit in the object (fd, size, offsets, pitches)");
    // AVDRMObjectDescriptor.format_modifier: the kernels address rows of `pitch` bytes, so a tiled or compressed surface would be
    // read as garbage without any error -- refuse everything but a linear layout (or "no modifier": the exporter's implicit, linear one)
    if (f.dmabuf_modifier != VSTAB_DRM_FORMAT_MOD_LINEAR && f.dmabuf_modifier != VSTAB_DRM_FORMAT_MOD_INVALID) {
        char mod[32];
        std::snprintf(mod, sizeof(mod), "0x%016llx", (unsigned long long)f.dmabuf_modifier);
        return fail(VSTAB_ERR_UNSUPPORTED, std::string("vstab_frame: DMA-BUF with format modifier ") + mod +
                                               " (tiled / compressed surface): only DRM_FORMAT_MOD_LINEAR is read; map the surface linear first");
    }
    struct stat sb;
    if (fstat(f.dmabuf_fd, &sb) != 0) return fail(VSTAB_ERR_INVALID, "vstab_frame: dmabuf_fd is not an open file descriptor");
    // ROCm's import maps the object (the kernel driver takes its own reference on the DMA-BUF) and neither consumes nor closes the
    // descriptor -- unlike CUDA's, which takes ownership.  So the caller's fd is handed over as it is: no duplicate to leak, and the
    // caller may close its fd as soon as the callback returns (test_dmabuf_import_leaves_no_descriptor_behind checks both).
    std::string err;
    auto import = [&](hipExternalMemory_t &ext, uint8_t *&base) {
        hipExternalMemoryHandleDesc hd;
        std::memset(&hd, 0, sizeof(hd));
        hd.type = hipExternalMemoryHandleTypeOpaqueFd, hd.handle.fd = f.dmabuf_fd, hd.size = f.dmabuf_size;
        hipError_t e = hipImportExternalMemory(&ext, &hd);
        if (e != hipSuccess) {
            err = std::string("hipImportExternalMemory(DMA-BUF): ") + hipGetErrorString(e);
            return false;
        }
        hipExternalMemoryBufferDesc bd;
        std::memset(&bd, 0, sizeof(bd));
        bd.offset = 0, bd.size = f.dmabuf_size;
        void *p = nullptr;
        e = hipExternalMemoryGetMappedBuffer(&p, ext, &bd);
        if (e != hipSuccess || !p) {
            (void)hipDestroyExternalMemory(ext);
            err = std::string("hipExternalMemoryGetMappedBuffer(DMA-BUF): ") + hipGetErrorString(e);
            return false;
        }
        base = static_cast<uint8_t *>(p);
        return true;
    };
    auto destroy = [&](hipExternalMemory_t &ext) {
        (void)hipStreamSynchronize(H->pstream);  // (rare: a copy out of the object may only just have been enqueued)
        (void)hipDestroyExternalMemory(ext);
    };
    // a frame stays in the pipeline for at most `slots` pulls (read-ahead + look-ahead window + warp)
    uint8_t *base = nullptr;
    if (!H->dmabufs.lookup((unsigned long long)sb.st_ino, f.dmabuf_size, (long)H->slots.size() + 2, import, destroy, base)) return fail(VSTAB_ERR_DEVICE, err);
    f.y = base + off_y, f.uv = base + off_uv, f.mem = VSTAB_MEM_DEVICE;
    return VSTAB_OK;
}

// pyr: the pyramid set the frame's levels go to; *level1_done: the copy kernel wrote level 1 as well (k_pack_pyr)
static vstab_status ingest(vstab_handle *H, const vstab_frame &f, int slot, int pyr, bool *level1_done) {
    *level1_done = false;
    GpuStage gs(H, vstab_handle::ST_INGEST);
    if (f.width != H->w || f.height != H->h) return fail(VSTAB_ERR_INVALID, "frame size changed mid-stream");
    vstab_handle::Slot &S = H->slots[slot];
    const bool wide = f.bit_depth > 8;
    if (f.bit_depth != 0 && f.bit_depth != 8 && f.bit_depth != 10 && f.bit_depth != 12 && f.bit_depth != 16)
        return fail(VSTAB_ERR_INVALID, "vstab_frame.bit_depth must be 8, 10, 12 or 16");
    if (wide && f.mem != 0) return fail(VSTAB_ERR_INVALID, "16-bit frames must be in device memory");
    if (H->cfg.pixel_depth == 10 && !wide) return fail(VSTAB_ERR_INVALID, "a pixel_depth 10 handle needs P010 device frames (vstab_frame.bit_depth > 8)");
    S.y16 = S.uv16 = nullptr;  // set again below when this frame has 16-bit planes to warp from
    S.copied_valid = false;
    // (the kernels form row offsets with 24-bit multiplies, into planes of less than 4 GiB: pack_pyr_ok and the warp's staging checks)
    if (f.mem == 0 && !wide && f.hold >= H->borrow_hold && f.pitch_y < (1u << 24) && f.pitch_uv < (1u << 24) && (uint64_t)f.pitch_y * f.height < (1ull << 32) &&
        (uint64_t)f.pitch_uv * (f.height / 2) < (1ull << 32)) {
        // zero copy: track, build the pyramid from and warp upstream's planes where they are
        S.y = static_cast<const uint8_t *>(f.y), S.uv = static_cast<const uint8_t *>(f.uv), S.pitch_y = f.pitch_y, S.pitch_uv = f.pitch_uv;
        S.borrowed = true, S.warp_pending = false, S.warped = -1;
        H->frames_borrowed++;
        return VSTAB_OK;  // (S.ingested keeps its completed state from the slot's previous use; tracking records it behind the pyramid)
    }
    VSTAB_TRY(S.buf.ensure((size_t)H->w * H->h * 3 / 2));
    uint8_t *dst = S.buf.as<uint8_t>();
    S.y = dst, S.uv = dst + (size_t)H->w * H->h, S.pitch_y = S.pitch_uv = (size_t)H->w, S.borrowed = false;
    H->frames_copied++;
    if (S.warp_pending) {  // the warp that last read this slot runs on another stream
        if (S.warped < 0) VSTAB_TRY(H->cover_warps());
        VSTAB_TRY(vstab_handle::wait_if_pending(H->pstream, H->warp_events[S.warped]));
        S.warp_pending = false, S.warped = -1;
    }
    if (wide) {
        VSTAB_TRY(pack_p010_planes(f.y, f.pitch_y, f.uv, f.pitch_uv, f.width, f.height, dst, H->cfg.pixel_depth == 10, H->pstream));
        if (H->cfg.pixel_depth == 10) {  // the warp reads the 16-bit planes; the tracker the narrowed luma above
            const size_t row = (size_t)H->w * 2;
            if (f.hold >= vstab_handle::HOLD_FOREVER) {
                S.y16 = static_cast<const uint8_t *>(f.y), S.uv16 = static_cast<const uint8_t *>(f.uv), S.pitch_y16 = f.pitch_y, S.pitch_uv16 = f.pitch_uv;
            } else {
                VSTAB_TRY(S.buf16.ensure(row * H->h * 3 / 2));
                uint8_t *d16 = S.buf16.as<uint8_t>();
                VSTAB_HIP_TRY(hipMemcpy2DAsync(d16, row, f.y, f.pitch_y, row, H->h, hipMemcpyDeviceToDevice, H->pstream));
                VSTAB_HIP_TRY(hipMemcpy2DAsync(d16 + row * H->h, row, f.uv, f.pitch_uv, row, H->h / 2, hipMemcpyDeviceToDevice, H->pstream));
                S.y16 = d16, S.uv16 = d16 + row * H->h, S.pitch_y16 = S.pitch_uv16 = row;
            }
        }
        // upstream's surface is free once these copies are through (not the pyramid behind them: see pack_nv12_planes) -- an event of its own,
        // but only for a frame somebody will wait for: a marker packet per frame costs the read-ahead stream what it saves the caller
        if (H->cfg.tracking && f.hold < (int)H->slots.size()) {
            VSTAB_HIP_TRY(hipEventRecord(S.copied, H->pstream));
            S.copied_valid = true;
        }
    } else if (f.mem == 0) {
        // (while tracking, `ingested` completes with the pyramid enqueued behind the copy: upstream's surface is free as soon as the copy is)
        S.copied_valid = H->cfg.tracking != 0;
        static const bool fuse = getenv("VSTAB_PACK_PYR") == nullptr || atoi(getenv("VSTAB_PACK_PYR")) != 0;  // development: =0 copies and builds level 1 in two launches
        uint8_t *l1 = H->cfg.tracking ? H->tracker.level1(pyr) : nullptr;
        if (fuse && l1 && pack_pyr_ok(f.y, f.pitch_y, f.uv, f.pitch_uv, f.width, f.height, dst, l1, H->tracker.level1_pitch())) {
            // one pass over the luma plane: the copy into the ring and the first pyramid level (k_pack_pyr)
            VSTAB_TRY(launch_pack_pyr(static_cast<const uint8_t *>(f.y), f.pitch_y, static_cast<const uint8_t *>(f.uv), f.pitch_uv, f.width, f.height, dst, l1,
                                      H->tracker.level1_pitch(), H->pstream, S.copied));
            *level1_done = true;
        } else
        VSTAB_TRY(pack_nv12_planes(f.y, f.pitch_y, f.uv, f.pitch_uv, f.width, f.height, dst, H->pstream, S.copied_valid ? S.copied : nullptr));
    } else {
        VSTAB_HIP_TRY(hipMemcpy2DAsync(dst, H->w, f.y, f.pitch_y, H->w, H->h, hipMemcpyHostToDevice, H->pstream));
        VSTAB_HIP_TRY(hipMemcpy2DAsync(dst + (size_t)H->w * H->h, H->w, f.uv, f.pitch_uv, H->w, H->h / 2, hipMemcpyHostToDevice, H->pstream));
        VSTAB_HIP_TRY(hipStreamSynchronize(H->pstream));  // the caller may reuse its host buffer on return
    }
    if (!H->cfg.tracking) VSTAB_HIP_TRY(hipEventRecord(S.ingested, H->pstream));  // tracking: recorded behind the pyramid instead
    return VSTAB_OK;
}

// ---------------------------------------------------------------------------------------------
// consume_frame (FrameSourceWarp.cpp:397-450) split into steps so that the copy + pyramid of the frames read ahead,
// the (chained) LK tracking of frames k+1 and k+2 and the speculative corner detection run on the GPU while the host
// estimates the rotation of frame k (PREFETCH_DEPTH frames of upstream read-ahead; four HIP streams ordered by events;
// DESIGN.md section 5b):
//   prefetch_next    pull the next upstream frame, copy it into the ring unless upstream holds it, build its pyramid
//                    (pstream); start the speculative corner detection when the counter says a key frame is coming
//   launch_tracking  key-frame rule (:415-419); adopt the launch chained behind the previous frame's tracker or launch
//                    one; chain the next frame's tracker (tstream)
//   finish_wait      LK results -> surviving pairs (:422-427)
//   post_estimate / finish_estimate  rotation (worker thread) + fallback + accumulation + filter.add + queue push (:429-446)
// Every step runs in frame order, so every decision, random draw and queue entry is the one the
// reference makes; only WHEN the upstream callback is called moves (up to PREFETCH_DEPTH + 1 frames earlier).
// ---------------------------------------------------------------------------------------------
// prefetch_next: upstream callback, copy into the ring, pyramid -- all on the prefetch stream, with no
// dependence on the tracking state, so it overlaps the LK kernel of the previous frame.
vstab_status prefetch_next(vstab_handle *H) {
    vstab_frame f;
    std::memset(&f, 0, sizeof(f));
    {
        // copies of frames whose planes upstream may recycle on this call must have finished (vstab_frame.hold)
        HT t(HostTimers::INGEST_SYNC);
        for (auto it = H->copies.begin(); it != H->copies.end();) {
            if (it->hold > 0) {
                it->hold--, ++it;
                continue;
            }
            const vstab_handle::Slot &S = H->slots[it->slot];
            if (S.ingest_serial == it->serial)  // (a re-used slot's newer copy was enqueued behind this one: also done)
                VSTAB_TRY(vstab_handle::host_wait(S.copied_valid ? S.copied : S.ingested));
            it = H->copies.erase(it);
        }
        // frames used in place: the warp reading them must be through before the callback that ends upstream's promise
        for (auto it = H->borrows.begin(); it != H->borrows.end();) {
            if (it->hold > 0) {
                it->hold--, ++it;
                continue;
            }
            if (!it->warp_enqueued)
                return fail(VSTAB_ERR_INVALID, "vstab_frame.hold ran out while the frame was still waiting in the look-ahead window");
            if (it->warped < 0) VSTAB_TRY(H->cover_warps());
            VSTAB_TRY(vstab_handle::host_wait(H->warp_events[it->warped]));
            it = H->borrows.erase(it);
        }
    }
    int rc;
    {
        HT t(HostTimers::PULL_CB);
        rc = H->src.pull(H->src.user, &f);
    }
    if (rc == VSTAB_EOF) {
        H->src_eof = true;
        return VSTAB_EOF;
    }
    if (rc != 0) {
        // The reference meets this error only when it consumes the failing frame (FrameSourceWarp.cpp:453-455), after it
        // has emitted every frame whose look-ahead window was complete; the frames read ahead here are still used.
        H->src_eof = true, H->src_error = rc;
        return VSTAB_EOF;
    }
    VSTAB_TRY(resolve_dmabuf(H, f));  // a DMA-BUF frame becomes an ordinary device frame here
    const int slot = H->acquire_slot();
    if (slot < 0) return fail(VSTAB_ERR_NOMEM, "look-ahead ring exhausted");
    const int pyr = (int)(H->prefetch_count % PYR_SETS);
    bool level1_done = false;
    {
        HT t(HostTimers::INGEST);
        VSTAB_TRY(ingest(H, f, slot, pyr, &level1_done));
    }
    H->last_ingest_slot = slot;
    H->slots[slot].have_delta = f.delta_rotation != nullptr;
    if (f.delta_rotation) std::memcpy(H->slots[slot].delta.m, f.delta_rotation, sizeof(double) * 9);
    H->slots[slot].have_readout = f.readout_rotation != nullptr;
    if (f.readout_rotation) {
        if (H->cfg.pixel_depth != 10 && H->map_mode != VSTAB_MAP_CREATEMAP_CL && H->map_mode != VSTAB_MAP_FISH_TO_RECT &&
            H->map_mode != VSTAB_MAP_CREATEMAP_CL_OPENCL)
            return fail(VSTAB_ERR_INVALID, "vstab_frame.readout_rotation: the 8-bit rolling-shutter warp exists for the preset and fisheye -> rectilinear maps only");
        std::memcpy(H->slots[slot].readout.m, f.readout_rotation, sizeof(double) * 9);
    }
    H->slots[slot].ingest_serial = ++H->ingest_serial;
    // (frames promised to outlive a whole ring of pulls are not tracked: the ring slot itself is recycled sooner)
    if (f.mem == 0 && !H->slots[slot].borrowed && f.hold < (int)H->slots.size())
        H->copies.push_back({slot, H->ingest_serial, f.hold < 0 ? 0 : f.hold});
    if (H->slots[slot].borrowed && f.hold < vstab_handle::HOLD_FOREVER) H->borrows.push_back({H->ingest_serial, f.hold, false, -1});
    H->slots[slot].queued = true;  // reserved from now on (released when its warp has been enqueued)
    if (H->cfg.tracking) {
        HT t(HostTimers::PYRAMID);
        GpuStage gs(H, vstab_handle::ST_PYRAMID);
        // `ingested` = copy AND pyramid of this frame: the event completes with the pyramid's last kernel (no marker packet on the stream)
        static const bool bind_event = getenv("VSTAB_PYR_EVENT_RECORD") == nullptr;  // development: =1 records the event behind the kernels instead
        bool bound = false;
        VSTAB_TRY(H->tracker.build_pyramid(pyr, H->gray(slot), H->gpitch(slot), H->pstream, bind_event ? H->slots[slot].ingested : nullptr, &bound, level1_done));
        if (!bound) VSTAB_HIP_TRY(hipEventRecord(H->slots[slot].ingested, H->pstream));
    }
    // Key-frame rule, counter half (:415): the frame after this one re-detects corners on THIS frame when
    // (index + 1) - last_key > 20.  That is known now, so the detector runs here, on the prefetch stream,
    // a whole frame period before its result is needed; launch_tracking falls back to detecting on demand
    // if the prediction turns out wrong (an extra key frame in between) or the candidates overflow.
    // (The rule has not been evaluated yet for the frames still in the read-ahead window; "== 21" is the
    // one frame for which it is false for every pending frame and true for the next.)
    if (H->cfg.tracking && H->speculate && H->last_key != -1 && (H->prefetch_count + 1) - H->last_key == 21)
    {
        if (debug_spec()) std::fprintf(stderr, "spec launch for frame %ld (last_key %ld)\n", H->prefetch_count, H->last_key);
        HT t(HostTimers::SPEC_DETECT);
        hipStream_t ds = H->dstream ? H->dstream : H->pstream;
        if (H->epoch_overlap) H->spec_stream = 1 - H->epoch_stream, ds = H->estream(H->spec_stream);  // the epoch after the newest one enqueued
        // the detector reads the frame's luma plane, nothing else: it waits for the copy into the ring (if there was one), not for the
        // pyramid enqueued behind it -- beside a saturating warp the detection needs most of the read-ahead's lead as it is
        if (ds != H->pstream) {
            const vstab_handle::Slot &DS = H->slots[slot];
            if (!DS.borrowed) VSTAB_HIP_TRY(hipStreamWaitEvent(ds, DS.copied_valid ? DS.copied : DS.ingested, 0));
        }
        VSTAB_TRY(H->detector.spec_launch(H->gray(slot), H->gpitch(slot), 0.01, ds, H->prefetch_count));
        H->detector.spec_select_async(200, 30.0);
    }
    H->prefetched.emplace_back(slot, pyr);
    H->prefetch_count++;
    return VSTAB_OK;
}

// undistort-only mode (BASELINE config 1): every frame gets the identity rotation
static void queue_untracked(vstab_handle *H, int slot) {
    if (H->last_key == -1) {
        H->last_key = H->frame_index;
        H->slots[slot].queued = false;  // the first frame is never emitted (:403-407)
        H->forget_borrow(H->slots[slot].ingest_serial);
    } else {
        if (H->slots[slot].have_delta) H->measured = H->slots[slot].delta * H->measured;  // :441 with the sensor's rotation
        if (H->sg) H->sg->add(H->measured);
        H->queue.emplace_back(slot, H->measured);
    }
}

// :403-407 the first frame only seeds the corner set
static vstab_status seed_corners(vstab_handle *H, int slot, const uint8_t *g, size_t pitch) {
    H->last_key = H->frame_index;
    VSTAB_HIP_TRY(hipStreamWaitEvent(H->tstream, H->slots[slot].ingested, 0));
    {
        HostStage hs(&H->prof.host_corners_ms);
        VSTAB_TRY(H->detector.good_features(g, pitch, 200, 0.01, 30.0, H->corners, H->tstream));
    }
    H->prof.key_frames++;
    H->slots[slot].queued = false;
    H->forget_borrow(H->slots[slot].ingest_serial);
    return VSTAB_OK;
}

// every later frame: key-frame rule, the launch that covers the frame (adopted or made now) and the launches enqueued ahead of it
static vstab_status track_frame(vstab_handle *H, int slot, int pyr, const uint8_t *g, size_t pitch) {
    vstab_handle::Tracked &T = H->inflight;
    T = vstab_handle::Tracked();
    T.slot = slot;
    const long F = H->frame_index;
    const uint8_t *pg = H->gray(H->last_slot);
    const size_t ppitch = H->gpitch(H->last_slot);
    // pyramid of a frame at or after F - 1 (all of them are in the ring: F - 1 is the last tracked frame, F the one launch_tracking
    // popped, the following ones wait in `prefetched`)
    auto pyr_of = [&](long fr) {
        if (fr == F - 1) return H->tracker.pyramid(H->cur_pyr, pg, ppitch);
        if (fr == F) return H->tracker.pyramid(pyr, g, pitch);
        const auto &pf = H->prefetched[(size_t)(fr - F - 1)];
        return H->tracker.pyramid(pf.second, H->gray(pf.first), H->gpitch(pf.first));
    };
    auto slot_of = [&](long fr) { return fr == F ? slot : H->prefetched[(size_t)(fr - F - 1)].first; };
    // the last frame read ahead whose copy + pyramid (prefetch stream) have COMPLETED, as far as the host can see without
    // waiting: a launch may only start once the pyramid of its last frame exists, so a segment that reached for the
    // frame pulled a moment ago would hold all its earlier frames back (measured: segments of 8 were slower than of 1)
    long reach = F;
    for (size_t j = 0; j < H->prefetched.size(); j++) {
        if (hipEventQuery(H->slots[H->prefetched[j].first].ingested) != hipSuccess) {
            (void)hipGetLastError();  // "not ready" is an answer, not an error the next launch check should find
            break;
        }
        reach = F + 1 + (long)j;
    }
    auto drop_segments = [&]() {
        for (const auto &sg : H->segs) H->seg_frames_dropped += sg.first + sg.n - std::max(sg.first, F);
        H->segs.clear();
    };
    // enqueue a segment of n frames from `first` on: from `start` (host points) or chained behind `parent`
    auto launch_segment = [&](long first, int n, bool key, const std::vector<float> *start, const Tracker::Launch *parent, long last_key_after,
                              bool timed, int stream_idx) -> vstab_status {
        LkPyramid pyrs[LK_SEG_MAX + 1];
        for (int i = 0; i <= n; i++) pyrs[i] = pyr_of(first - 1 + i);
        const hipStream_t es = H->estream(stream_idx);
        // copy + pyramid of the segment's frames: they are enqueued in frame order on the prefetch stream, the last one covers all
        VSTAB_TRY(vstab_handle::wait_if_pending(es, H->slots[slot_of(first + n - 1)].ingested));
        vstab_handle::Segment sg;
        sg.first = first, sg.n = n, sg.key = key, sg.last_key_after = last_key_after, sg.stream = stream_idx;
        if (start) {
            if (key) sg.corners = *start;
            VSTAB_TRY(H->tracker.track_launch(pyrs, n, *start, es, timed, sg.launch));
        } else {
            VSTAB_TRY(H->tracker.track_launch_chained(pyrs, n, *parent, es, sg.launch));  // (behind its parent: the same stream)
        }
        H->segs_launched++, H->seg_frames_launched += n;
        H->segs.push_back(std::move(sg));
        return VSTAB_OK;
    };
    while (!H->segs.empty() && H->segs.front().first + H->segs.front().n <= F) H->segs.pop_front();  // used up
    // :415-419 key-frame rule; corners are found in the PREVIOUS gray frame
    const bool is_key = F - H->last_key > 20 || H->corners.size() / 2 < 150;
    const vstab_handle::Segment *front = H->segs.empty() ? nullptr : &H->segs.front();
    // what was enqueued for this frame stands if it made the same decision: a key segment starting here for a key frame,
    // the inside of a segment (or the start of a chained one) for an ordinary frame
    const bool covered = front && front->first <= F;
    const bool planned_key = covered && front->key && front->first == F;
    bool adopt = covered && planned_key == is_key;
    if (covered && !adopt) H->chained_discarded++;
    if (is_key) {
        H->last_key = F - 1;
        HostStage hs(&H->prof.host_corners_ms);
        if (adopt) {
            H->corners = front->corners;  // this key frame's tracker is already running on them
            H->key_prelaunched++;
        } else {
            // the previous frame is F - 1: use its speculative detection if there is one
            const bool spec = H->detector.spec_tag() == F - 1 && H->detector.spec_finish(200, 30.0, H->corners);
            if (debug_spec()) std::fprintf(stderr, "key frame at %ld: spec_tag %ld used %d\n", F, H->detector.spec_tag(), (int)spec);
            if (!spec) VSTAB_TRY(H->detector.good_features(pg, ppitch, 200, 0.01, 30.0, H->corners, H->tstream));
        }
        T.lg.key_frame = 1;
        H->prof.key_frames++;
    }
    T.lg.n_corners = (int)(H->corners.size() / 2);
    T.prev = H->corners;
    // how many frames a launch may cover: the whole read-ahead when launches are chained ahead, one frame otherwise
    const bool ahead = H->chain_lk && H->profiling < 2;
    const int seg_max = ahead ? H->seg_max : 1;
    if (adopt) {
        H->chained_adopted++;
    } else {
        // everything enqueued ahead assumed another course of events (or nothing was enqueued): start afresh from the host's
        // corner list.  Dropped launches may still be running; this one queues behind them on the tracker stream.
        drop_segments();
        HT t(HostTimers::LK_LAUNCH);
        const long kc = H->last_key + 21;  // the next frame the counter makes a key frame
        const int n = (int)std::max<long>(1, std::min<long>({(long)seg_max, reach - F + 1, kc - F}));
        if (H->epoch_overlap) {  // whatever is still queued on the other epoch stream was dropped a moment ago (or is long finished): behind it
            VSTAB_HIP_TRY(hipEventRecord(H->epoch_tail, H->dstream));
            VSTAB_HIP_TRY(hipStreamWaitEvent(H->tstream, H->epoch_tail, 0));
        }
        H->epoch_stream = 0;
        VSTAB_TRY(launch_segment(F, n, false, &H->corners, nullptr, H->last_key, H->profiling >= 2, 0));
    }
    H->inflight_launch = H->segs.front().launch, H->inflight_idx = (int)(F - H->segs.front().first), H->inflight_stream = H->segs.front().stream;
    H->have_inflight = true;
    // Enqueue further segments as far as the read-ahead reaches: chained behind the last one up to the next key frame the
    // counter half of the rule (:415) predicts, and -- once that key frame's corners (detected speculatively on the frame before
    // it) are selected -- a segment from those corners, which does not depend on any earlier tracking at all.  The count half
    // (< 150 survivors) is checked when a frame's turn comes; if it fires, what was enqueued beyond is dropped (above).
    while (ahead) {
        HT t(HostTimers::LK_CHAIN);
        const vstab_handle::Segment &back = H->segs.back();
        const long tail = back.first + back.n - 1, next = tail + 1, avail = reach - tail;
        if (avail <= 0 || back.launch.n_slots == 0) break;
        const long kc = back.last_key_after + 21;  // next planned key frame
        if (next == kc) {
            if (H->detector.spec_tag() == tail) H->detector.spec_poll_inline();
            if (H->detector.spec_tag() != tail || H->detector.spec_state() != 2) {
                if (debug_spec() && H->detector.spec_tag() == tail)
                    std::fprintf(stderr, "frame %ld: corners for key frame %ld not selected yet (state %d)\n", F, next, H->detector.spec_state());
                break;  // not detected / selected yet: next pull, or on demand when the host gets there
            }
            std::vector<float> fresh;
            H->detector.spec_take(fresh);
            const int n = (int)std::min<long>({(long)seg_max, avail, 21});
            const int es = H->epoch_overlap ? H->spec_stream : 0;  // where its detection ran: not the stream of the epoch before it
            VSTAB_TRY(launch_segment(next, n, true, &fresh, nullptr, next - 1, false, es));
            H->epoch_stream = es;
            if (es == 1) H->epochs_on_second_stream++;
            continue;
        }
        const int n = (int)std::min<long>({(long)seg_max, avail, kc - next});
        // full segments; shorter ones only up to a key frame, or when nothing is enqueued beyond the host's frame
        if (n < H->seg_target && next + n != kc && tail > F) break;
        VSTAB_TRY(launch_segment(next, n, false, nullptr, &back.launch, back.last_key_after, false, back.stream));
    }
    return VSTAB_OK;
}

// launch_tracking: key-frame rule (:415-419) and the LK launch for the prefetched frame.  Needs the
// surviving corners of the previous frame (finish_wait), i.e. runs in frame order.
vstab_status launch_tracking(vstab_handle *H) {
    const int slot = H->prefetched.front().first, pyr = H->prefetched.front().second;
    H->prefetched.pop_front();
    const size_t pitch = H->gpitch(slot);
    const uint8_t *g = H->gray(slot);
    if (!H->cfg.tracking) queue_untracked(H, slot);
    else if (H->last_key == -1) VSTAB_TRY(seed_corners(H, slot, g, pitch));
    else VSTAB_TRY(track_frame(H, slot, pyr, g, pitch));
    H->cur_pyr = pyr;
    H->prof.frames_consumed++;
    if (H->last_slot >= 0) {
        H->slots[H->last_slot].last = false;
        if (!H->slots[H->last_slot].queued) H->slots[H->last_slot].freed_at = ++H->free_counter;
    }
    H->slots[slot].last = true;
    H->last_slot = slot;  // :448
    ++H->frame_index;     // :449
    return VSTAB_OK;
}

vstab_status finish_wait(vstab_handle *H) {
    if (!H->have_inflight) return VSTAB_OK;
    vstab_handle::Tracked &T = H->inflight;
    std::vector<float> nxt;
    std::vector<uint8_t> st;
    {
        HostStage hs(&H->prof.host_track_wait_ms);
        VSTAB_TRY(H->tracker.track_wait(H->inflight_launch, H->inflight_idx, T.prev.size() / 2, nxt, st, H->estream(H->inflight_stream),
                                        H->profiling >= 2 ? &H->prof.gpu_lk_ms : nullptr));
    }
    // :261-268 keep pairs with status != 0
    for (size_t i = 0; i < st.size(); i++)
        if (st[i]) {
            T.pp.push_back(T.prev[2 * i]), T.pp.push_back(T.prev[2 * i + 1]);
            T.cp.push_back(nxt[2 * i]), T.cp.push_back(nxt[2 * i + 1]);
        }
    H->corners = T.cp;  // :427
    T.lg.n_tracked = (int)(T.cp.size() / 2);
    H->ready = std::move(T);
    H->have_ready = true, H->have_inflight = false;
    return VSTAB_OK;
}

// start the rotation estimate of the ready frame on the worker thread (:429-431).  The frame moves on to `estimating`, so
// that the next frame's LK results can be read while this estimate runs: the worker gets a whole frame period (the launches
// of the following frames, the warp of the emitted one, the caller's own code) instead of the few microseconds between two
// steps of one call.  Estimates are still computed and applied strictly in frame order (one at a time: the random stream,
// the < 40 inlier fallback and the accumulation of :441 are sequential).
void post_estimate(vstab_handle *H) {
    if (!H->have_ready || H->have_estimating) return;
    H->estimating = std::move(H->ready);
    H->have_ready = false, H->have_estimating = true;
    if (!H->threaded_estimate) return;  // computed by finish_estimate on the calling thread
    vstab_handle::Tracked &T = H->estimating;
    H->worker.post(T.pp.data(), T.cp.data(), T.lg.n_tracked, &H->Kin, &H->Kout, &H->rng, H->in_fish, H->distortion());
    H->estimate_posted = true;
}

void finish_estimate(vstab_handle *H) {
    if (!H->have_estimating) return;
    vstab_handle::Tracked &T = H->estimating;
    vstab_frame_log &lg = T.lg;
    // :429-438 rotation since the last frame, with the < 40 inlier fallback
    Mat3 R;
    int inl;
    {
        HostStage hs(&H->prof.host_estimate_ms);  // threaded: only the time the caller still had to wait
        if (H->estimate_posted)
            inl = H->worker.join(R), H->estimate_posted = false;
        else
            inl = estimate_rotation(T.pp.data(), T.cp.data(), lg.n_tracked, H->Kin, H->Kout, H->rng, R, H->in_fish, H->distortion());
    }
    lg.n_inliers = inl;
    if (inl < 40) {
        R = H->have_last_rot ? H->last_rot : Mat3::identity();
        lg.fallback = 1;
    }
    H->last_rot = R, H->have_last_rot = true;
    H->measured = R * H->measured;  // :441 left-multiplied accumulation
    if (H->sg) H->sg->add(H->measured);
    H->queue.emplace_back(T.slot, H->measured);
    if (H->cfg.debug) H->slots[T.slot].feats = T.cp;
    std::memcpy(lg.R_frame, R.m, sizeof(R.m));
    std::memcpy(lg.R_accum, H->measured.m, sizeof(R.m));
    H->log.push_back(lg);
    if (H->log.size() > vstab_handle::LOG_KEEP) H->log.pop_front(), H->log_base++;
    H->have_estimating = false;
}

extern "C" {

vstab_status vstab_create(const vstab_config *cfg, const vstab_source *src, vstab_handle **out) {
    if (!cfg || !src || !out || !src->pull || !src->peek) return fail(VSTAB_ERR_INVALID, "vstab_create: null argument");
    if (cfg->abi_version != VSTAB_ABI_VERSION)
        return fail(VSTAB_ERR_INVALID, "vstab_create: vstab_config.abi_version is " + std::to_string(cfg->abi_version) + ", this library is version " +
                                           std::to_string(VSTAB_ABI_VERSION) + ": initialise the struct with vstab_config_default() of THIS library (include/vstab.h)");
    if (cfg->smooth_radius < 0 || cfg->smooth_radius > 10000) return fail(VSTAB_ERR_INVALID, "vstab_create: bad smooth_radius");
    if (cfg->interpolation != 1 && cfg->interpolation != 0)
        return fail(VSTAB_ERR_INVALID, "vstab_create: interpolation must be INTER_LINEAR (1, the only mode the reference passes) or INTER_NEAREST (0)");
    if (cfg->interpolation == 0 && (cfg->lens_mode != 0 || cfg->pixel_depth == 10))
        return fail(VSTAB_ERR_INVALID, "vstab_create: INTER_NEAREST exists for the reference's own map (lens_mode 0, 8-bit pixels)");
    if (cfg->resample != VSTAB_RESAMPLE_DEFAULT && cfg->resample != VSTAB_RESAMPLE_CUBIC && cfg->resample != VSTAB_RESAMPLE_LANCZOS4)
        return fail(VSTAB_ERR_INVALID,
                    "vstab_create: resample must be VSTAB_RESAMPLE_DEFAULT (0), VSTAB_RESAMPLE_CUBIC (2) or VSTAB_RESAMPLE_LANCZOS4 (4)");
    if (cfg->resample != VSTAB_RESAMPLE_DEFAULT && (cfg->interpolation != 1 || cfg->pixel_depth == 10))
        return fail(VSTAB_ERR_INVALID, std::string("vstab_create: ") + resample_name(cfg->resample) + " needs interpolation = INTER_LINEAR (1) and 8-bit pixels");
    if (!(cfg->scale > 0) || !(cfg->zoom > 0)) return fail(VSTAB_ERR_INVALID, "vstab_create: scale and zoom must be positive");
    if (cfg->smoother < VSTAB_SMOOTHER_SG || cfg->smoother > VSTAB_SMOOTHER_FIXED) return fail(VSTAB_ERR_INVALID, "vstab_create: unknown smoother");
    if (cfg->lens_mode != 0 && cfg->lens_mode != 1) return fail(VSTAB_ERR_INVALID, "vstab_create: lens_mode must be 0 or 1");
    if (cfg->pixel_depth != 0 && cfg->pixel_depth != 8 && cfg->pixel_depth != 10) return fail(VSTAB_ERR_INVALID, "vstab_create: pixel_depth must be 8 or 10");
    if (cfg->blend != VSTAB_BLEND_EXACT && cfg->blend != VSTAB_BLEND_FP16) return fail(VSTAB_ERR_INVALID, "vstab_create: unknown blend");
    if (cfg->map_precision != VSTAB_MAP_PRECISION_IEEE && cfg->map_precision != VSTAB_MAP_PRECISION_OPENCL)
        return fail(VSTAB_ERR_INVALID, "vstab_create: unknown map_precision");
    if (cfg->read_ahead < 0 || cfg->read_ahead > PREFETCH_MAX)
        return fail(VSTAB_ERR_INVALID, "vstab_create: read_ahead must be 0 (the default, " + std::to_string(PREFETCH_DEPTH) + ") or 1 .. " + std::to_string(PREFETCH_MAX));
    // (lens_mode 1 ignores map_precision: those maps are this library's own definitions, IEEE arithmetic throughout)
    std::unique_ptr<vstab_handle> H(new vstab_handle);
    H->cfg = *cfg, H->src = *src;
    H->rng = Pcg32(cfg->seed);
    if (const char *e = getenv("VSTAB_SPECULATE")) H->speculate = atoi(e) != 0;
    if (const char *e = getenv("VSTAB_THREADED_ESTIMATE")) H->threaded_estimate = atoi(e) != 0;
    if (const char *e = getenv("VSTAB_CHAIN_LK")) H->chain_lk = atoi(e) != 0;
    if (const char *e = getenv("VSTAB_LK_SEGMENT")) H->seg_max = std::max(1, std::min(atoi(e), LK_SEG_MAX));
    H->seg_target = std::min(H->seg_target, H->seg_max);
    if (const char *e = getenv("VSTAB_MAP_CACHE")) H->map_cache = atoi(e) != 0;
    if (const char *e = getenv("VSTAB_DMABUF_CACHE")) H->dmabufs.cap = std::max(1, atoi(e));
    H->stream = static_cast<hipStream_t>(cfg->stream);  // NULL = the default stream, as for the stateless operators
    {
        // the tracking chain is the per-frame critical path; the warp only has to finish before the
        // caller looks at dst, so the tracking stream gets the highest priority the device offers
        // every code object of the library now, not at the first launch of one of its kernels in the middle of the frame loop (and not after
        // whatever else the process has loaded and unloaded by then: vstab.h, vstab_preload_kernels)
        VSTAB_TRY(vstab_preload_kernels());
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        VSTAB_HIP_TRY(hipStreamCreateWithPriority(&H->tstream, hipStreamNonBlocking, hi));
        // copy + pyramid of the NEXT frame have a whole frame period of slack: lowest priority, so they fill
        // in behind the warp instead of taking its CUs
        VSTAB_HIP_TRY(hipStreamCreateWithPriority(&H->pstream, hipStreamNonBlocking, lo));
        // (this runtime offers two priority levels; beside a saturating warp the detection takes ~500 us at either)
        // The runtime multiplexes its streams onto four hardware queues, and two streams that share one serialise (a fifth
        // stream cost the 4K pipeline 4 k frames/s merely by existing): caller + tracker + prefetch leave ONE more: the
        // speculative corner detection's.
        // A caller that hands over a stream of its own very likely has the default stream in the process as well (any synchronous copy
        // uses it): with the detection's stream that makes five, and the fifth costs 15 % of the 4K rate and 10 % at 1080p, where queueing
        // the detection on the read-ahead stream costs 0.7 % and 3.5 % (profiles/r04_stream_count_ab.txt).  So the detection gets a stream
        // of its own only beside a caller on the default stream; VSTAB_DETECT_STREAM=1 / 0 overrides.
        const char *ds_env = getenv("VSTAB_DETECT_STREAM");
        const bool detect_stream = ds_env ? atoi(ds_env) != 0 : H->stream == nullptr;
        // (epochs in turn, below: the stream keeps the low priority -- at the tracker's priority the 4K rate lost 1.5 %, the 1080p rate gained nothing)
        if (detect_stream) VSTAB_HIP_TRY(hipStreamCreateWithPriority(&H->dstream, hipStreamNonBlocking, lo));
        for (auto &e : H->warp_events) VSTAB_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    // :214-219 peek the first frame for the input size, then derive both cameras
    vstab_frame f;
    std::memset(&f, 0, sizeof(f));
    const int rc = src->peek(src->user, &f);
    if (rc == VSTAB_EOF) return fail(VSTAB_EOF, "vstab_create: upstream has no frames");
    if (rc != 0) return fail(VSTAB_ERR_SOURCE, "vstab_create: upstream peek failed with " + std::to_string(rc));
    if (f.width <= 0 || f.height <= 0 || (f.width & 1) || (f.height & 1) || f.width > 32767 || f.height > 32767)
        return fail(VSTAB_ERR_INVALID, "vstab_create: frame size must be even and <= 32767");
    H->w = f.width, H->h = f.height;
    {
        // Epochs in turn (vstab_handle::epoch_overlap) pay where the tracker's dependent chain is longer than a frame's warp: 1080p + 10 - 13 %
        // (44.3 -> 49.5 k frames/s); at 4K the warp sets the period and a second tracker chain beside it costs 0.5 %.  Bit-identical either way.
        // VSTAB_EPOCH_OVERLAP=1 / 0 (development) overrides the size rule.
        const char *const eo = getenv("VSTAB_EPOCH_OVERLAP");  // (read here, on the caller's thread, like the other launch-shape switches)
        const int eo_forced = eo ? (atoi(eo) != 0 ? 1 : 0) : -1;
        const bool small_frame = (long)H->w * H->h <= 1920L * 1200;
        H->epoch_overlap = H->dstream && cfg->tracking && (eo_forced < 0 ? small_frame : eo_forced == 1);
        if (H->epoch_overlap) VSTAB_HIP_TRY(hipEventCreateWithFlags(&H->epoch_tail, hipEventDisableTiming));
    }
    if (cfg->lens_mode == 0) {
        if (!preset_camera(cfg->preset, H->w, H->h, H->Kin)) return fail(VSTAB_ERR_INVALID, "vstab_create: unknown preset");
        output_camera(H->Kin, H->w, H->h, cfg->scale, cfg->crop_borders != 0, cfg->zoom, H->Kout, H->ow, H->oh);
        if (cfg->map_precision == VSTAB_MAP_PRECISION_OPENCL) H->map_mode = VSTAB_MAP_CREATEMAP_CL_OPENCL;
    } else {
        // the libdewobble filter options as the CLI sets them (render.ts:669-683)
        H->ow = cfg->out_width > 0 ? cfg->out_width : H->w, H->oh = cfg->out_height > 0 ? cfg->out_height : H->h;
        const double out_dfov = cfg->out_dfov > 0 ? cfg->out_dfov : cfg->in_dfov;
        if (!lens_camera(cfg->in_projection, cfg->in_dfov, H->w, H->h, -1, -1, H->Kin) ||
            !lens_camera(cfg->out_projection, out_dfov, H->ow, H->oh, cfg->out_cx, cfg->out_cy, H->Kout))
            return fail(VSTAB_ERR_INVALID, "vstab_create: bad lens description (projection / field of view / size)");
        H->in_fish = cfg->in_projection == VSTAB_PROJ_FISH;
        const bool out_fish = cfg->out_projection == VSTAB_PROJ_FISH;
        H->map_mode = H->in_fish ? (out_fish ? VSTAB_MAP_FISH_TO_FISH : VSTAB_MAP_FISH_TO_RECT)
                                 : (out_fish ? VSTAB_MAP_RECT_TO_FISH : VSTAB_MAP_RECT_TO_RECT);
    }
    if (H->ow <= 0 || H->oh <= 0 || H->ow > 32767 || H->oh > 32767) return fail(VSTAB_ERR_INVALID, "vstab_create: output size out of range");
    if (cfg->smoother == VSTAB_SMOOTHER_SG) H->sg.reset(new RotationFilterSG(cfg->smooth_radius));
    if (cfg->read_ahead > 0) H->prefetch_depth = cfg->read_ahead;  // vstab_config.read_ahead: the caller's latency / throughput choice
    else if (const char *e = getenv("VSTAB_PREFETCH")) H->prefetch_depth = std::max(1, std::min(atoi(e), PREFETCH_MAX));  // (development sweeps)
    if (const char *e = getenv("VSTAB_LK_SEG_TARGET")) H->seg_target = std::max(1, std::min(atoi(e), H->seg_max));
    // queue (r + 1) + the frame whose estimate runs + the one whose results are read + the one in flight + first/last gray + 1 spare
    // + the read-ahead + the slots that wait for a shared warp event
    H->slots.resize((size_t)cfg->smooth_radius + 6 + H->prefetch_depth + vstab_handle::WARP_EVENT_STRIDE);
    for (auto &s : H->slots) {
        VSTAB_HIP_TRY(hipEventCreateWithFlags(&s.ingested, hipEventDisableTiming));
        VSTAB_HIP_TRY(hipEventCreateWithFlags(&s.copied, hipEventDisableTiming));
    }
    // a frame stays in the pipeline from its pull until its warp: read-ahead + look-ahead queue + the frames in between
    H->borrow_hold = getenv("VSTAB_ALWAYS_COPY") ? (1 << 30) + 1 : cfg->smooth_radius + H->prefetch_depth + 6;
    if (cfg->tracking) {
        VSTAB_TRY(H->tracker.init(H->w, H->h));
        VSTAB_TRY(H->detector.init(H->w, H->h));
    }
    *out = H.release();
    return VSTAB_OK;
}

vstab_status vstab_get_output_info(const vstab_handle *h, int *width, int *height, double K_in[9], double K_out[9]) {
    if (!h) return fail(VSTAB_ERR_INVALID, "null handle");
    if (width) *width = h->ow;
    if (height) *height = h->oh;
    if (K_in) std::memcpy(K_in, h->Kin.m, sizeof(h->Kin.m));
    if (K_out) std::memcpy(K_out, h->Kout.m, sizeof(h->Kout.m));
    return VSTAB_OK;
}

}  // extern "C"

// vstab_set_input_calibration / _ex: `resamplers`: whether a CUBIC or LANCZOS4 handle and a border mode are served (vstab_warp_nv12_dist_ex)
static vstab_status set_input_calibration(vstab_handle *h, const double K[9], const double D[4], const char *fn, bool resamplers) {
    const std::string n = std::string(fn) + ": ";
    if (!h || !D) return fail(VSTAB_ERR_INVALID, n + "null argument");
    const vstab_config &c = h->cfg;
    if (c.lens_mode != 1) return fail(VSTAB_ERR_INVALID, n + "a calibration belongs to lens_mode 1 (the preset path derives its output camera from the input's)");
    if (c.in_projection != VSTAB_PROJ_FISH) return fail(VSTAB_ERR_INVALID, n + "distortion belongs to a fisheye input (in_projection VSTAB_PROJ_FISH)");
    // (lens_mode 1 is INTER_LINEAR: vstab_create)
    if (!resamplers && c.resample != VSTAB_RESAMPLE_DEFAULT)
        return fail(VSTAB_ERR_INVALID, n + "the distorted-lens warp resamples with VSTAB_RESAMPLE_DEFAULT, this handle with " + resample_name(c.resample));
    if (c.pixel_depth == 10) return fail(VSTAB_ERR_INVALID, n + "the distorted-lens warp takes 8-bit pixels, this is a pixel_depth 10 handle");
    if (!resamplers && h->border_mode != VSTAB_BORDER_CONSTANT)
        return fail(VSTAB_ERR_INVALID, n + "the distorted-lens warp has the constant border, this handle has another border mode set (vstab_set_border_mode)");
    if (h->pulled) return fail(VSTAB_ERR_INVALID, n + "the calibration must be set before the first pull");
    if (h->colour()) return fail(VSTAB_ERR_UNSUPPORTED, n + "a colour spec is set (vstab_set_colour), and the distorted-lens warp converts with cvtColor's arithmetic");
    if (K && !(std::isfinite(K[0]) && std::isfinite(K[4]) && std::isfinite(K[2]) && std::isfinite(K[5]) && K[0] > 0 && K[4] > 0 && K[1] == 0 && K[3] == 0 &&
               K[6] == 0 && K[7] == 0 && K[8] == 1))
        return fail(VSTAB_ERR_INVALID, n + "K must be a camera matrix with fx, fy > 0, zero skew and last row 0 0 1");
    VSTAB_TRY(check_distortion(fn, D));
    if (K) std::memcpy(h->Kin.m, K, sizeof(h->Kin.m));
    for (int i = 0; i < 4; i++) h->dist[i] = D[i], h->dist32[i] = (float)D[i];
    h->calibrated = true, h->calibrated_borders = resamplers;
    return VSTAB_OK;
}

extern "C" {

vstab_status vstab_set_input_pinhole(vstab_handle *h, const double K[9], const double D[5]) {
    const std::string n = "vstab_set_input_pinhole: ";
    if (!h || !D) return fail(VSTAB_ERR_INVALID, n + "null argument");
    const vstab_config &c = h->cfg;
    if (c.lens_mode != 1) return fail(VSTAB_ERR_INVALID, n + "a calibration belongs to lens_mode 1 (the preset path derives its output camera from the input's)");
    if (c.in_projection != VSTAB_PROJ_RECT) return fail(VSTAB_ERR_INVALID, n + "pinhole distortion belongs to a rectilinear input (in_projection VSTAB_PROJ_RECT)");
    if (c.pixel_depth == 10) return fail(VSTAB_ERR_INVALID, n + "the pinhole-lens warp takes 8-bit pixels, this is a pixel_depth 10 handle");
    if (c.interpolation == 0 && c.resample == VSTAB_RESAMPLE_DEFAULT)
        return fail(VSTAB_ERR_INVALID, n + "the pinhole-lens warp resamples with INTER_LINEAR, INTER_CUBIC or INTER_LANCZOS4, this handle with INTER_NEAREST");
    if (h->pulled) return fail(VSTAB_ERR_INVALID, n + "the calibration must be set before the first pull");
    if (h->colour()) return fail(VSTAB_ERR_UNSUPPORTED, n + "a colour spec is set (vstab_set_colour), and the pinhole-lens warp converts with cvtColor's arithmetic");
    if (K && !(std::isfinite(K[0]) && std::isfinite(K[4]) && std::isfinite(K[2]) && std::isfinite(K[5]) && K[0] > 0 && K[4] > 0 && K[1] == 0 && K[3] == 0 &&
               K[6] == 0 && K[7] == 0 && K[8] == 1))
        return fail(VSTAB_ERR_INVALID, n + "K must be a camera matrix with fx, fy > 0, zero skew and last row 0 0 1");
    VSTAB_TRY(check_pinhole_distortion("vstab_set_input_pinhole", D));
    if (K) std::memcpy(h->Kin.m, K, sizeof(h->Kin.m));
    for (int i = 0; i < 5; i++) h->pdist[i] = D[i], h->pdist32[i] = (float)D[i];
    h->pinhole = true;
    return VSTAB_OK;
}

vstab_status vstab_set_input_calibration(vstab_handle *h, const double K[9], const double D[4]) {
    return set_input_calibration(h, K, D, "vstab_set_input_calibration", false);
}

// The handle's detection mask: the Detector keeps a copy and every detection of the handle reads it (seed_corners, track_frame's detection on
// demand, Detector::spec_launch).  Before the first pull nothing is in flight, so no stream has to be ordered behind the copy.
vstab_status vstab_set_detection_mask(vstab_handle *h, const void *mask, size_t pitch_mask, int mem) {
    const std::string n = "vstab_set_detection_mask: ";
    if (!h) return fail(VSTAB_ERR_INVALID, n + "null handle");
    if (!h->cfg.tracking) return fail(VSTAB_ERR_INVALID, n + "no detector runs on this handle (tracking = 0)");
    if (h->pulled) return fail(VSTAB_ERR_INVALID, n + "the mask must be set before the first pull");
    if (mask && pitch_mask < (size_t)h->w) return fail(VSTAB_ERR_INVALID, n + "the mask's pitch is smaller than the frame's width");
    if (mask && mem != VSTAB_MEM_DEVICE && mem != VSTAB_MEM_HOST) return fail(VSTAB_ERR_INVALID, n + "mem must be VSTAB_MEM_DEVICE (0) or VSTAB_MEM_HOST (1)");
    return h->detector.copy_mask(mask, pitch_mask, mem == VSTAB_MEM_HOST);
}

// The handle's corner response: read by every detection of the handle, as the mask is (Detector::set_response).
vstab_status vstab_set_corner_response(vstab_handle *h, int response, double k) {
    const std::string n = "vstab_set_corner_response: ";
    if (!h) return fail(VSTAB_ERR_INVALID, n + "null handle");
    if (!h->cfg.tracking) return fail(VSTAB_ERR_INVALID, n + "no detector runs on this handle (tracking = 0)");
    if (h->pulled) return fail(VSTAB_ERR_INVALID, n + "the response must be set before the first pull");
    if (response != VSTAB_CORNER_MIN_EIGENVAL && response != VSTAB_CORNER_HARRIS)
        return fail(VSTAB_ERR_INVALID, n + "response must be VSTAB_CORNER_MIN_EIGENVAL (0) or VSTAB_CORNER_HARRIS (1)");
    DetectSpec d;
    VSTAB_TRY(check_detect_spec("vstab_set_corner_response", nullptr, 0, response == VSTAB_CORNER_HARRIS, k, h->w, h->h, d));
    h->detector.set_response(d.harris, d.kf);
    return VSTAB_OK;
}

// The handle's corner block size (vstab.h, "Corner block size"): read by every detection of the handle, as the response is (Detector::set_block).
vstab_status vstab_set_corner_block(vstab_handle *h, int block_size) {
    const std::string n = "vstab_set_corner_block: ";
    if (!h) return fail(VSTAB_ERR_INVALID, n + "null handle");
    if (!h->cfg.tracking) return fail(VSTAB_ERR_INVALID, n + "no detector runs on this handle (tracking = 0)");
    if (h->pulled) return fail(VSTAB_ERR_INVALID, n + "the block size must be set before the first pull");
    VSTAB_TRY(check_corner_block("vstab_set_corner_block", block_size));
    h->detector.set_block(block_size);
    return VSTAB_OK;
}

// The handle's corner gradient size (vstab.h, "Corner gradient size"): read by every detection of the handle, as the block size is (Detector::set_gradient).
vstab_status vstab_set_corner_gradient(vstab_handle *h, int gradient_size) {
    const std::string n = "vstab_set_corner_gradient: ";
    if (!h) return fail(VSTAB_ERR_INVALID, n + "null handle");
    if (!h->cfg.tracking) return fail(VSTAB_ERR_INVALID, n + "no detector runs on this handle (tracking = 0)");
    if (h->pulled) return fail(VSTAB_ERR_INVALID, n + "the gradient size must be set before the first pull");
    VSTAB_TRY(check_corner_gradient("vstab_set_corner_gradient", gradient_size));
    h->detector.set_gradient(gradient_size);
    return VSTAB_OK;
}

// The handle's tracker options: read by every tracker launch of the handle, and the pyramids are capped to max_level + 1 levels
// (Tracker::set_options).  Before the first pull no pyramid has been built and no launch is in flight.
vstab_status vstab_set_tracker_options(vstab_handle *h, int max_level, int max_iter, double eps, double min_eig_threshold) {
    const std::string n = "vstab_set_tracker_options: ";
    if (!h) return fail(VSTAB_ERR_INVALID, n + "null handle");
    if (!h->cfg.tracking) return fail(VSTAB_ERR_INVALID, n + "no tracker runs on this handle (tracking = 0)");
    if (h->pulled) return fail(VSTAB_ERR_INVALID, n + "the options must be set before the first pull");
    LkOptions opt;
    VSTAB_TRY(check_lk_options("vstab_set_tracker_options", max_level, max_iter, eps, min_eig_threshold, opt));
    h->tracker.set_options(opt);
    return VSTAB_OK;
}

// The handle's tracker window (vstab.h, "Tracker window"): read by every tracker launch of the handle -- segments, chained launches and
// their fetch-ahead -- and the pyramids get the depth that window asks for (Tracker::set_window).
vstab_status vstab_set_tracker_window(vstab_handle *h, int win_size) {
    const std::string n = "vstab_set_tracker_window: ";
    if (!h) return fail(VSTAB_ERR_INVALID, n + "null handle");
    if (!h->cfg.tracking) return fail(VSTAB_ERR_INVALID, n + "no tracker runs on this handle (tracking = 0)");
    if (h->pulled) return fail(VSTAB_ERR_INVALID, n + "the window must be set before the first pull");
    if (!lk_window_offered(win_size)) return fail(VSTAB_ERR_INVALID, n + "win_size is 15, 21 or 31");
    return h->tracker.set_window(win_size);
}

vstab_status vstab_set_input_calibration_ex(vstab_handle *h, const double K[9], const double D[4]) {
    return set_input_calibration(h, K, D, "vstab_set_input_calibration_ex", true);
}

// test hook (not part of include/vstab.h): how many of the handle's warps read the quantised map written for an earlier frame
__attribute__((visibility("default"))) long vstabx_warps_from_cache(const vstab_handle *h) { return h ? h->warps_from_cache : -1; }

vstab_status vstab_enable_profiling(vstab_handle *h, int enable) {
    if (!h) return fail(VSTAB_ERR_INVALID, "null handle");
    h->profiling = enable < 0 ? 0 : enable > 2 ? 2 : enable;
    return VSTAB_OK;
}

vstab_status vstab_get_profile(vstab_handle *h, vstab_profile *out) {
    if (!h || !out) return fail(VSTAB_ERR_INVALID, "vstab_get_profile: null argument");
    h->fold_pending();
    h->prof.dmabuf_imports = h->dmabufs.imports, h->prof.dmabuf_evictions = h->dmabufs.evictions, h->prof.dmabuf_cached = (long)h->dmabufs.size();
    h->prof.corner_selections_by_caller = h->detector.selections_by_caller(), h->prof.corner_selections_by_helper = h->detector.selections_by_helper();
    h->prof.epochs_in_turn = h->epochs_on_second_stream;
    *out = h->prof;
    return VSTAB_OK;
}

void vstab_destroy(vstab_handle *h) {
    if (!h) return;
    if (g_ht.on) {
        for (int i = 0; i < HostTimers::N; i++)
            if (g_ht.calls[i]) std::fprintf(stderr, "host %-18s %8ld calls  %8.2f us/call\n", HostTimers::name(i), g_ht.calls[i], g_ht.ms[i] / g_ht.calls[i] * 1e3);
        g_ht = HostTimers();
    }
    h->fold_pending();
    h->tracker.report_clock();
    if (debug_spec())
        std::fprintf(stderr, "frames used in place %ld, copied into the ring %ld; warps from the cached map %ld\n", h->frames_borrowed, h->frames_copied,
                     h->warps_from_cache);
    if (debug_spec())
        std::fprintf(stderr, "tracker launches: %ld segments covering %ld frames (%ld of them dropped); frames taken from a launch enqueued ahead %ld, "
                             "replaced on demand %ld, of %ld; key frames pre-launched %ld of %ld\n",
                     h->segs_launched, h->seg_frames_launched, h->seg_frames_dropped, h->chained_adopted, h->chained_discarded, h->frame_index,
                     h->key_prelaunched, h->prof.key_frames);
    if (h->estimate_posted) {
        Mat3 r;
        (void)h->worker.join(r);
    }
    h->fold_pending();  // drains the streams
    delete h;           // ~vstab_handle releases the events and the internal streams
}

int vstab_frame_log_count(const vstab_handle *h) { return h ? (int)(h->log_base + (long)h->log.size()) : 0; }

vstab_status vstab_get_frame_log(const vstab_handle *h, int index, vstab_frame_log *out) {
    if (!h || !out || index < h->log_base || index >= h->log_base + (long)h->log.size())
        return fail(VSTAB_ERR_INVALID, "vstab_get_frame_log: bad index (only the most recent 65536 entries are kept)");
    *out = h->log[(size_t)(index - h->log_base)];
    return VSTAB_OK;
}

vstab_status vstab_get_warp_rotation(const vstab_handle *h, int index, double R[9]) {
    if (!h || !R || index < h->warp_log_base || index >= h->warp_log_base + (long)h->warp_log.size())
        return fail(VSTAB_ERR_INVALID, "vstab_get_warp_rotation: bad index (only the most recent 65536 entries are kept)");
    std::memcpy(R, h->warp_log[(size_t)(index - h->warp_log_base)].m, sizeof(double) * 9);
    return VSTAB_OK;
}

}  // extern "C"
