// vstab_testhooks.cpp -- the vstabx_* test hooks.
#include <algorithm>

#include "vstab_detect_host.hpp"
#include "vstab_hostlogic.hpp"
#include "vstab_pipeline.hpp"
#include "vstab_track_host.hpp"
#include "vstab_warp_bands.hpp"
#include "vstab_warp_request.hpp"

using namespace vstab;

// ---------------------------------------------------------------------------------------------------------------------------------
// Test hooks (vstabx_*: not part of the ABI of include/vstab.h, no device needed): the CPU suite -- and its sanitizer build -- drive
// the host-side bookkeeping of vstab_hostlogic.hpp with hand-made buffers (tests/test_hostlogic_cpu.py).
// ---------------------------------------------------------------------------------------------------------------------------------
extern "C" {
// Decode n hand-made tracker records as Tracker::track_wait does.  Returns the LkParse code; *n_out entries in xy / status; *next =
// the first record that was not ready (or n).
__attribute__((visibility("default"))) int vstabx_parse_records(const uint32_t *rec, int n, uint32_t seq, int expect_n, float *xy, unsigned char *status,
                                                                 int *n_out, int *next) {
    std::vector<float> pts;
    std::vector<uint8_t> st;
    int nx = 0;
    const LkParse r = lk_parse_records(rec, 0, n, seq, (size_t)expect_n, pts, st, &nx);
    for (size_t i = 0; i < st.size(); i++) xy[2 * i] = pts[2 * i], xy[2 * i + 1] = pts[2 * i + 1], status[i] = st[i];
    *n_out = (int)st.size(), *next = nx;
    return (int)r;
}
// Run a sequence of n lookups (object ids = inodes, all of one size unless sizes is given) through a DmaBufCache with fake import /
// destroy functions.  counts = {imports, evictions, mapped now, destroys seen, largest number mapped at once}; bases[i] = the base the
// i-th lookup returned (id * 4096 for the fake import: a stale mapping would show); fail_id: the import of this id fails (-1: none).
__attribute__((visibility("default"))) int vstabx_dmabuf_cache_sim(const unsigned long long *ids, const size_t *sizes, int n, int cap, long window,
                                                                    long long fail_id, long *counts, unsigned long long *bases) {
    DmaBufCache<unsigned long long> cache;
    cache.cap = cap;
    long destroys = 0, peak = 0;
    std::vector<unsigned long long> live;
    int failures = 0;
    for (int i = 0; i < n; i++) {
        uint8_t *base = nullptr;
        const unsigned long long id = ids[i];
        const bool ok = cache.lookup(id, sizes ? sizes[i] : 4096, window,
                                     [&](unsigned long long &h, uint8_t *&b) {
                                         if ((long long)id == fail_id) return false;
                                         h = id, b = reinterpret_cast<uint8_t *>(static_cast<uintptr_t>(id * 4096));
                                         live.push_back(id);
                                         return true;
                                     },
                                     [&](unsigned long long &h) {
                                         destroys++;
                                         for (size_t k = 0; k < live.size(); k++)
                                             if (live[k] == h) {
                                                 live.erase(live.begin() + (long)k);
                                                 break;
                                             }
                                     },
                                     base);
        failures += !ok;
        bases[i] = ok ? static_cast<unsigned long long>(reinterpret_cast<uintptr_t>(base)) : ~0ull;
        peak = std::max<long>(peak, (long)cache.size());
    }
    counts[0] = cache.imports, counts[1] = cache.evictions, counts[2] = (long)cache.size(), counts[3] = destroys, counts[4] = peak;
    cache.clear([&](unsigned long long &) { destroys++; });
    counts[5] = destroys;
    return failures;
}

// THE FIRST HOOK THAT NEEDS A DEVICE (tests/test_lk_segments_gpu.py; its argument checks run without one: tests/test_lk_segments_cpu.py).
// Tracks n points through K = sum(seg) frame pairs of the K + 1 device luma frames (frames[i], pitches[i]; w x h) the way the pipeline
// does: every frame's pyramid by Tracker::build_pyramid, then one launch per entry of seg (1 .. LK_SEG_MAX pairs each) on `stream` --
// the first by Tracker::track_launch from pts, every later one by Tracker::track_launch_chained behind the one before it (non-zero
// increasing tags, zeroed device records, host records in mapped memory).
//   uv, uv_pitches, rings (all NULL, or K + 1 entries each): level 1 of frame i is written by launch_pack_pyr together with the copy
//       of (frames[i], uv[i]) into the device buffer rings[i] (w * h * 3 / 2 bytes), and the frame is tracked from the ring's luma --
//       the pipeline's ingest of a frame upstream recycles.  Only where pack_pyr_ok holds for every frame.
//   bad_parent: the launch of this index (1 .. n_seg - 1; -1 = none) is handed a parent tag that is not its parent's.
//   host_rec, dev_rec: K * n records of 4 uint32 each, pair-major -- what the kernel left in the mapped and in the device copy.
//   pyr_out (optional): levels 1 .. of every frame's pyramid, dense, frame after frame.
//   win (vstabx_lk_segments_win; vstabx_lk_segments: 21): the tracker's window, 15, 21 or 31 -- the pyramids get its depth, every launch runs with it.
// Bad arguments are refused with VSTAB_ERR_INVALID before anything touches the device; fn names the hook in the refusals.
static int lk_segments_hook(const std::string &fn, const void *const *frames, const size_t *pitches, int w, int h, const float *pts, int n, const int *seg, int n_seg,
                            const void *const *uv, const size_t *uv_pitches, void *const *rings, int bad_parent, uint32_t *host_rec, uint32_t *dev_rec,
                            uint8_t *pyr_out, int win, void *stream) {
    if (!frames || !pitches || !pts || !seg || !host_rec || !dev_rec || w <= 0 || h <= 0 || n <= 0 || n_seg <= 0 || n_seg > Tracker::REC_BUFS)
        return fail(VSTAB_ERR_INVALID, fn + ": bad argument");
    if (!lk_window_offered(win)) return fail(VSTAB_ERR_INVALID, fn + ": win_size is 15, 21 or 31");
    int K = 0;
    for (int s = 0; s < n_seg; s++) {
        if (seg[s] < 1 || seg[s] > LK_SEG_MAX) return fail(VSTAB_ERR_INVALID, fn + ": a launch covers 1 .. LK_SEG_MAX frame pairs");
        K += seg[s];
    }
    // (the record buffers rotate through REC_BUFS: every pair of the call keeps its own)
    if (K > Tracker::REC_BUFS) return fail(VSTAB_ERR_INVALID, fn + ": more frame pairs than record buffers");
    if (bad_parent != -1 && (bad_parent < 1 || bad_parent >= n_seg)) return fail(VSTAB_ERR_INVALID, fn + ": bad_parent is not a chained launch");
    const bool pack = uv || uv_pitches || rings;
    if (pack && (!uv || !uv_pitches || !rings)) return fail(VSTAB_ERR_INVALID, fn + ": uv, uv_pitches and rings go together");
    if (pack && lk_levels(w, h, win) < 2) return fail(VSTAB_ERR_INVALID, fn + ": a one-level pyramid has no level 1 to pack");
    for (int i = 0; i <= K; i++) {
        if (!frames[i] || pitches[i] < (size_t)w || pitches[i] >= (1u << 24) || (uint64_t)pitches[i] * (uint64_t)h >= (1ull << 32))
            return fail(VSTAB_ERR_INVALID, fn + ": bad frame");
        // (level 1 is the Tracker's: a hipMalloc'd buffer, pitch (w + 1) / 2 -- the ring stands in for its base, which is aligned)
        if (pack && (!uv[i] || !rings[i] || !pack_pyr_ok(frames[i], pitches[i], uv[i], uv_pitches[i], w, h, rings[i], rings[i], (size_t)((w + 1) / 2))))
            return fail(VSTAB_ERR_INVALID, fn + ": planes not aligned for the fused copy");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    Tracker t;
    LkOptions opt;
    opt.win = win;
    VSTAB_TRY(t.init(w, h, opt));
    VSTAB_TRY(t.reserve_slots(n));
    const int levels = t.levels();
    size_t pyr_bytes = 0;
    for (int l = 1; l < levels; l++) pyr_bytes += (size_t)t.level_w(l) * t.level_h(l);
    // frame i -> pyramid set i % PYR_SETS: a launch spans at most LK_SEG_MAX + 1 < PYR_SETS frames, and a set is rebuilt only behind
    // every launch that reads it (one stream)
    std::vector<LkPyramid> pyr(K + 1);
    int built = -1;
    auto build = [&](int i) -> vstab_status {
        const int s = i % PYR_SETS;
        const uint8_t *y = static_cast<const uint8_t *>(frames[i]);
        size_t pitch = pitches[i];
        if (pack) {
            uint8_t *ring = static_cast<uint8_t *>(rings[i]);
            VSTAB_TRY(launch_pack_pyr(y, pitch, static_cast<const uint8_t *>(uv[i]), uv_pitches[i], w, h, ring, t.level1(s), t.level1_pitch(), st));
            y = ring, pitch = (size_t)w;
        }
        VSTAB_TRY(t.build_pyramid(s, y, pitch, st, nullptr, nullptr, pack));
        pyr[i] = t.pyramid(s, y, pitch);
        if (pyr_out) {
            uint8_t *o = pyr_out + pyr_bytes * i;
            for (int l = 1; l < levels; l++) {
                const size_t lw = (size_t)t.level_w(l), lh = (size_t)t.level_h(l);
                VSTAB_HIP_TRY(hipMemcpyAsync(o, pyr[i].img[l], lw * lh, hipMemcpyDeviceToHost, st));
                o += lw * lh;
            }
        }
        built = i;
        return VSTAB_OK;
    };
    std::vector<Tracker::Launch> launches(n_seg);
    std::vector<float> start(pts, pts + 2 * (size_t)n);
    int first = 0;
    for (int s = 0; s < n_seg; s++) {
        for (int i = built + 1; i <= first + seg[s]; i++) VSTAB_TRY(build(i));
        if (s == 0) {
            VSTAB_TRY(t.track_launch(&pyr[first], seg[s], start, st, false, launches[s]));
        } else {
            Tracker::Launch parent = launches[s - 1];
            if (s == bad_parent) parent.seq[parent.n_frames - 1] ^= 0x40u;  // a tag the parent never wrote (nor any launch of this call)
            VSTAB_TRY(t.track_launch_chained(&pyr[first], seg[s], parent, st, launches[s]));
        }
        first += seg[s];
    }
    VSTAB_HIP_TRY(hipStreamSynchronize(st));
    int k = 0;
    for (int s = 0; s < n_seg; s++)
        for (int i = 0; i < seg[s]; i++, k++) {
            std::memcpy(host_rec + (size_t)k * n * 4, t.host_records(launches[s], i), (size_t)n * 16);
            VSTAB_HIP_TRY(hipMemcpy(dev_rec + (size_t)k * n * 4, t.dev_records(launches[s], i), (size_t)n * 16, hipMemcpyDeviceToHost));
        }
    return VSTAB_OK;
}

__attribute__((visibility("default"))) int vstabx_lk_segments(const void *const *frames, const size_t *pitches, int w, int h, const float *pts, int n,
                                                               const int *seg, int n_seg, const void *const *uv, const size_t *uv_pitches,
                                                               void *const *rings, int bad_parent, uint32_t *host_rec, uint32_t *dev_rec,
                                                               uint8_t *pyr_out, void *stream) {
    return lk_segments_hook("vstabx_lk_segments", frames, pitches, w, h, pts, n, seg, n_seg, uv, uv_pitches, rings, bad_parent, host_rec, dev_rec, pyr_out, LK_WIN,
                            stream);
}
__attribute__((visibility("default"))) int vstabx_lk_segments_win(const void *const *frames, const size_t *pitches, int w, int h, const float *pts, int n,
                                                                   const int *seg, int n_seg, const void *const *uv, const size_t *uv_pitches,
                                                                   void *const *rings, int bad_parent, uint32_t *host_rec, uint32_t *dev_rec,
                                                                   uint8_t *pyr_out, int win, void *stream) {
    return lk_segments_hook("vstabx_lk_segments_win", frames, pitches, w, h, pts, n, seg, n_seg, uv, uv_pitches, rings, bad_parent, host_rec, dev_rec, pyr_out, win,
                            stream);
}

// the body of vstabx_corners_fused and vstabx_corners_fused_mask (both below); fn names the hook in the refusals, masked says whether `mask` is looked at
// harris: the Harris response with k, checked last; max_out (optional) receives the frame maximum the kernels published, as int32 float bits
static int corners_fused_hook(const std::string &fn, const void *gray, size_t pitch, int w, int h, const void *mask, size_t pitch_mask, bool masked, double quality,
                              unsigned int cap, unsigned int canary, unsigned long long *keys_out, unsigned int *counts_out, unsigned int *tile_counts,
                              void *stream, bool harris = false, double k = 0.0, int *max_out = nullptr, int block = 3, int gradient = 3) {
    if (!gray || !keys_out || !counts_out || !tile_counts || (masked && !mask)) return fail(VSTAB_ERR_INVALID, fn + ": bad argument");
    if (w < 3 || h < 3 || pitch < (size_t)w) return fail(VSTAB_ERR_INVALID, fn + ": an image is at least 3 x 3 and its pitch at least its width");
    if ((uint64_t)pitch * (uint64_t)h >= (1ull << 32) || (uint64_t)w * (uint64_t)h >= (1ull << 31))
        return fail(VSTAB_ERR_INVALID, fn + ": planes of 4 GiB or more and images of 2^31 pixels or more are not supported");
    if (!(quality > 0.0) || !(quality <= 1.0)) return fail(VSTAB_ERR_INVALID, fn + ": quality lies in (0, 1]");
    if (cap < 1 || cap > (1u << 24)) return fail(VSTAB_ERR_INVALID, fn + ": cap is 1 .. 2^24 keys");
    if (canary < 1 || canary > (1u << 16)) return fail(VSTAB_ERR_INVALID, fn + ": canary is 1 .. 2^16 keys");
    DetectSpec spec;
    VSTAB_TRY(check_detect_spec(fn, masked ? mask : nullptr, pitch_mask, harris, k, w, h, spec, block, gradient));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const CornersFusedScratch lay(w, h);  // the layout launch_corners_fused uses: the survivor counts are read back from it below
    const size_t scratch_bytes = lay.bytes;
    const size_t n_keys = (size_t)cap + canary;
    DevBuf scratch, keys, small;
    VSTAB_TRY(scratch.ensure(scratch_bytes));
    VSTAB_TRY(keys.ensure(n_keys * sizeof(unsigned long long)));
    VSTAB_TRY(small.ensure(256));
    // (under a mask the scratch starts out as garbage, as a Detector's does: a tile that returns early has to WRITE its count of 0)
    VSTAB_HIP_TRY(hipMemsetAsync(scratch.p, masked ? 0xA5 : 0, scratch_bytes, st));
    VSTAB_HIP_TRY(hipMemsetAsync(keys.p, 0xA5, n_keys * sizeof(unsigned long long), st));
    DetectorWords *words = small.as<DetectorWords>();
    VSTAB_TRY(launch_corners_fused(static_cast<const uint8_t *>(gray), pitch, w, h, quality, scratch.p, keys.as<unsigned long long>(), cap, words, st, spec));
    VSTAB_HIP_TRY(hipMemcpyAsync(keys_out, keys.p, n_keys * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    VSTAB_HIP_TRY(hipMemcpyAsync(counts_out, &words->kept, 2 * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    if (max_out) VSTAB_HIP_TRY(hipMemcpyAsync(max_out, &words->max, sizeof(int), hipMemcpyDeviceToHost, st));
    VSTAB_HIP_TRY(hipMemcpyAsync(tile_counts, scratch.as<uint8_t>() + lay.counts_off, (size_t)lay.tiles * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    VSTAB_HIP_TRY(hipStreamSynchronize(st));
    if (max_out) *max_out = (int)((unsigned int)*max_out ^ 0x80000000u);  // the kernels keep it biased (unsigned order); 0 there = nothing published = INT_MIN here
    return VSTAB_OK;
}
// THE RAW OUTPUT OF THE ONE-PASS DETECTOR (tests/test_corner_paths_gpu.py; its argument checks run without a device:
// tests/test_corner_tiles_cpu.py).  Runs launch_corners_fused (k_corners_fused, then k_filter_keys) on the w x h device luma plane `gray`
// with a key buffer of exactly `cap` keys followed by `canary` keys the kernels must not touch; the whole buffer is filled with the byte
// 0xA5 first.
//   keys_out    cap + canary keys as the kernels left them: the first min(counts_out[0], cap) are keys (float bits << 32 | raster index),
//               unsorted; everything behind them still holds the fill
//   counts_out  {keys kept (may exceed cap), tiles that spilled}
//   tile_counts div_up(w, 64) * div_up(h, 31) survivor counts of k_corners_fused, tile rows first
// Bad arguments are refused with VSTAB_ERR_INVALID before anything touches the device.
__attribute__((visibility("default"))) int vstabx_corners_fused(const void *gray, size_t pitch, int w, int h, double quality, unsigned int cap, unsigned int canary,
                                                                 unsigned long long *keys_out, unsigned int *counts_out, unsigned int *tile_counts,
                                                                 void *stream) {
    return corners_fused_hook("vstabx_corners_fused", gray, pitch, w, h, nullptr, 0, false, quality, cap, canary, keys_out, counts_out, tile_counts, stream);
}
// vstabx_corners_fused under a detection mask (tests/test_detection_mask_gpu.py, tests/corner_def.py): k_corners_fused_masked, then
// k_filter_keys.  mask: a w x h device plane of bytes of pitch pitch_mask, not NULL.  The same outputs (the scratch is filled with the byte 0xA5 first, so
// the count of 0 a tile that returns early reports is one it wrote) and the same refusals under this hook's name, then the mask's: a pitch below w, a
// plane of 4 GiB or more.
__attribute__((visibility("default"))) int vstabx_corners_fused_mask(const void *gray, size_t pitch, int w, int h, const void *mask, size_t pitch_mask, double quality,
                                                                      unsigned int cap, unsigned int canary, unsigned long long *keys_out, unsigned int *counts_out,
                                                                      unsigned int *tile_counts, void *stream) {
    return corners_fused_hook("vstabx_corners_fused_mask", gray, pitch, w, h, mask, pitch_mask, true, quality, cap, canary, keys_out, counts_out, tile_counts, stream);
}
// vstabx_corners_fused / vstabx_corners_fused_mask with the Harris response (tests/test_harris_gpu.py, tests/corner_def.py):
// k_corners_fused_harris or, with a mask (optional here: NULL = none), k_corners_fused_harris_masked, then k_filter_keys.  The same outputs
// and refusals under this hook's name, then "k lies in [0, 0.25)"; max_bits_out (optional): the frame maximum the kernels published, the
// bits of a float read as int32 -- negative means "no response above zero", where the host reports no corner whatever the keys say.
__attribute__((visibility("default"))) int vstabx_corners_fused_harris(const void *gray, size_t pitch, int w, int h, const void *mask, size_t pitch_mask, double quality,
                                                                        double k, unsigned int cap, unsigned int canary, unsigned long long *keys_out,
                                                                        unsigned int *counts_out, unsigned int *tile_counts, int *max_bits_out, void *stream) {
    return corners_fused_hook("vstabx_corners_fused_harris", gray, pitch, w, h, mask, pitch_mask, mask != nullptr, quality, cap, canary, keys_out, counts_out,
                              tile_counts, stream, true, k, max_bits_out);
}
// vstabx_corners_fused_harris with the block size and the response as arguments (tests/test_corner_block_gpu.py, tests/corner_def.py):
// k_corners_fused_block<block> or, with block 3, the kernel vstabx_corners_fused* runs for this mask and response; then k_filter_keys.
// response: VSTAB_CORNER_MIN_EIGENVAL (k is not looked at) or VSTAB_CORNER_HARRIS.  The same outputs; the refusals under this hook's name:
// first "response is 0 or 1", then vstabx_corners_fused_harris', with "block_size is 3, 5 or 7" ahead of the mask's and k's.
__attribute__((visibility("default"))) int vstabx_corners_fused_block(const void *gray, size_t pitch, int w, int h, const void *mask, size_t pitch_mask, double quality,
                                                                       double k, int block, int response, unsigned int cap, unsigned int canary,
                                                                       unsigned long long *keys_out, unsigned int *counts_out, unsigned int *tile_counts,
                                                                       int *max_bits_out, void *stream) {
    if (response != VSTAB_CORNER_MIN_EIGENVAL && response != VSTAB_CORNER_HARRIS) return fail(VSTAB_ERR_INVALID, "vstabx_corners_fused_block: response is 0 or 1");
    return corners_fused_hook("vstabx_corners_fused_block", gray, pitch, w, h, mask, pitch_mask, mask != nullptr, quality, cap, canary, keys_out, counts_out, tile_counts,
                              stream, response == VSTAB_CORNER_HARRIS, k, max_bits_out, block);
}
// vstabx_corners_fused_block with the gradient size behind the block size (tests/test_corner_gradient_gpu.py, tests/corner_def.py):
// k_corners_fused_block<block, gradient> or, with both 3, the kernel vstabx_corners_fused* runs for this mask and response; then
// k_filter_keys.  The same outputs; the refusals of vstabx_corners_fused_block under this hook's name, with "gradient_size is 3, 5 or 7"
// directly behind the block's.
__attribute__((visibility("default"))) int vstabx_corners_fused_grad(const void *gray, size_t pitch, int w, int h, const void *mask, size_t pitch_mask, double quality,
                                                                      double k, int block, int gradient, int response, unsigned int cap, unsigned int canary,
                                                                      unsigned long long *keys_out, unsigned int *counts_out, unsigned int *tile_counts,
                                                                      int *max_bits_out, void *stream) {
    if (response != VSTAB_CORNER_MIN_EIGENVAL && response != VSTAB_CORNER_HARRIS) return fail(VSTAB_ERR_INVALID, "vstabx_corners_fused_grad: response is 0 or 1");
    return corners_fused_hook("vstabx_corners_fused_grad", gray, pitch, w, h, mask, pitch_mask, mask != nullptr, quality, cap, canary, keys_out, counts_out, tile_counts,
                              stream, response == VSTAB_CORNER_HARRIS, k, max_bits_out, block, gradient);
}

// The cost-weighted XCD bands of the fused warp (vstab_warp_bands.hpp; tests/test_band_schedule_cpu.py), no device needed.
// weighted_bands for a dw x dh output: out = {band_y[9], split_y[8], tiles_x, grid}.  cost NULL: tile_schedule's even bands.
__attribute__((visibility("default"))) int vstabx_weighted_bands(int dw, int dh, int rwb, int lds_kb, double tail_rounds, const uint32_t *cost, int n_cost,
                                                                  int *out) {
    if (!out || dw < 1 || dh < 1 || (rwb != 4 && rwb != 8) || lds_kb < 1 || !(tail_rounds >= 0.0) || n_cost < 0)
        return fail(VSTAB_ERR_INVALID, "vstabx_weighted_bands: bad argument");
    FusedArgs ta = {};
    ta.w.dw = dw, ta.w.dh = dh;
    const unsigned grid = cost ? weighted_bands(ta, rwb, lds_kb, tail_rounds, cost, n_cost) : tile_schedule(ta, rwb, lds_kb, tail_rounds);
    for (int k = 0; k < 9; k++) out[k] = ta.band_y[k];
    for (int k = 0; k < 8; k++) out[9 + k] = ta.split_y[k];
    out[17] = ta.tiles_x, out[18] = (int)grid;
    return VSTAB_OK;
}
// band_costs: the model's cost of every half-height tile row (64 x ts tiles); cost has div_up(dh, ts) entries.
__attribute__((visibility("default"))) int vstabx_band_costs(const float *params, int nan_behind, int sw, int sh, int dw, int dh, int ts, uint32_t *cost, int n_cost) {
    if (!params || !cost || sw < 1 || sh < 1 || dw < 1 || dh < 1 || (ts != 8 && ts != 16) || n_cost != (int)div_up((unsigned)dh, (unsigned)ts))
        return fail(VSTAB_ERR_INVALID, "vstabx_band_costs: bad argument");
    std::vector<uint32_t> c;
    band_costs(params, nan_behind != 0, sw, sh, dw, dh, ts, c);
    std::copy(c.begin(), c.end(), cost);
    return VSTAB_OK;
}
// n launches (17 parameters each) of one sw x sh -> dw x dh warp through a fresh BandCache: out = 19 integers per launch as
// vstabx_weighted_bands; counts = {hits, misses, entries}.
__attribute__((visibility("default"))) int vstabx_band_cache_run(const float *params, int n, int sw, int sh, int dw, int dh, int map_mode, int rwb, int lds_kb,
                                                                  double tail_rounds, int *out, long *counts) {
    if (!params || !out || !counts || n < 1 || sw < 1 || sh < 1 || dw < 1 || dh < 1 || (rwb != 4 && rwb != 8) || lds_kb < 1 || !(tail_rounds >= 0.0))
        return fail(VSTAB_ERR_INVALID, "vstabx_band_cache_run: bad argument");
    BandCache cache;
    for (int i = 0; i < n; i++) {
        FusedArgs ta = {};
        ta.w.sw = sw, ta.w.sh = sh, ta.w.dw = dw, ta.w.dh = dh;
        const unsigned grid = cache.schedule(ta, params + 17 * (size_t)i, map_mode, rwb, lds_kb, tail_rounds);
        int *o = out + 19 * (size_t)i;
        for (int k = 0; k < 9; k++) o[k] = ta.band_y[k];
        for (int k = 0; k < 8; k++) o[9 + k] = ta.split_y[k];
        o[17] = ta.tiles_x, o[18] = (int)grid;
    }
    counts[0] = cache.hits, counts[1] = cache.misses, counts[2] = (long)cache.entries.size();
    return VSTAB_OK;
}

// The routing of the 8-bit NV12 warps (warp_route, vstab_warp_request.hpp; tests/test_warp_routes_cpu.py), no device needed.  lens: 0 ideal,
// 1 fisheye coefficients, 2 pinhole coefficients, 3 pinhole coefficients all zero; border_entry: 0 the entry point has no border mode, 1 it
// exists for its border kernels, 2 the border mode is an option beside a resampler; rs, keep, qmap: 0 / 1.  out = {family (0: no route),
// argument block, kernel mode tag}.
__attribute__((visibility("default"))) int vstabx_warp_route(int map_mode, int lens, int rs, int resample, int border_entry, int border_mode, int out_format, int keep,
                                                              int qmap, int *out) {
    if (!out) return fail(VSTAB_ERR_INVALID, "vstabx_warp_route: bad argument");
    const WarpRoute r = warp_route(map_mode, lens, rs != 0, resample, border_entry, border_mode, out_format, keep != 0, qmap != 0);
    out[0] = r.family, out[1] = r.block, out[2] = r.mode;
    return VSTAB_OK;
}

// The host half of goodFeaturesToTrack alone, no device needed (select_corners, vstab_hostlogic.hpp; tests/test_select_corners_cpu.py): the n
// candidate keys (float bits << 32 | raster index) of a w x h image -> up to max_corners corners in xy (room for min(n, max_corners)
// pairs; max_corners <= 0: all of them), *count of them.  The keys are copied: select_corners sorts in place.
__attribute__((visibility("default"))) int vstabx_select_corners(const unsigned long long *keys, unsigned int n, int w, int h, int max_corners, double min_distance,
                                                                  float *xy, int *count) {
    if ((n > 0 && !keys) || !xy || !count || w < 1 || h < 1 || !(min_distance >= 0.0))  // (+inf is a distance: select_corners clamps its cell)
        return fail(VSTAB_ERR_INVALID, "vstabx_select_corners: bad argument");
    for (unsigned int i = 0; i < n; i++)  // (the grid is indexed by the pixel a key names)
        if ((keys[i] & 0xffffffffu) >= (uint64_t)w * (uint64_t)h) return fail(VSTAB_ERR_INVALID, "vstabx_select_corners: a key names a pixel outside the image");
    std::vector<unsigned long long> k(keys, keys + n);
    std::vector<float> out;
    select_corners(k.data(), n, w, h, max_corners, min_distance, out);
    std::copy(out.begin(), out.end(), xy);
    *count = (int)(out.size() / 2);
    return VSTAB_OK;
}

// The detector's bookkeeping of a handle (not in vstab_profile: the ABI layout stays): out = {speculative selections that found more
// candidates than Detector::SPEC_CAP (the key frame then detects synchronously), fused detections that overflowed the key buffer (the
// two-pass detector re-ran them), the key capacity now in force (0 before the first synchronous detection)}.
__attribute__((visibility("default"))) int vstabx_detector_counters(const vstab_handle *h, long *out) {
    if (!h || !out) return fail(VSTAB_ERR_INVALID, "vstabx_detector_counters: bad argument");
    out[0] = h->detector.spec_over_cap(), out[1] = h->detector.fused_overflows(), out[2] = (long)h->detector.key_capacity();
    return VSTAB_OK;
}

// The launch bookkeeping of a handle's tracker (track_frame; not in vstab_profile: the ABI layout stays): out = {tracker launches, the frame
// pairs they cover, the pairs of launches dropped before the host reached them, frames that took the launch enqueued ahead of them, frames
// whose launch enqueued ahead was replaced on demand, planned key frames whose tracker already ran on the speculated corners}.
__attribute__((visibility("default"))) int vstabx_tracker_counters(const vstab_handle *h, long *out) {
    if (!h || !out) return fail(VSTAB_ERR_INVALID, "vstabx_tracker_counters: bad argument");
    out[0] = h->segs_launched, out[1] = h->seg_frames_launched, out[2] = h->seg_frames_dropped;
    out[3] = h->chained_adopted, out[4] = h->chained_discarded, out[5] = h->key_prelaunched;
    return VSTAB_OK;
}

// k_pack_pyr ALONE, on planes the caller lays out (tests/test_pyr_paths_gpu.py, tests/pyr_paths.py): the copy of the NV12 frame (y, uv) into `ring`
// (w * h * 3 / 2 bytes, rows of pitch w) and pyrDown of its luma into dst (pitch dpitch) by launch_pack_pyr, as the pipeline's ingest of a frame upstream
// recycles does.  Returns -1 where pack_pyr_ok says no (nothing is launched: the pipeline takes its two-kernel path there), else the status of
// launch_pack_pyr.  No launch logic of its own.
__attribute__((visibility("default"))) int vstabx_pack_pyr(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int w, int h, void *ring, void *dst,
                                                            size_t dpitch, void *stream) {
    if (!pack_pyr_ok(y, pitch_y, uv, pitch_uv, w, h, ring, dst, dpitch)) return -1;
    return launch_pack_pyr(static_cast<const uint8_t *>(y), pitch_y, static_cast<const uint8_t *>(uv), pitch_uv, w, h, static_cast<uint8_t *>(ring),
                           static_cast<uint8_t *>(dst), dpitch, static_cast<hipStream_t>(stream));
}
// launch_pack_pyr as it stands, for its own refusal: planes pack_pyr_ok refuses are VSTAB_ERR_INVALID before anything touches the device.
__attribute__((visibility("default"))) int vstabx_launch_pack_pyr(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int w, int h, void *ring, void *dst,
                                                                   size_t dpitch, void *stream) {
    return launch_pack_pyr(static_cast<const uint8_t *>(y), pitch_y, static_cast<const uint8_t *>(uv), pitch_uv, w, h, static_cast<uint8_t *>(ring),
                           static_cast<uint8_t *>(dst), dpitch, static_cast<hipStream_t>(stream));
}
// What launch_pyr_down (two_levels = 0; pitch_mid is not looked at) or launch_pyr_down_x2 refuses for planes of these pitches, without a launch and
// without a device (tests/test_pyr_paths_cpu.py): VSTAB_OK, or the launcher's status with its message in vstab_last_error.
__attribute__((visibility("default"))) int vstabx_pyr_down_check(size_t pitch_src, int w, int h, size_t pitch_mid, size_t pitch_dst, int two_levels) {
    return two_levels ? check_pyr_down_x2(pitch_src, w, h, pitch_mid, pitch_dst) : check_pyr_down(pitch_src, w, h, pitch_dst);
}
}  // extern "C"
